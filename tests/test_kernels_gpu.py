"""GPU: every HIP kernel (through the C ABI) against an independent fp64/fp32 torch-CPU
computation of the same op on seeded inputs.  Integer kernels are compared bit-exactly."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ctts_amd  # noqa: F401
from ctts_amd import kernels as K
from ctts_amd import ops
from tests.util import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _assert_restated_mask(mask, p, seed, off):
    """a mask drawn from K.rowscale_dropout(ones) is also the independent model's (tests/glue_restate64.drop_scale over keep_mask)"""
    from tests import glue_restate64 as G
    rows, C = mask.shape
    want = G.drop_scale(int(seed.item()) & 0xFFFFFFFFFFFFFFFF, off, p, rows, C, torch.float32)
    assert torch.equal(mask.float().cpu(), want), "the kernel-drawn dropout mask differs from the restated mask"


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def close(a, b, tol, name=""):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    err = (a - b).abs().max().item()
    ref = max(1.0, b.abs().max().item())
    assert err <= tol * ref, f"{name}: max-abs err {err:.3e} (ref scale {ref:.3e}, tol {tol})"


@pytest.mark.parametrize("M,N,Kd", [(200, 150, 100), (64, 64, 32), (1, 7, 4), (2048, 2048, 64), (130, 129, 260), (300, 11, 256)])
def test_gemm_nt(M, N, Kd):
    A, B = rnd(M, Kd, seed=1), rnd(N, Kd, seed=2)
    C = torch.empty(M, N, device=DEV)
    K.gemm(A.to(DEV), B.to(DEV), C, M, N, Kd, Kd, Kd, N, True, True)
    close(C, A.double() @ B.double().t(), 2e-6 * max(1, Kd / 16), "nt")


@pytest.mark.parametrize("M,N,Kd", [(200, 152, 100), (2048, 1024, 96), (33, 256, 11)])
def test_gemm_nn(M, N, Kd):
    A, B = rnd(M, Kd, seed=3), rnd(Kd, N, seed=4)
    C = torch.empty(M, N, device=DEV)
    K.gemm(A.to(DEV), B.to(DEV), C, M, N, Kd, Kd, N, N, True, False)
    close(C, A.double() @ B.double(), 2e-6 * max(1, Kd / 16), "nn")


@pytest.mark.parametrize("M,N,Kd,split", [(200, 152, 300, 1), (256, 256, 4096, 8), (11, 256, 500, 3), (1024, 2304, 2000, 4)])
def test_gemm_tn_splitk(M, N, Kd, split):
    A, B = rnd(Kd, M, seed=5), rnd(Kd, N, seed=6)   # C = A^T B
    C = torch.zeros(M, N, device=DEV)
    K.gemm(A.to(DEV), B.to(DEV), C, M, N, Kd, M, N, N, False, False, split_k=split, alpha=0.5)
    close(C, 0.5 * (A.double().t() @ B.double()), 3e-6 * max(1, Kd / 16), "tn")


@pytest.mark.parametrize("T,dh,nb", [(64, 32, 3), (200, 32, 2), (1000, 32, 1)])
def test_gemm_padded_view_operands(T, dh, nb):
    """Operands whose base / leading dimension is not a multiple of 4 floats (the relative-attention score slabs viewed as rows of
    T+1, conformer.py:423-431): both contractions of the buffer kernels, batched, against fp64."""
    slab = T * (T + 1)
    g = torch.Generator().manual_seed(12)
    mem = torch.randn(nb, slab, generator=g)
    view = torch.stack([mem[z, 1:1 + (T - 1) * (T + 1) + T].unfold(0, T, T + 1) for z in range(nb)])          # [nb, T, T] rows of T+1 behind 1 float
    assert view.shape == (nb, T, T)
    Bm = torch.randn(T, dh, generator=g)
    Cm = torch.randn(nb, T, dh, generator=g)
    dmem = mem.to(DEV)
    out = torch.empty(nb, T, dh, device=DEV)
    K.gemm(dmem, Bm.to(DEV), out, T, dh, T, T + 1, dh, dh, True, False, a_off=1, nb0=nb, nb1=1, sA=(slab, 0), sC=(T * dh, 0))
    close(out, view.double() @ Bm.double(), 2e-6 * max(1, T / 16), "padded view, K contiguous")
    out2 = torch.empty(nb, T, dh, device=DEV)
    K.gemm(dmem, Cm.to(DEV), out2, T, dh, T, T + 1, dh, dh, False, False, a_off=1, nb0=nb, nb1=1, sA=(slab, 0), sB=(T * dh, 0), sC=(T * dh, 0))
    close(out2, view.double().transpose(1, 2) @ Cm.double(), 2e-6 * max(1, T / 16), "padded view, M contiguous")
    # and as an output: rows of T+1 behind one float
    A2, B2 = torch.randn(nb, T, dh, generator=g), torch.randn(T, dh, generator=g)
    omem = torch.zeros(nb, slab, device=DEV)
    K.gemm(A2.to(DEV), B2.to(DEV), omem, T, T, dh, dh, dh, T + 1, True, True, c_off=1, nb0=nb, nb1=1, sA=(T * dh, 0), sC=(slab, 0))
    got = omem.view(nb, T, T + 1)
    close(got[:, :, 1:], A2.double() @ B2.double().t(), 2e-6 * max(1, dh / 16), "padded output")
    assert float(got[:, :, 0].abs().max()) == 0.0


def test_gemm_epilogue_all():
    M, N, Kd = 150, 200, 64
    A, B, bias, R, rs = rnd(M, Kd, seed=7), rnd(N, Kd, seed=8), rnd(N, seed=9), rnd(M, N, seed=10), (rnd(M, seed=11) > 0).float()
    for act, fn in [(0, lambda v: v), (1, torch.relu), (2, F.gelu), (3, torch.tanh)]:
        C = torch.empty(M, N, device=DEV)
        Z = torch.empty(M, N, device=DEV)
        K.gemm(A.to(DEV), B.to(DEV), C, M, N, Kd, Kd, Kd, N, True, True, alpha=0.3, bias=bias.to(DEV), Z=Z, ldz=N, act=act,
               R=R.to(DEV), ldr=N, rowscale=rs.to(DEV))
        z = 0.3 * (A.double() @ B.double().t() + bias.double())
        close(Z, z, 1e-5, f"Z act{act}")
        close(C, (fn(z) + R.double()) * rs.double()[:, None], 1e-5, f"C act{act}")


def test_gemm_dropout_mask_consistency():
    M, N, Kd, p = 256, 128, 32, 0.3
    A, B = rnd(M, Kd, seed=12), rnd(N, Kd, seed=13)
    drop = K.DropCtx(DEV, seed=5)
    off = drop.next_offset()
    C0 = torch.empty(M, N, device=DEV)
    C1 = torch.empty(M, N, device=DEV)
    K.gemm(A.to(DEV), B.to(DEV), C0, M, N, Kd, Kd, Kd, N, True, True)
    K.gemm(A.to(DEV), B.to(DEV), C1, M, N, Kd, Kd, Kd, N, True, True, p_drop=p, seed=drop.seed, drop_offset=off)
    kept = C1 != 0
    frac = kept.float().mean().item()
    assert abs(frac - (1 - p)) < 0.02, frac
    close(C1[kept], C0[kept] / (1 - p), 1e-5, "kept values scaled")
    # the standalone dropout kernel regenerates the identical mask from (seed, offset, index)
    ones = torch.ones(M, N, device=DEV)
    m2 = K.rowscale_dropout(ones, None, p, drop.seed, off)
    assert torch.equal(m2 != 0, kept)
    drop.advance()
    m3 = K.rowscale_dropout(ones, None, p, drop.seed, off)
    assert not torch.equal(m3 != 0, kept)


@pytest.mark.parametrize("B,T,Cin,Cout,k", [(3, 50, 256, 64, 9), (2, 37, 80, 512, 5), (4, 130, 128, 256, 5), (2, 9, 256, 256, 3)])
def test_conv1d_fwd_bwd(B, T, Cin, Cout, k):
    x, w, b = rnd(B, T, Cin, seed=20), rnd(Cout, Cin, k, seed=21, scale=0.1), rnd(Cout, seed=22)
    xr, wr, br = x.double().requires_grad_(), w.double().requires_grad_(), b.double().requires_grad_()
    yr = F.conv1d(xr.transpose(1, 2), wr, br, padding=k // 2).transpose(1, 2)
    xg, wg, bg = x.to(DEV).requires_grad_(), w.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
    y = ops.conv1d(xg, wg, bg)
    close(y, yr, 1e-5, "conv fwd")
    go = rnd(B, T, Cout, seed=23)
    yr.backward(go.double())
    y.backward(go.to(DEV))
    close(xg.grad, xr.grad, 1e-5, "conv dgrad")
    close(wg.grad, wr.grad, 2e-5, "conv wgrad")
    close(bg.grad, br.grad, 2e-5, "conv bgrad")


def test_linear_fused_fwd_bwd():
    B, T, Cin, Cout = 3, 40, 256, 128
    x, w, b, res = rnd(B, T, Cin, seed=30), rnd(Cout, Cin, seed=31, scale=0.1), rnd(Cout, seed=32), rnd(B, T, Cout, seed=33)
    rs = (rnd(B * T, seed=34) > -0.5).float()
    for act, fn in [(ops.ACT_NONE, lambda v: v), (ops.ACT_GELU, F.gelu), (ops.ACT_RELU, torch.relu)]:
        xr, wr, br, rr = [t.double().requires_grad_() for t in (x, w, b, res)]
        yr = (rr + fn(0.5 * (xr @ wr.t() + br))) * rs.double().view(B, T, 1)
        xg, wg, bg, rg = [t.to(DEV).requires_grad_() for t in (x, w, b, res)]
        y = ops.linear(xg, wg, bg, act=act, alpha=0.5, residual=rg, rowscale=rs.to(DEV))
        close(y, yr, 1e-5, "lin fwd")
        go = rnd(B, T, Cout, seed=35)
        yr.backward(go.double())
        y.backward(go.to(DEV))
        for n, a, r in [("dx", xg.grad, xr.grad), ("dw", wg.grad, wr.grad), ("db", bg.grad, br.grad), ("dres", rg.grad, rr.grad)]:
            close(a, r, 2e-5, f"lin {n} act{act}")


def test_linear_tiny_heads():
    # N = 1, 2, 11 heads (duration / stats / cwt linear layers) incl. their backward (unaligned scalar path)
    for N in (1, 2, 11):
        x, w, b = rnd(5, 33, 256, seed=40), rnd(N, 256, seed=41, scale=0.1), rnd(N, seed=42)
        rs = (rnd(5 * 33, seed=44) > -0.4).float()
        xr, wr, br = [t.double().requires_grad_() for t in (x, w, b)]
        yr = (xr @ wr.t() + br) * rs.double().view(5, 33, 1)
        xg, wg, bg = [t.to(DEV).requires_grad_() for t in (x, w, b)]
        y = ops.linear(xg, wg, bg, rowscale=rs.to(DEV))
        close(y, yr, 1e-5, f"head{N} fwd")
        go = rnd(5, 33, N, seed=43)
        yr.backward(go.double())
        y.backward(go.to(DEV))
        close(xg.grad, xr.grad, 1e-5, f"head{N} dx")
        close(wg.grad, wr.grad, 2e-5, f"head{N} dw")
        close(bg.grad, br.grad, 2e-5, f"head{N} db")


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("B,T,H,C", [(3, 70, 2, 256), (2, 130, 2, 256), (2, 33, 8, 256), (3, 1024, 2, 256), (2, 600, 2, 256), (2, 97, 4, 256)])
def test_self_attention_fwd_bwd(B, T, H, C, fused):
    """fused flash-style kernels (csrc/attn.hip, d_head 128 / 32 / 64) and the unfused GEMM + softmax pipeline, incl. the canonical
    decoder shape T = 1024 with ragged lengths (key tiling, query-loop split with atomic dK / dV, split-K dQ)"""
    ops.set_fused_attention(fused)
    qkv = rnd(B, T, 3 * C, seed=50)
    lens = torch.tensor([T, max(1, T // 2), max(1, T - 7)][:B], dtype=torch.int32)
    dh = C // H
    qr = qkv.double().requires_grad_()
    q, k, v = qr.split(C, dim=-1)
    q = q.reshape(B, T, H, dh).transpose(1, 2) * dh ** -0.5
    k = k.reshape(B, T, H, dh).transpose(1, 2)
    v = v.reshape(B, T, H, dh).transpose(1, 2)
    pad = torch.arange(T)[None, :] >= lens[:, None]
    s = (q @ k.transpose(-1, -2)).masked_fill(pad[:, None, None, :], float("-inf"))
    o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, T, C)
    o = o * (~pad)[..., None]
    qg = qkv.to(DEV).requires_grad_()
    out = ops.self_attention(qg, lens.to(DEV), H)
    close(out, o, 1e-5, "attn fwd")
    go = rnd(B, T, C, seed=51) * (~pad)[..., None]
    o.backward(go.double())
    out.backward(go.to(DEV))
    close(qg.grad, qr.grad, 2e-5, "attn dqkv")
    ops.set_fused_attention(None)


@pytest.mark.parametrize("rows,C,eps", [(100, 256, 1e-12), (37, 128, 1e-5), (64, 1024, 1e-5), (9, 80, 1e-5)])
def test_layernorm_fwd_bwd(rows, C, eps):
    x, g, b = rnd(rows, C, seed=60, scale=2.0), rnd(C, seed=61) + 1.5, rnd(C, seed=62)
    rs = (rnd(rows, seed=63) > -0.3).float()
    xr, gr, br = [t.double().requires_grad_() for t in (x, g, b)]
    yr = F.layer_norm(xr, (C,), gr, br, eps) * rs.double()[:, None]
    xg, gg, bg = [t.to(DEV).requires_grad_() for t in (x, g, b)]
    y = ops.layer_norm(xg, gg, bg, eps, rowscale=rs.to(DEV))
    close(y, yr, 1e-5, "ln fwd")
    go = rnd(rows, C, seed=64)
    yr.backward(go.double())
    y.backward(go.to(DEV))
    close(xg.grad, xr.grad, 2e-5, "ln dx")
    close(gg.grad, gr.grad, 2e-5, "ln dgamma")
    close(bg.grad, br.grad, 2e-5, "ln dbeta")


def test_layernorm_dropout_consistency():
    rows, C, p = 300, 256, 0.5
    x, g, b = rnd(rows, C, seed=65), torch.ones(C), torch.full((C,), 3.0)
    drop = K.DropCtx(DEV)
    xg = x.to(DEV).requires_grad_()
    y = ops.layer_norm(xg, g.to(DEV), b.to(DEV), 1e-5, p_drop=p, drop=drop)
    kept = y != 0
    assert abs(kept.float().mean().item() - 0.5) < 0.02
    y2 = ops.layer_norm(x.to(DEV), g.to(DEV), b.to(DEV), 1e-5)
    close(y[kept], 2 * y2[kept], 1e-5, "ln dropout scale")
    # backward uses the same mask: gradient of sum(y) wrt beta = sum(mask/(1-p)) per channel
    gb = b.to(DEV).requires_grad_()
    drop2 = K.DropCtx(DEV)
    yy = ops.layer_norm(x.to(DEV), g.to(DEV), gb, 1e-5, p_drop=p, drop=drop2)
    yy.sum().backward()
    close(gb.grad, (yy != 0).float().sum(0) * 2, 1e-5, "ln dropout bwd mask")


@pytest.mark.parametrize("act", [ops.ACT_TANH, ops.ACT_NONE])
def test_batchnorm_train_and_eval(act):
    B, T, C = 3, 50, 80
    x, g, b = rnd(B, T, C, seed=70, scale=2.0) + 0.3, rnd(C, seed=71) + 1.5, rnd(C, seed=72)
    bn = torch.nn.BatchNorm1d(C).double()
    with torch.no_grad():
        bn.weight.copy_(g); bn.bias.copy_(b)
    xr = x.double().requires_grad_()
    yr = bn(xr.transpose(1, 2)).transpose(1, 2)
    if act == ops.ACT_TANH:
        yr = torch.tanh(yr)
    rm, rv, nbt = torch.zeros(C, device=DEV), torch.ones(C, device=DEV), torch.tensor(0, device=DEV)
    xg, gg, bg = x.to(DEV).requires_grad_(), g.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
    y = ops.batch_norm_act(xg, gg, bg, rm, rv, nbt, True, act=act)
    close(y, yr, 1e-5, "bn fwd")
    close(rm, bn.running_mean, 1e-5, "running_mean")
    close(rv, bn.running_var, 1e-5, "running_var")
    go = rnd(B, T, C, seed=73)
    yr.backward(go.double())
    y.backward(go.to(DEV))
    close(xg.grad, xr.grad, 2e-5, "bn dx")
    close(gg.grad, bn.weight.grad, 2e-5, "bn dgamma")
    close(bg.grad, bn.bias.grad, 2e-5, "bn dbeta")
    bn.eval()
    ye = bn(x.double().transpose(1, 2)).transpose(1, 2)
    if act == ops.ACT_TANH:
        ye = torch.tanh(ye)
    y2 = ops.batch_norm_act(x.to(DEV), g.to(DEV), b.to(DEV), rm, rv, nbt, False, act=act)
    close(y2, ye, 1e-5, "bn eval")


def test_length_regulator_bit_exact_vs_reference_golden():
    g = load_golden("g7_integer")
    d, x = torch.from_numpy(g["lr.dur"]).to(DEV), torch.from_numpy(g["lr.x"]).to(DEV)
    for tag, max_len in (("none", None), ("crop", 50), ("pad", 200)):
        out, mel_len, mel2ph = ops.length_regulate(x, d, max_len)
        assert np.array_equal(out.cpu().numpy(), g[f"lr.{tag}.out"]), tag
        assert np.array_equal(mel_len.cpu().numpy(), g[f"lr.{tag}.mel_len"]), tag
        assert np.array_equal(mel2ph.cpu().numpy().astype(np.int64) - 1, g[f"lr.{tag}.idx"]), tag
    outf, mlf, _ = ops.length_regulate(torch.from_numpy(g["lrf.x"]).to(DEV), torch.from_numpy(g["lrf.dur"]).to(DEV), None)
    assert np.array_equal(outf.cpu().numpy(), g["lrf.out"]) and np.array_equal(mlf.cpu().numpy(), g["lrf.mel_len"])
    pad = torch.from_numpy(g["m2p.pad"]).to(DEV)
    assert np.array_equal(ops.dur_to_mel2ph(d, pad).cpu().numpy(), g["m2p.out"])
    assert np.array_equal(ops.dur_to_mel2ph(d, None).cpu().numpy(), g["m2p.out_nopad"])
    tok = torch.from_numpy(g["pos.in"]).to(DEV)
    assert np.array_equal(K.positions(tok, 1).cpu().numpy(), g["pos.out"])
    xf = torch.from_numpy(g["pos.in"]).float().to(DEV)[..., None].repeat(1, 1, 4).contiguous()
    assert np.array_equal(K.positions(xf, 4).cpu().numpy(), g["pos.out"])


def test_length_regulator_backward_and_roundtrip():
    B, Ts, C = 4, 37, 256
    g = torch.Generator().manual_seed(5)
    d = torch.randint(0, 7, (B, Ts), generator=g)
    x = rnd(B, Ts, C, seed=80)
    xg = x.to(DEV).requires_grad_()
    out, mel_len, mel2ph = ops.length_regulate(xg, d.to(DEV), 150)
    go = rnd(B, 150, C, seed=81)
    out.backward(go.to(DEV))
    ref = torch.zeros(B, Ts, C, dtype=torch.float64)
    m2p = mel2ph.cpu().long()
    for b in range(B):
        for t in range(150):
            if m2p[b, t] > 0:
                ref[b, m2p[b, t] - 1] += go[b, t].double()
    close(xg.grad, ref, 1e-6, "lr bwd")
    # size-independent property: frame counts per phoneme reproduce the (cropped) durations
    counts = torch.zeros(B, Ts + 1, dtype=torch.long).scatter_add(1, m2p, torch.ones_like(m2p))[:, 1:]
    cum = torch.cumsum(d, 1)
    expect = (cum.clamp(max=150) - (cum - d).clamp(max=150))
    assert torch.equal(counts, expect)


def _fp64_mel(y, n_fft=1024, hop=256, clip=1e-5):
    """float64 restatement of TacotronSTFT.mel_spectrogram (reflect pad, periodic hann, rFFT, |X|, Slaney mel, log clamp)"""
    from ctts_amd.audio import slaney_mel_basis
    y = y.double().numpy()
    pad = np.pad(y, ((0, 0), (n_fft // 2, n_fft // 2)), mode="reflect")
    F = 1 + y.shape[1] // hop
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)
    frames = np.stack([pad[:, f * hop:f * hop + n_fft] for f in range(F)], 1) * win
    mag = np.abs(np.fft.rfft(frames, axis=-1))                                   # [B,F,513]
    basis = slaney_mel_basis(22050, n_fft, 80, 0, 8000).astype(np.float64)
    mel = np.log(np.maximum(mag @ basis.T, clip)).transpose(0, 2, 1)             # [B,80,F]
    return torch.from_numpy(mag.transpose(0, 2, 1)), torch.from_numpy(mel), torch.from_numpy(np.sqrt((mag ** 2).sum(-1)))


@pytest.mark.parametrize("path", ["fft", "dft_gemm"])
def test_mel_spectrogram_vs_reference_golden(path):
    """TacotronSTFT.mel_spectrogram: the one-launch real-FFT kernel (csrc/mel.hip) and the DFT-as-GEMM path against the reference's own
    output (G8) AND against a float64 FFT of the same waveform.  The log amplifies fp32 noise of near-silent bins (a pure-tone row
    leaks ~1e-6), so the reference itself is ~1e-2 away from the float64 truth there: the all-bin log-mel error is reported for both
    and ours must not be farther from the truth than the reference's own conv1d arithmetic is."""
    g = load_golden("g8_stft")
    st = ctts_amd.TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000).to(DEV)
    st.use_fft = path == "fft"
    close(st.mel_basis, torch.from_numpy(g["mel_basis"]), 1e-6, "mel basis (librosa 0.7.2 restated)")
    y = torch.from_numpy(g["y"]).to(DEV)
    mel, energy = st.mel_spectrogram(y)
    mag = st.magnitudes(y)
    assert mel.shape == g["mel"].shape and energy.shape == g["energy"].shape
    close(mag, torch.from_numpy(g["mag"]), 2e-5, "magnitude")
    close(energy, torch.from_numpy(g["energy"]), 2e-5, "energy")
    ref = torch.from_numpy(g["mel"])
    loud = ref.exp() > 1e-3
    err = (mel.cpu() - ref)[loud].abs().max().item()
    assert err < 1e-3, f"log-mel max-abs {err} on bins above 1e-3"
    lin = (mel.cpu().exp() - ref.exp()).abs().max().item() / ref.exp().max().item()
    assert lin < 1e-5, f"linear mel relative-to-full-scale error {lin}"
    mag64, mel64, en64 = _fp64_mel(torch.from_numpy(g["y"]))
    all_ours = (mel.cpu().double() - mel64).abs().max().item()
    all_ref = (ref.double() - mel64).abs().max().item()
    all_vs_ref = (mel.cpu() - ref).abs().max().item()
    mag_ours = (mag.cpu().double() - mag64).abs().max().item()
    mag_ref = (torch.from_numpy(g["mag"]).double() - mag64).abs().max().item()
    print(f"[{path}] log-mel max-abs: loud bins vs reference {err:.2e}; ALL bins vs reference {all_vs_ref:.2e}; ALL bins vs float64 truth: "
          f"ours {all_ours:.2e}, reference {all_ref:.2e}; |X| vs float64: ours {mag_ours:.2e}, reference {mag_ref:.2e}; "
          f"linear mel rel err {lin:.2e}; loud fraction {loud.float().mean():.2f}")
    assert all_ours <= max(1.5 * all_ref, 1e-4), (all_ours, all_ref)
    assert mag_ours <= max(1.5 * mag_ref, 2e-5), (mag_ours, mag_ref)
    # the all-bin number, asserted: 4e-3 in the log domain over ALL 80 x F bins against the reference's own output (measured 2.4e-3 FFT /
    # 3.0e-3 DFT-GEMM; the reference itself is 1.75e-3 from the float64 truth on this waveform - near-silent bins, where exp(mel) ~ 1e-5,
    # carry all of it; INTEGRATION.md section 5 states this bound next to the 1e-3 loud-bin bound)
    assert all_vs_ref <= 4e-3, all_vs_ref


def test_mel_spectrogram_range_assert_strict_by_default_deferred_on_request():
    """audio/stft.py:177-178 asserts min(y) >= -1 and max(y) <= 1 before computing.  The FFT kernel raises a flag in pinned host memory
    instead of two reductions.  Default (strict_range): the SAME call raises AssertionError for an out-of-range or NaN waveform - also
    when it is the only or the last call.  strict_range = False (training hot path): no wait; the assertion arrives at
    check_range(), or at the next call once the flag has landed.  A valid waveform raises nothing either way."""
    st = ctts_amd.TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000).to(DEV)
    y = (torch.rand(2, 8192, generator=torch.Generator().manual_seed(3)) - 0.5).to(DEV)
    bad = y.clone(); bad[1, 4000] = 1.5
    nan = y.clone(); nan[0, 100] = float("nan")
    assert st.strict_range
    st.mel_spectrogram(y)                              # valid input: silent
    with pytest.raises(AssertionError, match="outside"):
        st.mel_spectrogram(bad)                        # raised by the offending call itself
    st.mel_spectrogram(y)                              # flag was cleared
    with pytest.raises(AssertionError):
        st.mel_spectrogram(nan)
    st.mel_spectrogram(y)
    st.strict_range = False
    st.mel_spectrogram(y)
    st.check_range()                                   # valid input: silent
    st.mel_spectrogram(bad)                            # launch succeeds (no sync) ...
    with pytest.raises(AssertionError, match="outside"):
        st.check_range()                               # ... the assertion arrives here
    st.mel_spectrogram(y); st.check_range()            # flag was cleared
    st.mel_spectrogram(nan)
    torch.cuda.synchronize()
    with pytest.raises(AssertionError):
        st.mel_spectrogram(y)                          # the NEXT call notices the earlier one without waiting for anything new


@pytest.mark.parametrize("B,N", [(1, 700), (3, 4096 + 37), (2, 22050), (1, 256 * 40)])
def test_mel_fft_kernel_vs_float64_ragged_lengths(B, N):
    """frame counts that are not multiples of the 16-frame tile, odd sample counts (unaligned pair loads), clips shorter than two FFT
    windows (every frame touches the reflect padding)"""
    st = ctts_amd.TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000).to(DEV)
    y = rnd(B, N, seed=300) * 0.9
    mel, energy = st.mel_spectrogram(y.to(DEV))
    mag = st.magnitudes(y.to(DEV))
    mag64, mel64, en64 = _fp64_mel(y)
    assert mel.shape == mel64.shape == (B, 80, 1 + N // 256)
    close(mag, mag64, 2e-5, "mag vs fp64")
    close(energy, en64, 2e-5, "energy vs fp64")
    lin = (mel.cpu().double().exp() - mel64.exp()).abs().max().item() / mel64.exp().max().item()
    assert lin < 2e-5, lin
    st.use_fft = False
    mel2, energy2 = st.mel_spectrogram(y.to(DEV))
    close(mel.exp(), mel2.exp(), 2e-5, "fft vs dft-gemm path")
    close(energy, energy2, 2e-5, "fft vs dft-gemm energy")


def test_batched_ragged_mel_extraction_equals_per_utterance_calls():
    """preprocessing path: one launch over a ragged batch == the reference's one-utterance-at-a-time get_mel_from_wav"""
    from ctts_amd.audio import get_mel_from_wav
    st = ctts_amd.TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000).to(DEV)
    rng = np.random.RandomState(3)
    wavs = [rng.uniform(-1.2, 1.2, size=n).astype(np.float32) for n in (22050, 700, 9001, 4096, 30001)]     # incl. values to clip
    batched = st.mel_spectrograms_ragged(wavs)
    for w, (mel, en) in zip(wavs, batched):
        y = torch.from_numpy(np.clip(w, -1, 1))[None].to(DEV)
        m1, e1 = st.mel_spectrogram(y)
        assert mel.shape == (80, 1 + len(w) // 256) and en.shape == (1 + len(w) // 256,) and mel.dtype == np.float32
        close(torch.from_numpy(mel).exp(), m1[0].exp(), 1e-6, "ragged batch vs single utterance (linear mel)")
        close(torch.from_numpy(en), e1[0], 1e-6, "ragged batch vs single utterance (energy)")
        m2, e2 = get_mel_from_wav(w, st)
        assert np.array_equal(m2, mel) and np.array_equal(e2, en)


def test_pad_row_skipping_is_equivalent_on_valid_rows():
    """Padded-row tile / K-block skipping (ctts_gemm_desc.row_lens) changes nothing that the model consumes:
    valid rows of the forward, and every gradient when the upstream gradient is zero on padded rows."""
    B, T, C = 3, 384, 256
    lens = torch.tensor([384, 100, 200], dtype=torch.int32)
    valid = (torch.arange(T)[None, :] < lens[:, None])
    rs = valid.float().reshape(-1)
    x = rnd(B, T, C, seed=90)
    for kind in ("linear", "conv"):
        w = rnd(512, C, 9, seed=91, scale=0.05) if kind == "conv" else rnd(512, C, seed=91, scale=0.05)
        b = rnd(512, seed=92)
        go = rnd(B, T, 512, seed=93) * valid[..., None]
        res = []
        for pr in (None, (lens.to(DEV), T)):
            xg, wg, bg = x.to(DEV).requires_grad_(), w.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
            fn = ops.conv1d if kind == "conv" else ops.linear
            y = fn(xg, wg, bg, act=ops.ACT_GELU, alpha=0.7, pad_rows=pr)
            y.backward(go.to(DEV))
            res.append((y.detach(), xg.grad, wg.grad, bg.grad))
        (y0, dx0, dw0, db0), (y1, dx1, dw1, db1) = res
        close(y1[valid], y0[valid], 1e-6, f"{kind} fwd valid rows")
        assert float(y1[2, 256:].abs().max()) == 0.0          # fully padded tile was zero-filled, not computed
        close(dx1, dx0, 1e-6, f"{kind} dx")
        close(dw1, dw0, 2e-5, f"{kind} dw")
        close(db1, db0, 1e-5, f"{kind} db")


def test_swish_linear_glu_depthwise_fwd_bwd():
    B, T, C = 3, 45, 256
    x, w, b = rnd(B, T, C, seed=100), rnd(128, C, seed=101, scale=0.1), rnd(128, seed=102)
    xr, wr, br = [t.double().requires_grad_() for t in (x, w, b)]
    z = xr @ wr.t() + br
    yr = z * torch.sigmoid(z)
    xg, wg, bg = [t.to(DEV).requires_grad_() for t in (x, w, b)]
    y = ops.linear(xg, wg, bg, act=ops.ACT_SWISH)
    close(y, yr, 1e-5, "swish fwd")
    go = rnd(B, T, 128, seed=103)
    yr.backward(go.double()); y.backward(go.to(DEV))
    close(xg.grad, xr.grad, 2e-5, "swish dx"); close(wg.grad, wr.grad, 2e-5, "swish dw")
    # GLU
    a = rnd(B, T, 2 * C, seed=104)
    ar = a.double().requires_grad_()
    gr = ar[..., :C] * torch.sigmoid(ar[..., C:])
    ag = a.to(DEV).requires_grad_()
    g = ops.glu(ag)
    close(g, gr, 1e-5, "glu fwd")
    go = rnd(B, T, C, seed=105)
    gr.backward(go.double()); g.backward(go.to(DEV))
    close(ag.grad, ar.grad, 2e-5, "glu bwd")
    # depthwise conv k=31 (and a short sequence, T < k)
    for (Bq, Tq) in ((3, 45), (2, 9), (2, 130)):
        xx, ww = rnd(Bq, Tq, C, seed=106), rnd(C, 1, 31, seed=107, scale=0.2)
        xr, wr = xx.double().requires_grad_(), ww.double().requires_grad_()
        yr = F.conv1d(xr.transpose(1, 2), wr, None, padding=15, groups=C).transpose(1, 2)
        xg, wg = xx.to(DEV).requires_grad_(), ww.to(DEV).requires_grad_()
        y = ops.depthwise_conv1d(xg, wg)
        close(y, yr, 1e-5, "dwconv fwd")
        go = rnd(Bq, Tq, C, seed=108)
        yr.backward(go.double()); y.backward(go.to(DEV))
        close(xg.grad, xr.grad, 2e-5, "dwconv dx"); close(wg.grad, wr.grad, 3e-5, "dwconv dw")


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("B,T,H,C", [(2, 36, 8, 256), (2, 51, 8, 256), (1, 132, 4, 128), (2, 200, 8, 256), (1, 64, 2, 256), (2, 9, 8, 256),
                                     (2, 1, 8, 256), (1, 33, 4, 256), (1, 1000, 8, 256)])
def test_relpos_attention_fwd_bwd(B, T, H, C, fused):
    """(1, 1000, 8, 256) is the conformer decoder's full length: the fused backward's 63-wide Toeplitz band, the lane rotation and the
    padded dS slab against an independent float64 reference (not only against the unfused pipeline)."""
    ops.set_fused_attention(fused)
    dh = C // H
    qu, qv, kv, pos = rnd(B, T, C, seed=110), rnd(B, T, C, seed=111), rnd(B, T, 2 * C, seed=112), rnd(T, C, seed=113)
    scale = 1.0 / C ** 0.5 * 4

    def ref(qu, qv, kv, pos):
        q1 = qu.view(B, T, H, dh).transpose(1, 2)
        q2 = qv.view(B, T, H, dh).transpose(1, 2)
        k = kv[..., :C].reshape(B, T, H, dh).permute(0, 2, 1, 3)
        v = kv[..., C:].reshape(B, T, H, dh).permute(0, 2, 1, 3)
        p = pos.view(T, H, dh).permute(1, 2, 0)[None]
        content = q1 @ k.transpose(2, 3)
        ps = q2 @ p
        padded = torch.cat([ps.new_zeros(B, H, T, 1), ps], dim=-1).view(B, H, T + 1, T)
        shifted = padded[:, :, 1:].reshape(B, H, T, T)
        attn = torch.softmax((content + shifted) * scale, -1)
        return (attn @ v).transpose(1, 2).reshape(B, T, C)
    tr = [t.double().requires_grad_() for t in (qu, qv, kv, pos)]
    tg = [t.to(DEV).requires_grad_() for t in (qu, qv, kv, pos)]
    yr = ref(*tr)
    y = ops.relpos_attention(*tg, H, scale)
    close(y, yr, 1e-5, "relpos fwd")
    go = rnd(B, T, C, seed=114)
    yr.backward(go.double()); y.backward(go.to(DEV))
    for n, a, r in zip(("dqu", "dqv", "dkv", "dpos"), tg, tr):
        close(a.grad, r.grad, 3e-5, "relpos " + n)
    ops.set_fused_attention(None)


def _sk_error_word():
    ws = K.gemm_workspace(torch.device(DEV))
    return int(ws.view(torch.int32)[2048].item())


@pytest.mark.parametrize("case", ["conv_fwd_ragged_epilogue", "conv_dgrad_halo", "conv_fwd_dense_128", "wgrad_tn_accumulate", "nn_dense"])
def test_persistent_stream_k_gemm_equals_tile_kernels(case):
    """csrc/gemm_sk.hip (persistent grid, direct-to-LDS operands, tiles cut between workgroups and summed in a fixed order) against the
    tile-per-workgroup kernels of csrc/gemm.hip on the same descriptor: conv views with time-boundary taps, padded-row schedules with
    halo, fused epilogue (bias + GELU + dropout + pre-activation store), 128x128 and 64x128 tiles, K-block schedule of the weight
    gradient with accumulation into an existing buffer.  The descriptor must really take the persistent path (asserted)."""
    torch.manual_seed(11)
    B, T = 16, 512
    M = B * T
    lens = torch.tensor([512, 490, 77, 300, 512, 64, 1, 257, 400, 333, 128, 129, 500, 20, 256, 384], dtype=torch.int32, device=DEV)
    if case == "conv_fwd_ragged_epilogue":
        x = torch.randn(B, T, 256, device=DEV); w = torch.randn(512, 2304, device=DEV) * 0.03
        bias = torch.randn(512, device=DEV); seed = torch.zeros(1, dtype=torch.int64, device=DEV)
        outs = [torch.empty(B, T, 512, device=DEV), torch.empty(B, T, 512, device=DEV)]
        args = (x, w, outs[0], M, 512, 2304, 256, 2304, 512, True, True)
        kw = dict(conv=(T, 4, 256), alpha=1 / 3, bias=bias, Z=outs[1], ldz=512, act=K.ACT_GELU, p_drop=0.1, seed=seed, drop_offset=3,
                  row_lens=lens, row_T=T, row_halo=0, tile_map=K.row_tile_map(lens, T, 0, M))
    elif case == "conv_dgrad_halo":
        dz = torch.randn(M, 512, device=DEV); wd = torch.randn(512, 4608, device=DEV) * 0.03
        outs = [torch.empty(B, T, 512, device=DEV)]
        args = (dz, wd, outs[0], M, 512, 4608, 512, 4608, 512, True, True)
        kw = dict(conv=(T, 4, 512), alpha=0.5, row_lens=lens, row_T=T, row_halo=4, tile_map=K.row_tile_map(lens, T, 4, M))
    elif case == "conv_fwd_dense_128":
        x = torch.randn(B, T, 512, device=DEV); w = torch.randn(512, 2560, device=DEV) * 0.03
        outs = [torch.empty(B, T, 512, device=DEV)]
        args = (x, w, outs[0], M, 512, 2560, 512, 2560, 512, True, True)
        kw = dict(conv=(T, 2, 512))
    elif case == "wgrad_tn_accumulate":
        rowmask = (torch.arange(T, device=DEV)[None, :] < lens[:, None]).reshape(M, 1).float()
        dz = torch.randn(M, 2048, device=DEV) * rowmask; x = torch.randn(B, T, 256, device=DEV)
        outs = [torch.zeros(2048, 2304, device=DEV)]
        args = (dz, x, outs[0], 2048, 2304, M, 2048, 256, 2304, False, False)
        kw = dict(conv=(T, 4, 256), conv_on_b=True, split_k=4, alpha=0.25, row_lens=lens, row_T=T, tile_map=K.row_tile_map(lens, T, 0, M))
    else:
        a = torch.randn(M, 2048, device=DEV); w = torch.randn(2048, 1024, device=DEV) * 0.03
        outs = [torch.empty(M, 1024, device=DEV)]
        args = (a, w, outs[0], M, 1024, 2048, 2048, 1024, 1024, True, False)
        kw = {}
    assert K.gemm_takes_persistent(*args, **kw), "the descriptor is expected to take the persistent path"
    res = []
    for use_sk in (False, True):
        for o in outs:
            o.fill_(0.5 if case == "wgrad_tn_accumulate" else float("nan"))      # accumulate: onto an existing value; else: every element written
        K.gemm(*args, use_sk=use_sk, **kw)
        torch.cuda.synchronize()
        res.append([o.clone() for o in outs])
    assert _sk_error_word() == 0
    for u, v in zip(res[0], res[1]):
        assert torch.isfinite(v).all()
        close(v, u, 3e-6 if case != "wgrad_tn_accumulate" else 2e-5, "stream-K vs tiles " + case)


def test_dominant_stream_k_kernel_vs_fp64_at_the_bench_shape():
    """the kernel bench.py's roofline block times - gemm_sk_kernel<NT layout, conv, 64 x 256 tiles> on the decoder FFN
    Conv1d k = 9 at its train-step arguments: M = 16,384 rows (B = 16, T = 1024, canonical ragged lengths, device-built tile schedule),
    N = 1024, K = 2304, bias + GELU + dropout epilogue with pre-activation store - DIRECTLY against float64 (it was only compared with
    the tile kernels at N = 512, a self-comparison).  The float64 reference is computed for a sample of rows spread over every
    utterance (first / last valid rows, tile edges, the conv's time boundary) and ALL 1024 columns; padded rows must be exactly zero."""
    from ctts_amd.synthetic import CANONICAL_SRC_LENS
    B, T, Cin, N, ks = 16, 1024, 256, 1024, 9
    M, Kd, pad = B * T, ks * Cin, 4
    lens_l = [8 * n for n in CANONICAL_SRC_LENS]
    lens = torch.tensor(lens_l, dtype=torch.int32, device=DEV)
    g = torch.Generator().manual_seed(77)
    x = (torch.rand(B, T, Cin, generator=g) - 0.5).to(DEV)
    w = ((torch.rand(N, Kd, generator=g) - 0.5) * 0.1).to(DEV)               # GEMM-major conv weight [Cout][k][Cin]
    bias = (torch.rand(N, generator=g) - 0.5).to(DEV)
    seed = torch.full((1,), 99, dtype=torch.int64, device=DEV)
    p, off, alpha = 0.1, 5, 1.0
    out = torch.full((B, T, N), float("nan"), device=DEV)
    Z = torch.full((B, T, N), float("nan"), device=DEV)
    args = (x, w, out, M, N, Kd, Cin, Kd, N, True, True)
    kw = dict(conv=(T, pad, Cin), alpha=alpha, bias=bias, Z=Z, ldz=N, act=K.ACT_GELU, p_drop=p, seed=seed, drop_offset=off,
              row_lens=lens, row_T=T, row_halo=0, tile_map=K.row_tile_map(lens, T, 0, M))
    assert K.gemm_takes_bf16_split(*args, **kw) or K.gemm_takes_persistent(*args, **kw), "expected on the bf16-split or the stream-K kernel"
    K.gemm(*args, **kw)
    torch.cuda.synchronize()
    assert _sk_error_word() == 0
    mask = K.rowscale_dropout(torch.ones(M, N, device=DEV), None, p, seed, off).view(B, T, N)        # 0 or 1/(1-p), from (seed, offset, m*N+n)
    _assert_restated_mask(mask.view(M, N), p, seed, off)
    xd, wd = x.double().cpu(), w.double().cpu().view(N, ks, Cin)
    worst_c = worst_z = 0.0
    for b in range(B):
        L = lens_l[b]
        rows = sorted({0, 1, 3, 4, 5, 63, 64, 65, L // 2, L - 65, L - 5, L - 4, L - 1} & set(range(L)))
        for t in rows:
            acc = torch.zeros(N, dtype=torch.float64)
            for kk in range(ks):
                tt = t - pad + kk
                if 0 <= tt < T:                                  # the conv pads with zeros at the utterance tensor's edges
                    acc += wd[:, kk, :] @ xd[b, tt]
            z = alpha * (acc + bias.double().cpu())
            ref = F.gelu(z) * mask[b, t].double().cpu()
            worst_z = max(worst_z, float((Z[b, t].double().cpu() - z).abs().max()))
            worst_c = max(worst_c, float((out[b, t].double().cpu() - ref).abs().max()))
        tail0 = (L + 63) // 64 * 64                              # rows of wholly padded 64-row tiles are defined as zero
        if tail0 < T:
            assert float(out[b, tail0:].abs().max()) == 0.0 and float(Z[b, tail0:].abs().max()) == 0.0
    assert torch.isfinite(out).all() and torch.isfinite(Z).all()
    print(f"stream-K 64x256 conv fwd vs fp64: pre-activation {worst_z:.2e}, output {worst_c:.2e}")
    assert worst_z <= 2e-5 and worst_c <= 2e-5, (worst_z, worst_c)


@pytest.mark.parametrize("ksize,act", [(9, "gelu"), (0, "swish")])
def test_epilogue_backward_in_the_consumer_gemm_equals_the_separate_pass(ksize, act):
    """ops.EpiLink: producer (Conv1d k=9 + GELU + dropout, or Linear + Swish + dropout) -> consumer Linear.  With the link the consumer's
    data-gradient GEMM applies mask / (1-p) * act'(Z) in its epilogue (ctts_gemm_desc.epi_bwd) and the producer skips epilogue_bwd;
    same dropout masks (same seed and call-site offsets) -> all gradients equal the unlinked run's, ragged rows included."""
    B, T, C, Hd, p = 3, 70, 64, 256, 0.2
    a = K.ACT_GELU if act == "gelu" else K.ACT_SWISH
    x0 = rnd(B, T, C, seed=150)
    w1 = rnd(Hd, C, ksize, seed=151, scale=0.2) if ksize else rnd(Hd, C, seed=151, scale=0.2)
    b1, w2, b2 = rnd(Hd, seed=152), rnd(C, Hd, seed=153, scale=0.2), rnd(C, seed=154)
    lens = torch.tensor([70, 33, 51], dtype=torch.int32, device=DEV)
    nonpad = (torch.arange(T, device=DEV)[None, :] < lens[:, None]).float().reshape(-1).contiguous()
    go = rnd(B, T, C, seed=155).to(DEV) * nonpad.view(B, T, 1)
    res = []
    for linked in (False, True):
        drop = K.DropCtx(DEV, seed=5)
        ts = [t.to(DEV).requires_grad_() for t in (x0, w1, b1, w2, b2)]
        pr = ops.PadRows(lens, T)
        link = ops.EpiLink() if linked else None
        f1 = ops.conv1d if ksize else ops.linear
        h = f1(ts[0], ts[1], ts[2], act=a, alpha=0.5, p_drop=p, drop=drop, pad_rows=pr, link=link, link_role=1)
        y = ops.linear(h, ts[3], ts[4], residual=ts[0], rowscale=nonpad, p_drop=p, drop=drop, pad_rows=pr, link=link, link_role=2)
        y.backward(go)
        if linked:
            assert not link.armed and not link.done          # taken by the consumer's forward, delivered dZ consumed by the producer's backward
            # a link object reused by a SECOND forward before the first backward: each backward uses the snapshot of its own
            # forward, so both passes still reproduce the unlinked gradients
            drop2 = K.DropCtx(DEV, seed=5)
            ts2 = [t.to(DEV).requires_grad_() for t in (x0, w1, b1, w2, b2)]
            ha = f1(ts2[0], ts2[1], ts2[2], act=a, alpha=0.5, p_drop=p, drop=drop2, pad_rows=pr, link=link, link_role=1)
            ya = ops.linear(ha, ts2[3], ts2[4], residual=ts2[0], rowscale=nonpad, p_drop=p, drop=drop2, pad_rows=pr, link=link, link_role=2)
            hb = f1(ts2[0], ts2[1], ts2[2], act=a, alpha=0.5, p_drop=0.5, drop=drop2, pad_rows=pr, link=link, link_role=1)     # re-arms the link
            yb = ops.linear(hb, ts2[3], ts2[4], residual=ts2[0], rowscale=nonpad, p_drop=p, drop=drop2, pad_rows=pr, link=link, link_role=2)
            ya.backward(go)
            for n, u, v in zip(("dx", "dw1", "db1", "dw2", "db2"), res[0][1:], [t.grad for t in ts2]):
                close(v, u, 2e-5, "EpiLink reused link, first pass " + n)
            del yb
        res.append([y.detach()] + [t.grad for t in ts])
    for n, u, v in zip(("y", "dx", "dw1", "db1", "dw2", "db2"), res[0], res[1]):
        close(v, u, 2e-5, "EpiLink " + n)


def test_relattn_split_fwd_bwd():
    """q + u_bias, q + v_bias, k | v from the packed projection (conformer.py:396-407) and the adjoint, against autograd."""
    B, T, H, C = 2, 37, 8, 256
    qkv, u, v = rnd(B, T, 3 * C, seed=140), rnd(H, C // H, seed=141), rnd(H, C // H, seed=142)
    gs = [rnd(B, T, C, seed=143), rnd(B, T, C, seed=144), rnd(B, T, 2 * C, seed=145)]
    tr = [t.double().requires_grad_() for t in (qkv, u, v)]
    outs_r = (tr[0][..., :C] + tr[1].reshape(1, 1, C), tr[0][..., :C] + tr[2].reshape(1, 1, C), tr[0][..., C:])
    torch.autograd.backward(outs_r, [g.double() for g in gs])
    tg = [t.to(DEV).requires_grad_() for t in (qkv, u, v)]
    outs = ops.relattn_split(*tg)
    for n, a, r in zip(("qu", "qv", "kv"), outs, outs_r):
        close(a, r, 1e-6, "relattn_split " + n)
    torch.autograd.backward(outs, [g.to(DEV) for g in gs])
    for n, a, r in zip(("dqkv", "du", "dv"), tg, tr):
        close(a.grad, r.grad, 2e-5, "relattn_split " + n)


@pytest.mark.parametrize("B,T,p", [(2, 77, 0.3), (1, 1000, 0.1)])
def test_fused_relpos_attention_equals_unfused_incl_dropout(B, T, p):
    """Same counter-RNG element indices in both paths -> identical dropout masks: outputs and all four gradients of the fused kernels
    against the unfused GEMM / softmax / shift pipeline, at a ragged T and at the conformer decoder's full length T = 1000."""
    H, C = 8, 256
    ts = [rnd(B, T, C, seed=130), rnd(B, T, C, seed=131), rnd(B, T, 2 * C, seed=132), rnd(T, C, seed=133)]
    go = rnd(B, T, C, seed=134).to(DEV)
    res = []
    for fused in (False, True):
        ops.set_fused_attention(fused)
        drop = K.DropCtx(DEV, seed=77)
        tg = [t.to(DEV).requires_grad_() for t in ts]
        y = ops.relpos_attention(*tg, H, 1.0 / 16, p_drop=p, drop=drop)
        y.backward(go)
        res.append([y.detach()] + [t.grad for t in tg])
    ops.set_fused_attention(None)
    for n, a, b in zip(("out", "dqu", "dqv", "dkv", "dpos"), res[0], res[1]):
        close(b, a, 2e-5, "fused vs unfused relpos " + n)


def test_relpos_attention_dropout_consistency():
    B, T, H, C, p = 2, 64, 8, 256, 0.3
    qu, qv, kv, pos = [t.to(DEV) for t in (rnd(B, T, C, seed=120), rnd(B, T, C, seed=121), rnd(B, T, 2 * C, seed=122), rnd(T, C, seed=123))]
    kv = kv.clone()
    kv[..., C:] = 1.0                                  # V = 1  ->  context = sum_j dropped probs = kept mass / (1-p)
    drop = K.DropCtx(DEV)
    kvg = kv.requires_grad_()
    y = ops.relpos_attention(qu, qv, kvg, pos, H, 0.1, p_drop=p, drop=drop)
    mass = y.detach()[..., 0]
    assert abs(mass.mean().item() - 1.0) < 0.05 and mass.std().item() > 0.01
    # backward regenerates the same mask: d/dV of sum(y) is the column sum of the dropped probabilities = same kept mass
    y.sum().backward()
    tot = kvg.grad[..., C:].sum().item()
    assert abs(tot - y.detach().sum().item()) < 1e-2 * abs(tot)


# ---- liu2021 prosody kernels (csrc/prosody.hip) ---------------------------------------------------------------------
@pytest.mark.parametrize("B,T,W,Cin,Cout", [(2, 13, 80, 4, 32), (3, 7, 5, 64, 128), (1, 9, 3, 128, 128), (2, 6, 40, 32, 32)])
def test_conv2d_3x3s2_fwd_bwd(B, T, W, Cin, Cout):
    """Conv2d 3x3 stride (1,2) pad (1,1): patch matrix + ctts_gemm + col2im against F.conv2d (fp64 CPU)."""
    x = rnd(B, T, W, Cin, seed=1).requires_grad_(True)
    w = rnd(Cout, Cin, 3, 3, seed=2, scale=0.2).requires_grad_(True)
    b = rnd(Cout, seed=3).requires_grad_(True)
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), stride=(1, 2), padding=(1, 1)).permute(0, 2, 3, 1)
    gy = rnd(*ref.shape, seed=4)
    ref.backward(gy.double())
    xd, wd, bd = [t.detach().to(DEV).requires_grad_(True) for t in (x, w, b)]
    y = ops.conv2d_3x3s2(xd, wd, bd)
    assert y.shape == ref.shape
    close(y, ref, 2e-5, "conv2d fwd")
    y.backward(gy.to(DEV))
    close(xd.grad, x.grad, 2e-5, "conv2d dx")
    close(wd.grad, w.grad, 2e-5, "conv2d dw")
    close(bd.grad, b.grad, 2e-5, "conv2d db")


@pytest.mark.parametrize("B,T,In,H,bi", [(3, 37, 256, 32, False), (2, 19, 256, 128, True), (1, 5, 48, 16, True), (4, 130, 64, 64, False)])
def test_gru_fwd_bwd_vs_torch(B, T, In, H, bi):
    """ctts_gru_fwd/bwd (+ the input-projection and dW_hh GEMMs) against torch.nn.GRU on the CPU in fp64."""
    torch.manual_seed(B * 100 + T)
    ref = torch.nn.GRU(In, H, batch_first=True, bidirectional=bi).double()
    x = rnd(B, T, In, seed=5).requires_grad_(True)
    mem, _ = ref(x.double())
    gy = rnd(*mem.shape, seed=6)
    mem.backward(gy.double())
    names = ["weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"]
    if bi:
        names += [n + "_reverse" for n in names]
    prm = {n: getattr(ref, n).detach().float().to(DEV).requires_grad_(True) for n in names}
    xd = x.detach().to(DEV).requires_grad_(True)
    args = [prm["weight_ih_l0"], prm["weight_hh_l0"], prm["bias_ih_l0"], prm["bias_hh_l0"]]
    if bi:
        args += [prm["weight_ih_l0_reverse"], prm["weight_hh_l0_reverse"], prm["bias_ih_l0_reverse"], prm["bias_hh_l0_reverse"]]
    out = ops.gru(xd, *args)
    close(out, mem, 2e-5, "gru out")
    out.backward(gy.to(DEV))
    close(xd.grad, x.grad, 5e-5, "gru dx")
    for n in names:
        close(prm[n].grad, getattr(ref, n).grad, 5e-5, "gru d" + n)


def test_gru_unsupported_hidden_size_fails_loudly():
    from ctts_amd._lib import CttsError
    with pytest.raises(CttsError):
        K.gru_fwd(torch.zeros(1, 2, 3 * 24, device=DEV), torch.zeros(1, 72, 24, device=DEV), torch.zeros(1, 72, device=DEV), 24, 1)


def test_masked_softmax_rect_and_bmm_nt():
    B, Tq, Tk, C = 3, 11, 70, 32
    q, k = rnd(B, Tq, C, seed=7).requires_grad_(True), rnd(B, Tk, C, seed=8).requires_grad_(True)
    klens, qlens = torch.tensor([70, 33, 1]), torch.tensor([11, 4, 7])
    s = torch.einsum("bqc,bkc->bqk", q.double(), k.double()) * 0.25
    s = s.masked_fill(torch.arange(Tk)[None, None, :] >= klens[:, None, None], float("-inf"))
    ref = torch.softmax(s, -1).masked_fill(torch.arange(Tq)[None, :, None] >= qlens[:, None, None], 0.0)
    gy = rnd(B, Tq, Tk, seed=9)
    ref.backward(gy.double())
    qd, kd = [t.detach().to(DEV).requires_grad_(True) for t in (q, k)]
    P = ops.masked_softmax(ops.bmm_nt(qd, kd, 0.25), klens.to(DEV).int(), qlens.to(DEV).int())
    close(P, ref, 1e-5, "softmax")
    assert (P[1, :, 33:] == 0).all() and (P[1, 4:] == 0).all()
    P.backward(gy.to(DEV))
    close(qd.grad, q.grad, 2e-5, "dq")
    close(kd.grad, k.grad, 2e-5, "dk")
    # no masks (STL token attention)
    P2 = ops.masked_softmax(torch.randn(1, 5, 32, device=DEV))
    close(P2.sum(-1), torch.ones(1, 5), 1e-6, "rows sum to 1")


@pytest.mark.parametrize("B,Tm,Ts", [(3, 61, 17), (2, 300, 130), (2, 40, 260)])
def test_forward_sum_kernel_vs_torch_ctc(B, Tm, Ts):
    """ctts_forward_sum_fwd/bwd against torch's CPU ctc_loss applied per utterance exactly as ForwardSumLoss does (loss.py:350-377),
    incl. an utterance with more tokens than frames (infinite nll -> zero loss and zero gradient)."""
    g = torch.Generator().manual_seed(B * Tm + Ts)
    a = (torch.randn(B, 1, Tm, Ts, generator=g) * 2).requires_grad_(True)
    in_lens = torch.tensor([Ts, max(1, Ts - 5), 3][:B])
    out_lens = torch.tensor([Tm, max(2, Tm - 7), 2][:B])          # B == 3: the last utterance has 3 tokens but 2 frames -> inf
    # reference formulation, float64 on the CPU
    total = 0.0
    pad = F.pad(a.double(), (1, 0), value=-1.0)
    for b in range(B):
        K_, T_ = int(in_lens[b]), int(out_lens[b])
        lp = torch.log_softmax(pad[b].permute(1, 0, 2)[:T_, :, :K_ + 1], dim=-1)
        total = total + F.ctc_loss(lp, torch.arange(1, K_ + 1)[None], torch.tensor([T_]), torch.tensor([K_]), blank=0,
                                   reduction="mean", zero_infinity=True)
    total = total / B
    total.backward()
    ad = a.detach().to(DEV).requires_grad_(True)
    from ctts_amd.loss import CompTransTTSLoss
    loss = CompTransTTSLoss.forward_sum_loss(ad, in_lens.to(DEV), out_lens.to(DEV))
    assert abs(float(loss) - float(total)) <= 2e-5 * max(1.0, abs(float(total))), (float(loss), float(total))
    loss.backward()
    close(ad.grad, a.grad, 2e-5, "forward-sum grad")
    assert torch.isfinite(ad.grad).all()


def test_fused_adam_clip_matches_torch():
    """ctts_adam_clip_step (flat arenas) against nn.utils.clip_grad_norm_ + torch.optim.Adam on the same tensors, 4 steps,
    with and without the clip being active."""
    from ctts_amd.dp import FlatGradArena, FlatAdam
    torch.manual_seed(3)
    shapes = [(257, 33), (1024,), (7,), (3, 5, 9), (1,)]
    ref = [torch.nn.Parameter(torch.randn(*s)) for s in shapes]
    mine = [torch.nn.Parameter(p.detach().clone().to(DEV)) for p in ref]
    opt = torch.optim.Adam(ref, lr=3e-3, betas=(0.9, 0.98), eps=1e-9)
    arena = FlatGradArena(mine)
    fa = FlatAdam(arena, 3e-3, betas=(0.9, 0.98), eps=1e-9, max_norm=1.0)
    for it in range(4):
        scale = 0.01 if it == 2 else 5.0                      # step 2: total norm below max_norm -> no clipping
        gs = [torch.randn(*s) * scale for s in shapes]
        for p, g in zip(ref, gs):
            p.grad = g.clone()
        total = torch.nn.utils.clip_grad_norm_(ref, 1.0)
        opt.step()
        for p, g in zip(mine, gs):
            p.grad.copy_(g.to(DEV))
        fa.step()
        assert abs(float(fa.total_norm) - float(total)) <= 1e-5 * max(1.0, float(total))
        for p, q in zip(ref, mine):
            close(q, p, 2e-6, f"param after step {it}")
    assert float(fa.state[1]) == 4.0 and abs(float(fa.state[0]) ** 0.5 - float(total)) <= 1e-5 * max(1.0, float(total))
    assert mine[0].data_ptr() == fa.flat_param.data_ptr()     # parameters are views of the flat arena


def test_row_tile_map_schedule():
    """ctts_row_tile_map: stable partition of the 64-row tiles into active (first) / wholly-padded, for two halos."""
    T, lens = 300, [300, 10, 0, 129, 64]
    M = T * len(lens)
    lt = torch.tensor(lens, dtype=torch.int32, device=DEV)
    for halo in (0, 4):
        tm = K.row_tile_map(lt, T, halo, M).cpu().numpy()
        tiles = (M + 63) // 64
        act, ina = [], []
        for t in range(tiles):
            r0, last = t * 64, min(t * 64 + 64, M) - 1
            b0, b1 = r0 // T, last // T
            (ina if (b0 == b1 and r0 - b0 * T >= lens[b0] + halo) else act).append(t)
        assert tm[0] == len(act) and list(tm[1:]) == act + ina


def test_gru_group_matches_separate_grus():
    """ops.gru_group: two independent forward GRUs in one launch == the same GRUs run one by one (values and gradients)."""
    B, T, In, H = 3, 29, 64, 32
    ps = []
    for i in range(2):
        torch.manual_seed(40 + i)
        ps.append([t.to(DEV).requires_grad_(True) for t in (rnd(3 * H, In, seed=i, scale=0.2), rnd(3 * H, H, seed=9 + i, scale=0.3),
                                                           rnd(3 * H, seed=20 + i), rnd(3 * H, seed=30 + i))])
    xs = [rnd(B, T, In, seed=50 + i).to(DEV).requires_grad_(True) for i in range(2)]
    gy = [rnd(B, T, H, seed=60 + i).to(DEV) for i in range(2)]
    sep = [ops.gru(xs[i], ps[i][0], ps[i][1], ps[i][2], ps[i][3]) for i in range(2)]
    (sep[0] * gy[0]).sum().backward(); (sep[1] * gy[1]).sum().backward()
    ref = [[t.grad.clone() for t in ps[i]] + [xs[i].grad.clone()] for i in range(2)]
    for t in ps[0] + ps[1] + xs:
        t.grad = None
    gis = [ops.linear(xs[i], ps[i][0], ps[i][2]) for i in range(2)]
    grp = ops.gru_group(gis, [ps[0][1], ps[1][1]], [ps[0][3], ps[1][3]])
    ((grp[0] * gy[0]).sum() + (grp[1] * gy[1]).sum()).backward()
    for i in range(2):
        close(grp[i], sep[i], 1e-6, f"gru_group out {i}")
        for a, b in zip([t.grad for t in ps[i]] + [xs[i].grad], ref[i]):
            close(a, b, 1e-5, f"gru_group grad {i}")


@pytest.mark.parametrize("V,C,shape", [(300, 256, (16, 1024)), (361, 256, (3, 50)), (17, 64, (5,)), (9, 384, (4, 7))])
def test_embedding_fwd_bwd_vs_torch(V, C, shape):
    """ctts_embedding_fwd/bwd against F.embedding with padding_idx=0 (zero gradient row), heavy index repetition included."""
    g = torch.Generator().manual_seed(V + C)
    ids = torch.randint(0, V, shape, generator=g)
    ids.view(-1)[::3] = 1                                   # one very popular row
    w = rnd(V, C, seed=5).requires_grad_(True)
    gy = rnd(*shape, C, seed=6)
    ref = F.embedding(ids, w.double(), padding_idx=0)
    ref.backward(gy.double())
    wd = w.detach().to(DEV).requires_grad_(True)
    out = ops.embedding(ids.to(DEV), wd, 0)
    assert torch.equal(out.cpu(), F.embedding(ids, w.detach()))
    out.backward(gy.to(DEV))
    close(wd.grad, w.grad, 1e-5, "embedding grad")
    assert float(wd.grad[0].abs().max()) == 0.0


def test_fused_mel_l1_pair_matches_torch_formula():
    """ctts_mel_l1_fwd/bwd against CompTransTTSLoss._masked_l1_mel (the reference's masked l1, loss.py:130-138), incl. an all-zero target
    row inside the valid region (weight 0) and padded rows."""
    from oracle.loss_restate import RefLoss as CompTransTTSLoss
    B, T, C = 3, 37, 80
    g = torch.Generator().manual_seed(9)
    tgt = torch.randn(B, T, C, generator=g)
    tgt[1, 5] = 0.0
    pad = torch.arange(T)[None, :] >= torch.tensor([37, 20, 1])[:, None]
    p1 = torch.randn(B, T, C, generator=g).requires_grad_(True)
    p2 = torch.randn(B, T, C, generator=g).requires_grad_(True)
    r1 = CompTransTTSLoss._masked_l1_mel(p1.double(), tgt.double(), pad)
    r2 = CompTransTTSLoss._masked_l1_mel(p2.double(), tgt.double(), pad)
    (r1 * 0.7 + r2 * 1.3).backward()
    d1, d2 = p1.detach().to(DEV).requires_grad_(True), p2.detach().to(DEV).requires_grad_(True)
    both = ops.mel_l1_pair(d1, d2, tgt.to(DEV), pad.to(DEV))
    close(both, torch.stack([r1, r2]), 1e-5, "mel l1 pair")
    (both[0] * 0.7 + both[1] * 1.3).backward()
    close(d1.grad, p1.grad, 1e-6, "d mel")
    close(d2.grad, p2.grad, 1e-6, "d postnet mel")


@pytest.mark.parametrize("Cc", [1, 3, 11, 64, 80])
def test_accumulators_are_rezeroed_on_every_graph_replay(Cc):
    """Zero-filled accumulators inside a captured hipGraph: hipMemsetAsync nodes left stale data in bytes 8..11 from the second replay
    on (found when a replayed train step diverged); the library zero-fills with a kernel (ctts_zero_async) - exact on every replay."""
    x = torch.randn(512, Cc, device=DEV)
    K.colsum(x)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = K.colsum(x)
    for _ in range(4):
        x.normal_()
        g.replay()
        torch.cuda.synchronize()
        close(res, x.double().sum(0), 1e-5, "colsum under graph replay")


def test_c_abi_rejects_bad_arguments_with_messages():
    """int status + thread-local error string (include/ctts.h conventions): every wrapper raises CttsError carrying ctts_last_error()."""
    from ctts_amd._lib import CttsError
    x = torch.zeros(4, 8, 6, device=DEV)                 # C = 6 is not a multiple of 4
    with pytest.raises(CttsError, match="C % 4"):
        K.im2col_3x3s2(x.view(1, 4, 8, 6))
    with pytest.raises(CttsError, match="conv view needs cin"):
        K.gemm(torch.zeros(8, 6, device=DEV), torch.zeros(4, 18, device=DEV), torch.zeros(8, 4, device=DEV), 8, 4, 18, 6, 18, 4, True, True,
               conv=(8, 1, 6))
    with pytest.raises(CttsError, match="p_drop"):
        K.gemm(torch.zeros(8, 8, device=DEV), torch.zeros(8, 8, device=DEV), torch.zeros(8, 8, device=DEV), 8, 8, 8, 8, 8, 8, True, True,
               p_drop=1.5)
    with pytest.raises(CttsError, match="excludes bias"):
        K.gemm(torch.zeros(8, 8, device=DEV), torch.zeros(8, 8, device=DEV), torch.zeros(8, 8, device=DEV), 8, 8, 8, 8, 8, 8, True, True,
               bias=torch.zeros(8, device=DEV), E=torch.zeros(8, 8, device=DEV), rowsub=torch.zeros(8, device=DEV))
    with pytest.raises(CttsError, match="Tk"):
        K.forward_sum_fwd(torch.zeros(1, 4, 2000, device=DEV), torch.ones(1, dtype=torch.int32, device=DEV),
                          torch.ones(1, dtype=torch.int32, device=DEV), -1.0)
    with pytest.raises(CttsError, match="CPU tensor"):
        K.colsum(torch.zeros(4, 4))
    # a failed call does not poison the library: the next valid call works
    assert float(K.colsum(torch.ones(5, 3, device=DEV)).sum()) == 15.0


@pytest.mark.parametrize("case", ["nt_plain", "nn_plain", "ff1_bias_swish_z_drop", "out_bias_drop_residual_ragged", "nn_epi_bwd_gelu_drop",
                                  "nn_epi_bwd_plain", "relu_inference", "edge_m_n_ldc", "edge_narrow"])
def test_weight_stationary_gemm_equals_tile_kernels_and_fp64(case):
    """csrc/gemm_ws.hip (K = 256: the weight slice of a workgroup in registers, A tiles streamed through LDS by DMA, epilogue with
    hardware range checks) against the other kernels of ctts_gemm on the SAME descriptor and against an fp64 computation: both operand
    layouts, every epilogue it compiles (bias / activation / pre-activation store / dropout / residual / backward of the producer's
    epilogue), padded-row schedule, M not a multiple of 64, N not a multiple of 128 or 32, ldc > N.  The descriptor must really take the
    weight-stationary path (asserted), and nothing outside C[:, :N] may be written."""
    torch.manual_seed(5)
    B, T = 8, 640
    M, N = B * T, 768
    lens = torch.tensor([640, 611, 77, 300, 512, 64, 1, 257], dtype=torch.int32, device=DEV)
    seed = torch.full((1,), 77, dtype=torch.int64, device=DEV)
    ldc = N
    kw, ref = {}, None
    if case in ("edge_m_n_ldc", "edge_narrow"):
        M, N = (4133, 200) if case == "edge_m_n_ldc" else (4100, 80)
        ldc = N + 8
    x = torch.randn(M, 256, device=DEV)
    w = torch.randn(N, 256, device=DEV) * 0.05
    bias = torch.randn(N, device=DEV) * 0.1
    R = torch.randn(M, N, device=DEV)
    Cbuf = torch.empty(M, ldc, device=DEV)
    outs = [Cbuf]
    nt = (x, w, Cbuf, M, N, 256, 256, 256, ldc, True, True)
    nn = (x, w.t().contiguous(), Cbuf, M, N, 256, 256, N, ldc, True, False)
    xw = x.double() @ w.double().t()
    if case in ("nt_plain", "edge_m_n_ldc", "edge_narrow"):
        args, ref = nt, [xw]
    elif case == "nn_plain":
        args, ref = nn, [xw]
    elif case == "ff1_bias_swish_z_drop":
        Z = torch.empty(M, N, device=DEV)
        outs.append(Z)
        args, kw = nt, dict(bias=bias, Z=Z, ldz=N, act=K.ACT_SWISH, p_drop=0.1, seed=seed, drop_offset=3)
    elif case == "out_bias_drop_residual_ragged":
        args = nt
        kw = dict(bias=bias, alpha=0.5, p_drop=0.1, seed=seed, drop_offset=5, R=R, ldr=N, row_lens=lens, row_T=T, row_halo=0,
                  tile_map=K.row_tile_map(lens, T, 0, M))
    elif case == "nn_epi_bwd_gelu_drop":
        args, kw = nn, dict(Z=R, ldz=N, act=K.ACT_GELU, p_drop=0.1, seed=seed, drop_offset=7, epi_bwd=True)
    elif case == "nn_epi_bwd_plain":
        args, kw = nn, dict(alpha=0.25, epi_bwd=True)
        ref = [0.25 * xw]
    else:
        args, kw = nt, dict(bias=bias, act=K.ACT_RELU)           # activation without Z: the store runs into an empty descriptor
        ref = [torch.relu(xw + bias.double())]
    assert K.gemm_takes_weight_stationary(*args, **kw), "the descriptor is expected to take the weight-stationary path"
    res = []
    try:
        for on in (False, True):
            K.gemm_ws_enable(on)
            for o in outs:
                o.fill_(float("nan"))
            K.gemm(*args, **kw)
            torch.cuda.synchronize()
            res.append([o.clone() for o in outs])
    finally:
        K.gemm_ws_enable(True)
    valid = slice(None)
    for u, v in zip(res[0], res[1]):
        if ldc > N:
            assert torch.isnan(v[:, N:]).all(), "columns beyond N were written"
            u, v = u[:, :N], v[:, :N]
        if case == "out_bias_drop_residual_ragged":              # padded rows of active tiles hold unspecified finite values in both
            rows = (torch.arange(T, device=DEV)[None, :] < lens[:, None]).reshape(M)
            assert torch.isfinite(v).all()
            u, v = u[rows], v[rows]
        assert torch.isfinite(v).all()
        close(v, u, 1e-6, "weight-stationary vs tile kernels " + case)
    if ref is not None:
        close(res[1][0][:, :N], ref[0], 2e-5, "weight-stationary vs fp64 " + case)


_LEAN = [  # (name, act, drop, residual, rowscale, bias, backward)
    ("plain", 0, False, False, False, False, False), ("b", 0, False, False, False, True, False),
    ("bdr", 0, True, True, False, True, False), ("br", 0, False, True, False, True, False),
    ("bdrs", 0, True, True, True, True, False), ("brs", 0, False, True, True, True, False),
    ("ba1z", 1, False, False, False, True, False), ("ba2zd", 2, True, False, False, True, False), ("ba2z", 2, False, False, False, True, False),
    ("ba4zd", 4, True, False, False, True, False), ("ba4z", 4, False, False, False, True, False),
    ("a1zB", 1, False, False, False, False, True), ("a2zdB", 2, True, False, False, False, True), ("a4zdB", 4, True, False, False, False, True)]


@pytest.mark.parametrize("mode", _LEAN, ids=[m[0] for m in _LEAN])
@pytest.mark.parametrize("M,N,Kd,pad", [(150, 200, 64, 0), (333, 77, 96, 5), (4200, 264, 256, 0)])
def test_gemm_lean_epilogue_modes_vs_fp64(mode, M, N, Kd, pad):
    """Every combination `gemm_epilogue_auto` (csrc/gemm_common.h) sends to the compile-time specialised epilogue with hardware range
    checks, on shapes that exercise the range checks (M, N not multiples of the tile, ldc / ldz / ldr > N) and on all three kernel
    families (tile kernels; K = 256 with >= 4096 rows: weight-stationary): C, the stored pre-activation, nothing written outside
    [:M, :N].  Reference in float64 with the dropout mask regenerated by the standalone kernel from (seed, offset, m*N + n)."""
    name, act, drop, res, rs, has_b, bwd = mode
    p = 0.25 if drop else 0.0
    ld = N + pad
    A, B = rnd(M, Kd, seed=31).to(DEV), rnd(N, Kd, seed=32, scale=0.3).to(DEV)
    bias = rnd(N, seed=33).to(DEV) if has_b else None
    R = torch.randn(M, ld, device=DEV) if res else None
    rowscale = (torch.rand(M, device=DEV) > 0.3).float() if rs else None
    seed = torch.full((1,), 4242, dtype=torch.int64, device=DEV)
    off, alpha = 11, 0.7
    Cb = torch.full((M + 3, ld), float("nan"), device=DEV)
    kw = dict(alpha=alpha, act=act, p_drop=p, seed=seed if drop else None, drop_offset=off)
    fns = {0: lambda v: v, 1: torch.relu, 2: lambda v: F.gelu(v), 4: lambda v: v * torch.sigmoid(v)}
    mask = torch.ones(M, N, dtype=torch.float64, device=DEV)
    if drop:
        mask = K.rowscale_dropout(torch.ones(M, N, device=DEV), None, p, seed, off).double()       # 0 or 1/(1-p)
        _assert_restated_mask(mask, p, seed, off)
    acc = A.double() @ B.double().t()
    if not bwd:
        Zb = torch.full((M + 3, ld), float("nan"), device=DEV) if act else None
        K.gemm(A, B, Cb, M, N, Kd, Kd, Kd, ld, True, True, bias=bias, Z=Zb, ldz=ld, R=R, ldr=ld, rowscale=rowscale, **kw)
        z = alpha * (acc + (bias.double() if has_b else 0.0))
        ref = fns[act](z) * mask
        if res:
            ref = ref + R[:, :N].double()
        if rs:
            ref = ref * rowscale.double()[:, None]
        if act:
            close(Zb[:M, :N], z, 1e-5, f"Z {name}")
            assert torch.isnan(Zb[M:]).all() and (pad == 0 or torch.isnan(Zb[:, N:]).all()), "Z written out of range"
    else:
        Zp = torch.randn(M, ld, device=DEV)                    # the producer's stored pre-activation: an input
        K.gemm(A, B, Cb, M, N, Kd, Kd, Kd, ld, True, True, Z=Zp, ldz=ld, epi_bwd=True, **kw)
        zz = Zp[:, :N].double().requires_grad_()
        fns[act](zz).sum().backward()
        ref = alpha * acc * mask * zz.grad
    close(Cb[:M, :N], ref, 2e-5, f"C {name}")
    assert torch.isnan(Cb[M:]).all() and (pad == 0 or torch.isnan(Cb[:, N:]).all()), "C written out of range"


def test_gemm_lean_split_k_partials_and_batched_limits():
    """The two remaining special forms: split-K (partial matrices in the workspace + the ordered reduce launch; rows / columns beyond the
    operand never touched) and the plain epilogue of a batched launch with per-batch length limits (each batch's descriptor ends at ITS
    valid extent)."""
    M, N, Kd = 130, 70, 2048
    A, B = rnd(Kd, M, seed=41).to(DEV), rnd(Kd, N, seed=42).to(DEV)                   # TN: both reduction-major
    Cb = torch.zeros(M + 2, N + 6, device=DEV)
    K.gemm(A, B, Cb, M, N, Kd, M, N, N + 6, False, False, split_k=4, alpha=0.5)
    close(Cb[:M, :N], 0.5 * (A.double().t() @ B.double()), 2e-5, "split-K")
    assert float(Cb[M:].abs().max()) == 0.0 and float(Cb[:, N:].abs().max()) == 0.0
    nb, T, dh = 3, 90, 32
    lens = torch.tensor([90, 41, 7], dtype=torch.int32, device=DEV)
    q, k = rnd(nb, T, dh, seed=43).to(DEV), rnd(nb, T, dh, seed=44).to(DEV)
    S = torch.full((nb, T, T), float("nan"), device=DEV)
    K.gemm(q, k, S, T, T, dh, dh, dh, T, True, True, nb0=nb, nb1=1, sA=(T * dh, 0), sB=(T * dh, 0), sC=(T * T, 0), lens=lens, lim=(1, 1, 0),
           alpha=0.25)
    for b in range(nb):
        L = int(lens[b])
        close(S[b, :L, :L], 0.25 * (q[b, :L].double() @ k[b, :L].double().t()), 1e-5, f"batched limits b={b}")
        assert torch.isnan(S[b, L:]).all() and torch.isnan(S[b, :, L:]).all(), "written beyond the batch's limits"


@pytest.mark.parametrize("layout", ["NT", "NN", "TN"])
@pytest.mark.parametrize("M,N,Kd,nb", [(1000, 32, 1000, 3), (300, 20, 129, 2), (257, 8, 64, 1)])
def test_gemm_narrow_output_tiles(layout, M, N, Kd, nb):
    """Outputs at most 32 columns wide run on 128 x 32 tiles (4 x 1 waves; csrc/gemm.hip dispatch_buf_narrow) - the [T, d_head = 32]
    gradients of the conformer's attention: all three operand layouts, batched with strides, ragged M / N / K, ldc > N."""
    torch.manual_seed(3)
    A = torch.randn(nb, M, Kd, device=DEV) if layout != "TN" else torch.randn(nb, Kd, M, device=DEV)
    Bm = torch.randn(nb, N, Kd, device=DEV) if layout == "NT" else torch.randn(nb, Kd, N, device=DEV)
    ldc = N + 4
    Cb = torch.full((nb, M, ldc), float("nan"), device=DEV)
    a_kc, b_kc = layout != "TN", layout == "NT"
    lda = Kd if a_kc else M
    ldb = Kd if b_kc else N
    K.gemm(A, Bm, Cb, M, N, Kd, lda, ldb, ldc, a_kc, b_kc, nb0=nb, nb1=1, sA=(A[0].numel(), 0), sB=(Bm[0].numel(), 0), sC=(M * ldc, 0),
           alpha=0.5)
    Ad = A.double() if a_kc else A.double().transpose(1, 2)
    Bd = Bm.double().transpose(1, 2) if b_kc else Bm.double()
    close(Cb[:, :, :N], 0.5 * (Ad @ Bd), 2e-5, f"narrow {layout}")
    assert torch.isnan(Cb[:, :, N:]).all()


@pytest.mark.parametrize("M,N,Kd", [(2048, 256, 1024), (1000, 200, 520), (300, 64, 2048), (2048, 1024, 256)])
def test_gemm_under_filled_two_group_kernel(M, N, Kd):
    """Launches with few 64 x 64 output tiles (the 2,048-row phoneme-level layers) run on 32 x 64 tiles with the reduction split between
    two wave groups inside the workgroup (csrc/gemm.hip gemm_buf_k2_kernel): NT with bias / alpha / ldc > N, NN, K not a multiple of 64,
    nothing written out of range; and the conv view on ragged rows (padded 32-row tiles zero-filled and skipped)."""
    torch.manual_seed(0)
    x = torch.randn(M, Kd, device=DEV); w = torch.randn(N, Kd, device=DEV) * 0.05; b = torch.randn(N, device=DEV)
    C = torch.full((M + 2, N + 4), float("nan"), device=DEV)
    K.gemm(x, w, C, M, N, Kd, Kd, Kd, N + 4, True, True, bias=b, alpha=0.5)
    close(C[:M, :N], 0.5 * (x.double() @ w.double().t() + b.double()), 2e-5, "NT")
    assert torch.isnan(C[M:]).all() and torch.isnan(C[:, N:]).all()
    C2 = torch.empty(M, N, device=DEV)
    K.gemm(x, w.t().contiguous(), C2, M, N, Kd, Kd, N, N, True, False)
    close(C2, x.double() @ w.double().t(), 2e-5, "NN")
    # TN with split-K partials added onto an existing value (a weight gradient accumulated into param.grad): reduction over M here
    Mo, No = (N, 320) if N >= 256 else (320, N)            # the routed range needs at least 256 output rows
    A = torch.randn(Kd, Mo, device=DEV); Bm = torch.randn(Kd, No, device=DEV)
    out = torch.full((Mo, No), 0.5, device=DEV)
    K.gemm(A, Bm, out, Mo, No, Kd, Mo, No, No, False, False, split_k=2, alpha=0.25)
    close(out, 0.5 + 0.25 * (A.double().t() @ Bm.double()), 2e-5, "TN split-K")


def test_gemm_under_filled_conv_ragged_rows():
    torch.manual_seed(1)
    B, T, Cin, Cout, ks = 16, 128, 256, 256, 5
    lens = torch.tensor([128, 123, 117, 115, 113, 112, 111, 96, 83, 82, 82, 81, 78, 63, 60, 55], dtype=torch.int32, device=DEV)
    xc = torch.randn(B, T, Cin, device=DEV); wc = torch.randn(Cout, ks * Cin, device=DEV) * 0.03
    bias = torch.randn(Cout, device=DEV); Z = torch.full((B, T, Cout), float("nan"), device=DEV)
    Cc = torch.full((B, T, Cout), float("nan"), device=DEV)
    K.gemm(xc, wc, Cc, B * T, Cout, ks * Cin, Cin, ks * Cin, Cout, True, True, conv=(T, ks // 2, Cin), bias=bias, Z=Z, ldz=Cout,
           act=K.ACT_RELU, row_lens=lens, row_T=T, row_halo=0, tile_map=K.row_tile_map(lens, T, 0, B * T))
    w3 = wc.view(Cout, ks, Cin).permute(0, 2, 1).contiguous()
    ref = F.conv1d(xc.double().transpose(1, 2), w3.double(), bias.double(), padding=ks // 2).transpose(1, 2)
    for b_ in range(B):
        L = int(lens[b_])
        close(Z[b_, :L], ref[b_, :L], 2e-5, f"conv Z b={b_}")
        close(Cc[b_, :L], torch.relu(ref[b_, :L]), 2e-5, f"conv C b={b_}")
    assert torch.isfinite(Cc).all() and torch.isfinite(Z).all()          # padded tiles are zero-filled, not left unwritten


@pytest.mark.parametrize("B,T,C,p,use_alpha,use_mask", [(3, 70, 256, 0.2, True, True), (2, 33, 64, 0.0, True, False), (2, 128, 256, 0.1, False, False)])
def test_positional_embedding_add_fwd_bwd(B, T, C, p, use_alpha, use_mask):
    """ops.posembed_add = `x + pos_embed_alpha * embed_positions(x)` + F.dropout + non-pad mask (transformer_fs2.py:41-52,113-119,
    modules.py:1349-1351) as one launch each way: against the torch composition in float64 with the dropout mask regenerated from
    (seed, offset, element index); the forward is BIT-identical to the unfused fp32 sequence (two roundings, no FMA)."""
    g = torch.Generator().manual_seed(B * T + C)
    x = (torch.rand(B, T, C, generator=g) - 0.5)
    lens = torch.tensor([T, max(1, T // 2), max(1, T - 9)][:B])
    x = x * (torch.arange(T)[None, :] < lens[:, None])[..., None]            # padded rows are zero: channel 0 marks non-pad (make_positions)
    x[..., 0] = torch.where(torch.arange(T)[None, :] < lens[:, None], x[..., 0].abs() + 0.1, torch.zeros(()))
    xg = x.to(DEV).requires_grad_()
    alpha = torch.tensor([0.7], device=DEV, requires_grad=True) if use_alpha else None
    nonpad = (torch.arange(T)[None, :] < lens[:, None]).float().reshape(-1).to(DEV) if use_mask else None
    drop = K.DropCtx(DEV, seed=9) if p > 0 else None
    pos = K.positions(xg.detach(), C)
    table = ops.sinusoid_table(T + 1, C, DEV)
    y = ops.posembed_add(xg, pos, table, alpha, nonpad, p, drop)
    go = (torch.rand(B, T, C, generator=g) - 0.5).to(DEV)
    y.backward(go)
    mask = torch.ones(B * T, C, device=DEV)
    if p > 0:
        mask = K.rowscale_dropout(torch.ones(B * T, C, device=DEV), None, p, drop.seed, 1)        # the op drew call-site offset 1
        _assert_restated_mask(mask, p, drop.seed, 1)
    mask = mask.view(B, T, C)
    pe = torch.nn.functional.embedding(pos.long(), table)
    a32 = alpha.detach() if use_alpha else torch.ones(1, device=DEV)
    y32 = (xg.detach() + a32 * pe) * mask
    if use_mask:
        y32 = y32 * nonpad.view(B, T, 1)
    assert torch.equal(y.detach(), y32), "forward differs from the unfused fp32 sequence"
    m64 = mask.double() * (nonpad.view(B, T, 1).double() if use_mask else 1.0)
    close(xg.grad, go.double() * m64, 1e-6, "posembed dx")
    if use_alpha:
        close(alpha.grad, (go.double() * m64 * pe.double()).sum().view(1), 1e-5 * (B * T * C) ** 0.5, "posembed dalpha")


def test_batched_conv_data_gradient_weights_equal_the_per_layer_repack():
    """ctts_conv_dgrad_weights (one launch for all Conv1d layers, 32 x 32 tiles through LDS) against ctts_conv_weight_repack mode 4 layer
    by layer - bit-identical copies, ragged channel counts (80), k = 1, more than 32 tasks (two launches) included - and
    ops.prepare_dgrad_weights feeding _LinearConv.backward the same data gradient as the per-layer path."""
    g = torch.Generator().manual_seed(3)
    shapes = [(1024, 256, 9), (256, 1024, 1), (512, 80, 5), (80, 512, 5), (256, 256, 3), (33, 7 * 4, 5)] + [(64, 32, 3)] * 30
    ws = [torch.rand(co, k, ci, generator=g).to(DEV) for co, ci, k in shapes]
    outs = K.conv_dgrad_weights([(w.view(w.shape[0], -1), co, ci, k) for w, (co, ci, k) in zip(ws, shapes)])
    for w, (co, ci, k), o in zip(ws, shapes, outs):
        ref = torch.empty(ci, k * co, device=DEV)
        K.conv_weight_repack(w.view(co, k * ci), ref, co, ci, k, 4)
        assert torch.equal(o, ref), (co, ci, k)
    # through the autograd function: prepared weights vs per-layer repack
    B, T, Cin, Cout, ks = 2, 70, 64, 128, 5
    wp = torch.nn.Parameter(torch.rand(Cout, ks, Cin, generator=g).to(DEV).permute(0, 2, 1))        # GEMM-major like model._Conv
    x = torch.rand(B, T, Cin, generator=g).to(DEV)
    go = torch.rand(B, T, Cout, generator=g).to(DEV)
    grads = []
    for prepared in (False, True):
        xi = x.clone().requires_grad_()
        if prepared:
            ops.prepare_dgrad_weights([wp])
            assert wp.data_ptr() in ops._DGRAD_W
        y = ops.conv1d(xi, wp, None)
        y.backward(go)
        assert wp.data_ptr() not in ops._DGRAD_W
        grads.append(xi.grad.clone())
        wp.grad = None
    assert torch.equal(grads[0], grads[1])
    ops.clear_dgrad_weights()


@pytest.mark.parametrize("kind", ["l1", "l2", "bce"])
def test_masked_loss_matches_torch_and_is_bit_reproducible(kind):
    """ops.masked_loss (csrc/loss.hip): sum(w * l(p, t)) / sum(w) and its gradient against stock torch in fp64; two runs identical."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(17)
    n = (16, 1000)
    p = torch.randn(n, generator=g).to(DEV).requires_grad_(True)
    t = (torch.rand(n, generator=g) < 0.4).float().to(DEV) if kind == "bce" else torch.randn(n, generator=g).to(DEV)
    w = (torch.rand(n, generator=g) < 0.7).float().to(DEV)
    fn = {"l1": lambda a, b: (a - b).abs(), "l2": lambda a, b: (a - b) ** 2,
          "bce": lambda a, b: F.binary_cross_entropy_with_logits(a, b, reduction="none")}[kind]
    p64 = p.detach().double().requires_grad_(True)
    ref = (fn(p64, t.double()) * w.double()).sum() / w.double().sum()
    ref.backward()
    outs = []
    for _ in range(2):
        p.grad = None
        v = ops.masked_loss(p, t, w, kind)
        (v * 3.0).backward()
        outs.append((v.item(), p.grad.clone()))
    assert outs[0][0] == outs[1][0] and torch.equal(outs[0][1], outs[1][1])
    assert abs(outs[0][0] - ref.item()) <= 2e-6 * max(1.0, abs(ref.item()))
    assert (outs[0][1].double() - 3.0 * p64.grad).abs().max().item() <= 1e-9 + 1e-5 * p64.grad.abs().max().item()


def _nt_gemm(A, B, M, N, Kd, **kw):
    out = torch.full((M, N), float("nan"), device=DEV)
    K.gemm(A, B, out, M, N, Kd, Kd, Kd, N, True, True, **kw)
    return out


def test_bf16_split_gemm_is_exact_where_fp32_is_and_fp32_class_elsewhere():
    """csrc/gemm.hip gemm_x6_kernel: fp32 products from six bf16 MFMA terms of the exact hi / mid / lo split of both operands.
    (1) integer operands whose products and sums are exactly representable in fp32 - one operand with 18 significant bits (needs all
    three pieces), the other sparse in {-1, 0, 1}, in both roles (the lo x hi and the hi x lo terms) - must come out EXACTLY; (2) on random
    data the error against float64 is not above the fp32-MFMA kernels' on the same launch (same-process A/B through
    ctts_gemm_bf16_split_enable); (3) two runs are bit-identical."""
    M, N, Kd = 8192, 768, 512
    g = torch.Generator().manual_seed(5)

    def big(rows):
        return torch.randint(-(1 << 17), (1 << 17) + 1, (rows, Kd), generator=g).float()

    def sparse(rows):
        return (torch.randint(-1, 2, (rows, Kd), generator=g) * (torch.rand(rows, Kd, generator=g) < 1 / 32)).float()
    for A, B in ((big(M), sparse(N)), (sparse(M), big(N))):
        assert K.gemm_takes_bf16_split(A.to(DEV), B.to(DEV), torch.empty(M, N, device=DEV), M, N, Kd, Kd, Kd, N, True, True)
        ref = A.double() @ B.double().t()
        assert float(ref.abs().max()) < 2 ** 24                    # every partial sum is an integer below 2^24: exact in fp32
        got = _nt_gemm(A.to(DEV), B.to(DEV), M, N, Kd)
        assert torch.equal(got.double().cpu(), ref), float((got.double().cpu() - ref).abs().max())
    A = torch.randn(M, Kd, generator=g).to(DEV)
    B = (torch.randn(N, Kd, generator=g) * 0.1).to(DEV)
    ref = A.double() @ B.double().t()
    x6 = _nt_gemm(A, B, M, N, Kd)
    assert torch.equal(x6, _nt_gemm(A, B, M, N, Kd))
    prev = K.gemm_bf16_split_enable(False)
    try:
        assert not K.gemm_takes_bf16_split(A, B, x6, M, N, Kd, Kd, Kd, N, True, True)
        f32 = _nt_gemm(A, B, M, N, Kd)
    finally:
        K.gemm_bf16_split_enable(prev)
    e6, e32 = float((x6.double() - ref).abs().max()), float((f32.double() - ref).abs().max())
    print(f"max |err| vs fp64: bf16-split {e6:.3e}, fp32 MFMA {e32:.3e}")
    assert e6 <= 1.25 * e32 + 1e-7, (e6, e32)


@pytest.mark.parametrize("act,drop", [(0, 0.0), (2, 0.2)])
def test_bf16_split_gemm_conv_view_ragged_rows_and_epilogues_equal_the_fp32_kernels(act, drop):
    """The same launch (im2col view on A, ragged utterances with the 64-row zero rule, bias / GELU + pre-activation store / dropout /
    residual / row scale) on the bf16-split kernel and on the fp32-MFMA kernels: equal to accumulation-order noise, identical zeros."""
    B_, T, Cin, N, ks = 16, 512, 128, 768, 5
    M, Kd = B_ * T, ks * Cin
    lens = torch.tensor([512, 200, 129, 64, 330, 1, 448, 449, 384, 385, 511, 65, 63, 128, 300, 256], dtype=torch.int32, device=DEV)
    x, w, bias = rnd(B_, T, Cin, seed=301).to(DEV), rnd(N, Kd, seed=302, scale=0.05).to(DEV), rnd(N, seed=303).to(DEV)
    R = rnd(B_, T, N, seed=304).to(DEV)
    rs = (torch.arange(T, device=DEV)[None, :] < lens[:, None]).float().reshape(-1).contiguous()
    seed = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    outs = {}
    for on in (True, False):
        prev = K.gemm_bf16_split_enable(on)
        try:
            out = torch.full((B_, T, N), float("nan"), device=DEV)
            Z = torch.full((B_, T, N), float("nan"), device=DEV) if act else None
            args = (x, w, out, M, N, Kd, Cin, Kd, N, True, True)
            kw = dict(conv=(T, ks // 2, Cin), alpha=0.5, bias=bias, act=act, p_drop=drop, seed=seed, drop_offset=3, R=R, ldr=N, rowscale=rs,
                      row_lens=lens, row_T=T, row_halo=0)
            if act:
                kw.update(Z=Z, ldz=N)
            assert K.gemm_takes_bf16_split(*args, **kw) == on
            K.gemm(*args, **kw)
            outs[on] = (out, Z)
        finally:
            K.gemm_bf16_split_enable(prev)
    (o6, z6), (o32, z32) = outs[True], outs[False]
    assert torch.isfinite(o6).all() and (o6 == 0).eq(o32 == 0).all()
    assert float((o6 - o32).abs().max()) <= 2e-5
    if act:
        assert float((z6 - z32).abs().max()) <= 2e-5 and (z6 == 0).eq(z32 == 0).all()


@pytest.mark.parametrize("conv,split,ragged,T", [(False, 1, False, 512), (False, 4, True, 512), (True, 4, True, 512), (True, 1, False, 512),
                                                 (True, 4, False, 1000)])       # T = 1000: the conformer's decoder length (not a multiple of 32)
def test_bf16_split_weight_gradient_gemm_vs_fp64_and_the_fp32_kernels(conv, split, ragged, T):
    """gemm_x6tn_kernel (TN layout: dW[m][n] = sum_k dZ[k][m] X[k][n], optional im2col view on X, K-blocks in padding skipped, ordered
    split-K partials): exact on integer data, against float64 not worse than the fp32-MFMA kernels on the same launch, bit-reproducible."""
    if os.environ.get("CTTS_X6_TN", "1") == "0":
        pytest.skip("CTTS_X6_TN=0")
    B_, Cin, ks, Mo = 8, 128, 3 if conv else 1, 512
    Kred, No = B_ * T, ks * Cin
    lens = torch.tensor([512, 200, 129, 64, 330, 1, 448, 385], dtype=torch.int32, device=DEV)
    valid = (torch.arange(T, device=DEV)[None, :] < lens[:, None]).float().reshape(-1, 1) if ragged else 1.0
    g = torch.Generator().manual_seed(9)
    force = K.gemm_bf16_split_enable(2)          # the test launches are below the kernel's size threshold
    try:
        _bf16_split_tn_body(conv, split, ragged, B_, T, Cin, ks, Mo, Kred, No, lens, valid, g)
    finally:
        K.gemm_bf16_split_enable(force)


def _bf16_split_tn_body(conv, split, ragged, B_, T, Cin, ks, Mo, Kred, No, lens, valid, g):
    def run(dz, x):
        out = torch.full((Mo, No), float("nan"), device=DEV) if split == 1 else torch.zeros(Mo, No, device=DEV)
        kw = dict(alpha=1.0)
        if conv:
            kw.update(conv=(T, ks // 2, Cin), conv_on_b=True)
        if ragged:
            kw.update(row_lens=lens, row_T=T, row_halo=0)
        if split > 1:
            kw.update(split_k=split)
        args = (dz, x, out, Mo, No, Kred, Mo, Cin, No, False, False)
        took = K.gemm_takes_bf16_split(*args, **kw)
        K.gemm(*args, **kw)
        return out, took

    def ref64(dz, x):
        xd = x.double().view(B_, T, Cin)
        if conv:
            pad = ks // 2
            xp = torch.nn.functional.pad(xd, (0, 0, pad, pad))
            cols = torch.cat([xp[:, kk:kk + T] for kk in range(ks)], dim=-1).reshape(Kred, No)       # [k][(tap, c)]
        else:
            cols = xd.reshape(Kred, No)
        return dz.double().t() @ cols

    # exact case: 18-bit integers against sparse +-1 (every fp32 partial sum exact)
    dz = (torch.randint(-1, 2, (Kred, Mo), generator=g) * (torch.rand(Kred, Mo, generator=g) < 1 / 64)).float().to(DEV) * valid
    x = torch.randint(-(1 << 17), (1 << 17) + 1, (Kred, Cin), generator=g).float().to(DEV)
    got, took = run(dz, x)
    assert took, "expected on the bf16-split weight-gradient kernel"
    ref = ref64(dz, x)
    assert float(ref.abs().max()) < 2 ** 24 and torch.equal(got.double(), ref), float((got.double() - ref).abs().max())
    # random data: error vs float64 next to the fp32-MFMA kernels, and run-to-run identity
    dz = torch.randn(Kred, Mo, generator=g).to(DEV) * valid
    x = torch.randn(Kred, Cin, generator=g).to(DEV)
    ref = ref64(dz, x)
    a, _ = run(dz, x)
    b, _ = run(dz, x)
    assert torch.equal(a, b)
    K.gemm_bf16_split_enable(False)
    try:
        f32, took32 = run(dz, x)
        assert not took32
    finally:
        K.gemm_bf16_split_enable(2)
    e6, e32 = float((a.double() - ref).abs().max()), float((f32.double() - ref).abs().max())
    print(f"TN max |err| vs fp64: bf16-split {e6:.3e}, fp32 MFMA {e32:.3e}")
    # both accumulate 4,096+ products per output in fp32; the fp32-MFMA path cuts that chain (stream-K / split-K pieces summed
    # afterwards), so its rounding error is somewhat smaller on unsplit launches - the products themselves are exact either way (above)
    assert e6 <= 2.5 * e32 + 1e-6, (e6, e32)


def _route_unit(M, N, Kd, g):              # test_gemm_nt's operands
    return torch.rand(M, Kd, generator=g) * 2 - 1, torch.rand(N, Kd, generator=g) * 2 - 1


def _route_exact(M, N, Kd, g):             # 18-bit integers against sparse +-1: every fp32 partial sum is an exact integer
    big = torch.randint(-(1 << 17), (1 << 17) + 1, (M, Kd), generator=g).float()
    return big, (torch.randint(-1, 2, (N, Kd), generator=g) * (torch.rand(N, Kd, generator=g) < 1 / 64)).float()


# kind, layout, M, N, K, operands [M, K] x [N, K], keyword arguments, bound on max |C - float64| given max |float64| - each the bound of
# the family's own test on that operand distribution (named on the line)
_ROUTE_CASES = [
    ("scalar64", "NT", 70, 50, 30, _route_unit, {}, lambda s: 2e-6 * max(1, 30 / 16) * max(1.0, s)),           # test_gemm_nt
    ("buf64", "NT", 130, 130, 64, _route_unit, {}, lambda s: 2e-6 * max(1, 64 / 16) * max(1.0, s)),            # test_gemm_nt
    ("buf_k2", "NT", 256, 64, 256, _route_unit, {}, lambda s: 2e-6 * max(1, 256 / 16) * max(1.0, s)),          # test_gemm_nt
    ("buf_narrow", "NT", 256, 32, 64, _route_unit, {}, lambda s: 2e-6 * max(1, 64 / 16) * max(1.0, s)),        # test_gemm_nt
    ("x6", "NT", 1024, 128, 256, _route_exact, dict(bf16_split=2), lambda s: 0.0),                             # test_bf16_split_gemm_is_exact_...
    ("x6tn", "TN", 128, 128, 2048, _route_exact, dict(bf16_split=2, split_k=2), lambda s: 0.0),                # test_bf16_split_weight_gradient_...
    ("weight_stationary", "NT", 4096, 64, 256,                                                                 # test_weight_stationary_gemm_...
     lambda M, N, Kd, g: (torch.randn(M, Kd, generator=g), torch.randn(N, Kd, generator=g) * 0.05), {}, lambda s: 2e-5 * max(1.0, s)),
    ("planes", "NT", 128, 256, 64, _route_unit, dict(bf16_split=2, planes=True), lambda s: 2e-5 * max(1.0, s)),        # test_planes_gpu: ..._vs_fp64
    ("planes_wgrad", "TN", 128, 256, 64, _route_unit, dict(bf16_split=2, split_k=2, planes=True), lambda s: 2e-6 * s),  # test_planes_wgrad_gpu close()
    ("stream_k", "NT", 4096, 1024, 2048,                                                                       # test_dominant_stream_k_kernel_vs_fp64_...
     lambda M, N, Kd, g: (torch.rand(M, Kd, generator=g) - 0.5, (torch.rand(N, Kd, generator=g) - 0.5) * 0.1), dict(bf16_split=0), lambda s: 2e-5),
]


@pytest.mark.parametrize("kind,layout,M,N,Kd,make,kw,bound", _ROUTE_CASES, ids=[c[0] for c in _ROUTE_CASES])
def test_every_route_kind_names_the_kernel_that_runs_the_launch(kind, layout, M, N, Kd, make, kw, bound):
    """K.gemm_route names `kind` for the descriptor, and the launch of the same descriptor computes the product: binds every route kind
    that a small launch reaches to its launcher (the vec kinds need an operand beyond 2 GiB: the test below; buf128 a tuning knob:
    tests/test_gemm_route_cpu.py)."""
    g = torch.Generator().manual_seed(41)
    A, Bm = make(M, N, Kd, g)
    ref = A.double() @ Bm.double().t()
    kw = dict(kw)
    if layout == "TN":                       # C = A'^T B' with A' = A^T [K, M], B' = B^T [K, N]; split_k > 1 adds into C
        dA, dB, out = A.t().contiguous().to(DEV), Bm.t().contiguous().to(DEV), torch.zeros(M, N, device=DEV)
        args = (dA, dB, out, M, N, Kd, M, N, N, False, False)
    else:
        dA, dB, out = A.to(DEV), Bm.to(DEV), torch.full((M, N), float("nan"), device=DEV)
        args = (dA, dB, out, M, N, Kd, Kd, Kd, N, True, True)
    if kw.pop("planes", False):
        kw["a_planes"], kw["b_planes"] = K.split_planes([dA, dB])
    route = K.gemm_route(*args, **kw)
    assert route.kind == kind, route
    K.gemm(*args, **kw)
    torch.cuda.synchronize()
    assert _sk_error_word() == 0
    err, scale = float((out.double().cpu() - ref).abs().max()), float(ref.abs().max())
    print(f"{kind}: max |err| vs fp64 {err:.3e} (|ref| max {scale:.3e}, bound {bound(scale):.3e})")
    if kind in ("x6", "x6tn"):
        assert scale < 2 ** 24
    assert err <= bound(scale), (err, bound(scale))


@pytest.mark.parametrize("kind,M,N,Kd,kw", [("vec64", 70, 50, 32, {}), ("vec128", 2048, 2048, 64, dict(bf16_split=0, use_sk=False))],
                         ids=["vec64", "vec128"])
def test_pointer_vec_route_kinds_run_an_operand_beyond_the_buffer_window(kind, M, N, Kd, kw):
    """The 16-byte pointer-load tile kernels take aligned operands that a 2 GiB buffer window does not cover: A is a view with the
    smallest leading dimension (a multiple of 4) for which (M * lda + K) * 4 >= 0x7FFF0000 - about 2.2 GB of uninitialised storage of
    which only the M rows used are written.  Route kind first, then the product against float64 under test_gemm_nt's bound; printed:
    whether the result is bit-equal to the buffer kernel's on a compact copy of the same operands."""
    g = torch.Generator().manual_seed(43)
    A, Bm = _route_unit(M, N, Kd, g)
    ref = A.double() @ Bm.double().t()
    lda = -(-(0x7FFF0000 // 4 - Kd) // M)            # ceil((0x7FFF0000 / 4 - K) / M) ...
    lda += -lda % 4                                   # ... rounded up to a multiple of 4
    assert (M * lda + Kd) * 4 >= 0x7FFF0000 > (M * (lda - 4) + Kd) * 4
    store = torch.empty((M - 1) * lda + Kd, device=DEV)
    dA = store.as_strided((M, Kd), (lda, 1))
    dA.copy_(A)
    dB, out = Bm.to(DEV), torch.full((M, N), float("nan"), device=DEV)
    args = (store, dB, out, M, N, Kd, lda, Kd, N, True, True)
    route = K.gemm_route(*args, **kw)
    assert route.kind == kind, route
    K.gemm(*args, **kw)
    compact, out_c = dA.contiguous(), torch.full((M, N), float("nan"), device=DEV)
    args_c = (compact, dB, out_c, M, N, Kd, Kd, Kd, N, True, True)
    kind_c = K.gemm_route(*args_c, **kw).kind
    K.gemm(*args_c, **kw)
    torch.cuda.synchronize()
    del store, dA
    err, scale = float((out.double().cpu() - ref).abs().max()), float(ref.abs().max())
    bound = 2e-6 * max(1, Kd / 16) * max(1.0, scale)
    print(f"{kind}: max |err| vs fp64 {err:.3e} (|ref| max {scale:.3e}, bound {bound:.3e}); bit-equal to {kind_c} on a compact copy: "
          f"{torch.equal(out, out_c)}")
    assert err <= bound, (err, bound)


def _view_cases():
    """name -> (base tensor shapes, lambda bases: (A, B, C) views): the layout classes of tests/test_gemm_views_cpu.py at B = 2, H = 2,
    T = 37, d_h = 8 (no multiple of a tile, more than one batch of each level)"""
    B, H, T, dh = 2, 2, 37, 8
    Cc, C3, Hh, hop, nfft, nre, F = H * dh, 3 * H * dh, 8, 4, 16, 18, 9

    def heads(x, parts=1):
        return x.view(x.shape[0], x.shape[1], parts, H, dh).permute(2, 0, 3, 1, 4).unbind(0)
    return {
        "2d_rowA_colB": (dict(a=(T, 11), w=(13, 11), c=(T, 13)), lambda t: (t["a"], t["w"].t(), t["c"])),
        "2d_colA_rowB": (dict(a=(11, T), b=(11, 13), c=(T, 13)), lambda t: (t["a"].t(), t["b"], t["c"])),
        "3d": (dict(a=(B, T, 11), b=(B, 11, 13), c=(B, T, 13)), lambda t: (t["a"], t["b"], t["c"])),
        "4d_QKt_offsets": (dict(qkv=(B, T, C3), c=(B, H, T, T)),
                           lambda t: (heads(t["qkv"], 3)[0], heads(t["qkv"], 3)[1].transpose(-1, -2), t["c"])),
        "4d_dV_into_a_slice": (dict(p=(B, H, T, T), do=(B, T, Cc), c=(B, T, C3)),
                               lambda t: (t["p"].transpose(-1, -2), heads(t["do"])[0], heads(t["c"], 3)[2])),
        "4d_dK_into_a_slice": (dict(p=(B, H, T, T), qkv=(B, T, C3), c=(B, T, C3)),
                               lambda t: (t["p"].transpose(-1, -2), heads(t["qkv"], 3)[0], heads(t["c"], 3)[1])),
        "expanded_batch": (dict(qv=(B, T, Cc), pos=(T, Cc), c=(B, H, T, T)),
                           lambda t: (heads(t["qv"])[0], heads(t["pos"].unsqueeze(0))[0].expand(B, H, T, dh).transpose(-1, -2), t["c"])),
        "size1_M": (dict(a=(B, 1, T), g=(B, T, Cc), c=(B, 1, Cc)), lambda t: (t["a"], t["g"], t["c"])),
        "2d_column_slices": (dict(dgh=(B * T, 2 * 3 * Hh), hp=(B * T, 2 * Hh), c=(2, 3 * Hh, Hh)),
                             lambda t: (t["dgh"][:, 3 * Hh:].t(), t["hp"][:, Hh:], t["c"][1])),
        "as_strided_frames": (dict(y=(B, (F - 1) * hop + nfft), basis=(nre, nfft), c=(B * F, nre)),
                              lambda t: (t["y"].as_strided((B, F, nfft), ((F - 1) * hop + nfft, hop, 1)),
                                         t["basis"].t().expand(B, nfft, nre), t["c"].view(B, F, nre))),
    }


@pytest.mark.parametrize("case", list(_view_cases()))
def test_bgemm_on_views_equals_float64_einsum_and_writes_only_the_view(case):
    """kernels.bgemm on device views of every layout class.  Operands are integers in [-64, 64] and K <= 74: every product and partial
    sum is an integer below 2^19, exact in fp32 on every kernel family, so the result EQUALS the float64 einsum of the views; the
    output's base tensor starts as NaN and is still NaN wherever the view does not reach."""
    shapes, views = _view_cases()[case]
    g = torch.Generator().manual_seed(len(case))
    host = {n: torch.randint(-64, 65, s, generator=g).float() for n, s in shapes.items()}
    host["c"] = torch.full(shapes["c"], float("nan"))
    dev = {n: t.to(DEV) for n, t in host.items()}
    A, Bv, Cv = views(dev)
    assert K.bgemm(A, Bv, Cv) is Cv
    torch.cuda.synchronize()
    hA, hB, _ = views(host)
    ref = torch.einsum("...mk,...kn->...mn", hA.double(), hB.double())
    got = dev["c"].cpu()
    written = torch.zeros(shapes["c"], dtype=torch.bool)
    views(dict(host, c=written))[2].fill_(True)
    assert torch.equal(views(dict(host, c=got))[2].double(), ref.expand(Cv.shape))
    assert ref.abs().max() > 0 and bool(torch.isnan(got[~written]).all()) and int(written.sum()) == Cv.numel()
