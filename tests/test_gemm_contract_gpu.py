"""GPU: every GEMM route against the float64 restatement of the descriptor (tests/gemm_restate64.py) on the case table of
tests/gemm_cases.py.  Per case: ctts_gemm_route names the kind the case was written for, the launch runs, and the WHOLE C, Z and split_out
buffers - guard rows in front and behind, guard columns between N and the leading dimension, the gaps between batches - are compared:
cells outside the written set bit-equal to their index-dependent sentinel, cells inside equal to float64 (exact recipe) or inside the
family's own bound (random recipe).  Dropped elements under dropout must be exactly what the host mask says.  The stream-K error word of
the workspace must stay 0.  No case skips.

Measured on the MI355X (one run of this file; per kind: cases, largest error / bound over the random cases): profiles/gemm_contract_gpu.md."""
import time

import pytest
import torch

import ctts_amd  # noqa: F401
from ctts_amd import kernels as K
from tests import gemm_cases as G
from tests import gemm_restate64 as R64

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _sk_error_word():
    ws = K.gemm_workspace(torch.device(DEV))
    return int(ws.view(torch.int32)[2048].item())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check(name, got, init, exp, written, exact, bound, dropped=None):
    """got / init float32 flat (device result, initial contents), exp float64, written bool.  -> (max error, bound) of a random case"""
    got = got.detach().cpu().reshape(-1)
    assert got.numel() == init.numel() == exp.numel() == written.numel(), name
    untouched = ~written
    same = _bits(got)[untouched] == _bits(init)[untouched]
    if not bool(same.all()):
        bad = torch.nonzero(untouched)[~same].reshape(-1)
        raise AssertionError(f"{name}: {bad.numel()} cells outside the written set changed, first flat indices {bad[:8].tolist()}")
    g64, e = got.double()[written], exp[written]
    assert bool(torch.isfinite(g64).all()), f"{name}: non-finite values written"
    if e.numel() == 0:
        return 0.0, 0.0
    scale = float(e.abs().max())
    if exact:
        assert scale < 2 ** 24, (name, scale)
        ne = g64 != e
        if bool(ne.any()):
            bad = torch.nonzero(written)[ne].reshape(-1)
            raise AssertionError(f"{name}: {bad.numel()} of {e.numel()} written cells differ from float64, first flat indices "
                                 f"{bad[:8].tolist()}, max |diff| {float((g64 - e).abs().max())}")
        return 0.0, 0.0
    if dropped is not None and bool(dropped.any()):                  # the mask itself is exact: dropped cells carry no rounding
        d = dropped[written]
        assert bool((g64[d] == e[d]).all()), f"{name}: dropped elements differ from the host mask's"
    err = float((g64 - e).abs().max())
    if bound is None:
        return err, None
    b = bound(scale)
    assert err <= b, f"{name}: max |err| {err:.3e} above the bound {b:.3e} (|ref| max {scale:.3e})"
    return err, b


def _launch(p, **override):
    """stage on the device, route, launch -> (route, device tensors, split_out info)"""
    args, kw, t = G.device_args(p, DEV)
    kw.update(override)
    route = K.gemm_route(*args, **kw)
    split = None
    if p.defer and not override:
        import ctypes as C
        from ctts_amd import _lib
        plan = G.split_plan_of(args, kw)
        assert plan is not None, "the split plan refuses a launch the table lists as deferrable"
        count, stride = plan
        P0 = G._sentinel(route.split_k * stride + 64, 5)
        t["P"] = P0.to(DEV)
        d = K._gemm_desc(*args, **kw)
        d.split_out, d.split_out_floats = t["P"].data_ptr(), route.split_k * stride
        _lib.check(_lib.load().ctts_gemm(C.byref(d), K._stream()), "ctts_gemm")
        split = (P0, count, stride)
    else:
        K.gemm(*args, **kw)
    torch.cuda.synchronize()
    return route, t, split


@pytest.mark.parametrize("case", G.CASES, ids=[c.id for c in G.CASES])
def test_gemm_contract(case):
    t0 = time.time()
    p = G.build(case)
    exact = case.recipe == "exact"
    route, t, split = _launch(p)
    assert route.kind == case.kind, route
    assert _sk_error_word() == 0
    rargs, rkw = G.restate_args(p)
    if split is not None:
        rkw.update(split_out=split[0], split_plan=split[1:], k_granule=route.k_granule)
    exp = R64.restate(*rargs, **rkw)
    bc, bz = (None, None) if exact else G.bound_of(case)
    vs_fp32 = not exact and bc is None
    err_c, b_c = _check("C", t["C"], p.C, exp.C, exp.written_C, exact, bc, exp.dropped_C)
    err_z = b_z = 0.0
    if "Zfull" in t:
        front = p.Zfull.numel() - p.kw["Z"].numel()
        exp_z = torch.cat([p.Zfull[:front].double(), exp.Z])
        w_z = torch.cat([torch.zeros(front, dtype=torch.bool), exp.written_Z])
        err_z, b_z = _check("Z", t["Zfull"], p.Zfull, exp_z, w_z, exact, bz)
    for name in ("A", "B"):
        assert torch.equal(t[name].cpu(), getattr(p, name)), f"operand {name} was written"
    if "Rfull" in t:
        assert torch.equal(t["Rfull"].cpu(), p.Rfull), "R was written"
    if split is not None:
        P0, count, stride = split
        _check("split_out", t["P"], P0, exp.split_out, exp.written_split, True, None)
        # the caller's half: C_dense += alpha * (P_0 + P_1 + ...) through ctts_partial_sums, on a dense [M, N] accumulation target
        M, N, alpha = p.M, p.N, p.kw["alpha"]
        D0 = G._sentinel(M * N, 6)
        D = D0.to(DEV)
        sink = K.PartialSink()
        sink.add(t["P"], count, stride, M * N, D, alpha)
        sink.flush()
        torch.cuda.synchronize()
        parts = sum(exp.split_out[s * stride:s * stride + M * N] for s in range(count))
        want = D0.double() + alpha * parts
        assert float(want.abs().max()) < 2 ** 24
        assert torch.equal(D.cpu().double(), want), "ctts_partial_sums of the deferred partials"
    if p.want_c_planes:
        got_pl, rows_total = t["c_planes_full"].cpu(), t["C"].numel() // p.ldc
        r0 = p.kw["c_off"] // p.ldc
        if case.kind == "weight_stationary":      # bit-identical to split_planes of the C it wrote, nothing outside the block's K-blocks
            want_pl = K.split_planes([t["C"].view(rows_total, p.ldc)])[0].cpu()
            blk = torch.zeros(rows_total, p.ldc // 32, dtype=torch.bool)
            blk[r0:r0 + p.M, :p.N // 32] = True
            assert torch.equal(got_pl.view(torch.int16)[blk], want_pl.view(torch.int16)[blk]), "C_planes differ from split_planes(C)"
            assert bool((got_pl.view(torch.int16)[~blk] == 0x1234).all()), "C_planes written outside the block"
        else:                                      # every other kernel ignores the field (include/ctts.h)
            assert bool((got_pl.view(torch.int16) == 0x1234).all()), "C_planes written by a kernel that must ignore it"
    if vs_fp32:
        # The bf16-split kernels have no float64 bound of their own for an epilogue term.  x6tn: its own test bounds it by the fp32-MFMA
        # kernels' error on the same launch, e6 <= 2.5 * e32 + 1e-6 (test_bf16_split_weight_gradient_gemm_vs_fp64_...).  x6: twice the
        # error of the existing fp32 path on the same operands against float64 (the fused path rounds in another order) - the fp32-MFMA
        # kernels on the same descriptor are that path.  (x6's own test bounds the PLAIN product of 8192 x 768 x 512 by 1.25 * e32 + 1e-7;
        # measured here on the epilogue cases at K = 288: e6 / e32 between 1.31 and 1.54.)
        route32, t32, _ = _launch(p, bf16_split=0)
        assert route32.kind not in ("x6", "x6tn", "planes", "planes_wgrad"), route32
        e32_c, _ = _check("C (fp32 kernels)", t32["C"], p.C, exp.C, exp.written_C, False, None, exp.dropped_C)
        f, add = (2.0, 0.0) if case.kind == "x6" else (2.5, 1e-6)
        b_c = f * e32_c + add
        assert err_c <= b_c, f"C: max |err| {err_c:.3e} above {f} x the fp32 kernels' {e32_c:.3e} + {add}"
        if "Zfull" in t:
            e32_z, _ = _check("Z (fp32 kernels)", t32["Zfull"], p.Zfull, exp_z, w_z, False, None)
            b_z = f * e32_z + add
            assert err_z <= b_z, f"Z: max |err| {err_z:.3e} above {f} x the fp32 kernels' {e32_z:.3e} + {add}"
    print(f"GEMMCASE {case.kind} {case.id} {case.recipe} errC {err_c:.3e} boundC {b_c or 0.0:.3e} errZ {err_z:.3e} boundZ {b_z or 0.0:.3e} "
          f"route {route.tile_m}x{route.tile_n} split {route.split_k} seconds {time.time() - t0:.2f}")
