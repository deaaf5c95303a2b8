"""float64 restatement of ctts_gemm_desc (include/ctts.h) in plain index arithmetic - no project kernel, no F.conv1d, no bmm: the oracle of
tests/test_gemm_contract_gpu.py, pinned against torch compositions by tests/test_gemm_restate_cpu.py.

`restate` takes HOST tensors and the keyword names of kernels._gemm_desc and returns what the flat C buffer (and Z, and split_out) must
hold after the launch, starting from what they held before: a cell the launch must not write keeps its initial value, so comparing whole
buffers is the guard-cell check.  `written` masks say which cells the contract lets the launch store to.

Rules the header leaves to the kernels are written where they are restated (and into the header's comment):
  - a conv view needs a dense operand, ld == conv_cin: element (row, kk) is X[(row - conv_pad) * ld + kk];
  - bias, R, Z and rowscale are not batched: every batch reads R[m * ldr + n], rowscale[m] and stores Z[m * ldz + n];
  - E is addressed like C WITHOUT the offset that went into the C pointer; rowsub is [batch * M + row] with the descriptor's M;
  - the dropout element index is batch * M * N + m * N + n with the descriptor's M and N, wrapping at 2^32;
  - split_k > 1 takes no epilogue term (alpha only);
  - padded rows: only whole tiles are skipped, so the operands must make every padded row's result zero (`restate` raises if they do
    not): output rows (a_kc = 1) then hold zero whichever tile they fall into, reduction rows (TN) of A are zero."""
import collections

import numpy as np
import torch

from tests.attention_restate import _G, _M32, ctts_drop_key, ctts_mix32

Restated = collections.namedtuple("Restated", "C Z split_out written_C written_Z written_split dropped_C")
F64 = torch.float64


def keep_mask(seed_u64, drop_offset, p, idx):
    """bool, shaped like `idx` (element indices, any integer array): kept iff mix32(idx * G + key) >= ceil(p * 2^24) << 8, p as float32"""
    key = ctts_drop_key(seed_u64, drop_offset)
    i = np.asarray(idx).astype(np.uint64) & _M32
    h = ctts_mix32((i * _G + key) & _M32)
    thr = np.uint64(int(np.ceil(float(np.float32(p)) * 16777216.0)) << 8)
    return torch.from_numpy(np.asarray(h >= thr))


def act(v, code):
    if code == 1:
        return torch.where(v > 0, v, torch.zeros_like(v))
    if code == 2:
        return 0.5 * v * (1.0 + torch.special.erf(v * 0.70710678118654752440))
    if code == 3:
        return torch.tanh(v)
    if code == 4:
        return v * torch.sigmoid(v)
    return v


def act_grad(z, code):
    if code == 1:
        return (z > 0).to(z.dtype)
    if code == 2:
        return 0.5 * (1.0 + torch.special.erf(z * 0.70710678118654752440)) + z * 0.39894228040143267794 * torch.exp(-0.5 * z * z)
    if code == 3:
        return 1.0 - torch.tanh(z) ** 2
    if code == 4:
        s = torch.sigmoid(z)
        return s * (1.0 + z * (1.0 - s))
    return torch.ones_like(z)


def split_ranges(K, split_k, granule):
    """[(k_begin, k_end)] of the non-empty pieces of a split: equal chunks of ceil(K / split_k) rounded up to the granule"""
    chunk = -(-(-(-K // split_k)) // granule) * granule
    return [(k, min(k + chunk, K)) for k in range(0, K, chunk)]


def _flat(t):
    return None if t is None else t.detach().cpu().reshape(-1).to(F64)


def _ints(t):
    return None if t is None else [int(v) for v in torch.as_tensor(t).cpu().reshape(-1)]


def _padded(rows, lens, T, halo):
    """bool [len(rows)]: row (b, t), t = row % T, is padding: t >= lens[b] + halo"""
    L = torch.tensor(lens, dtype=torch.int64)
    return rows % T >= L[rows // T] + halo


def operand_a(a, base, ld, kc, Mv, Kv, conv=None):
    """opA [Mv, Kv] gathered from the flat buffer: A[m * ld + k] (kc) or A[k * ld + m]; conv = (T, pad, cin): the im2col view on A"""
    m, k = torch.arange(Mv)[:, None], torch.arange(Kv)[None, :]
    if conv is None:
        return a[base + (m * ld + k if kc else k * ld + m)]
    T, pad, cin = conv
    assert kc and ld == cin, "conv view on A: K-contiguous dense rows (ld == conv_cin)"
    t = m % T - pad + k // cin
    ok = (t >= 0) & (t < T)
    idx = base + (m - pad) * ld + k
    return torch.where(ok, a[torch.where(ok, idx, torch.zeros_like(idx))], torch.zeros((), dtype=F64))


def operand_b(b, base, ld, kc, Kv, Nv, conv=None):
    """opB [Kv, Nv]: B[n * ld + k] (kc) or B[k * ld + n]; conv: the im2col view on B (TN: reduction rows are (b, t), columns (tap, channel))"""
    k, n = torch.arange(Kv)[:, None], torch.arange(Nv)[None, :]
    if conv is None:
        return b[base + (n * ld + k if kc else k * ld + n)]
    T, pad, cin = conv
    assert not kc and ld == cin, "conv view on B: reduction-major dense rows (ld == conv_cin)"
    t = k % T - pad + n // cin
    ok = (t >= 0) & (t < T)
    idx = base + (k - pad) * ld + n
    return torch.where(ok, b[torch.where(ok, idx, torch.zeros_like(idx))], torch.zeros((), dtype=F64))


def restate(A, B, C, M, N, K, lda, ldb, ldc, a_kc=True, b_kc=True, a_off=0, b_off=0, c_off=0, nb0=1, nb1=1, sA=(0, 0), sB=(0, 0),
            sC=(0, 0), lens=None, lim=(0, 0, 0), conv=None, conv_on_b=False, split_k=1, alpha=1.0, bias=None, Z=None, ldz=0, act_code=0,
            p_drop=0.0, seed=None, drop_offset=0, R=None, ldr=0, rowscale=None, row_lens=None, row_T=0, row_halo=0, E=None, rowsub=None,
            epi_bwd=False, split_overwrite=False, split_out=None, split_plan=None, k_granule=32, **unused):
    """Expected buffers of one ctts_gemm launch.  `act_code` is the descriptor's `act` (also accepted under that name); split_out (the
    initial contents) with split_plan = (count, stride) and the route's k_granule restates a deferred split-K launch: the partial
    matrices are written, C is left alone."""
    act_code = int(unused.pop("act", act_code))
    a, b = _flat(A), _flat(B)
    c = _flat(C).clone()
    z_io = _flat(Z)
    z_out = z_io.clone() if z_io is not None else None
    w_c = torch.zeros(c.numel(), dtype=torch.bool)
    w_z = torch.zeros(z_out.numel(), dtype=torch.bool) if z_out is not None else None
    s_out = _flat(split_out).clone() if split_out is not None else None
    w_s = torch.zeros(s_out.numel(), dtype=torch.bool) if s_out is not None else None
    dropped = torch.zeros(c.numel(), dtype=torch.bool)        # cells whose dropout decision is "dropped": their value has no rounding
    bias64, r64, rs64, e64, sub64 = _flat(bias), _flat(R), _flat(rowscale), _flat(E), _flat(rowsub)
    lens_l, rl = _ints(lens), _ints(row_lens)
    a_kc, b_kc, epi_bwd, split_overwrite = bool(a_kc), bool(b_kc), bool(epi_bwd), bool(split_overwrite)
    tn = not a_kc and not b_kc
    conv_a = tuple(conv) if conv is not None and not conv_on_b else None
    conv_b = tuple(conv) if conv is not None and conv_on_b else None
    assert a_kc or not b_kc, "layout a_kc = 0, b_kc = 1 does not exist"
    if split_k > 1:
        assert bias is None and Z is None and act_code == 0 and p_drop == 0 and R is None and rowscale is None and E is None and not epi_bwd
    seed64 = None if seed is None else int(torch.as_tensor(seed).reshape(-1)[0]) & 0xFFFFFFFFFFFFFFFF
    inv_keep = 1.0 / (1.0 - float(np.float32(p_drop)))
    for z0 in range(nb0):
        Mv, Nv, Kv = M, N, K
        if lens_l is not None:
            Mv = min(M, lens_l[z0]) if lim[0] else M
            Nv = min(N, lens_l[z0]) if lim[1] else N
            Kv = min(K, lens_l[z0]) if lim[2] else K
        limited = lens_l is not None and any(lim)
        for z1 in range(nb1):
            zi = z0 * nb1 + z1
            opA = operand_a(a, a_off + z0 * sA[0] + z1 * sA[1], lda, a_kc, Mv, Kv, conv_a)
            opB = operand_b(b, b_off + z0 * sB[0] + z1 * sB[1], ldb, b_kc, Kv, Nv, conv_b)
            if rl is not None and tn:
                pad_k = _padded(torch.arange(Kv), rl, row_T, row_halo)
                if bool((opA[:, pad_k] != 0).any()):
                    raise ValueError("TN launch with row_lens: the padded reduction rows of A must be zero (the caller's duty)")
            c0 = c_off + z0 * sC[0] + z1 * sC[1]
            m, n = torch.arange(Mv)[:, None], torch.arange(Nv)[None, :]
            cidx = c0 + m * ldc + n
            full = c0 + torch.arange(M)[:, None] * ldc + torch.arange(N)[None, :]
            pad_m = _padded(torch.arange(Mv), rl, row_T, row_halo)[:, None] if (rl is not None and a_kc) else None

            def zero_padded_rows(v):
                if pad_m is None:
                    return v
                if bool((torch.where(pad_m, v, torch.zeros_like(v)) != 0).any()):
                    raise ValueError("row_lens: the operands must make the result of every padded row zero (only whole tiles are skipped)")
                return torch.where(pad_m, torch.zeros_like(v), v)

            if split_k > 1 and s_out is not None:          # deferred: P_s [M, N rounded up to 4], `stride` floats apart, alpha = 1
                count, stride = split_plan
                ranges = split_ranges(Kv, split_k, k_granule)
                assert len(ranges) == count and nb0 * nb1 == 1 and not limited
                ldp = -(-N // 4) * 4
                for s, (k0, k1) in enumerate(ranges):
                    pidx = s * stride + m * ldp + n
                    s_out[pidx] = opA[:, k0:k1] @ opB[k0:k1]
                    w_s[pidx] = True
                continue
            acc = opA @ opB
            if split_k > 1:
                v = zero_padded_rows(alpha * acc)
                if split_overwrite:                        # "write everything": the whole [M, N] block, zero outside the limits
                    c[full] = 0.0
                    w_c[full] = True
                    c[cidx] = v
                else:
                    c[cidx] = c[cidx] + v
                    w_c[cidx] = True
                continue
            if limited and split_overwrite:
                c[full] = 0.0
                w_c[full] = True
            if E is not None:
                v = e64[cidx - c_off] * (alpha * acc - sub64[zi * M + m])
            elif epi_bwd:
                v = alpha * acc
                if p_drop > 0:
                    keep = keep_mask(seed64, drop_offset, p_drop, zi * M * N + m * N + n)
                    dropped[cidx] = ~keep
                    v = v * keep * inv_keep
                if act_code:
                    v = v * act_grad(z_io[m * ldz + n], act_code)
                v = zero_padded_rows(v)
            else:
                v = alpha * (acc + (bias64[n] if bias64 is not None else 0.0))
                if z_out is not None:
                    z_out[m * ldz + n] = zero_padded_rows(v)
                    w_z[m * ldz + n] = True
                v = act(v, act_code)
                if p_drop > 0:
                    keep = keep_mask(seed64, drop_offset, p_drop, zi * M * N + m * N + n)
                    dropped[cidx] = ~keep
                    v = v * keep * inv_keep
                if r64 is not None:
                    v = v + r64[m * ldr + n]
                if rs64 is not None:
                    v = v * rs64[m]
                v = zero_padded_rows(v)
            c[cidx] = v
            w_c[cidx] = True
    return Restated(c, z_out, s_out, w_c, w_z, w_s, dropped)
