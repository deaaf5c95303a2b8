"""Plain-torch restatement of the glue kernels between the GEMMs - csrc/lr.hip (length-regulator index, gather and its segment-sum
gradient, positions, embedding lookup and its weight gradient) and the backward / reduction half of csrc/elementwise.hip
(rowscale_dropout, act_dropout_bwd, epilogue_bwd, colsum, weighted_colsum, posembed forward / backward, partial_sums) - the oracle of
tests/test_glue_kernels_gpu.py (run in float64; the same code in float32 is the stock-torch yardstick the tests print).

Written from the kernel headers and include/ctts.h: host tensors, plain index arithmetic, no product code.  tests/test_glue_restate_cpu.py
pins every function against a stock torch composition (repeat_interleave / cumsum / searchsorted, F.embedding and autograd) and shows
that the inputs built here tell a subtly wrong model from the right one.  Where a result is a sum the function also returns the L2
norm of the float64 summands plus |old| of an accumulating call (`*_norm`), the scale a rounding error of that sum is measured against.

The dropout mask is tests/gemm_restate64.keep_mask (element index row * C + c of the flat [rows, C] tensor); a kept element is scaled
by the float32 constant fl32(1 / (1 - fl32(p))) the kernels compute, in every dtype: it is part of the operation, not a rounding of it.
The order of the float32 multiplications is the kernels' own, so that a float32 run of these functions is bit-comparable where the
kernels promise bit identity: rowscale_dropout (x * drop) * rowscale, posembed forward ((x + alpha * pe) * drop) * rowscale, the
backward kernels (dy * rowscale) * drop."""
import numpy as np
import torch

from tests.gemm_restate64 import act_grad, keep_mask

F64 = torch.float64
INT32_MAX = 2 ** 31 - 1
DUR_CAP = 2_000_000_000


def _sq(t):
    return t * t


# ------------------------------------------------------------------------------------------------ dropout
def drop_scale(seed_u64, drop_offset, p, rows, C, dtype=F64):
    """[rows, C]: 0 where element row * C + c is dropped, fl32(1 / (1 - p)) where it is kept; all ones for p = 0"""
    if not p > 0:
        return torch.ones(rows, C, dtype=dtype)
    idx = np.arange(rows * C, dtype=np.uint64).reshape(rows, C)
    inv_keep = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    return keep_mask(seed_u64, drop_offset, p, idx).to(dtype) * inv_keep


def _rs(rowscale, rows, dtype):
    return torch.ones(rows, 1, dtype=dtype) if rowscale is None else rowscale.to(dtype).reshape(rows, 1)


# ------------------------------------------------------------------------------------------------ length regulator
def durations(dur, pad=None, round_mode=0):
    """int64 [B,Ts]: float durations are truncated, or rounded half-to-even when round_mode is set; <= 0, -0.0 and NaN give 0, anything
    above 2e9 (+inf included) gives 2e9; int64 durations: <= 0 gives 0, above 2e9 gives 2e9; pad != 0 gives 0"""
    if dur.dtype.is_floating_point:
        f = dur.to(torch.float32).double()
        r = torch.round(f) if round_mode else torch.trunc(f)            # torch.round: half to even
        d = torch.where(r > 0, r.clamp(max=float(DUR_CAP)), torch.zeros_like(r)).to(torch.int64)      # NaN > 0 is False
    else:
        v = dur.to(torch.int64)
        d = torch.where(v > 0, v.clamp(max=DUR_CAP), torch.zeros_like(v))
    if pad is not None:
        d = torch.where(pad.reshape(d.shape) != 0, torch.zeros_like(d), d)
    return d


def lr_index(dur, Tm, pad=None, round_mode=0):
    """-> (mel2ph int32 [B,Tm], mel_len int64 [B], cum int32 [B,Ts]): prefix_i = d_0 + .. + d_i in int64 (at most Ts * 2e9, exact);
    mel_len = prefix_{Ts-1}; cum = min(prefix, 2^31 - 1); mel2ph[t] = 1 + #{i : prefix_i <= t} for t < min(mel_len, Tm), else 0"""
    d = durations(dur, pad, round_mode)
    B, Ts = d.shape
    prefix = torch.zeros(B, Ts, dtype=torch.int64)
    run = torch.zeros(B, dtype=torch.int64)
    for i in range(Ts):
        run = run + d[:, i]
        prefix[:, i] = run
    mel_len = prefix[:, -1].clone()
    t = torch.arange(Tm, dtype=torch.int64)
    count = (prefix[:, None, :] <= t[None, :, None]).sum(-1)
    mel2ph = torch.where(t[None, :] < mel_len[:, None].clamp(max=Tm), 1 + count, torch.zeros_like(count))
    return mel2ph.to(torch.int32), mel_len, prefix.clamp(max=INT32_MAX).to(torch.int32)


def lr_gather(x, mel2ph, dtype=F64):
    """x [B,Ts,C], mel2ph [B,Tm] -> out[b,t] = x[b, mel2ph[b,t] - 1], zeros where mel2ph is 0"""
    x = x.to(dtype)
    B, Tm = mel2ph.shape
    out = x.new_zeros(B, Tm, x.shape[2])
    for b in range(B):
        for t in range(Tm):
            ph = int(mel2ph[b, t])
            if ph > 0:
                out[b, t] = x[b, ph - 1]
    return out


def lr_gather_grad(dy, cum, dtype=F64):
    """dy [B,Tm,C], cum int32 [B,Ts] -> (dx [B,Ts,C], dx_norm): dx[b,i] = sum of dy[b,t] over the frame run [cum[i-1], min(cum[i], Tm))
    of phoneme i, frame after frame"""
    dy = dy.to(dtype)
    B, Tm, C = dy.shape
    Ts = cum.shape[1]
    dx, sq = dy.new_zeros(B, Ts, C), torch.zeros(B, Ts, C, dtype=F64)
    for b in range(B):
        for i in range(Ts):
            start = int(cum[b, i - 1]) if i > 0 else 0
            for t in range(start, min(int(cum[b, i]), Tm)):
                dx[b, i] += dy[b, t]
                sq[b, i] += _sq(dy[b, t].double())
    return dx, sq.sqrt()


def positions(src, stride=1):
    """src int [B,T], or float [B,T,stride] of which channel 0 is tested -> int32 [B,T]: the running count of non-zero entries at the
    non-zero entries (NaN counts as non-zero, -0.0 as zero), 0 at the zeros"""
    v = src if src.dim() == 2 else src[..., 0]
    assert src.dim() == 2 or src.shape[2] == stride
    nz = (v != 0).to(torch.int64)
    B, T = nz.shape
    pos = torch.zeros(B, T, dtype=torch.int64)
    run = torch.zeros(B, dtype=torch.int64)
    for t in range(T):
        run = run + nz[:, t]
        pos[:, t] = run * nz[:, t]
    return pos.to(torch.int32)


# ------------------------------------------------------------------------------------------------ embedding
def embedding(ids, weight, dtype=F64):
    """ids int64 [...], weight [V,C] -> [...,C]; an id outside [0, V) gives a zero row"""
    w = weight.to(dtype)
    V = w.shape[0]
    ok = (ids >= 0) & (ids < V)
    return w[ids.clamp(0, V - 1)] * ok[..., None].to(dtype)


def embedding_grad(ids, dy, V, padding_idx=-1, old=None, dtype=F64):
    """ids int64 [n], dy [n,C] -> (dw [V,C], dw_norm): row v = (old[v] +) the sum of dy[p] over ids[p] == v, position after position; an
    id outside [0, V) contributes nothing; the padding_idx row is zero (without old) or stays old[padding_idx]"""
    dy = dy.to(dtype)
    ids = ids.reshape(-1)
    ok = (ids >= 0) & (ids < V) & (ids != padding_idx)
    s = dy.new_zeros(V, dy.shape[1]).index_add_(0, ids[ok], dy[ok])
    norm = torch.zeros(V, dy.shape[1], dtype=F64).index_add_(0, ids[ok], _sq(dy[ok].double())).sqrt()
    if old is None:
        return s, norm
    return old.to(dtype) + s, norm + old.double().abs()


# ------------------------------------------------------------------------------------------------ positional embedding
def posembed(x, pos, table, alpha, rowscale, drop, dtype=F64):
    """x [rows,C], pos int [rows], table [n_pos,C], alpha a number or None (= 1), rowscale [rows] or None, drop = drop_scale(...)
    -> y = rowscale[row] * (drop * (x + alpha * table[pos[row]])), the product alpha * table rounded before the sum"""
    x, pe = x.to(dtype), table.to(dtype)[pos.long()]
    a = torch.ones((), dtype=dtype) if alpha is None else torch.as_tensor(alpha).to(dtype).reshape(())
    return ((x + a * pe) * drop.to(dtype)) * _rs(rowscale, x.shape[0], dtype)


def posembed_grad(dy, pos, table, rowscale, drop, old_alpha=None, dtype=F64):
    """-> (dx = (dy * rowscale) * drop, dalpha [1] = (old +) sum over all elements of dx * table[pos], dalpha_norm [1])"""
    dy, pe = dy.to(dtype), table.to(dtype)[pos.long()]
    dx = (dy * _rs(rowscale, dy.shape[0], dtype)) * drop.to(dtype)
    terms = dx * pe
    dalpha, norm = terms.sum().reshape(1), _sq(terms.double()).sum().sqrt().reshape(1)
    if old_alpha is not None:
        dalpha, norm = old_alpha.to(dtype).reshape(1) + dalpha, norm + old_alpha.double().abs().reshape(1)
    return dx, dalpha, norm


# ------------------------------------------------------------------------------------------------ elementwise backward
def rowscale_dropout(x, rowscale, drop, dtype=F64):
    """x [rows,C] -> (x * drop) * rowscale[row]"""
    x = x.to(dtype)
    return (x * drop.to(dtype)) * _rs(rowscale, x.shape[0], dtype)


def act_dropout_bwd(dg, z, act, drop, dtype=F64):
    """-> (dz = (dg * drop) * act'(z), scale = |dg * drop|, what an error of act' is multiplied by)"""
    g = dg.to(dtype) * drop.to(dtype)
    return g * act_grad(z.to(dtype), act), g.double().abs()


def epilogue_bwd(dy, rowscale, z, act, drop, bias_scale=1.0, old_bias=None, dtype=F64):
    """backward of y = rowscale * (R + drop(act(z))): gm = dy * rowscale; dz = (gm * drop) * act'(z) (act 0: no z); dbias = (old +)
    bias_scale * column sums of dz.  -> dict(gm, dz, dz_scale = |gm * drop|, dbias, dbias_norm)"""
    dy = dy.to(dtype)
    gm = dy * _rs(rowscale, dy.shape[0], dtype)
    g = gm * drop.to(dtype)
    dz = g * act_grad(z.to(dtype), act) if act else g
    dbias, norm = colsum(dz, scale=bias_scale, old=old_bias, dtype=dtype)
    return dict(gm=gm, dz=dz, dz_scale=g.double().abs(), dbias=dbias, dbias_norm=norm)


def colsum(x, scale=1.0, old=None, dtype=F64):
    """x [rows,C] (any view: a column slice of a wider matrix is the `ld` case) -> (out[c] = (old[c] +) scale * sum_r x[r,c], out_norm)"""
    x = x.to(dtype)
    out, norm = scale * x.sum(0), abs(scale) * _sq(x.double()).sum(0).sqrt()
    if old is not None:
        out, norm = old.to(dtype) + out, norm + old.double().abs()
    return out, norm


def weighted_colsum(x, w, scale=1.0, old=None, dtype=F64):
    """-> (out[c] = (old[c] +) scale * sum_r w[r] * x[r,c], out_norm)"""
    return colsum(x.to(dtype) * w.to(dtype).reshape(-1, 1), scale, old, dtype)


def partial_sums(dst, src, count, stride, n, alpha, dtype=F64):
    """dst [n], src flat -> (dst[i] + alpha * sum_{s < count} src[s * stride + i], norm = |alpha| * L2 over s + |dst|)"""
    src = src.to(dtype).reshape(-1)
    acc, sq = src.new_zeros(n), torch.zeros(n, dtype=F64)
    for s in range(count):
        part = src[s * stride:s * stride + n]
        acc = acc + part
        sq = sq + _sq(part.double())
    return dst.to(dtype) + alpha * acc, abs(alpha) * sq.sqrt() + dst.double().abs()


# ------------------------------------------------------------------------------------------------ inputs of the GPU tests
LR_B = 3
LR_TS = (1, 63, 64, 65, 128, 129, 200)
FLOAT_SPECIALS = (0.5, 1.5, 2.5, -3.0, -0.0, float("nan"))


def _gen(*key):
    seed = 17
    for k in key:
        seed = (seed * 1000003 + int(k)) % 2147483629
    return torch.Generator().manual_seed(seed)


def lr_int_durations(Ts, seed=0, big=False):
    """int64 [3,Ts]: row 0 random 0 .. 7 (never 0 in total) with a negative entry and zeros across elements 62 .. 66; row 1 all
    zeros; row 2 a single non-zero, at element 64 (at the last element where Ts <= 64): 5, or 3e9 (above the cap) with `big`"""
    d = torch.zeros(LR_B, Ts, dtype=torch.int64)
    d[0] = torch.randint(0, 8, (Ts,), generator=_gen(1, Ts, seed))
    d[0, 0] = 3
    if Ts > 2:
        d[0, 2] = -3
    d[0, 62:67] = 0
    d[2, min(64, Ts - 1)] = 3_000_000_000 if big else 5
    return d


def lr_float_durations(Ts, seed=0):
    """float32 [3,Ts]: random durations in [0, 6) with fractions; row 0 starts with 2.25, 0.5, 1.5, 2.5, -3.0, -0.0, NaN (as many as
    fit) and has zeros across 62 .. 66; row 1 holds 2.0e9 in the middle; row 2 ends with the specials reversed and one +inf as its last
    element.  No row holds two capped durations: every total stays below 2^31."""
    d = torch.rand(LR_B, Ts, generator=_gen(2, Ts, seed)) * 6.0
    sp = torch.tensor((2.25,) + FLOAT_SPECIALS)
    k = min(len(sp), Ts)
    d[0, :k] = sp[:k]
    d[0, 62:67] = 0.0
    d[1, Ts // 2] = 2.0e9
    d[2, Ts - k:] = sp[:k].flip(0)
    d[2, Ts - 1] = float("inf")
    return d


def lr_pad(Ts, seed=0):
    """uint8 [3,Ts]: about a quarter of the durations padded away, element 0 of row 0 kept"""
    pad = (torch.rand(LR_B, Ts, generator=_gen(3, Ts, seed)) < 0.25).to(torch.uint8)
    pad[0, 0] = 0
    return pad


def lr_tm_set(total):
    """Tm around the total of row 0, the smallest, and two past the 256-thread search loop"""
    return sorted({1, max(1, total - 1), max(1, total), total + 1, 257, 600})


def lr_overflow_durations():
    """([1,65] int64, [1,65] float32): 2e9 / +inf at elements 3 and 64 - a total of 4e9, past 2^31"""
    di = torch.zeros(1, 65, dtype=torch.int64)
    di[0, 3] = di[0, 64] = DUR_CAP
    df = torch.zeros(1, 65)
    df[0, 3] = df[0, 64] = float("inf")
    return di, df


def gather_durations(B, Ts, seed=0, long_run=0):
    """int64 [B,Ts] durations 0 .. 6 with at least one phoneme of 0 frames between two of several; long_run: one phoneme of that many"""
    d = torch.randint(0, 7, (B, Ts), generator=_gen(4, B, Ts, seed))
    d[:, 0] = 2
    if Ts > 2:
        d[:, Ts // 2] = 0
        d[:, Ts // 2 - 1] = 4
        d[:, Ts // 2 + 1] = 3
    if long_run:
        d[0, min(Ts - 1, 7)] = long_run
    return d


def positions_int_input(T):
    """int64 [4,T]: ids 1 .. 50 with zeros at the 64-lane chunk boundaries; an all-zero row; negative ids; a row that starts with zeros"""
    s = torch.randint(1, 51, (4, T), generator=_gen(5, T))
    for t in (0, 62, 63, 64, 65, 127, 128, 129):
        if t < T and t != 0:
            s[0, t] = 0
    s[1] = 0
    s[2] = -s[2]
    s[2, T // 2] = 0
    s[3, :min(T, 3)] = 0
    return s


def positions_float_input(T, C=3):
    """float32 [3,T,C]: channel 0 is zero at the chunk boundaries while the other channels are not; row 1 holds -0.0 (zero) and NaN
    (non-zero) in channel 0; row 2 has channel 0 all zero and the others non-zero"""
    x = torch.rand(3, T, C, generator=_gen(6, T)) + 0.5
    for t in (63, 64, 65, 128):
        if t < T:
            x[0, t, 0] = 0.0
    x[1, ::3, 0] = -0.0
    x[1, 1::5, 0] = float("nan")
    x[2, :, 0] = 0.0
    return x


def embedding_ids(n, V, kind="mixed", seed=0):
    """int64 [n]: `mixed` = random ids of [0, V) except V // 2, which never occurs, with -1, V and V + 3 strewn in (n >= 8);
    `equal` = every id 1"""
    if kind == "equal":
        return torch.full((n,), 1, dtype=torch.int64)
    ids = torch.randint(0, V - 1, (n,), generator=_gen(7, n, V, seed))
    ids = ids + (ids >= V // 2).to(torch.int64)
    if n >= 8:
        ids[1::97] = -1
        ids[3::101] = V
        ids[5::89] = V + 3
    return ids


def randn(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=_gen(8, seed, *shape)) * scale


def act_z(rows, C, seed=0):
    """[rows,C]: a random body (sigma 2) with exact 0, +-1e-3 and +-20 written over its first entries"""
    z = randn(rows, C, seed=seed + 100, scale=2.0)
    sp = torch.tensor([0.0, 1e-3, -1e-3, 20.0, -20.0])
    flat = z.view(-1)
    k = min(len(sp), flat.numel())
    flat[:k] = sp[:k]
    if flat.numel() >= 2 * len(sp):
        flat[-len(sp):] = sp
    return z


def rowscale_input(rows, seed=0):
    """[rows]: a 0 / 1 non-pad mask times a per-row factor; about a third of the rows are zero"""
    g = _gen(9, rows, seed)
    return (torch.rand(rows, generator=g) > 0.33).float() * (0.5 + torch.rand(rows, generator=g))


# ------------------------------------------------------------------------------------------------ shapes of the GPU tests
GATHER_FWD_CASES = [(2, 21, 4), (2, 21, 8), (2, 21, 256)]             # (B, Ts, C); each with Tm inside a run and Tm beyond the total
GATHER_FWD_LOOP = (2, 400, 1024, 1100)                                # (B, Ts, C, Tm): 2 * 1100 * 256 float4 > 2048 * 256
GATHER_BWD_TS = 65
POSITIONS_T = (1, 63, 64, 65, 130)
EMB_V = 9
EMB_N = (1, 63, 64, 65, 4032, 4095, 4096, 16385)                      # 4032 = 63 chunks: the last n with one group
EMB_C = (4, 64, 68, 256, 260, 512)
DROP_P = (0.0, 0.1, 0.5)
DROP_C = (1, 2, 11, 4, 64, 200)
DROP_ROWS = 37
DALPHA_SHAPES = [(1, 4), (16, 64), (70, 256)]                         # rows * C / 4 = 1, 256, 4480
EPI_ROWS = (1, 31, 32, 33, 100, 600)                                  # 100 rows = 3 stripes, one ticket level
EPI_C = (11, 200)
COLSUM_NARROW_C = (1, 2, 3, 5, 32)
COLSUM_ROWS = (64 * 17, 64 * 17 + 1, 96, 1000)
COLSUM_WIDE_C = (64, 65, 1000)


def gather_fwd_tms(dur):
    """(Tm that cuts row 0's phoneme Ts // 2 - 1 (4 frames) in the middle, Tm beyond every total)"""
    prefix = dur.cumsum(1)
    return int(prefix[0, dur.shape[1] // 2 - 1]) - 2, int(prefix[:, -1].max()) + 5


def colsum_fold(rows, C, ld=None):
    """the fold factor k of ctts_colsum's immediate mode: a dense [rows, C] is read as [rows / k, k * C], k the largest power of two
    with k * C <= 64 that divides rows"""
    k = 1
    if ld is None or ld == C:
        while C * k * 2 <= 64 and rows % (k * 2) == 0:
            k *= 2
    return k


def psum_tasks():
    """25 tasks (n, count, stride, dst_off) of one flush: a task over two workgroups, the scalar paths (a destination one float into
    its buffer, a stride that is no multiple of 4, a tail of fewer than 4), and counts 1, 7, 8, 9 in turn"""
    tasks = [(8200, 7, 8200, 0), (37, 9, 40, 1), (38, 8, 38, 0), (39, 9, 40, 0)]
    for t in range(4, 25):
        n = 64 + t
        tasks.append((n, (1, 7, 8, 9)[t % 4], (n + 3) // 4 * 4, (t // 4) % 2))      # every count on the aligned and on the scalar path
    return tasks
