"""Float64 model of ONE vocoder layer call (include/ctts.h ctts_vocoder_conv / ctts_vocoder_conv_h / ctts_vocoder_post*), written from
the operation's definition - a helper of tests/test_vocoder_layer_restate_cpu.py and tests/test_vocoder_contract_gpu.py, not a test.

  Conv1d(k, dil)            out[t] = sum_tap a[t + (tap - (k - 1) / 2) dil] @ W[:, :, tap].T            (shifted matmuls, zero padding)
  ConvTranspose1d(k, u)     out[q u - pad + j] += a[q] @ W[:, :, j],  pad = (k - u) / 2                  (the scatter definition)
  operand                   a = leaky_relu(x, slope) (slope None: a = x); half=True: fp16(leaky_relu(float32(x))), saturated
  epilogue                  beta * old + alpha * (acc + bias + R); beta == 0 never reads old
  lengths                   utterance b has Tb = min(max(lens[b], 0) len_mul, T) input rows and is computed ALONE from x[b, :Tb]: nothing
                            beyond Tb is ever touched (NaN there cannot reach the result); output rows from Tb u (Conv1d: Tb) on are
                            "not stored": the returned mask is False and the returned values NaN there
  mag                       sum |a| |w| + |bias| + |R|: what the rounding bounds of the tests scale with

Nothing here uses the polyphase form of the kernels or the reshape of kernels.vocoder_pack_weight.  The second half of the file is the
opposite: `geometry` restates vc_geometry's formulas (csrc/vocoder_common.h) and `walk` replays the kernels' index walk - packed weight,
tap shift, phase scatter - in float64 with "stored once" bookkeeping.  The CPU test holds the two against each other."""
import numpy as np
import torch

FP16_MAX = 65504.0
HALO_MAX = 64                      # VC_HALO_MAX

# the geometry lists of the contract tests: ConvTranspose1d (k, u) and Conv1d (k, dil)
KU = [(2, 2), (3, 3), (8, 8),                    # one tap, pad = 0, mextra = 0
      (1, 1), (3, 1), (5, 1),                    # u = 1: row_off = pad
      (4, 2), (16, 8),                           # k = 2u: V1's own path, the control
      (6, 2), (12, 4), (9, 3),                   # k = 3u: row_off = 1, mextra = 0, three taps
      (8, 2), (16, 4),                           # k = 4u: row_off = 1, mextra = 1, four taps
      (10, 2), (15, 3), (24, 4),                 # row_off = 2
      (130, 2)]                                  # 65 taps: the halo is exactly 64
KD = [(1, 1), (3, 1), (3, 32), (5, 16), (9, 8), (17, 4), (65, 1), (7, 3)]          # five of them on halo = 64


def slope32(slope):
    """the slope as the kernels hold it: a float"""
    return float(np.float32(slope))


def operand(x, slope, half=False):
    """the MFMA operand of x [.., Cin] in float64.  half: fp16(leaky_relu(float32(x), slope)) saturated to +-65504, as the fp16 mode
    stages it (the product with the slope is rounded to float32 first); otherwise leaky_relu in float64 with the float slope."""
    if half:
        x32 = x.float()
        if slope is not None:
            x32 = torch.where(x32 > 0, x32, x32 * slope)
        return x32.clamp(-FP16_MAX, FP16_MAX).half().double()
    a = x.double()
    return a if slope is None else torch.where(a > 0, a, a * slope32(slope))


def rows_of(lens, b, len_mul, T):
    """input rows of utterance b: min(max(lens[b], 0) len_mul, T); lens None: T"""
    return T if lens is None else min(max(int(lens[b]), 0) * int(len_mul), T)


def _conv1d(a, w, dil):
    """a [B, T, Cin], w [Cout, Cin, k] float64 -> [B, T, Cout]: tap by tap, out[t] += a[t + (tap - (k - 1) / 2) dil] @ W[:, :, tap].T"""
    B, T, k = a.shape[0], a.shape[1], w.shape[2]
    out = torch.zeros(B, T, w.shape[0], dtype=torch.float64, device=a.device)
    for tap in range(k):
        s = (tap - (k - 1) // 2) * dil                  # out[t] reads a[t + s]
        lo, hi = max(0, -s), min(T, T - s)
        if lo < hi:
            out[:, lo:hi] += a[:, lo + s:hi + s] @ w[:, :, tap].t()
    return out


def _conv_transpose1d(a, w, u):
    """a [B, T, Cin], w [Cin, Cout, k] float64 -> [B, T u, Cout] by the scatter definition out[q u - pad + j] += a[q] @ W[:, :, j]"""
    B, T, k = a.shape[0], a.shape[1], w.shape[2]
    pad = (k - u) // 2
    out = torch.zeros(B, T * u, w.shape[1], dtype=torch.float64, device=a.device)
    q = torch.arange(T, device=a.device)
    for j in range(k):
        to = q * u - pad + j
        ok = (to >= 0) & (to < T * u)
        if ok.any():
            out[:, to[ok]] += a[:, ok] @ w[:, :, j]     # one j: the targets of different q are different rows
    return out


def conv_layer(x, w, dil=1, u=0, slope=None, bias=None, R=None, old=None, alpha=1.0, beta=0.0, lens=None, len_mul=1, half=False):
    """One ctts_vocoder_conv / ctts_vocoder_conv_h call.  x [B, T, Cin] (any dtype), w Conv1d [Cout, Cin, k] or (u > 0) ConvTranspose1d
    [Cin, Cout, k] - for the fp16 mode the caller passes the fp16-rounded weight - bias [Cout], R / old [B, Tout, Cout].
    -> (out, mag, stored): out float64 [B, Tout, Cout], NaN where not stored; mag likewise; stored bool [B, Tout]."""
    B, T, _ = x.shape
    w = w.double()
    cout = w.shape[1] if u else w.shape[0]
    Tout = T * u if u else T
    out = torch.full((B, Tout, cout), float("nan"), dtype=torch.float64, device=x.device)
    mag = torch.full_like(out, float("nan"))
    stored = torch.zeros(B, Tout, dtype=torch.bool, device=x.device)
    # dense: the utterances share their length, one pass; ragged: utterance by utterance, each from its own rows alone
    for sel, Tb in ([(slice(0, B), T)] if lens is None else [(slice(b, b + 1), rows_of(lens, b, len_mul, T)) for b in range(B)]):
        n = Tb * u if u else Tb
        if n == 0:
            continue
        a = operand(x[sel, :Tb], slope, half)
        if u:
            acc, m = _conv_transpose1d(a, w, u), _conv_transpose1d(a.abs(), w.abs(), u)
        else:
            acc, m = _conv1d(a, w, dil), _conv1d(a.abs(), w.abs(), dil)
        if bias is not None:
            acc, m = acc + bias.double(), m + bias.double().abs()
        if R is not None:
            acc, m = acc + R[sel, :n].double(), m + R[sel, :n].double().abs()
        acc = alpha * acc
        if beta != 0.0:
            acc = beta * old[sel, :n].double() + acc
        out[sel, :n], mag[sel, :n], stored[sel, :n] = acc, m, True
    return out, mag, stored


def conv_post(x, w, bias, slope=0.01, lens=None, len_mul=1):
    """ctts_vocoder_post / _post_ragged / _post_h: x [B, T, C] (fp32 or fp16 values), w [k, C], bias [1].
    -> (pre, mag, wav) float64 [B, T]: pre = bias + sum_{tap, c} leaky_relu(x[t + tap - (k - 1) / 2, c]) w[tap, c] on the utterance's own
    Tb rows (NaN from Tb on: nothing is defined there), mag = sum |a||w| + |bias|, wav = tanh(pre) with exact zeros from Tb on."""
    B, T, C = x.shape
    wc = w.double().t().reshape(1, C, -1)               # the Conv1d weight [1, C, k]
    pre = torch.full((B, T), float("nan"), dtype=torch.float64, device=x.device)
    mag = torch.full_like(pre, float("nan"))
    wav = torch.zeros_like(pre)
    for sel, Tb in ([(slice(0, B), T)] if lens is None else [(slice(b, b + 1), rows_of(lens, b, len_mul, T)) for b in range(B)]):
        if Tb == 0:
            continue
        a = operand(x[sel, :Tb], slope)
        pre[sel, :Tb] = _conv1d(a, wc, 1)[:, :, 0] + bias.double()
        mag[sel, :Tb] = _conv1d(a.abs(), wc.abs(), 1)[:, :, 0] + bias.double().abs()
        wav[sel, :Tb] = torch.tanh(pre[sel, :Tb])
    return pre, mag, wav


# ---- the kernels' own index walk -------------------------------------------------------------------------------------------------
def geometry(T, k, dil=1, u=0):
    """vc_geometry's formulas (csrc/vocoder_common.h) -> dict(taps, dil, in_off, row_off, Mrows, mextra, u, pad), or None where
    vc_geometry refuses the layer (even k, k % u, (k - u) odd, halo above 64)"""
    if u == 0:
        if k % 2 == 0 or dil < 1:
            return None
        g = dict(taps=k, dil=dil, in_off=-((k - 1) * dil // 2), row_off=0, Mrows=T, u=0, pad=0)
    else:
        if k % u or (k - u) % 2:
            return None
        pad, J = (k - u) // 2, k // u
        qlo, qhi = pad // u, T + (pad + u - 1) // u
        g = dict(taps=J, dil=1, in_off=-(J - 1), row_off=qlo, Mrows=qhi - qlo, u=u, pad=pad)
    g["mextra"] = g["Mrows"] - T
    return g if (g["taps"] - 1) * g["dil"] <= HALO_MAX else None


def walk(a, packed, cin, cout, taps, dil, in_off, row_off, Mrows, mextra, u, pad, lens=None, len_mul=1):
    """The kernels' walk in float64.  a [B, T, Cin]: the operand (already activated); packed [roundup(N, 128), taps x roundup(Cin, 32)]:
    kernels.vocoder_pack_weight's result.  GEMM row m of utterance b is position p = row_off + m (m < Mb = Tb + mextra); tap `tap` reads
    input row p + in_off + tap dil (zero outside [0, Tb)) against packed[n, tap cin_pad + c]; column n = ph cout + co of row p goes to
    output row p u + ph - pad (Conv1d: p) if that lies in [0, Tb u) (Conv1d: [0, Tb)).
    -> (out [B, Tout, Cout] float64, zeros where nothing was stored; count [B, Tout, Cout]: how often each element was stored)."""
    B, T, _ = a.shape
    assert Mrows == T + mextra
    N = u * cout if u else cout
    cpad = -(-cin // 32) * 32
    assert tuple(packed.shape) == (-(-N // 128) * 128, taps * cpad)
    wk = packed.double().reshape(-1, taps, cpad)
    assert not wk[N:].any() and not wk[:, :, cin:].any()         # the padding of the pack holds zeros
    Tout = T * u if u else T
    out = torch.zeros(B, Tout, cout, dtype=torch.float64, device=a.device)
    count = torch.zeros(B, Tout, cout, dtype=torch.int64, device=a.device)
    for b in range(B):
        Tb = rows_of(lens, b, len_mul, T)
        Mb, Toutb = Tb + mextra, (Tb * u if u else Tb)
        if Tb == 0:
            continue
        p = row_off + torch.arange(Mb, device=a.device)
        acc = torch.zeros(Mb, N, dtype=torch.float64, device=a.device)
        for tap in range(taps):
            ti = p + in_off + tap * dil
            ok = (ti >= 0) & (ti < Tb)
            rows = torch.zeros(Mb, cin, dtype=torch.float64, device=a.device)
            rows[ok] = a[b, ti[ok]].double()
            acc += rows @ wk[:N, tap, :cin].t()
        for n in range(N):
            ph, co = (n // cout, n % cout) if u else (0, n)
            to = p * u + ph - pad if u else p
            ok = (to >= 0) & (to < Toutb)
            out[b, to[ok], co] = acc[ok, n]
            count[b, to[ok], co] += 1
    return out, count
