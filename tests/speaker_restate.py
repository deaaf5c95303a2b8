"""The float64 statement of the DeepSpeaker speaker embedding (voice span, filterbank features, crop / pad, ResCNN), written from
deepspeaker/audio_ds.py, batcher.py, conv_models.py and embedding.py of the reference, the published definition of
python_speech_features.fbank and Keras / TF layer semantics - and its float32 twin: the same formulas with float32 `torch.fft` and
`F.conv2d` on the CPU, the yardstick of tests/test_speaker_gpu.py (a kernel may differ from float64 by 4 x what the twin differs).
Also the test inputs and the seeded weight recipe.  Pinned by tests/test_speaker_restate_cpu.py.  PARITY with the TF model and
python_speech_features is UNPINNED (neither is installed; the pretrained checkpoint is not available)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

SR, NFILT, NFFT, FRAME, STEP, NUM_FRAMES = 22050, 64, 1024, 551, 221, 160
EPS = float(np.finfo(float).eps)
STAGES = (64, 128, 256, 512)


# ---- 1. voice span -------------------------------------------------------------------------------------------------------------------
def percentile95(a):
    """np.percentile(a, 95) (method 'linear') of a 1-D array, restated: a is taken to float64 exactly, sorted; the virtual index is
    (n - 1) q with q = 95 / 100, k its floor, g the fraction; a[k] + (a[k+1] - a[k]) g, or from
    g = 0.5 on a[k+1] - (a[k+1] - a[k]) (1 - g).  Every operation rounds to double."""
    s = np.sort(np.asarray(a, dtype=np.float64))
    n = len(s)
    q = np.float64(95) / np.float64(100)
    v = np.float64(n - 1) * q
    if v >= n - 1:
        return float(s[-1])
    k = 0 if v < 0 else int(np.floor(v))
    g = np.float64(0) if v < 0 else v - np.floor(v)
    lo, hi = s[k], s[min(k + 1, n - 1)]
    d = hi - lo
    return float(hi - d * (np.float64(1) - g)) if g >= 0.5 else float(lo + d * g)


def span(x, include_last=False):
    """-> (first, last, valid): the lowest / highest index with |x| > the 95th percentile (0, 0 when there is none); the span is
    x[first:last], valid = last - first >= 1.  The comparison is made in double on the float32 samples."""
    a = np.abs(np.asarray(x, dtype=np.float32)).astype(np.float64)
    if len(a) == 0:
        return 0, 0, 0
    idx = np.nonzero(a > percentile95(a))[0]
    if len(idx) == 0:
        return 0, 0, 0
    first, last = int(idx[0]), int(idx[-1])
    if include_last:                    # a WRONG reading, for the sensitivity test
        return first, last + 1, 1
    return first, last, int(last - first >= 1)


def n_frames(L):
    return 0 if L < 1 else (1 if L <= FRAME else 1 + -(-(L - FRAME) // STEP))


# ---- 2. filterbank features ----------------------------------------------------------------------------------------------------------
def hz2mel(hz):
    return 2595.0 * np.log10(1.0 + hz / 700.0)


def mel2hz(mel):
    return 700.0 * (10.0 ** (mel / 2595.0) - 1.0)


def bins():
    return np.floor((NFFT + 1) * mel2hz(np.linspace(hz2mel(0.0), hz2mel(SR / 2.0), NFILT + 2)) / SR).astype(np.int64)


def filterbank():
    """[64, 513] float64"""
    b = bins()
    fb = np.zeros((NFILT, NFFT // 2 + 1))
    for j in range(NFILT):
        for i in range(int(b[j]), int(b[j + 1])):
            fb[j, i] = (i - b[j]) / (b[j + 1] - b[j])
        for i in range(int(b[j + 1]), int(b[j + 2])):
            fb[j, i] = (b[j + 2] - i) / (b[j + 2] - b[j + 1])
    return fb


def fbank(sig, dtype=torch.float64, log=False, hann=False, sample_std=False):
    """sig: the span's samples -> normalised features [frames, 64] in `dtype`.  log / hann / sample_std are WRONG readings."""
    s = torch.as_tensor(np.asarray(sig, dtype=np.float32)).to(dtype)
    L = s.numel()
    y = torch.cat([s[:1], s[1:] - 0.97 * s[:-1]])
    nf = n_frames(L)
    pad = torch.zeros((nf - 1) * STEP + FRAME, dtype=dtype)
    pad[:L] = y
    idx = torch.arange(FRAME)[None, :] + STEP * torch.arange(nf)[:, None]
    frames = pad[idx]
    if hann:
        frames = frames * torch.hann_window(FRAME, periodic=False, dtype=dtype)
    spec = torch.fft.rfft(frames, NFFT)
    p = (spec.real ** 2 + spec.imag ** 2) / NFFT
    feat = p @ torch.as_tensor(filterbank()).to(dtype).T
    feat = torch.where(feat == 0, torch.full_like(feat, EPS), feat)
    if log:
        feat = torch.log(feat)
    m = feat.mean(1, keepdim=True)
    sd = feat.std(1, unbiased=sample_std, keepdim=True)
    return (feat - m) / sd.clamp(min=1e-12)


# ---- 3. crop or pad ------------------------------------------------------------------------------------------------------------------
def crop_pad(fb, r=None, rows=NUM_FRAMES):
    """[frames, 64] -> [rows, 64]: zero rows after a shorter input, [r, r + rows) of a longer one (None: the centre crop)"""
    nf = fb.shape[0]
    if nf >= rows:
        r = (nf - rows) // 2 if r is None else int(r)
        assert 0 <= r <= nf - rows
        return fb[r:r + rows]
    assert r in (None, 0)
    return torch.cat([fb, torch.zeros(rows - nf, fb.shape[1], dtype=fb.dtype)])


# ---- 4. ResCNN -----------------------------------------------------------------------------------------------------------------------
def same_pads(n, k, s, wrong_even=False):
    out = -(-n // s)
    total = max((out - 1) * s + k - n, 0)
    before = total // 2
    if wrong_even and total % 2:        # a WRONG reading: the odd cell in front (k5 s2 on even sizes: (2, 2) cropped to (2, 1))
        before = total - before
    return out, before, total - before


def conv_nhwc(x, w, stride, wrong_even=False):
    """x [B,H,W,Cin], w [kh,kw,Cin,Cout] (Keras) -> [B,Ho,Wo,Cout] with TF 'same' padding: the tap sum written out"""
    B, H, W, Cin = x.shape
    kh, kw, _, Cout = w.shape
    Ho, pt, pb = same_pads(H, kh, stride, wrong_even)
    Wo, pl, pr = same_pads(W, kw, stride, wrong_even)
    xp = torch.zeros(B, H + pt + pb, W + pl + pr, Cin, dtype=x.dtype)
    xp[:, pt:pt + H, pl:pl + W] = x
    out = torch.zeros(B * Ho * Wo, Cout, dtype=x.dtype)
    for i in range(kh):
        for j in range(kw):
            sl = xp[:, i:i + (Ho - 1) * stride + 1:stride, j:j + (Wo - 1) * stride + 1:stride]
            out += sl.reshape(-1, Cin) @ w[i, j]
    return out.view(B, Ho, Wo, Cout)


def conv_twin(x, w, stride):
    """the float32 twin's convolution: F.conv2d on the explicitly padded NCHW input"""
    _, pt, pb = same_pads(x.shape[1], w.shape[0], stride)
    _, pl, pr = same_pads(x.shape[2], w.shape[1], stride)
    xp = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    return F.conv2d(xp, w.permute(3, 2, 0, 1).contiguous(), stride=stride).permute(0, 2, 3, 1).contiguous()


def layer_names():
    out, cin = [], 1
    for stage, c in enumerate(STAGES, 1):
        out.append((f"conv{c}-s", 5, cin, c))
        for block in range(3):
            for branch in ("2a", "2b"):
                out.append((f"res{stage}_{block}_branch_{branch}", 3, c, c))
        cin = c
    return out


def make_weights(seed=20211):
    """Glorot-uniform kernels, bias U(+-0.1), gamma = 2 U(0.5, 1.5), beta U(+-0.5), moving_mean U(+-0.2), moving_variance U(0.5, 1.5):
    with gamma doubled the clipped outputs reach both bounds (tests/test_speaker_restate_cpu.py checks the shares)"""
    rng = np.random.default_rng(seed)
    w = {}

    def u(lo, hi, shape):
        return rng.uniform(lo, hi, shape).astype(np.float32)

    for name, k, cin, cout in layer_names():
        lim = np.sqrt(6.0 / (k * k * cin + k * k * cout))
        w[f"{name}/kernel"] = u(-lim, lim, (k, k, cin, cout))
        w[f"{name}/bias"] = u(-0.1, 0.1, (cout,))
        w[f"{name}_bn/gamma"] = 2.0 * u(0.5, 1.5, (cout,))
        w[f"{name}_bn/beta"] = u(-0.5, 0.5, (cout,))
        w[f"{name}_bn/moving_mean"] = u(-0.2, 0.2, (cout,))
        w[f"{name}_bn/moving_variance"] = u(0.5, 1.5, (cout,))
    lim = np.sqrt(6.0 / (2048 + 512))
    w["affine/kernel"] = u(-lim, lim, (2048, 512))
    w["affine/bias"] = u(-0.1, 0.1, (512,))
    return w


def rescnn(weights, fb, dtype=torch.float64, bn_eps=1e-3, wrong_even=False, feature_order="wc"):
    """fb [B,160,64] -> (embedding [B,512], the four stage outputs NHWC, the 40 clipped outputs).  float64: the tap-sum convolution;
    float32: the twin (F.conv2d).  BatchNorm unfolded, in inference form.  bn_eps / wrong_even / feature_order are WRONG readings."""
    twin = dtype == torch.float32
    W = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in weights.items()}
    clipped = []

    def layer(x, name, stride):
        y = conv_twin(x, W[f"{name}/kernel"], stride) if twin else conv_nhwc(x, W[f"{name}/kernel"], stride, wrong_even)
        y = y + W[f"{name}/bias"]
        y = (y - W[f"{name}_bn/moving_mean"]) / torch.sqrt(W[f"{name}_bn/moving_variance"] + bn_eps) * W[f"{name}_bn/gamma"] + W[f"{name}_bn/beta"]
        y = y.clamp(0, 20)
        clipped.append(y)
        return y

    x = torch.as_tensor(fb).to(dtype)[..., None]
    stages = []
    for stage, c in enumerate(STAGES, 1):
        x = layer(x, f"conv{c}-s", 2)
        for block in range(3):
            y = layer(x, f"res{stage}_{block}_branch_2a", 1)
            y = layer(y, f"res{stage}_{block}_branch_2b", 1)
            x = (y + x).clamp(0, 20)
            clipped.append(x)
        stages.append(x)
    B, T = x.shape[0], x.shape[1]
    feat = x.reshape(B, T, -1) if feature_order == "wc" else x.permute(0, 1, 3, 2).reshape(B, T, -1)
    z = feat.mean(1) @ W["affine/kernel"] + W["affine/bias"]
    emb = z / z.norm(dim=1, keepdim=True).clamp(min=1e-12)
    return emb, stages, clipped


def features(x, dtype=torch.float64, r=None, **wrong):
    """one utterance -> (features [160, 64], first, last, frames, valid); an invalid utterance gives zero features"""
    first, last, valid = span(x, include_last=wrong.pop("include_last", False))
    if not valid:
        return torch.zeros(NUM_FRAMES, NFILT, dtype=dtype), first, last, 0, 0
    fb = fbank(np.asarray(x)[first:last], dtype, **wrong)
    return crop_pad(fb, r), first, last, fb.shape[0], 1


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def speechlike(n, seed):
    """gliding fundamental + harmonics under a syllable envelope, noise in the unvoiced stretches"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / float(SR)
    f = 150.0 + 60.0 * np.sin(2 * np.pi * (0.7 + 0.3 * rng.random()) * t + rng.random() * 6) + 30.0 * np.sin(2 * np.pi * 2.3 * t)
    ph = 2 * np.pi * np.cumsum(f) / float(SR)
    x = sum(np.sin(k * ph) / k for k in range(1, 7))
    env = 0.5 + 0.5 * np.sin(2 * np.pi * 3.1 * t + rng.random() * 6)
    voiced = np.sin(2 * np.pi * 1.3 * t + rng.random() * 6) > -0.5
    return np.clip(np.where(voiced, 0.3 * x * env, 0.02 * rng.standard_normal(n)), -1, 1).astype(np.float32)


def with_span(L, seed, lead=137, tail=211, zeros=None):
    """a signal whose voice span is exactly [lead, lead + L): noise clipped to +-0.9 inside, the two loudest samples (+-1) at its ends,
    and 1 % of that level outside (fewer than 19 x the inside's samples, so the 95th percentile falls inside).  zeros = (a, b): the
    inside samples [a, b) relative to the span are exact zeros."""
    rng = np.random.default_rng(seed)
    n = lead + L + 1 + tail
    assert lead + tail < 10 * (L + 1)
    x = 0.003 * rng.standard_normal(n)
    x[lead:lead + L + 1] = np.clip(0.3 * rng.standard_normal(L + 1), -0.9, 0.9)
    if zeros is not None:
        x[lead + zeros[0]:lead + zeros[1]] = 0.0
    x[lead], x[lead + L] = 1.0, -1.0
    return x.astype(np.float32)


def span_cases():
    """name -> signal, for the exact span test"""
    rng = np.random.default_rng(7)
    sq = np.where((np.arange(4000) // 50) % 2 == 0, 0.5, -0.25).astype(np.float32)      # two levels: ties at the threshold
    sq2 = sq.copy()
    sq2[1000:1100] = 0.75                                                              # 2.5 % above a tied plateau
    loud = np.zeros(3000, np.float32)
    loud[1234] = 0.9
    cases = {f"len{n}": rng.standard_normal(n).astype(np.float32) for n in (1, 2, 20, 21, 30011)}
    cases.update({"square": sq, "square_step": sq2, "zeros": np.zeros(5000, np.float32), "one_loud": loud,
                  "speech": speechlike(30000, 3), "ramp41": (np.arange(41) / 40.0).astype(np.float32)})
    return cases


def fbank_cases():
    """name -> signal: the frame-count edges, a partial last frame, exact-zero frames inside the span"""
    return {"L551": with_span(551, 11), "L552": with_span(552, 12), "L773": with_span(773, 13), "L20011": with_span(20011, 14),
            "zeros_inside": with_span(9000, 15, zeros=(3000, 5000))}


def crop_cases():
    """(name, signal, frames, offsets to try)"""
    out = []
    for nf, L in ((1, 300), (159, 35469), (160, 35690), (161, 35911), (270, 60000)):
        assert n_frames(L) == nf
        offs = sorted({0, max(nf - NUM_FRAMES, 0) // 2, max(nf - NUM_FRAMES, 0)})
        out.append((f"F{nf}", with_span(L, 20 + nf), nf, offs))
    return out


def net_batch():
    """the whole-net batch: a long utterance (cropped), a short one (padded) and an invalid one (zeros)"""
    return [speechlike(52000, 31), speechlike(9000, 32), np.zeros(4000, np.float32)]


@functools.lru_cache(maxsize=None)
def net_reference():
    """float64 and float32-twin results of the whole chain on `net_batch()` with `make_weights()`; computed once per process"""
    w, batch = make_weights(), net_batch()
    out = {}
    for tag, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        feats = [features(x, dtype) for x in batch]
        fb = torch.stack([f[0] for f in feats])
        emb, stages, clipped = rescnn(w, fb, dtype)
        valid = torch.tensor([f[4] for f in feats])
        emb = emb * valid[:, None].to(dtype)
        out[tag] = {"fbank": fb, "embedding": emb, "stages": stages, "clipped": clipped,
                    "first": [f[1] for f in feats], "last": [f[2] for f in feats], "n_frames": [f[3] for f in feats], "valid": [f[4] for f in feats]}
    return out
