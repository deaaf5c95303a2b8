"""float64 numpy restatement of the reference's STFT / Griffin-Lim (audio/stft.py:22-134, audio/audio_processing.py:7-82) at the
shipped sizes (filter_length 1024, hop 256, win_length 1024, periodic hann): the oracle of tests/test_griffinlim_*.py at sizes no fixture
holds.  Same reflect padding, the inverse basis pinv(scale F)^T window = window * irfft / scale (irfft drops the imaginary parts of bins 0
and 512 like the pseudo-inverse does), overlap-add, division by the window sum-square where it exceeds tiny(float32), * n_fft / hop,
crop n_fft/2 at both ends.  Also the seeded inputs of the g19 fixture (tests/golden/make_goldens_griffinlim.py)."""
import numpy as np
import torch
import torch.nn.functional as TF

NFFT, HOP, NB = 1024, 256, 513
TINY32 = float(np.finfo(np.float32).tiny)


def hann():
    n = np.arange(NFFT)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * n / NFFT)


def window_sumsquare(n_frames):
    w2 = hann() ** 2
    x = np.zeros(NFFT + HOP * (n_frames - 1))
    for f in range(n_frames):
        x[f * HOP:f * HOP + NFFT] += w2
    return x


def transform(x):
    """x [B,N] -> (magnitude, phase) [B,513,F], F = 1 + N // 256"""
    x = np.asarray(x, dtype=np.float64)
    B, N = x.shape
    p = np.pad(x, ((0, 0), (NFFT // 2, NFFT // 2)), mode="reflect")
    F = 1 + N // HOP
    idx = np.arange(F)[:, None] * HOP + np.arange(NFFT)[None, :]
    X = np.fft.rfft(p[:, idx] * hann(), axis=-1)              # [B,F,513]
    return np.abs(X).transpose(0, 2, 1), np.angle(X).transpose(0, 2, 1)


def inverse(mag, phase):
    """(magnitude, phase) [B,513,F] -> [B,1,256 (F - 1)]"""
    mag, phase = np.asarray(mag, dtype=np.float64), np.asarray(phase, dtype=np.float64)
    X = (mag * np.cos(phase) + 1j * mag * np.sin(phase)).transpose(0, 2, 1)
    fr = np.fft.irfft(X, n=NFFT, axis=-1) * hann() / (NFFT / HOP)
    B, F, _ = fr.shape
    n = NFFT + HOP * (F - 1)
    blocks = np.zeros((B, F + 3, HOP))                       # overlap-add: quarter j of frame f lands on hop block f + j
    for j in range(NFFT // HOP):
        blocks[:, j:j + F] += fr[:, :, j * HOP:(j + 1) * HOP]
    out = blocks.reshape(B, n)
    wss = window_sumsquare(F)
    nz = wss > TINY32
    out[:, nz] /= wss[nz]
    out *= NFFT / HOP
    return out[:, None, NFFT // 2:n - NFFT // 2]


def griffin_lim(mag, angles, n_iters):
    signal = inverse(mag, angles)[:, 0]
    for _ in range(n_iters):
        _, angles = transform(signal)
        signal = inverse(mag, angles)[:, 0]
    return signal


def seeded_angles(shape, seed):
    """the reference's initial phase (audio_processing.py:74-75) after np.random.seed(seed), as float32"""
    np.random.seed(seed)
    return np.angle(np.exp(2j * np.pi * np.random.rand(*shape))).astype(np.float32)


class StockSTFT:
    """the reference STFT restated on stock torch ops at float32 (conv1d / conv_transpose1d against the dense [1026 x 1024] windowed
    bases, stft.py:32-127, written as the same GEMMs with unfold / fold: MIOpen searches and compiles a convolution kernel for every new
    signal length, minutes for a batch of ragged utterances): the baseline of tools/bench_griffinlim.py and, in the GPU tests, the measure of the reference algorithm's own
    float32 error on a given input"""

    def __init__(self, dev):
        X = np.fft.rfft(np.eye(NFFT), axis=0)                 # [513, 1024]: exp(-2 pi i k n / 1024)
        fb = np.concatenate([X.real, X.imag])                  # rows: real parts, then imaginary parts
        win = torch.from_numpy(hann().astype(np.float32))
        self.fwd = (torch.FloatTensor(fb[:, None, :]) * win).to(dev)
        self.inv = (torch.FloatTensor(np.linalg.pinv(NFFT / HOP * fb).T[:, None, :]) * win).to(dev)
        self.wss = {}
        self.dev = dev

    def transform(self, x):
        x = TF.pad(x.unsqueeze(1).unsqueeze(1), (NFFT // 2, NFFT // 2, 0, 0), mode="reflect").squeeze(1).squeeze(1)
        t = torch.matmul(x.unfold(-1, NFFT, HOP), self.fwd[:, 0, :].t()).transpose(1, 2)        # = F.conv1d(x, fwd, stride=HOP)
        re, im = t[:, :513], t[:, 513:]
        return torch.sqrt(re ** 2 + im ** 2), torch.atan2(im, re)

    def inverse(self, mag, phase):
        nf = mag.size(-1)
        n = NFFT + HOP * (nf - 1)
        cols = torch.matmul(self.inv[:, 0, :].t(), torch.cat([mag * torch.cos(phase), mag * torch.sin(phase)], dim=1))
        y = TF.fold(cols, output_size=(1, n), kernel_size=(1, NFFT), stride=(1, HOP)).view(mag.size(0), 1, n)   # = F.conv_transpose1d
        if nf not in self.wss:
            w = window_sumsquare(nf).astype(np.float32)
            idx = torch.from_numpy(np.where(w > np.finfo(np.float32).tiny)[0]).to(self.dev)
            self.wss[nf] = (idx, torch.from_numpy(w).to(self.dev)[idx])
        idx, w = self.wss[nf]
        y[:, :, idx] /= w
        y *= float(NFFT) / HOP
        return y[:, :, NFFT // 2:-(NFFT // 2)]

    def griffin_lim(self, mag, angles, n):
        s = self.inverse(mag, angles)[:, 0]
        for _ in range(n):
            s = self.inverse(mag, self.transform(s)[1])[:, 0]
        return s


def speechlike_magnitude(F, seed):
    """[1, 513, F] float32: |STFT| (float64 restatement) of a seeded harmonic signal with a wandering pitch - a consistent spectrogram,
    on which Griffin-Lim is far better conditioned than on random magnitudes"""
    rs = np.random.RandomState(seed)
    N = HOP * (F - 1)
    t = np.arange(N) / 22050.0
    f0 = rs.uniform(90, 180) + 40 * np.sin(2 * np.pi * rs.uniform(0.5, 2) * t + rs.uniform(0, 6))
    ph = 2 * np.pi * np.cumsum(f0) / 22050.0
    y = sum(np.sin(h * ph) / h for h in range(1, 30)) * (0.5 + 0.5 * np.sin(2 * np.pi * 3 * t) ** 2)
    m, _ = transform((0.1 * y + 0.01 * rs.standard_normal(N))[None])
    return m.astype(np.float32)


# ---- the inputs of tests/golden/g19_griffinlim.npz (the fixture stores outputs only)
GL_ITERS = (0, 1, 4, 60)
INV_FRAMES = (4, 5, 87)
GL_SEED, INVMEL_SEED = 196, 198


def g19_signal():
    """[1, 4000] float32: a few partials + noise, peak ~0.6 (F = 16 frames)"""
    rs = np.random.RandomState(190)
    t = np.arange(4000) / 22050.0
    y = sum(a * np.sin(2 * np.pi * f * t + p) for a, f, p in zip(rs.uniform(0.05, 0.2, 5), rs.uniform(80, 4000, 5), rs.uniform(0, 6, 5)))
    y = y + 0.02 * rs.standard_normal(4000)
    return y[None, :].astype(np.float32)


def g19_inverse_inputs(F):
    rs = np.random.RandomState(191 + F)
    mag = (rs.rand(1, NB, F) * (1.0 / (1.0 + np.arange(NB) / 40.0))[None, :, None]).astype(np.float32)
    phase = rs.uniform(-np.pi, np.pi, (1, NB, F)).astype(np.float32)
    return mag, phase


def g19_gl_magnitude():
    """[1, 513, 32] float32 target magnitude with a decaying spectral envelope"""
    rs = np.random.RandomState(195)
    env = 2.0 / (1.0 + np.arange(NB) / 30.0)
    return (rs.rand(1, NB, 32) * env[None, :, None]).astype(np.float32)


def g19_mel():
    """[80, 33] float32 log-mel for inv_mel_spec"""
    rs = np.random.RandomState(197)
    return (rs.standard_normal((80, 33)) * 0.8 - 5.0).astype(np.float32)


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))
