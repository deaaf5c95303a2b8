"""Drop-in `TacotronSTFT` (reference: audio/stft.py:137-185) on the gfx950 kernels.

mel_spectrogram(y[B,N] in [-1,1]) -> (mel[B,80,F], energy[B,F]),  F = 1 + N // hop.
For the reference's filter_length = 1024 the whole front end is ONE launch (csrc/mel.hip): a 1024-point real FFT per frame, hann
window and reflect padding folded into the load, |X| + energy in registers, the mel filterbank as a banded fp32-MFMA GEMM,
log-clamp fused.  Other FFT sizes take the DFT-as-GEMM path (the [2*(n_fft/2+1), n_fft] windowed basis the reference feeds
to F.conv1d, stft.py:32-56: rows = real parts then imaginary parts, periodic hann window).

PARITY UNPINNED for one ingredient: the mel filterbank restates the published algorithm of librosa==0.7.2 `filters.mel` (Slaney scale,
area normalisation, htk=False), which the reference pulls from a third-party dependency (requirements.txt:9) that is absent from
/root/reference and from this image.  The golden `tests/golden/g8_stft.npz` was captured from the reference's own `TacotronSTFT`
running on THIS restated basis (oracle/ref_import.py stubs librosa with it), so G8 pins the STFT / magnitude / log arithmetic against
the reference, but not the basis.  What pins the basis is tests/test_mel_basis_cpu.py: the Slaney mel scale against the worked examples
of librosa's own documentation (hz_to_mel / mel_to_hz / mel_frequencies(n_mels=40), all 40 values), and the triangle construction with
the 2 / (f[i+2] - f[i]) area normalisation against its published definition.  Swap in librosa's array (`stft.mel_basis.copy_(...)`,
`stft.set_mel_basis(...)` or `load_state_dict`) where it is available: both paths follow the buffer - what they derive from it (the
highest bin with weight, the padded copy, the FFT kernel's workspace) is rebuilt at the next call (TacotronSTFT._sync_filterbank).

Griffin-Lim (reference audio/stft.py:22-134 `STFT`, audio/audio_processing.py `griffin_lim` / `window_sumsquare` /
`dynamic_range_*`, audio/tools.py:18-34 `inv_mel_spec`): `STFT.transform` / `inverse` and every Griffin-Lim iteration run on
csrc/griffinlim.hip (a 1024-point real FFT per frame; one launch per iteration, plain or with momentum = fast Griffin-Lim; the
initial phase from numpy like the reference, as a tensor, or drawn on the device from a seed).  Supported: filter_length 1024, hop 256,
win_length 1024, hann - an `STFT` of other sizes can be built (so can `TacotronSTFT`), its methods raise.
"""
import math

import numpy as np
import torch
import torch.nn as nn

from . import ops


def _hz_to_mel(f):
    f = np.asanyarray(f, dtype=np.float64)
    f_sp = 200.0 / 3
    min_log_hz, logstep = 1000.0, np.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-10) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asanyarray(m, dtype=np.float64)
    f_sp = 200.0 / 3
    min_log_hz, logstep = 1000.0, np.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def slaney_mel_basis(sr, n_fft, n_mels, fmin, fmax):
    if fmax is None:
        fmax = sr / 2.0
    nb = 1 + n_fft // 2
    fftfreqs = np.linspace(0, sr / 2.0, nb)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fftfreqs)
    w = np.zeros((n_mels, nb))
    for i in range(n_mels):
        w[i] = np.maximum(0, np.minimum(-ramps[i] / fdiff[i], ramps[i + 2] / fdiff[i + 1]))
    w *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]
    return w.astype(np.float32)


def padded_window(n_fft, win_length):
    """scipy get_window('hann', fftbins=True) zero-padded (centred) to n_fft (stft.py:46-50), float32"""
    n = np.arange(win_length)
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / win_length)
    lpad = (n_fft - win_length) // 2
    return np.pad(win, (lpad, n_fft - win_length - lpad)).astype(np.float32)


def windowed_dft_basis(n_fft, win_length):
    """[2*(n_fft/2+1), n_fft]: rows [0,nb) = cos, [nb,2nb) = -sin, times the periodic hann window
    zero-padded (centred) to n_fft - the matrix of audio/stft.py:32-56."""
    nb = n_fft // 2 + 1
    four = np.fft.fft(np.eye(n_fft))
    basis = np.vstack([np.real(four[:nb, :]), np.imag(four[:nb, :])])
    n = np.arange(win_length)
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / win_length)       # scipy get_window('hann', fftbins=True)
    lpad = (n_fft - win_length) // 2
    win = np.pad(win, (lpad, n_fft - win_length - lpad))
    return (basis.astype(np.float32) * win.astype(np.float32)[None, :]).astype(np.float32)


def dynamic_range_compression(x, C=1, clip_val=1e-5):
    """audio_processing.py:85-91: log(clamp(x, clip_val) * C) (elementwise torch, any device - not a hot path)"""
    return torch.log(torch.clamp(x, min=clip_val) * C)


def dynamic_range_decompression(x, C=1):
    """audio_processing.py:94-100: exp(x) / C (elementwise torch, any device)"""
    return torch.exp(x) / C


def window_sumsquare(window, n_frames, hop_length, win_length, n_fft, dtype=np.float32, norm=None):
    """audio_processing.py:7-63 (librosa 0.6's window_sumsquare): the sum-square envelope [n_fft + hop_length (n_frames - 1)] of the
    window at the given hop, a host numpy helper like the reference's.  norm: only None (the reference's default and only use: librosa's
    normalize(norm=None) returns its input).  STFT.inverse does not call it: the kernels sum the same envelope per sample."""
    from scipy.signal import get_window
    if norm is not None:
        raise NotImplementedError("window_sumsquare: only norm=None (what STFT.inverse uses)")
    win_length = n_fft if win_length is None else win_length
    lpad = (n_fft - win_length) // 2
    w2 = np.zeros(n_fft)                                   # squared window, centred in n_fft
    w2[lpad:lpad + win_length] = get_window(window, win_length, fftbins=True) ** 2
    starts = hop_length * np.arange(max(int(n_frames), 0))
    env = np.zeros(max(n_fft + hop_length * (int(n_frames) - 1), 0))
    if len(starts):
        np.add.at(env, starts[:, None] + np.arange(n_fft)[None, :], np.broadcast_to(w2, (len(starts), n_fft)))
    return env.astype(dtype)


def _lens_arg(lens, B, lo, hi, what, dev):
    """per-utterance lengths of a ragged batch: a host sequence (checked against [lo, hi]) or an int32 device tensor (the kernels clamp)"""
    if lens is None:
        return None
    if torch.is_tensor(lens) and lens.is_cuda:
        if lens.numel() != B:                              # the kernels read one length per utterance: no fewer, no more
            raise ValueError(f"{what}: {lens.numel()} lengths for a batch of {B}")
        return lens.to(torch.int32).contiguous().view(B)
    v = [int(n) for n in (lens.tolist() if torch.is_tensor(lens) else lens)]
    if len(v) != B:
        raise ValueError(f"{what}: {len(v)} lengths for a batch of {B}")
    if min(v) < lo or max(v) > hi:
        raise ValueError(f"{what}: lengths must lie in [{lo}, {hi}], got {min(v)} .. {max(v)}")
    return torch.tensor(v, dtype=torch.int32).to(dev)


class STFT(nn.Module):
    """Drop-in `audio.stft.STFT` (stft.py:22-134) on csrc/griffinlim.hip.  transform(x [B,N]) -> (magnitude, phase) [B,513,F],
    F = 1 + N // 256; inverse(magnitude, phase) -> [B,1,256 (F - 1)]; forward = inverse(transform(x)).  Device tensors only.
    Optional `lens` (ragged batches): samples per utterance for transform, frames per utterance for inverse; every utterance gets what a
    B = 1 call on its own slice gives (reflection at its own end); positions past its end are 0."""

    def __init__(self, filter_length, hop_length, win_length, window="hann"):
        super().__init__()
        self.filter_length, self.hop_length, self.win_length, self.window = filter_length, hop_length, win_length, window
        if window is not None:
            assert filter_length >= win_length
        self.supported = (filter_length, hop_length, win_length, window) == (1024, 256, 1024, "hann")
        self.register_buffer("_win", torch.from_numpy(padded_window(filter_length, min(win_length, filter_length))), persistent=False)
        self._ws = None

    def _apply(self, fn, *args, **kwargs):
        # build the kernel workspace (a launch) as soon as the module lands on the device, outside any graph capture
        out = super()._apply(fn, *args, **kwargs)
        self._ws = None
        if self.supported and self._win.is_cuda and not torch.cuda.is_current_stream_capturing():
            from . import kernels as K
            self._ws = K.griffinlim_prepare(self._win)
        return out

    def _workspace(self, t, name):
        if not self.supported:
            raise NotImplementedError(f"STFT (ctts_amd) runs filter_length 1024, hop 256, win_length 1024, hann only; built with "
                                      f"{self.filter_length} / {self.hop_length} / {self.win_length} / {self.window}")
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError(f"STFT (ctts_amd) computes on the MI355X: pass {name} as a device tensor")
        from . import kernels as K
        if self._ws is None or self._ws.device != t.device:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("STFT (ctts_amd): move the module to the device (or call it once) before capturing a graph - its "
                                   "workspace is built by a kernel launch, which a capture would only record")
            if self._win.device != t.device:
                self.to(t.device)                          # builds the workspace (_apply)
            if self._ws is None or self._ws.device != t.device:
                self._ws = K.griffinlim_prepare(self._win)
        return self._ws

    def transform(self, input_data, lens=None):
        from . import kernels as K
        ws = self._workspace(input_data, "input_data")
        B, N = input_data.size(0), input_data.size(1)
        if N <= self.filter_length // 2:
            raise ValueError(f"STFT.transform: reflect padding needs more than {self.filter_length // 2} samples, got {N}")
        self.num_samples = N
        x = input_data.reshape(B, N).float().contiguous()
        return K.stft_transform(x, ws, _lens_arg(lens, B, self.filter_length // 2 + 1, N, "STFT.transform lens", x.device))

    def _frames(self, magnitude, lens, fmin):
        """fmin: 2 for inverse (256 (F - 1) samples out), 4 for Griffin-Lim (its transform needs more than n_fft/2 samples)"""
        B, _, F = magnitude.shape
        if F < fmin:
            raise ValueError(f"STFT (ctts_amd): needs at least {fmin} frames here, got {F}")
        return _lens_arg(lens, B, fmin, F, "frame lens", magnitude.device)

    def inverse(self, magnitude, phase, lens=None):
        from . import kernels as K
        ws = self._workspace(magnitude, "magnitude")
        self._workspace(phase, "phase")
        frames = self._frames(magnitude, lens, 2)
        Y, _ = K.istft_frames(magnitude.float().contiguous(), phase.float().contiguous(), ws, frames)
        return K.istft_ola(Y, ws, frames).unsqueeze(1)

    def forward(self, input_data):
        self.magnitude, self.phase = self.transform(input_data)
        return self.inverse(self.magnitude, self.phase)


def _seed_arg(seed):
    """seed of the device phase: None, a Python int (64 bits, taken modulo 2^64) or a one-element int64 tensor"""
    if seed is None:
        return None
    if torch.is_tensor(seed):
        if seed.dtype != torch.int64 or seed.numel() != 1:
            raise ValueError(f"griffin_lim: a tensor seed must hold one int64, got {seed.dtype} x {seed.numel()}")
        return seed
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise ValueError(f"griffin_lim: seed must be an int or a one-element int64 tensor, got {type(seed).__name__}")
    v = int(seed) & 0xFFFFFFFFFFFFFFFF
    return v - (1 << 64) if v >= (1 << 63) else v


def griffin_lim(magnitudes, stft_fn, n_iters=30, angles=None, lens=None, momentum=0.0, seed=None):
    """audio_processing.py:66-82 on the kernels: magnitudes [B,513,F] (device) -> signal [B, 256 (F - 1)].
    angles=None draws the initial phase from numpy's GLOBAL generator exactly like the reference (np.random.seed(s) reproduces a
    reference run); an explicit device tensor [B,513,F] skips the host draw (and is capturable).  lens: frames per utterance of a ragged
    batch.  Launches: one inverse (frames), one per iteration (csrc/griffinlim.hip gl_iter_kernel, ping-pong frame buffers), one
    overlap-add; no host synchronisation.
    momentum in [0, 1): fast Griffin-Lim (Perraudin et al. 2013; librosa and torchaudio default to 0.99) - the rebuilt spectrum X of an
    iteration is replaced by X - momentum / (1 + momentum) X_prev before its phase is taken; one state buffer per call holds X_prev.
    0.0 is the reference's plain iteration, on the code path it always took.
    seed (a Python int, or a one-element int64 device tensor - capturable, and a replay reads the tensor's value of that moment): the
    initial phase is drawn on the device, theta(b, k, f) = 2 pi u(seed, b, k, f): no host draw, no [B,513,F] angle tensor, and an
    utterance's start does not depend on the batch around it.  Not numpy's stream: np.random.seed does not reproduce it."""
    from . import kernels as K
    if not isinstance(stft_fn, STFT):
        raise TypeError("griffin_lim (ctts_amd): stft_fn must be a ctts_amd.audio.STFT (e.g. TacotronSTFT.stft_fn)")
    momentum = float(momentum)
    if not 0.0 <= momentum < 1.0:                          # NaN fails both comparisons
        raise ValueError(f"griffin_lim: momentum must lie in [0, 1), got {momentum}")
    seed = _seed_arg(seed)
    if seed is not None and angles is not None:
        raise ValueError("griffin_lim: pass either angles (an explicit initial phase) or seed (the device phase), not both")
    ws = stft_fn._workspace(magnitudes, "magnitudes")
    frames = stft_fn._frames(magnitudes, lens, 4)
    mag = magnitudes.float().contiguous()
    if seed is not None:
        if not torch.is_tensor(seed):
            seed = torch.tensor([seed], dtype=torch.int64).to(mag.device)
        elif seed.device != mag.device:
            seed = seed.to(mag.device)
        Y, magT = K.istft_frames_seeded(mag, ws, seed.view(1), frames, want_magT=n_iters > 0)
    else:
        if angles is None:
            angles = np.angle(np.exp(2j * np.pi * np.random.rand(*magnitudes.size())))
            angles = torch.from_numpy(angles.astype(np.float32)).to(magnitudes.device)
        else:
            stft_fn._workspace(angles, "angles")
        Y, magT = K.istft_frames(mag, angles.float().contiguous(), ws, frames, want_magT=n_iters > 0)
    if n_iters > 0:
        Y2 = torch.empty_like(Y)
        if momentum == 0.0:
            for _ in range(n_iters):
                K.griffinlim_iter(Y, magT, ws, Y2, frames)
                Y, Y2 = Y2, Y
        else:
            state = K.griffinlim_state(Y.shape[0], Y.shape[1], Y.device)
            coef = momentum / (1.0 + momentum)
            for i in range(n_iters):
                K.griffinlim_iter_momentum(Y, magT, state, ws, Y2, coef, i == 0, frames)
                Y, Y2 = Y2, Y
    return K.istft_ola(Y, ws, frames)


class TacotronSTFT(nn.Module):
    def __init__(self, filter_length, hop_length, win_length, n_mel_channels, sampling_rate, mel_fmin, mel_fmax):
        super().__init__()
        self.n_fft, self.hop, self.n_mel_channels, self.sampling_rate = filter_length, hop_length, n_mel_channels, sampling_rate
        self.nbins = filter_length // 2 + 1
        mel = slaney_mel_basis(sampling_rate, filter_length, n_mel_channels, mel_fmin, mel_fmax)
        self.register_buffer("mel_basis", torch.from_numpy(mel))
        ld = (self.nbins + 3) // 4 * 4
        padded = np.zeros((n_mel_channels, ld), dtype=np.float32)
        padded[:, :self.nbins] = mel
        self.register_buffer("_mel_basis_padded", torch.from_numpy(padded), persistent=False)
        self.register_buffer("_dft_basis", torch.from_numpy(windowed_dft_basis(filter_length, win_length)), persistent=False)
        self.register_buffer("_window", torch.from_numpy(padded_window(filter_length, win_length)), persistent=False)
        self.stft_fn = STFT(filter_length, hop_length, win_length)      # non-persistent buffers only: state_dict stays ['mel_basis']
        self._fft_ws = None          # device workspace of the FFT kernel (twiddles, transposed filterbank), built on first use
        self.use_fft = filter_length == 1024 and n_mel_channels <= 96
        # what is derived from the filterbank (_kmax, _mel_basis_padded, _fft_ws) follows the `mel_basis` buffer: see _sync_filterbank
        self._basis_key = None
        self._kmax_value = 0
        self._range = None           # range check of the FFT path: (flag in pinned host memory, event of the last launch)
        # strict_range = True (default): the reference's contract - the assertion is raised by the SAME call that was handed the bad
        # waveform (one event wait per call instead of the reference's two reductions + sync).  False: the training / bulk-extraction
        # hot path - the flag is looked at without waiting at the next call, or on demand with check_range() (call it before using the
        # last result).
        self.strict_range = True

    def spectral_normalize(self, magnitudes):
        """stft.py:158-160"""
        return dynamic_range_compression(magnitudes)

    def spectral_de_normalize(self, magnitudes):
        """stft.py:162-164"""
        return dynamic_range_decompression(magnitudes)

    # ---- the reference asserts min(y) >= -1 and max(y) <= 1 on the host before computing (stft.py:177-178): two reductions and a
    # device -> host synchronisation per call, which halves the throughput of a 50 us kernel.  Here the kernel raises a flag while it
    # loads the samples - one word of pinned host memory, written only by an offending input.  By default (strict_range) the call waits
    # for its own launch and raises like the reference; with strict_range = False the flag is looked at, without waiting, at the NEXT
    # call, or on demand with check_range() - same AssertionError, raised one call later at the latest (a single or final
    # call must not return a mel for NaN / out-of-range audio silently, so deferral is opt-in).
    def _range_state(self, dev):
        if self._range is None:
            self._range = (torch.zeros(1, dtype=torch.int32).pin_memory(), torch.cuda.Event())
        return self._range

    def _raise_if_out_of_range(self, wait):
        if self._range is None:
            return
        host, ev = self._range
        if wait:
            ev.synchronize()
        elif not ev.query():
            return
        bits = int(host[0]) & 0xFFFFFFFF
        if bits:
            host.zero_()
            if bits == 0x7FC0004B:                         # include/ctts.h CTTS_MEL_FLAG_KMAX
                raise RuntimeError("TacotronSTFT.mel_spectrogram: the filterbank of the kernel workspace carries weight above the kmax of "
                                   "the launch - the mel rows of those filters are NaN")
            val = np.array([bits], dtype=np.uint32).view(np.float32)[0]
            raise AssertionError(f"TacotronSTFT.mel_spectrogram: waveform outside [-1, 1] (largest |sample| {val})  [audio/stft.py:177-178]")

    def check_range(self):
        """block until the range flag of every mel_spectrogram call issued so far has arrived and raise if a waveform left [-1, 1]"""
        self._raise_if_out_of_range(wait=True)

    def _sync_filterbank(self):
        """`mel_basis` is the module's state: `stft.mel_basis.copy_(array)`, `load_state_dict` and `.to(device)` all change it.  Everything
        derived from it - the highest bin with filter weight (_kmax), the padded copy of the DFT-as-GEMM path and the FFT kernel's
        workspace - is rebuilt here whenever the buffer's (_version, device, data_ptr) differs from the one it was derived from."""
        mel = self.mel_basis
        key = (mel._version, mel.device, mel.data_ptr())
        if key == self._basis_key:
            return
        if mel.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("TacotronSTFT (ctts_amd): call the module once after changing mel_basis (or moving it) before capturing a "
                               "graph - what it derives from the filterbank is rebuilt by kernel launches and a host read, which a "
                               "capture would only record")
        mel = mel.detach()
        if tuple(mel.shape) != (self.n_mel_channels, self.nbins):
            raise ValueError(f"TacotronSTFT: mel_basis must stay [{self.n_mel_channels}, {self.nbins}], got {tuple(mel.shape)}")
        nz = torch.nonzero(mel.abs().sum(0) != 0)          # NaN weights count as weight
        self._kmax_value = int(nz.max()) + 1 if nz.numel() else 0      # bins above fmax carry no filter weight: not kept on chip
        padded = torch.zeros(self.n_mel_channels, (self.nbins + 3) // 4 * 4, dtype=torch.float32, device=mel.device)
        padded[:, :self.nbins] = mel
        self._mel_basis_padded = padded
        self._fft_ws = None                                # rebuilt by _workspace() from the filterbank held now
        self._basis_key = key

    @property
    def _kmax(self):
        """1 + the highest DFT bin that carries filter weight in the CURRENT mel_basis (0: none, the kernel keeps every bin)"""
        self._sync_filterbank()
        return self._kmax_value

    def set_mel_basis(self, basis):
        """replace the filterbank ([n_mel, n_fft/2 + 1] array or tensor, e.g. librosa.filters.mel); the same as mel_basis.copy_(...)"""
        with torch.no_grad():
            self.mel_basis.copy_(torch.as_tensor(np.asarray(basis) if not torch.is_tensor(basis) else basis))
        self._sync_filterbank()

    def _workspace(self):
        from . import kernels as K
        self._sync_filterbank()
        if self._fft_ws is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("TacotronSTFT (ctts_amd): call the module once before capturing a graph - its workspace is built by "
                                   "a kernel launch, which a capture would only record")
            self._fft_ws = K.mel_prepare(self.mel_basis.detach().float().contiguous(), self.n_fft)
        return self._fft_ws

    def mel_spectrogram(self, y):
        """y [B,N] float32 on the HIP device, values in [-1, 1] (asserted like stft.py:177-178, over the whole waveform: the FFT kernel
        also reads, for the check alone, the samples that no frame loads when hop > n_fft/2 + 1)."""
        if not y.is_cuda:
            raise RuntimeError("TacotronSTFT (ctts_amd) computes on the MI355X: pass a device tensor")
        if self._dft_basis.device != y.device:
            self.to(y.device)
        if self.use_fft:
            from . import kernels as K
            self._raise_if_out_of_range(wait=False)          # earlier calls: never blocks
            host, ev = self._range_state(y.device)
            mel, energy, _ = K.mel_spectrogram_fft(y.float().contiguous(), self._window, self._workspace(), self.n_fft, self.hop,
                                                   self.n_mel_channels, kmax=self._kmax, range_flag=host)
            ev.record()
            if self.strict_range:
                self._raise_if_out_of_range(wait=True)
            return mel, energy
        lo, hi = torch.aminmax(y.detach())              # DFT-as-GEMM path (other FFT sizes): one reduction + one sync for the two asserts
        assert lo >= -1 and hi <= 1
        self._sync_filterbank()
        mel, energy, _ = ops.mel_spectrogram(y.float(), self._dft_basis, self._mel_basis_padded, self.n_fft, self.hop,
                                             self.n_mel_channels, self.nbins)
        return mel, energy

    def magnitudes(self, y):
        if self._dft_basis.device != y.device:
            self.to(y.device)
        if self.use_fft:
            from . import kernels as K
            _, _, mag = K.mel_spectrogram_fft(y.float().contiguous(), self._window, self._workspace(), self.n_fft, self.hop,
                                              self.n_mel_channels, want_mag=True, kmax=self._kmax)
            return mag.view(y.shape[0], -1, mag.shape[-1])[:, :, :self.nbins].transpose(1, 2)
        self._sync_filterbank()
        _, _, mag = ops.mel_spectrogram(y.float(), self._dft_basis, self._mel_basis_padded, self.n_fft, self.hop,
                                        self.n_mel_channels, self.nbins)
        B = y.shape[0]
        return mag.view(B, -1, mag.shape[-1])[:, :, :self.nbins].transpose(1, 2)

    def mel_spectrograms_ragged(self, wavs):
        """Batched mel extraction for preprocessing (reference: preprocessor.py:387,467 -> audio/tools.py:8-15, one utterance per call,
        B = 1): `wavs` = list of 1-D float arrays / tensors of different lengths.  ONE pinned host buffer, one H2D copy, ONE kernel
        launch with per-utterance lengths (reflection at each utterance's own end), one D2H copy; returns the per-utterance
        (mel [n_mel, F_b] float32 numpy, energy [F_b]) exactly as `get_mel_from_wav` would, values clipped to [-1, 1] like it does."""
        from . import kernels as K
        if not self.use_fft:
            raise NotImplementedError("mel_spectrograms_ragged needs the FFT kernel (filter_length 1024)")
        dev = self.mel_basis.device
        if dev.type != "cuda":
            raise RuntimeError("TacotronSTFT (ctts_amd) computes on the MI355X: move the module to the device first")
        lens = [int(len(w)) for w in wavs]
        if min(lens) <= self.n_fft // 2:
            raise ValueError("reflect padding needs more than n_fft/2 samples per utterance")
        nmax = (max(lens) + 1) // 2 * 2
        host = torch.zeros(len(wavs), nmax, dtype=torch.float32, pin_memory=True)
        for i, w in enumerate(wavs):
            host[i, :lens[i]] = torch.as_tensor(np.asarray(w, dtype=np.float32)).clamp_(-1, 1)
        y = host.to(dev, non_blocking=True)
        lt = torch.tensor(lens, dtype=torch.int32).to(dev, non_blocking=True)
        mel, energy, _ = K.mel_spectrogram_fft(y, self._window, self._workspace(), self.n_fft, self.hop, self.n_mel_channels,
                                               kmax=self._kmax, lens=lt)
        mel, energy = mel.cpu().numpy(), energy.cpu().numpy()
        out = []
        for i, n in enumerate(lens):
            fb = 1 + n // self.hop
            out.append((np.ascontiguousarray(mel[i, :, :fb]), np.ascontiguousarray(energy[i, :fb])))
        return out


def get_mel_from_wav(audio, _stft):
    """audio/tools.py:8-15: one utterance (numpy) -> (mel [n_mel, F], energy [F]) float32 numpy, input clipped to [-1, 1]"""
    return _stft.mel_spectrograms_ragged([audio])[0]


def inv_mel_spec(mel, out_filename, _stft, griffin_iters=60, momentum=0.0, seed=None):
    """audio/tools.py:18-34: log-mel [n_mel, F] (device tensor) -> float32 wav at _stft.sampling_rate through Griffin-Lim, bug for bug:
    exp(mel) times the filterbank itself (not a pseudo-inverse), * 1000, the last frame dropped.  One deliberate deviation: the reference
    reads `_stft._stft_fn`, which does not exist (AttributeError); this version uses `_stft.stft_fn`.  momentum / seed: griffin_lim's."""
    from scipy.io.wavfile import write
    if not torch.is_tensor(mel) or not mel.is_cuda:
        raise RuntimeError("inv_mel_spec (ctts_amd) computes on the MI355X: pass the mel as a device tensor")
    if _stft.mel_basis.device != mel.device:
        _stft.to(mel.device)
    # spectral_de_normalize (exp, C = 1), the filterbank applied transposed, the fixed gain; drop the last frame, then Griffin-Lim
    spec = (torch.exp(mel).t() @ _stft.mel_basis).t().unsqueeze(0) * 1000.0     # [1, 513, F]
    wav = griffin_lim(spec[:, :, :-1], _stft.stft_fn, griffin_iters, momentum=momentum, seed=seed)[0]
    write(out_filename, _stft.sampling_rate, wav.cpu().numpy())
