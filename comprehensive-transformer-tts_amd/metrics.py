"""Objective evaluation on the device (csrc/metrics.hip): how close a synthesised utterance is to its recording.

  mel_cepstrum    log-mel [B,n_mel,F] -> cepstra [B,F,K]: the orthonormal DCT-II over the mel axis, coefficients 1 .. K (0 dropped)
  dtw             dynamic time warping of two cepstral sequences per pair: cost, path length and the path
  path_metrics    counts and the squared log-F0 distance in cents over the aligned frame pairs
  compare_mels    the three chained: mel-cepstral distortion (dB), log-F0 RMSE (cents) and voiced / unvoiced error per utterance
  wav_features    waveform -> (log-mel, frames, f0): the front end compare_wavs puts in front of compare_mels
  compare_wavs    waveform in: the mel front end and the pitch tracker of this package in front of compare_mels
  summarize       corpus numbers from a compare_* result

WHAT THE MCD HERE IS.  The cepstra are the DCT of THIS project's log-mel spectrogram (`TacotronSTFT`: 80 Slaney-scale channels of the
magnitude spectrum, natural log), i.e. an MFCC-style mel-cepstral distortion.  They are NOT the mel-cepstra that WORLD / SPTK extract
(mel-generalised cepstral analysis of a spectral envelope), which most published MCD figures use: numbers from this module compare
with each other, not with those.  PARITY UNPINNED against WORLD and SPTK: neither is installed where this project is built and tested.
The kernels are pinned against a float64 numpy restatement of the definitions below (tests/metrics_restate.py).

Definitions.  c_k = sqrt(2/M) sum_m mel[m] cos(pi k (m + 1/2) / M), k = 1 .. K.  Local cost d(i,j) = ||x_i - y_j||_2; accumulated cost
A(i,j) = d(i,j) + min(A(i-1,j-1), A(i-1,j), A(i,j-1)) with no window and no slope weights; the path is walked back from the last
frame pair, the diagonal winning ties, then (i-1,j), then (i,j-1).  mcd_db = (10 sqrt(2) / ln 10) cost / path_len; lf0_rmse_cents =
sqrt(sum over pairs voiced in both of (1200 log2(f0_ref / f0_syn))^2 / n_voiced); vuv_error = pairs whose voicing differs / path_len.
A quantity with a zero denominator is NaN, and its count (path_len, n_voiced) says why.

All calls are stream-ordered; lengths are device tensors, nothing synchronises, nothing runs on the CPU: CPU tensors raise.

WAVEFORM METRICS (csrc/wavmetrics.hip): the figures the vocoder literature reports for copy-synthesis, where the synthesised waveform is
sample-aligned with its recording and no DTW is needed.

  stoi                STOI or ESTOI (intelligibility) per utterance, with the frame counts
  si_sdr              scale-invariant signal-to-distortion ratio in dB
  mr_stft_distance    the Parallel-WaveGAN multi-resolution STFT distances: spectral convergence, log-magnitude, log-spectral distance
  waveform_metrics    the three chained; the resample to STOI's 10 kHz happens once
  summarize_waveform  corpus means over the utterances that have a value (the one function here that copies to the host)

All signals are [B, N] float32 device tensors, `lens` host sequences (checked) or device tensors (clamped); samples at and beyond
lens[b] are never read.  The float64 restatement in tests/wavmetrics_restate.py is the contract:

STOI / ESTOI (Taal et al. 2011; Jensen & Taal 2016).  fs = 10000, frames of 256 at hop 128, FFT 512 (frame zero-padded on the right),
window w = np.hanning(258)[1:-1], J = 15 third-octave bands, N = 30 frames per segment, beta = -15 dB, dynamic range 40 dB, eps = 2^-52.
 1. Utterance frame i starts at 128 i, i < F = (len - 256) // 128 + 1 (F = 0 below 256 samples).
 2. Silent-frame removal: e_i = 20 log10(||w x_i||_2 + eps) on the REFERENCE only; frame i is kept iff e_i > max_i e_i - 40.  The kept
    frames of both signals, windowed, are overlap-added at hop 128 in kept order into x', y' (K kept frames: 128 (K - 1) + 256 samples).
 3. Frames of x', y' (same framing, same window again) go to 512-point spectra; band amplitude = sqrt(sum_{k in band j} |X_k|^2), band j
    = bins [lo_j, hi_j) with lo, hi the bins nearest to 150 2^((2j - 1) / 6) and 150 2^((2j + 1) / 6) Hz on the grid k 10000 / 512:
    (7,9) (9,11) (11,14) (14,17) (17,22) (22,27) (27,34) (34,43) (43,55) (55,69) (69,87) (87,109) (109,138) (138,174) (174,219).
 4. For every m = 30 .. M (M = K frames of x') and the 15 x 30 blocks X_m, Y_m of band amplitudes over frames m - 30 .. m - 1:
    STOI: per band row alpha = ||x|| / (||y|| + eps), y' = min(alpha y, x (1 + 10^(15/20))); d_jm = the correlation of the mean-removed
    rows, each normalised by (norm + eps); the result is the mean over j, m.  ESTOI: rows mean-removed and normalised, then columns
    mean-removed and normalised (each by norm + eps); d_m = sum(Xn * Yn) / 30; the result is the mean over m.
 5. M < 30, or a reference whose largest frame energy is 0: NaN and segments = 0 (kept is then what rule 2 gives: every frame).
 6. Counts per utterance: frames (F), kept (K), segments (M - 29).
 7. rate != 10000: both signals first go through `resample.resample(..., rate, 10000, "kaiser_best")`, one ragged batch each.
PARITY with pystoi is UNPINNED: it is not installed where this project is built and tested, and its resampling filter differs from this
project's.  With rate = 10000 the definition above is pystoi's, step by step.

SI-SDR.  With the means over [0, len) removed: t = (<y,x> / <x,x>) x, si_sdr = 10 log10(||t||^2 / ||y - t||^2) dB; NaN for len = 0 or
<x,x> = 0, +inf where y = g x exactly (the device finds the residual exactly 0 for g a power of two).

MULTI-RESOLUTION STFT DISTANCE.  Resolutions (n_fft, hop, win), default (512, 50, 240), (1024, 120, 600), (2048, 240, 1200); window =
periodic Hann 0.5 - 0.5 cos(2 pi n / win), zero-padded on the right to n_fft; frames start at i hop for i < (len - win) // hop + 1, no
padding; |X| = sqrt(max(re^2 + im^2, 1e-7)).  Per utterance and resolution sc = || |X| - |Y| ||_F / || |X| ||_F, log_mag =
mean | ln|X| - ln|Y| |, lsd_db = mean over frames of sqrt(mean over bins of (20 log10|X| - 20 log10|Y|)^2); no frame: NaN.
n_fft in {512, 1024, 2048} and win <= n_fft; anything else raises.
"""
import math

import numpy as np
import torch

from . import kernels as K
from . import pitch_features as PF
from ._lib import CttsError
from .audio import _lens_arg

MCD_DB = 10.0 * math.sqrt(2.0) / math.log(10.0)


def _dev(t, what, name):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise CttsError(f"{what} computes on the MI355X: pass {name} as a device tensor - no CPU fallback exists")
    return t


def _f32(t):
    return t if t.dtype == torch.float32 and t.is_contiguous() else t.float().contiguous()


def _lens(lens, B, hi, what, dev):
    if lens is None:
        return torch.full((B,), hi, dtype=torch.int32, device=dev)
    try:
        return _lens_arg(lens, B, 0, hi, what, dev)
    except ValueError as e:
        raise CttsError(str(e)) from None


def mel_cepstrum(mel, frames=None, n_coef=13):
    """mel [B,n_mel,F] natural-log mel (the layout `TacotronSTFT.mel_spectrogram` returns), frames [B] (device tensor or host
    sequence; None = F) -> [B,F,n_coef]; rows at or beyond frames[b] are zero.  1 <= n_coef <= 32, n_coef < n_mel."""
    mel = _f32(_dev(mel, "mel_cepstrum", "mel"))
    if mel.dim() != 3:
        raise CttsError(f"mel_cepstrum: expected mel [B, n_mel, F], got {tuple(mel.shape)}")
    return K.mel_cepstrum(mel, None if frames is None else _lens(frames, mel.shape[0], mel.shape[2], "mel_cepstrum frames", mel.device), n_coef)


def dtw(x, x_lens, y, y_lens, align="dtw"):
    """x [B,Tx,K], y [B,Ty,K], x_lens / y_lens [B] -> dict(cost float32 [B] = A(Lx-1, Ly-1), path_len int32 [B],
    path int32 [B, Tx + Ty - 1, 2]: the (i, j) pairs in order from (0,0), -1 beyond path_len).  An empty sequence gives cost 0, path_len 0
    and an all -1 path.  align="none": frame i against frame i over min(Lx, Ly), the same outputs.  Padded Tx, Ty <= 2048, K <= 32."""
    x, y = _f32(_dev(x, "dtw", "x")), _f32(_dev(y, "dtw", "y"))
    if x.dim() != 3 or y.dim() != 3:
        raise CttsError(f"dtw: expected x [B, Tx, K] and y [B, Ty, K], got {tuple(x.shape)} / {tuple(y.shape)}")
    B = x.shape[0]
    cost, path_len, path = K.dtw(x, _lens(x_lens, B, x.shape[1], "dtw x_lens", x.device), y,
                                 _lens(y_lens, B, y.shape[1], "dtw y_lens", x.device), align)
    return {"cost": cost, "path_len": path_len, "path": path}


def path_metrics(path, path_len, f0_x, f0_y):
    """path int32 [B,P,2], path_len [B], f0_x [B,Tx], f0_y [B,Ty] in Hz with 0 = unvoiced -> float64 [B,4]: aligned pairs, pairs voiced in
    both, sum over those of (1200 log2(f0_x / f0_y))^2, pairs whose voicing differs."""
    path = _dev(path, "path_metrics", "path")
    f0_x, f0_y = _f32(_dev(f0_x, "path_metrics", "f0_x")), _f32(_dev(f0_y, "path_metrics", "f0_y"))
    if path.dim() != 3:
        raise CttsError(f"path_metrics: expected path [B, P, 2], got {tuple(path.shape)}")
    if path.dtype != torch.int32 or not path.is_contiguous():
        path = path.to(torch.int32).contiguous()
    return K.path_metrics(path, _lens(path_len, path.shape[0], path.shape[1], "path_metrics path_len", path.device), f0_x, f0_y)


def compare_mels(mel_ref, frames_ref, mel_syn, frames_syn, f0_ref=None, f0_syn=None, align="dtw", n_coef=13):
    """mel_ref [B,n_mel,Fr], mel_syn [B,n_mel,Fs] natural-log mels, frames_* [B]; f0_ref [B,Fr], f0_syn [B,Fs] in Hz (0 = unvoiced), both
    or neither.  -> dict of per-utterance device tensors: mcd_db, lf0_rmse_cents, vuv_error (float64), path_len, n_voiced (int32), and
    the sums they come from (cost float32, sq_cents float64, n_mismatch int32), which `summarize` pools.  Without f0 the two pitch
    measures are NaN and n_voiced is 0.  align="none" compares frame i with frame i over min(frames_ref, frames_syn): the mode for two
    vocoders fed the same mel; same path / path_metrics route."""
    if (f0_ref is None) != (f0_syn is None):
        raise CttsError("compare_mels: give f0_ref and f0_syn together or neither")
    mel_ref, mel_syn = _dev(mel_ref, "compare_mels", "mel_ref"), _dev(mel_syn, "compare_mels", "mel_syn")
    if mel_ref.dim() != 3 or mel_syn.dim() != 3 or mel_ref.shape[:2] != mel_syn.shape[:2]:
        raise CttsError(f"compare_mels: expected two [B, n_mel, F] mels of one batch, got {tuple(mel_ref.shape)} / {tuple(mel_syn.shape)}")
    B, dev = mel_ref.shape[0], mel_ref.device
    fr = _lens(frames_ref, B, mel_ref.shape[2], "compare_mels frames_ref", dev)
    fs = _lens(frames_syn, B, mel_syn.shape[2], "compare_mels frames_syn", dev)
    a = dtw(mel_cepstrum(mel_ref, fr, n_coef), fr, mel_cepstrum(mel_syn, fs, n_coef), fs, align)
    n = a["path_len"].double()
    out = {"mcd_db": MCD_DB * a["cost"].double() / n, "path_len": a["path_len"], "cost": a["cost"]}
    if f0_ref is None:
        nan = torch.full((B,), float("nan"), dtype=torch.float64, device=dev)
        zero = torch.zeros(B, dtype=torch.int32, device=dev)
        out.update(lf0_rmse_cents=nan, vuv_error=nan.clone(), n_voiced=zero, sq_cents=torch.zeros(B, dtype=torch.float64, device=dev),
                   n_mismatch=zero.clone())
        return out
    if f0_ref.shape != (B, mel_ref.shape[2]) or f0_syn.shape != (B, mel_syn.shape[2]):
        raise CttsError(f"compare_mels: f0 {tuple(f0_ref.shape)} / {tuple(f0_syn.shape)} must have the mels' frames")
    m = path_metrics(a["path"], a["path_len"], f0_ref, f0_syn)
    out.update(lf0_rmse_cents=torch.sqrt(m[:, 2] / m[:, 1]), vuv_error=m[:, 3] / n, n_voiced=m[:, 1].to(torch.int32), sq_cents=m[:, 2],
               n_mismatch=m[:, 3].to(torch.int32))
    return out


def wav_features(wav, lens, stft, what="wav_features"):
    """wav [B,N], lens [B] samples or None -> (mel [B,n_mel,F], frames [B] = 1 + len // hop, f0 [B,F] in Hz) with the framing `preprocess.process_batch` uses: device lengths, so
    every utterance is framed (and reflected at its own end) as in a call of its own"""
    wav = _dev(wav, what, "the waveforms")
    if wav.dim() != 2:
        raise CttsError(f"{what}: expected [B, N] waveforms, got {tuple(wav.shape)}")
    if not stft.use_fft:
        raise NotImplementedError(f"{what} needs the FFT mel kernel (filter_length 1024)")
    if stft._dft_basis.device != wav.device:
        stft.to(wav.device)
    B, N = wav.shape
    try:
        lens = torch.full((B,), N, dtype=torch.int32, device=wav.device) if lens is None else \
            _lens_arg(lens, B, stft.n_fft // 2 + 1, N, f"{what} lens", wav.device)
    except ValueError as e:
        raise CttsError(str(e)) from None
    y = wav.float()
    if N % 2:
        y = torch.nn.functional.pad(y, (0, 1))
    pos = torch.arange(y.shape[1], device=wav.device)[None, :]
    y = torch.where(pos < lens[:, None], y.clamp(-1, 1), torch.zeros_like(y)).contiguous()
    mel, _, _ = K.mel_spectrogram_fft(y, stft._window, stft._workspace(), stft.n_fft, stft.hop, stft.n_mel_channels, kmax=stft._kmax, lens=lens)
    f0, _ = PF.track_pitch(y, lens, sr=stft.sampling_rate, hop=stft.hop)
    frames = (1 + torch.div(lens, stft.hop, rounding_mode="floor")).to(torch.int32)
    return mel, frames, f0


def compare_wavs(ref, ref_lens, syn, syn_lens, stft, **kw):
    """ref [B,Nr], syn [B,Ns] waveforms in [-1,1] (clipped like `get_mel_from_wav`), *_lens [B] samples (device tensors, host sequences or
    None = all), stft: the `TacotronSTFT` -> `compare_mels` of their log-mels (frames = 1 + len // hop) and `track_pitch` contours.
    kw: align, n_coef."""
    mr, fr, pr = wav_features(ref, ref_lens, stft, "compare_wavs")
    ms, fs, ps = wav_features(syn, syn_lens, stft, "compare_wavs")
    return compare_mels(mr, fr, ms, fs, pr, ps, **kw)


def summarize(result):
    """Corpus numbers of a compare_* result as device scalars (float64): mcd_db and vuv_error are the per-utterance values weighted by
    path_len (utterances with path_len 0 carry no weight), lf0_rmse_cents comes from the pooled squared sum over the pooled voiced pairs;
    plus the two pooled counts.  A pooled zero denominator gives NaN."""
    n = result["path_len"].double()
    total, voiced = n.sum(), result["n_voiced"].double().sum()
    zero = torch.zeros_like(n)

    def weighted(v):
        return torch.where(n > 0, v.double() * n, zero).sum() / total
    return {"mcd_db": weighted(result["mcd_db"]), "lf0_rmse_cents": torch.sqrt(result["sq_cents"].double().sum() / voiced),
            "vuv_error": weighted(result["vuv_error"]), "path_len": total, "n_voiced": voiced}


# ---- waveform metrics (module docstring, WAVEFORM METRICS) ------------------------------------------------------------------------
STOI_RATE = 10000
MR_STFT_DEFAULT = ((512, 50, 240), (1024, 120, 600), (2048, 240, 1200))
_windows = {}


def stoi_window():
    """the 256-point analysis window of STOI, float64 on the host"""
    return np.hanning(K.STOI_FRAME + 2)[1:-1].copy()


def mr_stft_window(win):
    """periodic Hann of `win` samples, float64 on the host"""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(int(win)) / float(int(win)))


def _window(kind, n, dev):
    key = (kind, n, str(dev))
    if key not in _windows:
        _windows[key] = torch.from_numpy(stoi_window() if kind == "stoi" else mr_stft_window(n)).to(dev)
    return _windows[key]


def _pair(ref, syn, lens, what):
    ref, syn = _dev(ref, what, "ref"), _dev(syn, what, "syn")
    if ref.dim() != 2 or ref.shape != syn.shape or ref.shape[0] < 1 or ref.shape[1] < 1:
        raise CttsError(f"{what}: expected two non-empty [B, N] waveforms of one shape, got {tuple(ref.shape)} / {tuple(syn.shape)}")
    return _f32(ref), _f32(syn), _lens(lens, ref.shape[0], ref.shape[1], f"{what} lens", ref.device)


def _to_stoi_rate(ref, syn, lens, rate):
    rate = int(rate)
    if rate == STOI_RATE:
        return ref, syn, lens
    from . import resample as RS
    try:
        r, out_lens = RS.resample(ref, lens, rate, STOI_RATE, "kaiser_best")
        s, _ = RS.resample(syn, lens, rate, STOI_RATE, "kaiser_best")
    except ValueError as e:
        raise CttsError(str(e)) from None
    return r, s, out_lens


def _stoi_both(ref, syn, lens, rate):
    ref, syn, lens = _to_stoi_rate(ref, syn, lens, rate)
    limit = K.STOI_HOP * (K.stoi_max_frames() - 1) + K.STOI_FRAME + K.STOI_HOP - 1
    if ref.shape[1] > limit:
        raise CttsError(f"stoi: rows of {ref.shape[1]} samples at {STOI_RATE} Hz exceed the {K.stoi_max_frames()} frames ({limit} samples, "
                        f"{limit / STOI_RATE:.1f} s) one utterance may hold - cut the utterances")
    d, e, counts = K.stoi(ref, syn, lens, _window("stoi", K.STOI_FRAME, ref.device))
    return d, e, counts


def stoi(ref, syn, lens, rate, extended=False):
    """ref, syn [B,N] at `rate` Hz, lens [B] or None -> dict of device tensors: stoi float64 [B] (ESTOI with extended=True; NaN without
    a segment), frames, kept, segments int32 [B]."""
    ref, syn, lens = _pair(ref, syn, lens, "stoi")
    d, e, counts = _stoi_both(ref, syn, lens, rate)
    return {"stoi": e if extended else d, "frames": counts[:, 0], "kept": counts[:, 1], "segments": counts[:, 2]}


def si_sdr(ref, syn, lens):
    """ref, syn [B,N], lens [B] or None -> float64 [B] in dB on the device"""
    ref, syn, lens = _pair(ref, syn, lens, "si_sdr")
    return K.si_sdr(ref, syn, lens)


def _resolutions(resolutions):
    try:
        res = [tuple(int(v) for v in r) for r in resolutions]
    except (TypeError, ValueError):
        raise CttsError(f"mr_stft_distance: resolutions must be (n_fft, hop, win) triples, got {resolutions!r}") from None
    if not res or any(len(r) != 3 for r in res):
        raise CttsError(f"mr_stft_distance: resolutions must be (n_fft, hop, win) triples, got {resolutions!r}")
    for n_fft, hop, win in res:
        if n_fft not in K.MR_STFT_SIZES or not 1 <= win <= n_fft or hop < 1:
            raise CttsError(f"mr_stft_distance: resolution ({n_fft}, {hop}, {win}): n_fft must be one of {K.MR_STFT_SIZES}, "
                            "1 <= win <= n_fft and hop >= 1")
    return res


def mr_stft_distance(ref, syn, lens, resolutions=MR_STFT_DEFAULT):
    """ref, syn [B,N], lens [B] or None -> dict of [B, R] device tensors: sc, log_mag, lsd_db (float64; NaN without a frame), frames int32"""
    res = _resolutions(resolutions)
    ref, syn, lens = _pair(ref, syn, lens, "mr_stft_distance")
    outs, frames = zip(*(K.mr_stft(ref, syn, lens, _window("hann", win, ref.device), n_fft, hop) for n_fft, hop, win in res))
    v = torch.stack(outs, dim=1)
    return {"sc": v[:, :, 0], "log_mag": v[:, :, 1], "lsd_db": v[:, :, 2], "frames": torch.stack(frames, dim=1)}


def waveform_metrics(ref, syn, lens, rate):
    """The three chained: stoi, estoi, frames, kept, segments [B]; si_sdr [B]; sc, log_mag, lsd_db, mr_frames [B, R] at the default
    resolutions.  SI-SDR and the STFT distances are taken at `rate`, STOI and ESTOI on one resample to 10 kHz."""
    ref, syn, lens = _pair(ref, syn, lens, "waveform_metrics")
    d, e, counts = _stoi_both(ref, syn, lens, rate)
    mr = mr_stft_distance(ref, syn, lens)
    return {"stoi": d, "estoi": e, "frames": counts[:, 0], "kept": counts[:, 1], "segments": counts[:, 2], "si_sdr": K.si_sdr(ref, syn, lens),
            "sc": mr["sc"], "log_mag": mr["log_mag"], "lsd_db": mr["lsd_db"], "mr_frames": mr["frames"]}


def summarize_waveform(result):
    """Corpus numbers of a `waveform_metrics` / `stoi` / `mr_stft_distance` result, or of {"si_sdr": si_sdr(...)}: for every float
    entry {"mean": the mean over the utterances whose value is not NaN (per resolution for [B, R] entries; NaN when there is none),
    "count": how many those are}.  Host floats and ints: this is the one function of the module that copies to the host."""
    out = {}
    for name, v in result.items():
        if not torch.is_tensor(v) or not v.is_floating_point():
            continue
        a = v.detach().double().cpu().numpy()
        ok = ~np.isnan(a)
        n = ok.sum(axis=0)
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = np.where(ok, a, 0.0).sum(axis=0) / n
        out[name] = {"mean": mean.tolist(), "count": n.tolist()}
    return out


def speaker_similarity(ref, ref_lens, syn, syn_lens, embedder, source_rate=None):
    """Cosine of the DeepSpeaker embeddings of `ref` and `syn` per pair, float32 [B] on the device: the speaker-similarity figure of
    multi-speaker synthesis.  ref [B, N1], syn [B, N2] float32 at 22050 Hz (or at `source_rate`), lengths as in `speaker.DeepSpeakerEmbedder`
    (centre crop).  The embeddings are unit vectors, so the cosine is their dot product; a pair with an invalid side (no voice span) gives 0."""
    a = embedder(ref, ref_lens, source_rate=source_rate)["embedding"]
    b = embedder(syn, syn_lens, source_rate=source_rate)["embedding"]
    if a.shape != b.shape:
        raise CttsError(f"speaker_similarity: {a.shape[0]} reference and {b.shape[0]} synthesised utterances")
    return (a.double() * b.double()).sum(1).float()
