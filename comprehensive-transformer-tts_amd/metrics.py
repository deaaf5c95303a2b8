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
"""
import math

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
