"""Dataset preparation on the device (csrc/preprocess.hip): the three steps of the reference's preprocessor/preprocessor.py that ran
on the host, one utterance at a time, plus the batch driver that strings them together with the mel and pitch kernels.

  trim_silence      `load_audio` (:363-368): librosa 0.7.2 `effects.trim(ref=np.max)` restated - PARITY UNPINNED against librosa, which is
                    not installed where this project is built; pinned against a float64 numpy restatement of the published definition
  attention_prior   `beta_binomial_prior_distribution` (:551-560) as it is CALLED (:409-413, the two counts swapped against the
                    parameter names): pinned against the live reference (tests/golden/g20_preprocess.npz)
  outlier_stats     `remove_outlier` (:620-628) and the moments `StandardScaler.partial_fit` accumulates; `merge_moments` is the Chan
                    merge of the per-utterance triples in utterance order (host arithmetic on B triples)
  DatasetStats      accumulates what the reference writes to stats.json
  process_batch     wav -> every array the unsupervised branch saves (:420-446), one ragged batch at a time

Lengths are device tensors (clamped by the kernels) or host sequences (checked here); nothing synchronises except `process_batch`
(one device-to-host copy of its results) and `DatasetStats.finalize`.  CPU tensors raise: there is no CPU path.
"""
import math

import numpy as np
import torch

from . import kernels as K
from . import pitch_features as PF
from ._lib import CttsError
from .audio import _lens_arg


def _wav_arg(wav, what):
    if not torch.is_tensor(wav) or not wav.is_cuda:
        raise CttsError(f"{what} computes on the MI355X: pass device tensors - no CPU fallback exists")
    if wav.dim() != 2:
        raise CttsError(f"{what}: expected a [B, N] tensor, got {tuple(wav.shape)}")
    return wav.float().contiguous()


def trim_silence(wav, lens, top_db, frame_length=1024, hop=256, return_power=False):
    """wav [B,N] (device), lens [B] samples (host sequence, checked: frame_length / 2 < len <= N; or device tensor, clamped by the
    kernel) -> (start, end, duration) int32 [B] on the device: the utterance's non-silent span [start, end) in samples and
    duration = (end - start) // hop, the frame count `load_audio` returns.  return_power: also the frame powers mse [B, 1 + N // hop]."""
    wav = _wav_arg(wav, "trim_silence")
    B, N = wav.shape
    if lens is None:
        lens = [N] * B
    lens = _lens_arg(lens, B, int(frame_length) // 2 + 1, N, "trim_silence lens", wav.device)
    start, end, mse = K.trim_silence(wav, lens, top_db, frame_length, hop)
    duration = torch.div(end - start, int(hop), rounding_mode="floor")
    return (start, end, duration, mse) if return_power else (start, end, duration)


def _count_arg(lens, what, dev, B=None):
    """-> (int32 device tensor [B], host maximum or None when the lengths live on the device)"""
    if torch.is_tensor(lens) and lens.is_cuda:
        t = lens.reshape(-1)
        if t.dtype != torch.int32 or not t.is_contiguous():
            t = t.to(torch.int32).contiguous()
        hmax = None
    elif torch.is_tensor(lens) and dev is None:
        raise CttsError(f"{what} computes on the MI355X: pass device tensors (or host lists next to a device `out`) - no CPU fallback exists")
    else:
        v = [int(n) for n in (lens.tolist() if torch.is_tensor(lens) else lens)]
        if len(v) == 0 or min(v) < 0:
            raise ValueError(f"{what}: lengths must be non-negative and not empty, got {v}")
        if dev is None:
            raise CttsError(f"{what} computes on the MI355X: pass device tensors (or host lists next to a device `out`) - no CPU fallback exists")
        t, hmax = torch.tensor(v, dtype=torch.int32).to(dev), max(v)
    if B is not None and t.numel() != B:
        raise ValueError(f"{what}: {t.numel()} lengths for a batch of {B}")
    return t, hmax


def attention_prior(src_lens, mel_lens, scaling_factor=1.0, max_src_len=None, max_mel_len=None, out=None):
    """The beta-binomial alignment prior of a batch, padded like `pad_3D` / `data.reprocess`: [B, max_src_len, max_mel_len] float32,
    out[b, s, t] = BetaBinom.pmf(t; n = mel_len_b, a = sf (s + 1), b = sf (src_len_b - s)) inside the utterance, 0 outside.
    src_lens / mel_lens: device tensors (no host round trip: then give `out` or both maxima) or host sequences.
    out: a float32 [B, Ts, Tm] device view with a contiguous last dimension, e.g. a slice of a static training buffer - filled in
    place (every element), nothing is allocated for it."""
    dev = out.device if out is not None else next((t.device for t in (src_lens, mel_lens) if torch.is_tensor(t) and t.is_cuda), None)
    if out is not None and (not torch.is_tensor(out) or not out.is_cuda):
        raise CttsError("attention_prior computes on the MI355X: `out` must be a device tensor - no CPU fallback exists")
    if dev is None and torch.cuda.is_available() and not any(torch.is_tensor(t) for t in (src_lens, mel_lens)):
        dev = torch.device("cuda", torch.cuda.current_device())
    src, smax = _count_arg(src_lens, "attention_prior src_lens", dev)
    mel, mmax = _count_arg(mel_lens, "attention_prior mel_lens", dev, src.numel())
    B = src.numel()
    if out is None:
        Ts = int(max_src_len) if max_src_len is not None else smax
        Tm = int(max_mel_len) if max_mel_len is not None else mmax
        if Ts is None or Tm is None:
            raise CttsError("attention_prior: with device lengths give max_src_len and max_mel_len (or `out`): reading them back would synchronise")
        if (smax is not None and smax > Ts) or (mmax is not None and mmax > Tm):
            raise ValueError(f"attention_prior: lengths up to {smax} x {mmax} do not fit the padded {Ts} x {Tm}")
        out = torch.empty(B, Ts, Tm, dtype=torch.float32, device=dev)
    else:
        if out.dim() != 3 or out.shape[0] != B:
            raise ValueError(f"attention_prior: out {tuple(out.shape)} for a batch of {B}")
        if (max_src_len is not None and int(max_src_len) != out.shape[1]) or (max_mel_len is not None and int(max_mel_len) != out.shape[2]):
            raise ValueError(f"attention_prior: out {tuple(out.shape)} against max_src_len {max_src_len}, max_mel_len {max_mel_len}")
        if (smax is not None and smax > out.shape[1]) or (mmax is not None and mmax > out.shape[2]):
            raise ValueError(f"attention_prior: lengths up to {smax} x {mmax} do not fit out {tuple(out.shape)}")
    return K.attn_prior(src, mel, out, scaling_factor)


def outlier_stats(values, lens):
    """values [B,L] (device), lens [B] -> dict(keep uint8 [B,L] - `remove_outlier`'s mask (IQR rule, strict on both sides) -, count int32
    [B], sum / M2 float64 [B] and min / max float32 [B] over the kept values; M2 about the kept values' own mean).  L <= 4096."""
    values = _wav_arg(values, "outlier_stats")
    B, L = values.shape
    if lens is None:
        lens = [L] * B
    lens = _lens_arg(lens, B, 0, L, "outlier_stats lens", values.device)
    keep, count, s, m2, lo, hi = K.outlier_stats(values, lens)
    return {"keep": keep, "count": count, "sum": s, "M2": m2, "min": lo, "max": hi}


def merge_moments(counts, sums, m2s):
    """Chan's pairwise merge of per-utterance (count, sum, M2) in utterance order, in float64 -> (n, mean, std) with the population
    variance: what `StandardScaler.partial_fit` holds after being fed the utterances one at a time (empty ones skipped, as
    preprocessor.py:135-137 does)."""
    n, mean, m2 = 0, 0.0, 0.0
    for c, s, q in zip(np.asarray(counts).tolist(), np.asarray(sums, dtype=np.float64).tolist(), np.asarray(m2s, dtype=np.float64).tolist()):
        c = int(c)
        if c <= 0:
            continue
        mb = s / c
        if n == 0:
            n, mean, m2 = c, mb, q
            continue
        d, tot = mb - mean, n + c
        m2 = m2 + q + d * d * (n * c / tot)
        mean = mean + d * (c / tot)
        n = tot
    return n, mean, (math.sqrt(m2 / n) if n > 0 else float("nan"))


class DatasetStats:
    """What the reference collects into stats.json while it walks the corpus (preprocessor.py:123-133, 249-257, 265-299), one batch at a
    time: `update` runs on the device and keeps only per-utterance scalars there, `finalize` reads them back once and merges.

    branch "unsup" / "sup" names the keys: f0_<branch> = [mean, std] over the voiced (non-zero) frames (compute_f0_stats);
    energy_<branch>_frame = [min, max, mean, std] - mean / std over the values `remove_outlier` keeps per utterance, min / max over ALL
    stored values after normalisation with that mean / std (compute_energy_stats + normalize); spec_<branch>_min / _max per mel channel;
    max_seq_len.  Only what was fed appears."""

    def __init__(self, branch="unsup", energy_normalization=True):
        self.branch, self.energy_normalization = branch, energy_normalization
        self._e, self._f, self._spec, self._maxlen = [], [], [], []

    @staticmethod
    def _frame_mask(lens, T):
        return torch.arange(T, device=lens.device)[None, :] < lens[:, None]

    def update(self, lens, energy=None, f0=None, mel=None):
        """lens [B] frames (device); energy [B,T], f0 [B,T] Hz with 0 = unvoiced, mel [B,T,n_mel] - any subset, all on the device"""
        if not torch.is_tensor(lens) or not lens.is_cuda:
            raise CttsError("DatasetStats computes on the MI355X: pass device tensors - no CPU fallback exists")
        lens = lens.to(torch.int32).contiguous().view(-1)
        self._maxlen.append(lens.max())
        if energy is not None:
            o = outlier_stats(energy, lens)
            m = self._frame_mask(lens, energy.shape[1])
            e = energy.float()
            lo = torch.where(m, e, torch.full_like(e, float("inf"))).amin(1)
            hi = torch.where(m, e, torch.full_like(e, float("-inf"))).amax(1)
            self._e.append((o["count"], o["sum"], o["M2"], lo, hi))
        if f0 is not None:
            m = self._frame_mask(lens, f0.shape[1]) & (f0 != 0)
            x = torch.where(m, f0.double(), torch.zeros((), dtype=torch.float64, device=f0.device))
            c = m.sum(1)
            s = x.sum(1)
            d = torch.where(m, x - (s / c.clamp(min=1))[:, None], torch.zeros_like(x))
            self._f.append((c, s, (d * d).sum(1)))
        if mel is not None:
            m = self._frame_mask(lens, mel.shape[1])[..., None]
            x = mel.float()
            self._spec.append((torch.where(m, x, torch.full_like(x, float("inf"))).amin((0, 1)),
                               torch.where(m, x, torch.full_like(x, float("-inf"))).amax((0, 1))))

    def finalize(self):
        out, br = {}, self.branch
        if self._f:
            c, s, q = (torch.cat([t[i] for t in self._f]).cpu().numpy() for i in range(3))
            _, mean, std = merge_moments(c, s, q)
            out[f"f0_{br}"] = [float(mean), float(std)]
        if self._e:
            c, s, q, lo, hi = (torch.cat([t[i] for t in self._e]).cpu().numpy() for i in range(5))
            mean, std = 0.0, 1.0
            if self.energy_normalization:
                _, mean, std = merge_moments(c, s, q)
            out[f"energy_{br}_frame"] = [float((np.float64(lo.min()) - mean) / std), float((np.float64(hi.max()) - mean) / std), float(mean), float(std)]
        if self._spec:
            out[f"spec_{br}_min"] = torch.stack([t[0] for t in self._spec]).amin(0).cpu().double().tolist()
            out[f"spec_{br}_max"] = torch.stack([t[1] for t in self._spec]).amax(0).cpu().double().tolist()
        if self._maxlen:
            out["max_seq_len"] = int(torch.stack(self._maxlen).max())
        return out


def _to_stft_rate(wavs, source_rate, target_rate, quality):
    """the utterances as one ragged batch through `resample.resample` (librosa.load(path, sampling_rate) of :364); lengths stay on the host"""
    from . import resample as RS
    lens = [int(w.numel()) for w in wavs]
    if min(lens) < 1:
        raise ValueError("process_batch: empty utterance")
    wav = torch.zeros(len(wavs), max(lens), dtype=torch.float32, device=wavs[0].device)
    for i, w in enumerate(wavs):
        wav[i, :lens[i]] = w
    out, _ = RS.resample(wav, lens, source_rate, target_rate, quality)
    g = math.gcd(int(source_rate), int(target_rate))
    L, M = int(target_rate) // g, int(source_rate) // g
    return [out[i, :RS.output_length(n, L, M)] for i, n in enumerate(lens)]


def process_batch(wavs, n_phones, stft, preprocess_config, spans=None, source_rate=None, resample_quality="kaiser_best"):
    """One ragged batch through the unsupervised branch of `Preprocessor.process_utterance` (:375-446).
    wavs: sequence of 1-D float device tensors (raw audio at the STFT's sampling rate, or at `source_rate`); n_phones: phonemes per
    utterance (host ints); stft: the `TacotronSTFT` (FFT path, on the device); spans: optional [B,2] host ints `[start, end)` in samples
    that REPLACE the trim (the supervised branch cuts by TextGrid times, parsed on the host).
    source_rate: the sampling rate of `wavs` when it is not the STFT's: the utterances are first resampled to `stft.sampling_rate` as one
    ragged batch (`resample.resample` with `resample_quality`), and everything below - `spans`, start, end - is in target-rate samples.
    Chain: trim kernel -> the ragged mel / energy kernel on the trimmed spans -> `pitch_targets_from_wav` on the same spans -> prior
    kernel; every output is cut to `duration` = (end - start) // hop frames like :389-400.  Returns one dict of numpy arrays per
    utterance: mel [T,n_mel], energy [T], f0 [T] (Hz), pitch [T] (coarse ids), cwt_spec [T,10], f0cwt_mean_std [2], attn_prior
    [n_phones,T], duration, start, end, valid (as in `pitch_features`: 0 = no usable contour, the reference drops the utterance).
    The contour statistics and the CWT cover the tracker's 1 + len // hop frames of the span (pitch_targets_from_wav) before the cut."""
    from .model import f0_to_coarse
    if len(wavs) == 0:
        raise ValueError("process_batch: empty batch")
    for w in wavs:
        if not torch.is_tensor(w) or not w.is_cuda:
            raise CttsError("process_batch computes on the MI355X: pass device tensors - no CPU fallback exists")
        if w.dim() != 1:
            raise ValueError(f"process_batch: each utterance is a 1-D tensor, got {tuple(w.shape)}")
    if not stft.use_fft:
        raise NotImplementedError("process_batch needs the FFT mel kernel (filter_length 1024)")
    B, dev = len(wavs), wavs[0].device
    nph = [int(n) for n in n_phones]
    if len(nph) != B or min(nph) < 1:
        raise ValueError(f"process_batch: need one positive phoneme count per utterance, got {nph}")
    if source_rate is not None and int(source_rate) != int(stft.sampling_rate):
        wavs = _to_stft_rate(wavs, source_rate, stft.sampling_rate, resample_quality)
    if stft._dft_basis.device != dev:
        stft.to(dev)
    pp = preprocess_config["preprocessing"]
    top_db = pp["audio"].get("trim_top_db", 23)
    sf = pp.get("duration", {}).get("beta_binomial_scaling_factor", 1.0)
    n_fft, hop = stft.n_fft, stft.hop
    lens = [int(w.numel()) for w in wavs]
    if min(lens) <= n_fft // 2:
        raise ValueError("reflect padding needs more than n_fft/2 samples per utterance")
    N = (max(lens) + 1) // 2 * 2
    wav = torch.zeros(B, N, dtype=torch.float32, device=dev)
    for i, w in enumerate(wavs):
        wav[i, :lens[i]] = w
    if spans is None:
        start, end, _ = trim_silence(wav, lens, top_db, n_fft, hop)
    else:
        sp = [(int(a), int(b)) for a, b in spans]
        if len(sp) != B or any(a < 0 or b < a or b > n for (a, b), n in zip(sp, lens)):
            raise ValueError(f"process_batch: spans must satisfy 0 <= start <= end <= len, got {sp} for lengths {lens}")
        se = torch.tensor(sp, dtype=torch.int32).to(dev)
        start, end = se[:, 0].contiguous(), se[:, 1].contiguous()
    tl = (end - start).contiguous()                                            # samples per trimmed utterance
    duration = torch.div(tl, hop, rounding_mode="floor").to(torch.int32)
    # the trimmed spans, left-aligned and clipped to [-1, 1] like get_mel_from_wav: an index gather, no arithmetic
    pos = torch.arange(N, device=dev)[None, :]
    y = torch.gather(wav, 1, (pos + start[:, None]).clamp(max=N - 1).long())
    y = torch.where(pos < tl[:, None], y.clamp(-1, 1), torch.zeros_like(y)).contiguous()
    mel, energy, _ = K.mel_spectrogram_fft(y, stft._window, stft._workspace(), n_fft, hop, stft.n_mel_channels, kmax=stft._kmax, lens=tl)
    pt = PF.pitch_targets_from_wav(y, tl, stft)
    F = mel.shape[2]
    prior = attention_prior(nph, duration, sf, max_src_len=max(nph), max_mel_len=F)
    coarse = f0_to_coarse(pt["pitch"])
    mean_std = torch.stack([pt["f0_mean"], pt["f0_std"]], 1)
    host = [t.cpu().numpy() for t in (mel, energy, pt["pitch"], coarse, pt["cwt_spec"], mean_std, prior, duration, start, end, pt["valid"])]
    mel, energy, f0, coarse, cwt, mean_std, prior, duration, start, end, valid = host
    out = []
    for b in range(B):
        T = int(duration[b])
        out.append({"mel": np.ascontiguousarray(mel[b, :, :T].T), "energy": energy[b, :T].copy(), "f0": f0[b, :T].copy(),
                    "pitch": coarse[b, :T].copy(), "cwt_spec": cwt[b, :T].copy(), "f0cwt_mean_std": mean_std[b].copy(),
                    "attn_prior": prior[b, :nph[b], :T].copy(), "duration": T, "start": int(start[b]), "end": int(end[b]),
                    "valid": int(valid[b])})
    return out


def process_batch_loudness(wavs, n_phones, stft, preprocess_config, loudness=-22.0, spans=None, source_rate=None,
                           resample_quality="kaiser_best"):
    """`process_batch` on loudness-normalised audio, the order of the reference's `get_mel_from_wav` path with pyloudnorm
    (audio/stft.py:226-231): the utterances are resampled to the STFT's rate when `source_rate` says so, each is brought to `loudness`
    LUFS (ITU-R BS.1770 integrated loudness, `loudness.normalize_loudness` with the reference's peak guard) as one ragged batch on the
    device, and the result goes through `process_batch` unchanged.  The trim threshold is relative to the utterance's own loudest frame,
    so the trimmed spans are those of the unnormalised audio up to the rounding of one fp32 product per sample.  Every utterance must
    be at least 0.4 s long at the STFT's rate.  `process_batch` itself keeps its parameter list: earlier callers and tests pin it."""
    from .loudness import normalize_loudness
    if len(wavs) == 0:
        raise ValueError("process_batch_loudness: empty batch")
    for w in wavs:
        if not torch.is_tensor(w) or not w.is_cuda:
            raise CttsError("process_batch_loudness computes on the MI355X: pass device tensors - no CPU fallback exists")
        if w.dim() != 1:
            raise ValueError(f"process_batch_loudness: each utterance is a 1-D tensor, got {tuple(w.shape)}")
    if source_rate is not None and int(source_rate) != int(stft.sampling_rate):
        wavs = _to_stft_rate(wavs, source_rate, stft.sampling_rate, resample_quality)
    lens = [int(w.numel()) for w in wavs]
    wav = torch.zeros(len(wavs), max(lens), dtype=torch.float32, device=wavs[0].device)
    for i, w in enumerate(wavs):
        wav[i, :lens[i]] = w
    out = normalize_loudness(wav, lens, stft.sampling_rate, target=float(loudness), peak_limit=True, out=wav)[0]
    return process_batch([out[i, :n] for i, n in enumerate(lens)], n_phones, stft, preprocess_config, spans=spans)


def speaker_embeddings(wavs, speakers, embedder, source_rate=None):
    """The speaker-embedding files of the reference's preprocessor (preprocessor.py:246-263, 376): wavs - a sequence of 1-D float device
    tensors at 22050 Hz (or at `source_rate`), speakers - one speaker name per utterance, embedder - a `speaker.DeepSpeakerEmbedder`.
    Returns (per_utterance, per_speaker), numpy on the host: per_utterance = {"embedding" float32 [B,512] (zero rows where `valid` is 0),
    "valid" int32 [B]}; per_speaker = {speaker: the mean of the speaker's valid embeddings, float32 [512]} - what the reference saves as
    `{speaker}-spker_embed.npy`.  A speaker without a valid utterance is left out."""
    if len(wavs) == 0:
        raise ValueError("speaker_embeddings: empty batch")
    if len(speakers) != len(wavs):
        raise ValueError(f"speaker_embeddings: {len(speakers)} speakers for {len(wavs)} utterances")
    for w in wavs:
        if not torch.is_tensor(w) or not w.is_cuda:
            raise CttsError("speaker_embeddings computes on the MI355X: pass device tensors - no CPU fallback exists")
        if w.dim() != 1 or w.numel() < 1:
            raise ValueError(f"speaker_embeddings: each utterance is a non-empty 1-D tensor, got {tuple(w.shape)}")
    lens = [int(w.numel()) for w in wavs]
    wav = torch.zeros(len(wavs), max(lens), dtype=torch.float32, device=wavs[0].device)
    for i, w in enumerate(wavs):
        wav[i, :lens[i]] = w
    res = embedder(wav, lens, source_rate=source_rate)
    emb, valid = res["embedding"].cpu().numpy(), res["valid"].cpu().numpy()
    per_speaker = {}
    for spk in dict.fromkeys(speakers):
        rows = [i for i, s in enumerate(speakers) if s == spk and valid[i]]
        if rows:
            per_speaker[spk] = emb[rows].astype(np.float64).mean(0).astype(np.float32)
    return {"embedding": emb, "valid": valid}, per_speaker
