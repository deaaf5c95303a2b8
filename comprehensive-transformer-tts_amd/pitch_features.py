"""Pitch targets on the device: waveform -> F0 track -> the `p_targets` of the cwt pitch branch (csrc/pitchtrack.hip).

The reference makes these offline, one utterance at a time, with two third-party libraries: parselmouth (`get_pitch`,
utils/pitch_tools.py:85-132) and pycwt (`get_lf0_cwt`, :193-209), glued by `get_cont_lf0` (:152-190), `get_f0cwt`
(preprocessor.py:612-618) and the dataset's `norm_interp_f0` (:51-66).  Here a batch of utterances goes through three launches:

  track_pitch              Boersma-style autocorrelation tracker, a specified algorithm of this project (include/ctts.h) - NOT a clone
                           of parselmouth's `to_pitch_ac` (no path search across frames); framing is the mel kernel's, so f0 has the
                           mel's frame count by construction (the reference pads and trims, :109-120)
  f0_targets               uv, continuous log-F0, its mean / std, the 10-scale Mexican-hat CWT of the normalised contour, `valid`
  pitch_targets_from_wav   both, plus the model-side f0 target (`norm_interp_f0`), as the dict `CompTransTTS.forward` takes

PARITY UNPINNED against parselmouth and pycwt: neither library is installed where this project is built and tested.  The tracker does
not claim parselmouth's numbers.  The CWT restates pycwt's published definition (`cwt` with `MexicanHat`, dt = 0.005, dj = 1,
s0 = 0.01, J = 9); what pins it instead is a closed form (a cosine on an FFT bin) and the reference's own `inverse_cwt`
reconstructing the contour (tests/test_pitch_restate_cpu.py).  Everything else in the chain is pinned against the live reference
(tests/golden/g19_pitch_chain.npz).

All calls are stream-ordered and capturable (build the workspace first: `prepare(device)`); lengths are device tensors, nothing
synchronises, nothing runs on the CPU.
"""
import torch

from . import kernels as K
from ._lib import CttsError

_WS = {}


def prepare(device):
    """Build (once per device) the tracker's workspace - a kernel launch, so call it before capturing a graph."""
    device = torch.device(device)
    if device.type != "cuda":
        raise CttsError("pitch_features computes on the MI355X: pass device tensors - no CPU fallback exists")
    key = device.index if device.index is not None else torch.cuda.current_device()
    if key not in _WS:
        if torch.cuda.is_current_stream_capturing():
            raise CttsError("pitch_features: call prepare(device) before capturing a graph - the workspace is built by a kernel launch")
        _WS[key] = K.pitch_track_prepare(torch.device("cuda", key))
    return _WS[key]


def _device_lens(lens, B, dev, what):
    if lens is None:
        return None
    if not torch.is_tensor(lens) or not lens.is_cuda:
        raise CttsError(f"{what}: lengths must be a device tensor (no host round trip)")
    if lens.numel() != B:
        raise CttsError(f"{what}: {lens.numel()} lengths for a batch of {B}")
    return lens.to(torch.int32).contiguous().view(B)


def track_pitch(wav, lens=None, **params):
    """wav [B,N] float32 in [-1,1] (device), lens [B] samples (device, or None = N) -> (f0 [B,F] Hz with 0 = unvoiced, strength [B,F]),
    F = 1 + N // hop.  params: sr=22050, hop=256, f0_min=80, f0_max=750, voicing_threshold=0.6, silence_threshold=0.03."""
    if not torch.is_tensor(wav) or not wav.is_cuda:
        raise CttsError("track_pitch computes on the MI355X: pass wav as a device tensor - no CPU fallback exists")
    return K.pitch_track(wav, prepare(wav.device), _device_lens(lens, wav.shape[0], wav.device, "track_pitch"), **params)


def f0_targets(f0, frames):
    """f0 [B,F] Hz (0 = unvoiced), frames [B] (device) -> dict(uv [B,F], cont_lf0 [B,F], f0_mean [B], f0_std [B], cwt_spec [B,F,10],
    valid int32 [B]).  An utterance without a voiced frame, with a constant contour or with a non-finite result (which every utterance
    of two frames has: pycwt's normalisation is NaN at M = 2) has valid = 0 and all-zero rows; frames at or beyond frames[b] are zero."""
    if not torch.is_tensor(f0) or not f0.is_cuda:
        raise CttsError("f0_targets computes on the MI355X: pass f0 as a device tensor - no CPU fallback exists")
    uv, cont, mean_std, cwt, valid = K.f0_targets(f0, _device_lens(frames, f0.shape[0], f0.device, "f0_targets"))
    return {"uv": uv, "cont_lf0": cont, "f0_mean": mean_std[:, 0].contiguous(), "f0_std": mean_std[:, 1].contiguous(), "cwt_spec": cwt, "valid": valid}


def pitch_targets_from_wav(wav, lens, stft, mel2ph=None, eps=1e-9, **params):
    """wav [B,N], lens [B] samples (device) and the `TacotronSTFT` whose framing the mel uses -> the `p_targets` dict of
    `CompTransTTS.forward` for pitch_type "cwt": f0 [B,Tm] (log2, interpolated over unvoiced frames), uv [B,Tm], cwt_spec [B,Tm,10],
    f0_mean [B], f0_std [B], mel2ph (passed through), plus `pitch` (the raw track in Hz) and `valid` [B].  Tm = 1 + N // hop."""
    f0_hz, _ = track_pitch(wav, lens, sr=stft.sampling_rate, hop=stft.hop, **params)
    B, F = f0_hz.shape
    if lens is None:
        frames = torch.full((B,), F, dtype=torch.int32, device=wav.device)
    else:
        frames = (1 + torch.div(_device_lens(lens, B, wav.device, "pitch_targets_from_wav"), stft.hop, rounding_mode="floor")).to(torch.int32)
    t = f0_targets(f0_hz, frames)
    f0n, _ = K.norm_interp_f0(f0_hz, frames, eps)
    return {"pitch": f0_hz, "f0": f0n, "uv": t["uv"], "cwt_spec": t["cwt_spec"], "f0_mean": t["f0_mean"], "f0_std": t["f0_std"],
            "mel2ph": mel2ph, "valid": t["valid"]}
