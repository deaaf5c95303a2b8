"""DeepSpeaker speaker embeddings on the device (csrc/speaker.hip): what the reference's `PreDefinedEmbedder`
computes for `speaker_embedder: "DeepSpeaker"` (preprocessor.py:376, deepspeaker/embedding.py:13-27) - the 512-d vector CompTransTTS
takes as `spker_embeds` - without TensorFlow.  The float64 restatement in tests/speaker_restate.py is the contract; PARITY with the TF
model and python_speech_features is UNPINNED (neither is installed where this project is built, and the pretrained checkpoint is not
part of the reference checkout).

Per utterance (a ragged batch wav [B, N] float32 with lens):

1. Voice span (audio_ds.read_mfcc): thr = np.percentile(|x|, 95), linear interpolation, formed in double from the two fp32 order
   statistics a[k], a[k+1] around the virtual index 0.95 (n - 1), evaluated as numpy evaluates it; first / last = the lowest / highest
   index with |x| > thr; the span is x[first:last] (last excluded, as in the reference).  valid = 0 when no sample qualifies or
   last - first < 1: the reference raises there, here the embedding is all zeros and the flag says so.
2. Filterbank features (python_speech_features.fbank(samplerate=22050, nfilt=64, nfft=1024), then audio_ds.normalize_frames):
   pre-emphasis 0.97 inside the span, frames of 551 samples at step 221 (1 frame up to 551 samples, else 1 + ceil((L - 551) / 221), the
   tail zero-padded), rectangular window, |rfft(frame, 1024)|^2 / 1024, 64 triangular HTK-mel filters on the integer bins
   floor(1025 hz / 22050) of 66 mel-equidistant points, NO logarithm, exact zeros -> 2^-52, then (v - mean) / max(std, 1e-12) over the
   64 filters (population std).  float32 [frames, 64].
3. Crop or pad to 160 frames (batcher.sample_from_mfcc): shorter inputs get zero rows, longer ones are cut to [r, r + 160).
   DEVIATION: the reference draws r at random; here `frame_offset=None` takes the centre crop r = (F - 160) // 2, and an int tensor [B]
   gives explicit offsets (0 <= r <= max(F - 160, 0)), which reproduces any draw of the reference.
4. ResCNN (conv_models.py) on NHWC activations [B, 160, 64, 1]: for C in 64, 128, 256, 512 a 5 x 5 stride-2 'same' convolution + BN +
   clip to [0, 20], then three identity blocks conv3x3-BN-clip-conv3x3-BN-clip, + block input, clip.  BatchNorm in inference form
   with Keras's eps = 1e-3, folded into the convolution's weight and bias in float64 when the weights are loaded.  Then
   Reshape((-1, 2048)) (10 time steps, feature index w 512 + c), mean over the steps, Dense(2048 -> 512), x / max(||x||, 1e-12).

The rate is 22050 Hz: the reference hands the dataset's rate to `fbank` and the constants above are 22050's.  Audio at another rate
(VCTK's 48 kHz) is resampled first: pass `source_rate=`.  Device tensors only - there is no CPU path."""
import numpy as np
import torch

from . import kernels as K
from ._lib import CttsError
from .audio import _lens_arg

SAMPLE_RATE = 22050
NUM_FRAMES, NUM_FBANKS, EMBED_DIM = 160, 64, 512
FRAME_LEN, FRAME_STEP, NFFT = 551, 221, 1024
BN_EPS = 1e-3
CLIP_LO, CLIP_HI = 0.0, 20.0
STAGES = (64, 128, 256, 512)


def layer_names():
    """conv layers of the ResCNN in execution order: (name, kernel size, cin, cout)"""
    out, cin = [], 1
    for stage, c in enumerate(STAGES, 1):
        out.append((f"conv{c}-s", 5, cin, c))
        for block in range(3):
            for branch in ("2a", "2b"):
                out.append((f"res{stage}_{block}_branch_{branch}", 3, c, c))
        cin = c
    return out


def weight_shapes():
    """the mapping "<keras layer>/<var>" -> shape a `DeepSpeakerEmbedder` needs"""
    shapes = {}
    for name, k, cin, cout in layer_names():
        shapes[f"{name}/kernel"] = (k, k, cin, cout)
        shapes[f"{name}/bias"] = (cout,)
        for var in ("gamma", "beta", "moving_mean", "moving_variance"):
            shapes[f"{name}_bn/{var}"] = (cout,)
    shapes["affine/kernel"] = (4 * STAGES[-1], EMBED_DIM)
    shapes["affine/bias"] = (EMBED_DIM,)
    return shapes


def fbank_bins(samplerate=SAMPLE_RATE, nfilt=NUM_FBANKS, nfft=NFFT):
    """python_speech_features.get_filterbanks: floor((nfft + 1) hz / samplerate) of nfilt + 2 points equidistant in HTK mel"""
    high = 2595.0 * np.log10(1.0 + (samplerate / 2.0) / 700.0)
    mel = np.linspace(0.0, high, nfilt + 2)
    hz = 700.0 * (10.0 ** (mel / 2595.0) - 1.0)
    return np.floor((nfft + 1) * hz / samplerate).astype(np.int32)


def n_frames_of(span):
    """fbank frames of a span of `span` samples (host ints)"""
    span = int(span)
    return 0 if span < 1 else (1 if span <= FRAME_LEN else 1 + -(-(span - FRAME_LEN) // FRAME_STEP))


def fold_batchnorm(kernel, bias, gamma, beta, mean, var, eps=BN_EPS):
    """conv + inference BatchNorm as one conv, in float64: w' = w g / sqrt(var + eps), b' = (b - mean) g / sqrt(var + eps) + beta"""
    s = np.asarray(gamma, np.float64) / np.sqrt(np.asarray(var, np.float64) + eps)
    return np.asarray(kernel, np.float64) * s, (np.asarray(bias, np.float64) - np.asarray(mean, np.float64)) * s + np.asarray(beta, np.float64)


class DeepSpeakerEmbedder:
    """embedder = DeepSpeakerEmbedder(weights).to("cuda"); embedder(wav, lens)["embedding"] -> [B, 512].
    `weights`: a mapping "<keras layer>/<var>" -> array (`weight_shapes()` lists the keys: the conv layers `conv64-s`,
    `res1_0_branch_2a` ... `res4_2_branch_2b` with kernel [kh, kw, cin, cout] and bias, their `_bn` twins with gamma, beta, moving_mean,
    moving_variance, and `affine` with kernel [2048, 512] and bias).  Missing, extra or wrongly shaped entries are refused by key."""

    def __init__(self, weights, device=None, sampling_rate=SAMPLE_RATE):
        if int(sampling_rate) != SAMPLE_RATE:
            raise CttsError(f"DeepSpeakerEmbedder: the front end's constants are those of {SAMPLE_RATE} Hz, got sampling_rate "
                            f"{sampling_rate}; resample first (source_rate=)")
        shapes = weight_shapes()
        given = dict(weights)
        for key in shapes:
            if key not in given:
                raise CttsError(f"DeepSpeakerEmbedder: weight '{key}' is missing")
        for key in given:
            if key not in shapes:
                raise CttsError(f"DeepSpeakerEmbedder: unexpected weight '{key}'")
        self.weights = {}
        for key, shape in shapes.items():
            a = np.asarray(given[key].detach().cpu().numpy() if torch.is_tensor(given[key]) else given[key])
            if tuple(a.shape) != shape:
                raise CttsError(f"DeepSpeakerEmbedder: weight '{key}' has shape {tuple(a.shape)}, expected {shape}")
            if not np.isfinite(a).all():
                raise CttsError(f"DeepSpeakerEmbedder: weight '{key}' is not finite")
            self.weights[key] = np.ascontiguousarray(a, dtype=np.float32)
        self.device = None
        self._convs = self._affine = self._bins = None
        if device is not None:
            self.to(device)

    # ---- weights in and out
    def save_npz(self, path):
        np.savez(path, **self.weights)

    @classmethod
    def from_npz(cls, path, device=None):
        with np.load(path) as z:
            return cls({k: z[k] for k in z.files}, device)

    @classmethod
    def from_h5(cls, path, device=None):
        """a Keras `save_weights` file or a whole-model checkpoint (`model_weights` group): every dataset whose path ends in
        `<layer>/<var>:0` for a layer and variable of `weight_shapes()`"""
        try:
            import h5py
        except ImportError as e:
            raise ImportError("DeepSpeakerEmbedder.from_h5 needs h5py to read Keras checkpoints; convert the checkpoint to npz where h5py "
                              "is installed (save_npz) or install h5py") from e
        shapes, found = weight_shapes(), {}

        def visit(name, obj):
            if isinstance(obj, h5py.Dataset) and name.endswith(":0"):
                parts = name[:-2].split("/")
                if len(parts) >= 2 and f"{parts[-2]}/{parts[-1]}" in shapes:
                    found[f"{parts[-2]}/{parts[-1]}"] = np.asarray(obj)

        with h5py.File(path, "r") as f:
            f.visititems(visit)
        return cls(found, device)

    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise CttsError("DeepSpeakerEmbedder computes on the MI355X: needs a HIP device - no CPU fallback exists")
        w = self.weights
        self._convs = []
        for name, k, cin, cout in layer_names():
            wk, wb = fold_batchnorm(w[f"{name}/kernel"], w[f"{name}/bias"], w[f"{name}_bn/gamma"], w[f"{name}_bn/beta"],
                                    w[f"{name}_bn/moving_mean"], w[f"{name}_bn/moving_variance"])
            self._convs.append((torch.from_numpy(wk.astype(np.float32)).to(device), torch.from_numpy(wb.astype(np.float32)).to(device)))
        self._affine = (torch.from_numpy(w["affine/kernel"]).to(device), torch.from_numpy(w["affine/bias"]).to(device))
        self._bins = torch.from_numpy(fbank_bins()).to(device)
        self.device = device
        return self

    # ---- the computation
    def _batch(self, wav, lens, source_rate, what):
        if not torch.is_tensor(wav) or not wav.is_cuda:
            raise CttsError(f"{what} computes on the MI355X: pass device tensors - no CPU fallback exists")
        if wav.dim() != 2 or wav.shape[0] < 1 or wav.shape[1] < 1:
            raise CttsError(f"{what}: expected a non-empty [B, N] tensor, got {tuple(wav.shape)}")
        if self.device is None or self.device != wav.device:
            self.to(wav.device)
        wav = wav.float().contiguous()
        B, N = wav.shape
        lens = _lens_arg([N] * B if lens is None else lens, B, 0, N, f"{what} lens", wav.device)
        if source_rate is not None and int(source_rate) != SAMPLE_RATE:
            from . import resample as RS
            wav, lens = RS.resample(wav, lens, int(source_rate), SAMPLE_RATE)
        return wav, lens

    def features(self, wav, lens=None, source_rate=None):
        """the ragged normalised fbank features: {"fbank" [B, Fmax, 64] (zero rows at and beyond n_frames), "n_frames", "first", "last",
        "valid" int32 [B]}; Fmax is the frame count of a span of N samples"""
        wav, lens = self._batch(wav, lens, source_rate, "DeepSpeakerEmbedder.features")
        first, last, frames, valid = K.speaker_span(wav, lens)
        fb = K.speaker_fbank(wav, first, last, valid, self._bins, max(n_frames_of(wav.shape[1]), 1))
        return {"fbank": fb, "n_frames": frames, "first": first, "last": last, "valid": valid}

    def stage(self, x, i):
        """stage i (0-based) of the ResCNN on NHWC x: the strided convolution and its three identity blocks, seven launches"""
        convs = self._convs[7 * i:7 * i + 7]
        x = K.conv2d_nhwc(x, convs[0][0], convs[0][1], K.CONV_K5S2_SAME, CLIP_LO, CLIP_HI)
        for j in range(3):
            (wa, ba), (wb, bb) = convs[1 + 2 * j], convs[2 + 2 * j]
            y = K.conv2d_nhwc(x, wa, ba, K.CONV_K3S1, CLIP_LO, CLIP_HI)
            x = K.conv2d_nhwc(y, wb, bb, K.CONV_K3S1, CLIP_LO, CLIP_HI, res=x)
        return x

    def forward_features(self, fb, return_stages=False, valid=None):
        """fb [B, 160, 64] float32 -> embedding [B, 512]; with return_stages also the four stage outputs, NHWC
        [B,80,32,64], [B,40,16,128], [B,20,8,256], [B,10,4,512]"""
        if not torch.is_tensor(fb) or not fb.is_cuda:
            raise CttsError("DeepSpeakerEmbedder.forward_features computes on the MI355X: pass device tensors - no CPU fallback exists")
        if fb.dim() != 3 or fb.shape[2] != NUM_FBANKS or fb.shape[1] != NUM_FRAMES:
            raise CttsError(f"DeepSpeakerEmbedder.forward_features: expected [B, {NUM_FRAMES}, {NUM_FBANKS}], got {tuple(fb.shape)}")
        if self.device is None or self.device != fb.device:
            self.to(fb.device)
        x = fb.float().contiguous().unsqueeze(-1)
        stages = []
        for i in range(len(STAGES)):
            x = self.stage(x, i)
            stages.append(x)
        B, T = x.shape[0], x.shape[1]
        emb = K.speaker_head(x.view(B, T, -1), self._affine[0], self._affine[1], valid)
        return (emb, stages) if return_stages else emb

    def __call__(self, wav, lens=None, frame_offset=None, source_rate=None):
        """wav [B, N] float32 at 22050 Hz (or at `source_rate`: resampled first), lens [B] -> {"embedding" [B, 512] float32, "first",
        "last", "n_frames", "valid" int32 [B]}, all on the device.  frame_offset: None = the centre crop (no host sync), or [B] ints with
        0 <= r <= max(n_frames - 160, 0), checked on the host.  Invalid rows give a zero embedding."""
        wav, lens = self._batch(wav, lens, source_rate, "DeepSpeakerEmbedder")
        B = wav.shape[0]
        first, last, frames, valid = K.speaker_span(wav, lens)
        offs = None
        if frame_offset is not None:
            offs = torch.as_tensor(frame_offset).to(device=wav.device, dtype=torch.int32).contiguous().view(-1)
            if offs.numel() != B:
                raise CttsError(f"DeepSpeakerEmbedder: {offs.numel()} frame offsets for a batch of {B}")
            bad = (offs < 0) | (offs > (frames - NUM_FRAMES).clamp(min=0))
            if bool(bad.any()):
                i = int(bad.nonzero()[0])
                raise CttsError(f"DeepSpeakerEmbedder: frame_offset[{i}] = {int(offs[i])} is outside [0, max(n_frames - {NUM_FRAMES}, 0)] "
                                f"for n_frames = {int(frames[i])}")
        fb = K.speaker_fbank(wav, first, last, valid, self._bins, NUM_FRAMES, offsets=offs, centre=offs is None)
        emb = self.forward_features(fb, valid=valid)
        return {"embedding": emb, "first": first, "last": last, "n_frames": frames, "valid": valid}
