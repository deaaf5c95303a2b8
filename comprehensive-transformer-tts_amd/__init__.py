"""MI355X-native hot path for keonlee9420/Comprehensive-Transformer-TTS (CompTransTTS
forward / train step + the audio/stft.py mel front-end + the
hifigan/ vocoder's inference) behind the reference's own Python
surface.  See DESIGN.md.  Import as `ctts_amd` (root-level shim: the directory name
required by the build contract is not a valid Python identifier).

Importing the package never needs the GPU or the built library; the first kernel call loads
comprehensive-transformer-tts_amd/csrc/libctts_hip.so and raises if it is missing (no fallback)."""
from . import configs, synthetic  # noqa: F401
from . import _lib, kernels, ops, model, audio, loss, dp, conformer, vocoder, pitch_features, preprocess, metrics, resample, loudness, speaker  # noqa: F401
from .model import CompTransTTS, TextEncoder, Decoder, PostNet, VarianceAdaptor  # noqa: F401
from .audio import TacotronSTFT  # noqa: F401
from .vocoder import Generator as HiFiGANGenerator  # noqa: F401
from .pitch_features import track_pitch, f0_targets, pitch_targets_from_wav  # noqa: F401
from .preprocess import trim_silence, attention_prior, outlier_stats, merge_moments, DatasetStats, process_batch, process_batch_loudness, speaker_embeddings  # noqa: F401
from .metrics import mel_cepstrum, dtw, path_metrics, compare_mels, compare_wavs  # noqa: F401
from .metrics import stoi, si_sdr, mr_stft_distance, waveform_metrics, summarize_waveform, speaker_similarity  # noqa: F401
from .speaker import DeepSpeakerEmbedder  # noqa: F401
from .resample import resample_filter, peak_normalize  # noqa: F401  (the resampler itself is resample.resample: `resample` names the module)
from .loudness import kweighting, integrated_loudness, loudness_curve, normalize_loudness  # noqa: F401
