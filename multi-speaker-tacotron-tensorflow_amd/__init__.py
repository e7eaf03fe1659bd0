"""taco_amd -- MI355X-native Tacotron hot path (CBHG encoder -> attention decoder -> post-net CBHG ->
linear spectrogram) behind the reference's Tacotron / Synthesizer surface.  Compute lives in
csrc/libtaco_hip.so (hand-written gfx950 HIP); this package is the thin host mirror."""
from .hparams import hparams, HParams, basic_params, load_hparams, save_hparams   # noqa: F401
from .tacotron import Tacotron, create_model, input_lengths_from_tokens, speaker_weights  # noqa: F401
from .synthesizer import Synthesizer                                               # noqa: F401
from .audio import GriffinLim, Spectrogram, Resampler                                   # noqa: F401
from .trainer import Trainer                                                       # noqa: F401
from .feeder import DeviceCorpus                                                   # noqa: F401
from .silence import split_on_silence, split_on_silence_pydub, amplify             # noqa: F401
from .alignment import align_texts, align_text_batch                                # noqa: F401
from .metrics import dtw_distance, mel_cepstral_distortion, f0_track, f0_errors, prosody_distance  # noqa: F401
from .prosody import warp_map, semitones_to_scale, warp_formant                           # noqa: F401
from . import audio, weights, dist, _lib, train_ops, tf_checkpoint, text, korean, feeder, silence, alignment, metrics, prosody  # noqa: F401
