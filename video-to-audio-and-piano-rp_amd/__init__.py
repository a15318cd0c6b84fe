"""MI355X-native flow-matching V2A sampler (drop-in for the reference's E2TTS sampling path).

Import name: `v2a_amd` (the directory name contains hyphens; the repo-root shim `v2a_amd.py`
registers this package under that name).
"""
from .dit import DiTConfig, DiTEngine, PackedWeights, NOTES  # noqa: F401
from .e2tts import E2TTS, E2TTSReturn, LossBreakdown, sway_grid, lens_to_mask, val_span_mask, expected_state_dict_shapes  # noqa: F401
from .collate import collate_clips, ClipRequest  # noqa: F401
from .dist import shard_range, gather_latents  # noqa: F401
from .features import (feature_cache_path, save_clip_cache, load_clip_cache, resample_indices,  # noqa: F401
                       resample_clip_features, encode_video_cached, piano_frames_cache_path, save_piano_frames_cache,
                       piano_frame_indices, load_piano_frames, encode_mixed_cached, piano_frames_from_video, load_midi_ground_truth,
                       PianoConfig, PIANO_51, PIANO_88, piano_config)
from .video2roll import Video2RollEngine  # noqa: F401
from .roll2midi import Roll2MidiEngine, Roll2MidiEnhanceEngine  # noqa: F401
from .encodec import EncodecDecoder, EncodecEncoder, EncodecQuantizer  # noqa: F401
from .t5 import T5Encoder  # noqa: F401
from .clip import CLIPImageEncoder, CLIPViT2ImageEncoder  # noqa: F401
from .dinov2 import DINOv2ImageEncoder  # noqa: F401
from .convnext import CLIPConvNeXtImageEncoder, MixedImageEncoder  # noqa: F401
from .piano_frames import PianoFramePlan, PianoFramePreprocessor  # noqa: F401
from .wave import WaveFrontEnd, sinc_resample_table  # noqa: F401
from .mel import MelSpec, mel_filterbank, stft_basis  # noqa: F401
from .vocos import Vocos, istft_basis  # noqa: F401
from .hifigan import HiFiGAN  # noqa: F401
from .audioldm_vae import AudioLDMVaeDecoder, VaeVocoder  # noqa: F401
from .midi import roll_to_notes, notes_to_roll, write_midi, read_midi  # noqa: F401
from . import midi  # noqa: F401
from . import _lib  # noqa: F401

__all__ = ["E2TTS", "DiTConfig", "DiTEngine", "PackedWeights", "collate_clips", "ClipRequest",
           "shard_range", "gather_latents", "sway_grid", "lens_to_mask", "val_span_mask", "E2TTSReturn", "LossBreakdown", "load_midi_ground_truth", "expected_state_dict_shapes", "NOTES",
           "Video2RollEngine", "Roll2MidiEngine", "Roll2MidiEnhanceEngine", "EncodecDecoder", "EncodecEncoder", "EncodecQuantizer", "T5Encoder", "CLIPImageEncoder", "CLIPViT2ImageEncoder", "DINOv2ImageEncoder", "CLIPConvNeXtImageEncoder", "MixedImageEncoder", "PianoFramePlan", "PianoFramePreprocessor",
           "WaveFrontEnd", "sinc_resample_table", "MelSpec", "mel_filterbank", "stft_basis", "Vocos", "istft_basis", "HiFiGAN", "AudioLDMVaeDecoder", "VaeVocoder", "roll_to_notes", "notes_to_roll", "write_midi", "read_midi", "PianoConfig", "PIANO_51", "PIANO_88", "piano_config"]
