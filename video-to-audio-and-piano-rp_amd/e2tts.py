"""Drop-in `E2TTS` for the sampling path: same constructor keywords, `sample()`,
`transformer_with_pred_head()`, `cfg_transformer_with_pred_head()`, the validation pass `forward(val=True)` and checkpoint key
layout as the reference class (x3:1275-1318, 1993-2113, 2127-2305, 2307-2588; `x3` =
/root/reference/src/e2_tts_pytorch/e2_tts_crossatt3.py), running on the HIP kernels of
include/v2a_cfm.h.  Callers: predict.py:266, app.py:267, src/inference_v2a.py:183,
src/inference_v2p.py:183.

Scope: the Euler/CFG loop over the DiT.  The encoders that feed it run
once per clip and are out of scope, so their outputs are passed in through keyword-only
extensions (`text_embed`, `context`, `context_mask`, `frames_embed`, `y0`) or produced by
user-supplied callables (`video_encoder_fn`, `text_encoder_fn`, `frames_encoder_fn`).  The
reference draws the initial noise on the device inside sample() (x3:2248); `y0` makes it
injectable so results can be compared across devices.

There is no fallback path: without libv2a_cfm.so (gfx950) construction raises.
"""
from __future__ import annotations

import os
from collections import namedtuple
from pathlib import Path
from typing import Callable

import numpy as np
import torch

from . import _lib as L
from .clip import CLIPImageEncoder, CLIPViT2ImageEncoder
from .convnext import CLIPConvNeXtImageEncoder, MixedImageEncoder, MIXED_ORDER, is_convnext_state_dict
from .dinov2 import DINOv2ImageEncoder
from .dit import DiTConfig, DiTEngine, NOTES, process_streams

IMAGE_ENCODERS = {"clip_vit": CLIPImageEncoder, "clip_vit2": CLIPViT2ImageEncoder, "clip_convnext": CLIPConvNeXtImageEncoder,
                  "dinov2": DINOv2ImageEncoder, "mixed": MixedImageEncoder}     # video_encoder -> its HIP encoder

LossBreakdown = namedtuple("LossBreakdown", ["flow", "velocity_consistency", "a", "b"])                     # x3:132
E2TTSReturn = namedtuple("E2TTS", ["loss", "cond", "pred_flow", "pred_data", "loss_breakdown"])               # x3:134
_IncompatibleKeys = namedtuple("_IncompatibleKeys", ["missing_keys", "unexpected_keys"])
_V2R_PREFIX = "video2roll_net."


def lens_to_mask(t: torch.Tensor, length: int | None = None) -> torch.Tensor:
    """x3:296-305."""
    if length is None:
        length = int(t.amax())
    seq = torch.arange(length, device=t.device)
    return seq[None, :] < t[:, None]


def val_span_mask(lens: torch.Tensor, n: int) -> torch.Tensor:
    """The infilling span of the validation pass, (b, n) bool: `mask_from_frac_lengths(lens, frac, max_length=n, val=True) & mask`
    with frac = (0.7 + 1.0) / 2 (x3:316-337, 2358-2362), in the reference's torch float32 ops on the host: 85 % of every clip, centred."""
    lens = torch.as_tensor(lens).cpu().long()
    frac = torch.tensor([(0.7 + 1.0) / 2.0] * lens.shape[0]).float()
    lengths = (frac * lens).long()
    start = ((lens - lengths) * torch.tensor([0.5] * lens.shape[0]).float()).long().clamp(min=0)
    seq = torch.arange(int(n))
    span = (seq[None, :] >= start[:, None]) & (seq[None, :] < (start + lengths)[:, None])
    return span & lens_to_mask(lens, int(n))


def sway_grid(steps: int, sway_sampling: bool = True) -> torch.Tensor:
    """x3:2250-2252, evaluated in fp32 on the host (same op order as the reference)."""
    t = torch.linspace(0, 1, steps)
    if sway_sampling:
        t = t + -1.0 * (torch.cos(torch.pi / 2 * t) - 1 + t)
    return t


def expected_state_dict_shapes(cfg: DiTConfig) -> dict[str, tuple]:
    """Key layout of the sampled path inside a reference checkpoint (nested ModuleList
    indices of x3:824-933; SURVEY section 5 'Checkpoint / resume')."""
    d, dt, df, k = cfg.dim, cfg.dim_text, cfg.dim_frames, cfg.kernel_size
    inner, ih, fh = cfg.heads * cfg.dim_head, cfg.heads, cfg.frames_heads
    s: dict[str, tuple] = {}

    def attn(p, dim, heads, ctx=None):
        inn = heads * cfg.dim_head
        s[f"{p}.to_q.weight"] = (inn, dim)
        s[f"{p}.to_k.weight"] = (inn, ctx or dim)
        s[f"{p}.to_v.weight"] = (inn, ctx or dim)
        s[f"{p}.to_v_head_gate.weight"] = (heads, dim)
        s[f"{p}.to_v_head_gate.bias"] = (heads,)
        s[f"{p}.to_out.weight"] = (dim, inn)

    def ff(p, dim, mult):
        s[f"{p}.ff.0.proj.weight"] = (2 * dim * mult, dim)
        s[f"{p}.ff.0.proj.bias"] = (2 * dim * mult,)
        s[f"{p}.ff.2.weight"] = (dim, dim * mult)
        s[f"{p}.ff.2.bias"] = (dim,)

    def conv(p, dim):
        s[f"{p}.dw_conv1d.0.weight"] = (dim, 1, k)
        s[f"{p}.dw_conv1d.0.bias"] = (dim,)

    T = "transformer"
    s[f"{T}.abs_pos_emb.weight"] = (cfg.max_seq_len, d)
    s[f"{T}.registers"] = (cfg.num_registers, d)
    s[f"{T}.text_registers"] = (cfg.num_registers, dt)
    s[f"{T}.frames_registers"] = (cfg.num_registers, df)
    s[f"{T}.time_cond_mlp.0.weights"] = (d // 2,)
    s[f"{T}.time_cond_mlp.1.weight"] = (d, d + 1)
    s[f"{T}.time_cond_mlp.1.bias"] = (d,)
    for i in range(cfg.depth):
        P = f"{T}.layers.{i}"
        if i >= cfg.depth // 2:
            s[f"{P}.0.0.weight"] = (d, 2 * d)
        conv(f"{P}.0.1", d)
        for j in (2, 5, 8):
            s[f"{P}.0.{j}.to_gamma.weight"] = (d, d)
        for j in (4, 7, 10):
            s[f"{P}.0.{j}.to_gamma.weight"] = (d, d)
            s[f"{P}.0.{j}.to_gamma.bias"] = (d,)
        attn(f"{P}.0.3", d, ih)
        attn(f"{P}.0.6", d, ih, cfg.ctx_dim)
        ff(f"{P}.0.9", d, cfg.ff_mult)
        conv(f"{P}.1.0", dt)
        s[f"{P}.1.1.g"] = (dt,)
        attn(f"{P}.1.2", dt, ih)
        s[f"{P}.1.3.g"] = (dt,)
        ff(f"{P}.1.4", dt, cfg.ff_mult)
        s[f"{P}.1.5.text_frames_to_audio.weight"] = (d, d + dt + df)
        if i != cfg.depth - 1:
            s[f"{P}.1.5.audio_to_text.weight"] = (dt, d + dt)
            s[f"{P}.1.5.audio_to_frames.weight"] = (df, d + df)
        conv(f"{P}.2.0", df)
        s[f"{P}.2.1.g"] = (df,)
        attn(f"{P}.2.2", df, fh)
        s[f"{P}.2.3.g"] = (df,)
        ff(f"{P}.2.4", df, 4)
    s[f"{T}.final_norm.g"] = (d,)
    s["proj_in.weight"] = (d, cfg.num_channels)
    s["proj_in.bias"] = (d,)
    s["to_pred.weight"] = (cfg.num_channels, d)
    s["to_pred.bias"] = (cfg.num_channels,)
    s["proj_frames.weight"] = (df, cfg.notes)
    s["proj_frames.bias"] = (df,)
    if cfg.cond_proj_in:                      # x3:1365 (bias optional: cond_proj_in_bias)
        s["cond_proj_in.weight"] = (d, cfg.num_channels)
        s["cond_proj_in.bias"] = (d,)
    return s


class E2TTS:
    def __init__(
        self,
        transformer: dict | None = None,
        duration_predictor=None,
        odeint_kwargs: dict = dict(method="euler"),
        audiocond_drop_prob=0.30,
        cond_drop_prob=0.20,
        prompt_drop_prob=0.10,
        num_channels=None,
        mel_spec_module=None,
        char_embed_kwargs: dict = dict(),
        mel_spec_kwargs: dict = dict(),
        frac_lengths_mask=(0.7, 1.0),
        audiocond_snr=None,
        concat_cond=False,
        interpolated_text=False,
        text_num_embeds=None,
        tokenizer="char_utf8",
        use_vocos=True,
        pretrained_vocos_path="charactr/vocos-mel-24khz",
        sampling_rate=None,
        frame_size: int = 320,
        velocity_consistency_weight=-1e-5,
        if_cond_proj_in=True,
        cond_proj_in_bias=True,
        if_embed_text=True,
        if_text_encoder2=True,
        if_clip_encoder=False,
        video_encoder="clip_vit",
        *,
        # ---- build-side extensions (keyword-only) ----
        compute_dtype: str = "bf16x3",       # "bf16x3" (default: split-bf16 GEMMs, inside 1e-3 of the fp32 reference path, config.yaml:7) | "bf16" (2x faster, ~5e-2 off) | "fp32" (exact-fp32 MFMA)
        device="cuda",
        rope_layout: str = "interleaved",
        rope_cross: bool = False,            # x-transformers 1.37.4 ignores rotary_pos_emb when a context is given; True = the other reading
        use_graph: bool = True,              # capture the Euler step in a hipGraph
        bucket_frames: int = 0,              # > 0: plans are padded to a multiple of this many latent frames (ragged masks hide the padding)
        bucket_ctx: int = 0,                 # > 0: ... and to a multiple of this many context tokens (context_mask hides the padding)
        video_encoder_fn: Callable | None = None,   # (video_paths, n) -> (b, n, dim_text)
        text_encoder_fn: Callable | None = None,    # (prompts) -> ((b, nc, ctx) float, (b, nc) bool)
        frames_encoder_fn: Callable | None = None,  # (frames, n) -> (b, n, NOTES)
        frames_compute_dtype: str | None = None,    # Video2Roll encoder mode: None = "bf16" under compute_dtype "bf16", else "fp32"; or "fp32" | "bf16" | "bf16x3"
        piano_keys: int = 51,                       # 51: e2_tts_crossatt3.py | 88: e2_tts_crossatt3_2.py, the reference's 88-key piano configuration (features.PianoConfig)
    ):
        if not isinstance(transformer, dict):
            raise TypeError("transformer must be the keyword dict of the reference (predict.py:120-134)")
        if odeint_kwargs.get("method", "euler") != "euler":
            raise NotImplementedError("only the fixed-grid Euler solver of the shipped config is built (x3:1282-1287)")
        if concat_cond:
            raise NotImplementedError("concat_cond=True is not used by any shipped caller")
        tk = dict(transformer)
        for flag in ("if_text_modules", "if_cross_attn", "if_audio_conv", "if_text_conv"):
            if not tk.pop(flag, flag != "if_text_conv"):
                raise NotImplementedError(f"{flag}=False: only the shipped configuration (all True, predict.py:126-129) is built")
        tk.pop("cond_on_time", None)
        from .features import piano_config
        self.piano = piano_config(piano_keys)          # notes, note range, video_multi, roll expansion, frame layout
        if tk.setdefault("notes", self.piano.notes) != self.piano.notes:
            raise ValueError(f"transformer['notes']={tk['notes']} contradicts piano_keys={self.piano.notes}")
        if num_channels is None:
            raise ValueError("num_channels is required (predict.py:152)")
        self.cfg = DiTConfig(num_channels=num_channels, cond_proj_in=bool(if_cond_proj_in), **tk)
        self.cond_proj_in_bias = bool(cond_proj_in_bias)
        self.audiocond_snr = audiocond_snr
        self.dim, self.dim_text = self.cfg.dim, self.cfg.dim_text
        self.num_channels = num_channels
        self.sampling_rate = sampling_rate
        self.frame_size = frame_size
        self.audiocond_drop_prob, self.cond_drop_prob, self.prompt_drop_prob = audiocond_drop_prob, cond_drop_prob, prompt_drop_prob
        self.duration_predictor = duration_predictor
        self.mel_spec = mel_spec_module
        self.vocos = None
        self.video_encoder = video_encoder
        self.training = False
        self._device = torch.device(device)
        if compute_dtype not in ("bf16", "fp32", "bf16x3"):
            raise ValueError(f"compute_dtype must be 'bf16', 'fp32' or 'bf16x3', got {compute_dtype!r}")
        self._compute = compute_dtype
        if frames_compute_dtype is not None and frames_compute_dtype not in ("bf16", "fp32", "bf16x3"):
            raise ValueError(f"frames_compute_dtype must be None, 'bf16', 'fp32' or 'bf16x3', got {frames_compute_dtype!r}")
        self._frames_compute = frames_compute_dtype or ("bf16" if compute_dtype == "bf16" else "fp32")
        self._rope = (rope_layout, rope_cross)
        self._use_graph = use_graph
        # Shape buckets: captions and durations vary per clip (predict.py:210-237), and every new (frames, context) shape costs a
        # plan, an eager warm-up evaluation and a graph capture.  With buckets, sample() pads the latent frames and the context to
        # the bucket and lets the length masks (lens_to_mask x3:296-305, context_mask) hide the padding; results of the valid
        # frames do not change (tests/test_sampler_gpu.py::test_plan_cache_and_buckets).  0 = exact shapes.
        self.bucket_frames, self.bucket_ctx = int(bucket_frames), int(bucket_ctx)
        self.graph_captures = 0              # hipGraph captures so far (a plan / graph cache hit leaves it unchanged)
        self.video_encoder_fn, self.text_encoder_fn, self.frames_encoder_fn = video_encoder_fn, text_encoder_fn, frames_encoder_fn
        self._shapes = expected_state_dict_shapes(self.cfg)
        self._sd: dict[str, torch.Tensor] = {}
        self._engine: DiTEngine | None = None
        self._v2r_sd, self._v2r = None, None      # optional Video2Roll frame encoder (video2roll_net.*, x3:1523)
        self._t5 = None                           # optional FLAN-T5 prompt encoder (load_text_encoder, x3:1412-1413)
        self._clip = None                         # optional image encoder (load_image_encoder: CLIP x3:1423-1428 or DINOv2 x3:1432-1433)
        self._audio_encoder = None                # optional Encodec encoder behind a raw-wave cond (load_audio_encoder, x3:1350)
        self._audio_quantizer = None              # optional Encodec quantizer behind an integer cond of codes (load_audio_quantizer)
        self._wave_front_end = None               # resample + normalize_wav in front of the audio encoder (encode_audio), made on first use
        self._piano_pre = None                    # piano-frame preprocessor of this device (piano_frame_preprocessor, x3:1877-1891)
        self._r2m = None                          # optional Roll2Midi generator behind frames_to_midi (load_roll2midi)
        L.lib()  # no library -> no sampler

    # ---- nn.Module-like surface used by the callers (predict.py:156-170) -------------------
    @property
    def device(self):
        return self._device

    def to(self, device):
        self._device = torch.device(device)
        self._engine = None
        self._v2r = None
        self._piano_pre = None
        if self._clip is not None:
            self._clip.to(self._device)        # weights follow, buffers and tables are rebuilt on first use
        return self

    def eval(self):
        self.training = False
        return self

    def parameters(self):
        return iter(self._sd.values())

    def state_dict(self):
        sd = dict(self._sd)
        if self._v2r_sd is not None:
            sd.update({_V2R_PREFIX + k: v for k, v in self._v2r_sd.items()})
        return sd

    def load_state_dict(self, state_dict, strict: bool = True):
        """Accepts a reference checkpoint's `model_state_dict` (predict.py:168, strict=False there):
        keys of the sampled path are taken, encoder / vocoder / training-only keys are reported as
        unexpected."""
        missing, unexpected, new = [], [], {}
        for k, shp in self._shapes.items():
            if k == "cond_proj_in.bias" and not self.cond_proj_in_bias:
                new[k] = torch.zeros(shp)
                continue
            if k in state_dict:
                v = state_dict[k]
                if tuple(v.shape) != tuple(shp):
                    raise RuntimeError(f"size mismatch for {k}: checkpoint {tuple(v.shape)} vs model {tuple(shp)}")
                new[k] = v.detach().to("cpu", torch.float32).contiguous()
            else:
                missing.append(k)
        # optional: the Video2Roll frame encoder (`video2roll_net.*`, x3:1523) -- taken when the checkpoint holds it whole
        v2r = {k[len(_V2R_PREFIX):]: v.detach().to("cpu") for k, v in state_dict.items() if k.startswith(_V2R_PREFIX)}
        if v2r:
            from .video2roll import expected_state_dict_shapes as v2r_shapes
            lacking = [k for k in v2r_shapes() if k not in v2r and not k.endswith("num_batches_tracked")]
            if lacking:
                raise RuntimeError(f"load_state_dict: {_V2R_PREFIX}* is incomplete, e.g. {lacking[:3]}")
            if v2r["fc.weight"].shape[0] != self.cfg.notes:
                raise RuntimeError(f"size mismatch for {_V2R_PREFIX}fc.weight: checkpoint {tuple(v2r['fc.weight'].shape)} vs model "
                                   f"({self.cfg.notes}, 128): a checkpoint of the other piano configuration (E2TTS(piano_keys=...))")
            self._v2r_sd, self._v2r = v2r, None
        unexpected = [k for k in state_dict if k not in self._shapes and not k.startswith(_V2R_PREFIX)]
        if strict and (missing or unexpected):
            raise RuntimeError(f"load_state_dict(strict=True): missing {missing[:5]}..., unexpected {unexpected[:5]}...")
        self._sd.update(new)
        self._engine = None          # plans and their graphs go with the engine
        return _IncompatibleKeys(missing, unexpected)

    def engine(self) -> DiTEngine:
        if self._engine is None:
            absent = [k for k in self._shapes if k not in self._sd]
            if any(k.startswith("cond_proj_in.") for k in absent):
                # a checkpoint of the shipped configuration has no audio-prompt projection (predict.py:144): the sampler runs
                # without it and the infilling branch raises, as the reference's `None(cond)` would (x3:2034)
                absent = [k for k in absent if not k.startswith("cond_proj_in.")]
                self.cfg.cond_proj_in = False
            if absent:
                raise RuntimeError(f"{len(absent)} parameters were never loaded (e.g. {absent[0]}): call load_state_dict first")
            self._engine = DiTEngine(self.cfg, {k: v for k, v in self._sd.items() if self.cfg.cond_proj_in or not k.startswith("cond_proj_in.")},
                                     self._device, compute=self._compute,
                                     rope_layout=self._rope[0], rope_cross=self._rope[1])
        return self._engine

    # ---- conditioning helpers ---------------------------------------------------------------
    def encode_frames(self, x, l: int):
        """x3:1525-1553: (b, 1, t, 100, 900) grey frames -> piano-roll probabilities (b, l, notes) on the HIP Video2Roll
        encoder (video2roll.py): every frame's row x3 in time, or x2.5 under piano_keys=88 (x3_2:1546-1547).  Needs the
        `video2roll_net.*` weights of the checkpoint (load_state_dict)."""
        if self._v2r_sd is None:
            raise RuntimeError("encode_frames: no `video2roll_net.*` weights were loaded (load_state_dict), pass "
                               "frames_embed= or frames_encoder_fn= instead")
        return self._video2roll().encode_frames(x, l)

    def encode_video_frames(self, video_paths, l: int, piano, *, video_frames=None):
        """x3:1829-1991, the `piano` branch: the grey frame stacks of a batch of clips and the (unused) MIDI ground truth,
        `(frames (b, 1, t, 100, 900), midis (b, l, NOTES) zeros)`, or `(None, None)` when `piano` is false or no clip has frames.
        One video frame per `piano.video_multi` latent frames (3.0, or 2.5 under piano_keys=88, x3_2:1929-1930).
        `video_frames`: one (frames uint8 (F, H, W, 3), duration_s) or None per clip, the convention of `sample` -- not to be
        confused with `_encode_video_frames`, the CLIP batcher over the same list.  A clip with a frame cache
        `<video>.generated_frames_raw.2.npz` is read from it; one without goes through the HIP piano-frame preprocessor
        (piano_frames.py), all its frames, and its cache is written (x3:1877-1891).  `video_paths=None`: the clips have no
        place for a cache, only the frames each one uses are resized and nothing is written.  The stack is on this model's
        device whenever a clip was preprocessed.  The cache has the same name and shapes under both piano configurations, as in
        the reference: one written under piano_keys=51 (landscape frames) is silently wrong under 88 (portrait), and the reverse."""
        if not piano:
            return None, None
        from .features import load_piano_frames
        write = video_paths is not None
        if video_paths is None:
            if video_frames is None:
                return None, None
            # names under which no cache can exist; nothing is written (write_cache=False)
            video_paths = [None if fr is None else f"<clip {i}>.mp4" for i, fr in enumerate(video_frames)]
        stack = load_piano_frames(video_paths, l, video_frames=video_frames, write_cache=write, video_multi=self.piano.video_multi,
                                  preprocess=None if video_frames is None else self.piano_frame_preprocessor())
        if stack is None:
            return None, None
        return stack, torch.zeros(stack.shape[0], int(l), self.cfg.notes)

    def _video2roll(self):
        if self._v2r is None:
            from .video2roll import Video2RollEngine
            self._v2r = Video2RollEngine(self._v2r_sd, self._device, compute=self._frames_compute, expand=self.piano.expand)
        return self._v2r

    def load_roll2midi(self, src, **kw):
        """The Roll2Midi generator behind `frames_to_midi`, run as in Roll2Midi_inference.py: the plain net of src/audeo/Roll2MidiNet.py
        or the attention-gated one of Roll2MidiNet_enhance.py (what Roll2Midi_train.py writes), told apart by the state dict's keys
        (`roll2midi.engine_for`).  src: a `Roll2MidiEngine` or `Roll2MidiEnhanceEngine`, a state dict in the layout of the reference's
        `checkpoint['state_dict_G']`, a checkpoint dict holding `state_dict_G`, or a path to a torch-saved one of either.  `kw` go to
        the engine's constructor (compute, chunk)."""
        from .roll2midi import Roll2MidiEngine, engine_for
        if isinstance(src, Roll2MidiEngine):                      # the enhanced engine is a subclass
            self._r2m = src
            return src
        if isinstance(src, (str, Path)):
            src = torch.load(str(src), map_location="cpu")
        if not isinstance(src, dict):
            raise TypeError(f"load_roll2midi: a Roll2MidiEngine, a state dict, a checkpoint dict or a path, got {type(src).__name__}")
        self._r2m = engine_for(src.get("state_dict_G", src), self._device, **kw)
        return self._r2m

    def frames_to_midi(self, frames, window: int = 100, threshold: float = 0.5, tail: str = "own"):
        """(b, 1, t, 100, 900) grey piano frames -> (probs (b, t, 51) fp32, midi (b, t, 51) uint8) at the video frame rate: the
        Video2Roll encoder's per-frame key probabilities refined by the Roll2Midi generator, `midi = probs >= threshold`
        (`Roll2MidiEngine.refine`).  Both networks run on the device with no host visit between them.  Under piano_keys=88
        the generator gets keys 15..65 of the encoder's 88, and the result stays (b, t, 51)."""
        if self._v2r_sd is None:
            raise NotImplementedError("frames_to_midi needs the Video2Roll encoder: load a checkpoint holding `video2roll_net.*` (load_state_dict)")
        if self._r2m is None:
            raise NotImplementedError("frames_to_midi needs the Roll2Midi generator: load_roll2midi(state_dict_G, a checkpoint holding it, or its path)")
        from .features import PIANO_51
        probs = self._video2roll().frame_probs(frames)
        if self.piano.notes != PIANO_51.notes:
            # an 88-key roll: the generator reads keys 15..65 of it (Roll2Midi_inference.py:25-38, Roll2Midi_dataset.py:13-14, 89-131)
            probs = probs[..., PIANO_51.note_min - self.piano.note_min:PIANO_51.note_max - self.piano.note_min + 1].contiguous()
        return self._r2m.refine(probs, window=window, threshold=threshold, tail=tail)

    @property
    def piano_spf(self) -> float:
        """Seconds per video frame of the piano configuration: video_multi latent frames of 320 samples at 24 kHz -- 0.04 (25 fps,
        the `spf` of Midi_synth.py:29) under piano_keys=51, 1 / 30 under 88."""
        return self.piano.video_multi * 320 / 24000

    def midi_to_notes(self, midi, lens=None):
        """The (b, t, 51) `midi` of `frames_to_midi` -> one (n_i, 3) int32 array of (pitch, start_frame, end_frame) per clip, keys
        15..65 = pitches 36..86: `process_midi` and `GetNote` of Midi_synth.py:66-118 in one launch (midi.roll_to_notes).  lens (b):
        the valid video frames of every clip."""
        from .features import PIANO_51
        from .midi import roll_to_notes
        if midi.ndim != 3 or midi.shape[2] != PIANO_51.notes:
            raise ValueError(f"midi_to_notes: the (b, t, {PIANO_51.notes}) output of frames_to_midi, got {tuple(midi.shape)}")
        return roll_to_notes(midi, lens, note_min=PIANO_51.note_min, device=self._device)

    def frames_to_notes(self, frames, source: str = "midi", lens=None, **kw):
        """(b, 1, t, 100, 900) grey piano frames -> the notes of every clip, rows (pitch, start_frame, end_frame); a frame lasts
        `piano_spf` seconds.  source="midi": `frames_to_midi(frames, **kw)` and `midi_to_notes`, the roll staying on the device in
        between (Midi_synth.py with `self.midi = True`).  source="roll": the file's shipped default (`self.midi = False`, :14), the
        Video2Roll encoder's own roll -- probability >= 0.4 (Video2Roll_inference.py:71-78) over the model's keys, 51 from key 15 or
        88 from key 0 -- and no Roll2Midi generator."""
        from .midi import ROLL_THRESHOLD_BELOW, roll_to_notes
        if source == "midi":
            return self.midi_to_notes(self.frames_to_midi(frames, **kw)[1], lens)
        if source != "roll":
            raise ValueError(f"frames_to_notes: source is 'midi' or 'roll', got {source!r}")
        if kw:
            raise TypeError(f"frames_to_notes(source='roll') takes no {sorted(kw)}: they are frames_to_midi's")
        if self._v2r_sd is None:
            raise NotImplementedError("frames_to_notes needs the Video2Roll encoder: load a checkpoint holding `video2roll_net.*` (load_state_dict)")
        probs = self._video2roll().frame_probs(frames)
        return roll_to_notes(probs, lens, threshold=ROLL_THRESHOLD_BELOW, note_min=self.piano.note_min)

    def piano_frame_preprocessor(self):
        """The `PianoFramePreprocessor` of this model's device (made on first use)."""
        if self._piano_pre is None:
            from .piano_frames import PianoFramePreprocessor
            self._piano_pre = PianoFramePreprocessor(self._device, layout=self.piano.layout)
        return self._piano_pre

    def load_text_encoder(self, src, tokenizer=None):
        """The FLAN-T5 prompt encoder behind `prompt=` (x3:1412-1413): a `T5Encoder`, a local HF directory
        (./ckpts/flan-t5-large) or a state dict (T5EncoderModel keys, or a reference checkpoint with `text_encoder2.*`).
        A `text_encoder_fn` given to the constructor still takes precedence."""
        from .t5 import T5Encoder
        if isinstance(src, T5Encoder):
            enc = src
            if tokenizer is not None:
                enc.tokenizer = tokenizer
        elif isinstance(src, (str, Path)):
            enc = T5Encoder.from_pretrained(str(src), self._device)
            if tokenizer is not None:
                enc.tokenizer = tokenizer
        elif isinstance(src, dict):
            enc = T5Encoder(src, self._device, tokenizer=tokenizer)
        else:
            raise TypeError(f"load_text_encoder: a T5Encoder, a directory or a state dict, got {type(src).__name__}")
        self._t5 = enc
        return enc

    def load_audio_encoder(self, src, **kw):
        """The Encodec encoder behind a raw-wave `cond` (b, nw) (x3:1350, 2157-2160; `EncodecWrapper.forward`, x3:428-432): an
        `EncodecEncoder` or an EncodecModel / encoder state dict.  Sets `mel_spec` to an adapter (b, nw) -> (b, 128, ceil(nw / 320));
        every row of the batch has the same nw, so the latent length is one number.  `kw` go to the EncodecEncoder constructor."""
        from .encodec import EncodecEncoder
        if isinstance(src, EncodecEncoder):
            enc = src
        elif isinstance(src, dict):
            enc = EncodecEncoder(src, self._device, **kw)
        else:
            raise TypeError(f"load_audio_encoder: an EncodecEncoder or a state dict, got {type(src).__name__}")
        self._audio_encoder = enc
        self.mel_spec = lambda wave: enc.encoder(wave.unsqueeze(1))
        return enc

    def load_mel_spec(self, src=None, **mel_spec_kwargs):
        """The log-mel front end behind a raw-wave `cond` / `inp` (b, nw) of a model whose latents are mel frames (x3:2157-2160,
        2328-2331): a `MelSpec`, or the reference's `MelSpec` keywords to build one on the model's device.  Sets `mel_spec`."""
        from .mel import MelSpec
        if src is None:
            src = MelSpec(device=self._device, **mel_spec_kwargs)
        elif not isinstance(src, MelSpec) or mel_spec_kwargs:
            raise TypeError(f"load_mel_spec: a MelSpec, or keywords alone to build one, got {type(src).__name__}")
        if src.n_mel_channels != self.num_channels:
            raise ValueError(f"load_mel_spec: n_mel_channels={src.n_mel_channels} but the model has num_channels={self.num_channels}")
        self.mel_spec = src
        return src

    def load_vocoder(self, src, **kw):
        """The Vocos vocoder behind `sample(return_raw_output=False)` of a model whose latents are mel frames (x3:2275-2287; the
        reference's `Vocos.from_pretrained(pretrained_vocos_path)`, e2_tts_crossatt.py:1324): a `Vocos`, its state dict, or a local
        directory with config.yaml and pytorch_model.bin.  Sets `self.vocos` and returns it.  `kw` go to the Vocos constructor.
        A `HiFiGAN` instance (the vocoder of the reference's `self.vocos = 'vae'`, x3:1404-1409) is taken as it is; a state dict or a
        directory always means Vocos.  So is a `VaeVocoder` (the whole of `VaeWrapper.decode`: the AudioLDM VAE decoder in front of the
        HiFiGAN), which reads the 128-channel latents of a 'vae' model."""
        from .audioldm_vae import VaeVocoder
        from .hifigan import HiFiGAN
        from .vocos import Vocos
        if isinstance(src, (Vocos, HiFiGAN, VaeVocoder)):
            if kw:
                raise TypeError(f"load_vocoder: keywords go with a state dict or a directory, not with a {type(src).__name__}")
            voc = src
        elif isinstance(src, dict):
            voc = Vocos(src, self._device, **kw)
        elif isinstance(src, (str, os.PathLike)):
            voc = Vocos.from_pretrained(src, device=self._device, **kw)
        else:
            raise TypeError(f"load_vocoder: a Vocos, a state dict or a local directory, got {type(src).__name__}")
        if voc.C != self.num_channels:
            raise ValueError(f"load_vocoder: the vocoder reads {voc.C} channels but the model has num_channels={self.num_channels}")
        hop = getattr(self.mel_spec, "hop", None)
        if self.sampling_rate is not None and hop is not None and int(hop) != voc.hop:
            raise ValueError(f"load_vocoder: the vocoder's hop is {voc.hop} but the loaded mel_spec has hop_length={int(hop)}: "
                             f"the wave would not run at sampling_rate={self.sampling_rate}")
        self.vocos = voc
        return voc

    def wave_front_end(self):
        """The `WaveFrontEnd` in front of the audio encoder: any rate -> the model's rate, `normalize_wav`; made on first use."""
        from .wave import WaveFrontEnd
        dev = self._audio_encoder.dev if self._audio_encoder is not None else torch.device(self._device)
        if self._wave_front_end is None or self._wave_front_end.dev != dev:
            self._wave_front_end = WaveFrontEnd(dev, new_freq=self.sampling_rate or 24000)
        return self._wave_front_end

    def encode_audio(self, waves, rates, max_frames=None, normalize=True):
        """Audio as it comes out of a file -> ground-truth / prompt latents, all on the device: what the reference's data path does on
        the CPU in front of the model (trainer_multigpus_alldatas3.py:1047-1050, 1129-1134, 1427-1432).  waves: a list of (n_i,) or
        (channels, n_i) waves, of which channel 0 is taken; rates: their sample rates (one int for all).  Each goes through the
        `WaveFrontEnd` (resampled to the model's rate, `normalize_wav` unless normalize=False, cut to max_frames * hop samples -- the
        validation set's `val_length`) straight into the `EncodecEncoder` of `load_audio_encoder`.
        -> (latents (b, n, C) fp32 on the device, zero behind each clip's frames; lens (b,) int64 on the host)."""
        if self._audio_encoder is None:
            raise RuntimeError("encode_audio needs the Encodec encoder: load_audio_encoder(state_dict)")
        enc = self._audio_encoder
        rates = [int(rates)] * len(waves) if isinstance(rates, (int, float)) else [int(r) for r in rates]
        if len(rates) != len(waves) or not waves:
            raise ValueError(f"encode_audio: {len(waves)} waves, {len(rates)} rates")
        fe = self.wave_front_end()
        cut = None if max_frames is None else int(max_frames) * enc.hop
        lat = enc.encode_list([fe(w, r, normalize=normalize, max_samples=cut) for w, r in zip(waves, rates)])      # (C, T_i) each
        lens = torch.tensor([z.shape[1] for z in lat], dtype=torch.long)
        out = torch.zeros(len(lat), int(lens.max()), lat[0].shape[0], dtype=torch.float32, device=enc.dev)
        for i, z in enumerate(lat):
            out[i, :z.shape[1]] = z.t()
        return out, lens

    def load_audio_quantizer(self, src):
        """The Encodec quantizer behind an integer `cond` of codes (b, n_q, n) -- the layout of `EncodecModel.encode`'s audio_codes[0] --
        and behind `latents_to_codes`: an `EncodecQuantizer`, or an EncodecModel / quantizer state dict."""
        from .encodec import EncodecQuantizer
        if isinstance(src, EncodecQuantizer):
            q = src
        elif isinstance(src, dict):
            q = EncodecQuantizer(src, self._device)
        else:
            raise TypeError(f"load_audio_quantizer: an EncodecQuantizer or a state dict, got {type(src).__name__}")
        if q.dim != self.num_channels:
            raise ValueError(f"load_audio_quantizer: codebooks of dimension {q.dim}, the model has {self.num_channels} latent channels")
        self._audio_quantizer = q
        return q

    def latents_to_codes(self, latents, bandwidth=None):
        """Sampler output (b, n, C) -> Encodec codes (b, n_q, n) int64 at `bandwidth` kbps (None: every codebook), the layout of
        `EncodecModel.encode`'s audio_codes[0], which `sample(cond=codes)` and any Encodec decoder take."""
        if self._audio_quantizer is None:
            raise NotImplementedError("latents_to_codes needs the Encodec quantizer: load_audio_quantizer(state_dict)")
        return self._audio_quantizer.encode(latents, bandwidth, channels_last=True).transpose(0, 1)

    def load_image_encoder(self, src, **kw):
        """The image encoder behind `video_frames=` and uncached `video_paths`.  video_encoder="clip_vit" (x3:1423-1425, 1714,
        1733-1735): a `CLIPImageEncoder`, a local HF directory (IP-Adapter sdxl_models/image_encoder) or a state dict
        (CLIPVisionModelWithProjection keys, or a reference checkpoint with `image_encoder.*`).  video_encoder="clip_vit2"
        (x3:1426-1428, 1714, 1736-1738): a `CLIPViT2ImageEncoder` or a local HF directory (openai clip-vit-large-patch14-336); its
        projection_dim must equal dim_text (768 for that model).  A bare state dict is refused under this choice: it names neither the
        activation nor the head width, so build the `CLIPViT2ImageEncoder` from it yourself and pass that.  video_encoder="dinov2"
        (x3:1432-1433, 1714, 1742-1744): a `DINOv2ImageEncoder`, a local HF directory (dinov2-giant) or a state dict (Dinov2Model keys,
        or `image_encoder.*`); its hidden_size must equal dim_text.  video_encoder="clip_convnext" (x3:1429-1431, 1716-1720,
        1739-1741): a `CLIPConvNeXtImageEncoder`, a local open_clip directory or a state dict (`visual.trunk.*` / `visual.head.*`,
        `image_encoder.*` or bare `trunk.*` / `head.*`); its embed_dim must equal dim_text.  video_encoder="mixed" (x3:1745-1788): a
        `MixedImageEncoder`, a directory with one subdirectory per choice, or a dict with one entry per choice (an encoder, a
        directory or a state dict each); the widths must add up to dim_text.  `kw` go to the encoder's constructor (compute, chunk,
        config)."""
        cls = IMAGE_ENCODERS.get(self.video_encoder)
        if cls is None:
            raise NotImplementedError(f"load_image_encoder: video_encoder={self.video_encoder!r} has no HIP encoder (built: {', '.join(IMAGE_ENCODERS)})")
        if isinstance(src, dict) and self.video_encoder in ("clip_convnext", "mixed"):
            if self.video_encoder == "mixed" and set(src) == set(MIXED_ORDER):
                src = MixedImageEncoder({k: self._part_encoder(k, src[k], kw) for k in MIXED_ORDER})
            elif not is_convnext_state_dict(src) or self.video_encoder == "mixed":
                raise NotImplementedError(f"load_image_encoder: video_encoder={self.video_encoder!r} " +
                                          ("takes a MixedImageEncoder, a directory or a dict with one entry per choice " + str(list(MIXED_ORDER))
                                           if self.video_encoder == "mixed" else "takes ConvNeXt weights (trunk.stem.0.weight ...)") +
                                          "; a state dict without trunk.stem.0.weight holds the weights of 'clip_vit', 'clip_vit2' or 'dinov2'")
        if isinstance(src, cls):
            enc = src
        elif isinstance(src, (str, Path)):
            enc = cls.from_pretrained(str(src), self._device, **kw)
        elif isinstance(src, dict):
            if self.video_encoder == "clip_vit2":
                raise NotImplementedError("load_image_encoder: video_encoder='clip_vit2' takes a CLIPViT2ImageEncoder or a directory with config.json, "
                                          "not a state dict (which names neither quick_gelu nor the head width)")
            enc = cls(src, self._device, **kw)
        else:
            raise TypeError(f"load_image_encoder: a {cls.__name__}, a directory or a state dict, got {type(src).__name__}")
        if self.video_encoder == "dinov2" and enc.d != self.dim_text:
            raise ValueError(f"load_image_encoder: the DINOv2 encoder's hidden_size {enc.d} is not the model's dim_text {self.dim_text}")
        if self.video_encoder == "clip_vit2" and enc.out_dim != self.dim_text:
            raise ValueError(f"load_image_encoder: the CLIP encoder's projection_dim {enc.out_dim} is not the model's dim_text {self.dim_text}")
        if self.video_encoder == "clip_convnext" and enc.out_dim != self.dim_text:
            raise ValueError(f"load_image_encoder: the ConvNeXt encoder's embed_dim {enc.out_dim} is not the model's dim_text {self.dim_text}")
        if self.video_encoder == "mixed" and enc.out_dim != self.dim_text:
            raise ValueError(f"load_image_encoder: the mixed encoders' widths add up to {enc.out_dim}, not the model's dim_text {self.dim_text}")
        self._clip = enc
        return enc

    def _part_encoder(self, choice: str, src, kw: dict):
        """One part of a mixed encoder: an encoder as it is, a directory through from_pretrained, a state dict through the class."""
        cls = IMAGE_ENCODERS[choice]
        if isinstance(src, (str, Path)):
            return cls.from_pretrained(str(src), self._device, **kw)
        if isinstance(src, dict):
            return cls(src, self._device, **kw)
        return src

    def _encode_video_frames(self, clips, paths=None) -> list:
        """[(frames uint8 (F, H, W, 3), duration) or None] -> [(image_embeds (F, dim) float32 on the CPU, duration) or None]; the
        frames of all clips of one frame size go through the encoder in one batched pass.  Under "mixed" with `paths` (the videos
        the clips belong to) each clip goes through `encode_mixed_cached`: its parts' own caches are read and written (x3:1745-1788)."""
        out = [None] * len(clips)
        if paths is not None and isinstance(self._clip, MixedImageEncoder):
            from .features import encode_mixed_cached
            for i, c in enumerate(clips):
                if c is not None:
                    out[i] = (encode_mixed_cached(paths[i], c[0], float(c[1]), self._clip), float(c[1]))
            return out
        groups: dict[tuple, list[int]] = {}
        arrs = {}
        for i, c in enumerate(clips):
            if c is None:
                continue
            fr = c[0] if torch.is_tensor(c[0]) else torch.from_numpy(np.ascontiguousarray(c[0]))
            arrs[i] = fr
            groups.setdefault(tuple(fr.shape[1:]), []).append(i)
        for idx in groups.values():
            emb = self._clip(torch.cat([arrs[i] for i in idx], 0)).cpu()
            o = 0
            for i in idx:
                n = arrs[i].shape[0]
                out[i] = (emb[o:o + n], float(clips[i][1]))
                o += n
        return out

    def _get_context(self, prompt, context, context_mask, b, video_drop_prompt=None):
        if context is None:
            if prompt is None:
                raise ValueError("pass `prompt` (with text_encoder_fn) or precomputed `context`/`context_mask`")
            if self.text_encoder_fn is not None:
                context, context_mask = self.text_encoder_fn(list(prompt))     # encode_text x3:1648-1657
            elif getattr(self, "_t5", None) is not None:
                prompts = list(prompt)
                if video_drop_prompt is not None:              # x3:2053-2057 (the reference rewrites the caller's list in place)
                    prompts = ["the sound of X X" if video_drop_prompt[i] else p for i, p in enumerate(prompts)]
                context, context_mask = self._t5(prompts)      # encode_text x3:1648-1657, once per call
            else:
                raise NotImplementedError("FLAN-T5 encoding is outside the accelerated path (SURVEY 8): supply "
                                          "`context`/`context_mask` or construct with text_encoder_fn=")
        if context_mask is None:
            context_mask = torch.ones(context.shape[:2], dtype=torch.bool)
        assert context.shape[0] == b
        return context, context_mask

    def _clip_conditioning(self, text, video_paths, video_frames, batch: int, n: int):
        """The (b, n, dim_text) CLIP conditioning of `sample` and `forward` (x3:2183-2184, 2335-2336) when no text_embed= was given."""
        cfgm = self.cfg
        if video_paths is not None and self.video_encoder_fn is not None:
            return self.video_encoder_fn(video_paths, n)
        if video_paths is not None:
            # cached CLIP features next to the videos, resampled to the latent rate (encode_video's cache branch,
            # x3:1796-1813); with video_frames and the image encoder, missing caches are encoded first (x3:1706-1793)
            from .features import encode_video_cached, feature_cache_path
            encoder_fn = None
            if video_frames is not None:
                if self._clip is None:
                    raise RuntimeError("video_frames needs the CLIP image encoder: call load_image_encoder first")
                if len(video_frames) != len(video_paths):
                    raise ValueError(f"video_frames: {len(video_frames)} entries for {len(video_paths)} video_paths")
                plain = [vp[0] if isinstance(vp, tuple) else vp for vp in video_paths]
                todo = [fr if vp is not None and fr is not None and not os.path.exists(feature_cache_path(vp, self.video_encoder)) else None
                        for vp, fr in zip(plain, video_frames)]
                done = {vp: e for vp, e in zip(plain, self._encode_video_frames(todo, plain)) if e is not None}
                def encoder_fn(vp):
                    if vp not in done:
                        raise FileNotFoundError(f"{feature_cache_path(vp, self.video_encoder)}: no cached CLIP features and no frames for {vp}")
                    return done[vp]
            return encode_video_cached(video_paths, n, dim=cfgm.dim_text, video_encoder=self.video_encoder,
                                       sampling_rate=self.sampling_rate or 24000, frame_size=self.frame_size, encoder_fn=encoder_fn)
        if video_frames is not None:
            if self._clip is None:
                raise RuntimeError("video_frames needs the CLIP image encoder: call load_image_encoder first")
            if len(video_frames) != batch:
                raise ValueError(f"video_frames: {len(video_frames)} entries for a batch of {batch}")
            from .features import resample_clip_features
            rows = []
            for e in self._encode_video_frames(list(video_frames)):
                rows.append(torch.zeros(n, cfgm.dim_text) if e is None else
                            resample_clip_features(e[0], e[1], n, sampling_rate=self.sampling_rate or 24000,
                                                   frame_size=self.frame_size))
            return torch.stack(rows, 0)
        if torch.is_tensor(text) and text.ndim == 3:
            return text
        raise NotImplementedError("pass video_paths (with cached .npz CLIP features), text_embed= (b, n, dim_text) "
                                  "or video_encoder_fn=")

    # ---- reference API: one forward ----------------------------------------------------------
    @torch.no_grad()
    def transformer_with_pred_head(self, x, cond=None, times=None, mask=None, text=None, frames_embed=None,
                                   prompt=None, video_drop_prompt=None, audio_drop_prompt=None,
                                   drop_audio_cond: bool | None = None, drop_text_cond: bool | None = None,
                                   drop_text_prompt: bool | None = None, return_drop_conditions=False,
                                   *, context=None, context_mask=None):
        """x3:1993-2088.  x (b,n,C); times (b,) or 0-dim; mask (b,n) bool prefix mask or None;
        text (b,n,dim_text) float; frames_embed (b,n,NOTES).  Returns (b,n,C) on x.device."""
        if cond is not None and not self.cfg.cond_proj_in:
            raise NotImplementedError("cond != None needs cond_proj_in (E2TTS(if_cond_proj_in=True), x3:1365): with the shipped "
                                      "configuration (predict.py:144) the reference has no such layer either (x3:2034)")
        if self.training:
            raise NotImplementedError("training-time random condition dropping is out of scope")
        b, n, _ = x.shape
        dtc, dtp = bool(drop_text_cond), bool(drop_text_prompt)
        eng = self.engine()
        context, context_mask = self._get_context(prompt, context, context_mask, b, video_drop_prompt)
        times = torch.as_tensor(times, dtype=torch.float32)
        if times.ndim == 0:
            times = times.repeat(b)
        eng.setup(b, n, context.shape[1], b, cfg_mode=False)
        p = eng.plan
        p["per_sample_t"] = True
        lens = None if mask is None else _mask_to_lens(mask)
        if frames_embed is None:
            frames_embed = torch.zeros(b, n, self.cfg.notes)
        drop_ctx = [dtp or bool(video_drop_prompt is not None and video_drop_prompt[i]) for i in range(b)]
        step_cond = None
        if cond is not None:                                  # x3:2015-2020: dropped prompts are zeroed (in place in the reference)
            step_cond = cond.detach().to(torch.float32).clone()
            for i in range(b):
                if bool(drop_audio_cond) or (audio_drop_prompt is not None and audio_drop_prompt[i]):
                    step_cond[i] = 0
        eng.prepare(text, frames_embed, context, context_mask, times, lens=lens,
                    drop_text=[dtc] * b, drop_ctx=drop_ctx, step_cond=step_cond)
        eng.embed(x.to(self._device, torch.float32).contiguous())
        pred = eng.forward(n_ctx_seqs=b)
        out = pred[:, self.cfg.num_registers:, :].to(x.device).clone()
        p["per_sample_t"] = False
        if return_drop_conditions:
            return out, [bool(drop_audio_cond)] * b, dtc, [dtp] * b
        return out

    @torch.no_grad()
    def cfg_transformer_with_pred_head(self, *args, cfg_strength: float = 1.0, remove_parallel_component: bool = True,
                                       keep_parallel_frac: float = 0.0, **kwargs):
        """x3:2090-2113 (two forwards; sample() uses the batched in-engine form instead)."""
        pred = self.transformer_with_pred_head(*args, drop_audio_cond=False, drop_text_cond=False, drop_text_prompt=False, **kwargs)
        if cfg_strength < 1e-5:
            return pred
        null = self.transformer_with_pred_head(*args, drop_audio_cond=True, drop_text_cond=True, drop_text_prompt=True, **kwargs)
        upd = pred - null
        if remove_parallel_component:
            shp = upd.shape
            xd, yd = upd.reshape(shp[0], -1).double(), pred.reshape(shp[0], -1).double()
            unit = torch.nn.functional.normalize(yd, dim=-1)
            par = (xd * unit).sum(-1, keepdim=True) * unit
            upd = ((xd - par) + par * keep_parallel_frac).reshape(shp).to(pred.dtype)
        return pred + upd * cfg_strength

    # ---- reference API: the validation pass ------------------------------------------------------
    @torch.no_grad()
    def forward(self, inp, *, text=None, times=None, lens=None, velocity_consistency_model=None, velocity_consistency_delta=1e-3,
                prompt=None, video_drop_prompt=None, audio_drop_prompt=None, val=False, video_paths=None, frames=None, midis=None,
                # build-side extensions
                x0=None, text_embed=None, context=None, context_mask=None, frames_embed=None, video_frames=None):
        """x3:2307-2588, the `val=True` branch -- what the trainer's evaluate() calls: a fixed span (`val_span_mask`), fixed noise, one
        evaluation of the DiT with nothing dropped, the flow-matching loss on the span and, with `frames`, the roll loss and the
        precision / recall / f1 / accuracy of the Video2Roll encoder against `midis`.  Returns the reference's
        `E2TTSReturn(loss, cond, pred_flow, pred_data, LossBreakdown(precision, recall, f1, acc))` on inp's device, loss = flow loss +
        10 * roll loss; `val_stats` keeps the parts (flow, roll, tp, fp, fn, tn) of the last call.  Training (`val=False`) is out of scope.
        `inp` (b, n, C) latents or a raw wave (b, nw) through `mel_spec`; `times` a scalar, (b,) or None (= torch.rand(b));
        `frames` (bf, 1, t, 100, 900) with `midis` (bf, n, NOTES) cover the last bf <= b clips.
        `x0`: the noise (b, n, C); without it, randn of a generator seeded 0 on the model's device -- the reference seeds the global
        RNG with 0 and re-seeds it from the clock (x3:2373-2377), this leaves the global RNG alone.
        `text_embed`, `context`, `context_mask`, `video_frames`: as in `sample`; `frames_embed` (bf, n, NOTES): the roll in place of
        `encode_frames(frames, n)`."""
        if not val:
            raise NotImplementedError("forward(val=False) is the training step (random spans, random condition dropping, gradients): "
                                      "out of scope, only the validation pass val=True is built")
        if velocity_consistency_model is not None:
            raise NotImplementedError("velocity_consistency_model: the velocity consistency loss is a training term (x3:2508-2536)")
        has_cond = not self.audiocond_drop_prob > 1.0                                  # x3:2400-2407
        if has_cond and self.audiocond_snr is not None:
            raise NotImplementedError("audiocond_snr: the reference adds fresh device noise to the audio condition (x3:2115-2125, 2406)")
        self.eval()
        if inp.ndim == 2:                                                              # raw wave (x3:2328-2331)
            if self.mel_spec is None:
                raise NotImplementedError("a raw-wave `inp` needs mel_spec_module, which the shipped config does not set "
                                          "(load_audio_encoder sets the Encodec encoder)")
            inp = self.mel_spec(inp).permute(0, 2, 1)                                  # b d n -> b n d
            assert inp.shape[-1] == self.num_channels, (tuple(inp.shape), self.num_channels)
        b, n = inp.shape[:2]
        out_device, dev, C_ = inp.device, self._device, self.num_channels
        if text_embed is None:
            text_embed = self._clip_conditioning(text, video_paths, video_frames, b, n)    # x3:2335-2336
        lens = torch.full((b,), n, dtype=torch.long) if lens is None else torch.as_tensor(lens).cpu().long()
        mask = lens_to_mask(lens, n)                                                   # x3:2348
        span = val_span_mask(lens, n)                                                  # x3:2358-2362
        mask_u8, span_u8 = mask.to(dev, torch.uint8).contiguous(), span.to(dev, torch.uint8).contiguous()
        x1 = inp.detach().to(dev, torch.float32).contiguous()
        if x0 is None:
            x0 = torch.randn(b, n, C_, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
        x0 = x0.to(dev, torch.float32).contiguous()
        assert x0.shape == x1.shape == (b, n, C_), (tuple(x0.shape), tuple(x1.shape))
        if times is None:
            times = torch.rand(b)                                                      # x3:2382
        times = torch.as_tensor(times, dtype=torch.float32).cpu()
        times = times.repeat(b) if times.ndim == 0 else times                          # x3:2384
        assert times.shape == (b,), tuple(times.shape)
        w, flow = torch.empty_like(x1), torch.empty_like(x1)
        cond = torch.empty_like(x1) if has_cond else None
        L.cfm_interp(x0, x1, times.to(dev), span_u8 if has_cond else None, w, flow, cond)      # x3:2394-2407
        # -- roll loss and metrics of the frame encoder (x3:2418-2448); no frames: roll and midis are zero, and so are all five
        stats = torch.zeros(8, dtype=torch.float64, device=dev)                        # flow: sum, count; roll: sum, count, tp, fp, fn, tn
        roll = torch.zeros(b, n, self.cfg.notes, device=dev)
        if frames is not None or frames_embed is not None:
            if midis is None:
                raise ValueError("forward: `frames` needs `midis` (bf, n, NOTES), the MIDI ground truth of the same clips")
            if frames_embed is None:
                frames_embed = (self.frames_encoder_fn or self.encode_frames)(frames, n)       # x3:2423
            fe = frames_embed.to(dev, torch.float32).contiguous()
            md = midis.to(dev, torch.float32).contiguous()
            bf = fe.shape[0]
            if not (0 < bf <= b and fe.shape == md.shape == (bf, n, self.cfg.notes)):
                raise ValueError(f"forward: roll {tuple(fe.shape)} and midis {tuple(md.shape)}, expected (bf <= {b}, {n}, {self.cfg.notes})")
            L.roll_metrics(fe, md, mask_u8[b - bf:], stats[2:])                        # x3:2429-2443
            roll[b - bf:] = fe                                                         # x3:2469-2470: zero clips in front
        pred = self.transformer_with_pred_head(w, cond, times=times, mask=mask, text=text_embed, frames_embed=roll, prompt=prompt,
                                               video_drop_prompt=video_drop_prompt, audio_drop_prompt=audio_drop_prompt,
                                               drop_audio_cond=False, drop_text_cond=False, drop_text_prompt=False,
                                               context=context, context_mask=context_mask)                  # x3:2488-2502
        L.masked_sqerr(pred, flow, span_u8, stats[:2])                                 # x3:2542-2547
        st = stats.cpu()                                                               # the one transfer of the scalars
        flow_loss = st[0] / st[1]                                                      # an empty span: 0 / 0 = nan, as torch's mean of nothing
        roll_loss = st[2] / st[3] if frames_embed is not None else st[2]               # no frames: 0 (x3:2419-2420)
        tp, fp, fn, tn = (float(v) for v in st[4:])
        ratio = lambda num, den: num / den if den != 0 else 0.0                        # x3:2445-2448
        pre, rec, f1, acc = ratio(tp, tp + fp), ratio(tp, tp + fn), ratio(2 * tp, 2 * tp + fp + fn), ratio(tp, tp + fp + fn)
        self.val_stats = dict(flow=float(flow_loss), roll=float(roll_loss), tp=tp, fp=fp, fn=fn, tn=tn)
        f32 = lambda v: torch.as_tensor(v, dtype=torch.float64).to(torch.float32).to(out_device)
        total = f32(flow_loss + 10.0 * roll_loss)                                      # x3:2574-2577
        return E2TTSReturn(total, (cond if has_cond else w).to(out_device), pred.to(out_device), (x0 + pred).to(out_device),
                           LossBreakdown(f32(pre), f32(rec), f32(f1), f32(acc)))        # x3:2579, 2588

    __call__ = forward

    # ---- reference API: the sampler ------------------------------------------------------------
    @torch.no_grad()
    def sample(self, cond, *, text=None, lens=None, duration=None, steps=32, cfg_strength=1.0,
               remove_parallel_component=True, sway_sampling=True, max_duration=4096, vocoder=None,
               return_raw_output=None, save_to_filename=None, prompt=None, video_drop_prompt=None,
               audio_drop_prompt=None, video_paths=None, frames=None, midis=None,
               # build-side extensions
               y0=None, text_embed=None, context=None, context_mask=None, frames_embed=None, trajectory_out=None, video_frames=None,
               piano=False):
        """x3:2127-2305.  With lens == duration (every shipped call, predict.py:261-263) `cond` (b, n, C) only fixes shape and
        device.  With lens[0] != duration[0] it is the audio prompt of the infilling branch (x3:2196-2231, 2260-2261; needs
        if_cond_proj_in=True): zero-padded to the longest duration, masked to lens, added through cond_proj_in at every
        evaluation (dropped in the null pass), and returned unchanged in the first lens[b] frames.
        An integer `cond` (b, n_q, n) is that prompt as Encodec codes (`EncodecModel.encode`'s audio_codes[0]): the quantizer of
        load_audio_quantizer decodes it to (b, n, C) first.
        `trajectory_out`: optional list that receives a device copy of y at every grid point (the `trajectory` of
        x3:2255, of which the reference keeps only [-1]); test aid, adds a copy per step.
        `video_frames`: one (frames uint8 (F, H, W, 3), duration_s) per clip (or None), encoded by the CLIP image encoder
        (load_image_encoder): with `video_paths` only the clips without a feature cache are encoded -- in one batched pass -- and
        their caches written (x3:1706-1793; an existing cache wins); without `video_paths` the embeddings are resampled to the
        latent rate and nothing is written.
        `piano`: with `frames` None and `video_frames` given, the same list also feeds the V2P frame encoder: `encode_video_frames`
        builds the grey (b, 1, t, 100, 900) stack on the GPU (frame caches next to `video_paths` honoured and written; without
        `video_paths` nothing is written) and hands it to `encode_frames` without leaving the device."""
        self.eval()
        if cond.ndim == 3 and not (cond.is_floating_point() or cond.is_complex()):  # Encodec codes (b, n_q, n): the prompt, quantized
            if self._audio_quantizer is None:
                raise NotImplementedError("an integer `cond` is a prompt of Encodec codes (b, n_q, n) and needs the quantizer: "
                                          "load_audio_quantizer(state_dict)")
            cond = self._audio_quantizer.decode(cond.transpose(0, 1), channels_last=True).to(cond.device)      # (b, n, C)
        if cond.ndim == 2:                                                          # raw wave (x3:2157-2160)
            if self.mel_spec is None:
                raise NotImplementedError("raw-wave `cond` needs mel_spec_module, which the shipped config does not set "
                                          "(load_audio_encoder sets the Encodec encoder)")
            cond = self.mel_spec(cond).permute(0, 2, 1)                              # b d n -> b n d
            assert cond.shape[-1] == self.num_channels, (tuple(cond.shape), self.num_channels)
        batch, cond_seq_len = cond.shape[:2]
        out_device = cond.device
        cfgm = self.cfg
        # -- frames / piano roll (x3:2164-2176)
        if frames_embed is None and frames is None and piano and video_frames is not None:
            if len(video_frames) != batch:
                raise ValueError(f"video_frames: {len(video_frames)} entries for a batch of {batch}")
            frames, _ = self.encode_video_frames(video_paths, cond_seq_len, True, video_frames=video_frames)      # predict.py:231
        if frames_embed is None:
            if frames is None or isinstance(frames, (int, float)):
                # no frames (V2A): all-zero roll (x3:2164-2165).  predict.py:270 also lets a float placeholder through, which the
                # reference's encode_frames would fail on (`x.shape`, x3:1527); here it means "no frames" instead of reaching the encoder
                frames_embed = torch.zeros(batch, cond_seq_len, cfgm.notes)
            elif self.frames_encoder_fn is not None:
                frames_embed = self.frames_encoder_fn(frames, cond_seq_len)
            elif self._v2r_sd is not None:
                frames_embed = self.encode_frames(frames, cond_seq_len)     # x3:2169
            else:
                raise NotImplementedError("`frames` needs the Video2Roll encoder: load a checkpoint holding `video2roll_net.*`, "
                                          "or pass frames_embed= / frames_encoder_fn=")
        if lens is None:
            lens = torch.full((batch,), cond_seq_len, dtype=torch.long)
        lens = torch.as_tensor(lens).cpu().long()
        # -- CLIP conditioning (x3:2183-2184)
        if text_embed is None:
            text_embed = self._clip_conditioning(text, video_paths, video_frames, batch, cond_seq_len)
        # -- duration (x3:2196-2216)
        if duration is None:
            duration = lens.clone()
        elif isinstance(duration, int):
            duration = torch.full((batch,), duration, dtype=torch.long)
        duration = torch.maximum(lens, torch.as_tensor(duration).cpu().long()).clamp(max=max_duration)
        assert duration.shape[0] == batch
        n = int(duration.amax())
        if frames_embed.shape[1] < n:
            pad = torch.zeros(batch, n - frames_embed.shape[1], cfgm.notes, dtype=frames_embed.dtype, device=frames_embed.device)
            frames_embed = torch.cat([frames_embed, pad], 1)
        frames_embed = frames_embed[:, :n]
        if text_embed.shape[1] != n:
            raise ValueError(f"text_embed has {text_embed.shape[1]} frames, the longest duration is {n}")
        # -- audio prompt (x3:2196-2231): the reference decides on clip 0 for the whole batch (x3:2224)
        step_cond = cond_mask = condp = None
        if int(lens[0]) != int(duration[0]):
            if not cfgm.cond_proj_in:
                raise NotImplementedError("lens != duration (audio-prompted infilling) needs cond_proj_in (E2TTS(if_cond_proj_in=True), "
                                          "x3:1365): with the shipped configuration the reference fails at x3:2034 as well")
            if self.audiocond_snr is not None:
                # (the reference cannot get through this branch either: add_noise indexes signal[mask] with the (b, n, 1) cond_mask of
                # x3:2213 on the (b, n, C) prompt, which torch refuses -- IndexError at x3:2124 -- so there is no behaviour to mirror)
                raise NotImplementedError("audiocond_snr: the reference adds fresh device noise to the prompt at every step (x3:2115-2125, 2228)")
            condp = torch.nn.functional.pad(cond.detach().to("cpu", torch.float32)[:, :n], (0, 0, 0, max(0, n - cond_seq_len)))   # x3:2212
            cond_mask = lens_to_mask(lens, n)[..., None]                                                            # x3:2196, 2213-2214
            step_cond = torch.where(cond_mask, condp, torch.zeros_like(condp))                                      # x3:2228
            for i in range(batch):                                                                                  # x3:2018-2020
                if audio_drop_prompt is not None and audio_drop_prompt[i]:
                    step_cond[i] = 0
        elif n != cond_seq_len:
            raise ValueError(f"cond has {cond_seq_len} frames but the longest duration is {n}")
        context, context_mask = self._get_context(prompt, context, context_mask, batch, video_drop_prompt)
        drop_ctx = [bool(video_drop_prompt is not None and video_drop_prompt[i]) for i in range(batch)]
        # -- grid (x3:2250-2252) and noise (x3:2248)
        t = sway_grid(steps, sway_sampling)
        S = steps - 1
        if y0 is None:
            y0 = torch.randn(batch, n, cfgm.num_channels, device=self._device)
        # -- shape buckets (constructor): pad frames / context, the masks hide the padding; RoPE positions of the cross-attention
        #    keys stay those of the unpadded call (DiTEngine.prepare)
        nc = context.shape[1]
        n_plan = -(-n // self.bucket_frames) * self.bucket_frames if self.bucket_frames > 0 else n
        if n_plan > cfgm.max_seq_len:       # the bucket would run past the position table: exact shape for this call
            n_plan = n
        nc_plan = -(-nc // self.bucket_ctx) * self.bucket_ctx if self.bucket_ctx > 0 else nc
        pad_t = lambda x: x if x is None or x.shape[1] == n_plan else torch.nn.functional.pad(x, (0, 0, 0, n_plan - x.shape[1]))
        if nc_plan != nc:
            context = torch.nn.functional.pad(context, (0, 0, 0, nc_plan - nc))
            context_mask = torch.nn.functional.pad(context_mask.to(torch.bool), (0, nc_plan - nc))
        eng = self.engine()
        eng.setup(batch, n_plan, nc_plan, S, cfg_mode=True)
        p = eng.plan
        if "y" not in p:
            p["y"] = torch.empty(batch, n_plan, cfgm.num_channels, dtype=torch.float32, device=self._device)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        eng.prepare(pad_t(text_embed), pad_t(frames_embed), context, context_mask, t[:-1], lens=duration,
                    drop_ctx=drop_ctx, dt=t[1:] - t[:-1], step_cond=pad_t(step_cond),
                    rope_len=cfgm.num_registers + n, rope_ctx_len=nc, fold_embed=True)
        ev[1].record()
        self._run_steps(eng, pad_t(y0), S, float(cfg_strength), bool(remove_parallel_component), trajectory_out, n)
        ev[2].record()
        self._phase_events = ev          # device-side phase marks of this call (no host sync here): see phase_ms()
        out = p["y"][:, :n].to(out_device).clone()
        if step_cond is not None:
            out = torch.where(cond_mask.to(out_device), condp.to(out_device), out)        # x3:2260-2261: the prompt frames come back unchanged
        if return_raw_output:
            return out
        # -- waveform decode (x3:2270-2305), only if the caller attached a vocoder module
        mask = lens_to_mask(duration)
        if vocoder is not None:
            return vocoder(out.transpose(1, 2))
        if self.vocos is None:
            return out
        audio = [self.vocos.decode(mel[m].transpose(0, 1)[None]).squeeze(0) for mel, m in zip(out, mask)]
        if save_to_filename is not None:
            import torchaudio  # optional dependency of the caller's environment
            path = Path(save_to_filename)
            path.parents[0].mkdir(exist_ok=True, parents=True)
            for ind, one in enumerate(audio):
                name = path.name if len(audio) == 1 else f"{ind + 1}.{path.name}"
                torchaudio.save(str(path.parents[0] / name), one.detach().cpu()[None], sample_rate=self.sampling_rate)
        return audio

    def phase_ms(self):
        """(prepare_ms, euler_loop_ms) of the last sample() call, from events on the launch stream; synchronises."""
        ev = getattr(self, "_phase_events", None)
        if ev is None:
            return None
        ev[2].synchronize()
        return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])

    def _run_steps(self, eng: DiTEngine, y0, S, cfg_strength, apg, traj=None, n_valid=None):
        """steps-1 Euler evaluations (A12 of SURVEY 8c).  cfg_strength < 1e-5 (x3:2101) still
        runs the batched pass; the null half then has weight 0."""
        p = eng.plan
        y = eng.begin_steps(y0)        # y0 into plan["y"]; arms the folded embed where prepare() left its tables (DiTEngine.fold_embed)
        p["step"].zero_()
        if traj is not None:
            traj.append(y[:, :n_valid].clone())
        if not self._use_graph:
            for _ in range(S):
                eng.euler_step(y, cfg_strength, apg)
                if traj is not None:
                    traj.append(y[:, :n_valid].clone())
            return
        # graphs live in the plan they were captured on (DiTEngine keeps the last few plans, least recently used first); the key
        # holds everything that changes the captured launch sequence: embed() and forward() issue different launches with an
        # audio prompt (has_cond), ragged lengths, or any tuning knob of the engine
        key = (cfg_strength, apg, eng.launch_signature())
        g = p["graphs"].get(key)
        if g is None:
            # warm-up on the real buffers (first-launch attribute calls must not happen under capture)
            keep = y.clone()
            eng.euler_step(y, cfg_strength, apg)
            torch.cuda.synchronize()
            eng.begin_steps(keep)       # restores y and, on an armed plan, its operand planes
            p["step"].zero_()
            g = torch.cuda.CUDAGraph()
            # thread-local capture mode: only this thread's calls are policed, so a communication library's watchdog thread
            # (RCCL under torch.distributed) polling its events meanwhile cannot invalidate the capture
            with torch.cuda.graph(g, stream=process_streams(self._device)[2], capture_error_mode="thread_local"):
                eng.euler_step(y, cfg_strength, apg)
            p["graphs"][key] = g
            self.graph_captures += 1
        for _ in range(S):
            g.replay()
            if traj is not None:
                traj.append(y[:, :n_valid].clone())


def _mask_to_lens(mask: torch.Tensor) -> torch.Tensor:
    mask = mask.to(torch.bool).cpu()
    lens = mask.sum(-1)
    if not bool((mask == lens_to_mask(lens, mask.shape[1])).all()):
        raise NotImplementedError("only prefix masks (lens_to_mask form, x3:296-305) are supported")
    return lens
