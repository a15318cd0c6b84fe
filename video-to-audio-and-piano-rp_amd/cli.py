"""Batched V2A inference CLI.

Same positional arguments as the reference's `src/inference_v2a.py:3-11`
    ckpt  drop_prompt(0|1)  test_scp  start  end  out_dir
(`test_scp`: one `video_path<TAB>caption` per line, tests/vgg_test.scp) plus batching: clips [start, end)
are collated `--batch` at a time (the reference samples one clip per call, src/inference_v2a.py:157,183) and,
under torchrun, sharded contiguously over the ranks with ONE all-gather of the latents per batch.

What it needs next to each video: the cached CLIP features `<video>.generated.npz` (features.py) and a cached
FLAN-T5 context `<video>.t5.npz` (arr_0 = (nc, 1024) hidden states) unless `--t5 ./ckpts/flan-t5-large` points at
local T5 weights.  Output: `<out_dir>/<name>.latent.npy`, the (n, 128) Encodec latent that the reference feeds to
`vocos.decode` (src/inference_v2a.py / predict.py:277-278).

  --clip DIR         encode the videos that have no CLIP feature cache (moviepy decode, HIP CLIP encoder of this rank's GPU)
  --video-encoder {clip_vit,clip_vit2,clip_convnext,dinov2,mixed}   which frame encoder the checkpoint was trained on: selects the class --clip DIR loads (the
                     HIP CLIP ViT-bigG, CLIP ViT-L/14-336 or DINOv2 encoder) and the cache name (`<video>.generated.npz` /
                     `<video>.generated.clip_vit2.npz` / `<video>.generated.dinov2.npz`); clip_vit2 is accepted only with --clip DIR
  --t5-engine hip    run --t5 on the HIP FLAN-T5 encoder (t5.py) of this rank's GPU instead of transformers on the CPU
  --piano            V2P (src/inference_v2p.py): the grey frames `<video>.generated_frames_raw.2.npz` (features.py; made on the GPU
                     by piano_frames.py from a moviepy decode when the cache is missing) go
                     through the HIP Video2Roll encoder; the checkpoint must hold `video2roll_net.*`
  --piano-keys {51,88}   the piano configuration of the checkpoint (features.PianoConfig): 51 = e2_tts_crossatt3.py, 88 =
                     e2_tts_crossatt3_2.py (trainer_multigpus_alldatas3_2.py): 88 keys, a video frame per 2.5 latent frames, portrait
                     frames.  The frame cache has one name and one shape under both: a cache of the other configuration is silently wrong
  --encodec STATE    torch-saved state dict of `EncodecModel.from_pretrained("facebook/encodec_24khz")` (or of its decoder):
                     each clip's valid frames are decoded by the HIP vocoder and written as `<name>.wav` (24 kHz float32),
                     what the reference does with `save_to_filename` / torchaudio.save (x3:2291-2303, predict.py:279-281).
  --vocos DIR        the vocoder of a checkpoint whose latents are log-mel frames: a local directory with `config.yaml` and
                     `pytorch_model.bin` as the hub stores `charactr/vocos-mel-24khz` (the reference's `Vocos.from_pretrained`,
                     e2_tts_crossatt.py:1324; nothing is fetched).  Each clip's valid frames are decoded by the HIP Vocos (vocos.py) and
                     written as `<name>.wav`; a clip has 24000 / hop frames per second, hop from the vocoder's config (256), not 320.
                     As the vocoder it is exclusive with --encodec.
  --audioldm CKPT    the vocoder of a checkpoint whose latents are the AudioLDM VAE's (the reference's `self.vocos = 'vae'`, x3:1404-1409):
                     a local torch checkpoint file, the state dict itself or a dict that holds it under `state_dict`
                     (`first_stage_model.decoder.*`, `first_stage_model.post_quant_conv.*`, `first_stage_model.vocoder.*`, `scale_factor`).
                     Each clip's valid frames go through the HIP VAE decoder and HiFi-GAN (audioldm_vae.py, hifigan.py) and are written as
                     `<name>.wav` at 16 kHz; a clip has 16000 / 640 = 25 frames per second.  Exclusive with --vocos and --encodec.
  --audio-prompt-seconds S   (with --encodec, checkpoint built with if_cond_proj_in) the first S seconds of `<video>.wav` (24 kHz) are
                     encoded by the HIP Encodec encoder and given to the sampler as the audio prompt: `cond` = the raw waves,
                     `lens` = ceil(24000 S / 320) frames, which come back unchanged in front of the generated ones (x3:2196-2231).
  --codes KBPS       (with --encodec, whose state dict holds the quantizer) also write `<name>.codes.npy`: int16 (n_q, n) Encodec codes
                     of the clip's valid frames at 1.5 / 3 / 6 / 12 / 24 kbps (2 / 4 / 8 / 16 / 32 codebooks of 10 bits at 75 Hz), what
                     `EncodecModel.encode(...).audio_codes[0][0]` holds and any Encodec decoder reads.  The `.wav` is still decoded from
                     the continuous latents.
  --validate         no sampling: the reference's validation pass, `E2TTS.forward(val=True)` at times = 0.5 as the trainer's evaluate() calls
                     it (trainer_multigpus_alldatas3.py:271-290), on the ground-truth latents `<video>.latent.npy` (n, C) next to each video;
                     with --piano also the roll loss and the Video2Roll metrics against `<video>.3.npy`.  Prints one JSON line per batch:
                     loss, roll_loss, precision, recall, f1, acc.  One rank only; nothing is written.
  --wav              (with --encodec) `<video>.wav` may have any sample rate: its first channel goes through the HIP wave front end
                     (wave.py: resampled to 24 kHz and normalised as the reference's data path does on the CPU,
                     trainer_multigpus_alldatas3.py:1047-1050, 1427-1431) into the HIP Encodec encoder.  Under --validate a video without
                     `<video>.latent.npy` takes its ground truth from `<video>.wav` (an existing `.latent.npy` wins); under
                     --audio-prompt-seconds the prompt is the first S seconds of the front end's output.
  --roll2midi CKPT   (with --piano) the Roll2Midi generator of the reference's Audeo chain, run as in Roll2Midi_inference.py: a
                     torch-saved checkpoint holding `state_dict_G`, or that state dict -- the plain net (src/audeo/Roll2MidiNet.py) or
                     the attention-gated one its trainer writes (Roll2MidiNet_enhance.py); the keys tell which.  The per-frame key
                     probabilities of the Video2Roll encoder go through it on the GPU and `<name>.midi.npz` is written next to each output:
                     `midi` (t, 51) uint8, the reference's key name (Roll2Midi_inference.py:79), and `prob` (t, 51) float32.
  --midi-file {midi,roll}   (with --piano) the next link, src/audeo/Midi_synth.py up to its FluidSynth rendering: the notes of the roll
                     (one v2a_roll_notes launch per batch) written as `<name>.mid`, a format-1 Standard MIDI File at tempo 80, program 0,
                     velocity 100 (Midi_synth.py:136-148).  midi: the notes of the Roll2Midi roll (needs --roll2midi); roll: the notes
                     of the Video2Roll encoder's own roll, probability >= 0.4 -- Midi_synth.py's shipped default -- without a generator.
The moviepy mux of audio and video stays outside (out of scope).
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

LATENT_RATE = 24000 / 320          # torch_tools.py:32-40


def read_scp(path: str, start: int, end: int, step: int = 1):
    out = []
    with open(path) as f:
        for ln in f.read().splitlines():
            if ln.strip():
                p, _, cap = ln.partition("\t")
                out.append((p, cap))
    return out[start:end:step]


def read_frames_with_moviepy(video_path: str):
    """x3:98-113: every decoded frame, (F, H, W, 3) uint8 RGB, and the clip duration in seconds (moviepy, imported on use)."""
    from moviepy.editor import VideoFileClip
    clip = VideoFileClip(video_path)
    return np.array(list(clip.iter_frames())), clip.duration


def read_audio_prompt(video_path: str, seconds: float) -> torch.Tensor:
    """The first `seconds` of `<video>.wav` as (nw,) float32 (first channel): 24 kHz, read with torchaudio or soundfile."""
    path = video_path.rsplit(".", 1)[0] + ".wav"
    nw = int(round(24000 * seconds))
    try:
        import torchaudio
        wav, rate = torchaudio.load(path)
        wav = wav[0]
    except ImportError:
        try:
            import soundfile
        except ImportError as e:
            raise RuntimeError("--audio-prompt-seconds reads <video>.wav with torchaudio or soundfile; neither is installed") from e
        data, rate = soundfile.read(path, dtype="float32", always_2d=True)
        wav = torch.from_numpy(data[:, 0].copy())
    if rate != 24000:
        raise ValueError(f"{path}: {rate} Hz, the Encodec encoder takes 24 000 Hz")
    if wav.shape[0] < nw:
        raise ValueError(f"{path}: {wav.shape[0]} samples, --audio-prompt-seconds {seconds} needs {nw}")
    return wav[:nw].float().contiguous()


def read_wave(path: str):
    """--wav: the first channel of an audio file at whatever rate it has -> ((n,) float32, rate), read with torchaudio or soundfile."""
    try:
        import torchaudio
        wav, rate = torchaudio.load(path)
        wav = wav[0]
    except ImportError:
        try:
            import soundfile
        except ImportError as e:
            raise RuntimeError("--wav reads <video>.wav with torchaudio or soundfile; neither is installed") from e
        data, rate = soundfile.read(path, dtype="float32", always_2d=True)
        wav = torch.from_numpy(data[:, 0].copy())
    return wav.float().contiguous(), int(rate)


def wave_prompt(model, video_path: str, seconds: float) -> torch.Tensor:
    """--wav --audio-prompt-seconds: the first `seconds` of `<video>.wav` after the front end (24 kHz, normalised), (nw,) on the device."""
    path = video_path.rsplit(".", 1)[0] + ".wav"
    nw = int(round(24000 * seconds))
    wav = model.wave_front_end()(*read_wave(path))
    if wav.shape[0] < nw:
        raise ValueError(f"{path}: {wav.shape[0]} samples at 24 000 Hz, --audio-prompt-seconds {seconds} needs {nw}")
    return wav[:nw]


def validation_sources(video_paths, wav: bool = False):
    """--validate: where each clip's ground-truth latents come from, ("latent", `<video>.latent.npy`) or, with --wav and no such
    file, ("wav", `<video>.wav`).  An existing `.latent.npy` wins; without --wav it is the only source, present or not."""
    out = []
    for vp in video_paths:
        stem = vp.rsplit(".", 1)[0]
        if wav and not os.path.exists(stem + ".latent.npy") and os.path.exists(stem + ".wav"):
            out.append(("wav", stem + ".wav"))
        else:
            out.append(("latent", stem + ".latent.npy"))
    return out


def load_audioldm_state_dict(path):
    """The state dict of --audioldm: a torch-saved dict of tensors, or a dict that holds one under `state_dict`.  Loaded with
    weights_only=True; a file that holds other objects (a trainer's whole checkpoint), or no dict at all, is refused with what to do."""
    import pickle
    try:
        ck = torch.load(path, map_location="cpu", weights_only=True)
    except pickle.UnpicklingError as e:
        raise ValueError(f"--audioldm {path}: the file holds objects other than tensors ({e}); save its state dict alone: "
                         f"torch.save(ckpt['state_dict'], ...)") from e
    sd = ck.get("state_dict", ck) if isinstance(ck, dict) else None
    if not isinstance(sd, dict) or not all(isinstance(k, str) for k in sd):
        raise ValueError(f"--audioldm {path}: expected a state dict, or a dict with one under 'state_dict', got {type(ck).__name__}")
    return sd


def build_requests(items, drop_prompt: bool, n_frames: int, t5_encode=None, clip_encode=None, video_encoder: str = "clip_vit", hop: int = 320,
                   rate: int = 24000):
    """clip_encode: optional `video_path -> (image_embeds, duration)` that makes a missing `<video>.generated.npz` (--clip);
    video_encoder: which cache name is read and written (--video-encoder); hop: samples per latent frame (320: Encodec; --vocos: the
    vocoder's hop; --audioldm: 640) at `rate` samples per second (--audioldm: 16000)."""
    from .collate import ClipRequest
    from .features import feature_cache_path, load_clip_cache, resample_clip_features, save_clip_cache
    reqs = []
    for vp, cap in items:
        fp = feature_cache_path(vp, video_encoder)
        if not os.path.exists(fp):
            if clip_encode is None:
                raise FileNotFoundError(f"{fp}: no cached CLIP features for {vp}; pass --clip DIR (with moviepy installed) to encode it")
            save_clip_cache(fp, *clip_encode(vp))                                # x3:1706-1793
        emb, duration = load_clip_cache(fp)
        n = min(n_frames, int(duration * rate) // hop) if n_frames > 0 else int(duration * rate) // hop
        clip = resample_clip_features(emb.float(), duration, n)
        prompt = "" if drop_prompt else cap
        t5p = vp.replace(".mp4", ".t5.npz")
        if t5_encode is not None:
            ctx = t5_encode(prompt if prompt else "the sound of X X")        # x3:2053-2056
        elif os.path.exists(t5p):
            ctx = torch.from_numpy(np.load(t5p)["arr_0"]).float()
        else:
            raise FileNotFoundError(f"{t5p}: no cached T5 context and no --t5 model")
        reqs.append(ClipRequest(vp, prompt, n, clip, ctx))
    return reqs


def piano_frames_for(video_paths, l: int, preprocess, decode, video_multi: float = 3.0):
    """--piano: the (b, 1, t, 100, 900) stack of a batch.  Clips with a frame cache are read from it; the others are decoded by
    `decode(video_path) -> (frames, duration)` and go through `preprocess` (a PianoFramePreprocessor), which also writes their cache.
    Without moviepy (`decode` raises ImportError) a missing cache is load_piano_frames' FileNotFoundError, as without this path.
    `video_multi`: latent frames per video frame of the piano configuration (--piano-keys)."""
    from .features import load_piano_frames, piano_frames_cache_path

    def frames_of(vp):
        if os.path.exists(piano_frames_cache_path(vp)):
            return None
        try:
            return decode(vp)
        except ImportError:
            return None

    return load_piano_frames(video_paths, l, video_frames=[frames_of(vp) for vp in video_paths], preprocess=preprocess,
                             video_multi=video_multi)


def validate_batch(model, video_paths, extras, frames=None, wav: bool = False) -> dict:
    """--validate: one `forward(val=True)` over a collated batch.  The ground-truth latents `<video>.latent.npy` (n, C) are zero
    padded to the longest clip of the batch and `lens` holds their lengths; `frames`: the --piano stack of the same clips.
    wav (--wav): a clip without `.latent.npy` is encoded from `<video>.wav` by `E2TTS.encode_audio`, cut at the batch's n frames."""
    from .features import load_midi_ground_truth
    n = extras["text_embed"].shape[1]
    lat = []
    for kind, path in validation_sources(video_paths, wav):
        if kind == "wav":
            w, rate = read_wave(path)
            z, zl = model.encode_audio([w], [rate], max_frames=n)
            lat.append(z[0, :int(zl[0])].cpu())
        else:
            lat.append(torch.from_numpy(np.load(path)).float())
    lens = torch.tensor([min(x.shape[0], n) for x in lat])
    inp = torch.stack([torch.nn.functional.pad(x[:n], (0, 0, 0, n - min(x.shape[0], n))) for x in lat])
    midis = None if frames is None else load_midi_ground_truth(video_paths, n, model.piano)
    r = model.forward(inp, times=0.5, lens=lens, val=True, frames=frames, midis=midis, text_embed=extras["text_embed"],
                      context=extras["context"], context_mask=extras["context_mask"])
    return dict(clips=len(video_paths), loss=float(r.loss), roll_loss=model.val_stats["roll"],
                **{k: float(v) for k, v in zip(("precision", "recall", "f1", "acc"), r.loss_breakdown)})


class _Parser(argparse.ArgumentParser):
    """`--video-encoder clip_vit2`, `clip_convnext` and `mixed` are errors without `--clip DIR`: the choice stands for the pair."""

    def parse_known_args(self, args=None, namespace=None):
        ns, rest = super().parse_known_args(args, namespace)
        if getattr(ns, "video_encoder", None) == "clip_vit2" and ns.clip is None:
            self.error("--video-encoder clip_vit2 needs --clip DIR (a local openai clip-vit-large-patch14-336 directory)")
        if getattr(ns, "video_encoder", None) == "clip_convnext" and ns.clip is None:
            self.error("--video-encoder clip_convnext needs --clip DIR (a local open_clip CLIP-convnext_xxlarge directory)")
        if getattr(ns, "video_encoder", None) == "mixed" and ns.clip is None:
            self.error("--video-encoder mixed needs --clip DIR (one subdirectory per choice: clip_vit, clip_vit2, clip_convnext, dinov2)")
        return ns, rest


def build_parser() -> argparse.ArgumentParser:
    ap = _Parser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("ckpt")
    ap.add_argument("drop_prompt", type=int)
    ap.add_argument("test_scp")
    ap.add_argument("start", type=int)
    ap.add_argument("end", type=int)
    ap.add_argument("out_dir")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=64)                 # src/inference_v2a.py:183
    ap.add_argument("--cfg-strength", type=float, default=2.0)
    ap.add_argument("--frames", type=int, default=750, help="latent frames per clip (10 s)")
    ap.add_argument("--dtype", default="bf16x3", choices=["bf16", "bf16x3", "fp32"],
                    help="bf16: fastest, |delta mel| ~ 5e-2 vs the fp32 reference arithmetic; bf16x3: split-bf16 products, < 1e-3 at ~0.4x the "
                         "bf16 speed; fp32: exact-fp32 MFMA, < 1e-3 at ~0.18x")
    ap.add_argument("--bucket-frames", type=int, default=64, help="pad plans to a multiple of this many latent frames (0 = exact shapes): "
                    "durations vary per clip, and every new shape costs a plan and a hipGraph capture")
    ap.add_argument("--bucket-ctx", type=int, default=16, help="pad the T5 context to a multiple of this many tokens (0 = exact)")
    ap.add_argument("--t5", default=None, help="local FLAN-T5 directory (reference: ./ckpts/flan-t5-large)")
    ap.add_argument("--t5-engine", default="torch", choices=["torch", "hip"],
                    help="what runs --t5: stock transformers on the CPU (torch) or the HIP T5Encoder on this rank's GPU (hip)")
    ap.add_argument("--clip", default=None, help="local CLIP image encoder directory (IP-Adapter sdxl_models/image_encoder): videos "
                    "without <video>.generated.npz are decoded with moviepy and encoded on this rank's GPU, and the cache is written")
    ap.add_argument("--video-encoder", default="clip_vit", choices=["clip_vit", "clip_vit2", "clip_convnext", "dinov2", "mixed"],
                    help="the frame encoder of the checkpoint: which class --clip DIR loads (CLIP ViT-bigG, CLIP ViT-L/14-336, CLIP ConvNeXt-XXLarge, "
                         "DINOv2, or all four side by side from DIR's subdirectories of those names) and which feature cache is used")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--model-config", default=None, help="JSON dict of transformer kwargs (default: predict.py:120-134)")
    ap.add_argument("--piano", action="store_true", help="V2P: condition on the piano frames through the Video2Roll encoder; a video without "
                    "<video>.generated_frames_raw.2.npz is decoded with moviepy and resized on this rank's GPU, and the cache is written")
    ap.add_argument("--piano-keys", type=int, default=51, choices=[51, 88],
                    help="the piano configuration of the checkpoint: 51 (e2_tts_crossatt3.py: keys 15..65, a video frame per 3 latent frames, "
                         "landscape frames) or 88 (e2_tts_crossatt3_2.py: all keys, a video frame per 2.5 latent frames, portrait frames "
                         "resized to 100 x 900 and transposed).  The frame cache <video>.generated_frames_raw.2.npz has the same name and "
                         "shapes under both, as in the reference: one written under the other value is silently wrong")
    ap.add_argument("--frames-dtype", default=None, choices=["fp32", "bf16", "bf16x3"],
                    help="compute mode of the Video2Roll encoder behind --piano (default: bf16 under --dtype bf16, else fp32); bf16x3: "
                         "split-bf16 implicit GEMM inside 1e-4 of the reference probabilities")
    ap.add_argument("--encodec", default=None, help="state dict (.pt) of the Encodec model / decoder: also write <name>.wav")
    ap.add_argument("--vocos", default=None, metavar="DIR", help="local Vocos directory (config.yaml, pytorch_model.bin) of a checkpoint whose latents "
                    "are mel frames: also write <name>.wav through the HIP Vocos; exclusive with --encodec")
    ap.add_argument("--audioldm", default=None, metavar="CKPT", help="local torch checkpoint of the AudioLDM VAE (a state dict, or a dict with one "
                    "under state_dict) of a checkpoint whose latents are its 128-channel latents: also write <name>.wav at 16 kHz through the HIP "
                    "VAE decoder and HiFi-GAN; exclusive with --vocos and --encodec")
    ap.add_argument("--audio-prompt-seconds", type=float, default=0.0, help="with --encodec and a checkpoint built with if_cond_proj_in: "
                    "prompt every clip with the first S seconds of <video>.wav, encoded by the HIP Encodec encoder")
    ap.add_argument("--codes", type=float, default=None, choices=[1.5, 3.0, 6.0, 12.0, 24.0], metavar="KBPS",
                    help="with --encodec: also write <name>.codes.npy, the int16 (n_q, n) Encodec codes of the clip at this bandwidth")
    ap.add_argument("--validate", action="store_true", help="instead of sampling, run the validation pass forward(val=True) on "
                    "<video>.latent.npy and print one JSON line per batch: loss, roll_loss, precision, recall, f1, acc")
    ap.add_argument("--wav", action="store_true", help="with --encodec: <video>.wav at any sample rate goes through the HIP wave front end "
                    "(resample to 24 kHz, normalize_wav) into the HIP Encodec encoder: the ground truth of --validate for a video without "
                    "<video>.latent.npy, and the prompt of --audio-prompt-seconds")
    ap.add_argument("--roll2midi", default=None, metavar="CKPT", help="with --piano: checkpoint (or state dict) of the Roll2Midi generator "
                    "(`state_dict_G` of Roll2MidiNet.py or of Roll2MidiNet_enhance.py, told apart by its keys): also write <name>.midi.npz with `midi` (t, 51) uint8 and `prob` (t, 51) float32 per video frame")
    ap.add_argument("--roll2midi-dtype", default="bf16x3", choices=["fp32", "bf16", "bf16x3"], help="compute mode of the Roll2Midi generator")
    ap.add_argument("--midi-file", default=None, choices=["midi", "roll"],
                    help="with --piano: also write <name>.mid, a Standard MIDI File of the clip's notes (Midi_synth.py up to the FluidSynth "
                         "rendering): midi = from the Roll2Midi generator's roll (needs --roll2midi), roll = from the Video2Roll encoder's "
                         "own roll, probability >= 0.4 (the reference's shipped default)")
    return ap


def write_midi_rolls(model, frames, video_paths, out_dir, midi_file: bool = False) -> list:
    """--roll2midi: `E2TTS.frames_to_midi` over the --piano stack of a batch -> `<out_dir>/<name>.midi.npz` per clip.
    midi_file (--midi-file midi): the notes of the same roll, taken on the device, also go to `<out_dir>/<name>.mid`."""
    probs, midi = model.frames_to_midi(frames)
    notes = model.midi_to_notes(midi) if midi_file else None
    probs, midi = probs.cpu().numpy(), midi.cpu().numpy()
    paths = []
    for i, vp in enumerate(video_paths):
        name = vp.rsplit("/", 1)[-1].rsplit(".", 1)[0]
        paths.append(os.path.join(out_dir, name + ".midi.npz"))
        np.savez(paths[-1], midi=midi[i], prob=probs[i])
    if midi_file:
        paths += write_note_files(notes, video_paths, out_dir, model.piano_spf)
    return paths


def write_note_files(notes, video_paths, out_dir, spf) -> list:
    """--midi-file: one clip's rows (pitch, start_frame, end_frame) per video -> `<out_dir>/<name>.mid` (midi.write_midi)."""
    from .midi import write_midi
    paths = []
    for one, vp in zip(notes, video_paths):
        name = vp.rsplit("/", 1)[-1].rsplit(".", 1)[0]
        paths.append(os.path.join(out_dir, name + ".mid"))
        write_midi(paths[-1], one, spf)
    return paths


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.audio_prompt_seconds < 0 or (a.audio_prompt_seconds > 0 and not a.encodec):
        ap.error("--audio-prompt-seconds needs a positive S and --encodec (the state dict that holds the encoder)")

    if a.vocos and a.encodec:
        ap.error("--vocos and --encodec are exclusive: each is the vocoder of its own latents (mel frames / Encodec latents)")

    if a.audioldm and (a.vocos or a.encodec):
        ap.error("--audioldm is exclusive with --vocos and --encodec: each is the vocoder of its own latents (VAE latents / mel frames / "
                 "Encodec latents)")

    if a.codes is not None and not a.encodec:
        ap.error("--codes needs --encodec (the state dict that holds the quantizer's codebooks)")

    if a.wav and not a.encodec:
        ap.error("--wav needs --encodec (the state dict that holds the encoder)")

    if a.roll2midi and not a.piano:
        ap.error("--roll2midi needs --piano (the frames the Video2Roll encoder reads)")

    if a.midi_file and not a.piano:
        ap.error("--midi-file needs --piano (the frames the Video2Roll encoder reads)")

    if a.midi_file == "midi" and not a.roll2midi:
        ap.error("--midi-file midi needs --roll2midi (the generator whose roll the notes are taken from); --midi-file roll does without")

    if a.validate and int(os.environ.get("WORLD_SIZE", 1)) > 1:
        ap.error("--validate runs on one rank")

    import torch.distributed as dist
    from . import E2TTS, collate_clips, gather_latents, shard_range
    rank, world, local = (int(os.environ.get(k, d)) for k, d in (("RANK", 0), ("WORLD_SIZE", 1), ("LOCAL_RANK", 0)))
    if world > 1:
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    tk = dict(depth=12, dim=1024, dim_text=1280, heads=16, dim_head=64)
    if a.model_config:
        import json
        tk = json.loads(a.model_config)
    channels = tk.pop("num_channels", 128)
    model = E2TTS(transformer=dict(if_text_modules=True, if_cross_attn=True, if_audio_conv=True, if_text_conv=True, **tk),
                  num_channels=channels, sampling_rate=24000, if_cond_proj_in=a.audio_prompt_seconds > 0, tokenizer="phoneme_zh",
                  audiocond_drop_prob=0.3 if a.audio_prompt_seconds > 0 else 1.1,          # predict.py:71-72, 144: the two travel together
                  compute_dtype=a.dtype, device=torch.device("cuda", local), bucket_frames=a.bucket_frames, bucket_ctx=a.bucket_ctx,
                  frames_compute_dtype=a.frames_dtype, video_encoder=a.video_encoder, piano_keys=a.piano_keys)
    ck = torch.load(a.ckpt, map_location="cpu")
    res = model.load_state_dict(ck.get("model_state_dict", ck), strict=False)      # predict.py:161-168
    if res.missing_keys:
        raise RuntimeError(f"checkpoint lacks {len(res.missing_keys)} parameters of the sampled path, e.g. {res.missing_keys[0]}")
    if a.roll2midi:
        model.load_roll2midi(a.roll2midi, compute=a.roll2midi_dtype)
    t5_encode = None
    if a.t5 and a.t5_engine == "hip":
        from .t5 import T5Encoder
        enc = T5Encoder.from_pretrained(a.t5, torch.device("cuda", local))
        def t5_encode(prompt):
            return enc([prompt])[0][0].cpu()
    elif a.t5:
        from transformers import AutoTokenizer, T5EncoderModel
        tok, enc = AutoTokenizer.from_pretrained(a.t5), T5EncoderModel.from_pretrained(a.t5).eval()
        def t5_encode(prompt):
            b = tok([prompt], max_length=tok.model_max_length, padding=True, truncation=True, return_tensors="pt")
            with torch.no_grad():
                return enc(input_ids=b.input_ids, attention_mask=b.attention_mask)[0][0]
    decoded: dict = {}                 # video path -> (frames, duration): --clip and --piano share one moviepy decode per batch

    def decode(vp):
        if vp not in decoded:
            decoded[vp] = read_frames_with_moviepy(vp)
        return decoded[vp]

    clip_encode = None
    if a.clip:
        from .e2tts import IMAGE_ENCODERS
        cenc = IMAGE_ENCODERS.get(a.video_encoder, IMAGE_ENCODERS["clip_vit"]).from_pretrained(a.clip, torch.device("cuda", local))
        def clip_encode(vp):
            try:
                frames, duration = decode(vp)
            except ImportError as e:
                raise FileNotFoundError(f"{vp}: no cached CLIP features and moviepy is not installed to decode it for --clip") from e
            if a.video_encoder == "mixed":                          # the parts' own caches are read and written too (x3:1745-1788)
                from .features import encode_mixed_cached
                return encode_mixed_cached(vp, frames, duration, cenc), duration
            return cenc(frames).cpu(), duration
    if a.audio_prompt_seconds > 0 or a.wav:                          # a checkpoint without cond_proj_in.* was refused above
        model.load_audio_encoder(torch.load(a.encodec, map_location="cpu"))
    vocoder = None
    if a.encodec and rank == 0:
        from .encodec import EncodecDecoder
        esd = torch.load(a.encodec, map_location="cpu")
        vocoder = EncodecDecoder(esd, torch.device("cuda", local))
        if a.codes is not None:
            model.load_audio_quantizer(esd)
    hop = 320                                                        # samples per latent frame (torch_tools.py:32-40)
    if a.vocos:
        voc = model.load_vocoder(a.vocos)                            # refuses a vocoder whose channels are not the model's
        hop = voc.hop
        vocoder = voc if rank == 0 else None
    rate = 24000
    if a.audioldm:                                                   # x3:1404-1409: the 'vae' vocoder, 16 kHz, 640 samples per latent frame
        from .audioldm_vae import VaeVocoder
        voc = model.load_vocoder(VaeVocoder.from_state_dict(load_audioldm_state_dict(a.audioldm), torch.device("cuda", local)))
        hop, rate = voc.hop, 16000
        vocoder = voc if rank == 0 else None
    items = read_scp(a.test_scp, a.start, a.end)
    os.makedirs(a.out_dir, exist_ok=True)
    gen = torch.Generator().manual_seed(a.seed)
    written = []
    for b0 in range(0, len(items), a.batch):
        chunk = items[b0:b0 + a.batch]
        s, e, per = shard_range(len(chunk), rank, world)
        mine = chunk[s:e]
        if mine:
            batch8, extras = collate_clips(build_requests(mine, bool(a.drop_prompt), a.frames, t5_encode, clip_encode, a.video_encoder, hop, rate), channels, gen, notes=model.cfg.notes)
            frames = None
            if a.piano:
                # x3:1829, predict.py:231; a clip without a frame cache is decoded and resized on this rank's GPU, its cache written
                frames = piano_frames_for([vp for vp, _ in mine], int(batch8[3].max()), model.piano_frame_preprocessor(), decode,
                                          model.piano.video_multi)
            decoded.clear()
            if a.roll2midi and frames is not None and not a.validate:
                written += write_midi_rolls(model, frames, [vp for vp, _ in mine], a.out_dir, midi_file=a.midi_file == "midi")
            if a.midi_file == "roll" and frames is not None and not a.validate:
                written += write_note_files(model.frames_to_notes(frames, source="roll"), [vp for vp, _ in mine], a.out_dir, model.piano_spf)
            if a.validate:
                import json
                print(json.dumps(dict(batch=b0 // a.batch, **validate_batch(model, [vp for vp, _ in mine], extras, frames, a.wav))), flush=True)
                continue
            cond, lens = batch8[1], batch8[3]
            if frames is not None:
                # the collator's all-zero roll would win over `frames` in sample() (a given frames_embed is taken as the roll):
                # with --piano the roll comes from the frames, through the Video2Roll encoder
                extras.pop("frames_embed")
            if a.audio_prompt_seconds > 0:                           # raw waves (b, nw): sample() encodes them (x3:2157-2160)
                cond = torch.stack([wave_prompt(model, vp, a.audio_prompt_seconds) if a.wav else read_audio_prompt(vp, a.audio_prompt_seconds)
                                    for vp, _ in mine])
                lens = torch.full((len(mine),), -(-cond.shape[1] // 320), dtype=torch.int32)
            lat = model.sample(cond, lens=lens, duration=batch8[3], steps=a.steps, cfg_strength=a.cfg_strength,
                               remove_parallel_component=False, sway_sampling=True, video_drop_prompt=batch8[4],
                               return_raw_output=True, frames=frames, **extras).to(torch.device("cuda", local))
        else:
            lat = torch.zeros(0, a.frames, channels, device=torch.device("cuda", local))
        if lat.shape[1] < a.frames:
            lat = torch.nn.functional.pad(lat, (0, 0, 0, a.frames - lat.shape[1]))
        allat = gather_latents(lat, len(chunk), per)
        if rank == 0:
            for (vp, _), one in zip(chunk, allat):
                name = vp.rsplit("/", 1)[-1].rsplit(".", 1)[0]
                path = os.path.join(a.out_dir, name + ".latent.npy")
                np.save(path, one.float().cpu().numpy())
                written.append(path)
                if vocoder is not None:
                    from scipy.io import wavfile
                    from .features import load_clip_cache, feature_cache_path
                    n = min(a.frames, int(load_clip_cache(feature_cache_path(vp, a.video_encoder))[1] * rate) // hop) if a.frames > 0 else one.shape[0]
                    wav = vocoder.decode(one[:n].t()[None].float())[0]                     # predict.py:277-278
                    wavfile.write(os.path.join(a.out_dir, name + ".wav"), rate, wav.cpu().numpy())
                    if a.codes is not None:
                        codes = model.latents_to_codes(one[None, :n].float(), a.codes)[0]          # (n_q, n)
                        np.save(os.path.join(a.out_dir, name + ".codes.npy"), codes.cpu().numpy().astype(np.int16))
    if world > 1:
        dist.destroy_process_group()
    return written


if __name__ == "__main__":
    main()
