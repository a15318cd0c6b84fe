"""Cached CLIP features: on-disk format and frame-rate resampler.

Mirrors the cache half of `E2TTS.encode_video` (x3:1659-1827, `x3` =
/root/reference/src/e2_tts_pytorch/e2_tts_crossatt3.py): the CLIP image encoder runs once per
video and its output is kept next to the video as an `.npz` written by
`np.savez(feature_path, image_embeddings, duration)` (x3:1793), i.e.
    arr_0 : (n_video_frames, dim) float embeddings, one per decoded video frame
    arr_1 : 0-d float, clip duration in seconds
and every later call only resamples those rows to the 75 Hz latent rate by nearest video frame
(x3:1803-1813).  A missing cache is made by the HIP ViT-bigG encoder (clip.py: 0.75 s per 250-frame clip in bf16x3) through
`encode_video_cached(..., encoder_fn=)`, which E2TTS.sample(video_frames=...) and the CLI's --clip drive.
The V2P side has the same two halves: the grey-frame cache `<video>.generated_frames_raw.2.npz` with its nearest-frame selection,
and, for a video without one, `load_piano_frames(video_frames=, preprocess=)` over the HIP preprocessor of piano_frames.py.
"""
from __future__ import annotations

import os
from typing import NamedTuple

import numpy as np
import torch


# ---- the two piano configurations the reference ships ----------------------------------------------------------------------
class PianoConfig(NamedTuple):
    """What differs between e2_tts_crossatt3.py (x3) and e2_tts_crossatt3_2.py (x3_2), the same file with three switches flipped:
    `notes`, `note_min`, `note_max` (`NOTES`, `NOTTE_MIN`, `NOTE_MAX`, :70-76), `video_multi` latent frames per video frame
    (:1929-1930), `expand` = (rep, group) of encode_frames -- every roll row `rep` times, every `group` of them averaged
    (:1544-1547) -- and the frame `layout` of the module-level `transform` (:60-68): "landscape" resizes to 900 x 100,
    "portrait" to 100 wide x 900 tall and transposes, out[i, j] = img[j, i].  Both give (100, 900) frames."""
    notes: int
    note_min: int
    note_max: int
    video_multi: float
    expand: tuple
    layout: str


PIANO_51 = PianoConfig(51, 15, 65, 3.0, (3, 1), "landscape")          # x3, trainer_multigpus_alldatas3.py (piano_2h, 25 fps)
PIANO_88 = PianoConfig(88, 0, 87, 2.5, (5, 2), "portrait")            # x3_2, trainer_multigpus_alldatas3_2.py (piano_20h, 30 fps)
PIANO_CONFIGS = {51: PIANO_51, 88: PIANO_88}


def piano_config(piano_keys) -> PianoConfig:
    """51 | 88 (or a PianoConfig) -> the configuration; anything else is a ValueError."""
    if isinstance(piano_keys, PianoConfig):
        return piano_keys
    if isinstance(piano_keys, bool) or piano_keys not in PIANO_CONFIGS:
        raise ValueError(f"piano_keys must be 51 or 88, got {piano_keys!r}")
    return PIANO_CONFIGS[piano_keys]


_SUFFIX = {"clip_vit": ".generated.npz", "clip_vit2": ".generated.clip_vit2.npz",
           "clip_convnext": ".generated.clip_convnext.npz", "dinov2": ".generated.dinov2.npz", "mixed": ".generated.mixed.npz"}
_VGG_DIR = {"clip_vit": "/feature/", "clip_vit2": "/feature_clip_vit2/", "clip_convnext": "/feature_clip_convnext/",
            "dinov2": "/feature_dinov2/", "mixed": "/feature_mixed/"}
_VGG_ROOT = "/ailab-train2/speech/zhanghaomin/VGGSound/"


def feature_cache_path(video_path: str, video_encoder: str = "clip_vit") -> str:
    """x3:1678-1701: where encode_video looks for / writes the cache of one video."""
    if video_encoder not in _SUFFIX:
        raise ValueError("Invalid video_encoder " + video_encoder)
    if video_path.startswith(_VGG_ROOT):
        return video_path.replace("/video/", _VGG_DIR[video_encoder]).replace(".mp4", ".npz")
    return video_path.replace(".mp4", _SUFFIX[video_encoder])


def save_clip_cache(path: str, image_embeddings, duration: float) -> None:
    """x3:1793 `np.savez(feature_path, image_embeddings, duration)` -> keys arr_0, arr_1."""
    emb = image_embeddings.detach().cpu().numpy() if torch.is_tensor(image_embeddings) else np.asarray(image_embeddings)
    np.savez(path, emb, duration)


def load_clip_cache(path: str) -> tuple[torch.Tensor, float]:
    """x3:1796-1800."""
    data = np.load(path)
    return torch.from_numpy(data["arr_0"]), data["arr_1"].item()


def resample_indices(n_video_frames: int, duration: float, l: int, sampling_rate: int = 24000, frame_size: int = 320,
                     start_sample: int = 0, max_sample: int | None = None) -> list[int]:
    """x3:1801-1808: for every latent frame (hop `frame_size` samples) the index of the nearest video frame,
    at most `l` of them.  Python's round() (half to even) is part of the reference behaviour."""
    if max_sample is None:
        max_sample = int(duration * sampling_rate)
    out = []
    for i in range(start_sample, max_sample, frame_size):
        j = min(round((i + frame_size // 2) / sampling_rate / (duration / (n_video_frames - 1))), n_video_frames - 1)
        out.append(j)
        if len(out) >= l:
            break
    return out


def resample_clip_features(image_embeddings: torch.Tensor, duration: float, l: int, **kw) -> torch.Tensor:
    """(n_video_frames, dim) -> (l, dim): nearest-frame resampling, zero padded to l (x3:1815-1824)."""
    idx = resample_indices(image_embeddings.shape[0], duration, l, **kw)
    out = torch.zeros(l, image_embeddings.shape[1], dtype=image_embeddings.dtype)
    if idx:
        out[: len(idx)] = image_embeddings[torch.tensor(idx)]
    return out


def encode_video_cached(video_paths, l: int, dim: int = 1280, video_encoder: str = "clip_vit", sampling_rate: int = 24000,
                        frame_size: int = 320, encoder_fn=None) -> torch.Tensor:
    """Batch form of encode_video for cached features: (b, l, dim) float32 on the CPU.
    `None` paths give zero rows (x3:1669-1672); tuples are (path, start_sample, max_sample) (x3:1673-1674).
    A missing cache is produced by `encoder_fn(video_path) -> (embeddings, duration)` and saved, as the
    reference does with its CLIP model (x3:1706-1793); without encoder_fn it is an error."""
    rows = []
    for vp in video_paths:
        if vp is None:
            rows.append(torch.zeros(l, dim))
            continue
        start_sample, max_sample = 0, None
        if isinstance(vp, tuple):
            vp, start_sample, max_sample = vp
        fp = feature_cache_path(vp, video_encoder)
        if not os.path.exists(fp):
            if encoder_fn is None:
                raise FileNotFoundError(f"{fp}: no cached CLIP features for {vp} and no encoder_fn to create them")
            emb, duration = encoder_fn(vp)
            save_clip_cache(fp, emb, duration)
        emb, duration = load_clip_cache(fp)
        rows.append(resample_clip_features(emb.float(), duration, l, sampling_rate=sampling_rate, frame_size=frame_size,
                                           start_sample=start_sample, max_sample=max_sample))
    return torch.stack(rows, 0)


def encode_mixed_cached(video_path: str, frames, duration: float, mixed) -> torch.Tensor:
    """The `mixed` branch of encode_video for one uncached video (x3:1745-1788): every part (`clip_vit`, `clip_vit2`, `clip_convnext`,
    `dinov2`) is read from its own cache next to the video when that exists, else computed by `mixed.encoders[part]` and written
    there -- the reference leaves the write of the clip_vit part commented out; here all four are written, under the names their own
    choices use -- and the parts are joined per frame, cut to the shortest: (F, sum of widths) float32 on the CPU.  The caller
    writes the `.generated.mixed.npz` cache."""
    parts = {}
    for k, enc in mixed.encoders.items():
        fp = feature_cache_path(video_path, k)
        if os.path.exists(fp):
            parts[k] = load_clip_cache(fp)[0].float()
        else:
            parts[k] = enc(frames).cpu()
            save_clip_cache(fp, parts[k], duration)
    return mixed.concat(parts)


# ---- piano-frame cache of the V2P path (the `piano` branch of E2TTS.encode_video_frames, x3:1829-1991) ------------------
def piano_frames_cache_path(video_path: str) -> str:
    """x3:1876: the grey 100x900 frames of a video are cached next to it."""
    return video_path.replace(".mp4", ".generated_frames_raw.2.npz")


def save_piano_frames_cache(path: str, frames_raw, duration: float) -> None:
    """x3:1890-1891 `np.savez(frames_raw_path, frames_raw, duration)`: arr_0 = (n_video_frames, 100, 900, 1) float32 in
    [0, 1] (ToTensor of the 'L' image), arr_1 = duration in seconds."""
    fr = frames_raw.detach().cpu().numpy() if torch.is_tensor(frames_raw) else np.asarray(frames_raw)
    np.savez(path, fr.astype(np.float32), duration)


def piano_frame_indices(n_video_frames: int, duration: float, l: int, start_sample: int = 0, max_sample: int | None = None,
                        video_multi: float = 3.0, sampling_rate: int = 24000, frame_size: int = 320) -> list[int]:
    """x3:1903-1913: one video frame per `video_multi` latent frames (hop 3 * 320 samples), nearest by time, at most
    floor(l / video_multi) + 1 of them.  The loop runs one hop past max_sample, as the reference's does."""
    if max_sample is None:
        max_sample = int(duration * sampling_rate)
    hop = int(video_multi * frame_size)
    out = []
    for i in range(start_sample, max_sample + hop, hop):
        out.append(min(round(i / sampling_rate / (duration / n_video_frames)), n_video_frames - 1))
        if len(out) >= int(l // video_multi) + 1:
            break
    return out


def piano_frames_from_video(frames, duration: float, l: int, preprocess, start_sample: int = 0, max_sample: int | None = None,
                            video_multi: float = 3.0) -> torch.Tensor:
    """One clip's (t_i, Ho, Wo) float32 stack from its decoded frames (F, H, W, 3) uint8: the frames `piano_frame_indices` picks,
    each distinct one resized once by `preprocess(frames, select=[...]) -> (n, Ho, Wo)` (a `PianoFramePreprocessor`) and then
    gathered -- a 30 fps clip repeats no frame, a 12 fps one uses each about twice.  The result stays on preprocess's device."""
    idx = piano_frame_indices(frames.shape[0], duration, l, start_sample, max_sample, video_multi)
    distinct = sorted(set(idx))
    out = preprocess(frames, select=distinct)
    if len(distinct) == len(idx):
        return out
    pos = {j: k for k, j in enumerate(distinct)}
    return out[torch.tensor([pos[j] for j in idx], device=out.device)]


def load_piano_frames(video_paths, l: int, *, video_frames=None, preprocess=None, write_cache: bool = True,
                      video_multi: float = 3.0) -> torch.Tensor | None:
    """Batch form of the `piano` branch of encode_video_frames: (b, 1, t, 100, 900) float32 with
    t = max(floor(l / video_multi) + 1, longest clip) and zero frames as padding (x3:1935-1948); `None` paths give all-zero clips
    (x3:1939-1941).  Returns None when no path has frames (x3:1927-1928).  Tuples are (path, start_sample, max_sample).
    `video_frames`: one (frames uint8 (F, H, W, 3), duration_s) or None per path, the decoded video of a clip whose cache may be
    missing; such a clip goes through `preprocess` (x3:1877-1891) instead of raising.  With `write_cache` all its F frames are
    resized and saved in the reference's format, so that the reference and the next call read them; without, only the frames the
    clip uses are resized and nothing is written.  An existing cache wins.  The result is on preprocess's device when any clip
    was preprocessed, else on the CPU.
    `video_multi` (`PianoConfig.video_multi`): 3.0, or 2.5 for the 88-key configuration, whose `preprocess` is the portrait one.
    The cache name is the same in both reference files and so are the shapes: a cache written under one configuration is
    silently wrong under the other, here as there."""
    if video_frames is not None and len(video_frames) != len(video_paths):
        raise ValueError(f"video_frames: {len(video_frames)} entries for {len(video_paths)} video_paths")
    clips, lens = [], []
    for n, vp in enumerate(video_paths):
        if vp is None:
            clips.append(None)
            lens.append(0)
            continue
        start_sample, max_sample = 0, None
        if isinstance(vp, tuple):
            vp, start_sample, max_sample = vp
        fp = piano_frames_cache_path(vp)
        if os.path.exists(fp):
            data = np.load(fp)
            raw = torch.from_numpy(data["arr_0"])
            idx = piano_frame_indices(raw.shape[0], data["arr_1"].item(), l, start_sample, max_sample, video_multi)
            clip = raw[torch.tensor(idx)]
        elif video_frames is not None and video_frames[n] is not None:
            if preprocess is None:
                raise ValueError("load_piano_frames: video_frames needs preprocess= (a PianoFramePreprocessor)")
            fr, duration = video_frames[n]
            if write_cache:
                raw = preprocess(fr).unsqueeze(-1)                                # (F, 100, 900, 1), x3:1890
                save_piano_frames_cache(fp, raw, float(duration))
                idx = piano_frame_indices(raw.shape[0], float(duration), l, start_sample, max_sample, video_multi)
                clip = raw[torch.tensor(idx, device=raw.device)]
            else:
                clip = piano_frames_from_video(fr, float(duration), l, preprocess, start_sample, max_sample, video_multi).unsqueeze(-1)
        else:
            raise FileNotFoundError(f"{fp}: no cached piano frames for {vp} (the reference decodes the video with moviepy here)")
        clips.append(clip)
        lens.append(clip.shape[0])
    if not any(c is not None for c in clips):
        return None
    H, W = next(c for c in clips if c is not None).shape[1:3]
    dev = next((c.device for c in clips if c is not None and c.device.type != "cpu"), torch.device("cpu"))
    t = max(int(l // video_multi) + 1, max(lens))
    out = torch.zeros(len(clips), t, H, W, 1, device=dev)
    for i, c in enumerate(clips):
        if c is not None:
            out[i, : c.shape[0]] = c
    return out.permute(0, 4, 1, 2, 3).contiguous()


# ---- MIDI ground truth of the V2P validation pass (x3:1852-1866) -------------------------------------------------------
NOTE_MIN, NOTE_MAX = PIANO_51.note_min, PIANO_51.note_max          # x3:71-72 (`NOTTE_MIN`, `NOTE_MAX`): the 51 piano keys the roll covers


def midi_ground_truth_path(video_path: str) -> str:
    """x3:1852: the frame-level MIDI roll of a clip lies next to it."""
    return video_path.replace(".mp4", ".3.npy")


def load_midi_ground_truth(video_paths, l: int, piano_keys=51) -> torch.Tensor | None:
    """x3:1852-1866: `<video>.3.npy` (frames, 88 keys) -> columns note_min..note_max of the configuration (15..65, or all 88 with
    piano_keys=88) as float32, zero padded or cut to `l` frames: (b', l, notes) over the paths that are not None (tuples are (path, start_sample, max_sample)), or None when there is none.  This is
    `midis` of `E2TTS.forward(val=True)`; `E2TTS.encode_video_frames` keeps returning zeros, as the reference's live branch does."""
    pc = piano_config(piano_keys)
    rows = []
    for vp in video_paths:
        if vp is None:
            continue
        if isinstance(vp, tuple):
            vp = vp[0]
        gt = torch.from_numpy(np.load(midi_ground_truth_path(vp)).astype(np.float32))[:, pc.note_min:pc.note_max + 1]
        out = torch.zeros(int(l), gt.shape[1])
        k = min(int(l), gt.shape[0])
        out[:k] = gt[:k]
        rows.append(out)
    return torch.stack(rows, 0) if rows else None
