"""Clip-wise video inference and repetition counting on top of the HIP TSM engine.

Counterpart of workoutdetector/utils/inference_count.py for the video-model path:

  inference_video        :246-282   one clip -> [(class_id, score)] * num_class (unsorted enumerate)
  inference_dataset      :342-421   every video of the selected splits -> {out_dir}/{video}.score.json
  count_by_video_model   :285-339   streaming 8-frame windows -> (count, reps)   [intent, see below]
  pred_to_count          :114-165   (re-exported from .counting)
  inference_image        :168-189   one frame through the IMAGE model -> scores [num_class]
  count_by_image_model   :192-243   per-frame scores, vote over the last 7 arg-maxes, pred_to_count(states, step=7)
  save_scores_to_json    :47-67

What differs from the reference, on purpose:
  * ``model`` is anything with the onnxruntime duck type (``get_inputs()[0].name`` / ``run``) -- the batched paths also take a
    torch module or a plain callable (``staging.call_host``); ``inference_video`` keeps the reference's session call; a
    ``TsmEngine`` additionally gets the batched device path: the uint8 frames of a video go to the GPU
    once, the fused HIP transform (``tsm_preprocess``: resize 256 / crop 224 / normalise -> NHWC4) runs
    once per *frame* (each even frame belongs to two half-overlapping windows; the transform is
    per-frame, so this equals transforming per clip) and the windows are pushed through the engine in
    batches instead of one synchronous ``run`` per clip.
  * ``person_crop=True`` takes the boxes from the caller (``boxes=``; the Faster-RCNN detector is out of scope): the box is
    per clip, so the transform moves behind the clip windows -- one ``tsm_preprocess_clips`` launch per batch cuts,
    crops, resizes, normalises and packs straight from the staged uint8 frames (``shard='clips'`` / ``'videos'``).
  * videos come from a pluggable ``video_reader`` (the image has no H.264 decoder): ``.npy`` files of
    uint8 [F,H,W,3] frames are read natively, anything else goes to ``torchvision.io.read_video`` when
    that is importable.
  * under ``torch.distributed`` a dataset run lays out the global (video, clip) index once: whole videos go to
    ranks longest-first by clip count, every rank runs full batches with no collective in its loop, and the
    per-clip logits are all-gathered ONCE at the end (RCCL over xGMI with the nccl backend); every rank writes
    the JSON files of its own videos (``shard='global'``).  ``shard='clips'`` splits the clips of each video instead (one all-gather per
    video: the single-stream latency form); ``shard='videos'`` is the lock-stepped round-robin of round 2.
  * ``count_by_video_model`` in the reference snapshot is broken (asserts on the missing transform and
    always reads class 0 from an unsorted list, :270,:276,:327); this one implements the documented
    intent: arg-max class of each non-overlapping 8-frame window, softmax + threshold as in
    utils/eval.py:153-164, incremental ``pred_to_count``.

Reference quirks reproduced by default (flags to change): frames are NOT divided by 255
(``scale_255=False``), the tail clip is zero-padded, windows take 8 frames out of 16 with stride 2,
``scores`` is keyed by the clip's first frame index and JSON turns the int keys into strings.
"""
from __future__ import annotations

import json
import os
import os.path as osp
import queue
import threading
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import Callable, Deque, Dict, Iterable, Iterator, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import distributed as tdist
from . import staging
from .counting import RepCounter, pred_to_count, scores_to_preds, vote_states  # noqa: F401  (re-export)
from .repcount import RepcountHelper
from .transform import (ImageTransform, PersonCropTransform, TestTransform, as_frames_u8, build_test_transform,
                        black_frame, check_frame_format, frame_hw, need_frame_engine, nv12_black, nv12_to_rgb,
                        yuv_frame_bytes_view, yuv_to_rgb)

NUM_SEGMENTS = 8
CLIP_SPAN = 16
CLIP_STRIDE = 2
CLIP_STEP = 8
# Upper bound on the uint8 frames of one video staged (page-locked + on the device) at a time.  A long 1080p video
# holds several GB of even frames; beyond this bound the clip range is processed in pieces (each piece re-stages the
# 8-frame overlap it needs), so pinned host memory stays <= 3 pool slots x 1.25 x this and device memory proportional.
MAX_STAGE_BYTES = 1 << 30
PIECE_CLIPS = 64              # clips per staged piece of the dataset loop (two batches of 32: 58 MB of 360 x 206 frames)


# ---- video sources -------------------------------------------------------------------------------------
def read_video(path: str) -> torch.Tensor:
    """uint8 [F,H,W,3].  ``.npy`` raw frames natively; otherwise torchvision.io.read_video if present."""
    if path.endswith('.npy'):
        arr = np.load(path, mmap_mode='r')
        if arr.dtype != np.uint8 or arr.ndim != 4 or arr.shape[-1] != 3:
            raise ValueError(f'{path}: expected uint8 [F,H,W,3], got {arr.dtype} {arr.shape}')
        return torch.from_numpy(np.array(arr))  # copy out of the read-only memory map
    try:
        from torchvision.io import read_video as tv_read_video  # type: ignore
    except ImportError as e:
        raise RuntimeError(f'cannot decode {path}: no video decoder in this environment (torchvision.io absent); '
                           'pass video_reader=... or provide frames as a uint8 .npy [F,H,W,3]') from e
    return tv_read_video(path)[0]


def clip_starts(total_frames: int, step: int = CLIP_STEP) -> List[int]:
    """First source frame of every clip: ``range(0, len(vid), 8)`` (utils/inference_count.py:411)."""
    return list(range(0, total_frames, step))


def make_clip(video_thwc_u8: torch.Tensor, start: int) -> torch.Tensor:
    """``vid[start:start+16:2]`` zero-padded to 8 frames, promoted to float32 0..255 (:412-414)."""
    clip = video_thwc_u8[start:start + CLIP_SPAN:CLIP_STRIDE].to(torch.float32)
    pad = NUM_SEGMENTS - clip.shape[0]
    if pad > 0:
        clip = torch.cat([clip, torch.zeros((pad,) + tuple(clip.shape[1:]), dtype=torch.float32, device=clip.device)])
    return clip


def need_clip_rows(model, where: str) -> None:
    """The pipelines here take ONE row of scores per clip: refuse a model that returns one per segment up front (an engine
    built with consensus_type='identity', logits [B, T, num_class]) instead of failing later on a shape.  Sessions and
    stubs without the attribute are 'avg'.  They also build clips of ONE frame per segment: a TDN engine, which takes five, is
    refused here too (NotImplementedError), never run on the wrong input."""
    if getattr(model, 'tdn_depths', None):
        raise NotImplementedError(f'{where} builds clips of one frame per segment; a TDN engine takes five ([B, T, 5, 3, H, W]): '
                                  'call the engine on clips you assemble yourself')
    consensus = getattr(model, 'consensus_type', 'avg')
    if consensus != 'avg':
        raise ValueError(f"{where} needs one row of scores per clip: the model was built with consensus_type={consensus!r} "
                         "(per-segment logits [B, T, num_class]); build it with consensus_type='avg'")


# ---- single clip, reference signature ------------------------------------------------------------------
def inference_video(model, inputs: Union[torch.Tensor, np.ndarray], threshold: float = 0.5,
                    transform: Optional[Callable] = None) -> List[Tuple[int, float]]:
    """One clip through ``model``; returns ``list(enumerate(scores))`` like the reference's ORT branch.

    inputs: Tensor [8,H,W,3] (decoder layout; permuted to [8,3,H,W] here) or ndarray already [8,3,H,W].
    ``threshold`` is accepted and unused, as in the reference (:248,:258)."""
    need_clip_rows(model, 'inference_video')
    if not isinstance(inputs, torch.Tensor):
        x = torch.from_numpy(np.asarray(inputs)).float()
    else:
        x = inputs.permute(0, 3, 1, 2)
    assert transform is not None
    x = transform(x).unsqueeze(0)
    name = model.get_inputs()[0].name
    outs = model.run(None, {name: x.cpu().numpy()})
    score = outs[0][0]
    return list(enumerate(score.tolist()))


# ---- batched device path -------------------------------------------------------------------------------
@dataclass
class StagedVideo:
    """The frames a clip range needs, on their way to (or already on) the engine's device."""
    total: int                      # frames in the whole video
    lo: int
    hi: int                         # clip range [lo, hi)
    f_lo: int                       # index (in even-frame units) of the first staged frame
    hw: Tuple[int, int]
    frames: torch.Tensor            # uint8 [n_even (+1 zero frame on the HIP path), H, W, 3]; 'nv12': [..., 3H/2, W]
    on_device: bool
    ready: Optional[object] = None  # torch.cuda.Event recorded after the H2D copy
    frame_format: str = 'rgb'       # 'nv12': decoder surfaces, converted inside the HIP transforms' taps (hw is the luma size)
    colorimetry: Optional[str] = None   # of 'nv12' frames (transform.COLORIMETRIES)


def clips_per_piece(per_frame_bytes: int) -> int:
    """The most consecutive clips whose staged frames fit ``MAX_STAGE_BYTES`` (read now, at the call): n clips sample 4 n + 4
    even frames and stage a zero frame behind them.  At least 1, whatever the frame size."""
    return max(1, (MAX_STAGE_BYTES // max(1, per_frame_bytes) - CLIP_SPAN // CLIP_STRIDE) // (CLIP_STEP // CLIP_STRIDE))


def even_frame_range(total: int, lo: int, hi: int) -> Tuple[int, int]:
    """[f_lo, f_hi) in even-frame units (source frame // 2) of what clips [lo, hi), lo < hi, sample in a video of ``total``
    frames: only even source frames are ever sampled (starts are multiples of 8, stride 2)."""
    return CLIP_STEP * lo // CLIP_STRIDE, min((CLIP_STEP * (hi - 1) + CLIP_SPAN) // CLIP_STRIDE, (total + 1) // CLIP_STRIDE)


def _stage(dev, total: int, lo: int, hi: int, f_lo: int, hw: Tuple[int, int], even: torch.Tensor,
           stream: Optional[object] = None, frame_format: str = 'rgb', colorimetry: Optional[str] = None) -> StagedVideo:
    """``even`` -- the frames ``even_frame_range`` names for clips [lo, hi) -- and a zero frame behind them, to ``dev``.
    Behind NV12 frames the pad is ``nv12_black`` (behind the other YUV formats ``black_frame``), not zero bytes: the reference
    pads a clip with RGB-zero frames, and only black converts to that (zero bytes are a saturated green)."""
    def fill(pinned: torch.Tensor) -> None:
        pinned[:-1].copy_(even)
        if frame_format == 'nv12':
            pinned[-1].copy_(torch.from_numpy(nv12_black(hw[0], hw[1], colorimetry)))
        elif frame_format != 'rgb':
            pinned[-1].copy_(torch.from_numpy(black_frame(hw[0], hw[1], frame_format, colorimetry)))
        else:
            pinned[-1].zero_()          # the zero frame the padded tail clip reads
    frames, ready = staging.upload((even.shape[0] + 1,) + tuple(even.shape[1:]), fill, dev, stream)
    return StagedVideo(total, lo, hi, f_lo, hw, frames, True, ready, frame_format, colorimetry)


def _rgb_staged(st: StagedVideo) -> StagedVideo:
    """A staged YUV range as host RGB frames (``nv12_to_rgb`` / ``yuv_to_rgb``): what every path that is not a HIP transform
    takes."""
    if st.frame_format == 'rgb':
        return st
    if st.on_device:
        staging.wait_upload(st.frames, st.ready)
    even = (st.frames[:-1] if st.on_device else st.frames).cpu()
    to_rgb = nv12_to_rgb if st.frame_format == 'nv12' else (lambda a, c: yuv_to_rgb(a, st.frame_format, c))
    rgb = torch.from_numpy(to_rgb(even.numpy(), st.colorimetry)) if even.shape[0] else even.new_zeros((0,) + st.hw + (3,))
    return StagedVideo(st.total, st.lo, st.hi, st.f_lo, st.hw, rgb, False)


def stage_video(model, video_thwc_u8: torch.Tensor, clip_range: Optional[Tuple[int, int]] = None,
                stream: Optional[object] = None, frame_format: str = 'rgb', colorimetry: Optional[str] = None) -> StagedVideo:
    """Slice the even frames a clip range samples and, for a TsmEngine, copy them to its GPU through a
    pinned buffer on ``stream`` (so the copy of video i+1 can run under the compute of video i).
    ``frame_format='nv12'``: the video is uint8 [T, 3H/2, W] decoder surfaces (``colorimetry``: default ``'bt601'``), staged
    as they are -- half the bytes of RGB -- with ``nv12_black`` as the pad frame; ``hw`` is the luma size.  A model without a
    device path gets ``nv12_to_rgb`` of the sampled frames on the host, and from there exactly the RGB path.  A
    ``transform.YUV_FORMATS`` name: the same with that format's container per frame, ``black_frame`` and ``yuv_to_rgb``."""
    colorimetry = check_frame_format(frame_format, colorimetry)
    yuv = frame_format != 'rgb'                   # (any YUV format: one 2-d uint8 container per frame)
    if yuv and frame_format != 'nv12':
        video_thwc_u8 = yuv_frame_bytes_view(video_thwc_u8, frame_format)
    if yuv and (video_thwc_u8.dtype != torch.uint8 or video_thwc_u8.dim() != 3):
        what = 'an NV12 video must be uint8 [T, 3H/2, W]' if frame_format == 'nv12' else f'a {frame_format} video must be uint8 [T, rows, bytes]'
        raise ValueError(f'{what}, got {video_thwc_u8.dtype} {tuple(video_thwc_u8.shape)}')
    total = int(video_thwc_u8.shape[0])
    lo, hi = clip_range if clip_range is not None else (0, len(clip_starts(total)))
    hw = frame_hw(video_thwc_u8.shape, frame_format) if yuv else (int(video_thwc_u8.shape[1]), int(video_thwc_u8.shape[2]))
    if hi <= lo:
        return StagedVideo(total, lo, lo, 0, hw, video_thwc_u8[:0], False, None, frame_format, colorimetry)
    f_lo, f_hi = even_frame_range(total, lo, hi)
    even = video_thwc_u8[0::CLIP_STRIDE][f_lo:f_hi]
    if not staging.device_path(model):
        return _rgb_staged(StagedVideo(total, lo, hi, f_lo, hw, even, False, None, frame_format, colorimetry))
    if int(even.numel()) > MAX_STAGE_BYTES:
        # (too large to pin / upload in one piece: hand the (strided, un-copied) host view on;
        #  staged_clip_logits walks the clip range in pieces that fit)
        return StagedVideo(total, lo, hi, f_lo, hw, even, False, None, frame_format, colorimetry)
    return _stage(staging.engine_device(model), total, lo, hi, f_lo, hw, even, stream, frame_format, colorimetry)


def staged_clip_logits(model, st: StagedVideo, transform: Union[TestTransform, PersonCropTransform], batch_clips: int = 32,
                       video_name: Optional[str] = None) -> torch.Tensor:
    """Raw logits [hi - lo, num_class] (CPU float32) of a staged clip range.  Frames are transformed once
    each; clips are gathered from the transformed frames.  A ``PersonCropTransform`` (one box per clip, looked up under
    ``video_name``) transforms per clip instead, behind the windows: ``_person_crop_logits``."""
    if st.hi <= st.lo:
        return torch.empty((0, getattr(model, 'num_class', 0)), dtype=torch.float32)
    person = isinstance(transform, PersonCropTransform)
    if person and video_name is None:
        raise ValueError('a PersonCropTransform looks its boxes up by video: pass video_name')
    if (not st.on_device and staging.device_path(model)
            and isinstance(transform, (TestTransform, PersonCropTransform)) and int(st.frames.numel()) > MAX_STAGE_BYTES):
        # oversized video: pieces of consecutive clips whose even frames fit the staging bound, each staged on its own
        step = clips_per_piece(int(st.frames[0].numel()))
        parts = []
        for a in range(st.lo, st.hi, step):
            b = min(a + step, st.hi)
            f_a, f_b = even_frame_range(st.total, a, b)
            piece = _stage(staging.engine_device(model), st.total, a, b, f_a, st.hw, st.frames[f_a - st.f_lo:f_b - st.f_lo],
                           None, st.frame_format, st.colorimetry)
            parts.append(staged_clip_logits(model, piece, transform, batch_clips, video_name))
        return torch.cat(parts, dim=0)
    if not (st.on_device and hasattr(model, 'packed_layout') and isinstance(transform, (TestTransform, PersonCropTransform))):
        st = _rgb_staged(st)             # (no HIP transform will read these frames: NV12 becomes RGB on the host)
    if person:
        return _person_crop_logits(model, st, transform, batch_clips, video_name)
    frames, idx, hip_transform = _staged_clips(model, st, transform)
    n = int(idx.shape[0])
    out = [_forward_clips(model, _gather(frames, idx, st, b, min(b + batch_clips, n)), hip_transform)
           for b in range(0, n, batch_clips)]
    return torch.cat(out, dim=0).to(torch.float32).cpu()


def _person_crop_logits(model, st: StagedVideo, transform: PersonCropTransform, batch_clips: int, video_name: str) -> torch.Tensor:
    """``staged_clip_logits`` for a per-clip box.  Device-staged frames of a TsmEngine: the range's boxes go up once (a few
    hundred bytes from a pinned int32 tensor), then every batch is ONE ``tsm_preprocess_clips`` launch from the uint8 frames
    straight into the engine's packed input, and the forward -- no transformed intermediate, no gather, no torch kernel.
    Anything else (a session, a stub, no GPU): the torch ``PersonCropTransform`` clip by clip."""
    n = st.hi - st.lo
    dev = staging.engine_device(model)
    if st.on_device and hasattr(model, 'packed_layout'):
        from .engine import preprocess_clips
        staging.wait_upload(st.frames, st.ready)
        boxes = staging.upload_table(transform.box_rows(video_name, st.lo, st.hi), dev)
        frames = st.frames[:-1]           # (the staged zero frame of the centre-crop path: this kernel needs no pad frame)
        out = []
        for a in range(0, n, batch_clips):
            b = min(a + batch_clips, n)
            clips = preprocess_clips(frames, boxes[a:b], st.f_lo, st.total, st.lo + a, b - a, size=transform.size,
                                     scale_255=transform.scale_255, layout=model.packed_layout, n_segment=NUM_SEGMENTS,
                                     clip_step=CLIP_STEP, clip_stride=CLIP_STRIDE, frame_format=st.frame_format,
                                     colorimetry=st.colorimetry)
            out.append(model.forward_device(clips, layout=model.packed_layout))
        return torch.cat(out, dim=0).to(torch.float32).cpu()
    even = st.frames[:-1] if st.on_device else st.frames
    if dev is not None and not even.is_cuda:
        even = even.to(dev, non_blocking=True)
    clips = []
    for c in range(st.lo, st.hi):
        j = [(CLIP_STEP * c + CLIP_STRIDE * k) // CLIP_STRIDE - st.f_lo for k in range(NUM_SEGMENTS)
             if CLIP_STEP * c + CLIP_STRIDE * k < st.total]
        clip = even[j[0]:j[-1] + 1].to(torch.float32)
        if len(j) < NUM_SEGMENTS:        # the zero-padded tail, padded BEFORE the transform as the reference does
            clip = torch.cat([clip, clip.new_zeros((NUM_SEGMENTS - len(j),) + tuple(clip.shape[1:]))])
        clips.append(transform(clip.permute(0, 3, 1, 2), transform.box(video_name, c)))
    out = [_forward_clips(model, torch.stack(clips[a:a + batch_clips]), False) for a in range(0, n, batch_clips)]
    return torch.cat(out, dim=0).to(torch.float32).cpu()


def _staged_clips(model, st: StagedVideo, transform: TestTransform) -> Tuple[torch.Tensor, torch.Tensor, bool]:
    """Transformed frames of a staged clip range (each frame once), the [n_clips, 8] frame indices of its clips as a
    HOST tensor (the zero-padded tail points at one shared zero frame, the last of the buffer), and whether the frames
    are in the engine's packed device format (HIP transform) rather than float32 [n,3,224,224]."""
    dev = staging.engine_device(model)
    hip_transform = st.on_device and isinstance(transform, TestTransform)
    if not hip_transform:
        st = _rgb_staged(st)
    if hip_transform:
        # HIP path: uint8 frames (+ one zero frame for the padded tail) -> fused resize/crop/normalise
        # kernel -> the engine's packed input format, consumed in place.
        from .engine import preprocess_frames
        staging.wait_upload(st.frames, st.ready)
        frames = preprocess_frames(st.frames, resize=transform.size, crop=transform.crop,
                                   scale_255=transform.scale_255, layout=model.packed_layout, frame_format=st.frame_format,
                                   colorimetry=st.colorimetry)
    else:
        even = st.frames[:-1] if st.on_device else st.frames
        if dev is not None and not even.is_cuda:
            even = even.to(dev, non_blocking=True)
        frames = transform(even.permute(0, 3, 1, 2).to(torch.float32))        # [n_even, 3, 224, 224]
        zero = transform(torch.zeros((1, 3) + st.hw, dtype=torch.float32, device=frames.device))
        frames = torch.cat([frames, zero], dim=0)                              # + the zero-padded tail frame
    # frame index of segment k of clip i: (start_i + 2k) / 2 - f_lo, or the shared zero frame past the end of the video:
    # a few hundred integers, kept on the HOST -- on the GPU the windows are cut by tsm_gather_clips from (f_lo, total,
    # first clip) alone (see _gather); only the torch fallback uploads them.
    zi = frames.shape[0] - 1
    src = (CLIP_STEP * np.arange(st.lo, st.hi, dtype=np.int64)[:, None]
           + CLIP_STRIDE * np.arange(NUM_SEGMENTS, dtype=np.int64)[None, :])
    idx = torch.from_numpy(np.where(src < st.total, src // CLIP_STRIDE - st.f_lo, zi).astype(np.int64))
    return frames, idx, hip_transform


def _gather(frames: torch.Tensor, idx: torch.Tensor, st: Optional[StagedVideo], a: int, b: int,
            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Clips ``a .. b`` of a staged range as [b - a, 8, ...one frame] (into ``out`` -- [(b - a) * 8, ...] -- if given).
    Device frames: ``tsm_gather_clips`` cuts the windows from the range's (first frame, total frames, first clip);
    nothing is uploaded and no torch kernel runs (``index_select`` / advanced indexing cost two first-use code-object
    loads, 4 + 150 ms with the GPU idle at the head of a cold job).  Host frames, or no staged range: torch."""
    n = b - a
    if st is not None and frames.is_cuda and frames.is_contiguous() and (frames[0].numel() * frames.element_size()) % 16 == 0:
        from .engine import gather_clips
        got = gather_clips(frames, st.f_lo, st.total, st.lo + a, n, out=out, n_segment=NUM_SEGMENTS, clip_step=CLIP_STEP,
                           clip_stride=CLIP_STRIDE)
        return got.view((n, NUM_SEGMENTS) + tuple(frames.shape[1:]))
    sel = idx[a:b].reshape(-1)
    if frames.is_cuda:
        sel = staging.upload_table(sel, frames.device)
    got = torch.index_select(frames, 0, sel) if out is None else torch.index_select(frames, 0, sel, out=out)
    return got.view((n, NUM_SEGMENTS) + tuple(frames.shape[1:]))


def _forward_clips(model, clips: torch.Tensor, hip_transform: bool) -> torch.Tensor:
    """One batch of gathered clips ([b, 8, 3, 224, 224] float32, or [b, 8, ...packed] on the HIP path) -> logits
    [b, num_class] (a device tensor on the engine paths: no host sync here)."""
    if hip_transform:
        return model.forward_device(clips.contiguous(), layout=model.packed_layout)
    if staging.engine_device(model) is not None and hasattr(model, 'forward_device'):
        return model.forward_device(clips.contiguous())
    return torch.from_numpy(staging.call_host(model, clips))


def video_clip_logits(model, video_thwc_u8: torch.Tensor, transform: Union[TestTransform, PersonCropTransform],
                      clip_range: Optional[Tuple[int, int]] = None, batch_clips: int = 32,
                      video_name: Optional[str] = None, frame_format: str = 'rgb',
                      colorimetry: Optional[str] = None) -> torch.Tensor:
    """Raw logits [n_clips_in_range, num_class] (CPU float32) for the clips ``clip_range`` (default all)
    of one video (``video_name``: the key a ``PersonCropTransform`` looks its boxes up under).  ``frame_format='nv12'``: the
    video is uint8 [T, 3H/2, W] (``stage_video``); the logits equal those of ``nv12_to_rgb(video)`` bit for bit."""
    st = stage_video(model, video_thwc_u8, clip_range, None, frame_format, colorimetry)
    return staged_clip_logits(model, st, transform, batch_clips, video_name)


def prefetch_staged(model, videos: Iterable[Tuple[object, torch.Tensor]],
                    clip_range_of: Optional[Callable[[torch.Tensor], Optional[Tuple[int, int]]]] = None,
                    frame_format: str = 'rgb', colorimetry: Optional[str] = None) -> Iterator[Tuple[object, StagedVideo]]:
    """Double buffering over a stream of ``(key, uint8 video)``: while the caller computes on video i, a
    worker thread reads / slices / pins video i+1 and copies it to the GPU on a side stream."""
    side = torch.cuda.Stream(staging.engine_device(model)) if staging.device_path(model) else None

    def work(item):
        key, vid = item
        vid = vid() if callable(vid) else vid          # lazy readers run on the worker thread too
        rng = clip_range_of(vid) if clip_range_of is not None else None
        return key, stage_video(model, vid, rng, side, frame_format, colorimetry)

    it = iter(videos)
    with ThreadPoolExecutor(max_workers=1) as pool:
        try:
            fut = pool.submit(work, next(it))
        except StopIteration:
            return
        while fut is not None:
            cur = fut.result()
            try:
                fut = pool.submit(work, next(it))
            except StopIteration:
                fut = None
            yield cur


class prefetch_pieces:
    """Iterator of ``(key, staged piece, is the video's last piece)`` over a stream of ``(key, uint8 video or reader)``:
    one worker thread, started here, reads each video once and stages it in pieces of ``piece_clips`` consecutive clips
    (fewer if the frames are so large that a piece would pass ``MAX_STAGE_BYTES``), up to ``depth`` pieces ahead of the
    caller.  Against whole videos: the first kernel of a job starts after one piece (a few ms of pinning and copying
    instead of the whole first video: 0.14 s, which every rank of a multi-GPU job pays on a job N times shorter), the
    page-locked buffers and the device blocks have ONE size for the whole job (no re-pinning when a longer video
    arrives), and the device footprint is a piece, not a video.  ``close()`` (also at exhaustion) sends the worker
    home even if it is blocked on the full queue."""

    def __init__(self, model, videos: Iterable[Tuple[object, torch.Tensor]], piece_clips: int = PIECE_CLIPS,
                 depth: int = 3):
        self._model, self._videos, self._piece = model, videos, int(piece_clips)
        self._side = torch.cuda.Stream(staging.engine_device(model)) if staging.device_path(model) else None
        self._out: 'queue.Queue' = queue.Queue(maxsize=max(1, int(depth)))
        self._stop = threading.Event()
        self._worker = threading.Thread(target=self._produce, name='tsm-stage', daemon=True)
        self._worker.start()       # (now, not at the first next(): the caller's own setup overlaps the first piece)

    def _put(self, x) -> bool:
        while not self._stop.is_set():
            try:
                self._out.put(x, timeout=0.05)
                return True
            except queue.Full:
                pass
        return False

    def _produce(self) -> None:
        try:
            for key, vid in self._videos:
                vid = vid() if callable(vid) else vid
                n = len(clip_starts(int(vid.shape[0])))
                step = max(1, min(self._piece, clips_per_piece(int(vid[0].numel()) if n else 1)))
                if n == 0 and not self._put((key, stage_video(self._model, vid, (0, 0), self._side), True)):
                    return
                for a in range(0, n, step):
                    b = min(a + step, n)
                    if not self._put((key, stage_video(self._model, vid, (a, b), self._side), b == n)):
                        return
            self._put(None)
        except BaseException as e:      # surfaces in the caller
            self._put(e)

    def __iter__(self):
        return self

    def __next__(self) -> Tuple[object, StagedVideo, bool]:
        if self._stop.is_set():
            raise StopIteration
        item = self._out.get()
        if item is None or isinstance(item, BaseException):
            self.close()
            if item is None:
                raise StopIteration
            raise item
        return item

    def close(self) -> None:
        self._stop.set()
        self._worker.join(timeout=5.0)


def _rank_clip_range(total_frames: int) -> Optional[Tuple[int, int]]:
    """This rank's contiguous block of the video's clips (None = all of them, single process)."""
    rank, world = tdist.world_info()
    if world == 1:
        return None
    return tdist.shard_range(len(clip_starts(total_frames)), world, rank)


def _gather_video_logits(model, local: torch.Tensor, total_frames: int) -> torch.Tensor:
    """All-gather the per-rank blocks of one video's clip logits (no-op in a single process)."""
    rank, world = tdist.world_info()
    if not tdist.collective_enabled():
        return local
    n = len(clip_starts(total_frames))
    lo, hi = tdist.shard_range(n, world, rank)
    num_class = getattr(model, 'num_class', local.shape[1] if local.numel() else 0)
    local = local.reshape(hi - lo, num_class)
    return tdist.all_gather_host(local, staging.engine_device(model), n_total=n)


def scores_dict(logits: torch.Tensor, total_frames: int) -> Dict[int, Dict[int, float]]:
    """``scores[first_frame_index] = {class_id: float(score)}`` (:416)."""
    starts = clip_starts(total_frames)
    assert logits.shape[0] == len(starts)
    rows = logits.tolist()
    return {s: {c: float(v) for c, v in enumerate(row)} for s, row in zip(starts, rows)}


def _write_score_json(out_dir: str, item, checkpoint: str, logits: torch.Tensor, n_frames: int) -> None:
    res_dict = dict(video_name=item.video_name, model='video_model', input_shape=[1, 8, 3, 224, 224],
                    checkpoint=checkpoint, total_frames=n_frames, ground_truth=item.reps, action=item.class_)
    res_dict['scores'] = scores_dict(logits, n_frames)
    out_path = os.path.join(out_dir, f'{item.video_name}.score.json')
    with open(out_path, 'w') as f:
        json.dump(res_dict, f)
    print(f'{item.video_name} result saved to {out_path}')


def _inference_dataset_by_videos(model, items: list, out_dir: str, checkpoint: str, transform, reader,
                                 batch_clips: int, frame_format: str = 'rgb', colorimetry: Optional[str] = None) -> None:
    """``shard='videos'``: rank r decodes and runs videos r, r+W, r+2W, ... whole (no video is decoded twice);
    per round of W videos the ranks exchange [frame count, clip count] and then the padded logits (two small
    all-gathers), and rank 0 writes the round's JSON files."""
    rank, world = tdist.world_info()
    dev = staging.engine_device(model)
    num_class = getattr(model, 'num_class', None)
    mine = items[rank::world]
    staged = prefetch_staged(model, ((it, (lambda p=it.video_path: reader(p))) for it in mine), None, frame_format, colorimetry)
    for r0 in range(0, len(items), world):
        try:
            item, st = next(staged) if r0 + rank < len(items) else (None, None)
        except StopIteration:            # cannot happen: `mine` has one entry per round this rank takes part in
            item, st = None, None
        if st is not None:
            local = staged_clip_logits(model, st, transform, batch_clips, item.video_name)
            meta = torch.tensor([st.total, local.shape[0], local.shape[1]], dtype=torch.int64)
        else:
            local = torch.empty((0, num_class or 0), dtype=torch.float32)
            meta = torch.zeros(3, dtype=torch.int64)
        if not tdist.collective_enabled():
            _write_score_json(out_dir, item, checkpoint, local, st.total)
            continue
        metas = tdist.all_gather_host(meta.reshape(1, 3), dev)
        per, ncls = int(metas[:, 1].max()), int(metas[:, 2].max())
        every = tdist.gather_padded_host(local.reshape(local.shape[0], ncls), per, dev)
        if rank == 0:
            for r in range(min(world, len(items) - r0)):
                _write_score_json(out_dir, items[r0 + r], checkpoint, every[r, :int(metas[r, 1])], int(metas[r, 0]))


def estimated_clips(item, frame_counter: Optional[Callable[[str], int]] = None) -> int:
    """Clip count of a video WITHOUT decoding it, for the shard plan only (the real frame count comes from the decoded
    video): ``frame_counter(path)`` if given, the rawframes count of the annotation helper, the header of a ``.npy``
    frame file, else the last annotated repetition frame (a lower bound)."""
    frames = -1
    if frame_counter is not None:
        frames = int(frame_counter(item.video_path))
    elif getattr(item, 'total_frames', -1) > 0:
        frames = int(item.total_frames)
    elif item.video_path.endswith('.npy') and os.path.exists(item.video_path):
        frames = int(np.load(item.video_path, mmap_mode='r').shape[0])
    if frames <= 0:
        frames = max([int(r) for r in item.reps] + [CLIP_STEP])
    return len(clip_starts(frames))


class _ClipBatcher:
    """Full ``batch_clips`` batches across video boundaries: clips of consecutive videos are gathered into one
    persistent batch buffer and forwarded whenever it is full (the ragged remainder once, at the end), and every
    logits row goes back to the video it came from.  Clips are independent units (the temporal shift never leaves a
    clip) and the engine's results do not depend on the batch a clip rides in, so this is bit-identical to per-video
    batches.  The buffer is reused batch after batch: gather and forward are ordered on one stream."""

    def __init__(self, model, batch_clips: int):
        self.model, self.batch = model, int(batch_clips)
        self.buf: Optional[torch.Tensor] = None                   # [batch * 8, ...one frame]
        self.hip: Optional[bool] = None
        self.queue: List[Tuple[int, int]] = []                    # (video key, clips) of the rows in the buffer
        self.queued = 0
        self.rows: Dict[int, List[torch.Tensor]] = {}

    def add(self, key: int, frames: torch.Tensor, idx: torch.Tensor, hip_transform: bool,
            st: Optional[StagedVideo] = None) -> None:
        """Queue every clip of a staged range: ``frames`` / ``idx`` / ``hip_transform`` as ``_staged_clips`` returns
        them, ``st`` the range itself (lets device frames be cut by the HIP gather; None: torch ``index_select``)."""
        self.rows.setdefault(key, [])
        if self.buf is None:
            self.buf = torch.empty((self.batch * NUM_SEGMENTS,) + tuple(frames.shape[1:]), dtype=frames.dtype, device=frames.device)
            self.hip = hip_transform
        assert hip_transform == self.hip and frames.shape[1:] == self.buf.shape[1:] and frames.dtype == self.buf.dtype, \
            'one job, one frame format'
        pos, n = 0, int(idx.shape[0])
        while pos < n:
            take = min(self.batch - self.queued, n - pos)
            _gather(frames, idx, st, pos, pos + take,
                    out=self.buf[self.queued * NUM_SEGMENTS:(self.queued + take) * NUM_SEGMENTS])
            self.queue.append((key, take))
            self.queued += take
            pos += take
            if self.queued == self.batch:
                self.flush()

    def flush(self) -> None:
        if not self.queue:
            return
        clips = self.buf[:self.queued * NUM_SEGMENTS].view((self.queued, NUM_SEGMENTS) + tuple(self.buf.shape[1:]))
        out = _forward_clips(self.model, clips, bool(self.hip))
        pos = 0
        for key, n in self.queue:
            self.rows[key].append(out[pos:pos + n])
            pos += n
        self.queue, self.queued = [], 0

    def complete(self, key: int) -> bool:
        """Every clip of video ``key`` handed to ``add`` so far has been forwarded."""
        return key in self.rows and all(k != key for k, _ in self.queue)

    def parts(self, key: int) -> List[torch.Tensor]:
        """The logits rows of video ``key``, in clip order, as the slices of the batches they rode in."""
        return self.rows.pop(key)

    def logits(self, key: int) -> torch.Tensor:
        parts = self.rows.pop(key)
        return torch.cat(parts, dim=0) if parts else torch.empty((0, getattr(self.model, 'num_class', 0)))


class _ScoreWriter:
    """Score files of finished videos, written WHILE the GPU works on the batches behind them: a finished video's logits
    go to page-locked host memory with an asynchronous copy, and its JSON file is encoded once the event behind that copy
    has completed -- polled between batches, never waited for before the end of the job.  (Encoding the whole dataset
    after the last forward was a serial 0.5 s of the 6-s RepCount-val job; a writer THREAD fights the launch loop for the
    interpreter lock.)  ``drain`` returns the host logits of every video in submission order."""

    def __init__(self, out_dir: str, checkpoint: str, expected_rows: int, num_class: Optional[int] = None,
                 pin: bool = False):
        self.out_dir, self.checkpoint, self.expected = out_dir, checkpoint, max(64, int(expected_rows))
        # one pinned block for the rank's rows (grown by whole blocks if the plan undercounted); with a known class count
        # it is pinned NOW, while the first piece is still being staged, not between two forwards
        self.host: Optional[torch.Tensor] = (torch.empty((self.expected, int(num_class)), dtype=torch.float32, pin_memory=True)
                                             if pin and num_class else None)
        self.used = 0
        self.pending: Deque = deque()                 # (item, host rows, frames, event)
        self.done: List[torch.Tensor] = []

    def _rows(self, n: int, ncls: int, pin: bool) -> torch.Tensor:
        if n == 0:
            return torch.empty((0, ncls), dtype=torch.float32)
        if self.host is None or self.used + n > self.host.shape[0] or self.host.shape[1] != ncls:
            self.host = torch.empty((max(n, self.expected), ncls), dtype=torch.float32, pin_memory=pin)
            self.used = 0
        out = self.host[self.used:self.used + n]
        self.used += n
        return out

    def submit(self, item, parts: Sequence[torch.Tensor], n_frames: int) -> None:
        """``parts``: the video's rows as [n_i, classes] slices in clip order (no concatenation on the device: each slice is
        one small asynchronous copy into its place in the host block)."""
        parts = [p.to(torch.float32) for p in parts if p.shape[0]]
        n = sum(int(p.shape[0]) for p in parts)
        ncls = int(parts[0].shape[1]) if parts else 0
        cuda = any(p.is_cuda for p in parts)
        host = self._rows(n, ncls, cuda)
        pos = 0
        for p in parts:
            host[pos:pos + p.shape[0]].copy_(p, non_blocking=True)
            pos += int(p.shape[0])
        ev = None
        if cuda:
            ev = torch.cuda.Event()
            ev.record()
        self.pending.append((item, host, n_frames, ev))
        self.poll()

    def poll(self, wait: bool = False) -> None:
        while self.pending:
            item, host, n_frames, ev = self.pending[0]
            if ev is not None:
                if wait:
                    ev.synchronize()
                elif not ev.query():
                    return
            self.pending.popleft()
            _write_score_json(self.out_dir, item, self.checkpoint, host, n_frames)
            self.done.append(host)

    def drain(self) -> List[torch.Tensor]:
        self.poll(wait=True)
        return self.done


def _inference_dataset_global(model, items: list, out_dir: str, checkpoint: str, transform, reader, batch_clips: int,
                              frame_counter: Optional[Callable[[str], int]] = None) -> Dict[str, torch.Tensor]:
    """``shard='global'``: the (video, clip) index of the whole job is laid out once -- whole videos, longest first,
    each to the least-loaded rank (``distributed.plan_video_shards``) -- every rank then decodes and runs ITS videos
    with full cross-video batches and NO collective inside the loop, and the job ends with one exchange: an
    all-gather of the per-video [index, frames, clips] table and ONE padded all-gather of the per-clip logits
    ``[clips_on_rank, num_class]`` (returned per video on every rank).  Each rank writes the JSON files of its own videos
    while its GPU works on the videos behind them -- ``out_dir`` must therefore be ONE directory all ranks see (the ranks
    of one node always do; a multi-node job needs a shared file system, or ``shard='clips'`` / ``'videos'``, whose files
    are all written by rank 0).

    Failure behaviour: the plan is computed by every rank from its own view of the dataset, so the ranks compare a
    checksum of it BEFORE any work (a rank that sees other frame counts fails the job in its first second, on every
    rank, instead of after the last video); and a rank whose loop raises still enters the final exchange, with an error
    marker in the video table, so that the others raise too instead of blocking in an all-gather that never completes."""
    rank, world = tdist.world_info()
    dev = staging.engine_device(model)
    plan_failure: Optional[BaseException] = None
    counts: List[int] = []
    owner: List[int] = []
    try:
        counts = [estimated_clips(it, frame_counter) for it in items]
        owner = tdist.plan_video_shards(counts, world)
    except Exception as exc:       # (a frame_counter that raises on ONE rank): the others are about to enter the checksum exchange
        if not tdist.collective_enabled():
            raise
        plan_failure = exc
    if tdist.collective_enabled():
        import zlib
        # [checksum of the plan, videos, status]: the status word carries a planning failure into the first exchange, so that
        # no rank is left blocked in it
        sig = torch.tensor([[zlib.crc32(repr((owner, counts)).encode()), len(items), 0 if plan_failure is None else 1]],
                           dtype=torch.int64)
        sigs = tdist.all_gather_host(sig, dev)
        failed = [r for r in range(world) if int(sigs[r, 2]) != 0]
        if failed:
            if plan_failure is not None:
                raise plan_failure
            raise RuntimeError(f'rank(s) {failed} failed while planning the dataset job; nothing was run (rank {rank})')
        if not bool((sigs == sigs[0]).all()):
            raise RuntimeError(f'shard plan differs between ranks (checksum, videos) = {sigs[:, :2].tolist()}: every rank must '
                               f'see the same dataset and frame counts (rank {rank})')
    mine = [v for v in range(len(items)) if owner[v] == rank]

    def make_pieces():
        # (the stager's worker starts on the first video here, before the warm-up below)
        return prefetch_pieces(model, ((v, (lambda p=items[v].video_path: reader(p))) for v in mine))

    def warm() -> None:
        if dev is not None and hasattr(model, 'warmup') and mine:
            # Cold-job costs out of the loop: the kernels of the two batch sizes this rank will run -- full
            # batches and the ragged last one -- are tuned (tsm_tune: the engine's own zeroed buffer, no torch kernel) or
            # read from the tune cache NOW, while the stager's worker reads, pins and uploads the first pieces; without
            # this the first batch and the last batch of every cold job each stopped for a tuning pass mid-loop.
            my_clips = sum(counts[v] for v in mine)
            tail = my_clips % batch_clips
            model.warmup(sorted({b for b in (min(batch_clips, my_clips), tail) if b > 0}))

    # (the stager's start and the warm-up run INSIDE _run_global's failure bracket: a tsm_tune HIP error or an OOM in either
    #  still reaches the other ranks through the status row of the final exchange)
    return _run_global(model, items, mine, counts, make_pieces, warm, out_dir, checkpoint, transform, batch_clips, dev, rank, world)


def _run_global(model, items: list, mine: List[int], counts: List[int], make_pieces, warm, out_dir: str, checkpoint: str,
                transform, batch_clips: int, dev, rank: int, world: int) -> Dict[str, torch.Tensor]:
    """The stager's start, the warm-up, the loop, the score files and the final exchange of ``_inference_dataset_global``."""
    # rows of MY videos: [video index, frames, clips, classes]; the last row is this rank's status word (0 = loop completed)
    meta = torch.full((len(items) + 1, 4), -1, dtype=torch.int64)
    slot_of = {v: i for i, v in enumerate(mine)}
    whole = 0                                                      # videos of ``mine`` whose last piece has been queued
    handed = 0                                                     # ... already with the writer (in order)

    def hand_over(final: bool) -> None:
        # every rank writes the files of ITS videos (a node's ranks share the file system), each as soon as its last clip
        # has been forwarded and its rows have reached the host -- under the GPU work of the videos behind it
        nonlocal handed
        while handed < whole and (final or batcher.complete(mine[handed])):
            writer.submit(items[mine[handed]], batcher.parts(mine[handed]), int(meta[handed, 1]))
            handed += 1
        writer.poll()

    failure: Optional[BaseException] = None
    per_video: List[torch.Tensor] = []
    pieces = None
    batcher = writer = None
    try:
        pieces = make_pieces()
        warm()
        batcher = _ClipBatcher(model, batch_clips)
        writer = _ScoreWriter(out_dir, checkpoint, sum(counts[v] for v in mine) + 8 * len(mine),
                              getattr(model, 'num_class', None), pin=dev is not None)
        for v, st, last in pieces:
            slot = slot_of[v]
            done = max(0, int(meta[slot, 2]))
            meta[slot, :3] = torch.tensor([v, st.total, done + st.hi - st.lo])
            if st.hi > st.lo:
                batcher.add(v, *_staged_clips(model, st, transform), st=st)
            else:
                batcher.rows.setdefault(v, [])
            if last:
                whole = slot + 1
            hand_over(False)
        batcher.flush()
        hand_over(True)
        per_video = writer.drain()                                 # host rows of my videos, in ``mine`` order
    except Exception as exc:                                       # (reader error, tuning error, OOM, ...): still take part in the exchange below
        if not tdist.collective_enabled():
            raise
        failure = exc
    finally:
        if pieces is not None:
            pieces.close()       # (a failure anywhere above must not leave the stager blocked on its full queue)
    num_class = getattr(model, 'num_class', None) or (int(per_video[0].shape[1]) if per_video else 0)
    local = (torch.cat([t.reshape(-1, num_class) for t in per_video], dim=0) if per_video and failure is None
             else torch.empty((0, num_class), dtype=torch.float32))
    if not tdist.collective_enabled():
        out, pos = {}, 0
        for slot, v in enumerate(mine):
            n = int(meta[slot, 2])
            out[items[v].video_name] = local[pos:pos + n]
            pos += n
        return out
    meta[:len(mine), 3] = num_class      # (a rank without videos does not know the class count: it rides in the table)
    meta[-1] = torch.tensor([0 if failure is None else 1, 0, 0, 0])
    metas = tdist.all_gather_host(meta, dev).reshape(world, len(items) + 1, 4)
    failed = [r for r in range(world) if int(metas[r, -1, 0]) != 0]
    if failed:       # every rank sees the same table: all of them stop here, none is left waiting in the logits all-gather
        if failure is not None:
            raise failure
        raise RuntimeError(f'rank(s) {failed} failed in their share of the dataset job; no logits were exchanged (rank {rank})')
    metas = metas[:, :-1]
    per = max(1, int(metas[:, :, 2].clamp(min=0).sum(dim=1).max()))
    ncls = max(num_class, int(metas[:, :, 3].max()))
    every = tdist.gather_padded_host(local.reshape(local.shape[0], ncls), per, dev)
    # the exchange leaves every rank with the whole job's per-clip logits in dataset order (what the serial rep counter of
    # utils/eval.py needs); the score files are already on disk
    where = {}
    for r in range(world):
        pos = 0
        for v, frames, n, _c in metas[r].tolist():
            if v >= 0:
                where[v] = (r, pos, n, frames)
                pos += n
    assert sorted(where) == list(range(len(items))), 'every video must come back from exactly one rank'
    return {items[v].video_name: every[where[v][0], where[v][1]:where[v][1] + where[v][2]] for v in range(len(items))}


def inference_dataset(model, splits: List[str], out_dir: str, checkpoint: str, person_crop: bool = False,
                      data_root: Optional[str] = None, anno_path: Optional[str] = None,
                      video_reader: Optional[Callable[[str], torch.Tensor]] = None, action: Sequence[str] = ('all',),
                      batch_clips: int = 32, scale_255: bool = False, shard: Optional[str] = None,
                      frame_counter: Optional[Callable[[str], int]] = None, boxes=None, frame_format: str = 'rgb',
                      colorimetry: Optional[str] = None) -> Optional[Dict[str, torch.Tensor]]:
    """Inference the RepCount dataset; one ``{video_name}.score.json`` per video with the reference's
    schema: video_name, model, input_shape, checkpoint, total_frames, ground_truth, action, scores.

    ``shard='global'`` (the default: the dataset-throughput form, SURVEY 8e "global clip index over a batch of videos
    ... gather once per many videos") assigns whole videos to ranks by clip count, longest first, runs full
    cross-video batches with no collective inside the loop, writes every score file under the GPU work of the videos
    behind it and, under ``torch.distributed``, exchanges once at the end (``frame_counter(path) -> frames`` feeds the
    plan when neither rawframes nor ``.npy`` headers can; without it the annotation's last repetition frame does);
    ``shard='clips'`` is the reference's loop shape, one video at a time, and under ``torch.distributed`` splits the
    clips of every video over the ranks (one all-gather per video: lowest latency for ONE stream, but every rank reads
    every video); ``shard='videos'`` is the round-2 form, whole videos round-robin with an exchange per round of W
    videos (each round lasts as long as its longest video).  All three write identical files.

    ``person_crop=True`` is the reference's PersonCrop -> Resize((224, 224)) -> Normalize with the boxes given by the caller:
    ``boxes`` is a callable ``(video_name, clip_index) -> (top, left, h, w) or None`` or a mapping ``video_name -> boxes``
    (``transform.PersonCropTransform``; the detector is out of scope).  It runs under ``shard='clips'`` (the default then)
    or ``'videos'``; ``'global'`` is refused: its batcher shares transformed frames between overlapping clips.

    ``frame_format='nv12'`` (``colorimetry``: default ``'bt601'``): ``video_reader`` returns uint8 [T, 3H/2, W] decoder
    surfaces, staged as they are and converted inside the HIP transforms (``stage_video``).  It runs under ``shard='clips'``
    (the default then) or ``'videos'``; ``'global'`` is not implemented: its stager sizes and cuts pieces as RGB frames."""
    need_clip_rows(model, 'inference_dataset')
    colorimetry = check_frame_format(frame_format, colorimetry)
    rank, _world = tdist.world_info()
    if shard is None:
        shard = 'clips' if person_crop or frame_format != 'rgb' else 'global'
    if frame_format != 'rgb' and shard == 'global':
        raise NotImplementedError(f"frame_format={frame_format!r} runs with shard='clips' or 'videos'; shard='global' takes RGB frames only")
    if shard not in ('clips', 'videos', 'global'):
        raise ValueError("shard must be 'clips', 'videos' or 'global'")
    if person_crop and shard == 'global':
        raise ValueError("person_crop=True runs with shard='clips' or 'videos': the global batcher transforms every frame once "
                         "and shares it between overlapping clips, and a person box is per clip")
    transform = build_test_transform(person_crop=person_crop, scale_255=scale_255, boxes=boxes)
    os.makedirs(out_dir, exist_ok=True)       # (every rank: with shard='global' each writes the files of its own videos)
    data_root = osp.expanduser(data_root or '~/data/RepCount/')
    helper = RepcountHelper(data_root, anno_path or osp.join(data_root, 'annotation.csv'))
    data = helper.get_rep_data(splits, action=list(action))
    reader = video_reader or read_video
    if rank == 0:
        print('==> transform:', transform)
    if shard == 'videos':
        _inference_dataset_by_videos(model, list(data.values()), out_dir, checkpoint, transform, reader, batch_clips,
                                     frame_format, colorimetry)
        return
    if shard == 'global':     # (returns {video_name: logits [clips, classes]} on every rank; the reference returns None)
        return _inference_dataset_global(model, list(data.values()), out_dir, checkpoint, transform, reader, batch_clips,
                                         frame_counter)
    # Video i+1 is read, sliced, pinned and copied to the GPU by a worker thread while video i computes.
    videos = ((item, (lambda p=item.video_path: reader(p))) for item in data.values())
    for item, staged in prefetch_staged(model, videos, lambda v: _rank_clip_range(int(v.shape[0])), frame_format, colorimetry):
        n_frames = staged.total
        logits = _gather_video_logits(model, staged_clip_logits(model, staged, transform, batch_clips, item.video_name),
                                      n_frames)
        if rank == 0:
            _write_score_json(out_dir, item, checkpoint, logits, n_frames)


def save_scores_to_json(scores: Sequence[Sequence[float]], output_path: str, video_path: str, step: int) -> None:
    """``{video_path, scores: {clip_index*step: {class: score}}}``; refuses to overwrite (:47-67)."""
    if not output_path.endswith('.json'):
        output_path += '.json'
    assert not os.path.exists(output_path), f'{output_path} already exists'
    d = dict(video_path=video_path, scores={i * step: {c: float(v) for c, v in enumerate(row)}
                                            for i, row in enumerate(scores)})
    with open(output_path, 'w') as f:
        json.dump(d, f)


# ---- streaming counter ---------------------------------------------------------------------------------
def count_by_video_model(model, frames: Iterable[Union[np.ndarray, torch.Tensor]],
                         ground_truth: Optional[list] = None, threshold: float = 0.5, softmax: bool = True,
                         transform: Optional[Callable] = None, step: int = CLIP_STEP,
                         on_window: Optional[Callable[[int, int, int], None]] = None) -> Tuple[int, List[int]]:
    """Online counting over a frame source (HWC uint8, RGB): every 8 queued frames form one window
    (non-overlapping, stride 8), the window's state is pushed into an incremental counter.
    ``on_window(window_index, state, count)`` is called after each window."""
    need_clip_rows(model, 'count_by_video_model')
    transform = transform or build_test_transform(False)
    queue: Deque[torch.Tensor] = deque(maxlen=NUM_SEGMENTS)
    counter = RepCounter(step)
    widx = 0
    for frame in frames:
        queue.append(torch.as_tensor(np.asarray(frame) if not isinstance(frame, torch.Tensor) else frame))
        if len(queue) == NUM_SEGMENTS:
            clip = torch.stack(list(queue)).to(torch.float32)                 # [8,H,W,3], 0..255
            scores = [s for _, s in inference_video(model, clip, transform=transform)]
            state = scores_to_preds([scores], threshold=threshold, softmax=softmax)[0]
            counter.push(state)
            if on_window is not None:
                on_window(widx, state, counter.count)
            widx += 1
            queue.clear()
    if ground_truth is not None:
        gt = len(ground_truth) // 2
        print(f'count={counter.count}, gt_count={gt}, correct={abs(gt - counter.count) <= 1}')
    return counter.count, list(counter.reps)


# ---- the image-model path ------------------------------------------------------------------------------
def _image_geometry(model) -> Tuple[int, int]:
    """(resize, crop) of the model's ``data_transform``: what ``create_image_model`` recorded, else the reference's 256 / 224."""
    return int(getattr(model, 'image_resize', 256)), int(getattr(model, 'image_crop', 224))


def _image_logits_device(model, frames_u8: torch.Tensor) -> torch.Tensor:
    """Engine path of one batch: pinned staging, ONE ``tsm_preprocess_image`` launch into the engine's packed layout, the
    forward; returns the CUDA logits [n, num_class] (nothing synchronised)."""
    from .engine import preprocess_image
    need_clip_rows(model, 'inference_images')
    dev = staging.engine_device(model)
    resize, crop = _image_geometry(model)
    need_frame_engine(model, crop, 'image', 'create_image_model')
    staged = (frames_u8.contiguous() if frames_u8.is_cuda
              else staging.upload(frames_u8.shape, lambda pinned: pinned.copy_(frames_u8), dev)[0])
    x = preprocess_image(staged, resize, crop, out_layout=model.packed_layout)
    n = x.shape[0]
    return model.forward_device(x.view((n, 1) + tuple(x.shape[1:])), layout=model.packed_layout)


def _image_scores_host(model, frames_u8: torch.Tensor, transform: ImageTransform) -> np.ndarray:
    """Non-engine models: the CPU ``ImageTransform``, then a torch module (``model(x[n,3,H,W])``) or an onnxruntime-style
    session (one ``run`` per frame on [1,3,H,W], as the reference feeds it)."""
    return staging.call_host(model, transform(frames_u8), one_per_run=True)


def inference_images(model, frames_u8) -> np.ndarray:
    """The batched form of ``inference_image``: uint8 frames [n,H,W,3] (ndarray or tensor) -> float32 scores [n, num_class].
    A ``TsmEngine`` (``engine.create_image_model``) stages the frames, does ONE ``tsm_preprocess_image`` launch and the
    forward (``max_frames`` frames per engine call); any other model takes the CPU ``ImageTransform``.  The channel order is
    kept as given: the reference hands cv2's BGR frames to its transform as they are -- the caller's business."""
    frames = as_frames_u8(frames_u8)
    if staging.device_path(model):
        return _image_logits_device(model, frames).cpu().numpy()
    resize, crop = _image_geometry(model)
    return _image_scores_host(model, frames, ImageTransform(resize, crop))


def inference_image(model, frame: np.ndarray) -> np.ndarray:
    """One frame (H, W, 3) uint8 through the image model -> scores [num_class] float32 (utils/inference_count.py:168-189)."""
    f = frame if isinstance(frame, torch.Tensor) else np.asarray(frame)
    return inference_images(model, f[None])[0].astype(np.float32)


def _frame_batches(frames, batch: int) -> Iterator[torch.Tensor]:
    """uint8 [<= batch, H, W, 3] pieces of a [N,H,W,3] array / tensor or of an iterable of HWC frames."""
    if (isinstance(frames, torch.Tensor) or isinstance(frames, np.ndarray)) and frames.ndim == 4:
        for a in range(0, int(frames.shape[0]), batch):
            yield as_frames_u8(frames[a:a + batch])
        return
    held: List[torch.Tensor] = []
    for f in frames:
        held.append(torch.as_tensor(np.asarray(f) if not isinstance(f, torch.Tensor) else f))
        if len(held) == batch:
            yield as_frames_u8(torch.stack(held))
            held = []
    if held:
        yield as_frames_u8(torch.stack(held))


def image_states(model, frames, batch_frames: Optional[int] = None,
                 return_scores: bool = False) -> Tuple[List[int], Optional[np.ndarray]]:
    """The voted per-frame states (0 / 1) of a video under the image model, and its scores [N, num_class] when asked for:
    the loop of ``count_by_image_model`` without the count.  A ``TsmEngine`` works in batches of ``batch_frames`` (default:
    its ``max_clips``): pinned staging, one ``tsm_preprocess_image`` launch, the forward, one ``tsm_frame_votes`` launch with
    the history of the last 6 arg-maxes carried on the device; states -- and scores -- cross PCIe once, at the end.  Any other
    model takes the CPU ``ImageTransform`` and the host vote (``counting.vote_states``)."""
    engine = staging.device_path(model)
    batch = int(batch_frames or (getattr(model, 'max_clips', 32) if engine else 32))
    if batch <= 0:
        raise ValueError(f'batch_frames must be positive, got {batch_frames}')
    scores: List = []
    if engine:
        from .engine import frame_votes
        states_dev: List[torch.Tensor] = []
        history = None
        for piece in _frame_batches(frames, batch):
            logits = _image_logits_device(model, piece)
            _pred, state, history = frame_votes(logits, history)
            states_dev.append(state)
            if return_scores:
                scores.append(logits)
        states = torch.cat(states_dev).cpu().tolist() if states_dev else []
        rows = torch.cat(scores).cpu().numpy() if scores else None
    else:
        transform = ImageTransform(*_image_geometry(model))
        states, hist = [], []
        for piece in _frame_batches(frames, batch):
            s = _image_scores_host(model, piece, transform)
            st, hist = vote_states(s.argmax(axis=1).tolist(), hist)
            states += st
            scores.append(s)
        rows = np.concatenate(scores) if scores and return_scores else None
    return states, rows


def count_by_image_model(model, frames: Iterable[Union[np.ndarray, torch.Tensor]], ground_truth: Optional[list] = None,
                         pred_out_path: Optional[str] = None, threshold: float = 0.1,
                         batch_frames: Optional[int] = None) -> Tuple[int, List[int]]:
    """Repetition count of a video with the per-frame image model (utils/inference_count.py:192-243): every frame's scores,
    a vote over the arg-max of the last 7 frames (``sum(que) >= 4``: over class ids, as the reference sums them), then
    ``pred_to_count(states, step=7)``.  Returns ``(count, reps)``.

    frames: an iterable of HWC uint8 frames or a [N,H,W,3] array / tensor, as ``count_by_video_model`` takes them (no cv2
    here; the channel order is kept as given -- the reference reads BGR with cv2 and never converts).
    The per-batch work is ``image_states``': on a ``TsmEngine`` everything up to the states stays on the GPU and crosses PCIe
    once, at the end -- and so do the scores, when ``pred_out_path`` is given (``save_scores_to_json(scores, path, '',
    step=1)``).  ``threshold`` is accepted and unused, as in the reference (:197,:208).  ``video_out_path`` /
    ``write_to_video`` is out of scope."""
    states, rows = image_states(model, frames, batch_frames, return_scores=bool(pred_out_path))
    count, reps = pred_to_count(states, step=7)
    if ground_truth is not None:
        gt = len(ground_truth) // 2
        print(f'count={count} gt_count={gt} correct={abs(count - gt) <= 1}')
    if pred_out_path:
        save_scores_to_json([] if rows is None else rows.tolist(), pred_out_path, '', step=1)
    return count, reps
