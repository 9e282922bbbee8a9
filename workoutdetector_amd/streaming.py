"""Online repetition counting for many concurrent frame streams on one engine.

Counterpart of the reference's streaming consumers of the video model -- ``count_by_video_model``
(workoutdetector/utils/inference_count.py:285-339: a ``deque(maxlen=8)``, one inference per 8 queued
frames, ``input_queue.clear()``) and the WebSocket loop of ``app/inference.py:87-111`` / ``app/server.py:85-100``
(one client = one stream, 8 frames per window) -- re-shaped for the GPU: every stream only queues frames;
``StreamBatcher.step()`` collects the windows that are complete across ALL streams and pushes them through the
engine as ONE batch (fused HIP transform + ``tsm_forward``), then feeds each stream's incremental counter.
The reference runs one blocking batch-1 ``session.run`` per client window.

``person_crop=True`` is the reference's accuracy option (``build_test_transform(person_crop=True)``, datasets/build.py:123-129)
on streams: ``push(..., box=)`` carries the detector's first box of a frame, a window is cropped to the union of its frames'
boxes (``transform.person_box``).  The detector and any tracker stay the caller's.

``ImageStreamBatcher`` is the same for the per-frame image model (``count_by_image_model``, utils/inference_count.py:192-243):
every frame of every stream, of any mix of sizes, through ONE ``tsm_preprocess_windows`` launch in image mode per batch; the
vote over the last 7 frames and the counter per stream on the host.

No transport here (the WebSocket/HTTP front is outside the hot path): a server
calls ``push`` from its receive loop and ``step`` on a timer or whenever ``ready()`` is large enough.
"""
from __future__ import annotations

from collections import deque
from dataclasses import dataclass, field
from typing import Callable, Deque, Dict, Hashable, List, Optional, Tuple

import numpy as np
import torch

from . import staging
from .counting import VOTE_WINDOW, RepCounter, scores_to_state_list, vote_states
from .inference_count import NUM_SEGMENTS, need_clip_rows
from .transform import (IMAGE_WINDOW_FORMATS, Box, ImageTransform, PersonCropTransform, TestTransform, build_test_transform,
                        check_frame_format, image_tables, image_window_descriptors, person_box, pushed_frame, window_descriptors,
                        yuv_luma_hw)


@dataclass
class StreamState:
    counter: RepCounter
    frames: List[np.ndarray] = field(default_factory=list)        # frames of the window being filled (host path)
    windows: Deque[object] = field(default_factory=deque)         # complete [8,H,W,3] uint8 windows not yet run
    crops: Deque[Optional[Box]] = field(default_factory=deque)    # one per entry of `windows`: its person box, None = whole frame
    boxes: List[Tuple[float, ...]] = field(default_factory=list)  # detector boxes pushed with the frames of the window being filled
    states: List[int] = field(default_factory=list)               # one state per processed window
    frames_seen: int = 0
    cur: Optional[torch.Tensor] = None                            # HIP path: page-locked window being filled
    n_cur: int = 0


class StreamBatcher:
    """``push(stream_id, frame)`` HWC uint8 RGB frames; ``step()`` runs every complete 8-frame window of every
    stream in batches of at most ``max_batch`` and returns ``{stream_id: [(window_index, state, count), ...]}``.

    Windows are non-overlapping with stride 8 like the reference's streaming loop; ``softmax``/``threshold``
    follow utils/eval.py:153-164; frame sizes may differ between streams (a batch of mixed sizes is still ONE transform
    launch, ``tsm_preprocess_windows``, in batch order at 224x224).  A model that is no ``TsmEngine`` on a GPU takes the host
    path -- the torch transform and ``staging.call_host``: an onnxruntime-style session, a torch module or a plain callable on
    ``[B, 8, 3, H, W]``.

    ``person_crop=True``: ``push(stream_id, frame, box=(x1, y1, x2, y2))`` takes the detector's first box of that frame; a
    complete window is cropped to ``transform.person_box`` of the boxes pushed with its frames and resized to the crop size
    without keeping the aspect ratio; a window none of whose frames came with a box is "no person": the whole frame.

    ``frame_format='nv12'`` (``colorimetry``: ``transform.COLORIMETRIES``, default ``'bt601'``): ``push`` takes decoder
    surfaces, uint8 [3H/2, W] of any mix of even sizes; boxes are in luma pixels.  A batch is still ONE launch, and one launch
    has one pixel code, so the format belongs to the batcher, not to the frame.  The windows are staged as they are (half the
    bytes of RGB, in the pinned budget too) and converted inside the transform's taps: states and counts equal those of an RGB
    batcher fed ``nv12_to_rgb`` of the frames.  On the host path the frames are converted when they arrive.  A
    ``transform.YUV_FORMATS`` name (``'i420'``, ``'yv12'``, ``'p010'``, ``'yuyv'``, ``'uyvy'``): the same with that format's
    uint8 container per frame (a 16-bit ``'p010'`` frame is taken as its bytes) and ``yuv_to_rgb`` as the conversion."""

    def __init__(self, model, threshold: float = 0.5, softmax: bool = True, step: int = 8, max_batch: int = 32,
                 transform: Optional[TestTransform] = None,
                 on_window: Optional[Callable[[Hashable, int, int, int], None]] = None,
                 max_pinned_bytes: int = 1 << 30, max_free_per_shape: int = 64, person_crop: bool = False,
                 frame_format: str = 'rgb', colorimetry: Optional[str] = None):
        self.colorimetry = check_frame_format(frame_format, colorimetry)
        self.frame_format = frame_format
        need_clip_rows(model, 'StreamBatcher')
        self.model = model
        self.threshold, self.softmax, self.step_frames = threshold, softmax, step
        self.max_batch = max_batch
        self.transform = transform or build_test_transform(False)
        self.on_window = on_window
        self.person_crop = bool(person_crop)
        # (host path: the torch person-crop transform at this transform's output size; its box comes with each call)
        self._crop_transform = PersonCropTransform({}, size=self.transform.crop, scale_255=self.transform.scale_255)
        self.streams: Dict[Hashable, StreamState] = {}
        # HIP path: every frame is copied into a page-locked [8,H,W,3] window buffer when it ARRIVES (push), so that a
        # complete window is one DMA away from the GPU when step() runs -- the 1.8-MB host gather of a 360x206 window
        # (~0.15 ms) leaves the window's critical path.  Buffers are recycled once their H2D copy has completed.
        self._dev = staging.engine_device(model) if staging.device_path(model) else None
        # Page-locked memory is bounded: at most ``max_pinned_bytes`` in window buffers (a producer that runs ahead of
        # step(), or many resolutions, falls back to pageable windows beyond it -- slower upload, no hipHostMalloc on
        # the frame-arrival path, no unbounded pinning), at most ``max_free_per_shape`` idle buffers per frame size.
        self._free: Dict[Tuple[int, ...], List[torch.Tensor]] = {}
        self._inflight: List[Tuple[object, torch.Tensor]] = []
        self.max_pinned_bytes, self.max_free_per_shape = int(max_pinned_bytes), int(max_free_per_shape)
        self.pinned_bytes = 0

    # ---- ingest -------------------------------------------------------------------------------------------
    def open(self, stream_id: Hashable) -> StreamState:
        if stream_id not in self.streams:
            self.streams[stream_id] = StreamState(RepCounter(self.step_frames))
        return self.streams[stream_id]

    def push(self, stream_id: Hashable, frame, box=None) -> None:
        if box is not None:
            if not self.person_crop:
                raise ValueError('a box needs StreamBatcher(person_crop=True)')
            box = tuple(float(v) for v in np.asarray(box, dtype=np.float64).reshape(-1))
            if len(box) != 4 or not all(np.isfinite(box)):
                raise ValueError(f'box must be four finite numbers (x1, y1, x2, y2), got {box}')
        st = self.open(stream_id)
        arr, _hw = pushed_frame(frame, self.frame_format, self.colorimetry, to_rgb=self._dev is None)
        st.frames_seen += 1
        if self._dev is not None:
            if st.cur is None:
                st.cur, st.n_cur = self._take_window(tuple(arr.shape)), 0
            elif tuple(st.cur.shape[1:]) != tuple(arr.shape):
                raise ValueError('frame size changed inside a window')
            if box is not None:
                st.boxes.append(box)
            st.cur[st.n_cur].copy_(torch.from_numpy(np.ascontiguousarray(arr)))
            st.n_cur += 1
            if st.n_cur == NUM_SEGMENTS:
                buf, st.cur = st.cur, None      # input_queue.clear() of the reference
                self._complete(st, buf)
            return
        if st.frames and st.frames[0].shape != arr.shape:
            raise ValueError('frame size changed inside a window')
        if box is not None:
            st.boxes.append(box)
        st.frames.append(arr)
        if len(st.frames) == NUM_SEGMENTS:
            frames, st.frames = st.frames, []   # input_queue.clear() of the reference
            self._complete(st, np.stack(frames))

    def _complete(self, st: StreamState, window) -> None:
        """Queue a complete window with its crop box: ``person_box`` over the boxes that came with its frames (the union,
        enlarged by 10 %; datasets/transform.py:247-259), None -- the whole frame -- when none came or the union is empty.
        A union that the enlargement leaves with a side of 0 pixels raises ValueError as ``person_box`` does (the reference
        fails inside Resize there); that window is dropped."""
        boxes, st.boxes = st.boxes, []
        try:
            crop = person_box(boxes) if boxes else None
        except ValueError:
            if isinstance(window, torch.Tensor):
                self._give_back(window)
            raise
        st.windows.append(window)
        st.crops.append(crop)

    def _recycle(self, wait: bool = False) -> None:
        """Window buffers whose upload has finished go back to the free lists (capped per shape; the surplus and every
        pageable fallback buffer is simply dropped)."""
        still = []
        for ev, buf in self._inflight:
            if wait:
                ev.synchronize()
            if ev.query():
                self._give_back(buf)
            else:
                still.append((ev, buf))
        self._inflight = still

    def _give_back(self, buf: torch.Tensor) -> None:
        """An idle window buffer returns to its shape's free list while that list is below ``max_free_per_shape``; beyond
        the cap (and for pageable fallback buffers) it is dropped and its page-locked bytes leave the budget."""
        if not buf.is_pinned():
            return
        free = self._free.setdefault(tuple(buf.shape[1:]), [])
        if len(free) < self.max_free_per_shape:
            free.append(buf)
        else:
            self.pinned_bytes -= buf.numel()

    def _take_window(self, frame_shape: Tuple[int, ...]) -> torch.Tensor:
        """A uint8 [8,H,W,3] window buffer: a recycled page-locked one if one of this size is free, a newly pinned one
        while the pinned budget lasts, else pageable memory."""
        self._recycle()
        free = self._free.get(frame_shape)
        if free:
            return free.pop()
        nbytes = NUM_SEGMENTS * int(np.prod(frame_shape))
        if self.pinned_bytes + nbytes > self.max_pinned_bytes:
            self._trim_free(keep=frame_shape)           # idle buffers of other resolutions give their budget back first
        if self.pinned_bytes + nbytes > self.max_pinned_bytes:
            return torch.empty((NUM_SEGMENTS,) + frame_shape, dtype=torch.uint8)
        self.pinned_bytes += nbytes
        return torch.empty((NUM_SEGMENTS,) + frame_shape, dtype=torch.uint8, pin_memory=True)

    def _trim_free(self, keep: Optional[Tuple[int, ...]] = None) -> None:
        """Release the idle page-locked buffers of every frame size no open stream is filling (except ``keep``)."""
        live = {tuple(s.cur.shape[1:]) for s in self.streams.values() if s.cur is not None}
        for shape in list(self._free):
            if shape != keep and shape not in live:
                self.pinned_bytes -= sum(b.numel() for b in self._free.pop(shape))

    def ready(self) -> int:
        return sum(len(s.windows) for s in self.streams.values())

    def close(self, stream_id: Hashable) -> Tuple[int, List[int]]:
        """Drop a stream (an incomplete last window is discarded, like the reference) -> (count, reps)."""
        st = self.streams.pop(stream_id)
        for buf in ([st.cur] if st.cur is not None else []) + [w for w in st.windows if isinstance(w, torch.Tensor)]:
            self._give_back(buf)                             # half-filled / never-run windows: the same capped path as _recycle
        self._trim_free()
        return st.counter.count, list(st.counter.reps)

    def result(self, stream_id: Hashable) -> Tuple[int, List[int]]:
        st = self.streams[stream_id]
        return st.counter.count, list(st.counter.reps)

    # ---- compute ------------------------------------------------------------------------------------------
    def _logits(self, windows: List[object], crops: List[Optional[Box]]):
        """[n,8,H,W,3] uint8 windows (possibly of different sizes) and their person boxes -> raw logits [n, num_class]: a CUDA
        tensor that is still being computed on the HIP path (the caller syncs once per step), an ndarray on the duck-typed
        CPU path."""
        dev = self._dev
        tf = self.transform
        if dev is not None:
            from .engine import preprocess_windows
            # every window into ONE device arena (they are already page-locked, filled at push time: one DMA each, each start
            # 16-byte aligned), one small descriptor table, ONE transform launch in batch order for any mix of frame sizes
            offsets, total = [], 0
            for w in windows:
                offsets.append(total)
                total += (w.numel() + 15) // 16 * 16
            arena = torch.empty((total,), dtype=torch.uint8, device=dev)
            for w, off in zip(windows, offsets):
                arena[off:off + w.numel()].copy_(w.view(-1), non_blocking=True)
            done = torch.cuda.Event()
            done.record()
            self._inflight += [(done, w) for w in windows]
            yuv = self.frame_format != 'rgb'
            table = window_descriptors([yuv_luma_hw(w.shape, self.frame_format) if yuv else tuple(w.shape[1:]) for w in windows], offsets,
                                       crops if self.person_crop else None, resize=tf.size, crop=tf.crop, frame_format=self.frame_format)
            clips = preprocess_windows(arena, staging.upload_table(torch.from_numpy(table), dev), len(windows), NUM_SEGMENTS,
                                       person_crop=self.person_crop, resize=tf.size, crop=tf.crop, scale_255=tf.scale_255,
                                       layout=self.model.packed_layout, frame_format=self.frame_format, colorimetry=self.colorimetry)
            return self.model.forward_device(clips, layout=self.model.packed_layout)
        if self.person_crop:
            xs = [self._crop_transform(torch.from_numpy(w).permute(0, 3, 1, 2).float(), box) for w, box in zip(windows, crops)]
        else:
            xs = [tf(torch.from_numpy(w).permute(0, 3, 1, 2).float()) for w in windows]
        return staging.call_host(self.model, torch.stack(xs))

    def step(self) -> Dict[Hashable, List[Tuple[int, int, int]]]:
        """Run all complete windows (oldest first, round-robin over streams) and update the counters."""
        out: Dict[Hashable, List[Tuple[int, int, int]]] = {}
        order: List[Hashable] = []
        pending = []
        while self.ready():
            batch: List[Tuple[Hashable, object, Optional[Box]]] = []
            progressed = True
            while len(batch) < self.max_batch and progressed:   # round-robin keeps per-stream order and fairness
                progressed = False
                for sid, st in self.streams.items():
                    if st.windows and len(batch) < self.max_batch:
                        batch.append((sid, st.windows.popleft(), st.crops.popleft()))
                        progressed = True
            # enqueue only: the host gathers / pins batch i+1 while the GPU still computes batch i
            pending.append(self._logits([w for _, w, _ in batch], [c for _, _, c in batch]))
            order += [sid for sid, _, _ in batch]
        if pending:
            # HIP path: softmax / arg-max / threshold on the GPU too (tsm_scores_to_states): one int32 per window crosses PCIe,
            # in the step's only host sync
            hip = isinstance(pending[0], torch.Tensor)
            states = scores_to_state_list(torch.cat(pending) if hip else np.concatenate(pending), self.threshold, self.softmax)
            if hip:
                self._recycle()     # that .cpu() was the step's sync: every upload queued before it has completed
            for sid, state in zip(order, states):
                st = self.streams[sid]
                widx = len(st.states)
                st.states.append(state)
                count = st.counter.push(state)
                out.setdefault(sid, []).append((widx, state, count))
                if self.on_window is not None:
                    self.on_window(sid, widx, state, count)
        return out


# ---- the image model on streams --------------------------------------------------------------------------------------------
@dataclass
class ImageStreamState:
    counter: RepCounter
    history: List[int] = field(default_factory=list)      # arg-max of the stream's last <= 6 processed frames (the vote's deque)
    states: List[int] = field(default_factory=list)       # one voted state per processed frame
    frames_seen: int = 0
    queued: int = 0                                       # frames pushed and not yet run


class _ImageChunk:
    """The frames of one future batch, in arrival order: on the engine path one byte arena (frames, and the coefficient
    block of every geometry the chunk holds, each start 16-byte aligned) that is ONE upload away from the GPU; on the host
    path the frames themselves."""

    def __init__(self):
        self.sids: List[Hashable] = []
        self.shapes: List[Tuple[int, int]] = []
        self.offsets: List[int] = []
        self.tables: Dict[Tuple[int, int], int] = {}
        self.buf: Optional[torch.Tensor] = None
        self.used = 0
        self.frames: List[np.ndarray] = []


class ImageStreamBatcher:
    """Online counting with the per-frame IMAGE model (the reference's default ``--model-type``; ``count_by_image_model``,
    utils/inference_count.py:192-243) for many concurrent streams on one engine.  ``push(stream_id, frame)`` queues an HWC
    uint8 frame -- every frame is a window of its own, so the size may change between the frames of a stream; ``step()`` runs
    every queued frame of every stream, in arrival order, in batches of at most ``max_batch`` (default: the engine's
    ``max_clips``) and returns ``{stream_id: [(frame_index, state, count), ...]}``; ``on_frame(stream_id, frame_index, state,
    count)`` is called per frame.  ``result`` / ``close`` give ``(count, reps)``.

    On a ``TsmEngine`` built by ``create_image_model`` a batch is: the frames and the coefficient tables of their geometries,
    copied into a page-locked arena as the frames arrive; ONE upload (the descriptor table rides at the arena's end); ONE
    ``tsm_preprocess_windows`` launch in image mode for any mix of sizes, into the engine's packed layout; the forward; one
    ``tsm_scores_to_states`` launch (no softmax, threshold -inf: the first arg-max, ``tsm_frame_votes``' tie rule); 4 bytes
    per frame back, once per step.  The vote -- ``counting.vote_states`` over a 6-deep history per stream -- and the
    incremental ``RepCounter(7)`` stay on the host: a handful of integers per frame.  For any interleaving of ``push`` and
    ``step`` a stream's states equal ``image_states(model, its frames)[0]`` and ``close`` equals ``count_by_image_model``.

    ``frame_format='nv12'`` (``colorimetry``: ``transform.COLORIMETRIES``, default ``'bt601'``): ``push`` takes decoder
    surfaces, uint8 [3H/2, W] with H and W even, staged as they are and converted inside the launch: states and counts equal
    those of an RGB batcher fed ``nv12_to_rgb`` of the frames.  Any other model (a stub, a torch module, an
    onnxruntime-style session) takes the host path: ``ImageTransform`` and the scoring of ``inference_images``, the same vote
    and counters; NV12 frames are converted when they arrive.

    Page-locked memory is bounded by ``max_pinned_bytes``: beyond it an arena is pageable (a slower upload, nothing else)."""

    def __init__(self, model, max_batch: Optional[int] = None, frame_format: str = 'rgb', colorimetry: Optional[str] = None,
                 on_frame: Optional[Callable[[Hashable, int, int, int], None]] = None, max_pinned_bytes: int = 1 << 30):
        if frame_format not in IMAGE_WINDOW_FORMATS:
            raise NotImplementedError(f'ImageStreamBatcher takes frame_format in {IMAGE_WINDOW_FORMATS} (Pillow\'s resample is 8-bit RGB), '
                                      f'got {frame_format!r}')
        self.colorimetry = check_frame_format(frame_format, colorimetry)
        self.frame_format = frame_format
        if getattr(model, 'tdn_depths', None):
            raise NotImplementedError('ImageStreamBatcher runs the per-frame image model; a TDN engine takes five frames per segment: '
                                      'use TdnStreamBatcher')
        if getattr(model, 'num_segments', 1) != 1:
            raise ValueError(f'ImageStreamBatcher needs an engine with num_segments=1 (engine.create_image_model), got '
                             f'{model.num_segments}: use StreamBatcher for the video model')
        need_clip_rows(model, 'ImageStreamBatcher')           # (consensus_type='identity')
        self.model = model
        self.resize, self.crop = int(getattr(model, 'image_resize', 256)), int(getattr(model, 'image_crop', 224))
        self._dev = staging.engine_device(model) if staging.device_path(model) else None
        if self._dev is not None and (model.height, model.width) != (self.crop, self.crop):
            raise ValueError(f'the engine takes {model.height} x {model.width} frames, the transform crops to {self.crop}')
        self.max_batch = int(max_batch if max_batch is not None else (getattr(model, 'max_clips', 32) if self._dev is not None else 32))
        if self.max_batch <= 0:
            raise ValueError(f'max_batch must be positive, got {max_batch}')
        self.on_frame = on_frame
        self.transform = ImageTransform(self.resize, self.crop)
        self.streams: Dict[Hashable, ImageStreamState] = {}
        self._chunks: Deque[_ImageChunk] = deque()
        self.max_pinned_bytes, self.pinned_bytes = int(max_pinned_bytes), 0
        self._free: List[torch.Tensor] = []                           # idle page-locked arenas
        self._inflight: List[Tuple[object, torch.Tensor]] = []        # (event behind the upload, arena)
        self._carry: Dict[Hashable, List[Tuple[int, int, int]]] = {}

    # ---- ingest -------------------------------------------------------------------------------------------
    def open(self, stream_id: Hashable) -> ImageStreamState:
        if stream_id not in self.streams:
            self.streams[stream_id] = ImageStreamState(RepCounter(VOTE_WINDOW))
        return self.streams[stream_id]

    def push(self, stream_id: Hashable, frame) -> None:
        arr, (h, w) = pushed_frame(frame, self.frame_format, self.colorimetry, to_rgb=self._dev is None)
        if 0 in (h, w):                                       # (an RGB frame: an NV12 one was refused above)
            raise ValueError(f'frame must be uint8 [H,W,3], got {arr.dtype} {arr.shape}')
        # the refusals of a window, before anything is queued: a side beyond 65535, a crop larger than the resized frame
        image_window_descriptors([(h, w)], [0], [0], self.resize, self.crop, self.frame_format)
        tables = image_tables(h, w, self.resize, self.crop) if self._dev is not None else None
        st = self.open(stream_id)
        if not self._chunks or len(self._chunks[-1].sids) >= self.max_batch:
            self._chunks.append(_ImageChunk())
        ch = self._chunks[-1]
        if self._dev is not None:
            if (h, w) not in ch.tables:
                ch.tables[(h, w)] = self._append(ch, tables.view(np.uint8)) if tables.size else 0
            ch.offsets.append(self._append(ch, arr.reshape(-1)))
        else:
            ch.frames.append(np.ascontiguousarray(arr))
        ch.sids.append(stream_id)
        ch.shapes.append((h, w))
        st.frames_seen += 1
        st.queued += 1

    def _append(self, ch: _ImageChunk, data: np.ndarray) -> int:
        """Copy ``data`` (uint8, flat) to the chunk's arena at the next 16-byte boundary; returns its byte offset."""
        off, n = ch.used, int(data.size)
        end = off + (n + 15) // 16 * 16
        if ch.buf is None or end > ch.buf.numel():
            old = ch.buf
            ch.buf = self._take(max(end, 2 * (old.numel() if old is not None else 0)))
            if old is not None:
                ch.buf[:off].copy_(old[:off])
                self._give_back(old)
        ch.buf.numpy()[off:off + n] = data
        ch.used = end
        return off

    def _take(self, nbytes: int) -> torch.Tensor:
        """An arena of at least ``nbytes``: an idle page-locked one that is large enough, a newly pinned one while the budget
        lasts (idle ones give their bytes back first), else pageable memory."""
        self._recycle()
        fit = [b for b in self._free if b.numel() >= nbytes]
        if fit:
            buf = min(fit, key=lambda b: b.numel())
            self._free = [b for b in self._free if b is not buf]
            return buf
        nbytes = max(nbytes, 1 << 20)
        if self.pinned_bytes + nbytes > self.max_pinned_bytes:
            self.pinned_bytes -= sum(b.numel() for b in self._free)
            self._free = []
        if self.pinned_bytes + nbytes > self.max_pinned_bytes:
            return torch.empty(nbytes, dtype=torch.uint8)
        self.pinned_bytes += nbytes
        return torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)

    def _give_back(self, buf: Optional[torch.Tensor]) -> None:
        if buf is not None and buf.is_pinned():
            self._free.append(buf)

    def _recycle(self) -> None:
        still = []
        for ev, buf in self._inflight:
            if ev.query():
                self._give_back(buf)
            else:
                still.append((ev, buf))
        self._inflight = still

    def ready(self) -> int:
        return sum(len(ch.sids) for ch in self._chunks)

    def result(self, stream_id: Hashable) -> Tuple[int, List[int]]:
        st = self.streams[stream_id]
        return st.counter.count, list(st.counter.reps)

    def close(self, stream_id: Hashable) -> Tuple[int, List[int]]:
        """Run what is still queued (a frame counts once it was pushed: ``count_by_image_model`` drops none; the other streams'
        rows of that step are returned by the next ``step()``), then drop the stream -> (count, reps)."""
        if self.streams[stream_id].queued:
            rest = self.step()
            rest.pop(stream_id, None)
            self._carry = rest                                # (the other streams' rows of that step: the next step() returns them)
        st = self.streams.pop(stream_id)
        if not self.streams:
            self.pinned_bytes -= sum(b.numel() for b in self._free)
            self._free = []
        return st.counter.count, list(st.counter.reps)

    # ---- compute ------------------------------------------------------------------------------------------
    def _preds_device(self, ch: _ImageChunk) -> torch.Tensor:
        """One batch on the engine: int32 CUDA [n], the first arg-max of every frame's logits (still being computed)."""
        from .engine import preprocess_image_windows, scores_to_states
        n = len(ch.sids)
        desc = image_window_descriptors(ch.shapes, ch.offsets, [ch.tables[s] for s in ch.shapes], self.resize, self.crop, self.frame_format)
        doff = self._append(ch, desc.reshape(-1).view(np.uint8))
        arena = ch.buf[:ch.used].to(self._dev, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        self._inflight.append((done, ch.buf))
        table = arena[doff:doff + n * 32].view(torch.int32).view(n, 8)
        x = preprocess_image_windows(arena, table, n, 1, resize=self.resize, crop=self.crop, out_layout=self.model.packed_layout,
                                     frame_format=self.frame_format, colorimetry=self.colorimetry)
        logits = self.model.forward_device(x, layout=self.model.packed_layout)
        return scores_to_states(logits, threshold=float('-inf'), softmax=False)

    def _preds_host(self, ch: _ImageChunk) -> List[int]:
        x = torch.cat([self.transform(f) for f in ch.frames])
        return staging.call_host(self.model, x, one_per_run=True).argmax(axis=1).tolist()

    def step(self) -> Dict[Hashable, List[Tuple[int, int, int]]]:
        """Run every queued frame (arrival order: a stream's frames stay in order) and update the votes and the counters."""
        out, self._carry = self._carry, {}
        order: List[Hashable] = []
        pending = []
        while self._chunks:
            ch = self._chunks.popleft()
            # enqueue only: the next batch's upload and launches queue up behind this one's
            pending.append(self._preds_device(ch) if self._dev is not None else self._preds_host(ch))
            order += ch.sids
        if not pending:
            return out
        if self._dev is not None:
            preds = torch.cat(pending).cpu().tolist()       # the step's only sync: 4 bytes per frame
            self._recycle()
        else:
            preds = [p for piece in pending for p in piece]
        for sid, pred in zip(order, preds):
            st = self.streams[sid]
            # (-1 is tsm_scores_to_states' answer to a NaN first logit, where the first arg-max is class 0)
            (state,), st.history = vote_states([max(int(pred), 0)], st.history)
            idx = len(st.states)
            st.states.append(state)
            st.queued -= 1
            count = st.counter.push(state)
            out.setdefault(sid, []).append((idx, state, count))
            if self.on_frame is not None:
                self.on_frame(sid, idx, state, count)
        return out
