"""Counting and accuracy pipelines for a TDN engine (``create_tdn_model``), beside ``inference_count`` and ``classification``,
which build clips of ONE frame per segment and keep refusing it.

A TDN clip is T segments of five consecutive frames.  Nothing here assembles ``[B, T, 5, 3, H, W]`` on the device path: every
staged frame is transformed ONCE (``preprocess_frames(packed=False)`` -> a pool ``[n, 3, H, W]``) and the engine's first kernel
finds its frames in the pool itself (``TsmEngine.forward_pool``, include/tsm_hip.h: TSM_LAYOUT_TDN_POOL):

* counting (``tdn_video_clip_logits``, ``tdn_count_video``): clips start every ``step`` = 8 frames and sample every 2nd frame, so
  segment k of clip c has centre ``8 c + 2 k`` and reads frames ``centre - 2 .. centre + 2`` clamped to the video; a segment whose
  centre is past the end reads the transformed zero frame five times (the reference's zero-padded tail: its differences are zero).
  WINDOW mode: the kernel computes the frame numbers from five integers, a step of the loop uploads nothing.
* accuracy (``tdn_eval_classification``): per labelled segment ``T x 5`` frames at ``tdn_sample_indices + start_index``; TABLE
  mode: an int32 table of pool frame numbers per directory piece.
* streams (``TdnStreamBatcher``) and ``reuse_segments=True``: everything in front of ``fuse2`` is computed per segment, and segment
  k of clip c is segment k - 4 of clip c + 1.  The per-segment part runs once per unique segment into a ring of feature slots
  (``TsmEngine.tdn_segments``) and the trunk finds its T segments there (``TsmEngine.forward_ring``); a live stream keeps the ring
  between steps.  ``TdnSegmentRing`` is the host bookkeeping of both.  The same bits as the whole forward.

Out of scope: YUV input, person crop and ``shard='global'``."""
from __future__ import annotations

from collections import deque
from typing import Callable, Deque, Dict, Hashable, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from . import inference_count as ic
from . import staging
from .classification import FrameReader, default_eval_transform, evaluate, read_frames
from .counting import RepCounter, pred_to_count, scores_to_state_list
from .transform import PersonCropTransform, TestTransform, pushed_frame

TDN_FRAMES = 5


# ---- frame numbers -------------------------------------------------------------------------------------------------------
def tdn_clip_indices(total: int, lo: int, hi: int, num_segments: int = 8, step: int = 8, stride: int = 2,
                     first_source_frame: int = 0, pad: int = -1, n_frames: Optional[int] = None) -> np.ndarray:
    """int32 ``[hi - lo, T, 5]``: the window rule of ``forward_pool`` (csrc/tsm_host_util.h: tdn_window_frame) in NumPy -- it
    calls no C, so that it can check the C function.  Segment k of clip c has centre ``step * c + stride * k``; frame j is
    ``clamp(centre - 2 + j, 0, total - 1) - first_source_frame``; a segment whose centre is ``>= total`` holds ``pad`` five
    times, and so does any entry outside ``[0, n_frames)`` when ``n_frames`` is given."""
    total, lo, hi = int(total), int(lo), int(hi)
    if total <= 0 or hi < lo or lo < 0 or step <= 0 or stride <= 0:
        raise ValueError(f'need total > 0, 0 <= lo <= hi and positive step / stride, got {total}, {lo}, {hi}, {step}, {stride}')
    centre = (step * np.arange(lo, hi, dtype=np.int64)[:, None] + stride * np.arange(num_segments, dtype=np.int64)[None, :])[:, :, None]
    src = np.clip(centre - 2 + np.arange(TDN_FRAMES, dtype=np.int64), 0, total - 1) - int(first_source_frame)
    out = np.where(centre < total, src, pad)
    if n_frames is not None:
        out = np.where((out >= 0) & (out < int(n_frames)), out, pad)
    return out.astype(np.int32)


def tdn_sample_indices(total: int, num_segments: int = 8, num_frames: int = 5, rng: Optional[np.random.RandomState] = None) -> np.ndarray:
    """int64 ``[T]``: the first of the ``num_frames`` consecutive frames of every segment, zero-based, of a video of ``total``
    frames.  With an ``np.random.RandomState`` this is the reference's ``TDNDataset.sample_indices`` to the integer (all three
    branches, its draws in its order; it raises numpy's ValueError where the reference's ``randint`` does).  With ``rng=None``
    the deterministic midpoints: ``k * d + d // 2`` where the reference adds ``randint(d)``;
    ``floor((k + 0.5) * (total - 4) / T)`` where it sorts random draws; zeros where it returns zeros.

    The reference then reads frames ``i .. i + 4`` whatever ``total`` is -- files that do not exist when a segment starts within
    four frames of the end.  ``tdn_sample_frames`` clamps frame numbers past the last frame to it."""
    n, T = int(total), int(num_segments)
    # (the reference's two arms of every choice differ only when num_frames != 5: `- 5 + 1` against `- num_frames + 1`)
    span = n - 5 + 1 if n - num_frames + 1 < T else n - num_frames + 1
    d = span // T
    if d > 0:
        draw = rng.randint(d, size=T) if rng is not None else np.full(T, d // 2)
        offsets = np.arange(T) * d + draw
    elif n > T:
        if rng is not None:
            offsets = np.sort(rng.randint(span, size=T))
        else:
            offsets = np.maximum(np.floor((np.arange(T) + 0.5) * span / T), 0)
    else:
        offsets = np.zeros((T,))
    return np.array(offsets).astype(np.int64)


def tdn_sample_frames(total: int, num_segments: int = 8, num_frames: int = 5, rng: Optional[np.random.RandomState] = None) -> np.ndarray:
    """int64 ``[T, num_frames]``: zero-based frame numbers ``tdn_sample_indices[k] + j``, those past the last frame clamped to
    it (the reference would read files that do not exist)."""
    if int(total) < 1:
        raise ValueError(f'a segment needs at least one frame, got total_frames = {total}')
    start = tdn_sample_indices(total, num_segments, num_frames, rng)
    return np.minimum(start[:, None] + np.arange(num_frames, dtype=np.int64)[None, :], int(total) - 1)


# ---- refusals, all before the library loads ------------------------------------------------------------------------------------
def _need_tdn_rows(model, transform, where: str, frame_format: str = 'rgb') -> None:
    if frame_format != 'rgb':
        raise NotImplementedError(f"{where} takes RGB uint8 frames only (frame_format={frame_format!r}): convert on the host")
    if isinstance(transform, PersonCropTransform):
        raise NotImplementedError(f'{where}: person crop is not implemented for TDN clips')
    if not isinstance(transform, TestTransform):
        raise ValueError(f'{where} needs a TestTransform, got {type(transform).__name__}')
    consensus = getattr(model, 'consensus_type', 'avg')
    if consensus != 'avg':
        raise ValueError(f"{where} needs one row of scores per clip: the model was built with consensus_type={consensus!r}; "
                         "build it with consensus_type='avg'")
    h, w = getattr(model, 'height', None), getattr(model, 'width', None)
    if h is not None and w is not None:
        if int(h) != int(w):
            raise ValueError(f'{where} crops squares: the engine is {h} x {w}')
        if int(transform.crop) != int(h):
            raise ValueError(f'{where}: the transform crops {transform.crop} pixels, the engine takes {h}')


def _stage_pool(fill, n: int, frame_shape, zero_last: bool, tf: TestTransform, dev, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """How frames reach an engine here: ``fill(pinned)`` writes ``n`` uint8 frames of ``frame_shape`` (with ``zero_last`` a frame of
    zeros rides behind them, as frame ``n``), ``staging.upload``, ONE ``preprocess_frames(packed=False)`` launch -> the pool."""
    from .engine import preprocess_frames

    def fill_all(pinned: torch.Tensor) -> None:
        fill(pinned[:n])
        if zero_last:
            pinned[n].zero_()
    staged, _ready = staging.upload((n + int(zero_last),) + tuple(frame_shape), fill_all, dev)
    return preprocess_frames(staged, resize=tf.size, crop=tf.crop, scale_255=tf.scale_255, packed=False, out=out)


# ---- counting --------------------------------------------------------------------------------------------------------------------
def tdn_frame_range(total: int, lo: int, hi: int, step: int = ic.CLIP_STEP, stride: int = ic.CLIP_STRIDE,
                    num_segments: int = ic.NUM_SEGMENTS) -> Tuple[int, int]:
    """Source frames ``[a, b)`` that clips ``[lo, hi)``, lo < hi, read: ``[step lo - 2, step (hi - 1) + stride (T - 1) + 3)``
    clipped to the video (``[8 lo - 2, 8 (hi - 1) + 17)`` for the counting geometry)."""
    return max(0, step * lo - 2), min(int(total), step * (hi - 1) + stride * (num_segments - 1) + 3)


def tdn_clips_per_piece(per_frame_bytes: int, step: int = ic.CLIP_STEP, stride: int = ic.CLIP_STRIDE,
                        num_segments: int = ic.NUM_SEGMENTS) -> int:
    """The most consecutive clips of one staged piece: their uint8 frames and the zero frame fit
    ``inference_count.MAX_STAGE_BYTES`` (read now, at the call), and -- the float pool counts too -- at most
    ``inference_count.PIECE_CLIPS``.  At least 1."""
    frames = ic.MAX_STAGE_BYTES // max(1, int(per_frame_bytes))
    fit = (frames - (stride * (num_segments - 1) + 5 + 1)) // step + 1      # n clips read step (n - 1) + stride (T - 1) + 5 frames
    return max(1, min(int(fit), ic.PIECE_CLIPS))


class TdnSegmentRing:
    """Which per-segment features the clips of ONE video need and where they live in a ring of feature slots: pure host
    bookkeeping, no tensor.

    Clips start every ``step`` frames and their segments every ``stride`` frames (``step`` a multiple of ``stride``), so segment k
    of clip c is segment NUMBER ``j = (step // stride) c + k`` of the video, with centre ``stride * j``, whatever clip reads it.
    Its five frames are ``clamp(centre - 2 + i, 0, total - 1)``: they depend on the centre and, within two frames of the end, on
    the video's length -- so a segment is keyed ``(j, reach)``, ``reach = min(2, total - 1 - centre)`` frames behind the centre
    (2 while the length is unknown: only FINAL segments, whose frame ``centre + 2`` exists, may be computed then).  All segments
    whose centre is ``>= total`` are one and the same pad segment, which lives in ``pad_slot``.

    ``free`` is the list of free slot numbers (``pop()`` hands out its last); several rings -- the streams of a
    ``TdnStreamBatcher`` -- may share one list and one pad slot.  A slot goes back to the list only through ``release`` /
    ``clear``: never while a clip that has not been released still names it."""

    def __init__(self, free: List[int], pad_slot: int, num_segments: int = ic.NUM_SEGMENTS, step: int = ic.CLIP_STEP,
                 stride: int = ic.CLIP_STRIDE):
        if step <= 0 or stride <= 0 or step % stride or num_segments < 1:
            raise ValueError(f'need step a positive multiple of stride, got {step}, {stride}')
        self.free, self.pad_slot = free, int(pad_slot)
        self.T, self.step, self.stride, self.per = int(num_segments), int(step), int(stride), int(step) // int(stride)
        self.slots: Dict[Tuple[int, int], int] = {}

    # ---- geometry ----------------------------------------------------------------------------------------------------------
    def key(self, j: int, total: Optional[int] = None) -> Optional[Tuple[int, int]]:
        """(j, reach) of segment number j in a video of ``total`` frames (None: length unknown); None for the pad segment."""
        centre = self.stride * j
        if total is not None and centre >= total:
            return None
        return (j, 2 if total is None else min(2, total - 1 - centre))

    def frames_of(self, key: Tuple[int, int]) -> List[int]:
        """The five source frames of a segment: ``clamp(centre - 2 + i, 0, centre + reach)``."""
        centre = self.stride * key[0]
        return [min(max(centre - 2 + i, 0), centre + key[1]) for i in range(TDN_FRAMES)]

    def n_final(self, frames_seen: int) -> int:
        """Segments 0 .. n - 1 are final once ``frames_seen`` frames exist: frame ``centre + 2`` is there."""
        return max(0, (int(frames_seen) - 3) // self.stride + 1) if frames_seen >= 3 else 0

    def is_final(self, j: int, frames_seen: int) -> bool:
        return self.stride * j + 2 <= int(frames_seen) - 1

    def n_due(self, frames_seen: int) -> int:
        """Clips 0 .. n - 1 are due: all T segments final, ``step c + stride (T - 1) + 2 <= frames_seen - 1``."""
        last = int(frames_seen) - 1 - self.stride * (self.T - 1) - 2
        return last // self.step + 1 if last >= 0 else 0

    def n_clips(self, total: int) -> int:
        """Clips of a finished video of ``total`` frames: one per ``step`` frames (``inference_count.clip_starts``)."""
        return len(ic.clip_starts(int(total), self.step))

    def segments(self, lo: int, hi: int, total: Optional[int] = None) -> List[Tuple[int, int]]:
        """The unique non-pad segments clips ``[lo, hi)`` read, ascending."""
        if hi <= lo:
            return []
        keys = (self.key(j, total) for j in range(self.per * lo, self.per * (hi - 1) + self.T))
        return [k for k in keys if k is not None]

    # ---- slots -------------------------------------------------------------------------------------------------------------
    @property
    def in_use(self) -> int:
        return len(self.slots)

    def assign(self, keys: Sequence[Tuple[int, int]]) -> List[Tuple[Tuple[int, int], int]]:
        """Give every key that has no slot yet one from the free list: [(key, slot)] of the NEW ones, in the order given.
        IndexError when the list runs out -- nothing is assigned then."""
        new = [k for k in dict.fromkeys(keys) if k not in self.slots]
        if len(new) > len(self.free):
            raise IndexError(f'{len(new)} new segments, {len(self.free)} free slots')
        out = []
        for k in new:
            self.slots[k] = self.free.pop()
            out.append((k, self.slots[k]))
        return out

    def table(self, lo: int, hi: int, total: Optional[int] = None) -> np.ndarray:
        """int32 ``[hi - lo, T]``: the slot of every segment of clips ``[lo, hi)``; KeyError for one that was never assigned."""
        out = np.empty((max(0, hi - lo), self.T), dtype=np.int32)
        for c in range(lo, hi):
            for k in range(self.T):
                key = self.key(self.per * c + k, total)
                out[c - lo, k] = self.pad_slot if key is None else self.slots[key]
        return out

    def release(self, below_clip: int) -> int:
        """Free the slots of the segments no clip ``>= below_clip`` reads (segment numbers ``< per * below_clip``); how many."""
        gone = [k for k in self.slots if k[0] < self.per * below_clip]
        for k in gone:
            self.free.append(self.slots.pop(k))
        return len(gone)

    def clear(self) -> int:
        n = len(self.slots)
        self.free.extend(self.slots.values())
        self.slots.clear()
        return n


def _ring_piece_logits(model, pool: torch.Tensor, a: int, nf: int, total: int, p_lo: int, p_hi: int, batch_clips: int, T: int, step: int,
                       stride: int, dev) -> List[torch.Tensor]:
    """``reuse_segments=True`` for the clips ``[p_lo, p_hi)`` of one staged piece (pool frame 0 is source frame ``a``, pool frame
    ``nf`` the transformed zero frame): ONE window-mode ``tdn_segments`` over the piece's unique segments -- consecutive segment
    numbers -- and, behind them, the pad segment; one slot table uploaded once; one ``forward_ring`` per batch."""
    probe = TdnSegmentRing([], 0, T, step, stride)
    keys = probe.segments(p_lo, p_hi, total)
    n = len(keys) + 1                                         # the pad segment last: the first segment number past the end,
    first = probe.per * p_lo                                  # or (no clip reads it then) one more real segment
    assert [k[0] for k in keys] == list(range(first, first + len(keys)))
    ring = TdnSegmentRing(list(range(n - 2, -1, -1)), n - 1, T, step, stride)
    ring.assign(keys)                                         # slot = segment number - first
    sa, sd = model.ring_shapes(n)
    ring_a, ring_d = torch.empty(sa, dtype=torch.float32, device=dev), torch.empty(sd, dtype=torch.float32, device=dev)
    model.tdn_segments(pool, window=dict(first_source_frame=a, total_frames=total, first_clip=first, clip_stride=stride, pad_frame=nf),
                       n_segments=n, out=(ring_a, ring_d))
    table = staging.upload_table(torch.from_numpy(ring.table(p_lo, p_hi, total)), dev)
    return [model.forward_ring(ring_a, ring_d, table[c - p_lo:c - p_lo + min(batch_clips, p_hi - c)], n_clips=min(batch_clips, p_hi - c))
            for c in range(p_lo, p_hi, batch_clips)]


def tdn_video_clip_logits(model, video_thwc_u8, transform: TestTransform, clip_range: Optional[Tuple[int, int]] = None,
                          batch_clips: int = 32, step: int = ic.CLIP_STEP, frame_format: str = 'rgb',
                          reuse_segments: bool = False) -> torch.Tensor:
    """Raw logits ``[hi - lo, num_class]`` (CPU float32) of the clips ``clip_range`` (default all: one per ``step`` frames) of
    one RGB uint8 video ``[F, H, W, 3]`` for a TDN model.

    A ``TsmEngine`` on a GPU: the contiguous source-frame range the clips read (``tdn_frame_range``) and one zero frame go up
    through ``staging.upload`` -- in pieces of at most ``tdn_clips_per_piece`` clips --, ONE ``preprocess_frames(packed=False)``
    launch per piece transforms them, and every batch is ONE ``forward_pool`` in window mode.  Any other model (a stub, a
    session, a callable taking ``[B, T, 5, 3, H, W]``): the torch transform and ``index_select`` by ``tdn_clip_indices``.

    ``reuse_segments=True`` (an engine only; host models ignore it): per piece ONE ``tdn_segments`` call over the piece's unique
    segments and the pad segment, then one ``forward_ring`` per batch through a slot table uploaded once per piece -- each
    segment's front end, ``resnext_layer1`` and ``layer1`` run once, not once per clip that reads it.  The same bits."""
    _need_tdn_rows(model, transform, 'tdn_video_clip_logits', frame_format)
    video = video_thwc_u8 if isinstance(video_thwc_u8, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(video_thwc_u8))
    if video.dtype != torch.uint8 or video.dim() != 4 or video.shape[3] != 3:
        raise ValueError(f'the video must be uint8 [F, H, W, 3], got {video.dtype} {tuple(video.shape)}')
    total = int(video.shape[0])
    T = int(getattr(model, 'num_segments', ic.NUM_SEGMENTS))
    stride = ic.CLIP_STRIDE
    lo, hi = clip_range if clip_range is not None else (0, len(ic.clip_starts(total, step)))
    if hi <= lo:
        return torch.empty((0, int(getattr(model, 'num_class', 0))), dtype=torch.float32)
    if batch_clips <= 0:
        raise ValueError(f'batch_clips must be positive, got {batch_clips}')
    engine = staging.device_path(model) and hasattr(model, 'forward_pool')
    dev = staging.engine_device(model) if engine else None
    hw = (int(video.shape[1]), int(video.shape[2]))
    per_piece = tdn_clips_per_piece(int(video[0].numel()), step, stride, T) if engine else hi - lo
    out: List[torch.Tensor] = []
    for p_lo in range(lo, hi, per_piece):
        p_hi = min(p_lo + per_piece, hi)
        a, b = tdn_frame_range(total, p_lo, p_hi, step, stride, T)
        nf = b - a                                  # (the zero frame is pool frame nf)
        if engine:
            pool = _stage_pool(lambda pinned, a=a, b=b: pinned.copy_(video[a:b]), nf, hw + (3,), True, transform, dev)
            if reuse_segments:
                out += _ring_piece_logits(model, pool, a, nf, total, p_lo, p_hi, batch_clips, T, step, stride, dev)
                continue
            for c in range(p_lo, p_hi, batch_clips):
                n = min(batch_clips, p_hi - c)
                window = dict(first_source_frame=a, total_frames=total, first_clip=c, clip_step=step, clip_stride=stride, pad_frame=nf)
                out.append(model.forward_pool(pool, window=window, n_clips=n))
        else:
            frames = transform(video[a:b].permute(0, 3, 1, 2).to(torch.float32))
            zero = transform(torch.zeros((1, 3) + hw, dtype=torch.float32))
            pool = torch.cat([frames, zero], dim=0)
            idx = torch.from_numpy(tdn_clip_indices(total, p_lo, p_hi, T, step, stride, a, nf, nf + 1).astype(np.int64))
            for c in range(0, p_hi - p_lo, batch_clips):
                sel = idx[c:c + batch_clips]
                x = torch.index_select(pool, 0, sel.reshape(-1)).view(tuple(sel.shape) + tuple(pool.shape[1:]))
                out.append(torch.from_numpy(staging.call_host(model, x)))
    return torch.cat(out, dim=0).to(torch.float32).cpu()


def tdn_count_video(model, video, transform: TestTransform, threshold: float = 0.5, softmax: bool = True,
                    step: int = ic.CLIP_STEP, reuse_segments: bool = False) -> Tuple[int, List[int]]:
    """(count, reps) of one video: ``tdn_video_clip_logits`` for every clip, then the states and the count exactly as the TSM
    path forms them -- on the GPU ``scores_to_states`` for an engine, ``counting.scores_to_preds`` otherwise, and
    ``counting.pred_to_count``."""
    logits = tdn_video_clip_logits(model, video, transform, step=step, reuse_segments=reuse_segments)
    if logits.shape[0] == 0:
        return 0, []
    rows = logits.to(staging.engine_device(model)) if staging.device_path(model) else logits.numpy()
    return pred_to_count(scores_to_state_list(rows, threshold, softmax), step)


# ---- streams ---------------------------------------------------------------------------------------------------------------------
class _TdnStream:
    """One open stream: its counter, its ring bookkeeping and the host frames from source frame ``base`` on."""

    def __init__(self, counter: RepCounter, ring: TdnSegmentRing):
        self.counter, self.ring = counter, ring
        self.frames: Deque[np.ndarray] = deque()
        self.base = 0          # source frame number of frames[0]
        self.seen = 0          # frames pushed
        self.computed = 0      # segments 0 .. computed - 1 have been computed (all final then)
        self.emitted = 0       # clips 0 .. emitted - 1 have been run
        self.shape: Optional[Tuple[int, ...]] = None


class TdnStreamBatcher:
    """Online counting for many concurrent frame streams on one TDN model: ``StreamBatcher``'s counterpart for clips of five
    frames per segment, in the counting geometry of ``tdn_count_video`` (clips every ``step`` = 8 frames, a segment every 2nd
    frame, overlapping by half).

    ``push(stream_id, frame)`` queues a uint8 ``[H, W, 3]`` RGB frame (one size per stream; sizes may differ between streams).
    Clip c of a stream is DUE once frame ``8 c + 16`` has arrived -- all eight segments are final, no frame they read can still
    clamp at the video's end.  ``step()`` runs the due clips of all streams, in stream order then clip order, and returns
    ``{stream_id: [(clip_index, state, count), ...]}``.  ``close(stream_id)`` first runs the clips still owed (those with ``8 c <
    frames_seen``: with the end-of-video clamp and the pad segment, at most two for a video longer than 16 frames), then returns
    ``(count, reps)``.  For any interleaving of ``push`` and ``step`` the logits of clip c are row c of
    ``tdn_video_clip_logits(model, all frames pushed)`` bit for bit, and ``close`` returns what ``tdn_count_video`` returns.

    A ``TsmEngine`` on a GPU runs in two phases.  ``step()`` uploads and transforms only the frames the NEW
    final segments read (one transform launch per frame size, into one pool), runs those segments through ``tdn_segments`` into a
    ring of feature slots kept between steps -- one call per run of consecutive free slots, usually one --, runs the due clips
    through ``forward_ring`` in batches of at most ``max_batch`` and forms the states on the GPU.  A new clip costs four new
    segments, not eight.  Host frames are kept only from the oldest segment that is not final on.  Ring slots: between steps an
    open stream holds at most 7 (the final segments of clips not yet due); inside a ``step`` or ``close`` that runs D clips of
    the stream at most ``4 D + 7``; all streams share one more slot, the pad segment; ``close`` frees the stream's slots.  The
    ring grows (by doubling, contents copied) when the free list runs out and never shrinks; a slot holds ``(H / 4)^2 x 256 +
    (H / 8)^2 x 256`` floats, 3.8 MiB at 224 x 224.

    Any other model (a stub, a session, a callable) takes the host path: clips ``[B, T, 5, 3, H, W]`` by ``tdn_clip_indices``.
    ``keep_logits=True`` keeps every emitted row in ``self.logits[stream_id]`` as ``(clip_index, float32 row)``, also past
    ``close``.  ``on_window(stream_id, clip_index, state, count)`` is called per emitted clip."""

    def __init__(self, model, threshold: float = 0.5, softmax: bool = True, step: int = ic.CLIP_STEP, max_batch: int = 32,
                 transform: Optional[TestTransform] = None,
                 on_window: Optional[Callable[[Hashable, int, int, int], None]] = None, keep_logits: bool = False,
                 frame_format: str = 'rgb'):
        transform = transform or default_eval_transform(model)
        _need_tdn_rows(model, transform, 'TdnStreamBatcher', frame_format)      # (before the library loads)
        if max_batch <= 0:
            raise ValueError(f'max_batch must be positive, got {max_batch}')
        self.model, self.transform = model, transform
        self.threshold, self.softmax, self.step_frames, self.max_batch = threshold, softmax, int(step), int(max_batch)
        self.stride = ic.CLIP_STRIDE
        self.T = int(getattr(model, 'num_segments', ic.NUM_SEGMENTS))
        self.on_window, self.keep_logits = on_window, bool(keep_logits)
        self.streams: Dict[Hashable, _TdnStream] = {}
        self.logits: Dict[Hashable, List[Tuple[int, np.ndarray]]] = {}
        self._engine = bool(staging.device_path(model) and hasattr(model, 'forward_ring'))
        self._dev = staging.engine_device(model) if self._engine else None
        # the ring: slot 0 is the pad segment (computed when a closing clip first reads it), the free list hands out the
        # lowest slot first so that the segments of a step tend to land in one run
        self._free: List[int] = []
        self._ring_a = self._ring_d = None
        self._pad_ready = False
        TdnSegmentRing(self._free, 0, self.T, self.step_frames, self.stride)     # (validates step / stride)

    # ---- ingest -------------------------------------------------------------------------------------------------------------
    def open(self, stream_id: Hashable) -> _TdnStream:
        if stream_id not in self.streams:
            self.streams[stream_id] = _TdnStream(RepCounter(self.step_frames),
                                                 TdnSegmentRing(self._free, 0, self.T, self.step_frames, self.stride))
        return self.streams[stream_id]

    def push(self, stream_id: Hashable, frame) -> None:
        arr, _hw = pushed_frame(frame, 'rgb', None, to_rgb=False)      # (RGB only: the constructor refused anything else)
        st = self.open(stream_id)
        if st.shape is None:
            st.shape = tuple(arr.shape)
        elif st.shape != tuple(arr.shape):
            raise ValueError(f'frame size changed inside a stream: {st.shape} then {tuple(arr.shape)}')
        st.frames.append(np.ascontiguousarray(arr))
        st.seen += 1

    def ready(self) -> int:
        """Due clips not yet run, over all streams."""
        return sum(max(0, st.ring.n_due(st.seen) - st.emitted) for st in self.streams.values())

    def slots_in_use(self) -> int:
        """Ring slots held by open streams (the shared pad slot not counted)."""
        return sum(st.ring.in_use for st in self.streams.values())

    def result(self, stream_id: Hashable) -> Tuple[int, List[int]]:
        st = self.streams[stream_id]
        return st.counter.count, list(st.counter.reps)

    # ---- compute ------------------------------------------------------------------------------------------------------------
    def step(self) -> Dict[Hashable, List[Tuple[int, int, int]]]:
        """Run the due clips of all streams and update the counters."""
        jobs = [(sid, st, st.emitted, st.ring.n_due(st.seen), None) for sid, st in self.streams.items()]
        return self._run(jobs)

    def close(self, stream_id: Hashable) -> Tuple[int, List[int]]:
        """Run the clips the stream is still owed -- its length is now known -- free its slots and drop it -> (count, reps)."""
        st = self.streams[stream_id]
        if st.seen > 0:
            self._run([(stream_id, st, st.emitted, st.ring.n_clips(st.seen), st.seen)])
        st.ring.clear()
        del self.streams[stream_id]
        return st.counter.count, list(st.counter.reps)

    def _run(self, jobs) -> Dict[Hashable, List[Tuple[int, int, int]]]:
        out: Dict[Hashable, List[Tuple[int, int, int]]] = {}
        rows = self._logits_engine(jobs) if self._engine else self._logits_host(jobs)
        order = [(sid, st, c) for sid, st, lo, hi, _total in jobs for c in range(lo, hi)]
        if order:
            # (an engine's rows: states on the GPU too, one int32 per clip crosses in the step's only sync; kept rows follow it)
            states = scores_to_state_list(rows, self.threshold, self.softmax)
            if self.keep_logits and isinstance(rows, torch.Tensor):
                rows = rows.cpu().numpy()
            for i, ((sid, st, c), state) in enumerate(zip(order, states)):
                count = st.counter.push(state)
                st.emitted = c + 1
                out.setdefault(sid, []).append((c, state, count))
                if self.keep_logits:
                    self.logits.setdefault(sid, []).append((c, np.array(rows[i], dtype=np.float32)))
                if self.on_window is not None:
                    self.on_window(sid, c, state, count)
        for _sid, st, _lo, _hi, _total in jobs:
            st.ring.release(st.emitted)
            # frames: from the first one the oldest segment still to compute reads (the engine path computes every final
            # segment; the host path recomputes a clip's segments, so it keeps those of the next clip to run)
            first = self.stride * (st.computed if self._engine else st.ring.per * st.emitted) - 2
            while st.base < first and st.frames:
                st.frames.popleft()
                st.base += 1
        return out

    def _grow(self, need: int) -> None:
        """Ring capacity for ``need`` more slots: doubled until the free list holds them (contents copied; not steady state)."""
        have = 0 if self._ring_a is None else int(self._ring_a.shape[0])
        want = max(have, 16)
        while want - max(have, 1) + len(self._free) < need:     # (slot 0 is the pad segment's, never on the free list)
            want *= 2
        if self._ring_a is not None and want == have:
            return
        sa, sd = self.model.ring_shapes(want)
        ring_a, ring_d = torch.empty(sa, dtype=torch.float32, device=self._dev), torch.empty(sd, dtype=torch.float32, device=self._dev)
        if self._ring_a is not None:
            ring_a[:have].copy_(self._ring_a)
            ring_d[:have].copy_(self._ring_d)
        self._ring_a, self._ring_d = ring_a, ring_d
        self._free.extend(range(max(have, 1), want))          # (slot 0 is the pad segment's)
        self._free.sort(reverse=True)

    def _logits_engine(self, jobs) -> Optional[torch.Tensor]:
        tf, dev = self.transform, self._dev
        # 1. the new segments of every job: the final ones not yet computed and, with the length known, the rest the clips read
        new: List[Tuple[_TdnStream, Tuple[int, int]]] = []
        need_pad = False
        for _sid, st, lo, hi, total in jobs:
            keys = [st.ring.key(j, total) for j in range(st.computed, st.ring.n_final(st.seen))]
            if total is not None:
                keys += st.ring.segments(lo, hi, total)
                need_pad = need_pad or (hi > lo and self.stride * (st.ring.per * (hi - 1) + self.T - 1) >= total)
            new += [(st, k) for k in dict.fromkeys(keys) if k not in st.ring.slots]
        want_pad = need_pad and not self._pad_ready
        if new or want_pad:
            self._free.sort(reverse=True)
            if self._ring_a is None or len(new) > len(self._free):
                self._grow(len(new))
            # 2. the frames they read: per frame size the union, in (stream, frame) order, into ONE pool; a zero frame for the pad
            groups: Dict[Tuple[int, ...], Dict[Tuple[int, int], int]] = {}
            for st, k in new:
                g = groups.setdefault(st.shape, {})
                for f in st.ring.frames_of(k):
                    g.setdefault((id(st), f), len(g))
            if want_pad and not groups:
                groups[next(st.shape for _s, st, *_ in jobs)] = {}
            n_pool = sum(len(g) for g in groups.values()) + (1 if want_pad else 0)
            pool = torch.empty((n_pool, 3, int(tf.crop), int(tf.crop)), dtype=torch.float32, device=dev)
            by_id = {id(st): st for st, _k in new}
            offset, where = 0, {}
            for gi, (shape, g) in enumerate(groups.items()):
                zero = 1 if want_pad and gi == 0 else 0        # (the zero frame rides with the first group, behind its frames)

                def fill(pinned: torch.Tensor, g=g) -> None:
                    for (sid_, f), i in g.items():
                        s_ = by_id[sid_]
                        pinned[i].copy_(torch.from_numpy(s_.frames[f - s_.base]))
                _stage_pool(fill, len(g), shape, bool(zero), tf, dev, out=pool[offset:offset + len(g) + zero])
                for key, i in g.items():
                    where[key] = offset + i
                if zero:
                    where['pad'] = offset + len(g)
                offset += len(g) + zero
            # 3. slots, then one tdn_segments call per run of consecutive slots over ONE index table in slot order
            pairs = []
            for st, k in new:
                (_, slot), = st.ring.assign([k])
                pairs.append((slot, [where[(id(st), f)] for f in st.ring.frames_of(k)]))
            if want_pad:
                pairs.append((0, [where['pad']] * TDN_FRAMES))
            pairs.sort(key=lambda p: p[0])
            index = staging.upload_table(torch.tensor([r for _s, r in pairs], dtype=torch.int32), dev)
            i = 0
            while i < len(pairs):
                j = i + 1
                while j < len(pairs) and pairs[j][0] == pairs[j - 1][0] + 1:
                    j += 1
                s0 = pairs[i][0]
                self.model.tdn_segments(pool, index[i:j], n_segments=j - i, out=(self._ring_a[s0:s0 + j - i], self._ring_d[s0:s0 + j - i]))
                i = j
            self._pad_ready = self._pad_ready or want_pad
        for _sid, st, _lo, _hi, total in jobs:
            st.computed = max(st.computed, st.ring.n_final(st.seen))
        # 4. the clips: one slot table for the step, forward_ring in batches
        tables = [st.ring.table(lo, hi, total) for _sid, st, lo, hi, total in jobs if hi > lo]
        if not tables:
            return None
        table = staging.upload_table(torch.from_numpy(np.concatenate(tables)), dev)
        n = int(table.shape[0])
        rows = [self.model.forward_ring(self._ring_a, self._ring_d, table[c:c + self.max_batch], n_clips=min(self.max_batch, n - c))
                for c in range(0, n, self.max_batch)]
        return rows[0] if len(rows) == 1 else torch.cat(rows)

    def _logits_host(self, jobs) -> Optional[np.ndarray]:
        """Clips ``[B, T, 5, 3, H, W]`` by ``tdn_clip_indices`` over the kept frames and one transformed zero frame."""
        tf, xs = self.transform, []
        for _sid, st, lo, hi, total in jobs:
            if hi <= lo:
                continue
            frames = tf(torch.from_numpy(np.stack(st.frames)).permute(0, 3, 1, 2).to(torch.float32))
            zero = tf(torch.zeros((1, 3) + st.shape[:2], dtype=torch.float32))
            pool = torch.cat([frames, zero], dim=0)
            nf = int(frames.shape[0])
            idx = tdn_clip_indices(st.seen if total is None else total, lo, hi, self.T, self.step_frames, self.stride, st.base, nf, nf + 1)
            sel = torch.from_numpy(idx.astype(np.int64))
            xs.append(torch.index_select(pool, 0, sel.reshape(-1)).view(tuple(sel.shape) + tuple(pool.shape[1:])))
        if not xs:
            return None
        x = torch.cat(xs, dim=0)
        return np.concatenate([staging.call_host(self.model, x[c:c + self.max_batch]) for c in range(0, x.shape[0], self.max_batch)])


# ---- accuracy --------------------------------------------------------------------------------------------------------------------
def _tdn_groups(samples: Sequence[Mapping], T: int, rng) -> List[Tuple[str, List[int], List[List[int]]]]:
    """(frame_dir, sample indices, their T * 5 frame numbers -- those of the file names), directories in first-appearance order;
    the draws of ``rng`` are made in sample order."""
    groups = {}
    for i, s in enumerate(samples):
        numbers = (tdn_sample_frames(int(s['total_frames']), T, TDN_FRAMES, rng) + int(s.get('start_index', 1))).reshape(-1).tolist()
        ids, rows = groups.setdefault(s['frame_dir'], ([], []))
        ids.append(i)
        rows.append(numbers)
    return [(d, ids, rows) for d, (ids, rows) in groups.items()]


def tdn_eval_classification(model, samples: Sequence[Mapping], frame_reader: Optional[FrameReader] = None,
                            rng: Optional[np.random.RandomState] = None, batch_clips: Optional[int] = None,
                            return_logits: bool = False, transform: Optional[TestTransform] = None) -> dict:
    """``classification.eval_classification`` for a TDN model: the same samples, reader, grouping by directory and result dict
    (``correct``, ``total``, ``acc``, ``overall``, ``preds``, and ``logits`` with ``return_logits``).  Per labelled segment the
    ``T x 5`` frames ``tdn_sample_frames(total_frames, T, 5, rng) + start_index`` (``rng=None``: the deterministic midpoints; an
    ``np.random.RandomState``: the reference's training-time draws, made in sample order).

    A ``TsmEngine`` on a GPU stages the union of a directory's frames (beyond ``inference_count.MAX_STAGE_BYTES`` in pieces of
    whole samples), makes ONE ``preprocess_frames(packed=False)`` launch per piece and, per batch, one table-mode
    ``forward_pool`` and one ``top1_tally`` into device counters.  Any other model (``staging.call_host`` on ``[B, T, 5, 3, H, W]``:
    a session, a torch module, a callable) takes the host path with the same result.  The loop, the tally and the result dict
    are ``classification.evaluate``'s; what is TDN's own is below: the frame numbers, the pool and the clips of the host path."""
    transform = transform or default_eval_transform(model)
    _need_tdn_rows(model, transform, 'tdn_eval_classification')
    T = int(getattr(model, 'num_segments', ic.NUM_SEGMENTS))

    def stage(union, _first, probe, read, dev):
        pool = _stage_pool(lambda pinned: pinned.copy_(read(union)), len(union), tuple(probe.shape[1:]), False, transform, dev)
        return lambda table, out: model.forward_pool(pool, table, n_clips=int(table.shape[0]), out=out)

    def host_clips(frames: torch.Tensor):
        pool = transform(frames.permute(0, 3, 1, 2).to(torch.float32))
        return lambda table: torch.index_select(pool, 0, table.reshape(-1)).view((table.shape[0], T, TDN_FRAMES) + tuple(pool.shape[1:]))
    samples = list(samples)
    return evaluate('tdn_eval_classification', model, samples, _tdn_groups(samples, T, rng), frame_reader or read_frames, batch_clips,
                    return_logits, lambda rows: rows[0][0], stage if hasattr(model, 'forward_pool') else None, host_clips)
