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

Out of scope: YUV input, person crop, streams (``StreamBatcher``) and ``shard='global'``; and computing the per-frame part of the
network once per unique segment of overlapping clips."""
from __future__ import annotations

from typing import List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from . import inference_count as ic
from . import staging
from .classification import RESIZE, FrameReader, _pieces, _read, _table, read_frames
from .counting import pred_to_count, scores_to_preds
from .transform import INPUT_SIZE, PersonCropTransform, TestTransform

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


def _call_host(model, x: torch.Tensor) -> np.ndarray:
    """A model without a device path on clips ``[B, T, 5, 3, H, W]``: the onnxruntime duck type, a torch module or a callable."""
    if hasattr(model, 'run') and hasattr(model, 'get_inputs'):
        return np.asarray(model.run(None, {model.get_inputs()[0].name: x.cpu().numpy()})[0], dtype=np.float32)
    return staging.call_host_module(model, x)


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


def tdn_video_clip_logits(model, video_thwc_u8, transform: TestTransform, clip_range: Optional[Tuple[int, int]] = None,
                          batch_clips: int = 32, step: int = ic.CLIP_STEP, frame_format: str = 'rgb') -> torch.Tensor:
    """Raw logits ``[hi - lo, num_class]`` (CPU float32) of the clips ``clip_range`` (default all: one per ``step`` frames) of
    one RGB uint8 video ``[F, H, W, 3]`` for a TDN model.

    A ``TsmEngine`` on a GPU: the contiguous source-frame range the clips read (``tdn_frame_range``) and one zero frame go up
    through ``staging.upload`` -- in pieces of at most ``tdn_clips_per_piece`` clips --, ONE ``preprocess_frames(packed=False)``
    launch per piece transforms them, and every batch is ONE ``forward_pool`` in window mode.  Any other model (a stub, a
    session, a callable taking ``[B, T, 5, 3, H, W]``): the torch transform and ``index_select`` by ``tdn_clip_indices``."""
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
            from .engine import preprocess_frames

            def fill(pinned: torch.Tensor, a=a, b=b) -> None:
                pinned[:-1].copy_(video[a:b])
                pinned[-1].zero_()
            staged, _ready = staging.upload((nf + 1,) + hw + (3,), fill, dev)
            pool = preprocess_frames(staged, resize=transform.size, crop=transform.crop, scale_255=transform.scale_255, packed=False)
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
                out.append(torch.from_numpy(_call_host(model, x)))
    return torch.cat(out, dim=0).to(torch.float32).cpu()


def tdn_count_video(model, video, transform: TestTransform, threshold: float = 0.5, softmax: bool = True,
                    step: int = ic.CLIP_STEP) -> Tuple[int, List[int]]:
    """(count, reps) of one video: ``tdn_video_clip_logits`` for every clip, then the states and the count exactly as the TSM
    path forms them -- on the GPU ``scores_to_states`` for an engine, ``counting.scores_to_preds`` otherwise, and
    ``counting.pred_to_count``."""
    logits = tdn_video_clip_logits(model, video, transform, step=step)
    if logits.shape[0] == 0:
        return 0, []
    if staging.device_path(model):
        from .engine import scores_to_states
        states = scores_to_states(logits.to(staging.engine_device(model)), threshold=threshold, softmax=softmax).cpu().tolist()
    else:
        states = scores_to_preds(logits.numpy(), threshold=threshold, softmax=softmax)
    return pred_to_count(states, step)


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


def _tdn_eval_engine(model, samples, groups, reader, batch: int, transform: TestTransform, want_logits: bool):
    from .engine import preprocess_frames, top1_tally
    dev = staging.engine_device(model)
    n, c = len(samples), int(model.num_class)
    counters = staging.upload_table(torch.zeros((2, c), dtype=torch.int32), dev)
    preds = torch.empty((n,), dtype=torch.int32, device=dev)
    logits = torch.empty((n, c), dtype=torch.float32, device=dev)
    done = 0
    for frame_dir, ids, rows in groups:
        probe = _read(reader, frame_dir, rows[0][:1])                        # one frame: the directory's geometry
        for a, b in _pieces(rows, int(probe[0].numel()), ic.MAX_STAGE_BYTES):
            union = sorted(set().union(*rows[a:b]))
            table = torch.from_numpy(_table(union, rows[a:b]))           # [b - a, T * 5], validated on the host
            labels = torch.tensor([int(samples[i]['label']) for i in ids[a:b]], dtype=torch.int32)

            def fill(pinned: torch.Tensor, union=union) -> None:
                got = _read(reader, frame_dir, union)
                if tuple(got.shape[1:]) != tuple(probe.shape[1:]):
                    raise ValueError(f'{frame_dir}: frames of {tuple(got.shape[1:3])} and {tuple(probe.shape[1:3])} pixels')
                pinned.copy_(got)
            staged, _ready = staging.upload((len(union),) + tuple(probe.shape[1:]), fill, dev)
            pool = preprocess_frames(staged, resize=transform.size, crop=transform.crop, scale_255=transform.scale_255, packed=False)
            table, labels = staging.upload_table(table, dev), staging.upload_table(labels, dev)
            for lo in range(0, b - a, batch):
                hi = min(lo + batch, b - a)
                out = model.forward_pool(pool, table[lo:hi], n_clips=hi - lo, out=logits[done:done + hi - lo])
                top1_tally(out, labels[lo:hi], counters[0], counters[1], out=preds[done:done + hi - lo])
                done += hi - lo
    counters = counters.cpu()
    return counters[0].tolist(), counters[1].tolist(), preds.cpu().tolist(), logits.cpu().numpy() if want_logits else None


def _tdn_eval_host(model, samples, groups, reader, batch: int, transform: TestTransform, want_logits: bool):
    c = int(getattr(model, 'num_class', 0))
    T = int(getattr(model, 'num_segments', ic.NUM_SEGMENTS))
    rows_out: List[np.ndarray] = []
    for frame_dir, ids, rows in groups:
        union = sorted(set().union(*rows))
        frames = transform(_read(reader, frame_dir, union).permute(0, 3, 1, 2).to(torch.float32))
        table = torch.from_numpy(_table(union, rows).astype(np.int64))
        for lo in range(0, len(ids), batch):
            sel = table[lo:lo + batch]
            x = torch.index_select(frames, 0, sel.reshape(-1)).view((sel.shape[0], T, TDN_FRAMES) + tuple(frames.shape[1:]))
            rows_out.append(_call_host(model, x))
    logits = np.concatenate(rows_out) if rows_out else np.zeros((0, c), dtype=np.float32)
    if logits.ndim != 2:
        raise ValueError(f'tdn_eval_classification needs one row of scores per clip, the model returned {logits.shape}')
    c = c or int(logits.shape[1])
    preds = logits.argmax(axis=1).astype(np.int64) if len(logits) else np.zeros((0,), dtype=np.int64)
    correct, total = [0] * c, [0] * c
    order = [i for _d, ids, _r in groups for i in ids]
    for p, i in zip(preds.tolist(), order):
        label = int(samples[i]['label'])
        if 0 <= label < c:
            total[label] += 1
            correct[label] += int(p == label)
    return correct, total, preds.tolist(), logits if want_logits else None


def tdn_eval_classification(model, samples: Sequence[Mapping], frame_reader: Optional[FrameReader] = None,
                            rng: Optional[np.random.RandomState] = None, batch_clips: Optional[int] = None,
                            return_logits: bool = False, transform: Optional[TestTransform] = None) -> dict:
    """``classification.eval_classification`` for a TDN model: the same samples, reader, grouping by directory and result dict
    (``correct``, ``total``, ``acc``, ``overall``, ``preds``, and ``logits`` with ``return_logits``).  Per labelled segment the
    ``T x 5`` frames ``tdn_sample_frames(total_frames, T, 5, rng) + start_index`` (``rng=None``: the deterministic midpoints; an
    ``np.random.RandomState``: the reference's training-time draws, made in sample order).

    A ``TsmEngine`` on a GPU stages the union of a directory's frames (beyond ``inference_count.MAX_STAGE_BYTES`` in pieces of
    whole samples), makes ONE ``preprocess_frames(packed=False)`` launch per piece and, per batch, one table-mode
    ``forward_pool`` and one ``top1_tally`` into device counters.  Any other model takes the host path with the same result."""
    if transform is None:
        transform = TestTransform(RESIZE, int(getattr(model, 'height', INPUT_SIZE)), scale_255=True)
    _need_tdn_rows(model, transform, 'tdn_eval_classification')
    reader = frame_reader or read_frames
    T = int(getattr(model, 'num_segments', ic.NUM_SEGMENTS))
    samples = list(samples)
    groups = _tdn_groups(samples, T, rng)
    engine = staging.device_path(model) and hasattr(model, 'forward_pool')
    limit = int(model.max_clips) if engine else None
    batch = int(batch_clips or limit or 32)
    if batch <= 0:
        raise ValueError(f'batch_clips must be positive, got {batch_clips}')
    if limit:
        batch = min(batch, limit)
    run = _tdn_eval_engine if engine and samples else _tdn_eval_host
    correct, total, preds, logits = run(model, samples, groups, reader, batch, transform, return_logits)
    order = [i for _d, ids, _r in groups for i in ids]
    back = np.empty(len(order), dtype=np.int64)
    back[order] = np.arange(len(order))
    res = {'correct': [int(v) for v in correct], 'total': [int(v) for v in total],
           'acc': [c / n if n else None for c, n in zip(correct, total)],
           'overall': sum(correct) / sum(total) if sum(total) else None,
           'preds': [int(preds[j]) for j in back]}
    if return_logits:
        res['logits'] = logits[back]
    return res
