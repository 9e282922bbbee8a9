"""Classification accuracy of a clip model over labelled state segments, on top of the HIP TSM engine.

Counterpart of workoutdetector/scripts/eval_classification.py over ``FrameDataset``:

  sample_frames          datasets/transform.py:16-65    the deterministic branch (``random=False``)
  load_annotation        datasets/common.py:74-97       ``frame_dir [start_index] total_frames label`` lines
  eval_classification    scripts/eval_classification.py:36-46 over datasets/common.py:99-117 (``FrameDataset.__getitem__``)
  main                   scripts/eval_classification.py:13-52, datasets/build.py:21-38

A sample is a labelled segment of a directory of frames.  The reference takes 8 of its frames uniformly
(``sample_frames(total, 8, start, random=False)``), runs ``build_test_transform(person_crop=False)`` on them
(ConvertImageDtype -> Resize(256) -> CenterCrop(224) -> Normalize; ``read_image`` yields uint8, so ConvertImageDtype DOES
divide by 255 here -- ``scale_255=True``; this path has no ``torch.cat`` promotion quirk), runs the model and compares.

What differs from the reference, on purpose:
  * the reference script never increments ``class_total`` (it divides by zero) and compares a logits ROW with the label
    (:45).  This module implements the intent -- the first arg-max of the row equals the label, counted per class -- as
    ``count_by_video_model`` implements the intent of its broken counterpart.
  * a ``TsmEngine`` gets the device path: per directory only the UNION of the sampled frames is staged (sorted, unique,
    uint8, pinned then device), an int32 table maps every (sample, segment) to its place in that buffer, and a batch is ONE
    ``tsm_preprocess_indexed`` launch into the engine's packed input, the forward, and ONE ``tsm_top1_tally`` launch.
    Counters, preds (and logits, when asked for) stay on the device and cross PCIe once, at the end.  No torch kernel runs.
  * frames come from a pluggable ``frame_reader(frame_dir, frame_numbers) -> uint8 [n,H,W,3]``; the default reads
    ``img_{:05}.jpg`` with Pillow.

Out of scope:
  * ``transform.person_crop`` of the reference's config: ``main(person_crop=True)`` is refused (the dataset loop has the
    person-crop transform, ``inference_count.inference_dataset(person_crop=True)``);
  * the random training branch of ``sample_frames`` (``random=True``): every split is sampled deterministically, as the
    reference samples 'val' and 'test';
  * multi-rank sharding: one process evaluates the whole list;
  * batching across directories: a batch holds samples of one directory, so a directory's last batch may be short.
"""
from __future__ import annotations

import json
import math
import os
from typing import Callable, Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from . import inference_count as ic
from . import staging
from .transform import INPUT_SIZE, TestTransform

FILENAME_TMPL = 'img_{:05}.jpg'
RESIZE = 256

FrameReader = Callable[[str, Sequence[int]], np.ndarray]


# ---- sampling and annotations --------------------------------------------------------------------------------------------
def sample_frames(total: int, num: int, offset: int = 0) -> List[int]:
    """``num`` frame numbers spread uniformly over a segment of ``total`` frames that starts at ``offset``: the first frame
    of each of ``num`` equal intervals (datasets/transform.py:16-65 with ``random=False``).  A segment shorter than ``num``
    repeats every frame ``ceil(num / total)`` times first, so frames occur more than once and the last ones may not occur
    at all: ``sample_frames(5, 8) == [0, 0, 1, 1, 2, 2, 3, 3]``.  ``total <= 0`` raises ValueError (the reference divides by
    zero there)."""
    total, num, offset = int(total), int(num), int(offset)
    if total <= 0 or num <= 0:
        raise ValueError(f'sample_frames needs total > 0 and num > 0, got total={total}, num={num}')
    if total < num:
        repeats = math.ceil(num / total)
        data = [x for x in range(total) for _ in range(repeats)]
    else:
        data = list(range(total))
    interval = len(data) // num
    return [data[i] + offset for i in range(0, len(data), interval)[:num]]


def load_annotation(anno_path: str, data_prefix: Optional[str] = None, anno_col: int = 4) -> List[dict]:
    """The samples of an annotation file (``FrameDataset.load_annotation``): lines ``frame_dir start_index total_frames
    label`` (``anno_col=4``; ``start_index`` is 1-based, the number in the frame's file name) or ``frame_dir total_frames
    label`` (``anno_col=3``: ``start_index`` 1).  ``data_prefix`` is joined in front of ``frame_dir`` where the segment has
    frames, as the reference does.  Returns dicts with ``frame_dir``, ``start_index``, ``total_frames`` and ``label``."""
    if anno_col not in (3, 4):
        raise ValueError(f'anno_col must be 3 or 4, got {anno_col}')
    samples = []
    with open(anno_path, 'r') as f:
        for ln, line in enumerate(f, start=1):
            parts = line.split()
            if not parts:
                continue
            if len(parts) != anno_col:
                raise ValueError(f'{anno_path}:{ln}: expected {anno_col} columns, got {len(parts)}')
            frame_dir = parts[0]
            start_index = int(parts[1]) if anno_col == 4 else 1
            total_frames, label = int(parts[-2]), int(parts[-1])
            if data_prefix is not None and total_frames > 0:
                frame_dir = os.path.join(data_prefix, frame_dir)
            samples.append(dict(frame_dir=frame_dir, start_index=start_index, total_frames=total_frames, label=label))
    return samples


def read_frames(frame_dir: str, frame_numbers: Sequence[int], filename_tmpl: str = FILENAME_TMPL) -> np.ndarray:
    """The default ``frame_reader``: ``frame_dir/img_{:05}.jpg`` for every number, decoded with Pillow -> uint8 [n,H,W,3]
    (RGB, as torchvision's ``read_image`` yields them)."""
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError('the default frame_reader decodes with Pillow, which is absent: pass frame_reader=...') from e
    frames = []
    for i in frame_numbers:
        with Image.open(os.path.join(frame_dir, filename_tmpl.format(int(i)))) as im:
            frames.append(np.asarray(im.convert('RGB'), dtype=np.uint8))
    return np.stack(frames)


def _read(reader: FrameReader, frame_dir: str, numbers: Sequence[int]) -> torch.Tensor:
    got = reader(frame_dir, list(numbers))
    got = got if isinstance(got, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(got))
    if got.dtype != torch.uint8 or got.dim() != 4 or got.shape[0] != len(numbers) or got.shape[3] != 3:
        raise ValueError(f'frame_reader({frame_dir!r}, {len(numbers)} numbers) must return uint8 [{len(numbers)},H,W,3], got '
                         f'{got.dtype} {tuple(got.shape)}')
    return got


# ---- the evaluation ------------------------------------------------------------------------------------------------------
def _by_directory(samples: Sequence[Mapping], num_segments: int) -> List[Tuple[str, List[int], List[List[int]]]]:
    """(frame_dir, sample indices, their sampled frame numbers), directories in first-appearance order."""
    groups: Dict[str, Tuple[List[int], List[List[int]]]] = {}
    for i, s in enumerate(samples):
        numbers = sample_frames(s['total_frames'], num_segments, s.get('start_index', 1))
        ids, rows = groups.setdefault(s['frame_dir'], ([], []))
        ids.append(i)
        rows.append(numbers)
    return [(d, ids, rows) for d, (ids, rows) in groups.items()]


def _table(union: Sequence[int], rows: Sequence[Sequence[int]]) -> np.ndarray:
    """int32 [n, T]: the place of every sampled frame number in the sorted, unique ``union``; validated here, on the host
    (the kernel is total in the table and would turn a wrong entry into a zero frame silently)."""
    u = np.asarray(union, dtype=np.int64)
    want = np.asarray(rows, dtype=np.int64)
    idx = np.searchsorted(u, want)
    if idx.size and (int(idx.max()) >= len(u) or not np.array_equal(u[idx], want)):
        raise AssertionError('index table does not address the staged frames')
    return idx.astype(np.int32)


def _pieces(rows: Sequence[Sequence[int]], per_frame_bytes: int, budget: int) -> List[Tuple[int, int]]:
    """Ranges [a, b) of whole samples whose union of frames fits ``budget`` bytes (a piece holds at least one sample)."""
    out, a, union = [], 0, set()
    for i, r in enumerate(rows):
        grown = union | set(r)
        if i > a and len(grown) * per_frame_bytes > budget:
            out.append((a, i))
            a, grown = i, set(r)
        union = grown
    out.append((a, len(rows)))
    return out


def default_eval_transform(model) -> TestTransform:
    """The test transform of an accuracy run or a TDN stream when none is given: ``TestTransform(256, model height or 224,
    scale_255=True)``."""
    return TestTransform(RESIZE, int(getattr(model, 'height', INPUT_SIZE)), scale_255=True)


def _eval_engine(model, samples, groups, reader, batch: int, want_logits: bool, probe_frame, stage):
    """The device path: see the module docstring.  Returns (correct, total, preds, logits | None) in PROCESSING order."""
    from .engine import top1_tally
    dev = staging.engine_device(model)
    n, c = len(samples), int(model.num_class)
    # (host zeros copied up, empty device buffers written by the library's own launches: no torch kernel anywhere)
    counters = staging.upload_table(torch.zeros((2, c), dtype=torch.int32), dev)
    preds = torch.empty((n,), dtype=torch.int32, device=dev)
    logits = torch.empty((n, c), dtype=torch.float32, device=dev)
    done = 0
    for frame_dir, ids, rows in groups:
        first = probe_frame(rows)
        probe = _read(reader, frame_dir, [first])                        # one frame: the directory's geometry

        def read(numbers: Sequence[int]) -> torch.Tensor:
            got = _read(reader, frame_dir, numbers)
            if tuple(got.shape[1:]) != tuple(probe.shape[1:]):
                raise ValueError(f'{frame_dir}: frames of {tuple(got.shape[1:3])} and {tuple(probe.shape[1:3])} pixels')
            return got
        for a, b in _pieces(rows, int(probe[0].numel()), ic.MAX_STAGE_BYTES):
            union = sorted(set().union(*rows[a:b]))
            table = torch.from_numpy(_table(union, rows[a:b]))           # validated on the host
            labels = torch.tensor([int(samples[i]['label']) for i in ids[a:b]], dtype=torch.int32)
            forward = stage(union, first, probe, read, dev)
            table, labels = staging.upload_table(table, dev), staging.upload_table(labels, dev)
            for lo in range(0, b - a, batch):
                hi = min(lo + batch, b - a)
                out = forward(table[lo:hi], logits[done:done + hi - lo])
                top1_tally(out, labels[lo:hi], counters[0], counters[1], out=preds[done:done + hi - lo])
                done += hi - lo
    counters = counters.cpu()
    return (counters[0].tolist(), counters[1].tolist(), preds.cpu().tolist(),
            logits.cpu().numpy() if want_logits else None)


def _eval_host(where: str, model, samples, groups, reader, batch: int, want_logits: bool, host_clips):
    """Any other model (``staging.call_host``: sessions, torch modules, callables, CPU stubs): every directory's union read
    once, ``host_clips`` of it, one call per batch, arg-max and tally in NumPy.  Same return as ``_eval_engine``."""
    c = int(getattr(model, 'num_class', 0))
    rows_out: List[np.ndarray] = []
    for frame_dir, ids, rows in groups:
        union = sorted(set().union(*rows))
        clips = host_clips(_read(reader, frame_dir, union))
        table = torch.from_numpy(_table(union, rows).astype(np.int64))
        for lo in range(0, len(ids), batch):
            rows_out.append(staging.call_host(model, clips(table[lo:lo + batch])))
    logits = np.concatenate(rows_out) if rows_out else np.zeros((0, c), dtype=np.float32)
    if logits.ndim != 2:
        raise ValueError(f'{where} needs one row of scores per clip, the model returned {logits.shape}')
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


def evaluate(where: str, model, samples: Sequence[Mapping], groups, reader: FrameReader, batch_clips: Optional[int],
             return_logits: bool, probe_frame, stage, host_clips) -> dict:
    """The accuracy loop behind ``eval_classification`` and ``tdn_pipeline.tdn_eval_classification`` (``where``: the one that
    was called, for messages): the batch size, the engine-or-host decision, the loop over directories, pieces and batches,
    the tally and the result dict.  ``groups``: ``(frame_dir, sample indices, their frame numbers)`` per directory.  What a
    family of models adds:

      ``probe_frame(rows)``    the frame number ``first`` that is read first, alone: ``probe``, the directory's frame size
                               (engine path);
      ``stage(union, first, probe, read, dev)``
                               stages the frames ``union`` of one piece on ``dev`` -- ``read(numbers)`` reads frames and
                               refuses another size than the probe's -- and returns ``forward(table rows, out)``, which
                               enqueues one batch into ``out``; None: the family has no device path for this model;
      ``host_clips(frames)``   takes a directory's uint8 ``[n,H,W,3]`` union and returns ``clips(table rows)``, the batch a
                               host model is called on."""
    engine = staging.device_path(model) and stage is not None
    limit = int(model.max_clips) if engine else None
    batch = int(batch_clips or limit or 32)
    if batch <= 0:
        raise ValueError(f'batch_clips must be positive, got {batch_clips}')
    if limit:
        batch = min(batch, limit)
    if engine and samples:
        correct, total, preds, logits = _eval_engine(model, samples, groups, reader, batch, return_logits, probe_frame, stage)
    else:
        correct, total, preds, logits = _eval_host(where, model, samples, groups, reader, batch, return_logits, host_clips)
    # processing order (by directory) -> sample order
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


def eval_classification(model, samples: Sequence[Mapping], frame_reader: Optional[FrameReader] = None,
                        batch_clips: Optional[int] = None, return_logits: bool = False,
                        transform: Optional[TestTransform] = None) -> dict:
    """Accuracy of ``model`` over labelled segments (``load_annotation``'s dicts): per sample ``num_segments`` frames by
    ``sample_frames(total_frames, num_segments, start_index)``, the centre-crop test transform with ``scale_255=True``, the
    model, and "the first arg-max of the scores equals the label" -- the INTENT of scripts/eval_classification.py:42-49,
    whose loop compares a logits row with the label and never counts ``class_total``; its bugs are not reproduced.

    Returns ``{'correct': [num_class], 'total': [num_class], 'acc': [correct / total, None for a class without samples],
    'overall': sum(correct) / sum(total) (None without any), 'preds': [n]}`` with ``preds`` in sample order, plus
    ``'logits'`` (float32 [n, num_class]) with ``return_logits``.  A label outside [0, num_class) is counted nowhere.

    ``frame_reader(frame_dir, frame_numbers) -> uint8 [n,H,W,3]`` (default ``read_frames``: ``img_{:05}.jpg`` with
    Pillow); the numbers are those of the file names (``start_index`` is 1-based).  Samples are grouped by ``frame_dir`` in
    first-appearance order and every directory's frames are read once: exactly the union of its sampled frames.

    A ``TsmEngine`` stages that union (pinned, then device; a directory beyond ``inference_count.MAX_STAGE_BYTES`` in
    pieces of whole samples) and runs, per batch of at most ``batch_clips`` (default and limit: its ``max_clips``) samples,
    one ``preprocess_indexed_kernel`` launch, the forward and one ``top1_tally_kernel`` launch; counters and preds come back
    once, at the end.  Any other model -- an onnxruntime-style session (``run()`` duck type), a torch module or a plain
    callable on ``[B, T, 3, H, W]`` (``staging.call_host``) -- takes the host path with the same result.  ``transform``:
    a ``TestTransform`` naming resize / crop / scaling (default ``default_eval_transform``: ``TestTransform(256, model height
    or 224, scale_255=True)``).  A model with per-segment scores (``consensus_type='identity'``) is refused up front.
    Out of scope: person crop, random sampling, multi-rank sharding, batches across directories (module docstring)."""
    ic.need_clip_rows(model, 'eval_classification')
    t = int(getattr(model, 'num_segments', ic.NUM_SEGMENTS))
    tf = transform or default_eval_transform(model)

    def stage(union, first, probe, read, dev):
        """The piece's union through ``staging.upload``, the probed frame copied from the probe, not read again; then per batch
        ONE ``preprocess_indexed`` launch into the packed input and the forward."""
        from .engine import preprocess_indexed
        rest = [f for f in union if f != first]

        def fill(pinned: torch.Tensor) -> None:
            if len(rest) < len(union):                               # (the probed frame is the smallest: row 0)
                pinned[0].copy_(probe[0])
            if rest:
                pinned[len(union) - len(rest):].copy_(read(rest))
        frames, _ready = staging.upload((len(union),) + tuple(probe.shape[1:]), fill, dev)
        return lambda table, out: model.forward_device(
            preprocess_indexed(frames, table, resize=tf.size, crop=tf.crop, scale_255=tf.scale_255, layout=model.packed_layout),
            out=out, layout=model.packed_layout)

    def host_clips(frames: torch.Tensor):
        chw = frames.permute(0, 3, 1, 2)
        return lambda table: torch.stack([tf(chw[row]) for row in table])
    samples = list(samples)
    return evaluate('eval_classification', model, samples, _by_directory(samples, t), frame_reader or read_frames, batch_clips,
                    return_logits, lambda rows: min(set().union(*rows)), stage, host_clips)


def main(annos: Mapping[str, str], data_root: str, out_json: str, model=None, checkpoint: Optional[str] = None,
         num_class: int = 12, data_prefix: Optional[str] = None, anno_col: int = 4, frame_reader: Optional[FrameReader] = None,
         batch_clips: Optional[int] = None, person_crop: bool = False, **model_kwargs) -> dict:
    """``scripts/eval_classification.py``: every split of ``annos`` = ``{split: annotation file}`` through
    ``eval_classification``; writes ``{split: {'correct', 'total', 'acc', 'overall', 'preds'}}`` to ``out_json`` and returns
    it.  Frame directories are ``data_root/data_prefix/frame_dir`` (datasets/common.py:66).  ``model``: anything
    ``eval_classification`` takes; None builds ``create_model(num_class, checkpoint=checkpoint, **model_kwargs)``.
    Every split is sampled deterministically and ``person_crop=True`` is refused (out of scope, module docstring)."""
    if person_crop:
        raise NotImplementedError('eval_classification runs the centre-crop test transform only: transform.person_crop of '
                                  "the reference's config is out of scope here (inference_dataset(person_crop=True) has it)")
    own = model is None
    if own:
        from .engine import create_model
        model = create_model(num_class=num_class, checkpoint=checkpoint, **model_kwargs)
    try:
        prefix = os.path.join(data_root, data_prefix if data_prefix else '')
        result = {split: eval_classification(model, load_annotation(path, prefix, anno_col), frame_reader, batch_clips)
                  for split, path in annos.items()}
    finally:
        if own:
            model.close()
    with open(out_json, 'w') as f:
        json.dump(result, f)
    return result
