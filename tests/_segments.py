"""Shared by the segment-evaluation tests (CPU and GPU): the deterministic frame sampling of the reference's FrameDataset and
the centre-crop test transform of its sampled frames, written out independently of the product.

    numbers = sample(total, 8, start)                 datasets/transform.py:16-65, random=False
    clip    = test_transform(frames[numbers])         oracle/transform_oracle.py (build_test_transform(person_crop=False))

Everything runs on the CPU.  ``reference`` is computed once per (video, table, geometry) and shared between the tests that
need it; callers must not write into what it returns.
"""
import functools

import numpy as np
import torch

from oracle import transform_oracle

MEAN = torch.tensor([0.485, 0.456, 0.406], dtype=torch.float32)
STD = torch.tensor([0.229, 0.224, 0.225], dtype=torch.float32)
ZERO = (0.0 - MEAN) / STD                      # what a zero pixel becomes, per channel


def video(seed, total, h, w):
    """uint8 [total, h, w, 3] noise: every pixel differs from its neighbours, so a tap one pixel (or one frame) off shows."""
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, size=(total, h, w, 3), dtype=np.uint8))


def sample(total, num, offset=0):
    """The first frame of each of `num` equal intervals of a segment, every frame repeated ceil(num / total) times first
    when the segment is shorter than `num` -- NumPy, not the product's list arithmetic."""
    data = np.arange(total)
    if total < num:
        data = np.repeat(data, -(-num // total))
    return (data[::len(data) // num][:num] + offset).tolist()


@functools.lru_cache(maxsize=None)
def reference(seed, total, h, w, table, size, crop, scale_255):
    """[n_clips, n_segment, 3, crop, crop]: clip c = the test transform of ``video(seed, total, h, w)[table[c]]``; `table` is
    a tuple of tuples of frame numbers inside the video."""
    vid = video(seed, total, h, w)
    return torch.stack([transform_oracle.test_transform(vid[list(row)].permute(0, 3, 1, 2).float(), size, crop, scale_255)
                        for row in table])


def tally(preds, labels, num_class):
    """(correct, total) per class as plain loops: a label outside [0, num_class) is counted nowhere."""
    correct, total = [0] * num_class, [0] * num_class
    for p, l in zip(preds, labels):
        if 0 <= l < num_class:
            total[l] += 1
            correct[l] += int(p == l)
    return correct, total
