"""Shared by the image-path tests (CPU and GPU): the Pillow fixtures of tests/golden/ref_image_transform.npz, the normalised
value NumPy computes from Pillow's uint8, and the reference's voting loop transcribed literally.  Everything here is computed
once and shared; callers must not write into what these functions return."""
import functools
import os
from collections import deque

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_image_transform.npz')
CASES = ('landscape', 'portrait', 'upscale', 'vskip', 'tall', 'constant')
MEAN = np.float32([0.485, 0.456, 0.406])
STD = np.float32([0.229, 0.224, 0.225])


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(frames uint8 [3,H,W,3], want uint8 [3,crop,crop,3], resize, crop) of one case."""
    z = np.load(GOLDEN)
    frames, want = z[name + '_frames'], z[name + '_want']
    resize, crop = (int(v) for v in z[name + '_geom'])
    for a in (frames, want):
        a.setflags(write=False)
    return frames, want, resize, crop


def normalised(u8):
    """((u8 / 255) - mean) / std in NumPy fp32, [..., 3] -> [..., 3]: three correctly rounded fp32 operations."""
    x = u8.astype(np.float32) / np.float32(255.0)
    return ((x - MEAN) / STD).astype(np.float32)


def ulps(got, want):
    """|got - want| in units of fp32 spacing at |want| (float64 array)."""
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)


def reference_vote(preds):
    """utils/inference_count.py:221-231, literally: a deque of 7, ``states.append(sum(que) >= 4)``."""
    que = deque(maxlen=7)
    states = []
    for p in preds:
        que.append(int(p))
        states.append(int(sum(que) >= 4))
    return states


def logits_with_ties(seed, n, c):
    """float32 [n, c] noise with exact ties planted: every third row has its maximum twice (the FIRST must win), every
    seventh row is constant."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, c)).astype(np.float32)
    for i in range(0, n, 3):
        j = int(x[i].argmax())
        x[i, (j + 1 + i) % c if c > 1 else j] = x[i, j]
    x[::7] = x[::7, :1]
    return x
