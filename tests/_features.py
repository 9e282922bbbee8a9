"""Shared pieces of the frame-embedding / self-similarity tests (tests/test_features_cpu.py, tests/test_features_gpu.py).

* ``feature_rows``: the seeded rows both files use (Gaussian or ReLU-like, one all-zero row, one duplicated row).
* ``simulate_kernel_distances``: the arithmetic of pool_feat_kernel's phase 2 / 3 and cosine_dist_kernel restated in NumPy
  float32 -- a sequential sum of squares, sqrt, a divide, a sequential dot over ascending k, 1 - s, the clip and the zero
  diagonal.  The CPU test holds it to the distance bar against float64, which proves the bar with the reference alone.
* ``pooled_reference``: the mean over HW of the oracle's last block output (read-only use of oracle.tsm_oracle, as
  tests/_consensus.py).
* ``repeating_video``: the 40-frame pattern video of the end-to-end test.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import tsm_oracle

DIST_BAR = 1e-5               # absolute, on the [0, 2] scale: ~10x the fp32 chain's own error, 4 orders below an indexing bug
N_ROWS = 97
WIDTHS = (8, 72, 512, 2048)
KINDS = ('gauss', 'relu')
KIND_OF = {8: 'gauss', 72: 'relu', 512: 'gauss', 2048: 'relu'}     # the kind the GPU test uses per width (the CPU test runs both)
ZERO_ROW, DUP_SRC, DUP_DST = 3, 5, 11     # row 3 is all-zero, row 11 repeats row 5 (both exist from n = 12 on)
BANDS = (((0, 5), (5, 40), (40, None)), ((0, 32), (32, None)), ((0, 64), (64, None)))     # None = n; the last: the kernel's own 64-row tile edge
SENTINEL = -7.0               # no distance: they lie in [0, 2]


def feature_rows(n, c, kind='gauss', seed=0):
    """float32 [n, c]: seeded rows standing in for pooled features -- Gaussian, or ReLU-like (non-negative, about half
    zeros: what a ResNet's pooled vector looks like); from n = 12 on with one all-zero row and one duplicated row."""
    rng = np.random.default_rng(1000 * c + 10 * n + seed + (1 if kind == 'relu' else 0))
    x = rng.standard_normal((n, c))
    if kind == 'relu':
        x = np.maximum(x, 0.0) * rng.uniform(0.2, 3.0, size=(n, 1))
    x = x.astype(np.float32)
    if n > DUP_DST:
        x[ZERO_ROW] = 0.0
        x[DUP_DST] = x[DUP_SRC]
    return x


def unit_rows_host(rows):
    """float32 unit rows made on the host: the float64 normalisation (a zero norm counts as 1) rounded once."""
    x = np.asarray(rows, dtype=np.float64)
    norms = np.sqrt((x * x).sum(1))
    norms[norms == 0.0] = 1.0
    return (x / norms[:, None]).astype(np.float32)


def simulate_kernel_unit(rows):
    """pool_feat_kernel's phase 2 / 3 in float32: ss summed sequentially over ascending k, sqrt, 0 -> 1, one divide per element."""
    x = np.asarray(rows, dtype=np.float32)
    ss = np.zeros(x.shape[0], dtype=np.float32)
    for k in range(x.shape[1]):
        ss = ss + x[:, k] * x[:, k]
    norm = np.sqrt(ss)
    norm[norm == 0.0] = np.float32(1.0)
    return x / norm[:, None]


def simulate_kernel_distances(unit):
    """cosine_dist_kernel in float32: per element one sequential dot over ascending k, 1 - s, clip to [0, 2], zero diagonal."""
    u = np.asarray(unit, dtype=np.float32)
    s = np.zeros((u.shape[0], u.shape[0]), dtype=np.float32)
    for k in range(u.shape[1]):
        s = s + u[:, k, None] * u[None, :, k]
    d = np.clip(np.float32(1.0) - s, np.float32(0.0), np.float32(2.0))
    np.fill_diagonal(d, 0.0)
    return d


def band_list(bands, n):
    return [(lo, n if hi is None else hi) for lo, hi in bands if lo < n]


def region_mask(n, row0, row1):
    """Boolean [n, n]: what one band call may write -- i in [row0, row1), j in [0, row1), and the mirror."""
    i = np.arange(n)
    band, valid = (i >= row0) & (i < row1), i < row1
    return (band[:, None] & valid[None, :]) | (valid[:, None] & band[None, :])


@torch.no_grad()
def pooled_reference(sdt, x, base_model='resnet50', place='blockres', bf16=False, n_segment=8, is_shift=True):
    """x [B,T,3,H,W] (ndarray or tensor) -> [B*T, feat_dim] float32 ndarray: the mean over HW of the oracle's last block
    output -- what a ``num_classes=0`` model returns per frame."""
    x = torch.as_tensor(x)
    feat = tsm_oracle.trunk(x.reshape((-1,) + tuple(x.shape[2:])).to(torch.float32), sdt, n_segment, is_shift=is_shift,
                            base_model=base_model, shift_place=place, bf16=bf16)
    return F.adaptive_avg_pool2d(feat, 1).flatten(1).numpy()


def repeating_video(n_frames=40, period=5, h=48, w=64, seed=3):
    """uint8 [n_frames, h, w, 3]: `period` distinct random frames (smooth blobs on noise) repeated: frame i == frame i + period."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, size=(period, h, w, 3), dtype=np.uint8)
    ramp = (np.arange(w, dtype=np.int64)[None, None, :, None] * np.arange(1, period + 1)[:, None, None, None] * 3) % 256
    base = ((base.astype(np.int64) + ramp) // 2).astype(np.uint8)
    return np.ascontiguousarray(np.tile(base, (n_frames // period + 1, 1, 1, 1))[:n_frames])
