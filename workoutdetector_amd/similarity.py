"""Frame embeddings and the temporal self-similarity matrix: the reference's classifier-free route to repetitions.

Counterpart of ``cnn_feature`` / ``video_feature`` / ``plot_sim`` (workoutdetector/utils/common.py:79-143): a ResNet with
``num_classes=0`` over every frame of a video, the pooled vector per frame, and the N x N cosine-distance matrix of those
vectors (``sklearn.metrics.pairwise_distances(feats, metric='cosine')``) -- the matrix RepNet-style counters read the period
from.  The heatmap, the commented-out row softmax and any period estimator are out of scope.

On a ``TsmEngine`` (``engine.create_feature_model``) the frames are staged once and every batch is three launches' worth of
host work: ONE ``tsm_preprocess`` launch, the forward -- whose pool launch writes the batch's rows straight into their band
of the [N, feature_dim] device buffer --, and for ``self_similarity`` ONE ``tsm_cosine_distances`` band launch.  Both
functions then return CUDA tensors; nothing crosses PCIe unless the caller asks.

Transform: the reference's is ``ToTensor -> Resize(224) -> Normalize`` with no crop, on whatever geometry a video has.  An
engine has one geometry, so the engine path is ``Resize(resize) -> CenterCrop(crop)`` (224 / 224 by default, values scaled
to [0, 1]) through ``tsm_preprocess``; a caller who wants the long side builds the engine with that height / width and feeds
``forward_features`` directly.  Any other model (a torch module or a callable ``model(x[n,3,H,W]) -> [n, feature_dim]``)
takes the CPU ``TestTransform`` of the same geometry and ``cosine_distances_host``.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import staging
from .transform import TestTransform, as_frames_u8, need_frame_engine


def cosine_distances_host(feats) -> np.ndarray:
    """scikit-learn's ``cosine_distances(X)`` restated in float64 NumPy (``pairwise_distances(X, metric='cosine')``):
    rows L2-normalised with a zero norm counted as 1 (``normalize``), ``S = Xn @ Xn.T``, ``D = 1 - S`` clipped to [0, 2],
    the diagonal set to 0 (X is Y).  feats [n, c] -> float64 [n, n]."""
    x = np.asarray(feats.detach().cpu().numpy() if isinstance(feats, torch.Tensor) else feats, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError(f'feats must be [n, c], got {x.shape}')
    norms = np.sqrt(np.einsum('ij,ij->i', x, x))
    norms[norms == 0.0] = 1.0
    xn = x / norms[:, None]
    d = 1.0 - xn @ xn.T
    np.clip(d, 0.0, 2.0, out=d)
    np.fill_diagonal(d, 0.0)
    return d


def _geometry(model):
    return int(getattr(model, 'image_resize', 224)), int(getattr(model, 'image_crop', 224))


def _engine_rows(model, frames: torch.Tensor, normalize: bool, batch_frames: Optional[int], dist: bool):
    """The engine path of both functions: (features [N, feature_dim], distances [N, N] or None), CUDA tensors."""
    from .engine import cosine_distances, preprocess_frames
    resize, crop = _geometry(model)
    need_frame_engine(model, crop, 'similarity', 'create_feature_model')
    dev = staging.engine_device(model)
    n = int(frames.shape[0])
    step = int(batch_frames) if batch_frames else model.max_clips
    if step <= 0:
        raise ValueError(f'batch_frames must be positive, got {batch_frames}')
    staged = frames.contiguous() if frames.is_cuda else staging.upload_table(frames, dev)   # once
    feats = torch.empty((n, model.feature_dim), dtype=torch.float32, device=dev)
    mat = torch.empty((n, n), dtype=torch.float32, device=dev) if dist else None
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        x = preprocess_frames(staged[lo:hi], resize=resize, crop=crop, scale_255=True, layout=model.packed_layout)
        model.forward_features(x.view((hi - lo, 1) + tuple(x.shape[1:])), normalize=normalize, out=feats[lo:hi],
                               layout=model.packed_layout)
        if dist:
            cosine_distances(feats, out=mat, rows=(lo, hi))
    return feats, mat


def _host_features(model, frames: torch.Tensor, batch_frames: Optional[int]) -> np.ndarray:
    resize, crop = _geometry(model)
    tf = TestTransform(resize, crop, scale_255=True)
    step = int(batch_frames) if batch_frames else 10          # (the reference's batch_size, utils/common.py:91)
    rows = []
    for lo in range(0, frames.shape[0], step):
        rows.append(staging.call_host_module(model, tf(frames[lo:lo + step].cpu().permute(0, 3, 1, 2))))
    return np.concatenate(rows).reshape(frames.shape[0], -1)


def video_features(model, frames_u8, normalize: bool = False, batch_frames: Optional[int] = None):
    """``video_feature`` (utils/common.py:109-130) from decoded frames on: uint8 frames [N, H, W, 3] (ndarray or tensor) ->
    float32 [N, feature_dim], one pooled vector per frame (``normalize``: each over its Euclidean norm).  A ``TsmEngine``
    returns a CUDA tensor (``batch_frames`` frames per forward, default the engine's ``max_clips``); any other model an
    ndarray."""
    frames = as_frames_u8(frames_u8)
    if staging.device_path(model):
        return _engine_rows(model, frames, normalize, batch_frames, dist=False)[0]
    feats = _host_features(model, frames, batch_frames)
    if normalize:
        norms = np.sqrt(np.einsum('ij,ij->i', feats.astype(np.float64), feats.astype(np.float64)))
        norms[norms == 0.0] = 1.0
        feats = (feats / norms[:, None]).astype(np.float32)
    return feats


def self_similarity(model, frames_u8, batch_frames: Optional[int] = None):
    """The temporal self-similarity matrix ``plot_sim`` draws (utils/common.py:133-134): uint8 frames [N, H, W, 3] ->
    [N, N] cosine distances of the frames' embeddings, symmetric, zero diagonal, values in [0, 2].  A ``TsmEngine`` returns a
    float32 CUDA tensor, built band by band as the batches come off the engine; any other model a float64 ndarray
    (``cosine_distances_host``)."""
    frames = as_frames_u8(frames_u8)
    if staging.device_path(model):
        return _engine_rows(model, frames, True, batch_frames, dist=True)[1]
    return cosine_distances_host(_host_features(model, frames, batch_frames))
