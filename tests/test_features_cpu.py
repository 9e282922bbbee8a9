"""Frame embeddings and the self-similarity matrix without a GPU: the host reference against an independent formulation and
scikit-learn's edge rules, the ABI (symbols, NULL calls, every refusal before a launch), the non-engine path of
``similarity``, the built code object, and the distance bar proved with the reference alone (a NumPy restatement of the
kernels' float32 arithmetic against float64)."""
import numpy as np
import pytest
import torch

from tests import _features as ft
from workoutdetector_amd import similarity
from workoutdetector_amd.similarity import cosine_distances_host


@pytest.fixture(scope='module')
def lib():
    from workoutdetector_amd import _lib
    from workoutdetector_amd.build import build_library
    build_library()
    return _lib.load()


# ---- the host reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ft.KINDS)
@pytest.mark.parametrize('c', ft.WIDTHS)
def test_host_reference_against_an_independent_formulation(c, kind):
    """1 - u @ u.T with u = x / ||x|| written row by row in float64 (np.linalg.norm, np.dot per pair)."""
    x = ft.feature_rows(33, c, kind).astype(np.float64)
    n = x.shape[0]
    want = np.zeros((n, n))
    for i in range(n):
        for j in range(n):
            ni, nj = np.linalg.norm(x[i]) or 1.0, np.linalg.norm(x[j]) or 1.0
            want[i, j] = 0.0 if i == j else min(max(1.0 - float(np.dot(x[i] / ni, x[j] / nj)), 0.0), 2.0)
    got = cosine_distances_host(x)
    assert got.dtype == np.float64 and got.shape == (n, n)
    assert np.abs(got - want).max() <= 1e-12
    assert np.array_equal(got, got.T) and (np.diag(got) == 0).all() and got.min() >= 0.0 and got.max() <= 2.0


def test_host_reference_edge_rules():
    x = ft.feature_rows(16, 72)
    d = cosine_distances_host(x)
    z, a, b = ft.ZERO_ROW, ft.DUP_SRC, ft.DUP_DST
    off = np.arange(16) != z
    assert (d[z, off] == 1.0).all() and (d[off, z] == 1.0).all() and d[z, z] == 0.0      # a zero row: 1 to everything, 0 to itself
    assert d[a, b] <= 1e-15 and np.allclose(d[a], d[b], atol=1e-15)                      # a duplicated row
    assert (np.diag(d) == 0.0).all()
    opp = np.stack([x[0], -x[0], x[1]]).astype(np.float64)                               # the clip: 1 - (-1 - eps) stays <= 2
    e = cosine_distances_host(opp)
    assert e.max() <= 2.0 and abs(e[0, 1] - 2.0) <= 1e-12 and e.min() >= 0.0
    same = cosine_distances_host(np.stack([x[0], x[0] * 3.0]))                           # ... and 1 - (1 + eps) stays >= 0
    assert same.min() >= 0.0 and same[0, 1] <= 1e-15
    assert torch.is_tensor(torch.from_numpy(x)) and np.array_equal(cosine_distances_host(torch.from_numpy(x)), d)
    with pytest.raises(ValueError):
        cosine_distances_host(np.zeros(4))


# ---- ABI --------------------------------------------------------------------------------------------------------------------
NEW = ('tsm_forward_features', 'tsm_pool_features', 'tsm_cosine_distances')


def test_symbols_null_calls_and_abi_version(lib):
    from workoutdetector_amd import _lib
    assert all(s in _lib.EXPORTS and getattr(lib, s) is not None for s in NEW)
    assert lib.tsm_abi_version() == _lib.ABI_VERSION == 7
    assert lib.tsm_forward_features(None, None, 0, 0, 1, None, 0, None) == -1
    assert lib.tsm_pool_features(None, None, None, 1, 1, 8, None) == -1
    assert lib.tsm_cosine_distances(None, 1, 8, 0, 1, None, None) == -1
    assert lib.tsm_set_consensus(None, 2) == -1 and lib.tsm_set_consensus(None, 1) == -1     # as before: the NULL engine comes first


def test_every_refusal_comes_before_a_launch(lib):
    """No GPU here: a call that got as far as a launch would return TSM_ERR_HIP (-2).  The pointers are never dereferenced
    by a refused call, so any aligned non-NULL address will do."""
    p, q = 1 << 20, 2 << 20
    pool, dist = lib.tsm_pool_features, lib.tsm_cosine_distances
    assert pool(p, None, None, 2, 4, 512, None) == -1 and b'pool_features' in lib.tsm_last_error(None)   # both outputs NULL
    assert pool(None, q, q, 2, 4, 512, None) == -1
    assert pool(p, q, None, 0, 4, 512, None) == -1 and pool(p, q, None, 2, 0, 512, None) == -1 and pool(p, q, None, 2, 4, 0, None) == -1
    assert pool(p + 4, q, None, 2, 4, 512, None) == -1 and pool(p, None, q + 8, 2, 4, 512, None) == -1     # alignment
    assert pool(p, q, None, 2, 4, 4096, None) == -7 and b'2048' in lib.tsm_last_error(None)
    assert pool(p, None, q, 2, 4, 12, None) == -7
    assert dist(None, 4, 8, 0, 4, q, None) == -1 and dist(p, 4, 8, 0, 4, None, None) == -1
    assert dist(p, 4, 8, -1, 4, q, None) == -1          # row0 < 0
    assert dist(p, 4, 8, 2, 2, q, None) == -1           # row0 >= row1
    assert dist(p, 4, 8, 3, 2, q, None) == -1
    assert dist(p, 4, 8, 0, 5, q, None) == -1           # row1 > n_total
    assert dist(p, 4, 0, 0, 4, q, None) == -1 and dist(p, 4, -8, 0, 4, q, None) == -1      # c <= 0
    assert dist(p + 4, 4, 8, 0, 4, q, None) == -1
    assert dist(p, 4, 12, 0, 4, q, None) == -7 and b'multiple of 8' in lib.tsm_last_error(None)
    assert dist(p, 4, 4, 0, 4, q, None) == -7


def test_header_documents_the_three_entry_points():
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'tsm_hip.h')).read()
    for s in NEW:
        assert text.count(s) >= 2, s             # the table at the top and the declaration
    assert 'utils/common.py:79-116' in text and 'utils/common.py:118-143' in text


# ---- pipelines on a non-engine model ---------------------------------------------------------------------------------------
class _Stub:
    """A `model(x[n,3,H,W]) -> [n, 6]` that is no TsmEngine: channel means and a few fixed pixels of the transformed frames."""

    def __init__(self):
        self.calls = []

    def __call__(self, x):
        self.calls.append(tuple(x.shape))
        return torch.cat([x.mean((2, 3)), x[:, :, 3, 5]], dim=1)


def test_non_engine_models_take_the_host_path():
    frames = ft.repeating_video(12, 5, 20, 28)
    stub = _Stub()
    feats = similarity.video_features(stub, frames, batch_frames=5)
    assert isinstance(feats, np.ndarray) and feats.dtype == np.float32 and feats.shape == (12, 6)
    assert stub.calls == [(5, 3, 224, 224), (5, 3, 224, 224), (2, 3, 224, 224)]
    assert np.array_equal(feats[0], feats[5]) and not np.array_equal(feats[0], feats[1])
    unit = similarity.video_features(stub, frames, normalize=True)
    assert np.allclose(np.linalg.norm(unit.astype(np.float64), axis=1), 1.0, atol=1e-6)
    d = similarity.self_similarity(stub, torch.from_numpy(frames), batch_frames=12)
    assert isinstance(d, np.ndarray) and d.dtype == np.float64 and d.shape == (12, 12)
    assert np.array_equal(d, cosine_distances_host(feats)) and np.array_equal(d, d.T)
    assert d[0, 5] <= 1e-12 and d[1, 11] <= 1e-12 and d[0, 1] > 0
    stub.image_resize, stub.image_crop = 32, 24                  # the geometry attributes create_feature_model records
    assert similarity.video_features(stub, frames).shape == (12, 6) and stub.calls[-1][1:] == (3, 24, 24)
    with pytest.raises(ValueError):
        similarity.video_features(stub, frames.astype(np.float32))


def test_create_feature_model_has_no_cpu_path():
    from workoutdetector_amd.engine import create_feature_model
    with pytest.raises(RuntimeError):
        create_feature_model(device='cpu')
    with pytest.raises(NotImplementedError):
        create_feature_model(base_model='resnet101')
    with pytest.raises(ValueError):
        create_feature_model(resize=64, crop=224)


# ---- code object ---------------------------------------------------------------------------------------------------------------
def test_new_kernels_in_the_code_object():
    from workoutdetector_amd import codeobj
    from workoutdetector_amd.build import build_library
    md = codeobj.kernel_metadata(build_library())
    for name in ('pool_feat_kernel<0>', 'pool_feat_kernel<1>', 'pool_feat_kernel<2>', 'cosine_dist_kernel'):
        assert name in md, f'{name} not in the code object'
        r = md[name]
        assert r['.wavefront_size'] == 64 and not r['.uses_dynamic_stack'], name
        assert r['.private_segment_fixed_size'] == 0 and r['.vgpr_spill_count'] == 0, name
        assert r['.group_segment_fixed_size'] <= 64 * 1024 and r['.max_flat_workgroup_size'] == 256, name


# ---- the distance bar, from the reference alone --------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ft.KINDS)
@pytest.mark.parametrize('c', ft.WIDTHS)
def test_float32_chain_stays_within_the_distance_bar(capsys, c, kind):
    """The kernels' arithmetic in NumPy float32 (sequential sum of squares, sqrt, divide, sequential dot over ascending k,
    1 - s) against float64 on the GPU test's inputs: the bar holds with a wide margin for the reference alone.  Maxima over
    both kinds and both ways of making the unit rows at n = 97: c = 8: 1.9e-7, 72: 2.5e-7, 512: 3.0e-7, 2048: 7.8e-7
    (DESIGN 4.17)."""
    x = ft.feature_rows(ft.N_ROWS, c, kind)
    want = cosine_distances_host(x)
    sim = ft.simulate_kernel_distances(ft.simulate_kernel_unit(x))
    err = float(np.abs(sim.astype(np.float64) - want).max())
    host_units = ft.simulate_kernel_distances(ft.unit_rows_host(x))           # what the per-op GPU test feeds the kernel
    err2 = float(np.abs(host_units.astype(np.float64) - want).max())
    with capsys.disabled():
        print(f'\n[fp32 chain c={c} {kind}] max|err| {err:.3g} (unit rows from the float32 chain), {err2:.3g} (from the host)')
    assert max(err, err2) <= ft.DIST_BAR
    assert np.array_equal(sim, sim.T) and (np.diag(sim) == 0).all()
    assert sim[ft.ZERO_ROW, 0] == 1.0 and sim[ft.DUP_SRC, ft.DUP_DST] <= ft.DIST_BAR
