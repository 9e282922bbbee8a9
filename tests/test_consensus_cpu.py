"""consensus_type='identity' without a GPU: the factory, the ABI symbols, the per-segment reference the GPU tests use, the
reference's executed SegmentConsensus('identity'), and the pipelines' up-front refusal."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import tsm_oracle
from tests import _consensus as cs
from tests._util import BF16_E2E_BAR, assert_close, make_input


@pytest.fixture(scope='module')
def lib():
    from workoutdetector_amd import _lib
    from workoutdetector_amd.build import build_library
    build_library()
    return _lib.load()


# ---- factory ------------------------------------------------------------------------------------------------------------
def test_factory_accepts_identity_and_reaches_the_device_check():
    """'identity' passes the reference's assert (tsm.py:438) and fails where 'avg' fails on a CPU: no CPU path."""
    from workoutdetector_amd.engine import create_model
    for consensus in ('avg', 'identity'):
        with pytest.raises(RuntimeError, match='no CPU path'):
            create_model(num_class=12, consensus_type=consensus, device='cpu')


@pytest.mark.parametrize('consensus', ['rnn', 'max', '', 'AVG'])
def test_factory_refuses_other_consensus_types_like_the_reference(consensus):
    from workoutdetector_amd.engine import create_model
    with pytest.raises(AssertionError):
        create_model(num_class=12, consensus_type=consensus, device='cpu')


def test_engine_refuses_other_consensus_types_before_loading_anything():
    from workoutdetector_amd.engine import TsmEngine
    with pytest.raises(ValueError, match='consensus_type'):
        TsmEngine(consensus_type='rnn')


def test_out_shape_is_the_one_place():
    """_out_shape / get_outputs of both kinds, on an engine object that never touched the library."""
    from workoutdetector_amd.engine import TsmEngine
    eng = TsmEngine.__new__(TsmEngine)
    eng.num_class, eng.num_segments, eng._h = 12, 8, None
    eng.consensus_type = 'avg'
    assert eng._out_shape(5) == (5, 12) and eng.get_outputs()[0].shape == [None, 12]
    eng.consensus_type = 'identity'
    assert eng._out_shape(5) == (5, 8, 12) and eng.get_outputs()[0].shape == [None, 8, 12]


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_and_null_engine(lib):
    from workoutdetector_amd import _lib
    assert 'tsm_set_consensus' in _lib.EXPORTS and 'tsm_head_segments' in _lib.EXPORTS
    assert lib.tsm_set_consensus(None, 1) == -1          # TSM_ERR_INVALID_ARG
    assert lib.tsm_set_consensus(None, 7) == -1          # (the NULL engine comes first)
    assert lib.tsm_head_segments(None, None, None, None, 1, 1, 512, 12, None) == -1
    assert lib.tsm_abi_version() == 7
    assert ctypes.sizeof(_lib.TsmConfig) == 40


# ---- the per-segment reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('t', [4, 8])
@pytest.mark.parametrize('place', cs.PLACES)
@pytest.mark.parametrize('base_model', cs.BASE_MODELS)
def test_reference_mean_is_the_oracle_forward(base_model, place, t):
    """ref.mean(1) == tsm_oracle.forward to fp32 round-off (the oracle's head IS linear-then-mean), fp32 and bf16-storage."""
    _, sdt = cs.state_dict(base_model, place)
    x = make_input(5 + t, 2, t, 64, 64)
    for bf16 in (False, True):
        ref = cs.per_segment_reference(sdt, x, base_model, place, bf16, n_segment=t)
        assert tuple(ref.shape) == (2, t, cs.NUM_CLASS)
        want = tsm_oracle.forward(sdt, torch.from_numpy(x), base_model, place, bf16, n_segment=t)
        assert_close(ref.mean(1).numpy(), want.numpy(), rtol=1e-6, atol_scale=1e-6, what=f'{base_model} {place} T{t} bf16={bf16}')


def test_reference_identity_consensus_vectors(golden_dir):
    """The reference's executed SegmentConsensus('identity') + squeeze(1) on [B, T, C]: the per-frame fc rows of the fixture,
    [B*T, C] as ``self.fc`` returns them, go through the helper's own layout step (the one per_segment_reference ends with) and
    must come out as the executed reference's output -- a helper that grouped frames by segment instead of by clip, or
    averaged, fails here."""
    z = np.load(f'{golden_dir}/ref_consensus_identity.npz')
    n = len(z.files) // 2
    assert n >= 4
    for i in range(n):
        x, y = z[f'x{i}'], z[f'y{i}']
        b, t, c = x.shape
        rows = torch.from_numpy(np.ascontiguousarray(x.reshape(b * t, c)))       # what fc returns: frame f = clip f // t, segment f % t
        got = cs.rows_to_segments(rows, t).numpy()
        assert got.shape == y.shape == (b, t, c) and np.array_equal(got, y)


@pytest.mark.parametrize('place', cs.PLACES)
@pytest.mark.parametrize('base_model', cs.BASE_MODELS)
def test_argmax_cap_holds_for_the_reference_alone(base_model, place):
    """The GPU tests assert arg-max equality on decided rows only and cap the undecided ones at one in eight: the seeds of
    tests/_consensus.py must meet that cap with the ORACLE alone, at the fp32 bar and at the bf16 bar."""
    _, sdt = cs.state_dict(base_model, place)
    x = cs.case_input(base_model, place)
    for bf16, bar in ((False, cs.F32_BAR), (True, BF16_E2E_BAR)):
        ref = cs.per_segment_reference(sdt, x, base_model, place, bf16).numpy()
        cs.assert_argmax(ref, ref, bar, f'{base_model} {place} bf16={bf16}')


# ---- pipelines --------------------------------------------------------------------------------------------------------------
class _PerSegmentModel:
    consensus_type = 'identity'


def test_pipelines_refuse_per_segment_models_up_front(tmp_path):
    from workoutdetector_amd import distributed as tdist
    from workoutdetector_amd.inference_count import count_by_video_model, inference_dataset, inference_video
    from workoutdetector_amd.streaming import StreamBatcher
    m = _PerSegmentModel()
    with pytest.raises(ValueError, match='consensus_type'):
        inference_video(m, np.zeros((8, 3, 4, 4), np.float32), transform=lambda v: v)
    with pytest.raises(ValueError, match='consensus_type'):
        inference_dataset(m, ['test'], str(tmp_path / 'out'), 'ckpt')
    assert not (tmp_path / 'out').exists(), 'refused before anything was created'
    with pytest.raises(ValueError, match='consensus_type'):
        count_by_video_model(m, iter([np.zeros((4, 4, 3), np.uint8)] * 8))
    with pytest.raises(ValueError, match='consensus_type'):
        StreamBatcher(m)
    with pytest.raises(ValueError, match='consensus_type'):
        tdist.gather_clip_logits(torch.zeros(3, 8, 12), 3)


def test_pipelines_still_take_models_without_the_attribute():
    from tests._stub import StubModel
    from workoutdetector_amd import distributed as tdist
    from workoutdetector_amd.inference_count import need_clip_rows
    from workoutdetector_amd.streaming import StreamBatcher
    need_clip_rows(StubModel(), 'test')
    StreamBatcher(StubModel())
    assert tuple(tdist.gather_clip_logits(torch.zeros(3, 12), 3).shape) == (3, 12)
