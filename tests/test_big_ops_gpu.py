"""The element-wise and reduction kernels on inputs past 2^32 bytes, by the periodic method of tests/test_big_conv_gpu.py: the
input is P frames (three clips) repeated R times, written straight into a guarded view; the output must repeat with the period
bit for bit (int32 words, compared on the device), and its first period meets the reference of the P frames alone at the bar
the small per-op test of that kernel uses -- bit-exact for the data-movement kernels.  The Python wrappers reach these kernels
in fp32 storage, so that is the format here; the period in bytes has an odd factor > 1 (frames of 7 x 9, 13 x 17 or 7 x 7, three
clips), so neither 2^31 nor 2^32 is a multiple of it.

(pack_input, from_f32 and to_f32 run on such sizes in test_big_conv_gpu.py, which asserts them from the trace.  The temporal
max-pool has no per-op entry point: tests/test_big_engine_gpu.py runs it inside a temporal_pool engine at B = 136.)"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import tsm_oracle
from tests._guard import check, guarded, guarded_out, guarded_repeat
from tests._util import assert_close, assert_periodic
from tests.test_conv_forms_gpu import _nchw, _nhwc

pytestmark = pytest.mark.gpu


def _past_2_32(t):
    assert t.numel() * t.element_size() > 1 << 32, (tuple(t.shape), t.numel() * t.element_size())
    return t


def _odd_factor(nbytes):
    while nbytes % 2 == 0:
        nbytes //= 2
    return nbytes > 1


def test_temporal_shift_past_2_32(hip_lib):
    """266 328 frames of 7 x 9 x 64 at T = 8: 1 073 834 496 elements in and out."""
    from workoutdetector_amd.engine import launch_trace, temporal_shift_nhwc
    T, P, R, c, h, w = 8, 24, 11097, 64, 7, 9
    assert _odd_factor(P * h * w * c * 4)
    x = torch.randn(P, c, h, w, generator=torch.Generator().manual_seed(1))
    try:
        xg = _past_2_32(guarded_repeat(_nhwc(x).cuda(), R, name='x'))
        y = guarded_out((P * R, h, w, c), name='y')
        with launch_trace() as tr:
            assert temporal_shift_nhwc(xg, T, 8, out=y) is y
        torch.cuda.synchronize()
        assert tr.kernels == ['temporal_shift_kernel'], tr.kernels
        check(xg, y)
        assert_periodic(y, R, 'temporal_shift')
        assert torch.equal(_nchw(y[:P].cpu()), tsm_oracle.temporal_shift(x, T, 8))
    finally:
        xg = y = None
        torch.cuda.empty_cache()


def test_maxpool_past_2_32(hip_lib):
    """75 918 frames of 13 x 17 x 64 (1 073 784 192 elements) -> 7 x 9: every last row and column window hangs over the edge."""
    from workoutdetector_amd.engine import launch_trace, maxpool3x3s2_nhwc
    P, R, c, h, w = 3, 25306, 64, 13, 17
    assert _odd_factor(P * h * w * c * 4)
    x = torch.randn(P, c, h, w, generator=torch.Generator().manual_seed(2))
    try:
        # (a max absorbs NaN and -inf: the input's bands are +inf, which no maximum survives)
        xg = _past_2_32(guarded_repeat(_nhwc(x).cuda(), R, fill=float('inf'), name='x'))
        y = guarded_out((P * R, 7, 9, c), name='y')
        with launch_trace() as tr:
            assert maxpool3x3s2_nhwc(xg, out=y) is y
        torch.cuda.synchronize()
        assert tr.kernels == ['maxpool3x3s2_kernel<kPrecF32>'], tr.kernels
        check(xg, y)
        assert_periodic(y, R, 'maxpool3x3s2')
        assert torch.equal(_nchw(y[:P].cpu()), F.max_pool2d(x, 3, 2, 1))
    finally:
        xg = y = None
        torch.cuda.empty_cache()


# ---- the heads and the feature pool: one feature tensor of 10 704 frames of 7 x 7 x 2048 (4 296 671 232 bytes) ------------------
HEAD_T, HEAD_P, HEAD_R, HEAD_C, HEAD_CLS = 4, 12, 892, 2048, 12


@pytest.fixture(scope='module')
def big_feat(hip_lib):
    g = torch.Generator().manual_seed(3)
    small = torch.randn(HEAD_P, 7, 7, HEAD_C, generator=g) * 3.0            # NHWC
    small[1] = 0.0                                                         # a zero frame: its unit row stays zero
    fc_w, fc_b = torch.randn(HEAD_CLS, HEAD_C, generator=g) * 0.05, torch.randn(HEAD_CLS, generator=g)
    assert _odd_factor(HEAD_P * 49 * HEAD_C * 4)
    feat = _past_2_32(guarded_repeat(small.cuda(), HEAD_R, name='feat'))
    ops = [feat, guarded(fc_w.cuda(), name='fc_w'), guarded(fc_b.cuda(), name='fc_b')]
    yield small, fc_w, fc_b, ops
    del feat, ops[:]
    torch.cuda.empty_cache()


def test_head_past_2_32(big_feat):
    from workoutdetector_amd.engine import head_nhwc, launch_trace
    small, fc_w, fc_b, ops = big_feat
    n_clips = HEAD_P * HEAD_R // HEAD_T
    out = guarded_out((n_clips, HEAD_CLS), name='logits')
    with launch_trace() as tr:
        assert head_nhwc(*ops, HEAD_T, out=out) is out
    torch.cuda.synchronize()
    assert tr.kernels == ['head_pool_kernel<kPrecF32>', 'head_fc_kernel'], tr.kernels
    check(out, *ops)
    assert_periodic(out, HEAD_R, 'head')
    want = tsm_oracle.head(_nchw(small), {'fc.weight': fc_w, 'fc.bias': fc_b}, HEAD_T)
    assert_close(out[:HEAD_P // HEAD_T].cpu().numpy(), want.numpy(), rtol=1e-4, atol_scale=1e-5, what='head')


def test_head_segments_past_2_32(big_feat):
    from workoutdetector_amd.engine import head_segments_nhwc, launch_trace
    small, fc_w, fc_b, ops = big_feat
    out = guarded_out((HEAD_P * HEAD_R, HEAD_CLS), name='logits')
    with launch_trace() as tr:
        assert head_segments_nhwc(*ops, out=out) is out
    torch.cuda.synchronize()
    assert tr.kernels == ['head_seg_kernel<kPrecF32>'], tr.kernels
    check(out, *ops)
    assert_periodic(out, HEAD_R, 'head_segments')
    want = F.linear(small.reshape(HEAD_P, 49, HEAD_C).mean(1), fc_w, fc_b)
    assert_close(out[:HEAD_P].cpu().numpy(), want.numpy(), rtol=1e-4, atol_scale=1e-5, what='head_segments')


def test_pool_features_past_2_32(big_feat):
    from workoutdetector_amd.engine import head_segments_nhwc, launch_trace, pool_features_nhwc
    small, _, _, ops = big_feat
    n = HEAD_P * HEAD_R
    pooled, unit = guarded_out((n, HEAD_C), name='pooled'), guarded_out((n, HEAD_C), name='unit')
    with launch_trace() as tr:
        pool_features_nhwc(ops[0], out=pooled, out_unit=unit)
    torch.cuda.synchronize()
    assert tr.kernels == ['pool_feat_kernel<kPrecF32>'], tr.kernels
    check(ops[0], pooled, unit)
    assert_periodic(pooled, HEAD_R, 'pooled')
    assert_periodic(unit, HEAD_R, 'unit')
    # pooled: the heads' pooled value to the bit (an identity classifier returns it unchanged); unit: its float64 normalisation
    want_pooled = head_segments_nhwc(small.cuda(), torch.eye(HEAD_C).cuda(), torch.zeros(HEAD_C).cuda())
    assert torch.equal(pooled[:HEAD_P], want_pooled)
    p64 = want_pooled.cpu().numpy().astype(np.float64)
    norms = np.sqrt((p64 * p64).sum(1))
    norms[norms == 0.0] = 1.0
    u = unit[:HEAD_P].cpu().numpy()
    assert np.isfinite(u).all() and np.allclose(u, p64 / norms[:, None], rtol=1e-5, atol=0.0)
    assert not u[1].any(), 'the zero frame\'s unit row is not zero'
