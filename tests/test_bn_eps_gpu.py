"""The BatchNorm eps of the TSM ResNet family on the MI355X: the small-variance cases of tests/_bn_cases.py, where eps = 1e-5 is a
tenth to ten times the variance under every root, through tsm_conv_op in hostile memory (tests/_guard.py) and through the engine
under TSM_POISON=1, against float64.  tests/test_bn_cases_cpu.py holds the preconditions: on these inputs a float32 implementation
uses under a tenth of every bar below, and eps = 1.1e-5 at any single fold site (the stem's bn1, the downsample BatchNorms, a
non-local W.1, layer4's last BatchNorm) misses the logits bar or the bar of the tap behind it at least 10 times over.

Bars, the project's existing ones: per op f32 1e-4 / 1e-4, bf16x3 3e-4 / 3e-4; engine logits rtol 1e-3 + 1e-5 of the scale, taps
rtol 1e-3 + 3e-5; the bf16 engine against the bf16-storage oracle at BF16_E2E_BAR (bf16_logits_report) and BF16_TAP_BAR."""
import re

import numpy as np
import pytest

from tests import _bn_cases as bc
from tests._guard import guarded_conv
from tests._util import BF16_TAP_BAR, assert_close, bf16_logits_report

pytestmark = pytest.mark.gpu

POISONED = {'TSM_POISON': '1'}


def _dual(trace):
    """The conv_igemm launches of the K-concatenated form: <..., PREC [| kPrecBlockShift], DUAL = true[, SEG = true]>."""
    return [k for k in trace.kernels if k.startswith('conv_igemm<') and re.search(r'kPrec[\w |]*, true(, true)?>', k)]


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


# ---- per op ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(bc.OP_CASES))
def test_conv_folds_small_variances_with_the_documented_eps(hip_lib, name):
    from workoutdetector_amd.engine import launch_trace
    op = bc.op_case(name)
    kw = {}
    if op['x2'] is not None:
        kw = dict(x2=_nhwc(op['x2']).cuda(), w2=op['w2'].cuda(), bn2=[b.cuda() for b in op['bn2']], stride2=op['stride2'])
    with launch_trace() as tr:
        got = guarded_conv(_nhwc(op['x']).cuda(), op['w'].cuda(), *[b.cuda() for b in op['bn']], stride=op['stride'], relu=True,
                           shift_segments=op['T'], fold_div=8, dtype=op['dtype'], **kw)
    assert not tr.ran('temporal_shift_kernel'), tr.kernels
    if name == 'stem bf16x3':           # the pair-packed fold goes with the direct stem
        assert tr.ran('stem_direct_kernel<'), tr.kernels
    elif name == 'conv3 + downsample':  # one K-concatenated GEMM
        assert _dual(tr), tr.kernels
    assert_close(got.cpu().permute(0, 3, 1, 2).numpy(), bc.op_reference(name), what=name, **bc.OP_BARS[op['dtype']])


# ---- the engine -------------------------------------------------------------------------------------------------------------------
def _assert_what_ran(case, tr):
    """The forms this geometry allows, as the tests of each form assert them: the pool-fused stem, no materialised shift, block
    placement's shifted-identity arm, a Bottleneck's conv3 + downsample GEMM, the five non-local attention launches."""
    assert tr.ran('stem_pool'), tr.kernels
    assert not tr.ran('temporal_shift_kernel'), tr.kernels
    igemm = [k for k in tr.kernels if k.startswith('conv_igemm<')]
    assert bool([k for k in igemm if 'kPrecBlockShift' in k]) == (case.place == 'block'), tr.kernels
    if case.base_model in (bc.R18, bc.R34) and case.place == 'blockres':
        assert any('KS = 3, SHIFT = true' in k for k in igemm), tr.kernels
    if case.base_model in (bc.R50, bc.WRN) and case.dtype != 'bf16':
        assert _dual(tr), tr.kernels
    if case.non_local:
        assert tr.count('nonlocal_attn_kernel<256>') == 2 and tr.count('nonlocal_attn_kernel<512>') == 3, tr.kernels
        assert tr.count('nonlocal_attn_kernel') == 5 and tr.count('maxpool2x2_kernel') == 5
    else:
        assert not tr.ran('nonlocal_attn_kernel'), tr.kernels


@pytest.mark.parametrize('case', bc.ENGINE_CASES, ids=repr)
def test_engine_folds_small_variances_with_the_documented_eps(hip_lib, capsys, case):
    from workoutdetector_amd.engine import launch_trace
    x = np.array(bc.clips(case.h, case.w))
    eng = bc.engine(case, POISONED)
    try:
        eng.run(None, {'input': x})                   # (the first forward of a bucket also runs the tuning pass)
        with launch_trace() as tr:
            got = eng.run(None, {'input': x})[0]
        _assert_what_ran(case, tr)
        assert got.shape == (bc.CLIPS, bc.NUM_CLASS) and got.dtype == np.float32
        if case.dtype == 'bf16':
            want16, taps16, want32 = bc.bf16_reference(case)
            bf16_logits_report(got, want16, want32, str(case), capsys)
            for name in case.taps:
                tap = eng.forward_tap(x, name)
                assert tap.shape == taps16[name].shape, name
                e = float(np.abs(tap - taps16[name]).max()) / float(np.abs(taps16[name]).max())
                assert e <= BF16_TAP_BAR, (str(case), name, e)
        else:
            logits, taps = bc.reference(case)
            assert_close(got, logits, what=f'{case} logits', **bc.LOGITS_BAR)
            for name in case.taps:
                assert_close(eng.forward_tap(x, name), taps[name], what=f'{case} {name}', **bc.TAP_BAR)
    finally:
        eng.close()


def test_small_variances_leave_the_tile_choice_bit_neutral(hip_lib):
    """The R50 f32 case tuned and with TSM_AUTOTUNE=0: logits and every tap bitwise equal -- the recipe leaves "the tile choice
    changes no bit" standing."""
    case = bc.TUNED_CASE
    x = np.array(bc.clips(case.h, case.w))
    out = {}
    for name, env in (('tuned', {'TSM_AUTOTUNE': '1'}), ('untuned', {'TSM_AUTOTUNE': '0'})):
        eng = bc.engine(case, env)
        try:
            if name == 'tuned':
                eng.warmup([bc.CLIPS])
                assert all(v != 'heuristic' for k, v in eng.conv_tiles(bc.CLIPS).items() if 'downsample' not in k and k != 'conv1')
            out[name] = [eng.run(None, {'input': x})[0]] + [eng.forward_tap(x, t) for t in case.taps]
        finally:
            eng.close()
    for a, b, what in zip(out['tuned'], out['untuned'], ('logits',) + case.taps):
        assert np.array_equal(a, b), what
    assert_close(out['tuned'][0], bc.reference(case)[0], what='tuned logits', **bc.LOGITS_BAR)
