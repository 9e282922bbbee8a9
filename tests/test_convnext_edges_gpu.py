"""The ConvNeXt kernels (csrc/tsm_convnext.hip) where tests/test_convnext_gpu.py's small frames and seeded weights do not reach,
through the same engine taps.  tests/test_convnext_cases_cpu.py holds every precondition: what the frames below cover, and that
each crafted case tells the documented arithmetic from its near misses.

A. tile walks.  176 x 224 (maps 44 x 56, 22 x 28, 11 x 14, 5 x 7) is the smallest frame at which every accumulator of
   dwconv7_ln_kernel's tile takes every one of its 49 taps from inside the frame in all four widths, with interior tiles at
   C = 128 .. 512; 176 x 176 leaves workgroups at C = 128 and C = 512 that hold tiles of two frames.
B. LayerNorm.  Crafted state dicts on 64 x 64: a small signal (variance around eps: pins 1e-6), a common offset (pins the two
   passes), dead rows (zero variance: eps keeps them finite, and nothing but norm.bias comes out).
C. GELU on 7 680 chosen inputs against the float64 exact GELU near ulp level.
Shallow engines, depths (1, 1, 2, 1); no frame larger than 176 x 224, no batch of more than two."""
import numpy as np
import pytest

from tests import _convnext as cn
from tests import _convnext_cases as cc
from tests._util import assert_close
from tests.test_convnext_gpu import NUM_CLASS, OP_BAR, SHALLOW, _bits, _engine, _sd

pytestmark = pytest.mark.gpu

DWLN_TAPS = tuple(f'stages.{s}.blocks.0.dwln' for s in range(4))


class _Taps:
    """The taps of one input through one engine, each fetched once."""

    def __init__(self, eng, x):
        self.eng, self.x, self.got = eng, x, {}

    def __call__(self, name):
        if name not in self.got:
            self.got[name] = self.eng.forward_tap(self.x, name)
        return self.got[name]


# ---- A. tile walks ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def wide_engine(hip_lib):
    eng = _engine(176, 224, max_clips=2)
    yield eng
    eng.close()


def test_every_operator_at_176x224_against_float64_from_the_tap_in_front_of_it(wide_engine, capsys):
    """The per-operator walk of test_convnext_gpu.py at 176 x 224, two frames of noise, at its bar: the production map widths 56,
    28, 14 and 7 with the ragged heights 11 (two tiles + 3) and 5 (two tiles + 1)."""
    x, tap, worst = cc.noise(176, 224), _Taps(wide_engine, cc.noise(176, 224)), {}
    for name, what, want in cc.operator_cases(_sd(SHALLOW), SHALLOW, x, tap):
        worst[what] = max(worst.get(what, 0.0), assert_close(tap(name), want, what=f'{name} ({what}) at 176x224', **OP_BAR))
    assert [tap(t).shape[1:3] for t in DWLN_TAPS] == [(44, 56), (22, 28), (11, 14), (5, 7)]
    with capsys.disabled():
        print('\n[convnext per-op 176x224] max|err|/scale: ' + ', '.join(f'{k} {v:.2g}' for k, v in worst.items()))


def test_a_frame_does_not_depend_on_its_batch_at_176x176(hip_lib):
    """A pair of frames against each alone, bit for bit: the .dwln tap of every stage and the logits.  176 x 176: 121 tiles per
    frame at C = 128 (8 lane groups per workgroup) and 9 at C = 512 (2), so workgroups of both widths hold tiles of two frames."""
    x = cc.noise(176, 176)
    eng = _engine(176, 176, max_clips=2)
    try:
        pair = eng.forward_host(x)
        alone = np.concatenate([eng.forward_host(x[i:i + 1]) for i in range(2)])
        assert pair.shape == (2, NUM_CLASS) and np.array_equal(_bits(pair), _bits(alone)) and not np.array_equal(pair[0], pair[1])
        for name in DWLN_TAPS:
            both = eng.forward_tap(x, name)
            for i in range(2):
                assert np.array_equal(_bits(both[i:i + 1]), _bits(eng.forward_tap(x[i:i + 1], name))), (name, i)
    finally:
        eng.close()


def test_poisoned_equals_plain_at_176x224(wide_engine):
    """TSM_POISON=1 (every buffer between poisoned bands that are verified behind the forward -- a guard error would raise -- and
    the workspace poisoned in front of it): logits and one .dwln tap per width equal the plain engine's bit for bit, so edge tiles
    and the dead lane group behind the last tile store nothing outside the map and read nothing they did not write."""
    x = cc.noise(176, 224)
    eng = _engine(176, 224, max_clips=2, poison=True)
    try:
        got = {name: eng.forward_tap(x, name) for name in DWLN_TAPS}
        got['logits'] = eng.forward_host(x)
    finally:
        eng.close()
    for name, v in got.items():
        plain = wide_engine.forward_host(x) if name == 'logits' else wide_engine.forward_tap(x, name)
        assert np.array_equal(_bits(v), _bits(plain)), name


# ---- B. LayerNorm ---------------------------------------------------------------------------------------------------------------
def _ln_outputs_against_float64(sd, only=None):
    """Every operator of the walk that holds a LayerNorm (``only``: these taps), on two 64 x 64 frames of noise through an engine
    of ``sd``: {tap: max|err| / scale}, each asserted at the per-op bar."""
    x = cc.noise(64, 64)
    eng = _engine(64, 64, max_clips=2, sd=sd)
    try:
        tap, worst = _Taps(eng, x), {}
        for name, what, want in cc.operator_cases(sd, SHALLOW, x, tap):
            if what in cc.LN_OPERATORS and (only is None or name in only):
                worst[name] = assert_close(tap(name), want, what=f'{name} ({what})', **OP_BAR)
    finally:
        eng.close()
    return worst


def test_layer_norm_eps_on_a_small_signal(hip_lib, capsys):
    """cc.small_signal_sd: the channel variance in front of every LayerNorm is 0.25 .. 6.9 eps (asserted per site on the CPU), where
    eps = 1e-5, 0 or 2e-6 in the float64 model miss this bar 500 to 6 000 times and the float32 two-pass order uses 0.002 of it."""
    worst = _ln_outputs_against_float64(cc.small_signal_sd(_sd(SHALLOW), SHALLOW))
    assert len(worst) == 1 + sum(SHALLOW) + 3 + 1
    with capsys.disabled():
        print('\n[convnext small signal] max|err|/scale: ' + ', '.join(f'{k} {v:.2g}' for k, v in worst.items()))


@pytest.mark.parametrize('which', sorted(cc.OFFSET_DICTS))
def test_layer_norm_two_passes_under_a_common_offset(hip_lib, which, capsys):
    """cc.OFFSET_DICTS[which]: a common offset K in front of the named LayerNorms, a power of two per site at which the float32
    two-pass order stays under a quarter of this bar while a one-pass variance misses it 16 to 137 times (the CPU test's table)."""
    sites = cc.OFFSET_DICTS[which]
    worst = _ln_outputs_against_float64(cc.offset_dict(_sd(SHALLOW), which), only=set(sites))
    assert set(worst) == set(sites)
    with capsys.disabled():
        print(f'\n[convnext offset {which}] max|err|/scale: ' + ', '.join(f'{k} (K = {sites[k][1]}) {v:.2g}' for k, v in worst.items()))


def test_dead_rows_come_out_as_the_norm_bias_bit_for_bit(hip_lib):
    """conv_dw.weight = 0, conv_dw.bias = 0.75: every deviation is exactly 0, so .dwln is norm.bias in every pixel, to the bit, in
    all four widths -- finite only because eps is not 0."""
    sd = cc.dead_rows_sd(_sd(SHALLOW))
    x = cc.noise(64, 64)
    eng = _engine(64, 64, max_clips=2, sd=sd)
    try:
        got = {name: eng.forward_tap(x, name) for name in DWLN_TAPS}
    finally:
        eng.close()
    for s, name in enumerate(DWLN_TAPS):
        want = sd[f'stages.{s}.blocks.0.norm.bias']
        assert got[name].shape == (2,) + tuple(cc.maps(64, 64)[s]) + want.shape and np.isfinite(got[name]).all(), name
        assert (_bits(got[name]) == _bits(want)).all(), name


# ---- C. GELU ----------------------------------------------------------------------------------------------------------------------
def test_gelu_on_chosen_inputs_against_float64(hip_lib, capsys):
    """cc.gelu_sd: the first block of every stage holds chosen numbers in front of gelu_kernel, 4 C per stage, the same in every
    pixel: [-6, 6] densely, +-0, +-1e-30, +-8, +-12, +-40, +-1e4 and their power-of-two multiples.  Against the float64 exact GELU of
    those float32 inputs at |err| <= 3.62e-7 |want| + 1.72e-6 (cc.GELU_RTOL, cc.GELU_ATOL), four times what the kernel's own formula
    loses in float32 on the CPU: 4.30e-7 absolute over all inputs, 9.06e-8 relative over x >= 4 (tests/test_convnext_cases_cpu.py,
    where the tanh and the sigmoid form miss the bar 275 and 11 800 times).  x >= 1e4 comes out as x, x <= -40 and +-0 as a zero.
    Measured on an MI355X: max |err| 2.9e-7, 4.2e-7, 4.2e-7, 4.3e-7 in the four stages, 0.09 .. 0.12 of the bar."""
    sd = cc.gelu_sd(_sd(SHALLOW))
    x = cc.noise(64, 64)
    eng = _engine(64, 64, max_clips=2, sd=sd)
    try:
        got = {s: (eng.forward_tap(x, f'stages.{s}.blocks.0.dwln'), eng.forward_tap(x, f'stages.{s}.blocks.0.fc1')) for s in range(4)}
    finally:
        eng.close()
    worst, lines = {}, []
    for s, (dwln, fc1) in got.items():
        b, xs = cc.gelu_rows(s), cc.gelu_inputs(s)
        assert dwln.shape == (2,) + tuple(cc.maps(64, 64)[s]) + b.shape and fc1.shape == dwln.shape[:3] + xs.shape
        # .dwln is norm.bias to the bit (norm.weight = 0); a zero of either sign where the bias is one (0 * v + -0.0 is +0.0 for v > 0)
        zero = b == 0
        assert (_bits(dwln)[..., ~zero] == _bits(b)[~zero]).all() and (dwln[..., zero] == 0).all(), s
        assert (_bits(fc1) == _bits(fc1)[0, 0, 0]).all(), f'stage {s}: the pixels differ'
        y, want = fc1[0, 0, 0], cn.gelu(xs)
        worst[s] = cc.gelu_ratio(y, want)
        lines.append(f'stage {s}, {xs.size} inputs: max |err| {np.abs(y - want).max():.3g}, {worst[s]:.3g} of the bar')
        assert worst[s] <= 1.0, lines[-1]
        assert (xs >= 1e4).sum() == 2 and np.array_equal(y[xs >= 1e4], xs[xs >= 1e4])
        assert (xs <= -40).sum() == 6 and (y[xs <= -40] == 0).all() and (xs == 0).sum() == 8 and (y[xs == 0] == 0).all()
    with capsys.disabled():
        print('\n[convnext gelu] ' + '; '.join(lines))
