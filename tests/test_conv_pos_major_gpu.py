"""The position-major form of the segmented fp32 3x3 launch (tile code bit 0x80, ConvParams::pos_major) per op, through
tsm_conv_op in hostile memory (tests/_guard.py), and in the engine under TSM_POISON=1.

A 64-row tile of the form is one output position of 64 frames, and the K-steps of a tap that is padding at that position are
never issued.  Every case sweeps the codes {3, 3 | 0x80} in both walk directions and asserts: the same bits from all four
launches; the float64 reference (tests/_conv_ref.py) at the per-op fp32 bar, rtol 1e-4 + 1e-4 of the scale; and from the
launch trace that conv_igemm<.., kPrecF32 | kPrecPosMajor, false, true> ran behind the bit and the natural instantiation
without it.

  A  cin 512 on 3x3 frames, N = 64: a K segment is one tap, so whole segments are skipped; the centre tile keeps all nine
  B  cin 256 on 2x5 frames, N = 128, cout 128: segment boundaries inside taps, no interior position, two tiles per position,
     two columns of tiles
  C  cin 128 at stride 2 on 6x6 (padding on one side) and 7x7 frames (on both)
  D  cin 128 and 512 on 1x1 frames: only the centre tap is live; at cin 128 its four steps straddle the boundary at step 18
  E  the tail split really applying (5 * n_cu * 7 / 5 tiles as tests/_k_cases.py's tail case): 3, 3 | TAILK, 3 | bit and
     3 | bit | TAILK bitwise equal, one reduction behind the split codes
  F  N = 8 and N = 72 with the bit set: the natural instantiation runs, same bits"""
import numpy as np
import pytest
import torch

from tests._conv_ref import conv_ref
from tests._guard import POISON, guarded_conv
from tests._util import make_input, sweep
from tests._walk_cases import tail_split_applies
from tests.test_conv_forms_gpu import _bn, _check, _nchw, _nhwc, _w

pytestmark = pytest.mark.gpu

POS, TAILK = 0x80, 0x200
POS_ARM = 'kPrecF32 | kPrecPosMajor, false, true>'
NATURAL_ARM = 'kPrecF32, false, true>'
KNOBS = ('TSM_AUTOTUNE', 'TSM_WALK', 'TSM_CONV_TILE', 'TSM_CONV_CODE', 'TSM_TUNE_CACHE', 'TSM_POISON', 'TSM_POS_MAJOR',
         'TSM_FUSE_CONV23')


def _launcher(x, w, bn, stride):
    from workoutdetector_amd.engine import launch_trace
    xd, wd, bnd = _nhwc(x).cuda(), w.cuda(), [b.cuda() for b in bn]

    def run(code, rev):
        with launch_trace() as tr:
            y = guarded_conv(xd, wd, *bnd, stride=stride, dtype='f32', code=code, reverse=rev, segmented=True)
        return _nchw(y.cpu()), tr
    return run


def _seg3x3(tr):
    """The trace lines of segmented 3x3 conv_igemm launches (launch_conv_seg's bracket has no RES)."""
    return [k for k in tr.kernels if k.startswith('conv_igemm<') and 'KS = 3, SHIFT = false]' in k and ', true>' in k]


def _expect(pos_applies, reduces=lambda code: 0):
    def expect(code, tr):
        lines = _seg3x3(tr)
        assert len(lines) == 1 and '[BM = 64, BN = 64, WGM = 2, WGN = 2,' in lines[0], (hex(code), tr.kernels)
        want = POS_ARM if (code & POS and pos_applies) else NATURAL_ARM
        assert want in lines[0], (hex(code), want, tr.kernels)
        n_red = sum(k.startswith(('splitk_reduce_kernel', 'splitk_reduce_pos_kernel')) for k in tr.kernels)
        assert n_red == reduces(code), (hex(code), tr.kernels)
        if reduces(code):
            assert tr.ran('splitk_reduce_pos_kernel') == bool(code & POS and pos_applies), (hex(code), tr.kernels)
    return expect


CASES = [  # id, cin, cout, n, hi, wi, stride
    ('A-512-3x3', 512, 64, 64, 3, 3, 1),
    ('B-256-2x5', 256, 128, 128, 2, 5, 1),
    ('C-128-s2-6x6', 128, 64, 64, 6, 6, 2),
    ('C-128-s2-7x7', 128, 64, 64, 7, 7, 2),
    ('D-128-1x1', 128, 64, 64, 1, 1, 1),
    ('D-512-1x1', 512, 64, 64, 1, 1, 1),
]


@pytest.mark.parametrize('name,cin,cout,n,hi,wi,stride', CASES, ids=[c[0] for c in CASES])
def test_position_major_equals_natural_order(hip_lib, name, cin, cout, n, hi, wi, stride):
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x, w, bn = torch.randn(n, cin, hi, wi, generator=g), _w(cout, cin, 3, g), _bn(cout, g)
    got = sweep([3, 3 | POS], _launcher(x, w, bn, stride), _expect(True))
    assert float((got != 0).float().mean()) > 0.2, f'{name}: the output is mostly zeros'
    _check(got.numpy(), conv_ref(x, w, bn, stride, True).numpy(), 'f32', name)


def test_position_major_with_the_tail_split(hip_lib):
    """E: cin 128, cout 256, N = 64: one whole round of 5 n_cu workgroups and 40 % of a second, so the tail split applies
    (asserted); whole tiles scatter their rows into y, the pieces' segment sums go through splitk_reduce_pos_kernel.  The four
    codes in both directions are compared bitwise with each other only (the other cases meet the float64 reference)."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    howo = 5 * n_cu * 7 // 5 // 4           # 4 columns of tiles, N = 64: one row of tiles per output position
    ho = max(d for d in range(1, int(howo ** 0.5) + 1) if howo % d == 0)
    wo = howo // ho
    assert tail_split_applies(64 * howo, 256, 2, n_cu), (n_cu, ho, wo)
    g = torch.Generator().manual_seed(97)
    x, w, bn = torch.randn(64, 128, ho, wo, generator=g), _w(256, 128, 3, g), _bn(256, g)
    got = sweep([3, 3 | TAILK, 3 | POS, 3 | POS | TAILK], _launcher(x, w, bn, 1), _expect(True, lambda code: 1 if code & TAILK else 0))
    assert float((got != 0).float().mean()) > 0.2


@pytest.mark.parametrize('n', [8, 72])
def test_frame_counts_off_64_run_in_natural_order(hip_lib, n):
    """F: the bit where pos_major_valid does not hold: the natural instantiation, the same bits."""
    g = torch.Generator().manual_seed(300 + n)
    x, w, bn = torch.randn(n, 128, 3, 5, generator=g), _w(64, 128, 3, g), _bn(64, g)
    got = sweep([3, 3 | POS], _launcher(x, w, bn, 1), _expect(False))
    _check(got.numpy(), conv_ref(x, w, bn, 1, True).numpy(), 'f32', f'F-{n}')


def test_engine_position_major_is_bitwise_natural_under_poison(hip_lib, monkeypatch, sd0):
    """8 clips x 8 segments at 96x96 (64 frames; layer2 12x12, layer3 6x6, layer4 3x3) under TSM_POISON=1: TSM_CONV_CODE = 3 | 0x80
    gives the logits of TSM_CONV_CODE = 3 bit for bit, every segmented 3x3 launch is on the position-major instantiation, and
    the engine's guard bands come back clean (a broken one fails the forward).  No tuning pass and no fused conv2 + conv3, so
    that the trace holds the forced code's launches only, layer2's 3x3 among them."""
    from workoutdetector_amd.engine import TsmEngine, launch_trace
    x = make_input(1964, 8, 8, 96, 96)

    def logits(code):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in {'TSM_AUTOTUNE': '0', 'TSM_CONV_CODE': str(code), 'TSM_TUNE_CACHE': 'off', 'TSM_FUSE_CONV23': '0', 'TSM_POISON': '1'}.items():
            monkeypatch.setenv(k, v)
        eng = TsmEngine(height=96, width=96, max_clips=8, state_dict=sd0)
        try:
            with launch_trace() as tr:
                out = eng.run(None, {'input': x})[0]
        finally:
            eng.close()
        assert np.isfinite(out).all() and not (np.ascontiguousarray(out).view(np.uint32) == POISON).any()
        return out, tr

    natural, tr0 = logits(3)
    pos, tr1 = logits(3 | POS)
    assert _seg3x3(tr0) and all(NATURAL_ARM in k for k in _seg3x3(tr0)), tr0.kernels
    assert len(_seg3x3(tr1)) == len(_seg3x3(tr0)) and all(POS_ARM in k for k in _seg3x3(tr1)), _seg3x3(tr1)
    assert np.array_equal(natural, pos), 'position-major logits differ from the natural order'
    # (the engine alternates directions: both walks of the arm run here)
    assert any(k.endswith(' [reverse]') for k in _seg3x3(tr1)) and any(not k.endswith(' [reverse]') for k in _seg3x3(tr1))
