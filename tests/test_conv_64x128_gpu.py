"""The 64x128 tile of the fp32 unsegmented 1x1 convs (tile code 9, conv_igemm<64, 128, 2, 2, 1, ..>) per op, through tsm_conv_op
in hostile memory (tests/_guard.py), and in the engine under TSM_POISON=1.

Every output element of the arm receives the 64x64 arm's MFMA sequence in the same k order, so every case asserts the SAME BITS
(torch.equal) as tile code 3 on the same operands, in both walk directions, and from the launch trace that the arm's
instantiation really ran; the float64 reference (tests/_conv_ref.py) is met at the per-op fp32 bar, rtol 1e-4 + 1e-4 of the
scale.  The shapes are the smallest at which each part of the kernel can go wrong:

  K        32 (the prologue's first step only: the K loop does not run, the last step multiplies alone), 64 (one loop step whose
           injected loads are all past K), 256 (loop steps with live loads).  cin is a power of two, so K = 96 -- loop steps 0 and
           1, then the last -- exists as the two-source case only (64 + 32).
  Cout     128 (one column tile) and 256 (two).
  M        3 frames of 5x5 = 75 rows: the second row tile holds 11 rows; y sits between poisoned bands (a store past M breaks
           the band behind it) and starts poisoned (a row not written stays poison).
  shift    T = 3, C = 64, fold 8: the boundaries at channels 8 and 16 fall inside the first K-step, on 16-byte chunks 2 and 4;
           one clip, so frames 0, 1 and 2 are the clip's first, a middle and its last frame.
  residual Cout 128 and 256 (both 64-column halves of the epilogue's staging, on one and on two column tiles).
  second   K1 = 64 + C2 = 32 with stride2 = 2 on 6x6 -> 3x3 frames: the sources' boundary lies between loop steps 1 and 2.
  refusals Cout = 192, a segmented layer and a 3x3: code 9 runs what code 0 runs, and gives its bits."""
import numpy as np
import pytest
import torch

from tests._conv_ref import conv_ref
from tests._guard import POISON, guarded_conv
from tests._util import make_input, ran_tile, sweep
from tests.test_conv_forms_gpu import _bn, _check, _nchw, _nhwc, _w

pytestmark = pytest.mark.gpu

TILE = 9
ARM = 'conv_igemm<64, 128, 2, 2, 1, '
PLAIN, SHIFT, RES, DUAL = 'false, false, kPrecF32>', 'true, false, kPrecF32>', 'false, true, kPrecF32>', 'false, false, kPrecF32, true>'
KNOBS = ('TSM_AUTOTUNE', 'TSM_WALK', 'TSM_CONV_TILE', 'TSM_CONV_CODE', 'TSM_TUNE_CACHE', 'TSM_POISON', 'TSM_POS_MAJOR',
         'TSM_TILE_64X128', 'TSM_FUSE_CONV23')


def _arm(tr):
    return [k for k in tr.kernels if k.startswith(ARM)]


def _launcher(x, w, bn, **kw):
    """run(code, reverse) -> (y NCHW on the host, trace) on guarded operands; tensors in `kw` go to the device."""
    from workoutdetector_amd.engine import launch_trace
    xd, wd, bnd = _nhwc(x).cuda(), w.cuda(), [b.cuda() for b in bn]
    kw = {k: ([b.cuda() for b in v] if k == 'bn2' else v.cuda() if torch.is_tensor(v) else v) for k, v in kw.items()}

    def run(code, rev):
        with launch_trace() as tr:
            y = guarded_conv(xd, wd, *bnd, dtype='f32', code=code, reverse=rev, **kw)
        return _nchw(y.cpu()), tr
    return run


def _expect_arm(arm):
    def expect(code, tr):
        igemm = [k for k in tr.kernels if k.startswith('conv_igemm<')]
        assert len(igemm) == 1, (code, tr.kernels)
        if code == TILE:
            assert _arm(tr) == igemm and igemm[0][len(ARM):].split(' [')[0] == arm, (arm, tr.kernels)
        else:
            assert not _arm(tr) and ran_tile(tr, '64x64'), tr.kernels
    return expect


def _live(y, what):
    assert float((y != 0).float().mean()) > 0.2, f'{what}: the output is mostly zeros'


@pytest.mark.parametrize('cout', [128, 256])
@pytest.mark.parametrize('cin', [32, 64, 256])
def test_plain_arm_equals_64x64(hip_lib, cin, cout):
    g = torch.Generator().manual_seed(9000 + cin + cout)
    x, w, bn = torch.randn(3, cin, 5, 5, generator=g), _w(cout, cin, 1, g), _bn(cout, g)
    got = sweep([3, TILE], _launcher(x, w, bn), _expect_arm(PLAIN))
    _live(got, f'K {cin} Cout {cout}')
    _check(got.numpy(), conv_ref(x, w, bn, 1, True).numpy(), 'f32', f'plain K {cin} Cout {cout}')


def test_plain_arm_without_relu(hip_lib):
    """The clamp's floor is -inf without the activation: negative outputs must come through."""
    g = torch.Generator().manual_seed(9101)
    x, w, bn = torch.randn(3, 64, 5, 5, generator=g), _w(128, 64, 1, g), _bn(128, g)
    got = sweep([3, TILE], _launcher(x, w, bn, relu=False), _expect_arm(PLAIN))
    assert float((got < 0).float().mean()) > 0.2
    _check(got.numpy(), conv_ref(x, w, bn, 1, False).numpy(), 'f32', 'plain, no ReLU')


def test_shifted_arm_equals_64x64(hip_lib):
    g = torch.Generator().manual_seed(9202)
    x, w, bn = torch.randn(3, 64, 5, 5, generator=g), _w(128, 64, 1, g), _bn(128, g)
    got = sweep([3, TILE], _launcher(x, w, bn, shift_segments=3, fold_div=8), _expect_arm(SHIFT))
    _live(got, 'shift')
    want = conv_ref(x, w, bn, 1, True, T=3, fold_div=8)
    _check(got.numpy(), want.numpy(), 'f32', 'shift T 3 fold 8')
    unshifted = conv_ref(x, w, bn, 1, True)
    assert float((unshifted - want).abs().max()) > 1e-2 * float(want.abs().max())     # the shift matters on these operands


@pytest.mark.parametrize('cout', [128, 256])
def test_residual_arm_equals_64x64(hip_lib, cout):
    g = torch.Generator().manual_seed(9303 + cout)
    x, w, bn = torch.randn(3, 64, 5, 5, generator=g), _w(cout, 64, 1, g), _bn(cout, g)
    res = torch.randn(3, cout, 5, 5, generator=g)
    got = sweep([3, TILE], _launcher(x, w, bn, residual=_nhwc(res)), _expect_arm(RES))
    _live(got, f'residual Cout {cout}')
    _check(got.numpy(), conv_ref(x, w, bn, 1, True, residual=res).numpy(), 'f32', f'residual Cout {cout}')


def test_second_source_arm_equals_64x64(hip_lib):
    g = torch.Generator().manual_seed(9404)
    x, w, bn = torch.randn(3, 64, 3, 3, generator=g), _w(128, 64, 1, g), _bn(128, g)
    x2, w2, bn2 = torch.randn(3, 32, 6, 6, generator=g), _w(128, 32, 1, g), _bn(128, g)
    got = sweep([3, TILE], _launcher(x, w, bn, x2=_nhwc(x2), w2=w2, bn2=bn2, stride2=2), _expect_arm(DUAL))
    _live(got, 'second source')
    _check(got.numpy(), conv_ref(x, w, bn, 1, True, x2=x2, w2=w2, bn2=bn2, stride2=2).numpy(), 'f32', 'K 64 + 32, stride2 2')


REFUSALS = [  # id, cin, cout, k, keyword arguments
    ('cout-192', 64, 192, 1, {}),
    ('segmented', 1024, 128, 1, {'segmented': True}),
    ('3x3', 32, 128, 3, {}),
]


@pytest.mark.parametrize('name,cin,cout,k,kw', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_code_falls_back_where_the_tile_does_not_apply(hip_lib, name, cin, cout, k, kw):
    g = torch.Generator().manual_seed(9505 + cin + cout + k)
    x, w, bn = torch.randn(3, cin, 5, 5, generator=g), _w(cout, cin, k, g), _bn(cout, g)
    ran = {}

    def expect(code, tr):
        assert not _arm(tr), (name, tr.kernels)
        lines = [l.replace(' [reverse]', '') for l in tr.kernels if l.startswith('conv_igemm<')]
        assert len(lines) == 1 and ran.setdefault('kernel', lines[0]) == lines[0], (name, code, lines, ran)     # the default's kernel
    got = sweep([0, TILE], _launcher(x, w, bn, **kw), expect)
    _live(got, name)
    _check(got.numpy(), conv_ref(x, w, bn, 1, True).numpy(), 'f32', name)


def test_engine_on_the_tile_is_bitwise_the_default_under_poison(hip_lib, monkeypatch, sd0):
    """1 clip x 8 segments at 32x32 under TSM_POISON=1, no tuning and no fused conv2 + conv3: TSM_CONV_TILE=64x128 gives the
    default engine's logits bit for bit, with the arm on every eligible launch -- the unsegmented 1x1 convs to a multiple of
    128 channels: conv3 of every block but layer4.0 (whose conv3 + downsample GEMM is segmented), 3 with a second source and
    12 with a residual, and the shifted conv1 of layer2.0-3 and layer3.0 (from layer3.1 on conv1 is segmented; layer1's has 64
    output channels) -- and every other launch on the kernel the default runs."""
    from workoutdetector_amd.engine import TsmEngine, launch_trace
    x = make_input(1128, 1, 8, 32, 32)

    def logits(env):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in dict({'TSM_AUTOTUNE': '0', 'TSM_TUNE_CACHE': 'off', 'TSM_FUSE_CONV23': '0', 'TSM_POISON': '1'}, **env).items():
            monkeypatch.setenv(k, v)
        eng = TsmEngine(height=32, width=32, max_clips=1, state_dict=sd0)
        try:
            with launch_trace() as tr:
                out = eng.run(None, {'input': x})[0]
        finally:
            eng.close()
        assert np.isfinite(out).all() and not (np.ascontiguousarray(out).view(np.uint32) == POISON).any()
        return out, tr

    default, tr0 = logits({})
    forced, tr1 = logits({'TSM_CONV_TILE': '64x128'})
    assert not _arm(tr0), tr0.kernels
    arms = [k[len(ARM):].replace(' [reverse]', '') for k in _arm(tr1)]
    assert {a: arms.count(a) for a in (PLAIN, SHIFT, RES, DUAL)} == {PLAIN: 0, SHIFT: 5, RES: 12, DUAL: 3}, arms
    assert len(tr1.kernels) == len(tr0.kernels)
    other0 = [k for k, k1 in zip(tr0.kernels, tr1.kernels) if not k1.startswith(ARM)]
    other1 = [k for k in tr1.kernels if not k.startswith(ARM)]
    assert other0 == other1                                            # every other launch is the default's
    assert all(k.startswith('conv_igemm<') and 'KS = 1' in k for k, k1 in zip(tr0.kernels, tr1.kernels) if k1.startswith(ARM))
    assert np.array_equal(default, forced), 'logits on the 64x128 tile differ from the default engine'
    assert any(k.endswith(' [reverse]') for k in _arm(tr1)) and any(not k.endswith(' [reverse]') for k in _arm(tr1))
