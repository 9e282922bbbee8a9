"""Both tile walk directions of every conv kernel family, at the tile counts where persistent grids go wrong.

1. Per op (tsm_conv_op through engine.conv_bn_act_nhwc(code=, reverse=)): the cases of tests/_walk_cases.py -- 1 tile, n_cu - 1,
   n_cu, n_cu + 1, 2 n_cu + 1 and a ragged last tile of each family, built from this device's CU count.  Every valid code in
   both directions gives the same bits; the trace shows the family the case is for and the direction of every tile-walking
   launch; the result matches the float64 reference (tests/_conv_ref.py) at the per-op bars and is not mostly zeros.
2. The fused kernels, which have no per-op entry (bneck_ws, front_s2, conv31_fused / conv31_pc, conv23_fused and bf16's
   conv3x3_ws_kernel<true>): engines with the form forced on under TSM_WALK = 0, 1 and unset give the same taps and logits bit
   for bit, the trace shows the fused kernel in the forced direction, and each fused launch's last op is anchored in float64
   to the separate-launch engine's taps."""
import numpy as np
import pytest
import torch

from tests._conv_ref import conv_ref
from tests._guard import guarded_conv
from tests._util import (IGEMM_TILE_DIMS, REVERSE_MARK, assert_bf16_op, assert_close, assert_walked, make_input, ran_tile,
                         sweep)
from tests._walk_cases import cases, count_tiles, tail_split_applies

pytestmark = pytest.mark.gpu

NAMES = {1: '128x128', 2: '128x64', 3: '64x64', 4: '32x32', 5: '128x128w8', 6: '256x256', 7: 'ws', 8: '256x256p'}
SPLITK, TAILK = 0x100, 0x200


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def _bn(c, g):
    return (torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.1,
            torch.randn(c, generator=g) * 0.1, torch.rand(c, generator=g) + 0.5)


def _w(cout, cin, k, g):
    return torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5


def _check(got, want, dtype, what):
    if dtype == 'bf16':
        assert_bf16_op(got, want, what=what)
    else:
        tol = 1e-4 if dtype == 'f32' else 3e-4
        assert_close(got, want, rtol=tol, atol_scale=tol, what=what)


def _family_code(inst):
    """The code whose kernel the case's `inst` names (None: a conv_igemm instantiation, which every igemm code runs)."""
    if inst.startswith('conv_bf16_256p_'):
        return 8
    if inst.startswith('conv_bf16_256_'):
        return 6
    if inst.startswith(('conv1x1_ws', 'conv3x3_ws')):
        return 7
    return None


CASES = cases(_n_cu())


@pytest.mark.parametrize('case', CASES, ids=[c['id'] for c in CASES])
def test_walk_per_op(hip_lib, monkeypatch, case):
    from workoutdetector_amd.engine import launch_trace
    monkeypatch.setenv('TSM_STEM_DIRECT', '0')   # (the bf16 stems through conv_igemm; tsm_conv_op reads it per call)
    c = case
    assert count_tiles(c) == c['tiles'], c['id']
    g = torch.Generator().manual_seed(sum(map(ord, c['id'])))
    dtype, form, T, div = c['dtype'], c['form'], c['T'], c['fold_div']
    x, w, bn = torch.randn(c['n'], c['cin'], c['hi'], c['wi'], generator=g), _w(c['cout'], c['cin'], c['k'], g), _bn(c['cout'], g)
    ho, wo = (c['hi'] + 2 * (c['k'] // 2) - c['k']) // c['stride'] + 1, (c['wi'] + 2 * (c['k'] // 2) - c['k']) // c['stride'] + 1
    kw, ref = {}, {}
    if form in ('res', 'shift_res'):
        res = torch.randn(c['n'], c['cout'], ho, wo, generator=g)
        kw['residual'], ref['residual'] = _nhwc(res).cuda(), res
    if form == 'dual':
        x2, w2, bn2 = torch.randn(c['n'], c['cin2'], c['hi2'], c['wi2'], generator=g), _w(c['cout'], c['cin2'], 1, g), _bn(c['cout'], g)
        kw.update(x2=_nhwc(x2).cuda(), w2=w2.cuda(), bn2=[b.cuda() for b in bn2], stride2=c['stride2'])
        ref.update(x2=x2, w2=w2, bn2=bn2, stride2=c['stride2'])
    shifted = form in ('shift', 'shift_res', 's2shift')
    if shifted:
        kw.update(shift_segments=T, fold_div=div, shift_identity=form != 'shift')
        ref.update(T=T, fold_div=div, shift_target=int(form != 'shift'))
    xd, wd, bnd = _nhwc(x).cuda(), w.cuda(), [b.cuda() for b in bn]
    fam_code = _family_code(c['inst'])
    tail = c['target'] == 'tail'
    if tail:
        assert tail_split_applies(c['n'] * ho * wo, c['cout'], 2, _n_cu()), c['id']

    def run(code, rev):
        with launch_trace() as tr:
            # (hostile memory: fp32 kernels run on these guarded tensors themselves, so a tile no direction writes stays POISON
            #  in y; the bf16 formats run on tsm_conv_op's own staging buffers, which are poisoned and banded the same way --
            #  an unwritten tile of d_ys reaches y as poison through the conversion, a stray store fails the call)
            y = guarded_conv(xd, wd, *bnd, stride=c['stride'], dtype=dtype, code=code, reverse=rev, **kw)
        return _nchw(y.cpu()), tr

    def expect(code, tr):
        base = code & 0xF
        if base in (6, 8, 7):
            fam = {6: 'conv_bf16_256_kernel<', 8: 'conv_bf16_256p_kernel<', 7: c['inst'] if fam_code == 7 else None}[base]
            if fam is not None:
                assert tr.ran(fam), (c['id'], code, tr.kernels)
        else:
            assert NAMES[base] in IGEMM_TILE_DIMS and ran_tile(tr, NAMES[base]), (c['id'], code, tr.kernels)
            if fam_code is None:
                assert any(c['inst'] in k for k in tr.kernels if k.startswith('conv_igemm<')), (c['id'], code, tr.kernels)
        if code == fam_code:
            assert tr.ran(c['inst']), (c['id'], code, tr.kernels)
        split = bool(code & SPLITK) or (bool(code & TAILK) and tail)
        assert tr.ran('splitk_reduce_kernel') == split, (c['id'], code, tr.kernels)

    got = sweep(c['codes'], run, expect)
    want = conv_ref(x, w, bn, c['stride'], True, bf16=dtype == 'bf16', **ref)
    assert float((got != 0).float().mean()) > 0.2, f'{c["id"]}: the output is mostly zeros'
    _check(got.numpy(), want.numpy(), dtype, c['id'])


# ---- 2. the fused kernels under TSM_WALK ----------------------------------------------------------------------------------
# (h, w, clips, T): the config-5 geometry, the headline and a ragged one (16 x 24 frames at layer1, 20 frames: every fused
# form still valid -- layer1 rows <= 64 pixels, an even layer1 height for the front, 256 / T pixels per conv31 tile)
GEOMETRIES = [(256, 256, 1, 16), (224, 224, 2, 8), (64, 96, 5, 4)]
# form -> (TSM_FUSE_* knob, kernel prefix, its tapped stage in the fused engine)
FORMS = {
    'block': ('TSM_FUSE_BLOCK', 'bneck_ws_kernel<', 'layer1.1'),
    'front': ('TSM_FUSE_FRONT', 'front_s2_kernel<', 'layer2.0.conv2'),
    'conv31': ('TSM_FUSE_C3C1', 'conv31_', 'layer2.1'),
    'conv23': ('TSM_FUSE_CONV23', None, 'layer1.1'),
}
FUSE_KNOBS = ('TSM_FUSE_BLOCK', 'TSM_FUSE_FRONT', 'TSM_FUSE_C3C1', 'TSM_FUSE_CONV23')
ENGINE_PARAMS = [(f, d) + geo for f in FORMS for d in (('bf16', 'f32', 'bf16x3') if f == 'conv23' else ('bf16',))
                 for geo in GEOMETRIES]


def _engine(monkeypatch, sd, h, w, b, t, dtype, fuse, walk):
    from workoutdetector_amd.engine import TsmEngine
    monkeypatch.setenv('TSM_AUTOTUNE', '0')
    for knob in FUSE_KNOBS:
        monkeypatch.setenv(knob, '1' if knob == fuse else '0')
    if walk is None:
        monkeypatch.delenv('TSM_WALK', raising=False)
    else:
        monkeypatch.setenv('TSM_WALK', walk)
    return TsmEngine(num_segments=t, height=h, width=w, max_clips=b, state_dict=sd, dtype=dtype)


def _fused_kernel(form, dtype):
    if form == 'conv23':
        return 'conv3x3_ws_kernel<true>' if dtype == 'bf16' else 'conv23_fused_kernel<'
    return FORMS[form][1]


def _t(sd, key):
    return torch.from_numpy(np.asarray(sd['base_model.' + key], dtype=np.float32))


def _bn_of(sd, prefix):
    return tuple(_t(sd, f'{prefix}.{s}') for s in ('weight', 'bias', 'running_mean', 'running_var'))


def _nchw_np(a):
    return torch.from_numpy(a).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize('form,dtype,h,w,b,t', ENGINE_PARAMS)
def test_fused_walk(hip_lib, monkeypatch, form, dtype, h, w, b, t):
    from workoutdetector_amd.engine import launch_trace
    from workoutdetector_amd.weights import make_state_dict
    sd = make_state_dict(31, 12)
    x = make_input(1100 + h + t, b, t, h, w)
    knob, _, stage = FORMS[form]
    kern = _fused_kernel(form, dtype)
    stages = [stage] + (['layer2.2.conv1'] if form == 'conv31' else [])
    got = {}
    for walk in (None, '0', '1'):
        eng = _engine(monkeypatch, sd, h, w, b, t, dtype, knob, walk)
        try:
            outs = []
            for s in stages:
                with launch_trace() as tr:
                    outs.append(eng.forward_tap(x, s))
                assert tr.ran(kern), (form, walk, s, sorted(set(tr.kernels)))
                if walk is not None:
                    assert_walked(tr, walk == '1', f'{form} TSM_WALK={walk} tap {s}')
            with launch_trace() as tr:
                outs.append(eng.run(None, {'input': x})[0])
            assert tr.ran(kern), (form, walk, sorted(set(tr.kernels)))
            if walk is not None:
                assert_walked(tr, walk == '1', f'{form} TSM_WALK={walk} forward')
                fused = [k for k in tr.kernels if k.startswith(kern)]
                assert all(k.endswith(REVERSE_MARK) == (walk == '1') for k in fused), fused
            else:   # the default schedule alternates: some launch of a forward walks each way
                assert any(k.endswith(REVERSE_MARK) for k in tr.kernels), sorted(set(tr.kernels))
        finally:
            eng.close()
        got[walk] = outs
    for i, name in enumerate(stages + ['logits']):
        assert np.array_equal(got['0'][i], got[None][i]), (name, 'TSM_WALK=0 vs unset')
        assert np.array_equal(got['1'][i], got[None][i]), (name, 'TSM_WALK=1 vs unset')
    assert np.isfinite(got[None][-1]).all()

    # float64 anchor of the fused launch's last op, from the separate-launch engine's taps
    sep = _engine(monkeypatch, sd, h, w, b, t, dtype, None, None)
    try:
        bf = dtype == 'bf16'
        if form in ('block', 'conv23'):
            mid, ident = sep.forward_tap(x, 'layer1.1.conv2'), sep.forward_tap(x, 'layer1.0')
            want = conv_ref(_nchw_np(mid), _t(sd, 'layer1.1.conv3.weight'), _bn_of(sd, 'layer1.1.bn3'), 1, True,
                            residual=_nchw_np(ident), bf16=bf)
            anchors = [(got[None][0], want, 'layer1.1 conv3 + identity')]
        elif form == 'front':
            mid = sep.forward_tap(x, 'layer2.0.conv1')
            want = conv_ref(_nchw_np(mid), _t(sd, 'layer2.0.conv2.weight'), _bn_of(sd, 'layer2.0.bn2'), 2, True, bf16=bf)
            anchors = [(got[None][0], want, 'layer2.0 conv2 (stride 2)')]
        else:
            mid, ident = sep.forward_tap(x, 'layer2.1.conv2'), sep.forward_tap(x, 'layer2.0')
            y = conv_ref(_nchw_np(mid), _t(sd, 'layer2.1.conv3.weight'), _bn_of(sd, 'layer2.1.bn3'), 1, True,
                         residual=_nchw_np(ident), bf16=bf)
            blk = sep.forward_tap(x, 'layer2.1')
            nxt = conv_ref(_nchw_np(blk), _t(sd, 'layer2.2.conv1.net.weight'), _bn_of(sd, 'layer2.2.bn1'), 1, True, T=t,
                           fold_div=8, bf16=bf)
            anchors = [(got[None][0], y, 'layer2.1 conv3 + identity'), (got[None][1], nxt, 'layer2.2 shift + conv1')]
    finally:
        sep.close()
    for tap, want, what in anchors:
        assert float((tap != 0).mean()) > 0.2, f'{what}: mostly zeros'
        _check(_nchw_np(tap).numpy(), want.numpy(), dtype, f'{form} {dtype} {h}x{w} T={t}: {what}')
