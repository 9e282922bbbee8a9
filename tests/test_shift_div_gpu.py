"""Every temporal-shift kernel arm at shift_div 1, 2, 4 and (fp32) 16 -- the suite otherwise runs almost everything at 8.

1. Per op (tsm_conv_op through engine.conv_bn_act_nhwc): the cases of tests/_shift_div_cases.py in hostile memory
   (tests/_guard.py: the bands are one whole frame, the reach of a wrong shift index).  The family's kernel forced and the 64x64
   conv_igemm tile forced agree bit for bit, in both tile walk directions; the trace shows the family's instantiation under its
   code and not under the 64x64 code; the result meets the dtype's per-op bar against the float64 reference
   (tests/_conv_ref.py).  Where 2 * fold exceeds the shifted channels (div 1) the call is refused with its status and launches
   nothing.
2. Whole engines against oracle/tsm_oracle.py at the engine's shift_div: logits and the conv1 tap of every stage's first block,
   blockres and block placement, ResNet-50 / ResNet-18 / Wide-ResNet-50-2; the fused forms that must fall back at a fold other
   than C / 8 and those that must still run; the weight-stationary and 256 x 256 kernels forced everywhere; the tuner; poison.

tests/test_shift_div_cases_cpu.py shows on the CPU that these very inputs tell a wrong fold (and exchanged neighbours) from the
right one by at least ten times each bar used here."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _shift_div_cases as sc
from tests._guard import guarded_conv
from tests._shift_div_ops import (engine_input, engine_oracle, engine_state_dict, logits_misses, misses, operands, reference,
                                  tap_misses)
from tests._util import IGEMM_TILE_DIMS, assert_fused_slots, ran_tile, sweep

pytestmark = pytest.mark.gpu

NAMES = {1: '128x128', 2: '128x64', 3: '64x64', 4: '32x32', 5: '128x128w8', 6: '256x256', 7: 'ws', 8: '256x256p'}
FUSE_KNOBS = ('TSM_FUSE_BLOCK', 'TSM_FUSE_FRONT', 'TSM_FUSE_C3C1', 'TSM_FUSE_CONV23')
BLOCK_ARM = 'kPrecBlockShift'


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


CASES = sc.cases(_n_cu())


# ---- 1. per op ------------------------------------------------------------------------------------------------------------------
def _launch_kw(c, ref):
    kw = {}
    if 'residual' in ref:
        kw['residual'] = _nhwc(ref['residual']).cuda()
    if 'x2' in ref:
        kw.update(x2=_nhwc(ref['x2']).cuda(), w2=ref['w2'].cuda(), bn2=[b.cuda() for b in ref['bn2']], stride2=ref['stride2'])
    kw.update(shift_segments=c['T'], fold_div=c['fold_div'], shift_identity=c['form'] != 'shift')
    return kw


def _ran_inst(tr, inst):
    return any(all(s in k for s in inst) for k in tr.kernels)


@pytest.mark.parametrize('case', CASES, ids=[c['id'] for c in CASES])
def test_shift_div_per_op(hip_lib, capsys, case):
    from workoutdetector_amd import _lib
    from workoutdetector_amd.engine import launch_trace
    c = case
    (x, w, bn), ref = operands(c)
    kw = _launch_kw(c, ref)
    xd, wd, bnd = _nhwc(x).cuda(), w.cuda(), [b.cuda() for b in bn]

    if c['expect'] == 'refuse':       # 2 * fold > the shifted channels: refused under every code, nothing launched
        for code in c['codes']:
            with launch_trace() as tr:
                with pytest.raises(_lib.TsmError) as ei:
                    guarded_conv(xd, wd, *bnd, stride=c['stride'], dtype=c['dtype'], code=code, segmented=c['segmented'], **kw)
            assert ei.value.status == c['status'] and sc.REFUSAL_TEXT in str(ei.value), (c['id'], code, ei.value)
            assert tr.kernels == [], (c['id'], code, tr.kernels)
        return

    def run(code, rev):
        with launch_trace() as tr:
            y = guarded_conv(xd, wd, *bnd, stride=c['stride'], dtype=c['dtype'], code=code, reverse=rev, segmented=c['segmented'], **kw)
        assert not tr.ran('temporal_shift_kernel'), ('the shifted tensor must never be materialised', tr.kernels)
        return _nchw(y.cpu()), tr

    own = c['family'] in ('igemm', 'igemm_seg')       # conv_igemm's own arms: every code of the case runs `inst` on its tile

    def expect(code, tr):
        base = code & 0xF
        if base in (6, 7, 8):
            assert _ran_inst(tr, c['inst']), (c['id'], code, c['inst'], tr.kernels)
            assert not tr.ran('conv_igemm<'), (c['id'], code, tr.kernels)
        else:
            assert NAMES[base] in IGEMM_TILE_DIMS and ran_tile(tr, NAMES[base]), (c['id'], code, tr.kernels)
            assert _ran_inst(tr, c['inst']) == own, (c['id'], code, c['inst'], tr.kernels)
            for fam in ('conv_bf16_256', 'conv1x1_ws', 'conv3x3_ws'):
                assert not tr.ran(fam), (c['id'], code, tr.kernels)
        assert tr.ran('splitk_reduce_kernel') == bool(code & sc.SPLITK), (c['id'], code, tr.kernels)

    got = sweep(c['codes'], run, expect)
    want = reference(c, (x, w, bn), ref)
    assert float((got != 0).float().mean()) > 0.2, f'{c["id"]}: the output is mostly zeros'
    m = misses(got.numpy(), want.numpy(), c['dtype'])
    with capsys.disabled():
        print(f'\n[{c["id"]}] fold {c["fold"]}: worst element at {m:.3f} of the {c["dtype"]} per-op bar')
    assert np.isfinite(got.numpy()).all() and m <= 1.0, (c['id'], m)


# ---- 2. engines -----------------------------------------------------------------------------------------------------------------
def _env(monkeypatch, autotune='0', **env):
    """TSM_AUTOTUNE = 0 unless the tuner is the subject; every other knob this file touches back to unset, then `env`."""
    for knob in FUSE_KNOBS + ('TSM_CONV_TILE', 'TSM_CONV_CODE', 'TSM_POISON', 'TSM_WALK'):
        monkeypatch.delenv(knob, raising=False)
    if autotune is None:
        monkeypatch.delenv('TSM_AUTOTUNE', raising=False)
    else:
        monkeypatch.setenv('TSM_AUTOTUNE', autotune)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _engine(case):
    from workoutdetector_amd.engine import TsmEngine
    base_model, place, dtype, div, geo = case
    t, h, w, _, _ = sc.GEOMETRIES[geo]
    return TsmEngine(num_class=12, num_segments=t, height=h, width=w, shift_div=div, max_clips=2, dtype=dtype, base_model=base_model,
                     shift_place=place, state_dict=engine_state_dict(base_model, place, geo))


def _last_block(base_model):
    return 'layer4.1' if base_model == 'resnet18' else 'layer4.2'


@pytest.mark.parametrize('case', sc.ENGINE_CASES, ids=[sc.engine_id(e) for e in sc.ENGINE_CASES])
def test_engine_against_oracle(hip_lib, monkeypatch, capsys, case):
    """Logits and taps against the oracle at the engine's shift_div, at the suite's bars: logits rtol 1e-3 + 1e-5 of the scale
    (bf16: BF16_E2E_BAR against the bf16-storage oracle, same arg-max), taps rtol 1e-3 + 3e-5 (bf16: BF16_TAP_BAR).  fp32 and
    split-bf16 ResNet-50 once more with the fused conv2 + conv3 launch: the same logits bit for bit."""
    from workoutdetector_amd.engine import launch_trace
    base_model, place, dtype, div, geo = case
    what = sc.engine_id(case)
    _, x = engine_input(geo)
    want, taps = engine_oracle(base_model, place, dtype == 'bf16', div, geo)
    _env(monkeypatch)
    eng = _engine(case)
    try:
        with launch_trace() as tr:
            got = eng.run(None, {'input': x})[0]
        assert not tr.ran('temporal_shift_kernel'), 'the shifted tensor must never be materialised'
        arms = [k for k in tr.kernels if k.startswith('conv_igemm<') and BLOCK_ARM in k]
        if place == 'block':      # the shifted identity / second source ran on conv_igemm's arms or the persistent 256 tile's
            assert arms or tr.ran('conv_bf16_256p_kernel<1, true, true, false>'), (what, sorted(set(tr.kernels)))
        else:
            assert not arms, (what, arms)
        figures = {'logits': logits_misses(got, want, dtype)}
        for stage in sc.CONV1_TAPS + (_last_block(base_model),):
            figures[stage] = tap_misses(eng.forward_tap(x, stage), taps[stage], dtype)
    finally:
        eng.close()
    with capsys.disabled():
        print(f'\n[{what}] fraction of each bar: ' + ', '.join(f'{k} {v:.3f}' for k, v in figures.items()))
    assert np.isfinite(got).all() and all(v <= 1.0 for v in figures.values()), (what, figures)
    if dtype == 'bf16':
        assert (got.argmax(1) == want.argmax(1)).all(), what
    if base_model == 'resnet50' and place == 'blockres' and dtype != 'bf16':
        out = {}
        for flag in ('0', '1'):
            _env(monkeypatch, TSM_FUSE_CONV23=flag)
            eng = _engine(case)
            try:
                with launch_trace() as tr:
                    out[flag] = eng.run(None, {'input': x})[0]
            finally:
                eng.close()
            assert tr.ran('conv23_fused_kernel<') == (flag == '1'), (what, flag, sorted(set(tr.kernels)))
        assert np.array_equal(out['0'], out['1']) and np.array_equal(out['0'], got), what


C31 = ((256, 'conv31_fused_kernel<K3, C, N1> [K3 = 128, C = 512, N1 = 128]', ('layer2.2.conv1', 'layer2.3.conv1')),
       (128, 'conv31_pc_kernel<K3, C, N1> [K3 = 128, C = 512, N1 = 256]', ('layer3.0.conv1',)),
       (128, 'conv31_pc_kernel<K3, C, N1> [K3 = 256, C = 1024, N1 = 256]', ('layer3.2.conv1', 'layer3.3.conv1', 'layer3.4.conv1', 'layer3.5.conv1')))
C31_FIRST = {'layer2.2.conv1': 'layer2.1.conv1', 'layer3.2.conv1': 'layer3.1.conv1'}


@pytest.mark.parametrize('div', [1, 2, 4])
def test_forced_fused_forms_fall_back_or_run_with_the_same_bits(hip_lib, monkeypatch, div):
    """A bf16 ResNet-50 with TSM_FUSE_BLOCK = TSM_FUSE_FRONT = TSM_FUSE_C3C1 = 1 at a fold other than C / 8: the whole-block and
    the front kernel need fold == cin / 8 and must fall back; the cross-block kernel takes every fold of whole 64-channel chunks
    with 2 * fold <= C and must run at div 2 and 4 (T = 4: a clip-major tile exists), and not at div 1.  Either way the taps and
    logits are those of an engine with all three switches at 0, bit for bit."""
    from workoutdetector_amd.engine import launch_trace
    case = ('resnet50', 'blockres', 'bf16', div, 'T4')
    t = sc.GEOMETRIES['T4'][0]
    _, x = engine_input('T4')
    stages = ('layer1.2', 'layer2.0.conv2', 'layer2.2.conv1', 'layer2.3', 'layer3.0.conv1', 'layer3.5')
    got = {}
    for flag in ('1', '0'):
        _env(monkeypatch, TSM_FUSE_BLOCK=flag, TSM_FUSE_FRONT=flag, TSM_FUSE_C3C1=flag, TSM_FUSE_CONV23='0')
        eng = _engine(case)
        try:
            with launch_trace() as tr:
                got[flag] = [eng.run(None, {'input': x})[0]] + [eng.forward_tap(x, s) for s in stages]
            assert not tr.ran('bneck_ws_kernel') and not tr.ran('front_s2_kernel'), (div, flag, sorted(set(tr.kernels)))
            taken = set()
            for rows, inst, names in C31:
                runs = flag == '1' and div != 1 and rows % t == 0 and rows // t >= 8
                assert sc.conv31_fold_ok(512, 512 // div) == (div != 1)
                assert tr.ran(inst) == runs, (div, flag, inst, sorted(set(tr.kernels)))
                if runs:
                    taken |= set(names)
            assert tr.ran('conv31_') == bool(taken)
            assert all('+' not in v for v in eng.conv_tiles(2).values())      # (a forced form is not a tuner choice)
            assert_fused_slots(eng, x, taken, f'div {div} switches {flag}')
        finally:
            eng.close()
    for name, a, b in zip(('logits',) + stages, got['1'], got['0']):
        assert np.array_equal(a, b), (div, name)
    want, _ = engine_oracle('resnet50', 'blockres', True, div, 'T4')
    assert logits_misses(got['1'][0], want, 'bf16') <= 1.0


WS_SHIFTED = ('conv1x1_ws_kernel<64>', 'conv1x1_ws_kernel<256>', 'conv1x1_wsn_kernel<256, 128, false>',
              'conv1x1_wsn_kernel<512, 128, false>', 'conv1x1_wsn_kernel<512, 256, false>')


@pytest.mark.parametrize('div', [1, 2, 4])
def test_forced_tiles_equal_the_igemm_engine_bitwise(hip_lib, monkeypatch, div):
    """A bf16 engine with TSM_CONV_TILE = ws, 256x256 and 256x256p against one forced onto 64x64: block outputs and logits bit for
    bit, and the trace shows the shifted weight-stationary and 256 kernels ran -- at div 1 the weight-stationary 1x1 kernels
    refuse 2 * fold > C and conv_igemm must run in their place, with the same bits."""
    from workoutdetector_amd.engine import launch_trace
    case = ('resnet50', 'blockres', 'bf16', div, 'T3')
    _, x = engine_input('T3')
    stages = ('layer1.0', 'layer1.2', 'layer2.0', 'layer2.3', 'layer3.0', 'layer4.0')
    got = {}
    for tile in ('64x64', 'ws', '256x256', '256x256p'):
        _env(monkeypatch, TSM_CONV_TILE=tile, **{k: '0' for k in FUSE_KNOBS})
        eng = _engine(case)
        try:
            with launch_trace() as tr:
                got[tile] = [eng.forward_tap(x, s) for s in stages] + [eng.run(None, {'input': x})[0]]
        finally:
            eng.close()
        names = sorted(set(tr.kernels))
        for fam in WS_SHIFTED:
            assert tr.ran(fam) == (tile == 'ws' and div != 1), (div, tile, fam, names)
        assert tr.ran('conv3x3_ws_kernel<false>') == (tile == 'ws'), (div, tile, names)       # (unshifted: whatever the fold)
        assert tr.ran('conv_bf16_256_kernel<1, true>') == (tile == '256x256'), (div, tile, names)
        assert tr.ran('conv_bf16_256p_kernel<1, true>') == (tile == '256x256p'), (div, tile, names)
        assert not tr.ran('temporal_shift_kernel')
    for tile in ('ws', '256x256', '256x256p'):
        for name, a, b in zip(stages + ('logits',), got[tile], got['64x64']):
            assert np.array_equal(a, b), (div, tile, name)
    want, _ = engine_oracle('resnet50', 'blockres', True, div, 'T3')
    assert logits_misses(got['64x64'][-1], want, 'bf16') <= 1.0


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_tuner_at_div_4_beside_a_div_8_cache(hip_lib, monkeypatch, tmp_path, dtype):
    """Autotune on, TSM_TUNE_CACHE holding the line a div-8 engine of the same geometry wrote first: the div-4 engine's logits are
    the TSM_AUTOTUNE = 0 engine's bit for bit; the tuner offers neither the whole-block nor the front kernel (no '+block' /
    '+front' code); a forward launches the cross-block kernel exactly once per '+conv1' code."""
    from workoutdetector_amd.engine import launch_trace
    cache = tmp_path / 'tune.txt'
    _, x = engine_input('T4')
    _env(monkeypatch, autotune=None, TSM_TUNE_CACHE=str(cache))
    first = _engine(('resnet50', 'blockres', dtype, 8, 'T4'))
    first.run(None, {'input': x})
    first.close()
    assert len(cache.read_text().splitlines()) == 1
    case = ('resnet50', 'blockres', dtype, 4, 'T4')
    eng = _engine(case)
    try:
        ya = eng.run(None, {'input': x})[0]
        with launch_trace() as tr:
            assert np.array_equal(eng.run(None, {'input': x})[0], ya)
        tiles = eng.conv_tiles(2)
    finally:
        eng.close()
    assert len(cache.read_text().splitlines()) == 2, 'a div-4 engine must not read the div-8 line'
    assert not any('+block' in v or '+front' in v for v in tiles.values()), tiles
    fused = [k for k, v in tiles.items() if v.endswith('+conv1')]
    assert tr.count('conv31_fused_kernel') + tr.count('conv31_pc_kernel') == len(fused), (fused, sorted(set(tr.kernels)))
    assert not tr.ran('bneck_ws_kernel') and not tr.ran('front_s2_kernel'), sorted(set(tr.kernels))
    _env(monkeypatch, TSM_TUNE_CACHE='off')
    ref = _engine(case)
    try:
        yb = ref.run(None, {'input': x})[0]
    finally:
        ref.close()
    assert np.array_equal(ya, yb)
    want, _ = engine_oracle('resnet50', 'blockres', dtype == 'bf16', 4, 'T4')
    assert logits_misses(ya, want, dtype) <= 1.0


@pytest.mark.parametrize('dtype,div', [('bf16', 2), ('f32', 4)])
def test_poison_changes_no_bit(hip_lib, monkeypatch, dtype, div):
    case = ('resnet50', 'blockres', dtype, div, 'T3')
    _, x = engine_input('T3')
    got = {}
    for flag in ('1', '0'):
        _env(monkeypatch, TSM_POISON=flag)
        eng = _engine(case)
        try:
            got[flag] = [eng.run(None, {'input': x})[0], eng.forward_tap(x, 'layer2.0.conv1'), eng.forward_tap(x, 'layer4.2')]
        finally:
            eng.close()
    for a, b in zip(got['1'], got['0']):
        assert np.array_equal(a, b)
    want, _ = engine_oracle('resnet50', 'blockres', dtype == 'bf16', div, 'T3')
    assert logits_misses(got['1'][0], want, dtype) <= 1.0


@pytest.mark.parametrize('dtype', ['f32', 'bf16x3', 'bf16'])
def test_block_placement_refuses_shift_div_1_up_front(hip_lib, dtype):
    """Block placement's shifted identity and downsample launches take 2 * fold <= channels, so at shift_div 1 every forward
    would be refused: tsm_set_shift_place refuses the placement itself (TSM_ERR_UNSUPPORTED, a message), nothing is created that
    fails at its first forward.  blockres takes shift_div 1 (test_engine_against_oracle), and so does an unshifted engine in
    either placement."""
    from workoutdetector_amd import _lib
    from workoutdetector_amd.engine import TsmEngine
    lib = _lib.load()
    for div, rc_block in ((1, -7), (2, 0)):
        cfg = _lib.TsmConfig(C.sizeof(_lib.TsmConfig), 12, 3, 64, 64, div, 1, 2, 0, _lib.DTYPES[dtype])
        h = C.c_void_p()
        _lib.check(lib.tsm_create(C.byref(cfg), C.byref(h)))
        try:
            assert lib.tsm_set_shift_place(h, 1) == rc_block
            if rc_block:
                assert b'shift_div >= 2' in lib.tsm_last_error(h)
            assert lib.tsm_set_shift_place(h, 0) == 0
        finally:
            lib.tsm_destroy(h)
    cfg = _lib.TsmConfig(C.sizeof(_lib.TsmConfig), 12, 3, 64, 64, 1, 0, 2, 0, _lib.DTYPES[dtype])      # is_shift = 0: no fold at all
    h = C.c_void_p()
    _lib.check(lib.tsm_create(C.byref(cfg), C.byref(h)))
    try:
        assert lib.tsm_set_shift_place(h, 1) == 0
    finally:
        lib.tsm_destroy(h)
    with pytest.raises(_lib.TsmError) as ei:
        TsmEngine(num_class=12, num_segments=3, height=64, width=64, shift_div=1, max_clips=2, dtype=dtype, shift_place='block',
                  state_dict=engine_state_dict('resnet50', 'block', 'T3'))
    assert ei.value.status == -7 and 'shift_div >= 2' in str(ei.value)
