"""The engine in hostile memory (TSM_POISON=1, README's hook list; DESIGN 2, the hostile-memory rule).

The engine's activations live in five buffers sized for the largest layer at max_clips, reused layer after layer and forward
after forward, so the kernels that exist only inside the engine (bneck_ws, front_s2, conv31_fused / conv31_pc, conv23_fused,
conv3x3_ws_kernel<true>) are otherwise always tested on buffers full of finite activations of the same geometry: a consumer
that reads an element its producer no longer writes, or a row past a layer's extent, gets a believable number.  Under
TSM_POISON=1 every device buffer sits between bands of the poison word, each forward first fills the activation and scratch
buffers with it, and after its last launch the bands are verified (TSM_ERR_GUARD fails the call).

Each case builds a clean engine and a poisoned one with the same weights, knobs and walk, and asserts: logits and every tap
bit-identical between the two, no poison word and no non-finite value in either, the launch trace of the POISONED engine shows
the form under test, and the logits meet the oracle bar of the corresponding existing test (fp32 / split-bf16: rtol 1e-3 +
1e-5 of the scale against the fp32 oracle, test_engine_gpu.py; bf16: BF16_E2E_BAR of the scale and the same arg-max against
the bf16-storage oracle, tests/_util.bf16_logits_report)."""
import numpy as np
import pytest
import torch

from oracle import tsm_oracle
from tests._guard import POISON
from tests._util import assert_close, assert_ran, assert_walked, bf16_logits_report, make_input
from tests.test_walk_gpu import ENGINE_PARAMS, FORMS, FUSE_KNOBS, GEOMETRIES, _fused_kernel

pytestmark = pytest.mark.gpu

R50_STAGES = ['stem', 'layer1.0', 'layer1.2', 'layer2.0', 'layer2.3', 'layer3.0', 'layer3.5', 'layer4.0', 'layer4.2']   # test_stage_taps_224
R18_STAGES = ['stem', 'layer1.0', 'layer1.1', 'layer2.0', 'layer2.1', 'layer3.0', 'layer3.1', 'layer4.0', 'layer4.1']
KNOBS = FUSE_KNOBS + ('TSM_AUTOTUNE', 'TSM_WALK', 'TSM_CONV_TILE', 'TSM_CONV_CODE', 'TSM_TUNE_CACHE', 'TSM_STEM_POOL',
                      'TSM_STEM_DIRECT', 'TSM_STEM_PLANAR', 'TSM_POISON')


def _env(monkeypatch, env, poison):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if poison:
        monkeypatch.setenv('TSM_POISON', '1')


def _hostile_free(name, a):
    a = np.ascontiguousarray(a)
    assert not (a.view(np.uint32) == POISON).any(), f'{name}: holds the poison word'
    assert np.isfinite(a).all(), f'{name}: non-finite values'


def _outputs(eng, x, stages):
    return {**{s: eng.forward_tap(x, s) for s in stages}, 'logits': eng.run(None, {'input': x})[0]}


def _pair(monkeypatch, env, make, run):
    """run(engine) -> {name: ndarray} on a clean engine and on a TSM_POISON=1 engine (same knobs): bit-identical, free of
    poison and of non-finite values.  Returns the poisoned engine's outputs and its launch trace."""
    from workoutdetector_amd.engine import launch_trace
    _env(monkeypatch, env, False)
    eng = make()
    try:
        clean = run(eng)
    finally:
        eng.close()
    _env(monkeypatch, env, True)
    eng = make()
    try:
        with launch_trace() as tr:
            hostile = run(eng)
    finally:
        eng.close()
    assert clean.keys() == hostile.keys()
    for name in clean:
        _hostile_free(f'{name} (clean)', clean[name])
        _hostile_free(f'{name} (TSM_POISON=1)', hostile[name])
        assert np.array_equal(clean[name], hostile[name]), f'{name}: TSM_POISON=1 moved bits'
    return hostile, tr


_ORACLE = {}


def _oracle_bar(got, sd, x, t, dtype, what, capsys, key=None, ref=None):
    """The logits against the oracle at the bar of the existing engine tests; `ref(bf16)` -> logits for another backbone."""
    if key not in _ORACLE or key is None:
        xt = torch.from_numpy(x)
        if ref is not None:
            want, want16 = ref(False), (ref(True) if dtype == 'bf16' else None)
        else:
            want = tsm_oracle.tsm_forward(sd, xt, t).numpy()
            want16 = tsm_oracle.tsm_forward_bf16(sd, xt, t).numpy() if dtype == 'bf16' else None
        _ORACLE[key] = (want, want16)
    want, want16 = _ORACLE[key]
    if dtype == 'bf16':
        bf16_logits_report(got, want16, want, what, capsys)
    else:
        assert_close(got, want, rtol=1e-3, atol_scale=1e-5, what=what)


@pytest.fixture(scope='module')
def sd31():
    from workoutdetector_amd.weights import make_state_dict, to_torch
    sd = make_state_dict(31, 12)
    return sd, to_torch(sd)


def _r50(sd, h, w, b, t, dtype):
    from workoutdetector_amd.engine import TsmEngine
    return lambda: TsmEngine(num_segments=t, height=h, width=w, max_clips=b, state_dict=sd, dtype=dtype)


# ---- each fused form forced on, alone, in both walk directions --------------------------------------------------------------
@pytest.mark.parametrize('walk', ['0', '1'])
@pytest.mark.parametrize('form,dtype,h,w,b,t', ENGINE_PARAMS)
def test_fused_form_under_poison(hip_lib, monkeypatch, capsys, sd31, form, dtype, h, w, b, t, walk):
    sd, sdt = sd31
    x = make_input(1100 + h + t, b, t, h, w)
    knob, _, stage = FORMS[form]
    stages = R50_STAGES + [stage] + (['layer2.2.conv1'] if form == 'conv31' else [])
    env = {'TSM_AUTOTUNE': '0', 'TSM_WALK': walk, **{k: ('1' if k == knob else '0') for k in FUSE_KNOBS}}
    out, tr = _pair(monkeypatch, env, _r50(sd, h, w, b, t, dtype), lambda e: _outputs(e, x, stages))
    assert_ran(tr, _fused_kernel(form, dtype), f'{form} {dtype} under TSM_POISON=1')
    assert_walked(tr, walk == '1', f'{form} TSM_WALK={walk}')
    _oracle_bar(out['logits'], sdt, x, t, dtype, f'{form} {dtype} {h}x{w} T{t} poisoned', capsys, key=(dtype, h, w, b, t))


@pytest.mark.parametrize('walk', ['0', '1'])
@pytest.mark.parametrize('h,w,b,t', GEOMETRIES)
def test_weight_stationary_everywhere_under_poison(hip_lib, monkeypatch, capsys, sd31, h, w, b, t, walk):
    sd, sdt = sd31
    x = make_input(1100 + h + t, b, t, h, w)
    env = {'TSM_AUTOTUNE': '0', 'TSM_WALK': walk, 'TSM_CONV_TILE': 'ws', **{k: '0' for k in FUSE_KNOBS}}
    out, tr = _pair(monkeypatch, env, _r50(sd, h, w, b, t, 'bf16'), lambda e: _outputs(e, x, R50_STAGES))
    for fam in ('conv3x3_ws_kernel<false>', 'conv3x3_ws128_kernel<', 'conv1x1_ws_kernel<64>', 'conv1x1_ws_kernel<256>',
                'conv1x1_wsn_kernel<'):
        assert_ran(tr, fam, 'TSM_CONV_TILE=ws under TSM_POISON=1')
    assert_walked(tr, walk == '1', f'ws TSM_WALK={walk}')
    _oracle_bar(out['logits'], sdt, x, t, 'bf16', f'ws {h}x{w} T{t} poisoned', capsys, key=('bf16', h, w, b, t))


# ---- fp32 split-K and the tail split: d_partial poisoned ------------------------------------------------------------------------
@pytest.mark.parametrize('clips,code', [(2, 0x100 | 3), (2, 0x100 | 4), (14, 0x200 | 3), (27, 0x200 | 3)])
def test_split_k_and_tail_split_under_poison(hip_lib, monkeypatch, capsys, sd0, clips, code):
    """Clip counts 14 and 27 as in test_tail_split_is_bitwise_identical_to_whole_k, whose bar is bit-identity with whole K:
    asserted here too (against a clean whole-K engine); the 2-clip split-K cases also meet the oracle."""
    from workoutdetector_amd.engine import TsmEngine
    x = make_input(900 + clips, clips, 8, 224, 224)
    make = lambda: TsmEngine(height=224, width=224, max_clips=clips, state_dict=sd0)      # noqa: E731
    out, tr = _pair(monkeypatch, {'TSM_AUTOTUNE': '1', 'TSM_CONV_CODE': str(code), 'TSM_TUNE_CACHE': 'off'}, make,
                    lambda e: _outputs(e, x, R50_STAGES))
    assert_ran(tr, 'splitk_reduce_kernel', f'code {code:#x} at {clips} clips under TSM_POISON=1')
    _env(monkeypatch, {'TSM_AUTOTUNE': '1', 'TSM_CONV_CODE': '3', 'TSM_TUNE_CACHE': 'off'}, False)
    eng = make()
    try:
        whole = eng.run(None, {'input': x})[0]
    finally:
        eng.close()
    assert np.array_equal(out['logits'], whole), 'split form differs from whole K'
    if clips == 2:
        _oracle_bar(out['logits'], sd0, x, 8, 'f32', f'split-K code {code:#x} poisoned', capsys)


# ---- the tuned engine: the forward after a tuning pass ----------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['f32', 'bf16x3', 'bf16'])
def test_tuned_engine_under_poison(hip_lib, monkeypatch, capsys, sd0, dtype):
    from workoutdetector_amd.engine import TsmEngine
    x = make_input(77, 2, 8, 224, 224)
    make = lambda: TsmEngine(height=224, width=224, max_clips=2, state_dict=sd0, dtype=dtype)      # noqa: E731

    def run(eng):
        first = eng.run(None, {'input': x})[0]          # tunes the bucket, then the forward proper
        assert eng.conv_tiles(2), 'nothing was tuned'
        return {**_outputs(eng, x, R50_STAGES), 'first': first}

    out, tr = _pair(monkeypatch, {'TSM_AUTOTUNE': '1', 'TSM_TUNE_CACHE': 'off'}, make, run)
    assert np.array_equal(out['first'], out['logits'])
    _oracle_bar(out['logits'], sd0, x, 8, dtype, f'tuned {dtype} poisoned', capsys, key=('tuned', dtype))


# ---- fewer clips than capacity, and a changing count on one engine ----------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['f32', 'bf16x3', 'bf16'])
def test_changing_clip_count_under_poison(hip_lib, monkeypatch, capsys, sd31, dtype):
    """max_clips = 5; forwards of 5, 1, 3, 2, 5 clips on ONE poisoned engine, each against a fresh clean engine's result for
    that count: persistent grids of min(N, n_cu), per-clip tiles, the slack behind a short batch."""
    sd, sdt = sd31
    h, w, t = 64, 96, 4
    env = {'TSM_AUTOTUNE': '0'}
    xs = {n: make_input(500 + n, n, t, h, w) for n in (5, 1, 3, 2)}
    make = _r50(sd, h, w, 5, t, dtype)
    _env(monkeypatch, env, True)
    hostile = make()
    try:
        for i, n in enumerate((5, 1, 3, 2, 5)):
            got = _outputs(hostile, xs[n], R50_STAGES)
            _env(monkeypatch, env, False)
            clean = make()
            try:
                want = _outputs(clean, xs[n], R50_STAGES)
            finally:
                clean.close()
            for name in want:
                _hostile_free(f'forward {i} ({n} clips) {name}', got[name])
                assert np.array_equal(got[name], want[name]), f'forward {i} ({n} clips): {name} differs from a fresh clean engine'
            _oracle_bar(got['logits'], sdt, xs[n], t, dtype, f'{n} of 5 clips {dtype} poisoned', capsys, key=('count', dtype, n))
    finally:
        hostile.close()


# ---- the packed-input paths at an odd width, and the stem switches -----------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['f32', 'bf16x3', 'bf16'])
def test_packed_input_at_an_odd_width_under_poison(hip_lib, monkeypatch, capsys, sd31, dtype):
    """Frames written by tsm_preprocess (LAYOUT_NTHWC4 / 8S / 8B), 65 x 65: the pad pixel of the last pixel pair is
    tsm_preprocess's, not pack_input_kernel's."""
    from workoutdetector_amd.engine import TsmEngine, preprocess_frames
    sd, sdt = sd31
    crop, t, b = 65, 4, 2
    vid = torch.from_numpy(np.random.default_rng(65).integers(0, 256, size=(b * t, 90, 110, 3), dtype=np.uint8)).cuda()
    nchw = preprocess_frames(vid, resize=72, crop=crop, packed=False, scale_255=True)
    x = nchw.cpu().numpy().reshape(b, t, 3, crop, crop)
    make = lambda: TsmEngine(num_segments=t, height=crop, width=crop, max_clips=b, state_dict=sd, dtype=dtype)      # noqa: E731

    def run(eng):
        packed = preprocess_frames(vid, resize=72, crop=crop, layout=eng.packed_layout, scale_255=True)
        dev = eng.forward_device(packed.reshape((b, t) + tuple(packed.shape[1:])), layout=eng.packed_layout).cpu().numpy()
        return {**_outputs(eng, x, R50_STAGES), 'packed logits': dev}

    out, _ = _pair(monkeypatch, {'TSM_AUTOTUNE': '0'}, make, run)
    _oracle_bar(out['packed logits'], sdt, x, t, dtype, f'packed 65x65 {dtype} poisoned', capsys, key=('packed', dtype))
    _oracle_bar(out['logits'], sdt, x, t, dtype, f'65x65 {dtype} poisoned', capsys, key=('packed', dtype))


@pytest.mark.parametrize('knob', ['TSM_STEM_POOL', 'TSM_STEM_DIRECT', 'TSM_STEM_PLANAR'])
def test_stem_switches_under_poison(hip_lib, monkeypatch, capsys, sd31, knob):
    sd, sdt = sd31
    h, w, b, t = 64, 97, 2, 4
    x = make_input(640 + w, b, t, h, w)
    out, tr = _pair(monkeypatch, {'TSM_AUTOTUNE': '0', knob: '0'}, _r50(sd, h, w, b, t, 'bf16'),
                    lambda e: _outputs(e, x, ['conv1'] + R50_STAGES))
    if knob == 'TSM_STEM_POOL':
        assert_ran(tr, 'maxpool3x3s2_kernel', knob)
    if knob == 'TSM_STEM_PLANAR':
        assert_ran(tr, 'pack_input_kernel', knob)
    _oracle_bar(out['logits'], sdt, x, t, 'bf16', f'{knob}=0 poisoned', capsys, key=('stem', h, w))


# ---- the other backbones and placement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('base_model,place,dtype', [('resnet18', 'blockres', 'f32'), ('wide_resnet50_2', 'blockres', 'bf16'),
                                                    ('resnet50', 'block', 'bf16')])
def test_other_backbones_under_poison(hip_lib, monkeypatch, capsys, base_model, place, dtype):
    from workoutdetector_amd.engine import TsmEngine
    from workoutdetector_amd.weights import make_state_dict
    h, w, b, t = 112, 128, 2, 8
    sd = make_state_dict(0, 12, base_model=base_model, shift_place=place)
    sdt = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    x = make_input(41 + t, b, t, h, w)
    xt = torch.from_numpy(x)
    make = lambda: TsmEngine(num_segments=t, height=h, width=w, max_clips=b, state_dict=sd, dtype=dtype,      # noqa: E731
                             base_model=base_model, shift_place=place)
    stages = R18_STAGES if base_model == 'resnet18' else R50_STAGES
    out, _ = _pair(monkeypatch, {'TSM_TUNE_CACHE': 'off'}, make, lambda e: _outputs(e, x, stages))
    ref = lambda bf16: tsm_oracle.forward(sdt, xt, base_model, place, bf16, n_segment=t).numpy()      # noqa: E731
    _oracle_bar(out['logits'], sdt, x, t, dtype, f'{base_model} {place} {dtype} poisoned', capsys, ref=ref)
