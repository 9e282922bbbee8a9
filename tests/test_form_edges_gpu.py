"""Engines on both sides of every fused form's geometry rule (the case table: tests/_form_edges.py; that the table is AT the
clauses of csrc/tsm_conv_rules.h: tests/test_form_edges_cpu.py).

Every engine-level test of bneck_ws, front_s2, the conv31 family and conv3x3_ws_kernel<true> otherwise runs where every form is
valid: layer1 maps of at most 64 columns, T in {4, 8, 16}.  Here the frames cross layer1's 64-column clause (32 x 256 | 257 | 264),
the 128-column tile cap (32 x 520), stay tall where they must NOT cross it (256 | 257 | 520 x 32), sit on both sides of the
front's even-height clause (36 | 40 x 64), and T runs through 1, 2 (tiles larger than the map), 3, 5, 6, 12 (no tile size
divides), 32 (conv31_fused valid, both conv31_pc invalid) and 64 (none).

a. a bf16 engine with ONE form forced: the form's kernel is in the launch trace if and only if the table says valid (and as
   often as the form has blocks), the timing slots it leaves unrecorded are exactly those of the launches it replaces, and the
   logits and taps equal the all-separate engine's bit for bit -- outside the envelope because the very same launches ran.
   (conv_tiles carries a fusion suffix for a TUNED form only -- a forced one is no tuner choice --, so under TSM_AUTOTUNE=0 it
   must report none; "a suffix exactly where the kernel ran" is asserted in c and d, where codes exist.)
b. the all-separate engine of every dtype is RIGHT at these frames: against the CPU oracle at the bars of tests/test_bf16_gpu.py,
   tests/test_engine_gpu.py and tests/test_bf16x3_gpu.py.
c. a tune-cache line that carries the bit of a form which cannot run is accepted, and the form does not run.
d. left to the tuner: the same bits, and only forms the table allows.

All engines run in hostile memory (TSM_POISON=1): a kernel that wrote outside its tensor fails the call."""
import numpy as np
import pytest
import torch

from oracle import tsm_oracle
from tests import _form_edges as fe
from tests._util import BF16_E2E_BAR, BF16_TAP_BAR, assert_close, assert_fused_slots, bf16_logits_report, make_input
from tests.test_poison_gpu import KNOBS
from tests.test_walk_gpu import FORMS, FUSE_KNOBS

pytestmark = pytest.mark.gpu

IDS = [c['id'] for c in fe.CASES]
BF16_TAPS = ('layer1.2', 'layer2.3', 'layer3.5')
F32_TAPS = ('stem', 'layer1.2', 'layer2.3', 'layer4.2')
# the taps compared bit for bit per engine form: FORMS' stage, and for conv31 one conv1 output (the fused launch's second
# result) of each instantiation
FORM_TAPS = {'block': ('layer1.1',), 'front': ('layer2.0.conv2',), 'conv23': ('layer1.1',),
             'conv31': ('layer2.1', 'layer2.2.conv1', 'layer3.0.conv1', 'layer3.2.conv1', 'layer2.3', 'layer3.5')}
assert all(FORM_TAPS[f][0] == FORMS[f][2] for f in FORMS)
ALL_TAPS = tuple(dict.fromkeys(t for taps in FORM_TAPS.values() for t in taps)) + ('layer1.2',)
# tsm_host_util.h: kCodeBlock (on conv1: the whole Bottleneck as one launch), kCodeConv31 (on conv3: + the next block's conv1)
CODE_BLOCK, CODE_CONV31 = 0x800, 0x1000
SUFFIX_KERNELS = {'+block': 'bneck_ws_kernel<', '+conv2': 'front_s2_kernel<', '+conv1': 'conv31_'}   # ('+conv3': by dtype)


def _env(monkeypatch, **env):
    """Every engine here: the knobs cleared, then TSM_POISON=1, the tune cache off and what `env` says (monkeypatch restores)."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('TSM_POISON', '1')
    monkeypatch.setenv('TSM_TUNE_CACHE', 'off')
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _forced(monkeypatch, form):
    """TSM_AUTOTUNE=0 and `form`'s knob at 1, the other three at 0 (form None: all four at 0)."""
    _env(monkeypatch, TSM_AUTOTUNE='0', **{k: '1' if form and k == FORMS[form][0] else '0' for k in FUSE_KNOBS})


def _engine(sd, c, dtype='bf16'):
    from workoutdetector_amd.engine import TsmEngine
    return TsmEngine(num_segments=c['T'], height=c['h'], width=c['w'], max_clips=c['clips'], state_dict=sd, dtype=dtype)


def _input(c):
    return make_input(fe.SEEDS[c['id']], c['clips'], c['T'], c['h'], c['w'])


_SEPARATE, _ORACLE = {}, {}


def _separate(monkeypatch, sd, c):
    """Logits and ALL_TAPS of the bf16 engine with all four forms off at case `c`: computed once per case, never changed."""
    if c['id'] not in _SEPARATE:
        from workoutdetector_amd.engine import launch_trace
        _forced(monkeypatch, None)
        eng = _engine(sd, c)
        try:
            x = _input(c)
            with launch_trace() as tr:
                out = {'logits': eng.run(None, {'input': x})[0]}
            for kern in ('bneck_ws_kernel<', 'front_s2_kernel<', 'conv31_', 'conv3x3_ws_kernel<true>'):
                assert not tr.ran(kern), (c['id'], kern)
            assert_fused_slots(eng, x, set(), c['id'] + ' separate')
            out.update({s: eng.forward_tap(x, s) for s in ALL_TAPS})
        finally:
            eng.close()
        for v in out.values():
            v.setflags(write=False)
        _SEPARATE[c['id']] = out
    return _SEPARATE[c['id']]


def _oracle(sd, c, bf16):
    """(logits, taps) of the CPU oracle at the case's frame and T: once per (h, w, T, clips) and storage format."""
    key = (c['h'], c['w'], c['T'], c['clips'], bf16)
    if key not in _ORACLE:
        taps = {}
        fn = tsm_oracle.tsm_forward_bf16 if bf16 else tsm_oracle.tsm_forward
        logits = fn(sd, torch.from_numpy(_input(c)), n_segment=c['T'], taps=taps).numpy()
        keep = BF16_TAPS if bf16 else F32_TAPS
        _ORACLE[key] = (logits, {s: taps[s].permute(0, 2, 3, 1).numpy() for s in keep})
    return _ORACLE[key]


def _expected(c, form):
    """What the table says a forward with `form` forced launches: {kernel prefix: (mark in the line, count)} and the conv
    launches the fused ones take over."""
    kernels, away = {}, set()
    v = c['forms']
    if form == 'block':
        kernels['bneck_ws_kernel<'] = ('', 3 if v['block'][0] else 0)
        away = {f'layer1.{b}.{p}' for b in range(3) for p in ('conv2', 'conv3')} if v['block'][0] else set()
    elif form == 'front':
        kernels['front_s2_kernel<'] = ('', 1 if v['front'][0] else 0)
        away = {'layer2.0.conv2'} if v['front'][0] else set()
    elif form == 'conv23':
        kernels['conv3x3_ws_kernel<true>'] = ('', 2 if v['conv23'][0] else 0)
        away = {'layer1.1.conv3', 'layer1.2.conv3'} if v['conv23'][0] else set()
    else:
        for name, (prefix, mark, count, conv1s) in fe.CONV31_KERNELS.items():
            kernels[(prefix, mark)] = (mark, count if v[name][0] else 0)
            away |= set(conv1s) if v[name][0] else set()
    return kernels, away


def _count(tr, prefix, mark):
    return sum(k.startswith(prefix) and mark in k for k in tr.kernels)


# ---- a. one form forced, both sides of its rule ---------------------------------------------------------------------------------
@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('case_id', IDS)
def test_forced_form_runs_exactly_inside_its_envelope(hip_lib, sd0, monkeypatch, case_id, form):
    from workoutdetector_amd.engine import launch_trace
    c = fe.case(case_id)
    want = _separate(monkeypatch, sd0, c)
    kernels, away = _expected(c, form)
    x = _input(c)
    _forced(monkeypatch, form)
    eng = _engine(sd0, c)
    try:
        with launch_trace() as tr:
            logits = eng.run(None, {'input': x})[0]
        lines = sorted(set(tr.kernels))
        for key, (mark, count) in kernels.items():
            prefix = key if isinstance(key, str) else key[0]
            assert _count(tr, prefix, mark) == count, (case_id, form, prefix, mark, count, lines)
        if form == 'conv31' and c['T'] == 32:     # the 256-row kernel alone
            assert tr.ran('conv31_fused_kernel<') and not tr.ran('conv31_pc_kernel<'), lines
        for other in set(FORMS) - {form}:         # and no other form
            kern = 'conv3x3_ws_kernel<true>' if other == 'conv23' else FORMS[other][1]
            assert not tr.ran(kern), (case_id, form, kern, lines)
        assert_fused_slots(eng, x, away, f'{case_id} {form}')
        # a forced form is no tuner choice: conv_tiles (no codes under TSM_AUTOTUNE=0) carries no suffix
        assert not any('+' in v for v in eng.conv_tiles(c['clips']).values()), eng.conv_tiles(c['clips'])
        assert np.array_equal(logits, want['logits']), (case_id, form, 'logits differ from the separate launches')
        for stage in FORM_TAPS[form]:
            with launch_trace() as tr:
                got = eng.forward_tap(x, stage)
            assert np.array_equal(got, want[stage]), (case_id, form, stage)
            if stage == FORMS[form][2]:           # the form's own tap still runs the kernel where it may
                for key, (mark, count) in kernels.items():
                    prefix = key if isinstance(key, str) else key[0]
                    if form != 'conv31' or key[0] == 'conv31_fused_kernel<':
                        assert tr.ran(prefix) == (count > 0), (case_id, form, stage, sorted(set(tr.kernels)))
    finally:
        eng.close()
    assert np.isfinite(logits).all()


# ---- b. the all-separate engine is right at these frames ------------------------------------------------------------------------
FRAME_IDS = [next(c['id'] for c in fe.CASES if (c['h'], c['w'], c['T'], c['clips']) == k) for k in fe.frames_tsq()]


@pytest.mark.parametrize('case_id', FRAME_IDS)
def test_separate_bf16_engine_against_the_bf16_oracle(hip_lib, sd0, monkeypatch, capsys, case_id):
    c = fe.case(case_id)
    got = _separate(monkeypatch, sd0, c)
    want_f32, _ = _oracle(sd0, c, False)
    want, taps = _oracle(sd0, c, True)
    # the arg-max the report asks for is defined: the oracle's two largest logits of a clip are further apart than two values
    # inside the bar can move (tests/_form_edges.py: SEEDS)
    for ref in (want, want_f32):
        top = np.sort(np.asarray(ref, dtype=np.float64), axis=1)
        assert ((top[:, -1] - top[:, -2]) / float(np.abs(want_f32).max())).min() > 2 * BF16_E2E_BAR, (case_id, top[:, -2:])
    bf16_logits_report(got['logits'], want, want_f32, f'bf16 {case_id}', capsys)
    for stage in BF16_TAPS:
        e = float(np.abs(got[stage] - taps[stage]).max()) / float(np.abs(taps[stage]).max())
        with capsys.disabled():
            print(f'[bf16 {case_id}] {stage}: max|err|/scale = {e:.3g} vs the bf16-storage oracle (bar {BF16_TAP_BAR:g})')
        assert got[stage].shape == taps[stage].shape and e <= BF16_TAP_BAR, (case_id, stage, e)


@pytest.mark.parametrize('dtype', ['f32', 'bf16x3'])
@pytest.mark.parametrize('case_id', FRAME_IDS)
def test_separate_fp32_engines_against_the_oracle(hip_lib, sd0, monkeypatch, capsys, case_id, dtype):
    c = fe.case(case_id)
    want, taps = _oracle(sd0, c, False)
    x = _input(c)
    _forced(monkeypatch, None)
    eng = _engine(sd0, c, dtype)
    try:
        worst = {'logits': assert_close(eng.run(None, {'input': x})[0], want, rtol=1e-3, atol_scale=1e-5, what=f'{dtype} {case_id} logits')}
        for stage in F32_TAPS:
            worst[stage] = assert_close(eng.forward_tap(x, stage), taps[stage], rtol=1e-3, atol_scale=1e-5 if dtype == 'f32' else 3e-5,
                                        what=f'{dtype} {case_id} {stage}')
    finally:
        eng.close()
    with capsys.disabled():
        print(f'\n[{dtype} {case_id}] max|err|/scale: ' + ', '.join(f'{k} {v:.3g}' for k, v in worst.items()))


# ---- c. the cached bit of a form that cannot run --------------------------------------------------------------------------------
@pytest.mark.parametrize('case_id,layer,bit,kernel,suffix', [('32x257', 'layer1.1.conv1', CODE_BLOCK, 'bneck_ws_kernel<', '+block'),
                                                             ('T3', 'layer2.1.conv3', CODE_CONV31, 'conv31_', '+conv1')])
def test_tune_cache_bit_of_a_form_outside_its_envelope(hip_lib, sd0, tmp_path, monkeypatch, case_id, layer, bit, kernel, suffix):
    """As test_tune_cache_fusion_bit_of_a_form_that_cannot_run (tests/test_engine_gpu.py), for the whole-block bit where layer1
    has 65 columns and the conv3 + conv1 bit at T = 3: the line is read back, the forward keeps the separate launches, conv_tiles
    reports what ran, and not a bit of the result moves."""
    from workoutdetector_amd.engine import launch_trace
    from workoutdetector_amd.weights import BACKBONES
    c = fe.case(case_id)
    assert not c['forms']['block' if suffix == '+block' else 'conv31_l2'][0]
    path = tmp_path / 'tiles.txt'
    _env(monkeypatch, TSM_TUNE_CACHE=str(path))
    x = _input(c)
    a = _engine(sd0, c)
    try:
        ya = a.run(None, {'input': x})[0]
    finally:
        a.close()
    key, codes = path.read_text().splitlines()[0].rsplit('|', 1)
    codes = [int(v) for v in codes.split(',')]
    # the line is in the engine's layer order: stem, then per block conv1, conv2, conv3 (, downsample)
    order = ['conv1'] + [f'layer{li}.{b}.{part}' for li, nb in enumerate(BACKBONES['resnet50'][0], 1) for b in range(nb)
                         for part in ('conv1', 'conv2', 'conv3') + (('downsample',) if b == 0 else ())]
    assert len(order) == len(codes) and not codes[order.index(layer)] & bit
    codes[order.index(layer)] |= bit
    path.write_text(key + '|' + ','.join(str(v) for v in codes) + '\n')
    b = _engine(sd0, c)
    try:
        with launch_trace() as tr:
            yb = b.run(None, {'input': x})[0]
        tiles = b.conv_tiles(c['clips'])
    finally:
        b.close()
    assert len(path.read_text().splitlines()) == 1, 'the edited line was rejected and the engine tuned again'
    assert not tr.ran(kernel), sorted(set(tr.kernels))
    assert suffix not in tiles[layer], tiles[layer]
    assert np.array_equal(ya, yb)
    assert np.array_equal(ya, _separate(monkeypatch, sd0, c)['logits'])


# ---- d. left to the tuner -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case_id', ['32x256', '32x257', 'T32'])
def test_tuner_picks_only_forms_the_table_allows(hip_lib, sd0, monkeypatch, capsys, case_id):
    from workoutdetector_amd.engine import launch_trace
    c = fe.case(case_id)
    want = _separate(monkeypatch, sd0, c)['logits']
    _env(monkeypatch)                  # TSM_AUTOTUNE and the four forms at their defaults, the cache off
    x = _input(c)
    eng = _engine(sd0, c)
    try:
        eng.run(None, {'input': x})    # (the tuning pass)
        with launch_trace() as tr:
            got = eng.run(None, {'input': x})[0]
        tiles = eng.conv_tiles(c['clips'])
        assert_fused_slots(eng, x, set(), case_id + ' tuned')
    finally:
        eng.close()
    assert np.array_equal(got, want), case_id
    picked = {k: v for k, v in tiles.items() if '+' in v}
    with capsys.disabled():
        print(f'\n[{case_id}] fused forms the tuner picked: {picked}')
    v = c['forms']
    conv31_of = fe.CONV31_OF
    for layer, name in picked.items():
        if '+block' in name:
            assert v['block'][0] and layer in ('layer1.0.conv1', 'layer1.1.conv1', 'layer1.2.conv1'), (layer, name)
        if '+conv2' in name:
            assert v['front'][0] and layer == 'layer2.0.conv1', (layer, name)
        if '+conv3' in name:
            assert v['conv23'][0] and layer in ('layer1.1.conv2', 'layer1.2.conv2'), (layer, name)
        if '+conv1' in name:
            assert layer in conv31_of and v[conv31_of[layer]][0], (layer, name)
    # a suffix exactly where the kernel ran
    for suffix, kern in dict(SUFFIX_KERNELS, **{'+conv3': 'conv3x3_ws_kernel<true>'}).items():
        assert tr.ran(kern) == any(suffix in name for name in picked.values()), (suffix, kern, picked, sorted(set(tr.kernels)))
    for name, (prefix, mark, _, conv1s) in fe.CONV31_KERNELS.items():
        n_picked = sum(conv31_of.get(layer) == name for layer, t in picked.items() if '+conv1' in t)
        assert _count(tr, prefix, mark) == n_picked, (name, picked, sorted(set(tr.kernels)))
