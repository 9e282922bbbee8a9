"""base_model='tdn_resnet50' without a GPU: tests/_tdn.py (written from the header's definition) against the reference's outputs in
tests/golden/ref_tdn.npz, the conditions that keep the GPU tests from passing by luck, the nearest-index formula, the key remap,
every refusal that never reaches the library, the new export in the header, the library and the binding, the new kernels' figures
in the built code object, the FLOP table, and the pure-host arithmetic under ASAN + UBSAN (tests/tdn_host.cpp)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _tdn
from workoutdetector_amd import engine, flops, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET = dict(num_class=7, T=3, depths=(1, 2, 1, 2), seed=5, clips=2, H=96, W=160)      # tests/golden/make_tdn_vectors.py
LOGITS_BAR = 1e-5      # the GPU tests' logits bar, as a fraction of the scale (tests/test_tdn_gpu.py)


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'ref_tdn.npz'))


@pytest.fixture(scope='module')
def net():
    """The fixture's network in float64, its input, logits and taps -- computed once, left unchanged."""
    model, w = _tdn.build(NET['num_class'], NET['T'], NET['depths'], NET['seed'])
    x = torch.from_numpy(_tdn.make_input(NET['seed'], NET['clips'], NET['T'], NET['H'], NET['W']))
    with torch.no_grad():
        logits, taps = model(x, taps=True)
    return dict(model=model, weights=w, x=x, logits=logits.numpy(), taps=taps)


def close(got, want, rel=1e-12):
    return np.abs(np.asarray(got) - want).max() <= rel * np.abs(want).max()


# ---- the test model is the reference's network ----------------------------------------------------------------------------
def test_modules_reproduce_the_reference(golden):
    x = torch.from_numpy(np.random.default_rng(21).standard_normal((6, 128, 5, 6)))
    with torch.no_grad():
        mse = _tdn.MSE(128, 3).double()
        _tdn.load(mse, _tdn.draw_weights(mse, 11))
        assert close(mse(x).numpy(), golden['mse_out'])
        shift = _tdn.Shift(128, 3).double()
        _tdn.load(shift, _tdn.draw_weights(shift, 12))
        assert close(shift(x).numpy(), golden['shift_out'])
        assert not close(shift(x).numpy(), x.numpy(), 1e-3)


def test_network_reproduces_the_reference(golden, net):
    assert golden['logits'].shape == (2, 7) and golden['features'].shape == (6, 2048)
    assert close(net['logits'], golden['logits']) and close(net['taps']['features'], golden['features'])
    names = [k[4:] for k in golden.files if k.startswith('tap:')]
    assert len(names) >= 10
    for name in names:
        tap = net['taps'][name]
        assert tuple(golden['shape:' + name]) == tap.shape, name
        assert close(tap.reshape(-1)[::97], golden['tap:' + name]), name
    assert net['taps']['layer4.1.mse.fwd'].shape == (6, 3, 5, 32) and net['taps']['layer3.0.conv1'].shape == (6, 12, 20, 256)   # odd maps: 5 -> 2, 3 -> 1


# ---- conditions on the test inputs ----------------------------------------------------------------------------------------
def test_gates_are_neither_saturated_nor_flat(net):
    es = {k: v.numpy() for k, v in net['taps'].items() if k.endswith('.mse.e')}
    assert len(es) == 5
    for name, e in es.items():
        print(name, 'share |e| > 4: %.3f' % (np.abs(e) > 4).mean(), 'std %.2f' % e.std())
        assert (np.abs(e) > 4).mean() <= 0.10 and e.std() >= 0.3, name


def _ablated(net, change):
    model, _w = _tdn.build(NET['num_class'], NET['T'], NET['depths'], NET['seed'])
    change(model)
    with torch.no_grad():
        out = model(net['x']).numpy()
    return np.abs(out - net['logits']).max() / np.abs(net['logits']).max()


def _zero_tap(k):
    def change(model):
        for m in model.modules():
            if isinstance(m, _tdn.Shift):
                m.conv.weight.data[:, :, k] = 0
    return change


def _set(cls, **attrs):
    def change(model):
        for m in model.modules():
            if isinstance(m, cls):
                for k, v in attrs.items():
                    setattr(m, k, v)
    return change


@pytest.mark.parametrize('name, change', [('gate removed', _set(_tdn.MSE, gate=False)), ('beta = 0', _set(_tdn.Base, beta=0.0)),
                                          ('tap 0 zeroed', _zero_tap(0)), ('tap 1 zeroed', _zero_tap(1)), ('tap 2 zeroed', _zero_tap(2)),
                                          ('zero ends swapped', _set(_tdn.MSE, swap_ends=True))])
def test_every_part_moves_the_logits(net, name, change):
    moved = _ablated(net, change)
    print(name, 'moves the logits by %.3g of the scale' % moved)
    assert moved > 100 * LOGITS_BAR


def test_nearest_index_is_torchs():
    for n_in in range(1, 65):
        src = torch.arange(n_in, dtype=torch.float32).view(1, 1, 1, n_in)
        for n_out in range(1, 65):
            want = F.interpolate(src, size=(1, n_out)).view(-1).long().tolist()
            assert [_tdn.nearest_index(i, n_in, n_out) for i in range(n_out)] == want, (n_in, n_out)
    t = torch.randn(2, 3, 3, 2)
    assert torch.equal(_tdn.up(t, (7, 5)), F.interpolate(t, (7, 5)))


# ---- keys -----------------------------------------------------------------------------------------------------------------
def test_specs_are_the_models_keys(net):
    want = {k: tuple(v.shape) for k, v in net['model'].state_dict().items() if 'num_batches_tracked' not in k and 'conv1_temp' not in k}
    specs = weights.tdn_specs(NET['depths']) + [('new_fc.weight', (7, 2048), 'fc'), ('new_fc.bias', (7,), 'bias')]
    assert {k: s for k, s, _ in specs} == want
    assert len(weights.tdn_specs()) > len(weights.tdn_specs(NET['depths']))
    sd = weights.make_tdn_state_dict(3, 7, NET['depths'])
    assert {k: v.shape for k, v in sd.items()} == want and all(v.dtype == np.float32 for v in sd.values())
    assert weights.tdn_alpha_beta(8) == (0.5, 0.5) and weights.tdn_alpha_beta(3) == (0.75, 0.25) and weights.tdn_alpha_beta(16) == (0.75, 0.25)
    for bad in ((3, 4, 6), (3, 0, 6, 3), (3, 4, 65, 3)):
        with pytest.raises(ValueError):
            weights.tdn_specs(bad)


def test_key_remap(net):
    w = net['weights']
    plain = weights.remap_tdn_keys(w, 7, NET['depths'])
    assert set(plain) == set(w) and 'base_model.conv1_temp.weight' in plain
    wrapped = {'state_dict': {'module.' + k: v for k, v in w.items()}}
    wrapped['state_dict']['module.base_model.bn1.num_batches_tracked'] = np.zeros(())
    wrapped['state_dict']['module.something.else'] = np.zeros(3)
    out = weights.remap_tdn_keys(wrapped, 7, NET['depths'])
    assert set(out) == set(w) | {'base_model.bn1.num_batches_tracked'} and all(out[k] is w[k] for k in w)
    net_spelling = {k.replace('.conv1.weight', '.conv1.net.weight') if '_bak.' in k and '.mse.' not in k else k: v for k, v in w.items()}
    assert any('.net.' in k for k in net_spelling)
    out = weights.remap_tdn_keys(net_spelling, 7, NET['depths'])
    assert set(out) == set(w)
    with pytest.raises(ValueError, match=r'\[7, 2048\].*\[12, 2048\]'):
        weights.remap_tdn_keys(w, 12, NET['depths'])


# ---- refusals, all before the library loads -------------------------------------------------------------------------------
def test_refusals_come_before_the_library(monkeypatch):
    from workoutdetector_amd import _lib, inference_count

    def no_library():
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(_lib, 'load', no_library)
    with pytest.raises(NotImplementedError, match='resnet50'):
        engine.create_tdn_model(12, base_model='resnet101')
    for dtype in ('bf16x3', 'bf16'):
        with pytest.raises(NotImplementedError, match="dtype='f32' only"):
            engine.create_tdn_model(12, dtype=dtype)
        with pytest.raises(NotImplementedError, match="dtype='f32' only"):
            engine.TsmEngine(base_model='tdn_resnet50', is_shift=False, dtype=dtype)
    with pytest.raises(NotImplementedError, match='onnx'):
        engine.create_tdn_model(12, checkpoint='tdn.onnx')
    with pytest.raises(NotImplementedError, match='num_frames'):
        engine.create_tdn_model(12, num_frames=3)
    with pytest.raises(ValueError, match='is_shift=False'):
        engine.TsmEngine(base_model='tdn_resnet50')
    with pytest.raises(ValueError, match='num_segments'):
        engine.TsmEngine(base_model='tdn_resnet50', is_shift=False, num_segments=1)
    for h, w in ((32, 64), (224, 200), (100, 224)):
        with pytest.raises(ValueError, match='multiples of 32'):
            engine.TsmEngine(base_model='tdn_resnet50', is_shift=False, height=h, width=w)
    with pytest.raises(NotImplementedError):
        engine.TsmEngine(base_model='tdn_resnet50', is_shift=False, non_local=True)
    with pytest.raises(ValueError, match='tdn_depths'):
        engine.TsmEngine(base_model='resnet50', tdn_depths=(1, 1, 1, 1))
    with pytest.raises(ValueError):
        engine.TsmEngine(base_model='tdn_resnet50', is_shift=False, tdn_depths=(1, 1, 1))

    class Tdn:      # what the pipelines see of a TDN engine
        tdn_depths = (3, 4, 6, 3)
        consensus_type = 'avg'
    for where in ('inference_dataset', 'StreamBatcher', 'eval_classification', 'count_by_video_model'):
        with pytest.raises(NotImplementedError, match='five'):
            inference_count.need_clip_rows(Tdn(), where)
    from workoutdetector_amd import classification, streaming
    with pytest.raises(NotImplementedError, match='five'):
        streaming.StreamBatcher(Tdn())
    with pytest.raises(NotImplementedError, match='five'):
        classification.eval_classification(Tdn(), [])
    with pytest.raises(NotImplementedError, match='five'):
        inference_count.inference_dataset(Tdn(), ['test'], 'out', 'ckpt')


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def test_the_setter_is_declared_exported_and_bound():
    from workoutdetector_amd import _lib
    from workoutdetector_amd.build import LIB_PATH, build_library
    build_library()
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'tsm_hip.h')).read(), flags=re.S)
    assert re.search(r'int\s+tsm_set_tdn\(tsm_engine \*e, const int32_t depths\[4\], float alpha, float beta\);', text)
    protos = re.findall(r'[^;{}]*\btsm_[a-z0-9_]+\s*\([^;]*\);', text)
    assert not [p for p in protos if 'tsm_set_tdn' in p and 'stream' in p]
    assert 'tsm_set_tdn' in _lib.EXPORTS
    out = subprocess.run(['nm', '-D', '--defined-only', LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r' T tsm_set_tdn$', out, flags=re.M)
    lib = _lib.load()
    assert lib.tsm_set_tdn.restype is ctypes.c_int and len(lib.tsm_set_tdn.argtypes) == 4
    assert lib.tsm_abi_version() == 7
    assert lib.tsm_set_tdn(None, (ctypes.c_int32 * 4)(3, 4, 6, 3), 0.5, 0.5) == -1          # no engine: refused, nothing touched


# ---- code object ----------------------------------------------------------------------------------------------------------
def test_new_kernels_use_no_scratch():
    """Every new kernel: no scratch, no spill; LDS only where the design stages something (the front end's 21 x 21 x 12 tile, the
    squeeze's 16 KB of rows); mse_excite_shift_kernel<512> keeps its 128 weight registers and still fits two waves per SIMD."""
    from workoutdetector_amd import codeobj
    from workoutdetector_amd.build import build_library
    md = codeobj.kernel_metadata(build_library())
    names = ['tdn_front_kernel', 'tdn_fuse_kernel'] + [f'{k}<{r}>' for k in ('mse_squeeze_kernel', 'mse_diff_kernel', 'mse_s2_kernel', 'mse_mix_kernel')
                                                       for r in (8, 16, 32)] + [f'mse_excite_shift_kernel<{c}>' for c in (128, 256, 512)]
    for name in names:
        r = md[name]
        assert r['.private_segment_fixed_size'] == 0 and r['.vgpr_spill_count'] == 0 and r['.sgpr_spill_count'] == 0, (name, r)
        lds = 21 * 21 * 12 * 4 if name == 'tdn_front_kernel' else 16384 if name.startswith('mse_squeeze') else 0
        assert r['.group_segment_fixed_size'] == lds, (name, r['.group_segment_fixed_size'])
    assert md['mse_excite_shift_kernel<512>']['.vgpr_count'] >= 128 and md['mse_excite_shift_kernel<512>']['waves_per_simd'] >= 2
    # 74: tdn_front_kernel's count at commit 2cac9cf, read from a build with these flags; a rewrite must not cost registers (DESIGN_HISTORY.md H7)
    assert md['tdn_front_kernel']['.vgpr_count'] <= 74, md['tdn_front_kernel']


def test_conv1s_output_has_two_readers_and_o_one_writer():
    """The schedule of the long-term module as the engine's code spells it (Forward::run_mse): conv1's output t1 goes to the squeeze
    and to the excite launch and nowhere else; obuf (o) is written by the excite launch alone; every other operand is one of the
    r-channel maps q[..].  tests/test_tdn_gpu.py checks the same launches in the trace."""
    src = open(os.path.join(ROOT, 'workoutdetector_amd', 'csrc', 'tsm_engine.hip')).read()
    body = src[src.index('int Forward::run_mse('):]
    body = body[:body.index('\n}\n')]
    launches = re.findall(r'tsm::(launch_\w+)\(([^;]*)\);', body)
    assert [name for name, _ in launches] == ['launch_mse_squeeze', 'launch_mse_diff', 'launch_mse_s2', 'launch_mse_mix', 'launch_mse_excite_shift']
    args = {name: [a.strip() for a in a_[:-1].split(',')] for name, a_ in launches}      # (a_ ends with TSM_LAUNCH's own bracket)
    assert [name for name, a in args.items() if 't1' in a] == ['launch_mse_squeeze', 'launch_mse_excite_shift']
    assert [name for name, a in args.items() if 'obuf' in a] == ['launch_mse_excite_shift']
    assert args['launch_mse_squeeze'][0] == 't1' and args['launch_mse_excite_shift'][0] == 't1' and args['launch_mse_excite_shift'][6] == 'obuf'
    for name in ('launch_mse_diff', 'launch_mse_s2', 'launch_mse_mix'):
        assert all(a.startswith(('q[', 'm.d_')) or a in ('nn', 'T', 'hh', 'ww', 'hq', 'wq', 'c', 's') for a in args[name]), args[name]
    # conv2 reads o: run_block / tune_block point conv2 (alone or fused with conv3) at obuf for a block with a long-term module
    assert src.count('if (blk.mse >= 0) L.p2.x = L.pf.x = obuf;') == 2


# ---- FLOPs ----------------------------------------------------------------------------------------------------------------
def test_flop_table():
    rows = flops.tdn_table(224, 224)
    for r in rows:
        assert r['macs'] == r['m'] * r['cout'] * r['cin'] * r['k'] ** (1 if r.get('one_d') else 2), r
    by = {r['name']: r for r in rows}
    assert by['diff.conv1_5']['m'] == 56 * 56 and by['resnext_layer1.0.conv2']['m'] == 28 * 28 and by['layer1.0.conv2']['m'] == 56 * 56
    assert by['layer4.2.mse.conv3_smallscale2']['m'] == 2 * 3 * 3 and by['layer4.2.mse.conv3']['m'] == 2 * 49 and by['layer2.0.mse.conv1']['m'] == 56 * 56
    trunk = sum(r['macs'] for r in flops.layer_table(224, 224, 'resnet50'))
    total = sum(r['macs'] for r in rows)
    extra = total - trunk
    assert 0 < extra < 0.15 * trunk      # the difference path and the long-term modules: a few per cent over the R50 trunk
    small = sum(r['macs'] for r in rows if 'smallscale' in r['name'] or r['name'].endswith('mse.conv2'))
    assert small < 0.01 * total          # the r-channel 3x3 convs: under 1 % (plain FMAs, no MFMA path)
    assert flops.flops_per_clip(8, 224, 224, 12, 'tdn_resnet50') == 2.0 * 8 * (total + 2048 * 12) == flops.tdn_flops_per_clip(8, 224, 224, 12)
    assert len(flops.tdn_table(96, 160, NET['depths'])) < len(rows)


# ---- host arithmetic ------------------------------------------------------------------------------------------------------
def test_host_arithmetic_under_sanitizers(tmp_path):
    """tests/tdn_host.cpp built with ASAN + UBSAN (runtimes linked statically: the program runs as it is) and run once."""
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path / 'tdn_host')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan',
           '-static-libubsan', '-fno-omit-frame-pointer', '-Wall', '-Wextra', '-Werror', os.path.join(ROOT, 'tests', 'tdn_host.cpp'),
           '-o', exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'runtime error' not in run.stdout + run.stderr and 'tdn_host ok' in run.stdout
