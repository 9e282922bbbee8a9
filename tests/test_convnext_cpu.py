"""base_model='convnext_base' without a GPU: the specs and the seeded weights (their own generator: no existing number moves),
the timm key remap, the FLOP table against a hand count, every refusal that never reaches the library, the new export in the
header, the library and the binding, the new kernels' figures in the built code object, the float64 model's residual stream, and
the pure-host arithmetic under ASAN + UBSAN (tests/convnext_host.cpp, a stand-alone program)."""
import ctypes
import hashlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import _convnext as cn
from workoutdetector_amd import engine, flops, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHALLOW = (1, 1, 2, 1)
FULL = (3, 3, 27, 3)


# ---- specs and seeded weights ---------------------------------------------------------------------------------------------
def test_specs_are_timm_convnext_base():
    specs = weights.convnext_specs()
    keys = [k for k, _s, _k in specs]
    assert len(keys) == len(set(keys)) == 4 + 3 * 4 + 36 * 9 + 2
    shapes = {k: s for k, s, _ in specs}
    assert shapes['stem.0.weight'] == (128, 3, 4, 4) and shapes['stem.0.bias'] == (128,) and shapes['stem.1.weight'] == (128,)
    assert 'stages.0.downsample.0.weight' not in shapes
    for s, c in ((1, 256), (2, 512), (3, 1024)):
        assert shapes[f'stages.{s}.downsample.0.weight'] == (c // 2,) and shapes[f'stages.{s}.downsample.1.weight'] == (c, c // 2, 2, 2)
        assert shapes[f'stages.{s}.downsample.1.bias'] == (c,)
    for s, (nb, c) in enumerate(zip(FULL, (128, 256, 512, 1024))):
        assert f'stages.{s}.blocks.{nb}.gamma' not in shapes
        p = f'stages.{s}.blocks.{nb - 1}'
        assert shapes[p + '.conv_dw.weight'] == (c, 1, 7, 7) and shapes[p + '.norm.bias'] == (c,) and shapes[p + '.gamma'] == (c,)
        assert shapes[p + '.mlp.fc1.weight'] == (4 * c, c) and shapes[p + '.mlp.fc2.weight'] == (c, 4 * c) and shapes[p + '.mlp.fc2.bias'] == (c,)
    assert shapes['head.norm.weight'] == (1024,) and keys[-1] == 'head.norm.bias'
    assert len(weights.convnext_specs(SHALLOW)) == 4 + 12 + 5 * 9 + 2
    assert weights.feature_width('convnext_base') == 1024 and weights.feature_width('resnet18') == 512
    for bad in ((3, 3, 27), (3, 0, 27, 3), (3, 3, 65, 3)):
        with pytest.raises(ValueError):
            weights.convnext_specs(bad)


def test_seeded_weights_make_every_part_matter():
    sd = weights.make_state_dict(0, 7, 'convnext_base', depths=SHALLOW)
    assert list(sd)[:-2] == [k for k, _s, _k in weights.convnext_specs(SHALLOW)] and list(sd)[-2:] == ['head.fc.weight', 'head.fc.bias']
    assert sd['head.fc.weight'].shape == (7, 1024) and all(v.dtype == np.float32 for v in sd.values())
    for (k, shape, kind) in weights.convnext_specs(SHALLOW):
        v = sd[k]
        assert v.shape == shape
        if kind == 'gamma':
            assert 0.1 <= v.min() and v.max() <= 0.3 and v.std() > 0.03, k          # not timm's 1e-6: a block must not be the identity
        elif kind == 'ln_w':
            assert 0.8 <= v.min() and v.max() <= 1.2 and v.std() > 0.05, k
        else:
            assert np.abs(v).max() > 0 and abs(float(v.mean())) < 0.1, k              # (biases, LayerNorm's included: non-zero)
    again = weights.make_state_dict(0, 7, 'convnext_base', depths=SHALLOW)
    other = weights.make_state_dict(1, 7, 'convnext_base', depths=SHALLOW)
    assert all(np.array_equal(sd[k], again[k]) for k in sd) and not np.array_equal(sd['stem.0.weight'], other['stem.0.weight'])
    with pytest.raises(ValueError):
        weights.make_state_dict(0, 7, 'resnet18', depths=SHALLOW)


def _digest(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(str(v.shape).encode())
        h.update(v.tobytes())
    return h.hexdigest()[:16]


@pytest.mark.parametrize('base_model, kw, want', [
    ('resnet18', {}, 'dc6b4352dc8feedd'), ('resnet34', {}, 'bb5ee5f358cc5171'), ('resnet50', {}, '16dcdfce240ae51f'),
    ('wide_resnet50_2', {}, '0cf940ad1a0f85ce'), ('resnet50', dict(shift_place='block'), '165690e486cd8e60'),
    ('resnet50', dict(non_local=True), '8e25d5f9c8a43656')])
def test_every_earlier_backbone_keeps_its_numbers(base_model, kw, want):
    """sha256 over keys, shapes and bytes of make_state_dict(3, 7, ...), recorded on the commit before the ConvNeXt weights."""
    assert _digest(weights.make_state_dict(3, 7, base_model, **kw)) == want


def test_timm_remap_with_and_without_the_lightning_prefix():
    sd = weights.make_state_dict(0, 3, 'convnext_base', depths=SHALLOW)
    plain = weights.remap_timm_keys(sd)
    assert list(plain) == list(sd) and all(plain[k] is sd[k] for k in sd)
    lit = weights.remap_timm_keys({'classifier.' + k: v for k, v in sd.items()})
    assert list(lit) == list(sd) and all(lit[k] is sd[k] for k in sd)
    for bad in ({}, {'classifier.stem.0.weight': 1, 'other.stem.0.bias': 2}, {'conv1.weight': 1}, {'stem.0.weight': 1, 'layer1.0.conv1.weight': 2}):
        with pytest.raises(ValueError):
            weights.remap_timm_keys(bad)


# ---- FLOPs ----------------------------------------------------------------------------------------------------------------
def test_flop_table_sums_to_the_hand_count():
    rows = flops.convnext_table(224, 224)
    assert len(rows) == 1 + 3 + 3 * 36 and rows == flops.layer_table(224, 224, 'convnext_base')
    for r in rows:
        assert r['macs'] == r['m'] * r['cout'] * r['cin'] * r['k'] ** 2, r
    by = {r['name']: r for r in rows}
    assert by['stem']['m'] == 56 * 56 and by['stages.3.blocks.2.fc2']['m'] == 49 and by['stages.2.downsample']['m'] == 196
    hand = 56 * 56 * 128 * 48                                                   # stem
    for px, c, nb in ((56 * 56, 128, 3), (28 * 28, 256, 3), (14 * 14, 512, 27), (7 * 7, 1024, 3)):
        hand += nb * px * (c * 49 + 8 * c * c)                                  # depthwise + fc1 + fc2
        if c > 128:
            hand += px * c * (c // 2) * 4                                       # downsample
    assert sum(r['macs'] for r in rows) == hand
    total = flops.macs_per_frame(224, 224, 1000, 'convnext_base')
    assert total == hand + 1024 * 1000 and 15.3e9 < total < 15.45e9            # 15.4 GMAC
    gemm = sum(r['macs'] for r in rows if not r['name'].endswith('conv_dw'))
    assert gemm / total > 0.98                                                  # the matrix work runs on conv_igemm
    assert flops.flops_per_clip(1, 224, 224, 1000, 'convnext_base') == 2.0 * total
    assert [r['m'] for r in flops.convnext_table(80, 80, SHALLOW) if r['name'].endswith('fc1')] == [400, 100, 25, 25, 4]   # floors


# ---- refusals, all before the library loads -------------------------------------------------------------------------------
def test_refusals_come_before_the_library(monkeypatch):
    from workoutdetector_amd import _lib

    def no_library():
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(_lib, 'load', no_library)
    with pytest.raises(NotImplementedError, match='no temporal shift'):
        engine.create_model(base_model='convnext_base')
    for dtype in ('bf16x3', 'bf16'):
        with pytest.raises(NotImplementedError, match="dtype='f32' only"):
            engine.create_image_model(base_model='convnext_base', dtype=dtype)
        with pytest.raises(NotImplementedError, match="dtype='f32' only"):
            engine.create_feature_model(base_model='convnext_base', dtype=dtype)
        with pytest.raises(NotImplementedError):
            engine.TsmEngine(base_model='convnext_base', num_segments=1, is_shift=False, dtype=dtype)
    for make in (engine.create_image_model, engine.create_feature_model):
        with pytest.raises(NotImplementedError, match='onnx'):
            make(base_model='convnext_base', checkpoint='exported.onnx')
        for other in ('convnext_tiny', 'convnext_small', 'convnext_large', 'convnext_xlarge'):
            with pytest.raises(NotImplementedError, match='not powers of two'):
                make(base_model=other)
    with pytest.raises(NotImplementedError, match='not powers of two'):
        engine.create_model(base_model='convnext_tiny')
    with pytest.raises(NotImplementedError, match='no temporal shift'):
        engine.TsmEngine(base_model='convnext_base', num_segments=8, is_shift=False)
    with pytest.raises(NotImplementedError, match='no temporal shift'):
        engine.TsmEngine(base_model='convnext_base', num_segments=1, is_shift=True)
    with pytest.raises(NotImplementedError):
        engine.TsmEngine(base_model='convnext_base', num_segments=1, is_shift=False, non_local=True)
    with pytest.raises(ValueError):
        engine.TsmEngine(base_model='convnext_base', num_segments=1, is_shift=False, convnext_depths=(1, 2, 3))
    with pytest.raises(ValueError, match='convnext_depths'):
        engine.TsmEngine(base_model='resnet18', convnext_depths=SHALLOW)
    with pytest.raises(NotImplementedError, match='the engine implements'):      # (an unknown backbone keeps its message)
        engine.create_image_model(base_model='resnet101')


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def test_the_setter_is_declared_exported_and_bound():
    from workoutdetector_amd import _lib
    from workoutdetector_amd.build import LIB_PATH, build_library
    build_library()
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'tsm_hip.h')).read(), flags=re.S)
    assert re.search(r'int\s+tsm_set_convnext\(tsm_engine \*e, const int32_t depths\[4\]\);', text)
    protos = re.findall(r'[^;{}]*\btsm_[a-z0-9_]+\s*\([^;]*\);', text)
    assert not [p for p in protos if 'tsm_set_convnext' in p and 'stream' in p]
    assert 'tsm_set_convnext' in _lib.EXPORTS
    out = subprocess.run(['nm', '-D', '--defined-only', LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r' T tsm_set_convnext$', out, flags=re.M)
    lib = _lib.load()
    assert lib.tsm_set_convnext.restype is ctypes.c_int and len(lib.tsm_set_convnext.argtypes) == 2
    assert lib.tsm_abi_version() == 7
    assert lib.tsm_set_convnext(None, (ctypes.c_int32 * 4)(3, 3, 27, 3)) == -1          # no engine: refused, nothing touched


# ---- code object ----------------------------------------------------------------------------------------------------------
def test_new_kernels_budgets():
    """dwconv7_ln_kernel<C>: no scratch, no spill, 1 KB of LDS at most (the LayerNorm's cross-wave sums), and registers for the
    occupancy the design keeps resident: two workgroups per CU (two waves per SIMD) with 4 x 4 tiles (C = 128 / 256 / 512: 64
    accumulators + a 10-quad input row + the taps in flight), four (four waves per SIMD) with 2 x 2 tiles (C = 1024)."""
    from workoutdetector_amd import codeobj
    from workoutdetector_amd.build import build_library
    md = codeobj.kernel_metadata(build_library())
    for c in (128, 256, 512, 1024):
        r = md[f'dwconv7_ln_kernel<{c}>']
        assert r['.max_flat_workgroup_size'] == 256 and r['.private_segment_fixed_size'] == 0 and r['.vgpr_spill_count'] == 0, r
        assert r['.group_segment_fixed_size'] <= 1024 <= codeobj.LDS_PER_CU and r['.agpr_count'] == 0
        groups, least = (2, 64 + 40) if c <= 512 else (4, 16 + 32)
        assert least <= r['.vgpr_count'] <= codeobj.SIMD_VGPRS // groups and r['waves_per_simd'] >= groups and r['workgroups_per_cu'] >= groups, (c, r['.vgpr_count'])
        for s2d in ('false', 'true'):
            q = md[f'ln_kernel<{c}, {s2d}>']
            assert q['.private_segment_fixed_size'] == 0 and q['.group_segment_fixed_size'] <= 64 and q['.vgpr_count'] <= 64, q
    for name in ('stem_pack4_kernel', 'gelu_kernel'):
        assert md[name]['.private_segment_fixed_size'] == 0 and md[name]['.group_segment_fixed_size'] == 0 and md[name]['.vgpr_count'] <= 64


# ---- the float64 model ----------------------------------------------------------------------------------------------------
def test_residual_stream_stays_in_range_over_all_36_blocks():
    """The seeded full-depth model on one 64 x 64 frame, in float64: finite, the root mean square of every block's output in
    0.5 .. 100, every block changes its input by a visible amount, and the logits tell two inputs apart."""
    sd = weights.make_state_dict(0, 4, 'convnext_base')
    x = np.random.default_rng(1).standard_normal((2, 3, 64, 64))
    out = cn.forward(sd, x, FULL, keep=('stages.2.blocks.12', 'stages.2.blocks.13'))
    assert len(out['rms']) == 36 and all(np.isfinite(out['rms'])) and 0.5 < min(out['rms']) and max(out['rms']) < 100.0, out['rms']
    step = out['stages.2.blocks.13'] - out['stages.2.blocks.12']
    assert 0.03 < np.sqrt((step ** 2).mean()) / out['rms'][6 + 12] < 1.0
    assert out['logits'].shape == (2, 4) and np.abs(out['logits'][0] - out['logits'][1]).max() > 0.1
    # the operators against torch's own, where it has one
    import torch
    import torch.nn.functional as F
    t = torch.from_numpy(x[:, :, :9, :10]).double()
    w = torch.randn(3, 1, 7, 7, dtype=torch.float64)
    b = torch.randn(3, dtype=torch.float64)
    want = F.conv2d(t, w, b, padding=3, groups=3).permute(0, 2, 3, 1).numpy()
    assert np.allclose(cn.dwconv7(t.permute(0, 2, 3, 1).numpy(), w.numpy(), b.numpy()), want, rtol=1e-12, atol=1e-12)
    w2 = torch.randn(5, 3, 2, 2, dtype=torch.float64)
    want = F.conv2d(t, w2, None, stride=2).permute(0, 2, 3, 1).numpy()
    assert np.allclose(cn.patch_conv(t.permute(0, 2, 3, 1).numpy(), w2.numpy(), np.zeros(5), 2), want, rtol=1e-12, atol=1e-12)
    v = torch.randn(4, 6, dtype=torch.float64)
    assert np.allclose(cn.gelu(v.numpy()), F.gelu(v).numpy(), rtol=1e-12, atol=1e-14)
    assert np.allclose(cn.layer_norm(v.numpy(), np.ones(6), np.zeros(6)), F.layer_norm(v, (6,), eps=1e-6).numpy(), rtol=1e-12, atol=1e-12)


# ---- host arithmetic ------------------------------------------------------------------------------------------------------
def test_host_arithmetic_under_sanitizers(tmp_path):
    """tests/convnext_host.cpp built with ASAN + UBSAN (runtimes linked statically: the program runs as it is) and run once."""
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path / 'convnext_host')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan',
           '-static-libubsan', '-fno-omit-frame-pointer', '-Wall', '-Wextra', '-Werror', os.path.join(ROOT, 'tests', 'convnext_host.cpp'),
           '-o', exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'runtime error' not in run.stdout + run.stderr and 'convnext_host ok' in run.stdout
