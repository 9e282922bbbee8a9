"""TSM-Wide-ResNet-50-2 on the CPU side: state-dict keys and shapes under both placements, the seeded weight streams,
FLOP accounting, create_model's argument checks, checkpoint and ONNX import (WRN told apart from R50 by layer1.0.conv1's
width), the C ABI declaration and the new fused conv2 + conv3 kernel in the built code object."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from oracle import tsm_oracle
from tests._torch_tsm import TorchTSM
from workoutdetector_amd import flops, weights

WRN = 'wide_resnet50_2'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('place', ['blockres', 'block'])
def test_wide_conv_specs_shapes_and_keys(place):
    specs = weights.conv_specs(WRN, place)
    r50 = weights.conv_specs('resnet50', place)
    assert len(specs) == 53
    assert [s[:2] for s in specs] == [s[:2] for s in r50]        # the same keys and BN prefixes as R50, in the same order
    cin = 64
    i = 1
    for li, (nb, p) in enumerate(zip((3, 4, 6, 3), (64, 128, 256, 512)), start=1):
        for b in range(nb):
            want = [(2 * p, cin, 1), (2 * p, 2 * p, 3), (4 * p, 2 * p, 1)] + ([(4 * p, cin, 1)] if b == 0 else [])
            got = [s[2:] for s in specs[i:i + len(want)]]
            assert got == want, (li, b, got)
            i += len(want)
            cin = 4 * p
    assert i == 53
    assert specs[0] == r50[0]
    assert weights.feature_width(WRN) == 2048 and weights.bottleneck_width(WRN) == 128
    assert weights.bottleneck_width('resnet50') == 64


@pytest.mark.parametrize('place', ['blockres', 'block'])
def test_wide_state_dict_matches_a_torch_module(place):
    sd = weights.make_state_dict(3, 12, base_model=WRN, shift_place=place)
    assert len(sd) == 53 * 5 + 2
    assert set(weights.required_keys(base_model=WRN, shift_place=place)) == set(sd)
    for w, bn, co, ci, k in weights.conv_specs(WRN, place):
        assert sd[w].shape == (co, ci, k, k) and sd[w].dtype == np.float32
        for s in ('.weight', '.bias', '.running_mean', '.running_var'):
            assert sd[bn + s].shape == (co,)
    assert sd['fc.weight'].shape == (12, 2048)
    if place == 'blockres':
        TorchTSM(WRN, 128).load_engine_state_dict(sd)                 # the module tree spells the same keys
        assert set(TorchTSM(WRN, 128).engine_state_dict()) == set(sd)


def test_wide_weights_stream_is_deterministic_and_r50_is_unchanged():
    a = weights.make_state_dict(0, 12, base_model=WRN)
    b = weights.make_state_dict(0, 12, base_model=WRN)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    c = weights.make_state_dict(1, 12, base_model=WRN)
    assert not np.array_equal(a['fc.weight'], c['fc.weight'])
    # the placements spell the same numbers
    blk = weights.make_state_dict(0, 12, base_model=WRN, shift_place='block')
    assert all(np.array_equal(x, y) for x, y in zip(a.values(), blk.values()))
    # R50's stream: the keys and the arrays of the default call, one seeded draw after another as before
    r50 = weights.make_state_dict(0, 12)
    rng = np.random.default_rng(0)
    for wkey, bnp, cout, cin, k in weights.conv_specs('resnet50'):
        want = (rng.standard_normal((cout, cin, k, k)) * np.sqrt(2.0 / (cin * k * k))).astype(np.float32)
        assert np.array_equal(r50[wkey], want), wkey
        rng.uniform(0.8, 1.2, cout), rng.standard_normal(cout), rng.standard_normal(cout), rng.uniform(0.6, 1.4, cout)
    assert np.array_equal(r50['fc.weight'], (rng.standard_normal((12, 2048)) * 0.05).astype(np.float32))


def test_wide_flops():
    rows = flops.layer_table(base_model=WRN)
    assert len(rows) == 53
    assert [r['name'] for r in rows] == [r['name'] for r in flops.layer_table()]
    assert rows[1] == dict(name='layer1.0.conv1', cin=64, cout=128, k=1, s=1, m=56 * 56, macs=56 * 56 * 128 * 64)
    l21 = next(r for r in rows if r['name'] == 'layer2.0.conv2')
    assert (l21['cin'], l21['cout'], l21['s'], l21['m']) == (256, 256, 2, 28 * 28)
    macs = flops.macs_per_frame(base_model=WRN, num_class=12)
    assert macs == sum(r['macs'] for r in rows) + 2048 * 12
    assert abs(sum(r['macs'] for r in rows) / 1e9 - 11.4) < 0.01            # torchvision: 11.4 GMAC per 224^2 frame
    assert flops.macs_per_frame() == 4087160832                              # R50 unchanged


def test_create_model_accepts_wrn_and_refuses_the_deep_backbones():
    from workoutdetector_amd.engine import create_model
    with pytest.raises(RuntimeError, match='no CPU path'):
        create_model(base_model=WRN, device='cpu')
    with pytest.raises(RuntimeError, match='no CPU path'):
        create_model(base_model=WRN, device='cpu', shift_place='block')
    for deep in ('wide_resnet101_2', 'resnet101', 'resnet152'):
        with pytest.raises(NotImplementedError):
            create_model(base_model=deep, device='cpu')
        with pytest.raises(NotImplementedError):
            weights.conv_specs(deep)


def test_wide_checkpoint_remap_keeps_the_r50_keys():
    net = TorchTSM(WRN, 128)
    raw = {'model.' + k: v for k, v in net.state_dict().items()}
    got = weights.remap_checkpoint_keys(raw, 12, base_model=WRN)
    want = net.engine_state_dict()
    assert set(k for k in got if not k.endswith('num_batches_tracked')) == set(want)
    for k, v in want.items():
        assert torch.equal(got[k], v), k


@pytest.mark.parametrize('style', ['training', 'eval'])
def test_wide_and_r50_onnx_exports_are_told_apart(tmp_path, style):
    """53 Conv nodes each: a WRN export imports as WRN, an R50 export of the same module class still as R50."""
    from tests._torch_tsm import LitWrapper, export_onnx
    from workoutdetector_amd.onnx_import import detect_backbone, load_onnx_state_dict, parse_onnx
    x = torch.randn(1, 8, 3, 64, 64, generator=torch.Generator().manual_seed(2))
    for base_model, width in ((WRN, 128), ('resnet50', 64)):
        sd = weights.make_state_dict(5, 12, base_model=base_model)
        net = TorchTSM(base_model, width).load_engine_state_dict(sd)
        path = str(tmp_path / f'{base_model}_{style}.onnx')
        export_onnx(LitWrapper(net), path, sample_shape=(1, 8, 3, 64, 64), training=(style == 'training'))
        inits, nodes = parse_onnx(path)
        assert sum(n['op_type'] == 'Conv' for n in nodes) == 53
        assert detect_backbone(inits, nodes) == base_model
        got = load_onnx_state_dict(path, 12)
        assert list(got) == list(load_onnx_state_dict(path, 12, base_model=base_model))
        other = 'resnet50' if base_model == WRN else WRN
        with pytest.raises(ValueError, match=base_model):
            load_onnx_state_dict(path, 12, base_model=other)
        if style == 'training':
            assert set(got) == set(sd) and all(np.array_equal(got[k], sd[k]) for k in sd)
        want = tsm_oracle.forward({k: torch.from_numpy(v) for k, v in sd.items()}, x, base_model)
        have = tsm_oracle.forward({k: torch.from_numpy(np.asarray(v)) for k, v in got.items()}, x, base_model)
        assert float((have - want).abs().max()) <= 1e-5 * float(want.abs().max())
        with torch.no_grad():
            assert float((net.eval()(x) - want).abs().max()) <= 1e-4 * float(want.abs().max())


def test_header_declares_and_library_exports_set_bottleneck_width():
    from workoutdetector_amd import _lib
    from workoutdetector_amd.build import LIB_PATH, build_library
    build_library()
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'tsm_hip.h')).read(), flags=re.S)
    assert re.search(r'int tsm_set_bottleneck_width\(tsm_engine \*e, int32_t width_per_group\);', text)
    assert re.search(r'#define TSM_ABI_VERSION 7\b', open(os.path.join(ROOT, 'include', 'tsm_hip.h')).read())
    assert 'tsm_set_bottleneck_width' in _lib.EXPORTS
    out = subprocess.run(['nm', '-D', '--defined-only', LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r' T tsm_set_bottleneck_width$', out, flags=re.M)


def test_two_chunk_fused_conv23_kernel_is_built_scratch_free():
    """conv23_fused2_kernel<128, X3>: 512 threads, the 70.6 KB LDS of its four-chunk sibling, <= 128 registers -> two
    workgroups = 16 waves per CU; no scratch.  The four-chunk kernels keep their names and figures."""
    from workoutdetector_amd import codeobj
    from workoutdetector_amd.build import build_library
    md = codeobj.kernel_metadata(build_library())
    for x3, vgprs in (('false', 98), ('true', 116)):
        r = md[f'conv23_fused2_kernel<128, {x3}>']
        assert r['.private_segment_fixed_size'] == 0 and r['.vgpr_spill_count'] == 0, x3
        assert r['.group_segment_fixed_size'] == 70656 and r['.max_flat_workgroup_size'] == 512, x3
        assert r['.vgpr_count'] <= vgprs and r['workgroups_per_cu'] == 2, (x3, r['.vgpr_count'], r['workgroups_per_cu'])
        assert r['workgroups_per_cu'] * 8 == 16
    assert not [n for n in md if n.startswith('conv23_fused2_kernel<') and not n.startswith('conv23_fused2_kernel<128,')]
    for cmid, lds in ((64, 35840), (128, 70656)):
        for x3 in ('false', 'true'):
            r = md[f'conv23_fused_kernel<{cmid}, {x3}>']
            assert r['.group_segment_fixed_size'] == lds and r['.private_segment_fixed_size'] == 0
