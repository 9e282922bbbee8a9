"""TSM-ResNet18 / 34 on the CPU side: state-dict keys and shapes, the R50 weights stream, FLOP accounting, checkpoint and
ONNX import, and the new conv_igemm instantiations in the built code object (shifted 3x3, 3x3 + residual)."""
import numpy as np
import pytest
import torch

from oracle import tsm_oracle
from tests._torch_tsm import TorchTSM
from workoutdetector_amd import flops, weights

BASIC = ['resnet18', 'resnet34']


@pytest.mark.parametrize('base_model', BASIC)
def test_basic_keys_and_shapes_match_a_torch_module(base_model):
    """conv_specs / make_state_dict / required_keys spell the module tree of TSM-R18/34 (conv1 wrapped as `.net`)."""
    want = TorchTSM(base_model).engine_state_dict()
    sd = weights.make_state_dict(3, 12, base_model=base_model)
    assert list(sd) == list(want)                                   # same keys, torchvision's module order
    for k, v in want.items():
        assert tuple(sd[k].shape) == tuple(v.shape), k
        assert sd[k].dtype == np.float32
    assert set(weights.required_keys(base_model=base_model)) == set(want)
    specs = weights.conv_specs(base_model)
    assert len(specs) == {'resnet18': 20, 'resnet34': 36}[base_model]
    assert all(tuple(want[w].shape) == (co, ci, k, k) for w, _bn, co, ci, k in specs)
    assert weights.feature_width(base_model) == 512 and sd['fc.weight'].shape == (12, 512)
    # bn2 closes the residual branch of a BasicBlock: it is the damped one
    assert sd['base_model.layer1.0.bn2.weight'].max() < 0.5 < sd['base_model.layer1.0.bn1.weight'].min()
    # and the engine-facing model loads it strictly
    TorchTSM(base_model).load_engine_state_dict(sd)


def test_r50_weights_stream_is_unchanged():
    a = weights.make_state_dict(0, 12)
    b = weights.make_state_dict(0, 12, base_model='resnet50')
    assert list(a) == list(b) and len(a) == 53 * 5 + 2
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert weights.conv_specs() == weights.conv_specs('resnet50') and weights.feature_width() == 2048


def test_unknown_backbone_is_refused():
    for fn in (weights.conv_specs, lambda m: weights.make_state_dict(0, 12, base_model=m)):
        with pytest.raises(NotImplementedError):
            fn('resnet101')
    from workoutdetector_amd.engine import create_model
    with pytest.raises(NotImplementedError):
        create_model(base_model='resnet101')


def _hand_macs(blocks, h=224, w=224):
    """BasicBlock MACs per frame, summed by hand: stem, then per block conv1 (3x3 at the stride), conv2, downsample."""
    def out(s, k, st):
        return (s + 2 * (k // 2) - k) // st + 1
    h, w = out(h, 7, 2), out(w, 7, 2)
    total = h * w * 64 * 3 * 49
    h, w = out(h, 3, 2), out(w, 3, 2)
    cin = 64
    for li, (nb, planes) in enumerate(zip(blocks, (64, 128, 256, 512))):
        for b in range(nb):
            st = 2 if (b == 0 and li > 0) else 1
            h, w = out(h, 3, st), out(w, 3, st)
            total += h * w * planes * cin * 9 + h * w * planes * planes * 9
            if st != 1 or cin != planes:
                total += h * w * planes * cin
            cin = planes
    return total


@pytest.mark.parametrize('base_model,blocks', [('resnet18', (2, 2, 2, 2)), ('resnet34', (3, 4, 6, 3))])
def test_basic_flops_match_a_hand_sum(base_model, blocks):
    conv = _hand_macs(blocks)
    assert sum(r['macs'] for r in flops.layer_table(base_model=base_model)) == conv
    assert flops.macs_per_frame(num_class=12, base_model=base_model) == conv + 512 * 12
    assert flops.flops_per_clip(8, num_class=12, base_model=base_model) == 2.0 * 8 * (conv + 512 * 12)
    assert sum(r['macs'] for r in flops.layer_table(160, 129, base_model=base_model)) == _hand_macs(blocks, 160, 129)
    # about 1.8 and 3.7 GMAC per frame
    assert abs(conv / 1e9 - {'resnet18': 1.81, 'resnet34': 3.66}[base_model]) < 0.01


def test_r50_flops_unchanged():
    assert flops.macs_per_frame() == 4087160832 == flops.macs_per_frame(base_model='resnet50')
    assert flops.layer_table(160, 129) == flops.layer_table(160, 129, base_model='resnet50')
    assert len(flops.layer_table()) == 53


def test_basic_checkpoint_remap():
    """A Lightning checkpoint of TSM-R18 (``model.`` prefix, ``new_fc`` last) maps onto the engine keys."""
    net = TorchTSM('resnet18')
    raw = {'model.' + k: v for k, v in net.state_dict().items()}
    got = weights.remap_checkpoint_keys(raw, 12, base_model='resnet18')
    want = net.engine_state_dict()
    assert set(k for k in got if not k.endswith('num_batches_tracked')) == set(want)
    for k, v in want.items():
        assert torch.equal(got[k], v), k


@pytest.mark.parametrize('style', ['training', 'eval'])
def test_basic_onnx_export_is_imported(tmp_path, style):
    """``torch.onnx.export`` of the R18 module: recognised as R18 from the graph; the names-kept export gives the state
    dict back exactly, the Conv+BN-fused one drives the CPU reference to the same logits."""
    from tests._torch_tsm import LitWrapper, export_onnx
    from workoutdetector_amd.onnx_import import load_onnx_state_dict, parse_onnx
    sd = weights.make_state_dict(5, 12, base_model='resnet18')
    net = TorchTSM('resnet18').load_engine_state_dict(sd)
    path = str(tmp_path / f'r18_{style}.onnx')
    export_onnx(LitWrapper(net), path, sample_shape=(1, 8, 3, 64, 64), training=(style == 'training'))
    inits, nodes = parse_onnx(path)
    assert sum(n['op_type'] == 'Conv' for n in nodes) == 20
    got = load_onnx_state_dict(path, 12)                      # recognised from the graph
    got2 = load_onnx_state_dict(path, 12, base_model='resnet18')
    assert list(got) == list(got2)
    with pytest.raises(ValueError, match='resnet18'):
        load_onnx_state_dict(path, 12, base_model='resnet50')
    if style == 'training':
        assert set(got) == set(sd) and all(np.array_equal(got[k], sd[k]) for k in sd)
    x = torch.randn(1, 8, 3, 64, 64, generator=torch.Generator().manual_seed(2))
    want = tsm_oracle.forward({k: torch.from_numpy(v) for k, v in sd.items()}, x, 'resnet18')
    have = tsm_oracle.forward({k: torch.from_numpy(np.asarray(v)) for k, v in got.items()}, x, 'resnet18')
    assert float((have - want).abs().max()) <= 1e-5 * float(want.abs().max())
    with torch.no_grad():
        assert float((net.eval()(x) - want).abs().max()) <= 1e-4 * float(want.abs().max())


def test_shifted_3x3_and_residual_3x3_kernels_are_built_scratch_free():
    from workoutdetector_amd import codeobj
    from workoutdetector_amd.build import build_library
    md = codeobj.kernel_metadata(build_library())

    def args(name):
        return [a.strip() for a in name[len('conv_igemm<'):-1].split(',')]
    igemm = {n: r for n, r in md.items() if n.startswith('conv_igemm<')}
    shifted3 = [n for n in igemm if args(n)[4] == '3' and args(n)[5] == 'true']
    res3 = [n for n in igemm if args(n)[4] == '3' and args(n)[6] == 'true']
    # five tile shapes x three precisions each; never a segmented shifted 3x3
    assert len(shifted3) == 15 and len(res3) == 15, (shifted3, res3)
    assert not any(args(n)[9] == 'true' for n in shifted3)
    for n in shifted3 + res3:
        assert igemm[n]['.private_segment_fixed_size'] == 0 and igemm[n]['.vgpr_spill_count'] == 0, n
    for prec in ('0', '1', '2'):
        assert f'conv_igemm<64, 64, 2, 2, 3, true, false, {prec}, false, false>' in igemm
        assert f'conv_igemm<128, 128, 2, 2, 3, false, true, {prec}, false, false>' in igemm
