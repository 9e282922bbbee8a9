"""Block placement of the temporal shift (``shift_place='block'``) on the CPU: argument checking, state-dict keys, the
checkpoint / mmaction2 / ONNX key mappings, the CPU reference (oracle/tsm_oracle.py) and the new kernel instantiations
in the built code object."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

from oracle import tsm_oracle
from tests._torch_tsm import TorchTSM
from workoutdetector_amd.weights import (SHIFT_PLACES, conv_specs, make_state_dict, remap_checkpoint_keys,
                                         remap_mmaction_keys)

MODELS = ['resnet18', 'resnet34', 'resnet50']


def test_create_model_accepts_block_placement():
    """It used to stop at ``assert shift_place == 'blockres'``; now it gets past argument checking and fails only where
    any engine does without a device (the CPU is refused as a device)."""
    from workoutdetector_amd.engine import create_model
    with pytest.raises(RuntimeError, match='no CPU path'):
        create_model(num_class=12, shift_place='block', device='cpu')


@pytest.mark.parametrize('place', ['foo', 'blocks', ''])
def test_unknown_placement_is_refused(place):
    from workoutdetector_amd.engine import TsmEngine, create_model
    with pytest.raises(ValueError, match='shift_place'):
        create_model(num_class=12, shift_place=place, device='cpu')
    with pytest.raises(ValueError, match='shift_place'):
        TsmEngine(num_class=12, shift_place=place)
    with pytest.raises(ValueError, match='shift_place'):
        conv_specs('resnet50', place)


@pytest.mark.parametrize('base_model', MODELS)
def test_block_keys(base_model):
    """Same convs in the same order; every block key sits under ``layerL.B.net``, conv1 unwrapped; stem and fc unchanged."""
    res, blk = conv_specs(base_model), conv_specs(base_model, 'block')
    assert len(res) == len(blk) == {'resnet18': 20, 'resnet34': 36, 'resnet50': 53}[base_model]
    assert res[0] == blk[0] == ('base_model.conv1.weight', 'base_model.bn1', 64, 3, 7)
    for (wr, br, *shape_r), (wb, bb, *shape_b) in zip(res[1:], blk[1:]):
        assert shape_r == shape_b
        layer, b = wr.split('.')[1:3]
        assert wb.startswith(f'base_model.{layer}.{b}.net.') and bb.startswith(f'base_model.{layer}.{b}.net.')
        assert '.conv1.net.' not in wb and wb == f'base_model.{layer}.{b}.net.' + wr.split('.', 3)[3].replace('conv1.net.', 'conv1.')
        assert bb == f'base_model.{layer}.{b}.net.' + br.split('.', 3)[3]
    sd_r = make_state_dict(5, 12, base_model)
    sd_b = make_state_dict(5, 12, base_model, shift_place='block')
    assert list(sd_b) == list(tsm_oracle.as_block_keys(sd_r))
    assert all(np.array_equal(a, b) for a, b in zip(sd_r.values(), sd_b.values()))     # one RNG stream, two spellings
    assert {k for k in sd_b if not k.startswith('base_model.layer')} == {k for k in sd_r if not k.startswith('base_model.layer')}


@pytest.mark.parametrize('base_model', MODELS)
def test_module_spelling_has_the_block_keys(base_model):
    net = TorchTSM(base_model, shift_place='block')
    keys = [k.replace('new_fc.', 'fc.') for k in net.state_dict() if not k.endswith('num_batches_tracked')]
    assert sorted(keys) == sorted(make_state_dict(0, 12, base_model, shift_place='block'))


def test_checkpoint_remap_keeps_block_keys():
    sd = make_state_dict(1, 12, 'resnet18', shift_place='block')
    ckpt = OrderedDict(('model.' + k, v) for k, v in sd.items())
    assert list(remap_checkpoint_keys(ckpt, 12, 'resnet18')) == list(sd)


def test_mmaction_remap_of_block_keys():
    """mmaction2's ResNetTSM(shift_place='block') puts ``.net`` after the block index."""
    raw = OrderedDict([
        ('backbone.conv1.conv.weight', 0), ('backbone.conv1.bn.weight', 1),
        ('backbone.layer1.0.net.conv1.conv.weight', 2), ('backbone.layer1.0.net.conv1.bn.running_var', 3),
        ('backbone.layer1.0.net.conv3.conv.weight', 4), ('backbone.layer1.0.net.conv3.bn.bias', 5),
        ('backbone.layer1.0.net.downsample.conv.weight', 6), ('backbone.layer1.0.net.downsample.bn.weight', 7),
        ('backbone.layer4.2.net.conv2.conv.weight', 8), ('cls_head.fc_cls.weight', 9), ('cls_head.fc_cls.bias', 10)])
    assert list(remap_mmaction_keys(raw)) == [
        'base_model.conv1.weight', 'base_model.bn1.weight',
        'base_model.layer1.0.net.conv1.weight', 'base_model.layer1.0.net.bn1.running_var',
        'base_model.layer1.0.net.conv3.weight', 'base_model.layer1.0.net.bn3.bias',
        'base_model.layer1.0.net.downsample.0.weight', 'base_model.layer1.0.net.downsample.1.weight',
        'base_model.layer4.2.net.conv2.weight', 'fc.weight', 'fc.bias']
    # the blockres spelling is unchanged
    assert list(remap_mmaction_keys({'backbone.layer1.0.conv1.conv.net.weight': 0})) == ['base_model.layer1.0.conv1.net.weight']


@pytest.mark.parametrize('base_model', MODELS)
def test_reference_matches_the_module_and_differs_from_blockres(base_model):
    """The functional reference agrees with the nn.Module spelling, and block placement is not blockres."""
    sd = make_state_dict(2, 12, base_model, shift_place='block')
    tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
    x = torch.randn(2, 8, 3, 64, 64, generator=torch.Generator().manual_seed(0))
    want = tsm_oracle.forward(tsd, x, base_model, 'block')
    with torch.no_grad():
        got = TorchTSM(base_model, shift_place='block').load_engine_state_dict(sd).eval()(x)
    assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())
    res_sd = {k: torch.from_numpy(v) for k, v in make_state_dict(2, 12, base_model).items()}
    blockres = tsm_oracle.forward(res_sd, x, base_model)
    assert float((blockres - want).abs().max()) > 1e-3 * float(want.abs().max())


@pytest.mark.parametrize('style', ['eval', 'training'])
@pytest.mark.parametrize('base_model', ['resnet50', 'resnet18'])
def test_torch_export_of_block_placement_is_imported(tmp_path, base_model, style):
    """Both export styles of a block-placement module (named initialisers ``...layerL.B.net.conv1.weight`` / anonymous
    eval-mode ones) load with ``shift_place='block'`` and drive the reference to the module's logits."""
    from tests._torch_tsm import LitWrapper, export_onnx
    from workoutdetector_amd.onnx_import import load_onnx_state_dict, parse_onnx
    sd = make_state_dict(4, 12, base_model, shift_place='block')
    path = str(tmp_path / f'block_{style}.onnx')
    export_onnx(LitWrapper(TorchTSM(base_model, shift_place='block').load_engine_state_dict(sd)), path,
                sample_shape=(1, 8, 3, 64, 64), training=(style == 'training'))
    inits, _ = parse_onnx(path)
    assert any(k.startswith('onnx::Conv_') for k in inits) == (style == 'eval')
    got = load_onnx_state_dict(path, 12, base_model, shift_place='block')
    if style == 'training':
        assert set(got) == set(sd) and all(np.array_equal(got[k], sd[k]) for k in sd)
    else:
        assert set(got) == set(sd)
    x = torch.randn(1, 8, 3, 64, 64, generator=torch.Generator().manual_seed(1))
    want = tsm_oracle.forward({k: torch.from_numpy(v) for k, v in sd.items()}, x, base_model, 'block')
    have = tsm_oracle.forward({k: torch.from_numpy(np.asarray(v)) for k, v in got.items()}, x, base_model, 'block')
    assert float((have - want).abs().max()) <= 1e-5 * float(want.abs().max())


# ---- the new kernel instantiations: conv_igemm with PREC | kPrecBlockShift (4), SHIFT = RES = false ----------------------------
IGEMM_TILES = ['128, 128, 2, 2', '128, 128, 4, 2', '128, 64, 2, 2', '64, 64, 2, 2', '32, 32, 1, 1']


def _block_kernels():
    names = []
    for tile in IGEMM_TILES:
        for prec in (0, 1, 2):
            p = prec | 4
            names += [f'conv_igemm<{tile}, 1, false, false, {p}, false, false>',    # Bottleneck conv3 + shifted identity
                      f'conv_igemm<{tile}, 3, false, false, {p}, false, false>',    # BasicBlock conv2 + shifted identity
                      f'conv_igemm<{tile}, 1, false, false, {p}, true, false>']     # conv3 + downsample of a shifted input
    names += [f'conv_igemm<{t}, 1, false, false, 4, true, true>' for t in ('64, 64, 2, 2', '32, 32, 1, 1')]   # fp32 long K
    return names


# Block arms whose occupancy sits below their blockres sibling's (the same tile and precision with an unshifted residual /
# second source), with the workgroups per CU they keep.  The shifted second source holds two more offsets per loader pass:
# fp32 64x64 DUAL needs 88 / 103 registers (segmented) against 80 / 96, one workgroup per CU less; asked for 5 waves per
# SIMD, the segmented form spilled 20 bytes, so it is built for 4 and stays scratch-free.
OCCUPANCY_EXCEPTIONS = {'conv_igemm<64, 64, 2, 2, 1, false, false, 4, true, false>': 5,
                        'conv_igemm<64, 64, 2, 2, 1, false, false, 4, true, true>': 4}


def _sibling(name):
    a = [x.strip() for x in name[len('conv_igemm<'):-1].split(',')]
    a[7] = str(int(a[7]) & 3)
    if a[8] == 'false':
        a[6] = 'true'
    return 'conv_igemm<' + ', '.join(a) + '>'


def test_block_placement_kernels_are_built_scratch_free():
    """Every new arm is scratch-free and keeps its blockres sibling's workgroups per CU, but for the listed exceptions."""
    from workoutdetector_amd import codeobj
    from workoutdetector_amd.build import build_library
    md = codeobj.kernel_metadata(build_library())
    names = _block_kernels()
    assert len(names) == 47
    for name in names:
        assert name in md, name
        r, sib = md[name], md[_sibling(name)]
        assert r['.private_segment_fixed_size'] == 0 and r['.vgpr_spill_count'] == 0, name
        assert r['.group_segment_fixed_size'] == sib['.group_segment_fixed_size'], name
        want = OCCUPANCY_EXCEPTIONS.get(name, sib['workgroups_per_cu'])
        assert r['workgroups_per_cu'] >= want, (name, r['workgroups_per_cu'], sib['workgroups_per_cu'])
    for name, wg in OCCUPANCY_EXCEPTIONS.items():
        assert md[name]['workgroups_per_cu'] == wg and md[_sibling(name)]['workgroups_per_cu'] == wg + 1, name
    assert set(SHIFT_PLACES) == {'blockres', 'block'}


def test_persistent_256_block_arms_fit_one_eight_wave_workgroup():
    """conv_bf16_256p_kernel<1, true, RES, DUAL>: block placement's shifted identity / second source on the persistent tile,
    in the budget of its family (tests/test_code_objects.py): <= 256 registers, no scratch, one workgroup per CU."""
    from workoutdetector_amd import codeobj
    from workoutdetector_amd.build import build_library
    md = codeobj.kernel_metadata(build_library())
    for args in ('1, true, true, false', '1, true, false, true'):
        r = md[f'conv_bf16_256p_kernel<{args}>']
        assert r['.max_flat_workgroup_size'] == 512 and r['.vgpr_count'] <= 256 and r['.group_segment_fixed_size'] == 0
        assert r['.private_segment_fixed_size'] == 0 and r['.vgpr_spill_count'] == 0
        assert codeobj.workgroups_per_cu(r, 131072 + 8192 + 8 * 2176) == 1
