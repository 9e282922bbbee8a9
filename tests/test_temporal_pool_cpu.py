"""create_model(temporal_pool=True) without a GPU: the wrapped module's state-dict keys through the checkpoint remap, the refusals
that never reach the GPU, the FLOP count from the shapes, the pool kernel's budgets in the built code object, and the pure-host
arithmetic under ASAN + UBSAN (tests/temporal_pool_host.cpp, a stand-alone program)."""
import os
import shutil
import subprocess

import pytest

from tests._temporal_pool import torch_tsm_tp, wrapper_keys
from workoutdetector_amd import engine, flops, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _checkpoint(net):
    """The module's raw state dict as a checkpoint spells it: one leading component, the classifier last."""
    return {'module.' + k: v for k, v in net.state_dict().items()}


@pytest.mark.parametrize('place', ['blockres', 'block'])
@pytest.mark.parametrize('base_model', ['resnet50', 'resnet18'])
def test_wrapped_keys_remap_to_engine_keys(base_model, place):
    net = torch_tsm_tp(base_model, place)
    raw = _checkpoint(net)
    assert list(raw)[-2:] == ['module.new_fc.weight', 'module.new_fc.bias']
    wrapped = 'module.base_model.layer2.net.0.' + ('net.conv1.weight' if place == 'block' else 'conv1.net.weight')
    assert wrapped in raw and not any(k.startswith('module.base_model.layer2.0.') for k in raw)
    back = weights.remap_checkpoint_keys(raw, 12, base_model, temporal_pool=True)
    have = {k for k in back if not k.endswith('num_batches_tracked')}
    assert have == set(weights.required_keys(base_model=base_model, shift_place=place))
    assert all(back[k[len('module.'):].replace('layer2.net.', 'layer2.', 1).replace('new_fc.', 'fc.')] is v for k, v in raw.items())
    # only layer2's keys move: the other stages' shift wrappers keep their ``net``
    assert ('base_model.layer3.0.net.conv1.weight' if place == 'block' else 'base_model.layer3.0.conv1.net.weight') in back


def test_plain_checkpoint_keys_still_remap():
    sd = weights.make_state_dict(0, 12)
    ckpt = {'module.' + k: v for k, v in sd.items() if not k.startswith('fc.')}
    ckpt.update({'module.new_fc.weight': sd['fc.weight'], 'module.new_fc.bias': sd['fc.bias']})
    for flag in (False, True):
        back = weights.remap_checkpoint_keys(ckpt, 12, temporal_pool=flag)
        assert set(back) == set(sd) and all(back[k] is sd[k] for k in sd)
    assert set(wrapper_keys(sd)) != set(sd) and len(wrapper_keys(sd)) == len(sd)


def test_refusals_before_the_gpu(tmp_path, monkeypatch):
    """dtype='bf16', is_shift=False, an odd num_segments, non_local=True and an .onnx checkpoint: raised before the library is even
    loaded, by the engine class and by the factory alike."""
    def no_gpu(*_a, **_k):
        raise AssertionError('the refusal must come before the library is touched')
    monkeypatch.setattr(engine._lib, 'load', no_gpu)
    for make in (engine.TsmEngine, engine.create_model):
        with pytest.raises(NotImplementedError):
            make(temporal_pool=True, dtype='bf16')
        with pytest.raises(NotImplementedError):
            make(temporal_pool=True, non_local=True)
        with pytest.raises(ValueError):
            make(temporal_pool=True, is_shift=False)
        for t in (1, 3, 7):
            with pytest.raises(ValueError):
                make(temporal_pool=True, num_segments=t)
        with pytest.raises(AssertionError, match='before the library'):      # what is in scope does reach the library
            make(temporal_pool=True, num_segments=2, dtype='bf16x3', max_clips=1, height=64, width=64)
    onnx = tmp_path / 'model.onnx'
    onnx.write_bytes(b'')
    with pytest.raises(NotImplementedError):
        engine.create_model(checkpoint=str(onnx), temporal_pool=True)
    with pytest.raises(ValueError):
        flops.flops_per_clip(temporal_pool=True, num_segments=7)
    with pytest.raises(ValueError):
        flops.flops_per_clip(temporal_pool=True, non_local=True)


@pytest.mark.parametrize('base_model', ['resnet50', 'wide_resnet50_2', 'resnet18'])
def test_flops_from_the_shapes(base_model):
    """Layers 2-4 and the classifier, which runs per remaining frame, at half the frames; the stem and layer1 at all of them."""
    for t, size in ((8, 224), (4, 64), (2, 80)):
        rows = flops.layer_table(size, size, base_model)
        later = sum(r['macs'] for r in rows if r['name'].split('.')[0] in ('layer2', 'layer3', 'layer4'))
        assert 0 < later < sum(r['macs'] for r in rows)
        fc = weights.feature_width(base_model) * 12
        plain = flops.flops_per_clip(t, size, size, base_model=base_model)
        pooled = flops.flops_per_clip(t, size, size, base_model=base_model, temporal_pool=True)
        assert pooled < plain and plain - pooled == 2.0 * (later + fc) * (t // 2)
        assert flops.flops_per_clip(t, size, size, base_model=base_model, temporal_pool=False) == plain
    # R50 at 224^2, T = 8: layers 2-4 carry most of a forward's FLOPs
    ratio = flops.flops_per_clip(temporal_pool=True) / flops.flops_per_clip()
    assert 0.55 < ratio < 0.65, ratio


def test_pool_kernel_budgets():
    """temporal_maxpool_kernel<format> in the built code object, fp32 and split-bf16: no LDS, no scratch, no spill."""
    from workoutdetector_amd import codeobj
    from workoutdetector_amd.build import build_library
    md = codeobj.kernel_metadata(build_library())
    names = [k for k in md if k.startswith('temporal_maxpool_kernel<')]
    assert len(names) == 2, names
    for k in names:
        r = md[k]
        assert r['.group_segment_fixed_size'] == 0 and r['.private_segment_fixed_size'] == 0 and r['.vgpr_spill_count'] == 0, (k, r)
        assert r['.max_flat_workgroup_size'] == 256


def test_host_arithmetic_under_sanitizers(tmp_path):
    """tests/temporal_pool_host.cpp built with ASAN + UBSAN (runtimes linked statically: the program runs as it is) and run once."""
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path / 'temporal_pool_host')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan',
           '-static-libubsan', '-fno-omit-frame-pointer', '-Wall', '-Wextra', '-Werror', os.path.join(ROOT, 'tests', 'temporal_pool_host.cpp'),
           '-o', exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'runtime error' not in run.stdout + run.stderr and 'temporal_pool_host ok' in run.stdout
