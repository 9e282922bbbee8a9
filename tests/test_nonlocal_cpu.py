"""create_model(non_local=True) without a GPU: the state-dict keys against a torch module with the module tree of the non-local
wrapper, the seeded weights (a second generator: no existing number moves), the sharpness of the seeded model's attention (neither
uniform nor one-hot, or the GPU tests could not see an indexing error), the FLOP count against a hand count, the pure-host
arithmetic under ASAN + UBSAN (tests/nonlocal_host.cpp, a stand-alone program), and the refusals that never reach the GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests._nonlocal import clip_input, run_with_taps, torch_tsm_nl
from workoutdetector_amd import engine, flops, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('place', ['blockres', 'block'])
@pytest.mark.parametrize('base_model', ['resnet50', 'wide_resnet50_2'])
def test_module_keys_equal_required_keys(base_model, place):
    net = torch_tsm_nl(base_model, place)
    have = {k.replace('new_fc.', 'fc.') for k in net.state_dict() if not k.endswith('num_batches_tracked')}
    want = set(weights.required_keys(base_model=base_model, shift_place=place, non_local=True))
    assert have == want, (sorted(have - want)[:5], sorted(want - have)[:5])
    sd = weights.make_state_dict(0, 12, base_model, place, non_local=True)
    assert set(sd) == want
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    for k, v in sd.items():
        assert tuple(v.shape) == shapes[k.replace('fc.', 'new_fc.') if k.startswith('fc.') else k], k
    assert sd['base_model.layer2.0.nl.theta.weight'].shape == (256, 512, 1, 1, 1)
    assert sd['base_model.layer3.4.nl.W.0.weight'].shape == (1024, 512, 1, 1, 1)
    block = 'base_model.layer2.0.block.net.conv1.weight' if place == 'block' else 'base_model.layer2.0.block.conv1.net.weight'
    plain = 'base_model.layer2.1.net.conv2.weight' if place == 'block' else 'base_model.layer2.1.conv2.weight'
    assert block in want and plain in want and not any(k.startswith('base_model.layer2.1.block') for k in want)


@pytest.mark.parametrize('place', ['blockres', 'block'])
def test_seeded_weights_keep_every_existing_number(place):
    plain = weights.make_state_dict(3, 12, 'resnet50', place)
    nl = weights.make_state_dict(3, 12, 'resnet50', place, non_local=True)
    assert len(nl) == len(plain) + 5 * 12
    for k, v in plain.items():
        k2 = k
        for li, b in weights.NL_BLOCKS:
            p = f'base_model.layer{li}.{b}.'
            if k.startswith(p):
                k2 = p + 'block.' + k[len(p):]
        assert nl[k2].tobytes() == v.tobytes(), k
    again = weights.make_state_dict(3, 12, 'resnet50', place, non_local=True)
    assert all(again[k].tobytes() == v.tobytes() for k, v in nl.items())
    other = weights.make_state_dict(4, 12, 'resnet50', place, non_local=True)
    assert other['base_model.layer2.0.nl.theta.weight'].tobytes() != nl['base_model.layer2.0.nl.theta.weight'].tobytes()
    # W's BatchNorm is NOT the zero of the original init (under which the block is the identity and no test could fail)
    assert np.abs(nl['base_model.layer3.2.nl.W.1.weight']).min() > 0.2


@pytest.mark.parametrize('size', [64, 48])
def test_seeded_attention_is_neither_uniform_nor_one_hot(size):
    """In every wrapped block of the float64 seeded model at least 90 % of the softmax rows have their largest probability strictly
    between 2 / N_k and 0.9; and the block is not the identity."""
    sd = weights.make_state_dict(0, 12, non_local=True)
    net = torch_tsm_nl(sd=sd)
    x = clip_input(5, 1, 8, size, size)
    _logits, _seg, _pooled, taps, sharp = run_with_taps(net, x)
    assert len(sharp) == 5
    for name, (row_max, nk) in sharp.items():
        frac = float(((row_max > 2.0 / nk) & (row_max < 0.9)).mean())
        print(f'{size}x{size} {name}: N_k {nk}, rows inside (2 / N_k, 0.9): {frac:.3f}, median max p {np.median(row_max):.3f}')
        assert frac >= 0.9, (name, nk, frac)
    moved = np.abs(taps['layer2.0'] - taps['layer2.0.block']).mean() / np.abs(taps['layer2.0.block']).mean()
    assert moved > 0.05, moved


def test_flops_against_a_hand_count():
    # 224^2, T = 8.  layer2: 28 x 28, C = 512, d = 256, N_q = 6272, N_k = 8 * 14 * 14 = 1568; layer3: 14 x 14, C = 1024, d = 512,
    # N_q = 1568, N_k = 8 * 7 * 7 = 392.  Per block: convs N_q * (C * 3 d + d * C) MACs, attention 2 * N_q * N_k * d MACs.
    l2 = 6272 * (512 * 768 + 256 * 512) + 2 * 6272 * 1568 * 256
    l3 = 1568 * (1024 * 1536 + 512 * 1024) + 2 * 1568 * 392 * 512
    added = 2.0 * (2 * l2 + 3 * l3)
    got = flops.flops_per_clip(non_local=True) - flops.flops_per_clip()
    assert got == added
    assert 56.5e9 < added < 57.0e9
    attn = 2.0 * sum(r['attn_macs'] for r in flops.nonlocal_table())
    assert 23.5e9 < attn < 24.5e9
    assert flops.flops_per_clip(non_local=False) == flops.flops_per_clip()
    assert flops.flops_per_clip(base_model='wide_resnet50_2', non_local=True) - flops.flops_per_clip(base_model='wide_resnet50_2') == added
    with pytest.raises(NotImplementedError):
        flops.flops_per_clip(base_model='resnet18', non_local=True)
    rows = flops.nonlocal_table(8, 80, 80)        # 10 x 10 -> 5 x 5 and 5 x 5 -> 2 x 2: the floor drops a row and a column
    assert [(r['nq'], r['nk']) for r in rows] == [(800, 200)] * 2 + [(200, 32)] * 3


def test_host_arithmetic_under_sanitizers(tmp_path):
    """tests/nonlocal_host.cpp built with ASAN + UBSAN (runtimes linked statically: the program runs as it is) and run once."""
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path / 'nonlocal_host')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan',
           '-static-libubsan', '-fno-omit-frame-pointer', '-Wall', '-Wextra', '-Werror', os.path.join(ROOT, 'tests', 'nonlocal_host.cpp'),
           '-o', exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'runtime error' not in run.stdout + run.stderr and 'nonlocal_host ok' in run.stdout


def test_attention_kernel_budgets():
    """nonlocal_attn_kernel<D> in the built code object: static LDS below the 64 KB that needs no opt-in, the D / 128 * 2 output
    tiles in accumulation registers, no scratch, two workgroups per CU for D = 256 and one for D = 512."""
    from workoutdetector_amd import codeobj
    from workoutdetector_amd.build import build_library
    md = codeobj.kernel_metadata(build_library())
    for d, agprs, groups in ((256, 64, 2), (512, 128, 1)):
        r = md[f'nonlocal_attn_kernel<{d}>']
        assert r['.max_flat_workgroup_size'] == 256 and r['.group_segment_fixed_size'] == 56576, r
        assert r['.private_segment_fixed_size'] == 0 and r['.vgpr_spill_count'] == 0
        assert r['.agpr_count'] >= agprs and r['.vgpr_count'] <= codeobj.SIMD_VGPRS // groups, (d, r['.vgpr_count'], r['.agpr_count'])
        assert r['workgroups_per_cu'] >= groups, (d, r['workgroups_per_cu'])
    r = md['maxpool2x2_kernel']
    assert r['.group_segment_fixed_size'] == 0 and r['.private_segment_fixed_size'] == 0


def test_refusals_before_the_gpu(tmp_path, monkeypatch):
    """resnet18 / resnet34, the bf16 formats and an .onnx checkpoint: NotImplementedError before the library is even loaded."""
    def no_gpu(*_a, **_k):
        raise AssertionError('the refusal must come before the library is touched')
    monkeypatch.setattr(engine._lib, 'load', no_gpu)
    for base_model in ('resnet18', 'resnet34'):
        with pytest.raises(NotImplementedError):
            engine.create_model(base_model=base_model, non_local=True)
        with pytest.raises(NotImplementedError):
            engine.TsmEngine(base_model=base_model, non_local=True)
    for dtype in ('bf16', 'bf16x3'):
        with pytest.raises(NotImplementedError):
            engine.create_model(non_local=True, dtype=dtype)
        with pytest.raises(NotImplementedError):
            engine.TsmEngine(non_local=True, dtype=dtype)
    onnx = tmp_path / 'model.onnx'
    onnx.write_bytes(b'')
    with pytest.raises(NotImplementedError):
        engine.create_model(checkpoint=str(onnx), non_local=True)
    with pytest.raises(NotImplementedError):
        weights.make_state_dict(0, 12, 'resnet34', non_local=True)
    with pytest.raises(KeyError):        # a plain checkpoint is not silently run as the non-local network
        weights.remap_checkpoint_keys({'module.' + k: v for k, v in weights.make_state_dict(0, 12).items()}, 12, non_local=True)
    sd = weights.make_state_dict(0, 12, non_local=True)
    ckpt = {'module.' + k: v for k, v in sd.items() if not k.startswith('fc.')}      # a checkpoint ends in its classifier
    ckpt.update({'module.new_fc.weight': sd['fc.weight'], 'module.new_fc.bias': sd['fc.bias']})
    back = weights.remap_checkpoint_keys(ckpt, 12, non_local=True)
    assert set(back) == set(sd) and all(back[k] is sd[k] for k in sd)
