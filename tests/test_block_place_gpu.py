"""Block placement of the temporal shift (``shift_place='block'``) on the MI355X: logits and stage taps against the CPU
reference (oracle/tsm_oracle.py) for R50 / R18 / R34 in every precision, the shifted-identity / shifted-second-source
arms of conv_igemm on every generic tile (bit-identical, asserted from the launch trace), the fused forms a block engine
refuses, the C ABI contract of tsm_set_shift_place, ONNX checkpoints and the counting pipeline.

Bars: f32 / bf16x3 rtol 1e-3 on logits and taps; bf16 against the bf16-storage restatement (BF16_E2E_BAR on logits,
BF16_TAP_BAR on taps)."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from oracle import tsm_oracle
from tests._util import BF16_TAP_BAR, IGEMM_TILE_DIMS, assert_close, bf16_logits_report, make_input

pytestmark = pytest.mark.gpu

BLOCK_ARM = 'kPrecBlockShift'   # how the launch trace spells the new conv_igemm arms (PREC | kPrecBlockShift)


def _sd(base_model, seed=0):
    from workoutdetector_amd.weights import make_state_dict
    return make_state_dict(seed, 12, base_model, shift_place='block')


def _t(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def _arms(tr):
    return [k for k in tr.kernels if k.startswith('conv_igemm<') and BLOCK_ARM in k]


# (base_model, dtype, B, T, H, W, shift_div): B = 1, odd T, T = 1 (every shifted channel reads zero), shift_div 4 / 16, odd sizes
CASES = [
    ('resnet50', 'f32', 2, 8, 224, 224, 8),
    ('resnet50', 'bf16x3', 2, 8, 224, 224, 8),
    ('resnet50', 'bf16', 2, 8, 224, 224, 8),
    ('resnet50', 'f32', 1, 3, 97, 131, 4),
    ('resnet50', 'bf16', 1, 5, 97, 131, 4),
    ('resnet50', 'bf16x3', 2, 1, 64, 96, 8),
    ('resnet18', 'f32', 2, 8, 224, 224, 8),
    ('resnet18', 'bf16x3', 1, 5, 97, 131, 8),
    ('resnet18', 'bf16', 2, 8, 224, 224, 8),
    ('resnet34', 'f32', 1, 3, 112, 144, 16),
    ('resnet34', 'bf16x3', 2, 8, 128, 128, 8),
    ('resnet34', 'bf16', 1, 1, 97, 131, 8),
]
TAPS = {'resnet50': ['layer1.0', 'layer1.2', 'layer2.0', 'layer3.3', 'layer4.0', 'layer4.2'],
        'resnet18': ['layer1.0.conv1', 'layer1.1', 'layer2.0', 'layer3.1', 'layer4.1'],
        'resnet34': ['layer1.2', 'layer2.0', 'layer2.3', 'layer3.0', 'layer4.2']}


@pytest.mark.parametrize('base_model,dtype,b,t,h,w,div', CASES)
def test_block_engine_against_reference(hip_lib, capsys, base_model, dtype, b, t, h, w, div):
    from workoutdetector_amd.engine import create_model, launch_trace
    sd = _sd(base_model)
    eng = create_model(num_class=12, num_segments=t, base_model=base_model, shift_div=div, shift_place='block', height=h,
                       width=w, max_clips=b, dtype=dtype)
    x = make_input(41, b, t, h, w)
    taps, taps16 = {}, {}
    want = tsm_oracle.forward(_t(sd), torch.from_numpy(x), base_model, 'block', n_segment=t, shift_div=div, taps=taps).numpy()
    with launch_trace() as tr:
        got = eng.run(None, {'input': x})[0]
    assert _arms(tr), tr.kernels
    assert not tr.ran('temporal_shift_kernel'), 'the shifted block input must never be materialised'
    what = f'{base_model} {dtype} B{b} T{t} {h}x{w} div{div}'
    if dtype == 'bf16':
        want16 = tsm_oracle.forward(_t(sd), torch.from_numpy(x), base_model, 'block', bf16=True, n_segment=t, shift_div=div,
                                    taps=taps16).numpy()
        bf16_logits_report(got, want16, want, what, capsys)
    else:
        assert_close(got, want, rtol=1e-3, atol_scale=1e-5, what=what + ' logits')
    for stage in TAPS[base_model]:
        g = eng.forward_tap(x, stage)
        if dtype == 'bf16':
            ref16 = taps16[stage].permute(0, 2, 3, 1).numpy()
            e = float(np.abs(g - ref16).max()) / float(np.abs(ref16).max())
            assert e <= BF16_TAP_BAR, (what, stage, e)
        else:
            assert_close(g, taps[stage].permute(0, 2, 3, 1).numpy(), rtol=1e-3, atol_scale=3e-5, what=f'{what} {stage}')
    eng.close()


@pytest.mark.parametrize('base_model,dtype,codes', [('resnet50', 'f32', (1, 2, 3, 4, 5, 0x103, 0x104)), ('resnet50', 'bf16x3', (1, 2, 3, 5)),
                                                    ('resnet50', 'bf16', (1, 2, 3, 5, 6, 8)), ('resnet18', 'f32', (1, 2, 3, 4, 5, 0x103, 0x104)),
                                                    ('resnet18', 'bf16', (1, 2, 3, 5))])
def test_every_generic_tile_is_bit_identical(hip_lib, monkeypatch, base_model, dtype, codes):
    """Each tile code forced through TSM_CONV_CODE gives the tuned forward's bits; the new arms ran on that tile (conv_igemm
    tiles), on the persistent 256x256 tile (its block arms), or, for the plain 256x256 tile, which has none, on a generic tile."""
    from workoutdetector_amd.engine import TsmEngine, create_model, launch_trace
    x = make_input(12, 2, 8, 112, 144)
    stages = ['layer1.0', 'layer2.0', 'layer3.1', 'layer4.0']
    kw = dict(num_class=12, base_model=base_model, shift_place='block', height=112, width=144, max_clips=2, dtype=dtype)
    eng = create_model(**kw)
    tuned = [eng.run(None, {'input': x})[0]] + [eng.forward_tap(x, s) for s in stages]
    eng.close()
    monkeypatch.setenv('TSM_AUTOTUNE', '0')
    for code in codes:
        monkeypatch.setenv('TSM_CONV_CODE', str(code))
        eng = create_model(**kw)
        with launch_trace() as tr:
            logits = eng.run(None, {'input': x})[0]
        arms = _arms(tr)
        if code & 0x100:   # split-K: R50's segmented layers run as (tile, segment) pieces and a reduction; a shifted R18 has no
            # segmented layer (its 3x3s are shifted or add the identity, its 1x1s are short), so the code falls back to whole-K
            assert tr.ran('splitk_reduce_kernel') == (base_model == 'resnet50'), (code, tr.kernels)
        name = TsmEngine.TILE_NAMES[code & 0xF]
        if name in IGEMM_TILE_DIMS:
            dims = '[BM = %d, BN = %d, WGM = %d, WGN = %d,' % IGEMM_TILE_DIMS[name]
            assert any(dims in k for k in arms), (code, arms)   # (fp32 long-K layers keep their segmented 64x64 / 32x32 tiles)
            if base_model == 'resnet50':   # a shifted identity (conv3) and a shifted downsample operand (conv3 + downsample)
                assert any('RES = true' in k and dims in k for k in arms), arms
                assert any(f'{BLOCK_ARM}, true' in k for k in arms), arms
            else:                          # a shifted identity (conv2) and the shifted 1x1 at stride 2 (downsample)
                assert any('KS = 3' in k for k in arms), arms
                assert any('KS = 1, SHIFT = true, RES = false' in k and dims in k for k in tr.kernels), tr.kernels
        elif code == 8:   # the persistent 256x256 tile has the shifted identity / second source of a 1x1 itself
            assert tr.ran('conv_bf16_256p_kernel<1, true, true, false>'), tr.kernels
            assert tr.ran('conv_bf16_256p_kernel<1, true, false, true>'), tr.kernels
        else:             # conv_bf16_256 has not: those launches run on conv_igemm
            assert arms, (code, tr.kernels)
            assert not tr.ran('conv_bf16_256_kernel<1, false, true'), tr.kernels
        got = [logits] + [eng.forward_tap(x, s) for s in stages]
        eng.close()
        for a, b, what in zip(got, tuned, ['logits'] + stages):
            assert np.array_equal(a, b), (base_model, dtype, code, what)


@pytest.mark.parametrize('dtype', ['f32', 'bf16x3', 'bf16'])
def test_fused_forms_are_refused_on_a_block_engine(hip_lib, monkeypatch, dtype):
    """TSM_FUSE_BLOCK / FRONT / CONV23 / C3C1 = 1 forced on a block engine: none of these forms reads a shifted identity,
    so every one is refused (absent from the trace) and the forward is bit-identical to all fusions off."""
    from workoutdetector_amd.engine import create_model, launch_trace
    x = make_input(5, 2, 8, 112, 112)
    kw = dict(num_class=12, shift_place='block', height=112, width=112, max_clips=2, dtype=dtype)
    out = {}
    for on in ('1', '0'):
        for var in ('TSM_FUSE_BLOCK', 'TSM_FUSE_FRONT', 'TSM_FUSE_CONV23', 'TSM_FUSE_C3C1'):
            monkeypatch.setenv(var, on)
        eng = create_model(**kw)
        with launch_trace() as tr:
            out[on] = eng.run(None, {'input': x})[0]
        for fam in ('bneck_ws_kernel', 'front_s2_kernel', 'conv23_fused_kernel', 'conv23_ws', 'conv31_fused_kernel',
                    'conv3x3_ws_kernel<true'):
            assert not tr.ran(fam), (dtype, on, fam)
        assert all('+' not in v for v in eng.conv_tiles(2).values())
        eng.close()
    assert np.array_equal(out['1'], out['0'])


def test_placement_matters(hip_lib):
    """Same numbers under both spellings of one seed: block and blockres logits differ; a blockres engine runs none of the
    new arms, a block engine does."""
    from workoutdetector_amd.engine import create_model, launch_trace
    x = make_input(6, 2, 8, 112, 112)
    got = {}
    for place in ('blockres', 'block'):
        eng = create_model(num_class=12, shift_place=place, height=112, width=112, max_clips=2, seed=3)
        with launch_trace() as tr:
            got[place] = eng.run(None, {'input': x})[0]
        assert bool(_arms(tr)) == (place == 'block'), (place, tr.kernels)
        eng.close()
    scale = float(np.abs(got['block']).max())
    assert float(np.abs(got['block'] - got['blockres']).max()) > 1e-3 * scale
    # is_shift=False ignores the placement
    a = create_model(num_class=12, is_shift=False, height=112, width=112, max_clips=2, seed=3)
    b = create_model(num_class=12, is_shift=False, shift_place='block', height=112, width=112, max_clips=2, seed=3)
    with launch_trace() as tr:
        nb = b.run(None, {'input': x})[0]
    assert np.array_equal(a.run(None, {'input': x})[0], nb) and not _arms(tr)
    a.close()
    b.close()


def test_set_shift_place_contract(hip_lib, tmp_path, monkeypatch):
    """tsm_set_shift_place: 0 / 1 between tsm_create and the first tsm_set_tensor, nothing else; blockres by default; block
    engines know the wrapped and the un-wrapped names but not blockres's conv1.net; tune-cache lines carry ' block' and
    neither placement reads the other's."""
    from workoutdetector_amd import _lib
    lib = _lib.load()
    cfg = _lib.TsmConfig(C.sizeof(_lib.TsmConfig), 12, 8, 64, 64, 8, 1, 1, 0, _lib.DTYPE_F32)
    h = C.c_void_p()
    _lib.check(lib.tsm_create(C.byref(cfg), C.byref(h)))
    try:
        assert lib.tsm_set_shift_place(h, 2) == -7 and lib.tsm_set_shift_place(h, -1) == -7
        one = np.ones(64, np.float32)
        shape = (C.c_int64 * 1)(64)
        w = np.ones(64 * 64, np.float32)
        wshape = (C.c_int64 * 4)(64, 64, 1, 1)
        assert lib.tsm_set_shift_place(h, 0) == 0 and lib.tsm_set_shift_place(h, 1) == 0
        assert lib.tsm_set_tensor(h, b'base_model.layer1.0.conv1.net.weight', w.ctypes.data, wshape, 4) == -1   # blockres name
        assert lib.tsm_set_shift_place(h, 0) == -1                                   # after the first tsm_set_tensor
        assert lib.tsm_set_tensor(h, b'base_model.layer1.0.net.conv1.weight', w.ctypes.data, wshape, 4) == 0
        assert lib.tsm_set_tensor(h, b'base_model.layer1.0.bn1.weight', one.ctypes.data, shape, 1) == 0        # un-wrapped
        assert lib.tsm_set_tensor(h, b'base_model.layer1.0.conv1.weight', w.ctypes.data, wshape, 4) == 0
    finally:
        lib.tsm_destroy(h)
    # a blockres checkpoint on a block engine fails loudly
    from workoutdetector_amd.engine import TsmEngine
    from workoutdetector_amd.weights import make_state_dict
    with pytest.raises(_lib.TsmError, match='missing'):
        TsmEngine(num_class=12, height=64, width=64, max_clips=1, shift_place='block', state_dict=make_state_dict(0, 12))
    from workoutdetector_amd.engine import create_model
    cache = tmp_path / 'tune.txt'
    monkeypatch.setenv('TSM_TUNE_CACHE', str(cache))
    create_model(num_class=12, shift_place='block', height=64, width=64, max_clips=1).warmup([1]).close()
    lines = cache.read_text().splitlines()
    assert len(lines) == 1 and ' block|' in lines[0]
    create_model(num_class=12, height=64, width=64, max_clips=1).warmup([1]).close()
    lines = cache.read_text().splitlines()
    assert len(lines) == 2 and ' block|' not in lines[1]
    create_model(num_class=12, base_model='resnet18', shift_place='block', height=64, width=64, max_clips=1).warmup([1]).close()
    lines = cache.read_text().splitlines()
    assert len(lines) == 3 and re.search(r' r18 block\|', lines[2])
    # a second process of each placement reads its own line: nothing new is appended
    create_model(num_class=12, shift_place='block', height=64, width=64, max_clips=1).warmup([1]).close()
    create_model(num_class=12, height=64, width=64, max_clips=1).warmup([1]).close()
    assert len(cache.read_text().splitlines()) == 3


@pytest.mark.parametrize('style', ['eval', 'training'])
def test_onnx_checkpoint_of_block_placement(hip_lib, tmp_path, style):
    from tests._torch_tsm import LitWrapper, TorchTSM, export_onnx
    from workoutdetector_amd.engine import create_model
    sd = _sd('resnet50', 7)
    path = str(tmp_path / f'block_{style}.onnx')
    export_onnx(LitWrapper(TorchTSM(shift_place='block').load_engine_state_dict(sd)), path,
                sample_shape=(1, 8, 3, 64, 64), training=(style == 'training'))
    eng = create_model(num_class=12, checkpoint=path, shift_place='block', height=96, width=112, max_clips=2)
    x = make_input(8, 2, 8, 96, 112)
    want = tsm_oracle.forward(_t(sd), torch.from_numpy(x), shift_place='block').numpy()
    assert_close(eng.run(None, {'input': x})[0], want, rtol=1e-3, atol_scale=1e-5, what=f'onnx block {style}')
    eng.close()


def test_counting_pipeline_with_a_block_engine(hip_lib):
    """Counting pipeline on a block engine (clip windows -> transform -> engine -> states -> count, inference_count): the
    states and the count equal the host state machine's on the reference logits of the same windows."""
    from oracle import counting_oracle, transform_oracle
    from tests._stub import synthetic_video
    from tests._util import fit_probe_fc
    from workoutdetector_amd import inference_count as ic
    from workoutdetector_amd.counting import pred_to_count, scores_to_preds
    from workoutdetector_amd.engine import TsmEngine
    from workoutdetector_amd.transform import build_test_transform
    from workoutdetector_amd.weights import make_state_dict
    sd = dict(_sd('resnet50'))
    probe = torch.from_numpy(synthetic_video(11, 96, 90, 52, period=24))
    fc_w, fc_b = fit_probe_fc(_t(make_state_dict(0, 12)), probe)   # (the same numbers in the blockres spelling)
    sd['fc.weight'], sd['fc.bias'] = fc_w.numpy(), fc_b.numpy()
    eng = TsmEngine(num_class=12, num_segments=8, max_clips=32, shift_place='block', state_dict=sd)
    vid = torch.from_numpy(synthetic_video(23, 140, 90, 52, period=24))
    got = ic.video_clip_logits(eng, vid, build_test_transform(False), batch_clips=32)
    want = torch.cat([tsm_oracle.forward(_t(sd), transform_oracle.clip_to_input(transform_oracle.make_clip(vid, s)),
                                         shift_place='block')
                      for s in range(0, 140, 8)])
    assert_close(got.numpy(), want.numpy(), rtol=1e-3, atol_scale=1e-5, what='block stream logits')
    states = scores_to_preds(got.tolist())
    assert states == counting_oracle.scores_to_preds(want.tolist())
    assert pred_to_count(states, 8) == counting_oracle.pred_to_count(states, 8)
    eng.close()
