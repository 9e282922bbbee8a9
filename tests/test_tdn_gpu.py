"""TDN engines (``TsmEngine(base_model='tdn_resnet50')``, include/tsm_hip.h: tsm_set_tdn) on the GPU, against the float64
tests/_tdn.py (pinned to the reference by tests/test_tdn_cpu.py) computing from the same fp32 weights.

Small depths: every kernel and every width runs and an engine is built in well under a second.  Sizes: 64 x 64 (trunk maps 16, 8,
4, 2: the mSE pools are 4, 2 and 2 -> 1), 96 x 160 (24 x 40 ... 3 x 5: not square, odd maps, pools 5 -> 2 -> 5 and 3 -> 1 -> 3) and
224 x 224 with two frames (7 -> 3 -> 7).

Bars, the project's own (tests/test_convnext_gpu.py): per operator, from the engine's own tap in front of it, rtol 1e-4 + 1e-4 of
the scale; network taps rtol 1e-3 + 3e-5 of the scale; logits rtol 1e-3 + 1e-5 of the scale.  Everything that compares two runs
of the engine is bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import _tdn
from tests._tdn_cases import LOGITS_BAR, NUM_CLASS, OP_BAR, TAP_BAR      # the bars of the docstring
from tests._tdn_cases import bits as _bits, engine as _cases_engine, tap_names as _tap_names, with_temporal as _with_temporal
from tests._tdn_cases import clips as _clips, network as _model, reference as _reference      # cached, shared, read-only
from tests._guard import guarded, guarded_out
from tests._util import assert_close

pytestmark = pytest.mark.gpu

D64, D96, D224, FLAT = (1, 1, 1, 2), (1, 2, 1, 2), (1, 1, 1, 2), (1, 1, 1, 1)


def _engine(h, w, T, depths, max_clips=3, sd=None, **kw):
    """tests/_tdn_cases.py: engine, of the seeded weights unless ``sd`` is given."""
    return _cases_engine(h, w, T, depths, sd if sd is not None else _model(depths, T)[1], max_clips=max_clips, **kw)


CASES = [(64, 64, D64, 2, 1, 'avg'), (64, 64, D64, 2, 3, 'identity'), (64, 64, D64, 3, 1, 'identity'), (64, 64, D64, 3, 3, 'avg'),
         (64, 64, D64, 8, 1, 'avg'), (64, 64, D64, 8, 3, 'identity'),
         (96, 160, D96, 2, 3, 'avg'), (96, 160, D96, 3, 1, 'avg'), (96, 160, D96, 3, 3, 'identity'), (96, 160, D96, 8, 1, 'identity'),
         (224, 224, D224, 2, 1, 'avg'), (224, 224, D224, 2, 1, 'identity')]


@pytest.mark.parametrize('h, w, depths, T, n, consensus', CASES, ids=lambda v: str(v).replace(' ', ''))
def test_taps_and_logits_against_float64(hip_lib, h, w, depths, T, n, consensus, capsys):
    x = _clips(h, w, T, n)
    seg, taps = _reference(h, w, depths, T, n)
    want = seg if consensus == 'identity' else seg.mean(1)
    eng = _engine(h, w, T, depths, max_clips=n, consensus=consensus)
    try:
        got = eng.forward_host(x)
        feats = eng.forward_features(x)
        worst = 0.0
        # every tap at the two smaller sizes; at 224 x 224 one block's worth (the 7 -> 3 -> 7 maps are layer4's)
        names = _tap_names(depths) if h < 224 else ['diff.stem', 'fuse2', 'layer4.1.conv1', 'layer4.1.mse.fwd', 'layer4.1.mse.bwd', 'layer4.1.shift', 'layer4.1']
        for name in names:
            worst = max(worst, assert_close(eng.forward_tap(x, name), taps[name], what=f'tap {name} at {h}x{w} T={T}', **TAP_BAR))
    finally:
        eng.close()
    assert got.shape == want.shape
    err = assert_close(got, want, what=f'logits at {h}x{w} T={T} n={n} {consensus}', **LOGITS_BAR)
    assert_close(feats, taps['features'], what='forward_features', **LOGITS_BAR)
    with capsys.disabled():
        print(f'\n[tdn {h}x{w} T={T} n={n} {consensus}] max|err|/scale: logits {err:.2g}, worst tap {worst:.2g}')


def test_the_gate_alone_and_the_temporal_conv_alone(hip_lib, capsys):
    """Temporal weights (0, 1, 0): the '.shift' tap is g, compared with the float64 gate of the engine's OWN conv1 tap, per
    operator.  The shift pattern in ONE block (everything in front of it unchanged, so its g is the same bits): o is
    tsm_temporal_shift(g, fold_div = 8), value for value -- once per width."""
    h, w, T, n, depths = 96, 160, 3, 2, D96
    model, weights = _model(depths, T)
    x = _clips(h, w, T, n)
    lib = hip_lib
    centre = _engine(h, w, T, depths, max_clips=n, sd=_with_temporal(weights))
    shifted = None
    worst = {}
    try:
        for li, b in ((2, 0), (2, 1), (3, 0), (4, 0), (4, 1)):
            p = f'layer{li}.{b}'
            c1 = centre.forward_tap(x, p + '.conv1')
            g = centre.forward_tap(x, p + '.shift')
            mse = getattr(model.base_model, f'layer{li}_bak')[b].mse
            with torch.no_grad():
                t = torch.from_numpy(c1).double().permute(0, 3, 1, 2)
                want_g = _tdn.nhwc(mse(t))
                ms, _es = mse.directions(t)
            worst[p] = assert_close(g, want_g, what=p + ' gate', **OP_BAR)
            for m, name in zip(ms, ('.mse.fwd', '.mse.bwd')):
                assert_close(centre.forward_tap(x, p + name), _tdn.nhwc(m), what=p + name, **OP_BAR)
            assert np.abs(g - c1).max() > 1e-2 * np.abs(c1).max()          # the gate does something
            if b != 0 and li != 4:
                continue
            shifted = _engine(h, w, T, depths, max_clips=n, sd=_with_temporal(weights, f'layer{li}_bak.{b}'))
            assert np.array_equal(_bits(c1), _bits(shifted.forward_tap(x, p + '.conv1')))
            o = shifted.forward_tap(x, p + '.shift')
            shifted.close()
            gd = torch.from_numpy(g).cuda()
            od = torch.empty_like(gd)
            nf, hh, ww, c = g.shape
            assert lib.tsm_temporal_shift(gd.data_ptr(), od.data_ptr(), nf, T, hh * ww, c, 8, None) == 0
            torch.cuda.synchronize()
            assert np.array_equal(o, od.cpu().numpy()), p          # (values: -0 counts as 0)
            assert not np.array_equal(o, g)
    finally:
        centre.close()
        if shifted is not None:
            shifted.close()
    with capsys.disabled():
        print('\n[tdn gate per-op] max|err|/scale: ' + ', '.join(f'{k} {v:.2g}' for k, v in worst.items()))


def test_a_clip_does_not_depend_on_its_batch_or_its_chunk(hip_lib):
    """64 x 64, depths (1, 1, 1, 1): a clip alone, first and last in a batch of 3; and 10 clips through an engine of 10 (front-end
    chunks of 8 and 2): the clips either side of the chunk boundary equal their single-clip forwards bit for bit."""
    h, w, T = 64, 64, 3
    x = _clips(h, w, T, 10)
    eng = _engine(h, w, T, FLAT, max_clips=10)
    try:
        assert eng.tdn_chunk_clips == 8
        alone = {i: eng.forward_host(x[i:i + 1]) for i in (0, 2, 7, 8, 9)}
        three = eng.forward_host(x[:3])
        ten = eng.forward_host(x)
        tap10 = eng.forward_tap(x, 'diff.conv1_5')
        tap8 = eng.forward_tap(x[8:9], 'diff.conv1_5')
    finally:
        eng.close()
    assert np.array_equal(_bits(three[0:1]), _bits(alone[0])) and np.array_equal(_bits(three[2:3]), _bits(alone[2]))
    for i in (0, 7, 8, 9):
        assert np.array_equal(_bits(ten[i:i + 1]), _bits(alone[i])), i
    assert np.array_equal(_bits(tap10[8 * T:9 * T]), _bits(tap8))
    assert not np.array_equal(ten[7], ten[8])


def test_every_tile_code_gives_the_same_bits(hip_lib):
    """The tuned engine's codes (tsm_conv_tiles), each forced on every conv through TSM_CONV_CODE: the same logits, bit for bit."""
    from workoutdetector_amd import _lib
    h, w, T, n = 64, 64, 2, 2
    x = _clips(h, w, T, n)
    eng = _engine(h, w, T, D64, max_clips=n, autotune=True)
    try:
        eng.warmup([n])
        base = eng.forward_host(x)
        buf, cnt = (C.c_int32 * 256)(), C.c_int32()
        _lib.check(hip_lib.tsm_conv_tiles(eng._h, n, buf, 256, C.byref(cnt)), eng._h)
        codes = sorted(({buf[i] & 0x3FF for i in range(cnt.value)} | {1, 2, 3, 4, 5, 3 | 0x100}) - {0})
        names = eng.conv_tiles(n)
        # the stem, conv1_5, three convs per block of both paths, a downsample in resnext_layer1 and in each trunk stage; every
        # conv that goes through the tuner has a code (not the stem, which runs its own pool-fused kernel, and not a downsample,
        # which runs inside conv3's GEMM)
        assert cnt.value == len(names) == 2 + 3 * (D64[0] + sum(D64)) + 5 and list(names)[:2] == ['conv1', 'diff.conv1_5']
        assert all(buf[i] > 0 for i, name in enumerate(names) if name != 'conv1' and not name.endswith('.downsample')), list(buf[:cnt.value])
    finally:
        eng.close()
    for code in codes:
        forced = _engine(h, w, T, D64, max_clips=n, code=code)
        try:
            assert np.array_equal(_bits(forced.forward_host(x)), _bits(base)), f'code {code:#x}'
        finally:
            forced.close()
    seg, _taps = _reference(h, w, D64, T, n)
    assert_close(base, seg.mean(1), what='tuned engine', **LOGITS_BAR)


MSE_ORDER = ('mse_squeeze_kernel', 'mse_diff_kernel', 'mse_s2_kernel', 'mse_mix_kernel', 'mse_excite_shift_kernel')


def test_the_launches_between_conv1_and_conv2(hip_lib):
    """A whole forward: one tdn_front + conv1_5 pair per chunk, two blends, and per BottleneckShift exactly the five mse launches,
    in order, directly behind a conv_igemm (conv1) and in front of a conv (conv2, alone or fused with conv3).  The tap pair
    conv1 / conv2 of one block brackets the same five and nothing else."""
    from workoutdetector_amd.engine import launch_trace
    h, w, T, n = 64, 64, 2, 2
    x = _clips(h, w, T, n)
    eng = _engine(h, w, T, D64, max_clips=n)
    try:
        with launch_trace() as tr:
            eng.forward_host(x)
        with launch_trace() as t1:
            eng.forward_tap(x, 'layer3.0.conv1')
        with launch_trace() as t2:
            eng.forward_tap(x, 'layer3.0.conv2')
        times_names = eng.launch_names()
        eng.set_layer_timing(1)
        eng.forward_host(x)
        times = eng.layer_times_ms(0)
    finally:
        eng.close()
    k = tr.kernels
    shift_blocks = sum(D64[1:])
    assert tr.count('tdn_front_kernel') == 1 and tr.count('tdn_fuse_kernel') == 2 and tr.count('stem_pool_f32_kernel') == 1
    for name in MSE_ORDER:
        assert tr.count(name) == shift_blocks, (name, k)
    starts = [i for i, name in enumerate(k) if name.startswith('mse_squeeze_kernel')]
    for i in starts:
        assert [n_.split('<')[0] for n_ in k[i:i + 5]] == list(MSE_ORDER), k[i:i + 6]
        assert k[i - 1].startswith('conv_igemm<') and k[i + 5].startswith(('conv_igemm<', 'conv23_fused')), k[i - 1:i + 6]
    widths = [re.search(r'<(\d+)>', k[i + 4]).group(1) for i in starts]
    assert widths == ['128', '256', '512', '512']
    between = t2.kernels[len(t1.kernels):]
    assert t2.kernels[:len(t1.kernels)] == t1.kernels
    assert [n_.split('<')[0] for n_ in between[:5]] == list(MSE_ORDER) and len(between) == 6 and between[5].startswith('conv_igemm<'), between
    # every new launch has a timing slot of its own
    assert list(times) == times_names and all(times[name] > 0 for name in times if '.mse_' in name or name.startswith(('diff.', 'fuse')) or name == 'conv1')
    assert sum('.mse_' in name for name in times) == 5 * shift_blocks


def test_the_whole_engine_under_poison(hip_lib):
    """TSM_POISON=1: every buffer, the patch rows and the nine r-channel maps included, between poisoned bands and poison all over
    before each forward.  Logits and taps keep their bits, and no launch stores into a band (TSM_ERR_GUARD would raise)."""
    h, w, T, n = 96, 160, 3, 2
    x = _clips(h, w, T, n)
    plain, hostile = _engine(h, w, T, D96, max_clips=3), _engine(h, w, T, D96, max_clips=3, poison=True)
    try:
        assert np.array_equal(_bits(plain.forward_host(x)), _bits(hostile.forward_host(x)))
        assert np.array_equal(_bits(plain.forward_host(x[:1])), _bits(hostile.forward_host(x[:1])))
        for name in ('diff.conv1_5', 'fuse2', 'layer2.1.mse.bwd', 'layer3.0.shift', 'layer4.1.mse.fwd', 'layer4.1'):
            assert np.array_equal(_bits(plain.forward_tap(x, name)), _bits(hostile.forward_tap(x, name))), name
        assert np.array_equal(_bits(plain.forward_features(x)), _bits(hostile.forward_features(x)))
    finally:
        plain.close()
        hostile.close()


def test_forward_captured_on_a_side_stream_replays_the_eager_logits(hip_lib):
    from tests._capture import captured
    h, w, T, b = 64, 64, 2, 2
    sets = [torch.from_numpy(np.random.default_rng([43, k]).standard_normal((b, T, 15, h, w)).astype(np.float32)) for k in range(3)]
    eng = _engine(h, w, T, D64, max_clips=b, autotune=True)
    try:
        x = guarded(torch.zeros(b, T, 15, h, w).cuda(), name='clips')
        out = guarded_out(eng._out_shape(b), name='logits')
        eng.warmup([b])
        tr = captured(lambda: eng.forward_device(x, out=out), [x], lambda k: [sets[k]], [out], engine=eng)
    finally:
        eng.close()
    model, _w = _model(D64, T)
    with torch.no_grad():
        want = model(sets[0].reshape(b * T, 15, h, w).double()).mean(1).numpy()
    assert tr.count('mse_excite_shift_kernel') == sum(D64[1:]) and tr.count('tdn_front_kernel') == 1
    assert_close(tr.refs['A'][0].cpu().numpy(), want, what='captured forward, set A', **LOGITS_BAR)


def test_a_checkpoint_file_loads_through_create_tdn_model(hip_lib, tmp_path):
    """A DataParallel-style checkpoint ('state_dict', 'module.' prefix, num_batches_tracked, conv1_temp) written here loads through
    create_tdn_model; the [B*T*5, 3, H, W] spelling of the input gives the 6-D spelling's logits."""
    from workoutdetector_amd.engine import create_tdn_model
    h, w, T, n = 64, 64, 8, 2
    model, weights = _model(D64, T)
    sd = {'module.' + k: torch.from_numpy(np.array(v)) for k, v in weights.items()}
    sd['module.base_model.bn1.num_batches_tracked'] = torch.zeros((), dtype=torch.long)
    path = str(tmp_path / 'tdn.pth')
    torch.save({'state_dict': sd}, path)
    keep = os.environ.get('TSM_AUTOTUNE')
    os.environ['TSM_AUTOTUNE'] = '0'
    try:
        eng = create_tdn_model(NUM_CLASS, num_segments=T, checkpoint=path, height=h, width=w, max_clips=n, depths=D64)
    finally:
        os.environ.pop('TSM_AUTOTUNE', None)
        if keep is not None:
            os.environ['TSM_AUTOTUNE'] = keep
    x = _clips(h, w, T, n)
    try:
        assert (eng.base_model, eng.tdn_depths, eng.planes, eng.feature_dim) == ('tdn_resnet50', D64, 15, 2048)
        assert eng.get_inputs()[0].shape == [None, T, 15, h, w]
        six = eng(x.reshape(n, T, 5, 3, h, w))
        four = eng(x.reshape(n * T * 5, 3, h, w))
        fifteen = eng(torch.from_numpy(np.array(x).reshape(n * T, 15, h, w)))
        ort = eng.run(None, {'input': x.reshape(n, T, 5, 3, h, w)})[0]
        with pytest.raises(ValueError):
            eng(x.reshape(n * T * 5, 3, h, w)[:-1])
    finally:
        eng.close()
    assert np.array_equal(_bits(six), _bits(four)) and np.array_equal(_bits(six), _bits(fifteen.numpy())) and np.array_equal(_bits(six), _bits(ort))
    seg, _taps = _reference(h, w, D64, T, n)      # T = 8: alpha = beta = 0.5, tdn_net's rule on both sides
    assert_close(six, seg.mean(1), what='checkpoint engine', **LOGITS_BAR)
    with pytest.raises(ValueError, match=r'\[7, 2048\].*\[3, 2048\]'):
        create_tdn_model(3, num_segments=T, checkpoint=path, height=h, width=w, depths=D64)


def test_the_setter_contract(hip_lib):
    """tsm_set_tdn's statuses and texts, the other topology calls on a TDN engine, the layouts a TDN forward takes."""
    from workoutdetector_amd import _lib
    lib = hip_lib
    base = (C.c_int32 * 4)(3, 4, 6, 3)

    def engine(t=8, shift=0, dtype=_lib.DTYPE_F32, h=64, w=64):
        cfg = _lib.TsmConfig(C.sizeof(_lib.TsmConfig), 3, t, h, w, 8, shift, 1, 0, dtype)
        e = C.c_void_p()
        _lib.check(lib.tsm_create(C.byref(cfg), C.byref(e)))
        return e

    def refused(e, code, text, depths=base):
        assert lib.tsm_set_tdn(e, depths, 0.5, 0.5) == code
        assert text in lib.tsm_last_error(e).decode(), lib.tsm_last_error(e)

    for kw, text in ((dict(dtype=_lib.DTYPE_BF16X3), 'TSM_DTYPE_F32 only'), (dict(dtype=_lib.DTYPE_BF16), 'TSM_DTYPE_F32 only'),
                     (dict(shift=1), 'is_shift must be 0'), (dict(t=1), 'num_segments >= 2'), (dict(h=32), 'multiples of 32'),
                     (dict(w=80), 'multiples of 32')):
        e = engine(**kw)
        refused(e, -7, text)
        lib.tsm_destroy(e)
    e = engine()
    refused(e, -7, '1 .. 64', (C.c_int32 * 4)(3, 0, 6, 3))
    refused(e, -7, '1 .. 64', (C.c_int32 * 4)(3, 4, 65, 3))
    refused(e, -1, 'depths is NULL', None)
    assert lib.tsm_set_tdn(e, base, float('nan'), 0.5) == -1
    assert lib.tsm_set_tdn(e, base, 0.5, 0.5) == 0 and lib.tsm_set_tdn(e, (C.c_int32 * 4)(*FLAT), 0.75, 0.25) == 0      # (the last call holds)
    for call in (lambda: lib.tsm_set_backbone(e, 18), lambda: lib.tsm_set_bottleneck_width(e, 128), lambda: lib.tsm_set_shift_place(e, 1),
                 lambda: lib.tsm_set_non_local(e, 1), lambda: lib.tsm_set_temporal_pool(e, 1), lambda: lib.tsm_set_convnext(e, base)):
        assert call() == -7 and 'TDN engine' in lib.tsm_last_error(e).decode()
    assert lib.tsm_set_consensus(e, 1) == 0
    one = np.ones(2048, np.float32)
    assert lib.tsm_set_tensor(e, b'base_model.layer2_bak.0.shift.conv.weight', one.ctypes.data, (C.c_int64 * 3)(128, 1, 3), 3) == 0
    assert lib.tsm_set_tensor(e, b'base_model.layer2_bak.1.shift.conv.weight', one.ctypes.data, (C.c_int64 * 3)(128, 1, 3), 3) == -1   # FLAT has one block
    assert lib.tsm_set_tensor(e, b'base_model.conv1_temp.bias', one.ctypes.data, (C.c_int64 * 1)(64), 1) == 0
    assert lib.tsm_set_tensor(e, b'base_model.layer1_bak.0.mse.conv1.weight', one.ctypes.data, (C.c_int64 * 1)(64), 1) == -1          # layer1 has no mSE
    assert lib.tsm_set_tensor(e, b'fc.weight', one.ctypes.data, (C.c_int64 * 1)(64), 1) == -1
    refused(e, -1, 'must come before the first tsm_set_tensor')
    assert lib.tsm_finalize(e) == -4 and 'missing' in lib.tsm_last_error(e).decode()
    lib.tsm_destroy(e)
    for setter, arg in ((lib.tsm_set_backbone, 50), (lib.tsm_set_non_local, 1)):
        e = engine()
        assert setter(e, arg) == 0
        refused(e, -7, 'excludes')
        lib.tsm_destroy(e)
    # layouts: NTCHW only
    eng = _engine(64, 64, 2, FLAT, max_clips=1)
    try:
        x = torch.zeros(1, 2, 15, 64, 64).cuda()
        out = torch.zeros(1, NUM_CLASS).cuda()
        for layout in (_lib.LAYOUT_NTHWC, _lib.LAYOUT_NTHWC4):
            assert lib.tsm_forward(eng._h, x.data_ptr(), _lib.MEM_DEVICE, layout, 1, out.data_ptr(), None) == -7
            assert 'TSM_LAYOUT_NTCHW only' in lib.tsm_last_error(eng._h).decode()
        torch.cuda.synchronize()
    finally:
        eng.close()
