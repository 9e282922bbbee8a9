"""create_model(non_local=True) on the MI355X: the two new kernels per op in hostile memory (tests/_guard.py) against float64 /
torch, and the engine against the float64 torch model with the wrapper's module tree (tests/_nonlocal.py).

Bars.  Attention per op: ``assert_close(rtol=1e-4, atol_scale=1e-4)`` against the float64 reference, the per-op conv bar (torch's
own fp32 composite sits at 3e-7 .. 1e-6 of the scale against float64).  Max-pool: bit-exact against torch.  Engine: the existing
engine bars, logits ``rtol=1e-3, atol_scale=1e-5`` and taps ``atol_scale=3e-5``.

Frames.  Square ones and the non-square ones of tests/_geometry_cases.py (48 x 80, 80 x 48, 64 x 112, 32 x 64): at H = W an exchange
of rows and columns in the host plumbing changes no bit (tests/test_geometry_cases_cpu.py), so every engine-level check also runs
where they differ, with tap shapes asserted from that table."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _geometry_cases as G
from tests._guard import POISON, check, guarded, guarded_out
from tests._nonlocal import TAPS, attention_ref, clip_input, run_with_taps, torch_tsm_nl
from tests._util import assert_close

pytestmark = pytest.mark.gpu

OP_BAR = dict(rtol=1e-4, atol_scale=1e-4)


# ---- nonlocal_attn_kernel per op --------------------------------------------------------------------------------------------
def _qkv(seed, b, nq, nk, d, spread=1.5):
    """q, k with scores of standard deviation ``spread`` (softmax neither uniform nor one-hot), v ~ N(0, 1): CPU float32."""
    g = torch.Generator().manual_seed(seed)
    s = (spread / d ** 0.5) ** 0.5
    return (torch.randn(b, nq, d, generator=g) * s, torch.randn(b, nk, d, generator=g) * s, torch.randn(b, nk, d, generator=g))


def _attend(q, k, v, what):
    """The kernel between guards on (CPU) q, k, v -> its output (CUDA), compared with the float64 reference at the bar."""
    from workoutdetector_amd.engine import nonlocal_attention
    gq, gk, gv = (guarded(t.cuda(), name=n) for t, n in ((q, 'q'), (k, 'k'), (v, 'v')))
    out = guarded_out(q.shape, name='y')
    got = nonlocal_attention(gq, gk, gv, out=out)
    assert got is out
    torch.cuda.synchronize()
    check(out, gq, gk, gv)
    assert_close(out.cpu().numpy(), attention_ref(q, k, v).numpy(), what=what, **OP_BAR)
    return out


@pytest.mark.parametrize('nk', [1, 8, 31, 64, 65, 100])
@pytest.mark.parametrize('nq', [1, 63, 64, 65, 200])
@pytest.mark.parametrize('d', [256, 512])
def test_attention_against_float64(hip_lib, d, nq, nk):
    q, k, v = _qkv(1000 * d + 10 * nq + nk, 2, nq, nk, d)
    _attend(q, k, v, f'd {d} nq {nq} nk {nk}')


@pytest.mark.parametrize('d', [256, 512])
def test_attention_strided_operands(hip_lib, d):
    """q a column slice of a [.., 3 d] tensor, k / v slices of a [.., 2 d] one; every other channel holds NaN."""
    from workoutdetector_amd.engine import nonlocal_attention
    b, nq, nk = 2, 70, 37
    q, k, v = _qkv(d + 1, b, nq, nk, d)
    wide_q = torch.full((b, nq, 3 * d), float('nan'))
    wide_q[..., d:2 * d] = q
    gq = guarded(wide_q.cuda(), name='qkv')
    gkv = guarded(torch.cat([k, v], dim=2).cuda(), name='kv')
    out = guarded_out((b, nq, d), name='y')
    nonlocal_attention(gq[..., d:2 * d], gkv[..., :d], gkv[..., d:], out=out)
    torch.cuda.synchronize()
    check(out, gq, gkv)
    assert_close(out.cpu().numpy(), attention_ref(q, k, v).numpy(), what=f'strided d {d}', **OP_BAR)
    dense = _attend(q, k, v, f'dense d {d}')
    assert torch.equal(out, dense), 'the row strides must not change a bit'


@pytest.mark.parametrize('d', [256, 512])
def test_attention_clips_are_independent_and_launches_repeat(hip_lib, d):
    """n_clips = 3 with different keys per clip: each clip equals its own single-clip launch bit for bit; two identical launches
    agree bit for bit."""
    q, k, v = _qkv(d + 2, 3, 130, 75, d)
    all3 = _attend(q, k, v, f'3 clips d {d}')
    again = _attend(q, k, v, f'3 clips again d {d}')
    assert torch.equal(all3, again)
    for c in range(3):
        one = _attend(q[c:c + 1], k[c:c + 1], v[c:c + 1], f'clip {c} d {d}')
        assert torch.equal(one[0], all3[c]), f'clip {c} depends on its position in the batch'


@pytest.mark.parametrize('d', [256, 512])
def test_attention_large_logits_do_not_overflow(hip_lib, d):
    """Rows whose largest logit is about +100: exp(100) is inf in fp32, so this needs the maximum subtracted."""
    q, k, v = _qkv(d + 3, 2, 66, 100, d)
    for i in range(q.shape[1]):
        j = (7 * i) % k.shape[1]
        q[:, i] = q[:, i] + k[:, j] * ((100.0 - (q[:, i] * k[:, j]).sum(-1)) / (k[:, j] * k[:, j]).sum(-1)).unsqueeze(-1)
    top = (q.double() @ k.double().transpose(1, 2)).max(-1).values
    assert 99.0 < float(top.min()) and float(top.max()) < 140.0
    _attend(q, k, v, f'logits +100 d {d}')


@pytest.mark.parametrize('d', [256, 512])
def test_attention_maximum_in_any_key_tile(hip_lib, d):
    """nk = 200 is four key tiles (64, 64, 64, 8).  Row groups whose maximum lies in the first tile (the running maximum never
    moves again: rescale factor 1), a middle tile, the last tile (the accumulators are rescaled), and rows whose maximum rises
    with every tile."""
    q, k, v = _qkv(d + 4, 2, 128, 200, d)
    kn = k / (k * k).sum(-1, keepdim=True)
    for i in range(q.shape[1]):
        group = i % 4
        if group < 3:
            q[:, i] += 14.0 * kn[:, (5, 100, 197)[group]]
        else:
            q[:, i] += 4.0 * kn[:, 20] + 7.0 * kn[:, 90] + 10.0 * kn[:, 150] + 13.0 * kn[:, 195]
    tile = (q.double() @ k.double().transpose(1, 2)).argmax(-1) // 64
    for group, want in enumerate((0, 1, 3)):
        assert bool((tile[:, group::4] == want).all()), group
    _attend(q, k, v, f'maximum placement d {d}')


def test_attention_refuses_other_widths(hip_lib):
    from workoutdetector_amd import _lib
    from workoutdetector_amd.engine import launch_trace, nonlocal_attention
    q, k, v = _qkv(9, 1, 16, 16, 128)
    out = guarded_out(q.shape, name='y')
    with launch_trace() as tr:
        with pytest.raises(_lib.TsmError) as err:
            nonlocal_attention(q.cuda(), k.cuda(), v.cuda(), out=out)
    assert err.value.status == -7 and not tr.kernels      # TSM_ERR_UNSUPPORTED, nothing launched
    torch.cuda.synchronize()
    assert bool((out.view(torch.int32) == POISON).all()), 'the refused call wrote to its output'


# ---- maxpool2x2_kernel per op -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', [(3, 3), (5, 5), (2, 2), (4, 6), (7, 4), (8, 8), (9, 10)])
def test_maxpool2x2_bit_exact(hip_lib, hw):
    """Odd and even sizes (3 x 3 -> 1 x 1, 5 x 5 -> 2 x 2: the floor drops a row and a column), a channel sub-range of a wider
    row; the rest of the row and the bands hold +inf (a max-pool would absorb a NaN), so a read outside the range shows."""
    from workoutdetector_amd.engine import maxpool2x2_nhwc
    h, w = hw
    n, cw, c0, c = 3, 24, 8, 12
    g = torch.Generator().manual_seed(h * 16 + w)
    x = torch.full((n, h, w, cw), float('inf'))
    x[..., c0:c0 + c] = torch.randn(n, h, w, c, generator=g)
    gx = guarded(x.cuda(), fill=float('inf'), name='x')
    want = F.max_pool2d(x[..., c0:c0 + c].permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).contiguous()
    assert want.shape == (n, h // 2, w // 2, c)
    for arm in ('c0', 'slice'):        # the channel range as arguments, and as a slice of the tensor
        out = guarded_out(want.shape, name='y')
        got = maxpool2x2_nhwc(gx, c0, c, out=out) if arm == 'c0' else maxpool2x2_nhwc(gx[..., c0:c0 + c], out=out)
        assert got is out
        torch.cuda.synchronize()
        check(out, gx)
        assert torch.equal(out.cpu(), want), (hw, arm)


# ---- the engine against the float64 torch model --------------------------------------------------------------------------
R50, WRN = 'resnet50', 'wide_resnet50_2'
# (base_model, shift_place, T, is_shift, size, mode): 64 -> layer2 8 x 8 -> 4 x 4, layer3 4 x 4 -> 2 x 2; 80 -> 10 x 10 -> 5 x 5 and
# 5 x 5 -> 2 x 2 (the floor drops a row and a column); 48 -> layer3 3 x 3 -> 1 x 1, N_k = T
CASES = [(R50, 'blockres', 8, True, 64, 'avg'), (R50, 'blockres', 8, True, 80, 'avg'), (R50, 'blockres', 8, True, 48, 'avg'),
         (R50, 'blockres', 3, True, 64, 'avg'), (R50, 'blockres', 8, False, 64, 'avg'), (R50, 'block', 8, True, 64, 'avg'),
         (WRN, 'blockres', 8, True, 64, 'avg'), (R50, 'blockres', 8, True, 64, 'identity'), (R50, 'blockres', 8, True, 64, 'features')]
# the non-square frames of tests/_geometry_cases.py (size = (h, w)): square frames hide an H/W exchange in the host plumbing
CASES += [(c['base_model'], 'blockres', c['T'], True, (c['h'], c['w']), 'avg') for c in G.NON_LOCAL]
CASES += [(R50, 'blockres', 8, True, (80, 48), 'identity'), (R50, 'blockres', 8, True, (80, 48), 'features')]
TAP_MAPS = {'layer2.0': ('layer2', 512), 'layer2.0.block': ('layer2', 512), 'layer2.2.nl.y': ('layer2', 256), 'layer3.4': ('layer3', 1024)}


def _hw(size):
    return (size, size) if isinstance(size, int) else tuple(size)


def _maps(size):
    """The stage maps of a frame: the table's record for a frame of the table, the restated arithmetic for the square ones."""
    h, w = _hw(size)
    return G.maps_of('non_local', h, w) if (h, w) in G.frames_of('non_local') else G.tsm_maps(h, w)


def _frame_id(v):
    return '%dx%d' % v if isinstance(v, tuple) else None


def _sd(base_model=R50, place='blockres', seed=0):
    from workoutdetector_amd.weights import make_state_dict
    return make_state_dict(seed, 12, base_model, place, non_local=True)


@functools.lru_cache(maxsize=None)
def _reference(base_model, place, T, is_shift, size):
    """The float64 torch model's outputs for the seeded weights and this configuration's two clips: computed once."""
    h, w = _hw(size)
    x = clip_input(100 + size + T if isinstance(size, int) else 100 + h + w + T, 2, T, h, w)
    net = torch_tsm_nl(base_model, place, 12, T, is_shift, sd=_sd(base_model, place))
    logits, seg, pooled, taps, _sharp = run_with_taps(net, x)
    return x, logits, seg, pooled, taps


def _engine(base_model=R50, place='blockres', T=8, is_shift=True, size=64, consensus='avg', max_clips=2, sd=None, non_local=True):
    from workoutdetector_amd.engine import TsmEngine
    h, w = _hw(size)
    return TsmEngine(num_class=12, num_segments=T, height=h, width=w, is_shift=is_shift, max_clips=max_clips,
                     state_dict=sd if sd is not None else _sd(base_model, place), base_model=base_model, shift_place=place,
                     consensus_type=consensus, non_local=non_local)


@pytest.mark.parametrize('base_model,place,T,is_shift,size,mode', CASES, ids=_frame_id)
def test_engine_against_float64_torch(hip_lib, base_model, place, T, is_shift, size, mode):
    """Tap shapes are held to the case table's maps (tests/_geometry_cases.py), not to what the engine or the reference says."""
    x, logits, seg, pooled, taps = _reference(base_model, place, T, is_shift, size)
    eng = _engine(base_model, place, T, is_shift, size, 'identity' if mode == 'identity' else 'avg')
    what = f'{base_model} {place} T{T} shift {is_shift} {"%dx%d" % _hw(size)} {mode}'
    maps = _maps(size)
    if mode == 'features':
        got = eng.forward_features(x)
        assert got.shape == (2 * T, 2048)
        assert_close(got, pooled, rtol=1e-3, atol_scale=1e-5, what=what + ' features')
    else:
        got = eng.run(None, {'input': x})[0]
        assert got.shape == ((2, T, 12) if mode == 'identity' else (2, 12))
        assert_close(got, seg if mode == 'identity' else logits, rtol=1e-3, atol_scale=1e-5, what=what + ' logits')
    for stage in TAPS:
        tap = eng.forward_tap(x, stage)
        assert tap.shape == (2 * T, *maps[TAP_MAPS[stage][0]], TAP_MAPS[stage][1]), (stage, tap.shape)
        assert_close(tap, taps[stage], rtol=1e-3, atol_scale=3e-5, what=f'{what} {stage}')
    eng.close()


def test_three_clips_through_two_slots_equal_the_single_runs(hip_lib):
    x = clip_input(31, 3, 8, 64, 64)
    eng = _engine()
    all3 = eng.run(None, {'input': x})[0]
    for c in range(3):
        assert np.array_equal(eng.run(None, {'input': x[c:c + 1]})[0][0], all3[c]), c
    eng.close()


def test_three_clips_through_two_slots_on_a_non_square_frame(hip_lib):
    x = clip_input(31, 3, 8, 48, 80)
    eng = _engine(size=(48, 80))
    all3 = eng.run(None, {'input': x})[0]
    assert all3.shape == (3, 12)
    for c in range(3):
        assert np.array_equal(eng.run(None, {'input': x[c:c + 1]})[0][0], all3[c]), c
    eng.close()
    assert not np.array_equal(all3[0], all3[1]) and not np.array_equal(all3[1], all3[2])


def test_tuned_and_untuned_on_both_orientations_share_one_cache_file(hip_lib, monkeypatch, tmp_path):
    """48 x 80 and 80 x 48 tune into ONE TSM_TUNE_CACHE file: two lines whose signatures differ in the frame alone, each engine's
    tuned logits bitwise its untuned ones (a line read back for the other orientation would carry tiles timed on other maps)."""
    path = tmp_path / 'tune.txt'
    monkeypatch.setenv('TSM_TUNE_CACHE', str(path))
    tuned, xs = {}, {}
    for hw in ((48, 80), (80, 48)):
        xs[hw] = clip_input(32 + hw[0], 2, 8, *hw)
        eng = _engine(size=hw)
        eng.warmup([2])
        tuned[hw] = eng.run(None, {'input': xs[hw]})[0]
        tiles = eng.conv_tiles(2)
        for li, b in ((2, 0), (2, 2), (3, 0), (3, 2), (3, 4)):
            assert f'layer{li}.{b}.nl.qkv' in tiles and f'layer{li}.{b}.nl.W' in tiles, (hw, li, b)
        assert len(tiles) == 53 + 10
        eng.close()
    lines = path.read_text().splitlines()
    assert len(lines) == 2, lines
    sigs = [ln.split('|')[0] for ln in lines]
    assert ' 48x80 ' in sigs[0] and ' 80x48 ' in sigs[1] and sigs[0] != sigs[1], sigs
    assert sigs[0].replace(' 48x80 ', ' 80x48 ') == sigs[1] and all(s.endswith(' nl') for s in sigs)
    # a second engine per orientation reads its own line: nothing is appended, the bits stay
    for hw in ((48, 80), (80, 48)):
        eng = _engine(size=hw)
        assert np.array_equal(eng.run(None, {'input': xs[hw]})[0], tuned[hw]), hw
        eng.close()
    assert path.read_text().splitlines() == lines
    monkeypatch.setenv('TSM_AUTOTUNE', '0')
    for hw in ((48, 80), (80, 48)):
        eng = _engine(size=hw)
        assert np.array_equal(eng.run(None, {'input': xs[hw]})[0], tuned[hw]), hw
        eng.close()


def test_tuned_and_untuned_forwards_are_bitwise_equal(hip_lib, monkeypatch, tmp_path):
    monkeypatch.setenv('TSM_TUNE_CACHE', str(tmp_path / 'tune.txt'))
    x = clip_input(32, 2, 8, 80, 80)
    eng = _engine(size=80)
    eng.warmup([2])
    tuned = eng.run(None, {'input': x})[0]
    tiles = eng.conv_tiles(2)
    assert 'layer2.0.nl.qkv' in tiles and 'layer3.4.nl.W' in tiles and len(tiles) == 53 + 10
    eng.close()
    line = (tmp_path / 'tune.txt').read_text().splitlines()
    assert len(line) == 1 and line[0].split('|')[0].endswith(' nl'), line
    monkeypatch.setenv('TSM_AUTOTUNE', '0')
    eng = _engine(size=80)
    plain = eng.run(None, {'input': x})[0]
    eng.close()
    assert np.array_equal(tuned, plain)


def test_poisoned_engine_gives_the_same_bits(hip_lib, monkeypatch):
    """TSM_POISON=1: every buffer between poisoned bands, the workspace poisoned before every forward -- the new launches
    rely on nothing they did not write and store nothing outside their buffers."""
    x = clip_input(33, 2, 8, 80, 80)
    eng = _engine(size=80)
    want = eng.run(None, {'input': x})[0]
    want_y = eng.forward_tap(x, 'layer3.2.nl.y')
    eng.close()
    monkeypatch.setenv('TSM_POISON', '1')
    eng = _engine(size=80)
    assert np.array_equal(eng.run(None, {'input': x})[0], want)
    assert np.array_equal(eng.run(None, {'input': x[:1]})[0], want[:1])
    assert np.array_equal(eng.forward_tap(x, 'layer3.2.nl.y'), want_y)
    eng.close()


@pytest.mark.parametrize('hw', [(48, 80), (80, 48)], ids=_frame_id)
def test_poisoned_engine_gives_the_same_bits_on_a_non_square_frame(hip_lib, monkeypatch, hw):
    """The check that catches a buffer sized with the wrong side: under TSM_POISON=1 a launch that writes or reads H x W words
    where W x H (or W / 2 x H / 2 keys) were allocated breaks a band or reads poison."""
    x = clip_input(33 + hw[1], 2, 8, *hw)
    eng = _engine(size=hw)
    want = eng.run(None, {'input': x})[0]
    want_y = eng.forward_tap(x, 'layer3.2.nl.y')
    eng.close()
    assert want_y.shape == (16, *G.maps_of('non_local', *hw)['layer3'], 512)
    monkeypatch.setenv('TSM_POISON', '1')
    eng = _engine(size=hw)
    assert np.array_equal(eng.run(None, {'input': x})[0], want)
    assert np.array_equal(eng.run(None, {'input': x[:1]})[0], want[:1])
    assert np.array_equal(eng.forward_tap(x, 'layer3.2.nl.y'), want_y)
    eng.close()


def test_launch_counts_by_width_on_a_non_square_frame(hip_lib):
    from workoutdetector_amd.engine import launch_trace
    x = clip_input(34, 1, 8, 80, 48)
    eng = _engine(size=(80, 48), max_clips=1)
    eng.run(None, {'input': x})
    with launch_trace() as tr:
        eng.run(None, {'input': x})
    eng.close()
    assert tr.count('nonlocal_attn_kernel<256>') == 2 and tr.count('nonlocal_attn_kernel<512>') == 3, tr.kernels
    assert tr.count('nonlocal_attn_kernel') == 5 and tr.count('maxpool2x2_kernel') == 5


def test_launch_trace_and_timing_slots(hip_lib):
    from workoutdetector_amd.engine import launch_trace
    x = clip_input(34, 1, 8, 64, 64)
    eng = _engine(max_clips=1)
    eng.run(None, {'input': x})
    with launch_trace() as tr:
        eng.run(None, {'input': x})
    assert tr.count('nonlocal_attn_kernel<256>') == 2 and tr.count('nonlocal_attn_kernel<512>') == 3, tr.kernels
    assert tr.count('nonlocal_attn_kernel') == 5 and tr.count('maxpool2x2_kernel') == 5
    eng.set_layer_timing(1)
    eng.run(None, {'input': x})
    times = eng.layer_times_ms(0)
    for li, b in ((2, 0), (2, 2), (3, 0), (3, 2), (3, 4)):
        for part in ('qkv', 'pool', 'attn', 'W'):
            assert times[f'layer{li}.{b}.nl.{part}'] > 0, (li, b, part, times)
    assert 'layer2.1.nl.attn' not in times
    eng.close()


def test_zero_W_batchnorm_is_the_plain_network(hip_lib):
    """nl.W.1.weight = nl.W.1.bias = 0: z = 0 + x, so the logits equal the plain engine's on the same base weights bit for bit --
    the residual path adds x and nothing else.  The plain engine launches none of the new kernels; the un-wrapped key spelling
    (without ``.block``) loads the same network."""
    from workoutdetector_amd.engine import launch_trace
    from workoutdetector_amd.weights import make_state_dict
    x = clip_input(35, 2, 8, 64, 64)
    plain = _engine(sd=make_state_dict(0, 12), non_local=False)
    with launch_trace() as tr:
        want = plain.run(None, {'input': x})[0]
    assert not tr.ran('nonlocal_attn_kernel') and not tr.ran('maxpool2x2_kernel'), tr.kernels
    assert not any('.nl.' in k for k in plain.launch_names())
    plain.close()
    sd = _sd()
    full = _engine(sd=sd)
    moved = full.run(None, {'input': x})[0]
    full.close()
    assert not np.array_equal(moved, want), 'the seeded non-local blocks must change the logits'
    zero = {k: (np.zeros_like(v) if k.endswith(('nl.W.1.weight', 'nl.W.1.bias')) else v) for k, v in sd.items()}
    eng = _engine(sd=zero)
    assert np.array_equal(eng.run(None, {'input': x})[0], want)
    eng.close()
    unwrapped = {k.replace('.block.', '.'): v for k, v in sd.items()}
    assert len(unwrapped) == len(sd) and not any('.block.' in k for k in unwrapped)
    eng = _engine(sd=unwrapped)
    assert np.array_equal(eng.run(None, {'input': x})[0], moved)
    eng.close()


def test_set_non_local_contract(hip_lib):
    from workoutdetector_amd import _lib
    from workoutdetector_amd.engine import TsmEngine, create_model
    lib = hip_lib

    def engine(dtype=_lib.DTYPE_F32):
        cfg = _lib.TsmConfig(C.sizeof(_lib.TsmConfig), 12, 8, 64, 64, 8, 1, 1, 0, dtype)
        h = C.c_void_p()
        _lib.check(lib.tsm_create(C.byref(cfg), C.byref(h)))
        return h
    for dtype in (_lib.DTYPE_BF16, _lib.DTYPE_BF16X3):
        h = engine(dtype)
        assert lib.tsm_set_non_local(h, 1) == -7 and lib.tsm_set_non_local(h, 0) == 0
        lib.tsm_destroy(h)
    for depth in (18, 34):                                   # either order
        h = engine()
        assert lib.tsm_set_backbone(h, depth) == 0 and lib.tsm_set_non_local(h, 1) == -7
        lib.tsm_destroy(h)
        h = engine()
        assert lib.tsm_set_non_local(h, 1) == 0 and lib.tsm_set_backbone(h, depth) == -7 and lib.tsm_set_backbone(h, 50) == 0
        lib.tsm_destroy(h)
    h = engine()
    assert lib.tsm_set_non_local(h, 2) == -7 and lib.tsm_set_non_local(h, 1) == 0
    assert lib.tsm_set_bottleneck_width(h, 128) == 0 and lib.tsm_set_shift_place(h, 1) == 0
    arr = np.ones(256 * 512, np.float32)
    shape = (C.c_int64 * 5)(256, 512, 1, 1, 1)
    assert lib.tsm_set_tensor(h, b'base_model.layer2.0.nl.theta.weight', arr.ctypes.data, shape, 5) == 0
    assert lib.tsm_set_tensor(h, b'base_model.layer2.1.nl.theta.weight', arr.ctypes.data, shape, 5) == -1      # not a wrapped block
    assert lib.tsm_set_non_local(h, 0) == -1 and lib.tsm_set_non_local(h, 1) == -1                             # after the first tsm_set_tensor
    lib.tsm_destroy(h)
    h = engine()                                             # a plain engine does not know the keys
    assert lib.tsm_set_tensor(h, b'base_model.layer2.0.nl.theta.weight', arr.ctypes.data, shape, 5) == -1
    lib.tsm_destroy(h)
    for dtype in ('bf16', 'bf16x3'):
        with pytest.raises(NotImplementedError):
            create_model(non_local=True, dtype=dtype, height=64, width=64)
        with pytest.raises(NotImplementedError):
            TsmEngine(non_local=True, dtype=dtype, height=64, width=64)
    with pytest.raises(_lib.TsmError, match='TSM_ERR_MISSING_TENSOR'):      # a plain checkpoint is not run as the non-local network
        from workoutdetector_amd.weights import make_state_dict
        TsmEngine(num_class=12, height=64, width=64, max_clips=1, non_local=True, state_dict=make_state_dict(0, 12))
