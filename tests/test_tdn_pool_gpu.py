"""A TDN engine's input as a pool of transformed frames (include/tsm_hip.h: TSM_LAYOUT_TDN_POOL; ``TsmEngine.forward_pool``;
csrc/tsm_tdn.hip: tdn_front_pool_kernel) and the pipelines on it (workoutdetector_amd/tdn_pipeline.py), on the GPU.

The pool kernel spells the plain front end's arithmetic the same way, so everything that compares the pool forward with the NTCHW
forward of the gathered planes is bit for bit.  Engines: depths (1, 1, 1, 2); 64 x 64 (2 x 2 front-end tiles: a halo across tiles
and the map border) and 96 x 96 (3 x 3: an interior tile with a halo on every side); and the non-square frames of
tests/_geometry_cases.py, 64 x 96, 96 x 64 and 160 x 96 -- where H = W the two kernels cannot differ in a row pitch.  Pools, tables and outputs are tests/_guard.py
tensors: a stray read reads poison, a stray store breaks a band."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _geometry_cases as G
from tests._guard import check, guarded, guarded_out
from tests._tdn_cases import LOGITS_BAR, NUM_CLASS, bits as _bits, engine as _cases_engine, network as _model
from tests._util import assert_close

pytestmark = pytest.mark.gpu

D64 = (1, 1, 1, 2)
TAPS = ('diff.conv1_5', 'diff.stem', 'stem')
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def _hw(size):
    return (size, size) if isinstance(size, int) else tuple(size)


def _frame_id(v):
    return '%dx%d' % v if isinstance(v, tuple) else str(v)


def _engine(size, T, max_clips=3, **kw):
    """``size``: the side of a square frame, or (h, w)."""
    h, w = _hw(size)
    return _cases_engine(h, w, T, D64, _model(D64, T)[1], max_clips=max_clips, **kw)


def _pool(n_frames, size, seed=7):
    h, w = _hw(size)
    x = np.random.default_rng([seed, n_frames, h] + ([] if isinstance(size, int) else [w])).standard_normal((n_frames, 3, h, w)).astype(np.float32)
    return guarded(torch.from_numpy(x).cuda(), name='pool')


def _table(n, T, n_frames, seed=11):
    """Random pool frame numbers with repeats: every segment also repeats one of its own frames."""
    t = np.random.default_rng([seed, n, T]).integers(0, n_frames, (n, T, 5)).astype(np.int32)
    t[:, :, 3] = t[:, :, 1]
    return t


def _gathered(pool, table):
    """[n, T, 15, H, W]: the planes the table names, an entry outside the pool as planes of zeros."""
    n, T, _ = table.shape
    ext = torch.cat([pool, torch.zeros_like(pool[:1])])
    t = torch.from_numpy(np.where((table >= 0) & (table < pool.shape[0]), table, pool.shape[0]).astype(np.int64)).cuda()
    return ext[t.reshape(-1)].reshape(n, T, 15, pool.shape[2], pool.shape[3]).contiguous()


def _same(a, b):
    a, b = (t.cpu().numpy() if hasattr(t, 'cpu') else t for t in (a, b))
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


TAP_MAPS = {'diff.conv1_5': 'conv1_5', 'diff.stem': 'ring_d', 'stem': 'ring_a'}          # (tests/_geometry_cases.py: tdn_maps)


def _assert_pool_equals_ntchw(eng, pool, table_np, taps=TAPS, maps=None):
    """``maps``: the case table's record of the frame -- the taps' shapes are then held to it."""
    n, T, _ = table_np.shape
    table = guarded(torch.from_numpy(table_np).cuda(), name='table')
    clips = _gathered(pool, table_np)
    out = guarded_out(eng._out_shape(n), name='logits')
    feats = guarded_out((n * T, eng.feature_dim), name='features')
    eng.forward_pool(pool, table, n_clips=n, out=out)
    eng.forward_features_pool(pool, table, n_clips=n, out=feats)
    torch.cuda.synchronize()
    check(out, feats, pool, table)
    want, want_feats = eng.forward_device(clips), eng.forward_features(clips)
    torch.cuda.synchronize()
    assert _same(out, want), 'logits'
    assert _same(feats, want_feats), 'features'
    assert float(want.abs().max()) > 0 and not _same(want[:1], eng.forward_device(torch.zeros_like(clips[:1])))
    for lo in range(0, n if taps else 0, eng.max_clips):
        hi = min(lo + eng.max_clips, n)
        for name in taps:
            got = eng.forward_tap_pool(pool, name, table[lo:hi], n_clips=hi - lo)
            torch.cuda.synchronize()
            assert _same(got, eng.forward_tap(clips[lo:hi].cpu().numpy(), name)), name
            if maps is not None:
                assert got.shape == ((hi - lo) * T, *maps[TAP_MAPS[name]], 64), (name, got.shape)
    check(pool, table)
    return out


# ---- 1. table mode against the NTCHW forward ------------------------------------------------------------------------------------
@pytest.mark.parametrize('h, T, n, max_clips, consensus', [(64, 2, 1, 1, 'avg'), (64, 8, 3, 3, 'avg'), (64, 8, 3, 3, 'identity'),
                                                          (96, 3, 3, 3, 'avg'), (64, 2, 10, 10, 'avg'), (64, 2, 5, 3, 'avg')] +
                         [((c['h'], c['w']), c['T'], c['clips'], c['clips'], 'avg') for c in G.TDN_POOL], ids=_frame_id)
def test_table_mode_is_the_ntchw_forward_of_the_gathered_planes(hip_lib, h, T, n, max_clips, consensus):
    """(64, 2, 10, 10): front-end chunks of 8 + 2 inside one call; (64, 2, 5, 3): calls of 3 + 2 clips, split by forward_pool.
    h = (rows, columns): the non-square frames of tests/_geometry_cases.py, 2 x 3, 3 x 2 and 5 x 3 front-end tiles -- the pool
    kernel's own copy of the plain front end's row pitch and tile walk, held to the plain kernel where H is not W."""
    eng = _engine(h, T, max_clips=max_clips, consensus=consensus)
    try:
        if max_clips == 10:
            assert eng.tdn_chunk_clips == 8
        maps = G.maps_of('tdn_pool', *h) if isinstance(h, tuple) else None
        out = _assert_pool_equals_ntchw(eng, _pool(11, h), _table(n, T, 11), maps=maps)
        assert tuple(out.shape) == ((n, T, NUM_CLASS) if consensus == 'identity' else (n, NUM_CLASS))
        if maps is not None:                                    # which kernel that was
            from workoutdetector_amd.engine import launch_trace
            with launch_trace() as tr:
                eng.forward_pool(_pool(11, h), torch.from_numpy(_table(n, T, 11)).cuda(), n_clips=n)
            assert tr.count('tdn_front_pool_kernel') == 1 and tr.count('tdn_front_kernel') == 0, tr.kernels
    finally:
        eng.close()


def test_non_square_pool_forward_against_float64(hip_lib, capsys):
    """96 x 64: the bitwise chain above anchored to the float64 network at this orientation too (tests._tdn_cases.reference's
    clips as the pool, the table naming each segment's five frames in place)."""
    h, w, T, n = 96, 64, 3, 2
    from tests._tdn_cases import clips_of, reference
    want, _taps = reference(h, w, D64, T, n)
    x = clips_of('plain', h, w, T, n)                                      # [n, T, 15, h, w]
    pool = guarded(torch.from_numpy(np.array(x).reshape(n * T * 5, 3, h, w)).cuda(), name='pool')
    table_np = np.arange(n * T * 5, dtype=np.int32).reshape(n, T, 5)
    eng = _engine((h, w), T, max_clips=n, consensus='identity')
    try:
        table = guarded(torch.from_numpy(table_np).cuda(), name='table')
        out = guarded_out(eng._out_shape(n), name='logits')
        eng.forward_pool(pool, table, n_clips=n, out=out)
        torch.cuda.synchronize()
        check(out, pool, table)
        err = assert_close(out.cpu().numpy(), want, what='pool forward 96x64', **LOGITS_BAR)
        with capsys.disabled():
            print(f'\n[tdn pool 96x64 T{T}] logits max|err|/scale {err:.2g}')
    finally:
        eng.close()


# ---- 2. the kernel is total in the table ----------------------------------------------------------------------------------------
def test_table_entries_outside_the_pool_are_planes_of_zeros(hip_lib):
    _entries_outside_the_pool(64)


def test_table_entries_outside_the_pool_on_a_non_square_frame(hip_lib):
    _entries_outside_the_pool((96, 64))


def _entries_outside_the_pool(h):
    T, n = 3, 3
    table = _table(n, T, 11)
    table[0, 0, 0], table[0, 1, 2], table[1, 0, 4], table[1, 2, 1], table[2, 1, 3] = -1, 11, I32_MIN, I32_MAX, 12
    table[2, 2] = (-1, 11, I32_MIN, I32_MAX, -2)            # a segment without any frame: an input of zeros
    eng = _engine(h, T)
    try:
        _assert_pool_equals_ntchw(eng, _pool(11, h), table)
    finally:
        eng.close()


# ---- 3. window mode against table mode of tdn_clip_indices ----------------------------------------------------------------------
# (total, lo, hi, first_source_frame, n_frames, pad_frame)
WINDOWS = {'clip 0: frames -2 and -1 clamp to 0': (45, 0, 3, 0, 34, 33),
           'mid-video, first_source_frame > 0': (45, 2, 4, 14, 28, 27),
           'a centre on the last frame, then past the end': (45, 4, 6, 30, 16, 15),
           'a centre on the last frame but one': (46, 4, 6, 30, 17, 16),
           'one frame': (1, 0, 1, 0, 2, 1),
           'no pad frame: zero planes': (45, 4, 6, 30, 15, -1),
           'frames in front of the pool take the pad': (45, 3, 6, 30, 16, 15)}


@pytest.mark.parametrize('case', list(WINDOWS), ids=lambda v: v.replace(' ', '_'))
def test_window_mode_is_table_mode_of_the_numpy_rule(hip_lib, case):
    _window_mode_is_table_mode(case, 64)


@pytest.mark.parametrize('case', ['clip 0: frames -2 and -1 clamp to 0', 'a centre on the last frame, then past the end'],
                         ids=lambda v: v.replace(' ', '_'))
def test_window_mode_on_a_non_square_frame(hip_lib, case):
    _window_mode_is_table_mode(case, (64, 96))


def _window_mode_is_table_mode(case, h):
    from workoutdetector_amd.tdn_pipeline import tdn_clip_indices
    total, lo, hi, first, n_frames, pad = WINDOWS[case]
    T, n = 8, hi - lo
    table_np = tdn_clip_indices(total, lo, hi, T, 8, 2, first_source_frame=first, pad=pad, n_frames=n_frames)
    if case.startswith('a centre on the last frame, then'):
        assert table_np[1, 2].tolist() == [12, 13, 14, 14, 14] and (table_np[1, 3:] == 15).all()
    if case.startswith('clip 0'):
        assert table_np[0, 0].tolist() == [0, 0, 0, 1, 2]
    pool = _pool(n_frames, h)
    window = dict(first_source_frame=first, total_frames=total, first_clip=lo, clip_step=8, clip_stride=2, pad_frame=pad)
    eng = _engine(h, T)
    try:
        table = guarded(torch.from_numpy(table_np).cuda(), name='table')
        want = eng.forward_pool(pool, table, n_clips=n)
        want_feats = eng.forward_features_pool(pool, table, n_clips=n)
        out = guarded_out(eng._out_shape(n), name='logits')
        eng.forward_pool(pool, window=window, n_clips=n, out=out)
        feats = eng.forward_features_pool(pool, window=window, n_clips=n)
        tap = eng.forward_tap_pool(pool, 'diff.conv1_5', window=window, n_clips=n)
        tap_want = eng.forward_tap_pool(pool, 'diff.conv1_5', table, n_clips=n)
        torch.cuda.synchronize()
        check(out, pool, table)
        assert _same(out, want) and _same(feats, want_feats) and _same(tap, tap_want)
        assert _same(want, eng.forward_device(_gathered(pool, table_np)))          # (and table mode is the NTCHW forward)
    finally:
        eng.close()


def test_window_mode_across_chunks_and_calls(hip_lib):
    """10 clips of T = 2 through an engine of 10 (front-end chunks of 8 + 2: the first clip advances by the chunk) and through an
    engine of 3 (calls of 3 + 3 + 3 + 1: forward_pool advances it by the call)."""
    from workoutdetector_amd.tdn_pipeline import tdn_clip_indices
    total, h, T, n = 73, 64, 2, 10
    table_np = tdn_clip_indices(total, 0, n, T, 8, 2, first_source_frame=0, pad=total, n_frames=total + 1)
    assert (table_np[9, 1] == total).all() and table_np[9, 0].tolist() == [70, 71, 72, 72, 72]
    pool = _pool(total + 1, h)
    window = dict(first_source_frame=0, total_frames=total, first_clip=0, clip_step=8, clip_stride=2, pad_frame=total)
    outs = []
    for max_clips in (10, 3):
        eng = _engine(h, T, max_clips=max_clips)
        try:
            want = eng.forward_pool(pool, torch.from_numpy(table_np).cuda(), n_clips=n)
            got = eng.forward_pool(pool, window=window, n_clips=n)
            torch.cuda.synchronize()
            assert _same(got, want)
            outs.append(got.cpu())
        finally:
            eng.close()
    assert _same(outs[0], outs[1])          # a clip's result depends neither on the chunking nor on the call it came in


# ---- 4. the launch trace ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n, max_clips, chunks', [(2, 2, 1), (10, 10, 2)])
def test_one_pool_kernel_per_chunk_and_nothing_else_changes(hip_lib, n, max_clips, chunks):
    from workoutdetector_amd.engine import launch_trace
    h, T = 64, 2
    pool, table_np = _pool(11, h), _table(n, T, 11)
    table = torch.from_numpy(table_np).cuda()
    window = dict(first_source_frame=0, total_frames=11, first_clip=0, clip_step=1, clip_stride=1, pad_frame=-1)
    eng = _engine(h, T, max_clips=max_clips)
    try:
        clips = _gathered(pool, table_np)
        with launch_trace() as plain:
            eng.forward_device(clips)
        with launch_trace() as by_table:
            eng.forward_pool(pool, table, n_clips=n)
        with launch_trace() as by_window:
            eng.forward_pool(pool, window=window, n_clips=n)
        names = eng.launch_names()
        eng.set_layer_timing(1)
        eng.forward_pool(pool, table, n_clips=n)
        torch.cuda.synchronize()
        times = eng.layer_times_ms(0)
    finally:
        eng.close()
    assert plain.count('tdn_front_kernel') == chunks and plain.count('tdn_front_pool_kernel') == 0
    for tr in (by_table, by_window):
        assert tr.count('tdn_front_pool_kernel') == chunks and tr.count('tdn_front_kernel') == 0, tr.kernels
        assert not [k for k in tr.kernels if 'preprocess' in k or 'gather' in k or 'pack' in k], tr.kernels
        assert [k.replace('tdn_front_pool_kernel', 'tdn_front_kernel') for k in tr.kernels] == plain.kernels
    # the same timing slots: diff.front holds the pool kernel
    assert list(times) == names
    for i in range((max_clips + 7) // 8):
        assert (times[f'diff.front.{i}'] > 0) == (i < chunks) and (times[f'diff.conv1_5.{i}'] > 0) == (i < chunks), times


# ---- 5. capture and replay --------------------------------------------------------------------------------------------------------
def test_forward_pool_captured_on_a_side_stream_reads_the_table_at_replay(hip_lib):
    """Sets A and B share the pool and differ in the TABLE alone: the replay on B after the capture on A gives B's eager logits,
    so the table is read on the device when the kernel runs and no frame number was baked into the graph."""
    from tests._capture import captured
    h, T, n = 64, 2, 2
    frames = [np.random.default_rng([47, k]).standard_normal((11, 3, h, h)).astype(np.float32) for k in range(2)]
    sets = [[torch.from_numpy(frames[0]), torch.from_numpy(_table(n, T, 11, seed=1))],
            [torch.from_numpy(frames[0]), torch.from_numpy(_table(n, T, 11, seed=2))],
            [torch.from_numpy(frames[1]), torch.from_numpy(_table(n, T, 11, seed=3))]]
    eng = _engine(h, T, max_clips=n, autotune=True)
    try:
        pool = guarded(torch.zeros(11, 3, h, h).cuda(), name='pool')
        table = guarded(torch.zeros(n, T, 5, dtype=torch.int32).cuda(), name='table')
        out = guarded_out(eng._out_shape(n), name='logits')
        eng.warmup([n])
        tr = captured(lambda: eng.forward_pool(pool, table, n_clips=n, out=out), [pool, table], lambda k: sets[k], [out], engine=eng)
        want_b = eng.forward_device(_gathered(sets[1][0].cuda(), sets[1][1].numpy()))
        torch.cuda.synchronize()
    finally:
        eng.close()
    assert tr.count('tdn_front_pool_kernel') == 1 and tr.count('tdn_front_kernel') == 0
    assert _same(tr.refs['B'][0], want_b) and not _same(tr.refs['A'][0], tr.refs['B'][0])


def test_window_mode_captured_on_a_side_stream(hip_lib):
    from tests._capture import captured
    h, T, n = 64, 2, 2
    sets = [[torch.from_numpy(np.random.default_rng([53, k]).standard_normal((20, 3, h, h)).astype(np.float32))] for k in range(3)]
    window = dict(first_source_frame=2, total_frames=19, first_clip=1, clip_step=8, clip_stride=2, pad_frame=19)
    eng = _engine(h, T, max_clips=n, autotune=True)
    try:
        pool = guarded(torch.zeros(20, 3, h, h).cuda(), name='pool')
        out = guarded_out(eng._out_shape(n), name='logits')
        eng.warmup([n])
        tr = captured(lambda: eng.forward_pool(pool, window=window, n_clips=n, out=out), [pool], lambda k: sets[k], [out], engine=eng)
    finally:
        eng.close()
    assert tr.count('tdn_front_pool_kernel') == 1


# ---- 6. poison ----------------------------------------------------------------------------------------------------------------------
def test_the_whole_engine_under_poison(hip_lib):
    _whole_engine_under_poison(96)


def test_the_whole_engine_under_poison_on_a_non_square_frame(hip_lib):
    _whole_engine_under_poison((96, 64))


def _whole_engine_under_poison(h):
    T, n = 3, 2
    pool, table_np = _pool(11, h), _table(n, T, 11)
    table_np[1, 1, 4] = -1
    table = torch.from_numpy(table_np).cuda()
    window = dict(first_source_frame=0, total_frames=10, first_clip=0, clip_step=8, clip_stride=2, pad_frame=10)
    plain, hostile = _engine(h, T), _engine(h, T, poison=True)
    try:
        for kw in (dict(index=table), dict(window=window)):
            assert _same(plain.forward_pool(pool, n_clips=n, **kw), hostile.forward_pool(pool, n_clips=n, **kw))
            one = dict(index=table[:1]) if 'index' in kw else kw
            assert _same(plain.forward_pool(pool, n_clips=1, **one), hostile.forward_pool(pool, n_clips=1, **one))
            assert _same(plain.forward_features_pool(pool, n_clips=n, **kw), hostile.forward_features_pool(pool, n_clips=n, **kw))
            for name in ('diff.conv1_5', 'stem', 'fuse2', 'layer4.1'):
                assert _same(plain.forward_tap_pool(pool, name, n_clips=n, **kw), hostile.forward_tap_pool(pool, name, n_clips=n, **kw)), name
        torch.cuda.synchronize()
        check(pool)
    finally:
        plain.close()
        hostile.close()


# ---- 7. the error contract --------------------------------------------------------------------------------------------------------
def test_the_error_contract_launches_nothing(hip_lib, sd0):
    from workoutdetector_amd import _lib
    from workoutdetector_amd.engine import TsmEngine, launch_trace
    lib = hip_lib
    h, T = 64, 2
    pool = _pool(11, h)
    table = torch.from_numpy(_table(1, T, 11)).cuda()
    out = guarded_out((1, NUM_CLASS), name='logits')
    feats = guarded_out((T, 2048), name='features')

    def desc(**kw):
        d = _lib.TsmTdnPool(struct_size=C.sizeof(_lib.TsmTdnPool), mode=0, frames=pool.data_ptr(), n_frames=11, index=table.data_ptr())
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    win = dict(mode=1, index=None, total_frames=11, clip_step=8, clip_stride=2, pad_frame=-1)
    invalid = {'struct_size': desc(struct_size=64), 'frames is NULL': desc(frames=None), '8-byte aligned': desc(frames=pool.data_ptr() + 4),
               'n_frames': desc(n_frames=0), 'n_frames ': desc(n_frames=-3), 'mode': desc(mode=2), 'mode ': desc(mode=-1),
               'needs index': desc(index=None), 'clip_step': desc(**dict(win, clip_step=0)), 'clip_step ': desc(**dict(win, clip_step=-8)),
               'clip_stride': desc(**dict(win, clip_stride=0)), 'total_frames': desc(**dict(win, total_frames=0))}
    eng = _engine(h, T, max_clips=1)
    other = TsmEngine(num_class=12, num_segments=T, height=h, width=h, max_clips=1, state_dict=sd0)
    shape = (C.c_int64 * 4)()
    try:
        def calls(e, d, memkind=_lib.MEM_DEVICE):
            p = C.addressof(d)
            return (lib.tsm_forward(e._h, p, memkind, _lib.LAYOUT_TDN_POOL, 1, out.data_ptr(), None),
                    lib.tsm_forward_features(e._h, p, memkind, _lib.LAYOUT_TDN_POOL, 1, feats.data_ptr(), 0, None),
                    lib.tsm_forward_tap(e._h, p, memkind, _lib.LAYOUT_TDN_POOL, 1, b'stem', feats.data_ptr(), feats.numel(), shape, None))
        with launch_trace() as tr:
            for what, d in invalid.items():
                assert calls(eng, d) == (-1, -1, -1), what
                assert what.strip().split()[0] in lib.tsm_last_error(eng._h).decode(), (what, lib.tsm_last_error(eng._h))
            assert calls(eng, desc(), _lib.MEM_HOST) == (-1, -1, -1) and 'TSM_MEM_DEVICE' in lib.tsm_last_error(eng._h).decode()
            assert calls(other, desc()) == (-7, -7, -7) and 'TDN engine' in lib.tsm_last_error(other._h).decode()
            assert lib.tsm_forward(eng._h, None, _lib.MEM_DEVICE, _lib.LAYOUT_TDN_POOL, 1, out.data_ptr(), None) == -1
            # 5 and 9 stay invalid layouts; the frame transforms keep refusing code 16 as an out_layout
            for layout in (5, 9, 15, 17):
                assert lib.tsm_forward(eng._h, C.addressof(desc()), _lib.MEM_DEVICE, layout, 1, out.data_ptr(), None) == -1
            u8 = torch.zeros(1, 80, 100, 3, dtype=torch.uint8).cuda()
            assert lib.tsm_preprocess(u8.data_ptr(), _lib.PIXEL_U8, 1, 80, 100, feats.data_ptr(), _lib.LAYOUT_TDN_POOL, 73, 64, 0, None) == -1
        assert tr.kernels == [], tr.kernels
        torch.cuda.synchronize()
        # nothing was written; and the Python wrapper refuses what the C ABI cannot see
        assert bool((out.view(torch.int32) == 0x7FC07FC0).all()) and bool((feats.view(torch.int32) == 0x7FC07FC0).all())
        for bad in (dict(index=table, window=dict(win)), dict(), dict(index=table.long()), dict(index=table[:, :1]), dict(window=dict(first_clip=0))):
            with pytest.raises(ValueError):
                eng.forward_pool(pool, n_clips=1, **bad)
        with pytest.raises(ValueError):
            eng.forward_pool(pool[:, :, :32], table, n_clips=1)
        with pytest.raises(ValueError):
            eng.forward_pool(pool.cpu(), table, n_clips=1)
        with pytest.raises(ValueError, match='TDN engine'):
            other.forward_pool(pool, table, n_clips=1)
        # and the descriptor that is accepted runs
        assert calls(eng, desc())[0] == 0
        torch.cuda.synchronize()
        check(out, pool)
    finally:
        eng.close()
        other.close()


def test_a_transposed_pool_is_refused_before_any_launch(hip_lib):
    """[n, 3, W, H] frames to an H x W engine: as many words as the right pool, so the C ABI's bare pointer could not tell --
    the wrapper's shape check is the only one there is."""
    from workoutdetector_amd.engine import launch_trace
    h, w, T = 96, 64, 2
    pool = _pool(11, (h, w))
    turned = guarded(pool.transpose(2, 3).contiguous(), name='transposed pool')
    assert tuple(turned.shape) == (11, 3, w, h) and turned.numel() == pool.numel()
    table = torch.from_numpy(_table(1, T, 11)).cuda()
    window = dict(first_source_frame=0, total_frames=11, first_clip=0, clip_step=8, clip_stride=2, pad_frame=-1)
    eng = _engine((h, w), T, max_clips=1)
    try:
        out = guarded_out(eng._out_shape(1), name='logits')
        with launch_trace() as tr:
            for kw in (dict(index=table), dict(window=window)):
                with pytest.raises(ValueError, match=r'\[n_frames, 3, 96, 64\], got \(11, 3, 64, 96\)'):
                    eng.forward_pool(turned, n_clips=1, out=out, **kw)
                with pytest.raises(ValueError, match='3, 96, 64'):
                    eng.forward_features_pool(turned, n_clips=1, **kw)
                with pytest.raises(ValueError, match='3, 96, 64'):
                    eng.forward_tap_pool(turned, 'stem', n_clips=1, **kw)
        assert tr.kernels == [], tr.kernels
        torch.cuda.synchronize()
        assert bool((out.view(torch.int32) == 0x7FC07FC0).all()), 'the refused call wrote to its output'
        check(turned)
        eng.forward_pool(pool, table, n_clips=1, out=out)          # and the pool the right way round runs
        torch.cuda.synchronize()
        check(out, pool)
    finally:
        eng.close()


# ---- 8. the counting pipeline -------------------------------------------------------------------------------------------------------
def _video(total, hh, ww, seed=3):
    return torch.from_numpy(np.random.default_rng([seed, hh, ww]).integers(0, 256, (total, hh, ww, 3), dtype=np.uint8))


class _HostOnly:
    """The engine as a model WITHOUT a device path: what the pipelines' host path is for."""

    def __init__(self, eng):
        self.eng, self.num_class, self.num_segments, self.height, self.width = eng, eng.num_class, eng.num_segments, eng.height, eng.width

    def __call__(self, x):
        return self.eng(x.cpu())


@pytest.mark.parametrize('hh, ww, resize, scale_255', [(80, 100, 73, True), (40, 56, 73, True), (80, 100, 73, False)], ids=str)
def test_counting_pipeline_on_a_synthetic_video(hip_lib, monkeypatch, capsys, hh, ww, resize, scale_255):
    """45 frames, clips 0 .. 5 (the last one's segments 3 .. 7 are past the end): the pipeline's logits are the per-clip forwards of
    clips assembled by hand from preprocess_frames(packed=False), bit for bit -- whole, in batches and in staged pieces -- and within
    LOGITS_BAR of the float64 network on the torch transform of the same frames (scale_255: inputs of the size the network's
    weights were drawn for)."""
    from workoutdetector_amd import inference_count as ic, tdn_pipeline as tp
    from workoutdetector_amd.engine import launch_trace, preprocess_frames
    from workoutdetector_amd.transform import TestTransform
    total, h, T = 45, 64, 8
    video = _video(total, hh, ww)
    tf = TestTransform(resize, h, scale_255=scale_255)
    eng = _engine(h, T, max_clips=4)
    try:
        with launch_trace() as tr:
            got = tp.tdn_video_clip_logits(eng, video, tf)
        assert tuple(got.shape) == (6, NUM_CLASS)
        assert tr.count('preprocess') == 1 and tr.count('tdn_front_pool_kernel') == 2 and tr.count('tdn_front_kernel') == 0, tr.kernels
        assert not [k for k in tr.kernels if 'gather' in k or 'indexed' in k], tr.kernels
        staged = torch.cat([video, torch.zeros_like(video[:1])]).cuda()
        pool = preprocess_frames(staged, resize=resize, crop=h, scale_255=scale_255, packed=False)
        idx = tp.tdn_clip_indices(total, 0, 6, pad=total)
        clips = _gathered(pool, idx)
        by_hand = torch.cat([eng.forward_device(clips[i:i + 1]) for i in range(6)]).cpu()
        assert _same(got, by_hand)
        assert _same(tp.tdn_video_clip_logits(eng, video, tf, batch_clips=2), by_hand)
        assert _same(tp.tdn_video_clip_logits(eng, video, tf, clip_range=(2, 5)), by_hand[2:5])
        monkeypatch.setattr(ic, 'MAX_STAGE_BYTES', 30 * hh * ww * 3)          # 30 frames: pieces of two clips
        assert tp.tdn_clips_per_piece(hh * ww * 3) == 2
        with launch_trace() as tr:
            pieces = tp.tdn_video_clip_logits(eng, video, tf)
        assert tr.count('preprocess') == 3 and _same(pieces, by_hand)
        monkeypatch.undo()
        if not scale_255:
            return
        # the float64 network on the CPU transform of the same frames
        frames = torch.cat([tf(video.permute(0, 3, 1, 2).float()), tf(torch.zeros(1, 3, hh, ww))])
        x = frames[torch.from_numpy(idx.astype(np.int64)).reshape(-1)].reshape(6 * T, 15, h, h)
        with torch.no_grad():
            want = _model(D64, T)[0](x.double()).mean(1).numpy()
        err = assert_close(got.numpy(), want, what=f'pipeline logits {hh}x{ww}', **LOGITS_BAR)
        with capsys.disabled():
            print(f'\n[tdn pipeline {hh}x{ww} -> {resize} -> {h}] logits max|err|/scale {err:.2g}')
        # the count: the engine path and the host path (the torch transform, index_select, the engine on host clips)
        from workoutdetector_amd.counting import scores_to_preds
        host = _HostOnly(eng)
        host_logits = tp.tdn_video_clip_logits(host, video, tf)
        assert_close(host_logits.numpy(), want, what='host path', **LOGITS_BAR)
        for threshold in (0.0, 0.2, 0.5):
            assert tp.tdn_count_video(eng, video, tf, threshold=threshold) == tp.tdn_count_video(host, video, tf, threshold=threshold)
        assert scores_to_preds(got.numpy(), threshold=0.0) == scores_to_preds(host_logits.numpy(), threshold=0.0)
    finally:
        eng.close()


# ---- 9. the classification pipeline -------------------------------------------------------------------------------------------------
def test_classification_pipeline_engine_and_host_paths_agree(hip_lib):
    from workoutdetector_amd import tdn_pipeline as tp
    from workoutdetector_amd.engine import launch_trace
    from workoutdetector_amd.transform import TestTransform
    h, T = 64, 8
    samples = [dict(frame_dir='a', start_index=1, total_frames=40, label=0), dict(frame_dir='b', start_index=5, total_frames=9, label=1),
               dict(frame_dir='a', start_index=11, total_frames=13, label=2), dict(frame_dir='a', start_index=30, total_frames=60, label=6)]
    calls = []

    def reader(frame_dir, numbers):
        calls.append((frame_dir, list(numbers)))
        return np.stack([np.random.default_rng([ord(frame_dir), n]).integers(0, 256, (80, 100, 3), dtype=np.uint8) for n in numbers])
    tf = TestTransform(73, h, scale_255=True)
    eng = _engine(h, T, max_clips=2)
    try:
        with launch_trace() as tr:
            on_engine = tp.tdn_eval_classification(eng, samples, reader, return_logits=True, transform=tf)
        assert tr.count('preprocess') == 2 and tr.count('tdn_front_pool_kernel') == 3 and tr.count('top1_tally') == 3, tr.kernels
        assert tr.count('tdn_front_kernel') == 0 and not [k for k in tr.kernels if 'indexed' in k or 'gather' in k]
        assert [d for d, _n in calls] == ['a', 'a', 'b', 'b']          # (the probe frame, then the union, per directory)
        on_host = tp.tdn_eval_classification(_HostOnly(eng), samples, reader, return_logits=True, transform=tf)
    finally:
        eng.close()
    assert_close(on_engine.pop('logits'), on_host.pop('logits'), what='engine path against host path', **LOGITS_BAR)
    assert on_engine == on_host and on_engine['total'] == [1, 1, 1, 0, 0, 0, 1] and len(on_engine['preds']) == 4


def test_classification_pipeline_reader_calls_launch_order_and_refusals(hip_lib, monkeypatch):
    """What the engine path asks of the frame reader and of the GPU, to the call: per directory ONE read of the first sample's first
    frame, then per staged piece one read of the piece's whole union; no read and no launch for an empty list; the same launches in
    the same order whether or not the logits are asked for; frames of another size than the probe's refused before any launch."""
    from workoutdetector_amd import inference_count as ic, tdn_pipeline as tp
    from workoutdetector_amd.engine import launch_trace
    from workoutdetector_amd.transform import TestTransform
    h, T = 64, 3
    samples = [dict(frame_dir=d, start_index=s, total_frames=t, label=l) for d, s, t, l in
               (('a', 1, 40, 0), ('b', 5, 9, 1), ('a', 11, 13, 2), ('a', 30, 60, 6), ('b', 2, 30, 3), ('a', 3, 5, 9), ('a', 20, 21, -1))]
    rows = {d: [(tp.tdn_sample_frames(s['total_frames'], T) + s['start_index']).reshape(-1).tolist() for s in samples if s['frame_dir'] == d]
            for d in 'ab'}
    union = {d: sorted(set().union(*rows[d])) for d in 'ab'}
    calls = []

    def reader(frame_dir, numbers, rows_of=40):
        calls.append((frame_dir, list(numbers)))
        return np.stack([np.random.default_rng([ord(frame_dir), n]).integers(0, 256, (rows_of, 56, 3), dtype=np.uint8) for n in numbers])
    tf = TestTransform(73, h, scale_255=True)
    eng = _engine(h, T, max_clips=2)
    try:
        with launch_trace() as with_logits:
            res = tp.tdn_eval_classification(eng, samples, reader, return_logits=True, transform=tf)
        assert calls == [('a', rows['a'][0][:1]), ('a', union['a']), ('b', rows['b'][0][:1]), ('b', union['b'])]
        assert res['total'] == [1, 1, 1, 1, 0, 0, 1] and len(res['preds']) == 7 and res['logits'].shape == (7, NUM_CLASS)
        with launch_trace() as without:
            plain = tp.tdn_eval_classification(eng, samples, reader, transform=tf)
        assert without.kernels == with_logits.kernels and plain == {k: v for k, v in res.items() if k != 'logits'}
        k = without.kernels                                             # per piece the transform, per batch the forward and the tally
        assert without.count('preprocess') == 2 and 'preprocess' in k[0] and without.count('top1_tally') == 3 + 1
        assert without.count('tdn_front_pool_kernel') == 4 and 'top1_tally' in k[-1]
        assert [i for i, name in enumerate(k) if 'preprocess' in name][1] == [i for i, name in enumerate(k) if 'top1_tally' in name][2] + 1
        # pieces of whole samples under a budget of 20 frames: each reads its whole union, the probe is read once per directory
        monkeypatch.setattr(ic, 'MAX_STAGE_BYTES', 20 * 40 * 56 * 3)
        del calls[:]
        pieces = tp.tdn_eval_classification(eng, samples, reader, return_logits=True, transform=tf)
        want = []
        for d in 'ab':
            parts, cur = [], set()
            for r in rows[d]:
                if cur and len(cur | set(r)) > 20:
                    parts.append(cur)
                    cur = set()
                cur |= set(r)
            want += [(d, rows[d][0][:1])] + [(d, sorted(p)) for p in parts + [cur]]
        assert calls == want and len(want) > 4, calls
        assert _same(pieces['logits'], res['logits']) and pieces['preds'] == res['preds'] and pieces['total'] == res['total']
        monkeypatch.undo()
        del calls[:]
        with launch_trace() as tr:
            empty = tp.tdn_eval_classification(eng, [], reader, return_logits=True, transform=tf)
        assert calls == [] and tr.kernels == [] and empty['preds'] == [] and empty['overall'] is None
        with launch_trace() as tr:
            with pytest.raises(ValueError, match=r'a: frames of \(39, 56\) and \(40, 56\) pixels'):
                tp.tdn_eval_classification(eng, samples, lambda d, n: reader(d, n, 40 if len(n) == 1 else 39), transform=tf)
        assert tr.kernels == []
    finally:
        eng.close()
