"""A TDN forward in two phases (include/tsm_hip.h: TSM_LAYOUT_TDN_SEGMENTS / TSM_LAYOUT_TDN_RING; ``TsmEngine.tdn_segments`` /
``forward_ring``; csrc/tsm_tdn.hip: tdn_fuse_ring_kernel), the ``reuse_segments`` route and ``TdnStreamBatcher``, on the GPU.

Every kernel keeps one summation order per output whatever the batch, and tdn_fuse_ring_kernel spells tdn_fuse_kernel's blend
the same way: everything that compares segment phase + trunk phase with the whole forward on the same frames is bit for bit.
Engines as in tests/test_tdn_pool_gpu.py: depths (1, 1, 1, 2) unless said otherwise; 64 x 96 and 96 x 64 from tests/_geometry_cases.py,
where h, w, hd and wd are four different numbers.  Pools, tables, rings and outputs are
tests/_guard.py tensors: a stray read reads poison, a stray store breaks a band."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _geometry_cases as G
from tests._guard import POISON, check, guarded, guarded_out
from tests._tdn_cases import LOGITS_BAR, NUM_CLASS, bits as _bits, engine as _cases_engine, network as _model
from tests._util import assert_close

pytestmark = pytest.mark.gpu

D64 = (1, 1, 1, 2)
TAPS = ('fuse2', 'layer2.0', 'layer4.0')
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def _hw(size):
    return (size, size) if isinstance(size, int) else tuple(size)


def _frame_id(v):
    return '%dx%d' % v if isinstance(v, tuple) else str(v)


def _engine(size, T, max_clips=3, depths=D64, **kw):
    """``size``: the side of a square frame, or (h, w)."""
    h, w = _hw(size)
    return _cases_engine(h, w, T, depths, _model(depths, T)[1], max_clips=max_clips, **kw)


def _pool(n_frames, size, seed=7):
    h, w = _hw(size)
    x = np.random.default_rng([seed, n_frames, h] + ([] if isinstance(size, int) else [w])).standard_normal((n_frames, 3, h, w)).astype(np.float32)
    return guarded(torch.from_numpy(x).cuda(), name='pool')


def _segment_table(n, n_frames, seed=11):
    """[n, 5] random pool frame numbers; every segment also repeats one of its own frames."""
    t = np.random.default_rng([seed, n]).integers(0, n_frames, (n, 5)).astype(np.int32)
    t[:, 3] = t[:, 1]
    return t


def _slot_table(n_clips, T, n_slots, seed=13, first=0):
    """[n_clips, T] slots of [first, first + n_slots): a permutation first (every slot is read), then repeats."""
    rng = np.random.default_rng([seed, n_clips, T, n_slots])
    flat = np.concatenate([rng.permutation(n_slots), rng.integers(0, n_slots, n_clips * T)])[:n_clips * T]
    return (first + rng.permutation(flat)).reshape(n_clips, T).astype(np.int32)


def _same(a, b):
    a, b = (t.cpu().numpy() if hasattr(t, 'cpu') else t for t in (a, b))
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _ring(eng, n_slots):
    sa, sd = eng.ring_shapes(n_slots)
    return guarded_out(sa, name='ring_a'), guarded_out(sd, name='ring_d')


def _words(t):
    return t.contiguous().view(torch.int32)


TAP_MAPS = {'fuse2': ('ring_a', 256), 'layer2.0': ('layer2', 512), 'layer4.0': ('layer4', 2048)}          # (tests/_geometry_cases.py)


def _assert_split_equals_whole(eng, pool, seg_np, slots_np, first=0, n_slots=None, taps=TAPS, features=True, maps=None):
    """Segments ``seg_np`` [n, 5] into slots [first, first + n) of a guarded ring, clips by ``slots_np`` [n_clips, T] through
    forward_ring: the forward_pool of the [n_clips, T, 5] table those slots expand to, bit for bit.  ``maps``: the case table's
    record of the frame -- the taps' shapes are then held to it."""
    n, (n_clips, T) = seg_np.shape[0], slots_np.shape
    ring_a, ring_d = _ring(eng, n_slots or first + n)
    seg = guarded(torch.from_numpy(seg_np).cuda(), name='segment table')
    slots = guarded(torch.from_numpy(slots_np).cuda(), name='slot table')
    got = eng.tdn_segments(pool, seg, n_segments=n, out=(ring_a[first:first + n], ring_d[first:first + n]))
    assert got[0].data_ptr() == ring_a[first:].data_ptr()
    out = guarded_out(eng._out_shape(n_clips), name='logits')
    eng.forward_ring(ring_a, ring_d, slots, n_clips=n_clips, out=out)
    torch.cuda.synchronize()
    check(out, pool, seg, slots)
    table = torch.from_numpy(seg_np[slots_np - first]).cuda()                   # [n_clips, T, 5]
    want = eng.forward_pool(pool, table, n_clips=n_clips)
    torch.cuda.synchronize()
    assert _same(out, want), 'logits'
    assert float(want.abs().max()) > 0
    if features:
        feats = guarded_out((n_clips * T, eng.feature_dim), name='features')
        eng.forward_features_ring(ring_a, ring_d, slots, n_clips=n_clips, out=feats)
        torch.cuda.synchronize()
        check(feats)
        assert _same(feats, eng.forward_features_pool(pool, table, n_clips=n_clips)), 'features'
    for lo in range(0, n_clips if taps else 0, eng.max_clips):
        hi = min(lo + eng.max_clips, n_clips)
        for name in taps:
            got_tap = eng.forward_tap_ring(ring_a, ring_d, slots[lo:hi], n_clips=hi - lo, stage=name)
            assert _same(got_tap, eng.forward_tap_pool(pool, name, table[lo:hi], n_clips=hi - lo)), name
            if maps is not None:
                assert got_tap.shape == ((hi - lo) * T, *maps[TAP_MAPS[name][0]], TAP_MAPS[name][1]), (name, got_tap.shape)
    torch.cuda.synchronize()
    check(pool, seg, slots)
    return ring_a, ring_d, out


# ---- 1. split equals whole --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h, T, n_clips, max_clips, consensus', [(64, 8, 3, 3, 'avg'), (64, 8, 3, 3, 'identity'), (96, 8, 2, 2, 'avg'),
                                                                (64, 2, 1, 1, 'avg')] +
                         [((c['h'], c['w']), T, n, n, 'avg') for T, n in ((8, 2), (2, 1)) for c in G.TDN_RING], ids=_frame_id)
def test_segment_phase_and_trunk_phase_are_the_whole_forward(hip_lib, h, T, n_clips, max_clips, consensus):
    """(64, 2, 1, 1): alpha = 0.75, beta = 0.25 -- a blend whose products round, so the order of the fused multiply-add counts.
    h = (rows, columns): the non-square frames of tests/_geometry_cases.py, ring maps 16 x 24 / 8 x 12 and their transposes --
    tdn_fuse_ring_kernel's own copy of the blend's h, w, hd, wd held to tdn_fuse_kernel where they differ."""
    eng = _engine(h, T, max_clips=max_clips, consensus=consensus)
    try:
        n = max(2, n_clips * T // 2 + 1)                       # fewer segments than clip positions: slots repeat
        maps = G.maps_of('tdn_ring', *h) if isinstance(h, tuple) else None
        if maps is not None:
            assert eng.ring_shapes(n) == ((n, *maps['ring_a'], 256), (n, *maps['ring_d'], 256))
        ring_a, ring_d, _out = _assert_split_equals_whole(eng, _pool(11, h), _segment_table(n, 11), _slot_table(n_clips, T, n), maps=maps)
        check(ring_a, ring_d)                                  # every word of every slot was written, no band touched
        if maps is not None:                                   # which kernel that was
            from workoutdetector_amd.engine import launch_trace
            with launch_trace() as tr:
                eng.forward_ring(ring_a, ring_d, torch.from_numpy(_slot_table(n_clips, T, n)).cuda(), n_clips=n_clips)
            assert tr.count('tdn_fuse_ring_kernel') == 1 and tr.count('tdn_fuse_kernel') == 0, tr.kernels
    finally:
        eng.close()


# ---- 2. only what was asked is written --------------------------------------------------------------------------------------------
def test_a_segment_call_writes_its_slots_and_nothing_else(hip_lib):
    _writes_its_slots_and_nothing_else(64)


def test_a_segment_call_writes_its_slots_on_a_non_square_frame(hip_lib):
    _writes_its_slots_and_nothing_else((96, 64))


def _writes_its_slots_and_nothing_else(h):
    T, first, n, n_slots = 8, 2, 3, 7
    eng = _engine(h, T)
    try:
        ring_a, ring_d, _out = _assert_split_equals_whole(eng, _pool(11, h), _segment_table(n, 11), _slot_table(1, T, n, first=first),
                                                          first=first, n_slots=n_slots, taps=(), features=False)
        for ring in (ring_a, ring_d):
            w = _words(ring)
            assert bool((w[:first] == POISON).all()) and bool((w[first + n:] == POISON).all())          # every other slot: poison, bit for bit
            assert not bool((w[first:first + n] == POISON).any())                                       # its own slots: no word left
        with pytest.raises(Exception):
            check(ring_a)                                       # (the guard agrees: payload words of the other slots are unwritten)
    finally:
        eng.close()


# ---- 3. the kernel is total in the slot table -------------------------------------------------------------------------------------
def test_table_entries_outside_the_ring_are_zeros(hip_lib):
    """T = 8: alpha = beta = 0.5, both products exact, so torch's multiply-then-add equals the kernel's fused form bit for bit
    and fuse2's tap can be held to a torch expression on the ring itself."""
    _entries_outside_the_ring(64)


def test_table_entries_outside_the_ring_on_a_non_square_frame(hip_lib):
    """64 x 96: the torch expression indexes rows with h / 4 and columns with w / 4, each on its own."""
    _entries_outside_the_ring((64, 96))


def _entries_outside_the_ring(size):
    (h, w), T, n_clips, n = _hw(size), 8, 2, 6
    eng = _engine(size, T)
    try:
        pool, seg_np = _pool(11, size), _segment_table(n, 11)
        ring_a, ring_d = _ring(eng, n + 1)                     # slot n: a segment of zeros
        eng.tdn_segments(pool, torch.from_numpy(seg_np).cuda(), n_segments=n, out=(ring_a[:n], ring_d[:n]))
        ring_a[n].zero_()
        ring_d[n].zero_()
        torch.cuda.synchronize()
        check(ring_a, ring_d)
        slots_np = _slot_table(n_clips, T, n)
        bad = slots_np.copy()
        bad[0, 1], bad[0, 6], bad[1, 0], bad[1, 7], bad[1, 3] = -1, n + 1, I32_MIN, I32_MAX, n + 2
        zeroed = np.where((bad >= 0) & (bad <= n), bad, n).astype(np.int32)
        assert (zeroed == n).sum() == 5
        bad_t = guarded(torch.from_numpy(bad).cuda(), name='slot table')
        got = eng.forward_ring(ring_a, ring_d, bad_t, n_clips=n_clips)
        want = eng.forward_ring(ring_a, ring_d, torch.from_numpy(zeroed).cuda(), n_clips=n_clips)
        tap = eng.forward_tap_ring(ring_a, ring_d, bad_t, n_clips=n_clips, stage='fuse2')
        torch.cuda.synchronize()
        check(ring_a, ring_d, bad_t)                            # no band is touched
        assert _same(got, want) and not _same(got, eng.forward_ring(ring_a, ring_d, torch.from_numpy(slots_np).cuda(), n_clips=n_clips))
        # fuse2 from the ring by torch: nearest upsample of an exact 2x is index // 2
        idx = torch.from_numpy(zeroed.reshape(-1).astype(np.int64)).cuda()
        a, d = ring_a[idx], ring_d[idx]
        rows, cols = torch.arange(h // 4).cuda() // 2, torch.arange(w // 4).cuda() // 2
        up = d[:, rows][:, :, cols]
        assert tuple(up.shape) == tuple(a.shape) == (n_clips * T, h // 4, w // 4, 256)
        assert _same(tap, (0.5 * a + 0.5 * up)), 'fuse2'
        assert not tap[1].any() and tap[0].any()                # clip 0, segment 1: zeros
    finally:
        eng.close()


# ---- 4. chunking ------------------------------------------------------------------------------------------------------------------
def test_more_segments_and_clips_than_one_call_holds(hip_lib):
    h, T, max_clips = 64, 8, 2
    eng = _engine(h, T, max_clips=max_clips)
    try:
        pool = _pool(11, h)
        n = max_clips * T + 3                                   # calls of 16 + 3 segments; 3 clips: calls of 2 + 1
        _assert_split_equals_whole(eng, pool, _segment_table(n, 11), _slot_table(max_clips + 1, T, n), taps=('fuse2',))
        _assert_split_equals_whole(eng, pool, _segment_table(5, 11, seed=3), _slot_table(1, T, 5), taps=())     # 5 segments: no multiple of T
    finally:
        eng.close()


# ---- 5. the launch cap ------------------------------------------------------------------------------------------------------------
def test_the_fuse_kernel_wraps_at_its_launch_cap(hip_lib):
    """257 segments of 16 x 16 x 64 quads: the first count above 16384 workgroups of 256."""
    from tests._tdn_cases import launch_pass
    assert launch_pass('tdn_fuse_ring_kernel', r'n_spans \* 256') == launch_pass('tdn_fuse_kernel', 'quads') == 16384 * 256
    assert 256 * 16 * 16 * 64 == 16384 * 256
    h, T, max_clips = 64, 8, 33
    eng = _engine(h, T, max_clips=max_clips, depths=(1, 1, 1, 1))
    try:
        slots = (np.arange(max_clips * T, dtype=np.int32) % 257).reshape(max_clips, T)
        slots[:, 7] = np.random.default_rng(5).integers(0, 257, max_clips)
        slots[32, 7] = 256                                      # the 257th segment, and the last segment of the launch
        _assert_split_equals_whole(eng, _pool(11, h), _segment_table(257, 11), slots, taps=('fuse2',), features=False)
    finally:
        eng.close()


# ---- 6. which kernels ran ---------------------------------------------------------------------------------------------------------
def test_each_phase_runs_its_own_launches_only(hip_lib):
    from workoutdetector_amd.engine import launch_trace
    h, T, n_clips = 64, 8, 2
    n = n_clips * T
    eng = _engine(h, T, max_clips=n_clips)
    try:
        pool, seg_np = _pool(11, h), _segment_table(n, 11)
        seg = torch.from_numpy(seg_np).cuda()
        slots = torch.arange(n, dtype=torch.int32).reshape(n_clips, T).cuda()
        ring_a, ring_d = _ring(eng, n)
        with launch_trace() as whole:
            eng.forward_pool(pool, seg.reshape(n_clips, T, 5), n_clips=n_clips)
        with launch_trace() as front:
            eng.tdn_segments(pool, seg, n_segments=n, out=(ring_a, ring_d))
        with launch_trace() as trunk:
            eng.forward_ring(ring_a, ring_d, slots, n_clips=n_clips)
        names = eng.launch_names()
        eng.set_layer_timing(2)
        eng.tdn_segments(pool, seg, n_segments=n, out=(ring_a, ring_d))
        eng.forward_ring(ring_a, ring_d, slots, n_clips=n_clips)
        torch.cuda.synchronize()
        t_front, t_trunk = eng.layer_times_ms(0), eng.layer_times_ms(1)
    finally:
        eng.close()
    plain = lambda tr: [k.replace(' [reverse]', '') for k in tr.kernels]
    assert whole.count('tdn_fuse_kernel') == 2 and whole.count('tdn_fuse_ring_kernel') == 0 and whole.count('tdn_front_pool_kernel') == 1
    cut = [i for i, k in enumerate(whole.kernels) if k.startswith('tdn_fuse_kernel')][1]
    # the segment phase: the whole forward's launches in front of fuse2, nothing behind; the trunk phase: the ring kernel in
    # fuse2's place, then the whole forward's launches behind it (walk directions aside: they alternate per launch)
    assert plain(front) == plain(whole)[:cut], (front.kernels, whole.kernels[:cut])
    assert trunk.count('tdn_fuse_ring_kernel') == 1 and trunk.kernels[0].startswith('tdn_fuse_ring_kernel')
    assert plain(trunk)[1:] == plain(whole)[cut + 1:]
    for tr, absent in ((trunk, ('tdn_front', 'stem', 'maxpool', 'tdn_fuse_kernel')), (front, ('mse_', 'head', 'tdn_fuse_ring', 'pool_feat'))):
        assert not [k for k in tr.kernels if k.startswith(absent)], tr.kernels
    assert front.count('tdn_fuse_kernel') == 1
    # the timing slots stay a whole forward's: what a phase does not launch is not recorded
    seam = names.index('fuse2')
    assert list(t_front) == list(t_trunk) == names
    assert all(t_trunk[k] < 0 for k in names[:seam]) and t_trunk['fuse2'] > 0 and t_trunk['head'] > 0
    assert all(t_front[k] < 0 for k in names[seam:]) and t_front['diff.front.0'] > 0 and t_front['fuse1'] > 0
    assert t_front['layer1.0.conv1'] > 0 and t_trunk['layer2.0.conv1'] > 0 and t_trunk['layer2.0.mse_squeeze'] > 0


# ---- 7. capture and replay ---------------------------------------------------------------------------------------------------------
def test_both_phases_captured_on_a_side_stream_read_the_slot_table_at_replay(hip_lib):
    """Sets A and B share the pool and the segment table and differ in the SLOT table alone: the replay on B gives B's eager
    logits, so the slots are read on the device when the kernel runs."""
    from tests._capture import captured
    h, T, n_clips, n = 64, 2, 2, 5
    frames = [np.random.default_rng([47, k]).standard_normal((11, 3, h, h)).astype(np.float32) for k in range(2)]
    seg_np = _segment_table(n, 11)
    sets = [[torch.from_numpy(frames[0]), torch.from_numpy(seg_np), torch.from_numpy(_slot_table(n_clips, T, n, seed=1))],
            [torch.from_numpy(frames[0]), torch.from_numpy(seg_np), torch.from_numpy(_slot_table(n_clips, T, n, seed=2))],
            [torch.from_numpy(frames[1]), torch.from_numpy(_segment_table(n, 11, seed=9)), torch.from_numpy(_slot_table(n_clips, T, n, seed=3))]]
    assert not np.array_equal(sets[0][2].numpy(), sets[1][2].numpy())
    eng = _engine(h, T, max_clips=n_clips, autotune=True)
    try:
        pool = guarded(torch.zeros(11, 3, h, h).cuda(), name='pool')
        seg = guarded(torch.zeros(n, 5, dtype=torch.int32).cuda(), name='segment table')
        slots = guarded(torch.zeros(n_clips, T, dtype=torch.int32).cuda(), name='slot table')
        ring_a, ring_d = _ring(eng, n)
        out = guarded_out(eng._out_shape(n_clips), name='logits')

        def run():
            eng.tdn_segments(pool, seg, n_segments=n, out=(ring_a, ring_d))
            eng.forward_ring(ring_a, ring_d, slots, n_clips=n_clips, out=out)
        run()                                                   # the first call of each bucket tunes inside the call
        torch.cuda.synchronize()
        tr = captured(run, [pool, seg, slots], lambda k: sets[k], [ring_a, ring_d, out], engine=eng)
        table_b = torch.from_numpy(seg_np[sets[1][2].numpy()]).cuda()
        want_b = eng.forward_pool(sets[1][0].cuda(), table_b, n_clips=n_clips)
        torch.cuda.synchronize()
    finally:
        eng.close()
    # (5 segments through an engine of max_clips * T = 4: tdn_segments makes two calls, 4 + 1 segments)
    assert tr.count('tdn_fuse_ring_kernel') == 1 and tr.count('tdn_front_pool_kernel') == 2 and tr.count('tdn_fuse_kernel') == 2
    assert _same(tr.refs['B'][2], want_b) and not _same(tr.refs['A'][2], tr.refs['B'][2])
    assert _same(tr.refs['A'][0], tr.refs['B'][0])              # (the ring itself: the same segments)


# ---- 8. poison ---------------------------------------------------------------------------------------------------------------------
def test_both_phases_under_poison(hip_lib):
    h, T, n_clips, n = 96, 8, 2, 9
    pool, seg_np = _pool(11, h), _segment_table(n, 11)
    seg_np[4, 4] = -1
    seg = torch.from_numpy(seg_np).cuda()
    slots_np = _slot_table(n_clips, T, n)
    slots_np[1, 2] = -1
    slots = torch.from_numpy(slots_np).cuda()
    plain, hostile = _engine(h, T, max_clips=n_clips), _engine(h, T, max_clips=n_clips, poison=True)
    try:
        rings = []
        for eng in (plain, hostile):
            ring_a, ring_d = _ring(eng, n)
            eng.tdn_segments(pool, seg, n_segments=n, out=(ring_a, ring_d))
            torch.cuda.synchronize()
            check(ring_a, ring_d)                               # written in full, and never poisoned by the engine
            rings.append((ring_a, ring_d))
        assert _same(rings[0][0], rings[1][0]) and _same(rings[0][1], rings[1][1])
        keep = [r.clone() for r in rings[1]]
        outs = [[eng.forward_ring(*r, slots, n_clips=n_clips), eng.forward_ring(*r, slots[:1], n_clips=1),
                 eng.forward_features_ring(*r, slots, n_clips=n_clips)] +
                [torch.from_numpy(eng.forward_tap_ring(*r, slots, n_clips=n_clips, stage=s)) for s in ('fuse2', 'layer4.1')]
                for eng, r in zip((plain, hostile), rings)]
        torch.cuda.synchronize()
        for a, b in zip(*outs):
            assert _same(a, b)
        assert _same(keep[0], rings[1][0]) and _same(keep[1], rings[1][1])          # the trunk phase reads the ring, nothing more
        for name in ('diff.stem', 'layer1.0'):
            taps = []
            for eng in (plain, hostile):
                d = _segments_desc(pool, seg, rings[0], n)
                taps.append(_tap(eng, d, 17, n, name))
            assert _same(*taps), name
        check(pool)
    finally:
        plain.close()
        hostile.close()


def _segments_desc(pool, seg, ring, n, **kw):
    from workoutdetector_amd import _lib
    d = _lib.TsmTdnSegments(struct_size=C.sizeof(_lib.TsmTdnSegments), mode=0, frames=pool.data_ptr(), n_frames=pool.shape[0],
                            index=seg.data_ptr(), out_a=ring[0].data_ptr(), out_d=ring[1].data_ptr())
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _ring_desc(ring, slots, **kw):
    from workoutdetector_amd import _lib
    d = _lib.TsmTdnRing(struct_size=C.sizeof(_lib.TsmTdnRing), n_slots=ring[0].shape[0], ring_a=ring[0].data_ptr(), ring_d=ring[1].data_ptr(),
                        table=slots.data_ptr())
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _tap(eng, desc, layout, n, stage):
    from workoutdetector_amd import _lib
    cap = n * eng.num_segments * eng.height * eng.width * 16
    buf = torch.empty(cap, dtype=torch.float32, device='cuda')
    shape = (C.c_int64 * 4)()
    _lib.check(eng._lib.tsm_forward_tap(eng._h, C.addressof(desc), _lib.MEM_DEVICE, layout, n, stage.encode(), buf.data_ptr(), cap, shape, None), eng._h)
    dims = tuple(int(v) for v in shape)
    return buf[:int(np.prod(dims))].reshape(dims).cpu()


# ---- 9. the error contract ---------------------------------------------------------------------------------------------------------
def test_the_error_contract_launches_nothing(hip_lib, sd0):
    from workoutdetector_amd import _lib
    from workoutdetector_amd.engine import TsmEngine, launch_trace
    lib = hip_lib
    h, T, n = 64, 2, 3
    pool = _pool(11, h)
    seg = torch.from_numpy(_segment_table(n, 11)).cuda()
    slots = torch.from_numpy(_slot_table(1, T, n)).cuda()
    eng = _engine(h, T, max_clips=2)
    other = TsmEngine(num_class=12, num_segments=T, height=h, width=h, max_clips=2, state_dict=sd0)
    ring = _ring(eng, n)
    out = guarded_out((1, NUM_CLASS), name='logits')
    feats = guarded_out((T, 2048), name='features')
    shape = (C.c_int64 * 4)()
    SEG, RING = _lib.LAYOUT_TDN_SEGMENTS, _lib.LAYOUT_TDN_RING
    bad_seg = {'struct_size': dict(struct_size=72), 'frames is NULL': dict(frames=None), '8-byte': dict(frames=pool.data_ptr() + 4),
               'n_frames': dict(n_frames=0), 'mode': dict(mode=2), 'needs index': dict(index=None),
               'clip_stride': dict(mode=1, total_frames=11, clip_stride=0), 'total_frames': dict(mode=1, total_frames=0, clip_stride=2),
               'NULL': dict(out_a=None), 'NULL ': dict(out_d=None), '16-byte': dict(out_a=ring[0].data_ptr() + 8),
               '16-byte ': dict(out_d=ring[1].data_ptr() + 4)}
    bad_ring = {'struct_size': dict(struct_size=24), 'n_slots': dict(n_slots=0), 'n_slots ': dict(n_slots=-1), 'NULL': dict(ring_a=None),
                'NULL ': dict(ring_d=None), '16-byte': dict(ring_a=ring[0].data_ptr() + 4), '16-byte ': dict(ring_d=ring[1].data_ptr() + 8),
                'table is NULL': dict(table=None), '4-byte': dict(table=slots.data_ptr() + 2)}
    try:
        def calls(e, d, layout, count, memkind=_lib.MEM_DEVICE, stage=None):
            p = C.addressof(d)
            stage = stage or (b'stem' if layout == SEG else b'fuse2')
            return (lib.tsm_forward(e._h, p, memkind, layout, count, out.data_ptr(), None),
                    lib.tsm_forward_tap(e._h, p, memkind, layout, count, stage, feats.data_ptr(), feats.numel(), shape, None))
        with launch_trace() as tr:
            for what, kw in bad_seg.items():
                assert calls(eng, _segments_desc(pool, seg, ring, n, **kw), SEG, n) == (-1, -1), what
                assert what.strip() in lib.tsm_last_error(eng._h).decode(), (what, lib.tsm_last_error(eng._h))
            for what, kw in bad_ring.items():
                assert calls(eng, _ring_desc(ring, slots, **kw), RING, 1) == (-1, -1), what
                assert what.strip() in lib.tsm_last_error(eng._h).decode(), (what, lib.tsm_last_error(eng._h))
            good_seg, good_ring = _segments_desc(pool, seg, ring, n), _ring_desc(ring, slots)
            # host memory; a TSM engine; NULL; the counts
            for d, layout, count in ((good_seg, SEG, n), (good_ring, RING, 1)):
                assert calls(eng, d, layout, count, _lib.MEM_HOST) == (-1, -1) and 'TSM_MEM_DEVICE' in lib.tsm_last_error(eng._h).decode()
                assert calls(other, d, layout, count) == (-7, -7) and 'TDN engine' in lib.tsm_last_error(other._h).decode()
                assert lib.tsm_forward(eng._h, None, _lib.MEM_DEVICE, layout, count, out.data_ptr(), None) == -1
                assert calls(eng, d, layout, 0) == (-1, -1)
            assert calls(eng, good_seg, SEG, 2 * T + 1) == (-6, -6) and 'max_clips * T' in lib.tsm_last_error(eng._h).decode()
            assert calls(eng, good_ring, RING, 3) == (-6, -6)
            # each tap name on the wrong side of the seam
            def tap(d, layout, count, stage):
                return lib.tsm_forward_tap(eng._h, C.addressof(d), _lib.MEM_DEVICE, layout, count, stage, feats.data_ptr(), feats.numel(), shape, None)
            for stage in (b'fuse2', b'layer2.0', b'layer2.0.conv1', b'layer4.1', b'layer3.0.shift'):
                assert tap(good_seg, SEG, n, stage) == -1 and 'segment phase' in lib.tsm_last_error(eng._h).decode(), stage
            for stage in (b'diff.conv1_5', b'diff.stem', b'stem', b'fuse1', b'resnext_layer1.0', b'layer1.0', b'layer1.0.conv2'):
                assert tap(good_ring, RING, 1, stage) == -1 and 'trunk phase' in lib.tsm_last_error(eng._h).decode(), stage
            # the segment phase has no feature rows; the trunk phase needs its output
            assert lib.tsm_forward_features(eng._h, C.addressof(good_seg), _lib.MEM_DEVICE, SEG, n, feats.data_ptr(), 0, None) == -7
            assert lib.tsm_forward(eng._h, C.addressof(good_ring), _lib.MEM_DEVICE, RING, 1, None, None) == -1
            assert lib.tsm_forward_features(eng._h, C.addressof(good_ring), _lib.MEM_DEVICE, RING, 1, None, 0, None) == -1
        assert tr.kernels == [], tr.kernels
        torch.cuda.synchronize()
        # nothing was written; and the Python wrappers refuse what the C ABI cannot see
        for t in (out, feats) + ring:
            assert bool((_words(t) == POISON).all())
        for bad in (lambda: eng.tdn_segments(pool, seg, n_segments=n, out=(ring[0][:2], ring[1][:2])),
                    lambda: eng.tdn_segments(pool, seg.long(), n_segments=n, out=ring),
                    lambda: eng.tdn_segments(pool, seg, window=dict(first_clip=0), n_segments=n, out=ring),
                    lambda: eng.tdn_segments(pool, n_segments=n, out=ring),
                    lambda: eng.tdn_segments(pool, seg, n_segments=n, out=(ring[1], ring[0])),
                    lambda: eng.forward_ring(ring[0], ring[1], slots.long(), n_clips=1),
                    lambda: eng.forward_ring(ring[0], ring[1], slots, n_clips=2),
                    lambda: eng.forward_ring(ring[0].cpu(), ring[1].cpu(), slots, n_clips=1),
                    lambda: eng.forward_ring(ring[0][:, :8], ring[1], slots, n_clips=1)):
            with pytest.raises(ValueError):
                bad()
        with pytest.raises(ValueError, match='TDN engine'):
            other.forward_ring(ring[0], ring[1], slots, n_clips=1)
        # and the descriptors that are accepted run: logits may be NULL for the segment phase
        assert lib.tsm_forward(eng._h, C.addressof(good_seg), _lib.MEM_DEVICE, SEG, n, None, None) == 0
        assert lib.tsm_forward(eng._h, C.addressof(good_ring), _lib.MEM_DEVICE, RING, 1, out.data_ptr(), None) == 0
        torch.cuda.synchronize()
        check(out, pool, *ring)
    finally:
        eng.close()
        other.close()


def test_a_ring_with_its_spatial_dims_exchanged_is_refused_before_any_launch(hip_lib):
    """a [n, W / 4, H / 4, 256] and d [n, W / 8, H / 8, 256] to an H x W engine: as many words as the right pair, so the C ABI's
    bare pointers could not tell -- ``_check_ring`` is the only check there is, for both phases."""
    from workoutdetector_amd.engine import launch_trace
    h, w, T, n = 64, 96, 2, 3
    eng = _engine((h, w), T, max_clips=2)
    try:
        pool = _pool(11, (h, w))
        seg = torch.from_numpy(_segment_table(n, 11)).cuda()
        slots = torch.from_numpy(_slot_table(1, T, n)).cuda()
        maps = G.maps_of('tdn_ring', h, w)
        sa, sd = (n, *maps['ring_a'], 256), (n, *maps['ring_d'], 256)
        assert eng.ring_shapes(n) == (sa, sd)
        turned = (guarded_out((n, sa[2], sa[1], 256), name='ring_a'), guarded_out((n, sd[2], sd[1], 256), name='ring_d'))
        good = _ring(eng, n)
        out = guarded_out((1, NUM_CLASS), name='logits')
        with launch_trace() as tr:
            for pair in (turned, (turned[0], good[1]), (good[0], turned[1])):
                with pytest.raises(ValueError, match=r'need a \[3, 16, 24, 256\] and d \[3, 8, 12, 256\]'):
                    eng._check_ring(*pair)
                with pytest.raises(ValueError, match='need a'):
                    eng.tdn_segments(pool, seg, n_segments=n, out=pair)
                with pytest.raises(ValueError, match='need a'):
                    eng.forward_ring(pair[0], pair[1], slots, n_clips=1, out=out)
                with pytest.raises(ValueError, match='need a'):
                    eng.forward_features_ring(pair[0], pair[1], slots, n_clips=1)
                with pytest.raises(ValueError, match='need a'):
                    eng.forward_tap_ring(pair[0], pair[1], slots, n_clips=1, stage='fuse2')
        assert tr.kernels == [], tr.kernels
        torch.cuda.synchronize()
        for t in (out,) + turned + good:
            assert bool((_words(t) == POISON).all())
        assert eng._check_ring(*good) == n                      # and the pair the right way round runs
        eng.tdn_segments(pool, seg, n_segments=n, out=good)
        eng.forward_ring(good[0], good[1], slots, n_clips=1, out=out)
        torch.cuda.synchronize()
        check(out, pool, *good)
    finally:
        eng.close()


# ---- 10. the pipelines -------------------------------------------------------------------------------------------------------------
def _video(total, hh, ww, seed=3):
    return torch.from_numpy(np.random.default_rng([seed, hh, ww]).integers(0, 256, (total, hh, ww, 3), dtype=np.uint8))


@pytest.mark.parametrize('hh, ww', [(80, 100), (40, 56)], ids=str)
def test_reuse_segments_is_the_default_route_bit_for_bit(hip_lib, monkeypatch, capsys, hh, ww):
    """45 frames (80 x 100 -> 73 -> 64, and 40 x 56 upscaled): 6 clips read 23 unique segments and the pad segment, not 48."""
    from workoutdetector_amd import inference_count as ic, tdn_pipeline as tp
    from workoutdetector_amd.engine import launch_trace
    from workoutdetector_amd.transform import TestTransform
    total, h, T = 45, 64, 8
    video = _video(total, hh, ww)
    tf = TestTransform(73, h, scale_255=True)
    eng = _engine(h, T, max_clips=4)
    try:
        want = tp.tdn_video_clip_logits(eng, video, tf)
        with launch_trace() as tr:
            got = tp.tdn_video_clip_logits(eng, video, tf, reuse_segments=True)
        assert _same(got, want)
        # one transform, ONE segment call (23 unique + pad = 24 segments: one front-end chunk), two trunk batches of 4 + 2 clips
        assert tr.count('preprocess') == 1 and tr.count('tdn_front_pool_kernel') == 1 and tr.count('tdn_fuse_ring_kernel') == 2, tr.kernels
        assert tr.count('tdn_fuse_kernel') == 1 and tr.count('tdn_front_kernel') == 0
        assert _same(tp.tdn_video_clip_logits(eng, video, tf, batch_clips=1, reuse_segments=True), want)
        assert _same(tp.tdn_video_clip_logits(eng, video, tf, clip_range=(2, 5), reuse_segments=True), want[2:5])
        for threshold in (0.0, 0.2):
            assert tp.tdn_count_video(eng, video, tf, threshold=threshold, reuse_segments=True) == tp.tdn_count_video(eng, video, tf, threshold=threshold)
        monkeypatch.setattr(ic, 'MAX_STAGE_BYTES', 30 * hh * ww * 3)          # 30 frames: pieces of two clips
        assert tp.tdn_clips_per_piece(hh * ww * 3) == 2
        with launch_trace() as tr:
            pieces = tp.tdn_video_clip_logits(eng, video, tf, reuse_segments=True)
        assert tr.count('preprocess') == 3 and tr.count('tdn_fuse_ring_kernel') == 3 and _same(pieces, want)
        monkeypatch.undo()
        # the float64 network on the CPU transform of the same frames: the bar tests/test_tdn_pool_gpu.py holds this pipeline to
        idx = tp.tdn_clip_indices(total, 0, 6, pad=total)
        frames = torch.cat([tf(video.permute(0, 3, 1, 2).float()), tf(torch.zeros(1, 3, hh, ww))])
        x = frames[torch.from_numpy(idx.astype(np.int64)).reshape(-1)].reshape(6 * T, 15, h, h)
        with torch.no_grad():
            ref = _model(D64, T)[0](x.double()).mean(1).numpy()
        err = assert_close(got.numpy(), ref, what=f'reuse_segments logits {hh}x{ww}', **LOGITS_BAR)
        with capsys.disabled():
            print(f'\n[tdn reuse_segments {hh}x{ww} -> 73 -> {h}] logits max|err|/scale {err:.2g}')
    finally:
        eng.close()


# ---- 11. streams -------------------------------------------------------------------------------------------------------------------
def test_streams_equal_the_offline_pipeline_bit_for_bit(hip_lib):
    """Three streams (45, 17 and 100 frames; two frame sizes) pushed in a seeded random interleaving with step() at random points."""
    from workoutdetector_amd import tdn_pipeline as tp
    from workoutdetector_amd.engine import launch_trace
    from workoutdetector_amd.transform import TestTransform
    h, T = 64, 8
    tf = TestTransform(73, h, scale_255=True)
    videos = {'a': _video(45, 80, 100, 3), 'b': _video(17, 40, 56, 4), 'c': _video(100, 80, 100, 5)}
    eng = _engine(h, T, max_clips=4)
    try:
        want = {k: tp.tdn_video_clip_logits(eng, v, tf) for k, v in videos.items()}
        counts = {k: tp.tdn_count_video(eng, v, tf, threshold=0.2) for k, v in videos.items()}
        sb = tp.TdnStreamBatcher(eng, threshold=0.2, transform=tf, max_batch=3, keep_logits=True)
        rng = np.random.default_rng(17)
        at = {k: 0 for k in videos}
        emitted = {k: [] for k in videos}
        peak = 0
        with launch_trace() as tr:
            while any(at[k] < len(v) for k, v in videos.items()):
                k = rng.choice([k for k, v in videos.items() if at[k] < len(v)])
                sb.push(k, videos[k][at[k]].numpy())
                at[k] += 1
                if rng.random() < 0.08:
                    n_ready = sb.ready()
                    res = sb.step()
                    assert sum(len(v) for v in res.values()) == n_ready and sb.ready() == 0
                    for sid, rows in res.items():
                        emitted[sid] += rows
                    assert all(st.ring.in_use <= 7 for st in sb.streams.values())              # the bound between steps
                    assert all(st.base == max(0, 2 * st.computed - 2) for st in sb.streams.values())
                    peak = max(peak, sb.slots_in_use())
        assert peak > 0 and tr.count('tdn_fuse_ring_kernel') > 0 and tr.count('tdn_front_kernel') == 0
        # every segment ran once: the front end saw 4 new segments per clip, not 8
        for k, v in videos.items():
            assert [c for c, _s, _n in emitted[k]] == list(range(len(emitted[k])))
            assert sb.close(k) == counts[k], k
            rows = sb.logits[k]
            assert [c for c, _r in rows] == list(range(want[k].shape[0])), k
            for c, r in rows:
                assert _same(r, want[k][c].numpy()), (k, c)
            assert len(rows) - len(emitted[k]) <= 2 or len(v) <= 17
        assert sb.slots_in_use() == 0 and not sb.streams
        assert sorted(sb._free) == list(range(1, sb._ring_a.shape[0]))                         # every slot but the pad's is free again
    finally:
        eng.close()


@pytest.mark.parametrize('total', [1, 16, 17])
def test_a_stream_closed_early(hip_lib, total):
    from workoutdetector_amd import tdn_pipeline as tp
    from workoutdetector_amd.transform import TestTransform
    h, T = 64, 8
    tf = TestTransform(73, h, scale_255=True)
    video = _video(total, 40, 56, total)
    eng = _engine(h, T, max_clips=2)
    try:
        sb = tp.TdnStreamBatcher(eng, threshold=0.2, transform=tf, keep_logits=True)
        for f in video:
            sb.push('s', f.numpy())
        if total == 17:
            assert sb.ready() == 1 and [c for c, _s, _n in sb.step()['s']] == [0]
        assert sb.close('s') == tp.tdn_count_video(eng, video, tf, threshold=0.2)
        want = tp.tdn_video_clip_logits(eng, video, tf)
        assert len(sb.logits['s']) == want.shape[0] == (total + 7) // 8
        assert all(_same(r, want[c].numpy()) for c, r in sb.logits['s'])
        assert sb.slots_in_use() == 0
    finally:
        eng.close()
