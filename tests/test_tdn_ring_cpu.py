"""The host side of the TDN forward in two phases (include/tsm_hip.h: TSM_LAYOUT_TDN_SEGMENTS / TSM_LAYOUT_TDN_RING) without a
GPU: ``TdnSegmentRing`` against brute force over ``tdn_clip_indices``, ``TdnStreamBatcher`` on a stub host model against the
offline functions, the refusals before the library loads, the ABI, and the host rules under sanitizers."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from workoutdetector_amd import tdn_pipeline as tp
from workoutdetector_amd.transform import PersonCropTransform, TestTransform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOTALS = [1, 5, 16, 17, 18, 24, 25, 45, 47, 64, 100]
PAD = 10 ** 6            # tdn_clip_indices' pad value here: no frame number reaches it


def _ring(n_slots=64, pad_slot=0):
    return tp.TdnSegmentRing([s for s in range(n_slots - 1, -1, -1) if s != pad_slot], pad_slot)


def _n_clips(total):
    return (total + 7) // 8


# ---- TdnSegmentRing against brute force -------------------------------------------------------------------------------------
@pytest.mark.parametrize('total', TOTALS)
def test_unique_segments_and_the_table_are_those_of_the_clip_indices(total):
    n = _n_clips(total)
    idx = tp.tdn_clip_indices(total, 0, n, pad=PAD)                       # [n, 8, 5]
    ring = _ring()
    for lo, hi in ((0, n), (n // 2, n), (0, max(1, n - 1))):
        rows = {tuple(r) for r in idx[lo:hi].reshape(-1, 5).tolist()} - {(PAD,) * 5}
        keys = ring.segments(lo, hi, total)
        assert len(keys) == len(set(keys)) == len(rows), (total, lo, hi)          # the unique-segment set, pad aside
        assert {tuple(ring.frames_of(k)) for k in keys} == rows
        assert keys == sorted(keys)
    # every segment is a function of its centre and the video's length alone: the same five frames whichever clip reads it
    by_centre = {}
    for c in range(n):
        for k in range(8):
            assert by_centre.setdefault(8 * c + 2 * k, idx[c, k].tolist()) == idx[c, k].tolist()
            assert (idx[c, k] == PAD).all() == (8 * c + 2 * k >= total)
    # the table: every row names slots whose segment has exactly the frames tdn_clip_indices gives
    new = ring.assign(ring.segments(0, n, total))
    assert [k for k, _s in new] == ring.segments(0, n, total) and ring.in_use == len(new)
    assert len({s for _k, s in new}) == len(new) and 0 not in {s for _k, s in new}                    # the pad slot is nobody's
    frames_in = {s: ring.frames_of(k) for k, s in new}
    frames_in[0] = [PAD] * 5
    table = ring.table(0, n, total)
    assert table.dtype == np.int32 and table.shape == (n, 8)
    for c in range(n):
        for k in range(8):
            assert frames_in[int(table[c, k])] == idx[c, k].tolist(), (total, c, k)
    assert ring.assign(ring.segments(0, n, total)) == []                                              # nothing is new twice


def test_the_counting_geometry_shares_half_of_every_clip():
    ring = _ring(256)
    assert len(ring.segments(0, 32, 1000)) == 132                          # 32 consecutive clips: 132 segments, not 256
    assert ring.segments(3, 4, 1000) == [(j, 2) for j in range(12, 20)] and ring.segments(4, 5, 1000)[:4] == [(j, 2) for j in range(16, 20)]
    assert ring.segments(5, 5, 1000) == []
    with pytest.raises(ValueError):
        tp.TdnSegmentRing([], 0, 8, 8, 3)


@pytest.mark.parametrize('total', TOTALS)
def test_finality_and_due_clips(total):
    ring = _ring()
    for seen in range(0, total + 1):
        # final: frame centre + 2 exists, so the five frames are what any longer video gives
        final = [j for j in range(60) if 2 * j + 2 <= seen - 1]
        assert ring.n_final(seen) == len(final) and all(ring.is_final(j, seen) == (j in final) for j in range(60))
        now, later = tp.tdn_clip_indices(max(seen, 1), 0, 16, pad=PAD), tp.tdn_clip_indices(seen + 50, 0, 16, pad=PAD)
        for j in final:                                                 # (segment j is segment j % 4 of clip j // 4)
            assert ring.key(j, seen) == ring.key(j, None) == ring.key(j, seen + 50) == (j, 2)
            assert ring.frames_of((j, 2)) == now[j // 4, j % 4].tolist() == later[j // 4, j % 4].tolist()
        # due: 8 c + 16 <= seen - 1
        due = [c for c in range(20) if 8 * c + 16 <= seen - 1]
        assert ring.n_due(seen) == len(due)
        assert all(ring.is_final(4 * c + k, seen) for c in due for k in range(8))
    assert ring.n_clips(total) == _n_clips(total)
    # a segment within two frames of the end is not final: its frames differ from the longer video's
    last = (total - 1) // 2
    if total >= 3:
        assert ring.key(last, total)[1] < 2 and ring.frames_of(ring.key(last, total)) != ring.frames_of((last, 2))


@pytest.mark.parametrize('total', TOTALS)
def test_slot_reuse_never_takes_a_slot_a_due_clip_still_needs(total):
    """A stream of `total` frames walked frame by frame: final segments are assigned as they become final, due clips read their
    table, and a slot goes back only once no later clip reads its segment."""
    ring = _ring(16)
    owner = {}                      # slot -> key, as this test tracks it
    emitted = computed = 0
    peak = 0
    for seen in range(1, total + 1):
        keys = [ring.key(j) for j in range(computed, ring.n_final(seen))]
        computed = ring.n_final(seen)
        for k, s in ring.assign(keys):
            assert s not in owner and s != 0, (seen, s)                 # never a slot somebody still holds
            owner[s] = k
        peak = max(peak, ring.in_use)
        for c in range(emitted, ring.n_due(seen)):
            row = ring.table(c, c + 1)[0]
            assert [owner[int(s)] for s in row] == [(4 * c + k, 2) for k in range(8)]
            emitted = c + 1
            ring.release(emitted)
            for s in [s for s, k in owner.items() if k[0] < 4 * emitted]:
                del owner[s]
            assert sorted(owner) == sorted(ring.slots.values())
            assert all(k[0] >= 4 * emitted for k in ring.slots)        # what the next clip reads is still there
    assert peak <= 8 and ring.in_use <= 7
    # the end: the owed clips with the clamp and the pad segment
    n = _n_clips(total)
    ring.assign(ring.segments(emitted, n, total))
    idx = tp.tdn_clip_indices(total, emitted, n, pad=PAD)
    frames_in = {s: ring.frames_of(k) for k, s in ring.slots.items()}
    frames_in[0] = [PAD] * 5
    for c, row in enumerate(ring.table(emitted, n, total)):
        assert [frames_in[int(s)] for s in row] == idx[c].tolist()
    assert n - emitted <= 2 or total <= 16
    ring.clear()
    assert ring.in_use == 0 and sorted(ring.free) == list(range(1, 16))
    with pytest.raises(IndexError):
        ring.assign([(j, 2) for j in range(16)])
    assert ring.in_use == 0


# ---- TdnStreamBatcher on a stub host model ---------------------------------------------------------------------------------
class Stub:
    """A 'TDN model' on the host (tests/test_tdn_pool_cpu.py's): logits that tell which frames a clip was given."""
    num_class, num_segments, height, width, consensus_type = 3, 8, 32, 32, 'avg'

    def __call__(self, x):
        assert x.dim() == 6 and tuple(x.shape[1:]) == (8, 5, 3, 32, 32), tuple(x.shape)
        centre = torch.stack([c[:, 2].mean() for c in x])
        diff = torch.stack([(c[:, 1:] - c[:, :-1]).abs().mean() for c in x])
        return torch.stack([centre, diff, torch.full_like(centre, 0.1)], dim=1)


def _video(total, h, w, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (total, h, w, 3), dtype=np.uint8))


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_streams_on_a_stub_equal_the_offline_functions(seed):
    tf = TestTransform(36, 32)
    videos = {'a': _video(45, 40, 56, 3), 'b': _video(26, 48, 40, 4)}
    calls = []
    sb = tp.TdnStreamBatcher(Stub(), threshold=0.3, transform=tf, max_batch=3, keep_logits=True,
                             on_window=lambda sid, c, state, count: calls.append((sid, c, state, count)))
    rng = np.random.default_rng(seed)
    at = {k: 0 for k in videos}
    got = {k: [] for k in videos}
    while any(at[k] < len(v) for k, v in videos.items()):
        k = rng.choice([k for k, v in videos.items() if at[k] < len(v)])
        sb.push(k, videos[k][at[k]].numpy())
        at[k] += 1
        if rng.random() < 0.15:
            n_ready = sb.ready()
            res = sb.step()
            assert sum(len(v) for v in res.values()) == n_ready and sb.ready() == 0
            for sid, rows in res.items():
                got[sid] += rows
            # host frames: kept only from the first frame the next clip reads
            for sid, st in sb.streams.items():
                assert st.base == max(0, 8 * st.emitted - 2) or st.seen <= st.base
    for k, v in videos.items():
        want = tp.tdn_video_clip_logits(Stub(), v, tf)
        count, reps = tp.tdn_count_video(Stub(), v, tf, threshold=0.3)
        before = len(got[k])
        assert sb.close(k) == (count, reps)
        rows = sb.logits[k]
        assert [c for c, _r in rows] == list(range(want.shape[0]))
        assert all(np.array_equal(r, want[c].numpy()) for c, r in rows)                      # exactly the offline row
        assert [c for c, _s, _n in got[k]] == list(range(before))
        assert len(rows) - before <= 2                                                       # at most two clips were still owed
    assert not sb.streams and [c for _sid, c, _s, _n in calls if _sid == 'a'] == list(range(6))
    with pytest.raises(ValueError, match='size changed'):
        sb.push('c', np.zeros((8, 8, 3), np.uint8))
        sb.push('c', np.zeros((8, 9, 3), np.uint8))
    with pytest.raises(ValueError, match='uint8'):
        sb.push('d', np.zeros((8, 8, 3), np.float32))


@pytest.mark.parametrize('total', [1, 16, 17])
def test_a_short_stream_closes_like_the_offline_count(total):
    tf = TestTransform(36, 32)
    v = _video(total, 40, 56, total)
    sb = tp.TdnStreamBatcher(Stub(), threshold=0.3, transform=tf, keep_logits=True)
    for f in v:
        sb.push(0, f.numpy())
        sb.step()
    assert sb.close(0) == tp.tdn_count_video(Stub(), v, tf, threshold=0.3)
    want = tp.tdn_video_clip_logits(Stub(), v, tf)
    assert len(sb.logits[0]) == want.shape[0] and all(np.array_equal(r, want[c].numpy()) for c, r in sb.logits[0])
    sb.open(1)
    assert sb.close(1) == (0, [])                                                            # a stream that never got a frame


def test_the_ring_grows_to_what_is_asked_and_keeps_its_contents():
    """The batcher's ring on host tensors: slot 0 is the pad segment's and never free, so 16 slots hold 15 segments."""
    class Shapes(Stub):
        def ring_shapes(self, n):
            return (n, 2, 2, 4), (n, 1, 1, 4)
    sb = tp.TdnStreamBatcher(Shapes(), transform=TestTransform(36, 32))
    sb._dev = 'cpu'
    for need in (15, 16, 256, 3):
        taken = [sb._free.pop() for _ in range(min(2, len(sb._free)))]          # slots somebody holds stay theirs
        if sb._ring_a is not None:
            sb._ring_a[taken] = 7.0
        sb._grow(need)
        assert len(sb._free) >= need and 0 not in sb._free and len(set(sb._free)) == len(sb._free)
        assert not set(taken) & set(sb._free) and max(sb._free) < sb._ring_a.shape[0] == sb._ring_d.shape[0]
        assert sb._free == sorted(sb._free, reverse=True)                          # pop() hands out the lowest slot
        assert bool((sb._ring_a[taken] == 7.0).all()) or not taken
    assert sb._ring_a.shape[0] == 512


def test_refusals_come_before_the_library(monkeypatch):
    from workoutdetector_amd import _lib

    def no_library():
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(_lib, 'load', no_library)
    tf = TestTransform(36, 32)

    class Tdn(Stub):
        tdn_depths = (3, 4, 6, 3)
    with pytest.raises(NotImplementedError, match='person crop'):
        tp.TdnStreamBatcher(Tdn(), transform=PersonCropTransform({}))
    with pytest.raises(NotImplementedError, match='RGB'):
        tp.TdnStreamBatcher(Tdn(), transform=tf, frame_format='nv12')
    m = Tdn()
    m.consensus_type = 'identity'
    with pytest.raises(ValueError, match="consensus_type='avg'"):
        tp.TdnStreamBatcher(m, transform=tf)
    m = Tdn()
    m.width = 64
    with pytest.raises(ValueError, match='squares'):
        tp.TdnStreamBatcher(m, transform=tf)
    with pytest.raises(ValueError, match='crops 24 pixels'):
        tp.TdnStreamBatcher(Tdn(), transform=TestTransform(36, 24))
    with pytest.raises(ValueError, match='max_batch'):
        tp.TdnStreamBatcher(Tdn(), transform=tf, max_batch=0)
    # host models ignore reuse_segments
    v = _video(20, 40, 56, 1)
    assert torch.equal(tp.tdn_video_clip_logits(Stub(), v, tf, reuse_segments=True), tp.tdn_video_clip_logits(Stub(), v, tf))
    # StreamBatcher keeps refusing a TDN engine
    from workoutdetector_amd.streaming import StreamBatcher
    with pytest.raises(NotImplementedError, match='five'):
        StreamBatcher(Tdn())


# ---- ABI -------------------------------------------------------------------------------------------------------------------
HOST_CPP = os.path.join(ROOT, 'tests', 'tdn_ring_host.cpp')


def _build_host(tmp_path):
    exe = str(tmp_path / 'tdn_ring_host')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan',
           '-static-libubsan', '-fno-omit-frame-pointer', '-Wall', '-Wextra', '-Werror', HOST_CPP, '-o', exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    return exe


def test_the_layouts_are_declared_and_bound_without_a_new_export():
    from workoutdetector_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'tsm_hip.h')).read(), flags=re.S)
    assert re.search(r'TSM_LAYOUT_TDN_SEGMENTS = 17\b', text) and _lib.LAYOUT_TDN_SEGMENTS == 17
    assert re.search(r'TSM_LAYOUT_TDN_RING = 18\b', text) and _lib.LAYOUT_TDN_RING == 18
    for name, cls in (('tsm_tdn_segments', _lib.TsmTdnSegments), ('tsm_tdn_ring', _lib.TsmTdnRing)):
        m = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), text, flags=re.S)
        assert re.findall(r'(\w+)\s*[,;]', m.group(1)) == [n for n, _t in cls._fields_], name
    assert ctypes.sizeof(_lib.TsmTdnSegments) == 88 and _lib.TsmTdnSegments.out_a.offset == 72 and _lib.TsmTdnSegments.out_d.offset == 80
    assert ctypes.sizeof(_lib.TsmTdnRing) == 32 and _lib.TsmTdnRing.ring_a.offset == 8 and _lib.TsmTdnRing.table.offset == 24
    assert re.search(r'#define TSM_ABI_VERSION 7\b', open(os.path.join(ROOT, 'include', 'tsm_hip.h')).read()) and _lib.ABI_VERSION == 7
    # no entry point of its own: the exports are what they were
    assert len(_lib.EXPORTS) == 44 and not [e for e in _lib.EXPORTS if 'ring' in e or 'segments' in e and e != 'tsm_head_segments']
    header_fns = set(re.findall(r'\b(tsm_\w+)\s*\(', text))
    assert header_fns == set(_lib.EXPORTS), header_fns ^ set(_lib.EXPORTS)


# ---- host rules ------------------------------------------------------------------------------------------------------------
def test_host_rules_under_sanitizers(tmp_path):
    """tests/tdn_ring_host.cpp built with ASAN + UBSAN (runtimes linked statically: the program runs as it is) and run once; it
    also prints the header's struct sizes, which are ctypes'."""
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    from workoutdetector_amd import _lib
    exe = _build_host(tmp_path)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'runtime error' not in run.stdout + run.stderr and 'tdn_ring_host ok' in run.stdout
    sizes = dict(re.findall(r'sizeof (\w+) = (\d+)', run.stdout))
    assert int(sizes['tsm_tdn_segments']) == ctypes.sizeof(_lib.TsmTdnSegments) and int(sizes['tsm_tdn_ring']) == ctypes.sizeof(_lib.TsmTdnRing)
    assert int(sizes['tsm_tdn_pool']) == ctypes.sizeof(_lib.TsmTdnPool)


def test_the_ring_kernel_uses_no_scratch_and_no_more_registers_than_fuse():
    from workoutdetector_amd import codeobj
    from workoutdetector_amd.build import build_library
    md = codeobj.kernel_metadata(build_library())
    ring, fuse = md['tdn_fuse_ring_kernel'], md['tdn_fuse_kernel']
    assert ring['.private_segment_fixed_size'] == 0 and ring['.vgpr_spill_count'] == 0 and ring['.sgpr_spill_count'] == 0, ring
    assert ring['.group_segment_fixed_size'] == 0
    # the slot lives in scalar registers: about the vector registers of the plain kernel, the same occupancy
    assert ring['.vgpr_count'] <= fuse['.vgpr_count'] + 4 and ring['waves_per_simd'] >= fuse['waves_per_simd'], (ring, fuse)
