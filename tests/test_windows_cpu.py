"""tsm_preprocess_windows without a GPU: the ABI declaration, the kernel's integer geometry and descriptor validity under
ASAN + UBSAN (tests/windows_host.cpp, a stand-alone program: the functions the kernel inlines, on the CPU first), the entry
point's host-side refusals, the descriptor builder, and StreamBatcher(person_crop=True) on the duck-typed host path."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests._stub import StubModel, synthetic_video

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_library_and_binding_carry_tsm_preprocess_windows():
    from workoutdetector_amd import _lib
    from workoutdetector_amd.build import LIB_PATH, build_library
    build_library()
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'tsm_hip.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+tsm_preprocess_windows\s*\(', text)
    assert re.search(r'#define\s+TSM_ABI_VERSION\s+7\b', text)
    out = subprocess.run(['nm', '-D', '--defined-only', LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r' T tsm_preprocess_windows\b', out)
    assert 'tsm_preprocess_windows' in _lib.EXPORTS
    # nm -D shows exactly the header's symbols
    declared = set(re.findall(r'\b(tsm_\w+)\s*\(', text))
    exported = set(re.findall(r' T (tsm_\w+)\b', out))
    assert exported == declared == set(_lib.EXPORTS), (exported ^ declared, declared ^ set(_lib.EXPORTS))
    lib = _lib.load()
    assert lib.tsm_abi_version() == _lib.ABI_VERSION == 7
    assert len(lib.tsm_preprocess_windows.argtypes) == 13


@pytest.fixture(scope='module')
def host_program(tmp_path_factory):
    """tests/windows_host.cpp built with ASAN + UBSAN (runtimes linked statically: the program runs as it is, whatever else
    the environment loads) and run once; returns (stdout, the geometry records int32 [n, 8])."""
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    tmp = tmp_path_factory.mktemp('windows_host')
    exe, dump = str(tmp / 'windows_host'), str(tmp / 'geometry.bin')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan',
           '-static-libubsan', '-fno-omit-frame-pointer', '-Wall', '-Wextra', '-Werror', os.path.join(ROOT, 'tests', 'windows_host.cpp'),
           '-o', exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    run = subprocess.run([exe, dump], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'runtime error' not in run.stdout + run.stderr
    return run.stdout, np.fromfile(dump, dtype=np.int32).reshape(-1, 8)


def test_integer_geometry_equals_the_host_rule_and_the_python_transform(host_program):
    """In the program: center_crop_geometry_int == center_crop_geometry for h, w in 1 .. 300 and the sides {1, 2, 255, 256,
    257, 32767, 65535} crossed, four (resize, crop) pairs.  Here: the same records equal transform.resized_hw / crop_offsets."""
    from workoutdetector_amd.transform import crop_offsets, resized_hw
    stdout, rec = host_program
    assert 'windows host ok' in stdout
    assert rec.shape[0] == 4 * (300 * 300 + 7 * 7)
    assert {(int(r), int(c)) for r, c in np.unique(rec[:, 2:4], axis=0)} == {(256, 224), (36, 32), (36, 33), (8, 8)}
    for h, w, resize, crop, nh, nw, top, left in rec.tolist():
        got = resized_hw(h, w, resize)
        assert got == (nh, nw) and crop_offsets(nh, nw, crop) == (top, left), (h, w, resize, crop)


def test_descriptor_validity_verdicts_under_the_sanitizers(host_program):
    """INT32_MIN / INT32_MAX / 0 in every word, offsets -16, arena_bytes, arena_bytes - bytes + 1, INT64_MAX, an unaligned
    offset, sides of 65536, n_segment * frame bytes past int64, 200 000 random descriptors against a 128-bit restatement of
    the rule: every verdict right (the program counts failures) and UBSAN silent (-fno-sanitize-recover: it would abort)."""
    stdout, _ = host_program
    assert 'FAIL' not in stdout and stdout.strip().endswith('windows host ok')


def test_invalid_arguments_are_refused_before_anything_touches_a_gpu():
    """Each host-side refusal of include/tsm_hip.h: TSM_ERR_INVALID_ARG and an empty launch trace.  The pointers are never
    dereferenced on the host and nothing is launched, so made-up addresses serve."""
    from workoutdetector_amd import _lib
    from workoutdetector_amd.build import build_library
    from workoutdetector_amd.engine import launch_trace
    build_library()
    lib = _lib.load()
    good = dict(arena=0x10000, arena_bytes=1 << 20, pixel=_lib.PIXEL_U8, desc=0x20000, n_windows=2, n_segment=8, person_crop=0,
                out=0x30000, out_layout=_lib.LAYOUT_NTHWC4, resize=256, crop=224, scale_255=0, stream=None)
    bad = [dict(arena=None), dict(desc=None), dict(out=None), dict(arena=0x10008), dict(desc=0x20004), dict(arena_bytes=0),
           dict(arena_bytes=-16), dict(n_windows=0), dict(n_windows=-1), dict(n_segment=0), dict(resize=0), dict(crop=0),
           dict(crop=-224), dict(pixel=2), dict(pixel=-1), dict(out_layout=_lib.LAYOUT_NTHWC), dict(out_layout=9),
           dict(person_crop=2), dict(person_crop=-1), dict(resize=224, crop=225), dict(resize=36, crop=37, person_crop=0)]
    for change in bad:
        args = dict(good, **change)
        with launch_trace() as tr:
            rc = lib.tsm_preprocess_windows(*args.values())
        assert rc == -1, change
        assert tr.kernels == [], (change, tr.kernels)
        assert b'preprocess_windows' in lib.tsm_last_error(None) or 'pixel' in change or 'out_layout' in change, change


def test_window_descriptors_layout_and_refusals():
    from workoutdetector_amd.transform import window_descriptors
    d = window_descriptors([(40, 56), (56, 40, 3), (36, 36)], [0, 53760, (1 << 32) + 16], resize=36, crop=33)
    assert d.dtype == np.int32 and d.shape == (3, 8)
    assert d.tolist() == [[0, 0, 40, 56, 0, 0, 0, 0], [53760, 0, 56, 40, 0, 0, 0, 0], [16, 1, 36, 36, 0, 0, 0, 0]]
    # off_lo is the low dword as an int32: bit 31 makes it negative
    assert window_descriptors([(8, 8)], [(1 << 31) + 32]).tolist() == [[-(1 << 31) + 32, 0, 8, 8, 0, 0, 0, 0]]
    assert window_descriptors([(8, 8)], [(5 << 32) + 0xFFFFFFF0])[0, :2].tolist() == [-16, 5]
    # boxes: (top, left, h, w) as they are, None = the all-zero "no person" row; no centre-crop check in this mode
    d = window_descriptors([(40, 56), (8, 8)], [0, 64], boxes=[(-6, -9, 25, 30), None], resize=8, crop=224)
    assert d.tolist() == [[0, 0, 40, 56, -6, -9, 25, 30], [64, 0, 8, 8, 0, 0, 0, 0]]
    assert window_descriptors([(4, 4)], [0], boxes=[(-2 ** 31, 2 ** 31 - 1, 0, -1)])[0, 4:].tolist() == [-2 ** 31, 2 ** 31 - 1, 0, -1]
    assert window_descriptors([], []).shape == (0, 8)
    for kw in (dict(shapes=[(0, 8)], offsets=[0]), dict(shapes=[(8, 65536)], offsets=[0]), dict(shapes=[(8, 8, 4)], offsets=[0]),
               dict(shapes=[(8,)], offsets=[0]), dict(shapes=[(8.0, 8)], offsets=[0]), dict(shapes=[(8, 8)], offsets=[-16]),
               dict(shapes=[(8, 8)], offsets=[8]), dict(shapes=[(8, 8)], offsets=[16.0]), dict(shapes=[(8, 8)], offsets=[1 << 63]),
               dict(shapes=[(8, 8)], offsets=[0, 16]), dict(shapes=[(8, 8)], offsets=[0], boxes=[]),
               dict(shapes=[(40, 56)], offsets=[0], resize=32, crop=36),            # a centre crop larger than the resized frame
               dict(shapes=[(8, 8)], offsets=[0], boxes=[(1, 2, 3)]), dict(shapes=[(8, 8)], offsets=[0], boxes=[(1, 2, 3, 4.5)]),
               dict(shapes=[(8, 8)], offsets=[0], boxes=[(1, 2, 3, 2 ** 31)])):
        with pytest.raises(ValueError):
            window_descriptors(**kw)


# ---- StreamBatcher(person_crop=True) on the duck-typed host path -------------------------------------------------------------
def _detector(sid, t, h, w):
    """A made-up detector: (x1, y1, x2, y2) of frame t, or None.  Stream 'b' has a window without any box (frames 8 .. 15), one
    with boxes on two frames only (16 .. 23) and one whose union has no area (24 .. 31)."""
    if sid == 'b':
        if 8 <= t < 16 or (16 <= t < 24 and t not in (17, 22)):
            return None
        if 24 <= t < 32:
            return (5.0, 3.0, 5.0, 20.0)
    cx, cy = w * (0.5 + 0.3 * np.sin(t / 5.0)), h * (0.5 + 0.2 * np.cos(t / 7.0))
    return (cx - 0.3 * w, cy - 0.35 * h, cx + 0.25 * w + t % 3, cy + 0.3 * h)


def test_stream_batcher_person_crop_equals_a_per_window_loop_on_the_host_path():
    """States and counts equal a per-window PersonCropTransform + model loop; a window's box is person_box of the boxes pushed
    with its frames; a window without boxes (and one whose union is empty) uses the whole frame; a box without
    person_crop=True is refused."""
    from workoutdetector_amd.counting import RepCounter, scores_to_preds
    from workoutdetector_amd.streaming import StreamBatcher
    from workoutdetector_amd.transform import PersonCropTransform, person_box
    vids = {'a': synthetic_video(1, 90, 45, 26, period=16), 'b': synthetic_video(2, 61, 30, 40, period=20)}
    model = StubModel(gain=8.0)
    sb = StreamBatcher(model, max_batch=3, person_crop=True)
    events = {k: [] for k in vids}
    queued = {k: [] for k in vids}
    for t in range(90):
        for k, v in vids.items():
            if t < len(v):
                sb.push(k, v[t], box=_detector(k, t, *v.shape[1:3]))
                if t % 8 == 7:
                    queued[k].append(sb.streams[k].crops[-1])
        if t % 10 == 9:
            for k, ev in sb.step().items():
                events[k] += ev
    for k, ev in sb.step().items():
        events[k] += ev
    assert sb.ready() == 0 and model.calls < sum(len(v) // 8 for v in vids.values())
    tf = PersonCropTransform({}, size=224)
    ref = StubModel(gain=8.0)
    for k, v in vids.items():
        counter, want = RepCounter(8), []
        for i in range(len(v) // 8):
            boxes = [b for b in (_detector(k, t, *v.shape[1:3]) for t in range(8 * i, 8 * i + 8)) if b is not None]
            box = person_box(boxes) if boxes else None
            assert queued[k][i] == box, (k, i)
            x = tf(torch.from_numpy(v[8 * i: 8 * i + 8]).permute(0, 3, 1, 2).float(), box)
            state = scores_to_preds(ref.run(None, {'input': x[None].numpy()})[0].tolist())[0]
            want.append((i, state, counter.push(state)))
        assert events[k] == want, k
        assert sb.result(k) == (counter.count, list(counter.reps))
    assert queued['b'][1] is None and queued['b'][3] is None and queued['b'][2] == person_box(
        [_detector('b', 17, 30, 40), _detector('b', 22, 30, 40)])
    assert queued['a'][0] is not None and len(set(events['a'][i][1] for i in range(len(events['a'])))) > 1
    # the crop changes what the model sees: the same frames without boxes give other logits for a cropped window
    whole = tf(torch.from_numpy(vids['a'][:8]).permute(0, 3, 1, 2).float(), None)
    assert not torch.equal(whole, tf(torch.from_numpy(vids['a'][:8]).permute(0, 3, 1, 2).float(), queued['a'][0]))
    # refusals
    with pytest.raises(ValueError):
        StreamBatcher(StubModel()).push('x', vids['a'][0], box=(1, 2, 3, 4))
    with pytest.raises(ValueError):
        sb.push('a', vids['a'][0], box=(1, 2, 3))
    with pytest.raises(ValueError):
        sb.push('a', vids['a'][0], box=(1, 2, float('nan'), 4))
    # the default mode is what it was: no boxes, the centre-crop transform
    plain, base = StreamBatcher(StubModel(gain=8.0), max_batch=3), StubModel(gain=8.0)
    for t in range(16):
        plain.push('a', vids['a'][t])
    got = plain.step()['a']
    x = torch.stack([plain.transform(torch.from_numpy(vids['a'][8 * i: 8 * i + 8]).permute(0, 3, 1, 2).float()) for i in range(2)])
    assert [s for _, s, _ in got] == scores_to_preds(base.run(None, {'input': x.numpy()})[0].tolist())
