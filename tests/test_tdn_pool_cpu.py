"""The host side of the TDN pool input (include/tsm_hip.h: TSM_LAYOUT_TDN_POOL) and of workoutdetector_amd/tdn_pipeline.py,
without a GPU: the frame-number rules against brute force and against the reference's recorded integers, the pipelines with a
stub model, the refusals before the library loads, the host arithmetic under sanitizers, and the new kernel's code object."""
import ctypes
import json
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
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'ref_tdn_sample_indices.json')


# ---- frame numbers ---------------------------------------------------------------------------------------------------------
def _brute_clip_indices(total, lo, hi, T, step, stride, first, pad):
    out = np.empty((hi - lo, T, 5), dtype=np.int64)
    for c in range(lo, hi):
        for k in range(T):
            centre = step * c + stride * k
            for j in range(5):
                out[c - lo, k, j] = pad if centre >= total else min(max(centre - 2 + j, 0), total - 1) - first
    return out


@pytest.mark.parametrize('total', [1, 2, 7, 8, 9, 15, 16, 17, 31, 45])
def test_clip_indices_against_a_loop(total):
    for T, step, stride in ((8, 8, 2), (3, 8, 2), (2, 3, 5), (8, 1, 1)):
        n = (total + step - 1) // step
        for lo, hi in ((0, n), (n // 2, n), (0, n + 1), (n, n + 2)):
            for first in (0, max(0, step * lo - 2), 3):
                got = tp.tdn_clip_indices(total, lo, hi, T, step, stride, first_source_frame=first, pad=-7)
                assert got.dtype == np.int32 and got.shape == (hi - lo, T, 5)
                assert np.array_equal(got, _brute_clip_indices(total, lo, hi, T, step, stride, first, -7)), (total, T, step, lo, hi, first)
    # entries outside a pool of n_frames take the pad too
    got = tp.tdn_clip_indices(45, 0, 6, 8, 8, 2, first_source_frame=10, pad=99, n_frames=20)
    want = _brute_clip_indices(45, 0, 6, 8, 8, 2, 10, 99)
    want[(want < 0) | (want >= 20)] = 99
    assert np.array_equal(got, want) and (got == 99).any() and (got == 0).any() and (got == 19).any()
    with pytest.raises(ValueError):
        tp.tdn_clip_indices(0, 0, 1)
    with pytest.raises(ValueError):
        tp.tdn_clip_indices(10, 2, 1)


def test_clip_0_the_last_frames_and_the_tail_by_hand():
    idx = tp.tdn_clip_indices(45, 0, 6, pad=45)
    assert idx[0, 0].tolist() == [0, 0, 0, 1, 2] and idx[0, 1].tolist() == [0, 1, 2, 3, 4]
    assert idx[5, 1].tolist() == [40, 41, 42, 43, 44] and idx[5, 2].tolist() == [42, 43, 44, 44, 44]       # centres 42 and 44 of 45
    assert (idx[5, 3:] == 45).all()                                                                        # centres 46 ..: the zero frame
    assert tp.tdn_clip_indices(1, 0, 1, pad=1)[0].tolist() == [[0] * 5] + [[1] * 5] * 7
    assert tp.tdn_frame_range(45, 0, 6) == (0, 45) and tp.tdn_frame_range(45, 2, 4) == (14, 41) and tp.tdn_frame_range(300, 3, 5) == (22, 49)


def test_sample_indices_are_the_references_to_the_integer():
    fixture = json.load(open(GOLDEN))
    assert fixture['num_frames'] == 5
    seen = set()
    for c in fixture['cases']:
        got = tp.tdn_sample_indices(c['total'], c['num_segments'], 5, np.random.RandomState(c['seed']))
        assert got.dtype == np.int64 and got.tolist() == c['offsets'], c
        seen.add((c['total'], c['num_segments']))
    assert seen == {(t, T) for t in (3, 5, 8, 9, 11, 12, 13, 40, 300) for T in (8, 3)}
    # all three branches are in the fixture: strided + draw, sorted draws, zeros
    by = {(c['total'], c['num_segments'], c['seed']): c['offsets'] for c in fixture['cases']}
    assert by[(8, 8, 0)] == [0] * 8 and by[(12, 8, 1)] == list(range(8))
    assert any(by[(9, 8, s)] != by[(9, 8, 0)] for s in (1, 2)) and all(sorted(by[(9, 8, s)]) == by[(9, 8, s)] and max(by[(9, 8, s)]) < 5 for s in range(3))
    assert any(by[(300, 8, s)] != by[(300, 8, 0)] for s in (1, 2))


def test_deterministic_sampling_and_the_clamp():
    assert tp.tdn_sample_indices(300).tolist() == [37 * k + 18 for k in range(8)]
    assert tp.tdn_sample_indices(40).tolist() == [4 * k + 2 for k in range(8)]
    assert tp.tdn_sample_indices(12).tolist() == list(range(8))                       # d = 1: d // 2 = 0
    assert tp.tdn_sample_indices(9).tolist() == [int(np.floor((k + 0.5) * 5 / 8)) for k in range(8)]
    assert tp.tdn_sample_indices(11, 8).tolist() == [int(np.floor((k + 0.5) * 7 / 8)) for k in range(8)]
    assert tp.tdn_sample_indices(8).tolist() == [0] * 8 and tp.tdn_sample_indices(3, 3).tolist() == [0] * 3
    assert tp.tdn_sample_indices(40, 3).tolist() == [6, 18, 30]
    for total in (1, 3, 5, 8, 9, 11, 12, 13, 40, 300):
        for T in (8, 3):
            f = tp.tdn_sample_frames(total, T)
            assert f.shape == (T, 5) and f.min() >= 0 and f.max() <= total - 1
            want = np.minimum(tp.tdn_sample_indices(total, T)[:, None] + np.arange(5), total - 1)
            assert np.array_equal(f, want)
    assert tp.tdn_sample_frames(3, 8)[0].tolist() == [0, 1, 2, 2, 2]            # the reference would read img 4 and 5 of 3
    with pytest.raises(ValueError):
        tp.tdn_sample_frames(0)


# ---- the pipelines with a stub model ---------------------------------------------------------------------------------------
class Stub:
    """A 'TDN model' on the host: logits that tell which frames a clip was given.  Class 0 grows with the centre frames' mean,
    class 1 with the mean absolute frame difference, class 2 is a constant."""
    num_class, num_segments, height, width, consensus_type = 3, 8, 32, 32, 'avg'

    def __init__(self, T=8):
        self.num_segments = T
        self.seen = []

    def __call__(self, x):
        assert x.dim() == 6 and tuple(x.shape[1:]) == (self.num_segments, 5, 3, 32, 32), tuple(x.shape)
        self.seen.append(x.clone())
        # (clip by clip: a row's sum must not depend on the batch it came in)
        centre = torch.stack([c[:, 2].mean() for c in x])
        diff = torch.stack([(c[:, 1:] - c[:, :-1]).abs().mean() for c in x])
        return torch.stack([centre, diff, torch.full_like(centre, 0.1)], dim=1)


def _video(total, h=40, w=56, seed=3):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (total, h, w, 3), dtype=np.uint8))


def test_counting_pipeline_with_a_stub():
    video = _video(45)
    tf = TestTransform(36, 32)
    stub = Stub()
    logits = tp.tdn_video_clip_logits(stub, video, tf, batch_clips=4)
    assert tuple(logits.shape) == (6, 3) and logits.dtype == torch.float32 and len(stub.seen) == 2
    # by hand: transform every frame and the zero frame, pick by the rule
    frames = tf(video.permute(0, 3, 1, 2).float())
    zero = tf(torch.zeros(1, 3, 40, 56))
    pool = torch.cat([frames, zero])
    idx = torch.from_numpy(tp.tdn_clip_indices(45, 0, 6, pad=45).astype(np.int64))
    want = Stub()(pool[idx.reshape(-1)].view(6, 8, 5, 3, 32, 32))
    assert torch.equal(logits, want)
    clips = torch.cat(stub.seen)
    assert torch.equal(clips[5, 3:], zero.expand(5 * 5, 3, 32, 32).reshape(5, 5, 3, 32, 32))          # the tail: five zero frames per segment
    # a clip range in mid-video is the same rows; so is any batch size
    assert torch.equal(tp.tdn_video_clip_logits(Stub(), video, tf, clip_range=(2, 5)), logits[2:5])
    assert torch.equal(tp.tdn_video_clip_logits(Stub(), video, tf, batch_clips=1), logits)
    assert tuple(tp.tdn_video_clip_logits(Stub(), video, tf, clip_range=(3, 3)).shape) == (0, 3)
    # the count: the existing states and counter
    from workoutdetector_amd.counting import pred_to_count, scores_to_preds
    count, reps = tp.tdn_count_video(Stub(), video, tf, threshold=0.3)
    assert (count, reps) == pred_to_count(scores_to_preds(logits.numpy(), threshold=0.3), 8)
    # the onnxruntime duck type gets the same clips
    class Session(Stub):
        def get_inputs(self):
            from workoutdetector_amd.engine import NodeArg
            return [NodeArg('input', [None, 8, 5, 3, 32, 32])]

        def run(self, names, feed):
            return [Stub.__call__(self, torch.from_numpy(feed['input'])).numpy()]
    assert torch.equal(tp.tdn_video_clip_logits(Session(), video, tf), logits)


def _samples():
    return [dict(frame_dir='a', start_index=1, total_frames=40, label=0), dict(frame_dir='b', start_index=5, total_frames=9, label=1),
            dict(frame_dir='a', start_index=11, total_frames=13, label=2), dict(frame_dir='a', start_index=30, total_frames=300, label=1)]


class Reader:
    """Frames whose every pixel tells (directory, number): what the pipeline read is what the stub is given."""

    def __init__(self):
        self.calls = []

    def __call__(self, frame_dir, numbers):
        self.calls.append((frame_dir, list(numbers)))
        base = {'a': 0, 'b': 100}[frame_dir]
        out = np.empty((len(numbers), 40, 56, 3), dtype=np.uint8)
        for i, n in enumerate(numbers):
            out[i] = (base + n) % 251
        return out


def test_classification_pipeline_with_a_stub():
    stub, reader = Stub(), Reader()
    tf = TestTransform(36, 32, scale_255=True)
    res = tp.tdn_eval_classification(stub, _samples(), reader, return_logits=True, transform=tf, batch_clips=2)
    assert set(res) == {'correct', 'total', 'acc', 'overall', 'preds', 'logits'}
    assert res['total'] == [1, 2, 1] and len(res['preds']) == 4 and res['logits'].shape == (4, 3)
    assert sum(res['correct']) == sum(int(p == s['label']) for p, s in zip(res['preds'], _samples()))
    assert res['overall'] == sum(res['correct']) / 4
    # every directory read once: the union of its samples' T x 5 numbers, those of the file names (start_index added), the
    # nine-frame segment clamped to its last frame
    assert [d for d, _n in reader.calls] == ['a', 'b']
    want_b = sorted(set((tp.tdn_sample_frames(9) + 5).reshape(-1).tolist()))
    assert reader.calls[1][1] == want_b and max(want_b) == 13
    want_a = sorted(set().union(*[set((tp.tdn_sample_frames(t) + s).reshape(-1).tolist()) for s, t in ((1, 40), (11, 13), (30, 300))]))
    assert reader.calls[0][1] == want_a
    # the logits are those of the sampled frames: class 0 is the mean of the centre frames' transformed pixel value
    for i, s in enumerate(_samples()):
        numbers = tp.tdn_sample_frames(s['total_frames']) + s['start_index']
        pix = torch.from_numpy(reader(s['frame_dir'], numbers.reshape(-1).tolist())).permute(0, 3, 1, 2)
        x = tf(pix.float()).view(1, 8, 5, 3, 32, 32)
        assert np.allclose(res['logits'][i], Stub()(x)[0].numpy(), rtol=1e-6, atol=1e-6), i
    # a RandomState draws in sample order and changes what is read
    drawn = Reader()
    tp.tdn_eval_classification(Stub(), _samples(), drawn, rng=np.random.RandomState(4), transform=tf)
    rng = np.random.RandomState(4)
    rows = [(s['frame_dir'], tp.tdn_sample_frames(s['total_frames'], 8, 5, rng) + s['start_index']) for s in _samples()]
    assert drawn.calls[0][1] == sorted(set().union(*[set(r.reshape(-1).tolist()) for d, r in rows if d == 'a']))
    assert drawn.calls[0][1] != reader.calls[0][1]
    assert tp.tdn_eval_classification(Stub(), [], reader, transform=tf)['overall'] is None


# ---- refusals, all before the library loads --------------------------------------------------------------------------------
def test_refusals_come_before_the_library(monkeypatch):
    from workoutdetector_amd import _lib

    def no_library():
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(_lib, 'load', no_library)
    video, tf = _video(10), TestTransform(36, 32)

    class Tdn(Stub):
        tdn_depths = (3, 4, 6, 3)
    for call in (lambda m, t, **kw: tp.tdn_video_clip_logits(m, video, t, **kw), lambda m, t, **kw: tp.tdn_eval_classification(m, [], transform=t)):
        with pytest.raises(NotImplementedError, match='person crop'):
            call(Tdn(), PersonCropTransform({}))
        m = Tdn()
        m.consensus_type = 'identity'
        with pytest.raises(ValueError, match="consensus_type='avg'"):
            call(m, tf)
        m = Tdn()
        m.width = 64
        with pytest.raises(ValueError, match='squares'):
            call(m, tf)
        with pytest.raises(ValueError, match='crops 24 pixels'):
            call(Tdn(), TestTransform(36, 24))
        with pytest.raises(ValueError, match='TestTransform'):
            call(Tdn(), lambda x: x)
    with pytest.raises(NotImplementedError, match='RGB'):
        tp.tdn_video_clip_logits(Tdn(), video, tf, frame_format='nv12')
    with pytest.raises(ValueError, match='uint8'):
        tp.tdn_video_clip_logits(Tdn(), video.float(), tf)
    with pytest.raises(ValueError, match='batch_clips'):
        tp.tdn_video_clip_logits(Tdn(), video, tf, batch_clips=0)
    # the existing pipelines keep refusing a TDN engine
    from workoutdetector_amd import inference_count
    with pytest.raises(NotImplementedError, match='five'):
        inference_count.need_clip_rows(Tdn(), 'inference_dataset')


def test_pieces_fit_the_staging_bound(monkeypatch):
    from workoutdetector_amd import inference_count as ic
    per = 360 * 640 * 3
    n = tp.tdn_clips_per_piece(per)
    assert n == ic.PIECE_CLIPS                                           # 1 GiB holds far more: the float pool's bound holds
    monkeypatch.setattr(ic, 'MAX_STAGE_BYTES', 60 * per)
    n = tp.tdn_clips_per_piece(per)
    a, b = tp.tdn_frame_range(10 ** 6, 7, 7 + n)
    assert (b - a + 1) * per <= 60 * per < (tp.tdn_frame_range(10 ** 6, 7, 8 + n)[1] - a + 1) * per and n == 6
    monkeypatch.setattr(ic, 'MAX_STAGE_BYTES', per)
    assert tp.tdn_clips_per_piece(per) == 1


# ---- ABI -------------------------------------------------------------------------------------------------------------------
def test_the_layout_is_declared_and_bound_without_a_new_export():
    from workoutdetector_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'tsm_hip.h')).read(), flags=re.S)
    assert re.search(r'TSM_LAYOUT_TDN_POOL = 16\b', text) and _lib.LAYOUT_TDN_POOL == 16
    m = re.search(r'typedef struct tsm_tdn_pool \{(.*?)\} tsm_tdn_pool;', text, flags=re.S)
    names = re.findall(r'(\w+)\s*[,;]', m.group(1))
    assert names == [n for n, _t in _lib.TsmTdnPool._fields_], names
    assert ctypes.sizeof(_lib.TsmTdnPool) == 72 and _lib.TsmTdnPool.pad_frame.offset == 64 and _lib.TsmTdnPool.frames.offset == 8
    assert re.search(r'#define TSM_ABI_VERSION 7\b', open(os.path.join(ROOT, 'include', 'tsm_hip.h')).read()) and _lib.ABI_VERSION == 7
    assert not [e for e in _lib.EXPORTS if 'tdn_pool' in e or 'forward_pool' in e]      # no entry point of its own


# ---- code object -----------------------------------------------------------------------------------------------------------
def test_the_pool_kernel_uses_no_scratch_and_the_plain_kernels_budget():
    from workoutdetector_amd import codeobj
    from workoutdetector_amd.build import build_library
    md = codeobj.kernel_metadata(build_library())
    pool, plain = md['tdn_front_pool_kernel'], md['tdn_front_kernel']
    assert pool['.private_segment_fixed_size'] == 0 and pool['.vgpr_spill_count'] == 0 and pool['.sgpr_spill_count'] == 0, pool
    assert pool['.group_segment_fixed_size'] == plain['.group_segment_fixed_size'] == 21 * 21 * 12 * 4
    # the frame numbers live in scalar registers: no more vector registers than the plain kernel, the same occupancy
    assert pool['.vgpr_count'] <= plain['.vgpr_count'] and pool['waves_per_simd'] >= plain['waves_per_simd'], (pool, plain)
    # 74: the plain kernel's count at commit 2cac9cf, read from a build with these flags -- the two kernels are copies kept
    # identical by hand, and a shared inlined body has cost the plain kernel 24 registers (DESIGN_HISTORY.md H7)
    assert plain['.vgpr_count'] <= 74, plain


# ---- host arithmetic -------------------------------------------------------------------------------------------------------
def test_host_arithmetic_under_sanitizers(tmp_path):
    """tests/tdn_pool_host.cpp built with ASAN + UBSAN (runtimes linked statically: the program runs as it is) and run once."""
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path / 'tdn_pool_host')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan',
           '-static-libubsan', '-fno-omit-frame-pointer', '-Wall', '-Wextra', '-Werror', os.path.join(ROOT, 'tests', 'tdn_pool_host.cpp'),
           '-o', exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'runtime error' not in run.stdout + run.stderr and 'tdn_pool_host ok' in run.stdout


def test_the_host_rule_is_the_numpy_rule(tmp_path):
    """tdn_window_frame (C, what the kernel runs) against tdn_clip_indices (NumPy, what the host path gathers by): a small
    program prints the C function's table for the counting geometry."""
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    src = tmp_path / 'rule.cpp'
    src.write_text('#include <cstdio>\n#include "%s"\n'
                   'int main() { for (long total : {1L, 9L, 45L, 47L}) for (long c = 0; c < 7; ++c) for (int k = 0; k < 8; ++k) for (int j = 0; j < 5; ++j)\n'
                   '  std::printf("%%ld\\n", (long)tsm_host::tdn_window_frame(6, total, c, k, j, 8, 2, 30, 29)); return 0; }\n'
                   % os.path.join(ROOT, 'workoutdetector_amd', 'csrc', 'tsm_host_util.h'))
    exe = str(tmp_path / 'rule')
    build = subprocess.run(['g++', '-std=c++17', '-O1', str(src), '-o', exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    got = np.array(subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split(), dtype=np.int64).reshape(4, 7, 8, 5)
    for i, total in enumerate((1, 9, 45, 47)):
        assert np.array_equal(got[i], tp.tdn_clip_indices(total, 0, 7, 8, 8, 2, first_source_frame=6, pad=29, n_frames=30)), total
