"""tsm_preprocess_clips (gather + person crop + resize + normalise + pack in one launch) against the torch composition of
tests/_person_crop.py run on the CPU, and the person_crop=True dataset path on a real engine.

Every launch runs in hostile memory (tests/_guard.py): frames and boxes between poisoned bands, the output poisoned before
the launch, bands and payload checked after it.  Tolerance: the project's preprocess bound, |err| <= 1e-5 |want| + 5e-4
(tests/test_preprocess_gpu.py::_check).  Shapes: 40 x 56 and 57 x 33 frames (an odd width, h > w), 27 frames = 4 clips of
which the last two end in padded tail segments, sizes 32 and 33 (33: a pixel-pair tail column in the bf16 layouts).
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import _person_crop as pc
from tests._guard import POISON, check, guarded, guarded_out
from tests._stub import synthetic_video

pytestmark = pytest.mark.gpu

TOTAL = 27                      # frames: clips start at 0, 8, 16, 24; clip 2 has 6 real segments, clip 3 has 2
N_CLIPS = 4
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def _check(got, want, what):
    got, want = got.double(), want.double()
    err = (got - want).abs()
    bound = 1e-5 * want.abs() + 5e-4
    print(f'{what}: max err {float(err.max()):.3g}, max err / bound {float((err / bound).max()):.3g}')
    assert bool((err <= bound).all()), f'{what}: max err {float(err.max()):.3g}'


def _rows(boxes):
    return torch.tensor([b or (0, 0, 0, 0) for b in boxes], dtype=torch.int32).reshape(len(boxes), 4)


def _shape(layout, n, size):
    from workoutdetector_amd.engine import _frame_shape
    return (n, 8) + _frame_shape(layout, size)


def _launch(even, boxes, size, layout, first_frame=0, first_clip=0, total=TOTAL, **kw):
    """engine.preprocess_clips in hostile memory; `even`: the staged even frames (CPU tensor), `boxes`: tuples / None."""
    from workoutdetector_amd.engine import preprocess_clips
    src = guarded(even.cuda(), name='frames')
    rows = guarded(_rows(boxes).cuda(), name='boxes')
    out = guarded_out(_shape(layout, len(boxes), size), name='out')
    assert preprocess_clips(src, rows, first_frame, total, first_clip, len(boxes), size=size, layout=layout, out=out, **kw) is out
    torch.cuda.synchronize()
    check(src, rows, out)
    return out.cpu()


def _groups(boxes, n=N_CLIPS):
    """The box kinds in launches of n clips (the last one filled up from the front), so that every kind meets the kernel."""
    boxes = list(boxes)
    return [tuple((boxes + boxes)[i:i + n]) for i in range(0, len(boxes), n)]


@pytest.mark.parametrize('layout_name', ['nthwc4', 'ntchw', 'nthwc8s', 'nthwc8b'])
@pytest.mark.parametrize('size', [32, 33])
@pytest.mark.parametrize('h,w', [(40, 56), (57, 33)])
def test_preprocess_clips_matches_the_torch_composition(hip_lib, h, w, size, layout_name):
    """Every box kind x every clip position (real segments and padded tails), uint8 and float sources, scale_255 on and off.
    fp32 layouts against the CPU reference under the preprocess bound, pad channel exactly 0; the pixel-pair layouts against
    the fp32 output of the same kernel: bf16 = RNE of it, split hi = the same and hi + lo within 2^-16, pad channel and the
    odd pixel of an odd size exactly 0."""
    from workoutdetector_amd import _lib
    layout = {'nthwc4': _lib.LAYOUT_NTHWC4, 'ntchw': _lib.LAYOUT_NTCHW, 'nthwc8s': _lib.LAYOUT_NTHWC8S,
              'nthwc8b': _lib.LAYOUT_NTHWC8B}[layout_name]
    seed = h * w
    even = pc.video(seed, TOTAL, h, w)[0::2].contiguous()             # 14 even frames, no pad frame
    pairs = (size + 1) // 2
    for boxes in _groups(pc.boxes_for(h, w, size)):
        for f32_src, scale_255 in [(False, False), (True, True), (False, True), (True, False)]:
            what = f'{h}x{w} -> {size} {layout_name} {"f32" if f32_src else "u8"} scale_255={scale_255} boxes {boxes}'
            src = even.float() if f32_src else even
            want = pc.clip_reference(seed, TOTAL, h, w, boxes, size, scale_255)           # [4,8,3,size,size]
            got = _launch(src, boxes, size, layout, scale_255=scale_255)
            if layout == _lib.LAYOUT_NTCHW:
                _check(got, want, what)
                continue
            if layout == _lib.LAYOUT_NTHWC4:
                assert float(got[..., 3].abs().max()) == 0.0, what
                _check(got[..., :3].permute(0, 1, 4, 2, 3), want, what)
                continue
            nchw = _launch(src, boxes, size, _lib.LAYOUT_NTCHW, scale_255=scale_255)
            _check(nchw, want, what + ' (its fp32 form)')
            f32 = nchw.permute(0, 1, 3, 4, 2)                                             # [4,8,size,size,3]
            if layout == _lib.LAYOUT_NTHWC8B:
                px = got.view(torch.bfloat16).reshape(N_CLIPS, 8, size, pairs * 2, 4).float()
                val = hi = px
            else:
                g = got.view(torch.bfloat16).reshape(N_CLIPS, 8, size, pairs, 2, 8).float()   # [hi x8 | lo x8] per pair
                hi = g[..., 0, :].reshape(N_CLIPS, 8, size, pairs * 2, 4)
                val = (g[..., 0, :] + g[..., 1, :]).reshape(N_CLIPS, 8, size, pairs * 2, 4)
            assert torch.equal(hi[..., :size, :3], f32.to(torch.bfloat16).float()), what
            if layout == _lib.LAYOUT_NTHWC8S:
                assert bool(((val[..., :size, :3] - f32).abs() <= f32.abs() * 2.0 ** -16 + 1e-30).all()), what
            assert float(val[..., 3].abs().max()) == 0.0, what
            if size % 2:
                assert float(val[..., size:, :].abs().max()) == 0.0, what


def test_padded_tail_is_exactly_the_normalised_zero_and_reads_nothing(hip_lib):
    """The tail segments of clips 2 and 3 equal (0 - mean) / std to the bit in every layout's fp32 form.  The buffer holds
    the 14 even frames and NO zero frame: behind the last frame lies the guard band."""
    from workoutdetector_amd import _lib
    h, w, size = 40, 56, 33
    even = pc.video(7, TOTAL, h, w)[0::2].contiguous()
    boxes = ((5, 7, 20, 17), None, (-6, -9, 25, 30), (h - 12, w - 10, 30, 27))
    for scale_255 in (False, True):
        got = _launch(even, boxes, size, _lib.LAYOUT_NTCHW, scale_255=scale_255)
        zero = pc.ZERO.view(1, 3, 1, 1).expand(1, 3, size, size)
        assert torch.equal(got[2, 6:], zero.expand(2, 3, size, size))
        assert torch.equal(got[3, 2:], zero.expand(6, 3, size, size))
        assert not torch.equal(got[2, 5], zero[0]) and not torch.equal(got[3, 1], zero[0])
        packed = _launch(even, boxes, size, _lib.LAYOUT_NTHWC4, scale_255=scale_255)
        assert torch.equal(packed[..., :3].permute(0, 1, 4, 2, 3), got)


@pytest.mark.parametrize('size', [16, 17])
def test_whole_frame_boxes_equal_the_gathered_centre_crop_bit_for_bit(hip_lib, size):
    """The two samplers share one core.  On square frames Resize((size, size)) of the whole frame and Resize(size) +
    CenterCrop(size) are the same map, so preprocess_clips with every box "no person" equals gather_clips(preprocess_frames(
    resize=size, crop=size)) bit for bit: all four layouts, uint8 and float32 sources, scale_255 on and off.  24 x 24 frames,
    14 staged even frames, 4 clips of which the last two end in the padded tail: preprocess_clips writes the normalised zero
    frame there, the other route transforms a staged raw zero frame and gathers it as the pad frame.  Size 17 ends every row in a
    half-filled pixel pair.  (An NTCHW frame of 17 x 17 is 3468 bytes, no multiple of gather_clips' 16: those clips are picked
    with torch from the same transformed frames.)"""
    from workoutdetector_amd import _lib
    from workoutdetector_amd.engine import _frame_shape, gather_clips, preprocess_frames
    even = pc.video(size, TOTAL, 24, 24)[0::2].contiguous()
    staged = torch.cat([even, torch.zeros_like(even[:1])])                    # ... + the pad frame, raw zeros
    pick = torch.tensor([[min(4 * c + k, 14) for k in range(8)] for c in range(N_CLIPS)])    # even frame of (clip, segment)
    for layout in (_lib.LAYOUT_NTHWC4, _lib.LAYOUT_NTCHW, _lib.LAYOUT_NTHWC8S, _lib.LAYOUT_NTHWC8B):
        for f32_src, scale_255 in [(False, False), (True, True), (False, True), (True, False)]:
            what = f'24x24 -> {size} layout {layout} {"f32" if f32_src else "u8"} scale_255={scale_255}'
            fused = _launch(even.float() if f32_src else even, (None,) * N_CLIPS, size, layout, scale_255=scale_255)
            src = guarded((staged.float() if f32_src else staged).cuda(), name='frames')
            frames = guarded_out((15,) + _frame_shape(layout, size), name='transformed')
            preprocess_frames(src, resize=size, crop=size, scale_255=scale_255, layout=layout, out=frames)
            if frames[0].numel() * 4 % 16 == 0:
                clips = guarded_out(_shape(layout, N_CLIPS, size), name='clips')
                gather_clips(frames, 0, TOTAL, 0, N_CLIPS, out=clips)
            else:
                clips = None
            torch.cuda.synchronize()
            check(src, frames, clips)
            want = clips.cpu() if clips is not None else frames.cpu()[pick]
            assert torch.equal(fused.view(torch.int32), want.view(torch.int32)), what
            assert not torch.equal(want[2, 5], want[2, 6]) and torch.equal(want[2, 6], want[3, 7]), what     # real / tail rows


@pytest.mark.parametrize('layout_name', ['nthwc4', 'nthwc8s'])
def test_a_sub_range_staged_alone_equals_the_rows_of_the_full_range(hip_lib, layout_name):
    """first_frame > 0 / first_clip > 0: clips 1 .. 3 from a buffer that starts at their first even frame, and clip 3 alone,
    bit for bit the rows of the whole video's launch."""
    from workoutdetector_amd import _lib
    layout = {'nthwc4': _lib.LAYOUT_NTHWC4, 'nthwc8s': _lib.LAYOUT_NTHWC8S}[layout_name]
    h, w, size = 57, 33, 33
    even = pc.video(11, TOTAL, h, w)[0::2].contiguous()
    boxes = ((5, 7, 20, 17), (-6, -9, 25, 30), (h - 12, w - 10, 30, 27), (3, -4, h - 5, w + 11))
    full = _launch(even, boxes, size, layout)
    for lo, hi in [(1, 3), (3, 4), (2, 4)]:
        f_lo = 8 * lo // 2
        f_hi = min((8 * (hi - 1) + 16) // 2, (TOTAL + 1) // 2)
        part = _launch(even[f_lo:f_hi].contiguous(), boxes[lo:hi], size, layout, first_frame=f_lo, first_clip=lo)
        assert torch.equal(part, full[lo:hi]), (lo, hi)


def test_extreme_boxes_give_a_defined_output_and_read_nothing_outside(hip_lib):
    """The kernel is total in the boxes (they live in device memory, no host check sees them): +-2^30 offsets, INT32_MIN /
    INT32_MAX sides.  Each has a defined result -- everything outside the frame, or "no person" = the whole frame -- and
    the bands around frames, boxes and output stay intact.  The documented behaviour, exercised; not an attempt to fault."""
    from workoutdetector_amd import _lib
    h, w, size = 40, 56, 32
    seed = 13
    even = pc.video(seed, TOTAL, h, w)[0::2].contiguous()
    outside = [(2 ** 30, 2 ** 30, 10, 10), (-2 ** 30, -2 ** 30, 5, 5), (I32_MAX, I32_MAX, I32_MAX, I32_MAX),
               (I32_MIN, I32_MIN, 7, 7), (-2 ** 30, -2 ** 30, I32_MAX, I32_MAX), (I32_MIN, 3, I32_MAX, 9),
               (3, I32_MAX, 9, I32_MAX), (I32_MAX - 3, 0, 8, 8)]
    whole = [(5, 5, I32_MIN, I32_MIN), (I32_MAX, I32_MIN, 0, I32_MAX), (I32_MIN, I32_MAX, I32_MAX, -1), (0, 0, I32_MIN, 4)]
    want_whole = pc.clip_reference(seed, TOTAL, h, w, (None,) * N_CLIPS, size, False)
    zero = pc.ZERO.view(1, 1, 3, 1, 1).expand(1, 8, 3, size, size)
    for layout in (_lib.LAYOUT_NTCHW, _lib.LAYOUT_NTHWC8B):
        for boxes in _groups(outside) + _groups(whole):
            got = _launch(even, boxes, size, layout)
            if layout != _lib.LAYOUT_NTCHW:
                continue                        # (the packed launch: bands and payload only, by _launch)
            for c, box in enumerate(boxes):
                if box in whole:
                    _check(got[c], want_whole[c], f'whole frame {box}')
                else:
                    assert torch.equal(got[c:c + 1], zero), box
    # a box that leaves int32 only in the SUM: top + y crosses 2^31 inside the box
    got = _launch(even, ((I32_MAX - 3, 0, 8, 8),) * N_CLIPS, size, _lib.LAYOUT_NTCHW, scale_255=True)
    assert torch.equal(got, zero.expand(N_CLIPS, 8, 3, size, size))


def test_host_validation_refuses_before_any_launch(hip_lib):
    """clip_step % clip_stride != 0, a clip that starts past the video, a range that reads outside the buffer, a buffer that
    starts behind the range's first frame: TSM_ERR_INVALID_ARG, the output still all poison, and the launch trace empty."""
    from workoutdetector_amd import _lib
    from workoutdetector_amd.engine import launch_trace, preprocess_clips
    h, w, size = 40, 56, 32
    even = guarded(pc.video(3, TOTAL, h, w)[0::2].contiguous().cuda(), name='frames')           # 14 frames
    rows = guarded(_rows([(5, 7, 20, 17)] * N_CLIPS).cuda(), name='boxes')
    cases = [dict(first_frame=0, total_frames=TOTAL, first_clip=0, n_clips=4, clip_step=8, clip_stride=3),
             dict(first_frame=0, total_frames=TOTAL, first_clip=4, n_clips=1),                    # clip 4 starts at frame 32 > 26
             dict(first_frame=0, total_frames=24, first_clip=3, n_clips=1),                      # ... at frame 24 = the end
             dict(first_frame=0, total_frames=77, first_clip=0, n_clips=4),                      # needs 20 even frames, 14 staged
             dict(first_frame=4, total_frames=TOTAL, first_clip=0, n_clips=4),                   # clip 0 lies before the buffer
             dict(first_frame=0, total_frames=0, first_clip=0, n_clips=4)]
    for kw in cases:
        n = kw['n_clips']
        out = guarded_out(_shape(_lib.LAYOUT_NTHWC4, n, size), name='out')
        with launch_trace() as tr:
            with pytest.raises(_lib.TsmError) as ei:
                preprocess_clips(even, rows[:n], size=size, out=out, **kw)
        assert ei.value.status == -1, kw
        assert tr.kernels == [], (kw, tr.kernels)
        torch.cuda.synchronize()
        assert bool((out.view(torch.int32) == POISON).all()), kw
        check(even, rows)
    # the binding's own refusals: boxes of another dtype / shape / device never reach the C ABI
    for bad in (rows.float(), rows[:3], rows.cpu()):
        with pytest.raises(ValueError):
            preprocess_clips(even, bad, 0, TOTAL, 0, N_CLIPS, size=size)
    # ... and the same call with good arguments launches exactly one kernel
    with launch_trace() as tr:
        preprocess_clips(even, rows, 0, TOTAL, 0, N_CLIPS, size=size)
    assert len(tr.kernels) == 1 and tr.ran('preprocess_clips_kernel<unsigned char>'), tr.kernels


# ---- the dataset path on a real engine ----------------------------------------------------------------------------------
VIDEOS = {'stu1_40.npy': (27, 48, 36), 'stu5_32.npy': (41, 36, 52)}           # frames, h, w: 4 and 6 clips
BOXES = {'stu1_40.npy': [(3, 2, 30, 25), (-5, -5, 40, 40), None, (30, 10, 40, 40)],
         'stu5_32.npy': [(1, 1, 9, 9), None, (0, 0, 36, 52), (50, 0, 5, 5), (10, -3, 8, 70), (2, 2, 1, 1)]}


def _video(name):
    frames, h, w = VIDEOS[name]
    return torch.from_numpy(synthetic_video(len(name) + frames, frames, h, w, period=12))


@pytest.fixture(scope='module')
def dataset(tmp_path_factory, golden_dir):
    import pandas as pd
    anno = pd.read_csv(f'{golden_dir}/repcount_annotation.csv', index_col=0)
    rows = anno[anno['name'].isin([n.replace('.npy', '.mp4') for n in VIDEOS])].copy()
    rows['name'] = [n.replace('.mp4', '.npy') for n in rows['name']]
    root = tmp_path_factory.mktemp('RepCount')
    rows.to_csv(root / 'annotation.csv')
    return str(root)


def _make_engine(sd0, poison):
    from workoutdetector_amd.engine import TsmEngine
    keep = {k: os.environ.get(k) for k in ('TSM_AUTOTUNE', 'TSM_POISON')}
    os.environ['TSM_AUTOTUNE'] = '0'
    os.environ.pop('TSM_POISON', None)
    if poison:
        os.environ['TSM_POISON'] = '1'
    try:
        return TsmEngine(num_class=12, num_segments=8, max_clips=4, state_dict=sd0)       # (TSM_* are read in tsm_create)
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.fixture(scope='module')
def engine(hip_lib, sd0):
    eng = _make_engine(sd0, poison=False)
    yield eng
    eng.close()


def _run_dataset(eng, dataset, out_dir, shard):
    from workoutdetector_amd import inference_count as ic
    ic.inference_dataset(eng, ['test'], out_dir, checkpoint='seed0', data_root=dataset, person_crop=True, boxes=BOXES,
                         video_reader=lambda path: _video(os.path.basename(path)), batch_clips=4, shard=shard)
    return {name: json.load(open(os.path.join(out_dir, f'{name}.score.json'))) for name in VIDEOS}


def _logits(d):
    return np.float32([[d['scores'][s][str(k)] for k in range(12)] for s in d['scores']])


def test_dataset_path_is_one_fused_launch_per_batch_and_matches_the_torch_transform(engine, dataset, tmp_path):
    """inference_dataset(person_crop=True) on a TsmEngine: per batch one preprocess_clips_kernel launch and the forward --
    neither preprocess_kernel nor gather_clips_kernel runs; shard None / 'clips' and 'videos' write identical files with the
    reference's schema; and the logits equal forward_device on the torch PersonCropTransform's output within the bound the
    pipeline test holds the HIP transform to against the torch one (tests/test_pipeline_gpu.py: rtol 1e-5, atol 1e-4)."""
    from workoutdetector_amd.engine import launch_trace
    from workoutdetector_amd.transform import PersonCropTransform
    with launch_trace() as tr:
        clips = _run_dataset(engine, dataset, str(tmp_path / 'clips'), None)
    assert tr.count('preprocess_clips_kernel') == 1 + 2, tr.kernels            # 4 clips = one batch, 6 clips = two
    assert not tr.ran('preprocess_kernel') and not tr.ran('gather_clips'), tr.kernels
    videos = _run_dataset(engine, dataset, str(tmp_path / 'videos'), 'videos')
    assert clips == videos
    tf = PersonCropTransform(BOXES)
    for name, d in clips.items():
        frames = VIDEOS[name][0]
        assert list(d) == ['video_name', 'model', 'input_shape', 'checkpoint', 'total_frames', 'ground_truth', 'action', 'scores']
        assert d['total_frames'] == frames and list(d['scores']) == [str(s) for s in range(0, frames, 8)]
        vid = _video(name)
        x = torch.stack([tf(pc.window(vid, c), tf.box(name, c)) for c in range(len(BOXES[name]))])     # torch, on the CPU
        want = torch.cat([engine.forward_device(x[a:a + 4].cuda()) for a in range(0, x.shape[0], 4)]).cpu().numpy()
        got = _logits(d)
        print(f'{name}: max |fused - torch| {np.abs(got - want).max():.3g}, logit scale {np.abs(want).max():.3g}')
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-4)


def test_whole_engine_under_poison_gives_the_same_score_files(engine, sd0, dataset, tmp_path):
    """TSM_POISON=1: every device buffer of the engine between poisoned bands, activations poisoned before each forward.
    The fused transform hands its packed clips to that engine: same files, bit for bit."""
    clean = _run_dataset(engine, dataset, str(tmp_path / 'clean'), 'clips')
    eng = _make_engine(sd0, poison=True)
    try:
        poisoned = _run_dataset(eng, dataset, str(tmp_path / 'poisoned'), 'clips')
    finally:
        eng.close()
    assert poisoned == clean
