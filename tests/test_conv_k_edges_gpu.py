"""Per-op conv tests ALONG K (tsm_conv_op through engine.conv_bn_act_nhwc), the cases of tests/_k_cases.py built for this device:

  a. short K, where the loop is shorter than its two-step prologue: one K-step (1x1 at cin 32 in fp32 / split-bf16, 64 -> 256 on
     conv_bf16_256_kernel, whose persistent twin must fall back), duals of 2 and 3 steps with the source switch inside the
     prologue's preloads, the 3x3 at cin 32 (nine steps, one tap each), Cout 320 and 4096 where a code does not fit;
  b. the engine's segmented single-source launches (segmented=True: shifted 1x1 at cin 1024 / 2048, 3x3 at cin 128 .. 512),
     whole-K, split-K and the tail split, and against the unsegmented launch of the same operands;
  c. mixed-source segmented duals (1024+32, 32+1024, 2048+32, 1024+64): the source switch strictly inside a segment or at step
     1, ragged last segments under 2 and 4 segments; the same shapes unsegmented in the bf16 formats;
  d. the longest whole-K chains (cin 4096 and 8192);
  e. the stem: fp32 at stride 1, and every format on frames smaller than the 7x7 window, on both stem kernels.

Every case runs in hostile memory (tests/_guard.py), asserts from the launch trace that the instantiation it names ran -- and,
where a code does not fit the launch, the tile the host rules fall back to -- and that the shift was never materialised, sweeps
its tile codes in both walk directions bit-identically, and is compared with the float64 reference (tests/_conv_ref.py) of the
fp32 operands.  Bars: the project's per-op ones -- fp32 rtol 1e-4 + 1e-4 of the scale, split-bf16 3e-4 + 3e-4, bf16
assert_bf16_op; tests/test_k_bars_cpu.py shows on the CPU that a correct kernel's chain stays below a tenth of them at these K."""
import pytest
import torch

from tests import _k_cases as kc
from tests._conv_ref import conv_ref
from tests._guard import guarded_conv
from tests._util import assert_close, ran_tile, sweep as _sweep
from tests.test_conv_forms_gpu import _bn, _check, _nchw, _nhwc, _w

pytestmark = pytest.mark.gpu


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


CASES = kc.cases(_n_cu())


def operands(c):
    """The case's operands on the CPU (NCHW, seeded by its id): (x, w, bn), the keyword arguments of the launch (CUDA tensors)
    and those of the reference."""
    g = torch.Generator().manual_seed(sum(map(ord, c['id'])))
    x, w, bn = torch.randn(c['n'], c['cin'], c['hi'], c['wi'], generator=g), _w(c['cout'], c['cin'], c['k'], g), _bn(c['cout'], g)
    ho, wo = kc.out_hw(c)
    kw, ref, form = {}, {}, c['form']
    if form in ('res', 'shift_res'):
        res = torch.randn(c['n'], c['cout'], ho, wo, generator=g)
        kw['residual'], ref['residual'] = _nhwc(res).cuda(), res
    if 'cin2' in c:
        x2, w2, bn2 = torch.randn(c['n'], c['cin2'], c['hi2'], c['wi2'], generator=g), _w(c['cout'], c['cin2'], 1, g), _bn(c['cout'], g)
        kw.update(x2=_nhwc(x2).cuda(), w2=w2.cuda(), bn2=[b.cuda() for b in bn2], stride2=c['stride2'])
        ref.update(x2=x2, w2=w2, bn2=bn2, stride2=c['stride2'])
    if c['T'] > 0:
        kw.update(shift_segments=c['T'], fold_div=c['fold_div'], shift_identity=form != 'shift')
        ref.update(T=c['T'], fold_div=c['fold_div'], shift_target=int(form != 'shift'))
    return (x, w, bn), kw, ref


def launcher(c, ops, kw):
    """run(code, reverse, segmented = the case's) -> (y NCHW on the CPU, the launch trace), in hostile memory."""
    from workoutdetector_amd.engine import launch_trace
    x, w, bn = ops
    xd, wd, bnd = _nhwc(x).cuda(), w.cuda(), [b.cuda() for b in bn]

    def run(code, rev, segmented=c['segmented']):
        with launch_trace() as tr:
            y = guarded_conv(xd, wd, *bnd, stride=c['stride'], dtype=c['dtype'], code=code, reverse=rev, segmented=segmented, **kw)
        assert not tr.ran('temporal_shift_kernel'), ('the shifted tensor must never be materialised', tr.kernels)
        return _nchw(y.cpu()), tr
    return run


def reference(c, ops, ref):
    x, w, bn = ops
    return conv_ref(x, w, bn, c['stride'], True, bf16=c['dtype'] == 'bf16', **ref)


def expect_ran(c, code, tr):
    """The trace of one launch: the tile the host rules end on for this code, the instantiation the case names, and the split
    reduction behind the split forms only."""
    tile = kc.tile_that_runs(c, code)
    others = [p for t, p in ((6, 'conv_bf16_256_kernel<'), (8, 'conv_bf16_256p_kernel<')) if t != tile]
    if tile in (6, 8):
        assert tr.ran(c['kernels'][tile]), (c['id'], code, tr.kernels)
    else:
        assert ran_tile(tr, kc.TILE_NAMES[tile]), (c['id'], code, kc.TILE_NAMES[tile], tr.kernels)
        lines = [k for k in tr.kernels if k.startswith('conv_igemm<')]
        assert any(all(s in k for s in c['inst']) for k in lines), (c['id'], code, c['inst'], tr.kernels)
    for p in others + ['conv1x1_ws', 'conv3x3_ws', 'stem_direct_kernel<']:
        assert not tr.ran(p), (c['id'], code, p, tr.kernels)
    split = bool(code & kc.SPLITK) or (bool(code & kc.TAILK) and bool(c.get('tail')))
    reduces = [k for k in tr.kernels if k.startswith('splitk_reduce_kernel')]
    assert len(reduces) == (1 if split and c['segs'] else 0), (c['id'], code, tr.kernels)


@pytest.mark.parametrize('case', CASES, ids=[c['id'] for c in CASES])
def test_conv_along_k(hip_lib, monkeypatch, case):
    c = case
    if c['env'] is None:
        monkeypatch.delenv('TSM_STEM_DIRECT', raising=False)     # (tsm_conv_op reads it per call)
    else:
        monkeypatch.setenv('TSM_STEM_DIRECT', c['env'])
    ops, kw, ref = operands(c)
    run = launcher(c, ops, kw)
    want = reference(c, ops, ref)
    if c['kernels'].get(3, '').startswith('stem_direct'):        # the direct stem walks no tiles and takes no code
        got, tr = run(0, False)
        assert tr.ran('stem_direct_kernel<') and not tr.ran('conv_igemm<'), tr.kernels
    else:
        got = _sweep(c['codes'], run, lambda code, tr: expect_ran(c, code, tr))
    assert float((got != 0).float().mean()) > 0.2, f'{c["id"]}: the output is mostly zeros'
    _check(got.numpy(), want.numpy(), c['dtype'], c['id'])
    if c['segmented']:
        # the same operands whole-K: another summation order, so not the same bits, but the same fp32 bar (each against the other
        # as against float64); its trace shows the unsegmented instantiation and no reduction
        plain, tr = run(3, False, segmented=False)
        assert any('kPrecF32>' in k for k in tr.kernels if k.startswith('conv_igemm<')) and not tr.ran('splitk_reduce_kernel'), tr.kernels
        _check(plain.numpy(), want.numpy(), 'f32', c['id'] + ' whole-K')
        assert_close(got.numpy(), plain.numpy(), rtol=1e-4, atol_scale=1e-4, what=c['id'] + ': segmented vs whole-K')


def test_segmented_refusals_launch_nothing(hip_lib):
    """segmented=True where no segmented kernel exists is refused (TSM_ERR_INVALID_ARG, its own text) before any launch."""
    from workoutdetector_amd import _lib
    from workoutdetector_amd.engine import conv_bn_act_nhwc, launch_trace
    g = torch.Generator().manual_seed(5)
    x = torch.randn(8, 2, 2, 1024, generator=g).cuda()
    bn = [t.cuda() for t in _bn(64, g)]
    w1 = _w(64, 1024, 1, g).cuda()
    res = torch.randn(8, 2, 2, 64, generator=g).cuda()
    x128 = torch.randn(8, 2, 2, 128, generator=g).cuda()
    w3 = _w(64, 128, 3, g).cuda()
    x512 = torch.randn(8, 2, 2, 512, generator=g).cuda()
    stem = torch.randn(2, 8, 8, 3, generator=g).cuda()
    cases = [
        ('a residual', 'residual', x, dict(w=w1, residual=res)),
        ('a shifted 3x3', 'shifted 3x3', x128, dict(w=w3, shift_segments=8)),
        ('the stem', 'stem', stem, dict(w=_w(64, 3, 7, g).cuda(), stride=2)),
        ('split-bf16', 'fp32 only', x, dict(w=w1, dtype='bf16x3')),
        ('bf16', 'fp32 only', x, dict(w=w1, dtype='bf16')),
        ('16 K-steps', '32 K-steps', x512, dict(w=_w(64, 512, 1, g).cuda())),
        ('a second source', 'second source', x, dict(w=w1, x2=x, w2=w1, bn2=bn)),
    ]
    for what, text, xin, kw in cases:
        kw = dict(kw)
        wt = kw.pop('w')
        with launch_trace() as tr:
            with pytest.raises(_lib.TsmError) as ei:
                conv_bn_act_nhwc(xin, wt, *bn, segmented=True, code=3, **kw)
        assert ei.value.status == -1 and text in str(ei.value), (what, ei.value)
        assert tr.kernels == [], (what, tr.kernels)
        conv_bn_act_nhwc(xin, wt, *bn, code=3, **kw)          # the same call without the bit is accepted
