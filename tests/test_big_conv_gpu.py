"""Every conv kernel family of tsm_conv_op on tensors past 2^31 and 2^32 bytes, and on both sides of its capacity rule: the
cases of tests/_big_cases.py, whose claims tests/test_big_cases_cpu.py checks.

Every operand with a frame dimension is PERIODIC -- P frames (three clips) repeated R times, written straight into a guarded
view (tests/_guard.py) -- so no big reference is needed.  For every tile code of a case, in both walk directions:

* the trace shows the family the case is for (or, for a case just outside a capacity rule, that the family did NOT run and a
  fallback did), every tile-walking launch in the direction asked for, the conversion / packing kernels of the format, and for
  a position-major launch whether its XCD runs were live-balanced (TSM_POS_BALANCE unset) or equal-count (= 0);
* the guard bands are intact and no output word is still poison (check);
* the output repeats with the period, compared on the device as int32 words: y.view(R, -1)[r] == y.view(R, -1)[0] for every r.
  An element's bits depend on its K-chain alone -- not on its tile, the walk or the launch -- so this is exact; a wrapped
  offset reads or writes another phase of the period, a sign-extended one leaves zeros or poison;
* the first AND the last period are bit-identical to those of the case's first run;

and the first period of the first run meets the float64 reference of the P frames (tests/_conv_ref.py) at the per-op bars of
tests/test_conv_forms_gpu.py and is not mostly zeros."""
import pytest
import torch

from tests._big_cases import POS, SPLITK, TAILK, cases, conv_num_segments_of, edges
from tests._conv_ref import conv_ref
from tests._guard import check, guarded, guarded_out, guarded_repeat
from tests._util import IGEMM_TILE_DIMS, REVERSE_MARK, assert_periodic, assert_walked, walked
from tests._walk_cases import out_hw, tail_split_applies
from tests.test_conv_forms_gpu import _bn, _check, _nchw, _nhwc, _w

pytestmark = pytest.mark.gpu

NAMES = {1: '128x128', 2: '128x64', 3: '64x64', 4: '32x32', 5: '128x128w8', 9: '64x128'}
FAMILY_KERNEL = {6: 'conv_bf16_256_kernel<', 8: 'conv_bf16_256p_kernel<'}
POS_ARM, NATURAL_ARM = 'kPrecF32 | kPrecPosMajor, false, true>', 'kPrecF32, false, true>'
ENV = ('TSM_STEM_DIRECT', 'TSM_POS_BALANCE', 'TSM_CONV_TILE')


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


def _has(tr, text):
    return any(text in k for k in tr.kernels)


def _family_code(inst):
    return 8 if inst.startswith('conv_bf16_256p_') else 6 if inst.startswith('conv_bf16_256_') else \
        7 if inst.startswith(('conv1x1_ws', 'conv3x3_ws')) else None


def _igemm_lines(tr):
    return [k for k in tr.kernels if k.startswith('conv_igemm<')]


def _expect(c, code, tr, n_cu):
    """What must (not) have run behind `code`."""
    cid, base, fam_code = (c['id'], hex(code)), code & 0xF, _family_code(c['inst'])
    ho, wo = out_hw(c)
    m = c['n'] * ho * wo
    if c['family'] == 'stem':
        assert tr.ran(c['inst']) and not _igemm_lines(tr), (cid, tr.kernels)
    elif base in FAMILY_KERNEL:
        assert tr.ran(FAMILY_KERNEL[base]), (cid, tr.kernels)
        if base == fam_code:
            assert tr.ran(c['inst']), (cid, tr.kernels)
    elif base == 7:
        if c['cap'] == 'outside':      # the rule refuses the size: the heuristic conv_igemm tile runs instead
            assert _igemm_lines(tr), (cid, tr.kernels)
        else:
            assert tr.ran(c['inst']), (cid, tr.kernels)
    elif base == 9:                    # (the 64x128 tile is launched as an explicit instantiation: no bracket)
        assert tr.ran('conv_igemm<64, 128, 2, 2, 1, false, false, kPrecF32>'), (cid, tr.kernels)
    else:
        want = '[BM = %d, BN = %d, WGM = %d, WGN = %d,' % IGEMM_TILE_DIMS[NAMES[base]]
        assert any(want in k for k in _igemm_lines(tr)), (cid, want, tr.kernels)
        if c['family'] == 'pos':
            arm = POS_ARM if code & POS and c['cap'] == 'inside' else NATURAL_ARM
            assert all(arm in k for k in _igemm_lines(tr)), (cid, arm, tr.kernels)
            if arm == POS_ARM:         # live-balanced XCD runs carry a bracket about their grid; TSM_POS_BALANCE=0 runs equal counts
                balanced = c['env'].get('TSM_POS_BALANCE') != '0'
                assert all((' [balanced ' in k) == balanced for k in _igemm_lines(tr)), (cid, balanced, tr.kernels)
        elif fam_code is None:
            assert any(c['inst'] in k for k in _igemm_lines(tr)), (cid, tr.kernels)
    if c['cap'] == 'outside':
        assert not _has(tr, c['inst']), f'{cid}: {c["inst"]} ran at a size its rule refuses: {tr.kernels}'
    nseg = conv_num_segments_of(c)
    split = c['segmented'] and (bool(code & SPLITK) or (bool(code & TAILK) and tail_split_applies(m, c['cout'], nseg, n_cu)))
    assert tr.ran('splitk_reduce') == split, (cid, tr.kernels)
    # the conversions at the boundary of the bf16 formats and the stem's packing ran on these sizes too
    if c['dtype'] != 'f32':
        assert tr.ran('to_f32_kernel<') and (c['k'] == 7 or tr.ran('from_f32_kernel<')), (cid, tr.kernels)
    if c['k'] == 7:
        assert tr.ran('pack_input_kernel'), (cid, tr.kernels)


CASES = cases(_n_cu())


@pytest.mark.parametrize('case', CASES, ids=[c['id'] for c in CASES])
def test_big_conv(hip_lib, monkeypatch, case):
    from workoutdetector_amd.engine import conv_bn_act_nhwc, launch_trace
    c, n_cu = case, _n_cu()
    free, total = torch.cuda.mem_get_info()
    if c['need'] << 30 > free:
        pytest.skip(f'{c["id"]} needs {c["need"]} GiB of device memory, {free / 2 ** 30:.1f} GiB of {total / 2 ** 30:.1f} are free')
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    for name, value in c['env'].items():
        monkeypatch.setenv(name, value)
    assert edges(c) == c['big'], c['id']
    g = torch.Generator().manual_seed(sum(map(ord, c['id'])))
    P, R, T, form, dtype = c['P'], c['R'], c['T'], c['form'], c['dtype']
    ho, wo = out_hw(c)
    x, w, bn = torch.randn(P, c['cin'], c['hi'], c['wi'], generator=g), _w(c['cout'], c['cin'], c['k'], g), _bn(c['cout'], g)
    kw, ref = {}, {}
    torch.cuda.reset_peak_memory_stats()
    try:
        if form in ('res', 'shift_res'):
            res = torch.randn(P, c['cout'], ho, wo, generator=g)
            kw['residual'], ref['residual'] = guarded_repeat(_nhwc(res).cuda(), R, name='residual'), res
        if 'cin2' in c:
            x2, w2, bn2 = torch.randn(P, c['cin2'], c['hi2'], c['wi2'], generator=g), _w(c['cout'], c['cin2'], 1, g), _bn(c['cout'], g)
            kw.update(x2=guarded_repeat(_nhwc(x2).cuda(), R, name='x2'), w2=guarded(w2.cuda(), name='w2'),
                      bn2=[guarded(b.cuda(), name=f'bn2[{i}]') for i, b in enumerate(bn2)], stride2=c['stride2'])
            ref.update(x2=x2, w2=w2, bn2=bn2, stride2=c['stride2'])
        if T > 0:
            identity = form != 'shift'
            kw.update(shift_segments=T, fold_div=c['fold_div'], shift_identity=identity)
            ref.update(T=T, fold_div=c['fold_div'], shift_target=int(identity))
        xd = guarded_repeat(_nhwc(x).cuda(), R, name='x')
        wd, bnd = guarded(w.cuda(), name='w'), [guarded(b.cuda(), name=f'bn[{i}]') for i, b in enumerate(bn)]
        operands = [xd, wd, *bnd, kw.get('residual'), kw.get('x2'), kw.get('w2'), *kw.get('bn2', ())]
        first = None
        for code in c['codes']:
            for rev in ((False,) if c['family'] == 'stem' else (False, True)):
                what = f'{c["id"]} code {code:#x} reverse {rev}'
                y = guarded_out((c['n'], ho, wo, c['cout']), torch.float32, 'cuda', name='y')
                with launch_trace() as tr:
                    got = conv_bn_act_nhwc(xd, wd, *bnd, stride=c['stride'], dtype=dtype, code=code, reverse=rev, out=y,
                                           segmented=c['segmented'], **kw)
                assert got is y
                torch.cuda.synchronize()
                _expect(c, code, tr, n_cu)
                if c['family'] == 'stem':
                    assert not any(k.endswith(REVERSE_MARK) for k in tr.kernels) and not walked(tr), tr.kernels
                else:
                    assert_walked(tr, rev, what)
                check(y, *operands)
                words = assert_periodic(y, R, what)
                if first is None:
                    first = (what, words[0].clone(), words[R - 1].clone())
                    got0 = _nchw(y[:P].cpu())
                else:
                    assert torch.equal(words[0], first[1]), f'{what}: the first period differs from that of {first[0]}'
                    assert torch.equal(words[R - 1], first[2]), f'{what}: the last period differs from that of {first[0]}'
                del y, got, words
        want = conv_ref(x, w, bn, c['stride'], True, bf16=dtype == 'bf16', **ref)
        assert float((got0 != 0).float().mean()) > 0.2, f'{c["id"]}: the output is mostly zeros'
        _check(got0.numpy(), want.numpy(), dtype, c['id'])
        print(f'\n[{c["id"]}] need {c["need"]} GiB, torch peak {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB')
    finally:
        xd = wd = bnd = operands = first = None
        kw.clear()
        torch.cuda.empty_cache()    # (multi-GiB blocks: hand them back before the next test)
