"""Case table of tests/test_conv_k_edges_gpu.py: what tsm_conv_op accepts along K, at the lengths where a hand-scheduled K loop
goes wrong -- a loop shorter than its two-step prologue, a source switch inside the prologue's preloads, the engine's
single-source segmented launches, segmented duals whose source switch sits inside a segment and whose last segment is ragged,
and the longest whole-K chains.  Pure arithmetic (no torch, no GPU): tests/test_k_cases_cpu.py checks every claim of a case
against the host rules restated below (tsm_host_util.h: layer_geometry, segment_len; tsm_igemm.hip: conv_num_segments,
conv_tile_valid, conv_tile_shape), and that the table as a whole holds the lengths it is there for.

A case is a dict: `id`, `group` (a .. e, the sections of the GPU test), the conv (`dtype`, `k`, `stride`, `cin`, `cout`, `n`,
`hi`, `wi`, `T`, `fold_div`, `form`; `cin2`, `hi2`, `wi2`, `stride2` for a second source; `segmented`), the tile `codes` to
sweep, `inst` (substrings that one conv_igemm trace line must all hold) and, for the other kernel families, `kernels`
{code: trace prefix}.  Its CLAIMS, written out by hand where the case is made and never computed:
  `steps`   K-steps of the launch in the case's format (32 channels-taps a step; bf16: 64),
  `segs`    the lengths of its accumulation segments in K-steps (None: whole-K), the last one ragged when shorter,
  `switch`  the K-step at which the operand source changes to the second one (None: a single source),
  `where`   what that step is to the loop: 'preload' (step 1: between the prologue's two preloads), 'inject' (step 2: the first
            load the loop body injects), 'inside' (strictly inside a segment), 'boundary' (on a segment boundary), 'loop'."""
from tests._walk_cases import _fit, _igemm_codes, _in_hw, tail_split_applies

KC = {'f32': 32, 'bf16x3': 32, 'bf16': 64}          # channels-taps per K-step
PREC = {'f32': 'kPrecF32', 'bf16x3': 'kPrecBf16x3', 'bf16': 'kPrecBf16'}
SPLITK, TAILK = 0x100, 0x200
SEG_CODES = [3, 4, 3 | SPLITK, 4 | SPLITK, 3 | TAILK]      # as _walk_cases.seg_codes
TILE_NAMES = {1: '128x128', 2: '128x64', 3: '64x64', 4: '32x32', 5: '128x128w8', 6: '256x256', 8: '256x256p'}


# ---- the host rules, restated -----------------------------------------------------------------------------------------------
def layer_geometry(cin, k, stride, dtype):
    """(cp, kp, kseg) of tsm_host::layer_geometry."""
    pairs = k == 7 and stride == 2 and dtype != 'f32'
    cp = 4 if k == 7 else cin
    unit = KC[dtype]
    kp = -(-(7 * 4 * 8 if pairs else k * k * cp) // unit) * unit
    return cp, kp, segment_len(kp, dtype)


def segment_len(kp, dtype):
    """tsm_host::segment_len: fp32 launches of at least 32 K-steps sum K in nk // 16 segments of equal length, rounded up."""
    nk = kp // 32
    if dtype != 'f32' or nk < 32:
        return 0
    nseg = nk // 16
    return -(-nk // nseg)


def conv_num_segments(kp, kseg):
    return 1 if kseg <= 0 else -(-(kp // 32) // kseg)


def kp_total(c):
    kp = layer_geometry(c['cin'], c['k'], c['stride'], c['dtype'])[1]
    return kp + (layer_geometry(c['cin2'], 1, c['stride2'], c['dtype'])[1] if 'cin2' in c else 0)


def kseg_of(c):
    """The launch's segment length: a second source is segmented by its whole K (set_second_source), a single source only
    where the case asks for the engine's form."""
    if 'cin2' in c:
        return segment_len(kp_total(c), c['dtype'])
    return layer_geometry(c['cin'], c['k'], c['stride'], c['dtype'])[2] if c['segmented'] else 0


def steps(c):
    return kp_total(c) // KC[c['dtype']]


def segments(c):
    kseg, nk = kseg_of(c), steps(c)
    if kseg <= 0:
        return None
    return [min(kseg, nk - s) for s in range(0, nk, kseg)]


def switch_step(c):
    return layer_geometry(c['cin'], c['k'], c['stride'], c['dtype'])[1] // KC[c['dtype']] if 'cin2' in c else None


def switch_where(c):
    s, kseg = switch_step(c), kseg_of(c)
    if s is None:
        return None
    if s == 1:
        return 'preload'
    if s == 2:
        return 'inject'
    if kseg > 0:
        return 'boundary' if s % kseg == 0 else 'inside'
    return 'loop'


def out_hw(c):
    pad = c['k'] // 2
    return (c['hi'] + 2 * pad - c['k']) // c['stride'] + 1, (c['wi'] + 2 * pad - c['k']) // c['stride'] + 1


def rows(c):
    ho, wo = out_hw(c)
    return c['n'] * ho * wo


def tile_valid(c, tile):
    """conv_tile_valid for the tiles these cases name (1 .. 6, 8)."""
    shifted_identity = c['T'] > 0 and c['form'] in ('shift_res', 's2shift', 'dual_shift')
    res, dual = c['form'] in ('res', 'shift_res'), 'cin2' in c
    if shifted_identity and (tile == 6 or (tile == 8 and (c['k'] != 1 or not (res or dual)))):
        return False
    if tile in (1, 5):
        return c['cout'] % 128 == 0
    if tile in (2, 3):
        return True
    if tile == 4:
        return c['dtype'] == 'f32'
    if tile in (6, 8):
        ok = (c['dtype'] == 'bf16' and c['cout'] % 256 == 0 and c['k'] != 7 and c['cin'] % 64 == 0 and not (res and dual) and
              (c['k'] != 3 or (not res and c['T'] == 0)) and (not dual or c['cin2'] % 64 == 0))
        return ok and (tile == 6 or (kp_total(c) >= 128 and c['cout'] <= 2048))
    return False


def heuristic_tile(m, cout):
    """conv_tile_shape: 128 x 128 (128 x 64 where Cout is no multiple of 128), 64 x 64 while that leaves under 256 tiles."""
    bn = 128 if cout % 128 == 0 else 64
    return 3 if -(-m // 128) * (cout // bn) < 256 else (1 if bn == 128 else 2)


def tile_that_runs(c, code):
    """The tile code a launch with `code` ends on: checked_code sends a code that does not fit to the heuristic, and a segmented
    launch runs on 64 x 64 unless it asked for 32 x 32 (launch_conv_ks)."""
    tile = code & 0xF
    if not tile_valid(c, tile):
        tile = heuristic_tile(rows(c), c['cout'])
    if kseg_of(c) > 0 and tile != 4:
        tile = 3
    return tile


# ---- shapes -----------------------------------------------------------------------------------------------------------------
# one 64-row tile that still crosses frames and clips: T -> (clips, ho, wo); 60, 54 and 56 rows
ONE_TILE = {1: (4, 3, 5), 3: (3, 2, 3), 8: (7, 1, 1)}
ONE_TILE_7 = {1: (1, 7, 7), 3: (1, 4, 4), 8: (1, 2, 3)}      # 49, 48 and 48 rows: larger frames, one clip


def _case(group, name, dtype, k, stride, cin, cout, T, form, shape, codes, inst, *, steps, segs=None, switch=None, where=None,
          fold_div=8, cin2=None, stride2=1, even=False, segmented=False, kernels=None, env=None):
    clips, ho, wo = shape
    hi, wi = _in_hw(ho, wo, k, stride)
    if even and stride == 2:
        hi, wi = 2 * ho, 2 * wo           # (the last output then reads the last input column but one)
    c = dict(id=f'{group}-{name}-{dtype}', group=group, dtype=dtype, k=k, stride=stride, cin=cin, cout=cout, n=clips * max(T, 1),
             hi=hi, wi=wi, T=T, fold_div=fold_div, form=form, segmented=segmented, codes=list(codes), inst=tuple(inst),
             kernels=dict(kernels or {}), env=env, steps=steps, segs=segs, switch=switch, where=where)
    if cin2 is not None:
        c.update(cin2=cin2, stride2=stride2)
        c['hi2'], c['wi2'] = (2 * ho, 2 * wo) if (even and stride2 == 2) else _in_hw(ho, wo, 1, stride2)
    return c


def _arm(dtype, form, seg=False):
    """The conv_igemm template tail of a form: <..., PREC [| kPrecBlockShift][, DUAL[, SEG]]>."""
    p = PREC[dtype] + (' | kPrecBlockShift' if form in ('shift_res', 'dual_shift') else '')
    if form in ('dual', 'dual_shift'):
        return p + (', true, true>' if seg else ', true>')
    return p + (', false, true>' if seg else '>')


def _ks(k, form, seg=False):
    """The bracket of the trace line: the launcher's own template parameters (launch_conv_seg has no RES)."""
    s = f'KS = {k}, SHIFT = {"true" if form == "shift" or (form == "s2shift") else "false"}'
    return s + ']' if seg else s + f', RES = {"true" if form in ("res", "shift_res") else "false"}]'


def cases(n_cu):
    out = []
    big = lambda T: _fit(n_cu + 1, 64, max(T, 1), exact=False)      # n_cu + 1 tiles of 64 rows, the last one ragged

    # ---- a. short K: the loop is shorter than its prologue ---------------------------------------------------------------------
    for dtype in ('f32', 'bf16x3'):
        for cout in (64, 320):        # 320 = 64 x 5: the 128-wide codes 1 and 5 do not fit and fall back
            codes = [1, 2, 3, 4, 5] if dtype == 'f32' else [1, 2, 3, 5]
            if cout == 64:
                codes = _igemm_codes(dtype, 64)
            forms = [('plain', 'plain', 1, 0, 8, ONE_TILE[1]), ('shift4', 'shift', 1, 3, 4, ONE_TILE[3]),
                     ('shiftres', 'shift_res', 1, 8, 4, ONE_TILE[8]), ('s2shift', 's2shift', 2, 3, 4, ONE_TILE_7[3])]
            if dtype == 'f32':
                forms.append(('shift8', 'shift', 1, 8, 8, ONE_TILE_7[8]))      # fold 4: one 16-byte chunk each way
            for name, form, stride, T, div, shape in forms:
                out.append(_case('a', f'1x1-32-{name}-c{cout}', dtype, 1, stride, 32, cout, T, form, shape, codes,
                                 (_arm(dtype, form), _ks(1, form)), steps=1, fold_div=div))
        out.append(_case('a', '1x1-32-shift4-big', dtype, 1, 1, 32, 64, 3, 'shift', big(3), _igemm_codes(dtype, 64),
                         (_arm(dtype, 'shift'), _ks(1, 'shift')), steps=1, fold_div=4))
        # duals of 2 and 3 steps: the source switch inside the prologue's preloads / at the first injected load
        for c1, c2, nsteps, sw, where in ((32, 32, 2, 1, 'preload'), (32, 64, 3, 1, 'preload'), (64, 32, 3, 2, 'inject')):
            for s2 in (1, 2):
                for shift in (False, True):
                    form, T = ('dual_shift', 3 if s2 == 1 else 8) if shift else ('dual', 0)
                    shape = ONE_TILE[T] if shift else ONE_TILE_7[1 if s2 == 1 else 3]
                    out.append(_case('a', f'dual-{c1}+{c2}-s{s2}{"-shift" if shift else ""}', dtype, 1, 1, c1, 64, T, form, shape,
                                     _igemm_codes(dtype, 64), (_arm(dtype, form), _ks(1, form)), steps=nsteps, switch=sw,
                                     where=where, fold_div=4, cin2=c2, stride2=s2, even=shift))
        # 3x3 at cin 32: nine steps, one tap each
        for stride in (1, 2):
            out.append(_case('a', f'3x3-32-s{stride}', dtype, 3, stride, 32, 64, 0, 'plain', ONE_TILE[3 if stride == 1 else 1],
                             _igemm_codes(dtype, 64), (_arm(dtype, 'plain'), _ks(3, 'plain')), steps=9, even=stride == 2))
    for stride in (1, 2):
        out.append(_case('a', f'3x3-32-s{stride}-shift', 'f32', 3, stride, 32, 64, 3, 'shift', ONE_TILE_7[3], _igemm_codes('f32', 64),
                         (_arm('f32', 'shift'), _ks(3, 'shift')), steps=9, fold_div=4))
    # bf16: one K-tile on the 256 x 256 kernel (code 6); the persistent one (code 8) needs two and falls back to the heuristic
    bf = _igemm_codes('bf16', 256)
    for name, form, T, kern6 in (('plain', 'plain', 0, 'conv_bf16_256_kernel<1, false>'),
                                 ('res', 'res', 0, 'conv_bf16_256_kernel<1, false, true, false>'),
                                 ('shift', 'shift', 8, 'conv_bf16_256_kernel<1, true>')):
        out.append(_case('a', f'1x1-64-256-{name}', 'bf16', 1, 1, 64, 256, T, form, ONE_TILE[max(T, 1)] if T else ONE_TILE_7[1],
                         bf + [6, 8], (_arm('bf16', form), _ks(1, form)), steps=1, kernels={6: kern6}))
    # Cout above code 8's 2048 (its bias sits in LDS): the fallback again, with one step and with two
    for cin in (64, 128):
        out.append(_case('a', f'1x1-{cin}-4096', 'bf16', 1, 1, cin, 4096, 0, 'plain', ONE_TILE[3], [3, 6, 8],
                         (_arm('bf16', 'plain'), _ks(1, 'plain')), steps=cin // 64, kernels={6: 'conv_bf16_256_kernel<1, false>'}))

    # ---- b. the engine's segmented single-source forms -------------------------------------------------------------------------
    def seg_case(name, k, stride, cin, T, shape, steps, segs, cout=64, even=False):
        form = 'shift' if T else 'plain'
        return _case('b', name, 'f32', k, stride, cin, cout, T, form, shape, SEG_CODES, (_arm('f32', form, True), _ks(k, form, True)),
                     steps=steps, segs=segs, segmented=True, even=even)
    out.append(seg_case('1x1-1024-shift', 1, 1, 1024, 8, ONE_TILE[8], 32, [16, 16]))
    out.append(seg_case('1x1-2048-shift', 1, 1, 2048, 3, ONE_TILE[3], 64, [16, 16, 16, 16]))
    out.append(seg_case('3x3-128-s1', 3, 1, 128, 0, ONE_TILE[3], 36, [18, 18]))
    out.append(seg_case('3x3-128-s2', 3, 2, 128, 0, ONE_TILE_7[1], 36, [18, 18]))
    out.append(seg_case('3x3-128-s2-even', 3, 2, 128, 0, ONE_TILE[1], 36, [18, 18], even=True))
    # (3 x 5 frames, not 1 x 1: there the last K-steps are the padding tap (2, 2) and a lost last step would change nothing)
    out.append(seg_case('3x3-256-s1', 3, 1, 256, 0, ONE_TILE[1], 72, [18, 18, 18, 18]))
    out.append(seg_case('3x3-512-s1-big', 3, 1, 512, 0, big(1), 144, [16] * 9))
    out.append(seg_case('3x3-512-s2', 3, 2, 512, 0, ONE_TILE[3], 144, [16] * 9))
    # the tail split really applying: 5 resident 64x64 workgroups per CU, one whole round and 40 % of a second, 4 columns
    tail_tiles = 5 * n_cu * 7 // 5
    tail = seg_case('1x1-1024-shift-tail', 1, 1, 1024, 8, _fit(tail_tiles // 4, 64, 8, exact=False), 32, [16, 16], cout=256)
    tail['tail'] = True
    assert tail_split_applies(rows(tail), 256, 2, n_cu)
    out.append(tail)

    # ---- c. mixed-source segmented duals: the switch inside a segment, ragged last segments -------------------------------------
    mixed = ((1024, 32, 33, [17, 16], 32, 'inside'), (32, 1024, 33, [17, 16], 1, 'preload'),
             (2048, 32, 65, [17, 17, 17, 14], 64, 'inside'), (1024, 64, 34, [17, 17], 32, 'inside'))
    for c1, c2, nsteps, segs, sw, where in mixed:
        for s2 in (1, 2):
            for shift in (False, True):
                T = 0 if not shift else (3 if s2 == 1 else 8)
                form = 'dual_shift' if shift else 'dual'
                div = 8 if c2 >= 64 else 4           # (fold = cin2 / div: 8 channels of 32, 8 of 64, 128 of 1024)
                is_big = (c1, c2, s2, shift) == (2048, 32, 2, True)
                shape = big(T) if is_big else (ONE_TILE[T] if shift else ONE_TILE_7[3 if s2 == 1 else 8])
                name = f'{c1}+{c2}-s{s2}{"-shift" if shift else ""}{"-big" if is_big else ""}'
                out.append(_case('c', name, 'f32', 1, 1, c1, 64, T, form, shape, SEG_CODES, (_arm('f32', form, True), _ks(1, form, True)),
                                 steps=nsteps, segs=segs, switch=sw, where=where, fold_div=div, cin2=c2, stride2=s2, even=shift))
                out.append(_case('c', name, 'bf16x3', 1, 1, c1, 64, T, form, shape, _igemm_codes('bf16x3', 64),
                                 (_arm('bf16x3', form), _ks(1, form)), steps=nsteps, switch=sw,
                                 where='preload' if sw == 1 else 'loop', fold_div=div, cin2=c2, stride2=s2, even=shift))
                if c1 % 64 == 0 and c2 % 64 == 0:    # bf16: 16 + 1 steps of 64
                    out.append(_case('c', name, 'bf16', 1, 1, c1, 64, T, form, shape, _igemm_codes('bf16', 64),
                                     (_arm('bf16', form), _ks(1, form)), steps=17, switch=16, where='loop', fold_div=div, cin2=c2,
                                     stride2=s2, even=shift))

    # ---- d. long whole-K chains through the same entry ---------------------------------------------------------------------------
    for cin, n32 in ((4096, 128), (8192, 256)):
        for dtype in ('f32', 'bf16x3', 'bf16'):
            codes = [c for c in (1, 2, 3, 4, 5) if c != 4 or dtype == 'f32'] + ([6, 8] if dtype == 'bf16' else [])
            kern = {6: 'conv_bf16_256_kernel<1, false>', 8: 'conv_bf16_256p_kernel<1, false>'} if dtype == 'bf16' else {}
            out.append(_case('d', f'1x1-{cin}', dtype, 1, 1, cin, 256, 0, 'plain', ONE_TILE[3 if cin == 4096 else 8], codes,
                             (_arm(dtype, 'plain'), _ks(1, 'plain')), steps=n32 // (2 if dtype == 'bf16' else 1), kernels=kern))
    # n_cu + 1 tiles of 64 x 64 over 4 columns of Cout, the last row of tiles ragged
    out.append(_case('d', '1x1-4096-big', 'bf16x3', 1, 1, 4096, 256, 0, 'plain', _fit(-(-(n_cu + 1) // 4), 64, 1, exact=False),
                     [1, 2, 3, 5], (_arm('bf16x3', 'plain'), _ks(1, 'plain')), steps=128))

    # ---- e. the stem -------------------------------------------------------------------------------------------------------------
    for hi, wi in ((9, 11), (7, 7)):           # fp32 at stride 1 (the bf16 formats refuse it)
        c = _case('e', f'stem-s1-{hi}x{wi}', 'f32', 7, 1, 3, 64, 0, 'plain', (3, hi, wi), _igemm_codes('f32', 64),
                  (_arm('f32', 'plain'), 'KS = 7'), steps=7)
        out.append(c)
    for hi, wi in ((1, 1), (2, 3), (6, 6)):    # frames smaller than the 7 x 7 window, every format, stride 2
        for dtype in ('f32', 'bf16x3', 'bf16'):
            for env in ((None,) if dtype == 'f32' else ('0', None)):       # TSM_STEM_DIRECT = 0: conv_igemm; unset: the direct stem
                direct = dtype != 'f32' and env is None
                c = _case('e', f'stem-s2-{hi}x{wi}{"-direct" if direct else ""}', dtype, 7, 2, 3, 64, 0, 'plain', (5, 1, 1),
                          [3] if direct else _igemm_codes(dtype, 64), () if direct else (_arm(dtype, 'plain'), 'KS = 7'),
                          steps=7 if dtype != 'bf16' else 4, env=env, kernels={3: 'stem_direct_kernel<'} if direct else None)
                c['hi'], c['wi'] = hi, wi
                out.append(c)
    ids = [c['id'] for c in out]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    return out
