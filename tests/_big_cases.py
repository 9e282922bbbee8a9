"""Case table of tests/test_big_conv_gpu.py: every conv kernel family tsm_conv_op reaches, on tensors just past 2^31 and 2^32
bytes -- the sizes at which a 32-bit byte offset wraps or turns negative -- and, for the families whose capacity rule keeps them
below 2^31 bytes by design, at the largest size the rule accepts and the smallest it refuses.  Pure arithmetic (no torch, no
GPU): tests/test_big_cases_cpu.py recomputes every claim of a case from the host rules restated here and in _walk_cases.py /
_k_cases.py, for several CU counts.

No reference of a 4 GiB conv is computed.  Every big operand is PERIODIC: `P` frames (three clips of T frames, so the temporal
shift is periodic too) repeated `R` times, n = P * R frames.  The output must then repeat with the same period bit for bit, and
its first period is checked against the float64 reference of the P frames alone.  A wrapped offset reads or writes another
phase of the period and shows as a mismatch; a sign-extended one falls outside the buffer window (zeros read, the store dropped)
and leaves poison.  Two conditions keep that honest (the CPU test checks both): the period in bytes of every tensor has an odd
factor > 1, so neither 2^31 nor 2^32 is a multiple of it and a wrap cannot land on identical data; and the period's rows are no
multiple of the family's tile rows, so successive periods sit at different places inside tiles.

A case is a dict: `id`, `family` (as _walk_cases.py names the tile rules, plus 'stem' for stem_direct_kernel and 'pos' for the
position-major 3x3), the conv (`dtype`, `k`, `stride`, `cin`, `cout`, `hi`, `wi`, `T`, `fold_div`, `form`; `cin2`, `hi2`, `wi2`,
`stride2` for a second source; `segmented`), `P`, `R`, `n` = P * R, the tile `codes` to sweep, `inst` (a substring of the launch
the case's family makes), `env` (switches set for the case).  Its CLAIMS, written out by hand where the case is made:
  `big`   {tensor: 31 | 32}: the tensors of the launch ('x', 'y', 'residual', 'x2', 'd_part') whose size IN THE FORMAT THE KERNEL
          SEES (bf16: 2 bytes an element; the split-K scratch d_part: fp32 segment sums) exceeds 2^31 resp. 2^32 bytes; every
          other tensor stays at or below 2^31.  A bf16 tensor cannot pass 2^32 under conv_op_check's 2^31-element rule.
  `cap`   None, or for a family with a capacity rule 'inside' (the largest periodic size its rule accepts: the family must run)
          or 'outside' (the smallest it refuses: the family must NOT run, the fallback must, with the same checks)
  `need`  GiB of device memory the case needs at once (operands, output, the library's staging copies, compare scratch): the
          NEED table below, by hand; the CPU test recomputes it from the shapes (need_gib)."""
from tests._k_cases import conv_num_segments, kseg_of
from tests._walk_cases import _igemm_codes, out_hw, tail_split_applies

SPLITK, TAILK, POS = 0x100, 0x200, 0x80
EB = {'f32': 4, 'bf16x3': 4, 'bf16': 2}      # bytes per stored activation element (split-bf16: hi + lo)
# GEMM rows per tile of the row-tiled families (the 3x3 weight-stationary kernels tile frames; 'pos': 64 FRAMES per tile)
UNIT = {'igemm64': 64, 'igemm128': 128, '256': 256, '256p': 256, 'ws1x1': 128, 'stem': None, 'ws3x3': None, 'ws128': None,
        'ws128s2': None, 'pos': None}


def unit_rows(c):
    if c['family'] == 'wsn':
        return 128 if c['cin'] + c.get('cin2', 0) <= 256 else 64
    return UNIT[c['family']]


# ---- sizes ---------------------------------------------------------------------------------------------------------------------
def elements(c, frames=None):
    """Element counts of the launch's tensors over `frames` frames (default: all n), as conv_op_check counts them (the stem's
    input: the 8 staged slots per pixel) -- each must stay below 2^31."""
    n = c['n'] if frames is None else frames
    ho, wo = out_hw(c)
    e = {'x': n * c['hi'] * c['wi'] * (8 if c['k'] == 7 else c['cin']), 'y': n * ho * wo * c['cout']}
    if c['form'] in ('res', 'shift_res'):
        e['residual'] = e['y']
    if 'cin2' in c:
        e['x2'] = n * c['hi2'] * c['wi2'] * c['cin2']
    return e


def kernel_bytes(c, frames=None):
    """Bytes of every tensor the kernels address, in their own format.  The stem's packed input holds pixel PAIRS: 8 slots of the
    format per pair and row (fp32: 4 floats per pixel)."""
    e, eb = elements(c, frames), EB[c['dtype']]
    n = c['n'] if frames is None else frames
    b = {k: v * eb for k, v in e.items()}
    if c['k'] == 7:
        b['x'] = n * c['hi'] * c['wi'] * 16 if c['dtype'] == 'f32' else n * c['hi'] * ((c['wi'] + 1) // 2) * 8 * eb
    nseg = conv_num_segments_of(c)
    if nseg > 1 and any(code & (SPLITK | TAILK) for code in c['codes']):
        b['d_part'] = nseg * e['y'] * 4
    return b


def conv_num_segments_of(c):
    if c['dtype'] != 'f32':
        return 1
    from tests._k_cases import kp_total
    return conv_num_segments(kp_total(c), kseg_of(c))


def edges(c):
    """{tensor: 31 | 32} recomputed: which tensors pass which edge."""
    return {k: 32 if v > 1 << 32 else 31 for k, v in kernel_bytes(c).items() if v > 1 << 31}


def need_gib(c):
    """The caller's fp32 tensors, the library's staging copies (the bf16 formats, the stem's packed input), the split-K scratch,
    and 2 GiB for the compares' temporaries (a bool per output word, twice)."""
    e, kb = elements(c), kernel_bytes(c)
    raw = dict(e, x=c['n'] * c['hi'] * c['wi'] * 3) if c['k'] == 7 else e
    total = sum(v * 4 for v in raw.values())
    if c['dtype'] != 'f32':
        total += sum(v for k, v in kb.items() if k != 'd_part')
    elif c['k'] == 7:
        total += kb['x']
    total += kb.get('d_part', 0) + e['y'] * 2 // 4 * 4 + (2 << 30)
    return -(-total // (1 << 30))


# ---- the capacity rules, restated (tsm_conv_rules.h) ---------------------------------------------------------------------------
def rule_accepts(c, n=None):
    """Does the family's capacity rule accept the case at n frames?  (The shape conditions hold for every case of a family.)"""
    n = c['n'] if n is None else n
    ho, wo = out_hw(c)
    m, fam = n * ho * wo, c['family']
    if fam in ('ws1x1', 'ws3x3'):      # conv1x1_ws_valid, conv3x3_ws_valid: one descriptor over the output
        return m * 128.0 < 2.0e9 and (128 + 2.0 * c['hi'] * c['wi']) * c['cin'] * 2.0 < 2.0e9
    if fam in ('ws128', 'ws128s2'):    # conv3x3_ws128_common
        return m * 256.0 < 2.0e9 and c['hi'] * c['wi'] * 256.0 < 2.0e9
    if fam == 'pos':                   # pos_major_valid: y and all N input frames inside one descriptor
        return n % 64 == 0 and float(n) * c['hi'] * c['wi'] * c['cin'] * 4.0 < 2.0e9 and float(m) * c['cout'] * 4.0 < 2.0e9
    raise ValueError(fam)


def cap_step(c):
    """Frames between two periodic sizes of the case (position-major: whole periods that keep N % 64 == 0)."""
    return c['P'] * (64 if c['family'] == 'pos' else 1)


# ---- the table -----------------------------------------------------------------------------------------------------------------
def _case(name, family, dtype, k, stride, cin, cout, T, form, codes, inst, R, big, hw=(7, 9), cap=None, fold_div=8, segmented=False,
          env=None, cin2=None, stride2=1):
    ho, wo = hw
    hi, wi = (ho, wo) if stride == 1 else (2 * ho - 1, 2 * wo - 1)
    P = 3 * max(T, 1)
    c = dict(id=f'{name}-{dtype}-T{T}', family=family, dtype=dtype, k=k, stride=stride, cin=cin, cout=cout, hi=hi, wi=wi, T=T,
             fold_div=fold_div, form=form, codes=codes, inst=inst, P=P, R=R, n=P * R, big=big, cap=cap, segmented=segmented,
             env=env or {})
    if cin2:
        c.update(cin2=cin2, stride2=stride2, hi2=ho if stride2 == 1 else 2 * ho - 1, wi2=wo if stride2 == 1 else 2 * wo - 1)
    c['need'] = NEED[c['id']]
    return c


# GiB of device memory per case: the caller's fp32 tensors + the library's staging copies + the split-K scratch + compare scratch
NEED = {
    'igemm-shift1x1-x-f32-T8': 8, 'igemm-1x1-xy-f32-T0': 13, 'igemm-res1x1-y-bf16x3-T0': 23, 'igemm-shiftres-y-f32-T3': 14,
    'igemm-3x3s1-xy-bf16-T16': 17, 'igemm-3x3s2-x-f32-T0': 7, 'igemm-dual-s2-x2-bf16x3-T0': 12, 'igemm-dual-s1-x2-f32-T8': 9,
    'igemm-stem-y-f32-T0': 10, 'igemm-stem-y-bf16x3-T0': 14, 'igemm-stem-y-bf16-T0': 12, 'stem-direct-y-bf16-T0': 12,
    'stem-direct-y-bf16x3-T0': 14, 'seg-tail-x-f32-T0': 7, 'seg-dpart-f32-T0': 12, 'seg3x3-natural-x-f32-T0': 14,
    'pos-inside-f32-T0': 8, 'pos-inside-unbalanced-f32-T0': 8, 'pos-outside-f32-T0': 8,
    '256-1x1-xy-bf16-T0': 17, '256p-shift1x1-x-bf16-T8': 13, '256-res-y-bf16-T0': 20, '256-dual-y-bf16-T0': 14,
    '256p-shiftres-y-bf16-T3': 20, '256-3x3-y-bf16-T0': 12, 'wsn-512-128-x-bf16-T8': 11, 'wsn-512-256-x-bf16-T16': 13,
    'wsn-dual-l1-y-bf16-T0': 14, 'wsn-dual-l2-y-bf16-T0': 23, 'ws1x1-256-x-bf16-T8': 11, 'ws1x1-64-inside-bf16-T1': 16,
    'ws1x1-64-outside-bf16-T1': 16, 'ws3x3-inside-bf16-T0': 16, 'ws3x3-outside-bf16-T0': 16, 'ws128-inside-bf16-T0': 16,
    'ws128-outside-bf16-T0': 16, 'ws128s2-x-bf16-T0': 11, 'ws128s2-inside-bf16-T0': 18, 'ws128s2-outside-bf16-T0': 18,
}


SEG_CODES = [3, 4, 3 | SPLITK, 4 | SPLITK, 3 | TAILK]
POS_CODES = [3, 3 | POS, 3 | POS | TAILK]
BF = _igemm_codes('bf16', 256)           # conv_igemm's tiles of a 256-channel bf16 launch


def tail_reps(n_cu):
    """R of the tail-split case: the first R >= 5600 (x past 2^32 bytes) with a ragged last tile at which the split applies."""
    for r in range(5600, 5600 + 4096):
        m = 3 * r * 63
        if m % 32 and tail_split_applies(m, 64, 2, n_cu):
            return r
    raise ValueError(n_cu)


def cases(n_cu):
    """Every case for a device of n_cu compute units (only the tail-split case depends on it).  Frames are 7 x 9 outputs (13 x 17
    inputs at stride 2) unless said otherwise; P = 3 clips; the comments give M = n * 63 rows."""
    f32_1x1 = lambda cout: _igemm_codes('f32', cout) + ([9] if cout % 128 == 0 else [])
    out = [
        # ---- conv_igemm --------------------------------------------------------------------------------------------------------
        # the shifted 1x1, 256 -> 64 (the issue's worked example): M = 4 195 800, x = 1 074 124 800 elements
        _case('igemm-shift1x1-x', 'igemm64', 'f32', 1, 1, 256, 64, 8, 'shift', _igemm_codes('f32', 64),
              'KS = 1, SHIFT = true, RES = false', 2775, {'x': 32}),
        # the plain 1x1, 128 -> 128, every fp32 tile (64x128 included): x and y both past 2^32; M = 8 391 600
        _case('igemm-1x1-xy', 'igemm128', 'f32', 1, 1, 128, 128, 0, 'plain', f32_1x1(128),
              'KS = 1, SHIFT = false, RES = false', 44400, {'x': 32, 'y': 32}),
        # 1x1 + residual, 32 -> 128: y and the residual big; M = 8 391 600
        _case('igemm-res1x1-y', 'igemm128', 'bf16x3', 1, 1, 32, 128, 0, 'res', _igemm_codes('bf16x3', 128),
              'KS = 1, SHIFT = false, RES = true', 44400, {'y': 32, 'residual': 32}),
        # the shifted identity + 1x1 (block placement's conv3): the residual read through the shift
        _case('igemm-shiftres-y', 'igemm128', 'f32', 1, 1, 32, 128, 3, 'shift_res', _igemm_codes('f32', 128),
              'KS = 1, SHIFT = false', 14800, {'y': 32, 'residual': 32}),
        # the shifted 3x3 at stride 1, 64 -> 64: x and y past 2^31 (bf16); M = 16 786 224
        _case('igemm-3x3s1-xy', 'igemm64', 'bf16', 3, 1, 64, 64, 16, 'shift', _igemm_codes('bf16', 64),
              'KS = 3, SHIFT = true, RES = false', 5551, {'x': 31, 'y': 31}),
        # the 3x3 at stride 2, 128 -> 64 on 13 x 17 frames: x big; n = 37 971
        _case('igemm-3x3s2-x', 'igemm64', 'f32', 3, 2, 128, 64, 0, 'plain', _igemm_codes('f32', 64),
              'KS = 3, SHIFT = false, RES = false', 12657, {'x': 32}),
        # conv3 + downsample as one GEMM: the second source big, at stride 2 (plain) and stride 1 (shifted: block placement)
        _case('igemm-dual-s2-x2', 'igemm64', 'bf16x3', 1, 1, 32, 64, 0, 'dual', _igemm_codes('bf16x3', 64),
              'KS = 1, SHIFT = false, RES = false', 6329, {'x2': 32}, cin2=256, stride2=2),
        _case('igemm-dual-s1-x2', 'igemm64', 'f32', 1, 1, 32, 64, 8, 'dual', _igemm_codes('f32', 64),
              'KS = 1, SHIFT = false', 2775, {'x2': 32}, cin2=256, stride2=1),
        # the 7x7 stem through conv_igemm (the bf16 formats with TSM_STEM_DIRECT=0), 13 x 17 frames: y big; M = 16 786 224
        _case('igemm-stem-y', 'igemm64', 'f32', 7, 2, 3, 64, 0, 'plain', _igemm_codes('f32', 64), 'KS = 7', 88801, {'y': 32}),
        _case('igemm-stem-y', 'igemm64', 'bf16x3', 7, 2, 3, 64, 0, 'plain', _igemm_codes('bf16x3', 64), 'KS = 7', 88801, {'y': 32},
              env={'TSM_STEM_DIRECT': '0'}),
        _case('igemm-stem-y', 'igemm64', 'bf16', 7, 2, 3, 64, 0, 'plain', _igemm_codes('bf16', 64), 'KS = 7', 88801, {'y': 31},
              env={'TSM_STEM_DIRECT': '0'}),
        # ---- stem_direct_kernel (the bf16 formats' own stem) ---------------------------------------------------------------------
        _case('stem-direct-y', 'stem', 'bf16', 7, 2, 3, 64, 0, 'plain', [0], 'stem_direct_kernel<false, 4>', 88801, {'y': 31}),
        _case('stem-direct-y', 'stem', 'bf16x3', 7, 2, 3, 64, 0, 'plain', [0], 'stem_direct_kernel<true, 8>', 88801, {'y': 32}),
        # ---- segmented fp32 (the engine's long-K form): whole-K, split-K, the tail split -------------------------------------------
        # 1024 -> 64 (2 segments): x big; the tail split applies at this R (checked)
        _case('seg-tail-x', 'igemm64', 'f32', 1, 1, 1024, 64, 0, 'plain', SEG_CODES, 'kPrecF32, false, true>', tail_reps(n_cu),
              {'x': 32}, segmented=True),
        # 2048 -> 512 (4 segments): the segment scratch past 2^32 while y is not; M = 530 145
        _case('seg-dpart', 'igemm64', 'f32', 1, 1, 2048, 512, 0, 'plain', [3, 3 | SPLITK, 4 | SPLITK], 'kPrecF32, false, true>', 2805,
              {'x': 32, 'd_part': 32}, segmented=True),
        # the segmented 3x3 in NATURAL row order, 128 -> 64, at a size the position-major rule refuses: x and the segment scratch past
        # 2^32, y past 2^31; the position-major bit is ignored (N % 64 != 0, x past the rule); M = 8 391 789
        _case('seg3x3-natural-x', 'igemm64', 'f32', 3, 1, 128, 64, 0, 'plain', [3, 4, 3 | SPLITK, 3 | TAILK, 3 | POS],
              'kPrecF32, false, true>', 44401, {'x': 32, 'y': 31, 'd_part': 32}, segmented=True),
        # ---- position-major 3x3 (128 -> 64, segmented; N % 64 == 0): its rule keeps x below 2e9 bytes, so the edge IS the rule ----
        _case('pos-inside', 'pos', 'f32', 3, 1, 128, 64, 0, 'plain', POS_CODES, 'kPrecF32 | kPrecPosMajor, false, true>', 20608, {},
              cap='inside', segmented=True),
        _case('pos-inside-unbalanced', 'pos', 'f32', 3, 1, 128, 64, 0, 'plain', POS_CODES, 'kPrecF32 | kPrecPosMajor, false, true>',
              20608, {}, cap='inside', segmented=True, env={'TSM_POS_BALANCE': '0'}),
        _case('pos-outside', 'pos', 'f32', 3, 1, 128, 64, 0, 'plain', POS_CODES, 'kPrecF32 | kPrecPosMajor, false, true>', 20672, {},
              cap='outside', segmented=True),
        # ---- conv_bf16_256 (code 6) / conv_bf16_256p (code 8) -----------------------------------------------------------------------
        # 1x1 256 -> 256: x and y both past 2^31; M = 4 195 800
        _case('256-1x1-xy', '256p', 'bf16', 1, 1, 256, 256, 0, 'plain', BF + [6, 8], 'conv_bf16_256p_kernel<1, false>', 22200,
              {'x': 31, 'y': 31}),
        _case('256p-shift1x1-x', '256p', 'bf16', 1, 1, 512, 256, 8, 'shift', BF + [6, 8], 'conv_bf16_256p_kernel<1, true>', 1388,
              {'x': 31}),
        _case('256-res-y', '256', 'bf16', 1, 1, 128, 256, 0, 'res', BF + [6, 8], 'conv_bf16_256_kernel<1, false, true, false>', 22200,
              {'y': 31, 'residual': 31}),
        _case('256-dual-y', '256p', 'bf16', 1, 1, 64, 256, 0, 'dual', BF + [6, 8], 'conv_bf16_256p_kernel<1, false, false, true>',
              22200, {'y': 31}, cin2=64, stride2=1),
        _case('256p-shiftres-y', '256p', 'bf16', 1, 1, 128, 256, 3, 'shift_res', BF + [8],
              'conv_bf16_256p_kernel<1, true, true, false>', 7400, {'y': 31, 'residual': 31}),
        _case('256-3x3-y', '256', 'bf16', 3, 1, 64, 256, 0, 'plain', BF + [6, 8], 'conv_bf16_256_kernel<3, false>', 22200, {'y': 31}),
        # ---- conv1x1_wsn -----------------------------------------------------------------------------------------------------------
        _case('wsn-512-128-x', 'wsn', 'bf16', 1, 1, 512, 128, 8, 'shift', [1, 3, 7], 'conv1x1_wsn_kernel<512, 128, false>', 1388,
              {'x': 31}),
        _case('wsn-512-256-x', 'wsn', 'bf16', 1, 1, 512, 256, 16, 'shift', [1, 3, 7], 'conv1x1_wsn_kernel<512, 256, false>', 694,
              {'x': 31}),
        _case('wsn-dual-l1-y', 'wsn', 'bf16', 1, 1, 64, 256, 0, 'dual', [1, 3, 7], 'conv1x1_wsn_kernel<128, 256, true>', 22200,
              {'y': 31}, cin2=64, stride2=1),
        # (128 + 256 at stride 2 -> 512: the 13 x 17 second source passes 2^31 with the output)
        _case('wsn-dual-l2-y', 'wsn', 'bf16', 1, 1, 128, 512, 0, 'dual', [1, 3, 7], 'conv1x1_wsn_kernel<384, 256, true, 2>', 11100,
              {'y': 31, 'x2': 31}, cin2=256, stride2=2),
        # ---- conv1x1_ws: 256 -> 64 with x past 2^31 inside its rule; 64 -> 64 at the rule (M * 128 < 2.0e9) --------------------------
        _case('ws1x1-256-x', 'ws1x1', 'bf16', 1, 1, 256, 64, 8, 'shift', [3, 2, 7], 'conv1x1_ws_kernel<256>', 2775, {'x': 31}),
        _case('ws1x1-64-inside', 'ws1x1', 'bf16', 1, 1, 64, 64, 1, 'shift', [3, 2, 7], 'conv1x1_ws_kernel<64>', 82671, {},
              cap='inside'),
        _case('ws1x1-64-outside', 'ws1x1', 'bf16', 1, 1, 64, 64, 1, 'shift', [3, 2, 7], 'conv1x1_ws_kernel<64>', 82672, {},
              cap='outside'),
        # ---- the 3x3 weight-stationary kernels at their rules ------------------------------------------------------------------------
        _case('ws3x3-inside', 'ws3x3', 'bf16', 3, 1, 64, 64, 0, 'plain', [3, 2, 7], 'conv3x3_ws_kernel<false>', 82671, {}, cap='inside'),
        _case('ws3x3-outside', 'ws3x3', 'bf16', 3, 1, 64, 64, 0, 'plain', [3, 2, 7], 'conv3x3_ws_kernel<false>', 82672, {}, cap='outside'),
        _case('ws128-inside', 'ws128', 'bf16', 3, 1, 128, 128, 0, 'plain', [3, 2, 7, 1], 'conv3x3_ws128_kernel<false>', 41335, {},
              cap='inside'),
        _case('ws128-outside', 'ws128', 'bf16', 3, 1, 128, 128, 0, 'plain', [3, 2, 7, 1], 'conv3x3_ws128_kernel<false>', 41336, {},
              cap='outside'),
        # stride 2: x past 2^31 on 13 x 17 frames, well inside the rule; and AT the rule on 1 x 3 frames (1 x 2 outputs), where
        # x passes 2^31 as well
        _case('ws128s2-x', 'ws128s2', 'bf16', 3, 2, 128, 128, 0, 'plain', [3, 2, 7, 1], 'conv3x3_ws128_kernel<true>', 12657, {'x': 31}),
        _case('ws128s2-inside', 'ws128s2', 'bf16', 3, 2, 128, 128, 0, 'plain', [3, 2, 7, 1], 'conv3x3_ws128_kernel<true>', 1302083,
              {'x': 31}, hw=(1, 2), cap='inside'),
        _case('ws128s2-outside', 'ws128s2', 'bf16', 3, 2, 128, 128, 0, 'plain', [3, 2, 7, 1], 'conv3x3_ws128_kernel<true>', 1302084,
              {'x': 31}, hw=(1, 2), cap='outside'),
    ]
    return out
