"""Case table of tests/test_shift_div_gpu.py: every kernel arm that takes the temporal shift's fold at run time, at the
shift_div values the suite otherwise never leaves 8 for -- 1, 2, 4 and (fp32) 16.  Pure arithmetic (no torch, no GPU):
tests/test_shift_div_cases_cpu.py checks every claim of a case against the host rules restated below (tsm_conv_rules.h,
tsm_host_util.h: conv_op_check) and that the table's inputs tell a right fold from a wrong one.

What moves with shift_div: fold = channels of the shifted tensor // shift_div.  Channels [0, fold) read frame t + 1, [fold, 2 fold)
frame t - 1, the rest their own frame.  At div 8 the two boundaries sit at C / 8 and C / 4; at div 4 and 2 they sit in other k16
groups, planes and waves of every loader; at div 2 no channel reads its own frame; at div 1 fold = C: every channel reads t + 1
and the second group is empty (what the reference's slicing gives).

A per-op case is a dict: `id`, `family` (the kernel family it is for), `dtype`, the conv (`k`, `stride`, `cin`, `cout`, `n`,
`hi`, `wi`, `T`, `fold_div`, `form`; `cin2`, `hi2`, `wi2`, `stride2` for a second source; `segmented`), the tile `codes` to
sweep -- the first is the 64x64 conv_igemm tile every other one is compared with bit for bit -- `inst`, the substrings one
launch-trace line of the family's code must all hold, `persistent` (the family walks its tiles from a grid of one workgroup per
CU), and the CLAIMS, written where the case is made: `fold`, `rule` (the host rule of FOLD_RULES the fold must meet for the
family's kernel to run) and `expect`:
  'run'     the family's code runs `inst`,
  'refuse'  tsm_conv_op refuses the launch with `status` before anything is launched (2 * fold > the shifted channels: div 1).
`engine_div1` says what an ENGINE does with the family at div 1, where conv_op_check's rule does not stand in front of it:
'runs' (the loader's masks compute it), 'fallback' (the family's rule refuses 2 * fold > C: conv_igemm runs instead) or
'refused' (block placement's arms: tsm_set_shift_place refuses the engine up front).

Forms: 'shift' the input through the shift (Bottleneck / BasicBlock conv1), 's2shift' the shifted 1x1 at stride 2 (shift_target
1 with neither residual nor second source), 'shift_res' the shifted identity (a residual, shift_target 1), 'dual_shift' the
shifted second source (x2, shift_target 1)."""
from tests._k_cases import _arm, _ks
from tests._walk_cases import _fit, _igemm_codes, _in_hw

DIVS = {'f32': (1, 2, 4, 16), 'bf16x3': (1, 2, 4), 'bf16': (1, 2, 4)}
DTYPES = ('f32', 'bf16x3', 'bf16')
T = 3                         # a first, a middle and a last frame
CLIPS = 2
FRAME = (7, 5)                # 35 pixels: 210 rows, so that a 64- or 128-row tile holds frames of both clips
FRAME_S2 = (9, 7)             # the input of a stride-2 conv: 5 x 4 outputs, 120 rows
SPLITK, TAILK = 0x100, 0x200
INVALID_ARG = -1              # TSM_ERR_INVALID_ARG: conv_op_check's "2 * fold exceeds the shifted tensor's channels"
REFUSAL_TEXT = "2 * fold exceeds the shifted tensor's channels"


# ---- the host rules, restated -----------------------------------------------------------------------------------------------
def shifted_channels(c):
    """The channels of the tensor the shift moves (conv_op_check: shifted_c)."""
    return {'shift': c['cin'], 's2shift': c['cin'], 'shift_res': c['cout'], 'dual_shift': c.get('cin2')}[c['form']]


def fold_of(c):
    return shifted_channels(c) // c['fold_div']


def group_of(dtype):
    """Channels that move together: a 16-byte chunk of fp32, 8 channels of the bf16 formats."""
    return 4 if dtype == 'f32' else 8


def conv_op_admits(c):
    """conv_op_check's shift rules: whole groups, and both groups inside the tensor."""
    fold, ch = fold_of(c), shifted_channels(c)
    return c['n'] % c['T'] == 0 and fold % group_of(c['dtype']) == 0 and 2 * fold <= ch


FOLD_RULES = {
    # conv_args_refused: fold % 4 (fp32) / % 8; a shifted identity or second source also 2 fold <= its channels.  The A loader's
    # masks (c < fold, c < 2 fold) hold for any fold up to C.
    'igemm': lambda fold, ch, dtype, block: fold % group_of(dtype) == 0 and (not block or 2 * fold <= ch),
    'igemm_seg': lambda fold, ch, dtype, block: dtype == 'f32' and fold % 4 == 0 and not block,
    # conv1x1_ws_valid / conv1x1_wsn_valid: fold % 8 == 0 and 2 fold <= C
    'ws1x1': lambda fold, ch, dtype, block: dtype == 'bf16' and fold % 8 == 0 and 2 * fold <= ch and not block,
    'wsn': lambda fold, ch, dtype, block: dtype == 'bf16' and fold % 8 == 0 and 2 * fold <= ch and not block,
    # conv_bf16_256_valid / its persistent form: a shifted conv1 (no residual, no second source), any fold (lane masks)
    '256': lambda fold, ch, dtype, block: dtype == 'bf16' and not block,
    '256p': lambda fold, ch, dtype, block: dtype == 'bf16' and not block,
    # conv_bf16_256p_valid's block-placement arms: fold % 8 == 0 and 2 fold <= the shifted channels
    '256p_block': lambda fold, ch, dtype, block: dtype == 'bf16' and block and fold % 8 == 0 and 2 * fold <= ch,
}
# what an engine does with the family at div 1 (fold == C)
ENGINE_DIV1 = {'igemm': 'runs', 'igemm_block': 'refused', 'igemm_seg': 'runs', 'ws1x1': 'fallback', 'wsn': 'fallback', '256': 'runs',
               '256p': 'runs', '256p_block': 'refused'}


# the fused forms' fold rules (an engine's TSM_FUSE_* switches): which of them may run at a fold
def bneck_ws_fold_ok(cin, fold):
    return fold == cin // 8                      # bneck_ws_valid


def front_s2_fold_ok(fold):
    return fold == 32                            # front_s2_valid (cin 256)


def conv31_fold_ok(c, fold):
    return fold % 64 == 0 and 2 * fold <= c      # conv31_valid: a 64-channel chunk is shifted as a whole


def out_hw(c):
    pad = c['k'] // 2
    return (c['hi'] + 2 * pad - c['k']) // c['stride'] + 1, (c['wi'] + 2 * pad - c['k']) // c['stride'] + 1


def rows(c):
    ho, wo = out_hw(c)
    return c['n'] * ho * wo


def tiles_of(c):
    """Tiles of the case's persistent family (conv_route): 128 pixels (wsn at K > 256: 64), 256 x 256."""
    fam, m = c['family'], rows(c)
    if fam == 'ws1x1':
        return -(-m // 128)
    if fam == 'wsn':
        return -(-m // (128 if c['cin'] <= 256 else 64))
    if fam in ('256p', '256p_block'):
        return -(-m // 256) * (c['cout'] // 256)
    raise ValueError(fam)


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def _case(name, family, rule, dtype, div, k, stride, cin, cout, form, codes, inst, *, shape=None, cin2=None, stride2=1,
          segmented=False, persistent=False):
    if shape is None:         # two clips of small frames; a second source read at stride 2 is the larger tensor
        clips = CLIPS
        hi, wi = FRAME_S2 if stride == 2 else (5, 4) if cin2 and stride2 == 2 else FRAME
    else:
        clips, ho, wo = shape
        hi, wi = _in_hw(ho, wo, k, stride)
    c = dict(id=f'{name}-{dtype}-div{div}', family=family, rule=rule, dtype=dtype, k=k, stride=stride, cin=cin, cout=cout,
             n=clips * T, hi=hi, wi=wi, T=T, fold_div=div, form=form, segmented=segmented, codes=list(codes), inst=tuple(inst),
             persistent=persistent, big=shape is not None)
    if cin2 is not None:
        c.update(cin2=cin2, stride2=stride2)
        c['hi2'], c['wi2'] = _in_hw(*out_hw(c), 1, stride2)
    block = form in ('shift_res', 'dual_shift')
    c['fold'] = shifted_channels(c) // div
    c['expect'] = 'run' if 2 * c['fold'] <= shifted_channels(c) else 'refuse'
    c['status'] = None if c['expect'] == 'run' else INVALID_ARG
    c['engine_div1'] = ENGINE_DIV1['igemm_block' if family == 'igemm' and (block or form == 's2shift') else family]
    return c


def cases(n_cu):
    """Every per-op case for a device of n_cu compute units."""
    out = []
    big = lambda unit, tiles=n_cu + 1: _fit(tiles, unit, T, exact=False)       # more tiles than workgroups, the last one ragged
    for dtype in DTYPES:
        for div in DIVS[dtype]:
            ig = _igemm_codes(dtype, 64)
            ig = [3] + [t for t in ig if t != 3]
            # conv_igemm: the shifted 1x1 (Bottleneck conv1) at cin 64 and 256; fp32 div 16 at cin 64: fold 4, one chunk each way
            for cin in (64, 256):
                out.append(_case(f'igemm-1x1-{cin}', 'igemm', 'igemm', dtype, div, 1, 1, cin, 64, 'shift', ig,
                                 (_arm(dtype, 'shift'), _ks(1, 'shift'))))
            # the shifted 3x3 at stride 1 and 2 (BasicBlock conv1)
            for stride in (1, 2):
                out.append(_case(f'igemm-3x3-s{stride}', 'igemm', 'igemm', dtype, div, 3, stride, 64, 64, 'shift', ig,
                                 (_arm(dtype, 'shift'), _ks(3, 'shift'))))
            # the shifted 1x1 at stride 2 (BasicBlock downsample under block placement)
            out.append(_case('igemm-1x1-s2', 'igemm', 'igemm', dtype, div, 1, 2, 64, 64, 's2shift', ig,
                             (_arm(dtype, 's2shift'), _ks(1, 's2shift'))))
            # the shifted identity and the shifted second source (block placement's conv3 / conv3 + downsample)
            out.append(_case('igemm-shiftres', 'igemm', 'igemm', dtype, div, 1, 1, 64, 64, 'shift_res', ig,
                             (_arm(dtype, 'shift_res'), _ks(1, 'shift_res'))))
            for s2 in (1, 2):
                out.append(_case(f'igemm-dualshift-s{s2}', 'igemm', 'igemm', dtype, div, 1, 1, 64, 64, 'dual_shift', ig,
                                 (_arm(dtype, 'dual_shift'), _ks(1, 'dual_shift')), cin2=64, stride2=s2))
    # fp32 segmented forms: whole-K, split-K and the tail-split code, all the same bits
    for div in DIVS['f32']:
        for cin in (1024, 2048):
            out.append(_case(f'seg-1x1-{cin}', 'igemm_seg', 'igemm_seg', 'f32', div, 1, 1, cin, 64, 'shift', [3, 3 | SPLITK, 3 | TAILK],
                             (_arm('f32', 'shift', True), _ks(1, 'shift', True)), segmented=True))
    # the bf16 families with a loader of their own
    for div in DIVS['bf16']:
        for cin in (64, 256):
            out.append(_case(f'ws1x1-{cin}', 'ws1x1', 'ws1x1', 'bf16', div, 1, 1, cin, 64, 'shift', [3, 7], (f'conv1x1_ws_kernel<{cin}>',),
                             persistent=True))
        for cin, cout in ((256, 128), (512, 128), (512, 256)):
            out.append(_case(f'wsn-{cin}-{cout}', 'wsn', 'wsn', 'bf16', div, 1, 1, cin, cout, 'shift', [3, 7],
                             (f'conv1x1_wsn_kernel<{cin}, {cout}, false>',), persistent=True))
        for cin, cout in ((1024, 256), (2048, 512)):
            out.append(_case(f'256-{cin}-{cout}', '256', '256', 'bf16', div, 1, 1, cin, cout, 'shift', [3, 6], ('conv_bf16_256_kernel<1, true>',)))
            out.append(_case(f'256p-{cin}-{cout}', '256p', '256p', 'bf16', div, 1, 1, cin, cout, 'shift', [3, 8],
                             ('conv_bf16_256p_kernel<1, true>',), persistent=True))
        # block placement's arms on the persistent 256 x 256 tile (K >= 128)
        out.append(_case('256p-shiftres', '256p_block', '256p_block', 'bf16', div, 1, 1, 128, 256, 'shift_res', [3, 8],
                         ('conv_bf16_256p_kernel<1, true, true, false>',), persistent=True))
        out.append(_case('256p-dualshift', '256p_block', '256p_block', 'bf16', div, 1, 1, 64, 256, 'dual_shift', [3, 8],
                         ('conv_bf16_256p_kernel<1, true, false, true>',), cin2=64, stride2=2, persistent=True))
    # one case per persistent family with more tiles than workgroups (tiles of 7 x 5 .. frames, T = 3)
    out.append(_case('ws1x1-256-big', 'ws1x1', 'ws1x1', 'bf16', 2, 1, 1, 256, 64, 'shift', [3, 7], ('conv1x1_ws_kernel<256>',),
                     shape=big(128), persistent=True))
    out.append(_case('wsn-512-128-big', 'wsn', 'wsn', 'bf16', 4, 1, 1, 512, 128, 'shift', [3, 7],
                     ('conv1x1_wsn_kernel<512, 128, false>',), shape=big(64), persistent=True))
    out.append(_case('256p-128-256-big', '256p', '256p', 'bf16', 2, 1, 1, 128, 256, 'shift', [3, 8], ('conv_bf16_256p_kernel<1, true>',),
                     shape=big(256), persistent=True))
    out.append(_case('256p-shiftres-big', '256p_block', '256p_block', 'bf16', 4, 1, 1, 128, 256, 'shift_res', [3, 8],
                     ('conv_bf16_256p_kernel<1, true, true, false>',), shape=big(256), persistent=True))
    ids = [c['id'] for c in out]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    return out


# ---- the engine cases (tests/test_shift_div_gpu.py, engine part) ---------------------------------------------------------------
# B = 2; (T, H, W, state-dict seed, input seed): the inputs the CPU preconditions are about
GEOMETRIES = {'T3': (3, 64, 64, 7, 103), 'T4': (4, 64, 96, 7, 104)}
CONV1_TAPS = ('layer1.0.conv1', 'layer2.0.conv1', 'layer3.0.conv1', 'layer4.0.conv1')

# (base_model, shift_place, dtype, shift_div, geometry)
ENGINE_CASES = (
    [('resnet50', 'blockres', dt, div, geo) for dt in DTYPES for div in DIVS[dt] for geo in ('T3', 'T4')] +
    # ResNet-18 (the shifted 3x3 conv1) and Wide-ResNet-50-2
    [('resnet18', 'blockres', 'f32', 4, 'T3'), ('resnet18', 'blockres', 'f32', 16, 'T4'), ('resnet18', 'blockres', 'bf16', 2, 'T3'),
     ('resnet18', 'blockres', 'bf16x3', 2, 'T4'), ('wide_resnet50_2', 'blockres', 'bf16x3', 4, 'T3')] +
    # block placement: what tests/test_block_place_gpu.py's CASES leave open
    [('resnet50', 'block', 'bf16x3', 2, 'T3'), ('resnet50', 'block', 'bf16x3', 4, 'T4'), ('resnet50', 'block', 'bf16', 2, 'T4'),
     ('resnet50', 'block', 'f32', 2, 'T3'), ('resnet18', 'block', 'f32', 2, 'T4')])


def engine_id(e):
    return '-'.join(str(v) for v in e[:3]) + f'-div{e[3]}-{e[4]}'
