"""Case table of tests/test_walk_gpu.py: every conv kernel family tsm_conv_op reaches, at the tile counts where a persistent or
XCD-remapped tile walk goes wrong -- 1 tile, n_cu - 1, n_cu, n_cu + 1, 2 n_cu + 1 and a ragged last tile -- built from the
device's CU count.  Pure arithmetic (no torch, no GPU): tests/test_walk_cases_cpu.py checks that each case has the tile count
it claims, for several CU counts, with the launchers' own rules restated below.

A case is a dict: `family` (the tile rule its count is claimed for), `target` (a label), `tiles` (the count the label asks for),
the conv (`dtype`, `k`, `stride`, `cin`, `cout`, `n`, `hi`, `wi`, `T`, `fold_div`, `form`; `cin2`, `hi2`, `wi2`, `stride2` for a
second source), the tile `codes` to sweep and `inst`, a substring of the launch the case's family must make."""

WS_PATCH_MAX = 352      # kWsPatchMax (tsm_ws.hip): 11 DMA rounds of 32 patch pixels
W8_PATCH_MAX = 192      # kW8PatchMax: the 128-channel form's patch
S2_PATCH_MAX = 289      # kS2PatchMax: the 128-channel stride-2 form's patch

TARGETS = ('1', 'n-1', 'n', 'n+1', '2n+1', 'ragged')


def target_tiles(label, n_cu):
    return {'1': 1, 'n-1': n_cu - 1, 'n': n_cu, 'n+1': n_cu + 1, '2n+1': 2 * n_cu + 1, 'ragged': n_cu + 1}[label]


def ws_tile_geometry(h, w, max_px=256, max_patch=WS_PATCH_MAX):
    """ws_tile_geometry (tsm_ws.hip): TR x TC <= max_px outputs, (TR + 2) x (TC + 2) <= max_patch, fewest tiles per frame
    (ties: the smaller patch).  None when nothing fits."""
    best = None
    for tc in range(4, 129):
        tr = min(max_px // tc, h)
        if tr < 1 or (tr + 2) * (tc + 2) > max_patch:
            continue
        tiles, patch = -(-h // tr) * -(-w // tc), (tr + 2) * (tc + 2)
        if best is None or tiles < best[0] or (tiles == best[0] and patch < best[1]):
            best = (tiles, patch, tr, tc)
    return None if best is None else best[2:]


def ws128_tiles_per_frame(h, w):
    """Tiles per frame of conv3x3_ws128_kernel<false> (ws128_tile_geometry): the fewest over TR = 128 / TC (<= H),
    (TR + 2) x (TC + 2) <= W8_PATCH_MAX.  (Which of the tied shapes runs is a bank-conflict model's choice; the count is not.)"""
    counts = [-(-h // min(128 // tc, h)) * -(-w // tc) for tc in range(4, 129)
              if 128 // tc >= 1 and (min(128 // tc, h) + 2) * (tc + 2) <= W8_PATCH_MAX]
    return min(counts) if counts else None


def ws_s2_tiles_per_frame(ho, wo):
    """Tiles per output frame of conv3x3_ws128_kernel<true> (ws_s2_tile_geometry)."""
    best = None
    for tc in range(1, 65):
        lanes = 8 if tc <= 8 else 16 if tc <= 16 else 32 if tc <= 32 else 64
        tr = min(64 // lanes, ho)
        if tr < 1 or (2 * tr + 1) * (2 * tc + 1) > S2_PATCH_MAX or 2 * tr * (2 * tc + 1) + lanes + tc >= S2_PATCH_MAX:
            continue
        tiles = -(-ho // tr) * -(-wo // tc)
        best = tiles if best is None else min(best, tiles)
    return best


def out_hw(c):
    pad = c['k'] // 2
    return (c['hi'] + 2 * pad - c['k']) // c['stride'] + 1, (c['wi'] + 2 * pad - c['k']) // c['stride'] + 1


def rows(c):
    ho, wo = out_hw(c)
    return c['n'] * ho * wo


def count_tiles(c):
    """The tile count of the case's family, by the launcher's rule."""
    fam, m = c['family'], rows(c)
    if fam.startswith('igemm') or fam in ('256', '256p'):
        bm, bn = {'igemm64': (64, 64), 'igemm128': (128, 128), '256': (256, 256), '256p': (256, 256)}[fam]
        return -(-m // bm) * (c['cout'] // bn)
    if fam == 'ws1x1':
        return -(-m // 128)
    if fam == 'wsn':
        kp = c['cin'] + c.get('cin2', 0)
        return -(-m // (128 if kp <= 256 else 64))
    ho, wo = out_hw(c)
    if fam == 'ws3x3':
        tr, tc = ws_tile_geometry(ho, wo)
        return c['n'] * -(-ho // tr) * -(-wo // tc)
    if fam == 'ws128':
        return c['n'] * ws128_tiles_per_frame(ho, wo)
    if fam == 'ws128s2':
        return c['n'] * ws_s2_tiles_per_frame(ho, wo)
    raise ValueError(fam)


def ragged(c):
    """Is the last tile of the case's family only partly filled?"""
    fam, m = c['family'], rows(c)
    unit = {'igemm64': 64, 'igemm128': 128, '256': 256, '256p': 256, 'ws1x1': 128,
            'wsn': 128 if c['cin'] + c.get('cin2', 0) <= 256 else 64}.get(fam)
    if unit:
        return m % unit != 0
    ho, wo = out_hw(c)
    if fam == 'ws3x3':
        tr, tc = ws_tile_geometry(ho, wo)
        return ho % tr != 0 or wo % tc != 0
    return count_tiles(dict(c, n=1)) * 128 > ho * wo if fam == 'ws128' else ho * wo < 64 * count_tiles(dict(c, n=1))


def tail_split_applies(m, cout, nseg, n_cu):
    """tail_split_from (tsm_host_util.h): whole rounds of 5 n_cu 64x64 workgroups, then a tail of at most 85 % of a round
    split over the K segments."""
    ntn, ntm = cout // 64, (m + 63) // 64
    tiles, slots = ntm * ntn, 5 * n_cu
    rounds, rem = tiles // slots, tiles % slots
    if nseg < 2 or rounds < 1 or rem == 0 or rem * 100 > slots * 85:
        return False
    frm = rounds * slots // ntn * ntn
    return 0 < frm < tiles


# frames (output size) the row-tiled cases are built from, tried in order: odd and square, single-pixel, 2 x 3 ...
FRAMES = ((7, 7), (5, 3), (3, 5), (2, 3), (1, 1), (4, 4), (1, 2))


def _fit(tiles, unit, T, exact):
    """(clips, ho, wo) with clips * T * ho * wo rows in ((tiles - 1) unit, tiles unit]: exactly tiles * unit when `exact`, else
    with a ragged last tile."""
    for ho, wo in FRAMES:
        per = T * ho * wo
        if exact:
            if (tiles * unit) % per == 0:
                return tiles * unit // per, ho, wo
            continue
        clips = -(-((tiles - 1) * unit + 1) // per)
        m = clips * per
        if m <= tiles * unit and m % unit:
            return clips, ho, wo
    raise ValueError(f'no frame gives {tiles} tiles of {unit} rows at T = {T}')


def _in_hw(ho, wo, k, stride):
    """The input size that gives ho x wo (an odd one at stride 2: the last output reads the last input column)."""
    return (ho, wo) if stride == 1 else (2 * ho - 1, 2 * wo - 1)


def _row_case(name, label, n_cu, family, unit, dtype, k, stride, cin, cout, T, form, codes, inst, fold_div=8, **extra):
    ntn = cout // {'igemm64': 64, 'igemm128': 128, '256': 256, '256p': 256}[family] if family in BN_OF else 1
    t = target_tiles(label, n_cu) // ntn     # (every case but the tail split has one column of tiles)
    clips, ho, wo = _fit(t, unit, max(T, 1), exact=label == 'n')
    hi, wi = _in_hw(ho, wo, k, stride)
    c = dict(id=f'{name}-{label}-{dtype}-T{T}', family=family, target=label, tiles=target_tiles(label, n_cu), dtype=dtype, k=k,
             stride=stride, cin=cin, cout=cout, n=clips * max(T, 1), hi=hi, wi=wi, T=T, fold_div=fold_div, form=form, codes=codes,
             inst=inst)
    for key in ('cin2', 'stride2'):
        if key in extra:
            c[key] = extra[key]
    if 'cin2' in c:
        c['hi2'], c['wi2'] = _in_hw(ho, wo, 1, c['stride2'])
    return c


def _igemm_codes(dtype, cout):
    return [c for c in (1, 2, 3, 4, 5) if (cout % 128 == 0 or c in (2, 3, 4)) and (c != 4 or dtype == 'f32')]


BN_OF = ('igemm64', 'igemm128', '256', '256p')
DTYPES = ('f32', 'bf16x3', 'bf16')
TS = (1, 3, 8, 16)


def cases(n_cu):
    """Every case for a device of n_cu compute units.  The comments give each case's tile count on a 256-CU part."""
    out = []
    for i, label in enumerate(TARGETS):
        dt = DTYPES[i % 3]
        T = TS[i % 4]
        # conv_igemm, 128x128 (code 1): the shifted 1x1 (Bottleneck.conv1); 1 / 255 / 256 / 257 / 513 / 257 (ragged) tiles
        out.append(_row_case('igemm-shift1x1', label, n_cu, 'igemm128', 128, dt, 1, 1, 64, 128, T, 'shift', _igemm_codes(dt, 128),
                             'KS = 1, SHIFT = true, RES = false'))
        # conv_igemm, 64x64 (code 3): 1x1 + residual (conv3); 1 / 255 / 256 / 257 / 513 / 257 tiles
        out.append(_row_case('igemm-res1x1', label, n_cu, 'igemm64', 64, DTYPES[(i + 1) % 3], 1, 1, 128, 64, 0, 'res',
                             _igemm_codes(DTYPES[(i + 1) % 3], 64), 'KS = 1, SHIFT = false, RES = true'))
        # conv_igemm, 64x64: the shifted 3x3 at stride 1 (BasicBlock.conv1); 1 / 255 / 256 / 257 / 513 / 257 tiles
        out.append(_row_case('igemm-3x3s1', label, n_cu, 'igemm64', 64, DTYPES[(i + 2) % 3], 3, 1, 64, 64, T, 'shift',
                             _igemm_codes(DTYPES[(i + 2) % 3], 64), 'KS = 3, SHIFT = true, RES = false'))
        # conv_igemm, 128x128: the 3x3 at stride 2; 1 / 255 / 256 / 257 / 513 / 257 tiles
        out.append(_row_case('igemm-3x3s2', label, n_cu, 'igemm128', 128, dt, 3, 2, 64, 128, 0, 'plain', _igemm_codes(dt, 128),
                             'KS = 3, SHIFT = false, RES = false'))
        # conv_igemm, 64x64: the shifted 1x1 at stride 2 (BasicBlock downsample under block placement); 1 .. 513 tiles
        out.append(_row_case('igemm-1x1s2', label, n_cu, 'igemm64', 64, DTYPES[(i + 1) % 3], 1, 2, 64, 64, T, 's2shift',
                             _igemm_codes(DTYPES[(i + 1) % 3], 64), 'KS = 1, SHIFT = true, RES = false'))
        # conv_igemm, 128x128: conv3 + downsample as one GEMM (T = 0); 1 .. 513 tiles
        out.append(_row_case('igemm-dual', label, n_cu, 'igemm128', 128, DTYPES[(i + 2) % 3], 1, 1, 64, 128, 0, 'dual',
                             _igemm_codes(DTYPES[(i + 2) % 3], 128), 'KS = 1, SHIFT = false, RES = false', cin2=64, stride2=2))
    for label in ('1', 'n', 'n+1'):
        for dt in DTYPES:
            # conv_igemm, 64x64: the 7x7 stem (bf16 formats through igemm with TSM_STEM_DIRECT=0); 1 / 256 / 257 tiles
            out.append(_row_case('igemm-stem', label, n_cu, 'igemm64', 64, dt, 7, 2, 3, 64, 0, 'plain', _igemm_codes(dt, 64), 'KS = 7'))
    # fp32 segmented layers: tsm_conv_op segments the K-concatenated GEMM only (512 + 512 channels = 32 K-steps: 2 segments
    # of 16); whole-K 64x64 / 32x32, split-K, the tail split
    seg_codes = [3, 4, 3 | 0x100, 4 | 0x100, 3 | 0x200]
    for label in ('1', 'n+1'):
        # 1 / 257 tiles of 64 x 64
        out.append(_row_case('igemm-seg', label, n_cu, 'igemm64', 64, 'f32', 1, 1, 512, 64, 0, 'dual', seg_codes,
                             'kPrecF32, true, true>', cin2=512, stride2=1))
    # the tail split: 5 resident 64x64 workgroups per CU; one whole round and 40 % of a second (1792 tiles on 256 CUs, 4 columns)
    tail = _row_case('igemm-tail', 'n', n_cu, 'igemm64', 64, 'f32', 1, 1, 512, 256, 0, 'dual', seg_codes,
                     'kPrecF32, true, true>', cin2=512, stride2=1)
    tail_tiles = 5 * n_cu * 7 // 5
    clips, ho, wo = _fit(tail_tiles // 4, 64, 1, exact=False)
    tail.update(id='igemm-tail-f32', target='tail', tiles=tail_tiles // 4 * 4, n=clips, hi=ho, wi=wo, hi2=ho, wi2=wo)
    assert tail_split_applies(rows(tail), tail['cout'], 2, n_cu)
    out.append(tail)

    # conv_bf16_256 (code 6) and conv_bf16_256p (code 8): 256 x 256 tiles; 256p's grid is min(tiles, n_cu & ~7)
    for i, label in enumerate(TARGETS):
        T = TS[i % 4]
        bf = _igemm_codes('bf16', 256)
        # 1x1 (conv1 form, plain 128 -> 256); 1 / 255 / 256 / 257 / 513 / 257 tiles
        out.append(_row_case('256-1x1', label, n_cu, '256p', 256, 'bf16', 1, 1, 128, 256, 0, 'plain', bf + [6, 8],
                             'conv_bf16_256p_kernel<1, false>'))
        # the shifted 1x1 (conv1) on 256p; the same counts
        out.append(_row_case('256p-shift1x1', label, n_cu, '256p', 256, 'bf16', 1, 1, 128, 256, T, 'shift', bf + [6, 8],
                             'conv_bf16_256p_kernel<1, true>'))
    for i, label in enumerate(('1', 'n-1', 'n+1', 'ragged')):
        T = TS[i % 4]
        bf = _igemm_codes('bf16', 256)
        # the shifted identity 1x1 + residual (block placement's conv3); 1 / 255 / 257 / 257 tiles
        out.append(_row_case('256p-shiftres', label, n_cu, '256p', 256, 'bf16', 1, 1, 128, 256, T, 'shift_res', bf + [8],
                             'conv_bf16_256p_kernel<1, true, true, false>'))
        # conv3 + downsample (unshifted: 256 and 256p), 64 + 64 -> 256; 1 / 255 / 257 / 257 tiles
        out.append(_row_case('256-dual', label, n_cu, '256p', 256, 'bf16', 1, 1, 64, 256, 0, 'dual', bf + [6, 8],
                             'conv_bf16_256p_kernel<1, false, false, true>', cin2=64, stride2=1))
        # 1x1 + residual; the same counts
        out.append(_row_case('256-res', label, n_cu, '256', 256, 'bf16', 1, 1, 128, 256, 0, 'res', bf + [6, 8],
                             'conv_bf16_256_kernel<1, false, true, false>'))
    for label in ('1', 'n+1'):
        bf = _igemm_codes('bf16', 256)
        # 3x3 at stride 1 and 2 (64 -> 256: K = 576); 1 / 257 tiles
        out.append(_row_case('256-3x3s1', label, n_cu, '256', 256, 'bf16', 3, 1, 64, 256, 0, 'plain', bf + [6, 8],
                             'conv_bf16_256_kernel<3, false>'))
        out.append(_row_case('256p-3x3s2', label, n_cu, '256p', 256, 'bf16', 3, 2, 64, 256, 0, 'plain', bf + [6, 8],
                             'conv_bf16_256p_kernel<3, false>'))

    # weight-stationary kernels (code 7), bf16
    for i, label in enumerate(TARGETS):
        T = TS[i % 4]
        # conv1x1_ws 64 -> 64 and 256 -> 64, shifted: 128-row tiles; 1 / 255 / 256 / 257 / 513 / 257 tiles
        out.append(_row_case('ws1x1-64', label, n_cu, 'ws1x1', 128, 'bf16', 1, 1, 64, 64, T, 'shift', [3, 2, 7],
                             'conv1x1_ws_kernel<64>'))
        out.append(_row_case('ws1x1-256', label, n_cu, 'ws1x1', 128, 'bf16', 1, 1, 256, 64, T, 'shift', [3, 2, 7],
                             'conv1x1_ws_kernel<256>'))
        # conv1x1_wsn: 256 -> 128 (128-pixel tiles), 512 -> 128 and 512 -> 256 (64-pixel tiles), shifted; the same counts
        out.append(_row_case('wsn-256-128', label, n_cu, 'wsn', 128, 'bf16', 1, 1, 256, 128, T, 'shift', [1, 3, 7],
                             'conv1x1_wsn_kernel<256, 128, false>'))
        out.append(_row_case('wsn-512-128', label, n_cu, 'wsn', 64, 'bf16', 1, 1, 512, 128, T, 'shift', [1, 3, 7],
                             'conv1x1_wsn_kernel<512, 128, false>'))
        out.append(_row_case('wsn-512-256', label, n_cu, 'wsn', 64, 'bf16', 1, 1, 512, 256, T, 'shift', [1, 3, 7],
                             'conv1x1_wsn_kernel<512, 256, false>'))
        # the dual forms: 64 + 64 -> 256 (128-pixel tiles) and 128 + 256 -> 512 in two halves of 256 (64-pixel tiles; the
        # grid: pairs of workgroups, a multiple of 8 pairs); the same counts
        out.append(_row_case('wsn-dual-l1', label, n_cu, 'wsn', 128, 'bf16', 1, 1, 64, 256, 0, 'dual', [1, 3, 7],
                             'conv1x1_wsn_kernel<128, 256, true>', cin2=64, stride2=1))
        out.append(_row_case('wsn-dual-l2', label, n_cu, 'wsn', 64, 'bf16', 1, 1, 128, 512, 0, 'dual', [1, 3, 7],
                             'conv1x1_wsn_kernel<384, 256, true, 2>', cin2=256, stride2=2))
    # the 3x3 weight-stationary kernels: frames small enough for one tile each count frames; the ragged case has partial tiles
    for i, label in enumerate(TARGETS):
        t = target_tiles(label, n_cu)
        if label == 'ragged':
            # (257 tiles on 256 CUs rounded up to whole frames)
            ws = dict(family='ws3x3', hi=19, wi=19)       # 19 x 19 frames: 2 tiles of 19 x 10, the second 9 columns wide
            w8 = dict(family='ws128', hi=12, wi=12)       # 12 x 12: 2 tiles per frame, 144 of 256 pixels filled
            s2 = dict(family='ws128s2', hi=19, wi=19)     # 10 x 10 outputs: 3 tiles per frame, 100 of 192 pixels filled
        else:
            ws = dict(family='ws3x3', hi=4, wi=4)         # one tile per frame: 1 / 255 / 256 / 257 / 513 tiles
            w8 = dict(family='ws128', hi=4, wi=4)
            s2 = dict(family='ws128s2', hi=7, wi=7)       # 4 x 4 outputs
        for name, geo, cio, stride, inst in (('ws3x3', ws, 64, 1, 'conv3x3_ws_kernel<false>'),
                                              ('ws128', w8, 128, 1, 'conv3x3_ws128_kernel<false>'),
                                              ('ws128s2', s2, 128, 2, 'conv3x3_ws128_kernel<true>')):
            c = dict(id=f'{name}-{label}-bf16', family=geo['family'], target=label, tiles=t, dtype='bf16', k=3, stride=stride,
                     cin=cio, cout=cio, n=1, hi=geo['hi'], wi=geo['wi'], T=0, fold_div=8, form='plain',
                     codes=[3, 2, 7] + ([1] if cio == 128 else []), inst=inst)
            per = count_tiles(c)
            c['n'] = max(1, -(-t // per))
            c['tiles'] = c['n'] * per if label == 'ragged' else t
            out.append(c)
    return out
