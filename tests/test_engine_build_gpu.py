"""The construction side of the host engine through the raw C ABI: which names tsm_set_tensor takes per family, and what
tsm_finalize answers to a state dict with exactly one defect -- status and full tsm_last_error text.

Every case is a tsm_create, host-side calls and at most one or two tsm_finalize of the smallest engine of its family
(64 x 64, max_clips = 1; ConvNeXt and TDN with depths (1, 1, 1, 1)).  No forward runs.  The expected texts are literals: they are
part of the ABI's behaviour (engine.load_state_dict matches on 'unknown tensor name')."""
import ctypes as C
import functools

import numpy as np
import pytest

from workoutdetector_amd import _lib
from workoutdetector_amd import weights as W

pytestmark = pytest.mark.gpu

OK, INVALID, MISSING, SHAPE, CAPACITY = 0, -1, -4, -5, -6
ONES = (1, 1, 1, 1)

# name -> (tsm_create's num_segments / is_shift, the setters, the options of weights.required_keys / make_state_dict)
ENGINES = {
    'r18': dict(base_model='resnet18'),
    'r50': dict(base_model='resnet50'),
    'r50_block': dict(base_model='resnet50', shift_place='block'),
    'r50_nl': dict(base_model='resnet50', non_local=True),
    'r50_nl_block': dict(base_model='resnet50', non_local=True, shift_place='block'),
    'r50_tpool': dict(base_model='resnet50', temporal_pool=True),
    'wrn': dict(base_model='wide_resnet50_2'),
    'convnext': dict(base_model=W.CONVNEXT),
    'tdn': dict(base_model=W.TDN),
}
RESNETS = [k for k in ENGINES if k not in ('convnext', 'tdn')]


class Engine:
    """One tsm_engine behind the raw C calls; `with` destroys it."""

    def __init__(self, lib, name, height=64, width=64, max_clips=1, num_class=12):
        self.lib, opt = lib, ENGINES[name]
        base = opt['base_model']
        T, shift = {W.CONVNEXT: (1, 0), W.TDN: (2, 0)}.get(base, (8, 1))
        cfg = _lib.TsmConfig(C.sizeof(_lib.TsmConfig), num_class, T, height, width, 8, shift, max_clips, 0, _lib.DTYPE_F32)
        self.h = C.c_void_p()
        _lib.check(lib.tsm_create(C.byref(cfg), C.byref(self.h)))
        if base == W.CONVNEXT:
            _lib.check(lib.tsm_set_convnext(self.h, (C.c_int32 * 4)(*ONES)), self.h)
        elif base == W.TDN:
            _lib.check(lib.tsm_set_tdn(self.h, (C.c_int32 * 4)(*ONES), 0.75, 0.25), self.h)
        elif W.DEPTHS[base] != 50:
            _lib.check(lib.tsm_set_backbone(self.h, W.DEPTHS[base]), self.h)
        if base in W.WIDTHS:
            _lib.check(lib.tsm_set_bottleneck_width(self.h, W.WIDTHS[base]), self.h)
        if opt.get('shift_place') == 'block':
            _lib.check(lib.tsm_set_shift_place(self.h, 1), self.h)
        if opt.get('non_local'):
            _lib.check(lib.tsm_set_non_local(self.h, 1), self.h)
        if opt.get('temporal_pool'):
            _lib.check(lib.tsm_set_temporal_pool(self.h, 1), self.h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.tsm_destroy(self.h)

    def set(self, name, arr=None):
        arr = np.zeros(1, np.float32) if arr is None else np.ascontiguousarray(arr, dtype=np.float32)
        return self.lib.tsm_set_tensor(self.h, name.encode(), arr.ctypes.data, (C.c_int64 * arr.ndim)(*arr.shape), arr.ndim)

    def load(self, sd):
        for k, v in sd.items():
            assert self.set(k, v) == OK, (k, self.error())

    def finalize(self):
        return self.lib.tsm_finalize(self.h)

    def error(self):
        return (self.lib.tsm_last_error(self.h) or b'').decode()


def spec_keys(name):
    """The Python side's list of the tensors an engine reads."""
    opt = ENGINES[name]
    if opt['base_model'] == W.CONVNEXT:
        return [k for k, _s, _k in W.convnext_specs(ONES)] + ['head.fc.weight', 'head.fc.bias']
    if opt['base_model'] == W.TDN:
        return [k for k, _s, _k in W.tdn_specs(ONES)] + ['new_fc.weight', 'new_fc.bias']
    return list(W.required_keys(True, opt['base_model'], opt.get('shift_place', 'blockres'), opt.get('non_local', False)))


def bn_prefixes(name):
    opt = ENGINES[name]
    if opt['base_model'] == W.CONVNEXT:
        return []
    if opt['base_model'] == W.TDN:
        return [k[:-len('.weight')] for k, _s, kind in W.tdn_specs(ONES) if kind == 'bn_w']
    nl = [p + '.W.1' for p, _c, _d in W.nonlocal_specs(opt['base_model'])] if opt.get('non_local') else []
    return [bnp for _w, bnp, *_ in W.conv_specs(opt['base_model'], opt.get('shift_place', 'blockres'), opt.get('non_local', False))] + nl


def alternates(name, key):
    """Every other spelling of `key` the engine takes: without the shift wrapper's `.net` (`conv1.weight` for
    `conv1.net.weight`), without the non-local wrapper's `.block`, without both; on the temporal-pool engine each spelling of a
    layer2 key once more under `base_model.layer2.net.<b>.`."""
    opt = ENGINES[name]

    def no_net(k):
        if opt.get('shift_place') == 'block':
            return k.replace('.net.', '.', 1) if '.net.' in k else None
        return k[:-len('.conv1.net.weight')] + '.conv1.weight' if k.endswith('.conv1.net.weight') else None

    def no_block(k):
        return k.replace('.block.', '.', 1) if '.block.' in k else None

    alts = [no_net(key), no_block(key), no_net(no_block(key)) if no_block(key) else None]
    if opt.get('temporal_pool') and key.startswith('base_model.layer2.'):
        alts += ['base_model.layer2.net.' + k[len('base_model.layer2.'):] for k in (key, no_net(key)) if k]
    return [a for a in alts if a]


REFUSED = {name: ['base_model.layer2.0.nl.theta.weight', 'base_model.layer2.0.nl.W.1.running_mean', 'head.fc.weight', 'new_fc.weight',
                  'base_model.conv1_temp.weight', 'base_model.layer2_bak.0.mse.conv1.weight', 'base_model.layer2.0.mse.bn1.weight',
                  'base_model.conv1.bias', 'base_model.layer1.0.conv2.bias', 'base_model.layer2.net.0.conv2.weight',
                  'base_model.layer2.net.0.bn2.weight'] for name in RESNETS}
for _name in ('r50_nl', 'r50_nl_block'):
    REFUSED[_name] = [k for k in REFUSED[_name] if '.nl.' not in k] + ['base_model.layer1.0.nl.theta.weight', 'base_model.layer2.1.nl.W.0.weight']
for _name in ('r50_block', 'r50_nl_block'):      # the other placement's spelling
    REFUSED[_name] += ['base_model.layer1.0.conv1.net.weight', 'base_model.layer2.1.conv1.net.weight']
REFUSED['r50_tpool'] = [k for k in REFUSED['r50_tpool'] if '.layer2.net.' not in k] + ['base_model.layer3.net.0.conv2.weight',
                                                                                      'base_model.layer1.net.0.bn2.weight']
REFUSED['convnext'] = ['fc.weight', 'fc.bias', 'new_fc.weight', 'base_model.conv1.weight', 'stages.0.downsample.0.weight',
                       'stages.0.blocks.1.gamma', 'stem.0.gamma', 'stem.1.running_mean', 'base_model.layer2.0.nl.theta.weight']
REFUSED['tdn'] = ['fc.weight', 'fc.bias', 'head.fc.weight', 'base_model.conv1_5.0.bias', 'base_model.layer1_bak.0.mse.conv1.weight',
                  'base_model.resnext_layer1.0.shift.conv.weight', 'base_model.layer1.0.conv1.net.weight',
                  'base_model.layer2.0.nl.theta.weight', 'base_model.conv1_temp.running_mean']


@pytest.mark.parametrize('name', list(ENGINES))
def test_set_tensor_accepts_and_refuses(hip_lib, name):
    keys = spec_keys(name)
    assert len(set(keys)) == len(keys)
    with Engine(hip_lib, name) as e:
        for k in keys:
            assert e.set(k) == OK, (k, e.error())
        n_alt = 0
        for k in keys + [p + '.num_batches_tracked' for p in bn_prefixes(name)]:
            for a in alternates(name, k):
                assert e.set(a) == OK, (k, a, e.error())
                n_alt += 1
        for p in bn_prefixes(name):
            assert e.set(p + '.num_batches_tracked') == OK, (p, e.error())
        if name == 'tdn':
            assert e.set('base_model.conv1_temp.weight') == OK and e.set('base_model.conv1_temp.bias') == OK
        # (the table above is not vacuous: every ResNet spells conv1 of each block with a wrapper)
        assert (n_alt > 0) == (name in RESNETS), n_alt
        for k in REFUSED[name]:
            assert e.set(k) == INVALID, k
            assert e.error() == 'unknown tensor name: ' + k


def test_alternate_spellings_counted():
    """The spellings per engine key, by family: one without `.net`; three around a non-local block; doubled under the pool."""
    assert alternates('r50', 'base_model.layer2.0.conv1.net.weight') == ['base_model.layer2.0.conv1.weight']
    assert alternates('r50', 'base_model.layer2.0.conv2.weight') == []
    assert alternates('r50_block', 'base_model.layer2.0.net.bn2.bias') == ['base_model.layer2.0.bn2.bias']
    assert alternates('r50_nl', 'base_model.layer2.0.block.conv1.net.weight') == [
        'base_model.layer2.0.block.conv1.weight', 'base_model.layer2.0.conv1.net.weight', 'base_model.layer2.0.conv1.weight']
    assert alternates('r50_nl_block', 'base_model.layer2.0.block.net.bn1.weight') == [
        'base_model.layer2.0.block.bn1.weight', 'base_model.layer2.0.net.bn1.weight', 'base_model.layer2.0.bn1.weight']
    assert alternates('r50_tpool', 'base_model.layer2.1.conv1.net.weight') == [
        'base_model.layer2.1.conv1.weight', 'base_model.layer2.net.1.conv1.net.weight', 'base_model.layer2.net.1.conv1.weight']
    assert alternates('r50_tpool', 'base_model.layer3.1.conv2.weight') == []


@functools.lru_cache(maxsize=None)
def seeded(name):
    """The seeded state dict of a family, made once; the rows below copy the dict, never an array."""
    opt = ENGINES[name]
    if opt['base_model'] == W.TDN:
        return W.make_tdn_state_dict(0, 12, ONES)
    if opt['base_model'] == W.CONVNEXT:
        return W.make_state_dict(0, 12, base_model=W.CONVNEXT, depths=ONES)
    return W.make_state_dict(0, 12, base_model=opt['base_model'], non_local=opt.get('non_local', False))


def drop(key):
    return lambda sd: sd.pop(key)


def reshape(key, shape):
    def apply(sd):
        sd[key] = np.zeros(shape, np.float32)
    return apply


NL = 'base_model.layer2.0.nl'
CNX = 'stages.0.blocks.0'
TDN1, TDN2 = 'base_model.layer1_bak.0', 'base_model.layer2_bak.0'
# (engine, the one defect, status, tsm_last_error)
DEFECTS = [
    ('r18', drop('base_model.layer1.0.conv2.weight'), MISSING, 'missing base_model.layer1.0.conv2.weight'),
    ('r18', drop('base_model.layer1.0.bn2.running_mean'), MISSING, 'missing BatchNorm tensors of base_model.layer1.0.bn2'),
    ('r18', reshape('base_model.layer1.0.conv1.net.weight', (64, 64, 1, 1)), SHAPE, 'shape mismatch for base_model.layer1.0.conv1.net.weight'),
    ('r18', reshape('base_model.layer1.0.bn2.bias', (65,)), SHAPE, 'BN shape mismatch for base_model.layer1.0.bn2'),
    ('r18', drop('fc.bias'), MISSING, 'missing fc.weight / fc.bias'),
    ('r18', reshape('fc.weight', (12, 2048)), SHAPE, 'fc shape mismatch (want [num_class, 512])'),
    ('r50', drop('base_model.layer1.0.conv1.net.weight'), MISSING, 'missing base_model.layer1.0.conv1.net.weight'),
    ('r50', drop('base_model.layer1.0.downsample.1.weight'), MISSING, 'missing BatchNorm tensors of base_model.layer1.0.downsample.1'),
    ('r50', reshape('base_model.layer1.0.conv2.weight', (64, 64, 1, 1)), SHAPE, 'shape mismatch for base_model.layer1.0.conv2.weight'),
    ('r50', reshape('base_model.bn1.running_var', (1, 64)), SHAPE, 'BN shape mismatch for base_model.bn1'),
    ('r50', drop('fc.bias'), MISSING, 'missing fc.weight / fc.bias'),
    ('r50', reshape('fc.weight', (12, 512)), SHAPE, 'fc shape mismatch (want [num_class, 2048])'),
    ('r50_nl', drop(NL + '.theta.bias'), MISSING, f'missing {NL}.theta.bias'),
    ('r50_nl', reshape(NL + '.W.0.weight', (512, 256, 1, 1)), SHAPE, f'shape mismatch for {NL}.W.0.weight'),
    ('r50_nl', drop(NL + '.W.1.running_var'), MISSING, f'missing BatchNorm tensors of {NL}.W.1'),
    ('r50_nl', reshape(NL + '.phi.0.weight', (256, 512, 1, 1)), SHAPE, f'shape mismatch for {NL}.phi.0.weight'),
    ('convnext', drop(CNX + '.gamma'), MISSING, f'missing {CNX}.gamma'),
    ('convnext', drop(CNX + '.norm.bias'), MISSING, f'missing {CNX}.norm.bias'),
    ('convnext', reshape(CNX + '.conv_dw.weight', (128, 1, 3, 3)), SHAPE, f'shape mismatch for {CNX}.conv_dw.weight'),
    ('convnext', reshape('stem.0.weight', (128, 3, 2, 2)), SHAPE, 'shape mismatch for stem.0.weight'),
    ('convnext', reshape('head.fc.weight', (12, 512)), SHAPE, 'shape mismatch for head.fc.weight'),
    ('tdn', drop(TDN1 + '.conv1.bias'), MISSING, f'missing {TDN1}.conv1.bias'),
    ('tdn', reshape('base_model.conv1_5.0.weight', (64, 3, 7, 7)), SHAPE, 'shape mismatch for base_model.conv1_5.0.weight'),
    ('tdn', drop(TDN2 + '.mse.conv3_smallscale2.weight'), MISSING, f'missing {TDN2}.mse.conv3_smallscale2.weight'),
    ('tdn', drop(TDN2 + '.mse.bn3.running_var'), MISSING, f'missing {TDN2}.mse.bn3.running_var'),
    ('tdn', reshape(TDN2 + '.shift.conv.weight', (128, 3, 1)), SHAPE, f'shape mismatch for {TDN2}.shift.conv.weight'),
    ('tdn', drop('new_fc.bias'), MISSING, 'missing new_fc.bias'),
]


@pytest.mark.parametrize('name,defect,status,text', DEFECTS, ids=[f'{d[0]}-{d[3].replace(" ", "_")}' for d in DEFECTS])
def test_finalize_names_the_one_defect(hip_lib, name, defect, status, text):
    sd = dict(seeded(name))
    defect(sd)
    with Engine(hip_lib, name) as e:
        e.load(sd)
        assert e.finalize() == status
        assert e.error() == text


def test_convnext_capacity_refusal(hip_lib):
    """max_clips * 56 * 56 * 512 = 335 * 2^20 * 1.53 >= 2^29 activations, while tsm_create's own row check (335 * 112 * 112 rows)
    passes: TSM_ERR_CAPACITY from tsm_finalize, with every tensor in place."""
    assert 335 * 56 * 56 * 512 >= 2 ** 29 > 334 * 56 * 56 * 512
    with Engine(hip_lib, 'convnext', height=224, width=224, max_clips=335) as e:
        e.load(seeded('convnext'))
        assert e.finalize() == CAPACITY
        assert e.error() == 'max_clips * (H / 4) * (W / 4) * 512 activations must stay below 2^29 (32-bit byte offsets)'


@pytest.mark.parametrize('name,key', [('r18', 'base_model.layer2.0.downsample.0.weight'), ('tdn', TDN2 + '.conv3.bias')])
def test_finalize_again_after_a_refusal(hip_lib, name, key):
    """A refused finalize keeps the host tensors: set what was missing, finalize again."""
    sd = dict(seeded(name))
    held = sd.pop(key)
    with Engine(hip_lib, name) as e:
        e.load(sd)
        assert e.finalize() == MISSING
        assert e.error() == 'missing ' + key
        assert e.set(key, held) == OK
        assert e.finalize() == OK, e.error()
        assert e.finalize() == OK                      # (idempotent once finalized)
        assert e.set(key, held) == INVALID and e.error() == 'engine already finalized'
