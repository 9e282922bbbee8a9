"""Weights from an exported ``.onnx`` TSM model (R50, WRN-50-2, R18 or R34) -> engine state dict, without the ``onnx`` package.

The reference deploys ``checkpoints/*.onnx`` produced by ``torch.onnx.export(model, sample[1,8,3,224,224],
opset_version=11)`` (workoutdetector/scripts/export_model.py:35-47, trainer.py:325-330) and runs it with
onnxruntime (utils/inference_count.py:620).  Neither ``onnx`` nor ``onnxruntime`` exists in this image, so
this module reads the protobuf wire format directly (ModelProto.graph -> initializer / node; only the
fields needed) and maps the tensors onto the engine's ``TSM.state_dict()`` keys:

  * initialisers that still carry state-dict names (``...base_model.layer1.0.conv1.net.weight``,
    BatchNormalization inputs ``...bn1.weight/bias/running_mean/running_var``): any prefix in front of
    ``base_model.`` / ``fc.`` / ``new_fc.`` is stripped; a BatchNormalization node whose ``epsilon`` attribute is not the
    engine's 1e-5 (absent: ONNX's default, 1e-5) is refused -- a state dict cannot carry it and the engine folds with its own;
  * exports where the exporter folded BatchNorm into the convolutions (eval-mode Conv+BN fusion: anonymous
    ``onnx::Conv_###`` weight + bias initialisers): every Conv node is identified by CONNECTIVITY, not by its
    position in the file -- the number of Conv nodes upstream of it in the dataflow graph fixes its place in the
    network (conv1 and downsample of a block see the same upstream set, conv2 one more, conv3 two more; the two
    1x1 convs that share a count always differ in output channels; in a BasicBlock conv1 is a 3x3 and the downsample
    a 1x1), the weight shape must agree, and anything ambiguous or missing raises -- and every conv gets an identity
    BatchNorm carrying its bias.

The backbone is read from the graph: 53 Conv nodes and a 2048-wide classifier are R50, or WRN-50-2 where layer1.0.conv1
is 128 channels wide instead of 64; 20 / 36 Conv nodes, no ``conv3`` and a 512-wide classifier are R18 / R34.

Tested on files written by torch's own exporter (``torch.onnx.export(..., opset_version=11)`` of an nn.Module with
the reference's module tree, both export styles; tests/_torch_tsm.py) and on hand-written files
(``tests/_onnx_writer.py``) for the malformed cases.
"""
from __future__ import annotations

import struct
from collections import OrderedDict
from typing import Dict, List, Optional, Tuple

import numpy as np

from .weights import BACKBONES, DEPTHS, conv_specs, feature_width

BN_EPS = 1e-5


# ---- protobuf wire format -------------------------------------------------------------------------------
def _varint(buf: memoryview, pos: int) -> Tuple[int, int]:
    result = shift = 0
    while True:
        b = buf[pos]
        pos += 1
        result |= (b & 0x7F) << shift
        if not b & 0x80:
            return result, pos
        shift += 7


def _fields(buf: memoryview):
    """Yield (field_number, wire_type, value) for one message; LEN values are memoryview slices."""
    pos, end = 0, len(buf)
    while pos < end:
        tag, pos = _varint(buf, pos)
        field, wt = tag >> 3, tag & 7
        if wt == 0:
            val, pos = _varint(buf, pos)
        elif wt == 1:
            val, pos = bytes(buf[pos:pos + 8]), pos + 8
        elif wt == 2:
            n, pos = _varint(buf, pos)
            val, pos = buf[pos:pos + n], pos + n
        elif wt == 5:
            val, pos = bytes(buf[pos:pos + 4]), pos + 4
        else:
            raise ValueError(f'unsupported protobuf wire type {wt}')
        yield field, wt, val


def _packed_varints(buf: memoryview) -> List[int]:
    out, pos = [], 0
    while pos < len(buf):
        v, pos = _varint(buf, pos)
        out.append(v)
    return out


def _parse_tensor(buf: memoryview) -> Tuple[str, np.ndarray]:
    """TensorProto: dims=1, data_type=2, float_data=4, int64_data=7, name=8, raw_data=9."""
    dims: List[int] = []
    dtype, name, raw, floats, ints = 0, '', None, [], []
    for f, wt, v in _fields(buf):
        if f == 1:
            dims += _packed_varints(v) if wt == 2 else [v]
        elif f == 2:
            dtype = v
        elif f == 4:
            floats += list(struct.unpack(f'<{len(v) // 4}f', bytes(v))) if wt == 2 else [struct.unpack('<f', v)[0]]
        elif f == 7:
            ints += _packed_varints(v) if wt == 2 else [v]
        elif f == 8:
            name = bytes(v).decode()
        elif f == 9:
            raw = bytes(v)
    if dtype == 1:      # FLOAT
        arr = np.frombuffer(raw, dtype='<f4') if raw is not None else np.asarray(floats, dtype=np.float32)
    elif dtype == 7:    # INT64
        arr = np.frombuffer(raw, dtype='<i8') if raw is not None else np.asarray(ints, dtype=np.int64)
    else:
        return name, np.zeros(0, dtype=np.float32)      # other types are never weights of this model
    return name, arr.reshape(dims).copy()


def _parse_float_attribute(buf: memoryview) -> Tuple[str, Optional[float]]:
    """AttributeProto: name=1, f=2 (fixed32), type=20 (1 = FLOAT) -> (name, the float; None for every other type)."""
    name, value, kind = '', None, None
    for f, wt, v in _fields(buf):
        if f == 1 and wt == 2:
            name = bytes(v).decode()
        elif f == 2 and wt == 5:
            value = struct.unpack('<f', v)[0]
        elif f == 20 and wt == 0:
            kind = v
    return name, (value if kind in (None, 1) else None)      # (type is optional before IR version 3)


def _parse_node(buf: memoryview) -> dict:
    """NodeProto: input=1, output=2, name=3, op_type=4, attribute=5 (the float ones only: BatchNormalization's epsilon)."""
    node = dict(input=[], output=[], name='', op_type='', attrs={})
    for f, wt, v in _fields(buf):
        if f == 1:
            node['input'].append(bytes(v).decode())
        elif f == 2:
            node['output'].append(bytes(v).decode())
        elif f == 3:
            node['name'] = bytes(v).decode()
        elif f == 4:
            node['op_type'] = bytes(v).decode()
        elif f == 5 and wt == 2:
            name, value = _parse_float_attribute(v)
            if value is not None:
                node['attrs'][name] = value
    return node


def _check_batchnorm_eps(path: str, nodes: List[dict]) -> None:
    """The engine folds every BatchNorm with eps = 1e-5 (csrc/tsm_host_util.h: kBnEps) and a state dict has no place for
    another value: a BatchNormalization node whose ``epsilon`` (absent: ONNX's default, 1e-5) is not float32(1e-5) raises."""
    for n in nodes:
        if n['op_type'] != 'BatchNormalization':
            continue
        eps = n['attrs'].get('epsilon', BN_EPS)
        if np.float32(eps) != np.float32(BN_EPS):
            raise ValueError(f'{path}: BatchNormalization "{n["name"]}" has epsilon = {eps:g}; the engine folds every BatchNorm '
                             f'with {BN_EPS:g} and cannot represent another value')


def parse_onnx(path: str) -> Tuple[Dict[str, np.ndarray], List[dict]]:
    """(initialisers by name, nodes in graph order) of an ONNX ModelProto file."""
    data = memoryview(open(path, 'rb').read())
    graph = None
    for f, wt, v in _fields(data):
        if f == 7 and wt == 2:      # ModelProto.graph
            graph = v
    if graph is None:
        raise ValueError(f'{path}: no graph in the ONNX file')
    inits: Dict[str, np.ndarray] = OrderedDict()
    nodes: List[dict] = []
    for f, wt, v in _fields(graph):
        if f == 1 and wt == 2:      # GraphProto.node
            nodes.append(_parse_node(v))
        elif f == 5 and wt == 2:    # GraphProto.initializer
            name, arr = _parse_tensor(v)
            inits[name] = arr
    return inits, nodes


# ---- mapping to the engine's state dict ---------------------------------------------------------------------
def _strip_prefix(name: str) -> str:
    for anchor in ('base_model.', 'new_fc.', 'fc.'):
        i = name.find(anchor)
        if i >= 0 and (i == 0 or name[i - 1] == '.'):
            return name[i:].replace('new_fc.', 'fc.')
    return name


def _resolve_convs(path: str, nodes: List[dict], inits: Dict[str, np.ndarray], specs) -> List[dict]:
    """The Conv node of every entry of ``conv_specs()``, found by dataflow position + weight shape."""
    convs = [i for i, n in enumerate(nodes) if n['op_type'] == 'Conv']
    if len(convs) != len(specs):
        raise ValueError(f'{path}: {len(convs)} Conv nodes, the TSM-ResNet has {len(specs)}')
    bit = {ni: 1 << k for k, ni in enumerate(convs)}
    upstream: Dict[str, int] = {}          # tensor name -> bitmask of the Conv nodes it depends on
    depth: Dict[int, int] = {}
    for ni, n in enumerate(nodes):         # ONNX graphs are topologically sorted
        m = 0
        for t in n['input']:
            m |= upstream.get(t, 0)
        if ni in bit:
            depth[ni] = bin(m).count('1')
            m |= bit[ni]
        for t in n['output']:
            upstream[t] = m
    by_key: Dict[Tuple[int, tuple], List[int]] = {}
    for ni in convs:
        w = inits.get(nodes[ni]['input'][1]) if len(nodes[ni]['input']) > 1 else None
        if w is None:
            raise ValueError(f'{path}: Conv "{nodes[ni]["name"]}" has no initialiser weight')
        by_key.setdefault((depth[ni], tuple(w.shape)), []).append(ni)
    out, before = [], 0                    # `before` = Conv nodes upstream of the current block's input
    for idx, (wkey, _bnp, cout, cin, k) in enumerate(specs):
        if idx == 0:
            want = 0
        else:
            role = wkey.rsplit('.', 2)[-2]   # conv2 | conv3 | 0 (downsample) | conv1 | net (blockres: conv1.net)
            want = before + {'net': 0, 'conv1': 0, '0': 0, 'conv2': 1, 'conv3': 2}[role]
        cands = by_key.get((want, (cout, cin, k, k)), [])
        if len(cands) != 1:
            raise ValueError(f'{path}: {len(cands)} Conv nodes with {want} upstream convs and weight {(cout, cin, k, k)} '
                             f'for {wkey}; cannot map the graph onto the TSM-ResNet')
        out.append(nodes[cands[0]])
        nxt = specs[idx + 1][0] if idx + 1 < len(specs) else ''
        if idx == 0 or (nxt.endswith(('.conv1.net.weight', '.net.conv1.weight')) or nxt == ''):
            before = idx + 1               # a block is complete: everything so far is upstream of the next one
    return out


def _layer1_mid_width(inits: Dict[str, np.ndarray], nodes: List[dict]) -> int:
    """Output width of layer1.0.conv1 = input width of the first 3x3 Conv after the 7x7 stem (layer1.0.conv2), whatever
    order the export wrote conv1 and the downsample in."""
    for n in nodes:
        if n['op_type'] != 'Conv' or len(n['input']) < 2:
            continue
        w = inits.get(n['input'][1])
        if w is not None and w.ndim == 4 and w.shape[2:] == (3, 3):
            return int(w.shape[1])
    raise ValueError('no 3x3 Conv node with an initialiser weight: cannot tell the bottleneck width')


def detect_backbone(inits: Dict[str, np.ndarray], nodes: List[dict]) -> str:
    """'resnet18' | 'resnet34' | 'resnet50' | 'wide_resnet50_2' from the graph: the Conv node count (20 / 36 / 53 / 53 --
    the stem, two or three convs per block, the downsample convs), then, where the count is shared (R50 and WRN-50-2),
    the output width of layer1.0.conv1 (64 / 128); checked against the state-dict names where the export kept them."""
    n_conv = sum(n['op_type'] == 'Conv' for n in nodes)
    by_count: Dict[int, List[str]] = {}
    for m in DEPTHS:
        by_count.setdefault(len(conv_specs(m)), []).append(m)
    if n_conv not in by_count:
        raise ValueError(f'{n_conv} Conv nodes: not a TSM-ResNet18 / 34 / 50 or WRN-50-2 ({sorted(by_count)})')
    cands = by_count[n_conv]
    if len(cands) > 1:
        width = _layer1_mid_width(inits, nodes)
        by_width = {conv_specs(m)[1][2]: m for m in cands}   # (conv_specs()[1] = layer1.0.conv1)
        if width not in by_width:
            raise ValueError(f'{n_conv} Conv nodes, layer1.0.conv1 {width} channels wide: not one of '
                             f'{", ".join(f"{m} ({w})" for w, m in sorted(by_width.items()))}')
        cands = [by_width[width]]
    model = cands[0]
    if BACKBONES[model][1] != 'bottleneck' and any('.conv3.' in k for k in inits):   # (a folded export has anonymous names: counts only)
        raise ValueError(f'{n_conv} Conv nodes ({model}) but the initialisers hold conv3 weights')
    return model


def load_onnx_state_dict(path: str, num_class: int, base_model: Optional[str] = None,
                         shift_place: str = 'blockres') -> 'OrderedDict[str, np.ndarray]':
    """Engine state dict (``TsmEngine.load_state_dict``) from a TSM-R50 / R18 / R34 / WRN-50-2 ``.onnx`` export.  The backbone is
    recognised from the graph (``detect_backbone``); a ``base_model`` that disagrees with it raises.  The shift placement
    comes from the caller: it names the keys (``conv_specs``); the graph's convs are the same under both placements."""
    inits, nodes = parse_onnx(path)
    _check_batchnorm_eps(path, nodes)
    found = detect_backbone(inits, nodes)
    if base_model is not None and base_model != found:
        raise ValueError(f'{path}: the graph is a {found}, not a {base_model}')
    specs = conv_specs(found, shift_place)
    feat = feature_width(found)
    named = OrderedDict((_strip_prefix(k), v) for k, v in inits.items())
    unwrap = ('.net.', '.') if shift_place == 'block' else ('.conv1.net.', '.conv1.')
    if all(w in named or w.replace(*unwrap) in named for w, *_ in specs):
        sd = OrderedDict((k, v) for k, v in named.items()
                         if (k.startswith('base_model.') or k.startswith('fc.')) and v.dtype == np.float32)
    else:
        sd = OrderedDict()
        for (wkey, bnp, cout, cin, k), node in zip(specs, _resolve_convs(path, nodes, inits, specs)):
            w = inits[node['input'][1]]
            b = inits[node['input'][2]] if len(node['input']) > 2 else np.zeros(cout, np.float32)
            sd[wkey] = w.astype(np.float32)
            # identity BatchNorm carrying the folded bias: scale = 1/sqrt(var + eps) = 1, bias = beta
            sd[bnp + '.weight'] = np.ones(cout, np.float32)
            sd[bnp + '.bias'] = b.astype(np.float32)
            sd[bnp + '.running_mean'] = np.zeros(cout, np.float32)
            sd[bnp + '.running_var'] = np.full(cout, 1.0 - BN_EPS, np.float32)
        fc = [n for n in nodes if n['op_type'] in ('Gemm', 'MatMul')]
        if not fc:
            raise ValueError(f'{path}: no Gemm/MatMul node for the classifier')
        w = next(inits[i] for i in fc[-1]['input'] if i in inits and inits[i].ndim == 2)
        if w.shape == (feat, num_class):
            w = w.T
        sd['fc.weight'] = np.ascontiguousarray(w, dtype=np.float32)
        bias = [inits[i] for i in fc[-1]['input'] if i in inits and inits[i].ndim == 1]
        if not bias:        # MatMul followed by Add
            adds = [n for n in nodes if n['op_type'] == 'Add' and fc[-1]['output'][0] in n['input']]
            bias = [inits[i] for n in adds for i in n['input'] if i in inits and inits[i].ndim == 1]
        sd['fc.bias'] = bias[0].astype(np.float32) if bias else np.zeros(num_class, np.float32)
    if tuple(sd['fc.weight'].shape) != (num_class, feat):
        raise ValueError(f'{path}: classifier is {tuple(sd["fc.weight"].shape)}, expected ({num_class}, {feat})')
    return sd
