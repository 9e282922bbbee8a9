"""An nn.Module spelling of the TSM-ResNet eval graph (every backbone, width and shift placement the engine implements)
with the reference's module tree, for EXPORT and key tests only.

Test infrastructure, like oracle/: it exists so that ``torch.onnx.export`` (the exporter the reference uses,
workoutdetector/scripts/export_model.py:35-47, trainer.py:325-330) can write a REAL ``.onnx`` file for
``workoutdetector_amd.onnx_import`` to read -- a file this repository's own writer (tests/_onnx_writer.py) did not
produce.  Module names follow ``TSM.state_dict()``: ``base_model.{conv1,bn1,layerL.B.{conv1.net,bn1,conv2,bn2,conv3,bn3,
downsample.0,downsample.1}}`` (``layerL.B.net.{conv1,bn1,...}`` under block placement, tsm.py:104-124) and ``new_fc``
(workoutdetector/models/tsm.py:134-136,250-262); the Lightning wrapper adds
the ``model.`` prefix (trainer.py:25-40).  The forward flattens ``[B,T,3,H,W]`` to ``[B*T,3,H,W]`` first (the
``x.view(-1, 3, 224, 224)`` commented out in trainer.py:38-40, without which the 5-D export sample cannot run)."""
import torch
import torch.nn as nn

from oracle.tsm_oracle import BACKBONES, EXPANSION, R50_PLANES, temporal_shift


class _Shifted(nn.Module):
    """TemporalShift wrapper: the wrapped conv (or, under block placement, the wrapped block) is the attribute ``net``
    (tsm.py:17-32)."""

    def __init__(self, net, n_segment, fold_div):
        super().__init__()
        self.net, self.n_segment, self.fold_div = net, n_segment, fold_div

    def forward(self, x):
        return self.net(temporal_shift(x, self.n_segment, self.fold_div))


def _conv1(conv, shift):
    """blockres: conv1 is wrapped (``conv1.net``), ``shift`` = (n_segment, fold_div); block: plain conv, ``shift`` None."""
    return _Shifted(conv, *shift) if shift else conv


class _Bottleneck(nn.Module):
    """torchvision's Bottleneck with ``width_per_group = width``: conv1 / conv2 are ``planes * width / 64`` wide, conv3
    and the downsample ``planes * 4``."""

    def __init__(self, cin, planes, width, stride, down, shift):
        super().__init__()
        mid = planes * width // 64
        self.conv1 = _conv1(nn.Conv2d(cin, mid, 1, bias=False), shift)
        self.bn1 = nn.BatchNorm2d(mid)
        self.conv2 = nn.Conv2d(mid, mid, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(mid)
        self.conv3 = nn.Conv2d(mid, planes * EXPANSION, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * EXPANSION)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = nn.Sequential(nn.Conv2d(cin, planes * EXPANSION, 1, stride, bias=False),
                                        nn.BatchNorm2d(planes * EXPANSION)) if down else None

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        identity = x if self.downsample is None else self.downsample(x)
        return self.relu(out + identity)


class _BasicBlock(nn.Module):
    def __init__(self, cin, planes, stride, shift):
        super().__init__()
        self.conv1 = _conv1(nn.Conv2d(cin, planes, 3, stride, 1, bias=False), shift)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = (nn.Sequential(nn.Conv2d(cin, planes, 1, stride, bias=False), nn.BatchNorm2d(planes))
                           if (stride != 1 or cin != planes) else None)

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        identity = x if self.downsample is None else self.downsample(x)
        return self.relu(out + identity)


class _Trunk(nn.Module):
    def __init__(self, base_model, width, shift_place, n_segment, fold_div):
        super().__init__()
        assert shift_place in ('blockres', 'block'), shift_place
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        nblocks, kind = BACKBONES[base_model]
        shift = (n_segment, fold_div) if shift_place == 'blockres' else None
        cin = 64
        for li, (nb, planes) in enumerate(zip(nblocks, R50_PLANES), start=1):
            blocks = []
            for b in range(nb):
                stride = 2 if (b == 0 and li > 1) else 1
                if kind == 'basic':
                    blk, cout = _BasicBlock(cin, planes, stride, shift), planes
                else:
                    blk, cout = _Bottleneck(cin, planes, width, stride, b == 0, shift), planes * EXPANSION
                # block placement wraps every block whole: ``layerL.B.net.conv1.weight``, ``layerL.B.net.bn1.*``, ...
                blocks.append(_Shifted(blk, n_segment, fold_div) if shift_place == 'block' else blk)
                cin = cout
            setattr(self, f'layer{li}', nn.Sequential(*blocks))
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.out_channels = cin

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.avgpool(x).flatten(1)


class TorchTSM(nn.Module):
    """TSM over a torchvision-style ResNet (``oracle.tsm_oracle.BACKBONES``) with the reference's module tree:
    ``base_model.*`` and ``new_fc`` [num_class, 2048 or 512].  ``width`` is the Bottlenecks' ``width_per_group`` (64: R50,
    128: WRN-50-2; BasicBlocks ignore it); ``shift_place`` as in ``TSM(shift_place=...)``."""

    def __init__(self, base_model='resnet50', width=64, shift_place='blockres', num_class=12, n_segment=8, fold_div=8):
        super().__init__()
        self.n_segment = n_segment
        self.base_model = _Trunk(base_model, width, shift_place, n_segment, fold_div)
        self.new_fc = nn.Linear(self.base_model.out_channels, num_class)

    def forward(self, x):
        x = x.view((-1,) + tuple(x.shape[-3:]))
        out = self.new_fc(self.base_model(x))
        out = out.view(-1, self.n_segment, out.shape[-1])
        return out.mean(dim=1, keepdim=True).squeeze(1)

    def engine_state_dict(self):
        """This module's tensors under engine / oracle keys (``fc.*``; no num_batches_tracked)."""
        return {k.replace('new_fc.', 'fc.'): v.detach().clone() for k, v in self.state_dict().items()
                if not k.endswith('num_batches_tracked')}

    def load_engine_state_dict(self, sd):
        """Engine / oracle keys (``fc.*``) -> this module's (``new_fc.*``); strict: no unexpected key, and nothing missing
        but the ``num_batches_tracked`` counters."""
        missing, unexpected = self.load_state_dict(
            {k.replace('fc.', 'new_fc.') if k.startswith('fc.') else k: torch.as_tensor(v) for k, v in sd.items()},
            strict=False)
        assert not unexpected and all(k.endswith('num_batches_tracked') for k in missing), (missing, unexpected)
        return self


class LitWrapper(nn.Module):
    """The reference exports its Lightning module, whose network is the attribute ``model`` (trainer.py:25-40)."""

    def __init__(self, net):
        super().__init__()
        self.model = net

    def forward(self, x):
        return self.model(x)


def export_onnx(module, path, sample_shape=(1, 8, 3, 224, 224), training=False):
    """``torch.onnx.export(model, sample, path, opset_version=11)`` as scripts/export_model.py:43-46 calls it, through
    torch's TorchScript exporter (``dynamo=False``).  The ``onnx`` Python package is absent from this image and the
    exporter imports it in ONE post-pass, ``_add_onnxscript_fn``, which re-serialises the model only when the graph
    holds onnxscript custom functions (never the case here: the pass returns its input bytes unchanged); the harness
    replaces that pass by the identity, everything else -- tracing, ONNX lowering, eval-mode Conv+BatchNorm fusion,
    protobuf serialisation -- is torch's own C++ exporter."""
    import warnings

    from torch.onnx._internal.torchscript_exporter import onnx_proto_utils, utils
    saved = onnx_proto_utils._add_onnxscript_fn
    onnx_proto_utils._add_onnxscript_fn = lambda model_bytes, custom_opsets: model_bytes
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            module = module.train() if training else module.eval()
            if training:        # tracing runs one forward: keep it from moving the BatchNorm running statistics
                for m in module.modules():
                    if isinstance(m, nn.BatchNorm2d):
                        m.momentum = 0.0
            mode = torch.onnx.TrainingMode.TRAINING if training else torch.onnx.TrainingMode.EVAL
            torch.onnx.export(module, torch.randn(*sample_shape), path, opset_version=11, dynamo=False, training=mode,
                              do_constant_folding=not training)
    finally:
        onnx_proto_utils._add_onnxscript_fn = saved
        assert utils is not None
    return path
