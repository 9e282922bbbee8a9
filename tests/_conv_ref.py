"""High-precision reference of one conv launch as tsm_conv_op makes it (tests/test_conv_forms_gpu.py).

    y = act( conv(x, w) + bn  [+ shift?(residual)]  [+ conv1x1(shift?(x2), w2, stride2) + bn2] )

fp32 / split-bf16: every operation in float64 from the given fp32 operands (BatchNorm unfolded), so a bar measures the
kernel's error alone.  bf16: the operands rounded exactly as the engine rounds them (input, BN-folded weights, residual, second
source; fold_bn is the host fold to the bit), float64 accumulation, conv3 and the downsample in ONE sum with the fp32 sum of
the two folded biases (tsm_host::concat_k_pair, as _bottleneck_bf16 adds them), the result left unrounded for assert_bf16_op.

Tensors are NCHW torch float32; the result is NCHW float64.  T > 0 shifts (fold = channels of the shifted tensor // fold_div):
shift_target 0 the input, 1 the identity -- the residual if given, else x2, else (a 1x1 at stride 2) the input."""
import torch
import torch.nn.functional as F

from oracle.tsm_oracle import BN_EPS, bf16_round, fold_bn, temporal_shift


def _bn64(h, bn):
    g, b, m, v = (t.to(torch.float64)[None, :, None, None] for t in bn)
    return (h - m) / torch.sqrt(v + BN_EPS) * g + b


def conv_ref(x, w, bn, stride=1, relu=True, residual=None, T=0, fold_div=8, shift_target=0, x2=None, w2=None, bn2=None,
             stride2=1, bf16=False):
    k = w.shape[-1]
    sh = (lambda t: temporal_shift(t, T, fold_div)) if T > 0 else (lambda t: t)
    if shift_target == 1:
        if residual is not None:
            residual = sh(residual)
        elif x2 is not None:
            x2 = sh(x2)
        else:
            assert k == 1 and stride == 2, 'shift_target 1 with nothing to shift'
            x = sh(x)
    else:
        x = sh(x)
    if not bf16:
        h = _bn64(F.conv2d(x.to(torch.float64), w.to(torch.float64), stride=stride, padding=k // 2), bn)
        if x2 is not None:
            h = h + _bn64(F.conv2d(x2.to(torch.float64), w2.to(torch.float64), stride=stride2), bn2)
        if residual is not None:
            h = h + residual.to(torch.float64)
    else:
        wf, bias = fold_bn(w, bn)
        h = F.conv2d(bf16_round(x).to(torch.float64), bf16_round(wf).to(torch.float64), stride=stride, padding=k // 2)
        if x2 is not None:
            wf2, bias2 = fold_bn(w2, bn2)
            h = h + F.conv2d(bf16_round(x2).to(torch.float64), bf16_round(wf2).to(torch.float64), stride=stride2)
            bias = bias + bias2                     # (fp32, as the host sums the two folded biases)
        h = h + bias.to(torch.float64)[None, :, None, None]
        if residual is not None:
            h = h + bf16_round(residual).to(torch.float64)
    return torch.relu(h) if relu else h
