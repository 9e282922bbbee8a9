"""TsmEngine: Python host side of the MI355X TSM-ResNet clip-inference engine (R50; R18 / R34 / WRN-50-2 via ``base_model``;
``base_model='convnext_base'``: the ConvNeXt-Base image model of ``create_image_model`` / ``create_feature_model``).

Drop-in for the two duck types the reference's hot path is written against:

  * onnxruntime.InferenceSession style (workoutdetector/utils/inference_count.py:265,273-275,
    scripts/eval_classification.py:29,44):   ``model.get_inputs()[0].name`` and
    ``model.run(None, {name: float32[B,T,3,H,W]}) -> [float32[B,num_class]]`` (any B >= 1; the
    reference's export is fixed at B = 1).
  * nn.Module style (tests/test_models.py:26-28):   ``model(x[B*T,3,H,W]) -> [B,num_class]``
    with the factory ``create_model(num_class, num_segments, base_model, checkpoint, device, ...)``
    (workoutdetector/models/tsm.py:422-476).

All arithmetic happens in libtsm_hip.so (hand-written HIP for gfx950) through the C ABI in
include/tsm_hip.h.  No CPU fallback: construction raises if the library or a GPU is missing.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Mapping, Optional, Sequence

import numpy as np

from . import _lib
from .weights import (BACKBONES, CONVNEXT, CONVNEXT_DEPTHS, CONVNEXT_WIDTHS, DEPTHS, NL_BLOCKS, SHIFT_PLACES, TDN, TDN_FRAMES, WIDTHS,
                      _convnext_depths, _tdn_depths, feature_width, is_convnext, is_mmaction_state_dict, make_state_dict, make_tdn_state_dict,
                      remap_checkpoint_keys, remap_mmaction_keys, remap_tdn_keys, remap_timm_keys, remap_torchvision_keys, tdn_alpha_beta)

CONSENSUS_TYPES = {'avg': 0, 'identity': 1}      # tsm_set_consensus


@dataclass
class NodeArg:
    """Minimal stand-in for onnxruntime.NodeArg (only what the reference reads)."""
    name: str
    shape: list
    type: str = 'tensor(float)'


def _as_f32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a), dtype=np.float32)


def _addr(t) -> int:
    """The address of an ndarray's or a tensor's first element."""
    return t.ctypes.data if isinstance(t, np.ndarray) else t.data_ptr()


@dataclass
class _Input:
    """What a forward reads, whatever it writes: ``chunks`` [(first clip, clips, address, keepalive)] is one C call each -- the
    address of a clip slice or of a descriptor struct, which ``keepalive`` holds until the call has returned."""
    layout: int
    memkind: int
    n_clips: int
    like: object                # the ndarray or CUDA tensor outputs are allocated like
    stream: Optional[int]       # None: host memory, the engine's own stream
    chunks: list


class TsmEngine:
    INPUT_NAME = 'input'
    OUTPUT_NAME = 'output'

    def __init__(self, num_class: int = 12, num_segments: int = 8, height: int = 224, width: int = 224,
                 shift_div: int = 8, is_shift: bool = True, max_clips: int = 32, device: int = 0,
                 state_dict: Optional[Mapping[str, object]] = None, dtype: str = 'f32',
                 base_model: str = 'resnet50', shift_place: str = 'blockres', consensus_type: str = 'avg',
                 non_local: bool = False, temporal_pool: bool = False, convnext_depths: Optional[Sequence[int]] = None,
                 tdn_depths: Optional[Sequence[int]] = None, tdn_alpha: Optional[float] = None, tdn_beta: Optional[float] = None):
        # base_model='convnext_base' (include/tsm_hip.h: tsm_set_convnext): an image model -- num_segments=1, is_shift=False,
        # dtype='f32' -- of ``convnext_depths`` blocks per stage, (3, 3, 27, 3) unless given (tests build shallow engines).
        # base_model='tdn_resnet50' (include/tsm_hip.h: tsm_set_tdn): clips of 15 planes per segment, is_shift=False, dtype='f32',
        # ``tdn_depths`` blocks per stage, (3, 4, 6, 3) unless given; ``tdn_alpha`` / ``tdn_beta`` default to tdn_net's rule.
        convnext_depths, tdn_depths = _check_engine_args(      # every refusal before the library loads
            base_model, num_segments=num_segments, is_shift=is_shift, dtype=dtype, height=height, width=width, shift_place=shift_place,
            consensus_type=consensus_type, non_local=non_local, temporal_pool=temporal_pool, convnext_depths=convnext_depths,
            tdn_depths=tdn_depths, tdn_alpha=tdn_alpha, tdn_beta=tdn_beta)
        tdn, convnext = tdn_depths is not None, convnext_depths is not None
        if tdn and (tdn_alpha is None or tdn_beta is None):
            tdn_alpha, tdn_beta = tdn_alpha_beta(num_segments)
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self.num_class, self.num_segments = int(num_class), int(num_segments)
        self.height, self.width = int(height), int(width)
        self.max_clips, self.device = int(max_clips), int(device)
        self.dtype = dtype
        self.base_model = base_model
        self.shift_place = shift_place
        self.consensus_type = consensus_type
        self.non_local = bool(non_local)
        self.temporal_pool = bool(temporal_pool)
        self.convnext_depths = convnext_depths      # None for a ResNet engine
        self.tdn_depths = tdn_depths                # None unless a TDN engine
        self.planes = 3 * TDN_FRAMES if tdn else 3  # input planes per segment
        self.feature_dim = 2048 if tdn else feature_width(base_model)      # row width of forward_features
        # layout tsm_preprocess must write for this engine to consume frames in place
        self.packed_layout = {'f32': _lib.LAYOUT_NTHWC4, 'bf16x3': _lib.LAYOUT_NTHWC8S,
                              'bf16': _lib.LAYOUT_NTHWC8B}[dtype]
        cfg = _lib.TsmConfig(C.sizeof(_lib.TsmConfig), num_class, num_segments, height, width, shift_div,
                             1 if is_shift else 0, max_clips, device, _lib.DTYPES[dtype])
        _lib.check(self._lib.tsm_create(C.byref(cfg), C.byref(self._h)))
        if convnext:
            _lib.check(self._lib.tsm_set_convnext(self._h, (C.c_int32 * 4)(*convnext_depths)), self._h)
        elif tdn:
            _lib.check(self._lib.tsm_set_tdn(self._h, (C.c_int32 * 4)(*tdn_depths), float(tdn_alpha), float(tdn_beta)), self._h)
        elif DEPTHS[base_model] != 50:
            _lib.check(self._lib.tsm_set_backbone(self._h, DEPTHS[base_model]), self._h)
        if base_model in WIDTHS:
            _lib.check(self._lib.tsm_set_bottleneck_width(self._h, WIDTHS[base_model]), self._h)
        if shift_place != 'blockres':
            _lib.check(self._lib.tsm_set_shift_place(self._h, SHIFT_PLACES[shift_place]), self._h)
        if consensus_type != 'avg':
            _lib.check(self._lib.tsm_set_consensus(self._h, CONSENSUS_TYPES[consensus_type]), self._h)
        if non_local:
            _lib.check(self._lib.tsm_set_non_local(self._h, 1), self._h)
        if temporal_pool:
            _lib.check(self._lib.tsm_set_temporal_pool(self._h, 1), self._h)
        self._finalized = False
        if state_dict is not None:
            self.load_state_dict(state_dict)

    # ---- weights ---------------------------------------------------------------------------------
    def load_state_dict(self, state_dict: Mapping[str, object], strict: bool = False) -> 'TsmEngine':
        """Hand every tensor to the engine (it folds BatchNorm and packs), then finalize.
        Non-strict like the reference's ``load_state_dict(base_dict, strict=False)`` (tsm.py:473):
        unknown keys are skipped, ``num_batches_tracked`` is ignored; missing tensors raise."""
        for name, value in state_dict.items():
            if name.endswith('num_batches_tracked'):
                continue
            arr = _as_f32(value.detach().cpu().numpy() if hasattr(value, 'detach') else value)
            shape = (C.c_int64 * arr.ndim)(*arr.shape)
            rc = self._lib.tsm_set_tensor(self._h, name.encode(), arr.ctypes.data, shape, arr.ndim)
            if rc == -1 and not strict and b'unknown tensor name' in (self._lib.tsm_last_error(self._h) or b''):
                continue
            _lib.check(rc, self._h)
        _lib.check(self._lib.tsm_finalize(self._h), self._h)
        self._finalized = True
        return self

    # ---- onnxruntime.InferenceSession duck type ---------------------------------------------------
    def get_inputs(self) -> List[NodeArg]:
        return [NodeArg(self.INPUT_NAME, [None, self.num_segments, self.planes, self.height, self.width])]

    def get_outputs(self) -> List[NodeArg]:
        return [NodeArg(self.OUTPUT_NAME, [None] + list(self._out_shape(0)[1:]))]

    @property
    def out_segments(self) -> int:
        """Segments per clip behind the backbone -- the rows of ``forward_features`` and of the 'identity' logits: T, or T / 2
        behind the temporal pool."""
        return self.num_segments // 2 if getattr(self, 'temporal_pool', False) else self.num_segments

    def _out_shape(self, b: int) -> tuple:
        """Logits of ``b`` clips: [b, num_class] ('avg'), [b, T, num_class] ('identity': the fc output of every segment,
        tsm.py:165-174; T / 2 segments behind the temporal pool).  Dimension 0 is the clip axis either way, so a ``max_clips``
        chunk is a contiguous slice."""
        return (b, self.out_segments, self.num_class) if self.consensus_type == 'identity' else (b, self.num_class)

    def run(self, output_names: Optional[Sequence[str]], input_feed: Dict[str, np.ndarray]) -> List[np.ndarray]:
        if output_names is not None and list(output_names) != [self.OUTPUT_NAME]:
            raise ValueError(f'unknown outputs {output_names}; engine has [{self.OUTPUT_NAME!r}]')
        if set(input_feed) != {self.INPUT_NAME}:
            raise ValueError(f'feed must have exactly the key {self.INPUT_NAME!r}, got {sorted(input_feed)}')
        x = input_feed[self.INPUT_NAME]
        want = (self.num_segments, self.planes, self.height, self.width)
        if self.tdn_depths and x.ndim == 6 and tuple(x.shape[1:]) == (want[0], TDN_FRAMES, 3) + want[2:]:
            x = x.reshape((x.shape[0],) + want)
        if x.ndim != 5 or tuple(x.shape[1:]) != want:
            raise ValueError(f'input must be [B,{want[0]},{want[1]},{want[2]},{want[3]}], got {tuple(x.shape)}')
        return [self.forward_host(_as_f32(x))]

    # ---- nn.Module duck type ----------------------------------------------------------------------
    def __call__(self, x):
        """x: [B*T,3,H,W] (or [B,T,3,H,W]) torch tensor (cpu or on this engine's GPU) or ndarray;
        returns logits [B,num_class] ([B,T,num_class] with consensus_type='identity') of the same kind."""
        is_torch = hasattr(x, 'is_cuda')
        shape = tuple(x.shape)
        hw, p = (self.height, self.width), self.planes
        if len(shape) == 4 and shape[1:] == (p,) + hw and shape[0] % self.num_segments == 0:
            b = shape[0] // self.num_segments
        elif len(shape) == 4 and self.tdn_depths and shape[1:] == (3,) + hw and shape[0] % (self.num_segments * TDN_FRAMES) == 0:
            b = shape[0] // (self.num_segments * TDN_FRAMES)      # [B*T*5, 3, H, W]: the same memory (the reference's reshape)
        elif len(shape) == 4:
            raise ValueError(f'input must be [B*{self.num_segments},{p},{self.height},{self.width}], got {shape}')
        elif len(shape) == 5 and shape[1:] == (self.num_segments, p) + hw:
            b = shape[0]
        elif len(shape) == 6 and self.tdn_depths and shape[1:] == (self.num_segments, TDN_FRAMES, 3) + hw:
            b = shape[0]
        else:
            raise ValueError(f'bad input shape {shape}')
        if is_torch and x.is_cuda:
            return self.forward_device(x.reshape(b, self.num_segments, p, self.height, self.width))
        arr = _as_f32(x.detach().numpy() if is_torch else x)
        out = self.forward_host(arr.reshape(b, self.num_segments, p, self.height, self.width))
        if is_torch:
            import torch
            return torch.from_numpy(out)
        return out

    def eval(self) -> 'TsmEngine':  # nn.Module API used by callers; inference-only engine
        return self

    def to(self, *_args, **_kw) -> 'TsmEngine':
        return self

    # ---- forwards ---------------------------------------------------------------------------------
    def _floats_per_clip(self, layout: int) -> int:
        """float32 slots one clip occupies in ``layout`` (the C ABI takes bare pointers: sizes are checked here)."""
        t, h, w = self.num_segments, self.height, self.width
        per = {_lib.LAYOUT_NTCHW: self.planes * h * w, _lib.LAYOUT_NTHWC: 3 * h * w, _lib.LAYOUT_NTHWC4: 4 * h * w,
               _lib.LAYOUT_NTHWC8S: 8 * h * ((w + 1) // 2), _lib.LAYOUT_NTHWC8B: 4 * h * ((w + 1) // 2)}
        if layout not in per:
            raise ValueError(f'unknown layout {layout}')
        return t * per[layout]

    def _check_clips(self, n_elems: int, b: int, layout: int) -> None:
        if b <= 0 or n_elems != b * self._floats_per_clip(layout):
            raise ValueError(f'clips hold {n_elems} float32 values; layout {layout} needs {self._floats_per_clip(layout)} '
                             f'per clip x {b} clips (T={self.num_segments}, H={self.height}, W={self.width})')

    # A builder (_clips_input, _pool_input, _ring_input) owns the checks on an input and describes it as an _Input; a runner
    # (_run_logits, _run_features, _run_tap) owns the output and the C calls.  Every public forward is one of each.
    def _clips_input(self, clips, layout: int, on_device: bool, need: str = '') -> '_Input':
        """Dense clips in ``layout``: anything NumPy reads (host memory, the engine's own stream) or, ``on_device``, a float32 CUDA
        tensor on this engine's device (torch's current stream) -- ``need`` is the refusal of any other tensor."""
        self._need_finalized()
        if on_device:
            import torch
            if not (clips.is_cuda and clips.dtype == torch.float32):
                raise ValueError(need)
            if clips.device.index != self.device:
                raise ValueError(f'tensor on cuda:{clips.device.index}, engine on cuda:{self.device}')
            clips = clips.contiguous()
            b = clips.shape[0]
            self._check_clips(clips.numel(), b, layout)
            memkind, stream = _lib.MEM_DEVICE, torch.cuda.current_stream(clips.device).cuda_stream
        else:
            clips = _as_f32(clips)
            b = clips.shape[0]
            self._check_clips(clips.size, b, layout)
            memkind, stream = _lib.MEM_HOST, None
        chunks = [(s, min(self.max_clips, b - s), _addr(clips[s:s + self.max_clips]), clips) for s in range(0, b, self.max_clips)]
        return _Input(layout, memkind, b, clips, stream, chunks)

    def _descriptor_input(self, layout: int, n: int, like, make, per: Optional[int] = None) -> '_Input':
        """``n`` clips that descriptor structs describe (a CUDA input): ``make(first, count)`` is the struct of one chunk of ``per``."""
        import torch
        per = per or self.max_clips
        structs = [(s, min(per, n - s), make(s, min(per, n - s))) for s in range(0, n, per)]
        return _Input(layout, _lib.MEM_DEVICE, n, like, torch.cuda.current_stream(like.device).cuda_stream,
                      [(s, m, C.addressof(d), d) for s, m, d in structs])

    def _rows(self, inp: '_Input', shape: tuple, out, own_message: bool = False):
        """What a runner writes into: an ndarray for a host input, else ``out`` -- checked -- or a new tensor like the input."""
        if inp.memkind == _lib.MEM_HOST:
            return np.empty(shape, dtype=np.float32)
        import torch
        if own_message and out is not None:           # (forward_device's own, older wording)
            if not (out.is_cuda and out.device == inp.like.device and out.dtype == torch.float32 and out.is_contiguous()
                    and tuple(out.shape) == shape):
                raise ValueError(f'out must be a contiguous float32 {list(shape)} tensor on {inp.like.device}')
            return out
        return _out(out, shape, torch.float32, inp.like)

    def _run_logits(self, inp: '_Input', out=None, own_message: bool = False):
        """``tsm_forward`` per chunk: clips [s, s + n) write rows [s, s + n) of ``_out_shape(n_clips)``."""
        out = self._rows(inp, self._out_shape(inp.n_clips), out, own_message)
        for s, n, address, _keepalive in inp.chunks:
            _lib.check(self._lib.tsm_forward(self._h, address, inp.memkind, inp.layout, n, _addr(out[s:s + n]), inp.stream), self._h)
        return out

    def _run_features(self, inp: '_Input', normalize: bool, out=None):
        """``tsm_forward_features`` per chunk: clips [s, s + n) write rows [s t, (s + n) t) of [n_clips * t, feature_dim]."""
        t = self.out_segments
        out = self._rows(inp, (inp.n_clips * t, self.feature_dim), out)
        for s, n, address, _keepalive in inp.chunks:
            _lib.check(self._lib.tsm_forward_features(self._h, address, inp.memkind, inp.layout, n, _addr(out[s * t:(s + n) * t]),
                                                      int(bool(normalize)), inp.stream), self._h)
        return out

    def _run_tap(self, inp: '_Input', stage: str, cap: int, one_chunk: str = '') -> np.ndarray:
        """``tsm_forward_tap`` on ALL the input's clips in one call -- ``one_chunk`` names a caller that refuses more than
        ``max_clips`` itself -- into a buffer of ``cap`` floats beside the input; the NHWC activation as an ndarray."""
        if one_chunk and len(inp.chunks) != 1:
            raise ValueError(f'{one_chunk} takes at most max_clips = {self.max_clips} clips')
        if inp.memkind == _lib.MEM_HOST:
            buf = np.empty(cap, dtype=np.float32)
        else:
            import torch
            buf = torch.empty(cap, dtype=torch.float32, device=inp.like.device)
        shape = (C.c_int64 * 4)()
        _lib.check(self._lib.tsm_forward_tap(self._h, inp.chunks[0][2], inp.memkind, inp.layout, inp.n_clips, stage.encode(), _addr(buf), cap,
                                             shape, inp.stream), self._h)
        dims = tuple(int(v) for v in shape)
        res = buf[:int(np.prod(dims))].reshape(dims)
        return res.copy() if inp.memkind == _lib.MEM_HOST else res.cpu().numpy()

    def forward_host(self, clips: np.ndarray, layout: int = _lib.LAYOUT_NTCHW) -> np.ndarray:
        """clips: float32 [B,T,3,H,W] (or [B,T,H,W,3] with LAYOUT_NTHWC) in host memory."""
        return self._run_logits(self._clips_input(clips, layout, False))

    def forward_device(self, clips, out=None, layout: int = _lib.LAYOUT_NTCHW):
        """clips: contiguous float32 CUDA tensor [B,T,3,H,W] on this engine's device.  Enqueues on
        torch's current stream and returns a CUDA tensor [B,num_class] ([B,T,num_class] with consensus_type='identity';
        no host sync).  An engine takes ONE in-flight call: a host forward (``run`` / ``forward_host`` / ``forward_tap``) runs on the
        engine's own non-blocking stream over the same workspace, so synchronise (``torch.cuda.synchronize()`` or the stream) after
        a device forward before the next host call on this engine."""
        return self._run_logits(self._clips_input(clips, layout, True, 'forward_device needs a float32 CUDA tensor'), out, own_message=True)

    def forward_features(self, clips, normalize: bool = False, out=None, layout: int = _lib.LAYOUT_NTCHW):
        """Frame embeddings (``tsm_forward_features``; the reference's ``cnn_feature``, utils/common.py:79-106): the forward with
        ONE ``pool_feat_kernel`` launch in place of the head.  clips: what ``forward_device`` (a float32 CUDA tensor) or
        ``forward_host`` (an ndarray) takes.  Returns float32 [B*T, feature_dim] of the same kind: the mean over the pixels of
        every frame's last block output, or with ``normalize`` that row over its Euclidean norm (an all-zero row stays zero).
        ``out`` (CUDA input only): a contiguous float32 [B*T, feature_dim] tensor to write into, e.g. a band of a video's
        feature buffer.  Any engine: consensus, backbone, placement and dtype change nothing about the call."""
        self._need_finalized()
        on_device = hasattr(clips, 'is_cuda')
        if out is not None and not on_device:
            raise ValueError('out= goes with a CUDA tensor')
        need = 'forward_features needs a float32 CUDA tensor or an ndarray'
        return self._run_features(self._clips_input(clips, layout, on_device, need), normalize, out)

    def forward_tap(self, clips: np.ndarray, stage: str) -> np.ndarray:
        """Activation after ``stage`` as NHWC float32 ndarray (parity tests)."""
        inp = self._clips_input(clips, _lib.LAYOUT_NTCHW, False)
        n = inp.n_clips * self.num_segments
        h1, w1 = (self.height - 1) // 2 + 1, (self.width - 1) // 2 + 1          # stem conv output
        hp, wp = (h1 - 1) // 2 + 1, (w1 - 1) // 2 + 1                            # after the max-pool = layer1's size
        cap = n * max(h1 * w1 * 64, hp * wp * 256, self.height * self.width * 8)
        if self.convnext_depths:                                                  # the largest tap: fc1's output in stage 0
            cap = max(cap, n * (self.height // 4) * (self.width // 4) * 4 * CONVNEXT_WIDTHS[0])
        return self._run_tap(inp, stage, cap)

    # ---- a TDN engine's input as a pool of transformed frames (include/tsm_hip.h: TSM_LAYOUT_TDN_POOL) ------------------
    @staticmethod
    def _pool_source(frames, index, window, rows: tuple, keys: tuple):
        """The checks on WHERE in a pool the frames are found, once for ``forward_pool`` (``rows`` = (n_clips, T)) and
        ``tdn_segments`` ((n_segments,)): exactly one of an int32 table of ``rows x 5`` pool frame numbers and a window rule with
        exactly ``keys``.  Returns ``point(d, first)``, which points a descriptor at the chunk that starts ``first`` rows[0] on."""
        import torch
        if (index is None) == (window is None):
            raise ValueError('give exactly one of index (table mode) and window= (window mode)')
        if index is not None:
            if not (hasattr(index, 'is_cuda') and index.is_cuda and index.device == frames.device and index.dtype == torch.int32
                    and index.is_contiguous() and index.numel() == int(np.prod(rows)) * TDN_FRAMES):
                raise ValueError(f'index must be a contiguous int32 tensor of {" x ".join(str(r) for r in rows + (TDN_FRAMES,))} pool frame '
                                 f'numbers on {frames.device}')
        elif not isinstance(window, Mapping) or set(window) != set(keys):
            raise ValueError(f'window= must be a mapping with exactly the keys {keys}')
        else:
            window = {k: int(window[k]) for k in keys}

        def point(d, first: int) -> None:
            if index is not None:
                d.mode = _lib.TDN_POOL_TABLE
                d.index = index.data_ptr() + 4 * first * int(np.prod(rows[1:])) * TDN_FRAMES
            else:
                d.mode = _lib.TDN_POOL_WINDOW
                for k, v in window.items():
                    setattr(d, k, v)
                d.clip_step = window.get('clip_step', window['clip_stride'])      # (a segment is a clip of one: tdn_segments)
                d.first_clip = window['first_clip'] + first
        return point

    def _pool_input(self, frames, index, window, n_clips: int) -> '_Input':
        """The checks of ``forward_pool`` (the C ABI takes bare pointers) and one ``TsmTdnPool`` per ``max_clips`` chunk."""
        import torch
        self._need_finalized()
        if not self.tdn_depths:
            raise ValueError('forward_pool goes with a TDN engine (base_model=%r) only' % TDN)
        if not (hasattr(frames, 'is_cuda') and frames.is_cuda and frames.dtype == torch.float32 and frames.is_contiguous()):
            raise ValueError('frames must be a contiguous float32 CUDA tensor [n_frames, 3, H, W]')
        if frames.device.index != self.device:
            raise ValueError(f'tensor on cuda:{frames.device.index}, engine on cuda:{self.device}')
        if frames.dim() != 4 or tuple(frames.shape[1:]) != (3, self.height, self.width) or frames.shape[0] < 1:
            raise ValueError(f'frames must be [n_frames, 3, {self.height}, {self.width}], got {tuple(frames.shape)}')
        n_clips = int(n_clips)
        if n_clips <= 0:
            raise ValueError('n_clips must be positive')
        point = self._pool_source(frames, index, window, (n_clips, self.num_segments),
                                  ('first_source_frame', 'total_frames', 'first_clip', 'clip_step', 'clip_stride', 'pad_frame'))

        def make(s: int, _n: int):
            d = _lib.TsmTdnPool(struct_size=C.sizeof(_lib.TsmTdnPool), frames=frames.data_ptr(), n_frames=frames.shape[0])
            point(d, s)
            return d
        return self._descriptor_input(_lib.LAYOUT_TDN_POOL, n_clips, frames, make)

    def forward_pool(self, frames, index=None, *, window=None, n_clips: int, out=None):
        """The forward of a TDN engine on clips whose frames are FOUND in a pool (``tsm_forward`` with TSM_LAYOUT_TDN_POOL): no
        [B, T, 15, H, W] tensor exists.  frames: contiguous float32 CUDA tensor [n_frames, 3, H, W] of transformed frames, what
        ``preprocess_frames(packed=False)`` writes.  Exactly one of

        * ``index`` (table mode): int32 CUDA tensor [n_clips, T, 5] of pool frame numbers, read on the device when the kernel runs;
          an entry outside ``[0, n_frames)`` stands for a frame of zeros;
        * ``window=dict(first_source_frame, total_frames, first_clip, clip_step, clip_stride, pad_frame)`` (window mode): segment
          k of clip c has centre ``clip_step * c + clip_stride * k``, frame j is ``clamp(centre - 2 + j, 0, total_frames - 1) -
          first_source_frame``; a centre past the end or a frame outside the pool takes ``pad_frame``
          (``tdn_pipeline.tdn_clip_indices`` is the same rule in NumPy).  Nothing is uploaded.

        Enqueues on torch's current stream and returns what ``forward_device`` returns, bit for bit that of the gathered
        planes; more than ``max_clips`` clips run in chunks."""
        return self._run_logits(self._pool_input(frames, index, window, n_clips), out)

    def forward_features_pool(self, frames, index=None, *, window=None, n_clips: int, normalize: bool = False, out=None):
        """``forward_features`` on the clips ``forward_pool`` describes: float32 CUDA [n_clips * T, feature_dim]."""
        return self._run_features(self._pool_input(frames, index, window, n_clips), normalize, out)

    def forward_tap_pool(self, frames, stage: str, index=None, *, window=None, n_clips: int) -> np.ndarray:
        """``forward_tap`` on the clips ``forward_pool`` describes (at most ``max_clips``): the activation behind ``stage`` as an
        NHWC float32 ndarray (parity tests)."""
        inp = self._pool_input(frames, index, window, n_clips)      # (cap: forward_tap's bound, the stem conv's output, layer1's)
        return self._run_tap(inp, stage, inp.n_clips * self.num_segments * self.height * self.width * 16, 'forward_tap_pool')

    def preprocess_image_windows(self, arena, desc, n_windows: int, n_segment: Optional[int] = None, **kw):
        """``engine.preprocess_image_windows`` into THIS engine's input: its ``packed_layout``, its ``num_segments`` and the
        ``data_transform`` geometry ``create_image_model`` recorded (256 / the engine's height otherwise), unless given."""
        kw.setdefault('resize', int(getattr(self, 'image_resize', 256)))
        kw.setdefault('crop', int(getattr(self, 'image_crop', self.height)))
        kw.setdefault('out_layout', self.packed_layout)
        return preprocess_image_windows(arena, desc, n_windows, self.num_segments if n_segment is None else n_segment, **kw)

    # ---- a TDN forward in two phases (include/tsm_hip.h: TSM_LAYOUT_TDN_SEGMENTS / TSM_LAYOUT_TDN_RING) ------------------
    def ring_shapes(self, n_slots: int) -> tuple:
        """Shapes of a ring of ``n_slots`` per-segment features: (a [n, H / 4, W / 4, 256], d [n, H / 8, W / 8, 256])."""
        return ((int(n_slots), self.height // 4, self.width // 4, 256), (int(n_slots), self.height // 8, self.width // 8, 256))

    def _check_ring(self, a, d, what: str = 'ring') -> int:
        """The checks on a pair of per-segment feature tensors (the C ABI takes bare pointers); their slot count."""
        import torch
        self._need_finalized()
        if not self.tdn_depths:
            raise ValueError('the two-phase forward goes with a TDN engine (base_model=%r) only' % TDN)
        for t in (a, d):
            if not (hasattr(t, 'is_cuda') and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 4):
                raise ValueError(f'{what}: a and d must be contiguous float32 CUDA tensors [n, h, w, 256]')
            if t.device.index != self.device:
                raise ValueError(f'tensor on cuda:{t.device.index}, engine on cuda:{self.device}')
        n = int(a.shape[0])
        sa, sd = self.ring_shapes(n)
        if n < 1 or tuple(a.shape) != sa or tuple(d.shape) != sd:
            raise ValueError(f'{what}: need a {list(sa)} and d {list(sd)} with n >= 1, got {tuple(a.shape)} and {tuple(d.shape)}')
        return n

    def tdn_segments(self, frames, index=None, *, window=None, n_segments: int, out):
        """The SEGMENT phase of a TDN forward (``tsm_forward`` with TSM_LAYOUT_TDN_SEGMENTS): everything in front of ``fuse2``,
        once per segment.  ``frames`` is the pool of ``forward_pool``; exactly one of ``index`` (int32 CUDA ``[n_segments, 5]``
        pool frame numbers) and ``window=dict(first_source_frame, total_frames, first_clip, clip_stride, pad_frame)`` (segment i
        has centre ``clip_stride * (first_clip + i)``).  ``out=(a, d)``: float32 CUDA ``[n_segments, H / 4, W / 4, 256]`` and
        ``[n_segments, H / 8, W / 8, 256]`` -- usually slices of a ring -- which the last blocks of layer1 and resnext_layer1
        write directly.  More than ``max_clips * T`` segments run in chunks.  Enqueues on torch's current stream; returns ``out``."""
        import torch
        a, d = out
        n = int(n_segments)
        if self._check_ring(a, d, 'out') != n:
            raise ValueError(f'out holds {a.shape[0]} segments, n_segments = {n}')
        if not (hasattr(frames, 'is_cuda') and frames.is_cuda and frames.dtype == torch.float32 and frames.is_contiguous()
                and frames.dim() == 4 and tuple(frames.shape[1:]) == (3, self.height, self.width) and frames.shape[0] >= 1):
            raise ValueError(f'frames must be a contiguous float32 CUDA tensor [n_frames, 3, {self.height}, {self.width}]')
        if frames.device != a.device:
            raise ValueError(f'frames on {frames.device}, out on {a.device}')
        point = self._pool_source(frames, index, window, (n,), ('first_source_frame', 'total_frames', 'first_clip', 'clip_stride', 'pad_frame'))

        def make(s: int, m: int):
            desc = _lib.TsmTdnSegments(struct_size=C.sizeof(_lib.TsmTdnSegments), frames=frames.data_ptr(), n_frames=frames.shape[0],
                                       out_a=a[s:s + m].data_ptr(), out_d=d[s:s + m].data_ptr())
            point(desc, s)
            return desc
        inp = self._descriptor_input(_lib.LAYOUT_TDN_SEGMENTS, n, frames, make, self.max_clips * self.num_segments)
        for _s, m, address, _keepalive in inp.chunks:      # (the descriptor names the outputs: no out pointer)
            _lib.check(self._lib.tsm_forward(self._h, address, inp.memkind, inp.layout, m, None, inp.stream), self._h)
        return out

    def _ring_input(self, ring_a, ring_d, table, n_clips: int) -> '_Input':
        """The checks of ``forward_ring`` and one ``TsmTdnRing`` per ``max_clips`` chunk."""
        import torch
        n_slots = self._check_ring(ring_a, ring_d)
        n_clips, T = int(n_clips), self.num_segments
        if n_clips <= 0:
            raise ValueError('n_clips must be positive')
        if not (hasattr(table, 'is_cuda') and table.is_cuda and table.device == ring_a.device and table.dtype == torch.int32
                and table.is_contiguous() and table.numel() == n_clips * T):
            raise ValueError(f'table must be a contiguous int32 tensor of {n_clips} x {T} slot numbers on {ring_a.device}')
        return self._descriptor_input(_lib.LAYOUT_TDN_RING, n_clips, ring_a, lambda s, _n: _lib.TsmTdnRing(
            struct_size=C.sizeof(_lib.TsmTdnRing), n_slots=n_slots, ring_a=ring_a.data_ptr(), ring_d=ring_d.data_ptr(),
            table=table.data_ptr() + 4 * s * T))

    def forward_ring(self, ring_a, ring_d, table, *, n_clips: int, out=None):
        """The TRUNK phase of a TDN forward (``tsm_forward`` with TSM_LAYOUT_TDN_RING): ``fuse2`` onward on clips whose segments
        are FOUND in a ring that ``tdn_segments`` filled.  ``table``: int32 CUDA ``[n_clips, T]`` of slot numbers, read on the
        device when the kernel runs; an entry outside ``[0, n_slots)`` stands for a segment of zeros.  Returns what
        ``forward_pool`` returns for the clips those segments make, bit for bit; more than ``max_clips`` clips run in chunks."""
        return self._run_logits(self._ring_input(ring_a, ring_d, table, n_clips), out)

    def forward_features_ring(self, ring_a, ring_d, table, *, n_clips: int, normalize: bool = False, out=None):
        """``forward_features`` on the clips ``forward_ring`` describes: float32 CUDA [n_clips * T, feature_dim]."""
        return self._run_features(self._ring_input(ring_a, ring_d, table, n_clips), normalize, out)

    def forward_tap_ring(self, ring_a, ring_d, table, *, n_clips: int, stage: str) -> np.ndarray:
        """``forward_tap`` on the clips ``forward_ring`` describes (at most ``max_clips``; stages from ``fuse2`` on): the
        activation behind ``stage`` as an NHWC float32 ndarray (parity tests)."""
        inp = self._ring_input(ring_a, ring_d, table, n_clips)      # (cap: forward_tap's bound, layer1's width at its size)
        return self._run_tap(inp, stage, inp.n_clips * self.num_segments * self.height * self.width * 16, 'forward_tap_ring')

    def warmup(self, batch_sizes: Optional[Sequence[int]] = None) -> 'TsmEngine':
        """Tune every power-of-two bucket of the clip count that will occur (default: 1, 2, 4, ... max_clips) now
        (``tsm_tune``: a few hundred ms each of timed launches on the engine's own zeroed input buffer, or nothing when
        the tune cache file already holds the bucket), not inside the first real request."""
        import torch
        self._need_finalized()
        if batch_sizes is None:
            batch_sizes, b = [], 1
            while b < self.max_clips:
                batch_sizes.append(b)
                b *= 2
            batch_sizes.append(self.max_clips)
        stream = torch.cuda.current_stream(torch.device('cuda', self.device)).cuda_stream
        for b in batch_sizes:
            b = max(1, min(int(b), self.max_clips))
            _lib.check(self._lib.tsm_tune(self._h, b, stream), self._h)
        return self

    # ---- per-launch timing (bench.py roofline) -------------------------------------------------------
    def launch_names(self) -> List[str]:
        """Names of the kernel launches of one forward, in launch order (matches tsm_layer_times).  A non-local engine's
        wrapped blocks add four: the theta | phi | g conv, the pool, the attention and the W conv."""
        if self.tdn_depths:           # (csrc/tsm_engine.hip, run_tdn: one front + conv1_5 pair per chunk the engine's capacity holds)
            names = []
            for i in range(-(-self.max_clips // self.tdn_chunk_clips)):
                names += [f'diff.front.{i}', f'diff.conv1_5.{i}']
            names += ['diff.maxpool', 'conv1', 'fuse1']
            for li, nb in zip(range(5), (self.tdn_depths[0],) + tuple(self.tdn_depths)):      # 0: resnext_layer1
                for b in range(nb):
                    p = f'resnext_layer1.{b}' if li == 0 else f'layer{li}.{b}'
                    names += ['fuse2'] if (li, b) == (2, 0) else []
                    names += ([p + '.downsample'] if b == 0 else []) + [p + '.conv1']
                    names += [p + part for part in ('.mse_squeeze', '.mse_diff', '.mse_s2', '.mse_mix', '.mse_excite_shift')] if li >= 2 else []
                    names += [p + '.conv2', p + '.conv3']
            return names + ['head']
        if self.convnext_depths:      # (csrc/tsm_engine.hip, run_convnext)
            names = ['pack_input', 'stem.pack', 'stem.conv', 'stem.norm']
            for s, nb in enumerate(self.convnext_depths):
                names += [f'stages.{s}.downsample.norm', f'stages.{s}.downsample'] if s else []
                for b in range(nb):
                    names += [f'stages.{s}.blocks.{b}' + part for part in ('.dwln', '.fc1', '.gelu', '.fc2')]
            return names + ['head.pool', 'head.norm', 'head']
        names = ['pack_input', 'conv1', 'maxpool']
        blocks, kind = BACKBONES[self.base_model]
        for li, nb in enumerate(blocks, start=1):
            for b in range(nb):
                p = f'layer{li}.{b}'
                if kind == 'basic':   # [downsample,] conv1 (shift fused), conv2 (+ identity)
                    names += ([p + '.downsample'] if b == 0 and li > 1 else []) + [p + '.conv1', p + '.conv2']
                else:
                    names += ([p + '.downsample'] if b == 0 else []) + [p + '.conv1', p + '.conv2', p + '.conv3']
                    if self.non_local and (li, b) in NL_BLOCKS:
                        names += [p + '.nl.qkv', p + '.nl.pool', p + '.nl.attn', p + '.nl.W']
            if self.temporal_pool and li == 1:      # the pool's own launch, behind layer1's last block
                names.append('layer2.tpool')
        return names + ['head']

    @property
    def tdn_chunk_clips(self) -> int:
        """Clips per front-end chunk of a TDN engine (tsm_host_util.h: tdn_chunk_clips): at most 8, and few enough that the patch
        rows of a chunk stay below 2^29 floats."""
        per_clip = (self.height // 4) * (self.width // 4) * self.num_segments * 1024
        return max(1, min(8, self.max_clips, ((1 << 29) - 1) // per_clip))

    TILE_NAMES = {0: 'heuristic', 1: '128x128', 2: '128x64', 3: '64x64', 4: '32x32', 5: '128x128w8', 6: '256x256', 7: 'ws',
                  8: '256x256p', 9: '64x128'}

    @classmethod
    def tile_name(cls, code: int) -> str:
        """``tile + 256 * split``: '64x64/splitK' = one workgroup per (tile, K segment), combined in segment order
        (segmented fp32 layers at small batch); '64x64/pos' = position-major rows: a tile is one output position of 64 frames
        and the padding taps' K-steps are not issued (fp32 3x3 of layer2-4 on whole 64-frame batches); '64x64/tailK' = only the tiles of the last, partly filled round of resident
        workgroups run that way (ConvParams::ksplit = 2); '+conv3' on a block's conv2 = conv2 + conv3 + residual run as one fused
        kernel (the conv3 entry of that block is then unused); '+block' on a block's conv1 = the whole Bottleneck runs as one
        launch (bf16 layer1.1 / layer1.2; the conv2 / conv3 entries are then unused); '+conv1' on a block's conv3 = that
        launch also runs the NEXT block's shift + conv1 (bf16 layer2: conv31_fused_kernel; the next block's conv1 entry is then
        unused); '+conv2' on a block's conv1 = that launch also runs the block's stride-2 conv2 (bf16 layer2.0: front_s2_kernel; the
        conv2 entry is then unused)."""
        return (cls.TILE_NAMES[code & 15] + ('/pos' if code & 0x80 else '') + ('/splitK' if code & 0x100 else '') + ('/tailK' if code & 0x200 else '') + ('+conv3' if code & 0x400 else '') +
                ('+block' if code & 0x800 else '') + ('+conv1' if code & 0x1000 else '') + ('+conv2' if code & 0x2000 else ''))

    def conv_tiles(self, n_clips: int) -> Dict[str, str]:
        """Tile shape the autotuner chose per conv launch for an ``n_clips`` forward."""
        buf = (C.c_int32 * 256)()
        n = C.c_int32()
        _lib.check(self._lib.tsm_conv_tiles(self._h, n_clips, buf, 256, C.byref(n)), self._h)
        if self.tdn_depths:           # the stem, conv1_5 (one layer, whatever the chunks), then every block's convs
            names = ['conv1', 'diff.conv1_5'] + [k for k in self.launch_names() if k.startswith(('resnext_layer1.', 'layer'))
                                                 and k.endswith(('.downsample', '.conv1', '.conv2', '.conv3'))]
            assert n.value == len(names)
            return {k: self.tile_name(buf[i]) for i, k in enumerate(names)}
        if self.convnext_depths:
            names = [k for k in self.launch_names() if k == 'stem.conv' or k.endswith(('.downsample', '.fc1', '.fc2'))]
            assert n.value == len(names)
            return {k: self.tile_name(buf[i]) for i, k in enumerate(names)}
        names = [k for k in self.launch_names() if k not in ('pack_input', 'maxpool', 'head', 'layer2.tpool') and not k.endswith(('.nl.pool', '.nl.attn'))]
        assert n.value == len(names)
        return {k: self.tile_name(buf[i]) for i, k in enumerate(names)}

    def set_layer_timing(self, n_forwards: int, only_conv3x3: bool = False) -> None:
        _lib.check(self._lib.tsm_set_layer_timing(self._h, n_forwards, int(only_conv3x3)), self._h)

    def layer_times_ms(self, forward_index: int) -> Dict[str, float]:
        buf = (C.c_float * 512)()
        n = C.c_int32()
        _lib.check(self._lib.tsm_layer_times(self._h, forward_index, C.addressof(buf), 512, C.byref(n)), self._h)
        names = self.launch_names()
        assert n.value == len(names), (n.value, len(names))
        return {k: float(buf[i]) for i, k in enumerate(names)}

    @property
    def last_forward_ms(self) -> float:
        return float(self._lib.tsm_last_forward_ms(self._h))

    def _need_finalized(self) -> None:
        if not self._finalized:
            raise _lib.TsmError(-3, 'load_state_dict() has not been called')

    def close(self) -> None:
        if getattr(self, '_h', None) is not None and self._h.value:
            self._lib.tsm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _f32_only(family: str, dtype: str) -> None:
    """A family that runs in fp32 only: NotImplementedError for the bf16 formats, ValueError for an unknown dtype."""
    if dtype != 'f32':
        if dtype in _lib.DTYPES:
            raise NotImplementedError(f"{family} runs in dtype='f32' only, not {dtype!r}")
        raise ValueError(f'dtype must be one of {sorted(_lib.DTYPES)}, got {dtype!r}')


def _check_engine_args(base_model: str = 'resnet50', *, num_segments: int = 8, is_shift: bool = True, dtype: str = 'f32', height: int = 224,
                       width: int = 224, shift_place: str = 'blockres', consensus_type: str = 'avg', non_local: bool = False,
                       temporal_pool: bool = False, convnext_depths=None, tdn_depths=None, tdn_alpha=None, tdn_beta=None):
    """The argument checks of an engine, for ``TsmEngine`` and for the factories in front of their checkpoint: everything the
    engine cannot do is refused up front, never ignored, before the library loads.  Returns ``(convnext_depths, tdn_depths)``, each
    None unless the engine is of that family (then (3, 3, 27, 3) / (3, 4, 6, 3) unless given).

    * ``base_model='tdn_resnet50'``: fp32 only, no TSM shift, at least two segments, sides that are multiples of 32 and at least 64.
    * ``base_model='convnext_base'`` is an image model: one frame per clip, no temporal shift, fp32 only.
    * ``non_local=True``: Bottleneck backbones in fp32 (the bf16 formats' cross-block fused forms and storage formats do not know
      the block).
    * ``temporal_pool=True``: not ``dtype='bf16'`` (its cross-block and whole-block kernels tile over all T frames of a clip), not
      ``is_shift=False`` (make_temporal_pool is a branch of make_temporal_shift), not an odd ``num_segments``, and not together
      with ``non_local=True`` (whose wrapper assumes one segment count)."""
    tdn = base_model == TDN
    convnext = not tdn and is_convnext(base_model)
    if tdn:
        _f32_only(TDN, dtype)
        if is_shift:
            raise ValueError(f'{TDN} has no TSM shift (its temporal conv is learned): pass is_shift=False')
        if non_local or temporal_pool or shift_place != 'blockres':
            raise NotImplementedError(f'{TDN} has no non_local / temporal_pool / shift_place')
        if num_segments < 2:
            raise ValueError(f'{TDN} needs num_segments >= 2, got {num_segments}')
        if height < 64 or width < 64 or height % 32 or width % 32:
            raise ValueError(f'{TDN} needs height and width that are multiples of 32 and at least 64, got {height} x {width}')
        tdn_depths = _tdn_depths(tdn_depths)
    elif tdn_depths is not None or tdn_alpha is not None or tdn_beta is not None:
        raise ValueError(f'tdn_depths= / tdn_alpha= / tdn_beta= go with base_model={TDN!r} only')
    if convnext:
        _f32_only(CONVNEXT, dtype)
        if num_segments != 1 or is_shift:
            raise NotImplementedError(f'{CONVNEXT} is an image model (num_segments=1, is_shift=False): there is no temporal shift in this family')
        if non_local or temporal_pool or shift_place != 'blockres':
            raise NotImplementedError(f'{CONVNEXT} has no non_local / temporal_pool / shift_place')
        convnext_depths = _convnext_depths(convnext_depths)
    elif convnext_depths is not None:
        raise ValueError(f'convnext_depths= goes with base_model={CONVNEXT!r} only')
    elif not tdn and base_model not in DEPTHS:
        raise NotImplementedError(f'{base_model}: the engine implements {", ".join(sorted(DEPTHS))}')
    if non_local and not convnext and not tdn:
        if BACKBONES[base_model][1] != 'bottleneck':
            raise NotImplementedError(f'non_local=True needs a Bottleneck backbone (resnet50, wide_resnet50_2), not {base_model}')
        if dtype != 'f32':
            raise NotImplementedError(f"non_local=True runs in dtype='f32' only, not {dtype!r}")
    if temporal_pool:
        if dtype == 'bf16':
            raise NotImplementedError("temporal_pool=True runs in dtype='f32' and 'bf16x3' only, not 'bf16'")
        if non_local:
            raise NotImplementedError('temporal_pool=True and non_local=True exclude each other')
        if not is_shift:
            raise ValueError('temporal_pool=True needs is_shift=True')
        if num_segments <= 0 or num_segments % 2:
            raise ValueError(f'temporal_pool=True needs an even num_segments, got {num_segments}')
    if shift_place not in SHIFT_PLACES:
        raise ValueError(f"shift_place must be one of {list(SHIFT_PLACES)}, got {shift_place!r}")
    if consensus_type not in CONSENSUS_TYPES:
        raise ValueError(f"consensus_type must be one of {list(CONSENSUS_TYPES)}, got {consensus_type!r}")
    if dtype not in _lib.DTYPES:
        raise ValueError(f'dtype must be one of {sorted(_lib.DTYPES)}, got {dtype!r}')
    return convnext_depths, tdn_depths


def _device_index(device) -> int:
    """The factories' ``device`` argument (None, 'cuda', 'cuda:1', a ``torch.device``) as a device number; 'cpu' raises."""
    if device is None:
        return 0
    s = str(device)
    if s == 'cpu':
        raise RuntimeError('TsmEngine has no CPU path; pass a CUDA/HIP device')
    return int(s.split(':')[1]) if ':' in s else 0


def _is_onnx(checkpoint) -> bool:
    return checkpoint is not None and str(checkpoint).endswith('.onnx')


def _load_state_dict(checkpoint):
    """A ``torch.save``d checkpoint on the CPU: its ``state_dict`` entry where it has one, else the mapping itself."""
    import torch
    ckpt = torch.load(checkpoint, map_location='cpu')
    return ckpt['state_dict'] if 'state_dict' in ckpt else ckpt


def create_tdn_model(num_class: int, num_segments: int = 8, base_model: str = 'resnet50', num_frames: int = 5,
                     checkpoint: Optional[str] = None, consensus_type: str = 'avg', dropout: float = 0.5, partial_bn: bool = False,
                     fc_lr5: bool = False, device: Optional[object] = None, height: int = 224, width: int = 224, max_clips: int = 32,
                     seed: int = 0, dtype: str = 'f32', depths: Optional[Sequence[int]] = None, **kwargs) -> 'TsmEngine':
    """Counterpart of the reference's TDN factory (models/tdn.py:20-73: ``TSN(backbone_fn=tdn_net)``) returning a ready
    ``TsmEngine(base_model='tdn_resnet50', tdn_depths=(3, 4, 6, 3))`` with tdn_net's blend weights (0.5 / 0.5 at eight segments,
    else 0.75 / 0.25).  The engine takes [B, T, 5, 3, H, W], [B, T, 15, H, W] or [B*T*5, 3, H, W] -- one memory layout.
    ``checkpoint``: a ``torch.save``d TDN checkpoint (``weights.remap_tdn_keys``: ``state_dict`` wrapper, ``module.`` prefix and
    ``.net`` spellings as the reference's loader takes them; a ``new_fc`` of another class count raises).  Without one the engine
    gets the seeded weights of ``weights.make_tdn_state_dict``.  ``dropout`` / ``partial_bn`` / ``fc_lr5`` are training options.
    NotImplementedError, before the library loads: ``base_model='resnet101'`` (or anything but 'resnet50'), the bf16 formats, an
    ``.onnx`` file, ``num_frames != 5``.  ``depths``: blocks per stage of a shallower engine (tests)."""
    if base_model != 'resnet50':
        raise NotImplementedError(f'TDN on {base_model}: the engine implements resnet50 (depths 3, 4, 6, 3) only')
    if num_frames != TDN_FRAMES:
        raise NotImplementedError(f'num_frames must be {TDN_FRAMES} (four differences around the centre frame), got {num_frames}')
    assert consensus_type in ['avg', 'identity']
    _convnext, depths = _check_engine_args(TDN, num_segments=num_segments, is_shift=False, dtype=dtype, height=height, width=width,
                                           consensus_type=consensus_type, tdn_depths=depths)
    if _is_onnx(checkpoint):
        raise NotImplementedError('a TDN .onnx file: the importer reads TSM graphs only')
    dev = _device_index(device)
    if checkpoint is not None:
        sd = remap_tdn_keys(_load_state_dict(checkpoint), num_class, depths)
    else:
        sd = make_tdn_state_dict(seed=seed, num_class=num_class, depths=depths)
    alpha, beta = tdn_alpha_beta(num_segments)
    return TsmEngine(num_class=num_class, num_segments=num_segments, height=height, width=width, is_shift=False, max_clips=max_clips,
                     device=dev, state_dict=sd, dtype=dtype, base_model=TDN, consensus_type=consensus_type, tdn_depths=depths,
                     tdn_alpha=alpha, tdn_beta=beta)


def create_model(num_class: int = 2, num_segments: int = 8, base_model: str = 'resnet50',
                 checkpoint: Optional[str] = None, device: Optional[object] = None, fc_lr5: bool = True,
                 is_shift: bool = True, shift_div: int = 8, shift_place: str = 'blockres',
                 consensus_type: str = 'avg', img_feature_dim: int = 256, non_local: bool = False,
                 height: int = 224, width: int = 224, max_clips: int = 32, seed: int = 0, dtype: str = 'f32',
                 temporal_pool: bool = False, **kwargs) -> TsmEngine:
    """Counterpart of the reference factory (tsm.py:422-476) returning a ready TsmEngine.

    ``checkpoint`` is a ``torch.save``d dict with a ``state_dict`` entry (mmaction2 ``backbone.*``/``cls_head.*``
    checkpoints of the reference's --mmlab branch are recognised and mapped by ``weights.remap_mmaction_keys``); its keys are remapped like
    the reference does (strip the first dotted component, last two entries are the classifier).  A path
    ending in ``.onnx`` (the reference's exported model, scripts/export_model.py:35-47) is read by
    ``onnx_import.load_onnx_state_dict``.
    Without a checkpoint the reference starts from torchvision's ImageNet weights, which cannot be
    fetched offline: the engine then gets the seeded synthetic weights of ``weights.make_state_dict``.
    ``base_model``: 'resnet50' (Bottleneck), 'wide_resnet50_2' (Bottleneck, mid widths doubled: torchvision's
    width_per_group = 128; the keys are R50's), 'resnet18' or 'resnet34' (BasicBlock: the shift fused into the 3x3 conv1,
    fc [num_class, 512]); any other backbone raises NotImplementedError.
    ``shift_place``: 'blockres' (the shift wraps conv1 of every block) or 'block' (it wraps every block whole: the identity
    and the downsample read the shifted input too; state-dict keys ``base_model.layerL.B.net.*``); anything else raises
    as the reference's assert does.  ``is_shift=False`` ignores it.
    ``consensus_type``: 'avg' (logits [B, num_class], the mean of the segments' fc outputs) or 'identity' (the fc output of
    every segment, [B, T, num_class]: one launch, head_seg_kernel); anything else fails the reference's assert
    (tsm.py:438).  It is the caller's argument for every kind of checkpoint: an ``.onnx`` file is read for its weights only,
    the consensus is not detected from its graph.
    ``non_local=True``: blocks 0 and 2 of layer2 and 0, 2 and 4 of layer3 are wrapped in an embedded-Gaussian non-local block
    (self-attention over all T*H*W positions of a clip; state-dict keys ``layerL.B.block.*`` / ``layerL.B.nl.*``,
    include/tsm_hip.h: tsm_set_non_local).  ``dtype='f32'`` and Bottleneck backbones only; the bf16 formats, resnet18 / 34 and
    an ``.onnx`` checkpoint raise NotImplementedError, and mmaction2's non-local key spelling is not mapped.
    ``temporal_pool=True``: layer2 is wrapped in TemporalPool (a max-pool over time, kernel 3, stride 2, padding 1, per clip:
    include/tsm_hip.h: tsm_set_temporal_pool), so layers 2-4 and the head see ``num_segments // 2`` frames per clip
    (``engine.out_segments``): 'avg' logits stay [B, num_class], 'identity' logits are [B, T/2, num_class].  A checkpoint's
    ``layer2.net.<b>.*`` keys are mapped (``weights.remap_checkpoint_keys``).  ``dtype='bf16'``, ``non_local=True`` and an
    ``.onnx`` checkpoint raise NotImplementedError; ``is_shift=False`` and an odd ``num_segments`` raise ValueError.
    """
    if is_convnext(base_model):
        raise NotImplementedError(f'{base_model} is an image model: there is no temporal shift in this family; use create_image_model / '
                                  'create_feature_model')
    if base_model not in DEPTHS:
        raise NotImplementedError(f'{base_model}: the engine implements {", ".join(sorted(DEPTHS))}')
    assert consensus_type in ['avg', 'identity']
    _check_engine_args(base_model, num_segments=num_segments, is_shift=is_shift, dtype=dtype, height=height, width=width,
                       shift_place=shift_place, consensus_type=consensus_type, non_local=non_local, temporal_pool=temporal_pool)
    if non_local and _is_onnx(checkpoint):
        raise NotImplementedError('non_local=True with an .onnx checkpoint: the importer does not read non-local blocks')
    if temporal_pool and _is_onnx(checkpoint):
        raise NotImplementedError('temporal_pool=True with an .onnx checkpoint: the importer does not read the pooled graph')
    dev = _device_index(device)
    if _is_onnx(checkpoint):
        from .onnx_import import load_onnx_state_dict        # the reference's deployed artefact
        sd = load_onnx_state_dict(checkpoint, num_class, base_model, shift_place=shift_place)
    elif checkpoint is not None:
        raw = _load_state_dict(checkpoint)
        # mmaction2 checkpoints (the reference's --mmlab branch) vs the reference's own TSM / Lightning ones
        if non_local and is_mmaction_state_dict(raw):
            raise NotImplementedError('non_local=True with an mmaction2 checkpoint: its non-local key spelling is not mapped')
        sd = (remap_mmaction_keys(raw) if is_mmaction_state_dict(raw)
              else remap_checkpoint_keys(raw, num_class, base_model, non_local=non_local, temporal_pool=temporal_pool))
    else:
        sd = make_state_dict(seed=seed, num_class=num_class, base_model=base_model, shift_place=shift_place, non_local=non_local)
    return TsmEngine(num_class=num_class, num_segments=num_segments, height=height, width=width,
                     shift_div=shift_div, is_shift=is_shift, max_clips=max_clips, device=dev, state_dict=sd,
                     dtype=dtype, base_model=base_model, shift_place=shift_place, consensus_type=consensus_type,
                     non_local=non_local, temporal_pool=temporal_pool)


def create_image_model(num_class: int = 2, base_model: str = 'resnet18', checkpoint: Optional[str] = None, max_frames: int = 32,
                       dtype: str = 'f32', resize: int = 256, crop: int = 224, seed: int = 0,
                       device: Optional[object] = None) -> TsmEngine:
    """The reference's per-frame image classifier (image_classification.py:214: a torchvision ``resnet18`` with a replaced
    ``fc``; ``inference_image`` / ``count_by_image_model``, utils/inference_count.py:168-243) as a ``TsmEngine`` with
    ``num_segments=1``, ``is_shift=False``, ``consensus_type='avg'`` and ``height = width = crop``: one frame is one clip, so
    ``max_frames`` is the engine's ``max_clips``.  ``resize`` / ``crop`` are the ``data_transform`` the engine's frames go
    through (``engine.image_resize`` / ``engine.image_crop``; ``inference_count.inference_images`` reads them).
    ``checkpoint``: a ``torch.save``d ``state_dict`` (or a dict with a ``state_dict`` entry) with plain torchvision keys --
    ``conv1.weight``, ``layer1.0.*``, ``fc.*`` -- or a Lightning one whose keys carry one leading component
    (``weights.remap_torchvision_keys``).  Without one the engine gets the seeded synthetic weights, as ``create_model`` does.
    ``base_model='convnext_base'``: the classifier the reference's own image training produces (train_img.py:28-43:
    ``timm.create_model('convnext_base', num_classes=...)`` under a Lightning module's ``classifier``; timm 0.5.4) -- a
    ``TsmEngine(base_model='convnext_base', convnext_depths=(3, 3, 27, 3))``, include/tsm_hip.h: tsm_set_convnext.  Its
    ``checkpoint`` has timm's keys, with or without that one leading component (``weights.remap_timm_keys``).  ``dtype`` other
    than 'f32', an ``.onnx`` checkpoint and every other ConvNeXt variant raise NotImplementedError before the library loads."""
    return _create_frame_model(num_class, base_model, checkpoint, max_frames, dtype, resize, crop, seed, device)


def create_feature_model(base_model: str = 'resnet18', checkpoint: Optional[str] = None, max_frames: int = 32, dtype: str = 'f32',
                         resize: int = 224, crop: int = 224, seed: int = 0, device: Optional[object] = None) -> TsmEngine:
    """The reference's feature extractor (utils/common.py:129: ``timm.create_model(name, pretrained=True, num_classes=0)``) as
    a ``TsmEngine`` built like ``create_image_model``'s -- ``num_segments=1``, ``is_shift=False``, ``height = width = crop`` --
    whose product is ``forward_features`` ([n, feature_dim]: 512 for resnet18 / resnet34, 2048 for resnet50 /
    wide_resnet50_2); ``similarity.video_features`` / ``self_similarity`` drive it.  ``checkpoint``: a ``torch.save``d
    torchvision-keyed ``state_dict`` as ``create_image_model`` reads it; a ``num_classes=0`` model has no ``fc.*``, so a zero
    ``fc`` [1, feature_dim] stands in (the engine's finalize wants a classifier; its logits are never asked for).  Without a
    checkpoint: the seeded synthetic weights.  ``resize`` / ``crop``: ``Resize(resize)`` + ``CenterCrop(crop)`` through
    ``tsm_preprocess`` (the reference resizes to 224 without a crop; an engine has one geometry -- DESIGN 4.17).
    ``base_model='convnext_base'`` (timm keys, ``weights.remap_timm_keys``): ``forward_features`` is [n, 1024], the head
    LayerNorm's output -- what timm's ``num_classes=0`` model returns; the stand-in classifier is ``head.fc``."""
    return _create_frame_model(None, base_model, checkpoint, max_frames, dtype, resize, crop, seed, device)


def _create_frame_model(num_class: Optional[int], base_model: str, checkpoint, max_frames: int, dtype: str, resize: int, crop: int,
                        seed: int, device) -> TsmEngine:
    """The body of ``create_image_model`` and ``create_feature_model`` (``num_class=None``: one class, or the checkpoint's own,
    and a zero classifier where the checkpoint has none).  Every refusal -- another ConvNeXt variant, a bf16 format or an ``.onnx``
    file with ``convnext_base`` -- comes before a checkpoint is read or the library loads."""
    convnext = is_convnext(base_model)
    if not convnext and base_model not in DEPTHS:
        raise NotImplementedError(f'{base_model}: the engine implements {", ".join(sorted(DEPTHS))}')
    _check_engine_args(base_model, num_segments=1, is_shift=False, dtype=dtype, height=crop, width=crop)
    if convnext and _is_onnx(checkpoint):
        raise NotImplementedError(f'{base_model} with an .onnx checkpoint: the importer reads the TSM-ResNet export only')
    if crop > resize:
        raise ValueError(f'crop {crop} is larger than resize {resize}: the shorter side of a resized frame is {resize}')
    dev = _device_index(device)
    features, num_class = num_class is None, 1 if num_class is None else num_class
    if checkpoint is not None:
        sd = (remap_timm_keys if convnext else remap_torchvision_keys)(_load_state_dict(checkpoint))
        fc = 'head.fc' if convnext else 'fc'
        if features and fc + '.weight' in sd:
            num_class = int(sd[fc + '.weight'].shape[0])
        elif features:
            sd[fc + '.weight'] = np.zeros((1, feature_width(base_model)), dtype=np.float32)
            sd[fc + '.bias'] = np.zeros((1,), dtype=np.float32)
    else:
        sd = make_state_dict(seed=seed, num_class=num_class, base_model=base_model)
    eng = TsmEngine(num_class=num_class, num_segments=1, height=crop, width=crop, is_shift=False, max_clips=max_frames,
                    device=dev, state_dict=sd, dtype=dtype, base_model=base_model, consensus_type='avg',
                    convnext_depths=CONVNEXT_DEPTHS if convnext else None)
    eng.image_resize, eng.image_crop = int(resize), int(crop)
    return eng


# ---- launch trace (tests): which kernels did the calls inside the block launch? ----------------------------
class launch_trace:
    """``with launch_trace() as tr: ...`` records one line per kernel launch the library makes from THIS thread inside the
    block (``tsm_trace_launches`` / ``tsm_launch_trace``); afterwards ``tr.kernels`` is the list of kernel names as the launch
    sites spell them (template arguments of an enclosing launcher template resolved in a trailing ``[BM = 64, ...]``) and
    ``tr.ran('bneck_ws_kernel')`` asks for a family by prefix.  The bitwise tests of forced kernel forms use it to assert
    that the kernel under test is the one that ran -- a silent fall-back would make 'bit-identical' trivially true."""

    def __init__(self):
        self.kernels: List[str] = []

    def __enter__(self) -> 'launch_trace':
        _lib.load().tsm_trace_launches(1)
        return self

    def __exit__(self, *exc) -> None:
        lib = _lib.load()
        need = int(lib.tsm_launch_trace(None, 0))
        buf = C.create_string_buffer(need)
        lib.tsm_launch_trace(buf, need)
        lib.tsm_trace_launches(0)
        self.kernels = [ln for ln in buf.value.decode().split('\n') if ln]

    def ran(self, prefix: str) -> bool:
        return any(k.startswith(prefix) for k in self.kernels)

    def count(self, prefix: str) -> int:
        return sum(k.startswith(prefix) for k in self.kernels)


# ---- per-op wrappers over the C ABI (device tensors), used by tests ----------------------------------
def _ptr(t) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _stream(t) -> int:
    import torch
    return torch.cuda.current_stream(t.device).cuda_stream


def _need_cuda_f32(**tensors) -> None:
    """The C ABI takes bare device pointers: refuse anything that is not a float32 CUDA tensor up front."""
    import torch
    for name, t in tensors.items():
        if t is None:
            continue
        if not (hasattr(t, 'is_cuda') and t.is_cuda and t.dtype == torch.float32):
            raise ValueError(f'{name} must be a float32 CUDA tensor')


def _out(out, shape, dtype, like, name: str = 'out'):
    """The op wrappers' optional ``out=``: checked here, before anything is launched (the C ABI takes a bare pointer) -- a
    contiguous tensor of exactly this shape and dtype on `like`'s device; allocated when None."""
    import torch
    shape = tuple(int(d) for d in shape)
    if out is None:
        return torch.empty(shape, dtype=dtype, device=like.device)
    if not (hasattr(out, 'is_cuda') and out.is_cuda and out.device == like.device and out.dtype == dtype
            and tuple(out.shape) == shape and out.is_contiguous()):
        raise ValueError(f'{name} must be a contiguous {dtype} tensor of shape {shape} on {like.device}, got '
                         f'{getattr(out, "dtype", type(out))} {tuple(getattr(out, "shape", ()))} on {getattr(out, "device", None)}')
    return out


def temporal_shift_nhwc(x, n_segment: int, fold_div: int = 8, out=None):
    """x: CUDA float32 [N*T, H, W, C] (NHWC) -> shifted copy (tsm.py:35-50)."""
    import torch
    _need_cuda_f32(x=x)
    x = x.contiguous()
    n, h, w, c = x.shape
    if n_segment <= 0 or n % n_segment:
        raise ValueError(f'{n} frames are not a whole number of {n_segment}-frame clips')
    y = _out(out, x.shape, torch.float32, x)
    _lib.check(_lib.load().tsm_temporal_shift(x.data_ptr(), y.data_ptr(), n, n_segment, h * w, c, fold_div,
                                              _stream(x)))
    return y


def conv_bn_act_nhwc(x, w, gamma, beta, mean, var, stride: int = 1, relu: bool = True, residual=None,
                     shift_segments: int = 0, fold_div: int = 8, dtype: str = 'f32', *, shift_identity: bool = False,
                     x2=None, w2=None, bn2=None, stride2: int = 1, code: Optional[int] = None, reverse: bool = False, out=None,
                     segmented: bool = False):
    """x NHWC [n,h,w,cin], w OIHW; returns NHWC [n,ho,wo,cout].

    The keyword arguments reach the engine's other conv forms through ``tsm_conv_op``: ``shift_identity`` shifts the
    identity (the residual, else the second source; for a 1x1 at stride 2 the input) instead of the input; ``x2`` [n,h2,w2,cin2]
    with ``w2`` [cout,cin2,1,1] and ``bn2`` = (gamma, beta, mean, var) adds a 1x1 conv of x2 at ``stride2`` to a 1x1 main conv
    as one K-concatenated GEMM (conv3 + downsample); ``code`` is a tile code (0 = heuristic), ``reverse`` the tile walk.
    ``out``: write into this tensor (contiguous float32 [n,ho,wo,cout] on x's device) instead of allocating one.
    ``segmented``: a single fp32 source accumulates K in the engine's segments (TSM_CONV_CODE_SEGMENTED), the form the engine
    launches for its long-K layers, so that the split-K / tail-split codes apply; refused where no such kernel exists."""
    import torch
    _need_cuda_f32(x=x, w=w, gamma=gamma, beta=beta, mean=mean, var=var, residual=residual, x2=x2, w2=w2)
    x = x.contiguous()
    n, hi, wi, cin = x.shape
    cout, wcin, k, k2 = w.shape
    if wcin != cin or k != k2 or any(tuple(t.shape) != (cout,) for t in (gamma, beta, mean, var)):
        raise ValueError(f'w {tuple(w.shape)} / BatchNorm vectors do not match x {tuple(x.shape)}')
    pad = k // 2
    ho, wo = (hi + 2 * pad - k) // stride + 1, (wi + 2 * pad - k) // stride + 1
    y = _out(out, (n, ho, wo, cout), torch.float32, x)
    if residual is not None and tuple(residual.shape) != tuple(y.shape):
        raise ValueError(f'residual {tuple(residual.shape)} must have the output shape {tuple(y.shape)}')
    res = None if residual is None else residual.contiguous()
    args = [t.contiguous() for t in (w, gamma, beta, mean, var)]
    lib = _lib.load()
    if not shift_identity and x2 is None and code is None and not reverse and not segmented:
        _lib.check(lib.tsm_conv_bn_act(x.data_ptr(), *[a.data_ptr() for a in args], _ptr(res), y.data_ptr(),
                                       n, hi, wi, cin, cout, k, stride, int(relu), shift_segments, fold_div,
                                       _lib.DTYPES[dtype], _stream(x)))
        return y
    a = _lib.TsmConvArgs()
    a.struct_size = C.sizeof(_lib.TsmConvArgs)
    a.x, a.w, a.gamma, a.beta, a.mean, a.var = x.data_ptr(), *[t.data_ptr() for t in args]
    a.residual, a.y = _ptr(res), y.data_ptr()
    a.n, a.hi, a.wi, a.cin, a.cout, a.k, a.stride, a.relu = n, hi, wi, cin, cout, k, stride, int(relu)
    a.shift_segments, a.fold_div, a.dtype, a.shift_target = shift_segments, fold_div, _lib.DTYPES[dtype], int(shift_identity)
    keep = []   # (the contiguous copies must outlive the call)
    if x2 is not None:
        if w2 is None or bn2 is None:
            raise ValueError('a second source needs w2 and bn2')
        _need_cuda_f32(**{f'bn2[{i}]': t for i, t in enumerate(bn2)})
        x2c = x2.contiguous()
        n2, hi2, wi2, cin2 = x2c.shape
        if n2 != n or tuple(w2.shape) != (cout, cin2, 1, 1) or any(tuple(t.shape) != (cout,) for t in bn2):
            raise ValueError(f'x2 {tuple(x2.shape)} / w2 {tuple(w2.shape)} / bn2 do not match x {tuple(x.shape)}, cout {cout}')
        keep = [x2c] + [t.contiguous() for t in (w2, *bn2)]
        a.x2, a.w2, a.gamma2, a.beta2, a.mean2, a.var2 = (t.data_ptr() for t in keep)
        a.cin2, a.hi2, a.wi2, a.stride2 = cin2, hi2, wi2, stride2
    a.code, a.reverse = int(code or 0) | (_lib.CONV_CODE_SEGMENTED if segmented else 0), int(reverse)
    _lib.check(lib.tsm_conv_op(C.byref(a), _stream(x)))
    del keep
    return y


def _frame_shape(layout: int, size: int, what: str = 'layout') -> tuple:
    """Shape of ONE size x size frame as the frame transforms write it (float32 slots).  The bf16 formats store pixel PAIRS:
    one 8-element group = 2 pixels x 4 channels, split-bf16 in 8 float slots, bf16 in 4 (8 bf16 = 16 bytes)."""
    pairs = (size + 1) // 2
    shapes = {_lib.LAYOUT_NTHWC4: (size, size, 4), _lib.LAYOUT_NTHWC8S: (size, pairs, 8), _lib.LAYOUT_NTHWC8B: (size, pairs, 4),
              _lib.LAYOUT_NTCHW: (3, size, size)}
    if layout not in shapes:
        raise ValueError(f'{what} must be NTHWC4, NTHWC8S, NTHWC8B or NTCHW, got {layout}')
    return shapes[layout]


def _pixel_of(frames, want: str, u8_only: bool = False, min_frames: int = 0) -> int:
    """The C ABI's pixel code of staged raw frames -- a contiguous CUDA uint8 or float32 tensor [n >= min_frames,H,W,3] -- or
    ValueError (``want``: how the caller words that requirement)."""
    import torch
    if not u8_only and getattr(frames, 'dtype', None) not in (torch.uint8, torch.float32):
        raise ValueError(f'frames must be uint8 or float32, got {getattr(frames, "dtype", type(frames))}')
    if not (hasattr(frames, 'is_cuda') and frames.is_cuda and frames.dim() == 4 and frames.shape[3] == 3 and frames.is_contiguous()
            and frames.shape[0] >= min_frames and (frames.dtype == torch.uint8 or not u8_only)):
        raise ValueError(f'frames must be {want}')
    return _lib.PIXEL_U8 if frames.dtype == torch.uint8 else _lib.PIXEL_F32


def _staged_frames(frames, frame_format: str, colorimetry: Optional[str], want: str, min_frames: int = 0) -> tuple:
    """``(pixel, n, h, w)`` of staged raw frames: ``_pixel_of``'s for ``frame_format='rgb'``; for ``'nv12'`` a contiguous CUDA
    uint8 tensor [n, 3h/2, w] with h and w even (h, w: the luma size) and the pixel code of the colorimetry; for the other
    YUV formats (``transform.YUV_FORMATS``) the same with that format's container and parity.  Every refusal is a
    ValueError raised before the library is touched."""
    import torch
    from .transform import check_frame_format, yuv_luma_hw
    colorimetry = check_frame_format(frame_format, colorimetry)
    if frame_format == 'rgb':
        pixel = _pixel_of(frames, want, min_frames=min_frames)
        return (pixel,) + tuple(int(d) for d in frames.shape[:3])
    if not (hasattr(frames, 'is_cuda') and frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 3
            and frames.is_contiguous() and frames.shape[0] >= min_frames):
        raise ValueError(f'{frame_format.upper()} frames must be a contiguous uint8 CUDA tensor [n >= {min_frames}, rows, bytes], got '
                         f'{getattr(frames, "dtype", type(frames))} {tuple(getattr(frames, "shape", ()))}')
    h, w = yuv_luma_hw(frames.shape, frame_format)
    return _lib.pixel_code(frame_format, colorimetry), int(frames.shape[0]), h, w


def _yuv_bytes(frames, frame_format: str):
    """Staged frames as the uint8 container of their format: a 16-bit ``'p010'`` tensor [n, 3h/2, w] is viewed as bytes."""
    from .transform import yuv_frame_bytes_view
    return yuv_frame_bytes_view(frames, frame_format) if hasattr(frames, 'is_cuda') else frames


def preprocess_frames(frames, resize: int = 256, crop: int = 224, scale_255: bool = False, packed: bool = True,
                      layout: Optional[int] = None, out=None, frame_format: str = 'rgb', colorimetry: Optional[str] = None):
    """HIP test transform.  frames: CUDA uint8 or float32 [n,H,W,3] (decoder layout, values 0..255).
    Returns float32 [n,crop,crop,4] (``packed``: feed ``forward_device(..., layout=LAYOUT_NTHWC4)``),
    [n,3,crop,crop] (``packed=False``), or with ``layout=engine.packed_layout`` the packed format of that
    engine (LAYOUT_NTHWC8S for a bf16x3 engine: a float32-typed buffer [n,crop,ceil(crop/2),8] holding one
    split-bf16 group per pixel pair; LAYOUT_NTHWC8B: [n,crop,ceil(crop/2),4] float slots = 8 bf16 per pair).
    ``frame_format='nv12'``: frames are CUDA uint8 [n,3H/2,W] decoder surfaces (H, W even), converted to RGB inside the
    launch's taps by ``colorimetry`` (``transform.COLORIMETRIES``, default ``'bt601'``): bit for bit the result for
    ``transform.nv12_to_rgb(frames)``, and no RGB frame is written.  ``frame_format`` in ``transform.YUV_FORMATS``
    (``'i420'``, ``'yv12'``, ``'p010'``, ``'yuyv'``, ``'uyvy'``): the uint8 container of that format (a 16-bit ``'p010'``
    tensor is taken as its bytes), bit for bit the result for ``transform.yuv_to_rgb(frames, frame_format, colorimetry)``."""
    import torch
    if hasattr(frames, 'contiguous'):
        frames = frames.contiguous()
    frames = _yuv_bytes(frames, frame_format)
    pixel, n, h, w = _staged_frames(frames, frame_format, colorimetry, 'a CUDA tensor [n,H,W,3]')
    if layout is None:
        layout = _lib.LAYOUT_NTHWC4 if packed else _lib.LAYOUT_NTCHW
    out = _out(out, (n,) + _frame_shape(layout, crop), torch.float32, frames)
    _lib.check(_lib.load().tsm_preprocess(frames.data_ptr(), pixel, n, h, w, out.data_ptr(), layout, resize, crop,
                                          int(scale_255), _stream(frames)))
    return out


_image_tables_dev: Dict[tuple, object] = {}       # (h, w, resize, crop, device) -> int32 CUDA tensor


def image_tables_device(h: int, w: int, resize: int, crop: int, device):
    """``transform.image_tables`` on ``device``: built on the host in double once per geometry, uploaded once per device."""
    import torch
    from .transform import image_tables
    key = (int(h), int(w), int(resize), int(crop), str(device))
    t = _image_tables_dev.get(key)
    if t is None:
        if len(_image_tables_dev) >= 64:
            _image_tables_dev.clear()
        t = _image_tables_dev[key] = torch.from_numpy(image_tables(*key[:4]).copy()).to(device)
    return t


def preprocess_image(frames, resize: int = 256, crop: int = 224, out_layout: Optional[int] = None, out=None, tables=None):
    """The image model's per-frame transform on the GPU (``tsm_preprocess_image``: ``ToPILImage -> Resize(resize) ->
    CenterCrop(crop) -> ToTensor -> Normalize`` of utils/inference_count.py:27-34, Pillow's antialiased 8-bit resample to the
    bit), one launch.  frames: CUDA uint8 [n,H,W,3]; the channel order is kept as given (the reference feeds cv2's BGR frames
    to ToPILImage as they are: the caller's business).  Returns float32 in ``out_layout`` (default LAYOUT_NTHWC4), shaped as
    ``preprocess_frames`` shapes it.  ``tables``: the int32 CUDA table block of this geometry (``transform.image_tables``);
    built, cached and uploaded here when None."""
    import torch
    _pixel_of(frames, 'a contiguous uint8 CUDA tensor [n,H,W,3]', u8_only=True)
    n, h, w, _ = frames.shape
    layout = _lib.LAYOUT_NTHWC4 if out_layout is None else out_layout
    shape = (n,) + _frame_shape(layout, crop, 'out_layout')
    if tables is None:
        tables = image_tables_device(h, w, resize, crop, frames.device)
    elif not (hasattr(tables, 'is_cuda') and tables.is_cuda and tables.device == frames.device and tables.dtype == torch.int32
              and tables.dim() == 1 and tables.is_contiguous()):
        raise ValueError(f'tables must be a contiguous 1-d int32 tensor on {frames.device}')
    out = _out(out, shape, torch.float32, frames)
    _lib.check(_lib.load().tsm_preprocess_image(frames.data_ptr(), n, h, w, tables.data_ptr() if tables.numel() else None,
                                                tables.numel(), out.data_ptr(), layout, resize, crop, _stream(frames)))
    return out


def frame_votes(logits, history=None, out=None):
    """The image model's vote on the GPU (``tsm_frame_votes``; utils/inference_count.py:221-231): CUDA float32 logits
    [n, num_class] -> ``(pred, state, history)``: int32 [n] first arg-max per frame (numpy.argmax's tie rule), int32 [n]
    0 / 1 = ``sum(last <= 7 preds) >= 4``, and the int32 preds of the last min(6, ...) frames for the next batch.  The sum is
    over CLASS IDS, exactly as the reference's ``sum(que) >= 4`` -- not repaired for more than two classes.
    ``history``: int32 CUDA tensor of 0..6 preds of the frames before this batch (what the previous call returned), or None.
    ``out``: ``(pred [n], state [n], history [6])`` to write into; the history buffer must not be the one passed in.
    One launch on torch's current stream; no host sync."""
    import torch
    _need_cuda_f32(logits=logits)
    if logits.dim() != 2 or logits.shape[0] == 0 or logits.shape[1] == 0:
        raise ValueError(f'logits must be [n >= 1, num_class >= 1], got {tuple(logits.shape)}')
    logits = logits.contiguous()
    n, c = logits.shape
    n_hist = 0
    if history is not None:
        if not (hasattr(history, 'is_cuda') and history.is_cuda and history.device == logits.device and history.dtype == torch.int32
                and history.dim() == 1 and history.shape[0] <= 6 and history.is_contiguous()):
            raise ValueError(f'history must be a contiguous int32 tensor of at most 6 preds on {logits.device}')
        n_hist = int(history.shape[0])
    o_pred, o_state, o_hist = out if out is not None else (None, None, None)
    pred = _out(o_pred, (n,), torch.int32, logits, 'out[0]')
    state = _out(o_state, (n,), torch.int32, logits, 'out[1]')
    hist = _out(o_hist, (6,), torch.int32, logits, 'out[2]')
    if n_hist and hist.data_ptr() == history.data_ptr():
        raise ValueError('out[2] must not be the history passed in')
    _lib.check(_lib.load().tsm_frame_votes(logits.data_ptr(), n, c, history.data_ptr() if n_hist else None, n_hist,
                                           pred.data_ptr(), state.data_ptr(), hist.data_ptr(), _stream(logits)))
    return pred, state, hist[:min(6, n_hist + n)]


def gather_clips(frames, first_frame: int, total_frames: int, first_clip: int, n_clips: int, out=None,
                 n_segment: int = 8, clip_step: int = 8, clip_stride: int = 2, pad_frame: Optional[int] = None):
    """The clip windows of the dataset loop on the GPU (``tsm_gather_clips``; the reference's ``vid[i:i + 16:2]`` for
    ``i in range(0, len(vid), 8)``, tail zero-padded: utils/inference_count.py:411-414) over transformed frames.

    frames: CUDA tensor [n, ...] holding every ``clip_stride``-th frame of the video from source frame
    ``clip_stride * first_frame`` on (any ``preprocess_frames`` layout); ``pad_frame`` (default: the last frame of the
    buffer) stands in for positions past ``total_frames``.  Returns ``out`` [n_clips, n_segment, ...] (allocated when
    None; else any contiguous CUDA tensor of that many bytes, e.g. a slice of a persistent batch buffer)."""
    import torch
    if not frames.is_cuda or not frames.is_contiguous():
        raise ValueError('frames must be a contiguous CUDA tensor')
    n = int(frames.shape[0])
    frame_bytes = int(frames[0].numel()) * frames.element_size()
    if out is None:
        out = torch.empty((n_clips, n_segment) + tuple(frames.shape[1:]), dtype=frames.dtype, device=frames.device)
    if (not out.is_cuda or not out.is_contiguous() or out.device != frames.device
            or out.numel() * out.element_size() != n_clips * n_segment * frame_bytes):
        raise ValueError('out must be a contiguous CUDA tensor of n_clips * n_segment frames on the frames\' device')
    # (ranges of any length: the library cuts them into launches of <= 65535 rows itself)
    _lib.check(_lib.load().tsm_gather_clips(frames.data_ptr(), n, frame_bytes, int(first_frame), int(total_frames),
                                            n - 1 if pad_frame is None else int(pad_frame), int(first_clip), n_clips,
                                            n_segment, clip_step, clip_stride, out.data_ptr(), _stream(frames)))
    return out


def preprocess_clips(frames, boxes, first_frame: int, total_frames: int, first_clip: int, n_clips: int, size: int = 224,
                     scale_255: bool = False, layout: Optional[int] = None, packed: bool = True, n_segment: int = 8,
                     clip_step: int = 8, clip_stride: int = 2, out=None, frame_format: str = 'rgb',
                     colorimetry: Optional[str] = None):
    """The person-crop test transform fused with the clip windows (``tsm_preprocess_clips``: PersonCrop -> Resize((size,
    size)) -> Normalize of the reference's ``build_test_transform(person_crop=True)``, from the detector's box on), one
    launch from staged raw frames to the engine's input.

    frames: CUDA uint8 or float32 [n,H,W,3] (values 0..255) holding every ``clip_stride``-th frame of the video from source
    frame ``clip_stride * first_frame`` on (``gather_clips``' convention; no pad frame is needed).  boxes: CUDA int32
    [n_clips, 4] = (top, left, h, w) in source-frame pixels, row c for clip ``first_clip + c``; a box may leave the frame
    (zero fill) and a non-positive h or w stands for the whole frame.  Returns float32 [n_clips, n_segment, ...one frame]
    in the layouts of ``preprocess_frames`` with ``size`` in place of ``crop``; the zero-padded tail segments of the last
    clips are (0 - mean) / std.  ``frame_format='nv12'`` / ``colorimetry``: as ``preprocess_frames``; the boxes are in luma
    pixels and the zero fill is RGB 0."""
    import torch
    frames = _yuv_bytes(frames, frame_format)
    pixel, n, h, w = _staged_frames(frames, frame_format, colorimetry, 'a contiguous CUDA tensor [n,H,W,3]')
    if not (hasattr(boxes, 'is_cuda') and boxes.is_cuda and boxes.device == frames.device and boxes.dtype == torch.int32
            and tuple(boxes.shape) == (n_clips, 4) and boxes.is_contiguous()):
        raise ValueError(f'boxes must be a contiguous int32 tensor [{n_clips}, 4] = (top, left, h, w) on {frames.device}')
    if layout is None:
        layout = _lib.LAYOUT_NTHWC4 if packed else _lib.LAYOUT_NTCHW
    out = _out(out, (n_clips, n_segment) + _frame_shape(layout, size), torch.float32, frames)
    _lib.check(_lib.load().tsm_preprocess_clips(frames.data_ptr(), pixel, n, h, w, int(first_frame), int(total_frames),
                                                int(first_clip), n_clips, n_segment, clip_step, clip_stride, boxes.data_ptr(),
                                                out.data_ptr(), layout, size, int(scale_255), _stream(frames)))
    return out


def preprocess_indexed(frames, index, resize: int = 256, crop: int = 224, scale_255: bool = True, layout: Optional[int] = None,
                       out=None, frame_format: str = 'rgb', colorimetry: Optional[str] = None):
    """The centre-crop test transform through a device index table (``tsm_preprocess_indexed``), one launch from staged raw
    frames to the engine's input: the access pattern of the reference's ``FrameDataset`` (``sample_frames`` per labelled
    segment: irregular lists, repeated frames, no shared windows).

    frames: contiguous CUDA uint8 or float32 [n,H,W,3] (values 0..255), whatever frames the caller staged.  index: contiguous
    CUDA int32 [n_clips, n_segment] of buffer-frame numbers.  Returns float32 [n_clips, n_segment, ...one frame] in the
    layouts of ``preprocess_frames`` (default LAYOUT_NTHWC4); row (c, k) equals ``preprocess_frames``' row for frame
    ``index[c, k]`` bit for bit.  An entry outside [0, n) reads nothing and yields the normalised zero frame (0 - mean) / std
    -- the kernel is total in the table; validate the table on the host where a wrong entry should be an error.
    ``frame_format='nv12'`` / ``colorimetry``: as ``preprocess_frames``."""
    import torch
    if frame_format == 'rgb' and (not hasattr(frames, 'is_cuda') or frames.dtype not in (torch.uint8, torch.float32)):
        raise ValueError(f'frames must be a uint8 or float32 tensor, got {getattr(frames, "dtype", type(frames))}')
    frames = _yuv_bytes(frames, frame_format)
    pixel, n, h, w = _staged_frames(frames, frame_format, colorimetry, 'a contiguous CUDA tensor [n >= 1,H,W,3]', min_frames=1)
    if not (hasattr(index, 'is_cuda') and index.is_cuda and index.device == frames.device and index.dtype == torch.int32
            and index.dim() == 2 and index.shape[0] > 0 and index.shape[1] > 0 and index.is_contiguous()):
        raise ValueError(f'index must be a contiguous int32 tensor [n_clips >= 1, n_segment >= 1] on {frames.device}')
    n_clips, n_segment = (int(d) for d in index.shape)
    if layout is None:
        layout = _lib.LAYOUT_NTHWC4
    out = _out(out, (n_clips, n_segment) + _frame_shape(layout, crop), torch.float32, frames)
    _lib.check(_lib.load().tsm_preprocess_indexed(frames.data_ptr(), pixel, n, h, w, index.data_ptr(), n_clips, n_segment,
                                                  out.data_ptr(), layout, int(resize), int(crop), int(scale_255),
                                                  _stream(frames)))
    return out


def preprocess_windows(arena, desc, n_windows: int, n_segment: int = 8, person_crop: bool = False, resize: int = 256,
                       crop: int = 224, scale_255: bool = False, layout: Optional[int] = None, out=None,
                       frame_format: str = 'rgb', colorimetry: Optional[str] = None):
    """Either test transform over windows of different frame sizes (``tsm_preprocess_windows``), one launch from raw frames
    to the engine's input, in batch order: what one step of ``StreamBatcher`` needs.

    arena: contiguous CUDA uint8 or float32 tensor (values 0..255; any shape) holding every window's frames; desc: contiguous
    CUDA int32 [n_windows, 8], row c = (off_lo, off_hi, h, w, top, left, bh, bw) -- window c is ``n_segment`` contiguous
    frames [h, w, 3] from byte ``off`` of the arena on (``transform.window_descriptors`` builds and validates the table).
    ``person_crop=False``: Resize(resize) + CenterCrop(crop) + Normalize, every row bit for bit ``preprocess_frames``' row for
    that frame; ``True``: the window's box -> Resize((crop, crop)) -> Normalize, bit for bit ``preprocess_clips``' row.  Returns
    float32 [n_windows, n_segment, ...one frame] in the layouts of ``preprocess_frames`` (default LAYOUT_NTHWC4).  The kernel
    is total in the table: a window whose descriptor does not lie in the arena (or whose centre crop does not fit) reads
    nothing and yields normalised zero frames.  ``frame_format='nv12'``: the same uint8 arena with windows of ``n_segment``
    contiguous NV12 frames [3h/2, w] (``window_descriptors(..., frame_format='nv12')``; h, w of a row the luma size), converted
    in the taps by ``colorimetry``; a row with an odd side is invalid.  A ``transform.YUV_FORMATS`` name: windows of that
    format's frames, and a row whose side has the wrong parity for it is invalid."""
    import torch
    from .transform import check_frame_format
    colorimetry = check_frame_format(frame_format, colorimetry)
    if colorimetry is not None and getattr(arena, 'dtype', None) != torch.uint8:
        raise ValueError(f'an arena of {frame_format.upper()} windows must be a uint8 tensor')
    if not (hasattr(arena, 'is_cuda') and arena.is_cuda and arena.dtype in (torch.uint8, torch.float32) and arena.is_contiguous()
            and arena.numel() > 0 and arena.data_ptr() % 16 == 0):
        raise ValueError('arena must be a contiguous, 16-byte aligned, non-empty uint8 or float32 CUDA tensor')
    n_windows, n_segment = int(n_windows), int(n_segment)
    if n_windows <= 0 or n_segment <= 0:
        raise ValueError(f'n_windows and n_segment must be positive, got {n_windows}, {n_segment}')
    if not (hasattr(desc, 'is_cuda') and desc.is_cuda and desc.device == arena.device and desc.dtype == torch.int32
            and tuple(desc.shape) == (n_windows, 8) and desc.is_contiguous() and desc.data_ptr() % 16 == 0):
        raise ValueError(f'desc must be a contiguous, 16-byte aligned int32 tensor [{n_windows}, 8] on {arena.device}')
    if layout is None:
        layout = _lib.LAYOUT_NTHWC4
    out = _out(out, (n_windows, n_segment) + _frame_shape(layout, crop), torch.float32, arena)
    pixel = _lib.pixel_code(frame_format, colorimetry) if colorimetry is not None else _lib.PIXEL_U8 if arena.dtype == torch.uint8 else _lib.PIXEL_F32
    _lib.check(_lib.load().tsm_preprocess_windows(arena.data_ptr(), arena.numel() * arena.element_size(), pixel, desc.data_ptr(),
                                                  n_windows, n_segment, int(bool(person_crop)), out.data_ptr(), layout,
                                                  int(resize), int(crop), int(scale_255), _stream(arena)))
    return out


def preprocess_image_windows(arena, desc, n_windows: int, n_segment: int = 1, resize: int = 256, crop: int = 224,
                             out_layout: Optional[int] = None, frame_format: str = 'rgb', colorimetry: Optional[str] = None,
                             out=None):
    """The image model's transform over windows of different frame sizes (``tsm_preprocess_windows`` with ``person_crop =
    _lib.WINDOWS_IMAGE``), one launch from raw frames to the engine's input in batch order: what one step of
    ``ImageStreamBatcher`` needs.

    arena: contiguous, 16-byte aligned CUDA uint8 tensor holding every window's frames AND the coefficient block of every
    geometry (``transform.image_tables``); desc: contiguous CUDA int32 [n_windows, 8], row c = (off_lo, off_hi, h, w, tab_lo,
    tab_hi, 0, 0) (``transform.image_window_descriptors`` builds and validates it, ``transform.image_window_arena`` lays the
    arena out).  Returns float32 [n_windows, n_segment, ...one frame] in ``out_layout`` (default LAYOUT_NTHWC4); every row
    equals ``preprocess_image``'s row for that frame bit for bit.  ``frame_format='nv12'``: windows of NV12 frames [3h/2, w]
    converted tap by tap by ``colorimetry`` -- ``preprocess_image`` of ``transform.nv12_to_rgb`` of the frame; any other format
    is NotImplementedError.  The kernel is total in the table: an invalid window reads nothing and yields normalised zero
    frames."""
    import torch
    from .transform import IMAGE_WINDOW_FORMATS, check_frame_format
    if frame_format not in IMAGE_WINDOW_FORMATS:
        raise NotImplementedError(f'the image transform takes frame_format in {IMAGE_WINDOW_FORMATS}, got {frame_format!r}')
    colorimetry = check_frame_format(frame_format, colorimetry)
    if not (hasattr(arena, 'is_cuda') and arena.is_cuda and arena.dtype == torch.uint8 and arena.is_contiguous()
            and arena.numel() > 0 and arena.data_ptr() % 16 == 0):
        raise ValueError('arena must be a contiguous, 16-byte aligned, non-empty uint8 CUDA tensor')
    n_windows, n_segment = int(n_windows), int(n_segment)
    if n_windows <= 0 or n_segment <= 0:
        raise ValueError(f'n_windows and n_segment must be positive, got {n_windows}, {n_segment}')
    if not (hasattr(desc, 'is_cuda') and desc.is_cuda and desc.device == arena.device and desc.dtype == torch.int32
            and tuple(desc.shape) == (n_windows, 8) and desc.is_contiguous() and desc.data_ptr() % 16 == 0):
        raise ValueError(f'desc must be a contiguous, 16-byte aligned int32 tensor [{n_windows}, 8] on {arena.device}')
    layout = _lib.LAYOUT_NTHWC4 if out_layout is None else out_layout
    out = _out(out, (n_windows, n_segment) + _frame_shape(layout, crop, 'out_layout'), torch.float32, arena)
    pixel = _lib.pixel_code(frame_format, colorimetry) if colorimetry is not None else _lib.PIXEL_U8
    _lib.check(_lib.load().tsm_preprocess_windows(arena.data_ptr(), arena.numel(), pixel, desc.data_ptr(), n_windows, n_segment,
                                                  _lib.WINDOWS_IMAGE, out.data_ptr(), layout, int(resize), int(crop), 0,
                                                  _stream(arena)))
    return out


def top1_tally(logits, labels, correct, total, out=None):
    """The accuracy tally on the GPU (``tsm_top1_tally``; the intent of scripts/eval_classification.py:42-49): CUDA float32
    logits [n, num_class] and int32 labels [n] -> int32 ``pred`` [n], the first arg-max per row (numpy.argmax's tie rule),
    while the int32 counters ``correct`` / ``total`` [num_class] ACCUMULATE ``pred == label`` / 1 under every label in
    [0, num_class); any other label is counted nowhere.  Zero the counters once, call this once per batch (on one stream),
    read them once.  ``out``: the pred tensor to write into.  One launch on torch's current stream; no host sync."""
    import torch
    _need_cuda_f32(logits=logits)
    if logits.dim() != 2 or logits.shape[0] == 0 or logits.shape[1] == 0 or not logits.is_contiguous():
        raise ValueError(f'logits must be contiguous [n >= 1, num_class >= 1], got {tuple(logits.shape)}')
    n, c = (int(d) for d in logits.shape)
    for name, t, shape in (('labels', labels, (n,)), ('correct', correct, (c,)), ('total', total, (c,))):
        if not (hasattr(t, 'is_cuda') and t.is_cuda and t.device == logits.device and t.dtype == torch.int32
                and tuple(t.shape) == shape and t.is_contiguous()):
            raise ValueError(f'{name} must be a contiguous int32 tensor of shape {shape} on {logits.device}')
    if correct.data_ptr() == total.data_ptr():
        raise ValueError('correct and total must be two tensors')
    pred = _out(out, (n,), torch.int32, logits)
    _lib.check(_lib.load().tsm_top1_tally(logits.data_ptr(), labels.data_ptr(), n, c, pred.data_ptr(), correct.data_ptr(),
                                          total.data_ptr(), _stream(logits)))
    return pred


def scores_to_states(logits, threshold: float = 0.5, softmax: bool = True, return_top: bool = False, out=None, out_top=None):
    """K9 on the GPU: CUDA float32 logits [n, num_class] -> int32 states [n] (utils/eval.py:153-164: softmax, first
    arg-max, class id if its score >= threshold else -1) and optionally the winning score.  Enqueues on torch's
    current stream; no host sync."""
    import torch
    _need_cuda_f32(logits=logits)
    if logits.dim() != 2 or logits.shape[0] == 0:
        raise ValueError(f'logits must be [n >= 1, num_class], got {tuple(logits.shape)}')
    logits = logits.contiguous()
    n, c = logits.shape
    if out_top is not None and not return_top:
        raise ValueError('out_top needs return_top=True')
    states = _out(out, (n,), torch.int32, logits)
    top = _out(out_top, (n,), torch.float32, logits, 'out_top') if return_top else None
    _lib.check(_lib.load().tsm_scores_to_states(logits.data_ptr(), n, c, int(softmax), float(threshold),
                                                states.data_ptr(), _ptr(top), _stream(logits)))
    return (states, top) if return_top else states


def maxpool3x3s2_nhwc(x, out=None):
    import torch
    _need_cuda_f32(x=x)
    x = x.contiguous()
    n, hi, wi, c = x.shape
    y = _out(out, (n, (hi - 1) // 2 + 1, (wi - 1) // 2 + 1, c), torch.float32, x)
    _lib.check(_lib.load().tsm_maxpool3x3s2(x.data_ptr(), y.data_ptr(), n, hi, wi, c, _stream(x)))
    return y


def _rows_view(t, name: str):
    """(pointer, row stride in floats, shape) of a tensor whose LAST dimension is contiguous and whose leading dimensions
    are laid out like a contiguous tensor of rows ``ld`` floats apart: a contiguous tensor or a channel slice of one."""
    shape = tuple(int(d) for d in t.shape)
    strides = tuple(int(v) for v in t.stride())
    ld, acc, ok = None, 1, strides[-1] == 1 or shape[-1] == 1
    for dim, st in zip(reversed(shape[:-1]), reversed(strides[:-1])):      # (the stride of a dimension of size 1 means nothing)
        if dim != 1:
            if ld is None:
                ok, ld = ok and st % acc == 0, st // acc
            else:
                ok = ok and st == ld * acc
        acc *= dim
    ld = shape[-1] if ld is None else ld
    if not ok or ld < shape[-1] or 0 in shape:
        raise ValueError(f'{name} must be a non-empty contiguous tensor or a channel slice of one, got shape {shape} strides {strides}')
    return t.data_ptr(), ld, shape


def maxpool2x2_nhwc(x, c0: int = 0, c: Optional[int] = None, out=None):
    """``tsm_maxpool2x2``: MaxPool3d((1, 2, 2)) of channels [c0, c0 + c) of x, CUDA float32 [N, H, W, C] (NHWC; a channel
    slice of a wider tensor keeps its row stride) -> dense [N, H // 2, W // 2, c].  Floor mode: a last odd row / column is
    dropped.  One launch on torch's current stream."""
    import torch
    _need_cuda_f32(x=x)
    ptr, ld, (n, hi, wi, cx) = _rows_view(x, 'x')
    c = cx - c0 if c is None else int(c)
    if c0 < 0 or c <= 0 or c0 + c > cx:
        raise ValueError(f'channels [{c0}, {c0 + c}) are not inside the {cx} of x')
    y = _out(out, (n, hi // 2, wi // 2, c), torch.float32, x)
    _lib.check(_lib.load().tsm_maxpool2x2(ptr, ld, c0, c, y.data_ptr(), n, hi, wi, _stream(x)))
    return y


def nonlocal_attention(q, k, v, out=None):
    """``tsm_nonlocal_attention``: q CUDA float32 [B, Nq, d], k and v [B, Nk, d] (each a contiguous tensor or a channel slice
    of one; k and v with the same row stride) -> y [B, Nq, d] = softmax_j(q . k^T) v without a scale factor, by the fused
    online-softmax kernel (d = 256 or 512; nothing of size Nq * Nk is allocated).  ``out``: a contiguous [B, Nq, d] tensor.
    One launch on torch's current stream."""
    import torch
    _need_cuda_f32(q=q, k=k, v=v)
    qp, ldq, (b, nq, d) = _rows_view(q, 'q')
    kp, ldk, kshape = _rows_view(k, 'k')
    vp, ldv, vshape = _rows_view(v, 'v')
    if kshape != vshape or kshape[0] != b or kshape[2] != d or ldk != ldv:
        raise ValueError(f'q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)} do not fit (k and v share shape and row stride)')
    y = _out(out, (b, nq, d), torch.float32, q)
    _lib.check(_lib.load().tsm_nonlocal_attention(qp, ldq, kp, vp, ldk, y.data_ptr(), d, b, nq, kshape[1], d, _stream(q)))
    return y


def head_nhwc(feat, fc_w, fc_b, n_segment: int, out=None):
    import torch
    _need_cuda_f32(feat=feat, fc_w=fc_w, fc_b=fc_b)
    feat = feat.contiguous()
    n, h, w, c = feat.shape
    if n_segment <= 0 or n % n_segment or tuple(fc_w.shape)[1:] != (c,) or tuple(fc_b.shape) != (fc_w.shape[0],):
        raise ValueError(f'feat {tuple(feat.shape)}, fc_w {tuple(fc_w.shape)}, fc_b {tuple(fc_b.shape)}, T={n_segment} do not fit')
    b = n // n_segment
    out = _out(out, (b, fc_w.shape[0]), torch.float32, feat)
    _lib.check(_lib.load().tsm_head(feat.data_ptr(), fc_w.contiguous().data_ptr(), fc_b.contiguous().data_ptr(),
                                    out.data_ptr(), b, n_segment, h * w, c, fc_w.shape[0], _stream(feat)))
    return out


def head_segments_nhwc(feat, fc_w, fc_b, out=None):
    """The per-segment head (``tsm_head_segments``): feat CUDA float32 [n_frames, H, W, C] (NHWC) -> logits
    [n_frames, num_class], fc of every frame's average-pooled features (consensus_type='identity': no mean over the segments)."""
    import torch
    _need_cuda_f32(feat=feat, fc_w=fc_w, fc_b=fc_b)
    feat = feat.contiguous()
    n, h, w, c = feat.shape
    if n <= 0 or h * w <= 0 or tuple(fc_w.shape)[1:] != (c,) or tuple(fc_b.shape) != (fc_w.shape[0],):
        raise ValueError(f'feat {tuple(feat.shape)}, fc_w {tuple(fc_w.shape)}, fc_b {tuple(fc_b.shape)} do not fit')
    out = _out(out, (n, fc_w.shape[0]), torch.float32, feat)
    _lib.check(_lib.load().tsm_head_segments(feat.data_ptr(), fc_w.contiguous().data_ptr(), fc_b.contiguous().data_ptr(),
                                             out.data_ptr(), n, h * w, c, fc_w.shape[0], _stream(feat)))
    return out


def pool_features_nhwc(feat, out=None, out_unit=None):
    """The pool of ``forward_features`` on its own (``tsm_pool_features``): feat CUDA float32 [n_frames, H, W, C] (NHWC) ->
    ``(pooled, unit)``, each [n_frames, C]: the mean over the pixels (``head_nhwc``'s pooled value to the bit) and that row
    over its Euclidean norm (a zero row stays zero).  ``out`` / ``out_unit``: tensors to write into; pass ``False`` for one
    of them to skip that output (it is then returned as None).  One launch on torch's current stream; no host sync."""
    import torch
    _need_cuda_f32(feat=feat)
    feat = feat.contiguous()
    n, h, w, c = feat.shape
    if n <= 0 or h * w <= 0:
        raise ValueError(f'feat {tuple(feat.shape)} is empty')
    if out is False and out_unit is False:
        raise ValueError('at least one of out / out_unit must be produced')
    pooled = None if out is False else _out(out, (n, c), torch.float32, feat)
    unit = None if out_unit is False else _out(out_unit, (n, c), torch.float32, feat, 'out_unit')
    _lib.check(_lib.load().tsm_pool_features(feat.data_ptr(), _ptr(pooled), _ptr(unit), n, h * w, c, _stream(feat)))
    return pooled, unit


def cosine_distances(unit, out=None, rows=None):
    """The cosine-distance matrix of unit rows (``tsm_cosine_distances``; scikit-learn's ``cosine_distances(X)``, which the
    reference's ``plot_sim`` calls through ``pairwise_distances(metric='cosine')``): unit CUDA float32 [n, C], rows of unit
    length -> ``out`` [n, n] with D[i][j] = clip(1 - <u_i, u_j>, 0, 2), a zero diagonal and D == D.T bit for bit.
    ``rows=(row0, row1)`` writes the band i in [row0, row1), j in [0, row1) and its mirror only (rows of ``unit`` from row1
    on are not read, the rest of ``out`` is not touched): call once per batch of a long video; the bands add up to the
    one-shot matrix bit for bit.  ``out`` is allocated (uninitialised outside the band) when None.  One launch; no host sync."""
    import torch
    _need_cuda_f32(unit=unit)
    if unit.dim() != 2 or unit.shape[0] == 0 or not unit.is_contiguous():
        raise ValueError(f'unit must be contiguous [n >= 1, C], got {tuple(unit.shape)}')
    n, c = (int(d) for d in unit.shape)
    row0, row1 = (0, n) if rows is None else (int(rows[0]), int(rows[1]))
    out = _out(out, (n, n), torch.float32, unit)
    _lib.check(_lib.load().tsm_cosine_distances(unit.data_ptr(), n, c, row0, row1, out.data_ptr(), _stream(unit)))
    return out
