"""ctypes binding of libtsm_hip.so (include/tsm_hip.h).  Fails loudly when the library is missing:
there is no CPU fallback for the product path."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

from .build import LIB_PATH, build_id

ABI_VERSION = 7

MEM_HOST, MEM_DEVICE = 0, 1
LAYOUT_NTCHW, LAYOUT_NTHWC, LAYOUT_NTHWC4, LAYOUT_NTHWC8S, LAYOUT_NTHWC8B = 0, 1, 2, 3, 4
LAYOUT_TDN_POOL = 16      # a TDN engine's input as a TsmTdnPool descriptor (host memory) naming device memory
LAYOUT_TDN_SEGMENTS = 17  # the segment phase of a TDN forward: a TsmTdnSegments descriptor, n_clips counts segments
LAYOUT_TDN_RING = 18      # the trunk phase: a TsmTdnRing descriptor naming a ring of per-segment features and a slot table
TDN_POOL_TABLE, TDN_POOL_WINDOW = 0, 1
WINDOWS_IMAGE = 16        # tsm_preprocess_windows' person_crop argument: the image model's transform (TSM_WINDOWS_IMAGE)
PIXEL_U8, PIXEL_F32 = 0, 1
PIXEL_NV12_BT601, PIXEL_NV12_BT709, PIXEL_NV12_BT601_FULL, PIXEL_NV12_BT709_FULL = 16, 17, 18, 19
_NV12_PIXELS = {'bt601': PIXEL_NV12_BT601, 'bt709': PIXEL_NV12_BT709, 'bt601-full': PIXEL_NV12_BT601_FULL,
                'bt709-full': PIXEL_NV12_BT709_FULL}


def nv12_pixel(colorimetry: str = 'bt601') -> int:
    """The tsm_pixel code of NV12 frames of a colorimetry (transform.COLORIMETRIES), or ValueError."""
    try:
        return _NV12_PIXELS[colorimetry]
    except (KeyError, TypeError):
        raise ValueError(f'colorimetry must be one of {tuple(_NV12_PIXELS)}, got {colorimetry!r}') from None


# The other YUV formats: code 32 + 4 f + c, f in the order of YUV_FORMATS, c in the order of the NV12 codes (include/tsm_hip.h).
YUV_FORMATS = ('i420', 'yv12', 'p010', 'yuyv', 'uyvy')
PIXEL_YUV_BASE = 32
for _f, _name in enumerate(YUV_FORMATS):
    for _c, _col in enumerate(_NV12_PIXELS):
        globals()[f'PIXEL_{_name.upper()}_{_col.upper().replace("-", "_")}'] = PIXEL_YUV_BASE + 4 * _f + _c
del _f, _name, _c, _col


def pixel_code(frame_format: str, colorimetry=None) -> int:
    """The tsm_pixel code of uint8 frames of a frame format (``'rgb'``, ``'nv12'`` or one of YUV_FORMATS) and, for the YUV
    formats, a colorimetry (transform.COLORIMETRIES; None: ``'bt601'``); ValueError for an unknown name, or a colorimetry given with ``'rgb'``."""
    if frame_format == 'rgb':
        if colorimetry is not None:
            raise ValueError(f"colorimetry={colorimetry!r} was given with frame_format='rgb': RGB frames have none")
        return PIXEL_U8
    c = nv12_pixel('bt601' if colorimetry is None else colorimetry) - PIXEL_NV12_BT601
    if frame_format == 'nv12':
        return PIXEL_NV12_BT601 + c
    if not isinstance(frame_format, str) or frame_format not in YUV_FORMATS:
        raise ValueError(f"frame_format must be one of {('rgb', 'nv12') + YUV_FORMATS}, got {frame_format!r}")
    return PIXEL_YUV_BASE + 4 * YUV_FORMATS.index(frame_format) + c


DTYPE_F32, DTYPE_BF16X3, DTYPE_BF16 = 0, 1, 2
CONV_CODE_SEGMENTED = 0x4000   # TSM_CONV_CODE_SEGMENTED: tsm_conv_args.code only
DTYPES = {'f32': DTYPE_F32, 'bf16x3': DTYPE_BF16X3, 'bf16': DTYPE_BF16}

STATUS_NAMES = {0: 'TSM_OK', -1: 'TSM_ERR_INVALID_ARG', -2: 'TSM_ERR_HIP', -3: 'TSM_ERR_NOT_FINALIZED',
                -4: 'TSM_ERR_MISSING_TENSOR', -5: 'TSM_ERR_SHAPE', -6: 'TSM_ERR_CAPACITY',
                -7: 'TSM_ERR_UNSUPPORTED', -8: 'TSM_ERR_GUARD'}


class TsmConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ('struct_size', 'num_class', 'num_segments', 'height', 'width',
                                         'shift_div', 'is_shift', 'max_clips', 'device_id', 'dtype')]


class TsmTdnPool(C.Structure):
    """struct tsm_tdn_pool (include/tsm_hip.h): what ``clips`` points to with LAYOUT_TDN_POOL."""
    _fields_ = [('struct_size', C.c_uint32), ('mode', C.c_int32), ('frames', C.c_void_p), ('n_frames', C.c_int64),
                ('index', C.c_void_p), ('first_source_frame', C.c_int64), ('total_frames', C.c_int64), ('first_clip', C.c_int64),
                ('clip_step', C.c_int32), ('clip_stride', C.c_int32), ('pad_frame', C.c_int64)]


class TsmTdnSegments(C.Structure):
    """struct tsm_tdn_segments (include/tsm_hip.h): what ``clips`` points to with LAYOUT_TDN_SEGMENTS."""
    _fields_ = TsmTdnPool._fields_ + [('out_a', C.c_void_p), ('out_d', C.c_void_p)]


class TsmTdnRing(C.Structure):
    """struct tsm_tdn_ring (include/tsm_hip.h): what ``clips`` points to with LAYOUT_TDN_RING."""
    _fields_ = [('struct_size', C.c_uint32), ('n_slots', C.c_int32), ('ring_a', C.c_void_p), ('ring_d', C.c_void_p),
                ('table', C.c_void_p)]


class TsmError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f'{STATUS_NAMES.get(status, status)}: {message}')
        self.status = status


class TsmConvArgs(C.Structure):
    """struct tsm_conv_args (include/tsm_hip.h), the argument block of tsm_conv_op."""
    _fields_ = ([('struct_size', C.c_int32)] + [(n, C.c_void_p) for n in ('x', 'w', 'gamma', 'beta', 'mean', 'var', 'residual', 'y')]
                + [(n, C.c_int32) for n in ('n', 'hi', 'wi', 'cin', 'cout', 'k', 'stride', 'relu', 'shift_segments', 'fold_div',
                                            'dtype', 'shift_target')]
                + [(n, C.c_void_p) for n in ('x2', 'w2', 'gamma2', 'beta2', 'mean2', 'var2')]
                + [(n, C.c_int32) for n in ('cin2', 'hi2', 'wi2', 'stride2', 'code', 'reverse')])


EXPORTS = ('tsm_abi_version', 'tsm_build_id', 'tsm_trace_launches', 'tsm_launch_trace', 'tsm_create', 'tsm_destroy', 'tsm_last_error', 'tsm_set_backbone', 'tsm_set_bottleneck_width', 'tsm_set_shift_place', 'tsm_set_consensus', 'tsm_set_non_local', 'tsm_set_temporal_pool', 'tsm_set_convnext', 'tsm_set_tdn', 'tsm_set_tensor', 'tsm_finalize',
           'tsm_forward', 'tsm_tune', 'tsm_forward_tap', 'tsm_last_forward_ms', 'tsm_set_layer_timing', 'tsm_layer_times', 'tsm_conv_tiles', 'tsm_temporal_shift', 'tsm_conv_bn_act',
           'tsm_conv_op', 'tsm_maxpool3x3s2', 'tsm_head', 'tsm_head_segments', 'tsm_preprocess', 'tsm_gather_clips', 'tsm_preprocess_clips', 'tsm_scores_to_states', 'tsm_preprocess_image', 'tsm_frame_votes',
           'tsm_preprocess_indexed', 'tsm_preprocess_windows', 'tsm_top1_tally', 'tsm_forward_features', 'tsm_pool_features', 'tsm_cosine_distances', 'tsm_maxpool2x2', 'tsm_nonlocal_attention')

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """dlopen the in-tree library and declare every prototype of include/tsm_hip.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f'{LIB_PATH} is missing: build it with `python -m workoutdetector_amd.build` '
                          '(hipcc --offload-arch=gfx950). There is no CPU fallback.')
    # PyTorch-ROCm wheels bundle their own libamdhip64 (same SONAME as /opt/rocm's).  Two HIP runtimes
    # in one process cannot both own the device, so make sure torch's copy is the one already mapped
    # when libtsm_hip.so's DT_NEEDED is resolved: import torch first (it is the plumbing for device
    # memory and streams anyway).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    vp, fp, i32, i64 = C.c_void_p, C.c_void_p, C.c_int32, C.c_int64  # float* travel as raw addresses
    lib.tsm_abi_version.restype = C.c_int
    lib.tsm_abi_version.argtypes = []
    lib.tsm_build_id.restype = C.c_char_p
    lib.tsm_build_id.argtypes = []
    lib.tsm_trace_launches.restype = C.c_int
    lib.tsm_trace_launches.argtypes = [i32]
    lib.tsm_launch_trace.restype = i64
    lib.tsm_launch_trace.argtypes = [C.c_char_p, i64]
    lib.tsm_create.restype = C.c_int
    lib.tsm_create.argtypes = [C.POINTER(TsmConfig), C.POINTER(vp)]
    lib.tsm_destroy.restype = None
    lib.tsm_destroy.argtypes = [vp]
    lib.tsm_last_error.restype = C.c_char_p
    lib.tsm_last_error.argtypes = [vp]
    lib.tsm_set_backbone.restype = C.c_int
    lib.tsm_set_backbone.argtypes = [vp, i32]
    lib.tsm_set_bottleneck_width.restype = C.c_int
    lib.tsm_set_bottleneck_width.argtypes = [vp, i32]
    lib.tsm_set_shift_place.restype = C.c_int
    lib.tsm_set_shift_place.argtypes = [vp, i32]
    lib.tsm_set_consensus.restype = C.c_int
    lib.tsm_set_consensus.argtypes = [vp, i32]
    lib.tsm_set_non_local.restype = C.c_int
    lib.tsm_set_non_local.argtypes = [vp, i32]
    lib.tsm_set_temporal_pool.restype = C.c_int
    lib.tsm_set_temporal_pool.argtypes = [vp, i32]
    lib.tsm_set_convnext.restype = C.c_int
    lib.tsm_set_convnext.argtypes = [vp, C.POINTER(i32)]
    lib.tsm_set_tdn.restype = C.c_int
    lib.tsm_set_tdn.argtypes = [vp, C.POINTER(i32), C.c_float, C.c_float]
    lib.tsm_set_tensor.restype = C.c_int
    lib.tsm_set_tensor.argtypes = [vp, C.c_char_p, fp, C.POINTER(i64), i32]
    lib.tsm_finalize.restype = C.c_int
    lib.tsm_finalize.argtypes = [vp]
    lib.tsm_forward.restype = C.c_int
    lib.tsm_forward.argtypes = [vp, vp, i32, i32, i32, fp, vp]
    lib.tsm_forward_tap.restype = C.c_int
    lib.tsm_forward_tap.argtypes = [vp, vp, i32, i32, i32, C.c_char_p, fp, i64, C.POINTER(i64), vp]
    lib.tsm_last_forward_ms.restype = C.c_float
    lib.tsm_last_forward_ms.argtypes = [vp]
    lib.tsm_set_layer_timing.restype = C.c_int
    lib.tsm_set_layer_timing.argtypes = [vp, i32, i32]
    lib.tsm_layer_times.restype = C.c_int
    lib.tsm_layer_times.argtypes = [vp, i32, fp, i32, C.POINTER(i32)]
    lib.tsm_conv_tiles.restype = C.c_int
    lib.tsm_conv_tiles.argtypes = [vp, i32, C.POINTER(i32), i32, C.POINTER(i32)]
    lib.tsm_temporal_shift.restype = C.c_int
    lib.tsm_temporal_shift.argtypes = [fp, fp, i64, i32, i64, i32, i32, vp]
    lib.tsm_conv_bn_act.restype = C.c_int
    lib.tsm_conv_bn_act.argtypes = [fp] * 8 + [i32] * 11 + [vp]
    lib.tsm_conv_op.restype = C.c_int
    lib.tsm_conv_op.argtypes = [C.POINTER(TsmConvArgs), vp]
    lib.tsm_maxpool3x3s2.restype = C.c_int
    lib.tsm_maxpool3x3s2.argtypes = [fp, fp, i32, i32, i32, i32, vp]
    lib.tsm_preprocess.restype = C.c_int
    lib.tsm_preprocess.argtypes = [vp, i32, i32, i32, i32, fp, i32, i32, i32, i32, vp]
    lib.tsm_tune.restype = C.c_int
    lib.tsm_tune.argtypes = [vp, i32, vp]
    lib.tsm_gather_clips.restype = C.c_int
    lib.tsm_gather_clips.argtypes = [vp, i64, i64, i64, i64, i64, i64, i32, i32, i32, i32, vp, vp]
    lib.tsm_preprocess_clips.restype = C.c_int
    lib.tsm_preprocess_clips.argtypes = [vp, i32, i64, i32, i32, i64, i64, i64, i32, i32, i32, i32, vp, fp, i32, i32, i32, vp]
    lib.tsm_head.restype = C.c_int
    lib.tsm_head.argtypes = [fp, fp, fp, fp, i32, i32, i32, i32, i32, vp]
    lib.tsm_head_segments.restype = C.c_int
    lib.tsm_head_segments.argtypes = [fp, fp, fp, fp, i32, i32, i32, i32, vp]
    lib.tsm_scores_to_states.restype = C.c_int
    lib.tsm_scores_to_states.argtypes = [fp, i32, i32, i32, C.c_float, vp, fp, vp]
    lib.tsm_preprocess_image.restype = C.c_int
    lib.tsm_preprocess_image.argtypes = [vp, i32, i32, i32, vp, i64, fp, i32, i32, i32, vp]
    lib.tsm_frame_votes.restype = C.c_int
    lib.tsm_frame_votes.argtypes = [fp, i32, i32, vp, i32, vp, vp, vp, vp]
    lib.tsm_preprocess_indexed.restype = C.c_int
    lib.tsm_preprocess_indexed.argtypes = [vp, i32, i64, i32, i32, vp, i32, i32, fp, i32, i32, i32, i32, vp]
    lib.tsm_preprocess_windows.restype = C.c_int
    lib.tsm_preprocess_windows.argtypes = [vp, i64, i32, vp, i32, i32, i32, fp, i32, i32, i32, i32, vp]
    lib.tsm_top1_tally.restype = C.c_int
    lib.tsm_top1_tally.argtypes = [fp, vp, i32, i32, vp, vp, vp, vp]
    lib.tsm_forward_features.restype = C.c_int
    lib.tsm_forward_features.argtypes = [vp, vp, i32, i32, i32, fp, i32, vp]
    lib.tsm_pool_features.restype = C.c_int
    lib.tsm_pool_features.argtypes = [fp, fp, fp, i32, i32, i32, vp]
    lib.tsm_cosine_distances.restype = C.c_int
    lib.tsm_cosine_distances.argtypes = [fp, i32, i32, i32, i32, fp, vp]
    lib.tsm_maxpool2x2.restype = C.c_int
    lib.tsm_maxpool2x2.argtypes = [fp, i64, i32, i32, fp, i32, i32, i32, vp]
    lib.tsm_nonlocal_attention.restype = C.c_int
    lib.tsm_nonlocal_attention.argtypes = [fp, i64, fp, fp, i64, fp, i64, i32, i32, i32, i32, vp]
    if lib.tsm_abi_version() != ABI_VERSION:
        raise ImportError(f'libtsm_hip.so ABI {lib.tsm_abi_version()} != binding {ABI_VERSION}; rebuild')
    # The library is git-ignored and travels prebuilt: refuse one that was not built from THIS tree (a stale .so would be
    # tested and benchmarked silently).  TSM_LIB_PATH names an A/B build on purpose and is taken as it is.
    have, want = lib.tsm_build_id().decode(), build_id()
    if have != want and not os.environ.get('TSM_LIB_PATH'):
        raise ImportError(f'{LIB_PATH} was built from other sources (build id {have}, this tree is {want}): '
                          'rebuild it with `python -m workoutdetector_amd.build`')
    _lib = lib
    return lib


def check(status: int, engine: Optional[int] = None) -> None:
    if status != 0:
        msg = load().tsm_last_error(engine)
        raise TsmError(status, msg.decode() if msg else '')
