"""Test-time transform in front of the engine: resize(256) -> centre-crop(224) -> normalise.

Counterpart of ``build_test_transform(person_crop=False)`` (workoutdetector/datasets/build.py:131-136)
with torchvision-0.13 *tensor* semantics: ``Resize(int)`` sets the short side to ``size`` and the long
side to ``int(size * long / short)``, bilinear, ``align_corners=False``, no antialias; ``CenterCrop``
starts at ``int(round((dim - crop) / 2))``; ``Normalize`` uses the ImageNet mean/std.

Input-scaling quirk: ``inference_dataset`` feeds float32 frames with
values 0..255 (``torch.cat`` promotion, utils/inference_count.py:412-414) so ``ConvertImageDtype`` is a
no-op and frames are NOT divided by 255.  ``scale_255=False`` (default) reproduces that; ``True`` is the
"fixed" behaviour.

Runs as torch ops on whatever device the frames live on (the engine's GPU in the dataset driver).

``build_test_transform(person_crop=True, boxes=...)`` is the reference's other test transform,
``ConvertImageDtype -> PersonCrop -> Resize((224, 224)) -> Normalize`` (datasets/build.py:123-129,
datasets/transform.py:226-259), from the detector's boxes on: ``PersonCropTransform``.  The Faster-RCNN detector itself is
out of scope; the boxes are the caller's (their own detector, a tracker, annotations).

The IMAGE model's transform is a third one (``data_transform``, utils/inference_count.py:27-34): ``ToPILImage -> Resize(256)
-> CenterCrop(224) -> ToTensor -> Normalize`` -- Pillow's antialiased two-pass resample on uint8, NOT the tensor bilinear
above.  ``pil_resample_tables`` / ``pil_resize_u8`` / ``ImageTransform`` reproduce it to the bit without Pillow;
``image_tables`` packs the tables ``tsm_preprocess_image`` takes; ``image_window_descriptors`` /
``image_window_arena`` build the table and the arena of ``tsm_preprocess_windows`` in image mode (frames of different sizes).
"""
from __future__ import annotations

import functools
import math
from typing import Callable, Mapping, Optional, Sequence, Tuple, Union

import numpy as np
import torch
import torch.nn.functional as F

INPUT_SIZE = 224
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def resized_hw(h: int, w: int, size: int = 256) -> Tuple[int, int]:
    return (size, int(size * w / h)) if h <= w else (int(size * h / w), size)


def crop_offsets(h: int, w: int, crop: int = INPUT_SIZE) -> Tuple[int, int]:
    return int(round((h - crop) / 2.0)), int(round((w - crop) / 2.0))


class TestTransform:
    """Callable on float tensors [T,3,H,W] -> [T,3,crop,crop]."""

    __test__ = False  # not a pytest class

    def __init__(self, size: int = 256, crop: int = INPUT_SIZE, scale_255: bool = False):
        self.size, self.crop, self.scale_255 = size, crop, scale_255

    def __call__(self, frames_tchw: torch.Tensor) -> torch.Tensor:
        x = frames_tchw.to(torch.float32)
        if self.scale_255:
            x = x / 255.0
        nh, nw = resized_hw(x.shape[-2], x.shape[-1], self.size)
        x = F.interpolate(x, size=(nh, nw), mode='bilinear', align_corners=False)
        top, left = crop_offsets(nh, nw, self.crop)
        x = x[..., top:top + self.crop, left:left + self.crop]
        mean = torch.tensor(MEAN, dtype=torch.float32, device=x.device).view(1, 3, 1, 1)
        std = torch.tensor(STD, dtype=torch.float32, device=x.device).view(1, 3, 1, 1)
        return ((x - mean) / std).contiguous()

    def __repr__(self):
        return (f'TestTransform(Resize({self.size}), CenterCrop({self.crop}), Normalize(ImageNet), '
                f'scale_255={self.scale_255})')


Box = Tuple[int, int, int, int]     # (top, left, height, width) in source-frame pixels, as torchvision's crop takes them


def person_box(first_boxes) -> Optional[Box]:
    """The reference's box arithmetic (datasets/transform.py:248-259) for the first detected boxes ``[T, 4]`` =
    ``(x1, y1, x2, y2)`` of one clip's frames: the union over the clip, enlarged by 10 % about its centre, every ``int()``
    truncating toward zero.  Returns ``(top, left, h, w)`` -- it may leave the frame on any side (the crop zero-pads) --
    or None for a zero-area union (the reference's "no person": the frames are used whole).  An enlarged side of 0 raises
    ValueError: the reference would fail inside ``Resize`` there."""
    b = torch.as_tensor(first_boxes, dtype=torch.float32).reshape(-1, 4)
    if b.shape[0] == 0:
        raise ValueError('person_box needs at least one box')
    x1, y1 = b[:, 0].min().item(), b[:, 1].min().item()
    x2, y2 = b[:, 2].max().item(), b[:, 3].max().item()
    w, h = x2 - x1, y2 - y1
    if w * h == 0:
        return None
    left, top = int(x1 - w * 0.05), int(y1 - h * 0.05)
    w, h = int(w * 1.1), int(h * 1.1)
    if w <= 0 or h <= 0:
        raise ValueError(f'person box of {h} x {w} pixels after the 10 % enlargement: nothing to resize')
    return top, left, h, w


class PersonCropTransform:
    """``PersonCrop -> Resize((size, size)) -> Normalize`` from the box on.  ``boxes`` says where the person of a clip is:
    a callable ``(video_name, clip_index) -> (top, left, h, w) or None`` or a mapping ``video_name -> sequence of boxes``
    (one per clip; None = no person).  ``__call__(frames [T,3,H,W], box)`` is the torch implementation, on whatever device
    the frames live on: crop to the box with zero fill where it leaves the frame (torchvision's tensor ``crop``), bilinear
    resize to ``size`` x ``size`` without keeping the aspect ratio (``align_corners=False``, no antialias), normalise.  A box
    of None -- or one with a non-positive side -- is the whole frame.  A ``TsmEngine`` runs the same from staged uint8 frames
    in one launch per batch (``engine.preprocess_clips``)."""

    def __init__(self, boxes: Union[Callable[[str, int], Optional[Box]], Mapping[str, Sequence[Optional[Box]]]],
                 size: int = INPUT_SIZE, scale_255: bool = False):
        if not callable(boxes) and not isinstance(boxes, Mapping):
            raise TypeError('boxes must be a callable (video_name, clip_index) -> box or a mapping video_name -> boxes')
        self.boxes, self.size, self.scale_255 = boxes, size, scale_255

    def box(self, video_name: str, clip_index: int) -> Optional[Box]:
        """The box of one clip, None for "no person"."""
        b = self.boxes(video_name, clip_index) if callable(self.boxes) else self.boxes[video_name][clip_index]
        if b is None:
            return None
        top, left, h, w = (int(v) for v in b)
        return top, left, h, w

    def box_rows(self, video_name: str, lo: int, hi: int) -> torch.Tensor:
        """int32 [hi - lo, 4] rows (top, left, h, w) of clips ``lo .. hi``, "no person" as the all-zero row the kernel reads
        as the whole frame."""
        rows = [self.box(video_name, c) or (0, 0, 0, 0) for c in range(lo, hi)]
        return torch.tensor(rows, dtype=torch.int32).reshape(hi - lo, 4)

    def __call__(self, frames_tchw: torch.Tensor, box: Optional[Box] = None) -> torch.Tensor:
        x = frames_tchw.to(torch.float32)
        if self.scale_255:
            x = x / 255.0
        ih, iw = int(x.shape[-2]), int(x.shape[-1])
        if box is not None and box[2] > 0 and box[3] > 0:
            top, left, h, w = (int(v) for v in box)
            # the part of the box inside the frame, then zeros around it (F.pad: left, right, top, bottom)
            y0, y1 = min(max(top, 0), ih), min(max(top + h, 0), ih)
            x0, x1 = min(max(left, 0), iw), min(max(left + w, 0), iw)
            if y1 <= y0 or x1 <= x0:
                x = x.new_zeros(tuple(x.shape[:-2]) + (h, w))
            else:
                x = F.pad(x[..., y0:y1, x0:x1], (x0 - left, left + w - x1, y0 - top, top + h - y1))
        x = F.interpolate(x, size=(self.size, self.size), mode='bilinear', align_corners=False)
        mean = torch.tensor(MEAN, dtype=torch.float32, device=x.device).view(1, 3, 1, 1)
        std = torch.tensor(STD, dtype=torch.float32, device=x.device).view(1, 3, 1, 1)
        return ((x - mean) / std).contiguous()

    def __repr__(self):
        return (f'PersonCropTransform(PersonCrop(boxes given), Resize(({self.size}, {self.size})), Normalize(ImageNet), '
                f'scale_255={self.scale_255})')


def build_test_transform(person_crop: bool = False, scale_255: bool = False, boxes=None):
    if person_crop:
        if boxes is None:
            raise NotImplementedError('person_crop needs one box per clip: the Faster-RCNN detector is out of scope, the boxes '
                                      'are the caller\'s -- pass boxes=(video_name, clip_index) -> (top, left, h, w) or a mapping '
                                      'video_name -> boxes (transform.person_box turns detections into such a box)')
        return PersonCropTransform(boxes, scale_255=scale_255)
    return TestTransform(scale_255=scale_255)


# ---- NV12 frames: what a hardware decoder leaves, and the exact integer conversion the kernels run in their taps -------------
# One frame [3h/2, w] uint8: h rows of luma, then h/2 rows of interleaved (U, V) pairs; h and w even.  Luma pixel (y, x) takes
# the pair at chroma row y >> 1, columns 2 (x >> 1) and 2 (x >> 1) + 1 (nearest-neighbour chroma, as cv2.COLOR_YUV2RGB_NV12;
# ffmpeg's default swscale path interpolates chroma and is NOT reproduced bit for bit).  With C = Y - y_off, D = U - 128,
# E = V - 128, in int32 with an arithmetic shift:
#   R = clamp((cy C + crv E + 8192) >> 14),  G = clamp((cy C + cgu D + cgv E + 8192) >> 14),  B = clamp((cy C + cbu D + 8192) >> 14)
# name -> (y_off, cy, crv, cgu, cgv, cbu): round(x * 2^14) of the BT.601 / BT.709 matrices, limited range (255/219 for luma,
# 255/224 for chroma) or full range.  The order is that of the pixel codes 16 .. 19 (include/tsm_hip.h).
_NV12_COEFFICIENTS = {
    'bt601': (16, 19077, 26149, -6419, -13320, 33050),
    'bt709': (16, 19077, 29372, -3494, -8731, 34610),
    'bt601-full': (0, 16384, 22970, -5638, -11700, 29032),
    'bt709-full': (0, 16384, 25802, -3069, -7670, 30402),
}
COLORIMETRIES = tuple(_NV12_COEFFICIENTS)
YUV_FORMATS = ('i420', 'yv12', 'p010', 'yuyv', 'uyvy')     # the order of the pixel codes 32 + 4 f + c (include/tsm_hip.h)
FRAME_FORMATS = ('rgb', 'nv12') + YUV_FORMATS
# (Kr, Kb, limited) of each colorimetry: the float64 matrices the integer rows are rounded from
_NV12_MATRIX = {'bt601': (0.299, 0.114, True), 'bt709': (0.2126, 0.0722, True),
                'bt601-full': (0.299, 0.114, False), 'bt709-full': (0.2126, 0.0722, False)}


def nv12_coefficients(colorimetry: str = 'bt601') -> Tuple[int, int, int, int, int, int]:
    """``(y_off, cy, crv, cgu, cgv, cbu)`` of a colorimetry, or ValueError."""
    try:
        return _NV12_COEFFICIENTS[colorimetry]
    except (KeyError, TypeError):
        raise ValueError(f'colorimetry must be one of {COLORIMETRIES}, got {colorimetry!r}') from None


def check_frame_format(frame_format: str, colorimetry: Optional[str]) -> Optional[str]:
    """The colorimetry a call runs with: None for ``'rgb'`` frames (which take none: giving one is a ValueError), for
    ``'nv12'`` and the YUV_FORMATS the given one (default ``'bt601'``), checked.  Touches nothing but its arguments."""
    if frame_format not in FRAME_FORMATS:
        raise ValueError(f'frame_format must be one of {FRAME_FORMATS}, got {frame_format!r}')
    if frame_format == 'rgb':
        if colorimetry is not None:
            raise ValueError(f"colorimetry={colorimetry!r} was given with frame_format='rgb': RGB frames have none")
        return None
    colorimetry = 'bt601' if colorimetry is None else colorimetry
    nv12_coefficients(colorimetry)
    return colorimetry


def nv12_luma_hw(shape) -> Tuple[int, int]:
    """The luma size ``(h, w)`` of NV12 frames whose last two dimensions are ``[3h/2, w]``; ValueError unless the rows are a
    multiple of 3 and h and w are even and positive."""
    rows, w = int(shape[-2]), int(shape[-1])
    if rows <= 0 or w <= 0 or rows % 3 != 0 or w % 2 != 0:       # (h = 2 rows / 3 is then even)
        raise ValueError(f'NV12 frames are [3h/2, w] with h and w even, got {rows} x {w}')
    return rows // 3 * 2, w


# ---- The other YUV formats (YUV_FORMATS), all dense; (h, w) is the luma size and w is even:
#   'i420'  [3h/2, w] bytes: h rows of Y, then the h/2 x w/2 U plane, then the V plane (FFmpeg's yuv420p); h even.
#   'yv12'  'i420' with the V plane before the U plane.
#   'p010'  [3h/2, 2w] bytes: NV12's arrangement in 16-bit little-endian samples, 10 significant bits on top (a 16-bit
#           array [3h/2, w] is taken as its bytes); h even.  A sample converts as its HIGH byte, the low byte is ignored:
#           a P010 frame is the NV12 frame of its high bytes.
#   'yuyv'  [h, 2w] bytes: per pixel pair (Y0, U, Y1, V); the pair shares U and V, rows share nothing; any h >= 1.
#   'uyvy'  [h, 2w] bytes: per pixel pair (U, Y0, V, Y1).
def _is_420(frame_format: str) -> bool:
    return frame_format in ('nv12', 'i420', 'yv12', 'p010')


def yuv_luma_hw(shape, frame_format: str) -> Tuple[int, int]:
    """The luma size ``(h, w)`` of frames of ``'nv12'`` or a YUV_FORMATS name whose last two dimensions are those of the
    format's uint8 container; ValueError when they cannot be: rows no multiple of 3 (4:2:0), an odd w, a side of 0."""
    if frame_format in ('nv12', 'i420', 'yv12'):
        try:
            return nv12_luma_hw(shape)
        except ValueError:
            raise ValueError(f'{frame_format} frames are [3h/2, w] with h and w even, got {int(shape[-2])} x {int(shape[-1])}') from None
    if frame_format not in YUV_FORMATS:
        raise ValueError(f'frame_format must be one of {FRAME_FORMATS[1:]}, got {frame_format!r}')
    rows, cols = int(shape[-2]), int(shape[-1])
    if frame_format == 'p010':
        if rows <= 0 or cols <= 0 or rows % 3 != 0 or cols % 4 != 0:
            raise ValueError(f'p010 frames are [3h/2, 2w] bytes with h and w even, got {rows} x {cols}')
        return rows // 3 * 2, cols // 2
    if rows <= 0 or cols <= 0 or cols % 4 != 0:
        raise ValueError(f'{frame_format} frames are [h, 2w] bytes with w even, got {rows} x {cols}')
    return rows, cols // 2


def frame_container(h: int, w: int, frame_format: str) -> Tuple[int, ...]:
    """The shape of one uint8 frame of luma size h x w as it is staged: ``(h, w, 3)`` for ``'rgb'``, else the two dimensions
    listed above; ValueError for a side of the wrong parity."""
    if frame_format not in FRAME_FORMATS:
        raise ValueError(f'frame_format must be one of {FRAME_FORMATS}, got {frame_format!r}')
    if frame_format == 'rgb':
        return (h, w, 3)
    if h <= 0 or w <= 0 or w % 2 or (_is_420(frame_format) and h % 2):
        raise ValueError(f'{frame_format} needs an even w' + (' and an even h' if _is_420(frame_format) else '') + f', got {h} x {w}')
    return {'p010': (3 * h // 2, 2 * w), 'yuyv': (h, 2 * w), 'uyvy': (h, 2 * w)}.get(frame_format, (3 * h // 2, w))


def frame_hw(shape, frame_format: str = 'rgb') -> Tuple[int, int]:
    """``(h, w)`` of one frame of a video or frame whose shape is ``[..., h, w, 3]`` (``'rgb'``) or ends in the container
    of a YUV format (``[..., 3h/2, w]`` for ``'nv12'``)."""
    return (int(shape[-3]), int(shape[-2])) if frame_format == 'rgb' else yuv_luma_hw(shape, frame_format)


def frame_bytes(h: int, w: int, frame_format: str = 'rgb') -> int:
    """Bytes of one staged uint8 frame of luma size h x w."""
    return {'rgb': 3 * h * w, 'p010': 3 * h * w, 'yuyv': 2 * h * w, 'uyvy': 2 * h * w}.get(frame_format, 3 * h * w // 2)


def yuv_frame_bytes_view(frames, frame_format: str):
    """``frames`` (NumPy array or tensor) as the uint8 container of its format: a 16-bit ``'p010'`` array [..., 3h/2, w] is
    viewed as bytes [..., 3h/2, 2w] (little-endian, as the format is); anything else is returned as it is."""
    if frame_format != 'p010':
        return frames
    if isinstance(frames, torch.Tensor):
        if frames.dtype in (torch.int16, getattr(torch, 'uint16', torch.int16)):
            return frames.contiguous().view(torch.uint8)
    elif isinstance(frames, np.ndarray) and frames.dtype in (np.uint16, np.int16):
        return np.ascontiguousarray(frames).astype('<u2', copy=False).view(np.uint8)
    return frames


def yuv_planes(frames, frame_format: str) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """uint8 frames ``[n, ...container]`` -> the 8-bit samples every pixel converts from: ``(Y, U, V)``, each uint8
    ``[n, h, w]`` (chroma repeated over the pixels that share it).  ``'nv12'`` and the YUV_FORMATS."""
    h, w = yuv_luma_hw(frames.shape, frame_format)
    a = frames.reshape((-1,) + tuple(frames.shape[-2:]))
    n = a.shape[0]
    up = lambda p: p.repeat(2, axis=1).repeat(2, axis=2)
    if frame_format == 'nv12':
        uv = a[:, h:].reshape(n, h // 2, w // 2, 2)
        return a[:, :h], up(uv[..., 0]), up(uv[..., 1])
    if frame_format in ('i420', 'yv12'):
        planes = a[:, h:].reshape(n, 2, h // 2, w // 2)
        first, second = up(planes[:, 0]), up(planes[:, 1])
        return (a[:, :h], first, second) if frame_format == 'i420' else (a[:, :h], second, first)
    if frame_format == 'p010':
        hi = a[:, :, 1::2]                                    # the high byte of every little-endian sample
        uv = hi[:, h:].reshape(n, h // 2, w // 2, 2)
        return hi[:, :h], up(uv[..., 0]), up(uv[..., 1])
    g = a.reshape(n, h, w // 2, 4)
    y0, u, y1, v = (0, 1, 2, 3) if frame_format == 'yuyv' else (1, 0, 3, 2)
    return g[..., [y0, y1]].reshape(n, h, w), g[..., u].repeat(2, axis=2), g[..., v].repeat(2, axis=2)


def yuv_to_rgb(frames, frame_format: str, colorimetry: str = 'bt601') -> np.ndarray:
    """uint8 frames ``[n, ...container]`` (or one frame) of ``'nv12'`` or a YUV_FORMATS name -> uint8 ``[n, h, w, 3]``: the
    NumPy text of the device arithmetic (the int32 formula of ``nv12_to_rgb`` on the samples of ``yuv_planes``) -- to the bit
    what the kernels of that format feed their bilinear taps."""
    y_off, cy, crv, cgu, cgv, cbu = nv12_coefficients(colorimetry)
    if frame_format != 'nv12' and frame_format not in YUV_FORMATS:
        raise ValueError(f'frame_format must be one of {FRAME_FORMATS[1:]}, got {frame_format!r}')
    a = yuv_frame_bytes_view(frames, frame_format)
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    if a.dtype != np.uint8 or a.ndim not in (2, 3):
        raise ValueError(f'{frame_format} frames must be uint8 [n, rows, bytes] or [rows, bytes], got {a.dtype} {a.shape}')
    y, u, v = yuv_planes(a, frame_format)
    c = cy * (y.astype(np.int32) - y_off) + 8192
    d, e = u.astype(np.int32) - 128, v.astype(np.int32) - 128
    rgb = np.stack([(c + crv * e) >> 14, (c + cgu * d + cgv * e) >> 14, (c + cbu * d) >> 14], axis=-1)
    return np.clip(rgb, 0, 255).astype(np.uint8)


def rgb_to_yuv(frames, frame_format: str, colorimetry: str = 'bt601') -> np.ndarray:
    """uint8 ``[n, h, w, 3]`` (or one ``[h, w, 3]``) -> uint8 frames ``[n, ...container]`` of ``'nv12'`` or a YUV_FORMATS
    name: the float64 forward matrix of ``rgb_to_nv12``, chroma the mean of the pixels that share it (a 2x2 block, or a pair
    of one row for the 4:2:2 formats), rounded half up and clipped; ``'p010'`` holds the 8-bit value in the high byte and 0
    in the low one.  For building inputs; it is no codec's exact output."""
    nv12_coefficients(colorimetry)
    if frame_format != 'nv12' and frame_format not in YUV_FORMATS:
        raise ValueError(f'frame_format must be one of {FRAME_FORMATS[1:]}, got {frame_format!r}')
    a = frames.cpu().numpy() if isinstance(frames, torch.Tensor) else np.asarray(frames)
    if a.dtype != np.uint8 or a.ndim not in (3, 4) or a.shape[-1] != 3:
        raise ValueError(f'RGB frames must be uint8 [n, h, w, 3] or [h, w, 3], got {a.dtype} {a.shape}')
    a = a.reshape((-1,) + a.shape[-3:])
    n, h, w = a.shape[:3]
    shape = frame_container(h, w, frame_format)
    if _is_420(frame_format):
        nv = rgb_to_nv12(a, colorimetry)
        if frame_format == 'nv12':
            return nv
        uv = nv[:, h:].reshape(n, h // 2, w // 2, 2)
        out = np.zeros((n,) + shape, dtype=np.uint8)
        if frame_format == 'p010':
            out[:, :, 1::2] = nv
            return out
        out[:, :h] = nv[:, :h]
        u, v = (0, 1) if frame_format == 'i420' else (1, 0)
        out[:, h:].reshape(n, 2, h // 2, w // 2)[:, u] = uv[..., 0]
        out[:, h:].reshape(n, 2, h // 2, w // 2)[:, v] = uv[..., 1]
        return out
    kr, kb, limited = _NV12_MATRIX[colorimetry]
    r, g, b = (a[..., i].astype(np.float64) for i in range(3))
    y = kr * r + (1.0 - kr - kb) * g + kb * b
    cb, cr = (b - y) / (2.0 * (1.0 - kb)), (r - y) / (2.0 * (1.0 - kr))
    ys, yo, cs = (219.0 / 255.0, 16.0, 224.0 / 255.0) if limited else (1.0, 0.0, 1.0)
    quant = lambda p: np.clip(np.floor(p + 0.5), 0, 255).astype(np.uint8)
    pair = lambda p: p.reshape(n, h, w // 2, 2).mean(axis=3)
    out = np.empty((n, h, w // 2, 4), dtype=np.uint8)
    y0, u, y1, v = (0, 1, 2, 3) if frame_format == 'yuyv' else (1, 0, 3, 2)
    yq = quant(y * ys + yo).reshape(n, h, w // 2, 2)
    out[..., y0], out[..., y1] = yq[..., 0], yq[..., 1]
    out[..., u], out[..., v] = quant(pair(cb) * cs + 128.0), quant(pair(cr) * cs + 128.0)
    return out.reshape((n,) + shape)


def black_frame(h: int, w: int, frame_format: str, colorimetry: str = 'bt601') -> np.ndarray:
    """One uint8 frame of a format that converts to RGB (0, 0, 0) everywhere: Y = the colorimetry's offset, chroma 128
    (``'p010'``: those values in the high byte, 0 in the low one); zero bytes for ``'rgb'``.  The staged pad frame: a YUV
    frame of zero bytes is green (``nv12_black``)."""
    shape = frame_container(h, w, frame_format)
    if frame_format == 'rgb':
        return np.zeros(shape, dtype=np.uint8)
    y_off = nv12_coefficients(colorimetry)[0]
    if frame_format == 'nv12':
        return nv12_black(h, w, colorimetry)
    out = np.full(shape, 128, dtype=np.uint8)
    if frame_format in ('i420', 'yv12'):
        out[:h] = y_off
    elif frame_format == 'p010':
        out[:, 0::2] = 0
        out[:h, 1::2] = y_off
    else:
        out[:, (0 if frame_format == 'yuyv' else 1)::2] = y_off
    return out


def nv12_to_rgb(frames, colorimetry: str = 'bt601') -> np.ndarray:
    """uint8 ``[n, 3h/2, w]`` (or one ``[3h/2, w]``) -> uint8 ``[n, h, w, 3]``: the conversion above, in int32 -- to the bit
    what the NV12 kernels feed their bilinear taps."""
    y_off, cy, crv, cgu, cgv, cbu = nv12_coefficients(colorimetry)
    a = frames.cpu().numpy() if isinstance(frames, torch.Tensor) else np.asarray(frames)
    if a.dtype != np.uint8 or a.ndim not in (2, 3):
        raise ValueError(f'NV12 frames must be uint8 [n, 3h/2, w] or [3h/2, w], got {a.dtype} {a.shape}')
    h, w = nv12_luma_hw(a.shape)
    a = a.reshape(-1, 3 * h // 2, w)
    c = cy * (a[:, :h].astype(np.int32) - y_off) + 8192
    uv = a[:, h:].reshape(-1, h // 2, w // 2, 2).astype(np.int32) - 128
    uv = uv.repeat(2, axis=1).repeat(2, axis=2)              # a 2x2 block shares one pair
    d, e = uv[..., 0], uv[..., 1]
    rgb = np.stack([(c + crv * e) >> 14, (c + cgu * d + cgv * e) >> 14, (c + cbu * d) >> 14], axis=-1)
    return np.clip(rgb, 0, 255).astype(np.uint8)


def rgb_to_nv12(frames, colorimetry: str = 'bt601') -> np.ndarray:
    """uint8 ``[n, h, w, 3]`` (or one ``[h, w, 3]``; h, w even) -> uint8 ``[n, 3h/2, w]``: the float64 forward matrix, chroma
    the mean of each 2x2 block, rounded half up and clipped.  A convenience for tests, tools and callers without a decoder;
    it is no codec's exact output."""
    nv12_coefficients(colorimetry)
    kr, kb, limited = _NV12_MATRIX[colorimetry]
    a = frames.cpu().numpy() if isinstance(frames, torch.Tensor) else np.asarray(frames)
    if a.dtype != np.uint8 or a.ndim not in (3, 4) or a.shape[-1] != 3:
        raise ValueError(f'RGB frames must be uint8 [n, h, w, 3] or [h, w, 3], got {a.dtype} {a.shape}')
    a = a.reshape((-1,) + a.shape[-3:])
    n, h, w = a.shape[:3]
    if h <= 0 or w <= 0 or h % 2 or w % 2:
        raise ValueError(f'NV12 needs an even h and an even w, got {h} x {w}')
    r, g, b = (a[..., i].astype(np.float64) for i in range(3))
    y = kr * r + (1.0 - kr - kb) * g + kb * b
    cb, cr = (b - y) / (2.0 * (1.0 - kb)), (r - y) / (2.0 * (1.0 - kr))
    ys, yo, cs = (219.0 / 255.0, 16.0, 224.0 / 255.0) if limited else (1.0, 0.0, 1.0)
    block = lambda p: p.reshape(n, h // 2, 2, w // 2, 2).mean(axis=(2, 4))
    out = np.empty((n, 3 * h // 2, w), dtype=np.uint8)
    quant = lambda v: np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)
    out[:, :h] = quant(y * ys + yo)
    out[:, h:, 0::2] = quant(block(cb) * cs + 128.0)
    out[:, h:, 1::2] = quant(block(cr) * cs + 128.0)
    return out


def nv12_black(h: int, w: int, colorimetry: str = 'bt601') -> np.ndarray:
    """One NV12 frame ``[3h/2, w]`` that converts to RGB (0, 0, 0) everywhere: luma ``y_off``, chroma 128.  (A frame of zero
    bytes does NOT: under ``'bt601'`` it is (0, 136, 0).)"""
    y_off = nv12_coefficients(colorimetry)[0]
    if h <= 0 or w <= 0 or h % 2 or w % 2:
        raise ValueError(f'NV12 needs an even h and an even w, got {h} x {w}')
    out = np.full((3 * h // 2, w), 128, dtype=np.uint8)
    out[:h] = y_off
    return out


def pushed_frame(frame, frame_format: str, colorimetry: Optional[str], to_rgb: bool) -> Tuple[np.ndarray, Tuple[int, int]]:
    """What a stream batcher's ``push`` asks of ONE frame of its ``frame_format``: ``'rgb'`` uint8 [H,W,3]; ``'nv12'`` uint8
    [3H/2,W]; a YUV_FORMATS name that format's uint8 container (a 16-bit ``'p010'`` frame is taken as its bytes); ValueError
    otherwise.  Returns the array to queue -- with ``to_rgb`` (the host path converts on arrival) ``nv12_to_rgb`` /
    ``yuv_to_rgb`` of it -- and its luma ``(h, w)``."""
    arr = np.asarray(frame)
    if frame_format == 'rgb':
        if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] != 3:
            raise ValueError(f'frame must be uint8 [H,W,3], got {arr.dtype} {arr.shape}')
        return arr, (int(arr.shape[0]), int(arr.shape[1]))
    if frame_format == 'nv12':
        if arr.dtype != np.uint8 or arr.ndim != 2:
            raise ValueError(f'an NV12 frame must be uint8 [3H/2,W], got {arr.dtype} {arr.shape}')
        hw = nv12_luma_hw(arr.shape)
    else:
        arr = yuv_frame_bytes_view(arr, frame_format)
        if arr.dtype != np.uint8 or arr.ndim != 2:
            raise ValueError(f'a {frame_format} frame must be its uint8 container [rows, bytes], got {arr.dtype} {arr.shape}')
        hw = yuv_luma_hw(arr.shape, frame_format)
    if to_rgb:
        arr = (nv12_to_rgb(arr, colorimetry) if frame_format == 'nv12' else yuv_to_rgb(arr, frame_format, colorimetry))[0]
    return arr, hw


def window_descriptors(shapes, offsets, boxes=None, resize: int = 256, crop: int = INPUT_SIZE,
                       frame_format: str = 'rgb') -> np.ndarray:
    """The descriptor table ``tsm_preprocess_windows`` takes (include/tsm_hip.h), built and VALIDATED on the host: int32
    [n, 8], row c = ``(off_lo, off_hi, h, w, top, left, bh, bw)``.  ``shapes``: one frame size ``(h, w)`` (or ``(h, w, 3)``)
    per window; ``offsets``: the byte offset of each window's first frame in the arena.  ``boxes=None`` builds a centre-crop
    table (the box words are 0; ``resize`` / ``crop`` are those of the launch); otherwise one box ``(top, left, h, w)`` or
    None ("no person": the all-zero box the kernel reads as the whole frame) per window.

    The kernel is total in this table and turns an invalid row into zero frames; a caller who builds the table here gets an
    error instead: ValueError for a side outside 1 .. 65535, an offset that is negative or no multiple of 16, a centre crop
    larger than the resized frame, a box that is not four integers of the int32 range.  ``frame_format='nv12'`` or a
    YUV_FORMATS name: the windows hold frames of that format, ``shapes`` are their luma sizes ``(h, w)``, and a side of the
    wrong parity (an odd w; an odd h except for ``'yuyv'`` / ``'uyvy'``) is a ValueError too."""
    if frame_format not in FRAME_FORMATS:
        raise ValueError(f'frame_format must be one of {FRAME_FORMATS}, got {frame_format!r}')
    shapes, offsets = list(shapes), list(offsets)
    if len(shapes) != len(offsets) or (boxes is not None and len(boxes) != len(shapes)):
        raise ValueError('shapes, offsets and boxes must have one entry per window')
    desc = np.zeros((len(shapes), 8), dtype=np.int32)
    for c, (shape, off) in enumerate(zip(shapes, offsets)):
        shape = tuple(shape)
        if len(shape) not in (2, 3) or (len(shape) == 3 and shape[2] != 3) or not all(isinstance(d, (int, np.integer)) for d in shape):
            raise ValueError(f'window {c}: shape must be (h, w) or (h, w, 3), got {shape}')
        h, w = int(shape[0]), int(shape[1])
        if not (1 <= h <= 65535 and 1 <= w <= 65535):
            raise ValueError(f'window {c}: frame sides must lie in 1 .. 65535, got {h} x {w}')
        if frame_format == 'nv12' and (len(shape) != 2 or h % 2 or w % 2):
            raise ValueError(f'window {c}: an NV12 window is (h, w) with both sides even, got {shape}')
        if frame_format in YUV_FORMATS and (len(shape) != 2 or w % 2 or (_is_420(frame_format) and h % 2)):
            raise ValueError(f'window {c}: a {frame_format} window is (h, w) with an even w' +
                             (' and an even h' if _is_420(frame_format) else '') + f', got {shape}')
        if not isinstance(off, (int, np.integer)) or off < 0 or off % 16 != 0 or off >= 1 << 63:
            raise ValueError(f'window {c}: offset must be a non-negative multiple of 16 bytes, got {off!r}')
        off = int(off)
        desc[c, :4] = ((off & 0xFFFFFFFF) - ((off & 0x80000000) << 1), off >> 32, h, w)
        if boxes is None:
            nh, nw = resized_hw(h, w, resize)
            if crop > nh or crop > nw:
                raise ValueError(f'window {c}: crop {crop} larger than the resized frame {nh} x {nw}')
        elif boxes[c] is not None:
            box = tuple(boxes[c])
            if len(box) != 4 or not all(isinstance(v, (int, np.integer)) and -2 ** 31 <= v < 2 ** 31 for v in box):
                raise ValueError(f'window {c}: box must be four int32 (top, left, h, w) or None, got {boxes[c]!r}')
            desc[c, 4:] = [int(v) for v in box]
    return desc


# ---- the image model's transform: Pillow's 8-bit bilinear resample, to the bit ------------------------------------------
PRECISION_BITS = 32 - 8 - 2         # Pillow's fixed point: weights are scaled by 2^22


def pil_ksize(in_size: int, out_size: int) -> int:
    """Taps per row of the coefficient table: ``int(ceil(support)) * 2 + 1`` with support = max(in / out, 1)."""
    return int(math.ceil(max(in_size / out_size, 1.0))) * 2 + 1


def _pil_rows(in_size: int, out_size: int, first: int, count: int) -> Tuple[np.ndarray, np.ndarray]:
    """Rows ``first .. first + count - 1`` of Pillow's coefficient tables of one axis (below), all at once: every step is the
    scalar loop's IEEE double operation on a column of rows -- the weights are added tap by tap, in order (Pillow adds them
    so, in double; a tap behind a row's last adds 0.0) -- so the integers are those of the loop, whatever the rows asked for."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = (np.arange(first, first + count, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(0, (center - support + 0.5).astype(np.int64))                    # (int(): towards zero, as astype)
    xmax = np.minimum(in_size, (center + support + 0.5).astype(np.int64)) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    w = np.maximum(0.0, 1.0 - np.abs(((x + xmin[:, None]) - center[:, None] + 0.5) * ss))
    w[x >= xmax[:, None]] = 0.0
    ww = np.zeros(count, dtype=np.float64)
    for t in range(ksize):
        ww += w[:, t]
    w = np.where((ww != 0.0)[:, None], w / np.where(ww != 0.0, ww, 1.0)[:, None], w)
    kk = (w * float(1 << PRECISION_BITS) + np.where(w < 0.0, -0.5, 0.5)).astype(np.int64).astype(np.int32)
    return np.stack([xmin, xmax], axis=1).astype(np.int32), kk


@functools.lru_cache(maxsize=64)
def pil_resample_tables(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """Pillow's coefficient tables of one axis for the bilinear (triangle) filter on 8-bit channels (Resample.c:
    ``precompute_coeffs`` + ``normalize_coeffs_8bpc``), computed in double: ``bounds`` int32 [out, 2] = (first source index,
    taps) and ``kk`` int32 [out, ksize] = the weights, normalised to sum 1, times 2^22, rounded half away from zero, zero
    behind a row's taps.  The returned arrays are cached and read-only."""
    if in_size <= 0 or out_size <= 0:
        raise ValueError(f'sizes must be positive, got {in_size} -> {out_size}')
    bounds, kk = _pil_rows(in_size, out_size, 0, out_size)
    bounds.setflags(write=False)
    kk.setflags(write=False)
    return bounds, kk


def _pil_pass(img: np.ndarray, in_size: int, out_size: int) -> np.ndarray:
    """One pass along axis 0 of uint8 [in, ...]: u8 = clamp((2^21 + sum(pixel * k)) >> 22, 0, 255)."""
    bounds, kk = pil_resample_tables(in_size, out_size)
    out = np.empty((out_size,) + img.shape[1:], dtype=np.uint8)
    src = img.astype(np.int64)
    for i in range(out_size):
        xmin, n = int(bounds[i, 0]), int(bounds[i, 1])
        acc = np.tensordot(kk[i, :n].astype(np.int64), src[xmin:xmin + n], axes=1) + (1 << (PRECISION_BITS - 1))
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def pil_resize_u8(frame_hwc_u8: np.ndarray, resize: int = 256) -> np.ndarray:
    """``Resize(resize)`` of torchvision on a PIL image = ``Image.resize((nw, nh), BILINEAR)`` of Pillow, in NumPy: uint8
    [H, W, C] -> uint8 [nh, nw, C] with the shorter side ``resize`` and the longer ``int(resize * long / short)``; the
    horizontal pass first, rounded to uint8, then the vertical one; a pass whose axis keeps its size is skipped."""
    img = np.asarray(frame_hwc_u8)
    if img.dtype != np.uint8 or img.ndim != 3:
        raise ValueError(f'frame must be uint8 [H, W, C], got {img.dtype} {img.shape}')
    h, w = img.shape[:2]
    nh, nw = resized_hw(h, w, resize)
    if nw != w:
        img = _pil_pass(img.transpose(1, 0, 2), w, nw).transpose(1, 0, 2)
    if nh != h:
        img = _pil_pass(img, h, nh)
    return np.ascontiguousarray(img)


@functools.lru_cache(maxsize=64)
def image_tables(h: int, w: int, resize: int = 256, crop: int = INPUT_SIZE) -> np.ndarray:
    """The table block ``tsm_preprocess_image`` takes for h x w frames (include/tsm_hip.h): int32, rows of the crop window's
    output indices only -- [hb crop x 2][hk crop x ksx] when the width changes, then [vb crop x 2][vk crop x ksy] when the
    height does; empty when neither does.  A few KB per geometry, cached; the engine uploads it once per device."""
    nh, nw = resized_hw(h, w, resize)
    if crop > nh or crop > nw:
        raise ValueError(f'crop {crop} larger than the resized frame {nh} x {nw}')
    top, left = crop_offsets(nh, nw, crop)
    parts = []
    for size, new, first in ((w, nw, left), (h, nh, top)):
        if new != size:
            bounds, kk = _pil_rows(size, new, first, crop)         # (the window's rows only: a long side can run to 65535 x resize)
            parts += [bounds.reshape(-1), kk.reshape(-1)]
    block = np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, dtype=np.int32)
    block.setflags(write=False)
    return block


IMAGE_WINDOW_FORMATS = ('rgb', 'nv12')      # what tsm_preprocess_windows takes in image mode: Pillow's path is 8-bit


def image_window_descriptors(shapes, offsets, table_offsets, resize: int = 256, crop: int = INPUT_SIZE,
                             frame_format: str = 'rgb') -> np.ndarray:
    """The descriptor table ``tsm_preprocess_windows`` takes in image mode (``_lib.WINDOWS_IMAGE``; include/tsm_hip.h), built
    and VALIDATED on the host: int32 [n, 8], row c = ``(off_lo, off_hi, h, w, tab_lo, tab_hi, 0, 0)``.  ``shapes`` / ``offsets``
    as ``window_descriptors`` takes them, with its refusals (a side outside 1 .. 65535, an odd NV12 side, an offset that is
    negative or no multiple of 16, a crop larger than the resized frame); ``table_offsets``: per window the byte offset in the
    arena of ``image_tables(h, w, resize, crop)``, under the same rule as an offset.  Windows of one geometry may name one
    block; a geometry whose block is empty (neither axis changes) may name anything valid, 0 for instance."""
    if frame_format not in IMAGE_WINDOW_FORMATS:
        raise ValueError(f'frame_format must be one of {IMAGE_WINDOW_FORMATS} in image mode, got {frame_format!r}')
    table_offsets = list(table_offsets)
    desc = window_descriptors(shapes, offsets, None, resize=resize, crop=crop, frame_format=frame_format)
    if len(table_offsets) != desc.shape[0]:
        raise ValueError('shapes, offsets and table_offsets must have one entry per window')
    for c, tab in enumerate(table_offsets):
        if not isinstance(tab, (int, np.integer)) or tab < 0 or tab % 16 != 0 or tab >= 1 << 63:
            raise ValueError(f'window {c}: table offset must be a non-negative multiple of 16 bytes, got {tab!r}')
        tab = int(tab)
        desc[c, 4:6] = ((tab & 0xFFFFFFFF) - ((tab & 0x80000000) << 1), tab >> 32)
    return desc


def image_window_arena(shapes, n_segment: int = 1, resize: int = 256, crop: int = INPUT_SIZE, frame_format: str = 'rgb'):
    """The layout of one step's arena in image mode: the windows' frames in order (window c = ``n_segment`` contiguous frames
    of ``shapes[c]``), then one table block per DISTINCT geometry (the cached ``image_tables``), each start 16-byte aligned.
    Returns ``(desc, offsets, tables, nbytes)``: the descriptors (``image_window_descriptors``), the byte offset of every
    window, ``[(byte offset, int32 block), ...]`` to copy in, and the arena's size, a multiple of 16."""
    shapes = [tuple(int(d) for d in s[:2]) for s in shapes]
    offsets, total = [], 0
    for h, w in shapes:
        offsets.append(total)
        total += (n_segment * frame_bytes(h, w, frame_format) + 15) // 16 * 16
    where, tables = {}, []
    for h, w in shapes:
        if (h, w) not in where:
            block = image_tables(h, w, resize, crop)
            where[(h, w)] = total
            if block.size:
                tables.append((total, block))
                total += (block.nbytes + 15) // 16 * 16
    desc = image_window_descriptors(shapes, offsets, [where[s] for s in shapes], resize, crop, frame_format)
    return desc, offsets, tables, max(total, 16)


class ImageTransform:
    """``data_transform`` of the image model (utils/inference_count.py:27-34) on the CPU, for models that are not engines:
    uint8 frames [n, H, W, 3] (or one [H, W, 3]; ndarray or tensor) -> float32 tensor [n, 3, crop, crop] = ``ToPILImage ->
    Resize(resize) -> CenterCrop(crop) -> ToTensor -> Normalize(ImageNet)``, built on ``pil_resize_u8``: no Pillow at run
    time.  The channel order is kept as given: the reference feeds cv2's BGR frames straight into ToPILImage, so whatever
    order the model was trained on is the caller's business.  A ``TsmEngine`` runs the same in one launch per batch
    (``engine.preprocess_image``)."""

    def __init__(self, resize: int = 256, crop: int = INPUT_SIZE):
        self.resize, self.crop = int(resize), int(crop)

    def crop_u8(self, frame_hwc_u8: np.ndarray) -> np.ndarray:
        """uint8 [crop, crop, C]: the resized frame's centre window."""
        img = pil_resize_u8(frame_hwc_u8, self.resize)
        if self.crop > img.shape[0] or self.crop > img.shape[1]:
            raise ValueError(f'crop {self.crop} larger than the resized frame {img.shape[0]} x {img.shape[1]}')
        top, left = crop_offsets(img.shape[0], img.shape[1], self.crop)
        return img[top:top + self.crop, left:left + self.crop]

    def __call__(self, frames_u8) -> torch.Tensor:
        a = frames_u8.cpu().numpy() if isinstance(frames_u8, torch.Tensor) else np.asarray(frames_u8)
        if a.ndim == 3:
            a = a[None]
        u8 = np.stack([self.crop_u8(f) for f in a])
        x = u8.astype(np.float32) / np.float32(255.0)
        x = (x - np.float32(MEAN)) / np.float32(STD)
        return torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2)))

    def __repr__(self):
        return f'ImageTransform(ToPILImage, Resize({self.resize}), CenterCrop({self.crop}), ToTensor, Normalize(ImageNet))'


# ---- the per-frame engine paths (image model, frame embeddings): what both ask of their input and of their engine -----------
def as_frames_u8(frames) -> torch.Tensor:
    """Decoded frames (ndarray or tensor) as a uint8 tensor [n >= 1, H, W, 3], or ValueError."""
    t = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frames))
    if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3 or t.shape[0] == 0:
        raise ValueError(f'frames must be uint8 [n >= 1, H, W, 3], got {t.dtype} {tuple(t.shape)}')
    return t


def need_frame_engine(model, crop: int, path: str, factory: str) -> None:
    """A per-frame path feeds every frame as a clip of one segment, cropped to the engine's own size: refuse any other
    engine up front (``path`` / ``factory``: how the caller's message names itself and the constructor to use)."""
    if getattr(model, 'num_segments', 1) != 1:
        raise ValueError(f'the {path} path needs an engine with num_segments=1 (engine.{factory})')
    if (model.height, model.width) != (crop, crop):
        raise ValueError(f'the engine takes {model.height} x {model.width} frames, the transform crops to {crop}')
