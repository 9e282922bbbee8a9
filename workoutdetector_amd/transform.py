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
"""
from __future__ import annotations

from typing import Callable, Mapping, Optional, Sequence, Tuple, Union

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
