"""The person-crop test transform written out independently of the product, for the CPU and the GPU tests:

    ConvertImageDtype -> PersonCrop (from the box on) -> Resize((size, size)) -> Normalize

as torchvision's tensor ops compose it: ``crop`` zero-pads the image where the box leaves it (``F.pad``) and slices, ``resize``
is ``F.interpolate(mode='bilinear', align_corners=False)`` without antialias, ``Normalize`` comes last -- so a padded pixel
becomes (0 - mean) / std.  Everything runs on the CPU.  ``clip_reference`` is computed once per (video, boxes, size, scale)
and shared between the tests that need it; callers must not write into what it returns.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

MEAN = torch.tensor([0.485, 0.456, 0.406], dtype=torch.float32).view(1, 3, 1, 1)
STD = torch.tensor([0.229, 0.224, 0.225], dtype=torch.float32).view(1, 3, 1, 1)
ZERO = ((0.0 - MEAN) / STD).view(3)          # what a zero pixel becomes, per channel


def reference(frames_tchw, box, size, scale_255=False):
    """frames [T,3,H,W] (values 0..255), box (top, left, h, w) or None -> [T,3,size,size]."""
    x = frames_tchw.to(torch.float32)
    if scale_255:
        x = x / 255.0
    if box is not None and box[2] > 0 and box[3] > 0:
        top, left, h, w = (int(v) for v in box)
        ih, iw = x.shape[-2:]
        pt, pl = max(0, -top), max(0, -left)
        pb, pr = max(0, top + h - ih), max(0, left + w - iw)
        x = F.pad(x, (pl, pr, pt, pb))[..., top + pt: top + pt + h, left + pl: left + pl + w]
    x = F.interpolate(x, size=(size, size), mode='bilinear', align_corners=False)
    return (x - MEAN) / STD


def video(seed, total, h, w):
    """uint8 [total, h, w, 3] noise: every pixel differs from its neighbours, so a tap one pixel off shows."""
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, size=(total, h, w, 3), dtype=np.uint8))


def window(vid_thwc, clip):
    """The reference loop's window: vid[8 * clip: 8 * clip + 16: 2], zero-padded to 8 frames, float32 [8,3,H,W]."""
    w = vid_thwc[8 * clip: 8 * clip + 16: 2].to(torch.float32)
    if w.shape[0] < 8:
        w = torch.cat([w, torch.zeros((8 - w.shape[0],) + tuple(w.shape[1:]))])
    return w.permute(0, 3, 1, 2)


@functools.lru_cache(maxsize=None)
def clip_reference(seed, total, h, w, boxes, size, scale_255):
    """[n_clips, 8, 3, size, size]: clip c of ``video(seed, total, h, w)`` under ``boxes[c]`` (a tuple of boxes / None)."""
    vid = video(seed, total, h, w)
    return torch.stack([reference(window(vid, c), boxes[c], size, scale_255) for c in range(len(boxes))])


def boxes_for(h, w, size):
    """The box kinds a crop kernel can get wrong, for an h x w frame resized to `size`: interior, overhang top-left (negative
    top / left), overhang bottom-right, 1 x 1, wider than the frame, entirely outside, bh = 0 (whole frame), one up-scaling
    (bh < size) and one down-scaling box.  The frames here are larger than `size` in one direction at least."""
    return (
        (5, 7, 20, 17),                     # interior (and up-scaling for size 32 / 33: 20 < size)
        (-6, -9, 25, 30),                   # overhangs the top and the left edge
        (h - 12, w - 10, 30, 27),           # overhangs the bottom and the right edge
        (h // 2, w // 3, 1, 1),             # one pixel
        (3, -4, h - 5, w + 11),             # wider than the frame: overhangs left and right at once
        (h + 5, 2, 9, 9),                   # entirely outside, below
        (4, 4, 0, 13),                      # bh = 0: "no person", the whole frame
        (2, 1, 6, 5),                       # up-scaling in both directions
        (0, 0, h, w) if h > size or w > size else (-20, -20, h + 40, w + 40),   # down-scaling
        (-7, 3, 2 * size + 9, 3 * size + 1),            # down-scaling, past the bottom / right edge
        (-3, -w - 4, 11, w),                # entirely outside, to the left (touches column -5 .. -w-4)
        None,                               # no person
    )
