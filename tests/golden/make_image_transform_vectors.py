"""Writes tests/golden/ref_image_transform.npz: what Pillow gives for the image model's Resize + CenterCrop.

    python tests/golden/make_image_transform_vectors.py

For every case: ``<name>_frames`` uint8 [3, H, W, 3] (seeded noise, or three constant frames), ``<name>_want`` uint8
[3, crop, crop, 3] = ``Image.fromarray(frame).resize((nw, nh), Image.BILINEAR)`` cropped as torchvision's ``center_crop``
crops, and ``<name>_geom`` = (resize, crop).  Sizes as torchvision's ``Resize(int)`` on a PIL image: the shorter side becomes
``resize``, the longer ``int(resize * long / short)``.  Needs Pillow (the vectors in the repository came from 12.2.0); the
tests that read the file do not.
"""
import os

import numpy as np
from PIL import Image

# name: (H, W, resize, crop)
CASES = {
    'landscape': (37, 53, 24, 16),        # downscale, support > 1
    'portrait': (53, 37, 24, 16),
    'upscale': (20, 30, 32, 32),          # support 1
    'vskip': (24, 41, 24, 16),            # the height keeps its size: no vertical pass
    'tall': (90, 31, 16, 15),             # ~5.6x downscale, odd crop, odd crop offset
    'constant': (11, 17, 8, 6),           # constant frames: do a row's integer weights sum to exactly 2^22?
}
CONSTANTS = (255, 1, 128)


def resized_hw(h, w, size):
    return (size, int(size * w / h)) if h <= w else (int(size * h / w), size)


def main():
    out = {}
    for i, (name, (h, w, resize, crop)) in enumerate(CASES.items()):
        if name == 'constant':
            frames = np.stack([np.full((h, w, 3), v, dtype=np.uint8) for v in CONSTANTS])
        else:
            frames = np.random.default_rng(100 + i).integers(0, 256, size=(3, h, w, 3), dtype=np.uint8)
        nh, nw = resized_hw(h, w, resize)
        top, left = int(round((nh - crop) / 2.0)), int(round((nw - crop) / 2.0))
        want = []
        for f in frames:
            img = Image.fromarray(f)
            if (nh, nw) != (h, w):
                img = img.resize((nw, nh), Image.BILINEAR)
            want.append(np.asarray(img)[top:top + crop, left:left + crop])
        out[name + '_frames'] = frames
        out[name + '_want'] = np.stack(want).astype(np.uint8)
        out[name + '_geom'] = np.int32([resize, crop])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'ref_image_transform.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
