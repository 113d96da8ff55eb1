#!/usr/bin/env python3
"""Generate tests/golden/resample/resample_wide.npz: Pillow's own bytes for crop boxes beyond 2.5 times the size they are resized to --
the cases of the wide-tap resample kernels (csrc/resample_wide.h, csrc/resample_wide.hip).

Build container only (needs PIL; the arrays it writes are data and are what travels).  Nothing of the reference runs here: the pipelines
are torchvision's ``Resize`` / ``CenterCrop`` rules restated in tests/resample_refs.py (``eval_geometry``) and Pillow's ``Image.resize``;
``make_golden`` is imported for the recipes' common path set-up only.

Four cases, each a source, the row of csrc/resample.h (src_h, src_w, top, left, box_h, box_w, full_h, full_w, off_y, off_x, flags) and
Pillow's output ``img.crop(box).resize((full_w, full_h), BICUBIC).crop(window)`` (+ ``transpose(FLIP_LEFT_RIGHT)``):

    ``wide``    40 x 1500 -> 224 x 224, mirrored: scale 6.7 across (28 taps), an upscale down
    ``tall``    1500 x 40 -> 224 x 224: scale 6.7 down, an upscale across
    ``eval``    600 x 640, Resize(224) + CenterCrop(224): full 224 x 238, offsets 0, 7 (scales 2.68 and 2.69: just beyond the 11 taps)
    ``noaug``   375 x 1242 (a KITTI frame's shape), Resize((224, 224)): scales 1.67 down and 5.54 across
    a box with odd edges (top 3, left 5, 33 x 1201) inside the ``wide`` source comes fifth, as ``box``: its taps clamp at the box's edges

The sources are not stored (the two large ones alone would exceed 1 MB): they are ``resample_wide_refs.pattern(h, w)``, integer
arithmetic on the pixel coordinates -- gradients, saturated 0 / 255 checkerboards of periods 1 to 3 (the overshoot clamps at both ends)
and a band of hashed noise.  Keys: ``<case>_size`` (h, w of the pattern), ``<case>_row`` [11], ``<case>_out`` [224, 224, 3];
``pillow_version``.

tests/test_resample_wide_host.py pins tests/resample_wide_refs.py to the bytes, tests/test_gpu_u8_resample_wide.py the kernels.
Usage:  python tests/golden/make_golden_resample_wide.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402,F401  (as every recipe: the reference's root in front of sys.path, the third-party stand-ins)

sys.path.insert(1, os.path.dirname(HERE))
import resample_refs as R  # noqa: E402
import resample_wide_refs as W  # noqa: E402


def main():
    import PIL
    out = {"pillow_version": np.array(PIL.__version__)}
    wide, tall, ev, noaug = W.pattern(40, 1500), W.pattern(1500, 40), W.pattern(600, 640), W.pattern(375, 1242)
    fh, fw, oy, ox = R.eval_geometry(600, 640, resize=224)
    assert (fh, fw, oy, ox) == (224, 238, 0, 7)
    cases = {
        "wide": (wide, (40, 1500, 0, 0, 40, 1500, 224, 224, 0, 0, 1)),
        "tall": (tall, (1500, 40, 0, 0, 1500, 40, 224, 224, 0, 0, 0)),
        "eval": (ev, (600, 640, 0, 0, 600, 640, fh, fw, oy, ox, 0)),
        "noaug": (noaug, (375, 1242, 0, 0, 375, 1242, 224, 224, 0, 0, 0)),
        "box": (wide, (40, 1500, 3, 5, 33, 1201, 224, 224, 0, 0, 0)),
    }
    for name, (img, row) in cases.items():
        got = R.pillow_row(img, row).copy()
        out[name + "_size"] = np.array(img.shape[:2], dtype=np.int32)
        out[name + "_row"], out[name + "_out"] = np.array(row, dtype=np.int32), got
        assert 2 * row[4] > 5 * row[6] or 2 * row[5] > 5 * row[7]          # beyond the 11-tap kernels on an axis
        assert name == "box" or (got.min() == 0 and got.max() == 255), name   # whole sources reach both clamps
        print("%s: row %s, %d distinct bytes" % (name, row, len(np.unique(got))))
    os.makedirs(os.path.join(HERE, "resample"), exist_ok=True)
    path = os.path.join(HERE, "resample", "resample_wide.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 900 * 1024, size
    print("wrote %s (%d bytes)" % (path, size))


if __name__ == "__main__":
    main()
