#!/usr/bin/env python3
"""Generate tests/golden/resample/resample.npz: the boxes the reference's RandomResizedCrop draws, and Pillow's bytes for a few rows.

Build container only (reads /root/reference and needs PIL; the arrays it writes are data and are what travels).  The reference's
util/crop.py is loaded BY FILE PATH.  It subclasses ``torchvision.transforms.RandomResizedCrop`` and torchvision is not installed here, so
the module is loaded with a stand-in ``torchvision`` of two empty classes; ``get_params`` itself -- a static method that touches torch and
PIL only -- is the reference's own code.

(a) Draws.  For each of two seeds ``torch.manual_seed(seed)``, then for 16 images of mixed sizes, in loader order:
    ``get_params(img, (0.08, 1.0), (3/4, 4/3))`` -> (i, j, h, w), then ``torch.rand(1) < 0.5`` -- the call RandomHorizontalFlip.forward
    makes.  torchvision is absent, so that ONE line is restated here, not executed from torchvision.  After the 16 images one more
    ``torch.rand(1)`` is recorded: it pins the number of draws consumed.
    ``draw<seed>_sizes`` [16, 2] (h, w), ``draw<seed>_boxes`` [16, 4], ``draw<seed>_flips`` [16], ``draw<seed>_next`` (fp32).
(b) Pixels.  Six small sources (at most 64 x 64, stored padded to 64 x 64 with 0xFF) with one row each -- a 1 x 1 box, an upsampled
    8 x 10 box, a whole image, a box flush with a corner, a mirrored row, a saturated 0 / 255 checkerboard -- and one 300 x 400 evaluation
    case (Resize(256) + CenterCrop(224): full 256 x 341, offsets 16, 58).  Per case the source bytes, the row of csrc/resample.h
    (src_h, src_w, top, left, box_h, box_w, full_h, full_w, off_y, off_x, flags) and Pillow's output
    ``img.crop(box).resize((full_w, full_h), BICUBIC).crop(window)`` (+ ``transpose(FLIP_LEFT_RIGHT)``): ``small_src`` [6, 64, 64, 3],
    ``small_rows`` [6, 11], ``small_out`` [6, 224, 224, 3], ``eval_src`` [300, 400, 3], ``eval_row`` [11], ``eval_out`` [224, 224, 3],
    ``eval_sizes`` (the sizes torchvision's rule gives, computed here from its formula) and ``pillow_version``.

tests/test_resample_refs_host.py pins tests/resample_refs.py to the bytes, tests/test_crop_host.py pins util.crop to the draws.
Usage:  python tests/golden/make_golden_resample.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (the reference's root in front of sys.path, the third-party stand-ins)

REF = os.path.join(mg.REF, "util", "crop.py")
SEEDS = (0, 1234)
SIZES = [(256, 256), (500, 375), (375, 500), (512, 512), (64, 48), (224, 224), (333, 500), (480, 360),
         (32, 32), (256, 341), (500, 500), (427, 640 - 128), (96, 128), (300, 400), (512, 384), (233, 311)]   # (h, w)


def load_reference():
    """The reference's util/crop.py with a stand-in for the absent torchvision (its base class and the unused ``functional``)."""
    saved = {k: sys.modules.get(k) for k in ("torchvision", "torchvision.transforms", "torchvision.transforms.functional")}
    tv, tr, fn = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms"), types.ModuleType("torchvision.transforms.functional")
    tr.RandomResizedCrop = type("RandomResizedCrop", (), {})
    tr.functional, tv.transforms = fn, tr
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tr, "torchvision.transforms.functional": fn})
    try:
        spec = importlib.util.spec_from_file_location("reference_util_crop", REF)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


def pillow(img, row):
    from PIL import Image
    sh, sw, top, left, bh, bw, fh, fw, oy, ox, flags = (int(v) for v in row)
    im = Image.fromarray(np.ascontiguousarray(img[:sh, :sw]))
    im = im.crop((left, top, left + bw, top + bh)).resize((fw, fh), Image.BICUBIC).crop((ox, oy, ox + 224, oy + 224))
    if flags & 1:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(im).copy()


def main():
    import PIL
    from PIL import Image
    ref = load_reference()
    out = {"pillow_version": np.array(PIL.__version__)}
    for seed in SEEDS:
        torch.manual_seed(seed)
        boxes, flips = [], []
        for (h, w) in SIZES:
            boxes.append(ref.RandomResizedCrop.get_params(Image.new("RGB", (w, h)), (0.08, 1.0), (3. / 4., 4. / 3.)))
            flips.append(bool(torch.rand(1) < 0.5))   # RandomHorizontalFlip.forward's call, restated (torchvision is absent)
        out["draw%d_sizes" % seed] = np.array(SIZES, dtype=np.int32)
        out["draw%d_boxes" % seed] = np.array(boxes, dtype=np.int32)
        out["draw%d_flips" % seed] = np.array(flips, dtype=np.bool_)
        out["draw%d_next" % seed] = np.float32(torch.rand(1).item())
        assert any(flips) and not all(flips)
        print("seed %d: boxes %s flips %s" % (seed, boxes[:3], flips[:6]))
    rng = np.random.default_rng(5)
    checker = ((np.add.outer(np.arange(64), np.arange(64)) & 1) * 255).astype(np.uint8)[..., None].repeat(3, axis=2)
    smooth = (np.add.outer(np.arange(64) * 3, np.arange(64) * 2)[..., None] + np.array([0, 40, 90])).astype(np.uint8)
    cases = [   # (source, row)
        (rng.integers(0, 256, (64, 64, 3), dtype=np.uint8), (64, 64, 37, 11, 1, 1, 224, 224, 0, 0, 0)),
        (rng.integers(0, 256, (48, 64, 3), dtype=np.uint8), (48, 64, 20, 30, 8, 10, 224, 224, 0, 0, 0)),
        (smooth, (64, 64, 0, 0, 64, 64, 224, 224, 0, 0, 0)),
        (rng.integers(0, 256, (33, 57, 3), dtype=np.uint8), (33, 57, 33 - 21, 57 - 40, 21, 40, 224, 224, 0, 0, 0)),
        (rng.integers(0, 256, (64, 40, 3), dtype=np.uint8), (64, 40, 3, 5, 50, 31, 224, 224, 0, 0, 1)),
        (checker, (64, 64, 1, 2, 60, 45, 224, 224, 0, 0, 1)),
    ]
    src = np.full((len(cases), 64, 64, 3), 0xFF, dtype=np.uint8)
    rows = np.array([r for _, r in cases], dtype=np.int32)
    outs = []
    for i, (img, row) in enumerate(cases):
        src[i, :img.shape[0], :img.shape[1]] = img
        outs.append(pillow(src[i], row))
    out["small_src"], out["small_rows"], out["small_out"] = src, rows, np.stack(outs)
    yy, xx = np.mgrid[0:300, 0:400]
    ev = np.stack([(yy * 255 // 299), (xx * 255 // 399), ((yy // 8 + xx // 8) & 1) * 255], axis=2).astype(np.uint8)
    ev[100:140, 150:210] = rng.integers(0, 256, (40, 60, 3), dtype=np.uint8)
    fh, fw = 256, int(256 * 400 / 300)                                              # torchvision's Resize(256): short side 256, long side int(256 * long / short)
    oy, ox = int(round((fh - 224) / 2.0)), int(round((fw - 224) / 2.0))             # CenterCrop(224)
    assert (fh, fw, oy, ox) == (256, 341, 16, 58)
    erow = (300, 400, 0, 0, 300, 400, fh, fw, oy, ox, 0)
    out["eval_src"], out["eval_row"], out["eval_out"] = ev, np.array(erow, dtype=np.int32), pillow(ev, erow)
    out["eval_sizes"] = np.array([fh, fw, oy, ox], dtype=np.int32)
    assert np.array_equal(out["eval_out"], np.asarray(Image.fromarray(ev).resize((341, 256), Image.BICUBIC).crop((58, 16, 58 + 224, 16 + 224))))
    assert out["small_out"][5].min() == 0 and out["small_out"][5].max() == 255       # the checkerboard's overshoot clamps at both ends
    os.makedirs(os.path.join(HERE, "resample"), exist_ok=True)
    path = os.path.join(HERE, "resample", "resample.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
