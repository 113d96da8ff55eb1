#!/usr/bin/env python3
"""Generate tests/golden/erase/erase_draws.npz: the boxes the reference's RandomErasing draws, as erased-pixel masks.

Build container only (reads /root/reference; the arrays it writes are data and are what travels).  The reference's
video_datasets/random_erasing.py is loaded BY FILE PATH (the package's __init__ pulls the video dependencies; the file alone needs torch
only).  For each configuration the ``random`` module is seeded, the eraser runs in ``mode='const'`` on a tensor of ones -- 16 images, or
8 clips of 2 frames one clip per call with ``cube=True``, the way the clip pipeline calls it -- and the script records

* ``<name>_mask``: the zeroed pixels [16, 224, 224] through ``np.packbits``;
* ``<name>_next``: the value of the next ``random.random()``, which pins the number of draws consumed;
* ``<name>_boxes`` / ``<name>_attempts``: per unit the boxes placed and the attempts made (counted by wrapping ``random.uniform`` /
  ``random.randint`` around the calls; the stream is untouched);
* ``<name>_cfg``: seed, units, frames, cube, probability, max_area, min_count, max_count.

tests/test_erase_host.py checks that util.erasing.DeviceRandomErasing(generator=random.Random(seed)) reproduces every mask and the next
draw exactly.  Usage:  python tests/golden/make_golden_erase.py
"""
import importlib.util
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (the reference's root in front of sys.path, the third-party stand-ins)

REF = os.path.join(mg.REF, "video_datasets", "random_erasing.py")
SEED = 7
# name -> (units, frames, cube, kwargs)
CONFIGS = {
    "p25_count1": (16, 1, False, dict(probability=0.25)),
    "p25_count1to3": (16, 1, False, dict(probability=0.25, min_count=1, max_count=3)),
    "p100_area100": (16, 1, False, dict(probability=1.0, max_area=1.0)),
    "p50_cube": (8, 2, True, dict(probability=0.5)),
}


def load_reference():
    spec = importlib.util.spec_from_file_location("reference_random_erasing", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Counter:
    """Counts random.uniform / random.randint calls without touching the stream."""

    def __enter__(self):
        self.uniform = self.randint = 0
        self._u, self._r = random.uniform, random.randint

        def uniform(a, b):
            self.uniform += 1
            return self._u(a, b)

        def randint(a, b):
            self.randint += 1
            return self._r(a, b)
        random.uniform, random.randint = uniform, randint
        return self

    def __exit__(self, *exc):
        random.uniform, random.randint = self._u, self._r


def main():
    ref = load_reference()
    out = {}
    for name, (units, frames, cube, kw) in CONFIGS.items():
        eraser = ref.RandomErasing(mode="const", device="cpu", cube=cube, **kw)
        random.seed(SEED)
        x = torch.ones(units * frames, 3, 224, 224)
        boxes, attempts = [], []
        for u in range(units):
            with Counter() as cnt:
                view = x[u * frames:(u + 1) * frames] if cube else x[u:u + 1]
                eraser(view)
            drew_count = eraser.min_count != eraser.max_count and cnt.uniform > 0
            attempts.append(cnt.uniform // 2)
            boxes.append((cnt.randint - (1 if drew_count else 0)) // 2)
        nxt = random.random()
        mask = (x[:, 0] == 0).numpy()
        assert np.array_equal(mask, (x[:, 1] == 0).numpy()) and np.array_equal(mask, (x[:, 2] == 0).numpy())
        erased = mask.reshape(units, frames, -1).any(axis=(1, 2))
        boxes, attempts = np.array(boxes, dtype=np.int32), np.array(attempts, dtype=np.int32)
        assert np.array_equal(erased, boxes > 0)
        assert erased.any() and (not erased.all() or kw["probability"] >= 1.0), name
        if cube:
            m = mask.reshape(units, frames, 224, 224)
            assert all(np.array_equal(m[:, 0], m[:, f]) for f in range(frames))   # all frames of a clip share the boxes
        print("%-14s erased %d of %d units, boxes %s, attempts %s, next %.17g" % (name, erased.sum(), units, boxes.tolist(), attempts.tolist(), nxt))
        out[name + "_mask"] = np.packbits(mask.reshape(-1))
        out[name + "_next"] = np.float64(nxt)
        out[name + "_boxes"] = boxes
        out[name + "_attempts"] = attempts
        out[name + "_cfg"] = np.array([SEED, units, frames, int(cube), kw["probability"], kw.get("max_area", 1 / 3), kw.get("min_count", 1),
                                       kw.get("max_count", kw.get("min_count", 1))], dtype=np.float64)
    # what the golden must contain
    assert (out["p25_count1_boxes"] == 0).any() and (out["p25_count1_boxes"] > 0).any()       # an untouched and an erased image
    assert (out["p25_count1to3_boxes"] >= 2).any()                                             # an image with 2 or more boxes
    assert (out["p100_area100_attempts"] > out["p100_area100_boxes"]).any()                    # a rejected attempt (h or w >= 224)
    assert (out["p50_cube_boxes"] > 0).any() and (out["p50_cube_boxes"] == 0).any()
    os.makedirs(os.path.join(HERE, "erase"), exist_ok=True)
    path = os.path.join(HERE, "erase", "erase_draws.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
