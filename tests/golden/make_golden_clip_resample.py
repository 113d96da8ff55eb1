#!/usr/bin/env python3
"""Generate tests/golden/resample/clip_resample.npz: the draws and the pixels of the reference's video spatial pipeline.

Build container only (reads /root/reference; the arrays it writes are data and are what travels).  The reference's
video_datasets/transform.py and video_datasets/k400.py are loaded BY FILE PATH, as the modules of a package made here, with empty
stand-ins for the absent ``torchvision``, ``decord`` and ``av`` (none of the functions run below touches them).  Executed from the
reference, its OWN code: ``random_short_side_scale_jitter``, ``random_crop``, ``random_resized_crop``, ``_get_param_spatial_crop``,
``VideoDataset._generate_spatial_crops`` (called on a stand-in ``self`` that carries num_spatial_views and spatial_size) and the default
``mean`` / ``std`` of ``VideoDataset.__init__``.  RESTATED here, because they are lines inside ``VideoDataset.__getitem__`` that cannot run
without a video decoder:
  * ``frames = torch.as_tensor(np.stack(frames)).float() / 255.``, ``frames = (frames - self.mean) / self.std`` and
    ``frames.permute(3, 0, 1, 2)`` (k400.py:127, 141-142 and 190-193);
  * the mirror ``if self.mirror and torch.rand(1).item() < 0.5: frames = frames.flip(dims=(-1,))`` (:163-164);
  * the evaluation resize ``new_width = W * size // H, new_height = size`` (or the other way round) and the ``interpolate`` call behind it
    (:195-203).
``random_crop`` and ``random_resized_crop`` do not return their offsets / box: they are learnt by running the same function (or
``_get_param_spatial_crop``) a second time from the same generator state -- on a tensor of coordinates for ``random_crop``.

(a) Draws, for each of two seeds and 12 clip sizes in loader order (``sizes`` [12, 2] = height, width):
    ``jit<seed>_rows`` [12, 5] = full_h, full_w, off_y, off_x, mirror of the K400 train path with scale_range (1.0, 1.15) and mirror on
    (np.random.seed(seed), torch.manual_seed(seed)); ``jit<seed>_next`` = the next np.random.uniform() and torch.rand(1);
    ``rrc<seed>_boxes`` [12, 4] = i, j, h, w of ``_get_param_spatial_crop((0.08, 1.0), (3/4, 4/3), h, w)`` (random.seed(seed),
    np.random.seed(seed)); ``rrc<seed>_next`` = the next random.random() and np.random.uniform() -- they pin the number consumed.
    ``uni_rows1`` [12, 4] and ``uni_rows3`` [12, 3, 4] = full_h, full_w, off_y, off_x of the evaluation path with 1 and 3 spatial views.
(b) Pixels: ``px_src`` uint8 [5, 2, 64, 64, 3] (sources of at most 64 x 64, padded with 0xFF), ``px_rows`` [7, 12] -- rows of
    csrc/resample_clip.h: src_h, src_w, top, left, box_h, box_w, full_h, full_w, off_y, off_x, flags, src -- ``px_frames`` [7] (1 or 2
    frames are valid) and the reference's fp32 output: ``px_full`` [3, 224, 224] = frame 0 of row 0 in full, and ``px_samples``
    [7, 2, 3, 33, 33] = rows and columns ``px_index`` (every 7th and the last) of every row's frames.  ``eval_src`` uint8
    [1, 300, 400, 3] (one frame), ``eval_rows`` [3, 12] (three spatial views sharing src 0) and ``eval_samples`` [3, 2, 3, 33, 33] (the
    second frame is zeros).  One full frame and strided samples keep the file under the repository's 1 MiB limit.
    ``norm`` [2, 3] = the mean and std used (the reference's defaults).

tests/test_clip_resample_refs_host.py pins tests/clip_resample_refs.py to the pixels, tests/test_clip_crop_host.py pins util.crop to the draws.
Usage:  python tests/golden/make_golden_clip_resample.py
"""
import importlib
import inspect
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (the reference's root in front of sys.path, the third-party stand-ins)

REF_DIR = os.path.join(mg.REF, "video_datasets")
SEEDS = (0, 1234)
SIZES = [(240, 320), (256, 340), (320, 240), (224, 224), (480, 640), (128, 171), (360, 360), (225, 400),
         (32, 512), (512, 32), (96, 64), (300, 400)]   # (h, w); the two 16:1 clips make _get_param_spatial_crop fall back
OUT = 224
INDEX = np.r_[0:OUT:7, OUT - 1]


def load_reference():
    """(transform, k400) of the reference, as modules of a package ``reference_video_datasets`` whose path is the reference's directory."""
    names = ("torchvision", "torchvision.transforms", "torchvision.transforms.functional", "decord", "av")
    saved = {k: sys.modules.get(k) for k in names}
    tv, tr, fn = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms"), types.ModuleType("torchvision.transforms.functional")
    tr.functional, tv.transforms = fn, tr
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tr, "torchvision.transforms.functional": fn,
                        "decord": types.ModuleType("decord"), "av": types.ModuleType("av")})
    try:
        pkg = types.ModuleType("reference_video_datasets")
        pkg.__path__ = [REF_DIR]
        sys.modules["reference_video_datasets"] = pkg
        transform = importlib.import_module("reference_video_datasets.transform")
        k400 = importlib.import_module("reference_video_datasets.k400")
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    assert os.path.realpath(transform.__file__).startswith(REF_DIR) and os.path.realpath(k400.__file__).startswith(REF_DIR)
    return transform, k400


def normalised(clip, mean, std):
    """k400.py:127 / 141-142, restated: uint8 [T, H, W, 3] -> fp32 [C, T, H, W]."""
    frames = torch.as_tensor(np.ascontiguousarray(clip)).float() / 255.
    frames = (frames - mean) / std
    return frames.permute(3, 0, 1, 2)


def coordinates(h, w):
    """[2, 1, h, w]: the row and the column number of every position."""
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    return torch.stack([yy, xx])[:, None]


def crop_offsets(tr, h, w):
    """The offsets the reference's random_crop draws for a clip of h x w: its own call, on coordinates."""
    cropped, _ = tr.random_crop(coordinates(h, w), OUT)
    return int(cropped[0, 0, 0, 0]), int(cropped[1, 0, 0, 0])


def jitter_row(tr, h, w, min_size, max_size):
    """(full_h, full_w, off_y, off_x, mirror) of one clip through the K400 train path, consuming the generators as the dataset does."""
    frames, _ = tr.random_short_side_scale_jitter(torch.zeros(3, 1, h, w), min_size=min_size, max_size=max_size, interpolation="bilinear")
    fh, fw = int(frames.shape[2]), int(frames.shape[3])
    oy, ox = crop_offsets(tr, fh, fw)
    mirror = torch.rand(1).item() < 0.5      # k400.py:163, restated
    return fh, fw, oy, ox, int(mirror)


def eval_full(h, w):
    """k400.py:195-200, restated."""
    if h < w:
        return OUT, w * OUT // h
    return h * OUT // w, OUT


def spatial_offsets(k400, fh, fw, views):
    me = types.SimpleNamespace(num_spatial_views=views, spatial_size=OUT)
    crops = k400.VideoDataset._generate_spatial_crops(me, coordinates(fh, fw))
    return [(int(c[0, 0, 0, 0]), int(c[1, 0, 0, 0])) for c in crops]


def sampled(frames):
    """fp32 [T, 3, 224, 224] -> [2, 3, 33, 33] (a missing second frame is zeros)."""
    out = np.zeros((2, 3, len(INDEX), len(INDEX)), dtype=np.float32)
    out[:frames.shape[0]] = frames[:, :, INDEX][:, :, :, INDEX]
    return out


def main():
    tr, k400 = load_reference()
    sig = inspect.signature(k400.VideoDataset.__init__).parameters
    mean, std = sig["mean"].default, sig["std"].default
    out = {"sizes": np.array(SIZES, dtype=np.int32), "norm": np.stack([mean.numpy(), std.numpy()]).astype(np.float32), "px_index": INDEX.astype(np.int32)}
    min_size, max_size = round(OUT * 1.0), round(OUT * 1.15)
    for seed in SEEDS:
        np.random.seed(seed)
        torch.manual_seed(seed)
        rows = [jitter_row(tr, h, w, min_size, max_size) for (h, w) in SIZES]
        out["jit%d_rows" % seed] = np.array(rows, dtype=np.int32)
        out["jit%d_next" % seed] = np.array([np.random.uniform(), torch.rand(1).item()], dtype=np.float64)
        assert any(r[4] for r in rows) and not all(r[4] for r in rows)
        random.seed(seed)
        np.random.seed(seed)
        boxes = [tr._get_param_spatial_crop((0.08, 1.0), (3.0 / 4.0, 4.0 / 3.0), h, w) for (h, w) in SIZES]
        out["rrc%d_boxes" % seed] = np.array(boxes, dtype=np.int32)
        out["rrc%d_next" % seed] = np.array([random.random(), np.random.uniform()], dtype=np.float64)
        print("seed %d: jitter %s boxes %s" % (seed, rows[:3], boxes[:3]))
    uni1, uni3 = [], []
    for (h, w) in SIZES:
        fh, fw = eval_full(h, w)
        uni1.append((fh, fw) + spatial_offsets(k400, fh, fw, 1)[0])
        uni3.append([(fh, fw) + o for o in spatial_offsets(k400, fh, fw, 3)])
    out["uni_rows1"], out["uni_rows3"] = np.array(uni1, dtype=np.int32), np.array(uni3, dtype=np.int32)

    # (b) pixels
    rng = np.random.default_rng(11)
    smooth = (np.add.outer(np.arange(64) * 3, np.arange(64) * 2)[..., None] + np.array([0, 40, 90])).astype(np.uint8)
    checker = ((np.add.outer(np.arange(64), np.arange(64)) & 1) * 255).astype(np.uint8)[..., None].repeat(3, axis=2)
    shapes = [(2, 48, 64), (2, 64, 40), (1, 64, 64), (2, 33, 57), (2, 64, 64)]
    src = np.full((5, 2, 64, 64, 3), 0xFF, dtype=np.uint8)
    for i, (t, h, w) in enumerate(shapes):
        src[i, :t, :h, :w] = rng.integers(0, 256, (t, h, w, 3), dtype=np.uint8)
    src[2, 0] = smooth
    src[4, 1] = checker
    rows, frames_of, outs = [], [], []

    def valid(i):
        t, h, w = shapes[i]
        return src[i, :t, :h, :w], t, h, w

    # rows 0-2: the K400 train path (scale jitter, random crop, mirror) on sources 0, 1, 2
    np.random.seed(7)
    torch.manual_seed(7)
    for i in (0, 1, 2):
        clip, t, h, w = valid(i)
        frames, _ = tr.random_short_side_scale_jitter(normalised(clip, mean, std), min_size=min_size, max_size=max_size, interpolation="bilinear")
        fh, fw = int(frames.shape[2]), int(frames.shape[3])
        state = np.random.get_state()
        oy, ox = crop_offsets(tr, fh, fw)
        np.random.set_state(state)
        frames, _ = tr.random_crop(frames, OUT)
        mirror = torch.rand(1).item() < 0.5 if i != 1 else True
        if mirror:
            frames = frames.flip(dims=(-1,))
        rows.append((h, w, 0, 0, h, w, fh, fw, oy, ox, int(mirror), i))
        frames_of.append(t)
        outs.append(frames.permute(1, 0, 2, 3).contiguous().numpy())
    # rows 3-5: the SSV2 train path (random resized crop) on sources 3, 4 and 0
    random.seed(7)
    np.random.seed(7)
    for i in (3, 4, 0):
        clip, t, h, w = valid(i)
        states = random.getstate(), np.random.get_state()
        bi, bj, bh, bw = tr._get_param_spatial_crop((0.08, 1.0), (3.0 / 4.0, 4.0 / 3.0), h, w)
        random.setstate(states[0])
        np.random.set_state(states[1])
        frames = tr.random_resized_crop(normalised(clip, mean, std), OUT, OUT, scale=(0.08, 1.0), interpolation="bilinear")
        rows.append((h, w, bi, bj, bh, bw, OUT, OUT, 0, 0, 0, i))
        frames_of.append(t)
        outs.append(frames.permute(1, 0, 2, 3).contiguous().numpy())
    # row 6: the evaluation path, one view, on source 3 (33 x 57 -> 224 x 386)
    clip, t, h, w = valid(3)
    fh, fw = eval_full(h, w)
    full = torch.nn.functional.interpolate(normalised(clip, mean, std), size=(fh, fw), mode="bilinear", align_corners=False)   # :202, restated
    me = types.SimpleNamespace(num_spatial_views=1, spatial_size=OUT)
    (view,) = k400.VideoDataset._generate_spatial_crops(me, full)
    rows.append((h, w, 0, 0, h, w, fh, fw) + spatial_offsets(k400, fh, fw, 1)[0] + (0, 3))
    frames_of.append(t)
    outs.append(view.permute(1, 0, 2, 3).contiguous().numpy())
    assert all(o.shape[1:] == (3, OUT, OUT) for o in outs)
    out["px_src"], out["px_rows"], out["px_frames"] = src, np.array(rows, dtype=np.int32), np.array(frames_of, dtype=np.int32)
    out["px_full"] = outs[0][0]
    out["px_samples"] = np.stack([sampled(o) for o in outs])
    # the 300 x 400 evaluation case, three views of one source
    yy, xx = np.mgrid[0:300, 0:400]
    ev = np.stack([(yy * 255 // 299), (xx * 255 // 399), ((yy // 8 + xx // 8) & 1) * 255], axis=2).astype(np.uint8)
    ev = ev[None].copy()
    ev[:, 100:140, 150:210] = rng.integers(0, 256, (1, 40, 60, 3), dtype=np.uint8)
    fh, fw = eval_full(300, 400)
    assert (fh, fw) == (224, 298)
    full = torch.nn.functional.interpolate(normalised(ev, mean, std), size=(fh, fw), mode="bilinear", align_corners=False)
    me = types.SimpleNamespace(num_spatial_views=3, spatial_size=OUT)
    views = k400.VideoDataset._generate_spatial_crops(me, full)
    offs = spatial_offsets(k400, fh, fw, 3)
    assert offs == [(0, 0), (0, 37), (0, 74)]
    out["eval_src"] = ev
    out["eval_rows"] = np.array([(300, 400, 0, 0, 300, 400, fh, fw) + o + (0, 0) for o in offs], dtype=np.int32)
    out["eval_samples"] = np.stack([sampled(v.permute(1, 0, 2, 3).contiguous().numpy()) for v in views])
    os.makedirs(os.path.join(HERE, "resample"), exist_ok=True)
    path = os.path.join(HERE, "resample", "clip_resample.npz")
    np.savez_compressed(path, **out)
    print("rows %s" % (rows,))
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
