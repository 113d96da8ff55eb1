"""Shared by tests/test_mix_host.py and tests/test_gpu_mix.py: the torch / numpy references of the on-device Mixup / CutMix.

The fused path is DEFINED as "the float path on the mixed image": ``lam * x + (1.0 - lam) * x.flip(0)`` as torch evaluates it (three fp32
roundings; synth.mixup_batch's expression), a box copied from ``x.flip(0)`` for cutmix, the image itself for the identity draw.  For the video
model ``flip(0)`` acts on clips.  The targets are synth.mixup_batch's second return value.  Every comparison built on these is exact."""
import math

import numpy as np
import torch

IMG = 224
BOXES = {"empty": (40, 40, 10, 90), "full": (0, 224, 0, 224), "crossing": (5, 37, 3, 50), "aligned": (16, 48, 32, 64), "one_pixel": (0, 1, 223, 224)}


def partner_images(x, frames=1):
    """x [n,...] -> the image every image is paired with: the same frame of the mirrored clip (x.flip(0) for frames == 1)."""
    n = x.shape[0]
    return x.reshape(n // frames, frames, *x.shape[1:]).flip(0).reshape(x.shape)


def mix_images(x, draw, frames=1):
    """fp32 [n,3,224,224] mixed as ``draw`` (util.mixup.MixDraw) says, with torch on x's device."""
    assert x.dtype == torch.float32 and tuple(x.shape[1:]) == (3, IMG, IMG)
    xp = partner_images(x, frames)
    if draw.mode == 0:
        return x.clone()
    if draw.mode == 1:
        lam = draw.lam
        return lam * x + (1.0 - lam) * xp
    yl, yh, xl, xh = draw.box
    out = x.clone()
    out[:, :, yl:yh, xl:xh] = xp[:, :, yl:yh, xl:xh]
    return out


def one_hot_rows(y, num_classes, smoothing):
    """synth.mixup_batch's t(y)."""
    off = smoothing / num_classes
    return torch.full((y.shape[0], num_classes), off, dtype=torch.float32, device=y.device).scatter_(1, y.view(-1, 1), 1.0 - smoothing + off)


def mix_targets(y, num_classes, draw, smoothing, criterion_smoothing=0.0):
    """synth.mixup_batch's second return value for the draw's lam, then train_step's map of the criterion's label_smoothing."""
    lam = draw.lam
    t = one_hot_rows(y, num_classes, smoothing)
    t = lam * t + (1.0 - lam) * t.flip(0)
    if criterion_smoothing > 0.0:
        t = t * (1.0 - criterion_smoothing) + criterion_smoothing / num_classes
    return t


def mix_targets_f64(y, num_classes, draw, smoothing, criterion_smoothing=0.0):
    """The same in float64 from the exact parameters: what the three (five) fp32 roundings approximate."""
    off = smoothing / num_classes
    t = np.full((y.shape[0], num_classes), off, dtype=np.float64)
    t[np.arange(y.shape[0]), y.cpu().numpy()] = 1.0 - smoothing + off
    t = draw.lam * t + (1.0 - draw.lam) * t[::-1]
    if criterion_smoothing > 0.0:
        t = t * (1.0 - criterion_smoothing) + criterion_smoothing / num_classes
    return t


def callable_for(draws, num_classes, smoothing, frames=1):
    """A ``mixup_fn`` of the loop's callable branch that applies ``draws`` in order with the functions above: float images [n,3,224,224] or
    clips [b,3,t,224,224] and integer labels in, mixed images and class-probability targets out."""
    queue = list(draws)

    def mixup_fn(samples, targets):
        d = queue.pop(0)
        if samples.dim() == 5:
            b, c, t, h, w = samples.shape
            fr = samples.permute(0, 2, 1, 3, 4).reshape(b * t, c, h, w)
            mixed = mix_images(fr.float(), d, t).reshape(b, t, c, h, w).permute(0, 2, 1, 3, 4)
        else:
            mixed = mix_images(samples.float(), d, frames)
        return mixed, mix_targets(targets, num_classes, d, smoothing)
    return mixup_fn


# ---- numpy tables of csrc/mix.h for tools/mix_check.cpp --------------------------------------------------------------------------------
def partner_table():
    rows = []
    for frames in (1, 2):
        for clips in (2, 4, 6):
            count = clips * frames
            ids = np.arange(count).reshape(clips, frames)
            want = ids[::-1].reshape(-1)
            rows += [(n, count, frames, int(want[n])) for n in range(count)]
    return np.asarray(rows, dtype="<i4")


def value_table(seed=7):
    """fp32 pairs x weights -> r(r(lam a) + r(oml b)) in numpy float32 (each operation rounds once)."""
    g = np.random.default_rng(seed)
    a = np.concatenate([g.standard_normal(4000), g.uniform(-3, 3, 4000) * 10.0 ** g.integers(-6, 6, 4000), [0.0, -0.0, 1.0, -1.0, 2.6400001, -2.1179039]]).astype(np.float32)
    b = np.concatenate([g.standard_normal(4000), g.uniform(-3, 3, 4000) * 10.0 ** g.integers(-6, 6, 4000), [-0.0, 0.0, 1.0, 3.0, -2.1179039, 2.6400001]]).astype(np.float32)
    lam = np.concatenate([g.beta(0.8, 0.8, a.size - 6), [0.7, 0.0, 1.0, 0.5, 0.999, 1e-3]])
    lam_f, oml_f = lam.astype(np.float32), (1.0 - lam).astype(np.float32)
    want = (lam_f * a).astype(np.float32) + (oml_f * b).astype(np.float32)
    assert want.dtype == np.float32
    return np.stack([a, b, lam_f, oml_f, want], axis=1).astype("<f4")


def predicate_table():
    rows = []
    for mode in (0, 1, 2):
        for box in list(BOXES.values()) + [(0, 0, 0, 0), (100, 101, 0, 224)]:
            yl, yh, xl, xh = box
            for y in sorted({0, 1, yl - 1, yl, yh - 1, yh, 223} & set(range(IMG))):
                for x in sorted({0, 2, xl - 1, xl, xl + 1, xh - 1, xh, 208, 223} & set(range(IMG))):
                    rows.append((mode, y, x, yl, yh, xl, xh, int(mode == 2 and yl <= y < yh and xl <= x < xh)))
    return np.asarray(rows, dtype="<i4")


def rand_bbox_numpy(lam, cy, cx):
    """timm's rand_bbox for a 224 x 224 image, centre given, and the corrected lam."""
    ratio = np.sqrt(1 - lam)
    cut_h, cut_w = int(IMG * ratio), int(IMG * ratio)
    yl, yh = np.clip(cy - cut_h // 2, 0, IMG), np.clip(cy + cut_h // 2, 0, IMG)
    xl, xh = np.clip(cx - cut_w // 2, 0, IMG), np.clip(cx + cut_w // 2, 0, IMG)
    return (int(yl), int(yh), int(xl), int(xh)), 1. - (yh - yl) * (xh - xl) / float(IMG * IMG)


def box_table():
    rec = np.dtype([("lam", "<f8"), ("want_lam", "<f8"), ("cy", "<i4"), ("cx", "<i4"), ("yl", "<i4"), ("yh", "<i4"), ("xl", "<i4"), ("xh", "<i4")])
    rows = []
    for lam in (0.0, 1.0, 0.5, 0.999, 0.3, 0.87):
        for cy, cx in ((0, 0), (0, 223), (223, 0), (223, 223), (112, 112), (17, 200)):
            box, want = rand_bbox_numpy(lam, cy, cx)
            rows.append((lam, float(want), cy, cx) + box)
    out = np.asarray(rows, dtype=rec)
    assert out.itemsize == 40
    return out


def write_tables(path, value=None):
    parts = [partner_table(), value_table() if value is None else value, predicate_table(), box_table()]
    with open(path, "wb") as f:
        f.write(np.asarray([len(p) for p in parts], dtype="<i4").tobytes())
        for p in parts:
            f.write(p.tobytes())


assert math.isclose(rand_bbox_numpy(0.5, 112, 112)[1], 1.0 - (2 * (int(IMG * math.sqrt(0.5)) // 2)) ** 2 / IMG ** 2)
