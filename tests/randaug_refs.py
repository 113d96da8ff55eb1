"""Numpy restatement of the twelve device operations of RandAugment (csrc/randaug.h): Pillow's 8-bit arithmetic behind the reference's
video_datasets/rand_augment.py -- ImageOps.autocontrast / equalize / invert / posterize / solarize, Image.point, ImageEnhance.Brightness /
Color / Contrast / Sharpness (Image.blend against a degenerate image), ImageFilter.SMOOTH and Image.transform(AFFINE) with a fill colour
and the bilinear or bicubic filter -- operation for operation in the order Pillow's C evaluates them, so every comparison is byte for byte.
tests/test_randaug_refs_host.py pins this file to the reference's recorded output (tests/golden/randaug/randaug.npz) and to live Pillow.

A frame is uint8 [h, w, 3].  A row is ``(op, iarg, factor, coeffs[6], filter, fill[3])``; ``apply_row(frame, row)`` gives the new frame."""
import numpy as np

IDENTITY, INVERT, SOLARIZE, SOLARIZE_ADD, POSTERIZE, AUTO_CONTRAST, EQUALIZE, BRIGHTNESS, COLOR, CONTRAST, SHARPNESS, AFFINE = range(12)
OP_NAMES = ("Identity", "Invert", "Solarize", "SolarizeAdd", "Posterize", "AutoContrast", "Equalize", "Brightness", "Color", "Contrast",
            "Sharpness", "Affine")
BILINEAR, BICUBIC = 2, 3          # PIL.Image.BILINEAR / BICUBIC
FILL = (128, 128, 128)
NO_COEFFS = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def row(op, iarg=0, factor=0.0, coeffs=NO_COEFFS, filt=BICUBIC, fill=FILL):
    return (int(op), int(iarg), float(factor), tuple(float(c) for c in coeffs), int(filt), tuple(int(v) for v in fill))


def luminance(frame):
    """convert("L"): uint8 [h, w]"""
    f = frame.astype(np.int64)
    return ((f[..., 0] * 19595 + f[..., 1] * 38470 + f[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def clip8(t):
    """t <= 0 -> 0, t >= 255 -> 255, else truncated (a float array of any precision)"""
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.int64))).astype(np.uint8)


def blend(deg, img, alpha):
    """Image.blend(degenerate, image, alpha): fp32, truncated for 0 <= alpha <= 1 and clipped otherwise"""
    a = np.float32(alpha)
    d, v = deg.astype(np.int64), img.astype(np.int64)
    t = d.astype(np.float32) + a * (v - d).astype(np.float32)
    assert t.dtype == np.float32
    if 0.0 <= float(a) <= 1.0:
        return t.astype(np.int64).astype(np.uint8)
    return clip8(t)


def smooth(frame):
    """ImageFilter.SMOOTH: the one-pixel border is the source's; a frame with a side under 3 is copied"""
    h, w = frame.shape[:2]
    out = frame.copy()
    if h < 3 or w < 3:
        return out
    k = np.array([1, 1, 1, 1, 5, 1, 1, 1, 1], dtype=np.float32) / np.float32(13)
    f = frame.astype(np.float32)

    def line(r, k0, k1, k2):
        return (r[:, :-2] * k0 + r[:, 1:-1] * k1) + r[:, 2:] * k2
    ss = np.float32(0.5) + line(f[2:], k[0], k[1], k[2])       # the row below
    ss = ss + line(f[1:-1], k[3], k[4], k[5])
    ss = ss + line(f[:-2], k[6], k[7], k[8])                   # the row above
    assert ss.dtype == np.float32
    out[1:-1, 1:-1] = clip8(ss)
    return out


def histograms(frame):
    """int64 [4, 256]: R, G, B and L"""
    return np.stack([np.bincount(frame[..., c].ravel(), minlength=256) for c in range(3)] + [np.bincount(luminance(frame).ravel(), minlength=256)])


def autocontrast_table(hist):
    nz = np.nonzero(hist)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    if hi <= lo:
        return np.arange(256, dtype=np.uint8)
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return np.array([min(255, max(0, int(i * scale + offset))) for i in range(256)], dtype=np.uint8)


def equalize_table(hist):
    nz = [int(v) for v in hist if v]
    if len(nz) <= 1:
        return np.arange(256, dtype=np.uint8)
    step = (sum(nz) - nz[-1]) // 255
    if not step:
        return np.arange(256, dtype=np.uint8)
    lut, n = [], step // 2
    for i in range(256):
        lut.append(min(n // step, 255))
        n += int(hist[i])
    return np.array(lut, dtype=np.uint8)


def contrast_mean(hist_l):
    """int(ImageStat.Stat(L).mean[0] + 0.5)"""
    total = int(sum(i * int(hist_l[i]) for i in range(256)))
    return int(total / int(hist_l.sum()) + 0.5)


def table(op, iarg, hist):
    """uint8 [3, 256] of a table operation; ``hist`` [4, 256] of the frame (used by AutoContrast and Equalize only)"""
    i = np.arange(256)
    if op == IDENTITY:
        t = i
    elif op == INVERT:
        t = 255 - i
    elif op == SOLARIZE:
        t = np.where(i < iarg, i, 255 - i)
    elif op == SOLARIZE_ADD:
        t = np.where(i < 128, np.minimum(255, i + iarg), i)
    elif op == POSTERIZE:
        t = i if iarg >= 8 else i & ~((1 << (8 - iarg)) - 1)
    elif op == AUTO_CONTRAST:
        return np.stack([autocontrast_table(hist[c]) for c in range(3)])
    elif op == EQUALIZE:
        return np.stack([equalize_table(hist[c]) for c in range(3)])
    else:
        raise ValueError("op %d has no table" % op)
    return np.tile(t.astype(np.uint8), (3, 1))


def _cubic(v1, v2, v3, v4, d):
    p1 = v2
    p2 = -v1 + v3
    p3 = 2 * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    return p1 + d * (p2 + d * (p3 + d * p4))


def affine(frame, coeffs, filt=BICUBIC, fill=FILL):
    """Image.transform(size, AFFINE, coeffs, resample=filt, fillcolor=fill), fp64"""
    h, w = frame.shape[:2]
    a = [np.float64(c) for c in coeffs]
    xc = (np.arange(w, dtype=np.float64) + 0.5)[None, :]
    yc = (np.arange(h, dtype=np.float64) + 0.5)[:, None]
    xin = a[0] * xc + a[1] * yc + a[2]
    yin = a[3] * xc + a[4] * yc + a[5]
    inside = ~((xin < 0) | (xin >= w) | (yin < 0) | (yin >= h))
    xin, yin = np.where(inside, xin, 0.5) - 0.5, np.where(inside, yin, 0.5) - 0.5
    x0, y0 = np.floor(xin), np.floor(yin)
    dx, dy = (xin - x0)[..., None], (yin - y0)[..., None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    f = frame.astype(np.float64)

    def tap(yy, xx):
        return f[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
    if filt == BILINEAR:
        r0 = tap(y0, x0) + dx * (tap(y0, x0 + 1) - tap(y0, x0))
        r1 = tap(y0 + 1, x0) + dx * (tap(y0 + 1, x0 + 1) - tap(y0 + 1, x0))
        v = (r0 + dy * (r1 - r0)).astype(np.int64).astype(np.uint8)
    elif filt == BICUBIC:
        rows = [_cubic(tap(y0 + j, x0 - 1), tap(y0 + j, x0), tap(y0 + j, x0 + 1), tap(y0 + j, x0 + 2), dx) for j in (-1, 0, 1, 2)]
        v = clip8(_cubic(rows[0], rows[1], rows[2], rows[3], dy))
    else:
        raise ValueError("filter %r" % (filt,))
    return np.where(inside[..., None], v, np.array(fill, dtype=np.uint8)[None, None, :]).astype(np.uint8)


def apply_row(frame, r):
    op, iarg, factor, coeffs, filt, fill = r
    if op <= EQUALIZE:
        t = table(op, iarg, histograms(frame) if op in (AUTO_CONTRAST, EQUALIZE) else None)
        return np.stack([t[c][frame[..., c]] for c in range(3)], axis=2)
    if op == BRIGHTNESS:
        return blend(np.zeros_like(frame), frame, factor)
    if op == COLOR:
        return blend(np.repeat(luminance(frame)[..., None], 3, axis=2), frame, factor)
    if op == CONTRAST:
        return blend(np.full_like(frame, contrast_mean(histograms(frame)[3])), frame, factor)
    if op == SHARPNESS:
        return blend(smooth(frame), frame, factor)
    if op == AFFINE:
        return affine(frame, coeffs, filt, fill)
    raise ValueError("op %r" % (op,))


def rotate_coeffs(degrees, h, w):
    """The matrix PIL.Image.rotate(degrees) hands to transform(AFFINE) for an image of w x h (None: rotate() copies, angle % 360 == 0)"""
    import math
    angle = degrees % 360.0
    if angle == 0:
        return None
    cx, cy = w / 2.0, h / 2.0
    angle = -math.radians(angle)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0, round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return tuple(m)


def apply_batch(batch, sizes, rows, layers):
    """``batch`` uint8 [units, frames, Hs, Ws, 3], ``sizes`` [(h, w)] per unit, ``rows`` [units * layers] (unit-major): the augmented batch;
    bytes outside a unit's valid h x w stay as they are."""
    out = batch.copy()
    for u, (h, w) in enumerate(sizes):
        for f in range(batch.shape[1]):
            fr = np.ascontiguousarray(batch[u, f, :h, :w])
            for layer in range(layers):
                fr = apply_row(fr, rows[u * layers + layer])
            out[u, f, :h, :w] = fr
    return out
