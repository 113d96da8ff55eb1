"""The numpy restatement of tests/resample_refs.py without its bound of 11 taps: the reference of csrc/resample_wide.h /
csrc/resample_wide.hip (device crop / resize at any downscale).  Everything that does not depend on the tap count is imported from
resample_refs; ``coeffs`` sizes its arrays by the axis (Pillow's ksize = ceil(support) * 2 + 1) and ``coeff_table`` pads them to the 75
words the wide kernels store.  Pinned to Pillow's recorded bytes (tests/golden/resample/resample_wide.npz), to Pillow itself where PIL
imports and to resample_refs where both apply by tests/test_resample_wide_host.py."""
import math

import numpy as np

from resample_refs import OUT, PRECISION_BITS, bicubic, eval_geometry, pillow_row  # noqa: F401

KMAX = 75              # csrc/resample_wide.h's RSW_KMAX: a box side is at most 4096, `full` at least 224
FIELDS = 2 + KMAX


def ksize(in_size, out_size):
    """Pillow's ksize: the coefficient words it allocates per output position."""
    return int(math.ceil(2.0 * max(in_size / out_size, 1.0))) * 2 + 1


def coeffs(in_size, out_size, positions, width=None):
    """(first tap, tap count, int32 coefficients [n, width]) of the output positions ``positions`` of an axis that resizes ``in_size``
    source pixels to ``out_size``; ``width`` (None: Pillow's ksize) words per position.  resample_refs.coeffs operation for operation."""
    width = ksize(in_size, out_size) if width is None else int(width)
    xx = np.asarray(positions, dtype=np.float64)
    scale = np.float64(in_size) / np.float64(out_size)
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ss = 1.0 / fs
    center = (xx + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size) - xmin
    assert xmax.max() <= width, (in_size, out_size, int(xmax.max()), width)
    x = np.arange(width, dtype=np.int64)[None, :]
    w = bicubic(((x + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss)
    w = np.where(x < xmax[:, None], w, 0.0)
    ww = np.zeros(len(xx), dtype=np.float64)
    for j in range(width):            # summed in index order
        ww = ww + w[:, j]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    k = np.where(w < 0, np.trunc(-0.5 + w * float(1 << PRECISION_BITS)), np.trunc(0.5 + w * float(1 << PRECISION_BITS))).astype(np.int32)
    return xmin.astype(np.int32), xmax.astype(np.int32), k


def coeff_table(row):
    """int32 [2, FIELDS, 224]: what dyt_resample_wide_coeffs returns for the row (axis 0 = output rows, 1 = output columns)."""
    _, _, _, _, bh, bw, fh, fw, oy, ox, _ = row
    out = np.zeros((2, FIELDS, OUT), dtype=np.int32)
    for axis, (n_in, n_out, off) in enumerate(((bh, fh, oy), (bw, fw, ox))):
        lo, cnt, k = coeffs(n_in, n_out, off + np.arange(OUT), width=KMAX)
        out[axis, 0], out[axis, 1], out[axis, 2:] = lo, cnt, k.T
    return out


def _pass(pix, lo, cnt, k):
    """pix uint8 [n_in, m, 3] resampled along axis 0 -> uint8 [224, m, 3]: resample_refs._pass on bytes (a 4096 x 4096 source widened
    to int64 as a whole would take 400 MB), the accumulator of each output row in int64 and checked against int32."""
    out = np.empty((OUT,) + pix.shape[1:], dtype=np.uint8)
    for o in range(OUT):
        ss = np.full(pix.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int64)
        for x in range(int(cnt[o])):
            ss += pix[lo[o] + x].astype(np.int64) * int(k[o, x])
        assert ss.max() < 2 ** 31 and ss.min() >= -2 ** 31   # Pillow accumulates in int32
        out[o] = np.clip(ss >> PRECISION_BITS, 0, 255)
    return out


def resample_image(src, row):
    """src uint8 [Hs, Ws, 3] (padded), row as in resample_refs -> uint8 [224, 224, 3].  Only the source rows the window's vertical taps
    read are resampled horizontally (the others reach no output)."""
    sh, sw, top, left, bh, bw, fh, fw, oy, ox, flags = (int(v) for v in row)
    assert 1 <= sh <= src.shape[0] and 1 <= sw <= src.shape[1]
    assert bh >= 1 and bw >= 1 and top >= 0 and left >= 0 and top + bh <= sh and left + bw <= sw
    assert fh >= OUT and fw >= OUT and 0 <= oy <= fh - OUT and 0 <= ox <= fw - OUT
    vlo, vcnt, vk = coeffs(bh, fh, oy + np.arange(OUT))
    r0, r1 = int(vlo.min()), int((vlo + vcnt).max())
    box = src[top + r0:top + r1, left:left + bw]
    lo, cnt, k = coeffs(bw, fw, ox + np.arange(OUT))
    tmp = _pass(box.transpose(1, 0, 2), lo, cnt, k).transpose(1, 0, 2)        # horizontal first: [r1 - r0, 224, 3] bytes
    out = _pass(tmp, vlo - r0, vcnt, vk)                     # then vertical
    return out[:, ::-1].copy() if flags & 1 else out


def resample_batch(pixels, rows):
    """pixels uint8 [B, Hs, Ws, 3], one row per image -> uint8 [B, 224, 224, 3]"""
    return np.stack([resample_image(np.asarray(pixels[i]), rows[i]) for i in range(len(rows))])


def pattern(h, w):
    """A source uint8 [h, w, 3] made of the pixel coordinates alone, in integer arithmetic (the same bytes on every machine): gradients in
    two channels and checkerboards of periods 1 to 3 in the third; across the long axis a band of a saturated period-1 checkerboard in all
    channels and a band of hashed noise.  The sources behind tests/golden/resample/resample_wide.npz, which are too large to store."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    img = np.stack([yy * 255 // max(h - 1, 1), xx * 255 // max(w - 1, 1), (((yy + xx) // (1 + (yy // 7 + xx // 90) % 3)) & 1) * 255], axis=2)
    along = yy if h >= w else xx
    n = max(h, w)
    sat = (along >= n // 5) & (along < n // 5 + n // 10)
    img[sat] = ((((yy + xx) & 1) * 255)[sat])[:, None]
    noise = (along >= n // 2) & (along < n // 2 + n // 8)
    c = np.arange(3, dtype=np.int64)[None, None, :]
    mixed = (yy[..., None] * 73856093) ^ (xx[..., None] * 19349663) ^ ((c + 1) * 83492791)
    mixed = ((mixed & 0xFFFFF) * 2654435761) & 0xFFFFFFFF          # below 2^52: no wrap in int64
    img[noise] = ((mixed >> 13) & 0xFF)[noise]
    return img.astype(np.uint8)


def checkerboard(h, w, period=1):
    """A saturated 0 / 255 checkerboard uint8 [h, w, 3]: drives the accumulators to both clamps."""
    v = ((np.add.outer(np.arange(h), np.arange(w)) // period) & 1) * 255
    return v.astype(np.uint8)[..., None].repeat(3, axis=2)
