"""numpy restatement of Pillow's ``Image.resize`` for 8-bit RGB images with the bicubic filter, applied to a crop box that acts as the image
(``img.crop(box).resize(full, BICUBIC)``), of the 224 x 224 window cut from it and of the mirror: the reference of csrc/resample.h /
csrc/resample.hip.  Pinned to Pillow's recorded bytes and, where PIL imports, to Pillow itself by tests/test_resample_refs_host.py.

A row is the table row of csrc/resample.h as a tuple:
    (src_h, src_w, top, left, box_h, box_w, full_h, full_w, off_y, off_x, flags)

The arithmetic (Pillow's src/libImaging/Resample.c): per axis ``precompute_coeffs`` in fp64 -- elementwise numpy operations, which round
after every operation as the C code compiled for x86-64 does -- then ``normalize_coeffs_8bpc`` to 22 bits; the horizontal pass in integers,
rounded to uint8; the vertical pass on those bytes."""
import numpy as np

OUT, KMAX, PRECISION_BITS = 224, 11, 22
FIELDS = 2 + KMAX


def bicubic(x):
    a = -0.5
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def coeffs(in_size, out_size, positions):
    """(first tap, tap count, int32 coefficients [n, KMAX]) of the output positions ``positions`` of an axis that resizes ``in_size`` source
    pixels to ``out_size``."""
    xx = np.asarray(positions, dtype=np.float64)
    scale = np.float64(in_size) / np.float64(out_size)
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ss = 1.0 / fs
    center = (xx + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size) - xmin
    assert xmax.max() <= KMAX, (in_size, out_size, int(xmax.max()))
    x = np.arange(KMAX, dtype=np.int64)[None, :]
    w = bicubic(((x + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss)
    w = np.where(x < xmax[:, None], w, 0.0)
    ww = np.zeros(len(xx), dtype=np.float64)
    for j in range(KMAX):            # summed in index order
        ww = ww + w[:, j]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    k = np.where(w < 0, np.trunc(-0.5 + w * float(1 << PRECISION_BITS)), np.trunc(0.5 + w * float(1 << PRECISION_BITS))).astype(np.int32)
    return xmin.astype(np.int32), xmax.astype(np.int32), k


def coeff_table(row):
    """int32 [2, FIELDS, 224]: what dyt_resample_coeffs returns for the row (axis 0 = output rows, 1 = output columns)."""
    _, _, _, _, bh, bw, fh, fw, oy, ox, _ = row
    out = np.zeros((2, FIELDS, OUT), dtype=np.int32)
    for axis, (n_in, n_out, off) in enumerate(((bh, fh, oy), (bw, fw, ox))):
        lo, cnt, k = coeffs(n_in, n_out, off + np.arange(OUT))
        out[axis, 0], out[axis, 1], out[axis, 2:] = lo, cnt, k.T
    return out


def _pass(pix, lo, cnt, k):
    """pix int64 [n_in, m, 3] resampled along axis 0 -> uint8 [224, m, 3]"""
    out = np.empty((OUT,) + pix.shape[1:], dtype=np.uint8)
    for o in range(OUT):
        ss = np.full(pix.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int64)
        for x in range(int(cnt[o])):
            ss += pix[lo[o] + x] * int(k[o, x])
        assert ss.max() < 2 ** 31 and ss.min() >= -2 ** 31   # Pillow accumulates in int32
        out[o] = np.clip(ss >> PRECISION_BITS, 0, 255)
    return out


def resample_image(src, row):
    """src uint8 [Hs, Ws, 3] (padded), row as above -> uint8 [224, 224, 3]"""
    sh, sw, top, left, bh, bw, fh, fw, oy, ox, flags = (int(v) for v in row)
    assert 1 <= sh <= src.shape[0] and 1 <= sw <= src.shape[1]
    assert bh >= 1 and bw >= 1 and top >= 0 and left >= 0 and top + bh <= sh and left + bw <= sw
    assert fh >= OUT and fw >= OUT and 0 <= oy <= fh - OUT and 0 <= ox <= fw - OUT
    box = src[top:top + bh, left:left + bw].astype(np.int64)
    lo, cnt, k = coeffs(bw, fw, ox + np.arange(OUT))
    tmp = _pass(box.transpose(1, 0, 2), lo, cnt, k).transpose(1, 0, 2)        # horizontal first: [bh, 224, 3] bytes
    lo, cnt, k = coeffs(bh, fh, oy + np.arange(OUT))
    out = _pass(tmp.astype(np.int64), lo, cnt, k)                             # then vertical
    return out[:, ::-1].copy() if flags & 1 else out


def resample_batch(pixels, rows):
    """pixels uint8 [B, Hs, Ws, 3], one row per image -> uint8 [B, 224, 224, 3]"""
    return np.stack([resample_image(np.asarray(pixels[i]), rows[i]) for i in range(len(rows))])


def eval_geometry(h, w, resize=256, size=224):
    """(full_h, full_w, off_y, off_x) of torchvision's Resize(resize) (short side ``resize``, long side int(resize * long / short)) followed by
    CenterCrop(size) (offsets int(round((full - size) / 2.0)), Python's round) on an h x w image."""
    if w <= h:
        fw, fh = resize, int(resize * h / w)
    else:
        fh, fw = resize, int(resize * w / h)
    return fh, fw, int(round((fh - size) / 2.0)), int(round((fw - size) / 2.0))


def pillow_row(img, row):
    """The same row through Pillow itself (needs PIL): crop, resize, window, mirror."""
    from PIL import Image
    sh, sw, top, left, bh, bw, fh, fw, oy, ox, flags = (int(v) for v in row)
    im = Image.fromarray(np.ascontiguousarray(img[:sh, :sw]))
    im = im.crop((left, top, left + bw, top + bh)).resize((fw, fh), Image.BICUBIC)
    im = im.crop((ox, oy, ox + OUT, oy + OUT))
    if flags & 1:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(im)
