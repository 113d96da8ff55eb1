"""numpy fp32 restatement of the device clip pipeline (csrc/resample_clip.h): torch.nn.functional.interpolate(mode='bilinear',
align_corners=False) on normalised fp32 frames, applied to a box that acts as the image, a 224 x 224 window of the result, mirrored or not.

Every fp32 operation is one numpy float32 operation, except the FUSED multiply-adds, which numpy does not have: ``fma32`` forms the product
of the two fp32 factors in fp64 (exact: 24 + 24 bits), adds the fp32 addend with an error-free TwoSum, rounds the fp64 sum TO ODD where it
was inexact and only then rounds to fp32 -- with 53 >= 2 * 24 + 2 bits that is the single rounding of a true fma, with no double rounding.
tests/test_clip_resample_refs_host.py pins this file to the reference's recorded output and to live torch, bit for bit."""
import numpy as np

OUT = 224
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
f32 = np.float32


def fma32(a, b, c):
    """fp32 fma(a, b, c), correctly rounded, elementwise."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    a, b, c = np.broadcast_arrays(a, b, c)
    p = a * b                                   # exact
    s = p + c
    bb = s - p                                  # TwoSum: s + e = p + c exactly
    e = (p - (s - bb)) + (c - bb)
    bits = s.copy().view(np.int64)
    toward = np.where(e > 0, np.inf, -np.inf)
    other = np.nextafter(s, toward)
    odd = np.where((e != 0) & ((bits & 1) == 0), other, s)
    return odd.astype(np.float32)


def axis(n_in, n_out, d):
    """(i0, i1, l0, l1) of positions ``d`` of an axis that resizes ``n_in`` box pixels to ``n_out``: clip_axis of csrc/resample_clip.h."""
    d = np.asarray(d, dtype=np.int64)
    scale = f32(n_in) / f32(n_out)
    real = fma32(scale, d.astype(np.float32) + f32(0.5), f32(-0.5))
    real = np.where(real > 0, real, f32(0)).astype(np.float32)
    i0 = np.minimum(real.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = np.clip(real - i0.astype(np.float32), f32(0), f32(1)).astype(np.float32)
    l0 = (f32(1) - l1).astype(np.float32)
    return i0, i1, l0, l1


def lerp(w0, v0, w1, v1):
    """clip_lerp: fma(w0, v0, w1 * v1) with the second product rounded on its own."""
    p = (np.asarray(w1, dtype=np.float32) * np.asarray(v1, dtype=np.float32)).astype(np.float32)
    return fma32(w0, v0, p)


def norm_table(norm=None):
    """fp32 [3, 256]: ((float)u / 255 - mean[c]) / std[c], three correctly rounded fp32 operations (csrc/input_norm.h)."""
    mean, std = IMAGENET if norm is None else norm
    u = np.arange(256, dtype=np.float32) / f32(255)
    return np.stack([((u - f32(mean[c])) / f32(std[c])).astype(np.float32) for c in range(3)])


def coeff_table(row):
    """int32 [2, 4, 224]: what dyt_resample_clip_coeffs writes for a valid row."""
    sh, sw, top, left, bh, bw, fh, fw, oy, ox = (int(v) for v in row[:10])
    out = np.zeros((2, 4, OUT), dtype=np.int32)
    for a, (n_in, n_out, off) in enumerate(((bh, fh, oy), (bw, fw, ox))):
        i0, i1, l0, l1 = axis(n_in, n_out, off + np.arange(OUT))
        out[a, 0], out[a, 1], out[a, 2], out[a, 3] = i0, i1, l0.view(np.int32), l1.view(np.int32)
    return out


def resample_clip(clip, row, norm=None):
    """fp32 [T, 3, 224, 224] of one source clip uint8 [T, Hs, Ws, 3] (padded) and one row
    (src_h, src_w, top, left, box_h, box_w, full_h, full_w, off_y, off_x, flags[, src])."""
    sh, sw, top, left, bh, bw, fh, fw, oy, ox, flags = (int(v) for v in row[:11])
    clip = np.asarray(clip)
    assert clip.dtype == np.uint8 and clip.ndim == 4 and clip.shape[3] == 3
    assert 1 <= bh and 1 <= bw and top >= 0 and left >= 0 and top + bh <= sh <= clip.shape[1] and left + bw <= sw <= clip.shape[2]
    tab = norm_table(norm)
    box = clip[:, top:top + bh, left:left + bw]
    v = np.stack([tab[c][box[..., c]] for c in range(3)], axis=1)             # [T, 3, bh, bw] normalised fp32
    y0, y1, ly0, ly1 = axis(bh, fh, oy + np.arange(OUT))
    x0, x1, lx0, lx1 = axis(bw, fw, ox + np.arange(OUT))
    r = lerp(lx0, v[..., x0], lx1, v[..., x1])                                # [T, 3, bh, 224]: columns first
    out = lerp(ly0[:, None], r[:, :, y0, :], ly1[:, None], r[:, :, y1, :])    # [T, 3, 224, 224]
    return np.ascontiguousarray(out[..., ::-1]) if flags & 1 else out


def resample_batch(src, rows, norm=None):
    """fp32 [units, T, 3, 224, 224] of a batch uint8 [B, T, Hs, Ws, 3] and clip rows (12 words: the last names the source clip)."""
    return np.stack([resample_clip(src[int(r[11])], r, norm) for r in rows])


def torch_row(clip, row, norm=None):
    """The same through torch, as the reference's datasets compute it: ``frames.float() / 255.``, ``(frames - mean) / std``, the box,
    ``interpolate(..., 'bilinear', align_corners=False)`` to the full size, the window, the flip -> fp32 [T, 3, 224, 224]."""
    import torch
    sh, sw, top, left, bh, bw, fh, fw, oy, ox, flags = (int(v) for v in row[:11])
    mean, std = IMAGENET if norm is None else norm
    frames = torch.as_tensor(np.ascontiguousarray(clip)).float() / 255.
    frames = (frames - torch.tensor(mean, dtype=torch.float32)) / torch.tensor(std, dtype=torch.float32)
    frames = frames.permute(3, 0, 1, 2)[:, :, top:top + bh, left:left + bw]   # C, T, H, W
    full = torch.nn.functional.interpolate(frames, size=(fh, fw), mode="bilinear", align_corners=False)
    win = full[:, :, oy:oy + OUT, ox:ox + OUT]
    if flags & 1:
        win = win.flip(dims=(-1,))
    return win.permute(1, 0, 2, 3).contiguous().numpy()
