"""Shared by tests/test_erase_host.py, tests/test_erase_refs_host.py and tests/test_gpu_erase.py: the torch / numpy references of the on-device
Random Erasing (dynamic-tuning_amd/csrc/erase.h).

The fused path is DEFINED as "the float path on the erased image": on the NORMALISED fp32 image, the boxes of the image's unit are assigned in
order (a later box overwrites an earlier one) with 0.0 (const), one N(0,1) colour per image, box and channel (rand) or one N(0,1) value per
pixel and channel (pixel).  The noise is Philox4x32-10 (restated here in numpy, pinned by the published known answers) through Box-Muller;
it is evaluated here in float64 AND in numpy float32 from the same words: the device computes the float32 formula with its own 1-2 ulp
logf / sinf / cosf, so it is compared with the float64 values within ``noise_bound`` = 4 x the largest float32-to-float64 deviation of
this formula over the words of the comparison itself."""
import numpy as np
import torch

IMG = 224
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
TWO_PI_F32 = np.float32(6.2831855)
_U32 = np.uint64(0xFFFFFFFF)


def philox(seed, subseq, offset):
    """Philox4x32-10, key = the 64-bit ``seed``, counter = (offset, subseq) as two 64-bit words; ``subseq`` / ``offset`` are integers or
    uint64 arrays (broadcast).  Returns four uint32 arrays."""
    subseq, offset = np.broadcast_arrays(np.asarray(subseq, dtype=np.uint64), np.asarray(offset, dtype=np.uint64))
    seed = int(seed) & (2 ** 64 - 1)
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    c = [offset & _U32, offset >> np.uint64(32), subseq & _U32, subseq >> np.uint64(32)]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]   # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _U32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _U32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [w.astype(np.uint32) for w in c]


def u01(w):
    """((w >> 8) + 0.5) * 2^-24 as the library forms it in fp32 (the sum rounds for odd values >= 2^23; the product is exact)."""
    return (((np.asarray(w, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)).astype(np.float32)


def normal_pair(w0, w1, dtype=np.float64):
    """Box-Muller on a pair of words: r = sqrt(-2 log u1), t = 6.2831855f u2, (r cos t, r sin t), every operation in ``dtype``."""
    u1, u2 = u01(w0).astype(dtype), u01(w1).astype(dtype)
    r = np.sqrt(dtype(-2.0) * np.log(u1))
    t = dtype(TWO_PI_F32) * u2
    return r * np.cos(t), r * np.sin(t)


def pixel_noise(seed, images, dtype=np.float64):
    """[images, 3, 224, 224]: the value of every pixel in ``pixel`` mode.  Philox(seed, subseq = image, offset = (c 224 + y) 56 + (x >> 2));
    words (0,1) -> x & 3 == 0, 1; words (2,3) -> x & 3 == 2, 3."""
    n = np.arange(images, dtype=np.uint64).reshape(-1, 1, 1, 1)
    c = np.arange(3, dtype=np.uint64).reshape(1, -1, 1, 1)
    y = np.arange(IMG, dtype=np.uint64).reshape(1, 1, -1, 1)
    x4 = np.arange(IMG // 4, dtype=np.uint64).reshape(1, 1, 1, -1)
    w = philox(seed, n + 0 * (c + y + x4), (c * np.uint64(IMG) + y) * np.uint64(IMG // 4) + x4 + 0 * n)
    a, b = normal_pair(w[0], w[1], dtype)
    cc, d = normal_pair(w[2], w[3], dtype)
    return np.stack([a, b, cc, d], axis=-1).reshape(images, 3, IMG, IMG)


def box_colours(seed, images, dtype=np.float64):
    """[images, 4, 3]: the colour of every (image, box, channel) in ``rand`` mode.  Philox(seed, subseq = image, offset = 2^32 + box); channel
    0 and 1 are the pair of words (0,1), channel 2 the first value of the pair of words (2,3)."""
    n = np.arange(images, dtype=np.uint64).reshape(-1, 1)
    box = np.arange(4, dtype=np.uint64).reshape(1, -1)
    w = philox(seed, n + 0 * box, np.uint64(1 << 32) + box + 0 * n)
    a, b = normal_pair(w[0], w[1], dtype)
    cc, _ = normal_pair(w[2], w[3], dtype)
    return np.stack([a, b, cc], axis=-1)


def noise_bound(seed, images):
    """4 x the largest deviation of the float32 evaluation from the float64 one over these images' own words (pixel and colour)."""
    d = np.abs(pixel_noise(seed, images, np.float32).astype(np.float64) - pixel_noise(seed, images)).max()
    e = np.abs(box_colours(seed, images, np.float32).astype(np.float64) - box_colours(seed, images)).max()
    return 4.0 * float(max(d, e))


def hit_map(draw, images):
    """int8 [images, 224, 224]: the index of the last box of the image's unit that contains the pixel, -1 outside every box."""
    out = np.full((images, IMG, IMG), -1, dtype=np.int8)
    for i in range(images):
        u = i // draw.frames if draw.cube else i
        if u >= draw.units:
            continue
        for k, (top, h, left, w) in enumerate(draw.boxes[u]):
            out[i, top:top + h, left:left + w] = k
    return out


def erase_ref_f64(xn, draw):
    """float64 [n,3,224,224]: the normalised fp32 images ``xn`` (values unchanged) with the boxes assigned in order; the noise in float64."""
    x = xn.detach().cpu().numpy()
    n = x.shape[0]
    out = x.astype(np.float64)
    hit = hit_map(draw, n)
    inside = np.broadcast_to((hit >= 0)[:, None], out.shape)
    if draw.mode == 1:
        out[inside] = 0.0
    elif draw.mode == 3:
        out[inside] = pixel_noise(draw.seed, n)[inside]
    else:
        col = box_colours(draw.seed, n)                                   # [n, 4, 3]
        for i in range(n):
            for k in range(4):
                m = hit[i] == k
                out[i][:, m] = col[i, k][:, None]
    return out


def erase_ref(xn, draw):
    """fp32 torch [n,3,224,224] on xn's device.  const: exact (the comparison is bit for bit; NaN, inf and -0.0 outside the boxes are the
    input's bits).  rand / pixel: the float64 noise rounded to fp32 (the device is compared within ``noise_bound``)."""
    out = xn.detach().clone()
    hit = torch.from_numpy(hit_map(draw, xn.shape[0]) >= 0).to(xn.device)
    inside = hit[:, None].expand_as(out)
    if draw.mode == 1:
        out[inside] = 0.0
    else:
        ref = torch.from_numpy(erase_ref_f64(xn, draw).astype(np.float32)).to(xn.device)
        out[inside] = ref[inside]
    return out
