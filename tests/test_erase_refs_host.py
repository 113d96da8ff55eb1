"""CPU tests that pin tests/erase_refs.py, the references the Random Erasing tests compare against: the numpy Philox4x32-10 by the published
known answers and by the host program's restatement of the device rounds, the uniform and Box-Muller maps, the keying of the noise by
position, and erase_ref's assignment order."""
import numpy as np
import torch

import erase_refs as R


def test_philox_known_answers():
    assert [int(w) for w in R.philox(0, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    ones = 2 ** 64 - 1
    assert [int(w) for w in R.philox(ones, ones, ones)] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    # the third published vector: counter = 243f6a88 85a308d3 13198a2e 03707344, key = a4093822 299f31d0
    got = R.philox(0x299f31d0a4093822, 0x0370734413198a2e, 0x85a308d3243f6a88)
    assert [int(w) for w in got] == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    # arrays broadcast, one result per element
    w = R.philox(5, np.arange(3, dtype=np.uint64).reshape(3, 1), np.arange(4, dtype=np.uint64).reshape(1, 4))
    assert w[0].shape == (3, 4) and w[0].dtype == np.uint32
    assert int(w[2][1, 3]) == int(R.philox(5, 1, 3)[2])


def test_uniform_and_box_muller():
    u = R.u01(np.array([0, 0xFF, 0x100, 0xFFFFFFFF], dtype=np.uint32))
    assert u.dtype == np.float32 and u[0] == u[1] == np.float32(0.5 / 2 ** 24) and u[2] == np.float32(1.5 / 2 ** 24)
    assert u[3] == np.float32(1.0)   # 2^24 - 0.5 rounds to 2^24 in fp32: r = 0, never log(0)
    rng = np.random.default_rng(0)
    w0, w1 = (rng.integers(0, 2 ** 32, 1 << 16, dtype=np.uint64).astype(np.uint32) for _ in range(2))
    a, b = R.normal_pair(w0, w1)
    a32, b32 = R.normal_pair(w0, w1, np.float32)
    assert a.dtype == np.float64 and a32.dtype == np.float32
    assert np.allclose(a * a + b * b, -2.0 * np.log(R.u01(w0).astype(np.float64)), rtol=1e-12, atol=1e-12)
    dev = max(np.abs(a32 - a).max(), np.abs(b32 - b).max())
    assert 0 < dev < 5e-6   # the fp32 formula's own error: what the GPU bound is 4 x of
    z = np.concatenate([a, b])
    assert abs(z.mean()) < 5 / np.sqrt(z.size) and abs(z.var() - 1) < 5 * np.sqrt(2 / z.size)


def test_noise_is_keyed_by_position():
    seed = 77
    p = R.pixel_noise(seed, 2)
    assert p.shape == (2, 3, 224, 224)
    for (n, c, y, x) in ((0, 0, 0, 0), (1, 2, 223, 223), (1, 1, 17, 6)):
        w = R.philox(seed, n, (c * 224 + y) * 56 + (x >> 2))
        pair = R.normal_pair(w[0], w[1]) if (x & 3) < 2 else R.normal_pair(w[2], w[3])
        assert p[n, c, y, x] == pair[x & 1]
    col = R.box_colours(seed, 2)
    w = R.philox(seed, 1, 2 ** 32 + 3)
    a, b = R.normal_pair(w[0], w[1])
    cc, _ = R.normal_pair(w[2], w[3])
    assert col.shape == (2, 4, 3) and tuple(col[1, 3]) == (float(a), float(b), float(cc))
    assert not np.array_equal(R.pixel_noise(seed + 1, 1), p[:1])
    assert R.noise_bound(seed, 2) < 2e-5


def test_erase_ref_assigns_in_order():
    from util.erasing import EraseDraw
    x = torch.arange(4 * 3 * 224 * 224, dtype=torch.float32).reshape(4, 3, 224, 224) + 1.0
    x[3, 0, 0, 0], x[3, 1, 5, 5], x[3, 2, 9, 9] = float("nan"), float("inf"), -0.0
    boxes = [[(0, 2, 0, 3)], [(30, 50, 30, 50), (60, 50, 60, 50)], [], []]
    d = EraseDraw("const", boxes)
    out = R.erase_ref(x, d)
    assert (out[0, :, :2, :3] == 0).all() and out[0].ne(x[0]).sum() == 3 * 6
    assert torch.equal(out[2:].view(torch.int32), x[2:].view(torch.int32))   # untouched images: the input's bits, NaN included
    hit = R.hit_map(d, 4)
    assert hit[1, 70, 70] == 1 and hit[1, 40, 40] == 0 and hit[1, 100, 100] == 1 and hit[1, 29, 29] == -1 and (hit[2:] == -1).all()
    r = EraseDraw("rand", boxes, seed=3)
    o = R.erase_ref_f64(x, r)
    col = R.box_colours(3, 4)
    assert (o[1, :, 70, 70] == col[1, 1]).all() and (o[1, :, 40, 40] == col[1, 0]).all() and (o[0, :, 1, 2] == col[0, 0]).all()
    p = EraseDraw("pixel", boxes, seed=3)
    o = R.erase_ref_f64(x, p)
    noise = R.pixel_noise(3, 4)
    assert (o[1, :, 30:80, 30:80] == noise[1, :, 30:80, 30:80]).all() and o[1, 0, 29, 29] == float(x[1, 0, 29, 29])
    # cube: both frames of clip 0 share the box, their units are clips
    c = EraseDraw("const", [[(1, 1, 1, 1)], []], cube=True, frames=2)
    hit = R.hit_map(c, 4)
    assert hit[0, 1, 1] == 0 and hit[1, 1, 1] == 0 and (hit[2:] == -1).all()
