"""tests/clip_resample_refs.py -- the numpy restatement the GPU tests compare the clip resample kernel with -- is torch's float bilinear
arithmetic: pinned to the fp32 values the reference's own functions wrote into tests/golden/resample/clip_resample.npz, and to live
torch.nn.functional.interpolate on seeded random boxes.  Zero differing bit patterns in both.  Nothing here needs a GPU."""
import os

import numpy as np
import pytest

import clip_resample_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "resample", "clip_resample.npz")


def _diff(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    assert a.shape == b.shape, (a.shape, b.shape)
    return int((a.view(np.int32) != b.view(np.int32)).sum())


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _norm(golden):
    return tuple(golden["norm"][0].tolist()), tuple(golden["norm"][1].tolist())


def test_the_restatement_writes_the_references_recorded_bits(golden):
    src, rows, frames, idx = golden["px_src"], golden["px_rows"], golden["px_frames"], golden["px_index"]
    assert src.shape == (5, 2, 64, 64, 3) and rows.shape == (7, 12) and idx[0] == 0 and idx[-1] == 223
    norm = _norm(golden)
    got = R.resample_batch(src, rows, norm)
    assert got.shape == (7, 2, 3, 224, 224)
    assert _diff(got[0, 0], golden["px_full"]) == 0
    for i in range(7):
        t = int(frames[i])
        assert _diff(got[i, :t][:, :, idx][:, :, :, idx], golden["px_samples"][i, :t]) == 0, (i, rows[i].tolist())
    assert rows[:, 10].tolist().count(1) >= 2 and sorted(set(rows[:, 11].tolist())) == [0, 1, 2, 3, 4]   # mirrored rows, every source
    assert any(tuple(r[6:8]) == (224, 224) and tuple(r[4:6]) != tuple(r[0:2]) for r in rows.tolist())   # random resized crops
    assert any(r[6] > 224 and r[7] > 224 for r in rows.tolist())                                        # scale jitter


def test_the_restatement_writes_the_recorded_evaluation_views(golden):
    rows, idx = golden["eval_rows"], golden["px_index"]
    assert [tuple(r[6:10]) for r in rows.tolist()] == [(224, 298, 0, 0), (224, 298, 0, 37), (224, 298, 0, 74)] and set(rows[:, 11].tolist()) == {0}
    got = R.resample_batch(golden["eval_src"][None], rows, _norm(golden))
    assert got.shape == (3, 1, 3, 224, 224)
    assert _diff(got[:, :, :, idx][:, :, :, :, idx], golden["eval_samples"][:, :1]) == 0
    assert not golden["eval_samples"][:, 1].any()


def _cases():
    """(clip, row) of about 20 seeded size pairs: up- and downscaling, scale 1, 1-pixel boxes, boxes flush with each corner, windows in
    every corner of a larger `full`, scales up to 18."""
    rng = np.random.default_rng(20261020)
    rows = [(64, 64, 37, 11, 1, 1, 224, 224, 0, 0, 0), (64, 64, 5, 9, 1, 40, 224, 224, 0, 0, 1), (64, 64, 5, 9, 40, 1, 224, 224, 0, 0, 0),
            (300, 320, 10, 20, 224, 224, 224, 224, 0, 0, 1),                      # scale 1
            (240, 320, 0, 0, 240, 320, 224, 298, 0, 37, 0), (128, 171, 0, 0, 128, 171, 224, 299, 0, 75, 0),
            (480, 640, 0, 0, 480, 640, 258, 344, 34, 120, 1), (256, 340, 0, 0, 256, 340, 241, 320, 17, 0, 0),
            (64, 48, 0, 0, 20, 30, 224, 224, 0, 0, 0), (64, 48, 0, 48 - 25, 17, 25, 224, 224, 0, 0, 1),       # flush top-left, top-right
            (64, 48, 64 - 30, 0, 30, 22, 224, 224, 0, 0, 0), (33, 57, 33 - 21, 57 - 40, 21, 40, 224, 224, 0, 0, 0),   # bottom-left, bottom-right
            (48, 64, 20, 30, 8, 10, 224, 224, 0, 0, 0),                           # scale 1 / 28
            (512, 700, 0, 0, 512, 700, 224, 224, 0, 0, 0), (1024, 32, 0, 0, 1024, 32, 7168, 224, 6944, 0, 0),
            (4032, 30, 0, 0, 4032, 30, 224, 300, 0, 76, 1),                       # scale 18
            (96, 64, 0, 0, 96, 64, 336, 224, 112, 0, 0), (17, 23, 0, 0, 17, 23, 224, 303, 0, 39, 0),
            (225, 400, 3, 5, 201, 333, 257, 258, 33, 34, 0), (100, 100, 0, 0, 100, 100, 1000, 1000, 776, 776, 1)]
    cases = []
    for i, row in enumerate(rows):
        clip = rng.integers(0, 256, (1 + (i & 1), row[0], row[1], 3), dtype=np.uint8)
        if i % 5 == 4:   # saturated checkerboard
            clip[:] = (((np.add.outer(np.arange(row[0]), np.arange(row[1])) & 1) * 255).astype(np.uint8))[None, :, :, None]
        cases.append((clip, row))
    return cases


def test_the_restatement_equals_live_torch_interpolate_bit_for_bit():
    cases = _cases()
    assert len(cases) >= 20
    norms = [None, ((0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)), ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))]
    total = 0
    for i, (clip, row) in enumerate(cases):
        norm = norms[i % 3]
        got, want = R.resample_clip(clip, row, norm), R.torch_row(clip, row, norm)
        assert _diff(got, want) == 0, row
        total += got.size
    assert total > 3_000_000


def test_fma32_is_a_single_rounding():
    """Where the fp64 sum is exact fma32 is its rounding; where it is not, the tie cases that double rounding gets wrong come out right."""
    a, b = np.float32(1.0 + 2.0 ** -23), np.float32(1.0 + 2.0 ** -23)       # a * b = 1 + 2^-22 + 2^-46
    c = np.float32(2.0 ** -24)                                              # exact sum 1 + 2^-22 + 2^-24 + 2^-46: just above a tie of fp32
    assert R.fma32(a, b, c) == np.float32(1.0 + 2.0 ** -22 + 2.0 ** -23)    # rounds up; a * b rounded first would give the tie -> even -> down
    assert np.float32(np.float32(a * b) + c) == np.float32(1.0 + 2.0 ** -22)
    big = np.float32(2.0 ** 30)
    tiny = np.float32(1.0 + 2.0 ** -23)
    got = R.fma32(tiny, tiny, big)                                          # fp64 cannot hold 2^30 + 1 + 2^-22 + 2^-46: round to odd keeps the sticky bit
    assert got == big and got.dtype == np.float32
    rng = np.random.default_rng(3)
    x, y, z = (rng.standard_normal(100000).astype(np.float32) for _ in range(3))
    import torch
    want = torch.addcmul(torch.from_numpy(z).double(), torch.from_numpy(x).double(), torch.from_numpy(y).double())
    exact = (want - torch.from_numpy(z).double()) == torch.from_numpy(x).double() * torch.from_numpy(y).double()
    got = R.fma32(x, y, z)
    assert np.array_equal(got[exact.numpy()], want.float().numpy()[exact.numpy()])


def test_axis_properties():
    for n_in, n_out in ((224, 224), (1, 224), (8, 224), (300, 224), (400, 298), (4032, 224), (57, 386)):
        i0, i1, l0, l1 = R.axis(n_in, n_out, np.arange(n_out))
        assert i0.min() >= 0 and i1.max() <= n_in - 1 and np.all(i1 - i0 <= 1) and np.all(np.diff(i0) >= 0) and np.all(np.diff(i1) >= 0)
        assert l1.min() >= 0 and l1.max() <= 1 and l0.dtype == l1.dtype == np.float32
        if n_in == n_out:
            assert np.array_equal(i0, np.arange(n_out)) and not l1.any()
    assert R.coeff_table((64, 64, 0, 0, 64, 64, 224, 224, 0, 0, 0, 0)).shape == (2, 4, 224)
    tab = R.norm_table()
    assert tab.shape == (3, 256) and tab.dtype == np.float32 and tab[0, 0] == np.float32(np.float32(0 - np.float32(0.485)) / np.float32(0.229))
