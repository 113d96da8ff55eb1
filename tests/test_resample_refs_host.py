"""tests/resample_refs.py -- the numpy restatement the GPU tests compare the resample kernels with -- is Pillow's arithmetic: pinned to the
bytes Pillow wrote into tests/golden/resample/resample.npz (always), and to Pillow itself on 40 seeded random boxes where PIL imports.
Zero differing bytes in both.  Nothing here needs a GPU."""
import os

import numpy as np
import pytest

import resample_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "resample", "resample.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_the_restatement_writes_the_recorded_pillow_bytes(golden):
    src, rows, want = golden["small_src"], golden["small_rows"], golden["small_out"]
    assert src.shape == (6, 64, 64, 3) and rows.shape == (6, 11) and want.shape == (6, 224, 224, 3)
    got = R.resample_batch(src, rows)
    for i in range(6):
        assert int((got[i] != want[i]).sum()) == 0, (i, rows[i].tolist())
    assert rows[:, 10].tolist().count(1) == 2                                   # mirrored rows are in the set
    assert want[5].min() == 0 and want[5].max() == 255                          # the checkerboard clamps at both ends


def test_the_restatement_writes_the_recorded_evaluation_bytes(golden):
    row = golden["eval_row"]
    assert tuple(row[:2]) == (300, 400) and tuple(row[6:10]) == (256, 341, 16, 58)
    assert R.eval_geometry(300, 400) == tuple(golden["eval_sizes"].tolist()) == (256, 341, 16, 58)
    assert int((R.resample_image(golden["eval_src"], row) != golden["eval_out"]).sum()) == 0


def test_eval_geometry_is_torchvisions_rule():
    assert R.eval_geometry(400, 300) == (341, 256, 58, 16)
    assert R.eval_geometry(256, 256) == (256, 256, 16, 16)
    assert R.eval_geometry(500, 375) == (341, 256, 58, 16)
    assert R.eval_geometry(333, 500) == (256, 384, 16, 80)
    assert R.eval_geometry(480, 640) == (256, 341, 16, 58)                      # (341 - 224) / 2 = 58.5 rounds to even


def test_coefficients_of_the_identity_and_their_bounds():
    lo, cnt, k = R.coeffs(224, 224, np.arange(224))
    for xx in range(224):
        taps = {int(lo[xx]) + x: int(k[xx, x]) for x in range(int(cnt[xx]))}
        assert taps[xx] == 1 << 22 and all(v == 0 for p, v in taps.items() if p != xx)
    for n_in, n_out in ((512, 224), (560, 224), (490, 224), (1, 224), (8, 224), (300, 256), (400, 341)):
        lo, cnt, k = R.coeffs(n_in, n_out, np.arange(n_out))
        assert lo.min() >= 0 and cnt.min() >= 1 and cnt.max() <= R.KMAX - 1 and (lo + cnt).max() <= n_in
        assert np.all(np.abs(k.astype(np.int64).sum(axis=1) - (1 << 22)) <= R.KMAX)
        assert np.all(k[np.arange(R.KMAX)[None, :] >= cnt[:, None]] == 0)
    assert R.coeff_table((512, 512, 0, 0, 512, 490, 224, 224, 0, 0, 0)).shape == (2, 13, 224)


def _random_cases():
    rng = np.random.default_rng(20261020)
    cases = []
    for case in range(40):
        h, w = int(rng.integers(32, 513)), int(rng.integers(32, 513))
        if case % 10 == 2:
            h = w = 512
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if case % 4 == 1:       # saturated checkerboards: the overshoot clamps
            period = 1 + case // 8
            img = ((((np.add.outer(np.arange(h), np.arange(w)) // period) & 1) * 255).astype(np.uint8))[..., None].repeat(3, axis=2)
        bh, bw = int(rng.integers(1, h + 1)), int(rng.integers(1, w + 1))
        if case in (0, 20):
            bh, bw = (1, 1) if case == 0 else (int(rng.integers(1, h + 1)), 1)      # width-1 boxes
        if case % 10 == 2:
            bh = bw = 512                                                            # scale 2.29 from a 512 source
        if case % 10 == 3:
            bh = bw = min(224, h, w)                                                 # identity where the source allows it
        bh, bw = min(bh, 560), min(bw, 560)
        top, left = int(rng.integers(0, h - bh + 1)), int(rng.integers(0, w - bw + 1))
        cases.append((img, (h, w, top, left, bh, bw, 224, 224, 0, 0, case & 1)))
    return cases


def test_the_restatement_equals_pillow_on_random_boxes():
    pytest.importorskip("PIL")
    cases = _random_cases()
    assert any(r[4] == 1 and r[5] == 1 for _, r in cases) and any(r[4] == 224 and r[5] == 224 for _, r in cases)
    assert any(r[4] == 512 and r[5] == 512 for _, r in cases)
    for img, row in cases:
        assert int((R.resample_image(img, row) != R.pillow_row(img, row)).sum()) == 0, row
    img = np.random.default_rng(3).integers(0, 256, (300, 400, 3), dtype=np.uint8)
    row = (300, 400, 0, 0, 300, 400) + R.eval_geometry(300, 400) + (0,)
    assert int((R.resample_image(img, row) != R.pillow_row(img, row)).sum()) == 0
