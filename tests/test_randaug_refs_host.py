"""CPU tests of tests/randaug_refs.py, the numpy restatement of the twelve RandAugment operations that the GPU tests compare the kernels
with: it equals the reference's recorded output (tests/golden/randaug/randaug.npz, made by the reference's own op functions) byte for byte
-- every case, the observed tables, the Contrast constants, the four-layer chain -- and, where Pillow of the recorded version is
importable, live Pillow on seeded random frames of 20 sizes for every operation.  No tolerance anywhere."""
import os

import numpy as np
import pytest

import randaug_refs as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "randaug", "randaug.npz")
SIZES = [(1, 1), (2, 5), (3, 3), (300, 400), (5, 2), (1, 7), (3, 4), (4, 3), (33, 57), (48, 64), (64, 40), (7, 7), (16, 16), (2, 2), (10, 3),
         (3, 10), (17, 31), (31, 17), (64, 64), (9, 100)]


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


def _rows(g, prefix):
    return [R.row(int(o), int(i), float(f), tuple(c.tolist()), int(fl)) for o, i, f, c, fl in zip(
        g[prefix + "_op"], g[prefix + "_iarg"], g[prefix + "_factor"], g[prefix + "_coeffs"], g[prefix + "_filter"])]


def _same(got, want, what):
    bad = got != want
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8 and not bad.any(), "%s: %d bytes differ, first at %s" % (
        what, int(bad.sum()), np.argwhere(bad)[0].tolist() if bad.any() else None)


def test_the_golden_file_covers_what_the_tests_rely_on(g):
    assert len(SIZES) == 20 and len(set(SIZES)) == 20
    assert sorted(set(g["case_row_op"].tolist())) == list(range(12))                      # every device operation
    aff = g["case_row_op"] == R.AFFINE
    assert set(g["case_row_filter"][aff].tolist()) == {R.BILINEAR, R.BICUBIC}
    names = g["case_name"].tolist()
    assert names.count("Rotate") >= 3 and ("Posterize", 0) in zip(names, g["case_row_iarg"].tolist()) and ("Solarize", 256) in zip(names, g["case_row_iarg"].tolist())
    assert g["px_sizes"].tolist() == [[48, 64], [64, 40], [33, 57]] and g["px_src"].shape == (3, 2, 64, 64, 3)
    assert os.path.getsize(GOLDEN) < (1 << 20)
    # the translate that moves most of the frame out leaves mostly the fill colour
    k = [i for i, n in enumerate(names) if n == "TranslateXRel" and g["case_row_coeffs"][i][2] > 30][0]
    h, w = g["px_sizes"][g["case_src"][k]]
    assert (g["case_out"][k][:, :h, :w] == 128).all(axis=-1).mean() > 0.85


def test_the_restatement_equals_the_references_recorded_pixels(g):
    rows = _rows(g, "case_row")
    for k, r in enumerate(rows):
        i = int(g["case_src"][k])
        h, w = (int(v) for v in g["px_sizes"][i])
        want = g["case_out"][k]
        assert (want[:, h:] == 0xFF).all() and (want[:, :, w:] == 0xFF).all()
        for f in range(2):
            _same(R.apply_row(np.ascontiguousarray(g["px_src"][i, f, :h, :w]), r), want[f, :h, :w], "case %d %s frame %d" % (k, g["case_name"][k], f))


def test_apply_batch_runs_the_chain_and_leaves_the_padding(g):
    rows = _rows(g, "chain_row")
    assert len(rows) == 4
    got = R.apply_batch(g["px_src"][2:3], [(33, 57)], rows, 4)
    _same(got[0], g["chain_out"], "the four-layer chain")
    assert (got[0, :, 33:] == 0xFF).all() and (got[0, :, :, 57:] == 0xFF).all()
    # two units with different sequences, one layer skipped
    both = R.apply_batch(g["px_src"][1:3], [(64, 40), (33, 57)], [R.row(R.INVERT), R.row(R.IDENTITY), R.row(R.IDENTITY), R.row(R.INVERT)], 2)
    assert np.array_equal(both[0, :, :64, :40], 255 - g["px_src"][1, :, :64, :40]) and np.array_equal(both[1, :, :33, :57], 255 - g["px_src"][2, :, :33, :57])
    assert (both[0, :, :, 40:] == 0xFF).all()


def test_tables_and_contrast_constants_equal_what_pillow_used(g):
    rows = _rows(g, "case_row")
    for n, k in enumerate(g["tab_case"]):
        op = rows[k][0]
        assert op in (R.AUTO_CONTRAST, R.EQUALIZE)
        i = int(g["case_src"][k])
        h, w = (int(v) for v in g["px_sizes"][i])
        for f in range(2):
            hist = R.histograms(g["px_src"][i, f, :h, :w])
            assert np.array_equal(hist, g["tab_hist"][n, f])
            t, seen = R.table(op, 0, hist), g["tab_lut"][n, f]
            assert (seen >= 0).any() and np.array_equal(t[seen >= 0], seen[seen >= 0].astype(np.uint8)), (k, f)
    for n, k in enumerate(g["con_case"]):
        for f in range(2):
            assert R.contrast_mean(g["con_hist"][n, f]) == int(g["con_mean"][n, f])
    # the clamp of Equalize binds: a frame with one dominant value at the bottom
    hist = np.zeros(256, dtype=np.int64)
    hist[[0, 200, 255]] = [10, 3000, 62]
    assert R.equalize_table(hist)[255] == 255 and (11 // 2 + 3010) // 11 > 255   # step = (3072 - 62) // 255 = 11
    assert np.array_equal(R.table(R.POSTERIZE, 0, None), np.zeros((3, 256), np.uint8)) and np.array_equal(R.table(R.POSTERIZE, 8, None)[0], np.arange(256))
    assert np.array_equal(R.table(R.SOLARIZE, 256, None)[1], np.arange(256)) and np.array_equal(R.table(R.SOLARIZE, 0, None)[2], 255 - np.arange(256))


def _pillow_cases(h, w):
    """[(row, function of a PIL image)] for every operation"""
    from PIL import Image, ImageEnhance, ImageOps
    fill = (128, 128, 128)

    def point_add(im, add):
        lut = [min(255, i + add) if i < 128 else i for i in range(256)]
        return im.point(lut * 3)
    cases = [(R.row(R.INVERT), ImageOps.invert), (R.row(R.AUTO_CONTRAST), ImageOps.autocontrast), (R.row(R.EQUALIZE), ImageOps.equalize),
             (R.row(R.IDENTITY), lambda im: im.copy())]
    for a in (0, 100, 128, 256):
        cases.append((R.row(R.SOLARIZE, a), lambda im, a=a: ImageOps.solarize(im, a)))
    for a in (0, 60, 110):
        cases.append((R.row(R.SOLARIZE_ADD, a), lambda im, a=a: point_add(im, a)))
    for a in (0, 1, 4, 7):
        cases.append((R.row(R.POSTERIZE, a), lambda im, a=a: ImageOps.posterize(im, a)))
    for f in (0.1, 0.37, 1.0, 1.63, 1.9, 0.0):
        for op, enh in ((R.BRIGHTNESS, ImageEnhance.Brightness), (R.COLOR, ImageEnhance.Color), (R.CONTRAST, ImageEnhance.Contrast), (R.SHARPNESS, ImageEnhance.Sharpness)):
            cases.append((R.row(op, 0, f), lambda im, f=f, enh=enh: enh(im).enhance(f)))
    for filt in (Image.BILINEAR, Image.BICUBIC):
        for c in ((1, 0.21, 0, 0, 1, 0), (1, -0.3, 0, 0, 1, 0), (1, 0, 0, 0.21, 1, 0), (1, 0, 0, -0.3, 1, 0), (1, 0, 0.3 * w, 0, 1, 0), (1, 0, -0.45 * w, 0, 1, 0),
                  (1, 0, 0, 0, 1, 0.2 * h), (1, 0, 0, 0, 1, -0.45 * h), (1, 0, 0.9 * w, 0, 1, 0)):
            cases.append((R.row(R.AFFINE, coeffs=c, filt=filt), lambda im, c=c, filt=filt: im.transform(im.size, Image.AFFINE, c, resample=filt, fillcolor=fill)))
        for d in (21.0, -13.7, 30.0, -0.5):
            cases.append((R.row(R.AFFINE, coeffs=R.rotate_coeffs(d, h, w), filt=filt), lambda im, d=d, filt=filt: im.rotate(d, resample=filt, fillcolor=fill)))
    return cases


def test_the_restatement_equals_live_pillow_of_the_recorded_version(g):
    PIL = pytest.importorskip("PIL")
    if PIL.__version__ != str(g["pillow"]):
        pytest.skip("Pillow %s here, the golden was recorded with %s" % (PIL.__version__, g["pillow"]))
    from PIL import Image
    rng = np.random.default_rng(0)
    ops = set()
    for (h, w) in SIZES:
        fr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if h * w > 50:
            fr[..., 2] = rng.integers(100, 140, (h, w))
        img = Image.fromarray(fr)
        for r, fn in _pillow_cases(h, w):
            _same(R.apply_row(fr, r), np.asarray(fn(img)), "%d x %d %s %r" % (h, w, R.OP_NAMES[r[0]], r[1:5]))
            ops.add(r[0])
    assert ops == set(range(12))
    assert R.rotate_coeffs(0.0, 5, 7) is None and R.rotate_coeffs(360.0, 5, 7) is None
