"""CPU tests of the device crop / resize at any downscale (dyt_resample_wide_u8, dyt_resample_wide_scratch_bytes, dyt_resample_wide_coeffs;
util.crop's ``any_scale`` and ``DeviceResize``):

  1. the restatement is Pillow: tests/resample_wide_refs.py equals Pillow's recorded bytes (tests/golden/resample/resample_wide.npz), Pillow
     itself on seven geometries up to 4096 x 4096 where PIL imports, and tests/resample_refs.py exactly wherever the 11-tap restatement
     applies;
  2. the header is the restatement: dynamic-tuning_amd/csrc/resample_wide.h is walked by tools/resample_wide_check.cpp, built with the host
     compiler, and its coefficients equal the restatement's integer for integer -- and the 11-tap header's where that one applies;
  3. geometry and refusals: what ``any_scale=True`` takes and the default still refuses, the same boxes from the same seed, DeviceResize's
     rows, every other refusal of row_error, the entries' refusals without a device, the loops' argument check.

Nothing here needs a GPU; a missing compiler is a failure."""
import ctypes
import inspect
import os
import re
import shutil
import struct
import subprocess
import types

import numpy as np
import pytest
import torch

import resample_refs as R
import resample_wide_refs as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dynamic-tuning_amd", "csrc")
ENTRIES = {"dyt_resample_wide_u8", "dyt_resample_wide_scratch_bytes", "dyt_resample_wide_coeffs"}
GOLDEN = os.path.join(ROOT, "tests", "golden", "resample", "resample_wide.npz")
NARROW_GOLDEN = os.path.join(ROOT, "tests", "golden", "resample", "resample.npz")
PER_IMAGE = 2 * 77 * 224 * 4      # bytes of coefficient tables per image
T = (224, 224, 0, 0)
# (in, out, position) of test_crop_host.py's comparison of the 11-tap header with its restatement
NARROW_TUPLES = ((512, 224, 100), (512, 224, 0), (512, 224, 223), (490, 224, 57), (8, 224, 3), (10, 224, 223), (1, 224, 17), (224, 224, 5),
                 (300, 256, 16), (300, 256, 239), (400, 341, 58), (400, 341, 281), (560, 224, 111))


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8, (what, got.shape, want.shape)
    assert int((got != want).sum()) == 0, "%s: %d of %d bytes differ" % (what, int((got != want).sum()), got.size)


# ---- 1. the restatement is Pillow ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("case", ["wide", "tall", "eval", "noaug", "box"])
def test_the_restatement_writes_the_recorded_pillow_bytes(golden, case):
    h, w = (int(v) for v in golden[case + "_size"])
    row = tuple(int(v) for v in golden[case + "_row"])
    assert 2 * row[4] > 5 * row[6] or 2 * row[5] > 5 * row[7]      # beyond the 11 taps on an axis
    _same(W.resample_image(W.pattern(h, w), row), golden[case + "_out"], case)


def test_the_golden_cases_are_the_pipelines():
    g = np.load(GOLDEN)
    assert tuple(g["eval_row"][6:10]) == R.eval_geometry(600, 640, resize=224) == (224, 238, 0, 7)
    assert tuple(g["noaug_row"]) == (375, 1242, 0, 0, 375, 1242, 224, 224, 0, 0, 0)
    assert int(g["wide_row"][10]) == 1 and tuple(g["box_row"][2:6]) == (3, 5, 33, 1201)
    p = W.pattern(40, 1500)
    assert p.dtype == np.uint8 and p.shape == (40, 1500, 3) and p.min() == 0 and p.max() == 255
    assert len(np.unique(p[:, 750:937])) == 256      # the band of noise


def _pillow_geometries():
    """(source shape, row, checkerboard period) of the seven geometries; the sources are made by the test.  The checkerboards' squares are
    a few output pixels wide, so that the filter's overshoot reaches both clamps."""
    ev = R.eval_geometry(1200, 1600)
    return [((1200, 1600), (1200, 1600, 0, 0, 1200, 1600) + ev + (0,), 12),               # 1600 x 1200 to short side 256
            ((1400, 1500), (1400, 1500, 101, 77, 1100, 1300) + T + (1,), 16),            # a mirrored 1300 x 1100 box
            ((695, 1024), (695, 1024, 0, 0, 695, 1024) + T + (0,), 12),                  # 1024 x 695 to 224 x 224
            ((600, 4096), (600, 4096, 0, 0, 600, 4096) + T + (0,), 48),                  # strips
            ((4096, 300), (4096, 300, 0, 0, 4096, 300) + T + (0,), 48),
            ((4096, 4096), (4096, 4096, 0, 0, 4096, 4096) + T + (0,), 64),
            ((32, 32), (32, 32, 0, 0, 32, 32) + T + (0,), 1)]                            # an upscale


@pytest.mark.parametrize("index", range(7))
def test_the_restatement_equals_pillow_on_the_seven_geometries(index):
    pytest.importorskip("PIL")
    (h, w), row, period = _pillow_geometries()[index]
    rng = np.random.default_rng(20261021 + index)
    for what, img in (("noise", rng.integers(0, 256, (h, w, 3), dtype=np.uint8)), ("checkerboard", W.checkerboard(h, w, period))):
        want = R.pillow_row(img, row)
        assert what == "noise" or (want.min() == 0 and want.max() == 255), (row, int(want.min()), int(want.max()))
        _same(W.resample_image(img, row), want, "%s %r" % (what, row))


def test_the_tap_counts_and_the_accumulator_bound():
    lo, cnt, k = W.coeffs(4096, 224, np.arange(224))
    assert W.ksize(4096, 224) == 75 == W.KMAX and int(cnt.max()) == 74 and k.shape == (224, 75)
    assert (1 << 21) + 255 * int(np.abs(k.astype(np.int64)).sum(axis=1).max()) < 2 ** 31       # int32 never wraps
    assert np.all(np.diff(lo) >= 0) and np.all(np.diff(lo + cnt) >= 0)                          # both bounds grow with the position
    for n_in, n_out in ((561, 224), (700, 256), (1242, 224), (375, 224), (32, 224), (1, 224), (4096, 4096)):
        lo, cnt, k = W.coeffs(n_in, n_out, np.arange(n_out))
        assert lo.min() >= 0 and cnt.min() >= 1 and cnt.max() <= W.ksize(n_in, n_out) - 1 and (lo + cnt).max() <= n_in
        assert np.all(k[np.arange(k.shape[1])[None, :] >= cnt[:, None]] == 0)
    assert W.coeff_table((4096, 8, 0, 0, 4096, 8) + T + (0,)).shape == (2, 77, 224)


def test_where_both_apply_the_two_restatements_agree_exactly():
    for n_in, n_out, xx in NARROW_TUPLES:
        a, b = R.coeffs(n_in, n_out, [xx]), W.coeffs(n_in, n_out, [xx], width=W.KMAX)
        assert int(a[0][0]) == int(b[0][0]) and int(a[1][0]) == int(b[1][0])
        assert b[2][0, :R.KMAX].tolist() == a[2][0].tolist() and not b[2][0, R.KMAX:].any()
    row = (512, 512, 0, 22, 512, 490) + T + (0,)
    assert np.array_equal(W.coeff_table(row)[:, :13], R.coeff_table(row)) and not W.coeff_table(row)[:, 13:].any()
    g = np.load(NARROW_GOLDEN)
    _same(W.resample_batch(g["small_src"], g["small_rows"]), g["small_out"], "the 11-tap golden rows")
    _same(W.resample_image(g["eval_src"], g["eval_row"]), g["eval_out"], "the 11-tap evaluation case")
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (300, 600, 3), dtype=np.uint8)
    for row in ((300, 600, 0, 40, 300, 560) + T + (1,), (300, 600, 0, 0, 300, 400, 256, 341, 16, 58, 0), (300, 600, 250, 500, 9, 7) + T + (0,)):
        _same(W.resample_image(img, row), R.resample_image(img, row), repr(row))


# ---- header, binding, libraries --------------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "dyt_hip.h")).read()


def _args(name, ret="int"):
    m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (ret, name), _header())
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_binding_and_both_libraries_have_the_entries():
    import _lib
    assert _args("dyt_resample_wide_u8") == _args("dyt_resample_u8")      # the same call: a draw uploads the same way for both routes
    assert _args("dyt_resample_wide_scratch_bytes", "int64_t") == ["int batch", "int src_h"]
    assert _args("dyt_resample_wide_coeffs") == _args("dyt_resample_coeffs")
    assert ENTRIES <= set(_lib.SYMBOLS) and ENTRIES <= _lib.OPTIONAL_SYMBOLS   # discovered by symbol
    assert [len(_lib.SYMBOLS[n][1]) for n in ("dyt_resample_wide_u8", "dyt_resample_wide_scratch_bytes", "dyt_resample_wide_coeffs")] == [10, 2, 7]
    for fp16 in (False, True):
        L = _lib.lib(fp16=fp16)
        assert L.dyt_version() == 5
        assert all(hasattr(L, n) for n in ENTRIES)
        assert L.dyt_resample_wide_scratch_bytes(1, 1) == PER_IMAGE + 672 and L.dyt_resample_wide_scratch_bytes(4, 700) == 4 * (PER_IMAGE + 700 * 672)
        assert L.dyt_resample_wide_scratch_bytes(128, 4096) == 128 * (PER_IMAGE + 4096 * 672)
        assert L.dyt_resample_wide_scratch_bytes(0, 64) == 0 and L.dyt_resample_wide_scratch_bytes(4, 0) == 0 and L.dyt_resample_wide_scratch_bytes(4, 4097) == 0
        assert L.dyt_resample_scratch_bytes(128) == 128 * 23296      # the 11-tap route's scratch is what it was


def _refuses_without(monkeypatch, _lib, symbol, call, named=None):
    """``call`` raises a DyTError naming ``symbol`` (or ``named``) and "rebuild it" when the loaded library is one that lacks ``symbol``."""
    real = _lib.lib()
    stand_in = types.SimpleNamespace(**{n: getattr(real, n) for n in _lib.SYMBOLS if n != symbol and hasattr(real, n)})
    monkeypatch.setattr(_lib, "lib", lambda fp16=False: stand_in)
    with pytest.raises(_lib.DyTError) as e:
        call()
    assert (named or symbol) in str(e.value) and "rebuild it" in str(e.value), str(e.value)


def test_python_refuses_by_name_when_the_library_lacks_the_entries(monkeypatch):
    import _lib
    import runtime
    src = inspect.getsource(runtime.DyTEngine.resample)
    assert "dyt_resample_wide" in src and "hasattr(" in src and "rebuild it" in src
    # the wrappers delegate to one body: called with a library that lacks the symbol, before any argument is looked at
    _refuses_without(monkeypatch, _lib, "dyt_resample_wide_u8", lambda: _lib.resample_wide_u8(None, None))
    _refuses_without(monkeypatch, _lib, "dyt_resample_wide_scratch_bytes", lambda: _lib.resample_wide_u8(None, None), named="dyt_resample_wide_u8")
    _refuses_without(monkeypatch, _lib, "dyt_resample_wide_coeffs", lambda: _lib.resample_wide_coeffs(None, 0, 64, 64))


def test_resample_wide_h_is_hip_free_and_a_new_file_beside_the_old():
    src = open(os.path.join(CSRC, "resample_wide.h")).read()
    assert re.findall(r"#include\s*[<\"]([^>\"]+)", src) == ["resample.h"]      # readable by a host compiler alone, as that file is
    # the coefficient arithmetic and its pragma are resample.h's one template: no floating-point arithmetic of this file's own
    assert "contract" not in src and not re.search(r"\b(float|double)\b", src)
    assert open(os.path.join(CSRC, "resample.h")).read().count("#pragma clang fp contract(off)") == 2
    consts = dict(re.findall(r"\b(RSW_[A-Z_]+) = (\d+)", src))
    import _lib
    assert int(consts["RSW_KMAX"]) == W.KMAX == _lib.RESAMPLE_WIDE_KMAX == 75 and _lib.RESAMPLE_WIDE_COEFF_WORDS * 4 == PER_IMAGE
    assert "RSW_COEFF_FIELDS = 2 + RSW_KMAX" in src
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bresample\.hip\b.*\bresample_wide\.hip\b", mk, re.M) and "contract" not in mk
    hip = open(os.path.join(CSRC, "resample_wide.hip")).read()
    assert "atomic" not in hip.replace("no atomics", "") and not re.search(r"\b(float|double)\b", hip.split("resample_wide_h_kernel(", 1)[1])
    dev = open(os.path.join(CSRC, "resample_dev.h")).read()                      # the pixel helpers both vertical passes and the staging share
    pixel = dev.split("namespace dyt {", 1)[1].split("the coefficient kernel of a bicubic route", 1)[0]
    assert "resample_acc_pack" in pixel and "resample_stage_row" in pixel and '#include "resample_dev.h"' in hip
    assert "atomic" not in dev.replace("No atomics", "") and not re.search(r"\b(float|double)\b", pixel)


# ---- 2. csrc/resample_wide.h through the host compiler --------------------------------------------------------------------------------------
def _cxx():
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler (CXX, c++, g++, clang++)"
    return cxx


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("resample_wide") / "resample_wide_check")
    subprocess.run([_cxx(), "-std=c++17", "-O2", "-I", CSRC, os.path.join(ROOT, "tools", "resample_wide_check.cpp"), "-o", exe], check=True)
    return exe


def test_resample_wide_h_walked_by_the_host_program(checker):
    p = subprocess.run([checker], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    for part in ("rows ok", "coefficients ok", "refusals ok", "all ok", "widest 74 taps"):
        assert part in p.stdout, p.stdout


def _ints(checker, mode, n_in, n_out, xx):
    got = subprocess.run([checker, mode, str(n_in), str(n_out), str(xx)], capture_output=True, text=True, check=True).stdout.split()
    return [int(v) for v in got]


def test_the_header_coefficients_are_the_restatements(checker):
    tuples = [(4096, 224, 0), (4096, 224, 111), (4096, 224, 223)]
    for n_in, n_out in ((561, 224), (560, 224), (700, 256), (1242, 224), (375, 224), (32, 224), (1, 224)):
        tuples += [(n_in, n_out, 0), (n_in, n_out, n_out // 2 - 1), (n_in, n_out, n_out - 1)]
    for n_in, n_out, xx in tuples:
        lo, cnt, k = W.coeffs(n_in, n_out, [xx], width=W.KMAX)
        assert _ints(checker, "coeffs", n_in, n_out, xx) == [int(lo[0]), int(cnt[0])] + [int(v) for v in k[0]], (n_in, n_out, xx)
    widest = int(np.argmax(W.coeffs(4096, 224, np.arange(224))[1]))
    assert _ints(checker, "coeffs", 4096, 224, widest)[1] == 74


def test_on_the_narrow_list_the_wide_header_gives_the_narrow_headers_integers(checker):
    for n_in, n_out, xx in NARROW_TUPLES:
        lo, cnt, k = W.coeffs(n_in, n_out, [xx], width=W.KMAX)
        wide, narrow = _ints(checker, "coeffs", n_in, n_out, xx), _ints(checker, "narrow", n_in, n_out, xx)
        assert wide == [int(lo[0]), int(cnt[0])] + [int(v) for v in k[0]], (n_in, n_out, xx)
        assert len(narrow) == 13 and wide[:13] == narrow and not any(wide[13:]), (n_in, n_out, xx)


# ---- 3. geometry and refusals --------------------------------------------------------------------------------------------------------------
def test_any_scale_takes_the_rows_the_default_refuses():
    from util.crop import CropDraw, DeviceResizeCenterCrop
    with pytest.raises(ValueError, match="more than 2.5 times"):
        DeviceResizeCenterCrop().draw_for([(700, 700)])
    d = DeviceResizeCenterCrop(any_scale=True).draw_for([(700, 700), (1200, 1600)])
    assert d.wide and d.rows == [(700, 700, 0, 0, 700, 700, 256, 256, 16, 16, 0), (1200, 1600, 0, 0, 1200, 1600) + R.eval_geometry(1200, 1600) + (0,)]
    assert not DeviceResizeCenterCrop().draw_for([(300, 400)]).wide and not CropDraw([(64, 64, 0, 0, 64, 64) + T + (0,)]).wide
    row = (700, 700, 0, 0, 700, 700, 256, 256, 16, 16, 0)
    with pytest.raises(ValueError, match="more than 2.5 times"):
        CropDraw([row])
    w = CropDraw([row], wide=True)
    assert w.wide and w.words()[:8] == struct.pack("<2i", 3, 1) and len(w.words()) == 4 * (16 + 12)      # the same table: filter word 3
    assert "wide=True" in repr(w) and "wide" not in repr(CropDraw([(64, 64, 0, 0, 64, 64) + T + (0,)]))
    with pytest.raises(ValueError):
        CropDraw([row + (0,)], filter=2, wide=True)      # clip rows have no scale bound and no wide route
    w.check(700, 700)
    with pytest.raises(ValueError, match="more than 2.5 times"):
        w.check(700, 700, wide=False)
    with pytest.raises(ValueError, match="valid extent"):
        w.check(699, 700)


@pytest.mark.parametrize("seed", [0, 1234])
def test_any_scale_draws_the_same_boxes_from_the_same_seed(seed):
    from util.crop import DeviceRandomResizedCrop
    golden = np.load(NARROW_GOLDEN)
    sizes, boxes, flips = golden["draw%d_sizes" % seed], golden["draw%d_boxes" % seed], golden["draw%d_flips" % seed]
    g = torch.Generator().manual_seed(seed)
    d = DeviceRandomResizedCrop(any_scale=True, generator=g).draw_for(torch.from_numpy(sizes))
    assert d.wide and d.boxes() == [tuple(b) for b in boxes.tolist()] and d.flips() == flips.tolist()
    assert np.float32(torch.rand(1, generator=g).item()) == golden["draw%d_next" % seed]
    g2 = torch.Generator().manual_seed(seed)
    d2 = DeviceRandomResizedCrop(generator=g2).draw_for(torch.from_numpy(sizes))
    assert d2.rows == d.rows and not d2.wide
    # large images: the default refuses a draw with a side above 560, any_scale draws it
    big = [(1600, 1200)] * 8
    g3 = torch.Generator().manual_seed(seed)
    d3 = DeviceRandomResizedCrop(any_scale=True, generator=g3).draw_for(big)
    assert max(max(r[4], r[5]) for r in d3.rows) > 560
    with pytest.raises(ValueError, match="more than 2.5 times"):
        DeviceRandomResizedCrop(generator=torch.Generator().manual_seed(seed)).draw_for(big)


def test_device_resize_rows_and_refusals():
    from util.crop import DeviceResize
    d = DeviceResize(any_scale=True).draw_for([(375, 1242), (32, 32)])
    assert d.wide and d.rows == [(375, 1242, 0, 0, 375, 1242, 224, 224, 0, 0, 0), (32, 32, 0, 0, 32, 32, 224, 224, 0, 0, 0)]
    assert DeviceResize().draw_for([(32, 32), (560, 300)]).rows[1] == (560, 300, 0, 0, 560, 300, 224, 224, 0, 0, 0)
    assert not DeviceResize().draw_for([(32, 32)]).wide and DeviceResize().size == DeviceResize(size=[224, 224]).size == (224, 224)
    with pytest.raises(ValueError, match="more than 2.5 times"):
        DeviceResize().draw_for([(375, 1242)])      # the default keeps the 11-tap route and its bound
    torch.manual_seed(3)
    before = torch.rand(1).item()
    torch.manual_seed(3)
    DeviceResize().draw_for([(100, 100)] * 4)      # makes no draw
    assert torch.rand(1).item() == before
    for make in (lambda: DeviceResize(size=192), lambda: DeviceResize(size=(224, 192)), lambda: DeviceResize(size=(256, 256)),
                 lambda: DeviceResize(size=224),      # torchvision's Resize(224) is the short-side rule, another geometry
                 lambda: DeviceResize(interpolation=2), lambda: DeviceResize(interpolation="bilinear")):
        with pytest.raises(NotImplementedError):
            make()
    for bad in ([(0, 5)], [(5000, 5)], [], [(1, 2, 3)]):
        with pytest.raises(ValueError):
            DeviceResize(any_scale=True).draw_for(bad)


def test_row_error_wide_keeps_every_other_refusal():
    """The table of test_crop_host.py's test_every_refusal: with wide=True only the two rows refused for their scale pass."""
    from util.crop import CropDraw, row_error
    good = (300, 400, 10, 20, 200, 300, 256, 341, 16, 58, 0)
    assert row_error(good, wide=True) is None and row_error(good, 300, 400, wide=True) is None
    assert row_error(good, 299, 400, wide=True) and row_error(good, 300, 399, wide=True)
    bad = {"empty extent": (0, 400) + good[2:], "box h 0": good[:4] + (0,) + good[5:], "box w 0": good[:5] + (0,) + good[6:],
           "top < 0": good[:2] + (-1,) + good[3:], "left < 0": good[:3] + (-1,) + good[4:], "box below the image": good[:2] + (101,) + good[3:],
           "box right of the image": good[:3] + (101,) + good[4:], "full h < 224": good[:6] + (223, 341, 0, 58, 0),
           "full w < 224": good[:6] + (256, 223, 16, 0, 0), "window below full": good[:8] + (33, 58, 0), "window right of full": good[:8] + (16, 118, 0),
           "off < 0": good[:8] + (-1, 58, 0)}
    for what, row in bad.items():
        assert row_error(row, wide=True) == row_error(row), what      # the same refusal, the same text
        assert row_error(row, wide=True), what
        with pytest.raises(ValueError):
            CropDraw([good, row], wide=True)
    for row in ((600, 600, 0, 0, 561, 100, 224, 224, 0, 0, 0), (600, 600, 0, 0, 100, 561, 224, 224, 0, 0, 0)):
        assert row_error(row) and row_error(row, wide=True) is None and row_error(row, 600, 600, wide=True) is None
    assert row_error((4097, 100, 0, 0, 100, 100) + T + (0,), wide=True)      # a side no entry takes
    assert row_error((4096, 4096, 0, 0, 4096, 4096) + T + (0,), wide=True) is None


def test_refusals_of_the_entries_need_no_device():
    import _lib
    for L in (_lib.lib(), _lib.lib(fp16=True)):
        src, dst, tab, scr = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000), ctypes.c_void_p(0x30000), ctypes.c_void_p(0x40000)
        need = 4 * (PER_IMAGE + 64 * 672)
        bad = {
            "null src": (None, 4, 64, 64, dst, tab, 4, scr, need),
            "null dst": (src, 4, 64, 64, None, tab, 4, scr, need),
            "null table": (src, 4, 64, 64, dst, None, 4, scr, need),
            "null scratch": (src, 4, 64, 64, dst, tab, 4, None, need),
            "misaligned src": (ctypes.c_void_p(0x10008), 4, 64, 64, dst, tab, 4, scr, need),
            "misaligned dst": (src, 4, 64, 64, ctypes.c_void_p(0x20004), tab, 4, scr, need),
            "misaligned table": (src, 4, 64, 64, dst, ctypes.c_void_p(0x30004), 4, scr, need),
            "misaligned scratch": (src, 4, 64, 64, dst, tab, 4, ctypes.c_void_p(0x40002), need),
            "batch 0": (src, 0, 64, 64, dst, tab, 4, scr, need),
            "batch above capacity": (src, 5, 64, 64, dst, tab, 4, scr, 2 * need),
            "capacity 0": (src, 1, 64, 64, dst, tab, 0, scr, need),
            "short scratch": (src, 4, 64, 64, dst, tab, 4, scr, need - 1),
            "the narrow route's scratch": (src, 4, 64, 64, dst, tab, 4, scr, 4 * 23296),
            "scratch for a lower batch": (src, 4, 65, 64, dst, tab, 4, scr, need),
            "side 0": (src, 4, 0, 64, dst, tab, 4, scr, need),
            "side above 4096": (src, 4, 64, 4097, dst, tab, 4, scr, need),
            "height above 4096": (src, 4, 4097, 64, dst, tab, 4, scr, 1 << 40),
        }
        for what, a in bad.items():
            assert L.dyt_resample_wide_u8(*a, None) == -1, what
            text = L.dyt_last_error()
            assert text and b"dyt_resample_wide_u8: resample:" in text, what
        out = ctypes.c_void_p(0x50000)
        for what, a in {"null table": (None, 4, 0, 64, 64, out), "null out": (tab, 4, 0, 64, 64, None), "row 4 of 4": (tab, 4, 4, 64, 64, out),
                        "row -1": (tab, 4, -1, 64, 64, out), "misaligned out": (tab, 4, 0, 64, 64, ctypes.c_void_p(0x50004)),
                        "side above 4096": (tab, 4, 0, 5000, 64, out), "capacity 0": (tab, 0, 0, 64, 64, out)}.items():
            assert L.dyt_resample_wide_coeffs(*a, None) == -1, what
            text = L.dyt_last_error()
            assert text and b"dyt_resample_wide_coeffs" in text, what


def test_the_loops_accept_device_resize_in_both_slots_and_still_refuse_clip_classes():
    import engine_finetune as E
    from _lib import DyTError
    from util.crop import DeviceClipUniformCrop, DeviceRandomResizedCrop, DeviceResize, DeviceResizeCenterCrop
    model = types.SimpleNamespace(input_norm=((0.5,) * 3, (0.5,) * 3))
    for resize in (DeviceResize(), DeviceResize(any_scale=True)):
        assert E._device_crop(types.SimpleNamespace(device_crop=resize), "device_crop", DeviceRandomResizedCrop, model) is resize
        assert E._device_crop(types.SimpleNamespace(device_eval_crop=resize), "device_eval_crop", DeviceResizeCenterCrop, model) is resize
        with pytest.raises(DyTError, match="video"):
            E._device_crop(types.SimpleNamespace(device_crop=resize), "device_crop", DeviceRandomResizedCrop, model, video=True)
    for crop in (DeviceRandomResizedCrop(any_scale=True), DeviceResizeCenterCrop(any_scale=True)):
        kind = type(crop)
        name = "device_crop" if kind is DeviceRandomResizedCrop else "device_eval_crop"
        assert E._device_crop(types.SimpleNamespace(**{name: crop}), name, kind, model) is crop
    with pytest.raises(DyTError, match="DeviceResizeCenterCrop"):      # the slots still tell their own classes apart
        E._device_crop(types.SimpleNamespace(device_eval_crop=DeviceRandomResizedCrop(any_scale=True)), "device_eval_crop", DeviceResizeCenterCrop, model)
    clip = DeviceClipUniformCrop()
    for name, kind in (("device_crop", DeviceRandomResizedCrop), ("device_eval_crop", DeviceResizeCenterCrop)):
        with pytest.raises(DyTError, match="video clips"):
            E._device_crop(types.SimpleNamespace(**{name: clip}), name, kind, model)
    with pytest.raises(DyTError, match="input_norm"):
        E._device_crop(types.SimpleNamespace(device_crop=DeviceResize()), "device_crop", DeviceRandomResizedCrop, types.SimpleNamespace(input_norm=None))
    with pytest.raises(DyTError, match="video clips"):
        E._resample_batch(model, DeviceResize(any_scale=True), torch.zeros(2, 4, 64, 64, 3, dtype=torch.uint8))
