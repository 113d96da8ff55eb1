"""CPU tests of the device crop / resize (dyt_resample_u8, dyt_resample_scratch_bytes, dyt_resample_coeffs; util.crop): the header, the
ctypes binding and both libraries agree without a version or flag change; dynamic-tuning_amd/csrc/resample.h -- row check, coefficient
function and every argument check -- is walked by tools/resample_check.cpp, built with the host compiler (its header gives the sanitizer
build of the same stand-alone program), and its coefficients equal tests/resample_refs.py's; the entries refuse bad arguments without a
device; DeviceRandomResizedCrop reproduces the reference's recorded boxes and flips (tests/golden/resample/resample.npz) draw for draw;
the evaluation geometry, the table words, every refusal and pad_collate.  Nothing here needs a GPU; a missing compiler is a failure."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dynamic-tuning_amd", "csrc")
ENTRIES = {"dyt_resample_u8", "dyt_resample_scratch_bytes", "dyt_resample_coeffs"}
GOLDEN = os.path.join(ROOT, "tests", "golden", "resample", "resample.npz")


def _header():
    return open(os.path.join(ROOT, "include", "dyt_hip.h")).read()


def _args(name, ret="int"):
    m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (ret, name), _header())
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


# ---- header, binding, libraries --------------------------------------------------------------------------------------------------------
def test_header_declares_the_entries_and_no_new_flag():
    assert _args("dyt_resample_u8") == ["const uint8_t* src", "int batch", "int src_h", "int src_w", "uint8_t* dst", "const void* table_dev",
                                        "int capacity", "void* scratch_dev", "int64_t scratch_bytes", "void* stream"]
    assert _args("dyt_resample_scratch_bytes", "int64_t") == ["int batch"]
    assert _args("dyt_resample_coeffs") == ["const void* table_dev", "int capacity", "int row", "int src_h", "int src_w", "int32_t* out_dev",
                                            "void* stream"]
    values = [int(v) for v in re.findall(r"#define\s+DYT_F_[A-Z0-9_]+\s+(\d+)\b", _header())]
    assert len(values) == len(set(values)) == 11   # the cropped batch uses the existing byte flags


def test_binding_equals_the_header_and_the_version_stays_5():
    import _lib
    declared = set(re.findall(r"\b(dyt_[a-z0-9_]+)\s*\(", _header()))
    assert ENTRIES <= declared
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    assert ENTRIES <= _lib.OPTIONAL_SYMBOLS   # discovered by symbol
    assert [len(_lib.SYMBOLS[n][1]) for n in ("dyt_resample_u8", "dyt_resample_scratch_bytes", "dyt_resample_coeffs")] == [10, 1, 7]
    for fp16 in (False, True):
        L = _lib.lib(fp16=fp16)
        assert L.dyt_version() == 5
        assert all(hasattr(L, n) for n in ENTRIES)
        assert L.dyt_resample_scratch_bytes(1) == 2 * 13 * 224 * 4 and L.dyt_resample_scratch_bytes(128) == 128 * 23296
        assert L.dyt_resample_scratch_bytes(0) == 0 and L.dyt_resample_scratch_bytes(-3) == 0


def _refuses_without(monkeypatch, _lib, symbol, call):
    """``call`` raises a DyTError naming ``symbol`` and "rebuild it" when the loaded library is one that lacks ``symbol``."""
    real = _lib.lib()
    stand_in = types.SimpleNamespace(**{n: getattr(real, n) for n in _lib.SYMBOLS if n != symbol and hasattr(real, n)})
    monkeypatch.setattr(_lib, "lib", lambda fp16=False: stand_in)
    with pytest.raises(_lib.DyTError) as e:
        call()
    assert symbol in str(e.value) and "rebuild it" in str(e.value), str(e.value)


def test_python_refuses_by_name_when_the_library_lacks_the_entries(monkeypatch):
    import _lib
    import runtime
    src = inspect.getsource(runtime.DyTEngine.resample)
    assert "hasattr(" in src and "rebuild it" in src
    # the wrappers delegate to one body: called with a library that lacks the symbol, before any argument is looked at
    _refuses_without(monkeypatch, _lib, "dyt_resample_u8", lambda: _lib.resample_u8(None, None))
    _refuses_without(monkeypatch, _lib, "dyt_resample_coeffs", lambda: _lib.resample_coeffs(None, 0, 64, 64))


def test_resample_h_is_hip_free_and_fixes_the_strides():
    src = open(os.path.join(CSRC, "resample.h")).read()
    assert re.findall(r"#include\s*[<\"]([^>\"]+)", src) == ["math.h"]   # and that one for the host compiler only
    assert "static_assert(sizeof(ResampleRow) == RS_ROW_WORDS * 4 && sizeof(ResampleRow) % 16 == 0" in src
    assert "static_assert(sizeof(ResampleHeader) == RS_HEADER_WORDS * 4" in src
    assert src.count("#pragma clang fp contract(off)") == 2   # the filter and the coefficient function, nothing else
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bresample\.hip\b", mk, re.M)
    assert "contract" not in mk   # the flags of the other units are not touched
    from util import crop
    import _lib
    consts = dict(re.findall(r"\b(RS_[A-Z_]+) = (\d+)", src))
    assert (int(consts["RS_HEADER_WORDS"]), int(consts["RS_ROW_WORDS"])) == (crop.HEADER_WORDS, crop.ROW_WORDS) == (16, 12)
    assert (_lib.RESAMPLE_HEADER_WORDS, _lib.RESAMPLE_ROW_WORDS, _lib.RESAMPLE_COEFF_WORDS) == (16, 12, 2 * 13 * 224)
    assert int(consts["RS_OUT"]) == crop.OUT == R.OUT == 224 and int(consts["RS_KMAX"]) == R.KMAX == 11
    assert int(consts["RS_BICUBIC"]) == crop.BICUBIC == 3 and int(consts["RS_MAX_SIDE"]) == crop.MAX_SIDE == _lib.RESAMPLE_MAX_SIDE == 4096
    assert int(consts["RS_PRECISION_BITS"]) == R.PRECISION_BITS == 22 and int(consts["RS_FLAG_MIRROR"]) == crop.FLAG_MIRROR == 1


# ---- the entries refuse without a device -------------------------------------------------------------------------------------------------
def test_refusals_of_the_entries_need_no_device():
    import _lib
    for L in (_lib.lib(), _lib.lib(fp16=True)):
        src, dst, tab, scr = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000), ctypes.c_void_p(0x30000), ctypes.c_void_p(0x40000)
        need = 4 * 23296
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
            "batch above capacity": (src, 5, 64, 64, dst, tab, 4, scr, 5 * 23296),
            "capacity 0": (src, 1, 64, 64, dst, tab, 0, scr, need),
            "small scratch": (src, 4, 64, 64, dst, tab, 4, scr, need - 1),
            "side 0": (src, 4, 0, 64, dst, tab, 4, scr, need),
            "side above 4096": (src, 4, 64, 4097, dst, tab, 4, scr, need),
            "height above 4096": (src, 4, 4097, 64, dst, tab, 4, scr, need),
        }
        for what, a in bad.items():
            assert L.dyt_resample_u8(*a, None) == -1, what
            text = L.dyt_last_error()
            assert text and b"dyt_resample_u8" in text, what
        out = ctypes.c_void_p(0x50000)
        for what, a in {"null table": (None, 4, 0, 64, 64, out), "null out": (tab, 4, 0, 64, 64, None), "row 4 of 4": (tab, 4, 4, 64, 64, out),
                        "row -1": (tab, 4, -1, 64, 64, out), "misaligned out": (tab, 4, 0, 64, 64, ctypes.c_void_p(0x50004)),
                        "side above 4096": (tab, 4, 0, 5000, 64, out), "capacity 0": (tab, 0, 0, 64, 64, out)}.items():
            assert L.dyt_resample_coeffs(*a, None) == -1, what
            text = L.dyt_last_error()
            assert text and b"dyt_resample_coeffs" in text, what


# ---- csrc/resample.h through the host compiler ---------------------------------------------------------------------------------------------
def _cxx():
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler (CXX, c++, g++, clang++)"
    return cxx


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("resample") / "resample_check")
    subprocess.run([_cxx(), "-std=c++17", "-O2", "-I", CSRC, os.path.join(ROOT, "tools", "resample_check.cpp"), "-o", exe], check=True)
    return exe


def test_resample_h_walked_by_the_host_program(checker):
    p = subprocess.run([checker], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    for part in ("rows ok", "coefficients ok", "refusals ok", "all ok"):
        assert part in p.stdout, p.stdout


def test_the_header_coefficients_are_the_restatements(checker):
    for n_in, n_out, xx in ((512, 224, 100), (512, 224, 0), (512, 224, 223), (490, 224, 57), (8, 224, 3), (10, 224, 223), (1, 224, 17),
                            (224, 224, 5), (300, 256, 16), (300, 256, 239), (400, 341, 58), (400, 341, 281), (560, 224, 111)):
        lo, cnt, k = R.coeffs(n_in, n_out, [xx])
        got = subprocess.run([checker, "coeffs", str(n_in), str(n_out), str(xx)], capture_output=True, text=True, check=True).stdout.split()
        assert [int(v) for v in got] == [int(lo[0]), int(cnt[0])] + [int(v) for v in k[0]], (n_in, n_out, xx)


# ---- util.crop ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("seed", [0, 1234])
def test_the_draws_are_the_references(golden, seed):
    """A seeded generator reproduces the boxes and flips the seeded reference drew, and the draw that follows them."""
    from util.crop import DeviceRandomResizedCrop
    sizes, boxes, flips = golden["draw%d_sizes" % seed], golden["draw%d_boxes" % seed], golden["draw%d_flips" % seed]
    g = torch.Generator().manual_seed(seed)
    d = DeviceRandomResizedCrop(generator=g).draw_for(torch.from_numpy(sizes))
    assert d.boxes() == [tuple(b) for b in boxes.tolist()]
    assert d.flips() == flips.tolist()
    assert np.float32(torch.rand(1, generator=g).item()) == golden["draw%d_next" % seed]
    assert [r[:2] for r in d.rows] == [tuple(s) for s in sizes.tolist()] and all(r[6:10] == (224, 224, 0, 0) for r in d.rows)
    torch.manual_seed(seed)   # generator=None: torch's global generator, as the reference
    d2 = DeviceRandomResizedCrop().draw_for(sizes.tolist())
    assert d2.rows == d.rows and np.float32(torch.rand(1).item()) == golden["draw%d_next" % seed]


def test_flip_none_makes_no_flip_draw_and_injection_is_handed_out():
    from util.crop import CropDraw, DeviceRandomResizedCrop
    g = torch.Generator().manual_seed(5)
    a = DeviceRandomResizedCrop(flip=None, generator=g).draw_for([(300, 400)] * 3)
    g2 = torch.Generator().manual_seed(5)
    c = DeviceRandomResizedCrop(flip=None, generator=g2)
    assert [c.get_params(300, 400) for _ in range(3)] == a.boxes() and not any(a.flips())
    fixed = CropDraw([(64, 64, 0, 0, 64, 64, 224, 224, 0, 0, 1)])
    c.inject([fixed])
    assert c.draw_for([(64, 64)]) is fixed
    c.inject([fixed])
    with pytest.raises(ValueError):
        c.draw_for([(64, 64)] * 2)


def test_eval_geometry(golden):
    from util.crop import DeviceResizeCenterCrop
    e = DeviceResizeCenterCrop()
    assert e.geometry(300, 400) == tuple(golden["eval_sizes"].tolist()) == (256, 341, 16, 58)
    for h, w in ((400, 300), (256, 256), (500, 375), (333, 500), (480, 640), (224, 224), (640, 256)):
        assert e.geometry(h, w) == R.eval_geometry(h, w)
    d = e.draw_for([(300, 400), (400, 300)])
    assert d.rows == [(300, 400, 0, 0, 300, 400, 256, 341, 16, 58, 0), (400, 300, 0, 0, 400, 300, 341, 256, 58, 16, 0)]
    assert tuple(golden["eval_row"].tolist()) == d.rows[0]
    with pytest.raises(ValueError):
        e.draw_for([(700, 700)])    # 700 > 2.5 * 256: more than 11 taps


def test_table_words():
    from util.crop import CropDraw, table_words
    rows = [(300, 400, 0, 0, 300, 400, 256, 341, 16, 58, 0), (64, 48, 3, 5, 50, 31, 224, 224, 0, 0, 1)]
    d = CropDraw(rows)
    w = d.words(5)
    assert len(w) == 4 * table_words(5) == 4 * (16 + 12 * 5)
    assert struct.unpack("<16i", w[:64]) == (3, 2) + (0,) * 14
    got = [struct.unpack("<12i", w[64 + 48 * k:64 + 48 * (k + 1)]) for k in range(5)]
    assert got[0] == rows[0] + (0,) and got[1] == rows[1] + (0,) and got[2] == got[3] == got[4] == (0,) * 12
    assert len(d.words()) == 4 * table_words(2) and (d.units, d.images()) == (2, 2)
    with pytest.raises(ValueError):
        d.words(1)


def test_every_refusal():
    from util.crop import CropDraw, DeviceRandomResizedCrop, DeviceResizeCenterCrop, row_error
    good = (300, 400, 10, 20, 200, 300, 256, 341, 16, 58, 0)
    assert row_error(good) is None and row_error(good, 300, 400) is None
    assert row_error(good, 299, 400) and row_error(good, 300, 399)
    bad = {"empty extent": (0, 400) + good[2:], "box h 0": good[:4] + (0,) + good[5:], "box w 0": good[:5] + (0,) + good[6:],
           "top < 0": good[:2] + (-1,) + good[3:], "left < 0": good[:3] + (-1,) + good[4:], "box below the image": good[:2] + (101,) + good[3:],
           "box right of the image": good[:3] + (101,) + good[4:], "full h < 224": good[:6] + (223, 341, 0, 58, 0),
           "full w < 224": good[:6] + (256, 223, 16, 0, 0), "window below full": good[:8] + (33, 58, 0), "window right of full": good[:8] + (16, 118, 0),
           "off < 0": good[:8] + (-1, 58, 0), "more than 2.5": (600, 600, 0, 0, 561, 100, 224, 224, 0, 0, 0),
           "more than 2.5 across": (600, 600, 0, 0, 100, 561, 224, 224, 0, 0, 0)}
    for what, row in bad.items():
        assert row_error(row), what
        with pytest.raises(ValueError):
            CropDraw([good, row])
    assert row_error((600, 600, 0, 0, 560, 560, 224, 224, 0, 0, 0)) is None
    for make in (lambda: CropDraw([]), lambda: CropDraw([good[:10]]),
                 lambda: DeviceRandomResizedCrop(scale=(0.5, 0.1)), lambda: DeviceRandomResizedCrop(ratio=(0.0, 1.0)),
                 lambda: DeviceRandomResizedCrop(flip=1.5), lambda: DeviceResizeCenterCrop(resize=200),
                 lambda: DeviceRandomResizedCrop().draw_for([(0, 5)]), lambda: DeviceRandomResizedCrop().draw_for([(5000, 5)]),
                 lambda: DeviceRandomResizedCrop().draw_for([]), lambda: DeviceRandomResizedCrop().draw_for([(1, 2, 3)])):
        with pytest.raises(ValueError):
            make()
    for make in (lambda: DeviceRandomResizedCrop(size=192), lambda: DeviceRandomResizedCrop(size=(224, 192)), lambda: DeviceRandomResizedCrop(interpolation=2),
                 lambda: DeviceResizeCenterCrop(size=192), lambda: DeviceResizeCenterCrop(interpolation=0)):
        with pytest.raises(NotImplementedError):
            make()
    assert DeviceRandomResizedCrop(size=(224, 224)).size == 224
    # the loop refuses what it cannot feed, before any device work
    import engine_finetune as E
    from _lib import DyTError
    crop = DeviceRandomResizedCrop()
    model = types.SimpleNamespace(input_norm=None)
    with pytest.raises(DyTError, match="input_norm"):
        E._device_crop(types.SimpleNamespace(device_crop=crop), "device_crop", DeviceRandomResizedCrop, model)
    model.input_norm = ((0.5,) * 3, (0.5,) * 3)
    assert E._device_crop(types.SimpleNamespace(device_crop=crop), "device_crop", DeviceRandomResizedCrop, model) is crop
    assert E._device_crop(types.SimpleNamespace(), "device_crop", DeviceRandomResizedCrop, model) is None
    assert E._device_crop(None, "device_crop", DeviceRandomResizedCrop, model) is None
    with pytest.raises(DyTError, match="video"):
        E._device_crop(types.SimpleNamespace(device_crop=crop), "device_crop", DeviceRandomResizedCrop, model, video=True)
    with pytest.raises(DyTError, match="DeviceResizeCenterCrop"):
        E._device_crop(types.SimpleNamespace(device_eval_crop=crop), "device_eval_crop", DeviceResizeCenterCrop, model)
    with pytest.raises(DyTError, match="video clips"):
        E._resample_batch(model, crop, torch.zeros(2, 4, 64, 64, 3, dtype=torch.uint8))
    with pytest.raises(DyTError, match="uint8"):
        E._resample_batch(model, crop, torch.zeros(2, 3, 64, 64))


def test_pad_collate():
    from util.crop import pad_collate
    rng = np.random.default_rng(1)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((40, 64), (64, 33), (17, 23))]
    (pixels, sizes), labels = pad_collate([(imgs[0], 3), (torch.from_numpy(imgs[1]), 1), (imgs[2], 7)])
    assert pixels.dtype == torch.uint8 and tuple(pixels.shape) == (3, 64, 64, 3) and pixels.is_contiguous()
    assert sizes.dtype == torch.int32 and sizes.tolist() == [[40, 64], [64, 33], [17, 23]]
    assert labels.dtype == torch.int64 and labels.tolist() == [3, 1, 7]
    for i, im in enumerate(imgs):
        assert np.array_equal(pixels[i, :im.shape[0], :im.shape[1]].numpy(), im)
        assert int(pixels[i, im.shape[0]:].sum()) == 0 and int(pixels[i, :, im.shape[1]:].sum()) == 0
    (pixels, _), _ = pad_collate([(imgs[0], 0)], pad_to=(128, 96))
    assert tuple(pixels.shape) == (1, 128, 96, 3)
    for bad in (lambda: pad_collate([(imgs[0], 0)], pad_to=(32, 96)), lambda: pad_collate([(imgs[0].astype(np.float32), 0)]),
                lambda: pad_collate([(imgs[0][..., 0], 0)]), lambda: pad_collate([(imgs[0].transpose(2, 0, 1), 0)])):
        with pytest.raises(ValueError):
            bad()
