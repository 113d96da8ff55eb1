"""CPU tests of the device clip pipeline (dyt_resample_clip_f32, dyt_resample_clip_coeffs; util.crop's clip classes): the header, the ctypes
binding and both libraries agree without a version or flag change; dynamic-tuning_amd/csrc/resample_clip.h -- row check, index / weight
function, two-tap sum and every argument check -- is walked by tools/resample_clip_check.cpp, built with the host compiler, and its
integers and bit patterns equal tests/clip_resample_refs.py's; the entries refuse bad arguments without a device; the three classes
reproduce the reference's recorded draws (tests/golden/resample/clip_resample.npz) draw for draw, and the draw after them; the table
words, every refusal, the loop's cross-type refusals and pad_collate_clips.  Nothing here needs a GPU; a missing compiler is a failure."""
import ctypes
import inspect
import os
import random
import re
import shutil
import struct
import subprocess
import types

import numpy as np
import pytest
import torch

import clip_resample_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dynamic-tuning_amd", "csrc")
ENTRIES = {"dyt_resample_clip_f32", "dyt_resample_clip_coeffs"}
GOLDEN = os.path.join(ROOT, "tests", "golden", "resample", "clip_resample.npz")
GOOD = (300, 400, 10, 20, 200, 300, 256, 341, 16, 58, 1, 1)


def _header():
    return open(os.path.join(ROOT, "include", "dyt_hip.h")).read()


def _args(name, ret="int"):
    m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (ret, name), _header())
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


# ---- header, binding, libraries --------------------------------------------------------------------------------------------------------
def test_header_declares_the_entries_and_no_new_flag():
    assert _args("dyt_resample_clip_f32") == ["const uint8_t* src", "int batch", "int frames", "int src_h", "int src_w", "float* dst", "int units",
                                              "const void* table_dev", "int capacity", "const float mean[3]", "const float std[3]", "void* stream"]
    assert _args("dyt_resample_clip_coeffs") == ["const void* table_dev", "int capacity", "int row", "int src_h", "int src_w", "int32_t* out_dev",
                                                 "void* stream"]
    values = [int(v) for v in re.findall(r"#define\s+DYT_F_[A-Z0-9_]+\s+(\d+)\b", _header())]
    assert len(values) == len(set(values)) == 11


def _refuses_without(monkeypatch, _lib, symbol, call):
    """``call`` raises a DyTError naming ``symbol`` and "rebuild it" when the loaded library is one that lacks ``symbol``."""
    real = _lib.lib()
    stand_in = types.SimpleNamespace(**{n: getattr(real, n) for n in _lib.SYMBOLS if n != symbol and hasattr(real, n)})
    monkeypatch.setattr(_lib, "lib", lambda fp16=False: stand_in)
    with pytest.raises(_lib.DyTError) as e:
        call()
    assert symbol in str(e.value) and "rebuild it" in str(e.value), str(e.value)


def test_binding_equals_the_header_and_the_version_stays_5(monkeypatch):
    import _lib
    declared = set(re.findall(r"\b(dyt_[a-z0-9_]+)\s*\(", _header()))
    assert ENTRIES <= declared and declared == set(_lib.SYMBOLS)
    assert ENTRIES <= _lib.OPTIONAL_SYMBOLS   # discovered by symbol
    assert [len(_lib.SYMBOLS[n][1]) for n in ("dyt_resample_clip_f32", "dyt_resample_clip_coeffs")] == [12, 7]
    for fp16 in (False, True):
        L = _lib.lib(fp16=fp16)
        assert L.dyt_version() == 5 and all(hasattr(L, n) for n in ENTRIES)
    import runtime
    for fn in (_lib.resample_clip_f32, runtime.DyTEngine.resample_clip):
        src = inspect.getsource(fn)
        assert "hasattr(" in src and "rebuild it" in src
    # resample_clip_coeffs delegates: called with a library that lacks the symbol, before any argument is looked at
    _refuses_without(monkeypatch, _lib, "dyt_resample_clip_coeffs", lambda: _lib.resample_clip_coeffs(None, 0, 64, 64))


def test_resample_clip_h_is_hip_free_and_one_definition():
    src = open(os.path.join(CSRC, "resample_clip.h")).read()
    assert re.findall(r"#include\s*[<\"]([^>\"]+)", src) == ["resample.h"]
    assert "__global__" not in src and "hip" not in src.lower().replace("hip-free", "").replace("hip type", "").replace("resample_clip.hip", "")
    assert src.count("#pragma clang fp contract(off)") == 2 and src.count("fmaf(") >= 2   # clip_axis and clip_lerp spell their fused steps out
    kernel = open(os.path.join(CSRC, "resample_clip.hip")).read()
    assert '#include "resample_clip.h"' in kernel and "fmaf" not in kernel.split("namespace dyt {", 1)[1]   # the kernels call the header's functions
    tool = open(os.path.join(ROOT, "tools", "resample_clip_check.cpp")).read()
    assert '#include "resample_clip.h"' in tool
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bresample_clip\.hip\b", mk, re.M) and "contract" not in mk
    assert mk.count("CXXFLAGS =") == 1 and "-O3 -std=c++17 -fPIC -Wno-unused-result -Wno-unused-value $(CXXFLAGS_EXTRA)" in mk   # no new flag
    from util import crop
    import _lib
    consts = dict(re.findall(r"\b(RS_[A-Z0-9_]+) = ([0-9<> ]+);", src))
    assert int(consts["RS_BILINEAR_F32"]) == crop.BILINEAR_F32 == _lib.RESAMPLE_BILINEAR_F32 == 2
    assert consts["RS_CLIP_MAX_FULL"].replace(" ", "") == "1<<23" and crop.MAX_FULL == 1 << 23
    assert _lib.RESAMPLE_CLIP_COEFF_WORDS == 2 * 4 * 224
    # the bicubic kernels never read word 11: the shared loader fills it, and neither their files nor their row check name it
    for name in ("resample.hip", "resample_wide.hip", "resample_wide.h"):
        text = open(os.path.join(CSRC, name)).read()
        assert ".pad" not in text and "q2.w" not in text and "clip_row_src" not in text, name
    rs = open(os.path.join(CSRC, "resample.h")).read()
    assert ".pad" not in rs.split("resample_row_ok_core(", 1)[1] and "int pad;" in rs
    assert "r.pad = q2.w;" in open(os.path.join(CSRC, "resample_dev.h")).read()


# ---- the entries refuse without a device -------------------------------------------------------------------------------------------------
def test_refusals_of_the_entries_need_no_device():
    import _lib
    f3 = lambda *v: (ctypes.c_float * 3)(*v)   # noqa: E731
    mean, std = f3(0.485, 0.456, 0.406), f3(0.229, 0.224, 0.225)
    for L in (_lib.lib(), _lib.lib(fp16=True)):
        src, dst, tab = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000), ctypes.c_void_p(0x30000)
        bad = {
            "null src": (None, 2, 2, 64, 64, dst, 2, tab, 4, mean, std),
            "null dst": (src, 2, 2, 64, 64, None, 2, tab, 4, mean, std),
            "null table": (src, 2, 2, 64, 64, dst, 2, None, 4, mean, std),
            "misaligned src": (ctypes.c_void_p(0x10008), 2, 2, 64, 64, dst, 2, tab, 4, mean, std),
            "misaligned dst": (src, 2, 2, 64, 64, ctypes.c_void_p(0x20004), 2, tab, 4, mean, std),
            "misaligned table": (src, 2, 2, 64, 64, dst, 2, ctypes.c_void_p(0x30004), 4, mean, std),
            "batch 0": (src, 0, 2, 64, 64, dst, 2, tab, 4, mean, std),
            "frames 0": (src, 2, 0, 64, 64, dst, 2, tab, 4, mean, std),
            "units 0": (src, 2, 2, 64, 64, dst, 0, tab, 4, mean, std),
            "units above capacity": (src, 2, 2, 64, 64, dst, 5, tab, 4, mean, std),
            "capacity 0": (src, 2, 2, 64, 64, dst, 1, tab, 0, mean, std),
            "side 0": (src, 2, 2, 0, 64, dst, 2, tab, 4, mean, std),
            "side above 4096": (src, 2, 2, 64, 4097, dst, 2, tab, 4, mean, std),
            "height above 4096": (src, 2, 2, 4097, 64, dst, 2, tab, 4, mean, std),
            "frames above 65535": (src, 2, 65536, 64, 64, dst, 2, tab, 4, mean, std),
            "std 0": (src, 2, 2, 64, 64, dst, 2, tab, 4, mean, f3(0.229, 0.0, 0.225)),
            "std inf": (src, 2, 2, 64, 64, dst, 2, tab, 4, mean, f3(float("inf"), 0.224, 0.225)),
            "std nan": (src, 2, 2, 64, 64, dst, 2, tab, 4, mean, f3(0.229, 0.224, float("nan"))),
            "mean nan": (src, 2, 2, 64, 64, dst, 2, tab, 4, f3(float("nan"), 0.456, 0.406), std),
            "null std": (src, 2, 2, 64, 64, dst, 2, tab, 4, mean, None),
        }
        for what, a in bad.items():
            assert L.dyt_resample_clip_f32(*a, None) == -1, what
            text = L.dyt_last_error()
            assert text and b"dyt_resample_clip_f32: resample clip:" in text, (what, text)
        out = ctypes.c_void_p(0x50000)
        for what, a in {"null table": (None, 4, 0, 64, 64, out), "null out": (tab, 4, 0, 64, 64, None), "row 4 of 4": (tab, 4, 4, 64, 64, out),
                        "row -1": (tab, 4, -1, 64, 64, out), "misaligned out": (tab, 4, 0, 64, 64, ctypes.c_void_p(0x50004)),
                        "side above 4096": (tab, 4, 0, 5000, 64, out), "capacity 0": (tab, 0, 0, 64, 64, out)}.items():
            assert L.dyt_resample_clip_coeffs(*a, None) == -1, what
            text = L.dyt_last_error()
            assert text and b"dyt_resample_clip_coeffs" in text, what


# ---- csrc/resample_clip.h through the host compiler ----------------------------------------------------------------------------------------
def _cxx():
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler (CXX, c++, g++, clang++)"
    return cxx


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("resample_clip") / "resample_clip_check")
    subprocess.run([_cxx(), "-std=c++17", "-O2", "-I", CSRC, os.path.join(ROOT, "tools", "resample_clip_check.cpp"), "-o", exe], check=True)
    return exe


def test_resample_clip_h_walked_by_the_host_program(checker):
    p = subprocess.run([checker], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    for part in ("rows ok", "axis ok", "lerp ok", "refusals ok", "all ok"):
        assert part in p.stdout, p.stdout


def test_the_headers_integers_and_bit_patterns_are_numpys(checker):
    for n_in, n_out in ((224, 224), (1, 224), (8, 224), (10, 224), (300, 224), (400, 298), (240, 227), (57, 386), (480, 258), (4032, 224), (4096, 300),
                        (33, 224), (100, 1000)):
        got = subprocess.run([checker, "axis", str(n_in), str(n_out), "0", str(n_out)], capture_output=True, text=True, check=True).stdout.split()
        got = np.array([int(v) for v in got], dtype=np.int64).reshape(n_out, 4)
        i0, i1, l0, l1 = R.axis(n_in, n_out, np.arange(n_out))
        want = np.stack([i0, i1, l0.view(np.uint32).astype(np.int64), l1.view(np.uint32).astype(np.int64)], axis=1)
        assert np.array_equal(got, want), (n_in, n_out, np.argwhere(got != want)[:3].tolist())
    rng = np.random.default_rng(9)
    for _ in range(40):
        w1 = np.float32(rng.random())
        w0, v0, v1 = np.float32(1) - w1, np.float32(rng.normal() * 2), np.float32(rng.normal() * 2)
        words = ["%08x" % int(np.array(x, dtype=np.float32).view(np.uint32)) for x in (w0, v0, w1, v1)]
        got = subprocess.run([checker, "lerp"] + words, capture_output=True, text=True, check=True).stdout.strip()
        assert got == "%08x" % int(R.lerp(w0, v0, w1, v1).view(np.uint32)), words


def test_row_error_and_clip_row_ok_agree_on_hostile_rows(checker):
    from util.crop import clip_row_error
    big, low = 2 ** 31 - 1, -2 ** 31
    rows = [GOOD, (big,) * 12, (low,) * 12, (-1,) * 12, (0,) * 12, GOOD[:11] + (3,), GOOD[:11] + (2,), GOOD[:11] + (-1,),
            (64, 64, big, big, big, big, big, big, big, big, 1, 0), (64, 64, 0, 0, 64, 64, 224, 224, low, low, 0, 0),
            (512, 640, 0, 0, 512, 640, 224, 224, 0, 0, 0, 0), (513, 640, 0, 0, 512, 640, 224, 224, 0, 0, 0, 0), (512, 641, 0, 0, 512, 640, 224, 224, 0, 0, 0, 0),
            (64, 64, 0, 0, 64, 64, 1 << 23, 1 << 23, (1 << 23) - 224, 0, 0, 0), (64, 64, 0, 0, 64, 64, (1 << 23) + 1, 224, 0, 0, 0, 0),
            (64, 64, 60, 0, 5, 5, 224, 224, 0, 0, 0, 0), (64, 64, 0, 0, 64, 64, 223, 224, 0, 0, 0, 0), (64, 64, 0, 0, 64, 64, 224, 224, 1, 0, 0, 0),
            (64, 64, 0, 0, 0, 64, 224, 224, 0, 0, 0, 0)]
    for field in range(12):
        for v in (low, -1, 0, 1, 223, 224, 4097, big):
            rows.append(GOOD[:field] + (v,) + GOOD[field + 1:])
    verdicts = []
    for r in rows:
        out = subprocess.run([checker, "row", "3", "512", "640"] + [str(v) for v in r], capture_output=True, text=True, check=True).stdout.strip()
        verdicts.append(out == "1")
        assert (clip_row_error(r, 3, 512, 640) is None) == (out == "1"), (r, out, clip_row_error(r, 3, 512, 640))
    assert verdicts[0] and not any(verdicts[1:5]) and verdicts[6] and not verdicts[5] and 20 < sum(verdicts) < len(rows) - 40


# ---- util.crop: the draws ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("seed", [0, 1234])
def test_scale_jitter_draws_are_the_references(golden, seed):
    from util.crop import DeviceClipScaleJitterCrop
    sizes, want = golden["sizes"], golden["jit%d_rows" % seed]
    rng, g = np.random.RandomState(seed), torch.Generator().manual_seed(seed)
    d = DeviceClipScaleJitterCrop(np_rng=rng, generator=g).draw_for(torch.from_numpy(sizes))
    assert d.clip and d.filter == 2 and d.units == 12 and d.sources() == list(range(12))
    assert [r[6:10] + (r[10] & 1,) for r in d.rows] == [tuple(w) for w in want.tolist()]
    assert [r[:6] for r in d.rows] == [(h, w, 0, 0, h, w) for h, w in sizes.tolist()]
    assert [rng.uniform(), torch.rand(1, generator=g).item()] == golden["jit%d_next" % seed].tolist()
    np.random.seed(seed)       # generators None: the global ones, as the reference
    torch.manual_seed(seed)
    d2 = DeviceClipScaleJitterCrop().draw_for(sizes.tolist())
    assert d2.rows == d.rows and [np.random.uniform(), torch.rand(1).item()] == golden["jit%d_next" % seed].tolist()
    # mirror=None: no mirror draw; the numpy draws are the same
    rng3, g3 = np.random.RandomState(seed), torch.Generator().manual_seed(seed)
    d3 = DeviceClipScaleJitterCrop(mirror=None, np_rng=rng3, generator=g3).draw_for(sizes.tolist())
    assert [r[6:10] for r in d3.rows] == [r[6:10] for r in d.rows] and not any(d3.flips())
    assert torch.rand(1, generator=g3).item() == torch.rand(1, generator=torch.Generator().manual_seed(seed)).item()


@pytest.mark.parametrize("seed", [0, 1234])
def test_random_resized_crop_draws_are_the_references(golden, seed):
    from util.crop import DeviceClipRandomResizedCrop
    sizes, want = golden["sizes"], golden["rrc%d_boxes" % seed]
    py, rng = random.Random(seed), np.random.RandomState(seed)
    d = DeviceClipRandomResizedCrop(py_rng=py, np_rng=rng).draw_for(sizes.tolist())
    assert d.boxes() == [tuple(b) for b in want.tolist()]
    assert all(r[6:11] == (224, 224, 0, 0, 0) for r in d.rows) and d.sources() == list(range(12))
    assert [py.random(), rng.uniform()] == golden["rrc%d_next" % seed].tolist()
    random.seed(seed)
    np.random.seed(seed)
    d2 = DeviceClipRandomResizedCrop().draw_for(sizes.tolist())
    assert d2.rows == d.rows and [random.random(), np.random.uniform()] == golden["rrc%d_next" % seed].tolist()
    # the 16:1 clips end in the central fallback: ten attempts, ten numpy draws each
    assert tuple(want[8]) == (0, 234, 32, 43) and tuple(want[9]) == (234, 0, 43, 32)


def test_uniform_crop_rows_are_the_references(golden):
    from util.crop import DeviceClipUniformCrop
    sizes = golden["sizes"].tolist()
    one = DeviceClipUniformCrop().draw_for(sizes)
    assert [r[6:10] for r in one.rows] == [tuple(w) for w in golden["uni_rows1"].tolist()] and one.sources() == list(range(12))
    three = DeviceClipUniformCrop(spatial_views=3).draw_for(sizes)
    assert three.units == 36 and three.sources() == [i for i in range(12) for _ in range(3)]
    assert [r[6:10] for r in three.rows] == [tuple(w) for w3 in golden["uni_rows3"].tolist() for w in w3]
    assert [tuple(r) for r in golden["eval_rows"].tolist()] == DeviceClipUniformCrop(spatial_views=3).draw_for([(300, 400)]).rows
    assert DeviceClipUniformCrop(spatial_views=3).draw_for([(400, 300)]).rows == [(400, 300, 0, 0, 400, 300, 298, 224, o, 0, 0, 0) for o in (0, 37, 74)]
    assert not any(one.flips()) and not any(three.flips())


def test_clip_table_words_and_injection():
    from util.crop import BILINEAR_F32, CropDraw, DeviceClipScaleJitterCrop, probe_clip_draw, table_words
    rows = [(300, 400, 0, 0, 300, 400, 224, 298, 0, 37, 0, 1), (64, 48, 3, 5, 50, 31, 224, 224, 0, 0, 1, 0)]
    d = CropDraw(rows, filter=BILINEAR_F32)
    w = d.words(5)
    assert len(w) == 4 * table_words(5) == 4 * (16 + 12 * 5)
    assert struct.unpack("<16i", w[:64]) == (2, 2) + (0,) * 14
    got = [struct.unpack("<12i", w[64 + 48 * k:64 + 48 * (k + 1)]) for k in range(5)]
    assert got[0] == rows[0] and got[1] == rows[1] and got[2] == got[3] == got[4] == (0,) * 12
    assert d.sources() == [1, 0] and d.flips() == [False, True] and (d.units, d.clip) == (2, True)
    d.check(300, 400, 2)
    with pytest.raises(ValueError, match="source clip"):
        d.check(300, 400, 1)
    # an image draw is what it was: 11 words, the 12th packed as zero, the bicubic code
    img = CropDraw([rows[0][:11][:6] + (256, 341, 16, 58, 0)])
    assert not img.clip and struct.unpack("<16i", img.words()[:64])[0] == 3 and struct.unpack("<12i", img.words()[64:])[11] == 0
    c = DeviceClipScaleJitterCrop().inject([d])
    assert c.draw_for([(300, 400), (64, 48)]) is d
    c.inject([d])
    with pytest.raises(ValueError):
        c.draw_for([(300, 400)])
    c = DeviceClipScaleJitterCrop().inject([img])
    with pytest.raises(ValueError, match="image rows"):
        c.draw_for([(300, 400)])
    p = probe_clip_draw([(300, 400), (64, 48)])
    assert p.clip and p.sources() == [0, 1] and p.rows[1][4:8] == (64, 48, 224, 224)


def test_every_refusal():
    from util.crop import (BILINEAR_F32, CropDraw, DeviceClipRandomResizedCrop, DeviceClipScaleJitterCrop, DeviceClipUniformCrop,
                           DeviceRandomResizedCrop, DeviceResizeCenterCrop, clip_row_error)
    assert clip_row_error(GOOD) is None and clip_row_error(GOOD, 2, 300, 400) is None
    assert clip_row_error(GOOD, 1) and clip_row_error(GOOD, 2, 299, 400) and clip_row_error(GOOD[:11])
    assert clip_row_error((600, 600, 0, 0, 561, 561, 224, 224, 0, 0, 0, 0)) is None            # no 2.5x bound
    for bad in (GOOD[:11], GOOD[:4] + (0,) + GOOD[5:], GOOD[:6] + ((1 << 23) + 1,) + GOOD[7:], GOOD[:11] + (-1,)):
        with pytest.raises(ValueError):
            CropDraw([GOOD, bad], filter=BILINEAR_F32)
    with pytest.raises(ValueError):
        CropDraw([GOOD], filter=1)
    with pytest.raises(ValueError):
        CropDraw([GOOD])                       # 12 words under the bicubic code
    for make in (lambda: DeviceClipScaleJitterCrop(size=192), lambda: DeviceClipScaleJitterCrop(interpolation="bicubic"),
                 lambda: DeviceClipRandomResizedCrop(size=(224, 192)), lambda: DeviceClipRandomResizedCrop(interpolation=3),
                 lambda: DeviceClipUniformCrop(size=256), lambda: DeviceClipUniformCrop(spatial_views=2), lambda: DeviceClipUniformCrop(interpolation="nearest")):
        with pytest.raises(NotImplementedError):
            make()
    for make in (lambda: DeviceClipScaleJitterCrop(scale_range=(0.9, 1.1)), lambda: DeviceClipScaleJitterCrop(scale_range=(1.2, 1.1)),
                 lambda: DeviceClipScaleJitterCrop(mirror=1.5), lambda: DeviceClipRandomResizedCrop(scale=(0.5, 0.1)),
                 lambda: DeviceClipRandomResizedCrop(ratio=(0.0, 1.0)), lambda: DeviceClipUniformCrop().draw_for([(0, 5)]),
                 lambda: DeviceClipUniformCrop().draw_for([])):
        with pytest.raises(ValueError):
            make()
    assert DeviceClipUniformCrop(size=(224, 224)).size == 224
    # the loops refuse the wrong kind of class, before any device work
    import engine_finetune as E
    from _lib import DyTError
    model = types.SimpleNamespace(input_norm=((0.5,) * 3, (0.5,) * 3), _frames=None)
    jit, uni, rrc, rcc = DeviceClipScaleJitterCrop(), DeviceClipUniformCrop(), DeviceRandomResizedCrop(), DeviceResizeCenterCrop()
    ns = types.SimpleNamespace
    assert E._device_crop(ns(device_crop=jit), "device_crop", DeviceRandomResizedCrop, model, video=True) is jit
    assert E._device_crop(ns(device_crop=DeviceClipRandomResizedCrop()), "device_crop", DeviceRandomResizedCrop, model, video=True) is not None
    assert E._device_crop(ns(device_eval_crop=uni), "device_eval_crop", DeviceResizeCenterCrop, model, video=True) is uni
    with pytest.raises(DyTError, match="crops video clips"):
        E._device_crop(ns(device_crop=jit), "device_crop", DeviceRandomResizedCrop, model)
    with pytest.raises(DyTError, match="crops video clips"):
        E._device_crop(ns(device_eval_crop=uni), "device_eval_crop", DeviceResizeCenterCrop, model)
    with pytest.raises(DyTError, match="video clips are not implemented"):
        E._device_crop(ns(device_crop=rrc), "device_crop", DeviceRandomResizedCrop, model, video=True)
    with pytest.raises(DyTError, match="video clips are not implemented"):
        E._device_crop(ns(device_eval_crop=rcc), "device_eval_crop", DeviceResizeCenterCrop, model, video=True)
    with pytest.raises(DyTError, match="DeviceClipUniformCrop"):
        E._device_crop(ns(device_eval_crop=jit), "device_eval_crop", DeviceResizeCenterCrop, model, video=True)
    with pytest.raises(DyTError, match="DeviceClipScaleJitterCrop"):
        E._device_crop(ns(device_crop=uni), "device_crop", DeviceRandomResizedCrop, model, video=True)
    with pytest.raises(DyTError, match="input_norm"):
        E._device_crop(ns(device_crop=jit), "device_crop", DeviceRandomResizedCrop, ns(input_norm=None), video=True)
    with pytest.raises(DyTError, match="image batches go through"):
        E._resample_batch(model, jit, torch.zeros(2, 64, 64, 3, dtype=torch.uint8))
    with pytest.raises(DyTError, match="image batches go through"):
        E._resample_batch(model, jit, torch.zeros(2, 3, 2, 64, 64, 3, dtype=torch.uint8))    # temporal views are evaluation's
    with pytest.raises(DyTError, match="uint8"):
        E._resample_batch(model, jit, torch.zeros(2, 2, 64, 64, 3))
    with pytest.raises(DyTError, match="image model"):
        E._resample_batch(ns(input_norm=model.input_norm, _frames=1), jit, torch.zeros(2, 2, 64, 64, 3, dtype=torch.uint8))
    with pytest.raises(DyTError, match="video clips"):
        E._resample_batch(model, rrc, torch.zeros(2, 4, 64, 64, 3, dtype=torch.uint8))


def test_pad_collate_clips():
    from util.crop import pad_collate_clips
    rng = np.random.default_rng(1)
    clips = [rng.integers(0, 256, (4, h, w, 3), dtype=np.uint8) for h, w in ((40, 64), (64, 33), (17, 23))]
    (out, sizes), labels = pad_collate_clips([(clips[0], 3), (torch.from_numpy(clips[1]), 1), (clips[2], 7)])
    assert out.dtype == torch.uint8 and tuple(out.shape) == (3, 4, 64, 64, 3) and out.is_contiguous()
    assert sizes.dtype == torch.int32 and sizes.tolist() == [[40, 64], [64, 33], [17, 23]]
    assert labels.dtype == torch.int64 and labels.tolist() == [3, 1, 7]
    for i, cl in enumerate(clips):
        assert np.array_equal(out[i, :, :cl.shape[1], :cl.shape[2]].numpy(), cl)
        assert int(out[i, :, cl.shape[1]:].sum()) == 0 and int(out[i, :, :, cl.shape[2]:].sum()) == 0
    (out, _), _ = pad_collate_clips([(clips[0], 0)], pad_to=(128, 96))
    assert tuple(out.shape) == (1, 4, 128, 96, 3)
    for bad in (lambda: pad_collate_clips([(clips[0], 0)], pad_to=(32, 96)), lambda: pad_collate_clips([(clips[0].astype(np.float32), 0)]),
                lambda: pad_collate_clips([(clips[0][0], 0)]), lambda: pad_collate_clips([(clips[0], 0), (clips[1][:2], 1)]),
                lambda: pad_collate_clips([(clips[0].transpose(0, 3, 1, 2), 0)]), lambda: pad_collate_clips([])):
        with pytest.raises(ValueError):
            bad()
