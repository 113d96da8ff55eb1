"""CPU tests of the on-device Random Erasing (dyt_set_erase, dyt_erase_images; util.erasing.DeviceRandomErasing): the header, the ctypes
binding and both libraries agree without a version or flag change; dynamic-tuning_amd/csrc/erase.h -- box test, run test, unit choice,
noise and every argument check -- is walked by tools/erase_check.cpp, built with the host compiler (its header gives the sanitizer build of
the same stand-alone program); the context-free entry refuses bad arguments without a device; DeviceRandomErasing reproduces the
reference's recorded boxes (tests/golden/erase/erase_draws.npz) draw for draw.  Nothing here needs a GPU; a missing compiler is a failure."""
import ctypes
import inspect
import os
import random
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import erase_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dynamic-tuning_amd", "csrc")
ENTRIES = {"dyt_set_erase", "dyt_erase_images"}
GOLDEN = os.path.join(ROOT, "tests", "golden", "erase", "erase_draws.npz")


def _header():
    return open(os.path.join(ROOT, "include", "dyt_hip.h")).read()


def _args(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


# ---- header, binding, libraries --------------------------------------------------------------------------------------------------------
def test_header_declares_the_entries_and_no_new_flag():
    h = _header()
    assert _args("dyt_set_erase") == ["dyt_ctx* ctx", "const void* table_dev", "int units_capacity", "int frames"]
    assert _args("dyt_erase_images") == ["const void* src", "float* dst", "int count", "int frames", "int src_kind", "const float mean[3]",
                                         "const float std[3]", "const void* table_dev", "const void* mix_params_dev", "void* stream"]
    values = [int(v) for v in re.findall(r"#define\s+DYT_F_[A-Z0-9_]+\s+(\d+)\b", h)]
    assert len(values) == len(set(values)) == 11   # erasing is context state, not a flag


def test_binding_equals_the_header_and_the_version_stays_5():
    import _lib
    declared = set(re.findall(r"\b(dyt_[a-z0-9_]+)\s*\(", _header()))
    assert ENTRIES <= declared
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    assert ENTRIES <= _lib.OPTIONAL_SYMBOLS   # discovered by symbol
    assert [len(_lib.SYMBOLS[n][1]) for n in ("dyt_set_erase", "dyt_erase_images")] == [4, 10]
    for fp16 in (False, True):
        L = _lib.lib(fp16=fp16)
        assert L.dyt_version() == 5
        assert all(hasattr(L, n) for n in ENTRIES)


def test_python_refuses_by_name_when_the_library_lacks_the_entries():
    import _lib
    import runtime
    for fn in (_lib.erase_images, runtime.DyTEngine.set_erase):
        src = inspect.getsource(fn)
        assert "hasattr(" in src and "rebuild it" in src


def test_erase_h_is_hip_free_and_fixes_the_strides():
    src = open(os.path.join(CSRC, "erase.h")).read()
    assert re.findall(r"#include\s*[<\"]([^>\"]+)", src) == ["math.h"]   # and that one for the host compiler only
    assert "hip" not in " ".join(re.findall(r"#include.*", src)).lower()
    assert "static_assert(sizeof(EraseRow) == ERASE_ROW_WORDS * 4" in src and "static_assert(sizeof(EraseHeader) == ERASE_HEADER_WORDS * 4" in src
    for fast in ("__logf", "__sinf", "__cosf", "__expf"):
        assert fast not in src   # the accurate functions
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\berase\.hip\b", mk, re.M)
    from util import erasing
    consts = dict(re.findall(r"\b(ERASE_[A-Z_]+) = (\d+)", src))
    assert (int(consts["ERASE_HEADER_WORDS"]), int(consts["ERASE_ROW_WORDS"]), int(consts["ERASE_MAX_BOXES"])) == (
        erasing.HEADER_WORDS, erasing.ROW_WORDS, erasing.MAX_BOXES) == (16, 20, 4)
    assert [int(consts[k]) for k in ("ERASE_OFF", "ERASE_CONST", "ERASE_RAND", "ERASE_PIXEL")] == [erasing.OFF, erasing.CONST, erasing.RAND, erasing.PIXEL] == [0, 1, 2, 3]


def test_table_layout():
    """EraseDraw.words() is csrc/erase.h's table: 16 header words, 20 words per unit, zero rows up to the capacity."""
    from util.erasing import EraseDraw, table_words
    d = EraseDraw("pixel", [[(1, 2, 3, 4)], [], [(0, 224, 0, 224), (223, 1, 223, 1)]], seed=0x1122334455667788, cube=True, frames=2)
    w = d.words(5)
    assert len(w) == 4 * table_words(5) == 4 * (16 + 20 * 5)
    assert struct.unpack("<4i2I", w[:24]) == (3, 2, 1, 3, 0x55667788, 0x11223344) and w[24:64] == b"\0" * 40
    rows = [struct.unpack("<20i", w[64 + 80 * k:64 + 80 * (k + 1)]) for k in range(5)]
    assert rows[0] == (1, 1, 2, 3, 4) + (0,) * 15
    assert rows[1] == (0,) * 20
    assert rows[2] == (2, 0, 224, 0, 224, 223, 1, 223, 1) + (0,) * 11
    assert rows[3] == rows[4] == (0,) * 20
    assert (d.units, d.images()) == (3, 6) and EraseDraw("const", [[]] * 4).images() == 4
    assert len(d.words()) == 4 * table_words(3)
    box = (0, 1, 0, 1)
    for bad in (lambda: EraseDraw(0, [[box]]), lambda: EraseDraw(4, [[box]]), lambda: EraseDraw("const", []), lambda: EraseDraw("const", [[box] * 5]),
                lambda: EraseDraw("const", [[(0, 0, 0, 1)]]), lambda: EraseDraw("const", [[(0, 1, 0, 0)]]), lambda: EraseDraw("const", [[(-1, 1, 0, 1)]]),
                lambda: EraseDraw("const", [[(1, 224, 0, 1)]]), lambda: EraseDraw("const", [[(0, 1, 224, 1)]]), lambda: EraseDraw("const", [[box]], frames=0),
                lambda: d.words(2)):
        with pytest.raises(ValueError):
            bad()


# ---- the entries refuse without a device -------------------------------------------------------------------------------------------------
def test_refusals_of_the_entries_need_no_device():
    import _lib
    for L in (_lib.lib(), _lib.lib(fp16=True)):
        m, s = _lib.float3((0.5, 0.5, 0.5)), _lib.float3((0.5, 0.5, 0.5))
        src, dst, tab, par = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000), ctypes.c_void_p(0x30000), ctypes.c_void_p(0x40000)
        bad = {
            "count 0": (src, dst, 0, 1, 0, m, s, tab, None),
            "frames 0": (src, dst, 2, 0, 0, m, s, tab, None),
            "count not a multiple of frames": (src, dst, 5, 2, 1, m, s, tab, None),
            "null src": (None, dst, 2, 1, 0, m, s, tab, None),
            "null dst": (src, None, 2, 1, 0, m, s, tab, None),
            "null table": (src, dst, 2, 1, 0, m, s, None, None),
            "misaligned table": (src, dst, 2, 1, 0, m, s, ctypes.c_void_p(0x30004), None),
            "misaligned byte pointer": (ctypes.c_void_p(0x10004), dst, 2, 1, 1, m, s, tab, None),
            "misaligned dst": (src, ctypes.c_void_p(0x20008), 2, 1, 0, m, s, tab, None),
            "src_kind 3": (src, dst, 2, 1, 3, m, s, tab, None),
            "src_kind -1": (src, dst, 2, 1, -1, m, s, tab, None),
            "bytes without statistics": (src, dst, 2, 1, 1, None, None, tab, None),
            "std 0": (src, dst, 2, 1, 2, m, _lib.float3((0.5, 0.0, 0.5)), tab, None),
            "mix with an odd count": (src, dst, 3, 1, 0, m, s, tab, par),
            "mix with odd clips": (src, dst, 6, 2, 0, m, s, tab, par),
            "misaligned mix block": (src, dst, 2, 1, 0, m, s, tab, ctypes.c_void_p(0x40004)),
        }
        for what, a in bad.items():
            assert L.dyt_erase_images(*a, None) == -1, what
            text = L.dyt_last_error()
            assert text and b"dyt_erase_images" in text, what
        assert L.dyt_set_erase(None, tab, 4, 1) == -1 and L.dyt_last_error()


# ---- csrc/erase.h through the host compiler ------------------------------------------------------------------------------------------------
def _cxx():
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler (CXX, c++, g++, clang++)"
    return cxx


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("erase") / "erase_check")
    subprocess.run([_cxx(), "-std=c++17", "-O2", "-I", CSRC, os.path.join(ROOT, "tools", "erase_check.cpp"), "-o", exe], check=True)
    return exe


def test_erase_h_walked_by_the_host_program(checker):
    p = subprocess.run([checker], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    for part in ("boxes ok", "units ok", "refusals ok", "noise ok", "all ok"):
        assert part in p.stdout, p.stdout


def test_the_header_noise_is_the_reference_noise(checker):
    """erase.h's noise on the host (glibc's logf / sinf / cosf) against the fp64 reference from the same Philox words, within the bound
    the GPU test uses: 4 x the fp32-to-fp64 deviation of the formula over these words."""
    seed, images = 0x9E3779B97F4A7C15, 3
    want, bound = R.pixel_noise(seed, images), R.noise_bound(seed, images)
    assert 0 < bound < 2e-5
    for (n, c, y, x4) in ((0, 0, 0, 0), (2, 1, 223, 55), (1, 2, 100, 17), (2, 0, 7, 31)):
        out = subprocess.run([checker, "noise", str(seed), str(n), str(c), str(y), str(x4)], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
        got = np.array([int(v, 16) for v in out], dtype=np.uint32).view(np.float32).astype(np.float64)
        assert np.abs(got - want[n, c, y, x4 * 4:x4 * 4 + 4]).max() <= bound
    col = R.box_colours(seed, images)
    for (n, box, c) in ((0, 0, 0), (1, 3, 1), (2, 2, 2)):
        out = subprocess.run([checker, "colour", str(seed), str(n), str(box), str(c)], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
        got = float(np.array([int(out[0], 16)], dtype=np.uint32).view(np.float32)[0])
        assert abs(got - col[n, box, c]) <= bound


# ---- DeviceRandomErasing ------------------------------------------------------------------------------------------------------------------
def test_signature_and_unsupported_options():
    from util.erasing import DeviceRandomErasing
    p = inspect.signature(DeviceRandomErasing.__init__).parameters
    assert list(p)[1:] == ["probability", "min_area", "max_area", "min_aspect", "max_aspect", "mode", "min_count", "max_count", "num_splits",
                           "cube", "generator"]
    assert [p[k].default for k in list(p)[1:]] == [0.5, 0.02, 1 / 3, 0.3, None, 'const', 1, None, 0, False, None]
    for kw in (dict(num_splits=2), dict(max_count=5), dict(min_count=5)):
        with pytest.raises(NotImplementedError):
            DeviceRandomErasing(**kw)
    with pytest.raises(ValueError):
        DeviceRandomErasing(mode="colour")
    import engine_finetune
    import runtime
    assert "erase" in inspect.signature(engine_finetune.train_step).parameters
    assert list(inspect.signature(runtime.DyTEngine.erase_images).parameters)[1:] == ["images", "draw", "mix"]


def _golden():
    g = np.load(GOLDEN)
    names = sorted(k[:-5] for k in g.files if k.endswith("_mask"))
    assert names == ["p100_area100", "p25_count1", "p25_count1to3", "p50_cube"]
    return g, names


def _eraser(cfg, rng):
    from util.erasing import DeviceRandomErasing
    seed, units, frames, cube, prob, max_area, lo, hi = cfg.tolist()
    return DeviceRandomErasing(probability=prob, max_area=max_area, min_count=int(lo), max_count=int(hi), cube=bool(cube), generator=rng), int(units), int(frames)


def test_the_golden_holds_what_it_must():
    g, names = _golden()
    assert (g["p25_count1_boxes"] == 0).any() and int((g["p25_count1_boxes"] > 0).sum()) == 6   # untouched and erased images
    assert (g["p25_count1to3_boxes"] >= 2).any()                                                  # 2 or more boxes
    assert (g["p100_area100_attempts"] > g["p100_area100_boxes"]).any()                           # rejected attempts
    assert os.path.getsize(GOLDEN) < 64 * 1024


def test_a_seeded_generator_reproduces_the_references_boxes_and_its_next_draw():
    g, names = _golden()
    for name in names:
        cfg = g[name + "_cfg"]
        rng = random.Random(int(cfg[0]))
        eraser, units, frames = _eraser(cfg, rng)
        boxes = eraser.draw_boxes(units)
        assert rng.random() == float(g[name + "_next"]), name          # exactly the reference's number of draws was consumed
        assert [len(b) for b in boxes] == g[name + "_boxes"].tolist(), name
        # and through draw(): the same boxes, the seed taken after them
        rng2 = random.Random(int(cfg[0]))
        eraser2, _, _ = _eraser(cfg, rng2)
        d = eraser2.draw_for(units * frames, frames)
        assert d.boxes == [list(b) for b in boxes] and d.units == units and d.images() == units * frames
        check = random.Random(int(cfg[0]))
        _eraser(cfg, check)[0].draw_boxes(units)
        assert d.seed == check.getrandbits(64)
        mask = np.unpackbits(g[name + "_mask"]).astype(bool).reshape(units * frames, 224, 224)
        assert np.array_equal(R.hit_map(d, units * frames) >= 0, mask), name


def test_draws_injection_and_seeds():
    from util.erasing import DeviceRandomErasing, EraseDraw
    a = DeviceRandomErasing(probability=0.7, max_count=3, mode="pixel", generator=5)
    b = DeviceRandomErasing(probability=0.7, max_count=3, mode="pixel", generator=random.Random(5))
    da, db = [a.draw(8) for _ in range(6)], [b.draw(8) for _ in range(6)]
    assert [d.words() for d in da] == [d.words() for d in db]
    assert len({d.seed for d in da}) == 6 and all(d.mode == 3 and not d.cube and d.frames == 1 for d in da)
    assert [d.words() for d in da] != [DeviceRandomErasing(probability=0.7, max_count=3, mode="pixel", generator=6).draw(8).words() for _ in range(6)]
    fixed = EraseDraw("rand", [[(0, 1, 0, 1)], []], seed=9)
    e = DeviceRandomErasing(generator=1).inject([fixed])
    assert e.draw(2) is fixed
    assert e.draw(2).words() == DeviceRandomErasing(generator=1).draw(2).words()   # then the generator, from its start
    with pytest.raises(ValueError):
        DeviceRandomErasing(generator=1).inject([fixed]).draw(3)
    c = DeviceRandomErasing(probability=1.0, cube=True, generator=3).draw_for(8, 2)
    assert (c.units, c.cube, c.frames, c.images()) == (4, True, 2, 8)
    with pytest.raises(ValueError):
        DeviceRandomErasing(cube=True).draw_for(7, 2)


def test_args_build_the_eraser_the_reference_pipeline_asks_for():
    import engine_finetune as E
    from util.erasing import DeviceRandomErasing

    class A:
        pass
    a = A()
    assert E._device_erasing(None) is None and E._device_erasing(a) is None
    a.reprob, a.remode, a.recount = 0.25, "pixel", 1
    assert E._device_erasing(a) is None            # the reference's names alone switch nothing on
    a.device_erase = True
    e = E._device_erasing(a)
    assert isinstance(e, DeviceRandomErasing) and (e.probability, e.mode, e.min_count, e.max_count, e.cube) == (0.25, "pixel", 1, 1, False)
    assert E._device_erasing(a) is e               # one generator for the run
    b = A()
    b.reprob, b.remode, b.recount, b.device_erase = 0.25, "pixel", 1, True
    assert E._device_erasing(b, cube_default=True).cube is True
    own = DeviceRandomErasing(mode="rand")
    a.random_erasing = own
    assert E._device_erasing(a) is own
    a.random_erasing = object()
    with pytest.raises(Exception):
        E._device_erasing(a)
