"""CPU tests of the device RandAugment (dyt_randaug_u8, dyt_randaug_table; util.randaug): the header, the ctypes binding and both libraries
agree without a version or flag change; dynamic-tuning_amd/csrc/randaug.h -- row check, table builders, blend, SMOOTH, the affine gather with
both filters and every argument check -- is walked by tools/randaug_check.cpp, built with the host compiler (plainly and with
-fsanitize=address,undefined), against the reference's recorded tables and pixels; the entries refuse bad arguments without a device;
DeviceRandAugment reproduces the reference's recorded draws (tests/golden/randaug/randaug.npz) draw for draw, and the draw after them;
AugDraw's check agrees with the header's on hostile rows; the table words, the buffer bookkeeping and the launch masks.  Nothing here needs a
GPU; a missing compiler is a failure."""
import ctypes
import inspect
import math
import os
import random
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import randaug_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dynamic-tuning_amd", "csrc")
ENTRIES = {"dyt_randaug_u8", "dyt_randaug_table"}
GOLDEN = os.path.join(ROOT, "tests", "golden", "randaug", "randaug.npz")


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


def _header():
    return open(os.path.join(ROOT, "include", "dyt_hip.h")).read()


def _args(name, ret="int"):
    m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (ret, name), _header())
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


# ---- header, binding, libraries --------------------------------------------------------------------------------------------------------
def test_header_declares_the_entries_and_the_binding_equals_it():
    import _lib
    import runtime
    assert _args("dyt_randaug_u8") == ["const uint8_t* src", "int units", "int frames", "int src_h", "int src_w", "uint8_t* dst", "uint8_t* work",
                                       "int32_t* stats", "const void* table_dev", "int capacity", "int layers", "const uint32_t* launch_mask", "void* stream"]
    assert _args("dyt_randaug_table")[-5:] == ["int unit", "int frame", "int layer", "int32_t* out_dev", "void* stream"]
    declared = set(re.findall(r"\b(dyt_[a-z0-9_]+)\s*\(", _header()))
    assert ENTRIES <= declared and declared == set(_lib.SYMBOLS)
    assert ENTRIES <= _lib.OPTIONAL_SYMBOLS   # discovered by symbol
    assert [len(_lib.SYMBOLS[n][1]) for n in ("dyt_randaug_u8", "dyt_randaug_table")] == [len(_args("dyt_randaug_u8")), len(_args("dyt_randaug_table"))]
    for fp16 in (False, True):
        L = _lib.lib(fp16=fp16)
        assert L.dyt_version() == 5 and all(hasattr(L, n) for n in ENTRIES)
    for fn in (_lib._randaug_args, _lib.randaug_table, runtime.DyTEngine.randaug):
        src = inspect.getsource(fn)
        assert "hasattr(" in src and "rebuild it" in src


def test_randaug_h_is_hip_free_and_one_definition():
    from util import randaug
    import _lib
    src = open(os.path.join(CSRC, "randaug.h")).read()
    assert re.findall(r"#include\s*[<\"]([^>\"]+)", src) == ["stdint.h", "resample.h"]
    assert "__global__" not in src and "hip" not in src.lower().replace("hip-free", "").replace("hip type", "").replace("randaug.hip", "")
    assert src.count("#pragma clang fp contract(off)") >= 8 and "fma(" not in src and "fmaf(" not in src
    kernel = open(os.path.join(CSRC, "randaug.hip")).read()
    assert '#include "randaug.h"' in kernel and "contract" not in kernel
    for fn in ("aug_row_ok", "aug_build_table", "aug_contrast_mean", "aug_blend", "aug_smooth", "aug_affine_pixel", "aug_luma"):
        assert fn + "(" in kernel and fn + "(" in src                     # the kernels call the header's functions
    assert "atomicAdd" in kernel and not re.search(r"atomicAdd\(\s*\(?\s*float", kernel)
    tool = open(os.path.join(ROOT, "tools", "randaug_check.cpp")).read()
    assert '#include "randaug.h"' in tool and "int main(" in tool
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\brandaug\.hip\b", mk, re.M) and "contract" not in mk
    assert mk.count("CXXFLAGS =") == 1 and "-O3 -std=c++17 -fPIC -Wno-unused-result -Wno-unused-value $(CXXFLAGS_EXTRA)" in mk   # no new flag
    consts = dict(re.findall(r"\b(AUG_[A-Z0-9_]+) = ([0-9a-fx]+)[;,]", src))
    assert int(consts["AUG_MAGIC"], 16) == randaug.MAGIC and int(consts["AUG_HEADER_WORDS"]) == randaug.HEADER_WORDS == _lib.RANDAUG_HEADER_WORDS
    assert int(consts["AUG_ROW_WORDS"]) == randaug.ROW_WORDS == _lib.RANDAUG_ROW_WORDS == len(randaug.pack_row(randaug.aug_row(0, 1, 1))) // 4
    assert int(consts["AUG_MAX_LAYERS"]) == randaug.MAX_LAYERS == _lib.RANDAUG_MAX_LAYERS and int(consts["AUG_BILINEAR"]) == randaug.BILINEAR == R.BILINEAR
    order = re.search(r"enum AugOp \{([^}]*)\}", src).group(1).replace("= 0", "").replace(" ", "").replace("\n", "").split(",")
    assert [o[4:].replace("_", "").lower() for o in order[:-1]] == [n.lower() for n in randaug.OP_NAMES] == [n.lower() for n in R.OP_NAMES]
    assert randaug.HIST_WORDS == _lib.RANDAUG_HIST_WORDS == 1024 and randaug.TABLE_WORDS == _lib.RANDAUG_TABLE_WORDS == 769


def test_refusals_of_the_entries_need_no_device():
    import _lib
    for L in (_lib.lib(), _lib.lib(fp16=True)):
        src, dst, work, stats, tab = (ctypes.c_void_p(v) for v in (0x10000, 0x20000, 0x30000, 0x40000, 0x50000))
        ok = dict(src=src, units=2, frames=2, h=64, w=64, dst=dst, work=work, stats=stats, tab=tab, cap=4, layers=4)
        bad = {"null src": dict(src=None), "null dst": dict(dst=None), "null work": dict(work=None), "null stats": dict(stats=None), "null table": dict(tab=None),
               "misaligned src": dict(src=ctypes.c_void_p(0x10008)), "misaligned dst": dict(dst=ctypes.c_void_p(0x20004)),
               "misaligned work": dict(work=ctypes.c_void_p(0x30002)), "misaligned stats": dict(stats=ctypes.c_void_p(0x40004)),
               "misaligned table": dict(tab=ctypes.c_void_p(0x50004)), "src == dst": dict(dst=src), "work == dst": dict(work=dst), "work == src": dict(work=src),
               "units 0": dict(units=0), "frames 0": dict(frames=0), "layers 0": dict(layers=0), "layers 9": dict(layers=9), "units above capacity": dict(units=5),
               "capacity 0": dict(cap=0, units=1), "units * frames above 65535": dict(units=256, frames=256, cap=256), "units above 65535": dict(units=65536, frames=1, cap=70000),
               "side 0": dict(h=0), "width 0": dict(w=0), "side above 4096": dict(w=4097), "height above 4096": dict(h=4097), "negative": dict(units=-1)}
        for what, change in bad.items():
            a = dict(ok, **change)
            rc = L.dyt_randaug_u8(a["src"], a["units"], a["frames"], a["h"], a["w"], a["dst"], a["work"], a["stats"], a["tab"], a["cap"], a["layers"], None, None)
            assert rc == -1, what
            text = L.dyt_last_error()
            assert text and b"dyt_randaug_u8: randaug:" in text, (what, text)
        out = ctypes.c_void_p(0x60000)
        for what, a in {"null src": (None, 2, 2, 64, 64, stats, tab, 4, 4, 0, 0, 0, out), "null out": (src, 2, 2, 64, 64, stats, tab, 4, 4, 0, 0, 0, None),
                        "unit 2 of 2": (src, 2, 2, 64, 64, stats, tab, 4, 4, 2, 0, 0, out), "frame -1": (src, 2, 2, 64, 64, stats, tab, 4, 4, 0, -1, 0, out),
                        "layer 4 of 4": (src, 2, 2, 64, 64, stats, tab, 4, 4, 0, 0, 4, out), "side above 4096": (src, 2, 2, 5000, 64, stats, tab, 4, 4, 0, 0, 0, out),
                        "misaligned out": (src, 2, 2, 64, 64, stats, tab, 4, 4, 0, 0, 0, ctypes.c_void_p(0x60004))}.items():
            assert L.dyt_randaug_table(*a, None) == -1, what
            text = L.dyt_last_error()
            assert text and b"dyt_randaug_table" in text, what


# ---- csrc/randaug.h through the host compiler ----------------------------------------------------------------------------------------------
def _cxx():
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler (CXX, c++, g++, clang++)"
    return cxx


@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    d = tmp_path_factory.mktemp("randaug")
    plain, san = str(d / "randaug_check"), str(d / "randaug_check_san")
    tool = os.path.join(ROOT, "tools", "randaug_check.cpp")
    subprocess.run([_cxx(), "-std=c++17", "-O2", "-I", CSRC, tool, "-o", plain], check=True)
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, tool, "-o", san], check=True)
    return plain, san


def test_randaug_h_walked_by_the_host_program_plain_and_sanitized(checkers):
    for exe in checkers:
        p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert p.returncode == 0, p.stdout
        for part in ("rows ok", "arithmetic ok", "refusals ok", "all ok"):
            assert part in p.stdout, p.stdout


def _ints(a):
    return " ".join(str(int(v)) for v in np.asarray(a).ravel())


def test_the_headers_tables_and_pixels_equal_the_references_recorded_ones(checkers, g, tmp_path):
    """Every golden case, frame 0: the table builders against the tables observed from Pillow's output, the Contrast constants, and each
    operation's pixels (both filters of the affine ones) through the header's functions on the CPU."""
    lines = []
    ops, iargs = g["case_row_op"], g["case_row_iarg"]
    for n, k in enumerate(g["tab_case"]):
        for f in range(2):
            for c in range(3):
                lines += ["T %d %d" % (ops[k], iargs[k]), _ints(g["tab_hist"][n, f, c]), _ints(g["tab_lut"][n, f, c])]
    for n in range(len(g["con_case"])):
        for f in range(2):
            lines += ["C %d" % g["con_mean"][n, f], _ints(g["con_hist"][n, f])]
    frames = 0
    for k in range(len(ops)):
        i = int(g["case_src"][k])
        h, w = (int(v) for v in g["px_sizes"][i])
        for f in range(2):
            lines += ["P %d %d %s %d %s %d %d" % (ops[k], iargs[k], float(np.float32(g["case_row_factor"][k])).hex(), g["case_row_filter"][k],
                                                " ".join(float(c).hex() for c in g["case_row_coeffs"][k]), h, w),
                      _ints(g["px_src"][i, f, :h, :w]), _ints(g["case_out"][k, f, :h, :w])]
            frames += 1
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    for exe in checkers:
        p = subprocess.run([exe, "file", str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert p.returncode == 0, p.stdout[-3000:]
        assert "file ok (%d tables, %d means, %d frames, 0 bytes differ)" % (6 * len(g["tab_case"]), 2 * len(g["con_case"]), frames) in p.stdout, p.stdout


# ---- draws ---------------------------------------------------------------------------------------------------------------------------------
def _recorded(g, prefix, names):
    return [[(names[o], bool(a), None if math.isnan(v) else v) for o, a, v in zip(ro, ra, rv)] for ro, ra, rv in zip(g[prefix + "_op"], g[prefix + "_applied"], g[prefix + "_arg"])]


@pytest.mark.parametrize("own_generators", [False, True])
def test_the_class_reproduces_the_references_recorded_draws_and_the_draw_after_them(g, own_generators):
    from util.randaug import DeviceRandAugment
    names, sizes = g["names"].tolist(), [tuple(int(v) for v in s) for s in g["sizes"]]
    for seed in (0, 1234):
        if own_generators:
            py, nprng = random.Random(seed), np.random.RandomState(seed)
        else:
            py, nprng = None, None
            random.seed(seed)
            np.random.seed(seed)
        got = []
        for (h, w) in sizes:   # one transform per clip, as the reference's dataset builds it
            aug = DeviceRandAugment.from_reference((h, w), str(g["config"]), "bicubic", py_rng=py, np_rng=nprng)
            assert aug.translate_const == int(min(h, w) * 0.45) and aug.fill == (128, 128, 128) and aug.interpolation == 3
            got.append(aug.draw_unit(h, w))
        want = _recorded(g, "draw%d" % seed, names)
        assert got == want, [(a, b) for a, b in zip(got, want) if a != b][:2]
        nxt = [(py or random).random(), (nprng or np.random).uniform()]
        assert nxt == g["draw%d_next" % seed].tolist()
        applied = g["draw%d_filter" % seed][g["draw%d_applied" % seed] == 1]
        assert (applied == 3).all() and (g["draw%d_filter" % seed][g["draw%d_applied" % seed] == 0] == 0).all()


def test_inc0_selects_the_increasing_set_and_no_mstd_draws_no_gauss(g):
    from util.randaug import DeviceRandAugment, RAND_INCREASING_TRANSFORMS, RAND_TRANSFORMS, parse_config
    assert list(RAND_INCREASING_TRANSFORMS) == g["names"].tolist() == g["inc0_names"].tolist() and list(RAND_TRANSFORMS) == g["names_plain"].tolist()
    assert parse_config("rand-m9-n2-inc0") == (9, 2, 0, RAND_INCREASING_TRANSFORMS) and parse_config("rand-m9-n2")[3] == RAND_TRANSFORMS
    assert parse_config("rand-m7-n4-mstd0.5-inc1") == (7, 4, 0.5, RAND_INCREASING_TRANSFORMS) and parse_config("rand") == (10.0, 2, 0, RAND_TRANSFORMS)
    assert parse_config("rand-mstd1-mstd2-n8")[1:3] == (8, 1.0)   # the first mstd wins (hparams.setdefault)
    random.seed(3)
    np.random.seed(3)
    aug = DeviceRandAugment(str(g["config_inc0"]), interpolation="bicubic")
    sizes = [tuple(int(v) for v in s) for s in g["sizes"]]
    got = [aug.draw_unit(h, w) for (h, w) in sizes]
    assert got == _recorded(g, "inc0", g["names"].tolist())
    assert [random.random(), np.random.uniform()] == g["inc0_next"].tolist()
    for bad, exc in (("rand-w0", NotImplementedError), ("rand-n9", NotImplementedError), ("rand-n0", NotImplementedError), ("rand-q3", NotImplementedError), ("augmix-m3", ValueError)):
        with pytest.raises(exc):
            DeviceRandAugment(bad)
    with pytest.raises(NotImplementedError, match="random"):
        DeviceRandAugment("rand-m9", interpolation="random")
    with pytest.raises(NotImplementedError):
        DeviceRandAugment.from_reference((224, 224), "rand-m9", "lanczos")
    with pytest.raises(NotImplementedError):
        DeviceRandAugment.from_reference((224, 224), "rand-m9", "random")
    assert DeviceRandAugment.from_reference((8, 240, 320), "rand-m9", "bilinear").interpolation == 2
    assert DeviceRandAugment.from_reference(224, "rand-m9", "nearest").translate_const == 100


def test_device_rows_of_a_draw_equal_the_rows_the_golden_cases_were_recorded_with(g):
    """``device_row(name, arg, h, w)`` -- the 24 names onto the 12 operations, Rotate's matrix from (h, w), TranslateRel's pct * size --
    gives the rows the reference's pixels were recorded with; ``draw_for`` assembles them and a skipped op is an Identity."""
    from util.randaug import AFFINE, IDENTITY, OPS, AugDraw, DeviceRandAugment, aug_row
    assert len(OPS) == 24 and {v[0] for v in OPS.values()} | {IDENTITY} == set(range(12))
    for k, name in enumerate(g["case_name"].tolist()):
        h, w = (int(v) for v in g["px_sizes"][g["case_src"][k]])
        filt = int(g["case_row_filter"][k])
        aug = DeviceRandAugment("rand-m9", interpolation="bilinear" if filt == 2 else "bicubic")
        op = int(g["case_row_op"][k])
        arg = None if OPS[name][1] is None else (g["case_row_iarg"][k] if op in (R.SOLARIZE, R.SOLARIZE_ADD, R.POSTERIZE) else float(g["case_row_factor"][k]))
        if OPS[name][0] == AFFINE:   # the level argument is not in the row: recover it from the coefficients the recipe built
            c = g["case_row_coeffs"][k]
            arg = {"ShearX": c[1], "ShearY": c[3], "TranslateXRel": c[2] / w, "TranslateYRel": c[5] / h}.get(name)
            if name == "Rotate":
                arg = next(d for d in (21.0, -13.7, 30.0, -7.5, 0.0) if (R.rotate_coeffs(d, h, w) or R.NO_COEFFS) == tuple(c.tolist()))
        got = aug.device_row(name, arg, h, w)
        want = aug_row(op, h, w, int(g["case_row_iarg"][k]), float(g["case_row_factor"][k]), g["case_row_coeffs"][k].tolist(), filt if op == AFFINE else got[4])
        if name.startswith("Translate"):
            assert got[:3] == want[:3] and np.allclose(got[3], want[3], rtol=1e-15, atol=0) and got[4:] == want[4:]   # (c / w) * w
        else:
            assert got == want, (name, got, want)
    aug = DeviceRandAugment("rand-m7-n4-mstd0.5-inc1", py_rng=random.Random(5), np_rng=np.random.RandomState(5))
    d = aug.draw_for([(48, 64), (33, 57)])
    assert isinstance(d, AugDraw) and d.units == 2 and d.layers == 4 and d.sizes() == [(48, 64), (33, 57)]
    twin = DeviceRandAugment("rand-m7-n4-mstd0.5-inc1", py_rng=random.Random(5), np_rng=np.random.RandomState(5))
    units = [twin.draw_unit(48, 64), twin.draw_unit(33, 57)]
    assert [[n for n in row] for row in d.names()] == [[("Identity" if not a or (nm == "Rotate" and v % 360.0 == 0) else R.OP_NAMES[OPS[nm][0]]) for nm, a, v in u] for u in units]
    fixed = AugDraw([aug_row(R.INVERT, 5, 6)], 1)
    assert aug.inject(fixed).draw_for([(5, 6)]) is fixed and aug.inject([fixed]).draw_for([(5, 6)]) is fixed
    with pytest.raises(ValueError, match="injected"):
        aug.inject(fixed).draw_for([(5, 7)])


# ---- AugDraw -------------------------------------------------------------------------------------------------------------------------------
def test_check_agrees_with_the_headers_row_check_on_hostile_rows(checkers):
    from util.randaug import AugDraw, aug_row, pack_row, row_error
    big = 2 ** 31 - 1
    good = [aug_row(op, 33, 57, iarg=3 if op in (R.SOLARIZE, R.SOLARIZE_ADD, R.POSTERIZE) else 0, factor=0.7, coeffs=(1, 0.2, -3, 0, 1, 4.5)) for op in range(12)]
    good += [aug_row(R.SOLARIZE, 64, 80, iarg=256), aug_row(R.SOLARIZE_ADD, 1, 1, iarg=255), aug_row(R.POSTERIZE, 64, 80, iarg=8), aug_row(R.AFFINE, 64, 80, filter=2),
             aug_row(R.AFFINE, 64, 80, coeffs=(2.0 ** 40, -2.0 ** 40, 0, 0, 5e-324, 0)), aug_row(R.COLOR, 64, 80, factor=-3.0e38), aug_row(R.AFFINE, 2, 2, fill=(0, 255, 7))]
    base = aug_row(R.AFFINE, 33, 57, factor=0.5)

    def change(**kw):
        r = dict(zip(("op", "iarg", "factor", "coeffs", "filter", "fill", "h", "w"), base))
        r.update(kw)
        return (r["op"], r["iarg"], r["factor"], tuple(r["coeffs"]), r["filter"], tuple(r["fill"]), r["h"], r["w"])
    hostile = [change(h=0), change(w=0), change(h=65), change(w=81), change(h=-1), change(h=big), change(w=-big - 1), change(op=12), change(op=-1), change(op=big),
               change(iarg=-1), change(iarg=257), change(op=R.SOLARIZE_ADD, iarg=256), change(op=R.POSTERIZE, iarg=9), change(filter=0), change(filter=1), change(filter=4),
               change(filter=-big), change(fill=(-1, 0, 0)), change(fill=(0, 0, 300)), change(factor=float("nan")), change(factor=float("inf")), change(factor=float("-inf")),
               change(coeffs=(float("nan"), 0, 0, 0, 1, 0)), change(coeffs=(1, 0, float("inf"), 0, 1, 0)), change(coeffs=(1, 0, 0, 0, 1, 2.0 ** 41)),
               change(coeffs=(1, 0, 0, -1e300, 1, 0))]
    plain = checkers[0]
    for r in good + hostile:
        words = struct.unpack("<20I", pack_row(r))
        p = subprocess.run([plain, "row", "0", "64", "80"] + ["%x" % v for v in words], stdout=subprocess.PIPE, text=True, check=True)
        assert (p.stdout.strip() == "1") == (row_error(r, 64, 80) is None) == (r in good), (r, p.stdout, row_error(r, 64, 80))
    for r in hostile:
        with pytest.raises(ValueError, match="randaug: unit 0, layer 0"):
            AugDraw([r], 1).check(64, 80)
    with pytest.raises(ValueError, match="disagree"):
        AugDraw([aug_row(R.INVERT, 5, 6), aug_row(R.INVERT, 5, 7)], 2)
    for rows, layers in (([], 1), ([good[0]] * 3, 2), ([good[0]], 0), ([good[0]] * 9, 9), ([good[0][:7]], 1)):
        with pytest.raises(ValueError):
            AugDraw(rows, layers)


def test_words_buffers_and_launch_masks():
    from util.randaug import (BUF_DST, BUF_SRC, BUF_WORK, FAM_AFFINE, FAM_BLEND, FAM_SHARP, FAM_TABLE, LAUNCH_STATS, MAGIC, AugDraw, aug_row, table_words)
    S, D, W = BUF_SRC, BUF_DST, BUF_WORK
    aff, inv, ident, sharp, con, eq = (aug_row(op, 33, 57, factor=0.5, coeffs=(1, 0.1, 0, 0, 1, 0)) for op in (R.AFFINE, R.INVERT, R.IDENTITY, R.SHARPNESS, R.CONTRAST, R.EQUALIZE))
    d = AugDraw([aff, inv, inv, aff, ident, ident, aff, sharp], 2)
    assert d.units == 4 and d.buffers() == [(S, D), (D, D), (S, W), (W, D), (S, D), (D, D), (S, W), (W, D)]
    assert d.launch_mask() == [1 << FAM_AFFINE | 1 << FAM_TABLE, 1 << FAM_TABLE | 1 << FAM_AFFINE | 1 << FAM_SHARP]
    four = AugDraw([aff, sharp, con, aff, ident, ident, ident, ident, eq, con, inv, sharp], 4)
    assert four.buffers() == [(S, D), (D, W), (W, W), (W, D)] + [(S, D), (D, D), (D, D), (D, D)] + [(S, W), (W, W), (W, W), (W, D)]
    for u in range(four.units):   # the properties the kernels check: layer 0 reads the source, the layers link, the last one writes dst
        b = four.buffers()[u * 4:(u + 1) * 4]
        assert b[0][0] == S and b[-1][1] == D and all(b[k][0] == b[k - 1][1] for k in range(1, 4)) and all(s != S for s, _ in b[1:])
        for (s, t), r in zip(b, four.unit_rows(u)):
            assert (s != t) if r[0] in (R.AFFINE, R.SHARPNESS) else (s == t or s == S)
    assert four.launch_mask() == [1 << FAM_AFFINE | 1 << FAM_TABLE | LAUNCH_STATS, 1 << FAM_SHARP | 1 << FAM_BLEND | LAUNCH_STATS,
                                  1 << FAM_BLEND | 1 << FAM_TABLE | LAUNCH_STATS, 1 << FAM_AFFINE | 1 << FAM_SHARP]
    words = d.words(6)
    assert len(words) == 4 * table_words(6, 2) == 4 * (16 + 20 * 6 * 2)
    assert struct.unpack("<16i", words[:64]) == (MAGIC, 4, 2) + (0,) * 13
    row = lambda layer, u: struct.unpack("<6ifi6d", words[64 + 80 * (layer * 6 + u):64 + 80 * (layer * 6 + u) + 80])   # noqa: E731
    assert row(0, 0) == (R.AFFINE, 33, 57, 0, 3, 128 | 128 << 8 | 128 << 16, 0.5, S | D << 8, 1.0, 0.1, 0.0, 0.0, 1.0, 0.0)
    assert row(1, 1)[0] == R.AFFINE and row(1, 1)[7] == W | D << 8 and row(0, 1)[7] == S | W << 8 and row(1, 3)[0] == R.SHARPNESS
    assert not any(words[64 + 80 * 4:64 + 80 * 6]) and not any(words[64 + 80 * 10:])   # zero rows behind the draw's units, in both layers
    assert d.words() == AugDraw(d.rows, 2).words(4)
    with pytest.raises(ValueError, match="holds 4 units"):
        d.words(3)
