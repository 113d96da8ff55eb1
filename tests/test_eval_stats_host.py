"""CPU tests of the streaming-evaluation entries (dyt_eval_rows, dyt_eval_keep): the header, the ctypes binding and both libraries agree without
a version change; dynamic-tuning_amd/csrc/eval_stats.h includes nothing and is walked lane by lane by tools/eval_stats_check.cpp, built with
the host compiler under AddressSanitizer / UBSan; the two entries refuse bad arguments without a device.  Nothing here needs a GPU; a missing
compiler is a failure."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dynamic-tuning_amd", "csrc")
ENTRIES = {"dyt_eval_rows", "dyt_eval_keep"}


def _header():
    return open(os.path.join(ROOT, "include", "dyt_hip.h")).read()


def _args(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_entries():
    assert _args("dyt_eval_rows") == ["const float* logits", "int64_t ld", "const int64_t* labels", "int rows", "int classes", "int64_t* counts",
                                      "int64_t* per_class", "double* loss_sum", "int32_t* row_rank", "float* row_loss", "void* stream"]
    assert _args("dyt_eval_keep") == ["const float* token_select", "int images", "int layers", "int tokens", "int64_t* counts", "void* stream"]


def test_binding_equals_the_header_and_the_version_stays_5():
    import _lib
    declared = set(re.findall(r"\b(dyt_[a-z0-9_]+)\s*\(", _header()))
    assert ENTRIES <= declared
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    assert ENTRIES <= _lib.OPTIONAL_SYMBOLS   # discovered by symbol
    assert [len(_lib.SYMBOLS[n][1]) for n in ("dyt_eval_rows", "dyt_eval_keep")] == [11, 6]
    assert _lib.SYMBOLS["dyt_eval_rows"][1][1] is ctypes.c_int64   # ld
    for fp16 in (False, True):
        L = _lib.lib(fp16=fp16)
        assert L.dyt_version() == 5
        assert all(hasattr(L, n) for n in ENTRIES)


def test_layout_constants_agree_in_the_three_places():
    """csrc/eval_stats.h == DYT_EVAL_* of the public header == _lib.EVAL_*."""
    import _lib
    src = open(os.path.join(CSRC, "eval_stats.h")).read()
    h = _header()

    def internal(name):
        m = re.search(r"\b%s\s*=\s*([A-Z_0-9 +]+?)\s*[,;]" % name, src)
        assert m, name
        return m.group(1)
    want = dict(HEAD_WORDS=8, ROWS=0, IGNORED=1, NAN_ROWS=2, MASK_ROWS=3, RANK_BINS=16, OFF_RANK=8, OFF_KEEP=24)
    for name, v in want.items():
        m = re.search(r"#define\s+DYT_EVAL_%s\s+(\d+)\b" % name, h)
        assert m and int(m.group(1)) == v, name
        assert getattr(_lib, "EVAL_" + name) == v, name
    assert [internal("EVAL_" + n) for n in ("HEAD_WORDS", "ROWS", "IGNORED", "NAN_ROWS", "MASK_ROWS", "RANK_BINS")] == ["8", "0", "1", "2", "3", "16"]
    assert internal("EVAL_OFF_RANK") == "EVAL_HEAD_WORDS" and internal("EVAL_OFF_KEEP") == "EVAL_OFF_RANK + EVAL_RANK_BINS"
    assert _lib.eval_counts_words(12, 196) == 24 + 12 * 197
    assert _lib.eval_counts_words(12, 196) * 8 == 19104   # the "19 KB" of the all-reduce


def test_python_refuses_by_name_when_the_library_lacks_the_entries():
    import _lib
    for fn in (_lib.eval_rows, _lib.eval_keep):
        src = inspect.getsource(fn)
        assert "hasattr(" in src and "rebuild it" in src


def test_eval_stats_h_includes_nothing_and_is_in_the_makefile():
    src = open(os.path.join(CSRC, "eval_stats.h")).read()
    assert "#include" not in src   # no HIP header: a plain host compiler reads it
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\beval_stats\.hip\b", mk, re.M)
    hip = open(os.path.join(CSRC, "eval_stats.hip")).read()
    adds = re.findall(r"atomicAdd\(([^;]*)\);", hip)   # no float atomic: every add is an integer, the loss goes through the fold's tree
    assert len(adds) >= 6 and all(a.rstrip().endswith(("1u", "1ull", "(unsigned long long)images")) for a in adds), adds


def test_refusals_need_no_device():
    import _lib
    for fp16 in (False, True):
        L = _lib.lib(fp16=fp16)
        P = ctypes.c_void_p
        lg, lb, cn, pc, ls, rr, rl = (P(0x10000 * k) for k in range(1, 8))
        good = (lg, 10, lb, 4, 10, cn, pc, ls, rr, rl)
        bad_rows = {
            "null logits": (None,) + good[1:],
            "null labels": good[:2] + (None,) + good[3:],
            "null counts": good[:5] + (None,) + good[6:],
            "null loss_sum": good[:7] + (None,) + good[8:],
            "null row_rank": good[:8] + (None,) + good[9:],
            "null row_loss": good[:9] + (None,),
            "rows 0": good[:3] + (0,) + good[4:],
            "rows -1": good[:3] + (-1,) + good[4:],
            "rows 2^20 + 1": good[:3] + ((1 << 20) + 1,) + good[4:],
            "classes 0": good[:4] + (0,) + good[5:],
            "classes 65537": (lg, 65537, lb, 4, 65537) + good[5:],
            "ld < classes": (lg, 9) + good[2:],
            "ld 0": (lg, 0) + good[2:],
            "misaligned logits": (P(0x10002),) + good[1:],
            "misaligned labels": good[:2] + (P(0x20004),) + good[3:],
            "misaligned counts": good[:5] + (P(0x30004),) + good[6:],
            "misaligned per_class": good[:6] + (P(0x40004),) + good[7:],
            "misaligned loss_sum": good[:7] + (P(0x50004),) + good[8:],
        }
        for what, a in bad_rows.items():
            assert L.dyt_eval_rows(*a, None) == -1, what
            assert L.dyt_last_error() and b"eval" in L.dyt_last_error(), what
        ts = P(0x80000)
        bad_keep = {
            "null masks": (None, 3, 12, 196, cn),
            "null counts": (ts, 3, 12, 196, None),
            "images 0": (ts, 0, 12, 196, cn),
            "images 2^20 + 1": (ts, (1 << 20) + 1, 12, 196, cn),
            "layers 0": (ts, 3, 0, 196, cn),
            "layers 65": (ts, 3, 65, 196, cn),
            "tokens 0": (ts, 3, 12, 0, cn),
            "tokens 1025": (ts, 3, 12, 1025, cn),
            "misaligned counts": (ts, 3, 12, 196, P(0x30004)),
        }
        for what, a in bad_keep.items():
            assert L.dyt_eval_keep(*a, None) == -1, what
            assert L.dyt_last_error() and b"eval" in L.dyt_last_error(), what


def test_python_wrappers_refuse_cpu_tensors():
    import torch
    import _lib
    import pytest
    from util.metrics import StreamingEval
    st = StreamingEval(10, device="cpu")
    with pytest.raises(_lib.DyTError, match="no CPU path"):
        st.update(torch.zeros(2, 10), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(_lib.DyTError, match="no CPU path"):
        _lib.eval_keep(torch.zeros(2, 12, 196), st.counts, 12, 196)


def _cxx():
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler (CXX, c++, g++, clang++)"
    return cxx


def test_the_sanitized_index_checker_passes(tmp_path):
    """tools/eval_stats_check.cpp: every shape of tests/test_gpu_eval_stats.py played lane by lane -- bounds, alignment, exact cover, layout."""
    exe = str(tmp_path / "eval_stats_check")
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tools", "eval_stats_check.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    for part in ("rows ok", "layout ok", "refusals ok", "all ok"):
        assert part in p.stdout, p.stdout


def test_the_checker_and_the_gpu_test_name_the_same_shapes():
    src = open(os.path.join(ROOT, "tools", "eval_stats_check.cpp")).read()
    cl = [int(v) for v in re.search(r"CLASSES\[\]\s*=\s*\{([^}]*)\}", src).group(1).split(",")]
    rw = [int(v) for v in re.search(r"ROWS\[\]\s*=\s*\{([^}]*)\}", src).group(1).split(",")]
    import test_gpu_eval_stats as G
    assert set(c for c, _ in G.SHAPES) == set(cl) and set(r for _, r in G.SHAPES) == set(rw)
