"""CPU tests of the GEMM tile routing (dynamic-tuning_amd/csrc/gemm_route.h, the function gemm.hip's dispatch switches over):
tools/gemm_route_check.cpp is compiled with the host C++ compiler and run.  On its own it asserts the hand-derived routes at the routing's
thresholds and, for every M in 1..26000, that body and tail cover every row once; with ``--table`` it routes the GEMMs of
tests/golden/gemm_routes.json -- every GEMM a training step issues at B = 128 and B = 16 in the fp16, fp32 and fp16x3q modes, recorded from
a build whose launches were equal to its parent's (profiles/round8) -- and the answers must be the recorded ones.  Nothing here needs a GPU;
a missing compiler is a failure."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = ["family", "M", "N", "K", "cat", "lead", "wp", "store_epi", "a_map", "a_ld", "a_fold", "m_dev", "a2", "w2", "splitk_fits", "f8_begin"]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler (CXX, c++, g++, clang++)"
    exe = str(tmp_path_factory.mktemp("gemm_route") / "gemm_route_check")
    subprocess.run([cxx, "-std=c++17", "-O2", "-I", os.path.join(ROOT, "dynamic-tuning_amd", "csrc"),
                    os.path.join(ROOT, "tools", "gemm_route_check.cpp"), "-o", exe], check=True)
    return exe


def test_hand_derived_routes_and_row_coverage(checker):
    p = subprocess.run([checker], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    assert "hand-derived routes ok" in p.stdout and "every row covered once" in p.stdout


def test_route_header_includes_nothing():
    src = open(os.path.join(ROOT, "dynamic-tuning_amd", "csrc", "gemm_route.h")).read()
    assert "#include" not in src   # no HIP header: a plain host compiler reads it


def test_recorded_step_routes(checker):
    table = json.load(open(os.path.join(ROOT, "tests", "golden", "gemm_routes.json")))
    assert table["fields"] == ["mode", "B"] + INPUTS + ["kernel", "body"]
    rows = table["routes"]
    assert {(r[0], r[1]) for r in rows} == {(m, b) for m in ("fp16", "fp32", "fp16x3q") for b in (16, 128)}
    feed = "".join(" ".join(str(int(v)) for v in r[2:2 + len(INPUTS)]) + "\n" for r in rows)
    p = subprocess.run([checker, "--table"], input=feed, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    got = [line.split() for line in p.stdout.splitlines()]
    assert len(got) == len(rows)
    for r, g in zip(rows, got):
        assert [g[0], int(g[1])] == r[-2:], (r, g)
