"""CPU tests of the attention routing (dynamic-tuning_amd/csrc/attn_route.h, the two functions attention.hip's launchers switch over):
tools/attn_route_check.cpp is compiled with the host C++ compiler and run.  It asserts the kernel of every configuration a call site
produces -- one hand-derived row per (mode, pass, position) -- and, over the full cross product of the shapes' fields, the routing's
invariants (an error exactly on a violated precondition, lse dropped only where a no-save variant exists, the DYT_OPT_ATTN_V2 bits and the
precision honoured, one-part instances only on planes).  Nothing here needs a GPU; a missing compiler is a failure."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler (CXX, c++, g++, clang++)"
    exe = str(tmp_path_factory.mktemp("attn_route") / "attn_route_check")
    subprocess.run([cxx, "-std=c++17", "-O2", "-I", os.path.join(ROOT, "dynamic-tuning_amd", "csrc"),
                    os.path.join(ROOT, "tools", "attn_route_check.cpp"), "-o", exe], check=True)
    return exe


def test_call_site_routes_and_invariants(checker):
    p = subprocess.run([checker], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    assert "call-site routes ok" in p.stdout and "invariants hold" in p.stdout


def test_route_header_includes_nothing():
    src = open(os.path.join(ROOT, "dynamic-tuning_amd", "csrc", "attn_route.h")).read()
    assert "#include" not in src   # no HIP header: a plain host compiler reads it
