"""CPU test of the image-load work items (dynamic-tuning_amd/csrc/image_items.h, the map image_load.hip's kernel and launcher share):
tools/image_items_check.cpp is compiled with the host C++ compiler and run.  For batch 1 and 2 and every (source kind, destination) it walks
all items and asserts the item count, one writer per destination element, runs that stay inside their row, aligned in-bounds source
offsets, and that every destination element receives its own pixel.  Nothing here needs a GPU; a missing compiler is a failure."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler (CXX, c++, g++, clang++)"
    exe = str(tmp_path_factory.mktemp("image_items") / "image_items_check")
    subprocess.run([cxx, "-std=c++17", "-O2", "-I", os.path.join(ROOT, "dynamic-tuning_amd", "csrc"),
                    os.path.join(ROOT, "tools", "image_items_check.cpp"), "-o", exe], check=True)
    return exe


def test_every_item_of_every_source_and_destination(checker):
    p = subprocess.run([checker], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    assert "every destination element has one writer and its own pixel" in p.stdout


def test_items_header_includes_nothing():
    src = open(os.path.join(ROOT, "dynamic-tuning_amd", "csrc", "image_items.h")).read()
    assert "#include" not in src   # no HIP header: a plain host compiler reads it
