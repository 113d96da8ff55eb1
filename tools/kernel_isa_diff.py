#!/usr/bin/env python3
"""Are the device functions of two csrc/ trees the same instructions?  For a refactor that only moves kernels between files.

    python tools/kernel_isa_diff.py OLD_CSRC NEW_CSRC [-j JOBS]

For the plain build and the -DDYT_FP16=1 build, every .hip of both directories is compiled with the CXXFLAGS of that directory's
Makefile plus `--cuda-device-only -S` into a temporary directory (no GPU needed).  Each .s is cut into units keyed by mangled
function name -- the body from its label to its .Lfunc_end, which holds a kernel's .amdhsa_kernel descriptor block -- and what
depends only on the position in the file is normalised away (comments, blank lines, the function index in local labels).  The
units of all files of a tree are pooled, so a kernel may change its translation unit.  Whole units are compared for equality;
names that are missing, added or different are listed, and the exit status is 1 if there are any.

Each directory must stand in its tree (ctx.h includes ../../include/dyt_hip.h): for a commit, `git worktree add DIR COMMIT`.
"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

BUILDS = (("plain", []), ("fp16", ["-DDYT_FP16=1"]))

_TYPE = re.compile(r"^\s*\.type\s+([^\s,]+),@function")
_END = re.compile(r"^\.Lfunc_end\d+:")
_KERNEL = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")
_LOCAL = re.compile(r"\.(L[A-Za-z]+)\d+_(\d+)")          # .LBB<function>_<n>, .LJTI<function>_<n>, ...
_FUNC = re.compile(r"\.Lfunc_(begin|end)\d+")


def normalise(lines):
    """Comments and blank lines dropped; .LBB<function>_<n> -> .LBB_<n> and .Lfunc_end<function> -> .Lfunc_end."""
    out = []
    for ln in lines:
        ln = ln.split(";", 1)[0].rstrip()
        if not ln.strip():
            continue
        out.append(_FUNC.sub(r".Lfunc_\1", _LOCAL.sub(r".\1_\2", ln)))
    return "\n".join(out)


def split_units(text):
    """{mangled name: (normalised unit, is_kernel)} of one assembly text."""
    units, funcs, name, body, kernel = {}, set(), None, [], False
    for ln in text.splitlines():
        m = _TYPE.match(ln)
        if m:
            funcs.add(m.group(1))
        if name is None:
            label = ln.split(";", 1)[0].strip()
            if label.endswith(":") and label[:-1] in funcs:
                name, body, kernel = label[:-1], [ln], False
            continue
        body.append(ln)
        m = _KERNEL.match(ln)
        if m and m.group(1) == name:
            kernel = True
        if _END.match(ln):
            units[name] = (normalise(body), kernel)
            name = None
    return units


def compare(old, new):
    """(missing, added, different): sorted name lists of two {name: [unit, ...]} pools."""
    missing = sorted(set(old) - set(new))
    added = sorted(set(new) - set(old))
    different = sorted(n for n in set(old) & set(new) if sorted(old[n]) != sorted(new[n]))
    return missing, added, different


def makefile_flags(csrc):
    """The CXXFLAGS line of csrc/Makefile with ARCH = gfx950 and no CXXFLAGS_EXTRA."""
    for ln in open(os.path.join(csrc, "Makefile")):
        if ln.startswith("CXXFLAGS"):
            return ln.split("=", 1)[1].replace("$(ARCH)", "gfx950").replace("$(CXXFLAGS_EXTRA)", "").split()
    raise SystemExit("%s/Makefile has no CXXFLAGS line" % csrc)


def _compile(job):
    csrc, src, extra, out = job
    cmd = [os.environ.get("HIPCC", "hipcc")] + makefile_flags(csrc) + extra + ["--cuda-device-only", "-S", src, "-o", out]
    r = subprocess.run(cmd, cwd=csrc, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return job, r.returncode, r.stdout


def pool(tmp, tag, csrc, extra, ex):
    """Compile every .hip of csrc; -> ({name: [unit, ...]}, {file: kernel count})."""
    csrc = os.path.abspath(csrc)
    os.makedirs(os.path.join(tmp, tag))
    srcs = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    jobs = [(csrc, f, extra, os.path.join(tmp, tag, f[:-4] + ".s")) for f in srcs]
    units, kernels = {}, {}
    for (_, f, _, out), rc, log in ex.map(_compile, jobs):
        if rc != 0:
            raise SystemExit("hipcc failed on %s/%s:\n%s" % (csrc, f, log))
        found = split_units(open(out).read())
        kernels[f] = sum(1 for _, k in found.values() if k)
        for name, (unit, _) in found.items():
            units.setdefault(name, []).append(unit)
    return units, kernels


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old_csrc")
    ap.add_argument("new_csrc")
    ap.add_argument("-j", "--jobs", type=int, default=min(16, os.cpu_count() or 1), help="compiler jobs at a time (at most 16)")
    a = ap.parse_args(argv)
    bad = 0
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(max(1, min(16, a.jobs))) as ex:
        for build, extra in BUILDS:
            old, old_k = pool(tmp, build + "_old", a.old_csrc, extra, ex)
            new, new_k = pool(tmp, build + "_new", a.new_csrc, extra, ex)
            missing, added, different = compare(old, new)
            print("== build %s: %d functions (%d kernels) old, %d functions (%d kernels) new" %
                  (build, len(old), sum(old_k.values()), len(new), sum(new_k.values())))
            for side, ks in (("old", old_k), ("new", new_k)):
                print("   kernels per file, %s: %s" % (side, " ".join("%s=%d" % (f, n) for f, n in sorted(ks.items()) if n)))
            for what, names in (("missing", missing), ("added", added), ("different", different)):
                print("   %s: %d" % (what, len(names)))
                for n in names:
                    print("      " + n)
            bad += len(missing) + len(added) + len(different)
    print("RESULT: %s" % ("identical" if not bad else "%d functions missing, added or different" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
