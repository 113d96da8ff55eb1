"""CPU tests of the on-device Mixup / CutMix (dyt_set_mix, dyt_mix_images, dyt_mix_targets; util.mixup.DeviceMixup): the header, the ctypes
binding and both libraries agree without a version or flag change; dynamic-tuning_amd/csrc/mix.h -- pairing, scalar formula, source
predicate, box and every argument check -- is walked by tools/mix_check.cpp, built with the host compiler (its header gives the
sanitizer build of the same stand-alone program), against numpy tables from tests/mix_refs.py; the two context-free entries
refuse bad arguments without a device; DeviceMixup draws reproducibly in the documented order.  Nothing here needs a GPU; a missing
compiler is a failure."""
import ctypes
import inspect
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import mix_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dynamic-tuning_amd", "csrc")
ENTRIES = {"dyt_set_mix", "dyt_mix_images", "dyt_mix_targets"}


def _header():
    return open(os.path.join(ROOT, "include", "dyt_hip.h")).read()


def _args(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


# ---- header, binding, libraries --------------------------------------------------------------------------------------------------------
def test_header_declares_the_entries_and_no_new_flag():
    h = _header()
    assert _args("dyt_set_mix") == ["dyt_ctx* ctx", "const void* params_dev", "int frames"]
    assert _args("dyt_mix_images") == ["const void* src", "float* dst", "int count", "int frames", "int src_kind", "const float mean[3]",
                                       "const float std[3]", "const void* params_dev", "void* stream"]
    assert _args("dyt_mix_targets") == ["const int64_t* labels", "float* out", "int rows", "int num_classes", "const void* params_dev", "void* stream"]
    values = [int(v) for v in re.findall(r"#define\s+DYT_F_[A-Z0-9_]+\s+(\d+)\b", h)]
    assert len(values) == len(set(values)) == 11   # mix is context state, not a flag


def test_binding_equals_the_header_and_the_version_stays_5():
    import _lib
    declared = set(re.findall(r"\b(dyt_[a-z0-9_]+)\s*\(", _header()))
    assert ENTRIES <= declared
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    assert ENTRIES <= _lib.OPTIONAL_SYMBOLS   # discovered by symbol
    assert [len(_lib.SYMBOLS[n][1]) for n in ("dyt_set_mix", "dyt_mix_images", "dyt_mix_targets")] == [3, 9, 6]
    for fp16 in (False, True):
        L = _lib.lib(fp16=fp16)
        assert L.dyt_version() == 5
        assert all(hasattr(L, n) for n in ENTRIES)


def test_python_refuses_by_name_when_the_library_lacks_the_entries():
    import _lib
    import runtime
    for fn in (_lib.mix_images, _lib.mix_targets, runtime.DyTEngine.set_mix):
        src = inspect.getsource(fn)
        assert "hasattr(" in src and "rebuild it" in src


def test_mix_h_includes_nothing_and_switches_contraction_off():
    src = open(os.path.join(CSRC, "mix.h")).read()
    assert "#include" not in src   # no HIP header: a plain host compiler reads it
    assert src.count("#pragma clang fp contract(off)") == 2 and "fma(" not in src   # mix_value, mix_smooth: every rounding kept apart
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bmix\.hip\b", mk, re.M)


def test_params_block_layout():
    """MixDraw.words() is csrc/mix.h's MixParams: 16 words, every float the double expression rounded once."""
    from util.mixup import MixDraw
    d = MixDraw.mixup(0.7).with_targets(0.1, 10)
    w = d.words(criterion_smoothing=0.2)
    assert len(w) == 64
    mode, lam_f, oml_f, yl, yh, xl, xh, on, off, sm_on, keep, add = struct.unpack("<iff4iffiff", w[:48])
    f32 = lambda v: float(np.float32(v))   # noqa: E731
    assert (mode, yl, yh, xl, xh, sm_on) == (1, 0, 0, 0, 0, 1)
    assert (lam_f, oml_f) == (f32(0.7), f32(1.0 - 0.7))
    assert (on, off) == (f32(1.0 - 0.1 + 0.1 / 10), f32(0.1 / 10)) and (keep, add) == (f32(1.0 - 0.2), f32(0.2 / 10))
    assert struct.unpack("<4i", w[48:]) == (0, 0, 0, 0)
    c = MixDraw.cutmix((5, 37, 3, 50)).with_targets(0.0, 1000)
    assert c.mode == 2 and c.lam == 1.0 - 32 * 47 / 224.0 ** 2
    assert struct.unpack("<i", c.words()[36:40]) == (0,)
    assert MixDraw.mixup(1.0).mode == 0 and MixDraw.identity().lam == 1.0
    for bad in (lambda: MixDraw(1, 1.5), lambda: MixDraw(1, -0.1), lambda: MixDraw(1, float("nan")), lambda: MixDraw(3, 0.5),
                lambda: MixDraw(2, 0.5, (0, 225, 0, 10)), lambda: MixDraw(2, 0.5, (-1, 5, 0, 10)), lambda: MixDraw(2, 0.5, (10, 9, 0, 10)),
                lambda: MixDraw.mixup(0.5).words(), lambda: MixDraw.mixup(0.5).with_targets(0.1, 0).words()):
        with pytest.raises(ValueError):
            bad()


# ---- the context-free entries refuse without a device ----------------------------------------------------------------------------------------
def test_refusals_of_the_context_free_entries_need_no_device():
    import _lib
    L = _lib.lib()
    m, s = _lib.float3((0.5, 0.5, 0.5)), _lib.float3((0.5, 0.5, 0.5))
    src, dst, par = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000), ctypes.c_void_p(0x30000)
    bad_images = {
        "odd count": (src, dst, 3, 1, 0, m, s, par),
        "odd clips": (src, dst, 6, 2, 1, m, s, par),
        "count not a multiple of frames": (src, dst, 5, 2, 1, m, s, par),
        "count 0": (src, dst, 0, 1, 0, m, s, par),
        "frames 0": (src, dst, 2, 0, 0, m, s, par),
        "null src": (None, dst, 2, 1, 0, m, s, par),
        "null dst": (src, None, 2, 1, 0, m, s, par),
        "null params": (src, dst, 2, 1, 0, m, s, None),
        "misaligned params": (src, dst, 2, 1, 0, m, s, ctypes.c_void_p(0x30004)),
        "misaligned byte pointer": (ctypes.c_void_p(0x10004), dst, 2, 1, 1, m, s, par),
        "misaligned dst": (src, ctypes.c_void_p(0x20008), 2, 1, 0, m, s, par),
        "src_kind 3": (src, dst, 2, 1, 3, m, s, par),
        "src_kind -1": (src, dst, 2, 1, -1, m, s, par),
        "bytes without statistics": (src, dst, 2, 1, 1, None, None, par),
        "std 0": (src, dst, 2, 1, 2, m, _lib.float3((0.5, 0.0, 0.5)), par),
    }
    for what, a in bad_images.items():
        assert L.dyt_mix_images(*a, None) == -1, what
        assert L.dyt_last_error(), what
    lab, out = ctypes.c_void_p(0x40000), ctypes.c_void_p(0x50000)
    bad_targets = {
        "odd rows": (lab, out, 3, 10, par),
        "rows 0": (lab, out, 0, 10, par),
        "num_classes 0": (lab, out, 2, 0, par),
        "num_classes -1": (lab, out, 2, -1, par),
        "num_classes 65537": (lab, out, 2, 65537, par),
        "null labels": (None, out, 2, 10, par),
        "null out": (lab, None, 2, 10, par),
        "misaligned out": (lab, ctypes.c_void_p(0x50004), 2, 10, par),
        "null params": (lab, out, 2, 10, None),
    }
    for what, a in bad_targets.items():
        assert L.dyt_mix_targets(*a, None) == -1, what
        assert L.dyt_last_error(), what
    assert L.dyt_set_mix(None, par, 1) == -1


# ---- csrc/mix.h through the host compiler ------------------------------------------------------------------------------------------------
def _cxx():
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler (CXX, c++, g++, clang++)"
    return cxx


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mix") / "mix_check")
    subprocess.run([_cxx(), "-std=c++17", "-O2", "-ffp-contract=off", "-I", CSRC, os.path.join(ROOT, "tools", "mix_check.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("mix_tables") / "tables.bin")
    R.write_tables(path)
    return path


def _run(exe, path):
    return subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_mix_h_against_the_numpy_tables(checker, tables):
    p = _run(checker, tables)
    assert p.returncode == 0, p.stdout
    for part in ("partner ok", "value ok", "predicate ok", "box ok", "refusals ok"):
        assert part in p.stdout, p.stdout


def test_a_contracted_value_table_is_noticed(checker, tmp_path):
    """The checker compares bits: the table of the fused multiply-add form is refused."""
    v = R.value_table()
    a, b, lam_f, oml_f = (v[:, k].astype(np.float64) for k in range(4))
    fused = (lam_f * a + (v[:, 3] * v[:, 1]).astype(np.float32).astype(np.float64)).astype(np.float32)   # fma(lam, a, r(oml b))
    assert not np.array_equal(fused, v[:, 4])
    wrong = v.copy()
    wrong[:, 4] = fused
    path = str(tmp_path / "wrong.bin")
    R.write_tables(path, value=wrong)
    p = _run(checker, path)
    assert p.returncode != 0 and "value ok" not in p.stdout


def test_the_references_agree_with_synth_mixup_batch():
    """mix_refs restates synth.mixup_batch (images and targets) bit for bit, and the numpy value table is torch's arithmetic."""
    import synth
    from util.mixup import MixDraw
    x, y = synth.make_batch(4, 10, seed=3)
    for lam in (0.7, 0.31415926):
        d = MixDraw.mixup(lam).with_targets(0.1, 10)
        xm, t = synth.mixup_batch(x, y, 10, lam=lam, smoothing=0.1)
        assert torch.equal(R.mix_images(x, d), xm) and torch.equal(R.mix_targets(y, 10, d, 0.1), t)
    v = torch.from_numpy(R.value_table().astype(np.float32))
    for lam_f, oml_f in ((0.7, 1.0 - 0.7), (0.25, 0.75)):
        rows = v[(v[:, 2] == np.float32(lam_f))]
        if len(rows):
            assert torch.equal(lam_f * rows[:, 0] + oml_f * rows[:, 1], rows[:, 4])
    # video pairing: frame f of clip b with frame f of clip nb-1-b
    ids = torch.arange(8.0).view(8, 1, 1, 1).expand(8, 3, 224, 224).contiguous()
    assert R.partner_images(ids, 2)[:, 0, 0, 0].tolist() == [6, 7, 4, 5, 2, 3, 0, 1]
    assert R.partner_images(ids, 1)[:, 0, 0, 0].tolist() == [7, 6, 5, 4, 3, 2, 1, 0]
    # cutmix: the box, and only the box, comes from the partner; identity copies
    d = MixDraw.cutmix(R.BOXES["crossing"])
    out = R.mix_images(x, d)
    yl, yh, xl, xh = d.box
    inside = torch.zeros(224, 224, dtype=torch.bool)
    inside[yl:yh, xl:xh] = True
    assert torch.equal(out[:, :, inside], x.flip(0)[:, :, inside]) and torch.equal(out[:, :, ~inside], x[:, :, ~inside])
    assert torch.equal(R.mix_images(x, MixDraw.identity()), x)


# ---- DeviceMixup ------------------------------------------------------------------------------------------------------------------------------
def test_device_mixup_signature_and_unsupported_options():
    from util.mixup import DeviceMixup
    p = inspect.signature(DeviceMixup.__init__).parameters
    assert list(p)[1:] == ["mixup_alpha", "cutmix_alpha", "cutmix_minmax", "prob", "switch_prob", "mode", "correct_lam", "label_smoothing",
                           "num_classes", "generator"]
    assert [p[k].default for k in list(p)[1:10]] == [1., 0., None, 1.0, 0.5, 'batch', True, 0.1, 1000]
    for kw in (dict(mode="elem"), dict(mode="pair"), dict(cutmix_minmax=(0.2, 0.8)), dict(correct_lam=False)):
        with pytest.raises(NotImplementedError):
            DeviceMixup(**kw)
    with pytest.raises(ValueError):
        DeviceMixup(mixup_alpha=0., cutmix_alpha=0.)
    import engine_finetune
    assert "mix" in inspect.signature(engine_finetune.train_step).parameters


def test_the_same_seed_gives_the_same_draws():
    from util.mixup import DeviceMixup
    kw = dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.9, switch_prob=0.5, label_smoothing=0.1, num_classes=10)
    a, b = DeviceMixup(generator=123, **kw), DeviceMixup(generator=np.random.default_rng(123), **kw)
    da, db = [a.draw() for _ in range(50)], [b.draw() for _ in range(50)]
    assert [d.words() for d in da] == [d.words() for d in db]
    assert {d.mode for d in da} == {0, 1, 2}   # prob < 1: identity, mixup and cutmix all occur in 50 draws
    other = [DeviceMixup(generator=124, **kw).draw().words() for _ in range(50)]
    assert other != [d.words() for d in da]
    for d in da:
        d.check()
        assert (d.smoothing, d.num_classes) == (0.1, 10)
        if d.mode == 2:
            assert d.lam == 1.0 - (d.box[1] - d.box[0]) * (d.box[3] - d.box[2]) / 224.0 ** 2


def test_the_documented_draw_order():
    """random() < prob; [random() < switch_prob]; beta(alpha, alpha); [integers(0, 224) for cy, then cx]: replayed with a second
    generator of the same seed."""
    from util.mixup import DeviceMixup
    for kw in (dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.7), dict(mixup_alpha=0.4, cutmix_alpha=0.), dict(mixup_alpha=0., cutmix_alpha=1.0, prob=0.5)):
        mix, g = DeviceMixup(generator=77, label_smoothing=0.0, num_classes=5, **kw), np.random.default_rng(77)
        ma, ca, prob = kw["mixup_alpha"], kw["cutmix_alpha"], kw.get("prob", 1.0)
        for _ in range(40):
            d = mix.draw()
            if not g.random() < prob:
                assert d.mode == 0 and d.lam == 1.0
                continue
            cut = bool(g.random() < 0.5) if (ma > 0 and ca > 0) else not ma > 0
            alpha = ca if cut else ma
            lam = float(g.beta(alpha, alpha))
            if cut:
                cy = int(g.integers(0, 224))
                cx = int(g.integers(0, 224))
                box, want = R.rand_bbox_numpy(lam, cy, cx)
                assert d.mode == 2 and d.box == box and d.lam == float(want)
            else:
                assert d.mode == (0 if lam == 1.0 else 1) and d.lam == lam


def test_injected_draws_come_first_and_get_the_targets_filled():
    from util.mixup import DeviceMixup, MixDraw
    mix = DeviceMixup(label_smoothing=0.2, num_classes=7, generator=1).inject([MixDraw.mixup(0.7), MixDraw.cutmix((5, 37, 3, 50)), MixDraw.identity()])
    got = [mix.draw() for _ in range(3)]
    assert [d.mode for d in got] == [1, 2, 0] and got[0].lam == 0.7 and got[1].box == (5, 37, 3, 50)
    assert all((d.smoothing, d.num_classes) == (0.2, 7) for d in got)
    want = DeviceMixup(label_smoothing=0.2, num_classes=7, generator=1).draw()
    assert mix.draw().words() == want.words()   # then the generator, from its start
