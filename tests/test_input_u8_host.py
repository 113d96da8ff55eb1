"""CPU tests of the byte-image input (DYT_F_IMAGES_U8 / DYT_F_IMAGES_NHWC, dyt_set_input_norm, dyt_normalize_u8): the header, the ctypes
binding and the library agree; dynamic-tuning_amd/csrc/input_norm.h -- the scalar formula the kernels evaluate and every argument
check -- is walked by tools/input_norm_check.cpp, built with the host compiler, against tests/golden/input_u8/input_norm_table.npz; the three
model classes take ``input_norm`` and leave a uint8 input of a model WITHOUT it exactly as it was (``.float()``).  Nothing here needs
a GPU; a missing compiler is a failure."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import input_u8_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dynamic-tuning_amd", "csrc")


class Cfg(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def _header():
    return open(os.path.join(ROOT, "include", "dyt_hip.h")).read()


def _build(mod, tuning_extra=None, **kw):
    tuning = Cfg(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option="none", ffn_adapter_init_option="lora",
                 ffn_adapter_scalar="0.1", ffn_num=8, d_model=768, **(tuning_extra or {}))
    return mod.vit_base_patch16_224_in21k(num_classes=10, drop_path_rate=0.0, tuning_config=tuning,
                                          select_config=Cfg(open=True, keep_layers=0), **kw)


def _args(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_flags_and_the_entries():
    h = _header()
    assert re.search(r"#define\s+DYT_F_IMAGES_U8\s+512\b", h) and re.search(r"#define\s+DYT_F_IMAGES_NHWC\s+1024\b", h)
    assert _args("dyt_set_input_norm") == ["dyt_ctx* ctx", "const float mean[3]", "const float std[3]"]
    assert _args("dyt_normalize_u8") == ["const uint8_t* src", "float* dst", "int batch", "int nhwc", "const float mean[3]",
                                         "const float std[3]", "void* stream"]
    # no existing flag value is reused
    values = [int(v) for v in re.findall(r"#define\s+DYT_F_[A-Z0-9_]+\s+(\d+)\b", h)]
    assert len(values) == len(set(values)) == 11


def test_binding_equals_the_header_and_the_version_stays_5():
    import _lib
    declared = set(re.findall(r"\b(dyt_[a-z0-9_]+)\s*\(", _header()))
    assert {"dyt_set_input_norm", "dyt_normalize_u8"} <= declared
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    assert (_lib.F_IMAGES_U8, _lib.F_IMAGES_NHWC) == (512, 1024)
    assert {"dyt_set_input_norm", "dyt_normalize_u8"} <= _lib.OPTIONAL_SYMBOLS   # discovered by symbol, like dyt_adamw_segments
    res, argtypes = _lib.SYMBOLS["dyt_set_input_norm"]
    assert res is ctypes.c_int and len(argtypes) == 3
    res, argtypes = _lib.SYMBOLS["dyt_normalize_u8"]
    assert res is ctypes.c_int and len(argtypes) == 7 and argtypes[2] is ctypes.c_int and argtypes[3] is ctypes.c_int
    for fp16 in (False, True):
        L = _lib.lib(fp16=fp16)
        assert L.dyt_version() == 5
        assert hasattr(L, "dyt_set_input_norm") and hasattr(L, "dyt_normalize_u8")


def test_refusals_of_the_context_free_entry_need_no_device():
    """dyt_normalize_u8 checks its arguments before it launches: every refusal returns DYT_ERR_ARG (-1) with a text, on a machine
    without a GPU too."""
    import _lib
    L = _lib.lib()
    ok_m, ok_s = _lib.float3((0.5, 0.5, 0.5)), _lib.float3((0.5, 0.5, 0.5))
    src, dst = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000)
    bad = {
        "misaligned src": (ctypes.c_void_p(0x10004), dst, 1, 0, ok_m, ok_s),
        "misaligned dst": (src, ctypes.c_void_p(0x20008), 1, 0, ok_m, ok_s),
        "null src": (None, dst, 1, 0, ok_m, ok_s),
        "batch 0": (src, dst, 0, 0, ok_m, ok_s),
        "std 0": (src, dst, 1, 1, ok_m, _lib.float3((0.5, 0.0, 0.5))),
        "std < 0": (src, dst, 1, 1, ok_m, _lib.float3((0.5, 0.5, -1.0))),
        "std inf": (src, dst, 1, 0, ok_m, _lib.float3((float("inf"), 0.5, 0.5))),
        "std nan": (src, dst, 1, 0, ok_m, _lib.float3((0.5, float("nan"), 0.5))),
        "mean nan": (src, dst, 1, 0, _lib.float3((float("nan"), 0.5, 0.5)), ok_s),
        "mean inf": (src, dst, 1, 0, _lib.float3((0.5, 0.5, float("-inf"))), ok_s),
    }
    for what, a in bad.items():
        assert L.dyt_normalize_u8(*a, None) == -1, what
        assert L.dyt_last_error(), what
    assert L.dyt_set_input_norm(None, ok_m, ok_s) == -1


# ---- csrc/input_norm.h through the host compiler ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_table():
    z = np.load(os.path.join(ROOT, "tests", "golden", "input_u8", "input_norm_table.npz"))
    for name, (mean, std) in R.STATS.items():
        assert np.array_equal(z[name + "_mean"], np.asarray(mean, dtype=np.float32))
        assert np.array_equal(z[name + "_std"], np.asarray(std, dtype=np.float32))
        assert z[name].dtype == np.float32 and z[name].shape == (3, 256)
    return z


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler (CXX, c++, g++, clang++)"
    exe = str(tmp_path_factory.mktemp("input_norm") / "input_norm_check")
    subprocess.run([cxx, "-std=c++17", "-O2", "-I", CSRC, os.path.join(ROOT, "tools", "input_norm_check.cpp"), "-o", exe], check=True)
    return exe


def test_scalar_formula_and_refusals_in_the_host_build(checker, golden_table, tmp_path):
    path = str(tmp_path / "table.bin")
    np.stack([golden_table["imagenet"], golden_table["inception"]]).astype("<f4").tofile(path)
    p = subprocess.run([checker, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    assert "formula ok" in p.stdout and "refusals ok" in p.stdout


def test_a_wrong_table_is_noticed(checker, golden_table, tmp_path):
    """The checker compares bits: the table of the reciprocal-multiply shortcut is refused."""
    u = np.arange(256, dtype=np.float32)[None, :]
    wrong = []
    for name in ("imagenet", "inception"):
        m, s = (np.asarray(v, dtype=np.float32)[:, None] for v in R.STATS[name])
        wrong.append((u * (np.float32(1) / np.float32(255)) - m) * (np.float32(1) / s))
    assert not np.array_equal(wrong[0], golden_table["imagenet"])
    path = str(tmp_path / "wrong.bin")
    np.stack(wrong).astype("<f4").tofile(path)
    p = subprocess.run([checker, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode != 0 and "formula ok" not in p.stdout


def test_header_of_the_formula_includes_nothing():
    src = open(os.path.join(CSRC, "input_norm.h")).read()
    assert "#include" not in src   # no HIP header: a plain host compiler reads it
    assert "255.0f" in src and "1.0f / 255" not in src


def test_torch_numpy_and_the_golden_table_agree_bit_for_bit(golden_table):
    u = R.byte_images(2, seed=5)
    for name in R.STATS:
        want = R.normalize_cpu(u, name)
        assert want.dtype == torch.float32 and np.array_equal(want.numpy(), R.normalize_numpy(u, name))
        t = torch.from_numpy(golden_table[name])
        for c in range(3):
            assert torch.equal(want[:, c], t[c][u[:, c].long()])
    nhwc = R.to_nhwc(u)
    assert tuple(nhwc.shape) == (2, 224, 224, 3) and torch.equal(nhwc.permute(0, 3, 1, 2), u)


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------
def test_models_and_engine_accept_input_norm():
    import _lib
    import runtime
    import models.vision_transformer_IN21K as image
    import models.model_speed_test as twin
    import video_models.video_vision_transformer_IN21K as video
    for mod in (image, twin, video):
        p = inspect.signature(mod.VisionTransformer.__init__).parameters
        if mod is image:
            assert "input_norm" in p and p["input_norm"].default is None
        assert _build(mod).input_norm is None                             # off unless asked for
        assert _build(mod, input_norm="imagenet").input_norm == R.STATS["imagenet"]
        assert _build(mod, input_norm="inception").input_norm == R.STATS["inception"]
        assert _build(mod, input_norm=((0.1, 0.2, 0.3), (1, 2, 3))).input_norm == ((0.1, 0.2, 0.3), (1.0, 2.0, 3.0))
    assert _build(image, tuning_extra=dict(dyt_input_norm="inception")).input_norm == R.STATS["inception"]
    assert _build(image, tuning_extra=dict(dyt_input_norm="inception"), input_norm="imagenet").input_norm == R.STATS["imagenet"]   # the keyword wins
    for bad in ("caffe", ((0.5, 0.5), (0.5, 0.5)), ((0.5, 0.5, 0.5), (0.5, 0.0, 0.5)), ((float("nan"), 0.5, 0.5), (0.5, 0.5, 0.5))):
        with pytest.raises(ValueError):
            _build(image, input_norm=bad)
    assert _lib.INPUT_NORMS == R.STATS
    assert hasattr(runtime.DyTEngine, "set_input_norm")
    p = inspect.signature(runtime.DyTEngine.step_graph).parameters
    assert "images" in p


def test_uint8_input_without_input_norm_is_still_converted_with_float():
    """Up to the point where the device is required: what the entries hand to the engine."""
    import models.vision_transformer_IN21K as image
    import video_models.video_vision_transformer_IN21K as video
    from _lib import DyTError
    u = R.byte_images(2, seed=3)
    plain, byte = _build(image), _build(image, input_norm="imagenet")
    x = plain.prepare_input(u)
    assert x.dtype == torch.float32 and torch.equal(x, u.float()) and not plain.takes_bytes(u)
    for t in (u, R.to_nhwc(u)):
        y = byte.prepare_input(t)
        assert y.dtype == torch.uint8 and y.is_contiguous() and torch.equal(y, t) and byte.takes_bytes(t)
    f = torch.randn(2, 3, 224, 224)
    assert torch.equal(byte.prepare_input(f), f) and not byte.takes_bytes(f)     # float inputs are untouched by the setting
    with pytest.raises(DyTError):                                                # no CPU path behind it
        plain(u)
    # video: clips are folded to frames on the bytes, both layouts; the float fold is the one it was
    clips = u.reshape(1, 2, 3, 224, 224).permute(0, 2, 1, 3, 4).contiguous()     # [b,3,t,224,224]
    vb, vp = _build(video, input_norm="inception"), _build(video)
    frames = vb.prepare_input(clips)
    assert frames.dtype == torch.uint8 and torch.equal(frames, u) and vb._frames == 2
    last = R.to_nhwc(u).reshape(1, 2, 224, 224, 3)                                # [b,t,224,224,3]
    frames = vb.prepare_input(last)
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == (2, 224, 224, 3) and torch.equal(frames, R.to_nhwc(u))
    assert torch.equal(vp.prepare_input(clips), u.float())


def test_layout_is_decided_by_the_shape():
    from _lib import DyTError, byte_image_layout
    assert byte_image_layout(torch.zeros(2, 3, 224, 224)) is None
    assert byte_image_layout(torch.zeros(2, 3, 224, 224, dtype=torch.uint8)) == "nchw"
    assert byte_image_layout(torch.zeros(2, 224, 224, 3, dtype=torch.uint8)) == "nhwc"
    with pytest.raises(DyTError):
        byte_image_layout(torch.zeros(2, 3, 32, 32, dtype=torch.uint8))
