"""CPU tests of the wide head's host side (ABI v4): the header declares dyt_ctx_create_ex / DYT_CREATE_WIDE_HEAD / dyt_head_wide, both
libraries export exactly the header, dyt_config is field for field what it was, and the Python surface -- ``DyTEngine(wide_head=)``, the
image models' ``wide_head=`` keyword with its tuning_config / environment / num_classes fall-backs -- exists.  A 21 843-class model
(the ImageNet-21K classifier) builds on the CPU.  No compute call: nothing here needs a GPU."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import wide_head_refs as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG_FIELDS = [("int32_t", "num_classes"), ("int32_t", "ffn_num"), ("int32_t", "depth"), ("int32_t", "precision"), ("int32_t", "max_batch"),
                 ("int32_t", "slots"), ("float", "adapter_scale"), ("float", "adapter_dropout"), ("float", "tau"), ("float", "threshold"),
                 ("int32_t", "frames"), ("int32_t", "adapter_ln"), ("int32_t", "inference_only")]
C_TYPES = {"int32_t": ctypes.c_int32, "float": ctypes.c_float}


class Cfg(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def _header():
    return open(os.path.join(ROOT, "include", "dyt_hip.h")).read()


def test_header_declares_the_wide_head_entries():
    h = _header()
    assert re.search(r"#define\s+DYT_CREATE_WIDE_HEAD\s+1u\b", h)
    assert re.search(r"\bint\s+dyt_ctx_create_ex\s*\(\s*const\s+dyt_config\s*\*\s*cfg\s*,\s*uint32_t\s+create_flags\s*,\s*dyt_ctx\s*\*\*\s*out\s*\)\s*;", h)
    m = re.search(r"\bint\s+dyt_head_wide\s*\((.*?)\)\s*;", h, re.S)
    assert m, "dyt_head_wide is not declared"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["cls_x", "norm_w", "norm_b", "head_w", "head_b", "logits", "dlogits", "dx", "d_head_w",
                                                         "d_head_b", "batch", "C", "stream"], args


def test_config_struct_is_field_for_field_what_it_was():
    import _lib
    body = re.search(r"typedef struct dyt_config \{(.*?)\}\s*dyt_config;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(int32_t|int64_t|uint64_t|float)\s+([a-z_0-9]+)\s*;", body)
    assert fields == CONFIG_FIELDS
    assert list(_lib.Config._fields_) == [(n, C_TYPES[t]) for t, n in CONFIG_FIELDS]
    assert ctypes.sizeof(_lib.Config) == 4 * len(CONFIG_FIELDS)
    assert _lib.CREATE_WIDE_HEAD == 1


def test_libraries_are_abi_v4_and_export_exactly_the_header():
    import _lib
    declared = set(re.findall(r"\b(dyt_[a-z0-9_]+)\s*\(", _header()))
    assert {"dyt_ctx_create_ex", "dyt_head_wide"} <= declared
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    for fp16 in (False, True):
        L = _lib.lib(fp16=fp16)
        assert L.dyt_version() >= 4
        for name in declared:
            assert hasattr(L, name), (fp16, name)


def test_engine_and_image_models_take_the_keyword():
    import runtime
    import models.vision_transformer_IN21K as image
    import models.model_speed_test as twin
    import video_models.video_vision_transformer_IN21K as video
    p = inspect.signature(runtime.DyTEngine.__init__).parameters
    assert "wide_head" in p and p["wide_head"].default is False
    for mod in (image, twin):
        p = inspect.signature(mod.VisionTransformer.__init__).parameters
        assert "wide_head" in p and p["wide_head"].default is None, mod.__name__
    assert "wide_head" not in inspect.signature(video.VisionTransformer.__init__).parameters
    with pytest.raises(TypeError, match="wide_head"):
        _build(video, wide_head=True)
    assert _build(video, num_classes=2000).wide_head is False   # (> 1024 classes: the library's refusal, as before)


def _build(mod, tuning_extra=None, num_classes=1000, **kw):
    tuning = Cfg(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option="none", ffn_adapter_init_option="lora",
                 ffn_adapter_scalar="0.1", ffn_num=8, d_model=768, **(tuning_extra or {}))
    return mod.vit_base_patch16_224_in21k(num_classes=num_classes, drop_path_rate=0.0, tuning_config=tuning,
                                          select_config=Cfg(open=True, keep_layers=0), **kw)


def test_a_21843_class_model_builds_and_resolves_to_the_wide_head(monkeypatch):
    import models.vision_transformer_IN21K as image
    import models.model_speed_test as twin
    monkeypatch.delenv("DYT_WIDE_HEAD", raising=False)
    for mod in (image, twin):
        m = _build(mod, num_classes=21843)
        sd = m.state_dict()
        assert len(sd) == 224
        assert tuple(sd["head.weight"].shape) == (21843, 768) and tuple(sd["head.bias"].shape) == (21843,)
        assert m.wide_head is True and m.num_classes == 21843
        assert m._engine is None   # no library context on the CPU


def test_keyword_then_tuning_config_then_environment_then_class_count(monkeypatch):
    import models.vision_transformer_IN21K as image
    monkeypatch.delenv("DYT_WIDE_HEAD", raising=False)
    assert _build(image, num_classes=1000).wide_head is False
    assert _build(image, num_classes=1024).wide_head is False
    assert _build(image, num_classes=1025).wide_head is True
    assert _build(image, num_classes=1000, wide_head=True).wide_head is True
    assert _build(image, num_classes=2000, wide_head=False).wide_head is False                                       # the keyword wins
    assert _build(image, tuning_extra=dict(dyt_wide_head=True)).wide_head is True
    assert _build(image, tuning_extra=dict(dyt_wide_head=True), wide_head=False).wide_head is False
    monkeypatch.setenv("DYT_WIDE_HEAD", "1")
    assert _build(image).wide_head is True
    assert _build(image, tuning_extra=dict(dyt_wide_head=False)).wide_head is False                                  # tuning_config before the environment
    assert _build(image, wide_head=False).wide_head is False
    monkeypatch.setenv("DYT_WIDE_HEAD", "0")
    assert _build(image).wide_head is False
    assert _build(image, num_classes=2000).wide_head is False                                                        # the environment before the class count
    assert _build(image, num_classes=2000, tuning_extra=dict(dyt_wide_head=True)).wide_head is True


@pytest.mark.parametrize("B,C", [(1, 1), (3, 65), (5, 1025)])
def test_head_full_ref_in_fp32_equals_torch_modules_under_autograd(B, C):
    g = torch.Generator().manual_seed(1000 * B + C)
    x = torch.randn(B, 768, generator=g)
    ln = torch.nn.LayerNorm(768, eps=1e-6)
    fc = torch.nn.Linear(768, C)
    with torch.no_grad():
        ln.weight.copy_(1.0 + 0.1 * torch.randn(768, generator=g))
        ln.bias.copy_(0.1 * torch.randn(768, generator=g))
        fc.weight.copy_(0.02 * torch.randn(C, 768, generator=g))
        fc.bias.copy_(0.02 * torch.randn(C, generator=g))
    dl = torch.randn(B, C, generator=g)
    xr = x.clone().requires_grad_(True)
    out = fc(ln(xr))
    dx, dW, db = torch.autograd.grad((out * dl).sum(), (xr, fc.weight, fc.bias))
    got = WR.head_full_ref(x, ln.weight, ln.bias, fc.weight, fc.bias, dl, dtype=torch.float32)
    for name, a, b in zip(("logits", "dx", "dW", "db"), got, (out.detach(), dx, dW, db)):
        assert a.dtype == torch.float32 and a.shape == b.shape, name
        tol = 2e-5 * float(b.abs().max()) + 1e-7   # two fp32 evaluations of one formula (fused kernel vs elementwise ops): a few ulp of the largest entry
        assert float((a - b).abs().max()) <= tol, (name, float((a - b).abs().max()), tol)
    r64 = WR.head_full_ref(x, ln.weight, ln.bias, fc.weight, fc.bias, dl)
    assert all(t.dtype == torch.float64 for t in r64)
    lo = WR.head_full_ref(x, ln.weight, ln.bias, fc.weight, fc.bias, None)
    assert lo[1] is None and lo[2] is None and lo[3] is None and torch.equal(lo[0], r64[0])
