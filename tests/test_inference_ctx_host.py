"""CPU tests of the inference-only context's host side (ABI v3): ``dyt_config.inference_only`` is the header's and the ctypes
struct's LAST field, both agree on the struct's size, the library reports version >= 3, and the Python surface --
``DyTEngine(inference=)``, the three model classes' ``inference_only=`` keyword with its tuning_config / environment fall-backs --
exists.  No compute call: nothing here needs a GPU."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_TYPES = {"int32_t": ctypes.c_int32, "float": ctypes.c_float, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64}


class Cfg(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def _header():
    return open(os.path.join(ROOT, "include", "dyt_hip.h")).read()


def _header_config_fields():
    """[(C type, name)] of ``typedef struct dyt_config { ... } dyt_config;`` with the comments taken out."""
    body = re.search(r"typedef struct dyt_config \{(.*?)\}\s*dyt_config;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"\b(int32_t|int64_t|uint64_t|float)\s+([a-z_0-9]+)\s*;", body)


def test_header_declares_inference_only_last():
    fields = _header_config_fields()
    assert fields[-1] == ("int32_t", "inference_only"), fields[-3:]
    assert fields[-2] == ("int32_t", "adapter_ln")   # appended, nothing moved


def test_ctypes_struct_matches_the_header_field_for_field():
    import _lib
    fields = _header_config_fields()
    assert _lib.Config._fields_[-1] == ("inference_only", ctypes.c_int32)
    assert [n for n, _ in _lib.Config._fields_] == [n for _, n in fields]
    assert [t for _, t in _lib.Config._fields_] == [C_TYPES[t] for t, _ in fields]

    class FromHeader(ctypes.Structure):
        _fields_ = [(n, C_TYPES[t]) for t, n in fields]
    assert ctypes.sizeof(_lib.Config) == ctypes.sizeof(FromHeader) == 4 * len(fields)
    # the shorter positional form older callers use leaves the appended field at 0 = the training layout
    assert _lib.Config(100, 64, 12, 1, 2, 2, 0.1, 0.1, 5.0, 0.5).inference_only == 0


def test_library_is_abi_v3_and_still_exports_exactly_the_header():
    import _lib
    for fp16 in (False, True):
        L = _lib.lib(fp16=fp16)
        assert L.dyt_version() >= 3
        declared = set(re.findall(r"\b(dyt_[a-z0-9_]+)\s*\(", _header()))
        assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
        for name in declared:
            assert hasattr(L, name), name


def test_engine_and_models_accept_the_keyword():
    import runtime
    import models.vision_transformer_IN21K as image
    import models.model_speed_test as twin
    import video_models.video_vision_transformer_IN21K as video
    p = inspect.signature(runtime.DyTEngine.__init__).parameters
    assert "inference" in p and p["inference"].default is False
    for mod in (image, twin, video):
        p = inspect.signature(mod.VisionTransformer.__init__).parameters
        assert "inference_only" in p and p["inference_only"].default is None, mod.__name__


def _build(mod, tuning_extra=None, **kw):
    tuning = Cfg(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option="none", ffn_adapter_init_option="lora",
                 ffn_adapter_scalar="0.1", ffn_num=8, d_model=768, **(tuning_extra or {}))
    return mod.vit_base_patch16_224_in21k(num_classes=10, drop_path_rate=0.0, tuning_config=tuning,
                                          select_config=Cfg(open=True, keep_layers=0), **kw)


def test_keyword_falls_back_to_tuning_config_then_environment_then_off(monkeypatch):
    import models.vision_transformer_IN21K as image
    import models.model_speed_test as twin
    import video_models.video_vision_transformer_IN21K as video
    monkeypatch.delenv("DYT_INFERENCE_ONLY", raising=False)
    for mod in (image, twin, video):
        assert _build(mod).inference_only is False                       # the default stays off everywhere
        assert _build(mod, inference_only=True).inference_only is True
    assert _build(image, tuning_extra=dict(dyt_inference_only=True)).inference_only is True
    assert _build(image, tuning_extra=dict(dyt_inference_only=True), inference_only=False).inference_only is False   # the keyword wins
    monkeypatch.setenv("DYT_INFERENCE_ONLY", "1")
    assert _build(image).inference_only is True
    assert _build(image, tuning_extra=dict(dyt_inference_only=False)).inference_only is False   # tuning_config before the environment
    monkeypatch.setenv("DYT_INFERENCE_ONLY", "0")
    assert _build(image).inference_only is False


def test_inference_only_model_refuses_training_before_any_library_call():
    """train() mode, train_step and as_fused raise DyTError from Python: the model is on the CPU here and no context exists, so reaching
    the library (or the device check in front of it) would fail differently."""
    import pytest
    import torch
    import engine_finetune as E
    import models.vision_transformer_IN21K as image
    from _lib import DyTError
    m = _build(image, inference_only=True)
    m.train()
    x = torch.zeros(1, 3, 224, 224)
    with pytest.raises(DyTError, match="inference_only"):
        m._refuse_training("forward")
    with pytest.raises(DyTError, match="inference_only"):
        E.train_step(m, x, torch.zeros(1, dtype=torch.long), optimizer=None)
    with pytest.raises(DyTError, match="inference_only"):
        E.as_fused(torch.optim.AdamW([p for p in m.parameters()][:1]), m)
    m.eval()
    for p in m.parameters():
        p.requires_grad_(True)
    with pytest.raises(DyTError, match="inference_only"):   # eval mode, but autograd would need a saved pass
        m._refuse_training("forward")
    with torch.no_grad():
        m._refuse_training("forward")                       # the inference call: nothing to refuse
    assert m._engine is None
