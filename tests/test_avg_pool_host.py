"""CPU tests of the mean-pooled / fc_norm head (ABI v5, DYT_CREATE_AVG_POOL / DYT_CREATE_FC_NORM).

  * tests/pool_head_refs.py (the oracle's block stack + pool + fc_norm + head in torch) reproduces the two fixtures recorded from the real
    reference built with ``global_pool='avg'`` and ``global_pool='token', fc_norm=True`` (tests/golden/pool/*.npz, recipe
    tests/golden/make_golden_avg_pool.py) within the bars tests/test_oracle_golden.py holds for the other goldens: logits 2e-5, masks
    bit-exact, loss components 1e-5 relative, gradients 1e-4 relative.
  * the mirror model, built on the CPU, has the reference's key set, reports the recorded missing / unexpected keys for a checkpoint-style
    state dict, still refuses ``''`` and ``('avg', fc_norm=False)``, and synth.is_trainable agrees with the freeze rule.
  * header, ctypes binding and engine signature carry the flags, the parameter ids and dyt_pool_head.
No compute call into the library: nothing here needs a GPU."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import pool_head_refs as PH
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = {"avg": "avg_pool_step.npz", "token": "token_fc_norm_step.npz"}
MODEL_KW = {"avg": dict(global_pool="avg"), "token": dict(global_pool="token", fc_norm=True)}


class Cfg(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def _load(golden_dir, pool):
    return dict(np.load(os.path.join(golden_dir, "pool", FIXTURES[pool])))


def _state(g):
    return synth.make_state_dict(int(g["meta_num_classes"]), int(g["meta_ffn_num"]), seed=int(g["meta_seed"]), kind="test",
                                 gate_bias=float(g["meta_gate_bias"]), head_norm="fc_norm")


def _build(mod=None, num_classes=10, **kw):
    if mod is None:
        import models.vision_transformer_IN21K as mod
    tuning = Cfg(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option="none", ffn_adapter_init_option="lora",
                 ffn_adapter_scalar="0.1", ffn_num=8, d_model=768)
    return mod.vit_base_patch16_224_in21k(num_classes=num_classes, drop_path_rate=0.0, tuning_config=tuning,
                                          select_config=Cfg(open=True, keep_layers=0), **kw)


_steps = {}


def _step(golden_dir, pool):
    """The fixture and pool_head_refs.step_grads on its inputs: computed once per pooling, shared, never modified."""
    if pool not in _steps:
        g = _load(golden_dir, pool)
        B, C, r, seed = int(g["meta_batch"]), int(g["meta_num_classes"]), int(g["meta_ffn_num"]), int(g["meta_seed"])
        sd = _state(g)
        x, y = synth.make_batch(B, C, seed=seed)
        keep = synth.make_dropout_masks(B, r, seed=seed + 3)
        d, grads, outs = PH.step_grads(sd, x, y, torch.from_numpy(g["g1"]), torch.from_numpy(g["g2"]), keep, scale=float(g["meta_scale"]),
                                       mode="masked", pool=pool)
        _steps[pool] = (g, sd, d, grads, outs)
    return _steps[pool]


@pytest.mark.parametrize("pool", ["avg", "token"])
def test_fixture_is_what_the_issue_asks_for(golden_dir, pool):
    g = _load(golden_dir, pool)
    assert (int(g["meta_batch"]), int(g["meta_num_classes"]), int(g["meta_ffn_num"]), float(g["meta_gate_bias"])) == (3, 10, 8, 0.3)
    assert str(g["meta_global_pool"]) == pool
    # the seed of the recipe was chosen for this: no decision of the recorded step is a near-tie
    assert float(g["min_gate_margin"]) >= 1e-4
    z = (torch.from_numpy(g["token_logits"])[..., 0].permute(1, 0, 2) + torch.from_numpy(g["g1"])[0] - torch.from_numpy(g["g2"])[0]) / 5.0
    assert abs(float(z.abs().min()) - float(g["min_gate_margin"])) < 1e-9
    names = [k[len("gradnorm/"):] for k in g if k.startswith("gradnorm/")]
    assert len(names) == 76 and "fc_norm.weight" in names and "fc_norm.bias" in names and not any(n.startswith("norm.") for n in names)
    assert sorted(k for k in g if k.startswith("param_after/")) == ["param_after/" + n for n in ("fc_norm.bias", "fc_norm.weight", "head.bias", "head.weight")]
    assert float(g["gradnorm/fc_norm.weight"]) > 0.1 and float(g["gradnorm/fc_norm.bias"]) > 0.1   # gamma / beta are exercised
    # what the reference reported for a checkpoint-style state dict: everything the freeze rule trains is missing, norm.* is unexpected
    assert [str(k) for k in g["missing_keys"]] == sorted(names) and [str(k) for k in g["unexpected_keys"]] == ["norm.bias", "norm.weight"]


@pytest.mark.parametrize("pool", ["avg", "token"])
def test_refs_reproduce_the_reference_logits_masks_and_losses(golden_dir, pool):
    g, sd, d, grads, (ls, lt, tok) = _step(golden_dir, pool)
    assert np.abs(ls.detach().numpy() - g["logits_student"]).max() < 2e-5
    assert np.abs(lt.detach().numpy() - g["logits_teacher"]).max() < 2e-5
    assert np.abs(tok["token_logits"].detach().numpy() - g["token_logits"]).max() < 2e-5
    assert np.array_equal(tok["token_select"].detach().numpy().astype(np.uint8), g["token_select"])
    for k in ("loss", "base_loss", "token_loss", "teacher_loss", "distillation_loss"):
        assert abs(float(d[k]) - float(g["stat_" + k])) < 1e-5 * max(1.0, abs(float(g["stat_" + k]))), k


@pytest.mark.parametrize("pool", ["avg", "token"])
def test_refs_reproduce_the_reference_gradients_and_adamw(golden_dir, pool):
    from oracle import dyt_oracle as O
    g, sd, d, grads, _ = _step(golden_dir, pool)
    assert len(grads) == 76 and sum(n.startswith("fc_norm.") for n in grads) == 2
    for n, gr in grads.items():
        ref_norm = float(g["gradnorm/" + n])
        assert abs(float(gr.double().norm()) - ref_norm) <= 1e-4 * ref_norm + 1e-8, n
        if "grad/" + n in g:
            assert np.abs(gr.numpy() - g["grad/" + n]).max() <= 1e-4 * np.abs(g["grad/" + n]).max() + 1e-8, n
    for key in (k for k in g if k.startswith("param_after/")):
        n = key.split("/", 1)[1]
        gref = torch.from_numpy(g["grad/" + n])
        p, _, _ = O.adamw_update(sd[n], gref, torch.zeros_like(gref), torch.zeros_like(gref), 1, float(g["meta_lr"]), float(g["meta_wd"]))
        assert np.abs(p.numpy() - g[key]).max() < 1e-7, n


def test_the_two_poolings_differ_and_token_pooling_ignores_the_patch_rows(golden_dir):
    """pool_rows: 'avg' excludes the cls row, 'token' is the cls row -- on a tensor where a mix-up shows."""
    t = torch.arange(2 * 197 * 768, dtype=torch.float64).reshape(2, 197, 768)
    assert torch.equal(PH.pool_rows(t, "token"), t[:, 0])
    assert torch.allclose(PH.pool_rows(t, "avg"), t[:, 1:].sum(1) / 196)
    t2 = t.clone()
    t2[:, 0] = 1e9
    assert torch.equal(PH.pool_rows(t2, "avg"), PH.pool_rows(t, "avg"))
    a, b = _load(golden_dir, "avg"), _load(golden_dir, "token")
    assert np.abs(a["logits_student"] - b["logits_student"]).max() > 1e-2


@pytest.mark.parametrize("pool", ["avg", "token"])
def test_head_ref_in_fp32_equals_torch_modules_under_autograd(pool):
    B, C = 3, 7
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(B, 197, 768, generator=gen)
    ln, fc = torch.nn.LayerNorm(768, eps=1e-6), torch.nn.Linear(768, C)
    with torch.no_grad():
        ln.weight.copy_(1.0 + 0.1 * torch.randn(768, generator=gen))
        ln.bias.copy_(0.1 * torch.randn(768, generator=gen))
    dl = torch.randn(B, C, generator=gen)
    xr = x.clone().requires_grad_(True)
    out = fc(ln(xr[:, 1:].mean(1) if pool == "avg" else xr[:, 0]))
    want = (out.detach(),) + torch.autograd.grad((out * dl).sum(), (xr, ln.weight, ln.bias, fc.weight, fc.bias))
    got = PH.head_ref(x, ln.weight, ln.bias, fc.weight, fc.bias, dl, pool, dtype=torch.float32)
    for name, a, b in zip(("logits", "dx", "d gamma", "d beta", "dW", "db"), got, want):
        assert a.dtype == torch.float32 and a.shape == b.shape, name
        assert float((a - b).abs().max()) <= 2e-5 * float(b.abs().max()) + 1e-7, name
    assert PH.head_ref(x, ln.weight, ln.bias, fc.weight, fc.bias, None, pool)[1] is None


# ---- the mirror model on the CPU ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pool", ["avg", "token"])
def test_mirror_has_the_reference_key_set_and_reports_its_keys(golden_dir, pool):
    g = _load(golden_dir, pool)
    m = _build(**MODEL_KW[pool])
    shapes = synth.param_shapes(10, 8, head_norm="fc_norm")
    sd = m.state_dict()
    assert set(sd) == set(shapes) and len(sd) == 224
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(shapes[k]), k
    assert isinstance(m.norm, torch.nn.Identity) and not any(k.startswith("norm.") for k in sd)
    assert bool((m.fc_norm.weight == 1).all()) and bool((m.fc_norm.bias == 0).all())   # reference init
    assert m.global_pool == pool and m.use_fc_norm is True and m._engine is None
    # a checkpoint-style (norm.*-keyed, no adapters / gates / head / fc_norm) state dict: the reference's own report
    ckpt = {k: v for k, v in synth.make_state_dict(10, 8, seed=1, kind="test").items() if not synth.is_trainable(k)}
    msg = m.load_state_dict(ckpt, strict=False)
    assert sorted(msg.unexpected_keys) == [str(k) for k in g["unexpected_keys"]] == ["norm.bias", "norm.weight"]
    assert sorted(msg.missing_keys) == [str(k) for k in g["missing_keys"]]
    assert sorted(k for k in msg.missing_keys if k.startswith("fc_norm.")) == ["fc_norm.bias", "fc_norm.weight"]
    assert sorted(msg.missing_keys) == sorted(k for k in shapes if synth.is_trainable(k))   # the freeze rule: missing from the checkpoint = trained
    assert sum(1 for k in shapes if synth.is_trainable(k)) == 76
    m.load_state_dict(_state(g), strict=True)


def test_default_model_is_unchanged_and_the_factory_passes_the_arguments_through():
    m = _build()
    assert m.global_pool == "token" and m.use_fc_norm is False and isinstance(m.fc_norm, torch.nn.Identity)
    assert set(m.state_dict()) == set(synth.param_shapes(10, 8)) and "norm.weight" in m.state_dict()
    assert _build(global_pool="token", fc_norm=False).use_fc_norm is False
    assert _build(global_pool="avg", fc_norm=None).use_fc_norm is True and _build(global_pool="avg", fc_norm=True).use_fc_norm is True


def test_refused_configurations_stay_refused():
    import video_models.video_vision_transformer_IN21K as video
    with pytest.raises(NotImplementedError, match="global_pool=''"):
        _build(global_pool="")
    with pytest.raises(NotImplementedError, match="fc_norm=False"):
        _build(global_pool="avg", fc_norm=False)
    for kw in (dict(global_pool="avg"), dict(global_pool="token", fc_norm=True), dict(global_pool="")):
        with pytest.raises(NotImplementedError, match="global_pool"):
            _build(video, **kw)
    assert _build(video).global_pool == "token"


def test_key_map_freeze_rule_and_parameter_ids():
    import _lib
    for k, want in (("fc_norm.weight", _lib.P_FC_NORM_W), ("fc_norm.bias", _lib.P_FC_NORM_B)):
        pid, layer = _lib.key_to_param(k)
        assert pid == want and layer == 0 and _lib.is_trainable_param(pid) and synth.is_trainable(k)
    assert (_lib.P_FC_NORM_W, _lib.P_FC_NORM_B, _lib.P_COUNT_ALL) == (_lib.P_AD_LN_B + 1, _lib.P_AD_LN_B + 2, _lib.P_AD_LN_B + 3)
    assert (_lib.CREATE_WIDE_HEAD, _lib.CREATE_AVG_POOL, _lib.CREATE_FC_NORM) == (1, 2, 4)
    assert not synth.is_trainable("norm.weight") and not _lib.is_trainable_param(_lib.key_to_param("norm.weight")[0])
    for k in synth.param_shapes(10, 8, head_norm="fc_norm"):
        assert _lib.is_trainable_param(_lib.key_to_param(k)[0]) == synth.is_trainable(k), k
    sd = synth.make_state_dict(10, 8, seed=3, kind="test", head_norm="fc_norm")
    assert float((sd["fc_norm.weight"] - 1).abs().max()) > 0.05 and float(sd["fc_norm.bias"].abs().max()) > 0.05   # non-trivial gamma / beta
    assert bool((synth.make_state_dict(10, 8, seed=3, kind="bench", head_norm="fc_norm")["fc_norm.weight"] == 1).all())


def test_header_binding_and_engine_carry_the_feature():
    import _lib
    import runtime
    h = open(os.path.join(ROOT, "include", "dyt_hip.h")).read()
    assert re.search(r"#define\s+DYT_CREATE_AVG_POOL\s+2u\b", h) and re.search(r"#define\s+DYT_CREATE_FC_NORM\s+4u\b", h)
    enum = re.sub(r"/\*.*?\*/", "", re.search(r"enum dyt_param \{(.*?)\};", h, re.S).group(1), flags=re.S)
    ids = [t.split("=")[0].strip() for t in enum.split(",") if t.strip()]
    assert ids[-3:] == ["DYT_P_FC_NORM_W", "DYT_P_FC_NORM_B", "DYT_P_COUNT"] and len(ids) == _lib.P_COUNT_ALL + 1
    assert ids.index("DYT_P_FC_NORM_W") == _lib.P_FC_NORM_W and ids.index("DYT_P_AD_LN_B") == _lib.P_AD_LN_B
    m = re.search(r"\bint\s+dyt_pool_head\s*\((.*?)\)\s*;", h, re.S)
    assert m, "dyt_pool_head is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["x_tokens", "fc_norm_w", "fc_norm_b", "head_w", "head_b", "logits", "dlogits", "dx_tokens",
                                                         "d_fc_norm_w", "d_fc_norm_b", "d_head_w", "d_head_b", "batch", "C", "create_flags", "stream"]
    assert len(_lib.SYMBOLS["dyt_pool_head"][1]) == len(args)
    for fp16 in (False, True):
        L = _lib.lib(fp16=fp16)
        assert L.dyt_version() == 5 and hasattr(L, "dyt_pool_head")
    p = inspect.signature(runtime.DyTEngine.__init__).parameters
    assert p["avg_pool"].default is False and p["fc_norm"].default is False
