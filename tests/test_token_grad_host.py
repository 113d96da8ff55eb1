"""CPU tests of the token-level training route (dyt_forward_taps / dyt_backward_tokens; forward_features with out_indices).

  * _lib.check_out_indices: every refusal, and what it accepts.
  * tests/token_grad_refs.py::tap_loss_grads, the reference of tests/test_gpu_token_grad.py, is pinned three ways at depth 3, B = 2:
      - fp32 against fp64 (the decisions of the two are asserted equal first): per-tensor relative L2 under 2e-3, the bar the project holds
        an fp32 implementation to against this oracle (tests/gpu_diag.py);
      - against a central finite difference in fp64, step 1e-5 along a unit-norm direction, to 1e-6 relative: truncation is
        h^2 |L'''| / 6 ~ 1e-10 of L', round-off eps |L| / h ~ 2e-16 * 1 / 1e-5 = 2e-11 against derivatives of 1e-4 ... 1e-2.  Two adapter
        tensors and one gate tensor.  The gate's decision enters the forward value as a hard 0 / 1 (straight-through,
        models/dynamic_adapter.py:47-51), so a finite difference cannot see the surrogate gradient that autograd sends through every
        gate BEHIND the perturbed tensor.  Hence: the last block's up_proj (no gate behind it) with the whole student functional; block
        0's down_proj with the complete_model pass (no mask in the forward value) and every term but token_select; the LAST block's gate
        weight with the token_logits term alone, the one output that depends on it differentiably (an earlier block's gate also
        reaches the later blocks' token_logits through its own hard decision);
      - classification identity: with R_taps = 0 and R_tokens = d CE(head(tokens[:, 0])) / d tokens, the functional's gradients are the
        gradients of CE(oracle.forward(...)) -- the student cross-entropy part of oracle.step_loss -- over the same tensors.
  * header, ctypes table and engine / model signatures carry the new entries.
Nothing here needs a GPU."""
import inspect
import os
import re

import pytest
import torch
import torch.nn.functional as F

import synth
import token_grad_refs as TG
from oracle import dyt_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTH, B, C, RANK = 3, 2, 10, 8


def test_out_indices_validation():
    from _lib import check_out_indices as ck
    assert ck((3, 5, 7, 11), 12) == (3, 5, 7, 11)
    assert ck([11, 3], 12) == (11, 3)            # the order given is kept
    assert ck((-1, 0), 12) == (11, 0)            # negative values count from the end
    assert ck((-12,), 12) == (0,)
    assert ck(range(3), 3) == (0, 1, 2)
    for bad, word in (((12,), "outside"), ((-13,), "outside"), ((3, 3), "distinct"), ((11, -1), "distinct"), ((1.0,), "not an int"),
                      ((True,), "not an int"), (("3",), "not an int"), ((None,), "not an int"), (5, "sequence"), ("35", "sequence"), ((), "at least one")):
        with pytest.raises(ValueError, match=word):
            ck(bad, 12)


@pytest.fixture(scope="module")
def case():
    """Weights, images, draws and R's of the depth-3 case, with the fp64 and fp32 gradients of the whole functional: computed once."""
    torch.manual_seed(0)
    sd = synth.make_state_dict(C, RANK, seed=1, kind="test", depth=DEPTH, gate_bias=0.85)
    x, _ = synth.make_batch(B, C, seed=1)
    g1, g2 = synth.make_noise(B, depth=DEPTH, seed=2, passes=1)
    keep = synth.make_dropout_masks(B, RANK, depth=DEPTH, seed=3, passes=1)
    draws = (g1.reshape(DEPTH, B, 196), g2.reshape(DEPTH, B, 196), keep.reshape(DEPTH, B * 197, RANK))
    gen = torch.Generator().manual_seed(5)
    R = TG.unit_R(gen, B, DEPTH, taps=(0, 2), tokens=True, gates=True)
    kw = dict(depth=DEPTH, mode="masked")
    g64, o64 = TG.tap_loss_grads(sd, x, draws, *R, dtype=torch.float64, **kw)
    g32, o32 = TG.tap_loss_grads(sd, x, draws, *R, dtype=torch.float32, **kw)
    return dict(sd=sd, x=x, draws=draws, R=R, kw=kw, g64=g64, g32=g32, o64=o64, o32=o32)


def test_reference_fp32_agrees_with_fp64(case):
    assert torch.equal(case["o64"]["token_select"] > 0.5, case["o32"]["token_select"] > 0.5), "fp32 and fp64 decide differently: choose other seeds"
    assert sorted(case["g64"]) == sorted(TG.backbone_names(case["sd"])) and not any(k.startswith("head.") for k in case["g64"])
    worst = 0.0
    for n, g in case["g64"].items():
        assert float(g.norm()) > 0, n + ": the functional does not reach this tensor"
        e = float((case["g32"][n].double() - g).norm() / g.norm())
        worst = max(worst, e)
        assert e < 2e-3, (n, e)
    print("tap_loss_grads fp32 against fp64: worst per-tensor rel L2 %.2e" % worst)


@pytest.mark.parametrize("name,form", [("blocks.0.adaptmlp.down_proj.weight", "complete"), ("blocks.2.adaptmlp.up_proj.weight", "student"),
                                       ("blocks.2.mlp_token_select.mlp_head.weight", "gate")])
def test_reference_against_finite_differences(case, name, form):
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in case["sd"].items()}
    x, R, kw = case["x"].double(), case["R"], case["kw"]
    draws = (case["draws"][0].double(), case["draws"][1].double(), case["draws"][2])
    if form == "gate":   # token_logits term alone (module docstring)
        R = (None, None, None, R[3])
        grads, _ = TG.tap_loss_grads(case["sd"], case["x"], case["draws"], *R, dtype=torch.float64, **kw)
    elif form == "complete":   # a tensor with gates downstream: the complete_model pass, whose forward value applies no mask
        R, kw = (R[0], R[1], None, R[3]), dict(kw, complete_model=True)
        grads, _ = TG.tap_loss_grads(case["sd"], case["x"], case["draws"], *R, dtype=torch.float64, **kw)
    else:   # the last block's adapter: no gate behind it, the whole student functional
        grads = case["g64"]
    gen = torch.Generator().manual_seed(11)
    d = torch.randn(sd64[name].shape, generator=gen, dtype=torch.float64)
    d /= d.norm()
    h = 1e-5

    def L(step):
        s = dict(sd64)
        s[name] = sd64[name] + step * d
        with torch.no_grad():
            val, out = TG.tap_functional(s, x, draws, *R, **kw)
        return float(val), out["token_select"]
    (lp, sp), (lm, sm) = L(h), L(-h)
    assert torch.equal(sp, sm), "a decision changes inside the difference step: choose another direction"
    fd = (lp - lm) / (2 * h)
    an = float((grads[name] * d).sum())
    print("%s: directional derivative %.9e, central difference %.9e, relative %.2e" % (name, an, fd, abs(fd - an) / abs(an)))
    assert abs(an) > 1e-8 and abs(fd - an) <= 1e-6 * abs(an), (name, an, fd)


def test_classification_identity(case):
    sd, x, draws = case["sd"], case["x"], case["draws"]
    y = torch.tensor([3, 7])
    names = TG.backbone_names(sd)
    leaf = {k: (v.double().clone().requires_grad_(True) if k in names else (v.double() if v.is_floating_point() else v)) for k, v in sd.items()}
    logits, _ = O.forward(leaf, x.double(), draws[0].double(), draws[1].double(), draws[2], depth=DEPTH, mode="masked")
    want = torch.autograd.grad(F.cross_entropy(logits, y), [leaf[k] for k in names], allow_unused=True)
    # R_tokens = d CE(head(tokens[:, 0])) / d tokens on the oracle's own tokens
    tok = case["o64"]["tokens"].clone().requires_grad_(True)
    ce = F.cross_entropy(F.linear(tok[:, 0], sd["head.weight"].double(), sd["head.bias"].double()), y)
    (R_tokens,) = torch.autograd.grad(ce, tok)
    got, _ = TG.tap_loss_grads(sd, x, draws, R_tokens, None, None, None, dtype=torch.float64, **case["kw"])
    for n, w in zip(names, want):
        w = torch.zeros_like(got[n]) if w is None else w
        e = float((got[n] - w).norm() / max(float(w.norm()), 1e-30))
        assert e < 1e-9, (n, e)   # the same fp64 graph, entered at the tokens instead of at the loss


def test_header_binding_and_signatures():
    import _lib
    hdr = open(os.path.join(ROOT, "include", "dyt_hip.h")).read()
    for name in ("dyt_forward_taps", "dyt_backward_tokens", "dyt_unit_ln_bwd_tap"):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SYMBOLS[name][1]), name
        assert name in _lib.OPTIONAL_SYMBOLS
    from runtime import DyTEngine
    p = inspect.signature(DyTEngine.forward_features_tokens).parameters
    assert p["save"].default is False and p["taps"].default is None
    assert list(inspect.signature(DyTEngine.backward_tokens).parameters)[:7] == ["self", "slot", "dtokens", "dtaps", "grad", "dtoken_select", "dtoken_logits"]
    from models.vision_transformer_IN21K import VisionTransformer
    assert list(inspect.signature(VisionTransformer.forward_features).parameters) == ["self", "x", "complete_model", "gumbel", "keep_mask", "out_indices"]
