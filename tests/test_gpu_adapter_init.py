"""GPU tests of the adapter at the reference's own init (pytest -m gpu).

The reference zero-inits up_proj and both adapter biases (models/dynamic_adapter.py:112-117) and warms the lr up from 0, so for the
first tens of steps |W_up| runs through 1e-8 .. 1e-4 -- below IEEE half's normal range (6.1e-5).  Every other parity test uses
up_proj ~ N(0, 0.02).  Here the same matrix is walked down a ladder of powers of two (synth.scale_up_proj) and every gradient is
held to the bar its mode already carries:
  * the sub-module C ABI (dyt_adapter_fwd / dyt_adapter_bwd) in both libraries against fp64 autograd;
  * one fused step of the whole model in five modes against the CPU oracle."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import gpu_diag as D  # noqa: E402
import parity_rules as PR  # noqa: E402
import synth  # noqa: E402
from oracle import dyt_oracle as O  # noqa: E402
from test_gpu_round2 import SPLIT_MODES  # noqa: E402

INF = float("inf")


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the sub-module entries
# ---------------------------------------------------------------------------------------------------------------------------
def _unit_inputs(r, M=1000, seed=0):
    g = torch.Generator().manual_seed(100 + r + seed)
    bound = 1.0 / 768 ** 0.5
    return dict(x=torch.randn(M, 768, generator=g), res=torch.randn(M, 768, generator=g),
                down_w=(torch.rand(r, 768, generator=g) * 2 - 1) * bound, down_b=torch.randn(r, generator=g) * 0.02,
                W=torch.randn(768, r, generator=g) * 0.02, up_b=torch.randn(768, generator=g) * 0.02,
                dout=torch.randn(M, 768, generator=g) * 0.01, keep=torch.rand(M, r, generator=g) > 0.1)


def _unit_run(L, prec, t, up_w, dout, scale=0.1):
    """dyt_adapter_fwd (with the residual) and dyt_adapter_bwd on one set of inputs: out, dx, d_down_w, d_down_b, d_up_w, d_up_b."""
    import _lib
    M, r = t["x"].shape[0], t["down_w"].shape[0]
    dev = lambda a: a.detach().float().contiguous().cuda()   # noqa: E731
    x, dw, db, uw, ub, res, go = dev(t["x"]), dev(t["down_w"]), dev(t["down_b"]), dev(up_w), dev(t["up_b"]), dev(t["res"]), dev(dout)
    km = t["keep"].to(torch.uint8).contiguous().cuda()
    out = torch.full((M, 768), float("nan"), device="cuda")
    _lib.check(L.dyt_adapter_fwd(_lib.ptr(x), _lib.ptr(dw), _lib.ptr(db), _lib.ptr(uw), _lib.ptr(ub), _lib.ptr(res), _lib.ptr(out), M, r,
                                 scale, 0.1, _lib.ptr(km), ctypes.c_uint64(0), prec, _lib.stream_ptr()), L)
    dx = torch.full((M, 768), float("nan"), device="cuda")
    gdw, gdb, guw, gub = torch.zeros(r, 768, device="cuda"), torch.zeros(r, device="cuda"), torch.zeros(768, r, device="cuda"), torch.zeros(768, device="cuda")
    _lib.check(L.dyt_adapter_bwd(_lib.ptr(x), _lib.ptr(dw), _lib.ptr(db), _lib.ptr(uw), _lib.ptr(go), _lib.ptr(dx), _lib.ptr(gdw), _lib.ptr(gdb),
                                 _lib.ptr(guw), _lib.ptr(gub), M, r, scale, 0.1, _lib.ptr(km), ctypes.c_uint64(0), prec, _lib.stream_ptr()), L)
    torch.cuda.synchronize()
    return dict(out=out.cpu(), dx=dx.cpu(), d_down_w=gdw.cpu(), d_down_b=gdb.cpu(), d_up_w=guw.cpu(), d_up_b=gub.cpu())


def _unit_ref(t, up_w, dout, scale=0.1):
    """fp64 autograd through the oracle's adapter (the form of test_adapter_submodule_forward_and_backward_vs_oracle)."""
    sd = {"blocks.0.adaptmlp.down_proj.weight": t["down_w"], "blocks.0.adaptmlp.down_proj.bias": t["down_b"],
          "blocks.0.adaptmlp.up_proj.weight": up_w, "blocks.0.adaptmlp.up_proj.bias": t["up_b"]}
    leaf = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    xg = t["x"].double().clone().requires_grad_(True)
    y = O.adapter(leaf, "blocks.0.", xg, scale, t["keep"], 0.1)
    (y * dout.double()).sum().backward()
    p = "blocks.0.adaptmlp."
    return dict(out=t["res"].double() + y.detach(), dx=xg.grad, d_down_w=leaf[p + "down_proj.weight"].grad,
                d_down_b=leaf[p + "down_proj.bias"].grad, d_up_w=leaf[p + "up_proj.weight"].grad, d_up_b=leaf[p + "up_proj.bias"].grad)


def _rel(got, ref):
    return float((got.double() - ref).norm() / (ref.norm() + 1e-300))


@pytest.mark.parametrize("fp16", [False, True], ids=["bf16lib", "fp16lib"])
@pytest.mark.parametrize("r", [16, 64])
def test_adapter_submodule_from_zero_up_proj(fp16, r):
    """dyt_adapter_fwd / dyt_adapter_bwd with up_proj exactly 0 and at 2^-k x N(0, 0.02), k = 0, 8, 14, 20, 26 (|w| 2e-2 .. 3e-10),
    and with dout at 2^-16 x its size, at precision 0 (fp32) and 1 (the library's 16-bit type).
      zero:  dx, d_down_w, d_down_b exactly 0, out = residual + scale up_b bit for bit, everything finite;
      fp32:  dx, d_down_w, d_down_b scale by exactly 2^-k, d_up_w / d_up_b unchanged, bit for bit;
      16-bit: the relative error of every output against fp64 at every rung <= 1.5 x its error at k = 0."""
    import _lib
    L = _lib.lib(fp16=fp16)
    t = _unit_inputs(r)
    scale = 0.1
    for prec in (0, 1):
        tag = "%s r=%d precision=%d" % ("fp16 lib" if fp16 else "bf16 lib", r, prec)
        # ---- up_proj exactly 0 ----
        z = _unit_run(L, prec, t, torch.zeros(768, r), t["dout"])
        for k, v in z.items():
            assert bool(torch.isfinite(v).all()), (tag, k)
        for k in ("dx", "d_down_w", "d_down_b"):
            assert z[k].count_nonzero() == 0, (tag, k, float(z[k].abs().max()))
        res, ub = t["res"], t["up_b"]
        plain = res + torch.tensor(scale, dtype=torch.float32) * ub                    # round(res + round(s b))
        fused = (res.double() + torch.tensor(scale, dtype=torch.float32).double() * ub.double()).float()   # round(res + s b): contracted
        same = (z["out"] == plain) | (z["out"] == fused)
        assert bool(same.all()), (tag, int((~same).sum()), float((z["out"] - plain).abs().max()))
        # ---- the up_proj ladder ----
        base, errs = None, {}
        for k in (0, 8, 14, 20, 26):
            uw = t["W"] * 2.0 ** -k
            got = _unit_run(L, prec, t, uw, t["dout"])
            ref = _unit_ref(t, uw, t["dout"], scale)
            errs[k] = {n: _rel(got[n], ref[n]) for n in got}
            for n, v in got.items():
                assert bool(torch.isfinite(v).all()), (tag, k, n)
            if k == 0:
                base = got
            elif prec == 0:
                for n in ("dx", "d_down_w", "d_down_b"):
                    assert torch.equal(got[n], base[n] * 2.0 ** -k), (tag, k, n, float((got[n] - base[n] * 2.0 ** -k).abs().max()))
                for n in ("d_up_w", "d_up_b"):
                    assert torch.equal(got[n], base[n]), (tag, k, n)
        print("%s rel-L2 vs fp64 per rung k:" % tag)
        for k, e in errs.items():
            print("    k=%2d  " % k + "  ".join("%s %.2e" % (n, v) for n, v in e.items()))
        if prec == 1:
            for k, e in errs.items():
                for n, v in e.items():
                    assert v <= 1.5 * errs[0][n] + 1e-12, (tag, k, n, v, errs[0][n])
        # ---- gradient-sized dout ----
        de = {}
        for k in (0, 16):
            go = t["dout"] * 2.0 ** -k
            got, ref = _unit_run(L, prec, t, t["W"], go), _unit_ref(t, t["W"], go, scale)
            de[k] = {n: _rel(got[n], ref[n]) for n in got if n != "out"}
        print("%s dout x 2^-16: " % tag + "  ".join("%s %.2e (k=0: %.2e)" % (n, de[16][n], de[0][n]) for n in de[0]))
        for n in de[0]:
            assert de[16][n] <= 1.5 * de[0][n] + 1e-12, (tag, n, de[16][n], de[0][n])


# ---------------------------------------------------------------------------------------------------------------------------
# 2. one fused step of the whole model
# ---------------------------------------------------------------------------------------------------------------------------
LADDER = (INF, 6, 12, 18, 24)
B, C, R, MODE, TARGET, SEED = 4, 100, 64, "compact", 0.5, 11
_oracle = {}


def _ladder_sd(k):
    return synth.scale_up_proj(synth.reference_adapter_init(synth.make_state_dict(C, R, seed=0, kind="test", gate_bias=0.85)), k)


def _inputs():
    x, y = synth.make_batch(B, C, seed=SEED)
    g1, g2 = synth.make_noise(B, seed=SEED + 1)
    keep = synth.make_dropout_masks(B, R, seed=SEED + 2)
    return x, y, g1, g2, keep


def _oracle_at(k):
    """One oracle step (and its tie band) per rung, shared by the five modes."""
    if k not in _oracle:
        sd = _ladder_sd(k)
        x, y, g1, g2, keep = _inputs()
        d_ref, g_ref, (ref_ls, ref_lt, tok) = O.step_grads(sd, x, y, g1, g2, keep, scale=0.1, mode=MODE, token_target_ratio=TARGET)
        tl = tok["token_logits"].detach()[..., 0]
        z = ((tl.permute(1, 0, 2) + g1[0] - g2[0]) / 5.0).abs().permute(1, 0, 2)   # [B,12,196] decision margins
        band = PR.tie_band(sd, x, g1[0], g2[0], keep[0], MODE, tl, key=("adapter_init", B, C, R, MODE, SEED, k))
        _oracle[k] = (sd, d_ref, g_ref, ref_ls.detach(), tok["token_select"].detach()[..., 0].float(), z, band)
    return _oracle[k]


def _tol(name, prec):
    if prec == "fp32":
        return 2e-3
    if prec in SPLIT_MODES:
        return D.TOL[prec]["grad"]
    return (D.FP16_GRAD_TOL_SMALL_B if prec == "fp16" else D.BF16_GRAD_TOL_SMALL_B)[D.grad_kind(name)]


def _model(prec, sd):
    from models.vision_transformer_IN21K import vit_base_patch16_224_in21k
    tuning = D.Cfg(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option="none", ffn_adapter_init_option="lora",
                   ffn_adapter_scalar="0.1", ffn_num=R, d_model=768)
    m = vit_base_patch16_224_in21k(num_classes=C, drop_path_rate=0.0, tuning_config=tuning, select_config=D.Cfg(open=True, keep_layers=0),
                                   precision=prec, train_mode=MODE, max_batch=B)
    m.load_state_dict(sd)
    for n, p in m.named_parameters():
        p.requires_grad = synth.is_trainable(n)
    return m.cuda().train()


def _step_and_compare(prec, eng, sd, inputs, g_ref, ref_ls, ref_ts, z, band, zero_down, tag):
    """One step_fwd_bwd of `eng` on the injected draws, judged against the oracle's step by the rules of test_gpu_round2.py: the tie rule
    for the modes with exact masks, the ReLU-side rule for down_proj rows, each mode's own bars on all 74 gradients (the 12 gate biases
    as one 12-vector); zero_down: every down_proj gradient exactly 0.  Returns the worst rel-L2 per tensor kind (None: a tie flipped)."""
    x, y, g1, g2, keep = inputs
    ls = torch.empty(B, C, device="cuda"); lt = torch.empty(B, C, device="cuda"); ts = torch.zeros(B, 12, 196, device="cuda")
    losses = eng.step_fwd_bwd(x.cuda(), y.cuda(), TARGET, 2.0, 0.0, 0.0, g1=g1.cuda().contiguous(), g2=g2.cuda().contiguous(),
                              keep_mask=keep.cuda().contiguous(), logits_s=ls, logits_t=lt, token_select=ts).cpu()
    assert bool(torch.isfinite(losses).all()) and bool(torch.isfinite(eng.grad).all()), (prec, tag)
    flip = ts.cpu() != ref_ts
    if prec == "fp32" or prec in SPLIT_MODES:
        n, outside, zmax, blk = PR.judge_decisions(flip, z, band)
        assert outside == 0, (prec, tag, n, outside, zmax, blk)
        if n:   # a tie went the other way: the later blocks see another token set
            print("%s %s: %d decision(s) inside the tie band differ; gradients not compared" % (prec, tag, n))
            return None
    else:
        assert int(flip.sum()) <= (max(6, B // 4) if prec == "fp16" else max(8, B * 3 // 2)), (prec, tag, int(flip.sum()))   # test_gpu_round2.py's rule
    ltol = {"fp16": 0.015, "bf16": 0.03}.get(prec, 1e-3)
    assert float((ls.cpu() - ref_ls).abs().max()) < ltol, (prec, tag)
    relu = PR.ReluSideBudget(eng, sd, x, g1, g2, keep, MODE)
    worst, scalars = {}, []
    for n, gr in g_ref.items():
        got = eng.trainable_view(n, gr.shape, eng.grad).cpu()
        if zero_down and "down_proj" in n:
            assert gr.count_nonzero() == 0 and got.count_nonzero() == 0, (prec, n, float(got.abs().max()))
            continue
        if gr.numel() == 1:   # the 12 gate biases, judged as one 12-vector (test_gpu_round2.py)
            scalars.append((float(got), float(gr)))
            continue
        e = float((got - gr).norm() / (gr.norm() + 1e-30))
        if e >= _tol(n, prec) and prec in SPLIT_MODES and "down_proj" in n:
            e = relu.without_side_units(n, got, gr, e, "%s %s %s" % (prec, tag, n), fwd_roundoff=1e-4)
        assert e < _tol(n, prec), (prec, tag, n, e)
        kind = D.grad_kind(n)
        worst[kind] = max(worst.get(kind, 0.0), e)
    a, b = torch.tensor(scalars, dtype=torch.float64).unbind(1)
    e = float((a - b).norm() / (b.norm() + 1e-30))
    assert e < _tol("mlp_token_select.mlp_head.bias", prec), (prec, tag, e)
    worst["gate bias"] = e
    return worst


@pytest.mark.parametrize("prec", ["fp32", "fp16x3q", "fp16x3h", "fp16", "bf16"])
def test_step_from_reference_adapter_init_vs_oracle(prec):
    """Image model, compact mode, B = 4, C = 100, r = 64, weights of synth.reference_adapter_init with up_proj = 2^-k x N(0, 0.02),
    k = inf (exact 0), 6, 12, 18, 24: one step_fwd_bwd against O.step_grads.  All 74 gradients within the bar the mode already carries
    (fp32 2e-3; fp16x3q / fp16x3h TOL["grad"]; fp16 / bf16 the small-batch tables of gpu_diag) at every rung, gate decisions by the one
    tie rule, down_proj rows only by the one ReLU-side rule; at k = inf every down_proj gradient is exactly 0.  Prints the errors of
    down_proj, the gate and up_proj per rung."""
    x, y, g1, g2, keep = _inputs()
    m = None
    rows = []
    for k in LADDER:
        sd, d_ref, g_ref, ref_ls, ref_ts, z, band = _oracle_at(k)
        if m is None:
            m = _model(prec, sd)
            eng = m.engine(B, torch.device("cuda", 0))
        else:   # the same engine, new adapter weights (the frozen backbone is the same at every rung)
            for n in sd:
                if "adaptmlp." in n:
                    eng.set_param(n, sd[n])
        worst = _step_and_compare(prec, eng, sd, (x, y, g1, g2, keep), g_ref, ref_ls, ref_ts, z, band, zero_down=(k == INF), tag="k=%s" % k)
        if worst is None:
            continue
        rows.append((k, worst))
    print("%s: worst rel-L2 per tensor kind and rung" % prec)
    for k, w in rows:
        print("    k=%-4s " % ("inf" if k == INF else k) + "  ".join("%s %.2e" % (n, v) for n, v in sorted(w.items())))
    del m, eng
    torch.cuda.empty_cache()


@pytest.mark.parametrize("prec", ["fp16x3q", "fp16"])
def test_warmup_steps_from_reference_adapter_init_vs_oracle(prec):
    """The regime reached the way a real run reaches it: synth.reference_adapter_init, then four steps of the oracle with the AdamW update
    of main_image.py:285 (O.adamw_update) at the warm-up lr of util/lr_sched.py (O.lr_at, lr 1e-3 warmed up over one epoch of 10 000
    iterations: 0, 1e-7, 2e-7, 3e-7), so up_proj runs 0 -> ~1e-7 -> ~3e-7.  At every step the library computes the gradients at the
    oracle's parameters (its own update would move each weight by about +-lr wherever the sign of a near-zero gradient differs, which
    the next step's down_proj gradient would then measure) and they are held to the mode's bars (step 0: down_proj exactly 0)."""
    lr0, wd, epoch_len = 1e-3, 0.05, 10000
    sd = _ladder_sd(INF)
    names = O.trainable_names(sd)
    ref = {k: v.clone() for k, v in sd.items()}
    mom = {k: (torch.zeros_like(sd[k]), torch.zeros_like(sd[k])) for k in names}
    m = _model(prec, sd)
    eng = m.engine(B, torch.device("cuda", 0))
    rows = []
    for it in range(4):
        lr = O.lr_at(it / epoch_len, lr0, 1e-6, 1, 10)
        x, y = synth.make_batch(B, C, seed=SEED + 10 * it)
        g1, g2 = synth.make_noise(B, seed=SEED + 10 * it + 1)
        keep = synth.make_dropout_masks(B, R, seed=SEED + 10 * it + 2)
        _, g_ref, (ref_ls, _, tok) = O.step_grads(ref, x, y, g1, g2, keep, scale=0.1, mode=MODE, token_target_ratio=TARGET)
        tl = tok["token_logits"].detach()[..., 0]
        z = ((tl.permute(1, 0, 2) + g1[0] - g2[0]) / 5.0).abs().permute(1, 0, 2)
        band = PR.tie_band(ref, x, g1[0], g2[0], keep[0], MODE, tl, key=("adapter_warmup", B, C, R, MODE, SEED, it))
        up = max(float(ref[k].abs().max()) for k in names if "up_proj.weight" in k)
        for k in names:
            eng.set_param(k, ref[k])
        worst = _step_and_compare(prec, eng, ref, (x, y, g1, g2, keep), g_ref, ref_ls.detach(), tok["token_select"].detach()[..., 0].float(),
                                  z, band, zero_down=(it == 0), tag="step %d" % it)
        if worst is not None:   # (None: a tie inside the band flipped -- that step's gradients are not compared)
            rows.append((it, lr, up, worst))
        for k in names:
            p, mm, vv = O.adamw_update(ref[k], g_ref[k], mom[k][0], mom[k][1], it + 1, lr, wd)
            ref[k], mom[k] = p, (mm, vv)
    print("%s: warm-up steps from the reference init, worst rel-L2 per tensor kind" % prec)
    for it, lr, up, w in rows:
        print("    step %d lr %.1e max|up_proj| %.1e  " % (it, lr, up) + "  ".join("%s %.2e" % (n, v) for n, v in sorted(w.items())))
    del m, eng
    torch.cuda.empty_cache()
