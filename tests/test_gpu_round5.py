"""GPU tests added in round 5 (pytest -m gpu), all through the C ABI.
  * the round-5 attention kernels (csrc/attention_v2.hip) against an fp64 restatement of Attention.forward
    (models/vision_transformer_IN21K.py:60-70 of the reference) and its autograd backward, against the round 1-4 kernels, and
    bit for bit against themselves (run to run; the cls-only tail against the full gradient is held by
    tests/test_gpu_unit_attention.py::test_cls_only_tail_equals_the_full_gradient)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _attn_ref(qkv, B, dout):
    x = qkv.double().reshape(B, 197, 3, 12, 64).permute(2, 0, 3, 1, 4).clone().requires_grad_(True)
    q, k, v = x[0], x[1], x[2]
    s = (q * 0.125) @ k.transpose(-1, -2)
    o = (s.softmax(-1) @ v).transpose(1, 2).reshape(B * 197, 768)
    o.backward(dout.double())
    return o.detach(), x.grad.permute(1, 3, 0, 2, 4).reshape(B * 197, 2304)


def _run(L, qkv, dout, B):
    from _lib import check, ptr, stream_ptr
    out = torch.full((B * 197, 768), float("nan"), device="cuda")
    dqkv = torch.full((B * 197, 2304), float("nan"), device="cuda")
    check(L.dyt_attention(ptr(qkv), ptr(out), ptr(dout), ptr(dqkv), B, 1, stream_ptr()), L)
    torch.cuda.synchronize()
    return out, dqkv


@pytest.mark.parametrize("fp16", [True, False])
@pytest.mark.parametrize("B", [1, 3, 23])
def test_attention_v2_vs_fp64_and_vs_round4_kernels(B, fp16):
    """Forward and backward of the round-5 kernels at 12 / 36 / 276 (image, head) pairs (276 > 256 persistent workgroups: the
    second head of a workgroup runs on prefetched images and rotated LDS slots) in both 16-bit operand types: no further from fp64
    than 1.5x the round 1-4 kernels (+ 2e-4 of the tensor's maximum), which stay available behind DYT_OPT_ATTN_V2 = 0.  The
    inputs carry spikes (one key row x 6) so that the forward's deferred running-max update is taken after the first key tile."""
    import _lib
    from _lib import check
    L = _lib.lib(fp16=fp16)
    g = torch.Generator().manual_seed(100 + B)
    qkv = torch.randn(B * 197, 2304, generator=g) * 1.5
    qkv[100::197, 768:1536] *= 6.0     # token 100 of every image: keys far above the first tile's maximum (tile 3)
    qkv[190::197, 768 + 64:768 + 128] *= 9.0   # and one head's key in the last full tile
    dout = torch.randn(B * 197, 768, generator=g)
    ref_o, ref_g = _attn_ref(qkv, B, dout)
    qd, dd = qkv.cuda(), dout.cuda()
    res = {}
    for v2 in (0, 3):
        check(L.dyt_set_global_option(_lib.OPT_ATTN_V2, v2))
        res[v2] = _run(L, qd, dd, B)
    check(L.dyt_set_global_option(_lib.OPT_ATTN_V2, 3))

    def err(a, b):
        return float((a.cpu().double() - b).abs().max() / b.abs().max())
    for name, sl in (("out", None), ("dq", slice(0, 768)), ("dk", slice(768, 1536)), ("dv", slice(1536, 2304))):
        if sl is None:
            e0, e3 = err(res[0][0], ref_o), err(res[3][0], ref_o)
        else:
            e0, e3 = err(res[0][1][:, sl], ref_g[:, sl]), err(res[3][1][:, sl], ref_g[:, sl])
        print("B=%d fp16=%d %s: round-4 kernels %.2e, round-5 kernels %.2e of max|ref|" % (B, fp16, name, e0, e3))
        assert torch.isfinite(res[3][0]).all() and torch.isfinite(res[3][1]).all()
        assert e3 < 1.5 * e0 + 2e-4, (name, e0, e3)
        assert e3 < (8e-3 if fp16 else 6e-2), (name, e3)   # spiky inputs: the round-4 kernels sit at 3e-3 / 3e-2 here


@pytest.mark.parametrize("B", [3, 128])
def test_attention_v2_is_bitwise_reproducible(B):
    """Four launches of the round-5 forward + backward on the same operands give the same bits (B=128: six heads per persistent
    workgroup, every prefetch / slot rotation / deferred store in steady state).  This is the test that caught a matrix-core -> VALU
    read hazard hipcc does not pad for inline asm (attention_v2.hip: acc_max16)."""
    import _lib
    L = _lib.lib(fp16=True)
    g = torch.Generator(device="cuda").manual_seed(B)
    qkv = torch.randn(B * 197, 2304, device="cuda", generator=g) * 1.5
    dout = torch.randn(B * 197, 768, device="cuda", generator=g)
    first = _run(L, qkv, dout, B)
    for rep in range(3):
        again = _run(L, qkv, dout, B)
        assert torch.equal(again[0], first[0]), (rep, int((again[0] != first[0]).sum()))
        assert torch.equal(again[1], first[1]), (rep, int((again[1] != first[1]).sum()))


# Worst over the five draws (B=16, compact, LayerNorm-2 folded = the default; profiles/round4/r4_ln_fold_ab.txt, re-measured by this test and
# printed): what bench.py / INTEGRATION.md quote for the headline mode.  Bounds = ~1.3 x the worst draw.
FAST_MODE_WORST = {
    # prec: (student logits, teacher logits, differing decisions of 37 632, gate, down_proj, up_proj, head gradient rel-L2)
    "fp16": dict(ls=4.8e-3, lt=1.9e-3, flips=4, gate=2.6e-2, down=8.2e-2, up=1.1e-3, head=8.2e-4),
    "bf16": dict(ls=1.9e-2, lt=1.3e-2, flips=20, gate=6.1e-2, down=9.9e-2, up=8.3e-3, head=6.4e-3),
}
FAST_MODE_BOUND = {
    "fp16": dict(ls=6.5e-3, lt=2.5e-3, flips=6, gate=4e-2, down=0.12, up=2e-3, head=1.5e-3),
    "bf16": dict(ls=2.6e-2, lt=1.8e-2, flips=28, gate=9e-2, down=0.14, up=1.2e-2, head=9e-3),
}


@pytest.mark.parametrize("seed", [31, 41, 51, 61, 71])
@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_fast_modes_vs_oracle_over_seeds(prec, seed):
    """The headline mode (fp16: the reference's own autocast dtype, engine_finetune.py:47) and bf16 against the CPU oracle at BASELINE
    configs[0] size over the same five draws the parity modes are judged on -- NOT inside north_star's 1e-3 / bit-exact bar, and the
    numbers quoted for them are the WORST of these draws (bench.py quoted the best)."""
    import synth
    from oracle import dyt_oracle as O
    from test_gpu_round2 import _bench_model
    B, C, r, target, mode = 16, 100, 64, 0.5, "compact"
    x, y = synth.make_batch(B, C, seed=seed)
    g1, g2 = synth.make_noise(B, seed=seed + 1)
    keep = synth.make_dropout_masks(B, r, seed=seed + 2)
    sd = synth.make_state_dict(C, r, seed=0, kind="test", gate_bias=0.85)
    d_ref, g_ref, (ref_ls, ref_lt, tok) = O.step_grads(sd, x, y, g1, g2, keep, scale=0.1, mode=mode, token_target_ratio=target)
    m, _ = _bench_model(prec, mode, B, 0.85, classes=C, r=r, kind="test")
    m.train()
    eng = m.engine(B, torch.device("cuda", 0))
    ls = torch.empty(B, C, device="cuda"); lt = torch.empty(B, C, device="cuda"); ts = torch.zeros(B, 12, 196, device="cuda")
    eng.step_fwd_bwd(x.cuda(), y.cuda(), target, 2.0, 0.0, 0.0, g1=g1.cuda().contiguous(), g2=g2.cuda().contiguous(),
                     keep_mask=keep.cuda().contiguous(), logits_s=ls, logits_t=lt, token_select=ts)
    got = dict(ls=float((ls.cpu() - ref_ls.detach()).abs().max()), lt=float((lt.cpu() - ref_lt.detach()).abs().max()),
               flips=int((ts.cpu() != tok["token_select"].detach()[..., 0].float()).sum()), gate=0.0, down=0.0, up=0.0, head=0.0)
    for n, gr in g_ref.items():
        if gr.numel() == 1:
            continue
        e = float((eng.trainable_view(n, gr.shape, eng.grad).cpu() - gr).norm() / (gr.norm() + 1e-20))
        k = "gate" if "mlp_token_select" in n else "down" if "down_proj" in n else "up" if "up_proj" in n else "head"
        got[k] = max(got[k], e)
    print("%s seed %d: logits %.2e / %.2e, %d of %d decisions differ, gradients gate %.1e down_proj %.1e up_proj %.1e head %.1e" % (
        prec, seed, got["ls"], got["lt"], got["flips"], ts.numel(), got["gate"], got["down"], got["up"], got["head"]))
    for k, bound in FAST_MODE_BOUND[prec].items():
        assert got[k] <= bound, (prec, seed, k, got[k], bound)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("B", [5, 23, 130])
def test_splitk_cls_tail_gemms_agree_with_the_tile_kernels_and_are_reproducible(precision, B):
    """DYT_OPT_GEMM_SPLITK (csrc/gemm_skinny.h): the two K = 3072 GEMMs of the cls-only last block -- fc2 forward with the adapter's operand
    pair, fc1 dgrad -- as 256-wide k slices + a reduce launch that runs the epilogue functor.  Against the same step on the 128x128 tile
    kernels: identical masks, logits / losses / the flat gradient to the rounding of a different fp32 summation order; the split form itself
    twice: identical bits.  B = 5 and 23 leave partial 32-row groups (rows past the batch are neither read nor stored); B = 130 takes a second,
    mostly empty 128-row workgroup row."""
    import _lib
    import synth
    from test_gpu_parity import _bench_model
    x, y = synth.make_batch(B, 100, seed=41)
    g1, g2 = synth.make_noise(B, seed=42)
    keep = synth.make_dropout_masks(B, 64, seed=43)
    L = _lib.lib(fp16=(precision == "fp16"))
    res = []
    try:
        for splitk in (0, 1, 1):
            _lib.check(L.dyt_set_global_option(_lib.OPT_GEMM_SPLITK, splitk))
            m = _bench_model(precision, "compact", B, 0.7)
            m.train()
            eng = m.engine(B, torch.device("cuda", 0))
            ls = torch.empty(B, 100, device="cuda")
            ts = torch.zeros(B, 12, 196, device="cuda")
            losses = eng.step_fwd_bwd(x.cuda(), y.cuda(), 0.5, 2.0, 0.0, 0.0, g1=g1.cuda().contiguous(), g2=g2.cuda().contiguous(),
                                      keep_mask=keep.cuda().contiguous(), logits_s=ls, token_select=ts).clone()
            torch.cuda.synchronize()
            res.append((losses.cpu(), ls.cpu(), ts.cpu(), eng.grad.clone().cpu()))
            del m, eng
    finally:
        _lib.check(L.dyt_set_global_option(_lib.OPT_GEMM_SPLITK, 1))
    tile, sk, sk2 = res
    for a, b in zip(sk, sk2):
        assert torch.equal(a, b)
    assert torch.equal(sk[2], tile[2])
    tol = 1e-3 if precision == "fp16" else 4e-3
    dl = float((sk[1] - tile[1]).abs().max())
    dg = float((sk[3] - tile[3]).norm() / tile[3].norm())
    print("%s B=%d split-K vs tiles: logits %.2e, losses %.2e, gradient (relative norm) %.2e" % (precision, B, dl, float((sk[0][:5] - tile[0][:5]).abs().max()), dg))
    assert dl < tol and dg < tol * 5 and float((sk[0][:5] - tile[0][:5]).abs().max()) < tol * 5
    assert torch.isfinite(sk[3]).all()


@pytest.mark.parametrize("precision", ["fp16x3q"])   # (the only mode whose complete_model pass takes the one-part attention)
def test_complete_model_attention_of_the_exact_forward_modes_on_the_round5_kernel(precision):
    """The complete_model (teacher) pass of the exact-forward modes takes the hi * hi product alone in its attention forward.  With
    DYT_OPT_ATTN_V2 bit 0 that product runs on the round-5 16-bit kernel (planes as they are, the fp32 result split into the proj GEMM's
    [hi | e4m3 | e4m3] operand image on the way out) instead of attn_fwd_split_kernel<PLANES, 1>: the teacher logits of a step stay within
    1e-4 of the round-4 kernel's, the student logits / masks (three-part attention: untouched) are bit-identical, the gradient agrees to
    1e-3 of its norm; and the step is reproducible bit for bit."""
    import _lib
    import synth
    from test_gpu_parity import _bench_model
    B = 6
    x, y = synth.make_batch(B, 100, seed=51)
    g1, g2 = synth.make_noise(B, seed=52)
    keep = synth.make_dropout_masks(B, 64, seed=53)
    L = _lib.lib(fp16=True)
    res = []
    try:
        for v2 in (2, 3, 3):   # 2: the round-5 backward with the round-4 forward kernels -> only the teacher's forward attention differs
            _lib.check(L.dyt_set_global_option(_lib.OPT_ATTN_V2, v2))
            m = _bench_model(precision, "compact", B, 0.7)
            m.train()
            eng = m.engine(B, torch.device("cuda", 0))
            ls = torch.empty(B, 100, device="cuda")
            lt = torch.empty(B, 100, device="cuda")
            ts = torch.zeros(B, 12, 196, device="cuda")
            eng.step_fwd_bwd(x.cuda(), y.cuda(), 0.5, 2.0, 0.0, 0.0, g1=g1.cuda().contiguous(), g2=g2.cuda().contiguous(),
                             keep_mask=keep.cuda().contiguous(), logits_s=ls, logits_t=lt, token_select=ts)
            torch.cuda.synchronize()
            res.append((ls.cpu(), lt.cpu(), ts.cpu(), eng.grad.clone().cpu()))
            del m, eng
    finally:
        _lib.check(L.dyt_set_global_option(_lib.OPT_ATTN_V2, 3))
    old, new, new2 = res
    for a, b in zip(new, new2):
        assert torch.equal(a, b)
    assert torch.equal(new[2], old[2])
    dt = float((new[1] - old[1]).abs().max())
    ds = float((new[0] - old[0]).abs().max())
    dg = float((new[3] - old[3]).norm() / old[3].norm())
    print("%s B=%d teacher logits %.2e, student logits %.2e, gradient (relative norm) %.2e vs the round-4 one-part kernel" % (precision, B, dt, ds, dg))
    assert dt < 1e-4 and dg < 1e-3 and ds == 0.0
    assert torch.isfinite(new[3]).all()


# ---- stochastic depth (dyt_set_drop_path; reference models/vision_transformer_IN21K.py:121,131,148,159,285) ----
def _drop_path_model(g, precision, mode, rate):
    import gpu_diag as D
    import synth
    from models.vision_transformer_IN21K import vit_base_patch16_224_in21k
    C, r = int(g["meta_num_classes"]), int(g["meta_ffn_num"])
    sd = synth.make_state_dict(C, r, seed=int(g["meta_seed"]), kind="test", gate_bias=float(g["meta_gate_bias"]))
    tuning = D.Cfg(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option="none", ffn_adapter_init_option="lora",
                   ffn_adapter_scalar=str(float(g["meta_scale"])), ffn_num=r, d_model=768)
    m = vit_base_patch16_224_in21k(num_classes=C, drop_path_rate=rate, tuning_config=tuning, select_config=D.Cfg(open=True, keep_layers=0),
                                   precision=precision, train_mode=mode)
    m.load_state_dict(sd, strict=True)
    for n, p in m.named_parameters():
        p.requires_grad = synth.is_trainable(n)
    return m.cuda(), sd


@pytest.mark.parametrize("precision", ["fp32", "fp16x3", "fp16x3q", "fp16", "bf16"])
def test_drop_path_step_vs_reference_golden_and_oracle(precision):
    """drop_path_rate = 0.3 with the reference's recorded Bernoulli draws injected (tests/golden/drop_path_step.npz: the REAL reference model
    stepped through its own train_one_epoch; 31 of the two passes' 88 branch instances dropped): logits, masks, the five loss components and
    the gradients of a step against the reference's (masked mode) and against the oracle's compact-mode semantics, in the exact mode, the
    parity mode and both fast modes, at the bounds the drop_path 0 goldens are held to (tests/gpu_diag.py TOL)."""
    import os
    import numpy as np
    import gpu_diag as D
    import synth
    from oracle import dyt_oracle as O
    g = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "drop_path_step.npz")))
    B, C, r, seed = int(g["meta_batch"]), int(g["meta_num_classes"]), int(g["meta_ffn_num"]), int(g["meta_seed"])
    x, y = synth.make_batch(B, C, seed=seed)
    keep = synth.make_dropout_masks(B, r, seed=seed + 3)
    g1, g2 = torch.from_numpy(g["g1"]), torch.from_numpy(g["g2"])
    scales = torch.from_numpy(g["drop_scales"])
    tol = D.TOL[precision]
    for mode in ("masked", "compact"):
        model, sd = _drop_path_model(g, precision, mode, float(g["meta_rate"]))
        model.train()
        eng = model.engine(B, torch.device("cuda", 0))
        assert eng.drop_path_rate == pytest.approx(0.3)
        sc = [scales[p].cuda().contiguous() for p in range(2)]
        eng.set_drop_path_scales(0, sc[0])
        eng.set_drop_path_scales(1, sc[1])
        ls, lt = torch.empty(B, C, device="cuda"), torch.empty(B, C, device="cuda")
        ts = torch.zeros(B, 12, 196, device="cuda")
        losses = eng.step_fwd_bwd(x.cuda(), y.cuda(), 0.5, 2.0, 0.0, 0.0, masked_dense=(mode == "masked"), g1=g1.cuda().contiguous(),
                                  g2=g2.cuda().contiguous(), keep_mask=keep.cuda().contiguous(), logits_s=ls, logits_t=lt, token_select=ts).cpu()
        assert torch.equal(eng.debug_drop_path(0, B).cpu(), scales[0]) and torch.equal(eng.debug_drop_path(1, B).cpu(), scales[1])
        es = float(np.abs(ls.cpu().numpy() - g["logits_student"]).max())
        et = float(np.abs(lt.cpu().numpy() - g["logits_teacher"]).max())
        flips = int((ts.cpu().numpy().astype(np.uint8) != g["token_select"][..., 0]).sum())
        el = max(abs(float(losses[i]) - float(g["stat_" + k])) / max(1.0, abs(float(g["stat_" + k])))
                 for i, k in enumerate(("loss", "base_loss", "token_loss", "teacher_loss", "distillation_loss")))
        if mode == "masked":
            gref = {n[len("grad/"):]: torch.from_numpy(v) for n, v in g.items() if n.startswith("grad/")}
        else:
            _, gref, _ = O.step_grads(sd, x, y, g1, g2, keep, scale=float(g["meta_scale"]), mode="compact", drop_scales=scales)
        worst = {}
        items = [(n, eng.trainable_view(n, gr.shape, eng.grad).cpu(), gr) for n, gr in gref.items()]
        if precision != "fp32":   # the 12 one-number gate bias gradients as one vector (gpu_diag.report_grads)
            sc1 = [it for it in items if it[2].numel() == 1]
            items = [it for it in items if it[2].numel() > 1]
            if sc1:
                items.append(("mlp_token_select.mlp_head.bias (12 blocks)", torch.stack([a.reshape(()) for _, a, _ in sc1]), torch.stack([b.reshape(()) for _, _, b in sc1])))
        for n, got, ref in items:
            e = float((got - ref).norm() / max(float(ref.norm()), 1e-20))
            k = D.grad_kind(n) if precision in ("fp16", "bf16") else "all"
            if e > worst.get(k, (0.0, ""))[0]:
                worst[k] = (e, n)
        print("drop_path %s/%s: logits %.2e / %.2e, %d of %d decisions differ, losses %.1e, gradients %s" %
              (precision, mode, es, et, flips, ts.numel(), el, {k: "%.1e" % v[0] for k, v in worst.items()}))
        assert es <= tol["logits"] and et <= tol["logits"] and flips <= tol["step_flips"] and el <= tol["loss"]
        for k, (e, n) in worst.items():
            bound = 2e-3 if precision == "fp32" else (tol["grad"] if precision in D.SPLIT_MODES else
                                                     (D.FP16_GRAD_TOL_SMALL_B if precision == "fp16" else D.BF16_GRAD_TOL_SMALL_B)[k])
            assert e <= bound, (mode, k, n, e, bound)
        eng.set_drop_path_scales(0, None)
        eng.set_drop_path_scales(1, None)
        del model, eng
        torch.cuda.empty_cache()


def test_drop_path_library_draws_eval_and_rate_zero():
    """The library's own draws: factors are 0 or 1 / keep_l with keep_l = 1 - rate l / 11, block 0 never dropped, the two passes and the two
    branches draw independently, the kept fraction of 2 x 11 x 64 draws per pass is within 4 sigma of its expectation; the same seed gives the same
    step bit for bit, another seed another; evaluation passes and rate 0 are untouched (bit-identical to a model built without drop_path)."""
    import synth
    g = {"meta_num_classes": 10, "meta_ffn_num": 8, "meta_seed": 5, "meta_gate_bias": 0.3, "meta_scale": 1.0}
    B, rate = 64, 0.4
    x, y = synth.make_batch(B, 10, seed=61)
    xd, yd = x.cuda(), y.cuda()

    def step(model, seed):
        eng = model.engine(B, torch.device("cuda", 0))
        ls = torch.empty(B, 10, device="cuda")
        losses = eng.step_fwd_bwd(xd, yd, 0.5, 2.0, 0.0, 0.0, seed=seed, logits_s=ls).clone()
        torch.cuda.synchronize()
        return eng, losses.cpu(), ls.cpu(), eng.grad.clone().cpu()

    m, _ = _drop_path_model(g, "fp16", "compact", rate)
    m.train()
    eng, l1, s1, g1_ = step(m, 1234)
    f0, f1 = eng.debug_drop_path(0, B).cpu(), eng.debug_drop_path(1, B).cpu()
    dpr = torch.linspace(0, rate, 12)
    for f in (f0, f1):
        assert bool((f[:, 0] == 1).all())
        for l in range(1, 12):
            k = 1.0 - float(dpr[l])
            v = f[:, l]
            assert bool(((v == 0) | ((v - 1.0 / k).abs() < 1e-6)).all()), l
        kept = float((f[:, 1:] > 0).float().mean())
        want = float((1.0 - dpr[1:]).mean())
        sigma = float(((dpr[1:] * (1 - dpr[1:])).sum() * 2 * B).sqrt() / (2 * 11 * B))
        assert abs(kept - want) < 4 * sigma, (kept, want, sigma)
    assert not torch.equal(f0, f1) and not torch.equal(f0[0], f0[1])
    _, l2, s2, g2_ = step(m, 1234)
    assert torch.equal(l1, l2) and torch.equal(s1, s2) and torch.equal(g1_, g2_)
    _, l3, s3, _ = step(m, 99)
    assert not torch.equal(s1, s3)
    # the captured step (hipGraph replay, seed on the device) draws the factors the eager step with the same seed draws
    eng.step_graph(xd, yd, 0.5, 2.0, 0.0, 0.0, seed=1234)
    torch.cuda.synchronize()
    assert torch.equal(eng.grad.cpu(), g1_) and torch.equal(eng.debug_drop_path(0, B).cpu(), f0)
    # evaluation: no stochastic depth; rate 0: the plain model
    m0, _ = _drop_path_model(g, "fp16", "compact", 0.0)
    m.eval(); m0.eval()
    with torch.no_grad():
        a, _ = m(xd[:8])
        b, _ = m0(xd[:8])
    assert torch.equal(a, b)
    m0.train()
    e0, p1, q1, r1 = step(m0, 1234)
    with pytest.raises(Exception):
        e0.debug_drop_path(0, B)   # that pass ran without
    m.drop_path_rate = 0.0
    m.train()
    _, p2, q2, r2 = step(m, 1234)
    assert torch.equal(q1, q2) and torch.equal(r1, r2)


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_drop_path_video_model_vs_oracle(precision):
    """The video model (2 clips x 2 frames: DropPath acts per FRAME there, the trunk sees [(b t), 197, 768],
    video_models/video_vision_transformer_IN21K.py:437) with injected factors against the oracle: logits, masks, losses, all gradients
    (trunk + pooling head), compact mode."""
    import numpy as np
    import gpu_diag as D
    import synth
    from oracle import dyt_oracle as O
    from video_models.video_vision_transformer_IN21K import vit_base_patch16_224_in21k
    clips, frames, C, r, seed, rate = 2, 2, 10, 8, 21, 0.35
    B = clips * frames
    sd = synth.make_state_dict(C, r, seed=seed, kind="test", gate_bias=0.3, video=True)
    tuning = D.Cfg(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option="none", ffn_adapter_init_option="lora",
                   ffn_adapter_scalar="1.0", ffn_num=r, d_model=768)
    model = vit_base_patch16_224_in21k(num_classes=C, drop_path_rate=rate, tuning_config=tuning, select_config=D.Cfg(open=True, keep_layers=0),
                                       precision=precision, train_mode="compact")
    model.load_state_dict(sd, strict=True)
    for n, p in model.named_parameters():
        p.requires_grad = synth.is_trainable(n)
    model = model.cuda()
    x, _ = synth.make_batch(B, C, seed=seed)
    xc = x.reshape(clips, frames, 3, 224, 224).permute(0, 2, 1, 3, 4).contiguous()
    y = torch.tensor([3, 7])
    keep = synth.make_dropout_masks(B, r, seed=seed + 3)
    g1, g2 = synth.make_noise(B, seed=seed + 1)
    gen = torch.Generator().manual_seed(seed + 5)
    scales = torch.stack([O.drop_path_scales(torch.rand(2, 12, B, generator=gen), rate) for _ in range(2)])
    assert int((scales == 0).sum()) >= 8
    model.train()
    model.fold_input(xc)
    eng = model.engine(B, torch.device("cuda", 0))
    sc = [scales[p].cuda().contiguous() for p in range(2)]
    eng.set_drop_path_scales(0, sc[0])
    eng.set_drop_path_scales(1, sc[1])
    ls, lt = torch.empty(clips, C, device="cuda"), torch.empty(clips, C, device="cuda")
    ts = torch.zeros(B, 12, 196, device="cuda")
    losses = eng.step_fwd_bwd(x.cuda(), y.cuda(), 0.5, 2.0, 0.0, 0.0, g1=g1.cuda().contiguous(), g2=g2.cuda().contiguous(),
                              keep_mask=keep.cuda().contiguous(), logits_s=ls, logits_t=lt, token_select=ts).cpu()
    d, gref, outs = O.step_grads(sd, x, y, g1, g2, keep, scale=1.0, mode="compact", frames=frames, drop_scales=scales)
    es, et = float((ls.cpu() - outs[0]).abs().max()), float((lt.cpu() - outs[1]).abs().max())
    flips = int((ts.cpu() != outs[2]["token_select"][..., 0]).sum())
    worst, wn = 0.0, ""
    for n, gr in gref.items():
        got = eng.trainable_view(n, tuple(sd[n].shape), eng.grad).cpu()
        e = float((got - gr).norm() / max(float(gr.norm()), 1e-4 if precision == "fp32" else 3e-4))
        if gr.numel() > 1 and e > worst:
            worst, wn = e, n
    print("drop_path video %s: logits %.2e / %.2e, %d decisions differ, loss %.1e, worst gradient %.1e (%s)" %
          (precision, es, et, flips, abs(float(losses[0]) - float(d["loss"])), worst, wn))
    tol = D.TOL[precision]
    assert es <= tol["vlogits"] and et <= tol["vlogits"] and flips <= tol["vstep_flips"]
    assert abs(float(losses[0]) - float(d["loss"])) <= tol["vloss"] * max(1.0, abs(float(d["loss"])))
    assert worst <= (2e-3 if precision == "fp32" else 0.20), (wn, worst)


# ---- tuning_config.ffn_adapter_scalar = "learnable_scalar" (DYT_OPT_LEARNABLE_SCALE; reference models/dynamic_adapter.py:101-102,138) ----
@pytest.mark.parametrize("precision", ["fp32", "fp16x3q", "fp16", "bf16"])
def test_learnable_scalar_step_vs_reference_golden(precision):
    """The reference model with a trainable adapter scale per block, stepped through its own train_one_epoch
    (tests/golden/learnable_scalar_step.npz, twelve distinct scales): logits, masks, losses and all 86 gradients -- the twelve d(scale)
    included -- of the fused step, masked mode against the reference's values and compact mode against the oracle's; fp32 also the
    parameters after one AdamW update (the scales are ordinary words of the flat buffer)."""
    import os
    import numpy as np
    import gpu_diag as D
    import synth
    from oracle import dyt_oracle as O
    from models.vision_transformer_IN21K import vit_base_patch16_224_in21k
    g = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "learnable_scalar_step.npz")))
    B, C, r, seed = int(g["meta_batch"]), int(g["meta_num_classes"]), int(g["meta_ffn_num"]), int(g["meta_seed"])
    x, y = synth.make_batch(B, C, seed=seed)
    keep = synth.make_dropout_masks(B, r, seed=seed + 3)
    g1, g2 = torch.from_numpy(g["g1"]), torch.from_numpy(g["g2"])
    sd = synth.add_learnable_scales(synth.make_state_dict(C, r, seed=seed, kind="test", gate_bias=0.3), seed=seed)
    tuning = D.Cfg(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option="none", ffn_adapter_init_option="lora",
                   ffn_adapter_scalar="learnable_scalar", ffn_num=r, d_model=768)
    tol = D.TOL[precision]
    for mode in ("masked", "compact"):
        model = vit_base_patch16_224_in21k(num_classes=C, drop_path_rate=0.0, tuning_config=tuning, select_config=D.Cfg(open=True, keep_layers=0),
                                           precision=precision, train_mode=mode)
        msg = model.load_state_dict(sd, strict=True)
        for n, p in model.named_parameters():
            p.requires_grad = synth.is_trainable(n)
        model = model.cuda()
        assert sum(p.requires_grad for p in model.parameters()) == 86
        model.train()
        eng = model.engine(B, torch.device("cuda", 0))
        assert eng.learnable_scale
        ls, lt = torch.empty(B, C, device="cuda"), torch.empty(B, C, device="cuda")
        ts = torch.zeros(B, 12, 196, device="cuda")
        losses = eng.step_fwd_bwd(x.cuda(), y.cuda(), 0.5, 2.0, 0.0, 0.0, masked_dense=(mode == "masked"), g1=g1.cuda().contiguous(),
                                  g2=g2.cuda().contiguous(), keep_mask=keep.cuda().contiguous(), logits_s=ls, logits_t=lt, token_select=ts).cpu()
        es = float(np.abs(ls.cpu().numpy() - g["logits_student"]).max())
        et = float(np.abs(lt.cpu().numpy() - g["logits_teacher"]).max())
        flips = int((ts.cpu().numpy().astype(np.uint8) != g["token_select"][..., 0]).sum())
        el = max(abs(float(losses[i]) - float(g["stat_" + k])) / max(1.0, abs(float(g["stat_" + k])))
                 for i, k in enumerate(("loss", "base_loss", "token_loss", "teacher_loss", "distillation_loss")))
        if mode == "masked":
            gref = {n[len("grad/"):]: torch.from_numpy(v) for n, v in g.items() if n.startswith("grad/")}
        else:
            _, gref, _ = O.step_grads(sd, x, y, g1, g2, keep, scale=float("nan"), mode="compact")
        items = [(n, eng.trainable_view(n, gr.shape, eng.grad).cpu(), gr) for n, gr in gref.items()]
        sc = [it for it in items if it[0].endswith("adaptmlp.scale")]
        assert len(sc) == 12
        gs_got, gs_ref = torch.stack([a.reshape(()) for _, a, _ in sc]), torch.stack([b.reshape(()) for _, _, b in sc])
        e_scale = float((gs_got - gs_ref).norm() / gs_ref.norm())
        items = [it for it in items if not it[0].endswith("adaptmlp.scale")]
        if precision != "fp32":
            sc1 = [it for it in items if it[2].numel() == 1]
            items = [it for it in items if it[2].numel() > 1]
            if sc1:
                items.append(("mlp_token_select.mlp_head.bias (12 blocks)", torch.stack([a.reshape(()) for _, a, _ in sc1]), torch.stack([b.reshape(()) for _, _, b in sc1])))
        worst = {}
        for n, got, ref in items:
            e = float((got - ref).norm() / max(float(ref.norm()), 1e-20))
            k = D.grad_kind(n) if precision in ("fp16", "bf16") else "all"
            if e > worst.get(k, (0.0, ""))[0]:
                worst[k] = (e, n)
        print("learnable_scalar %s/%s: logits %.2e / %.2e, %d decisions differ, losses %.1e, d(scale) x12 %.1e, gradients %s" %
              (precision, mode, es, et, flips, el, e_scale, {k: "%.1e" % v[0] for k, v in worst.items()}))
        assert es <= tol["logits"] and et <= tol["logits"] and flips <= tol["step_flips"] and el <= tol["loss"]
        assert e_scale <= (2e-3 if precision == "fp32" else (tol["grad"] if precision in D.SPLIT_MODES else (0.02 if precision == "fp16" else 0.10)))
        for k, (e, n) in worst.items():
            bound = 2e-3 if precision == "fp32" else (tol["grad"] if precision in D.SPLIT_MODES else
                                                     (D.FP16_GRAD_TOL_SMALL_B if precision == "fp16" else D.BF16_GRAD_TOL_SMALL_B)[k])
            assert e <= bound, (mode, k, n, e, bound)
        if precision == "fp32" and mode == "masked":
            D.D_adamw(eng, float(g["meta_lr"]), float(g["meta_wd"]))
            for key in g:
                if key.startswith("param_after/"):
                    n = key.split("/", 1)[1]
                    got = eng.trainable_view(n, g[key].shape).cpu().numpy()
                    assert np.abs(got - g[key]).max() < 2e-5, n
        del model, eng
        torch.cuda.empty_cache()


def test_learnable_scalar_gradient_accumulation_and_default_layout():
    """The up-projection / scale gradients go through a scratch buffer and a chain-rule kernel; with accumulate=True they must ADD to what
    the gradient buffer holds (micro-batches), exactly like every other tensor.  And the scale lives in a padding word of the flat layout:
    a model with a fixed scalar has the same number of trainable words and never touches that word."""
    import gpu_diag as D
    import synth
    from models.vision_transformer_IN21K import vit_base_patch16_224_in21k
    B, C, r, seed = 3, 10, 8, 13

    def build(scalar):
        tuning = D.Cfg(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option="none", ffn_adapter_init_option="lora",
                       ffn_adapter_scalar=scalar, ffn_num=r, d_model=768)
        m = vit_base_patch16_224_in21k(num_classes=C, drop_path_rate=0.0, tuning_config=tuning, select_config=D.Cfg(open=True, keep_layers=0),
                                       precision="fp32", train_mode="compact")
        sd = synth.make_state_dict(C, r, seed=seed, kind="test", gate_bias=0.3)
        if scalar == "learnable_scalar":
            synth.add_learnable_scales(sd, seed=seed)
        m.load_state_dict(sd, strict=True)
        for n, p in m.named_parameters():
            p.requires_grad = synth.is_trainable(n)
        return m.cuda().train()

    m = build("learnable_scalar")
    eng = m.engine(B, torch.device("cuda", 0))
    batches = []
    for i in range(2):
        x, y = synth.make_batch(B, C, seed=seed + i)
        g1, g2 = synth.make_noise(B, seed=seed + 10 + i)
        batches.append((x.cuda(), y.cuda(), g1.cuda().contiguous(), g2.cuda().contiguous(), synth.make_dropout_masks(B, r, seed=seed + 20 + i).cuda().contiguous()))
    single = []
    for x, y, g1, g2, km in batches:
        eng.step_fwd_bwd(x, y, 0.5, 2.0, 0.0, 0.0, g1=g1, g2=g2, keep_mask=km)
        single.append(eng.grad.clone())
    x, y, g1, g2, km = batches[0]
    eng.step_fwd_bwd(x, y, 0.5, 2.0, 0.0, 0.0, g1=g1, g2=g2, keep_mask=km)
    x, y, g1, g2, km = batches[1]
    eng.step_fwd_bwd(x, y, 0.5, 2.0, 0.0, 0.0, g1=g1, g2=g2, keep_mask=km, accumulate=True)
    want = single[0] + single[1]
    assert float((eng.grad - want).abs().max()) <= 1e-6 * float(want.abs().max())
    off, num = eng.trainable_slice("blocks.5.adaptmlp.scale")
    assert num == 1 and float(single[0][off].abs()) > 0
    m0 = build("0.7")
    e0 = m0.engine(B, torch.device("cuda", 0))
    assert e0.n_train == eng.n_train and not e0.learnable_scale
    x, y, g1, g2, km = batches[0]
    e0.step_fwd_bwd(x, y, 0.5, 2.0, 0.0, 0.0, g1=g1, g2=g2, keep_mask=km)
    assert float(e0.grad[off]) == 0.0 and float(e0.flat[off]) == 0.0


def test_learnable_scalar_through_the_mirror_training_loop():
    """engine_finetune.train_one_epoch + FusedAdamW on a learnable-scalar model (fp32 mode): the loop's freeze-rule check accepts the 86
    trainable tensors, the returned statistics are the reference's, and the twelve scales (and block 6's adapter) after the AdamW step
    are the reference's parameters after its own step."""
    import os
    import types
    import numpy as np
    import gpu_diag as D
    import synth
    from engine_finetune import FusedAdamW, train_one_epoch
    from models.losses import AdaLoss
    from models.vision_transformer_IN21K import vit_base_patch16_224_in21k
    g = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "learnable_scalar_step.npz")))
    B, C, r, seed = int(g["meta_batch"]), int(g["meta_num_classes"]), int(g["meta_ffn_num"]), int(g["meta_seed"])
    sd = synth.add_learnable_scales(synth.make_state_dict(C, r, seed=seed, kind="test", gate_bias=0.3), seed=seed)
    tuning = D.Cfg(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option="none", ffn_adapter_init_option="lora",
                   ffn_adapter_scalar="learnable_scalar", ffn_num=r, d_model=768)
    model = vit_base_patch16_224_in21k(num_classes=C, drop_path_rate=0.0, tuning_config=tuning, select_config=D.Cfg(open=True, keep_layers=0),
                                       precision="fp32", train_mode="masked")
    model.load_state_dict(sd, strict=True)
    for n, p in model.named_parameters():
        p.requires_grad = synth.is_trainable(n)
    model = model.cuda()
    lr, wd = float(g["meta_lr"]), float(g["meta_wd"])
    opt = FusedAdamW(model, lr=lr, weight_decay=wd)
    crit = AdaLoss(torch.nn.CrossEntropyLoss(), token_target_ratio=0.5, token_loss_ratio=2.0, token_minimal=0.0, token_minimal_weight=0.0)
    args = types.SimpleNamespace(accum_iter=1, lr=lr, min_lr=0.0, warmup_epochs=0, epochs=10, metric="accuracy", nb_classes=C)
    x, y = synth.make_batch(B, C, seed=seed)
    keep = synth.make_dropout_masks(B, r, seed=seed + 3)
    loader = [(x, y, (torch.from_numpy(g["g1"]), torch.from_numpy(g["g2"])), keep)]
    stats = train_one_epoch(model, crit, loader, opt, torch.device("cuda", 0), 0, None, 0, None, None, args=args)
    for k in ("loss", "base_loss", "token_loss", "teacher_loss", "distillation_loss"):
        ref = float(g["stat_" + k])
        assert abs(stats[k] - ref) < 1e-4 * max(1.0, abs(ref)), (k, stats[k], ref)
    params = dict(model.named_parameters())
    n_checked = 0
    for key in g:
        if key.startswith("param_after/"):
            n = key.split("/", 1)[1]
            assert np.abs(params[n].detach().cpu().numpy() - g[key]).max() < 5e-5, n
            n_checked += 1
    assert n_checked >= 16
    # and a checkpoint of it carries the scales under the reference's key names
    assert all(("blocks.%d.adaptmlp.scale" % i) in model.state_dict() for i in range(12))
