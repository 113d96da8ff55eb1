"""GPU parity tests proper (pytest -m gpu): the HIP path, called through the C ABI, against
(i) golden vectors captured from the reference, (ii) the CPU oracle on the same seeded inputs,
(iii) size-independent properties at BASELINE.json's full size (B=128)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gpu_diag as D  # noqa: E402  (tests/gpu_diag.py: the individual checks)
import synth  # noqa: E402


def _run(fn):
    del D.RESULTS[:]
    fn()
    bad = [n for n, ok in D.RESULTS if not ok]
    assert D.RESULTS and not bad, bad


def test_layernorm_kernel():
    _run(D.t_layernorm)


def test_linear_kernels_fp32_and_bf16():
    _run(D.t_linear)


def test_linear_row_ranges_across_tile_dispatch():
    _run(D.t_linear_row_ranges)


def test_attention_fwd_bwd_kernels():
    _run(D.t_attention)


def test_gate_and_compaction_kernel():
    _run(D.t_gate)


def test_eval_forward_vs_reference_golden():
    """logits within 1e-3 (fp32 mode), masks bit-exact, vs engine_finetune.evaluate's run of the reference."""
    _run(D.t_eval_golden)


def test_finetune_step_vs_reference_golden():
    """fused step: logits, masks, 5 loss components, 74 trainable grads (masked mode vs the reference's
    own train_one_epoch; compact mode vs the oracle), AdamW update; both arithmetic modes."""
    _run(D.t_step_golden)


def test_video_model_vs_reference_golden():
    """video model (frames folded into the batch + attentive pooling head, 88 trainable tensors): eval forward
    and fused step vs the reference's video_vision_transformer_IN21K / train_video_one_epoch; both modes."""
    _run(D.t_video_golden)


def test_video_full_clip_length_vs_oracle():
    """train_video.sh geometry (8 frames -> 1576 keys per clip, 400 classes), 2 clips: eval logits of the HIP path
    (fp32 mode) vs the oracle; clip order is a pure permutation of the logits rows (clips never mix)."""
    from oracle import dyt_oracle as O
    clips, frames, C, r = 2, 8, 400, 64
    g = {"meta_num_classes": C, "meta_ffn_num": r, "meta_seed": 21, "meta_gate_bias": 0.6, "meta_scale": 0.1}
    model, sd = D.build_video_model(g, "fp32")
    model.eval()
    x, _ = synth.make_batch(clips * frames, C, seed=21)
    xc = x.reshape(clips, frames, 3, 224, 224).permute(0, 2, 1, 3, 4).contiguous()
    with torch.no_grad():
        got, aux = model(xc.cuda())
        swapped, _ = model(xc.flip(0).contiguous().cuda())
        ref, tok = O.forward(sd, x, scale=0.1, training=False, frames=frames)
    assert got.shape == (clips, C)
    assert float((got.cpu() - ref).abs().max()) < 1e-3
    flips = int((aux["token_select"].cpu() != tok["token_select"]).sum())
    assert flips <= 2, flips          # decisions within fp32 round-off of the threshold may differ
    assert torch.equal(swapped.flip(0), got)


def test_video_module_api_autograd_bridge():
    _run(D.t_video_autograd_api)


def test_module_api_autograd_bridge():
    _run(D.t_autograd_api)


def test_vtab_shape_two_steps(golden_dir):
    """r=8, scale 1, wd 1e-4, AdaLoss minimal-token term on, two AdamW steps (main_vtab.py shape)."""
    g = dict(np.load(os.path.join(golden_dir, "step_r8.npz")))
    B, C, r, seed = int(g["meta_batch"]), int(g["meta_num_classes"]), int(g["meta_ffn_num"]), int(g["meta_seed"])
    model, sd = D.build_model(g, "fp32", "masked")
    model.train()
    eng = model.engine(B, torch.device("cuda", 0))
    for s in range(2):
        x, y = synth.make_batch(B, C, seed=seed + 10 * s)
        keep = synth.make_dropout_masks(B, r, seed=seed + 3 + 10 * s).cuda().contiguous()
        g1 = torch.from_numpy(g["s%d_g1" % s]).cuda().contiguous()
        g2 = torch.from_numpy(g["s%d_g2" % s]).cuda().contiguous()
        losses = eng.step_fwd_bwd(x.cuda(), y.cuda(), float(g["meta_target_ratio"]), 2.0, float(g["meta_token_minimal"]),
                                  float(g["meta_token_minimal_weight"]), masked_dense=True, g1=g1, g2=g2, keep_mask=keep).cpu()
        for i, k in enumerate(("loss", "base_loss", "token_loss", "teacher_loss", "distillation_loss")):
            ref = float(g["s%d_stat_%s" % (s, k)])
            assert abs(float(losses[i]) - ref) < 1e-4 * max(1.0, abs(ref)), (s, k, float(losses[i]), ref)
        D.D_adamw(eng, float(g["meta_lr"]), float(g["meta_wd"]))
        for key in g:
            if key.startswith("s%d_param_after/" % s):
                n = key.split("/", 1)[1]
                got = eng.trainable_view(n, g[key].shape).cpu().numpy()
                big = np.abs(g["s%d_grad/%s" % (s, n)]) > 1e-6
                assert np.abs(got - g[key])[big].max(initial=0.0) < 5e-5, (s, n)


def _bench_model(precision, mode, B, gate_bias):
    from models.vision_transformer_IN21K import vit_base_patch16_224_in21k
    sd = synth.make_state_dict(100, 64, seed=0, kind="bench", gate_bias=gate_bias)
    tuning = D.Cfg(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option="none", ffn_adapter_init_option="lora",
                   ffn_adapter_scalar="0.1", ffn_num=64, d_model=768)
    m = vit_base_patch16_224_in21k(num_classes=100, drop_path_rate=0.0, tuning_config=tuning,
                                   select_config=D.Cfg(open=True, keep_layers=0), precision=precision, train_mode=mode, max_batch=B)
    m.load_state_dict(sd)
    return m.cuda()


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_full_size_properties(precision):
    """B=128 (BASELINE configs[1]): compacted and mask-multiplied student passes agree; with every token
    kept the student pass equals the complete_model pass; with every patch token dropped it still runs."""
    B = 128 if precision == "bf16" else 32
    x, y = synth.make_batch(B, 100, seed=5)
    x = x.cuda()
    tol = 2e-2 if precision == "bf16" else 1e-4
    m = _bench_model(precision, "compact", B, 0.85)
    m.eval()
    with torch.no_grad():
        lc, ac = m(x)
        lt, _ = m(x, complete_model=True)
        keep = float(ac["token_select"].mean())
        assert 0.3 < keep < 0.95, keep
        assert float((lc - lt).abs().max()) > 1e-4      # dropping tokens does change the logits ...
        # eval-mode masked-dense forward through the engine (same values as the compacted forward)
        lm, ts_m, _ = m._engine.forward(x, slot=0, training=False, masked_dense=True)
        # fp32: the two forms compute the same values bit for bit.  16-bit modes: the compacted inference pass adds the adapter's
        # up-projection inside the fc2 contraction (DYT_OPT_FC2_CAT), the mask-multiplied pass in a launch of its own -> fp32
        # round-off differences in x_out, i.e. a handful of tie-level decisions out of 128 x 2352
        flips = int((ts_m != ac["token_select"][..., 0]).sum())
        print("compact vs masked-dense eval forward, %s: %d of %d decisions differ" % (precision, flips, ts_m.numel()))
        assert flips <= (0 if precision == "fp32" else 150), flips
        assert float((lm - lc).abs().max()) < tol, float((lm - lc).abs().max())
        for blk in m.blocks:                               # ... keep everything: student == teacher
            blk.mlp_token_select.mlp_head.bias.fill_(100.0)
        la, aa = m(x)
        assert float(aa["token_select"].min()) == 1.0
        assert float((la - lt).abs().max()) < tol
        for blk in m.blocks:                               # drop every patch token: only cls goes through the MLP
            blk.mlp_token_select.mlp_head.bias.fill_(-100.0)
        ld, ad = m(x)
        assert float(ad["token_select"].max()) == 0.0 and torch.isfinite(ld).all()


def test_batch_of_one_and_regrow():
    m = _bench_model("fp32", "compact", 1, 0.5)
    m.eval()
    x, _ = synth.make_batch(3, 100, seed=9)
    with torch.no_grad():
        l1, _ = m(x[:1].cuda())
        l3, _ = m(x.cuda())          # engine is re-created for the larger batch, weights re-uploaded
    assert float((l1 - l3[:1]).abs().max()) < 1e-4


def test_training_rng_stream_statistics():
    """On-device Philox noise: keep ratio responds to the gate bias like E[sigmoid(l + b)], dropout keeps ~90 %."""
    m = _bench_model("bf16", "compact", 16, 0.0)
    m.train()
    x, _ = synth.make_batch(16, 100, seed=11)
    with torch.no_grad():
        _, a0 = m(x.cuda())
        _, a1 = m(x.cuda())
    k0, k1 = float(a0["token_select"].mean()), float(a1["token_select"].mean())
    assert 0.35 < k0 < 0.65 and 0.35 < k1 < 0.65
    assert not torch.equal(a0["token_select"], a1["token_select"])   # fresh noise each call


def test_token_select_module_standalone():
    from models.dynamic_adapter import TokenSelect
    ts = TokenSelect(768, 1).cuda().eval()
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 197, 768, generator=g)
    with torch.no_grad():
        ts.mlp_head.weight.copy_(torch.randn(1, 768, generator=g) * 0.05)
        ts.mlp_head.bias.fill_(0.1)
        sel, logits = ts(x.cuda())
    ref = x[:, 1:] @ ts.mlp_head.weight.cpu().t() + 0.1
    assert float((logits.cpu() - ref).abs().max()) < 1e-5
    assert torch.equal(sel.cpu()[:, 1:], (ref.sigmoid() > 0.5).float())
    assert torch.equal(ts.last_keep_index.cpu().long(), sel.cpu().reshape(-1).nonzero()[:, 0])


def test_gemm_variants_full_occupancy_bitwise():
    """Regression for an LDS-DMA race that only shows when every CU is busy: the 256x256 pipelined GEMM, the
    pre-shuffled-weight GEMM (variant 70: weight fragments straight from global memory, hand-counted vmcnt waits)
    and the 128x128 GEMM accumulate in the same k order, so their bf16 outputs must be BITWISE equal
    on every row at the bench's full size, run after run; all must match an fp32 reference."""
    from _lib import check, lib, ptr, stream_ptr
    for (M, N, K) in [(25216, 2304, 768), (17690, 3072, 768), (25216, 768, 3072)]:
        g = torch.Generator(device="cuda").manual_seed(M + N)
        a = torch.randn(M, K, device="cuda", generator=g).bfloat16()
        w = (torch.randn(N, K, device="cuda", generator=g) * 0.05).bfloat16()
        outs = []
        for variant in (0, 10, 10, 10, 70, 70, 70, 30):
            c = torch.zeros(2 * M, N, device="cuda", dtype=torch.bfloat16)
            check(lib().dyt_gemm_bf16_raw(ptr(a), ptr(w), ptr(c), M, N, K, variant, stream_ptr()))
            torch.cuda.synchronize()
            outs.append(c[:M].clone())
        for o in outs[1:]:
            assert torch.equal(o, outs[0]), (M, N, K, int((o != outs[0]).sum()))
        ref = a.float() @ w.float().t()
        assert float((outs[0].float() - ref).abs().max() / ref.abs().max()) < 1e-2


def test_product_dispatch_route_boundaries_bitwise():
    """The product dispatch (variant 30: csrc/gemm_route.h) at the thresholds of its routing -- M = 2047 / 2048 (128x128 tiles below, 256x256
    above), 16128 / 16129 rows of N = 768 (189 / 192 tiles of 256x256: below / at 3/4 of a round of the 256 CUs) and 21761 rows (a 256x256 body
    of whole rounds + a one-row 128x128 tail).  Every kernel accumulates in the same k order, so the bf16 output must be BITWISE that of
    128x128 tiles everywhere (variant 0); both must match an fp32 reference."""
    from _lib import check, lib, ptr, stream_ptr
    for (M, N, K) in [(2047, 2304, 768), (2048, 2304, 768), (2048, 768, 768), (16128, 768, 3072), (16129, 768, 3072), (21761, 768, 3072)]:
        g = torch.Generator(device="cuda").manual_seed(M + N)
        a = torch.randn(M, K, device="cuda", generator=g).bfloat16()
        w = (torch.randn(N, K, device="cuda", generator=g) * 0.05).bfloat16()
        outs = []
        for variant in (0, 30):
            c = torch.zeros(M, N, device="cuda", dtype=torch.bfloat16)
            check(lib().dyt_gemm_bf16_raw(ptr(a), ptr(w), ptr(c), M, N, K, variant, stream_ptr()))
            torch.cuda.synchronize()
            outs.append(c)
        assert torch.equal(outs[1], outs[0]), (M, N, K, int((outs[1] != outs[0]).sum()))
        ref = a.float() @ w.float().t()
        assert float((outs[0].float() - ref).abs().max() / ref.abs().max()) < 1e-2, (M, N, K)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_scheduling_options_do_not_change_results(precision):
    """Stream overlap (1: the two passes on two HIP streams, 2: plus per-block adapter-branch streams), the cls-only tail
    of the last block and the shared block-0 attention branch are pure scheduling / dead- or duplicate-work elimination: losses, logits, masks and all 74 gradients must equal the plain serial, all-rows schedule."""
    import _lib
    B = 6
    x, y = synth.make_batch(B, 100, seed=21)
    g1, g2 = synth.make_noise(B, seed=22)
    keep = synth.make_dropout_masks(B, 64, seed=23)
    res = []
    for overlap, tail, share in ((0, 0, 0), (1, 0, 0), (2, 0, 0), (4, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
        m = _bench_model(precision, "compact", B, 0.85)
        m.train()
        eng = m.engine(B, torch.device("cuda", 0))
        eng.set_option(_lib.OPT_STREAM_OVERLAP, overlap)
        eng.set_option(_lib.OPT_CLS_TAIL, tail)
        eng.set_option(_lib.OPT_SHARE_BLOCK0, share)
        ls = torch.empty(B, 100, device="cuda")
        ts = torch.zeros(B, 12, 196, device="cuda")
        losses = eng.step_fwd_bwd(x.cuda(), y.cuda(), 0.5, 2.0, 0.0, 0.0, g1=g1.cuda().contiguous(), g2=g2.cuda().contiguous(),
                                  keep_mask=keep.cuda().contiguous(), logits_s=ls, token_select=ts).clone()
        torch.cuda.synchronize()
        res.append((losses.cpu(), ls.cpu(), ts.cpu(), eng.grad.clone().cpu()))
        del m, eng
    tol = 1e-5 if precision == "fp32" else 2e-3
    base = res[0]
    for r in res[1:]:
        assert torch.equal(r[2], base[2])                                   # masks
        assert float((r[1] - base[1]).abs().max()) < tol                    # logits
        assert float((r[0][:5] - base[0][:5]).abs().max()) < tol * 10       # losses
        assert float((r[3] - base[3]).norm() / base[3].norm()) < tol * 10   # flat gradient


@pytest.mark.parametrize("overlap", [0, 4, 1])
def test_reproducible_schedules_are_bitwise(overlap):
    """Every schedule gives the same bits on every run: DYT_OPT_STREAM_OVERLAP 0 (one stream), 4 (forward passes overlapped,
    backward passes one after the other) and 1 (the default, the one bench.py measures: both passes overlap end to end).
    Until round 3 the default schedule differed run to run at the 1e-6 level: ln_bwd consumed its per-row
    (mean, rstd) pair under a partial `s_waitcnt vmcnt(N)` and, with the other pass's weight-gradient workgroups on the same
    CU, occasionally before the load had landed; every row kernel now completes its load group with one full, pinned drain.
    B=16 (pre-shuffled-weight GEMMs included), fast mode, two steps each, contexts rebuilt."""
    import _lib
    B = 16
    x, y = synth.make_batch(B, 100, seed=21)
    runs = []
    for _ in range(3):
        m = _bench_model("bf16", "compact", B, 0.85)
        m.train()
        eng = m.engine(B, torch.device("cuda", 0))
        eng.set_option(_lib.OPT_STREAM_OVERLAP, overlap)
        out = []
        for i in range(2):
            losses = eng.step_fwd_bwd(x.cuda(), y.cuda(), 0.5, 2.0, 0.0, 0.0, seed=900 + i).clone()
            torch.cuda.synchronize()
            out.append((losses.cpu(), eng.grad.clone().cpu()))
        runs.append(out)
        del m, eng
    for r in runs[1:]:
        for i in range(2):
            assert torch.equal(r[i][0], runs[0][i][0])          # losses: forward only
            assert float(r[i][1].abs().max()) > 0
            assert torch.equal(r[i][1], runs[0][i][1])


@pytest.mark.parametrize("mode,precision", [("compact", "bf16"), ("masked", "bf16"), ("compact", "fp16"), ("compact", "fp16x3q"), ("compact", "fp16f8")])
def test_default_schedule_is_bitwise_at_bench_size(mode, precision):
    """The benchmarked configuration itself: B=128, bf16, both passes overlapped end to end (DYT_OPT_STREAM_OVERLAP = 1).
    11 rebuilt contexts x 2 steps = 20 comparisons against the first run, gradients bit for bit (round 2: every one of them
    differed, ~2e-6 absolute in ~1.09 M of the 1.28 M gradient elements)."""
    import _lib
    B = 128
    x, y = synth.make_batch(B, 100, seed=23)
    x, y = x.cuda(), y.cuda()
    ref = None
    for run in range(11 if precision in ("bf16", "fp16") else 5):   # (the split modes: 4 x 2 comparisons, their contexts are 38 GB each)
        m = _bench_model(precision, mode, B, 0.85)
        m.train()
        eng = m.engine(B, torch.device("cuda", 0))
        eng.set_option(_lib.OPT_STREAM_OVERLAP, 1)
        out = []
        for i in range(2):
            losses = eng.step_fwd_bwd(x, y, 0.5, 2.0, 0.0, 0.0, masked_dense=(mode == "masked"), seed=700 + i).clone()
            torch.cuda.synchronize()
            out.append((losses.clone(), eng.grad.clone()))
        del m, eng
        torch.cuda.empty_cache()
        if ref is None:
            ref = out
            assert float(ref[0][1].abs().max()) > 0
            continue
        for i in range(2):
            assert torch.equal(out[i][0], ref[i][0]), (run, i)
            assert torch.equal(out[i][1], ref[i][1]), (run, i, float((out[i][1] - ref[i][1]).abs().max()))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("M", [4, 788, 25216])
def test_adapter_weight_gradient_kernel(precision, M):
    """models/dynamic_adapter.py:117-134 backward, the products with the token dimension as contraction: dW[c][j] = sum_m
    X[m][c] Y[m][j] plus both column sums (the bias gradients), against fp64 torch; M = cls tail of B=4, B=4, B=128."""
    import _lib
    from _lib import check, lib, ptr
    L = lib()
    P = 0 if precision == "fp32" else 1
    gen = torch.Generator(device="cuda").manual_seed(M)
    X = torch.randn(M, 768, device="cuda", generator=gen) * 1e-2
    Y = torch.randn(M, 64, device="cuda", generator=gen)
    Y[:, 40:] = 0.0                                         # rank 40 of the 64-wide tile
    if P:
        X, Y = X.bfloat16(), Y.bfloat16()
    part = torch.zeros(int(L.dyt_wgrad_scratch_floats(M)), device="cuda")
    w = torch.full((768 * 40,), 0.5, device="cuda")         # the kernel accumulates into its outputs
    xs = torch.zeros(768, device="cuda")
    ys = torch.zeros(40, device="cuda")
    check(L.dyt_wgrad_raw(ptr(X), ptr(Y), M, 40, P, ptr(part), ptr(w), ptr(xs), ptr(ys), _lib.stream_ptr()))
    torch.cuda.synchronize()
    ref = X.double().t() @ Y.double()[:, :40]
    tol = 2e-6
    assert float((w.view(768, 40).double() - 0.5 - ref).abs().max() / ref.abs().max()) < tol
    assert float((xs.double() - X.double().sum(0)).abs().max() / X.double().sum(0).abs().max()) < tol
    assert float((ys.double() - Y.double()[:, :40].sum(0)).abs().max() / Y.double()[:, :40].sum(0).abs().max()) < tol


def test_c_abi_error_paths():
    """Misuse is reported through the status code + dyt_last_error (DyTError in the mirror), never a crash."""
    from _lib import DyTError
    from runtime import DyTEngine
    dev = torch.device("cuda", 0)
    eng = DyTEngine(10, 8, 0.1, dev, precision="fp32", max_batch=2)
    x = torch.zeros(3, 3, 224, 224, device=dev)
    with pytest.raises(DyTError, match="max_batch"):
        eng.forward(x)                                            # batch 3 > max_batch 2
    g = torch.zeros(eng.n_train, device=dev)
    with pytest.raises(DyTError, match="saved forward"):
        eng.backward(0, torch.zeros(2, 10, device=dev), g)        # no forward with DYT_F_SAVE before
    with pytest.raises(DyTError, match="g1 and g2"):
        eng.forward(x[:2], training=True, g1=torch.zeros(12, 2, 196, device=dev))
    with pytest.raises(DyTError):
        DyTEngine(10, 65, 0.1, dev)                               # adapter rank > 64
    with pytest.raises(DyTError, match="multiple of frames"):
        DyTEngine(10, 8, 0.1, dev, max_batch=6, frames=4)         # video: max_batch must hold whole clips
    veng = DyTEngine(10, 8, 0.1, dev, precision="fp32", max_batch=4, frames=2)
    with pytest.raises(DyTError, match="multiple of frames"):
        veng.forward(x)                                           # 3 frames with 2 frames per clip
    with pytest.raises(DyTError, match="video model only"):
        eng.trainable_slice("query_token")


def test_full_size_backward_is_linear_and_batch_equivariant():
    """B=128, bf16, compact mode (the bench configuration).  (i) Doubling the upstream gradient doubles every trainable
    gradient BIT FOR BIT (the backward pass is linear and a factor 2 commutes with every rounding).  (ii) Reversing the
    image order reverses logits and masks bit for bit (no kernel mixes rows of different images; the compacted row
    order changes, the values must not)."""
    B = 128
    m = _bench_model("bf16", "compact", B, 0.85)
    m.train()
    x, _ = synth.make_batch(B, 100, seed=17)
    x = x.cuda()
    eng = m.engine(B, x.device)
    g1, g2 = synth.make_noise(B, seed=4, passes=1)
    g1, g2 = g1[0].cuda().contiguous(), g2[0].cuda().contiguous()
    logits, ts, _ = eng.forward(x, slot=0, training=True, save=True, g1=g1, g2=g2, seed=5)
    dl = torch.randn(B, 100, device="cuda") * 0.01
    ga, gb = torch.zeros_like(eng.flat), torch.zeros_like(eng.flat)
    eng.backward(0, dl, ga)
    eng.backward(0, (2.0 * dl).contiguous(), gb)
    assert float(ga.abs().max()) > 0
    assert torch.equal(2.0 * ga, gb)
    # image order: same dropout stream is keyed by token row, so switch the adapter dropout off for this comparison
    m.eval()
    with torch.no_grad():
        la, aa = m(x)
        lb, ab = m(x.flip(0).contiguous())
    assert torch.equal(lb.flip(0), la)
    assert torch.equal(ab["token_select"].flip(0), aa["token_select"])


def test_gradient_accumulation_flag():
    """DYT_F_ACCUM_GRAD (engine_finetune.py:43-46,66-76 accum_iter): two micro-batches accumulated == sum of their gradients."""
    g = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "step_r8.npz")))
    model, sd = D.build_model(g, "fp32", "masked")
    model.train()
    B, C = 3, int(g["meta_num_classes"])
    eng = model.engine(B, torch.device("cuda", 0))
    grads = []
    batches = [synth.make_batch(B, C, seed=40 + i) for i in range(2)]
    for i, (x, y) in enumerate(batches):
        eng.step_fwd_bwd(x.cuda(), y.cuda(), seed=100 + i)
        grads.append(eng.grad.clone())
    for i, (x, y) in enumerate(batches):
        eng.step_fwd_bwd(x.cuda(), y.cuda(), seed=100 + i, accumulate=(i > 0))
    ref = grads[0] + grads[1]
    assert float(ref.abs().max()) > 0
    assert float((eng.grad - ref).abs().max()) <= 1e-6 * float(ref.abs().max())
