"""GPU tests of the on-device Mixup / CutMix (pytest -m gpu): dyt_mix_images, dyt_mix_targets, and dyt_set_mix -- the mix fused into the
patch-embedding load of the forward pass and the fused step, driven by util.mixup.DeviceMixup through train_one_epoch.

The fused path is defined as the float path on the mixed image (tests/mix_refs.py: torch's ``lam * x + (1.0 - lam) * x.flip(0)``, a box copied
from ``x.flip(0)``, or the image itself) with synth.mixup_batch's class-probability targets, so every comparison but two is exact and is
made on the raw bits (``_same_bits``); the two with a tolerance are the fp64 check of the targets (4 x 2^-24 absolute: three roundings of
values in [0, 1]) and the reference golden (the bounds of tests/test_gpu_round6.py::test_mixup_step_vs_reference_golden, read from
gpu_diag).  B <= 4, r = 8, C = 10 unless stated; models are built once per module where a test does not train them."""
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gpu_diag as D  # noqa: E402
import input_u8_refs as U  # noqa: E402
import mix_refs as R  # noqa: E402
import synth  # noqa: E402

C, RANK, SEED, BMAX, SMOOTH = 10, 8, 71, 4, 0.1
DEV = torch.device("cuda", 0)
NORM = U.STATS["imagenet"]


def _draws():
    from util.mixup import MixDraw
    beta = float(np.random.default_rng(SEED).beta(0.8, 0.8))
    d = {"identity": MixDraw.identity(), "mixup_0.7": MixDraw.mixup(0.7), "mixup_beta": MixDraw.mixup(beta)}
    d.update({"cutmix_" + k: MixDraw.cutmix(box) for k, box in R.BOXES.items()})
    return {k: v.with_targets(SMOOTH, C) for k, v in d.items()}


DRAWS = _draws()


def _same_bits(got, want, what):
    got, want = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, (what, got.shape, want.shape, got.dtype)
    if not torch.equal(got.view(torch.int32), want.view(torch.int32)):
        bad = got.view(torch.int32) != want.view(torch.int32)
        raise AssertionError("%s: %d of %d values differ in their bits (max |d| = %.3e)" % (
            what, int(bad.sum()), bad.numel(), float((got - want)[bad].abs().nan_to_num(float("inf")).max())))


def _tuning():
    return D.Cfg(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option="none", ffn_adapter_init_option="lora",
                 ffn_adapter_scalar="0.1", ffn_num=RANK, d_model=768)


def _model(precision, sd, mode="compact", kind="image", classes=C, **kw):
    if kind == "video":
        from video_models.video_vision_transformer_IN21K import vit_base_patch16_224_in21k
    else:
        from models.vision_transformer_IN21K import vit_base_patch16_224_in21k
    m = vit_base_patch16_224_in21k(num_classes=classes, drop_path_rate=0.0, tuning_config=_tuning(), select_config=D.Cfg(open=True, keep_layers=0),
                                   precision=precision, train_mode=mode, max_batch=BMAX, **kw)
    m.load_state_dict(sd)
    for n, p in m.named_parameters():
        p.requires_grad = synth.is_trainable(n)
    return m.cuda()


@pytest.fixture(scope="module")
def data():
    """Byte batch (B = 4), its channels-last twin, the CPU-normalised floats, an unrelated float batch and labels with an equal pair
    (rows 1 and 2 pair up and share a label): computed once, read only."""
    u = U.byte_images(BMAX, seed=SEED)
    return types.SimpleNamespace(u=u, nhwc=U.to_nhwc(u), xn=U.normalize_cpu(u, "imagenet"), xf=synth.make_batch(BMAX, C, seed=SEED)[0],
                                 y=torch.tensor([3, 7, 7, 0], dtype=torch.int64))


@pytest.fixture(scope="module")
def sd():
    return synth.make_state_dict(C, RANK, seed=SEED, kind="test", gate_bias=0.85)


@pytest.fixture(scope="module")
def models(sd):
    cache = {}

    def get(precision):
        if precision not in cache:
            cache[precision] = _model(precision, sd, input_norm="imagenet").eval()
        return cache[precision]
    yield get
    cache.clear()
    torch.cuda.empty_cache()


def _params(draw, criterion_smoothing=0.0):
    return torch.frombuffer(bytearray(draw.words(criterion_smoothing)), dtype=torch.int32).to(DEV)


# ---- 1. dyt_mix_images -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DRAWS))
def test_mix_images_equals_the_torch_reference(name, data):
    """fp32 / uint8 NCHW / uint8 NHWC, 2 and 4 images, and 2 clips of 2 frames, against mix_refs on the CPU."""
    from _lib import mix_images
    d, p = DRAWS[name], _params(DRAWS[name])
    for n, frames in ((2, 1), (4, 1), (4, 2)):
        what = "%s n=%d frames=%d" % (name, n, frames)
        _same_bits(mix_images(data.xf[:n].cuda(), p, frames=frames), R.mix_images(data.xf[:n], d, frames), what + " fp32")
        want = R.mix_images(data.xn[:n], d, frames)
        _same_bits(mix_images(data.u[:n].cuda(), p, frames=frames, norm=NORM), want, what + " u8 nchw")
        _same_bits(mix_images(data.nhwc[:n].cuda(), p, frames=frames, norm=NORM), want, what + " u8 nhwc")
    if d.mode == 2:   # what the box exercises
        yl, yh, xl, xh = d.box
        got = mix_images(data.xf.cuda(), p).cpu()
        inside = torch.zeros(224, 224, dtype=torch.bool)
        inside[yl:yh, xl:xh] = True
        assert int(inside.sum()) == (yh - yl) * (xh - xl)
        assert torch.equal(got[:, :, inside], data.xf.flip(0)[:, :, inside]) and torch.equal(got[:, :, ~inside], data.xf[:, :, ~inside])


def test_identity_copies_the_own_image_and_nothing_of_the_partner(data):
    """-0.0 (and inf) in the own image pass through with their bits; a partner full of NaN leaves no trace."""
    from _lib import mix_images
    x = data.xf[:2].clone()
    x[0, :, ::2, ::3] = -0.0
    x[0, 1, 5, 7] = float("inf")
    x[1] = float("nan")
    got = mix_images(x.cuda(), _params(DRAWS["identity"])).cpu()
    _same_bits(got[0], x[0], "identity, own image")
    assert bool(torch.isnan(got[1]).all()) and not bool(torch.isnan(got[0]).any())
    assert bool((got[0].view(torch.int32)[:, ::2, ::3] == -2 ** 31).all())   # the sign bit of -0.0


# ---- 2. dyt_mix_targets ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classes", [10, 1000])
def test_mix_targets_equal_the_torch_expression(classes, data):
    from _lib import mix_targets
    from util.mixup import MixDraw
    bound = 4 * 2.0 ** -24
    for name, base in (("mixup", MixDraw.mixup(0.7)), ("beta", MixDraw.mixup(DRAWS["mixup_beta"].lam)), ("cutmix", MixDraw.cutmix(R.BOXES["crossing"])),
                       ("identity", MixDraw.identity())):
        d = base.with_targets(SMOOTH, classes)
        for rows in (2, 4):
            y = data.y[:rows] if classes == 10 else data.y[:rows] * 97 + 13
            assert rows < 4 or int(y[1]) == int(y[2])   # a pair with equal labels
            for e in (0.0, 0.2):
                got = mix_targets(y.cuda(), classes, _params(d, e)).cpu()
                _same_bits(got, R.mix_targets(y, classes, d, SMOOTH, e), "%s C=%d rows=%d criterion smoothing %g" % (name, classes, rows, e))
                err = float(np.abs(got.numpy().astype(np.float64) - R.mix_targets_f64(y, classes, d, SMOOTH, e)).max())
                print("mix_targets %s C=%d rows=%d e=%g: max |fp32 - fp64| = %.3e (bound %.3e)" % (name, classes, rows, e, err, bound))
                assert err <= bound
                assert abs(float(got.sum(dim=1).mean()) - 1.0) < 1e-4   # rows stay probability rows
    if classes == 10:   # synth.mixup_batch itself
        d = MixDraw.mixup(0.7).with_targets(SMOOTH, 10)
        _same_bits(mix_targets(data.y.cuda(), 10, _params(d)), synth.mixup_batch(data.xf, data.y, 10, lam=0.7, smoothing=SMOOTH)[1], "synth.mixup_batch")


# ---- 3. forward --------------------------------------------------------------------------------------------------------------------------------
def _eval(m, x):
    with torch.no_grad():
        logits, aux = m(x)
    return logits, aux["token_logits"]


@pytest.mark.parametrize("precision", ["fp32", "fp16", "bf16"])
def test_forward_with_mix_on_equals_the_float_path_on_the_mixed_image(precision, models, data):
    m = models(precision)
    eng = m.engine(BMAX, DEV)
    for name in ("mixup_beta", "cutmix_crossing", "identity"):
        d = DRAWS[name]
        want = _eval(m, R.mix_images(data.xn, d).cuda())
        want_f = _eval(m, R.mix_images(data.xf, d).cuda())
        assert bool(torch.isfinite(want[0]).all())
        eng.set_mix(d)
        try:
            assert eng._mix_on
            for what, x, w in (("nchw bytes", data.u, want), ("nhwc bytes", data.nhwc, want), ("float", data.xf, want_f)):
                got = _eval(m, x.cuda())
                _same_bits(got[0], w[0], "%s %s %s: logits" % (precision, name, what))
                _same_bits(got[1], w[1], "%s %s %s: token logits" % (precision, name, what))
        finally:
            eng.set_mix(None)
        if d.mode != 0:   # and off again: the unmixed image gives other logits
            assert not torch.equal(_eval(m, data.u.cuda())[0], want[0])


# ---- 4. the training loop: fused against today's callable branch ------------------------------------------------------------------------------------
def _epoch_args(lr, graph=False):
    return types.SimpleNamespace(accum_iter=1, lr=lr, min_lr=0.0, warmup_epochs=0, epochs=10, metric="accuracy", nb_classes=C, hip_graph=graph)


def _criterion(e=0.0):
    from models.losses import AdaLoss
    return AdaLoss(torch.nn.CrossEntropyLoss(label_smoothing=e), token_target_ratio=0.5, token_loss_ratio=2.0, token_minimal=0.1, token_minimal_weight=1.0)


def _train(model, loader, mixup_fn, lr=1e-3, graph=False, e=0.0, epoch=0, opt=None):
    from engine_finetune import FusedAdamW, train_one_epoch
    opt = FusedAdamW(model, lr=lr, weight_decay=0.01) if opt is None else opt
    stats = train_one_epoch(model, _criterion(e), loader, opt, DEV, epoch, None, 0, mixup_fn, None, args=_epoch_args(lr, graph))
    torch.cuda.synchronize()
    return stats, model._engine.flat.clone(), opt


@pytest.mark.parametrize("mode,loader_kind", [("masked", "bytes"), ("masked", "float"), ("compact", "bytes"), ("compact", "float")])
def test_two_steps_of_the_fused_path_equal_the_callable_branch(mode, loader_kind, sd, data, monkeypatch):
    """train_one_epoch with a DeviceMixup holding two injected draws (mixup, cutmix) against the same loop with mixup_fn = the mix_refs
    callable on the same draws: epoch statistics and every trainable parameter.  The masked cases add the criterion's own label
    smoothing on top of the mixed rows."""
    from util.mixup import DeviceMixup
    monkeypatch.setenv("DYT_PREFETCH", "0")
    e = 0.1 if mode == "masked" else 0.0
    draws = [DRAWS["mixup_beta"], DRAWS["cutmix_crossing"]]
    extra = [(synth.make_noise(BMAX, seed=SEED + 20 + i), synth.make_dropout_masks(BMAX, RANK, seed=SEED + 30 + i)) for i in range(2)]
    if loader_kind == "bytes":
        loader = [((data.nhwc if i == 1 else data.u), data.y, extra[i][0], extra[i][1]) for i in range(2)]
        kw = dict(input_norm="imagenet")
    else:
        loader = [(data.xf, data.y, extra[i][0], extra[i][1]) for i in range(2)]
        kw = {}
    ma, mb = _model("fp16", sd, mode, **kw), _model("fp16", sd, mode, **kw)
    fused = DeviceMixup(label_smoothing=SMOOTH, num_classes=C).inject(draws)
    sa, fa, _ = _train(ma, loader, fused, e=e)
    assert not ma._engine._mix_on and not fused._injected   # both draws used, mix switched off after the epoch
    sb, fb, _ = _train(mb, loader, R.callable_for(draws, C, SMOOTH), e=e)
    assert sa == sb, (sa, sb)
    _same_bits(fa, fb, "%s %s: trainable parameters" % (mode, loader_kind))
    moved = max(float((p.detach().cpu() - sd[n]).abs().max()) for n, p in ma.named_parameters() if p.requires_grad)
    assert moved > 0 and np.isfinite(sa["loss"])
    del ma, mb


def test_video_clips_through_the_fused_path_equal_the_callable_branch(data, monkeypatch):
    """2 clips of 2 frames, bytes: frame f of clip 0 pairs with frame f of clip 1, targets per clip."""
    from util.mixup import DeviceMixup
    monkeypatch.setenv("DYT_PREFETCH", "0")
    vsd = synth.make_state_dict(C, RANK, seed=SEED, kind="test", gate_bias=0.85, video=True)
    clips = data.u.reshape(2, 2, 3, 224, 224).permute(0, 2, 1, 3, 4).contiguous()   # [b,3,t,224,224] bytes
    y = data.y[:2]
    loader = [(clips, y)]
    draws = [DRAWS["cutmix_crossing"]]
    ma, mb = (_model("fp16", vsd, "compact", kind="video", input_norm="imagenet") for _ in range(2))
    sa, fa, _ = _train(ma, loader, DeviceMixup(label_smoothing=SMOOTH, num_classes=C).inject(draws))
    sb, fb, _ = _train(mb, loader, R.callable_for(draws, C, SMOOTH))
    assert sa == sb, (sa, sb)
    _same_bits(fa, fb, "video: trainable parameters")
    # and the drop-in callable form of the class on the same clips
    mixed, soft = DeviceMixup(label_smoothing=SMOOTH, num_classes=C).inject(draws)(clips.cuda(), y.cuda(), norm=NORM)
    want_x, want_t = R.callable_for(draws, C, SMOOTH)(U.normalize_cpu(data.u, "imagenet").reshape(2, 2, 3, 224, 224).permute(0, 2, 1, 3, 4), y)
    _same_bits(mixed.contiguous(), want_x.contiguous(), "DeviceMixup.__call__ on clips: images")
    _same_bits(soft, want_t, "DeviceMixup.__call__ on clips: targets")
    del ma, mb


# ---- 5. the reference golden ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_fused_mixup_step_vs_reference_golden(precision):
    """tests/golden/mixup_step.npz (the reference's own train_one_epoch with synth.mixup_batch as its mixup_fn) through the FUSED path:
    the unmixed batch and its integer labels go in, mix is on with the golden's lam and smoothing.  Bounds: those of
    tests/test_gpu_round6.py::test_mixup_step_vs_reference_golden (gpu_diag.TOL and the small-batch gradient bounds), masked mode."""
    from util.mixup import DeviceMixup, MixDraw
    from models.vision_transformer_IN21K import vit_base_patch16_224_in21k
    g = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "mixup_step.npz")))
    B, Cg, r, seed = int(g["meta_batch"]), int(g["meta_num_classes"]), int(g["meta_ffn_num"]), int(g["meta_seed"])
    lam, sm = float(g["meta_lam"]), float(g["meta_smoothing"])
    x, y = synth.make_batch(B, Cg, seed=seed)
    keep = synth.make_dropout_masks(B, r, seed=seed + 3)
    g1, g2 = torch.from_numpy(g["g1"]), torch.from_numpy(g["g2"])
    gsd = synth.make_state_dict(Cg, r, seed=seed, kind="test", gate_bias=0.3)
    tol = D.TOL[precision]
    tuning = D.Cfg(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option="none", ffn_adapter_init_option="lora",
                   ffn_adapter_scalar="0.1", ffn_num=r, d_model=768)
    model = vit_base_patch16_224_in21k(num_classes=Cg, drop_path_rate=0.0, tuning_config=tuning, select_config=D.Cfg(open=True, keep_layers=0),
                                       precision=precision, train_mode="masked")
    model.load_state_dict(gsd, strict=True)
    for n, p in model.named_parameters():
        p.requires_grad = synth.is_trainable(n)
    model = model.cuda().train()
    eng = model.engine(B, DEV)
    eng.set_mix(DeviceMixup(label_smoothing=sm, num_classes=Cg).inject([MixDraw.mixup(lam)]).draw())
    ls, lt = torch.empty(B, Cg, device=DEV), torch.empty(B, Cg, device=DEV)
    ts = torch.zeros(B, 12, 196, device=DEV)
    losses = eng.step_fwd_bwd(x.cuda(), y.cuda(), 0.5, 2.0, 0.0, 0.0, masked_dense=True, g1=g1.cuda().contiguous(), g2=g2.cuda().contiguous(),
                              keep_mask=keep.cuda().contiguous(), logits_s=ls, logits_t=lt, token_select=ts).cpu()
    eng.set_mix(None)
    es = float(np.abs(ls.cpu().numpy() - g["logits_student"]).max())
    et = float(np.abs(lt.cpu().numpy() - g["logits_teacher"]).max())
    flips = int((ts.cpu().numpy().astype(np.uint8) != g["token_select"][..., 0]).sum())
    el = max(abs(float(losses[i]) - float(g["stat_" + k])) / max(1.0, abs(float(g["stat_" + k])))
             for i, k in enumerate(("loss", "base_loss", "token_loss", "teacher_loss", "distillation_loss")))
    gref = {n[len("grad/"):]: torch.from_numpy(v) for n, v in g.items() if n.startswith("grad/")}
    items = [(n, eng.trainable_view(n, gr.shape, eng.grad).cpu(), gr) for n, gr in gref.items()]
    if precision != "fp32":
        sc1 = [it for it in items if it[2].numel() == 1]
        items = [it for it in items if it[2].numel() > 1]
        if sc1:
            items.append(("mlp_token_select.mlp_head.bias (12 blocks)", torch.stack([a.reshape(()) for _, a, _ in sc1]), torch.stack([b.reshape(()) for _, _, b in sc1])))
    worst = {}
    for n, got, ref in items:
        err = float((got - ref).norm() / max(float(ref.norm()), 1e-20))
        k = D.grad_kind(n) if precision in ("fp16", "bf16") else "all"
        if err > worst.get(k, (0.0, ""))[0]:
            worst[k] = (err, n)
    print("fused mixup %s: logits %.2e / %.2e, %d decisions differ, losses %.1e, gradients %s" %
          (precision, es, et, flips, el, {k: "%.1e" % v[0] for k, v in worst.items()}))
    assert es <= tol["logits"] and et <= tol["logits"] and flips <= tol["step_flips"] and el <= tol["loss"]
    for k, (err, n) in worst.items():
        bound = 2e-3 if precision == "fp32" else D.FP16_GRAD_TOL_SMALL_B[k]
        assert err <= bound, (k, n, err, bound)
    del model, eng
    torch.cuda.empty_cache()


# ---- 6. hipGraph replay ------------------------------------------------------------------------------------------------------------------------
def test_three_draws_replay_one_captured_graph_and_equal_the_eager_steps(sd, data, monkeypatch):
    """args.hip_graph with a mixup, a cutmix and an identity draw: the three replays read their draw from the engine's device block, so
    ONE captured graph serves them, and they equal the three eager steps bit for bit (per-step losses, statistics, parameters)."""
    import engine_finetune as E
    from util.mixup import DeviceMixup
    monkeypatch.setenv("DYT_PREFETCH", "0")
    draws = [DRAWS["mixup_beta"], DRAWS["cutmix_aligned"], DRAWS["identity"]]
    loader = [(data.u, data.y), (data.u.flip(1).contiguous(), data.y.flip(0).contiguous()), (data.u, data.y)]
    out = {}
    real = E.train_step
    for graph in (False, True):
        seq = []

        def spy(*a, **kw):
            r = real(*a, **kw)
            seq.append(kw["losses_out"].clone())
            return r
        monkeypatch.setattr(E, "train_step", spy)
        m = _model("fp16", sd, "compact", input_norm="imagenet")
        stats, flat, _ = _train(m, loader, DeviceMixup(label_smoothing=SMOOTH, num_classes=C).inject(draws), graph=graph)
        monkeypatch.setattr(E, "train_step", real)
        out[graph] = (stats, flat, torch.stack(seq).cpu(), len(m._engine._graphs), [k[-1] for k in m._engine._graphs])
        del m
    assert out[False][3] == 0 and out[True][3] == 1 and out[True][4] == [True]   # one graph for the three draws, keyed "mix on"
    assert out[False][0] == out[True][0], (out[False][0], out[True][0])
    _same_bits(out[True][2], out[False][2], "per-step losses, graph against eager")
    _same_bits(out[True][1], out[False][1], "trainable parameters, graph against eager")
    seq = out[True][2]
    assert len({float(v) for v in seq[:, 0]}) == 3   # three draws, three losses


# ---- 7. state and refusals ------------------------------------------------------------------------------------------------------------------------
def test_the_epoch_after_a_mixed_one_trains_unmixed_on_integer_labels(sd, data, monkeypatch):
    """A mixed epoch leaves nothing behind: a fused step and evaluate() on the model that mixed equal those of a model that never did
    and holds the same parameters."""
    from engine_finetune import evaluate
    from util.mixup import DeviceMixup
    monkeypatch.setenv("DYT_PREFETCH", "0")
    loader = [(data.u, data.y)]
    a = _model("fp16", sd, "compact", input_norm="imagenet")
    _, _, opt = _train(a, loader, DeviceMixup(label_smoothing=SMOOTH, num_classes=C).inject([DRAWS["mixup_0.7"]]))
    assert not a._engine._mix_on and getattr(a._engine, "_soft_keep", None) is None
    b = _model("fp16", {k: v.detach().cpu().clone() for k, v in a.state_dict().items()}, "compact", input_norm="imagenet")
    g1, g2 = (t.cuda().contiguous() for t in synth.make_noise(BMAX, seed=SEED + 1))
    keep = synth.make_dropout_masks(BMAX, RANK, seed=SEED + 2).cuda().contiguous()

    def step(m):
        eng = m.engine(BMAX, DEV)
        losses = torch.zeros(8, device=DEV)
        eng.step_fwd_bwd(data.u.cuda(), data.y.cuda(), 0.5, 2.0, 0.1, 1.0, g1=g1, g2=g2, keep_mask=keep, seed=5, losses=losses)
        torch.cuda.synchronize()
        return losses.clone(), eng.grad.clone()
    (la, ga), (lb, gb) = step(a), step(b)
    _same_bits(la, lb, "losses of the step after the mixed epoch")
    _same_bits(ga, gb, "gradient of the step after the mixed epoch")
    ea, eb = (evaluate([(data.u, data.y)], m, DEV, args=types.SimpleNamespace(metric="accuracy", nb_classes=C)) for m in (a, b))
    assert ea == eb, (ea, eb)
    # a plain epoch on the model that mixed: integer labels, another loss than the mixed epoch's
    s2, _, _ = _train(a, loader, None, epoch=1, opt=opt)
    assert np.isfinite(s2["loss"]) and not a._engine._mix_on
    del a, b


def test_refusals_come_with_a_text_before_anything_is_enqueued(models, data):
    from _lib import DyTError
    from engine_finetune import FusedAdamW, train_step
    from runtime import DyTEngine
    m = models("fp16")
    eng = m.engine(BMAX, DEV)
    d = DRAWS["mixup_0.7"]
    u3, y3 = data.u[:3].cuda(), data.y[:3].cuda()
    eng.set_mix(d)
    try:
        # an odd batch: the forward and the step refuse, nothing runs
        with pytest.raises(DyTError, match="odd number"):
            eng.forward(u3, gate_always=True)
        eng.grad.fill_(7.0)
        with pytest.raises(DyTError, match="odd number"):
            eng.step_fwd_bwd(u3, y3, 0.5, 2.0, 0.0, 0.0)
        torch.cuda.synchronize()
        assert bool((eng.grad == 7.0).all()), "something was enqueued"
        # mix together with caller-set class-probability targets
        soft = torch.full((BMAX, C), 1.0 / C, device=DEV)
        with pytest.raises(DyTError, match="mix is on"):
            eng.set_soft_targets(soft)
        assert getattr(eng, "_soft_keep", None) is None
    finally:
        eng.set_mix(None)
        eng.grad.zero_()
    eng.set_soft_targets(torch.full((BMAX, C), 1.0 / C, device=DEV))
    try:
        with pytest.raises(DyTError, match="dyt_set_soft_targets"):
            eng.set_mix(d)
        assert not eng._mix_on
    finally:
        eng.set_soft_targets(None)
    # train_step refuses an odd batch and class-probability targets together with mix=
    m.train()
    opt = FusedAdamW(m, lr=1e-3)
    before = eng.flat.clone()
    with pytest.raises(DyTError, match="odd number"):
        train_step(m, u3, y3, opt, target_ratio=0.5, token_minimal=0.0, token_minimal_weight=0.0, mix=d)
    with pytest.raises(DyTError, match="integer labels"):
        train_step(m, data.u.cuda(), torch.full((BMAX, C), 1.0 / C, device=DEV), opt, target_ratio=0.5, token_minimal=0.0, token_minimal_weight=0.0, mix=d)
    torch.cuda.synchronize()
    assert torch.equal(eng.flat, before) and not eng._mix_on
    m.eval()
    # a draw for another number of classes, and an inference-only engine
    with pytest.raises(DyTError, match="classes"):
        eng.set_mix(d.with_targets(SMOOTH, C + 1))
    inf = DyTEngine(C, RANK, 0.1, DEV, precision="fp16", max_batch=2, depth=1, inference=True)
    with pytest.raises(DyTError, match="inference_only"):
        inf.set_mix(d)
    rc = inf.L.dyt_set_mix(inf.h, _params(d).data_ptr(), 1)
    assert rc != 0 and b"inference_only" in inf.L.dyt_last_error()
    # the context is as it was
    _same_bits(eng.forward(data.u.cuda(), gate_always=True)[0], eng.forward(data.xn.cuda(), gate_always=True)[0], "after the refusals")


# ---- 8. wide head ------------------------------------------------------------------------------------------------------------------------------
def test_wide_head_rows_with_a_class_count_that_is_no_multiple_of_four(data):
    """C = 1031 (DYT_CREATE_WIDE_HEAD), B = 2, two blocks: the scalar-store form of mix_targets_kernel and the context's soft-target buffer with
    an odd row stride, against the float path on the mixed image with the reference rows handed in (dyt_set_soft_targets)."""
    from _lib import mix_targets
    from runtime import DyTEngine
    CW, B = 1031, 2
    y = torch.tensor([1030, 517], dtype=torch.int64)
    d = DRAWS["mixup_beta"].with_targets(SMOOTH, CW)
    _same_bits(mix_targets(y.cuda(), CW, _params(d, 0.1)), R.mix_targets(y, CW, d, SMOOTH, 0.1), "C=1031 rows")
    eng = DyTEngine(CW, RANK, 0.1, DEV, precision="fp16", max_batch=B, depth=2, wide_head=True)
    wsd = synth.make_state_dict(CW, RANK, seed=SEED, kind="test", depth=2, gate_bias=0.85)
    eng.load_state_dict(wsd)
    bytes_before = eng.bytes
    g1, g2 = (t.cuda().contiguous() for t in synth.make_noise(B, depth=2, seed=SEED + 1))
    keep = synth.make_dropout_masks(B, RANK, depth=2, seed=SEED + 2).cuda().contiguous()

    def step(x, soft=None):
        losses, ls = torch.zeros(8, device=DEV), torch.zeros(B, CW, device=DEV)
        eng.set_soft_targets(soft)
        eng.step_fwd_bwd(x, y.cuda(), 0.5, 2.0, 0.0, 0.0, g1=g1, g2=g2, keep_mask=keep, losses=losses, logits_s=ls)
        torch.cuda.synchronize()
        eng.set_soft_targets(None)
        return losses.clone(), ls, eng.grad.clone()
    want = step(R.mix_images(data.xn[:B], d).cuda(), R.mix_targets(y, CW, d, SMOOTH, 0.0).cuda())
    eng.set_mix(d)
    assert eng.bytes == bytes_before + B * CW * 4   # the context-owned rows are counted
    got = step(data.u[:B].cuda())
    eng.set_mix(None)
    for i, what in enumerate(("losses", "student logits", "gradient")):
        _same_bits(got[i], want[i], "wide head: " + what)
    assert bool(torch.isfinite(got[0]).all()) and float(got[2].abs().max()) > 0
    del eng
