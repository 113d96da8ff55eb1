"""GPU tests of the byte-image input (pytest -m gpu): uint8 batches, channels-first or channels-last, normalised where the patch
embedding loads them (DYT_F_IMAGES_U8 / DYT_F_IMAGES_NHWC, dyt_set_input_norm) and by dyt_normalize_u8.

The byte path is defined as the float path on the normalised image -- ``(u.float().div(255) - mean) / std`` computed by torch on the CPU
(tests/input_u8_refs.py) -- so EVERY comparison here is ``torch.equal``: no tolerance exists.  The test images hold all 256 byte values
in every channel, so a formula that differs from the reference's in any entry of the 3 x 256 value table shows in the fp32 cases.
Models and their library contexts are built once per module (r = 8, C = 10, B <= 5)."""
import ctypes
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

import gpu_diag as D  # noqa: E402
import input_u8_refs as R  # noqa: E402
import synth  # noqa: E402

C, RANK, SEED, BMAX = 10, 8, 53, 5
DEV = torch.device("cuda", 0)


def _tuning():
    return D.Cfg(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option="none", ffn_adapter_init_option="lora",
                 ffn_adapter_scalar="0.1", ffn_num=RANK, d_model=768)


def _model(precision, sd, kind="image", **kw):
    if kind == "video":
        from video_models.video_vision_transformer_IN21K import vit_base_patch16_224_in21k
    elif kind == "twin":
        from models.model_speed_test import vit_base_patch16_224_in21k
    else:
        from models.vision_transformer_IN21K import vit_base_patch16_224_in21k
    m = vit_base_patch16_224_in21k(num_classes=C, drop_path_rate=0.0, tuning_config=_tuning(), select_config=D.Cfg(open=True, keep_layers=0),
                                   precision=precision, train_mode="compact", max_batch=BMAX, **kw)
    m.load_state_dict(sd)
    for n, p in m.named_parameters():
        p.requires_grad = synth.is_trainable(n)
    return m.cuda().eval()


def _eval(m, x):
    with torch.no_grad():
        logits, aux = m(x)
    return logits, aux["token_select"], aux["token_logits"]


def _same(a, b, what):
    for name, ta, tb in zip(("logits", "token_select", "token_logits"), a, b):
        assert ta.shape == tb.shape and torch.equal(ta, tb), "%s: %s differs (max |d| = %.3e)" % (what, name, float((ta - tb).abs().max()))


@pytest.fixture(scope="module")
def data():
    """The byte batch (B = 5; the tests take slices), its channels-last twin, and the CPU-normalised float images per statistics: computed
    once, read only."""
    u = R.byte_images(BMAX, seed=SEED)
    return types.SimpleNamespace(u=u, nhwc=R.to_nhwc(u), x={name: R.normalize_cpu(u, name) for name in R.STATS},
                                 y=synth.make_batch(BMAX, C, seed=SEED)[1])


@pytest.fixture(scope="module")
def sd():
    return synth.make_state_dict(C, RANK, seed=SEED, kind="test", gate_bias=0.85)


@pytest.fixture(scope="module")
def models(sd):
    """precision -> image model built with input_norm='imagenet' (float inputs are untouched by the setting: the same model and context
    run both sides of a comparison), on first use."""
    cache = {}

    def get(precision):
        if precision not in cache:
            cache[precision] = _model(precision, sd, input_norm="imagenet")
        return cache[precision]
    yield get
    cache.clear()
    torch.cuda.empty_cache()


# ---- 1. dyt_normalize_u8 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stats", ["imagenet", "inception"])
def test_normalize_u8_equals_the_cpu_formula(stats, data):
    from _lib import normalize_u8
    mean, std = R.STATS[stats]
    want = data.x[stats][:3]
    for name, src in (("nchw", data.u[:3]), ("nhwc", data.nhwc[:3])):
        got = normalize_u8(src.cuda(), mean, std)
        torch.cuda.synchronize()
        assert got.dtype == torch.float32 and tuple(got.shape) == (3, 3, 224, 224)
        bad = int((got.cpu() != want).sum())
        assert bad == 0, "%s %s: %d of %d values differ from (u / 255 - mean) / std" % (stats, name, bad, want.numel())


# ---- 2. eval forward ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16", "fp16x3q"])
def test_eval_forward_on_bytes_equals_the_float_path(precision, models, data):
    """B = 3 and B = 1, both byte layouts, against the same context fed the CPU-normalised image.  fp32 is the case that catches a wrong
    formula: there the embedding GEMM's operand IS the normalised value."""
    from _lib import F_IMAGES_NHWC, F_IMAGES_U8
    m = models(precision)
    for lo, hi in ((0, 3), (3, 4)):
        want = _eval(m, data.x["imagenet"][lo:hi].cuda())
        assert want[0].shape == (hi - lo, C) and bool(torch.isfinite(want[0]).all())
        _same(_eval(m, data.u[lo:hi].cuda()), want, "%s B=%d nchw bytes" % (precision, hi - lo))
        _same(_eval(m, data.nhwc[lo:hi].cuda()), want, "%s B=%d nhwc bytes" % (precision, hi - lo))
    eng = m._engine
    assert eng._image_flags(data.u[:1].cuda()) == F_IMAGES_U8 and eng._image_flags(data.nhwc[:1].cuda()) == F_IMAGES_U8 | F_IMAGES_NHWC
    assert eng._image_flags(data.x["imagenet"][:1].cuda()) == 0 and eng.input_norm == R.STATS["imagenet"]
    # not the raw 0..255 values
    assert not torch.equal(_eval(m, data.u[:3].cuda().float())[0], _eval(m, data.u[:3].cuda())[0])
    if precision == "fp32":   # forward_features takes the same path (DYT_F_TOKENS_OUT)
        fa, aa = m.forward_features(data.nhwc[:3].cuda())
        fb, ab = m.forward_features(data.x["imagenet"][:3].cuda())
        assert torch.equal(fa, fb) and torch.equal(aa["token_logits"], ab["token_logits"])


def test_set_input_norm_changes_the_statistics_of_later_passes(models, data):
    m = models("fp32")
    eng = m.engine(3, DEV)
    try:
        eng.set_input_norm(*R.STATS["inception"])
        got = eng.forward(data.nhwc[:3].cuda(), gate_always=True)
        want = eng.forward(data.x["inception"][:3].cuda(), gate_always=True)
        _same(got, want, "inception statistics")
        assert not torch.equal(got[0], eng.forward(data.x["imagenet"][:3].cuda(), gate_always=True)[0])
    finally:
        eng.set_input_norm(*R.STATS["imagenet"])
    _same(eng.forward(data.u[:3].cuda(), gate_always=True), eng.forward(data.x["imagenet"][:3].cuda(), gate_always=True), "back to imagenet")


# ---- 3. the fused step ---------------------------------------------------------------------------------------------------------------------
def _step(eng, x, y, g1, g2, keep, seed=11):
    ls, lt = (torch.zeros(x.shape[0], C, device=DEV) for _ in range(2))
    losses = torch.zeros(8, device=DEV)
    eng.step_fwd_bwd(x, y, 0.5, 2.0, 0.1, 1.0, g1=g1, g2=g2, keep_mask=keep, seed=seed, logits_s=ls, logits_t=lt, losses=losses)
    torch.cuda.synchronize()
    return losses.clone(), ls, lt, eng.grad.clone()


def _graph_step(eng, x, y, seed=11):
    losses = torch.zeros(8, device=DEV)
    eng.step_graph(x, y, 0.5, 2.0, 0.1, 1.0, losses=losses, seed=seed)
    torch.cuda.synchronize()
    return losses.clone(), eng.grad.clone()


def _equal_all(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and torch.equal(a, b), "%s: output %d differs (max |d| = %.3e)" % (what, i, float((a - b).abs().max()))


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_step_on_bytes_equals_the_float_step(precision, models, data):
    """B = 4, injected Gumbel draws and keep mask: the 8 loss outputs, both logits and the whole flat gradient.  Both passes read the
    bytes: with block 0 shared (the default) and with the teacher's own embedding (DYT_OPT_SHARE_BLOCK0 = 0)."""
    from _lib import OPT_SHARE_BLOCK0
    B = 4
    eng = models(precision).engine(B, DEV)
    y = data.y[:B].cuda()
    g1, g2 = (t.cuda().contiguous() for t in synth.make_noise(B, seed=SEED + 1))
    keep = synth.make_dropout_masks(B, RANK, seed=SEED + 2).cuda().contiguous()
    xn = data.x["imagenet"][:B].cuda()
    want = _step(eng, xn, y, g1, g2, keep)
    assert bool(torch.isfinite(want[0]).all()) and float(want[3].abs().max()) > 0
    _equal_all(_step(eng, data.u[:B].cuda(), y, g1, g2, keep), want, "%s nchw bytes" % precision)
    _equal_all(_step(eng, data.nhwc[:B].cuda(), y, g1, g2, keep), want, "%s nhwc bytes" % precision)
    eng.set_option(OPT_SHARE_BLOCK0, 0)
    try:
        own = _step(eng, xn, y, g1, g2, keep)
        _equal_all(_step(eng, data.nhwc[:B].cuda(), y, g1, g2, keep), own, "%s nhwc bytes, teacher's own embedding" % precision)
    finally:
        eng.set_option(OPT_SHARE_BLOCK0, 1)


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_step_graph_is_keyed_by_dtype_layout_and_norm(precision, models, data):
    """The captured step on bytes equals the captured step on the normalised floats; a float batch and a byte batch of ONE shape
    ([4,3,224,224]) do not share a graph or a static input buffer, in either order; a byte step captured under other statistics is
    another graph."""
    B = 4
    eng = models(precision).engine(B, DEV)
    y = data.y[:B].cuda()
    xn, u, nhwc = data.x["imagenet"][:B].cuda(), data.u[:B].cuda(), data.nhwc[:B].cuda()
    other = synth.make_batch(B, C, seed=SEED + 7)[0].cuda()   # a float batch that is NOT the normalised bytes
    eng._graphs = {}
    a = _graph_step(eng, xn, y)
    _equal_all(_graph_step(eng, u, y), a, "graph, nchw bytes")
    c = _graph_step(eng, other, y)
    assert not torch.equal(c[1], a[1])
    _equal_all(_graph_step(eng, u, y), a, "graph, nchw bytes after a float step of the same shape")
    _equal_all(_graph_step(eng, other, y), c, "graph, float step after a byte step of the same shape")
    _equal_all(_graph_step(eng, nhwc, y), a, "graph, nhwc bytes")
    assert len(eng._graphs) == 3
    assert sorted(str(k[1]) for k in eng._graphs) == ["torch.float32", "torch.uint8", "torch.uint8"]
    try:
        eng.set_input_norm(*R.STATS["inception"])
        want = _graph_step(eng, data.x["inception"][:B].cuda(), y)
        _equal_all(_graph_step(eng, u, y), want, "graph, bytes under the inception statistics")
        assert len(eng._graphs) == 4 and not torch.equal(want[1], a[1])
    finally:
        eng.set_input_norm(*R.STATS["imagenet"])
    _equal_all(_graph_step(eng, u, y), a, "graph, bytes back under the imagenet statistics")
    assert len(eng._graphs) == 4
    eng._graphs = {}


# ---- 4. the training loop ---------------------------------------------------------------------------------------------------------------
def test_device_prefetcher_keeps_byte_batches_as_bytes(data):
    """The loop's input feeding: uint8 batches of both layouts and a float batch in turn through the prefetcher's device buffers arrive
    with their dtype, shape and values.  (The copy stream is the current stream here: what is under test is the buffer handling.)"""
    from engine_finetune import DevicePrefetcher
    cur = torch.cuda.current_stream(DEV)
    loader = [(data.u[:2], data.y[:2]), (data.nhwc[:2], data.y[:2]), (data.x["imagenet"][:2], data.y[:2]), (data.u[2:4], data.y[2:4]),
              (data.nhwc[1:4], data.y[1:4])]
    pf = DevicePrefetcher(loader, DEV, pick_stream=lambda samples, targets: cur)
    n = 0
    for it, xs, ys, rest in pf:
        want = loader[it][0]
        assert xs.is_cuda and xs.dtype == want.dtype and xs.shape == want.shape and xs.is_contiguous()
        assert torch.equal(xs.cpu(), want) and torch.equal(ys.cpu(), loader[it][1])
        n += 1
    assert n == len(loader) and pf.copy_stream is cur
    assert pf.copied_bytes == sum(x.numel() * x.element_size() + y.numel() * 8 for x, y in loader)


def test_train_one_epoch_on_a_byte_loader_equals_the_float_loader(sd, data, monkeypatch):
    """3 iterations of B = 4: a loader that yields uint8 (NCHW, NHWC, NCHW; model with input_norm) against one that yields the
    CPU-normalised floats (model without).  Then one more epoch of the same with a deterministic mixup_fn (fixed lambda), which sees
    the fp32 images dyt_normalize_u8 makes of the bytes.  The copies stay on the compute stream (DYT_PREFETCH=0): the measured pick of a
    copy stream is the business of tests/test_gpu_round6.py, and both loops here must place their copies alike."""
    from engine_finetune import FusedAdamW, train_one_epoch
    from models.losses import AdaLoss
    monkeypatch.setenv("DYT_PREFETCH", "0")
    B, lr = 4, 1e-3
    args = types.SimpleNamespace(accum_iter=1, lr=lr, min_lr=0.0, warmup_epochs=0, epochs=10, metric="accuracy", nb_classes=C)
    crit = AdaLoss(torch.nn.CrossEntropyLoss(), token_target_ratio=0.5, token_loss_ratio=2.0, token_minimal=0.1, token_minimal_weight=1.0)
    order = [(0, 4), (1, 5), (0, 4)]
    extra = [(synth.make_noise(B, seed=SEED + 20 + i), synth.make_dropout_masks(B, RANK, seed=SEED + 30 + i)) for i in range(3)]
    byte_loader = [((data.nhwc if i == 1 else data.u)[lo:hi].contiguous(), data.y[lo:hi], extra[i][0], extra[i][1]) for i, (lo, hi) in enumerate(order)]
    float_loader = [(data.x["imagenet"][lo:hi].contiguous(), data.y[lo:hi], extra[i][0], extra[i][1]) for i, (lo, hi) in enumerate(order)]
    mb, mf = _model("fp16", sd, input_norm="imagenet"), _model("fp16", sd)
    assert mb.input_norm is not None and mf.input_norm is None
    ob, of = FusedAdamW(mb, lr=lr, weight_decay=0.01), FusedAdamW(mf, lr=lr, weight_decay=0.01)
    for epoch, mixup in ((0, None), (1, lambda x, t: synth.mixup_batch(x, t, C))):
        sb = train_one_epoch(mb, crit, byte_loader, ob, DEV, epoch, None, 0, mixup, None, args=args)
        sf = train_one_epoch(mf, crit, float_loader, of, DEV, epoch, None, 0, mixup, None, args=args)
        torch.cuda.synchronize()
        assert sb == sf, (epoch, sb, sf)
        assert torch.equal(mb._engine.flat, mf._engine.flat), "epoch %d: trainable parameters differ (max |d| = %.3e)" % (
            epoch, float((mb._engine.flat - mf._engine.flat).abs().max()))
        for (n, p), (_, q) in zip(mb.named_parameters(), mf.named_parameters()):
            if p.requires_grad:
                assert torch.equal(p, q), n
    moved = max(float((p.detach().cpu() - sd[n]).abs().max()) for n, p in mb.named_parameters() if p.requires_grad)
    assert moved > 0   # the loop did train
    del mb, mf


# ---- 5. video -------------------------------------------------------------------------------------------------------------------------------
def test_video_clips_as_bytes_equal_float_clips(data):
    """Clips [2,3,2,224,224] and [2,2,224,224,3] as bytes against the float clips: fold_input folds on the bytes."""
    clips, frames = 2, 2
    vsd = synth.make_state_dict(C, RANK, seed=SEED, kind="test", gate_bias=0.85, video=True)
    u = data.u[:clips * frames]
    first = u.reshape(clips, frames, 3, 224, 224).permute(0, 2, 1, 3, 4).contiguous()     # [b,3,t,224,224]
    last = data.nhwc[:clips * frames].reshape(clips, frames, 224, 224, 3).contiguous()    # [b,t,224,224,3]
    xf = data.x["inception"][:clips * frames].reshape(clips, frames, 3, 224, 224).permute(0, 2, 1, 3, 4).contiguous()
    for precision in ("fp32", "fp16"):
        m = _model(precision, vsd, kind="video", input_norm="inception")
        want = _eval(m, xf.cuda())
        assert want[0].shape == (clips, C)
        _same(_eval(m, first.cuda()), want, "video %s [b,3,t,h,w] bytes" % precision)
        _same(_eval(m, last.cuda()), want, "video %s [b,t,h,w,3] bytes" % precision)
        assert m._engine.frames == frames and m._engine.input_norm == R.STATS["inception"]
        del m


# ---- 6. inference-only contexts and the speed twin --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["inference_only", "twin"])
def test_inference_only_and_speed_twin_take_bytes(kind, sd, data):
    m = _model("fp16", sd, kind="twin", input_norm="imagenet") if kind == "twin" else _model("fp16", sd, inference_only=True, input_norm="imagenet")
    with torch.no_grad():
        out = [m(t[:3].cuda()) for t in (data.x["imagenet"], data.u, data.nhwc)]
    logits = [o if kind == "twin" else o[0] for o in out]
    assert logits[0].shape == (3, C)
    assert torch.equal(logits[1], logits[0]) and torch.equal(logits[2], logits[0])
    if kind == "inference_only":
        assert m._engine.inference
    del m


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refused_combinations_enqueue_nothing_and_leave_the_context_usable(models, data):
    from _lib import DyTError, F_GATE_ALWAYS, F_IMAGES_NHWC, F_IMAGES_U8, F_TOKENS_IN, F_TOKENS_OUT, float3, ptr, stream_ptr
    m = models("fp16")
    B = 3
    eng = m.engine(B, DEV)
    L = eng.L
    u, xn = data.u[:B].cuda(), data.x["imagenet"][:B].cuda()
    want = eng.forward(xn, gate_always=True)
    torch.cuda.synchronize()
    pad = torch.zeros(u.numel() + 64, dtype=torch.uint8, device=DEV)
    pad[4:4 + u.numel()] = u.reshape(-1)
    misaligned = ctypes.c_void_p(pad.data_ptr() + 4)
    tokens = torch.zeros(B, 197, 768, device=DEV)
    logits = torch.full((B, C), 7.0, device=DEV)
    big = torch.full((B, 197, 768), 7.0, device=DEV)

    def fwd(images, flags, out):
        return L.dyt_forward(eng.h, 0, images, B, flags, ptr(eng.flat), None, None, None, ctypes.c_uint64(0), ptr(out), None, None, stream_ptr())

    cases = {
        "NHWC without U8": (ptr(xn), F_IMAGES_NHWC, logits),
        "U8 with TOKENS_IN": (ptr(tokens), F_IMAGES_U8 | F_TOKENS_IN | F_TOKENS_OUT | F_GATE_ALWAYS, big),
        "NHWC with TOKENS_IN": (ptr(tokens), F_IMAGES_NHWC | F_TOKENS_IN | F_TOKENS_OUT | F_GATE_ALWAYS, big),
        "misaligned bytes": (misaligned, F_IMAGES_U8, logits),
        "misaligned nhwc bytes": (misaligned, F_IMAGES_U8 | F_IMAGES_NHWC, logits),
    }
    for what, (images, flags, out) in cases.items():
        rc = fwd(images, flags, out)
        assert rc == -1 and L.dyt_last_error(), what
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), "%s: something was enqueued" % what
    # the fused step refuses the same way, before it touches the gradient buffer
    eng.grad.fill_(7.0)
    y = data.y[:B].cuda()
    for what, (images, flags) in {"step, misaligned": (misaligned, F_IMAGES_U8), "step, NHWC without U8": (ptr(xn), F_IMAGES_NHWC)}.items():
        rc = L.dyt_step_fwd_bwd(eng.h, images, ptr(y), B, flags, ptr(eng.flat), None, None, None, ctypes.c_uint64(0), 0.5, 2.0, 0.0, 0.0,
                                ptr(eng.grad), ptr(eng.losses), None, None, None, stream_ptr())
        assert rc == -1 and L.dyt_last_error(), what
        torch.cuda.synchronize()
        assert bool((eng.grad == 7.0).all()), "%s: something was enqueued" % what
    eng.grad.zero_()
    # statistics
    for mean, std in (((0.5, 0.5, 0.5), (0.5, 0.0, 0.5)), ((0.5, 0.5, 0.5), (0.5, 0.5, -1.0)), ((0.5, 0.5, 0.5), (float("inf"), 0.5, 0.5)),
                      ((0.5, 0.5, 0.5), (0.5, float("nan"), 0.5)), ((float("nan"), 0.5, 0.5), (0.5, 0.5, 0.5)), ((0.5, float("-inf"), 0.5), (0.5, 0.5, 0.5))):
        with pytest.raises(DyTError):
            eng.set_input_norm(mean, std)
        assert L.dyt_normalize_u8(ptr(u), ptr(big), B, 0, float3(mean), float3(std), stream_ptr()) == -1
    assert L.dyt_normalize_u8(misaligned, ptr(big), B, 0, float3((0.5,) * 3), float3((0.5,) * 3), stream_ptr()) == -1
    torch.cuda.synchronize()
    assert bool((big == 7.0).all()) and eng.input_norm == R.STATS["imagenet"]
    with pytest.raises(DyTError):   # a uint8 tensor that is not an image batch
        eng.forward(torch.zeros(B, 3, 32, 32, dtype=torch.uint8, device=DEV))
    # the context is as it was: the refused statistics were not taken, a valid byte forward gives the float path's result
    _same(eng.forward(u, gate_always=True), want, "after the refusals")
    _same(eng.forward(data.nhwc[:B].cuda(), gate_always=True), want, "after the refusals, nhwc")


# ---- 8. the guard on existing behaviour ---------------------------------------------------------------------------------------------------------------
def test_model_without_input_norm_uses_uint8_as_raw_values(sd, data):
    """Passes before and after the feature: a model built without input_norm converts a uint8 batch with .float()."""
    m = _model("fp16", sd)
    assert getattr(m, "input_norm", None) is None
    u = data.u[:3].cuda()
    got, want = _eval(m, u), _eval(m, u.float())
    _same(got, want, "uint8 without input_norm")
    del m
