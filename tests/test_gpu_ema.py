"""Model EMA on the GPU: dyt_ema_update (csrc/ema.hip) on plain fp32 tensors through the C ABI, then util.model_ema.DeviceModelEma inside the
small model of tests/test_gpu_param_groups.py (depth 2, B = 4, 10 classes, rank 8).

The yardstick is exact everywhere.  The kernel's contract is three fp32 roundings per element -- torch's ``decay * e + (1. - decay) * m``, to
which tests/ema_refs.py is pinned on the CPU (tests/test_ema_refs_host.py) -- so kernel and reference are compared BIT FOR BIT (NaN by
position), on the 16-byte path, the scalar path and mixed alignments, with +-0, +-inf, NaN, denormals and near-overflow values planted.
In the model the shadow after every update equals the reference applied to the previous shadow and the parameters of that moment; the
evaluation view equals the model with the shadow copied over its parameters (torch.equal); a resumed run equals the uninterrupted one."""
import copy
import ctypes
import math
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _lib  # noqa: E402
import ema_refs as R  # noqa: E402
import synth  # noqa: E402

DEV = "cuda:0"
ERR_ARG = -1   # DYT_ERR_ARG (include/dyt_hip.h)
CANARY = 77.25
LEAD = 4       # elements in front of the 16-byte aligned base of every test allocation: room for a canary in front of offset 0
OFFSETS = [(0, 0), (1, 1), (1, 2), (0, 3)]   # (ema, param) element offsets: 16-byte path with no head / with a head; mixed: all scalar


def _rc(e, p, n, decay, stream=None):
    d, o = R.scalars(decay)
    return _lib.lib().dyt_ema_update(ctypes.c_void_p(e.data_ptr()) if e is not None else None, ctypes.c_void_p(p.data_ptr()) if p is not None else None,
                                     n, float(d), float(o), _lib.stream_ptr() if stream is None else stream)


def _same(got, want, tag):
    assert R.same_bits(got, want), "%s: first difference (index, gpu, reference, count) %r" % (tag, R.first_difference(got, want))


def _alloc(values, off):
    """A device allocation filled with canaries, ``values`` at element LEAD + off of it (LEAD x 4 bytes keeps torch's alignment of the base
    modulo 16), and the view of that range."""
    n = len(values)
    buf = torch.full((LEAD + off + n + 5,), CANARY, dtype=torch.float32)
    buf[LEAD + off:LEAD + off + n] = torch.from_numpy(values)
    buf = buf.to(DEV)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[LEAD + off:LEAD + off + n]


# ------------------------------------------------------------------------------------------------------------------------------
# 1: kernel bits
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 257, 1023, 70001])
def test_kernel_equals_the_reference_bit_for_bit(n):
    for scale in (1e-3, 1.0, 1e3):
        e0, p0 = R.draws(n, seed=1000 + n, scale=scale)
        for oe, op in OFFSETS:
            pbuf, p = _alloc(p0, op)
            pbuf0 = pbuf.cpu()
            for decay in R.DECAYS:
                tag = "n=%d scale %g offsets (%d, %d) decay %r" % (n, scale, oe, op, decay)
                ebuf, e = _alloc(e0, oe)
                assert (e.data_ptr() % 16, p.data_ptr() % 16) == (4 * oe, 4 * op), tag
                assert _rc(e, p, n, decay) == 0, (tag, _lib.lib().dyt_last_error().decode())
                got = ebuf.cpu().numpy()
                a = LEAD + oe
                _same(got[a:a + n], R.ema_ref(e0, p0, decay), tag)
                assert (got[:a] == CANARY).all() and (got[a + n:] == CANARY).all(), "%s: a canary next to the range was written" % tag
            assert R.same_bits(pbuf.cpu().numpy(), pbuf0.numpy()), "param is read only"


def test_denormals_pass_through_and_the_ends_of_the_decay_range():
    e0 = np.array([1e-42, 1e-45, 3e-39, -2e-40, 1.0, 0.0, -0.0, 1e-38], np.float32)
    p0 = np.array([0.0, 1e-45, 1e-42, 2e-40, 1e-45, 1e-45, -0.0, -1e-38], np.float32)
    for decay in R.DECAYS:
        pbuf, p = _alloc(p0, 0)
        ebuf, e = _alloc(e0, 0)
        assert _rc(e, p, 8, decay) == 0
        got = e.cpu().numpy()
        _same(got, R.ema_ref(e0, p0, decay), "denormals, decay %r" % decay)
    pbuf, p = _alloc(p0, 0)
    ebuf, e = _alloc(e0, 0)
    assert _rc(e, p, 8, 0.5) == 0
    got = e.cpu().numpy()
    assert 0 < got[0] < np.float32(1e-42)   # 0.5 x 1e-42: halved, not flushed
    assert got[1] == 0                      # 0.5 x the smallest denormal is a tie that rounds to even, on both sides: 0 + 0
    assert 0 < got[2] < np.float32(3e-39)   # a sum of two denormals


# ------------------------------------------------------------------------------------------------------------------------------
# 2: chained updates
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decay", R.DECAYS)
def test_200_chained_updates_with_a_fresh_param_each_time(decay):
    n, steps = 257, 200
    e0, _ = R.draws(n, seed=21)
    g = np.random.default_rng(22)
    params = g.standard_normal((steps, n)).astype(np.float32)
    params[7, :9], params[150, 20:29] = R.SPECIALS, R.SPECIALS   # specials arrive mid-chain too (NaN and inf then stay, as in the reference)
    dev = torch.from_numpy(params).to(DEV)
    ebuf, e = _alloc(e0, 1)
    want = e0
    for k in range(steps):
        assert _rc(e, dev[k], n, decay) == 0
        want = R.ema_ref(want, params[k], decay)
        if k % 20 == 19 or k in (7, 8, 150):
            _same(e.cpu().numpy(), want, "decay %r step %d" % (decay, k))
    got = ebuf.cpu().numpy()
    _same(got[LEAD + 1:LEAD + 1 + n], want, "decay %r, end of the chain" % decay)
    assert (got[:LEAD + 1] == CANARY).all() and (got[LEAD + 1 + n:] == CANARY).all()


# ------------------------------------------------------------------------------------------------------------------------------
# 3: refusals
# ------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_anything_is_enqueued():
    n = 300
    e0, p0 = R.draws(n, seed=31, plant=False)
    ebuf, e = _alloc(e0, 0)
    pbuf, p = _alloc(p0, 0)
    L = _lib.lib()
    s = _lib.stream_ptr()
    ev, pv = ctypes.c_void_p(e.data_ptr()), ctypes.c_void_p(p.data_ptr())
    nan, inf = float("nan"), float("inf")
    cases = [("null ema", None, pv, n, 0.5, 0.5), ("null param", ev, None, n, 0.5, 0.5), ("numel < 0", ev, pv, -1, 0.5, 0.5),
             ("decay < 0", ev, pv, n, -1e-6, 1.0), ("decay > 1", ev, pv, n, 1.0001, 0.0), ("decay NaN", ev, pv, n, nan, 0.5),
             ("decay inf", ev, pv, n, inf, 0.5), ("decay -inf", ev, pv, n, -inf, 0.5), ("1 - decay < 0", ev, pv, n, 1.0, -1e-6),
             ("1 - decay > 1", ev, pv, n, 0.0, 1.0001), ("1 - decay NaN", ev, pv, n, 0.5, nan), ("1 - decay inf", ev, pv, n, 0.5, inf)]
    for what, a, b, cnt, d, o in cases:
        assert L.dyt_ema_update(a, b, cnt, d, o, s) == ERR_ARG, what
        assert "dyt_ema_update" in L.dyt_last_error().decode(), what
    torch.cuda.synchronize()
    assert R.same_bits(e.cpu().numpy(), e0) and R.same_bits(p.cpu().numpy(), p0)
    assert L.dyt_ema_update(ev, pv, 0, 0.5, 0.5, s) == 0 and L.dyt_ema_update(None, None, 0, 0.5, 0.5, s) == 0   # numel == 0: a successful no-op
    torch.cuda.synchronize()
    assert R.same_bits(ebuf.cpu().numpy()[LEAD:LEAD + n], e0)
    assert _rc(e, p, n, 0.9) == 0   # and the entry still works
    _same(e.cpu().numpy(), R.ema_ref(e0, p0, 0.9), "after the refusals")


def test_engine_refuses_a_wrong_shadow_and_an_inference_only_engine():
    from _lib import DyTError
    from runtime import DyTEngine
    eng = DyTEngine(C, RANK, 0.1, DEV, precision="fp32", max_batch=1, depth=1)
    flat0 = eng.flat.clone()
    with pytest.raises(DyTError, match="holds %d elements, the engine trains %d" % (eng.n_train - 1, eng.n_train)):
        eng.ema_update(torch.zeros(eng.n_train - 1, device=DEV), 0.5)
    with pytest.raises(DyTError, match="contiguous fp32"):
        eng.ema_update(torch.zeros(eng.n_train, device=DEV, dtype=torch.float64), 0.5)
    with pytest.raises(DyTError, match="contiguous fp32"):
        eng.ema_update(torch.zeros(eng.n_train), 0.5)
    with pytest.raises(DyTError, match="dyt_ema_update"):
        eng.ema_update(torch.zeros(eng.n_train, device=DEV), 1.5)
    inf_eng = DyTEngine(C, RANK, 0.1, DEV, precision="fp32", max_batch=1, depth=1, inference=True)
    with pytest.raises(DyTError, match="inference_only"):
        inf_eng.ema_update(torch.zeros(inf_eng.n_train, device=DEV), 0.5)
    sh = torch.full((eng.n_train,), 2.0, device=DEV)
    eng.flat.fill_(1.0)
    eng.ema_update(sh, 0.75)
    assert torch.equal(sh, torch.full_like(sh, 1.75)) and torch.equal(eng.flat, torch.ones_like(flat0))


# ------------------------------------------------------------------------------------------------------------------------------
# 4 - 7: in the model
# ------------------------------------------------------------------------------------------------------------------------------
C, DEPTH, B, RANK, SEED = 10, 2, 4, 8, 31
DECAY = 0.9


class Cfg(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def _build(pool="token", precision="fp32", **kw):
    from models.vision_transformer_IN21K import VisionTransformer
    tuning = Cfg(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option="none", ffn_adapter_init_option="lora", ffn_adapter_scalar="0.1",
                 ffn_num=RANK, d_model=768)
    m = VisionTransformer(patch_size=16, embed_dim=768, depth=DEPTH, num_heads=12, mlp_ratio=4.0, qkv_bias=True, num_classes=C, drop_path_rate=0.0,
                          tuning_config=tuning, select_config=Cfg(open=True, keep_layers=0), precision=precision, train_mode="masked", max_batch=B,
                          global_pool=pool, **kw)
    for n, p in m.named_parameters():
        p.requires_grad = synth.is_trainable(n)
    m.load_state_dict(synth.make_state_dict(C, RANK, seed=SEED, kind="test", depth=DEPTH, gate_bias=0.85, head_norm="fc_norm" if pool == "avg" else "norm"),
                      strict=True)
    return m.cuda().train()


@pytest.fixture(scope="module")
def batch():
    x, y = synth.make_batch(B, C, seed=SEED)
    g1, g2 = synth.make_noise(B, depth=DEPTH, seed=SEED + 1)
    keep = synth.make_dropout_masks(B, RANK, depth=DEPTH, seed=SEED + 2)
    return x.cuda(), y.cuda(), (g1.cuda().contiguous(), g2.cuda().contiguous()), keep.cuda().contiguous()


def _step(model, opt, batch, seed, update=True):
    from engine_finetune import train_step
    x, y, gumbel, keep = batch
    return train_step(model, x, y, opt, gumbel=gumbel, keep_mask=keep, seed=seed, target_ratio=0.5, token_minimal=0.0, token_minimal_weight=0.0,
                      update=update)


def _np(t):
    return t.detach().cpu().numpy()


def _criterion():
    from models.losses import AdaLoss
    return AdaLoss(base_criterion=torch.nn.CrossEntropyLoss(), token_target_ratio=0.5, token_loss_ratio=2.0, token_minimal=0.0, token_minimal_weight=0.0)


def _loop_args(**kw):
    return types.SimpleNamespace(accum_iter=1, lr=1e-3, min_lr=1e-5, warmup_epochs=0, epochs=4, hip_graph=False, **kw)


@pytest.mark.parametrize("pool", ["token", "avg"])
def test_shadow_follows_the_reference_through_train_steps(pool, batch):
    from engine_finetune import FusedAdamW
    from util.model_ema import DeviceModelEma
    model = _build(pool)
    ema = DeviceModelEma(model, DECAY)
    opt = FusedAdamW(model, lr=1e-3, weight_decay=0.05)
    eng = model.engine(B, torch.device(DEV))
    flat0 = eng.flat.clone()
    assert eng.n_train == flat0.numel() and ema.shadow is None
    for i in range(3):
        _step(model, opt, batch, 700 + i)
        prev = ema.buffer().clone()
        if i == 0:   # the snapshot at construction, homed: the parameters as they were before the first step
            assert torch.equal(prev, flat0) and not torch.equal(eng.flat, flat0)
        ema.update()
        torch.cuda.synchronize()
        _same(_np(ema.shadow), R.ema_ref(_np(prev), _np(eng.flat), DECAY), "%s round %d" % (pool, i))
        assert ema.updates == i + 1 and not torch.equal(ema.shadow, eng.flat) and not torch.equal(ema.shadow, prev)
    assert opt.applied_and_skipped() == (3, 0)
    assert ema.shadow.data_ptr() != eng.flat.data_ptr()


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("pool", ["token", "avg"])
def test_train_one_epoch_updates_once_per_optimizer_update(pool, graph, batch, monkeypatch):
    from engine_finetune import FusedAdamW, train_one_epoch
    from util.model_ema import DeviceModelEma
    monkeypatch.setenv("DYT_PREFETCH", "0")   # (the copy-stream probe is a timing measurement: not what this test is about)
    x, y, gumbel, keep = batch
    one = (x.cpu(), y.cpu()) if graph else (x.cpu(), y.cpu(), tuple(t.cpu() for t in gumbel), keep.cpu())   # (a captured step draws on the device)
    loader = [one] * 4
    model = _build(pool)
    ema = DeviceModelEma(model, DECAY)
    opt = FusedAdamW(model, lr=1e-3, weight_decay=0.05)
    eng = model.engine(B, torch.device(DEV))
    flat0 = eng.flat.clone()
    post = []
    step = opt.step

    def recording_step(*a, **k):   # the parameters right behind every optimizer update, in stream order
        step(*a, **k)
        post.append(eng.flat.clone())
    opt.step = recording_step
    args = _loop_args(model_ema=ema)
    args.accum_iter, args.hip_graph = 2, graph
    train_one_epoch(model, _criterion(), loader, opt, torch.device(DEV), 0, None, 0, None, None, args=args)
    torch.cuda.synchronize()
    assert model._engine is eng and ema.updates == 2 and len(post) == 2 and opt.applied_and_skipped() == (2, 0)
    assert not torch.equal(post[0], flat0) and not torch.equal(post[1], post[0]) and torch.equal(post[1], eng.flat)
    want = _np(flat0)
    for s in post:
        want = R.ema_ref(want, _np(s), DECAY)
    _same(_np(ema.shadow), want, "%s graph=%s" % (pool, graph))
    if graph:
        assert len(eng._graphs) == 2   # the two captured steps (first / accumulating micro-batch); the update runs outside them


# ------------------------------------------------------------------------------------------------------------------------------
# 5: a skipped optimizer update
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [math.inf, math.nan])
def test_the_shadow_still_moves_when_the_guard_skips_the_update(value, batch):
    from engine_finetune import FusedAdamW
    from util.model_ema import DeviceModelEma
    model = _build()
    ema = DeviceModelEma(model, DECAY)
    opt = FusedAdamW(model, lr=1e-3, weight_decay=0.05)
    _step(model, opt, batch, 800)
    ema.update()
    eng = model._engine
    _step(model, opt, batch, 801, update=False)
    eng.grad[eng.n_train // 2] = value
    before, prev = eng.flat.clone(), ema.shadow.clone()
    opt.step()
    ema.update()
    torch.cuda.synchronize()
    assert torch.equal(eng.flat, before), "a skipped update leaves the parameters where they were"
    assert opt.applied_and_skipped() == (1, 1) and ema.updates == 2
    _same(_np(ema.shadow), R.ema_ref(_np(prev), _np(before), DECAY), "skipped update")
    assert not torch.equal(ema.shadow, prev)


# ------------------------------------------------------------------------------------------------------------------------------
# 6: the evaluation view
# ------------------------------------------------------------------------------------------------------------------------------
def _averaged(pool, precision, batch, **kw):
    """A model whose shadow differs from its parameters whatever the step does: the parameters are scaled after the snapshot, then one
    step and one update at decay 0.5."""
    from engine_finetune import FusedAdamW
    from util.model_ema import DeviceModelEma
    model = _build(pool, precision, **kw)
    ema = DeviceModelEma(model, 0.5)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if p.requires_grad:
                p.mul_(1.0625)
    opt = FusedAdamW(model, lr=1e-3, weight_decay=0.05)
    _step(model, opt, batch, 600)
    ema.update()
    return model, ema, opt


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("head", ["token", "avg", "wide"])
def test_view_equals_the_model_with_the_shadow_copied_over_its_parameters(head, precision, batch):
    x = batch[0]
    model, ema, _ = _averaged("avg" if head == "avg" else "token", precision, batch, **(dict(wide_head=True) if head == "wide" else {}))
    eng = model._engine
    assert eng.wide_head is (head == "wide") and not torch.equal(ema.shadow, eng.flat)
    model.eval()
    with torch.no_grad():
        own, own_aux = model(x)
        before = eng.flat.clone()
        out, aux = ema.module(x)
        torch.cuda.synchronize()
        assert torch.equal(eng.flat, before), "the view wrote the model's parameters"
        eng.flat.copy_(ema.shadow)
        want, want_aux = model(x)
        eng.flat.copy_(before)
        again, _ = model(x)
    torch.cuda.synchronize()
    assert torch.equal(out, want) and torch.equal(aux["token_select"], want_aux["token_select"]) and torch.equal(aux["token_logits"], want_aux["token_logits"])
    assert bool(torch.isfinite(out).all()) and not torch.equal(out, own), "the view ran on the model's own parameters"
    assert torch.equal(again, own) and tuple(aux["token_select"].shape) == (B, DEPTH, 196, 1)


def test_view_forward_features_refusals_and_delegation(batch):
    from _lib import DyTError
    x = batch[0]
    model, ema, _ = _averaged("token", "fp32", batch)
    eng, view = model._engine, ema.module
    with torch.no_grad(), pytest.raises(DyTError, match="eval"):   # train mode
        view(x)
    assert view.eval() is view and not model.training
    for call in (lambda: view(x), lambda: view.forward_features(x), lambda: model._forward(x, trainable=ema.shadow)):   # grad enabled
        with pytest.raises(DyTError, match="no_grad"):
            call()
    with torch.no_grad():
        before = eng.flat.clone()
        tok, aux = view.forward_features(x)
        tok2, taps, _ = view.forward_features(x, out_indices=(0,))
        assert torch.equal(eng.flat, before)
        eng.flat.copy_(ema.shadow)
        want, want_aux = model.forward_features(x)
        want2, want_taps, _ = model.forward_features(x, out_indices=(0,))
        eng.flat.copy_(before)
        own, _ = model.forward_features(x)
        with pytest.raises(DyTError, match="%d elements" % eng.n_train):
            model._forward(x, trainable=ema.shadow[:-1])
    torch.cuda.synchronize()
    assert torch.equal(tok, want) and torch.equal(aux["token_select"], want_aux["token_select"]) and not torch.equal(tok, own)
    assert torch.equal(tok2, want2) and torch.equal(taps[0], want_taps[0])
    assert view._engine is eng and view.prepare_input(x).data_ptr() == model.prepare_input(x).data_ptr() and view.takes_bytes(x) is False
    assert getattr(view, "module", view) is view


@pytest.mark.parametrize("stream", [False, True])
def test_evaluate_on_the_view_equals_evaluate_on_a_model_loaded_from_the_full_state_dict(stream, batch, monkeypatch):
    from engine_finetune import evaluate
    monkeypatch.setenv("DYT_PREFETCH", "0")
    x, y = batch[0], batch[1]
    model, ema, _ = _averaged("token", "fp32", batch)
    loader = [(x.cpu(), y.cpu()), (x.flip(0).cpu(), y.flip(0).cpu())]
    args = types.SimpleNamespace(metric="accuracy", nb_classes=C, stream_eval=stream)
    before = model._engine.flat.clone()
    got = evaluate(loader, ema.module, torch.device(DEV), None, None, None, args)
    assert not model.training and torch.equal(model._engine.flat, before)
    full = ema.state_dict(full=True)
    assert list(full) == list(model.state_dict())
    twin = _build()
    twin.load_state_dict(full, strict=True)
    want = evaluate(loader, twin, torch.device(DEV), None, None, None, args)
    own = evaluate(loader, model, torch.device(DEV), None, None, None, args)
    assert torch.equal(twin._engine.flat, ema.shadow)
    assert got == want and set(got) == set(own), (got, want)
    assert "metric" in got and "keep_ratio" in got and (not stream or "loss" in got)
    if stream:
        assert got["loss"] != own["loss"]   # the averaged model is another model


# ------------------------------------------------------------------------------------------------------------------------------
# 7: checkpoint round trip
# ------------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip_with_the_average(tmp_path, batch, monkeypatch):
    """train_one_epoch with args.model_ema, misc.save_model, misc.load_model into a fresh model + optimizer + DeviceModelEma: the next epoch's
    shadow, update count and parameters equal the uninterrupted run's bit for bit (fp32 mode: no atomics).  An old-style checkpoint
    without the keys still loads and leaves the shadow at its construction snapshot."""
    import misc
    from engine_finetune import train_one_epoch
    from util.model_ema import DeviceModelEma
    monkeypatch.setenv("DYT_PREFETCH", "0")
    x, y, gumbel, keep = batch
    loader = [(x.cpu(), y.cpu(), tuple(t.cpu() for t in gumbel), keep.cpu())] * 2
    crit = _criterion()
    dev = torch.device(DEV)

    def make():
        m = _build()
        o = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3, weight_decay=0.05)
        e = DeviceModelEma(m, DECAY)
        a = _loop_args(output_dir=str(tmp_path), save_freq=1, auto_remove=False, resume="", start_epoch=0, eval=False, model_ema=e)
        return m, o, e, a
    ma, oa, ea, args_a = make()
    train_one_epoch(ma, crit, loader, oa, dev, 0, None, 0, None, None, args=args_a)
    misc.save_model(args=args_a, epoch=0, model=ma, model_without_ddp=ma, optimizer=oa, save_force=True)
    ck = torch.load(tmp_path / "checkpoint-0.pth", map_location="cpu", weights_only=False)
    names = [n for n, p in ma.named_parameters() if p.requires_grad]
    assert sorted(ck["model_ema"]) == sorted(names) and len(names) == 6 * DEPTH + 2 and ck["model_ema_updates"] == 2
    assert all(not t.is_cuda and tuple(t.shape) == tuple(dict(ma.named_parameters())[n].shape) for n, t in ck["model_ema"].items())
    assert not hasattr(ck["args"], "model_ema") and args_a.model_ema is ea
    assert not torch.equal(ck["model_ema"]["head.weight"], ck["model"]["head.weight"])
    train_one_epoch(ma, crit, loader, oa, dev, 1, None, 0, None, None, args=args_a)

    mb, ob, eb, args_b = make()
    args_b.resume = str(tmp_path / "checkpoint-0.pth")
    misc.load_model(args=args_b, model_without_ddp=mb, optimizer=ob)
    assert args_b.start_epoch == 1 and eb.updates == 2 and eb.shadow is None   # pending until an engine exists
    train_one_epoch(mb, crit, loader, ob, dev, 1, None, 0, None, None, args=args_b)
    torch.cuda.synchronize()
    assert ea.updates == eb.updates == 4
    assert torch.equal(ea.shadow, eb.shadow), "the resumed run's shadow differs from the uninterrupted run's"
    for (n, a), (_, b) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(a.detach(), b.detach()), n
    assert not torch.equal(ea.shadow, ma._engine.flat)

    # an old-style checkpoint: no 'model_ema' keys
    plain = copy.copy(args_a)
    del plain.model_ema
    misc.save_model(args=plain, epoch=7, model=ma, model_without_ddp=ma, optimizer=oa, save_force=True)
    old = torch.load(tmp_path / "checkpoint-7.pth", map_location="cpu", weights_only=False)
    assert "model_ema" not in old and "model_ema_updates" not in old
    mc, oc, ec, args_c = make()
    snap = {k: v.clone() for k, v in ec.state_dict().items()}
    args_c.resume = str(tmp_path / "checkpoint-7.pth")
    misc.load_model(args=args_c, model_without_ddp=mc, optimizer=oc)
    assert args_c.start_epoch == 8 and ec.updates == 0
    assert all(torch.equal(ec.state_dict()[k], snap[k]) for k in snap)
    for (n, a), (_, c) in zip(ma.named_parameters(), mc.named_parameters()):
        assert torch.equal(a.detach().cpu(), c.detach().cpu()), n
