"""Parameter groups of the fused AdamW on the GPU: dyt_adamw_segments (csrc/step_tail.hip adamw_segments_kernel) on plain fp32 tensors through
the C ABI, then inside the model behind torch.optim.AdamW(param_groups_lrd(...)).

The kernel's contract is that every element sees the arithmetic of the one-group kernels, so the first yardstick is exact: one segmented
launch == dyt_adamw called slice by slice with each segment's lr / weight_decay, BIT FOR BIT.  The second is the rule of
tests/test_gpu_step_tail.py (its ``_cmp``): against tests/tail_refs.adamw_ref in fp64, with the same function in fp32 on the CPU as the
floor, max|gpu - fp64| <= 4 floor + 4 ulp.  Inside the model the reference is a CPU torch.optim.AdamW over fp64 copies of the parameters in
the same groups, fed the gradient the GPU step produced, and an fp32 one for the floor; a one-element tensor has no floor worth the name
(that module's note on scalars), so parameters are compared group by group -- a gate's [1] bias together with the other 1-D tensors of
its block."""
import ctypes
import math
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

import _lib  # noqa: E402
import synth  # noqa: E402
import tail_refs as R  # noqa: E402
import test_gpu_step_tail as T  # noqa: E402  (its helpers: _cmp, _adamw_inputs, _adamw_call)
from _lib import ptr, stream_ptr  # noqa: E402

DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
B1, B2, EPS = 0.9, 0.999, 1e-8
LRS, WDS = (0.0, 1e-3, 3e-2), (0.0, 0.05)
NUMELS = [1, 255, 257, 70001]


class Cfg(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def _seg_rc(p, g, m, v, state, step, table, gs=1.0, n=None):
    arr = _lib.adamw_segment_array(table) if table else (_lib.AdamwSegment * 1)()
    return _lib.lib().dyt_adamw_segments(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), ptr(state), int(step), ctypes.cast(arr, ctypes.c_void_p),
                                         len(table) if n is None else n, B1, B2, EPS, gs, stream_ptr())


def _seg_call(*a, **k):
    _lib.check(_seg_rc(*a, **k))


def _table(ends):
    """lr cycles over {0, 1e-3, 3e-2}, weight_decay over {0, 0.05}: all six pairs appear from six segments on."""
    return [(e, LRS[k % 3], WDS[k % 2]) for k, e in enumerate(ends)]


def _tables(n):
    out = {"one segment": [(n, 1e-3, 0.05)]}
    cuts = sorted(c for c in {1, 63, 64, 65, 256, 257, 511, n - 1} if 0 < c < n)
    if cuts:   # inside a wave, on a wave edge, on a workgroup edge, one-element segments, one segment over many workgroups
        out["edges"] = _table(cuts + [n])
    if n == 70001:   # the full table: 31 one-element segments in a row, cuts on 20 workgroup edges, the rest drawn
        cuts = set(range(1000, 1031)) | {256 * k for k in range(100, 120)}
        g = torch.Generator().manual_seed(128)
        while len(cuts) < 127:
            cuts.add(int(torch.randint(1, n, (1,), generator=g)))
        out["128 segments"] = _table(sorted(cuts) + [n])
        assert len(out["128 segments"]) == 128
    return out


def _sliced(p0, g0, m0, v0, step, table, gs):
    """dyt_adamw slice by slice: the parent's kernel with each segment's hyper-parameters."""
    dev = [t.clone().cuda() for t in (p0, g0, m0, v0)]
    a = 0
    for e, lr, wd in table:
        T._adamw_call(*(t[a:e] for t in dev), step, lr, B1, B2, EPS, wd, gs)
        a = e
    return dev


def _refs(p0, g0, m0, v0, step, table, gs, dtype):
    parts, a = [], 0
    for e, lr, wd in table:
        parts.append(R.adamw_ref(p0[a:e], g0[a:e], m0[a:e], v0[a:e], step, lr, B1, B2, EPS, wd, gs, dtype=dtype))
        a = e
    return tuple(torch.cat([q[i] for q in parts]) for i in range(3))


# ------------------------------------------------------------------------------------------------------------------------------
# 1 + 2: segmented against sliced (bitwise) and against fp64
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NUMELS)
def test_segments_equal_sliced_updates_bitwise_and_fp64_within_the_rule(n):
    for step in (1, 1000):
        p0, g0, m0, v0, _ = T._adamw_inputs(n, 40 + step, with_moments=step > 1)
        zero_p = p0 == 0
        for name, table in _tables(n).items():
            for gs in (1.0, 0.125):
                tag = "n=%d step %d %s grad_scale %g" % (n, step, name, gs)
                want = _sliced(p0, g0, m0, v0, step, table, gs)
                dev = [t.clone().cuda() for t in (p0, g0, m0, v0)]
                _seg_call(*dev, None, step, table, gs)
                gd = [t.clone().cuda() for t in (p0, g0, m0, v0)]
                state = torch.tensor([step - 1, 0, 0, 7], dtype=torch.int32, device=DEV)
                _seg_call(*gd, state, 0, table, gs)   # guarded: `step` is ignored, the count is state[0] + 1
                torch.cuda.synchronize()
                for i, what in ((0, "p"), (2, "m"), (3, "v")):
                    assert torch.equal(dev[i], want[i]), "%s: %s differs from the sliced dyt_adamw calls" % (tag, what)
                    assert torch.equal(gd[i], dev[i]), "%s: guarded %s differs from the unguarded" % (tag, what)
                assert state.cpu().tolist() == [step, 0, 0, 7], tag
                assert torch.equal(dev[1].cpu(), g0) and torch.equal(gd[1].cpu(), g0), "the gradient is read only"
                # lr = 0: the parameters stay bit-identical while the moments advance
                a = 0
                for e, lr, wd in table:
                    if lr == 0.0:
                        assert torch.equal(dev[0][a:e].cpu(), p0[a:e]), (tag, a, e)
                        moved = g0[a:e] != 0
                        if bool(moved.any()):
                            assert bool((dev[2][a:e].cpu()[moved] != m0[a:e][moved]).any()) and bool((dev[3][a:e].cpu()[moved] != v0[a:e][moved]).any()), (tag, a, e)
                    a = e
                r64, r32 = _refs(p0, g0, m0, v0, step, table, gs, F64), _refs(p0, g0, m0, v0, step, table, gs, F32)
                for what, got, b, c in zip(("p", "m", "v"), (dev[0], dev[2], dev[3]), r64, r32):
                    T._cmp("adamw_segments", "%s %s" % (tag, what), got, b, c)
                if bool(zero_p.any()):
                    T._cmp("adamw_segments", "%s p where it was 0" % tag, dev[0].cpu()[zero_p], r64[0][zero_p], r32[0][zero_p])


# ------------------------------------------------------------------------------------------------------------------------------
# 3: the guard covers every segment
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where,value", [(0, math.inf), (70000, -math.inf), (1010, math.nan)])
def test_guard_skips_every_segment_when_one_gradient_is_not_finite(where, value):
    n, gs = 70001, 1.0
    table = _tables(n)["128 segments"]
    p0, g0, m0, v0, _ = T._adamw_inputs(n, 5, True)
    bad = g0.clone()
    bad[where] = value
    dev = [t.clone().cuda() for t in (p0, bad, m0, v0)]
    state = torch.tensor([4, 2, 0, 0], dtype=torch.int32, device=DEV)
    _seg_call(*dev, state, 0, table, gs)
    torch.cuda.synchronize()
    assert torch.equal(dev[0].cpu(), p0) and torch.equal(dev[2].cpu(), m0) and torch.equal(dev[3].cpu(), v0)
    assert state.cpu().tolist()[:3] == [4, 3, 1]
    dev[1] = g0.clone().cuda()
    _seg_call(*dev, state, 0, table, gs)
    plain = [t.clone().cuda() for t in (p0, g0, m0, v0)]
    _seg_call(*plain, None, 5, table, gs)
    torch.cuda.synchronize()
    assert state.cpu().tolist()[:3] == [5, 3, 0]
    assert torch.equal(dev[0], plain[0]) and torch.equal(dev[2], plain[2]) and torch.equal(dev[3], plain[3])


# ------------------------------------------------------------------------------------------------------------------------------
# 4: refusals
# ------------------------------------------------------------------------------------------------------------------------------
def test_bad_tables_are_refused_before_anything_is_enqueued():
    n = 300
    p0, g0, m0, v0, _ = T._adamw_inputs(n, 9, True)
    dev = [t.clone().cuda() for t in (p0, g0, m0, v0)]
    state = torch.tensor([3, 1, 0, 0], dtype=torch.int32, device=DEV)
    L = _lib.lib()
    ok = (1e-3, 0.05)
    cases = [("no segment", [], 0), ("129 segments", [(i + 1,) + ok for i in range(128)] + [(n,) + ok], None),
             ("equal ends", [(100,) + ok, (100,) + ok, (n,) + ok], None), ("falling ends", [(200,) + ok, (100,) + ok, (n,) + ok], None),
             ("an empty first segment", [(0,) + ok, (n,) + ok], None), ("a short table", [(100,) + ok, (n - 1,) + ok], None),
             ("a long table", [(100,) + ok, (n + 1,) + ok], None)]
    for what, table, cnt in cases:
        for st in (None, state):
            assert _seg_rc(*dev, st, 1, table, n=cnt) == -1, what   # DYT_ERR_ARG
            assert L.dyt_last_error().decode().strip(), what
    torch.cuda.synchronize()
    assert torch.equal(dev[0].cpu(), p0) and torch.equal(dev[2].cpu(), m0) and torch.equal(dev[3].cpu(), v0)
    assert state.cpu().tolist() == [3, 1, 0, 0]
    table = _table([100, n])
    _seg_call(*dev, state, 0, table)
    want = _sliced(p0, g0, m0, v0, 4, table, 1.0)
    torch.cuda.synchronize()
    assert torch.equal(dev[0], want[0]) and torch.equal(dev[2], want[2]) and torch.equal(dev[3], want[3]) and state.cpu().tolist()[:3] == [4, 1, 0]


# ------------------------------------------------------------------------------------------------------------------------------
# 5 - 7: in the model
# ------------------------------------------------------------------------------------------------------------------------------
C, DEPTH, B, RANK, SEED = 10, 2, 4, 8, 31


def _build(pool="token", precision="fp32"):
    from models.vision_transformer_IN21K import VisionTransformer
    tuning = Cfg(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option="none", ffn_adapter_init_option="lora", ffn_adapter_scalar="0.1",
                 ffn_num=RANK, d_model=768)
    m = VisionTransformer(patch_size=16, embed_dim=768, depth=DEPTH, num_heads=12, mlp_ratio=4.0, qkv_bias=True, num_classes=C, drop_path_rate=0.0,
                          tuning_config=tuning, select_config=Cfg(open=True, keep_layers=0), precision=precision, train_mode="masked", max_batch=B,
                          global_pool=pool)
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


def _cpu_twin(model, groups, dtype):
    """torch.optim.AdamW on the CPU over copies of the parameters in the same groups; the scalars a C float carries are widened from their
    float32 value (tail_refs.f32), so that the comparison measures the arithmetic."""
    twin = {id(p): torch.nn.Parameter(p.detach().to("cpu", dtype).clone()) for _, p in model.named_parameters() if p.requires_grad}
    gs = [dict(params=[twin[id(p)] for p in g["params"]], lr_scale=g["lr_scale"], weight_decay=R.f32(g["weight_decay"])) for g in groups]
    return twin, torch.optim.AdamW(gs, lr=1e-3, betas=(R.f32(B1), R.f32(B2)), eps=R.f32(EPS))


@pytest.mark.parametrize("pool", ["token", "avg"])
def test_layer_decay_groups_in_the_model_against_cpu_adamw(pool, batch):
    import util.lr_sched as lr_sched
    from engine_finetune import FusedAdamW, as_fused
    from util.lr_decay import param_groups_lrd
    model = _build(pool)
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    assert len(named) == 6 * DEPTH + (4 if pool == "avg" else 2)
    groups = param_groups_lrd(model, 0.05, model.no_weight_decay(), 0.75)
    assert len(groups) == 2 * (DEPTH + 1)
    topt = torch.optim.AdamW(groups, lr=1e-3)
    opt = as_fused(topt, model)
    assert opt.param_groups is topt.param_groups and len(opt.param_groups) == len(groups)
    eng = model.engine(B, torch.device(DEV))

    # the 1-D tensors really see weight_decay 0: with a zero gradient (and zero moments) and lr > 0 they do not move, the matrices decay
    before = eng.flat.clone()
    eng.grad.zero_()
    probe = FusedAdamW(model, params=[dict(g) for g in groups], lr=1e-3)
    probe.step()
    torch.cuda.synchronize()
    for n, p in named:
        off, num = eng.trainable_slice(n)
        old = before[off:off + num]
        if p.ndim == 1:
            assert torch.equal(p.detach().reshape(-1), old), n
        else:
            assert not torch.equal(p.detach().reshape(-1), old), n
            torch.testing.assert_close(p.detach().reshape(-1), old * (1.0 - 1e-3 * 0.05), rtol=1e-6, atol=0.0)
    assert probe.applied_and_skipped() == (1, 0)
    eng.flat.copy_(before)

    tw64, o64 = _cpu_twin(model, groups, F64)
    tw32, o32 = _cpu_twin(model, groups, F32)
    args = types.SimpleNamespace(lr=1e-3, min_lr=0.0, warmup_epochs=1.0, epochs=2.0)
    seen_tables = []
    for i in range(3):
        for o in (opt, o64, o32):   # warm-up over the three steps
            lr = lr_sched.adjust_learning_rate(o, (i + 1) / 3.0, args)
        assert abs(lr - 1e-3 * (i + 1) / 3.0) < 1e-15 and opt.param_groups[0]["lr"] == lr * 0.75 ** DEPTH
        for o in (o64, o32):
            for g in o.param_groups:
                g["lr"] = R.f32(g["lr"])
        _step(model, opt, batch, 900 + i, update=False)
        grad = eng.grad.clone()
        seen_tables.append(opt.segment_table(eng))
        opt.step()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0
        for n, p in named:
            off, num = eng.trainable_slice(n)
            g = grad[off:off + num].view(p.shape).cpu()
            tw64[id(p)].grad, tw32[id(p)].grad = g.double(), g.clone()
        o64.step()
        o32.step()
        for k, g in enumerate(groups):
            cat = lambda tw: torch.cat([tw[id(p)].detach().reshape(-1) for p in g["params"]])   # noqa: E731
            got = torch.cat([p.detach().reshape(-1) for p in g["params"]])
            T._cmp("adamw_segments", "%s model step %d group %d (lr_scale %.4g, weight_decay %g, %d tensors)" % (
                pool, i + 1, k, g["lr_scale"], g["weight_decay"], len(g["params"])), got, cat(tw64), cat(tw32))
    assert opt.applied_and_skipped() == (3, 0)
    # decay / no_decay alternate tensor by tensor in the flat buffer and the lr changes block by block: many segments, all in one launch
    assert all(len(t) > 2 * (DEPTH + 1) for t in seen_tables) and seen_tables[0] != seen_tables[1]
    assert seen_tables[0][-1][0] == eng.n_train


def test_checkpoint_round_trip_of_a_multi_group_run(tmp_path, batch, monkeypatch):
    """Decay / no_decay groups over the blocks and the head in a group of its own at lr_scale 10, behind the driver's torch.optim.AdamW:
    train_one_epoch, misc.save_model, misc.load_model into a fresh model + optimizer, and the next epoch equals the uninterrupted run's bit
    for bit (fp32 mode: no atomics)."""
    import misc
    from engine_finetune import train_one_epoch
    from models.losses import AdaLoss
    monkeypatch.setenv("DYT_PREFETCH", "0")   # (the copy-stream probe is a timing measurement: not what this test is about)
    x, y, gumbel, keep = batch
    loader = [(x.cpu(), y.cpu(), tuple(t.cpu() for t in gumbel), keep.cpu())] * 2
    crit = AdaLoss(base_criterion=torch.nn.CrossEntropyLoss(), token_target_ratio=0.5, token_loss_ratio=2.0, token_minimal=0.0, token_minimal_weight=0.0)
    args = types.SimpleNamespace(output_dir=str(tmp_path), epochs=4, save_freq=1, auto_remove=False, resume="", start_epoch=0, eval=False,
                                 accum_iter=1, lr=1e-3, min_lr=1e-5, warmup_epochs=1, hip_graph=False)

    def make():
        m = _build()
        body = [(n, p) for n, p in m.named_parameters() if p.requires_grad and not n.startswith("head.")]
        gs = [dict(params=[p for n, p in body if p.ndim > 1], weight_decay=0.05), dict(params=[p for n, p in body if p.ndim == 1], weight_decay=0.0),
              dict(params=[m.head.bias, m.head.weight], weight_decay=0.05, lr_scale=10.0)]
        return m, torch.optim.AdamW(gs, lr=1e-3)
    dev = torch.device(DEV)
    ma, oa = make()
    train_one_epoch(ma, crit, loader, oa, dev, 0, None, 0, None, None, args=args)
    misc.save_model(args=args, epoch=0, model=ma, model_without_ddp=ma, optimizer=oa, save_force=True)
    ck = torch.load(tmp_path / "checkpoint-0.pth", map_location="cpu", weights_only=False)
    n_train = 6 * DEPTH + 2
    assert [len(g["params"]) for g in ck["optimizer"]["param_groups"]] == [3 * DEPTH, 3 * DEPTH, 2] and len(ck["optimizer"]["state"]) == n_train
    assert ck["optimizer"]["param_groups"][2]["lr_scale"] == 10.0 and "lr_scale" not in ck["optimizer"]["param_groups"][0]
    assert ck["optimizer"]["param_groups"][2]["lr"] == 10.0 * ck["optimizer"]["param_groups"][0]["lr"]
    assert all(float(st["step"]) == 2.0 for st in ck["optimizer"]["state"].values())
    assert tuple(ck["optimizer"]["state"][n_train - 2]["exp_avg"].shape) == (C,)   # group order: head.bias before head.weight
    stats_a = train_one_epoch(ma, crit, loader, oa, dev, 1, None, 0, None, None, args=args)
    mb, ob = make()
    args.resume = str(tmp_path / "checkpoint-0.pth")
    misc.load_model(args=args, model_without_ddp=mb, optimizer=ob)
    assert args.start_epoch == 1 and ob.param_groups[2]["lr_scale"] == 10.0
    stats_b = train_one_epoch(mb, crit, loader, ob, dev, 1, None, 0, None, None, args=args)
    torch.cuda.synchronize()
    assert stats_a["loss"] == stats_b["loss"] and stats_a["lr"] == stats_b["lr"]
    for (n, a), (_, b) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(a.detach(), b.detach()), n
    assert oa._dyt_fused.applied_and_skipped() == ob._dyt_fused.applied_and_skipped() == (4, 0)
    assert len(ob._dyt_fused.param_groups) == 3 and ob._dyt_fused.param_groups is ob.param_groups


def test_groups_with_equal_hyper_parameters_are_the_single_group_run(batch):
    """Three groups with one lr / weight_decay merge into one segment, and the segmented launch is the parent's kernel bit for bit."""
    from engine_finetune import FusedAdamW
    ma, mb = _build(), _build()
    pa = [p for _, p in ma.named_parameters() if p.requires_grad]
    one = FusedAdamW(mb, lr=1e-3, weight_decay=0.05)
    three = FusedAdamW(ma, params=[dict(params=pa[0::3]), dict(params=pa[2::3][::-1]), dict(params=pa[1::3])], lr=1e-3, weight_decay=0.05)
    for i in range(3):
        la = _step(ma, three, batch, 50 + i).clone()
        lb = _step(mb, one, batch, 50 + i).clone()
        torch.cuda.synchronize()
        assert torch.equal(la, lb), i
        assert torch.equal(ma._engine.flat, mb._engine.flat), "parameters differ after step %d" % (i + 1)
    assert len(three.segment_table(ma._engine)) == 1 and three.applied_and_skipped() == one.applied_and_skipped() == (3, 0)
    assert torch.equal(three.exp_avg, one.exp_avg) and torch.equal(three.exp_avg_sq, one.exp_avg_sq)
