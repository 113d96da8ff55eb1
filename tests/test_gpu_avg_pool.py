"""GPU tests of the mean-pooled / fc_norm classification head (csrc/pool_avg.hip, DYT_CREATE_AVG_POOL / DYT_CREATE_FC_NORM): the context-free
unit entry dyt_pool_head on both libraries, whole steps against the two fixtures recorded from the real reference, the B = 16 parity shape
against tests/pool_head_refs.py, context properties (inference-only contexts, wide against row-kernel head, the adapter's LayerNorm,
refusals, the flat layout) and a checkpoint round trip.

Bounds.  Unit entry and the head inside a context: the rule of tests/test_gpu_step_tail.py -- the reference is evaluated in fp64 and, on the
CPU, in fp32; floor = max|fp32_cpu - fp64|; the kernel must satisfy max|gpu - fp64| <= 4 floor + 4 ulp(max|fp64|).  The mean over 196 rows
is one more summation (7 runs of 28) of the kind the factor 4 was set for.  Whole steps: the bars of tests/gpu_diag.py (TOL,
FP16_GRAD_TOL_SMALL_B, BF16_GRAD_TOL_SMALL_B; fp32 gradients 2e-3 relative L2 as report_grads has it); fc_norm.* is judged under the
``head`` bound.  Decisions at B = 16: the tie rule of tests/parity_rules.py.  The AdamW bars are those of
test_gpu_round6.test_adapter_layernorm_step_vs_reference_golden.  No tolerance of its own is introduced here."""
import ctypes
import math
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _lib  # noqa: E402
import gpu_diag as D  # noqa: E402
import parity_rules as PR  # noqa: E402
import pool_head_refs as PH  # noqa: E402
import synth  # noqa: E402
import tail_refs as R  # noqa: E402
from _lib import DyTError, ptr, stream_ptr  # noqa: E402
from oracle import dyt_oracle as O  # noqa: E402
from runtime import DyTEngine  # noqa: E402

DEV = "cuda:0"
RANK, SEED = 8, 91
F32, F64 = torch.float32, torch.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pool")
FIXTURES = {"avg": "avg_pool_step.npz", "token": "token_fc_norm_step.npz"}
MODEL_KW = {"avg": dict(global_pool="avg"), "token": dict(global_pool="token", fc_norm=True)}
POOL_FLAGS = {"avg": _lib.CREATE_AVG_POOL | _lib.CREATE_FC_NORM, "token": _lib.CREATE_FC_NORM}
WORST = {}


def _cmp(kernel, what, gpu, ref64, ref32):
    """max|gpu - fp64| <= 4 max|fp32_cpu - fp64| + 4 ulp(max|fp64|); prints error / floor."""
    gpu, ref64, ref32 = gpu.detach().to("cpu", F64), ref64.detach().to(F64), ref32.detach().to("cpu", F64)
    assert gpu.shape == ref64.shape == ref32.shape, (what, gpu.shape, ref64.shape, ref32.shape)
    assert bool(torch.isfinite(ref64).all()) and bool(torch.isfinite(ref32).all()), "%s: the reference is not finite" % what
    err = float((gpu - ref64).abs().max()) if bool(torch.isfinite(gpu).all()) else math.inf
    floor = float((ref32 - ref64).abs().max())
    bound = 4.0 * floor + 4.0 * R.ulp(ref64.abs().max())
    ratio = err / floor if floor > 0 else (0.0 if err == 0 else math.inf)
    print("[%s] %s: error %.3e floor %.3e error/floor %s bound %.3e" % (kernel, what, err, floor, "%.2f" % ratio if floor > 0 else ("-" if err == 0 else "inf"), bound))
    if math.isfinite(ratio) and ratio > WORST.get(kernel, (-1.0, ""))[0]:
        WORST[kernel] = (ratio, what)
    assert err <= bound, "[%s] %s: |gpu - fp64| = %.3e > 4 * %.3e + 4 ulp = %.3e" % (kernel, what, err, floor, bound)


@pytest.fixture(scope="module", autouse=True)
def _worst_table():
    yield
    print("\nworst error / floor per kernel:")
    for k in sorted(WORST):
        print("  %-28s %8.2f   (%s)" % (k, WORST[k][0], WORST[k][1]))


def _gen(*key):
    return torch.Generator().manual_seed(abs(hash(tuple(int(k) for k in key))) % (2 ** 31))


# ------------------------------------------------------------------------------------------------------------------------------
# unit entry: dyt_pool_head
# ------------------------------------------------------------------------------------------------------------------------------
UNIT_SHAPES = [(B, C) for B in (1, 3, 33) for C in (1, 10, 1000, 1025, 2049)]
NAMES = ("logits", "dx_tokens", "d fc_norm.weight", "d fc_norm.bias", "d head.weight", "d head.bias")
_unit_cache = {}


def _unit_inputs(B, C, pool):
    """Inputs and the fp64 / fp32 references of one case: computed once, shared by the two libraries, never modified.  The rows the pooling
    must NOT read carry 1e4-scale values: the cls row under 'avg', the patch rows under 'token'."""
    key = (B, C, pool)
    if key not in _unit_cache:
        g = _gen(B, C, len(pool), 13)
        x = torch.randn(B, 197, 768, generator=g)
        loud = 1e4 * torch.randn(B, 197, 768, generator=g)
        if pool == "avg":
            x[:, 0] = loud[:, 0]
        else:
            x[:, 1:] = loud[:, 1:]
        nw, nb = 1.0 + 0.1 * torch.randn(768, generator=g), 0.1 * torch.randn(768, generator=g)
        hw, hb = 0.02 * torch.randn(C, 768, generator=g), 0.02 * torch.randn(C, generator=g)
        single = torch.zeros(B, C)
        single[B // 2, C // 2] = 1.5
        dls = {"randn": torch.randn(B, C, generator=g), "single entry": single}
        pre = [0.5 * torch.randn(768, generator=g), 0.5 * torch.randn(768, generator=g), torch.randn(C, 768, generator=g), torch.randn(C, generator=g)]
        refs = {k: (PH.head_ref(x, nw, nb, hw, hb, dl, pool), PH.head_ref(x, nw, nb, hw, hb, dl, pool, dtype=F32)) for k, dl in dls.items()}
        _unit_cache[key] = (x, nw, nb, hw, hb, dls, pre, refs)
    return _unit_cache[key]


def _pool_head(L, dev, dl, dx, dgw, dgb, dW, db, B, C, flags):
    x, nw, nb, hw, hb = dev
    logits = torch.full((B, C), float("nan"), device=DEV)
    _lib.check(L.dyt_pool_head(ptr(x), ptr(nw), ptr(nb), ptr(hw), ptr(hb), ptr(logits), ptr(dl), ptr(dx), ptr(dgw), ptr(dgb), ptr(dW), ptr(db),
                               B, C, flags, stream_ptr()), L)
    return logits


@pytest.mark.parametrize("fp16_lib", [False, True], ids=["libdyt_hip", "libdyt_hip_f16"])
@pytest.mark.parametrize("pool", ["avg", "token"])
@pytest.mark.parametrize("B,C", UNIT_SHAPES)
def test_pool_head_unit_entry_against_fp64(B, C, pool, fp16_lib):
    L = _lib.lib(fp16=fp16_lib)
    flags = POOL_FLAGS[pool] | (_lib.CREATE_WIDE_HEAD if C > 1024 else 0)
    x, nw, nb, hw, hb, dls, pre, refs = _unit_inputs(B, C, pool)
    dev = tuple(t.cuda().contiguous() for t in (x, nw, nb, hw, hb))
    kern = "pool_head %s %s" % (pool, "wide" if C > 1024 else "rows")
    tag0 = "%s %s C=%d B=%d" % ("f16 lib" if fp16_lib else "lib", pool, C, B)

    def run(dl, prefill=None):
        dx = torch.full((B, 197, 768), float("nan"), device=DEV)
        outs = [torch.zeros(768, device=DEV), torch.zeros(768, device=DEV), torch.zeros(C, 768, device=DEV), torch.zeros(C, device=DEV)]
        if prefill is not None:
            outs = [p.cuda().contiguous() for p in prefill]
        logits = _pool_head(L, dev, dl, dx, outs[0], outs[1], outs[2], outs[3], B, C, flags)
        torch.cuda.synchronize()
        return [logits, dx] + outs

    for kind, dl_cpu in dls.items():
        dl = dl_cpu.cuda().contiguous()
        r64, r32 = refs[kind]
        got = run(dl)
        tag = "%s dlogits %s" % (tag0, kind)
        for i, name in enumerate(NAMES):
            if i == 0 and kind != "randn":
                continue
            _cmp(kern, tag + " " + name, got[i], r64[i], r32[i])
        dx = got[1].cpu()
        if pool == "avg":   # the cls row is exactly 0 and every patch row of an image is the same bits
            assert float(dx[:, 0].abs().max()) == 0.0 and not bool(torch.signbit(dx[:, 0]).any())
            assert torch.equal(dx[:, 1:], dx[:, 1:2].expand(B, 196, 768))
        else:               # only the cls row carries a gradient
            assert float(dx[:, 1:].abs().max()) == 0.0
        if kind == "single entry":   # nothing leaks into another class's row or bias, nor into another image
            rest = torch.ones(C, dtype=torch.bool)
            rest[C // 2] = False
            dWc, dbc = got[4].cpu(), got[5].cpu()
            assert float(dWc[rest].abs().max() if C > 1 else 0.0) == 0.0 and float(dbc[rest].abs().max() if C > 1 else 0.0) == 0.0
            assert float(dbc[C // 2]) == 1.5
            other = torch.ones(B, dtype=torch.bool)
            other[B // 2] = False
            assert float(dx[other].abs().max() if B > 1 else 0.0) == 0.0
            continue
        # the += contract: pre-filled gradients come back as themselves plus the gradient; dx_tokens is overwritten either way
        got2 = run(dl, prefill=pre)
        for i in range(2, 6):
            _cmp(kern, tag + " pre-filled " + NAMES[i], got2[i], pre[i - 2].double() + r64[i], pre[i - 2] + r32[i])
        # two identical calls: the same bits in every output
        got3 = run(dl)
        assert all(torch.equal(a, b) for a, b in zip(got3, got)) and torch.equal(got2[0], got[0]) and torch.equal(got2[1], got[1])
        # every d_* may be NULL; forward only (dlogits NULL) touches no gradient
        dx4 = torch.full((B, 197, 768), float("nan"), device=DEV)
        logits4 = _pool_head(L, dev, dl, dx4, None, None, None, None, B, C, flags)
        assert torch.equal(logits4, got[0]) and torch.equal(dx4, got[1])
        mark = torch.full((B, 197, 768), 7.0, device=DEV)
        logits5 = _pool_head(L, dev, None, mark, None, None, None, None, B, C, flags)
        assert torch.equal(logits5, got[0]) and bool((mark == 7.0).all())


def test_pool_head_unit_entry_refuses_bad_arguments():
    L = _lib.lib()
    t = torch.zeros(197 * 768, device=DEV)
    args = lambda C, flags: (ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), None, None, None, None, None, None, 1, C, flags, stream_ptr())   # noqa: E731
    for C, flags, word in ((1, 0, "create_flags"), (1, _lib.CREATE_WIDE_HEAD, "create_flags"), (1, 8 | POOL_FLAGS["avg"], "create_flags"),
                           (1, _lib.CREATE_AVG_POOL, "create_flags"), (1025, POOL_FLAGS["avg"], "1..1024"), (0, _lib.CREATE_FC_NORM, "bad argument")):
        assert L.dyt_pool_head(*args(C, flags)) == -1
        assert word in L.dyt_last_error().decode(), (C, flags, L.dyt_last_error())


# ------------------------------------------------------------------------------------------------------------------------------
# whole steps against the fixtures recorded from the real reference
# ------------------------------------------------------------------------------------------------------------------------------
def _tuning(r, ln="none"):
    return D.Cfg(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option=ln, ffn_adapter_init_option="lora", ffn_adapter_scalar="0.1",
                 ffn_num=r, d_model=768)


def _kind(name):
    return "head" if name.startswith("fc_norm.") else D.grad_kind(name)


def _judge_grads(precision, items):
    """items: (name, got, ref).  The bars of gpu_diag.report_grads with fc_norm.* under ``head``; returns {kind: (worst, name)}."""
    if precision != "fp32":   # the 12 one-number gate-bias gradients as one 12-vector (report_grads)
        sc1 = [it for it in items if it[2].numel() == 1]
        items = [it for it in items if it[2].numel() > 1]
        if sc1:
            items.append(("mlp_token_select.mlp_head.bias (12 blocks)", torch.stack([a.reshape(()) for _, a, _ in sc1]), torch.stack([b.reshape(()) for _, _, b in sc1])))
    worst = {}
    for n, got, ref in items:
        e = float((got - ref).norm() / max(float(ref.norm()), 1e-20))
        k = _kind(n) if precision in ("fp16", "bf16") else ("fc_norm" if n.startswith("fc_norm.") else "all")
        if e > worst.get(k, (-1.0, ""))[0]:
            worst[k] = (e, n)
    small_b = D.FP16_GRAD_TOL_SMALL_B if precision == "fp16" else D.BF16_GRAD_TOL_SMALL_B
    for k, (e, n) in worst.items():
        bound = 2e-3 if precision == "fp32" else (D.TOL[precision]["grad"] if precision in D.SPLIT_MODES else small_b[k])
        assert e <= bound, (precision, k, n, e, bound)
    return worst


@pytest.mark.parametrize("pool", ["avg", "token"])
@pytest.mark.parametrize("precision", ["fp32", "fp16x3q", "fp16", "bf16"])
def test_step_vs_reference_golden(precision, pool):
    """The reference model built with global_pool='avg' (resp. 'token', fc_norm=True), stepped through its own train_one_epoch: logits of
    both passes, decisions, the five loss components, all 76 gradients -- d fc_norm.weight / .bias included -- of the fused step in the
    masked mode; fp32 also fc_norm.* and head.* after one AdamW update."""
    from models.vision_transformer_IN21K import vit_base_patch16_224_in21k
    g = dict(np.load(os.path.join(GOLDEN, FIXTURES[pool])))
    B, C, r, seed = int(g["meta_batch"]), int(g["meta_num_classes"]), int(g["meta_ffn_num"]), int(g["meta_seed"])
    x, y = synth.make_batch(B, C, seed=seed)
    keep = synth.make_dropout_masks(B, r, seed=seed + 3)
    g1, g2 = torch.from_numpy(g["g1"]), torch.from_numpy(g["g2"])
    sd = synth.make_state_dict(C, r, seed=seed, kind="test", gate_bias=float(g["meta_gate_bias"]), head_norm="fc_norm")
    tol = D.TOL[precision]
    model = vit_base_patch16_224_in21k(num_classes=C, drop_path_rate=0.0, tuning_config=_tuning(r), select_config=D.Cfg(open=True, keep_layers=0),
                                       precision=precision, train_mode="masked", **MODEL_KW[pool])
    msg = model.load_state_dict(sd, strict=True)
    assert not msg.missing_keys and not msg.unexpected_keys
    for n, p in model.named_parameters():
        p.requires_grad = synth.is_trainable(n)
    model = model.cuda()
    assert sum(p.requires_grad for p in model.parameters()) == 76
    model.train()
    eng = model.engine(B, torch.device("cuda", 0))
    assert eng.fc_norm is True and eng.avg_pool is (pool == "avg")
    ls, lt = torch.empty(B, C, device="cuda"), torch.empty(B, C, device="cuda")
    ts = torch.zeros(B, 12, 196, device="cuda")
    losses = eng.step_fwd_bwd(x.cuda(), y.cuda(), 0.5, 2.0, 0.0, 0.0, masked_dense=True, g1=g1.cuda().contiguous(), g2=g2.cuda().contiguous(),
                              keep_mask=keep.cuda().contiguous(), logits_s=ls, logits_t=lt, token_select=ts).cpu()
    es = float(np.abs(ls.cpu().numpy() - g["logits_student"]).max())
    et = float(np.abs(lt.cpu().numpy() - g["logits_teacher"]).max())
    flips = int((ts.cpu().numpy().astype(np.uint8) != g["token_select"][..., 0]).sum())
    el = max(abs(float(losses[i]) - float(g["stat_" + k])) / max(1.0, abs(float(g["stat_" + k])))
             for i, k in enumerate(("loss", "base_loss", "token_loss", "teacher_loss", "distillation_loss")))
    gref = {n[len("grad/"):]: torch.from_numpy(v) for n, v in g.items() if n.startswith("grad/")}
    assert "fc_norm.weight" in gref and "fc_norm.bias" in gref
    items = [(n, eng.trainable_view(n, gr.shape, eng.grad).cpu(), gr) for n, gr in gref.items()]
    e_fn = {n: float((a - b).norm() / float(b.norm())) for n, a, b in items if n.startswith("fc_norm.")}
    print("pooled head %r %s/masked: logits %.2e / %.2e, %d decisions differ (reference margin %.1e), losses %.1e, d fc_norm %s" %
          (pool, precision, es, et, flips, float(g["min_gate_margin"]), el, {k: "%.1e" % v for k, v in e_fn.items()}))
    assert es <= tol["logits"] and et <= tol["logits"] and flips <= tol["step_flips"] and el <= tol["loss"]
    worst = _judge_grads(precision, items)
    print("pooled head %r %s/masked: gradients %s" % (pool, precision, {k: "%.1e (%s)" % v for k, v in worst.items()}))
    if precision == "fp32":
        D.D_adamw(eng, float(g["meta_lr"]), float(g["meta_wd"]))
        keys = [k for k in g if k.startswith("param_after/")]
        assert len(keys) == 4
        for key in keys:
            n = key.split("/", 1)[1]
            got = eng.trainable_view(n, g[key].shape).cpu().numpy()
            gg = np.abs(g["grad/" + n])
            err = np.abs(got - g[key])
            assert err[gg > 1e-6].max(initial=0.0) < 2e-5 and err.max() < 0.1 * float(g["meta_lr"]), n
        # eval: forward_features returns the un-normalised tokens, forward_head pools, applies fc_norm and the head
        model.eval()
        with torch.no_grad():
            le, _ = model(x.cuda())
            oe, _ = PH.forward({k: p.detach().cpu() for k, p in model.state_dict().items()}, x, training=False, mode="compact", pool=pool)
        assert float((le.cpu() - oe).abs().max()) <= tol["logits"]
        feats, _ = model.forward_features(x.cuda())
        assert float((model.forward_head(feats) - le).abs().max()) < 2e-5
        pre = model.forward_head(feats, pre_logits=True)
        assert tuple(pre.shape) == (B, 768)
        w, b = model.head.weight.detach(), model.head.bias.detach()
        assert float((pre @ w.t() + b - le).abs().max()) < 2e-5
    del model, eng
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------------------
# B = 16, C = 100, r = 64 against pool_head_refs (compact mode)
# ------------------------------------------------------------------------------------------------------------------------------
_b16 = {}


def _b16_reference():
    """Both passes of one training step through tests/pool_head_refs.py, and the fp64 tie band: computed once, shared by the precisions."""
    if not _b16:
        B, C, r, seed = 16, 100, 64, 31
        x, y = synth.make_batch(B, C, seed=seed)
        g1, g2 = synth.make_noise(B, seed=seed + 1)
        keep = synth.make_dropout_masks(B, r, seed=seed + 2)
        sd = synth.make_state_dict(C, r, seed=0, kind="test", gate_bias=0.85, head_norm="fc_norm")
        with torch.no_grad():
            ls, tok = PH.forward(sd, x, g1[0], g2[0], keep[0], 0.1, False, True, "compact", "avg")
            lt, _ = PH.forward(sd, x, g1[1], g2[1], keep[1], 0.1, True, True, "compact", "avg")
        tl32 = tok["token_logits"][..., 0]
        z = ((tl32.permute(1, 0, 2) + g1[0] - g2[0]) / 5.0).abs()
        band = PR.tie_band(PH._oracle_sd(sd), x, g1[0], g2[0], keep[0], "compact", tl32)
        _b16.update(args=(B, C, r), data=(x, y, g1, g2, keep, sd), ref=(ls, lt, tok["token_select"], z, band))
    return _b16


@pytest.mark.parametrize("precision", ["fp32", "fp16x3q"])
def test_avg_pool_step_at_b16_vs_pool_head_refs(precision):
    from models.vision_transformer_IN21K import vit_base_patch16_224_in21k
    ref = _b16_reference()
    (B, C, r), (x, y, g1, g2, keep, sd), (ref_ls, ref_lt, ref_ts, z, band) = ref["args"], ref["data"], ref["ref"]
    model = vit_base_patch16_224_in21k(num_classes=C, drop_path_rate=0.0, tuning_config=_tuning(r), select_config=D.Cfg(open=True, keep_layers=0),
                                       precision=precision, train_mode="compact", global_pool="avg")
    model.load_state_dict(sd, strict=True)
    for n, p in model.named_parameters():
        p.requires_grad = synth.is_trainable(n)
    model = model.cuda().train()
    eng = model.engine(B, torch.device("cuda", 0))
    ls, lt = torch.empty(B, C, device="cuda"), torch.empty(B, C, device="cuda")
    ts = torch.zeros(B, 12, 196, device="cuda")
    eng.step_fwd_bwd(x.cuda(), y.cuda(), 0.5, 2.0, 0.0, 0.0, masked_dense=False, g1=g1.cuda().contiguous(), g2=g2.cuda().contiguous(),
                     keep_mask=keep.cuda().contiguous(), logits_s=ls, logits_t=lt, token_select=ts)
    flip = ts.cpu() != ref_ts[..., 0].float()
    nflip, outside, zmax, blk = PR.judge_decisions(flip, z.permute(1, 0, 2), band)
    es, et = float((ls.cpu() - ref_ls).abs().max()), float((lt.cpu() - ref_lt).abs().max())
    print("avg pool B=16 %s/compact: logits %.2e / %.2e, %d of %d decisions differ (first in block %d: largest margin %.1e, %d outside the tie band)" % (
        precision, es, et, nflip, flip.numel(), blk, zmax, outside))
    assert outside == 0, (precision, nflip, outside, zmax, blk)
    assert et <= 1e-3, et                      # the complete_model pass has no gate: always comparable
    if not nflip:                              # (a tie inside the band that went the other way changes the token set: parity_rules)
        assert es <= 1e-3, es
    assert bool(torch.isfinite(eng.grad).all()) and float(eng.trainable_view("fc_norm.weight", (768,), eng.grad).abs().max()) > 0
    del model, eng
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------------------
# context properties
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inputs():
    x, _ = synth.make_batch(23, 10, seed=SEED)
    g1, g2 = synth.make_noise(23, depth=2, seed=SEED + 1, passes=1)
    keep = synth.make_dropout_masks(23, RANK, depth=2, seed=SEED + 2, passes=1)
    x = x.cuda()

    def take(B, depth):
        return (x[:B].contiguous(), g1[0, :depth, :B].contiguous().cuda(), g2[0, :depth, :B].contiguous().cuda(),
                keep[0, :depth, :B * 197].contiguous().cuda())
    return take


def _sd(C, depth, seed=SEED):
    return synth.make_state_dict(C, RANK, seed=seed, kind="test", depth=depth, gate_bias=0.85, head_norm="fc_norm")


def _engine(C, depth, pool, sd, max_batch, precision="fp32", **kw):
    eng = DyTEngine(C, RANK, 0.1, DEV, precision=precision, max_batch=max_batch, depth=depth, avg_pool=(pool == "avg"), fc_norm=True, **kw)
    eng.load_state_dict(sd)
    return eng


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("pool", ["avg", "token"])
def test_inference_only_context_equals_the_training_layout_bit_for_bit(pool, precision, inputs):
    C, depth = 10, 2
    sd = _sd(C, depth)
    full = _engine(C, depth, pool, sd, 23, precision)
    inf = _engine(C, depth, pool, sd, 23, precision, inference=True)
    assert inf.bytes < full.bytes and inf.n_train == full.n_train
    for B in (16, 23):
        x = inputs(B, depth)[0]
        for complete in (False, True):
            a, ta, _ = full.forward(x, complete_model=complete, gate_always=True)
            b, tb, _ = inf.forward(x, complete_model=complete, gate_always=True)
            torch.cuda.synchronize()
            assert torch.equal(a, b) and torch.equal(ta, tb), (pool, precision, B, complete)
            assert bool(torch.isfinite(a).all())
    with pytest.raises(DyTError, match="inference_only"):
        inf.forward(inputs(3, depth)[0], save=True)


@pytest.mark.parametrize("pool", ["avg", "token"])
def test_wide_and_row_kernel_head_agree_under_the_fp64_rule(pool, inputs):
    """C = 1000: both head forms in one configuration, each within 4 floor + 4 ulp of pool_head_refs.head_ref on the tokens the block stack
    produced (the same bits in both contexts); logits, d fc_norm.*, d head.*."""
    C, depth, B = 1000, 1, 17
    sd = _sd(C, depth)
    x, g1, g2, keep = inputs(B, depth)
    kw = dict(training=True, g1=g1, g2=g2, keep_mask=keep)
    dl = torch.randn(B, C, generator=_gen(C, B, 5))
    out = {}
    for wide in (False, True):
        eng = _engine(C, depth, pool, sd, B, wide_head=wide)
        eng.set_option(_lib.OPT_CLS_TAIL, 0)   # ('token': both forms then run the same block launches as forward_features_tokens)
        tokens = eng.forward_features_tokens(x, **kw)[0]
        logits, ts, _ = eng.forward(x, slot=0, save=True, **kw)
        grad = torch.zeros(eng.n_train, device=DEV)
        eng.backward(0, dl.cuda(), grad)
        torch.cuda.synchronize()
        args = (tokens, sd["fc_norm.weight"], sd["fc_norm.bias"], sd["head.weight"], sd["head.bias"], dl, pool)
        r64, r32 = PH.head_ref(*args), PH.head_ref(*args, dtype=F32)
        name = "pooled head in a context (%s)" % ("wide" if wide else "rows")
        tag = "%s C=%d B=%d" % (pool, C, B)
        _cmp(name, tag + " logits", logits, r64[0], r32[0])
        for i, key in ((2, "fc_norm.weight"), (3, "fc_norm.bias"), (4, "head.weight"), (5, "head.bias")):
            _cmp(name, tag + " d " + key, eng.trainable_view(key, r64[i].shape, grad), r64[i], r32[i])
        out[wide] = (tokens, ts)
        del eng
    assert torch.equal(out[False][0], out[True][0]) and torch.equal(out[False][1], out[True][1])


def test_avg_pool_with_the_adapters_layernorm_step_vs_refs():
    """adapter_ln = "in" together with global_pool='avg' at depth 2: one fused fp32 step against pool_head_refs (oracle blocks with the
    adapter's LayerNorm): logits, losses, all gradients."""
    from models.vision_transformer_IN21K import VisionTransformer
    C, depth, B, seed = 10, 2, 3, 17
    sd = synth.add_adapter_layernorm(_sd(C, depth, seed=seed), seed=seed, depth=depth)
    x, y = synth.make_batch(B, C, seed=seed)
    g1, g2 = synth.make_noise(B, depth=depth, seed=seed + 1)
    keep = synth.make_dropout_masks(B, RANK, depth=depth, seed=seed + 2)
    sd_ref = dict(sd)
    sd_ref[O.ADAPTER_LN_KEY] = torch.tensor(1)
    d_ref, g_ref, (ref_ls, ref_lt, tok) = PH.step_grads(sd_ref, x, y, g1, g2, keep, scale=0.1, mode="masked", pool="avg", depth=depth)
    g_ref = {k: v for k, v in g_ref.items() if k != O.ADAPTER_LN_KEY}
    assert len(g_ref) == 8 * depth + 4
    m = VisionTransformer(patch_size=16, embed_dim=768, depth=depth, num_heads=12, mlp_ratio=4.0, qkv_bias=True, num_classes=C, drop_path_rate=0.0,
                          tuning_config=_tuning(RANK, "in"), select_config=D.Cfg(open=True, keep_layers=0), precision="fp32", train_mode="masked",
                          max_batch=B, global_pool="avg")
    m.load_state_dict(sd, strict=True)
    for n, p in m.named_parameters():
        p.requires_grad = synth.is_trainable(n)
    m = m.cuda().train()
    eng = m.engine(B, torch.device("cuda", 0))
    assert eng.adapter_ln == 1 and eng.avg_pool
    ls, lt = torch.empty(B, C, device="cuda"), torch.empty(B, C, device="cuda")
    ts = torch.zeros(B, depth, 196, device="cuda")
    losses = eng.step_fwd_bwd(x.cuda(), y.cuda(), 0.5, 2.0, 0.0, 0.0, masked_dense=True, g1=g1.cuda().contiguous(), g2=g2.cuda().contiguous(),
                              keep_mask=keep.cuda().contiguous(), logits_s=ls, logits_t=lt, token_select=ts).cpu()
    tol = D.TOL["fp32"]
    assert int((ts.cpu() != tok["token_select"].detach()[..., 0].float()).sum()) <= tol["step_flips"]
    assert float((ls.cpu() - ref_ls.detach()).abs().max()) <= tol["logits"] and float((lt.cpu() - ref_lt.detach()).abs().max()) <= tol["logits"]
    for i, k in enumerate(("loss", "base_loss", "token_loss", "teacher_loss", "distillation_loss")):
        assert abs(float(losses[i]) - float(d_ref[k])) <= tol["loss"] * max(1.0, abs(float(d_ref[k]))), k
    worst = _judge_grads("fp32", [(n, eng.trainable_view(n, gr.shape, eng.grad).cpu(), gr) for n, gr in g_ref.items()])
    print("avg pool + adapter LayerNorm 'in', depth 2: gradients %s" % {k: "%.1e (%s)" % v for k, v in worst.items()})


def test_flat_layout_grad_part_and_refusals(inputs):
    C, depth = 10, 2
    sd = _sd(C, depth)
    plain = DyTEngine(C, RANK, 0.1, DEV, precision="fp32", max_batch=3, depth=depth)
    L = plain.L
    off, num = ctypes.c_int64(), ctypes.c_int64()
    for pid in (_lib.P_FC_NORM_W, _lib.P_FC_NORM_B):   # the two ids exist only with the flag
        assert L.dyt_trainable_offset(plain.h, pid, 0, ctypes.byref(off), ctypes.byref(num)) == -1
        assert "DYT_CREATE_FC_NORM" in L.dyt_last_error().decode()
    for pool in ("avg", "token"):
        eng = _engine(C, depth, pool, sd, 3)
        # every other offset is what it is without the flag; the two [768] tensors sit directly behind head.bias, at the end of the buffer
        for k in sd:
            if synth.is_trainable(k) and not k.startswith("fc_norm."):
                assert eng.trainable_slice(k) == plain.trainable_slice(k), k
        hb, fw, fb = eng.trainable_slice("head.bias"), eng.trainable_slice("fc_norm.weight"), eng.trainable_slice("fc_norm.bias")
        assert fw == ((hb[0] + hb[1] + 3) // 4 * 4, 768) and fb == (fw[0] + 768, 768) and eng.n_train == fb[0] + 768 == plain.n_train + 1536
        p0, n0 = eng.grad_part(0)
        p1, n1 = eng.grad_part(1)
        assert p0 <= fw[0] and fb[0] + 768 <= p0 + n0 == eng.n_train and (p1, n1) == (0, p0)
        assert eng.bytes > plain.bytes
        # the final norm is an identity there: uploading it is refused, by name
        t = torch.ones(768, device=DEV)
        for pid in (_lib.P_NORM_W, _lib.P_NORM_B):
            assert L.dyt_set_frozen(eng.h, pid, 0, ptr(t), stream_ptr()) == -1
            assert "DYT_CREATE_FC_NORM" in L.dyt_last_error().decode()
        with pytest.raises(DyTError, match="DYT_CREATE_FC_NORM"):
            eng.set_param("norm.weight", t)
        if pool == "avg":   # the cls-only tail cannot be switched back on: every patch token reaches the head
            x, g1, g2, keep = inputs(3, depth)
            a, _, _ = eng.forward(x, training=True, g1=g1, g2=g2, keep_mask=keep)
            eng.set_option(_lib.OPT_CLS_TAIL, 1)
            b, _, _ = eng.forward(x, training=True, g1=g1, g2=g2, keep_mask=keep)
            assert torch.equal(a, b)
        del eng
    cfg = _lib.Config(C, RANK, 1, _lib.PREC_FP32, 4, 2, 0.1, 0.1, 5.0, 0.5, 2, 0, 0)   # frames = 2
    for flags, word in ((_lib.CREATE_FC_NORM, "DYT_CREATE_FC_NORM"), (_lib.CREATE_AVG_POOL | _lib.CREATE_FC_NORM, "DYT_CREATE_AVG_POOL")):
        h = ctypes.c_void_p()
        assert L.dyt_ctx_create_ex(ctypes.byref(cfg), flags, ctypes.byref(h)) == -1 and not h.value
        msg = L.dyt_last_error().decode()
        assert word in msg and "frames=2" in msg, msg
    with pytest.raises(DyTError, match="image model only"):
        DyTEngine(C, RANK, 0.1, DEV, precision="fp32", max_batch=4, depth=1, frames=2, avg_pool=True)
    cfg1 = _lib.Config(C, RANK, 1, _lib.PREC_FP32, 1, 2, 0.1, 0.1, 5.0, 0.5, 1, 0, 0)
    for flags in (8, 8 | _lib.CREATE_AVG_POOL, 0x80000000):
        h = ctypes.c_void_p()
        assert L.dyt_ctx_create_ex(ctypes.byref(cfg1), flags, ctypes.byref(h)) == -1 and not h.value
        assert "unknown create_flags" in L.dyt_last_error().decode()
    for flags in (_lib.CREATE_AVG_POOL, _lib.CREATE_AVG_POOL | _lib.CREATE_WIDE_HEAD):   # 'avg' without fc_norm: the refused configuration, by name
        h = ctypes.c_void_p()
        assert L.dyt_ctx_create_ex(ctypes.byref(cfg1), flags, ctypes.byref(h)) == -1 and not h.value
        msg = L.dyt_last_error().decode()
        assert "create_flags" in msg and "DYT_CREATE_AVG_POOL without DYT_CREATE_FC_NORM" in msg, msg
    for flags in (_lib.CREATE_FC_NORM, 5, 6, 7):   # every other combination of the known bits creates
        h = ctypes.c_void_p()
        assert L.dyt_ctx_create_ex(ctypes.byref(cfg1), flags, ctypes.byref(h)) == 0 and h.value
        n = ctypes.c_int64()
        assert L.dyt_trainable_numel(h, ctypes.byref(n)) == 0 and n.value > 1536
        assert L.dyt_ctx_destroy(h) == 0


def test_steps_are_bit_reproducible_with_avg_pool(inputs):
    """Two identical fp32 steps on the serial schedule: the same bits in logits and in every gradient (no atomics in the new kernels)."""
    C, depth, B = 10, 2, 5
    sd = _sd(C, depth)
    eng = _engine(C, depth, "avg", sd, B)
    eng.set_option(_lib.OPT_STREAM_OVERLAP, 0)
    x, g1, g2, keep = inputs(B, depth)
    y = torch.arange(B, device=DEV) % C
    runs = []
    for _ in range(2):
        ls = torch.empty(B, C, device=DEV)
        eng.step_fwd_bwd(x, y, 0.5, 2.0, 0.0, 0.0, masked_dense=True, g1=torch.stack([g1, g1]), g2=torch.stack([g2, g2]),
                         keep_mask=torch.stack([keep, keep]), logits_s=ls)
        torch.cuda.synchronize()
        runs.append((ls.clone(), eng.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert float(eng.trainable_view("fc_norm.bias", (768,), runs[0][1]).abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------------------------
# checkpoint round trip
# ------------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip_keeps_fc_norm_and_its_moments(tmp_path):
    import misc
    from engine_finetune import FusedAdamW, train_step
    from models.vision_transformer_IN21K import VisionTransformer
    C, depth, B = 10, 2, 4

    def build():
        m = VisionTransformer(patch_size=16, embed_dim=768, depth=depth, num_heads=12, mlp_ratio=4.0, qkv_bias=True, num_classes=C, drop_path_rate=0.0,
                              tuning_config=_tuning(RANK), select_config=D.Cfg(open=True, keep_layers=0), precision="fp16", train_mode="masked",
                              max_batch=B, global_pool="avg")
        for n, p in m.named_parameters():
            p.requires_grad = synth.is_trainable(n)
        return m.cuda()
    m = build()
    m.load_state_dict(_sd(C, depth), strict=True)
    m.train()
    opt = FusedAdamW(m, lr=1e-3, weight_decay=0.01)
    assert len(opt.param_groups[0]["params"]) == 6 * depth + 4
    x, y = synth.make_batch(B, C, seed=5)
    x, y = x.cuda(), y.cuda()
    for i in range(3):
        train_step(m, x, y, opt, seed=700 + i, target_ratio=0.5, token_minimal=0.0, token_minimal_weight=0.0)
    torch.cuda.synchronize()
    assert opt.applied_and_skipped() == (3, 0)
    before = _sd(C, depth)
    assert float((m.fc_norm.weight.detach().cpu() - before["fc_norm.weight"]).abs().max()) > 1e-4   # fc_norm trains
    args = types.SimpleNamespace(output_dir=str(tmp_path), epochs=4, save_freq=1, auto_remove=False, resume="", start_epoch=0, eval=False)
    misc.save_model(args=args, epoch=0, model=m, model_without_ddp=m, optimizer=opt, save_force=True)
    ck = torch.load(tmp_path / "checkpoint-0.pth", map_location="cpu", weights_only=False)
    names = [n for n, p in m.named_parameters() if p.requires_grad]
    assert "fc_norm.weight" in ck["model"] and "norm.weight" not in ck["model"] and len(ck["optimizer"]["state"]) == len(names) == 6 * depth + 4
    m2 = build()
    opt2 = FusedAdamW(m2, lr=5e-4, weight_decay=0.0)
    args.resume = str(tmp_path / "checkpoint-0.pth")
    misc.load_model(args=args, model_without_ddp=m2, optimizer=opt2)
    assert args.start_epoch == 1 and opt2.param_groups[0]["lr"] == 1e-3
    m2.train()
    m2.engine(B, torch.device("cuda", 0))
    sd1, sd2 = opt.state_dict(), opt2.state_dict()
    for key in ("fc_norm.weight", "fc_norm.bias", "head.bias"):
        i = names.index(key)
        assert torch.equal(dict(m.named_parameters())[key].detach(), dict(m2.named_parameters())[key].detach()), key
        assert float(sd1["state"][i]["exp_avg_sq"].abs().max()) > 0 and float(sd2["state"][i]["step"]) == 3.0
        assert torch.equal(sd1["state"][i]["exp_avg"], sd2["state"][i]["exp_avg"]) and torch.equal(sd1["state"][i]["exp_avg_sq"], sd2["state"][i]["exp_avg_sq"])
    # and the resumed run continues as the original does
    la = train_step(m, x, y, opt, seed=710, target_ratio=0.5, token_minimal=0.0, token_minimal_weight=0.0).clone()
    lb = train_step(m2, x, y, opt2, seed=710, target_ratio=0.5, token_minimal=0.0, token_minimal_weight=0.0).clone()
    torch.cuda.synchronize()
    assert torch.equal(la, lb) and torch.equal(m.fc_norm.weight.detach(), m2.fc_norm.weight.detach())
