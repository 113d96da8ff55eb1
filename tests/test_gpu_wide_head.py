"""GPU tests of the wide classification head (csrc/head_wide.hip, DYT_CREATE_WIDE_HEAD): the context-free unit entry dyt_head_wide on
both libraries, and the context path -- wide against row-kernel form, whole steps against the oracle, the loss above 1024 classes,
determinism and hipGraph replay, inference-only contexts, refusals, a short training run.

Bounds.  The rule of tests/test_gpu_step_tail.py, restated: for every compared tensor the same reference is evaluated in fp64 (the
reference) and in fp32 on the CPU; floor = max|fp32_cpu - fp64| is what plain fp32 arithmetic costs on these very inputs, and the kernel
must satisfy  max|gpu - fp64| <= 4 floor + 4 ulp(max|fp64|).  The 4 is that file's allowance for another summation order; for the logits
(contraction K = 768) and dW (K = B) it carries over unchanged.  The dx contraction is up to 21 843 classes long: the issue's CPU study of
a sequential fp32 chain per slice of 1024 classes, slices added in order, gave error / floor 2.4 / 1.6 / 1.4 (randn dlogits) and 1.5 / 1.3 / 2.1
(loss-gradient dlogits) at C = 1025 / 4099 / 21 843, slices of 256 below 1.1, and an unsliced chain 4.6 at C = 4099 and 11.0 at C = 21 843: hence
slices of at most 1024 classes, and the same factor 4.  head_wide_dx_kernel sums a slice as chains of 256 classes added to the slice's total
(one 1024-class chain measured 4.08 at C = 1025, B = 33 on the MI355X); head_wide_dx_finish_kernel adds the slices in ascending order.  A ratio above 4 is a finding
about the kernel's summation, not a reason to widen the bound.  Every case prints error / floor; the module prints the worst per kernel
(the table is in DESIGN.md 7h).

Whole-step bounds are those of tests/gpu_diag.py (TOL["fp32"]: logits 1e-3, losses 1e-4; report_grads' fp32 bar 2e-3 relative L2 for all 74
gradients), masks under the tie rule of tests/parity_rules.py.

Inputs of the unit entry: cls_x randn; head.weight, head.bias N(0, 0.02); the final norm's gamma 1 + N(0, 0.02), beta N(0, 0.02)."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _lib  # noqa: E402
import gpu_diag as D  # noqa: E402
import parity_rules as PR  # noqa: E402
import synth  # noqa: E402
import tail_refs as R  # noqa: E402
import wide_head_refs as WR  # noqa: E402
from _lib import DyTError, ptr, stream_ptr  # noqa: E402
from oracle import dyt_oracle as O  # noqa: E402
from runtime import DyTEngine  # noqa: E402

DEV = "cuda:0"
RANK, SEED = 8, 77
F32, F64 = torch.float32, torch.float64
GATE_KEY = "blocks.0.mlp_token_select.mlp_head.bias"
WORST = {}   # kernel -> (ratio, case)


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
# unit entry: dyt_head_wide on both libraries
# ------------------------------------------------------------------------------------------------------------------------------
CS = (1, 63, 64, 65, 129, 1023, 1024, 1025, 2049, 4099)
BS = (1, 3, 31, 33, 129)
UNIT_SHAPES = sorted({(B, C) for C in CS for B in (1, 33)} | {(B, C) for B in BS for C in (65, 1025, 2049)}) + [(2, 21843)]
KINDS = ("randn", "loss gradient", "single entry")
_unit_cache = {}


def _unit_inputs(B, C):
    """Inputs and the fp64 / fp32 references of one shape: computed once, shared by the two libraries' cases, never modified."""
    if (B, C) not in _unit_cache:
        g = _gen(B, C, 11)
        x = torch.randn(B, 768, generator=g)
        nw, nb = 1.0 + 0.02 * torch.randn(768, generator=g), 0.02 * torch.randn(768, generator=g)
        hw, hb = 0.02 * torch.randn(C, 768, generator=g), 0.02 * torch.randn(C, generator=g)
        y = torch.randint(0, C, (B,), generator=g)
        single = torch.zeros(B, C)
        single[B // 2, C // 2] = 1.5
        dls = {"randn": torch.randn(B, C, generator=g),
               "loss gradient": (torch.softmax(torch.randn(B, C, generator=g), dim=-1) - torch.nn.functional.one_hot(y, C).float()) / B,
               "single entry": single}
        pre = torch.randn(C, 768, generator=g)
        refs = {k: (WR.head_full_ref(x, nw, nb, hw, hb, dl), WR.head_full_ref(x, nw, nb, hw, hb, dl, dtype=F32)) for k, dl in dls.items()}
        _unit_cache[(B, C)] = (x, nw, nb, hw, hb, dls, pre, refs)
    return _unit_cache[(B, C)]


def _head_wide(L, dev, dl, dx, dW, db, B, C):
    x, nw, nb, hw, hb = dev
    logits = torch.full((B, C), float("nan"), device=DEV)
    _lib.check(L.dyt_head_wide(ptr(x), ptr(nw), ptr(nb), ptr(hw), ptr(hb), ptr(logits), ptr(dl), ptr(dx), ptr(dW), ptr(db), B, C, stream_ptr()), L)
    return logits


@pytest.mark.parametrize("fp16_lib", [False, True], ids=["libdyt_hip", "libdyt_hip_f16"])
@pytest.mark.parametrize("B,C", UNIT_SHAPES)
def test_head_wide_unit_entry_against_fp64(B, C, fp16_lib):
    L = _lib.lib(fp16=fp16_lib)
    x, nw, nb, hw, hb, dls, pre, refs = _unit_inputs(B, C)
    dev = tuple(t.cuda().contiguous() for t in (x, nw, nb, hw, hb))
    tag0 = "%s C=%d B=%d" % ("f16 lib" if fp16_lib else "lib", C, B)
    for kind in KINDS:
        dl = dls[kind].cuda().contiguous()
        r64, r32 = refs[kind]
        dx = torch.full((B, 768), float("nan"), device=DEV)
        dW, db = torch.zeros(C, 768, device=DEV), torch.zeros(C, device=DEV)
        logits = _head_wide(L, dev, dl, dx, dW, db, B, C)
        tag = "%s dlogits %s" % (tag0, kind)
        if kind == "randn":
            _cmp("head_wide_logits", tag + " logits", logits, r64[0], r32[0])
        _cmp("head_wide_dx", tag + " dx", dx, r64[1], r32[1])
        _cmp("head_wide_dw", tag + " d head.weight", dW, r64[2], r32[2])
        _cmp("head_wide_dw", tag + " d head.weight + d head.bias", torch.cat([dW.flatten(), db]).cpu(), torch.cat([r64[2].flatten(), r64[3]]),
             torch.cat([r32[2].flatten(), r32[3]]))
        if kind == "single entry":   # nothing leaks into another class's row or bias
            rest = torch.ones(C, dtype=torch.bool)
            rest[C // 2] = False
            dWc, dbc = dW.cpu(), db.cpu()
            assert float(dWc[rest].abs().max() if C > 1 else 0.0) == 0.0 and float(dbc[rest].abs().max() if C > 1 else 0.0) == 0.0
            assert float(dbc[C // 2]) == 1.5
        if kind != "randn":
            continue
        # the += contract: a pre-filled gradient comes back as itself plus dW
        dW2, db2 = pre.cuda().contiguous(), pre[:, 0].cuda().contiguous()
        dx2 = torch.full((B, 768), float("nan"), device=DEV)
        logits2 = _head_wide(L, dev, dl, dx2, dW2, db2, B, C)
        _cmp("head_wide_dw", tag + " pre-filled d head.weight", dW2, pre.double() + r64[2], pre + r32[2])
        _cmp("head_wide_dw", tag + " pre-filled d head.bias", db2, pre[:, 0].double() + r64[3], pre[:, 0] + r32[3])
        # two identical calls: the same bits in every output
        dx3 = torch.full((B, 768), float("nan"), device=DEV)
        dW3, db3 = torch.zeros(C, 768, device=DEV), torch.zeros(C, device=DEV)
        logits3 = _head_wide(L, dev, dl, dx3, dW3, db3, B, C)
        assert torch.equal(logits3, logits) and torch.equal(logits2, logits) and torch.equal(dx3, dx) and torch.equal(dx2, dx)
        assert torch.equal(dW3, dW) and torch.equal(db3, db)
        # forward only (dlogits NULL): no gradient is touched
        mark = [torch.full((B, 768), 7.0, device=DEV), torch.full((C, 768), 8.0, device=DEV), torch.full((C,), 9.0, device=DEV)]
        logits4 = _head_wide(L, dev, None, mark[0], mark[1], mark[2], B, C)
        assert torch.equal(logits4, logits)
        assert bool((mark[0] == 7.0).all()) and bool((mark[1] == 8.0).all()) and bool((mark[2] == 9.0).all())


# ------------------------------------------------------------------------------------------------------------------------------
# context path
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inputs():
    """Images, gate noise and adapter-dropout masks for up to 17 images at depth 1 (a batch of B takes the first B)."""
    x, _ = synth.make_batch(17, 10, seed=SEED)
    g1, g2 = synth.make_noise(17, depth=1, seed=SEED + 1, passes=1)
    keep = synth.make_dropout_masks(17, RANK, depth=1, seed=SEED + 2, passes=1)
    x = x.cuda()

    def take(B):
        return (x[:B].contiguous(), g1[0, :, :B].contiguous().cuda(), g2[0, :, :B].contiguous().cuda(),
                keep[0, :, :B * 197].contiguous().cuda())
    return take


@pytest.fixture(scope="module")
def engines():
    """Depth-1 contexts, one per (num_classes, max_batch, precision, wide, inference), on one set of synthetic weights."""
    base = synth.make_state_dict(1, RANK, seed=SEED, kind="test", depth=1, gate_bias=0.85)
    cache, sds = {}, {}

    def get(C, max_batch, wide, precision="fp32", inference=False):
        key = (C, max_batch, wide, precision, inference)
        if key not in cache:
            if C not in sds:
                sd = dict(base)
                sd["head.weight"] = synth._normal("head.weight", (C, 768), SEED, 0.02)
                sd["head.bias"] = synth._normal("head.bias", (C,), SEED, 0.02)
                sds[C] = sd
            eng = DyTEngine(C, RANK, 0.1, DEV, precision=precision, max_batch=max_batch, depth=1, wide_head=wide, inference=inference)
            assert eng.wide_head is bool(wide)
            eng.load_state_dict(sds[C])
            cache[key] = (eng, sds[C])
        return cache[key]
    yield get
    cache.clear()
    torch.cuda.empty_cache()


def _tokens_of_a_saving_pass(eng, x, g1, g2, keep):
    """forward_features_tokens with DYT_F_SAVE added.  In the 16-bit modes a saving forward is not the bits of a non-saving one (measured in the
    fp16 mode, C = 1000, B = 3, row-kernel head: logits 2.8e-5 from the reference on forward_features_tokens' output with DYT_F_SAVE, 3.4e-7
    without, whatever DYT_OPT_FC2_CAT and the masked mode are set to), so the reference's input has to come from a pass with the flags of the
    pass whose head is tested; in fp32 contexts the two are the same bits."""
    B = x.shape[0]
    flags = _lib.F_TRAINING | _lib.F_SAVE | _lib.F_GATE_ALWAYS | _lib.F_TOKENS_OUT
    out = torch.empty(B, 197, 768, device=DEV)
    ts, tl = torch.zeros(B, eng.depth, 196, device=DEV), torch.zeros(B, eng.depth, 196, device=DEV)
    eng._ck(eng.L.dyt_forward(eng.h, 0, ptr(x), B, flags, ptr(eng.flat), ptr(g1), ptr(g2), ptr(keep), ctypes.c_uint64(0), ptr(out), ptr(ts), ptr(tl),
                              stream_ptr()))
    return out


def _form_case(engines, inputs, C, B, precision):
    """The wide and the row-kernel head on the same weights, noise and masks: the block stack's outputs are the same bits, and the logits
    and the head's slice of the flat gradient of BOTH are within the bound of tail_refs.head_ref on forward_features_tokens' output
    (DYT_OPT_CLS_TAIL = 0: both passes then run the same launches, tests/test_gpu_step_tail.py; fp16: _tokens_of_a_saving_pass)."""
    x, g1, g2, keep = inputs(B)
    kw = dict(training=True, g1=g1, g2=g2, keep_mask=keep)
    dl = torch.randn(B, C, generator=_gen(C, B, 5))
    out = {}
    for wide in (False, True):
        eng, sd = engines(C, 17, wide, precision)
        eng.set_option(_lib.OPT_CLS_TAIL, 0)
        eng.set_param(GATE_KEY, torch.tensor([0.85]))
        tokens = eng.forward_features_tokens(x, **kw)[0] if precision == "fp32" else _tokens_of_a_saving_pass(eng, x, g1, g2, keep)
        logits, ts, tl = eng.forward(x, slot=0, save=True, **kw)
        grad = torch.zeros(eng.n_train, device=DEV)
        eng.backward(0, dl.cuda(), grad)
        torch.cuda.synchronize()
        ow, nw = eng.trainable_slice("head.weight")
        ob, nb = eng.trainable_slice("head.bias")
        assert nw == C * 768 and nb == C and ob + nb <= eng.n_train
        args = (tokens, sd["norm.weight"], sd["norm.bias"], sd["head.weight"], sd["head.bias"], dl)
        r64, r32 = R.head_ref(*args), R.head_ref(*args, dtype=F32)
        name = ("head_wide" if wide else "head (row kernels)") + " in a context"
        tag = "%s C=%d B=%d %s" % (precision, C, B, "wide" if wide else "rows")
        _cmp(name, tag + " logits", logits, r64[0], r32[0])
        dW, db = grad[ow:ow + nw].view(C, 768).cpu(), grad[ob:ob + nb].cpu()
        _cmp(name, tag + " d head.weight", dW, r64[1], r32[1])
        _cmp(name, tag + " d head.weight + d head.bias", torch.cat([dW.flatten(), db]), torch.cat([r64[1].flatten(), r64[2]]),
             torch.cat([r32[1].flatten(), r32[2]]))
        out[wide] = (tokens, ts, tl, grad)
    assert torch.equal(out[False][0], out[True][0])                                              # the head cannot touch the block stack ...
    assert torch.equal(out[False][1], out[True][1]) and torch.equal(out[False][2], out[True][2])   # ... nor token_select / token_logits


@pytest.mark.parametrize("C", [5, 1000])
@pytest.mark.parametrize("B", [3, 17])
def test_wide_and_row_kernel_head_side_by_side(C, B, engines, inputs):
    _form_case(engines, inputs, C, B, "fp32")


def test_wide_and_row_kernel_head_side_by_side_in_the_fp16_mode(engines, inputs):
    _form_case(engines, inputs, 1000, 3, "fp16")


def _model(C, depth, precision, B, mode="masked", sd=None, **kw):
    from models.vision_transformer_IN21K import VisionTransformer
    if sd is None:
        sd = synth.make_state_dict(C, RANK, seed=0, kind="test", depth=depth, gate_bias=0.85)
    tuning = D.Cfg(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option="none", ffn_adapter_init_option="lora",
                   ffn_adapter_scalar="0.1", ffn_num=RANK, d_model=768)
    m = VisionTransformer(patch_size=16, embed_dim=768, depth=depth, num_heads=12, mlp_ratio=4.0, qkv_bias=True, num_classes=C, drop_path_rate=0.0,
                          tuning_config=tuning, select_config=D.Cfg(open=True, keep_layers=0), precision=precision, train_mode=mode, max_batch=B, **kw)
    m.load_state_dict(sd, strict=True)
    for n, p in m.named_parameters():
        p.requires_grad = synth.is_trainable(n)
    return m.cuda(), sd


def _tie_band(sd, x, g1s, g2s, keeps, mode, tl32, depth, tau=5.0):
    """parity_rules.tie_band for a model of `depth` blocks (that function runs the 12-block oracle)."""
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        _, o64 = O.forward(sd64, x.double(), g1s.double(), g2s.double(), keeps, scale=0.1, training=True, mode=mode, depth=depth)
    tl64 = o64["token_logits"][..., 0]
    d = (tl32.double() - tl64).abs().amax(dim=(0, 2))
    z64 = (tl64 + (g1s - g2s).permute(1, 0, 2).double()) / tau
    z32 = (tl32.double() + (g1s - g2s).permute(1, 0, 2).double()) / tau
    split = ((z64 > 0) != (z32 > 0)).any(dim=2).any(dim=0)
    if bool(split.any()):
        first = int(split.nonzero()[0])
        d[first + 1:] = d[:first + 1].max()
    return PR.TIE_K * d / tau


@pytest.mark.parametrize("depth,B,cls_tail", [(12, 3, 1), (2, 2, 0)], ids=["depth12-B3", "depth2-B2-no-cls-tail"])
def test_whole_step_with_a_wide_head_against_the_oracle(depth, B, cls_tail):
    """num_classes = 1100 resolves to the wide head by itself.  cls_tail = 0 is the other stride of the head's dx (all 197 rows of an image,
    zero-filled): the gate and adapter gradients are what show a wrong dx."""
    C, mode, target, seed = 1100, "masked", 0.5, 31
    x, y = synth.make_batch(B, C, seed=seed)
    g1, g2 = synth.make_noise(B, depth=depth, seed=seed + 1)
    keep = synth.make_dropout_masks(B, RANK, depth=depth, seed=seed + 2)
    m, sd = _model(C, depth, "fp32", B, mode)
    assert m.wide_head is True
    d_ref, g_ref, (ref_ls, ref_lt, tok) = O.step_grads(sd, x, y, g1, g2, keep, scale=0.1, mode=mode, token_target_ratio=target, depth=depth)
    assert len(g_ref) == 6 * depth + 2
    ref_ls, ref_lt, ref_ts = ref_ls.detach(), ref_lt.detach(), tok["token_select"].detach()
    tl32 = tok["token_logits"].detach()[..., 0]
    z = ((tl32.permute(1, 0, 2) + g1[0] - g2[0]) / 5.0).abs()
    band = _tie_band(sd, x, g1[0], g2[0], keep[0], mode, tl32, depth)
    m.train()
    eng = m.engine(B, torch.device("cuda", 0))
    assert eng.wide_head is True and eng.num_classes == C
    eng.set_option(_lib.OPT_CLS_TAIL, cls_tail)
    ls, lt = torch.empty(B, C, device="cuda"), torch.empty(B, C, device="cuda")
    ts = torch.zeros(B, depth, 196, device="cuda")
    losses = eng.step_fwd_bwd(x.cuda(), y.cuda(), target, 2.0, 0.0, 0.0, masked_dense=True, g1=g1.cuda().contiguous(), g2=g2.cuda().contiguous(),
                              keep_mask=keep.cuda().contiguous(), logits_s=ls, logits_t=lt, token_select=ts).cpu()
    tol = D.TOL["fp32"]
    els, elt = float((ls.cpu() - ref_ls).abs().max()), float((lt.cpu() - ref_lt).abs().max())
    flip = ts.cpu() != ref_ts[..., 0].float()
    nflip, outside, zmax, blk = PR.judge_decisions(flip, z.permute(1, 0, 2), band)
    print("wide head step depth %d B=%d: logits %.2e / %.2e, %d of %d decisions differ (%d outside the tie band)" % (depth, B, els, elt, nflip, flip.numel(), outside))
    assert outside == 0, (nflip, outside, zmax, blk)
    assert nflip == 0, "a tie inside the reference's own band went the other way: choose another seed (%d decisions, block %d, margin %.1e)" % (nflip, blk, zmax)
    assert els <= tol["logits"] and elt <= tol["logits"], (els, elt)
    for i, k in enumerate(("loss", "base_loss", "token_loss", "teacher_loss", "distillation_loss")):
        ref = float(d_ref[k])
        assert abs(float(losses[i]) - ref) <= tol["loss"] * max(1.0, abs(ref)), (k, float(losses[i]), ref)
    n0 = len(D.RESULTS)
    D.report_grads("wide head fp32/%s depth %d" % (mode, depth), "fp32", [(n, eng.trainable_view(n, gr.shape, eng.grad).cpu(), gr, 1e-20) for n, gr in g_ref.items()])
    assert len(D.RESULTS) > n0 and all(ok for _, ok in D.RESULTS[n0:]), D.RESULTS[n0:]
    del D.RESULTS[n0:]


@pytest.mark.parametrize("C", [1025, 21843])
def test_loss_kernels_above_1024_classes(C, engines, inputs):
    """dyt_loss against tail_refs.loss_ref: the loss kernels' class loops were never run past 1024 classes."""
    B = 3
    eng, _ = engines(C, 3, True)
    eng.set_param(GATE_KEY, torch.tensor([0.85]))
    x, g1, g2, keep = inputs(B)
    eng.forward(x, slot=0, training=True, save=True, g1=g1, g2=g2, keep_mask=keep)
    counts = eng.debug_dispatch(0, 0, B)[2]
    torch.cuda.synchronize()
    counts = counts.cpu().view(1, B)
    g = _gen(C, B, 6)
    y = torch.randint(0, C, (B,), generator=g)
    target, ratio = 0.5, 2.0
    for kind, scale in (("randn", 1.0), ("randn x 30", 30.0)):
        s1, t1 = scale * torch.randn(B, C, generator=g), scale * torch.randn(B, C, generator=g)
        dls, dlt, losses, dtok = eng.loss(s1.cuda().contiguous(), t1.cuda().contiguous(), y.cuda(), target, ratio, 0.0, 0.0)
        torch.cuda.synchronize()
        r64 = R.loss_ref(s1, t1, y, counts, 1, target, ratio, 0.0, 0.0)
        r32 = R.loss_ref(s1, t1, y, counts, 1, target, ratio, 0.0, 0.0, dtype=F32)
        tag = "C=%d B=%d %s" % (C, B, kind)
        _cmp("loss_rows (C > 1024)", tag + " dlogits_s", dls, r64[1], r32[1])
        _cmp("loss_rows (C > 1024)", tag + " dlogits_t", dlt, r64[2], r32[2])
        _cmp("loss_final (C > 1024)", tag + " losses[0:5]", losses[:5], r64[0][:5], r32[0][:5])
        _cmp("loss_final (C > 1024)", tag + " dtok", dtok, r64[3], r32[3])


def test_step_is_bit_reproducible_and_replays_from_a_graph():
    from engine_finetune import FusedAdamW, train_step
    C, B = 1100, 5
    m, _ = _model(C, 2, "fp32", B)   # (two blocks: dyt_step_fwd_bwd sums the lower depth / 2 blocks' gradients in a launch of their own, empty at depth 1)
    m.train()
    eng = m.engine(B, torch.device("cuda", 0))
    assert eng.wide_head is True
    x, y = synth.make_batch(B, C, seed=61)
    x, y = x.cuda(), y.cuda()
    runs = []
    for _ in range(2):
        ls, lt = torch.empty(B, C, device="cuda"), torch.empty(B, C, device="cuda")
        losses = eng.step_fwd_bwd(x, y, 0.5, 2.0, 0.0, 0.0, masked_dense=True, seed=123, logits_s=ls, logits_t=lt).clone()
        torch.cuda.synchronize()
        runs.append((eng.grad.clone(), ls, lt, losses))
    for a, b in zip(*runs):
        assert torch.equal(a, b), float((a - b).abs().max())
    ow, nw = eng.trainable_slice("head.weight")
    assert float(runs[0][0][ow:ow + nw].abs().max()) > 0 and bool(torch.isfinite(runs[0][0]).all())
    opt = FusedAdamW(m, lr=1e-3, weight_decay=0.01)
    replays = [train_step(m, x, y, opt, seed=321, target_ratio=0.5, token_minimal=0.0, token_minimal_weight=0.0, graph=True, update=False).clone()
               for _ in range(2)]
    torch.cuda.synchronize()
    assert len(m._engine._graphs) == 1, "the step did not go through a captured graph"
    assert bool(torch.isfinite(replays[0][:5]).all()) and torch.equal(replays[0], replays[1]), (replays[0].tolist(), replays[1].tolist())


def test_inference_only_context_with_a_wide_head(engines, inputs):
    C, B = 1100, 3
    full, _ = engines(C, 3, True)
    inf, _ = engines(C, 3, True, inference=True)
    assert inf.wide_head and inf.inference and inf.bytes < full.bytes
    x, _, _, _ = inputs(B)
    a, _, _ = full.forward(x)
    b, _, _ = inf.forward(x)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    with pytest.raises(DyTError, match="inference_only"):
        inf.forward(x, slot=0, training=True, save=True)
    with pytest.raises(DyTError, match="inference_only"):
        inf.backward(0, torch.zeros(B, C, device=DEV), torch.zeros(inf.n_train, device=DEV))
    with pytest.raises(DyTError, match="inference_only"):
        inf.step_fwd_bwd(x, torch.zeros(B, dtype=torch.long, device=DEV))
    c, _, _ = inf.forward(x)
    torch.cuda.synchronize()
    assert torch.equal(b, c)


def test_refusals_leave_other_contexts_usable(engines, inputs):
    eng, _ = engines(5, 17, True)
    x, g1, g2, keep = inputs(3)
    eng.set_param(GATE_KEY, torch.tensor([0.85]))
    before, _, _ = eng.forward(x, training=True, g1=g1, g2=g2, keep_mask=keep)
    with pytest.raises(DyTError, match=r"num_classes=65537 \(1\.\.65536 with DYT_CREATE_WIDE_HEAD"):
        DyTEngine(65537, RANK, 0.1, DEV, precision="fp32", max_batch=1, depth=1, wide_head=True)
    with pytest.raises(DyTError, match="wide head: image model only"):
        DyTEngine(5, RANK, 0.1, DEV, precision="fp32", max_batch=8, depth=1, frames=8, wide_head=True)
    L = _lib.lib()
    cfg = _lib.Config(5, RANK, 1, _lib.PREC_FP32, 1, 2, 0.1, 0.1, 5.0, 0.5, 1, 0, 0)
    for flags in (2, 3, 0x80000000):
        h = ctypes.c_void_p()
        assert L.dyt_ctx_create_ex(ctypes.byref(cfg), flags, ctypes.byref(h)) == -1 and not h.value   # DYT_ERR_ARG
        assert "create_flags" in L.dyt_last_error().decode()
    with pytest.raises(DyTError, match=r"num_classes=1025 \(1\.\.1024\)"):
        DyTEngine(1025, RANK, 0.1, DEV, precision="fp32", max_batch=1, depth=1)
    after, _, _ = eng.forward(x, training=True, g1=g1, g2=g2, keep_mask=keep)
    torch.cuda.synchronize()
    assert torch.equal(before, after)


def test_a_wide_head_trains_in_the_default_fp16_mode():
    """40 fused steps on one repeated batch (library noise, guarded AdamW): finite losses, no skipped update, head.weight moves and the
    task loss falls."""
    from engine_finetune import FusedAdamW, train_step
    C, B = 1100, 4
    m, sd = _model(C, 2, None, B)
    assert m.wide_head is True and m.precision == _lib.PREC_FP16
    m.train()
    opt = FusedAdamW(m, lr=1e-3, weight_decay=0.01)
    x, y = synth.make_batch(B, C, seed=62)
    x, y = x.cuda(), y.cuda()
    hist = [train_step(m, x, y, opt, seed=900 + i, target_ratio=0.5, token_minimal=0.0, token_minimal_weight=0.0).clone() for i in range(40)]
    torch.cuda.synchronize()
    hist = torch.stack(hist).cpu()
    assert bool(torch.isfinite(hist[:, :5]).all()), hist[:, :5]
    assert opt.applied_and_skipped() == (40, 0)
    eng = m._engine
    assert eng.wide_head is True
    moved = (eng.trainable_view("head.weight", (C, 768)).cpu() - sd["head.weight"]).abs().max()
    assert float(moved) > 1e-4, float(moved)
    print("wide head training: task loss %.4f -> %.4f, head.weight moved by up to %.2e" % (float(hist[0, 1]), float(hist[-1, 1]), float(moved)))
    assert float(hist[-1, 1]) < float(hist[0, 1])
