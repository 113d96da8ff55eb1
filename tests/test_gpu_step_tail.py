"""Unit tests of the kernels that finish a step (csrc/step_tail.hip), each next to an fp64 reference (tests/tail_refs.py), through the C ABI:

  loss_rows_kernel / loss_final_kernel          dyt_loss after one saved student pass has filled the slot's token counts
  head_fwd_kernel / head_bwd_dw_kernel          dyt_forward / dyt_backward: logits, d head.weight, d head.bias
  adamw_kernel / adamw_guarded_kernel / grad_nonfinite_kernel     dyt_adamw, dyt_adamw_guarded on plain tensors
  sqsum_kernel / clip_scale_kernel              dyt_clip_grad_norm on a tensor of our own

These kernels are pure fp32, so no error number is written down here.  For every compared tensor the same tail_refs function is evaluated
in fp64 (the reference) and in fp32 on the CPU; floor = max|fp32_cpu - fp64| is what plain fp32 arithmetic costs on these very inputs, and
the kernel must satisfy  max|gpu - fp64| <= 4 floor + 4 ulp(max|fp64|)  (4: another summation order -- 64 strided lanes and a DPP tree
against torch's sums -- and device expf / logf / sqrtf within 1-2 ulp; the ulp term: the CPU's fp32 result may happen to be exact).
Named exactness properties are torch.equal.  Scalars have no floor worth the name (one draw of a rounding error), so the five loss values
are compared as the tensor they are returned in (and the three row sums base / teacher / KL once more as a tensor of their own), and
d head.bias together with d head.weight as the head's slice of the flat gradient, next to d head.weight alone.

Every case prints its error / floor ratio and the module prints the worst per kernel at its end.  The table (also DESIGN.md 7g):

  kernel(s)                        compared                     worst error / floor (one MI355X run)
  loss_rows                        dlogits_s, dlogits_t         8.54 (C=65 B=1, randn x 30, dlogits_s)
  loss_final                       losses, dtok                 112 (C=1000 B=5, student == teacher: floor 3e-9 on a loss of 15, error inside the 4-ulp term; otherwise <= 5.1)
  head_fwd                         logits                       1.68 (C=2 B=3)
  head_bwd_dw                      d head.weight, d head.bias   1.84 (C=1 B=17)
  adamw / adamw_guarded            p, m, v                      14.9 (numel 1, step 1000: one element, error inside the 4-ulp term)
  sqsum / clip_scale               norm, clipped gradient       5.95 (norm at numel 65537, inside the 4-ulp term); gradient 2.98

Not reachable from here: head_bwd_dx_kernel has no output of its own (its result is consumed by the block stack's backward); it stays
covered through the whole-step tests only.  head_bwd_dw's 1024-image LDS chunking needs B > 1024.  num_classes > 1024 is refused when the
context is created (dyt_ctx_create), so launch_head_bwd's own C > 1024 refusal cannot be reached through the ABI; the test checks the
refusal that can be, and that other contexts stay usable after it.
The head test runs with DYT_OPT_CLS_TAIL = 0: the token stream a DYT_F_TOKENS_OUT pass returns is computed for all rows, the saved pass's
cls-only tail evaluates the last block's MLP on the gathered cls rows; with the option off both passes run the same launches on the same
inputs and the reference's input is bit for bit what head_fwd_kernel read.

Contexts are depth 1, fp32, one per (num_classes, max_batch), shared by the tests of this module."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _lib  # noqa: E402
import synth  # noqa: E402
import tail_refs as R  # noqa: E402
from _lib import DyTError, ptr, stream_ptr  # noqa: E402
from runtime import DyTEngine  # noqa: E402

DEV = "cuda:0"
RANK, SEED = 8, 77
F32, F64 = torch.float32, torch.float64
GATE_KEY = "blocks.0.mlp_token_select.mlp_head.bias"
WORST = {}   # kernel -> (ratio, case)


def _cmp(kernel, what, gpu, ref64, ref32):
    """max|gpu - fp64| <= 4 max|fp32_cpu - fp64| + 4 ulp(max|fp64|); prints error / floor; returns the bound."""
    gpu, ref64, ref32 = gpu.detach().to("cpu", F64), ref64.detach().to(F64), ref32.detach().to("cpu", F64)
    assert gpu.shape == ref64.shape == ref32.shape, (what, gpu.shape, ref64.shape, ref32.shape)
    assert bool(torch.isfinite(ref64).all()) and bool(torch.isfinite(ref32).all()), "%s: the reference is not finite" % what
    err = float((gpu - ref64).abs().max()) if bool(torch.isfinite(gpu).all()) else math.inf
    floor = float((ref32 - ref64).abs().max())
    top = float(ref64.abs().max())
    assert top == 0.0 or top >= float(np.finfo(np.float32).tiny), "%s: the whole reference is subnormal in fp32 (%.3e): choose other inputs" % (what, top)
    bound = 4.0 * floor + 4.0 * R.ulp(ref64.abs().max())
    ratio = err / floor if floor > 0 else (0.0 if err == 0 else math.inf)
    print("[%s] %s: error %.3e floor %.3e error/floor %s bound %.3e" % (kernel, what, err, floor, "%.2f" % ratio if floor > 0 else ("-" if err == 0 else "inf"), bound))
    if math.isfinite(ratio) and ratio > WORST.get(kernel, (-1.0, ""))[0]:
        WORST[kernel] = (ratio, what)
    assert err <= bound, "[%s] %s: |gpu - fp64| = %.3e > 4 * %.3e + 4 ulp = %.3e" % (kernel, what, err, floor, bound)
    return bound


@pytest.fixture(scope="module", autouse=True)
def _worst_table():
    yield
    print("\nworst error / floor per kernel:")
    for k in sorted(WORST):
        print("  %-28s %8.2f   (%s)" % (k, WORST[k][0], WORST[k][1]))


@pytest.fixture(scope="module")
def inputs():
    """Images, gate noise and adapter-dropout masks for up to 257 images (drawn once; a batch of B takes the first B)."""
    x, _ = synth.make_batch(257, 10, seed=SEED)
    g1, g2 = synth.make_noise(257, depth=1, seed=SEED + 1, passes=1)
    keep = synth.make_dropout_masks(257, RANK, depth=1, seed=SEED + 2, passes=1)
    x = x.cuda()

    def take(B):
        return (x[:B].contiguous(), g1[0, :, :B].contiguous().cuda(), g2[0, :, :B].contiguous().cuda(),
                keep[0, :, :B * 197].contiguous().cuda())
    return take


@pytest.fixture(scope="module")
def engines():
    base = synth.make_state_dict(1, RANK, seed=SEED, kind="test", depth=1, gate_bias=0.85)
    cache = {}

    def get(C, max_batch):
        if (C, max_batch) not in cache:
            sd = dict(base)
            sd["head.weight"] = synth._normal("head.weight", (C, 768), SEED, 0.02)
            sd["head.bias"] = synth._normal("head.bias", (C,), SEED, 0.02)
            eng = DyTEngine(C, RANK, 0.1, DEV, precision="fp32", max_batch=max_batch, depth=1)
            eng.load_state_dict(sd)
            cache[(C, max_batch)] = (eng, sd)
        return cache[(C, max_batch)]
    yield get
    cache.clear()
    torch.cuda.empty_cache()


def _gen(*key):
    return torch.Generator().manual_seed(abs(hash(tuple(int(k) for k in key))) % (2 ** 31))


# ------------------------------------------------------------------------------------------------------------------------------
# loss
# ------------------------------------------------------------------------------------------------------------------------------
def _student_counts(eng, take, B, gate_bias):
    """One saved training student pass of B images with the gate bias set; returns the slot's kept-token counts [1, B] (CPU int32)."""
    eng.set_param(GATE_KEY, torch.tensor([float(gate_bias)]))
    x, g1, g2, keep = take(B)
    eng.forward(x, slot=0, training=True, save=True, g1=g1, g2=g2, keep_mask=keep)
    counts = eng.debug_dispatch(0, 0, B)[2]
    torch.cuda.synchronize()
    counts = counts.cpu().view(1, B)
    if gate_bias <= -60:
        assert bool((counts == 1).all()), "gate bias -60 must drop every patch token"
    if gate_bias >= 60:
        assert bool((counts == 197).all()), "gate bias +60 must keep every token"
    return counts


def _loss_case(eng, tag, ls, lt, y, counts, soft=None, token=(0.0, 0.0), ref_inputs=None):
    """dyt_loss on (ls, lt) against loss_ref; ``ref_inputs`` = (ls, lt, targets) the fp64 REFERENCE is evaluated on instead (an input
    that must give the same result in exact arithmetic: the unshifted logits, the integer labels of one-hot rows); the floor is always
    taken on the inputs the kernel saw.  Returns the GPU results."""
    B = ls.shape[0]
    tmin, tw = token
    target, ratio = 0.5, 2.0
    sdev = None if soft is None else soft.cuda().contiguous()
    eng.set_soft_targets(sdev)
    try:
        dls, dlt, losses, dtok = eng.loss(ls.cuda().contiguous(), lt.cuda().contiguous(), y.cuda(), target, ratio, tmin, tw)
        torch.cuda.synchronize()
    finally:
        eng.set_soft_targets(None)
    tg = y if soft is None else soft
    r32 = R.loss_ref(ls, lt, tg, counts, 1, target, ratio, tmin, tw, dtype=F32)
    r64 = R.loss_ref(ls, lt, tg, counts, 1, target, ratio, tmin, tw) if ref_inputs is None else \
        R.loss_ref(ref_inputs[0], ref_inputs[1], ref_inputs[2], counts, 1, target, ratio, tmin, tw)
    _cmp("loss_rows", tag + " dlogits_s", dls, r64[1], r32[1])
    _cmp("loss_rows", tag + " dlogits_t", dlt, r64[2], r32[2])
    _cmp("loss_final", tag + " losses[0:5]", losses[:5], r64[0][:5], r32[0][:5])
    rows = torch.tensor([1, 3, 4])
    _cmp("loss_final", tag + " base/teacher/kl", losses.cpu()[rows], r64[0][rows], r32[0][rows])
    _cmp("loss_final", tag + " dtok", dtok, r64[3], r32[3])
    lc = losses.cpu()
    total = float(lc[1].double() + lc[2].double() + lc[3].double() + lc[4].double())
    assert abs(float(lc[0]) - total) <= 4 * R.ulp(total), (tag, lc.tolist())
    kept = int(counts.sum()) - counts.numel()
    N = counts.numel() * 196
    assert float(lc[6]) == float(kept) and float(lc[5]) == float(np.float32(kept) / np.float32(N)) and float(lc[7]) == 0.0, (tag, lc.tolist(), kept, N)
    return dls, dlt, lc, dtok.cpu()


def _grid(base_shift):
    """Logits on the float32 grid of [8192, 16384) (multiples of 2^-10), so that adding +-1e4 is exact."""
    return (base_shift + 1.0e4) - 1.0e4


LOSS_SHAPES = [(C, 5) for C in (1, 2, 63, 64, 65, 397, 1000)] + [(65, B) for B in (1, 3, 4, 130, 257)]


@pytest.mark.parametrize("C,B", LOSS_SHAPES)
def test_loss_against_fp64_over_class_and_batch_loops(C, B, engines, inputs):
    """Every C at B = 5 (class loop: below, at and past 64 lanes, 1000) and every B at C = 65 (4 images per workgroup, 256 threads of
    the batch reduction: 257 needs a second trip); the three gate settings; every logit family."""
    eng, _ = engines(C, 5 if B <= 5 else 257)
    g = _gen(C, B, 1)
    y = torch.randint(0, C, (B,), generator=g)
    s1, t1 = torch.randn(B, C, generator=g), torch.randn(B, C, generator=g)
    for bias in (-60.0, 60.0, 0.85):
        counts = _student_counts(eng, inputs, B, bias)
        tag = "C=%d B=%d gate %+g" % (C, B, bias)
        _loss_case(eng, tag + " randn", s1, t1, y, counts)
    # (the slot now holds the gate-0.85 pass)
    _loss_case(eng, tag + " randn x 30", 30 * s1, 30 * t1, y, counts)
    sg, tgd = _grid(s1), _grid(t1)
    _loss_case(eng, tag + " grid", sg, tgd, y, counts)
    for shift in (1.0e4, -1.0e4):
        assert torch.equal((sg + shift) - shift, sg) and torch.equal((tgd + shift) - shift, tgd)
        _loss_case(eng, tag + " shift %+g" % shift, sg + shift, tgd + shift, y, counts)
        _loss_case(eng, tag + " shift %+g vs unshifted" % shift, sg + shift, tgd + shift, y, counts, ref_inputs=(sg, tgd, y))
    if C > 1:   # one class 90 above the rest, the label on another: CE ~ 90, every other probability underflows
        hot = (y + 1 + torch.randint(0, C - 1, (B,), generator=g)) % C
        assert bool((hot != y).all())
        sp, tp = s1.clone(), t1.clone()
        sp[torch.arange(B), hot] += 90.0
        _loss_case(eng, tag + " student peaked +90", sp, t1, y, counts)
        hot_t = (y + 1 + torch.randint(0, C - 1, (B,), generator=g)) % C   # the teacher's own peak, off the label too (on the label every
        assert bool((hot_t != y).all())                                     # entry of dlogits_t would be subnormal: nothing fp32 can measure)
        tp[torch.arange(B), hot_t] += 90.0
        _loss_case(eng, tag + " both peaked +90", sp, tp, y, counts)
        _loss_case(eng, tag + " teacher peaked +90", s1, tp, y, counts)
        st, tt = s1.clone(), t1.clone()   # exact ties at the maximum: on two classes, and on all
        st[:, 0] = st[:, C - 1] = 4.0
        tt[:, 0] = tt[:, C // 2] = 5.0
        _loss_case(eng, tag + " ties", st, tt, y, counts)
        _loss_case(eng, tag + " all equal", torch.full((B, C), 2.5), torch.full((B, C), -1.25), y, counts)
    dls, dlt, lc, _ = _loss_case(eng, tag + " student == teacher", s1, s1.clone(), y, counts)
    assert torch.equal(dls, dlt) and float(lc[1]) == float(lc[3])   # (KL <= the bound: its fp64 value is 0, checked above)


@pytest.mark.parametrize("B", [5, 130])
def test_loss_token_terms_and_dtok(B, engines, inputs):
    """token_minimal {0, 0.3, 1.5} x token_minimal_weight {0, 2} at each gate setting: the branches token_minimal > 0 and > 1 of the
    loss and all three dtok entries (uniform, extra for dropped, extra for kept), against autograd on the mask."""
    C = 65
    eng, _ = engines(C, 5 if B <= 5 else 257)
    g = _gen(B, 2)
    y = torch.randint(0, C, (B,), generator=g)
    s1, t1 = torch.randn(B, C, generator=g), torch.randn(B, C, generator=g)
    for bias in (-60.0, 60.0, 0.85):
        counts = _student_counts(eng, inputs, B, bias)
        for tmin in (0.0, 0.3, 1.5):
            for tw in (0.0, 2.0):
                _, _, _, dtok = _loss_case(eng, "B=%d gate %+g token_minimal %g weight %g" % (B, bias, tmin, tw), s1, t1, y, counts, token=(tmin, tw))
                if tw == 0.0:
                    assert float(dtok[1]) == 0.0 and float(dtok[2]) == 0.0
                else:   # exactly -ratio * weight where clamp(token_minimal - mask) passes a gradient (autograd: AT its bound too), else 0
                    assert float(dtok[1]) == -4.0 and float(dtok[2]) == (-4.0 if tmin >= 1.0 else 0.0)


@pytest.mark.parametrize("C", [2, 65, 397])
def test_loss_soft_targets(C, engines, inputs):
    """dyt_set_soft_targets: mixup rows, label smoothing, one-hot rows (= the integer-label path), rows summing to 0.5 and to 2 (the
    gradient is p sum(t) - t), exact zeros on classes whose probability underflows."""
    B = 5
    eng, _ = engines(C, 5)
    g = _gen(C, 3)
    y = torch.randint(0, C, (B,), generator=g)
    s1, t1 = torch.randn(B, C, generator=g), torch.randn(B, C, generator=g)
    counts = _student_counts(eng, inputs, B, 0.85)
    onehot = torch.zeros(B, C).scatter_(1, y.view(-1, 1), 1.0)
    smooth = onehot * 0.9 + 0.1 / C
    mix = 0.7 * smooth + 0.3 * smooth.flip(0)
    tag = "C=%d soft " % C
    _loss_case(eng, tag + "mixup", s1, t1, y, counts, soft=mix)
    _loss_case(eng, tag + "smoothing 0.1", s1, t1, y, counts, soft=smooth)
    _loss_case(eng, tag + "one-hot", s1, t1, y, counts, soft=onehot)
    _loss_case(eng, tag + "one-hot vs integer labels", s1, t1, y, counts, soft=onehot, ref_inputs=(s1, t1, y))
    _loss_case(eng, tag + "rows summing to 0.5", s1, t1, y, counts, soft=0.5 * mix)
    _loss_case(eng, tag + "rows summing to 2", s1, t1, y, counts, soft=2.0 * mix)
    hot = (y + 1) % C
    sp, tp = s1.clone(), t1.clone()
    sp[torch.arange(B), hot] += 90.0
    tp[torch.arange(B), hot] += 90.0
    sparse = torch.zeros(B, C)   # mass on the peaked class and on the label only: exact zeros wherever p underflows
    sparse[torch.arange(B), hot] += 0.75
    sparse[torch.arange(B), y] += 0.25
    _loss_case(eng, tag + "zeros where p underflows", sp, tp, y, counts, soft=sparse)
    _loss_case(eng, tag + "randn x 30", 30 * s1, 30 * t1, y, counts, soft=mix)


# ------------------------------------------------------------------------------------------------------------------------------
# head
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2, 5, 63, 65, 397, 1000, 1024])
def test_head_forward_and_weight_gradients(C, engines, inputs):
    eng, sd = engines(C, 17)
    eng.set_option(_lib.OPT_CLS_TAIL, 0)   # (module docstring: both passes then run the same launches)
    eng.set_param(GATE_KEY, torch.tensor([0.85]))
    ow, nw = eng.trainable_slice("head.weight")
    ob, nb = eng.trainable_slice("head.bias")
    assert nw == C * 768 and nb == C
    hw, hb = eng.flat[ow:ow + nw].view(C, 768), eng.flat[ob:ob + nb]
    assert torch.equal(hw.cpu(), sd["head.weight"]) and torch.equal(hb.cpu(), sd["head.bias"])
    for B in (1, 3, 8, 9, 17):   # 8 / 9: head_bwd_dw's unroll by 8 and its scalar tail
        x, g1, g2, keep = inputs(B)
        kw = dict(training=True, g1=g1, g2=g2, keep_mask=keep)
        tokens, _, _ = eng.forward_features_tokens(x, **kw)
        g = _gen(C, B, 4)
        dl_randn = torch.randn(B, C, generator=g)
        single = torch.zeros(B, C)
        single[B // 2, C // 2] = 1.5
        for kind, dl in (("randn", dl_randn), ("randn x 1e4", 1.0e4 * dl_randn), ("single entry", single)):
            logits, _, _ = eng.forward(x, slot=0, save=True, **kw)
            grad = torch.zeros(eng.n_train, device=DEV)
            eng.backward(0, dl.cuda(), grad)
            torch.cuda.synchronize()
            args = (tokens, sd["norm.weight"], sd["norm.bias"], sd["head.weight"], sd["head.bias"], dl)
            l64, w64, b64 = R.head_ref(*args)
            l32, w32, b32 = R.head_ref(*args, dtype=F32)
            tag = "C=%d B=%d dlogits %s" % (C, B, kind)
            if kind == "randn":
                _cmp("head_fwd", tag + " logits", logits, l64, l32)
            dW, db = grad[ow:ow + nw].view(C, 768).cpu(), grad[ob:ob + nb].cpu()
            _cmp("head_bwd_dw", tag + " d head.weight", dW, w64, w32)
            _cmp("head_bwd_dw", tag + " d head.weight + d head.bias", torch.cat([dW.flatten(), db]), torch.cat([w64.flatten(), b64]),
                 torch.cat([w32.flatten(), b32]))
            if kind == "single entry":   # nothing leaks into another class's row or bias
                rest = torch.ones(C, dtype=torch.bool)
                rest[C // 2] = False
                assert float(dW[rest].abs().max() if C > 1 else 0.0) == 0.0 and float(db[rest].abs().max() if C > 1 else 0.0) == 0.0
                assert float(db[C // 2]) == 1.5


def test_more_than_1024_classes_is_refused_and_other_contexts_stay_usable(engines, inputs):
    eng, _ = engines(5, 17)
    x, g1, g2, keep = inputs(3)
    before, _, _ = eng.forward(x, training=True, g1=g1, g2=g2, keep_mask=keep)
    with pytest.raises(DyTError, match=r"num_classes=1025 \(1\.\.1024\)"):
        DyTEngine(1025, RANK, 0.1, DEV, precision="fp32", max_batch=1, depth=1)
    after, _, _ = eng.forward(x, training=True, g1=g1, g2=g2, keep_mask=keep)
    torch.cuda.synchronize()
    assert torch.equal(before, after)


# ------------------------------------------------------------------------------------------------------------------------------
# AdamW
# ------------------------------------------------------------------------------------------------------------------------------
NUMELS = [1, 255, 256, 257, 65537, 1200003]


def _adamw_inputs(n, seed, with_moments):
    """p = 0.02 randn with every third entry exactly 0; g = randn 10^u, u uniform in [-9, 2]; every seventh entry (from index 3) has
    g = m = v = 0.  Moments (later steps): m of the gradient's size, v of its square."""
    g = _gen(n, seed)
    idx = torch.arange(n)
    p = 0.02 * torch.randn(n, generator=g)
    p[idx % 3 == 0] = 0.0
    scale = 10.0 ** torch.empty(n).uniform_(-9.0, 2.0, generator=g)
    grad = torch.randn(n, generator=g) * scale
    if with_moments:
        m = 0.5 * torch.randn(n, generator=g) * scale
        v = (0.5 + torch.rand(n, generator=g)) * scale * scale
    else:
        m, v = torch.zeros(n), torch.zeros(n)
    still = idx % 7 == 3
    grad[still] = 0.0
    m[still] = 0.0
    v[still] = 0.0
    return p, grad, m, v, still


def _adamw_call(p, g, m, v, step, lr, b1, b2, eps, wd, gs):
    L = _lib.lib()
    _lib.check(L.dyt_adamw(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), int(step), lr, b1, b2, eps, wd, gs, stream_ptr()))


def _guarded_call(p, g, m, v, state, lr, b1, b2, eps, wd, gs):
    L = _lib.lib()
    _lib.check(L.dyt_adamw_guarded(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), ptr(state), lr, b1, b2, eps, wd, gs, stream_ptr()))


def _cmp_adamw(tag, got, r64, r32, zero_p):
    """p, m, v; the entries whose parameter was exactly 0 before the update as a tensor of their own, so that they are measured relative
    to the update (it IS the parameter there) and not to the largest parameter."""
    for name, a, b, c in zip(("p", "m", "v"), got, r64, r32):
        _cmp("adamw", "%s %s" % (tag, name), a, b, c)
    if bool(zero_p.any()):
        _cmp("adamw", "%s p where it was 0" % tag, got[0].cpu()[zero_p], r64[0][zero_p], r32[0][zero_p])


@pytest.mark.parametrize("n", NUMELS)
def test_adamw_single_updates_against_fp64(n):
    lr, b1, b2 = 1e-3, 0.9, 0.999
    combos = [(wd, gs, eps) for wd in (0.0, 0.05) for gs in (1.0, 0.125) for eps in (1e-8, 1e-3)]
    if n > 65537:
        combos = [combos[0], combos[-1], combos[3], combos[4]]
    for step in (1, 2, 3, 10, 1000):
        p0, g0, m0, v0, still = _adamw_inputs(n, step, with_moments=step > 1)
        zero_p = p0 == 0
        for wd, gs, eps in combos:
            dev = [t.clone().cuda() for t in (p0, g0, m0, v0)]
            _adamw_call(*dev, step, lr, b1, b2, eps, wd, gs)
            gd = [t.clone().cuda() for t in (p0, g0, m0, v0)]
            state = torch.tensor([step - 1, 0, 0, 0], dtype=torch.int32, device=DEV)
            _guarded_call(*gd, state, lr, b1, b2, eps, wd, gs)
            torch.cuda.synchronize()
            args = (p0, g0, m0, v0, step, lr, b1, b2, eps, wd, gs)
            r64, r32 = R.adamw_ref(*args), R.adamw_ref(*args, dtype=F32)
            tag = "n=%d step %d wd %g grad_scale %g eps %g" % (n, step, wd, gs, eps)
            _cmp_adamw(tag, (dev[0], dev[2], dev[3]), r64, r32, zero_p)
            # the guarded form with state[0] = step - 1 is the same update bit for bit, and counts it
            assert torch.equal(gd[0], dev[0]) and torch.equal(gd[2], dev[2]) and torch.equal(gd[3], dev[3]), tag
            assert state.cpu().tolist()[:3] == [step, 0, 0], tag
            assert torch.equal(dev[1].cpu(), g0), "the gradient is read only"
            if bool(still.any()):   # g = m = v = 0: the moments stay 0 and the parameter sees the decay alone (none at wd = 0)
                pn, mn, vn = dev[0].cpu()[still], dev[2].cpu()[still], dev[3].cpu()[still]
                assert float(mn.abs().max()) == 0.0 and float(vn.abs().max()) == 0.0, tag
                assert torch.equal(pn[p0[still] == 0], torch.zeros(int((p0[still] == 0).sum()))), tag
                if wd == 0.0:
                    assert torch.equal(pn, p0[still]), tag


def test_adamw_twenty_step_trajectory():
    """The kernel carries its own fp32 state through 20 updates with a gradient that changes every step; the fp64 and the fp32 CPU
    reference carry theirs."""
    n, lr, b1, b2, eps, wd, gs = 65537, 1e-3, 0.9, 0.999, 1e-8, 0.05, 0.125
    p0, _, _, _, _ = _adamw_inputs(n, 99, False)
    zero_p = p0 == 0
    g = _gen(n, 100)
    scale = 10.0 ** torch.empty(n).uniform_(-9.0, 2.0, generator=g)
    dev = [p0.clone().cuda(), None, torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]
    s64 = (p0.double(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64))
    s32 = (p0.clone(), torch.zeros(n), torch.zeros(n))
    for step in range(1, 21):
        grad = torch.randn(n, generator=g) * scale * (1.0 + 0.5 * math.sin(step))
        dev[1] = grad.cuda()
        _adamw_call(*dev, step, lr, b1, b2, eps, wd, gs)
        s64 = R.adamw_ref(s64[0], grad, s64[1], s64[2], step, lr, b1, b2, eps, wd, gs)
        s32 = R.adamw_ref(s32[0], grad, s32[1], s32[2], step, lr, b1, b2, eps, wd, gs, dtype=F32)
    torch.cuda.synchronize()
    _cmp_adamw("20 steps n=%d" % n, (dev[0], dev[2], dev[3]), s64, s32, zero_p)


@pytest.mark.parametrize("where,value", [(0, math.inf), (-1, -math.inf), (70000, math.nan)])
def test_guarded_adamw_skips_a_non_finite_gradient(where, value):
    """+inf at index 0, -inf at the last index, NaN at index 70000 (past grad_nonfinite_kernel's first grid-stride pass of 256 x 256
    elements), each alone: p, m, v stay bit-identical, state = {applied, skipped + 1, 1, _}; the next finite call applies with the
    unchanged step count."""
    n, lr, b1, b2, eps, wd, gs = 1200003, 1e-3, 0.9, 0.999, 1e-8, 0.05, 1.0
    p0, g0, m0, v0, _ = _adamw_inputs(n, 5, True)
    bad = g0.clone()
    bad[where] = value
    dev = [t.clone().cuda() for t in (p0, bad, m0, v0)]
    state = torch.tensor([4, 2, 0, 0], dtype=torch.int32, device=DEV)
    _guarded_call(*dev, state, lr, b1, b2, eps, wd, gs)
    torch.cuda.synchronize()
    assert torch.equal(dev[0].cpu(), p0) and torch.equal(dev[2].cpu(), m0) and torch.equal(dev[3].cpu(), v0)
    assert state.cpu().tolist()[:3] == [4, 3, 1]
    dev[1] = g0.clone().cuda()
    _guarded_call(*dev, state, lr, b1, b2, eps, wd, gs)
    plain = [t.clone().cuda() for t in (p0, g0, m0, v0)]
    _adamw_call(*plain, 5, lr, b1, b2, eps, wd, gs)
    torch.cuda.synchronize()
    assert state.cpu().tolist()[:3] == [5, 3, 0]
    assert torch.equal(dev[0], plain[0]) and torch.equal(dev[2], plain[2]) and torch.equal(dev[3], plain[3])


# ------------------------------------------------------------------------------------------------------------------------------
# clipping
# ------------------------------------------------------------------------------------------------------------------------------
def _clip_call(eng, g, max_norm, pre_scale, norm_out):
    eng._ck(eng.L.dyt_clip_grad_norm(eng.h, ptr(g), g.numel(), float(max_norm), float(pre_scale), ptr(norm_out), stream_ptr()))


@pytest.mark.parametrize("n", NUMELS)
def test_clip_grad_norm_against_fp64(n, engines):
    eng, _ = engines(2, 5)
    g0 = torch.randn(n, generator=_gen(n, 6))
    norm1 = float(g0.double().norm())
    cases = [("below max_norm", 2.0 * norm1, 1.0), ("3x above", norm1 / 3.0, 1.0), ("1e4x above", norm1 / 1.0e4, 1.0),
             ("3x above, pre_scale 0.125", 0.125 * norm1 / 3.0, 0.125), ("3x above, pre_scale -0.5", 0.5 * norm1 / 3.0, -0.5),
             ("below, pre_scale -0.5", norm1, -0.5)]
    for name, max_norm, pre in cases:
        g = g0.clone().cuda()
        out = torch.full((1,), -1.0, device=DEV)
        _clip_call(eng, g, max_norm, pre, out)
        torch.cuda.synchronize()
        (n64, c64), (n32, c32) = R.clip_ref(g0, max_norm, pre), R.clip_ref(g0, max_norm, pre, dtype=F32)
        tag = "n=%d %s" % (n, name)
        _cmp("clip", tag + " norm", out[0], n64, n32)
        if name.startswith("below"):
            assert torch.equal(g.cpu(), g0), tag + ": a gradient inside the ball is not touched"
        else:
            assert float(c64.abs().max()) < float(g0.abs().max())
            _cmp("clip", tag + " gradient", g, c64, c32)
    g = g0.clone().cuda()   # norm_out = NULL: the same clipped gradient
    _clip_call(eng, g, norm1 / 3.0, 1.0, None)
    h = g0.clone().cuda()
    _clip_call(eng, h, norm1 / 3.0, 1.0, torch.empty(1, device=DEV))
    z = torch.zeros(n, device=DEV)   # all-zero gradient: unchanged, norm 0
    zn = torch.full((1,), -1.0, device=DEV)
    _clip_call(eng, z, 1.0, 1.0, zn)
    torch.cuda.synchronize()
    assert torch.equal(g, h) and float(zn[0]) == 0.0 and float(z.abs().max()) == 0.0
