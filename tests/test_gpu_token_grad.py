"""GPU tests of the token-level training route: dyt_forward_taps / dyt_backward_tokens (DyTEngine.forward_features_tokens(save=, taps=),
DyTEngine.backward_tokens), the tapped ln_bwd instantiations alone (dyt_unit_ln_bwd_tap) and VisionTransformer.forward_features with
grad and out_indices.  The reference is tests/token_grad_refs.py (pinned on the CPU by tests/test_token_grad_host.py).

Shapes: B = 2 (394 rows, no multiple of ln_bwd's 4 rows per workgroup) and B = 3 (591); engine-level contexts at depth 3 with taps {0, 2}
or {1}; module-level tests at the real depth 12, B = 2, taps (3, 5, 7, 11).

Bars of the whole-backward comparisons (per-tensor relative L2 against the fp32 oracle, tests/gpu_diag.py): 2e-3 in fp32, TOL[prec]["grad"]
in the split modes, FP16_ / BF16_GRAD_TOL_SMALL_B by tensor class in the 16-bit modes; the gate-bias gradients (one number per block, a
cancelling sum) are judged as one vector over the blocks outside fp32, as gpu_diag.report_grads does.  No row of a down_proj gradient is
set aside (the ReLU-side rule of tests/parity_rules.py is not invoked: stricter).  Token decisions: the draws are chosen so that the fp32
and the fp64 oracle decide alike and every reference margin lies outside four times parity_rules' tie band (asserted before the launch);
in fp32 and fp16x3q any differing decision fails the test.  In the 16-bit modes a decision may differ (gpu_diag.TOL[...]["step_flips"]
of them); the gradients of such a pass are consequences of another token set and are then not compared -- printed, so that it shows.

The tapped kernel (test 2): dx / dmask_next under test_gpu_step_tail._cmp's rule (max|gpu - fp64| <= 4 max|fp32_cpu - fp64| + 4 ulp(max|fp64|))
with the reference extended by the one add, PLUS half an ulp of max|sum| for that add's own rounding: the fp32 CPU floor already contains
one rounding of the add, the kernel's is a second, independent one of at most ulp(max|d + tap|) / 2.  g_at next to dx: bit for bit (one
rounding of the same register); g_at alone (base_at form): test_gpu_row_bwd._cmp16's allowance plus the same half ulp; out3: the split
check against the dx of the same launch, unchanged."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import _lib  # noqa: E402
import gpu_diag as D  # noqa: E402
import parity_rules as PR  # noqa: E402
import synth  # noqa: E402
import token_grad_refs as TG  # noqa: E402
from _lib import DyTError, ptr, stream_ptr  # noqa: E402
from oracle import dyt_oracle as O  # noqa: E402
from runtime import DyTEngine  # noqa: E402
from tail_refs import ulp  # noqa: E402

DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
C, RANK, DEPTH = 10, 8, 3
NT, DIM = 197, 768
SEED = 31


# ------------------------------------------------------------------------------------------------------------------------------
# shared inputs and references (computed once, never modified)
# ------------------------------------------------------------------------------------------------------------------------------
_cache = {}


def _once(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _sd(depth=DEPTH, variant="plain"):
    def make():
        sd = synth.make_state_dict(C, RANK, seed=SEED, kind="test", depth=depth, gate_bias=0.85, head_norm="fc_norm" if variant == "fc_norm" else "norm")
        if variant == "scale":
            sd = synth.add_learnable_scales(dict(sd), seed=SEED, depth=depth)
        if variant == "ln_in":
            sd = synth.add_adapter_layernorm(sd, seed=SEED, depth=depth)
        return sd
    return _once(("sd", depth, variant), make)


def _inputs(B, depth=DEPTH, rank=RANK):
    """(x, (g1, g2, keep)) on the CPU: [B,3,224,224], [depth,B,196] x 2, [depth,B*197,r] uint8."""
    def make():
        x, _ = synth.make_batch(B, C, seed=SEED)
        g1, g2 = synth.make_noise(B, depth=depth, seed=SEED + 1, passes=1)
        keep = synth.make_dropout_masks(B, rank, depth=depth, seed=SEED + 2, passes=1)
        return x, (g1[0].contiguous(), g2[0].contiguous(), keep[0].contiguous())
    return _once(("in", B, depth, rank), make)


def _dev_draws(draws):
    return dict(g1=draws[0].cuda(), g2=draws[1].cuda(), keep_mask=draws[2].cuda())


def _engine(prec, depth=DEPTH, B=3, variant="plain", **kw):
    sd = _sd(depth, variant)
    scale = torch.ones(1) if variant == "scale" else 0.1
    eng = DyTEngine(C, RANK, scale, DEV, precision=prec, max_batch=B, depth=depth, fc_norm=(variant == "fc_norm"),
                    adapter_ln=1 if variant == "ln_in" else 0, **kw)
    eng.load_state_dict(sd)
    return eng


def _oracle_sd(variant, depth=DEPTH):
    sd = dict(_sd(depth, variant))
    if variant == "ln_in":
        sd[O.ADAPTER_LN_KEY] = torch.tensor(1)
    if variant == "fc_norm":   # the functional's tokens are the raw last-block tokens (final_norm=False); the oracle's own head still names norm.*
        sd["norm.weight"], sd["norm.bias"] = sd["fc_norm.weight"], sd["fc_norm.bias"]
    return sd


FUNCTIONALS = {"a": dict(tokens=True, taps=(), gates=False), "b": dict(tokens=False, taps=(1,), gates=False),
               "c": dict(tokens=False, taps=(DEPTH - 1,), gates=False), "d": dict(tokens=True, taps=(0, 2), gates=True)}


def _R(B, which, depth=DEPTH):
    return _once(("R", B, which, depth), lambda: TG.unit_R(torch.Generator().manual_seed(SEED + 7), B, depth, **FUNCTIONALS[which]))


def _reference(B, mode, complete, which, variant="plain", drop_scales=None):
    """fp32 oracle gradients of the functional + its outputs; for the student passes also the tie band and the margins."""
    def make():
        sd, (x, draws) = _oracle_sd(variant), _inputs(B)
        R = _R(B, which)
        if complete:   # a complete_model pass has no gate gradient in the library (its mask is not applied): the functional leaves the gate outputs out
            R = (R[0], R[1], None, None)
        kw = dict(depth=DEPTH, mode=mode, complete_model=complete, final_norm=(variant != "fc_norm"), drop_scales=drop_scales)
        if variant == "scale":
            kw["scale"] = 1.0   # (read from the state dict's adaptmlp.scale)
        g32, o32 = TG.tap_loss_grads(sd, x, draws, *R, dtype=F32, **kw)
        with torch.no_grad():
            sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
            _, o64 = TG.tap_functional(sd64, x.double(), (draws[0].double(), draws[1].double(), draws[2]), **kw)
        tl32, tl64 = o32["token_logits"].double(), o64["token_logits"]
        noise = (draws[0] - draws[1]).permute(1, 0, 2).double()
        z32, z64 = (tl32 + noise) / 5.0, (tl64 + noise) / 5.0
        band = PR.TIE_K * (tl32 - tl64).abs().amax(dim=(0, 2)) / 5.0   # parity_rules.tie_band's rule at this depth
        return dict(R=R, g=g32, o=o32, z=z32.abs(), band=band, same=bool(((z32 > 0) == (z64 > 0)).all()))
    return _once(("ref", B, mode, complete, which, variant, drop_scales is not None), make)


def _assert_margins(ref):
    """The chosen draws: fp32 and fp64 oracle decide alike, every margin outside four times the band."""
    assert ref["same"], "fp32 and fp64 oracle decide differently: choose other seeds"
    assert bool((ref["z"] > 4.0 * ref["band"].view(1, -1, 1)).all()), "a reference margin lies inside four times the tie band: choose other seeds"


def _bar(prec, name):
    if prec == "fp32":
        return 2e-3
    if prec in D.SPLIT_MODES:
        return D.TOL[prec]["grad"]
    return (D.FP16_GRAD_TOL_SMALL_B if prec == "fp16" else D.BF16_GRAD_TOL_SMALL_B)[D.grad_kind(name)]


WORST = {}


def _judge(tag, prec, eng, gbuf, gref, bar_factor=1.0):
    """Per-tensor relative L2 under the mode's bar; outside fp32 the scalar gate-bias gradients are one vector over the blocks."""
    items, scal = [], []
    for n, r in gref.items():
        got = eng.trainable_view(n, r.shape, gbuf).cpu()
        if float(r.norm()) == 0.0:
            assert float(got.abs().max()) == 0.0, (tag, n, "the reference gradient is zero, the library's is not")
            continue
        (scal if (r.numel() == 1 and prec != "fp32") else items).append((n, got, r))
    if scal:
        items.append(("mlp_token_select.mlp_head.bias (all blocks)", torch.cat([g.reshape(-1) for _, g, _ in scal]), torch.cat([r.reshape(-1) for _, _, r in scal])))
    assert items
    for n, got, r in items:
        e = float((got - r).norm() / r.norm())
        k = (prec, D.grad_kind(n))
        if e > WORST.get(k, (0.0, ""))[0]:
            WORST[k] = (e, tag + " " + n)
        assert e <= bar_factor * _bar(prec, n), "%s %s: rel L2 %.3e over %.3e" % (tag, n, e, bar_factor * _bar(prec, n))


@pytest.fixture(scope="module", autouse=True)
def _worst_table():
    yield
    print("\nworst per-tensor relative L2 per (mode, tensor class):")
    for k in sorted(WORST):
        print("  %-8s %-22s %.3e   (%s)" % (k[0], k[1], WORST[k][0], WORST[k][1]))


def _decisions_ok(tag, prec, ts_gpu, ref):
    """True when the pass made the reference's decisions.  fp32 / split modes: anything else fails.  16-bit modes: see the module docstring."""
    want = ref["o"]["token_select"] > 0.5
    flip = (ts_gpu.cpu() > 0.5) != want
    n = int(flip.sum())
    if n == 0:
        return True
    assert prec in ("fp16", "bf16"), "%s: %d token decisions differ from the reference (margins were asserted outside the tie band)" % (tag, n)
    assert n <= D.TOL[prec]["step_flips"], (tag, n)
    print("%s: %d decisions differ (largest margin %.2e): the gradients of this pass are consequences, not compared" % (tag, n, float(ref["z"][flip].max())))
    return False


def _run(eng, B, mode, complete, R, slot=0, taps=None, variant="plain"):
    x, draws = _inputs(B)
    res = eng.forward_features_tokens(x.cuda(), training=True, complete_model=complete, masked_dense=(mode == "masked"), save=True,
                                      taps=taps, slot=slot, **_dev_draws(draws))
    tok, ts = res[0], res[-2]
    dtaps = [None] * eng.depth
    for i, r in R[1].items():
        dtaps[i] = r.cuda()
    g = torch.zeros_like(eng.flat)
    eng.backward_tokens(slot, None if R[0] is None else R[0].cuda(), dtaps, g,
                        dtoken_select=None if R[2] is None else R[2].cuda(), dtoken_logits=None if R[3] is None else R[3].cuda())
    torch.cuda.synchronize()
    return res, ts, g


# ------------------------------------------------------------------------------------------------------------------------------
# 1. forward, bitwise
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_forward_taps_are_the_pass_own_snapshots(prec):
    B = 2
    x, draws = _inputs(B)
    kw = dict(training=True, masked_dense=True, **_dev_draws(draws))
    eng = _engine(prec)
    plain = eng.forward_features_tokens(x.cuda(), **kw)
    tok, taps, ts, tl = eng.forward_features_tokens(x.cuda(), taps=(0, 2, 1), **kw)
    saved0 = eng.forward_features_tokens(x.cuda(), save=True, **kw)
    saved = eng.forward_features_tokens(x.cuda(), taps=(1, 2), save=True, **kw)
    torch.cuda.synchronize()
    # tapping changes no other output bit, in a plain and in a saved pass (a saved pass of the 16-bit modes is not the unsaved one bit for
    # bit: its fc1 epilogue evaluates GELU together with its derivative); the top tap is the token output itself
    for a, b in zip(plain, (tok, ts, tl)):
        assert torch.equal(a, b)
    for a, b in zip(saved0, (saved[0], saved[2], saved[3])):
        assert torch.equal(a, b)
    assert torch.equal(taps[1], tok) and torch.equal(saved[1][1], saved[0])
    if prec == "fp32":
        assert torch.equal(saved[0], tok) and torch.equal(saved[1][0], taps[2])
    # tap i of a depth-d pass == the token output of a depth-(i+1) context with the same weights and draws
    sd = _sd()
    for i, tap in ((0, taps[0]), (1, taps[2])):
        d = i + 1
        small = DyTEngine(C, RANK, 0.1, DEV, precision=prec, max_batch=B, depth=d)
        small.load_state_dict({k: v for k, v in sd.items() if not k.startswith("blocks.") or int(k.split(".")[1]) < d})
        out = small.forward_features_tokens(x.cuda(), training=True, masked_dense=True, g1=draws[0][:d].contiguous().cuda(),
                                            g2=draws[1][:d].contiguous().cuda(), keep_mask=draws[2][:d].contiguous().cuda())[0]
        torch.cuda.synchronize()
        assert torch.equal(out, tap), (prec, i)
        del small
    # the inference-only context gives the same taps (eval pass: it has no training forward with saved tensors to offer)
    inf = _engine(prec, inference=True)
    a = eng.forward_features_tokens(x.cuda(), taps=(0, 1, 2))
    b = inf.forward_features_tokens(x.cuda(), taps=(0, 1, 2))
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and all(torch.equal(p, q) for p, q in zip(a[1], b[1])) and torch.equal(a[2], b[2])


def _model(prec, depth=12, train_mode="masked", variant="plain", sd=None, rank=64, num_classes=100, **kw):
    from models.vision_transformer_IN21K import VisionTransformer
    sd = sd if sd is not None else _once(("msd", depth, variant, rank, num_classes), lambda: synth.make_state_dict(
        num_classes, rank, seed=SEED, kind="test", depth=depth, gate_bias=0.85, head_norm="fc_norm" if variant == "fc_norm" else "norm"))
    tuning = D.Cfg(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option="none", ffn_adapter_init_option="lora",
                   ffn_adapter_scalar="0.1", ffn_num=rank, d_model=768)
    m = VisionTransformer(num_classes=num_classes, depth=depth, drop_path_rate=0.0, tuning_config=tuning, select_config=D.Cfg(open=True, keep_layers=0),
                          precision=prec, train_mode=train_mode, fc_norm=(variant == "fc_norm"), **kw)
    m.load_state_dict(sd, strict=True)
    for n, p in m.named_parameters():
        p.requires_grad = synth.is_trainable(n)
    return m.cuda(), sd


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_forward_features_without_grad_is_the_old_route(prec):
    """forward_features(x) under no_grad == eng.forward_features_tokens + dyt_layernorm, the route it always took; with out_indices the
    tokens are the same bits and the taps are the engine's; with grad enabled (eval mode) the values are the same again."""
    B = 2
    m, _ = _model(prec)
    m.eval()
    x, _ = synth.make_batch(B, 100, seed=SEED)
    x = x.cuda()
    with torch.no_grad():
        feats, aux = m.forward_features(x)
        f2, taps, aux2 = m.forward_features(x, out_indices=(3, 5, 7, -1))
    eng = m._engine
    tok, ts, tl = eng.forward_features_tokens(x)
    want = torch.empty_like(tok)
    _lib.check(_lib.lib().dyt_layernorm(ptr(tok.view(-1, DIM)), ptr(m.norm.weight.detach().float().contiguous()), ptr(m.norm.bias.detach().float().contiguous()),
                                        ptr(want.view(-1, DIM)), B * NT, stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(feats, want) and torch.equal(f2, want) and torch.equal(aux["token_select"][..., 0], ts) and torch.equal(aux2["token_logits"][..., 0], tl)
    assert len(taps) == 4 and torch.equal(taps[3], tok) and not feats.requires_grad
    et = eng.forward_features_tokens(x, taps=(3, 5, 7, 11))[1]
    assert all(torch.equal(a, b) for a, b in zip(taps, et))
    # eval mode, grad enabled: without out_indices the call stays what it was (forward only, the same bits); with out_indices it is differentiable
    # (a saved pass: the same bits in fp32, the 16-bit modes' saved-pass arithmetic otherwise)
    fe, _ = m.forward_features(x)
    assert not fe.requires_grad and torch.equal(fe, want)
    fg, tg, _ = m.forward_features(x, out_indices=(3, 5, 7, 11))
    assert fg.requires_grad and tg[0].requires_grad
    if prec == "fp32":
        assert torch.equal(fg.detach(), want) and all(torch.equal(a.detach(), b) for a, b in zip(tg, et))
    else:
        assert float((fg.detach() - want).abs().max()) < 5e-3
    with pytest.raises(ValueError, match="distinct"):
        m.forward_features(x, out_indices=(3, 3))


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the tapped ln_bwd instantiations alone
# ------------------------------------------------------------------------------------------------------------------------------
def _unit_mode(name):
    import test_gpu_row_bwd as RT
    return RT._mode(name)


def _tap_call(mode, dy, x, stats, w, base, base_at, dx, rows, tap, g_at=None, h_next=None, dst=None, dm=None, out3=None, s3=1.0, hi_only=0):
    L, prec, dt, gs = _unit_mode(mode)
    fn = L.dyt_unit_ln_bwd_tap if tap is not None else None
    if fn is None:
        rc = L.dyt_unit_ln_bwd(ptr(dy), ptr(x), ptr(stats), ptr(w), ptr(base), ptr(base_at), ptr(dx), rows, ptr(g_at), ptr(h_next), ptr(dst), ptr(dm),
                               gs, ptr(out3), s3, hi_only, prec, stream_ptr())
    else:
        rc = fn(ptr(dy), ptr(x), ptr(stats), ptr(w), ptr(base), ptr(base_at), ptr(dx), rows, ptr(g_at), ptr(h_next), ptr(dst), ptr(dm),
                gs, ptr(out3), s3, hi_only, ptr(tap), prec, stream_ptr())
    assert rc == 0, (rc, L.dyt_last_error())


def _cmp_tap(what, gpu, r64, r32, extra_rel=None):
    """_cmp's rule + half an ulp of max|sum| (module docstring); extra_rel: + that fraction of |fp64| per element (a 16-bit output alone)."""
    gpu, r64, r32 = gpu.detach().to("cpu", F64), r64.to(F64), r32.to("cpu", F64)
    assert gpu.shape == r64.shape and bool(torch.isfinite(gpu).all()), what
    floor = float((r32 - r64).abs().max())
    allowed = 4.0 * floor + 4.5 * ulp(r64.abs().max()) + (extra_rel * r64.abs() if extra_rel else 0.0)
    ratio = float(((gpu - r64).abs() / allowed).max())
    print("[ln_bwd tap] %s: worst error / allowed %.3f (fp32 floor %.3e)" % (what, ratio, floor))
    assert ratio <= 1.0, "%s: error exceeds the allowance by a factor %.3f" % (what, ratio)


@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("rows", [1, 4, 394])
def test_tapped_ln_bwd_against_fp64(rows, mode):
    import test_gpu_row_bwd as RT
    L, prec, dt, gs = _unit_mode(mode)
    g, x, w, dy, mean, rstd, stats = RT._ln_inputs(rows, mode, 12)
    tap = RT._randn(g, rows, DIM)
    base = RT._randn(g, rows, DIM)
    keep = torch.rand(rows, generator=g) < 0.6
    keep[0] = True
    dst = RT._compact(keep)
    h_next = RT._randn(g, int(keep.sum()), DIM).to(dt)
    xd, wd, dyd, sd_, td = (RT._dev(t) for t in (x, w, dy, stats, tap))
    tag = "rows=%d %s " % (rows, mode)
    kw0 = dict(gs=gs)
    # (i) no base, no prep: dx alone
    dx = RT._out_rows(rows, DIM, F32)
    _tap_call(mode, dyd, xd, sd_, wd, None, None, dx, rows, td)
    r64, _ = TG.ln_bwd_tap_ref(dy, x, mean, rstd, w, tap, **kw0)
    r32, _ = TG.ln_bwd_tap_ref(dy, x, mean, rstd, w, tap, dtype=F32, **kw0)
    _cmp_tap(tag + "plain dx", dx[:rows], r64, r32)
    RT._tail_untouched(dx, rows, tag)
    # (ii) base in place + the fused next-block prep (g_at, dmask_next through dst_of_next)
    dx = RT._out_rows(rows, DIM, F32)
    dx[:rows] = RT._dev(base)
    g_at, dm = RT._out_rows(rows, DIM, dt), RT._out_rows(rows, 1, F32).view(-1)
    _tap_call(mode, dyd, xd, sd_, wd, dx, None, dx, rows, td, g_at=g_at, h_next=RT._dev(h_next), dst=RT._dev(dst), dm=dm)
    kw = dict(base=base, gs=gs, h_next=h_next, dst_of_next=dst)
    (b64, m64), (b32, m32) = TG.ln_bwd_tap_ref(dy, x, mean, rstd, w, tap, **kw), TG.ln_bwd_tap_ref(dy, x, mean, rstd, w, tap, dtype=F32, **kw)
    _cmp_tap(tag + "base + tap dx", dx[:rows], b64, b32)
    RT._same_rounding(tag + "g_at", g_at[:rows], dx[:rows], gs, dt, b64)
    _cmp_tap(tag + "dmask_next", dm[:rows].cpu()[keep], m64[keep], m32[keep])
    if bool((~keep).any()):
        assert float(dm[:rows].cpu()[~keep].abs().max()) == 0.0
    for buf in (dx, g_at, dm):
        RT._tail_untouched(buf, rows, tag)
    # (iii) without h_next / dst_of_next: dmask_next is written as 0, g_at still the rounded row
    g_at2, dm2 = RT._out_rows(rows, DIM, dt), RT._out_rows(rows, 1, F32).view(-1)
    dx2 = RT._out_rows(rows, DIM, F32)
    _tap_call(mode, dyd, xd, sd_, wd, RT._dev(base), None, dx2, rows, td, g_at=g_at2, dm=dm2)
    assert torch.equal(dx2[:rows], dx[:rows]) and torch.equal(g_at2[:rows], g_at[:rows]) and float(dm2[:rows].abs().max()) == 0.0
    # (iv) a tap of zeros == the untapped kernel, bit for bit, in every output
    z = torch.zeros(rows, DIM, device=DEV)
    outs = []
    for t in (z, None):
        dxz = RT._out_rows(rows, DIM, F32)
        gz, dz = RT._out_rows(rows, DIM, dt), RT._out_rows(rows, 1, F32).view(-1)
        _tap_call(mode, dyd, xd, sd_, wd, RT._dev(base), None, dxz, rows, t, g_at=gz, h_next=RT._dev(h_next), dst=RT._dev(dst), dm=dz)
        outs.append((dxz, gz, dz))
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(*outs)), tag + "tap of zeros differs from the untapped kernel"
    if prec == 0:
        return
    # (v) the 16-bit stream: base_at in, g_at out, no fp32 row
    base_at = (gs * RT._randn(g, rows, DIM)).to(dt)
    g_at = RT._out_rows(rows, DIM, dt)
    _tap_call(mode, dyd, xd, sd_, wd, None, RT._dev(base_at), None, rows, td, g_at=g_at)
    s64, _ = TG.ln_bwd_tap_ref(dy, x, mean, rstd, w, tap, base_at=base_at, gs=gs)
    s32, _ = TG.ln_bwd_tap_ref(dy, x, mean, rstd, w, tap, base_at=base_at, gs=gs, dtype=F32)
    RT._assert_normal(s64, gs, dt, tag + "base_at + tap")
    _cmp_tap(tag + "base_at + tap -> g_at", g_at[:rows].to(F64) / gs, s64, s32, extra_rel=torch.finfo(dt).eps / 2)
    gz, gn = RT._out_rows(rows, DIM, dt), RT._out_rows(rows, DIM, dt)
    _tap_call(mode, dyd, xd, sd_, wd, None, RT._dev(base_at), None, rows, z, g_at=gz)
    _tap_call(mode, dyd, xd, sd_, wd, None, RT._dev(base_at), None, rows, None, g_at=gn)
    assert torch.equal(gz.view(torch.int16), gn.view(torch.int16))


@pytest.mark.parametrize("hi_only", [0, 1])
@pytest.mark.parametrize("rows", [1, 394])
def test_tapped_ln_bwd_split_operand(rows, hi_only):
    import test_gpu_row_bwd as RT
    mode, s3 = "fp32h", 4096.0
    g, x, w, dy, mean, rstd, stats = RT._ln_inputs(rows, mode, 13)
    tap = RT._randn(g, rows, DIM)
    outs = []
    for t in (tap, torch.zeros_like(tap), None):
        dx = RT._out_rows(rows, DIM, F32)
        out3 = torch.full((rows + 3, 2 * DIM), RT.SENT, dtype=torch.float16)
        out3[:rows, :DIM if hi_only else 2 * DIM] = math.nan
        out3 = out3.to(DEV)
        _tap_call(mode, RT._dev(dy), RT._dev(x), RT._dev(stats), RT._dev(w), None, None, dx, rows, RT._dev(t), out3=out3, s3=s3, hi_only=hi_only)
        outs.append((dx, out3))
    r64, _ = TG.ln_bwd_tap_ref(dy, x, mean, rstd, w, tap)
    r32, _ = TG.ln_bwd_tap_ref(dy, x, mean, rstd, w, tap, dtype=F32)
    tag = "rows=%d hi_only=%d " % (rows, hi_only)
    _cmp_tap(tag + "dx next to out3", outs[0][0][:rows], r64, r32)
    RT._split_check(tag + "out3", outs[0][1][:rows].cpu(), s3, bool(hi_only), outs[0][0][:rows])
    RT._tail_untouched(outs[0][1], rows, tag)
    assert torch.equal(outs[1][0][:rows], outs[2][0][:rows]) and torch.equal(outs[1][1][:rows, :DIM].view(torch.int16), outs[2][1][:rows, :DIM].view(torch.int16))


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the whole backward against tap_loss_grads
# ------------------------------------------------------------------------------------------------------------------------------
_engines = {}


def _shared_engine(prec, variant="plain"):
    k = (prec, variant)
    if k not in _engines:
        _engines.clear()   # one context at a time
        torch.cuda.empty_cache()
        _engines[k] = _engine(prec, variant=variant)
    return _engines[k]


PASSES = [("masked", False), ("compact", False), ("masked", True)]


@pytest.mark.parametrize("which", ["a", "b", "c", "d"])
@pytest.mark.parametrize("mode,complete", PASSES)
@pytest.mark.parametrize("prec", ["fp32", "fp16x3q", "fp16", "bf16"])
def test_backward_tokens_against_the_oracle(prec, mode, complete, which):
    B = 2
    ref = _reference(B, mode, complete, which)
    if not complete:
        _assert_margins(ref)
    eng = _shared_engine(prec)
    tag = "%s %s%s (%s)" % (prec, mode, " complete" if complete else "", which)
    res, ts, g = _run(eng, B, mode, complete, ref["R"], slot=1 if complete else 0)
    tok_err = float((res[0].cpu() - ref["o"]["blocks"][-1]).abs().max())
    print("%s: last-block tokens max abs error %.2e" % (tag, tok_err))
    if not complete and not _decisions_ok(tag, prec, ts, ref):
        return
    assert float(g.abs().max()) > 0 and bool(torch.isfinite(g).all())
    off, num = eng.trainable_slice("head.weight")
    assert float(g[off:].abs().max()) == 0.0, "the head's range of grad_flat was written"
    _judge(tag, prec, eng, g, ref["g"])


# ------------------------------------------------------------------------------------------------------------------------------
# 4. against the classification path: same model, same draws
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_features_plus_torch_head_equals_forward(prec):
    B, NC, r = 2, 100, 64
    m, sd = _model(prec)
    m.train()
    x, y = synth.make_batch(B, NC, seed=SEED)
    g1, g2 = synth.make_noise(B, seed=SEED + 1, passes=1)
    keep = synth.make_dropout_masks(B, r, seed=SEED + 2, passes=1)
    draws = (g1[0].contiguous(), g2[0].contiguous(), keep[0].contiguous())
    kw = dict(gumbel=(draws[0].cuda(), draws[1].cuda()), keep_mask=draws[2].cuda())
    params = dict(m.named_parameters())

    def grads():
        out = {n: p.grad.detach().clone().cpu() for n, p in params.items() if p.grad is not None}
        for p in params.values():
            p.grad = None
        return out
    feats, aux_f = m.forward_features(x.cuda(), **kw)
    logits_f = F.linear(feats[:, 0], m.head.weight, m.head.bias)
    F.cross_entropy(logits_f, y.cuda()).backward()
    gf = grads()
    logits, aux = m(x.cuda(), **kw)
    F.cross_entropy(logits, y.cuda()).backward()
    gc = grads()
    torch.cuda.synchronize()
    # the oracle: CE of its own student forward over the same tensors
    names = O.trainable_names(sd)
    leaf = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in sd.items()}
    lo, oo = O.forward(leaf, x, *draws, mode="masked")
    go = dict(zip(names, torch.autograd.grad(F.cross_entropy(lo, y), [leaf[k] for k in names], allow_unused=True)))
    band = PR.tie_band(sd, x, draws[0], draws[1], draws[2], "masked", oo["token_logits"].detach()[..., 0])
    z = ((oo["token_logits"].detach()[..., 0].double() + (draws[0] - draws[1]).permute(1, 0, 2).double()) / 5.0).abs()
    assert bool((z > 4.0 * band.view(1, -1, 1)).all()), "a reference margin lies inside four times the tie band: choose other seeds"
    want = oo["token_select"].detach()
    assert torch.equal(aux_f["token_select"].detach().cpu(), aux["token_select"].detach().cpu())
    same = torch.equal(aux["token_select"].detach().cpu() > 0.5, want > 0.5)
    assert same or prec != "fp32", "decisions differ from the oracle"
    tol = D.TOL[prec]["logits"]
    e = float((logits_f - logits).detach().abs().max())
    print("%s: logits through forward_features + torch head vs forward: %.2e; vs oracle %.2e" % (prec, e, float((logits.detach().cpu() - lo.detach()).abs().max())))
    assert e <= tol
    assert sorted(gf) == sorted(gc)
    for n in sorted(gc):
        bar = _bar(prec, n)
        if gc[n].numel() == 1 and prec != "fp32":
            continue   # single gate-bias numbers: judged as one vector below
        if float(gc[n].norm()) == 0.0:   # the last block's gate: only the cls row reaches this loss, and the cls token is never gated
            assert "blocks.11.mlp_token_select" in n and float(gf[n].abs().max()) == 0.0, (prec, n)
            continue
        e = float((gf[n] - gc[n]).norm() / gc[n].norm())
        assert e <= bar, (prec, n, "two routes", e)
        if same and go.get(n) is not None:
            for tagn, got in (("features", gf[n]), ("forward", gc[n])):
                eo = float((got - go[n]).norm() / go[n].norm())
                k = (prec, D.grad_kind(n))
                if eo > WORST.get(k, (0.0, ""))[0]:
                    WORST[k] = (eo, "classification dlogits, %s route, %s" % (tagn, n))
                assert eo <= bar, (prec, n, tagn, "oracle", eo)
    bias = sorted(n for n in gc if n.endswith("mlp_head.bias") and float(gc[n].norm()) > 0)
    vf, vc = torch.cat([gf[n] for n in bias]), torch.cat([gc[n] for n in bias])
    assert float((vf - vc).norm() / vc.norm()) <= _bar(prec, bias[0])


# ------------------------------------------------------------------------------------------------------------------------------
# 5. properties
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_backward_tokens_is_reproducible_and_null_is_zero(prec):
    B = 2
    R = _R(B, "d")
    eng = _shared_engine(prec)
    runs = [_run(eng, B, "masked", False, R)[2] for _ in range(2)]
    assert float(runs[0].abs().max()) > 0 and torch.equal(runs[0], runs[1])
    # dtaps[i] of zeros == NULL, bit for bit (functional (a) with zero taps at every block against no taps)
    Ra = _R(B, "a")
    zeros = {i: torch.zeros(B, NT, DIM) for i in range(DEPTH)}
    g0 = _run(eng, B, "masked", False, Ra)[2]
    g1 = _run(eng, B, "masked", False, (Ra[0], zeros, None, None))[2]
    assert torch.equal(g0, g1)


def test_backward_tokens_batch_equivariance():
    """B = 3 in one pass against three B = 1 passes on the same images, draws and gradients, fp32 mode: the sums agree to the re-ordering of
    fp32 sums of at most 591 terms (sqrt(591) eps ~ 1.5e-6 relative per element): 1e-5 of the largest element per tensor."""
    B = 3
    eng = _shared_engine("fp32")
    x, draws = _inputs(B)
    R = _R(B, "d")
    whole = _run(eng, B, "masked", False, R)[2]
    parts = torch.zeros_like(whole)
    for b in range(B):
        kw = dict(g1=draws[0][:, b:b + 1].contiguous().cuda(), g2=draws[1][:, b:b + 1].contiguous().cuda(),
                  keep_mask=draws[2][:, b * NT:(b + 1) * NT].contiguous().cuda())
        eng.forward_features_tokens(x[b:b + 1].cuda(), training=True, masked_dense=True, save=True, **kw)
        dtaps = [None] * DEPTH
        for i, r in R[1].items():
            dtaps[i] = r[b:b + 1].contiguous().cuda()
        eng.backward_tokens(0, R[0][b:b + 1].contiguous().cuda(), dtaps, parts, dtoken_select=R[2][b:b + 1].contiguous().cuda(),
                            dtoken_logits=R[3][b:b + 1].contiguous().cuda())
    torch.cuda.synchronize()
    for n in TG.backbone_names(_sd()):
        a, b_ = eng.trainable_view(n, (-1,), whole), eng.trainable_view(n, (-1,), parts)
        assert float(a.abs().max()) > 0 and float((a - b_).abs().max()) <= 1e-5 * float(a.abs().max()), n


# ------------------------------------------------------------------------------------------------------------------------------
# 6. options (fp32, depth 3, against the oracle)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["drop_path", "scale", "ln_in", "fc_norm"])
def test_options_against_the_oracle(variant):
    B = 2
    ev = "plain" if variant == "drop_path" else variant
    drop = None
    if variant == "drop_path":
        gen = torch.Generator().manual_seed(SEED + 9)
        dpr = torch.linspace(0, 0.1, DEPTH)
        drop = torch.ones(2, DEPTH, B)
        for l in range(1, DEPTH):
            kp = 1.0 - float(dpr[l])
            drop[:, l] = (torch.rand(2, B, generator=gen) < 0.5).float() / kp   # (half of the branches dropped: at 0.1 none would be in so small a case)
    ref = _reference(B, "masked", False, "d", variant=ev, drop_scales=drop)
    _assert_margins(ref)
    eng = _shared_engine("fp32", variant=ev)
    if drop is not None:
        eng.set_drop_path(0.1)
        eng.set_drop_path_scales(0, drop.cuda().contiguous())
    try:
        res, ts, g = _run(eng, B, "masked", False, ref["R"])
        assert _decisions_ok(variant, "fp32", ts, ref)
        _judge("option " + variant, "fp32", eng, g, ref["g"])
        if variant == "fc_norm":
            # identity final norm: dtokens and the top tap are gradients of the same tensor -- equal inputs, equal bits
            Rt = ref["R"][0]
            ga = _run(eng, B, "masked", False, (Rt, {}, None, None))[2]
            gb = _run(eng, B, "masked", False, (None, {DEPTH - 1: Rt}, None, None))[2]
            assert float(ga.abs().max()) > 0 and torch.equal(ga, gb)
    finally:
        if drop is not None:
            _engines.clear()   # (the injected factors belong to this test)


# ------------------------------------------------------------------------------------------------------------------------------
# 7. refusals
# ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched():
    B = 2
    x, draws = _inputs(B)
    eng = _shared_engine("fp32")
    R = _R(B, "a")
    g = torch.full_like(eng.flat, 3.0)
    kw = dict(training=True, masked_dense=True, **_dev_draws(draws))
    # slot kinds crossed, both ways
    eng.forward_features_tokens(x.cuda(), save=True, **kw)
    with pytest.raises(DyTError, match="its backward is dyt_backward_tokens, not dyt_backward"):
        eng.backward(0, torch.zeros(B, C, device=DEV), g)
    eng.forward(x.cuda(), slot=0, training=True, save=True, masked_dense=True, gate_always=True, **_dev_draws(draws))
    with pytest.raises(DyTError, match="its backward is dyt_backward, not dyt_backward_tokens"):
        eng.backward_tokens(0, R[0].cuda(), None, g)
    # every gradient input NULL
    eng.forward_features_tokens(x.cuda(), save=True, **kw)
    with pytest.raises(DyTError, match="every gradient input is NULL"):
        eng.backward_tokens(0, None, [None] * DEPTH, g)
    # a slot without a saved pass
    eng.forward_features_tokens(x.cuda(), **kw)
    with pytest.raises(DyTError, match="holds no saved forward"):
        eng.backward_tokens(0, R[0].cuda(), None, g)
    torch.cuda.synchronize()
    assert bool((g == 3.0).all()), "a refused call wrote grad_flat"
    # inference-only context
    inf = _engine("fp32", inference=True)
    with pytest.raises(DyTError, match="inference_only"):
        inf.forward_features_tokens(x.cuda(), save=True, taps=(1,))
    gi = torch.full_like(inf.flat, 3.0)
    with pytest.raises(DyTError, match="dyt_backward_tokens: the context was created with dyt_config.inference_only"):
        inf.backward_tokens(0, R[0].cuda(), None, gi)
    assert bool((gi == 3.0).all())
    del inf
    # video model
    vid = DyTEngine(C, RANK, 0.1, DEV, precision="fp32", max_batch=2, depth=1, frames=2)
    tok = torch.full((2, NT, DIM), 3.0, device=DEV)
    gv = torch.full_like(vid.flat, 3.0)
    with pytest.raises(DyTError, match="dyt_forward_taps: image model only"):
        vid.forward_features_tokens(x.cuda(), taps=(0,))
    with pytest.raises(DyTError, match="dyt_backward_tokens: image model only"):
        vid.backward_tokens(0, tok, None, gv)
    assert bool((gv == 3.0).all()) and bool((tok == 3.0).all())
    del vid


def test_autograd_bridge_refuses_an_overwritten_slot_and_the_video_model():
    m, _ = _model("fp32", depth=2, sd=None, rank=RANK, num_classes=C)
    m.train()
    x, _ = synth.make_batch(2, C, seed=SEED)
    feats, taps, _ = m.forward_features(x.cuda(), out_indices=(0,))
    m.forward_features(x.cuda())   # a later forward of the same kind overwrites the slot
    with pytest.raises(DyTError, match="whose saved activations were overwritten by a later forward"):
        (feats.sum() + taps[0].sum()).backward()
    assert all(p.grad is None for p in m.parameters())
    m.norm.weight.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="norm.requires_grad=True"):
        m.forward_features(x.cuda())
    m.norm.weight.requires_grad_(False)
    # (there is no captured-graph form of this route to ask for: it is not part of the fused step, which is what hip_graph replays)
    m._frames = 2
    with pytest.raises(NotImplementedError, match="forward_features of the video model"):
        m.forward_features(x.cuda())


# ------------------------------------------------------------------------------------------------------------------------------
# 8. end to end: a torch pyramid head over taps (3, 5, 7, 11), AdamW over adapters, gates and head
# ------------------------------------------------------------------------------------------------------------------------------
class _Pyramid(torch.nn.Module):
    """Four scales from four taps: x4 (two transposed convolutions with a GELU between), x2, x1, x1/2; a 1x1 classifier on each, summed at
    the coarsest common size into per-pixel class scores [B, classes, 14, 14]."""

    def __init__(self, dim=DIM, classes=5):
        super().__init__()
        nn = torch.nn
        self.up4 = nn.Sequential(nn.ConvTranspose2d(dim, dim // 4, 2, 2), nn.GELU(), nn.ConvTranspose2d(dim // 4, dim // 8, 2, 2))
        self.up2 = nn.ConvTranspose2d(dim, dim // 4, 2, 2)
        self.same = nn.Identity()
        self.down = nn.MaxPool2d(2, 2)
        self.cls = nn.ModuleList([nn.Conv2d(c, classes, 1) for c in (dim // 8, dim // 4, dim, dim)])

    def forward(self, taps):
        maps = [t[:, 1:].transpose(1, 2).reshape(t.shape[0], DIM, 14, 14) for t in taps]
        feats = [self.up4(maps[0]), self.up2(maps[1]), self.same(maps[2]), self.down(maps[3])]
        return sum(F.adaptive_avg_pool2d(c(f), 14) for c, f in zip(self.cls, feats))


def test_five_steps_with_a_pyramid_head():
    B = 2
    sd = synth.reference_adapter_init(synth.make_state_dict(100, 64, seed=SEED, kind="test", gate_bias=0.85), seed=SEED)
    m, _ = _model("fp16", sd=sd)
    m.train()
    torch.manual_seed(SEED)
    head = _Pyramid().cuda()
    x, _ = synth.make_batch(B, 100, seed=SEED)
    target = torch.randint(0, 5, (B, 14, 14), generator=torch.Generator().manual_seed(SEED)).cuda()
    back = [p for n, p in m.named_parameters() if p.requires_grad and not n.startswith("head.")]
    up = {n: p for n, p in m.named_parameters() if n.endswith("adaptmlp.up_proj.weight")}
    assert len(up) == 12 and all(float(p.abs().max()) == 0.0 for p in up.values())
    opt = torch.optim.AdamW(back + list(head.parameters()), lr=1e-3, weight_decay=0.0)
    losses = []
    for _ in range(5):
        opt.zero_grad(set_to_none=True)
        _, taps, aux = m.forward_features(x.cuda(), out_indices=(3, 5, 7, 11))
        loss = F.cross_entropy(head(taps), target) + 0.1 * (aux["token_select"].mean() - 0.5) ** 2
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print("pyramid head, five AdamW steps: loss", " ".join("%.4f" % v for v in losses))
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0]
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in up.values())
    assert all(float(p.detach().abs().max()) > 0 for p in up.values()), "an up_proj is still at its zero initialisation"
    assert all(p.grad is None for n, p in m.named_parameters() if n.startswith("head."))
