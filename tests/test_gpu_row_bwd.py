"""Unit tests of the row kernels that carry the gradient from one block to the next (csrc/block_bwd.hip, csrc/ln.hip), each alone through its unit entry
(include/dyt_hip.h: dyt_unit_bwd_prep, dyt_unit_ln_bwd, dyt_unit_ln_param_grad, dyt_unit_tok_bwd) next to an fp64 reference
(tests/rowbwd_refs.py, pinned to autograd by tests/test_rowbwd_refs_host.py):

  bwd_prep_kernel                                   g_at, dH, dmask
  ln_bwd_kernel                                     dx, g_at, out3, dmask_next
  ln_param_grad_kernel / ln_param_reduce_kernel     out[1536] (+=)
  tok_bwd_kernel / reduce_partials_batch_kernel     du, du_at, du3, d_gate[769] (+=, through queue_tok_reduce + flush_reductions)

The rule is the one of tests/test_gpu_step_tail.py (_cmp, imported from there): for every fp32 output the reference is evaluated in fp64
and in fp32 on the CPU from the very values the kernel read (16-bit inputs upcast exactly), floor = max|fp32_cpu - fp64|, and the kernel
must satisfy  max|gpu - fp64| <= 4 floor + 4 ulp(max|fp64|).  As there, a scalar has no floor worth the name: d_gate[768] (the gate bias
gradient) is compared inside the whole d_gate[0:769], next to d_gate[0:768] alone.
16-bit outputs: where the launch also writes the fp32 value, the 16-bit output equals (fp32 output * gs) rounded to the operand type bit
for bit (one rounding of the same register); where it does not (the fp16 stream forms), |out / gs - fp64| <= the fp32 bound + eps/2 |fp64|
per element.  Both need the scaled values to be normal and finite in the operand type: asserted on the reference (zeros excluded).
Split outputs (out3 / du3, the [rows][hi 768 | lo 768] image of store4_split3, IEEE-half library at precision 0): (hi + lo) / scale is
within 2^-21 |value| of the fp32 output of the same launch, hi alone within eps(fp16)/2 |value|; elements whose lo (hi) part would be
subnormal in fp16 -- |value * scale| < 2^-2 (2^-14) -- are left out (they are a 1e-4 fraction of a row at the magnitudes used here).
Buffers a call must not write hold a finite sentinel and are compared bit for bit afterwards; outputs it must write start as NaN.

Modes: "fp32" = libdyt_hip.so at precision 0; "bf16" = libdyt_hip.so at precision 1 (gs 1); "fp16" = libdyt_hip_f16.so at precision 1
with the fp16 build's gradient factor (read from csrc/ctx.hip); "fp32h" = libdyt_hip_f16.so at precision 0 (the split forms).

Every case prints its error / floor ratio and the module prints the worst per kernel at its end.  The table (also DESIGN.md 7m; records
of one run, not bounds):

  kernel(s)                        compared                     worst error / floor (one MI355X run; all 82 tests pass, 2 s)
  bwd_prep                         dmask                        1.34 (rows=3 bf16); g_at and dH bit for bit
  ln_bwd                           dx, dmask_next               2.33 (rows=4 fp32, dmask_next); g_at bit for bit next to dx;
                                                                base_at -> g_at alone: 0.994 of what it is allowed (rows=197)
  ln_param_grad / ln_param_reduce  d gamma, d beta              1.47 (rows=32 fp32, d gamma)
  tok_bwd                          du                           1.16 (dense, B=2 fp16); du_at bit for bit next to du; du_at alone
                                                                (fp16 stream form): 0.992 of what it is allowed (B=2 bf16)
  tok_bwd + reduce_partials_batch  d_gate                       1.03 (dad + du_at, B=2 bf16, d_gate[0:768])

Each of these edits to csrc/block_bwd.hip / csrc/ln.hip turns the named tests red (checked once on the MI355X, on scratch copies): `dmk *= bs` dropped --
test_tok_bwd_branch_scale; the cat subtraction dropped -- test_tok_bwd_cat_correction; `du += e` without inv_gs --
test_tok_bwd_16bit_adapter_dgrad_and_stream[fp16]; `/ a.tau` skipped, or rv read at lane (k >> 2) ^ 1 -- every tok_bwd test with a gate,
resp. with dA2 (26 cases each); dmask_next from the gs-scaled row in ln_bwd_kernel -- test_ln_bwd[3 / 4 / 5 / 197-fp16].

Not reachable from here: the kernels' behaviour under a concurrently running stream (the reason for their full vmcnt drains, DESIGN.md
7b) -- the entries launch them alone; M beyond 591 tokens (the index arithmetic is size_t throughout).  (reduce_partials_batch_kernel with
more than one queued pair, blockIdx.y > 0, and the adapter weight-gradient half of flush_reductions are reached by
tests/test_gpu_unit_wgrad.py.)"""
import ctypes
import math
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

import _lib  # noqa: E402
import rowbwd_refs as R  # noqa: E402
from _lib import ptr, stream_ptr  # noqa: E402
from tail_refs import ulp  # noqa: E402
from test_gpu_step_tail import WORST, _cmp  # noqa: E402   (the project's comparison rule, unchanged)

DEV = "cuda:0"
F32, F64, I32 = torch.float32, torch.float64, torch.int32
NT, NP, D = R.NT, R.NP, R.D
SENT = 7.0   # finite sentinel, exact in every operand type
ERR_ARG = -1   # DYT_ERR_ARG (include/dyt_hip.h)
KERNELS = ("bwd_prep", "ln_bwd", "ln_param_grad", "tok_bwd", "tok_bwd+reduce")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fp16_gs():
    """The factor the fp16 build's 16-bit gradient operands carry, as the engine takes it: dyt_ctx::gs, set where the context is created."""
    src = open(os.path.join(ROOT, "dynamic-tuning_amd", "csrc", "ctx.hip")).read()
    m = re.search(r"#ifdef DYT_FP16\s*\n\s*if \(c->prec != DYT_PREC_FP32\) c->gs = ([0-9.]+)f;", src)
    assert m, "csrc/ctx.hip no longer sets the fp16 build's gs where this test looks for it"
    return float(m.group(1))


def _mode(name):
    """(library, precision, operand dtype, gs)"""
    if name == "fp32":
        return _lib.lib(), 0, F32, 1.0
    if name == "bf16":
        return _lib.lib(), 1, torch.bfloat16, 1.0
    if name == "fp16":
        return _lib.lib(fp16=True), 1, torch.float16, _fp16_gs()
    assert name == "fp32h"
    return _lib.lib(fp16=True), 0, F32, 1.0


MODES = ["fp32", "bf16", "fp16"]
MODES16 = ["bf16", "fp16"]


@pytest.fixture(scope="module", autouse=True)
def _worst_table():
    yield
    print("\nworst error / floor per kernel:")
    for k in KERNELS:
        if k in WORST:
            print("  %-28s %8.2f   (%s)" % (k, WORST[k][0], WORST[k][1]))


def _gen(*key):
    return torch.Generator().manual_seed(abs(hash(tuple(int(k) for k in key))) % (2 ** 31))


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _stats(x):
    """(mean, rstd, stats [rows, 2]) of an fp64 LayerNorm(eps 1e-6) of the fp32 rows x, rounded to fp32."""
    xd = x.double()
    mean = xd.mean(-1)
    rstd = 1.0 / (((xd - mean.view(-1, 1)) ** 2).mean(-1) + 1e-6).sqrt()
    mean, rstd = mean.float(), rstd.float()
    return mean, rstd, torch.stack([mean, rstd], 1).contiguous()


def _out_rows(rows, cols, dt, fill=math.nan, extra=3):
    """Device buffer [rows + extra, cols]: ``fill`` in the rows the call owns, the sentinel behind them."""
    t = torch.full((rows + extra, cols), SENT, dtype=dt)
    t[:rows] = fill
    return t.to(DEV)


def _tail_untouched(buf, rows, what):
    assert bool((buf[rows:] == SENT).all()), what + ": rows behind the last one were written"


def _assert_normal(ref64, gs, dt, what):
    """Every non-zero |ref * gs| is normal and finite in dt, with a factor 2 to spare on either side."""
    if dt == F32:
        return
    a = (ref64.double() * gs).abs()
    a = a[a != 0]
    fi = torch.finfo(dt)
    assert a.numel() and float(a.max()) <= fi.max / 2 and float(a.min()) >= 2 * fi.tiny, \
        "%s: scaled reference spans [%.3e, %.3e], outside the normal range of %s: choose other inputs" % (what, float(a.min()), float(a.max()), dt)


def _same_rounding(what, out16, out32, gs, dt, ref64):
    """16-bit output next to the fp32 output of the same launch: one rounding of the same register value."""
    _assert_normal(ref64, gs, dt, what)
    want = (out32 * gs).to(dt)
    assert torch.equal(out16, want), "%s: %d elements differ from (fp32 output * gs) rounded to %s" % (what, int((out16 != want).sum()), dt)


def _cmp16(kernel, what, out16, gs, dt, ref64, ref32):
    """16-bit output without an fp32 copy: |out / gs - fp64| <= 4 floor + 4 ulp(max|fp64|) + eps/2 |fp64| per element."""
    _assert_normal(ref64, gs, dt, what)
    got = out16.detach().to("cpu", F64) / gs
    ref64, ref32 = ref64.to(F64), ref32.to("cpu", F64)
    assert got.shape == ref64.shape and bool(torch.isfinite(got).all()), what
    floor = float((ref32 - ref64).abs().max())
    allowed = 4.0 * floor + 4.0 * ulp(ref64.abs().max()) + torch.finfo(dt).eps / 2 * ref64.abs()
    ratio = float(((got - ref64).abs() / allowed).max())
    print("[%s] %s: 16-bit only, worst |out/gs - fp64| / allowed %.3f (fp32 floor %.3e)" % (kernel, what, ratio, floor))
    assert ratio <= 1.0, "[%s] %s: |out/gs - fp64| exceeds the fp32 bound + half an ulp of %s by a factor %.3f" % (kernel, what, dt, ratio)


def _split_check(what, img, scale, hi_only, out32):
    """out3 / du3 against the fp32 output of the same launch (module docstring)."""
    v = out32.detach().to("cpu", F64)
    assert float((v * scale).abs().max()) <= 65504 / 2, what
    got = R.split3_value(img, scale, hi_only)
    assert bool(torch.isfinite(got).all()), what + ": NaN-filled operand was not (fully) written"
    ok = (v * scale).abs() >= (2.0 ** -14 if hi_only else 2.0 ** -2)
    assert float(ok.double().mean()) > 0.99, what
    rel = torch.finfo(torch.float16).eps / 2 if hi_only else 2.0 ** -21
    excess = float((((got - v).abs() - rel * v.abs())[ok]).max())
    assert excess <= 0.0, "%s: split operand off by %.3e more than %.3e |value|" % (what, excess, rel)
    if hi_only:
        assert bool((img[:, D:] == SENT).all()), what + ": the lo half is written although hi_only"


def _keep_mask(g, B, pattern):
    """[B, 197] bool: cls always kept, about half of the patches dropped; "mixed": image 1 with every patch dropped, image 2 with none."""
    keep = torch.rand(B, NT, generator=g) < 0.5
    keep[:, 0] = True
    if pattern == "mixed":
        if B >= 2:
            keep[1, 1:] = False
        if B >= 3:
            keep[2, :] = True
    return keep


def _compact(keep_flat, stride=1):
    idx = (torch.cumsum(keep_flat.to(torch.int64), 0) - 1) * stride
    return torch.where(keep_flat, idx, torch.full_like(idx, -1)).to(I32)


# ------------------------------------------------------------------------------------------------------------------------------
# bwd_prep
# ------------------------------------------------------------------------------------------------------------------------------
def _prep_call(mode, g, h, dst_of, row_mask, g_at, dH, dmask, M, expect=0):
    L, prec, dt, gs = _mode(mode)
    rc = L.dyt_unit_bwd_prep(ptr(g), ptr(h), ptr(dst_of), ptr(row_mask), ptr(g_at), ptr(dH), ptr(dmask), M, gs, prec, stream_ptr())
    assert rc == expect, (rc, L.dyt_last_error())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 197])
def test_bwd_prep(rows, mode):
    """4 rows per workgroup: 1, 3, 4, 5 and 197 rows.  dst_of with -1 entries and compact rows 0, 2, 4, ... (the odd rows of dH are named
    by nobody); h = NULL; row_mask with dH; g_at alone."""
    L, prec, dt, gs = _mode(mode)
    g = _gen(rows, 1)
    G = _randn(g, rows, D)
    keep = torch.rand(rows, generator=g) < 0.6
    keep[0] = True
    dst_of = _compact(keep, stride=2)
    K2 = 2 * int(keep.sum())
    h = _randn(g, K2, D).to(dt)
    row_mask = torch.where(keep, torch.tensor([1.0, 0.75])[torch.arange(rows) % 2], torch.zeros(rows))
    Gd, hd, dd, md = _dev(G), _dev(h), _dev(dst_of), _dev(row_mask)
    kept = dst_of >= 0
    tag = "rows=%d %s " % (rows, mode)
    named = torch.zeros(K2 + 3, dtype=torch.bool)
    named[dst_of[kept].long()] = True

    def check_dH(dH, rows_ref32, what):
        want = (rows_ref32 * gs).to(dt)
        _assert_normal(rows_ref32[kept], gs, dt, what)
        assert torch.equal(dH.cpu()[dst_of[kept].long()], want[kept]), what
        assert bool((dH.cpu()[~named] == SENT).all()), what + ": a row no token names was written"

    # dst_of with -1 entries, h, every output
    g_at, dH, dmask = _out_rows(rows, D, dt), _out_rows(K2, D, dt, fill=SENT), _out_rows(rows, 1, F32).view(-1)
    _prep_call(mode, Gd, hd, dd, None, g_at, dH, dmask, rows)
    r64, m64 = R.bwd_prep_ref(G, h, dst_of)
    r32, m32 = R.bwd_prep_ref(G, h, dst_of, dtype=F32)
    _cmp("bwd_prep", tag + "dmask", dmask[:rows], m64, m32)
    assert float(dmask[:rows].cpu()[~kept].abs().max() if bool((~kept).any()) else 0.0) == 0.0
    _same_rounding(tag + "g_at", g_at[:rows], Gd, gs, dt, G)
    check_dH(dH, r32, tag + "dH")
    for buf, n in ((g_at, rows), (dmask, rows)):
        _tail_untouched(buf, n, tag)
    # h = NULL: dmask is written as zeros
    dmask = _out_rows(rows, 1, F32).view(-1)
    _prep_call(mode, Gd, None, dd, None, None, None, dmask, rows)
    assert float(dmask[:rows].abs().max()) == 0.0 and bool((dmask[rows:] == SENT).all())
    # row_mask with dH (masked-dense form): dH = mask g, dmask unchanged by the mask
    dH, dmask = _out_rows(K2, D, dt, fill=SENT), _out_rows(rows, 1, F32).view(-1)
    _prep_call(mode, Gd, hd, dd, md, None, dH, dmask, rows)
    rm32, mm32 = R.bwd_prep_ref(G, h, dst_of, row_mask, dtype=F32)
    check_dH(dH, rm32, tag + "dH with row_mask")
    _cmp("bwd_prep", tag + "dmask with row_mask", dmask[:rows], m64, mm32)
    # g_at alone, dense
    g_at = _out_rows(rows, D, dt)
    _prep_call(mode, Gd, None, None, None, g_at, None, None, rows)
    _same_rounding(tag + "g_at alone", g_at[:rows], Gd, gs, dt, G)
    _tail_untouched(g_at, rows, tag)


# ------------------------------------------------------------------------------------------------------------------------------
# ln_bwd
# ------------------------------------------------------------------------------------------------------------------------------
def _ln_call(mode, dy, x, stats, w, base, base_at, dx, rows, g_at=None, h_next=None, dst_of_next=None, dmask_next=None, out3=None, s3=1.0,
             hi_only=0, expect=0):
    L, prec, dt, gs = _mode(mode)
    rc = L.dyt_unit_ln_bwd(ptr(dy), ptr(x), ptr(stats), ptr(w), ptr(base), ptr(base_at), ptr(dx), rows, ptr(g_at), ptr(h_next),
                           ptr(dst_of_next), ptr(dmask_next), gs, ptr(out3), s3, hi_only, prec, stream_ptr())
    assert rc == expect, (rc, L.dyt_last_error())


def _ln_inputs(rows, mode, seed):
    L, prec, dt, gs = _mode(mode)
    g = _gen(rows, seed)
    x = 1.5 * _randn(g, rows, D) + 0.2
    w = 1.0 + 0.3 * _randn(g, D)
    dy = (gs * 0.5 * _randn(g, rows, D)).to(dt)
    mean, rstd, stats = _stats(x)
    return g, x, w, dy, mean, rstd, stats


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 197])
def test_ln_bwd(rows, mode):
    """plain; base in place (dx == base); fused next-block prep; the fp16 stream form (base_at, dx = NULL); deliberately wrong stats."""
    L, prec, dt, gs = _mode(mode)
    g, x, w, dy, mean, rstd, stats = _ln_inputs(rows, mode, 2)
    xd, wd, dyd, sd = _dev(x), _dev(w), _dev(dy), _dev(stats)
    tag = "rows=%d %s " % (rows, mode)
    # plain
    dx = _out_rows(rows, D, F32)
    _ln_call(mode, dyd, xd, sd, wd, None, None, dx, rows)
    r64, _ = R.ln_bwd_kernel_ref(dy, x, mean, rstd, w, gs=gs)
    r32, _ = R.ln_bwd_kernel_ref(dy, x, mean, rstd, w, gs=gs, dtype=F32)
    _cmp("ln_bwd", tag + "plain dx", dx[:rows], r64, r32)
    _tail_untouched(dx, rows, tag)
    # base in place, with the next block's prep fused: g_at, <dx, h_next[dst_of_next]>
    base = _randn(g, rows, D)
    keep = torch.rand(rows, generator=g) < 0.6
    if rows > 1:
        keep[0] = True
    dst = _compact(keep)
    h_next = _randn(g, max(1, int(keep.sum())), D).to(dt)
    dx = _out_rows(rows, D, F32)
    dx[:rows] = _dev(base)
    g_at, dm = _out_rows(rows, D, dt), _out_rows(rows, 1, F32).view(-1)
    _ln_call(mode, dyd, xd, sd, wd, dx, None, dx, rows, g_at=g_at, h_next=_dev(h_next), dst_of_next=_dev(dst), dmask_next=dm)
    kw = dict(base=base, gs=gs, h_next=h_next, dst_of_next=dst)
    (b64, m64), (b32, m32) = R.ln_bwd_kernel_ref(dy, x, mean, rstd, w, **kw), R.ln_bwd_kernel_ref(dy, x, mean, rstd, w, dtype=F32, **kw)
    _cmp("ln_bwd", tag + "base in place dx", dx[:rows], b64, b32)
    _same_rounding(tag + "g_at", g_at[:rows], dx[:rows], gs, dt, b64)
    if bool(keep.any()):
        _cmp("ln_bwd", tag + "dmask_next", dm[:rows].cpu()[keep], m64[keep], m32[keep])
    assert float(dm[:rows].cpu()[~keep].abs().max() if bool((~keep).any()) else 0.0) == 0.0, tag + "dmask_next of a dropped token"
    for buf in (dx, g_at, dm):
        _tail_untouched(buf, rows, tag)
    # deliberately wrong statistics: the kernel uses the ones it is given
    bad_mean, bad_rstd = mean + 0.05, rstd * 1.1
    bad = torch.stack([bad_mean, bad_rstd], 1).contiguous()
    dx = _out_rows(rows, D, F32)
    _ln_call(mode, dyd, xd, _dev(bad), wd, None, None, dx, rows)
    p64, _ = R.ln_bwd_kernel_ref(dy, x, bad_mean, bad_rstd, w, gs=gs)
    p32, _ = R.ln_bwd_kernel_ref(dy, x, bad_mean, bad_rstd, w, gs=gs, dtype=F32)
    bound = _cmp("ln_bwd", tag + "perturbed stats dx", dx[:rows], p64, p32)
    assert float((p64 - r64).abs().max()) > 1000 * bound   # (the two sets of statistics are told apart)
    if prec == 0:
        return
    # the 16-bit stream: base_at in, g_at out, no fp32 row
    base_at = (gs * _randn(g, rows, D)).to(dt)
    g_at = _out_rows(rows, D, dt)
    _ln_call(mode, dyd, xd, sd, wd, None, _dev(base_at), None, rows, g_at=g_at)
    s64, _ = R.ln_bwd_kernel_ref(dy, x, mean, rstd, w, base_at=base_at, gs=gs)
    s32, _ = R.ln_bwd_kernel_ref(dy, x, mean, rstd, w, base_at=base_at, gs=gs, dtype=F32)
    _cmp16("ln_bwd", tag + "base_at -> g_at", g_at[:rows], gs, dt, s64, s32)
    _tail_untouched(g_at, rows, tag)


@pytest.mark.parametrize("hi_only", [0, 1])
@pytest.mark.parametrize("rows", [1, 5, 197])
def test_ln_bwd_split_operand(rows, hi_only):
    mode, s3 = "fp32h", 4096.0   # (a power of two, like dyt_ctx::split_gs)
    g, x, w, dy, mean, rstd, stats = _ln_inputs(rows, mode, 3)
    dx = _out_rows(rows, D, F32)
    out3 = torch.full((rows + 3, 2 * D), SENT, dtype=torch.float16)
    out3[:rows, :D if hi_only else 2 * D] = math.nan
    out3 = out3.to(DEV)
    _ln_call(mode, _dev(dy), _dev(x), _dev(stats), _dev(w), None, None, dx, rows, out3=out3, s3=s3, hi_only=hi_only)
    r64, _ = R.ln_bwd_kernel_ref(dy, x, mean, rstd, w)
    r32, _ = R.ln_bwd_kernel_ref(dy, x, mean, rstd, w, dtype=F32)
    tag = "rows=%d hi_only=%d " % (rows, hi_only)
    _cmp("ln_bwd", tag + "dx next to out3", dx[:rows], r64, r32)
    _split_check(tag + "out3", out3[:rows].cpu(), s3, bool(hi_only), dx[:rows])
    _tail_untouched(out3, rows, tag)


# ------------------------------------------------------------------------------------------------------------------------------
# ln_param_grad
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("rows", [1, 3, 31, 32, 33, 197])
def test_ln_param_grad(rows, mode):
    """32 rows per workgroup, four waves striding over them; out is accumulated into."""
    L, prec, dt, gs = _mode(mode)
    g, x, w, dy, mean, rstd, stats = _ln_inputs(rows, mode, 4)
    seed = _randn(g, 2 * D)
    out = torch.cat([seed, torch.full((3,), SENT)]).to(DEV)
    dyd, xd, sd = _dev(dy), _dev(x), _dev(stats)   # (held: a temporary's memory is handed to the next allocation)
    rc = L.dyt_unit_ln_param_grad(ptr(dyd), ptr(xd), ptr(sd), ptr(out), rows, gs, prec, stream_ptr())
    assert rc == 0, L.dyt_last_error()
    r64 = seed.double() + R.ln_param_grad_ref(dy, x, mean, rstd, gs)
    r32 = seed + R.ln_param_grad_ref(dy, x, mean, rstd, gs, dtype=F32)
    tag = "rows=%d %s " % (rows, mode)
    _cmp("ln_param_grad", tag + "d gamma", out[:D], r64[:D], r32[:D])
    _cmp("ln_param_grad", tag + "d beta", out[D:2 * D], r64[D:], r32[D:])
    assert bool((out[2 * D:] == SENT).all())


# ------------------------------------------------------------------------------------------------------------------------------
# tok_bwd
# ------------------------------------------------------------------------------------------------------------------------------
def _tok_inputs(B, mode, seed, pattern="mixed"):
    """One draw of everything a token backward can read; a case takes what its call form sets."""
    L, prec, dt, gs = _mode(mode)
    g = _gen(B, seed)
    M = B * NT
    keep = _keep_mask(g, B, pattern).reshape(M)
    c = dict(B=B, M=M, keep=keep, maskf=keep.float(), dst_of=_compact(keep), K=int(keep.sum()))
    c["u"] = 1.5 * _randn(g, M, D) + 0.2
    c["mean2"], c["rstd2"], c["stats2"] = _stats(c["u"])
    c["ln2_w"] = 1.0 + 0.3 * _randn(g, D)
    c["gate_w"] = 0.5 * _randn(g, D)
    c["soft"] = torch.sigmoid(1.5 * _randn(g, M))
    c["dmask"] = 2.0 * _randn(g, M) * c["maskf"]   # <g, h>: 0 for a dropped token
    c["dtok"] = torch.tensor([0.3, -0.7, 0.2])
    c["du"] = _randn(g, M, D)
    c["du_in_at"] = (gs * _randn(g, M, D)).to(dt)
    c["dA2"] = (gs * 0.5 * _randn(g, c["K"], D)).to(dt)
    c["dA2_dense"] = (gs * 0.5 * _randn(g, M, D)).to(dt)
    c["dA2_cls"] = (gs * 0.5 * _randn(g, B, D)).to(dt)
    c["g_cls"] = _randn(g, B, D)
    c["dad"] = (gs * 0.5 * _randn(g, M, D)).to(dt)
    c["sel"], c["dlg"] = _randn(g, B, 3, NP), 0.1 * _randn(g, B, 3, NP)   # user gradients [B, depth 3, 196]
    c["cat_dact"] = _randn(g, M, 64).clamp(min=0).to(dt)
    c["cat_ddz"] = (gs * 32.0 * 0.05 * _randn(g, M, 64)).to(dt)        # carries gs and a lift of 2^5
    c["gate_seed"] = 0.1 * _randn(g, D + 1)
    return c


PTRS = ("dA2", "dst_of", "ln2_w", "gate_w", "soft", "maskf", "dmask", "dtok", "dad", "g_cls", "cat_dact", "cat_ddz", "cat_ddz_dscale",
        "branch_scale", "du_in_at")


def _tok_run(mode, c, tag, ref_kw, write_du=1, with_du=True, with_du_at=None, du3=None, check=True):
    """One dyt_unit_tok_bwd call whose fields are the keyword arguments of R.tok_bwd_ref (the same CPU tensors, uploaded), plus the
    output buffers; compares every output the form produces.  Returns the device outputs and the references."""
    L, prec, dt, gs = _mode(mode)
    M, B = c["M"], c["B"]
    a = _lib.UnitTokBwdArgs()
    hold = []

    def put(name, t):
        t = _dev(t)
        hold.append(t)
        setattr(a, name, t.data_ptr())
        return t
    for k in PTRS:
        if ref_kw.get(k) is not None:
            put(k, ref_kw[k])
    put("u", c["u"])
    if ref_kw.get("dA2") is not None:
        put("stats2", c["stats2"])
    for name in ("dtoken_select", "dtoken_logits"):   # the layer-1 slice of a [B, 3, 196] user tensor: pointer offset, stride 3 * 196
        if ref_kw.get(name) is not None:
            full = c["sel" if name == "dtoken_select" else "dlg"]
            assert torch.equal(full[:, 1], ref_kw[name])
            full = _dev(full)
            hold.append(full)
            setattr(a, name, full.data_ptr() + NP * 4)
            a.out_stride = 3 * NP
    a.training, a.tau = int(ref_kw.get("training", 0)), float(ref_kw.get("tau", 1.0))
    a.cat_scale, a.cat_ddz_scale = 0.1, float(ref_kw.get("cat_ddz_scale", 0.0))
    a.M, a.write_du, a.gs = M, write_du, gs
    reads_du = write_du and ref_kw.get("g_cls") is None and ref_kw.get("du_in_at") is None
    du = du_at = du3_buf = None
    if with_du:
        du = _out_rows(M, D, F32, fill=math.nan if write_du else SENT)
        if reads_du:
            du[:M] = _dev(ref_kw["du"])
        a.du = du.data_ptr()
    if with_du_at is None:
        with_du_at = prec == 1 and bool(write_du)
    if with_du_at:
        du_at = _out_rows(M, D, dt)
        a.du_at = du_at.data_ptr()
    if du3 is not None:
        du3_buf = torch.full((M + 3, 2 * D), SENT, dtype=torch.float16)
        du3_buf[:M, :D if du3 else 2 * D] = math.nan
        du3_buf = du3_buf.to(DEV)
        a.du3, a.du3_scale, a.du3_hi_only = du3_buf.data_ptr(), 4096.0, int(du3)
    d_gate = torch.cat([c["gate_seed"], torch.full((3,), SENT)]).to(DEV)
    rc = L.dyt_unit_tok_bwd(ctypes.byref(a), ptr(d_gate), prec, stream_ptr())
    assert rc == 0, (tag, rc, L.dyt_last_error())
    torch.cuda.synchronize()
    kw = dict(ref_kw, mean2=c["mean2"], rstd2=c["rstd2"], gs=gs)
    r64, r32 = R.tok_bwd_ref(M, c["u"], **kw), R.tok_bwd_ref(M, c["u"], dtype=F32, **kw)
    out = dict(du=du, du_at=du_at, du3=du3_buf, d_gate=d_gate, r64=r64, r32=r32)
    tag = "%s B=%d %s " % (tag, B, mode)
    assert bool((d_gate[D + 1:] == SENT).all()), tag + "d_gate[769:]"
    for buf in (du, du_at, du3_buf):
        if buf is not None:
            _tail_untouched(buf, M, tag)
    if not check:
        return out
    if not write_du:
        assert du is None or bool((du == SENT).all()), tag + "du written although write_du = 0"
    elif du is not None:
        _cmp("tok_bwd", tag + "du", du[:M], r64[0], r32[0])
        if du_at is not None:
            _same_rounding(tag + "du_at", du_at[:M], du[:M], gs, dt, r64[0])
        if du3_buf is not None:
            _split_check(tag + "du3", du3_buf[:M].cpu(), 4096.0, bool(du3), du[:M])
    elif du_at is not None:
        _cmp16("tok_bwd", tag + "du_at", du_at[:M], gs, dt, r64[0], r32[0])
    if ref_kw.get("gate_w") is not None:
        s64, s32 = c["gate_seed"].double() + r64[1], c["gate_seed"] + r32[1]
        _cmp("tok_bwd+reduce", tag + "d_gate[0:768]", d_gate[:D], s64[:D], s32[:D])
        _cmp("tok_bwd+reduce", tag + "d_gate[0:769]", d_gate[:D + 1], s64, s32)
    else:
        assert torch.equal(d_gate[:D + 1].cpu(), c["gate_seed"]), tag + "d_gate written without a gate"
    return out


def _student(c, **over):
    """The student block l > 0, compact (backward.hip: the per-token tail), as keyword arguments of the reference."""
    kw = dict(du=c["du"], dA2=c["dA2"], dst_of=c["dst_of"], ln2_w=c["ln2_w"], gate_w=c["gate_w"], soft=c["soft"], maskf=c["maskf"],
              dmask=c["dmask"], dtok=c["dtok"], training=1, tau=5.0)
    kw.update(over)
    return {k: v for k, v in kw.items() if v is not None}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B", [1, 2, 3])
def test_tok_bwd_student_block(B, mode):
    """Case 1 (B = 1: 7 workgroups, the last with 5 tokens; B = 2: an image boundary inside a workgroup; B = 3), case 3 (eval: no
    division by tau), case 4 (first block: only d_gate changes), case 5 (teacher: only du changes), case 6 (dense)."""
    c = _tok_inputs(B, mode, 10)
    one = _tok_run(mode, c, "student compact", _student(c))
    ev = _tok_run(mode, c, "eval", _student(c, training=0))
    assert float((ev["r64"][0] - one["r64"][0]).abs().max()) > 0.01   # (tau = 5 is told from tau = 1 far above any bound)
    _tok_run(mode, c, "first block", _student(c, du=None, dA2=None, dst_of=None), write_du=0)
    _tok_run(mode, c, "teacher", _student(c, gate_w=None, soft=None, dmask=None, dtok=None))
    _tok_run(mode, c, "dense", _student(c, dA2=c["dA2_dense"], dst_of=None))


@pytest.mark.parametrize("mode", MODES)
def test_tok_bwd_user_gradients_index_their_layer(mode):
    """Case 2: dtoken_select / dtoken_logits with out_stride = 3 * 196 and the pointers offset to layer 1: index b * out_stride + n - 1."""
    c = _tok_inputs(3, mode, 11)
    _tok_run(mode, c, "user gradients", _student(c, dtok=None, dtoken_select=c["sel"][:, 1].contiguous(), dtoken_logits=c["dlg"][:, 1].contiguous()))


@pytest.mark.parametrize("mode", MODES + ["fp16 stream"])
def test_tok_bwd_cls_only_tail(mode):
    """Case 7: g_cls [B, 768], dA2 [B, 768].  Without a gate (the teacher's tail) the patch rows come out exactly zero; with one (the
    student's, dmask = NULL) they are dlogit w_gate; the cls rows are g_cls + LN2bwd either way.  "fp16 stream": du = NULL, du_at only."""
    stream = mode == "fp16 stream"
    mode = "fp16" if stream else mode
    L, prec, dt, gs = _mode(mode)
    c = _tok_inputs(3, mode, 12)
    cls = (torch.arange(c["M"]) % NT) == 0
    base = dict(g_cls=c["g_cls"], dA2=c["dA2_cls"], ln2_w=c["ln2_w"])
    for name, kw in (("tail, no gate", base),
                     ("tail, gate", dict(base, gate_w=c["gate_w"], soft=c["soft"], maskf=c["maskf"], dtok=c["dtok"], training=1, tau=5.0))):
        o = _tok_run(mode, c, name, kw, with_du=not stream)
        got = (o["du_at"][:c["M"]].cpu().double() / gs) if stream else o["du"][:c["M"]].cpu().double()
        r64, r32 = o["r64"][0], o["r32"][0]
        tag = "%s %s " % (name, "fp16 stream" if stream else mode)
        if "gate_w" not in kw:
            assert float(got[~cls].abs().max()) == 0.0, tag + "patch rows are not exactly zero"
            if not stream:
                assert float(o["du_at"][:c["M"]].cpu()[~cls].abs().max() if o["du_at"] is not None else 0.0) == 0.0
        elif not stream:
            want64 = o["r64"][2].view(-1, 1) * c["gate_w"].double()
            want32 = o["r32"][2].view(-1, 1) * c["gate_w"]
            _cmp("tok_bwd", tag + "patch rows = dlogit w_gate", o["du"][:c["M"]].cpu()[~cls], want64[~cls], want32[~cls])
        if not stream:
            _cmp("tok_bwd", tag + "cls rows", o["du"][:c["M"]].cpu()[cls], r64[cls], r32[cls])


@pytest.mark.parametrize("mode", MODES)
def test_tok_bwd_cat_correction(mode):
    """Case 8: the saved MLP output includes the adapter's term; <cat_dact, cat_ddz> cat_ddz_scale *cat_ddz_dscale (a device word, 2^-5)
    is taken off dmask for the kept tokens.  The correction is about a tenth of dmask; dropped tokens are unaffected bit for bit."""
    L, prec, dt, gs = _mode(mode)
    c = _tok_inputs(3, mode, 13)
    czs = 1.0 / ((1.0 / 0.9) * gs)   # 1 / (inv_keep gs), as backward.hip forms it
    cat = dict(cat_dact=c["cat_dact"], cat_ddz=c["cat_ddz"], cat_ddz_scale=czs, cat_ddz_dscale=torch.tensor([2.0 ** -5]))
    corr = (c["cat_dact"].double() * c["cat_ddz"].double()).sum(-1) * czs * 2.0 ** -5
    ratio = float(corr[c["keep"]].abs().mean() / c["dmask"][c["keep"]].abs().mean())
    assert 0.05 < ratio < 0.2, ratio
    plain = _tok_run(mode, c, "no cat", _student(c), check=False)
    o = _tok_run(mode, c, "cat", _student(c, **cat))
    bound = 4.0 * float((o["r32"][0].double() - o["r64"][0]).abs().max()) + 4.0 * ulp(o["r64"][0].abs().max())
    assert float((plain["r64"][0] - o["r64"][0]).abs().max()) > 100 * bound   # (dropping the correction cannot hide under the floor)
    dropped = ~c["keep"]
    assert torch.equal(o["du"][:c["M"]].cpu()[dropped], plain["du"][:c["M"]].cpu()[dropped]), "a dropped token saw the cat correction"
    nodev = _tok_run(mode, c, "cat, no device word", _student(c, **dict(cat, cat_ddz_scale=czs * 2.0 ** -5, cat_ddz_dscale=None)))
    assert torch.equal(nodev["du"], o["du"]) and torch.equal(nodev["d_gate"], o["d_gate"])


@pytest.mark.parametrize("mode", MODES)
def test_tok_bwd_branch_scale(mode):
    """Case 9: stochastic depth [0, 1/0.9, 1] over three images (every image with a random keep mask): image 0's LN2 and dmask terms
    vanish exactly -- its rows equal, bit for bit, a call without dA2 and dmask."""
    c = _tok_inputs(3, mode, 14, pattern="random")
    bs = torch.tensor([0.0, 1.0 / 0.9, 1.0])
    o = _tok_run(mode, c, "branch_scale", _student(c, branch_scale=bs))
    z = _tok_run(mode, c, "no MLP branch", _student(c, dA2=None, dst_of=None, dmask=None), check=False)
    assert torch.equal(o["du"][:NT], z["du"][:NT]), "image 0 (branch_scale 0) still sees its LN2 or dmask term"
    if o["du_at"] is not None:
        assert torch.equal(o["du_at"][:NT], z["du_at"][:NT])
    one = _tok_run(mode, c, "branch_scale all 1", _student(c, branch_scale=torch.ones(3)), check=False)
    assert float((one["r64"][0][NT:2 * NT] - o["r64"][0][NT:2 * NT]).abs().max()) > 0.01   # (1 / 0.9 is told from 1)


@pytest.mark.parametrize("mode", MODES16)
def test_tok_bwd_16bit_adapter_dgrad_and_stream(mode):
    """Case 10: dad (the adapter dgrad as a 16-bit gs-scaled operand) with du and du_at; and the fp16 mode's stream form: du = NULL,
    the incoming gradient in du_in_at, the result in du_at alone."""
    c = _tok_inputs(2, mode, 15)
    _tok_run(mode, c, "dad + du_at", _student(c, dad=c["dad"]))
    _tok_run(mode, c, "stream", _student(c, du=None, du_in_at=c["du_in_at"], dad=c["dad"]), with_du=False)
    _tok_run(mode, c, "stream + fp32 copy", _student(c, du=None, du_in_at=c["du_in_at"], dad=c["dad"]))


@pytest.mark.parametrize("hi_only", [0, 1])
def test_tok_bwd_split_operand(hi_only):
    """Case 11: du3, the proj dgrad's split operand (IEEE-half library, precision 0)."""
    c = _tok_inputs(2, "fp32h", 16)
    _tok_run("fp32h", c, "du3 hi_only=%d" % hi_only, _student(c), du3=hi_only)


# ------------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_bad_arguments_are_refused_and_the_library_stays_usable(mode):
    L, prec, dt, gs = _mode(mode)
    rows = 4
    g, x, w, dy, mean, rstd, stats = _ln_inputs(rows, mode, 5)
    xd, wd, dyd, sd = _dev(x), _dev(w), _dev(dy), _dev(stats)
    dx = _out_rows(rows, D, F32)
    out = torch.zeros(2 * D, device=DEV)
    o3 = torch.zeros(rows, 2 * D, dtype=torch.float16, device=DEV)

    def refused(rc, needle):
        msg = L.dyt_last_error().decode()
        assert rc == ERR_ARG and needle in msg, (rc, msg)
    S = stream_ptr()
    refused(L.dyt_unit_bwd_prep(None, None, None, None, None, None, ptr(dx), rows, gs, prec, S), "dyt_unit_bwd_prep")
    refused(L.dyt_unit_bwd_prep(ptr(xd), None, None, None, None, None, None, rows, gs, prec, S), "no output")
    refused(L.dyt_unit_bwd_prep(ptr(xd), None, None, None, None, None, ptr(dx), rows, gs, 2, S), "precision 2")
    refused(L.dyt_unit_ln_bwd(None, ptr(xd), ptr(sd), ptr(wd), None, None, ptr(dx), rows, None, None, None, None, gs, None, 1.0, 0, prec, S), "NULL")
    refused(L.dyt_unit_ln_bwd(ptr(dyd), ptr(xd), None, ptr(wd), None, None, ptr(dx), rows, None, None, None, None, gs, None, 1.0, 0, prec, S), "NULL")
    refused(L.dyt_unit_ln_bwd(ptr(dyd), ptr(xd), ptr(sd), ptr(wd), None, None, ptr(dx), rows, None, None, None, None, gs, None, 1.0, 0, -1, S), "precision -1")
    refused(L.dyt_unit_ln_bwd(ptr(dyd), ptr(xd), ptr(sd), ptr(wd), None, None, ptr(dx), rows, None, None, None, None, gs, ptr(o3), 1.0, 0, 1, S), "out3")
    refused(L.dyt_unit_ln_param_grad(ptr(dyd), ptr(xd), ptr(sd), None, rows, gs, prec, S), "NULL")
    refused(L.dyt_unit_ln_param_grad(ptr(dyd), ptr(xd), ptr(sd), ptr(out), rows, gs, 3, S), "precision 3")
    c = _tok_inputs(1, mode, 17)
    M = c["M"]
    du, du3 = _dev(c["du"]), torch.zeros(M, 2 * D, dtype=torch.float16, device=DEV)
    ud, dg = _dev(c["u"]), torch.zeros(D + 1, device=DEV)

    def tok(precision=prec, **f):
        a = _lib.UnitTokBwdArgs()
        a.M, a.write_du, a.gs, a.tau, a.u, a.du = M, 1, (gs if precision else 1.0), 5.0, ud.data_ptr(), du.data_ptr()
        for k, v in f.items():
            setattr(a, k, v.data_ptr() if torch.is_tensor(v) else v)
        return L.dyt_unit_tok_bwd(ctypes.byref(a), ptr(dg), precision, S)
    refused(L.dyt_unit_tok_bwd(None, ptr(dg), prec, S), "NULL")
    refused(tok(M=M - 1), "multiple of 197")
    refused(tok(M=0), "multiple of 197")
    refused(tok(precision=2), "precision 2")
    refused(tok(du3=du3), "du3")
    refused(tok(du=None, du_at=None), "write_du without du or du_at")
    refused(tok(gate_w=_dev(c["gate_w"])), "soft")
    refused(tok(dA2=_dev(c["dA2"])), "stats2")
    refused(tok(u=None, dA2=_dev(c["dA2"])), "u is NULL")
    before = du.clone()
    assert tok() == 0, L.dyt_last_error()   # a later valid call on the same library succeeds (no term set: du comes back as it went in)
    torch.cuda.synchronize()
    assert torch.equal(du, before)
    _ln_call(mode, dyd, xd, sd, wd, None, None, dx, rows)
    assert bool(torch.isfinite(dx[:rows]).all())
