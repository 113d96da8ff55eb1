"""Unit tests of the attention kernels (csrc/attention_16.hip, attention_exact.hip, attention_split.hip, attention_v2.hip), each route of csrc/attn_route.h launched alone through
dyt_unit_attn_fwd / dyt_unit_attn_bwd and compared element by element with the fp64 references of tests/attn_refs.py (pinned to torch
autograd by tests/test_attn_refs_host.py).  DESIGN.md 7v holds the derivations.

The rule.  fp32 outputs of the exact kernels (AF_EXACT, AB_EXACT: out, lse, delta, dqkv) and the fp32 row statistics of every kernel (lse;
delta where a route stores it) are held to ``_cmp`` of tests/test_gpu_step_tail.py, imported unchanged: |gpu - fp64| <= 4 max|fp32_cpu -
fp64| + 4 ulp(max|fp64|), the fp32 CPU restatement on the same inputs being the floor.  Every other stored element e is held to its own
allowance A(e) = that bound + one term per rounding point of the kernel (attn_refs.fwd_allowance / bwd_allowance / lse_allowance): a unit
roundoff times an fp64 abs-product of the reference.  The share |gpu - fp64| / A is printed per case and its worst kept per kernel.
The backward is tested in isolation: lse = the fp64 lse rounded to fp32, out = the fp64 out rounded to the operand type.
Every output buffer starts as NaN with finite sentinel rows behind it; what a route does not write (lse of a *_NOSAVE route, delta of AB_V2,
the lo half of an out_hi_only image, anything of a refused call) must keep its bits.

Shapes: B = 1 (one head per workgroup; every family), 2 (two images' row offsets), 22 (264 pairs: 8 of the 256 persistent workgroups take a
second head) with the randn and spike families, and 65 (780 pairs: a fourth head, the first reuse of the round-5 backward's slot triple) for
AF_V2 / AB_V2 on randn.  The split and fp8-image routes run where the product runs them, on the IEEE-half library.
The route a call takes is attn_fwd_route / attn_bwd_route restated (attn_refs.fwd_route / bwd_route) and asserted in every call helper.

Not reachable from here: the kernels next to a concurrently running stream, the launchers' dbg_skip, the ABL / SETPRIO probe instances."""
import contextlib
import ctypes
import functools
import math
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import _lib  # noqa: E402
import attn_refs as R  # noqa: E402
import rowfwd_refs as RF  # noqa: E402
from _lib import stream_ptr  # noqa: E402
from test_gpu_row_bwd import SENT, _dev, _mode, _out_rows, _tail_untouched  # noqa: E402
from test_gpu_step_tail import WORST, _cmp  # noqa: E402   (the project's comparison rule, unchanged)

DEV = "cuda:0"
F16, F32, F64 = torch.float16, torch.float32, torch.float64
NT, NH, HD, D = R.NT, R.NH, R.HD, R.D
ERR = -1          # DYT_ERR_ARG, and what launch_attn_fwd / launch_attn_bwd return for a refused route
SEED = 5
GS_UNIT = 4096.0  # attention_split.hip launch_attn_bwd_split: the lift of dout in the split backward kernels when no dqkv3 is asked for
WORST_A = {}      # kernel -> (worst share of the allowance, case)
_SWITCHES = {}    # library -> (DYT_OPT_ATTN_V2, DYT_OPT_ATTN_BWD_FUSED) as _switches() last set them (the libraries' defaults: 3, 1)
T0 = time.time()
MODES16 = ["bf16", "fp16"]
BATCHES = [1, 2, 22]


@pytest.fixture(scope="module", autouse=True)
def _worst_table():
    yield
    print("\nworst error / floor per kernel (fp32 outputs under _cmp), worst share of the derived allowance (every other output):")
    for k in sorted(set(WORST) | set(WORST_A)):
        if k.startswith("attn") or k in WORST_A:
            a = "%8.2f   (%s)" % WORST[k] if k in WORST else "       -"
            b = "%6.3f   (%s)" % WORST_A[k] if k in WORST_A else "     -"
            print("  %-26s %s\n  %-26s %s" % (k, a, "", b))
    print("tests/test_gpu_unit_attention.py: %.1f s wall" % (time.time() - T0))


@contextlib.contextmanager
def _switches(L, v2=3, fused=1):
    """The process-wide switches for one case; the defaults come back whatever happens."""
    before = _SWITCHES.get(id(L), (3, 1))
    try:
        _lib.check(L.dyt_set_global_option(_lib.OPT_ATTN_V2, v2), L)
        _lib.check(L.dyt_set_global_option(_lib.OPT_ATTN_BWD_FUSED, fused), L)
        _SWITCHES[id(L)] = (v2, fused)
        yield
    finally:
        L.dyt_set_global_option(_lib.OPT_ATTN_V2, before[0])
        L.dyt_set_global_option(_lib.OPT_ATTN_BWD_FUSED, before[1])
        L.dyt_set_global_option(_lib.OPT_F32_SPLIT16, 0)
        _SWITCHES[id(L)] = before


def _families(B):
    return R.FAMILIES if B == 1 else ("randn", "spike")


def _held(kernel, what, got, ref64, A):
    s = R.share(got, ref64, A)
    print("[%s] %s: worst |gpu - fp64| / allowance %.3f" % (kernel, what, s))
    if s > WORST_A.get(kernel, (-1.0, ""))[0]:
        WORST_A[kernel] = (s, what)
    assert s <= 1.0, "[%s] %s: |gpu - fp64| is %.3f times its derived allowance" % (kernel, what, s)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same_bits(a, b, what):
    n = int((_bits(a) != _bits(b)).sum())
    assert n == 0, "%s: %d elements differ" % (what, n)


def _all_nan(t, what):
    assert bool(torch.isnan(t.float()).all()), what + ": a buffer this route does not write was written"


# ---- references, computed once per (family, B, operand type, dout kind) ----------------------------------------------------------
@functools.lru_cache(maxsize=6)
def _ref(family, B, dt, dout_kind="randn", fwd_only=False):
    """Inputs rounded to the operand type dt (fp32: as they are) and everything the comparisons need, on the CPU."""
    q, k, v, dout = R.make_inputs(family, B, SEED, dout_kind)
    if dt != F32:
        q, k, v, dout = (x.to(dt).float() for x in (q, k, v, dout))
    R.check_family(family, q, k)
    c = dict(q=q, k=k, v=v, dout=dout, B=B, dt=dt)
    c["f64"], c["f32"] = R.attn_fwd_ref(q, k, v), R.attn_fwd_ref(q, k, v, F32)
    if not fwd_only:
        c["out_given"] = c["f64"][0].to(dt).float()   # what the backward is handed: the fp64 out rounded to the operand type
        c["lse_given"] = c["f64"][1].float()
        c["b64"] = R.attn_bwd_ref(q, k, v, c["out_given"], dout, lse=c["lse_given"])
        c["b32"] = R.attn_bwd_ref(q, k, v, c["out_given"], dout, F32, lse=c["lse_given"])
    return c


def _op(x, dt):
    """CPU fp32 tensor -> device operand of type dt."""
    return _dev(x.to(dt))


# ---- call helpers ----------------------------------------------------------------------------------------------------------------
def _fwd(L, prec, B, expect, **f):
    """One dyt_unit_attn_fwd call; tensors by field name.  `expect`: the route it must take under the switches in force.  Returns the
    return code."""
    v2, _ = _SWITCHES.get(id(L), (3, 1))
    planes = f.get("q_hi") is not None
    route = R.fwd_route(prec, split=bool(f.get("split16")), out=f.get("out") is not None, out3=f.get("out3") is not None, planes=planes,
                        saved=any(f.get(n) is not None for n in ("q16", "k16", "v16")), o16=f.get("o16") is not None,
                        out3_f8=bool(f.get("out3_f8")), parts=f.get("parts", 3), lse_optional=bool(f.get("lse_optional")), v2=v2)
    assert route == expect, "this call would run %s, not %s" % (route, expect)
    a = _lib.UnitAttnFwdArgs()
    a.parts, a.batch, a.planar = 3, B, int(planes)
    for n, val in f.items():
        setattr(a, n, val.data_ptr() if torch.is_tensor(val) else (int(val) if val is not None else None))
    rc = L.dyt_unit_attn_fwd(ctypes.byref(a), prec, stream_ptr())
    torch.cuda.synchronize()
    return rc


def _bwd(L, prec, B, expect, **f):
    v2, fused = _SWITCHES.get(id(L), (3, 1))
    route = R.bwd_route(prec, split=bool(f.get("split16")), grad_parts=f.get("grad_parts", 3), out_strided=f.get("out_ld", 0) not in (0, D),
                        v2=v2, fused=fused)
    assert route == expect, "this call would run %s, not %s" % (route, expect)
    a = _lib.UnitAttnBwdArgs()
    a.grad_parts, a.q_tiles, a.batch, a.s3 = 3, 7, B, 1.0
    for n, val in f.items():
        setattr(a, n, val.data_ptr() if torch.is_tensor(val) else val)
    rc = L.dyt_unit_attn_bwd(ctypes.byref(a), prec, stream_ptr())
    torch.cuda.synchronize()
    return rc


def _ok(L, rc, what=""):
    assert rc == 0, (what, rc, L.dyt_last_error())


def _refused(L, rc, needle, what=""):
    msg = L.dyt_last_error().decode()
    assert rc == ERR and needle in msg, (what, rc, msg, needle)


def _fwd_bufs(B, dt):
    return _out_rows(B * NT, D, dt), _out_rows(B * NH, NT, F32)


def _check_fwd_stats(kernel, tag, c, lse, exp2_form=False, ds=None):
    H = c["B"] * NH
    _tail_untouched(lse, H, tag + "lse")
    if not exp2_form and ds is None:
        _cmp(kernel, tag + "lse", lse[:H], c["f64"][1], c["f32"][1])
    else:
        A = R.lse_allowance(c["q"], c["k"], R.cmp_bound(c["f64"][1], c["f32"][1]), exp2_form, ds)
        _held(kernel, tag + "lse", lse[:H], c["f64"][1], A)


def _out_heads(out, B):
    return R.to_heads(out[:B * NT].detach().float().cpu(), B)


# ==================================================================================================================================
# forward, 16-bit kernels: AF_16 (round 4), AF_V2 / AF_V2_NOSAVE (round 5)
# ==================================================================================================================================
FWD16 = {"AF_16": ("attn_fwd_bf16", 2), "AF_V2": ("attn_fwd_v2", 3)}   # route -> (kernel, DYT_OPT_ATTN_V2)


def _run_fwd16(L, route, c, dt, tag):
    kernel, v2 = FWD16[route]
    B = c["B"]
    q, k, v = (_op(c[n], dt) for n in "qkv")
    out, lse = _fwd_bufs(B, dt)
    with _switches(L, v2=v2):
        _ok(L, _fwd(L, 1, B, route, q=q, k=k, v=v, out=out, lse=lse), tag)
        _tail_untouched(out, B * NT, tag + "out")
        u, t = R.unit(dt)
        A = R.fwd_allowance(c["v"], c["f64"][2], c["f64"][0], R.cmp_bound(c["f64"][0], c["f32"][0]), u, t, store_dt=dt)
        _held(kernel, tag + "out", _out_heads(out, B), c["f64"][0], A)
        _check_fwd_stats(kernel, tag, c, lse, exp2_form=route == "AF_V2")
        if route == "AF_V2":   # the no-save twin: the same output bits, lse untouched
            out2, lse2 = _fwd_bufs(B, dt)
            _ok(L, _fwd(L, 1, B, "AF_V2_NOSAVE", q=q, k=k, v=v, out=out2, lse=lse2, lse_optional=1), tag)
            _same_bits(out2, out, tag + "AF_V2_NOSAVE out vs AF_V2")
            _all_nan(lse2[:B * NH], tag + "AF_V2_NOSAVE lse")
            _tail_untouched(lse2, B * NH, tag + "lse")
    return out


@pytest.mark.parametrize("mode", MODES16)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("route", sorted(FWD16))
def test_forward_16bit(route, B, mode):
    L, _, dt, _ = _mode(mode)
    for family in _families(B):
        _run_fwd16(L, route, _ref(family, B, dt), dt, "%s %s B=%d %s: " % (route, mode, B, family))


@pytest.mark.parametrize("mode", MODES16)
def test_forward_v2_fourth_head_per_workgroup(mode):
    L, _, dt, _ = _mode(mode)
    _run_fwd16(L, "AF_V2", _ref("randn", 65, dt, "randn", True), dt, "AF_V2 %s B=65 randn: " % mode)


# ==================================================================================================================================
# forward, exact fp32 kernel
# ==================================================================================================================================
@pytest.mark.parametrize("mode", ["fp32", "fp32h"])
@pytest.mark.parametrize("B", [1, 2])
def test_forward_exact(B, mode):
    L, prec, _, _ = _mode(mode)
    for family in R.FAMILIES:
        c = _ref(family, B, F32)
        tag = "AF_EXACT %s B=%d %s: " % (mode, B, family)
        out, lse = _fwd_bufs(B, F32)
        with _switches(L):
            _ok(L, _fwd(L, prec, B, "AF_EXACT", q=_dev(c["q"]), k=_dev(c["k"]), v=_dev(c["v"]), out=out, lse=lse), tag)
        _tail_untouched(out, B * NT, tag + "out")
        _cmp("attn_fwd_f32", tag + "out", _out_heads(out, B), c["f64"][0], c["f32"][0])
        _check_fwd_stats("attn_fwd_f32", tag, c, lse)


# ==================================================================================================================================
# forward, split kernels (IEEE-half library, precision 0): AF_SPLIT_F32 / _P3 / _P1, AF_V2_F8 and their no-save twins
# ==================================================================================================================================
def _planes(x):
    hi, lo = RF.split3_image_ref(x.reshape(-1, HD))
    return hi.reshape(x.shape), lo.reshape(x.shape)


def _image_cap(v64, what, scale=1.0):
    """Elements below 2^-14 are left out of the image comparisons; at most 1 % of a tensor, asserted on the fp64 reference."""
    left = float(((v64.double() * scale).abs() < 2.0 ** -14).double().mean())
    assert left <= 0.01, "%s: %.2e of the reference is below 2^-14: choose other inputs" % (what, left)


def _check_hi_lo(tag, v32, hi, lo=None):
    """[hi | lo] planes of store4_split3 against the fp32 values of a second launch: hi is bit for bit half(v); hi + lo is within
    2^-21 |v| + 2^-25 (the second term: lo = half(v - hi) of an element below 2^-3 is subnormal, spacing 2^-24)."""
    v32 = v32.detach().cpu().float()
    n = v32.abs().double() >= 2.0 ** -14
    assert float(v32.abs().max()) <= 65504 / 2, tag
    want = v32.to(F16)
    hi = hi.detach().cpu()
    assert bool(torch.isfinite(hi.float()).all()), tag + "hi plane not fully written"
    bad = int((_bits(hi)[n] != _bits(want)[n]).sum())
    assert bad == 0, tag + "hi differs from half(v) in %d elements" % bad
    if lo is not None:
        lo = lo.detach().cpu()
        assert bool(torch.isfinite(lo.float()).all()), tag + "lo plane not fully written"
        excess = float((((hi.double() + lo.double()) - v32.double()).abs() - 2.0 ** -21 * v32.double().abs() - 2.0 ** -25)[n].max())
        assert excess <= 0.0, tag + "hi + lo off by %.3e more than 2^-21 |v| + 2^-25" % excess


def _check_f8(tag, v32, img):
    """The [hi16 | e4m3(hi) | e4m3(lo 2^12)] image of store4_split_f8 against the fp32 values v32."""
    v32 = v32.detach().cpu().float()
    n = v32.abs().double() >= 2.0 ** -14
    h16, h8, l8 = RF.f8_image_parts(img)
    want, s_hi, s_lo = RF.f8_sources_ref(v32)
    assert int((_bits(h16)[n] != _bits(want)[n]).sum()) == 0, tag + "f8 image: hi16 differs from half(v)"
    for name, byt, src in (("e4m3(hi)", h8, s_hi), ("e4m3(lo 2^12)", l8, s_lo)):
        dec = RF.e4m3_decode(byt)
        assert bool(torch.isfinite(dec).all()), tag + name + ": NaN byte"
        worst = float(((dec - src).abs() / RF.e4m3_half_step(src))[n].max())
        print("[f8] %s%s: worst |decoded - source| / half step %.3f" % (tag, name, worst))
        assert worst <= 1.0, tag + name + ": more than half an e4m3 step from its source (%.3f)" % worst


def _img_buf(rows, dt=F16, fill=math.nan):
    return _out_rows(rows, 2 * D, dt, fill=fill)


@pytest.mark.parametrize("B", BATCHES)
def test_forward_split_three_part(B):
    """AF_SPLIT_F32 on fp32 q / k / v and AF_SPLIT_P3 on their hi / lo planes: out, lse; the no-save twins; out3 in both image forms, o16 and
    q16 / k16 / v16 against the fp32 values."""
    L, prec, _, _ = _mode("fp32h")
    M, H = B * NT, B * NH
    for family in _families(B):
        c = _ref(family, B, F32)
        q, k, v = (_dev(c[n]) for n in "qkv")
        pl = {n: _planes(c[n]) for n in "qkv"}
        ph = {n + "_hi": _dev(pl[n][0]) for n in "qkv"}
        ph.update({n + "_lo": _dev(pl[n][1]) for n in "qkv"})
        ds = R.score_err3(c["q"], c["k"])
        A = R.fwd_allowance(c["v"], c["f64"][2], c["f64"][0], R.cmp_bound(c["f64"][0], c["f32"][0]), R.SPLIT_U, 2.0 ** -25, ds=ds, t_v=2.0 ** -25)
        outs, lses = {}, {}
        with _switches(L):
            for route, ops in (("AF_SPLIT_F32", dict(q=q, k=k, v=v)), ("AF_SPLIT_P3", ph)):
                tag = "%s B=%d %s: " % (route, B, family)
                out, lse = _fwd_bufs(B, F32)
                _ok(L, _fwd(L, prec, B, route, split16=1, out=out, lse=lse, **ops), tag)
                _tail_untouched(out, M, tag + "out")
                _held("attn_fwd_split<3>", tag + "out", _out_heads(out, B), c["f64"][0], A)
                _check_fwd_stats("attn_fwd_split<3>", tag, c, lse, ds=ds)
                out2, lse2 = _fwd_bufs(B, F32)
                _ok(L, _fwd(L, prec, B, route + "_NOSAVE", split16=1, out=out2, lse=lse2, lse_optional=1, **ops), tag)
                _same_bits(out2, out, tag + "no-save twin")
                _all_nan(lse2[:H], tag + "no-save lse")
                outs[route], lses[route] = out, lse
            print("AF_SPLIT_P3 on split3_image_ref planes vs AF_SPLIT_F32 B=%d %s: bit-equal %s" % (B, family, bool(torch.equal(outs["AF_SPLIT_P3"], outs["AF_SPLIT_F32"]))))
            if family not in ("randn", "spike"):
                continue
            # operand images and 16-bit copies, against the fp32 out of the launch above
            o32 = outs["AF_SPLIT_F32"][:M]
            _image_cap(c["f64"][0], "out")
            for n in "qkv":
                _image_cap(c[n], n)
            tag = "AF_SPLIT_F32 B=%d %s images: " % (B, family)
            o3, o8, o16 = _img_buf(M), _img_buf(M), _out_rows(M, D, F16)
            c16 = {n + "16": _out_rows(H * NT, HD, F16) for n in "qkv"}
            lse3, lse8 = _out_rows(H, NT, F32), _out_rows(H, NT, F32)
            _ok(L, _fwd(L, prec, B, "AF_SPLIT_F32", split16=1, q=q, k=k, v=v, out3=o3, o16=o16, lse=lse3, **c16), tag)
            _ok(L, _fwd(L, prec, B, "AF_SPLIT_F32_NOSAVE", split16=1, q=q, k=k, v=v, out3=o8, out3_f8=1, lse=lse8, lse_optional=1), tag)
            _all_nan(lse8[:H], tag + "no-save lse")
            for buf, rows in ((o3, M), (o8, M), (o16, M), (lse3, H)) + tuple((c16[n], H * NT) for n in c16):
                _tail_untouched(buf, rows, tag)
            _check_hi_lo(tag + "out3 ", o32, o3[:M, :D], o3[:M, D:])
            _check_hi_lo(tag + "o16 ", o32, o16[:M])
            _check_f8(tag, o32, o8[:M])
            for n in "qkv":
                _check_hi_lo(tag + n + "16 ", c[n].reshape(-1, HD), c16[n + "16"][:H * NT])
            _same_bits(lse3[:H], lses["AF_SPLIT_F32"][:H], tag + "lse next to out3")
            # the planar form writes the same images from its own fp32 result
            o3p, lse3p = _img_buf(M), _out_rows(H, NT, F32)
            _ok(L, _fwd(L, prec, B, "AF_SPLIT_P3", split16=1, out3=o3p, lse=lse3p, **ph), tag)
            _check_hi_lo("AF_SPLIT_P3 B=%d %s out3 " % (B, family), outs["AF_SPLIT_P3"][:M], o3p[:M, :D], o3p[:M, D:])


@pytest.mark.parametrize("B", BATCHES)
def test_forward_one_part(B):
    """AF_SPLIT_P1 and AF_V2_F8: 16-bit attention on the hi planes (the lo planes are handed over and must not be read into the result):
    fp64 on the hi planes is the reference.  AF_V2_F8's hi16 plane against AF_V2's out on the same planes."""
    L, prec, _, _ = _mode("fp32h")
    M, H = B * NT, B * NH
    u, t = R.unit(F16)
    for family in _families(B):
        c = _ref(family, B, F16)   # q / k / v rounded to half: they ARE the hi planes
        raw = R.make_inputs(family, B, SEED)
        lo = {n: _planes(raw[i])[1] for i, n in enumerate("qkv")}
        ph = {n + "_hi": _op(c[n], F16) for n in "qkv"}
        ph.update({n + "_lo": _dev(lo[n]) for n in "qkv"})
        base = R.cmp_bound(c["f64"][0], c["f32"][0])
        with _switches(L):
            tag = "AF_SPLIT_P1 B=%d %s: " % (B, family)
            out, lse = _fwd_bufs(B, F32)
            _ok(L, _fwd(L, prec, B, "AF_SPLIT_P1", split16=1, parts=1, out=out, lse=lse, **ph), tag)
            _tail_untouched(out, M, tag + "out")
            _held("attn_fwd_split<1>", tag + "out", _out_heads(out, B), c["f64"][0], R.fwd_allowance(c["v"], c["f64"][2], c["f64"][0], base, u, t))
            _check_fwd_stats("attn_fwd_split<1>", tag, c, lse)
            out2, lse2 = _fwd_bufs(B, F32)
            _ok(L, _fwd(L, prec, B, "AF_SPLIT_P1_NOSAVE", split16=1, parts=1, out=out2, lse=lse2, lse_optional=1, **ph), tag)
            _same_bits(out2, out, tag + "no-save twin")
            _all_nan(lse2[:H], tag + "no-save lse")
            # AF_V2_F8: the operand image alone
            tag = "AF_V2_F8 B=%d %s: " % (B, family)
            o8, lse8 = _img_buf(M), _out_rows(H, NT, F32)
            _ok(L, _fwd(L, prec, B, "AF_V2_F8", split16=1, parts=1, out3=o8, out3_f8=1, lse=lse8, **ph), tag)
            _tail_untouched(o8, M, tag + "out3")
            h16, h8, l8 = RF.f8_image_parts(o8[:M])
            A16 = R.fwd_allowance(c["v"], c["f64"][2], c["f64"][0], base, u, t, store_dt=F16)
            _held("attn_fwd_v2<OUT3>", tag + "hi16", R.to_heads(h16.float(), B), c["f64"][0], A16)
            _check_fwd_stats("attn_fwd_v2<OUT3>", tag, c, lse8, exp2_form=True)
            # e4m3(hi) is one rounding of the stored hi16; hi16 + lo / 2^12 is the fp32 result to half an e4m3 step of lo (2^-4 of the
            # decoded byte; the lo value is rounded to half first, attention_v2.hip pack_rows(pl, lo, 1.0f): 2^-10 of it covers that) +
            # 2^-10 (a subnormal e4m3) -- and that result is the 16-bit kernel's without the store rounding
            src_hi = h16.double().clamp(-448.0, 448.0)
            dec_hi, dec_lo = RF.e4m3_decode(h8), RF.e4m3_decode(l8)
            n = h16.double().abs() >= 2.0 ** -14
            worst = float(((dec_hi - src_hi).abs() / RF.e4m3_half_step(src_hi))[n].max())
            print("[f8] %se4m3(hi): worst |decoded - hi16| / half step %.3f" % (tag, worst))
            assert worst <= 1.0, tag
            A32 = R.fwd_allowance(c["v"], c["f64"][2], c["f64"][0], base, u, t) + R.to_heads(((2.0 ** -4 + 2.0 ** -10) * dec_lo.abs() + 2.0 ** -10) / 4096.0, B)
            _held("attn_fwd_v2<OUT3>", tag + "hi16 + lo", R.to_heads(h16.double() + dec_lo / 4096.0, B), c["f64"][0], A32)
            o8n, lse8n = _img_buf(M), _out_rows(H, NT, F32)
            _ok(L, _fwd(L, prec, B, "AF_V2_F8_NOSAVE", split16=1, parts=1, out3=o8n, out3_f8=1, lse=lse8n, lse_optional=1, **ph), tag)
            _same_bits(o8n, o8, tag + "no-save twin")
            _all_nan(lse8n[:H], tag + "no-save lse")
            # The same planes through AF_V2 at precision 1.  Not the same bits: AF_V2 folds o * (1 / sum) and the conversion of half of
            # a lane's results into v_fma_mixlo_f16 (one rounding of the exact product), AF_V2_F8 pins the fp32 product it takes lo
            # against and converts that (two roundings) -- DESIGN.md 7v.  2e-5 of the elements sit on the other side of a half rounding
            # boundary (a record); each plane is held to the 16-bit allowance, and no element is further than the next half value away.
            out16, lse16 = _fwd_bufs(B, F16)
            _ok(L, _fwd(L, 1, B, "AF_V2", q=ph["q_hi"], k=ph["k_hi"], v=ph["v_hi"], out=out16, lse=lse16), tag)
            _held("attn_fwd_v2", tag + "AF_V2 out on the hi planes", _out_heads(out16, B), c["f64"][0], A16)
            step = (_bits(h16.to(DEV)).int() - _bits(out16[:M]).int()).abs()
            print("%shi16 plane vs AF_V2 out: %d of %d elements differ, by at most %d half value(s)" % (tag, int((step != 0).sum()), step.numel(), int(step.max())))
            assert int(step.max()) <= 1, tag + "hi16 plane and AF_V2 out are more than one half value apart"
            _same_bits(lse8[:H], lse16[:H], tag + "lse vs AF_V2 lse")
            if family in ("randn", "spike"):   # AF_SPLIT_P1's images against its own fp32 out
                tag = "AF_SPLIT_P1 B=%d %s images: " % (B, family)
                o3, o8b, lse3 = _img_buf(M), _img_buf(M), _out_rows(H, NT, F32)
                outb = _out_rows(M, D, F32)
                _ok(L, _fwd(L, prec, B, "AF_SPLIT_P1", split16=1, parts=1, out=outb, out3=o3, lse=lse3, **ph), tag)
                _same_bits(outb, out, tag + "out next to out3")
                _check_hi_lo(tag + "out3 ", out[:M], o3[:M, :D], o3[:M, D:])
                with _switches(L, v2=2):   # without the round-5 forward the image-only call stays on the split kernel
                    _ok(L, _fwd(L, prec, B, "AF_SPLIT_P1", split16=1, parts=1, out3=o8b, out3_f8=1, lse=lse3, **ph), tag)
                _check_f8(tag, out[:M], o8b[:M])


# ==================================================================================================================================
# backward, 16-bit kernels: AB_16_TWO, AB_16_FUSED, AB_16_FUSED_AHEAD (round 4), AB_V2 (round 5)
# ==================================================================================================================================
BWD16 = {"AB_16_TWO": ("attn_bwd_dq/dkv_bf16", 0, 0), "AB_16_FUSED": ("attn_bwd_fused<false>", 0, 1),
         "AB_16_FUSED_AHEAD": ("attn_bwd_fused<true>", 0, 2), "AB_V2": ("attn_bwd_v2", 3, 1)}   # route -> (kernel, ATTN_V2, ATTN_BWD_FUSED)


def _bwd_ops16(c, dt):
    B = c["B"]
    ops = {n: _op(c[n], dt) for n in "qkv"}
    ops["out"] = _op(R.to_tokens(c["out_given"], B), dt)
    ops["dout"] = _op(R.to_tokens(c["dout"], B), dt)
    ops["lse"] = _dev(c["lse_given"])
    return ops


def _split_dqkv(dqkv, B):
    g = dqkv[:B * NT].detach().float().cpu()
    return [R.to_heads(g[:, i * D:(i + 1) * D], B) for i in range(3)]


def _bwd16_allowances(c, dt):
    u, t = R.unit(dt)
    bases = [R.cmp_bound(c["b64"][i], c["b32"][i]) for i in range(3)]
    return R.bwd_allowance(c["q"], c["k"], c["v"], c["dout"], c["f64"][2], c["b64"][4], c["b64"][:3], bases, u, t, store_dt=dt)


def _run_bwd16(L, route, c, dt, tag, ops=None, **extra):
    _, v2, fused = BWD16[route]
    B = c["B"]
    M, H = B * NT, B * NH
    ops = ops or _bwd_ops16(c, dt)
    dqkv, delta = _out_rows(M, 3 * D, dt), _out_rows(H, NT, F32)
    with _switches(L, v2=v2, fused=fused):
        _ok(L, _bwd(L, 1, B, route, dqkv=dqkv, delta=delta, **ops, **extra), tag)
    _tail_untouched(dqkv, M, tag + "dqkv")
    _tail_untouched(delta, H, tag + "delta")
    return dqkv, delta


def _check_bwd16(route, c, dt, tag, dqkv, delta):
    kernel = BWD16[route][0]
    for name, got, ref, A in zip(("dq", "dk", "dv"), _split_dqkv(dqkv, c["B"]), c["b64"][:3], _bwd16_allowances(c, dt)):
        _held(kernel, tag + name, got, ref, A)
    if route == "AB_V2":
        _all_nan(delta[:c["B"] * NH], tag + "delta (AB_V2 keeps it in LDS)")
    else:
        _cmp(kernel, tag + "delta", delta[:c["B"] * NH], c["b64"][3], c["b32"][3])


@pytest.mark.parametrize("mode", MODES16)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("route", sorted(BWD16))
def test_backward_16bit(route, B, mode):
    L, _, dt, _ = _mode(mode)
    cases = [(f, "randn") for f in _families(B)] + ([("randn", "cls")] if B == 1 else [])
    for family, dk in cases:
        c = _ref(family, B, dt, dk)
        tag = "%s %s B=%d %s%s: " % (route, mode, B, family, "" if dk == "randn" else " / %s dout" % dk)
        dqkv, delta = _run_bwd16(L, route, c, dt, tag)
        _check_bwd16(route, c, dt, tag, dqkv, delta)


@pytest.mark.parametrize("mode", MODES16)
def test_backward_v2_fourth_head_per_workgroup(mode):
    """B = 65: a workgroup's fourth head is the first to reuse the first head's three LDS slots (the rotation has period 3)."""
    L, _, dt, _ = _mode(mode)
    c = _ref("randn", 65, dt)
    tag = "AB_V2 %s B=65 randn: " % mode
    dqkv, delta = _run_bwd16(L, "AB_V2", c, dt, tag)
    _check_bwd16("AB_V2", c, dt, tag, dqkv, delta)


@pytest.mark.parametrize("mode", MODES16)
@pytest.mark.parametrize("B", [1, 22])
@pytest.mark.parametrize("route", ["AB_16_FUSED", "AB_16_FUSED_AHEAD", "AB_V2"])
def test_cls_only_tail_equals_the_full_gradient(route, B, mode):
    """q_tiles = 1 (what every teacher pass of a step runs) gives the bits of q_tiles = 7 when dout is non-zero in row 0 of each image only,
    the dQ rows from 32 on -- written as zeros by waves that skip phase A -- included; and both stay inside the allowance."""
    L, _, dt, _ = _mode(mode)
    c = _ref("randn", B, dt, "cls")
    tag = "%s %s B=%d cls-only dout: " % (route, mode, B)
    ops = _bwd_ops16(c, dt)
    full, _ = _run_bwd16(L, route, c, dt, tag + "q_tiles 7 ", ops, q_tiles=7)
    tail, delta = _run_bwd16(L, route, c, dt, tag + "q_tiles 1 ", ops, q_tiles=1)
    _same_bits(tail, full, tag + "q_tiles 1 vs 7")
    dq = tail[:B * NT, :D].reshape(B, NT, D)[:, 32:]
    assert bool((_bits(dq) == 0).all()), tag + "dQ rows 32.. are not zeros"
    _check_bwd16(route, c, dt, tag + "q_tiles 1 ", tail, delta)


@pytest.mark.parametrize("mode", MODES16)
@pytest.mark.parametrize("route", sorted(BWD16))
def test_strided_out_equals_the_contiguous_call(route, mode):
    """`out` as the hi plane of a [B*197][SPLIT_A*768] operand image (out_ld = 1536), the rest of the image NaN."""
    L, _, dt, _ = _mode(mode)
    B = 2
    c = _ref("randn", B, dt)
    tag = "%s %s B=%d strided out: " % (route, mode, B)
    ops = _bwd_ops16(c, dt)
    flat, delta = _run_bwd16(L, route, c, dt, tag, ops)
    img = torch.full((B * NT, 2 * D), math.nan, dtype=dt, device=DEV)
    img[:, :D] = ops["out"]
    strided, delta2 = _run_bwd16(L, route, c, dt, tag, dict(ops, out=img), out_ld=2 * D)
    _same_bits(strided, flat, tag + "dqkv")
    if route != "AB_V2":
        _same_bits(delta2, delta, tag + "delta")


@pytest.mark.parametrize("mode", MODES16)
@pytest.mark.parametrize("case", ["strided out", "cls-only tail"])
def test_fused_routes_equal_the_two_kernel_form(case, mode):
    """The fused kernels run the two phase bodies of the two-kernel form (attention_16.hip: bwd16_dkv_phase, bwd16_dq_phase), so AB_16_FUSED
    and AB_16_FUSED_AHEAD give AB_16_TWO's dq, dk and dv (torch.equal) in the two calls whose argument only the fused kernels' phases see
    differently: a strided `out` (out_ld = 1536), and a cls-only dout with q_tiles = 1 against the two-kernel form's seven query tiles."""
    L, _, dt, _ = _mode(mode)
    B = 2
    M = B * NT
    cls = case == "cls-only tail"
    c = _ref("randn", B, dt, "cls" if cls else "randn")
    tag = "%s B=%d %s: " % (mode, B, case)
    ops, extra = _bwd_ops16(c, dt), {}
    if not cls:
        img = torch.full((M, 2 * D), math.nan, dtype=dt, device=DEV)
        img[:, :D] = ops["out"]
        ops, extra = dict(ops, out=img), dict(out_ld=2 * D)
    two, _ = _run_bwd16(L, "AB_16_TWO", c, dt, tag + "AB_16_TWO ", ops, q_tiles=7, **extra)
    for route in ("AB_16_FUSED", "AB_16_FUSED_AHEAD"):
        got, _ = _run_bwd16(L, route, c, dt, tag + route + " ", ops, q_tiles=1 if cls else 7, **extra)
        for i, name in enumerate(("dq", "dk", "dv")):
            assert torch.equal(got[:M, i * D:(i + 1) * D], two[:M, i * D:(i + 1) * D]), tag + "%s of %s differs from AB_16_TWO" % (name, route)


# ==================================================================================================================================
# backward, fp32-mode kernels: AB_EXACT, AB_SPLIT3, AB_SPLIT1
# ==================================================================================================================================
def _bwd_ops32(c):
    B = c["B"]
    ops = {n: _dev(c[n]) for n in "qkv"}
    ops["out"] = _dev(R.to_tokens(c["out_given"], B))
    ops["dout"] = _dev(R.to_tokens(c["dout"], B))
    ops["lse"] = _dev(c["lse_given"])
    return ops


@pytest.mark.parametrize("mode", ["fp32", "fp32h"])
@pytest.mark.parametrize("B", [1, 2])
def test_backward_exact(B, mode):
    L, prec, _, _ = _mode(mode)
    M, H = B * NT, B * NH
    for family, dk in [(f, "randn") for f in R.FAMILIES] + [("randn", "cls"), ("randn", "grad")]:
        c = _ref(family, B, F32, dk)
        tag = "AB_EXACT %s B=%d %s%s: " % (mode, B, family, "" if dk == "randn" else " / %s dout" % dk)
        dqkv, delta = _out_rows(M, 3 * D, F32), _out_rows(H, NT, F32)
        with _switches(L):
            _ok(L, _bwd(L, prec, B, "AB_EXACT", dqkv=dqkv, delta=delta, **_bwd_ops32(c)), tag)
        _tail_untouched(dqkv, M, tag + "dqkv")
        _tail_untouched(delta, H, tag + "delta")
        for name, got, i in zip(("dq", "dk", "dv"), _split_dqkv(dqkv, B), range(3)):
            _cmp("attn_bwd_dq/dkv_f32", tag + name, got, c["b64"][i], c["b32"][i])
        _cmp("attn_bwd_dq/dkv_f32", tag + "delta", delta[:H], c["b64"][3], c["b32"][3])
        if mode == "fp32h" and (family, dk) == ("randn", "grad"):   # dqkv3: dqkv * s3 as the [hi | lo] image, against the fp32 dqkv above
            s3 = GS_UNIT
            for i in range(3):
                _image_cap(c["b64"][i], tag + "dqkv3", s3)
            img, delta3 = _out_rows(M, 6 * D, F16), _out_rows(H, NT, F32)
            with _switches(L):
                _ok(L, _bwd(L, prec, B, "AB_EXACT", dqkv3=img, s3=s3, delta=delta3, **_bwd_ops32(c)), tag)
            _tail_untouched(img, M, tag + "dqkv3")
            _check_hi_lo(tag + "dqkv3 ", dqkv[:M] * s3, img[:M, :3 * D], img[:M, 3 * D:])
            _same_bits(delta3, delta, tag + "delta next to dqkv3")


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("route", ["AB_SPLIT1", "AB_SPLIT3"])
def test_backward_split(route, B):
    """Gradient-sized dout (times 1e-3), as tests/test_gpu_round3.py's split attention test and for its reason: the kernels lift dout by
    2^12 before they split it, which a unit-variance dout times the peaked families' dS would carry past the half range.  AB_SPLIT1 gets
    q / k / v / dout that are IEEE-half values (its gradient products are hi * hi alone: fp64 on the hi planes is the reference)."""
    L, prec, _, _ = _mode("fp32h")
    M, H = B * NT, B * NH
    three = route == "AB_SPLIT3"
    kernel = "attn_bwd_split<%d>" % (3 if three else 1)
    for family in _families(B):
        c = _ref(family, B, F32 if three else F16, "grad")
        if not three:   # out stays an fp32 tensor in this mode: the fp64 out rounded to fp32
            c = dict(c, out_given=c["f64"][0].float())
            c["b64"] = R.attn_bwd_ref(c["q"], c["k"], c["v"], c["out_given"], c["dout"], lse=c["lse_given"])
            c["b32"] = R.attn_bwd_ref(c["q"], c["k"], c["v"], c["out_given"], c["dout"], F32, lse=c["lse_given"])
        tag = "%s B=%d %s / grad dout: " % (route, B, family)
        assert float((c["dout"].abs().max() * GS_UNIT)) < 65504 / 2 and float(c["b64"][4].abs().max() * GS_UNIT) < 65504 / 2, tag
        bases = [R.cmp_bound(c["b64"][i], c["b32"][i]) for i in range(3)]
        if three:
            A = R.bwd_allowance(c["q"], c["k"], c["v"], c["dout"], c["f64"][2], c["b64"][4], c["b64"][:3], bases, R.SPLIT_U, 2.0 ** -25, gs=GS_UNIT,
                                ds=R.score_err3(c["q"], c["k"]), dp=R.dp_err3(c["dout"], c["v"], GS_UNIT), t_op=2.0 ** -25)
        else:
            u, t = R.unit(F16)
            A = R.bwd_allowance(c["q"], c["k"], c["v"], c["dout"], c["f64"][2], c["b64"][4], c["b64"][:3], bases, u, t, gs=GS_UNIT)
        ops = _bwd_ops32(c)
        gp = 3 if three else 1
        dqkv, delta = _out_rows(M, 3 * D, F32), _out_rows(H, NT, F32)
        with _switches(L):
            _ok(L, _bwd(L, prec, B, route, split16=1, grad_parts=gp, dqkv=dqkv, delta=delta, **ops), tag)
            _tail_untouched(dqkv, M, tag + "dqkv")
            _tail_untouched(delta, H, tag + "delta")
            for name, got, ref, a in zip(("dq", "dk", "dv"), _split_dqkv(dqkv, B), c["b64"][:3], A):
                _held(kernel, tag + name, got, ref, a)
            _cmp(kernel, tag + "delta", delta[:H], c["b64"][3], c["b32"][3])
            # a strided out is a 16-bit-kernel feature
            d2 = _out_rows(M, 3 * D, F32, fill=SENT)
            _refused(L, _bwd(L, prec, B, "AB_ERROR", split16=1, grad_parts=gp, dqkv=d2, delta=delta, **dict(ops, out_ld=2 * D)), "strided", tag)
            assert bool((d2 == SENT).all()), tag + "a refused call wrote"
            if family != "randn":
                continue
            # dqkv3: dqkv * s3 as the [hi | lo] operand image, against the fp32 dqkv above.  s3 = 2^12 is the lift the fp32-output launch
            # used, so both launches run the same arithmetic and the image is the split of dqkv * 2^12 exactly (the only s3 with an fp32
            # twin; at it 8 % of the spike family's dq is below 2^-14, past the 1 % cap, so the image case is the randn family)
            s3 = GS_UNIT
            for i in range(3):
                _image_cap(c["b64"][i], tag + "dqkv3", s3)
            v32 = dqkv[:M] * s3
            for hi_only in (0, 1):
                img, delta3 = _out_rows(M, 6 * D, F16), _out_rows(H, NT, F32)
                _ok(L, _bwd(L, prec, B, route, split16=1, grad_parts=gp, dqkv3=img, s3=s3, out_hi_only=hi_only, delta=delta3, **ops), tag)
                _tail_untouched(img, M, tag + "dqkv3")
                _check_hi_lo(tag + "dqkv3%s " % (" hi only" if hi_only else ""), v32, img[:M, :3 * D], None if hi_only else img[:M, 3 * D:])
                if hi_only:
                    _all_nan(img[:M, 3 * D:], tag + "lo half of an out_hi_only image")
                _same_bits(delta3, delta, tag + "delta next to dqkv3")


# ==================================================================================================================================
# refusals: every AF_ERROR / AB_ERROR configuration, a saving route without lse, the entries' own checks
# ==================================================================================================================================
@pytest.mark.parametrize("mode", ["fp32h", "fp16", "bf16"])
def test_refused_calls_return_the_error_and_write_nothing(mode):
    L, prec, dt, _ = _mode(mode)
    B = 1
    M, H = B * NT, B * NH
    c = _ref("randn", B, dt)
    q, k, v = (_op(c[n], dt) for n in "qkv")
    hi = {n + "_hi": _op(c[n], F16) for n in "qkv"}
    lo = {n + "_lo": _op(c[n] * 0, F16) for n in "qkv"}
    out, lse = _out_rows(M, D, dt, fill=SENT), _out_rows(H, NT, F32, fill=SENT)
    o3, x16 = _img_buf(M, fill=SENT), _out_rows(H * NT, HD, F16, fill=SENT)
    dqkv, delta = _out_rows(M, 3 * D, dt, fill=SENT), _out_rows(H, NT, F32, fill=SENT)
    S = stream_ptr()
    with _switches(L):
        _refused(L, L.dyt_unit_attn_fwd(None, prec, S), "NULL")
        _refused(L, L.dyt_unit_attn_bwd(None, prec, S), "NULL")
        a = _lib.UnitAttnFwdArgs()
        _refused(L, L.dyt_unit_attn_fwd(ctypes.byref(a), prec, S), "batch = 0")
        _refused(L, L.dyt_unit_attn_fwd(ctypes.byref(a), 2, S), "precision 2")
        b = _lib.UnitAttnBwdArgs()
        _refused(L, L.dyt_unit_attn_bwd(ctypes.byref(b), prec, S), "batch = 0")
        _refused(L, L.dyt_unit_attn_bwd(ctypes.byref(b), -1, S), "precision -1")
        if prec == 1:
            E = "AF_ERROR"
            _refused(L, _fwd(L, 1, B, E, q=q, k=k, v=v, out=out, lse=lse, **hi, **lo), "need the split kernel", "planes at precision 1")
            _refused(L, _fwd(L, 1, B, E, q=q, k=k, v=v, out=out, lse=lse, q16=x16), "need the split kernel", "q16 at precision 1")
            _refused(L, _fwd(L, 1, B, E, q=q, k=k, v=v, out=out, lse=lse, o16=out), "need the split kernel", "o16 at precision 1")
            _refused(L, _fwd(L, 1, B, E, q=q, k=k, v=v, lse=lse), "need the split kernel", "no out at precision 1")
            _refused(L, _fwd(L, 1, B, "AF_V2", q=q, k=k, v=v, out=out), "writes lse", "AF_V2 without lse")
            with _switches(L, v2=2):
                _refused(L, _fwd(L, 1, B, "AF_16", q=q, k=k, v=v, out=out), "writes lse", "AF_16 without lse")
                _refused(L, _fwd(L, 1, B, "AF_16", q=q, k=k, v=v, out=out, lse_optional=1), "writes lse", "AF_16 has no no-save twin")
        else:
            E = "AF_ERROR"
            _refused(L, _fwd(L, 0, B, E, q=q, k=k, v=v, out=out, lse=lse, out3=o3), "split output without the split kernel", "out3 on the exact kernel")
            _refused(L, _fwd(L, 0, B, E, q=q, k=k, v=v, lse=lse, out3=o3), "need the split kernel", "no out on the exact kernel")
            _refused(L, _fwd(L, 0, B, E, out=out, lse=lse, **hi, **lo), "need the split kernel", "planes without split16")
            _refused(L, _fwd(L, 0, B, E, split16=1, q=q, k=k, v=v, lse=lse), "no output", "split kernel without out and out3")
            _refused(L, _fwd(L, 0, B, E, split16=1, parts=1, q=q, k=k, v=v, out=out, lse=lse), "one-part form needs the planar", "parts 1 without planes")
            _refused(L, _fwd(L, 0, B, E, split16=1, parts=2, out=out, lse=lse, **hi, **lo), "one-part form needs the planar", "parts 2")
            _refused(L, _fwd(L, 0, B, "AF_EXACT", q=q, k=k, v=v, out=out), "writes lse", "AF_EXACT without lse")
            _refused(L, _fwd(L, 0, B, "AF_EXACT", q=q, k=k, v=v, out=out, lse_optional=1), "writes lse", "AF_EXACT has no no-save twin")
            _refused(L, _fwd(L, 0, B, "AF_SPLIT_F32", split16=1, q=q, k=k, v=v, out=out), "writes lse", "AF_SPLIT_F32 without lse")
            _refused(L, _fwd(L, 0, B, "AF_SPLIT_P3", split16=1, out=out, **hi, **lo), "writes lse", "AF_SPLIT_P3 without lse")
            _refused(L, _fwd(L, 0, B, "AF_SPLIT_P1", split16=1, parts=1, out=out, **hi, **lo), "writes lse", "AF_SPLIT_P1 without lse")
            _refused(L, _fwd(L, 0, B, "AF_V2_F8", split16=1, parts=1, out3=o3, out3_f8=1, **hi, **lo), "writes lse", "AF_V2_F8 without lse")
            ops = dict(q=q, k=k, v=v, out=_dev(torch.zeros(M, 2 * D)), dout=_dev(torch.zeros(M, D)), lse=lse, delta=delta, dqkv=dqkv)
            _refused(L, _bwd(L, 0, B, "AB_ERROR", out_ld=2 * D, **ops), "strided", "AB_EXACT with a strided out")
            _refused(L, _bwd(L, 0, B, "AB_ERROR", out_ld=2 * D, split16=1, **ops), "strided", "AB_SPLIT3 with a strided out")
            _refused(L, _bwd(L, 0, B, "AB_ERROR", out_ld=2 * D, split16=1, grad_parts=1, **ops), "strided", "AB_SPLIT1 with a strided out")
    torch.cuda.synchronize()
    for t in (out, lse, o3, x16, dqkv, delta):
        assert bool((t == SENT).all()), "a refused call wrote"
    # a later valid call on the same library succeeds
    o, l = _fwd_bufs(B, dt)
    with _switches(L):
        _ok(L, _fwd(L, prec, B, "AF_V2" if prec else "AF_EXACT", q=q, k=k, v=v, out=o, lse=l))
    assert bool(torch.isfinite(o[:M].float()).all())
