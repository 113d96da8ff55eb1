"""Plain-torch CPU references of the attention kernels (csrc/attention_16.hip, attention_exact.hip, attention_split.hip, attention_v2.hip), for tests/test_gpu_unit_attention.py.

Every tensor here is in the kernels' head layout: q / k / v / out / dout / dq / dk / dv [H = B*12][197][64], q already times 1/8, lse / delta
[H][197]; ``to_tokens`` / ``to_heads`` move between that and the [B*197][768] token rows of `out` / `dout` / `dqkv`.  Every function takes
``dtype``: float64 is the reference, float32 the CPU restatement whose distance from fp64 is the error floor of tests/test_gpu_step_tail.py's
``_cmp``.  tests/test_attn_refs_host.py pins the references to torch autograd and holds the CPU emulation of a 16-bit kernel (and three broken
emulations) against the allowances below, so that neither can drift with the kernels.

The allowance of a stored element is the ``_cmp`` bound of its tensor (``cmp_bound``) plus one term per rounding point of the kernel that wrote
it; each term is a unit roundoff times an fp64 abs-product of the reference (DESIGN.md 7v lists them per kernel with the line of code each
comes from).  u / t of an operand type: u = 2^-8 (bfloat16) or 2^-11 (IEEE half) is the relative step of one rounding, t = 2^-25 (half; 0 for
bfloat16, whose exponent range is fp32's) half the subnormal spacing, the absolute error of a rounding below 2^-14."""
import math

import torch

from tail_refs import ulp

NT, NH, HD, D = 197, 12, 64, 768
NPAD = 224
F32, F64 = torch.float32, torch.float64
SPLIT_U = 2.5 * 2.0 ** -21   # one three-part product: |x - hi - lo| <= 2^-21 |x| for either operand, the dropped lo * lo at 2^-22
FAMILIES = ("randn", "spike", "staircase", "negative", "peak-last", "peak-first", "uniform")
RESCALE_THR = 8.0            # attention_v2.hip: the running maximum is raised when a key tile exceeds it by more than e^8


def _cv(x, dtype):
    return x.detach().to("cpu").to(dtype)


def unit(dt):
    """(u, t) of a 16-bit operand type; (0, 0) for fp32 (its rounding is the ``_cmp`` part of an allowance)."""
    if dt == torch.bfloat16:
        return 2.0 ** -8, 0.0
    if dt == torch.float16:
        return 2.0 ** -11, 2.0 ** -25
    assert dt == F32, dt
    return 0.0, 0.0


def to_tokens(x, B):
    """[B*12][197][64] -> [B*197][768] (column h * 64 + d)."""
    return x.reshape(B, NH, NT, HD).permute(0, 2, 1, 3).reshape(B * NT, D).contiguous()


def to_heads(x, B):
    """[B*197][768] -> [B*12][197][64]."""
    return x.reshape(B, NT, NH, HD).permute(0, 2, 1, 3).reshape(B * NH, NT, HD).contiguous()


# ---- references ------------------------------------------------------------------------------------------------------------------
def attn_fwd_ref(q, k, v, dtype=F64):
    """(out, lse, P): P = softmax(q k^T) over the 197 keys, out = P v, lse = log sum_j exp(s_j) (natural log, of the scores as given)."""
    q, k, v = _cv(q, dtype), _cv(k, dtype), _cv(v, dtype)
    s = q @ k.transpose(-1, -2)
    m = s.max(-1, keepdim=True).values
    e = (s - m).exp()
    l = e.sum(-1, keepdim=True)
    P = e / l
    return P @ v, (m + l.log()).squeeze(-1), P


def attn_bwd_ref(q, k, v, out_given, dout, dtype=F64, lse=None):
    """(dq, dk, dv, delta, dS) of out = softmax(q k^T) v for the upstream gradient dout, as the kernels form it: P = exp(s - lse) from the
    lse they are handed (``lse``; None: the exact one), delta = rowsum(dout * out_given) from the output they are handed, dS = P (dP - delta),
    dq = dS k / 8 (q carries the 1/8, so the gradient w.r.t. the unscaled q does too), dk = dS^T q, dv = P^T dout."""
    q, k, v, o, do = (_cv(x, dtype) for x in (q, k, v, out_given, dout))
    s = q @ k.transpose(-1, -2)
    L = s.logsumexp(-1) if lse is None else _cv(lse, dtype)
    P = (s - L.unsqueeze(-1)).exp()
    dP = do @ v.transpose(-1, -2)
    delta = (do * o).sum(-1)
    dS = P * (dP - delta.unsqueeze(-1))
    return 0.125 * (dS @ k), dS.transpose(-1, -2) @ q, P.transpose(-1, -2) @ do, delta, dS


# ---- allowances ------------------------------------------------------------------------------------------------------------------
def cmp_bound(ref64, ref32):
    """The bound of ``_cmp`` (tests/test_gpu_step_tail.py) as a number: 4 max|fp32_cpu - fp64| + 4 ulp_fp32(max|fp64|)."""
    ref64, ref32 = _cv(ref64, F64), _cv(ref32, F64)
    return 4.0 * float((ref32 - ref64).abs().max()) + 4.0 * ulp(ref64.abs().max())


def store_term(x, dt):
    """The rounding of the stored value: u |x| + t (t: a result below 2^-14 is rounded to the subnormal spacing)."""
    u, t = unit(dt)
    return u * x.abs() + t


def score_err3(a, b):
    """Error of one three-part product a b^T [.., n, m] of fp32 operands split into IEEE-half hi + lo: SPLIT_U sum|a||b| plus the absolute
    floor 2^-25 of either operand's lo part (an element below 2^-3 has a subnormal or zero lo)."""
    a, b = _cv(a, F64).abs(), _cv(b, F64).abs()
    return SPLIT_U * (a @ b.transpose(-1, -2)) + 2.0 ** -25 * (a.sum(-1).unsqueeze(-1) + b.sum(-1).unsqueeze(-2))


def fwd_allowance(v, P, out, base, u, t, store_dt=None, ds=None, t_v=0.0):
    """Allowance of `out` [H][197][64].  base: the ``cmp_bound`` of the tensor.  u, t: the rounding of P before P v (a 16-bit kernel: ``unit``
    of its operand type; a three-part product: SPLIT_U and 2^-25).  store_dt: the 16-bit type `out` is stored in (None: fp32).  ds [H][197][197]:
    the error of the scores (three-part kernels): a perturbation d of a row's scores moves P_j by at most 2 max|d| P_j.  t_v: the absolute
    floor of v's own lo part, times sum_j P_j = 1."""
    v, P, out = _cv(v, F64), _cv(P, F64), _cv(out, F64)
    pv = P @ v.abs()
    A = base + u * pv + t * v.abs().sum(-2, keepdim=True) + t_v
    if ds is not None:
        A = A + 2.0 * ds.max(-1, keepdim=True).values * pv
    if store_dt is not None:
        A = A + store_term(out, store_dt)
    return A


def lse_allowance(q, k, base, exp2_form=False, ds=None):
    """Allowance of lse [H][197]: ``_cmp`` alone, plus max_j |s_j| 2^-23 where the kernel forms s log2(e) - m in fp32 (attention_v2.hip) and
    the score error of a three-part kernel."""
    s = _cv(q, F64) @ _cv(k, F64).transpose(-1, -2)
    A = torch.full(s.shape[:-1], float(base), dtype=F64)
    if exp2_form:
        A = A + s.abs().max(-1).values * 2.0 ** -23
    if ds is not None:
        A = A + ds.max(-1).values
    return A


def bwd_allowance(q, k, v, dout, P, dS, grads, bases, u, t, gs=1.0, store_dt=None, ds=None, dp=None, t_op=0.0):
    """Allowances (A_dq, A_dk, A_dv) of dq (stored times 1/8), dk, dv [H][197][64].  bases: their three ``cmp_bound``s.  u, t: the rounding
    of P (for dv) and of dS (for dq, dk) before their products; the kernels that lift dout by gs (a power of two) round gs dS, whose floor is
    t / gs.  ds / dp [H][197][197]: the errors of the recomputed scores and of dP (three-part kernels), which reach dS as |dS| ds + P dp and P
    as P ds.  t_op: the absolute floor of the other operand's lo part (three-part kernels)."""
    q, k, v, do, P, dS = (_cv(x, F64) for x in (q, k, v, dout, P, dS))
    aS, T = dS.abs(), lambda x: x.transpose(-1, -2)
    A_dq = u * (aS @ k.abs()) + (t / gs) * k.abs().sum(-2, keepdim=True) + t_op * aS.sum(-1, keepdim=True)
    A_dk = u * (T(aS) @ q.abs()) + (t / gs) * q.abs().sum(-2, keepdim=True) + t_op * T(aS).sum(-1, keepdim=True)
    A_dv = u * (T(P) @ do.abs()) + t * do.abs().sum(-2, keepdim=True) + (t_op / gs) * T(P).sum(-1, keepdim=True)
    if ds is not None:
        eS = aS * ds + (P * dp if dp is not None else 0.0)
        A_dq = A_dq + eS @ k.abs()
        A_dk = A_dk + T(eS) @ q.abs()
        A_dv = A_dv + T(P * ds) @ do.abs()
    A_dq = 0.125 * A_dq
    out = []
    for A, g, base in zip((A_dq, A_dk, A_dv), grads, bases):
        A = A + base
        if store_dt is not None:
            A = A + store_term(_cv(g, F64), store_dt)
        out.append(A)
    return out


def dp_err3(dout, v, gs):
    """Error of the three-part product dP = dout v^T whose first operand is lifted by gs before it is split."""
    do, v = _cv(dout, F64).abs(), _cv(v, F64).abs()
    return SPLIT_U * (do @ v.transpose(-1, -2)) + 2.0 ** -25 * (do.sum(-1).unsqueeze(-1) + v.sum(-1).unsqueeze(-2) / gs)


def share(got, ref64, A):
    """max over the elements of |got - ref| / A (0 / 0 counts as 0, x / 0 as inf); a non-finite `got` is inf."""
    got, ref64 = _cv(got, F64), _cv(ref64, F64)
    assert got.shape == ref64.shape == A.shape, (got.shape, ref64.shape, A.shape)
    if not bool(torch.isfinite(got).all()):
        return math.inf
    err = (got - ref64).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / A)
    return float(r.max())


# ---- a 16-bit kernel on the CPU --------------------------------------------------------------------------------------------------
def emulate_fwd16(q, k, v, dt, leak_pad=False, drop_last=False):
    """The arithmetic of the 16-bit forward kernels in fp32 with their roundings: scores and the row sum in fp32, P rounded to dt before P v
    (attention_16.hip `pack8(st[kt], ..)`, attention_v2.hip `pack8(s, ..)`), out = (P16 v) / sum rounded to dt by the store; (out dt, lse fp32).
    leak_pad: the 27 padding keys (score 0, v = 0) join the row sum; drop_last: key 196 is masked with them -- the two mask faults."""
    q, k, v = (_cv(x, dt).float() for x in (q, k, v))
    s = q @ k.transpose(-1, -2)
    if drop_last:
        s[..., NT - 1] = -math.inf
    m = s.max(-1, keepdim=True).values
    if leak_pad:
        m = m.clamp_min(0.0)
    p = (s - m).exp()
    l = p.sum(-1, keepdim=True)
    if leak_pad:
        l = l + (NPAD - NT) * (-m).exp()
    o = (p.to(dt).float() @ v) / l
    return o.to(dt), (m + l.log()).squeeze(-1)


def emulate_bwd16(q, k, v, out16, dout, lse, dt, drop_delta=False):
    """... of the 16-bit backward kernels: S, dP, delta and dS in fp32, P and dS rounded to dt before P^T dO, dS^T q and dS k, the three
    results rounded to dt by the store.  drop_delta: dS = P dP."""
    q, k, v, o, do = (_cv(x, dt).float() for x in (q, k, v, out16, dout))
    s = q @ k.transpose(-1, -2)
    p = (s - _cv(lse, F32).unsqueeze(-1)).exp()
    dP = do @ v.transpose(-1, -2)
    delta = (do * o).sum(-1, keepdim=True)
    dS = p * (dP if drop_delta else dP - delta)
    dS16, p16 = dS.to(dt).float(), p.to(dt).float()
    return ((dS16 @ k) * 0.125).to(dt), (dS16.transpose(-1, -2) @ q).to(dt), (p16.transpose(-1, -2) @ do).to(dt)


# ---- input families --------------------------------------------------------------------------------------------------------------
def staircase_rows():
    """Which of the 197 query rows of the staircase family step by ~8.5 per key tile (True) and which by ~7.5: query tiles 0-2 all 7.5 (the
    rescale is deferred on every other tile), 5-6 all 8.5 (taken on every tile), 3-4 alternating (`__any` makes one row's step raise all)."""
    i = torch.arange(NT)
    tile = i // 32
    return (tile >= 5) | ((tile >= 3) & (i % 2 == 1))


def make_inputs(family, B, seed, dout_kind="randn"):
    """(q, k, v, dout) fp32 in head layout, q already times 1/8.  dout_kind: "randn", "cls" (row 0 of every image only) or "grad" (times
    1e-3, the size of a real gradient)."""
    g = torch.Generator().manual_seed(1000 * seed + FAMILIES.index(family))
    H = B * NH

    def rn(*shape):
        return torch.randn(*shape, generator=g)

    def ru(*shape):
        return torch.rand(*shape, generator=g)

    if family in ("randn", "spike", "uniform"):
        q, k, v = 1.5 * rn(H, NT, HD) * 0.125, 1.5 * rn(H, NT, HD), 1.5 * rn(H, NT, HD)
        if family == "spike":       # tests/test_gpu_round5.py: key 100 of every head times 6, key 190 of one head per image times 9
            k[:, 100] *= 6.0
            k[1::NH, 190] *= 9.0
        if family == "uniform":
            q = torch.zeros(H, NT, HD)
    else:
        q, k, v = 0.02 * rn(H, NT, HD), 0.3 * rn(H, NT, HD), 1.5 * rn(H, NT, HD)
        j = torch.arange(NT)
        if family == "staircase":
            q[:, :, 0] = torch.where(staircase_rows(), torch.tensor(8.5 / 7.5), torch.tensor(1.0))
            jitter = 0.5 * ru(H, NT)
            jitter[:, j % 32 == 0] = 0.0   # the first key of a tile carries the tile's maximum
            k[:, :, 0] = 7.5 * (j // 32).float() - jitter
        elif family == "negative":
            q[:, :, 0] = 1.0 + ru(H, NT)
            k[:, :, 0] = -(16.0 + 12.0 * ru(H, NT))
        else:
            assert family in ("peak-last", "peak-first"), family
            q, k = 0.05 * rn(H, NT, HD), 0.3 * rn(H, NT, HD)
            q[:, :, 0] = 1.0 + 0.25 * ru(H, NT)
            k[:, :, 0] = 0.0
            k[:, NT - 1 if family == "peak-last" else 0, 0] = 48.0
    dout = rn(B * NT, D)
    if dout_kind == "cls":
        keep = torch.zeros(B * NT, 1)
        keep[::NT] = 1.0
        dout = dout * keep
    elif dout_kind == "grad":
        dout = dout * 1e-3
    else:
        assert dout_kind == "randn", dout_kind
    return q.contiguous(), k.contiguous(), v.contiguous(), to_heads(dout, B)


def check_family(family, q, k):
    """The property a family exists for, on the operands as the kernel gets them (after their rounding)."""
    s = _cv(q, F64) @ _cv(k, F64).transpose(-1, -2)
    if family == "negative":
        assert float(s.max()) <= -15.0 and float(s.min()) >= -60.0, (float(s.min()), float(s.max()))
        assert float(s.logsumexp(-1).max()) < 0.0
    elif family in ("peak-last", "peak-first"):
        w = NT - 1 if family == "peak-last" else 0
        other = torch.cat([s[..., :w], s[..., w + 1:]], -1).max(-1).values
        assert float((s[..., w] - other).min()) > 40.0, float((s[..., w] - other).min())
    elif family == "staircase":
        pad = torch.full(s.shape[:-1] + (NPAD - NT,), -math.inf, dtype=F64)
        tmax = torch.cat([s, pad], -1).reshape(s.shape[:-1] + (7, 32)).max(-1).values
        step = tmax[..., 1:] - tmax[..., :-1]
        big = staircase_rows()
        lo, hi = step[:, ~big], step[:, big]
        assert float(lo.min()) > 6.5 and float(lo.max()) < RESCALE_THR, (float(lo.min()), float(lo.max()))
        assert float(hi.min()) > RESCALE_THR and float(hi.max()) < 9.5, (float(hi.min()), float(hi.max()))
    elif family == "uniform":
        assert float(s.abs().max()) == 0.0


# ---- attn_route.h, restated ------------------------------------------------------------------------------------------------------
def fwd_route(precision, split=False, out=True, out3=False, planes=False, saved=False, o16=False, out3_f8=False, parts=3,
              lse_optional=False, v2=3):
    """attn_fwd_route() of csrc/attn_route.h: the kernel's name, or "AF_ERROR"."""
    def pick(name, nosave=True):
        return name + "_NOSAVE" if lse_optional and nosave else name
    split = precision == 0 and split
    if (planes or saved or o16 or not out) and not split:
        return "AF_ERROR"
    if not out and not out3:
        return "AF_ERROR"
    if split:
        if parts != 3 and not (planes and parts == 1):
            return "AF_ERROR"
        if planes and parts == 1:
            if not out and out3_f8 and not o16 and (v2 & 1):
                return pick("AF_V2_F8")
            return pick("AF_SPLIT_P1")
        return pick("AF_SPLIT_P3") if planes else pick("AF_SPLIT_F32")
    if precision == 0:
        return "AF_ERROR" if out3 else "AF_EXACT"
    return pick("AF_V2") if v2 & 1 else "AF_16"


def bwd_route(precision, split=False, grad_parts=3, out_strided=False, v2=3, fused=1):
    """attn_bwd_route() of csrc/attn_route.h."""
    if precision == 0:
        if out_strided:
            return "AB_ERROR"
        if split:
            return "AB_SPLIT3" if grad_parts >= 3 else "AB_SPLIT1"
        return "AB_EXACT"
    if v2 & 2:
        return "AB_V2"
    if fused:
        return "AB_16_FUSED_AHEAD" if fused == 2 else "AB_16_FUSED"
    return "AB_16_TWO"
