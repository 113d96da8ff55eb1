"""Pins tests/attn_refs.py -- the fp64 references and the element-wise allowances tests/test_gpu_unit_attention.py holds the attention kernels
to -- without a GPU:
  * the references against torch autograd on the restatement of Attention.forward tests/test_gpu_round5.py uses, at 1e-12 in float64;
  * the CPU emulation of a 16-bit kernel (fp32 arithmetic, a rounding to the operand type at each documented point) stays inside the
    allowance for every input family in both operand types -- the allowance is not too tight for a correct kernel;
  * three broken emulations leave it by a wide margin -- a dropped delta (dk / dq), the padding keys in the row sum, key 196 masked with
    them (out / lse) -- so the allowance cannot be loosened into emptiness unnoticed;
  * each family has the property it exists for after the operands' rounding; the route restatement agrees with csrc/attn_route.h's cases.
4 heads of one image, seed 5."""
import pytest
import torch

import attn_refs as R

F64, F32 = torch.float64, torch.float32
NT, NH, HD, D = R.NT, R.NH, R.HD, R.D
HEADS, SEED = 4, 5
MARGIN = 8.0   # a dropped delta must overrun its allowance at least this far: the allowance could grow eightfold before the fault escaped
TYPES = [torch.bfloat16, torch.float16]


def _close(a, b, what, tol=1e-12):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    err = float((a - b).abs().max())
    assert a.shape == b.shape and err <= tol * max(1.0, float(b.abs().max())), "%s: |d| = %.3e" % (what, err)


@pytest.mark.parametrize("B", [1, 2])
def test_references_are_torch_autograd(B):
    g = torch.Generator().manual_seed(B)
    qkv = (torch.randn(B * NT, 3 * D, generator=g) * 1.5).double()
    dout = torch.randn(B * NT, D, generator=g).double()
    x = qkv.reshape(B, NT, 3, NH, HD).permute(2, 0, 3, 1, 4).clone().requires_grad_(True)   # tests/test_gpu_round5.py: _attn_ref
    s = (x[0] * 0.125) @ x[1].transpose(-1, -2)
    o = (s.softmax(-1) @ x[2]).transpose(1, 2).reshape(B * NT, D)
    o.backward(dout)
    q, k, v = (x[i].detach().reshape(B * NH, NT, HD) * (0.125 if i == 0 else 1.0) for i in range(3))
    out, lse, P = R.attn_fwd_ref(q, k, v)
    _close(R.to_tokens(out, B), o.detach(), "out")
    _close(lse, s.detach().reshape(B * NH, NT, NT).logsumexp(-1), "lse")
    _close(P, s.detach().softmax(-1).reshape(B * NH, NT, NT), "P")
    dq, dk, dv, delta, dS = R.attn_bwd_ref(q, k, v, out, R.to_heads(dout, B))
    gr = x.grad.reshape(3, B * NH, NT, HD)
    for name, got, want in (("dq", dq, gr[0]), ("dk", dk, gr[1]), ("dv", dv, gr[2])):
        _close(got, want, name)
    _close(delta, (R.to_heads(dout, B) * out).sum(-1), "delta")
    _close(dS.sum(-1), torch.zeros(B * NH, NT, dtype=F64), "rows of dS sum to 0 with the exact out")
    _close(R.to_heads(R.to_tokens(out, B), B), out, "layout round trip")
    # the lse the backward is handed takes the place of the exact one
    dq2 = R.attn_bwd_ref(q, k, v, out, R.to_heads(dout, B), lse=lse)[0]
    _close(dq2, dq, "dq from the given lse")


def _case(family, dt, dout_kind="randn"):
    q, k, v, dout = (x[:HEADS] for x in R.make_inputs(family, 1, SEED, dout_kind))
    q, k, v, dout = (x.to(dt).float() for x in (q, k, v, dout))
    return q, k, v, dout


def _fwd_shares(family, dt, **fault):
    q, k, v, _ = _case(family, dt)
    r64, r32 = R.attn_fwd_ref(q, k, v), R.attn_fwd_ref(q, k, v, F32)
    u, t = R.unit(dt)
    A_out = R.fwd_allowance(v, r64[2], r64[0], R.cmp_bound(r64[0], r32[0]), u, t, store_dt=dt)
    A_lse = R.lse_allowance(q, k, R.cmp_bound(r64[1], r32[1]))
    out, lse = R.emulate_fwd16(q, k, v, dt, **fault)
    return R.share(out, r64[0], A_out), R.share(lse, r64[1], A_lse)


def _bwd_shares(family, dt, dout_kind="randn", **fault):
    q, k, v, dout = _case(family, dt, dout_kind)
    out64, lse64, P = R.attn_fwd_ref(q, k, v)
    out16, lse = out64.to(dt), lse64.float()
    r64 = R.attn_bwd_ref(q, k, v, out16, dout, lse=lse)
    r32 = R.attn_bwd_ref(q, k, v, out16, dout, F32, lse=lse)
    u, t = R.unit(dt)
    A = R.bwd_allowance(q, k, v, dout, P, r64[4], r64[:3], [R.cmp_bound(r64[i], r32[i]) for i in range(3)], u, t, store_dt=dt)
    got = R.emulate_bwd16(q, k, v, out16, dout, lse, dt, **fault)
    return [R.share(got[i], r64[i], A[i]) for i in range(3)]


@pytest.mark.parametrize("dt", TYPES)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_families_and_the_emulation_inside_the_allowance(family, dt):
    q, k, v, _ = _case(family, dt)
    R.check_family(family, q, k)
    so, sl = _fwd_shares(family, dt)
    sq, sk, sv = _bwd_shares(family, dt)
    print("%s %s: share of the allowance out %.3f lse %.3f dq %.3f dk %.3f dv %.3f" % (family, dt, so, sl, sq, sk, sv))
    assert max(so, sl) <= 1.0 and max(sq, sk, sv) <= 1.0, (so, sl, sq, sk, sv)


@pytest.mark.parametrize("dt", TYPES)
@pytest.mark.parametrize("dout_kind", ["cls", "grad"])
def test_emulation_inside_the_allowance_for_the_other_gradients(dout_kind, dt):
    s = _bwd_shares("randn", dt, dout_kind)
    print("randn / %s dout %s: dq %.3f dk %.3f dv %.3f" % (dout_kind, dt, *s))
    assert max(s) <= 1.0, s


@pytest.mark.parametrize("dt", TYPES)
@pytest.mark.parametrize("family", [f for f in R.FAMILIES])
def test_a_dropped_delta_leaves_the_allowance(family, dt):
    sq, sk, _ = _bwd_shares(family, dt, drop_delta=True)
    print("%s %s without delta: dq %.1f dk %.1f times the allowance" % (family, dt, sq, sk))
    assert sq >= MARGIN, sq
    if family != "uniform":   # (q = 0: dk = dS^T q is zero whatever dS is)
        assert sk >= MARGIN, sk


@pytest.mark.parametrize("dt", TYPES)
@pytest.mark.parametrize("family", ["randn", "negative"])
def test_leaked_padding_keys_leave_the_allowance(family, dt):
    s = max(_fwd_shares(family, dt, leak_pad=True))
    print("%s %s with the padding keys in the sum: %.1f times the allowance" % (family, dt, s))
    assert s >= 4.0, s


@pytest.mark.parametrize("dt", TYPES)
@pytest.mark.parametrize("family", ["randn", "spike", "negative", "peak-last", "uniform"])
def test_a_dropped_last_key_leaves_the_allowance(family, dt):
    s = max(_fwd_shares(family, dt, drop_last=True))
    print("%s %s without key 196: %.1f times the allowance" % (family, dt, s))
    assert s >= 100.0, s


def test_route_restatement():
    f, b = R.fwd_route, R.bwd_route
    assert f(1) == "AF_V2" and f(1, v2=2) == "AF_16" and f(1, lse_optional=True) == "AF_V2_NOSAVE" and f(1, v2=0, lse_optional=True) == "AF_16"
    assert f(0) == "AF_EXACT" and f(0, lse_optional=True) == "AF_EXACT" and f(0, out3=True) == "AF_ERROR"
    assert f(0, split=True) == "AF_SPLIT_F32" and f(0, split=True, saved=True, o16=True, out=False, out3=True) == "AF_SPLIT_F32"
    assert f(0, split=True, planes=True) == "AF_SPLIT_P3" and f(0, split=True, planes=True, lse_optional=True) == "AF_SPLIT_P3_NOSAVE"
    assert f(0, split=True, planes=True, parts=1) == "AF_SPLIT_P1"
    assert f(0, split=True, planes=True, parts=1, out=False, out3=True, out3_f8=True) == "AF_V2_F8"
    assert f(0, split=True, planes=True, parts=1, out=False, out3=True, out3_f8=True, v2=2) == "AF_SPLIT_P1"
    assert f(0, split=True, planes=True, parts=1, out=False, out3=True, out3_f8=True, lse_optional=True) == "AF_V2_F8_NOSAVE"
    assert f(0, split=True, parts=1) == "AF_ERROR" and f(0, split=True, out=False) == "AF_ERROR"
    assert f(1, planes=True) == "AF_ERROR" and f(1, saved=True) == "AF_ERROR" and f(1, o16=True) == "AF_ERROR" and f(0, planes=True) == "AF_ERROR"
    assert b(0) == "AB_EXACT" and b(0, split=True) == "AB_SPLIT3" and b(0, split=True, grad_parts=1) == "AB_SPLIT1"
    assert b(0, out_strided=True) == "AB_ERROR" and b(0, split=True, out_strided=True) == "AB_ERROR"
    assert b(1) == "AB_V2" and b(1, v2=1) == "AB_16_FUSED" and b(1, v2=1, fused=2) == "AB_16_FUSED_AHEAD" and b(1, v2=0, fused=0) == "AB_16_TWO"
    assert b(1, out_strided=True) == "AB_V2"
