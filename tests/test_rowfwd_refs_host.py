"""Pins tests/rowfwd_refs.py -- the fp64 references tests/test_gpu_row_fwd.py holds the forward row kernels against -- to torch and to the
oracle, at 1e-12 relative in float64 (the same operation written twice), so that the references cannot drift together with the kernels.
Also the facts about the on-device draw the GPU tests rely on: the top Philox word gives u = 1.0 and the noise +inf (a kept token, soft = 1,
no NaN), the bottom word a finite value; and the choice of inputs of the ln_fold_w test (rounded and unrounded column sums differ).  No GPU."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import erase_refs as E
import rowfwd_refs as R
from oracle import dyt_oracle

TOL = 1e-12
F64, F32 = torch.float64, torch.float32
NT, NP, D = R.NT, R.NP, R.D


def _close(a, b, what):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    err = float((a - b).abs().max()) if a.numel() else 0.0
    assert a.shape == b.shape and err <= TOL * max(1.0, float(b.abs().max()) if b.numel() else 1.0), "%s: |d| = %.3e" % (what, err)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("eps", [1e-6, 1e-5])
@pytest.mark.parametrize("rows", [1, 5, 33])
def test_layernorm_ref_is_torch_layer_norm(rows, eps):
    g = _gen(rows)
    x = (3.0 * torch.randn(rows, D, generator=g) + 1.0).to(F64)
    w, b, resid = (torch.randn(D, generator=g).to(F64), torch.randn(D, generator=g).to(F64), torch.randn(rows, D, generator=g).to(F64))
    e = float(np.float32(eps))   # (the reference widens the C float)
    out, mean, rstd = R.layernorm_ref(x, w, b, eps)
    _close(out, F.layer_norm(x, (D,), w, b, e), "out")
    _close(mean, x.mean(-1), "mean")
    _close(rstd, 1.0 / (x.var(-1, unbiased=False) + e).sqrt(), "rstd")
    _close(R.layernorm_ref(x, w, b, eps, resid=resid)[0], F.layer_norm(x, (D,), w, b, e) + resid, "out + resid")
    const = torch.full((2, D), 4.25, dtype=F64)
    out, mean, rstd = R.layernorm_ref(const, w, b, eps)
    _close(out, b.expand(2, D), "constant row = bias")
    _close(rstd, torch.full((2,), e ** -0.5, dtype=F64), "constant row rstd")


@pytest.mark.parametrize("training,tau", [(True, 5.0), (True, 1.0), (False, 5.0)])
def test_gate_ref_with_injected_noise_is_the_oracle(training, tau):
    g = _gen(7)
    B = 3
    u = torch.randn(B, NT, D, generator=g).to(F64)
    w, b = 0.1 * torch.randn(D, generator=g).to(F64), torch.tensor([0.05], dtype=F64)
    g1 = -torch.log(-torch.log(torch.rand(B, NP, generator=g).to(F64)))
    g2 = -torch.log(-torch.log(torch.rand(B, NP, generator=g).to(F64)))
    logit = R.gate_logit_ref(u.reshape(-1, D), w, b).view(B, NT)
    _close(logit[:, 1:], F.linear(u[:, 1:], w.view(1, D), b).squeeze(-1), "logit")
    _, soft = R.gate_soft_ref(logit[:, 1:], training, tau, g1=g1, g2=g2)
    for thr in (0.3, 0.5, 0.7):
        sel, y_soft = dyt_oracle.gumbel_sigmoid(logit[:, 1:], g1, g2, tau, float(np.float32(thr)), training)
        _close(soft, y_soft, "soft")
        keep = R.gate_keep_ref(torch.cat([torch.ones(B, 1, dtype=F64), soft], 1), thr)
        assert bool(keep[:, 0].all()) and torch.equal(keep[:, 1:], sel.detach() > 0.5)
    # the noise term enters like g1 - g2
    n = torch.randn(B, NP, generator=g).to(F64)
    _close(R.gate_soft_ref(logit[:, 1:], True, tau, noise=n)[1], R.gate_soft_ref(logit[:, 1:], True, tau, g1=n, g2=torch.zeros_like(n))[1], "noise")


def test_force_first_keeps_a_prefix():
    soft = torch.rand(2, NT, generator=_gen(3))
    for ff in (1, 50, 197):
        keep = R.gate_keep_ref(soft, 0.5, force_first=ff)
        assert torch.equal(keep, (torch.arange(NT) < ff).expand(2, NT))


def test_noise_ref_edges_and_stream():
    """The top word: u01 = 1.0 exactly, noise +inf, z = +inf, soft = 1 (finite, kept, zero gate gradient soft (1 - soft)); the bottom word:
    u01 = 2^-25, noise finite.  Both in fp64 and in fp32."""
    assert float(E.u01(np.uint32(0xFFFFFFFF))) == 1.0 and float(E.u01(np.uint32(0))) == 2.0 ** -25
    for dt in (F64, F32):
        n = R.noise_from_words(np.array([0xFFFFFFFF, 0, 0x80000000], dtype=np.uint32), dt)
        assert float(n[0]) == math.inf and math.isfinite(float(n[1])) and float(n[1]) < -17.0 and abs(float(n[2])) < 1e-6
        z, soft = R.gate_soft_ref(torch.tensor([0.3, 0.3], dtype=dt), True, 5.0, noise=n[:2], dtype=dt)
        assert float(z[0]) == math.inf and float(soft[0]) == 1.0 and 0.0 < float(soft[1]) < 0.1
        assert not bool(torch.isnan(soft).any()) and float(soft[0] * (1 - soft[0])) == 0.0
    # the stream: word 0 of philox(seed, subseq, t), t = b * 197 + n; another subseq or seed is another stream
    w = R.gate_words(1234, (1 << 32) | 6, 3)
    assert w.shape == (3, NT) and w.dtype == np.uint32
    assert int(w[2, 5]) == int(E.philox(1234, (1 << 32) | 6, 2 * NT + 5)[0])
    assert not np.array_equal(w, R.gate_words(1234, 6, 3)) and not np.array_equal(w, R.gate_words(1235, (1 << 32) | 6, 3))
    n = R.gate_noise_ref(1234, 6, 3)
    assert n.shape == (3, NT) and bool(torch.isfinite(n).all())
    x = torch.from_numpy(E.u01(R.gate_words(1234, 6, 3))).double()
    _close(n, torch.logit(x), "noise = logit(u01)")


@pytest.mark.parametrize("B", [1, 2, 65])
def test_index_ref_is_nonzero(B):
    g = _gen(B)
    keep = torch.rand(B, NT, generator=g) < 0.3
    keep[:, 0] = True
    if B >= 2:
        keep[0, 1:] = False
        keep[B - 1] = True
    ix = R.index_ref(keep)
    flat = keep.reshape(-1)
    assert torch.equal(ix["row_src"].long(), flat.nonzero().view(-1))
    assert torch.equal(ix["drop_src"].long(), (~flat).nonzero().view(-1))
    assert ix["total"].tolist() == [int(flat.sum()), B * NT - int(flat.sum())]
    assert torch.equal(ix["counts"].long(), keep.sum(1))
    assert torch.equal(ix["dst_of"] >= 0, flat)
    kept = ix["dst_of"] >= 0
    assert torch.equal(ix["row_src"][ix["dst_of"][kept].long()].long(), kept.nonzero().view(-1))
    for b in range(B):
        c = int(ix["counts"][b])
        assert torch.equal(ix["keep_local"][b, :c].long(), keep[b].nonzero().view(-1)) and bool((ix["keep_local"][b, c:] == -1).all())


@pytest.mark.parametrize("at", [torch.bfloat16, torch.float16])
def test_fold_w_ref_and_the_choice_of_inputs(at):
    """The reference against plain torch; and the inputs of the GPU test's cs check: the sum of the rounded weights and the sum of the
    unrounded products differ by far more than fp32 summation error, so a kernel that sums before rounding cannot pass."""
    g = _gen(11)
    N = 5
    W, gamma, beta, bias = (torch.randn(N, D, generator=g), 1.0 + 0.3 * torch.randn(D, generator=g), 0.2 * torch.randn(D, generator=g),
                            torch.randn(N, generator=g))
    Wf, cs, csu, bf = R.fold_w_ref(W, gamma, beta, bias, at)
    assert Wf.dtype == at and torch.equal(Wf, (W * gamma).to(at))
    _close(cs, Wf.double().sum(-1), "cs")
    _close(csu, (W.double() * gamma.double()).sum(-1), "cs unrounded")
    _close(bf, bias.double() + F.linear(W.double(), beta.double().view(1, D)).squeeze(-1), "bf")
    W, gamma, beta, bias = R.fold_w_biased_inputs(N, at, g)
    Wf, cs, csu, bf = R.fold_w_ref(W, gamma, beta, bias, at)
    cs32 = R.fold_w_ref(W, gamma, beta, bias, at, dtype=F32)[1].double()
    floor = float((cs32 - cs).abs().max())
    assert float((cs - csu).abs().min()) > 100 * (4 * floor + 4 * float(np.spacing(np.float32(cs.abs().max()))))


def test_split_images_and_e4m3():
    g = _gen(5)
    v = 3.0 * torch.randn(4, D, generator=g)
    hi, lo = R.split3_image_ref(v)
    assert hi.dtype == torch.float16 and torch.equal(hi, v.half())
    ok = v.abs() >= 2.0 ** -2
    assert float(((hi.double() + lo.double() - v.double()).abs() - 2.0 ** -21 * v.abs().double())[ok].max()) <= 0.0
    # e4m3 decode: every byte against torch's own type where it exists
    allb = torch.arange(256, dtype=torch.uint8)
    dec = R.e4m3_decode(allb)
    assert float(dec[0x7E]) == 448.0 and float(dec[0x01]) == 2.0 ** -9 and float(dec[0x08]) == 2.0 ** -6 and math.isnan(float(dec[0x7F]))
    if hasattr(torch, "float8_e4m3fn"):
        t = allb.view(torch.float8_e4m3fn).to(F64)
        fin = torch.isfinite(dec)
        assert torch.equal(torch.isfinite(t), fin) and torch.equal(t[fin], dec[fin])
    # the image layout and the half-step rule on a round-to-nearest of our own
    img = torch.zeros(2, 2 * D, dtype=torch.float16)
    raw = img.view(torch.uint8)
    raw[:, 2 * D:3 * D] = 0x38   # 1.0
    raw[:, 3 * D:] = 0xB8        # -1.0
    h16, h8, l8 = R.f8_image_parts(img)
    assert h16.shape == (2, D) and float(R.e4m3_decode(h8).min()) == 1.0 and float(R.e4m3_decode(l8).max()) == -1.0
    hi16, s_hi, s_lo = R.f8_sources_ref(1000.0 * v)
    assert float(s_hi.abs().max()) == 448.0 and torch.equal(hi16, (1000.0 * v).half())
    grid = dec[torch.isfinite(dec)]
    for s in (R.f8_sources_ref(v)[1].reshape(-1), R.f8_sources_ref(v)[2].reshape(-1)):
        nearest = grid[(grid.view(1, -1) - s.view(-1, 1)).abs().argmin(1)]
        assert bool(((nearest - s).abs() <= R.e4m3_half_step(s)).all())


def test_embed_refs():
    g = _gen(9)
    img = torch.randn(2, 3, 224, 224, generator=g)
    cols = R.im2col_ref(img)
    unf = F.unfold(img, kernel_size=16, stride=16).transpose(1, 2).reshape(2 * NP, D)   # (c, i, j) channel order, patches row-major
    assert torch.equal(cols, unf)
    assert float(cols[NP + 3 * 14 + 5, 2 * 256 + 7 * 16 + 9]) == float(img[1, 2, 3 * 16 + 7, 5 * 16 + 9])
    src = torch.randn(8, D, generator=g)
    p = R.pad_convert_ref(src, 64, D, False, torch.bfloat16)
    assert torch.equal(p[:8], src.bfloat16()) and float(p[8:].abs().max()) == 0.0
    t = R.pad_convert_ref(src, D, 64, True, torch.float16)
    assert torch.equal(t[:, :8], src.t().half()) and float(t[:, 8:].abs().max()) == 0.0
