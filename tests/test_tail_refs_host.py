"""Pins tests/tail_refs.py -- the fp64 references tests/test_gpu_step_tail.py holds the step's tail kernels against -- to torch's own
operators, at 1e-12 in float64, so that the references cannot drift together with the kernels.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import tail_refs as R

TOL = 1e-12
F64 = torch.float64


def _close(a, b, what):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    err = float((a - b).abs().max()) if a.numel() else 0.0
    assert a.shape == b.shape and err <= TOL * max(1.0, float(b.abs().max()) if b.numel() else 1.0), "%s: |d| = %.3e" % (what, err)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("B,C", [(1, 1), (3, 2), (5, 65), (7, 1000)])
def test_loss_ref_is_cross_entropy_plus_batchmean_kl(B, C, soft):
    g = _gen(B * 1000 + C)
    s = (3 * torch.randn(B, C, generator=g, dtype=F64)).requires_grad_(True)
    t = (3 * torch.randn(B, C, generator=g, dtype=F64)).requires_grad_(True)
    if soft:   # rows that do NOT sum to 1 as well: F.cross_entropy takes any non-negative weights
        y = torch.rand(B, C, generator=g, dtype=F64) * torch.tensor([0.5, 1.0, 2.0], dtype=F64)[torch.arange(B) % 3].view(B, 1)
    else:
        y = torch.randint(0, C, (B,), generator=g)
    losses, ds, dt, dtok = R.loss_ref(s, t, y, None, 1, 0.5, 2.0, 0.3, 2.0)
    base, teacher = F.cross_entropy(s, y), F.cross_entropy(t, y)
    kl = F.kl_div(F.log_softmax(s, -1), F.log_softmax(t.detach(), -1), reduction="batchmean", log_target=True)
    gs, gt = torch.autograd.grad(base + teacher + kl, (s, t))
    _close(losses[1], base.detach(), "base")
    _close(losses[3], teacher.detach(), "teacher")
    _close(losses[4], kl.detach(), "kl")
    _close(losses[0], (base + teacher + kl).detach(), "loss without gate statistics")
    _close(ds, gs, "dlogits_s")
    _close(dt, gt, "dlogits_t")
    assert float(losses[2]) == 0.0 and float(dtok.abs().max()) == 0.0 and losses.shape == (7,)


@pytest.mark.parametrize("token_minimal,weight", [(0.0, 0.0), (0.0, 2.0), (0.3125, 0.0), (0.3125, 2.0), (1.5, 2.0), (1.0, 2.0)])
def test_loss_ref_token_terms_are_adaloss_and_dtok_is_its_mask_gradient(token_minimal, weight):
    """The token loss equals models.losses.AdaLoss._get_token_loss on the reference-shaped mask [B, depth, 196, 1]; dtok, laid out as
    tok_bwd consumes it (dtok[0] + (kept ? dtok[2] : dtok[1]) per element), equals autograd on that module and a central finite
    difference of the fp64 token loss on the mask relaxed to real values (token_minimal 0.3125 / 1.5, exact in float32 like every scalar here: the clamp's kink is away from 0 and 1)."""
    from models.losses import AdaLoss
    depth, B = 2, 3
    counts = torch.tensor([[1, 197, 58], [120, 2, 196]], dtype=torch.int32)
    s = torch.randn(B, 5, generator=_gen(1), dtype=F64)
    y = torch.tensor([0, 4, 2])
    target, ratio = 0.5, 2.0
    losses, _, _, dtok = R.loss_ref(s, s, y, counts, depth, target, ratio, token_minimal, weight)
    mask = R.mask_from_counts(counts)
    ada = AdaLoss(None, token_target_ratio=target, token_loss_ratio=ratio, token_minimal=token_minimal, token_minimal_weight=weight)
    mref = mask.permute(1, 0, 2).unsqueeze(-1).clone().requires_grad_(True)
    tl = ratio * ada._get_token_loss(s, mref)
    _close(losses[2], tl.detach(), "token loss")
    _close(losses[5], mask.mean(), "keep ratio")
    _close(losses[6], (counts.sum() - counts.numel()).to(F64), "kept tokens")
    per_elem = dtok[0] + torch.where(mask.permute(1, 0, 2).unsqueeze(-1) != 0, dtok[2], dtok[1])
    if tl.requires_grad:
        _close(per_elem, torch.autograd.grad(tl, mref)[0], "dtok against autograd on AdaLoss")
    if token_minimal in (0.0, 1.0):
        return   # the clamp's kink sits ON a mask value: one-sided there, autograd's convention (x >= min passes) is checked above

    def f(m):
        return float(ratio * R.token_term(m, R.f32(target), R.f32(token_minimal), R.f32(weight)))
    h = 1e-2   # the terms are piecewise linear / quadratic in each element: the central quotient is exact up to rounding
    for kind in (0.0, 1.0):
        e = torch.zeros_like(mask)
        e[tuple((mask == kind).nonzero()[0])] = h
        fd = (f(mask + e) - f(mask - e)) / (2 * h)   # the mask relaxed to real values around one dropped / one kept element
        want = float(dtok[0] + (dtok[2] if kind else dtok[1]))
        assert abs(fd - want) <= 1e-8 * max(1.0, abs(want)), (kind, fd, want)


def test_adamw_ref_is_torch_adamw_over_five_steps():
    """Betas, lr, eps and weight decay exactly representable in float32, so widening them changes nothing against torch's doubles."""
    lr, b1, b2, eps, wd = 2.0 ** -10, 0.875, 1.0 - 2.0 ** -10, 2.0 ** -27, 0.0625
    g = _gen(5)
    p0 = 0.02 * torch.randn(1000, generator=g, dtype=F64)
    p0[::3] = 0.0
    for scale in (1.0, 0.125):
        par = p0.clone().requires_grad_(True)
        opt = torch.optim.AdamW([par], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
        p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        gg = _gen(6)
        for step in range(1, 6):
            grad = torch.randn(1000, generator=gg, dtype=F64) * 10.0 ** torch.empty(1000, dtype=F64).uniform_(-9, 2, generator=gg)
            par.grad = grad * scale
            opt.step()
            p, m, v = R.adamw_ref(p, grad, m, v, step, lr, b1, b2, eps, wd, scale)
            st = opt.state[par]
            _close(p, par.detach(), "p at step %d" % step)
            _close(m, st["exp_avg"], "m at step %d" % step)
            _close(v, st["exp_avg_sq"], "v at step %d" % step)


@pytest.mark.parametrize("n", [1, 255, 65537])
@pytest.mark.parametrize("max_norm,pre_scale", [(1e9, 1.0), (1.0, 1.0), (0.5, 0.125), (0.25, -0.5)])
def test_clip_ref_is_clip_grad_norm(n, max_norm, pre_scale):
    """clip_ref(g, max_norm, pre_scale) = clip_grad_norm_ applied to pre_scale * g, handed back in g's own scale."""
    g = torch.randn(n, generator=_gen(n), dtype=F64)
    par = torch.zeros(n, dtype=F64, requires_grad=True)
    par.grad = g * R.f32(pre_scale)
    total = torch.nn.utils.clip_grad_norm_([par], R.f32(max_norm))
    norm, clipped = R.clip_ref(g, max_norm, pre_scale)
    _close(norm, total, "norm")
    _close(clipped * R.f32(pre_scale), par.grad, "clipped gradient")
    if float(total) + 1e-6 < max_norm:
        assert torch.equal(clipped, g)


@pytest.mark.parametrize("B,C", [(1, 1), (3, 5), (9, 65)])
def test_head_ref_is_layer_norm_then_linear(B, C):
    g = _gen(B + C)
    tokens = torch.randn(B, 197, 768, generator=g, dtype=F64)
    nw, nb = 1 + 0.1 * torch.randn(768, generator=g, dtype=F64), 0.1 * torch.randn(768, generator=g, dtype=F64)
    W = (0.02 * torch.randn(C, 768, generator=g, dtype=F64)).requires_grad_(True)
    b = (0.02 * torch.randn(C, generator=g, dtype=F64)).requires_grad_(True)
    dl = torch.randn(B, C, generator=g, dtype=F64)
    want = F.linear(F.layer_norm(tokens[:, 0], (768,), nw, nb, eps=R.f32(1e-6)), W, b)
    dW, db = torch.autograd.grad((want * dl).sum(), (W, b))
    logits, gW, gb = R.head_ref(tokens, nw, nb, W, b, dl)
    _close(logits, want.detach(), "logits")
    _close(gW, dW, "d head.weight")
    _close(gb, db, "d head.bias")
    _close(R.head_ref(tokens[:, 0], nw, nb, W, b, None)[0], want.detach(), "logits from cls rows")


def test_fp32_evaluation_keeps_fp32_and_differs_from_fp64():
    """The ``dtype`` argument really runs the arithmetic in that type: the GPU tests' error floor is |fp32 - fp64| of these functions."""
    g = _gen(11)
    s, t = torch.randn(5, 65, generator=g), torch.randn(5, 65, generator=g)
    y = torch.randint(0, 65, (5,), generator=g)
    counts = torch.full((1, 5), 100, dtype=torch.int32)
    a = R.loss_ref(s, t, y, counts, 1, 0.5, 2.0, 0.3, 2.0, dtype=torch.float32)
    b = R.loss_ref(s, t, y, counts, 1, 0.5, 2.0, 0.3, 2.0)
    for x32, x64 in zip(a, b):
        assert x32.dtype == torch.float32 and x64.dtype == F64
    assert 0.0 < float((a[1].double() - b[1]).abs().max()) < 1e-5
    p = 0.02 * torch.randn(257, generator=g)
    gr = torch.randn(257, generator=g)
    z = torch.zeros(257)
    a = R.adamw_ref(p, gr, z, z, 2, 1e-3, 0.9, 0.999, 1e-8, 0.05, 1.0, dtype=torch.float32)
    b = R.adamw_ref(p, gr, z, z, 2, 1e-3, 0.9, 0.999, 1e-8, 0.05, 1.0)
    assert a[0].dtype == torch.float32 and 0.0 < float((a[0].double() - b[0]).abs().max()) < 1e-8
