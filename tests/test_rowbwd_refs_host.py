"""Pins tests/rowbwd_refs.py -- the fp64 references tests/test_gpu_row_bwd.py holds the backward row kernels against -- to torch autograd,
at 1e-12 relative in float64 (the same operation written twice), so that the references cannot drift together with the kernels.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import rowbwd_refs as R

TOL = 1e-12
F64 = torch.float64
NT, NP, D = R.NT, R.NP, R.D
EPS = 1e-6


def _close(a, b, what):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    err = float((a - b).abs().max()) if a.numel() else 0.0
    assert a.shape == b.shape and err <= TOL * max(1.0, float(b.abs().max()) if b.numel() else 1.0), "%s: |d| = %.3e" % (what, err)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _stats(x):
    mean = x.mean(-1)
    var = ((x - mean.view(-1, 1)) ** 2).mean(-1)
    return mean, 1.0 / (var + EPS).sqrt()


def _keep(B, g):
    """maskf [M] (cls kept, about half of the patches) and dst_of [M] (compact row or -1)."""
    maskf = (torch.rand(B, NT, generator=g) < 0.5).to(F64)
    maskf[:, 0] = 1.0
    maskf = maskf.reshape(-1)
    dst_of = torch.where(maskf != 0, torch.cumsum(maskf, 0).long() - 1, torch.full((B * NT,), -1))
    return maskf, dst_of


@pytest.mark.parametrize("rows", [1, 5, 33])
def test_ln_refs_are_layer_norm_backward(rows):
    g = _gen(rows)
    x = (2.0 * torch.randn(rows, D, generator=g, dtype=F64) + 0.5).requires_grad_(True)
    w = (1.0 + 0.3 * torch.randn(D, generator=g, dtype=F64)).requires_grad_(True)
    b = torch.zeros(D, dtype=F64, requires_grad=True)
    dy = torch.randn(rows, D, generator=g, dtype=F64)
    dx, dw, db = torch.autograd.grad((F.layer_norm(x, (D,), w, b, eps=EPS) * dy).sum(), (x, w, b))
    mean, rstd = _stats(x.detach())
    _close(R.ln_bwd_ref(dy, x, mean, rstd, w), dx, "ln_bwd_ref")
    _close(R.ln_param_grad_ref(dy, x, mean, rstd), torch.cat([dw, db]), "ln_param_grad_ref")
    _close(R.ln_param_grad_ref(dy * 4096.0, x, mean, rstd, gs=4096.0), torch.cat([dw, db]), "ln_param_grad_ref with gs")
    base = torch.randn(rows, D, generator=g, dtype=F64)
    h = torch.randn(rows, D, generator=g, dtype=F64)
    dst = torch.arange(rows) - 1   # row 0 dropped
    d, dm = R.ln_bwd_kernel_ref(dy * 4096.0, x, mean, rstd, w, base_at=base * 4096.0, gs=4096.0, h_next=h, dst_of_next=dst)
    _close(d, dx + base, "ln_bwd_kernel_ref d")
    want = ((dx + base)[1:] * h[:rows - 1]).sum(-1)
    _close(dm[1:], want, "ln_bwd_kernel_ref dmask_next")
    assert float(dm[0]) == 0.0
    d2, dm2 = R.ln_bwd_kernel_ref(dy, x, mean, rstd, w, base=base)
    _close(d2, dx + base, "ln_bwd_kernel_ref with base")
    assert float(dm2.abs().max()) == 0.0


def test_bwd_prep_ref_is_the_mask_gradient_of_the_scattered_mlp_output():
    """x' = u + scatter(mask[t] h[dst_of[t]]): d L / d mask[t] = <g[t], h[dst_of[t]]> for the kept tokens, and the gradient reaching
    h[dst_of[t]] is mask[t] g[t]."""
    g = _gen(3)
    B = 1
    maskf, dst_of = _keep(B, g)
    K = int(maskf.sum())
    h = torch.randn(K, D, generator=g, dtype=F64).requires_grad_(True)
    m = maskf.clone().requires_grad_(True)
    up = torch.randn(B * NT, D, generator=g, dtype=F64)
    kept = dst_of >= 0
    xo = torch.zeros(B * NT, D, dtype=F64)
    xo = xo.index_put((kept.nonzero().view(-1),), m[kept].view(-1, 1) * h[dst_of[kept]])
    dm, dh = torch.autograd.grad((xo * up).sum(), (m, h))
    rows, dmask = R.bwd_prep_ref(up, h, dst_of, maskf)
    _close(dmask[kept], dm[kept], "dmask")
    assert float(dmask[~kept].abs().max()) == 0.0
    _close(rows[kept], dh[dst_of[kept]], "dH rows")


@pytest.mark.parametrize("training,tau", [(1, 5.0), (0, 1.0)])
@pytest.mark.parametrize("user_grads", [False, True])
def test_tok_bwd_ref_is_autograd_of_gate_and_scattered_ln2(training, tau, user_grads):
    """One block's tail written with torch operators: the kept tokens' LN2 outputs feed a linear read-out (upstream gradient dA2, times
    the image's stochastic-depth factor), the gate's y_soft = sigmoid((<u, w> + b + c) / tau) receives dmask + ext, the gate's logits
    receive dtoken_logits, and u also receives the residual gradient and the adapter's dgrad."""
    g = _gen(11 + training + 2 * user_grads)
    B = 3
    M = B * NT
    maskf, dst_of = _keep(B, g)
    maskf.view(B, NT)[1, 1:] = 0.0   # one image with every patch dropped
    maskf.view(B, NT)[2, :] = 1.0    # one with none
    dst_of = torch.where(maskf != 0, torch.cumsum(maskf, 0).long() - 1, torch.full((M,), -1))
    kept = dst_of >= 0
    K = int(kept.sum())
    u = (torch.randn(M, D, generator=g, dtype=F64) * 1.5 + 0.2).requires_grad_(True)
    ln2_w = 1.0 + 0.3 * torch.randn(D, generator=g, dtype=F64)
    wg = (0.05 * torch.randn(D, generator=g, dtype=F64)).requires_grad_(True)
    bg = torch.zeros(1, dtype=F64, requires_grad=True)
    c = torch.randn(M, generator=g, dtype=F64)
    gs = 4096.0
    dA2 = torch.randn(K, D, generator=g, dtype=F64)
    du_in, dad = torch.randn(M, D, generator=g, dtype=F64), torch.randn(M, D, generator=g, dtype=F64)
    dmask = torch.randn(M, generator=g, dtype=F64) * kept
    branch = torch.tensor([0.0, 1.0 / 0.9, 1.0], dtype=F64)
    dtok = torch.tensor([0.3, -0.7, 0.2], dtype=F64)
    sel = torch.randn(B, NP, generator=g, dtype=F64) if user_grads else None
    dlg = torch.randn(B, NP, generator=g, dtype=F64) if user_grads else None
    patch = (torch.arange(M) % NT) != 0
    bs = branch[torch.arange(M) // NT]

    logits = u @ wg + bg
    soft = torch.sigmoid((logits + c) / tau) if training else torch.sigmoid(logits)
    if user_grads:
        ext = torch.cat([torch.zeros(B, 1, dtype=F64), sel], 1).reshape(M)
        lg_up = torch.cat([torch.zeros(B, 1, dtype=F64), dlg], 1).reshape(M)
    else:
        ext = dtok[0] + torch.where(maskf != 0, dtok[2], dtok[1])
        lg_up = torch.zeros(M, dtype=F64)
    xn = F.layer_norm(u[kept], (D,), ln2_w, None, eps=EPS)
    L = (xn * dA2 * bs[kept].view(-1, 1)).sum() + (soft * (dmask * bs + ext))[patch].sum() + (logits * lg_up)[patch].sum() \
        + (u * (du_in + dad)).sum()
    du_want, dw_want, db_want = torch.autograd.grad(L, (u, wg, bg))

    mean, rstd = _stats(u.detach())
    got, d_gate, _ = R.tok_bwd_ref(M, u, du_in_at=du_in * gs, dad=dad * gs, dA2=dA2 * gs, dst_of=dst_of, mean2=mean, rstd2=rstd, ln2_w=ln2_w,
                                   gate_w=wg, soft=soft, maskf=maskf, dmask=dmask, dtoken_select=sel, dtoken_logits=dlg,
                                   dtok=None if user_grads else dtok, training=training, tau=tau, gs=gs, branch_scale=branch)
    _close(got, du_want, "du")
    _close(d_gate[:D], dw_want, "d gate weight")
    _close(d_gate[D:], db_want, "d gate bias")
    # the fp32 stream form reads du instead of du_in_at; the dense form takes dst_of = identity
    got2, _, _ = R.tok_bwd_ref(M, u, du=du_in + dad, dA2=dA2 * gs, dst_of=dst_of, mean2=mean, rstd2=rstd, ln2_w=ln2_w, gate_w=wg, soft=soft,
                               maskf=maskf, dmask=dmask, dtoken_select=sel, dtoken_logits=dlg, dtok=None if user_grads else dtok,
                               training=training, tau=tau, gs=gs, branch_scale=branch)
    _close(got2, du_want, "du from the fp32 stream")


def test_tok_bwd_ref_cls_tail_and_cat_correction():
    g = _gen(21)
    B = 2
    M = B * NT
    u = torch.randn(M, D, generator=g, dtype=F64).requires_grad_(True)
    ln2_w = 1.0 + 0.3 * torch.randn(D, generator=g, dtype=F64)
    g_cls, dA2 = torch.randn(B, D, generator=g, dtype=F64), torch.randn(B, D, generator=g, dtype=F64)
    cls = (torch.arange(M) % NT) == 0
    L = (F.layer_norm(u[cls], (D,), ln2_w, None, eps=EPS) * dA2).sum() + (u[cls] * g_cls).sum()
    (want,) = torch.autograd.grad(L, u)
    mean, rstd = _stats(u.detach())
    got, d_gate, _ = R.tok_bwd_ref(M, u, g_cls=g_cls, dA2=dA2, mean2=mean, rstd2=rstd, ln2_w=ln2_w)
    _close(got, want, "cls-only tail")
    assert float(got[~cls].abs().max()) == 0.0 and float(d_gate.abs().max()) == 0.0
    # cat: the saved MLP output carries s d_act W_up^T, so dmask = <g, h'> is too large by <d_act, ddz> / gs with ddz = gs s g W_up
    maskf, dst_of = _keep(B, g)
    s, gs = 0.1, 4096.0
    gup = torch.randn(M, D, generator=g, dtype=F64)
    h = torch.randn(M, D, generator=g, dtype=F64)
    dact = torch.randn(M, 64, generator=g, dtype=F64).clamp(min=0)
    wup = 0.02 * torch.randn(D, 64, generator=g, dtype=F64)
    kept = maskf != 0
    dm_plain = (gup * h).sum(-1) * kept
    dm_cat = (gup * (h + s * dact @ wup.t())).sum(-1) * kept
    ddz = gs * s * (gup @ wup) * 2.0 ** 5   # lifted by 2^5: the device word takes it out again
    wg = 0.05 * torch.randn(D, generator=g, dtype=F64)
    soft = torch.rand(M, generator=g, dtype=F64)
    kw = dict(gate_w=wg, soft=soft, maskf=maskf, training=1, tau=5.0)
    a = R.tok_bwd_ref(M, u, dmask=dm_plain, **kw)
    b = R.tok_bwd_ref(M, u, dmask=dm_cat, cat_dact=dact, cat_ddz=ddz, cat_ddz_scale=1.0 / gs, cat_ddz_dscale=torch.tensor([2.0 ** -5], dtype=F64), **kw)
    for x, y, what in zip(a, b, ("du", "d_gate", "dlogit")):
        _close(y, x, "cat correction: " + what)


def test_fp32_evaluation_keeps_fp32_and_split3_value_reads_the_layout():
    g = _gen(31)
    x, dy, w = torch.randn(4, D, generator=g), torch.randn(4, D, generator=g), torch.randn(D, generator=g)
    mean, rstd = _stats(x.double())
    a = R.ln_bwd_ref(dy, x, mean.float(), rstd.float(), w, dtype=torch.float32)
    b = R.ln_bwd_ref(dy, x, mean.float(), rstd.float(), w)
    assert a.dtype == torch.float32 and b.dtype == F64 and 0.0 < float((a.double() - b).abs().max()) < 1e-4
    v = torch.randn(3, D, generator=g) * 8.0
    hi = v.to(torch.float16)
    lo = (v - hi.float()).to(torch.float16)
    img = torch.cat([hi, lo], 1)
    assert float((R.split3_value(img, 8.0) - v.double() / 8.0).abs().max()) <= 2.0 ** -21 * float(v.abs().max()) / 8.0
    assert torch.equal(R.split3_value(img, 1.0, hi_only=True), hi.double())
