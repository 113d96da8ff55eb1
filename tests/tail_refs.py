"""Plain-torch CPU references of the kernels that finish a step (csrc/step_tail.hip: loss_rows / loss_final, head_fwd / head_bwd_dw,
adamw / adamw_guarded / grad_nonfinite, sqsum / clip_scale), for tests/test_gpu_step_tail.py.

Every function takes ``dtype``: float64 is the reference; the GPU tests evaluate the same function a second time in float32 to learn how
far plain fp32 arithmetic is from fp64 on the very inputs of a case (their error floor).  Scalars that cross the C ABI as ``float`` are
widened from their float32 value (``f32``), so a comparison measures the arithmetic and not the rounding of 0.999 or 1e-8.
tests/test_tail_refs_host.py pins these functions to torch's own operators so that they cannot drift with the kernels."""
import math

import numpy as np
import torch

NP = 196   # patch tokens per image: the gate decides on these (the cls token is always kept)


def f32(x):
    """The double a C ``float`` argument holds for the Python number ``x``."""
    return float(np.float32(x))


def ulp(x):
    """Spacing of float32 at |x| (x: Python number or 0-dim tensor)."""
    return float(np.spacing(np.float32(abs(float(x)))))


def mask_from_counts(counts, dtype=torch.float64):
    """{0,1} mask [depth, B, 196] with counts[l, b] - 1 ones per (block, image): ``counts`` are the kept tokens per image INCLUDING the cls
    token (dyt_debug_dispatch).  Which patch positions carry the ones is irrelevant to the loss."""
    c = counts.to(torch.int64) - 1
    return (torch.arange(NP).view(1, 1, NP) < c.unsqueeze(-1)).to(dtype)


def _log_softmax(x):
    z = x - x.max(dim=-1, keepdim=True).values
    return z - z.exp().sum(dim=-1, keepdim=True).log()


def token_term(mask, target_ratio, token_minimal, token_minimal_weight):
    """AdaLoss._get_token_loss (models/losses.py; reference models/losses.py:62-82) on a mask tensor: its last axis has one decision per
    element (the reference's mask is [B, 12, 196, 1], so its mean(-1) is the element itself)."""
    tok = (mask.mean() - target_ratio) ** 2
    if token_minimal_weight > 0:
        tok = tok + token_minimal_weight * (token_minimal - mask).clamp(min=0.).sum()
    return tok


def loss_ref(logits_s, logits_t, targets_or_soft, counts, depth, target_ratio, loss_ratio, token_minimal, token_minimal_weight,
             dtype=torch.float64):
    """The step loss as include/dyt_hip.h states it for dyt_loss:
      loss = CE(s, y) + ratio * ((mean(mask) - target)^2 + w_min * sum(clamp(t_min - mask, 0))) + CE(t, y) + KL(log_softmax s || log_softmax t.detach())
    ``targets_or_soft``: int64 labels [B] or class-probability rows [B, C] (dyt_set_soft_targets).  ``counts`` int [depth, B] or None
    (no gate statistics: the token terms are 0).
    Returns (losses[7] = loss, base, scaled token loss, teacher CE, KL, mean keep ratio, kept tokens; dlogits_s; dlogits_t; dtok[3]).
    Gradients come from autograd.  dtok = {uniform, extra for a dropped, extra for a kept} gradient per mask element, i.e. what tok_bwd
    adds up as dtok[0] + (kept ? dtok[2] : dtok[1]): the ratio term's gradient is uniform over the mask; the minimal term's gradient is
    read at one dropped and one kept element (appended to the mask as a two-element probe so that both exist whatever the gate did)."""
    target_ratio, loss_ratio, token_minimal, token_minimal_weight = map(f32, (target_ratio, loss_ratio, token_minimal, token_minimal_weight))
    s = logits_s.detach().to("cpu", dtype).requires_grad_(True)
    t = logits_t.detach().to("cpu", dtype).requires_grad_(True)
    B = s.shape[0]
    lps, lpt = _log_softmax(s), _log_softmax(t)
    tg = targets_or_soft.detach().cpu()
    if tg.dtype == torch.int64:
        rows = torch.arange(B)
        base, teacher = -lps[rows, tg].sum() / B, -lpt[rows, tg].sum() / B
    else:
        tg = tg.to(dtype)
        base, teacher = -(tg * lps).sum() / B, -(tg * lpt).sum() / B
    lq = lpt.detach()
    kl = (lq.exp() * (lq - lps)).sum() / B
    zero = torch.zeros((), dtype=dtype)
    tok_scaled, mean, kept, dtok = zero, zero, zero, torch.zeros(3, dtype=dtype)
    if counts is not None:
        assert tuple(counts.shape) == (depth, B), (counts.shape, depth, B)
        mask = mask_from_counts(counts.cpu(), dtype).requires_grad_(True)
        tok_scaled = loss_ratio * token_term(mask, target_ratio, token_minimal, token_minimal_weight)
        (g_uniform,) = torch.autograd.grad(loss_ratio * token_term(mask, target_ratio, 0.0, 0.0), mask)
        assert float(g_uniform.max() - g_uniform.min()) == 0.0   # the ratio term pulls on every element alike
        d_drop = d_keep = zero
        if token_minimal_weight > 0:
            ext = torch.cat([mask.detach().flatten(), torch.tensor([0.0, 1.0], dtype=dtype)]).requires_grad_(True)   # + one dropped, one kept
            (g_min,) = torch.autograd.grad(loss_ratio * token_minimal_weight * (token_minimal - ext).clamp(min=0.).sum(), ext)
            d_drop, d_keep = g_min[-2], g_min[-1]
            assert bool(((g_min == d_drop) | (ext.detach() != 0)).all()) and bool(((g_min == d_keep) | (ext.detach() != 1)).all())
        dtok = torch.stack([g_uniform.flatten()[0], d_drop, d_keep]).detach()
        mean, kept = mask.detach().mean(), mask.detach().sum()
    loss = base + tok_scaled + teacher + kl
    ds, dt = torch.autograd.grad(loss, (s, t))
    losses = torch.stack([x.detach().to(dtype) for x in (loss, base, tok_scaled, teacher, kl, mean, kept)])
    return losses, ds, dt, dtok


def head_ref(tokens, norm_w, norm_b, head_w, head_b, dlogits, dtype=torch.float64):
    """forward_head of the image model (vision_transformer_IN21K.py:375-380): LayerNorm(eps 1e-6) of the cls row, then Linear.
    ``tokens`` [B, 197, 768] (the block stack's output) or the cls rows [B, 768].  Returns (logits, d head.weight, d head.bias) for the
    upstream gradient ``dlogits`` (None: logits alone)."""
    cv = lambda x: x.detach().to("cpu", dtype)
    x = cv(tokens)
    x = x[:, 0] if x.dim() == 3 else x
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    y = (x - mean) / (var + f32(1e-6)).sqrt() * cv(norm_w) + cv(norm_b)
    W, b = cv(head_w).requires_grad_(True), cv(head_b).requires_grad_(True)
    logits = y @ W.t() + b
    if dlogits is None:
        return logits.detach(), None, None
    dW, db = torch.autograd.grad((logits * cv(dlogits)).sum(), (W, b))
    return logits.detach(), dW, db


def adamw_ref(p, g, m, v, step, lr, b1, b2, eps, wd, grad_scale, dtype=torch.float64):
    """One torch.optim.AdamW update (decoupled decay, bias corrections formed in double whatever the tensors' dtype, as torch does) of
    the gradient ``grad_scale * g``; ``step`` is 1-based.  Returns the new (p, m, v)."""
    lr, b1, b2, eps, wd, grad_scale = map(f32, (lr, b1, b2, eps, wd, grad_scale))
    cv = lambda x: x.detach().to("cpu", dtype)
    p, g, m, v = cv(p), cv(g) * grad_scale, cv(m), cv(v)
    p = p * (1.0 - lr * wd)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    denom = v.sqrt() / math.sqrt(bc2) + eps
    return p - (lr / bc1) * (m / denom), m, v


def clip_ref(g, max_norm, pre_scale, dtype=torch.float64):
    """torch.nn.utils.clip_grad_norm_ on the gradient AdamW will see, ``pre_scale * g``: returns (norm = ||pre_scale g||_2,
    g * min(1, max_norm / (norm + 1e-6))) -- the stored gradient itself stays unscaled by ``pre_scale`` (dyt_clip_grad_norm)."""
    max_norm, pre_scale = f32(max_norm), f32(pre_scale)
    g = g.detach().to("cpu", dtype)
    norm = (g * g).sum().sqrt() * abs(pre_scale)
    coef = torch.clamp(max_norm / (norm + f32(1e-6)), max=1.0)
    return norm, g * coef
