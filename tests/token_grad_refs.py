"""CPU references of the token-level training route (dyt_forward_taps / dyt_backward_tokens, VisionTransformer.forward_features with
out_indices), for tests/test_token_grad_host.py and tests/test_gpu_token_grad.py.

tap_loss_grads: the oracle's forward with return_blocks, a LINEAR functional of everything the route returns,

    L = <LN_final(blocks[-1]), R_tokens> + sum_i <blocks[i + 1], R_taps[i]> + <token_select, R_ts> + <token_logits, R_tl>

and torch.autograd.grad over the trainable tensors in front of the tokens (adapters, gates, adapter LayerNorms, learnable scales; the
head is behind the tokens).  A linear functional makes the R's exactly the gradients the library is handed: dtokens = R_tokens,
dtaps[i] = R_taps[i], dtoken_select = R_ts, dtoken_logits = R_tl.  blocks[i + 1] is the residual stream behind block i (tap i).

ln_bwd_tap_ref: tests/rowbwd_refs.py's restatement of ln_bwd_kernel plus the one add of the tapped instantiations."""
import torch

import rowbwd_refs as RB
from oracle import dyt_oracle as O


def backbone_names(sd):
    """The trainable tensors a gradient on tokens / taps / gate outputs can reach: the oracle's freeze rule without the head side."""
    return [k for k in O.trainable_names(sd) if not (k.startswith("head.") or k.startswith("fc_norm."))]


def tap_functional(sd, x, draws, R_tokens=None, R_taps=None, R_ts=None, R_tl=None, depth=O.DEPTH, mode="masked", complete_model=False,
                   scale=0.1, training=True, final_norm=True, drop_scales=None):
    """(L, outs): the functional above on ``sd`` as it is (no leaves made), outs = dict(tokens, blocks, token_select, token_logits).
    draws = (g1, g2, keep) of this pass ([depth,B,196] x 2, [depth,B*197,r]) or None.  R_taps: {block index: R} (or None).
    final_norm=False: the model's final norm is an identity (fc_norm models): tokens = blocks[-1]."""
    g1, g2, keep = draws if draws is not None else (None, None, None)
    _, out = O.forward(sd, x, g1, g2, keep, scale, complete_model, training, mode, depth=depth, return_blocks=True, drop_scales=drop_scales)
    blocks = out["blocks"]
    tokens = O.layer_norm(blocks[-1], sd["norm.weight"], sd["norm.bias"]) if final_norm else blocks[-1]
    ts, tl = out["token_select"][..., 0], out["token_logits"][..., 0]   # [B, depth, 196]
    L = tokens.new_zeros(())
    if R_tokens is not None:
        L = L + (tokens * R_tokens.to(tokens.dtype)).sum()
    for i, R in (R_taps or {}).items():
        L = L + (blocks[i + 1] * R.to(tokens.dtype)).sum()
    if R_ts is not None:
        L = L + (ts * R_ts.to(tokens.dtype)).sum()
    if R_tl is not None:
        L = L + (tl * R_tl.to(tokens.dtype)).sum()
    return L, dict(tokens=tokens, blocks=blocks, token_select=ts, token_logits=tl)


def tap_loss_grads(sd, x, draws, R_tokens=None, R_taps=None, R_ts=None, R_tl=None, dtype=torch.float32, **kw):
    """(grads {name: tensor}, outs): gradients of L over backbone_names(sd), everything computed in ``dtype``; a tensor the functional
    does not reach gets zeros."""
    names = backbone_names(sd)
    cv = lambda v: v.detach().to(dtype) if v.is_floating_point() else v.detach()   # noqa: E731
    leaf = {k: (cv(v).clone().requires_grad_(True) if k in names else cv(v)) for k, v in sd.items()}
    draws_t = None if draws is None else (draws[0].to(dtype), draws[1].to(dtype), draws[2])
    if kw.get("drop_scales") is not None:
        kw = dict(kw, drop_scales=kw["drop_scales"].to(dtype))
    L, outs = tap_functional(leaf, x.to(dtype), draws_t, R_tokens, R_taps, R_ts, R_tl, **kw)
    grads = torch.autograd.grad(L, [leaf[k] for k in names], allow_unused=True)
    grads = {k: (torch.zeros_like(leaf[k]) if g is None else g.detach()) for k, g in zip(names, grads)}
    return grads, {k: ([b.detach() for b in v] if isinstance(v, list) else v.detach()) for k, v in outs.items()}


def unit_R(gen, B, depth, taps=(), tokens=True, gates=False, n_tok=197):
    """Random unit-variance R's scaled by 1 / (B * 197): the gradient magnitudes of a mean loss.  -> (R_tokens, {i: R_tap}, R_ts, R_tl)"""
    s = 1.0 / (B * n_tok)
    rt = torch.randn(B, n_tok, 768, generator=gen) * s if tokens else None
    rtaps = {i: torch.randn(B, n_tok, 768, generator=gen) * s for i in taps}
    rts = torch.randn(B, depth, n_tok - 1, generator=gen) * s if gates else None
    rtl = torch.randn(B, depth, n_tok - 1, generator=gen) * s if gates else None
    return rt, rtaps, rts, rtl


def ln_bwd_tap_ref(dy, x, mean, rstd, w, tap, base=None, base_at=None, gs=1.0, h_next=None, dst_of_next=None, dtype=torch.float64):
    """(d, dmask_next) of the tapped ln_bwd_kernel: d = LNbwd(dy / gs) + (base | base_at / gs | 0) + tap, the tap added last;
    dmask_next from that d (rowbwd_refs.ln_bwd_kernel_ref with the one add in front of every output)."""
    d, _ = RB.ln_bwd_kernel_ref(dy, x, mean, rstd, w, base=base, base_at=base_at, gs=gs, dtype=dtype)
    d = d + tap.detach().to("cpu", dtype)
    _, dmask = RB.bwd_prep_ref(d, h_next, dst_of_next, None, dtype)
    return d, dmask
