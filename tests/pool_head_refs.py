"""References of the mean-pooled / fc_norm classification head (DYT_CREATE_AVG_POOL, DYT_CREATE_FC_NORM), for tests/test_avg_pool_host.py
and tests/test_gpu_avg_pool.py.

The oracle (oracle/dyt_oracle.py) restates the reference with ``global_pool='token'`` and a final ``norm``.  With ``fc_norm`` the reference's
final norm is an Identity and the head reads ``fc_norm(pool(x))`` of the block stack's un-normalised output (models/vision_transformer_IN21K.py
:314-317, :375-380).  ``forward`` therefore runs the oracle for the block stack (``return_blocks=True``, ``blocks[-1]``) and restates pool +
fc_norm + head in torch; autograd carries gradients through ``blocks[-1]`` into the oracle's blocks.  tests/test_avg_pool_host.py pins these
functions to fixtures recorded from the real reference (tests/golden/pool/*.npz).

``head_ref`` is the head alone on given tokens, in a chosen dtype (float64 = the reference, float32 = the error floor of plain fp32
arithmetic; the rule of tests/tail_refs.py)."""
import torch
import torch.nn.functional as F

from oracle import dyt_oracle as O

POOLS = ("avg", "token")


def pool_rows(tokens, pool):
    """[B,197,768] -> [B,768]: the mean of the 196 patch rows (cls row excluded) or the cls row (reference :377)."""
    assert pool in POOLS, pool
    return tokens[:, 1:].mean(dim=1) if pool == "avg" else tokens[:, 0]


def _oracle_sd(sd):
    """The oracle's forward applies ``norm.*`` and a cls head of its own; its logits are discarded here -- give it an identity-like norm."""
    out = {k: v for k, v in sd.items() if not k.startswith("fc_norm.")}
    out["norm.weight"] = torch.ones_like(sd["fc_norm.weight"]).detach()
    out["norm.bias"] = torch.zeros_like(sd["fc_norm.bias"]).detach()
    return out


def forward(sd, x, g1=None, g2=None, keep_masks=None, scale=0.1, complete_model=False, training=True, mode="masked", pool="avg", **kw):
    """oracle.forward's contract for a model built with fc_norm: ``sd`` has ``fc_norm.*`` and no ``norm.*``.  Returns (logits, aux); aux
    also holds ``blocks`` (the oracle's) and ``pre_logits`` = fc_norm(pool(blocks[-1]))."""
    assert "fc_norm.weight" in sd and "norm.weight" not in sd
    _, aux = O.forward(_oracle_sd(sd), x, g1, g2, keep_masks, scale, complete_model, training, mode, return_blocks=True, **kw)
    pre = O.layer_norm(pool_rows(aux["blocks"][-1], pool), sd["fc_norm.weight"], sd["fc_norm.bias"])   # :377-378
    aux = dict(aux, pre_logits=pre)
    return F.linear(pre, sd["head.weight"], sd["head.bias"]), aux   # :380


def trainable_names(sd):
    """The freeze rule (main_image.py:250-256) on an fc_norm-keyed state dict: the oracle's names plus fc_norm.*."""
    return [k for k in sd if k in O.trainable_names(sd) or k.startswith("fc_norm.")]


def step_loss(sd, x, y, g1, g2, keep_masks, scale=0.1, mode="masked", pool="avg", token_target_ratio=0.5, token_loss_ratio=2.0,
              token_minimal=0.0, token_minimal_weight=0.0, **kw):
    """oracle.step_loss (engine_finetune.py:47-65) with the pooled head."""
    out_s, tok = forward(sd, x, g1[0], g2[0], None if keep_masks is None else keep_masks[0], scale, False, True, mode, pool, **kw)
    out_t, _ = forward(sd, x, g1[1], g2[1], None if keep_masks is None else keep_masks[1], scale, True, True, mode, pool, **kw)
    kl = F.kl_div(F.log_softmax(out_s, dim=-1), F.log_softmax(out_t.detach(), dim=-1), reduction="batchmean", log_target=True)
    teacher = F.cross_entropy(out_t, y)
    loss, d = O.ada_loss(out_s, tok["token_select"], y, token_target_ratio, token_loss_ratio, token_minimal, token_minimal_weight)
    loss = loss + teacher + kl
    return loss, dict(d, teacher_loss=teacher, distillation_loss=kl, loss=loss), (out_s, out_t, tok)


def step_grads(sd, x, y, g1, g2, keep_masks, **kw):
    """Loss components and the gradients of the 76 trainable tensors of one step (oracle.step_grads with the pooled head)."""
    names = trainable_names(sd)
    leaf = {k: (v.detach().clone().requires_grad_(True) if k in names else v.detach()) for k, v in sd.items()}
    loss, d, outs = step_loss(leaf, x, y, g1, g2, keep_masks, **kw)
    grads = torch.autograd.grad(loss, [leaf[k] for k in names])
    return {k: v.detach() for k, v in d.items()}, dict(zip(names, grads)), outs


def head_ref(tokens, fn_w, fn_b, head_w, head_b, dlogits, pool, dtype=torch.float64):
    """The pooled head alone on ``tokens`` [B,197,768] in ``dtype``: (logits, d tokens, d fc_norm.weight, d fc_norm.bias, d head.weight,
    d head.bias) for the upstream gradient ``dlogits`` (None: logits alone).  eps is the float32 value of 1e-6 widened, as in tail_refs."""
    import numpy as np
    cv = lambda t: t.detach().to("cpu", dtype)   # noqa: E731
    leaves = [cv(t).requires_grad_(True) for t in (tokens, fn_w, fn_b, head_w, head_b)]
    x, gw, gb, W, b = leaves
    r = pool_rows(x, pool)
    mean = r.mean(-1, keepdim=True)
    var = ((r - mean) ** 2).mean(-1, keepdim=True)
    y = (r - mean) / (var + float(np.float32(1e-6))).sqrt() * gw + gb
    logits = y @ W.t() + b
    if dlogits is None:
        return (logits.detach(),) + (None,) * 5
    grads = torch.autograd.grad((logits * cv(dlogits)).sum(), leaves)
    return (logits.detach(),) + tuple(grads)
