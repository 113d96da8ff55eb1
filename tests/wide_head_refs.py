"""Plain-torch CPU reference of the wide classification head (csrc/head_wide.hip), for tests/test_gpu_wide_head.py: the whole head --
final LayerNorm (eps 1e-6) of the cls rows, Linear(768, C) -- and its backward, from torch.autograd in the given dtype.  float64 is the
reference; the GPU tests evaluate it a second time in float32 to learn the error floor of plain fp32 arithmetic on the very inputs of a
case (the rule of tests/test_gpu_step_tail.py).  tests/test_wide_head_host.py pins it to torch's own modules."""
import torch

from tail_refs import f32


def head_full_ref(cls_x, norm_w, norm_b, head_w, head_b, dlogits, dtype=torch.float64):
    """``cls_x`` [B, 768] un-normalised cls rows.  Returns (logits [B, C], dx [B, 768], d head.weight [C, 768], d head.bias [C]) for the
    upstream gradient ``dlogits`` [B, C] (None: logits alone, the three gradients None).  The arithmetic of tail_refs.head_ref, with the
    input a leaf as well."""
    cv = lambda t: t.detach().to("cpu", dtype)
    x = cv(cls_x).requires_grad_(True)
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    y = (x - mean) / (var + f32(1e-6)).sqrt() * cv(norm_w) + cv(norm_b)
    W, b = cv(head_w).requires_grad_(True), cv(head_b).requires_grad_(True)
    logits = y @ W.t() + b
    if dlogits is None:
        return logits.detach(), None, None, None
    dx, dW, db = torch.autograd.grad((logits * cv(dlogits)).sum(), (x, W, b))
    return logits.detach(), dx, dW, db
