"""Plain-torch CPU references of the forward row kernels (csrc/dispatch.hip, csrc/ln.hip, csrc/embed.hip: the token dispatcher, the LayerNorm
family around it, the folded form's weight side, the embedding prologue), for tests/test_gpu_row_fwd.py.

As tests/rowbwd_refs.py: every arithmetic function takes ``dtype`` -- float64 is the reference, float32 gives the error floor of plain fp32
arithmetic on the very inputs of a case -- and scalars that cross the C ABI as ``float`` are widened from their float32 value.  Each function
states the operation (include/dyt_hip.h: dyt_unit_gate ... dyt_unit_pad_convert), not the kernel's loop order.  The Gumbel noise of the
training route is reproduced exactly from tests/erase_refs.py's Philox4x32-10 and u01 (pinned there by known answers).
tests/test_rowfwd_refs_host.py pins these functions to torch."""
import numpy as np
import torch

import erase_refs as E
from tail_refs import f32

NT, NP, D = 197, 196, 768
F8_LO_SCALE = 4096.0   # csrc/dyt_common.h: 2^12 on the lo part of the hi16 / fp8 image


def _cv(x, dtype):
    return None if x is None else x.detach().to("cpu", dtype)


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------------
def layernorm_ref(x, w, b, eps, resid=None, dtype=torch.float64):
    """(out, mean, rstd): mean and biased variance over the last axis, rstd = (var + eps)^-1/2, out = (x - mean) rstd w + b (+ resid)."""
    x, w, b = _cv(x, dtype), _cv(w, dtype), _cv(b, dtype)
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / (var + f32(eps)).sqrt()
    out = (x - mean) * rstd * w + b
    if resid is not None:
        out = out + _cv(resid, dtype)
    return out, mean.squeeze(-1), rstd.squeeze(-1)


# ---- the gate --------------------------------------------------------------------------------------------------------------------
def gate_logit_ref(u, w, b, dtype=torch.float64):
    """[M]: <u[t], w> + b[0] for every row (the kernel writes the patch rows only)."""
    return (_cv(u, dtype) * _cv(w, dtype)).sum(-1) + _cv(b, dtype).reshape(())


def noise_from_words(words, dtype=torch.float64):
    """logit(u01(word)) = log(x) - log1p(-x), x = u01(word) (an fp32 value, widened exactly): Gumbel - Gumbel ~ Logistic(0, 1).
    The top word gives x = 1.0 exactly ((w >> 8) + 0.5 rounds up in fp32) and the noise +inf."""
    x = torch.from_numpy(np.ascontiguousarray(E.u01(words))).to(dtype)
    return torch.log(x) - torch.log1p(-x)


def gate_words(seed, subseq, batch):
    """uint32 [batch, 197]: word 0 of Philox4x32-10(key = seed, counter = (offset = t, subseq)), t = b * 197 + n."""
    t = np.arange(batch * NT, dtype=np.uint64).reshape(batch, NT)
    return E.philox(seed, np.uint64(int(subseq) & (2 ** 64 - 1)), t)[0]


def gate_noise_ref(seed, subseq, batch, dtype=torch.float64):
    """[batch, 197] (the cls column is drawn like the others and never used)."""
    return noise_from_words(gate_words(seed, subseq, batch), dtype)


def gate_soft_ref(logit, training, tau, noise=None, g1=None, g2=None, dtype=torch.float64):
    """(z, soft) per token: z = logit (eval), (logit + noise) / tau or (logit + g1 - g2) / tau (training); soft = 1 / (1 + exp(-z)).
    logit, noise, g1, g2 of one shape."""
    z = _cv(logit, dtype)
    if training:
        z = (z + _cv(noise, dtype)) if g1 is None else (z + _cv(g1, dtype) - _cv(g2, dtype))
        z = z / f32(tau)
    return z, 1.0 / (1.0 + torch.exp(-z))


def gate_keep_ref(soft, threshold, force_first=0):
    """bool [B, 197] from soft [B, 197]: the cls token always; a patch token n when soft > threshold, or n < force_first when that is > 0."""
    soft = soft.detach().to("cpu")
    if force_first > 0:
        keep = (torch.arange(NT) < force_first).expand(soft.shape[0], NT).clone()
    else:
        keep = soft > torch.tensor(f32(threshold), dtype=torch.float64).to(soft.dtype)
    keep[:, 0] = True
    return keep


# ---- index arrays ----------------------------------------------------------------------------------------------------------------
def index_ref(keep):
    """From a bool mask [B, 197], with torch's nonzero: dict of int32 tensors
      keep_local [B, 197] (the kept n of each image ascending, -1 behind them), counts [B],
      row_src [total0] (the kept rows t ascending), dst_of [B * 197] (compact row or -1), total [2], drop_src [total1] (dropped rows ascending)."""
    keep = keep.detach().to("cpu", torch.bool)
    B = keep.shape[0]
    flat = keep.reshape(-1)
    row_src = flat.nonzero().view(-1)
    drop_src = (~flat).nonzero().view(-1)
    dst_of = torch.full((B * NT,), -1, dtype=torch.int64)
    dst_of[row_src] = torch.arange(row_src.numel())
    keep_local = torch.full((B, NT), -1, dtype=torch.int64)
    for b in range(B):
        n = keep[b].nonzero().view(-1)
        keep_local[b, :n.numel()] = n
    i32 = torch.int32
    return dict(keep_local=keep_local.to(i32), counts=keep.sum(1).to(i32), row_src=row_src.to(i32), dst_of=dst_of.to(i32),
                total=torch.tensor([row_src.numel(), drop_src.numel()], dtype=i32), drop_src=drop_src.to(i32))


# ---- the folded LayerNorm form's weight side -------------------------------------------------------------------------------------
def fold_w_ref(W, gamma, beta, bias, at, dtype=torch.float64):
    """(Wf, cs, cs_unrounded, bf): Wf = at(gamma W) (the fp32 product, one rounding), cs[n] = sum_k Wf[n, k] (the ROUNDED weights, what the
    matrix cores contract), cs_unrounded[n] = sum_k gamma[k] W[n, k], bf[n] = bias[n] + <W[n], beta>; the sums in ``dtype``."""
    Wf = (W.detach().cpu().float() * gamma.detach().cpu().float()).to(at)
    W, gamma, beta, bias = _cv(W, dtype), _cv(gamma, dtype), _cv(beta, dtype), _cv(bias, dtype)
    return Wf, Wf.to(dtype).sum(-1), (W * gamma).sum(-1), bias + (W * beta).sum(-1)


def fold_w_biased_inputs(N, at, g):
    """(W, gamma, beta, bias) on which the two column sums are far apart: every product gamma W sits 0.2 eps(at) (relative) ABOVE a value
    of ``at`` and rounds down to it (half a step is at least eps / 4), all weights positive, so the sum of the rounded weights is below
    the sum of the products by about 0.2 eps(at) * 900.  gamma is a power of two (the fp32 product is then exact)."""
    q = (torch.randn(N, D, generator=g).abs() + 0.5).to(at).float()
    gamma = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (D,), generator=g)]
    W = (q.double() * (1.0 + 0.2 * torch.finfo(at).eps)).float() / gamma
    return W, gamma, 0.2 * torch.randn(D, generator=g), torch.randn(N, generator=g)


# ---- split operand images --------------------------------------------------------------------------------------------------------
def split3_image_ref(v, at=torch.float16):
    """(hi, lo) of store4_split3 (csrc/dyt_common.h) for fp32 values v: hi = at(v), lo = at(v - hi) (the difference is exact in fp32)."""
    v = v.detach().cpu().float()
    hi = v.to(at)
    return hi, (v - hi.float()).to(at)


def e4m3_decode(b):
    """float64 values of e4m3 (OCP "fn": bias 7, no infinity, 0x7f / 0xff = NaN) bytes (uint8 tensor)."""
    b = b.detach().cpu().to(torch.int64)
    s, e, m = b >> 7, (b >> 3) & 15, b & 7
    val = torch.where(e == 0, m.double() * 2.0 ** -9, (1.0 + m.double() / 8.0) * torch.pow(torch.tensor(2.0, dtype=torch.float64), (e - 7).double()))
    val = torch.where((e == 15) & (m == 7), torch.full_like(val, float("nan")), val)
    return torch.where(s == 1, -val, val)


def f8_image_parts(img):
    """An [rows, 2 * 768] IEEE-half tensor holding the [hi16 768 | e4m3(hi) 768 bytes | e4m3(lo 2^12) 768 bytes] image of store4_split_f8 ->
    (hi16 [rows, 768] half, hi8 bytes [rows, 768] uint8, lo8 bytes [rows, 768] uint8)."""
    img = img.detach().cpu().contiguous()
    assert img.dtype == torch.float16 and img.dim() == 2 and img.shape[1] == 2 * D
    raw = img.view(torch.uint8)
    return img[:, :D], raw[:, 2 * D:3 * D], raw[:, 3 * D:4 * D]


def f8_sources_ref(v):
    """(hi16, source of the hi byte, source of the lo byte) for fp32 values v: hi16 = half(v); the bytes are e4m3 of hi16 and of
    (v - hi16) 2^12 (exact in fp32), each clamped to +-448 first."""
    v = v.detach().cpu().float()
    hi = v.to(torch.float16)
    lo = (v - hi.float()) * F8_LO_SCALE
    return hi, hi.double().clamp(-448.0, 448.0), lo.double().clamp(-448.0, 448.0)


def e4m3_half_step(src):
    """Half an e4m3 step at the (clamped) source value: 2^-4 |s| for normal values (|s| >= 2^-6), 2^-10 below -- any round-to-nearest
    lands within it."""
    a = src.abs()
    return torch.where(a >= 2.0 ** -6, a * 2.0 ** -4, torch.full_like(a, 2.0 ** -10))


# ---- embedding prologue ----------------------------------------------------------------------------------------------------------
def im2col_ref(img):
    """[B, 3, 224, 224] -> [B * 196, 768]: row b * 196 + py * 14 + px, column c * 256 + i * 16 + j = img[b, c, py * 16 + i, px * 16 + j]."""
    B = img.shape[0]
    return img.detach().cpu().reshape(B, 3, 14, 16, 14, 16).permute(0, 2, 4, 1, 3, 5).reshape(B * NP, D).contiguous()


def pad_convert_ref(src, dst_rows, dst_cols, transpose, at):
    """dst [dst_rows, dst_cols] = src (or its transpose), zero outside the source, rounded to ``at``."""
    s = src.detach().cpu().float()
    if transpose:
        s = s.t()
    out = torch.zeros(dst_rows, dst_cols, dtype=torch.float32)
    r, c = min(dst_rows, s.shape[0]), min(dst_cols, s.shape[1])
    out[:r, :c] = s[:r, :c]
    return out.to(at)
