"""Plain-torch CPU references of the row kernels that carry the gradient from one block to the next (csrc/block_bwd.hip and csrc/ln.hip: bwd_prep, ln_bwd,
ln_param_grad / ln_param_reduce, tok_bwd with the deferred gate-gradient reduction), for tests/test_gpu_row_bwd.py.

As tests/tail_refs.py: every function takes ``dtype`` -- float64 is the reference, float32 gives the error floor of plain fp32 arithmetic
on the very inputs of a case -- and scalars that cross the C ABI as ``float`` are widened from their float32 value.  Each function states
the operation (csrc/kernels.h: BwdPrepArgs, launch_ln_bwd, launch_ln_param_grad, TokBwdArgs), not the kernel's loop order.  16-bit
operands are passed in as the tensors the kernel read (their upcast is exact); ``gs`` is the factor those gradient operands carry, and it
is divided out here.  tests/test_rowbwd_refs_host.py pins these functions to torch autograd."""
import torch

from tail_refs import f32

NT, NP, D = 197, 196, 768


def _cv(x, dtype):
    return None if x is None else x.detach().to("cpu", dtype)


def _rows(idx):
    return None if idx is None else idx.detach().to("cpu", torch.int64)


def ln_bwd_ref(dy, x, mean, rstd, w, dtype=torch.float64):
    """LayerNorm input gradient with the GIVEN statistics: xh = (x - mean) rstd, t = dy w, dx = rstd (t - mean(t) - xh mean(t xh)).
    dy, x [rows, 768]; mean, rstd [rows]; w [768]."""
    dy, x, w = _cv(dy, dtype), _cv(x, dtype), _cv(w, dtype)
    mean, rstd = _cv(mean, dtype).view(-1, 1), _cv(rstd, dtype).view(-1, 1)
    xh = (x - mean) * rstd
    t = dy * w
    return rstd * (t - t.mean(-1, keepdim=True) - xh * (t * xh).mean(-1, keepdim=True))


def ln_param_grad_ref(dy, x, mean, rstd, gs=1.0, dtype=torch.float64):
    """[1536]: d gamma = sum_t (dy[t] / gs) xh[t], then d beta = sum_t dy[t] / gs."""
    dy, x = _cv(dy, dtype) / f32(gs), _cv(x, dtype)
    xh = (x - _cv(mean, dtype).view(-1, 1)) * _cv(rstd, dtype).view(-1, 1)
    return torch.cat([(dy * xh).sum(0), dy.sum(0)])


def bwd_prep_ref(g, h=None, dst_of=None, row_mask=None, dtype=torch.float64):
    """(rows, dmask): rows[t] = row_mask[t] g[t] (what goes to dH[dst_of[t]], before the factor gs and the rounding to the operand type;
    g itself goes to g_at), dmask[t] = <g[t], h[dst_of[t]]> for dst_of[t] >= 0, else 0 (dst_of None: the identity; h None: all 0)."""
    g = _cv(g, dtype)
    M = g.shape[0]
    r = _rows(dst_of) if dst_of is not None else torch.arange(M)
    rows = g if row_mask is None else g * _cv(row_mask, dtype).view(-1, 1)
    dmask = torch.zeros(M, dtype=dtype)
    if h is not None:
        kept = r >= 0
        dmask[kept] = (g[kept] * _cv(h, dtype)[r[kept]]).sum(-1)
    return rows, dmask


def ln_bwd_kernel_ref(dy, x, mean, rstd, w, base=None, base_at=None, gs=1.0, h_next=None, dst_of_next=None, dtype=torch.float64):
    """(d, dmask_next): d = LNbwd(dy / gs) + (base | base_at / gs | 0); dmask_next[row] = <d[row], h_next[dst_of_next[row]]> where that
    index is >= 0 (None: the identity), else 0 -- the product of d itself, not of a rounded copy."""
    gs = f32(gs)
    d = ln_bwd_ref(_cv(dy, dtype) / gs, x, mean, rstd, w, dtype)
    if base_at is not None:
        d = d + _cv(base_at, dtype) / gs
    elif base is not None:
        d = d + _cv(base, dtype)
    _, dmask = bwd_prep_ref(d, h_next, dst_of_next, None, dtype)
    return d, dmask


def tok_bwd_ref(M, u, du=None, du_in_at=None, g_cls=None, dad=None, dA2=None, dst_of=None, mean2=None, rstd2=None, ln2_w=None,
                gate_w=None, soft=None, maskf=None, dmask=None, dtoken_select=None, dtoken_logits=None, dtok=None, training=0, tau=1.0,
                gs=1.0, cat_dact=None, cat_ddz=None, cat_ddz_scale=0.0, cat_ddz_dscale=None, branch_scale=None, dtype=torch.float64):
    """The per-token tail of a block's backward (TokBwdArgs), for M = 197 B tokens t = 197 b + n.  Returns (du', d_gate [769], dlogit [M]).

      du'    = incoming + dad / gs + branch_scale[b] LNbwd(dA2[r] / gs; u[t], stats2[t], ln2_w) [r >= 0] + dlogit[t] gate_w [n >= 1]
      incoming = g_cls given: g_cls[b] on the cls row, 0 on the patch rows; else du_in_at / gs if given; else du; all None: 0
      r      = g_cls given: b on the cls row, none elsewhere (dA2 is [B, 768]); else dst_of[t] (None: t)
      dlogit = (branch_scale[b] (dmask[t] - [maskf[t] != 0] <cat_dact[t], cat_ddz[t]> cat_ddz_scale cat_ddz_dscale) + ext[t])
               soft[t] (1 - soft[t]) (/ tau if training) + dtoken_logits[b, n - 1]           (0 on cls rows and without gate_w;
               the cat term only with dmask given)
      ext    = dtoken_select[b, n - 1] if given, else dtok[0] + (dtok[2] if maskf[t] != 0 else dtok[1]) if dtok given, else 0
      d_gate = (sum_t dlogit[t] u[t], sum_t dlogit[t])
    dtoken_select / dtoken_logits: [B, 196] (the layer's own slice)."""
    gs, tau, cat_ddz_scale = f32(gs), f32(tau), f32(cat_ddz_scale)
    B = M // NT
    assert M == B * NT
    u = _cv(u, dtype)
    n_of = torch.arange(M) % NT
    b_of = torch.arange(M) // NT
    cls = n_of == 0
    out = torch.zeros(M, D, dtype=dtype)
    if g_cls is not None:
        out[cls] = _cv(g_cls, dtype)
    elif du_in_at is not None:
        out = _cv(du_in_at, dtype) / gs
    elif du is not None:
        out = _cv(du, dtype).clone()
    if dad is not None:
        out = out + _cv(dad, dtype) / gs
    bs = torch.ones(M, dtype=dtype) if branch_scale is None else _cv(branch_scale, dtype)[b_of]
    if dA2 is not None:
        if g_cls is not None:
            r = torch.where(cls, b_of, torch.full((M,), -1, dtype=torch.int64))
        else:
            r = _rows(dst_of) if dst_of is not None else torch.arange(M)
        kept = r >= 0
        ln = ln_bwd_ref(_cv(dA2, dtype)[r[kept]] / gs, u[kept], _cv(mean2, dtype)[kept], _cv(rstd2, dtype)[kept], ln2_w, dtype)
        out[kept] = out[kept] + ln * bs[kept].view(-1, 1)
    dlogit = torch.zeros(M, dtype=dtype)
    d_gate = torch.zeros(D + 1, dtype=dtype)
    if gate_w is not None:
        gate_w, s = _cv(gate_w, dtype), _cv(soft, dtype)
        kept_f = None if maskf is None else (_cv(maskf, dtype) != 0)
        dmk = torch.zeros(M, dtype=dtype) if dmask is None else _cv(dmask, dtype).clone()
        if cat_dact is not None and dmask is not None:
            czs = cat_ddz_scale * (1.0 if cat_ddz_dscale is None else _cv(cat_ddz_dscale, dtype).reshape(()))
            corr = (_cv(cat_dact, dtype) * _cv(cat_ddz, dtype)).sum(-1) * czs
            dmk = dmk - torch.where(kept_f, corr, torch.zeros_like(corr))
        dmk = dmk * bs
        ext = torch.zeros(M, dtype=dtype)

        def per_token(t):   # [B, 196] -> [M] (0 on the cls rows)
            return torch.cat([torch.zeros(B, 1, dtype=dtype), _cv(t, dtype).reshape(B, NP)], 1).reshape(M)
        if dtoken_select is not None:
            ext = per_token(dtoken_select)
        elif dtok is not None:
            dt = _cv(dtok, dtype)
            ext = dt[0] + torch.where(kept_f, dt[2], dt[1])
        dlogit = (dmk + ext) * s * (1.0 - s)
        if training:
            dlogit = dlogit / tau
        if dtoken_logits is not None:
            dlogit = dlogit + per_token(dtoken_logits)
        dlogit = torch.where(cls, torch.zeros_like(dlogit), dlogit)
        out = out + dlogit.view(-1, 1) * gate_w
        d_gate = torch.cat([(dlogit.view(-1, 1) * u).sum(0), dlogit.sum().view(1)])
    return out, d_gate, dlogit


def split3_value(img, scale, hi_only=False):
    """The fp32 values an [rows, 2 * 768] hi | lo split operand image (store4_split3, csrc/dyt_common.h: hi = rn16(v), lo = rn16(v - hi),
    the lo plane 768 elements behind the hi plane of the same row) stands for, divided by ``scale``; hi_only: the hi plane alone."""
    img = img.detach().to("cpu", torch.float64)
    assert img.dim() == 2 and img.shape[1] == 2 * D
    v = img[:, :D] if hi_only else img[:, :D] + img[:, D:]
    return v / f32(scale)
