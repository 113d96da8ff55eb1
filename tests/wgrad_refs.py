"""Plain-torch CPU references of the adapter weight-gradient products and the partial reductions (csrc/wgrad.hip: wgrad_bf16_kernel,
wgrad_f32_kernel, wgrad_reduce_kernel / wgrad_reduce_batch_kernel, reduce_partials_kernel / reduce_partials_batch_kernel), for
tests/test_gpu_unit_wgrad.py.

As tests/rowbwd_refs.py: every function takes ``dtype`` -- float64 is the reference, float32 gives the error floor of plain fp32 arithmetic
on the very inputs of a case -- and scalars that cross the C ABI as ``float`` are widened from their float32 value.  The functions state the
operation (csrc/kernels.h: WgradArgs, launch_reduce_partials), not the kernels' loop order; ``geometry`` and ``chain`` restate what
launch_wgrad and the kernels do with the token dimension, for the shapes and the per-element allowance of the GPU test.
tests/test_wgrad_refs_host.py pins ``wgrad`` to torch autograd of the two nn.Linear layers it serves."""
import numpy as np
import torch

D, RP = 768, 64
WG_ROWS, WG_J = D + 8, 80    # one chunk of `partial`: [776][80] floats
WG_CHUNK = 512
MAX_WG, MAX_TOK = 32, 16     # ReduceQueue (csrc/kernels.h)


def _f32(x):
    return float(np.float32(x))


def geometry(M):
    """(chunk, nchunks) of launch_wgrad: tokens per workgroup and workgroups along the token dimension.  768 / 128 = 6 channel blocks, so
    256 / 6 = 42 chunks fill the 256 CUs once: chunk = ceil(M / 42) rounded up to 64 tokens, at least 512."""
    cblocks = D // 128
    per = 256 // cblocks
    want = (M + per - 1) // per
    chunk = max(WG_CHUNK, (want + 63) // 64 * 64)
    return chunk, (M + chunk - 1) // chunk


def scratch_floats(M):
    """dyt_wgrad_scratch_floats restated: one [776][80] block per 512 tokens (chunk >= 512, so nchunks never exceeds it)."""
    return (M + 511) // 512 * WG_ROWS * WG_J


def chain(M, kernel):
    """The longest chain of fp32 roundings one output of a product launch passes through, counted from csrc/wgrad.hip.  kernel: "bf16"
    (wgrad_bf16_kernel, every instantiation) or "f32" (wgrad_f32_kernel).

    wgrad_bf16_kernel: a workgroup walks its chunk in steps of TS = 64 tokens; per step and 32-column block the kk loop issues 4 MFMA 32x32x16,
    each contracting 16 tokens (8 per half-wave) into the same accumulator: chunk / 16 accumulations per chunk (chunk is a multiple of 64;
    tokens beyond M are zeros).  The products of two 16-bit operands are exact in fp32.  A term passes through at most 16 additions inside
    the MFMA that takes it in (the order in there is the hardware's: counted as the worst, a sequential sum of its 16 terms) and then through
    one addition per later MFMA: 16 + chunk / 16.  The column sums stay below that: sum8 is at most 8 additions, then one `xs +=` per kk
    (chunk / 16) and one __shfl_xor addition.
    wgrad_f32_kernel: a wave takes every 4th token pair of the chunk: chunk / 8 MFMA 32x32x2 per accumulator, each with two fp32 products that
    are rounded (1) and two additions (2); the four waves are summed through LDS in wave order (3 additions).  The column sums: chunk / 8
    additions per lane, the same 3 wave sums and one __shfl_xor addition -- below 3 + chunk / 8 + 3 as well.
    Both: wgrad_reduce_kernel / wgrad_reduce_batch_kernel add the nchunks partials in order (nchunks), form alpha * alpha_dev (1), multiply
    (1) and add into the output (1)."""
    chunk, nchunks = geometry(M)
    if kernel == "bf16":
        return 16 + chunk // 16 + nchunks + 3
    assert kernel == "f32", kernel
    return 3 + chunk // 8 + 3 + nchunks + 3


def _assert_normal(t, dt, what):
    """Every non-zero value of the 16-bit tensor t is normal and finite in its type."""
    a = t.double().abs()
    a = a[a != 0]
    fi = torch.finfo(dt)
    assert bool(torch.isfinite(t.double()).all()) and (a.numel() == 0 or (float(a.max()) <= fi.max and float(a.min()) >= fi.tiny)), \
        "%s: scaled operand spans [%.3e, %.3e], outside the normal range of %s: choose other inputs or scales" % (
            what, float(a.min()) if a.numel() else 0.0, float(a.max()) if a.numel() else 0.0, dt)


def operands(X, Y, x_scale=1.0, y_scale=1.0, half_dtype=None):
    """The values the matrix cores see, as float64 CPU tensors.  16-bit and fp32 inputs upcast exactly; with half_dtype (the half_products
    form) the fp32 inputs are multiplied by their scales in fp32 and rounded to that type (round to nearest even, the cast of wg_load8)."""
    X, Y = X.detach().to("cpu"), Y.detach().to("cpu")
    if half_dtype is not None:
        assert X.dtype == torch.float32 and Y.dtype == torch.float32
        X = (X * torch.tensor(_f32(x_scale), dtype=torch.float32)).to(half_dtype)
        Y = (Y * torch.tensor(_f32(y_scale), dtype=torch.float32)).to(half_dtype)
        _assert_normal(X, half_dtype, "X * x_scale")
        _assert_normal(Y, half_dtype, "Y * y_scale")
    else:
        for t, what in ((X, "X"), (Y, "Y")):
            if t.dtype in (torch.float16, torch.bfloat16):
                _assert_normal(t, t.dtype, what)
    return X.double(), Y.double()


def wgrad(X, Y, r, sc, sj, alpha, alpha_x, alpha_y, alpha_dev=None, x_scale=1.0, y_scale=1.0, half_dtype=None, dtype=torch.float64,
          absolute=False):
    """The three increments of one product (WgradArgs): (w, xsum, ysum) with
        w[c * sc + j * sj] = alpha a sum_m X[m][c] Y[m][j]   (flat [768 * r]; c < 768, j < r),
        xsum[c] = alpha_x a sum_m X[m][c]   [768],      ysum[j] = alpha_y a sum_m Y[m][j]   [r],
    a = alpha_dev (the value of the device word) or 1.  X [M, 768], Y [M, 64]: columns j >= r of Y take no part.  With half_dtype the operands
    are those of ``operands`` and the alphas are divided by the scales in fp32, as launch_wgrad divides them.
    absolute: the same sums over |X|, |Y| with |alpha|: sum_m |alpha a X Y|, what the per-element allowance is a multiple of."""
    Xo, Yo = operands(X, Y, x_scale, y_scale, half_dtype)
    al, ax, ay = np.float32(alpha), np.float32(alpha_x), np.float32(alpha_y)
    if half_dtype is not None:
        xs, ys = np.float32(x_scale), np.float32(y_scale)
        al, ax, ay = al / (xs * ys), ax / xs, ay / ys
    ad = 1.0 if alpha_dev is None else _f32(alpha_dev)
    Xo, Yo = Xo.to(dtype), Yo[:, :r].to(dtype)
    al, ax, ay, ad = (torch.tensor(float(v), dtype=dtype) for v in (al, ax, ay, ad))
    if absolute:
        Xo, Yo, al, ax, ay, ad = Xo.abs(), Yo.abs(), al.abs(), ax.abs(), ay.abs(), ad.abs()
    C = Xo.t() @ Yo                                    # [768, r]
    idx = w_index(r, sc, sj)
    w = torch.zeros(int(idx.max()) + 1, dtype=dtype)
    w[idx] = ((al * ad) * C).reshape(-1)
    return w, (ax * ad) * Xo.sum(0), (ay * ad) * Yo.sum(0)


def w_index(r, sc, sj):
    """[768 * r] flat positions c * sc + j * sj of out_w, (c, j) row-major; the strides must not send two (c, j) to one cell.
    The increment ``wgrad`` returns is flat [max position + 1], zero in the cells no (c, j) names."""
    idx = (torch.arange(D).view(-1, 1) * sc + torch.arange(r).view(1, -1) * sj).reshape(-1)
    assert int(idx.min()) >= 0 and idx.unique().numel() == D * r, "strides (%d, %d) send two of the [768, %d] products to one cell" % (sc, sj, r)
    return idx


def reduce_partials(partial, nparts, stride, n, alpha, dtype=torch.float64, absolute=False):
    """[n]: alpha sum_p partial[p * stride + i] of a flat buffer (launch_reduce_partials; stride 0 reads the same n floats nparts times)."""
    flat = partial.detach().to("cpu", dtype).reshape(-1)
    idx = torch.arange(nparts).view(-1, 1) * stride + torch.arange(n).view(1, -1)
    v = flat[idx]
    a = torch.tensor(_f32(alpha), dtype=dtype)
    if absolute:
        v, a = v.abs(), a.abs()
    return a * v.sum(0)
