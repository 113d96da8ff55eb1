"""CPU tests of tests/wgrad_refs.py, the references tests/test_gpu_unit_wgrad.py holds csrc/wgrad.hip to: ``wgrad`` against torch autograd of
the two nn.Linear layers of the adapter (models/dynamic_adapter.py: down_proj, ReLU, up_proj, times scale), ``reduce_partials`` against a
plain sum, the scratch formula against the launch geometry for every token count, and the rounding of the half-product form."""
import pytest
import torch

import wgrad_refs as R

F64 = torch.float64
D, RP = R.D, R.RP


@pytest.mark.parametrize("M,r", [(1, 1), (5, 8), (37, 40), (130, 64)])
def test_wgrad_is_the_parameter_gradient_of_the_adapters_linear_layers(M, r):
    g = torch.Generator().manual_seed(1000 * M + r)
    scale = 0.1
    down = torch.nn.Linear(D, r).double()
    up = torch.nn.Linear(r, D).double()
    with torch.no_grad():
        up.weight.copy_(torch.randn(D, r, generator=g, dtype=F64) * 0.05)
    u = torch.randn(M, D, generator=g, dtype=F64)
    G = torch.randn(M, D, generator=g, dtype=F64)           # the upstream gradient of the adapter's output
    z = down(u)
    z.retain_grad()
    act = torch.relu(z)
    out = up(act) * scale
    (out * G).sum().backward()
    pad = torch.randn(M, RP - r, generator=g, dtype=F64)    # columns r .. 63 of Y take no part
    d_act = torch.cat([act.detach(), pad], 1)
    ddz = torch.cat([z.grad, pad], 1)

    # up_proj: X = g, Y = d_act, out_w [768, r] (sc = r, sj = 1), bias = xsum, all times scale
    w, xsum, ysum = R.wgrad(G, d_act, r, r, 1, scale, scale, 0.0)
    sf = float(torch.tensor(scale, dtype=torch.float32)) / scale   # the reference widens the float32 value of `scale`
    tol = lambda t: 1e-12 * max(1.0, float(t.abs().max()))
    assert float((w.view(D, r) - up.weight.grad * sf).abs().max()) <= tol(up.weight.grad)
    assert float((xsum - up.bias.grad * sf).abs().max()) <= tol(up.bias.grad)
    assert float(ysum.abs().max()) == 0.0

    # down_proj: X = u, Y = ddz, out_w [r, 768] (sc = 1, sj = 768), bias = ysum
    w, xsum, ysum = R.wgrad(u, ddz, r, 1, D, 1.0, 0.0, 1.0)
    assert float((w.view(r, D) - down.weight.grad).abs().max()) <= tol(down.weight.grad)
    assert float((ysum - down.bias.grad).abs().max()) <= tol(down.bias.grad)
    assert float(xsum.abs().max()) == 0.0

    # the device word multiplies all three; `absolute` bounds every increment
    w2, x2, y2 = R.wgrad(u, ddz, r, 1, D, 0.75, 0.5, -0.25, alpha_dev=2.0 ** -5)
    assert float((w2 - 0.75 * 2.0 ** -5 * w).abs().max()) <= tol(w) and float((y2 + 0.25 * 2.0 ** -5 * ysum).abs().max()) <= tol(ysum)
    assert float((x2 - 0.5 * 2.0 ** -5 * u.sum(0)).abs().max()) <= tol(u.sum(0))
    wa, xa, ya = R.wgrad(u, ddz, r, 1, D, 0.75, 0.5, -0.25, alpha_dev=2.0 ** -5, absolute=True)
    assert bool((wa >= w2.abs() - 1e-15).all()) and bool((xa >= x2.abs() - 1e-15).all()) and bool((ya >= y2.abs() - 1e-15).all())


@pytest.mark.parametrize("hd,xs", [(torch.float16, 2.0 ** 14), (torch.bfloat16, 2.0 ** 14)])
def test_half_product_form_rounds_the_scaled_operands_and_divides_the_alphas(hd, xs):
    g = torch.Generator().manual_seed(7)
    M, r = 33, 8
    X = torch.randn(M, D, generator=g) * 1e-6
    X = torch.where(X.abs() < 2e-7, torch.full_like(X, 2e-7), X)
    Y = torch.randn(M, RP, generator=g)
    Y = torch.where(Y.abs() < 1e-2, torch.zeros_like(Y), Y)     # exact zeros are allowed
    w, xsum, ysum = R.wgrad(X, Y, r, r, 1, 0.3, 0.2, 0.1, x_scale=xs, y_scale=1.0, half_dtype=hd)
    Xh, Yh = (X * xs).to(hd).double(), Y.to(hd).double()
    a = lambda v: float(torch.tensor(v, dtype=torch.float32))
    assert float((w.view(D, r) - a(0.3) / xs * (Xh.t() @ Yh[:, :r])).abs().max()) <= 1e-12 * float(w.abs().max())
    assert float((xsum - a(0.2) / xs * Xh.sum(0)).abs().max()) <= 1e-12 * float(xsum.abs().max())
    assert float((ysum - a(0.1) * Yh[:, :r].sum(0)).abs().max()) <= 1e-12 * float(ysum.abs().max())
    # the rounding is visible: the unrounded product differs by about eps(half) / 2
    w0, _, _ = R.wgrad(X.double(), Y.double(), r, r, 1, 0.3, 0.2, 0.1)
    assert float((w - w0).abs().max()) > 1e-6 * float(w0.abs().max())
    # gradient-sized X without a scale is subnormal in IEEE half: refused by the reference
    if hd == torch.float16:
        with pytest.raises(AssertionError, match="normal range"):
            R.wgrad(X, Y, r, r, 1, 0.3, 0.2, 0.1, x_scale=1.0, y_scale=1.0, half_dtype=hd)


def test_colliding_strides_are_refused_and_gaps_stay_zero():
    X, Y = torch.ones(2, D), torch.ones(2, RP)
    with pytest.raises(AssertionError, match="to one cell"):
        R.wgrad(X, Y, 8, 1, 1, 1.0, 1.0, 1.0)
    w, _, _ = R.wgrad(X, Y, 8, RP, 1, 1.0, 1.0, 1.0)          # [768, 64] rows with 8 columns used
    assert w.numel() == 767 * RP + 8 and bool((w.view(-1)[:RP] == torch.tensor([2.0] * 8 + [0.0] * 56, dtype=F64)).all())


@pytest.mark.parametrize("nparts,n,stride", [(1, 5, 5), (9, 33, 33), (4, 7, 11), (1, 12, 0), (3, 12, 0)])
def test_reduce_partials_is_alpha_times_the_column_sum(nparts, n, stride):
    g = torch.Generator().manual_seed(nparts * 100 + n)
    buf = torch.randn(max(1, (nparts - 1) * stride + n) + 3, generator=g, dtype=F64)
    got = R.reduce_partials(buf, nparts, stride, n, 0.25)
    if stride == 0:
        want = 0.25 * nparts * buf[:n]
    else:
        want = 0.25 * torch.stack([buf[p * stride:p * stride + n] for p in range(nparts)]).sum(0)
    assert float((got - want).abs().max()) <= 1e-12
    assert bool((R.reduce_partials(buf, nparts, stride, n, -0.25, absolute=True) >= got.abs() - 1e-15).all())


def test_scratch_formula_holds_every_chunk_of_every_token_count():
    for M in range(1, 30001):
        chunk, nchunks = R.geometry(M)
        assert chunk >= 512 and chunk % 64 == 0 and (nchunks - 1) * chunk < M <= nchunks * chunk, M
        assert nchunks * R.WG_ROWS * R.WG_J <= R.scratch_floats(M), M
    assert R.geometry(512) == (512, 1) and R.geometry(513) == (512, 2) and R.geometry(1025) == (512, 3)
    assert R.geometry(21504) == (512, 42) and R.geometry(21505) == (576, 38) and 21505 - 37 * 576 == 193
    assert R.geometry(25216) == (640, 40)   # B = 128: the 6 x 40 grid csrc/wgrad.hip names


def test_chain_counts():
    assert R.chain(1, "bf16") == 16 + 32 + 1 + 3 and R.chain(1, "f32") == 3 + 64 + 3 + 1 + 3
    assert R.chain(21505, "bf16") == 16 + 36 + 38 + 3 and R.chain(21505, "f32") == 3 + 72 + 3 + 38 + 3
