"""Unit tests of csrc/wgrad.hip -- the adapter weight-gradient products and every deferred reduction of a backward pass -- through
dyt_unit_wgrad / dyt_unit_reduce_partials (include/dyt_hip.h), next to the fp64 references of tests/wgrad_refs.py (pinned to torch autograd
by tests/test_wgrad_refs_host.py).  DESIGN.md 7y holds the derivations.

  wgrad_f32_kernel                        mode "fp32"
  wgrad_bf16_kernel<16-bit operand>       modes "bf16" (libdyt_hip.so), "fp16" (libdyt_hip_f16.so), precision 1
  wgrad_bf16_kernel<float>                modes "fp32+hp" (libdyt_hip.so: bf16 conversion) and "fp32h+hp" (libdyt_hip_f16.so: IEEE-half conversion,
                                          the form "fp16x3f" runs): precision 0 with half_products
  wgrad_reduce_kernel                     defer = 0             wgrad_reduce_batch_kernel      defer = 1 (ReduceQueue + flush_reductions)
  reduce_partials_batch_kernel            the token reductions of a queue (blockIdx.y > 0 included)
  reduce_partials_kernel                  dyt_unit_reduce_partials

The rule.  Every fp32 output tensor is held to ``_cmp`` of tests/test_gpu_step_tail.py, imported unchanged: the reference evaluated in fp64
and in fp32 on the CPU from the very values the kernel read (16-bit inputs upcast exactly, half_products inputs scaled and rounded by the
reference), max|gpu - fp64| <= 4 max|fp32_cpu - fp64| + 4 ulp(max|fp64|).  Every element is also held to its own allowance
chain * 2^-24 * sum_m |alpha a X Y| + 2 ulp(out) (wgrad_refs.chain: the roundings one output passes through, counted from the code; the
sum is the fp64 abs-product of the reference), so that a small entry beside a large one is not hidden by the max norm.  The same for the
reductions with chain = ceil(nparts / 8) + 8 + 2 (the group loop, the 8 group sums, the factor and the +=).
Buffers: `partial` starts as NaN with sentinel floats behind dyt_wgrad_scratch_floats(M): finite outputs show that the reduce reads no cell
the product kernel does not write (pad rows 769..775, columns 65..79, [768][64]); the sentinel and every cell at or beyond
nchunks * 776 * 80 keep their bits.  Outputs are += : they start from known non-zero values; out_w rows / columns at or beyond r and the
floats behind every output hold a sentinel and keep it; Y[:, r:] holds non-zero values (and a case of its own shows them without effect).
Named exactness properties are torch.equal on bits.

Every case prints error / floor and its worst share of the allowance; the module prints the worst per kernel and its wall time at its end.
Records of one MI355X run (not bounds; all 189 tests pass, 9 s of which 6 s are the CPU references at M = 21505):

  kernel                                  worst error / floor                              worst share of the allowance
  wgrad_f32                               3.79 (M=513 r=1 [r,768] out_ysum: one element)   0.242 (M=1)
  wgrad_bf16<bf16> / <f16>                2.21 (M=513 r=64 [r,768] out_w) / 1.22           0.248 / 0.245 (M=1)
  wgrad_bf16<float> bf16 / IEEE half      2.14 (M=513 r=63 sc=64 out_w) / 1.06             0.247 / 0.240 (M=1)
  reduce_partials_batch                   1.25 (nparts=15, full queue)                     0.235 (nparts=1)
  reduce_partials                         3.09 (nparts=64 n=1: one element)                0.244 (nparts=1)

Each of these value edits of csrc/wgrad.hip turns the named tests red (checked once on the MI355X, separate builds, none kept):
`col = j < r ? j : 63` in wgrad_reduce_kernel -- the 125 cases that hold an immediate out_xsum to a reference or compare the two reduce
kernels' bits; o.nchunks -> b.e[0].nchunks in wgrad_reduce_batch_kernel -- test_queue_of_products_with_their_own_chunk_counts[*] alone;
`ad` dropped from the out_ysum line of wgrad_reduce_kernel -- the 119 cases with a device word and an out_ysum; the
`xs += __shfl_xor(xs, 32, 64)` line of wgrad_bf16_kernel dropped -- the 85 cases of its four modes with an out_xsum and M > 8;
`alpha / (xs * ys)` without ys -- test_half_products_mirror_image[*] and the half-product modes of
test_production_pair_immediate_and_deferred.
Found on the way: launch_wgrad enqueued the product kernel before it refused mixed ranks in a queue; the check now stands in front of the
launch (test_bad_arguments_are_refused_and_the_library_stays_usable holds the refused product's `partial` to its bits).

Not reachable from here: the kernels next to a concurrently running stream; the launcher's dbg_skip and DYT_DBG_WGRAD_LDS hooks; "reduce queue
full" (the entry's own n_prod / n_tok limits are the queue's)."""
import ctypes
import math
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _lib  # noqa: E402
import wgrad_refs as R  # noqa: E402
from _lib import ptr, stream_ptr  # noqa: E402
from test_gpu_row_bwd import SENT, _dev, _mode  # noqa: E402
from test_gpu_step_tail import WORST, _cmp  # noqa: E402   (the project's comparison rule, unchanged)

DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
D, RP = R.D, R.RP
ERR_ARG = -1      # DYT_ERR_ARG, and what launch_wgrad returns for a refused call
TAIL = 64         # sentinel floats behind every buffer
U = 2.0 ** -24    # unit roundoff of fp32
WORST_A = {}      # kernel -> (worst share of the allowance, case)
T0 = time.time()

# name -> (mode of test_gpu_row_bwd._mode, half_products, the 16-bit type the fp32 inputs are converted to, chain's kernel, name in the tables)
MODE = {
    "fp32": ("fp32", 0, None, "f32", "wgrad_f32"),
    "bf16": ("bf16", 0, None, "bf16", "wgrad_bf16<bf16>"),
    "fp16": ("fp16", 0, None, "bf16", "wgrad_bf16<f16>"),
    "fp32+hp": ("fp32", 1, torch.bfloat16, "bf16", "wgrad_bf16<float> bf16"),
    "fp32h+hp": ("fp32h", 1, torch.float16, "bf16", "wgrad_bf16<float> f16"),
}
MODES = list(MODE)
HP_SCALE = 2.0 ** 14   # brings 1e-6-sized operands (>= 5e-8, below) into IEEE half's normal range with a factor 8 to spare


@pytest.fixture(scope="module", autouse=True)
def _worst_table():
    yield
    print("\nworst error / floor per kernel (_cmp) and worst share of the per-element allowance:")
    for k in sorted(set(WORST_A)):
        a = "%8.2f   (%s)" % WORST[k] if k in WORST else "       -"
        print("  %-26s %s\n  %-26s %6.3f   (%s)" % (k, a, "", WORST_A[k][0], WORST_A[k][1]))
    print("tests/test_gpu_unit_wgrad.py: %.1f s wall" % (time.time() - T0))


def _gen(*key):
    return torch.Generator().manual_seed(abs(hash(tuple(int(k) for k in key))) % (2 ** 31))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same_bits(a, b, what):
    n = int((_bits(a) != _bits(b)).sum())
    assert n == 0, "%s: %d elements differ" % (what, n)


def _draw(g, shape, mag, zeros=0.0):
    """mag * N(0, 1) with |.| >= 0.05 mag (nothing near the subnormals of a 16-bit type), a fraction `zeros` set to exact 0 (ReLU-like)."""
    z = torch.randn(*shape, generator=g)
    v = torch.sign(z) * z.abs().clamp_min(0.05) * mag
    if zeros > 0:
        v = torch.where(torch.rand(*shape, generator=g) < zeros, torch.zeros_like(v), v)
    return v


def _pow2_below(x):
    return 2.0 ** math.floor(math.log2(x)) if x > 0 else 2.0 ** -6


def _start(n, mag):
    """Known non-zero starting values of a += output: +-mag * {1 .. 5}, mag a power of two (exact in fp32)."""
    i = torch.arange(n)
    return ((1 + i % 5).float() * (1 - 2 * (i % 2)).float()) * mag


def _ulp32(t64):
    return torch.from_numpy(np.spacing(t64.abs().numpy().astype(np.float32)).astype(np.float64))


def _held(kernel, what, got, ref64, allow):
    """Every element within its own allowance; prints and records the worst share."""
    got = got.detach().to("cpu", F64)
    s = float(((got - ref64).abs() / allow).max()) if bool(torch.isfinite(got).all()) else math.inf
    print("[%s] %s: worst |gpu - fp64| / allowance %.4f" % (kernel, what, s))
    if s > WORST_A.get(kernel, (-1.0, ""))[0]:
        WORST_A[kernel] = (s, what)
    assert s <= 1.0, "[%s] %s: |gpu - fp64| is %.3f times its derived allowance" % (kernel, what, s)


class Prod:
    """One product of a dyt_unit_wgrad call: inputs as the kernel reads them, caller-owned scratch and outputs, and the checks."""

    def __init__(self, mode, M, r, layout="up", alpha=0.75, alpha_x=-1.5, alpha_y=0.375, alpha_dev=None, xsum=True, ysum=True,
                 x_mag=0.05, y_mag=1.0, x_scale=1.0, y_scale=1.0, seed=0, y_pad=True):
        base, self.hp, self.hd, self.chain_kernel, self.kernel = MODE[mode]
        self.L, self.prec, dt, self.gs = _mode(base)
        self.mode, self.M, self.r, self.layout = mode, M, r, layout
        self.alpha, self.alpha_x, self.alpha_y, self.alpha_dev = alpha, alpha_x, alpha_y, alpha_dev
        self.x_scale, self.y_scale = (x_scale, y_scale) if self.hp else (1.0, 1.0)
        self.sc, self.sj = {"up": (r, 1), "up64": (RP, 1), "down": (1, D)}[layout]
        g = _gen(M, r, seed, len(mode))
        X = _draw(g, (M, D), x_mag)
        Y = _draw(g, (M, RP), y_mag, zeros=0.3)
        if not y_pad:
            Y[:, r:] = 0.0
        self.X, self.Y = X.to(dt), Y.to(dt)                 # what the kernel reads (CPU copies)
        self.Xd, self.Yd = _dev(self.X), _dev(self.Y)
        self.tag = "M=%d r=%d %s %s" % (M, r, layout, mode)
        # scratch: NaN where the launch may write, the sentinel behind dyt_wgrad_scratch_floats(M)
        self.scratch = int(self.L.dyt_wgrad_scratch_floats(M))
        assert self.scratch == R.scratch_floats(M), (self.scratch, R.scratch_floats(M))
        self.chunk, self.nchunks = R.geometry(M)
        self.used = self.nchunks * R.WG_ROWS * R.WG_J
        assert self.used <= self.scratch
        p = torch.full((self.scratch + TAIL,), math.nan)
        p[self.scratch:] = SENT
        self.partial0 = p.to(DEV)
        self.partial = self.partial0.clone()
        # outputs: known non-zero starts in the cells the product names, the sentinel everywhere else
        ad = 1.0 if alpha_dev is None else alpha_dev
        xs, ys = self.x_scale, self.y_scale
        self.idx = R.w_index(r, self.sc, self.sj)
        rows = D * RP if layout != "up" else D * r
        w = torch.full((rows + TAIL,), SENT)
        w[self.idx] = _start(D * r, _pow2_below(abs(alpha * ad) * x_mag * y_mag))
        self.w0 = w.to(DEV)
        x0 = torch.full((D + TAIL,), SENT)
        x0[:D] = _start(D, _pow2_below(abs(alpha_x * ad) * x_mag))
        self.x0 = x0.to(DEV) if xsum else None
        y0 = torch.full((RP + TAIL,), SENT)
        y0[:r] = _start(r, _pow2_below(abs(alpha_y * ad) * y_mag))
        self.y0 = y0.to(DEV) if ysum else None
        self.adev = None if alpha_dev is None else torch.tensor([alpha_dev], dtype=F32, device=DEV)
        self.reset()

    def reset(self):
        self.partial.copy_(self.partial0)
        self.w = self.w0.clone()
        self.xs = None if self.x0 is None else self.x0.clone()
        self.ys = None if self.y0 is None else self.y0.clone()

    def args(self):
        a = _lib.UnitWgradArgs()
        a.X, a.Y, a.M, a.r, a.partial = self.Xd.data_ptr(), self.Yd.data_ptr(), self.M, self.r, self.partial.data_ptr()
        a.out_w, a.sc, a.sj, a.alpha = self.w.data_ptr(), self.sc, self.sj, self.alpha
        a.out_xsum, a.alpha_x = (None if self.xs is None else self.xs.data_ptr()), self.alpha_x
        a.out_ysum, a.alpha_y = (None if self.ys is None else self.ys.data_ptr()), self.alpha_y
        a.half_products, a.x_scale, a.y_scale = self.hp, self.x_scale, self.y_scale
        a.alpha_dev = None if self.adev is None else self.adev.data_ptr()
        return a

    def buffers(self):
        return [t for t in (self.Xd, self.Yd, self.partial, self.w, self.xs, self.ys, self.adev) if t is not None]

    def outputs(self):
        return [t.clone() for t in (self.w, self.xs, self.ys) if t is not None]

    def refs(self):
        if not hasattr(self, "_refs"):
            kw = dict(alpha_dev=self.alpha_dev, x_scale=self.x_scale, y_scale=self.y_scale, half_dtype=self.hd)
            a = (self.X, self.Y, self.r, self.sc, self.sj, self.alpha, self.alpha_x, self.alpha_y)
            self._refs = (R.wgrad(*a, **kw), R.wgrad(*a, dtype=F32, **kw), R.wgrad(*a, absolute=True, **kw))
        return self._refs

    def check(self, note=""):
        """The three outputs against the references (rule of the module docstring), and every cell the call must not write."""
        torch.cuda.synchronize()
        assert (self.chunk, self.nchunks) == R.geometry(self.M)
        i64, i32, iabs = self.refs()
        ch = R.chain(self.M, self.chain_kernel)
        tag = self.tag + note
        named = [("out_w", self.w, self.w0, self.idx, 0), ("out_xsum", self.xs, self.x0, torch.arange(D), 1), ("out_ysum", self.ys, self.y0, torch.arange(self.r), 2)]
        for name, out, start, idx, k in named:
            if out is None:
                continue
            got, st = out.cpu(), start.cpu()
            r64 = st[idx].double() + i64[k][idx]
            r32 = st[idx] + i32[k][idx]
            _cmp(self.kernel, "%s %s" % (tag, name), got[idx], r64, r32)
            _held(self.kernel, "%s %s" % (tag, name), got[idx], r64, ch * U * iabs[k][idx] + 2.0 * _ulp32(r64))
            keep = torch.ones(got.numel(), dtype=torch.bool)
            keep[idx] = False
            assert bool((got[keep] == SENT).all()), "%s %s: a cell outside the product's [768, r] was written" % (tag, name)
        pb, p0 = _bits(self.partial[self.used:]), _bits(self.partial0[self.used:])
        assert torch.equal(pb, p0), "%s: `partial` written at or beyond nchunks * 776 * 80 = %d (of %d + sentinel)" % (tag, self.used, self.scratch)


def _call(prods, pair=0, defer=0, toks=(), expect=0):
    L, prec = prods[0].L, prods[0].prec
    arr = (_lib.UnitWgradArgs * len(prods))(*[p.args() for p in prods])
    tarr = (_lib.UnitTokReduceArgs * max(1, len(toks)))()
    for i, t in enumerate(toks):
        tarr[i].partial, tarr[i].nparts, tarr[i].out = t.partial.data_ptr(), t.nparts, t.out.data_ptr()
    rc = L.dyt_unit_wgrad(arr, len(prods), pair, defer, tarr if toks else None, len(toks), prec, stream_ptr())
    assert rc == expect, (rc, L.dyt_last_error())
    torch.cuda.synchronize()


class Tok:
    """One queue_tok_reduce entry: partial [nparts][769], out[769] (+=) with the sentinel behind it."""

    def __init__(self, nparts, seed):
        g = _gen(nparts, seed, 769)
        self.nparts = nparts
        self.p_cpu = torch.randn(nparts, D + 1, generator=g)
        self.partial = _dev(self.p_cpu)
        o = torch.full((D + 1 + TAIL,), SENT)
        o[:D + 1] = _start(D + 1, 0.25)
        self.out0 = o.to(DEV)
        self.out = self.out0.clone()

    def reset(self):
        self.out = self.out0.clone()

    def check(self, note=""):
        _check_reduce("reduce_partials_batch", "nparts=%d%s" % (self.nparts, note), self.out, self.out0, self.p_cpu, self.nparts, D + 1, D + 1, 1.0)


def _check_reduce(kernel, tag, out, out0, p_cpu, nparts, stride, n, alpha):
    torch.cuda.synchronize()
    got, st = out.cpu(), out0.cpu()
    r64 = st[:n].double() + R.reduce_partials(p_cpu, nparts, stride, n, alpha)
    r32 = st[:n] + R.reduce_partials(p_cpu, nparts, stride, n, alpha, dtype=F32)
    _cmp(kernel, tag, got[:n], r64, r32)
    ch = (nparts + 7) // 8 + 8 + 2
    _held(kernel, tag, got[:n], r64, ch * U * R.reduce_partials(p_cpu, nparts, stride, n, alpha, absolute=True) + 2.0 * _ulp32(r64))
    assert bool((got[n:] == SENT).all()), "%s: floats behind out[%d] were written" % (tag, n)


def _two_forms(mode, M, r, seed=0, **kw):
    """The two stride layouts with all three outputs each: [768, r] with distinct alphas and no device word, [r, 768] (rows >= r hold the
    sentinel) scaled by a device word 2^-5.  The half-product modes get gradient-sized X lifted by x_scale."""
    hp = MODE[mode][1]
    m = dict(x_mag=1e-6, x_scale=HP_SCALE) if hp else {}
    m.update(kw)
    return [Prod(mode, M, r, "up", alpha=0.75, alpha_x=-1.5, alpha_y=0.375, seed=seed, **m),
            Prod(mode, M, r, "down", alpha=-0.625, alpha_x=0.4375, alpha_y=1.25, alpha_dev=2.0 ** -5, seed=seed + 1, **m)]


# ------------------------------------------------------------------------------------------------------------------------------
# the products against the references
# ------------------------------------------------------------------------------------------------------------------------------
def test_scratch_formula_is_the_librarys():
    for L in (_lib.lib(), _lib.lib(fp16=True)):
        for M in list(range(1, 2200)) + [21504, 21505, 25216, 30000]:
            assert int(L.dyt_wgrad_scratch_floats(M)) == R.scratch_floats(M), M


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M", [1, 2, 7, 63, 64, 65, 511, 512, 513, 1025])
def test_products_over_the_token_loop(M, mode):
    """r = 40, both layouts, immediate reduce (wgrad_reduce_kernel): one token, one pair, an odd tail of the f32 kernel's 4-waves-by-pairs
    stride, one 64-token step and its neighbours, one chunk and a second chunk of one token, three chunks."""
    prods = _two_forms(mode, M, 40, seed=M)
    want = {1: (512, 1), 512: (512, 1), 513: (512, 2), 1025: (512, 3)}.get(M)
    assert want is None or R.geometry(M) == want
    _call(prods)
    for p in prods:
        p.check()


@pytest.mark.parametrize("mode", MODES)
def test_products_at_the_first_chunk_above_512(mode):
    """M = 21505: chunk 576, 38 chunks, 193 tokens in the last; 5 chunks of `partial` stay untouched."""
    M = 21505
    assert R.geometry(M) == (576, 38) and M - 37 * 576 == 193 and R.scratch_floats(M) == 43 * 776 * 80
    prods = _two_forms(mode, M, 40, seed=3)
    _call(prods, pair=1)
    for p in prods:
        p.check()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M", [65, 513])
@pytest.mark.parametrize("r", [1, 8, 63, 64])
def test_products_over_the_rank(r, M, mode):
    """(r = 40 is the sweep above.)  The [768, 64]-strided layout (sc = 64: columns >= r hold the sentinel) rides along where r < 64."""
    prods = _two_forms(mode, M, r, seed=100 + r)
    if r < RP:
        hp = MODE[mode][1]
        prods.append(Prod(mode, M, r, "up64", alpha=1.25, alpha_x=0.5, alpha_y=-0.75, seed=7, **(dict(x_mag=1e-6, x_scale=HP_SCALE) if hp else {})))
    _call(prods)
    for p in prods:
        p.check()


def _production_pair(mode, M, r, seed=11):
    """The pair csrc/backward.hip builds: up_proj (X = g carrying gs, Y = d_act, [768, r], bias = xsum, scale / gs, no ysum, no word) and
    down_proj (X = u, Y = ddz carrying gs, [r, 768], bias = ysum, 1 / gs, no xsum, the word ddz_unlift); one-part products: a.x_scale =
    b.y_scale = split_gs."""
    hp = MODE[mode][1]
    gs = _mode(MODE[mode][0])[3]
    scale, split_gs = 0.1, 4096.0
    gmag = 1e-6 if hp else 1e-3 * gs
    a = Prod(mode, M, r, "up", alpha=scale / gs, alpha_x=scale / gs, alpha_y=0.0, xsum=True, ysum=False, x_mag=gmag, y_mag=1.0,
             x_scale=split_gs, seed=seed)
    b = Prod(mode, M, r, "down", alpha=1.0 / gs, alpha_x=0.0, alpha_y=1.0 / gs, alpha_dev=2.0 ** -5, xsum=False, ysum=True, x_mag=1.0, y_mag=gmag,
             y_scale=split_gs, seed=seed + 1)
    return [a, b]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M", [65, 513, 1025])
def test_production_pair_immediate_and_deferred(M, mode):
    """One launch for both products (blockIdx.z), reduced at once and through the queue; NULL out_ysum / out_xsum write nothing; each product
    inside the pair equals the same product alone, the deferred reduce equals the immediate one, and a second run agrees, bit for bit."""
    prods = _production_pair(mode, M, 40)
    _call(prods, pair=1)
    for p in prods:
        p.check(" pair")
    first = [p.outputs() for p in prods]
    for defer, pair, what in ((1, 1, "pair, deferred"), (0, 1, "pair, second run"), (0, 0, "alone"), (1, 0, "alone, deferred")):
        for p in prods:
            p.reset()
        _call(prods, pair=pair, defer=defer)
        for p, f in zip(prods, first):
            for t, u in zip(p.outputs(), f):
                _same_bits(t, u, "%s: %s against the immediate pair" % (p.tag, what))
        if defer and pair:
            for p in prods:
                p.check(" pair deferred")


@pytest.mark.parametrize("mode", ["fp32+hp", "fp32h+hp"])
@pytest.mark.parametrize("M", [65, 513])
def test_half_products_mirror_image(M, mode):
    """Gradient-sized Y lifted by y_scale, x_scale = 1 (the down_proj product of "fp16x3f"); all three outputs, both layouts."""
    prods = _two_forms(mode, M, 40, seed=21, x_mag=1.0, x_scale=1.0, y_mag=1e-6, y_scale=HP_SCALE)
    _call(prods)
    for p in prods:
        p.check(" y_scale")


@pytest.mark.parametrize("mode", MODES)
def test_columns_beyond_the_rank_have_no_effect(mode):
    M, r = 513, 40
    outs = []
    for y_pad in (True, False):
        prods = _two_forms(mode, M, r, seed=31, y_pad=y_pad)
        assert bool((prods[0].Y[:, r:] != 0).any()) == y_pad
        _call(prods)
        outs.append([p.outputs() for p in prods])
    for a, b in zip(outs[0], outs[1]):
        for t, u in zip(a, b):
            _same_bits(t, u, "Y[:, r:] non-zero against zero")


# ------------------------------------------------------------------------------------------------------------------------------
# the queue
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_queue_of_products_with_their_own_chunk_counts(mode):
    """Three products (M = 5, 513, 1025: 1, 2 and 3 chunks) of one rank and two token reductions of different nparts in ONE queue, flushed
    once: each against its reference, and bit for bit what the same product gives alone with the immediate reduce."""
    r = 40
    prods = [_two_forms(mode, M, r, seed=40 + i)[i % 2] for i, M in enumerate((5, 513, 1025))]
    assert [p.nchunks for p in prods] == [1, 2, 3]
    toks = [Tok(7, 1), Tok(17, 2)]
    _call(prods, defer=1, toks=toks)
    for p in prods:
        p.check(" queued")
    for t in toks:
        t.check(" queued behind 3 products")
    queued = [p.outputs() for p in prods]
    for p, q in zip(prods, queued):
        p.reset()
        _call([p])
        for t, u in zip(p.outputs(), q):
            _same_bits(t, u, "%s: queued among others against alone" % p.tag)


def test_token_reductions_over_the_group_loop():
    """nparts in {1, 7, 8, 9, 17} (per = ceil(nparts / 8) partials per group) in one flush: every blockIdx.y with its own nparts; each equals
    the same reduction flushed alone."""
    p = Prod("fp32", 5, 8)
    toks = [Tok(n, 3) for n in (1, 7, 8, 9, 17)]
    _call([p], defer=1, toks=toks)
    p.check(" with 5 token reductions")
    for t in toks:
        t.check(" one of 5")
    many = [t.out.clone() for t in toks]
    for t, m in zip(toks, many):
        t.reset()
        p.reset()
        _call([p], defer=1, toks=[t])
        _same_bits(t.out, m, "nparts=%d: one of 5 against alone" % t.nparts)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_full_queue(mode):
    """ReduceQueue::MAX_WG products of M = 5 and MAX_TOK token reductions in one flush."""
    prods = [Prod(mode, 5, 8, "up" if i % 2 == 0 else "down", alpha=0.5 + i / 64.0, alpha_dev=(2.0 ** -5 if i % 3 == 0 else None), seed=200 + i)
             for i in range(R.MAX_WG)]
    toks = [Tok(1 + i, 50 + i) for i in range(R.MAX_TOK)]
    _call(prods, pair=1, defer=1, toks=toks)
    for p in prods:
        p.check(" in a full queue")
    for t in toks:
        t.check(" in a full queue")


# ------------------------------------------------------------------------------------------------------------------------------
# dyt_unit_reduce_partials
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [1.0, 0.25])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 769, 3072])
@pytest.mark.parametrize("nparts", [1, 7, 8, 9, 64])
def test_reduce_partials(nparts, n, alpha):
    L = _lib.lib()
    g = _gen(nparts, n, 9)
    p_cpu = torch.randn(nparts * n, generator=g)
    o = torch.full((n + TAIL,), SENT)
    o[:n] = _start(n, 0.25)
    out0 = o.to(DEV)
    out, pd = out0.clone(), _dev(p_cpu)
    rc = L.dyt_unit_reduce_partials(ptr(pd), nparts, n, ptr(out), n, alpha, stream_ptr())
    assert rc == 0, L.dyt_last_error()
    _check_reduce("reduce_partials", "nparts=%d n=%d alpha=%g" % (nparts, n, alpha), out, out0, p_cpu, nparts, n, n, alpha)
    if nparts == 1:   # the merge form of csrc/step.hip: stride 0, one part
        out2 = out0.clone()
        rc = L.dyt_unit_reduce_partials(ptr(pd), 1, 0, ptr(out2), n, alpha, stream_ptr())
        assert rc == 0, L.dyt_last_error()
        _check_reduce("reduce_partials", "nparts=1 stride=0 n=%d alpha=%g" % (n, alpha), out2, out0, p_cpu, 1, 0, n, alpha)
        _same_bits(out2, out, "stride 0 against stride n at one part")


# ------------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------------
def _snapshot(objs):
    torch.cuda.synchronize()
    return [[t.clone() for t in o.buffers()] for o in objs]


def _unchanged(objs, snap, what, skip=()):
    torch.cuda.synchronize()
    for o, s in zip(objs, snap):
        for t, u in zip(o.buffers(), s):
            if any(t is k for k in skip):
                continue
            _same_bits(t, u, what + ": a buffer of a refused call changed")


def test_bad_arguments_are_refused_and_the_library_stays_usable():
    L = _lib.lib()
    a, b = _two_forms("fp32", 65, 8, seed=61)
    c = Prod("fp32", 130, 8, seed=63)                  # another M
    d = Prod("fp32", 65, 40, seed=64)                  # another r
    h = Prod("fp32+hp", 65, 8, x_mag=1e-6, x_scale=HP_SCALE, seed=65)
    w = Prod("bf16", 65, 8, seed=66)
    tok = Tok(3, 5)
    tok.buffers = lambda: [tok.partial, tok.out]
    objs = [a, b, c, d, h, w, tok]
    snap = _snapshot(objs)
    S = stream_ptr()

    def refused(rc, needle, skip=()):
        msg = L.dyt_last_error().decode()
        assert rc == ERR_ARG and needle in msg, (rc, msg, needle)
        _unchanged(objs, snap, needle, skip)

    def raw(prods, n=None, pair=0, defer=0, toks=None, n_tok=0, prec=0, edit=None):
        arr = (_lib.UnitWgradArgs * max(1, len(prods)))(*[p.args() for p in prods])
        if edit:
            edit(arr)
        return L.dyt_unit_wgrad(arr if prods else None, len(prods) if n is None else n, pair, defer, toks, n_tok, prec, S)

    def tokarr(partial=True, out=True, nparts=3):
        t = (_lib.UnitTokReduceArgs * 1)()
        t[0].partial, t[0].nparts, t[0].out = (tok.partial.data_ptr() if partial else None), nparts, (tok.out.data_ptr() if out else None)
        return t

    def setf(field, value, i=0):
        return lambda arr: setattr(arr[i], field, value)

    refused(raw([], n=1), "prods is NULL")
    for f in ("X", "Y", "partial", "out_w"):
        refused(raw([a], edit=setf(f, None)), "X / Y / partial / out_w is NULL")
        refused(raw([a, b], edit=setf(f, None, 1)), "product 1")
    refused(raw([a], edit=setf("r", 0)), "r = 0")
    refused(raw([a], edit=setf("r", 65)), "r = 65")
    refused(raw([a], edit=setf("M", 0)), "M = 0")
    refused(raw([a], n=0), "n_prod = 0")
    refused(raw([a] * 33), "n_prod = 33")
    refused(raw([a], defer=1, toks=tokarr(), n_tok=-1), "n_tok = -1")
    refused(raw([a], defer=1, toks=tokarr(), n_tok=17), "n_tok = 17")
    refused(raw([a], defer=0, toks=tokarr(), n_tok=1), "without defer")
    refused(raw([a], defer=1, toks=None, n_tok=1), "toks is NULL")
    refused(raw([a], defer=1, toks=tokarr(partial=False), n_tok=1), "token reduction 0")
    refused(raw([a], defer=1, toks=tokarr(out=False), n_tok=1), "token reduction 0")
    refused(raw([a], defer=1, toks=tokarr(nparts=0), n_tok=1), "nparts = 0")
    refused(raw([a, b, a], pair=1), "odd n_prod = 3")
    refused(raw([w], prec=1, edit=setf("half_products", 1)), "half_products exists at precision 0 only")
    refused(raw([h], edit=setf("x_scale", 0.0)), "x_scale = 0")
    refused(raw([h], edit=setf("y_scale", -1.0)), "y_scale = -1")
    refused(raw([a], edit=setf("x_scale", math.nan)), "x_scale = nan")
    refused(raw([a], prec=2), "precision 2")
    # the launcher's own refusals
    refused(raw([a, c], pair=1), "launch_wgrad: bad pair")                                            # different M
    refused(raw([a, d], pair=1), "launch_wgrad: bad pair")                                            # different r
    refused(raw([a, b], pair=1, edit=setf("partial", a.partial.data_ptr(), 1)), "launch_wgrad: bad pair")   # one partial buffer
    refused(raw([a, h], pair=1), "mixed product forms in a pair")
    refused(raw([h, a], pair=1, defer=1), "mixed product forms in a pair")
    # mixed ranks in a queue: product 0 is accepted and runs (its `partial` is scratch of an accepted launch: exempt), product 1 is refused
    # before its kernel is enqueued, and nothing is reduced
    refused(raw([a, d], defer=1), "mixed ranks", skip=(a.partial,))
    a.partial.copy_(a.partial0)
    # reduce_partials
    o = tok.out
    for rc in (L.dyt_unit_reduce_partials(None, 3, D + 1, ptr(o), D + 1, 1.0, S), L.dyt_unit_reduce_partials(ptr(tok.partial), 3, D + 1, None, D + 1, 1.0, S)):
        refused(rc, "dyt_unit_reduce_partials: partial / out is NULL")
    refused(L.dyt_unit_reduce_partials(ptr(tok.partial), 0, D + 1, ptr(o), D + 1, 1.0, S), "nparts = 0")
    refused(L.dyt_unit_reduce_partials(ptr(tok.partial), 3, D + 1, ptr(o), 0, 1.0, S), "n = 0")
    refused(L.dyt_unit_reduce_partials(ptr(tok.partial), 3, -1, ptr(o), D + 1, 1.0, S), "stride = -1")
    # the libraries stay usable
    _call([a, b], pair=1, defer=1, toks=[tok])
    a.check(" after the refusals")
    b.check(" after the refusals")
    tok.check(" after the refusals")
    _call([w])
    w.check(" after the refusals")
    _call([h])
    h.check(" after the refusals")
