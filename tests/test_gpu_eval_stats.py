"""GPU tests of dyt_eval_rows / dyt_eval_keep (csrc/eval_stats.hip) through the C ABI of BOTH libraries, against tests/eval_refs.py: counts, ranks,
histograms and per_class exactly; row_loss under the rule of DESIGN 7g -- floor = max|fp32_cpu - fp64| of the reference on the same input,
max|gpu - fp64| <= 4 floor + 4 ulp(max|fp64|) -- with the worst error / floor printed per shape for the DESIGN 7p table.

Every shape runs as ceil(12 / rows) (at least 2) batches of `rows` rows whose row kinds rotate through: randn x 30, shifted by +-1e4, one class
90 above the rest, a fully tied row, the label tied with its neighbours on both index sides, the label at 0 and at C - 1, -inf on non-label
classes, a NaN row, labels -1 and C.  The batches accumulate into one state, which must equal the reference's fold of the concatenation;
each layout -- contiguous, ld = C + 1, ld = C + 3, a view offset by one element -- sees the same batches."""
import ctypes
import math

import pytest
import torch

import eval_refs as R

pytestmark = pytest.mark.gpu

# every class count with two row counts, every row count with (at least) three class counts
SHAPES = [(1, 1), (1, 257), (2, 3), (2, 64), (5, 4), (5, 65), (63, 5), (63, 1), (64, 64), (64, 3), (65, 65), (65, 4), (255, 257), (255, 5),
          (256, 1), (256, 64), (257, 3), (257, 65), (1000, 4), (1000, 257), (1024, 5), (1024, 64), (1025, 64), (1025, 1), (4099, 65), (4099, 3),
          (21843, 257), (21843, 4), (65536, 5), (65536, 3)]
LAYOUTS = ("contiguous", "ld+1", "ld+3", "offset1")
KINDS = 12
L, T = 12, 196


def _batch(C, rows, first, seed):
    """rows x C logits (fp32 values) and labels; row i is of kind (first + i) % KINDS."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C, generator=g) * 30.0
    y = torch.randint(0, C, (rows,), generator=g)
    for i in range(rows):
        kind, t = (first + i) % KINDS, int(y[i])
        if kind == 1:
            x[i] += 1e4
        elif kind == 2:
            x[i] -= 1e4
        elif kind == 3:
            k = int(torch.randint(0, C, (1,), generator=g))
            x[i] = torch.randn(C, generator=g)
            x[i, k] = float(x[i].max()) + 90.0
        elif kind == 4:
            x[i] = 0.5
        elif kind == 5:
            x[i, max(0, t - 1):t + 2] = float(x[i].median())
        elif kind == 6:
            y[i] = 0
        elif kind == 7:
            y[i] = C - 1
        elif kind == 8:
            off = torch.rand(C, generator=g) < 0.5
            off[t] = False
            x[i, off] = float("-inf")
        elif kind == 9:
            x[i, int(torch.randint(0, C, (1,), generator=g))] = float("nan")
        elif kind == 10:
            y[i] = -1
        elif kind == 11:
            y[i] = C
    return x, y


_REF = {}


def _reference(C, rows):
    """The batches of a shape with their fp64 / fp32 reference rows and the fold of the concatenation: computed once, shared, never modified."""
    key = (C, rows)
    if key not in _REF:
        nb = max(2, math.ceil(KINDS / rows))
        batches = []
        for b in range(nb):
            x, y = _batch(C, rows, b * rows, seed=1000 * C + 10 * rows + b)
            rank, loss64 = R.rows(x.double(), y)
            _, loss32 = R.rows(x, y)
            batches.append((x, y, rank, loss64, loss32))
        rank = torch.cat([b[2] for b in batches])
        fold = R.fold(rank, torch.cat([b[3] for b in batches]), torch.cat([b[1] for b in batches]), C, L, T)
        _REF[key] = (batches, fold)
    return _REF[key]


def _place(x, layout):
    """The batch on the device in one of the four layouts; what is not part of a row holds NaN (a kernel that read it would report a NaN row)."""
    rows, C = x.shape
    if layout == "contiguous":
        return x.cuda()
    if layout == "offset1":
        buf = torch.full((rows * C + 1,), float("nan"), device="cuda")
        v = buf[1:].view(rows, C)
    else:
        ld = C + (1 if layout == "ld+1" else 3)
        buf = torch.full((rows, ld), float("nan"), device="cuda")
        v = buf[:, :C]
    v.copy_(x)
    return v


class _State:
    def __init__(self, C, rows):
        self.counts = torch.zeros(R.counts_words(L, T), dtype=torch.int64, device="cuda")
        self.per_class = torch.zeros(2 * C, dtype=torch.int64, device="cuda")
        self.loss_sum = torch.zeros(1, dtype=torch.float64, device="cuda")
        self.rank = torch.full((rows,), -7, dtype=torch.int32, device="cuda")
        self.loss = torch.full((rows,), float("nan"), device="cuda")


def _eval_rows(lib, v, y, st, per_class=True):
    import _lib
    rows, C = v.shape
    ld = v.stride(0) if rows > 1 else max(C, v.stride(0))
    rc = lib.dyt_eval_rows(ctypes.c_void_p(v.data_ptr()), ld, _lib.ptr(y), rows, C, _lib.ptr(st.counts), _lib.ptr(st.per_class) if per_class else None,
                           _lib.ptr(st.loss_sum), _lib.ptr(st.rank), _lib.ptr(st.loss), _lib.stream_ptr())
    assert rc == 0, lib.dyt_last_error()


def _libs():
    import _lib
    return (("bf16", _lib.lib()), ("fp16", _lib.lib(fp16=True)))


@pytest.mark.parametrize("C,rows", SHAPES)
def test_rows_against_the_reference(C, rows):
    batches, (want_counts, want_pc, want_sum) = _reference(C, rows)
    worst, first_state = 0.0, {}
    for name, lib in _libs():
        for layout in LAYOUTS:
            st = _State(C, rows)
            own_sum, own_abs = 0.0, 0.0
            for x, y, rank, loss64, loss32 in batches:
                v, yd = _place(x, layout), y.cuda()
                if layout != "contiguous":
                    assert v.data_ptr() % 16 != 0 or v.stride(0) != C
                _eval_rows(lib, v, yd, st)
                got_rank, got_loss = st.rank.cpu().long(), st.loss.cpu()
                assert torch.equal(got_rank, rank), (name, layout, got_rank.tolist()[:8], rank.tolist()[:8])
                live = (rank >= 0) & (rank < C)
                assert bool((got_loss[~live] == 0).all())
                if bool(live.any()):
                    floor, bound = R.loss_bound(loss64[live], loss32[live])
                    err = float((got_loss[live].double() - loss64[live]).abs().max())
                    ratio = err / floor if floor > 0 else (0.0 if err == 0 else float("inf"))
                    print("eval_rows %s %s C=%d rows=%d: error %.3e floor %.3e error/floor %.2f bound %.3e" % (name, layout, C, rows, err, floor, ratio, bound))
                    if floor > 0:
                        worst = max(worst, ratio)
                    assert err <= bound, (name, layout, err, floor, bound)
                own_sum += float(got_loss[live].double().sum())
                own_abs += float(got_loss[live].double().abs().sum())
            counts, pc, ls = st.counts.cpu(), st.per_class.cpu(), float(st.loss_sum.cpu()[0])
            assert torch.equal(counts, want_counts), (name, layout, counts[:24].tolist(), want_counts[:24].tolist())
            assert torch.equal(pc, want_pc), (name, layout)
            total = rows * len(batches)
            assert abs(ls - own_sum) <= total * 2.0 ** -52 * own_abs, (name, layout, ls, own_sum)   # the fold: a double sum of the kernel's own row_loss
            assert abs(ls - float(want_sum)) <= total * R.loss_bound(torch.cat([b[3] for b in batches]), torch.cat([b[4] for b in batches]))[1]
            # both libraries hold the same code: the same bits per layout (a layout changes which lane adds what, so the loss word only
            # agrees across layouts within the bounds above; the integers are the reference's everywhere)
            if layout not in first_state:
                first_state[layout] = ls
            else:
                assert ls == first_state[layout], (name, layout, ls, first_state[layout])
    print("eval_rows C=%d rows=%d: worst error/floor %.2f" % (C, rows, worst))


@pytest.mark.parametrize("C,rows", [(100, 128), (1000, 65), (21843, 65)])
def test_accumulation_and_reproducibility(C, rows):
    """Two updates equal one update of the concatenation (integers exactly, the loss word within the double-sum bound), the state and the row
    results are bit-identical over two runs, and per_class may be NULL."""
    import _lib
    lib = _lib.lib()
    x, y = _batch(C, 2 * rows, 0, seed=77 + C)
    xd, yd = x.cuda(), y.cuda()

    def run(parts, per_class=True):
        st = _State(C, 2 * rows)
        outs = []
        for sl in parts:
            _eval_rows(lib, xd[sl], yd[sl].contiguous(), st, per_class)
            n = sl.stop - sl.start
            outs.append((st.rank[:n].clone(), st.loss[:n].clone()))
        return st, outs
    whole, (wo,) = run([slice(0, 2 * rows)])
    again, (ao,) = run([slice(0, 2 * rows)])
    split, so = run([slice(0, rows), slice(rows, 2 * rows)])
    assert torch.equal(whole.counts, again.counts) and torch.equal(whole.per_class, again.per_class) and torch.equal(whole.loss_sum, again.loss_sum)
    assert torch.equal(wo[0], ao[0]) and torch.equal(wo[1].view(torch.int32), ao[1].view(torch.int32))
    assert torch.equal(split.counts, whole.counts) and torch.equal(split.per_class, whole.per_class)
    assert torch.equal(torch.cat([so[0][0], so[1][0]]), wo[0]) and torch.equal(torch.cat([so[0][1], so[1][1]]).view(torch.int32), wo[1].view(torch.int32))
    bound = 2 * rows * 2.0 ** -52 * float(wo[1].double().abs().sum())
    assert abs(float(split.loss_sum) - float(whole.loss_sum)) <= bound
    bare, _ = run([slice(0, 2 * rows)], per_class=False)
    assert torch.equal(bare.counts, whole.counts) and int(bare.per_class.abs().sum()) == 0 and torch.equal(bare.loss_sum, whole.loss_sum)
    assert int(whole.counts[R.ROWS]) + int(whole.counts[R.IGNORED]) == 2 * rows and int(whole.counts[R.NAN_ROWS]) > 0 and int(whole.counts[R.IGNORED]) > 0


@pytest.mark.parametrize("tokens", [196, 1])
@pytest.mark.parametrize("images", [1, 3, 65])
def test_keep_histogram(images, tokens):
    import _lib
    g = torch.Generator().manual_seed(images * 1000 + tokens)
    masks = {"kept": torch.ones(images, L, tokens), "dropped": torch.zeros(images, L, tokens),
             "random": (torch.rand(images, L, tokens, generator=g) < torch.rand(images, L, 1, generator=g)).float()}
    for name, lib in _libs():
        counts = torch.zeros(R.counts_words(L, tokens), dtype=torch.int64, device="cuda")
        want = torch.zeros_like(counts).cpu()
        for kind, m in masks.items():
            md = m.cuda()
            assert lib.dyt_eval_keep(_lib.ptr(md), images, L, tokens, _lib.ptr(counts), _lib.stream_ptr()) == 0, lib.dyt_last_error()
            want += R.keep_counts(m)
            assert torch.equal(counts.cpu(), want), (name, kind)
        assert int(want[R.MASK_ROWS]) == 3 * images and int(want[R.OFF_KEEP:].sum()) == 3 * images * L
        assert int(want[:R.MASK_ROWS].sum()) == 0 and int(want[R.OFF_RANK:R.OFF_KEEP].sum()) == 0   # the row words are not the keep kernel's


def test_refusals_leave_the_library_usable():
    import _lib
    C, rows = 10, 4
    x, y = _batch(C, rows, 0, seed=5)
    for name, lib in _libs():
        st = _State(C, rows)
        v, yd = x.cuda(), y.cuda()
        args = [ctypes.c_void_p(v.data_ptr()), C, _lib.ptr(yd), rows, C, _lib.ptr(st.counts), _lib.ptr(st.per_class), _lib.ptr(st.loss_sum),
                _lib.ptr(st.rank), _lib.ptr(st.loss), _lib.stream_ptr()]
        for at, bad in ((3, 0), (3, (1 << 20) + 1), (4, 0), (4, 65537), (1, C - 1), (0, None), (5, None), (7, ctypes.c_void_p(st.loss_sum.data_ptr() + 4))):
            a = list(args)
            a[at] = bad
            assert lib.dyt_eval_rows(*a) == -1 and lib.dyt_last_error(), (name, at)
        m = torch.ones(2, L, T, device="cuda")
        for a in ((None, 2, L, T, _lib.ptr(st.counts)), (_lib.ptr(m), 0, L, T, _lib.ptr(st.counts)), (_lib.ptr(m), 2, 65, T, _lib.ptr(st.counts)),
                  (_lib.ptr(m), 2, L, 1025, _lib.ptr(st.counts)), (_lib.ptr(m), 2, L, T, None)):
            assert lib.dyt_eval_keep(*a, _lib.stream_ptr()) == -1 and lib.dyt_last_error(), name
        torch.cuda.synchronize()
        assert int(st.counts.abs().sum()) == 0 and float(st.loss_sum) == 0.0   # nothing was enqueued
        _eval_rows(lib, v, yd, st)
        assert lib.dyt_eval_keep(_lib.ptr(m), 2, L, T, _lib.ptr(st.counts), _lib.stream_ptr()) == 0
        rank, _ = R.rows(x.double(), y)
        assert torch.equal(st.rank.cpu().long(), rank) and int(st.counts[R.MASK_ROWS]) == 2
