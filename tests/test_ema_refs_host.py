"""tests/ema_refs.py against torch on the CPU: the three-rounding restatement of the model-EMA update equals timm ModelEmaV2's expression
``decay * ema_v + (1. - decay) * model_v`` on fp32 tensors BIT FOR BIT (NaN by position), for every decay the GPU tests use, with +-0,
+-inf, NaN, denormals and near-overflow values planted, and over 200 chained updates.  Then the decay schedule of
util.model_ema (a float, or a callable of the 0-based update count).  Nothing here needs a GPU or the library."""
import numpy as np
import pytest
import torch

import ema_refs as R


def _torch_update(e, m, decay):
    e, m = torch.from_numpy(np.array(e, dtype=np.float32)), torch.from_numpy(np.array(m, dtype=np.float32))
    return (decay * e + (1. - decay) * m).numpy()


def _assert_same(got, want, tag):
    assert R.same_bits(got, want), "%s: first difference (index, got, want, count) %r" % (tag, R.first_difference(got, want))


def test_the_cpu_keeps_fp32_denormals():
    """The premise of the denormal cases: neither numpy nor torch flushes them on this host."""
    tiny = np.float32(1e-45)
    assert tiny > 0 and np.float32(0.5) * np.float32(1e-42) > 0
    assert float((torch.tensor([1e-42]) * 0.5)[0]) > 0


@pytest.mark.parametrize("decay", R.DECAYS)
def test_restatement_equals_torch_bit_for_bit(decay):
    for scale in (1e-3, 1.0, 1e3):
        for n in (1, 5, 257, 70001):
            e, p = R.draws(n, seed=n + int(scale * 7), scale=scale)
            _assert_same(R.ema_ref(e, p, decay), _torch_update(e, p, decay), "decay %r scale %g n %d" % (decay, scale, n))


def test_every_special_meets_every_special():
    k = len(R.SPECIALS)
    e, p = R.draws(257, seed=1)
    pairs = {(e[i].tobytes(), p[i].tobytes()) for i in range(k * k)}
    assert len(pairs) == k * k
    for decay in R.DECAYS:
        out = R.ema_ref(e, p, decay)
        _assert_same(out, _torch_update(e, p, decay), "specials, decay %r" % decay)
    # what the formula implies at the ends: decay 1 keeps a finite average, but 0 x inf is NaN on either side
    keep = R.ema_ref(e, p, 1.0)
    fin = np.isfinite(e) & np.isfinite(p)
    assert np.array_equal(keep[fin].view(np.uint32), (e[fin] + np.float32(0.0) * p[fin]).view(np.uint32))
    assert np.isnan(keep[np.isinf(p) & np.isfinite(e)]).all()
    # denormals pass through: 0.5 x 1e-42 is a denormal, not zero
    half = R.ema_ref(np.array([1e-42], np.float32), np.array([0.0], np.float32), 0.5)
    assert 0 < half[0] < np.float32(1e-42)


@pytest.mark.parametrize("decay", R.DECAYS)
def test_200_chained_updates_on_257_elements(decay):
    e, _ = R.draws(257, seed=11)
    ref, tor = e.copy(), e.copy()
    g = np.random.default_rng(12)
    for step in range(200):
        p = g.standard_normal(257).astype(np.float32)
        ref, tor = R.ema_ref(ref, p, decay), _torch_update(tor, p, decay)
        _assert_same(ref, tor, "decay %r step %d" % (decay, step))


def test_scalars_are_rounded_once_from_the_double_difference():
    d, o = R.scalars(0.9998)
    assert d == np.float32(0.9998) and o == np.float32(1.0 - 0.9998)
    assert o != np.float32(1.0) - np.float32(0.9998)   # the difference of the rounded floats is another number
    assert R.scalars(0.0) == (0.0, 1.0) and R.scalars(1.0) == (1.0, 0.0)


# ---- the decay schedule ------------------------------------------------------------------------------------------------------------------
def test_decay_is_a_float_or_a_callable_of_the_update_count():
    from util.model_ema import decay_at
    assert decay_at(0.9998, 0) == 0.9998 and decay_at(0.9998, 12345) == 0.9998
    assert decay_at(0, 3) == 0.0 and decay_at(1, 3) == 1.0
    seen = []

    def warmup(n):   # timm V3's shape, as a caller would write it
        seen.append(n)
        return min(0.9998, (1. + n) / (10. + n))
    assert [decay_at(warmup, n) for n in range(3)] == [1. / 10., 2. / 11., 3. / 12.]
    assert seen == [0, 1, 2]
    assert decay_at(warmup, 10 ** 6) == 0.9998
    equal_weight = lambda n: n / (n + 1.)   # noqa: E731
    assert [decay_at(equal_weight, n) for n in range(4)] == [0.0, 0.5, 2. / 3., 0.75]


@pytest.mark.parametrize("bad", [-0.1, 1.0001, float("nan"), float("inf"), "x", None])
def test_bad_decays_are_refused(bad):
    from util.model_ema import decay_at
    with pytest.raises(ValueError):
        decay_at(bad, 0)
    with pytest.raises(ValueError):
        decay_at(lambda n: bad, 7)


def test_equal_weight_schedule_gives_the_running_mean():
    """n / (n + 1) through the reference: after k updates the shadow is the mean of the k parameter states (to rounding)."""
    from util.model_ema import decay_at
    g = np.random.default_rng(3)
    states = [g.standard_normal(64).astype(np.float32) for _ in range(8)]
    shadow = np.full(64, 123.0, np.float32)   # wiped by the first update (decay 0)
    for n, p in enumerate(states):
        shadow = R.ema_ref(shadow, p, decay_at(lambda k: k / (k + 1.), n))
    assert np.allclose(shadow, np.mean(np.stack(states).astype(np.float64), axis=0), rtol=0, atol=1e-6)
