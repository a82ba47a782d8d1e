"""CPU: the model of the slot meters' summation plan (tests/slot_sum_plan.py) that the device sums
are compared with bit for bit in test_gpu_squelch.py and test_gpu_freq.py.

Two things are checked here.  The model is a sum of the right terms: it lies within the bounds the
device tests already allow against the exactly rounded sums.  And the bit comparison is not vacuous:
on its own inputs the model differs, in some slot, from the same terms added left to right, at every
length from 4097 up for the level meter's float32 terms and from 65 up for the frequency meter's
double terms.  Below those lengths a sum of so few terms of 24 or 48 significant bits is exact in
double, or nearly always so, and no order of additions can be told from another: nothing is asserted
there."""
import numpy as np
import pytest

import freq_ref
import slot_sum_plan as plan
import squelch_ref


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def test_no_terms_and_one_term():
    assert bits(plan.plan_sum(np.zeros(0)))[()] == 0                # +0.0
    for v in (0.0, 1.5, -2.0 ** -40, 3e300):
        assert bits(plan.plan_sum(np.array([v])))[()] == bits(v)[()]
    assert [t.size for t in plan.power_terms(1)] == [1] * plan.K
    assert [tr.size for tr, _ in plan.r1_terms(0, False)] == [0] * plan.K
    assert [tr.size for tr, _ in plan.r1_terms(1, False)] == [1] * plan.K
    re, im = plan.r1_sums(1, False)                                  # one sample, no predecessor: nothing summed
    assert not bits(re).any() and not bits(im).any()


def test_small_integers_add_exactly_in_any_order():
    rng = np.random.Generator(np.random.PCG64(1))
    for n in (1, 255, 256, 257, plan.TILE, plan.TILE + 1, 5 * plan.TILE + 3):
        t = rng.integers(-1000, 1000, n).astype(np.float64)
        assert plan.plan_sum(t) == t.sum() == plan.sequential_sum(t), n


@pytest.mark.parametrize("n", plan.POWER_LENGTHS)
def test_power_model_is_within_the_level_bound_and_differs_from_a_sequential_sum(n):
    re, im = plan.pin_rows(n)
    differs = False
    for k, t in enumerate(plan.power_terms(n)):
        got, exact = plan.plan_sum(t), squelch_ref.exact_sum(re[k], im[k])
        assert abs(got - exact) <= 1e-13 * exact, (n, k, got, exact)          # test_gpu_squelch's bound on the sums
        assert squelch_ref.within_one_ulp(squelch_ref.level_of_sum(got, n), squelch_ref.level(re[k], im[k])), (n, k)
        differs = differs or bits(got)[()] != bits(plan.sequential_sum(t))[()]
    if n >= 4097:
        assert differs, n


@pytest.mark.parametrize("carried", [False, True])
@pytest.mark.parametrize("n", plan.R1_LENGTHS)
def test_r1_model_is_within_the_meter_bound_and_differs_from_a_sequential_sum(n, carried):
    re, im = plan.pin_rows(n)
    got_re, got_im = plan.r1_sums(n, carried)
    differs = False
    for k, (tr, ti) in enumerate(plan.r1_terms(n, carried)):
        assert tr.size == ti.size == n
        want = freq_ref.r1(re[k], im[k], (re[k, -1], im[k, -1]) if carried and n else None)
        assert want[2] == (n if carried else max(n - 1, 0))
        assert abs(got_re[k] - want[0]) <= want[3], (n, k, got_re[k], want[0], want[3])
        assert abs(got_im[k] - want[1]) <= want[4], (n, k, got_im[k], want[1], want[4])
        differs = differs or bits(got_re[k])[()] != bits(plan.sequential_sum(tr))[()] \
            or bits(got_im[k])[()] != bits(plan.sequential_sum(ti))[()]
    if n >= 65:
        assert differs, n
