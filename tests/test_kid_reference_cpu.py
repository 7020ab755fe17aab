"""The bounds of the kernel-Inception-distance path, measured on the CPU (tests/kid_cases.py).  Sums: two fp64 evaluations of every
case against the longdouble oracle -- plain numpy and the restatement of the kernel's summation order.  End to end: the
disagreement of the two in a subset pair's mmd2 at the end-to-end test's size.  Every figure is printed; kid_cases records them,
and each recorded bound must be 4 x the recorded figure at least and under its ceiling.  The exact cases' construction is checked
here too, so a failure of the GPU module cannot come from the cases themselves."""
import numpy as np
import pytest

import kid_cases as K

CASES = list(K.CASES)


def _held(recorded, worst):
    for k, v in worst.items():
        assert recorded[k] >= v, "%s: measured %.3e above the recorded %.3e" % (k, v, recorded[k])
        assert recorded[k] <= 1.25 * v + 1e-18, "the recorded figure of %s is stale: measured %.3e" % (k, v)


def test_sum_tol_is_four_times_the_measured_fp64_error():
    worst = {"numpy fp64": 0.0, "restatement": 0.0}
    for case in CASES:
        ref = K.reference(case)
        args = (ref["x"], ref["y"], ref["ix"], ref["iy"], ref["gamma"])
        e_np = K.sum_error(K.numpy_fp64(*args), ref["sums"], ref["mag"])
        e_re = K.sum_error(K.restatement(*args), ref["sums"], ref["mag"])
        print("%-24s numpy fp64 %.3e   restatement %.3e" % (case, e_np, e_re))
        worst["numpy fp64"], worst["restatement"] = max(worst["numpy fp64"], e_np), max(worst["restatement"], e_re)
    print("worst: %s -> SUM_TOL >= %.3e (recorded %s, SUM_TOL %.2e)" % (worst, 4 * max(worst.values()), K.MEASURED, K.SUM_TOL))
    _held(K.MEASURED, worst)
    assert 4 * max(K.MEASURED.values()) <= K.SUM_TOL <= K.SUM_TOL_CEILING


def test_the_cases_are_what_they_claim():
    for case in CASES:
        S, s, D, Nx, Ny = case
        ref = K.reference(case)
        assert ref["x"].shape == (Nx, D) and ref["y"].shape == (Ny, D) and ref["x"].dtype == ref["y"].dtype == np.float32
        assert ref["ix"].shape == ref["iy"].shape == (S, s) and ref["ix"].dtype == ref["iy"].dtype == np.int32
        assert 0 <= ref["ix"].min() and ref["ix"].max() < Nx and 0 <= ref["iy"].min() and ref["iy"].max() < Ny
        assert all(len(set(r)) == s for r in ref["ix"]) and all(len(set(r)) == s for r in ref["iy"])
        assert (ref["mag"] > 0).all() and (ref["mag"] >= np.abs(ref["sums"])).all()
    ix, iy = K.HAND_INDEX[(1, 3, 16, 5, 4)]
    assert list(ix[0]) != sorted(ix[0]) and list(iy[0]) != sorted(iy[0])          # the hand-written table is unsorted
    ix = K.reference((2, 5, 17, 9, 9))["ix"]
    assert set(ix[0]) & set(ix[1])                                                # two subsets that overlap
    ix = K.reference(K.INDEPENDENCE_CASE)["ix"]
    assert not (ix[0] == ix[1]).all() and not (ix[1] == ix[2]).all() and not (ix[0] == ix[2]).all()


def test_one_dropped_pair_is_far_above_the_bound():
    """the weight of a single ordered pair in a sum at s = 130: orders of magnitude above SUM_TOL and its ceiling"""
    ref = K.reference((2, 130, 100, 130, 200))
    a = ref["x"][ref["ix"][0]].astype(np.float64)
    t = (a[:1] @ a[1:2].T) * ref["gamma"] + 1.0
    weight = float(abs((t * t) * t)[0, 0] / ref["mag"][0, 0])
    print("one pair of 130 * 129: %.3e of the sum (SUM_TOL %.2e)" % (weight, K.SUM_TOL))
    assert weight > 1e6 * K.SUM_TOL_CEILING


@pytest.mark.parametrize("case", list(K.EXACT_CASES), ids=str)
def test_exact_cases_are_exact_in_any_order(case):
    """integer inputs in [-4, 4], gamma a power of two: numpy fp64, the tiled restatement (K steps of 4 and of 1) and longdouble
    give the same sums to the bit"""
    x, y, ix, iy, gamma = K.make_exact_inputs(case, K.EXACT_CASES[case])
    S, s, D, Nx, Ny, _ = case
    assert (x == np.round(x)).all() and (y == np.round(y)).all() and max(np.abs(x).max(), np.abs(y).max()) <= 4
    assert np.log2(gamma) == np.round(np.log2(gamma)) and 16 * D * gamma + 1 <= 17 and s * s < 2 ** 15
    want = K.exact_expected(x, y, ix, iy, gamma)
    assert want.shape == (S, 3) and want.dtype == np.float64
    for kstep in (4, 1):
        got = K.restatement(x, y, ix, iy, gamma, kstep=kstep)
        assert (got.view(np.int64) == want.view(np.int64)).all()
    ld, _ = K.oracle(x, y, ix, iy, gamma)
    assert (ld == want).all()
    assert (want * 2.0 ** 21 == np.round(want * 2.0 ** 21)).all()


def test_end_to_end_bound_at_that_size():
    """(4 subset pairs of 8 out of 12 codes, 2048 features, four seeds): a subset pair's mmd2 from plain numpy fp64 against the
    restatement's, relative to |sums0| / (s (s - 1)) + |sums1| / (s (s - 1)) + 2 |sums2| / s^2"""
    S, s, D, Nx, Ny = K.E2E
    worst = 0.0
    for seed in K.E2E_SEEDS:
        x, y = K.make_inputs(K.E2E, seed)
        ix, iy = K.make_indices(K.E2E, seed)
        s_np, s_re = K.numpy_fp64(x, y, ix, iy, 1.0 / D), K.restatement(x, y, ix, iy, 1.0 / D)
        rel = np.abs(K.KIDMOD.mmd2_from_sums(s_np, s) - K.KIDMOD.mmd2_from_sums(s_re, s)) / K.mmd2_scale(s_np, s)
        print("e2e %s seed %d: mmd2 apart by %s of the scale" % (K.E2E, seed, " ".join("%.3e" % v for v in rel)))
        worst = max(worst, float(rel.max()))
    print("worst %.3e (recorded %.3e, KID_E2E_TOL %.2e)" % (worst, K.KID_MEASURED["e2e"], K.KID_E2E_TOL))
    _held(K.KID_MEASURED, {"e2e": worst})
    assert 4 * K.KID_MEASURED["e2e"] <= K.KID_E2E_TOL <= K.SUM_TOL_CEILING
