"""The bounds and the cases of the precision / recall / density / coverage path, checked on the CPU (tests/prdc_cases.py).  Radii:
two fp64 evaluations of every case against the longdouble oracle -- the Gram form in plain numpy and the restatement of the kernel's
order; every figure is printed, prdc_cases records them, and the recorded bound must be 4 x the recorded figure at least and under
its ceiling.  Counts: every decision of every problem of every case is MARGIN * A away from its radius in longdouble, which is what
makes equality with the oracle a legitimate demand on the device; the inputs give mixed decisions.  The exact cases' construction
is checked here too, so a failure of the GPU module cannot come from the cases themselves."""
import numpy as np
import pytest

import prdc_cases as P

CASES = list(P.CASES)


def _held(recorded, worst):
    for k, v in worst.items():
        assert recorded[k] >= v, "%s: measured %.3e above the recorded %.3e" % (k, v, recorded[k])
        assert recorded[k] <= 1.25 * v + 1e-18, "the recorded figure of %s is stale: measured %.3e" % (k, v)


def test_radii_tol_is_four_times_the_measured_fp64_error():
    worst = {"numpy fp64": 0.0, "restatement": 0.0}
    for case in CASES:
        ref = P.reference(case)
        line = []
        for name, d2 in (("numpy fp64", P.numpy_fp64_d2), ("restatement", P.restatement_d2)):
            e = 0.0
            for s in ref["radii"]:
                got, order = P.knn_of(d2(ref[s], ref[s]), ref["K"][s])
                assert (order == ref["order"][s]).all(), "%s %s: the fp64 evaluation ranks the neighbours of %s differently" % (case, name, s)
                e = max(e, P.radii_error(got, ref["radii"][s], ref["mag"][(s, s)], ref["order"][s]))
            worst[name] = max(worst[name], e)
            line.append("%s %.3e" % (name, e))
        print("%-22s %s" % (case, "   ".join(line)))
    print("worst: %s -> RADII_TOL >= %.3e (recorded %s, RADII_TOL %.2e)" % (worst, 4 * max(worst.values()), P.MEASURED, P.RADII_TOL))
    _held(P.MEASURED, worst)
    assert 4 * max(P.MEASURED.values()) <= P.RADII_TOL <= P.RADII_TOL_CEILING


def test_every_decision_is_far_from_its_radius_and_the_decisions_are_mixed():
    smallest = (np.inf, None)
    for case in CASES:
        N, M, D, K = case
        ref = P.reference(case)
        assert ref["x"].shape == (N, D) and ref["y"].shape == (M, D) and ref["x"].dtype == ref["y"].dtype == np.float32
        assert set(ref["counts"]) == {p[0] for p in P.problems(case)} and len(ref["counts"]) == (4 if M >= 2 else 2)
        for name, q, p, of, side in P.problems(case):
            m = P.margin_of(ref["d2"][(q, p)], ref["mag"][(q, p)], ref["given"][of], side)
            count = ref["counts"][name]
            share = (count > 0).mean(axis=0)
            print("%-22s %-22s margin %.3e A   share of queries counted per column %s   largest count %d"
                  % (case, name, m, " ".join("%.2f" % v for v in share), count.max()))
            assert m >= P.MARGIN, "%s %s: a decision %.3e A from its radius -- change the case's seed" % (case, name, m)
            assert count.shape == (ref[q].shape[0], len(P.ks(ref["K"][of])))
            assert N < 5 or count.min() < count.max(), "%s %s decides nothing" % (case, name)
            smallest = min(smallest, (m, (case, name)))
        if N >= 5:
            share = (ref["counts"]["y in the balls of x"] > 0).mean(axis=0)
            assert 0.2 <= share.min() and share.max() <= 0.8, "%s: the share of y inside some ball of x is %s" % (case, share)
    print("smallest margin %.3e A at %s (MARGIN %.0e, ceiling of the radii bound %.0e)" % (smallest[0], smallest[1], P.MARGIN,
                                                                                           P.RADII_TOL_CEILING))
    assert P.MARGIN >= 1e3 * P.RADII_TOL_CEILING


def test_the_radius_columns():
    assert [P.ks(K) for K in (1, 2, 3, 5, 8)] == [[1], [1, 2], [1, 2, 3], [1, 2, 3, 5], [1, 2, 4, 8]]
    for case in CASES:
        assert 1 <= case[3] <= 8 and case[0] >= case[3] + 1


@pytest.mark.parametrize("case", list(P.EXACT_CASES), ids=str)
def test_exact_cases_are_exact_in_any_order(case):
    """integer inputs in [-4, 4]: numpy fp64, the restatement (K steps of 4 and of 1) and longdouble give the same distances to
    the bit, radii and counts follow; genuine ties d2 = r2 occur in the D = 48 case"""
    N, M, D, K = case
    ref = P.exact_reference(case)
    x, y = ref["x"], ref["y"]
    assert (x == np.round(x)).all() and (y == np.round(y)).all() and max(np.abs(x).max(), np.abs(y).max()) <= 4 and 64 * D <= 2 ** 13
    for a, b in (("x", "x"), ("y", "y"), ("y", "x")):
        want = ref["d2"][(a, b)]
        assert (want == np.round(want)).all()
        for got in (P.numpy_fp64_d2(ref[a], ref[b]), P.restatement_d2(ref[a], ref[b]), P.restatement_d2(ref[a], ref[b], kstep=1)):
            assert got.dtype == np.float64 and (got == want).all()
    for s in ("x", "y"):
        got, _ = P.knn_of(P.numpy_fp64_d2(ref[s], ref[s]), K)
        assert (got == ref["radii"][s]).all() and (got[:, P.np.array(P.ks(K)) - 1] == ref["given"][s]).all()
    ties = 0
    for name, q, p, of, side in P.problems(case):
        d2 = P.numpy_fp64_d2(ref[q], ref[p])
        assert (P.counts_of(d2, ref["given"][of], side) == ref["counts"][name]).all()
        r = ref["given"][of]
        ties += int((d2[:, :, None] == (r[None, :, :] if side == "support" else r[:, None, :])).sum())
    print("%s: %d ties d2 = r2 over the four problems" % (case, ties))
    if D == 48:
        assert ties > 0, "no tie: the <= of the counts is not exercised"


def test_the_duplicated_row():
    case = P.DUP_CASE
    K = case[3]
    ref = P.exact_reference(case)
    x, y = ref["x"], ref["y"]
    assert len(P.DUP_AT) == K + 1 and all((x[i] == x[P.DUP_ROW]).all() for i in P.DUP_AT) and (y[P.DUP_QUERY] == x[P.DUP_ROW]).all()
    assert min(P.DUP_AT) < 64 <= max(P.DUP_AT)                       # the copies lie in both tiles
    others = [i for i in range(case[0]) if i not in P.DUP_AT]
    assert (ref["radii"]["x"][list(P.DUP_AT)] == 0).all()            # K copies elsewhere: every radius up to the K-th is 0
    assert (ref["radii"]["x"][others][:, 0] > 0).all()
    count = ref["counts"]["y in the balls of x"]
    assert (count[P.DUP_QUERY] >= K + 1).all()                       # the bit copy is inside each copy's ball of radius 0
