"""The bound and the cases of the cross-set nearest-neighbour path, checked on the CPU (tests/nn_cases.py).  Distances: two fp64
evaluations of every case against the longdouble oracle -- the Gram form in plain numpy and the restatement of the kernel's order;
every figure is printed, nn_cases records them, and the recorded bound must be 4 x the recorded figure at least and under its
ceiling.  Indices: for every query the K + 1 smallest oracle distances are MARGIN * A apart, which is what makes equality with the
oracle's positions a legitimate demand on the device, and the same holds for the authenticity comparison, whose outcome is mixed.
The exact cases' construction is checked here too -- above all that their ties cross tiles and shares -- so a failure of the GPU
module cannot come from the cases themselves."""
import numpy as np
import pytest

import nn_cases as C
import prdc_cases as P

CASES = list(C.CASES)


def _held(recorded, worst):
    for k, v in worst.items():
        assert recorded[k] >= v, "%s: measured %.3e above the recorded %.3e" % (k, v, recorded[k])
        assert recorded[k] <= 1.25 * v + 1e-18, "the recorded figure of %s is stale: measured %.3e" % (k, v)


def test_the_cases():
    assert CASES == [(1, 1, 1, 1), (4, 5, 16, 3), (9, 9, 17, 5), (64, 64, 48, 8), (100, 67, 80, 5), (200, 130, 100, 3),
                     (9, 200, 24, 8), (3, 1100, 8, 8), (96, 96, 2048, 5)]
    for M, N, D, K in CASES + list(C.EXACT_CASES):
        assert 1 <= K <= 8 and N >= K and M >= 1
        ref = (C.reference if (M, N, D, K) in C.CASES else C.exact_reference)((M, N, D, K))
        assert ref["q"].shape == (M, D) and ref["p"].shape == (N, D) and ref["q"].dtype == ref["p"].dtype == np.float32
    assert C.shares(9, 200) == 4 and C.shares(3, 1100) == 18 and C.shares(5, 1100) == 18 and C.shares(200, 130) == 3
    assert C.shares(64, 64) == 1 and C.shares(30000, 80000) == 2
    assert list(C.share_of(np.array([0, 63, 64, 1099]), 3, 1100)) == [0, 0, 1, 17]
    assert list(C.share_of(np.array([0, 63, 64, 127, 128, 199]), 9, 200)) == [0, 0, 1, 1, 2, 3]
    assert C.ws_bytes(3, 1100, 8) == 8 * (3 + 1100 + 18 * 3 * 8) + 4 * 18 * 3 * 8
    assert C.ws_bytes(1, 1, 1) == 8 * 3 + 8                          # 4 bytes of positions, rounded up to 8


def test_dist_tol_is_four_times_the_measured_fp64_error():
    worst = {"numpy fp64": 0.0, "restatement": 0.0}
    for case in CASES:
        ref = C.reference(case)
        line = []
        for name, d2 in (("numpy fp64", P.numpy_fp64_d2), ("restatement", P.restatement_d2)):
            got, order = C.nearest(d2(ref["q"], ref["p"]), case[3])
            assert (order == ref["idx"]).all(), "%s %s: the fp64 evaluation ranks the neighbours differently" % (case, name)
            e = C.dist_error(got, ref)
            worst[name] = max(worst[name], e)
            line.append("%s %.3e" % (name, e))
        print("%-22s %s" % (case, "   ".join(line)))
    print("worst: %s -> DIST_TOL >= %.3e (recorded %s, DIST_TOL %.2e)" % (worst, 4 * max(worst.values()), C.MEASURED, C.DIST_TOL))
    _held(C.MEASURED, worst)
    assert 4 * max(C.MEASURED.values()) <= C.DIST_TOL <= C.DIST_TOL_CEILING


def test_every_neighbour_is_far_from_the_next_and_authenticity_is_mixed():
    smallest, smallest_auth = (np.inf, None), (np.inf, None)
    for case in CASES:
        M, N, D, K = case
        ref = C.reference(case)
        assert ref["q"].shape == (M, D) and ref["p"].shape == (N, D) and ref["d2"].shape == ref["idx"].shape == (M, K)
        gap = C.neighbour_gap(ref["all"], ref["mag_all"], K)
        line = "%-22s gap between a query's K + 1 first neighbours %.3e A" % (case, gap)
        assert gap >= C.MARGIN, "%s: two neighbours %.3e A apart -- change the case's seed" % (case, gap)
        smallest = (gap, case) if gap < smallest[0] else smallest
        if N >= 2:
            flags, margin = C.authentic(ref)
            share = float(flags.mean())
            line += "   authenticity margin %.3e A, authentic share %.2f" % (margin, share)
            assert margin >= C.MARGIN, "%s: an authenticity decision %.3e A from equality -- change the case's seed" % (case, margin)
            assert 0.5 < share < 0.95, "%s: the authentic share is %.2f" % (case, share)
            smallest_auth = (margin, case) if margin < smallest_auth[0] else smallest_auth
        print(line)
    print("smallest gap %.3e A at %s, smallest authenticity margin %.3e A at %s (MARGIN %.0e, ceiling of the distance bound %.0e)"
          % (smallest + smallest_auth + (C.MARGIN, C.DIST_TOL_CEILING)))
    assert C.MARGIN >= 1e3 * C.DIST_TOL_CEILING


@pytest.mark.parametrize("case", list(C.EXACT_CASES), ids=str)
def test_exact_cases_are_exact_and_tie_across_tiles_and_shares(case):
    """integer inputs in [-4, 4]: numpy fp64, the restatement (K steps of 4 and of 1) and longdouble give the same distances to the
    bit; among a query's K + 1 first neighbours equal distances occur whose positions lie in different 64-column tiles and in
    different shares -- at the K-th / (K + 1)-th place too, where the position decides who is reported"""
    M, N, D, K = case
    ref = C.exact_reference(case)
    q, p = ref["q"], ref["p"]
    assert (q == np.round(q)).all() and (p == np.round(p)).all() and max(np.abs(q).max(), np.abs(p).max()) <= 4 and 64 * D <= 2 ** 13
    want = ref["all"]
    assert (want == np.round(want)).all()
    for got in (P.numpy_fp64_d2(q, p), P.restatement_d2(q, p), P.restatement_d2(q, p, kstep=1)):
        assert got.dtype == np.float64 and (got == want).all()
    top, order = C.nearest(want, K + 1)
    assert (top[:, :K] == ref["d2"]).all() and (order[:, :K] == ref["idx"]).all()
    tie = top[:, 1:] == top[:, :-1]
    assert (order[:, 1:][tie] > order[:, :-1][tie]).all()            # the lower position first
    tiles = order // 64
    share = C.share_of(order, M, N)
    across_tiles = tie & (tiles[:, 1:] != tiles[:, :-1])
    across_shares = tie & (share[:, 1:] != share[:, :-1])
    print("%s: %d ties among the K + 1 first, %d across tiles, %d across shares (%d shares), %d at the cut"
          % (case, tie.sum(), across_tiles.sum(), across_shares.sum(), C.shares(M, N), across_shares[:, K - 1].sum()))
    assert C.shares(M, N) > 1
    assert across_tiles.any() and across_shares.any(), "no tie across tiles / shares: the position rule of the merge is not exercised"
    if case == (5, 1100, 4, 8):
        assert across_shares[:, K - 1].any(), "no tie at the cut between the K-th and the next"
        assert len(set(share[0])) > 2                                # one query's neighbours come from several shares


def test_the_duplicated_rows():
    """(70, 67, 48, 5): the bank holds K + 1 bit copies of one row and query DUP_QUERY is one more: its K nearest are the K lowest
    positions of the copies, each at exactly 0"""
    case = (70, 67, 48, 5)
    assert (case[1], case[0]) + case[2:] == P.DUP_CASE
    ref = C.exact_reference(case)
    assert (ref["d2"][P.DUP_QUERY] == 0).all() and list(ref["idx"][P.DUP_QUERY]) == sorted(P.DUP_AT)[:case[3]]
    assert min(P.DUP_AT) < 64 <= max(P.DUP_AT)
