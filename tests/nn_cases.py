"""Shapes, seeded inputs, oracle and measured bound of the cross-set nearest-neighbour entry point mogan_knn_cross_f64
(csrc/mogan_knn.hip), shared by tests/test_nn_reference_cpu.py (which measures the bound and checks the cases)
and tests/test_nn_gpu.py (which applies them).  Modelled on tests/prdc_cases.py, whose inputs and distance evaluations it reuses.

A case (M, N, D, K) is M queries against a bank of N rows with D features and K neighbours per query, built as
prdc_cases.make_inputs((N, M, D, K), seed): x, the first set, is the bank, and y, of which every odd row is pushed outward, the
queries.

Oracle.  d2 in numpy.longdouble by direct differences (prdc_cases.oracle_d2), then a STABLE argsort of every query's row: the K
first positions and their distances, the lower position first where two distances are equal.

Indices.  Equality with the oracle, every query, every column.  That is legitimate because the CPU module asserts that for every
query the K + 1 smallest oracle distances (all N where N <= K) are pairwise MARGIN * A = 1e-9 A apart at least, A the larger of
the two pairs' magnitudes |a|^2 + |b|^2 + 2 sum |a_k b_k| -- four orders above the ceiling of the distance bound, so no fp64
evaluation within the bound can order them differently.  It is a condition on the cases, not a tolerance: no query is left out.
The same margin is asserted for the comparison the authenticity figure makes, d2(q, t*) against d2_NN(t*), whose outcome over a
case's queries must be mixed.

Distance bound.  err = |got - oracle| / A of the pair the oracle's k-th neighbour is.  DIST_TOL is 4 x the largest err over CASES
of the two fp64 CPU evaluations prdc_cases.numpy_fp64_d2 and prdc_cases.restatement_d2 (the kernel's order).  MEASURED holds the
figures the CPU module printed; that module holds DIST_TOL to them and to the ceiling 1e-13 (fid_cases.MOMENT_TOL_CEILING).  No
bound comes from the code under test.

Exact cases.  Integer-valued fp32 inputs in [-4, 4] (prdc_cases.make_exact_inputs): every distance is an integer, exact in fp64 in
any order, so the distances must equal numpy_fp64_d2's bit for bit and the indices the stable argsort of the integers.  Ties are
plentiful, and the CPU module asserts that ties among a query's K + 1 first occur ACROSS 64-column tiles and across the shares the
tiles are split into: there the position decides, and a merge that ignored it would be seen.  (5, 1100, 4, 8) spreads equal
distances over 18 shares of one tile each.
"""
import numpy as np

import fid_cases
import prdc_cases as P

LD = np.longdouble
MARGIN = P.MARGIN
DIST_TOL_CEILING = fid_cases.MOMENT_TOL_CEILING

# (M, N, D, K) -> seed
CASES = {
    (1, 1, 1, 1): 0,              # the smallest legal problem
    (4, 5, 16, 3): 0,
    (9, 9, 17, 5): 0,             # a D tail of 1
    (64, 64, 48, 8): 0,           # exactly one tile, K max
    (100, 67, 80, 5): 0,          # a tail of 3 in the second tile, M != N
    (200, 130, 100, 3): 0,        # three stripe rows
    (9, 200, 24, 8): 0,           # 4 shares
    (3, 1100, 8, 8): 0,           # 18 shares, deep merge
    (96, 96, 2048, 5): 0,         # the workload's D
}
EXACT_CASES = {(70, 67, 48, 5): 1, (140, 130, 128, 8): 1, (5, 1100, 4, 8): 1}

# ---- recorded by tests/test_nn_reference_cpu.py (it fails when a figure is exceeded or stale) ----
MEASURED = {"numpy fp64": 3.7e-16, "restatement": 1.2e-15}
DIST_TOL = 4.8e-15


def shares(rows, cols):
    """the closed form of the split of the support tiles: min(ceil(512 / Tr), Tc, 64)"""
    tr, tc = (rows + 63) // 64, (cols + 63) // 64
    return max(1, min(-(-512 // tr), tc, 64))


def ws_bytes(M, N, K):
    """the header's formula: 8 (M + N + shares M K) + 4 shares M K rounded up to 8"""
    lists = shares(M, N) * M * K
    return 8 * (M + N + lists) + (4 * lists + 7) // 8 * 8


def share_of(pos, M, N):
    """the share that holds bank position `pos`: share s walks the tiles T s // S .. T (s + 1) // S - 1"""
    T, S = (N + 63) // 64, shares(M, N)
    tile = np.asarray(pos) // 64
    edges = np.array([T * s // S for s in range(S + 1)])
    return np.searchsorted(edges, tile, side="right") - 1


def make_inputs(case, seed):
    """(queries (M, D), bank (N, D)) fp32"""
    M, N, D, K = case
    x, y = P.make_inputs((N, M, D, K), seed)
    return y, x


def make_exact_inputs(case, seed):
    """(queries, bank): integer-valued fp32 in [-4, 4]; (70, 67, 48, 5) has prdc_cases' duplicate rows"""
    M, N, D, K = case
    x, y = P.make_exact_inputs((N, M, D, K), seed)
    return y, x


def nearest(d2, K):
    """(the K smallest of every row of d2 (M, N), ascending, the lower position first among equals (M, K); their positions)"""
    order = np.argsort(d2, axis=1, kind="stable")[:, :K]
    return np.take_along_axis(d2, order, axis=1), order


def neighbour_gap(d2, mag, K):
    """the smallest (d_(k+1) - d_(k)) / max(A_(k), A_(k+1)) over every query and k < min(K + 1, N) - 1; inf where N = 1"""
    top, order = nearest(d2, min(K + 1, d2.shape[1]))
    a = np.take_along_axis(mag, order, axis=1)
    if top.shape[1] < 2:
        return np.inf
    return float(((top[:, 1:] - top[:, :-1]) / np.maximum(a[:, 1:], a[:, :-1])).min())


def dist_error(got, ref):
    """the largest |got - oracle| / A over (query, k), A of the pair the oracle's k-th neighbour is"""
    return float((np.abs(np.asarray(got, LD) - ref["d2"]) / ref["mag"]).max())


_REF = {}


def _reference(key, q, p, K):
    if key not in _REF:
        d_all, a_all = P.oracle_d2(q, p)
        d2, idx = nearest(d_all, K)
        ref = {"q": q, "p": p, "K": K, "all": d_all, "mag_all": a_all, "d2": d2, "idx": idx,
               "mag": np.take_along_axis(a_all, idx, axis=1)}
        if p.shape[0] >= 2:
            d_pp, a_pp = P.oracle_d2(p, p)
            nn, nn_at = P.knn_of(d_pp, 1)
            ref.update({"bank": d_pp, "mag_bank": a_pp, "nn_bank": nn[:, 0], "nn_at": nn_at[:, 0]})
        for a in ref.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def reference(case):
    """{"q", "p", "K", "all" (M, N), "mag_all", "d2" (M, K), "idx" (M, K), "mag" (M, K)} of a case of CASES under its seed, in
    longdouble, and where N >= 2 the bank's own "bank" (N, N), "mag_bank", "nn_bank" (N,), "nn_at" (N,); computed once, frozen"""
    key = (case, "c")
    if key not in _REF:
        _reference(key, *make_inputs(case, CASES[case]), case[3])
    return _REF[key]


def exact_reference(case):
    """the same of a case of EXACT_CASES; every figure is an integer, so longdouble and fp64 agree to the bit"""
    key = (case, "e")
    if key not in _REF:
        _reference(key, *make_exact_inputs(case, EXACT_CASES[case]), case[3])
    return _REF[key]


def authentic(ref):
    """(authentic (M,) bool, margin): d2(q, t*) >= d2_NN(t*) per query in longdouble and the smallest |difference| / A over the
    queries, A the larger of the magnitudes of (q, t*) and of (t*, its nearest other bank row)"""
    t = ref["idx"][:, 0]
    own = ref["nn_bank"][t]
    a = np.maximum(ref["mag"][:, 0], ref["mag_bank"][t, ref["nn_at"][t]])
    return ref["d2"][:, 0] >= own, float((np.abs(ref["d2"][:, 0] - own) / a).min())
