"""The bounds of the Frechet-distance path, measured on the CPU (tests/fid_cases.py).  Moments: two fp64 evaluations of every case
against the longdouble oracle -- numpy.mean / numpy.cov and the restatement of the kernels' summation order.  Distance:
fid.frechet_distance against Tr scipy.linalg.sqrtm(S1 S2) on full-rank pairs, the self-distance of a full-rank set, and the
sensitivity of a rank-deficient pair of the end-to-end test's size to which fp64 evaluation of the covariances it is given.  Every
figure is printed; fid_cases records them, and each recorded bound must be 4 x the recorded figure at least and under its ceiling.
The exact cases' construction is checked here too, so a failure of the GPU module cannot come from the cases themselves."""
import numpy as np
import pytest
import torch

import fid_cases as K
from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import fid as F  # noqa: E402

SHAPES = list(K.CASES)


def _held(recorded, worst):
    for k, v in worst.items():
        assert recorded[k] >= v, "%s: measured %.3e above the recorded %.3e" % (k, v, recorded[k])
        assert recorded[k] <= 1.25 * v + 1e-18, "the recorded figure of %s is stale: measured %.3e" % (k, v)


def test_moment_tol_is_four_times_the_measured_fp64_error():
    worst = {"numpy fp64": 0.0, "restatement": 0.0}
    for shape in SHAPES:
        ref = K.reference(shape)
        oracle = (ref["mean"], ref["cov"])
        e_np = K.moment_error(K.numpy_fp64(ref["x"]), oracle)
        e_re = K.moment_error(K.restatement(ref["x"]), oracle)
        print("%-12s numpy fp64 %.3e   restatement %.3e" % (shape, e_np, e_re))
        worst["numpy fp64"], worst["restatement"] = max(worst["numpy fp64"], e_np), max(worst["restatement"], e_re)
    print("worst: %s -> MOMENT_TOL >= %.3e (recorded %s, MOMENT_TOL %.2e)" % (worst, 4 * max(worst.values()), K.MEASURED, K.MOMENT_TOL))
    _held(K.MEASURED, worst)
    assert 4 * max(K.MEASURED.values()) <= K.MOMENT_TOL <= K.MOMENT_TOL_CEILING


@pytest.mark.parametrize("shape", list(K.EXACT_CASES), ids=str)
def test_exact_cases_are_exact_in_any_order(shape):
    """integer means, and the same covariance bits from three summation orders; numpy.cov's reciprocal is off by at most one unit
    in the last place and is off somewhere -- the difference the entry point's true division is specified against"""
    x = K.make_exact_inputs(shape, K.EXACT_CASES[shape])
    N = shape[0]
    assert (x == np.round(x)).all() and not (x.astype(np.int64).sum(0) % N).any()
    mean, cov = K.exact_expected(x)
    m_re, c_re = K.restatement(x)
    assert (m_re == mean).all() and (c_re.view(np.int64) == cov.view(np.int64)).all()
    m_ld, c_ld = K.oracle(x)
    assert (m_ld == mean).all() and (np.abs(c_ld - cov) <= np.spacing(np.abs(cov))).all()   # (numpy.cov: a reciprocal there too)
    assert (cov == cov.T).all() and (np.diag(cov) > 0).all()
    m_np, c_np = K.numpy_fp64(x)
    ulp = np.spacing(np.abs(cov))
    assert (np.abs(c_np - cov) <= ulp).all()
    print("%s: numpy.cov (reciprocal) differs from the division on %d of %d elements" % (shape, int((c_np != cov).sum()), cov.size))
    assert (c_np != cov).any()


def _stats(x):
    m, c = K.stats64(x)
    return torch.from_numpy(m), torch.from_numpy(c)


def _sqrtm_distance(m1, S1, m2, S2):
    linalg = pytest.importorskip("scipy.linalg")
    root = linalg.sqrtm(S1.numpy() @ S2.numpy())
    d = m1 - m2
    return float(d.dot(d)) + float(torch.trace(S1)) + float(torch.trace(S2)) - 2.0 * float(np.trace(root).real)


def test_fd_tol_against_sqrtm_on_full_rank_pairs():
    """Both figures are a handful of fp64 roundings of threaded eigen-solvers and are NOT reproducible to the digit: they move with the
    thread count and, at one thread count, from run to run (seen over two dozen runs: 1.3e-15 ... 1.5e-15 against sqrtm, 1.6e-15 ...
    1.9e-15 for the self-distance).  So the figure of a run is the largest over three seeds per case and four thread counts, the
    record in fid_cases is the largest ever seen, and a run is held to the record within a factor 2 above (it then still has half of
    the 4 x margin of the bound left) and a factor 4 below (the record is not stale)."""
    pytest.importorskip("scipy")
    worst = {"vs sqrtm": 0.0, "self": 0.0}
    threads = torch.get_num_threads()
    try:
        for nt in (1, 2, 4, threads):
            torch.set_num_threads(nt)
            for case, seed in K.FD_CASES.items():
                for s in (seed, seed + 1, seed + 2):
                    x1, x2 = K.fd_pair(case, s)
                    a, b = _stats(x1), _stats(x2)
                    d, terms = F.frechet_distance(*a, *b)
                    ref = _sqrtm_distance(*a, *b)
                    rel = abs(d - ref) / abs(ref)
                    d0, t0 = F.frechet_distance(*a, *a)
                    own = abs(d0) / (2.0 * t0["tr_s1"])
                    print("%d threads %-18s seed %d: distance %.6e  vs sqrtm %.3e   self / 2 Tr S %.3e" % (nt, case, s, d, rel, own))
                    assert d > 0 and terms["tr_sqrt"] > 0
                    worst["vs sqrtm"], worst["self"] = max(worst["vs sqrtm"], rel), max(worst["self"], own)
    finally:
        torch.set_num_threads(threads)
    print("worst: %s (recorded %s; FD_TOL %.2e, FD_SELF_TOL %.2e)" % (worst, K.FD_MEASURED, K.FD_TOL, K.FD_SELF_TOL))
    for k, v in worst.items():
        assert v <= 2 * K.FD_MEASURED[k], "%s: measured %.3e, more than twice the recorded %.3e" % (k, v, K.FD_MEASURED[k])
        assert K.FD_MEASURED[k] <= 4 * v, "the recorded figure of %s is stale: measured %.3e" % (k, v)
    assert 4 * K.FD_MEASURED["vs sqrtm"] <= K.FD_TOL <= K.FD_TOL_CEILING
    assert 4 * K.FD_MEASURED["self"] <= K.FD_SELF_TOL <= K.FD_TOL_CEILING


def test_a_rank_deficient_pair_is_not_judged_against_sqrtm():
    """the record of why: at (D = 64; 20 / 30 rows) the two routes differ by far more than on full-rank pairs, and the error is
    sqrtm's (a general matrix square root of a singular product); printed, held loosely to the recorded order of magnitude"""
    pytest.importorskip("scipy")
    x1, x2 = K.fd_pair(K.FD_RANK_DEFICIENT, 0)
    a, b = _stats(x1), _stats(x2)
    d, _ = F.frechet_distance(*a, *b)
    rel = abs(d - _sqrtm_distance(*a, *b)) / abs(d)
    print("rank-deficient %s: distance %.6e, sqrtm route off by %.3e (recorded %.1e)" % (K.FD_RANK_DEFICIENT, d, rel,
                                                                                     K.FD_RANK_DEFICIENT_VS_SQRTM))
    assert rel > K.FD_TOL
    assert K.FD_RANK_DEFICIENT_VS_SQRTM / 30 <= rel <= K.FD_RANK_DEFICIENT_VS_SQRTM * 30


def test_end_to_end_bound_on_a_rank_deficient_pair_of_that_size():
    """(2048 features; 12 / 12 rows, two seeds): the distance from numpy.cov's covariances against the distance from three other
    valid fp64 evaluations of the same covariances (the longdouble oracle rounded, the restatement in K steps of 4 and of 1; all
    within MOMENT_TOL of each other), relative to Tr S1 + Tr S2.  With 12 rows some 2036 eigenvalues of each covariance are rounding
    noise of the order 1e-16 Tr S around 0; those that come out positive enter through a square root, 1e-8 each, so the figure is
    ill-conditioned by construction and moves severalfold with the BLAS thread count: the record (twice the largest seen) is held
    within a factor 2 above, as the other distance figures are, and a factor 16 below."""
    worst = 0.0
    for seed in (0, 1):
        x1, x2 = K.fd_pair(K.FD_E2E, seed)
        d_np, t = F.frechet_distance(*_stats(x1), *_stats(x2))
        for name, ev in (("oracle rounded", lambda x: [np.asarray(v, np.float64) for v in K.oracle(x)]),
                         ("restatement 4", K.restatement), ("restatement 1", lambda x: K.restatement(x, kstep=1))):
            d, _ = F.frechet_distance(*[torch.from_numpy(np.ascontiguousarray(v)) for v in list(ev(x1)) + list(ev(x2))])
            rel = abs(d_np - d) / (t["tr_s1"] + t["tr_s2"])
            print("e2e %s seed %d, %-14s: distance %.6e / %.6e, apart by %.3e of Tr S1 + Tr S2" % (K.FD_E2E, seed, name, d_np, d, rel))
            worst = max(worst, rel)
    print("worst %.3e (recorded %.3e, FD_E2E_TOL %.2e)" % (worst, K.FD_MEASURED["e2e"], K.FD_E2E_TOL))
    assert worst <= 2 * K.FD_MEASURED["e2e"] and K.FD_MEASURED["e2e"] <= 16 * worst
    assert 4 * K.FD_MEASURED["e2e"] <= K.FD_E2E_TOL
