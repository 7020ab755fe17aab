"""Host side of the kernel Inception distance (attngan/kid.py) and its command line (attngan/main.py), without a GPU: the subset
draws and their documented order, the estimator on hand-computed sets and against a plain double loop, the mean and spread, the
subset-size rule, and the --kid options."""
import numpy as np
import pytest

import kid_cases as K
from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import kid as KID  # noqa: E402
from mogan_amd.attngan import main as entry  # noqa: E402


# ------------------------------------------------------------------------------------------------- draw_subsets
def test_draw_subsets_shape_range_repeats_and_determinism():
    ix, iy = KID.draw_subsets(50, 40, 7, 13, seed=5)
    assert ix.shape == iy.shape == (7, 13) and ix.dtype == iy.dtype == np.int32
    assert ix.min() >= 0 and ix.max() < 50 and iy.min() >= 0 and iy.max() < 40
    assert all(len(set(r)) == 13 for r in ix) and all(len(set(r)) == 13 for r in iy)
    ix2, iy2 = KID.draw_subsets(50, 40, 7, 13, seed=5)
    assert (ix2 == ix).all() and (iy2 == iy).all()
    ix3, iy3 = KID.draw_subsets(50, 40, 7, 13, seed=6)
    assert not (ix3 == ix).all() and not (iy3 == iy).all()
    full, _ = KID.draw_subsets(9, 9, 3, 9, seed=1)                    # s = n: every row a permutation
    assert all(sorted(r) == list(range(9)) for r in full)


def test_draw_subsets_order_is_the_documented_one():
    """ONE RandomState(seed); per subset pair first the real side's choice, then the generated side's"""
    ix, iy = KID.draw_subsets(30, 20, 4, 6, seed=100)
    rng = np.random.RandomState(100)
    for k in range(4):
        assert (ix[k] == rng.choice(30, 6, replace=False)).all()
        assert (iy[k] == rng.choice(20, 6, replace=False)).all()
    longer, _ = KID.draw_subsets(30, 20, 6, 6, seed=100)              # more subset pairs extend the table, they do not change it
    assert (longer[:4] == ix).all()


@pytest.mark.parametrize("kw", [dict(subsets=0), dict(subset_size=1), dict(subset_size=11), dict(subset_size=0)])
def test_draw_subsets_rejects(kw):
    args = dict(n_real=12, n_fake=10, subsets=3, subset_size=5, seed=0)
    args.update(kw)
    with pytest.raises(ValueError):
        KID.draw_subsets(**args)


# ------------------------------------------------------------------------------------------------- the estimator
def test_mmd2_on_hand_computed_sets():
    """D = 1, gamma = 1, coef0 = 1: x = (0, 1), y = (1, 2).  k(a, b) = (a b + 1)^3:
    xx off-diagonal: k(0, 1) twice = 2;  yy: k(1, 2) = 27 twice = 54;  xy: k(0,1) + k(0,2) + k(1,1) + k(1,2) = 1 + 1 + 8 + 27 = 37.
    mmd2 = 2 / 2 + 54 / 2 - 2 * 37 / 4 = 9.5"""
    x, y = np.array([[0.0], [1.0]], np.float32), np.array([[1.0], [2.0]], np.float32)
    idx = np.array([[0, 1]], dtype=np.int32)
    sums = K.numpy_fp64(x, y, idx, idx, 1.0)
    assert sums.tolist() == [[2.0, 54.0, 37.0]]
    assert KID.mmd2_from_sums(sums, 2).tolist() == [9.5]
    # three points a side, identical sets: x = y = (0, 1, -1): xx = 2 (k(0,1) + k(0,-1) + k(1,-1)) = 2 (1 + 1 + 0) = 4,
    # xy = xx + the diagonal (1 + 8 + 8) = 21; mmd2 = 4 / 6 + 4 / 6 - 2 * 21 / 9: negative -- the estimator is not clamped
    x = np.array([[0.0], [1.0], [-1.0]], np.float32)
    idx = np.array([[0, 1, 2]], dtype=np.int32)
    sums = K.numpy_fp64(x, x, idx, idx, 1.0)
    assert sums.tolist() == [[4.0, 4.0, 21.0]]
    got = KID.mmd2_from_sums(sums, 3)
    assert got[0] == 4.0 / 6.0 + 4.0 / 6.0 - 2.0 * 21.0 / 9.0 and got[0] < 0
    # position, not value, decides i != j: a row listed twice pairs with itself
    idx = np.array([[1, 1]], dtype=np.int32)
    assert K.numpy_fp64(x, x, idx, idx, 1.0).tolist() == [[16.0, 16.0, 32.0]]


def _double_loop(x, y, gamma, coef0=1.0):
    x, y = x.astype(np.float64), y.astype(np.float64)
    k = lambda a, b: (gamma * float(np.dot(a, b)) + coef0) ** 3       # noqa: E731
    n, m = len(x), len(y)
    xx = sum(k(x[i], x[j]) for i in range(n) for j in range(n) if i != j) / (n * (n - 1))
    yy = sum(k(y[i], y[j]) for i in range(m) for j in range(m) if i != j) / (m * (m - 1))
    xy = sum(k(x[i], y[j]) for i in range(n) for j in range(m)) / (n * m)
    return xx + yy - 2.0 * xy


@pytest.mark.parametrize("case", [(16, 40, 40), (24, 33, 33)], ids=str)
def test_mmd2_against_a_plain_double_loop_on_full_rank_pairs(case):
    D, n, _ = case
    x, y = K.fid_cases.fd_pair(case, 3)
    idx = np.arange(n, dtype=np.int32)[None]
    sums = K.numpy_fp64(x, y, idx, idx, 1.0 / D)
    got = KID.mmd2_from_sums(sums, n)[0]
    want = _double_loop(x, y, 1.0 / D)
    scale = K.mmd2_scale(sums, n)[0]
    print("%s: mmd2 %.9e, double loop %.9e, apart by %.3e of the scale" % (case, got, want, abs(got - want) / scale))
    # both are fp64 evaluations of the same sums of n^2 terms (pow against two multiplications: 1 ulp per term at most); the
    # sums' own bound K.SUM_TOL, measured for exactly this kind of disagreement, holds with room
    assert abs(got - want) <= K.SUM_TOL * scale
    assert got > 0


def test_mmd2_order_of_operations_and_rejections():
    sums = np.array([[3.0, 5.0, 7.0], [1e20, -1e20, 1.0]])
    s = 4
    want = [r[0] / 12.0 + r[1] / 12.0 - 2.0 * r[2] / 16.0 for r in sums.tolist()]
    got = KID.mmd2_from_sums(sums, s)
    assert got.dtype == np.float64 and got.tolist() == want
    for bad in (np.zeros((3,)), np.zeros((2, 2)), np.zeros((2, 3, 1))):
        with pytest.raises(ValueError):
            KID.mmd2_from_sums(bad, 4)
    with pytest.raises(ValueError):
        KID.mmd2_from_sums(sums, 1)


def test_kid_is_the_mean_and_the_population_std():
    rng = np.random.RandomState(2)
    sums = rng.uniform(1.0, 2.0, (9, 3)) * 1e4
    mean, std, per = KID.kid_from_sums(sums, 10)
    m = KID.mmd2_from_sums(sums, 10)
    assert (per == m).all() and per.shape == (9,)
    assert mean == float(np.mean(m)) and std == float(np.std(m, ddof=0))
    assert abs(std - np.sqrt(np.mean((m - m.mean()) ** 2))) <= 1e-15 * abs(std)
    assert std != float(np.std(m, ddof=1))
    one = KID.kid_from_sums(sums[:1], 10)
    assert one[0] == m[0] and one[1] == 0.0


def test_subset_size_is_lowered_to_the_smaller_set_and_needs_two():
    assert KID.subset_size(30000, 30000, 1000) == 1000
    assert KID.subset_size(12, 30000, 1000) == 12 and KID.subset_size(30000, 12, 1000) == 12
    assert KID.subset_size(12, 12, 8) == 8 and KID.subset_size(2, 2) == 2
    for bad in ((1, 30, 1000), (30, 1, 1000), (30, 30, 1), (0, 0, 1000)):
        with pytest.raises(ValueError, match="2 codes at least"):
            KID.subset_size(*bad)
    assert (KID.SUBSETS, KID.SUBSET_SIZE, KID.DEGREE, KID.COEF0) == (100, 1000, 3, 1.0)


# ------------------------------------------------------------------------------------------------- the command line
def test_kid_parses_with_its_options():
    a = entry.parse_args(["--kid"])
    assert a.kid and not a.fid and a.kid_subsets == 100 and a.kid_subset_size == 1000
    a = entry.parse_args(["--kid", "--kid_subsets", "7", "--kid_subset_size", "33"])
    assert a.kid and a.kid_subsets == 7 and a.kid_subset_size == 33
    a = entry.parse_args(["--fid", "--kid", "--fid_stats", "s.npz"])
    assert a.fid and a.kid and a.fid_stats == "s.npz"
    a = entry.parse_args(["--fid"])
    assert a.fid and not a.kid


@pytest.mark.parametrize("other", ["--sampling", "--r_precision"])
def test_kid_excludes_sampling_and_r_precision(other, capsys):
    for argv in (["--kid", other], ["--fid", "--kid", other]):
        with pytest.raises(SystemExit) as e:
            entry.parse_args(argv)
        assert e.value.code == 2
        err = capsys.readouterr().err
        assert ("--kid cannot be combined with --sampling or --r_precision" in err
                or "--fid cannot be combined with --sampling or --r_precision" in err)
    with pytest.raises(SystemExit):
        entry.parse_args(["--kid", other])
    assert "--kid cannot be combined with --sampling or --r_precision" in capsys.readouterr().err
