"""Host side of precision / recall / density / coverage (attngan/prdc.py) and its command line (attngan/main.py), without a GPU:
the choice of the k's, the four figures on hand-made counts and on sets whose scores are known in closed form, and the --prdc options."""
import numpy as np
import pytest

import prdc_cases as P
from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import main as entry  # noqa: E402
from mogan_amd.attngan import prdc as PRDC  # noqa: E402


# ------------------------------------------------------------------------------------------------- neighbours
def test_the_constants_and_the_lowering_of_k():
    assert (PRDC.K_PR, PRDC.K_DC, PRDC.K_MAX) == (3, 5, 8)
    assert PRDC.neighbours(30000, 30000) == (3, 5)
    assert PRDC.neighbours(30000, 30000, 3, 5) == (3, 5) and PRDC.neighbours(30000, 30000, 8, 1) == (8, 1)
    assert PRDC.neighbours(6, 30000) == (3, 5) and PRDC.neighbours(5, 30000) == (3, 4) and PRDC.neighbours(30000, 5) == (3, 4)
    assert PRDC.neighbours(4, 4) == (3, 3) and PRDC.neighbours(3, 9) == (2, 2) and PRDC.neighbours(2, 2) == (1, 1)
    assert PRDC.neighbours(12, 12, 3, 5) == (3, 5)
    for bad in ((1, 30), (30, 1), (0, 0)):
        with pytest.raises(ValueError, match="2 codes at least"):
            PRDC.neighbours(*bad)
    for k_pr, k_dc in ((0, 5), (3, 0), (-1, 5), (9, 5), (3, 9)):
        with pytest.raises(ValueError, match=r"outside \[1, 8\]"):
            PRDC.neighbours(100, 100, k_pr, k_dc)


# ------------------------------------------------------------------------------------------------- the four figures
def test_scores_on_hand_made_counts():
    """4 generated and 5 real codes, k_dc = 2.  fake_in_real: column 0 (k_pr) holds 0, 2, 0, 1 -> 2 of 4 inside some ball; column 1
    (k_dc) sums to 0 + 3 + 1 + 2 = 6 -> 6 / (2 * 4).  real_in_fake 0, 0, 1, 4, 0 -> 2 of 5.  real_own 1, 0, 2, 5, 0 -> 3 of 5."""
    f = np.array([[0, 0], [2, 3], [0, 1], [1, 2]], dtype=np.int32)
    s = PRDC.scores_from_counts(f, np.array([0, 0, 1, 4, 0], dtype=np.int32), np.array([1, 0, 2, 5, 0], dtype=np.int32), 2)
    assert s == {"precision": 0.5, "recall": 0.4, "density": 0.75, "coverage": 0.6}
    assert all(type(v) is float for v in s.values())
    # density is a mean count over k, not a share: above 1 where the balls overlap over the generated codes
    s = PRDC.scores_from_counts(np.array([[5, 7], [5, 8]]), np.array([1, 1, 1]), np.array([2, 2, 2]), 5)
    assert s == {"precision": 1.0, "recall": 1.0, "density": 1.5, "coverage": 1.0}
    s = PRDC.scores_from_counts(np.zeros((3, 2), dtype=np.int64), np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int64), 5)
    assert s == {"precision": 0.0, "recall": 0.0, "density": 0.0, "coverage": 0.0}
    # one division each: the exact quotient of the integers
    f = np.ones((7, 2), dtype=np.int32)
    f[:4, 0] = 0
    s = PRDC.scores_from_counts(f, np.array([1, 0, 0]), np.array([0, 1, 1]), 3)
    assert s == {"precision": 3 / 7, "recall": 1 / 3, "density": 7 / 21, "coverage": 2 / 3}


def test_scores_reject_what_are_not_counts():
    f, r, o = np.zeros((4, 2), dtype=np.int32), np.zeros(5, dtype=np.int32), np.zeros(5, dtype=np.int32)
    PRDC.scores_from_counts(f, r, o, 5)
    for bad in ((f[:, 0], r, o), (np.zeros((4, 3), dtype=np.int32), r, o), (f.astype(np.float64), r, o), (f, r[:, None], o),
                (f, r, o[:4]), (f, r.astype(np.float32), o), (f - 1, r, o), (f, r, o - 1), (f[:0], r, o), (f, r[:0], o[:0])):
        with pytest.raises(ValueError):
            PRDC.scores_from_counts(*bad, k_dc=5)
    with pytest.raises(ValueError):
        PRDC.scores_from_counts(f, r, o, 0)


@pytest.mark.parametrize("n,D", [(12, 16), (40, 64)], ids=str)
def test_identical_sets_score_one(n, D):
    """fake = real: every code lies in its own copy's ball (d2 = 0 <= r2), so precision = recall = coverage = 1; a ball of the k-th
    neighbour's radius holds its centre's copy and k others, so the memberships number n (k_dc + 1) from either side and density is
    (k_dc + 1) / k_dc > 1.  Taken with the oracle's distances, which are bitwise symmetric: the radius IS one of the distances."""
    x = P.fid_cases.fd_pair((D, n, 2), 4)[0]
    k_pr, k_dc = PRDC.neighbours(n, n)
    f, r, o = P.prdc_counts(x, x.copy(), k_pr, k_dc, d2=lambda a, b: P.oracle_d2(a, b)[0])
    assert (f[:, 0] >= 1).all() and (r >= 1).all()
    assert (o == k_dc + 1).all()                                     # a ball of the k-th neighbour's radius holds itself and k others
    assert int(f[:, 1].sum()) == n * (k_dc + 1)                      # the same memberships, counted from the other side
    s = PRDC.scores_from_counts(f, r, o, k_dc)
    assert s["precision"] == s["recall"] == s["coverage"] == 1.0 and s["density"] == (k_dc + 1) / k_dc
    got = P.prdc_numpy(x, x.copy(), k_pr, k_dc)                      # fp64 Gram form: a radius may tie with itself either way
    assert got["precision"] == got["recall"] == got["coverage"] == 1.0 and got["density"] >= 1.0


def test_far_apart_sets_score_zero():
    """two clouds of spread ~1 whose centres are 1000 apart in every feature: no ball of one reaches the other"""
    rng = np.random.RandomState(3)
    real = rng.standard_normal((30, 24)).astype(np.float32)
    fake = (rng.standard_normal((25, 24)) + 1000.0).astype(np.float32)
    assert P.prdc_numpy(real, fake, 3, 5) == {"precision": 0.0, "recall": 0.0, "density": 0.0, "coverage": 0.0}


def test_collapsed_and_sloppy_generators_are_told_apart():
    """what the scores are for: a generator that repeats one good image has precision 1 and recall near 0; one that scatters far
    beyond the data has recall high and precision low"""
    rng = np.random.RandomState(5)
    real = rng.standard_normal((60, 8)).astype(np.float32)
    collapsed = np.repeat(real[:1], 60, axis=0) + np.float32(1e-3) * rng.standard_normal((60, 8)).astype(np.float32)
    sloppy = (6.0 * rng.standard_normal((60, 8))).astype(np.float32)
    c, s = P.prdc_numpy(real, collapsed, 3, 5), P.prdc_numpy(real, sloppy, 3, 5)
    print("collapsed %s\nsloppy    %s" % (c, s))
    assert c["precision"] == 1.0 and c["recall"] <= 0.05 and c["coverage"] <= 0.1
    assert s["precision"] <= 0.3 and s["recall"] >= 0.5


def test_prdc_counts_agree_with_the_oracle_on_a_case():
    """the numpy fp64 evaluation the end-to-end test leans on decides like the longdouble oracle where the margins hold"""
    case = (67, 100, 80, 5)
    ref = P.reference(case)
    real, fake = ref["x"], ref["y"]
    assert P.prdc_margin(real, fake, 3, 5) >= P.MARGIN
    f, r, o = P.prdc_counts(real, fake, 3, 5)
    fl, rl, ol = P.prdc_counts(real, fake, 3, 5, d2=lambda a, b: P.oracle_d2(a, b)[0])
    assert (f == fl).all() and (r == rl).all() and (o == ol).all()
    assert 0 < f[:, 0].astype(bool).mean() < 1 and 0 < o.astype(bool).mean() <= 1


# ------------------------------------------------------------------------------------------------- the command line
def test_prdc_parses_with_its_options():
    a = entry.parse_args(["--prdc"])
    assert a.prdc and not a.fid and not a.kid and a.prdc_k_pr == 3 and a.prdc_k_dc == 5
    a = entry.parse_args(["--prdc", "--prdc_k_pr", "2", "--prdc_k_dc", "7"])
    assert a.prdc and a.prdc_k_pr == 2 and a.prdc_k_dc == 7
    a = entry.parse_args(["--fid", "--kid", "--prdc", "--fid_stats", "s.npz"])
    assert a.fid and a.kid and a.prdc and a.fid_stats == "s.npz"
    a = entry.parse_args(["--fid", "--kid"])
    assert a.fid and a.kid and not a.prdc
    assert not entry.parse_args([]).prdc


@pytest.mark.parametrize("other", ["--sampling", "--r_precision"])
def test_prdc_excludes_sampling_and_r_precision(other, capsys):
    with pytest.raises(SystemExit) as e:
        entry.parse_args(["--prdc", other])
    assert e.value.code == 2
    assert "--prdc cannot be combined with --sampling or --r_precision" in capsys.readouterr().err
    for argv in (["--fid", "--prdc", other], ["--kid", "--prdc", other], ["--fid", "--kid", "--prdc", other]):
        with pytest.raises(SystemExit) as e:
            entry.parse_args(argv)
        assert e.value.code == 2
        assert "cannot be combined with --sampling or --r_precision" in capsys.readouterr().err
