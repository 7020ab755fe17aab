"""The host side of the Frechet distance (attngan/fid.py, main.py --fid): closed forms, symmetry, shifts, the statistics file and
the command line.  None of it needs a GPU.  Bounds: fid_cases.FD_TOL / FD_SELF_TOL (measured by tests/test_fid_reference_cpu.py) where
they apply, otherwise from the precision of fp64 as written next to each."""
import numpy as np
import pytest
import torch

import fid_cases as K
from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import fid as F  # noqa: E402

EPS = 2.0 ** -52


def _commuting(a, b, seed=0):
    D = len(a)
    Q, _ = np.linalg.qr(np.random.RandomState(seed).standard_normal((D, D)))
    return (Q * np.asarray(a)) @ Q.T, (Q * np.asarray(b)) @ Q.T


# ------------------------------------------------------------------------------------------------------------ closed forms
def test_commuting_covariances_full_rank():
    """S1 = Q diag(a) Q^T, S2 = Q diag(b) Q^T: Tr (S1 S2)^(1/2) = sum sqrt(a_i b_i).  Each of the D eigenvalues of a symmetric
    eigen-decomposition carries a backward error of a few units of 2^-52 |S|; with a, b in [0.5, 2] a square root halves relative
    errors: 4 D 2^-52 (Tr S1 + Tr S2) covers the two decompositions and the products between them."""
    rng = np.random.RandomState(1)
    D = 24
    a, b = rng.uniform(0.5, 2.0, D), rng.uniform(0.5, 2.0, D)
    S1, S2 = _commuting(a, b)
    mu1, mu2 = rng.standard_normal(D), rng.standard_normal(D)
    d, t = F.frechet_distance(mu1, S1, mu2, S2)
    bound = 4 * D * EPS * (a.sum() + b.sum())
    assert t["tr_sqrt"] == pytest.approx(np.sqrt(a * b).sum(), abs=bound)
    assert t["mean_sq"] == pytest.approx(((mu1 - mu2) ** 2).sum(), rel=1e-14)
    assert t["tr_s1"] == pytest.approx(a.sum(), rel=1e-14) and t["tr_s2"] == pytest.approx(b.sum(), rel=1e-14)
    assert d == t["mean_sq"] + t["tr_s1"] + t["tr_s2"] - 2.0 * t["tr_sqrt"]
    assert isinstance(d, float) and set(t) == {"mean_sq", "tr_s1", "tr_s2", "tr_sqrt"}


def test_commuting_covariances_rank_deficient():
    """some a_i = 0 (and one b_i = 0): the product's zero eigenvalues come out as rounding noise of the order D 2^-52 |S1| |S2|
    around 0 -- the negative ones are clamped, the positive ones enter through a square root.  k zero eigenvalues therefore
    contribute k sqrt(D 2^-52 max a max b) at most; the others as in the full-rank case."""
    rng = np.random.RandomState(2)
    D = 24
    a, b = rng.uniform(0.5, 2.0, D), rng.uniform(0.5, 2.0, D)
    a[[0, 5, 6, 17]] = 0.0
    b[[5, 9]] = 0.0
    S1, S2 = _commuting(a, b, seed=3)
    d, t = F.frechet_distance(np.zeros(D), S1, np.zeros(D), S2)
    k = int(((a == 0) | (b == 0)).sum())
    bound = 4 * D * EPS * (a.sum() + b.sum()) + k * np.sqrt(D * EPS * a.max() * b.max())
    print("rank-deficient closed form: off by %.3e (bound %.3e)" % (abs(t["tr_sqrt"] - np.sqrt(a * b).sum()), bound))
    assert np.isfinite(d) and t["tr_sqrt"] == pytest.approx(np.sqrt(a * b).sum(), abs=bound)
    # a zero covariance on one side: the distance is the other side's trace
    d0, t0 = F.frechet_distance(np.zeros(D), np.zeros((D, D)), np.zeros(D), S2)
    assert t0["tr_sqrt"] == 0.0 and d0 == pytest.approx(b.sum(), rel=1e-14)


def _full_rank_stats():
    x1, x2 = K.fd_pair((64, 200, 300), K.FD_CASES[(64, 200, 300)])
    return [torch.from_numpy(v) for v in K.stats64(x1)], [torch.from_numpy(v) for v in K.stats64(x2)]


def test_identical_inputs_and_symmetry():
    a, b = _full_rank_stats()
    d0, t0 = F.frechet_distance(*a, *a)
    assert t0["mean_sq"] == 0.0 and abs(d0) <= K.FD_SELF_TOL * 2.0 * t0["tr_s1"]          # measured, not assumed to be 0
    dab, tab = F.frechet_distance(*a, *b)
    dba, tba = F.frechet_distance(*b, *a)
    assert tab["tr_s1"] == tba["tr_s2"] and tab["tr_s2"] == tba["tr_s1"] and tab["mean_sq"] == tba["mean_sq"]
    assert abs(dab - dba) <= 2 * K.FD_TOL * abs(dab)                 # each is within FD_TOL of the same number
    # numpy arrays and torch tensors, fp32 stats widened: the same function
    dn, _ = F.frechet_distance(a[0].numpy(), a[1].numpy(), b[0].numpy(), b[1].numpy())
    assert dn == dab


def test_shifts():
    """a common shift of both sets leaves every term alone (the covariance terms bit for bit: they never see the means); a shift of
    one set moves |mu1 - mu2|^2 only"""
    a, b = _full_rank_stats()
    d, t = F.frechet_distance(*a, *b)
    c = torch.from_numpy(np.random.RandomState(0).randint(-4, 5, 64).astype(np.float64))
    ds, ts = F.frechet_distance(a[0] + c, a[1], b[0] + c, b[1])
    assert (ts["tr_s1"], ts["tr_s2"], ts["tr_sqrt"]) == (t["tr_s1"], t["tr_s2"], t["tr_sqrt"])
    assert ts["mean_sq"] == pytest.approx(t["mean_sq"], rel=1e-13)
    d1, t1 = F.frechet_distance(a[0] + c, a[1], b[0], b[1])
    assert (t1["tr_s1"], t1["tr_s2"], t1["tr_sqrt"]) == (t["tr_s1"], t["tr_s2"], t["tr_sqrt"])
    assert t1["mean_sq"] == pytest.approx(float(((a[0] + c - b[0]) ** 2).sum()), rel=1e-14)
    assert d1 - d == pytest.approx(t1["mean_sq"] - t["mean_sq"], rel=1e-12)
    # the same on the codes themselves: moments of shifted codes, an integer shift that fp32 takes exactly
    x1, x2 = K.fd_pair((16, 40, 50), 0)
    x1, x2 = np.round(x1 * 64) / 64, np.round(x2 * 64) / 64
    base, tb = F.frechet_distance(*K.stats64(x1), *K.stats64(x2))
    both, tc = F.frechet_distance(*K.stats64(x1 + np.float32(3)), *K.stats64(x2 + np.float32(3)))
    assert both == pytest.approx(base, rel=1e-12) and tc["tr_sqrt"] == pytest.approx(tb["tr_sqrt"], rel=1e-12)


def test_shape_errors():
    with pytest.raises(ValueError):
        F.frechet_distance(np.zeros(3), np.eye(3), np.zeros(4), np.eye(4))
    with pytest.raises(ValueError):
        F.frechet_distance(np.zeros(3), np.eye(4), np.zeros(3), np.eye(3))


# ------------------------------------------------------------------------------------------------------------ the statistics file
class TinyEncoder(torch.nn.Module):
    HEADS = ("emb_features", "emb_cnn_code")

    def __init__(self):
        super().__init__()
        self.Conv2d_1a_3x3 = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3, bias=False), torch.nn.BatchNorm2d(4))
        self.emb_features = torch.nn.Conv2d(4, 2, 1, bias=False)
        self.emb_cnn_code = torch.nn.Linear(4, 2)


def test_trunk_digest_covers_the_trunk_and_only_the_trunk():
    torch.manual_seed(0)
    enc = TinyEncoder()
    d0 = F.trunk_digest(enc)
    assert len(d0) == 64 and F.trunk_digest(enc) == d0
    with torch.no_grad():
        enc.emb_cnn_code.weight.add_(1.0)                       # a head: not part of it
        enc.emb_features.weight.mul_(2.0)
    assert F.trunk_digest(enc) == d0
    with torch.no_grad():
        enc.Conv2d_1a_3x3[1].running_var[2] += 0.5              # a buffer of the trunk
    d1 = F.trunk_digest(enc)
    assert d1 != d0
    with torch.no_grad():
        enc.Conv2d_1a_3x3[0].weight[0, 0, 0, 0] += 2.0 ** -20   # one parameter, one bit pattern
    assert F.trunk_digest(enc) not in (d0, d1)


def test_feature_stats_round_trip_and_refusals(tmp_path):
    x = K.make_inputs((40, 6), 0)
    mean, cov = K.stats64(x)
    st = F.FeatureStats(mean, cov, 40, "ab" * 32)
    path = str(tmp_path / "stats.npz")
    st.save(path)
    with np.load(path) as z:
        assert z["mean"].dtype == np.float64 and z["cov"].dtype == np.float64 and sorted(z.files) == ["cov", "mean", "n", "trunk_digest"]
    back = F.FeatureStats.load(path, "ab" * 32, 6)
    assert back.n == 40 and back.trunk_digest == "ab" * 32
    assert np.array_equal(back.mean.numpy(), mean) and np.array_equal(back.cov.numpy(), cov)
    with pytest.raises(ValueError, match="another Inception trunk"):
        F.FeatureStats.load(path, "cd" * 32, 6)
    with pytest.raises(ValueError, match="features"):
        F.FeatureStats.load(path, "ab" * 32, 2048)
    with pytest.raises(ValueError):
        F.FeatureStats(mean, cov[:5], 40, "ab" * 32)


# ------------------------------------------------------------------------------------------------------------ the command line
def test_fid_flag_is_parsed_and_excludes_the_other_modes(capsys):
    from mogan_amd.attngan import main as entry
    args = entry.parse_args(["--fid"])
    assert args.fid is True and args.fid_stats is None and not args.sampling and not args.r_precision
    args = entry.parse_args(["--fid", "--fid_stats", "real.npz"])
    assert args.fid and args.fid_stats == "real.npz"
    assert entry.parse_args([]).fid is False
    for other in ("--sampling", "--r_precision"):
        with pytest.raises(SystemExit):
            entry.parse_args(["--fid", other])
        assert "--fid cannot be combined" in capsys.readouterr().err
    both = entry.parse_args(["--sampling", "--r_precision"])            # (as before: not this change's business)
    assert both.sampling and both.r_precision
