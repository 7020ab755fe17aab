"""The definition of the Inception Score (attngan/inception_score.py) on the host: figures whose value is known in
closed form, the split rule, the lowering of S, the population standard deviation, the marginals' KL divergence, the head reader."""
import math

import numpy as np
import pytest
import torch

from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import inception_score as IS  # noqa: E402


def _codes_for_logits(z):
    """codes, weight, bias under which the logits are exactly z (n, C): D = C, the head is the identity"""
    z = np.asarray(z, dtype=np.float32)
    return z, np.eye(z.shape[1], dtype=np.float32), np.zeros(z.shape[1], dtype=np.float32)


def test_equal_logits_give_a_score_of_one():
    for C in (1, 2, 7, 1000):
        out = IS.score(*_codes_for_logits(np.full((23, C), 0.75)), splits=4)
        assert out["splits"] == 4 and len(out["per_split"]) == 4
        for v in out["per_split"] + [out["inception_score"], out["inception_score_all"]]:
            assert abs(v - 1.0) <= 1e-12
        assert out["inception_score_std"] <= 1e-12
    # one class: exactly
    out = IS.score(np.random.RandomState(0).rand(9, 5).astype(np.float32), np.ones((1, 5), np.float32), np.ones(1, np.float32), 3)
    assert out["per_split"] == [1.0, 1.0, 1.0] and out["inception_score"] == 1.0 and out["inception_score_std"] == 0.0


@pytest.mark.parametrize("C", (2, 5, 10))
def test_one_hot_rows_cycling_through_the_classes_give_the_number_of_classes(C):
    S, per = 3, 4 * C                                                  # every split holds each class four times
    z = np.full((S * per, C), -400.0, dtype=np.float32)
    z[np.arange(S * per), np.arange(S * per) % C] = 400.0              # exp(-800) is exactly 0: one-hot rows
    out = IS.score(*_codes_for_logits(z), splits=S)
    for v in out["per_split"] + [out["inception_score"], out["inception_score_all"]]:
        assert abs(v - C) <= 1e-12 * C
    assert out["inception_score_std"] <= 1e-12 * C


def test_the_split_bounds():
    want = {(10, 3): [(0, 3), (3, 6), (6, 10)], (11, 3): [(0, 3), (3, 7), (7, 11)], (19, 3): [(0, 6), (6, 12), (12, 19)],
            (10, 10): [(i, i + 1) for i in range(10)],
            (11, 10): [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7), (7, 8), (8, 9), (9, 11)],
            (19, 10): [(0, 1), (1, 3), (3, 5), (5, 7), (7, 9), (9, 11), (11, 13), (13, 15), (15, 17), (17, 19)]}
    for (n, S), bounds in want.items():
        assert IS.split_bounds(n, S) == bounds, (n, S)
    for n, S in ((30000, 10), (12, 5), (130, 3), (1, 1), (65535, 65535)):
        b = IS.split_bounds(n, S)
        assert b[0][0] == 0 and b[-1][1] == n and all(b[i][1] == b[i + 1][0] for i in range(S - 1))
        assert all(n // S <= hi - lo <= -(-n // S) for lo, hi in b)
    for n, S in ((3, 4), (3, 0), (0, 1)):
        with pytest.raises(ValueError):
            IS.split_bounds(n, S)


def test_the_number_of_splits_is_lowered_to_the_number_of_rows():
    assert IS.effective_splits(30000) == 10 and IS.effective_splits(7) == 7 and IS.effective_splits(7, 3) == 3
    assert IS.effective_splits(1, 10) == 1
    for n, S in ((0, 10), (5, 0)):
        with pytest.raises(ValueError):
            IS.effective_splits(n, S)
    rng = np.random.RandomState(1)
    x, w, b = rng.rand(4, 6).astype(np.float32), rng.randn(3, 6).astype(np.float32), rng.randn(3).astype(np.float32)
    out = IS.score(x, w, b)                                            # ten asked for, four rows
    assert out["splits"] == 4 and all(abs(v - 1.0) <= 1e-14 for v in out["per_split"])       # a split of one row: p = pbar, KL = 0
    assert out["inception_score_all"] > 1.0


def test_the_standard_deviation_is_the_populations():
    rng = np.random.RandomState(2)
    x, w, b = rng.rand(40, 8).astype(np.float32), (3 * rng.randn(5, 8)).astype(np.float32), rng.randn(5).astype(np.float32)
    out = IS.score(x, w, b, splits=4)
    assert len(set(out["per_split"])) == 4
    assert abs(out["inception_score"] - np.mean(out["per_split"])) <= 1e-15 * out["inception_score"]
    assert abs(out["inception_score_std"] - np.std(out["per_split"])) <= 1e-14                    # ddof = 0, as the original code
    assert abs(out["inception_score_std"] - np.std(out["per_split"], ddof=1)) > 1e-6
    # the figures against the textbook formula, split by split
    z = x.astype(np.float64) @ w.astype(np.float64).T + b.astype(np.float64)
    p = np.exp(z - z.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    for (lo, hi), got in zip(IS.split_bounds(40, 4), out["per_split"]):
        q = p[lo:hi]
        kl = (q * (np.log(q) - np.log(q.mean(axis=0, keepdims=True)))).sum(axis=1).mean()
        assert abs(got - math.exp(kl)) <= 1e-12 * got
    q = p.mean(axis=0, keepdims=True)
    assert abs(out["inception_score_all"] - math.exp((p * (np.log(p) - np.log(q))).sum(axis=1).mean())) <= 1e-12 * out["inception_score_all"]


def test_from_sums_takes_what_the_device_hands_over():
    rng = np.random.RandomState(3)
    x, w, b = rng.rand(19, 8).astype(np.float32), rng.randn(6, 8).astype(np.float32), rng.randn(6).astype(np.float32)
    lse, h, p = IS.row_sums(x, w, b)
    assert np.all(np.abs(p.sum(axis=1) - 1.0) <= 1e-14) and np.all(h <= 0.0) and np.all(h >= -math.log(6) - 1e-14)
    psum = IS.split_sums(p, 19, 3)
    assert psum.shape == (3, 6) and np.all(np.abs(psum.sum(axis=1) - np.array([6, 6, 7])) <= 1e-13)
    assert IS.finish(h, psum, 19) == IS.score(x, w, b, 3)
    assert np.all(np.abs(IS.all_rows(psum)[0] - p.sum(axis=0)) <= 1e-14)
    for bad in ((h[:5], psum, 19), (h, psum[0], 19), (h, np.zeros((20, 6)), 19)):
        with pytest.raises(ValueError):
            IS.from_sums(*bad)


def test_the_marginals_divergence():
    rng = np.random.RandomState(4)
    a = rng.rand(1, 9) * 30
    assert IS.kl_marginals(a, 30, a, 30) == 0.0
    assert IS.kl_marginals(a, 30, 2 * a, 60) == 0.0                     # the marginals, not the sums
    b = rng.rand(1, 9) * 30
    pa, pb = a[0] / 30, b[0] / 30
    assert abs(IS.kl_marginals(a, 30, b, 30) - float((pa * (np.log(pa) - np.log(pb))).sum())) <= 1e-13
    zero = a.copy()
    zero[0, 3] = 0.0
    assert math.isfinite(IS.kl_marginals(zero, 30, a, 30)) and IS.kl_marginals(a, 30, zero, 30) == float("inf")
    with pytest.raises(ValueError):
        IS.kl_marginals(a, 30, a[:, :5], 30)


def test_the_head_reader_and_its_digest():
    w, b = torch.randn(7, 12), torch.randn(7)
    got = IS.read_head({"fc.weight": w, "fc.bias": b, "Conv2d_1a_3x3.conv.weight": torch.zeros(1)})
    assert np.array_equal(got[0], w.numpy()) and np.array_equal(got[1], b.numpy())
    assert IS.read_head({"emb_cnn_code.weight": w}) is None
    for bad in ({"fc.weight": w}, {"fc.bias": b}, {"fc.weight": w, "fc.bias": b[:5]}, {"fc.weight": w.double(), "fc.bias": b.double()},
                {"fc.weight": w[0], "fc.bias": b}):
        with pytest.raises(ValueError):
            IS.read_head(bad)
    d = IS.head_digest(*got)
    assert len(d) == 64 and d == IS.head_digest(w.numpy().copy(), b.numpy().copy())
    w2 = w.numpy().copy()
    w2[3, 4] = np.nextafter(w2[3, 4], np.float32(9))
    assert IS.head_digest(w2, b.numpy()) != d and IS.head_digest(w.numpy(), b.numpy()[::-1].copy()) != d


def test_the_mode_is_refused_beside_the_others():
    from mogan_amd.attngan import main as entry
    from mogan_amd.attngan.evaluate import SCORES
    assert "inception_score" not in SCORES
    for flag in ["sampling", "r_precision", "layout_shift"] + list(SCORES):
        with pytest.raises(SystemExit):
            entry.parse_args(["--inception_score", "--" + flag])
    with pytest.raises(SystemExit):
        entry.parse_args(["--inception_score", "--is_splits", "0"])
    args = entry.parse_args(["--inception_score", "--is_head", "h.pth", "--trunk", "t.pth"])
    assert (args.is_head, args.trunk, args.is_splits, args.is_real) == ("h.pth", "t.pth", 10, False)
    assert entry.parse_args([]).trunk is None and not entry.parse_args([]).inception_score


def test_a_trunk_file_is_refused_beside_training(tmp_path):
    from mogan_amd.attngan import main as entry
    from mogan_amd.attngan.miscc.config import cfg
    yml = tmp_path / "train.yml"
    yml.write_text("TRAIN: {FLAG: True}\n")
    try:
        with pytest.raises(SystemExit, match="evaluation flag"):
            entry.main(["--cfg", str(yml), "--trunk", str(tmp_path / "inception_v3.pth")])
    finally:
        cfg.TRAIN.FLAG = True
