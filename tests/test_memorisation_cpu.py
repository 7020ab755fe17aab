"""attngan/memorisation.py and fid.NeighbourBank on the host: the three figures on examples small enough to compute by hand, the
limits of the Mann-Whitney statistic, the tie and zero-denominator rules of most_suspicious, the ValueErrors, and the bank file's
round trip and wrong-trunk error.  No GPU."""
import os

import numpy as np
import pytest

from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import memorisation as MEM  # noqa: E402
from mogan_amd.attngan.fid import NeighbourBank  # noqa: E402

# a bank of 4 rows whose nearest other rows are at 4, 4, 9 and 1
NN_BANK = np.array([4.0, 4.0, 9.0, 1.0])


def test_authenticity_by_hand():
    # row 0: 3 < 4 no; row 1: 4 >= 4 yes (equality is authentic); row 2: 10 >= 9 yes; row 3: 0.5 < 1 no; row 4: 1 >= 1 yes
    out = MEM.authenticity(np.array([3.0, 4.0, 10.0, 0.5, 1.0]), np.array([0, 1, 2, 3, 3]), NN_BANK)
    assert out == {"authentic": 3, "n": 5, "authenticity": 3 / 5}
    assert MEM.authenticity(np.array([0.0]), np.array([2]), NN_BANK) == {"authentic": 0, "n": 1, "authenticity": 0.0}
    assert MEM.authenticity(np.array([9.0]), np.array([2], dtype=np.int32), NN_BANK)["authenticity"] == 1.0
    # a bank row with a twin (d2_NN = 0): nothing is closer than 0, every code is authentic against it, a copy included
    assert MEM.authenticity(np.array([0.0, 2.0]), np.array([1, 1]), np.array([3.0, 0.0]))["authentic"] == 2


def test_copying_by_hand():
    # f = 1, 2, 5; h = 2, 3: 1 < 2, 1 < 3, 2 = 2, 2 < 3, 5 > 2, 5 > 3 -> less 3, equal 1 of 6 pairs
    out = MEM.copying(np.array([1.0, 2.0, 5.0]), np.array([2.0, 3.0]))
    assert out == {"less": 3, "equal": 1, "pairs": 6, "copying": 7 / 12}
    rng = np.random.RandomState(0)
    f, h = rng.rand(37), rng.rand(23)
    f[:5] = h[:5]                                                    # genuine ties
    brute_less = int((f[:, None] < h[None, :]).sum())
    brute_equal = int((f[:, None] == h[None, :]).sum())
    out = MEM.copying(f, h)
    assert (out["less"], out["equal"], out["pairs"]) == (brute_less, brute_equal, 37 * 23) and brute_equal >= 5
    assert out["copying"] == (2 * brute_less + brute_equal) / (2 * 37 * 23)


def test_copying_is_a_half_for_equal_sets_and_one_for_copies():
    rng = np.random.RandomState(1)
    d = rng.rand(41)
    d[7] = d[8]
    assert MEM.copying(d, d)["copying"] == 0.5                       # exactly: less + greater + equal = pairs, less = greater
    assert MEM.copying(d, d[::-1].copy())["copying"] == 0.5
    assert MEM.copying(np.zeros(9), 1.0 + rng.rand(13))["copying"] == 1.0      # bit copies of bank rows, H away from the bank
    assert MEM.copying(1.0 + rng.rand(13), np.zeros(9))["copying"] == 0.0
    assert MEM.copying(np.zeros(3), np.zeros(4))["copying"] == 0.5


def test_most_suspicious_by_hand_ties_and_zero_denominators():
    bank = np.array([4.0, 2.0, 0.0, 8.0, 0.0])
    #           ratio:  2/4   1/2   3/0   0/0   4/8   0/8   0/0   8/8
    d2 = np.array([2.0, 1.0, 3.0, 0.0, 4.0, 0.0, 0.0, 8.0])
    idx = np.array([0, 1, 2, 2, 3, 3, 4, 3])
    rows, ratio = MEM.most_suspicious(d2, idx, bank, 8)
    # 0 / 0 first (rows 3, 6, by row), then ratio 0 (row 5), the three at 0.5 by row (0, 1, 4), 1 (row 7), x / 0 last as +inf
    assert list(rows) == [3, 6, 5, 0, 1, 4, 7, 2] and rows.dtype == np.int64
    assert list(ratio) == [0.0, 0.0, 0.0, 0.5, 0.5, 0.5, 1.0, np.inf] and ratio.dtype == np.float64
    rows, ratio = MEM.most_suspicious(d2, idx, bank, 3)
    assert list(rows) == [3, 6, 5] and list(ratio) == [0.0, 0.0, 0.0]
    rows, ratio = MEM.most_suspicious(d2, idx, bank, 100)            # m above the number of rows: all of them
    assert len(rows) == 8
    rows, ratio = MEM.most_suspicious(d2, idx, bank, 0)
    assert len(rows) == 0 and len(ratio) == 0


def test_scores_holds_the_three_figures_and_their_counts():
    d2_f, idx_f = np.array([3.0, 4.0, 10.0, 0.5]), np.array([0, 1, 2, 3])
    d2_h, idx_h = np.array([5.0, 1.0, 9.0]), np.array([0, 0, 2])
    out = MEM.scores(d2_f, idx_f, d2_h, idx_h, NN_BANK)
    assert out["authenticity"] == 2 / 4 and out["authentic"] == 2
    assert out["authenticity_heldout"] == 2 / 3 and out["authentic_heldout"] == 2
    c = MEM.copying(d2_f, d2_h)
    assert (out["copying"], out["copying_less"], out["copying_equal"], out["copying_pairs"]) == (c["copying"], c["less"], c["equal"], 12)
    assert set(out) == {"authenticity", "authentic", "authenticity_heldout", "authentic_heldout", "copying", "copying_less",
                        "copying_equal", "copying_pairs"}


def test_value_errors():
    d2, idx = np.array([1.0, 2.0]), np.array([0, 1])
    bad = [
        (np.array([]), np.array([], dtype=np.int64), NN_BANK),       # empty
        (np.ones((2, 2)), np.zeros((2, 2), dtype=np.int64), NN_BANK),    # mis-shaped
        (d2, np.array([0, 1, 2]), NN_BANK), (d2, np.array([[0, 1]]), NN_BANK),
        (d2, np.array([0.0, 1.0]), NN_BANK),                         # positions must be integers
        (d2, np.array([0, 4]), NN_BANK), (d2, np.array([-1, 0]), NN_BANK),    # outside the bank
        (d2, idx, np.array([1.0])), (d2, idx, np.array([])),         # a bank with fewer than 2 rows
        (d2, idx, np.ones((2, 2))),
        (np.array([1.0, -1e-9]), idx, NN_BANK), (np.array([1.0, np.nan]), idx, NN_BANK),
        (d2, idx, np.array([1.0, -2.0, 3.0])), (d2, idx, np.array([1.0, np.nan, 3.0])),
        (np.array([1, 2]), idx, NN_BANK),                            # integer "distances"
    ]
    for a, b, c in bad:
        with pytest.raises(ValueError):
            MEM.authenticity(a, b, c)
        with pytest.raises(ValueError):
            MEM.most_suspicious(a, b, c, 1)
    with pytest.raises(ValueError):
        MEM.most_suspicious(d2, idx, NN_BANK, -1)
    for f, h in ((np.array([]), d2), (d2, np.array([])), (np.ones((2, 2)), d2), (d2, np.array([np.nan])), (np.array([-1.0]), d2),
                 (d2, np.array([1, 2]))):
        with pytest.raises(ValueError):
            MEM.copying(f, h)
    with pytest.raises(ValueError):
        MEM.scores(d2, idx, np.array([np.nan]), np.array([0]), NN_BANK)
    # +inf is a distance (an overflow far away), not an error
    assert MEM.authenticity(np.array([np.inf]), np.array([0]), NN_BANK)["authentic"] == 1


def test_bank_round_trip_and_wrong_trunk(tmp_path):
    rng = np.random.RandomState(3)
    codes = rng.randn(7, 12).astype(np.float32)
    positions = np.array([0, 2, 3, 5, 8, 13, 21])
    bank = NeighbourBank(codes, positions, "a" * 64, "train")
    assert len(bank) == 7
    path = str(tmp_path / "bank.npz")
    bank.save(path)
    assert os.path.isfile(path) and not os.path.exists(path + ".npz")
    back = NeighbourBank.load(path, "a" * 64, 12)
    assert back.codes.dtype == np.float32 and (back.codes.view(np.int32) == codes.view(np.int32)).all()
    assert back.positions.dtype == np.int64 and (back.positions == positions).all()
    assert back.trunk_digest == "a" * 64 and back.split == "train" and len(back) == 7
    with pytest.raises(ValueError, match="another Inception trunk"):
        NeighbourBank.load(path, "b" * 64, 12)
    with pytest.raises(ValueError, match="features"):
        NeighbourBank.load(path, "a" * 64, 2048)
    for c, p in ((codes.astype(np.float64), positions), (codes[0], positions[:1]), (codes, positions[:3]), (codes[:0], positions[:0])):
        with pytest.raises(ValueError):
            NeighbourBank(c, p, "a" * 64, "train")
    import torch
    assert (NeighbourBank(torch.from_numpy(codes), positions, "a" * 64, "train").codes == codes).all()
