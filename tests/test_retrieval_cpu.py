"""The host side of R-precision (attngan/retrieval.py): the mismatched draw, the fold figures, the bank's long-caption rule and
row order -- with a stand-in text encoder on the CPU; none of it needs a GPU."""
import numpy as np
import pytest
import torch

from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import retrieval as R  # noqa: E402


# ------------------------------------------------------------------------------------------------------------ draw_mismatched
def _index(n_img=9, per=5):
    return np.arange(n_img * per) // per


def test_draw_rows_are_distinct_and_never_the_querys_own():
    image_index = _index()
    q = np.array([0, 3, 3, 8, 5])
    t = R.draw_mismatched(image_index, q, 30, np.random.RandomState(1))
    assert t.dtype == np.int32 and t.shape == (5, 30)
    assert t.min() >= 0 and t.max() < len(image_index)
    for row, img in zip(t, q):
        assert len(set(row.tolist())) == 30
        assert not (image_index[row] == img).any()


def test_draw_can_take_every_eligible_row_and_no_more():
    image_index = _index(4, 3)
    t = R.draw_mismatched(image_index, [2], 9, np.random.RandomState(0))
    assert sorted(t[0].tolist()) == [0, 1, 2, 3, 4, 5, 9, 10, 11]
    with pytest.raises(ValueError):
        R.draw_mismatched(image_index, [2], 10, np.random.RandomState(0))
    with pytest.raises(ValueError):                      # the second query is the one without enough rows
        R.draw_mismatched(np.array([0, 1, 1, 1, 2]), [0, 1], 3, np.random.RandomState(0))


def test_draw_same_seed_same_table_and_every_row_reachable():
    image_index = _index(6, 2)
    a = R.draw_mismatched(image_index, [1, 4, 0], 7, np.random.RandomState(42))
    b = R.draw_mismatched(image_index, [1, 4, 0], 7, np.random.RandomState(42))
    c = R.draw_mismatched(image_index, [1, 4, 0], 7, np.random.RandomState(43))
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    rng, seen = np.random.RandomState(5), set()
    for _ in range(200):
        seen |= set(R.draw_mismatched(image_index, [2], 3, rng)[0].tolist())
    assert seen == set(range(12)) - {4, 5}


def test_draw_with_scattered_own_rows():
    image_index = np.array([7, 1, 7, 2, 3, 7, 4])      # the own rows need not be consecutive
    t = R.draw_mismatched(image_index, [7], 4, np.random.RandomState(3))
    assert sorted(t[0].tolist()) == [1, 3, 4, 6]


def test_eligible():
    assert R.eligible(_index(20, 5), 95) and not R.eligible(_index(20, 5), 96)
    assert not R.eligible(np.array([], dtype=np.int64), 1)


# ------------------------------------------------------------------------------------------------------------------ fold_stats
def test_fold_stats_without_remainder():
    ranks = np.array([0, 0, 3, 0,   1, 0, 0, 2,   0, 0, 0, 0])
    out = R.fold_stats(ranks, folds=3)
    f = np.array([0.75, 0.5, 1.0])
    assert out["n"] == 12 and out["folds"] == 3
    assert out["r_precision"] == pytest.approx(9 / 12) and out["mean"] == pytest.approx(f.mean())
    assert out["std"] == pytest.approx(f.std())


def test_fold_stats_drops_the_remainder_from_the_folds_only():
    ranks = np.array([0, 5, 0, 0, 1, 1, 0])            # two folds of three; the last image counts for r_precision alone
    out = R.fold_stats(ranks, folds=2)
    assert out["n"] == 7 and out["r_precision"] == pytest.approx(4 / 7)
    assert out["mean"] == pytest.approx((2 / 3 + 1 / 3) / 2) and out["std"] == pytest.approx(1 / 6)
    few = R.fold_stats(np.array([0, 1]), folds=10)     # fewer images than folds: no fold figures
    assert few["r_precision"] == 0.5 and np.isnan(few["mean"]) and np.isnan(few["std"])


# ------------------------------------------------------------------------------------------------------------ the bank
class BagEncoder(torch.nn.Module):
    """stand-in text encoder: sentence code = sum over the valid tokens of (token, token^2, position * token); checks the contract
    the real one relies on (lengths falling, at most ENCODER_BATCH captions, zero padding, eval mode, no gradients)"""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(1))
        self.calls = []

    def init_hidden(self, bsz):
        return torch.zeros(2, bsz, 1)

    def forward(self, captions, cap_lens, hidden):
        lens = cap_lens.tolist()
        assert not self.training and not torch.is_grad_enabled()
        assert lens == sorted(lens, reverse=True) and len(lens) == captions.shape[0] <= R.ENCODER_BATCH
        assert hidden.shape[1] == captions.shape[0]
        for row, n in zip(captions, lens):
            assert (row[:n] > 0).all() and (row[n:] == 0).all()
        self.calls.append(len(lens))
        c = captions.double()
        pos = torch.arange(captions.shape[1], dtype=torch.float64)
        return None, torch.stack([c.sum(1), (c * c).sum(1), (c * pos).sum(1)], 1).float()


def _captions(n=150, seed=0, longest=30):
    rng = np.random.RandomState(seed)
    return [rng.randint(1, 50, rng.randint(1, longest + 1)).tolist() for _ in range(n)]


def test_fit_caption_keeps_a_sorted_reproducible_subset():
    cap = np.arange(100, 140)
    a = R.fit_caption(cap, 12, np.random.RandomState(9))
    b = R.fit_caption(cap, 12, np.random.RandomState(9))
    c = R.fit_caption(cap, 12, np.random.RandomState(10))
    assert a.dtype == np.int64 and len(a) == 12 and np.array_equal(a, b) and not np.array_equal(a, c)
    assert (np.diff(a) > 0).all() and set(a.tolist()) <= set(cap.tolist())       # the words keep their order
    assert np.array_equal(R.fit_caption(cap[:12], 12, np.random.RandomState(0)), cap[:12])    # a caption that fits is untouched
    assert np.array_equal(R.fit_caption(cap[:3], 12, np.random.RandomState(0)), cap[:3])


def test_bank_rows_follow_the_captions_whatever_the_chunk():
    caps, T = _captions(), 12
    image_index = np.arange(len(caps)) // 5
    enc = BagEncoder().train()
    banks = [R.SentenceBank.build(enc, caps, image_index, T, seed=3, chunk=ch) for ch in (1024, 16, 7, 1)]
    assert enc.training                                   # left in the mode it was found in
    rng = np.random.RandomState(3)
    want = []
    for cap in caps:
        k = R.fit_caption(cap, T, rng).astype(np.float64)
        want.append([k.sum(), (k * k).sum(), (k * np.arange(len(k))).sum()])
    want = torch.tensor(want).float()
    for b in banks:
        assert len(b) == len(caps) and b.bank.dtype == torch.float32 and np.array_equal(b.image_index, image_index)
        assert torch.equal(b.bank, want)
    assert any(len(c) > T for c in caps) and max(enc.calls) == R.ENCODER_BATCH
    other = R.SentenceBank.build(enc, caps, image_index, T, seed=4)
    assert not torch.equal(other.bank, want)              # another seed, other subsets of the long captions
    with pytest.raises(ValueError):
        R.SentenceBank.build(enc, caps, image_index[:-1], T, seed=3)


def test_dataset_adapters():
    from mogan_amd.attngan.datasets import SyntheticTextDataset
    from mogan_amd.attngan.miscc.config import cfg
    ds = SyntheticTextDataset(length=6, n_words=40, seed=2)
    caps, image_index, keys = R.dataset_captions(ds)
    assert len(caps) == 6 and image_index.tolist() == list(range(6)) and keys == ['synthetic_%06d' % i for i in range(6)]
    for i, c in enumerate(caps):
        s = ds[i]
        assert len(c) == s[2] and np.array_equal(c, s[1][:s[2], 0]) and (np.asarray(c) > 0).all()

    class Split:                                          # what the adapter reads of a TextDataset
        embeddings_num = 3
        filenames = ["a", "b"]
        captions = [[1], [2, 2], [3], [4], [5, 5], [6], [7]]          # a trailing caption without an image is left out

    caps, image_index, keys = R.dataset_captions(Split())
    assert caps == Split.captions[:6] and image_index.tolist() == [0, 0, 0, 1, 1, 1] and keys == ["a", "b"]
    bank = R.SentenceBank.from_dataset(BagEncoder(), Split(), cfg.TEXT.WORDS_NUM, seed=0)
    assert bank.images_of(["b", "a", "b"]).tolist() == [1, 0, 1] and len(bank) == 6


# ------------------------------------------------------------------------------------------------------------------ the op
def test_op_checks_a_host_idx_and_has_no_cpu_path():
    from mogan_amd.hip import lib, ops
    code, pos, bank = torch.randn(2, 8), torch.randn(2, 8), torch.randn(5, 8)
    for bad in (np.array([[0, 5], [1, 2]]), np.array([[0, -1], [1, 2]])):
        with pytest.raises(IndexError):
            ops.retrieval_rank(code, pos, bank, bad)
    with pytest.raises(lib.MoganHipError):               # host tensors: there is no CPU path in the product
        ops.retrieval_rank(code, pos, bank, np.array([[0, 4], [1, 2]]))
    with pytest.raises(ValueError):
        ops.retrieval_rank(code, pos[:1], bank, np.array([[0, 4], [1, 2]]))
