"""Host side of the memorisation figures of a generator checkpoint (the reference repository has no code for
it): is the generator reproducing its TRAINING images?  Every other score of attngan/evaluate.py compares the generated images
with the real images of the evaluation split, or with each other, and a generator that has memorised the training set scores well
on all of them.

Three sets of codes: the bank T, the codes of the training images; H, the codes of held-out real images (the evaluation split);
F, the codes of the generated images.  All distances are squared Euclidean distances d2 of codes.  What this module is given:

    d2_f (n_fake,), idx_f (n_fake,)   every generated code's distance to its nearest bank row t* and the position of t*
    d2_h (n_held,), idx_h (n_held,)   the same for every held-out code
    nn_bank (n_bank,)                 every bank row's distance to its nearest OTHER bank row, d2_NN(t)

(on the device: hip/ops.knn_cross(F, T, k), hip/ops.knn_cross(H, T, 1), hip/ops.knn_sqdist(T, 1)).

  * `authenticity` (Alaa et al. 2022, "How Faithful is Your Synthetic Data?"): a generated code f is AUTHENTIC iff
    d2(f, t*) >= d2_NN(t*) -- it is not closer to a training image than that image's own nearest training neighbour.  The figure is
    authentic / n_fake, one division of two integers.  The same figure of H is the data's own value: unseen real images are not
    all authentic either, and a generator need not be more authentic than the data.
  * `copying` (after Meehan et al. 2020, "A Non-Parametric Test to Detect Data-Copying"): the Mann-Whitney statistic
    P(d2(f, T) < d2(h, T)) + 1/2 P(d2(f, T) = d2(h, T)) over all pairs (f, h), from integer counts: (2 less + equal) / (2 n_fake
    n_held), exact in fp64.  0.5: the generated images sit as far from the training set as unseen real images do; towards 1: they
    sit closer -- copying; towards 0: they keep away from it.
  * `most_suspicious`: the generated rows with the smallest ratio d2(f, t*) / d2_NN(t*), ties by row -- the rows of the figure
    "generated images next to their nearest training images".  A ratio with denominator 0 (t* has a twin in the bank) is ordered
    as +inf, unless the numerator is 0 too (f is a copy of both): that row comes first, before every other, with the ratio 0.

All three depend on the size of the bank: a larger bank lies closer to everything.  Pure numpy; nothing here needs a GPU.
"""
import numpy as np


def _distances(who, name, d2):
    d2 = np.asarray(d2)
    if d2.ndim != 1 or d2.size < 1:
        raise ValueError("%s: %s must be a non-empty vector of distances, got shape %s" % (who, name, d2.shape))
    if not np.issubdtype(d2.dtype, np.floating):
        raise ValueError("%s: %s must hold floating-point distances, got %s" % (who, name, d2.dtype))
    d2 = d2.astype(np.float64)
    if np.isnan(d2).any() or (d2 < 0).any():
        raise ValueError("%s: %s holds NaN or negative distances" % (who, name))
    return d2


def _bank(who, nn_bank):
    nn_bank = _distances(who, "nn_bank", nn_bank)
    if nn_bank.size < 2:
        raise ValueError("%s: a bank of %d row has no nearest other row; two at least" % (who, nn_bank.size))
    return nn_bank


def _nearest(who, d2, idx, nn_bank):
    """(d2 (n,) fp64, d2_NN of each row's nearest bank row (n,)) after the checks"""
    d2, nn_bank = _distances(who, "d2", d2), _bank(who, nn_bank)
    idx = np.asarray(idx)
    if idx.shape != d2.shape or not np.issubdtype(idx.dtype, np.integer):
        raise ValueError("%s: idx must be integer positions of shape %s, got %s %s" % (who, d2.shape, idx.dtype, idx.shape))
    if int(idx.min()) < 0 or int(idx.max()) >= nn_bank.size:
        raise ValueError("%s: idx holds positions outside the bank's [0, %d)" % (who, nn_bank.size))
    return d2, nn_bank[idx.astype(np.int64)]


def authenticity(d2, idx, nn_bank):
    """{"authentic": count, "n": rows, "authenticity": count / rows} of a set of codes given each row's nearest bank distance d2
    (n,), that bank row's position idx (n,) and nn_bank (n_bank,)"""
    d2, own = _nearest("authenticity", d2, idx, nn_bank)
    authentic = int((d2 >= own).sum())
    return {"authentic": authentic, "n": int(d2.size), "authenticity": authentic / d2.size}


def copying(d2_f, d2_h):
    """{"less": #{d2_f < d2_h}, "equal": #{d2_f == d2_h}, "pairs": n_fake n_held, "copying": (2 less + equal) / (2 pairs)} over all
    pairs of a generated and a held-out row's nearest bank distance"""
    f, h = _distances("copying", "d2_f", d2_f), np.sort(_distances("copying", "d2_h", d2_h))
    lo, hi = np.searchsorted(h, f, side="left"), np.searchsorted(h, f, side="right")
    less, equal, pairs = int((h.size - hi).sum()), int((hi - lo).sum()), int(f.size) * int(h.size)
    return {"less": less, "equal": equal, "pairs": pairs, "copying": (2 * less + equal) / (2 * pairs)}


def most_suspicious(d2_f, idx_f, nn_bank, m):
    """(rows (m',) int64, ratio (m',) fp64), m' = min(m, n_fake): the generated rows with the smallest d2(f, t*) / d2_NN(t*),
    ascending, ties by row; 0 / 0 first with the ratio 0, another ratio over 0 as +inf (module docstring)"""
    d2, own = _nearest("most_suspicious", d2_f, idx_f, nn_bank)
    m = int(m)
    if m < 0:
        raise ValueError("most_suspicious: m >= 0 expected, got %d" % m)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(own > 0, d2 / own, np.inf)
    twice = (own == 0) & (d2 == 0)
    ratio[twice] = 0.0
    key = np.where(twice, -1.0, ratio)
    rows = np.argsort(key, kind="stable")[:m]
    return rows.astype(np.int64), ratio[rows]


def scores(d2_f, idx_f, d2_h, idx_h, nn_bank):
    """the three figures and the counts behind them, as memorisation.json holds them"""
    a_f, a_h, c = authenticity(d2_f, idx_f, nn_bank), authenticity(d2_h, idx_h, nn_bank), copying(d2_f, d2_h)
    return {"authenticity": a_f["authenticity"], "authentic": a_f["authentic"],
            "authenticity_heldout": a_h["authenticity"], "authentic_heldout": a_h["authentic"],
            "copying": c["copying"], "copying_less": c["less"], "copying_equal": c["equal"], "copying_pairs": c["pairs"]}
