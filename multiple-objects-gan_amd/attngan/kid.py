"""Host side of the kernel Inception distance between two sets of Inception pool codes (Binkowski et al.,
"Demystifying MMD GANs", 2018; the reference repository has no code for it).

Two sets of (n, 2048) pooled trunk codes (CNN_ENCODER.pool_code) are compared by the unbiased estimate of the squared maximum
mean discrepancy under the polynomial kernel k(a, b) = (<a, b> / D + 1)^3, averaged over random subset pairs of s codes each:

    mmd2 = sum_{i != j} k(x_i, x_j) / (s (s - 1)) + sum_{i != j} k(y_i, y_j) / (s (s - 1)) - 2 sum_{i, j} k(x_i, y_j) / s^2

The three sums per subset pair come from the device (hip/ops.poly_mmd_sums); this module draws the subsets and forms the figure:

  * `draw_subsets`    the index tables of the subset pairs, from one seeded numpy generator in a documented order;
  * `subset_size`     the subset size a pair of sets allows;
  * `mmd2_from_sums`  the estimator above per subset pair, in fp64, in that order of operations;
  * `kid_from_sums`   its mean and population standard deviation over the subset pairs.
The estimator is unbiased and may be negative: nothing is clamped.  Nothing in this module needs a GPU.
"""
import numpy as np

DEGREE = 3
COEF0 = 1.0
SUBSETS = 100
SUBSET_SIZE = 1000


def subset_size(n_real, n_fake, requested=SUBSET_SIZE):
    """min(requested, n_real, n_fake); ValueError where that leaves fewer than 2 codes (the estimator divides by s - 1)"""
    s = min(int(requested), int(n_real), int(n_fake))
    if s < 2:
        raise ValueError("kid: a subset needs 2 codes at least (requested %d; %d real, %d generated codes)"
                         % (requested, n_real, n_fake))
    return s


def draw_subsets(n_real, n_fake, subsets, subset_size, seed):
    """(ix, iy), int32 (subsets, subset_size) each: rows of the real and of the generated codes, without repeats inside a row.
    ONE numpy.random.RandomState(seed); for k = 0, 1, ... first choice(n_real, subset_size, replace=False) for ix[k], then
    choice(n_fake, subset_size, replace=False) for iy[k].  The order is part of the contract."""
    S, s = int(subsets), int(subset_size)
    if S < 1:
        raise ValueError("draw_subsets: one subset pair at least, got %d" % S)
    if s < 2 or s > n_real or s > n_fake:
        raise ValueError("draw_subsets: subset_size %d outside [2, min(%d, %d)]" % (s, n_real, n_fake))
    rng = np.random.RandomState(seed)
    ix = np.empty((S, s), dtype=np.int32)
    iy = np.empty((S, s), dtype=np.int32)
    for k in range(S):
        ix[k] = rng.choice(n_real, s, replace=False)
        iy[k] = rng.choice(n_fake, s, replace=False)
    return ix, iy


def mmd2_from_sums(sums, s):
    """fp64 (S,): sums[k, 0] / (s (s - 1)) + sums[k, 1] / (s (s - 1)) - 2 sums[k, 2] / s^2 per subset pair, in this order"""
    sums = np.asarray(sums, dtype=np.float64)
    s = int(s)
    if sums.ndim != 2 or sums.shape[1] != 3:
        raise ValueError("mmd2_from_sums: sums (S, 3) expected, got %s" % (sums.shape,))
    if s < 2:
        raise ValueError("mmd2_from_sums: s >= 2 expected, got %d" % s)
    pairs, cross = float(s) * float(s - 1), float(s) * float(s)
    return sums[:, 0] / pairs + sums[:, 1] / pairs - 2.0 * sums[:, 2] / cross


def kid_from_sums(sums, s):
    """(mean, population standard deviation (ddof = 0), the per-subset fp64 array) of mmd2_from_sums"""
    m = mmd2_from_sums(sums, s)
    return float(np.mean(m)), float(np.std(m)), m
