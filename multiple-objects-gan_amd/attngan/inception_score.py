"""The Inception Score of a set of Inception pool codes under a classifier head (Salimans et al., "Improved
Techniques for Training GANs", 2016; the reference repository has no code for it).  This module is the definition, in pure numpy;
nothing in it needs a GPU.

For n pool codes x_i (fp32, D = 2048; CNN_ENCODER.pool_code) and a head W (C, D), b (C), both fp32 (torchvision's `fc`: C = 1000):

    z_i     = W x_i + b                        in fp64
    log p_i = z_i - lse(z_i)                   lse with the maximum subtracted
    h_i     = sum_y p_iy log p_iy              (0 log 0 = 0)

The n rows, in the order of the pass, are cut into S contiguous splits [floor(s n / S), floor((s + 1) n / S)) (S = 10 by default,
lowered to n where n < S), and per split

    pbar_s  = mean of p_i over the split
    IS_s    = exp(mean_i h_i - sum_y pbar_sy log pbar_sy)          = exp of the mean KL(p_i || pbar_s)

`inception_score` is the mean of IS_s, `inception_score_std` their population standard deviation (numpy.std, as the original code),
`inception_score_all` the S = 1 figure.  On the device the three sums -- h_i per row, sum_i p_i per split -- come from
hip/ops.softmax_head_sums in one call; `from_sums` finishes the figures from them with math.fsum, and `score` is the same thing from
the codes on the host:

  * `split_bounds`   the split rule, which the kernel's header states too;
  * `effective_splits`  S lowered to n;
  * `row_sums`       (row_lse, row_h, p) of codes under a head, numpy fp64;
  * `from_sums`      the figures from row_h and psum;
  * `score`          row_sums + from_sums;
  * `kl_marginals`   KL(pbar_a || pbar_b) of two sides' all-row marginals;
  * `read_head`, `head_digest`   a head out of a state dict, and the SHA-256 of its two tensors.
"""
import hashlib
import math

import numpy as np

SPLITS = 10
HEAD_KEYS = ("fc.weight", "fc.bias")


def effective_splits(n, splits=SPLITS):
    """min(splits, n); ValueError where that is below 1"""
    n, splits = int(n), int(splits)
    if n < 1 or splits < 1:
        raise ValueError("inception_score: one row and one split at least, got n = %d, splits = %d" % (n, splits))
    return min(splits, n)


def split_bounds(n, splits):
    """[(lo, hi)] of the S contiguous splits of n rows: lo = floor(s n / S), hi = floor((s + 1) n / S); 1 <= S <= n"""
    n, S = int(n), int(splits)
    if S < 1 or S > n:
        raise ValueError("split_bounds: 1 <= splits <= n expected, got splits = %d, n = %d" % (S, n))
    return [(s * n // S, (s + 1) * n // S) for s in range(S)]


def row_sums(codes, weight, bias):
    """(row_lse (n), row_h (n), p (n, C)) in numpy fp64 of fp32 codes (n, D) under the head weight (C, D), bias (C)"""
    x = np.asarray(codes, dtype=np.float32).astype(np.float64)
    w = np.asarray(weight, dtype=np.float32).astype(np.float64)
    b = np.asarray(bias, dtype=np.float32).astype(np.float64)
    if x.ndim != 2 or w.ndim != 2 or b.ndim != 1 or x.shape[1] != w.shape[1] or w.shape[0] != b.shape[0] or w.shape[0] < 1:
        raise ValueError("inception_score: codes (n, D), weight (C, D), bias (C) expected, got %s, %s, %s" % (x.shape, w.shape, b.shape))
    return row_sums_of_logits(x @ w.T + b)


def row_sums_of_logits(z):
    """row_sums from the fp64 logits z (n, C)"""
    z = np.asarray(z, dtype=np.float64)
    m = z.max(axis=1, keepdims=True)
    lse = m + np.log(np.exp(z - m).sum(axis=1, keepdims=True))
    logp = z - lse
    p = np.exp(logp)
    with np.errstate(invalid="ignore"):
        h = np.where(p == 0.0, 0.0, p * logp).sum(axis=1)
    return lse[:, 0], h, p


def neg_entropy(pbar):
    """sum_y pbar_y log pbar_y with 0 log 0 = 0, by math.fsum"""
    return math.fsum(float(v) * math.log(float(v)) for v in np.asarray(pbar, dtype=np.float64) if v > 0.0)


def from_sums(row_h, psum, n):
    """The figures from the device's sums: row_h (n) fp64 and psum (S, C) fp64, psum[s] = sum of p over split s of split_bounds(n, S).
    {"inception_score", "inception_score_std", "per_split", "splits"}; every sum by math.fsum."""
    row_h = np.asarray(row_h, dtype=np.float64)
    psum = np.asarray(psum, dtype=np.float64)
    n = int(n)
    if row_h.shape != (n,) or psum.ndim != 2 or not 1 <= psum.shape[0] <= n:
        raise ValueError("from_sums: row_h (n,) and psum (S <= n, C) expected, got %s, %s for n = %d" % (row_h.shape, psum.shape, n))
    per_split = []
    for (lo, hi), ps in zip(split_bounds(n, psum.shape[0]), psum):
        rows = hi - lo
        mean_h = math.fsum(row_h[lo:hi].tolist()) / rows
        per_split.append(math.exp(mean_h - neg_entropy(ps / rows)))
    mean = math.fsum(per_split) / len(per_split)
    std = math.sqrt(math.fsum((v - mean) ** 2 for v in per_split) / len(per_split))
    return {"inception_score": mean, "inception_score_std": std, "per_split": per_split, "splits": len(per_split)}


def split_sums(p, n, splits):
    """psum (S, C) of the host's p (n, C): each split's rows added by math.fsum per class"""
    return np.array([[math.fsum(col.tolist()) for col in p[lo:hi].T] for lo, hi in split_bounds(n, splits)], dtype=np.float64)


def all_rows(psum):
    """(1, C): the all-row sum of p from the splits' sums, per class by math.fsum"""
    return np.array([[math.fsum(col.tolist()) for col in np.asarray(psum, dtype=np.float64).T]], dtype=np.float64)


def finish(row_h, psum, n):
    """from_sums, with "inception_score_all" -- the S = 1 figure, from all_rows(psum) -- beside it"""
    out = from_sums(row_h, psum, n)
    out["inception_score_all"] = from_sums(row_h, all_rows(psum), n)["inception_score"]
    return out


def score(codes, weight, bias, splits=SPLITS):
    """The whole definition on the host: finish() of row_sums of the codes, S = effective_splits(n, splits)"""
    _, h, p = row_sums(codes, weight, bias)
    n = h.shape[0]
    return finish(h, split_sums(p, n, effective_splits(n, splits)), n)


def kl_marginals(psum_a, n_a, psum_b, n_b):
    """KL(pbar_a || pbar_b) = sum_y pbar_a (log pbar_a - log pbar_b) of the two all-row marginals psum / n (0 log 0 = 0; +inf where
    pbar_b is 0 and pbar_a is not), by math.fsum"""
    a = np.asarray(psum_a, dtype=np.float64).reshape(-1) / int(n_a)
    b = np.asarray(psum_b, dtype=np.float64).reshape(-1) / int(n_b)
    if a.shape != b.shape:
        raise ValueError("kl_marginals: two marginals over the same classes expected, got %s, %s" % (a.shape, b.shape))
    if np.any((a > 0.0) & (b <= 0.0)):
        return float("inf")
    return math.fsum(float(u) * (math.log(float(u)) - math.log(float(v))) for u, v in zip(a, b) if u > 0.0)


def read_head(state, where="the head file"):
    """(weight (C, D) fp32, bias (C) fp32), numpy, of a state dict's `fc.weight` / `fc.bias`; None where it holds neither.
    ValueError for one without the other, another dtype or shapes that do not fit."""
    have = [k in state for k in HEAD_KEYS]
    if not any(have):
        return None
    if not all(have):
        raise ValueError("inception_score: %s holds one of %s without the other" % (where, HEAD_KEYS))
    w, b = (state[k].detach().cpu().contiguous().numpy() for k in HEAD_KEYS)
    if w.dtype != np.float32 or b.dtype != np.float32 or w.ndim != 2 or b.shape != (w.shape[0],) or w.shape[0] < 1:
        raise ValueError("inception_score: fp32 fc.weight (C, D) and fc.bias (C) expected in %s, got %s %s, %s %s"
                         % (where, w.dtype, w.shape, b.dtype, b.shape))
    return w, b


def head_digest(weight, bias):
    """SHA-256 (hex) over name, dtype, shape and bytes of the head's two tensors, as fid.trunk_digest hashes the trunk's"""
    h = hashlib.sha256()
    for name, a in zip(HEAD_KEYS, (weight, bias)):
        a = np.ascontiguousarray(a)
        h.update(("%s %s %s\n" % (name, a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()
