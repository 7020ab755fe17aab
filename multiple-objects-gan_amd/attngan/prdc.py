"""Host side of improved precision / recall (Kynkaanniemi et al., "Improved Precision and Recall Metric for Assessing Generative
Models", 2019; k = 3) and density / coverage (Naeem et al., "Reliable Fidelity and Diversity Metrics for Generative Models", 2020;
k = 5) between two sets of Inception pool codes (the reference repository has no code for them).

Every code owns a ball: its centre is the code, its radius the distance to the code's k-th nearest neighbour inside its OWN set
(the code itself not counted, by position).  With B_k(r) the ball of real code r and B_k(f) that of generated code f:

    precision = share of generated codes that lie in some B_k_pr(r)            are the generated images on the real manifold?
    recall    = share of real codes that lie in some B_k_pr(f)                 is the real manifold covered by the generated one?
    density   = sum_f #{ r : f in B_k_dc(r) } / (k_dc n_fake)                  how many real balls hold a generated code (may be > 1)
    coverage  = share of real codes r whose own B_k_dc(r) holds a generated code

"in" is d^2 <= radius^2, equality included.  The radii and the counts come from the device (hip/ops.knn_sqdist, hip/ops.ball_counts);
this module chooses the k's and forms the four figures from the counts:

  * `neighbours`          the k's a pair of sets allows;
  * `scores_from_counts`  the four figures, each a ratio of integers.
All four depend on the number of codes and are comparable at equal n only.  Nothing in this module needs a GPU.
"""
import numpy as np

K_PR = 3
K_DC = 5
K_MAX = 8            # the device keeps the 8 smallest distances per row


def neighbours(n_real, n_fake, k_pr=K_PR, k_dc=K_DC):
    """(k_pr, k_dc), each lowered to min(n_real, n_fake) - 1 where there are fewer codes (a code has n - 1 neighbours in its own set);
    ValueError where a set has fewer than 2 codes or a k is outside [1, 8]"""
    n = min(int(n_real), int(n_fake))
    if n < 2:
        raise ValueError("prdc: a set needs 2 codes at least (%d real, %d generated codes)" % (n_real, n_fake))
    out = []
    for name, k in (("k_pr", k_pr), ("k_dc", k_dc)):
        k = int(k)
        if k < 1 or k > K_MAX:
            raise ValueError("prdc: %s = %d outside [1, %d]" % (name, k, K_MAX))
        out.append(min(k, n - 1))
    return tuple(out)


def _counts(name, a, ndim):
    a = np.asarray(a)
    if a.ndim != ndim or a.shape[0] < 1 or not np.issubdtype(a.dtype, np.integer) or (ndim == 2 and a.shape[1] != 2):
        raise ValueError("scores_from_counts: %s must be integer counts of shape %s, got %s %s"
                         % (name, "(n,)" if ndim == 1 else "(n, 2)", a.dtype, a.shape))
    if a.min() < 0:
        raise ValueError("scores_from_counts: %s holds a negative count" % name)
    return a.astype(np.int64)


def scores_from_counts(fake_in_real, real_in_fake, real_own, k_dc):
    """{"precision", "recall", "density", "coverage"} as python floats, each ONE division of two integers.
    fake_in_real (n_fake, 2): per generated code the number of real balls that hold it, column 0 under the radii of k_pr, column 1
                              under those of k_dc;
    real_in_fake (n_real,):   per real code the number of generated balls (k_pr) that hold it;
    real_own     (n_real,):   per real code the number of generated codes inside its own ball (k_dc)."""
    f = _counts("fake_in_real", fake_in_real, 2)
    r = _counts("real_in_fake", real_in_fake, 1)
    o = _counts("real_own", real_own, 1)
    k_dc = int(k_dc)
    if k_dc < 1:
        raise ValueError("scores_from_counts: k_dc >= 1 expected, got %d" % k_dc)
    if r.shape != o.shape:
        raise ValueError("scores_from_counts: real_in_fake and real_own differ in length: %s, %s" % (r.shape, o.shape))
    n_fake, n_real = f.shape[0], r.shape[0]
    return {"precision": int((f[:, 0] > 0).sum()) / n_fake,
            "recall": int((r > 0).sum()) / n_real,
            "density": int(f[:, 1].sum()) / (k_dc * n_fake),
            "coverage": int((o > 0).sum()) / n_real}
