"""Shared cases, an exact logit oracle and the error bound of the softmax-head kernel (mogan_softmax_head_f64)
for tests/test_softmax_head_gpu.py and tests/test_inception_score_gpu.py.  A plain helper module, not a conftest.

ORACLE.  The product of two fp32 values has at most 48 significant bits: it is exact in fp64.  math.fsum adds exactly and rounds
once, so fsum(products of a row, bias) is the CORRECTLY ROUNDED logit.  The softmax stages (attngan/inception_score.
row_sums_of_logits) then run in numpy fp64 on those logits.

BOUND (derived in DESIGN.md section 9o; u = 2^-53; every constant below is from that derivation, none from a measured error).
  logit     only the additions round: the D - 1 of the accumulation (the first product meets an accumulator of zero), the one of the
            bias, and the oracle's own final rounding -- D + 1 roundings between the device's logit and the oracle's:
            ez_i = (D + 1) u A_i,  A_i = max_y (sum_k |x_ik w_yk| + |b_y|).
  exp       exp(fl(a - b)) against exp(a - b): the subtraction's rounding moves the exponent by |a - b| u, the function itself is
            within one ulp (2 u).  Every such difference in a row is a difference of two of its logits, at most the row's range
            R_i = max_y z_iy - min_y z_iy (+ 1 for the logits' own errors), and nothing beyond 745 gives a result that is not
            zero: E_i = min(745, R_i + 1) + 2, relatively, in units of u.
  Z         the sum of at most C such terms, all positive, behind at most 2 Tc + 1 rescalings (E + 1 each: an exp and a product;
            Tc = ceil(C / 64), a lane sees two columns per tile) and a chain of at most 2 Tc + 32 additions:
            R_Z = E_i + (2 Tc + 32) + (2 Tc + 1)(E_i + 1), relatively, in units of u.
  row_lse   lse is 1-Lipschitz in the sup norm of z; log is within one ulp of a value in [0, log C]; one addition:
            e_lse_i = ez_i + (R_Z + 2 log max(C, 2) + |lse_i|) u.
  log p     e_lp_i = ez_i + e_lse_i + min(745, R_i + log C + 1) u (the subtraction: |lp| <= R_i + log C; wherever p is not zero)
  p         relatively e_lp_i + 2 u
  row_h     sum_y p lp: each term p |lp| (e_lp + 3 u) + p e_lp, a chain of at most 2 Tc + 32 additions; sum_y p |lp| = H_i, the row's
            entropy, and sum_y p = 1:  e_h_i = (e_lp_i + (35 + 2 Tc) u) H_i + e_lp_i.
  psum      a split's column: at most 8 + 2 + 1 additions inside a stripe and T_s = ceil(n_s / 64) between stripes:
            e_psum[s][y] = psum[s][y] (max_{i in s} e_lp_i + (13 + T_s) u).
Each is multiplied by SECOND_ORDER for the products of these first-order terms.
TOLERANCE of a comparison with the exact-logit oracle (`tolerance`): the bound above, in which ez already holds the oracle's one
rounding, plus the same bound with ez = 0 for the oracle's own softmax stages -- numpy on correctly rounded logits errs by the same
steps with shorter chains and a libm within one ulp.  The logit term is counted ONCE.  Only where the other side forms its logits in
floating point too (the end-to-end test: numpy's matmul, D roundings of its own in whatever order) is the whole bound taken twice
(BOTH_SIDES)."""
import math

import numpy as np

from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import inception_score as IS  # noqa: E402

U = 2.0 ** -53
LOG_TINY = 745.0                   # exp of anything below -745 is exactly 0 in fp64
SECOND_ORDER = 1.001
BOTH_SIDES = 2.0
TINY = 1e-300                      # what a sum may lose to terms that underflow on one side only

# (n, D, C, S): every n of {1, 63, 64, 65, 130}, D of {1, 3, 32, 36, 70} (32, 36: the vector loads), C of {1, 2, 63, 64, 65, 130} and
# S of {1, 2, 3, n} appears; 130 rows are three stripes at S = 1 and four at S = 2 (65 + 65)
SHAPES = ((1, 1, 1, 1), (1, 3, 2, 1), (1, 36, 130, 1), (63, 32, 63, 2), (63, 70, 64, 63), (64, 36, 64, 3), (64, 1, 130, 1),
          (64, 3, 65, 64), (65, 70, 65, 65), (65, 32, 1, 2), (130, 3, 130, 3), (130, 36, 2, 130), (130, 70, 65, 2), (130, 32, 63, 1))
SPECIAL = {"spread": (65, 36, 130, 3), "zero head": (65, 32, 65, 2)}
_CASES = {}


def make_inputs(shape, kind="plain", seed=5):
    """(x (n, D), w (C, D), b (C)) fp32: non-negative codes around 0.5 as the trunk's pooled ReLU outputs are; w ~ N(0, 0.05^2), logits
    O(1).  "spread": w ~ N(0, 6^2), logits to +-40 and beyond, class 7 lifted by 40, every fifth class pushed down by 1000 so that its
    p underflows to exactly 0.  "zero head": w = 0, the logits are the bias."""
    n, D, C, S = shape
    rng = np.random.RandomState(seed + 1000 * n + 100 * D + C)
    x = rng.uniform(0.0, 1.0, size=(n, D)).astype(np.float32)
    w = (rng.standard_normal((C, D)) * 0.05).astype(np.float32)
    b = (rng.standard_normal(C) * 0.05).astype(np.float32)
    if kind == "spread":
        w = (rng.standard_normal((C, D)) * 6.0).astype(np.float32)
        b[7] += np.float32(40.0)
        b[::5] -= np.float32(1000.0)
    elif kind == "zero head":
        w = np.zeros((C, D), dtype=np.float32)
    return x, w, b


def exact_logits(x, w, b):
    """(n, C) fp64: the correctly rounded <x_i, w_y> + b_y -- exact fp64 products, math.fsum"""
    x64, w64, b64 = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (x, w, b))
    z = np.empty((x64.shape[0], w64.shape[0]), dtype=np.float64)
    for i in range(x64.shape[0]):
        prod = w64 * x64[i][None, :]                      # exact
        for y in range(w64.shape[0]):
            z[i, y] = math.fsum(prod[y].tolist() + [float(b64[y])])
    return z


def logit_scale(x, w, b):
    """A_i = max_y (sum_k |x_ik w_yk| + |b_y|), fp64 (n,)"""
    x64, w64, b64 = (np.abs(np.asarray(a, dtype=np.float32).astype(np.float64)) for a in (x, w, b))
    return (x64 @ w64.T + b64[None, :]).max(axis=1)


def bounds(D, C, A, R, lse, h, psum, S):
    """{"row_lse" (n), "log_p" (n), "row_h" (n), "psum" (S, C)}: the bound of the module's docstring, for ONE side, from the shapes,
    the operands' magnitudes A (n), the rows' logit ranges R (n) and the oracle's lse (n), h (n) and psum (S, C)"""
    n = len(A)
    Tc = (C + 63) // 64
    ez = (D + 1) * U * np.asarray(A, dtype=np.float64)
    e_exp = np.minimum(LOG_TINY, np.asarray(R, dtype=np.float64) + 1.0) + 2.0
    r_z = e_exp + (2 * Tc + 32) + (2 * Tc + 1) * (e_exp + 1.0)
    e_lse = ez + (r_z + 2.0 * math.log(max(C, 2)) + np.abs(lse)) * U
    e_lp = ez + e_lse + np.minimum(LOG_TINY, np.asarray(R, dtype=np.float64) + math.log(C) + 1.0) * U
    e_h = (e_lp + (35 + 2 * Tc) * U) * np.abs(h) + e_lp + TINY
    e_ps = np.empty((S, C), dtype=np.float64)
    for s, (lo, hi) in enumerate(IS.split_bounds(n, S)):
        e_ps[s] = psum[s] * (e_lp[lo:hi].max() + (13 + (hi - lo + 63) // 64) * U) + (hi - lo) * TINY
    return {"row_lse": SECOND_ORDER * e_lse, "log_p": SECOND_ORDER * e_lp, "row_h": SECOND_ORDER * e_h, "psum": SECOND_ORDER * e_ps}


def tolerance(D, C, A, R, lse, h, psum, S):
    """what a comparison of the device with the exact-logit oracle allows: bounds() plus bounds() at exact logits (A = 0) for the
    oracle's own stages; the logit term enters once"""
    dev, own = bounds(D, C, A, R, lse, h, psum, S), bounds(D, C, np.zeros(len(A)), R, lse, h, psum, S)
    return {k: dev[k] + own[k] for k in dev}


def score_bounds(D, C, A, R, lse, h, psum, S):
    """(S,) the bound, for ONE side, of log IS_s = mean_i h_i + G(pbar_s), G = -sum_y pbar log pbar: the mean moves by at most the
    largest e_h of its rows; pbar_y = psum_y / n_s moves relatively by r = e_psum / psum + u, and G by at most
    sum_y |dpbar_y| (|log pbar_y| + 1) <= r (G + 1); the host's fsum, log and exp add a few u on figures of size |log IS| + G + 1"""
    n = len(A)
    one = bounds(D, C, A, R, lse, h, psum, S)
    out = np.empty(S, dtype=np.float64)
    for s, (lo, hi) in enumerate(IS.split_bounds(n, S)):
        pbar = psum[s] / (hi - lo)
        G = -IS.neg_entropy(pbar)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = float(np.nanmax(np.where(psum[s] > 0.0, one["psum"][s] / psum[s], 0.0))) + U
        mean_h = math.fsum(h[lo:hi].tolist()) / (hi - lo)
        out[s] = one["row_h"][lo:hi].max() + r * (G + 1.0) + 16.0 * U * (abs(mean_h) + G + 1.0)
    return SECOND_ORDER * out


def case(shape, kind="plain"):
    """the frozen inputs and the oracle's figures of a case, computed once: dict x, w, b, z, lse, h, p, psum, A, bound"""
    key = (tuple(shape), kind)
    if key not in _CASES:
        n, D, C, S = shape
        x, w, b = make_inputs(shape, kind)
        z = exact_logits(x, w, b)
        lse, h, p = IS.row_sums_of_logits(z)
        psum = IS.split_sums(p, n, S)
        A = logit_scale(x, w, b)
        R = z.max(axis=1) - z.min(axis=1)
        out = {"x": x, "w": w, "b": b, "z": z, "lse": lse, "h": h, "p": p, "psum": psum, "A": A, "R": R,
               "bound": bounds(D, C, A, R, lse, h, psum, S), "tol": tolerance(D, C, A, R, lse, h, psum, S)}
        for a in list(out.values()) + list(out["bound"].values()) + list(out["tol"].values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CASES[key] = out
    return _CASES[key]
