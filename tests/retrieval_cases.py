"""Shapes, seeded inputs, the fp64 oracle and the score bound of mogan_retrieval_rank (csrc/mogan_damsm.hip), shared by
tests/test_retrieval_reference_cpu.py (which measures the bound) and tests/test_retrieval_gpu.py (which applies it).

Oracle.  The reference repository has no R-precision code; the oracle is the metric's formula written with the project's own
miscc/losses.cosine_similarity and torch.argmax in fp64 on the CPU: candidate 0 is the query's own sentence code, candidates
1..Rn the bank rows of idx (clamped to [0, N - 1] as the kernel clamps them); score = cosine; the image is retrieved when argmax
over the candidates is 0 (argmax returns the FIRST maximal index: a tie counts for the match); rank = the number of mismatched
candidates with a strictly larger score, so that rank == 0 is exactly argmax == 0 -- the oracle asserts it.

Bound.  |score - fp64| <= TOL.  A cosine is a ratio of sums whose first-order error terms are bounded by the ratio itself
(|score| <= 1), so the bound is absolute.  TOL is 4 x the larger error of two fp32 CPU evaluations (the margin is
conv_cases.TOL's / bn_cases.TOL's): a numpy restatement of the kernel's summation order (64 lane partials as fma chains over
the lane-strided channels, then the wave's butterfly) and torch fp32 evaluating the oracle's formula; MEASURED holds the two
figures the CPU module printed, and that module holds TOL to them and to the ceiling of 1e-6.

Condition.  Rank equality with fp64 means something only away from near-ties, so gap() must be >= GAP = 1e-5 (about a hundred
times the fp32 error) for EVERY query of a case: the seeds below were picked for it (RandomState(seed) normal draws; of the seeds
0..19, 18 pass for (16, 99, 256, 500), all for (5, 99, 300, 130), 19 for (2, 1023, 64, 2000)) and the GPU module asserts it.
"""
import numpy as np
import torch

from helpers import load_pkg

load_pkg()

EPS = 1e-8
GAP = 1e-5
TOL_CEILING = 1e-6
# max |score - fp64| over CASES: {"restatement": numpy fp32 in the kernel's summation order, "torch fp32": the oracle's formula}
MEASURED = {"restatement": 4.6e-8, "torch fp32": 6.3e-8}
TOL = 2.6e-7

# (Q, Rn, C, N) -> seed
CASES = {
    (1, 1, 1, 1): 4,              # every score +-1; the seed's two candidates have opposite signs (the pure tie is test_tie_rule's)
    (3, 2, 5, 4): 0,              # small, not a multiple of anything
    (2, 4, 63, 7): 0,             # the lane boundary
    (2, 4, 64, 7): 0,
    (2, 4, 65, 7): 0,
    (5, 99, 300, 130): 0,         # the protocol's 99: stripes not a multiple of the 4 waves, C not a multiple of 64
    (16, 99, 256, 500): 0,        # the workload's row
    (2, 1023, 64, 2000): 0,       # the LDS limit
}


def make_inputs(shape, seed):
    """code (Q, C), pos (Q, C), bank (N, C) fp32 normal draws, idx (Q, Rn) int32 uniform in [0, N)"""
    Q, Rn, C, N = shape
    rng = np.random.RandomState(seed)
    code = rng.standard_normal((Q, C)).astype(np.float32)
    pos = rng.standard_normal((Q, C)).astype(np.float32)
    bank = rng.standard_normal((N, C)).astype(np.float32)
    idx = rng.randint(0, N, (Q, Rn)).astype(np.int32)
    return torch.from_numpy(code), torch.from_numpy(pos), torch.from_numpy(bank), torch.from_numpy(idx)


def candidates(pos, bank, idx):
    """(Q, Rn + 1, C): the match, then the bank rows of idx (clamped)"""
    rows = idx.long().clamp(0, bank.shape[0] - 1)
    return torch.cat([pos[:, None, :], bank[rows]], 1)


def scores(code, pos, bank, idx, dtype=torch.float64, eps=EPS):
    """the oracle's formula at `dtype`: (Q, Rn + 1)"""
    from mogan_amd.attngan.miscc.losses import cosine_similarity
    cand = candidates(pos.to(dtype), bank.to(dtype), idx)
    x = code.to(dtype)[:, None, :].expand_as(cand)
    return cosine_similarity(x, cand, dim=2, eps=eps).reshape(cand.shape[0], cand.shape[1])


def oracle(code, pos, bank, idx, eps=EPS):
    """fp64: (score (Q, Rn + 1), rank (Q,) int64)"""
    s = scores(code, pos, bank, idx, torch.float64, eps)
    rank = (s[:, 1:] > s[:, :1]).sum(1)
    assert torch.equal(rank == 0, torch.argmax(s, 1) == 0)
    return s, rank


def gap(score64):
    """the smallest |score[q, r] - score[q, 0]| over all q and r >= 1"""
    return float((score64[:, 1:] - score64[:, :1]).abs().min())


_REF = {}


def reference(shape):
    """inputs and fp64 oracle of a case, computed once and shared: {"in": (code, pos, bank, idx), "score", "rank"}"""
    if shape not in _REF:
        ins = make_inputs(shape, CASES[shape])
        s, r = oracle(*ins)
        _REF[shape] = {"in": ins, "score": s, "rank": r}
    return _REF[shape]


# ------------------------------------------------------------------------------------------------ the kernel's order, in numpy
def _fma(a, b, c):
    """fp32 fma through fp64: the product of two fp32 numbers is exact in fp64, the sum is rounded once there and once to fp32
    (double rounding: off a true fma by at most one fp32 ulp in rare cases -- an equally valid fp32 evaluation for an error figure)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _wave_sum(v):
    """v (..., 64) fp32: the xor butterfly of wave_sum; every lane ends with the same bits"""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., lanes ^ o]).astype(np.float32)
    return v[..., 0]


def _lane_dot(a, b):
    """sum_c a[..., c] b[..., c] as the kernel forms it: lane l chains c = l, l + 64, ... with fma, then the butterfly"""
    C = a.shape[-1]
    pad = (-C) % 64
    if pad:
        z = np.zeros(a.shape[:-1] + (pad,), np.float32)
        a, b = np.concatenate([a, z], -1), np.concatenate([b, z], -1)      # fma(0, 0, acc) = acc: a padded lane step is a no-op
    acc = np.zeros(a.shape[:-1] + (64,), np.float32)
    for k in range(a.shape[-1] // 64):
        acc = _fma(a[..., 64 * k:64 * k + 64], b[..., 64 * k:64 * k + 64], acc)
    return _wave_sum(acc)


def restatement(code, pos, bank, idx, eps=EPS):
    """numpy fp32 in the summation order of retrieval_rank_kernel: (Q, Rn + 1) fp32"""
    x = code.numpy()
    cand = candidates(pos, bank, idx).numpy()
    xb = np.broadcast_to(x[:, None, :], cand.shape)
    n0 = np.sqrt(_lane_dot(x, x)).astype(np.float32)
    d = _lane_dot(xb, cand)
    n1 = np.sqrt(_lane_dot(cand, cand)).astype(np.float32)
    den = np.maximum((n0[:, None] * n1).astype(np.float32), np.float32(eps))
    return (d / den).astype(np.float32)
