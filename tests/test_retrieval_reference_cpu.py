"""The score bound of mogan_retrieval_rank, measured on the CPU (tests/retrieval_cases.py): two fp32 evaluations of every case
against the fp64 oracle -- the numpy restatement of the kernel's summation order and torch fp32 on the oracle's own formula.  The
figures are printed; retrieval_cases.MEASURED records them and TOL must be 4 x the larger one at least, and under the ceiling.
The seeded inputs' condition (no near-tie with the match) and the restatement's ranks are checked here too, so a failure of the GPU
module cannot come from the cases themselves."""
import numpy as np
import pytest
import torch

import retrieval_cases as K

SHAPES = list(K.CASES)


def _errors(shape):
    ref = K.reference(shape)
    e_re = float(np.abs(K.restatement(*ref["in"]).astype(np.float64) - ref["score"].numpy()).max())
    e_t32 = float((K.scores(*ref["in"], dtype=torch.float32).double() - ref["score"]).abs().max())
    return e_re, e_t32


def test_tol_is_four_times_the_measured_fp32_error():
    worst = {"restatement": 0.0, "torch fp32": 0.0}
    for shape in SHAPES:
        e_re, e_t32 = _errors(shape)
        print("%-22s restatement %.3e   torch fp32 %.3e" % (shape, e_re, e_t32))
        worst["restatement"] = max(worst["restatement"], e_re)
        worst["torch fp32"] = max(worst["torch fp32"], e_t32)
    print("worst: %s -> TOL >= %.3e (recorded %s, TOL %.2e)" % (worst, 4 * max(worst.values()), K.MEASURED, K.TOL))
    for k, v in worst.items():
        assert K.MEASURED[k] >= v, (k, v)
        assert K.MEASURED[k] <= 1.25 * v + 1e-9, "the recorded figure of %s is stale: measured %.3e" % (k, v)
    assert 4 * max(K.MEASURED.values()) <= K.TOL <= K.TOL_CEILING
    assert K.GAP >= 30 * K.TOL                      # the gap condition sits far above the bound it protects


@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_seeded_inputs_are_away_from_ties_for_every_query(shape):
    ref = K.reference(shape)
    assert K.gap(ref["score"]) >= K.GAP
    assert tuple(ref["score"].shape) == (shape[0], shape[1] + 1) and ref["rank"].dtype == torch.int64
    # under that condition any evaluation within TOL ranks as fp64 does
    got = torch.from_numpy(K.restatement(*ref["in"]))
    assert torch.equal((got[:, 1:] > got[:, :1]).sum(1), ref["rank"])


def test_oracle_by_hand():
    """three candidates in the plane: the match at 45 degrees, one mismatched closer (0 degrees), one opposite"""
    code = torch.tensor([[2.0, 0.0]])
    pos = torch.tensor([[1.0, 1.0]])
    bank = torch.tensor([[3.0, 0.0], [-1.0, 0.0], [0.0, 0.0]])
    s, r = K.oracle(code, pos, bank, torch.tensor([[0, 1, 2]], dtype=torch.int32))
    assert torch.allclose(s, torch.tensor([[0.5 ** 0.5, 1.0, -1.0, 0.0]], dtype=torch.float64), atol=1e-15)
    assert r.tolist() == [1]
    # a tie counts for the match, and out-of-range rows are clamped
    s, r = K.oracle(code, bank[:1], bank, torch.tensor([[0, -5, 9]], dtype=torch.int32))
    assert s[0, 0] == s[0, 1] == s[0, 2] == 1.0 and s[0, 3] == 0.0 and r.tolist() == [0]


def test_restatement_gives_equal_bits_for_equal_candidates():
    """what the tie rule rests on, in the restatement: a bank row that is a bit copy of pos gets the match's bits at any position"""
    code, pos, bank, idx = K.make_inputs((3, 9, 70, 11), 1)
    bank[4] = pos[1]
    idx[1, 0], idx[1, 4], idx[1, 8] = 4, 4, 4
    got = K.restatement(code, pos, bank, idx)
    assert got[1, 0] == got[1, 1] == got[1, 5] == got[1, 9]
