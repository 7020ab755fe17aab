"""-m gpu: nearest neighbours with labels on the device -- mogan_knn_label_f64 (csrc/mogan_knn.hip) through
ctypes in guard-banded, poisoned memory, as tests/test_nn_gpu.py does for mogan_knn_cross_f64.  Every check but the last is
EXACT, so none needs a tolerance:

  1. d2 / idx are mogan_knn_cross_f64's bits for the same inputs in the same process;
  2. for every label l, same_* of the queries labelled l is knn_cross(q_l, p[plabel == l], 1), the distance bit for bit and the
     position after mapping through the partition's ascending index list, and other_* likewise against p[plabel != l] -- a
     distance's bits depend on the two rows only and the partition keeps the order, so equality is the contract, not luck;
  3. planted inputs: bit copies across a tile and share border, a query that is a copy of a bank row of its class, a query label
     the bank does not hold, a bank of one label;
  4. two calls give the same bits;  5. nothing outside the outputs and the stated workspace is written, the inputs keep their bits;
  6. on cases of tests/nn_cases.py the K lists meet the bound tests/test_nn_gpu.py applies to mogan_knn_cross_f64: positions equal
     to the longdouble oracle's, distances within nn_cases.DIST_TOL.

Shapes: M in {1, 70}, N in {8, 130, 200} (200: four column tiles and, for up to 512 stripes, four shares), D in {33, 256} (the
scalar and the vector load path), K in {1, 5, 8}, K = N = 8 included."""
import itertools

import numpy as np
import pytest
import torch

import memguard as MG
import nn_cases as C
from helpers import load_pkg

load_pkg()
from mogan_amd.hip import lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FULL = (slice(None),)
NO_ROW = (1 << 31) - 1
INT_MIN = -(1 << 31)
LABELS = np.array([INT_MIN, -1, 0, NO_ROW], dtype=np.int32)        # arbitrary int32: no value is special
ABSENT = 77                                                        # a query label no bank row has
SHAPES = [(M, N, D, K) for M, N, D, K in itertools.product((1, 70), (8, 130, 200), (33, 256), (1, 5, 8))]
_INPUTS = {}


def _inputs(shape):
    """(q (M, D), qlabel (M,), p (N, D), plabel (N,)) of a shape, seeded, made once and frozen"""
    if shape not in _INPUTS:
        M, N, D, K = shape
        q, p = C.make_inputs(shape, 3)
        rng = np.random.RandomState(17 + M + N)
        plabel = LABELS[rng.randint(0, len(LABELS), size=N)]
        qlabel = np.concatenate([LABELS, [ABSENT]]).astype(np.int32)[rng.randint(0, len(LABELS) + 1, size=M)]
        if M == 1:
            qlabel[0] = plabel[N // 2]
        out = tuple(np.ascontiguousarray(a) for a in (q, qlabel, p, plabel))
        for a in out:
            a.setflags(write=False)
        _INPUTS[shape] = out
    return _INPUTS[shape]


def _frozen(a):
    """a host fp32 or int32 array in guarded device memory, bit for bit"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        t = torch.from_numpy(np.array(a)).to(DEV)
        return MG.Guarded(tuple(t.shape), FULL, DEV, base=t)
    assert a.dtype == np.int32
    t = torch.from_numpy(np.array(a)).view(torch.uint8).to(DEV)
    return MG.Guarded(tuple(t.shape), FULL, DEV, dtype=torch.uint8, base=t)


class Label:
    """the memory contract around a call: outputs and workspace as poisoned byte buffers inside bands, inputs bitwise frozen"""

    def __init__(self, q, qlabel, p, plabel, K):
        self.M, self.N, self.D, self.K = q.shape[0], p.shape[0], q.shape[1], int(K)
        assert p.shape[1] == self.D and qlabel.shape == (self.M,) and plabel.shape == (self.N,)
        self.inputs = [_frozen(q), _frozen(qlabel), _frozen(p), _frozen(plabel)]
        self.ws_bytes = int(lib.load().mogan_knn_label_ws_bytes(self.M, self.N, self.K))
        assert self.ws_bytes == C.ws_bytes(self.M, self.N, self.K) + 24 * C.shares(self.M, self.N) * self.M
        sizes = {"d2": 8 * self.M * self.K, "idx": 4 * self.M * self.K, "same_d2": 8 * self.M, "same_idx": 4 * self.M,
                 "other_d2": 8 * self.M, "other_idx": 4 * self.M}
        self.out = {name: MG.Guarded((n,), FULL, DEV, dtype=torch.uint8) for name, n in sizes.items()}
        self.ws = MG.Guarded((self.ws_bytes,), FULL, DEV, dtype=torch.uint8)

    def call(self):
        q, ql, p, pl = self.inputs
        o = self.out
        rc = lib.load().mogan_knn_label_f64(q.ptr, ql.ptr, self.M, p.ptr, pl.ptr, self.N, self.D, self.K, o["d2"].ptr, o["idx"].ptr,
                                            o["same_d2"].ptr, o["same_idx"].ptr, o["other_d2"].ptr, o["other_idx"].ptr, self.ws.ptr,
                                            self.ws_bytes, lib.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def run(self, what):
        """{"d2" (M, K) fp64, "idx" (M, K) int32, "same_d2" (M,), "same_idx" (M,), "other_d2" (M,), "other_idx" (M,)} on the host"""
        assert self.call() == 0
        res = {}
        for name, g in self.out.items():
            wide = name.endswith("d2")
            g.check(what="%s %s" % (what, name), written=False)                  # nothing outside the output changed
            never = g.view.view(torch.int64 if wide else torch.int32) == -1      # a double / an int still 0xFF in every byte
            assert not bool(never.any()), "%s: %d of %s never written (first at %d)" % (what, int(never.sum()), name,
                                                                                      int(torch.nonzero(never)[0]))
            a = g.view.view(torch.float64 if wide else torch.int32).cpu().numpy()
            res[name] = a.reshape(self.M, self.K) if name in ("d2", "idx") else a
        self.ws.check(what=what + " ws", written=False)                          # nothing outside the workspace changed
        for name, g in zip(("q", "qlabel", "p", "plabel"), self.inputs):
            assert g.untouched(), "%s: %s or its bands were modified" % (what, name)
        return res

    def again(self, what):
        for g in self.out.values():
            g.reset()
        self.ws.reset()
        return self.run(what)


def _same(got, want, what):
    """bit for bit: doubles by their int64 image, positions as they are"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s, want %s %s" % (what, got.dtype, got.shape, want.dtype,
                                                                                          want.shape)
    g, w = (got.view(np.int64), want.view(np.int64)) if got.dtype == np.float64 else (got, want)
    bad = np.argwhere(g != w)
    assert not len(bad), "%s: %d of %d differ, first at %s: got %r, want %r" % (what, len(bad), got.size, tuple(bad[0]),
                                                                                got[tuple(bad[0])], want[tuple(bad[0])])


def _cross(q, p, K):
    """ops.knn_cross on host arrays: (d2, idx) on the host"""
    d2, idx = ops.knn_cross(torch.from_numpy(np.array(q)).to(DEV), torch.from_numpy(np.array(p)).to(DEV), K)
    return d2.cpu().numpy(), idx.cpu().numpy()


def _by_partition(q, qlabel, p, plabel):
    """what same_* and other_* must be, from the formulation the kernel replaces: per label of a query one knn_cross against the bank
    rows of that label and one against the others, positions mapped back through the partition's ascending index list"""
    M = q.shape[0]
    want = {"same_d2": np.full(M, np.inf), "same_idx": np.full(M, NO_ROW, dtype=np.int32),
            "other_d2": np.full(M, np.inf), "other_idx": np.full(M, NO_ROW, dtype=np.int32)}
    for lab in np.unique(qlabel):
        rows = np.nonzero(qlabel == lab)[0]
        for name, part in (("same", np.nonzero(plabel == lab)[0]), ("other", np.nonzero(plabel != lab)[0])):
            if len(part):
                d2, idx = _cross(q[rows], p[part], 1)
                want[name + "_d2"][rows] = d2[:, 0]
                want[name + "_idx"][rows] = part[idx[:, 0]].astype(np.int32)
    return want


def _check_all(res, q, qlabel, p, plabel, K, what):
    d2, idx = _cross(q, p, K)                                           # 1: the K lists are knn_cross's
    _same(res["d2"], d2, what + " d2 against mogan_knn_cross_f64")
    _same(res["idx"], idx, what + " idx against mogan_knn_cross_f64")
    want = _by_partition(q, qlabel, p, plabel)                           # 2: the label lists are the partitioned calls'
    for name in want:
        _same(res[name], want[name], "%s %s against the partitioned bank" % (what, name))
    return want


# ------------------------------------------------------------------------------------------------- 1, 2, 4, 5: every shape
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_lists_bit_for_bit_in_guarded_memory(shape):
    q, qlabel, p, plabel = _inputs(shape)
    run = Label(q, qlabel, p, plabel, shape[3])
    res = run.run(str(shape))
    want = _check_all(res, q, qlabel, p, plabel, shape[3], str(shape))
    # the overall nearest row is the earlier of the two label lists' heads, and belongs to the list its label says
    first_same = (res["same_d2"] < res["other_d2"]) | ((res["same_d2"] == res["other_d2"]) & (res["same_idx"] < res["other_idx"]))
    _same(np.where(first_same, res["same_idx"], res["other_idx"]), res["idx"][:, 0], "the nearest of all")
    has = res["same_idx"] != NO_ROW
    assert (plabel[res["same_idx"][has]] == qlabel[has]).all() and np.isinf(res["same_d2"][~has]).all()
    has = res["other_idx"] != NO_ROW
    assert (plabel[res["other_idx"][has]] != qlabel[has]).all() and np.isinf(res["other_d2"][~has]).all()
    if shape[0] > 1:
        assert (want["same_idx"] == NO_ROW).any() and (want["same_idx"] != NO_ROW).any()     # the absent label occurs, and others
    again = run.again("%s, second call" % (shape,))                      # 4
    for name in res:
        _same(again[name], res[name], "second call " + name)


# ------------------------------------------------------------------------------------------------- 3: planted inputs
@pytest.mark.parametrize("D", (33, 256))
def test_planted_copies_ties_and_empty_sets(D):
    shape = (70, 200, D, 5)
    q, qlabel, p, plabel = (np.array(a) for a in _inputs(shape))
    assert C.shares(70, 200) == 4                                        # one column tile per share: 63 | 64 and 127 | 128 are borders
    A, B = 5, -5
    plabel[:] = np.where(np.arange(200) % 2 == 0, 1, 2)
    qlabel[:] = np.where(np.arange(70) % 3 == 0, 2, 1)
    p[64], p[128] = p[63], p[127]                                        # bit copies with different labels, across a border
    plabel[[63, 64, 127, 128]] = A, B, A, B
    p[190] = p[60]                                                       # bit copies with ONE label, three shares apart
    plabel[[60, 190]] = 9
    q[0], qlabel[0] = p[63], A                                           # a copy of a bank row of its own label ...
    q[1], qlabel[1] = p[64], B                                           # ... and of its twin
    q[2], qlabel[2] = p[128], A
    q[3], qlabel[3] = p[60], 9
    q[4], qlabel[4] = p[190], 1                                          # the copies are of another label
    qlabel[5] = ABSENT                                                   # a label the bank does not hold
    assert (p != np.round(p)).any()
    res = Label(q, qlabel, p, plabel, 5).run("planted D = %d" % D)
    _check_all(res, q, qlabel, p, plabel, 5, "planted D = %d" % D)

    def at(j):
        return tuple((float(res[n + "_d2"][j]), int(res[n + "_idx"][j])) for n in ("same", "other"))
    assert at(0) == ((0.0, 63), (0.0, 64)) and list(res["idx"][0, :2]) == [63, 64] and list(res["d2"][0, :2]) == [0.0, 0.0]
    assert at(1) == ((0.0, 64), (0.0, 63)) and list(res["idx"][1, :2]) == [63, 64]       # the lower position first in the K list
    assert at(2) == ((0.0, 127), (0.0, 128)) and list(res["idx"][2, :2]) == [127, 128]
    assert at(3)[0] == (0.0, 60) and at(3)[1][0] > 0 and list(res["idx"][3, :2]) == [60, 190]   # the tie inside ONE list: lower wins
    assert at(4)[1] == (0.0, 60) and at(4)[0][0] > 0
    assert at(5)[0] == (np.inf, NO_ROW) and at(5)[1] == (float(res["d2"][5, 0]), int(res["idx"][5, 0]))
    # a bank of one label: nothing else to be nearest to
    one = np.full(200, A, dtype=np.int32)
    res = Label(q, qlabel, p, one, 5).run("one label D = %d" % D)
    mine = qlabel == A
    assert mine.any() and not mine.all()
    assert np.isinf(res["other_d2"][mine]).all() and (res["other_idx"][mine] == NO_ROW).all()
    assert np.isinf(res["same_d2"][~mine]).all() and (res["same_idx"][~mine] == NO_ROW).all()
    _same(res["same_d2"][mine], res["d2"][mine, 0], "one label: same is the nearest of all")
    _same(res["other_idx"][~mine], res["idx"][~mine, 0], "one label: other is the nearest of all")


# ------------------------------------------------------------------------------------------------- 6: the oracle's bound
@pytest.mark.parametrize("case", [(100, 67, 80, 5), (200, 130, 100, 3), (9, 200, 24, 8)], ids=str)
def test_k_lists_against_longdouble_within_the_bound_of_knn_cross(case):
    ref = C.reference(case)
    rng = np.random.RandomState(23)
    qlabel, plabel = (LABELS[rng.randint(0, len(LABELS), size=n)] for n in (case[0], case[1]))
    res = Label(ref["q"], qlabel, ref["p"], plabel, case[3]).run(str(case))
    err = np.abs(res["d2"].astype(C.LD) - ref["d2"]) / ref["mag"]
    print("%s: worst %.3e of A (DIST_TOL %.2e)" % (case, float(err.max()), C.DIST_TOL))
    _same(res["idx"], ref["idx"].astype(np.int32), "%s positions against the oracle" % (case,))
    assert (err <= C.DIST_TOL).all()
    # the label lists from the oracle's own distances: the same positions (these cases keep every decision MARGIN apart)
    for name, keep in (("same", plabel[None, :] == qlabel[:, None]), ("other", plabel[None, :] != qlabel[:, None])):
        masked = np.where(keep, ref["all"], np.inf)
        want = np.where(keep.any(1), masked.argmin(1), NO_ROW).astype(np.int32)
        two, order = C.nearest(masked, 2)                                # a condition on the case, from the oracle alone
        a = np.take_along_axis(ref["mag_all"], order, axis=1).max(1)
        rows = np.isfinite(two[:, 1])
        assert ((two[rows, 1] - two[rows, 0]) / a[rows]).min() >= C.MARGIN
        _same(res[name + "_idx"], want, "%s %s positions against the oracle" % (case, name))


# ------------------------------------------------------------------------------------------------- the op
def test_op_matches_the_entry_point_and_raises():
    shape = (70, 130, 256, 5)
    q, qlabel, p, plabel = _inputs(shape)
    tq, tql, tp, tpl = (torch.from_numpy(np.array(a)).to(DEV) for a in (q, qlabel, p, plabel))
    for K in (1, 5, 8):
        out = ops.knn_label(tq, tql, tp, tpl, K)
        want = Label(q, qlabel, p, plabel, K).run("op K = %d" % K)
        assert [tuple(t.shape) for t in out] == [(70, K), (70, K), (70,), (70,), (70,), (70,)]
        assert [t.dtype for t in out] == [torch.float64, torch.int32] * 3 and all(t.is_cuda and not t.requires_grad for t in out)
        for t, name in zip(out, ("d2", "idx", "same_d2", "same_idx", "other_d2", "other_idx")):
            _same(t.cpu().numpy(), want[name], "knn_label K = %d %s" % (K, name))
    wide = torch.cat([tp, tp], dim=1)
    two = torch.stack([tql, tql], dim=1)
    for args in ((tq.double(), tql, tp, tpl, 3), (tq, tql, tp.half(), tpl, 3), (tq, tql, wide, tpl, 3), (tq.cpu(), tql, tp, tpl, 3),
                 (tq, tql, tp, tpl, 0), (tq, tql, tp, tpl, 9), (tq, tql, tp[:4], tpl[:4], 5),
                 (tq, tql.long(), tp, tpl, 3), (tq, tql, tp, tpl.float(), 3), (tq, tql[:-1], tp, tpl, 3), (tq, tql, tp, tpl[:-1], 3),
                 (tq, tql.cpu(), tp, tpl, 3), (tq, tql, tp, tpl.cpu(), 3), (tq, two[:, 0], tp, tpl, 3), (tq, two, tp, tpl, 3),
                 (tq, qlabel, tp, tpl, 3)):
        with pytest.raises(ValueError):
            ops.knn_label(*args)
