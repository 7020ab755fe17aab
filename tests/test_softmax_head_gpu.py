"""-m gpu: the sums of the Inception Score on the device -- mogan_softmax_head_f64 (csrc/mogan_softmax_head.hip)
through ctypes in guard-banded, poisoned memory, as tests/test_knn_label_gpu.py does for its entry point.

  1. per element against the exact-logit oracle of tests/inception_score_cases.py, within the bound derived there (a formula in D, C,
     the split's row count and the operands' magnitudes; plus the same bound at exact logits for the numpy stages' own error -- the logit
     term enters once, inception_score_cases.tolerance); the worst
     error / tolerance ratio is printed (DESIGN.md section 9o records the MI355X's);
  2. the bit contracts, bitwise: a row alone against the same row at positions 0, 63, 64 and 129 of a batch; psum[s] against the S = 1
     call on the split's rows; two calls; C = 1 exactly;
  3. the memory contract: every output element written, nothing outside the outputs and the stated workspace, the inputs unchanged.

Shapes: inception_score_cases.SHAPES (n in {1, 63, 64, 65, 130}, D in {1, 3, 32, 36, 70}, C in {1, 2, 63, 64, 65, 130}, S in {1, 2, 3, n})
and the two special inputs: logits spread past +-40 with tails that underflow, and a head of zeros."""
import numpy as np
import pytest
import torch

import inception_score_cases as C
import memguard as MG
from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import inception_score as IS  # noqa: E402
from mogan_amd.hip import lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FULL = (slice(None),)
WORST = [0.0]


def _frozen(a):
    t = torch.from_numpy(np.array(a, dtype=np.float32)).to(DEV)
    return MG.Guarded(tuple(t.shape), FULL, DEV, base=t)


class Head:
    """the memory contract around a call: outputs and workspace as poisoned byte buffers inside bands, inputs bitwise frozen"""

    def __init__(self, x, w, b, S, want_lse=True):
        self.n, self.D, self.C, self.S = x.shape[0], x.shape[1], w.shape[0], int(S)
        assert w.shape[1] == self.D and b.shape == (self.C,)
        self.inputs = [_frozen(x), _frozen(w), _frozen(b)]
        self.ws_bytes = int(lib.load().mogan_softmax_head_ws_bytes(self.n, self.C, self.S))
        most = -(-self.n // self.S)
        assert self.ws_bytes == 8 * self.S * (-(-most // 64)) * self.C                     # the header's formula
        sizes = {"row_h": 8 * self.n, "psum": 8 * self.S * self.C}
        if want_lse:
            sizes["row_lse"] = 8 * self.n
        self.out = {name: MG.Guarded((k,), FULL, DEV, dtype=torch.uint8) for name, k in sizes.items()}
        self.ws = MG.Guarded((self.ws_bytes,), FULL, DEV, dtype=torch.uint8)

    def call(self):
        x, w, b = self.inputs
        o = self.out
        rc = lib.load().mogan_softmax_head_f64(x.ptr, self.n, self.D, w.ptr, b.ptr, self.C, self.S,
                                               o["row_lse"].ptr if "row_lse" in o else None, o["row_h"].ptr, o["psum"].ptr,
                                               self.ws.ptr, self.ws_bytes, lib.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def run(self, what):
        """{"row_lse" (n), "row_h" (n), "psum" (S, C)} fp64 on the host"""
        assert self.call() == 0
        res = {}
        for name, g in self.out.items():
            g.check(what="%s %s" % (what, name), written=False)                  # nothing outside the output changed
            never = g.view.view(torch.int64) == -1                               # a double still 0xFF in every byte
            assert not bool(never.any()), "%s: %d of %s never written (first at %d)" % (what, int(never.sum()), name,
                                                                                      int(torch.nonzero(never)[0]))
            a = g.view.view(torch.float64).cpu().numpy()
            res[name] = a.reshape(self.S, self.C) if name == "psum" else a
        self.ws.check(what=what + " ws", written=False)                          # nothing outside the workspace changed
        for name, g in zip(("x", "w", "bias"), self.inputs):
            assert g.untouched(), "%s: %s or its bands were modified" % (what, name)
        return res

    def again(self, what):
        for g in self.out.values():
            g.reset()
        self.ws.reset()
        return self.run(what)


def _same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64, what
    bad = np.argwhere(got.view(np.int64) != want.view(np.int64))
    assert not len(bad), "%s: %d of %d differ, first at %s: got %r, want %r" % (what, len(bad), got.size, tuple(bad[0]),
                                                                                got[tuple(bad[0])], want[tuple(bad[0])])


def _within(got, case, what):
    worst = 0.0
    for name, ref in (("row_lse", case["lse"]), ("row_h", case["h"]), ("psum", case["psum"])):
        tol = case["tol"][name]
        err = np.abs(got[name] - ref)
        assert np.all(np.isfinite(got[name])), "%s: %s is not finite" % (what, name)
        assert np.all(tol > 0.0)
        ratio = float(np.max(err / tol))
        print("%s %s: worst error %.3e, error / tolerance %.4f" % (what, name, float(err.max()), ratio))
        worst = max(worst, ratio)
        bad = np.argwhere(~(err <= tol))
        assert not len(bad), "%s: %s off at %s: got %r, want %r, tolerance %r" % (what, name, tuple(bad[0]), got[name][tuple(bad[0])],
                                                                                  ref[tuple(bad[0])], tol[tuple(bad[0])])
    WORST[0] = max(WORST[0], worst)
    print("worst error / tolerance so far: %.4f" % WORST[0])


@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "n%d-D%d-C%d-S%d" % s)
def test_every_case_within_its_bound_in_guarded_memory_and_twice_the_same(shape):
    case = C.case(shape)
    head = Head(case["x"], case["w"], case["b"], shape[3])
    got = head.run(str(shape))
    _within(got, case, str(shape))
    again = head.again(str(shape) + " again")
    for name in got:
        _same(again[name], got[name], "%s second call %s" % (shape, name))
    # without row_lse the other outputs keep their bits
    lean = Head(case["x"], case["w"], case["b"], shape[3], want_lse=False).run(str(shape) + " no lse")
    for name in lean:
        _same(lean[name], got[name], "%s without row_lse %s" % (shape, name))


@pytest.mark.parametrize("kind", list(C.SPECIAL))
def test_spread_logits_and_a_head_of_zeros(kind):
    shape = C.SPECIAL[kind]
    case = C.case(shape, kind)
    got = Head(case["x"], case["w"], case["b"], shape[3]).run(kind)
    _within(got, case, kind)
    if kind == "spread":
        assert float(np.abs(case["z"]).max()) > 40.0 and bool((case["p"] == 0.0).any())     # tails that underflow: 0, not NaN
        assert float(case["p"].max()) > 0.99                                              # and a dominant class
        dead = np.flatnonzero((case["p"] == 0.0).all(axis=0))
        assert len(dead) and np.all(got["psum"][:, dead] == 0.0)
    else:
        _same(got["row_lse"], np.full(shape[0], got["row_lse"][0]), "a head of zeros: every row has the bias alone")
        _same(got["row_h"], np.full(shape[0], got["row_h"][0]), "a head of zeros: every row has the bias alone")


def test_a_row_has_the_bits_it_has_alone_at_any_position_and_under_any_split():
    shape = (130, 36, 130, 3)
    for D in (36, 3):                                               # the vector and the scalar loads
        x, w, b = C.make_inputs((130, D, 130, 3))
        row = x[5].copy()
        alone = Head(row[None, :], w, b, 1).run("alone")
        for pos in (0, 63, 64, 129):
            batch = x.copy()
            batch[pos] = row
            for S in (1, 3, 130):
                got = Head(batch, w, b, S).run("position %d S %d" % (pos, S))
                for name in ("row_lse", "row_h"):
                    _same(got[name][pos:pos + 1], alone[name], "D %d position %d S %d %s" % (D, pos, S, name))
                if S == 130:
                    _same(got["psum"][pos:pos + 1], alone["psum"], "D %d position %d: a split of one row" % (D, pos))


@pytest.mark.parametrize("shape", [(130, 70, 65, 2), (130, 36, 130, 3), (65, 32, 63, 65), (130, 3, 2, 130)], ids=str)
def test_a_splits_sums_are_those_of_the_call_on_its_rows_alone(shape):
    n, D, Cn, S = shape
    x, w, b = C.make_inputs(shape)
    whole = Head(x, w, b, S).run(str(shape))
    for s, (lo, hi) in enumerate(IS.split_bounds(n, S)):
        if S > 3 and s not in (0, 1, S // 2, S - 1):
            continue
        part = Head(x[lo:hi], w, b, 1).run("%s split %d" % (shape, s))
        _same(whole["psum"][s:s + 1], part["psum"], "%s psum of split %d" % (shape, s))
        _same(whole["row_h"][lo:hi], part["row_h"], "%s row_h of split %d" % (shape, s))


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (65, 32, 1, 2), (130, 3, 1, 130)], ids=str)
def test_one_class_gives_exact_values(shape):
    n, D, Cn, S = shape
    x, w, b = C.make_inputs(shape)
    got = Head(x, w, b, S).run(str(shape))
    assert np.all(got["row_h"] == 0.0)
    rows = np.array([[hi - lo] for lo, hi in IS.split_bounds(n, S)], dtype=np.float64)
    _same(got["psum"], rows, "psum is the row count")
    out = IS.finish(got["row_h"], got["psum"], n)
    assert out["inception_score"] == 1.0 and out["inception_score_all"] == 1.0 and out["per_split"] == [1.0] * S
    assert np.all(np.abs(got["row_lse"] - C.exact_logits(x, w, b)[:, 0]) <= (D + 1) * C.U * C.logit_scale(x, w, b))


def test_ops_softmax_head_sums_gives_the_entry_points_bits_and_checks_its_arguments():
    shape = (130, 36, 130, 3)
    case = C.case(shape)
    want = Head(case["x"], case["w"], case["b"], 3).run("ctypes")
    x, w, b = (torch.from_numpy(np.array(case[k])).to(DEV) for k in ("x", "w", "b"))
    row_h, psum = ops.softmax_head_sums(x, w, b, 3)
    lse, row_h2, psum2 = ops.softmax_head_sums(x, w, b, 3, want_lse=True)
    assert row_h.dtype == psum.dtype == torch.float64 and tuple(psum.shape) == (3, 130)
    for got, name in ((row_h, "row_h"), (psum, "psum"), (row_h2, "row_h"), (psum2, "psum"), (lse, "row_lse")):
        _same(got.cpu().numpy(), want[name], "ops %s" % name)
    for args in ((x.double(), w, b, 1), (x, w[:, :8].contiguous(), b, 1), (x, w, b[:5].contiguous(), 1), (x, w, b, 0), (x, w, b, 131),
                 (x.t(), w, b, 1), (x, w, b.cpu(), 1)):
        with pytest.raises(ValueError):
            ops.softmax_head_sums(*args)


def test_rejected_arguments_write_nothing():
    case = C.case((65, 32, 1, 2))
    head = Head(case["x"], case["w"], case["b"], 2)
    head.S = 66                                                      # more splits than rows
    assert head.call() == -1
    head.S = 2
    head.ws_bytes -= 8
    assert head.call() == -3
    for g in list(head.out.values()) + [head.ws] + head.inputs:
        assert g.untouched()
