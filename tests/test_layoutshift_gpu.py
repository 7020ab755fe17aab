"""-m gpu: the sums of the layout-shift score on the device -- the entry of csrc/mogan_layout.hip through ctypes with every buffer in
guard-banded, poisoned memory against the numpy fp64 oracle (tests/layout_cases.py: cases, seeds and the derived bound), the five bit
contracts of include/mogan_hip.h, the rows the kernel should never see, the op, and the accumulator against the oracle's figures.
No bound here comes from the code under test.

The fp32 images live in memguard.Guarded's float mode and are held bit for bit (memguard.Frozen holds the op's inputs); the int32
tables and the fp64 / int32 outputs live in its byte mode as in tests/test_spectrum_gpu.py."""
import json

import numpy as np
import pytest
import torch

import layout_cases as LC
import memguard as MG
from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import layoutshift as LS  # noqa: E402
from mogan_amd.hip import lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FULL = (slice(None),)


def _frozen(a, skew=0):
    """an input in guarded memory: fp32 as it is (skew: that many floats past a 16-byte boundary), anything else as its bytes"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        t = torch.from_numpy(a.copy()).to(DEV)
        if skew:
            g = MG.Guarded((t.numel() + skew,), (slice(skew, None),), DEV, base=t.reshape(-1))
            assert g.ptr % 16 == 4 * skew
            return g
        g = MG.Guarded(tuple(t.shape), FULL, DEV, base=t)
        assert g.ptr % 16 == 0
        return g
    t = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(DEV)
    return MG.Guarded(tuple(t.shape), FULL, DEV, dtype=torch.uint8, base=t)


def _bits_equal(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype == np.float64 and got.shape == want.shape
    bad = np.argwhere(got.view(np.int64) != want.view(np.int64))
    assert not len(bad), "%s: %d of %d values differ, first at %s: got %r, want %r" % (what, len(bad), got.size, tuple(bad[0]),
                                                                                     got[tuple(bad[0])], want[tuple(bad[0])])


class Shift:
    """one call of mogan_box_shift_sums_f64 with every buffer guarded: run() -> (sums (P, 7) fp64, counts (P, 5) int32) on the host"""

    def __init__(self, a, b, edit, others, skew=(0, 0)):
        self.P, self.C, self.S, _ = a.shape
        others = np.zeros((self.P, 0, 4), dtype=np.int32) if others is None else np.asarray(others, dtype=np.int32)
        self.G = int(others.shape[1])
        self.inputs = {"a": _frozen(a, skew[0]), "b": _frozen(b, skew[1]), "edit": _frozen(np.asarray(edit, dtype=np.int32))}
        if self.G:
            self.inputs["others"] = _frozen(others)
        self.sums = MG.Guarded((8 * self.P * 7,), FULL, DEV, dtype=torch.uint8)
        self.counts = MG.Guarded((4 * self.P * 5,), FULL, DEV, dtype=torch.uint8)

    def call(self, **kw):
        i = self.inputs
        v = dict(a=i["a"].ptr, b=i["b"].ptr, P=self.P, C=self.C, S=self.S, edit=i["edit"].ptr,
                 others=i["others"].ptr if self.G else None, G=self.G, sums=self.sums.ptr, counts=self.counts.ptr)
        v.update(kw)
        rc = lib.load().mogan_box_shift_sums_f64(v["a"], v["b"], v["P"], v["C"], v["S"], v["edit"], v["others"], v["G"], v["sums"],
                                                 v["counts"], lib.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def run(self, what):
        assert self.call() == 0
        for name, g in self.inputs.items():
            assert g.untouched(), "%s: %s or its bands were modified" % (what, name)
        self.sums.check(what=what + " sums", written=False)          # nothing outside the P * 7 doubles
        self.counts.check(what=what + " counts", written=False)
        s, c = self.sums.view.view(torch.int64), self.counts.view.view(torch.int32)
        assert not bool((s == -1).any()) and not bool((c == -1).any()), "%s: an output was never written" % what
        return (self.sums.view.view(torch.float64).cpu().numpy().reshape(self.P, 7),
                c.cpu().numpy().reshape(self.P, 5))

    def again(self, what):
        for g in (self.sums, self.counts):
            g.reset()
        return self.run(what)


# ------------------------------------------------------------------------------------------------- 1: the entry point
@pytest.mark.parametrize("key", LC.CASES, ids=str)
def test_every_case_within_its_bound_in_guarded_memory(key):
    a, b, edit, others = LC.case(key)
    want, want_counts, bound = LC.expected(key)
    run = Shift(a, b, edit, others if key[3] else None)
    got, counts = run.run("case %s" % (key,))
    assert (counts == want_counts).all(), "%s: counts %s, want %s" % (key, counts.tolist(), want_counts.tolist())
    with np.errstate(invalid="ignore", divide="ignore"):
        share = np.where(bound > 0, np.abs(got - want) / bound, 0.0)
    print("case %s: the worst sum uses %.4f of its bound (n + 4) 2^-52 want" % (key, share.max()))
    bad = np.argwhere(~(np.abs(got - want) <= bound))
    assert not len(bad), "%s: %d sums off, first (pair, sum) %s: got %r, want %r, bound %r" % (
        key, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])], bound[tuple(bad[0])])
    again, counts_again = run.again("second call")                                           # contract (a)
    _bits_equal(again, got, "a second call")
    assert (counts_again == counts).all()
    # the op is the entry: host tables, frozen device images
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    frozen = [MG.Frozen(ta), MG.Frozen(tb)]
    s, c = ops.box_shift_sums(ta, tb, torch.from_numpy(edit), torch.from_numpy(others))
    for f in frozen:
        f.check("ops.box_shift_sums %s" % (key,))
    assert s.dtype == torch.float64 and c.dtype == torch.int32 and s.is_cuda and c.is_cuda
    assert tuple(s.shape) == (key[0], 7) and tuple(c.shape) == (key[0], 5)
    _bits_equal(s.cpu().numpy(), got, "the op against the entry")
    assert (c.cpu().numpy() == counts).all()


# ------------------------------------------------------------------------------------------------- 2: the bit contracts
@pytest.mark.parametrize("key", [(3, 3, 16, 2), (5, 3, 64, 2), (2, 3, 256, 3)], ids=str)
def test_a_pairs_row_has_the_bits_it_has_alone_and_at_any_position(key):
    a, b, edit, others = LC.case(key)
    whole, counts = Shift(a, b, edit, others).run("P = %d" % key[0])
    for p in range(key[0]):
        alone, c = Shift(a[p:p + 1], b[p:p + 1], edit[p:p + 1], others[p:p + 1]).run("P = 1")
        _bits_equal(alone[0], whole[p], "pair %d alone against its row" % p)
        assert (c[0] == counts[p]).all()
    back, c = Shift(a[::-1], b[::-1], edit[::-1], others[::-1]).run("reversed")
    _bits_equal(back[::-1], whole, "the batch in reverse order")
    assert (c[::-1] == counts).all()


@pytest.mark.parametrize("key", [(3, 3, 16, 2), (2, 3, 20, 1), (2, 3, 7, 1)], ids=str)
def test_the_bits_do_not_depend_on_the_alignment_of_the_images(key):
    """16-byte loads where both images allow them, 4-byte loads otherwise: the same values in the same order"""
    a, b, edit, others = LC.case(key)
    whole, counts = Shift(a, b, edit, others).run("aligned")
    for skew in ((1, 0), (0, 3), (2, 2)):
        got, c = Shift(a, b, edit, others, skew=skew).run("images %d and %d floats past a 16-byte boundary" % skew)
        _bits_equal(got, whole, "skew %s against aligned images" % (skew,))
        assert (c == counts).all()


@pytest.mark.parametrize("key", LC.CASES, ids=str)
def test_a_bit_copy_gives_exact_zeros_and_moved_equal_to_baseline(key):
    a, b, edit, others = LC.case(key)
    got, counts = Shift(a, a.copy(), edit, others if key[3] else None).run("b = a")
    assert (got[:, :5] == 0.0).all() and not np.signbit(got[:, :5]).any()
    _bits_equal(got[:, 5], got[:, 6], "moved against baseline where b is a bit copy of a")
    assert (got[:, 6] > 0).all() and (counts == LC.expected(key)[1]).all()


@pytest.mark.parametrize("key", LC.CASES, ids=str)
def test_exchanging_a_and_b_changes_no_bit_of_the_class_sums(key):
    a, b, edit, others = LC.case(key)
    oth = others if key[3] else None
    ab, _ = Shift(a, b, edit, oth).run("a, b")
    ba, _ = Shift(b, a, edit, oth).run("b, a")
    _bits_equal(ba[:, :5], ab[:, :5], "the class sums with a and b exchanged")
    assert (ba[:, 6] != ab[:, 6]).any()                              # the baseline is a's own


def test_an_offset_of_zero_gives_a_baseline_of_exactly_zero():
    for key in LC.CASES[1:4] + LC.CASES[5:]:
        a, b, edit, others = LC.case(key)
        still = edit.copy()
        still[:, 4:] = 0
        got, counts = Shift(a, b, still, others).run("delta = 0")
        assert (got[:, 6] == 0.0).all() and not np.signbit(got[:, 6]).any() and (got[:, 5] > 0).all()
        assert (counts[:, 0] == 0).all() and (counts[:, 1] == 0).all()                       # old == new: class 2 only
        # moved and the class-2 sum are then the same terms in another order
        assert (np.abs(got[:, 5] - got[:, 2]) <= (counts[:, 2] * key[1] + 4) * LC.EPS * got[:, 2]).all()


# ------------------------------------------------------------------------------------------------- 3: rows that are never sent
NEVER = [("empty in x", [4, 3, 4, 8, 1, 1]), ("x1 < x0", [9, 3, 2, 8, 0, 1]), ("x0 < 0", [-1, 3, 6, 8, 4, 0]), ("y1 > S", [2, 3, 6, 17, 0, -3]),
         ("moved past the left edge", [2, 3, 6, 8, -3, 0]), ("moved past the bottom edge", [2, 3, 6, 8, 0, 9]),
         ("an offset that wraps 32 bits", [2, 3, 6, 8, 2 ** 31 - 1, 0]), ("a rectangle far outside", [10 ** 9, 10 ** 9, 2 * 10 ** 9, 2 * 10 ** 9, 0, 0]),
         ("an offset far outside", [2, 3, 6, 8, -2 ** 31, -2 ** 31])]


@pytest.mark.parametrize("row", [c[1] for c in NEVER], ids=[c[0] for c in NEVER])
def test_a_row_the_kernel_should_never_see_gets_zeros_and_its_neighbours_are_untouched(row):
    key = (3, 3, 16, 2)
    a, b, edit, others = LC.case(key)
    want, want_counts, _ = LC.expected(key)
    whole, _ = Shift(a, b, edit, others).run("the legal batch")
    bad = edit.copy()
    bad[1] = np.array(row, dtype=np.int64).astype(np.int32)
    got, counts = Shift(a, b, bad, others).run("row 1 illegal")
    assert (got[1] == 0.0).all() and not np.signbit(got[1]).any() and (counts[1] == 0).all()
    _bits_equal(got[[0, 2]], whole[[0, 2]], "the neighbours of a row that is answered with zeros")
    assert (counts[[0, 2]] == want_counts[[0, 2]]).all()
    o_sums, o_counts = LS.sums_numpy(a, b, bad, others)                                      # the oracle agrees on what is never seen
    assert (o_sums[1] == 0).all() and (o_counts[1] == 0).all()


def test_rejected_arguments_return_non_zero_and_write_nothing():
    a, b, edit, others = LC.case((3, 3, 16, 2))
    run = Shift(a, b, edit, others)
    for kw in (dict(P=0), dict(C=0), dict(C=5), dict(S=1), dict(S=1025), dict(G=-1), dict(G=9), dict(a=None), dict(b=None),
               dict(edit=None), dict(others=None), dict(sums=None), dict(counts=None)):
        assert run.call(**kw) == -1, kw
        assert run.sums.untouched() and run.counts.untouched(), kw
    run.run("after the rejections")


# ------------------------------------------------------------------------------------------------- 4: the accumulator
def test_the_accumulator_on_the_device_against_the_oracles_figures():
    S, C, n = 64, 3, 9
    rng = np.random.RandomState(LC.seed_of("accumulator", (S, C, n)))
    boxes = np.full((n, 3, 4), -1.0, dtype=np.float32)
    for i in range(n):
        for g in range(i % 4):                                          # images 0, 4, 8 have no object
            boxes[i, g] = (rng.uniform(0, 0.5), rng.uniform(0, 0.5), rng.uniform(0.1, 0.45), rng.uniform(0.1, 0.45))
    a = np.clip(rng.standard_normal((n, C, S, S)) * 0.5, -1, 1).astype(np.float32)
    b = np.clip(a + rng.standard_normal((n, C, S, S)).astype(np.float32) * 0.1, -1, 1).astype(np.float32)
    b[5] = a[5]                                                         # one unchanged pair
    results = []
    for sums in (None, LS.sums_numpy):
        for step in (3, 4):
            acc = LS.ShiftResponse(S, C, n + 1, None, 1, 5, DEV, sums=sums, keep=2)
            for at in range(0, n, step):
                table = acc.edits(torch.from_numpy(boxes[at:at + step]), min(step, n - at))
                acc.add(torch.from_numpy(a[at:at + step]).to(DEV), torch.from_numpy(b[at:at + step]).to(DEV), table)
            results.append((acc.result(3), acc.raw(), [v[:2] for v in acc.kept]))
    (dev3, raw3, kept3), (dev4, raw4, kept4), (ora3, oraw, okept), _ = results
    assert json.dumps(dev3, sort_keys=True) == json.dumps(dev4, sort_keys=True)            # the same bits in batches of 3 and of 4
    assert (raw3[0].view(np.int64) == raw4[0].view(np.int64)).all() and (raw3[1] == oraw[1]).all()
    assert (dev3["n_pairs"], dev3["no_objects"], dev3["n_images"], dev3["unchanged"]) == (6, 3, 9, 1)
    edit = np.array([e["rect"] + e["offset"] for e in acc.info])
    bound = LC.bound_of(oraw[0], oraw[1], edit, C)
    assert (np.abs(raw3[0] - oraw[0]) <= bound).all()
    # a figure is a ratio of sums each within rel = (n + 4) 2^-52 of the oracle's: within 3 rel of it, and a mean of such figures too
    rel = 3 * float((LC.addends(oraw[1], edit, C) + 4).max()) * LC.EPS
    for name in ("follow", "locality", "spill_others", "spill_background"):
        assert dev3[name]["n"] == ora3[name]["n"] and abs(dev3[name]["mean"] - ora3[name]["mean"]) <= rel * max(1.0, abs(ora3[name]["mean"])) * 4
    assert dev3["area_share"] == ora3["area_share"] and [e["pair"] for e in dev3["most_ignored"]] == [e["pair"] for e in ora3["most_ignored"]]
    assert kept3 and [p for _, p in kept3] == [e["pair"] for e in dev3["most_ignored"]][:2]
