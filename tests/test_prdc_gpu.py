"""-m gpu: the precision / recall / density / coverage path on the device -- mogan_knn_sqdist_f64 and mogan_ball_count_f64 through
ctypes in guard-banded, poisoned memory against the longdouble oracle (tests/prdc_cases.py: cases, seeds, RADII_TOL, MARGIN), the
exact cases bit for bit, repeatability, the two contract properties (a distance's bits depend on the two rows only: permutation,
symmetry, a bit copy at exactly 0); ops.knn_sqdist / ops.ball_counts; condGANTrainer.prdc end to end (directly, and with --fid --kid
through main.py in one pass).  No bound here comes from the code under test.

The fp64 and int32 outputs live in memguard.Guarded's byte mode as in tests/test_kid_gpu.py: a buffer of the output's bytes between
bands of 1024 bytes (8-byte alignment kept); Guarded is asked for the outside of the slice only and the runs look for doubles /
ints that are still 0xFF in every byte (a NaN no kernel computes; a count of -1).  The fp64 radius tables are held bit for bit in
a byte Guarded too."""
import json
import os

import numpy as np
import pytest
import torch

import memguard as MG
import prdc_cases as P
from eval_setup import tiny_checkpoint as _tiny_checkpoint, trainer as _trainer
from helpers import load_pkg

load_pkg()
from mogan_amd.hip import lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FULL = (slice(None),)
CASES = list(P.CASES)
SIDES = {"support": 0, "query": 1}


def _frozen(a):
    """a host array (fp32, or fp64 as bytes) in guarded device memory, bit for bit"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        t = torch.from_numpy(np.array(a)).to(DEV)
        return MG.Guarded(tuple(t.shape), FULL, DEV, base=t)
    assert a.dtype == np.float64
    t = torch.from_numpy(np.array(a)).view(torch.uint8).flatten().to(DEV)
    return MG.Guarded(tuple(t.shape), FULL, DEV, dtype=torch.uint8, base=t)


def _shares(rows, cols):
    tr, tc = (rows + 63) // 64, (cols + 63) // 64
    return max(1, min(-(-512 // tr), tc, 64))


class _Run:
    """the memory contract around a call: outputs and workspace as poisoned byte buffers inside bands, inputs bitwise frozen"""

    def finish(self, what, out, width, names):
        assert self.call() == 0
        out.check(what=what + " output", written=False)                          # nothing outside the output changed
        never = out.view.view(torch.int64 if width == 8 else torch.int32) == -1
        assert not bool(never.any()), "%s: %d outputs never written (first at %d)" % (what, int(never.sum()),
                                                                                      int(torch.nonzero(never)[0]))
        self.ws.check(what=what + " ws", written=False)                          # nothing outside the workspace changed
        for name, g in zip(names, self.inputs):
            assert g.untouched(), "%s: %s or its bands were modified" % (what, name)


class Knn(_Run):
    def __init__(self, x, K):
        self.N, self.D, self.K = x.shape[0], x.shape[1], int(K)
        self.inputs = [_frozen(x)]
        self.ws_bytes = int(lib.load().mogan_knn_sqdist_ws_bytes(self.N, self.K))
        assert self.ws_bytes == 8 * (self.N + _shares(self.N, self.N) * self.N * self.K)
        self.out = MG.Guarded((8 * self.N * self.K,), FULL, DEV, dtype=torch.uint8)
        self.ws = MG.Guarded((self.ws_bytes,), FULL, DEV, dtype=torch.uint8)

    def call(self):
        rc = lib.load().mogan_knn_sqdist_f64(self.inputs[0].ptr, self.N, self.D, self.K, self.out.ptr, self.ws.ptr, self.ws_bytes,
                                             lib.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def run(self, what):
        """out (N, K) fp64 on the host"""
        self.finish(what, self.out, 8, ("x",))
        return self.out.view.view(torch.float64).view(self.N, self.K).cpu().numpy()

    def again(self, what):
        self.out.reset()
        self.ws.reset()
        return self.run(what)


class Ball(_Run):
    def __init__(self, q, p, r2, side):
        r2 = np.asarray(r2, dtype=np.float64)
        r2 = r2[:, None] if r2.ndim == 1 else r2
        self.M, self.N, self.D, self.R, self.side = q.shape[0], p.shape[0], q.shape[1], r2.shape[1], SIDES[side]
        assert r2.shape[0] == (self.N if side == "support" else self.M)
        self.inputs = [_frozen(q), _frozen(p), _frozen(r2)]
        self.ws_bytes = int(lib.load().mogan_ball_count_ws_bytes(self.M, self.N, self.R))
        assert self.ws_bytes == 8 * (self.M + self.N) + (4 * _shares(self.M, self.N) * self.M * self.R + 7) // 8 * 8
        self.count = MG.Guarded((4 * self.M * self.R,), FULL, DEV, dtype=torch.uint8)
        self.ws = MG.Guarded((self.ws_bytes,), FULL, DEV, dtype=torch.uint8)

    def call(self):
        q, p, r2 = self.inputs
        rc = lib.load().mogan_ball_count_f64(q.ptr, self.M, p.ptr, self.N, self.D, r2.ptr, self.R, self.side, self.count.ptr,
                                             self.ws.ptr, self.ws_bytes, lib.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def run(self, what):
        """count (M, R) int32 on the host"""
        self.finish(what, self.count, 4, ("q", "p", "r2"))
        return self.count.view.view(torch.int32).view(self.M, self.R).cpu().numpy()

    def again(self, what):
        self.count.reset()
        self.ws.reset()
        return self.run(what)


def _same_counts(got, want, what):
    bad = np.argwhere(got != want)
    assert not len(bad), "%s: %d of %d counts differ, first at %s: got %d, want %d" % (what, len(bad), got.size, tuple(bad[0]),
                                                                                       got[tuple(bad[0])], want[tuple(bad[0])])


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    bad = np.argwhere(got.view(np.int64) != want.view(np.int64))
    assert not len(bad), "%s: %d of %d doubles differ, first at %s: got %r, want %r" % (what, len(bad), got.size, tuple(bad[0]),
                                                                                        got[tuple(bad[0])], want[tuple(bad[0])])


# ------------------------------------------------------------------------------------------------- 1: the kernels, per element
@pytest.mark.parametrize("case", CASES, ids=[str(c) for c in CASES])
def test_radii_against_longdouble_in_guarded_memory(case):
    ref = P.reference(case)
    for s in ref["radii"]:
        run = Knn(ref[s], ref["K"][s])
        out = run.run("%s %s" % (case, s))
        assert np.isfinite(out).all() and (out >= 0).all() and (np.diff(out, axis=1) >= 0).all()
        err = np.abs(out.astype(P.LD) - ref["radii"][s]) / np.take_along_axis(ref["mag"][(s, s)], ref["order"][s], axis=1)
        print("%s %s (%d rows, K = %d): worst %.3e of A (RADII_TOL %.2e)" % (case, s, out.shape[0], out.shape[1],
                                                                             float(err.max()), P.RADII_TOL))
        bad = np.argwhere(~(err <= P.RADII_TOL))
        assert not len(bad), "%d radii off, first at %s: got %r, want %r" % (len(bad), tuple(bad[0]), out[tuple(bad[0])],
                                                                            float(ref["radii"][s][tuple(bad[0])]))
        _same_bits(run.again("%s %s, second call" % (case, s)), out, "second call")


@pytest.mark.parametrize("case", CASES, ids=[str(c) for c in CASES])
def test_counts_equal_the_oracle_in_guarded_memory(case):
    """every problem of the case, both values of `side`: every query, every column"""
    ref = P.reference(case)
    assert {side for _, _, _, _, side in P.problems(case)} == set(SIDES)
    for name, q, p, of, side in P.problems(case):
        run = Ball(ref[q], ref[p], ref["given"][of], side)
        what = "%s %s (%s)" % (case, name, side)
        got = run.run(what)
        print("%s: %d x %d counts, largest %d, %d queries counted nowhere" % (what, got.shape[0], got.shape[1], got.max(),
                                                                          int((got == 0).all(axis=1).sum())))
        _same_counts(got, ref["counts"][name], what)
        _same_counts(run.again(what + ", second call"), got, "second call")


@pytest.mark.parametrize("case", list(P.EXACT_CASES), ids=str)
def test_exact_cases_bit_for_bit(case):
    ref = P.exact_reference(case)
    for s in ("x", "y"):
        out = Knn(ref[s], ref["K"][s]).run("exact %s %s" % (case, s))
        _same_bits(out, ref["radii"][s].astype(np.float64), "exact %s radii of %s" % (case, s))
    for name, q, p, of, side in P.problems(case):
        got = Ball(ref[q], ref[p], ref["given"][of], side).run("exact %s %s" % (case, name))
        _same_counts(got, ref["counts"][name], "exact %s %s" % (case, name))            # ties d2 = r2 included
    if case == P.DUP_CASE:
        K = case[3]
        out = Knn(ref["x"], K).run("duplicates")
        assert (out[list(P.DUP_AT)] == 0).all()                      # the K other copies are the K nearest, each at exactly 0
        zero = Ball(ref["y"], ref["x"], np.zeros(case[0]), "support").run("duplicates, radius 0")
        assert zero[P.DUP_QUERY, 0] == K + 1                         # the query is a bit copy of each of the K + 1 copies
        _same_counts(zero, P.counts_of(ref["d2"][("y", "x")], np.zeros(case[0]), "support"), "duplicates, radius 0")


# ------------------------------------------------------------------------------------------------- 2: the contract properties
@pytest.mark.parametrize("case", [(67, 100, 80, 5), (130, 200, 100, 3), (96, 96, 2048, 5)], ids=str)
def test_a_permutation_of_the_rows_permutes_the_radii_bitwise(case):
    x, K = P.reference(case)["x"], case[3]
    out = Knn(x, K).run("in order")
    perm = np.random.RandomState(11).permutation(x.shape[0])
    assert (perm != np.arange(x.shape[0])).any() and (perm // 64 != np.arange(x.shape[0]) // 64).any()      # rows change tiles
    _same_bits(Knn(x[perm], K).run("permuted"), out[perm], "permuted %s" % (case,))


@pytest.mark.parametrize("case", [(67, 100, 80, 5), (130, 200, 100, 3)], ids=str)
def test_distances_are_symmetric_bitwise(case):
    """seen through ball_counts(x, x) under knn_sqdist(x)'s OWN radii.  Side "query": the ball of row j under its k-th radius holds
    j itself and its k nearest, k + 1 exactly -- the k-th neighbour only if the distance the count forms has the radius's bits.
    Side "support": count[j] - 1 is the number of i != j whose k-ball holds j, which the oracle knows; i's k-th neighbour is in i's
    ball only if d2(j, i), formed with j as the query, has the bits of d2(i, j), formed with i as the row.  The oracle's rows have no
    ties and every other decision is MARGIN away from its radius (asserted here, from the oracle alone)."""
    ref = P.reference(case)
    x, K, n = ref["x"], case[3], case[0]
    d2, mag, radii, order = ref["d2"][("x", "x")], ref["mag"][("x", "x")], ref["radii"]["x"], ref["order"]["x"]
    cols = [k - 1 for k in P.ks(K)]
    out = Knn(x, K).run("radii")
    own = np.ascontiguousarray(out[:, cols])
    by_query = Ball(x, x, own, "query").run("symmetry, query")
    by_support = Ball(x, x, own, "support").run("symmetry, support")
    for c, col in enumerate(cols):
        gap = np.abs(d2 - radii[:, col:col + 1]) / mag                # row i against its own radius
        gap[np.arange(n), order[:, col]] = np.inf                    # the k-th neighbour itself: equality, by symmetry
        assert gap.min() >= P.MARGIN
        inside = d2 <= radii[:, col:col + 1]                         # inside[i, j]: j in the k-ball of i (i itself included)
        assert (inside.sum(axis=1) == col + 2).all()
        _same_counts(by_query[:, c], inside.sum(axis=1), "%s query k = %d" % (case, col + 1))
        _same_counts(by_support[:, c], inside.sum(axis=0), "%s support k = %d" % (case, col + 1))
    assert (by_query == np.array(cols) + 2).all()


def test_a_bit_copy_is_at_distance_zero_on_non_integer_inputs():
    """rows of y replaced by bit copies of rows of x from both tiles; under a radius table of zeros exactly those are counted,
    once -- with either side owning the radius, and with the copy as the query or as the support point"""
    ref = P.reference((67, 100, 80, 5))
    x, y = ref["x"], np.array(ref["y"])
    pairs = {5: 66, 70: 2, 99: 64, 64: 63}                           # row of y -> row of x
    for j, i in pairs.items():
        y[j] = x[i]
    assert (x != np.round(x)).any() and (ref["d2"][("x", "x")] + np.eye(67) > 0).all()       # no two rows of x coincide
    want = np.zeros((100, 1), dtype=np.int64)
    want[list(pairs)] = 1
    _same_counts(Ball(y, x, np.zeros(67), "support").run("copies, support"), want, "copies as queries, support")
    _same_counts(Ball(y, x, np.zeros(100), "query").run("copies, query"), want, "copies as queries, query")
    back = np.zeros((67, 1), dtype=np.int64)
    back[list(pairs.values())] = 1
    _same_counts(Ball(x, y, np.zeros(100), "support").run("copies as support"), back, "copies as support points")
    # and inside one set: the copies are each other's nearest neighbour at exactly 0
    both = np.concatenate([x, y[list(pairs)]])
    out = Knn(both, 1).run("copies in one set")
    twins = list(pairs.values()) + list(range(67, 67 + len(pairs)))
    assert (out[twins, 0] == 0).all() and (np.delete(out[:, 0], twins) > 0).all()


# ------------------------------------------------------------------------------------------------- 3: the ops
def test_ops_match_the_entry_points_and_raise():
    case = (67, 100, 80, 5)
    ref = P.reference(case)
    x, y = torch.from_numpy(np.array(ref["x"])).to(DEV), torch.from_numpy(np.array(ref["y"])).to(DEV)
    for K in (1, 5, 8):
        out = ops.knn_sqdist(x, K)
        assert out.dtype == torch.float64 and tuple(out.shape) == (67, K) and out.is_cuda and not out.requires_grad
        _same_bits(out.cpu().numpy(), Knn(ref["x"], K).run("op K = %d" % K), "knn_sqdist K = %d" % K)
    grad = x.clone().requires_grad_(True)
    assert not ops.knn_sqdist(grad, 3).requires_grad                 # no gradient
    given = ref["given"]["x"]
    r2 = torch.from_numpy(np.array(given)).to(DEV)
    for q, p, table, side in ((y, x, r2, "support"), (x, y, r2, "query")):
        count = ops.ball_counts(q, p, table, side)
        assert count.dtype == torch.int32 and tuple(count.shape) == (q.shape[0], 4) and count.is_cuda
        want = Ball(q.cpu().numpy(), p.cpu().numpy(), given, side).run("op %s" % side)
        _same_counts(count.cpu().numpy(), want, "ball_counts %s" % side)
    assert torch.equal(ops.ball_counts(y, x, r2), ops.ball_counts(y, x, r2, "support"))          # the default side
    one = r2[:, 3].contiguous()                                      # 1-D radii for R = 1
    count = ops.ball_counts(y, x, one)
    assert tuple(count.shape) == (100, 1) and torch.equal(count[:, 0], ops.ball_counts(y, x, r2)[:, 3])
    # nothing is converted for the caller
    wide = torch.cat([x, x], dim=1)
    for bad, K in ((x.double(), 3), (x.half(), 3), (x[0], 3), (x.view(67, 8, 10), 3), (wide[:, ::2], 3), (x, 0), (x, 9), (x, -1),
                   (x[:5], 5), (x[:1], 1), (ref["x"], 3)):
        with pytest.raises(ValueError):
            ops.knn_sqdist(bad, K)
    assert tuple(ops.knn_sqdist(x[:6].contiguous(), 5).shape) == (6, 5)                         # K = N - 1 is the limit
    rq = torch.zeros((100, 2), dtype=torch.float64, device=DEV)
    for q, p, table, side in ((y.double(), x, r2, "support"), (y, x.half(), r2, "support"),     # wrong dtype of the codes
                              (y, x, r2.float(), "support"), (y, x, r2.long(), "support"),      # ... of the radii
                              (y[0], x, r2, "support"), (y, x.view(67, 8, 10), r2, "support"),  # wrong rank
                              (y, x, r2.view(67, 2, 2), "support"), (y, x, r2[0, 0], "support"),
                              (y, torch.cat([x, x], dim=1), r2, "support"),                     # width mismatch
                              (wide[:, ::2], x, r2, "support"), (y, x, r2[:, ::2], "support"),  # non-contiguous
                              (y, x, r2.t(), "support"),
                              (y.cpu(), x, r2, "support"), (y, x.cpu(), r2, "support"), (y, x, r2.cpu(), "support"),   # other device
                              (y, x, rq, "support"), (y, x, r2, "query"),                       # the radii are the other side's
                              (y, x, torch.cat([r2, r2[:, :1]], dim=1), "support"),             # R = 5
                              (y, x, r2[:, :0], "support"), (y, x, r2, "both"), (y, x, r2, 0)):
        with pytest.raises(ValueError):
            ops.ball_counts(q, p, table, side)


# ------------------------------------------------------------------------------------------------- 4: end to end
FIELDS = {"precision", "recall", "density", "coverage", "k_pr", "k_dc", "n_real", "n_fake", "seed", "NET_G", "NET_E", "trunk_digest",
          "note"}
SCORES = ("precision", "recall", "density", "coverage")


def _check_json(out, ckpt, seed, n, k_pr, k_dc, lowered):
    path = os.path.join(ckpt[:-4], "valid", "prdc.json")
    assert os.path.isfile(path) and json.load(open(path)) == out
    assert set(out) == FIELDS
    assert out["n_real"] == out["n_fake"] == n and out["seed"] == seed and out["NET_G"] == ckpt and out["NET_E"] == ''
    assert out["k_pr"] == k_pr and out["k_dc"] == k_dc and len(out["trunk_digest"]) == 64
    assert "random-init" in out["note"] and "ImageNet" in out["note"] and "comparable at equal n only" in out["note"]
    assert ("lowered" in out["note"]) == lowered
    for name in ("precision", "recall", "coverage"):
        assert 0.0 <= out[name] <= 1.0 and abs(out[name] * n - round(out[name] * n)) < 1e-9
    assert out["density"] >= 0.0


def test_prdc_end_to_end(tmp_path, capsys):
    cfg, ev, ckpt = _tiny_checkpoint(tmp_path)
    try:
        algo = _trainer(tmp_path)
        for seed in (100, 101, 102, 103):
            out, codes = algo.prdc("test", seed=seed, return_codes=True)
            assert "PRDC (12 real, 12 generated images; k = 3 / 5): precision" in capsys.readouterr().out
            real, fake = codes["real"].numpy(), codes["fake"].numpy()
            assert real.shape == fake.shape == (12, 2048) and real.dtype == np.float32 and not (real == fake).all()
            margin = P.prdc_margin(real, fake, 3, 5)
            print("seed %d: the closest decision on the returned codes is %.3e A from its radius (MARGIN %.0e)" % (seed, margin, P.MARGIN))
            if margin >= P.MARGIN:                                  # else this run cannot be held to equality: the next seed
                break
        else:
            pytest.fail("no seed whose codes keep every decision MARGIN away from its radius")
        _check_json(out, ckpt, seed, 12, 3, 5, lowered=False)
        want = P.prdc_numpy(real, fake, 3, 5)
        print("end to end: %s\nfrom numpy: %s" % ({k: out[k] for k in SCORES}, want))
        assert {k: out[k] for k in SCORES} == want                  # ratios of small integers: exactly
        out2, codes2 = algo.prdc("test", seed=seed, return_codes=True)                          # same seed, same JSON
        assert out2 == out and torch.equal(codes2["fake"], codes["fake"]) and torch.equal(codes2["real"], codes["real"])
        # handed-over codes: no pass of its own; with 5 images a side k_dc is lowered to 4 and the JSON says so
        digest = out["trunk_digest"]
        few = {"real": codes["real"][:5].to(DEV), "fake": codes["fake"][:5].to(DEV), "n": 5, "trunk_digest": digest, "seed": seed}
        low = algo.prdc("test", seed=seed, codes=few)
        _check_json(low, ckpt, seed, 5, 3, 4, lowered=True)
        assert "k_dc lowered from 5 to 4" in low["note"] and "k_pr lowered" not in low["note"]
        assert "k_dc = 4 instead of 5" in capsys.readouterr().out
        if P.prdc_margin(real[:5], fake[:5], 3, 4) >= P.MARGIN:
            assert {k: low[k] for k in SCORES} == P.prdc_numpy(real[:5], fake[:5], 3, 4)
        # a random-init generator's images are nowhere near the data and score 0 throughout; the same path on handed-over codes
        # whose decisions are mixed (the D = 2048 case: every margin is asserted by the CPU module)
        ref = P.reference((96, 96, 2048, 5))
        mixed = {"real": torch.from_numpy(np.array(ref["x"])).to(DEV), "fake": torch.from_numpy(np.array(ref["y"])).to(DEV), "n": 96,
                 "trunk_digest": digest, "seed": seed}
        got = algo.prdc("test", seed=seed, codes=mixed)
        want = P.prdc_numpy(ref["x"], ref["y"], 3, 5)
        print("mixed: %s" % ({k: got[k] for k in SCORES},))
        assert {k: got[k] for k in SCORES} == want and all(0.0 < want[k] < 1.0 for k in SCORES)
        _check_json(got, ckpt, seed, 96, 3, 5, lowered=False)
        with pytest.raises(ValueError, match="seed"):
            algo.prdc("test", seed=seed + 1, codes=few)
        with pytest.raises(ValueError, match="no real side"):
            algo.prdc("test", seed=seed, codes=dict(few, real=None))
        with pytest.raises(ValueError, match="two at least"):
            algo.prdc("test", seed=seed, codes=dict(few, n=1))
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.FLAG = '', True


def test_main_fid_kid_and_prdc_in_one_pass(tmp_path, monkeypatch):
    from mogan_amd.attngan import main as entry
    from mogan_amd.attngan import model
    cfg, ev, ckpt = _tiny_checkpoint(tmp_path)
    images, pool_code = [], model.CNN_ENCODER.pool_code

    def counted(self, x):
        images.append(int(x.shape[0]))
        return pool_code(self, x)
    monkeypatch.setattr(model.CNN_ENCODER, "pool_code", counted)
    try:
        base = ["--cfg", str(ev), "--synthetic", "12", "--manualSeed", "7", "--output_dir", str(tmp_path), "--kid_subsets", "5"]
        entry.main(base + ["--fid", "--kid", "--prdc", "--prdc_k_dc", "4"])
        assert sum(images) == 24 and len(images) == 6               # 12 real and 12 generated images, once each, in batches of 4
        paths = [os.path.join(ckpt[:-4], "valid", n) for n in ("fid.json", "kid.json", "prdc.json")]
        with_prdc = [open(p, "rb").read() for p in paths[:2]]
        _check_json(json.load(open(paths[2])), ckpt, 7, 12, 3, 4, lowered=False)
        for p in paths:
            os.remove(p)
        del images[:]
        entry.main(base + ["--fid", "--kid"])
        assert sum(images) == 24 and not os.path.exists(paths[2])
        assert [open(p, "rb").read() for p in paths[:2]] == with_prdc      # fid.json and kid.json keep their bytes
        del images[:]
        entry.main(base + ["--prdc"])                                # alone: a pass of its own
        assert sum(images) == 24 and len(images) == 6
        _check_json(json.load(open(paths[2])), ckpt, 7, 12, 3, 5, lowered=False)
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.FLAG = '', True
