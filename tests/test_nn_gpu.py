"""-m gpu: nearest training neighbours on the device -- mogan_knn_cross_f64 through ctypes in guard-banded, poisoned memory against
the longdouble oracle (tests/nn_cases.py: cases, seeds, DIST_TOL, MARGIN): distances within the bound, positions EQUAL; the exact
cases bit for bit, ties across tiles and shares included; repeatability; the contract properties (the distances are
mogan_knn_sqdist_f64's bits, symmetric in the two sets, a permutation of the bank permutes the positions, a bit copy is at exactly
0); ops.knn_cross; condGANTrainer.memorisation end to end (directly, with planted copies, and with --fid --prdc through main.py in
one pass).  No bound here comes from the code under test.

The fp64 and int32 outputs live in memguard.Guarded's byte mode as in tests/test_prdc_gpu.py: a buffer of the output's bytes
between bands of 1024 bytes; Guarded is asked for the outside of the slice only and the runs look for doubles / ints that are
still 0xFF in every byte (a NaN no kernel computes; a position of -1)."""
import json
import os

import numpy as np
import pytest
import torch

import memguard as MG
import nn_cases as C
import prdc_cases as P
from eval_setup import tiny_checkpoint as _tiny_checkpoint, trainer as _trainer
from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import memorisation as MEM  # noqa: E402
from mogan_amd.attngan.fid import NeighbourBank  # noqa: E402
from mogan_amd.hip import lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FULL = (slice(None),)
CASES = list(C.CASES)


def _frozen(a):
    """a host fp32 array in guarded device memory, bit for bit"""
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    t = torch.from_numpy(np.array(a)).to(DEV)
    return MG.Guarded(tuple(t.shape), FULL, DEV, base=t)


class Cross:
    """the memory contract around a call: outputs and workspace as poisoned byte buffers inside bands, inputs bitwise frozen"""

    def __init__(self, q, p, K):
        self.M, self.N, self.D, self.K = q.shape[0], p.shape[0], q.shape[1], int(K)
        assert p.shape[1] == self.D
        self.inputs = [_frozen(q), _frozen(p)]
        self.ws_bytes = int(lib.load().mogan_knn_cross_ws_bytes(self.M, self.N, self.K))
        assert self.ws_bytes == C.ws_bytes(self.M, self.N, self.K)
        self.d2 = MG.Guarded((8 * self.M * self.K,), FULL, DEV, dtype=torch.uint8)
        self.idx = MG.Guarded((4 * self.M * self.K,), FULL, DEV, dtype=torch.uint8)
        self.ws = MG.Guarded((self.ws_bytes,), FULL, DEV, dtype=torch.uint8)

    def call(self):
        q, p = self.inputs
        rc = lib.load().mogan_knn_cross_f64(q.ptr, self.M, p.ptr, self.N, self.D, self.K, self.d2.ptr, self.idx.ptr, self.ws.ptr,
                                            self.ws_bytes, lib.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def run(self, what):
        """(d2 (M, K) fp64, idx (M, K) int32) on the host"""
        assert self.call() == 0
        for out, width, name in ((self.d2, torch.int64, "d2"), (self.idx, torch.int32, "idx")):
            out.check(what="%s %s" % (what, name), written=False)                # nothing outside the output changed
            never = out.view.view(width) == -1
            assert not bool(never.any()), "%s: %d of %s never written (first at %d)" % (what, int(never.sum()), name,
                                                                                      int(torch.nonzero(never)[0]))
        self.ws.check(what=what + " ws", written=False)                          # nothing outside the workspace changed
        for name, g in zip(("q", "p"), self.inputs):
            assert g.untouched(), "%s: %s or its bands were modified" % (what, name)
        return (self.d2.view.view(torch.float64).view(self.M, self.K).cpu().numpy(),
                self.idx.view.view(torch.int32).view(self.M, self.K).cpu().numpy())

    def again(self, what):
        self.d2.reset()
        self.idx.reset()
        self.ws.reset()
        return self.run(what)


def _same_ints(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s, want %s" % (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert not len(bad), "%s: %d of %d positions differ, first at %s: got %d, want %d" % (what, len(bad), got.size, tuple(bad[0]),
                                                                                          got[tuple(bad[0])], want[tuple(bad[0])])


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, "%s: shape %s, want %s" % (what, got.shape, want.shape)
    bad = np.argwhere(got.view(np.int64) != want.view(np.int64))
    assert not len(bad), "%s: %d of %d doubles differ, first at %s: got %r, want %r" % (what, len(bad), got.size, tuple(bad[0]),
                                                                                        got[tuple(bad[0])], want[tuple(bad[0])])


def _knn_sqdist(x, K):
    """mogan_knn_sqdist_f64 on x: (N, K) fp64 on the host"""
    return ops.knn_sqdist(torch.from_numpy(np.array(x)).to(DEV), K).cpu().numpy()


# ------------------------------------------------------------------------------------------------- 1: the kernel, per element
@pytest.mark.parametrize("case", CASES, ids=[str(c) for c in CASES])
def test_neighbours_against_longdouble_in_guarded_memory(case):
    ref = C.reference(case)
    run = Cross(ref["q"], ref["p"], case[3])
    d2, idx = run.run(str(case))
    assert d2.dtype == np.float64 and idx.dtype == np.int32
    assert np.isfinite(d2).all() and (d2 >= 0).all() and (np.diff(d2, axis=1) >= 0).all()
    err = np.abs(d2.astype(C.LD) - ref["d2"]) / ref["mag"]
    print("%s (%d queries, %d bank rows, K = %d, %d shares): worst %.3e of A (DIST_TOL %.2e)"
          % (case, case[0], case[1], case[3], C.shares(case[0], case[1]), float(err.max()), C.DIST_TOL))
    _same_ints(idx, ref["idx"], "%s positions" % (case,))                       # every query, every column
    bad = np.argwhere(~(err <= C.DIST_TOL))
    assert not len(bad), "%d distances off, first at %s: got %r, want %r" % (len(bad), tuple(bad[0]), d2[tuple(bad[0])],
                                                                            float(ref["d2"][tuple(bad[0])]))
    d2_again, idx_again = run.again("%s, second call" % (case,))
    _same_bits(d2_again, d2, "second call")
    _same_ints(idx_again, idx, "second call")


@pytest.mark.parametrize("case", list(C.EXACT_CASES), ids=str)
def test_exact_cases_bit_for_bit(case):
    """integer distances: numpy fp64's bits and the stable argsort's positions, ties across tiles and shares included"""
    ref = C.exact_reference(case)
    want_d2, want_idx = C.nearest(P.numpy_fp64_d2(ref["q"], ref["p"]), case[3])
    assert (want_idx == ref["idx"]).all()
    run = Cross(ref["q"], ref["p"], case[3])
    d2, idx = run.run("exact %s" % (case,))
    _same_bits(d2, want_d2, "exact %s distances" % (case,))
    _same_ints(idx, want_idx, "exact %s positions" % (case,))
    d2_again, idx_again = run.again("exact %s, second call" % (case,))
    _same_bits(d2_again, d2, "second call")
    _same_ints(idx_again, idx, "second call")
    if case == (70, 67, 48, 5):
        assert (d2[P.DUP_QUERY] == 0).all() and list(idx[P.DUP_QUERY]) == sorted(P.DUP_AT)[:5]
    for K in (1, 3):                                                 # a smaller K reports the head of the same list
        d2_k, idx_k = Cross(ref["q"], ref["p"], K).run("exact %s K = %d" % (case, K))
        _same_bits(d2_k, want_d2[:, :K], "K = %d" % K)
        _same_ints(idx_k, want_idx[:, :K], "K = %d" % K)


# ------------------------------------------------------------------------------------------------- 2: the contract properties
@pytest.mark.parametrize("case", [(100, 67, 80, 5), (200, 130, 100, 3), (9, 200, 24, 8), (96, 96, 2048, 5)], ids=str)
def test_the_bank_against_itself_gives_knn_sqdist_bits(case):
    """x against x with K + 1 neighbours: every row finds itself at exactly 0 first, and what remains once position i is left out
    is mogan_knn_sqdist_f64's row i bit for bit -- the two entry points form the same distances"""
    K = min(case[3], 7)
    x = C.reference(case)["p"]
    n = x.shape[0]
    d2, idx = Cross(x, x, K + 1).run("%s bank against itself" % (case,))
    _same_ints(idx[:, 0], np.arange(n), "a row's nearest bank row is itself")
    assert (d2[:, 0] == 0).all()
    _same_bits(d2[:, 1:], _knn_sqdist(x, K), "%s: the others' distances" % (case,))
    assert (idx[:, 1:] != np.arange(n)[:, None]).all()


@pytest.mark.parametrize("case", [(100, 67, 80, 5), (200, 130, 100, 3)], ids=str)
def test_distances_are_symmetric_bitwise(case):
    """d2 of (q = x, p = y) and of (q = y, p = x): a pair both calls report has the same bits in both"""
    ref = C.reference(case)
    x, y, K = ref["p"], ref["q"], case[3]
    d_xy, i_xy = Cross(x, y, K).run("x against y")
    d_yx, i_yx = Cross(y, x, K).run("y against x")
    both = 0
    for a in range(x.shape[0]):
        for col, b in enumerate(i_xy[a]):
            back = np.nonzero(i_yx[b] == a)[0]
            if len(back):
                both += 1
                assert d_xy[a, col].view(np.int64) == d_yx[b, back[0]].view(np.int64), (a, b, d_xy[a, col], d_yx[b, back[0]])
    print("%s: %d pairs reported from both sides" % (case, both))
    assert both > 0


@pytest.mark.parametrize("case", [(100, 67, 80, 5), (9, 200, 24, 8), (3, 1100, 8, 8)], ids=str)
def test_a_permutation_of_the_bank_permutes_the_positions(case):
    """no ties in these cases (the CPU module asserts the gaps): d2 keeps its bits and idx follows the rows"""
    ref = C.reference(case)
    q, p, K = ref["q"], ref["p"], case[3]
    d2, idx = Cross(q, p, K).run("in order")
    perm = np.random.RandomState(11).permutation(p.shape[0])         # new row r holds old row perm[r]
    assert (perm // 64 != np.arange(p.shape[0]) // 64).any()         # rows change tiles
    d2_p, idx_p = Cross(q, p[perm], K).run("permuted")
    _same_bits(d2_p, d2, "permuted %s" % (case,))
    _same_ints(perm[idx_p], idx, "permuted %s" % (case,))


def test_a_bit_copy_of_a_bank_row_is_at_exactly_zero():
    ref = C.reference((100, 67, 80, 5))
    q, p = np.array(ref["q"]), ref["p"]
    pairs = {5: 66, 70: 2, 99: 64, 64: 63}                           # query -> bank row, from both tiles
    for j, i in pairs.items():
        q[j] = p[i]
    assert (p != np.round(p)).any()
    d2, idx = Cross(q, p, 5).run("copies")
    for j, i in pairs.items():
        assert d2[j, 0] == 0 and idx[j, 0] == i and d2[j, 1] > 0
    others = np.delete(np.arange(100), list(pairs))
    assert (d2[others, 0] > 0).all()
    _same_ints(idx[others], ref["idx"][others], "the other queries")


# ------------------------------------------------------------------------------------------------- 3: the op
def test_op_matches_the_entry_point_and_raises():
    case = (100, 67, 80, 5)
    ref = C.reference(case)
    q, p = torch.from_numpy(np.array(ref["q"])).to(DEV), torch.from_numpy(np.array(ref["p"])).to(DEV)
    for K in (1, 5, 8):
        d2, idx = ops.knn_cross(q, p, K)
        assert d2.dtype == torch.float64 and idx.dtype == torch.int32 and tuple(d2.shape) == tuple(idx.shape) == (100, K)
        assert d2.is_cuda and idx.is_cuda and not d2.requires_grad
        want_d2, want_idx = Cross(ref["q"], ref["p"], K).run("op K = %d" % K)
        _same_bits(d2.cpu().numpy(), want_d2, "knn_cross K = %d" % K)
        _same_ints(idx.cpu().numpy(), want_idx, "knn_cross K = %d" % K)
    _same_ints(ops.knn_cross(q, p, 5)[1].cpu().numpy(), ref["idx"], "knn_cross against the oracle")
    grad = q.clone().requires_grad_(True)
    assert not ops.knn_cross(grad, p, 3)[0].requires_grad            # no gradient
    assert tuple(ops.knn_cross(q, p[:5].contiguous(), 5)[0].shape) == (100, 5)                   # K = N is the limit
    wide = torch.cat([p, p], dim=1)
    for bad_q, bad_p, K in ((q.double(), p, 3), (q, p.half(), 3), (q[0], p, 3), (q, p.view(67, 8, 10), 3), (q, wide, 3),
                            (q, wide[:, ::2], 3), (q.cpu(), p, 3), (q, p.cpu(), 3), (q, p, 0), (q, p, 9), (q, p, -1), (q, p[:4], 5),
                            (ref["q"], p, 3)):
        with pytest.raises(ValueError):
            ops.knn_cross(bad_q, bad_p, K)


# ------------------------------------------------------------------------------------------------- 4: end to end
FIELDS = {"authenticity", "authentic", "authenticity_heldout", "authentic_heldout", "copying", "copying_less", "copying_equal",
          "copying_pairs", "n_bank", "k", "bank_path", "bank_split", "show", "most_suspicious", "grid", "n_real", "n_fake", "seed",
          "NET_G", "NET_E", "trunk_digest", "note"}
SCORES = ("authenticity", "authentic", "authenticity_heldout", "authentic_heldout", "copying", "copying_less", "copying_equal",
          "copying_pairs")


def _numpy_scores(fake, real, bank, k):
    """(the figures, d2_f (n, k), idx_f (n, k), nn_bank) by attngan/memorisation.py on numpy fp64 distances"""
    d2_f, idx_f = C.nearest(P.numpy_fp64_d2(fake, bank), k)
    d2_h, idx_h = C.nearest(P.numpy_fp64_d2(real, bank), 1)
    nn_bank = P.knn_of(P.numpy_fp64_d2(bank, bank), 1)[0][:, 0]
    return MEM.scores(d2_f[:, 0], idx_f[:, 0], d2_h[:, 0], idx_h[:, 0], nn_bank), d2_f, idx_f, nn_bank


def _margin(fake, real, bank, k):
    """the smallest relative distance in longdouble of any decision behind _numpy_scores from equality: neighbours' order,
    authenticity of both sides, and the pairs of the Mann-Whitney count"""
    d_pp, a_pp = P.oracle_d2(bank, bank)
    nn, nn_at = P.knn_of(d_pp, 1)
    worst = np.inf
    nearest = []
    for codes, kk in ((fake, k), (real, 1)):
        d, a = P.oracle_d2(codes, bank)
        worst = min(worst, C.neighbour_gap(d, a, kk))
        top, order = C.nearest(d, 1)
        t = order[:, 0]
        scale = np.maximum(np.take_along_axis(a, order, axis=1)[:, 0], a_pp[t, nn_at[t, 0]])
        worst = min(worst, float((np.abs(top[:, 0] - nn[t, 0]) / scale).min()))
        nearest.append((top[:, 0], np.take_along_axis(a, order, axis=1)[:, 0]))
    (f, af), (h, ah) = nearest
    worst = min(worst, float((np.abs(f[:, None] - h[None, :]) / np.maximum(af[:, None], ah[None, :])).min()))
    return worst


def _check_json(out, ckpt, seed, n, n_bank, k, show):
    path = os.path.join(ckpt[:-4], "valid", "memorisation.json")
    assert os.path.isfile(path) and json.load(open(path)) == out
    assert set(out) == FIELDS
    assert out["n_real"] == out["n_fake"] == n and out["seed"] == seed and out["NET_G"] == ckpt and out["NET_E"] == ''
    assert out["n_bank"] == n_bank and out["k"] == k and out["show"] == len(out["most_suspicious"]) == show
    assert len(out["trunk_digest"]) == 64
    assert "random-init" in out["note"] and "ImageNet" in out["note"] and "depends on n_bank: comparable at equal bank only" in out["note"]
    assert out["authenticity"] == out["authentic"] / n and out["authenticity_heldout"] == out["authentic_heldout"] / n
    assert out["copying"] == (2 * out["copying_less"] + out["copying_equal"]) / (2 * out["copying_pairs"]) and out["copying_pairs"] == n * n
    for e in out["most_suspicious"]:
        assert len(e["d2"]) == len(e["bank_rows"]) == len(e["bank_positions"]) == k and e["d2"] == sorted(e["d2"])


def test_memorisation_end_to_end(tmp_path, capsys):
    from PIL import Image
    cfg, ev, ckpt = _tiny_checkpoint(tmp_path)
    try:
        algo = _trainer(tmp_path)
        for seed in (100, 101, 102, 103):
            bank = algo.neighbour_bank(seed=seed, bank_size=10)       # batches of 4: the last one is filled up
            assert len(bank) == 10 and bank.split == "synthetic-train" and bank.codes.shape == (10, 2048)
            assert list(bank.positions) == list(range(10)) and bank.codes.dtype == np.float32
            out, codes = algo.memorisation("test", seed=seed, bank=bank, k=3, show=4, return_codes=True)
            assert ("Memorisation (12 generated, 12 held-out real images against 10 training images; k = 3): authenticity"
                    in capsys.readouterr().out)
            real, fake, T = codes["real"].numpy(), codes["fake"].numpy(), codes["bank"].numpy()
            assert real.shape == fake.shape == (12, 2048) and T.shape == (10, 2048) and (T == bank.codes).all()
            margin = _margin(fake, real, T, 3)
            print("seed %d: the closest decision on the returned codes is %.3e A from equality (MARGIN %.0e)" % (seed, margin, C.MARGIN))
            if margin >= C.MARGIN:                                   # else this run cannot be held to equality: the next seed
                break
        else:
            pytest.fail("no seed whose codes keep every decision MARGIN away from equality")
        _check_json(out, ckpt, seed, 12, 10, 3, 4)
        assert out["bank_split"] == "synthetic-train" and out["bank_path"] is None and "second synthetic set" in out["note"]
        assert out["trunk_digest"] == bank.trunk_digest and out["grid"] == "nn_grid.png"
        grid = Image.open(os.path.join(ckpt[:-4], "valid", "nn_grid.png"))
        assert grid.size == (4 * 64, 4 * 64) and grid.mode == "RGB"                # 4 rows of [generated | 3 training images]
        assert np.asarray(grid).std() > 0
        for e in out["most_suspicious"]:
            assert e["bank_keys"] == ['synthetic_%06d' % p for p in e["bank_positions"]] and e["bank_rows"] == e["bank_positions"]
        want, d2_f, idx_f, nn_bank = _numpy_scores(fake, real, T, 3)
        print("end to end: %s\nfrom numpy: %s" % ({s: out[s] for s in SCORES}, want))
        assert {s: out[s] for s in SCORES} == want                   # ratios of integers: exactly
        rows, ratio = MEM.most_suspicious(d2_f[:, 0], idx_f[:, 0], nn_bank, 4)
        assert [e["row"] for e in out["most_suspicious"]] == list(rows)
        assert [e["bank_rows"] for e in out["most_suspicious"]] == [list(idx_f[r]) for r in rows]
        # the same seed gives the same JSON; a file bank is saved, loaded, and refused for another trunk
        path = str(tmp_path / "bank.npz")
        bank.save(path)
        again = algo.memorisation("test", seed=seed, bank_path=path, k=3, show=4)
        assert "Load the training bank from" in capsys.readouterr().out
        assert {s: again[s] for s in SCORES} == {s: out[s] for s in SCORES} and again["most_suspicious"] == out["most_suspicious"]
        assert again["bank_path"] == path
        NeighbourBank(bank.codes, bank.positions, "0" * 64, bank.split).save(path)
        handed = {"real": codes["real"].to(DEV), "fake": codes["fake"].to(DEV), "n": 12, "seed": seed, "trunk_digest": out["trunk_digest"]}
        with pytest.raises(ValueError, match="another Inception trunk"):
            algo.memorisation("test", seed=seed, bank_path=path, k=3, show=0, codes=handed)
        with pytest.raises(ValueError, match="another Inception trunk"):
            algo.memorisation("test", seed=seed, bank=NeighbourBank(bank.codes, bank.positions, "0" * 64, bank.split), show=0,
                              codes=handed)
        none = algo.memorisation("test", seed=seed, bank=bank, k=3, show=0, codes=handed)           # show = 0: no list, no grid
        assert none["grid"] is None and none["most_suspicious"] == [] and {s: none[s] for s in SCORES} == want
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.FLAG = '', True


def test_memorisation_finds_planted_copies(tmp_path):
    """handed-over codes on the D = 2048 case, whose margins the CPU module asserts: the first half of `fake` are bit copies of
    chosen bank rows"""
    cfg, ev, ckpt = _tiny_checkpoint(tmp_path)
    try:
        algo = _trainer(tmp_path)
        ref = C.reference((96, 96, 2048, 5))
        T, q = ref["p"], ref["q"]
        n, half = 96, 48
        planted = np.random.RandomState(5).permutation(96)[:half]
        fake = np.array(q)
        fake[:half] = T[planted]
        real = np.array(q)                                           # the held-out side: the queries as they were
        digest = "1" * 64
        bank = NeighbourBank(T, np.arange(96) * 3, digest, "planted")
        codes = {"real": torch.from_numpy(real).to(DEV), "fake": torch.from_numpy(fake).to(DEV), "n": n, "seed": 100,
                 "trunk_digest": digest}
        out = algo.memorisation("test", seed=100, bank=bank, k=5, show=half + 2, codes=codes)
        _check_json(out, ckpt, 100, n, 96, 5, half + 2)
        assert out["grid"] is None and out["bank_split"] == "planted"
        flags, margin = C.authentic(ref)
        assert margin >= C.MARGIN
        remaining = int(flags[half:].sum())
        assert out["authentic"] == remaining and out["authenticity"] == remaining / n            # no copy is authentic
        assert 0 < remaining < n - half
        head = out["most_suspicious"][:half]
        assert [e["row"] for e in head] == list(range(half)) and all(e["ratio"] == 0 and e["d2"][0] == 0 for e in head)
        assert [e["bank_rows"][0] for e in head] == list(planted)
        assert [e["bank_positions"][0] for e in head] == list(planted * 3) and "bank_keys" not in head[0]
        assert all(e["ratio"] > 0 for e in out["most_suspicious"][half:])
        assert out["authentic_heldout"] == int(flags.sum()) and out["authenticity_heldout"] == int(flags.sum()) / n
        # copying, from the oracle alone: a copy is closer than every held-out code; the other rows ARE the held-out rows, so each
        # meets its own distance once (a genuine tie) and every other pair is MARGIN apart
        d, a = ref["d2"][:, 0], ref["mag"][:, 0]
        gap = np.abs(d[:, None] - d[None, :]) / np.maximum(a[:, None], a[None, :]) + np.eye(n)
        assert gap.min() >= C.MARGIN and (d > 0).all()
        less = half * n + int((d[half:, None] < d[None, :]).sum())
        assert (out["copying_less"], out["copying_equal"], out["copying_pairs"]) == (less, n - half, n * n)
        assert out["copying"] == (2 * less + n - half) / (2 * n * n) and out["copying"] > 0.5
        # k is lowered to the bank's size, and the JSON says so
        low = algo.memorisation("test", seed=100, bank=bank, bank_size=3, k=5, show=2, codes=codes)
        _check_json(low, ckpt, 100, n, 3, 3, 2)
        assert "k lowered from 5 to 3" in low["note"]
        with pytest.raises(ValueError, match="seed"):
            algo.memorisation("test", seed=101, bank=bank, codes=codes)
        with pytest.raises(ValueError, match="no real side"):
            algo.memorisation("test", seed=100, bank=bank, codes=dict(codes, real=None))
        with pytest.raises(ValueError, match="two at least"):
            algo.memorisation("test", seed=100, bank=bank, bank_size=1, codes=codes)
        with pytest.raises(ValueError):
            algo.memorisation("test", seed=100, bank=bank, k=9, codes=codes)
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.FLAG = '', True


def test_main_memorisation_fid_and_prdc_in_one_pass(tmp_path):
    from mogan_amd.attngan import main as entry
    cfg, ev, ckpt = _tiny_checkpoint(tmp_path)
    try:
        base = ["--cfg", str(ev), "--synthetic", "12", "--manualSeed", "7", "--output_dir", str(tmp_path)]
        paths = [os.path.join(ckpt[:-4], "valid", n) for n in ("fid.json", "prdc.json", "memorisation.json", "nn_grid.png")]
        entry.main(base + ["--fid", "--prdc"])
        alone = [open(p, "rb").read() for p in paths[:2]]
        assert not os.path.exists(paths[2])
        for p in paths[:2]:
            os.remove(p)
        bank_path = str(tmp_path / "bank.npz")
        entry.main(base + ["--memorisation", "--fid", "--prdc", "--nn_bank", bank_path, "--nn_k", "2", "--nn_show", "3"])
        assert [open(p, "rb").read() for p in paths[:2]] == alone      # fid.json and prdc.json keep their bytes
        out = json.load(open(paths[2]))
        _check_json(out, ckpt, 7, 12, 12, 2, 3)
        assert os.path.isfile(paths[3]) and os.path.isfile(bank_path) and out["bank_path"] == bank_path
        assert "second synthetic set" in out["note"]
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.FLAG = '', True
