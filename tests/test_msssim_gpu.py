"""-m gpu: MS-SSIM on the device -- the entries of csrc/mogan_ssim.hip through ctypes in guard-banded, poisoned memory against the
numpy fp64 oracle (tests/msssim_cases.py: cases, seeds, bounds), the two bit-level properties and repeatability at every case; the
ops; attngan/msssim.PairSimilarity against the oracle's terms and score; condGANTrainer.msssim end to end (directly, and with --swd
through main.py in one pass).  No bound here comes from the code under test.

fp32 outputs live in memguard.Guarded's float mode (slice poisoned, 1024 sentinels on both sides), the fp64 terms and the workspace
in its byte mode as in tests/test_swd_gpu.py.  Every input is held bit for bit."""
import json
import os

import numpy as np
import pytest
import torch

import memguard as MG
import msssim_cases as S
from eval_setup import tiny_checkpoint as _tiny_checkpoint, trainer as _trainer
from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import msssim as MS  # noqa: E402
from mogan_amd.hip import lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FULL = (slice(None),)


def _frozen(a):
    t = torch.from_numpy(np.array(a, dtype=np.float32)).to(DEV)
    return MG.Guarded(tuple(t.shape), FULL, DEV, base=t)


def _t(a):
    return torch.from_numpy(np.array(a))


def _bits_equal(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape
    view = np.int64 if got.dtype == np.float64 else np.int32
    bad = np.argwhere(got.view(view) != want.view(view))
    assert not len(bad), "%s: %d of %d values differ, first at %s: got %r, want %r" % (what, len(bad), got.size, tuple(bad[0]),
                                                                                     got[tuple(bad[0])], want[tuple(bad[0])])


class Level:
    """one call of mogan_ssim_level_f64 with every buffer guarded: run() -> (terms (P, 2) fp64, ssim_map, cs_map) on the host"""

    def __init__(self, a, b, win):
        self.P, self.C, self.S, _ = a.shape
        self.n = len(win)
        self.M = self.S - self.n + 1
        self.inputs = {"a": _frozen(a), "b": _frozen(b), "win": _frozen(win)}
        self.ws_bytes = int(lib.load().mogan_ssim_level_ws_bytes(self.P, self.C, self.S, self.n))
        assert self.ws_bytes == 16 * self.P * self.C * (-(-self.M // S.TILE)) ** 2
        self.terms = MG.Guarded((16 * self.P,), FULL, DEV, dtype=torch.uint8)
        self.ws = MG.Guarded((self.ws_bytes,), FULL, DEV, dtype=torch.uint8)
        self.maps = [MG.Guarded((self.P, self.C, self.M, self.M), FULL, DEV) for _ in range(2)]

    def run(self, what, maps=True):
        i = self.inputs
        rc = lib.load().mogan_ssim_level_f64(i["a"].ptr, i["b"].ptr, self.P, self.C, self.S, i["win"].ptr, self.n, self.terms.ptr,
                                             self.maps[0].ptr if maps else None, self.maps[1].ptr if maps else None,
                                             self.ws.ptr, self.ws_bytes, lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0
        for name, g in i.items():
            assert g.untouched(), "%s: %s or its bands were modified" % (what, name)
        self.ws.check(what=what + " ws", written=False)
        never = self.ws.view.view(torch.int64) == -1
        assert not bool(never.any()), "%s: %d workspace doubles never written" % (what, int(never.sum()))
        self.terms.check(what=what + " terms", written=False)
        never = self.terms.view.view(torch.int64) == -1
        assert not bool(never.any()), "%s: %d terms never written" % (what, int(never.sum()))
        for m in self.maps:
            if maps:
                m.check(what=what + " map")                          # nothing outside, every element written
            else:
                assert m.untouched(), "%s: a map that was not handed over was written" % what
        return (self.terms.view.view(torch.float64).cpu().numpy().reshape(self.P, 2),
                self.maps[0].view.cpu().numpy(), self.maps[1].view.cpu().numpy())

    def again(self, what, maps=True):
        for g in [self.terms, self.ws] + self.maps:
            g.reset()
        return self.run(what, maps)


# ------------------------------------------------------------------------------------------------- 1: the 2 x 2 mean
@pytest.mark.parametrize("shape", S.DOWN_SHAPES, ids=str)
def test_avg_down2_bit_for_bit_on_integer_images(shape):
    NC, H, W = shape
    x = S.integer_image(shape, S.seed_of("down", shape))
    want = S.avg_down2(x, np.float32)
    assert np.array_equal(want.astype(np.float64), S.avg_down2(x))              # sums of four integers below 2^10: exact
    gx, out = _frozen(x), MG.Guarded((NC, H // 2, W // 2), FULL, DEV)
    rc = lib.load().mogan_avg_down2(gx.ptr, NC, H, W, out.ptr, lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and gx.untouched()
    out.check(_t(want), exact=True, what="avg_down2 %s" % (shape,))
    assert torch.equal(ops.avg_down2(_t(x).to(DEV)).cpu(), _t(want))


# ------------------------------------------------------------------------------------------------- 2: one level
@pytest.mark.parametrize("case", S.KERNEL_CASES, ids=str)
def test_a_level_against_the_oracle_in_guarded_memory(case):
    a, b, win, ssim, cs, terms = S.kernel_case(case)
    run = Level(a, b, win)
    got_terms, got_ssim, got_cs = run.run("level %s" % (case,))
    print("level %s: ssim map off by %.3e, cs map by %.3e (bound %.3e); terms by %.3e (bound %.3e)"
          % (case, np.abs(got_ssim - ssim).max(), np.abs(got_cs - cs).max(), S.TOL_MAP, np.abs(got_terms - terms).max(), S.TOL_TERM))
    run.maps[0].check(_t(ssim), atol=S.TOL_MAP, what="ssim map %s" % (case,))
    run.maps[1].check(_t(cs), atol=S.TOL_MAP, what="cs map %s" % (case,))
    assert (np.abs(got_terms - terms) <= S.TOL_TERM).all(), (got_terms, terms)
    # a second call gives the same bits; without the maps the terms keep theirs and the maps stay untouched
    t2, s2, c2 = run.again("second call")
    _bits_equal(t2, got_terms, "terms, second call")
    _bits_equal(s2, got_ssim, "ssim map, second call")
    _bits_equal(c2, got_cs, "cs map, second call")
    _bits_equal(run.again("without maps", maps=False)[0], got_terms, "terms without maps")
    # the op is the entry
    ot, os_, oc = ops.ssim_level(_t(a).to(DEV), _t(b).to(DEV), _t(win).to(DEV), maps=True)
    assert torch.equal(ot.cpu(), _t(got_terms)) and torch.equal(os_.cpu(), _t(got_ssim)) and torch.equal(oc.cpu(), _t(got_cs))
    assert torch.equal(ops.ssim_level(_t(a).to(DEV), _t(b).to(DEV), _t(win).to(DEV)).cpu(), _t(got_terms))


@pytest.mark.parametrize("case", S.KERNEL_CASES, ids=str)
def test_a_copy_is_at_exactly_1_and_a_swap_changes_no_bit(case):
    a, b, win, _, _, _ = S.kernel_case(case)
    terms, ssim, cs = Level(a, a.copy(), win).run("copy %s" % (case,))
    assert (terms == 1.0).all() and (ssim == 1.0).all() and (cs == 1.0).all()
    ab = Level(a, b, win).run("a, b")
    ba = Level(b, a, win).run("b, a")
    for x, y, name in zip(ab, ba, ("terms", "ssim map", "cs map")):
        _bits_equal(y, x, "%s after the swap" % name)


def test_ops_refuse_tensors_on_two_devices_and_bad_windows():
    a, w = torch.zeros(2, 3, 16, 16, device=DEV), torch.full((11,), 1 / 11.0, device=DEV)
    for args in ((a, a.cpu(), w), (a, a, w.cpu()), (a, a, torch.zeros(12, device=DEV)), (a, a[:, :, :, ::2], w), (a.double(), a, w)):
        with pytest.raises(ValueError):
            ops.ssim_level(*args)
    with pytest.raises(ValueError):
        ops.avg_down2(torch.zeros(3, 5, 4, device=DEV))


# ------------------------------------------------------------------------------------------------- 3: all levels
def _similarity(case, pairs=S.PAIRS):
    size, L, C = case
    return MS.PairSimilarity(size, C, pairs, scales=L, device=DEV)


@pytest.mark.parametrize("case", S.TOLERANCE_CASES, ids=str)
def test_all_levels_and_the_score_against_the_oracle(case):
    size, L, C = case
    a, b, terms, score = S.tolerance_case(case, S.SEEDS[0])
    assert float(terms.min()) >= S.TERM_FLOOR                       # every pair, every level: the powers are well conditioned
    ta, tb = _t(a).to(DEV), _t(b).to(DEV)
    keep = (ta.clone(), tb.clone())
    ps = _similarity(case, S.PAIRS + 3)
    ps.add(ta[:3].contiguous(), tb[:3].contiguous())                # two batches, a buffer larger than what is added
    ps.add(ta[3:].contiguous(), tb[3:].contiguous())
    assert torch.equal(ta, keep[0]) and torch.equal(tb, keep[1]) and ps.n == S.PAIRS
    got = ps.terms[:ps.n].cpu().numpy()
    got_score = MS.score_from_terms(got)[0]
    print("%s: terms off by %.3e (bound %.3e), the score by %.3e (bound %.3e)"
          % (case, np.abs(got - terms).max(), S.TOL_TERM, np.abs(got_score - score).max(), S.TOL_SCORE))
    assert (np.abs(got - terms) <= S.TOL_TERM).all()
    assert (np.abs(got_score - score) <= S.TOL_SCORE).all()
    res = ps.result()
    assert res["pairs"] == S.PAIRS and res["clamped"] == 0 and res["levels"] == S.sides(size, L)
    assert abs(res["mean"] - score.mean()) <= S.TOL_SCORE and abs(res["std"] - score.std()) <= 2 * S.TOL_SCORE
    assert (np.abs(np.array(res["ssim"]) - terms[:, :, 0].mean(axis=0)) <= S.TOL_TERM).all()
    assert (np.abs(np.array(res["cs"]) - terms[:, :, 1].mean(axis=0)) <= S.TOL_TERM).all()
    # one batch of all pairs gives the bits of the two batches; so does a second run
    one = _similarity(case)
    one.add(ta, tb)
    _bits_equal(one.terms.cpu().numpy(), got, "one batch against two")
    assert one.result() == res
    # a bit copy scores exactly 1 with no spread; the swap keeps every bit
    same = _similarity(case)
    same.add(ta, ta.clone())
    r = same.result()
    assert (same.terms.cpu().numpy() == 1.0).all() and r["mean"] == 1.0 and r["std"] == 0.0 and r["clamped"] == 0
    swapped = _similarity(case)
    swapped.add(tb, ta)
    _bits_equal(swapped.terms.cpu().numpy(), got, "b, a against a, b")


def test_a_negative_level_mean_is_the_devices_too_and_the_clamp_is_the_hosts():
    a, b, terms = S.find_clamp_pair()
    k = S.CLAMP_CASE
    used = np.concatenate([terms[:-1, 1], terms[-1:, 0]])
    assert float(used.min()) < -0.01 and MS.score_from_terms(terms)[0] == 0.0
    good = S.tolerance_case((32, 4, 3), 0)
    ps = MS.PairSimilarity(k["S"], k["C"], 3, scales=k["L"], device=DEV)
    ps.add(_t(np.concatenate([good[0][:1], a, good[0][1:2]])).to(DEV), _t(np.concatenate([good[1][:1], b, good[1][1:2]])).to(DEV))
    got = ps.terms.cpu().numpy()
    assert (np.abs(got[1] - terms) <= S.TOL_TERM).all() and float(got[1].min()) < -0.01        # the device keeps the negative mean
    assert (np.abs(got[[0, 2]] - good[2][:2]) <= S.TOL_TERM).all()
    res = ps.result()
    assert res["clamped"] == 1 and res["pairs"] == 3
    assert abs(res["mean"] - (good[3][0] + 0.0 + good[3][1]) / 3) <= S.TOL_SCORE


# ------------------------------------------------------------------------------------------------- 4: end to end
FIGURE = {"mean", "std", "ssim", "cs", "pairs", "clamped"}
COMMON = {"levels", "scales", "seed", "NET_G", "NET_E", "note"}
LEVELS = [256, 128, 64, 32, 16]


def _oracle_figure(a, b, scales=5):
    terms = S.all_levels(a, b, scales)
    score, clamped = S.score(terms)
    return {"mean": float(score.mean()), "std": float(score.std()), "ssim": terms[:, :, 0].mean(axis=0), "cs": terms[:, :, 1].mean(axis=0),
            "pairs": len(score), "clamped": int(clamped.sum())}


def _check_figure(got, want, what):
    assert set(got) == FIGURE and got["pairs"] == want["pairs"] and got["clamped"] == want["clamped"], what
    print("%s: mean %.6f against %.6f, std %.6f against %.6f" % (what, got["mean"], want["mean"], got["std"], want["std"]))
    assert abs(got["mean"] - want["mean"]) <= S.TOL_SCORE and abs(got["std"] - want["std"]) <= 2 * S.TOL_SCORE, what
    assert (np.abs(np.array(got["ssim"]) - want["ssim"]) <= S.TOL_TERM).all(), what
    assert (np.abs(np.array(got["cs"]) - want["cs"]) <= S.TOL_TERM).all(), what


def test_msssim_end_to_end_against_the_oracle_on_the_images_of_the_pass(tmp_path, capsys, monkeypatch):
    from mogan_amd.attngan.evaluate import CheckpointEvaluation
    cfg, ev, ckpt = _tiny_checkpoint(tmp_path)

    def no_trunk(self):
        raise AssertionError("msssim() alone must not load the image encoder")
    monkeypatch.setattr(CheckpointEvaluation, "_load_image_encoder", no_trunk)
    try:
        algo = _trainer(tmp_path)
        seen = {"real": [], "fake": [], "first": [], "again": []}
        make = algo.msssim_images

        def recording(*args, **kw):
            acc = make(*args, **kw)
            sink, resample = acc.sink, acc.resample_sink

            def image_sink(real, fake, take):
                seen["real"].append(real[:take].float().cpu().numpy())
                seen["fake"].append(fake[:take].float().cpu().numpy())
                sink(real, fake, take)

            def resample_sink(fake, again, take):
                seen["first"].append(fake[:take].float().cpu().numpy())
                seen["again"].append(again[:take].float().cpu().numpy())
                resample(fake, again, take)
            acc.sink, acc.resample_sink = image_sink, resample_sink
            return acc
        monkeypatch.setattr(algo, "msssim_images", recording)
        out = algo.msssim("test", seed=100)
        text = capsys.readouterr().out
        assert "MS-SSIM (5 scales; mean +- std over pairs): real " in text and "same_caption" in text and "(12 pairs)" in text
        path = os.path.join(ckpt[:-4], "valid", "msssim.json")
        assert os.path.isfile(path) and json.load(open(path)) == out
        assert set(out) == COMMON | {"real", "generated", "same_caption"}
        assert (out["levels"], out["scales"], out["seed"], out["NET_G"], out["NET_E"]) == (LEVELS, 5, 100, ckpt, '')
        assert "trunk-free" in out["note"] and "caption length" in out["note"] and "8 bits" in out["note"]
        assert len(seen["real"]) == len(seen["fake"]) == len(seen["again"]) == 3 and all(x.shape == (4, 3, 256, 256) for x in seen["real"])
        for name, key in (("real", "real"), ("generated", "fake")):
            a = np.concatenate([x[:2] for x in seen[key]])                         # row j against row j + take // 2
            b = np.concatenate([x[2:] for x in seen[key]])
            assert out[name]["pairs"] == 6
            _check_figure(out[name], _oracle_figure(a, b), name)
        assert out["same_caption"]["pairs"] == 12
        assert all(np.array_equal(f, g) for f, g in zip(seen["first"], seen["fake"]))               # the image the pass makes anyway
        _check_figure(out["same_caption"], _oracle_figure(np.concatenate(seen["fake"]), np.concatenate(seen["again"])), "same_caption")
        assert not any(np.array_equal(f, g) for f, g in zip(seen["fake"], seen["again"]))           # fresh noise: another image
        monkeypatch.setattr(algo, "msssim_images", make)
        assert algo.msssim("test", seed=100) == out                                                # same seed, same JSON
        few = algo.msssim("test", num_samples=7, seed=100, scales=3, same_caption=False)
        assert set(few) == COMMON | {"real", "generated"} and few["levels"] == [256, 128, 64] and few["real"]["pairs"] == 3
        with pytest.raises(ValueError, match="scales"):
            algo.msssim("test", scales=7)
        acc = algo.msssim_images(seed=100, scales=5)
        for kw in (dict(seed=101), dict(scales=4), dict(same_caption=False)):
            with pytest.raises(ValueError, match="other parameters"):
                algo.msssim("test", **dict(dict(seed=100, scales=5, same_caption=True, images=acc), **kw))
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.FLAG = '', True


def test_main_msssim_and_swd_in_one_pass(tmp_path):
    from mogan_amd.attngan import main as entry
    cfg, ev, ckpt = _tiny_checkpoint(tmp_path)
    try:
        base = ["--cfg", str(ev), "--synthetic", "12", "--manualSeed", "7", "--output_dir", str(tmp_path), "--swd_patches", "16",
                "--swd_dirs", "16", "--swd_repeats", "2"]
        paths = [os.path.join(ckpt[:-4], "valid", n) for n in ("swd.json", "msssim.json")]
        entry.main(base + ["--swd", "--msssim"])
        both = [open(p, "rb").read() for p in paths]
        out = json.loads(both[1])
        assert set(out) == COMMON | {"real", "generated", "same_caption"} and out["seed"] == 7
        assert (out["real"]["pairs"], out["generated"]["pairs"], out["same_caption"]["pairs"]) == (6, 6, 12)
        for p in paths:
            os.remove(p)
        entry.main(base + ["--swd"])                                # alone: no second image is drawn
        assert not os.path.exists(paths[1])
        assert open(paths[0], "rb").read() == both[0]               # the resample draws from a generator of its own
        os.remove(paths[0])
        entry.main(base + ["--msssim"])
        assert not os.path.exists(paths[0])
        assert open(paths[1], "rb").read() == both[1]               # msssim.json alone keeps the bytes of the shared pass
        os.remove(paths[1])
        entry.main(base + ["--msssim", "--msssim_no_resample"])
        less = json.load(open(paths[1]))
        assert set(less) == COMMON | {"real", "generated"}
        assert less["real"] == out["real"] and less["generated"] == out["generated"]
        os.remove(paths[1])
        entry.main(base + ["--msssim", "--msssim_scales", "3"])
        assert json.load(open(paths[1]))["levels"] == [256, 128, 64]
        for other in ("--sampling", "--r_precision"):
            with pytest.raises(SystemExit):
                entry.parse_args(["--msssim", other])
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.FLAG = '', True
