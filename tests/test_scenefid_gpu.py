"""-m gpu: the object-level Frechet distance on the device -- mogan_roi_resize (csrc/mogan_roi.hip) through ctypes in guard-banded,
poisoned memory against the numpy oracle (tests/scenefid_cases.py: cases and the derived bound), repeatability, the op and its
out= argument; the exact cases bit for bit; what the kernel does with a list the op would have refused; condGANTrainer.scene_fid end
to end (directly, and with --fid through main.py in one pass).  No bound here comes from the code under test."""
import json
import os

import numpy as np
import pytest
import torch

import fid_cases as K
import memguard as MG
import scenefid_cases as S
from eval_setup import tiny_checkpoint as _tiny_checkpoint, trainer as _trainer
from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import scenefid as SF  # noqa: E402
from mogan_amd.hip import lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FULL = (slice(None),)


def _frozen(a):
    """an input in guarded memory: fp32 as it is, anything else as its bytes"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        t = torch.from_numpy(a).to(DEV)
        return MG.Guarded(tuple(t.shape), FULL, DEV, base=t)
    t = torch.from_numpy(a.view(np.uint8).reshape(-1)).to(DEV)
    return MG.Guarded(tuple(t.shape), FULL, DEV, dtype=torch.uint8, base=t)


def _t(a):
    return torch.from_numpy(np.array(a))


class Crop:
    """one call of mogan_roi_resize with every buffer guarded: run() -> y (R, C, OH, OW) on the host, after the memory contract"""

    def __init__(self, x, boxes, index, OH, OW):
        self.B, self.C, self.H, self.W = x.shape
        self.R, self.OH, self.OW = len(index), OH, OW
        self.inputs = {"x": _frozen(x), "boxes": _frozen(boxes), "image_index": _frozen(np.asarray(index, dtype=np.int32))}
        self.y = MG.Guarded((self.R, self.C, OH, OW), FULL, DEV)

    def run(self, what, expect=None, **kw):
        i = self.inputs
        rc = lib.load().mogan_roi_resize(i["x"].ptr, self.B, self.C, self.H, self.W, i["boxes"].ptr, i["image_index"].ptr, self.R,
                                         self.y.ptr, self.OH, self.OW, lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0
        for name, g in i.items():
            assert g.untouched(), "%s: %s or its bands were modified" % (what, name)
        self.y.check(expect, what=what, **kw)                          # nothing outside, every element written, the values
        return self.y.view.cpu().numpy()

    def again(self, what):
        self.y.reset()
        return self.run(what)


def _bits_equal(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    bad = np.argwhere(got.view(np.int32) != want.view(np.int32))
    assert not len(bad), "%s: %d of %d values differ, first at %s: got %r, want %r" % (what, len(bad), got.size, tuple(bad[0]),
                                                                                     got[tuple(bad[0])], want[tuple(bad[0])])


# ------------------------------------------------------------------------------------------------- 1: the kernel's cases
@pytest.mark.parametrize("name", list(S.KERNEL_CASES))
def test_the_crop_against_the_oracle_in_guarded_memory(name):
    x, boxes, index, OH, OW, want = S.kernel_case(name)
    R, C = len(index), x.shape[1]
    run = Crop(x, boxes, index, OH, OW)
    tol = S.tol_blend(x)
    got = run.run(name, _t(want), atol=tol)
    print("%s: off the oracle by %.3e (bound %.3e = %d x 2^-24 max|x|)" % (name, np.abs(got - want).max(), tol, S.TOL_BLEND_ULPS))
    absent = boxes[:, 2] <= 0
    assert absent.any() or name == "one block"
    assert not got[absent].view(np.int32).any() and all(got[r].any() for r in np.flatnonzero(~absent))     # zeros, +0.0 at that
    _bits_equal(run.again(name + ", second call"), got, "second call")
    # the op is the entry: host boxes and index (int32 and int64), a tensor of its own or rows of a larger buffer
    tx, tb, ti = _t(x).to(DEV), _t(boxes), _t(index)
    _bits_equal(ops.roi_resize(tx, tb, ti, OH, OW).cpu().numpy(), got, "ops.roi_resize")
    _bits_equal(ops.roi_resize(tx, tb, ti.long(), OH, OW).cpu().numpy(), got, "ops.roi_resize, int64 index")
    larger = MG.Guarded((R + 2, C, OH, OW), (slice(0, R),), DEV)
    out = ops.roi_resize(tx, tb, ti, OH, OW, out=larger.view)
    torch.cuda.synchronize()
    assert out.data_ptr() == larger.view.data_ptr()
    larger.check(_t(got), exact=True, what=name + ", out= on the leading rows")                          # the other rows untouched
    assert torch.equal(tx.cpu(), _t(x))


# ------------------------------------------------------------------------------------------------- 2: the exact cases
@pytest.mark.parametrize("name", list(S.EXACT_CASES))
def test_the_exact_cases_bit_for_bit(name):
    x, boxes, index, OH, OW, want = S.exact_case(name)
    run = Crop(x, boxes, index, OH, OW)
    got = run.run(name, _t(want.astype(np.float32)), exact=True)
    _bits_equal(run.again(name + ", second call"), got, "second call")
    _bits_equal(ops.roi_resize(_t(x).to(DEV), _t(boxes), _t(index), OH, OW).cpu().numpy(), got, "ops.roi_resize")


def test_a_list_the_op_would_refuse_gives_zeros_and_reads_nothing_else():
    """the entry is safe by construction: a box value that is not finite, a w or h that is not positive, an image index outside
    [0, B) -- each gets zeros in its slab, the rows around it their crops"""
    x = np.random.RandomState(S.seed_of("safe", 0)).uniform(-1, 1, (2, 3, 9, 8)).astype(np.float32)
    good = (0.1, 0.2, 0.5, 0.6)
    boxes = np.array([good, (0.1, np.nan, 0.5, 0.5), (np.inf, 0.1, 0.5, 0.5), (0.1, 0.1, -np.inf, 0.5), (0.1, 0.1, 0.0, 0.5),
                      (0.1, 0.1, 0.5, -0.5), good, good, good, good, S.ABSENT, good], dtype=np.float32)
    index = np.array([0, 1, 0, 1, 0, 1, 2, -1, 1 << 30, -(1 << 31), 0, 1], dtype=np.int32)
    want = S.roi_resize_oracle(x, boxes, index, 6, 5)
    assert [bool(w.any()) for w in want] == [True] + [False] * 10 + [True]
    got = Crop(x, boxes, index, 6, 5).run("unsafe list", _t(want), atol=S.tol_blend(x))
    assert not got[1:11].view(np.int32).any()
    assert torch.equal(ops.roi_resize(_t(x).to(DEV), _t(boxes[:0]), _t(index[:0]), 6, 5).cpu(), torch.zeros(0, 3, 6, 5))
    tx = _t(x).to(DEV)
    for args in ((tx, _t(boxes), _t(index)), (tx, _t(boxes[:1]).to(DEV), _t(index[:1])), (tx, _t(boxes[:1]), _t(index[:1]).to(DEV)),
                 (tx[:, :, :, ::2], _t(boxes[:1]), _t(index[:1]))):
        with pytest.raises(ValueError):
            ops.roi_resize(*args, 6, 5)
    with pytest.raises(ValueError):
        ops.roi_resize(tx, _t(boxes[:1]), _t(index[:1]), 6, 5, out=torch.zeros(1, 3, 6, 5))                  # out on the host


# ------------------------------------------------------------------------------------------------- 3: end to end
FIELDS = {"scene_fid", "mean_sq", "tr_s1", "tr_s2", "tr_sqrt", "n_objects", "n_images", "min_side", "seed", "NET_G", "NET_E",
          "trunk_digest", "note"}


def _check_json(out, ckpt, seed, n):
    path = os.path.join(ckpt[:-4], "valid", "scene_fid.json")
    assert os.path.isfile(path) and json.load(open(path)) == out
    assert set(out) == FIELDS
    assert (out["n_objects"], out["n_images"], out["min_side"], out["seed"], out["NET_G"], out["NET_E"]) == (n, 12, 1.0, seed, ckpt, '')
    assert len(out["trunk_digest"]) == 64 and "rank-deficient" in out["note"] and "n = %d < 2048" % n in out["note"]
    assert "The boxes are the data's on both sides" in out["note"]
    assert out["scene_fid"] == out["mean_sq"] + out["tr_s1"] + out["tr_s2"] - 2.0 * out["tr_sqrt"]


def test_scene_fid_end_to_end(tmp_path, capsys, monkeypatch):
    from mogan_amd.attngan import fid as FID
    cfg, ev, ckpt = _tiny_checkpoint(tmp_path)
    try:
        algo = _trainer(tmp_path, length=12)
        want_index, want_box = SF.object_list(S.loader_boxes(12, 7).view(12, 3, 4), 12, 256)     # the data set's own boxes
        n = int(want_index.shape[0])
        assert 24 <= n <= 36
        seen = []
        make = algo.scene_fid_objects

        def recording(*args, **kw):
            acc = make(*args, **kw)
            sink = acc.sink

            def object_sink(real, fake, tm, take, image_encoder):
                seen.append((real[:take].clone(), image_encoder))
                sink(real, fake, tm, take, image_encoder)
            acc.sink = object_sink
            return acc
        monkeypatch.setattr(algo, "scene_fid_objects", recording)
        out, codes = algo.scene_fid("test", seed=100, return_codes=True)
        monkeypatch.setattr(algo, "scene_fid_objects", make)
        text = capsys.readouterr().out
        assert "SceneFID (%d objects of 12 images" % n in text and "rank-deficient" in text
        _check_json(out, ckpt, 100, n)
        # the object list is the data's: image order then slot order, the boxes as boxes_from_theta gives them back
        assert codes["image"].tolist() == want_index.tolist()
        assert float((codes["box"].double() - want_box.double()).abs().max()) <= 4 * S.EPS
        assert torch.equal(codes["box"][:, 2:], want_box[:, 2:])
        assert tuple(codes["real"].shape) == (n, 2048) == tuple(codes["fake"].shape) and codes["real"].dtype == torch.float32
        assert not torch.equal(codes["real"], codes["fake"])
        # the reported distance against numpy.cov of the returned codes, within the project's end-to-end bound
        want, terms = FID.frechet_distance(*K.stats64(codes["real"].numpy()), *K.stats64(codes["fake"].numpy()))
        scale = terms["tr_s1"] + terms["tr_s2"]
        print("end to end: scene_fid %.9e, from numpy.cov %.9e, apart by %.3e of Tr S1 + Tr S2 (FD_E2E_TOL %.2e)"
              % (out["scene_fid"], want, abs(out["scene_fid"] - want) / scale, K.FD_E2E_TOL))
        assert abs(out["scene_fid"] - want) <= K.FD_E2E_TOL * scale
        # the real codes are the trunk's on the crops of the pass's real images, at the pass's batch shape, bit for bit
        assert len(seen) == 3
        reals, enc = torch.cat([s[0] for s in seen]), seen[0][1]
        with torch.no_grad():
            crops = ops.roi_resize(reals, codes["box"], codes["image"], 299, 299)
            mine = []
            for s in range(0, n, 4):
                batch = torch.zeros((4, 3, 299, 299), device=DEV)
                k = min(4, n - s)
                batch[:k] = crops[s:s + k]
                mine.append(enc.pool_code(batch)[:k])
        assert torch.equal(torch.cat(mine).cpu(), codes["real"])
        # the parameters of a handed-over accumulator are checked, and a pass without two objects has no covariance
        acc = algo.scene_fid_objects(seed=100, min_side=1)
        for kw in (dict(seed=101), dict(min_side=2)):
            with pytest.raises(ValueError, match="other parameters"):
                algo.scene_fid("test", **dict(dict(seed=100, min_side=1, objects=acc), **kw))
        with pytest.raises(ValueError, match="two at least"):
            algo.scene_fid("test", seed=100, objects=acc)
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.FLAG = '', True


def test_main_scene_fid_and_fid_in_one_pass(tmp_path):
    from mogan_amd.attngan import main as entry
    cfg, ev, ckpt = _tiny_checkpoint(tmp_path)
    try:
        base = ["--cfg", str(ev), "--synthetic", "12", "--manualSeed", "7", "--output_dir", str(tmp_path)]
        paths = [os.path.join(ckpt[:-4], "valid", n) for n in ("fid.json", "scene_fid.json")]
        entry.main(base + ["--scene_fid", "--fid"])
        both = [open(p, "rb").read() for p in paths]
        out = json.loads(both[1])
        assert set(out) == FIELDS and out["seed"] == 7 and out["n_images"] == 12 and 24 <= out["n_objects"] <= 36
        for p in paths:
            os.remove(p)
        entry.main(base + ["--fid"])
        assert not os.path.exists(paths[1])
        assert open(paths[0], "rb").read() == both[0]               # the crops draw nothing: fid.json keeps its bytes
        os.remove(paths[0])
        entry.main(base + ["--scene_fid"])
        assert not os.path.exists(paths[0])
        assert open(paths[1], "rb").read() == both[1]               # scene_fid.json alone keeps the bytes of the shared pass
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.FLAG = '', True
