"""-m gpu: the Frechet-distance path on the device -- mogan_col_mean_f64 / mogan_cov_f64 through ctypes in guard-banded, poisoned
memory against the longdouble oracle (tests/fid_cases.py: cases, seeds, MOMENT_TOL), the exact cases bit for bit, symmetry and
repeatability bitwise; ops.feature_moments; CNN_ENCODER.pool_code on both trunk paths; condGANTrainer.fid end to end (directly,
with a statistics file, through main.py).  No bound here comes from the code under test.

The fp64 outputs live in memguard.Guarded's byte mode: a buffer of 8 * count bytes between bands of 1024 bytes (8-byte alignment
kept), viewed as float64.  Guarded's own "never written" test is per byte and a written double may hold a 0xFF byte, so it is asked
for the outside of the slice only and `Run.check_output` looks for doubles that are still 0xFF in every byte."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fid_cases as K
import memguard as MG
from eval_setup import tiny_checkpoint as _tiny_checkpoint, trainer as _trainer
from helpers import load_pkg

load_pkg()
from mogan_amd.hip import lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FULL = (slice(None),)
SHAPES = list(K.CASES)


class Run:
    """one problem in guarded memory: x with bands (bitwise frozen), mean and cov as poisoned byte buffers inside bands"""

    def __init__(self, x):
        self.N, self.D = x.shape
        self.x = MG.Guarded((self.N, self.D), FULL, DEV, base=torch.from_numpy(np.array(x, dtype=np.float32)).to(DEV))
        self.mean = MG.Guarded((8 * self.D,), FULL, DEV, dtype=torch.uint8)
        self.cov = MG.Guarded((8 * self.D * self.D,), FULL, DEV, dtype=torch.uint8)

    def call_mean(self):
        rc = lib.load().mogan_col_mean_f64(self.x.ptr, self.N, self.D, self.mean.ptr, lib.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def call_cov(self):
        rc = lib.load().mogan_cov_f64(self.x.ptr, self.mean.ptr, self.N, self.D, self.cov.ptr, lib.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def f64(self, g):
        return g.view.view(torch.float64)

    def bits(self, g):
        return g.view.view(torch.int64).clone()

    def results(self):
        return self.f64(self.mean).cpu().numpy(), self.f64(self.cov).view(self.D, self.D).cpu().numpy()

    def check_output(self, g, what):
        g.check(what=what, written=False)                                        # nothing outside the output changed
        never = g.view.view(torch.int64) == -1
        assert not bool(never.any()), "%s: %d elements never written (first at %d)" % (what, int(never.sum()),
                                                                                       int(torch.nonzero(never)[0]))

    def moments(self, what):
        """both calls with the memory contract checked around each: (mean, cov) on the host"""
        assert self.call_mean() == 0
        self.check_output(self.mean, what + " mean")
        assert self.cov.untouched() and self.x.untouched(), what + ": the mean call touched cov or x"
        held = self.mean.buf.clone()
        assert self.call_cov() == 0
        self.check_output(self.cov, what + " cov")
        assert torch.equal(self.mean.buf, held), what + ": the cov call modified its mean input or its bands"
        assert self.x.untouched(), what + ": x or its bands were modified"
        return self.results()


# ------------------------------------------------------------------------------------------------- 1: the kernels, per element
@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_moments_against_longdouble_in_guarded_memory(shape):
    ref = K.reference(shape)
    run = Run(ref["x"])
    mean, cov = run.moments(str(shape))
    em = np.abs(mean.astype(K.LD) - ref["mean"]) / np.abs(ref["mean"]).max()
    ec = np.abs(cov.astype(K.LD) - ref["cov"]) / np.abs(ref["cov"]).max()
    print("%s: mean %.3e, cov %.3e of the largest element (MOMENT_TOL %.2e)" % (shape, float(em.max()), float(ec.max()), K.MOMENT_TOL))
    assert np.isfinite(mean).all() and np.isfinite(cov).all()
    assert (em <= K.MOMENT_TOL).all(), "mean: %d elements off, worst %.3e" % (int((em > K.MOMENT_TOL).sum()), float(em.max()))
    bad = np.argwhere(~(ec <= K.MOMENT_TOL))
    assert not len(bad), "cov: %d elements off, first at %s, worst %.3e" % (len(bad), tuple(bad[0]), float(ec.max()))
    assert (cov.view(np.int64) == cov.T.view(np.int64)).all(), "cov is not bitwise symmetric"
    # the same inputs give the same bits on every call
    m1, c1 = run.bits(run.mean), run.bits(run.cov)
    run.mean.reset()
    run.cov.reset()
    run.moments("%s, second call" % (shape,))
    assert torch.equal(run.bits(run.mean), m1) and torch.equal(run.bits(run.cov), c1)


@pytest.mark.parametrize("shape", list(K.EXACT_CASES), ids=str)
def test_exact_cases_bit_for_bit(shape):
    x = K.make_exact_inputs(shape, K.EXACT_CASES[shape])
    mean_ref, cov_ref = K.exact_expected(x)
    mean, cov = Run(x).moments("exact %s" % (shape,))
    assert (mean.view(np.int64) == mean_ref.view(np.int64)).all(), "mean: first off at %s" % (np.argwhere(mean != mean_ref)[:1],)
    bad = np.argwhere(cov.view(np.int64) != cov_ref.view(np.int64))
    assert not len(bad), "cov: %d of %d elements differ, first at %s: got %r, want %r" % (
        len(bad), cov.size, tuple(bad[0]), cov[tuple(bad[0])], cov_ref[tuple(bad[0])])


def test_op_matches_the_entry_points_and_raises():
    shape = (67, 80)
    ref = K.reference(shape)
    m_ref, c_ref = Run(ref["x"]).moments("op")
    x = torch.from_numpy(np.array(ref["x"])).to(DEV)
    mean, cov = ops.feature_moments(x)
    assert mean.dtype == cov.dtype == torch.float64 and tuple(mean.shape) == (80,) and tuple(cov.shape) == (80, 80) and cov.is_cuda
    assert (mean.cpu().numpy().view(np.int64) == m_ref.view(np.int64)).all()
    assert (cov.cpu().numpy().view(np.int64) == c_ref.view(np.int64)).all()
    for bad in (x.double(), x[0], x[:1], x.t(), x[:, ::2], x.view(67, 8, 10)):
        with pytest.raises(ValueError):
            ops.feature_moments(bad)


# ------------------------------------------------------------------------------------------------- 2: the pool code
def _bits32(t):
    return t.detach().contiguous().view(torch.int32)


def test_pool_code_on_both_trunk_paths_and_forward_unchanged(monkeypatch):
    from mogan_amd.attngan import inception, model
    from mogan_amd.attngan.miscc.config import cfg
    cfg.TRAIN.FLAG = True
    torch.manual_seed(3)
    enc = model.CNN_ENCODER(32).to(DEV).eval()
    for p in enc.parameters():
        p.requires_grad = False
    x = (torch.rand(2, 3, 64, 64) * 2 - 1).to(DEV)
    runs, fwd = [], inception.PanelTrunk.forward

    def recorded(self, x299):
        out = fwd(self, x299)
        runs.append((out[1].detach().clone(), out[2].detach().clone()))
        return out
    monkeypatch.setattr(inception.PanelTrunk, "forward", recorded)
    assert inception.FAST_TRUNK and enc._frozen()
    with torch.no_grad():
        f0, c0 = enc(x)
        code = enc.pool_code(x)
        assert len(runs) == 2                                       # one walk of the fast trunk per call
        assert tuple(code.shape) == (2, 2048) and code.dtype == torch.float32
        assert torch.equal(_bits32(enc.emb_cnn_code(code)), _bits32(c0))
        # forward, as it was before pool_code existed: the two heads on the trunk's outputs.  First the same modules (bits), ...
        feat, last = runs[0]
        assert torch.equal(_bits32(enc.emb_features(feat)), _bits32(f0))
        assert torch.equal(_bits32(enc.emb_cnn_code(ops.avg_pool2d(last, 8).view(2, -1))), _bits32(c0))
        # ... then stock torch in fp64.  Both heads are fp32 dot products: 2^-24 sum |a||b| per product sum (include/mogan_hip.h,
        # "Arithmetic"), and the pooled vector carries the roundings of a 64-term fp32 mean besides (6 levels of pairwise adds,
        # 2^-24 each at most, and one division): 8 x 2^-24 sum |a||b| covers both
        feat, last = feat.cpu().double(), last.cpu().double()
        w = {k: p.detach().cpu().double() for k, p in enc.named_parameters() if k.split(".")[0] in enc.HEADS}
        pooled = F.avg_pool2d(last, 8).flatten(1)
        fr = F.conv2d(feat, w["emb_features.weight"])
        cr = F.linear(pooled, w["emb_cnn_code.weight"], w["emb_cnn_code.bias"])
        fb = F.conv2d(feat.abs(), w["emb_features.weight"].abs())
        cb = F.linear(pooled.abs(), w["emb_cnn_code.weight"].abs(), w["emb_cnn_code.bias"].abs())
        assert bool(((f0.cpu().double() - fr).abs() <= 8 * 2.0 ** -24 * fb).all())
        assert bool(((c0.cpu().double() - cr).abs() <= 8 * 2.0 ** -24 * cb).all())
        assert float((code.cpu().double() - pooled).abs().max()) <= 8 * 2.0 ** -24 * float(pooled.abs().max())
        # the module path
        fast, inception.FAST_TRUNK = inception.FAST_TRUNK, False
        try:
            assert not enc._frozen()
            fm, cm = enc(x)
            code_m = enc.pool_code(x)
        finally:
            inception.FAST_TRUNK = fast
        assert len(runs) == 2                                       # (the fast trunk did not run)
        assert tuple(code_m.shape) == (2, 2048)
        assert torch.equal(_bits32(enc.emb_cnn_code(code_m)), _bits32(cm))


# ------------------------------------------------------------------------------------------------- 3: end to end
FIELDS = {"fid", "mean_sq", "tr_s1", "tr_s2", "tr_sqrt", "n_real", "n_fake", "seed", "NET_G", "NET_E", "trunk_digest", "note"}


def _check_json(out, ckpt, seed):
    path = os.path.join(ckpt[:-4], "valid", "fid.json")
    assert os.path.isfile(path) and json.load(open(path)) == out
    assert set(out) == FIELDS
    assert out["n_real"] == out["n_fake"] == 12 and out["seed"] == seed and out["NET_G"] == ckpt and out["NET_E"] == ''
    assert len(out["trunk_digest"]) == 64 and "rank-deficient" in out["note"] and "n = 12 < 2048" in out["note"]
    scale = out["tr_s1"] + out["tr_s2"]
    assert np.isfinite(out["fid"]) and scale > 0 and out["fid"] >= -K.FD_TOL * scale
    assert out["fid"] == out["mean_sq"] + out["tr_s1"] + out["tr_s2"] - 2.0 * out["tr_sqrt"]


def test_fid_end_to_end(tmp_path, capsys):
    from mogan_amd.attngan import fid as FID
    cfg, ev, ckpt = _tiny_checkpoint(tmp_path)
    try:
        algo = _trainer(tmp_path)
        out, codes = algo.fid("test", seed=100, return_codes=True)
        assert "rank-deficient" in capsys.readouterr().out
        _check_json(out, ckpt, 100)
        assert tuple(codes["real"].shape) == (12, 2048) == tuple(codes["fake"].shape) and codes["real"].dtype == torch.float32
        assert not torch.equal(codes["real"], codes["fake"])
        # the reported distance against numpy.cov of the returned codes, within the bound the CPU module measured at this size
        want, terms = FID.frechet_distance(*K.stats64(codes["real"].numpy()), *K.stats64(codes["fake"].numpy()))
        scale = terms["tr_s1"] + terms["tr_s2"]
        print("end to end: fid %.9e, from numpy.cov %.9e, apart by %.3e of Tr S1 + Tr S2 (FD_E2E_TOL %.2e)"
              % (out["fid"], want, abs(out["fid"] - want) / scale, K.FD_E2E_TOL))
        assert abs(out["fid"] - want) <= K.FD_E2E_TOL * scale
        out2, codes2 = algo.fid("test", seed=100, return_codes=True)                 # same seed, same JSON
        assert out2 == out and torch.equal(codes2["fake"], codes["fake"]) and torch.equal(codes2["real"], codes["real"])
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.FLAG = '', True


def test_fid_with_a_statistics_file(tmp_path):
    from mogan_amd.attngan import fid as FID
    cfg, ev, ckpt = _tiny_checkpoint(tmp_path)
    try:
        algo = _trainer(tmp_path)
        stats = str(tmp_path / "real_stats.npz")
        first = algo.fid("test", seed=100, stats_path=stats)
        assert os.path.isfile(stats)
        with np.load(stats) as z:
            assert z["mean"].dtype == z["cov"].dtype == np.float64 and z["cov"].shape == (2048, 2048) and int(z["n"]) == 12
            assert str(z["trunk_digest"]) == first["trunk_digest"]
        again, codes = algo.fid("test", seed=100, stats_path=stats, return_codes=True)  # loaded: the real images skip the trunk
        assert codes["real"] is None and again == first                                # the same distance, bit for bit
        foreign = FID.FeatureStats.load(stats, first["trunk_digest"], 2048)
        foreign.trunk_digest = "0" * 64
        foreign.save(stats)
        with pytest.raises(ValueError, match="another Inception trunk"):
            algo.fid("test", seed=100, stats_path=stats)
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.FLAG = '', True


def test_main_fid_on_synthetic(tmp_path):
    from mogan_amd.attngan import main as entry
    cfg, ev, ckpt = _tiny_checkpoint(tmp_path)
    try:
        stats = str(tmp_path / "s.npz")
        entry.main(["--cfg", str(ev), "--synthetic", "12", "--manualSeed", "7", "--output_dir", str(tmp_path), "--fid",
                    "--fid_stats", stats])
        out = json.load(open(os.path.join(ckpt[:-4], "valid", "fid.json")))
        _check_json(out, ckpt, 7)
        assert os.path.isfile(stats)
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.FLAG = '', True
