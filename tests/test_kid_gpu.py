"""-m gpu: the kernel-Inception-distance path on the device -- mogan_poly3_mmd_f64 through ctypes in guard-banded, poisoned memory
against the longdouble oracle (tests/kid_cases.py: cases, seeds, SUM_TOL), the exact cases bit for bit, repeatability and the
independence of the subset pairs bitwise; ops.poly_mmd_sums; condGANTrainer.kid end to end (directly, and with --fid through main.py
in one pass).  No bound here comes from the code under test.

The fp64 outputs live in memguard.Guarded's byte mode as in tests/test_fid_gpu.py: a buffer of 8 * count bytes between bands of 1024
bytes (8-byte alignment kept), viewed as float64; Guarded is asked for the outside of the slice only and `Run.run` looks for
doubles that are still 0xFF in every byte.  The int32 index tables are held bit for bit in an fp32 Guarded."""
import json
import os

import numpy as np
import pytest
import torch

import kid_cases as K
import memguard as MG
from eval_setup import tiny_checkpoint as _tiny_checkpoint, trainer as _trainer
from helpers import load_pkg

load_pkg()
from mogan_amd.hip import lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FULL = (slice(None),)
CASES = list(K.CASES)


def _frozen(a):
    """a host array (fp32 or int32) in guarded device memory, bit for bit"""
    t = torch.from_numpy(np.array(a)).to(DEV)
    return MG.Guarded(tuple(t.shape), FULL, DEV, base=t if t.dtype == torch.float32 else t.view(torch.float32))


class Run:
    """one problem in guarded memory: x, y, ix, iy with bands (bitwise frozen), sums and ws as poisoned byte buffers inside bands"""

    def __init__(self, x, y, ix, iy, gamma, coef0=1.0):
        self.Nx, self.D = x.shape
        self.Ny = y.shape[0]
        self.S, self.s = ix.shape
        self.gamma, self.coef0 = float(gamma), float(coef0)
        self.inputs = [_frozen(a) for a in (x, y, ix, iy)]
        self.ws_bytes = int(lib.load().mogan_poly3_mmd_ws_bytes(self.S, self.s))
        T = (self.s + 63) // 64
        assert self.ws_bytes == self.S * (T * (T + 1) + T * T) * 8
        self.sums = MG.Guarded((8 * self.S * 3,), FULL, DEV, dtype=torch.uint8)
        self.ws = MG.Guarded((self.ws_bytes,), FULL, DEV, dtype=torch.uint8)

    def call(self):
        x, y, ix, iy = self.inputs
        rc = lib.load().mogan_poly3_mmd_f64(x.ptr, self.Nx, y.ptr, self.Ny, self.D, ix.ptr, iy.ptr, self.S, self.s, self.gamma,
                                            self.coef0, self.sums.ptr, self.ws.ptr, self.ws_bytes, lib.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def bits(self):
        return self.sums.view.view(torch.int64).clone()

    def run(self, what):
        """the call with the memory contract checked around it: sums (S, 3) on the host"""
        assert self.call() == 0
        self.sums.check(what=what + " sums", written=False)                      # nothing outside the output changed
        never = self.sums.view.view(torch.int64) == -1
        assert not bool(never.any()), "%s: %d sums never written (first at %d)" % (what, int(never.sum()), int(torch.nonzero(never)[0]))
        self.ws.check(what=what + " ws", written=False)                          # nothing outside the workspace changed
        for name, g in zip(("x", "y", "ix", "iy"), self.inputs):
            assert g.untouched(), "%s: %s or its bands were modified" % (what, name)
        return self.sums.view.view(torch.float64).view(self.S, 3).cpu().numpy()

    def again(self, what):
        self.sums.reset()
        self.ws.reset()
        return self.run(what)


# ------------------------------------------------------------------------------------------------- 1: the kernel, per sum
@pytest.mark.parametrize("case", CASES, ids=[str(c) for c in CASES])
def test_sums_against_longdouble_in_guarded_memory(case):
    ref = K.reference(case)
    run = Run(ref["x"], ref["y"], ref["ix"], ref["iy"], ref["gamma"])
    sums = run.run(str(case))
    err = np.abs(sums.astype(K.LD) - ref["sums"]) / ref["mag"]
    print("%s: worst %.3e of the sum over |k| (SUM_TOL %.2e); per sum %s" % (case, float(err.max()), K.SUM_TOL,
                                                                        " ".join("%.2e" % float(v) for v in err.ravel())))
    assert np.isfinite(sums).all()
    bad = np.argwhere(~(err <= K.SUM_TOL))
    assert not len(bad), "%d sums off, first at %s: got %r, want %r" % (len(bad), tuple(bad[0]), sums[tuple(bad[0])],
                                                                       float(ref["sums"][tuple(bad[0])]))
    first = run.bits()
    run.again("%s, second call" % (case,))                        # the same inputs give the same bits on every call
    assert torch.equal(run.bits(), first)


@pytest.mark.parametrize("case", list(K.EXACT_CASES), ids=str)
def test_exact_cases_bit_for_bit(case):
    x, y, ix, iy, gamma = K.make_exact_inputs(case, K.EXACT_CASES[case])
    want = K.exact_expected(x, y, ix, iy, gamma)
    got = Run(x, y, ix, iy, gamma).run("exact %s" % (case,))
    bad = np.argwhere(got.view(np.int64) != want.view(np.int64))
    assert not len(bad), "%d of %d sums differ, first at %s: got %r, want %r" % (len(bad), got.size, tuple(bad[0]),
                                                                                got[tuple(bad[0])], want[tuple(bad[0])])


def test_subsets_are_independent():
    """one launch of three subset pairs against three launches of one: the same bits per subset pair"""
    ref = K.reference(K.INDEPENDENCE_CASE)
    together = Run(ref["x"], ref["y"], ref["ix"], ref["iy"], ref["gamma"]).run("together")
    for k in range(K.INDEPENDENCE_CASE[0]):
        alone = Run(ref["x"], ref["y"], ref["ix"][k:k + 1], ref["iy"][k:k + 1], ref["gamma"]).run("subset %d alone" % k)
        assert (alone.view(np.int64) == together[k:k + 1].view(np.int64)).all(), "subset pair %d: %r alone, %r together" % (
            k, alone, together[k])


# ------------------------------------------------------------------------------------------------- 2: the op
def test_op_matches_the_entry_point_and_raises():
    case = K.INDEPENDENCE_CASE
    ref = K.reference(case)
    want = Run(ref["x"], ref["y"], ref["ix"], ref["iy"], ref["gamma"]).run("op")
    x, y = torch.from_numpy(np.array(ref["x"])).to(DEV), torch.from_numpy(np.array(ref["y"])).to(DEV)
    ix, iy = np.array(ref["ix"]), np.array(ref["iy"])
    dix, diy = torch.from_numpy(ix).to(DEV), torch.from_numpy(iy).to(DEV)
    for tables in ((ix, iy), (dix, diy), (ix, diy)):                # host tables, device tables, one of each
        sums = ops.poly_mmd_sums(x, y, *tables)                     # gamma defaults to 1 / D
        assert sums.dtype == torch.float64 and tuple(sums.shape) == (case[0], 3) and sums.is_cuda and not sums.requires_grad
        assert (sums.cpu().numpy().view(np.int64) == want.view(np.int64)).all()
    explicit = ops.poly_mmd_sums(x, y, ix, iy, gamma=ref["gamma"], coef0=1.0)
    assert (explicit.cpu().numpy().view(np.int64) == want.view(np.int64)).all()
    other = ops.poly_mmd_sums(x, y, ix, iy, gamma=0.5 * ref["gamma"], coef0=2.0).cpu().numpy()
    o_ref, o_mag = K.oracle(ref["x"], ref["y"], ref["ix"], ref["iy"], 0.5 * ref["gamma"], 2.0)
    assert K.sum_error(other, o_ref, o_mag) <= K.SUM_TOL
    # a device index out of range is clamped by the kernel: the same bits as the clamped table
    wild = dix.clone()
    wild[0, 0], wild[1, 3], wild[2, 66] = x.shape[0] + 5, -7, 2 ** 31 - 1
    tame = wild.clamp(0, x.shape[0] - 1)
    assert not torch.equal(wild, tame)
    assert torch.equal(ops.poly_mmd_sums(x, y, wild, diy).view(torch.int64), ops.poly_mmd_sums(x, y, tame, diy).view(torch.int64))
    # a host index out of range
    for bad_ix, bad_iy in ((np.where(ix == ix.max(), x.shape[0], ix), iy), (ix, np.where(iy == iy.min(), -1, iy)),
                           (ix, np.where(iy == iy.max(), y.shape[0], iy))):
        with pytest.raises(IndexError):
            ops.poly_mmd_sums(x, y, bad_ix.astype(np.int32), bad_iy.astype(np.int32))
    # nothing is converted for the caller
    wide = torch.cat([x, x], dim=1)
    for bx, by in ((x.double(), y), (x, y.half()),                                  # wrong dtype
                   (x[0], y), (x, y.view(y.shape[0], 8, 10)),                       # wrong rank
                   (wide[:, ::2], y), (x, wide[:, :80]),                            # non-contiguous
                   (x, y.cpu()), (x.cpu(), y),                                      # other device
                   (x, torch.cat([y, y], dim=1))):                                  # D mismatch
        with pytest.raises(ValueError):
            ops.poly_mmd_sums(bx, by, ix, iy)
    for tix, tiy in ((dix.long(), diy), (dix, diy[:, :5]), (dix[0], diy[0]), (dix.cpu(), diy), (dix[:, :1], diy[:, :1])):
        with pytest.raises(ValueError):
            ops.poly_mmd_sums(x, y, tix, tiy)


# ------------------------------------------------------------------------------------------------- 3: end to end
FIELDS = {"kid", "kid_std", "subsets", "subset_size", "n_real", "n_fake", "seed", "gamma", "coef0", "degree", "NET_G", "NET_E",
          "trunk_digest", "note"}


def _check_json(out, ckpt, seed, subsets, s, lowered):
    path = os.path.join(ckpt[:-4], "valid", "kid.json")
    assert os.path.isfile(path) and json.load(open(path)) == out
    assert set(out) == FIELDS
    assert out["n_real"] == out["n_fake"] == 12 and out["seed"] == seed and out["NET_G"] == ckpt and out["NET_E"] == ''
    assert out["subsets"] == subsets and out["subset_size"] == s and out["degree"] == 3 and out["coef0"] == 1.0
    assert out["gamma"] == 1.0 / 2048 and len(out["trunk_digest"]) == 64
    assert "random-init" in out["note"] and "ImageNet" in out["note"] and ("lowered" in out["note"]) == lowered
    assert np.isfinite(out["kid"]) and np.isfinite(out["kid_std"]) and out["kid_std"] >= 0


def test_kid_end_to_end(tmp_path, capsys):
    from mogan_amd.attngan import kid as KID
    cfg, ev, ckpt = _tiny_checkpoint(tmp_path)
    try:
        algo = _trainer(tmp_path)
        out, codes = algo.kid("test", seed=100, subsets=4, subset_size=8, return_codes=True)
        assert "KID (12 real, 12 generated images; 4 subset pairs of 8)" in capsys.readouterr().out
        _check_json(out, ckpt, 100, 4, 8, lowered=False)
        real, fake = codes["real"].numpy(), codes["fake"].numpy()
        assert real.shape == fake.shape == (12, 2048) and real.dtype == np.float32 and not (real == fake).all()
        # the reported figure against numpy fp64 on the returned codes and the subsets redrawn under the same seed
        ix, iy = KID.draw_subsets(12, 12, 4, 8, 100)
        sums = K.numpy_fp64(real, fake, ix, iy, 1.0 / 2048)
        mean, std, _ = KID.kid_from_sums(sums, 8)
        scale = float(K.mmd2_scale(sums, 8).mean())
        print("end to end: kid %.9e +- %.9e, from numpy %.9e +- %.9e, apart by %.3e / %.3e of the scale (KID_E2E_TOL %.2e)"
              % (out["kid"], out["kid_std"], mean, std, abs(out["kid"] - mean) / scale, abs(out["kid_std"] - std) / scale,
                 K.KID_E2E_TOL))
        assert abs(out["kid"] - mean) <= K.KID_E2E_TOL * scale
        assert abs(out["kid_std"] - std) <= K.KID_E2E_TOL * scale
        out2, codes2 = algo.kid("test", seed=100, subsets=4, subset_size=8, return_codes=True)       # same seed, same JSON
        assert out2 == out and torch.equal(codes2["fake"], codes["fake"]) and torch.equal(codes2["real"], codes["real"])
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.FLAG = '', True


def test_main_fid_and_kid_in_one_pass(tmp_path, monkeypatch):
    from mogan_amd.attngan import main as entry
    from mogan_amd.attngan import model
    cfg, ev, ckpt = _tiny_checkpoint(tmp_path)
    images, pool_code = [], model.CNN_ENCODER.pool_code

    def counted(self, x):
        images.append(int(x.shape[0]))
        return pool_code(self, x)
    monkeypatch.setattr(model.CNN_ENCODER, "pool_code", counted)
    try:
        base = ["--cfg", str(ev), "--synthetic", "12", "--manualSeed", "7", "--output_dir", str(tmp_path)]
        entry.main(base + ["--fid", "--kid", "--kid_subsets", "5"])
        assert sum(images) == 24 and len(images) == 6               # 12 real and 12 generated images, once each, in batches of 4
        fid_path, kid_path = [os.path.join(ckpt[:-4], "valid", n) for n in ("fid.json", "kid.json")]
        both = open(fid_path, "rb").read()
        out = json.load(open(kid_path))
        _check_json(out, ckpt, 7, 5, 12, lowered=True)              # the default 1000 lowered to the 12 images there are
        assert "from 1000 to 12" in out["note"]
        os.remove(fid_path)
        del images[:]
        entry.main(base + ["--fid"])
        assert sum(images) == 24
        assert open(fid_path, "rb").read() == both                  # --fid alone writes the same file, byte for byte
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.FLAG = '', True
