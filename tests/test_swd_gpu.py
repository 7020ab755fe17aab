"""-m gpu: the sliced Wasserstein path on the device -- the six entries of csrc/mogan_swd.hip through ctypes in guard-banded, poisoned
memory against the numpy oracle (tests/swd_cases.py: cases, seeds, bounds), the exact cases bit for bit, repeatability; the ops;
attngan/swd.SlicedWasserstein against the oracle's whole score; condGANTrainer.swd end to end (directly, and with --fid through
main.py in one pass).  No bound here comes from the code under test.

fp32 outputs live in memguard.Guarded's float mode (slice poisoned, 1024 sentinels on both sides), the fp64 outputs and the
workspace in its byte mode as in tests/test_prdc_gpu.py: Guarded is asked for the outside of the slice only and the runs look for
doubles that are still 0xFF in every byte.  Every input is held bit for bit."""
import json
import os

import numpy as np
import pytest
import torch

import memguard as MG
import swd_cases as S
from eval_setup import tiny_checkpoint as _tiny_checkpoint, trainer as _trainer
from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import swd as SWD  # noqa: E402
from mogan_amd.hip import lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FULL = (slice(None),)


def _frozen(a):
    """a host array (fp32, or fp64 / int32 as bytes) in guarded device memory, bit for bit"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        t = torch.from_numpy(np.array(a)).to(DEV)
        return MG.Guarded(tuple(t.shape), FULL, DEV, base=t)
    assert a.dtype in (np.float64, np.int32)
    t = torch.from_numpy(np.array(a)).view(torch.uint8).flatten().to(DEV)
    return MG.Guarded(tuple(t.shape), FULL, DEV, dtype=torch.uint8, base=t)


def _held(inputs, what):
    for name, g in inputs.items():
        assert g.untouched(), "%s: %s or its bands were modified" % (what, name)


def _doubles(g, n, what):
    """the n doubles of a byte-mode output: nothing outside changed, every one written"""
    g.check(what=what, written=False)
    never = g.view.view(torch.int64) == -1
    assert not bool(never.any()), "%s: %d outputs never written" % (what, int(never.sum()))
    return g.view.view(torch.float64).cpu().numpy().reshape(n)


def _sync(rc):
    torch.cuda.synchronize()
    assert rc == 0
    return rc


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _bits_equal(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape
    view = np.int64 if got.dtype == np.float64 else np.int32
    bad = np.argwhere(got.view(view) != want.view(view))
    assert not len(bad), "%s: %d of %d values differ, first at %s: got %r, want %r" % (what, len(bad), got.size, tuple(bad[0]),
                                                                                     got[tuple(bad[0])], want[tuple(bad[0])])


# ------------------------------------------------------------------------------------------------- 1: the pyramid kernels
def _down(x, what):
    """mogan_pyr_down on a host array in guarded memory -> (the Guarded output, the frozen input)"""
    NC, H, W = x.shape
    gx, out = _frozen(x), MG.Guarded((NC, H // 2, W // 2), FULL, DEV)
    _sync(lib.load().mogan_pyr_down(gx.ptr, NC, H, W, out.ptr, lib.stream_ptr()))
    _held({"x": gx}, what)
    return out


def _resid(x, down, what):
    NC, H, W = x.shape
    gx, gd, out = _frozen(x), _frozen(down), MG.Guarded((NC, H, W), FULL, DEV)
    _sync(lib.load().mogan_lap_residual(gx.ptr, gd.ptr, NC, H, W, out.ptr, lib.stream_ptr()))
    _held({"x": gx, "down": gd}, what)
    return out


@pytest.mark.parametrize("shape", S.PYRAMID_SHAPES, ids=str)
def test_pyramid_exact_cases_bit_for_bit(shape):
    x = S.integer_image(shape, S.seed_of("exact", shape))
    down = S.pyr_down(x, np.float32)
    _down(x, "pyr_down %s" % (shape,)).check(_t(down), exact=True, what="pyr_down %s" % (shape,))
    want = S.lap_residual(x, down, np.float32)
    _resid(x, down, "lap_residual %s" % (shape,)).check(_t(want), exact=True, what="lap_residual %s" % (shape,))
    again = _down(x, "second call")
    again.check(_t(down), exact=True, what="pyr_down, second call")


def test_pyramid_two_deep_chain_of_0_1_images_bit_for_bit():
    x = S.integer_image((6, 16, 16), 9, high=2)
    d1 = S.pyr_down(x, np.float32)
    d2 = S.pyr_down(d1, np.float32)
    got1 = _down(x, "chain 1")
    got1.check(_t(d1), exact=True, what="chain, first step")
    got2 = _down(got1.view.cpu().numpy(), "chain 2")               # the device's own first level feeds the second
    got2.check(_t(d2), exact=True, what="chain, second step")
    _resid(got1.view.cpu().numpy(), got2.view.cpu().numpy(), "chain residual").check(
        _t(S.lap_residual(d1, d2, np.float32)), exact=True, what="chain, residual of the second level")


@pytest.mark.parametrize("shape", S.PYRAMID_SHAPES, ids=str)
def test_pyramid_gaussian_images_within_the_closed_form_bound(shape):
    x = S.gaussian_image(shape, S.seed_of("gauss", shape))
    want, bound = S.pyr_down(x), S.down_bound(x)
    out = _down(x, "pyr_down %s" % (shape,))
    err = (out.view.cpu().double().numpy() - want)
    print("pyr_down %s: worst %.3e of its bound" % (shape, float(np.max(np.abs(err) / bound))))
    out.check(_t(want), atol=_t(bound), what="pyr_down %s" % (shape,))
    down = want.astype(np.float32)                                  # the residual from a given fp32 down
    want, bound = S.lap_residual(x, down), S.residual_bound(x, down)
    out = _resid(x, down, "lap_residual %s" % (shape,))
    err = (out.view.cpu().double().numpy() - want)
    print("lap_residual %s: worst %.3e of its bound" % (shape, float(np.max(np.abs(err) / bound))))
    out.check(_t(want), atol=_t(bound), what="lap_residual %s" % (shape,))


# ------------------------------------------------------------------------------------------------- 2: gather
@pytest.mark.parametrize("case", S.GATHER_CASES, ids=str)
def test_gather_is_a_copy_into_its_rows_only(case):
    C, size, R = case
    N, row0, total = 3, 5, 5 + R + 7
    level = S.gaussian_image((N, C, size, size), S.seed_of("gather", case))
    centres = S.gather_centres(N, size, R, S.seed_of("centres", case))
    if size > 7 and R >= 4:
        pairs = {tuple(c) for c in centres[:, 1:].tolist()}
        assert {(3, 3), (size - 4, size - 4), (3, size - 4), (size - 4, 3)} <= pairs
    gl, gc = _frozen(level), _frozen(centres)
    desc = MG.Guarded((total, 49 * C), (slice(row0, row0 + R),), DEV)          # the rows before and after stay poisoned
    rc = lib.load().mogan_swd_gather(gl.ptr, N, C, size, size, gc.ptr, R, desc.parent.data_ptr(), row0, total, lib.stream_ptr())
    _sync(rc)
    _held({"level": gl, "centres": gc}, "gather %s" % (case,))
    desc.check(_t(S.descriptors(level, centres)), exact=True, what="gather %s" % (case,))


def test_gather_op_checks_uploads_and_matches_the_entry():
    C, size, R = 3, 16, 130
    level = S.gaussian_image((3, C, size, size), 4)
    centres = S.gather_centres(3, size, R, 5)
    lv = _t(level).to(DEV)
    buf = torch.full((R + 9, 147), 7.0, device=DEV)
    assert ops.swd_gather(lv, centres.astype(np.int64), buf, 4) is buf
    want = S.descriptors(level, centres)
    assert torch.equal(buf[4:4 + R].cpu(), _t(want)) and bool((buf[:4] == 7).all()) and bool((buf[4 + R:] == 7).all())
    buf2 = torch.zeros((R, 147), device=DEV)
    ops.swd_gather(lv, _t(centres).to(DEV), buf2, 0)                # an int32 device table is taken as it is
    assert torch.equal(buf2.cpu(), _t(want))
    with pytest.raises(ValueError, match="centres outside"):
        ops.swd_gather(lv, np.array([[0, 3, 13]]), buf, 0)
    with pytest.raises(ValueError):
        ops.swd_gather(lv, _t(centres), buf, 0)                     # a host tensor is not uploaded for the caller
    with pytest.raises(ValueError):
        ops.swd_gather(lv, centres, buf.cpu(), 0)


# ------------------------------------------------------------------------------------------------- 3: moments
class Moments:
    def __init__(self, desc, C):
        self.rows, self.C = desc.shape[0], C
        self.inputs = {"desc": _frozen(desc)}
        self.ws_bytes = int(lib.load().mogan_swd_moments_ws_bytes(self.rows, C))
        assert self.ws_bytes == 8 * C * min(-(-self.rows // 64), 2048)
        self.out = MG.Guarded((16 * C,), FULL, DEV, dtype=torch.uint8)
        self.ws = MG.Guarded((self.ws_bytes,), FULL, DEV, dtype=torch.uint8)

    def run(self, what):
        _sync(lib.load().mogan_swd_moments_f64(self.inputs["desc"].ptr, self.rows, self.C, self.out.ptr, self.ws.ptr, self.ws_bytes,
                                               lib.stream_ptr()))
        self.ws.check(what=what + " ws", written=False)
        _held(self.inputs, what)
        return _doubles(self.out, 2 * self.C, what).reshape(self.C, 2)

    def again(self, what):
        self.out.reset()
        self.ws.reset()
        return self.run(what)


@pytest.mark.parametrize("case", S.MOMENT_CASES, ids=str)
def test_moments_against_longdouble_in_guarded_memory(case):
    rows, C = case
    desc = S.moment_inputs(rows, C, S.seed_of("moments", case))
    ref, bound = S.moments(desc, C), S.moments_bounds(desc, C)
    run = Moments(desc, C)
    got = run.run("moments %s" % (case,))
    err = np.abs(got.astype(S.LD) - ref).astype(np.float64)
    print("moments %s: mean off by %.3e (bound %.3e), std by %.3e (bound %.3e)" % (case, err[:, 0].max(), bound[:, 0].max(),
                                                                                  err[:, 1].max(), bound[:, 1].max()))
    assert (err <= bound).all(), "moments %s: errors %s exceed %s" % (case, err.tolist(), bound.tolist())
    _bits_equal(run.again("second call"), got, "moments, second call")
    assert torch.equal(ops.swd_moments(_t(desc).to(DEV)).cpu(), _t(got))


def test_a_constant_channel_has_a_standard_deviation_of_exactly_0():
    desc = S.moment_inputs(257, 3, 8).reshape(257, 3, 49)
    desc[:, 1] = 2.5
    got = Moments(desc.reshape(257, 147), 3).run("constant channel")
    assert got[1, 0] == 2.5 and got[1, 1] == 0.0 and got[0, 1] > 0 and got[2, 1] > 0
    sw = SWD.SlicedWasserstein(32, 3, 16, patches=8, dirs=4, repeats=1, min_res=16, seed=1, device=DEV)
    real, _ = S.score_images(3, 3)
    flat = np.array(real[:2])
    flat[:, 2] = 17.0                                               # a constant channel: its Laplacian level is exactly 0
    sw.add(_t(real[:2]).to(DEV), _t(flat).to(DEV))
    with pytest.raises(ValueError, match="level 32, channel 2 of the generated images"):
        sw.result()


# ------------------------------------------------------------------------------------------------- 4: project
def _project(desc, mom, dirs, what):
    rows, C, D = desc.shape[0], mom.shape[0], dirs.shape[1]
    inputs = {"desc": _frozen(desc), "moments": _frozen(mom), "dirs": _frozen(dirs)}
    out = MG.Guarded((D, rows), FULL, DEV)
    _sync(lib.load().mogan_swd_project(inputs["desc"].ptr, rows, C, inputs["moments"].ptr, inputs["dirs"].ptr, D, out.ptr,
                                       lib.stream_ptr()))
    _held(inputs, what)
    return out


@pytest.mark.parametrize("case", S.PROJECT_CASES, ids=str)
def test_projections_within_four_times_numpys_own_deviation(case):
    desc, mom, dirs = S.project_inputs(case)
    want, dev = S.projections(desc, mom, dirs), S.numpy_fp32_deviation(desc, mom, dirs)
    out = _project(desc, mom, dirs, "project %s" % (case,))
    got = out.view.cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("project %s: numpy fp32 deviates by %.3e, the kernel by %.3e (bound %.3e)" % (case, dev, err, 4 * dev))
    out.check(_t(want), atol=S.projection_bound(desc, mom, dirs), what="project %s" % (case,))
    _bits_equal(_project(desc, mom, dirs, "second call").view.cpu().numpy(), got, "project, second call")
    assert torch.equal(ops.swd_project(_t(desc).to(DEV), _t(mom).to(DEV), _t(dirs).to(DEV)).cpu(), _t(got))


def test_a_rows_projections_do_not_depend_on_its_position_or_its_batch():
    desc, mom, dirs = S.project_inputs((130, 3, 130))
    base = _project(desc, mom, dirs, "in place").view.cpu().numpy()
    pick = np.concatenate([np.arange(100, 130), np.arange(0, 37)])              # 67 rows: other tiles, other lanes, another tail
    moved = _project(desc[pick], mom, dirs, "moved").view.cpu().numpy()
    _bits_equal(moved, base[:, pick], "moved rows")
    few = _project(desc[pick], mom, dirs[:, 64:69].copy(), "fewer directions").view.cpu().numpy()
    _bits_equal(few, base[64:69][:, pick], "a direction in another slot of another pass")


# ------------------------------------------------------------------------------------------------- 5: absdiff
def _absdiff(a, b, what):
    D, rows = a.shape
    inputs = {"a": _frozen(a), "b": _frozen(b)}
    out = MG.Guarded((8 * D,), FULL, DEV, dtype=torch.uint8)
    _sync(lib.load().mogan_swd_absdiff_f64(inputs["a"].ptr, inputs["b"].ptr, rows, D, out.ptr, lib.stream_ptr()))
    _held(inputs, what)
    return _doubles(out, D, what)


@pytest.mark.parametrize("case", S.ABSDIFF_CASES, ids=str)
def test_absdiff_exact_on_dyadic_inputs_and_within_the_fp64_bound(case):
    rows, D = case
    a, b = S.absdiff_inputs(rows, D, S.seed_of("dyadic", case), dyadic=True)
    _bits_equal(_absdiff(a, b, "dyadic %s" % (case,)), S.absdiff(a, b).astype(np.float64), "dyadic %s" % (case,))
    a, b = S.absdiff_inputs(rows, D, S.seed_of("general", case), dyadic=False)
    got = _absdiff(a, b, "general %s" % (case,))
    err = np.abs(got.astype(S.LD) - S.absdiff(a, b)).astype(np.float64)
    print("absdiff %s: worst %.3e of its bound" % (case, float((err / np.maximum(S.absdiff_bound(a, b), 1e-300)).max())))
    assert (err <= S.absdiff_bound(a, b)).all()
    _bits_equal(_absdiff(a, b, "second call"), got, "absdiff, second call")
    assert torch.equal(ops.swd_absdiff(_t(a).to(DEV), _t(b).to(DEV)).cpu(), _t(got))


# ------------------------------------------------------------------------------------------------- 6: the whole score
def _contract_draws(C):
    """the centres and directions of ONE batch of all images, drawn here from the three streams as attngan/swd.py documents"""
    n, P, seed = S.SCORE["images"], S.SCORE["patches"], S.SCORE["seed"]
    sizes = [32, 16]
    image = (np.arange(n * P) // P).astype(np.int32)
    centres = {}
    for side, s in (("real", seed), ("fake", seed + 1)):
        rng = np.random.RandomState(s)
        centres[side] = []
        for size in sizes:
            cx = rng.randint(3, size - 3, n * P)
            cy = rng.randint(3, size - 3, n * P)
            centres[side].append(np.stack([image, cy, cx], axis=1).astype(np.int32))
    rng = np.random.RandomState(seed + 2)
    directions = []
    for _ in sizes:
        per = []
        for _ in range(S.SCORE["repeats"]):
            d = rng.randn(C * 49, S.SCORE["dirs"])
            per.append(np.ascontiguousarray((d / np.sqrt((d * d).sum(axis=0, keepdims=True))).astype(np.float32)))
        directions.append(per)
    return sizes, centres, directions


def _score(C, rows=None):
    k = S.SCORE
    return SWD.SlicedWasserstein(k["size"], C, rows or k["images"] * k["patches"], k["patches"], k["dirs"], k["repeats"], k["min_res"],
                                 k["seed"], DEV)


@pytest.mark.parametrize("C", S.SCORE_CASES, ids=["C = 1", "C = 3"])
def test_the_whole_score_against_the_oracle(C):
    real, fake = S.score_images(C, S.seed_of("score", C))
    sizes, centres, directions = _contract_draws(C)
    want, bounds = S.score_oracle(real, fake, centres, directions, sizes)
    r, f = _t(real).to(DEV), _t(fake).to(DEV)
    sw = _score(C)
    sw.add(r, f)
    got = sw.result()
    assert got["levels"] == sizes and got["rows"] == 128 and len(got["per_level"]) == 2
    for size, g, w, b in zip(sizes, got["per_level"], want, bounds):
        print("C = %d, level %d: %.6f against %.6f, off by %.3e (bound %.3e)" % (C, size, g, w, abs(g - w), b))
    assert all(abs(g - w) <= b for g, w, b in zip(got["per_level"], want, bounds))
    assert got["swd"] == (got["per_level"][0] + got["per_level"][1]) / 2 and all(w > 10 * b for w, b in zip(want, bounds))
    # two runs give the same bits
    again = _score(C)
    again.add(r, f)
    assert again.result() == got
    # two batches of 8 under the one batch's centres give the same bits as one of 16; the buffers may be larger than what is added
    half = S.SCORE["images"] // 2 * S.SCORE["patches"]
    split = _score(C, rows=3 * half)
    for lo in (0, 1):
        part = {side: [np.ascontiguousarray(t[lo * half:(lo + 1) * half] - np.array([8 * lo, 0, 0], dtype=np.int32)) for t in centres[side]]
                for side in centres}
        split.add(r[8 * lo:8 * lo + 8].contiguous(), f[8 * lo:8 * lo + 8].contiguous(), centres=part)
    assert split.result() == got
    # a bit copy under the same centres is at exactly 0.0
    same = _score(C)
    same.add(r, r.clone(), centres={"real": centres["real"], "fake": centres["real"]})
    zero = same.result()
    assert zero["swd"] == 0.0 and zero["per_level"] == [0.0, 0.0]


# ------------------------------------------------------------------------------------------------- 7: end to end
FIELDS = {"swd", "levels", "per_level", "patches", "dirs", "repeats", "n_real", "n_fake", "seed", "NET_G", "NET_E", "note"}


def _check_json(out, ckpt, seed, n, patches, dirs, repeats, levels):
    path = os.path.join(ckpt[:-4], "valid", "swd.json")
    assert os.path.isfile(path) and json.load(open(path)) == out
    assert set(out) == FIELDS
    assert out["n_real"] == out["n_fake"] == n and out["seed"] == seed and out["NET_G"] == ckpt and out["NET_E"] == ''
    assert (out["patches"], out["dirs"], out["repeats"], out["levels"]) == (patches, dirs, repeats, levels)
    assert len(out["per_level"]) == len(levels) and all(np.isfinite(v) and v > 0 for v in out["per_level"])
    assert out["swd"] == sum(out["per_level"]) / len(levels) or abs(out["swd"] - np.mean(out["per_level"])) < 1e-12 * out["swd"]
    assert "trunk-free" in out["note"] and "patches" in out["note"] and "8 bits" in out["note"]


def test_swd_end_to_end_without_an_image_encoder(tmp_path, capsys, monkeypatch):
    from mogan_amd.attngan.evaluate import CheckpointEvaluation
    cfg, ev, ckpt = _tiny_checkpoint(tmp_path)

    def no_trunk(self):
        raise AssertionError("swd() alone must not load the image encoder")
    monkeypatch.setattr(CheckpointEvaluation, "_load_image_encoder", no_trunk)
    try:
        algo = _trainer(tmp_path)
        out = algo.swd("test", seed=100, patches=16, dirs=16, repeats=2)
        text = capsys.readouterr().out
        assert "SWD (12 real, 12 generated images; 16 patches, 16 directions, 2 repeats):" in text and "GB of descriptors" in text
        _check_json(out, ckpt, 100, 12, 16, 16, 2, [256, 128, 64, 32, 16])
        assert algo.swd("test", seed=100, patches=16, dirs=16, repeats=2) == out               # same seed, same JSON
        coarse = algo.swd("test", seed=100, patches=16, dirs=16, repeats=2, min_res=64)
        _check_json(coarse, ckpt, 100, 12, 16, 16, 2, [256, 128, 64])
        few = algo.swd("test", num_samples=8, seed=100, patches=16, dirs=16, repeats=2)
        _check_json(few, ckpt, 100, 8, 16, 16, 2, [256, 128, 64, 32, 16])
        with pytest.raises(ValueError, match="power of two"):
            algo.swd("test", min_res=48)
        acc = algo.swd_images(seed=100, patches=16, dirs=16, repeats=2)
        with pytest.raises(ValueError, match="other parameters"):
            algo.swd("test", seed=101, patches=16, dirs=16, repeats=2, images=acc)
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.FLAG = '', True


def test_main_swd_and_fid_in_one_pass(tmp_path, monkeypatch):
    from mogan_amd.attngan import main as entry
    from mogan_amd.attngan import model
    cfg, ev, ckpt = _tiny_checkpoint(tmp_path)
    images, pool_code = [], model.CNN_ENCODER.pool_code

    def counted(self, x):
        images.append(int(x.shape[0]))
        return pool_code(self, x)
    monkeypatch.setattr(model.CNN_ENCODER, "pool_code", counted)
    try:
        base = ["--cfg", str(ev), "--synthetic", "12", "--manualSeed", "7", "--output_dir", str(tmp_path), "--swd_patches", "16",
                "--swd_dirs", "16", "--swd_repeats", "2"]
        paths = [os.path.join(ckpt[:-4], "valid", n) for n in ("swd.json", "fid.json")]
        entry.main(base + ["--swd", "--fid"])
        assert sum(images) == 24 and len(images) == 6               # 12 real and 12 generated images through the trunk, once each
        both = [open(p, "rb").read() for p in paths]
        _check_json(json.load(open(paths[0])), ckpt, 7, 12, 16, 16, 2, [256, 128, 64, 32, 16])
        for p in paths:
            os.remove(p)
        del images[:]
        entry.main(base + ["--swd"])                                # alone: a pass of its own, no trunk
        assert not images and not os.path.exists(paths[1])
        assert open(paths[0], "rb").read() == both[0]               # the same figures, bit for bit
        os.remove(paths[0])
        entry.main(base + ["--fid"])
        assert sum(images) == 24 and not os.path.exists(paths[0])
        assert open(paths[1], "rb").read() == both[1]               # fid.json keeps its bytes
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.FLAG = '', True
