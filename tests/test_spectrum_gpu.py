"""-m gpu: the radial power spectrum on the device -- the entry of csrc/mogan_spectrum.hip through ctypes with every buffer in
guard-banded, poisoned memory against the numpy fp64 oracle (tests/spectrum_cases.py: cases, seeds, bounds), the analytic images, the
rejections, the three bit-level contracts; the op; attngan/spectrum.RadialSpectrum against the oracle's figures; condGANTrainer.spectrum
end to end (directly, through main.py, and with --swd --msssim in one pass); and the one behavioural check: a period-4 grid on the
generated side is reported at period 4.  No bound here comes from the code under test.

The fp32 inputs live in memguard.Guarded's float mode, everything else (fp64 twiddle factors and sums, the int32 table, the workspace)
in its byte mode as in tests/test_msssim_gpu.py.  Every input is held bit for bit."""
import json
import os

import numpy as np
import pytest
import torch

import memguard as MG
import spectrum_cases as S
from eval_setup import tiny_checkpoint as _tiny_checkpoint
from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import spectrum as SP  # noqa: E402
from mogan_amd.hip import lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FULL = (slice(None),)


def _frozen(a):
    """an input in guarded memory: fp32 as it is, anything else as its bytes"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        t = torch.from_numpy(a.copy()).to(DEV)
        return MG.Guarded(tuple(t.shape), FULL, DEV, base=t)
    t = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(DEV)
    return MG.Guarded(tuple(t.shape), FULL, DEV, dtype=torch.uint8, base=t)


def _t(a):
    return torch.from_numpy(np.array(a))


def _bits_equal(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype == np.float64 and got.shape == want.shape
    bad = np.argwhere(got.view(np.int64) != want.view(np.int64))
    assert not len(bad), "%s: %d of %d values differ, first at %s: got %r, want %r" % (what, len(bad), got.size, tuple(bad[0]),
                                                                                     got[tuple(bad[0])], want[tuple(bad[0])])


def closed_form(B, size):
    V = size // 2 + 1
    cols = min(V, 2048 // size)
    return min(B, 64) * (V * size * 16 + -(-V // cols) * 2048)


class Power:
    """one call of mogan_radial_power_f64 with every buffer guarded: run() -> (B, n_bins) fp64 on the host"""

    def __init__(self, x, weight, win, table=None, n_bins=None):
        self.B, self.C, self.S, _ = x.shape
        if table is None:
            table, count = SP.radial_bins(self.S)
            n_bins = len(count)
        self.n_bins = int(n_bins)
        self.inputs = {"x": _frozen(x), "weight": _frozen(weight), "twiddle": _frozen(ops.twiddle_table(self.S)),
                       "bins": _frozen(np.asarray(table, dtype=np.int32))}
        if win is not None:
            self.inputs["window"] = _frozen(win)
        self.ws_bytes = int(lib.load().mogan_radial_power_ws_bytes(self.B, self.S))
        assert self.ws_bytes == closed_form(self.B, self.S)
        self.out = MG.Guarded((8 * self.B * self.n_bins,), FULL, DEV, dtype=torch.uint8)
        self.ws = MG.Guarded((self.ws_bytes,), FULL, DEV, dtype=torch.uint8)

    def call(self, **kw):
        i = self.inputs
        a = dict(x=i["x"].ptr, B=self.B, C=self.C, S=self.S, weight=i["weight"].ptr, window=i["window"].ptr if "window" in i else None,
                 twiddle=i["twiddle"].ptr, bins=i["bins"].ptr, n_bins=self.n_bins, out=self.out.ptr, ws=self.ws.ptr,
                 ws_bytes=self.ws_bytes)
        a.update(kw)
        rc = lib.load().mogan_radial_power_f64(a["x"], a["B"], a["C"], a["S"], a["weight"], a["window"], a["twiddle"], a["bins"],
                                               a["n_bins"], a["out"], a["ws"], a["ws_bytes"], lib.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def run(self, what):
        assert self.call() == 0
        for name, g in self.inputs.items():
            assert g.untouched(), "%s: %s or its bands were modified" % (what, name)
        self.ws.check(what=what + " ws", written=False)              # nothing outside ws_bytes
        self.out.check(what=what + " out", written=False)
        never = self.out.view.view(torch.int64) == -1
        assert not bool(never.any()), "%s: %d sums never written" % (what, int(never.sum()))
        return self.out.view.view(torch.float64).cpu().numpy().reshape(self.B, self.n_bins)

    def again(self, what):
        for g in (self.out, self.ws):
            g.reset()
        return self.run(what)


# ------------------------------------------------------------------------------------------------- 1: the entry point
@pytest.mark.parametrize("key", S.CASES, ids=str)
def test_every_case_within_its_bound_in_guarded_memory(key):
    x, weight, win = S.case(key)
    want, bound = S.expected(key)
    run = Power(x, weight, win)
    got = run.run("case %s" % (key,))
    unit = S.unit(x, weight, win)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        print("case %s: off by %.3f units of eps log2(S^2) total at the most (bound %.0f units)"
              % (key, np.nanmax(np.abs(got - want) / unit), S.MULTIPLE))
    bad = np.argwhere(~(np.abs(got - want) <= bound))
    assert not len(bad), "%s: %d bins off, first (image, bin) %s: got %r, want %r, bound %r" % (
        key, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])], bound[tuple(bad[0])])
    _bits_equal(run.again("second call"), got, "a second call")                              # contract (a)
    # the op is the entry
    table, count = SP.radial_bins(key[0])
    dev = [_t(x).to(DEV), _t(weight).to(DEV), None if win is None else _t(win).to(DEV), _t(table).to(DEV)]
    keep = dev[0].clone()
    op = ops.radial_power(*dev, len(count))
    assert op.dtype == torch.float64 and tuple(op.shape) == got.shape and torch.equal(dev[0], keep)
    _bits_equal(op.cpu().numpy(), got, "the op against the entry")
    buf = torch.full((key[1] + 2, len(count)), -7.0, dtype=torch.float64, device=DEV)
    assert ops.radial_power(*dev, len(count), out=buf[1:-1]).data_ptr() == buf[1:-1].data_ptr()
    _bits_equal(buf[1:-1].cpu().numpy(), got, "the op into rows of a larger buffer")
    assert bool((buf[0] == -7.0).all()) and bool((buf[-1] == -7.0).all())


@pytest.mark.parametrize("size", (8, 32))
@pytest.mark.parametrize("C", (1, 3))
def test_the_analytic_images(size, C):
    x, rows = S.analytic(size, C)
    got = Power(x, S.weights(C), None).run("analytic S = %d, C = %d" % (size, C))
    worst = S.analytic_check(got, size, C)
    print("S = %d, C = %d: %d analytic images, %.3f of the tolerance used at the most" % (size, C, len(rows), worst))
    p = got[0] / S.count_of(size)                                   # the impulse: every bin's p is equal
    assert np.abs(p - p[0]).max() <= S.MULTIPLE * S.unit(x[:1], S.weights(C), None)[0]


@pytest.mark.parametrize("size", (8, 32))
def test_a_table_with_a_region_left_out_and_entries_past_n_bins(size):
    table, n_bins = S.custom_table(size)
    x, weight, win = S.case((size, 5, 3, "hann"))
    want = S.sums(x, weight, win, table, n_bins)
    bound = S.bound(want, S.sums_direct(x, weight, win, table, n_bins), x, weight, win)
    got = Power(x, weight, win, table, n_bins).run("custom table")
    assert got.shape == (5, n_bins) and (np.abs(got - want) <= bound).all()
    # a -1 region contributes nothing: one bin for the whole plane against one bin for half of it, on an image whose power lies
    # in the half that is left out
    keep = np.zeros((size, size // 2 + 1), dtype=np.int32)
    none = np.full_like(keep, -1)
    low = keep.copy()
    low[:, size // 4 + 1:] = -1
    high = S.images([S.cosine(size, 0, size // 2)], 1)              # all of it at (0, S / 2), exactly
    every = Power(high, S.weights(1), None, keep, 1).run("one bin")
    assert abs(every[0, 0] - float(size) ** 4) <= S.MULTIPLE * S.unit(high, S.weights(1), None)[0]
    assert Power(high, S.weights(1), None, none, 1).run("no bin")[0, 0] == 0.0
    assert Power(high, S.weights(1), None, low, 1).run("low half")[0, 0] <= S.MULTIPLE * S.unit(high, S.weights(1), None)[0]


def test_rejected_arguments_return_non_zero_and_write_nothing():
    x, weight, win = S.case((16, 3, 3, "hann"))
    run = Power(x, weight, win)
    for kw in (dict(S=12), dict(S=4), dict(S=512), dict(C=0), dict(C=5), dict(n_bins=0), dict(n_bins=257), dict(B=0),
               dict(x=None), dict(weight=None), dict(twiddle=None), dict(bins=None), dict(out=None)):
        assert run.call(**kw) == -1, kw
        assert run.out.untouched() and run.ws.untouched(), kw
    for kw in (dict(ws_bytes=run.ws_bytes - 1), dict(ws_bytes=0), dict(ws=None), dict(ws=run.ws.ptr + 8, ws_bytes=run.ws_bytes)):
        assert run.call(**kw) == -3, kw
        assert run.out.untouched() and run.ws.untouched(), kw
    run.run("after the rejections")                                 # and the same buffers serve a legal call


# ------------------------------------------------------------------------------------------------- 2: the bit contracts
@pytest.mark.parametrize("key", [(8, 5, 3, "hann"), (32, 5, 1, "none"), (32, 5, 3, "hann")], ids=str)
def test_an_images_row_has_the_bits_it_has_alone(key):
    x, weight, win = S.case(key)
    whole = Power(x, weight, win).run("B = 5")
    for b in (0, 2, 4):
        _bits_equal(Power(x[b:b + 1], weight, win).run("B = 1")[0], whole[b], "image %d alone against its row in B = 5" % b)
    back = Power(x[::-1], weight, win).run("reversed")             # ... and at any position
    _bits_equal(back[::-1], whole, "the batch in reverse order")


def test_the_bits_do_not_depend_on_the_batch_past_one_round_of_launches():
    x, weight, win = S.case((8, 5, 3, "hann"))
    many = np.ascontiguousarray(np.concatenate([x] * 27)[:131])     # three rounds of at most 64 images
    got = Power(many, weight, win).run("B = 131")
    want = Power(x, weight, win).run("B = 5")
    for b in range(131):
        _bits_equal(got[b], want[b % 5], "image %d of 131" % b)


def test_a_zero_image_gives_exactly_zero():
    for size, B, C, name in ((8, 5, 1, "none"), (32, 5, 3, "hann"), (256, 2, 3, "hann")):
        x = np.zeros((3, C, size, size), dtype=np.float32)
        x[1] = S.case((size, B, C, name))[0][0]                     # a case's normal image between two zero images
        got = Power(x, S.weights(C), S.window(name, size)).run("zeros")
        assert (got[0] == 0.0).all() and (got[2] == 0.0).all() and not np.signbit(got[[0, 2]]).any() and (got[1] > 0).any()


def test_the_op_refuses_tensors_on_two_devices():
    table, count = SP.radial_bins(16)
    x, w, win, bins = (torch.zeros(2, 3, 16, 16, device=DEV), _t(SP.channel_weights(3)).to(DEV), _t(SP.hann(16)).to(DEV),
                       _t(table).to(DEV))
    for args in ((x.cpu(), w, win, bins), (x, w.cpu(), win, bins), (x, w, win.cpu(), bins), (x, w, win, bins.cpu()),
                 (x.double(), w, win, bins), (x[:, :, :, ::2], w, win, bins)):
        with pytest.raises(ValueError):
            ops.radial_power(*args, len(count))
    with pytest.raises(ValueError):
        ops.radial_power(x, w, win, bins, len(count), out=torch.zeros(2, len(count), dtype=torch.float64))
    assert bool((ops.radial_power(x, w, win, bins, len(count)) == 0).all())


# ------------------------------------------------------------------------------------------------- 3: the accumulator
def _sides(size, C, n, seed):
    """two sides of n noise images of one variance: the fake side carries lines of period 4 along one axis, 10 dB above the noise
    of their ring"""
    rng = np.random.RandomState(seed)
    real = rng.standard_normal((n, C, size, size)) * 0.3
    fake = rng.standard_normal((n, C, size, size)) * 0.3
    i = np.arange(size)
    fake = fake + 0.2 * np.cos(2 * np.pi * i / 4)[None, None, :, None]
    return np.clip(real, -1, 1).astype(np.float32), np.clip(fake, -1, 1).astype(np.float32)


@pytest.mark.parametrize("size,C,name", [(32, 3, "hann"), (64, 1, "none")])
def test_the_accumulator_against_the_oracles_figures_in_batches_of_3_and_of_5(size, C, name):
    n = 15
    real, fake = _sides(size, C, n, S.seed_of("sides", (size, C, name)))
    weight, win, count = S.weights(C), S.window(name, size), S.count_of(size)
    P = [S.profile(x, weight, win).mean(axis=0) for x in (real, fake)]
    want = S.figures(P[0], P[1], count, size)
    # what the kernel's bound on the sums allows the figures: a sum moves by at most `rel` of itself, a dB value by 10 / ln 10
    # times that, d by twice as much; lsd (an rms of d) and hf (a ratio of sums) by no more than d; a slope by sum |c_k| times a dB
    # value's, c the least-squares coefficients
    rel = max(float((S.MULTIPLE * S.unit(x, weight, win)[:, None] / S.sums(x, weight, win)).max()) for x in (real, fake))
    tol_db = 2 * 10 / np.log(10) * rel
    xs = np.log10(np.arange(1, size // 2 + 1))
    tol_slope = float(np.abs((xs - xs.mean()) / ((xs - xs.mean()) ** 2).sum()).sum()) * tol_db
    results = []
    for step in (3, 5):
        acc = SP.RadialSpectrum(size, C, n + 2, window=name, seed=3, device=DEV)       # a buffer larger than what is added
        tr, tf = _t(real).to(DEV), _t(fake).to(DEV)
        keep = (tr.clone(), tf.clone())
        for at in range(0, n, step):
            acc.add(tr[at:at + step].contiguous(), tf[at:at + step].contiguous())
        assert acc.n == n and torch.equal(tr, keep[0]) and torch.equal(tf, keep[1])
        for side, x in (("real", real), ("fake", fake)):
            got = acc.sums[side][:n].cpu().numpy()
            ref = S.sums(x, weight, win)
            assert (np.abs(got - ref) <= S.MULTIPLE * S.unit(x, weight, win)[:, None]).all(), side
        results.append(acc.result())
    a, b = results
    assert json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)                  # the same bits in batches of 3 and of 5
    print("S = %d, C = %d, %s: lsd %.6f (oracle %.6f), hf %.6f (%.6f), slopes %.4f / %.4f (%.4f / %.4f), peak %s; tolerance %.2e dB"
          % (size, C, name, a["lsd_db"], want["lsd_db"], a["hf_db"], want["hf_db"], a["slope_real"], a["slope_fake"],
             want["slope_real"], want["slope_fake"], a["peak"], tol_db))
    assert a["n"] == n and a["empty_bins"] == want["empty_bins"] == [] and a["count"] == count.tolist()
    assert abs(a["lsd_db"] - want["lsd_db"]) <= tol_db and abs(a["hf_db"] - want["hf_db"]) <= tol_db
    assert abs(a["slope_real"] - want["slope_real"]) <= tol_slope and abs(a["slope_fake"] - want["slope_fake"]) <= tol_slope
    assert a["peak"]["bin"] == want["peak"]["bin"] == size // 4 and a["peak"]["period"] == 4.0
    assert abs(a["peak"]["excess_db"] - want["peak"]["excess_db"]) <= tol_db
    with np.errstate(divide="ignore"):
        assert np.abs(np.array(a["profile_real_db"]) - 10 * np.log10(P[0])).max() <= tol_db
        assert np.abs(np.array(a["excess_db"]) - (10 * np.log10(P[1]) - 10 * np.log10(P[0]))).max() <= tol_db


# ------------------------------------------------------------------------------------------------- 4: end to end
KEYS = {"lsd_db", "hf_db", "slope_real", "slope_fake", "peak", "profile_real_db", "profile_fake_db", "excess_db", "count", "empty_bins",
        "size", "window", "n_real", "n_fake", "seed", "NET_G", "NET_E", "note"}


def _main_trainer(tmp_path, seed=7, length=12):
    """the trainer main.py builds for --synthetic 12 --manualSeed 7 under the tiny config"""
    from mogan_amd.attngan.datasets import SyntheticTextDataset
    from mogan_amd.attngan.miscc.config import cfg
    from mogan_amd.attngan.trainer import condGANTrainer
    ds = SyntheticTextDataset(length, seed=seed, eval=False)
    dl = torch.utils.data.DataLoader(ds, batch_size=cfg.TRAIN.BATCH_SIZE, drop_last=True, shuffle=True, num_workers=0)
    return condGANTrainer(str(tmp_path), dl, ds.n_words, ds.ixtoword, '', distributed=False)


def test_spectrum_end_to_end_three_ways_with_the_same_bytes(tmp_path, capsys, monkeypatch):
    from mogan_amd.attngan import main as entry
    from mogan_amd.attngan.evaluate import CheckpointEvaluation
    cfg, ev, ckpt = _tiny_checkpoint(tmp_path)
    try:
        base = ["--cfg", str(ev), "--synthetic", "12", "--manualSeed", "7", "--output_dir", str(tmp_path), "--swd_patches", "16",
                "--swd_dirs", "16", "--swd_repeats", "2", "--msssim_scales", "3"]
        paths = {n: os.path.join(ckpt[:-4], "valid", n + ".json") for n in ("spectrum", "swd", "msssim")}
        entry.main(base + ["--swd", "--msssim"])                    # the other two scores without this one
        without = {n: open(paths[n], "rb").read() for n in ("swd", "msssim")}
        assert not os.path.exists(paths["spectrum"])
        for n in ("swd", "msssim"):
            os.remove(paths[n])
        entry.main(base + ["--spectrum", "--swd", "--msssim"])      # one pass for all three
        shared = open(paths["spectrum"], "rb").read()
        for n in ("swd", "msssim"):
            assert open(paths[n], "rb").read() == without[n], "%s.json changed its bytes beside --spectrum" % n
            os.remove(paths[n])
        os.remove(paths["spectrum"])

        def no_trunk(self):
            raise AssertionError("spectrum() alone must not load the image encoder")
        monkeypatch.setattr(CheckpointEvaluation, "_load_image_encoder", no_trunk)
        entry.main(base + ["--spectrum"])                           # alone, through main.py
        assert open(paths["spectrum"], "rb").read() == shared and not os.path.exists(paths["swd"])
        os.remove(paths["spectrum"])
        cfg_from_main = (cfg.TRAIN.NET_G, cfg.TRAIN.FLAG)
        assert cfg_from_main == (ckpt, False)
        capsys.readouterr()
        algo = _main_trainer(tmp_path)
        out = algo.spectrum("test", seed=7)                         # directly
        text = capsys.readouterr().out
        assert open(paths["spectrum"], "rb").read() == shared and json.loads(shared) == out
        assert "Spectrum (12 real, 12 generated images; window hann): LSD " in text and "spectrum.json" in text
        assert set(out) == KEYS and (out["size"], out["window"], out["n_real"], out["n_fake"], out["seed"]) == (256, "hann", 12, 12, 7)
        assert (out["NET_G"], out["NET_E"]) == (ckpt, '') and len(out["count"]) == len(out["excess_db"]) == 182
        for word in ("trunk-free", "window", "not quantised", "partial rings"):
            assert word in out["note"], word
        assert out["empty_bins"] == [] and out["lsd_db"] > 0 and out["peak"]["period"] == 256.0 / out["peak"]["bin"]
        other = algo.spectrum("test", seed=7, window="none")
        assert other["window"] == "none" and other["lsd_db"] != out["lsd_db"]
        entry.main(base + ["--spectrum", "--spectrum_window", "none"])
        assert json.load(open(paths["spectrum"])) == other
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.FLAG = '', True


def test_a_period_4_grid_on_the_generated_side_is_reported_at_period_4(tmp_path):
    cfg, ev, ckpt = _tiny_checkpoint(tmp_path)
    try:
        algo = _main_trainer(tmp_path)
        seen = []
        algo.pool_codes("test", seed=7, want_real=False, trunk=False, image_sink=lambda real, fake, take: seen.append(fake[:take].float()))
        fake = torch.cat(seen).contiguous()
        assert tuple(fake.shape) == (12, 3, 256, 256)
        i = torch.arange(256, device=fake.device, dtype=torch.float32)
        wave = torch.cos(2 * np.pi * i / 4)
        grid = 0.05 * 0.5 * (wave[:, None] + wave[None, :])         # period 4 along both axes, amplitude 0.05
        plain = SP.RadialSpectrum(256, 3, 12, device=DEV)
        plain.add(fake, fake.clone())
        marked = SP.RadialSpectrum(256, 3, 12, device=DEV)
        marked.add(fake, (fake + grid).contiguous())
        a, b = plain.result(), marked.result()
        assert a["lsd_db"] == 0.0 and a["hf_db"] == 0.0 and all(d == 0.0 for d in a["excess_db"])
        print("with the grid: peak %s, hf_db %.4f, lsd_db %.4f" % (b["peak"], b["hf_db"], b["lsd_db"]))
        assert b["peak"]["bin"] == 64 and b["peak"]["period"] == 4.0 and b["peak"]["excess_db"] > 0
        assert b["hf_db"] > a["hf_db"] and b["lsd_db"] > 0
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.FLAG = '', True
