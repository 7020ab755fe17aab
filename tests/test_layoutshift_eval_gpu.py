"""-m gpu: the layout-shift score end to end -- on eval_setup's tiny checkpoint through attngan/main.py and
directly, with the A images held bit for bit to those of pool_codes under the same seed and the JSON to the figures of the numpy
oracle on the images read back; the same through two family trees' main.py (multi-mnist, and coco stage II, which moves both box
sets); and the two behavioural checks with stand-in generators: one that paints every box's rectangle in a flat colour on a textured
ground must score follow = 1 and locality = 1 exactly, one that ignores `tmi` follow = 0 with every pair unchanged.

The tolerance of the oracle comparison is derived in _close; no bound here comes from the code under test."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

import layout_cases as LC
from eval_setup import tiny_checkpoint as _tiny_checkpoint
from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import layoutshift as LS  # noqa: E402
from mogan_amd.attngan.datasets import SyntheticTextDataset  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIGURES = ("follow", "locality", "area_share", "spill_others", "spill_background")
KEYS = {"n_pairs", "flat", "unchanged", "follow", "locality", "area_share", "change", "spill_others", "spill_background", "most_ignored",
        "n_images", "no_objects", "immovable", "min_shift", "min_side", "size", "show", "grid", "seed", "NET_G", "note"}


class Pairs:
    """an image sink of layout_shift(): the pairs' images and tables on the host, every A image of the pass beside them"""

    def __init__(self):
        self.a, self.b, self.edit, self.others, self.every_a = [], [], [], [], []

    def __call__(self, a, b, table, take):
        rows = table["row"].to(a.device)
        self.a.append(a[rows].float().cpu())
        self.b.append(b[rows].float().cpu())
        self.edit.append(table["edit"])
        self.others.append(table["others"])
        self.every_a.append(a[:take].clone())

    def oracle(self, size, channels, show):
        a, b = torch.cat(self.a).numpy(), torch.cat(self.b).numpy()
        edit, others = torch.cat(self.edit).numpy(), torch.cat(self.others).numpy()
        sums, counts = LS.sums_numpy(a, b, edit, others)
        return LS.figures(sums, counts, size, channels, show), sums, counts, edit


def _close(out, want, sums, counts, edit, channels):
    """The JSON against the oracle's figures.  Every device sum is within r = (n + 4) 2^-52 of the oracle's, relatively
    (tests/layout_cases.py), n <= S S C; a ratio of two such sums, or of sums of them, is within 3 r of the oracle's ratio, relatively;
    1 - ratio, a mean of such values and their population standard deviation (1-Lipschitz in every value up to a factor 2) are
    therefore within 6 r v of the oracle's, v the largest magnitude among the pairs' values.  Integers are exact."""
    r = float(LC.addends(counts, edit, channels).max() + 4) * LC.EPS
    with np.errstate(divide="ignore", invalid="ignore"):
        follow = LS.follow_of(sums)
        box = sums[:, :3].sum(axis=1) / counts[:, :3].sum(axis=1)
        spill = np.concatenate([(sums[:, k] / counts[:, k]) / box for k in (3, 4)])
    v = 1.0 + max(float(np.nanmax(np.abs(follow))), float(np.nanmax(np.where(np.isfinite(spill), spill, 0.0))))
    for k in ("n_pairs", "flat", "unchanged"):
        assert out[k] == want[k], k
    worst = 0.0
    for k in FIGURES:
        assert out[k]["n"] == want[k]["n"], k
        for part in ("mean", "std"):
            if want[k][part] is None:
                assert out[k][part] is None
            else:
                worst = max(worst, abs(out[k][part] - want[k][part]) / (6 * r * v))
                assert abs(out[k][part] - want[k][part]) <= 6 * r * v, (k, part, out[k][part], want[k][part])
    for name, st in want["change"].items():
        assert out["change"][name]["n"] == st["n"]
        if st["n"]:
            assert abs(out["change"][name]["mean"] - st["mean"]) <= 2 * r * st["mean"] and abs(out["change"][name]["std"] - st["std"]) <= 4 * r * 4.0
    print("the figures use %.4f of their tolerance at the most" % worst)
    return [e["pair"] for e in out["most_ignored"]]


def _main_trainer(tmp_path, seed=7, length=12, dataset=None):
    """the trainer main.py builds for --synthetic 12 --manualSeed 7 under the tiny config"""
    from mogan_amd.attngan.miscc.config import cfg
    from mogan_amd.attngan.trainer import condGANTrainer
    ds = dataset or SyntheticTextDataset(length, seed=seed, eval=False)
    dl = torch.utils.data.DataLoader(ds, batch_size=cfg.TRAIN.BATCH_SIZE, drop_last=True, shuffle=True, num_workers=0)
    return condGANTrainer(str(tmp_path), dl, ds.n_words, ds.ixtoword, '', distributed=False)


# ------------------------------------------------------------------------------------------------- 1: coco-attngan
def test_layout_shift_through_main_twice_and_directly_with_the_same_bytes(tmp_path, capsys, monkeypatch):
    from mogan_amd.attngan import main as entry
    from mogan_amd.attngan.evaluate import CheckpointEvaluation
    cfg, ev, ckpt = _tiny_checkpoint(tmp_path)
    try:
        def no_trunk(self):
            raise AssertionError("layout_shift() must not load the image encoder")
        monkeypatch.setattr(CheckpointEvaluation, "_load_image_encoder", no_trunk)
        base = ["--cfg", str(ev), "--synthetic", "12", "--manualSeed", "7", "--output_dir", str(tmp_path), "--layout_shift",
                "--ls_min_shift", "24", "--ls_show", "5"]
        paths = [os.path.join(ckpt[:-4], "valid", n) for n in ("layout_shift.json", "layout_grid.png")]
        entry.main(base)
        first = [open(p, "rb").read() for p in paths]
        for p in paths:
            os.remove(p)
        entry.main(base)
        assert [open(p, "rb").read() for p in paths] == first                   # twice: the same bytes
        for p in paths:
            os.remove(p)
        capsys.readouterr()
        algo = _main_trainer(tmp_path)
        seen = Pairs()
        out = algo.layout_shift("test", seed=7, min_shift=24, show=5, image_sink=seen)         # directly
        text = capsys.readouterr().out
        assert [open(p, "rb").read() for p in paths] == first and json.loads(first[0]) == json.loads(json.dumps(out))
        assert "Layout shift (%d pairs of 12 images; " % out["n_pairs"] in text and "layout_shift.json and layout_grid.png" in text
        assert set(out) == KEYS | {"NET_E"} and (out["size"], out["seed"], out["NET_G"], out["min_shift"], out["n_images"]) == (256, 7, ckpt, 24, 12)
        # the cap: at least half of the split's images yield a pair (every synthetic image has two or three boxes of at most half the
        # side, so draw_edit finds an offset of 24 pixels for each)
        assert out["n_pairs"] >= 6 and out["n_pairs"] + out["no_objects"] + out["immovable"] == 12
        assert out["show"] == len(out["most_ignored"]) == 5 and out["grid"] == "layout_grid.png"
        for word in ("same noise", "follow", "locality", "area_share", "min_shift"):
            assert word in out["note"], word
        from PIL import Image
        grid = Image.open(paths[1])
        assert grid.size == (3 * 256, 5 * 256) and grid.mode == "RGB"
        # the JSON against the oracle on the images read back
        want, sums, counts, edit = seen.oracle(256, 3, 5)
        assert _close(out, want, sums, counts, edit, 3) == [e["pair"] for e in want["most_ignored"]]
        for e in out["most_ignored"]:
            assert e["key"].startswith("synthetic_") and e["rect"] + e["offset"] == edit[e["pair"]].tolist() and 0 <= e["slot"] < 3
            assert max(abs(e["offset"][0]), abs(e["offset"][1])) >= 24
        # the A images are those every other score sees under the seed, bit for bit
        fakes = []
        algo = _main_trainer(tmp_path)
        algo.pool_codes("test", seed=7, want_real=False, trunk=False, image_sink=lambda real, fake, take: fakes.append(fake[:take].clone()))
        ours, theirs = torch.cat(seen.every_a), torch.cat(fakes)
        assert tuple(ours.shape) == (12, 3, 256, 256) and ours.dtype == theirs.dtype
        assert torch.equal(ours.view(torch.int32), theirs.view(torch.int32))
        assert not torch.equal(torch.cat(seen.a), torch.cat(seen.b))             # and the edit reaches the generator
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.FLAG = '', True


class AlignedBoxes(SyntheticTextDataset):
    """the synthetic split with one to three boxes per image whose corners lie on pixel corners of the 256 x 256 image: every value is
    k / 256, so the fp32 matrices of a box and of its moved copy hold the box exactly enough for a stand-in that paints from `tmi`"""

    def __getitem__(self, index):
        item = list(super().__getitem__(index))
        rng = np.random.RandomState(977 + index)
        bbox = np.full((3, 4), -1.0, dtype=np.float32)
        for g in range(1 + index % 3):
            bbox[g] = np.array([rng.randint(0, 129), rng.randint(0, 129), rng.randint(16, 101), rng.randint(16, 101)]) / 256.0
        item[5] = self._matrices(bbox)
        return tuple(item)


class StandIn(torch.nn.Module):
    """G_NET's call: a textured ground that depends on the noise alone; paint=True: every box of `tmi` as a rectangle of one flat colour"""

    def __init__(self, paint):
        super().__init__()
        self.paint = paint
        self.ground = torch.from_numpy(np.random.RandomState(3).uniform(-0.9, 0.9, (3, 256, 256)).astype(np.float32))

    def forward(self, noise, sent_emb, words_embs, mask, tmi, label_one_hot, eps=None):
        img = self.ground.to(noise.device)[None] * (0.6 + 0.3 * torch.tanh(noise[:, :1]))[:, :, None, None]
        img = img.contiguous()
        if self.paint:
            t = tmi.double().cpu().numpy()
            for b in range(t.shape[0]):
                for g in range(t.shape[1]):
                    if t[b, g, 0, 0] <= 0:
                        continue
                    w, h = 1.0 / t[b, g, 0, 0], 1.0 / t[b, g, 1, 1]
                    x, y = 0.5 - t[b, g, 0, 2] * w / 2 - w / 2, 0.5 - t[b, g, 1, 2] * h / 2 - h / 2
                    x0, y0, x1, y1 = LS.pixel_rect([x, y, w, h], 256)
                    img[b, :, y0:y1, x0:x1] = 0.5
        return [img], None, None, None


@pytest.mark.parametrize("paint", (True, False), ids=("a painter of boxes", "a generator that ignores tmi"))
def test_stand_in_generators_score_what_they_do(tmp_path, monkeypatch, paint):
    from mogan_amd.attngan.evaluate import CheckpointEvaluation
    cfg, ev, ckpt = _tiny_checkpoint(tmp_path)
    try:
        load = CheckpointEvaluation._load_eval_models

        def stand_in(self):
            return StandIn(paint).to(self.device), load(self)[1]
        monkeypatch.setattr(CheckpointEvaluation, "_load_eval_models", stand_in)
        algo = _main_trainer(tmp_path, dataset=AlignedBoxes(12, seed=7, eval=False))
        seen = Pairs()
        out = algo.layout_shift("test", seed=7, show=3, image_sink=seen)
        n = out["n_pairs"]
        assert n >= 6 and n + out["no_objects"] + out["immovable"] == 12 and out["flat"] == 0 and out["min_shift"] == 32
        if paint:
            assert out["follow"] == {"mean": 1.0, "std": 0.0, "n": n} and out["locality"] == {"mean": 1.0, "std": 0.0, "n": n}
            assert out["unchanged"] == 0 and out["spill_background"]["mean"] == 0.0 and out["change"]["rest"]["mean"] == 0.0
            assert out["change"]["others"]["n"] == 0 or out["change"]["others"]["mean"] == 0.0
        else:
            assert out["follow"] == {"mean": 0.0, "std": 0.0, "n": n} and out["unchanged"] == n and out["locality"]["n"] == 0
            assert torch.equal(torch.cat(seen.a), torch.cat(seen.b))
        want, sums, counts, edit = seen.oracle(256, 3, 3)
        assert (want["follow"], want["locality"], want["unchanged"]) == (out["follow"], out["locality"], out["unchanged"])
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.FLAG = '', True


# ------------------------------------------------------------------------------------------------- 2: the family trees
COMMON = "GPU_ID: '0'\nZ_DIM: 100\nWORKERS: 0\nUSE_BBOX_LAYOUT: True\n"
TREES = {
    "mnist": ("multi_mnist", 1, "GAN: {CONDITION_DIM: 128, DF_DIM: 4, GF_DIM: 4}\n", 4),
    "coco_s2": ("coco", 2, "STAGE: 2\nIMSIZE: 256\nGAN: {CONDITION_DIM: 128, DF_DIM: 4, GF_DIM: 192, R_NUM: 1}\nTEXT: {DIMENSION: 16}\n", 2),
}


def _checkpoint(tmp_path, case):
    """(entry module, cfg, yml path, checkpoint path): a seeded random-init generator written by the tree's own save_model"""
    from mogan_amd.stackgan.trainer_base import save_model, weights_init
    pkg, stage, gan, batch = TREES[case]
    entry = importlib.import_module("mogan_amd.stackgan.%s.main" % pkg)
    model = importlib.import_module("mogan_amd.stackgan.%s.model" % pkg)
    text = COMMON + gan
    train = tmp_path / "init.yml"
    train.write_text(text + "NET_G: ''\nTRAIN: {FLAG: True, BATCH_SIZE: %d}\n" % batch)
    entry.cfg_from_file(str(train))
    torch.manual_seed(5)
    netG = model.STAGE1_G() if stage == 1 else model.STAGE2_G(model.STAGE1_G())
    netG.apply(weights_init)
    model_dir = tmp_path / "Model"
    model_dir.mkdir()
    save_model(netG, None, None, None, 0, str(model_dir))
    ckpt = str(model_dir / "checkpoint_0000.pth")
    ev = tmp_path / "eval.yml"
    ev.write_text(text + "NET_G: '%s'\nTRAIN: {FLAG: False, BATCH_SIZE: %d}\n" % (ckpt, batch))
    return entry, entry.cfg, str(ev), ckpt


@pytest.mark.parametrize("case", list(TREES))
def test_layout_shift_through_a_family_trees_main(tmp_path, case):
    entry, cfg, ev, ckpt = _checkpoint(tmp_path, case)
    size, channels, batch = (256 if case == "coco_s2" else 64), (1 if case == "mnist" else 3), TREES[case][3]
    n_images = 12 if case == "mnist" else 6
    try:
        base = ["--cfg", ev, "--synthetic", str(n_images), "--batch_size", str(batch), "--manualSeed", "7", "--output_dir", str(tmp_path),
                "--layout_shift", "--ls_show", "4"]
        algo = entry.main(base)
        d = os.path.join(ckpt[:-4], "synthetic")
        assert sorted(os.listdir(d)) == ["layout_grid.png", "layout_shift.json"]
        first = {f: open(os.path.join(d, f), "rb").read() for f in os.listdir(d)}
        out = json.loads(first["layout_shift.json"])
        assert out == json.loads(json.dumps(algo.scores["layout_shift"]))
        assert (out["seed"], out["NET_G"], out["size"], out["channels"], out["split"], out["stage"]) == (
            7, ckpt, size, channels, "synthetic", TREES[case][1])
        assert out["min_shift"] == size // 8 and out["n_images"] == n_images and out["grid"] == "layout_grid.png"
        # the cap: every synthetic item has boxes of at most half the side, so draw_edit finds an offset for each
        assert out["n_pairs"] >= n_images // 2 and out["n_pairs"] + out["no_objects"] + out["immovable"] == n_images
        for f in first:
            os.remove(os.path.join(d, f))
        seen = Pairs()
        again = algo.evaluation.layout_shift(30000, 7, None, 1, 4, image_sink=seen)            # a second run: the same bytes
        assert {f: open(os.path.join(d, f), "rb").read() for f in os.listdir(d)} == first and json.loads(json.dumps(again)) == out
        want, sums, counts, edit = seen.oracle(size, channels, 4)
        assert _close(out, want, sums, counts, edit, channels) == [e["pair"] for e in want["most_ignored"]]
        assert all(e["key"] == "synthetic_%06d" % e["image"] for e in out["most_ignored"])
        assert not torch.equal(torch.cat(seen.a), torch.cat(seen.b))             # the edit reaches the generator
        # the A images are those of the scores' own pass under the seed, bit for bit
        fakes = []
        algo.evaluation.one_pass(30000, 7, image_sinks=[lambda real, fake, take: fakes.append(fake[:take].clone())])
        ours, theirs = torch.cat(seen.every_a), torch.cat(fakes)
        assert tuple(ours.shape) == (n_images, channels, size, size)
        assert torch.equal(ours.float().view(torch.int32), theirs.float().view(torch.int32))
    finally:
        cfg.NET_G, cfg.TRAIN.FLAG = '', True
        if "STAGE" in cfg:
            cfg.STAGE = 1
