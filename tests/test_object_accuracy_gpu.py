"""-m gpu: object accuracy by nearest labelled training crops end to end (stackgan/objaccuracy.py has the
definition, stackgan/evaluate.py the pass).

(a) the accumulator ObjectCrops driven directly with hand-made images in which every class paints a constant pattern of its own
    into its (pixel-aligned) box: "generated" images equal to the data are right everywhere -- accuracy, accuracy_1nn and margin
    exactly 1 -- and the same images asked for the next class are wrong everywhere;
(b) the three trees' main.py on synthetic items with a checkpoint written by the tree's own save_model: every integer figure of
    object_accuracy.json equals the numpy definition applied to numpy fp64 distances of the crops the pass returns (the test
    first checks, on those numpy distances alone, that every query's distances are MARGIN apart, so no fp64 evaluation orders
    them differently); all flags together give each file the bytes of its flag alone; two runs under one seed give the same bytes;
    the same mains on tiny real-data trees: the 'test' split against a bank of the 'train' split;
(c) without a score flag main still reaches sample and train as before (a stand-in trainer)."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

import nn_cases as C
import prdc_cases as P
from helpers import load_pkg

load_pkg()
from mogan_amd.attngan.synthetic import bbox_to_theta  # noqa: E402
from mogan_amd.stackgan import evaluate as EV  # noqa: E402
from mogan_amd.stackgan import main_base  # noqa: E402
from mogan_amd.stackgan import objaccuracy as OA  # noqa: E402
from mogan_amd.stackgan.trainer_base import save_model, weights_init  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
INTEGERS = ("n", "right", "right_1nn", "classes", "per_class", "images", "margin_n", "margin_left_out")


# ------------------------------------------------------------------------------------------------- (a) hand-made images
def _painted(tree, n_images, first_class, seed):
    """(images (n, C, 64, 64), tm (n, G, 2, 3), label_one_hot (n, G, L), classes (n, G) with -1 for an absent slot): 20 x 20 pixel
    boxes in columns of their own (they never overlap), at a random row; class c paints the constant PATTERN[c] into its box"""
    rng = np.random.RandomState(seed)
    G, C_, L = (4, 3, 13) if tree == "clevr" else (3, 1, 10)
    n_classes = 12 if tree == "clevr" else 10                    # clevr: shapes 0..2 x colours 0..3
    img = rng.uniform(-0.05, 0.05, (n_images, C_, 64, 64)).astype(np.float32)
    bbox = np.full((n_images, G, 4), -1.0 / 64.0, dtype=np.float32)
    lab = np.zeros((n_images, G, L), dtype=np.float32)
    classes = np.full((n_images, G), -1, dtype=np.int64)
    for i in range(n_images):
        for g in range(3):                                       # clevr's fourth slot stays absent
            c = (first_class + 3 * i + g) % n_classes
            x0, y0 = 22 * g, int(rng.randint(0, 44))
            bbox[i, g] = (x0 / 64.0, y0 / 64.0, 20 / 64.0, 20 / 64.0)
            if tree == "clevr":
                shape, colour = c // 4, c % 4
                lab[i, g, shape], lab[i, g, 4 + colour] = 1, 1
                classes[i, g] = shape * 9 + colour
                pattern = (-0.9 + 0.6 * shape, -0.9 + 0.5 * colour, 0.3)
            else:
                lab[i, g, c] = 1
                classes[i, g] = c
                pattern = (-0.9 + 0.2 * c,)
            for ch in range(C_):
                img[i, ch, y0:y0 + 20, x0:x0 + 20] = pattern[ch]
        if tree == "clevr":
            lab[i, 3, 3], lab[i, 3, 12] = 1, 1                   # the absent slot's classes
    tm = bbox_to_theta(torch.from_numpy(bbox).view(-1, 4))[0].view(n_images, G, 2, 3)
    return torch.from_numpy(img), tm, torch.from_numpy(lab), classes


def _fill(acc, img, tm, lab, fake=None, batch=4):
    for s in range(0, img.shape[0], batch):
        e = min(s + batch, img.shape[0])
        real = img[s:e].to(DEV)
        acc.sink(real, real if fake is None else fake[s:e].to(DEV), tm[s:e].to(DEV), lab[s:e].to(DEV), e - s)
    return acc


@pytest.mark.parametrize("tree", ["mnist", "clevr"])
def test_painted_classes_are_found_and_rotated_labels_are_not(tree):
    G, C_ = (4, 3) if tree == "clevr" else (3, 1)
    n_classes = 12 if tree == "clevr" else 10
    b_img, b_tm, b_lab, b_cls = _painted(tree, 20, 0, seed=1)            # the bank: 60 objects, every class five or six times
    q_img, q_tm, q_lab, q_cls = _painted(tree, 10, 1, seed=2)            # the evaluation split: 30 objects in three batches
    bank = _fill(EV.ObjectCrops(tree, 20, 64, C_, G, device=DEV, both=False), b_img, b_tm, b_lab)
    bank_classes = bank.objects()[0].numpy()
    assert bank.n == 60 and (bank_classes == b_cls[b_cls >= 0]).all() and min(np.unique(bank_classes, return_counts=True)[1]) >= 5
    acc = _fill(EV.ObjectCrops(tree, 10, 64, C_, G, device=DEV), q_img, q_tm, q_lab)
    asked, image, slot, box = (t.numpy() for t in acc.objects())
    assert acc.n == 30 and acc.n_images == 10 and (asked == q_cls[q_cls >= 0]).all()
    assert image.tolist() == [i for i in range(10) for _ in range(3)] and slot.tolist() == [0, 1, 2] * 10
    crops = acc.finish()
    assert crops["real"].shape == (30, C_ * 256) and torch.equal(crops["real"], crops["fake"])      # generated = the data
    found = EV.search(crops["fake"], asked, bank.finish()["real"], bank_classes, 5)
    assert (found["same_d2"] == 0).all() and (found["other_d2"] > 0).all() and (found["d2"][:, :5] == 0).all()
    assert (found["neighbour_classes"] == asked[:, None]).all()
    # a class's crops are bit copies of each other, so the first of them by position is the one listed
    first = {int(c): int(np.nonzero(bank_classes == c)[0][0]) for c in np.unique(bank_classes)}
    assert found["same_idx"].tolist() == [first[int(c)] for c in asked] and found["idx"][:, 0].tolist() == found["same_idx"].tolist()
    out = EV.figures_of(found, asked, image)
    assert out["accuracy"] == out["accuracy_1nn"] == out["accuracy_per_class"] == out["accuracy_per_image"] == 1.0
    assert out["right"] == out["right_1nn"] == out["n"] == 30 and out["margin"] == 1.0 and out["margin_left_out"] == 0
    assert out["classes"] == n_classes and out["images"] == 10
    # the same images, asked for the next class
    order = np.unique(bank_classes)
    nxt = dict(zip(order.tolist(), np.roll(order, -1).tolist()))
    rotated = np.array([nxt[int(c)] for c in asked])
    found = EV.search(crops["fake"], rotated, bank.finish()["real"], bank_classes, 5)
    assert (found["other_d2"] == 0).all() and (found["same_d2"] > 0).all()
    out = EV.figures_of(found, rotated, image)
    assert out["accuracy"] == out["accuracy_1nn"] == out["accuracy_per_class"] == out["accuracy_per_image"] == 0.0
    assert out["right"] == out["right_1nn"] == 0 and out["margin"] == -1.0 and out["margin_left_out"] == 0


# ------------------------------------------------------------------------------------------------- (b) main, end to end
COMMON = "GPU_ID: '0'\nZ_DIM: 100\nWORKERS: 0\nUSE_BBOX_LAYOUT: True\n"
TREES = {
    "mnist": ("multi_mnist", 1, "GAN: {CONDITION_DIM: 128, DF_DIM: 4, GF_DIM: 4}\n", 4),
    "clevr": ("clevr", 1, "GAN: {CONDITION_DIM: 16, DF_DIM: 4, GF_DIM: 4}\n", 4),
    "coco_s1": ("coco", 1, "STAGE: 1\nIMSIZE: 64\nGAN: {CONDITION_DIM: 128, DF_DIM: 4, GF_DIM: 192}\nTEXT: {DIMENSION: 16}\n", 4),
    "coco_s2": ("coco", 2, "STAGE: 2\nIMSIZE: 256\nGAN: {CONDITION_DIM: 128, DF_DIM: 4, GF_DIM: 192, R_NUM: 1}\nTEXT: {DIMENSION: 16}\n", 2),
}
FILES = {"object_accuracy": ("object_accuracy.json", "oa_grid.png"), "swd": ("swd.json",), "msssim": ("msssim.json",),
         "spectrum": ("spectrum.json",)}


def _checkpoint(tmp_path, case):
    """(entry module, cfg, yml path, checkpoint path): a seeded random-init generator written by the tree's own save_model"""
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


def _restore(cfg):
    cfg.NET_G, cfg.TRAIN.FLAG = '', True
    if "STAGE" in cfg:
        cfg.STAGE = 1


def _read(ckpt, names):
    out = {}
    for n in names:
        for f in FILES[n]:
            path = os.path.join(ckpt[:-4], "synthetic", f)
            assert os.path.isfile(path), path
            out[f] = open(path, "rb").read()
    return out


def _wipe(ckpt):
    d = os.path.join(ckpt[:-4], "synthetic")
    for f in os.listdir(d):
        os.remove(os.path.join(d, f))


def _numpy_found(queries, asked, bank, bank_classes, k):
    """what evaluate.search returns, from numpy fp64 distances, and the smallest relative gap between two distances of one query"""
    d2 = P.numpy_fp64_d2(queries, bank)
    top, order = C.nearest(d2, d2.shape[1])
    scale = np.maximum((queries.astype(np.float64) ** 2).sum(1)[:, None] + (bank.astype(np.float64) ** 2).sum(1)[None, :], 1e-300)
    gap = float(((top[:, 1:] - top[:, :-1]) / np.take_along_axis(scale, order, axis=1)[:, 1:]).min())
    found = {"d2": top[:, :k], "idx": order[:, :k], "neighbour_classes": bank_classes[order[:, :k]]}
    for name, keep in (("same", bank_classes[None, :] == asked[:, None]), ("other", bank_classes[None, :] != asked[:, None])):
        masked = np.where(keep, d2, np.inf)
        has = keep.any(1)
        found[name + "_idx"] = np.where(has, masked.argmin(1), OA.NO_ROW)
        found[name + "_d2"] = np.where(has, masked.min(1), np.inf)
    return found, gap


@pytest.mark.parametrize("case", list(TREES))
def test_main_scores_a_checkpoint(tmp_path, case):
    entry, cfg, ev, ckpt = _checkpoint(tmp_path, case)
    batch = TREES[case][3]
    try:
        base = ["--cfg", ev, "--synthetic", "12", "--batch_size", str(batch), "--manualSeed", "7", "--output_dir", str(tmp_path)]
        every = ["--object_accuracy", "--swd", "--msssim", "--spectrum", "--oa_k", "3", "--oa_show", "4", "--swd_patches", "16",
                 "--swd_dirs", "16", "--swd_repeats", "1"]
        algo = entry.main(base + every)
        together = _read(ckpt, FILES)
        assert set(algo.scores) == set(FILES)
        out = json.loads(together["object_accuracy.json"])
        assert out == json.loads(json.dumps(algo.scores["object_accuracy"]))
        size, channels = (256 if case == "coco_s2" else 64), (1 if case == "mnist" else 3)
        assert (out["seed"], out["NET_G"], out["k"], out["side"], out["D"]) == (7, ckpt, 3, 16, channels * 256)
        assert (out["size"], out["channels"], out["split"], out["bank_split"], out["n_images"]) == (size, channels, "synthetic",
                                                                                                    "synthetic-train", 12)
        assert "second synthetic set" in out["note"] and "depends on side (16), k (3) and the bank" in out["note"]
        assert out["n_objects"] == out["generated"]["n"] == out["real"]["n"] and out["n_bank_images"] == 12
        assert 24 <= out["n_objects"] <= 12 * (4 if case == "clevr" else 3) and out["unlabelled"] == 0
        assert out["show"] == len(out["most_wrong"]) == 4 and out["grid"] == "oa_grid.png"
        for e in out["most_wrong"]:
            assert len(e["neighbours"]) == len(e["d2"]) == 3 and e["d2"] == sorted(e["d2"]) and len(e["box"]) == 4
            assert all(p["key"] == "synthetic_%06d" % p["image"] for p in e["neighbours"])
            assert e["same"] is None or e["same"]["class"] == e["asked"]
            assert e["other"] is None or e["other"]["class"] != e["asked"]
        from PIL import Image
        grid = Image.open(os.path.join(ckpt[:-4], "synthetic", "oa_grid.png"))
        assert grid.size == ((3 + 3) * 16, 4 * 16) and grid.mode == "RGB" and np.asarray(grid).std() > 0
        for name, keys in (("swd", ("swd", "per_level")), ("msssim", ("real", "generated", "same_caption")), ("spectrum", ("lsd_db",))):
            got = json.loads(together[name + ".json"])
            assert all(k in got for k in keys + ("seed", "NET_G", "note", "size", "channels")) and got["size"] == size
        # a second run, on the evaluation main made: the same bytes, and the crops behind the figures
        _wipe(ckpt)
        again, crops = algo.evaluation.run_scores({"object_accuracy": dict(k=3, side=16, min_side=1, bank_size=None, show=4)},
                                                  num_samples=30000, seed=7, return_crops=True)["object_accuracy"]
        alone = _read(ckpt, ["object_accuracy"])
        assert alone == {f: together[f] for f in alone}                      # its flag alone, and a second run: the same bytes
        asked, image, bank_classes = crops["asked"], crops["image"], crops["bank_classes"]
        for side, key in (("fake", "generated"), ("real", "real")):
            found, gap = _numpy_found(crops[side].numpy(), asked, crops["bank"].numpy(), bank_classes, 3)
            print("%s %s: the closest two distances of one query are %.3e apart (MARGIN %.0e)" % (case, key, gap, C.MARGIN))
            assert gap >= C.MARGIN                                           # a condition on the inputs, from numpy alone
            want = OA.figures(asked, found["neighbour_classes"], found["same_d2"], found["same_idx"], found["other_d2"],
                              found["other_idx"], image)
            assert {k: out[key][k] for k in INTEGERS} == {k: want[k] for k in INTEGERS}, key
            assert out[key]["accuracy"] == want["right"] / want["n"] and out[key]["accuracy_1nn"] == want["right_1nn"] / want["n"]
        if case == "coco_s2":
            return
        # every other flag alone gives the bytes it had beside the others (mnist: each; the larger trees: one, to stay quick)
        alone_flags = {"mnist": ("swd", "msssim", "spectrum"), "clevr": ("swd",), "coco_s1": ("msssim",)}[case]
        for name in alone_flags:
            _wipe(ckpt)
            entry.main(base + ["--" + name] + every[4:])
            assert os.listdir(os.path.join(ckpt[:-4], "synthetic")) == [name + ".json"]
            assert _read(ckpt, [name]) == {name + ".json": together[name + ".json"]}, name
    finally:
        _restore(cfg)


@pytest.mark.parametrize("case", list(TREES))
def test_main_scores_the_real_data_splits(tmp_path, case):
    """the 'test' split against a bank of the 'train' split through the trees' TextDatasets (tests/stackgan_data_cases.py builds the
    file formats): uncropped, unflipped items, keys from the file names; the tiny coco tree's two splits hold the same six images,
    so every real object finds itself in the bank at exactly 0"""
    import stackgan_data_cases as D
    entry, cfg, ev, ckpt = _checkpoint(tmp_path, case)
    tree = TREES[case][0]
    try:
        extra = ""
        if tree == "coco":
            data_dir, img_dir, raw = D.build_coco_tree(str(tmp_path))
            extra = "IMG_DIR: '%s'\n" % img_dir
        else:
            data_dir = (D.build_clevr_tree if tree == "clevr" else D.build_mnist_tree)(str(tmp_path))
        with open(ev, "a") as f:
            f.write(extra)
        algo = entry.main(["--cfg", ev, "--data_dir", data_dir, "--batch_size", "4", "--manualSeed", "7", "--output_dir", str(tmp_path),
                           "--object_accuracy", "--spectrum", "--oa_k", "2", "--oa_show", "3"])
        d = os.path.join(ckpt[:-4], "test")
        assert sorted(os.listdir(d)) == ["oa_grid.png", "object_accuracy.json", "spectrum.json"]
        out = json.load(open(os.path.join(d, "object_accuracy.json")))
        assert (out["split"], out["bank_split"], out["n_images"], out["n_bank_images"]) == ("test", "train", D.N_ITEMS, D.N_ITEMS)
        assert "second synthetic set" not in out["note"] and out["unlabelled"] == 0
        want = {"multi_mnist": 3 * D.N_ITEMS, "clevr": sum(1 + i % 4 for i in range(D.N_ITEMS)),
                "coco": sum(2 + i % 2 for i in range(D.N_ITEMS))}[tree]
        assert out["n_objects"] == out["n_bank"] == want == out["real"]["n"] == out["generated"]["n"]
        names = {"multi_mnist": "%05d.png", "clevr": "CLEVR_train_%06d.json", "coco": "COCO_train2014_%012d"}[tree]
        bank_names = algo.evaluation.bank[0].filenames
        for e in out["most_wrong"]:
            assert all(p["key"] == os.path.basename(bank_names[p["image"]]) for p in e["neighbours"]), e
            assert tree == "clevr" or all(p["key"] == names % p["image"] for p in e["neighbours"]), e
        if tree == "clevr":                                    # glob's order is the file system's: every scene once, whatever the order
            assert sorted(algo.evaluation.bank[0].filenames) == sorted(os.path.join(data_dir, "train", "scenes", names % i)
                                                                       for i in range(D.N_ITEMS))
        if tree == "coco":
            assert out["real"]["right_1nn"] == want and out["real"]["accuracy_1nn"] == 1.0 and out["real"]["margin"] == 1.0
            assert out["size"] == (256 if case == "coco_s2" else 64)
        assert json.load(open(os.path.join(d, "spectrum.json")))["n_real"] == D.N_ITEMS
    finally:
        _restore(cfg)
        if "IMG_DIR" in cfg:
            cfg.IMG_DIR = ''
        cfg.DATA_DIR = ''


# ------------------------------------------------------------------------------------------------- (c) the unchanged path
def test_without_a_score_flag_main_samples_and_trains_as_before(tmp_path, monkeypatch):
    from mogan_amd.stackgan.multi_mnist.miscc.config import cfg, cfg_from_file
    seen = []

    class StandIn:
        def __init__(self, output_dir, use_graph=False):
            seen.append(("init", use_graph))

        def sample(self, data, num_samples=25, **kw):
            seen.append(("sample", data, num_samples, kw))

        def train(self, loader, stage):
            seen.append(("train", len(loader.dataset), loader.batch_size, stage))

    monkeypatch.setattr(main_base, "score", lambda *a, **k: seen.append(("score", list(a[5]))))
    try:
        off = tmp_path / "off.yml"
        off.write_text(COMMON + "NET_G: 'none.pth'\nDATA_DIR: 'data'\nTRAIN: {FLAG: False, BATCH_SIZE: 4}\n")
        base = ["--cfg", str(off), "--manualSeed", "3", "--output_dir", str(tmp_path)]
        main_base.run("mnist", cfg, cfg_from_file, StandIn, base)
        assert seen == [("init", False), ("sample", os.path.join("data", "test"), 25, {"draw_bbox": True})]
        del seen[:]
        main_base.run("mnist", cfg, cfg_from_file, StandIn, base + ["--synthetic", "12"])          # --synthetic alone still samples
        assert [s[0] for s in seen] == ["init", "sample"]
        del seen[:]
        main_base.run("mnist", cfg, cfg_from_file, StandIn, base + ["--spectrum", "--object_accuracy"])
        assert seen == [("score", ["object_accuracy", "spectrum"])]
        del seen[:]
        on = tmp_path / "on.yml"
        on.write_text(COMMON + "NET_G: ''\nTRAIN: {FLAG: True, BATCH_SIZE: 4}\n")
        main_base.run("mnist", cfg, cfg_from_file, StandIn, ["--cfg", str(on), "--manualSeed", "3", "--output_dir", str(tmp_path / "o"),
                                                            "--synthetic", "8", "--swd"])     # training ignores the score flags
        assert seen == [("init", False), ("train", 8, 4, 1)]
    finally:
        _restore(cfg)
