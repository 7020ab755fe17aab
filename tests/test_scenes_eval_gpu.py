"""-m gpu: the scene mode end to end on eval_setup's tiny checkpoint, through attngan/main.py and directly: a
file of three scenes -- one, two and three objects, one with a sweep of three steps, one with a word the vocabulary does not hold."""
import glob
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from eval_setup import tiny_checkpoint
from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import attnsheet as AS  # noqa: E402
from mogan_amd.attngan.datasets import SyntheticTextDataset  # noqa: E402
from mogan_amd.attngan.miscc import vis  # noqa: E402
from mogan_amd.hip import ops  # noqa: E402

pytestmark = pytest.mark.gpu

SOLO = {"name": "solo", "caption": "W5 w9, w3 zebra w12 w7!", "samples": 2, "objects": [{"label": 3, "box": [0.25, 0.25, 0.5, 0.5]}]}
PAIR = {"name": "pair", "caption": "w1 w2 w3 w4 w5 w6 w7 w8", "samples": 2,
        "objects": [{"label": 7, "box": [0.05, 0.1, 0.4, 0.45]}, {"label": 11, "box": [0.5, 0.5, 0.5, 0.5]}],
        "sweep": {"object": 0, "to": [0.55, 0.1], "steps": 3}}
TRIO = {"name": "trio", "caption": "w40 w41 w42", "objects": [{"label": 0, "box": [0.0, 0.0, 0.3, 0.3]}, {"label": 79, "box": [0.35, 0.35, 0.3, 0.3]},
                                                              {"label": 5, "box": [0.7, 0.7, 0.3, 0.3]}]}
TOPK = 4


def _files(root):
    return {os.path.relpath(p, root): open(p, "rb").read() for p in sorted(glob.glob(root + "/**/*", recursive=True)) if os.path.isfile(p)}


def _size(data_or_path):
    with Image.open(data_or_path) as im:
        return im.size                                                                    # (width, height)


def test_the_mode_through_main_its_files_and_its_bytes(tmp_path, capsys):
    from mogan_amd.attngan import main as entry
    cfg, ev, ckpt = tiny_checkpoint(tmp_path)
    try:
        three = tmp_path / "three.json"
        three.write_text(json.dumps({"scenes": [SOLO, PAIR, TRIO]}))
        base = ["--cfg", str(ev), "--synthetic", "12", "--manualSeed", "7", "--output_dir", str(tmp_path), "--scene_samples", "3",
                "--scene_topk", str(TOPK)]
        root = os.path.join(ckpt[:-4], "scenes")
        entry.main(base + ["--scenes", str(three)])
        assert "Scenes (3 scenes, 7 images, attention sheets of the top %d words) -> %s" % (TOPK, root) in capsys.readouterr().out
        first = _files(root)
        want = {"scenes.json"}
        for sc, n, words in ((SOLO, 2, 5), (PAIR, 2, 6), (TRIO, 3, 3)):                     # zebra dropped; eight words cut to WORDS_NUM = 6
            K = min(TOPK, words)
            for k in range(n):
                for g, side in enumerate((64, 128, 256)):
                    assert _size("%s/%s/s%d_g%d.png" % (root, sc["name"], k, g)) == (side, side)
                for a in range(2):
                    assert _size("%s/%s/s%d_a%d.png" % (root, sc["name"], k, a)) == (K * 258, vis.FONT_MAX + 256)
                want |= {"%s/s%d_%s%d.png" % (sc["name"], k, c, i) for c, top in (("g", 3), ("a", 2)) for i in range(top)}
            assert _size("%s/%s/samples.png" % (root, sc["name"])) == (4 * 256, n * 256)
            want.add("%s/samples.png" % sc["name"])
        assert _size(root + "/pair/sweep.png") == (3 * 256, 256)
        assert set(first) == want | {"pair/sweep.png"}
        rec = json.loads(first["scenes.json"])
        assert set(rec) == {"scenes", "file", "topk", "attention", "seed", "NET_G", "NET_E", "note"} and (rec["seed"], rec["NET_G"], rec["topk"]) == (7, ckpt, TOPK)
        solo, pair, trio = rec["scenes"]
        assert (solo["words"], solo["tokens"], solo["dropped"], solo["truncated"]) == (["w5", "w9", "w3", "w12", "w7"], [5, 9, 3, 12, 7], ["zebra"], False)
        assert pair["truncated"] and pair["tokens"] == [1, 2, 3, 4, 5, 6] and pair["sweep"] == PAIR["sweep"] and trio["samples"] == 3
        assert [s["seed"] for s in rec["scenes"]] == [int(np.random.SeedSequence([7, i]).generate_state(1)[0]) for i in range(3)]
        assert solo["boxes_px"] == [[64, 64, 128, 128]] and trio["labels"] == [0, 79, 5] and len(trio["boxes_px"]) == 3
        assert [(s["sample"], s["stage"]) for s in pair["sheets"]] == [(0, 0), (0, 1), (1, 0), (1, 1)]
        for s in pair["sheets"]:
            assert len(s["words"]) == len(s["conf"]) == len(s["lo"]) == len(s["hi"]) == len(s["flag"]) == TOPK and set(s["flag"]) <= {0, 1}
            assert s["conf"] == sorted(s["conf"], reverse=True) and all(0 <= w < 6 for w in s["words"]) and len(set(s["words"])) == TOPK
        # the layout on black: white lines exactly at the drawn box, nothing else
        layout = np.array(Image.open(root + "/solo/samples.png"))[:256, :256]
        assert set(np.unique(layout)) == {0, 255} and layout[64, 64:192].min() == 255 and layout[100, 100].max() == 0 and layout[63].max() == 0
        # a second run: the same bytes in every file
        for p in first:
            os.remove(os.path.join(root, p))
        entry.main(base + ["--scenes", str(three)])
        assert _files(root) == first
        # a scene alone in a file has the bytes it has among the others (the first: a scene's seed is its position's)
        for p in first:
            os.remove(os.path.join(root, p))
        alone = tmp_path / "alone.json"
        alone.write_text(json.dumps({"scenes": [SOLO]}))
        entry.main(base + ["--scenes", str(alone)])
        got = _files(root)
        assert {p: b for p, b in got.items() if p != "scenes.json"} == {p: b for p, b in first.items() if p.startswith("solo/")}
        assert json.loads(got["scenes.json"])["scenes"] == [solo]
        # without the sheets: no _a*.png, the same _g*.png
        for p in got:
            os.remove(os.path.join(root, p))
        entry.main(base + ["--scenes", str(three), "--scene_no_attention"])
        bare = _files(root)
        assert set(bare) == {p for p in first if "_a" not in p}
        assert all(bare[p] == first[p] for p in bare if p != "scenes.json")
        assert all(s["sheets"] == [] for s in json.loads(bare["scenes.json"])["scenes"])
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.FLAG = '', True


def test_the_sweep_starts_at_sample_zero_and_the_sheets_words_are_the_ops_order(tmp_path):
    from mogan_amd.attngan.trainer import condGANTrainer
    cfg, ev, ckpt = tiny_checkpoint(tmp_path)
    try:
        three = tmp_path / "three.json"
        three.write_text(json.dumps({"scenes": [SOLO, PAIR, TRIO]}))
        ds = SyntheticTextDataset(12, seed=7, eval=False)
        dl = torch.utils.data.DataLoader(ds, batch_size=cfg.TRAIN.BATCH_SIZE, drop_last=True, shuffle=True, num_workers=0)
        algo = condGANTrainer(str(tmp_path), dl, ds.n_words, ds.ixtoword, '', distributed=False)
        seen = {}

        def sink(sc, fake_imgs, att_maps, swept):
            seen[sc.name] = ([t.clone() for t in fake_imgs], [t.clone() for t in att_maps], None if swept is None else swept.clone())
        out = algo.scenes(str(three), seed=7, samples=3, topk=TOPK, image_sink=sink)
        assert set(seen) == {"solo", "pair", "trio"} and seen["solo"][2] is None and seen["trio"][2] is None
        imgs, atts, swept = seen["pair"]
        assert tuple(swept.shape) == (3, 3, 256, 256) and tuple(imgs[2].shape) == (2, 3, 256, 256)
        assert torch.equal(swept[0], imgs[2][0])                                           # step 0 is sample 0, bit for bit
        assert not torch.equal(swept[2], imgs[2][0]) and not torch.equal(swept[1], swept[2])
        root = os.path.join(ckpt[:-4], "scenes")
        png = np.array(Image.open(root + "/pair/s0_g2.png"))
        assert (png == imgs[2][0].add(1.0).mul(127.5).clamp(0, 255).byte().permute(1, 2, 0).cpu().numpy()).all()
        for entry, name in zip(out["scenes"], ("solo", "pair", "trio")):
            imgs, atts, _ = seen[name]
            n, T = atts[0].shape[:2]
            assert T == len(entry["tokens"]) and [tuple(a.shape[2:]) for a in atts] == [(64, 64), (128, 128)]
            lens = torch.full((n,), T, dtype=torch.int32)
            for s in entry["sheets"]:
                conf = ops.attn_conf(atts[s["stage"]].contiguous(), lens).cpu().numpy()[s["sample"]]
                order = np.argsort(conf)[::-1][:TOPK]
                assert s["words"] == [int(k) for k in order] and s["conf"] == [float(conf[k]) for k in order]
                want = AS.conf_numpy(atts[s["stage"]].cpu().numpy(), lens.numpy())[s["sample"]]
                att = atts[s["stage"]].shape[-1]
                assert (np.abs(conf - want) <= (att * att + 4) * 2.0 ** -52 * want).all()       # tests/attnsheet_cases.py derives it
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.FLAG = '', True
