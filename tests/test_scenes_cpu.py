"""The rules of scene files (attngan/scenes.py) without a GPU: every rule and every ValueError with its scene and
field, dropped words, truncation, the class-name file, sweep geometry, the per-scene seed, and main.py's flags with their exclusions."""
import copy
import json

import numpy as np
import pytest

from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import scenes as SC  # noqa: E402

VOCAB = {"<end>": 0, "a": 1, "red": 2, "bus": 3, "on": 4, "the": 5, "street": 6, "caf": 7, "dog": 8, "and": 9, "cat": 10}
GOOD = {"name": "bus_1", "caption": "A red bus on the street",
        "objects": [{"label": 5, "box": [0.1, 0.2, 0.5, 0.4]}, {"label": 0, "box": [0.6, 0.6, 0.4, 0.4]}],
        "samples": 2, "sweep": {"object": 0, "to": [0.5, 0.6], "steps": 3}}


def check(scene, **kw):
    args = dict(wordtoix=VOCAB, words_num=6, n_classes=81, samples=4, classes=None, seed=100)
    args.update(kw)
    return SC.check_file({"scenes": [scene]}, **args)[0]


def edited(**kw):
    s = copy.deepcopy(GOOD)
    for k, v in kw.items():
        if v is None:
            s.pop(k)
        else:
            s[k] = v
    return s


def test_a_good_scene():
    s = check(GOOD)
    assert (s.name, s.words, s.tokens, s.dropped, s.truncated) == ("bus_1", ["a", "red", "bus", "on", "the", "street"], [1, 2, 3, 4, 5, 6], [], False)
    assert s.boxes.dtype == np.float32 and s.boxes.shape == (3, 4) and s.labels.tolist() == [5, 0, -1] and s.n_objects == 2
    assert (s.boxes[:2] == np.array([[0.1, 0.2, 0.5, 0.4], [0.6, 0.6, 0.4, 0.4]], dtype=np.float32)).all() and (s.boxes[2] == -1).all()
    assert s.samples == 2 and s.sweep == {"object": 0, "to": [0.5, 0.6], "steps": 3} and s.index == 0
    assert check(edited(samples=None, sweep=None)).samples == 4 and check(edited(samples=None), samples=9).samples == 9
    assert check(edited(sweep=None)).sweep is None


def test_the_caption_rules():
    s = check(edited(caption="A RED, red  bus!  Zebra on the café-street and a dog and a cat"))
    # lower-cased, \w+ tokens, "café" reduced to its ASCII characters "caf", "zebra" unknown, cut to six words
    assert s.words == ["a", "red", "red", "bus", "on", "the"] and s.dropped == ["zebra"] and s.truncated
    assert SC.tokenize("Café-Street, x_1 é 7up") == ["caf", "street", "x_1", "7up"]
    assert check(edited(caption="a bus")).truncated is False
    assert check(edited(caption="end a")).words == ["a"]                                    # the terminator's index 0 is no word
    for bad in ("zebra giraffe", "", "!!! ...", "é"):
        with pytest.raises(ValueError, match=r"scene 'bus_1', caption"):
            check(edited(caption=bad))
    with pytest.raises(ValueError, match=r"scene 'bus_1', caption"):
        check(edited(caption=["a", "bus"]))


BAD_BOXES = [[0.1, 0.2, 0.0, 0.4], [0.1, 0.2, 0.5, -0.1], [-0.01, 0.2, 0.5, 0.4], [0.1, -0.2, 0.5, 0.4], [0.6, 0.2, 0.5, 0.4], [0.1, 0.7, 0.5, 0.4],
             [0.1, 0.2, 0.5], [0.1, 0.2, 0.5, "0.4"], [0.1, 0.2, 0.5, float("nan")], [0.1, 0.2, float("inf"), 0.4], "box", [0.1, 0.2, 0.5, True]]


@pytest.mark.parametrize("box", BAD_BOXES, ids=str)
def test_a_bad_box_names_the_scene_and_the_object(box):
    objects = copy.deepcopy(GOOD["objects"])
    objects[1]["box"] = box
    with pytest.raises(ValueError, match=r"scene 'bus_1', objects\[1\]\.box"):
        check(edited(objects=objects, sweep=None))


def test_boxes_on_the_images_edge_are_legal_and_drawn_inside_it():
    s = check(edited(objects=[{"label": 1, "box": [0.0, 0.0, 1.0, 1.0]}, {"label": 2, "box": [0.5, 0.5, 0.5, 0.5]}], sweep=None))
    for x, y, w, h in s.pixel_boxes(256):
        assert 0 <= x and 0 <= y and x + w <= 255 and y + h <= 255
    assert (s.boxes[0] == np.array([0, 0, 1, 1], dtype=np.float32)).all()                   # the generator sees the box as written


def test_the_object_list_and_the_labels():
    box = [0.1, 0.1, 0.2, 0.2]
    for objects in ([], [{"label": 1, "box": box}] * 4, "objects", None):
        with pytest.raises(ValueError, match=r"scene 'bus_1', objects:"):
            check(edited(objects=objects, sweep=None))
    for obj in ({"label": 1}, {"box": box}, {"label": 1, "box": box, "colour": "red"}, [1, box]):
        with pytest.raises(ValueError, match=r"scene 'bus_1', objects\[0\]:"):
            check(edited(objects=[obj], sweep=None))
    for label in (-1, 80, 81, 1.0, True, None, [1]):
        with pytest.raises(ValueError, match=r"scene 'bus_1', objects\[0\]\.label"):
            check(edited(objects=[{"label": label, "box": box}], sweep=None))
    assert check(edited(objects=[{"label": 79, "box": box}], sweep=None)).labels.tolist() == [79, -1, -1]
    assert check(edited(objects=[{"label": 1, "box": box}] * 3, sweep=None)).n_objects == 3
    with pytest.raises(ValueError, match=r"scene 'bus_1', objects\[0\]\.label: the name 'bus' needs a class-name file"):
        check(edited(objects=[{"label": "bus", "box": box}], sweep=None))
    names = ["person", "bicycle", "bus"]
    assert check(edited(objects=[{"label": "bus", "box": box}, {"label": 1, "box": box}], sweep=None), classes=names).labels.tolist() == [2, 1, -1]
    with pytest.raises(ValueError, match=r"scene 'bus_1', objects\[0\]\.label: 'tram' is not a name"):
        check(edited(objects=[{"label": "tram", "box": box}], sweep=None), classes=names)


def test_the_class_name_file(tmp_path):
    f = tmp_path / "classes.txt"
    f.write_text("person\nbicycle \n bus\n")
    assert SC.read_classes(str(f)) == ["person", "bicycle", "bus"]
    for text in ("", "person\n\nbus\n", "bus\nbus\n"):
        f.write_text(text)
        with pytest.raises(ValueError, match="class file"):
            SC.read_classes(str(f))


def test_names_samples_and_unknown_fields():
    for name in ("", ".hidden", "a/b", "..", "a b", "ä", 7, None, "x" * 101, "a\\b"):
        with pytest.raises(ValueError, match=r"scene #0, name"):
            check(edited(name=name))
    assert check(edited(name="A-1.b_c")).name == "A-1.b_c"
    with pytest.raises(ValueError, match=r"scene 'bus_1', name: used twice"):
        SC.check_file({"scenes": [GOOD, GOOD]}, VOCAB, 6, 81)
    for n in (0, 65, -1, 2.0, "2", True):
        with pytest.raises(ValueError, match=r"scene 'bus_1', samples"):
            check(edited(samples=n))
    assert check(edited(samples=64)).samples == 64 and check(edited(samples=1)).samples == 1
    with pytest.raises(ValueError, match=r"scene 'bus_1', colour: unknown field"):
        check(dict(GOOD, colour="red"))
    with pytest.raises(ValueError, match=r"scene #1, scene"):
        SC.check_file({"scenes": [GOOD, "scene"]}, VOCAB, 6, 81)
    for doc in ({}, {"scenes": []}, {"scenes": GOOD}, [GOOD], {"scenes": [GOOD], "more": 1}):
        with pytest.raises(ValueError, match="scene file"):
            SC.check_file(doc, VOCAB, 6, 81)
    with pytest.raises(ValueError, match="scene file"):
        SC.check_file({"scenes": [GOOD]}, VOCAB, 6, 81, samples=0)


def test_the_sweeps_geometry():
    for field, sweep in (("sweep", {"object": 0, "to": [0.5, 0.6]}), ("sweep", [0, [0.5, 0.6], 3]), ("sweep", {"object": 0, "to": [0.5, 0.6], "steps": 3, "x": 1}),
                         ("sweep.object", {"object": 2, "to": [0.5, 0.6], "steps": 3}), ("sweep.object", {"object": -1, "to": [0.5, 0.6], "steps": 3}),
                         ("sweep.object", {"object": 0.0, "to": [0.5, 0.6], "steps": 3}), ("sweep.steps", {"object": 0, "to": [0.5, 0.6], "steps": 1}),
                         ("sweep.steps", {"object": 0, "to": [0.5, 0.6], "steps": 33}), ("sweep.steps", {"object": 0, "to": [0.5, 0.6], "steps": 3.0}),
                         ("sweep.to", {"object": 0, "to": [0.51, 0.6], "steps": 3}), ("sweep.to", {"object": 0, "to": [0.5, 0.61], "steps": 3}),
                         ("sweep.to", {"object": 0, "to": [-0.1, 0.6], "steps": 3}), ("sweep.to", {"object": 0, "to": [0.5], "steps": 3}),
                         ("sweep.to", {"object": 0, "to": [0.5, float("nan")], "steps": 3}), ("sweep.to", {"object": 0, "to": "right", "steps": 3})):
        with pytest.raises(ValueError, match=r"scene 'bus_1', %s:" % field.replace(".", r"\.")):
            check(edited(sweep=sweep))
    s = check(GOOD)
    path = s.sweep_boxes()
    assert path.dtype == np.float32 and path.shape == (3, 4)
    assert (path[0] == s.boxes[0]).all()                                                    # step 0: the box's own bits
    assert np.allclose(path[1], [0.3, 0.4, 0.5, 0.4]) and np.allclose(path[2], [0.5, 0.6, 0.5, 0.4]) and (path[:, 2:] == s.boxes[0, 2:]).all()
    assert check(edited(sweep={"object": 1, "to": [0.0, 0.0], "steps": 32})).sweep_boxes().shape == (32, 4)


def test_every_scene_has_a_seed_of_its_own_that_depends_on_its_position_only():
    doc = {"scenes": [edited(name="n%d" % i, sweep=None) for i in range(3)]}
    seeds = [s.seed for s in SC.check_file(doc, VOCAB, 6, 81, seed=100)]
    assert seeds == [int(np.random.SeedSequence([100, i]).generate_state(1)[0]) for i in range(3)] and len(set(seeds)) == 3
    assert [s.seed for s in SC.check_file(doc, VOCAB, 6, 81, seed=101)] != seeds
    assert SC.scene_seed(100, 2) == seeds[2] and all(isinstance(v, int) and 0 <= v < 2 ** 32 for v in seeds)


def test_load_reads_a_file_and_names_a_file_that_is_not_json(tmp_path):
    f = tmp_path / "scenes.json"
    f.write_text(json.dumps({"scenes": [GOOD]}))
    assert SC.load(str(f), VOCAB, 6, 81)[0].name == "bus_1"
    f.write_text("{scenes: ")
    with pytest.raises(ValueError, match="is not JSON"):
        SC.load(str(f), VOCAB, 6, 81)


def test_the_vocabulary_of_a_dataset_without_wordtoix():
    from mogan_amd.attngan.datasets import SyntheticTextDataset
    v = SC.vocabulary(SyntheticTextDataset(4, n_words=50))
    assert v["w1"] == 1 and v["w49"] == 49 and v["<end>"] == 0 and len(v) == 50
    s = SC.check_file({"scenes": [edited(caption="w3 w49 w50 end w1")]}, v, 6, 81)[0]
    assert s.tokens == [3, 49, 1] and s.dropped == ["w50", "end"]


def test_main_refuses_the_scene_mode_beside_every_other_mode(capsys):
    from mogan_amd.attngan import main as entry
    from mogan_amd.attngan.evaluate import SCORES
    for other in ["sampling", "r_precision", "layout_shift", "inception_score"] + list(SCORES):
        with pytest.raises(SystemExit):
            entry.parse_args(["--scenes", "s.json", "--%s" % other])
        assert "cannot be combined" in capsys.readouterr().err
    for flags in (["--scene_samples", "0"], ["--scene_samples", "65"], ["--scene_topk", "0"], ["--scene_topk", "9"]):
        with pytest.raises(SystemExit):
            entry.parse_args(["--scenes", "s.json"] + flags)
    args = entry.parse_args(["--scenes", "s.json"])
    assert (args.scenes, args.scene_samples, args.scene_topk, args.scene_no_attention, args.scene_classes) == ("s.json", 4, 5, False, None)
    args = entry.parse_args(["--scenes", "s.json", "--scene_samples", "64", "--scene_topk", "8", "--scene_no_attention", "--scene_classes", "c.txt"])
    assert (args.scene_samples, args.scene_topk, args.scene_no_attention, args.scene_classes) == (64, 8, True, "c.txt")


def test_a_bad_file_is_refused_before_any_checkpoint_is_loaded(tmp_path, monkeypatch):
    import torch
    from eval_setup import tiny_checkpoint
    from mogan_amd.attngan.datasets import SyntheticTextDataset
    from mogan_amd.attngan.evaluate import CheckpointEvaluation
    cfg, ev, ckpt = tiny_checkpoint(tmp_path)
    try:
        def no_load(self, *a, **k):
            raise AssertionError("a checkpoint was loaded before the scene file was checked")
        monkeypatch.setattr(CheckpointEvaluation, "_load_seeded", no_load)
        f = tmp_path / "bad.json"
        f.write_text(json.dumps({"scenes": [edited(caption="w1 w2", objects=[{"label": 1, "box": [0.5, 0.5, 0.6, 0.2]}], sweep=None)]}))
        algo = CheckpointEvaluation()                                 # what the mode needs of a trainer, without a device
        ds = SyntheticTextDataset(length=4, n_words=100, seed=7)
        algo.device, algo.data_loader, algo.n_words, algo.ixtoword = torch.device("cpu"), torch.utils.data.DataLoader(ds, batch_size=4), 100, ds.ixtoword
        with pytest.raises(ValueError, match=r"scene 'bus_1', objects\[0\]\.box"):
            algo.scenes(str(f), seed=7)
        f.write_text(json.dumps({"scenes": [edited(caption="w1 w2", sweep=None)]}))
        with pytest.raises(ValueError, match="topk"):
            algo.scenes(str(f), seed=7, topk=9)
        cfg.TRAIN.NET_G = ''
        assert algo.scenes(str(f), seed=7) is None                                         # the guard comes first
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.FLAG = '', True
