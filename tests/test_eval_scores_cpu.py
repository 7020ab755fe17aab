"""The table of checkpoint scores (attngan/evaluate.SCORES) and what main.py derives from it: the order a shared pass finishes the
scores in, every row's flag, its exclusions, the boxes the evaluation dataset leaves out, and that the table, main.py's keyword map
and the methods' signatures name the same things.  No GPU: main() runs against a stand-in trainer."""
import inspect

import pytest

from eval_setup import TINY
from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import main as entry  # noqa: E402
from mogan_amd.attngan.evaluate import SCORES, CheckpointEvaluation, fan_out  # noqa: E402

ORDER = ["scene_fid", "swd", "msssim", "spectrum", "fid", "kid", "prdc", "memorisation"]
TAKES = {"scene_fid": "objects", "swd": "images", "msssim": "images", "spectrum": "images", "fid": "codes", "kid": "codes",
         "prdc": "codes", "memorisation": "codes"}


def test_the_table_is_in_finishing_order_and_says_what_each_score_takes():
    assert list(SCORES) == ORDER and [row.name for row in SCORES.values()] == ORDER
    assert {name: row.takes for name, row in SCORES.items()} == TAKES
    assert {name: row.factory for name, row in SCORES.items() if row.factory} == {
        "scene_fid": "scene_fid_objects", "swd": "swd_images", "msssim": "msssim_images", "spectrum": "spectrum_images",
        "memorisation": "thumbnails"}
    assert CheckpointEvaluation().thumbnails(show=0) is None and CheckpointEvaluation().thumbnails(show=2) is not None


def test_the_table_main_and_the_methods_name_the_same_keywords():
    asked = entry.asked_scores(entry.parse_args(["--" + name for name in ORDER]))
    assert list(asked) == ORDER
    for name, row in SCORES.items():
        method = inspect.signature(getattr(CheckpointEvaluation, name)).parameters
        assert list(method)[:4] == ["self", "split_dir", "num_samples", "seed"] and row.takes in method, name
        assert set(asked[name]) <= set(method) and set(row.params) <= set(asked[name]), name
        if row.factory:
            factory = inspect.signature(getattr(CheckpointEvaluation, row.factory)).parameters
            assert list(factory) == ["self", "num_samples", "seed"] + list(row.params), name
    assert entry.asked_scores(entry.parse_args([])) == {}


@pytest.mark.parametrize("name", ORDER)
def test_every_rows_flag_parses_and_is_refused_beside_sampling_and_r_precision(name, capsys):
    args = entry.parse_args(["--" + name])
    assert getattr(args, name) is True and list(entry.asked_scores(args)) == [name]
    for other in ("--sampling", "--r_precision"):
        with pytest.raises(SystemExit):
            entry.parse_args(["--" + name, other])
        assert "--%s cannot be combined with --sampling or --r_precision" % name in capsys.readouterr().err


def test_every_rows_flag_switches_the_boxes_off_and_reaches_run_scores(tmp_path, monkeypatch, capsys):
    from mogan_amd.attngan.miscc.config import cfg
    ev = tmp_path / "eval.yml"
    ev.write_text(TINY + "B_VALIDATION: True\nTRAIN: {FLAG: False, BATCH_SIZE: 4, NET_G: '%s', NET_E: ''}\n" % (tmp_path / "none.pth"))
    seen = {}

    class StandIn:
        def __init__(self, output_dir, loader, *rest, **kw):
            seen.update(with_bbox=loader.dataset.eval, asked=None)

        def run_scores(self, split_dir, asked, seed):
            seen.update(asked=asked, split_dir=split_dir, seed=seed)

        def sample(self, split_dir, num_samples, draw_bbox):
            seen.update(sampled=True)
    monkeypatch.setattr(entry, "trainer", StandIn)
    keep = cfg.B_VALIDATION
    try:
        base = ["--cfg", str(ev), "--synthetic", "12", "--manualSeed", "7", "--output_dir", str(tmp_path)]
        entry.main(base)
        assert seen["with_bbox"] is True and seen["asked"] is None and seen["sampled"]      # no score: sample() and its boxes
        for name in ORDER:
            entry.main(base + ["--" + name])
            assert seen["with_bbox"] is False and list(seen["asked"]) == [name] and (seen["split_dir"], seen["seed"]) == ("test", 7)
        entry.main(base + ["--" + name for name in reversed(ORDER)])
        assert seen["with_bbox"] is False and list(seen["asked"]) == ORDER                   # any order of flags: the table's
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.FLAG, cfg.B_VALIDATION = '', True, keep
    capsys.readouterr()


def test_run_scores_refuses_what_the_table_does_not_hold_and_the_guard_runs_once(capsys):
    ev = CheckpointEvaluation()
    for asked in ({}, {"fid": {}, "inception_score": {}}):
        with pytest.raises(ValueError, match="run_scores"):
            ev.run_scores("test", asked)
    capsys.readouterr()
    assert ev.run_scores("test", {"fid": {}, "swd": {}}) is None and ev.run_scores("test", {"kid": {}}) == {"kid": None}
    assert capsys.readouterr().out.count("Error: the path for model NET_G is not found!") == 2   # once per call


def test_fan_out_composes_sinks_in_order():
    got = []
    assert fan_out([]) is None
    fan_out([got.append])("alone")
    assert got.pop() == "alone"
    fan_out([lambda *a: got.append(("a",) + a), lambda *a: got.append(("b",) + a)])(1, 2)
    assert got == [("a", 1, 2), ("b", 1, 2)]
