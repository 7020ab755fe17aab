"""The host side of the layout-shift score (attngan/layoutshift.py), no GPU: the pixel rectangle at its clamps,
the edit's draw -- the same for image i however the pass is cut into batches, never outside the image --, what is left out and
counted, the numpy oracle's own contracts on the shared cases, the figures on hand-made pairs, and the flags of both entry points."""
import numpy as np
import pytest
import torch

import layout_cases as LC
from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import layoutshift as LS  # noqa: E402

ABSENT = [-1.0, -1.0, -1.0, -1.0]


# ------------------------------------------------------------------------------------------------- the rectangle
def test_pixel_rect_rounds_to_the_nearest_pixel_and_clamps():
    assert LS.pixel_rect([0.25, 0.5, 0.25, 0.125], 16) == (4, 8, 8, 10)
    assert LS.pixel_rect([0.0, 0.0, 1.0, 1.0], 256) == (0, 0, 256, 256)
    assert LS.pixel_rect([0.26, 0.26, 0.01, 0.01], 16) == (4, 4, 5, 5)             # thinner than a pixel: one pixel
    assert LS.pixel_rect([0.999, 0.999, 0.2, 0.2], 16) == (15, 15, 16, 16)         # x0 clamped to S - 1, x1 to S
    assert LS.pixel_rect([-0.3, -0.01, 0.2, 0.5], 16) == (0, 0, 1, 8)              # x0 clamped to 0, x1 to x0 + 1
    assert LS.pixel_rect([0.5, 0.5, 0.9, 0.9], 20) == (10, 10, 20, 20)
    # floor(v + 1/2), not round-half-even: 2.5 -> 3, 3.5 -> 4
    assert LS.pixel_rect([2.5 / 16, 3.5 / 16, 4.0 / 16, 4.0 / 16], 16) == (3, 4, 7, 8)
    # fp64 arithmetic on the fp32 values: the fp32 nearest to 0.1 is above 0.1
    x = np.float32(0.1)
    assert LS.pixel_rect([x, x, x, x], 5) == (1, 1, 2, 2) and float(x) * 5 + 0.5 > 1.0


def test_feasible_offsets_are_dy_major_inside_the_image_and_far_enough():
    got = LS.feasible_offsets((1, 1, 3, 3), 4, 1)
    assert got == [(-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)]
    assert LS.feasible_offsets((0, 0, 4, 4), 4, 1) == []
    assert LS.feasible_offsets((0, 2, 4, 3), 4, 2) == [(0, -2)]
    for dx, dy in LS.feasible_offsets((3, 5, 9, 8), 20, 4):
        assert max(abs(dx), abs(dy)) >= 4 and 3 + dx >= 0 and 9 + dx <= 20 and 5 + dy >= 0 and 8 + dy <= 20


# ------------------------------------------------------------------------------------------------- the draw
def _boxes(n, G=3, seed=5):
    rng = np.random.RandomState(seed)
    b = np.full((n, G, 4), -1.0, dtype=np.float32)
    for i in range(n):
        for g in range(rng.randint(0, G + 1)):
            x, y = rng.uniform(0.0, 0.6, 2)
            b[i, g] = (x, y, rng.uniform(0.05, 0.4), rng.uniform(0.05, 0.4))
    return b


def test_the_edit_of_image_i_does_not_depend_on_the_batch_split_and_never_leaves_the_image():
    boxes = _boxes(23)
    S = 64

    def run(step, rows=23):
        acc = LS.ShiftResponse(S, 3, rows, None, 1, 11, "cpu", sums=LS.sums_numpy)
        out = {}
        for at in range(0, rows, step):
            batch = torch.from_numpy(boxes[at:at + step].copy())
            take = min(step, rows - at)
            t = acc.edits(batch, take)
            z = torch.zeros((batch.shape[0], 3, S, S))
            acc.add(z, z, t)
            for k, j in enumerate(t["row"].tolist()):
                out[at + j] = (int(t["slot"][k]), t["edit"][k].tolist(), t["moved"][k].numpy().tobytes(), t["others"][k].tolist())
                # every other value of the batch's boxes keeps its bits
                keep = batch.clone()
                keep[j, int(t["slot"][k])] = t["moved"][k]
                assert torch.equal(t["boxes"][j].view(torch.int32), keep[j].view(torch.int32))
        return out, acc
    whole, acc = run(23)
    for step in (1, 4, 7):
        assert run(step)[0] == whole
    short = run(5, rows=12)[0]                                       # ... nor on num_samples
    assert short == {i: v for i, v in whole.items() if i < 12}
    assert len(whole) + acc.no_objects + acc.immovable == 23 and acc.n == len(whole) and acc.n_images == 23
    assert acc.no_objects == int((boxes[:, :, 2] <= 0).all(axis=1).sum()) > 0
    for i, (slot, e, moved, others) in whole.items():
        x0, y0, x1, y1, dx, dy = e
        assert (x0, y0, x1, y1) == LS.pixel_rect(boxes[i, slot], S) and boxes[i, slot, 2] > 0
        assert max(abs(dx), abs(dy)) >= S // 8 and x0 + dx >= 0 and y0 + dy >= 0 and x1 + dx <= S and y1 + dy <= S
        single = LS.draw_edit(boxes[i], S, 11, i)
        assert (single["slot"], list(single["rect"]) + list(single["offset"])) == (slot, e) and single["box"].tobytes() == moved
        x, y, w, h = boxes[i, slot]
        want = np.array([np.float32(float(x) + dx / 64.0), np.float32(float(y) + dy / 64.0), w, h], dtype=np.float32)
        assert want.tobytes() == moved
    assert len({v[0] for v in whole.values()}) > 1 and len({tuple(v[1][4:]) for v in whole.values()}) > 3
    other_seed = LS.draw_edit(boxes[next(iter(whole))], S, 12, next(iter(whole)))
    assert isinstance(other_seed, dict)


def test_no_objects_and_immovable_are_left_out_and_counted():
    S = 16
    boxes = torch.tensor([[ABSENT, ABSENT],                               # no object
                          [[0.0, 0.0, 1.0, 1.0], ABSENT],                 # the whole image: nowhere to go
                          [[0.25, 0.25, 0.25, 0.25], ABSENT],             # movable
                          [[0.1, 0.1, 0.01, 0.5], ABSENT],                # thinner than min_side = 2 pixels: no object
                          [[0.0, 0.2, 1.0, 0.7], ABSENT]],                # full width, rows 3..13: 3 rows of room at the most
                         dtype=torch.float32)
    acc = LS.ShiftResponse(S, 1, 5, 4, 2, 3, "cpu", sums=LS.sums_numpy)
    t = acc.edits(boxes, 5)
    assert t["row"].tolist() == [2] and (t["no_objects"], t["immovable"]) == (2, 2)
    z = torch.zeros((5, 1, S, S))
    acc.add(z, z, t)
    assert (acc.n, acc.n_images, acc.no_objects, acc.immovable) == (1, 5, 2, 2)
    out = acc.result()
    assert (out["n_pairs"], out["n_images"], out["no_objects"], out["immovable"], out["min_shift"], out["min_side"]) == (1, 5, 2, 2, 4, 2.0)
    assert LS.draw_edit(boxes[0].numpy(), S, 3, 0) == "no_objects" and LS.draw_edit(boxes[1].numpy(), S, 3, 1) == "immovable"
    with pytest.raises(ValueError):
        acc.edits(boxes, 1)                                              # the accumulator is full
    with pytest.raises(ValueError):
        LS.ShiftResponse(S, 1, 5, 0, 1, 3, "cpu")                        # min_shift 0 would allow the offset (0, 0)
    empty = LS.ShiftResponse(S, 1, 5, 4, 1, 3, "cpu", sums=LS.sums_numpy)
    t = empty.edits(boxes[:2], 2)
    empty.add(z[:2], z[:2], t)
    with pytest.raises(ValueError):
        empty.result()


def test_a_table_is_scored_where_it_was_made():
    acc = LS.ShiftResponse(16, 1, 8, 2, 1, 3, "cpu", sums=LS.sums_numpy)
    boxes = torch.tensor([[[0.25, 0.25, 0.25, 0.25]]], dtype=torch.float32)
    z = torch.zeros((1, 1, 16, 16))
    t = acc.edits(boxes, 1)
    acc.add(z, z, t)
    with pytest.raises(ValueError):
        acc.add(z, z, t)                                                 # made at image 0, the accumulator stands at 1
    with pytest.raises(ValueError):
        acc.add(z.double(), z.double(), acc.edits(boxes, 1))


# ------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("key", LC.CASES, ids=str)
def test_the_oracles_own_contracts(key):
    a, b, edit, others = LC.case(key)
    P, C, S, G = key
    sums, counts, bound = LC.expected(key)
    assert sums.shape == (P, 7) and counts.shape == (P, 5) and (counts.sum(axis=1) == S * S).all() and (sums >= 0).all()
    for p in range(P):
        cls = LS.classes_numpy(S, edit[p], others[p])
        x0, y0, x1, y1, dx, dy = edit[p]
        assert (cls[y0:y1, x0:x1] % 2 == 0).all() and (cls[y0:y1, x0:x1] <= 2).all()           # the old rectangle: classes 0 and 2
        assert counts[p, 0] + counts[p, 2] == (x1 - x0) * (y1 - y0) == counts[p, 1] + counts[p, 2]
        d2 = ((a[p].astype(np.float64) - b[p].astype(np.float64)) ** 2).sum(axis=0)
        assert abs(sums[p, :5].sum() - d2.sum()) <= 1e-12 * d2.sum()
    same, _ = LS.sums_numpy(a, a, edit, others)
    assert (same[:, :5] == 0).all() and (same[:, 5] == same[:, 6]).all()
    back, _ = LS.sums_numpy(b, a, edit, others)
    assert (back[:, :5] == sums[:, :5]).all()
    still = edit.copy()
    still[:, 4:] = 0
    assert (LS.sums_numpy(a, b, still, others)[0][:, 6] == 0).all()


def test_the_hand_made_case_covers_what_it_claims():
    edit, others = LC.tables((3, 3, 16, 2))
    sums, counts, _ = LC.expected((3, 3, 16, 2))
    rects = [tuple(e[:4]) for e in edit] + [(e[0] + e[4], e[1] + e[5], e[2] + e[4], e[3] + e[5]) for e in edit]
    assert {0} <= {r[0] for r in rects} and {0} <= {r[1] for r in rects} and {16} <= {r[2] for r in rects} and {16} <= {r[3] for r in rects}
    assert counts[0, 2] > 0 and counts[1, 2] == 0 and counts[2, 2] == 0           # old and new overlap in pair 0 only
    assert counts[2, 0] == 1 and edit[1, 2] - edit[1, 0] == 16 and edit[1, 4] == 0
    assert (counts[:, 3] > 0).all()
    cls = LS.classes_numpy(16, edit[0], others[0])
    assert (cls[1:4, 2:5] != 3).all() and cls[8, 8] == 3                          # an overlapping object yields to the rectangles


def test_a_row_that_should_never_be_sent_gets_zeros():
    a, b, edit, others = LC.case((3, 3, 16, 2))
    bad = edit.copy()
    bad[1] = [4, 4, 4, 8, 1, 1]                                                   # empty
    sums, counts = LS.sums_numpy(a, b, bad, others)
    want = LC.expected((3, 3, 16, 2))
    assert (sums[1] == 0).all() and (counts[1] == 0).all()
    assert (sums[[0, 2]] == want[0][[0, 2]]).all() and (counts[[0, 2]] == want[1][[0, 2]]).all()


# ------------------------------------------------------------------------------------------------- the figures
def _ground(S, C, seed=1):
    rng = np.random.RandomState(seed)
    return rng.uniform(-0.9, 0.9, (C, S, S)).astype(np.float32)


def _painted(S, C, rect, colour=0.5):
    img = _ground(S, C)
    img[:, rect[1]:rect[3], rect[0]:rect[2]] = colour
    return img


def test_figures_on_hand_made_pairs():
    S, C = 32, 3
    edit = np.array([[4, 6, 12, 16, 10, 7]] * 4, dtype=np.int32)
    old, new = (4, 6, 12, 16), (14, 13, 22, 23)
    a = np.stack([_painted(S, C, old),                         # 0: the square travels with its box
                  _painted(S, C, old),                         # 1: B = A: the edit is ignored
                  np.full((C, S, S), 0.25, dtype=np.float32),  # 2: a flat image that stays flat
                  _painted(S, C, old)])                        # 3: the square travels and the whole background changes too
    b = np.stack([_painted(S, C, new), a[1].copy(), a[2].copy(), -_painted(S, C, new)])
    b[3][:, 13:23, 14:22] = 0.5
    sums, counts = LS.sums_numpy(a, b, edit, None)
    info = [{"image": 10 + i, "key": "k%d" % i, "slot": 0, "rect": list(old), "offset": [10, 7]} for i in range(4)]
    out = LS.figures(sums, counts, S, C, show=3, info=info)
    assert (out["n_pairs"], out["flat"], out["unchanged"]) == (4, 1, 2)
    f = LS.follow_of(sums)
    assert f[0] == 1.0 and f[1] == 0.0 and np.isnan(f[2]) and f[3] == 1.0
    assert out["follow"] == {"mean": 2.0 / 3.0, "std": float(np.std([1.0, 0.0, 1.0])), "n": 3}
    loc = sums[[0, 3], :3].sum(axis=1) / sums[[0, 3], :5].sum(axis=1)
    assert loc[0] == 1.0 and 0 < loc[1] < 1
    assert out["locality"] == {"mean": float(loc.mean()), "std": float(loc.std()), "n": 2}
    share = (8 * 10 * 2) / float(S * S)
    assert out["area_share"] == {"mean": share, "std": 0.0, "n": 4}
    assert out["change"]["both"]["n"] == 0 and out["change"]["others"]["n"] == 0 and out["change"]["rest"]["n"] == 4
    assert out["change"]["old_only"]["mean"] == float((sums[:, 0] / (80 * C)).mean())
    assert out["spill_others"]["n"] == 0 and out["spill_background"]["n"] == 2
    want = (sums[[0, 3], 4] / counts[[0, 3], 4]) / (sums[[0, 3], :3].sum(axis=1) / 160.0)
    assert out["spill_background"]["mean"] == float(want.mean()) and want[0] == 0.0 and want[1] > 0
    # lowest follow first, the earlier pair first among equals, a flat pair never
    assert [(e["pair"], e["follow"], e["image"], e["key"]) for e in out["most_ignored"]] == [(1, 0.0, 11, "k1"), (0, 1.0, 10, "k0"),
                                                                                          (3, 1.0, 13, "k3")]
    assert out["most_ignored"][0]["rect"] == list(old) and out["most_ignored"][0]["offset"] == [10, 7]
    assert LS.figures(sums, counts, S, C, show=0)["most_ignored"] == []
    with pytest.raises(ValueError):
        LS.figures(-sums, counts, S, C)


def test_the_accumulator_gives_the_figures_of_its_pairs_and_keeps_the_most_ignored_images():
    key = (5, 3, 64, 2)
    a, b, edit, others = LC.case(key)
    sums, counts, _ = LC.expected(key)
    results = []
    for keep in (0, 2):
        acc = LS.ShiftResponse(64, 3, 5, 8, 1, 3, "cpu", sums=LS.sums_numpy, keep=keep)
        for at in (0, 2):
            n = min(3, 5 - at) if at else 2
            rows = torch.arange(n)
            table = {"row": rows, "slot": rows * 0, "edit": torch.from_numpy(edit[at:at + n]), "others": torch.from_numpy(others[at:at + n]),
                     "no_objects": 0, "immovable": 0, "first": at, "take": n}
            acc.add(torch.from_numpy(a[at:at + n]), torch.from_numpy(b[at:at + n]), table, keys=["k%d" % (at + j) for j in range(n)])
        results.append(acc.result(2))
        s, c = acc.raw()
        assert (s == sums).all() and (c == counts).all()
    want = LS.figures(sums, counts, 64, 3, 2, acc.info)
    assert {k: v for k, v in results[1].items() if k in want} == want == {k: v for k, v in results[0].items() if k in want}
    assert [v[1] for v in acc.kept] == [e["pair"] for e in want["most_ignored"]]
    for _, pair, ua, ub in acc.kept:
        assert ua.dtype == np.uint8 and ua.shape == (3, 64, 64)
        assert (ua == np.clip((a[pair] + 1.0) * 127.5, 0, 255).astype(np.uint8)).all()


def test_the_grid_is_one_row_of_three_tiles_per_kept_pair(tmp_path):
    from PIL import Image
    S = 16
    a = np.zeros((1, S, S), dtype=np.uint8)
    b = np.full((1, S, S), 40, dtype=np.uint8)
    info = [{"rect": [2, 3, 6, 8], "offset": [5, 4]}, {"rect": [0, 0, 16, 1], "offset": [0, 15]}]
    name = LS.layout_grid(str(tmp_path), [(0.5, 1, a, b), (0.1, 0, a, b)], info)
    sheet = np.asarray(Image.open(tmp_path / name))
    assert name == "layout_grid.png" and sheet.shape == (2 * S, 3 * S, 3)
    assert (sheet[3, 2:6, 0] == 255).all() and sheet[4, 3, 0] == 0                 # pair 0 first: the old box on A
    assert (sheet[7, S + 7:S + 11, 0] == 255).all() and sheet[8, S + 8, 0] == 40   # the new box on B
    assert (sheet[:S, 2 * S:] == 40).all()                                         # |A - B|
    assert (sheet[S, 0:S, 0] == 255).all() and (sheet[S + 15, S:2 * S, 0] == 255).all()


# ------------------------------------------------------------------------------------------------- the flags
def test_the_flags_of_the_attngan_entry_point():
    from mogan_amd.attngan import main as entry
    from mogan_amd.attngan.evaluate import SCORES
    args = entry.parse_args(["--layout_shift"])
    assert args.layout_shift and (args.ls_min_shift, args.ls_min_side, args.ls_show) == (None, 1, 16)
    assert entry.asked_scores(args) == {}
    args = entry.parse_args(["--layout_shift", "--ls_min_shift", "12", "--ls_min_side", "3.5", "--ls_show", "0"])
    assert (args.ls_min_shift, args.ls_min_side, args.ls_show) == (12, 3.5, 0)
    assert not entry.parse_args([]).layout_shift and "layout_shift" not in SCORES
    for other in ["--sampling", "--r_precision"] + ["--" + name for name in SCORES]:
        with pytest.raises(SystemExit):
            entry.parse_args(["--layout_shift", other])
    for bad in (["--ls_min_shift", "0"], ["--ls_show", "-1"], ["--ls_min_side", "-1"], ["--ls_min_side", "nan"], ["--ls_min_side", "inf"]):
        with pytest.raises(SystemExit):
            entry.parse_args(["--layout_shift"] + bad)
    assert entry.parse_args(["--layout_shift", "--ls_min_side", "0"]).ls_min_side == 0


def test_the_refusal_keeps_the_existing_wording(capsys):
    from mogan_amd.attngan import main as entry
    with pytest.raises(SystemExit):
        entry.parse_args(["--layout_shift", "--sampling"])
    assert "--layout_shift cannot be combined with --sampling or --r_precision" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        entry.parse_args(["--layout_shift", "--fid"])
    assert "--fid cannot be combined with --layout_shift" in capsys.readouterr().err


def test_the_flags_of_the_family_entry_point():
    from mogan_amd.stackgan import evaluate as FE
    from mogan_amd.stackgan import main_base
    args = main_base.parse_args(["--layout_shift", "--ls_min_shift", "6", "--ls_show", "4", "--num_samples", "9"])
    assert args.layout_shift and (args.ls_min_shift, args.ls_min_side, args.ls_show, args.num_samples) == (6, 1, 4, 9)
    assert FE.asked_scores(args) == {} and "layout_shift" not in FE.SCORES
    assert not main_base.parse_args([]).layout_shift
    for name in FE.SCORES:
        with pytest.raises(SystemExit):
            main_base.parse_args(["--layout_shift", "--" + name])
    for bad in (["--ls_min_shift", "0"], ["--ls_show", "-1"], ["--ls_min_side", "-0.5"], ["--ls_min_side", "nan"]):
        with pytest.raises(SystemExit):
            main_base.parse_args(["--layout_shift"] + bad)
    for bad in (-1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            LS.ShiftResponse(16, 1, 4, None, bad, 3, "cpu")
