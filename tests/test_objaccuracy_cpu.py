"""The numpy definition of object accuracy by nearest labelled training crops (stackgan/objaccuracy.py) on
hand-made cases whose counts are known: the vote and its tie rule, the class of a slot in the three trees, the figures, the
queries the margin leaves out, a class the bank does not hold, the listing -- and, still without a GPU, the host side of the
accumulator stackgan/evaluate.ObjectCrops (which slots are objects, their order, the unlabelled ones) with a stand-in for the crop
kernel, and the new flags of stackgan/main_base."""
import numpy as np
import pytest
import torch

from helpers import load_pkg

load_pkg()
from mogan_amd.stackgan import evaluate as EV  # noqa: E402
from mogan_amd.stackgan import main_base  # noqa: E402
from mogan_amd.stackgan import objaccuracy as OA  # noqa: E402
from mogan_amd.stackgan import synthetic  # noqa: E402

INF, NO = np.inf, OA.NO_ROW


def test_vote_most_members_then_the_earliest_first_member():
    lists = np.array([[3, 3, 7, 7, 7],        # 7 has most
                      [3, 7, 7, 3, 1],        # 3 and 7 tie at two: 3's first member comes first
                      [7, 3, 3, 7, 1],        # the same members, 7 first
                      [1, 2, 3, 4, 5],        # all tie at one: the nearest
                      [5, 5, 5, 5, 5],
                      [2, 9, 9, -1, -1],      # empty slots vote for nothing
                      [4, -1, -1, -1, -1],
                      [-1, -1, -1, -1, -1]])  # nothing listed
    assert OA.vote(lists).tolist() == [7, 3, 7, 1, 5, 9, 4, -1]
    assert OA.vote(np.array([[6], [0]])).tolist() == [6, 0]                     # K = 1: the nearest
    assert OA.vote(np.array([[0, 1, 1, 0]])).tolist() == [0] and OA.vote(np.array([[1, 0, 0, 1]])).tolist() == [1]
    for bad in (np.zeros((3,), dtype=np.int64), np.zeros((3, 0), dtype=np.int64), np.zeros((3, 2))):
        with pytest.raises(ValueError):
            OA.vote(bad)


def test_classes_of_the_three_trees():
    eye = np.eye(10, dtype=np.float32)
    assert OA.classes_of("mnist", eye[[3, 0, 9]]).tolist() == [3, 0, 9]
    assert OA.classes_of("mnist", eye[[[3, 0, 9], [1, 1, 2]]]).tolist() == [[3, 0, 9], [1, 1, 2]]
    clevr = np.zeros((4, 13), dtype=np.float32)
    for row, (shape, colour) in enumerate(((0, 0), (2, 7), (1, 4), (3, 8))):     # (3, 8): the absent slot's classes
        clevr[row, shape], clevr[row, 4 + colour] = 1, 1
    assert OA.classes_of("clevr", clevr).tolist() == [0, 2 * 9 + 7, 1 * 9 + 4, 3 * 9 + 8]
    assert max(s * 9 + c for s in range(4) for c in range(9)) == 35 and OA.CLASSES["clevr"] == 36
    coco = np.eye(81, dtype=np.float32)[[0, 79, 80, 17]]
    assert OA.classes_of("coco", coco).tolist() == [0, 79, -1, 17]              # class 80: no label
    with pytest.raises(ValueError):
        OA.classes_of("coco", eye)
    with pytest.raises(ValueError):
        OA.classes_of("birds", eye)
    # the synthetic batches' labels decode to what they were made from
    b = synthetic.make_batch("clevr", 6, seed=4)
    got = OA.classes_of("clevr", b["label_one_hot"].numpy())
    lab = b["label_one_hot"].numpy()
    assert (got == lab[..., :4].argmax(-1) * 9 + lab[..., 4:].argmax(-1)).all() and got.shape == (6, 4)


def test_before_is_the_lexicographic_order():
    assert OA.before([1.0, 2.0, 2.0, 2.0, INF, INF, 0.0], [5, 1, 1, 3, 4, NO, 2],
                     [2.0, 1.0, 2.0, 2.0, INF, INF, 0.0], [0, 9, 3, 1, NO, 4, 2]).tolist() == [True, False, True, False, True, False,
                                                                                              False]


# six queries of three images against a bank, by hand: (asked, neighbours' classes, same (d2, i), other (d2, i), image)
CASE = [
    (0, [0, 0, 1], (1.0, 4), (9.0, 7), 0),        # right; 1-NN right; margin (3 - 1) / (3 + 1) = 0.5
    (0, [1, 1, 0], (4.0, 2), (1.0, 3), 0),        # wrong; 1-NN wrong; margin (1 - 2) / (1 + 2) = -1/3
    (1, [1, 2, 3], (0.0, 5), (0.0, 6), 1),        # right by the tie rule; 1-NN right by position; both 0: no margin
    (1, [2, 1, 1], (4.0, 8), (4.0, 1), 1),        # right (two of three); 1-NN wrong by position; margin 0
    (2, [0, 1, 0], (INF, NO), (16.0, 0), 2),      # class 2 is not in the bank: wrong, 1-NN wrong, no margin
    (0, [0, 0, 0], (0.0, 9), (INF, NO), 2),       # nothing else in ... the other set is empty: right, 1-NN right, no margin
]


def _case(rows=CASE):
    asked = np.array([r[0] for r in rows])
    nbr = np.array([r[1] for r in rows])
    sd, si = np.array([r[2][0] for r in rows]), np.array([r[2][1] for r in rows])
    od, oi = np.array([r[3][0] for r in rows]), np.array([r[3][1] for r in rows])
    return asked, nbr, sd, si, od, oi, np.array([r[4] for r in rows])


def test_figures_of_a_hand_made_case():
    out = OA.figures(*_case())
    assert (out["n"], out["right"], out["right_1nn"]) == (6, 4, 3)
    assert out["accuracy"] == 4 / 6 and out["accuracy_1nn"] == 3 / 6
    assert out["per_class"] == {"0": [2, 3], "1": [2, 2], "2": [0, 1]} and out["classes"] == 3
    assert out["accuracy_per_class"] == pytest.approx((2 / 3 + 1 + 0) / 3, abs=1e-15)
    assert out["images"] == 3 and out["accuracy_per_image"] == pytest.approx((0.5 + 1.0 + 0.5) / 3, abs=1e-15)
    assert (out["margin_n"], out["margin_left_out"]) == (3, 3)                  # both 0; same infinite; other infinite
    assert out["margin"] == pytest.approx((0.5 - 1 / 3 + 0.0) / 3, abs=1e-15)
    assert OA.right(_case()[0], _case()[1]).tolist() == [True, False, True, True, False, True]


def test_the_queries_the_margin_leaves_out():
    m, has = OA.margins([1.0, 0.0, INF, 5.0, INF, 0.0, 4.0], [9.0, 0.0, 3.0, INF, INF, 1.0, 0.0])
    assert has.tolist() == [True, False, False, False, False, True, True]
    assert m[0] == 0.5 and m[5] == 1.0 and m[6] == -1.0 and np.isnan(m[[1, 2, 3, 4]]).all()
    every = OA.figures(*_case([CASE[2], CASE[4], CASE[5]]))
    assert every["margin"] is None and every["margin_n"] == 0 and every["margin_left_out"] == 3
    for bad in (([1.0], [np.nan]), ([-1.0], [1.0]), ([1.0, 2.0], [1.0])):
        with pytest.raises(ValueError):
            OA.margins(*bad)


def test_an_empty_class_and_perfect_and_rotated_labels():
    # the bank holds classes 0 and 1 only; every query is a copy of a bank row of its OWN class: all right, margin 1
    asked = np.array([0, 1, 0, 1])
    out = OA.figures(asked, np.array([[0, 0], [1, 1], [0, 1], [1, 0]]), np.zeros(4), np.arange(4), np.full(4, 25.0), np.arange(4) + 4,
                     np.array([0, 0, 1, 1]))
    assert out["accuracy"] == out["accuracy_1nn"] == out["accuracy_per_class"] == out["accuracy_per_image"] == 1.0
    assert out["margin"] == 1.0 and out["margin_left_out"] == 0
    # the same crops asked for class + 1 (class 2 is empty in the bank): all wrong, same and other change places
    out = OA.figures(asked + 1, np.array([[0, 0], [1, 1], [0, 1], [1, 0]]), np.array([25.0, INF, 25.0, INF]),
                     np.array([4, NO, 6, NO]), np.zeros(4), np.arange(4), np.array([0, 0, 1, 1]))
    assert out["accuracy"] == out["accuracy_1nn"] == out["accuracy_per_class"] == out["accuracy_per_image"] == 0.0
    assert out["margin"] == -1.0 and out["margin_left_out"] == 2 and out["per_class"] == {"1": [0, 2], "2": [0, 2]}


def test_most_wrong_ranks_by_margin_ties_by_row_and_places_the_left_out_at_their_limits():
    asked, nbr, sd, si, od, oi, image = _case()
    rows, margin = OA.most_wrong(sd, od, 10)
    # margins: 0.5, -1/3, (0: both 0), 0, (-1: same infinite), (+1: other infinite)
    assert rows.tolist() == [4, 1, 2, 3, 0, 5]
    assert np.isnan(margin[[0, 2, 5]]).all() and margin[1] == pytest.approx(-1 / 3) and margin[3] == 0.0 and margin[4] == 0.5
    assert OA.most_wrong(sd, od, 2)[0].tolist() == [4, 1] and OA.most_wrong(sd, od, 0)[0].tolist() == []
    with pytest.raises(ValueError):
        OA.most_wrong(sd, od, -1)


def test_figures_refuse_what_is_not_a_set_of_queries():
    a = _case()
    for bad in ((a[0][:0],) + a[1:], (a[0] - 1,) + a[1:], a[:2] + (a[2][:-1],) + a[3:], a[:6] + (a[6][:-1],), (a[0].astype(float),) + a[1:]):
        with pytest.raises(ValueError):
            OA.figures(*bad)


# ------------------------------------------------------------------------------------------------- the accumulator's host side
def _stand_in_resize(x, boxes, index, OH, OW, out=None):
    """not the kernel: the mean of the image and the box's four numbers, so that every row says where it came from"""
    for r in range(index.shape[0]):
        out[r] = x[int(index[r])].mean()
        out[r, 0, 0, :4] = boxes[r]
    return out


@pytest.mark.parametrize("tree", ["mnist", "clevr", "coco"])
def test_object_crops_lists_objects_in_image_then_slot_order(tree):
    b = synthetic.make_batch(tree, 5, seed=11, text_dim=8)
    G, C = b["tm"].shape[1], b["real_imgs"].shape[1]
    acc = EV.ObjectCrops(tree, 9, 64, C, G, side=4, device="cpu", resize=_stand_in_resize)
    fake = -b["real_imgs"]
    acc.sink(b["real_imgs"], fake, b["tm"], b["label_one_hot"], 5)
    acc.sink(b["real_imgs"], fake, b["tm"], b["label_one_hot"], 3)          # the last batch counts three images only
    classes, image, slot, box = acc.objects()
    cls = OA.classes_of(tree, b["label_one_hot"].numpy())
    bbox = b["bbox"].numpy().astype(np.float32)
    want = [(i, g) for i in range(5) for g in range(G) if bbox[i, g, 2] > 0 and bbox[i, g, 3] > 0 and cls[i, g] >= 0]
    want = want + [(5 + i, g) for i, g in want if i < 3]
    assert list(zip(image.tolist(), slot.tolist())) == want and acc.n == len(want) and acc.n_images == 8
    assert classes.tolist() == [int(cls[i % 5, g]) for i, g in want]
    absent = int((bbox[:, :, 2] <= 0).sum())
    assert len(want) == 8 * G - absent - int((bbox[:3, :, 2] <= 0).sum()) and (absent == 0 or tree != "mnist")
    if tree == "coco":
        assert acc.unlabelled == 0                                           # an absent slot has no box: it is no object at all
    crops = acc.finish()
    assert crops["real"].shape == crops["fake"].shape == (len(want), C * 16)
    for r, (i, g) in enumerate(want):
        assert crops["real"][r, 4] == b["real_imgs"][i % 5].mean() and crops["fake"][r, 4] == fake[i % 5].mean()
        assert np.abs(crops["real"][r, :4].numpy() - bbox[i % 5, g]).max() <= 4 * 2.0 ** -24     # boxes_from_theta's bound
    with pytest.raises(ValueError, match="do not fit"):
        acc.sink(b["real_imgs"], fake, b["tm"], b["label_one_hot"], 2)


def test_object_crops_counts_a_box_without_a_label_as_unlabelled():
    b = synthetic.make_batch("coco", 4, seed=2, text_dim=8)
    lab = b["label_one_hot"].clone()
    present = b["bbox"][:, :, 2] > 0
    lab[0, 0] = 0
    lab[0, 0, 80] = 1                                                        # a box whose label is "none"
    assert bool(present[0, 0])
    acc = EV.ObjectCrops("coco", 4, 64, 3, 3, side=4, device="cpu", resize=_stand_in_resize)
    acc.sink(b["real_imgs"], b["real_imgs"], b["tm"], lab, 4)
    assert acc.unlabelled == 1 and acc.n == int(present.sum()) - 1
    assert (0, 0) not in list(zip(acc.objects()[1].tolist(), acc.objects()[2].tolist()))
    assert (acc.objects()[0] >= 0).all() and (acc.objects()[0] < 80).all()


def test_min_side_leaves_small_boxes_out():
    b = synthetic.make_batch("mnist", 6, seed=5)
    w = np.minimum(b["bbox"][:, :, 2].numpy(), b["bbox"][:, :, 3].numpy()).astype(np.float32) * 64
    acc = EV.ObjectCrops("mnist", 6, 64, 1, 3, side=4, min_side=16, device="cpu", resize=_stand_in_resize)
    acc.sink(b["real_imgs"], b["real_imgs"], b["tm"], b["label_one_hot"], 6)
    assert 0 < acc.n == int((w >= 16).sum()) < 18


# ------------------------------------------------------------------------------------------------- the flags
def test_the_score_flags_parse_with_the_defaults_of_the_attngan_entry_point():
    from mogan_amd.attngan import main as attn
    none = main_base.parse_args([])
    assert EV.asked_scores(none) == {} and none.num_samples == 30000
    assert (none.oa_k, none.oa_side, none.oa_min_side, none.oa_bank_size, none.oa_show) == (5, 16, 1, None, 16)
    ref = attn.parse_args([])
    for name in ("swd_patches", "swd_dirs", "swd_repeats", "swd_min_res", "msssim_scales", "msssim_no_resample", "spectrum_window"):
        assert getattr(none, name) == getattr(ref, name), name
    every = main_base.parse_args(["--spectrum", "--msssim", "--swd", "--object_accuracy", "--oa_k", "3", "--msssim_no_resample"])
    asked = EV.asked_scores(every)
    assert list(asked) == list(EV.SCORES) == ["object_accuracy", "swd", "msssim", "spectrum"]       # any order of flags: the table's
    assert asked["object_accuracy"] == dict(k=3, side=16, min_side=1, bank_size=None, show=16)
    assert asked["msssim"] == dict(scales=5, same_caption=False) and asked["spectrum"] == dict(window="hann")
    assert asked["swd"] == dict(patches=128, dirs=128, repeats=4, min_res=16)
