"""The oracle of the object crop (tests/scenefid_cases.py) against itself and against torch, without a GPU: its fp32 blend against
its fp64 blend under the derived bound TOL_BLEND (the figure the module records is measured here again), the exact cases bit for
bit, the full box against torch.nn.functional.interpolate, and what an absent box gives."""
import numpy as np
import torch
import torch.nn.functional as F

import scenefid_cases as S


def test_the_fp32_blend_is_within_the_derived_bound_of_the_fp64_blend():
    """400 random cases; the worst error in units of 2^-24 max|x| is printed, held under the bound of 7 and to the record"""
    rng = np.random.RandomState(S.seed_of("blend", 400))
    worst = 0.0
    for _ in range(400):
        x, boxes, index, OH, OW = S.random_case(rng)
        want = S.roi_resize_oracle(x, boxes, index, OH, OW)
        got = S.roi_resize_oracle(x, boxes, index, OH, OW, blend=np.float32)
        assert got.dtype == np.float32 and want.dtype == np.float64
        err = float(np.abs(got.astype(np.float64) - want).max())
        assert err <= S.tol_blend(x), (err, S.tol_blend(x))
        worst = max(worst, err / (S.EPS * float(np.abs(x).max())))
    print("fp32 blend against fp64 over 400 cases: %.3f x 2^-24 max|x| (recorded %.2f, bound %d)"
          % (worst, S.MEASURED["blend_ulps"], S.TOL_BLEND_ULPS))
    assert worst <= S.TOL_BLEND_ULPS
    assert abs(worst - S.MEASURED["blend_ulps"]) <= 0.05 * S.MEASURED["blend_ulps"]           # the record is this measurement


def test_the_kernel_cases_hold_what_they_are_there_for():
    cs = S.KERNEL_CASES
    assert {c[1] for c in cs.values()} >= {1, 3, 4}                                          # C
    assert any(c[2] != c[3] and c[4] != c[5] for c in cs.values())                           # non-square both ways
    assert any(c[4] == 1 for c in cs.values()) and any(c[5] == 1 for c in cs.values())
    assert any(c[2] * c[3] % 64 for c in cs.values()) and all(len(c[6]) * c[4] * c[5] % 256 for c in cs.values())
    assert any(len(c[6]) * c[4] * c[5] < 256 for c in cs.values()) and any(len(c[6]) * c[4] * c[5] > 512 for c in cs.values())
    boxes = [b for _, b in S.MIXED]
    images = [i for i, _ in S.MIXED]
    assert S.ABSENT in boxes[1:-1] and images.count(0) >= 2 and 1 not in images               # absent mid-list; an image with none
    f = np.float32
    assert any(f(f(b[0]) + f(b[2])) == f(0.999) and f(f(b[1]) + f(b[3])) == f(0.999) for b in boxes)
    assert (0.0, 0.0, 1.0, 1.0) in boxes and any(0 < b[2] * 40 < 1 for b in boxes) and any(b[0] + b[2] > 1 for b in boxes)
    assert any(b[0] < 0 for b in boxes if b != S.ABSENT)


def test_the_exact_cases_are_exact():
    for name in S.EXACT_CASES:
        x, boxes, index, OH, OW, want = S.exact_case(name)
        got = S.roi_resize_oracle(x, boxes, index, OH, OW, blend=np.float32)
        assert np.array_equal(got.astype(np.float64), want), name                            # every fp64 value is a fp32 number
        assert np.abs(want).max() > 0 and float(np.abs(x).max()) < 64


def test_the_full_box_is_bilinear_interpolation():
    """within 4 * 2^-24 max|x| (the two blends' roundings) + 2^-16 (one ulp of a coordinate below 256) x the largest difference
    between neighbouring pixels"""
    worst = 0.0
    for shape, out in (((2, 3, 256, 256), (299, 299)), ((2, 3, 33, 40), (19, 23)), ((1, 4, 7, 5), (1, 9)), ((1, 1, 16, 12), (64, 75))):
        x = np.random.RandomState(S.seed_of("interpolate", shape)).uniform(-1, 1, shape).astype(np.float32)
        B = shape[0]
        boxes = np.tile(np.array([[0, 0, 1, 1]], dtype=np.float32), (B, 1))
        got = S.roi_resize_oracle(x, boxes, np.arange(B), out[0], out[1], blend=np.float32)
        want = F.interpolate(torch.from_numpy(x), size=out, mode="bilinear", align_corners=False).numpy()
        step = max(float(np.abs(np.diff(x, axis=2)).max()) if shape[2] > 1 else 0.0,
                   float(np.abs(np.diff(x, axis=3)).max()) if shape[3] > 1 else 0.0)
        bound = 4 * S.EPS * float(np.abs(x).max()) + 2.0 ** -16 * step
        err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
        print("%s -> %s: the full box is %.3e off F.interpolate (bound %.3e)" % (shape, out, err, bound))
        assert err <= bound, (shape, err, bound)
        worst = max(worst, err)
    print("worst %.3e (recorded %.1e)" % (worst, S.MEASURED["interpolate"]))
    assert worst <= 2 * S.MEASURED["interpolate"]


def test_an_absent_box_a_bad_value_and_a_bad_index_give_zeros():
    x = np.random.RandomState(5).uniform(-1, 1, (2, 3, 9, 8)).astype(np.float32)
    boxes = np.array([S.ABSENT, (0.1, 0.1, 0.0, 0.5), (0.1, 0.1, 0.5, -0.5), (0.1, np.nan, 0.5, 0.5), (np.inf, 0.1, 0.5, 0.5),
                      (0.1, 0.1, 0.5, 0.5), (0.1, 0.1, 0.5, 0.5), (0.1, 0.1, 0.5, 0.5)], dtype=np.float32)
    index = np.array([0, 1, 0, 1, 0, 2, -1, 1])
    out = S.roi_resize_oracle(x, boxes, index, 6, 5)
    assert not out[:7].any() and out[7].any()
