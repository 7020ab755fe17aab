"""The host side of MS-SSIM (attngan/msssim.py) against the definition written out in tests/msssim_cases.py, and that module's own
record: the oracle's closed-form properties, the two fp32 CPU evaluations whose error sets the bounds of tests/test_msssim_gpu.py,
the floor of the tolerance inputs' level terms, and the pair that is clamped.  No GPU: PairSimilarity.result is run on terms that
are put into its buffer by hand."""
import numpy as np
import pytest
import torch

import msssim_cases as S
from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import msssim as MS  # noqa: E402

SMALL = tuple(c for c in S.TOLERANCE_CASES if c[0] <= 64)


def test_scales_of():
    assert MS.scales_of(256, 5) == [256, 128, 64, 32, 16] and MS.scales_of(64, 5) == [64, 32, 16, 8, 4]
    assert MS.scales_of(256) == [256, 128, 64, 32, 16] and MS.scales_of(32, 4) == [32, 16, 8, 4] and MS.scales_of(4, 1) == [4]
    for size, scales in ((32, 5), (48, 5), (66, 3), (3, 1), (256, 0), (256, 6), (0, 1)):
        with pytest.raises(ValueError):
            MS.scales_of(size, scales)


@pytest.mark.parametrize("side", [1, 2, 4, 5, 8, 10, 11, 12, 16, 256])
def test_window(side):
    g = MS.window(side)
    n = min(11, side)
    assert g.dtype == np.float32 and g.shape == (n,) and g.flags["C_CONTIGUOUS"]
    assert abs(float(g.astype(np.float64).sum()) - 1.0) <= 2.0 ** -24                  # one fp32 rounding of a value near 1
    assert np.array_equal(g.view(np.int32), g[::-1].view(np.int32))                   # symmetric bit for bit
    assert np.array_equal(g.view(np.int32), S.window(side).view(np.int32))            # the definition's bits
    # the shrink rule: sigma = 1.5 n / 11, read from the ratio of the two middle-most distinct taps
    sigma = 1.5 * n / 11
    if n >= 3:
        c = (n - 1) / 2.0
        want = np.exp(-((0 - c) ** 2 - (1 - c) ** 2) / (2 * sigma * sigma))
        assert abs(float(g[0]) / float(g[1]) - want) <= 4 * 2.0 ** -24 * want
    if side >= 11:
        assert abs(float(g[5]) / float(g[4]) - np.exp(0.5 / 2.25)) <= 1e-6                # sigma = 1.5


def test_score_from_terms_against_closed_forms():
    ones = np.ones((5, 2))
    s, c = MS.score_from_terms(ones)
    assert s.shape == () and float(s) == 1.0 and not bool(c)
    for L in (1, 2, 3, 4, 5):
        w = np.array(S.WEIGHTS[:L]) / (1.0 if L == 5 else sum(S.WEIGHTS[:L]))
        for j in range(L):
            for x in (0.3, 0.75):
                t = np.ones((L, 2))
                t[j, 0 if j == L - 1 else 1] = x                        # the term that enters the product at level j
                t[j, 1 if j == L - 1 else 0] = -5.0 if j < L - 1 else 1.0    # ssim of a level but the last is not used
                s, c = MS.score_from_terms(t)
                assert abs(float(s) - x ** w[j]) <= 4 * np.finfo(np.float64).eps and not bool(c), (L, j, x)
    assert MS.weights_of(5).tolist() == list(S.WEIGHTS)               # as published: they add up to 1.0001
    assert abs(sum(MS.weights_of(3)) - 1.0) < 1e-15
    rng = np.random.RandomState(3)
    t = rng.uniform(-0.2, 1.0, (7, 3, 4, 2))
    got, want = MS.score_from_terms(t), S.score(t)
    assert got[0].shape == (7, 3) and np.allclose(got[0], want[0], rtol=1e-14, atol=0) and np.array_equal(got[1], want[1])
    assert want[1].any() and not want[1].all() and (got[0][got[1]] == 0).all() and (got[0][~got[1]] > 0).all()
    for bad in (np.ones((6, 2)), np.ones((5, 3)), np.ones((2,)), np.full((5, 2), np.nan)):
        with pytest.raises(ValueError):
            MS.score_from_terms(bad)


def test_the_oracle_gives_1_for_a_copy_and_is_symmetric():
    a, b = S.smooth_pairs(2, 3, 32, 5)
    assert (S.all_levels(a, a.copy(), 4) == 1.0).all()
    assert np.array_equal(S.all_levels(a, b, 4), S.all_levels(b, a, 4))
    ssim, cs, terms = S.level(a, b, S.window(32))
    assert ssim.shape == cs.shape == (2, 3, 22, 22) and terms.shape == (2, 2)
    assert (ssim <= cs + 1e-12).all() and (terms < 1).all()


def test_avg_down2_of_the_oracle_is_exact_on_integer_images():
    x = S.integer_image((3, 6, 10), 1)
    want = x.reshape(3, 3, 2, 5, 2).sum(axis=(2, 4)) / 4
    assert np.array_equal(S.avg_down2(x), want) and np.array_equal(S.avg_down2(x, np.float32), want.astype(np.float32))


def test_the_recorded_deviations_hold_on_the_small_cases():
    """MEASURED is the worst over all tolerance cases and seeds; the sides up to 64 under two seeds, measured here, stay within it
    for the numpy evaluation (elementwise IEEE arithmetic: the same on every CPU) and within twice of it for torch's conv2d, whose
    summation order is the library's"""
    worst = {"numpy": dict(map=0.0, term=0.0, score=0.0), "torch": dict(map=0.0, term=0.0, score=0.0)}
    for case in SMALL:
        size, L, C = case
        for seed in S.SEEDS[:2]:
            a, b, terms, sc = S.tolerance_case(case, seed)
            win = S.window(size)
            ssim, cs, _ = S.level(a, b, win)
            for name, t32, maps in (("numpy", S.all_levels(a, b, L, np.float32), S.level(a, b, win, np.float32)),
                                    ("torch", S.all_levels(a, b, L, np.float32, S.level_torch), S.level_torch(a, b, win))):
                w = worst[name]
                w["term"] = max(w["term"], float(np.abs(t32 - terms).max()))
                w["score"] = max(w["score"], float(np.abs(S.score(t32)[0] - sc).max()))
                w["map"] = max(w["map"], float(np.abs(maps[0] - ssim).max()), float(np.abs(maps[1] - cs).max()))
    print("fp32 CPU evaluations against fp64 on the small cases: %s; recorded over all cases: %s" % (worst, S.MEASURED))
    for k, v in S.MEASURED.items():
        assert 0 < worst["numpy"][k] <= v and 0 < worst["torch"][k] <= 2 * v, (k, worst, v)
    assert (S.TOL_MAP, S.TOL_TERM, S.TOL_SCORE) == tuple(4 * S.MEASURED[k] for k in ("map", "term", "score"))


@pytest.mark.parametrize("case", SMALL, ids=str)
def test_every_level_term_of_the_tolerance_pairs_is_above_the_floor(case):
    for seed in S.SEEDS:
        a, b, terms, sc = S.tolerance_case(case, seed)
        assert terms.shape == (S.PAIRS, case[1], 2) and float(terms.min()) >= S.TERM_FLOOR, (case, seed, float(terms.min()))
        assert (sc > S.TERM_FLOOR).all() and (sc < 1).all()


def test_the_clamped_pair():
    a, b, terms = S.find_clamp_pair()
    used = np.concatenate([terms[:-1, 1], terms[-1:, 0]])
    assert float(used.min()) < -0.01
    s, c = MS.score_from_terms(terms)
    assert float(s) == 0.0 and bool(c)
    assert S.score(terms)[0] == 0.0 and bool(S.score(terms)[1])


def test_result_on_terms_put_into_the_buffer_by_hand():
    ps = MS.PairSimilarity(32, 3, 6, scales=4, device="cpu")
    assert ps.sizes == [32, 16, 8, 4] and [int(w.numel()) for w in ps.windows] == [11, 11, 8, 4]
    with pytest.raises(ValueError, match="no pairs"):
        ps.result()
    rng = np.random.RandomState(2)
    terms = rng.uniform(0.3, 1.0, (5, 4, 2))
    terms[3] = S.find_clamp_pair()[2]
    ps.terms[:5] = torch.from_numpy(terms)
    ps.n = 5
    res = ps.result()
    sc = S.score(terms)[0]
    assert res["pairs"] == 5 and res["clamped"] == 1 and res["levels"] == [32, 16, 8, 4] and sc[3] == 0
    assert abs(res["mean"] - sc.mean()) <= 1e-14 and abs(res["std"] - sc.std()) <= 1e-14
    assert np.allclose(res["ssim"], terms[:, :, 0].mean(axis=0), rtol=1e-14) and np.allclose(res["cs"], terms[:, :, 1].mean(axis=0), rtol=1e-14)
    for kw in (dict(channels=0), dict(channels=5), dict(pairs=0), dict(size=32, scales=5), dict(size=100)):
        args = dict(size=32, channels=3, pairs=4, scales=4, device="cpu")
        args.update(kw)
        with pytest.raises(ValueError):
            MS.PairSimilarity(**args)


def test_add_refuses_what_it_would_have_to_convert():
    ps = MS.PairSimilarity(16, 3, 4, scales=3, device="cpu")
    good = torch.zeros(2, 3, 16, 16)
    for a, b in ((good.double(), good), (good, good[:, :, :, ::2]), (good[0], good[0]), (good, torch.zeros(3, 3, 16, 16)),
                 (torch.zeros(2, 1, 16, 16), torch.zeros(2, 1, 16, 16)), (good.numpy(), good),
                 (torch.zeros(5, 3, 16, 16), torch.zeros(5, 3, 16, 16)), (good.to("meta"), good.to("meta"))):
        with pytest.raises(ValueError):
            ps.add(a, b)
    assert ps.n == 0
