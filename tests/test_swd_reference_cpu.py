"""The oracle of the sliced Wasserstein tests (tests/swd_cases.py) against hand-computed values, the draw-order contract of
attngan/swd.py, figure_from_sums, and the claim the GPU module relies on: the exact cases really are exact -- the fp32 and the fp64
oracle agree bit for bit.  Nothing here needs a GPU or the library."""
import math

import numpy as np
import pytest

import swd_cases as S
from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import swd as SWD  # noqa: E402

# The mirror rule written out by hand as matrices: out = D x D^T for pyr_down, U d U^T for pyr_up (U carries the factor 2 per axis).
# Row oy of D_n lists the weights (in 16ths) the taps 2 oy - 2 .. 2 oy + 2 leave on rows 0 .. n - 1 after mirroring; row y of U_n
# the weights (in 8ths) that the taps y - 2 .. y + 2 leave on the EVEN rows 0, 2, .. of the zero-inserted image.
D4 = np.array([[6, 8, 2, 0], [1, 4, 7, 4]]) / 16.0
D6 = np.array([[6, 8, 2, 0, 0, 0], [1, 4, 6, 4, 1, 0], [0, 0, 1, 4, 7, 4]]) / 16.0
D8 = np.array([[6, 8, 2, 0, 0, 0, 0, 0], [1, 4, 6, 4, 1, 0, 0, 0], [0, 0, 1, 4, 6, 4, 1, 0], [0, 0, 0, 0, 1, 4, 7, 4]]) / 16.0
U4 = np.array([[6, 2], [4, 4], [1, 7], [0, 8]]) / 8.0
U6 = np.array([[6, 2, 0], [4, 4, 0], [1, 6, 1], [0, 4, 4], [0, 1, 7], [0, 0, 8]]) / 8.0
U8 = np.array([[6, 2, 0, 0], [4, 4, 0, 0], [1, 6, 1, 0], [0, 4, 4, 0], [0, 1, 6, 1], [0, 0, 4, 4], [0, 0, 1, 7], [0, 0, 0, 8]]) / 8.0


def test_the_mirror_rule_leaves_the_edge_sample_out():
    assert [S.mirror(i, 4) for i in range(-2, 6)] == [2, 1, 0, 1, 2, 3, 2, 1]
    assert [S.mirror(i, 7) for i in (-2, -1, 6, 7, 8)] == [2, 1, 6, 5, 4]


def test_pyr_down_of_a_4x4_image_by_hand():
    x = np.arange(16.0).reshape(1, 4, 4)                           # x[i][j] = 4 i + j: linear, so out = 4 r[a] + r[b]
    want = np.array([[3.75, 4.875], [8.25, 9.375]])               # r = (12, 30) / 16, the weighted mean index of D4's rows
    assert (S.pyr_down(x)[0] == want).all() and (D4 @ x[0] @ D4.T == want).all()
    assert (S.pyr_down(np.full((2, 4, 4), 7.0)) == 7.0).all()      # the weights add up to 1 at every border


def test_pyr_up_of_a_2x2_image_by_hand():
    d = np.array([[[1.0, 2.0], [3.0, 4.0]]])                       # d[i][j] = 1 + 2 i + j
    r = np.array([0.25, 0.5, 0.875, 1.0])                          # the weighted mean index of U4's rows
    want = 1 + 2 * r[:, None] + r[None, :]
    assert (S.pyr_up(d)[0] == want).all() and (U4 @ d[0] @ U4.T == want).all()
    assert (S.pyr_up(np.full((1, 2, 2), 3.0)) == 3.0).all()        # zero-insert parity: every phase of the filter adds up to 1 / 4


def test_a_6x8_image_by_hand():
    x = S.integer_image((2, 6, 8), 5)
    down = S.pyr_down(x)
    assert down.shape == (2, 3, 4)
    for n in range(2):
        assert (down[n] == D6 @ x[n].astype(np.float64) @ D8.T).all()          # dyadic rationals: exactly
        assert (S.pyr_up(down)[n] == U6 @ down[n] @ U8.T).all()
    assert (S.lap_residual(x, down) == x - S.pyr_up(down)).all()
    t = S.pyr_down(np.transpose(x, (0, 2, 1)))                     # H != W: a transposed image gives the transposed result
    assert (t == np.transpose(down, (0, 2, 1))).all()


def test_the_oracle_is_scipys_mirror_convolution():
    ndimage = pytest.importorskip("scipy.ndimage")
    k = np.outer(S.W5, S.W5)
    for shape in S.PYRAMID_SHAPES + [(1, 6, 8)]:
        x = S.gaussian_image(shape, 3).astype(np.float64)
        down = S.pyr_down(x)
        for n in range(shape[0]):
            assert np.allclose(down[n], ndimage.convolve(x[n], k, mode='mirror')[::2, ::2], rtol=0, atol=1e-14)
            z = np.zeros(shape[1:])
            z[::2, ::2] = down[n]
            assert np.allclose(S.pyr_up(down)[n], ndimage.convolve(z, 4 * k, mode='mirror'), rtol=0, atol=1e-14)


@pytest.mark.parametrize("shape", S.PYRAMID_SHAPES, ids=str)
def test_the_exact_cases_are_exact(shape):
    """integer images 0..255: one pyr_down step and one lap_residual step from the oracle's own down in fp32 = in fp64, bit for bit"""
    x = S.integer_image(shape, S.seed_of("exact", shape))
    d32, d64 = S.pyr_down(x, np.float32), S.pyr_down(x, np.float64)
    assert d32.dtype == np.float32 and (d32.astype(np.float64) == d64).all()
    r32, r64 = S.lap_residual(x, d32, np.float32), S.lap_residual(x, d64, np.float64)
    assert r32.dtype == np.float32 and (r32.astype(np.float64) == r64).all()
    assert (S.down_bound(x) >= 0).all() and (S.residual_bound(x, d64) > 0).any()


def test_a_two_deep_chain_is_exact_for_images_of_0_and_1_only():
    x = S.integer_image((2, 16, 16), 9, high=2)
    d1, d2 = S.pyr_down(x, np.float32), S.pyr_down(S.pyr_down(x, np.float32), np.float32)
    e1, e2 = S.pyr_down(x), S.pyr_down(S.pyr_down(x))
    assert (d2.astype(np.float64) == e2).all()
    assert (S.lap_residual(d1, d2, np.float32).astype(np.float64) == S.lap_residual(e1, e2)).all()
    lv32, lv64 = S.laplacian_levels(x.reshape(1, 2, 16, 16), [16, 8, 4], np.float32), S.laplacian_levels(x.reshape(1, 2, 16, 16), [16, 8, 4])
    assert all((a.astype(np.float64) == b).all() for a, b in zip(lv32, lv64))
    wide = S.integer_image((1, 16, 16), 9)                         # 0..255: the second level's residual needs more than 24 bits
    w1, w2 = S.pyr_down(wide), S.pyr_down(S.pyr_down(wide))
    assert not (S.lap_residual(w1, w2, np.float32).astype(np.float64) == S.lap_residual(w1, w2)).all()


def test_the_whole_score_cases_have_exact_levels():
    for C in S.SCORE_CASES:
        real, fake = S.score_images(C, S.seed_of("score", C))
        sizes = SWD.levels(S.SCORE["size"], S.SCORE["min_res"])
        assert sizes == [32, 16]
        for img in (real, fake):
            a, b = S.laplacian_levels(img, sizes, np.float32), S.laplacian_levels(img, sizes)
            assert all((u.astype(np.float64) == v).all() for u, v in zip(a, b))


# ------------------------------------------------------------------------------------------------------ the draw order
def test_centres_are_drawn_per_batch_per_level_all_x_then_all_y():
    sizes, B, P, seed = [64, 32, 16], 3, 5, 77
    rng = np.random.RandomState(seed)
    got = [SWD.draw_centres(rng, sizes, B, P) for _ in range(2)]   # two batches from one stream
    ref = np.random.RandomState(seed)
    for batch in got:
        assert len(batch) == 3
        for size, table in zip(sizes, batch):
            cx = ref.randint(3, size - 3, B * P)
            cy = ref.randint(3, size - 3, B * P)
            assert table.dtype == np.int32 and table.shape == (B * P, 3)
            assert (table[:, 0] == np.arange(B * P) // P).all() and (table[:, 1] == cy).all() and (table[:, 2] == cx).all()
            assert table[:, 1:].min() >= 3 and table[:, 1:].max() < size - 3
    assert ref.randint(0, 1 << 30) == rng.randint(0, 1 << 30)      # nothing else was drawn
    one = SWD.draw_centres(np.random.RandomState(1), [7], 2, 4)[0]     # a 7 x 7 level has one legal centre
    assert (one[:, 1:] == 3).all()


def test_directions_are_drawn_per_level_per_repeat_in_fp64_and_rounded_once():
    rng, ref = np.random.RandomState(9), np.random.RandomState(9)
    for C, D in ((3, 16), (3, 16), (1, 5)):
        got = SWD.draw_directions(rng, C, D)
        d = ref.randn(C * 49, D)
        want = (d / np.sqrt((d * d).sum(axis=0, keepdims=True))).astype(np.float32)
        assert got.dtype == np.float32 and got.shape == (C * 49, D) and got.flags["C_CONTIGUOUS"]
        assert (got == want).all()
        assert np.allclose(np.sqrt((got.astype(np.float64) ** 2).sum(axis=0)), 1.0, rtol=0, atol=1e-6)


def test_the_centre_streams_are_seed_and_seed_plus_1():
    """seen on the class with host buffers: its generators and sizes need no device (the directions' stream, seed + 2, is held by
    the whole-score test of the GPU module, whose oracle draws from it)"""
    sw = SWD.SlicedWasserstein(32, 3, 16, patches=8, dirs=4, repeats=1, min_res=16, seed=40, device="cpu")
    assert sw.rng["real"].randint(0, 1 << 30) == np.random.RandomState(40).randint(0, 1 << 30)
    assert sw.rng["fake"].randint(0, 1 << 30) == np.random.RandomState(41).randint(0, 1 << 30)
    assert sw.sizes == [32, 16] and sw.bytes == 2 * 2 * 16 * 147 * 4


# ------------------------------------------------------------------------------------------------------ the figure
def test_figure_from_sums():
    sums = np.array([[3.0, 5.0], [1.0, 7.0], [2.0, 2.0]])          # 3 repeats, 2 directions, 4 rows
    assert SWD.figure_from_sums(sums, 4) == ((8.0 / 8 + 8.0 / 8 + 4.0 / 8) / 3) * 1000.0
    assert SWD.figure_from_sums(np.zeros((2, 5)), 9) == 0.0
    assert isinstance(SWD.figure_from_sums(sums, 4), float)
    rng = np.random.RandomState(0)
    s = rng.rand(4, 128) * 1e6
    want = float(np.mean([math.fsum(r) / (1000 * 128) for r in s.tolist()])) * 1000
    assert abs(SWD.figure_from_sums(s, 1000) - want) <= 4 * 2.0 ** -53 * want
    assert SWD.figure_from_sums(s[:, ::-1], 1000) == SWD.figure_from_sums(s, 1000)          # exactly rounded sums: no order
    for bad, rows in ((np.zeros(3), 4), (np.zeros((0, 3)), 4), (np.zeros((2, 0)), 4), (sums, 0), (-sums, 4),
                      (np.array([[np.nan, 1.0]]), 4), (np.array([[np.inf, 1.0]]), 4)):
        with pytest.raises(ValueError):
            SWD.figure_from_sums(bad, rows)


def test_the_oracles_bounds_are_of_the_size_the_formats_give():
    """the closed forms, looked at once: a few ulps of the values they bound"""
    x = S.gaussian_image((2, 8, 32), 1)
    assert (S.down_bound(x) <= 25 * S.U32 * np.abs(x).max()).all() and S.down_bound(x).max() > S.U32 * 0.1
    desc = S.moment_inputs(257, 3, 2)
    b = S.moments_bounds(desc, 3)
    ref = S.moments(desc, 3).astype(np.float64)
    assert (b > 0).all() and (b[:, 0] < 1e-9 * (np.abs(ref[:, 0]) + ref[:, 1])).all() and (b[:, 1] < 1e-9 * ref[:, 1]).all()
    got = np.stack([desc.astype(np.float64).reshape(257, 3, 49).mean(axis=(0, 2)), desc.astype(np.float64).reshape(257, 3, 49).std(axis=(0, 2))], axis=1)
    assert (np.abs(got - ref) <= b).all()                          # numpy's own fp64 moments lie inside them
    for case in S.PROJECT_CASES:
        d, m, v = S.project_inputs(case)
        dev = S.numpy_fp32_deviation(d, m, v)
        print("%s: numpy fp32 matmul deviates from fp64 by %.3e at most" % (case, dev))
        assert 0 < dev < 1e-4
