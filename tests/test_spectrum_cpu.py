"""attngan/spectrum.py without a GPU: the table of bins against a brute-force one and the integer rule, the figures on hand-made
profiles, and the normalisation -- white noise of unit variance averages to 1 in every bin."""
import json

import numpy as np
import pytest

import spectrum_cases as S
from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import spectrum as SP  # noqa: E402

SIZES = (8, 16, 32, 64, 128, 256)


@pytest.mark.parametrize("size", SIZES)
def test_radial_bins_against_brute_force_and_the_integer_rule(size):
    table, count = SP.radial_bins(size)
    full = S.full_table(size)
    assert table.dtype == np.int32 and table.shape == (size, size // 2 + 1) and table.flags["C_CONTIGUOUS"]
    assert np.array_equal(table, full[:, :size // 2 + 1])
    # the integer rule at every entry of the full plane: (2 r - 1)^2 <= 4 (fu^2 + fv^2) < (2 r + 1)^2 -- no float rounding decides it
    f = S.signed(size).astype(np.int64)
    q = 4 * (f[:, None] ** 2 + f[None, :] ** 2)
    r = S.unfold(table, size)
    assert np.array_equal(r, full)
    assert (((2 * r - 1) ** 2 <= q) | (r == 0)).all() and (q < (2 * r + 1) ** 2).all() and (q[r == 0] == 0).all()
    # sqrt(fu^2 + fv^2) is a half-integer where 4 (fu^2 + fv^2) is an odd square: a multiple of 4 never is, so there is no
    # frequency at which float rounding and the rule could part
    root = np.round(np.sqrt(q.astype(np.float64))).astype(np.int64)
    assert not ((root * root == q) & (root % 2 == 1)).any()
    n_bins = int(full[size // 2, size // 2]) + 1
    assert len(count) == n_bins == int(table.max()) + 1 and count.sum() == size * size and count[0] == 1 and (count > 0).all()
    assert np.array_equal(count, np.bincount(full.ravel()))
    # the half plane with multiplicity 1 at v in {0, S / 2} and 2 elsewhere reproduces the full plane's counts
    m = np.full(size // 2 + 1, 2)
    m[0] = m[-1] = 1
    assert np.array_equal(np.bincount(table.ravel(), weights=np.broadcast_to(m, table.shape).ravel()).astype(np.int64), count)
    assert n_bins <= 256                                            # one thread per bin in the kernel


def test_the_window_the_weights_and_the_energy():
    for size in SIZES:
        w = SP.hann(size)
        assert w.dtype == np.float32 and np.array_equal(w, S.hann(size)) and w[0] == 0 and w[size // 2] == 1
        assert np.array_equal(w[1:], w[1:][::-1])                   # periodic: symmetric about S / 2
        assert SP.window_energy(w, size) == pytest.approx(S.energy(w, size), rel=1e-15)
        assert SP.window_energy(None, size) == float(size) ** 2
        assert SP.make_window("none", size) is None and SP.make_window(None, size) is None
    assert np.array_equal(SP.channel_weights(3), np.asarray(S.LUMA, np.float32)) and np.array_equal(SP.channel_weights(1), [1.0])
    assert SP.window_name(None) == "none" and SP.window_name("hann") == "hann"


def _profile(size, f):
    _, count = SP.radial_bins(size)
    k = np.arange(len(count), dtype=np.float64)
    return np.array([f(max(x, 0.5)) for x in k]), count


def test_identical_sides_give_zero_everywhere():
    p, count = _profile(64, lambda k: 3.0 / k ** 1.5)
    out = SP.figures(p, p.copy(), count, 64)
    assert out["lsd_db"] == 0.0 and out["hf_db"] == 0.0 and all(d == 0.0 for d in out["excess_db"]) and out["empty_bins"] == []
    assert out["slope_real"] == out["slope_fake"] and out["count"] == count.tolist()
    json.dumps(out)


def test_doubling_the_power_from_a_quarter_of_the_sampling_frequency_upwards():
    p, count = _profile(64, lambda k: 3.0 / k ** 1.5)
    q = p.copy()
    q[64 // 4 + 1:] *= 2
    out = SP.figures(p, q, count, 64)
    assert out["hf_db"] == pytest.approx(10 * np.log10(2.0), abs=1e-12)
    n = len(p) - 1
    assert out["lsd_db"] == pytest.approx(10 * np.log10(2.0) * np.sqrt((n - 16) / n), rel=1e-12)
    assert SP.figures(q, p, count, 64)["hf_db"] == pytest.approx(-10 * np.log10(2.0), abs=1e-12)


def test_a_profile_that_falls_as_the_square_of_the_frequency_has_a_slope_of_minus_20_db_per_decade():
    p, count = _profile(256, lambda k: 7.0 / k ** 2)
    q, _ = _profile(256, lambda k: 0.1 / k ** 3)
    out = SP.figures(p, q, count, 256)
    assert out["slope_real"] == pytest.approx(-20.0, abs=1e-9) and out["slope_fake"] == pytest.approx(-30.0, abs=1e-9)
    want = S.figures(p, q, count, 256)
    for key in ("lsd_db", "hf_db", "slope_real", "slope_fake"):
        assert out[key] == pytest.approx(want[key], rel=1e-12), key
    assert out["peak"]["bin"] == want["peak"]["bin"]


def test_the_peak_is_found_at_the_planted_bin_with_its_period():
    for size, k in ((256, 64), (256, 128), (256, 32), (64, 16), (256, 181)):
        p, count = _profile(size, lambda f: 2.0 / f ** 2)
        q = p.copy()
        q[k] *= 10 ** 0.7                                          # +7 dB at one bin
        out = SP.figures(p, q, count, size)
        assert out["peak"]["bin"] == k and out["peak"]["period"] == size / k
        assert out["peak"]["excess_db"] == pytest.approx(7.0, abs=1e-9) and out["excess_db"][k] == out["peak"]["excess_db"]
    out = SP.figures(q, p, count, 256)                              # a deficit is a peak too
    assert out["peak"]["bin"] == 181 and out["peak"]["excess_db"] == pytest.approx(-7.0, abs=1e-9)


def test_empty_bins_are_left_out_and_listed():
    p, count = _profile(32, lambda k: 1.0 / k)
    q = p * 1.5
    p2, q2 = p.copy(), q.copy()
    p2[5] = 0.0
    q2[20] = 0.0
    out = SP.figures(p2, q2, count, 32)
    assert out["empty_bins"] == [5, 20]
    assert out["excess_db"][5] is None and out["excess_db"][20] is None
    assert out["profile_real_db"][5] is None and out["profile_fake_db"][5] is not None and out["profile_fake_db"][20] is None
    assert out["lsd_db"] == pytest.approx(10 * np.log10(1.5), rel=1e-12)        # the others all differ by the same factor
    assert out["hf_db"] == pytest.approx(10 * np.log10(1.5), rel=1e-12)
    want = S.figures(p2, q2, count, 32)
    assert out["empty_bins"] == want["empty_bins"] and out["slope_real"] == pytest.approx(want["slope_real"], rel=1e-12)
    json.dumps(out)
    with pytest.raises(ValueError, match="no bin"):
        SP.figures(np.zeros_like(p), q, count, 32)


def test_white_noise_of_unit_variance_averages_to_1_in_every_bin():
    """64 seeded normal images at S = 32, no clipping.  Per image and frequency |F|^2 / energy is (for a real plane) exponentially
    distributed with mean 1 and standard deviation 1 -- chi^2 with one degree of freedom, standard deviation sqrt(2), at the four
    frequencies that are their own mirror image; a frequency and its mirror image carry the same value.  So a bin of count[k]
    members averages count[k] / 2 independent values per image at the least, and the mean over N images has a standard error of
    at most sqrt(2 / (N count[k])) (sqrt(2 / N) for the bins of a single member).  The test allows 5 standard errors: 47 bins,
    one chance in 40 000 per seed, and the seed is fixed."""
    size, N = 32, 64
    rng = np.random.RandomState(S.seed_of("white", size))
    x = rng.standard_normal((N, 1, size, size)).astype(np.float32)
    count = S.count_of(size)
    for name in S.WINDOWS:
        win = S.window(name, size)
        p = S.profile(x, S.weights(1), win)
        mine = SP.profiles(S.sums(x, S.weights(1), win), SP.radial_bins(size)[1], SP.window_energy(win, size))
        assert np.allclose(mine, p, rtol=1e-14, atol=0)
        P = SP.side_profile(mine)
        se = np.sqrt(2.0 / (N * count))
        if name == "hann":                 # the window correlates neighbouring frequencies: fewer independent values per bin.  The
            se = se * 35.0 / 18.0          # variance of an average grows by S sum w^4 / (sum w^2)^2 = 35 / 18 per axis
        worst = np.abs(P - 1.0) / se
        print("window %s: worst bin %d at %.2f standard errors" % (name, int(worst.argmax()), worst.max()))
        assert (worst <= 5.0).all(), (name, int(worst.argmax()), float(worst.max()))
