"""The two CPU references of the radial-power-spectrum tests against each other (tests/spectrum_cases.py): the fp64 oracle on
numpy.fft.fft2 and the direct DFT in longdouble, at every case -- where the spread that the bound's multiple was chosen from is
asserted --, Parseval's identity, the analytic images, and the custom table."""
import numpy as np
import pytest

import spectrum_cases as S


@pytest.mark.parametrize("key", S.CASES, ids=str)
def test_the_oracle_against_the_direct_dft_in_longdouble(key):
    x, weight, win = S.case(key)
    assert x.dtype == np.float32 and x.shape == (key[1], key[2], key[0], key[0]) and float(np.abs(x).max()) <= 1.0
    want, bound = S.expected(key)
    spread = S.spread(key)
    print("%s: the references differ by %.4f units of eps log2(S^2) total (recorded maximum %.2f)" % (key, spread, S.MEASURED_SPREAD))
    # the record the multiple was chosen from holds here; twice it is allowed for another CPU's libm and FFT build, and even
    # that leaves the second term of the bound the larger one by a factor of three
    assert spread <= 2 * S.MEASURED_SPREAD and 2 * S.MEASURED_SPREAD < 1.0 / 3
    assert want.shape == bound.shape == (key[1], len(S.count_of(key[0]))) and (bound >= 0).all() and (want >= 0).all()
    assert (np.abs(want - S.references(key)[1]) <= bound / S.MULTIPLE).all()


def test_the_dynamic_range_image_keeps_its_artefact_above_the_bound():
    """a period-2 checkerboard of amplitude 1e-3 on a ramp of mean 0.6: its bin, the last, holds (1e-3 / 0.62)^2 = 2.6e-6 of bin 0's
    power -- images in [-1, 1] give no more at this amplitude -- and nothing else: a ramp that is linear in i and in j has no power
    off the two axes.  The bound there is another eight decades further down, so the artefact is resolved to eight digits."""
    for key in ((256, 2, 3, "none"), (32, 5, 1, "none")):
        x, weight, _ = S.case(key)
        want, bound = S.expected(key)
        b = S.KINDS.index("checker_on_ramp")
        last = want.shape[1] - 1
        assert 1e5 < want[b, 0] / want[b, last] < 1e6               # bin 0 against the checkerboard's bin
        assert bound[b, last] < 1e-8 * want[b, last]
        size = key[0]
        i = np.arange(size)
        sign = 1 - 2 * ((i[:, None] + i[None, :]) % 2)
        line = float((S.plane(x[b:b + 1], weight, None)[0] * sign).sum()) ** 2          # |F(S/2, S/2)|^2, directly
        assert abs(want[b, last] - line) <= bound[b, last]


@pytest.mark.parametrize("key", [k for k in S.CASES if k[0] <= 64], ids=str)
def test_parseval_with_a_table_that_keeps_every_bin(key):
    x, weight, win = S.case(key)
    want, _ = S.expected(key)
    total = S.total_power(x, weight, win)                           # S^2 sum (w y)^2
    assert np.allclose(want.sum(axis=1), total, rtol=1e-13, atol=0)
    one_bin = np.zeros((key[0], key[0] // 2 + 1), dtype=np.int32)   # ... and so does a table of a single bin
    assert np.allclose(S.sums(x, weight, win, one_bin, 1)[:, 0], total, rtol=1e-13, atol=0)


@pytest.mark.parametrize("size", (8, 32))
@pytest.mark.parametrize("C", (1, 3))
def test_the_analytic_images_hold_on_the_oracle(size, C):
    x, rows = S.analytic(size, C)
    assert len(rows) == len(x) and {r[0] for r in rows} >= {"impulse", "constant", "cosine %s" % ((size // 2, 0),),
                                                             "cosine %s" % ((size // 2, size // 2),)}
    worst = S.analytic_check(S.sums(x, S.weights(C), None), size, C)
    print("S = %d, C = %d: the oracle uses %.3f of the analytic tolerance" % (size, C, worst))
    got = S.sums(x, S.weights(C), None)
    p = got[0] / S.count_of(size)                                   # the impulse: every bin's p is equal
    assert np.allclose(p, p[0], rtol=1e-13, atol=0)


def test_a_custom_table_leaves_out_what_it_says():
    for size in (8, 32):
        table, n_bins = S.custom_table(size)
        assert (table == -1).any() and (table >= n_bins).any()
        x, weight, win = S.case((size, 5, 3, "hann"))
        part, every = S.sums(x, weight, win, table, n_bins), S.sums(x, weight, win)
        assert part.shape == (5, n_bins) and (part <= every[:, :n_bins] * (1 + 1e-12)).all() and (part[:, 1:] < every[:, 1:n_bins]).any()
        assert np.allclose(part, S.sums_direct(x, weight, win, table, n_bins), rtol=0, atol=float(S.unit(x, weight, win).max()))
