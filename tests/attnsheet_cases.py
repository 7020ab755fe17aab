"""The cases the tests of the attention sheets share (tests/test_attnsheet_gpu.py, test_attnsheet_reference_cpu.py): attention maps,
caption lengths, images, tables, picks, the expected values of the numpy oracle (attngan/attnsheet.py) and the bounds a device value
is held to.  A plain module.

CASES are (P, T, att, up): picks, words, side of the attention map, upscaling (vis = att * up).
  att in {2, 5, 16} x up in {1, 2, 3}   every small shape: odd att (the zero-padded last term), vis below one strip of 32 rows, below
                                        one wave's 64 columns, vis = 48 (a second, partial strip), up = 1 (the identity table)
  (2, 12, 64, 4), (2, 12, 128, 2)       the product's two stages
B = 3 samples (2 for the two large cases) with captions of length 1, T and in between; at length 1 the softmax is 1 everywhere and
nothing passes the threshold 2 / 1: a flat map.  The attention is a softmax over a caption's words of seeded logits, zero past the
caption's length, as the generator's.  The small cases smooth with sigma = up (sigma = 20 flattens a map of 8 pixels until
hi / (hi - lo) passes 10^4); the large ones with the reference's 20.

The bounds.  u = 2^-53.  The fp32 map is widened exactly and both sides threshold it in fp32 against the same fp32 constants, so A is
the same matrix.  Every entry of M and A is >= 0, so every sum below has non-negative terms and an error relative to the sum itself.
  S = (M A) M^T.  A dot product of n terms carries at most n roundings per term whatever the order and whether or not product and sum
      are fused (one per fma, or one for the product and n - 1 for the additions): the computed value is the exact one times
      (1 + theta), |theta| <= gamma_n = n u / (1 - n u).  U = M A has n = att, S = U M^T has n = att over computed U: each side's S
      is within gamma_{2 att} of the exact product, the device's and the oracle's within 2 * 2 att * u = 2 att 2^-52 of each other up
      to second order, which the + 4 covers generously: rel = c (2 att + 4) 2^-52 with c = 1.
  lo, hi: the minimum of values each within rel of their counterparts is within rel of the counterparts' minimum; stats bound =
      rel * |oracle's value|.
  conf: n = att^2 exact products added in any order: (n - 1) u per side, bound = (n + 4) 2^-52 conf.
  v = (S - lo) / (hi - lo) * 255.  With f = (S - lo) / (hi - lo) in [0, 1] and the SAME lo in numerator and denominator, to first order
      dv / 255 = [dS - (1 - f) dlo - f dhi] / (hi - lo), |.| <= rel [S + (1 - f) lo + f hi] / (hi - lo) <= 2 rel hi / (hi - lo);
      the bound takes 3 for the second order, plus 4 ulp of 255 for the three roundings of the expression on either side:
      v_bound = 255 * 3 * rel * hi / (hi - lo) + 4 * 255 * 2^-52, from the ORACLE's hi and lo.
  A byte of the sheet may differ from the oracle's only where the oracle's v lies within v_bound of an integer, then by one level of q,
  which moves the blended byte by at most ceil(alpha / 255) = 1.
Derived, not measured."""
import zlib

import numpy as np

from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import attnsheet as AS  # noqa: E402

SMALL = [(3, 1, 2, 1), (4, 3, 2, 2), (3, 4, 2, 3), (4, 5, 5, 1), (3, 6, 5, 2), (4, 7, 5, 3), (3, 4, 16, 1), (4, 9, 16, 2), (3, 32, 16, 3)]
LARGE = [(2, 12, 64, 4), (2, 12, 128, 2)]
CASES = SMALL + LARGE
EPS = 2.0 ** -52
ALPHA = 180


def seed_of(what, key):
    return zlib.crc32(("%s %s" % (what, key)).encode()) & 0x7FFFFFFF


def sigma_of(key):
    return 20.0 if key in LARGE else float(key[3])


_tables = {}


def table_of(att, up, sigma):
    k = (att, up, sigma)
    if k not in _tables:
        _tables[k] = AS.table(att, up, sigma)
        _tables[k].setflags(write=False)
    return _tables[k]


def lengths(key):
    P, T, att, up = key
    if key in LARGE:
        return np.array([T, (T + 1) // 2 + 1], dtype=np.int32)
    return np.array([1, T, max(1, (T + 1) // 2)], dtype=np.int32)


def attention(key, lens=None, what="attn"):
    """(B, T, att, att) fp32: per sample a softmax over its caption's words, zeros past its length"""
    P, T, att, up = key
    lens = lengths(key) if lens is None else lens
    rng = np.random.RandomState(seed_of(what, key))
    out = np.zeros((len(lens), T, att, att), dtype=np.float32)
    for b, n in enumerate(lens):
        z = rng.standard_normal((int(n), att, att)) * 2.0
        e = np.exp(z - z.max(axis=0, keepdims=True))
        out[b, :int(n)] = (e / e.sum(axis=0, keepdims=True)).astype(np.float32)
    return out


def image(key, B=None):
    P, T, att, up = key
    B = len(lengths(key)) if B is None else B
    rng = np.random.RandomState(seed_of("img", key))
    return np.clip(rng.standard_normal((B, 3, att * up, att * up)) * 0.6, -1, 1).astype(np.float32)


def picks(key):
    """(P, 2) int32: legal picks that reach every sample -- the length-1 caption's only word among them (small cases)"""
    P, T, att, up = key
    lens = lengths(key)
    rng = np.random.RandomState(seed_of("pick", key))
    rows = []
    for p in range(P):
        b = p % len(lens)
        rows.append((b, int(rng.randint(int(lens[b])))))
    return np.array(rows, dtype=np.int32)


def case(key):
    """(attn, cap_lens, img, M, pick) of a case, numpy"""
    return attention(key), lengths(key), image(key), table_of(key[2], key[3], sigma_of(key)), picks(key)


def rel_of(att):
    return (2 * att + 4) * EPS


def v_bound(lo, hi, att):
    return 255.0 * 3.0 * rel_of(att) * hi / (hi - lo) + 4 * 255.0 * EPS


def near_integer(v, bound):
    """where v lies within bound of an integer: the pixels whose level a legal error may move"""
    return np.abs(v - np.round(v)) <= bound


_expected = {}


def expected(key):
    """the oracle's answers for a case, computed once and handed out read-only: dict(conf, conf_bound, sheet, stats, stats_bound, flags,
    may (list per pick: bool (vis, vis), the pixels that may differ by one level))"""
    if key not in _expected:
        attn, lens, img, M, pick = case(key)
        e = expected_of(attn, lens, img, M, pick)
        _expected[key] = e
    return _expected[key]


def expected_of(attn, lens, img, M, pick, alpha=ALPHA):
    att = attn.shape[2]
    conf = AS.conf_numpy(attn, lens)
    sheet, stats, flags, vs = AS.sheet_numpy(attn, lens, img, M, pick, alpha, want_v=True)
    may = []
    for p, v in enumerate(vs):
        if v is None:
            may.append(np.zeros(sheet.shape[1:3], dtype=bool))
        else:
            may.append(near_integer(v, v_bound(stats[p, 0], stats[p, 1], att)))
    e = dict(conf=conf, conf_bound=(att * att + 4) * EPS * conf, sheet=sheet, stats=stats, stats_bound=rel_of(att) * np.abs(stats),
             flags=flags, may=may)
    for t in list(e.values())[:-1] + may:
        t.setflags(write=False)
    return e


def check_sheet(got, e, what):
    """a device sheet against the oracle's: equal bytes, or one level apart where the oracle's v is within its bound of an integer, at
    most one such pixel per map -> the number of such pixels"""
    want = e["sheet"]
    assert got.shape == want.shape and got.dtype == np.uint8
    total = 0
    for p in range(want.shape[0]):
        d = np.abs(got[p].astype(np.int64) - want[p].astype(np.int64)).max(axis=2)
        off = d > 0
        assert not (off & ~e["may"][p]).any(), "%s: pick %d, %d bytes differ where the oracle's v is not within its bound of an integer, " \
            "first at %s" % (what, p, int((off & ~e["may"][p]).sum()), tuple(np.argwhere(off & ~e["may"][p])[0]))
        assert d.max() <= 1, "%s: pick %d differs by %d levels" % (what, p, int(d.max()))
        assert int(off.sum()) <= 1, "%s: pick %d has %d pixels one level apart" % (what, p, int(off.sum()))
        total += int(off.sum())
    return total
