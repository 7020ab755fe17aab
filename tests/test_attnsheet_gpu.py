"""-m gpu: the attention sheets on the device -- the two entries of csrc/mogan_attn_sheet.hip through ctypes with every buffer in
guard-banded, poisoned memory against the numpy fp64 oracle (tests/attnsheet_cases.py: cases, seeds and the derived bounds), the five
bit contracts of include/mogan_hip.h, the picks the kernel should never see, the rejected arguments and the two ops.  No bound here
comes from the code under test.

The fp32 inputs live in memguard.Guarded's float mode and are held bit for bit (memguard.Frozen holds the ops' inputs); the int32 and
fp64 tables and all outputs live in its byte mode as in tests/test_layoutshift_gpu.py."""
import numpy as np
import pytest
import torch

import attnsheet_cases as AC
import memguard as MG
from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import attnsheet as AS  # noqa: E402
from mogan_amd.hip import lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FULL = (slice(None),)


def _frozen(a, skew=0):
    """an input in guarded memory: fp32 as it is (skew: that many floats past a 16-byte boundary), anything else as its bytes"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        t = torch.from_numpy(a.copy()).to(DEV)
        if skew:
            g = MG.Guarded((t.numel() + skew,), (slice(skew, None),), DEV, base=t.reshape(-1))
            assert g.ptr % 16 == 4 * skew
            return g
        g = MG.Guarded(tuple(t.shape), FULL, DEV, base=t)
        assert g.ptr % 16 == 0
        return g
    t = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(DEV)
    g = MG.Guarded(tuple(t.shape), FULL, DEV, dtype=torch.uint8, base=t)
    assert g.ptr % 8 == 0
    return g


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert got.tobytes() == want.tobytes(), "%s: %d of %d bytes differ" % (
        what, int((got.view(np.uint8) != want.view(np.uint8)).sum()), got.nbytes)


def _all_same(got, want, what):
    for g, w, name in zip(got, want, ("sheet", "stats", "flags")):
        _same_bits(g, w, "%s, %s" % (what, name))


class Sheet:
    """one call of mogan_attn_sheet_f64 with every buffer guarded: run() -> (sheet (P, vis, vis, 3) u8, stats (P, 2), flags (P))"""

    def __init__(self, attn, lens, img, M, pick, alpha=AC.ALPHA, skew=(0, 0)):
        self.B, self.T, self.att, _ = attn.shape
        self.vis, self.alpha = int(M.shape[0]), alpha
        pick = np.asarray(pick, dtype=np.int32).reshape(-1, 2)
        self.P = pick.shape[0]
        self.inputs = {"attn": _frozen(attn, skew[0]), "cap_lens": _frozen(np.asarray(lens, dtype=np.int32)), "img": _frozen(img, skew[1]),
                       "table": _frozen(np.asarray(M, dtype=np.float64)), "pick": _frozen(pick)}
        self.sheet = MG.Guarded((self.P * self.vis * self.vis * 3,), FULL, DEV, dtype=torch.uint8)
        self.stats = MG.Guarded((8 * self.P * 2,), FULL, DEV, dtype=torch.uint8)
        self.flags = MG.Guarded((4 * self.P,), FULL, DEV, dtype=torch.uint8)
        self.outputs = (self.sheet, self.stats, self.flags)

    def call(self, **kw):
        v = {k: g.ptr for k, g in self.inputs.items()}
        v.update(P=self.P, B=self.B, T=self.T, att=self.att, vis=self.vis, alpha=self.alpha, sheet=self.sheet.ptr, stats=self.stats.ptr,
                 flags=self.flags.ptr)
        v.update(kw)
        rc = lib.load().mogan_attn_sheet_f64(v["attn"], v["cap_lens"], v["img"], v["table"], v["pick"], v["P"], v["B"], v["T"], v["att"],
                                             v["vis"], v["alpha"], v["sheet"], v["stats"], v["flags"], lib.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def run(self, what):
        # the sheet's bytes may equal the poison byte: a first fill with 0x00 and a second with 0x5A show that every byte is written
        results = []
        for fill in (0x00, 0x5A):
            for g in self.outputs:
                g.reset()
            self.sheet.view.fill_(fill)
            assert self.call() == 0
            for name, g in self.inputs.items():
                assert g.untouched(), "%s: %s or its bands were modified" % (what, name)
            for g, name in zip(self.outputs, ("sheet", "stats", "flags")):
                g.check(what="%s %s" % (what, name), written=False)                          # nothing outside the outputs
            s, f = self.stats.view.view(torch.int64), self.flags.view.view(torch.int32)
            assert not bool((s == -1).any()) and not bool((f == -1).any()), "%s: an output was never written" % what
            results.append((self.sheet.view.cpu().numpy().reshape(self.P, self.vis, self.vis, 3),
                            self.stats.view.view(torch.float64).cpu().numpy().reshape(self.P, 2), f.cpu().numpy().reshape(self.P)))
        _all_same(results[1], results[0], what + ": a second call over another fill")       # every byte written, and contract (a)
        return results[0]


class Conf:
    def __init__(self, attn, lens, skew=0):
        self.B, self.T, self.att, _ = attn.shape
        self.inputs = {"attn": _frozen(attn, skew), "cap_lens": _frozen(np.asarray(lens, dtype=np.int32))}
        self.conf = MG.Guarded((8 * self.B * self.T,), FULL, DEV, dtype=torch.uint8)

    def call(self, **kw):
        v = dict(attn=self.inputs["attn"].ptr, cap_lens=self.inputs["cap_lens"].ptr, B=self.B, T=self.T, att=self.att, conf=self.conf.ptr)
        v.update(kw)
        rc = lib.load().mogan_attn_conf_f64(v["attn"], v["cap_lens"], v["B"], v["T"], v["att"], v["conf"], lib.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def run(self, what):
        self.conf.reset()
        assert self.call() == 0
        for name, g in self.inputs.items():
            assert g.untouched(), "%s: %s or its bands were modified" % (what, name)
        self.conf.check(what=what + " conf", written=False)
        c = self.conf.view.view(torch.int64)
        assert not bool((c == -1).any()), "%s: an output was never written" % what
        return self.conf.view.view(torch.float64).cpu().numpy().reshape(self.B, self.T)


def _within(got, want, bound, what):
    bad = np.argwhere(~(np.abs(got - want) <= bound))
    assert not len(bad), "%s: %d values off, first at %s: got %r, want %r, bound %r" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])], bound[tuple(bad[0])])
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.where(bound > 0, np.abs(got - want) / bound, 0.0).max())


# ------------------------------------------------------------------------------------------------- 1: the entry points and the ops
@pytest.mark.parametrize("key", AC.CASES, ids=str)
def test_every_case_within_its_bound_in_guarded_memory(key):
    attn, lens, img, M, pick = AC.case(key)
    e = AC.expected(key)
    conf = Conf(attn, lens).run("conf %s" % (key,))
    share_c = _within(conf, e["conf"], e["conf_bound"], "conf %s" % (key,))
    assert (conf[e["conf"] == 0] == 0).all() and not np.signbit(conf).any()
    _same_bits(Conf(attn, lens).run("conf again"), conf, "conf: a second call")
    sheet, stats, flags = Sheet(attn, lens, img, M, pick).run("case %s" % (key,))
    assert (flags == e["flags"]).all(), "%s: flags %s, want %s" % (key, flags.tolist(), e["flags"].tolist())
    share_s = _within(stats, e["stats"], e["stats_bound"], "stats %s" % (key,))
    n = AC.check_sheet(sheet, e, "case %s" % (key,))
    print("case %s: conf uses %.3g of its bound, stats %.3g; %d of %d pixels one level apart; flags %s"
          % (key, share_c, share_s, n, sheet.size // 3, flags.tolist()))
    # the ops are the entries: host tables, frozen device tensors
    ta, ti, tm = torch.from_numpy(attn.copy()).to(DEV), torch.from_numpy(img.copy()).to(DEV), torch.from_numpy(np.array(M)).to(DEV)
    frozen = [MG.Frozen(ta), MG.Frozen(ti), MG.Frozen(tm.view(torch.uint8))]
    c = ops.attn_conf(ta, torch.from_numpy(lens))
    s, st, fl = ops.attn_sheet(ta, torch.from_numpy(lens), ti, tm, torch.from_numpy(pick), AC.ALPHA)
    torch.cuda.synchronize()
    for f in frozen:
        f.check("the ops %s" % (key,))
    assert c.dtype == torch.float64 and tuple(c.shape) == attn.shape[:2] and c.is_cuda
    assert s.dtype == torch.uint8 and st.dtype == torch.float64 and fl.dtype == torch.int32 and s.is_cuda and st.is_cuda and fl.is_cuda
    _same_bits(c.cpu().numpy(), conf, "ops.attn_conf against the entry")
    _all_same((s.cpu().numpy(), st.cpu().numpy(), fl.cpu().numpy()), (sheet, stats, flags), "ops.attn_sheet against the entry")


# ------------------------------------------------------------------------------------------------- 2: the bit contracts
CONTRACT_CASES = [(3, 6, 5, 2), (3, 32, 16, 3), (2, 12, 64, 4)]


def _three_picks(key):
    attn, lens, img, M, _ = AC.case(key)
    B = attn.shape[0]
    pick = np.array([(B - 1, 0), (1, int(lens[1]) - 1), (0, 0)], dtype=np.int32)
    return attn, lens, img, M, pick


@pytest.mark.parametrize("key", CONTRACT_CASES, ids=str)
def test_a_pick_has_the_bits_it_has_alone_reversed_and_inside_a_larger_batch(key):
    attn, lens, img, M, pick = _three_picks(key)
    whole = Sheet(attn, lens, img, M, pick).run("P = 3")
    for p in range(3):
        alone = Sheet(attn, lens, img, M, pick[p:p + 1]).run("P = 1")
        _all_same(alone, tuple(w[p:p + 1] for w in whole), "pick %d alone against its place in the list" % p)
    back = Sheet(attn, lens, img, M, pick[::-1]).run("reversed")
    _all_same(tuple(b[::-1] for b in back), whole, "the list in reverse order")
    # a larger batch: two foreign samples in front, one behind; the picks' samples move by two
    other = AC.attention(key, lens, "foreign")                         # foreign samples keep the lengths their maps were made for
    attn2 = np.concatenate([other[:2], attn, other[:1]])
    lens2 = np.concatenate([lens[:2], lens, lens[:1]]).astype(np.int32)
    img2 = np.concatenate([img[::-1][:2], img, img[::-1][:1]])
    moved = pick + np.array([2, 0], dtype=np.int32)
    inside = Sheet(attn2, lens2, img2, M, moved).run("inside B = %d" % attn2.shape[0])
    _all_same(inside, whole, "the picks inside a larger batch")


@pytest.mark.parametrize("key", CONTRACT_CASES[:2] + [(4, 7, 5, 3)], ids=str)
def test_the_bits_do_not_depend_on_the_alignment_of_the_maps_or_the_images(key):
    attn, lens, img, M, pick = _three_picks(key)
    whole = Sheet(attn, lens, img, M, pick).run("aligned")
    conf = Conf(attn, lens).run("aligned")
    for skew in ((1, 0), (0, 3), (2, 2), (3, 1)):
        got = Sheet(attn, lens, img, M, pick, skew=skew).run("maps and images %d and %d floats past a 16-byte boundary" % skew)
        _all_same(got, whole, "skew %s against aligned tensors" % (skew,))
    for skew in (1, 2, 3):
        _same_bits(Conf(attn, lens, skew=skew).run("maps %d floats past a 16-byte boundary" % skew), conf, "conf, skew %d" % skew)


@pytest.mark.parametrize("key", [(4, 3, 2, 2), (3, 6, 5, 2), (3, 32, 16, 3)], ids=str)
def test_a_caption_of_one_word_gives_exact_zeros_and_lo_equal_to_hi(key):
    attn, lens, img, M, _ = AC.case(key)
    assert lens[0] == 1 and (attn[0, 0] == 1).all()
    sheet, stats, flags = Sheet(attn, lens, img, M, [(0, 0)]).run("a flat map")
    assert flags.tolist() == [AS.FLAT]
    assert stats.view(np.int64).tolist() == [[0, 0]]                                        # +0.0 twice, bitwise
    want = AS.blend_u8(AS.image_u8(img[0]).transpose(1, 2, 0), np.zeros((M.shape[0], M.shape[0], 1), dtype=np.uint8), AC.ALPHA)
    _same_bits(sheet[0], want, "the sheet of a flat map: the image under a map of exact zeros")


@pytest.mark.parametrize("T", [5, 12])
def test_with_the_identity_table_the_sheet_is_the_oracles_byte_for_byte(T):
    key = (4, T, 5, 1)
    attn, lens, img = AC.attention(key), AC.lengths(key), AC.image(key)
    M = AS.table(5, 1)
    pick = np.array([(b, w) for b in range(3) for w in range(int(lens[b]))], dtype=np.int32)
    sheet, stats, flags = Sheet(attn, lens, img, M, pick).run("the identity table")
    want_sheet, want_stats, want_flags = AS.sheet_numpy(attn, lens, img, M, pick, AC.ALPHA)
    assert (want_flags == 0).any()
    _all_same((sheet, stats, flags), (want_sheet, want_stats, want_flags), "the identity table: S is A exactly")


def test_a_non_finite_map_is_answered_as_a_flat_one_with_flag_two():
    key = (3, 6, 5, 2)
    attn, lens, img, M, _ = AC.case(key)
    hot = attn.copy()
    hot[1, 2, 3, 1] = np.inf
    hot[2, 0, 0, 0] = np.nan
    pick = np.array([(1, 2), (1, 1), (2, 0)], dtype=np.int32)
    got = Sheet(hot, lens, img, M, pick).run("non-finite maps")
    want = AS.sheet_numpy(hot, lens, img, M, pick, AC.ALPHA)
    assert want[2].tolist() == [AS.NONFINITE, AS.OK, AS.NONFINITE] and got[2].tolist() == want[2].tolist()
    _same_bits(got[0][[0, 2]], want[0][[0, 2]], "the sheets of non-finite maps")
    assert not got[1][[0, 2]].any()
    clean = Sheet(attn, lens, img, M, pick[1:2]).run("the finite neighbour alone")
    _all_same(tuple(g[1:2] for g in got), clean, "the finite neighbour of two non-finite maps")


# ------------------------------------------------------------------------------------------------- 3: picks that are never sent
def _never(key):
    attn, lens, _, _, _ = AC.case(key)
    B, T = attn.shape[:2]
    return [("sample -1", (-1, 0)), ("sample B", (B, 0)), ("word = len", (2, int(lens[2]))), ("word = T", (1, T)), ("word -1", (1, -1)),
            ("sample 2^31 - 1", (2 ** 31 - 1, 0)), ("word -2^31", (1, -2 ** 31))]


@pytest.mark.parametrize("name", [n for n, _ in _never((3, 6, 5, 2))])
def test_a_pick_the_kernel_should_never_see_gets_zeros_and_its_neighbours_are_untouched(name):
    key = (3, 6, 5, 2)
    attn, lens, img, M, pick = _three_picks(key)
    whole = Sheet(attn, lens, img, M, pick).run("the legal list")
    bad = pick.copy()
    bad[1] = np.array(dict(_never(key))[name], dtype=np.int64).astype(np.int32)
    sheet, stats, flags = Sheet(attn, lens, img, M, bad).run("pick 1 illegal")
    assert flags[1] == AS.NEVER and not sheet[1].any() and stats[1].view(np.int64).tolist() == [0, 0]
    _all_same(tuple(g[[0, 2]] for g in (sheet, stats, flags)), tuple(w[[0, 2]] for w in whole), "the neighbours of a pick answered with zeros")
    assert AS.sheet_numpy(attn, lens, img, M, bad)[2][1] == AS.NEVER                          # the oracle agrees on what is never seen


# ------------------------------------------------------------------------------------------------- 4: rejected arguments
def test_rejected_arguments_return_minus_one_and_write_nothing():
    attn, lens, img, M, pick = AC.case((3, 6, 5, 2))
    run = Sheet(attn, lens, img, M, pick)
    for kw in (dict(att=1), dict(att=129), dict(vis=257), dict(vis=12), dict(vis=0), dict(T=33), dict(T=0), dict(P=0), dict(B=0),
               dict(alpha=-1), dict(alpha=256), dict(attn=None), dict(cap_lens=None), dict(img=None), dict(table=None),
               dict(pick=None), dict(sheet=None), dict(stats=None), dict(flags=None)):
        assert run.call(**kw) == -1, kw
        assert all(g.untouched() for g in run.outputs), kw
    run.run("after the rejections")
    conf = Conf(attn, lens)
    for kw in (dict(att=1), dict(att=129), dict(T=33), dict(T=0), dict(B=0), dict(attn=None), dict(cap_lens=None), dict(conf=None)):
        assert conf.call(**kw) == -1, kw
        assert conf.conf.untouched(), kw
    conf.run("after the rejections")
