"""-m gpu: the entry points at the end of the train step, as include/mogan_hip.h declares them -- the discriminators' logits head,
the BCE / BCE-with-logits / KL losses and the reparametrisation, the DAMSM word and sentence similarities with their two
cross-entropies, the scalar sums and the fused Adam step -- through ctypes, per element against fp64 and under the memory contract
of tests/memguard.py: what tests/test_pathway_entry_points_gpu.py does for the object pathway.  Tables, inputs, references and
bounds are tests/loss_cases.py; tests/test_loss_reference_cpu.py derives the tolerances without a GPU and
tests/test_loss_rejections_cpu.py holds every rejection that is answered before a launch.

Memory, every call:
  * every output -- the nullable wt when asked for, the 2R scratch nll and out2 included -- is the payload of a guard-banded
    buffer, NaN-poisoned; afterwards every element is written and nothing outside has changed;
  * p / m / v / ema of the Adam step and the accumulating scalars and gradients hold a finite base in such a buffer: the one to
    three elements behind a ragged last float4 stay as they were;
  * every input -- cap_lens, labels (int64, as bytes), mask, g0 / g1, gout and dev_state where it is one included -- lives in NaN
    bands and is bitwise unchanged afterwards, bands included;
  * the same call a second time, after poisoning again, gives the same bits (the family has no atomics).

Values: every element within TOL[kind] * S (+ FLOOR) of loss_cases, exact zeros where S == 0, a -inf where the reference has one,
and beside that the whole-tensor figures of tests/test_kernels_gpu.py (loss_cases.REL).  Bit-for-bit identities between calls that
follow from the code are asserted where both sides run.  The last test asserts the census of what ran and prints the largest
err / bound per output kind."""
import ctypes

import numpy as np
import pytest
import torch

import loss_cases as K
import memguard as mg
from helpers import load_pkg, rel_l2

load_pkg()
from mogan_amd.hip import lib, ops  # noqa: E402
from oracle import attngan_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS = lambda v: str(v).replace(" ", "")
G1, G2, G3 = K.GAMMAS

RAN = set()
FIG = {}               # output kind -> largest err / bound


def L():
    return lib.load()


def _inp(t):
    """an input inside NaN guard bands, frozen (bands included); int32 travels as its fp32 bit pattern, int64 as bytes"""
    if t.dtype == torch.int32:
        t = t.view(torch.float32)
    if t.dtype == torch.int64:
        t = t.contiguous().view(torch.uint8)
    g = mg.Guarded(tuple(t.shape), (Ellipsis,), DEV, dtype=t.dtype, base=t)
    g.frozen = mg.Frozen(g.buf)
    return g


def _scalar(v):
    return _inp(torch.tensor([v], dtype=torch.float32))


def _out(shape, base=None):
    """an output: NaN-poisoned, or (base) holding the finite values the call adds onto / updates in place"""
    return mg.Guarded(tuple(shape), (Ellipsis,), DEV, base=base)


def _p(g):
    return None if g is None else g.ptr


def _sync(rc, what):
    torch.cuda.synchronize()
    assert rc == 0, "%s: return code %d" % (what, rc)


def _verify(g, ref, S, kind, what, rel=True):
    """the memory contract of the buffer; every element within loss_cases.bound(kind, S) -- an exact zero where S is 0, the
    same infinity where the reference has one; and the whole-tensor figure REL[kind] (rel=False: the one-channel words backward,
    loss_cases.words_rel_applies)"""
    assert g.problems() == [], "%s: %s" % (what, "; ".join(g.problems()))
    got = g.view.cpu().double()
    ref = ref.double().reshape(got.shape)
    bnd = K.bound(kind, S).reshape(got.shape)
    inf = torch.isinf(ref)
    assert bool((got[inf] == ref[inf]).all()), "%s: another value where the reference is infinite" % what
    err = torch.where(inf, torch.zeros_like(ref), (got - ref).abs())
    sel = (bnd > 0) | ~(err == 0)                       # (where the bound is 0 a correct element has nothing to report)
    frac = float(torch.nan_to_num(err / bnd.clamp_min(1e-300), nan=float("inf"))[sel].max()) if bool(sel.any()) else 0.0
    FIG[kind] = max(FIG.get(kind, 0.0), frac)
    print("%s: largest err / bound %.3f" % (what, frac))
    bad = ~(err <= bnd)
    if bool(bad.any()):
        i = tuple(torch.nonzero(bad)[0].tolist())
        raise AssertionError("%s: %d elements off the bound (largest err / bound %.3f; first at %s: got %r, want %r, bound %.3e)"
                             % (what, int(bad.sum()), frac, i, float(got[i]), float(ref[i]), float(bnd[i])))
    fig = K.figure(kind, torch.where(inf, torch.zeros_like(got), got), torch.where(inf, torch.zeros_like(ref), ref))
    assert fig <= K.REL[kind] or not rel, "%s: whole-tensor figure %.3e > %.1e" % (what, fig, K.REL[kind])


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b, what):
    assert torch.equal(_bits(a), _bits(b)), "%s: other bits" % what


def _twice(call, outs, what):
    """run `call` (-> return code), keep the bits, restore poison / base, run again: the same bits, everything written"""
    _sync(call(), what)
    first = [g.view.clone() for g in outs]
    for g in outs:
        g.reset()
    _sync(call(), what + ", second call")
    for g, f in zip(outs, first):
        assert g.problems() == [], (what, g.problems())
        _same_bits(f, g.view, what + ", second call")
    return first


def _frozen(gs, what):
    for g in gs:
        if g is not None:
            g.frozen.check(what)


# ------------------------------------------------------------------------------------------------------------ logits head
HEAD_CALLS = [r + (True,) for r in K.HEAD_ROWS] + [K.HEAD_ROWS[-1] + (False,)]


@pytest.mark.parametrize("B,Kd,Cout,with_bias", HEAD_CALLS, ids=IDS)
def test_logits_head_fwd_bwd(B, Kd, Cout, with_bias):
    what = "head %s bias %s" % ((B, Kd, Cout), with_bias)
    d = K.head_case(B, Kd, Cout, with_bias)
    ref, S = d["ref"], d["S"]
    x, w, dp, pin = (_inp(d[k]) for k in ("x", "w", "dp", "p_in"))
    bias = _inp(d["bias"]) if with_bias else None
    p = _out((B, Cout))
    _twice(lambda: L().mogan_logits_head_fwd(x.ptr, w.ptr, _p(bias), p.ptr, B, Kd, Cout, lib.stream_ptr()), [p], what + " fwd")
    _verify(p, ref["p"], S["p"], "p", what + " p")
    if (B, Kd, Cout) == K.HEAD_SATURATED:
        assert p.view[0, 0].item() == 1.0 and p.view[1, 0].item() == 0.0, what + ": not saturated"
        RAN.add(("head", "saturated"))
    bwd = lambda dx, dw, db, acc: L().mogan_logits_head_bwd(dp.ptr, pin.ptr, x.ptr, w.ptr, _p(dx), _p(dw), _p(db), B, Kd, Cout, acc,
                                                             lib.stream_ptr())
    for acc in (0, 1):
        mk = lambda: (_out((B, Kd)), _out((Cout, Kd), d["base_w"] if acc else None), _out((Cout,), d["base_b"] if acc else None))
        dx, dw, db = mk()
        first = _twice(lambda: bwd(dx, dw, db, acc), [dx, dw, db], what + " bwd acc %d" % acc)
        sfx = "+" if acc else ""
        _verify(dx, ref["dx"], S["dx"], "head_dx", what + " dx")
        _verify(dw, ref["dw" + sfx], S["dw" + sfx], "head_dw", what + " dw acc %d" % acc)
        _verify(db, ref["db" + sfx], S["db" + sfx], "head_db", what + " db acc %d" % acc)
        # each of dx / dw / db NULL in turn: the others keep their bits
        for skip in range(3):
            outs = list(mk())
            outs[skip] = None
            live = [g for g in outs if g is not None]
            _sync(bwd(*outs, acc), what + " bwd without %s" % ("dx", "dw", "db")[skip])
            for g, f in zip(live, [f for k, f in enumerate(first) if k != skip]):
                assert g.problems() == [], (what, g.problems())
                _same_bits(f, g.view, what + " bwd without %s" % ("dx", "dw", "db")[skip])
            RAN.add(("head NULL", ("dx", "dw", "db")[skip]))
        RAN.add(("head accumulate", acc))
    assert bwd(None, None, None, 0) == 0              # nothing wanted: returns 0, launches nothing
    torch.cuda.synchronize()
    RAN.add(("head NULL", "all"))
    _frozen((x, w, dp, pin, bias), what)
    RAN.add(("head", (B, Kd, Cout), with_bias))


# ------------------------------------------------------------------------------------------------------ elementwise losses
@pytest.mark.parametrize("n", K.ELEM_N)
def test_bce_and_bce_with_logits(n):
    inp = K.elem_inputs(n)
    p, x, gout = _inp(inp["p"]), _inp(inp["x"]), _scalar(K.GOUT)
    for fwd, bwd, src, case, kl, kg in (("mogan_bce_fwd", "mogan_bce_bwd", p, K.bce_case, "bce", "bce_dp"),
                                        ("mogan_bce_logits_fwd", "mogan_bce_logits_bwd", x, K.bcel_case, "bcel", "bcel_dx")):
        for t in K.TARGETS:
            for w in K.WEIGHTS:
                what = "%s n %d target %s weight %s" % (kl, n, t, w)
                plain = None
                for acc in (0, 1):
                    d = case(n, t, w, acc)
                    loss = _out((1,), torch.tensor([K.BASE]) if acc else None)
                    first, = _twice(lambda: getattr(L(), fwd)(src.ptr, t, w, loss.ptr, n, acc, lib.stream_ptr()), [loss],
                                    what + " fwd acc %d" % acc)
                    _verify(loss, d["ref"][kl], d["S"][kl], kl, what + " loss acc %d" % acc)
                    if acc:         # accumulate = 1 onto base is base + (the accumulate = 0 result), one fp32 addition
                        want = torch.tensor([K.BASE], dtype=torch.float32) + plain.cpu()
                        _same_bits(first.cpu(), want, what + ": accumulate against base + plain")
                    plain = first
                dg = _out((n,))
                _twice(lambda: getattr(L(), bwd)(src.ptr, t, w, gout.ptr, dg.ptr, n, lib.stream_ptr()), [dg], what + " bwd")
                _verify(dg, d["ref"][kg], d["S"][kg], kg, what + " gradient")
                assert bool(torch.isfinite(dg.view).all()), what
    _frozen((p, x, gout), "bce n %d" % n)
    RAN.add(("elem", "bce", n))
    RAN.add(("elem ends mid-wave", bool(n % 64)))


@pytest.mark.parametrize("n", K.ELEM_N)
def test_kl_and_reparametrisation(n):
    what = "kl n %d" % n
    inp, d = K.elem_inputs(n), K.kl_case(n)
    mu, lv, eps, dc, gout = _inp(inp["mu"]), _inp(inp["lv"]), _inp(inp["eps"]), _inp(inp["dc"]), _scalar(K.GOUT)
    loss, dmu, dlv = _out((1,)), _out((n,)), _out((n,))
    _twice(lambda: L().mogan_kl_fwd(mu.ptr, lv.ptr, loss.ptr, n, lib.stream_ptr()), [loss], what + " fwd")
    _verify(loss, d["ref"]["kl"], d["S"]["kl"], "kl", what + " loss")
    _twice(lambda: L().mogan_kl_bwd(mu.ptr, lv.ptr, gout.ptr, dmu.ptr, dlv.ptr, n, lib.stream_ptr()), [dmu, dlv], what + " bwd")
    _verify(dmu, d["ref"]["kl_dmu"], d["S"]["kl_dmu"], "kl_dmu", what + " dmu")
    _verify(dlv, d["ref"]["kl_dlv"], d["S"]["kl_dlv"], "kl_dlv", what + " dlogvar")
    c, rmu, rlv = _out((n,)), _out((n,)), _out((n,))
    _twice(lambda: L().mogan_reparam_fwd(mu.ptr, lv.ptr, eps.ptr, c.ptr, n, lib.stream_ptr()), [c], what + " reparam fwd")
    _verify(c, d["ref"]["c"], d["S"]["c"], "c", what + " c")
    _twice(lambda: L().mogan_reparam_bwd(lv.ptr, eps.ptr, dc.ptr, rmu.ptr, rlv.ptr, n, lib.stream_ptr()), [rmu, rlv], what + " reparam bwd")
    rmu.check(inp["dc"], exact=True, what=what + " reparam dmu = dc")
    _verify(rlv, d["ref"]["rp_dlv"], d["S"]["rp_dlv"], "rp_dlv", what + " reparam dlogvar")
    _frozen((mu, lv, eps, dc, gout), what)
    RAN.add(("elem", "kl", n))


# ------------------------------------------------------------------------------------------------------------------ words
def _words_fwd(ctx, words, lens, dims, outs, wt):
    B, Bc, C, S_, T_ = dims
    sim, a1, a2, wc = outs
    return L().mogan_damsm_words_fwd(ctx.ptr, words.ptr, lens.ptr, B, Bc, C, S_, T_, G1, G2, G3, sim.ptr, a1.ptr, a2.ptr, wc.ptr, _p(wt),
                                     lib.stream_ptr())


def _words_outs(B, Bc, C, S_, T_):
    return [_out((B, Bc)), _out((B, Bc, S_, T_)), _out((B, Bc, T_, S_)), _out((B, C, Bc, T_))]


@pytest.mark.parametrize("row", K.WORDS_ROWS, ids=IDS)
def test_words_fwd_bwd(row):
    B, Bc, C, S_, T_, kind = row
    dims = row[:5]
    what = "words %s" % (row,)
    d = K.words_case(*row)
    ref, S = d["ref"], d["S"]
    ctx, words, lens, dsim = _inp(d["ctx"]), _inp(d["words"]), _inp(d["lens"]), _inp(d["dsim"])
    outs, wt = _words_outs(*dims), _out((C, Bc, T_))
    first = _twice(lambda: _words_fwd(ctx, words, lens, dims, outs, wt), outs + [wt], what + " fwd")
    for g, k in zip(outs, ("sim", "a1", "a2", "wc")):
        _verify(g, ref[k], S[k], k, what + " " + k)
    # wt is the words transposed to (C, Bc, T) with zeros behind each caption's end, bit for bit
    wt.check(ref["wt"].float(), exact=True, what=what + " wt")
    # wt = NULL: the other outputs keep their bits
    outs2 = _words_outs(*dims)
    _sync(_words_fwd(ctx, words, lens, dims, outs2, None), what + " fwd, wt NULL")
    for g, f in zip(outs2, first):
        assert g.problems() == [], (what, g.problems())
        _same_bits(f, g.view, what + " fwd, wt NULL")
    # what the padded word slots hold does not matter: zero padding against NaN padding
    n = d["lens"].long().clamp(0, T_)
    if bool((n < T_).any()):
        wz = _inp(torch.nan_to_num(d["words"]))
        outs3, wt3 = _words_outs(*dims), _out((C, Bc, T_))
        _sync(_words_fwd(ctx, wz, lens, dims, outs3, wt3), what + " fwd, zero padding")
        for g, f in zip(outs3 + [wt3], first):
            assert g.problems() == [], (what, g.problems())
            _same_bits(f, g.view, what + " fwd, zero padding against NaN padding")
        _frozen((wz,), what)
        RAN.add(("words padding", "NaN against zero"))
    if bool((n == 0).any()):
        assert bool((outs[0].view[:, (n == 0).to(DEV)] == -float("inf")).all()), what + ": sim of an empty caption"
    # a pair's workgroup does not depend on the grid: the square sub-call that contains the pair
    if B != Bc:
        m = min(B, Bc)
        cs, ws, ls = _inp(d["ctx"][:m]), _inp(d["words"][:m]), _inp(d["lens"][:m])
        sub = _words_outs(m, m, C, S_, T_)
        _sync(_words_fwd(cs, ws, ls, (m, m, C, S_, T_), sub, None), what + " square sub-call")
        assert all(g.problems() == [] for g in sub), what
        _same_bits(first[0][:m, :m], sub[0].view, what + " sim against the square sub-call")
        _same_bits(first[1][:m, :m], sub[1].view, what + " a1 against the square sub-call")
        _same_bits(first[2][:m, :m], sub[2].view, what + " a2 against the square sub-call")
        _same_bits(first[3][:m, :, :m], sub[3].view, what + " wc against the square sub-call")
        _frozen((cs, ws, ls), what)
        RAN.add(("words non-square", "B < Bc" if B < Bc else "B > Bc"))
    # backward from the reference's saved tensors, rounded
    a1i, a2i, wci = (_inp(d["saved"][k]) for k in ("a1", "a2", "wc"))
    dwc, dst = _out((B, C, Bc, T_)), _out((B, Bc, T_, S_))
    _twice(lambda: L().mogan_damsm_words_bwd(ctx.ptr, words.ptr, lens.ptr, a1i.ptr, a2i.ptr, wci.ptr, dsim.ptr, B, Bc, C, S_, T_, G1, G2, G3,
                                             dwc.ptr, dst.ptr, lib.stream_ptr()), [dwc, dst], what + " bwd")
    rel = K.words_rel_applies(C)
    _verify(dwc, ref["dwc"], S["dwc"], "dwc", what + " dwc", rel)
    _verify(dst, ref["dscore_t"], S["dscore_t"], "dscore_t", what + " dscore_t", rel)
    _frozen((ctx, words, lens, dsim, a1i, a2i, wci), what)
    RAN.add(("words TT", K.words_tt(T_), "full" if T_ == K.words_tt(T_) else "part"))
    RAN.update(("words channel loop", t) for t in K.words_channel_loop(C))
    RAN.update([("words S fwd", K.words_s_regime(S_)[0]), ("words S bwd", K.words_s_regime(S_)[1]), ("words lens", kind)])
    RAN.update(("words lens clamp", k) for k, v in K.lens_clamps(d["lens"], T_).items() if v)
    if row == K.WORDS_LDS_EDGE:
        RAN.add(("words", "LDS edge"))


# -------------------------------------------------------------------------------------------------------- cross-entropies
def _ce_fwd(sim, lab, mask, R, outs):
    prow, pcol, nll, out2 = outs
    return L().mogan_damsm_ce_fwd(sim.ptr, lab.ptr, _p(mask), R, R, prow.ptr, pcol.ptr, nll.ptr, out2.ptr, lib.stream_ptr())


@pytest.mark.parametrize("R,mk,lk", K.CE_ROWS, ids=IDS)
def test_cross_entropies_fwd_bwd(R, mk, lk):
    what = "ce %s" % ((R, mk, lk),)
    d = K.ce_case(R, mk, lk)
    ref, S = d["ref"], d["S"]
    sim, lab = _inp(d["sim"]), _inp(d["lab"])
    mask = None if d["mask"] is None else _inp(d["mask"])
    outs = [_out((R, R)), _out((R, R)), _out((2 * R,)), _out((2,))]
    _twice(lambda: _ce_fwd(sim, lab, mask, R, outs), outs, what + " fwd")
    for g, k, kind in zip(outs, ("prow", "pcol", "nll", "out2"), ("prow", "pcol", "ce", "ce")):
        _verify(g, ref[k], S[k], kind, what + " " + k)
    if mask is not None and bool(d["mask"].any()):           # a masked entry: an exact zero, its NaN score read into nothing
        off = d["mask"].bool()
        assert float(outs[0].view.cpu()[off].abs().max()) == 0 and float(outs[1].view.cpu()[off].abs().max()) == 0, what
    prow, pcol = _inp(d["prow_in"]), _inp(d["pcol_in"])
    for g0v, g1v in K.CE_G:
        g0, g1 = (None if v is None else _scalar(v) for v in (g0v, g1v))
        dsim = _out((R, R))
        _twice(lambda: L().mogan_damsm_ce_bwd(prow.ptr, pcol.ptr, lab.ptr, _p(g0), _p(g1), R, R, dsim.ptr, lib.stream_ptr()), [dsim],
               what + " bwd %s" % ((g0v, g1v),))
        _verify(dsim, ref[("dsim", g0v, g1v)], S[("dsim", g0v, g1v)], "ce_dsim", what + " dsim %s" % ((g0v, g1v),))
        _frozen((g0, g1), what)
        RAN.add(("ce g", g0v is not None, g1v is not None))
    _frozen((sim, lab, mask, prow, pcol), what)
    RAN.add(("ce", R, mk, lk))


# ---------------------------------------------------------------------------------------------------------- sentence loss
@pytest.mark.parametrize("B,Bc,C,kind,eps", K.SENT_ROWS, ids=IDS)
def test_sentence_similarity_fwd_bwd(B, Bc, C, kind, eps):
    what = "sent %s" % ((B, Bc, C, kind, eps),)
    d = K.sent_case(B, Bc, C, kind, eps)
    cnn, rnn, dsim = _inp(d["cnn"]), _inp(d["rnn"]), _inp(d["dsim"])
    sim, dcnn = _out((B, Bc)), _out((B, C))
    _twice(lambda: L().mogan_damsm_sent_fwd(cnn.ptr, rnn.ptr, B, Bc, C, G3, eps, sim.ptr, lib.stream_ptr()), [sim], what + " fwd")
    _verify(sim, d["ref"]["ssim"], d["S"]["ssim"], "ssim", what + " sim")
    _twice(lambda: L().mogan_damsm_sent_bwd(cnn.ptr, rnn.ptr, dsim.ptr, B, Bc, C, G3, eps, dcnn.ptr, lib.stream_ptr()), [dcnn], what + " bwd")
    _verify(dcnn, d["ref"]["dcnn"], d["S"]["dcnn"], "dcnn", what + " dcnn")
    _frozen((cnn, rnn, dsim), what)
    RAN.add(("sent", (B, Bc, C), kind, eps))


# ------------------------------------------------------------------------------------------------------------ scalar sums
@pytest.mark.parametrize("n", K.SUM_N)
def test_scalar_sum_and_scale(n):
    what = "scalar n %d" % n
    d = K.sum_case(n)
    ins = [_scalar(float(v)) for v in d["v"]]
    tab = (ctypes.c_void_p * 8)(*([g.ptr for g in ins] + [None] * (8 - n)))
    w = (ctypes.c_float * 8)(*(d["w"].tolist() + [0.0] * (8 - n)))
    out = _out((1,))
    _twice(lambda: L().mogan_scalar_sum(ctypes.cast(tab, ctypes.c_void_p), ctypes.cast(w, ctypes.c_void_p), n, out.ptr, lib.stream_ptr()),
           [out], what + " sum")
    _verify(out, d["ref"], d["S"], "sum", what + " sum")
    g = _scalar(K.GOUT)
    outs = [_out((1,)) for _ in range(n)]
    otab = (ctypes.c_void_p * 8)(*([o.ptr for o in outs] + [None] * (8 - n)))
    _twice(lambda: L().mogan_scalar_scale(g.ptr, ctypes.cast(w, ctypes.c_void_p), n, ctypes.cast(otab, ctypes.c_void_p), lib.stream_ptr()),
           outs, what + " scale")
    for k, o in enumerate(outs):                # out[k] = w[k] * g, exactly
        o.check(torch.tensor([np.float32(d["w"][k].item()) * np.float32(K.GOUT)], dtype=torch.float32), exact=True,
                what=what + " scale %d" % k)
    _frozen(ins + [g], what)
    RAN.add(("scalar", n))


# ------------------------------------------------------------------------------------------------------------------- adam
def _adam_bufs(d, ema):
    return [_out((d["p"].numel(),), d[k]) for k in ("p", "m", "v")] + ([_out((d["p"].numel(),), d["ema"])] if ema else [])


def _adam_call(bufs, g, n, em, gs, step, state):
    h = K.ADAM_HYPER
    p, m, v = bufs[:3]
    ema = bufs[3] if len(bufs) > 3 else None
    return L().mogan_adam_step(p.ptr, g.ptr, m.ptr, v.ptr, _p(ema), n, h["lr"], h["beta1"], h["beta2"], h["eps"], step, _p(state), em, gs,
                               h["ema_decay"], lib.stream_ptr())


def _adam_verify(bufs, ref, S, what):
    for g, k in zip(bufs, ("adam_p", "adam_m", "adam_v", "adam_ema")):
        _verify(g, ref[k], S[k], k, what + " " + k)          # (the bands behind element n - 1 are part of the memory contract)


@pytest.mark.parametrize("row,zero", [(r, False) for r in K.ADAM_ROWS] + [(K.ADAM_ZERO_ROW, True)], ids=IDS)
def test_adam_step_in_place(row, zero):
    n, ema, em, gs, step = row                # (zero: the row with g = 0 and v = 0, denom = eps)
    what = "adam %s%s" % ((n, ema, em, gs, step), " zero" if zero else "")
    d = K.adam_inputs(n, zero)
    ref, S = K.adam_reference(d, em, gs, step)
    g, bufs = _inp(d["g"]), _adam_bufs(d, ema)
    assert all(b.ptr % 16 == 0 for b in bufs) and g.ptr % 16 == 0
    _twice(lambda: _adam_call(bufs, g, n, em, gs, step, None), bufs, what)
    _adam_verify(bufs, ref, S, what)
    _frozen((g,), what)
    RAN.update([("adam tail", K.adam_tail(n)), ("adam ema", bool(ema)), ("adam eps_mode", em), ("adam grad_scale", gs), ("adam step", step)])
    if zero:
        RAN.add(("adam", "denom = eps"))


@pytest.mark.parametrize("n,ema,em,gs", K.ADAM_DEV_ROWS, ids=IDS)
def test_adam_step_counts_on_the_device(n, ema, em, gs):
    """three consecutive calls through dev_state, starting from zeros: the count reads 1, 2, 3, the bias corrections are the fp64
    ones rounded to fp32 (to one fp32 step: the device forms them in double from its own pow), and each step's update is the
    reference's for that step.  The whole sequence a second time gives the same bits"""
    what = "adam dev_state %s" % ((n, ema, em, gs),)
    d = K.adam_inputs(n)
    g, bufs = _inp(d["g"]), _adam_bufs(d, ema)
    state = _out((3,), torch.zeros(3))
    seen = []
    for rep in range(2):
        state.reset()
        for step in (1, 2, 3):
            for b in bufs:
                b.reset()
            _sync(_adam_call(bufs, g, n, em, gs, 0, state), what + " step %d" % step)      # (the `step` argument is ignored)
            assert state.problems() == [], state.problems()
            st = state.view.cpu().double()
            ss, isb = K.adam_corrections(step, em)
            assert st[0].item() == step, "%s: the device counter reads %r after call %d" % (what, st[0].item(), step)
            assert abs(st[1].item() - ss) <= 2.0 ** -23 * ss and abs(st[2].item() - isb) <= 2.0 ** -23 * isb, (what, st.tolist(), ss, isb)
            if rep == 0:
                ref, S = K.adam_reference(d, em, gs, step)
                _adam_verify(bufs, ref, S, what + " step %d" % step)
                seen.append([b.view.clone() for b in bufs] + [state.view.clone()])
            else:
                for a, b in zip(seen[step - 1], bufs + [state]):
                    _same_bits(a, b.view, what + " step %d, second run" % step)
    _frozen((g,), what)
    RAN.update([("adam dev_state", bool(ema), em), ("adam dev_state tail", K.adam_tail(n))])


def test_adam_step_rejects_a_misaligned_bucket_before_it_counts():
    """p one float off 16-byte alignment, with a device counter: MOGAN_ERR_SHAPE, and neither the counter nor p / m / v / ema moved
    (the check used to stand behind the launch that advances dev_state[0])"""
    n = 16
    d = K.adam_inputs(n + 1)
    g = _inp(d["g"])
    bufs = [mg.Guarded((n + 1,), (slice(1, None),), DEV, base=d[k][1:]) for k in ("p", "m", "v", "ema")]
    state = _out((3,), torch.tensor([4.0, 0.25, 1.5]))
    assert bufs[0].ptr % 16 == 4
    for which in range(4):                    # p, m, v, ema misaligned in turn, the others aligned
        al = [_out((n,), d[k][:n]) for k in ("p", "m", "v", "ema")]
        use = [bufs[k] if k == which else al[k] for k in range(4)]
        rc = _adam_call(use, g, n, 0, 1.0, 0, state)
        torch.cuda.synchronize()
        assert rc == -1, "misaligned %s: return code %d" % (("p", "m", "v", "ema")[which], rc)
        assert state.untouched(), "a rejected call advanced the device counter: %s" % state.view.tolist()
        assert all(b.untouched() for b in use)
    _frozen((g,), "adam rejection")
    RAN.add(("adam", "rejects before it counts"))


# ------------------------------------------------------------------------------------------------------------------ chain
def test_chain_words_and_sentence_losses_to_the_image_gradients():
    """words_fwd -> ce_fwd -> ce_bwd -> words_bwd with the two mogan_bmm calls the header names for dctx, and sent_fwd -> ce_fwd ->
    ce_bwd -> sent_bwd, each kernel fed by the one before it: dctx and dcnn against fp64 autograd of 1.3 w0 + 0.7 w1 + 2 s0 + 0.5 s1
    (the figure of tests/test_kernels_gpu.py for these gradients, loss_cases.REL)"""
    B, C, S_, T_ = K.CHAIN_ROW[0], K.CHAIN_ROW[2], K.CHAIN_ROW[3], K.CHAIN_ROW[4]
    feat, words, lens, _ = K.words_inputs(B, B, C, S_, T_, "ragged")
    code, sent = K.T("chain.code", (B, C)), K.T("chain.sent", (B, C))
    n = lens.long().tolist()
    fd, cd = feat.double().requires_grad_(True), code.double().requires_grad_(True)
    ocfg = O.Cfg(words_num=T_, gamma1=G1, gamma2=G2, gamma3=G3)
    w0, w1, _ = O.words_loss(fd.reshape(B, C, S_, 1), torch.nan_to_num(words).double(), n, ocfg)
    s0, s1 = O.sent_loss(cd, sent.double(), ocfg)
    (1.3 * w0 + 0.7 * w1 + 2.0 * s0 + 0.5 * s1).backward()
    ctx, wd, ln, lab = _inp(feat), _inp(words), _inp(lens), _inp(torch.arange(B, dtype=torch.int64))
    dims = (B, B, C, S_, T_)
    sim, a1, a2, wc = outs = _words_outs(*dims)
    wt = _out((C, B, T_))
    _sync(_words_fwd(ctx, wd, ln, dims, outs, wt), "chain words_fwd")
    ce = [_out((B, B)), _out((B, B)), _out((2 * B,)), _out((2,))]
    _sync(_ce_fwd(sim, lab, None, B, ce), "chain ce_fwd")
    g = [_scalar(v) for v in (1.3, 0.7, 2.0, 0.5)]
    dsim, dwc, dst = _out((B, B)), _out((B, C, B, T_)), _out((B, B, T_, S_))
    _sync(L().mogan_damsm_ce_bwd(ce[0].ptr, ce[1].ptr, lab.ptr, g[0].ptr, g[1].ptr, B, B, dsim.ptr, lib.stream_ptr()), "chain ce_bwd")
    _sync(L().mogan_damsm_words_bwd(ctx.ptr, wd.ptr, ln.ptr, a1.ptr, a2.ptr, wc.ptr, dsim.ptr, B, B, C, S_, T_, G1, G2, G3, dwc.ptr, dst.ptr,
                                    lib.stream_ptr()), "chain words_bwd")
    dctx = _out((B, C, S_))
    ops.bmm_raw(dwc.view.view(B, C, B * T_), a2.view.view(B, B * T_, S_), dctx.view)
    ops.bmm_raw(wt.view.view(1, C, B * T_).expand(B, C, B * T_), dst.view.view(B, B * T_, S_), dctx.view, accumulate=True)
    cnn, rnn = _inp(code), _inp(sent)
    ssim, ce2, dss, dcnn = _out((B, B)), [_out((B, B)), _out((B, B)), _out((2 * B,)), _out((2,))], _out((B, B)), _out((B, C))
    _sync(L().mogan_damsm_sent_fwd(cnn.ptr, rnn.ptr, B, B, C, G3, 1e-8, ssim.ptr, lib.stream_ptr()), "chain sent_fwd")
    _sync(_ce_fwd(ssim, lab, None, B, ce2), "chain ce_fwd (sentence)")
    _sync(L().mogan_damsm_ce_bwd(ce2[0].ptr, ce2[1].ptr, lab.ptr, g[2].ptr, g[3].ptr, B, B, dss.ptr, lib.stream_ptr()), "chain ce_bwd (sentence)")
    _sync(L().mogan_damsm_sent_bwd(cnn.ptr, rnn.ptr, dss.ptr, B, B, C, G3, 1e-8, dcnn.ptr, lib.stream_ptr()), "chain sent_bwd")
    for gd in outs + [wt, dsim, dwc, dst, dctx, ssim, dss, dcnn] + ce + ce2:
        assert gd.problems() == [], gd.problems()
    for got, want, k in ((ce[3].view[0], w0, "w0"), (ce[3].view[1], w1, "w1"), (ce2[3].view[0], s0, "s0"), (ce2[3].view[1], s1, "s1")):
        r = abs(float(got) - float(want.detach())) / abs(float(want.detach()))
        print("chain %s: relative error %.3e" % (k, r))
        assert r <= 2e-5, (k, r)                          # (the rtol tests/test_kernels_gpu.py holds these four scalars to)
    for got, want, k in ((dctx, fd.grad, "dctx"), (dcnn, cd.grad, "dcnn")):
        r = rel_l2(got.view, want.reshape(got.view.shape))
        print("chain %s: rel-L2 %.3e" % (k, r))
        assert r <= K.REL["dcnn"], (k, r)
    _frozen([ctx, wd, ln, lab, cnn, rnn] + g, "chain")
    RAN.add(("chain",))


# ----------------------------------------------------------------------------------------------------------------- census
def test_census_of_what_ran():
    for k, v in sorted(FIG.items()):
        print("%-9s largest err / bound %.3f" % (k, v))
    want = {("head", r[:3], r[3]) for r in HEAD_CALLS} | {("head", "saturated")}
    want |= {("head NULL", k) for k in ("dx", "dw", "db", "all")} | {("head accumulate", a) for a in (0, 1)}
    want |= {("elem", k, n) for k in ("bce", "kl") for n in K.ELEM_N} | {("elem ends mid-wave", b) for b in (True, False)}
    want |= {("words TT", tt, f) for tt in (8, 12, 16, 24, 32) for f in ("full", "part")}
    want |= {("words channel loop", t) for t in ("C < 8", "eights and tail", "no second prefetch", "second prefetch")}
    want |= {("words S fwd", k) for k in ("registers", "loop")} | {("words S bwd", k) for k in ("one region", "two regions")}
    want |= {("words lens", k) for k in K.LENS_KINDS} | {("words lens clamp", k) for k in ("zero", "above", "negative", "one", "ragged")}
    want |= {("words non-square", k) for k in ("B < Bc", "B > Bc")} | {("words padding", "NaN against zero"), ("words", "LDS edge")}
    want |= {("ce",) + r for r in K.CE_ROWS} | {("ce g", a, b) for a in (True, False) for b in (True, False)}
    want |= {("sent", r[:3], r[3], r[4]) for r in K.SENT_ROWS} | {("scalar", n) for n in K.SUM_N}
    want |= {("adam tail", t) for t in range(4)} | {("adam ema", b) for b in (True, False)} | {("adam eps_mode", m) for m in (0, 1)}
    want |= {("adam grad_scale", s) for s in (1.0, 0.125)} | {("adam step", s) for s in K.ADAM_STEPS}
    want |= {("adam", "denom = eps"), ("adam", "rejects before it counts"), ("chain",)}
    want |= {("adam dev_state", e, m) for e in (True, False) for m in (0, 1)} | {("adam dev_state tail", t) for t in (1, 3)}
    assert want <= RAN, "never ran: %s" % sorted(map(str, want - RAN))
    assert set(FIG) == set(K.TOL), "no figure for %s" % sorted(set(K.TOL) - set(FIG))
    assert all(v <= 1.0 for v in FIG.values()), FIG
