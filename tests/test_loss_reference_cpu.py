"""The references and tolerances of tests/loss_cases.py, checked without a GPU (what tests/test_pathway_reference_cpu.py is to
tests/pathway_cases.py):
  * where the package's fp64 oracle states the operation -- O.words_loss, O.sent_loss, O.bce, O.kl_loss, O.adam_step -- the new
    reference equals it to 1e-12 relative on the square, in-range rows; elsewhere it equals torch's own fp64 operation or autograd
    (F.linear + sigmoid, binary_cross_entropy_with_logits, softmax / cross_entropy, the cosine's gradient);
  * TOL comes from fp32 CPU evaluations -- the numpy restatements of the kernels and, where torch has the operation, torch's own
    fp32 evaluation -- measured as max err / S over every row; the recorded constants are 4 x that (the project's margin for the
    GPU's different but equally valid contraction and summation order) and at most the project's ceiling; S = 0 implies err = 0;
    both fp32 evaluations stay within half of the whole-tensor figures REL;
  * the tables reach every path, by the predicates restated in loss_cases.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_cases as K
from oracle import attngan_oracle as O

FIG = {}            # kind -> {evaluation: largest err / S}
IDS = lambda v: str(v).replace(" ", "")
F64, F32 = torch.float64, torch.float32


def _ratio(kind, name, got, ref, S, rel=True):
    """records max err / S of one fp32 evaluation (what exceeds FLOOR: loss_cases.bound) and holds it to TOL / 4 and REL / 2"""
    got = torch.as_tensor(got).double().reshape(ref.shape)
    ref, S = ref.double(), S.double()
    inf = torch.isinf(ref)
    assert bool((got[inf] == ref[inf]).all()), "%s %s: another value where the reference is infinite" % (name, kind)
    err = torch.where(inf, torch.zeros_like(ref), (got - ref).abs())
    assert bool(torch.isfinite(err).all()), "%s %s: not finite" % (name, kind)
    assert bool((err[S == 0] == 0).all()), "%s %s: an error where S is 0" % (name, kind)
    r = float(((err - K.FLOOR).clamp_min(0) / S.clamp_min(1e-300))[S > 0].max()) if bool((S > 0).any()) else 0.0
    f = FIG.setdefault(kind, {})
    f[name] = max(f.get(name, 0.0), r)
    assert r <= K.TOL[kind] / 4, "%s %s: %.3e (%.2f x 2^-24) > TOL / 4 = %.2e" % (name, kind, r, r / K.EPS32, K.TOL[kind] / 4)
    fig = K.figure(kind, torch.where(inf, torch.zeros_like(got), got), torch.where(inf, torch.zeros_like(ref), ref))
    if rel:
        assert fig <= K.REL[kind] / 2, "%s %s: whole-tensor figure %.2e > REL / 2 = %.1e" % (name, kind, fig, K.REL[kind] / 2)
    else:           # (an exempted call, loss_cases.words_rel_applies: the exemption is needed)
        assert fig > K.REL[kind], "%s %s: whole-tensor figure %.2e on a call that is exempted from it" % (name, kind, fig)
    return r


def _equal(a, b, what, rel=1e-12):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    if a.numel() == 0:
        return
    e = float((a - b.reshape(a.shape)).abs().max())
    assert e <= rel * (float(b.abs().max()) + 1e-300), "%s: %.3e against a size of %.3e" % (what, e, float(b.abs().max()))


# ---------------------------------------------------------------------------------------------------------- logits head
HEAD_CALLS = [r + (True,) for r in K.HEAD_ROWS] + [K.HEAD_ROWS[-1] + (False,)]


@pytest.mark.parametrize("B,Kd,Cout,with_bias", HEAD_CALLS, ids=IDS)
def test_head_formulas_equal_torch_and_fp32_evaluations_stay_inside(B, Kd, Cout, with_bias):
    d = K.head_case(B, Kd, Cout, with_bias)
    ref, S = d["ref"], d["S"]

    def torch_eval(dtype, from_p_in):
        x, w = (d[k].to(dtype).clone().requires_grad_(True) for k in ("x", "w"))
        b = d["bias"].to(dtype).clone().requires_grad_(True) if with_bias else None
        p = torch.sigmoid(F.linear(x, w, b))
        if not from_p_in:
            p.backward(d["dp"].to(dtype))
            return {"p": p.detach(), "dx": x.grad, "dw": w.grad, "db": b.grad if with_bias else None}
        pin = d["p_in"].to(dtype)
        dz = d["dp"].to(dtype) * pin * (1 - pin)
        dw, db = dz.t() @ x.detach(), dz.sum(0)
        return {"p": p.detach(), "dx": dz @ w.detach(), "dw": dw, "db": db, "dw+": d["base_w"].to(dtype) + dw,
                "db+": d["base_b"].to(dtype) + db}
    w64 = torch_eval(F64, False)
    _equal(ref["p"], w64["p"], "p")
    if (B, Kd, Cout) != K.HEAD_SATURATED:          # (the backward runs from the ROUNDED p: equal to autograd to fp32 rounding)
        for k in ("dx", "dw") + (("db",) if with_bias else ()):
            _equal(ref[k], w64[k], k, rel=4e-7)
    else:
        assert d["p_in"][0, 0] == 1.0 and d["p_in"][1, 0] == 0.0 and abs(float(d["z"][0, 0])) > 100 and float(d["z"][1, 0]) < -100
        assert float(S["dx"][:2].max()) == 0 and float(ref["dx"][:2].abs().max()) == 0
    got = K.restate_head_fp32(d["x"].numpy(), d["w"].numpy(), d["bias"].numpy() if with_bias else None, d["dp"].numpy(),
                              d["p_in"].numpy(), d["base_w"].numpy(), d["base_b"].numpy())
    if (B, Kd, Cout) == K.HEAD_SATURATED:
        assert got["p"][0, 0] == 1.0 and got["p"][1, 0] == 0.0
    t32 = torch_eval(F32, True)
    for k, kind in (("p", "p"), ("dx", "head_dx"), ("dw", "head_dw"), ("db", "head_db"), ("dw+", "head_dw"), ("db+", "head_db")):
        _ratio(kind, "restatement", got[k], ref[k], S[k])
        _ratio(kind, "torch fp32", t32[k], ref[k], S[k])


# ---------------------------------------------------------------------------------------------------- elementwise losses
ELEM_CALLS = [(n, t, w, a) for n in K.ELEM_N for t in K.TARGETS for w in K.WEIGHTS for a in (0, 1)]


def _elem_row(n, target, weight, acc):
    inp = K.elem_inputs(n)
    t = float(np.float32(target))
    bce, bcel, kl = K.bce_case(n, target, weight, acc), K.bcel_case(n, target, weight, acc), K.kl_case(n)
    base = K.BASE if acc else 0.0

    def torch_eval(dtype):
        p, x, mu, lv = (inp[k].to(dtype).clone().requires_grad_(True) for k in ("p", "x", "mu", "lv"))
        eps, dc = inp["eps"].to(dtype), inp["dc"].to(dtype)
        tt = torch.full((n,), t, dtype=dtype)
        out = {}
        l = O.bce(p, tt)
        (l * K.GOUT * weight).backward()
        out["bce"], out["bce_dp"] = (base + weight * l.detach()).reshape(1), p.grad
        l = F.binary_cross_entropy_with_logits(x, tt)
        (l * K.GOUT * weight).backward()
        out["bcel"], out["bcel_dx"] = (base + weight * l.detach()).reshape(1), x.grad
        l = O.kl_loss(mu, lv)
        (l * K.GOUT).backward()
        out["kl"], out["kl_dmu"], out["kl_dlv"] = l.detach().reshape(1), mu.grad.clone(), lv.grad.clone()
        mu.grad = lv.grad = None
        c = eps * torch.exp(0.5 * lv) + mu
        c.backward(dc)
        out["c"], out["rp_dlv"], out["rp_dmu"] = c.detach(), lv.grad, mu.grad
        return out
    w64 = torch_eval(F64)
    inr = (inp["p"].double() * (1 - inp["p"].double())) > 1e-11         # torch clamps the backward at its own fp64 1e-12
    for k, c in (("bce", bce), ("bcel", bcel), ("bcel_dx", bcel), ("kl", kl), ("kl_dmu", kl), ("kl_dlv", kl), ("c", kl), ("rp_dlv", kl)):
        _equal(c["ref"][k], w64[k], "%s n=%d" % (k, n))
    _equal(bce["ref"]["bce_dp"][inr], w64["bce_dp"][inr], "bce_dp")
    assert torch.equal(w64["rp_dmu"], inp["dc"].double())
    got = K.restate_elem_fp32(n, target, weight, acc)
    t32 = torch_eval(F32)
    for k, c in (("bce", bce), ("bce_dp", bce), ("bcel", bcel), ("bcel_dx", bcel), ("kl", kl), ("kl_dmu", kl), ("kl_dlv", kl), ("c", kl),
                 ("rp_dlv", kl)):
        _ratio(k, "restatement", got[k], c["ref"][k], c["S"][k])
        _ratio(k, "torch fp32", t32[k], c["ref"][k], c["S"][k])


@pytest.mark.parametrize("n", K.ELEM_N)
def test_elementwise_losses_equal_the_oracle_and_fp32_evaluations_stay_inside(n):
    for c in ELEM_CALLS:
        if c[0] == n:
            _elem_row(*c)
    p, x, lv = (K.elem_inputs(n)[k] for k in ("p", "x", "lv"))
    k = min(n, len(K.BCE_SPECIAL))
    assert p[:k].tolist() == [float(np.float32(v)) for v in K.BCE_SPECIAL[:k]] and float(lv.abs().max()) <= 10
    if n >= 9:
        assert x[:9].tolist() == [float(np.float32(v)) for v in K.BCEL_SPECIAL] and lv[1:5].tolist() == list(K.LV_SPECIAL) and bool(torch.signbit(lv[2]))


# ------------------------------------------------------------------------------------------------------------------ words
def _words_row(row):
    B, Bc, C, S_, T_, kind = row
    d = K.words_case(*row)
    ref, S = d["ref"], d["S"]
    n = d["lens"].long().clamp(0, T_)
    pad = torch.arange(T_)[None] >= n[:, None]                                          # (Bc, T)
    # exact zeros behind each caption's end, with nothing to lose; a caption of length 0 has sim = -inf
    for k, where in (("a1", pad[None, :, None, :]), ("a2", pad[None, :, :, None]), ("wc", pad[None, None]), ("dwc", pad[None, None]),
                     ("dscore_t", pad[None, :, :, None])):
        m = where.expand_as(ref[k])
        assert float(ref[k][m].abs().max() if bool(m.any()) else 0.0) == 0 and float(S[k][m].max() if bool(m.any()) else 0.0) == 0, k
    assert bool((ref["wt"].permute(1, 0, 2)[pad[:, None, :].expand(Bc, C, T_)] == 0).all())
    assert bool(torch.isinf(ref["sim"][:, n == 0]).all()) and bool(torch.isfinite(ref["sim"][:, n > 0]).all())
    if bool(pad.any()):
        assert bool(torch.isnan(d["words"][pad[:, None, :].expand(Bc, C, T_)]).all())
    if B == Bc and kind in ("full", "ragged"):          # the oracle: both cross-entropies of sim and the attention maps
        x = d["ctx"].double().clone().requires_grad_(True)
        w0, w1, att = O.words_loss(x.reshape(B, C, S_, 1), torch.nan_to_num(d["words"]).double(), n.tolist(),
                                   O.Cfg(words_num=T_, gamma1=K.GAMMAS[0], gamma2=K.GAMMAS[1], gamma3=K.GAMMAS[2]))
        ce, _ = K.ce_reference(ref["sim"], torch.arange(B), None, prow_in="exact", pcol_in="exact")
        _equal(ce["out2"], torch.stack([w0, w1]).detach(), "words losses %s" % (row,))
        for i in range(B):
            _equal(ref["a2"][i, i, :int(n[i])], att[i].detach().reshape(int(n[i]), S_), "attention map %d" % i)
        # the backward's formulas, chained as the header chains them, against autograd of 1.3 w0 + 0.7 w1 (the saved tensors and
        # dsim travel as fp32: equal to fp32 rounding)
        (1.3 * w0 + 0.7 * w1).backward()
        ex, eS = K.words_reference(d["ctx"], d["words"], d["lens"], ce[("dsim", 1.3, 0.7)].float())
        dctx = torch.einsum("bcit,bits->bcs", ex["dwc"], ref["a2"]) + torch.einsum("cit,bits->bcs", ex["wt"], ex["dscore_t"])
        # (against the terms that enter, S: at C = 1 the cosines are +-1 and the terms of dwc cancel to nothing)
        size = torch.einsum("bcit,bits->bcs", eS["dwc"], ref["a2"]) + torch.einsum("cit,bits->bcs", ex["wt"].abs(), eS["dscore_t"])
        e = float((dctx - x.grad).abs().max())
        assert e <= 2e-7 * float(size.max()), "dctx %s: %.3e against terms of %.3e" % (row, e, float(size.max()))
    sv = d["saved"]
    got = K.restate_words_fp32(d["ctx"].numpy(), d["words"].numpy(), d["lens"].numpy(), d["dsim"].numpy(), sv["a1"].numpy(),
                               sv["a2"].numpy(), sv["wc"].numpy())
    for k in ("sim", "a1", "a2", "wc", "dwc", "dscore_t"):
        _ratio(k, "restatement", got[k], ref[k], S[k], rel=K.words_rel_applies(C) or k not in ("dwc", "dscore_t"))
    t32 = K.words_forward(d["ctx"], d["words"], d["lens"], dtype=F32)
    for k in ("sim", "a1", "a2", "wc"):
        _ratio(k, "torch fp32", t32[k], ref[k], S[k])


@pytest.mark.parametrize("row", K.WORDS_ROWS, ids=IDS)
def test_words_formulas_equal_the_oracle_and_fp32_evaluations_stay_inside(row):
    _words_row(row)


# -------------------------------------------------------------------------------------------------------- cross-entropies
def _ce_row(R, mk, lk):
    d = K.ce_case(R, mk, lk)
    ref, S = d["ref"], d["S"]
    lab = d["lab"].clamp(0, R - 1)
    off = torch.zeros(R, R, dtype=torch.bool) if d["mask"] is None else d["mask"].bool()
    assert not bool(off[torch.arange(R), lab].any()) and not bool(off[lab, torch.arange(R)].any())
    if d["mask"] is not None:
        assert bool(torch.isnan(d["sim"][off]).all()) and (R < 3 or bool(off.any()))
        assert float(ref["prow"][off].abs().max() if bool(off.any()) else 0.0) == 0

    def torch_eval(dtype, g0, g1):
        s = torch.where(off, torch.zeros((), dtype=dtype), d["sim"].to(dtype)).clone().requires_grad_(True)
        sm = s.masked_fill(off, -float("inf"))
        l0, l1 = F.cross_entropy(sm, lab), F.cross_entropy(sm.t(), lab)
        if g0 is not None or g1 is not None:
            ((g0 or 0.0) * l0 + (g1 or 0.0) * l1).backward()
        return {"prow": torch.softmax(sm, 1).detach(), "pcol": torch.softmax(sm, 0).detach(), "out2": torch.stack([l0, l1]).detach(),
                "dsim": s.grad if s.grad is not None else torch.zeros(R, R, dtype=dtype)}
    ex, _ = K.ce_reference(d["sim"], d["lab"], d["mask"], prow_in=ref["prow"], pcol_in=ref["pcol"])
    for g0, g1 in K.CE_G:
        w64 = torch_eval(F64, g0, g1)
        _equal(ex[("dsim", g0, g1)], w64["dsim"], "dsim %s" % ((g0, g1),))
    for k in ("prow", "pcol", "out2"):
        _equal(ref[k], w64[k], k)
    got = K.restate_ce_fp32(d["sim"].numpy(), d["lab"].numpy(), None if d["mask"] is None else d["mask"].numpy(),
                            d["prow_in"].numpy(), d["pcol_in"].numpy())
    t32 = torch_eval(F32, None, None)
    for k, kind in (("prow", "prow"), ("pcol", "pcol"), ("nll", "ce"), ("out2", "ce")):
        _ratio(kind, "restatement", got[k], ref[k], S[k])
        if k != "nll":
            _ratio(kind, "torch fp32", t32[k], ref[k], S[k])
    for g in K.CE_G:
        _ratio("ce_dsim", "restatement", got[("dsim",) + g], ref[("dsim",) + g], S[("dsim",) + g])
    assert float(S[("dsim", None, None)].max()) == 0


@pytest.mark.parametrize("R,mk,lk", K.CE_ROWS, ids=IDS)
def test_cross_entropies_equal_torch_and_fp32_evaluations_stay_inside(R, mk, lk):
    _ce_row(R, mk, lk)


# ---------------------------------------------------------------------------------------------------------- sentence loss
def _sent_row(B, Bc, C, kind, eps):
    d = K.sent_case(B, Bc, C, kind, eps)
    ref, S = d["ref"], d["S"]
    assert ref["margin"] > 1e-3, "a pair of the table sits on the clamp: |den - eps| / eps = %.2e" % ref["margin"]
    g3 = K.GAMMAS[2]

    def torch_eval(dtype):
        x, r = d["cnn"].to(dtype).clone().requires_grad_(True), d["rnn"].to(dtype)
        n0, n1 = x.norm(2, 1, keepdim=True), r.norm(2, 1, keepdim=True)
        s = x @ r.t() / (n0 @ n1.t()).clamp(min=float(np.float32(eps))) * g3
        s.backward(d["dsim"].to(dtype))
        return {"ssim": s.detach(), "dcnn": x.grad}
    w64 = torch_eval(F64)
    _equal(ref["ssim"], w64["ssim"], "sim")
    _equal(ref["dcnn"], w64["dcnn"], "dcnn")
    if kind == "tiny":          # the clamped branch: the gradient is g / eps on the first term only
        assert bool(ref["clamped"][1].all()) and not bool(ref["clamped"][0].any())
        _equal(ref["dcnn"][1], (d["dsim"][1].double() * g3 / float(np.float32(eps))) @ d["rnn"].double(), "clamped dcnn")
    if kind == "zero":
        assert float(ref["ssim"][0].abs().max()) == 0 and float(S["ssim"][0].max()) == 0
    if B == Bc and kind == "plain" and eps == 1e-8:
        s0, s1 = O.sent_loss(d["cnn"].double(), d["rnn"].double(), O.Cfg(gamma3=g3))
        ce, _ = K.ce_reference(ref["ssim"], torch.arange(B), None)
        _equal(ce["out2"], torch.stack([s0, s1]), "sentence losses")
    got = K.restate_sent_fp32(d["cnn"].numpy(), d["rnn"].numpy(), d["dsim"].numpy(), eps)
    t32 = torch_eval(F32)
    for k in ("ssim", "dcnn"):
        _ratio(k, "restatement", got[k], ref[k], S[k])
        _ratio(k, "torch fp32", t32[k], ref[k], S[k])


@pytest.mark.parametrize("B,Bc,C,kind,eps", K.SENT_ROWS, ids=IDS)
def test_sentence_similarity_equals_the_oracle_and_fp32_evaluations_stay_inside(B, Bc, C, kind, eps):
    _sent_row(B, Bc, C, kind, eps)


# ---------------------------------------------------------------------------------------------------- scalar sums, adam
def _sum_row(n):
    d = K.sum_case(n)
    _equal(d["ref"], (d["w"].double() * d["v"].double()).sum().reshape(1), "sum")
    _ratio("sum", "restatement", K.restate_sum_fp32(d["v"].numpy(), d["w"].numpy()), d["ref"], d["S"])
    _ratio("sum", "torch fp32", (d["w"] * d["v"]).sum().reshape(1), d["ref"], d["S"])


def test_scalar_sum():
    for n in K.SUM_N:
        _sum_row(n)
    assert 0.0 in K.SUM_W and min(K.SUM_W) < 0 and K.SUM_N == tuple(range(1, 9))


def _adam_row(n, ema, em, gs, step, zero=False):
    d = K.adam_inputs(n, zero)
    ref, S = K.adam_reference(d, em, gs, step)

    def oracle(dtype, as_given):
        # (as_given: python's own hyper-parameters, what the reference's trainer passes; else the fp32 values the entry receives --
        # 1 - fp32(0.999) is not fp32(0.001), and an fp32 evaluation is held to the function the entry computes)
        h = K._hyper(as_given)
        net = {"w": d["p"].to(dtype).clone().requires_grad_(True)}
        net["w"].grad = (d["g"].to(dtype) * gs)
        st = {"step": step - 1, "m": {"w": d["m"].to(dtype).clone()}, "v": {"w": d["v"].to(dtype).clone()}}
        O.adam_step(net, st, h["lr"], h["beta1"], h["beta2"], h["eps"], eps_mode="torch2" if em == 0 else "torch041")
        e = d["ema"].to(dtype).clone().mul_(h["ema_decay"]).add_(net["w"].detach(), alpha=1 - h["ema_decay"])
        return {"adam_p": net["w"].detach(), "adam_m": st["m"]["w"], "adam_v": st["v"]["w"], "adam_ema": e}
    w64 = oracle(F64, True)
    ex, _ = K.adam_reference(d, em, gs, step, as_given=True)
    for k in ref:
        _equal(ex[k], w64[k], "%s %s" % (k, (n, ema, em, gs, step)))
    got = K.restate_adam_fp32(d, em, gs, step)
    t32 = oracle(F32, False)
    for k in ref:
        _ratio(k, "restatement", got[k], ref[k], S[k])
        _ratio(k, "torch fp32", t32[k], ref[k], S[k])
    if zero:
        assert float(ref["adam_v"].abs().max()) == 0 and float(S["adam_v"].max()) == 0


def test_adam_equals_the_oracle_and_fp32_evaluations_stay_inside():
    for row in K.ADAM_ROWS:
        _adam_row(*row)
    _adam_row(*K.ADAM_ZERO_ROW, zero=True)
    for n, ema, em, gs in K.ADAM_DEV_ROWS:          # the three steps the device counter takes
        for step in (1, 2, 3):
            _adam_row(n, ema, em, gs, step)


# ----------------------------------------------------------------------------------------------- tolerances and coverage
def test_tolerances_come_from_the_fp32_evaluations():
    """the figures over every row (measured here, or by the tests above where they ran): the recorded ones are what was
    measured, TOL is 4 x that and under the ceiling"""
    for c in HEAD_CALLS:
        test_head_formulas_equal_torch_and_fp32_evaluations_stay_inside(*c)
    for c in ELEM_CALLS:
        _elem_row(*c)
    for row in K.WORDS_ROWS:
        _words_row(row)
    for c in K.CE_ROWS:
        _ce_row(*c)
    for c in K.SENT_ROWS:
        _sent_row(*c)
    test_scalar_sum()
    test_adam_equals_the_oracle_and_fp32_evaluations_stay_inside()
    assert set(FIG) == set(K.TOL) == set(K.MEASURED) == set(K.REL)
    bad = []
    for kind, f in sorted(FIG.items()):
        print("%-9s %s  -> MEASURED %.2f, TOL %.2e (%.2f x 2^-24)" % (
            kind, "  ".join("%s %.3f" % (n, v / K.EPS32) for n, v in sorted(f.items())), K.MEASURED_UNITS[kind], K.TOL[kind],
            K.TOL[kind] / K.EPS32))
        worst = max(f.values())
        ok = K.TOL[kind] <= K.TOL_CEILING and K.MEASURED[kind] >= worst and K.TOL[kind] == min(4 * K.MEASURED[kind], K.TOL_CEILING)
        # the recorded figure is the measured one, rounded up to the digits recorded (with pathway_cases' allowance for a torch
        # build whose fp32 sums run in another order)
        ok = ok and K.MEASURED[kind] <= 1.25 * worst + 0.02 * K.EPS32
        if not ok:
            bad.append("%s: recorded %.2f, measured %.3f" % (kind, K.MEASURED_UNITS[kind], worst / K.EPS32))
    assert not bad, bad


def test_the_tables_reach_every_path():
    rows = K.WORDS_ROWS
    Ts = {r[4] for r in rows}
    assert Ts >= {1, 8, 9, 12, 13, 16, 17, 24, 25, 32} and {K.words_tt(t) for t in Ts} == {8, 12, 16, 24, 32}
    for tt, below in ((8, None), (12, 8), (16, 12), (24, 16), (32, 24)):          # every instantiation full and one past the one below
        assert tt in Ts and (below is None or below + 1 in Ts) and K.words_tt(tt) == tt and (below is None or K.words_tt(below + 1) == tt)
    assert [K.words_tt(t) for t in (7, 12, 18)] == [8, 12, 24]
    loops = set().union(*(K.words_channel_loop(r[2]) for r in rows))
    assert loops == {"C < 8", "eights and tail", "no second prefetch", "second prefetch"}
    assert K.words_channel_loop(8) == {"no second prefetch"} and K.words_channel_loop(15) == {"eights and tail", "no second prefetch"}
    assert K.words_channel_loop(16) == {"second prefetch"} and K.words_channel_loop(7) == {"C < 8"}
    assert {r[2] for r in rows} >= {1, 7, 8, 15, 16, 23} and {r[3] for r in rows} >= {1, 63, 64, 65, 289, 320, 321, 640}
    assert {K.words_s_regime(r[3]) for r in rows} == {("registers", "one region"), ("loop", "two regions")}
    assert K.words_s_regime(320) == ("registers", "one region") and K.words_s_regime(321) == ("loop", "two regions")
    assert any(r[0] < r[1] for r in rows) and any(r[0] > r[1] for r in rows)
    assert {r[5] for r in rows} == set(K.LENS_KINDS)
    seen = {}
    for r in rows:
        for k, v in K.lens_clamps(K.words_lens(r[1], r[4], r[5]), r[4]).items():
            seen[k] = seen.get(k, False) or v
    assert all(seen[k] for k in ("zero", "above", "negative", "one", "ragged"))
    assert K.words_lens(3, 7, "over").tolist() == [10, -2, 6] and K.words_lens(3, 7, "zero").tolist() == [7, 4, 0]
    assert K.words_lens(2, 9, "ragged").tolist() == [9, 1] and sorted(K.words_lens(5, 7, "ragged").tolist(), reverse=True) == K.words_lens(5, 7, "ragged").tolist()
    # the LDS edge: exactly 64 KB, one channel more is refused (tests/test_loss_rejections_cpu.py)
    B, Bc, C, S_, T_, _ = K.WORDS_LDS_EDGE
    assert K.words_lds_bytes(C, S_, T_) == 65536 and K.words_lds_bytes(C + 1, S_, T_) > 65536
    assert all(K.words_lds_bytes(r[2], r[3], r[4]) <= 65536 for r in rows) and (2, 2, 256, 289, 12, "ragged") in rows
    assert K.words_lds_bytes(K.CHAIN_ROW[2], K.CHAIN_ROW[3], K.CHAIN_ROW[4]) <= 65536
    # cross-entropies
    assert {c[0] for c in K.CE_ROWS} == {1, 2, 5, 63, 64, 65, 256, 257} and {c[1] for c in K.CE_ROWS} == {None, "same"}
    assert {c[2] for c in K.CE_ROWS} == {"arange", "perm", "clamp"} and all(c[0] == 5 for c in K.CE_ROWS if c[2] == "clamp")
    lab = K.ce_labels(5, "clamp")
    assert lab.tolist() == [0, 5, 2, -1, 4] and lab.dtype == torch.int64
    assert any((K.ce_labels(R, "perm") != torch.arange(R)).any() for R in (5, 63))
    assert set(K.CE_G) == {(1.3, 0.7), (1.3, None), (None, 0.7), (None, None)}
    # sentence
    assert {r[:3] for r in K.SENT_ROWS} == set(K.SENT_SHAPES) and {r[4] for r in K.SENT_ROWS} == {1e-8, 0.5}
    assert {r[3] for r in K.SENT_ROWS} == {"plain", "tiny", "zero"} and (2, 9, 300) in K.SENT_SHAPES
    # head, elementwise, adam, sums
    assert K.HEAD_ROWS == [(1, 4, 1), (15, 32, 1), (5, 1028, 3), (16, 12288, 1), (3, 72, 4)] and K.HEAD_SATURATED in K.HEAD_ROWS
    assert K.ELEM_N == (1, 63, 64, 65, 255, 256, 257, 1600, 4099) and any(n % 64 for n in K.ELEM_N) and any(n > 256 and n % 256 for n in K.ELEM_N)
    assert {K.adam_tail(r[0]) for r in K.ADAM_ROWS} == {0, 1, 2, 3} and {r[0] for r in K.ADAM_ROWS} == set(K.ADAM_N)
    for n in K.ADAM_N:
        assert {r[1:4] for r in K.ADAM_ROWS if r[0] == n} == {(e, m, g) for e in (0, 1) for m in (0, 1) for g in (1.0, 0.125)}
    assert {r[4] for r in K.ADAM_ROWS} == {1, 2, 1000}
    assert {(r[1], r[2]) for r in K.ADAM_DEV_ROWS} == {(e, m) for e in (0, 1) for m in (0, 1)} and {K.adam_tail(r[0]) for r in K.ADAM_DEV_ROWS} == {1, 3}
