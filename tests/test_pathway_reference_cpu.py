"""The references and tolerances of tests/pathway_cases.py, checked without a GPU (what tests/test_bn_reference_cpu.py is to
tests/bn_cases.py):
  * the dense tent form equals F.affine_grid + F.grid_sample (bilinear, zeros) in fp64 on every transformer row, forward and
    autograd backward; the attention formulas equal bmm + masked_fill + softmax, the softmax formulas torch.softmax, the concat
    addressing the torch expression of test_kernels_gpu.test_cat_channels;
  * TOL comes from fp32 CPU evaluations -- the numpy restatements of the kernels and, where torch has the operation, torch's own
    fp32 evaluation -- measured as max err / S over every row; the recorded constants are 4 x that (conv_cases' margin for the
    GPU's different but equally valid contraction and summation order) and at most the project's ceiling; S = 0 implies err = 0;
  * bbox_to_theta's restatement against the formulas of miscc/utils.py in fp64;
  * the tables reach every path, by the predicates restated in pathway_cases.
"""
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pathway_cases as K

FIG = {}            # kind -> {evaluation: largest err / S}
IDS = lambda v: str(v).replace(" ", "")


def _ratio(kind, name, got, ref, S):
    got = torch.as_tensor(got).double().reshape(ref.shape)
    err = (got - ref).abs()
    assert bool((err[S == 0] == 0).all()), "%s %s: an error where S is 0" % (name, kind)
    r = float((err / S.clamp_min(1e-300))[S > 0].max()) if bool((S > 0).any()) else 0.0
    f = FIG.setdefault(kind, {})
    f[name] = max(f.get(name, 0.0), r)
    assert r <= K.TOL[kind] / 4, "%s %s: %.3e (%.2f x 2^-24) > TOL / 4 = %.2e" % (name, kind, r, r / K.EPS32, K.TOL[kind] / 4)
    return r


# ---------------------------------------------------------------------------------------------------------- transformer
def _torch_stn(x, theta, dy, shape, ac, xB, plane, tG, dtype):
    B, C, Hin, Win, Hout, Wout = shape
    th = theta[torch.from_numpy(K.theta_index(B, tG))].to(dtype).reshape(B, 2, 3)
    xl = x.to(dtype).clone().requires_grad_(True)
    xf = xl[:, :, None, None].expand(xB, C, Hin, Win) if plane else xl
    xs = xf.repeat(B // xB, 1, 1, 1)                    # sample b reads image b % xB
    with warnings.catch_warnings():                     # (torch warns about one-pixel grids with align_corners: they are rows here)
        warnings.simplefilter("ignore", UserWarning)
        grid = F.affine_grid(th, (B, C, Hout, Wout), align_corners=bool(ac))
    y = F.grid_sample(xs, grid, mode="bilinear", padding_mode="zeros", align_corners=bool(ac))
    y.backward(dy.to(dtype).reshape(y.shape))
    return {"y": y.detach().reshape(B, C, -1), "dx": xl.grad}


def _stn_row(row):
    B, C, Hin, Win, Hout, Wout, ac = row[:7]
    xB, plane, tG = row[7:] if len(row) > 7 else (B, 0, 0)
    d = K.stn_case(B, C, Hin, Win, Hout, Wout, ac, xB, plane, tG)
    want = _torch_stn(d["x"], d["theta"], d["dy"], row[:6], ac, xB, plane, tG, torch.float64)
    for k in ("y", "dx"):
        scale = float(d["S"][k].max()) + 1e-300
        e = float((d["ref"][k] - want[k].reshape(d["ref"][k].shape)).abs().max())
        assert e <= 1e-12 * scale, (k, e, scale)
    got = K.restate_stn_fp32(d["x"].numpy(), d["theta"].numpy(), d["dy"].numpy(), Hin, Win, Hout, Wout, ac, xB, bool(plane), tG)
    t32 = _torch_stn(d["x"], d["theta"], d["dy"], row[:6], ac, xB, plane, tG, torch.float32)
    rel = lambda a, k: float((torch.as_tensor(a).double().reshape(d["ref"][k].shape) - d["ref"][k]).norm() / (d["ref"][k].norm() + 1e-30))
    for k in ("y", "dx"):
        _ratio("stn_" + k, "restatement", got[k], d["ref"][k], d["S"][k])
        _ratio("stn_" + k, "torch fp32", t32[k], d["ref"][k], d["S"][k])
        # the whole-tensor figure the GPU module asserts is within reach of both fp32 evaluations on every call it is asked of --
        # with a factor 2 to spare, except on the 257-pixel source axis with align_corners (5.2e-6 on dx: within reach, without
        # the spare factor); on the one call it is not asked of, torch's own fp32 evaluation misses it
        figs = (rel(got[k], k), rel(t32[k], k))
        if K.stn_rel_applies(Hin, Win, ac):
            assert max(figs) <= K.REL["stn_" + k] / (2 if max(Hin, Win) <= 128 else 1), (k, figs)
        else:
            print("%s %s: rel-L2 of the restatement %.2e, of torch fp32 %.2e" % (row, k, *figs))
            assert min(figs) > K.REL["stn_" + k], (k, figs)
    # an absent object is exact zeros, with nothing to lose
    for b in range(B):
        if K.THETA_NAMES[K.theta_index(B, tG)[b] % K.NT].endswith("absent"):
            assert float(d["S"]["y"][b].max()) == 0 and float(d["ref"]["y"][b].abs().max()) == 0


@pytest.mark.parametrize("row", K.STN_ROWS + K.STN_EX_ROWS, ids=IDS)
def test_tent_form_equals_grid_sample_and_fp32_evaluations_stay_inside(row):
    _stn_row(row)


def test_bbox_to_theta_restatement():
    """against the formulas of miscc/utils.py:16-49 in fp64, to fp32 rounding; the absent object gives the documented matrices"""
    bb = np.array(K.BOXES, np.float32)
    th, thi = K.bbox_to_theta_fp32(bb)
    x, y, w, h = (bb[:, i].astype(np.float64) for i in range(4))
    want = np.stack([w, 0 * w, 2 * (x + w / 2) - 1, 0 * w, h, 2 * (y + h / 2) - 1], 1)
    wanti = np.stack([1 / w, 0 * w, (2 / w) * (0.5 - (x + w / 2)), 0 * w, 1 / h, (2 / h) * (0.5 - (y + h / 2))], 1)
    assert np.abs(th - want).max() <= 4 * K.EPS32 * 4 and (np.abs(thi - wanti) <= 8 * K.EPS32 * (np.abs(wanti) + 200)).all()
    assert thi[4].tolist() == [-1, 0, -4, 0, -1, -4] and th[4].tolist() == [-1, 0, -4, 0, -1, -4]
    # the table the GPU module compares bit for bit: one past a block, with inf and NaN patterns on both outputs
    bb = K.bbox_table()
    th, thi = K.bbox_to_theta_fp32(bb)
    assert bb.shape == (257, 4) and np.isinf(thi).any() and np.isnan(thi).any() and np.isnan(th).any() and np.isinf(th).any()
    fin = np.isfinite(bb).all(1) & (bb[:, 2] != 0) & (bb[:, 3] != 0)
    assert fin.sum() > 240 and np.isfinite(th[fin]).all()


# ------------------------------------------------------------------------------------------------------------ attention
ATTN_CALLS = [r + (m, g) for r in K.ATTN_ROWS for m in K.MASKS for g in (False, True)]


@pytest.mark.parametrize("B,idf,Q,T_,mk,with_dattn", ATTN_CALLS, ids=IDS)
def test_attention_formulas_equal_torch_and_fp32_evaluations_stay_inside(B, idf, Q, T_, mk, with_dattn):
    d = K.attn_case(B, idf, Q, T_, mk, with_dattn)
    ref, S = d["ref"], d["S"]
    assert ref["spread"] <= K.SPREAD
    if d["mask"] is not None:
        assert int((1 - d["mask"]).sum(1).min()) >= 1

    def torch_eval(dtype):
        h, src = (d[k].to(dtype).clone().requires_grad_(True) for k in ("h", "src"))
        sc = torch.bmm(h.transpose(1, 2), src).reshape(B * Q, T_)
        if d["mask"] is not None:
            rows = (torch.arange(B * Q) % B) if d["mode"] == 0 else (torch.arange(B * Q) // Q)
            sc = sc.masked_fill(d["mask"].bool()[rows], -float("inf"))
        att = torch.softmax(sc, 1).reshape(B, Q, T_).transpose(1, 2)
        wc = torch.bmm(src, att)
        loss = (wc * d["dwc"].to(dtype)).sum()
        if with_dattn:
            loss = loss + (att * d["dattn"].to(dtype)).sum()
        loss.backward()
        return {"attn": att.detach(), "wc": wc.detach(), "dh": h.grad}
    w64 = torch_eval(torch.float64)
    # the backward formulas at the exact p (autograd's), then at the rounded p the table uses
    rx, _ = K.attn_reference(d["h"], d["src"], d["mask"], d["mode"], d["dwc"], d["dattn"], attn_in=ref["attn"])
    for k, r in (("attn", ref), ("wc", ref), ("dh", rx)):
        assert float((r[k] - w64[k]).abs().max()) <= 1e-12 * (float(S[k].max()) + 1e-300), k
    got = K.restate_attn_fp32(d["h"].numpy(), d["src"].numpy(), None if d["mask"] is None else d["mask"].numpy(), d["mode"],
                              d["dwc"].numpy(), None if d["dattn"] is None else d["dattn"].numpy(), d["attn_in"].numpy())
    for k in ("attn", "wc", "dscore", "dh"):
        _ratio(k, "restatement", got[k], ref[k], S[k])
    t32 = torch_eval(torch.float32)
    for k in ("attn", "wc"):
        _ratio(k, "torch fp32", t32[k], ref[k], S[k])


# -------------------------------------------------------------------------------------------------------------- softmax
SM_CALLS = [r + (l, s) for r in K.SOFTMAX_ROWS for l in K.LENS for s in K.SCALES]


@pytest.mark.parametrize("outer,L,inner,with_lens,scale", SM_CALLS, ids=IDS)
def test_softmax_formulas_equal_torch_and_fp32_evaluations_stay_inside(outer, L, inner, with_lens, scale):
    d = K.softmax_case(outer, L, inner, with_lens, scale)
    ref, S = d["ref"], d["S"]
    n = torch.full((outer, inner), L) if d["lens"] is None else d["lens"].long().clamp(0, L).reshape(outer, inner)

    def torch_eval(dtype):
        x = d["x"].to(dtype).clone().requires_grad_(True)
        off = torch.arange(L).reshape(1, L, 1) >= n[:, None, :]
        y = torch.softmax((x * scale).masked_fill(off, -float("inf")), 1)
        y = torch.where(off | (n[:, None, :] == 0), torch.zeros_like(y), y)          # (an empty column: zeros, not NaN)
        y.backward(d["dy"].to(dtype))
        return {"y": y.detach(), "dx": torch.nan_to_num(x.grad)}
    w64 = torch_eval(torch.float64)
    rx, _ = K.softmax_reference(d["x"], d["lens"], scale, d["dy"], y_in=ref["y"])
    live = (n > 0)[:, None, :].expand_as(ref["y"])
    assert float((ref["y"] - w64["y"]).abs().max()) <= 1e-14
    assert float(((rx["dx"] - w64["dx"]) * live).abs().max()) <= 1e-12 * (float(S["dx"].max()) + 1e-300)
    assert float(ref["y"][~live].abs().max() if bool((~live).any()) else 0.0) == 0
    got = K.restate_softmax_fp32(d["x"].numpy(), None if d["lens"] is None else d["lens"].numpy(), scale, d["dy"].numpy(),
                                 d["y_in"].numpy())
    for k in ("y", "dx"):
        _ratio("sm_" + k, "restatement", got[k], ref[k], S[k])
    t32 = torch_eval(torch.float32)
    _ratio("sm_y", "torch fp32", t32["y"], ref["y"], S["y"])
    # torch's fp32 softmax backward from the same fp32 y the table hands to the kernel
    tdx = torch._softmax_backward_data(d["dy"], torch.where(torch.arange(L).reshape(1, L, 1) >= n[:, None, :], torch.zeros(()), d["y_in"]),
                                       1, torch.float32) * scale
    _ratio("sm_dx", "torch fp32", tdx, ref["dx"], S["dx"])


# --------------------------------------------------------------------------------------------------------------- concat
def _cat_torch(name, dtype):
    d = K.cat_case(name)
    HW, N, G = d["HW"], K.CAT_N, K.CAT_G
    leaves = [s.to(dtype).clone().requires_grad_(True) for s in d["srcs"]]
    parts = []
    for t, (kind, C) in zip(leaves, d["sources"]):
        parts.append({"full": lambda: t, "plane": lambda: t.view(N, C, 1).expand(N, C, HW), "rep": lambda: t.repeat(G, 1, 1),
                      "rep_plane": lambda: t.repeat(G, 1).view(N, C, 1).expand(N, C, HW),
                      "obj": lambda: t.transpose(0, 1).reshape(N, C, HW),
                      "obj_plane": lambda: t.transpose(0, 1).reshape(N, C, 1).expand(N, C, HW)}[kind]())
    y = torch.cat(parts, 1)
    y.backward(d["ddst"].to(dtype))
    return y.detach(), [t.grad for t in leaves]


@pytest.mark.parametrize("name", [c[0] for c in K.CAT_CASES])
def test_concat_addressing_equals_the_torch_expression_and_fp32_sums_stay_inside(name):
    d = K.cat_case(name)
    y, grads = _cat_torch(name, torch.float64)
    assert torch.equal(y.float(), d["dst"])
    for g, w in zip(d["grads"], grads):
        assert float((g - w).abs().max()) <= 1e-13 * (float(w.abs().max()) + 1)
    _, g32 = _cat_torch(name, torch.float32)
    c0 = 0
    for i, (kind, C) in enumerate(d["sources"]):
        got = K.restate_cat_bwd_fp32(d["ddst"].numpy(), kind, C, d["HW"], c0)
        _ratio("cat", "restatement", got, d["grads"][i], d["S"][i])
        _ratio("cat", "torch fp32", g32[i], d["grads"][i], d["S"][i])
        c0 += C


# ----------------------------------------------------------------------------------------------- tolerances and coverage
def test_tolerances_come_from_the_fp32_evaluations():
    """the figures over every row (measured here, or by the tests above where they ran): the recorded ones are what was
    measured, TOL is 4 x that and under the ceiling"""
    for row in K.STN_ROWS + K.STN_EX_ROWS:
        _stn_row(row)
    for c in ATTN_CALLS:
        test_attention_formulas_equal_torch_and_fp32_evaluations_stay_inside(*c)
    for c in SM_CALLS:
        test_softmax_formulas_equal_torch_and_fp32_evaluations_stay_inside(*c)
    for c in K.CAT_CASES:
        test_concat_addressing_equals_the_torch_expression_and_fp32_sums_stay_inside(c[0])
    assert set(FIG) == set(K.TOL) == set(K.MEASURED)
    for kind, f in sorted(FIG.items()):
        print("%-7s %s  -> TOL %.2e (%.2f x 2^-24)" % (kind, "  ".join("%s %.2f x 2^-24" % (n, v / K.EPS32) for n, v in sorted(f.items())),
                                                       K.TOL[kind], K.TOL[kind] / K.EPS32))
        worst = max(f.values())
        assert K.EPS32 <= K.TOL[kind] <= K.TOL_CEILING, kind
        assert K.MEASURED[kind] >= worst and K.TOL[kind] >= 4 * K.MEASURED[kind], (kind, worst / K.EPS32)
        assert K.MEASURED[kind] <= 1.25 * worst + 0.02 * K.EPS32, "%s: the recorded figure is not the measured one (%.2f x 2^-24)" % (
            kind, worst / K.EPS32)


def test_the_transformer_table_reaches_every_path():
    assert {K.theta_kind(n) for n in K.THETA_NAMES} == K.THETA_KINDS and K.NT == 18
    d = {n: K.theta_det(t) for n, t in zip(K.THETA_NAMES, K.THETAS)}
    assert d["singular zero"] == 0 and d["singular rank one"] == 0 and 0 < abs(d["nearly singular"]) <= 2e-12
    assert d["reflection"] < 0 and K.THETAS[K.THETA_NAMES.index("minification")][0] == 3
    assert {"crop " + n for n in K.BOX_NAMES} | {"place " + n for n in K.BOX_NAMES} <= set(K.THETA_NAMES)
    # every theta kind x align_corners: the thetas are the batch of every row
    assert all(r[0] >= 12 for r in K.STN_ROWS) and {r[6] for r in K.STN_ROWS} == {0, 1}
    full = [r for r in K.STN_ROWS if r[0] >= K.NT]
    assert {(r[4] * r[5]) for r in full} >= {255, 256, 257} and 257 in {r[2] * r[3] for r in full}
    assert any(r[2] != r[3] and r[4] != r[5] for r in full)
    for ac in (0, 1):
        rows = [r for r in full if r[6] == ac]
        assert any(r[2] == 1 for r in rows) and any(r[3] == 1 for r in rows)          # a source axis of 1, either way
        assert any(r[4] == 1 for r in rows) and any(r[5] == 1 for r in rows)          # an output axis of 1
    assert {1, 8, 13} <= {r[1] for r in full}
    assert [r[:7] for r in K.STN_ROWS + K.STN_EX_ROWS if not K.stn_rel_applies(r[2], r[3], r[6])] == [(K.NT, 3, 1, 257, 3, 5, 0)]
    # whole-output searches: singular thetas, and one-pixel source axes with align_corners
    th = K.THETAS[K.THETA_NAMES.index("singular rank one")]
    assert K.stn_searches_everything(th, 8, 8, 0) and not K.stn_searches_everything(K.THETAS[0], 8, 8, 1)
    assert K.stn_searches_everything(K.THETAS[0], 1, 257, 1) and not K.stn_searches_everything(K.THETAS[0], 1, 257, 0)
    # the forward's channel split
    split = {r[:6]: K.stn_fwd_split(r[0], r[1], r[4], r[5]) for r in K.STN_ROWS}
    assert split[(K.NT, 13, 5, 7, 15, 17)][0] == 13                                      # csplit == C
    assert split[(12, 50, 6, 5, 32, 32)] == (17, 3, 2)                                   # ragged: 16 chunks of 3, one of 2
    assert split[(256, 2, 4, 4, 32, 32)] == (1, 2, 2)                                    # csplit == 1
    # the _ex forms
    ex = K.STN_EX_ROWS
    assert any(r[7] < r[0] and not r[8] for r in ex) and any(r[8] and r[4] * r[5] < 256 for r in ex)
    assert any(r[8] and r[4] * r[5] > 256 for r in ex) and {r[9] for r in ex} == {0, 3}
    assert all(r[0] // r[9] > 1 for r in ex if r[9]) and any(r[9] and r[7] < r[0] for r in ex)
    assert sorted(K.theta_index(6, 3).tolist()) == list(range(6)) and K.theta_index(6, 3).tolist() == [0, 3, 1, 4, 2, 5]


def test_the_attention_softmax_and_concat_tables_reach_every_path():
    rows = K.ATTN_ROWS
    for slots in (8, 16, 32):           # every slot count full and one past the one below
        assert any(K.attn_slots(r[3]) == slots and r[3] == slots for r in rows)
    assert any(r[3] == 9 for r in rows) and any(r[3] == 17 for r in rows)
    assert any(r[1] >= 8 and r[1] % 8 for r in rows) and any(r[1] < 8 for r in rows) and any(r[1] % 8 == 0 for r in rows)
    assert max(r[1] for r in rows) == 128 and max(r[3] for r in rows) == 32
    assert any(r[2] == 1 for r in rows) and any(r[2] == 257 for r in rows) and any(r[2] % r[0] for r in rows)
    sm = K.SOFTMAX_ROWS
    assert any(o * i > 256 and i > 1 for o, _, i in sm) and any(i == 1 and o > 256 for o, _, i in sm) and (1, 1, 1) in sm
    seen = {k: False for k in ("zero", "above", "negative")}
    for o, L, i in sm:
        for k, v in K.lens_clamps(K.softmax_lens(o, L, i), L).items():
            seen[k] |= v
    assert all(seen.values()) and set(K.SCALES) == {1.0, 4.0, -2.5}
    cases = {c[0]: c for c in K.CAT_CASES}
    assert {c[1] for c in K.CAT_CASES} == {1, 15, 16, 256} and {len(c[2]) for c in K.CAT_CASES} == {1, 2, 3, 4}
    assert {k for c in K.CAT_CASES for k, _ in c[2]} == set(K.CAT_KINDS)
    bc = lambda c: [K.cat_layout(k, C, c[1])[4] for k, C in c[2]]
    assert bc(cases["broadcast first"])[0] == 1 and bc(cases["reversed"])[0] == 1 and bc(cases["base hw16"])[-1] == 1
    assert bc(cases["broadcast in the middle"]) == [0, 1, 0, 0]
    assert all(bc(cases["all broadcast"])) and not any(bc(cases["all plain"]))
    assert {c[3] for c in K.CAT_CASES if c[2] == K.BASE4} >= {(0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (0, 0, 0, 0)}
    # the forward's two kernels; the backward's two kinds of work item
    assert K.cat_vector(16, K.BASE4) and not K.cat_vector(15, K.BASE4) and not K.cat_vector(16, K.BASE4, misaligned=True)
    assert {K.cat_vector(c[1], c[2]) for c in K.CAT_CASES} == {True, False}
