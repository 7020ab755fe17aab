"""The references and tolerances of tests/pool_cases.py, checked without a GPU (what tests/test_bn_reference_cpu.py is to
tests/bn_cases.py):
  * the plain fp64 formulas equal F.avg_pool2d, F.max_pool2d and F.interpolate in fp64, and their autograd, at every row; the
    window offsets equal oracle.inception_oracle.pool_offsets where that applies and an explicit first-maximum search everywhere;
  * TOL["avg"] and TOL["bil"] come from two fp32 CPU evaluations -- torch's own fp32 operator and a numpy fp32 restatement of the
    kernel's arithmetic -- measured as the largest err / bound-with-TOL-1 over every row; the recorded constants are at least 4 x
    that and at most the project's ceiling.  The margin of 4 is conv_cases.TOL's: it covers the device's different but equally
    valid rounding order;
  * the bounds are not loose: wherever a wrong variant (align_corners=True, no half-pixel offset, swapped weights, no clamp of
    i1; count_include_pad=False) differs from the reference at all, it fails the bound at some element, forward and backward;
  * the feeder's numpy passes equal Pillow's Image.resize(BILINEAR) bit for bit at every size of the table, and tmp / out of the
    cases module agree with attngan/feeder.resample_u8_reference;
  * the rows reach what they are there for: both branches of bilinear_bwd_kernel, elements in 0, 1, 2 and 4 windows of the
    max-pool gather, rows no window covers in both pools, more than one block for every kernel, the grid-stride loop's second trip.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

import pool_cases as K
from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import feeder  # noqa: E402

ids = lambda v: str(v).replace(" ", "")  # noqa: E731
DIFFERS = 1e-12             # a variant "differs at all" where it is further than this (relative to the largest value) from the reference


def _close64(a, b, what):
    scale = float(b.abs().max()) + 1e-300
    assert float((a - b).abs().max()) <= 1e-12 * scale, (what, float((a - b).abs().max()), scale)


def _ratio(got, ref, bound, what):
    """largest err / bound; where the bound is 0 the values are equal"""
    err = (got.double() - ref).abs()
    assert bool((err[bound == 0] == 0).all()), what
    return float((err / bound.clamp_min(1e-300))[bound > 0].max()) if bool((bound > 0).any()) else 0.0


def _fails(variant, ref, bound, tol):
    """whether the variant leaves the bound at some element, given that it differs from the reference at all (else None)"""
    diff = (variant - ref).abs()
    if float(diff.max()) <= DIFFERS * (float(ref.abs().max()) + 1e-300):
        return None
    return bool((diff > tol * bound).any())


# ------------------------------------------------------------------------------------------------------------ average pool
def _avg_torch(x, dy, k, s, pad, dtype, include=True):
    xt = x.to(dtype)[None].clone().requires_grad_(True)
    y = F.avg_pool2d(xt, k, s, pad, count_include_pad=include)
    g, = torch.autograd.grad(y, xt, dy.to(dtype)[None])
    return y.detach()[0], g[0]


@functools.lru_cache(maxsize=None)
def _avg_ratios(row):
    P, H, W, k, s, pad = row
    d = K.avg_case(row)
    y32, _ = _avg_torch(d["x"], d["dy"], k, s, pad, torch.float32)
    yr = torch.from_numpy(K.avg_restate_fp32(d["x"].numpy(), k, s, pad))
    return {"torch fp32": _ratio(y32, d["y"], d["y_bound"], row), "restatement": _ratio(yr, d["y"], d["y_bound"], row)}


@pytest.mark.parametrize("row", K.AVG_ROWS, ids=ids)
def test_avgpool_formulas_equal_torch_and_fp32_evaluations_stay_inside(row):
    P, H, W, k, s, pad = row
    d = K.avg_case(row)
    y, dx = _avg_torch(d["x"], d["dy"], k, s, pad, torch.float64)
    assert tuple(y.shape) == (P, d["OH"], d["OW"])
    _close64(d["y"], y, "y")
    _close64(d["dx"], dx, "dx")
    assert bool((d["dx"][:, ~d["covered"]] == 0).all()) and bool((d["dx_bound"][:, ~d["covered"]] == 0).all())
    assert bool((d["dx_bound"][:, d["covered"]] > 0).all())
    # torch's fp32 backward stays inside the fixed bound of the trunk test
    _, dx32 = _avg_torch(d["x"], d["dy"], k, s, pad, torch.float32)
    assert _ratio(dx32, d["dx"], d["dx_bound"], row) <= 1.0
    for name, r in _avg_ratios(row).items():
        assert r <= K.TOL["avg"] / 4, "%s at %s: %.3f > %.3f" % (name, row, r, K.TOL["avg"] / 4)


@pytest.mark.parametrize("row", [r for r in K.AVG_ROWS if r[5] > 0], ids=ids)
def test_avgpool_bounds_reject_the_other_divisors(row):
    """count_include_pad=False (torch's own, and the plain formula with the clipped window's size) fails the bound, both ways"""
    P, H, W, k, s, pad = row
    d, m = K.avg_case(row), K.avg_case(row, "clipped")
    y, dx = _avg_torch(d["x"], d["dy"], k, s, pad, torch.float64, include=False)
    _close64(m["y"], y, "clipped y")
    _close64(m["dx"], dx, "clipped dx")
    assert _fails(y, d["y"], d["y_bound"], K.TOL["avg"]) is True
    assert _fails(m["y"], d["y"], d["y_bound"], K.TOL["avg"]) is True
    assert _fails(dx, d["dx"], d["dx_bound"], 1.0) is True
    assert _fails(m["dx"], d["dx"], d["dx_bound"], 1.0) is True


# ----------------------------------------------------------------------------------------------------------------- max pool
def _windows_of(P, H, W, k, s):
    """how many windows hold each element"""
    OH, OW = K.out_size(H, k, s), K.out_size(W, k, s)
    return K._scatter(torch.ones((1, OH, OW), dtype=torch.float64), H, W, k, s, 0, 1.0)[0]


@pytest.mark.parametrize("row", K.MAX_ROWS + [K.MAX_FWD_ONLY], ids=ids)
def test_maxpool_references(row):
    P, H, W, k, s = row
    d = K.max_case(row)
    x = d["x"]
    assert not bool(torch.isnan(x).any())
    # the first maximum in row-major order, searched explicitly (numpy's argmax returns the first)
    win = torch.stack(K._windows(x, k, s, 0, d["OH"], d["OW"]))
    top = win.max(0).values
    assert torch.equal(top, d["y"])
    first = np.argmax((win == top[None]).numpy(), axis=0)
    assert np.array_equal(first, d["idx"].numpy())
    if (k, s) == (3, 2):
        from oracle import inception_oracle as IO
        assert torch.equal(IO.pool_offsets(x[None])[0], d["idx"])
    # the planted windows
    p, oy, ox = d["planted"]["tie"]
    assert float(d["y"][p, oy, ox]) == 0.25 and int(d["idx"][p, oy, ox]) == 0
    p, oy, ox = d["planted"]["zeros"]
    w = x[p, oy * s:oy * s + k, ox * s:ox * s + k]
    assert bool((w[w > float("-inf")] == 0).all()) and bool(torch.signbit(w.flatten()[0])) and (k == 1 or not bool(torch.signbit(w.flatten()[1])))
    assert float(d["y"][p, oy, ox]) == 0 and bool(torch.signbit(d["y"][p, oy, ox])) and int(d["idx"][p, oy, ox]) == 0
    p, oy, ox = d["planted"]["-inf"]
    assert float(d["y"][p, oy, ox]) == float("-inf") and int(d["idx"][p, oy, ox]) == 0
    assert bool((x == 0).sum() > P * H * W // 4)                    # post-ReLU: ties among zeros
    # the routed gradient is torch's
    xt = x.double()[None].clone().requires_grad_(True)
    g, = torch.autograd.grad(F.max_pool2d(xt, k, s), xt, d["dy"].double()[None])
    _close64(d["dx"], g[0], "dx")
    assert bool((d["dx"][d["routed"] == 0] == 0).all()) and bool((d["dx_bound"][d["routed"] == 0] == 0).all())
    assert bool((d["routed"] <= _windows_of(P, H, W, k, s)[None]).all())


# ------------------------------------------------------------------------------------------------------------------ bilinear
def _bil_torch(x, dy, OH, OW, dtype, align=False):
    xt = x.to(dtype)[None].clone().requires_grad_(True)
    y = F.interpolate(xt, size=(OH, OW), mode="bilinear", align_corners=align)
    g, = torch.autograd.grad(y, xt, dy.to(dtype)[None])
    return y.detach()[0], g[0]


@functools.lru_cache(maxsize=None)
def _bil_ratios(row):
    P, H, W, OH, OW = row
    d = K.bil_case(row)
    out = {}
    y32, dx32 = _bil_torch(d["x"], d["dy"], OH, OW, torch.float32)
    out["torch fp32"] = max(_ratio(y32, d["y"], d["y_bound"], row), _ratio(dx32, d["dx"], d["dx_bound"], row))
    r = 0.0
    for contracted in (False, True):
        yr, dxr = K.bil_restate_fp32(d["x"].numpy(), d["dy"].numpy(), OH, OW, contracted)
        r = max(r, _ratio(torch.from_numpy(yr), d["y"], d["y_bound"], row), _ratio(torch.from_numpy(dxr), d["dx"], d["dx_bound"], row))
    out["restatement"] = r
    return out


@pytest.mark.parametrize("row", K.BIL_ROWS, ids=ids)
def test_bilinear_formulas_equal_torch_and_fp32_evaluations_stay_inside(row):
    P, H, W, OH, OW = row
    d = K.bil_case(row)
    y, dx = _bil_torch(d["x"], d["dy"], OH, OW, torch.float64)
    _close64(d["y"], y, "y")
    _close64(d["dx"], dx, "dx")
    M = K.bil_dense(row)
    assert not bool(M[:, P * H * W:].any())
    _close64((M[:, :P * H * W] @ d["x"].double().flatten()).view(P, OH, OW), d["y"], "dense y")
    _close64((M[:, :P * H * W].T @ d["dy"].double().flatten()).view(P, H, W), d["dx"], "dense dx")
    assert bool((d["dx"][d["unread"]] == 0).all())
    if row == K.BIL_IDENTITY:
        assert torch.equal(d["y"], d["x"].double()) and torch.equal(d["dx"], d["dy"].double())
        for contracted in (False, True):
            yr, dxr = K.bil_restate_fp32(d["x"].numpy(), d["dy"].numpy(), OH, OW, contracted)
            assert np.array_equal(yr.view(np.int32), d["x"].numpy().view(np.int32))
            assert np.array_equal(dxr.view(np.int32), d["dy"].numpy().view(np.int32))
    for name, r in _bil_ratios(row).items():
        assert r <= K.TOL["bil"] / 4, "%s at %s: %.3f > %.3f" % (name, row, r, K.TOL["bil"] / 4)


@pytest.mark.parametrize("row", K.BIL_ROWS, ids=ids)
@pytest.mark.parametrize("variant", K.BIL_VARIANTS)
def test_bilinear_bounds_reject_the_wrong_variants(variant, row):
    P, H, W, OH, OW = row
    d = K.bil_case(row)
    M = K.bil_dense(row, variant)
    xe = torch.cat([d["x"].double().flatten(), torch.zeros(W + 2, dtype=torch.float64)])
    y = (M @ xe).view(P, OH, OW)
    dx = (M.T @ d["dy"].double().flatten())[:P * H * W].view(P, H, W)
    if variant == "align_corners":
        yt, dxt = _bil_torch(d["x"], d["dy"], OH, OW, torch.float64, align=True)
        _close64(y, yt, "align_corners y")
        _close64(dx, dxt, "align_corners dx")
    fy, fdx = _fails(y, d["y"], d["y_bound"], K.TOL["bil"]), _fails(dx, d["dx"], d["dx_bound"], K.TOL["bil"])
    assert fy is not False, "forward: %s differs from the reference at %s and stays inside the bound" % (variant, row)
    assert fdx is not False, "backward: %s differs from the reference at %s and stays inside the bound" % (variant, row)
    test_bilinear_bounds_reject_the_wrong_variants.seen.add((variant, fy, fdx))


test_bilinear_bounds_reject_the_wrong_variants.seen = set()


def test_every_variant_differs_somewhere():
    seen = test_bilinear_bounds_reject_the_wrong_variants.seen
    if not seen:
        pytest.skip("needs the variant rows of this module to have run (a selection was made)")
    for v in K.BIL_VARIANTS:
        assert (v, True, True) in seen, v


# ------------------------------------------------------------------------------------------------------------- the constants
def test_tolerances_come_from_the_fp32_evaluations():
    fig = {"avg": {}, "bil": {}}
    for kind, rows, fn in (("avg", K.AVG_ROWS, _avg_ratios), ("bil", K.BIL_ROWS, _bil_ratios)):
        for row in rows:
            for name, r in fn(row).items():
                fig[kind][name] = max(fig[kind].get(name, 0.0), r)
    for kind in ("avg", "bil"):
        worst = max(fig[kind].values())
        print("%s  %s  MEASURED %.3f  TOL %.3f (%.2f x the larger), ceiling %.1e / 2^-24 = %.1f" % (
            kind, "  ".join("%s %.3f" % (n, v) for n, v in sorted(fig[kind].items())), K.MEASURED[kind], K.TOL[kind], K.TOL[kind] / worst,
            K.TOL_CEILING, K.TOL_CEILING / K.EPS32))
        assert K.MEASURED[kind] >= worst
        assert K.TOL[kind] >= 4 * K.MEASURED[kind] >= 4 * worst
        assert K.TOL[kind] <= 4.1 * K.MEASURED[kind] and K.MEASURED[kind] <= 1.05 * worst          # measured, not chosen
        # the bounds are TOL x 2^-24 x (sums of absolute terms): the constant in the units of conv_cases.TOL
        assert K.TOL[kind] * K.EPS32 <= K.TOL_CEILING


# ---------------------------------------------------------------------------------------------------------------------- sums
@pytest.mark.parametrize("n", K.SUM_N)
def test_sum_operands(n):
    for G in (2,) + K.SUM_G:
        x = K.sum_operands(n, G)
        assert not bool(torch.isnan(x).any())
        assert not bool(torch.isnan(K.group_sum_reference(x)).any())
        if G >= 2:
            assert not bool(torch.isnan(x[0] + x[1]).any())
    x = K.sum_operands(max(n, 16), 2)
    y = x[0] + x[1]
    sub = (y != 0) & (y.abs() < 2.0 ** -126)
    assert int(sub.sum()) >= 3, "torch on this CPU flushes subnormals: the expectation would not be IEEE's"
    assert bool(torch.isinf(y).any()) and bool(((y == 0) & torch.signbit(y)).any()) and bool(((y == 0) & ~torch.signbit(y)).any())
    nan = torch.isnan(x[0] * 0.0)
    assert int(nan.sum()) == int(torch.isinf(x[0]).sum()) > 0           # the one NaN result: inf * 0
    assert K.same_ieee(x[0] * 0.0, x[0] * 0.0) and not K.same_ieee(x[0], x[1])


# -------------------------------------------------------------------------------------------------------------------- feeder
def test_crop_expectations():
    assert K.PRECISION_BITS == feeder.PRECISION_BITS
    for row in K.CROP_ROWS:
        (B, ori, size), params = row
        d = K.crop_case(row)
        img = d["src"].float().permute(0, 3, 1, 2) / 255.0               # ToTensor
        for b, (h1, w1, flip) in enumerate(params):
            c = img[b, :, w1:w1 + size, h1:h1 + size]
            if flip:
                c = torch.flip(c, dims=[2])
            assert torch.equal((c - 0.5) / 0.5, d["out"][b])
            assert torch.equal((c * 255).round().to(torch.uint8).permute(1, 2, 0), d["q"][b])
        margin = ori - size
        assert margin == 0 or ({p[0] for p in params} >= {0, margin} and {p[1] for p in params} >= {0, margin})


@pytest.mark.parametrize("row", K.RESAMPLE_ROWS + [(K.CHAIN[0][0][0], K.CHAIN[0][0][2], K.CHAIN[1])], ids=ids)
def test_resample_passes_equal_pillow_bit_for_bit(row):
    B, S, OS = row
    d = K.resample_case(row, feeder.pil_bilinear_coeffs)
    assert tuple(d["tmp"].shape) == (B, S, OS, 3) and d["ksize"] == d["kk"].shape[1]
    kinds = set()
    for b in range(B):
        img = d["img"][b].numpy()
        want = np.asarray(Image.fromarray(img).resize((OS, OS), Image.BILINEAR))
        assert np.array_equal(feeder.resample_u8_reference(img, OS), want)
        assert np.array_equal(d["out_u8"][b], want)
        kinds.add(b % 3)
    assert torch.equal(d["out"], K.normalise(d["out_u8"]))
    bounds = d["bounds"].numpy()
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= S).all() and (bounds[:, 1] <= d["ksize"]).all()
    if row == (1, 20, 3):
        assert int(bounds[:, 1].max()) == 14
    if row == (2, 6, 9):
        assert d["ksize"] == 3


def test_the_chained_row_resamples_the_crop():
    crop, OS = K.CHAIN
    q = K.crop_case(crop)["q"]
    bounds, kk = feeder.pil_bilinear_coeffs(q.shape[1], OS)
    e = K.resample_expect(q, bounds, kk)
    for b in range(q.shape[0]):
        assert np.array_equal(e["out_u8"][b], np.asarray(Image.fromarray(q[b].numpy()).resize((OS, OS), Image.BILINEAR)))


# -------------------------------------------------------------------------------------------------------------------- census
def test_census_of_what_the_rows_reach():
    branches = set()
    for row in K.BIL_ROWS:
        branches |= K.bil_bwd_branches(row)
    assert branches == {"register", "loop"}
    assert K.bil_bwd_branches((1, 30, 30, 7, 200)) == {"loop"} and K.bil_bwd_branches((2, 4, 5, 32, 33)) == {"loop"}
    unread = {row: int(K.bil_case(row)["unread"].sum()) for row in K.BIL_ROWS}
    print("input elements no output reads:", {k: v for k, v in unread.items() if v})
    assert unread[(1, 30, 30, 7, 200)] > 0 and unread[K.BIL_IDENTITY] == 0
    # max pool: elements in 0, 1, 2 and 4 windows, and elements that 0, 1, 2 and 4 windows route their gradient to
    held, routed = set(), set()
    for row in K.MAX_ROWS:
        held |= set(_windows_of(*row).flatten().tolist())
        routed |= set(K.max_case(row)["routed"].flatten().tolist())
    assert held >= {0.0, 1.0, 2.0, 4.0} and routed >= {0.0, 1.0, 2.0, 4.0}, (held, routed)
    sub = K.max_case((2, 5, 5, 1, 2))
    assert float((sub["routed"] == 0).double().mean()) > 0.6            # sub-sampling: most of dx is exactly +0
    # rows (or columns) no window covers, in both pools
    assert any(bool((_windows_of(*row).sum(1) == 0).any()) for row in K.MAX_ROWS)
    assert any(bool((~K.avg_case(row)["covered"]).all(1).any()) for row in K.AVG_ROWS)
    assert not bool(K.avg_case((3, 9, 10, 2, 2, 0))["covered"][8].any())
    # padding-heavy corner: the first window of the pad = k / 2 row holds fewer in-bounds elements than padding
    t = K.avg_case((2, 7, 5, 5, 3, 2))["terms"]
    assert float(t[0, 0]) < 25 / 2
    # more than one block for every kernel, and the second trip of the grid-stride loop
    n = K.launches()
    assert all(v > K.BLOCK for v in n.values()), n
    assert any(P * K.out_size(H, k, s, p) * K.out_size(W, k, s, p) % K.BLOCK for P, H, W, k, s, p in K.AVG_ROWS if P == 300)
    assert K.GRID_CAP * K.BLOCK + K.BLOCK < K.ADD_LARGE_N <= K.GRID_CAP * K.BLOCK + 2 * K.BLOCK and max(K.SUM_N) <= K.GRID_CAP * K.BLOCK
    P, H, W, OH, OW = K.BIL_ROWS[-1]
    assert P * OH * OW > K.BLOCK and P * H * W > K.BLOCK and (P * OH * OW) % K.BLOCK and (P * H * W) % K.BLOCK
