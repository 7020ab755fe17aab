"""The references and tolerances of tests/bn_cases.py, checked without a GPU (what tests/test_conv_reference_cpu.py is to
tests/conv_cases.py):
  * the plain fp64 formulas equal F.batch_norm in fp64 with autograd through the activation wherever torch accepts the shape;
  * TOL comes from two fp32 CPU evaluations -- the numpy restatement of csrc/mogan_bn.h and torch's own fp32 batch_norm --
    measured as max (err - F) / S over every row and activation; the recorded constants are at least 4 x that and at most the
    project's ceiling.  The margin of 4 is conv_cases.TOL's: it covers the GPU's different but equally valid summation splits;
    torch's fp32 dx, whose channel sums are fp32, is held to the ceiling itself (see _kind);
  * the bounds of the affine, activation and bias entry points hold numpy fp32 evaluations of those kernels' formulas;
  * no RELU / LRELU pre-activation lies within KINK * TOL * S of 0, so the GPU module compares every element;
  * the table reaches every path x activation and both batch-chunk forms, by the predicates restated in bn_cases.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import bn_cases as K

TORCH_DX = "dx (torch's fp32 channel sums)"


def _act64(t, act):
    if act == K.RELU:
        return F.relu(t)
    if act == K.LRELU:
        return F.leaky_relu(t, K.SLOPE)
    if act == K.GLU:
        c = t.shape[1] // 2
        return t[:, :c] * torch.sigmoid(t[:, c:])
    return t


def _torch_eval(inp, act, res, dy, dtype):
    """F.batch_norm + activation (+ residual) and its autograd gradients in `dtype`"""
    x, gm, bt = (inp[k].to(dtype).clone().requires_grad_(True) for k in ("x", "gamma", "beta"))
    rm, rv = inp["rm"].to(dtype).clone(), inp["rv"].to(dtype).clone()
    y = _act64(F.batch_norm(x, rm, rv, gm, bt, True, K.MOM if dtype == torch.float64 else 0.1, K.EPS if dtype == torch.float64 else 1e-5), act)
    if res is not None:
        y = y + res.to(dtype)
    y.backward(dy.to(dtype))
    return {"y": y.detach(), "dx": x.grad, "dgamma": gm.grad, "dbeta": bt.grad, "rm": rm, "rv": rv}


def _kind(name, k):
    """which tolerance a figure belongs to.  torch's fp32 dx has a kind of its own: its backward sums a channel in fp32 and S_dx
    is written for the fp64 sums of the header (|s0| / n, not sum |d| / n), so where |d| and |xhat| are small torch's summation
    noise is all there is.  A finding (bn_cases.TOL), not the yardstick of TOL["dx"]; it is held to the ceiling itself instead."""
    if (name, k) == ("torch fp32", "dx"):
        return TORCH_DX
    return "y" if k == "y" else "dx" if k == "dx" else "dparam"


def _residual(shape, act, res):
    C = K.dims(shape)[1]
    return K.bn_res(shape)[:, :C // 2 if act == K.GLU else C].contiguous() if res else None


@functools.lru_cache(maxsize=None)
def _ratios(shape, act, res):
    """the two fp32 evaluations of one call -> {(evaluation, output): largest (err - F) / S}.  Where S is 0 the error is within F;
    the statistics of the restatement (fp64 sums, as the kernels') are within their fixed roundings alone."""
    B, C, HW = K.dims(shape)
    inp = K.bn_inputs(shape, K.kind_of(act))
    dy = K.bn_dy(shape, act)
    r = _residual(shape, act, res)
    d = K.bn_case(shape, act, res)
    ref, S, Fx = d["ref"], d["S"], d["F"]
    evals = {"restatement": {k: torch.from_numpy(v) for k, v in K.restate_fp32(
        inp["x"].numpy(), inp["gamma"].numpy(), inp["beta"].numpy(), act, None if r is None else r.numpy(), dy.numpy(),
        inp["rm"].numpy(), inp["rv"].numpy()).items()}}
    if B * HW > 1:
        evals["torch fp32"] = _torch_eval(inp, act, r, dy, torch.float32)
    out = {}
    for name, got in evals.items():
        for k in ("y", "dx", "dgamma", "dbeta"):
            err = (got[k].double() - ref[k]).abs() - Fx.get(k, 0.0)
            assert bool((err[S[k] == 0] <= 0).all()), (name, k)
            out[(name, k)] = float((err / S[k].clamp_min(1e-300))[S[k] > 0].max().clamp_min(0)) if bool((S[k] > 0).any()) else 0.0
    got = evals["restatement"]
    for k in ("mean", "invstd", "rm", "rv"):
        err = (got[k].double() - ref[k]).abs()
        assert bool((err <= Fx[k]).all()), (k, float((err / Fx[k]).max()))
    return out


def _limit(kind):
    return K.TOL_CEILING if kind == TORCH_DX else K.TOL[kind] / 4


@pytest.mark.parametrize("shape,act,res", K.BN_CALLS, ids=lambda v: str(v).replace(" ", ""))
def test_fp64_formulas_equal_torch_and_fp32_evaluations_stay_inside(shape, act, res):
    B, C, HW = K.dims(shape)
    if B * HW > 1:
        inp = K.bn_inputs(shape, K.kind_of(act))
        dy = K.bn_dy(shape, act)
        r = _residual(shape, act, res)
        # the formulas with torch's own 1 - momentum
        ref, S, Fx, ctx = K.bn_forward(inp["x"], inp["gamma"], inp["beta"], act, r, inp["rm"], inp["rv"], one_minus=1.0 - K.MOM)
        rb, Sb, _ = K.bn_backward(ctx, dy)
        ref.update(rb); S.update(Sb)
        del ctx
        want = _torch_eval(inp, act, r, dy, torch.float64)
        for k, w in want.items():           # (relative to the sum over the absolute terms where there is one: d gamma of a few values)
            scale = max(float(w.abs().max()), float(S[k].max()) if k in S else 0.0) + 1e-300
            assert float((ref[k] - w).abs().max()) <= 1e-12 * scale, (k, float((ref[k] - w).abs().max()), scale)
    for (name, k), ratio in _ratios(shape, act, res).items():
        kind = _kind(name, k)
        assert ratio <= _limit(kind), "%s %s of %s %s: %.3e (%.2f x 2^-24) > %.2e" % (
            name, k, shape, K.ACT_NAMES[act], ratio, ratio / K.EPS32, _limit(kind))


def test_tolerances_come_from_the_fp32_evaluations():
    """the figures over every call of the table (measured here, or taken from the rows above where they ran): the recorded ones
    are what was measured, TOL is 4 x the larger evaluation's and under the ceiling; torch's fp32 dx stays under the ceiling"""
    fig = {}
    for call in K.BN_CALLS:
        for (name, k), ratio in _ratios(*call).items():
            f = fig.setdefault(_kind(name, k), {})
            f[name] = max(f.get(name, 0.0), ratio)
    for kind, f in sorted(fig.items()):
        print("%-7s %s  -> held to %.2e (%.2f x 2^-24)" % (kind, "  ".join("%s %.2f x 2^-24" % (n, v / K.EPS32) for n, v in sorted(f.items())),
                                                         _limit(kind), _limit(kind) / K.EPS32))
    for kind in ("y", "dx", "dparam"):
        worst = max(fig[kind].values())
        assert K.EPS32 <= K.TOL[kind] <= K.TOL_CEILING
        assert K.TOL[kind] >= 4 * worst
        assert K.MEASURED[kind] >= worst and K.TOL[kind] >= 4 * K.MEASURED[kind]
    assert set(fig[TORCH_DX]) == {"torch fp32"} and fig[TORCH_DX]["torch fp32"] <= K.TOL_CEILING


# ------------------------------------------------------------------ the affine / activation / bias bounds, evaluated in fp32
@pytest.mark.parametrize("shape", K.AFFINE, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("act", [K.NONE, K.RELU, K.LRELU])
def test_affine_bounds_hold_an_fp32_evaluation(shape, act):
    """the bounds the GPU module applies to mogan_affine_act_fwd / _bwd (TOL["y"] * S for y, two roundings for dx) against the
    numpy fp32 restatement of affine_act_kernel: documented accuracy, not figures fitted to a kernel"""
    d = K.affine_inputs(shape, act)
    ref, S, Fx = K.affine_reference(d["x"], d["scale"], d["shift"], act, d["dy"])
    got = K.restate_affine_fp32(d["x"].numpy(), d["scale"].numpy(), d["shift"].numpy(), act, d["dy"].numpy())
    for k, bnd in (("y", K.bound("y", S, Fx)), ("dx", Fx["dx"])):
        err = (torch.from_numpy(got[k]).double() - ref[k]).abs()
        assert bool((err <= bnd).all()), (k, float((err / bnd.clamp_min(1e-300)).max()))


@pytest.mark.parametrize("shape", K.AFFINE + [K.GLU_C2], ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("act", [K.RELU, K.LRELU, K.GLU, K.TANH, K.SIGMOID])
def test_act_bounds_hold_an_fp32_evaluation(shape, act):
    """act_reference's absolute bounds (the fast exponential's and tanhf's documented accuracy plus the roundings of the formula)
    against the numpy fp32 restatement of act_kernel / glu_kernel on the inputs the GPU module uses"""
    B, C, HW = K.dims(shape)
    xt, dyt = K.T("actx%s" % (shape,), (B, C, HW), 1.5, 0.3), K.T("actg%s%d" % (shape, act), (B, C // 2 if act == K.GLU else C, HW))
    ref, Fx = K.act_reference(xt, act, dyt)
    got = K.restate_act_fp32(xt.numpy(), act, dyt.numpy())
    for k in ("y", "dx"):
        err = (torch.from_numpy(got[k]).double() - ref[k]).abs()
        assert bool((err <= Fx[k]).all()), (k, float((err / Fx[k].clamp_min(1e-300)).max()))


@pytest.mark.parametrize("shape", K.AFFINE + [(5, 300)], ids=lambda v: str(v).replace(" ", ""))
def test_bias_bounds_hold_an_fp32_evaluation(shape):
    """one rounding of y + bias; d bias as the fp64 sum rounded once (bias_grad_kernel sums in fp64)"""
    B, C, HW = K.dims(shape)
    y0, bias, dyt = K.T("biy%s" % (shape,), (B, C, HW)), K.T("bib%d" % C, (C,), 0.3), K.T("big%s" % (shape,), (B, C, HW))
    want = y0.double() + bias.double().view(1, -1, 1)
    assert bool((((y0 + bias.view(1, -1, 1)).double() - want).abs() <= K.EPS32 * want.abs()).all())
    s = dyt.double().sum((0, 2))
    assert bool(((s.float().double() - s).abs() <= K.EPS32 * s.abs()).all())


@pytest.mark.parametrize("shape,act", [(s, a) for s, a in K.BN_ROWS if a in (K.RELU, K.LRELU)], ids=lambda v: str(v).replace(" ", ""))
def test_no_preactivation_near_a_kink(shape, act):
    d = K.bn_case(shape, act)
    margin = d["t"].abs() - K.KINK * K.TOL["y"] * d["S_t"]
    assert float(margin.min()) >= 0, "%d pre-activations inside the kink band" % int((margin < 0).sum())
    assert d["inp"]["moved"] <= 4 + d["t"].numel() // 50000, d["inp"]["moved"]          # a handful


@pytest.mark.parametrize("shape", K.GROUPED)
def test_no_preactivation_near_a_kink_grouped(shape):
    G = shape[0]
    inp = K.bn_inputs(shape[1:], "kink", G)
    per = inp["x"].shape[0] // G
    for g in range(G):
        ctx = K.bn_forward(inp["x"][g * per:(g + 1) * per], inp["gamma"], inp["beta"], K.NONE)[3]
        assert float((ctx["t"].abs() - K.KINK * K.TOL["y"] * ctx["S_t"]).min()) >= 0


@pytest.mark.parametrize("shape", K.AFFINE)
def test_no_preactivation_near_a_kink_affine(shape):
    d = K.affine_inputs(shape, K.RELU)
    ref, S, _ = K.affine_reference(d["x"], d["scale"], d["shift"], K.NONE)
    assert float((ref["y"].abs() - K.KINK * K.TOL["y"] * S["y"]).min()) >= 0


def test_grouped_reference_is_the_calls_in_sequence():
    """grouped_reference against F.batch_norm called G times in fp64 (running statistics carried, parameter gradients summed)"""
    shape = K.GROUPED[0]
    G, B = shape[0], shape[1]
    for act in K.BN_ACTS:
        inp = K.bn_inputs(shape[1:], K.kind_of(act), G)
        dy = K.bn_dy(shape[1:], act, G)
        ref, _ = K.grouped_reference(inp["x"], inp["gamma"], inp["beta"], act, inp["rm"], inp["rv"], dy, G)
        x, gm, bt = (inp[k].double().clone().requires_grad_(True) for k in ("x", "gamma", "beta"))
        y = torch.cat([_act64(F.batch_norm(x[g * B:(g + 1) * B], None, None, gm, bt, True, K.MOM, K.EPS), act) for g in range(G)])
        y.backward(dy.double())
        for k, w in (("y", y.detach()), ("dx", x.grad), ("dgamma", gm.grad), ("dbeta", bt.grad)):
            assert float((ref[k] - w).abs().max()) <= 1e-12 * float(w.abs().max()), k


def test_the_table_reaches_every_path():
    reached = {(K.path_of(s), a) for s, a in K.BN_ROWS}
    assert reached == {(p, a) for p in ("one", "two", "three") for a in K.BN_ACTS}
    assert all(K.path_of(s) == "one" for s in K.ONE_LAUNCH) and all(K.path_of(s) == "two" for s in K.TWO_LAUNCH + list(K.BIG_TWO_LAUNCH.values()))
    assert all(K.path_of(s) == "three" for s in K.THREE_LAUNCH + K.BN1D)
    assert {K.stats_kernel(s) for s in K.BN1D} == {"per-channel-thread"}
    # the first size past one launch, the floor and the exactly full block
    assert K.dims(K.ONE_LAUNCH[0])[0] * K.dims(K.ONE_LAUNCH[0])[2] == 16 and K.dims(K.ONE_LAUNCH[3])[0] * K.dims(K.ONE_LAUNCH[3])[2] == 4096
    # the VEC apply kernel through the fused entry: three launches with HW % 4 == 0
    assert any(K.path_of(s) == "three" and K.dims(s)[2] % 4 == 0 and K.dims(s)[2] > 1 for s in K.THREE_LAUNCH)
    # both batch-chunk forms, every activation on the two-launch one
    for a in K.BN_ACTS:
        assert K.chunks(K.BIG_TWO_LAUNCH[a], a) == [64, 2]
    assert K.chunks((34, 2000, 3, 3), K.NONE) == [32, 2]
    assert all(len(K.chunks(s, K.NONE)) == 2 for s in K.AFFINE[1:])
    # a partial last tile of 4096 values (the ragged statistics slabs of this row: test_bn_rejections_cpu pins the split
    # through mogan_bn_ws_bytes)
    assert K.dims(K.TWO_LAUNCH[1])[2] % 4096 == 4
