"""-m gpu: the batch-norm, affine, activation and bias entry points of include/mogan_hip.h through ctypes, per element against
fp64 and under the memory contract of tests/memguard.py -- what tests/test_conv_entry_points_gpu.py does for the convolutions.
Shapes (one per path of the host dispatch in csrc/mogan_norm.hip, at the smallest sizes where the path can go wrong), inputs,
references and bounds are tests/bn_cases.py; tests/test_bn_reference_cpu.py derives the tolerances without a GPU and
tests/test_bn_rejections_cpu.py holds every rejection that is answered before a launch.

Memory, every call:
  * every output -- y, mean, invstd, both running buffers, dx (both GLU halves), dgamma, dbeta -- is the payload of a guard-banded
    buffer: NaN poison in write mode, a finite base in accumulate mode; afterwards every element is written, nothing outside changed;
  * every input lives in NaN bands and is bitwise unchanged afterwards, bands included;
  * the workspace is a guard-banded byte buffer of exactly mogan_bn_ws_bytes(B, C, HW), refilled with 0xFF before each call (a
    partial sum that is read and was never written shows as NaN); its bands stay intact.  One byte less, or NULL: MOGAN_ERR_WS and
    every output untouched on the paths that need it; the one-launch forward returns 0 with the same bits;
  * the same call a second time, after poisoning again, gives the same bits;
  * NULL running buffers, NULL dgamma / dbeta: every other output has the bits it has with the buffers present.

Values: every element of every output within bn_cases.bound (TOL * S + F), and beside that the whole-tensor figures of
test_kernels_gpu.test_bn_act (rel-L2: y 5e-6, running statistics 1e-6, gradients 2e-5), grouped calls included, over the ordinary
channels -- the constant and the large-offset channel carry an absolute error of 2^-24 * |x * sc| by construction, which only the
per-element bound can judge.
The last test asserts the census of (path, activation, direction) and prints the largest err / bound per output kind."""
import functools

import pytest
import torch

import bn_cases as K
import memguard as mg
from helpers import load_pkg

load_pkg()
from mogan_amd.hip import lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ERR_WS = -3
SLOPE, EPS, MOM = 0.2, 1e-5, 0.1          # (ctypes rounds them to the fp32 values bn_cases computes with)
BIG = 1 << 20                               # rows beyond this many values run the core calls only (time)

RAN = set()            # (path, activation, direction)
FIG = {}               # output kind -> largest err / bound


def L():
    return lib.load()


def _inp(t):
    """an input inside NaN guard bands, frozen (bands included)"""
    g = mg.Guarded(tuple(t.shape), (Ellipsis,), DEV, base=t)
    g.frozen = mg.Frozen(g.buf)
    return g


def _out(shape, base=None):
    return mg.Guarded(tuple(shape), (Ellipsis,), DEV, base=base)


def _p(g):
    return None if g is None else g.ptr


class _WS:
    """a guard-banded workspace of exactly `n` bytes"""

    def __init__(self, n):
        self.n = n
        self.b = mg.Banded((n,), torch.uint8, DEV)

    def args(self, kind):
        mg.poison_(self.b.t)
        return {"full": (self.b.t.data_ptr(), self.n), "short": (self.b.t.data_ptr(), self.n - 1), "null": (None, self.n)}[kind]

    def intact(self):
        return self.b.intact()


def _ws_for(shape):
    n = int(L().mogan_bn_ws_bytes(*K.dims(shape)))
    assert n > 0
    return _WS(n)


def _verify(g, ref, bnd, kind, what, rel=None, keep=None):
    """per element within the bound (and the memory contract of the buffer); rel: the whole-tensor rel-L2 figure over `keep`
    (indices of the ordinary channels along the channel dimension)"""
    got = g.view.cpu().double()
    ref = ref.double().reshape(got.shape)
    bnd = (bnd if torch.is_tensor(bnd) else torch.full_like(ref, float(bnd))).double().reshape(got.shape)
    err = (got - ref).abs()
    frac = float(torch.nan_to_num(err / bnd.clamp_min(1e-300), nan=float("inf")).max())
    FIG[kind] = max(FIG.get(kind, 0.0), frac)
    g.check(ref, bnd, what="%s (largest err / bound %.3f)" % (what, frac))
    if rel is not None and keep is not None and len(keep):
        dim = 0 if got.dim() == 1 else 1
        idx = torch.tensor(keep)
        a, b = got.index_select(dim, idx), ref.index_select(dim, idx)
        r = float((a - b).norm() / (b.norm() + 1e-30))
        assert r <= rel, "%s: rel-L2 %.3e > %.1e" % (what, r, rel)


def _same_bits(a, b, what):
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "%s: other bits" % what


def _ordinary(shape, act):
    """(x channels, y channels) that are neither constant nor on the large offset (nor, for GLU, paired with one)"""
    B, C, HW = K.dims(shape)
    if B * HW == 1:
        return [], []
    special = {0} | ({C - 1} if K.kind_of(act) == "lin" else set())
    if act != K.GLU:
        keep = [c for c in range(C) if c not in special]
        return keep, keep
    Cy = C // 2
    ys = [c for c in range(Cy) if c not in special and c + Cy not in special]
    return ys + [c + Cy for c in ys], ys


@functools.lru_cache(maxsize=None)
def _dev(shape, act, res=False):
    """a row's references and its inputs on the device, shared by the tests"""
    d = K.bn_case(shape, act, res)
    inp = d["inp"]
    return dict(d, x=_inp(inp["x"]), gamma=_inp(inp["gamma"]), beta=_inp(inp["beta"]), dyd=_inp(d["dy"]),
                resd=None if d["res"] is None else _inp(d["res"]))


def _frozen(d, what):
    for k in ("x", "gamma", "beta", "dyd", "resd"):
        if d.get(k) is not None:
            d[k].frozen.check(what)


# ----------------------------------------------------------------------------- mogan_bn_act_fwd_fused / mogan_bn_act_bwd
def _fwd_outs(shape, act, d, rm=True, rv=True):
    B, C, HW = K.dims(shape)
    Cy = C // 2 if act == K.GLU else C
    return dict(y=_out((B, Cy, HW)), mean=_out((C,)), invstd=_out((C,)), rm=_out((C,), d["inp"]["rm"]) if rm else None,
                rv=_out((C,), d["inp"]["rv"]) if rv else None)


def _fwd(shape, act, d, o, wsp, wsn):
    rc = L().mogan_bn_act_fwd_fused(d["x"].ptr, d["gamma"].ptr, d["beta"].ptr, _p(d["resd"]), _p(o["rm"]), _p(o["rv"]), o["mean"].ptr,
                                    o["invstd"].ptr, o["y"].ptr, *K.dims(shape), act, SLOPE, EPS, MOM, wsp, wsn, lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _written(o):
    for k, g in o.items():
        if g is not None:
            assert g.problems() == [], (k, g.problems())


@pytest.mark.parametrize("shape,act,res", K.BN_CALLS, ids=lambda v: str(v).replace(" ", ""))
def test_bn_act_fwd_fused(shape, act, res):
    d = _dev(shape, act, res)
    ref, S, Fx = d["ref"], d["S"], d["F"]
    path, what = K.path_of(shape), "fwd_fused %s %s" % (shape, K.ACT_NAMES[act])
    ws = _ws_for(shape)
    keep_x, keep_y = _ordinary(shape, act)
    o = _fwd_outs(shape, act, d)
    assert _fwd(shape, act, d, o, *ws.args("full")) == 0, what
    assert ws.intact(), what
    _frozen(d, what)
    _verify(o["y"], ref["y"], K.bound("y", S, Fx), "y", what + " y", 5e-6, keep_y)
    _verify(o["mean"], ref["mean"], K.bound("mean", S, Fx), "mean", what + " mean")
    _verify(o["invstd"], ref["invstd"], K.bound("invstd", S, Fx), "invstd", what + " invstd")
    _verify(o["rm"], ref["rm"], K.bound("rm", S, Fx), "running_mean", what + " running_mean", 1e-6, list(range(shape[1])))
    _verify(o["rv"], ref["rv"], K.bound("rv", S, Fx), "running_var", what + " running_var", 1e-6, list(range(shape[1])))
    RAN.add((path, act, "fwd"))
    first = {k: g.view.clone() for k, g in o.items()}
    # the same call again: same bits
    for g in o.values():
        g.reset()
    assert _fwd(shape, act, d, o, *ws.args("full")) == 0 and ws.intact(), what
    _written(o)
    for k, g in o.items():
        _same_bits(first[k], g.view, what + " second call " + k)
    # one byte less, or no workspace
    for kind in ("short", "null"):
        for g in o.values():
            g.reset()
        rc = _fwd(shape, act, d, o, *ws.args(kind))
        assert ws.intact(), what
        if path == "one":
            assert rc == 0, "%s: the one-launch shapes do not need the workspace (%s: %d)" % (what, kind, rc)
            _written(o)
            for k, g in o.items():
                _same_bits(first[k], g.view, "%s ws %s %s" % (what, kind, k))
        else:
            assert rc == ERR_WS, "%s ws %s: return code %d" % (what, kind, rc)
            assert all(g.untouched() for g in o.values()), "%s ws %s: MOGAN_ERR_WS, but an output was written" % (what, kind)
    if d["x"].view.numel() > BIG:
        return
    # NULL running buffers, also one at a time: everything else as with them
    for rm, rv in ((False, False), (True, False), (False, True)):
        o2 = _fwd_outs(shape, act, d, rm, rv)
        assert _fwd(shape, act, d, o2, *ws.args("full")) == 0 and ws.intact(), what
        _written(o2)
        for k, g in o2.items():
            if g is not None:
                _same_bits(first[k], g.view, "%s running_mean %s running_var %s: %s" % (what, rm, rv, k))
    _frozen(d, what)


@pytest.mark.parametrize("shape,act,res", K.BN_CALLS, ids=lambda v: str(v).replace(" ", ""))
def test_bn_act_bwd(shape, act, res):
    d = _dev(shape, act, res)
    ref, S, Fx = d["ref"], d["S"], d["F"]
    B, C, HW = K.dims(shape)
    path, what = K.path_of(shape), "bwd %s %s" % (shape, K.ACT_NAMES[act])
    ws = _ws_for(shape)
    keep_x, _ = _ordinary(shape, act)
    # the statistics the forward leaves (fp32 roundings of the fp64 ones: the bounds take them as that)
    mean, invstd = _inp(ref["mean"].float()), _inp(ref["invstd"].float())
    base = {"dgamma": K.T("bnbase_g%s" % (shape,), (C,)), "dbeta": K.T("bnbase_b%s" % (shape,), (C,))}

    def outs(accumulate=0, dgamma=True, dbeta=True):
        return dict(dx=_out((B, C, HW)), dgamma=_out((C,), base["dgamma"] if accumulate else None) if dgamma else None,
                    dbeta=_out((C,), base["dbeta"] if accumulate else None) if dbeta else None)

    def call(o, accumulate, wsp, wsn):
        rc = L().mogan_bn_act_bwd(d["x"].ptr, d["dyd"].ptr, mean.ptr, invstd.ptr, d["gamma"].ptr, d["beta"].ptr, o["dx"].ptr, _p(o["dgamma"]),
                                  _p(o["dbeta"]), B, C, HW, act, SLOPE, accumulate, wsp, wsn, lib.stream_ptr())
        torch.cuda.synchronize()
        assert ws.intact(), what
        _frozen(d, what); mean.frozen.check(what); invstd.frozen.check(what)
        return rc

    o = outs()
    assert call(o, 0, *ws.args("full")) == 0, what
    _verify(o["dx"], ref["dx"], K.bound("dx", S, Fx), "dx", what + " dx", 2e-5, keep_x)
    _verify(o["dgamma"], ref["dgamma"], K.bound("dgamma", S, Fx), "dgamma", what + " dgamma", 2e-5, keep_x)
    _verify(o["dbeta"], ref["dbeta"], K.bound("dbeta", S, Fx), "dbeta", what + " dbeta", 2e-5, keep_x)
    RAN.add((path, act, "bwd"))
    first = {k: g.view.clone() for k, g in o.items()}
    for g in o.values():
        g.reset()
    assert call(o, 0, *ws.args("full")) == 0, what
    _written(o)
    for k, g in o.items():
        _same_bits(first[k], g.view, what + " second call " + k)
    # the backward needs its workspace on every path
    for kind in ("short", "null"):
        for g in o.values():
            g.reset()
        rc = call(o, 0, *ws.args(kind))
        assert rc == ERR_WS, "%s ws %s: return code %d" % (what, kind, rc)
        assert all(g.untouched() for g in o.values()), "%s ws %s: MOGAN_ERR_WS, but an output was written" % (what, kind)
    # accumulate = 1 into non-zero parameter gradients
    oa = outs(1)
    assert call(oa, 1, *ws.args("full")) == 0, what
    _same_bits(first["dx"], oa["dx"].view, what + " accumulate dx")
    assert oa["dx"].problems() == []
    for k in ("dgamma", "dbeta"):
        _verify(oa[k], ref[k] + base[k].double(), K.bound(k, S, Fx, base[k]), k, "%s accumulate %s" % (what, k))
    if d["x"].view.numel() > BIG:
        return
    # NULL dgamma / dbeta: everything else as with them
    for dg, db in ((False, False), (True, False), (False, True)):
        o2 = outs(0, dg, db)
        assert call(o2, 0, *ws.args("full")) == 0, what
        _written(o2)
        for k, g in o2.items():
            if g is not None:
                _same_bits(first[k], g.view, "%s dgamma %s dbeta %s: %s" % (what, dg, db, k))


# -------------------------------------------------- mogan_bn_stats, mogan_bn_act_fwd (given statistics), mogan_bn_running_update
SMALL_SHAPES = [s for s in K.ONE_LAUNCH + K.TWO_LAUNCH + K.THREE_LAUNCH + K.BN1D if K.dims(s)[0] * K.dims(s)[1] * K.dims(s)[2] <= BIG]


@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_bn_stats_alone(shape):
    """the statistics half on its own, on every shape whatever path the fused entry gives it (HW == 1: the thread-per-channel kernel)"""
    d = _dev(shape, K.NONE)
    ref, S, Fx = d["ref"], d["S"], d["F"]
    B, C, HW = K.dims(shape)
    ws = _ws_for(shape)
    what = "bn_stats %s" % (shape,)
    first = None
    for rm, rv, kind in ((True, True, "full"), (True, True, "full"), (False, False, "full"), (True, False, "full"), (False, True, "full"),
                         (True, True, "short"), (True, True, "null")):
        o = dict(mean=_out((C,)), invstd=_out((C,)), rm=_out((C,), d["inp"]["rm"]) if rm else None, rv=_out((C,), d["inp"]["rv"]) if rv else None)
        wsp, wsn = ws.args(kind)
        rc = L().mogan_bn_stats(d["x"].ptr, B, C, HW, EPS, MOM, o["mean"].ptr, o["invstd"].ptr, _p(o["rm"]), _p(o["rv"]), wsp, wsn, lib.stream_ptr())
        torch.cuda.synchronize()
        assert ws.intact(), what
        d["x"].frozen.check(what)
        if kind != "full":
            assert rc == ERR_WS and all(g.untouched() for g in o.values() if g is not None), "%s ws %s: %d" % (what, kind, rc)
            continue
        assert rc == 0, what
        if first is None:
            for k, name in (("mean", "mean"), ("invstd", "invstd"), ("rm", "running_mean"), ("rv", "running_var")):
                _verify(o[k], ref[k], K.bound(k, S, Fx), name, "%s %s" % (what, k))
            first = {k: g.view.clone() for k, g in o.items()}
            RAN.add(("stats", K.stats_kernel(shape), "fwd"))
            continue
        _written(o)
        for k, g in o.items():
            if g is not None:
                _same_bits(first[k], g.view, "%s running_mean %s running_var %s: %s" % (what, rm, rv, k))


@pytest.mark.parametrize("shape,act", [(s, a) for s, a in K.BN_ROWS if s in SMALL_SHAPES], ids=lambda v: str(v).replace(" ", ""))
def test_bn_act_fwd_with_given_statistics(shape, act):
    """the apply half on its own: both forms of bn_act_fwd_kernel (HW % 4 == 0: four values per thread), with and without residual"""
    B, C, HW = K.dims(shape)
    for res in ((False, True) if act == K.NONE else (False,)):
        d = _dev(shape, act, res)
        mean32, invstd32 = d["ref"]["mean"].float(), d["ref"]["invstd"].float()
        inp = d["inp"]
        ref, S, Fx, _ = K.bn_forward(inp["x"], inp["gamma"], inp["beta"], act, d["res"], mean=mean32, invstd=invstd32)
        mean, invstd = _inp(mean32), _inp(invstd32)
        what = "bn_act_fwd %s %s res %s" % (shape, K.ACT_NAMES[act], res)
        y = _out(ref["y"].shape)
        first = None
        for _ in range(2):
            rc = L().mogan_bn_act_fwd(d["x"].ptr, mean.ptr, invstd.ptr, d["gamma"].ptr, d["beta"].ptr, _p(d["resd"]), y.ptr, B, C, HW, act, SLOPE,
                                      lib.stream_ptr())
            torch.cuda.synchronize()
            assert rc == 0, what
            _frozen(d, what); mean.frozen.check(what); invstd.frozen.check(what)
            if first is None:
                _verify(y, ref["y"], K.bound("y", S, Fx), "y", what, 5e-6, _ordinary(shape, act)[1])
                first = y.view.clone()
                y.reset()
            else:
                assert y.problems() == []
                _same_bits(first, y.view, what + " second call")
        RAN.add(("apply", "vec4" if HW % 4 == 0 else "scalar", act, res))


@pytest.mark.parametrize("shape", [(16, 24), (5, 300), (4, 8, 8, 8), (1, 3)], ids=lambda v: str(v).replace(" ", ""))
def test_bn_running_update(shape):
    """the deferred update from the statistics a call left: both buffers, each alone, both NULL.  The variance is 1 / invstd^2 - eps
    of the fp32 invstd it is given, in fp64: that IS the input, so the reference does the same and the bound is the update's
    three roundings and the one of the unbiased variance."""
    d = K.bn_case(shape, K.NONE)
    B, C, HW = K.dims(shape)
    n = B * HW
    mean32, invstd32 = d["ref"]["mean"].float(), d["ref"]["invstd"].float()
    var = (1.0 / invstd32.double() ** 2 - K.EPS).clamp_min(0)
    unb = var * n / (n - 1.0) if n > 1 else var
    mean, invstd = _inp(mean32), _inp(invstd32)
    first = {}
    for rm, rv in ((True, True), (True, False), (False, True), (False, False)):
        o = dict(rm=_out((C,), d["inp"]["rm"]) if rm else None, rv=_out((C,), d["inp"]["rv"]) if rv else None)
        rc = L().mogan_bn_running_update(mean.ptr, invstd.ptr, _p(o["rm"]), _p(o["rv"]), C, n, EPS, MOM, lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0
        mean.frozen.check("running_update"); invstd.frozen.check("running_update")
        for k, batch, Fb in (("rm", mean32.double(), 0.0), ("rv", unb, K.EPS32 * unb + K.U64 * 4 / invstd32.double() ** 2)):
            if o[k] is None:
                continue
            r = d["inp"][k].double()
            want = K.ONE_MINUS_MOM * r + K.MOM * batch
            bnd = 3 * K.EPS32 * ((K.ONE_MINUS_MOM * r).abs() + (K.MOM * batch).abs()) + K.MOM * Fb
            _verify(o[k], want, bnd, "running_update", "running_update %s %s" % (shape, k))
            if k in first:
                _same_bits(first[k], o[k].view, "running_update %s alone" % k)
            first.setdefault(k, o[k].view.clone())
    RAN.add(("running_update",))


# ------------------------------------------------------------------------------------ mogan_bn_act_grouped_fwd / _bwd
@pytest.mark.parametrize("shape", K.GROUPED, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("act", K.BN_ACTS)
def test_bn_act_grouped(shape, act):
    """G calls in one launch each way: against fp64, and for HW >= 16 bit for bit what G calls of mogan_bn_act_fwd_fused / _bwd give on
    the group slices, statistics and running buffers included"""
    G = shape[0]
    B, C, HW = K.dims(shape[1:])
    assert L().mogan_bn_act_grouped_eligible(G, B, C, HW) == 1
    assert L().mogan_bn_act_grouped_eligible(K.GROUPED_INELIGIBLE[0], *K.dims(K.GROUPED_INELIGIBLE[1:])) == 0
    Cy = C // 2 if act == K.GLU else C
    inp = K.bn_inputs(shape[1:], K.kind_of(act), G)
    dy = K.bn_dy(shape[1:], act, G)
    ref, bnd = K.grouped_reference(inp["x"], inp["gamma"], inp["beta"], act, inp["rm"], inp["rv"], dy, G)
    x, gamma, beta, dyd = _inp(inp["x"]), _inp(inp["gamma"]), _inp(inp["beta"]), _inp(dy)
    what = "grouped %s %s" % (shape, K.ACT_NAMES[act])
    st = lib.stream_ptr()
    keep_x, keep_y = _ordinary(shape[1:], act)
    rel = {"y": (5e-6, keep_y), "mean": (None, None), "invstd": (None, None), "rm": (1e-6, list(range(C))), "rv": (1e-6, list(range(C))),
           "dx": (2e-5, keep_x), "dgamma": (2e-5, keep_x), "dbeta": (2e-5, keep_x)}

    def frozen():
        for t in (x, gamma, beta, dyd):
            t.frozen.check(what)

    o = dict(y=_out((G * B, Cy, HW)), mean=_out((G, C)), invstd=_out((G, C)), rm=_out((C,), inp["rm"]), rv=_out((C,), inp["rv"]))
    first = None
    for _ in range(2):
        rc = L().mogan_bn_act_grouped_fwd(x.ptr, gamma.ptr, beta.ptr, o["rm"].ptr, o["rv"].ptr, o["mean"].ptr, o["invstd"].ptr, o["y"].ptr, G, B, C, HW,
                                          act, SLOPE, EPS, MOM, st)
        torch.cuda.synchronize()
        assert rc == 0, what
        frozen()
        if first is None:
            for k, name in (("y", "y"), ("mean", "mean"), ("invstd", "invstd"), ("rm", "running_mean"), ("rv", "running_var")):
                _verify(o[k], ref[k], bnd[k], name, "%s %s" % (what, k), *rel[k])
            first = {k: g.view.clone() for k, g in o.items()}
            for g in o.values():
                g.reset()
        else:
            _written(o)
            for k, g in o.items():
                _same_bits(first[k], g.view, what + " second call " + k)
    mean, invstd = _inp(first["mean"].cpu()), _inp(first["invstd"].cpu())
    base = {"dgamma": K.T("gbase_g%s" % (shape,), (C,)), "dbeta": K.T("gbase_b%s" % (shape,), (C,))}
    firstb = None
    for accumulate in (0, 0, 1):
        ob = dict(dx=_out((G * B, C, HW)), dgamma=_out((C,), base["dgamma"] if accumulate else None),
                  dbeta=_out((C,), base["dbeta"] if accumulate else None))
        rc = L().mogan_bn_act_grouped_bwd(x.ptr, dyd.ptr, mean.ptr, invstd.ptr, gamma.ptr, beta.ptr, ob["dx"].ptr, ob["dgamma"].ptr, ob["dbeta"].ptr,
                                          G, B, C, HW, act, SLOPE, accumulate, st)
        torch.cuda.synchronize()
        assert rc == 0, what
        frozen(); mean.frozen.check(what); invstd.frozen.check(what)
        if firstb is None:
            for k in ("dx", "dgamma", "dbeta"):
                _verify(ob[k], ref[k], bnd[k], k, "%s %s" % (what, k), *rel[k])
            firstb = {k: g.view.clone() for k, g in ob.items()}
        elif not accumulate:
            _written(ob)
            for k, g in ob.items():
                _same_bits(firstb[k], g.view, what + " second call " + k)
        else:
            _same_bits(firstb["dx"], ob["dx"].view, what + " accumulate dx")
            for k in ("dgamma", "dbeta"):
                _verify(ob[k], ref[k] + base[k].double(), bnd[k] + 2 * K.EPS32 * (base[k].double().abs() + bnd[k] / K.EPS32), k,
                        "%s accumulate %s" % (what, k))
    RAN.add(("grouped", act))
    if HW < 16:
        return          # (the one-group entry gives these shapes to the three-launch kernels: another summation split)
    # bit for bit the G calls on the slices
    ws = _ws_for((B, C, HW))
    lo = dict(y=_out((G * B, Cy, HW)), mean=_out((G, C)), invstd=_out((G, C)), rm=_out((C,), inp["rm"]), rv=_out((C,), inp["rv"]),
              dx=_out((G * B, C, HW)), dgamma=_out((C,)), dbeta=_out((C,)))
    for g in range(G):
        xg = x.ptr + 4 * g * B * C * HW
        rc = L().mogan_bn_act_fwd_fused(xg, gamma.ptr, beta.ptr, None, lo["rm"].ptr, lo["rv"].ptr, lo["mean"].ptr + 4 * g * C, lo["invstd"].ptr + 4 * g * C,
                                        lo["y"].ptr + 4 * g * B * Cy * HW, B, C, HW, act, SLOPE, EPS, MOM, *ws.args("full"), st)
        assert rc == 0
        rc = L().mogan_bn_act_bwd(xg, dyd.ptr + 4 * g * B * Cy * HW, mean.ptr + 4 * g * C, invstd.ptr + 4 * g * C, gamma.ptr, beta.ptr,
                                  lo["dx"].ptr + 4 * g * B * C * HW, lo["dgamma"].ptr, lo["dbeta"].ptr, B, C, HW, act, SLOPE, 1 if g else 0,
                                  *ws.args("full"), st)
        assert rc == 0
    torch.cuda.synchronize()
    assert ws.intact()
    _written(lo)
    for k, g in lo.items():
        _same_bits((first.get(k) if k in first else firstb[k]), g.view, "%s against the G calls: %s" % (what, k))


# ------------------------------------------------------------- mogan_affine_act_fwd / _bwd, mogan_affine_relu_bwd_out
def _twice(call, out, ref, bnd, kind, what, rel=None):
    """one output of an entry point without workspace: verified, then the same call again for the same bits"""
    assert call(out) == 0, what
    torch.cuda.synchronize()
    _verify(out, ref, bnd, kind, what, rel, list(range(ref.shape[1])) if rel and ref.dim() > 1 else list(range(ref.shape[0])) if rel else None)
    first = out.view.clone()
    out.reset()
    assert call(out) == 0, what
    torch.cuda.synchronize()
    assert out.problems() == [], what
    _same_bits(first, out.view, what + " second call")


@pytest.mark.parametrize("shape", K.AFFINE, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("act", [K.NONE, K.RELU, K.LRELU])
def test_affine_act(shape, act):
    B, C, HW = K.dims(shape)
    d = K.affine_inputs(shape, act)
    ref, S, Fx = K.affine_reference(d["x"], d["scale"], d["shift"], act, d["dy"])
    x, scale, shift, dy = _inp(d["x"]), _inp(d["scale"]), _inp(d["shift"]), _inp(d["dy"])
    st = lib.stream_ptr()
    what = "affine %s %s" % (shape, K.ACT_NAMES[act])
    _twice(lambda o: L().mogan_affine_act_fwd(x.ptr, scale.ptr, shift.ptr, o.ptr, B, C, HW, act, SLOPE, st), _out((B, C, HW)), ref["y"],
           K.bound("y", S, Fx), "affine y", what + " y", 5e-6)
    _twice(lambda o: L().mogan_affine_act_bwd(x.ptr, dy.ptr, scale.ptr, shift.ptr, o.ptr, B, C, HW, act, SLOPE, st), _out((B, C, HW)), ref["dx"],
           Fx["dx"], "affine dx", what + " dx", 2e-5)
    for t in (x, scale, shift, dy):
        t.frozen.check(what)
    RAN.add(("affine", act, len(K.chunks(shape, act))))


@pytest.mark.parametrize("shape", K.AFFINE, ids=lambda v: str(v).replace(" ", ""))
def test_affine_relu_bwd_out(shape):
    """dx = dy * scale[c] * (y > 0) from the OUTPUT y: exact zeros where the ReLU cut, one rounding elsewhere"""
    B, C, HW = K.dims(shape)
    y = K.T("aro%s" % (shape,), (B, C, HW)).clamp_min(0)
    dyt, scale = K.T("arg%s" % (shape,), (B, C, HW)), K.T("ars%d" % C, (C,), 0.5, 1.0)
    ref = torch.where(y > 0, dyt.double() * scale.double().view(1, -1, 1), torch.zeros((), dtype=torch.float64))
    yd, dyd, sd = _inp(y), _inp(dyt), _inp(scale)
    _twice(lambda o: L().mogan_affine_relu_bwd_out(yd.ptr, dyd.ptr, sd.ptr, o.ptr, B, C, HW, lib.stream_ptr()), _out((B, C, HW)), ref,
           K.EPS32 * ref.abs(), "affine dx", "affine_relu_bwd_out %s" % (shape,), 2e-5)
    for t in (yd, dyd, sd):
        t.frozen.check("affine_relu_bwd_out")
    RAN.add(("affine_relu_bwd_out",))


# ------------------------------------------------------------------------------------------------ mogan_act_fwd / _bwd
@pytest.mark.parametrize("shape", K.AFFINE + [K.GLU_C2], ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("act", [K.RELU, K.LRELU, K.GLU, K.TANH, K.SIGMOID])
def test_act(shape, act):
    B, C, HW = K.dims(shape)
    Cy = C // 2 if act == K.GLU else C
    xt, dyt = K.T("actx%s" % (shape,), (B, C, HW), 1.5, 0.3), K.T("actg%s%d" % (shape, act), (B, Cy, HW))
    ref, Fx = K.act_reference(xt, act, dyt)
    x, dy = _inp(xt), _inp(dyt)
    st = lib.stream_ptr()
    what = "act %s %s" % (shape, K.ACT_NAMES[act])
    _twice(lambda o: L().mogan_act_fwd(x.ptr, o.ptr, B, C, HW, act, SLOPE, st), _out((B, Cy, HW)), ref["y"], Fx["y"], "act y", what + " y", 2e-6)
    _twice(lambda o: L().mogan_act_bwd(x.ptr, dy.ptr, o.ptr, B, C, HW, act, SLOPE, st), _out((B, C, HW)), ref["dx"], Fx["dx"], "act dx", what + " dx",
           2e-6)
    x.frozen.check(what); dy.frozen.check(what)
    RAN.add(("act", act))


# ---------------------------------------------------------------------------------------- mogan_bias_add / mogan_bias_grad
@pytest.mark.parametrize("shape", K.AFFINE + [(5, 300)], ids=lambda v: str(v).replace(" ", ""))
def test_bias_add_and_grad(shape):
    """y += bias[c] in place (an accumulate-mode buffer); dbias[c] (+)= the fp64 sum over rows and HW, rounded once"""
    B, C, HW = K.dims(shape)
    y0, bias, dyt = K.T("biy%s" % (shape,), (B, C, HW)), K.T("bib%d" % C, (C,), 0.3), K.T("big%s" % (shape,), (B, C, HW))
    bd, dyd = _inp(bias), _inp(dyt)
    st = lib.stream_ptr()
    want = y0.double() + bias.double().view(1, -1, 1)
    _twice(lambda o: L().mogan_bias_add(o.ptr, bd.ptr, B, C, HW, st), _out((B, C, HW), y0), want, K.EPS32 * want.abs(), "bias", "bias_add %s" % (shape,))
    s = dyt.double().sum((0, 2))
    _twice(lambda o: L().mogan_bias_grad(dyd.ptr, o.ptr, B, C, HW, 0, st), _out((C,)), s, K.EPS32 * s.abs(), "bias", "bias_grad %s" % (shape,), 2e-6)
    base = K.T("bibase%d" % C, (C,))
    _twice(lambda o: L().mogan_bias_grad(dyd.ptr, o.ptr, B, C, HW, 1, st), _out((C,), base), s + base.double(),
           K.EPS32 * s.abs() + 2 * K.EPS32 * (base.double().abs() + s.abs()), "bias", "bias_grad accumulate %s" % (shape,))
    bd.frozen.check("bias"); dyd.frozen.check("bias")
    RAN.add(("bias",))


# ------------------------------------------------------------------------------------------------------------------ census
def test_census_of_paths_activations_and_directions():
    """every (path, activation, direction) of the table ran, every entry point beside them, both forms of the apply kernel with and
    without residual, both statistics kernels, one and two batch chunks of the affine kernel; prints the largest err / bound"""
    for k in sorted(FIG):
        print("%-16s largest err / bound = %.3f" % (k, FIG[k]))
    want = {(p, a, d) for p in ("one", "two", "three") for a in K.BN_ACTS for d in ("fwd", "bwd")}
    want |= {("stats", k, "fwd") for k in ("per-channel-thread", "per-slab-block")}
    want |= {("apply", v, a, False) for v in ("vec4", "scalar") for a in K.BN_ACTS} | {("apply", v, K.NONE, True) for v in ("vec4", "scalar")}
    want |= {("grouped", a) for a in K.BN_ACTS} | {("running_update",), ("affine_relu_bwd_out",), ("bias",)}
    want |= {("affine", a, n) for a in (K.NONE, K.RELU, K.LRELU) for n in (1, 2)}
    want |= {("act", a) for a in (K.RELU, K.LRELU, K.GLU, K.TANH, K.SIGMOID)}
    if not RAN:
        pytest.skip("the census needs the tests of this module to have run (a selection was made)")
    assert not want - RAN, "never ran: %s" % sorted(want - RAN, key=str)
    assert all(v <= 1.0 for v in FIG.values()), FIG
