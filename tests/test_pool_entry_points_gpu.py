"""-m gpu: the pooling, resize, sum and feeder entry points of include/mogan_hip.h through ctypes, per element against fp64 (or bit
for bit) and under the memory contract of tests/memguard.py -- what tests/test_bn_entry_points_gpu.py does for the batch-norm
family.  Rows, inputs, references and bounds are tests/pool_cases.py; tests/test_pool_reference_cpu.py derives the tolerances
without a GPU (and holds the Pillow comparison); tests/test_pool_rejections_cpu.py holds every rejection that is answered before
a launch.

Memory, every call:
  * every output -- y, idx, dx, q, tmp, out -- is the payload of a guard-banded buffer, NaN-poisoned (bytes: 0xFF); afterwards
    every element is written, within its bound or exact, and nothing outside changed.  tmp is exactly B * S * OS * 3 bytes
    between its bands;
  * every input -- params, bounds, kk and idx included -- lives in sentinel bands and is bitwise unchanged afterwards, bands included;
  * the same call a second time into the poisoned buffer again gives the same bits;
  * some rejections of the CPU table are repeated with these buffers: MOGAN_ERR_SHAPE and every output untouched.
The large mogan_add case (the grid-stride loop's second trip) is generated and compared on the device.
The `long long` instantiations behind POOL_LAUNCH need 2^31 elements and stay unrun.
The last test asserts the census (entry point x row ran) and prints the largest err / bound per kind."""
import time

import pytest
import torch

import memguard as mg
import pool_cases as K
from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import feeder  # noqa: E402
from mogan_amd.hip import lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPE = -1
ids = lambda v: str(v).replace(" ", "")  # noqa: E731

RAN = set()            # (entry point, row)
FIG = {}               # kind -> largest err / bound


def L():
    return lib.load()


def _inp(t):
    """an input (fp32, uint8 or int32) inside sentinel bands, frozen (bands included)"""
    g = mg.Guarded(tuple(t.shape), (Ellipsis,), DEV, dtype=t.dtype, base=t)
    g.frozen = mg.Frozen(g.buf)
    return g


def _out(shape, dtype=torch.float32):
    return mg.Guarded(tuple(shape), (Ellipsis,), DEV, dtype=dtype)


def _bits_equal(a, b):
    return torch.equal(mg._bits(a.contiguous()), mg._bits(b.contiguous()))


def _twice(call, outs, what):
    """the call into the poisoned outputs, twice: return code 0 both times and the same bits"""
    rc = call()
    torch.cuda.synchronize()
    assert rc == 0, "%s: return code %d" % (what, rc)
    first = {k: g.view.clone() for k, g in outs.items()}
    for g in outs.values():
        g.reset()
    rc = call()
    torch.cuda.synchronize()
    assert rc == 0, "%s: return code %d the second time" % (what, rc)
    for k, g in outs.items():
        assert _bits_equal(first[k], g.view), "%s: %s has other bits the second time" % (what, k)


def _declined(calls, outs, what):
    """every call is refused and has written nothing"""
    for g in outs:
        g.reset()
    for name, call in calls:
        rc = call()
        torch.cuda.synchronize()
        assert rc == SHAPE, "%s, %s: return code %d" % (what, name, rc)
        assert all(g.untouched() for g in outs), "%s, %s: MOGAN_ERR_SHAPE, but an output was written" % (what, name)


def _within(g, ref, bnd, kind, what):
    """every element written and within its bound (exact, and +0 for a zero, where the bound is 0); nothing outside changed"""
    got = g.view.cpu().double()
    ref = ref.double().reshape(got.shape)
    bnd = bnd.double().expand(got.shape) if bnd.dim() == got.dim() else bnd.double().reshape(got.shape)
    err = (got - ref).abs()
    pos = bnd > 0
    frac = float(torch.nan_to_num(err[pos] / bnd[pos], nan=float("inf")).max()) if bool(pos.any()) else 0.0
    FIG[kind] = max(FIG.get(kind, 0.0), frac)
    g.check(ref, bnd, what="%s (largest err / bound %.3f)" % (what, frac))
    zero = ~pos & (ref == 0)
    assert not bool(torch.signbit(g.view.cpu()[zero]).any()), "%s: -0 where nothing contributes" % what


def _exact(g, want, what, written=True):
    g.check(want, exact=True, what=what, written=written)


def _frozen(inputs, what):
    for t in inputs:
        t.frozen.check(what)


# ------------------------------------------------------------------------------------------------------------ average pool
@pytest.mark.parametrize("row", K.AVG_ROWS, ids=ids)
def test_avgpool(row):
    P, H, W, k, s, pad = row
    d = K.avg_case(row)
    OH, OW = d["OH"], d["OW"]
    x, dy = _inp(d["x"]), _inp(d["dy"])
    y, dx = _out((P, OH, OW)), _out((P, H, W))
    st = lib.stream_ptr()
    what = "avgpool %s" % (row,)
    _twice(lambda: L().mogan_avgpool_fwd(x.ptr, y.ptr, P, H, W, k, s, pad, st), {"y": y}, what + " fwd")
    _within(y, d["y"], K.TOL["avg"] * d["y_bound"], "avgpool y", what + " y")
    RAN.add(("mogan_avgpool_fwd", row))
    _twice(lambda: L().mogan_avgpool_bwd(dy.ptr, dx.ptr, P, H, W, k, s, pad, st), {"dx": dx}, what + " bwd")
    _within(dx, d["dx"], d["dx_bound"], "avgpool dx", what + " dx")
    assert int((d["dx_bound"] == 0).sum()) == P * int((~d["covered"]).sum())
    RAN.add(("mogan_avgpool_bwd", row))
    # the channel-slice entry without mask and accumulation is the same call
    first = dx.view.clone()
    dx.reset()
    assert L().mogan_avgpool_bwd_ex(dy.ptr, dx.ptr, None, 0, P, H, W, k, s, pad, st) == 0
    torch.cuda.synchronize()
    assert dx.problems() == [] and _bits_equal(first, dx.view), what + " bwd_ex"
    _frozen((x, dy), what)
    fwd = lambda **c: (lambda a: L().mogan_avgpool_fwd(a["x"], a["y"], a["P"], a["H"], a["W"], a["k"], a["s"], a["pad"], st))(
        dict(dict(x=x.ptr, y=y.ptr, P=P, H=H, W=W, k=k, s=s, pad=pad), **c))
    bwd = lambda **c: (lambda a: L().mogan_avgpool_bwd(a["dy"], a["dx"], a["P"], a["H"], a["W"], a["k"], a["s"], a["pad"], st))(
        dict(dict(dy=dy.ptr, dx=dx.ptr, P=P, H=H, W=W, k=k, s=s, pad=pad), **c))
    bad = [("s = 0", dict(s=0)), ("k = 0", dict(k=0)), ("pad < 0", dict(pad=-1)), ("2 pad > k", dict(pad=k)),
           ("H + 2 pad < k (truncating division)", dict(H=2, W=8, k=3, s=2, pad=0))]
    _declined([(n, lambda c=c: fwd(**c)) for n, c in bad] + [("NULL x", lambda: fwd(x=None)), ("NULL y", lambda: fwd(y=None))] +
              [(n, lambda c=c: bwd(**c)) for n, c in bad] + [("NULL dy", lambda: bwd(dy=None)), ("NULL dx", lambda: bwd(dx=None))],
              (y, dx), what)
    _frozen((x, dy), what)


# ----------------------------------------------------------------------------------------------------------------- max pool
@pytest.mark.parametrize("row", K.MAX_ROWS + [K.MAX_FWD_ONLY], ids=ids)
def test_maxpool(row):
    P, H, W, k, s = row
    d = K.max_case(row)
    OH, OW = d["OH"], d["OW"]
    x, dy, idx_in = _inp(d["x"]), _inp(d["dy"]), _inp(d["idx"])
    y, idx, dx = _out((P, OH, OW)), _out((P, OH, OW), torch.uint8), _out((P, H, W))
    st = lib.stream_ptr()
    what = "maxpool %s" % (row,)
    _twice(lambda: L().mogan_maxpool_fwd(x.ptr, y.ptr, idx.ptr, P, H, W, k, s, st), {"y": y, "idx": idx}, what + " fwd")
    _exact(y, d["y"], what + " y")
    _exact(idx, d["idx"], what + " idx")
    RAN.add(("mogan_maxpool_fwd", row))
    # without idx: the same y
    first = y.view.clone()
    y.reset()
    assert L().mogan_maxpool_fwd(x.ptr, y.ptr, None, P, H, W, k, s, st) == 0
    torch.cuda.synchronize()
    assert y.problems() == [] and _bits_equal(first, y.view) and idx.problems() == [], what + " fwd, idx = NULL"
    RAN.add(("mogan_maxpool_fwd idx=NULL", row))
    fwd = lambda **c: (lambda a: L().mogan_maxpool_fwd(a["x"], a["y"], a["idx"], a["P"], a["H"], a["W"], a["k"], a["s"], st))(
        dict(dict(x=x.ptr, y=y.ptr, idx=idx.ptr, P=P, H=H, W=W, k=k, s=s), **c))
    bwd = lambda **c: (lambda a: L().mogan_maxpool_bwd(a["idx"], a["dy"], a["dx"], a["P"], a["H"], a["W"], a["k"], a["s"], st))(
        dict(dict(idx=idx_in.ptr, dy=dy.ptr, dx=dx.ptr, P=P, H=H, W=W, k=k, s=s), **c))
    calls = [("fwd k = 0", lambda: fwd(k=0)), ("fwd s = 0", lambda: fwd(s=0)), ("fwd H < k", lambda: fwd(H=k - 1)),
             ("fwd k * k > 255", lambda: fwd(k=16)), ("fwd NULL x", lambda: fwd(x=None)), ("fwd NULL y", lambda: fwd(y=None)),
             ("bwd NULL idx", lambda: bwd(idx=None)), ("bwd NULL dy", lambda: bwd(dy=None)), ("bwd NULL dx", lambda: bwd(dx=None)),
             ("bwd k > 2 s", lambda: bwd(k=2 * s + 1, H=max(H, 2 * s + 1), W=max(W, 2 * s + 1))), ("bwd planes = 0", lambda: bwd(P=0))]
    if k > 2 * s:
        calls.append(("bwd of the forward-only row", lambda: bwd()))
    else:
        # the backward through the oracle's offsets, and through the ones the forward just wrote
        _twice(lambda: bwd(), {"dx": dx}, what + " bwd")
        _within(dx, d["dx"], d["dx_bound"], "maxpool dx", what + " dx")
        first = dx.view.clone()
        dx.reset()
        assert bwd(idx=idx.ptr) == 0
        torch.cuda.synchronize()
        assert dx.problems() == [] and _bits_equal(first, dx.view), what + " bwd through the forward's idx"
        assert idx.problems(d["idx"], exact=True) == []
        RAN.add(("mogan_maxpool_bwd", row))
    _declined(calls, (y, idx, dx), what)
    _frozen((x, dy, idx_in), what)


# ------------------------------------------------------------------------------------------------------------------ bilinear
@pytest.mark.parametrize("row", K.BIL_ROWS, ids=ids)
def test_bilinear(row):
    P, H, W, OH, OW = row
    d = K.bil_case(row)
    x, dy = _inp(d["x"]), _inp(d["dy"])
    y, dx = _out((P, OH, OW)), _out((P, H, W))
    st = lib.stream_ptr()
    what = "bilinear %s" % (row,)
    fwd = lambda **c: (lambda a: L().mogan_bilinear_fwd(a["x"], a["y"], a["P"], a["H"], a["W"], a["OH"], a["OW"], st))(
        dict(dict(x=x.ptr, y=y.ptr, P=P, H=H, W=W, OH=OH, OW=OW), **c))
    bwd = lambda **c: (lambda a: L().mogan_bilinear_bwd(a["dy"], a["dx"], a["P"], a["H"], a["W"], a["OH"], a["OW"], st))(
        dict(dict(dy=dy.ptr, dx=dx.ptr, P=P, H=H, W=W, OH=OH, OW=OW), **c))
    _twice(lambda: fwd(), {"y": y}, what + " fwd")
    _within(y, d["y"], K.TOL["bil"] * d["y_bound"], "bilinear y", what + " y")
    RAN.add(("mogan_bilinear_fwd", row))
    _twice(lambda: bwd(), {"dx": dx}, what + " bwd")
    _within(dx, d["dx"], K.TOL["bil"] * d["dx_bound"], "bilinear dx", what + " dx")
    got = dx.view.cpu()
    assert bool((got[d["unread"]].view(torch.int32) == 0).all()), what + ": dx of an element no output reads is not +0"
    RAN.add(("mogan_bilinear_bwd", row))
    if row == K.BIL_IDENTITY:
        assert _bits_equal(y.view.cpu(), d["x"]) and _bits_equal(got, d["dy"]), what + ": the identity is not bitwise"
    _declined([("fwd planes = 0", lambda: fwd(P=0)), ("fwd OH = 0", lambda: fwd(OH=0)), ("fwd NULL x", lambda: fwd(x=None)),
               ("fwd NULL y", lambda: fwd(y=None)), ("bwd W < 0", lambda: bwd(W=-W)), ("bwd OW = 0", lambda: bwd(OW=0)),
               ("bwd NULL dy", lambda: bwd(dy=None)), ("bwd NULL dx", lambda: bwd(dx=None))], (y, dx), what)
    _frozen((x, dy), what)


# ---------------------------------------------------------------------------------------------------------------------- sums
def _ieee(g, want, what):
    """written, nothing outside changed, and bit for bit the CPU's fp32 result (a NaN for a NaN)"""
    assert g.problems() == [], "%s: %s" % (what, g.problems())
    got = g.view.cpu()
    if not K.same_ieee(got, want):
        bad = (got.view(torch.int32) != want.view(torch.int32)) & ~(torch.isnan(got) & torch.isnan(want))
        sub = bad & (want != 0) & (want.abs() < 2.0 ** -126)
        i = tuple(torch.nonzero(bad)[0].tolist())
        raise AssertionError("%s: %d elements differ from the IEEE result (%d of them where it is subnormal: flushed?); first at %s: "
                             "got %r, want %r" % (what, int(bad.sum()), int(sub.sum()), i, float(got[i]), float(want[i])))


@pytest.mark.parametrize("n", K.SUM_N)
def test_add_and_scale(n):
    ab = K.sum_operands(n, 2)
    a, b = _inp(ab[0].contiguous()), _inp(ab[1].contiguous())
    y = _out((n,))
    st = lib.stream_ptr()
    _twice(lambda: L().mogan_add(a.ptr, b.ptr, y.ptr, n, st), {"y": y}, "add %d" % n)
    _ieee(y, ab[0] + ab[1], "add %d" % n)
    RAN.add(("mogan_add", n))
    for alpha in K.ALPHAS:
        y.reset()
        _twice(lambda: L().mogan_scale(a.ptr, alpha, y.ptr, n, st), {"y": y}, "scale %d by %r" % (n, alpha))
        _ieee(y, ab[0] * torch.tensor(alpha, dtype=torch.float32), "scale %d by %r" % (n, alpha))
        RAN.add(("mogan_scale", n, alpha))
    _declined([("add n < 0", lambda: L().mogan_add(a.ptr, b.ptr, y.ptr, -n, st)), ("add NULL a", lambda: L().mogan_add(None, b.ptr, y.ptr, n, st)),
               ("add NULL b", lambda: L().mogan_add(a.ptr, None, y.ptr, n, st)), ("add NULL y", lambda: L().mogan_add(a.ptr, b.ptr, None, n, st)),
               ("scale n < 0", lambda: L().mogan_scale(a.ptr, 0.5, y.ptr, -1, st)), ("scale NULL a", lambda: L().mogan_scale(None, 0.5, y.ptr, n, st)),
               ("scale NULL y", lambda: L().mogan_scale(a.ptr, 0.5, None, n, st))], (y,), "add / scale %d" % n)
    # an empty tensor: 0, nothing launched, nothing written
    assert L().mogan_add(a.ptr, b.ptr, y.ptr, 0, st) == 0 and L().mogan_scale(None, 0.5, None, 0, st) == 0
    torch.cuda.synchronize()
    assert y.untouched()
    _frozen((a, b), "add / scale %d" % n)


@pytest.mark.parametrize("G", K.SUM_G)
@pytest.mark.parametrize("n", K.SUM_N)
def test_group_sum_and_bcast(n, G):
    xt = K.sum_operands(n, G)
    x = _inp(xt)
    y, dx = _out((n,)), _out((G, n))
    st = lib.stream_ptr()
    what = "group_sum n = %d, G = %d" % (n, G)
    _twice(lambda: L().mogan_group_sum(x.ptr, y.ptr, n, G, st), {"y": y}, what)
    _ieee(y, K.group_sum_reference(xt), what)
    RAN.add(("mogan_group_sum", n, G))
    dy = _inp(xt[0].contiguous())                       # the specials, as a gradient: bitwise copies
    what = "group_bcast n = %d, G = %d" % (n, G)
    _twice(lambda: L().mogan_group_bcast(dy.ptr, dx.ptr, n, G, st), {"dx": dx}, what)
    _ieee(dx, xt[0].expand(G, n).contiguous(), what)
    RAN.add(("mogan_group_bcast", n, G))
    _declined([("group_sum G = 0", lambda: L().mogan_group_sum(x.ptr, y.ptr, n, 0, st)), ("group_sum n < 0", lambda: L().mogan_group_sum(x.ptr, y.ptr, -n, G, st)),
               ("group_sum NULL x", lambda: L().mogan_group_sum(None, y.ptr, n, G, st)), ("group_sum NULL y", lambda: L().mogan_group_sum(x.ptr, None, n, G, st)),
               ("group_bcast G < 0", lambda: L().mogan_group_bcast(dy.ptr, dx.ptr, n, -G, st)), ("group_bcast n < 0", lambda: L().mogan_group_bcast(dy.ptr, dx.ptr, -1, G, st)),
               ("group_bcast NULL dy", lambda: L().mogan_group_bcast(None, dx.ptr, n, G, st)),
               ("group_bcast NULL dx", lambda: L().mogan_group_bcast(dy.ptr, None, n, G, st))], (y, dx), what)
    assert L().mogan_group_sum(x.ptr, y.ptr, 0, G, st) == 0 and L().mogan_group_bcast(None, None, 0, 0, st) == 0
    torch.cuda.synchronize()
    assert y.untouched() and dx.untouched()
    _frozen((x, dy), what)


def test_add_takes_the_second_trip_of_the_grid_stride_loop():
    """n = 262144 * 256 + 257: the grid is capped at 262144 blocks, so the first 257 threads add a second element.  Generated and
    compared on the device (three 256 MB tensors); prints what it took."""
    n = K.ADD_LARGE_N
    t0 = time.perf_counter()
    gen = torch.Generator(device=DEV).manual_seed(n)
    a, b, y = (mg.Banded((n,), torch.float32, DEV) for _ in range(3))
    a.t.copy_(torch.randn(n, device=DEV, generator=gen))
    b.t.copy_(torch.randn(n, device=DEV, generator=gen))
    a0, b0 = a.t.clone(), b.t.clone()
    rc = L().mogan_add(a.t.data_ptr(), b.t.data_ptr(), y.t.data_ptr(), n, lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    want = a0 + b0
    assert torch.equal(y.t, want), "%d elements differ (the last %d are the second trip's)" % (int((y.t != want).sum()), n - K.GRID_CAP * K.BLOCK)
    assert torch.equal(y.t.view(torch.int32), want.view(torch.int32))
    assert a.intact() and b.intact() and y.intact(), "a guard band was written"
    assert torch.equal(a.t, a0) and torch.equal(b.t, b0), "an input was modified"
    RAN.add(("mogan_add", n))
    print("mogan_add n = %d: %.2f s" % (n, time.perf_counter() - t0))


# -------------------------------------------------------------------------------------------------------------------- feeder
def _crop(row):
    """the crop call of a row into fresh buffers: (inputs, outputs, call)"""
    (B, ori, size), _ = row
    d = K.crop_case(row)
    src, params = _inp(d["src"]), _inp(d["params"])
    q, out = _out((B, size, size, 3), torch.uint8), _out((B, 3, size, size))
    st = lib.stream_ptr()
    call = lambda **c: (lambda a: L().mogan_feed_crop_flip(a["src"], a["params"], a["q"], a["out"], a["B"], a["ori"], a["size"], st))(
        dict(dict(src=src.ptr, params=params.ptr, q=q.ptr, out=out.ptr, B=B, ori=ori, size=size), **c))
    return d, (src, params), (q, out), call


@pytest.mark.parametrize("row", K.CROP_ROWS, ids=lambda r: ids(r[0]))
def test_feed_crop_flip(row):
    d, (src, params), (q, out), call = _crop(row)
    what = "feed_crop_flip %s" % (row[0],)
    _twice(lambda: call(), {"q": q, "out": out}, what)
    _exact(q, d["q"], what + " q", written=False)
    _exact(out, d["out"], what + " out")
    RAN.add(("mogan_feed_crop_flip", row[0]))
    _declined([("B = 0", lambda: call(B=0)), ("ori < size", lambda: call(ori=row[0][2] - 1)), ("NULL src", lambda: call(src=None)),
               ("NULL params", lambda: call(params=None)), ("NULL q", lambda: call(q=None)), ("NULL out", lambda: call(out=None))], (q, out), what)
    _frozen((src, params), what)


def _resample(img_ptr, B, S, OS, bounds, kk):
    tmp, out = _out((B, S, OS, 3), torch.uint8), _out((B, 3, OS, OS))
    st = lib.stream_ptr()
    call = lambda **c: (lambda a: L().mogan_feed_resample(a["img"], a["tmp"], a["out"], a["bounds"], a["kk"], a["ksize"], a["B"], a["S"], a["OS"], st))(
        dict(dict(img=img_ptr, tmp=tmp.ptr, out=out.ptr, bounds=bounds.ptr, kk=kk.ptr, ksize=kk.view.shape[1], B=B, S=S, OS=OS), **c))
    return tmp, out, call


@pytest.mark.parametrize("row", K.RESAMPLE_ROWS, ids=ids)
def test_feed_resample(row):
    B, S, OS = row
    d = K.resample_case(row, feeder.pil_bilinear_coeffs)
    img, bounds, kk = _inp(d["img"]), _inp(d["bounds"]), _inp(d["kk"])
    tmp, out, call = _resample(img.ptr, B, S, OS, bounds, kk)
    assert tmp.view.numel() == B * S * OS * 3 and tmp.buf.numel() == B * S * OS * 3 + 2 * mg.BAND
    what = "feed_resample %s" % (row,)
    _twice(lambda: call(), {"tmp": tmp, "out": out}, what)
    _exact(tmp, d["tmp"], what + " tmp", written=False)
    _exact(out, d["out"], what + " out")
    RAN.add(("mogan_feed_resample", row))
    _declined([("ksize = 0", lambda: call(ksize=0)), ("OS = 0", lambda: call(OS=0)), ("S < 0", lambda: call(S=-S)), ("NULL in", lambda: call(img=None)),
               ("NULL tmp", lambda: call(tmp=None)), ("NULL out", lambda: call(out=None)), ("NULL bounds", lambda: call(bounds=None)),
               ("NULL kk", lambda: call(kk=None))], (tmp, out), what)
    _frozen((img, bounds, kk), what)


def test_feed_resample_consumes_the_crop():
    """mogan_feed_resample on the q that mogan_feed_crop_flip just wrote (17 -> 9: its vertical pass is more than one block)"""
    row, OS = K.CHAIN
    (B, ori, size), _ = row
    d, (src, params), (q, out), call = _crop(row)
    assert call() == 0
    tb, tk = feeder.pil_bilinear_coeffs(size, OS)
    e = K.resample_expect(d["q"], tb, tk)
    bounds, kk = _inp(torch.from_numpy(tb.copy())), _inp(torch.from_numpy(tk.copy()))
    tmp, out2, rs = _resample(q.ptr, B, size, OS, bounds, kk)
    what = "feed_resample of the crop %s -> %d" % (row[0], OS)
    _twice(lambda: rs(), {"tmp": tmp, "out": out2}, what)
    _exact(tmp, e["tmp"], what + " tmp", written=False)
    _exact(out2, e["out"], what + " out")
    _exact(q, d["q"], what + ": q afterwards", written=False)
    _exact(out, d["out"], what + ": the crop's out afterwards")
    _frozen((src, params, bounds, kk), what)
    RAN.add(("chain",))


# -------------------------------------------------------------------------------------------------------------------- census
def test_census_of_entry_points_and_rows():
    """every entry point ran every row of its table; prints the largest err / bound per kind (the bounds carry 4 x the CPU figures)"""
    for k in sorted(FIG):
        print("%-12s largest err / bound = %.3f" % (k, FIG[k]))
    want = {(e, r) for e in ("mogan_avgpool_fwd", "mogan_avgpool_bwd") for r in K.AVG_ROWS}
    want |= {(e, r) for e in ("mogan_maxpool_fwd", "mogan_maxpool_fwd idx=NULL") for r in K.MAX_ROWS + [K.MAX_FWD_ONLY]}
    want |= {("mogan_maxpool_bwd", r) for r in K.MAX_ROWS}
    want |= {(e, r) for e in ("mogan_bilinear_fwd", "mogan_bilinear_bwd") for r in K.BIL_ROWS}
    want |= {("mogan_add", n) for n in K.SUM_N + (K.ADD_LARGE_N,)} | {("mogan_scale", n, a) for n in K.SUM_N for a in K.ALPHAS}
    want |= {(e, n, G) for e in ("mogan_group_sum", "mogan_group_bcast") for n in K.SUM_N for G in K.SUM_G}
    want |= {("mogan_feed_crop_flip", r[0]) for r in K.CROP_ROWS} | {("mogan_feed_resample", r) for r in K.RESAMPLE_ROWS} | {("chain",)}
    if not RAN:
        pytest.skip("the census needs the tests of this module to have run (a selection was made)")
    assert not want - RAN, "never ran: %s" % sorted(want - RAN, key=str)
    assert set(FIG) == {"avgpool y", "avgpool dx", "maxpool dx", "bilinear y", "bilinear dx"}
    assert all(v <= 1.0 for v in FIG.values()), FIG
