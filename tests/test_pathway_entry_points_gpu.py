"""-m gpu: the object-pathway and attention entry points of include/mogan_hip.h -- the spatial transformer and its shared /
constant-source forms, bbox_to_theta, the word attention, the strided masked softmax and the broadcasting channel concat --
through ctypes, per element against fp64 and under the memory contract of tests/memguard.py: what
tests/test_bn_entry_points_gpu.py does for the batch-norm family.  Tables, inputs, references and bounds are
tests/pathway_cases.py; tests/test_pathway_reference_cpu.py derives the tolerances without a GPU and
tests/test_pathway_rejections_cpu.py holds every rejection that is answered before a launch.

Memory, every call:
  * every output is the payload of a guard-banded buffer, NaN-poisoned; afterwards every element is written and nothing outside
    has changed;
  * every input -- x, theta, dy, h, src, mask, attn, dwc, dattn, lens, y, ddst, the concat sources -- lives in NaN bands and is
    bitwise unchanged afterwards, bands included;
  * the same call a second time, after poisoning again, gives the same bits (the header's "Determinism" paragraph promises this for
    the transformer's backward).

Values: every element within TOL[kind] * S of pathway_cases, and beside that the whole-tensor rel-L2 figures of
tests/test_kernels_gpu.py (pathway_cases.REL; except on the one call where no fp32 evaluation reaches it, the transformer's 257-pixel
source axis without align_corners: pathway_cases.stn_rel_applies).  bbox_to_theta and the concat's forward are compared bit for bit.
Bit-for-bit identities between entry points that follow from the code are asserted where both sides run.
The last test asserts the census of what ran and prints the largest err / bound per output kind."""
import ctypes

import numpy as np
import pytest
import torch

import memguard as mg
import pathway_cases as K
from helpers import load_pkg

load_pkg()
from mogan_amd.hip import lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS = lambda v: str(v).replace(" ", "")

RAN = set()
FIG = {}               # output kind -> largest err / bound


def L():
    return lib.load()


def _inp(t):
    """an input inside NaN guard bands, frozen (bands included); int32 travels as its fp32 bit pattern"""
    if t.dtype == torch.int32:
        t = t.view(torch.float32)
    g = mg.Guarded(tuple(t.shape), (Ellipsis,), DEV, dtype=t.dtype, base=t)
    g.frozen = mg.Frozen(g.buf)
    return g


def _out(shape):
    return mg.Guarded(tuple(shape), (Ellipsis,), DEV)


def _p(g):
    return None if g is None else g.ptr


def _sync(rc, what):
    torch.cuda.synchronize()
    assert rc == 0, "%s: return code %d" % (what, rc)


def _verify(g, ref, S, kind, what, rel=True):
    """every element within TOL[kind] * S, the memory contract of the buffer, and the whole-tensor rel-L2 figure (rel=False: the
    one transformer call of which no fp32 evaluation meets it, pathway_cases.stn_rel_applies)"""
    got = g.view.cpu().double()
    ref = ref.double().reshape(got.shape)
    bnd = (K.TOL[kind] * S).double().reshape(got.shape)
    err = (got - ref).abs()
    frac = float(torch.nan_to_num(err / bnd.clamp_min(1e-300), nan=float("inf")).max())
    FIG[kind] = max(FIG.get(kind, 0.0), frac)
    print("%s: largest err / bound %.3f" % (what, frac))
    g.check(ref, bnd, what="%s (largest err / bound %.3f)" % (what, frac))
    r = float((got - ref).norm() / (ref.norm() + 1e-30))
    assert r <= K.REL[kind] or not rel, "%s: rel-L2 %.3e > %.1e" % (what, r, K.REL[kind])


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b, what):
    assert torch.equal(_bits(a), _bits(b)), "%s: other bits" % what


def _twice(call, outs, what):
    """run `call` (-> return code), keep the bits, poison again, run again: the same bits, everything written"""
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


# ------------------------------------------------------------------------------------------------------------ transformer
def _stn_call(fn, a, b, c, dims, ac, ex=None):
    args = (a.ptr, b.ptr, c.ptr) + tuple(dims) + (ac,)
    if ex is not None:
        return getattr(L(), "mogan_stn_%s_ex" % fn)(*args, *ex, lib.stream_ptr())
    return getattr(L(), "mogan_stn_" + fn)(*args, lib.stream_ptr())


@pytest.mark.parametrize("row", K.STN_ROWS, ids=IDS)
def test_stn_fwd_bwd(row):
    B, C, Hin, Win, Hout, Wout, ac = row
    d = K.stn_case(*row)
    what = "stn %s" % (row,)
    x, th, dy = _inp(d["x"]), _inp(d["theta"]), _inp(d["dy"])
    y, dx = _out((B, C, Hout * Wout)), _out((B, C, Hin, Win))
    yb, = _twice(lambda: _stn_call("fwd", x, th, y, row[:6], ac), [y], what + " fwd")
    rel = K.stn_rel_applies(Hin, Win, ac)
    _verify(y, d["ref"]["y"], d["S"]["y"], "stn_y", what + " y", rel)
    dxb, = _twice(lambda: _stn_call("bwd", dy, th, dx, row[:6], ac), [dx], what + " bwd")
    _verify(dx, d["ref"]["dx"], d["S"]["dx"], "stn_dx", what + " dx", rel)
    # the _ex entries with a source per sample, no plane and theta[b] are the plain ones
    y.reset(); dx.reset()
    _sync(_stn_call("fwd", x, th, y, row[:6], ac, (B, 0, 0)), what + " fwd_ex")
    _sync(_stn_call("bwd", dy, th, dx, row[:6], ac, (B, 0, 0)), what + " bwd_ex")
    assert y.problems() == [] and dx.problems() == [], what
    _same_bits(yb, y.view, what + " fwd_ex(xB = B, 0, 0) against fwd")
    _same_bits(dxb, dx.view, what + " bwd_ex(xB = B, 0, 0) against bwd")
    _frozen((x, th, dy), what)
    split = K.stn_fwd_split(B, C, Hout, Wout)
    RAN.add(("stn", ac, "csplit == C" if split[0] == C else "csplit == 1" if split[0] == 1 else "ragged" if split[2] != split[1] else "even"))
    RAN.update(("stn theta", ac, K.theta_kind(K.THETA_NAMES[b % K.NT])) for b in range(B))
    RAN.update(("stn axis", ac, n) for n, v in (("Hin 1", Hin), ("Win 1", Win), ("Hout 1", Hout), ("Wout 1", Wout)) if v == 1)
    RAN.add(("stn gather groups", "one" if C == 8 else "ragged" if C % 8 else "full"))


@pytest.mark.parametrize("row", K.STN_EX_ROWS, ids=IDS)
def test_stn_shared_and_constant_sources(row):
    B, C, Hin, Win, Hout, Wout, ac, xB, plane, tG = row
    d = K.stn_case(*row)
    what = "stn_ex %s" % (row,)
    dims = row[:6]
    x, th, dy = _inp(d["x"]), _inp(d["theta"]), _inp(d["dy"])
    y, dx = _out((B, C, Hout * Wout)), _out(tuple(d["x"].shape))
    yb, = _twice(lambda: _stn_call("fwd", x, th, y, dims, ac, (xB, plane, tG)), [y], what + " fwd")
    _verify(y, d["ref"]["y"], d["S"]["y"], "stn_y", what + " y")
    _twice(lambda: _stn_call("bwd", dy, th, dx, dims, ac, (xB, plane, tG)), [dx], what + " bwd")
    _verify(dx, d["ref"]["dx"], d["S"]["dx"], "stn_dx", what + " dx")
    # the same values through the plainer forms, bit for bit
    xm = d["x"][:, :, None, None].expand(xB, C, Hin, Win).contiguous() if plane else d["x"]
    if plane:         # the constant source against its materialised plane (the same four products in the same order)
        xg, y2 = _inp(xm), _out((B, C, Hout * Wout))
        _sync(_stn_call("fwd", xg, th, y2, dims, ac, (xB, 0, tG)), what + " materialised")
        assert y2.problems() == []
        _same_bits(yb, y2.view, what + " x_plane against the materialised plane")
        _frozen((xg,), what)
    # the shared source against the plain forward on x.repeat, theta_G against theta permuted to object-major
    xg, tg, y3 = _inp(xm.repeat(B // xB, 1, 1, 1)), _inp(d["theta"][torch.from_numpy(K.theta_index(B, tG))]), _out((B, C, Hout * Wout))
    _sync(_stn_call("fwd", xg, tg, y3, dims, ac), what + " plain")
    assert y3.problems() == []
    _same_bits(yb, y3.view, what + " against the plain forward on the repeated source and the permuted theta")
    _frozen((x, th, dy, xg, tg), what)
    RAN.add(("stn_ex", ac, "shared" if xB < B else "own", "plane" if plane else "image", "theta_G" if tG else "theta[b]",
             "<256" if Hout * Wout < 256 else ">256" if Hout * Wout > 256 else "=256"))


def test_bbox_to_theta_bit_for_bit():
    """against the numpy fp32 restatement in the operation order of miscc/utils.py:16-49: the same bits wherever the value is a
    number (infinities included), a NaN exactly where the restatement has one (a NaN's sign and payload are the machine's)"""
    bb = K.bbox_table()
    N = bb.shape[0]
    want = K.bbox_to_theta_fp32(bb)
    b = _inp(torch.from_numpy(bb))
    th, thi = _out((N, 6)), _out((N, 6))
    _twice(lambda: L().mogan_bbox_to_theta(b.ptr, th.ptr, thi.ptr, N, lib.stream_ptr()), [th, thi], "bbox_to_theta")
    b.frozen.check("bbox_to_theta")
    for g, w, name in ((th, want[0], "theta"), (thi, want[1], "theta_inv")):
        assert g.problems(written=False) == [], g.problems(written=False)
        got = g.view.cpu().numpy()
        nan = np.isnan(w)
        assert (np.isnan(got) == nan).all(), "%s: NaN in other places" % name
        assert (got.view(np.int32)[~nan] == w.view(np.int32)[~nan]).all(), "%s: %d values with other bits" % (
            name, int((got.view(np.int32)[~nan] != w.view(np.int32)[~nan]).sum()))
    RAN.add(("bbox",))


# -------------------------------------------------------------------------------------------------------------- attention
@pytest.mark.parametrize("mk", K.MASKS, ids=lambda v: "mask%s" % v)
@pytest.mark.parametrize("B,idf,Q,T_", K.ATTN_ROWS, ids=IDS)
def test_attention_fwd_bwd(B, idf, Q, T_, mk):
    what = "attn %s mask %s" % ((B, idf, Q, T_), mk)
    d = K.attn_case(B, idf, Q, T_, mk, False)
    h, src, attn_in, dwc = (_inp(d[k]) for k in ("h", "src", "attn_in", "dwc"))
    mask = None if d["mask"] is None else _inp(d["mask"])
    wc, attn = _out((B, idf, Q)), _out((B, T_, Q))
    _twice(lambda: L().mogan_attn_fwd(h.ptr, src.ptr, _p(mask), wc.ptr, attn.ptr, B, idf, Q, T_, d["mode"], lib.stream_ptr()),
           [wc, attn], what + " fwd")
    _verify(attn, d["ref"]["attn"], d["S"]["attn"], "attn", what + " attn")
    _verify(wc, d["ref"]["wc"], d["S"]["wc"], "wc", what + " wc")
    if d["mask"] is not None:           # a masked word: an exact zero
        off = d["mask"].bool()[K.attn_mask_rows(B, Q, d["mode"])].permute(0, 2, 1)
        assert float(attn.view.cpu()[off].abs().max()) == 0, what
    dh, ds = _out((B, idf, Q)), _out((B, T_, Q))
    bwd = lambda g: L().mogan_attn_bwd(src.ptr, attn_in.ptr, dwc.ptr, _p(g), dh.ptr, ds.ptr, B, idf, Q, T_, lib.stream_ptr())
    first = _twice(lambda: bwd(None), [dh, ds], what + " bwd, dattn NULL")
    _verify(ds, d["ref"]["dscore"], d["S"]["dscore"], "dscore", what + " dscore, dattn NULL")
    _verify(dh, d["ref"]["dh"], d["S"]["dh"], "dh", what + " dh, dattn NULL")
    # dattn = NULL is a zero dattn
    zero = _inp(torch.zeros(B, T_, Q))
    dh.reset(); ds.reset()
    _sync(bwd(zero), what + " bwd, zero dattn")
    _same_bits(first[0], dh.view, what + " dh: NULL against zero dattn")
    _same_bits(first[1], ds.view, what + " dscore: NULL against zero dattn")
    d2 = K.attn_case(B, idf, Q, T_, mk, True)
    dattn = _inp(d2["dattn"])
    dh.reset(); ds.reset()
    _twice(lambda: bwd(dattn), [dh, ds], what + " bwd")
    _verify(ds, d2["ref"]["dscore"], d2["S"]["dscore"], "dscore", what + " dscore")
    _verify(dh, d2["ref"]["dh"], d2["S"]["dh"], "dh", what + " dh")
    _frozen((h, src, attn_in, dwc, mask, zero, dattn), what)
    RAN.add(("attn", K.attn_slots(T_), "full" if T_ == K.attn_slots(T_) else "part", mk))
    RAN.add(("attn loops", "both" if idf >= 8 and idf % 8 else "tail" if idf < 8 else "eights"))


# ---------------------------------------------------------------------------------------------------------------- softmax
@pytest.mark.parametrize("scale", K.SCALES)
@pytest.mark.parametrize("with_lens", K.LENS, ids=lambda v: "lens" if v else "nolens")
@pytest.mark.parametrize("outer,L_,inner", K.SOFTMAX_ROWS, ids=IDS)
def test_softmax_fwd_bwd(outer, L_, inner, with_lens, scale):
    what = "softmax %s lens %s scale %s" % ((outer, L_, inner), with_lens, scale)
    d = K.softmax_case(outer, L_, inner, with_lens, scale)
    x, dy, y_in = _inp(d["x"]), _inp(d["dy"]), _inp(d["y_in"])
    lens = None if d["lens"] is None else _inp(d["lens"])
    y, dx = _out((outer, L_, inner)), _out((outer, L_, inner))
    _twice(lambda: L().mogan_softmax_fwd(x.ptr, y.ptr, _p(lens), outer, L_, inner, scale, lib.stream_ptr()), [y], what + " fwd")
    _verify(y, d["ref"]["y"], d["S"]["y"], "sm_y", what + " y")
    _twice(lambda: L().mogan_softmax_bwd(y_in.ptr, dy.ptr, dx.ptr, _p(lens), outer, L_, inner, scale, lib.stream_ptr()), [dx],
           what + " bwd")
    _verify(dx, d["ref"]["dx"], d["S"]["dx"], "sm_dx", what + " dx")
    _frozen((x, dy, y_in, lens), what)
    RAN.add(("softmax", (outer, L_, inner), with_lens))
    if with_lens:
        RAN.update(("lens", k) for k, v in K.lens_clamps(d["lens"], L_).items() if v)


# ----------------------------------------------------------------------------------------------------------------- concat
def _cat_tables(sources, HW, ptrs, sb=None):
    n = len(sources)
    lay = [K.cat_layout(k, C, HW) for k, C in sources]
    pad = lambda v, fill: list(v) + [fill] * (4 - n)
    arr = [(ctypes.c_void_p * 4)(*pad(ptrs, None)), (ctypes.c_int * 4)(*pad([C for _, C in sources], 1)),
           (ctypes.c_int * 4)(*pad([l[0] for l in lay], 1)), (ctypes.c_longlong * 4)(*pad(sb or [l[2] for l in lay], 1)),
           (ctypes.c_longlong * 4)(*pad([l[3] for l in lay], 0)), (ctypes.c_int * 4)(*pad([l[4] for l in lay], 0))]
    return arr, [ctypes.cast(a, ctypes.c_void_p) for a in arr]          # (the arrays must outlive the call)


def _cat_fwd(sources, HW, srcs, dst, sb=None):
    keep, args = _cat_tables(sources, HW, [g.ptr for g in srcs], sb)
    rc = L().mogan_concat_fwd(*args, len(sources), dst.ptr, K.CAT_N, HW, lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("name", [c[0] for c in K.CAT_CASES])
def test_concat_fwd_bwd(name):
    d = K.cat_case(name)
    HW, sources, want = d["HW"], d["sources"], d["want"]
    what = "concat %s" % name
    srcs = [_inp(s) for s in d["srcs"]]
    dst = _out(tuple(d["dst"].shape))
    if K.cat_vector(HW, sources):       # (the predicate takes aligned buffers for granted: the census must not claim more)
        assert dst.ptr % 16 == 0 and all(g.ptr % 16 == 0 for g in srcs), what
    _twice(lambda: _cat_fwd(sources, HW, srcs, dst), [dst], what + " fwd")
    dst.check(d["dst"], exact=True, what=what + " dst")
    ddst = _inp(d["ddst"])
    outs = [_out(tuple(s.shape)) if w else None for s, w in zip(d["srcs"], want)]
    keep, args = _cat_tables(sources, HW, [_p(g) for g in outs])
    live = [g for g in outs if g is not None]
    _twice(lambda: L().mogan_concat_bwd(ddst.ptr, *args, len(sources), K.CAT_N, HW, lib.stream_ptr()), live, what + " bwd")
    for i, g in enumerate(outs):
        if g is not None:
            _verify(g, d["grads"][i], d["S"][i], "cat", "%s d source %d (%s)" % (what, i, sources[i][0]))
    _frozen(srcs + [ddst], what)
    bc = [K.cat_layout(k, C, HW)[4] for (k, C), w in zip(sources, want) if w]
    RAN.add(("concat fwd", "vector" if K.cat_vector(HW, sources) else "scalar"))
    RAN.add(("concat bwd", "none" if not bc else "all broadcast" if all(bc) else "all plain" if not any(bc) else "mixed"))
    RAN.update(("concat dsrc NULL", i) for i, w in enumerate(want) if not w and any(want))


def test_concat_reads_a_channel_slice_of_a_wider_parent():
    """a non-broadcast source that is channels 2..4 of a 7-channel tensor (sb = 7 HW > C HW): forward only, the parent's other
    channels hold sentinels -- a read outside the slice shows as a NaN in dst"""
    HW, N = 16, K.CAT_N
    sources = (("plane", 2), ("full", 3))
    a, b = K.T("catsl.a", (N, 2)), K.T("catsl.b", (N, 3, HW))
    ga = _inp(a)
    gb = mg.Guarded((N, 7, HW), (slice(None), slice(2, 5)), DEV, base=b)
    fb = mg.Frozen(gb.buf)
    want = torch.cat((a[:, :, None].expand(N, 2, HW), b), 1)
    for hw, tag in ((HW, "vector"), (15, "scalar")):
        if hw != HW:
            gb = mg.Guarded((N, 7, hw), (slice(None), slice(2, 5)), DEV, base=b[:, :, :hw])
            fb = mg.Frozen(gb.buf)
            want = want[:, :, :hw].contiguous()
        dst = _out((N, 5, hw))
        assert K.cat_vector(hw, sources) == (tag == "vector") and (tag != "vector" or gb.ptr % 16 == 0 and dst.ptr % 16 == 0)
        _twice(lambda: _cat_fwd(sources, hw, [ga, gb], dst, sb=[2, 7 * hw]), [dst], "concat slice " + tag)
        dst.check(want, exact=True, what="concat slice " + tag)
        fb.check("concat slice"); ga.frozen.check("concat slice")
    RAN.add(("concat slice",))


def test_concat_scalar_and_vector_kernels_give_the_same_bits():
    """HW % 4 == 0 with a non-broadcast source whose pointer is one float off 16-byte alignment: the one-value-per-thread kernel
    takes the call and writes what the four-values-per-thread kernel writes for the aligned copy"""
    d = K.cat_case("base hw16")
    HW, sources = d["HW"], d["sources"]
    srcs = [_inp(s) for s in d["srcs"]]
    dst = _out(tuple(d["dst"].shape))
    assert _cat_fwd(sources, HW, srcs, dst) == 0
    vec = dst.view.clone()
    n = d["srcs"][0].numel()
    off = mg.Guarded((n + 1,), (slice(1, None),), DEV, base=d["srcs"][0].reshape(-1))
    fo = mg.Frozen(off.buf)
    assert srcs[0].ptr % 16 == 0 and dst.ptr % 16 == 0 and off.ptr % 16 == 4
    dst.reset()
    assert _cat_fwd(sources, HW, [off] + srcs[1:], dst) == 0
    dst.check(d["dst"], exact=True, what="concat, misaligned source")
    _same_bits(vec, dst.view, "concat scalar against vector")
    fo.check("concat, misaligned source")
    _frozen(srcs, "concat, misaligned source")
    RAN.add(("concat fwd", "scalar, HW % 4 == 0"))


# ----------------------------------------------------------------------------------------------------------------- census
def test_census_of_what_ran():
    for k, v in sorted(FIG.items()):
        print("%-13s largest err / bound %.3f" % (k, v))
    want = {("stn", ac, s) for ac in (0, 1) for s in ("csplit == C", "ragged", "csplit == 1")}
    want |= {("stn theta", ac, k) for ac in (0, 1) for k in K.THETA_KINDS}
    want |= {("stn axis", ac, n) for ac in (0, 1) for n in ("Hin 1", "Win 1", "Hout 1", "Wout 1")}
    want |= {("stn gather groups", g) for g in ("one", "ragged")}
    want |= {("stn_ex", ac) + r for ac in (0, 1) for r in (("shared", "image", "theta[b]", "<256"), ("own", "image", "theta_G", "<256"),
                                                             ("shared", "image", "theta_G", "<256"), ("shared", "plane", "theta[b]", "<256"),
                                                             ("own", "plane", "theta_G", ">256"), ("shared", "plane", "theta[b]", "=256"))}
    want |= {("bbox",)}
    want |= {("attn", s, f, mk) for s in (8, 16, 32) for f in ("full", "part") for mk in K.MASKS}
    want |= {("attn loops", l) for l in ("both", "tail", "eights")}
    want |= {("softmax", r, l) for r in K.SOFTMAX_ROWS for l in K.LENS} | {("lens", k) for k in ("zero", "above", "negative")}
    want |= {("concat fwd", k) for k in ("vector", "scalar", "scalar, HW % 4 == 0")}
    want |= {("concat bwd", k) for k in ("none", "all broadcast", "all plain", "mixed")}
    want |= {("concat dsrc NULL", i) for i in range(4)} | {("concat slice",)}
    assert want <= RAN, "never ran: %s" % sorted(map(str, want - RAN))
    assert set(FIG) == set(K.TOL), "no figure for %s" % sorted(set(K.TOL) - set(FIG))
    assert all(v <= 1.0 for v in FIG.values()), FIG
