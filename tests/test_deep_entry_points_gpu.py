"""-m gpu: the deep-block entry points of include/mogan_hip.h -- mogan_deep_conv_bn_act_fwd / _bwd, csrc/mogan_pgemm.hip -- through
ctypes, per element against staged fp64 references and under the memory contract of tests/memguard.py: what
tests/test_bn_entry_points_gpu.py does for the batch-norm family.  Rows (one per register class x group count x shape of the
tail's slab loop), inputs, references and bounds are tests/deep_cases.py; tests/test_deep_reference_cpu.py checks them without a
GPU and tests/test_deep_rejections_cpu.py holds every rejection with dummy pointers.

Memory, every call:
  * every output -- y, stats, z, the pixel panel of z, both running buffers, dy, dgamma, dbeta, dx -- is the payload of a guard-banded
    buffer: NaN poison in write mode, a finite base in accumulate mode (the running statistics; dgamma / dbeta with accumulate = 1);
    afterwards every element is written, nothing outside changed;
  * every input -- the packed weights too -- is bitwise unchanged afterwards;
  * the workspace is a guard-banded byte buffer of exactly the panel (rounded up to 256 bytes) plus the predicted slabs, refilled
    with 0xFF before each call; its bands stay intact, and the whole slabs behind the panel that no longer hold poison are counted:
    the K-split the row was written for is the one that ran;
  * the same call a second time gives the same bits; a NULL in a nullable place leaves every other output's bits as they were;
  * a declined call leaves every output and the workspace untouched.

Values: y against the fp64 convolution; stats, z and the running statistics against bn_cases' formulas ON THE y THE KERNEL WROTE;
dy, dgamma, dbeta against the backward formulas on that y; dx against the fp64 transposed convolution of the dy the kernel wrote;
the panels decode exactly to z and dy (the sum of the three pieces keeps every bit but a zero's sign); and beside that the
whole-tensor figures of test_deep_block_conv_bn_act against one fp64 chain from x, its gradients on the kernel's side of the kink
where an element of the band fell on the other one.  The last test asserts the census and prints the largest err / bound per output."""
import functools

import pytest
import torch

import bn_cases as BN
import conv_cases as CV
import deep_cases as K
import memguard as mg
from helpers import load_pkg, max_abs, rel_l2

load_pkg()
from mogan_amd.hip import lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ERR_SHAPE, ERR_WS = -1, -3
SLOPE, EPS, MOM = 0.2, 1e-5, 0.1          # (ctypes rounds them to the fp32 values bn_cases computes with)
GLU = 3

RAN = set()
FIG = {}

CASES = [(r, -1) for r in K.ROWS] + [(K.TILE_ROW, c) for c in (0, 1, 2)]


def _case_id(case):
    return K.row_id(case[0]) + ("" if case[1] < 0 else "-tile%d" % case[1])


def L():
    return lib.load()


def _inp(t):
    g = mg.Guarded(tuple(t.shape), (Ellipsis,), DEV, dtype=t.dtype, base=t)
    g.frozen = mg.Frozen(g.buf)
    return g


def _out(shape, base=None, dtype=torch.float32):
    return mg.Guarded(tuple(shape), (Ellipsis,), DEV, dtype=dtype, base=base)


def _p(g):
    return None if g is None else g.ptr


def _same_bits(a, b, what):
    assert torch.equal(mg._bits(a.contiguous()), mg._bits(b.contiguous())), "%s: other bits" % what


class _WS:
    """a guard-banded workspace of exactly `n` bytes, poisoned before each call"""

    def __init__(self, n):
        self.n = n
        self.b = mg.Banded((max(n, 1),), torch.uint8, DEV)

    def args(self, kind="full"):
        mg.poison_(self.b.t)
        return {"full": (self.b.t.data_ptr(), self.n), "short": (self.b.t.data_ptr(), self.n - 1), "null": (None, self.n)}[kind]

    def intact(self):
        return self.b.intact()

    def poisoned(self):
        return bool((self.b.t == mg.POISON_U8).all())

    def whole_slabs(self, head, slab_bytes):
        """how many whole slabs behind the first `head` bytes hold no poisoned fp32 any more"""
        n = 0
        for s in range((self.n - head) // slab_bytes):
            v = self.b.t[head + s * slab_bytes: head + (s + 1) * slab_bytes].view(torch.int32)
            n += int(not bool((v == -1).any()))
        return n


@functools.lru_cache(maxsize=None)
def _dev(geometry):
    """a geometry's inputs on the device (frozen) and the packed weights of both directions"""
    g, inp = K.geom(geometry), K.inputs(geometry)
    d = {k: _inp(inp[k]) for k in ("x", "w", "gamma", "beta", "dz")}
    kk = (g["Cout"], g["Cin"], g["k"], g["k"], g["s"])
    wf = torch.empty(int(L().mogan_pk_weight_bytes(*kk, 0)), dtype=torch.uint8, device=DEV)
    wd = torch.empty(int(L().mogan_pk_weight_bytes(*kk, 1)), dtype=torch.uint8, device=DEV)
    assert wf.numel() > 0 and wd.numel() > 0
    lib.call("mogan_pk_weight_pack_both", d["w"].ptr, wf.data_ptr(), wd.data_ptr(), g["Cout"], g["Cin"], g["k"], g["k"], g["s"], g["pad"], g["pad"],
             lib.stream_ptr())
    torch.cuda.synchronize()
    d["wf"], d["wd"] = _inp(wf), _inp(wd)
    return d


def _frozen(d, what, keys=("x", "w", "gamma", "beta", "dz", "wf", "wd")):
    for k in keys:
        d[k].frozen.check("%s (%s)" % (what, k))


def _verify(g, ref, bnd, kind, what):
    got = g.view.cpu().double()
    ref = ref.double().reshape(got.shape)
    bnd = (bnd if torch.is_tensor(bnd) else torch.full_like(ref, float(bnd))).double().reshape(got.shape)
    err = (got - ref).abs()
    frac = float(torch.nan_to_num(err / bnd.clamp_min(1e-300), nan=float("inf")).max())
    FIG[kind] = max(FIG.get(kind, 0.0), frac)
    g.check(ref, bnd, what="%s (largest err / bound %.3f)" % (what, frac))


def _written(o, what):
    for k, g in o.items():
        if g is not None and g.dtype == torch.float32:
            assert g.problems() == [], (what, k, g.problems())
        elif g is not None:
            assert g.problems(written=False) == [], (what, k, g.problems(written=False))


# ---------------------------------------------------------------------------------------------------------------- forward
def _fwd_outs(row, rm=True, rv=True, zpanel=True):
    g, inp = K.geom(row), K.inputs(row[:9])
    shp = (g["B"], g["Cout"], g["OH"], g["OW"])
    return dict(y=_out(shp), stats=_out((2, g["G"], g["Cout"])), z=_out(shp),
                zpanel=_out((g["B"] * g["HW"] * g["Cout"] * 6,), dtype=torch.uint8) if zpanel else None,
                rm=_out((g["Cout"],), inp["rm"]) if rm else None, rv=_out((g["Cout"],), inp["rv"]) if rv else None)


def _fwd(row, d, o, wsp, wsn, cfg=-1, x=True, xpanel=None, momentum=MOM, **kw):
    """the call with the row's forced split (and tile shape); kw: arguments that differ from the row's, for the declined calls"""
    g = dict(K.geom(row), act=row[9])
    g.update(kw)
    ptrs = dict(x=d["x"].ptr if x else None, xpanel=xpanel, wpk=d["wf"].ptr, gamma=d["gamma"].ptr, beta=d["beta"].ptr, rmean=_p(o["rm"]),
                rvar=_p(o["rv"]), y=o["y"].ptr, stats=o["stats"].ptr, z=o["z"].ptr, zpanel=_p(o["zpanel"]))
    for k in kw.get("null", ()):
        ptrs[k] = None
    L().mogan_pk_debug_force(1, cfg, row[10])
    try:
        rc = L().mogan_deep_conv_bn_act_fwd(*ptrs.values(), g["B"], g["Cin"], g["Hs"], g["Ws"], g["Cout"], g.get("KH", g["k"]), g.get("KW", g["k"]),
                                            g["s"], g["pad"], g["pad"], EPS, momentum, g["act"], SLOPE, g["G"], wsp, wsn, lib.stream_ptr())
        torch.cuda.synchronize()
    finally:
        L().mogan_pk_debug_force(0, -1, 0)
    return rc


def _fwd_room(row):
    """slabs the forward's workspace is sized for: the forced split's; for the heuristic's own split the most it may take (ntile / 4)"""
    g = K.geom(row)
    return K.slabs_of(g["ntile"], row[10]) if row[10] > 0 else max(1, g["ntile"] // 4)


def _panel_of(t):
    """(B, C, OH, OW) -> the (pixel, channel) matrix a pixel panel decodes to: all images in order"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _decodes_to(panel, t, what):
    """the panel's three bf16 pieces add up to t exactly, every pixel and channel (a zero's sign is not kept by the sum: -0 = +0;
    poison decodes to NaN, which equals nothing)"""
    want = _panel_of(t)
    assert torch.equal(K._panel_decode(panel, want.shape[0], want.shape[1]), want), what


@functools.lru_cache(maxsize=None)
def _forward(case):
    """one verified forward call of a case; what it left is the backward's input"""
    row, cfg = case
    g, inp, d = K.geom(row), K.inputs(row[:9]), _dev(row[:9])
    act, G = row[9], g["G"]
    what = "fwd " + _case_id(case)
    room = _fwd_room(row)
    head, slab = K.fwd_ws_bytes(row, 0), 4 * g["B"] * g["Cout"] * g["HW"]
    ws = _WS(K.fwd_ws_bytes(row, room))
    o = _fwd_outs(row)
    assert _fwd(row, d, o, *ws.args(), cfg=cfg) == 0, what
    assert ws.intact(), what + ": the workspace's bands"
    _frozen(d, what)
    # the K-split that ran: one slab is the GEMM's direct store into y, nothing behind the panel is written
    seen = ws.whole_slabs(head, slab)
    if row[10] > 0:
        want = K.slabs_of(g["ntile"], row[10])
        assert seen == (want if want > 1 else 0), "%s: %d whole slabs behind the panel, %d predicted" % (what, seen, want)
        RAN.add(("loop", K.ept_class(g["NE"], G), G, K.loop_shape(K.ept_class(g["NE"], G), want)))
    else:
        assert 0 <= seen <= room and seen != 1, (what, seen)
        RAN.add(("heuristic", max(seen, 1)))
    # stage 1: y against the fp64 convolution
    y_ref, S_y = K.conv_reference(row[:9])
    _verify(o["y"], y_ref, CV.TOL["fwd"] * S_y, "y", what + " y")
    # stage 2: statistics, z, running statistics from the y the kernel wrote
    yk, zk = o["y"].view.cpu(), o["z"].view.cpu()
    flat = lambda t: t.reshape(g["B"], g["Cout"], g["HW"])
    ref, S, Fx, bnd, extra = K.tail_reference(flat(yk), inp["gamma"], inp["beta"], act, inp["rm"], inp["rv"], flat(inp["dz"]), G, z_side=flat(zk))
    _verify(o["stats"], torch.stack([ref["mean"], ref["invstd"]]), torch.stack([bnd["mean"], bnd["invstd"]]), "stats", what + " stats")
    _verify(o["z"], ref["z"], bnd["z"], "z", what + " z")
    band = extra["band"]
    assert float(band.double().mean()) <= K.BAND_SHARE, what
    if act in (K.RELU, K.LRELU):
        assert bool(((flat(zk) > 0) == (extra["t"] > 0))[~band].all()), what + ": the sign of z outside the kink band"
    _verify(o["rm"], ref["rm"], bnd["rm"], "running_mean", what + " running_mean")
    _verify(o["rv"], ref["rv"], bnd["rv"], "running_var", what + " running_var")
    # the pixel panel of z: all B images in order, bit for bit
    assert o["zpanel"].problems(written=False) == [], what
    _decodes_to(o["zpanel"].view, o["z"].view, what + ": zpanel does not decode to z")
    # the whole block against one fp64 chain from x: the figures of test_deep_block_conv_bn_act
    c = K.chain(row[:9], act)
    assert max_abs(o["z"].view, c["z"]) <= 2e-5, what
    assert max_abs(o["rm"].view, c["rm"]) <= 1e-6 and max_abs(o["rv"].view, c["rv"]) <= 1e-5, what
    RAN.add(("fwd", row, cfg))
    keep = {k: v.view.clone() for k, v in o.items()}
    # the same call again: the same bits
    for v in o.values():
        v.reset()
    assert _fwd(row, d, o, *ws.args(), cfg=cfg) == 0 and ws.intact(), what
    _written(o, what)
    for k, v in o.items():
        _same_bits(keep[k], v.view, what + " second call " + k)
    return dict(keep, ref=ref, bnd=bnd, S=S, F=Fx)


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_deep_forward(case):
    _forward(case)


@pytest.mark.parametrize("row", K.VARIANT_ROWS, ids=K.row_id)
def test_deep_forward_nullable_arguments(row):
    g, inp, d = K.geom(row), K.inputs(row[:9]), _dev(row[:9])
    first = _forward((row, -1))
    what = "fwd variants " + K.row_id(row)
    ws = _WS(K.fwd_ws_bytes(row, _fwd_room(row)))

    def same(o, keys, tag):
        _written(o, what + tag)
        for k in keys:
            _same_bits(first[k], o[k].view, "%s %s: %s" % (what, tag, k))

    # the panel of x given (made by mogan_panel_tail_group), x itself NULL; the workspace then starts with the slabs
    xp = torch.empty(g["B"] * g["Hs"] * g["Ws"] * g["Cin"] * 6, dtype=torch.uint8, device=DEV)
    K._run_tail([K._tail_member(g["B"], g["Cin"], g["Hs"], g["Ws"], [(d["x"].ptr, g["Cin"] * g["Hs"] * g["Ws"], 0, 1)], panel=xp.data_ptr(), Cp=g["Cin"])])
    torch.cuda.synchronize()
    assert torch.equal(K._panel_decode(xp, g["B"] * g["Hs"] * g["Ws"], g["Cin"]), _panel_of(d["x"].view))
    xpf = mg.Frozen(xp)
    slab = 4 * g["B"] * g["Cout"] * g["HW"]
    ws2 = _WS(_fwd_room(row) * slab)
    for x in (False, True):
        o = _fwd_outs(row)
        assert _fwd(row, d, o, *ws2.args(), x=x, xpanel=xp.data_ptr()) == 0 and ws2.intact(), what
        same(o, ("y", "stats", "z", "zpanel", "rm", "rv"), " xpanel given, x %s" % ("given" if x else "NULL"))
        assert ws2.whole_slabs(0, slab) == _fwd_room(row), what
        xpf.check(what)
    o = _fwd_outs(row)
    assert _fwd(row, d, o, None, 0, x=False, xpanel=xp.data_ptr()) == 0, what + ": a panel given needs no workspace"
    y_ref, S_y = K.conv_reference(row[:9])
    _verify(o["y"], y_ref, CV.TOL["fwd"] * S_y, "y", what + " no workspace y")
    same(o, (), " no workspace")
    RAN.add(("xpanel", g["G"]))
    # no panel of z wanted
    o = _fwd_outs(row, zpanel=False)
    assert _fwd(row, d, o, *ws.args()) == 0 and ws.intact(), what
    same(o, ("y", "stats", "z", "rm", "rv"), " zpanel NULL")
    # no running statistics, also one at a time
    for rm, rv in ((False, False), (True, False), (False, True)):
        o = _fwd_outs(row, rm, rv)
        assert _fwd(row, d, o, *ws.args()) == 0 and ws.intact(), what
        same(o, [k for k in ("y", "stats", "z", "zpanel", "rm", "rv") if o[k] is not None], " running_mean %s running_var %s" % (rm, rv))
    # momentum 0: the running statistics come back as they were
    o = _fwd_outs(row)
    assert _fwd(row, d, o, *ws.args(), momentum=0.0) == 0 and ws.intact(), what
    same(o, ("y", "stats", "z", "zpanel"), " momentum 0")
    _same_bits(o["rm"].view, inp["rm"].to(DEV), what + " momentum 0 running_mean")
    _same_bits(o["rv"].view, inp["rv"].to(DEV), what + " momentum 0 running_var")
    # room for the panel and ONE slab: no K-split, the GEMM stores into y itself; y is still right
    ws1 = _WS(K.fwd_ws_bytes(row, 1))
    o = _fwd_outs(row)
    assert _fwd(row, d, o, *ws1.args()) == 0 and ws1.intact(), what
    assert ws1.whole_slabs(K.fwd_ws_bytes(row, 0), slab) == 0, what + ": one slab of room, but a slab was written"
    y_ref, S_y = K.conv_reference(row[:9])
    _verify(o["y"], y_ref, CV.TOL["fwd"] * S_y, "y", what + " direct store y")
    _written(o, what + " direct store")
    assert max_abs(o["z"].view, K.chain(row[:9], row[9])["z"]) <= 2e-5
    _frozen(d, what)
    RAN.add(("variants", g["G"]))


# --------------------------------------------------------------------------------------------------------------- backward
def _bwd_outs(row, accumulate=0, dparam=True, dx=True):
    g, inp = K.geom(row), K.inputs(row[:9])
    return dict(dy=_out((g["B"], g["Cout"], g["OH"], g["OW"])),
                dgamma=_out((g["Cout"],), inp["base_g"] if accumulate else None) if dparam else None,
                dbeta=_out((g["Cout"],), inp["base_b"] if accumulate else None) if dparam else None,
                dx=_out((g["B"], g["Cin"], g["Hs"], g["Ws"])) if dx else None)


def _bwd(row, d, fw, o, wsp, wsn, accumulate=0, cfg=-1, **kw):
    g = dict(K.geom(row), act=row[9])
    g.update(kw)
    ptrs = dict(dz=d["dz"].ptr, y=fw["y"].ptr, stats=fw["stats"].ptr, gamma=d["gamma"].ptr, beta=d["beta"].ptr, wpk_dgrad=d["wd"].ptr, dy=o["dy"].ptr,
                dgamma=_p(o["dgamma"]), dbeta=_p(o["dbeta"]), dx=_p(o["dx"]))
    for k in kw.get("null", ()):
        ptrs[k] = None
    p = list(ptrs.values())
    L().mogan_pk_debug_force(1, cfg, row[10])
    try:
        rc = L().mogan_deep_conv_bn_act_bwd(*p[:9], accumulate, p[9], g["B"], g["Cin"], g["Hs"], g["Ws"], g["Cout"], g.get("KH", g["k"]), g.get("KW", g["k"]),
                                            g["s"], g["pad"], g["pad"], g["act"], SLOPE, g["G"], wsp, wsn, lib.stream_ptr())
        torch.cuda.synchronize()
    finally:
        L().mogan_pk_debug_force(0, -1, 0)
    return rc


def _bwd_room(row):
    g = K.geom(row)
    return K.slabs_of(g["ntile_d"], row[10]) if row[10] > 0 else max(1, g["ntile_d"] // 4)


def _saved(case):
    """y and stats as the forward left them, as frozen inputs of the backward"""
    fw = _forward(case)
    return dict(y=_inp(fw["y"].cpu()), stats=_inp(fw["stats"].cpu()))


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_deep_backward(case):
    row, cfg = case
    g, inp, d = K.geom(row), K.inputs(row[:9]), _dev(row[:9])
    first_fw = _forward(case)
    fw = _saved(case)
    ref, bnd, S, Fx, G = first_fw["ref"], first_fw["bnd"], first_fw["S"], first_fw["F"], g["G"]
    what = "bwd " + _case_id(case)
    ws = _WS(K.bwd_ws_bytes(row, _bwd_room(row)))

    def frozen():
        _frozen(d, what)
        fw["y"].frozen.check(what); fw["stats"].frozen.check(what)

    o = _bwd_outs(row)
    assert _bwd(row, d, fw, o, *ws.args(), cfg=cfg) == 0, what
    assert ws.intact(), what
    frozen()
    # stage 3: dy, dgamma, dbeta from the y and z the kernel wrote (dgamma / dbeta of two groups: the groups' sums)
    _verify(o["dy"], ref["dy"], bnd["dy"], "dy", what + " dy")
    _verify(o["dgamma"], ref["dgamma"], bnd["dgamma"], "dgamma", what + " dgamma")
    _verify(o["dbeta"], ref["dbeta"], bnd["dbeta"], "dbeta", what + " dbeta")
    # the gradient's pixel panel at the head of the workspace: bit for bit dy
    _decodes_to(ws.b.t[:g["B"] * g["HW"] * g["Cout"] * 6], o["dy"].view, what + ": the panel does not decode to dy")
    # stage 4: dx against the fp64 transposed convolution of the dy the kernel wrote
    dx_ref, S_dx = K.dgrad_reference(row[:9], o["dy"].view.cpu())
    _verify(o["dx"], dx_ref, K.TOL_DX * S_dx, "dx", what + " dx")
    # the whole block against the fp64 chain from x
    c, taken = K.chain_on_the_side_of(row[:9], row[9], first_fw["z"].cpu())
    assert taken <= K.BAND_SHARE * first_fw["z"].numel(), (what, taken)
    assert rel_l2(o["dx"].view, c["dx"]) <= 5e-6, (what, rel_l2(o["dx"].view, c["dx"]))
    assert max_abs(o["dgamma"].view, c["dgamma"]) <= 2e-4 * max(1.0, float(c["dgamma"].abs().max())), what
    assert max_abs(o["dbeta"].view, c["dbeta"]) <= 2e-4 * max(1.0, float(c["dbeta"].abs().max())), what
    RAN.add(("bwd", row, cfg))
    keep = {k: v.view.clone() for k, v in o.items()}
    # the same call again
    for v in o.values():
        v.reset()
    assert _bwd(row, d, fw, o, *ws.args(), cfg=cfg) == 0 and ws.intact(), what
    _written(o, what)
    for k, v in o.items():
        _same_bits(keep[k], v.view, what + " second call " + k)
    # accumulate = 1 into non-zero parameter gradients
    oa = _bwd_outs(row, 1)
    assert _bwd(row, d, fw, oa, *ws.args(), accumulate=1, cfg=cfg) == 0 and ws.intact(), what
    _written(oa, what)
    _same_bits(keep["dy"], oa["dy"].view, what + " accumulate dy")
    _same_bits(keep["dx"], oa["dx"].view, what + " accumulate dx")
    for k, base in (("dgamma", inp["base_g"]), ("dbeta", inp["base_b"])):
        _verify(oa[k], ref[k] + base.double(), K.accumulate_bound(k, S, Fx, bnd, base, G), k, "%s accumulate %s" % (what, k))
    RAN.add(("accumulate", G))
    # no data gradient, no workspace
    o2 = _bwd_outs(row, dx=False)
    assert _bwd(row, d, fw, o2, None, 0, cfg=cfg, null=("wpk_dgrad",)) == 0, what
    _written(o2, what)
    for k in ("dy", "dgamma", "dbeta"):
        _same_bits(keep[k], o2[k].view, "%s dx NULL, ws NULL: %s" % (what, k))
    # no parameter gradients
    o3 = _bwd_outs(row, dparam=False)
    assert _bwd(row, d, fw, o3, *ws.args(), cfg=cfg) == 0 and ws.intact(), what
    _written(o3, what)
    _same_bits(keep["dy"], o3["dy"].view, what + " dgamma, dbeta NULL: dy")
    _same_bits(keep["dx"], o3["dx"].view, what + " dgamma, dbeta NULL: dx")
    frozen()
    RAN.add(("bwd variants", G))


# ---------------------------------------------------------------------------------------------------------- declined calls
SHAPE_KW = [("groups = 3", dict(G=3)), ("B % groups", dict(B=5, G=2)), ("Cin % 32", dict(Cin=48)), ("Cout % 32", dict(Cout=48)),
            ("stride = 0", dict(s=0)), ("OH <= 0", dict(Hs=1, pad=0)), ("act = GLU", dict(act=GLU)),
            ("KH * KW > 25", dict(KH=6, KW=6, pad=2)), ("B = 0", dict(B=0))]
STRIDE_ROW = K.ROWS[3]             # 4x4 stride 2: the data gradient's geometry can be declined on its own


@pytest.mark.parametrize("row", (K.ROWS[1], STRIDE_ROW, K.ROWS[4]), ids=K.row_id)
def test_declined_calls_write_nothing(row):
    g, d = K.geom(row), _dev(row[:9])
    fw = _saved((row, -1))
    what = "declined " + K.row_id(row)
    wsf, wsb = _WS(K.fwd_ws_bytes(row, _fwd_room(row))), _WS(K.bwd_ws_bytes(row, _bwd_room(row)))
    of, ob = _fwd_outs(row), _bwd_outs(row, 1)
    n = 0

    def declined(rc, want, o, ws, tag):
        nonlocal n
        assert rc == want, "%s %s: return code %d" % (what, tag, rc)
        assert all(v.untouched() for v in o.values()), "%s %s: declined, but an output was written" % (what, tag)
        assert ws.intact() and ws.poisoned(), "%s %s: declined, but the workspace was written" % (what, tag)
        n += 1

    # one image more per group than the registers hold: (B / groups) * OH * OW * groups > 2048
    too_many = g["G"] * (2048 // (g["G"] * g["HW"]) + 1)
    assert too_many // g["G"] * g["HW"] * g["G"] > 2048 >= (too_many // g["G"] - 1) * g["HW"] * g["G"]
    for tag, kw in SHAPE_KW + [("NE > 2048 / groups", dict(B=too_many))]:
        declined(_fwd(row, d, of, *wsf.args(), **kw), ERR_SHAPE, of, wsf, "fwd " + tag)
        declined(_bwd(row, d, fw, ob, *wsb.args(), accumulate=1, **kw), ERR_SHAPE, ob, wsb, "bwd " + tag)
    for k in ("gamma", "beta", "y", "stats", "z", "wpk"):
        declined(_fwd(row, d, of, *wsf.args(), null=(k,)), ERR_SHAPE, of, wsf, "fwd NULL " + k)
    declined(_fwd(row, d, of, *wsf.args(), null=("x", "xpanel")), ERR_SHAPE, of, wsf, "fwd x and xpanel NULL")
    declined(_fwd(row, d, of, *wsf.args("null")), ERR_WS, of, wsf, "fwd ws NULL")
    declined(_fwd(row, d, of, wsf.args()[0], K.fwd_ws_bytes(row, 0) - 1), ERR_WS, of, wsf, "fwd ws one byte short of the panel")
    for k in ("dz", "y", "stats", "gamma", "beta", "dy"):
        declined(_bwd(row, d, fw, ob, *wsb.args(), accumulate=1, null=(k,)), ERR_SHAPE, ob, wsb, "bwd NULL " + k)
    declined(_bwd(row, d, fw, ob, *wsb.args("null"), accumulate=1), ERR_WS, ob, wsb, "bwd ws NULL")
    declined(_bwd(row, d, fw, ob, wsb.args()[0], K.bwd_ws_bytes(row, 0) - 1, accumulate=1), ERR_WS, ob, wsb, "bwd ws one byte short of the panel")
    declined(_bwd(row, d, fw, ob, *wsb.args(), accumulate=1, null=("wpk_dgrad",)), ERR_WS, ob, wsb, "bwd wpk_dgrad NULL")
    declined(_bwd(row, d, fw, ob, *wsb.args(), accumulate=1, Cin=0), ERR_SHAPE, ob, wsb, "bwd Cin = 0 with dx")
    if g["s"] == 2:
        # the data gradient's geometry, declined BEFORE the tail kernel: dy poisoned, dgamma / dbeta still at their base
        for tag, kw in (("KH % stride", dict(KH=3)), ("KW % stride", dict(KW=3)), ("Hs % stride", dict(Hs=9)), ("Ws % stride", dict(Ws=9))):
            for acc in (1, 0):
                declined(_bwd(row, d, fw, ob, *wsb.args(), accumulate=acc, **kw), ERR_SHAPE, ob, wsb, "bwd %s accumulate %d" % (tag, acc))
        RAN.add(("declined stride rows",))
    _frozen(d, what)
    fw["y"].frozen.check(what); fw["stats"].frozen.check(what)
    RAN.add(("declined", g["G"], n))


# ------------------------------------------------------------------------------------------------------------------ census
def test_census_of_rows_and_variants():
    """every row ran both ways, under the forced tile shapes too; every cell of (class, groups, slab-loop shape); every variant per group
    count; the declined calls; prints the largest err / bound per output"""
    for k in sorted(FIG):
        print("%-14s largest err / bound = %.3f" % (k, FIG[k]))
    if not RAN:
        pytest.skip("the census needs the tests of this module to have run (a selection was made)")
    want = {(d, r, c) for d in ("fwd", "bwd") for r, c in CASES}
    want |= {("loop", 8, 1, (0, 0)), ("loop", 8, 1, (0, 2)), ("loop", 8, 1, (1, 0)), ("loop", 8, 1, (1, 1)), ("loop", 8, 2, (0, 2)),
             ("loop", 16, 1, (0, 1)), ("loop", 16, 1, (1, 0)), ("loop", 16, 1, (2, 1)), ("loop", 16, 2, (1, 0)),
             ("loop", 32, 1, (0, 0)), ("loop", 32, 1, (2, 0)), ("loop", 32, 2, (0, 0)), ("loop", 32, 2, (2, 0)),
             ("loop", 64, 1, (0, 0)), ("loop", 64, 1, (2, 0))}
    want |= {(v, G) for v in ("xpanel", "variants", "accumulate", "bwd variants") for G in (1, 2)}
    want |= {("declined stride rows",)}
    assert not want - RAN, "never ran: %s" % sorted(want - RAN, key=str)
    assert any(k[0] == "heuristic" for k in RAN) and sum(1 for k in RAN if k[0] == "declined") == 3
    assert all(v <= 1.0 for v in FIG.values()), FIG
