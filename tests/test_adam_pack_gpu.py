"""-m gpu: the one-pass update of the deep convolution weights -- Adam (+EMA), the gradient reset and both packed copies in one
launch (mogan_pk_adam_pack_both, csrc/mogan_pgemm.hip) -- against the two launches it replaces, bit for bit:

  * the entry point through ctypes on guard-banded buffers (tests/memguard.py): p, m, v, ema and both panels must be bitwise what
    mogan_adam_step followed by mogan_pk_weight_pack_both leave on a copy, g all zero (zero_g) or bitwise untouched, nothing outside
    the payloads changed, a declined call writes nothing; mogan_adam_prep + mogan_adam_apply on a range whose length is no multiple
    of four against mogan_adam_step;
  * trainer.FlatAdam with the path on and off over a bucket with one eligible weight between ineligible parameters: parameters,
    moments, step count and packed images equal after two steps, no separate pack launch on the fused side;
  * the first weight-gradient launch of a round overwriting instead of adding (hip/ops.WGRAD_OVERWRITE): the gradients of a
    two-call (real, fake) backward with a third, unmerged call equal, as numbers, those of the fill + accumulate path, step after
    step -- nothing stale survives the fill that is no longer made -- and a round without any launch reads zeros.
tests/test_adam_pack_rejections_cpu.py holds the rejections with dummy pointers."""
import copy
import itertools

import pytest
import torch

import memguard as mg
from helpers import load_pkg

load_pkg()
from mogan_amd.attngan.trainer import FlatAdam  # noqa: E402
from mogan_amd.hip import lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ERR_SHAPE = -1
LR, B1, B2, EPS, DECAY = 2e-4, 0.5, 0.999, 1e-8, 0.999
STEP = 5                                   # the 1-based step both sides take

# (Cout, Cin, KH, KW, stride, pad): a 4x4 stride-2 weight (two blocks along Cout, two along Cin, four stride-parity classes), a 3x3
# (rows of 144 floats: the quads of a row straddle taps) and a 1x1 (one quad row per (co, 16 ci))
WEIGHTS = [(64, 32, 4, 4, 2, 1), (32, 64, 3, 3, 1, 1), (64, 32, 1, 1, 1, 0)]
FLAGS = list(itertools.product((False, True), (0, 1), (False, True), (0, 1)))      # ema, eps_mode, dev_state, zero_g


def L():
    return lib.load()


def _rand(shape, seed, positive=False):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(shape, generator=g)
    return (t * t * 1e-3 if positive else t * 0.05).to(DEV)


def _inout(t):
    return mg.Guarded(tuple(t.shape), (Ellipsis,), DEV, dtype=t.dtype, base=t)


def _panel(nbytes):
    return mg.Guarded((nbytes,), (Ellipsis,), DEV, dtype=torch.uint8)


def _state(steps_done):
    s = torch.zeros(3, dtype=torch.float32, device=DEV)
    s[0] = steps_done
    return s


def _reference(w, p, g, m, v, ema, eps_mode, dev_state, gscale):
    """mogan_adam_step, then mogan_pk_weight_pack_both, on copies: (p, m, v, ema, fwd panel, dgrad panel)"""
    Cout, Cin, KH, KW, s, pad = w
    p, m, v = p.clone(), m.clone(), v.clone()
    ema = None if ema is None else ema.clone()
    ops.adam_step(p, g.clone(), m, v, ema, LR, B1, B2, EPS, step=STEP, dev_state=_state(STEP - 1) if dev_state else None,
                  eps_mode=eps_mode, grad_scale=gscale, ema_decay=DECAY)
    nb = [int(L().mogan_pk_weight_bytes(Cout, Cin, KH, KW, s, d)) for d in (0, 1)]
    pf, pd = (torch.empty(n, dtype=torch.uint8, device=DEV) for n in nb)
    lib.call("mogan_pk_weight_pack_both", p.data_ptr(), pf.data_ptr(), pd.data_ptr(), Cout, Cin, KH, KW, s, pad, pad, None)
    return p, m, v, ema, pf, pd


@pytest.fixture(scope="module")
def inputs():
    """random p, g, m, v (>= 0), ema per weight: made once, never written (every call works on guarded copies)"""
    out = {}
    for i, w in enumerate(WEIGHTS):
        shape = w[:4]
        out[w] = dict(p=_rand(shape, 10 * i + 1), g=_rand(shape, 10 * i + 2), m=_rand(shape, 10 * i + 3),
                      v=_rand(shape, 10 * i + 4, positive=True), ema=_rand(shape, 10 * i + 5))
    return out


@pytest.mark.parametrize("ema,eps_mode,dev_state,zero_g", FLAGS,
                         ids=["%s-eps%d-%s-zero_g%d" % ("ema" if f[0] else "noema", f[1], "dev" if f[2] else "host", f[3]) for f in FLAGS])
@pytest.mark.parametrize("w", WEIGHTS, ids=["%dx%dx%dx%d-s%d-p%d" % w for w in WEIGHTS])
def test_entry_point_equals_adam_then_pack(w, ema, eps_mode, dev_state, zero_g, inputs):
    Cout, Cin, KH, KW, s, pad = w
    t = inputs[w]
    gscale = 1.0 if eps_mode == 0 else 0.5
    want = _reference(w, t["p"], t["g"], t["m"], t["v"], t["ema"] if ema else None, eps_mode, dev_state, gscale)
    P, G, M, V = (_inout(t[k]) for k in "pgmv")
    E = _inout(t["ema"]) if ema else None
    PF, PD = (_panel(int(L().mogan_pk_weight_bytes(Cout, Cin, KH, KW, s, d))) for d in (0, 1))
    st = None
    if dev_state:
        st = _state(STEP - 1)
        assert L().mogan_adam_prep(st.data_ptr(), LR, B1, B2, eps_mode, None) == 0
    args = lambda Cin_=Cin: (P.ptr, G.ptr, M.ptr, V.ptr, None if E is None else E.ptr, PF.ptr, PD.ptr, Cout, Cin_, KH, KW, s, pad,
                             pad, LR, B1, B2, EPS, 0 if dev_state else STEP, None if st is None else st.data_ptr(), eps_mode,
                             gscale, DECAY, zero_g, None)
    # a declined call (Cin % 32) has written nothing
    assert L().mogan_pk_adam_pack_both(*args(Cin + 16)) == ERR_SHAPE
    torch.cuda.synchronize()
    for b in (P, G, M, V, PF, PD) + ((E,) if ema else ()):
        assert b.untouched(), "a declined call wrote"
    assert L().mogan_pk_adam_pack_both(*args()) == 0
    torch.cuda.synchronize()
    what = "%r ema=%s eps_mode=%d dev_state=%s zero_g=%d" % (w, ema, eps_mode, dev_state, zero_g)
    P.check(want[0], exact=True, what=what + " p")
    M.check(want[1], exact=True, what=what + " m")
    V.check(want[2], exact=True, what=what + " v")
    if ema:
        E.check(want[3], exact=True, what=what + " ema")
    PF.check(want[4], exact=True, what=what + " forward panel", written=False)
    PD.check(want[5], exact=True, what=what + " data-gradient panel", written=False)
    G.check(torch.zeros_like(t["g"]) if zero_g else t["g"], exact=True, what=what + " g")
    assert torch.equal(P.view, want[0]) and torch.equal(M.view, want[1]) and torch.equal(V.view, want[2])
    assert torch.equal(PF.view, want[4]) and torch.equal(PD.view, want[5])
    if dev_state:
        assert float(st[0]) == STEP                      # advanced once, by the prep alone


@pytest.mark.parametrize("n", [1, 3, 1021, 4099])
def test_prep_and_apply_equal_adam_step_on_a_ragged_range(n):
    """the two-part bucket step on a range that ends inside a quad: the tail path, nothing behind element n - 1 touched"""
    t = dict(p=_rand((n,), 71), g=_rand((n,), 72), m=_rand((n,), 73), v=_rand((n,), 74, positive=True), ema=_rand((n,), 75))
    for eps_mode, ema in itertools.product((0, 1), (False, True)):
        p, m, v = t["p"].clone(), t["m"].clone(), t["v"].clone()
        e = t["ema"].clone() if ema else None
        ops.adam_step(p, t["g"], m, v, e, LR, B1, B2, EPS, dev_state=_state(STEP - 1), eps_mode=eps_mode, grad_scale=0.5)
        P, G, M, V = (_inout(t[k]) for k in "pgmv")
        E = _inout(t["ema"]) if ema else None
        st = _state(STEP - 1)
        ops.adam_prep(st, LR, B1, B2, eps_mode)
        ops.adam_apply(P.view, G.view, M.view, V.view, None if E is None else E.view, B1, B2, EPS, st, eps_mode=eps_mode,
                       grad_scale=0.5)
        torch.cuda.synchronize()
        P.check(p, exact=True, what="p")
        M.check(m, exact=True, what="m")
        V.check(v, exact=True, what="v")
        G.check(t["g"], exact=True, what="g")
        if ema:
            E.check(e, exact=True, what="ema")


# ------------------------------------------------------------------------------------------------------- the bucket
class _Net(torch.nn.Module):
    """one eligible convolution weight between parameters the one-pass update does not take: a convolution with three input
    channels, a bias, a BatchNorm.  (The bucket pads every parameter to 64 elements, so its ranges are whole quads whatever the
    parameters' sizes: the ragged tail is test_prep_and_apply_equal_adam_step_on_a_ragged_range's.)"""

    def __init__(self):
        super().__init__()
        self.stem = torch.nn.Conv2d(3, 7, 3, 1, 1, bias=True)           # 189 weights + 7 biases
        self.deep = torch.nn.Conv2d(32, 64, 4, 2, 1, bias=False)
        self.bn = torch.nn.BatchNorm2d(7)


@pytest.fixture()
def take_all():
    """the panel formats' hard constraints alone decide (the size heuristic would leave these small layers to other kernels)"""
    L().mogan_pk_debug_force(1, -1, 0)
    try:
        yield
    finally:
        L().mogan_pk_debug_force(0, -1, 0)


def _bucket(net, fuse, with_ema):
    opt = FlatAdam(net, LR, with_ema=with_ema)
    opt.fuse_packs = fuse
    pk = net.deep.weight._mogan_pk
    for d in (0, 1):                                   # both panels in use, as after a forward and a data gradient
        assert pk.pointer(d, 2, 8, 8, 2, 1, 1) is not None
    return opt, pk


@pytest.mark.parametrize("overwrite", [True, False], ids=["overwrite", "zero_g"])
@pytest.mark.parametrize("with_ema", [False, True], ids=["noema", "ema"])
def test_bucket_steps_equal_with_the_path_on_and_off(with_ema, overwrite, take_all, monkeypatch):
    monkeypatch.setattr(ops, "WGRAD_OVERWRITE", overwrite)
    torch.manual_seed(5)
    net0 = _Net().to(DEV)
    nets = [net0, copy.deepcopy(net0)]
    (ref, pkr), (fus, pkf) = _bucket(nets[0], False, with_ema), _bucket(nets[1], True, with_ema)
    assert ref.numel == fus.numel and ref.numel % 64 == 0
    o, n = fus._pk_range[id(pkf)]
    for step in range(2):
        g = _rand((ref.numel,), 100 + step)
        for opt in (ref, fus):
            opt.zero_grad()
            opt.g.copy_(g)
        ops._first_of_round(fus.g[o:o + n])            # (what the round's first weight-gradient launch into the range does)
        ref.step()
        packs = ops.PK_STATS["packs"]
        fused_before = ops.PK_STATS.get("adam_packs", 0)
        fus.step()
        torch.cuda.synchronize()
        assert ops.PK_STATS["packs"] == packs, "the fused side launched a pack of its own"
        assert ops.PK_STATS.get("adam_packs", 0) == fused_before + 1
        for name in ("p", "m", "v", "state") + (("ema",) if with_ema else ()):
            assert torch.equal(getattr(ref, name), getattr(fus, name)), "step %d: %s differs" % (step, name)
        for d in (0, 1):
            assert torch.equal(pkr.slots[d].buf, pkf.slots[d].buf), "step %d: panel %d differs" % (step, d)
            assert pkf.slots[d].ready(pkf.cell)
        # the gradient: cleared by the kernel, or left for the first launch of the next round to overwrite
        assert torch.equal(fus.g[o:o + n], torch.zeros_like(g[o:o + n]) if not overwrite else g[o:o + n])
        assert torch.equal(fus.g[:o], g[:o]) and torch.equal(fus.g[o + n:], g[o + n:])
        fus.zero_grad()
        assert not bool(fus.g[:o].any()) and not bool(fus.g[o + n:].any())
        assert torch.equal(fus.g[o:o + n], torch.zeros_like(g[o:o + n]) if not overwrite else g[o:o + n])
    assert float(fus.state[0]) == 2.0
    fus.close()
    assert fus.g.data_ptr() + 4 * o not in ops._OVERWRITE


# ---------------------------------------------------------------------------------- the first launch of a round overwrites
class _ToyD(torch.nn.Module):
    """one deep-shaped weight (1024 x 128 x 4 x 4 = 2^21 elements: the smallest the merged weight gradient takes) and a small
    parameter beside it"""

    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(128, 1024, 4, 2, 1, bias=False)
        self.gain = torch.nn.Parameter(torch.ones(5))

    def forward(self, x):
        return ops.conv2d(x, self.conv.weight, None, 2, 1) * self.gain.sum()


def _rounds(net, fuse, xs):
    """zero_grad, one backward of three calls (real and fake merge into one launch, the third is a leftover at the join), Adam --
    per round; the last round has no backward at all.  Returns the gradients the optimizer read."""
    opt = FlatAdam(net, LR)
    opt.fuse_packs = fuse
    w = net.conv.weight
    grads = []
    for x3 in xs:
        opt.zero_grad()
        if x3 is not None:
            ins = [x.clone().requires_grad_(True) for x in x3]
            loss = sum((net(x) * (k + 1)).sum() for k, x in enumerate(ins))
            with ops.wgrad_overlap():
                loss.backward()
        torch.cuda.synchronize()
        if fuse and x3 is None:
            assert opt._fused                                  # (zero_grad left the range alone; step must not read it)
        grads.append(None if x3 is None else w.grad.clone())
        opt.step()
    torch.cuda.synchronize()
    return grads, opt


@pytest.mark.parametrize("overwrite", [True, False], ids=["overwrite", "zero_g"])
def test_first_launch_of_a_round_overwrites(overwrite, take_all, monkeypatch):
    monkeypatch.setattr(ops, "WGRAD_OVERWRITE", overwrite)
    assert ops.MERGE_WGRAD and ops.DIRECT_GRAD and not ops.GRAD_HOOKS
    torch.manual_seed(11)
    net0 = _ToyD().to(DEV)
    assert net0.conv.weight.numel() == ops._MERGE_W
    with torch.no_grad():
        net0.conv.weight.mul_(4.0)
    nets = [net0, copy.deepcopy(net0)]
    xs = [tuple(_rand((2, 128, 8, 8), 200 + 10 * r + k) * 20 for k in range(3)) for r in range(3)] + [None]
    wg = ops.PK_STATS.get("wgrad", 0)
    want, ref = _rounds(nets[0], False, xs)
    launches = ops.PK_STATS.get("wgrad", 0) - wg
    got, fus = _rounds(nets[1], True, xs)
    assert ops.PK_STATS.get("wgrad", 0) - wg == 2 * launches           # the same launches: merged pair + leftover per round
    assert fus._fused and (bool(fus._ow_ptrs) == overwrite)
    for r, (a, b) in enumerate(zip(want, got)):
        if a is not None:
            assert bool((a != 0).any())
            assert torch.equal(a, b), "round %d: the gradient differs from the fill + accumulate path" % r
    for name in ("p", "m", "v", "state"):
        assert torch.equal(getattr(ref, name), getattr(fus, name)), name
    for opt in (ref, fus):
        opt.close()
