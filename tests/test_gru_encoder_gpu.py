"""-m gpu: the text encoder with cfg.RNN_TYPE = 'GRU' on the HIP path (csrc/mogan_rnn.hip) -- the eval forward as one launch, the
training forward and back-propagation through time through the module, the three entry points under the memory contract, two
whole pre-training steps against the CPU restatement in fp64 (tests/damsm_gru_cases.py) and the pre-training entry point.

The references are torch on the CPU in fp64 (stock nn.Embedding / nn.GRU, and a step-by-step restatement that keeps what the
kernels save); every bound is stated where it is used and none of them is derived from the code under test."""
import ctypes
import os

import numpy as np
import pytest
import torch

import damsm_gru_cases as GC
import memguard as MG
from helpers import det_array, load_pkg, max_abs, rel_l2

load_pkg()
from mogan_amd.hip import lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ERR_SHAPE = -1
CASES = [(16, 12, [12, 12, 11, 10, 9, 9, 8, 8, 7, 7, 6, 6, 5, 5, 5, 5]), (6, 18, [15, 11, 9, 9, 6, 1]), (1, 12, [12]),
         (3, 32, [32, 20, 2])]


def T(name, shape, scale=1.0, shift=0.0):
    return torch.from_numpy(det_array(name, shape, scale, shift))


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _stats(*keys):
    return tuple(ops.PK_STATS.get(k, 0) for k in keys)


def _gru_encoder(model, cfg, seed):
    cfg.RNN_TYPE = 'GRU'
    try:
        torch.manual_seed(seed)
        return model.RNN_ENCODER(300, nhidden=256)
    finally:
        cfg.RNN_TYPE = 'LSTM'


def _captions(B, Tw, lens):
    cap = torch.zeros(B, Tw, dtype=torch.int64)
    for i, n in enumerate(lens):
        cap[i, :n] = torch.randint(1, 300, (n,))
    return cap


# ------------------------------------------------------------------------------------------- 1: eval forward, one launch
@pytest.mark.parametrize("case", CASES)
def test_gru_text_encoder_as_one_launch(case):
    """mogan_gru_encoder_fwd: RNN_ENCODER.forward with RNN_TYPE = 'GRU' in eval mode without gradients as one launch, against
    the stock nn.Embedding / nn.GRU path of the same module on the device (MIOpen) and against torch on the CPU in fp64, with
    a zero and a non-zero initial state: max-abs <= 5e-6 for words and sent (the project's figure for the LSTM eval kernel;
    torch's own fp32 nn.GRU on the CPU deviates from fp64 by at most 7.1e-8 on these cases), exact zeros behind each end,
    gru_fused counts the calls and stays put with FUSED = False."""
    from mogan_amd.attngan import model
    from mogan_amd.attngan.miscc.config import cfg
    B, Tw, lens = case
    enc = _gru_encoder(model, cfg, 5 + B).to(DEV).eval()
    assert isinstance(enc.rnn, torch.nn.GRU) and enc.rnn_type == 'GRU'
    enc64 = _gru_encoder(model, cfg, 0).double().eval()
    enc64.load_state_dict({k: v.double().cpu() for k, v in enc.state_dict().items()})
    cap = _captions(B, Tw, lens).to(DEV)
    for zero_state in (True, False):
        hid = enc.init_hidden(B)
        assert torch.is_tensor(hid) and tuple(hid.shape) == (2, B, 128)
        if not zero_state:
            hid = T("gruh_%d" % B, tuple(hid.shape), 0.5).to(DEV)
        with torch.no_grad():
            n0, l0 = _stats("gru_fused", "lstm_fused")
            w1, s1 = enc(cap, torch.tensor(lens), hid)
            assert _stats("gru_fused", "lstm_fused") == (n0 + 1, l0)
            model.RNN_ENCODER.FUSED = False
            try:
                w0, s0 = enc(cap, torch.tensor(lens), hid)
            finally:
                model.RNN_ENCODER.FUSED = True
            assert _stats("gru_fused", "lstm_fused") == (n0 + 1, l0)
            w64, s64 = enc64(cap.cpu(), torch.tensor(lens), hid.double().cpu())
        assert tuple(w1.shape) == tuple(w0.shape) == (B, 256, max(lens)) and tuple(s1.shape) == tuple(s0.shape) == (B, 256)
        print("zero_state=%s max|fused - fp64| words %.2e sent %.2e; stock on the device %.2e %.2e; fused - stock %.2e %.2e"
              % (zero_state, max_abs(w1, w64), max_abs(s1, s64), max_abs(w0, w64), max_abs(s0, s64), max_abs(w1, w0),
                 max_abs(s1, s0)))
        assert max_abs(w1, w64) <= 5e-6 and max_abs(s1, s64) <= 5e-6
        assert max_abs(w1, w0) <= 5e-6 and max_abs(s1, s0) <= 5e-6
        for i, n in enumerate(lens):                                   # exact zeros behind every caption's end
            if n < max(lens):
                assert float(w1[i, :, n:].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------- 2: training forward / backward
def _encoder_grads(enc, cap, lens, hid, mask, gw, gs):
    enc.zero_grad()
    w, s = enc(cap, torch.tensor(lens), hid, drop_mask=mask)
    ((w * gw).sum() + (s * gs).sum()).backward()
    return w.detach(), s.detach(), {k: p.grad.detach().clone() for k, p in enc.named_parameters()}


@pytest.mark.parametrize("case", CASES)
def test_gru_text_encoder_training_forward_and_backward(case):
    """RNN_ENCODER (GRU) with gradients on the fused path (mogan_gru_encoder_train_fwd / _bwd, mogan_embedding_bwd, mogan_bmm)
    -- (a) -- against (b) the stock modules on the device and (c) the stock modules on the CPU in fp64: training mode with an
    injected keep mask (p = 0.5) and a token repeated inside caption 0, eval mode without a mask, and training mode with a
    non-zero initial state (h' holds z * h and dW_hh reads h0 at the walk's first step).
    Forward: max |a - c| <= 5e-6, exact zeros behind each end.  Gradients of the nine parameters, per tensor:
    rel_l2(a, c) <= 4 * max(rel_l2(b, c), rel_l2(c32, c)), c32 = (c) in fp32 -- the rule of
    test_text_encoder_training_forward_and_backward; where MIOpen's GRU cannot differentiate a case (it raises), the cpu-fp32
    term alone is used.  Rows of absent tokens: gradient exactly 0.  A second run gives the same bits; gru_train_fused counts
    the calls and the lstm_* counters do not move."""
    from mogan_amd.attngan import model
    from mogan_amd.attngan.miscc.config import cfg
    B, Tw, lens = case
    enc = _gru_encoder(model, cfg, 5 + B).to(DEV)
    cap = _captions(B, Tw, lens)
    cap[0, 1] = cap[0, 0]
    mask = (torch.rand(B, Tw, 300) >= 0.5).to(torch.uint8)
    gw, gs = torch.randn(B, 256, max(lens)), torch.randn(B, 256)
    h0 = T("gruh0_%d" % B, (2, B, 128), 0.5)
    enc64 = _gru_encoder(model, cfg, 0).double()
    enc64.load_state_dict({k: v.double().cpu() for k, v in enc.state_dict().items()})
    enc32 = _gru_encoder(model, cfg, 0)
    enc32.load_state_dict({k: v.cpu() for k, v in enc.state_dict().items()})
    for train, nonzero in ((True, False), (False, False), (True, True)):
        m = mask if train else None
        md = m.to(DEV) if train else None
        hid = h0 if nonzero else torch.zeros(2, B, 128)
        for e in (enc, enc64, enc32):
            e.train(train)
        n_t, n_e, l_t, l_e = _stats("gru_train_fused", "gru_fused", "lstm_train_fused", "lstm_fused")
        wa, sa, ga = _encoder_grads(enc, cap.to(DEV), lens, hid.to(DEV), md, gw.to(DEV), gs.to(DEV))
        assert _stats("gru_train_fused", "gru_fused", "lstm_train_fused", "lstm_fused") == (n_t + 1, n_e, l_t, l_e)
        wa2, sa2, ga2 = _encoder_grads(enc, cap.to(DEV), lens, hid.to(DEV), md, gw.to(DEV), gs.to(DEV))
        model.RNN_ENCODER.FUSED = False
        enc.rnn.train()             # MIOpen's RNNs differentiate in training mode only; one layer: the same arithmetic
        gb = None
        try:
            wb, sb, gb = _encoder_grads(enc, cap.to(DEV), lens, hid.to(DEV), md, gw.to(DEV), gs.to(DEV))
        except RuntimeError as exc:                                    # MIOpen declines: the cpu-fp32 term alone bounds
            print("stock nn.GRU on the device does not differentiate this case: %r" % (exc,))
        finally:
            model.RNN_ENCODER.FUSED = True
            enc.rnn.train(train)
        assert _stats("gru_train_fused", "gru_fused", "lstm_train_fused", "lstm_fused") == (n_t + 2, n_e, l_t, l_e)
        wc, sc, gc = _encoder_grads(enc64, cap, lens, hid.double(), m, gw.double(), gs.double())
        _, _, g32 = _encoder_grads(enc32, cap, lens, hid, m, gw, gs)
        torch.cuda.synchronize()
        assert tuple(wa.shape) == (B, 256, max(lens)) and tuple(sa.shape) == (B, 256)
        print("train=%s h0=%s forward max|a-c| words %.2e sent %.2e" % (train, nonzero, max_abs(wa, wc), max_abs(sa, sc)))
        assert max_abs(wa, wc) <= 5e-6 and max_abs(sa, sc) <= 5e-6
        for i, n in enumerate(lens):
            if n < max(lens):
                assert float(wa[i, :, n:].abs().max()) == 0.0
        assert len(ga) == 9 and sorted(ga) == sorted(gc)
        fig = {}
        for k in gc:
            fig[k] = (rel_l2(ga[k], gc[k]), rel_l2(gb[k], gc[k]) if gb is not None else 0.0, rel_l2(g32[k], gc[k]))
            print("train=%s h0=%s %-28s fused %.2e  stock-device %.2e  cpu-fp32 %.2e" % ((train, nonzero, k) + fig[k]))
        for k, (a, b, c32) in fig.items():
            assert a <= 4 * max(b, c32), (k, a, b, c32)
        absent = torch.ones(300, dtype=torch.bool)
        for i, n in enumerate(lens):
            absent[cap[i, :n]] = False
        assert bool(absent.any()) and float(ga["encoder.weight"][absent.to(DEV)].abs().max()) == 0.0
        assert torch.equal(_bits(wa), _bits(wa2)) and torch.equal(_bits(sa), _bits(sa2))
        for k in ga:
            assert torch.equal(_bits(ga[k]), _bits(ga2[k])), k


# ------------------------------------------------------------------------------------------- 3: entry points, memory contract
def _gru_reference(cap, lens, emb, W, mask, scale, h0, gw, gs):
    """fp64 restatement of the packed bidirectional GRU, step by step, keeping what the training kernels save: x, the
    post-activation gates r, z, n, hn, the hidden state entering each step, and -- through autograd -- the gradients of the
    input-side and hidden-side pre-activations (dgi, dgh) for upstream gradients (gw, gs).  W[d] = (w_ih, w_hh, b_ih, b_hh);
    h0 (2, B, H) or None."""
    B, H, Tm = cap.shape[0], 128, max(lens)
    f64 = dict(dtype=torch.float64)
    valid = (torch.arange(Tm)[None, :] < torch.tensor(lens)[:, None]).double()[:, :, None]       # zero rows behind each end
    x = (emb[cap[:, :Tm]] * (mask[:, :Tm].double() * scale) * valid).requires_grad_(True)
    out = {"x": x, "gates": torch.zeros(2, B, Tm, 3 * H, **f64), "hn": torch.zeros(2, B, Tm, H, **f64),
           "hprev": torch.zeros(2, B, Tm, H, **f64), "dgi": torch.zeros(2, B, Tm, 3 * H, **f64),
           "dgh": torch.zeros(2, B, Tm, 3 * H, **f64)}
    words = [[None] * Tm for _ in range(B)]
    sent, pres = [], []
    for d in range(2):
        w_ih, w_hh, b_ih, b_hh = W[d]
        fin = []
        for b in range(B):
            h = h0[d, b].clone() if h0 is not None else torch.zeros(H, **f64)
            for s in range(lens[b]):
                t = lens[b] - 1 - s if d else s
                gi = w_ih @ x[b, t] + b_ih + torch.zeros(3 * H, **f64).requires_grad_(True)   # (gh of a first step with a constant
                gh = w_hh @ h + b_hh + torch.zeros(3 * H, **f64).requires_grad_(True)         # h0 would carry no gradient otherwise)
                gi.retain_grad(); gh.retain_grad()
                pres.append((d, b, t, gi, gh))
                r, z = torch.sigmoid(gi[:H] + gh[:H]), torch.sigmoid(gi[H:2 * H] + gh[H:2 * H])
                n = torch.tanh(gi[2 * H:] + r * gh[2 * H:])
                out["hprev"][d, b, t] = h.detach()
                out["gates"][d, b, t] = torch.cat([r, z, n]).detach()
                out["hn"][d, b, t] = gh[2 * H:].detach()
                h = (1 - z) * n + z * h
                words[b][t] = h if d == 0 else torch.cat([words[b][t], h])
            fin.append(h)
        sent.append(torch.stack(fin))
    zr = torch.zeros(2 * H, **f64)
    out["words"] = torch.stack([torch.stack([words[b][t] if t < lens[b] else zr for t in range(Tm)], 1) for b in range(B)])
    out["sent"] = torch.cat(sent, 1)
    ((out["words"] * gw).sum() + (out["sent"] * gs).sum()).backward()
    for d, b, t, gi, gh in pres:
        out["dgi"][d, b, t], out["dgh"][d, b, t] = gi.grad, gh.grad
    out["dx"] = x.grad
    return out


def _pp(tensors):
    arr = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def test_gru_entry_points_under_the_memory_contract():
    """mogan_gru_encoder_fwd, mogan_gru_encoder_train_fwd and mogan_gru_encoder_bwd through ctypes at the smallest shapes that
    reach every branch (B = 4, T = 5, T_max = 4, lens [4, 2, 1, 0], E = 8, V = 7, H = 128, a repeated token, a keep mask, scale
    2.0; the training pair with a non-zero h0, the eval entry with h0 = NULL): outputs in guard-banded, poisoned buffers, inputs
    NaN-banded and frozen.  All written, nothing outside touched, inputs unchanged; the forward to 5e-6, the saved tensors, dgi,
    dgh and both bias gradients to 2e-5 x the tensor's largest magnitude (the project's figure for such results) against the
    fp64 restatement; exact zeros at t >= lens; the empty caption gives a zero row, sent = h0 and zero gradients; d b_hh's n
    block differs from d b_ih's while the r and z blocks are equal; a second backward gives the same bits; declined calls leave
    every buffer untouched; the chain through mogan_embedding_bwd into a finite base is correct."""
    so = lib.load()
    B, Tt, Tm, lens, E, V, H = 4, 5, 4, [4, 2, 1, 0], 8, 7, 128
    g = torch.Generator().manual_seed(11)
    cap = torch.zeros(B, Tt, dtype=torch.int64)
    for i, n in enumerate(lens):
        cap[i, :n] = torch.randint(1, V - 1, (n,), generator=g)         # token V - 1 stays absent
    cap[0, 1] = cap[0, 0]
    emb = torch.rand(V, E, generator=g) * 0.2 - 0.1
    W = [tuple((torch.rand(*s, generator=g) * 2 - 1) / np.sqrt(H) for s in ((3 * H, E), (3 * H, H), (3 * H,), (3 * H,)))
         for _ in range(2)]
    mask = (torch.rand(B, Tt, E, generator=g) >= 0.5).to(torch.uint8)
    scale = 2.0
    h0 = torch.rand(2, B, H, generator=g) - 0.5
    gw, gs = torch.randn(B, 2 * H, Tm, generator=g), torch.randn(B, 2 * H, generator=g)
    W64 = [tuple(w.double() for w in Wd) for Wd in W]
    ref = _gru_reference(cap, lens, emb.double(), W64, mask, scale, h0.double(), gw.double(), gs.double())
    ref_eval = _gru_reference(cap, lens, emb.double(), W64, torch.ones_like(mask), 1.0, None, gw.double(), gs.double())

    def banded(t):                      # an input: its own allocation with NaN bands, frozen
        gd = MG.Guarded(tuple(t.shape), (slice(None),), DEV, dtype=t.dtype, base=t.to(DEV))
        return gd, MG.Frozen(gd.view)
    ins = {k: banded(v) for k, v in dict(cap8=cap.view(torch.uint8).reshape(B, Tt * 8), emb=emb, mask=mask, gw=gw, gs=gs, h0=h0,
                                         **{"w%d%d" % (d, k): W[d][k] for d in range(2) for k in range(4)}).items()}
    ptr = lambda k: ins[k][0].ptr
    keep = [_pp([ins["w0%d" % k][0].view, ins["w1%d" % k][0].view]) for k in range(4)]
    lens_c = (ctypes.c_int * B)(*lens)
    lens_p = ctypes.cast(lens_c, ctypes.c_void_p)
    full = (slice(None),)
    guarded = lambda shapes: {k: MG.Guarded(s, full, DEV) for k, s in shapes.items()}
    # ---- the eval entry, h0 = NULL
    ev = guarded(dict(words=(B, 2 * H, Tm), sent=(B, 2 * H)))

    def efwd(B_=B, Tt_=Tt, Tm_=Tm, E_=E, H_=H, emb_p=None, lens_=lens_p, words_p=None):
        return so.mogan_gru_encoder_fwd(ptr("cap8"), lens_, ptr("emb") if emb_p is None else emb_p, keep[0][1], keep[1][1],
                                        keep[2][1], keep[3][1], None, ev["words"].ptr if words_p is None else words_p,
                                        ev["sent"].ptr, B_, Tt_, Tm_, V, E_, H_, lib.stream_ptr())
    declined = (dict(H_=64), dict(B_=65), dict(Tm_=33, Tt_=33), dict(E_=6), dict(emb_p=0), dict(lens_=None))
    for kw in declined + (dict(words_p=0),):
        assert efwd(**kw) == ERR_SHAPE, kw
    torch.cuda.synchronize()
    assert all(o.untouched() for o in ev.values())
    assert efwd() == 0
    torch.cuda.synchronize()
    for k, o in ev.items():
        o.check(ref_eval[k].detach(), atol=5e-6, what="fwd " + k)
    assert float(ev["words"].view[3].abs().sum()) == 0.0 and float(ev["sent"].view[3].abs().sum()) == 0.0     # empty, h0 NULL
    # ---- the training forward, h0 given
    outs = guarded(dict(words=(B, 2 * H, Tm), sent=(B, 2 * H), x=(B, Tm, E), gates=(2, B, Tm, 3 * H), hn=(2, B, Tm, H),
                        hprev=(2, B, Tm, H)))

    def fwd(B_=B, Tt_=Tt, Tm_=Tm, E_=E, H_=H, emb_p=None, lens_=lens_p, hn_p=None):
        return so.mogan_gru_encoder_train_fwd(ptr("cap8"), lens_, ptr("emb") if emb_p is None else emb_p, keep[0][1], keep[1][1],
                                              keep[2][1], keep[3][1], ptr("h0"), ptr("mask"), scale, outs["words"].ptr,
                                              outs["sent"].ptr, outs["x"].ptr, outs["gates"].ptr,
                                              outs["hn"].ptr if hn_p is None else hn_p, outs["hprev"].ptr, B_, Tt_, Tm_, V, E_,
                                              H_, lib.stream_ptr())
    for kw in declined + (dict(hn_p=0),):
        assert fwd(**kw) == ERR_SHAPE, kw
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs.values())
    assert fwd() == 0
    torch.cuda.synchronize()
    for k, o in outs.items():
        r = ref[k].detach()
        o.check(r, atol=5e-6 if k in ("words", "sent") else 2e-5 * float(r.abs().max()), what="train_fwd " + k)
    for i, n in enumerate(lens):
        assert float(outs["words"].view[i, :, n:].abs().sum()) == 0.0 and float(outs["x"].view[i, n:].abs().sum()) == 0.0
        for k in ("gates", "hn", "hprev"):
            assert float(outs[k].view[:, i, n:].abs().sum()) == 0.0, k
    assert torch.equal(_bits(outs["sent"].view[3]), _bits(torch.cat([h0[0, 3], h0[1, 3]]).to(DEV)))          # empty: sent = h0
    # ---- backward: the saved tensors become frozen inputs
    saved = {k: MG.Frozen(outs[k].view) for k in ("gates", "hn", "hprev", "x")}
    bw = guarded(dict(dgi=(2, B, Tm, 3 * H), dgh=(2, B, Tm, 3 * H), dbi=(2, 3 * H), dbh=(2, 3 * H)))
    whh = _pp([ins["w01"][0].view, ins["w11"][0].view])

    def bwd(B_=B, Tm_=Tm, H_=H, gates_p=None, lens_=lens_p, dgh_p=None):
        return so.mogan_gru_encoder_bwd(ptr("gw"), ptr("gs"), lens_, outs["gates"].ptr if gates_p is None else gates_p,
                                        outs["hn"].ptr, outs["hprev"].ptr, whh[1], bw["dgi"].ptr,
                                        bw["dgh"].ptr if dgh_p is None else dgh_p, bw["dbi"].ptr, bw["dbh"].ptr, B_, Tm_, H_,
                                        lib.stream_ptr())
    for kw in (dict(H_=64), dict(B_=65), dict(Tm_=33), dict(gates_p=0), dict(lens_=None), dict(dgh_p=0)):
        assert bwd(**kw) == ERR_SHAPE, kw
    torch.cuda.synchronize()
    assert all(o.untouched() for o in bw.values())
    assert bwd() == 0
    torch.cuda.synchronize()
    want = dict(dgi=ref["dgi"], dgh=ref["dgh"], dbi=ref["dgi"].sum((1, 2)), dbh=ref["dgh"].sum((1, 2)))
    for k, o in bw.items():
        o.check(want[k], atol=2e-5 * float(want[k].abs().max()), what="gru_bwd " + k)
    for i, n in enumerate(lens):
        assert float(bw["dgi"].view[:, i, n:].abs().sum()) == 0.0 and float(bw["dgh"].view[:, i, n:].abs().sum()) == 0.0
    dbi, dbh = bw["dbi"].view, bw["dbh"].view
    assert float((want["dbi"][:, 2 * H:] - want["dbh"][:, 2 * H:]).abs().max()) > 1e-3 * float(want["dbi"].abs().max())
    assert torch.equal(_bits(dbi[:, :2 * H]), _bits(dbh[:, :2 * H])) and not torch.equal(_bits(dbi[:, 2 * H:]), _bits(dbh[:, 2 * H:]))
    first = {k: _bits(o.view).clone() for k, o in bw.items()}
    for o in bw.values():
        o.reset()
    assert bwd() == 0
    torch.cuda.synchronize()
    for k, o in bw.items():
        assert torch.equal(_bits(o.view), first[k]), k
    # ---- the chain into the embedding gradient: dx = sum_d dgi[d] . W_ih[d] (fp64 here, from the kernel's dgi), then
    # mogan_embedding_bwd adds into a finite base
    dgi64 = bw["dgi"].view.cpu().double()
    dx_k = sum(dgi64[d].reshape(B * Tm, 3 * H) @ W64[d][0] for d in range(2)).reshape(B, Tm, E)
    assert float((dx_k - ref["dx"]).abs().max()) <= 2e-5 * float(ref["dx"].abs().max())
    dx = MG.Guarded((B, Tm, E), full, DEV, base=dx_k.float().to(DEV))
    dxf = MG.Frozen(dx.view)
    base = torch.rand(V, E, generator=g)
    demb = MG.Guarded((V, E), full, DEV, base=base.to(DEV))
    assert so.mogan_embedding_bwd(ptr("cap8"), lens_p, dx.ptr, ptr("mask"), scale, demb.ptr, B, Tt, Tm, V, E, lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    wante = base.double().clone()
    dxm = ref["dx"] * (mask[:, :Tm].double() * scale)
    for b in range(B):
        for t in range(lens[b]):
            wante[cap[b, t]] += dxm[b, t]
    demb.check(wante, atol=2e-5 * float(wante.abs().max()), what="embedding_bwd after gru_bwd")
    absent = [v for v in range(V) if not any(int(cap[b, t]) == v for b in range(B) for t in range(lens[b]))]
    assert absent and torch.equal(_bits(demb.view[absent]), _bits(base[absent].to(DEV)))
    for k, (gd, fr) in ins.items():
        fr.check("input " + k)
    for k, fr in saved.items():
        fr.check("saved " + k)
    dxf.check("dx")


# ------------------------------------------------------------------------------------------- 4: two pre-training steps
def test_two_gru_pretraining_steps_against_the_fp64_restatement():
    """DAMSMEngine.step_from_features twice with RNN_TYPE = 'GRU' on the inputs, masks, LR and CLIP of
    test_two_pretraining_steps_against_the_fp64_restatement, against tests/damsm_gru_cases.reference_steps in fp64 under
    damsm_pretrain_cases.check_steps: the four losses and the pre-clip norm to rtol 2e-5, the clipped gradients to rel-L2 2e-5
    per tensor, the update element by element, >= 95 % of the 1 066 392 elements judged.  tests/test_gru_encoder_cpu.py holds
    torch's own fp32 to the same assertions."""
    from mogan_amd.attngan import model, pretrain_DAMSM as PD
    from mogan_amd.attngan.miscc.config import cfg
    cfg.TRAIN.FLAG, cfg.ADAM_EPS_MODE = True, 0
    cfg.TRAIN.SMOOTH.GAMMA1, cfg.TRAIN.SMOOTH.GAMMA2, cfg.TRAIN.SMOOTH.GAMMA3 = 4.0, 5.0, 10.0
    inp = GC.make_inputs()
    ref = GC.reference_steps(inp, torch.float64)
    cfg.RNN_TYPE = 'GRU'
    try:
        text, image = model.RNN_ENCODER(GC.V, nhidden=GC.NEF), model.CNN_ENCODER(GC.NEF)
    finally:
        cfg.RNN_TYPE = 'LSTM'
    text.load_state_dict({k: v for k, v in inp["weights"].items() if k in GC.TEXT_KEYS})
    image.load_state_dict({k: v for k, v in inp["weights"].items() if k in GC.HEAD_KEYS}, strict=False)
    eng = PD.DAMSMEngine(text.to(DEV), image.to(DEV), lr=GC.LR, clip=GC.CLIP)
    params = dict([(k, p) for k, p in text.named_parameters()] +
                  [(k, p) for k, p in image.named_parameters() if k in GC.HEAD_KEYS])
    assert sum(p.numel() for p in eng.opt.params) == GC.N_PARAMS and sorted(params) == sorted(GC.TEXT_KEYS + GC.HEAD_KEYS)
    assert eng.n_text >= sum(p.numel() for p in text.parameters())
    feat, code, cap = inp["feat768"].to(DEV), inp["code2048"].to(DEV), inp["captions"].to(DEV)
    n0 = _stats("gru_train_fused", "lstm_train_fused")
    got = []
    for s in range(GC.STEPS):
        before = {k: p.detach().clone() for k, p in params.items()}
        w0, w1, s0, s1, norm = eng.step_from_features(feat, code, cap, torch.tensor(inp["lens"]), np.arange(GC.B),
                                                      drop_mask=inp["masks"][s].to(DEV))
        torch.cuda.synchronize()
        got.append({"losses": [float(v) for v in (w0, w1, s0, s1)], "norm": float(norm),
                    "grad": {k: p.grad.detach().clone() for k, p in params.items()},
                    "delta": {k: p.detach() - before[k] for k, p in params.items()}})
    assert _stats("gru_train_fused", "lstm_train_fused") == (n0[0] + GC.STEPS, n0[1])
    GC.check_steps(got, ref, what="hip GRU")


# ------------------------------------------------------------------------------------------- 5: the entry point
def test_pretrain_entry_point_trains_and_reloads_a_gru_encoder(tmp_path):
    """pretrain_DAMSM.py --synthetic 2 on the yml of test_pretrain_entry_point_writes_loadable_encoders plus RNN_TYPE: 'GRU'
    (the public switch), with TEXT.EMBEDDING_DIM at the model's 256: that yml's 32 gives 16 units per direction, which the
    kernels decline by contract (H == 128), and then no counter could rise.  Both iterations run the fused training path, the
    written text state_dict has nn.GRU's keys and shapes, condGANTrainer.build_models loads the pair through TRAIN.NET_E, and
    one no_grad forward of the loaded text encoder is the one-launch eval kernel (gru_fused rises)."""
    from mogan_amd.attngan import pretrain_DAMSM as PD
    from mogan_amd.attngan.datasets import SyntheticTextDataset
    from mogan_amd.attngan.miscc.config import cfg
    from mogan_amd.attngan.trainer import condGANTrainer
    yml = tmp_path / "damsm_gru.yml"
    yml.write_text("CONFIG_NAME: 'damsm'\nDATASET_NAME: 'coco'\nWORKERS: 0\nRNN_TYPE: 'GRU'\nTREE: {BRANCH_NUM: 1, BASE_SIZE: 64}\n"
                   "GAN: {DF_DIM: 8, GF_DIM: 8, Z_DIM: 100, R_NUM: 1}\n"
                   "TEXT: {EMBEDDING_DIM: 256, CAPTIONS_PER_IMAGE: 5, WORDS_NUM: 12}\n"
                   "TRAIN: {FLAG: True, BATCH_SIZE: 4, MAX_EPOCH: 1, SNAPSHOT_INTERVAL: 1, NET_E: '', ENCODER_LR: 0.002}\n")
    out = tmp_path / "out"
    nef_was = cfg.TEXT.EMBEDDING_DIM
    try:
        n_t = _stats("gru_train_fused", "lstm_train_fused")
        eng = PD.main(["--cfg", str(yml), "--synthetic", "2", "--manualSeed", "7", "--output_dir", str(out)])
        assert float(eng.opt.state[0]) == 2.0                          # two iterations ...
        assert _stats("gru_train_fused", "lstm_train_fused") == (n_t[0] + 2, n_t[1])          # ... on the GRU kernels
        assert isinstance(eng.text_encoder.rnn, torch.nn.GRU)
        tp, ip = [os.path.join(str(out), "Model", "%s_encoder0.pth" % k) for k in ("text", "image")]
        tsd = torch.load(tp, map_location="cpu")
        ds = SyntheticTextDataset(length=4)
        gru = torch.nn.GRU(300, 128, 1, batch_first=True, bidirectional=True)
        want = [("encoder.weight", (ds.n_words, 300))] + [("rnn." + k, tuple(v.shape)) for k, v in gru.state_dict().items()]
        assert [(k, tuple(v.shape)) for k, v in tsd.items()] == want
        assert all(torch.isfinite(v).all() for v in tsd.values())
        assert os.path.isfile(ip)
        cfg.TRAIN.NET_E = tp
        algo = condGANTrainer(str(out), None, ds.n_words, ds.ixtoword, resume=False)
        text = algo.build_models()[0]
        for k, v in text.state_dict().items():
            assert torch.equal(v.cpu(), tsd[k]), k
        assert isinstance(text.rnn, torch.nn.GRU) and not text.training
        cap = torch.zeros(4, 12, dtype=torch.int64)
        lens = [12, 9, 4, 1]
        for i, n in enumerate(lens):
            cap[i, :n] = torch.randint(1, ds.n_words, (n,))
        dev = next(text.parameters()).device
        n_e = _stats("gru_fused", "lstm_fused")
        with torch.no_grad():
            words, sent = text(cap.to(dev), torch.tensor(lens), text.init_hidden(4))
        torch.cuda.synchronize()
        assert _stats("gru_fused", "lstm_fused") == (n_e[0] + 1, n_e[1])
        assert tuple(words.shape) == (4, 256, 12) and tuple(sent.shape) == (4, 256)
        assert bool(torch.isfinite(words).all()) and bool(torch.isfinite(sent).all())
    finally:
        cfg.RNN_TYPE, cfg.TRAIN.NET_E, cfg.TEXT.EMBEDDING_DIM = 'LSTM', '', nef_was
