"""-m gpu: DAMSM pre-training on the HIP path -- the text side of the matching losses, the text encoder's training forward and
back-propagation through time, the five new entry points under the memory contract, two whole pre-training steps against the
CPU restatement in fp64 (tests/damsm_pretrain_cases.py), the entry point, and CNN_ENCODER with trainable heads.

The references are torch on the CPU in fp64 (oracle/attngan_oracle.py, stock nn.Embedding / nn.LSTM); every bound is stated
where it is used and none of them is derived from the code under test."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import damsm_pretrain_cases as DC
import memguard as MG
from helpers import det_array, load_pkg, max_abs, rel_l2
from oracle import attngan_oracle as O

load_pkg()
from mogan_amd.hip import lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ERR_SHAPE = -1


def T(name, shape, scale=1.0, shift=0.0):
    return torch.from_numpy(det_array(name, shape, scale, shift))


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------- 1: text side of the losses
@pytest.mark.parametrize("B,C,hw,Tw,same_class", [(16, 256, 17, 12, False), (5, 32, 6, 7, True), (3, 16, 17, 18, False)])
def test_damsm_losses_text_side_gradients(B, C, hw, Tw, same_class):
    """words_loss / sent_loss with BOTH sides requiring a gradient, on the cases, inputs, loss weights and lengths of
    test_kernels_gpu.py::test_damsm_words_and_sentence_losses, against the fp64 oracle: rel-L2 <= 2e-5 for d words and d sent
    (the project's figure for the image side of the same function; 4 x torch's own fp32 CPU error on the text side, which is
    4.96e-6 / 8.6e-7 / 9.8e-7 for d words at the three cases), unchanged for d feat and d code; d words exactly 0 behind each
    caption's end; a second backward gives the same bits."""
    from mogan_amd.attngan.miscc import losses as L
    from mogan_amd.attngan.miscc.config import cfg
    cfg.TRAIN.SMOOTH.GAMMA1, cfg.TRAIN.SMOOTH.GAMMA2, cfg.TRAIN.SMOOTH.GAMMA3 = 4.0, 5.0, 10.0
    ocfg = O.Cfg(words_num=Tw)
    feat = T("damsm.feat%d" % B, (B, C, hw, hw))
    words = T("damsm.words%d" % B, (B, C, Tw))
    code, sent = T("damsm.code%d" % B, (B, C)), T("damsm.sent%d" % B, (B, C))
    lens = np.sort(np.random.RandomState(B).randint(2, Tw + 1, B))[::-1].copy()
    lens[0] = Tw
    class_ids = np.arange(B)
    if same_class:
        class_ids[2] = class_ids[0]
    ref = [t.double().requires_grad_(True) for t in (feat, words, code, sent)]
    w0, w1, _ = O.words_loss(ref[0], ref[1], lens, ocfg, class_ids if same_class else None)
    s0, s1 = O.sent_loss(ref[2], ref[3], ocfg, class_ids if same_class else None)
    (1.3 * w0 + 0.7 * w1 + 2.0 * s0 + 0.5 * s1).backward()
    for i in range(B):
        assert float(ref[1].grad[i, :, int(lens[i]):].abs().sum()) == 0.0        # the oracle's padded positions: exactly 0
    lab = torch.arange(B, device=DEV)
    lens_t = torch.from_numpy(lens.astype(np.int64))
    runs = []
    for _ in range(2):
        got = [t.to(DEV).requires_grad_(True) for t in (feat, words, code, sent)]
        g0, g1, _ = L.words_loss(got[0], got[1], lab, lens_t, class_ids, B)
        t0, t1 = L.sent_loss(got[2], got[3], lab, class_ids, B)
        ops.scalar_sum([g0, g1, t0, t1], [1.3, 0.7, 2.0, 0.5]).backward()
        torch.cuda.synchronize()
        runs.append([t.grad.clone() for t in got])
    for a, want, k in ((g0, w0, "w0"), (g1, w1, "w1"), (t0, s0, "s0"), (t1, s1, "s1")):
        np.testing.assert_allclose(float(a), float(want), rtol=2e-5, err_msg=k)
    rels = [rel_l2(a, r.grad) for a, r in zip(runs[0], ref)]
    print("rel-L2 d feat %.2e, d words %.2e, d code %.2e, d sent %.2e" % tuple(rels))
    assert all(r <= 2e-5 for r in rels), rels
    for i in range(B):
        assert float(runs[0][1][i, :, int(lens[i]):].abs().sum()) == 0.0
    for a, b in zip(*runs):
        assert torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------- 2: LSTM forward / backward
LSTM_CASES = [(16, 12, [12, 12, 11, 10, 9, 9, 8, 8, 7, 7, 6, 6, 5, 5, 5, 5]), (6, 18, [15, 11, 9, 9, 6, 1]), (1, 12, [12]),
              (3, 32, [32, 20, 2])]


def _encoder_grads(enc, cap, lens, mask, gw, gs):
    enc.zero_grad()
    w, s = enc(cap, torch.tensor(lens), enc.init_hidden(cap.shape[0]), drop_mask=mask)
    ((w * gw).sum() + (s * gs).sum()).backward()
    return w.detach(), s.detach(), {k: p.grad.detach().clone() for k, p in enc.named_parameters()}


@pytest.mark.parametrize("case", LSTM_CASES)
def test_text_encoder_training_forward_and_backward(case):
    """RNN_ENCODER with gradients on the fused path (mogan_lstm_encoder_train_fwd / _bwd, mogan_embedding_bwd, mogan_bmm) --
    (a) -- against (b) the stock modules on the device and (c) the stock modules on the CPU in fp64, same injected keep mask
    (p = 0.5) and a token repeated inside caption 0; then once more in eval mode without a mask.
    Forward: max |a - c| <= 5e-6 (the eval kernel's figure), exact zeros behind each end.  Gradients of the nine parameters, per
    tensor: rel_l2(a, c) <= 4 * max(rel_l2(b, c), rel_l2(c32, c)), c32 = (c) in fp32 -- the bound comes from the two references
    alone.  Rows of tokens absent from the batch: gradient exactly 0.  A second run gives the same bits."""
    from mogan_amd.attngan import model
    from mogan_amd.attngan.miscc.config import cfg
    B, Tw, lens = case
    cfg.RNN_TYPE = 'LSTM'
    torch.manual_seed(5 + B)
    enc = model.RNN_ENCODER(300, nhidden=256).to(DEV)
    cap = torch.zeros(B, Tw, dtype=torch.int64)
    for i, n in enumerate(lens):
        cap[i, :n] = torch.randint(1, 300, (n,))
    cap[0, 1] = cap[0, 0]
    mask = (torch.rand(B, Tw, 300) >= 0.5).to(torch.uint8)
    gw, gs = torch.randn(B, 256, max(lens)), torch.randn(B, 256)
    enc64 = model.RNN_ENCODER(300, nhidden=256).double()
    enc64.load_state_dict({k: v.double().cpu() for k, v in enc.state_dict().items()})
    enc32 = model.RNN_ENCODER(300, nhidden=256)
    enc32.load_state_dict({k: v.cpu() for k, v in enc.state_dict().items()})
    for train in (True, False):
        m = mask if train else None
        for e in (enc, enc64, enc32):
            e.train(train)
        n_t, n_e = ops.PK_STATS.get("lstm_train_fused", 0), ops.PK_STATS.get("lstm_fused", 0)
        wa, sa, ga = _encoder_grads(enc, cap.to(DEV), lens, m.to(DEV) if train else None, gw.to(DEV), gs.to(DEV))
        assert ops.PK_STATS.get("lstm_train_fused", 0) == n_t + 1 and ops.PK_STATS.get("lstm_fused", 0) == n_e
        wa2, sa2, ga2 = _encoder_grads(enc, cap.to(DEV), lens, m.to(DEV) if train else None, gw.to(DEV), gs.to(DEV))
        model.RNN_ENCODER.FUSED = False
        enc.rnn.train()             # MIOpen's LSTM differentiates in training mode only; one layer: the same arithmetic
        try:
            wb, sb, gb = _encoder_grads(enc, cap.to(DEV), lens, m.to(DEV) if train else None, gw.to(DEV), gs.to(DEV))
        finally:
            model.RNN_ENCODER.FUSED = True
            enc.rnn.train(train)
        assert ops.PK_STATS.get("lstm_train_fused", 0) == n_t + 2
        wc, sc, gc = _encoder_grads(enc64, cap, lens, m, gw.double(), gs.double())
        _, _, g32 = _encoder_grads(enc32, cap, lens, m, gw, gs)
        torch.cuda.synchronize()
        assert tuple(wa.shape) == (B, 256, max(lens)) and tuple(sa.shape) == (B, 256)
        print("train=%s forward max|a-c| words %.2e sent %.2e (stock on the device %.2e)"
              % (train, max_abs(wa, wc), max_abs(sa, sc), max_abs(wb, wc)))
        assert max_abs(wa, wc) <= 5e-6 and max_abs(sa, sc) <= 5e-6
        for i, n in enumerate(lens):
            if n < max(lens):
                assert float(wa[i, :, n:].abs().max()) == 0.0
        assert len(ga) == 9
        for k in gc:
            a, b, c32 = rel_l2(ga[k], gc[k]), rel_l2(gb[k], gc[k]), rel_l2(g32[k], gc[k])
            print("train=%s %-28s fused %.2e  stock-device %.2e  cpu-fp32 %.2e" % (train, k, a, b, c32))
        for k in gc:
            a, b, c32 = rel_l2(ga[k], gc[k]), rel_l2(gb[k], gc[k]), rel_l2(g32[k], gc[k])
            assert a <= 4 * max(b, c32), (k, a, b, c32)
        absent = torch.ones(300, dtype=torch.bool)
        absent[cap[cap > 0]] = False
        for i, n in enumerate(lens):
            absent[cap[i, :n]] = False
        assert bool(absent.any()) and float(ga["encoder.weight"][absent.to(DEV)].abs().max()) == 0.0
        assert torch.equal(_bits(wa), _bits(wa2)) and torch.equal(_bits(sa), _bits(sa2))
        for k in ga:
            assert torch.equal(_bits(ga[k]), _bits(ga2[k])), k


# ------------------------------------------------------------------------------------------- 3: entry points, memory contract
def _lstm_reference(cap, lens, emb, W, mask, scale, gw, gs):
    """fp64 restatement of the packed bidirectional LSTM, step by step, keeping what the training kernels save: x, the
    post-activation gates, c_t, the hidden state entering each step, and -- through autograd -- the pre-activation gate
    gradients for upstream gradients (gw, gs).  W[d] = (w_ih, w_hh, b_ih, b_hh)."""
    B, H, Tm = cap.shape[0], 128, max(lens)
    valid = (torch.arange(Tm)[None, :] < torch.tensor(lens)[:, None]).double()[:, :, None]       # zero rows behind each end
    x = (emb[cap[:, :Tm]] * (mask[:, :Tm].double() * scale) * valid).requires_grad_(True)
    out = {"x": x, "gates": torch.zeros(2, B, Tm, 4 * H, dtype=torch.float64), "cells": torch.zeros(2, B, Tm, H, dtype=torch.float64),
           "hprev": torch.zeros(2, B, Tm, H, dtype=torch.float64), "dg": torch.zeros(2, B, Tm, 4 * H, dtype=torch.float64)}
    words = [[None] * Tm for _ in range(B)]
    sent, pres = [], []
    for d in range(2):
        w_ih, w_hh, b_ih, b_hh = W[d]
        fin = []
        for b in range(B):
            h, c = torch.zeros(H, dtype=torch.float64), torch.zeros(H, dtype=torch.float64)
            for s in range(lens[b]):
                t = lens[b] - 1 - s if d else s
                pre = w_ih @ x[b, t] + b_ih + w_hh @ h + b_hh
                pre.retain_grad()
                pres.append((d, b, t, pre))
                i, f, g, o = torch.sigmoid(pre[:H]), torch.sigmoid(pre[H:2 * H]), torch.tanh(pre[2 * H:3 * H]), torch.sigmoid(pre[3 * H:])
                out["hprev"][d, b, t] = h.detach()
                c = f * c + i * g
                h = o * torch.tanh(c)
                out["gates"][d, b, t] = torch.cat([i, f, g, o]).detach()
                out["cells"][d, b, t] = c.detach()
                words[b][t] = h if d == 0 else torch.cat([words[b][t], h])
            fin.append(h)
        sent.append(torch.stack(fin))
    z = torch.zeros(2 * H, dtype=torch.float64)
    out["words"] = torch.stack([torch.stack([words[b][t] if t < lens[b] else z for t in range(Tm)], 1) for b in range(B)])
    out["sent"] = torch.cat(sent, 1)
    ((out["words"] * gw).sum() + (out["sent"] * gs).sum()).backward()
    for d, b, t, pre in pres:
        out["dg"][d, b, t] = pre.grad
    out["dx"] = x.grad
    return out


def _pp(tensors):
    arr = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def test_lstm_entry_points_under_the_memory_contract():
    """mogan_lstm_encoder_train_fwd, mogan_lstm_encoder_bwd and mogan_embedding_bwd through ctypes at the smallest shapes that
    reach every branch (B = 3, T = 5, T_max = 4, lens [4, 2, 1], E = 8, V = 7): outputs in guard-banded, poisoned buffers (the
    embedding gradient: a finite base it adds to), inputs NaN-banded and frozen.  All written, nothing outside touched, inputs
    unchanged, values against the fp64 restatement (max-abs <= 2e-5 x the tensor's largest magnitude, the project's figure for
    O(1) element-wise results; the forward to 5e-6); out-of-range arguments are declined with every buffer untouched."""
    so = lib.load()
    B, Tt, Tm, lens, E, V, H = 3, 5, 4, [4, 2, 1], 8, 7, 128
    g = torch.Generator().manual_seed(3)
    cap = torch.zeros(B, Tt, dtype=torch.int64)
    for i, n in enumerate(lens):
        cap[i, :n] = torch.randint(1, V, (n,), generator=g)
    cap[0, 1] = cap[0, 0]
    emb = torch.rand(V, E, generator=g) * 0.2 - 0.1
    W = [tuple((torch.rand(*s, generator=g) * 2 - 1) / np.sqrt(H) for s in ((4 * H, E), (4 * H, H), (4 * H,), (4 * H,)))
         for _ in range(2)]
    mask = (torch.rand(B, Tt, E, generator=g) >= 0.5).to(torch.uint8)
    scale = 2.0
    gw, gs = torch.randn(B, 2 * H, Tm, generator=g), torch.randn(B, 2 * H, generator=g)
    ref = _lstm_reference(cap, lens, emb.double(), [tuple(w.double() for w in Wd) for Wd in W], mask, scale, gw.double(),
                          gs.double())

    def banded(t):                      # an input: its own allocation with NaN bands, frozen
        gd = MG.Guarded(tuple(t.shape), (slice(None),), DEV, dtype=t.dtype, base=t.to(DEV))
        return gd, MG.Frozen(gd.view)
    ins = {k: banded(v) for k, v in dict(cap8=cap.view(torch.uint8).reshape(B, Tt * 8), emb=emb, mask=mask, gw=gw, gs=gs,
                                         **{"w%d%d" % (d, k): W[d][k] for d in range(2) for k in range(4)}).items()}
    ptr = lambda k: ins[k][0].ptr
    keep = [_pp([ins["w0%d" % k][0].view, ins["w1%d" % k][0].view]) for k in range(4)]
    lens_c = (ctypes.c_int * B)(*lens)
    lens_p = ctypes.cast(lens_c, ctypes.c_void_p)
    full = (slice(None),)
    outs = {k: MG.Guarded(s, full, DEV) for k, s in dict(words=(B, 2 * H, Tm), sent=(B, 2 * H), x=(B, Tm, E), gates=(2, B, Tm, 4 * H),
                                                        cells=(2, B, Tm, H), hprev=(2, B, Tm, H)).items()}

    def fwd(B_=B, Tt_=Tt, Tm_=Tm, E_=E, H_=H, emb_p=None, lens_=lens_p):
        return so.mogan_lstm_encoder_train_fwd(ptr("cap8"), lens_, ptr("emb") if emb_p is None else emb_p, keep[0][1], keep[1][1],
                                               keep[2][1], keep[3][1], None, None, ptr("mask"), scale, outs["words"].ptr,
                                               outs["sent"].ptr, outs["x"].ptr, outs["gates"].ptr, outs["cells"].ptr,
                                               outs["hprev"].ptr, B_, Tt_, Tm_, V, E_, H_, lib.stream_ptr())
    # declined calls first: nothing may be written
    for kw in (dict(H_=64), dict(B_=65), dict(Tm_=33, Tt_=33), dict(E_=6), dict(emb_p=0), dict(lens_=None)):
        assert fwd(**kw) == ERR_SHAPE, kw
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs.values())
    assert fwd() == 0
    torch.cuda.synchronize()
    for k, o in outs.items():
        r = ref[k].detach()
        o.check(r, atol=5e-6 if k in ("words", "sent") else 2e-5 * float(r.abs().max()), what="train_fwd " + k)
    for i, n in enumerate(lens):
        assert float(outs["words"].view[i, :, n:].abs().sum()) == 0.0 and float(outs["gates"].view[:, i, n:].abs().sum()) == 0.0
    # backward: the saved tensors become frozen inputs
    saved = {k: MG.Frozen(outs[k].view) for k in ("gates", "cells", "hprev", "x")}
    dg, db = MG.Guarded((2, B, Tm, 4 * H), full, DEV), MG.Guarded((2, 4 * H), full, DEV)
    whh = _pp([ins["w01"][0].view, ins["w11"][0].view])

    def bwd(B_=B, Tm_=Tm, H_=H, gates_p=None):
        return so.mogan_lstm_encoder_bwd(ptr("gw"), ptr("gs"), lens_p, outs["gates"].ptr if gates_p is None else gates_p,
                                         outs["cells"].ptr, outs["hprev"].ptr, None, whh[1], dg.ptr, db.ptr, B_, Tm_, H_,
                                         lib.stream_ptr())
    for kw in (dict(H_=64), dict(B_=65), dict(Tm_=33), dict(gates_p=0)):
        assert bwd(**kw) == ERR_SHAPE, kw
    torch.cuda.synchronize()
    assert dg.untouched() and db.untouched()
    assert bwd() == 0
    torch.cuda.synchronize()
    dg.check(ref["dg"], atol=2e-5 * float(ref["dg"].abs().max()), what="lstm_bwd dgates")
    db_ref = ref["dg"].sum((1, 2))
    db.check(db_ref, atol=2e-5 * float(db_ref.abs().max()), what="lstm_bwd dbias")
    for i, n in enumerate(lens):
        assert float(dg.view[:, i, n:].abs().sum()) == 0.0
    first = _bits(dg.view).clone()
    dg.reset(); db.reset()
    assert bwd() == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(dg.view), first)
    # embedding gradient: adds into a finite base
    dx = MG.Guarded((B, Tm, E), full, DEV, base=ref["dx"].float().to(DEV))
    dxf = MG.Frozen(dx.view)
    base = torch.rand(V, E, generator=g)
    demb = MG.Guarded((V, E), full, DEV, base=base.to(DEV))

    def ebwd(B_=B, Tt_=Tt, Tm_=Tm, E_=E, dx_p=None):
        return so.mogan_embedding_bwd(ptr("cap8"), lens_p, dx.ptr if dx_p is None else dx_p, ptr("mask"), scale, demb.ptr, B_, Tt_,
                                      Tm_, V, E_, lib.stream_ptr())
    for kw in (dict(B_=65), dict(Tm_=33, Tt_=33), dict(E_=6), dict(dx_p=0)):
        assert ebwd(**kw) == ERR_SHAPE, kw
    torch.cuda.synchronize()
    assert demb.untouched()
    assert ebwd() == 0
    torch.cuda.synchronize()
    want = base.double().clone()
    dxm = ref["dx"].float().double() * (mask[:, :Tm].double() * scale)
    for b in range(B):
        for t in range(lens[b]):
            want[cap[b, t]] += dxm[b, t]
    demb.check(want, atol=2e-5 * float(want.abs().max()), what="embedding_bwd")
    absent = [v for v in range(V) if not any(int(cap[b, t]) == v for b in range(B) for t in range(lens[b]))]
    assert absent and torch.equal(_bits(demb.view[absent]), _bits(base[absent].to(DEV)))
    once = _bits(demb.view).clone()
    demb.reset()
    assert ebwd() == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(demb.view), once)
    for k, (gd, fr) in ins.items():
        fr.check("input " + k)
    for k, fr in saved.items():
        fr.check("saved " + k)
    dxf.check("dx")


@pytest.mark.parametrize("S", [9, 330])
def test_damsm_text_entry_points_under_the_memory_contract(S):
    """mogan_damsm_words_bwd_text and mogan_damsm_sent_bwd_text through ctypes (B = 3, C = 10, T = 5, one caption of length 1;
    S = 9 and S = 330, two regions per thread in the kernels that produce wc): the direct term of d words against fp64 autograd
    through the cosines with the weighted contexts held fixed, d rnn against fp64 autograd; max-abs <= 2e-5 x the largest
    magnitude; exact zeros behind each caption's end; declined calls leave the buffers untouched."""
    so = lib.load()
    B, C, Tw, lens = 3, 10, 5, [5, 3, 1]
    g1, g2, g3 = 4.0, 5.0, 10.0
    g = torch.Generator().manual_seed(S)
    ctx, words = torch.randn(B, C, S, generator=g), torch.randn(B, C, Tw, generator=g)
    dsim = torch.randn(B, B, generator=g)
    d = lambda t: t.to(DEV).contiguous()
    ctx_d, lens_d = d(ctx), torch.tensor(lens, dtype=torch.int32, device=DEV)
    f32 = dict(dtype=torch.float32, device=DEV)
    sim, a1, a2 = torch.empty(B, B, **f32), torch.empty(B, B, S, Tw, **f32), torch.empty(B, B, Tw, S, **f32)
    wc = torch.empty(B, C, B, Tw, **f32)
    full = (slice(None),)
    wg = MG.Guarded((B, C, Tw), full, DEV, base=d(words))
    wcg = MG.Guarded((B, C, B, Tw), full, DEV, base=wc)
    assert so.mogan_damsm_words_fwd(ctx_d.data_ptr(), wg.ptr, lens_d.data_ptr(), B, B, C, S, Tw, g1, g2, g3, sim.data_ptr(),
                                    a1.data_ptr(), a2.data_ptr(), wcg.ptr, None, lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    dsg = MG.Guarded((B, B), full, DEV, base=d(dsim))
    frozen = [MG.Frozen(x.view) for x in (wg, wcg, dsg)]
    out = MG.Guarded((B, C, Tw), full, DEV)

    def call(T_=Tw, wc_p=None, B_=B):
        return so.mogan_damsm_words_bwd_text(wg.ptr, lens_d.data_ptr(), wcg.ptr if wc_p is None else wc_p, dsg.ptr, B_, B, C, T_,
                                             g2, g3, out.ptr, lib.stream_ptr())
    for kw in (dict(T_=33), dict(wc_p=0), dict(B_=0)):
        assert call(**kw) == ERR_SHAPE, kw
    torch.cuda.synchronize()
    assert out.untouched()
    assert call() == 0
    torch.cuda.synchronize()
    w64 = words.double().requires_grad_(True)
    wc64 = wcg.view.cpu().double()
    tot = 0
    for i in range(B):
        n = lens[i]
        wi = w64[i, :, :n]                                               # (C, n)
        for b in range(B):
            c = wc64[b, :, i, :n]
            cos = (wi * c).sum(0) / (wi.norm(2, 0) * c.norm(2, 0)).clamp(min=1e-8)
            tot = tot + float(dsim[b, i]) * g3 * torch.log(torch.exp(g2 * cos).sum())
    tot.backward()
    out.check(w64.grad, atol=2e-5 * float(w64.grad.abs().max()), what="words_bwd_text")
    for i, n in enumerate(lens):
        assert float(out.view[i, :, n:].abs().sum()) == 0.0
    once = _bits(out.view).clone()
    out.reset()
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(out.view), once)
    for f in frozen:
        f.check("words_bwd_text")
    # sentence side
    cnn, rnn = torch.randn(B, C, generator=g), torch.randn(B, C, generator=g)
    cg, rg = MG.Guarded((B, C), full, DEV, base=d(cnn)), MG.Guarded((B, C), full, DEV, base=d(rnn))
    frozen = [MG.Frozen(x.view) for x in (cg, rg, dsg)]
    dr = MG.Guarded((B, C), full, DEV)

    def scall(C_=C, rnn_p=None):
        return so.mogan_damsm_sent_bwd_text(cg.ptr, rg.ptr if rnn_p is None else rnn_p, dsg.ptr, B, B, C_, g3, 1e-8, dr.ptr,
                                            lib.stream_ptr())
    for kw in (dict(C_=0), dict(rnn_p=0)):
        assert scall(**kw) == ERR_SHAPE, kw
    torch.cuda.synchronize()
    assert dr.untouched()
    assert scall() == 0
    torch.cuda.synchronize()
    r64 = rnn.double().requires_grad_(True)
    c64 = cnn.double()
    s = c64 @ r64.t() / (c64.norm(2, 1, keepdim=True) @ r64.norm(2, 1, keepdim=True).t()).clamp(min=1e-8) * g3
    (s * dsim.double()).sum().backward()
    dr.check(r64.grad, atol=2e-5 * float(r64.grad.abs().max()), what="sent_bwd_text")
    for f in frozen:
        f.check("sent_bwd_text")


# ------------------------------------------------------------------------------------------- 4: two pre-training steps
def test_two_pretraining_steps_against_the_fp64_restatement():
    """DAMSMEngine.step_from_features twice on fixed inputs against tests/damsm_pretrain_cases.reference_steps in fp64 (stock
    torch modules, the oracle's losses, clip_grad_norm_, torch.optim.Adam) under check_steps: the four losses and the pre-clip
    norm to rtol 2e-5, the clipped gradients to rel-L2 2e-5 per tensor, the update element by element, >= 95 % of the 1 176 472
    elements judged.  tests/test_damsm_pretrain_cpu.py holds torch's own fp32 to the same assertions."""
    from mogan_amd.attngan import model, pretrain_DAMSM as PD
    from mogan_amd.attngan.miscc.config import cfg
    cfg.RNN_TYPE, cfg.TRAIN.FLAG, cfg.ADAM_EPS_MODE = 'LSTM', True, 0
    cfg.TRAIN.SMOOTH.GAMMA1, cfg.TRAIN.SMOOTH.GAMMA2, cfg.TRAIN.SMOOTH.GAMMA3 = 4.0, 5.0, 10.0
    inp = DC.make_inputs()
    ref = DC.reference_steps(inp, torch.float64)
    text, image = model.RNN_ENCODER(DC.V, nhidden=DC.NEF), model.CNN_ENCODER(DC.NEF)
    text.load_state_dict({k: v for k, v in inp["weights"].items() if k in DC.TEXT_KEYS})
    image.load_state_dict({k: v for k, v in inp["weights"].items() if k in DC.HEAD_KEYS}, strict=False)
    eng = PD.DAMSMEngine(text.to(DEV), image.to(DEV), lr=DC.LR, clip=DC.CLIP)
    params = dict([(k, p) for k, p in text.named_parameters()] +
                  [(k, p) for k, p in image.named_parameters() if k in DC.HEAD_KEYS])
    assert sum(p.numel() for p in eng.opt.params) == DC.N_PARAMS and sorted(params) == sorted(DC.TEXT_KEYS + DC.HEAD_KEYS)
    feat, code, cap = inp["feat768"].to(DEV), inp["code2048"].to(DEV), inp["captions"].to(DEV)
    got = []
    for s in range(DC.STEPS):
        before = {k: p.detach().clone() for k, p in params.items()}
        w0, w1, s0, s1, norm = eng.step_from_features(feat, code, cap, torch.tensor(inp["lens"]), np.arange(DC.B),
                                                      drop_mask=inp["masks"][s].to(DEV))
        torch.cuda.synchronize()
        got.append({"losses": [float(v) for v in (w0, w1, s0, s1)], "norm": float(norm),
                    "grad": {k: p.grad.detach().clone() for k, p in params.items()},
                    "delta": {k: p.detach() - before[k] for k, p in params.items()}})
    DC.check_steps(got, ref, what="hip")


# ------------------------------------------------------------------------------------------- 6: the entry point
def test_pretrain_entry_point_writes_loadable_encoders(tmp_path):
    """pretrain_DAMSM.py --synthetic 2 (nef 32, B 4, 12 words, one epoch of two iterations, the real trunk): writes
    text_encoder0.pth / image_encoder0.pth with the modules' state_dict keys and shapes, leaves the trunk's parameters bitwise
    alone, condGANTrainer.build_models loads the pair through TRAIN.NET_E, evaluate returns four finite numbers."""
    from mogan_amd.attngan import model, pretrain_DAMSM as PD
    from mogan_amd.attngan.datasets import SyntheticTextDataset
    from mogan_amd.attngan.miscc.config import cfg
    from mogan_amd.attngan.trainer import condGANTrainer
    yml = tmp_path / "damsm.yml"
    yml.write_text("CONFIG_NAME: 'damsm'\nDATASET_NAME: 'coco'\nWORKERS: 0\nTREE: {BRANCH_NUM: 1, BASE_SIZE: 64}\n"
                   "GAN: {DF_DIM: 8, GF_DIM: 8, Z_DIM: 100, R_NUM: 1}\n"
                   "TEXT: {EMBEDDING_DIM: 32, CAPTIONS_PER_IMAGE: 5, WORDS_NUM: 12}\n"
                   "TRAIN: {FLAG: True, BATCH_SIZE: 4, MAX_EPOCH: 1, SNAPSHOT_INTERVAL: 1, NET_E: '', ENCODER_LR: 0.002}\n")
    out = tmp_path / "out"
    # the encoders as main() will construct them (same seed, same order): what the trunk holds before any training
    PD.cfg_from_file(str(yml))
    torch.manual_seed(7)
    model.RNN_ENCODER(SyntheticTextDataset(length=4).n_words, nhidden=32)
    init = model.CNN_ENCODER(32).state_dict()
    trunk0 = {k: v.clone() for k, v in init.items() if k.split(".")[0] not in model.CNN_ENCODER.HEADS}
    eng = PD.main(["--cfg", str(yml), "--synthetic", "2", "--manualSeed", "7", "--output_dir", str(out)])
    assert float(eng.opt.state[0]) == 2.0                          # two iterations
    tp, ip = [os.path.join(str(out), "Model", "%s_encoder0.pth" % k) for k in ("text", "image")]
    tsd, isd = torch.load(tp, map_location="cpu"), torch.load(ip, map_location="cpu")
    for sd, net in ((tsd, eng.text_encoder), (isd, eng.image_encoder)):
        assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
        assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
    # same seed, same construction order as main(): the trunk is what the constructor made of it, bit for bit
    for k, v in trunk0.items():
        assert torch.equal(isd[k], v), k
    assert not torch.equal(isd["emb_features.weight"], init["emb_features.weight"])        # ... and the heads moved
    cfg.TRAIN.NET_E = tp
    try:
        ds = SyntheticTextDataset(length=4)
        algo = condGANTrainer(str(out), None, ds.n_words, ds.ixtoword, resume=False)
        text, image = algo.build_models()[:2]
    finally:
        cfg.TRAIN.NET_E = ''
    for k, v in text.state_dict().items():
        assert torch.equal(v.cpu(), tsd[k]), k
    assert torch.equal(image.state_dict()["emb_cnn_code.weight"].cpu(), isd["emb_cnn_code.weight"])
    dl = torch.utils.data.DataLoader(SyntheticTextDataset(length=4, seed=3), batch_size=4, drop_last=True)
    val = eng.evaluate(dl)
    assert len(val) == 4 and all(np.isfinite(v) for v in val), val


# ------------------------------------------------------------------------------------------- 7: trainable heads
def test_cnn_encoder_keeps_the_frozen_trunk_under_trainable_heads(monkeypatch):
    """CNN_ENCODER in eval mode with a frozen trunk and heads that require a gradient: the fast frozen trunk runs (PanelTrunk.
    forward is called), the outputs equal the all-frozen module's bitwise, and the head weight gradients match F.conv2d /
    F.linear autograd in fp64 on the HIP trunk's own outputs to rel-L2 2e-6 (the project's figure for these GEMMs)."""
    from mogan_amd.attngan import inception, model
    from mogan_amd.attngan.miscc.config import cfg
    cfg.TRAIN.FLAG = True
    torch.manual_seed(3)
    enc = model.CNN_ENCODER(32).to(DEV).eval()
    for p in enc.parameters():
        p.requires_grad = False
    x = (torch.rand(2, 3, 64, 64) * 2 - 1).to(DEV)
    with torch.no_grad():
        f0, c0 = enc(x)
    for name in enc.HEADS:
        for p in getattr(enc, name).parameters():
            p.requires_grad = True
    runs, fwd = [], inception.PanelTrunk.forward

    def recorded(self, x299):
        out = fwd(self, x299)
        runs.append((out[1].detach().clone(), out[2].detach().clone()))
        return out
    monkeypatch.setattr(inception.PanelTrunk, "forward", recorded)
    assert inception.FAST_TRUNK and enc._frozen()
    f1, c1 = enc(x)
    assert len(runs) == 1
    assert torch.equal(_bits(f1), _bits(f0)) and torch.equal(_bits(c1), _bits(c0))
    gf, gc = torch.randn(2, 32, 17, 17), torch.randn(2, 32)
    ((f1 * gf.to(DEV)).sum() + (c1 * gc.to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    feat, last = (t.cpu().double() for t in runs[0])
    w = {k: p.detach().cpu().double().requires_grad_(True) for k, p in enc.named_parameters() if k.split(".")[0] in enc.HEADS}
    fr = F.conv2d(feat, w["emb_features.weight"])
    cr = F.linear(F.avg_pool2d(last, 8).flatten(1), w["emb_cnn_code.weight"], w["emb_cnn_code.bias"])
    ((fr * gf.double()).sum() + (cr * gc.double()).sum()).backward()
    for k, p in enc.named_parameters():
        if k in w:
            print("%s rel-L2 %.2e" % (k, rel_l2(p.grad, w[k].grad)))
            assert rel_l2(p.grad, w[k].grad) <= 2e-6, (k, rel_l2(p.grad, w[k].grad))
        else:
            assert p.grad is None
    enc.train()
    assert not enc._frozen()                                          # training mode: the module-by-module path, as before
