"""Inputs, CPU restatement and assertions of the DAMSM pre-training step (a plain helper module, not a conftest), shared by
tests/test_damsm_pretrain_gpu.py (the HIP step against the restatement in fp64) and tests/test_damsm_pretrain_cpu.py (the
restatement in fp32 against itself in fp64: the reference must sit inside the very assertions the HIP step is held to).

The restatement is the arithmetic the reference's modules define, on stock torch ops: nn.Embedding -> dropout mask -> packed
bidirectional nn.LSTM (model.py:120-204), F.conv2d / F.linear heads (model.py:207-313), words_loss / sent_loss
(oracle/attngan_oracle.py), clip_grad_norm_ over the text encoder's parameters, torch.optim.Adam(betas=(0.5, 0.999))."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from oracle import attngan_oracle as O

B, T, LENS, V, E, NEF, H = 6, 18, [15, 11, 9, 9, 6, 1], 50, 300, 256, 128
LR, CLIP, STEPS = 2e-4, 0.25, 2
SEED = 23
N_PARAMS = 1176472
TEXT_KEYS = ["encoder.weight"] + ["rnn.%s_l0%s" % (k, r) for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")
                                  for r in ("", "_reverse")]
HEAD_KEYS = ["emb_features.weight", "emb_cnn_code.weight", "emb_cnn_code.bias"]
G_FLOOR = 1e-6          # |g_ref| below this: Adam's first steps are +-lr there, decided by noise -- not judged
LOSS_RTOL = NORM_RTOL = GRAD_REL_L2 = 2e-5
DELTA_TOL = 1e-2        # in units of lr
MIN_SHARE = 0.95


def make_inputs(seed=SEED):
    """everything the two steps read, float32 on the CPU, from one fixed seed"""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g) * 0.2 - 0.1
    inp = {"feat768": 0.5 * torch.randn(B, 768, 17, 17, generator=g).abs(),
           "code2048": 0.5 * torch.randn(B, 2048, generator=g).abs()}
    cap = torch.zeros(B, T, dtype=torch.int64)
    for i, n in enumerate(LENS):
        cap[i, :n] = torch.randint(1, V, (n,), generator=g)
    inp["captions"], inp["lens"] = cap, list(LENS)
    inp["masks"] = [(torch.rand(B, T, E, generator=g) >= 0.5).to(torch.uint8) for _ in range(STEPS)]
    k = 1.0 / np.sqrt(H)                                            # nn.LSTM's own initialisation range
    w = {"encoder.weight": u(V, E)}
    for r in ("", "_reverse"):
        w["rnn.weight_ih_l0" + r] = (torch.rand(4 * H, E, generator=g) * 2 - 1) * k
        w["rnn.weight_hh_l0" + r] = (torch.rand(4 * H, H, generator=g) * 2 - 1) * k
        w["rnn.bias_ih_l0" + r] = (torch.rand(4 * H, generator=g) * 2 - 1) * k
        w["rnn.bias_hh_l0" + r] = (torch.rand(4 * H, generator=g) * 2 - 1) * k
    w["emb_features.weight"], w["emb_cnn_code.weight"], w["emb_cnn_code.bias"] = u(NEF, 768, 1, 1), u(NEF, 2048), u(NEF)
    inp["weights"] = w
    assert sum(v.numel() for v in w.values()) == N_PARAMS
    return inp


def reference_steps(inp, dtype):
    """STEPS pre-training steps on the CPU in `dtype`.  Per step: {"losses": 4 floats, "norm": float, "grad": {key: clipped
    gradient}, "delta": {key: p_after - p_before}}."""
    w = {k: v.detach().clone().to(dtype) for k, v in inp["weights"].items()}
    emb = nn.Embedding(V, E).to(dtype)
    rnn = nn.LSTM(E, H, 1, batch_first=True, bidirectional=True).to(dtype)
    emb.load_state_dict({"weight": w["encoder.weight"]})
    rnn.load_state_dict({k[4:]: v for k, v in w.items() if k.startswith("rnn.")})
    heads = {k: w[k].requires_grad_(True) for k in HEAD_KEYS}
    params = dict([("encoder.weight", emb.weight)] + [("rnn." + k, p) for k, p in rnn.named_parameters()] + list(heads.items()))
    assert sorted(params) == sorted(TEXT_KEYS + HEAD_KEYS)
    opt = torch.optim.Adam(list(params.values()), lr=LR, betas=(0.5, 0.999))
    ocfg = O.Cfg(words_num=T, gamma1=4.0, gamma2=5.0, gamma3=10.0)
    feat768, code2048 = inp["feat768"].to(dtype), inp["code2048"].to(dtype)
    out = []
    for s in range(STEPS):
        opt.zero_grad()
        feats = F.conv2d(feat768, heads["emb_features.weight"])
        code = F.linear(code2048, heads["emb_cnn_code.weight"], heads["emb_cnn_code.bias"])
        x = emb(inp["captions"]) * (inp["masks"][s].to(dtype) * 2.0)                 # keep mask, scale 1 / (1 - 0.5)
        seq, (hn, _) = rnn(pack_padded_sequence(x, inp["lens"], batch_first=True))
        words = pad_packed_sequence(seq, batch_first=True)[0].transpose(1, 2)
        sent = hn.transpose(0, 1).reshape(B, 2 * H)
        w0, w1, _ = O.words_loss(feats, words, inp["lens"], ocfg)
        s0, s1 = O.sent_loss(code, sent, ocfg)
        (w0 + w1 + s0 + s1).backward()
        norm = torch.nn.utils.clip_grad_norm_([params[k] for k in TEXT_KEYS], CLIP)
        before = {k: p.detach().clone() for k, p in params.items()}
        grad = {k: p.grad.detach().clone() for k, p in params.items()}
        opt.step()
        out.append({"losses": [float(v.detach()) for v in (w0, w1, s0, s1)], "norm": float(norm), "grad": grad,
                    "delta": {k: p.detach() - before[k] for k, p in params.items()}})
    return out


def check_steps(got, ref, what=""):
    """The assertions of the pre-training step, `got` against the fp64 `ref` (both as reference_steps returns them); prints
    every figure before it asserts.  Per step: the four losses and the pre-clip norm to rtol 2e-5, every clipped gradient to
    rel-L2 2e-5, and the update dp element by element:
      * where the reference's clipped gradient is exactly 0 (absent tokens, dropped elements), dp is exactly 0,
      * where |g_ref| >= 1e-6, |dp - dp_ref| <= 1e-2 * lr,
      * the elements below that threshold are left out (Adam's first steps are +-lr there, decided by noise).
    One amendment at the second step: an element whose gradient is exactly 0 NOW but was not at the first step still moves by
    Adam's first moment -- in the reference too (1627 such elements on these inputs, in fp64) -- so "exactly 0" is asked where
    the gradient has been exactly 0 at EVERY step so far; the others are held to |dp - dp_ref| <= 1e-2 * lr like the judged
    ones if their earlier gradients were >= 1e-6, and left out otherwise.  Judged + exact-zero elements must be >= 95 % of all."""
    dd = lambda t: t.detach().cpu().double()
    seen_zero = seen_ok = None
    for s, (a, r) in enumerate(zip(got, ref)):
        for k, x, y in zip(("w_loss0", "w_loss1", "s_loss0", "s_loss1"), a["losses"], r["losses"]):
            print("%s step %d %s: %.8f vs %.8f (rel %.2e)" % (what, s, k, x, y, abs(x - y) / abs(y)))
        print("%s step %d norm: %.8f vs %.8f (rel %.2e)" % (what, s, a["norm"], r["norm"], abs(a["norm"] - r["norm"]) / r["norm"]))
        rels = {k: float((dd(a["grad"][k]) - dd(r["grad"][k])).norm() / dd(r["grad"][k]).norm()) for k in r["grad"]}
        print("%s step %d clipped-gradient rel-L2: %s" % (what, s, ", ".join("%s %.2e" % kv for kv in rels.items())))
        zero = {k: dd(v) == 0 for k, v in r["grad"].items()}
        ok = {k: (dd(v) == 0) | (dd(v).abs() >= G_FLOOR) for k, v in r["grad"].items()}
        seen_zero = zero if seen_zero is None else {k: seen_zero[k] & zero[k] for k in zero}
        seen_ok = ok if seen_ok is None else {k: seen_ok[k] & ok[k] for k in ok}
        n_all = n_judged = n_zero = bad_zero = bad = 0
        worst = 0.0
        for k in r["grad"]:
            da, dr = dd(a["delta"][k]), dd(r["delta"][k])
            z = seen_zero[k]
            j = ((dd(r["grad"][k]).abs() >= G_FLOOR) | (zero[k] & seen_ok[k])) & ~z
            n_all += z.numel(); n_zero += int(z.sum()); n_judged += int(j.sum())
            bad_zero += int((da[z] != 0).sum())
            err = (da - dr).abs()[j]
            if err.numel():
                worst = max(worst, float(err.max()))
                bad += int((err > DELTA_TOL * LR).sum())
        share = (n_zero + n_judged) / n_all
        print("%s step %d update: %d elements, %d exact-zero (%d moved), %d judged (worst |dp - dp_ref| %.2e lr, %d over), share "
              "%.2f %%" % (what, s, n_all, n_zero, bad_zero, n_judged, worst / LR, bad, 100 * share))
        for x, y in zip(a["losses"], r["losses"]):
            assert abs(x - y) <= LOSS_RTOL * abs(y), (s, a["losses"], r["losses"])
        assert abs(a["norm"] - r["norm"]) <= NORM_RTOL * r["norm"], (s, a["norm"], r["norm"])
        assert all(v <= GRAD_REL_L2 for v in rels.values()), (s, rels)
        assert n_all == N_PARAMS
        assert bad_zero == 0 and bad == 0, (s, bad_zero, bad, worst / LR)
        assert share >= MIN_SHARE, (s, share)
