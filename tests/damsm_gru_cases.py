"""The DAMSM pre-training step with cfg.RNN_TYPE = 'GRU': inputs, CPU restatement and assertions (a plain helper module, not a
conftest), shared by tests/test_gru_encoder_gpu.py (the HIP step against the restatement in fp64) and
tests/test_gru_encoder_cpu.py (the restatement in fp32 against itself in fp64).

Everything but the recurrent layer is tests/damsm_pretrain_cases.py's: the same features, captions, lengths, keep masks, head
and embedding weights (its make_inputs), LR, CLIP, STEPS and -- through check_steps below -- its very assertions.  The GRU's
weights are drawn in +-1 / sqrt(H), nn.GRU's own initialisation range, from a seed of their own."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

import damsm_pretrain_cases as DC
from damsm_pretrain_cases import B, CLIP, E, H, HEAD_KEYS, LR, NEF, STEPS, T, TEXT_KEYS, V  # noqa: F401
from oracle import attngan_oracle as O

GRU_SEED = 24
N_PARAMS = 1066392      # 50 * 300 + 2 * (384 * 300 + 384 * 128 + 2 * 384) + 256 * 768 + 256 * 2048 + 256


def make_inputs():
    """damsm_pretrain_cases.make_inputs() with the LSTM's eight tensors replaced by a GRU's (3H rows, gate order r, z, n)"""
    inp = DC.make_inputs()
    g = torch.Generator().manual_seed(GRU_SEED)
    k = 1.0 / np.sqrt(H)
    w = {key: v for key, v in inp["weights"].items() if not key.startswith("rnn.")}
    for r in ("", "_reverse"):
        w["rnn.weight_ih_l0" + r] = (torch.rand(3 * H, E, generator=g) * 2 - 1) * k
        w["rnn.weight_hh_l0" + r] = (torch.rand(3 * H, H, generator=g) * 2 - 1) * k
        w["rnn.bias_ih_l0" + r] = (torch.rand(3 * H, generator=g) * 2 - 1) * k
        w["rnn.bias_hh_l0" + r] = (torch.rand(3 * H, generator=g) * 2 - 1) * k
    inp["weights"] = w
    assert sum(v.numel() for v in w.values()) == N_PARAMS and sorted(w) == sorted(TEXT_KEYS + HEAD_KEYS)
    return inp


def reference_steps(inp, dtype):
    """damsm_pretrain_cases.reference_steps with nn.GRU as the recurrent layer: STEPS pre-training steps on the CPU in `dtype`,
    the same dictionary per step."""
    w = {k: v.detach().clone().to(dtype) for k, v in inp["weights"].items()}
    emb = nn.Embedding(V, E).to(dtype)
    rnn = nn.GRU(E, H, 1, batch_first=True, bidirectional=True).to(dtype)
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
        seq, hn = rnn(pack_padded_sequence(x, inp["lens"], batch_first=True))
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
    """damsm_pretrain_cases.check_steps itself -- every bound and the 95 % floor as they stand there -- with the one figure that
    belongs to the model, the number of elements it counts, set to the GRU configuration's for the duration of the call."""
    was = DC.N_PARAMS
    DC.N_PARAMS = N_PARAMS
    try:
        DC.check_steps(got, ref, what=what)
    finally:
        DC.N_PARAMS = was
