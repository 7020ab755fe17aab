"""The GRU text encoder (cfg.RNN_TYPE = 'GRU'), the part that needs no GPU: the CPU restatement of the pre-training step
(tests/damsm_gru_cases.py) in fp32 against itself in fp64 under the assertions the HIP step is held to
(tests/test_gru_encoder_gpu.py), and the host-side argument checks of the two GRU paths."""
import torch

import damsm_gru_cases as GC
from helpers import load_pkg

load_pkg()
from mogan_amd.hip import ops  # noqa: E402


def test_gru_reference_stays_inside_the_step_assertions():
    """torch fp32 against torch fp64 on the GRU step's own inputs: the losses, the norm, the clipped gradients, the update and
    the 95 % share of judged elements all hold for the reference itself, whatever the kernels do."""
    inp = GC.make_inputs()
    GC.check_steps(GC.reference_steps(inp, torch.float32), GC.reference_steps(inp, torch.float64), what="torch fp32 GRU")


def test_gru_encoder_argument_checks_decline_what_the_kernels_do_not_cover():
    """hip/ops._rnn_encoder_args, the one helper of the eval and the training path, with an nn.GRU and its one state: the covered
    module is accepted; an nn.LSTM handed that state, an nn.GRU handed (h, c), an nn.RNN, H != 128, a unidirectional module, a
    half-precision or off-device tensor, a mis-shaped h0, Tmax > 32, E % 4 != 0 and len(lens) != B give None (the caller keeps
    the stock modules) before any pointer is taken."""
    G = lambda *a, **k: torch.nn.GRU(*a, batch_first=True, **k)
    rnn = G(300, 128, 1, bidirectional=True)
    cap = torch.ones(3, 12, dtype=torch.int64)
    lens = [12, 5, 1]
    emb = torch.zeros(50, 300)
    h = torch.zeros(2, 3, 128)
    ok = ops._rnn_encoder_args(cap, lens, emb, rnn, (h,))
    assert ok is not None and ok[:6] == (3, 12, 50, 300, 128, 12) and len(ok[7]) == 8
    assert ops._rnn_encoder_args(cap, lens, emb, rnn, (None,)) is not None
    assert ops._rnn_encoder_args(cap, [12, 0, 0], emb, rnn, (None,)) is not None           # empty captions are covered
    bad = [dict(rnn=torch.nn.LSTM(300, 128, 1, batch_first=True, bidirectional=True)), dict(rnn=G(300, 64, 1, bidirectional=True)),
           dict(rnn=torch.nn.RNN(300, 128, 1, batch_first=True, bidirectional=True)),
           dict(rnn=G(300, 128, 1)), dict(rnn=G(300, 128, 2, bidirectional=True)), dict(rnn=G(300, 128, 1, bidirectional=True).half()),
           dict(rnn=G(300, 128, 1, bidirectional=True).to("meta")), dict(emb=emb.half()), dict(emb=emb.to("meta")),
           dict(emb=emb.t()), dict(h0=h.half()), dict(h0=h.to("meta")), dict(h0=torch.zeros(2, 4, 128)),
           dict(h0=torch.zeros(1, 3, 128)), dict(cap=torch.ones(3, 40, dtype=torch.int64), lens=[33, 5, 1]),
           dict(emb=torch.zeros(50, 302), rnn=G(302, 128, 1, bidirectional=True)), dict(emb=torch.zeros(50, 304)),
           dict(lens=[12, 5]), dict(lens=[13, 5, 1]), dict(lens=[12, 5, -1]), dict(cap=cap.int())]
    for kw in bad:
        a = dict(cap=cap, lens=lens, emb=emb, rnn=rnn, h0=h)
        a.update(kw)
        assert ops._rnn_encoder_args(a["cap"], a["lens"], a["emb"], a["rnn"], (a["h0"],)) is None, list(kw)
    assert ops._rnn_encoder_args(cap, lens, emb, rnn, (h, h)) is None                          # an nn.GRU handed (h, c)
    for fn in (ops.rnn_encoder_forward, ops.rnn_encoder_train):            # both public functions decline through it
        assert fn(cap, lens, emb.half(), rnn, (h,)) is None
        assert fn(cap, lens, emb, torch.nn.LSTM(300, 128, 1, batch_first=True, bidirectional=True), (h,)) is None
