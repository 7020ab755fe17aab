"""DAMSM pre-training, the part that needs no GPU: the CPU restatement of the step (tests/damsm_pretrain_cases.py) in fp32 against
itself in fp64 under the assertions the HIP step is held to (tests/test_damsm_pretrain_gpu.py), and the host-side argument
checks of the text-encoder paths."""
import torch

import damsm_pretrain_cases as DC
from helpers import load_pkg

load_pkg()
from mogan_amd.hip import ops  # noqa: E402


def test_reference_stays_inside_the_step_assertions():
    """torch fp32 against torch fp64 on the test's own inputs: the losses, the norm, the clipped gradients, the update and the
    95 % share of judged elements all hold for the reference itself.  A later change of the seeds that moves the reference
    outside the caps fails here, whatever the kernels do."""
    inp = DC.make_inputs()
    DC.check_steps(DC.reference_steps(inp, torch.float32), DC.reference_steps(inp, torch.float64), what="torch fp32")


def test_text_encoder_argument_checks_decline_what_the_kernels_do_not_cover():
    """hip/ops._rnn_encoder_args, the one helper of the eval and the training path, with an nn.LSTM and its two states: a module
    (an nn.GRU handed (h, c), an nn.RNN, an nn.LSTM handed one state) or tensors outside the kernels' contract give None (the
    caller keeps the stock modules) before any pointer is taken -- the embedding table and the initial states included (dtype,
    device, shape)."""
    rnn = torch.nn.LSTM(300, 128, 1, batch_first=True, bidirectional=True)
    cap = torch.ones(3, 12, dtype=torch.int64)
    lens = [12, 5, 1]
    emb = torch.zeros(50, 300)
    h = torch.zeros(2, 3, 128)
    ok = ops._rnn_encoder_args(cap, lens, emb, rnn, (h, h))
    assert ok is not None and ok[:6] == (3, 12, 50, 300, 128, 12)
    assert ops._rnn_encoder_args(cap, lens, emb, rnn, (None, None)) is not None
    bad = [dict(emb=emb.double()), dict(emb=emb.to("meta")), dict(emb=torch.zeros(50, 304)), dict(emb=emb.t()),
           dict(h0=h.double()), dict(c0=torch.zeros(2, 4, 128)), dict(h0=h.to("meta")), dict(cap=cap.int()),
           dict(lens=[12, 5]), dict(lens=[13, 5, 1]), dict(rnn=torch.nn.LSTM(300, 64, 1, batch_first=True, bidirectional=True)),
           dict(rnn=torch.nn.GRU(300, 128, 1, batch_first=True, bidirectional=True)),
           dict(rnn=torch.nn.RNN(300, 128, 1, batch_first=True, bidirectional=True)),
           dict(rnn=torch.nn.LSTM(300, 128, 1, batch_first=True))]
    for kw in bad:
        a = dict(cap=cap, lens=lens, emb=emb, rnn=rnn, h0=h, c0=h)
        a.update(kw)
        assert ops._rnn_encoder_args(a["cap"], a["lens"], a["emb"], a["rnn"], (a["h0"], a["c0"])) is None, list(kw)
    assert ops._rnn_encoder_args(cap, lens, emb, rnn, (h,)) is None                             # an nn.LSTM handed a GRU-shaped state
    for fn in (ops.rnn_encoder_forward, ops.rnn_encoder_train):            # both entry points decline through it
        assert fn(cap, lens, emb.double(), rnn, (h, h)) is None
