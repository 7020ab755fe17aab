"""The text encoder under training (RNN_ENCODER forward + backward, embedding dropout on) and the whole DAMSM pre-training step:
the fused HIP path against the stock nn.Embedding / nn.LSTM (or, with --rnn GRU, nn.GRU) path (RNN_ENCODER.FUSED = False, MIOpen)
in the same process.

Per shape and path: device time per call from hip events around ONE call (median of --iters after --warmup, the two paths
alternating), host time per call (the enqueue, no synchronise inside), and -- in a pass of its own under torch.profiler -- the
number of device kernels and their summed duration.  Then DAMSMEngine.step at B = 48 through the real trunk, both ways.
python tools/time_text_train.py [--rnn {LSTM,GRU}] [--out profiles/damsm_pretrain_timing.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mogan_loader  # noqa: E402
mogan_loader.load()
from mogan_amd.attngan import model, pretrain_DAMSM as PD, synthetic  # noqa: E402
from mogan_amd.attngan.miscc.config import cfg, set_coco_train_defaults  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--warmup", type=int, default=8)
ap.add_argument("--out", default="")
ap.add_argument("--rnn", choices=("LSTM", "GRU"), default="LSTM", help="cfg.RNN_TYPE of the text encoder")
args = ap.parse_args()
assert torch.cuda.is_available(), "timing needs the GPU"
set_coco_train_defaults()
cfg.TRAIN.FLAG = True
cfg.RNN_TYPE = args.rnn
dev = torch.device("cuda")
V = synthetic.VOCAB


def captions(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    lens = sorted([T] + [int(v) for v in torch.randint(5, T + 1, (B - 1,), generator=g)], reverse=True)
    cap = torch.zeros(B, T, dtype=torch.int64)
    for i, n in enumerate(lens):
        cap[i, :n] = torch.randint(1, V, (n,), generator=g)
    return cap.to(dev), torch.tensor(lens)


def timed(fn):
    """(device ms, host ms) of one call"""
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), (t1 - t0) * 1e3


def kernels(fn):
    """(number of device kernels, their summed duration in ms) of one call, or None where the profiler gives no device events"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        evs = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
        if not evs:
            return None
        dur = lambda e: getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0)
        return len(evs), sum(dur(e) for e in evs) / 1e3
    except Exception as exc:                                     # the measurement is then reported as missing, not guessed
        print("profiler pass failed: %r" % (exc,))
        return None


def compare(name, fn, result):
    """fn(fused: bool) runs one call; the two paths alternate inside the timed loop"""
    def run(fused):
        model.RNN_ENCODER.FUSED = fused
        try:
            fn()
        finally:
            model.RNN_ENCODER.FUSED = True
    for _ in range(args.warmup):
        run(True); run(False)
    t = {True: [], False: []}
    for _ in range(args.iters):
        for fused in (True, False):
            t[fused].append(timed(lambda: run(fused)))
    for fused in (True, False):
        k = kernels(lambda: run(fused))
        r = {"device_ms_median": statistics.median(x[0] for x in t[fused]), "device_ms_min": min(x[0] for x in t[fused]),
             "host_ms_median": statistics.median(x[1] for x in t[fused]), "iters": args.iters, "warmup": args.warmup,
             "kernels": k[0] if k else None, "kernel_ms": k[1] if k else None}
        result["%s %s" % (name, "fused" if fused else "stock")] = r
        print("%-28s %-5s device %.3f ms (min %.3f)  host %.3f ms  kernels %s  kernel time %s ms"
              % (name, "fused" if fused else "stock", r["device_ms_median"], r["device_ms_min"], r["host_ms_median"],
                 r["kernels"], "%.3f" % r["kernel_ms"] if k else "not measured"))


result = {}
for B, T in ((16, 12), (48, 12)):
    torch.manual_seed(0)
    enc = model.RNN_ENCODER(V, nhidden=cfg.TEXT.EMBEDDING_DIM).to(dev).train()
    cap, lens = captions(B, T, B)
    gw, gs = torch.randn(B, 256, int(lens.max()), device=dev), torch.randn(B, 256, device=dev)

    def fwd_bwd():
        for p in enc.parameters():
            p.grad = None
        w, s = enc(cap, lens, enc.init_hidden(B))
        torch.autograd.backward([w, s], [gw, gs])
    compare("RNN_ENCODER fwd+bwd B=%d T=%d" % (B, T), fwd_bwd, result)

B = 48
torch.manual_seed(1)
text = model.RNN_ENCODER(V, nhidden=cfg.TEXT.EMBEDDING_DIM).to(dev)
image = model.CNN_ENCODER(cfg.TEXT.EMBEDDING_DIM).to(dev)
eng = PD.DAMSMEngine(text, image)
cap, lens = captions(B, cfg.TEXT.WORDS_NUM, 7)
imgs = torch.rand(B, 3, 256, 256, device=dev) * 2 - 1
import numpy as np  # noqa: E402
batch = (imgs, cap, lens, np.arange(B))
compare("DAMSMEngine.step B=%d" % B, lambda: eng.step(batch), result)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print("wrote", args.out)
