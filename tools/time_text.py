"""The text encoder (RNN_ENCODER: Embedding + bi-LSTM or, with --rnn GRU, bi-GRU over packed captions, eval, no grad) alone: device
time and host time (the enqueue) per call, from 50 calls back to back between two hip events (median and minimum of --iters such
samples after --warmup calls).
python tools/time_text.py [--rnn {LSTM,GRU}]"""
import argparse, os, statistics, sys, time, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mogan_loader; mogan_loader.load()
from mogan_amd.attngan import model
from mogan_amd.attngan.miscc.config import cfg, set_coco_train_defaults
ap = argparse.ArgumentParser()
ap.add_argument("--rnn", choices=("LSTM", "GRU"), default="LSTM", help="cfg.RNN_TYPE of the text encoder")
ap.add_argument("--iters", type=int, default=11)
ap.add_argument("--warmup", type=int, default=5)
args = ap.parse_args()
set_coco_train_defaults()
cfg.RNN_TYPE = args.rnn
dev = torch.device("cuda")
torch.manual_seed(0)
enc = model.RNN_ENCODER(27297, nhidden=cfg.TEXT.EMBEDDING_DIM).to(dev).eval()
B, T = 16, cfg.TEXT.WORDS_NUM
g = torch.Generator().manual_seed(B)
lens = sorted([T] + [int(v) for v in torch.randint(5, T + 1, (B - 1,), generator=g)], reverse=True)
cap = torch.zeros(B, T, dtype=torch.int64)
for i, n in enumerate(lens):
    cap[i, :n] = torch.randint(1, 27297, (n,), generator=g)
cap = cap.to(dev)
lens_t = torch.tensor(lens)
def run():
    with torch.no_grad():
        return enc(cap, lens_t, enc.init_hidden(B))
for _ in range(args.warmup): run()
torch.cuda.synchronize()
dev_us, host_us = [], []
for _ in range(args.iters):                                      # one sample = 50 calls back to back between two events
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    t0 = time.perf_counter(); e0.record()
    for _ in range(50): run()
    e1.record(); t1 = time.perf_counter(); torch.cuda.synchronize()
    dev_us.append(e0.elapsed_time(e1) * 20); host_us.append((t1 - t0) * 2e4)
print("text encoder %s B=%d T=%d: device %.1f us per call (min %.1f), host %.1f us per call"
      % (args.rnn, B, T, statistics.median(dev_us), min(dev_us), statistics.median(host_us)))
