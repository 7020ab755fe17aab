"""Radial power spectrum (attngan/spectrum.py; csrc/mogan_spectrum.hip) at the real workload -- RadialSpectrum.add for 16 pairs of
3 x 256 x 256 images, one call per side -- against the same stages formed by stock torch ops on the device: the luminance as a
weighted sum of the channels in fp64, the window, torch.fft.rfft2 in fp64, |F|^2 times the half plane's multiplicities, index_add_ by
bin (which adds with atomics: its sums are not the same bits from call to call, and it writes the 2-D power plane to memory).  Hip
events around every call, 8 warm-up calls and the median of 30 per path, the two paths alternating call by call in one process.  A
record, not a gate: the project's kernel is the path whichever way it comes out -- what it is there for is the fp64 path with the
same bits for an image in any batch.  The torch formulation lives only here.
Also measured: the share of one spectrum() batch (coco_train widths, 16 captions) that the scoring takes next to the generator's
forward.
python tools/time_spectrum.py [--out profiles/spectrum_timing.json]"""
import argparse, json, os, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mogan_loader; mogan_loader.load()
from mogan_amd.attngan import spectrum as SP
ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=16, help="image pairs per add()")
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--window", default="hann", choices=SP.WINDOWS)
ap.add_argument("--warmup", type=int, default=8)
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--out", default="")
args = ap.parse_args()
assert torch.cuda.is_available(), "a timing needs the GPU"
dev = torch.device("cuda")
B, C, S = args.images, 3, args.size
g = torch.Generator(device=dev).manual_seed(5)
real = torch.rand((B, C, S, S), device=dev, generator=g) * 2 - 1
fake = (0.5 * real + 0.5 * (torch.rand((B, C, S, S), device=dev, generator=g) * 2 - 1)).contiguous()
acc = SP.RadialSpectrum(S, C, B, window=args.window, device=dev)
table, count = SP.radial_bins(S)
n_bins = len(count)
w64 = acc.weight.double().view(1, C, 1, 1)
win64 = None if acc.win is None else (acc.win.double()[:, None] * acc.win.double()[None, :])
mult = torch.full((S // 2 + 1,), 2.0, dtype=torch.float64, device=dev)
mult[0] = mult[-1] = 1.0
flat_bins = acc.table.long().view(-1)


def timed(fn):
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record(); out = fn(); e1.record()
    return out, (e0, e1)


def kernel_add():
    acc.n = 0
    acc.add(real, fake)
    return torch.stack([acc.sums["real"], acc.sums["fake"]])


def torch_side(x):
    y = (x.double() * w64).sum(dim=1)
    if win64 is not None:
        y = y * win64
    F = torch.fft.rfft2(y)
    p = (F.real * F.real + F.imag * F.imag) * mult
    out = torch.zeros((n_bins, x.shape[0]), dtype=torch.float64, device=dev)
    return out.index_add_(0, flat_bins, p.view(x.shape[0], -1).t()).t()


def torch_add():
    return torch.stack([torch_side(real), torch_side(fake)])


PATHS = {"kernel": kernel_add, "torch": torch_add}
events = {name: [] for name in PATHS}
sums = {}
for r in range(args.warmup + args.calls):
    for name, fn in PATHS.items():
        out, ev = timed(fn)
        if r >= args.warmup:
            events[name].append(ev)
        sums[name] = out
torch.cuda.synchronize()
us = {name: [e0.elapsed_time(e1) * 1e3 for e0, e1 in events[name]] for name in PATHS}
total = sums["kernel"].sum(dim=2, keepdim=True)
result = {"method": "hip events around every call; %d warm-up calls and the median of %d per path, the two paths alternating call by "
                    "call in one process; microseconds" % (args.warmup, args.calls),
          "device": torch.cuda.get_device_name(0),
          "workload": {"image_pairs": B, "channels": C, "size": S, "window": args.window, "bins": n_bins,
                       "calls_per_add": 2},
          "kernel_us": round(statistics.median(us["kernel"]), 1), "kernel_min_us": round(min(us["kernel"]), 1),
          "kernel_max_us": round(max(us["kernel"]), 1),
          "torch_us": round(statistics.median(us["torch"]), 1), "torch_min_us": round(min(us["torch"]), 1),
          "torch_max_us": round(max(us["torch"]), 1),
          "largest_difference_of_a_bin_between_the_paths_relative_to_the_images_total_power":
              float(((sums["kernel"] - sums["torch"]).abs() / total).max())}
result["torch_over_kernel"] = round(result["torch_us"] / result["kernel_us"], 3)
# what the algorithm has to read: both sides' images, once
need = 2 * B * C * S * S * 4
result["bytes_the_images_hold"] = need
result["kernel_TB_per_s_of_those_bytes"] = round(need / result["kernel_us"] / 1e6, 3)
print(json.dumps(result), flush=True)

# ------------------------------------------------------------------------------------------------ the share of one spectrum() batch
from mogan_amd.attngan import model, synthetic
from mogan_amd.attngan.miscc.config import cfg, set_coco_train_defaults
from mogan_amd.attngan.miscc.utils import weights_init
set_coco_train_defaults()
NB = 16
torch.manual_seed(3)
netG = model.G_NET()
netG.apply(weights_init)
netG = netG.to(dev).eval()
bt = synthetic.to_device(synthetic.make_batch(NB, words_num=cfg.TEXT.WORDS_NUM, nef=cfg.TEXT.EMBEDDING_DIM, seed=3), dev)
batch_acc = SP.RadialSpectrum(256, 3, NB, window=args.window, device=dev)


def forward():
    with torch.no_grad():
        return netG(bt["z"], bt["sent_emb"], bt["words_embs"], bt["mask"], bt["tmi"], bt["label_one_hot"], eps=bt["eps"])[0][-1]


gen = forward().float().contiguous()
data = bt["imgs"][-1].contiguous()


def scoring():
    batch_acc.n = 0
    batch_acc.add(data, gen)


share = {"forward": [], "scoring": []}
for r in range(args.warmup + args.calls):
    for name, fn in (("forward", forward), ("scoring", scoring)):
        _, ev = timed(fn)
        if r >= args.warmup:
            share[name].append(ev)
torch.cuda.synchronize()
fw = statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in share["forward"])
sc = statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in share["scoring"])
result["batch_share"] = {"captions": NB, "generator": "coco_train widths, random init, eval mode",
                         "one_generator_forward_us": round(fw, 1), "scoring_of_the_batch_us": round(sc, 1),
                         "scoring_share_of_one_forward_plus_scoring": round(sc / (fw + sc), 4)}
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
