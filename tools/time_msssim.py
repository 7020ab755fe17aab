"""MS-SSIM (attngan/msssim.py; csrc/mogan_ssim.hip) at the real workload -- PairSimilarity.add for 64 pairs of 3 x 256 x 256 images over
five levels -- against the same stages formed by stock torch ops on the device: per level a grouped F.conv2d with the window along x
and one along y for each of the five planes d_a, d_b, d_a d_a, d_b d_b, d_a d_b (which torch writes to memory), the l and cs
arithmetic elementwise, the means in fp64, F.avg_pool2d between the levels.  Hip events around every call, 8 warm-up calls and the
median of 30 per path, the two paths alternating call by call in one process.  A record, not a gate: the project's kernels are the
path whichever way it comes out.  The torch formulation lives only here.
Also measured: the share of one msssim() batch (coco_train widths, 16 captions) that the scoring takes next to the generator's two
forwards -- the generator forward, and the three add() calls of the batch (8 real pairs, 8 generated pairs, 16 same-caption pairs).
python tools/time_msssim.py [--out profiles/msssim_timing.json]"""
import argparse, json, os, statistics, sys
import numpy as np
import torch
import torch.nn.functional as F
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mogan_loader; mogan_loader.load()
from mogan_amd.attngan import msssim as MS
ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=64)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--channels", type=int, default=3)
ap.add_argument("--scales", type=int, default=5)
ap.add_argument("--warmup", type=int, default=8)
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--batch", type=int, default=16, help="captions per batch of the share measurement")
ap.add_argument("--out", default="")
args = ap.parse_args()
assert torch.cuda.is_available(), "a timing needs the GPU"
dev = torch.device("cuda")
P, C, S, L = args.pairs, args.channels, args.size, args.scales
sizes = MS.scales_of(S, L)
wins = [torch.from_numpy(MS.window(s)).to(dev) for s in sizes]
g = torch.Generator(device=dev).manual_seed(5)
a = torch.rand((P, C, S, S), device=dev, generator=g) * 2 - 1
b = (0.5 * a + 0.5 * (torch.rand((P, C, S, S), device=dev, generator=g) * 2 - 1)).contiguous()


def timed(fn):
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record(); out = fn(); e1.record()
    return out, (e0, e1)


def kernel_add():
    ps = kernel_add.ps
    ps.n = 0
    ps.add(a, b)
    return ps.terms


kernel_add.ps = MS.PairSimilarity(S, C, P, L, dev)


def torch_add():
    x, y, out = a, b, []
    for j, win in enumerate(wins):
        n = win.numel()
        kx, ky = win.view(1, 1, 1, n).expand(5 * C, 1, 1, n).contiguous(), win.view(1, 1, n, 1).expand(5 * C, 1, n, 1).contiguous()
        da, db = 127.5 * x, 127.5 * y
        f = F.conv2d(F.conv2d(torch.cat([da, db, da * da, db * db, da * db], dim=1), kx, groups=5 * C), ky, groups=5 * C)
        ma, mb, eaa, ebb, eab = f.split(C, dim=1)
        saa, sbb, sab = eaa - ma * ma, ebb - mb * mb, eab - ma * mb
        mua, mub = 127.5 + ma, 127.5 + mb
        cs = (2 * sab + MS.C2) / ((saa + sbb) + MS.C2)
        ssim = (2 * (mua * mub) + MS.C1) / ((mua * mua + mub * mub) + MS.C1) * cs
        out.append(torch.stack([ssim.mean(dim=(1, 2, 3), dtype=torch.float64), cs.mean(dim=(1, 2, 3), dtype=torch.float64)], dim=1))
        if j + 1 < len(wins):
            x, y = F.avg_pool2d(x, 2), F.avg_pool2d(y, 2)
    return torch.stack(out, dim=1)


PATHS = {"kernel": kernel_add, "torch": torch_add}
events = {name: [] for name in PATHS}
terms = {}
for r in range(args.warmup + args.calls):
    for name, fn in PATHS.items():
        out, ev = timed(fn)
        if r >= args.warmup:
            events[name].append(ev)
        terms[name] = out
torch.cuda.synchronize()
us = {name: [e0.elapsed_time(e1) * 1e3 for e0, e1 in events[name]] for name in PATHS}
diff = float((terms["kernel"][:P] - terms["torch"]).abs().max())
score = MS.score_from_terms(terms["kernel"][:P].cpu().numpy())[0]
result = {"method": "hip events around every call; %d warm-up calls and the median of %d per path, the two paths alternating call by "
                    "call in one process; microseconds" % (args.warmup, args.calls),
          "device": torch.cuda.get_device_name(0),
          "workload": {"pairs": P, "channels": C, "size": S, "levels": sizes, "taps": [int(w.numel()) for w in wins]},
          "kernel_us": round(statistics.median(us["kernel"]), 1), "kernel_min_us": round(min(us["kernel"]), 1),
          "kernel_max_us": round(max(us["kernel"]), 1),
          "torch_us": round(statistics.median(us["torch"]), 1), "torch_min_us": round(min(us["torch"]), 1),
          "torch_max_us": round(max(us["torch"]), 1),
          "largest_difference_of_a_level_term_between_the_paths": diff,
          "mean_score_of_the_timing_inputs": float(score.mean())}
result["torch_over_kernel"] = round(result["torch_us"] / result["kernel_us"], 3)
# what the algorithm has to read: both images at every level, once
need = sum(2 * P * C * s * s * 4 for s in sizes)
result["bytes_the_levels_read"] = need
result["kernel_TB_per_s_of_those_bytes"] = round(need / result["kernel_us"] / 1e6, 3)
print(json.dumps(result), flush=True)

# ------------------------------------------------------------------------------------------------ the share of one msssim() batch
from mogan_amd.attngan import model, synthetic
from mogan_amd.attngan.miscc.config import cfg, set_coco_train_defaults
from mogan_amd.attngan.miscc.utils import weights_init
set_coco_train_defaults()
B = args.batch
torch.manual_seed(3)
netG = model.G_NET()
netG.apply(weights_init)
netG = netG.to(dev).eval()
bt = synthetic.to_device(synthetic.make_batch(B, words_num=cfg.TEXT.WORDS_NUM, nef=cfg.TEXT.EMBEDDING_DIM, seed=3), dev)
figs = {k: MS.PairSimilarity(256, 3, n, 5, dev) for k, n in (("real", B // 2), ("generated", B // 2), ("same_caption", B))}


def forward():
    with torch.no_grad():
        return netG(bt["z"], bt["sent_emb"], bt["words_embs"], bt["mask"], bt["tmi"], bt["label_one_hot"], eps=bt["eps"])[0][-1]


fake = forward().float().contiguous()
again = fake.flip(0).contiguous()
real = bt["imgs"][-1].contiguous()


def scoring():
    for f in figs.values():
        f.n = 0
    h = B // 2
    figs["real"].add(real[:h].contiguous(), real[h:].contiguous())
    figs["generated"].add(fake[:h].contiguous(), fake[h:].contiguous())
    figs["same_caption"].add(fake, again)


share = {"forward": [], "scoring": []}
for r in range(args.warmup + args.calls):
    for name, fn in (("forward", forward), ("scoring", scoring)):
        _, ev = timed(fn)
        if r >= args.warmup:
            share[name].append(ev)
torch.cuda.synchronize()
fw = statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in share["forward"])
sc = statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in share["scoring"])
result["batch_share"] = {"captions": B, "generator": "coco_train widths, random init, eval mode",
                         "one_generator_forward_us": round(fw, 1), "scoring_of_the_batch_us": round(sc, 1),
                         "scoring_share_of_two_forwards_plus_scoring": round(sc / (2 * fw + sc), 4)}
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
