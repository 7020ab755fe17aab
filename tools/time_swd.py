"""The stages of the sliced Wasserstein distance (attngan/swd.py; csrc/mogan_swd.hip) at the real workload -- 256x256 images of 3
channels, 16 384 per side, 128 patches, 128 directions, 4 repeats, levels 256 .. 16 -- against the same stages formed by stock torch
ops on the device: the pyramid by F.conv2d over a reflect-padded image (stride 2 down; zero insertion, then the filter times 4 up),
the descriptors by an index gather, the moments by mean / std in fp64, the projection by an fp32 matmul of the standardised
descriptors, the reduction by (a - b).abs().double().sum.  The sort is torch.sort in both.  Hip events around every stage call, the
two paths alternating round by round in one process; per stage the sum over all batches, levels, sides and repeats of a round,
then the median over the rounds.  The images are drawn per batch on the device and are the same for both paths.  A record, not a
gate: the project's kernels are the path whichever way it comes out.  The torch formulation lives only here.
Also written: for the projection cases of tests/swd_cases.py, the deviation of numpy's fp32 matmul from the fp64 oracle and the
kernel's, so that a reader sees how much of the test's margin (4 x numpy's) is used.
python tools/time_swd.py [--images 16384] [--out profiles/swd_timing.json]"""
import argparse, json, os, statistics, sys
import numpy as np
import torch
import torch.nn.functional as F
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mogan_loader; mogan_loader.load()
from mogan_amd.attngan import swd as SWD
from mogan_amd.hip import ops
ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=16384)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--channels", type=int, default=3)
ap.add_argument("--patches", type=int, default=128)
ap.add_argument("--dirs", type=int, default=128)
ap.add_argument("--repeats", type=int, default=4)
ap.add_argument("--min_res", type=int, default=16)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--out", default="")
args = ap.parse_args()
dev = torch.device("cuda")
C, P, D = args.channels, args.patches, args.dirs
sizes = SWD.levels(args.size, args.min_res)
rows = args.images * P
STAGES = ("pyramid", "gather", "moments", "project", "sort", "absdiff")
W5 = torch.tensor([1.0, 4.0, 6.0, 4.0, 1.0], device=dev) / 16.0
K5 = (W5[:, None] * W5[None, :]).expand(C, 1, 5, 5).contiguous()
OFF = torch.arange(-3, 4, device=dev)


class Clock:
    """hip events around stage calls; the sums per stage are read once per round"""
    def __init__(self):
        self.pairs = []

    def run(self, stage, fn):
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        e0.record(); out = fn(); e1.record()
        self.pairs.append((stage, e0, e1))
        return out

    def sums(self):
        torch.cuda.synchronize()
        out = dict.fromkeys(STAGES, 0.0)
        for stage, e0, e1 in self.pairs:
            out[stage] += e0.elapsed_time(e1) * 1e3
        self.pairs = []
        return out


def images(batch_index, side):
    g = torch.Generator(device=dev).manual_seed(1000 * batch_index + side)
    img = torch.rand((args.batch, C, args.size, args.size), device=dev, generator=g) * 2 - 1
    return img if side == 0 else (img * 0.8 + 0.1 * torch.randn(img.shape, device=dev, generator=g)).clamp_(-1, 1)


# ---------------------------------------------------------------------------------------------------------------- the kernel path
def kernel_pyramid(img):
    B = img.shape[0]
    g, out = img.view(B * C, args.size, args.size), []
    for s in sizes[:-1]:
        down = ops.pyr_down(g)
        out.append(ops.lap_residual(g, down).view(B, C, s, s))
        g = down
    out.append(g.view(B, C, sizes[-1], sizes[-1]))
    return out


def kernel_tail(clock, real, fake, dirs):
    mom = clock.run("moments", lambda: (ops.swd_moments(real), ops.swd_moments(fake)))
    sums = []
    for d in dirs:
        pr = clock.run("project", lambda: ops.swd_project(real, mom[0], d))
        pf = clock.run("project", lambda: ops.swd_project(fake, mom[1], d))
        sr = clock.run("sort", lambda: torch.sort(pr, dim=-1).values)
        sf = clock.run("sort", lambda: torch.sort(pf, dim=-1).values)
        del pr, pf
        sums.append(clock.run("absdiff", lambda: ops.swd_absdiff(sr, sf)))
        del sr, sf
    return torch.stack(sums)


# ----------------------------------------------------------------------------------------------------------------- the torch path
def torch_down(g):
    return F.conv2d(F.pad(g, (2, 2, 2, 2), mode="reflect"), K5, stride=2, groups=C)


def torch_up(d):
    z = torch.zeros((d.shape[0], C, 2 * d.shape[2], 2 * d.shape[3]), device=dev)
    z[:, :, ::2, ::2] = d
    return F.conv2d(F.pad(z, (2, 2, 2, 2), mode="reflect"), K5 * 4, groups=C)


def torch_pyramid(img):
    g, out = img, []
    for s in sizes[:-1]:
        down = torch_down(g)
        out.append(g - torch_up(down))
        g = down
    out.append(g)
    return out


def torch_gather(level, tri, desc, row0):
    n, cy, cx = tri[:, 0].long(), tri[:, 1].long(), tri[:, 2].long()
    ch = torch.arange(C, device=dev)
    got = level[n[:, None, None, None], ch[None, :, None, None], (cy[:, None] + OFF[None, :])[:, None, :, None],
                (cx[:, None] + OFF[None, :])[:, None, None, :]]
    desc[row0:row0 + tri.shape[0]] = got.reshape(tri.shape[0], C * 49)


def torch_moments(desc):
    x = desc.view(desc.shape[0], C, 49)
    m = x.mean(dim=(0, 2), dtype=torch.float64)
    v = ((x.double() - m[None, :, None]) ** 2).mean(dim=(0, 2))
    return torch.stack([m, v.sqrt()], dim=1)


def torch_project(desc, mom, d):
    z = (desc.view(desc.shape[0], C, 49) - mom[None, :, 0, None].float()) / mom[None, :, 1, None].float()
    return torch.matmul(d.t(), z.view(desc.shape[0], C * 49).t())


def torch_tail(clock, real, fake, dirs):
    mom = clock.run("moments", lambda: (torch_moments(real), torch_moments(fake)))
    sums = []
    for d in dirs:
        pr = clock.run("project", lambda: torch_project(real, mom[0], d))
        pf = clock.run("project", lambda: torch_project(fake, mom[1], d))
        sr = clock.run("sort", lambda: torch.sort(pr, dim=-1).values)
        sf = clock.run("sort", lambda: torch.sort(pf, dim=-1).values)
        del pr, pf
        sums.append(clock.run("absdiff", lambda: (sr - sf).abs().double().sum(dim=1)))
        del sr, sf
    return torch.stack(sums)


PATHS = {"kernel": (kernel_pyramid, lambda lv, t, d, r: ops.swd_gather(lv, t, d, r), kernel_tail),
         "torch": (torch_pyramid, torch_gather, torch_tail)}


def one_round(name, desc):
    """the whole score once: (stage sums in microseconds, the per-level figures)"""
    pyramid, gather, tail = PATHS[name]
    clock = Clock()
    rng = [np.random.RandomState(100), np.random.RandomState(101)]
    for b in range(args.images // args.batch):
        for side in (0, 1):
            img = images(b, side)
            tables = [torch.from_numpy(t).to(dev) for t in SWD.draw_centres(rng[side], sizes, args.batch, P)]
            levels = clock.run("pyramid", lambda: pyramid(img))
            for lv, t, buf in zip(levels, tables, desc[side]):
                clock.run("gather", lambda: gather(lv.contiguous(), t, buf, b * args.batch * P))
    drng = np.random.RandomState(102)
    figures = []
    for li in range(len(sizes)):
        dirs = [torch.from_numpy(SWD.draw_directions(drng, C, D)).to(dev) for _ in range(args.repeats)]
        sums = tail(clock, desc[0][li], desc[1][li], dirs)
        figures.append(SWD.figure_from_sums(sums.cpu().numpy(), rows))
    return clock.sums(), figures


print("descriptors: %.2f GB for both sides" % (SWD.descriptor_bytes(len(sizes), rows, C) / 1e9), flush=True)
desc = [[torch.empty((rows, C * 49), dtype=torch.float32, device=dev) for _ in sizes] for _ in (0, 1)]
us = {name: {s: [] for s in STAGES} for name in PATHS}
figures = {}
for r in range(args.warmup + args.rounds):
    for name in PATHS:
        sums, figures[name] = one_round(name, desc)
        print("round %d %s: %s" % (r, name, {k: round(v) for k, v in sums.items()}), flush=True)
        if r >= args.warmup:
            for s in STAGES:
                us[name][s].append(sums[s])
result = {"method": "hip events around every stage call; per stage the sum over all batches, levels, sides and repeats of one round; "
                    "%d warm-up and %d timed rounds per path, paths alternating in one process; medians in microseconds"
                    % (args.warmup, args.rounds),
          "device": torch.cuda.get_device_name(0),
          "workload": {"images_per_side": args.images, "size": args.size, "channels": C, "patches": P, "dirs": D, "repeats": args.repeats,
                       "levels": sizes, "rows_per_level_and_side": rows, "batch": args.batch,
                       "descriptor_GB_both_sides": round(SWD.descriptor_bytes(len(sizes), rows, C) / 1e9, 2)},
          "figures_of_the_timing_inputs": {k: v for k, v in figures.items()}}
for name in PATHS:
    med = {s: round(statistics.median(us[name][s]), 1) for s in STAGES}
    result[name + "_us"] = med
    result[name + "_min_us"] = {s: round(min(us[name][s]), 1) for s in STAGES}
    result[name + "_total_us"] = round(sum(med.values()), 1)
k, t = result["kernel_us"], result["torch_us"]
result["torch_over_kernel_per_stage"] = {s: round(t[s] / k[s], 3) for s in STAGES}
result["torch_over_kernel_total"] = round(result["torch_total_us"] / result["kernel_total_us"], 3)
ours = [s for s in STAGES if s != "sort"]
result["torch_over_kernel_without_the_sort"] = round(sum(t[s] for s in ours) / sum(k[s] for s in ours), 3)
result["sort_share_of_the_kernel_path"] = round(k["sort"] / result["kernel_total_us"], 3)
# achieved bytes per second of the stages that stream the descriptors once (what the algorithm needs, from the shapes)
n_lr = len(sizes) * args.repeats * 2
result["kernel_project_TB_per_s"] = round(n_lr * (rows * C * 49 * 4 + rows * D * 4) / k["project"] / 1e6, 3)
result["kernel_absdiff_TB_per_s"] = round(n_lr * rows * D * 4 / k["absdiff"] / 1e6, 3)
result["kernel_moments_TB_per_s"] = round(len(sizes) * 2 * 2 * rows * C * 49 * 4 / k["moments"] / 1e6, 3)

import swd_cases as S
result["projection_deviation_from_fp64"] = []
for case in S.PROJECT_CASES:
    d, m, v = S.project_inputs(case)
    want = S.projections(d, m, v)
    got = ops.swd_project(torch.from_numpy(d).to(dev), torch.from_numpy(m).to(dev), torch.from_numpy(v).to(dev)).cpu().numpy()
    result["projection_deviation_from_fp64"].append({"rows_C_D": list(case), "numpy_fp32_matmul": S.numpy_fp32_deviation(d, m, v),
                                                     "kernel": float(np.abs(got.astype(np.float64) - want).max()),
                                                     "test_bound": S.projection_bound(d, m, v)})
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
