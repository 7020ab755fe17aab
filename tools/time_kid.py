"""The sums of the kernel Inception distance (ops.poly_mmd_sums: mogan_poly3_mmd_f64, csrc/mogan_mmd.hip) against the same sums formed
by torch in fp64 on the device (per subset pair: gather and widen the rows, three fp64 matmuls, t * g + c, cube, sums; the diagonal
of xx / yy masked).  Method of tools/time_fid.py: hip events, --warmup calls, then --iters timed calls of each path, the two paths
alternating in one process; medians.  A record, not a gate: the project's kernel is the path whichever way it comes out.  The
torch formulation lives only here.
python tools/time_kid.py [--out profiles/kid_timing.json]"""
import argparse, json, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mogan_loader; mogan_loader.load()
from mogan_amd.attngan import kid as KID
from mogan_amd.hip import ops
ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--warmup", type=int, default=8)
ap.add_argument("--out", default="")
args = ap.parse_args()
dev = torch.device("cuda")
# (S, s, N, D): the protocol on a full split, and the protocol's subset count on a small split (every subset the whole split)
SHAPES = ((100, 1000, 30000, 2048), (100, 512, 512, 2048))


def stock(x, y, ix, iy, gamma, coef0):
    out = torch.empty((ix.shape[0], 3), dtype=torch.float64, device=x.device)
    off = ~torch.eye(ix.shape[1], dtype=torch.bool, device=x.device)
    for k in range(ix.shape[0]):
        a, b = x[ix[k].long()].double(), y[iy[k].long()].double()
        for q, (u, v, m) in enumerate(((a, a, off), (b, b, off), (a, b, None))):
            t = (u @ v.t()) * gamma + coef0
            t = (t * t) * t
            out[k, q] = (t * m).sum() if m is not None else t.sum()
    return out


def timed(fn):
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


result = {"method": "hip events around one call, %d warm-up calls, %d timed calls per path, paths alternating in one process, "
                    "medians in microseconds" % (args.warmup, args.iters), "device": torch.cuda.get_device_name(0), "shapes": []}
for S, s, N, D in SHAPES:
    g = torch.Generator(device=dev).manual_seed(N)
    # pool codes are averages of ReLU outputs: non-negative, column scales spread over a decade
    x = (torch.randn(N, D, device=dev, generator=g).abs() * torch.logspace(-1, 0, D, device=dev)).contiguous()
    y = (torch.randn(N, D, device=dev, generator=g).abs() * torch.logspace(-1, 0, D, device=dev) * 1.05).contiguous()
    ix, iy = [torch.from_numpy(t).to(dev) for t in KID.draw_subsets(N, N, S, s, 100)]
    gamma = 1.0 / D
    paths = {"kernel": lambda: ops.poly_mmd_sums(x, y, ix, iy, gamma, 1.0), "torch_fp64": lambda: stock(x, y, ix, iy, gamma, 1.0)}
    s0, s1 = paths["kernel"](), paths["torch_fp64"]()
    apart = float(((s0 - s1).abs() / s1.abs()).max())
    kid = KID.kid_from_sums(s0.cpu().numpy(), s)[:2]
    del s0, s1
    for _ in range(args.warmup):
        for fn in paths.values(): fn()
    torch.cuda.synchronize()
    us = {k: [] for k in paths}
    for _ in range(args.iters):
        for k, fn in paths.items(): us[k].append(timed(fn))
    T = (s + 63) // 64
    tiles = T * (T + 1) + T * T
    flop = 2.0 * S * tiles * 64 * 64 * D
    row = {"S": S, "s": s, "N": N, "D": D, "tiles_per_subset": tiles, "max_sum_difference_between_the_paths_rel": apart,
           "kid_of_the_timing_inputs": kid[0], "kid_std_of_the_timing_inputs": kid[1]}
    row.update({k + "_us": round(statistics.median(v), 2) for k, v in us.items()})
    row.update({k + "_min_us": round(min(v), 2) for k, v in us.items()})
    row["kernel_fp64_tflops_on_the_tiles_it_runs"] = round(flop / statistics.median(us["kernel"]) / 1e6, 2)
    row["rows_gathered_GB"] = round(S * 4 * T * T * 64 * D * 4 / 1e9, 3)      # two 64-row panels per tile, one on a diagonal: 4 T^2
    result["shapes"].append(row)
    print(row, flush=True)
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
