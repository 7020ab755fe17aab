"""The five device calls of condGANTrainer.prdc (ops.knn_sqdist twice, ops.ball_counts three times: mogan_knn_sqdist_f64 and
mogan_ball_count_f64, csrc/mogan_knn.hip) against the same five steps formed by torch in fp64 on the device (row blocks of the
distance matrix in Gram form -- norms, one fp64 matmul, clamp --, kthvalue for the radii, compare and sum for the counts).  Method
of tools/time_kid.py: hip events, --warmup calls, then --iters timed calls of each path, the two paths alternating in one process;
medians.  A record, not a gate: the project's kernels are the path whichever way it comes out.  The torch formulation lives only here.
python tools/time_prdc.py [--out profiles/prdc_timing.json]"""
import argparse, json, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mogan_loader; mogan_loader.load()
from mogan_amd.attngan import prdc as PRDC
from mogan_amd.hip import ops
ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--block", type=int, default=2048, help="rows of the distance matrix the torch path holds at a time")
ap.add_argument("--out", default="")
args = ap.parse_args()
dev = torch.device("cuda")
# (N = M, D): a full split, and a small one (where the support tiles are split over several workgroups per stripe)
SHAPES = ((30000, 2048), (2048, 2048))
KP, KD = PRDC.K_PR, PRDC.K_DC
STEPS = ("radii_real", "radii_fake", "fake_in_real", "real_in_fake", "real_own")


def blocks(q, p, B):
    """row blocks (start, d2 (b, N) fp64) of the distance matrix of q against p, Gram form"""
    p64 = p.double()
    npp = (p64 * p64).sum(1)
    for i in range(0, q.shape[0], B):
        q64 = q[i:i + B].double()
        yield i, (((q64 * q64).sum(1)[:, None] + npp[None, :]) - 2.0 * (q64 @ p64.t())).clamp_(min=0.0)


def stock_radii(x, ks, B):
    out = torch.empty((x.shape[0], len(ks)), dtype=torch.float64, device=x.device)
    for i, d in blocks(x, x, B):
        d[torch.arange(d.shape[0], device=x.device), torch.arange(i, i + d.shape[0], device=x.device)] = float("inf")
        for c, k in enumerate(ks):
            out[i:i + d.shape[0], c] = d.kthvalue(k, dim=1).values
    return out


def stock_counts(q, p, r2, side, B):
    out = torch.empty((q.shape[0], r2.shape[1]), dtype=torch.int32, device=q.device)
    for i, d in blocks(q, p, B):
        for c in range(r2.shape[1]):
            r = r2[None, :, c] if side == "support" else r2[i:i + d.shape[0], c, None]
            out[i:i + d.shape[0], c] = (d <= r).sum(1)
    return out


def timed(fn):
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record(); out = fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3, out


def five(real, fake, radii, counts):
    """the five steps in the trainer's order through `radii(x, ks)` and `counts(q, p, r2, side)`: (microseconds per step, the
    (n, 4) counts the trainer reads back)"""
    us = {}
    us["radii_real"], rr = timed(lambda: radii(real, (KP, KD)))
    us["radii_fake"], rf = timed(lambda: radii(fake, (KP,)))
    us["fake_in_real"], a = timed(lambda: counts(fake, real, rr, "support"))
    us["real_in_fake"], b = timed(lambda: counts(real, fake, rf, "support"))
    us["real_own"], c = timed(lambda: counts(real, fake, rr[:, 1:].contiguous(), "query"))
    return us, torch.cat([a, b, c], dim=1)


def kernel_radii(x, ks):
    return ops.knn_sqdist(x, max(ks))[:, [k - 1 for k in ks]].contiguous()


result = {"method": "hip events around each of the five calls, %d warm-up rounds, %d timed rounds per path, paths alternating in one "
                    "process, medians in microseconds; torch path in row blocks of %d" % (args.warmup, args.iters, args.block),
          "device": torch.cuda.get_device_name(0), "k_pr": KP, "k_dc": KD, "shapes": []}
for N, D in SHAPES:
    g = torch.Generator(device=dev).manual_seed(N)
    # pool codes are averages of ReLU outputs: non-negative, column scales spread over a decade; the generated side is narrower
    # and slightly shifted, so that precision and recall differ
    scale = torch.logspace(-1, 0, D, device=dev)
    real = (torch.randn(N, D, device=dev, generator=g).abs() * scale).contiguous()
    fake = (torch.randn(N, D, device=dev, generator=g).abs() * scale * 0.97 + 0.003).contiguous()
    paths = {"kernel": lambda: five(real, fake, kernel_radii, ops.ball_counts),
             "torch_fp64": lambda: five(real, fake, lambda x, ks: stock_radii(x, ks, args.block),
                                        lambda q, p, r2, side: stock_counts(q, p, r2, side, args.block))}
    c0, c1 = paths["kernel"]()[1].cpu().numpy(), paths["torch_fp64"]()[1].cpu().numpy()
    scores = [PRDC.scores_from_counts(c[:, 0:2], c[:, 2], c[:, 3], KD) for c in (c0, c1)]
    differing = int((c0 != c1).sum())
    for _ in range(args.warmup):
        for fn in paths.values(): fn()
    torch.cuda.synchronize()
    us = {k: {s: [] for s in STEPS} for k in paths}
    for _ in range(args.iters):
        for k, fn in paths.items():
            for s, v in fn()[0].items(): us[k][s].append(v)
    flop = 2.0 * N * N * D                                    # one pass over the n^2 D products
    row = {"N": N, "M": N, "D": D, "scores_of_the_timing_inputs_kernel": scores[0], "scores_of_the_timing_inputs_torch_fp64": scores[1],
           "counts_that_differ_between_the_paths": differing, "of_counts": int(c0.size)}
    for k in paths:
        med = {s: statistics.median(us[k][s]) for s in STEPS}
        row[k + "_us"] = {s: round(v, 1) for s, v in med.items()}
        row[k + "_total_us"] = round(sum(med.values()), 1)
        row[k + "_total_min_us"] = round(sum(min(us[k][s]) for s in STEPS), 1)
    row["kernel_fp64_tflops_per_pass"] = {s: round(flop / statistics.median(us["kernel"][s]) / 1e6, 2) for s in STEPS}
    result["shapes"].append(row)
    print(row, flush=True)
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
