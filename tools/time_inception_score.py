"""The sums of the Inception Score (ops.softmax_head_sums: mogan_softmax_head_f64, csrc/mogan_softmax_head.hip) against the same stages
formed by stock torch in fp64 on the device (x.double() @ W.double().T + b, log_softmax, exp, the row sums of p log p, the splits' sums
of p -- which writes the n x C matrix the kernel never forms), at the score's size: n = 30 000 codes, D = 2048, C = 1000, S = 10.
Method of tools/time_kid.py: hip events, --warmup calls, then --iters timed calls of each path, the two paths alternating in one
process; medians with the range.  Beside it one batch of the trunk (CNN_ENCODER.pool_code, random-init, frozen, eval mode), which
every code has to pass first -- --trunk_warmup untimed batches, then --iters timed ones, each listed -- and the entry point's share of a
pass at the median and at both ends of the trunk's range.  A record, not a gate: no speed target was set, the kernel is the
path whichever way it comes out.  The torch formulation lives only here.
python tools/time_inception_score.py [--out profiles/inception_score_timing.json]"""
import argparse, json, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mogan_loader; mogan_loader.load()
from mogan_amd.attngan import inception_score as IS
from mogan_amd.hip import ops
ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--batch", type=int, default=32, help="images of the trunk batch")
ap.add_argument("--trunk_warmup", type=int, default=12, help="untimed trunk batches before the timed ones")
ap.add_argument("--out", default="")
args = ap.parse_args()
dev = torch.device("cuda")
SHAPES = ((30000, 2048, 1000, 10), (30000, 2048, 1000, 1), (5000, 2048, 1000, 10))


def stock(x, w, b, bounds):
    z = x.double() @ w.double().t() + b.double()
    lp = torch.log_softmax(z, dim=1)
    p = lp.exp()
    return (p * lp).sum(dim=1), torch.stack([p[lo:hi].sum(dim=0) for lo, hi in bounds])


def timed(fn):
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def spread(v):
    return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


result = {"method": "hip events around one call, %d warm-up calls, %d timed calls per path, paths alternating in one process, "
                    "median / min / max in microseconds" % (args.warmup, args.iters), "device": torch.cuda.get_device_name(0),
          "shapes": []}
for n, D, C, S in SHAPES:
    g = torch.Generator(device=dev).manual_seed(n + S)
    # pool codes are averages of ReLU outputs: non-negative, column scales spread over a decade; a head that gives logits of a few units
    x = (torch.randn(n, D, device=dev, generator=g).abs() * torch.logspace(-1, 0, D, device=dev)).contiguous()
    w = (torch.randn(C, D, device=dev, generator=g) * 0.1).contiguous()
    b = (torch.randn(C, device=dev, generator=g) * 0.1).contiguous()
    bounds = IS.split_bounds(n, S)
    paths = {"kernel": lambda: ops.softmax_head_sums(x, w, b, S), "torch_fp64": lambda: stock(x, w, b, bounds)}
    (h0, p0), (h1, p1) = paths["kernel"](), paths["torch_fp64"]()
    apart = {"row_h_abs": float((h0 - h1).abs().max()), "psum_rel": float(((p0 - p1).abs() / p1.abs().clamp_min(1e-300)).max())}
    figure = IS.finish(h0.cpu().numpy(), p0.cpu().numpy(), n)["inception_score"]
    del h0, p0, h1, p1
    for _ in range(args.warmup):
        for fn in paths.values(): fn()
    torch.cuda.synchronize()
    us = {k: [] for k in paths}
    for _ in range(args.iters):
        for k, fn in paths.items(): us[k].append(timed(fn))
    row = {"n": n, "D": D, "C": C, "S": S, "difference_between_the_paths": apart, "inception_score_of_the_timing_inputs": figure}
    row.update({k + "_us": spread(v) for k, v in us.items()})
    row["kernel_over_torch"] = round(statistics.median(us["kernel"]) / statistics.median(us["torch_fp64"]), 3)
    # the kernel forms every logit twice (one walk for the log-sum-exp, one for p)
    row["kernel_fp64_tflops_both_walks"] = round(2 * 2.0 * n * D * C / statistics.median(us["kernel"]) / 1e6, 2)
    row["matrix_torch_writes_MB"] = round(n * C * 8 / 1e6, 1)
    row["kernel_workspace_MB"] = round(int(ops.lib.load().mogan_softmax_head_ws_bytes(n, C, S)) / 1e6, 2)
    result["shapes"].append(row)
    print(row, flush=True)
    del x, w, b
    torch.cuda.empty_cache()

# one batch of the trunk, which every code passes before the head sees it
from mogan_amd.attngan.model import CNN_ENCODER
torch.manual_seed(0)
enc = CNN_ENCODER(256).to(dev).eval()
for p in enc.parameters():
    p.requires_grad = False
img = torch.rand(args.batch, 3, 256, 256, device=dev) * 2 - 1
with torch.no_grad():
    for _ in range(args.trunk_warmup): enc.pool_code(img)
    torch.cuda.synchronize()
    trunk = [timed(lambda: enc.pool_code(img)) for _ in range(args.iters)]
head = result["shapes"][0]["kernel_us"]["median"]


def share(us):
    """the head's call over trunk plus head, the trunk at `us` per batch for 30 000 images"""
    return round(head / (head + us / args.batch * 30000), 6)


# the calls in order, so that a run that has not settled shows; the share at the median and at both ends of the range
result["trunk"] = {"batch": args.batch, "warmup": args.trunk_warmup, "pool_code_us": spread(trunk),
                   "pool_code_us_each_call_in_order": [round(v, 1) for v in trunk],
                   "trunk_us_for_30000_images_at_the_median": round(statistics.median(trunk) / args.batch * 30000, 0),
                   "head_share_of_trunk_plus_head": {"median": share(statistics.median(trunk)), "at_the_fastest_trunk_call": share(min(trunk)),
                                                     "at_the_slowest_trunk_call": share(max(trunk))}}
print(result["trunk"], flush=True)
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
