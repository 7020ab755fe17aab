"""CNN_ENCODER.pool_code for one batch of 32 images at 256 x 256 under the two trunk variants: "torchvision", the
network DAMSM trains under, and "fid", the published FID Inception network -- the same weights (random-init, frozen, eval mode), two
encoders, so that each keeps its packed trunk.  What "fid" adds is one more GEMM member and one more tail member in Mixed_7c (the
max-pooled block input and branch_pool's own convolution over it); every other pool branch only changes its tail member's box mode.
Method of tools/time_inception_score.py: hip events around one call, --warmup untimed calls, then --iters timed calls of each
path, the two paths alternating in one process; medians with the range, and every call in order so that a run that has not settled shows.
A record, not a gate: no speed target was set.
--default_only times "torchvision" alone: with MOGAN_LIB pointing at a library built from another commit, the same tool shows
whether the train step's instantiations of the tail kernel moved.
python tools/time_trunk_variant.py [--out profiles/trunk_variant_timing.json]"""
import argparse, copy, json, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mogan_loader; mogan_loader.load()
from mogan_amd.attngan.model import CNN_ENCODER
ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--warmup", type=int, default=12)
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--default_only", action="store_true")
ap.add_argument("--out", default="")
args = ap.parse_args()
dev = torch.device("cuda")


def timed(fn):
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def spread(v):
    return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


torch.manual_seed(0)
base = CNN_ENCODER(256).eval()
for p in base.parameters():
    p.requires_grad = False
encoders = {"torchvision": base.to(dev)}
if not args.default_only:
    encoders["fid"] = copy.deepcopy(base).to(dev).set_trunk_variant("fid")
img = torch.rand(args.batch, 3, 256, 256, device=dev) * 2 - 1
us = {k: [] for k in encoders}
with torch.no_grad():
    for _ in range(args.warmup):
        for enc in encoders.values(): enc.pool_code(img)
    torch.cuda.synchronize()
    for _ in range(args.iters):
        for k, enc in encoders.items(): us[k].append(timed(lambda: enc.pool_code(img)))
    codes = {k: enc.pool_code(img) for k, enc in encoders.items()}
result = {"method": "hip events around one call of CNN_ENCODER.pool_code, %d warm-up calls, %d timed calls per variant, the variants "
                    "alternating in one process, median / min / max in microseconds" % (args.warmup, args.iters),
          "device": torch.cuda.get_device_name(0), "library": os.environ.get("MOGAN_LIB", "libmogan_hip.so"),
          "batch": args.batch, "image": [3, 256, 256]}
for k, v in us.items():
    result[k + "_us"] = spread(v)
    result[k + "_us_each_call_in_order"] = [round(t, 1) for t in v]
if "fid" in us:
    result["fid_over_torchvision"] = round(statistics.median(us["fid"]) / statistics.median(us["torchvision"]), 4)
    a, b = codes["fid"].double(), codes["torchvision"].double()
    result["pool_codes_apart_rel_l2"] = float((a - b).norm() / b.norm())
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
