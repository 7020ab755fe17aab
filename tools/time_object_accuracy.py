"""The device work of object accuracy by nearest labelled training crops, measured three ways.

1. ops.knn_label (mogan_knn_label_f64, csrc/mogan_knn.hip) at the score's size -- 30 000 query crops against 150 000 bank crops,
   K = 5, D = 256 (one channel of 16 x 16) and D = 768 (three) -- against the formulation it replaces: ONE ops.knn_cross over the
   whole bank for the K list plus, per class, one ops.knn_cross of the class's queries against the bank rows of that class and one
   against all others (index_select of queries and bank, positions mapped back).  That formulation is the code that existed before
   the kernel, not the code under test; both give the same bits, which the run checks first.
2. ops.knn_cross alone at the same sizes and at D = 2048: its time against D, and the straight line through the two score sizes
   taken to D = 0 -- what the selection, the norms and the merge cost when the MFMA tile loop costs nothing.  This is the figure
   behind the decision whether all four waves should select (section 9m).
3. The object-accuracy work of one 64-image multi-mnist batch in the pass -- ObjectCrops.sink: one read-back, the host list, one
   upload and two crop launches -- as a share of the generator's forward for that batch (the tree's default widths).

Method of tools/time_nn.py: hip events, --warmup rounds, then --iters timed rounds with the paths alternating in one process;
medians.  A record, not a gate.
python tools/time_object_accuracy.py [--out profiles/object_accuracy_timing.json]"""
import argparse, json, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mogan_loader; mogan_loader.load()
from mogan_amd.hip import ops
ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--shapes", default="30000x150000x256x5x10,30000x150000x768x5x36", help="M x N x D x K x classes, comma separated")
ap.add_argument("--cross_dims", default="256,768,2048", help="widths at which ops.knn_cross alone is timed (M, N, K of the first shape)")
ap.add_argument("--out", default="")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("time_object_accuracy.py measures on the GPU; none is present")
dev = torch.device("cuda")
SHAPES = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
NO_ROW = 2147483647


def partitioned(q, ql, p, pl, K, classes):
    """the formulation before the kernel: 1 + 2 per class calls of ops.knn_cross"""
    d2, idx = ops.knn_cross(q, p, K)
    M = q.shape[0]
    out = [torch.full((M,), float("inf"), dtype=torch.float64, device=q.device), torch.full((M,), NO_ROW, dtype=torch.int32, device=q.device),
           torch.full((M,), float("inf"), dtype=torch.float64, device=q.device), torch.full((M,), NO_ROW, dtype=torch.int32, device=q.device)]
    for c in range(classes):
        rows = (ql == c).nonzero().flatten()
        if not rows.numel():
            continue
        qc = q.index_select(0, rows)
        for o, part in ((0, (pl == c).nonzero().flatten()), (2, (pl != c).nonzero().flatten())):
            if part.numel():
                d, i = ops.knn_cross(qc, p.index_select(0, part), 1)
                out[o][rows] = d[:, 0]
                out[o + 1][rows] = part[i[:, 0].long()].int()
    return (d2, idx) + tuple(out)


def timed(fn):
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record(); out = fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3, out


def medians(paths, iters, warmup):
    for _ in range(warmup):
        for fn in paths.values(): fn()
    torch.cuda.synchronize()
    us = {k: [] for k in paths}
    for _ in range(iters):
        for k, fn in paths.items(): us[k].append(timed(fn)[0])
    return {k: (round(statistics.median(v), 1), round(min(v), 1)) for k, v in us.items()}


def crops_like(n, D, g):
    """rows shaped like crops: values in [-1, 1], smooth along the row (neighbouring pixels agree)"""
    base = torch.randn(n, D // 8 + 1, device=dev, generator=g).repeat_interleave(8, dim=1)[:, :D]
    return (0.7 * base + 0.3 * torch.randn(n, D, device=dev, generator=g)).clamp_(-1, 1).contiguous()


result = {"method": "hip events around one call, %d warm-up rounds, %d timed rounds per path, paths alternating in one process, "
                    "medians in microseconds" % (args.warmup, args.iters),
          "device": torch.cuda.get_device_name(0), "knn_label": [], "knn_cross_by_width": [], "batch": None}
for M, N, D, K, classes in SHAPES:
    g = torch.Generator(device=dev).manual_seed(N + D)
    bank, query = crops_like(N, D, g), crops_like(M, D, g)
    pl = torch.randint(0, classes, (N,), device=dev, generator=g).int()
    ql = torch.randint(0, classes, (M,), device=dev, generator=g).int()
    paths = {"knn_label": lambda: ops.knn_label(query, ql, bank, pl, K), "partitioned_knn_cross": lambda: partitioned(query, ql, bank, pl, K, classes),
             "knn_cross_alone": lambda: ops.knn_cross(query, bank, K)}
    a, b = paths["knn_label"](), paths["partitioned_knn_cross"]()
    same_bits = all(torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x, y.view(torch.int64) if y.dtype == torch.float64 else y)
                    for x, y in zip(a, b))
    del a, b
    med = medians(paths, args.iters, args.warmup)
    row = {"M": M, "N": N, "D": D, "K": K, "classes": classes, "calls_of_the_partitioned_formulation": 1 + 2 * classes,
           "both_formulations_give_the_same_bits": bool(same_bits)}
    for k, (m, lo) in med.items():
        row[k + "_us"], row[k + "_min_us"] = m, lo
    row["knn_label_over_partitioned"] = round(row["knn_label_us"] / row["partitioned_knn_cross_us"], 3)
    row["knn_label_over_knn_cross_alone"] = round(row["knn_label_us"] / row["knn_cross_alone_us"], 3)
    row["knn_label_fp64_tflops"] = round(2.0 * M * N * D / row["knn_label_us"] / 1e6, 2)
    result["knn_label"].append(row)
    print(row, flush=True)
    del bank, query, pl, ql

M, N, _, K, _ = SHAPES[0]
widths = [int(v) for v in args.cross_dims.split(",")]
for D in widths:
    g = torch.Generator(device=dev).manual_seed(N + D)
    bank, query = crops_like(N, D, g), crops_like(M, D, g)
    m, lo = medians({"knn_cross": lambda: ops.knn_cross(query, bank, K)}, max(6, args.iters // 3), args.warmup)["knn_cross"]
    row = {"M": M, "N": N, "D": D, "K": K, "knn_cross_us": m, "knn_cross_min_us": lo, "fp64_tflops": round(2.0 * M * N * D / m / 1e6, 2)}
    result["knn_cross_by_width"].append(row)
    print(row, flush=True)
    del bank, query
if len(widths) >= 2:
    (d0, t0), (d1, t1) = [(r["D"], r["knn_cross_us"]) for r in result["knn_cross_by_width"][:2]]
    slope = (t1 - t0) / (d1 - d0)
    at0 = t0 - slope * d0
    result["knn_cross_line"] = {"through": [d0, d1], "us_per_feature": round(slope, 2), "us_at_width_0": round(at0, 1),
                                "share_of_the_time_at_%d" % d0: round(at0 / t0, 3), "share_of_the_time_at_%d" % d1: round(at0 / t1, 3)}
    print(result["knn_cross_line"], flush=True)

# 3: one 64-image multi-mnist batch
from mogan_amd.stackgan import synthetic
from mogan_amd.stackgan.engine import generate
from mogan_amd.stackgan.evaluate import ObjectCrops
from mogan_amd.stackgan.multi_mnist import model
from mogan_amd.stackgan.multi_mnist.miscc.config import cfg
from mogan_amd.stackgan.trainer_base import weights_init
torch.manual_seed(0)
netG = model.STAGE1_G()
netG.apply(weights_init)
netG = netG.to(dev).eval()
b = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in synthetic.make_batch("mnist", 64, seed=0, z_dim=cfg.Z_DIM).items()}
b["real_imgs"], b["tm"], b["tmi"], b["label_one_hot"] = (b[k].float().contiguous() for k in ("real_imgs", "tm", "tmi", "label_one_hot"))
acc = ObjectCrops("mnist", 64 * (args.iters + args.warmup + 2), 64, 1, 3, device=dev)
with torch.no_grad():
    fake = generate(netG, model.VARIANT, 1, b)[0]
    med = medians({"generator_forward": lambda: generate(netG, model.VARIANT, 1, b)[0],
                   "object_crops_sink": lambda: acc.sink(b["real_imgs"], fake, b["tm"], b["label_one_hot"], 64)}, args.iters, args.warmup)
result["batch"] = {"tree": "multi-mnist", "images": 64, "objects": 192, "GF_DIM": int(cfg.GAN.GF_DIM),
                   "generator_forward_us": med["generator_forward"][0], "object_crops_sink_us": med["object_crops_sink"][0],
                   "sink_over_forward": round(med["object_crops_sink"][0] / med["generator_forward"][0], 3),
                   "note": "the sink's time is host time between two events: one read-back, the host list, one upload, two launches"}
print(result["batch"], flush=True)
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
