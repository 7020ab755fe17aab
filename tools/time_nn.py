"""ops.knn_cross (mogan_knn_cross_f64, csrc/mogan_knn.hip) at the memorisation pass's size -- 30 000 queries against a bank of 80 000
training codes, D = 2048, K = 5 -- against the same result formed by torch in fp64 on the device: row blocks of the distance matrix
in Gram form (norms, one fp64 matmul, clamp) and topk(K, largest=False) per block.  The stock formulation holds a (block x N) fp64
matrix in memory and has no rule for equal distances; the kernel writes no distance matrix and orders (d2, position)
lexicographically.  Method of tools/time_prdc.py: hip events, --warmup calls, then --iters timed calls of each path, the two paths
alternating in one process; medians.  A record, not a gate: the capability is the positions, whichever way the ratio falls.  The
torch formulation lives only here.
python tools/time_nn.py [--out profiles/nn_timing.json]"""
import argparse, json, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mogan_loader; mogan_loader.load()
from mogan_amd.hip import ops
ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=6)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--block", type=int, default=2048, help="rows of the distance matrix the torch path holds at a time")
ap.add_argument("--shapes", default="30000x80000x2048x5,2048x8192x2048x5", help="M x N x D x K, comma separated")
ap.add_argument("--out", default="")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("time_nn.py measures on the GPU; none is present")
dev = torch.device("cuda")
SHAPES = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]


def stock(q, p, K, B):
    p64 = p.double()
    npp = (p64 * p64).sum(1)
    d2 = torch.empty((q.shape[0], K), dtype=torch.float64, device=q.device)
    idx = torch.empty((q.shape[0], K), dtype=torch.int64, device=q.device)
    for i in range(0, q.shape[0], B):
        q64 = q[i:i + B].double()
        d = (((q64 * q64).sum(1)[:, None] + npp[None, :]) - 2.0 * (q64 @ p64.t())).clamp_(min=0.0)
        d2[i:i + B], idx[i:i + B] = d.topk(K, dim=1, largest=False, sorted=True)
    return d2, idx


def timed(fn):
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record(); out = fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3, out


result = {"method": "hip events around one call, %d warm-up rounds, %d timed rounds per path, paths alternating in one process, "
                    "medians in microseconds; torch path in row blocks of %d" % (args.warmup, args.iters, args.block),
          "device": torch.cuda.get_device_name(0), "shapes": []}
for M, N, D, K in SHAPES:
    g = torch.Generator(device=dev).manual_seed(N)
    # pool codes are averages of ReLU outputs: non-negative, column scales spread over a decade (tools/time_prdc.py)
    scale = torch.logspace(-1, 0, D, device=dev)
    bank = (torch.randn(N, D, device=dev, generator=g).abs() * scale).contiguous()
    query = (torch.randn(M, D, device=dev, generator=g).abs() * scale * 0.97 + 0.003).contiguous()
    paths = {"kernel": lambda: ops.knn_cross(query, bank, K), "torch_fp64": lambda: stock(query, bank, K, args.block)}
    (d_k, i_k), (d_t, i_t) = paths["kernel"](), paths["torch_fp64"]()
    differing = int((i_k.long() != i_t).sum())
    rel = float(((d_k - d_t).abs() / d_t.clamp_min(1e-300)).max())
    for _ in range(args.warmup):
        for fn in paths.values(): fn()
    torch.cuda.synchronize()
    us = {k: [] for k in paths}
    for _ in range(args.iters):
        for k, fn in paths.items(): us[k].append(timed(fn)[0])
    flop = 2.0 * M * N * D
    row = {"M": M, "N": N, "D": D, "K": K, "positions_that_differ_between_the_paths": differing, "of_positions": int(i_k.numel()),
           "largest_relative_difference_of_the_distances": rel}
    for k in paths:
        row[k + "_us"] = round(statistics.median(us[k]), 1)
        row[k + "_min_us"] = round(min(us[k]), 1)
    row["kernel_over_torch_fp64"] = round(row["kernel_us"] / row["torch_fp64_us"], 3)
    row["kernel_fp64_tflops"] = round(flop / row["kernel_us"] / 1e6, 2)
    row["torch_fp64_distance_matrix_bytes_per_block"] = 8 * min(args.block, M) * N
    result["shapes"].append(row)
    print(row, flush=True)
    del bank, query, d_k, i_k, d_t, i_t
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
