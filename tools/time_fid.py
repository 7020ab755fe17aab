"""The moments of the Frechet distance (ops.feature_moments: mogan_col_mean_f64 + mogan_cov_f64, csrc/mogan_stats.hip) against the same
statistic formed by torch in fp64 on the device (widen, mean, centre, one fp64 matmul for the whole matrix, divide).  Method of
tools/time_retrieval.py: hip events, --warmup calls, then --iters timed calls of each path, the two paths alternating in one process;
medians.  A record, not a gate: the project's kernels are the path whichever way it comes out.  The torch formulation lives only here.
python tools/time_fid.py [--out profiles/fid_timing.json] [--rows 30000]"""
import argparse, json, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mogan_loader; mogan_loader.load()
from mogan_amd.hip import ops
ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--warmup", type=int, default=8)
ap.add_argument("--rows", type=int, default=30000)
ap.add_argument("--out", default="")
args = ap.parse_args()
dev = torch.device("cuda")


def stock(x):
    x64 = x.double()
    mean = x64.mean(0)
    xc = x64 - mean
    return mean, (xc.t() @ xc) / (x.shape[0] - 1)


def timed(fn):
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


result = {"method": "hip events around one call, %d warm-up calls, %d timed calls per path, paths alternating in one process, "
                    "medians in microseconds" % (args.warmup, args.iters), "device": torch.cuda.get_device_name(0), "shapes": []}
for N, D in ((args.rows, 2048),):
    g = torch.Generator(device=dev).manual_seed(N)
    # pool codes are averages of ReLU outputs: non-negative, column scales spread over a decade
    x = (torch.randn(N, D, device=dev, generator=g).abs() * torch.logspace(-1, 0, D, device=dev)).contiguous()
    paths = {"kernel": lambda: ops.feature_moments(x), "torch_fp64": lambda: stock(x)}
    (m0, c0), (m1, c1) = paths["kernel"](), paths["torch_fp64"]()
    apart = float((c0 - c1).abs().max() / c1.abs().max())
    del m0, c0, m1, c1
    for _ in range(args.warmup):
        for fn in paths.values(): fn()
    torch.cuda.synchronize()
    us = {k: [] for k in paths}
    for _ in range(args.iters):
        for k, fn in paths.items(): us[k].append(timed(fn))
    # the covariance kernel alone (the mean is a small share), and the fp64 work it does: the tiles on and above the diagonal
    mean = ops.feature_moments(x)[0]
    cov = torch.empty((D, D), dtype=torch.float64, device=dev)
    only = [timed(lambda: ops.call("mogan_cov_f64", ops.ptr(x), ops.ptr(mean), N, D, ops.ptr(cov), ops.stream_ptr()))
            for _ in range(args.iters)]
    T = (D + 63) // 64
    flop = 2.0 * N * 64 * 64 * (T * (T + 1) // 2)
    row = {"N": N, "D": D, "max_cov_difference_between_the_paths_rel": apart}
    row.update({k + "_us": round(statistics.median(v), 2) for k, v in us.items()})
    row.update({k + "_min_us": round(min(v), 2) for k, v in us.items()})
    row["cov_kernel_alone_us"] = round(statistics.median(only), 2)
    row["cov_kernel_fp64_tflops_on_the_upper_triangle"] = round(flop / statistics.median(only) / 1e6, 2)
    row["panel_bytes_staged_GB"] = round(T * T * N * 64 * 4 / 1e9, 3)      # two 64-column panels per tile, one on the diagonal
    result["shapes"].append(row)
    print(row, flush=True)
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
