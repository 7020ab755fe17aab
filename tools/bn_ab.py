"""Bit comparison of the BatchNorm paths between two builds of the library (csrc/mogan_norm.hip, the deep-block tails of
csrc/mogan_pgemm.hip, csrc/mogan_bn.h).

  MOGAN_LIB=/path/to/libmogan_hip.so python tools/bn_ab.py dump a.npz     # one process per library
  python tools/bn_ab.py dump b.npz
  python tools/bn_ab.py compare a.npz b.npz [--out result.json]

dump runs seeded inputs through every path -- one / two / three launches, BatchNorm1d, batch chunks, grouped (one launch and the
per-group loop), the deferred running-statistics update, the eval affine, the deep-block tail with one and two groups -- and
stores y, mean, invstd, the running statistics, dx, dgamma, dbeta (deep block: z, dy, dx, dw as well).  compare views every array
as integers and asks for equality: the arithmetic order is the same in both builds or it is not, there is no tolerance."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rnd(name, shape, scale=1.0, shift=0.0):
    import zlib
    rng = np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)
    return (rng.standard_normal(tuple(shape)) * scale + shift).astype(np.float32)


def dump(path):
    import torch
    sys.path.insert(0, ROOT)
    import mogan_loader
    mogan_loader.load()
    from mogan_amd.hip import lib, ops
    dev = torch.device("cuda")
    out = {}
    acts = {"none": ops.ACT_NONE, "relu": ops.ACT_RELU, "lrelu": ops.ACT_LRELU, "glu": ops.ACT_GLU}

    def T(name, shape, scale=1.0, shift=0.0):
        return torch.from_numpy(rnd(name, shape, scale, shift)).to(dev)

    def put(key, **tensors):
        for k, v in tensors.items():
            if v is not None:
                out["%s/%s" % (key, k)] = v.detach().cpu().numpy()

    def bn(key, shape, act, groups=1, res=False, defer=False):
        C = shape[1]
        x = T(key + "x", shape, 1.5, 0.3).requires_grad_(True)
        gm, bt = T(key + "g", (C,), 0.2, 1.0).requires_grad_(True), T(key + "b", (C,), 0.2).requires_grad_(True)
        rm, rv = T(key + "rm", (C,), 0.1), T(key + "rv", (C,), 0.1).abs() + 1
        r = T(key + "r", shape).requires_grad_(True) if res else None
        if defer:
            ops.BN_DEFER = pending = []
        try:
            y = ops.bn_act(x, gm, bt, rm, rv, acts[act], 0.2, r, 1e-5, 0.1, groups=groups)
        finally:
            ops.BN_DEFER = None
        if defer:
            ops.bn_apply_deferred(pending)
        stats = y.grad_fn.saved_tensors[3]
        y.backward(T(key + "go", y.shape))
        put(key, y=y, mean=stats[0], invstd=stats[1], running_mean=rm, running_var=rv, dx=x.grad, dgamma=gm.grad, dbeta=bt.grad,
            dres=r.grad if res else None)

    paths = {"one_launch": (4, 8, 8, 8), "one_launch_full": (16, 6, 16, 16), "two_launch": (2, 10, 64, 64),
             "two_launch_tiles": (3, 4, 96, 96), "three_launch": (20, 4, 15, 15), "three_launch_tiny": (5, 4, 3, 3),
             "bn1d": (16, 24), "chunked_two_launch": (66, 2000, 8, 8), "chunked_three_launch": (66, 2000, 3, 3)}
    for name, shape in paths.items():
        for act in acts:
            bn("%s/%s" % (name, act), shape, act)
        bn("%s/none+res" % name, shape, "none", res=True)
    for act in ("none", "lrelu", "glu"):
        bn("deferred/%s" % act, (2, 10, 64, 64), act, defer=True)
        bn("deferred_small/%s" % act, (4, 8, 8, 8), act, defer=True)
        # grouped: one launch (G = 2, G = 3, a BatchNorm1d), and the per-group loop of the large-map kernels
        bn("grouped2/%s" % act, (2 * 16, 12, 15, 15), act, groups=2)
        bn("grouped3/%s" % act, (3 * 4, 6, 8, 8), act, groups=3)
        bn("grouped2_bn1d/%s" % act, (2 * 5, 10), act, groups=2)
        bn("grouped2_loop/%s" % act, (2 * 16, 8, 32, 32), act, groups=2)
        bn("grouped3_loop_odd/%s" % act, (3 * 4, 4, 70, 70), act, groups=3)

    for name, shape in (("affine", (3, 6, 5, 7)), ("affine_chunked", (66, 1000, 3, 3))):
        for act in ("none", "relu", "lrelu"):
            key = "%s/%s" % (name, act)
            x = T(key + "x", shape, 1.5, 0.3).requires_grad_(True)
            y = ops.affine_act(x, T(key + "s", (shape[1],), 0.5, 1.0), T(key + "b", (shape[1],), 0.3), acts[act], 0.2)
            y.backward(T(key + "go", shape))
            put(key, y=y, dx=x.grad)

    # deep block: conv -> BatchNorm(train) -> act with ONE tail kernel each way; split 0 / 3: direct store / the tail sums K-split slabs
    deep = [(16, 64, 8, 8, 64, 4, 2, 1), (16, 32, 16, 16, 96, 4, 2, 1), (3, 64, 4, 4, 96, 3, 1, 1), (32, 32, 16, 16, 32, 4, 2, 1)]
    for groups in (1, 2):
        for ci, (B, Cin, H, W, Cout, k, s, pad) in enumerate(deep):
            if groups * B * ((H + 2 * pad - k) // s + 1) ** 2 > 2048:
                continue
            for act in ("none", "relu", "lrelu"):
                for split in (0, 3):
                    key = "deep_g%d/case%d/%s/split%d" % (groups, ci, act, split)
                    ops.pk_debug_force(1, -1, split)
                    try:
                        x = T(key + "x", (groups * B, Cin, H, W)).requires_grad_(True)
                        w = T(key + "w", (Cout, Cin, k, k), 0.1).requires_grad_(True)
                        gm = T(key + "g", (Cout,), 0.3, 1.0).requires_grad_(True)
                        bt = T(key + "b", (Cout,), 0.2).requires_grad_(True)
                        rm, rv = torch.zeros(Cout, device=dev), torch.ones(Cout, device=dev)
                        ops.attach_packs(w)
                        assert ops.deep_block_eligible(x, w, s, pad, pad, acts[act], groups), key
                        z = ops.deep_conv_bn_act(x, w, gm, bt, rm, rv, acts[act], 0.2, 1e-5, 0.1, s, pad, pad, groups)
                        _, _, y, stats, _, _ = z.grad_fn.saved_tensors
                        dz = T(key + "dz", z.shape)
                        z.backward(dz)
                        # dy, the gradient at the convolution's output, stays inside the backward: the tail kernel once more, by hand
                        dy = torch.empty_like(y)
                        wsp, wsn = lib.workspace(dev)
                        lib.call("mogan_deep_conv_bn_act_bwd", lib.ptr(dz), lib.ptr(y), lib.ptr(stats), lib.ptr(gm), lib.ptr(bt),
                                 None, lib.ptr(dy), None, None, 0, None, groups * B, Cin, H, W, Cout, k, k, s, pad, pad, acts[act], 0.2,
                                 groups, wsp, wsn, lib.stream_ptr())
                        put(key, z=z, mean=stats[0], invstd=stats[1], running_mean=rm, running_var=rv, dy=dy, dx=x.grad, dw=w.grad,
                            dgamma=gm.grad, dbeta=bt.grad)
                    finally:
                        ops.pk_debug_force(0, -1, 0)
    torch.cuda.synchronize()
    np.savez(path, **out)
    print("%d arrays from %s -> %s" % (len(out), lib.LIB_PATH, path))


def compare(a_path, b_path, out_path):
    a, b = np.load(a_path), np.load(b_path)
    assert sorted(a.files) == sorted(b.files), "the two dumps hold different arrays"
    differ = {}
    for k in a.files:
        ia, ib = a[k].view(np.uint32), b[k].view(np.uint32)
        n = int((ia != ib).sum()) if ia.shape == ib.shape else -1
        if n:
            differ[k] = n
    res = {"arrays": len(a.files), "elements": int(sum(a[k].size for k in a.files)), "arrays_differing": len(differ),
           "differing_elements": differ, "bit_identical": not differ}
    print(json.dumps(res))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
    return 0 if not differ else 1


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) >= 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[5] if len(sys.argv) > 5 and sys.argv[4] == "--out" else ""))
    else:
        sys.exit(__doc__)
