"""Bit comparison of the fp64 Gram-tile kernels between two builds of the library (csrc/mogan_gram64.h and its callers
csrc/mogan_stats.hip, csrc/mogan_mmd.hip, csrc/mogan_knn.hip).

  MOGAN_LIB=/path/to/libmogan_hip.so python tools/gram_ab.py dump a.npz     # one process per library
  python tools/gram_ab.py dump b.npz
  python tools/gram_ab.py compare a.npz b.npz [--out result.json]

dump runs seeded inputs through ops.feature_moments, ops.poly_mmd_sums, ops.knn_sqdist and ops.ball_counts (both sides) and stores
every output.  The shapes are those of tests/fid_cases.py, tests/kid_cases.py and tests/prdc_cases.py, CASES and EXACT_CASES -- the
smallest at which tails, diagonal tiles, three tile rows and D tails occur -- plus, per entry point, a few hundred rows at the
workload's D = 2048 (the vector loads at full width) and one input that is a view one float past a 16-byte boundary with
D % 4 == 0 (the scalar loads at an aligned-looking D).  The radii given to ball_counts are formed on the host in numpy fp64, so
they do not depend on the library.  compare views every array as integers and asks for equality: the scores are decisions and the
arithmetic order is the same in both builds or it is not, there is no tolerance."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WIDE_FID = (300, 2048)
WIDE_KID = (2, 200, 2048, 300, 260)
WIDE_PRDC = (300, 260, 2048, 5)
OFFSET_FID = (67, 80)
OFFSET_KID = (3, 67, 80, 100, 90)
OFFSET_PRDC = (67, 100, 80, 5)


def dump(path):
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mogan_loader
    mogan_loader.load()
    import fid_cases
    import kid_cases
    import prdc_cases
    from mogan_amd.hip import lib, ops
    dev = torch.device("cuda")
    out = {}

    def up(a, offset=False):
        """the array on the device; offset: as a contiguous view that starts one float past a 16-byte boundary"""
        t = torch.from_numpy(np.ascontiguousarray(a))
        if not offset:
            return t.to(dev)
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
        assert buf.data_ptr() % 16 == 0
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v

    def put(key, **tensors):
        for k, v in tensors.items():
            out["%s/%s" % (key, k)] = v.detach().cpu().numpy()

    def fid(key, x, offset=False):
        mean, cov = ops.feature_moments(up(x, offset))
        put(key, mean=mean, cov=cov)

    def kid(key, x, y, ix, iy, gamma, offset=False):
        put(key, sums=ops.poly_mmd_sums(up(x, offset), up(y, offset), ix, iy, gamma))

    def prdc(key, case, x, y, offset=False):
        N, M, D, K = case
        dx, dy = up(x, offset), up(y, offset)
        sets, k_of, given = {"x": dx, "y": dy}, {"x": K, "y": min(K, M - 1)}, {}
        for s, a in (("x", x), ("y", y)):
            if k_of[s] < 1:
                continue
            put(key, **{"radii_" + s: ops.knn_sqdist(sets[s], k_of[s])})
            r2, _ = prdc_cases.knn_of(prdc_cases.numpy_fp64_d2(a, a), k_of[s])
            given[s] = up(r2[:, [k - 1 for k in prdc_cases.ks(k_of[s])]])
        for i, (_, q, p, of, side) in enumerate(prdc_cases.problems(case)):
            put(key, **{"count_%d_%s_in_%s_radii_%s_%s" % (i, q, p, of, side): ops.ball_counts(sets[q], sets[p], given[of], side)})

    for shape, seed in fid_cases.CASES.items():
        fid("fid/%dx%d" % shape, fid_cases.make_inputs(shape, seed))
    for shape, seed in fid_cases.EXACT_CASES.items():
        fid("fid_exact/%dx%d" % shape, fid_cases.make_exact_inputs(shape, seed))
    fid("fid_wide/%dx%d" % WIDE_FID, fid_cases.make_inputs(WIDE_FID, 2))
    fid("fid_offset/%dx%d" % OFFSET_FID, fid_cases.make_inputs(OFFSET_FID, 3), offset=True)

    for case, seed in kid_cases.CASES.items():
        x, y = kid_cases.make_inputs(case, seed)
        ix, iy = kid_cases.make_indices(case, seed)
        kid("kid/%d_%d_%d_%d_%d" % case, x, y, ix, iy, kid_cases.gamma_of(case))
    for case, seed in kid_cases.EXACT_CASES.items():
        kid("kid_exact/%d_%d_%d_%d_%d" % case[:5], *kid_cases.make_exact_inputs(case, seed))
    for name, case, seed, offset in (("kid_wide", WIDE_KID, 2, False), ("kid_offset", OFFSET_KID, 3, True)):
        x, y = kid_cases.make_inputs(case, seed)
        ix, iy = kid_cases.KIDMOD.draw_subsets(case[3], case[4], case[0], case[1], seed)
        kid("%s/%d_%d_%d_%d_%d" % ((name,) + case), x, y, ix, iy, kid_cases.gamma_of(case), offset)

    for case, seed in prdc_cases.CASES.items():
        prdc("prdc/%d_%d_%d_%d" % case, case, *prdc_cases.make_inputs(case, seed))
    for case, seed in prdc_cases.EXACT_CASES.items():
        prdc("prdc_exact/%d_%d_%d_%d" % case, case, *prdc_cases.make_exact_inputs(case, seed))
    prdc("prdc_wide/%d_%d_%d_%d" % WIDE_PRDC, WIDE_PRDC, *prdc_cases.make_inputs(WIDE_PRDC, 2))
    prdc("prdc_offset/%d_%d_%d_%d" % OFFSET_PRDC, OFFSET_PRDC, *prdc_cases.make_inputs(OFFSET_PRDC, 3), offset=True)

    torch.cuda.synchronize()
    np.savez(path, **out)
    print("%d arrays from %s -> %s" % (len(out), lib.LIB_PATH, path))


def compare(a_path, b_path, out_path):
    a, b = np.load(a_path), np.load(b_path)
    assert sorted(a.files) == sorted(b.files), "the two dumps hold different arrays"
    differ = {}
    for k in a.files:
        ia, ib = (v.view("u%d" % v.dtype.itemsize) for v in (a[k], b[k]))
        n = int((ia != ib).sum()) if ia.shape == ib.shape and ia.dtype == ib.dtype else -1
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
