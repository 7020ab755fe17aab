"""What the sliced Wasserstein path decides on the host, without a GPU: the ValueErrors of the six ops of hip/ops.py (nothing is
converted or copied for the caller; a legal host tensor reaches the library's "no CPU path" error instead), the levels() rule and
its errors, the centre-range check, the moments check, and the flags of attngan/main.py."""
import numpy as np
import pytest
import torch

from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import swd as SWD  # noqa: E402
from mogan_amd.hip import lib, ops  # noqa: E402


def f32(*shape):
    return torch.zeros(shape, dtype=torch.float32)


def test_levels():
    assert SWD.levels(256) == [256, 128, 64, 32, 16] and SWD.levels(64) == [64, 32, 16] and SWD.levels(16) == [16]
    assert SWD.levels(32, 16) == [32, 16] and SWD.levels(64, 8) == [64, 32, 16, 8] and SWD.levels(28, 7) == [28, 14, 7]
    for size, min_res in ((48, 16), (96, 16), (8, 16), (0, 16), (100, 16), (64, 6), (64, 0), (64, 24), (17, 16), (-64, 16)):
        with pytest.raises(ValueError):
            SWD.levels(size, min_res)


def test_the_centre_range_check():
    ok = np.array([[0, 3, 3], [1, 12, 12], [1, 3, 12]], dtype=np.int32)
    assert SWD.check_centres(ok, 2, 16) is not None
    for bad in ([[0, 2, 3]], [[0, 3, 2]], [[0, 13, 3]], [[0, 3, 13]], [[2, 3, 3]], [[-1, 3, 3]], [[0, -3, 3]]):
        with pytest.raises(ValueError, match="centres outside"):
            SWD.check_centres(np.array(bad, dtype=np.int32), 2, 16)
    with pytest.raises(ValueError):
        SWD.check_centres(np.array([[0, 3, 4]], dtype=np.int32), 1, 7)            # a 7 x 7 level has the one centre (3, 3)
    for bad in (np.zeros((0, 3), np.int32), np.zeros((4,), np.int32), np.zeros((4, 2), np.int32), np.full((4, 3), 3.0)):
        with pytest.raises(ValueError, match="integer"):
            SWD.check_centres(bad, 2, 16)
    # the op checks what it uploads, before it looks for a device
    level, desc = f32(2, 3, 16, 16), f32(10, 147)
    for bad in ([[0, 2, 3]], [[0, 3, 13]], [[2, 3, 3]], [[-1, 3, 3]]):
        with pytest.raises(ValueError, match="centres outside"):
            ops.swd_gather(level, np.array(bad, dtype=np.int64), desc, 0)
    with pytest.raises(lib.MoganHipError, match="no CPU path"):                    # legal centres: only the device is missing
        ops.swd_gather(level, ok.astype(np.int64), desc, 0)


def test_the_moments_check_names_level_and_channel():
    good = np.array([[0.5, 1.0], [2.0, 3.0]])
    assert SWD.check_moments(good, 32, "real") is not None
    for bad in (0.0, np.nan, np.inf, -1.0):
        m = good.copy()
        m[1, 1] = bad
        with pytest.raises(ValueError, match="level 32, channel 1 of the generated images"):
            SWD.check_moments(m, 32, "generated")
    m = good.copy()
    m[0, 0] = np.nan
    with pytest.raises(ValueError, match="level 16, channel 0 of the real images"):
        SWD.check_moments(m, 16, "real")


def test_the_class_checks_its_arguments():
    for kw in (dict(channels=2), dict(channels=4), dict(patches=0), dict(dirs=0), dict(dirs=1025), dict(repeats=0),
               dict(rows=12), dict(rows=0), dict(size=48), dict(min_res=5)):
        args = dict(size=32, channels=3, rows=16, patches=8, dirs=4, repeats=1, min_res=16, seed=1, device="cpu")
        args.update(kw)
        with pytest.raises(ValueError):
            SWD.SlicedWasserstein(**args)
    sw = SWD.SlicedWasserstein(32, 3, 16, patches=8, dirs=4, repeats=1, min_res=16, seed=1, device="cpu")
    img = f32(2, 3, 32, 32)
    for real, fake in ((img.double(), img), (img, img.half()), (img[0], img), (img, f32(2, 1, 32, 32)), (img, f32(2, 3, 16, 16)),
                       (img, f32(1, 3, 32, 32)), (img.transpose(2, 3), img),
                       (img.numpy(), img), (f32(3, 3, 32, 32), f32(3, 3, 32, 32))):
        with pytest.raises(ValueError):
            sw.add(real, fake)
    with pytest.raises(ValueError, match="no images"):
        sw.result()
    bad = {"real": [np.array([[0, 3, 3]] * 16), np.array([[0, 3, 13]] * 16)], "fake": [np.array([[0, 3, 3]] * 16)] * 2}
    with pytest.raises(ValueError, match="centres outside"):
        sw.add(img, img, centres=bad)
    with pytest.raises(ValueError, match="per level"):
        sw.add(img, img, centres={"real": bad["fake"][:1], "fake": bad["fake"]})
    assert sw.n == 0


def test_the_ops_raise_valueerror_and_convert_nothing():
    x, d = f32(6, 16, 16), f32(6, 8, 8)
    for bad in (x.double(), x.half(), x[0], x.view(2, 3, 16, 16), x[:, :, ::2], x.transpose(1, 2), f32(6, 15, 16), f32(6, 16, 6)[:, :, :5],
                f32(6, 2, 16), f32(6, 16, 2), x.numpy(), None, torch.zeros((0, 16, 16))):
        with pytest.raises(ValueError):
            ops.pyr_down(bad)
        with pytest.raises(ValueError):
            ops.lap_residual(bad, d)
    for bad in (d.double(), d[0], f32(6, 8, 4), f32(5, 8, 8), f32(6, 16, 16)[:, ::2, ::2], d.numpy(), None):
        with pytest.raises(ValueError):
            ops.lap_residual(x, bad)
    level, desc, tri = f32(2, 3, 16, 16), f32(10, 147), np.array([[0, 3, 3], [1, 12, 12]], dtype=np.int32)
    for lv, t, ds, row0 in ((level.double(), tri, desc, 0), (level[0], tri, desc, 0), (f32(2, 5, 16, 16), tri, f32(10, 245), 0),
                            (f32(2, 3, 6, 16), tri, desc, 0), (f32(2, 3, 16, 6), tri, desc, 0), (level[:, :, :, ::2], tri, desc, 0),
                            (level, tri, f32(10, 49), 0), (level, tri, desc.double(), 0), (level, tri, desc[:, ::1].t(), 0),
                            (level, tri, f32(10, 3, 49), 0), (level, tri, desc, 9), (level, tri, desc, -1), (level, tri, desc, 10),
                            (level, tri[:, :2], desc, 0), (level, tri.astype(np.float32), desc, 0), (level, tri[:0], desc, 0),
                            (level, tri.tolist(), desc, 0), (level, torch.from_numpy(tri).long(), desc, 0),
                            (level, torch.from_numpy(tri).t().contiguous().t(), desc, 0)):
        with pytest.raises(ValueError):
            ops.swd_gather(lv, t, ds, row0)
    mom, dirs = torch.zeros((3, 2), dtype=torch.float64), f32(147, 5)
    for bad in (desc.double(), desc[0], f32(10, 50), f32(10, 245), f32(10, 294)[:, ::2], desc.numpy(), f32(0, 147)):
        with pytest.raises(ValueError):
            ops.swd_moments(bad)
        with pytest.raises(ValueError):
            ops.swd_project(bad, mom, dirs)
    for m, v in ((mom.float(), dirs), (mom[:2], dirs), (mom.t().contiguous().t(), dirs), (mom.view(6), dirs), (mom.numpy(), dirs),
                 (mom, dirs.double()), (mom, f32(49, 5)), (mom, f32(147, 1025)), (mom, f32(147, 10)[:, ::2]), (mom, dirs[:, :0]),
                 (mom, f32(5, 147).t()), (mom, None)):
        with pytest.raises(ValueError):
            ops.swd_project(desc, m, v)
    a = f32(3, 100)
    for p, q in ((a.double(), a), (a, a.half()), (a[0], a[0]), (a, f32(3, 99)), (a, f32(2, 100)), (f32(1025, 4), f32(1025, 4)),
                 (a[:, ::2], a[:, ::2]), (a.t(), a.t()), (a.numpy(), a), (a, None), (f32(0, 4), f32(0, 4))):
        with pytest.raises(ValueError):
            ops.swd_absdiff(p, q)
    # legal host tensors: nothing left to object to but the device -- there is no CPU path
    for call in (lambda: ops.pyr_down(x), lambda: ops.lap_residual(x, d), lambda: ops.swd_moments(desc),
                 lambda: ops.swd_project(desc, mom, dirs), lambda: ops.swd_absdiff(a, a.clone())):
        with pytest.raises(lib.MoganHipError, match="no CPU path"):
            call()


def test_main_knows_the_flags():
    from mogan_amd.attngan import main as entry
    args = entry.parse_args(["--swd"])
    assert args.swd and (args.swd_patches, args.swd_dirs, args.swd_repeats, args.swd_min_res) == (128, 128, 4, 16)
    args = entry.parse_args(["--swd", "--fid", "--swd_patches", "8", "--swd_dirs", "16", "--swd_repeats", "2", "--swd_min_res", "32"])
    assert args.fid and (args.swd_patches, args.swd_dirs, args.swd_repeats, args.swd_min_res) == (8, 16, 2, 32)
    assert not entry.parse_args([]).swd
    for other in ("--sampling", "--r_precision"):
        with pytest.raises(SystemExit):
            entry.parse_args(["--swd", other])
