"""The rejections of the radial-power-spectrum path, as tests/test_msssim_rejections_cpu.py does for MS-SSIM: the two entries of
csrc/mogan_spectrum.hip answer every case on the host BEFORE any HIP call, so the table runs without a GPU -- the pointers are dummies
that are never dereferenced (-1 = MOGAN_ERR_SHAPE, -3 = MOGAN_ERR_WS; that the limits themselves pass both gates shows as
MOGAN_ERR_LAUNCH where no GPU is present); the size query is held to its closed form; hip/ops.radial_power, attngan/spectrum.py,
RadialSpectrum and CheckpointEvaluation.spectrum's hand-over check raise their ValueErrors before anything touches a device; and
main.py parses the two new flags."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import spectrum as SP  # noqa: E402
from mogan_amd.hip import lib, ops  # noqa: E402

PTR = [ctypes.c_void_p(v) for v in (256, 512, 1024, 2048, 4096, 8192, 16384)]     # non-null, aligned, never dereferenced
NULL = ctypes.c_void_p(None)
SHAPE, LAUNCH, WS = -1, -2, -3


def L():
    return lib.load()


def ws_bytes(B, S):
    return int(L().mogan_radial_power_ws_bytes(B, S))


def closed_form(B, S):
    """min(B, 64) ((S / 2 + 1) S 16 + G 2048), G = ceil((S / 2 + 1) / min(S / 2 + 1, 2048 / S)) column groups"""
    V = S // 2 + 1
    cols = min(V, 2048 // S)
    return min(B, 64) * (V * S * 16 + -(-V // cols) * 2048)


def power(x=PTR[0], weight=PTR[1], window=PTR[2], twiddle=PTR[3], bins=PTR[4], out=PTR[5], ws=PTR[6], ws_size=None, B=5, C=3, S=64,
          n_bins=47):
    if ws_size is None:
        ws_size = max(ws_bytes(B, S), 1 << 20)
    return L().mogan_radial_power_f64(x, B, C, S, weight, window, twiddle, bins, n_bins, out, ws, ws_size, NULL)


TABLE = [("NULL x", dict(x=NULL)), ("NULL weight", dict(weight=NULL)), ("NULL twiddle", dict(twiddle=NULL)), ("NULL bins", dict(bins=NULL)),
         ("NULL out", dict(out=NULL)), ("a twiddle table off 16 bytes", dict(twiddle=ctypes.c_void_p(1032))),
         ("an out off 8 bytes", dict(out=ctypes.c_void_p(8196))), ("B = 0", dict(B=0)), ("B < 0", dict(B=-1)),
         ("C = 0", dict(C=0)), ("C = 5", dict(C=5)), ("C < 0", dict(C=-3)), ("S = 4", dict(S=4)), ("S = 512", dict(S=512)),
         ("S = 0", dict(S=0)), ("S < 0", dict(S=-64)), ("S = 48", dict(S=48)), ("S = 100", dict(S=100)), ("S = 255", dict(S=255)),
         ("S = 2^30", dict(S=1 << 30)), ("n_bins = 0", dict(n_bins=0)), ("n_bins < 0", dict(n_bins=-1)), ("n_bins = 257", dict(n_bins=257)),
         ("B C S S = 2^31", dict(B=1 << 13, C=4, S=256)),
         ("a bad shape with a NULL workspace is a shape error", dict(C=0, ws=NULL, ws_size=0))]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


@pytest.mark.parametrize("kw", [t[1] for t in TABLE], ids=[t[0] for t in TABLE])
def test_rejects_shapes_before_any_launch(kw):
    assert power(**kw) == SHAPE


@pytest.mark.parametrize("kw", [dict(ws=NULL), dict(ws=NULL, ws_size=0), dict(ws_size=0), dict(ws=ctypes.c_void_p(264)),
                                dict(ws_size=closed_form(5, 64) - 1)],
                         ids=["NULL ws", "NULL ws of size 0", "size 0", "misaligned ws", "one byte short"])
def test_rejects_a_missing_workspace_before_any_launch(kw):
    assert power(**kw) == WS


def test_the_signatures_are_the_headers():
    P, I, Z = lib.P, lib.I, lib.Z
    assert lib.SIGNATURES["mogan_radial_power_ws_bytes"] == [I, I]
    assert lib.SIGNATURES["mogan_radial_power_f64"] == [P, I, I, I, P, P, P, P, I, P, P, Z, P]
    assert L().mogan_radial_power_ws_bytes.restype is ctypes.c_size_t
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mogan_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    kinds = {"mogan_radial_power_ws_bytes": (r"size_t", ["int", "int"]),
             "mogan_radial_power_f64": (r"int", ["const float*", "int", "int", "int", "const float*", "const float*", "const double*",
                                                 "const int*", "int", "double*", "void*", "size_t", "hipStream_t"])}
    as_ctypes = {"int": I, "size_t": Z}
    for name, (ret, params) in kinds.items():
        m = re.search(r"\b%s\s+%s\s*\(([^;]*?)\)\s*;" % (ret, name), header, flags=re.S)
        assert m, name
        got = [re.sub(r"\s*\b\w+$", "", p.strip()).replace(" *", "*") for p in m.group(1).split(",")]
        assert got == params, (name, got)
        assert lib.SIGNATURES[name] == [as_ctypes.get(p, P) for p in params]


def test_ws_bytes_follow_their_closed_form_and_are_0_for_illegal_arguments():
    for B in (1, 2, 5, 16, 63, 64, 65, 1000, 30000):
        for S in (8, 16, 32, 64, 128, 256):
            assert ws_bytes(B, S) == closed_form(B, S), (B, S)
    assert ws_bytes(1, 8) == 5 * 8 * 16 + 2048 and ws_bytes(16, 256) == 16 * (129 * 256 * 16 + 17 * 2048)
    assert ws_bytes(30000, 256) == ws_bytes(64, 256)                 # bounded whatever the batch
    for B, S in ((0, 64), (-1, 64), (5, 4), (5, 512), (5, 48), (5, 0), (5, -8), (5, 255)):
        assert ws_bytes(B, S) == 0, (B, S)


@pytest.mark.skipif(torch.cuda.is_available(), reason="dummy pointers must never reach a real launch")
def test_the_largest_accepted_sizes_pass_the_gates():
    assert power() == LAUNCH and power(window=NULL) == LAUNCH and power(B=1, C=1, S=8, n_bins=1) == LAUNCH
    assert power(C=4, S=256, n_bins=256) == LAUNCH and power(B=(1 << 13) - 1, C=4, S=256) == LAUNCH
    assert power(ws_size=closed_form(5, 64)) == LAUNCH


def _args(S=16, B=2, C=3):
    table, count = SP.radial_bins(S)
    return (torch.zeros(B, C, S, S), torch.from_numpy(SP.channel_weights(C)), torch.from_numpy(SP.hann(S)), torch.from_numpy(table),
            len(count))


def test_the_op_refuses_what_it_would_have_to_convert():
    x, w, win, bins, n = _args()
    bad = [(x.double(), w, win, bins, n), (x[0], w, win, bins, n), (x[:, :, :, ::2], w, win, bins, n), (x.numpy(), w, win, bins, n),
           (torch.zeros(2, 3, 16, 8), w, win, bins, n), (torch.zeros(2, 3, 4, 4), w, win, bins, n), (torch.zeros(2, 3, 24, 24), w, win, bins, n),
           (torch.zeros(1, 3, 512, 512), w, win, bins, n), (torch.zeros(2, 5, 16, 16), torch.ones(5), win, bins, n),
           (x, w.double(), win, bins, n), (x, w[:2], win, bins, n), (x, w.view(1, 3), win, bins, n), (x, torch.ones(6)[::2], win, bins, n),
           (x, w, win.double(), bins, n), (x, w, win[:8], bins, n), (x, w, torch.ones(32)[::2], bins, n), (x, w, win.numpy(), bins, n),
           (x, w, win, bins.long(), n), (x, w, win, bins[:, :8], n), (x, w, win, bins.t().contiguous().t(), n), (x, w, win, bins.numpy(), n),
           (x, w, win, bins[:8], n), (x, w, win, bins, 0), (x, w, win, bins, 257), (x, w, win, bins, -1),
           (x, w.to("meta"), win, bins, n), (x, w, win.to("meta"), bins, n), (x, w, win, bins.to("meta"), n), (x.to("meta"), w.to("meta"),
                                                                                                           win.to("meta"), bins.to("meta"), n)]
    for args in bad:
        with pytest.raises(ValueError, match="radial_power"):
            ops.radial_power(*args)
    for out in (torch.zeros(2, n), torch.zeros(3, n, dtype=torch.float64), torch.zeros(2, 2 * n, dtype=torch.float64)[:, ::2],
                torch.zeros(2, n, dtype=torch.float64, device="meta"), np.zeros((2, n))):
        with pytest.raises(ValueError, match="radial_power"):
            ops.radial_power(x, w, win, bins, n, out=out)
    # legal host tensors: nothing left to object to but the device -- there is no CPU path
    with pytest.raises(lib.MoganHipError, match="no CPU path"):
        ops.radial_power(x, w, win, bins, n)
    with pytest.raises(lib.MoganHipError, match="no CPU path"):
        ops.radial_power(x, w, None, bins, n, out=torch.zeros(2, n, dtype=torch.float64))
    tw = ops.twiddle_table(16)
    k = np.arange(8)
    assert tw.dtype == np.float64 and tw.shape == (8, 2) and tw.flags["C_CONTIGUOUS"]
    assert np.array_equal(tw[:, 0], np.cos(2 * np.pi * k / 16)) and np.array_equal(tw[:, 1], -np.sin(2 * np.pi * k / 16))


def test_the_definitions_value_errors():
    for size in (0, 4, 7, 24, 100, 512, -8):
        for fn in (SP.check_size, SP.hann, SP.radial_bins):
            with pytest.raises(ValueError, match="power of two"):
                fn(size)
    for C in (0, 2, 4, 5, -1):
        with pytest.raises(ValueError, match="1 or 3 channels"):
            SP.channel_weights(C)
    for w in ("hamming", "", 3, "Hann"):
        with pytest.raises(ValueError, match="window"):
            SP.window_name(w)
    with pytest.raises(ValueError, match="window of 16"):
        SP.window_energy(np.ones(8, np.float32), 16)
    _, count = SP.radial_bins(16)
    p = np.ones(len(count))
    for args in ((p, p[:-1], count, 16), (p, p, count[:-1], 16), (p[:, None], p[:, None], count, 16), (p, p * np.nan, count, 16),
                 (p, -p, count, 16), (p * 0, p, count, 16), (p[:1], p[:1], count[:1], 16)):
        with pytest.raises(ValueError, match="spectrum"):
            SP.figures(*args)
    with pytest.raises(ValueError, match="power of two"):
        SP.figures(p, p, count, 17)
    s = np.ones((3, len(count)))
    for args in ((s[0], count, 1.0), (s, count[:-1], 1.0), (s, count * 0, 1.0), (s, count, 0.0), (-s, count, 1.0), (s * np.inf, count, 1.0),
                 (s[:0], count, 1.0)):
        with pytest.raises(ValueError, match="spectrum"):
            SP.profiles(*args)


def test_the_accumulators_value_errors_come_before_any_device_call():
    for kw in (dict(size=48), dict(size=512), dict(channels=2), dict(channels=4), dict(images=0), dict(window="hamming")):
        with pytest.raises(ValueError, match="spectrum"):
            SP.RadialSpectrum(**dict(dict(size=16, channels=3, images=4, device="cpu"), **kw))
    acc = SP.RadialSpectrum(16, 3, 4, window=None, seed=7, device="cpu")
    assert (acc.window, acc.seed, acc.n, acc.n_bins, acc.win) == ("none", 7, 0, len(SP.radial_bins(16)[1]), None)
    assert tuple(acc.sums["real"].shape) == (4, acc.n_bins) and acc.sums["fake"].dtype == torch.float64
    x = torch.zeros(2, 3, 16, 16)
    for real, fake in ((x.double(), x), (x, x.half()), (x[0], x[0]), (x[:, :, :, ::2], x[:, :, :, ::2]), (x.numpy(), x), (x, x[:1]),
                       (torch.zeros(2, 1, 16, 16), torch.zeros(2, 1, 16, 16)), (torch.zeros(2, 3, 32, 32), torch.zeros(2, 3, 32, 32)),
                       (x[:0], x[:0]), (x.to("meta"), x.to("meta")), (torch.zeros(5, 3, 16, 16), torch.zeros(5, 3, 16, 16))):
        with pytest.raises(ValueError, match="spectrum"):
            acc.add(real, fake)
    assert acc.n == 0
    with pytest.raises(ValueError, match="no images"):
        acc.result()
    with pytest.raises(lib.MoganHipError, match="no CPU path"):       # legal host tensors: only the device is left to object to
        acc.add(x, x)
    assert acc.n == 0


def test_spectrum_refuses_an_accumulator_of_another_seed_or_window():
    from mogan_amd.attngan.evaluate import CheckpointEvaluation
    from mogan_amd.attngan.miscc.config import cfg
    ev = CheckpointEvaluation()
    acc = SP.RadialSpectrum(16, 3, 4, window="hann", seed=100, device="cpu")
    keep = cfg.TRAIN.NET_G
    cfg.TRAIN.NET_G = "nowhere/netG.pth"
    try:
        for kw in (dict(seed=101), dict(window="none"), dict(window=None)):
            with pytest.raises(ValueError, match="other parameters"):
                ev.spectrum("test", **dict(dict(seed=100, window="hann", images=acc), **kw))
        with pytest.raises(ValueError, match="window must be"):
            ev.spectrum("test", seed=100, window="hamming", images=acc)
        with pytest.raises(ValueError, match="no batch"):               # the right parameters: only the empty pass is left
            ev.spectrum("test", seed=100, window="hann", images=acc)
    finally:
        cfg.TRAIN.NET_G = keep
    assert ev.spectrum("test") is None                                  # no NET_G: the guard of every evaluation path


def test_main_parses_the_flags():
    from mogan_amd.attngan import main as entry
    a = entry.parse_args([])
    assert a.spectrum is False and a.spectrum_window == "hann"
    a = entry.parse_args(["--spectrum", "--spectrum_window", "none", "--swd", "--msssim", "--fid", "--kid", "--prdc", "--scene_fid",
                          "--memorisation"])
    assert a.spectrum and a.spectrum_window == "none" and a.swd and a.msssim and a.memorisation
    for bad in (["--spectrum", "--sampling"], ["--spectrum", "--r_precision"], ["--spectrum_window", "hamming"], ["--spectrum_window"]):
        with pytest.raises(SystemExit):
            entry.parse_args(bad)
