"""-m gpu: the pool modes of mogan_panel_tail_group that the published FID network needs (csrc/mogan_panel.hip, MoganTailArgs.box = 2:
the mean of the taps inside the map, box = 3: their maximum), per element and in guarded memory.

Every call writes an fp32 slice of a wider parent and a panel slice behind a foreign channel group, both between guard bands
(tests/memguard.py): nothing outside the slices may change, the panel must decode to the fp32 values, its pad channels must be zero.
Maps 1x1, 2x2, 2x3, 8x8, 8x17 with B = 3 and C = 33, 40: a partial channel group and a partial block of 64 pixels, one block and several.

Bounds (none comes from the code under test):
  * box = 3 is exact: a maximum rounds nothing.  Bit-equal to F.max_pool2d(x, 3, 1, 1) of the same fp32 values.
  * box = 2 against fp64 avg_pool2d(count_include_pad=False): 10 * 2^-24 * sum |taps| / count (trunk_variant_cases.MEAN_BOUND: at most
    seven additions per tap with two slabs, and one division).  The share of the bound that is used is printed.
  * a map holding one constant whose ninefold sum is exact comes out bit for bit constant (the division is a true one).
NaN inputs are out of scope, as tests/pool_cases.py says for the max-pool."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import memguard as G
import trunk_variant_cases as V
from deep_cases import _panel_decode, _run_tail, _tail_member
from helpers import load_pkg

load_pkg()
from mogan_amd.hip import lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = 3
MAPS = [(1, 1), (2, 2), (2, 3), (8, 8), (8, 17)]
CHANNELS = [33, 40]
CASES = [(C, H, W) for C in CHANNELS for H, W in MAPS]
FRONT, BEHIND = 3, 4                 # foreign channels of the fp32 parent in front of and behind the slice


def _ids(c):
    return "C%d_%dx%d" % c


def _rand(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g)


class Outputs:
    """the guarded fp32 slice and the guarded panel slice (behind one foreign group of 32 channels) of one member"""

    def __init__(self, C, H, W):
        self.C, self.H, self.W, self.Q = C, H, W, B * H * W
        self.ng = (C + 31) // 32
        self.Cp = (self.ng + 1) * 32
        self.dst = G.Guarded((B, FRONT + C + BEHIND, H, W), (slice(None), slice(FRONT, FRONT + C)), DEV)
        self.panel = G.Guarded((self.Q, self.ng + 1, 192), (slice(None), slice(1, self.ng + 1)), DEV, dtype=torch.uint8)

    def member(self, srcs, **kw):
        return _tail_member(B, self.C, self.H, self.W, srcs, dst=self.dst.ptr, dst_bs=self.dst.bstride,
                            panel=self.panel.parent.data_ptr(), Cp=self.Cp, c0=32, **kw)

    def check(self, expect, what, atol=None, exact=False):
        """the fp32 slice against `expect`; the panel decodes to the fp32 values with zero pad channels; nothing else changed"""
        self.dst.check(expect, atol=atol, exact=exact, what=what + ": fp32 slice")
        self.panel.check(written=False, what=what + ": panel")
        # (decoding the foreign group's sentinel bytes gives NaNs: only the slice's columns are read)
        dec = _panel_decode(self.panel.parent.contiguous().view(-1), self.Q, self.Cp)[:, 32:]
        got = self.dst.view.permute(0, 2, 3, 1).reshape(self.Q, self.C)
        assert torch.equal(dec[:, :self.C].view(torch.int32), got.contiguous().view(torch.int32)), what + ": the panel does not decode to the fp32 values"
        if self.ng * 32 > self.C:
            assert float(dec[:, self.C:].abs().max()) == 0.0, what + ": pad channels of the panel must be zero"

    def untouched(self):
        return self.dst.untouched() and self.panel.untouched()


def _src(x):
    """a dense (B, C, H, W) tensor, or slabs (S, B, C, H, W), as a tail source"""
    if x.dim() == 4:
        return (x.data_ptr(), x.stride(0), 0, 1)
    return (x.data_ptr(), x.stride(1), x.stride(0), x.shape[0])


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_mode_3_is_max_pool2d_bit_for_bit(case):
    C, H, W = case
    for what, x in (("random", _rand((B, C, H, W), 100 + C + H * W)),
                    ("all negative", -_rand((B, C, H, W), 200 + C + H * W).abs() - 1.0)):      # zero padding would win everywhere
        xd = x.to(DEV)
        frozen = G.Frozen(xd)
        out = Outputs(C, H, W)
        _run_tail([out.member([_src(xd)], box=3)])
        torch.cuda.synchronize()
        want = F.max_pool2d(x, 3, 1, 1)
        if what == "all negative":
            assert float(want.max()) < 0.0
        out.check(want, "box 3, %s %s" % (what, case), exact=True)
        frozen.check("box 3")


def test_mode_3_takes_the_affine_and_the_relu_after_the_maximum():
    C, H, W = 40, 8, 17
    x = _rand((B, C, H, W), 7)
    sc, sh = _rand((C,), 8) * 0.5 + 1.0, _rand((C,), 9) * 0.3
    xd, scd, shd = x.to(DEV), sc.to(DEV), sh.to(DEV)
    out = Outputs(C, H, W)
    _run_tail([out.member([_src(xd)], box=3, scale=scd.data_ptr(), shift=shd.data_ptr(), relu=1)])
    torch.cuda.synchronize()
    # one fp32 multiply-add (fused) on exact inputs, then a maximum with zero: fp32's own fma, bit for bit
    m = F.max_pool2d(x, 3, 1, 1).double()
    want = (m * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)).float().clamp_min(0)      # fp64 product + sum, rounded once
    out.check(want, "box 3 + affine + relu", atol=(m.abs() * sc.abs().view(1, -1, 1, 1) + sh.abs().view(1, -1, 1, 1)) * 2 * V.U)


@pytest.mark.parametrize("slabs", [1, 2])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_mode_2_is_the_mean_of_the_taps_inside_the_map(case, slabs):
    C, H, W = case
    x = _rand((slabs, B, C, H, W), 300 + 10 * slabs + C + H * W)
    xd = x.to(DEV)
    out = Outputs(C, H, W)
    _run_tail([out.member([_src(xd)], box=2)])
    torch.cuda.synchronize()
    want, mag = V.valid_mean(x.double())
    bound = V.MEAN_BOUND * mag
    used = float(((out.dst.view.cpu().double() - want).abs() / bound).max())
    print("box 2 %s, %d slab(s): %.3f of the bound 10 u sum|taps| / count is used" % (case, slabs, used))
    out.check(want, "box 2 %s x %d" % (case, slabs), atol=bound)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_mode_2_keeps_a_constant_map_constant_bit_for_bit(case):
    C, H, W = case
    c = float(torch.tensor(0.3).bfloat16())                 # 8 significant bits: every k * c, k <= 9, is exact in fp32
    assert float(torch.tensor(c * 9.0, dtype=torch.float32)) == c * 9.0
    x = torch.full((B, C, H, W), c)
    out = Outputs(C, H, W)
    _run_tail([out.member([_src(x.to(DEV))], box=2)])
    torch.cuda.synchronize()
    out.check(x, "box 2, constant map %s" % (case,), exact=True)


def test_a_group_mixing_mode_1_and_mode_2_gives_each_member_its_own_result():
    C, H, W = 40, 8, 17
    x = _rand((B, C, H, W), 11)
    xd = x.to(DEV)
    one, two, none, top = (Outputs(C, H, W) for _ in range(4))
    _run_tail([one.member([_src(xd)], box=1), two.member([_src(xd)], box=2), none.member([_src(xd)]), top.member([_src(xd)], box=3)])
    torch.cuda.synchronize()
    want2, mag2 = V.valid_mean(x.double()[None])
    # mode 1: the same sum (four roundings per tap with one slab), the rounding of the constant 1 / 9 and of the product
    want1, mag1 = F.avg_pool2d(x.double(), 3, 1, 1), F.avg_pool2d(x.double().abs(), 3, 1, 1)
    one.check(want1, "mixed group, box 1", atol=V.MEAN_BOUND * mag1)
    two.check(want2, "mixed group, box 2", atol=V.MEAN_BOUND * mag2)
    none.check(x, "mixed group, box 0", exact=True)
    top.check(F.max_pool2d(x, 3, 1, 1), "mixed group, box 3", exact=True)
    inner = (slice(None), slice(None), slice(1, H - 1), slice(1, W - 1))
    a, b = one.dst.view.cpu(), two.dst.view.cpu()
    assert float((a[inner].double() - b[inner].double()).abs().max()) <= float((2 * V.MEAN_BOUND * mag1[inner]).max())
    assert float((a[:, :, 0].double() * 1.5 - b[:, :, 0].double())[:, :, 1:-1].abs().max()) <= 1e-5       # six taps of nine on an edge


def _rc(members):
    arr = (lib.TailArgs * len(members))(*members)
    return lib.load().mogan_panel_tail_group(len(members), ctypes.cast(arr, ctypes.c_void_p), ctypes.c_void_p(lib.stream_ptr()))


def test_rejections_write_nothing():
    C, H, W = 33, 8, 8
    xd = _rand((2, B, C, H, W), 13).to(DEV)
    out, good = Outputs(C, H, W), Outputs(C, H, W)
    one = (xd.data_ptr(), xd.stride(1), 0, 1)
    for what, members in (("box 4", [out.member([one], box=4)]), ("box -1", [out.member([one], box=-1)]),
                          ("box 3, two sources", [out.member([one, one], box=3)]),
                          ("box 3, two slabs", [out.member([_src(xd)], box=3)]),
                          ("a good member in front of a bad one", [good.member([one], box=2), out.member([one], box=4)])):
        assert _rc(members) == -1, what                    # MOGAN_ERR_SHAPE
        torch.cuda.synchronize()
        assert out.untouched() and good.untouched(), what + ": a declined call has written"
