"""The rejections of mogan_attn_conf_f64 and mogan_attn_sheet_f64 (csrc/mogan_attn_sheet.hip), as
tests/test_layoutshift_rejections_cpu.py does for mogan_box_shift_sums_f64: every case is answered by the host BEFORE any HIP call, so
the table runs without a GPU -- the pointers are dummies that are never dereferenced.  -1 = MOGAN_ERR_SHAPE.  That the largest
accepted sizes pass the gate is shown by the answer changing to MOGAN_ERR_LAUNCH: that case runs only where no GPU is present.  Then
the ValueErrors of hip/ops.attn_conf and hip/ops.attn_sheet, which check their tensors before they touch the device or the library."""
import ctypes
import re

import pytest
import torch

from helpers import ROOT, load_pkg

load_pkg()
from mogan_amd.hip import lib, ops  # noqa: E402

PTR = ctypes.c_void_p(256)          # non-null, 16-byte aligned, never dereferenced
ODD = ctypes.c_void_p(260)          # 4-byte aligned only
NULL = ctypes.c_void_p(None)
SHAPE, LAUNCH = -1, -2
OK = dict(P=80, B=16, T=12, att=64, vis=256, alpha=180)
SHEET_POINTERS = ("attn", "cap_lens", "img", "table", "pick", "sheet", "stats", "flags")
CONF_POINTERS = ("attn", "cap_lens", "conf")


def sheet(**kw):
    d = dict(OK, **{k: v for k, v in kw.items() if k in OK})
    p = {name: kw.get(name, PTR) for name in SHEET_POINTERS}
    return lib.load().mogan_attn_sheet_f64(p["attn"], p["cap_lens"], p["img"], p["table"], p["pick"], d["P"], d["B"], d["T"], d["att"],
                                           d["vis"], d["alpha"], p["sheet"], p["stats"], p["flags"], NULL)


def conf(**kw):
    d = dict(OK, **{k: v for k, v in kw.items() if k in OK})
    p = {name: kw.get(name, PTR) for name in CONF_POINTERS}
    return lib.load().mogan_attn_conf_f64(p["attn"], p["cap_lens"], d["B"], d["T"], d["att"], p["conf"], NULL)


SHEET_CASES = [("NULL %s" % name, {name: NULL}) for name in SHEET_POINTERS] + [
    ("a table that is not 8-byte aligned", dict(table=ODD)), ("stats that are not 8-byte aligned", dict(stats=ODD)),
    ("P = 0", dict(P=0)), ("P < 0", dict(P=-1)), ("B = 0", dict(B=0)), ("B < 0", dict(B=-16)),
    ("T = 0", dict(T=0)), ("T = 33", dict(T=33)), ("T < 0", dict(T=-12)), ("T = 2^30", dict(T=1 << 30)),
    ("att = 1", dict(att=1, vis=256)), ("att = 0", dict(att=0)), ("att < 0", dict(att=-64)), ("att = 129", dict(att=129, vis=129)),
    ("att = 256", dict(att=256, vis=256)), ("vis = 257", dict(vis=257)), ("vis = 320", dict(vis=320)), ("vis = 512", dict(att=128, vis=512)),
    ("vis below att", dict(att=64, vis=32)), ("vis no multiple of att", dict(att=64, vis=200)), ("vis = 0", dict(vis=0)), ("vis < 0", dict(vis=-256)),
    ("alpha = -1", dict(alpha=-1)), ("alpha = 256", dict(alpha=256)),
    ("3 P vis vis = 3 * 2^31", dict(P=1 << 15)), ("3 B vis vis = 3 * 2^31", dict(B=1 << 15)),
    ("B T att att = 2^31", dict(B=1 << 14, T=32, att=64, vis=64)), ("P = 2^31 - 1", dict(P=2 ** 31 - 1)),
]
CONF_CASES = [("NULL %s" % name, {name: NULL}) for name in CONF_POINTERS] + [
    ("B = 0", dict(B=0)), ("B < 0", dict(B=-1)), ("T = 0", dict(T=0)), ("T = 33", dict(T=33)), ("T < 0", dict(T=-3)),
    ("att = 1", dict(att=1)), ("att = 0", dict(att=0)), ("att = 129", dict(att=129)), ("att < 0", dict(att=-64)), ("att = 2^30", dict(att=1 << 30)),
    ("B T att att = 2^31", dict(B=1 << 12, T=32, att=128)), ("B = 2^31 - 1", dict(B=2 ** 31 - 1)),
]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


@pytest.mark.parametrize("kw", [c[1] for c in SHEET_CASES], ids=[c[0] for c in SHEET_CASES])
def test_the_sheet_rejects_before_any_launch(kw):
    assert sheet(**kw) == SHAPE


@pytest.mark.parametrize("kw", [c[1] for c in CONF_CASES], ids=[c[0] for c in CONF_CASES])
def test_conf_rejects_before_any_launch(kw):
    assert conf(**kw) == SHAPE


@pytest.mark.skipif(torch.cuda.is_available(), reason="dummy pointers must never reach a real launch")
def test_the_largest_accepted_sizes_pass_the_gate():
    """the limits themselves and the smallest legal problem: not MOGAN_ERR_SHAPE; without a device the launch itself is what fails"""
    assert sheet() == LAUNCH and sheet(att=128, vis=256) == LAUNCH and sheet(att=128, vis=128) == LAUNCH and sheet(att=2, vis=2) == LAUNCH
    assert sheet(T=32) == LAUNCH and sheet(T=1, P=1, B=1) == LAUNCH and sheet(alpha=0) == LAUNCH and sheet(alpha=255) == LAUNCH
    assert sheet(att=2, vis=256) == LAUNCH and sheet(P=10922) == LAUNCH and sheet(attn=ODD, img=ODD) == LAUNCH
    assert conf() == LAUNCH and conf(B=1, T=1, att=2) == LAUNCH and conf(T=32, att=128) == LAUNCH and conf(B=4095, T=32, att=128) == LAUNCH


def _kinds(decl):
    P, L, I = lib.P, lib.L, lib.I
    kinds = []
    for arg in decl.split(","):
        arg = " ".join(arg.split())
        kinds.append(P if "*" in arg or arg.startswith("hipStream_t") else L if arg.startswith("long long") else I)
    return kinds


def test_the_signatures_are_the_headers():
    P, I = lib.P, lib.I
    assert lib.SIGNATURES["mogan_attn_conf_f64"] == [P, P, I, I, I, P, P]
    assert lib.SIGNATURES["mogan_attn_sheet_f64"] == [P, P, P, P, P, I, I, I, I, I, I, P, P, P, P]
    text = open("%s/include/mogan_hip.h" % ROOT).read()
    names = {"mogan_attn_conf_f64": ["attn", "cap_lens", "B", "T", "att", "conf", "stream"],
             "mogan_attn_sheet_f64": ["attn", "cap_lens", "img", "table", "pick", "P", "B", "T", "att", "vis", "alpha", "sheet", "stats", "flags",
                                      "stream"]}
    for name, want in names.items():
        assert name not in lib._RESTYPE
        decl = re.search(r"int %s\(([^)]*)\);" % name, text).group(1)
        assert _kinds(decl) == lib.SIGNATURES[name]
        assert [" ".join(a.split()).split()[-1].lstrip("*") for a in decl.split(",")] == want


# ------------------------------------------------------------------------------------------------- the ops' ValueErrors
def _args(B=2, T=4, att=8, up=2, P=3):
    attn = torch.full((B, T, att, att), 0.25)
    lens = torch.tensor([T, 2][:B], dtype=torch.int32)
    img = torch.zeros((B, 3, att * up, att * up))
    table = torch.zeros((att * up, att), dtype=torch.float64)
    pick = torch.tensor([[0, 0], [1, 1], [0, T - 1]][:P], dtype=torch.int32)
    return attn, lens, img, table, pick


@pytest.fixture()
def no_library(monkeypatch):
    """the checks come before any library call: the library must not even be opened"""
    def boom(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(lib, "load", boom)
    monkeypatch.setattr(ops, "call", boom)


BAD_PICKS = [("sample -1", [-1, 0]), ("sample B", [2, 0]), ("word -1", [0, -1]), ("word = T", [0, 4]), ("word = its caption's length", [1, 2]),
             ("word past its caption's length", [1, 3]), ("sample 2^31 - 1", [2 ** 31 - 1, 0])]


@pytest.mark.parametrize("row", [c[1] for c in BAD_PICKS], ids=[c[0] for c in BAD_PICKS])
def test_the_op_refuses_a_bad_pick_on_the_host(row, no_library):
    attn, lens, img, table, pick = _args()
    pick[1] = torch.tensor(row, dtype=torch.int32)
    with pytest.raises(ValueError, match="pick row 1"):
        ops.attn_sheet(attn, lens, img, table, pick)


def test_the_sheet_op_refuses_wrong_tensors_on_the_host(no_library):
    attn, lens, img, table, pick = _args()
    meta = torch.zeros((2, 4, 8, 8), device="meta")
    for args in ((attn.double(), lens, img, table, pick), (attn.numpy(), lens, img, table, pick), (attn[0], lens, img, table, pick),
                 (attn[:, :, :, ::2], lens, img, table, pick), (attn[:, :, :4].contiguous(), lens, img, table, pick),
                 (torch.zeros((2, 33, 8, 8)), lens, img, table, pick), (torch.zeros((2, 4, 1, 1)), lens, img, table, pick),
                 (torch.zeros((2, 4, 129, 129)), lens, img, table, pick), (meta, lens, img, table, pick),
                 (attn, lens.long(), img, table, pick), (attn, lens.float(), img, table, pick), (attn, lens.tolist(), img, table, pick),
                 (attn, lens[:1], img, table, pick), (attn, lens[None], img, table, pick), (attn, torch.zeros(4, dtype=torch.int32)[::2], img, table, pick),
                 (attn, torch.tensor([0, 2], dtype=torch.int32), img, table, pick), (attn, torch.tensor([5, 2], dtype=torch.int32), img, table, pick),
                 (attn, lens, img.double(), table, pick), (attn, lens, img[:1], table, pick), (attn, lens, img[:, :2], table, pick),
                 (attn, lens, torch.zeros((2, 3, 16, 8)), table, pick), (attn, lens, img[:, :, ::2, ::2], table, pick), (attn, lens, img.numpy(), table, pick),
                 (attn, lens, img, table.float(), pick), (attn, lens, img, table[:, :4].contiguous(), pick), (attn, lens, img, table.t().contiguous().t(), pick),
                 (attn, lens, img, table[0], pick), (attn, lens, img, table.numpy(), pick), (attn, lens, img, torch.zeros((12, 8), dtype=torch.float64), pick),
                 (attn, lens, torch.zeros((2, 3, 264, 264)), torch.zeros((264, 8), dtype=torch.float64), pick),
                 (attn, lens, img, table.to("meta"), pick),
                 (attn, lens, img, table, pick.long()), (attn, lens, img, table, pick.float()), (attn, lens, img, table, pick.numpy()),
                 (attn, lens, img, table, pick[:0]), (attn, lens, img, table, pick[:, 0]), (attn, lens, img, table, pick.t().contiguous().t()),
                 (attn, lens, img, table, torch.zeros((3, 3), dtype=torch.int32)),
                 (attn, lens, img, table, pick, -1), (attn, lens, img, table, pick, 256)):
        with pytest.raises(ValueError):
            ops.attn_sheet(*args)


def test_the_conf_op_refuses_wrong_tensors_on_the_host(no_library):
    attn, lens, _, _, _ = _args()
    for args in ((attn.double(), lens), (attn.numpy(), lens), (attn[0], lens), (attn[:, :, ::2], lens), (torch.zeros((2, 4, 8, 4)), lens),
                 (torch.zeros((2, 33, 8, 8)), lens), (torch.zeros((2, 4, 1, 1)), lens), (torch.zeros((2, 4, 129, 129)), lens),
                 (torch.zeros((2, 4, 8, 8), device="meta"), lens), (attn, lens.long()), (attn, lens.numpy()), (attn, lens[:1]),
                 (attn, torch.tensor([0, 2], dtype=torch.int32)), (attn, torch.tensor([4, 5], dtype=torch.int32))):
        with pytest.raises(ValueError):
            ops.attn_conf(*args)


def test_legal_host_arguments_reach_the_device_gate():
    """a host tensor is not the ops' to upload: no fallback"""
    attn, lens, img, table, pick = _args()
    with pytest.raises(lib.MoganHipError):
        ops.attn_conf(attn, lens)
    with pytest.raises(lib.MoganHipError):
        ops.attn_sheet(attn, lens, img, table, pick)
