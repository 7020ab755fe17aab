"""The owner-kept images of a convolution weight (hip/ops.py: WeightPacks -- packed panels, prepared filter images, the virtual
filters K of an up-convolution): which launches, event records and stream waits a sequence of uses produces.  A buffer that is
not current, or not ordered before its use, faults nowhere and fails no shape test -- the step trains on last step's filters -- so
the protocol is pinned here, on CPU, with the library, the stream / capture queries and the events mocked.  Only the public
surface is driven (attach_packs, pointer, wino_pointer, upconv_pointers, repack, repack_all, invalidate_all_packs, cell[0] += 1);
every assertion is on the whole trace."""
import ctypes
import types

import pytest
import torch

from helpers import load_pkg

load_pkg()
from mogan_amd.hip import lib, ops  # noqa: E402

GROUPS = {"mogan_conv_prep_group": "ppiiii", "mogan_upconv3x3_k4_group": "ppii"}      # array arguments after the member count


class Rig:
    def __init__(self, monkeypatch):
        self.state = {"handle": 7, "capturing": False, "prep_bytes": 128, "eligible": 1}
        self.trace = []
        self.counts = {"stream_ptr": 0, "capturing": 0, "prep_bytes": 0, "eligible": 0}
        rig, n_events = self, [0]

        def fake_call(name, *args):
            if name in GROUPS:                 # decode the ctypes arrays now: (n, [..], [..], ..., stream)
                n, out = args[0], [args[0]]
                for kind, a in zip(GROUPS[name], args[1:]):
                    ct = ctypes.c_void_p if kind == "p" else ctypes.c_int
                    out.append(list(ctypes.cast(a, ctypes.POINTER(ct))[:n]))
                args = tuple(out) + tuple(args[1 + len(GROUPS[name]):])
            rig.trace.append((name, args))

        def fake_stream_ptr():
            rig.counts["stream_ptr"] += 1
            return rig.state["handle"]

        def fake_capturing():
            rig.counts["capturing"] += 1
            return rig.state["capturing"]

        class Event:
            def __init__(self):
                self.id = n_events[0]
                n_events[0] += 1

            def record(self):
                rig.trace.append(("record", self.id, rig.state["handle"]))

        class Stream:
            def wait_event(self, ev):
                rig.trace.append(("wait", ev.id, rig.state["handle"]))

        def prep_bytes(*a):
            rig.counts["prep_bytes"] += 1
            return rig.state["prep_bytes"]

        def eligible(*a):
            rig.counts["eligible"] += 1
            return rig.state["eligible"]

        stub = types.SimpleNamespace(mogan_conv_prep_bytes=prep_bytes, mogan_pk_conv_eligible=eligible,
                                     mogan_pk_weight_bytes=lambda *a: 64)
        monkeypatch.setattr(ops, "call", fake_call)
        monkeypatch.setattr(ops, "ptr", lambda t: None if t is None else t.data_ptr())
        monkeypatch.setattr(ops, "stream_ptr", fake_stream_ptr)
        monkeypatch.setattr(lib, "_capturing", fake_capturing)
        monkeypatch.setattr(lib, "load", lambda: stub)
        monkeypatch.setattr(torch.cuda, "Event", Event)
        monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: Stream())
        for flag in ("PK_ENABLED", "WINO_PREP", "D2_PREP", "UPCONV_OWNED"):
            monkeypatch.setattr(ops, flag, True)

    def take(self):
        t, self.trace[:] = list(self.trace), []
        return t

    def on(self, handle, capturing=False):
        self.state["handle"], self.state["capturing"] = handle, capturing


@pytest.fixture
def rig(monkeypatch):
    return Rig(monkeypatch)


def stats():
    return {k: ops.PK_STATS.get(k, 0) for k in ("fwd", "dgrad", "wgrad", "packs", "wino_preps", "k4_builds")}


def delta(before, **changed):
    want = dict(before)
    for k, v in changed.items():
        want[k] += v
    return want


class Panel:
    """a (64, 32, 3, 3) weight whose forward takes the packed kernels"""
    shape, n_records = (64, 32, 3, 3), 1

    def __init__(self, cell=None, shape=None):
        self.w = torch.zeros(shape or self.shape)
        self.pk = ops.attach_packs(self.w, cell)
        self.p = {}

    def use(self, dgrad=0):
        self.p[dgrad] = self.pk.pointer(dgrad, 2, 8, 8, 1, 1, 1)
        return self.p[dgrad]

    def pack(self, handle, dgrad=0):
        Cout, Cin, KH, KW = self.w.shape
        return ("mogan_pk_weight_pack", (self.w.data_ptr(), self.p[dgrad], Cout, Cin, KH, KW, 1, 1, 1, dgrad, handle))

    def build(self, handle, ev):
        """the trace of a build at a use: the launch, then the record of event number `ev`"""
        return [self.pack(handle), ("record", ev, handle)]


class Image:
    """a (64, 32, 4, 4) weight whose 4x4 s2 forward takes a prepared filter image"""
    shape, n_records = (64, 32, 4, 4), 1

    def __init__(self, cell=None, shape=None):
        self.w = torch.zeros(shape or self.shape)
        self.pk = ops.attach_packs(self.w, cell)
        self.p = {}

    def use(self, dgrad=0, B=2):
        k = self.w.shape[2]
        self.p[dgrad] = self.pk.wino_pointer(dgrad, B, 16, 16, 2 if k == 4 else 1, 1, 1, 0)
        return self.p[dgrad]

    def member(self, dgrad=0):
        return (self.w.data_ptr(), self.p[dgrad], self.w.shape[0], self.w.shape[1], self.w.shape[2], dgrad)

    def build(self, handle, ev):
        return [prep_group([self.member()], handle), ("record", ev, handle)]


class Up:
    """a (32, 16, 3, 3) weight of an up-convolution: K = T w T^t (16, 32, 4, 4) and a filter image of K"""
    shape, n_records = (32, 16, 3, 3), 2

    def __init__(self, cell=None):
        self.w = torch.zeros(self.shape)
        self.pk = ops.attach_packs(self.w, cell)
        self.k, self.img = None, {}

    def use(self, dgrad=0):
        self.k, self.img[dgrad] = self.pk.upconv_pointers(dgrad, 2, 8, 8)
        return self.k, self.img[dgrad]

    def k_member(self):
        return (self.w.data_ptr(), self.k, 32, 16)

    def member(self, dgrad=0):
        """the image of K for direction `dgrad` of the up-convolution: the other direction of the virtual 4x4 s2 convolution"""
        return (self.k, self.img[dgrad], 16, 32, 4, 0 if dgrad else 1)

    def build(self, handle, ev):
        return [("mogan_upconv3x3_k4", (self.w.data_ptr(), self.k, 32, 16, handle)), ("record", ev, handle),
                prep_group([self.member()], handle), ("record", ev + 1, handle)]


def prep_group(members, handle):
    cols = [list(c) for c in zip(*members)]
    return ("mogan_conv_prep_group", (len(members),) + tuple(cols) + (handle,))


def k4_group(members, handle):
    cols = [list(c) for c in zip(*members)]
    return ("mogan_upconv3x3_k4_group", (len(members),) + tuple(cols) + (handle,))


KINDS = [Panel, Image, Up]


@pytest.mark.parametrize("kind", KINDS)
def test_first_use_builds_and_a_second_use_is_silent(rig, kind):
    before = stats()
    it = kind()
    got = it.use()
    assert got is not None and got != (None, None)
    assert rig.take() == it.build(7, 0)                               # launch(es) and one event each, no wait
    assert stats() == delta(before, **{Panel: {"packs": 1}, Image: {"wino_preps": 1}, Up: {"k4_builds": 1, "wino_preps": 1}}[kind])
    asked = rig.counts["capturing"]
    assert it.use() == got
    assert rig.take() == [] and rig.counts["capturing"] == asked      # same stream: the capture state is not even queried
    assert stats()["fwd"] == before["fwd"] and stats()["dgrad"] == before["dgrad"] and stats()["wgrad"] == before["wgrad"]


@pytest.mark.parametrize("kind", KINDS)
def test_use_on_another_stream_waits_for_the_build(rig, kind):
    it = kind()
    got = it.use()
    rig.take()
    rig.on(9)
    assert it.use() == got
    assert rig.take() == [("wait", ev, 9) for ev in range(kind.n_records)]        # one wait per buffer, no rebuild


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("built_capturing, used_capturing, waits", [(False, True, False), (True, True, True), (True, False, True)])
def test_capture_decides_the_wait(rig, kind, built_capturing, used_capturing, waits):
    """a capturing stream must not wait for an event recorded outside its capture; an event recorded inside one is waited for,
    by a capturing stream and by an eager one"""
    it = kind()
    rig.on(7, built_capturing)
    got = it.use()
    assert rig.take() == it.build(7, 0)
    rig.on(9, used_capturing)
    assert it.use() == got
    assert rig.take() == ([("wait", ev, 9) for ev in range(kind.n_records)] if waits else [])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("how", ["version", "global"])
def test_a_changed_weight_is_rebuilt_at_its_next_use(rig, kind, how):
    cell = [3]
    it = kind(cell)
    got = it.use()
    rig.take()
    if how == "version":
        cell[0] += 1
    else:
        ops.invalidate_all_packs()
    rig.on(9)                                                         # on another stream: a rebuild is followed by no wait
    assert it.use() == got                                            # the same buffers
    assert rig.take() == it.build(9, kind.n_records)                  # for an up-convolution: K, then the image built from it
    assert it.use() == got and rig.take() == []
    rig.on(7)
    assert it.use() == got
    assert rig.take() == [("wait", kind.n_records + i, 7) for i in range(kind.n_records)]      # the NEW events


def test_repack_of_both_directions(rig):
    before = stats()
    it = Panel()
    it.use(0), it.use(1)
    assert rig.take() == [it.pack(7, 0), ("record", 0, 7), it.pack(7, 1), ("record", 1, 7)]
    assert stats() == delta(before, packs=2)
    it.pk.repack()                                                    # 64 and 32 channels: both copies from one read of w
    assert rig.take() == [("mogan_pk_weight_pack_both", (it.w.data_ptr(), it.p[0], it.p[1], 64, 32, 3, 3, 1, 1, 1, 7)),
                          ("record", 2, 7)]
    assert stats() == delta(before, packs=3)
    rig.on(9)
    p = dict(it.p)
    assert (it.use(0), it.use(1)) == (p[0], p[1])
    assert rig.take() == [("wait", 2, 9), ("wait", 2, 9)]             # ONE event stands for both copies

    rig.on(7)
    before = stats()
    odd = Panel(shape=(64, 48, 3, 3))                                 # Cin = 48: one pack per copy
    odd.use(0), odd.use(1)
    rig.take()
    odd.pk.repack()
    assert rig.take() == [odd.pack(7, 0), ("record", 5, 7), odd.pack(7, 1), ("record", 6, 7)]
    assert stats() == delta(before, packs=4)

    one = Panel()                                                     # one direction in use: one pack
    one.use(1)
    rig.take()
    one.pk.repack()
    assert rig.take() == [one.pack(7, 1), ("record", 8, 7)]


def test_repack_all_of_a_bucket(rig):
    cell = [0]
    pan, i3, i4, up = Panel(cell), Image(cell, (64, 32, 3, 3)), Image(cell), Up(cell)
    pan.use(0), pan.use(1), i3.use(0), i3.use(1), i4.use(0), up.use(0), up.use(1)
    own = up.pk.wino_pointer(0, 2, 16, 16, 1, 1, 1, 0)                # the same 3x3 weight also runs a plain convolution
    idle = Panel(cell)                                                # attached, nothing in use
    rig.take()
    cell[0] += 1
    before = stats()
    ops.repack_all([pan.pk, i3.pk, idle.pk, i4.pk, up.pk])
    ev = 10                                                           # events 0..8: 2 panels, 3 images, K, 2 images of K, 1 own image
    images = [i3.member(0), i3.member(1), i4.member(0), (up.w.data_ptr(), own, 32, 16, 3, 0), up.member(0), up.member(1)]
    assert rig.take() == [("mogan_pk_weight_pack_both", (pan.w.data_ptr(), pan.p[0], pan.p[1], 64, 32, 3, 3, 1, 1, 1, 7)),
                          ("record", ev - 1, 7),
                          k4_group([up.k_member()], 7), ("record", ev, 7),            # K before the images built from it
                          prep_group(images, 7), ("record", ev + 1, 7)]
    assert stats() == delta(before, packs=1, k4_builds=1, wino_preps=1)

    def use_all():
        pan.use(0), pan.use(1), i3.use(0), i3.use(1), i4.use(0), up.use(0), up.use(1)
        assert up.pk.wino_pointer(0, 2, 16, 16, 1, 1, 1, 0) == own

    use_all()
    assert rig.take() == [] and stats() == delta(before, packs=1, k4_builds=1, wino_preps=1)
    rig.on(9)
    use_all()
    assert rig.take() == [("wait", e, 9) for e in (ev - 1, ev - 1, ev + 1, ev + 1, ev + 1, ev, ev + 1, ev, ev + 1, ev + 1)]
    rig.on(7)
    before = stats()
    ops.repack_all([])
    ops.repack_all([idle.pk])
    assert rig.take() == [] and stats() == before                     # empty groups launch nothing


@pytest.mark.parametrize("kind", KINDS)
def test_a_new_owner_makes_every_image_stale(rig, kind):
    cell, other = [0], [0]                                            # the same version number: only the invalidation tells
    it = kind(cell)
    got = it.use()
    rig.take()
    assert ops.attach_packs(it.w, cell) is it.pk and ops.attach_packs(it.w) is it.pk
    assert it.use() == got and rig.take() == []                       # the same owner again, or nobody: nothing changes
    assert ops.attach_packs(it.w, other) is it.pk and it.pk.cell is other
    if kind is Up:
        assert it.pk.k4 is not None and it.pk.k4pk.cell is other
    assert it.use() == got
    assert rig.take() == it.build(7, kind.n_records)
    cell[0] += 1                                                      # the old owner's counter no longer rules
    assert it.use() == got and rig.take() == []
    other[0] += 1
    assert it.use() == got
    assert rig.take() == it.build(7, 2 * kind.n_records)


def test_declined_geometries(rig):
    it = Panel()
    p = it.use()
    rig.take()
    asked = rig.counts["eligible"]
    assert it.pk.pointer(0, 2, 8, 8, 2, 1, 1) is None                 # one weight, a second convolution geometry
    assert it.pk.pointer(0, 2, 8, 8, 2, 1, 1) is None and it.use() == p
    assert rig.take() == [] and sorted(it.pk.slots) == [0]
    assert rig.counts["eligible"] == asked + 1                        # eligibility is asked once per geometry
    rig.state["eligible"] = 0
    assert it.pk.pointer(1, 2, 8, 8, 1, 1, 1) is None and it.pk.pointer(1, 2, 8, 8, 1, 1, 1) is None
    assert rig.take() == [] and sorted(it.pk.slots) == [0] and rig.counts["eligible"] == asked + 2

    rig.state["prep_bytes"] = 0                                       # the dispatch takes a kernel without an image
    im = Image()
    assert im.use() is None and im.use() is None
    assert rig.take() == [] and im.pk.wino == {} and rig.counts["prep_bytes"] == 1
    u = Up()
    k, img = u.use()
    assert k is not None and img is None and u.pk.k4pk.wino == {}     # K alone
    assert rig.take() == [("mogan_upconv3x3_k4", (u.w.data_ptr(), k, 32, 16, 7)), ("record", 1, 7)]


def test_a_larger_image_gets_a_new_buffer(rig):
    im = Image()
    p1 = im.use(B=2)
    assert rig.take() == im.build(7, 0)
    rig.state["prep_bytes"] = 256
    p2 = im.use(B=4)
    assert p2 != p1 and sorted(im.pk.wino) == [0]
    assert rig.take() == im.build(7, 1)                               # rebuilt into the new buffer (im.p[0] is p2 now)
    asked = rig.counts["prep_bytes"]
    assert im.use(B=2) == p2 and im.use(B=4) == p2                    # the smaller geometry's image fits: the same record
    assert rig.take() == [] and rig.counts["prep_bytes"] == asked
