"""torch.autograd.Function wrappers over the C ABI (include/mogan_hip.h).

These are the ONLY callers of libmogan_hip.so.  PyTorch supplies device memory, streams and the
autograd tape; all arithmetic on tensors happens inside the HIP kernels.  Every function raises
(MoganHipError) if the library is missing or an input is not on the GPU -- there is no fallback.
"""
import contextlib
import ctypes
import os

import torch

from . import lib
from .lib import call, ptr, stream_ptr, workspace

ACT_NONE, ACT_RELU, ACT_LRELU, ACT_GLU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3, 4, 5

# Test hook: when set to a list, every (Leaky)ReLU launch appends (activation code, its OUTPUT tensor).  A gradient check against a CPU
# reference can then hand the reference the same sign decisions: with millions of pre-activations per layer a few land
# within fp32 noise of the kink, and one flipped decision moves the weight gradients below it by ~1e-3 (tests/
# test_fullwidth_parity_gpu.py).  None (the default) costs one global lookup per launch.
ACT_TRACE = None


# Deferred running statistics (include/mogan_hip.h: mogan_bn_running_update).  While this is a list, training-mode BatchNorm
# launches leave running_mean / running_var alone and append what the update needs; bn_apply_deferred() performs the updates
# later, in list order -- the arithmetic of a call runs early, its place in the reference's call order is kept
# (miscc/losses.py: the "wrong pair" head of a discriminator update).
BN_DEFER = None


def bn_apply_deferred(pending):
    for mean, invstd, n, rm, rv, eps, momentum in pending:
        if rm is not None or rv is not None:
            call("mogan_bn_running_update", ptr(mean), ptr(invstd), ptr(rm), ptr(rv), mean.numel(), int(n), float(eps),
                 float(momentum), stream_ptr())
    del pending[:]


TRACE_GROUPS = 1            # set by a paired pass for the launches that do not know about groups (no BatchNorm inside)


def _trace(act, y, groups=1):
    """one ACT_TRACE entry per reference call: a tensor that stands for `groups` calls (groups batches one behind the other)
    is recorded as its per-call slices; inside a paired pass (TRACE_GROUPS > 1) the entries carry the call's index as a third
    element (discriminator_loss puts them back into the reference's call order: every layer of D(real), then of D(fake))"""
    if groups <= 1:
        ACT_TRACE.append((act, y))
        return
    n = y.shape[0] // groups
    for g in range(groups):
        ACT_TRACE.append((act, y[g * n:(g + 1) * n], g) if TRACE_GROUPS > 1 else (act, y[g * n:(g + 1) * n]))


# When a parameter already owns a dense .grad (the trainer's flat gradient buckets), the weight-gradient
# kernels accumulate straight into it (C += ...) and the Function returns None for that input: same result as
# autograd's `grad += new`, without the temporary and the extra read-modify-write pass (~350 launches/step).
DIRECT_GRAD = True


# Data-parallel overlap hook (attngan/trainer.ChunkedReducer): address ranges of flat gradient buckets whose owner wants to
# know when a parameter's .grad has just received a contribution (the kernel is queued on `stream`).  Empty unless N > 1.
GRAD_HOOKS = []


def _grad_hit(g, stream=None):
    if GRAD_HOOKS:
        p = g.data_ptr()
        for lo, hi, cb in GRAD_HOOKS:
            if lo <= p < hi:
                cb(p, stream)
                break


def _grad_buf(param):
    if not DIRECT_GRAD or param is None:
        return None
    g = getattr(param, "grad", None)
    if g is None or not g.is_contiguous() or g.dtype != torch.float32 or g.shape != param.shape:
        return None
    return g


# Weight gradients have no consumer until the optimizer step, so (in DIRECT_GRAD mode) they are launched on a
# side stream paired with the stream the backward runs on: the dgrad chain continues on the main stream and the
# wgrad launches fill the CUs its tails leave idle.  Opt-in per backward call through `with wgrad_overlap():`
# (the engines wrap every .backward() in it); leaving the context makes the current stream wait for the side
# stream, so the all-reduce / Adam / anybody reading .grad afterwards is ordered behind the weight gradients.
WGRAD_SIDE_STREAM = False
CAPTURE_WGRAD_OK = set()     # raw handles of streams that may fork a wgrad stream while being captured (depth-1 forks only)
_WGRAD_ENV = os.environ.get("MOGAN_WGRAD_STREAM", "1") != "0"
_wgrad_streams = {}


class _WgradFrame:
    """What ONE `with wgrad_overlap():` (one backward pass) owns: `used` = side streams that received its launches, `keep` =
    operands of its in-flight side-stream launches (released after the join so the caching allocator cannot hand their memory to
    a main-stream kernel that runs concurrently), `parked` = keys of the contributions it parked in _wgrad_pending.  A join
    waits for and clears only its own frame -- a nested or interleaved context on another stream keeps its waits and operands."""
    __slots__ = ("used", "keep", "parked")

    def __init__(self):
        self.used, self.keep, self.parked = [], [], []


_wgrad_frames = [_WgradFrame()]      # [0] = launches outside any context (joined by a bare join_wgrad())


# Merged weight gradients: a D update back-propagates through the same discriminator twice (real, fake).  For the deep
# layers (few output pixels, tens of MB of weights) a weight-gradient launch is bound by the read-modify-write of dW, not by
# its K = B*OH*OW; the first contribution is therefore parked and launched together with the second as ONE pass over the
# concatenated batch (dW = dY_1 X_1^t + dY_2 X_2^t -- the same sum), leftovers at the join.
MERGE_WGRAD = os.environ.get("MOGAN_MERGE_WGRAD", "1") != "0"
_wgrad_pending = {}
# under hipGraph capture too (the branch graphs of trainer.TrainEngine replay the merged launches): the parked contribution and
# the concatenated operands live in the graph's memory pool
MERGE_WGRAD_CAPTURED = True
_wgrad_ctx_depth = 0         # parking needs somebody to flush: only inside `with wgrad_overlap():`
_MERGE_K = 2048
_MERGE_W = 1 << 21


# The deep weights whose optimizer step and pack run as one pass (trainer.FlatAdam, mogan_pk_adam_pack_both) are not cleared
# by zero_grad.  WGRAD_OVERWRITE = True: the FIRST weight-gradient launch of an accumulation round writes dW instead of adding
# to it (the merged real + fake launch, as a rule the only one), later ones of the round -- the wrong-pair call of a
# conditional head, leftovers at the join -- add; nobody clears or reads a gradient nobody needs.  False: the fused kernel
# clears g behind its read (zero_g) and every launch adds, as everywhere else.  _OVERWRITE: gradient buffer address ->
# [the owner's round counter (a one-element list, bumped by its zero_grad), the round of the buffer's last launch].
FUSE_ADAM_PACK = os.environ.get("MOGAN_FUSE_ADAM_PACK", "1") != "0"       # read by trainer.TrainEngine when it is built
WGRAD_OVERWRITE = os.environ.get("MOGAN_WGRAD_OVERWRITE", "1") != "0"
_OVERWRITE = {}


def overwrite_register(g, round_cell):
    """g (a parameter's range of a flat gradient bucket) is no longer cleared by its owner: the first launch of each round
    overwrites it.  The round in progress counts as begun -- a launch before the next zero_grad adds, as it did before."""
    if g.data_ptr() in _OVERWRITE:
        return False
    _OVERWRITE[g.data_ptr()] = [round_cell, round_cell[0]]
    return True


def overwrite_drop(ptrs):
    """the owner clears these gradients itself again (or is gone)"""
    for p in ptrs:
        _OVERWRITE.pop(p, None)
    del ptrs[:]


def overwrite_stale(g):
    """g is registered and has received no launch in its owner's current round: it still holds the last round's gradient"""
    rec = _OVERWRITE.get(g.data_ptr())
    return rec is not None and rec[1] != rec[0][0]


def _first_of_round(g):
    """True: this launch into g is the first of its owner's accumulation round and g was not cleared -- it must overwrite"""
    rec = _OVERWRITE.get(g.data_ptr()) if _OVERWRITE else None
    if rec is None:
        return False
    first = rec[1] != rec[0][0]
    rec[1] = rec[0][0]
    return first


def _wgrad_launch(dy, x, w_shape, geom, g):
    stride, ph, pw, up = geom
    acc = not _first_of_round(g)
    if WGRAD_SIDE_STREAM:
        cur, side = _wgrad_stream()
        side.wait_stream(cur)                     # dy (and the zeroed / partly accumulated grad) are ready
        with torch.cuda.stream(side):
            conv2d_wgrad(dy, x, w_shape, stride, ph, pw, up, out=g, accumulate=acc)
        fr = _wgrad_frames[-1]
        if side not in fr.used:
            fr.used.append(side)
        fr.keep.append((dy, x))                   # freed only after the join (see join_wgrad)
        _grad_hit(g, side)
    else:
        conv2d_wgrad(dy, x, w_shape, stride, ph, pw, up, out=g, accumulate=acc)
        _grad_hit(g)


def _wgrad_accumulate(dy, x, w, geom, g):
    """dW += wgrad(dy, x) into the parameter's .grad buffer g, possibly deferred / merged (see MERGE_WGRAD)."""
    K = dy.shape[0] * dy.shape[2] * dy.shape[3]
    if not (MERGE_WGRAD and _wgrad_ctx_depth > 0 and K <= _MERGE_K and w.numel() >= _MERGE_W) \
            or (torch.cuda.is_current_stream_capturing() and not MERGE_WGRAD_CAPTURED):
        _wgrad_launch(dy, x, w.shape, geom, g)
        return
    cur = torch.cuda.current_stream()
    key = (g.data_ptr(), cur.cuda_stream)
    prev = _wgrad_pending.pop(key, None)
    if prev is None:
        # parked on THIS stream: autograd may be running the node on another stream than the one the context was entered on (the
        # tape of a replayed generator forward executes on its capture stream), so the flush goes by the context's own list of
        # keys and launches each leftover on the stream it was parked on
        _wgrad_pending[key] = (dy, x, tuple(w.shape), geom, g, cur)
        _wgrad_frames[-1].parked.append(key)
        return
    pdy, px, _, pgeom = prev[:4]
    if pgeom == geom and pdy.shape[1:] == dy.shape[1:] and px.shape[1:] == x.shape[1:]:
        _wgrad_launch(_cat_batch(pdy, dy), _cat_batch(px, x), w.shape, geom, g)
    else:
        _wgrad_launch(pdy, px, w.shape, pgeom, g)
        _wgrad_launch(dy, x, w.shape, geom, g)


def _cat_batch(a, b):
    """torch.cat([a, b]) along the batch axis of two dense tensors as one mogan_concat_fwd launch (the images of a tensor are the
    "channels" of a one-row concat)."""
    a, b = _c(a), _c(b)
    if a.shape[1:] != b.shape[1:]:
        raise lib.MoganHipError("_cat_batch: %r and %r differ behind the batch axis" % (tuple(a.shape), tuple(b.shape)))
    per = a[0].numel()
    out = torch.empty((a.shape[0] + b.shape[0],) + tuple(a.shape[1:]), dtype=torch.float32, device=a.device)
    arrs = _cat_arrays([(a.shape[0], 1, 0, 0, 0), (b.shape[0], 1, 0, 0, 0)], [a.data_ptr(), b.data_ptr()])
    call("mogan_concat_fwd", *arrs, 2, ptr(out), 1, per, stream_ptr())
    return out


class SplitBatchFn(torch.autograd.Function):
    """x (N, ...) -> (x[:B], x[B:]) as views; the two gradients come back as ONE dense tensor through one concat launch
    (autograd's own slice backward is a zero fill + a copy + an add per half)."""

    @staticmethod
    def forward(ctx, x, B):
        ctx.B, ctx.shape = B, tuple(x.shape)
        return x[:B], x[B:]

    @staticmethod
    def backward(ctx, da, db):
        B, shape = ctx.B, ctx.shape
        if da is None:
            da = torch.zeros((B,) + shape[1:], dtype=torch.float32, device=db.device)
        if db is None:
            db = torch.zeros((shape[0] - B,) + shape[1:], dtype=torch.float32, device=da.device)
        return _cat_batch(da, db), None


def split_batch(x, B):
    return SplitBatchFn.apply(_c(x), int(B))


def _wgrad_flush():
    """launch the single contributions the innermost context parked and nobody merged -- each on the stream it was parked on; the
    current stream then waits for every such stream that is not itself (the optimizer reads .grad behind the context)"""
    cur = torch.cuda.current_stream()
    fr = _wgrad_frames[-1]
    keys, fr.parked = fr.parked, []
    if len(_wgrad_frames) == 1:                      # a bare flush outside any context: everything that is still parked
        keys = list(_wgrad_pending)
    capturing = torch.cuda.is_current_stream_capturing()
    for key in keys:
        item = _wgrad_pending.pop(key, None)
        if item is None:
            continue                                  # merged with a second contribution meanwhile
        dy, x, w_shape, geom, g, st = item
        if st.cuda_stream == cur.cuda_stream:
            _wgrad_launch(dy, x, w_shape, geom, g)
        else:
            with torch.cuda.stream(st):
                _wgrad_launch(dy, x, w_shape, geom, g)
            if not capturing:
                cur.wait_stream(st)


@contextlib.contextmanager
def wgrad_overlap():
    global WGRAD_SIDE_STREAM, _wgrad_ctx_depth
    # not under hipGraph capture: hipStreamEndCapture segfaults (ROCm 7.2) on the nested fork pattern
    # capture stream -> branch stream -> wgrad stream; captured steps keep the weight gradients in line
    ok = _WGRAD_ENV
    if ok and torch.cuda.is_current_stream_capturing():
        ok = torch.cuda.current_stream().cuda_stream in CAPTURE_WGRAD_OK
    prev, WGRAD_SIDE_STREAM = WGRAD_SIDE_STREAM, ok
    _wgrad_ctx_depth += 1
    _wgrad_frames.append(_WgradFrame())
    try:
        yield
    finally:
        try:
            _wgrad_flush()                # parked single contributions (still under this context's stream policy)
        finally:
            _wgrad_ctx_depth -= 1
            WGRAD_SIDE_STREAM = prev
            join_wgrad()
            _wgrad_frames.pop()


def _wgrad_stream():
    cur = torch.cuda.current_stream()
    side = _wgrad_streams.get(cur.cuda_stream)
    if side is None:
        side = _wgrad_streams[cur.cuda_stream] = torch.cuda.Stream()
    return cur, side


def precreate_wgrad_stream(stream):
    """Create the weight-gradient side stream of `stream` now.  HIP multiplexes streams onto a few hardware queues
    (GPU_MAX_HW_QUEUES, 4 by default) in creation order, and two streams that share a queue serialize -- so the engines
    create their streams in one fixed order (branch streams, their wgrad streams, communication streams last) instead
    of leaving it to the first backward pass."""
    if stream.cuda_stream not in _wgrad_streams:
        _wgrad_streams[stream.cuda_stream] = torch.cuda.Stream()
    return _wgrad_streams[stream.cuda_stream]


def join_wgrad():
    """The current stream waits for the weight-gradient launches of the backward pass that just ended: for its own paired side
    stream AND for every side stream that received launches since the last join.  The second part matters when autograd ran the
    backward on ANOTHER stream than the caller's -- the nodes of a tape recorded on a capture stream (the generator's replayed
    forward, trainer.TrainEngine g_fwd_only) execute on that stream, so their weight gradients went to ITS side stream; joining
    only the caller's pair would let the optimizer read gradients that are still being written."""
    fr = _wgrad_frames[-1]
    if not _wgrad_streams:
        del fr.keep[:]
        return
    cur = torch.cuda.current_stream()
    side = _wgrad_streams.get(cur.cuda_stream)
    if side is not None:
        cur.wait_stream(side)
    capturing = torch.cuda.is_current_stream_capturing()
    for s_ in fr.used:
        if s_ is not side and not capturing:
            cur.wait_stream(s_)
    del fr.used[:]
    del fr.keep[:]


def _c(t):
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


# ------------------------------------------------------------------------------- convolution
def conv_out_hw(Hs, Ws, KH, KW, stride, ph, pw, up):
    H, W = Hs << up, Ws << up
    return (H + 2 * ph - KH) // stride + 1, (W + 2 * pw - KW) // stride + 1


# nearest-x2 upsample + conv3x3(p1) runs as the transposed 4x4-s2 convolution (include/mogan_hip.h: mogan_upconv3x3_*):
# 2.25x fewer FLOPs.  MOGAN_UPCONV4=0 keeps the fused-upsample 3x3 kernels (the kernel tests compare both).
UPCONV4 = True


def _is_upconv(w_shape, stride, ph, pw, up):
    return UPCONV4 and bool(up) and stride == 1 and ph == 1 and pw == 1 and w_shape[2] == 3 and w_shape[3] == 3


# ------------------------------------------------------------------------------- packed weights (csrc/mogan_pgemm.hip)
# The weight-heavy convolutions (deep discriminator layers) read their filters from a PACKED copy: the three bf16 pieces of
# every weight in matrix-instruction order, one copy per direction (forward / data gradient).  The copy belongs to the
# parameter's owner: trainer.FlatAdam attaches a WeightPacks object to every 4-D parameter of its bucket and re-packs the
# copies in use right after each optimizer step (one pack per weight version, used by the real, the fake and the generator
# pass); anything else that writes weights calls FlatAdam.touch() / invalidate_all_packs().  A parameter without the
# attribute (plain modules, the kernel tests' default) takes the unpacked kernels.
PK_ENABLED = True
PK_STATS = {"fwd": 0, "dgrad": 0, "wgrad": 0, "packs": 0}      # launches through the packed path (tests, diagnostics)
PK_WGRAD = True          # the deep layers' weight gradients on the packed kernels too
_pk_wgrad_elig = {}
_PK_GLOBAL = [0]


def invalidate_all_packs():
    """Every packed weight copy of the process is stale (weights were written behind the owners' backs: load_state_dict,
    load_params, a test poking .data); they are rebuilt at their next use."""
    _PK_GLOBAL[0] += 1


class WeightImage:
    """ONE derived device buffer of one weight -- a packed panel, a prepared filter image or the K of an up-convolution:
    `buf` was built from weight version `version` in global epoch `epoch` on stream `stream` (raw handle), `captured` = inside a
    hipGraph capture; `event` was recorded right behind the build.  `geom` = (stride, ph, pw) of a packed panel, else None."""
    __slots__ = ("buf", "version", "epoch", "event", "stream", "captured", "geom")

    def __init__(self, buf, geom=None):
        self.buf, self.geom = buf, geom
        self.version = self.epoch = -1
        self.event = self.stream = None
        self.captured = False

    def invalidate(self):
        self.version = -1

    def ready(self, cell):
        """False: stale, older than the weight version cell[0] or than the global epoch -- the caller rebuilds the buffer on the
        current stream (no wait follows).  True: current, and ordered before a use on the current stream"""
        if self.version != cell[0] or self.epoch != _PK_GLOBAL[0]:
            return False
        if self.stream != stream_ptr() and (self.captured or not lib._capturing()):
            # built on another stream: order behind that build (a capturing stream must not wait for an event recorded
            # outside its capture -- and need not: the device is synchronised before a capture begins)
            torch.cuda.current_stream().wait_event(self.event)
        return True


def _stamp(st, built):
    """the launch just queued on the current stream (handle `st`) built the images of `built`, (WeightImage, version cell)
    pairs: they are current now, and ONE event orders their uses on other streams behind it"""
    ev = torch.cuda.Event()
    ev.record()
    cap = bool(lib._capturing())
    for im, cell in built:
        im.version, im.epoch, im.event, im.stream, im.captured = cell[0], _PK_GLOBAL[0], ev, st, cap


def _group_args(n, pointers, ints):
    """the array arguments of a grouped launch with n members: a void* array per list of `pointers`, an int array per list of `ints`"""
    VP, CI = ctypes.c_void_p * n, ctypes.c_int * n
    return [ctypes.cast(VP(*v), ctypes.c_void_p) for v in pointers] + [ctypes.cast(CI(*v), ctypes.c_void_p) for v in ints]


class WeightPacks:
    """The derived images of ONE convolution weight, a WeightImage each, kept current by the weight's owner (version cell)."""

    def __init__(self, w, version_cell=None):
        self.w = w
        self.cell = version_cell if version_cell is not None else [0]
        # packed panels of the deep layers: slots[dgrad], geom = the convolution geometry they were packed for;
        # elig[(dgrad, geometry)] = does the call take the packed kernels
        self.slots = {}
        self.elig = {}
        # prepared filter images (include/mogan_hip.h "Prepared filter images"): wino[dgrad]; wbytes[(dgrad, geometry)] = image
        # size, 0 = the geometry takes a kernel without one
        self.wino = {}
        self.wbytes = {}
        # upsample + conv3x3 as the transposed 4x4 s2 convolution (mogan_upconv3x3_*): k4 = the virtual filters K = T w T^t of this
        # weight version (buf: (Cin, Cout, 4, 4)), and k4pk = a child WeightPacks over K (same version cell) that holds the
        # filter images of the kernels running the virtual convolution
        self.k4 = None
        self.k4pk = None

    def _pack(self, dgrad, slot):
        Cout, Cin, KH, KW = self.w.shape
        st = stream_ptr()
        stride, ph, pw = slot.geom
        call("mogan_pk_weight_pack", ptr(self.w), slot.buf.data_ptr(), Cout, Cin, KH, KW, stride, ph, pw, dgrad, st)
        _stamp(st, [(slot, self.cell)])
        PK_STATS["packs"] += 1

    def both_in_use(self):
        """both panels are in use, for one geometry, on a shape mogan_pk_weight_pack_both packs in one launch"""
        s0, s1 = self.slots.get(0), self.slots.get(1)
        Cout, Cin = self.w.shape[:2]
        return s0 is not None and s1 is not None and s0.geom == s1.geom and Cin % 32 == 0 and Cout % 32 == 0

    def adam_fusable(self):
        """... and the optimizer step can ride in that launch (mogan_pk_adam_pack_both: 4x4, 3x3 and 1x1 filters)"""
        return self.both_in_use() and self.w.shape[2] * self.w.shape[3] in (16, 9, 1)

    def repack(self):
        """re-pack every copy in use now, on the current stream (the owner just changed the weight): both directions from one
        read of the master where both are in use (mogan_pk_weight_pack_both)"""
        s0, s1 = self.slots.get(0), self.slots.get(1)
        Cout, Cin, KH, KW = self.w.shape
        if self.both_in_use():
            stride, ph, pw = s0.geom
            st = stream_ptr()
            call("mogan_pk_weight_pack_both", ptr(self.w), s0.buf.data_ptr(), s1.buf.data_ptr(), Cout, Cin, KH, KW, stride, ph, pw, st)
            _stamp(st, [(s0, self.cell), (s1, self.cell)])
            PK_STATS["packs"] += 1
            return
        for dgrad, slot in self.slots.items():
            self._pack(dgrad, slot)

    def pointer(self, dgrad, B, Hs, Ws, stride, ph, pw):
        """device pointer of the packed copy for this call's geometry, or None: take the unpacked kernels"""
        key = (dgrad, B, Hs, Ws, stride, ph, pw)
        e = self.elig.get(key)
        Cout, Cin, KH, KW = self.w.shape
        if e is None:
            e = self.elig[key] = bool(lib.load().mogan_pk_conv_eligible(B, Cin, Hs, Ws, Cout, KH, KW, stride, ph, pw, dgrad))
        if not e:
            return None
        slot = self.slots.get(dgrad)
        if slot is None:
            nbytes = int(lib.load().mogan_pk_weight_bytes(Cout, Cin, KH, KW, stride, dgrad))
            buf = torch.empty(nbytes, dtype=torch.uint8, device=self.w.device)
            slot = self.slots[dgrad] = WeightImage(buf, (stride, ph, pw))
        elif slot.geom != (stride, ph, pw):
            return None                                   # one weight, two convolution geometries: not a case of the step
        if not slot.ready(self.cell):
            self._pack(dgrad, slot)
        return slot.buf.data_ptr()

    def wino_pointer(self, dgrad, B, Hs, Ws, stride, ph, pw, up):
        """device pointer of this weight's prepared filter image for the direction, current and ordered before a use on the
        current stream -- or None: the convolution takes a kernel without one (or the library is a native-fp32 build).  The kind
        of image follows the filter size: the Winograd kernels' for 3x3 s1, dconv2_fwd_kernel's for 4x4 s2 (mogan_conv_prep_bytes)"""
        key = (dgrad, B, Hs, Ws, stride, ph, pw, up)
        nb = self.wbytes.get(key)
        if nb is None:
            Cout, Cin, KH, KW = self.w.shape
            nb = self.wbytes[key] = int(lib.load().mogan_conv_prep_bytes(B, Cin, Hs, Ws, Cout, KH, KW, stride, ph, pw, up, dgrad))
        if not nb:
            return None
        im = self.wino.get(dgrad)
        if im is None or im.buf.numel() < nb:
            im = self.wino[dgrad] = WeightImage(torch.empty(nb, dtype=torch.uint8, device=self.w.device))
        if not im.ready(self.cell):
            wino_prep([(self, dgrad, im)])
        return im.buf.data_ptr()

    def k4_build(self):
        """K = T w T^t of the current weight on the current stream (one launch)"""
        Cout, Cin = int(self.w.shape[0]), int(self.w.shape[1])
        st = stream_ptr()
        call("mogan_upconv3x3_k4", ptr(self.w), self.k4.buf.data_ptr(), Cout, Cin, st)
        _stamp(st, [(self.k4, self.cell)])
        PK_STATS["k4_builds"] = PK_STATS.get("k4_builds", 0) + 1

    def upconv_pointers(self, dgrad, B, Hs, Ws):
        """(K pointer, filter-image pointer or None) for the up-convolution of an (B, Cin, Hs, Ws) input with this 3x3 weight:
        direction 0 (forward) runs the DATA GRADIENT of the virtual 4x4 s2 convolution C4 (in = Cout, out = Cin) on 2Hs x 2Ws,
        direction 1 its forward.  Both current and ordered before a use on the current stream."""
        if self.k4 is None:
            Cout, Cin = int(self.w.shape[0]), int(self.w.shape[1])
            self.k4 = WeightImage(torch.empty((Cin, Cout, 4, 4), dtype=torch.float32, device=self.w.device))
            self.k4pk = WeightPacks(self.k4.buf, self.cell)
        if not self.k4.ready(self.cell):
            self.k4_build()
        img = self.k4pk.wino_pointer(0 if dgrad else 1, B, 2 * Hs, 2 * Ws, 2, 1, 1, 0) if D2_PREP else None
        return self.k4.buf.data_ptr(), img

    def invalidate(self, version_cell):
        """a new owner's version counter rules from now on: every image is stale"""
        self.cell = version_cell
        for im in list(self.slots.values()) + list(self.wino.values()):
            im.invalidate()
        if self.k4 is not None:
            self.k4.invalidate()
            self.k4pk.invalidate(version_cell)


def wino_prep(items):
    """(WeightPacks, dgrad, image) triples -> their prepared filter images rebuilt on the current stream in one launch per kind
    (mogan_conv_prep_group: the Winograd images of the 3x3 weights, dconv2's images of the 4x4 s2 weights)"""
    n = len(items)
    if not n:
        return
    ws = [[pk.w.data_ptr() for pk, _, _ in items], [im.buf.data_ptr() for _, _, im in items]]
    shapes = [pk.w.shape for pk, _, _ in items]
    ints = [[s[i] for s in shapes] for i in (0, 1, 2)] + [[int(d) for _, d, _ in items]]        # Cout, Cin, KH, direction
    st = stream_ptr()
    call("mogan_conv_prep_group", n, *_group_args(n, ws, ints), st)
    _stamp(st, [(im, pk.cell) for pk, _, im in items])
    PK_STATS["wino_preps"] = PK_STATS.get("wino_preps", 0) + 1


def k4_build_group(pks):
    """K = T w T^t of every pack in `pks` on the current stream in one launch (mogan_upconv3x3_k4_group)"""
    n = len(pks)
    if not n:
        return
    ws = [[pk.w.data_ptr() for pk in pks], [pk.k4.buf.data_ptr() for pk in pks]]
    shapes = [pk.w.shape for pk in pks]
    st = stream_ptr()
    call("mogan_upconv3x3_k4_group", n, *_group_args(n, ws, [[s[i] for s in shapes] for i in (0, 1)]), st)
    _stamp(st, [(pk.k4, pk.cell) for pk in pks])
    PK_STATS["k4_builds"] = PK_STATS.get("k4_builds", 0) + 1


def repack_all(packs, packed=()):
    """Every derived weight image of a bucket brought up to date on the current stream (the owner changed the weights): the
    packed panels pack by pack, the virtual filters of the up-convolutions in one launch, then the prepared filter images of
    all weights -- those built from the virtual filters among them -- in one launch.  `packed`: ids of the packs whose panels
    the owner's optimizer step has already written (adam_pack_both)."""
    items, k4s = [], []
    for pk in packs:
        if id(pk) not in packed:
            pk.repack()
        items += [(pk, d, im) for d, im in pk.wino.items()]
        if pk.k4 is not None:                  # the virtual filters of an up-convolution, then the images built from them
            k4s.append(pk)
            items += [(pk.k4pk, d, im) for d, im in pk.k4pk.wino.items()]
    k4_build_group(k4s)
    wino_prep(items)


def _wino_prep_ptr(w, dgrad, B, Hs, Ws, stride, ph, pw, up):
    pk = getattr(w, "_mogan_pk", None)
    if pk is None or not WINO_PREP:
        return None
    return pk.wino_pointer(dgrad, B, Hs, Ws, stride, ph, pw, up)


WINO_PREP = True      # (module attribute: False = every convolution prepares its filters per call, as without an owner)


D2_PREP = True        # (module attribute: False = the 4x4 s2 convolutions prepare dconv2's filter image per call)
UPCONV_OWNED = True   # (module attribute: False = the up-convolutions build K = T w T^t per call, mogan_upconv3x3_fwd / _dgrad)


def _prep_kind(KH, KW, stride, up):
    """filter sizes that may have a prepared image: 3x3 s1 (Winograd) and 4x4 s2 (dconv2_fwd_kernel)"""
    return (KH == 3 and KW == 3 and stride == 1) or (D2_PREP and KH == 4 and KW == 4 and stride == 2 and not up)


def attach_packs(w, version_cell=None):
    pk = getattr(w, "_mogan_pk", None)
    if pk is None:
        pk = w._mogan_pk = WeightPacks(w, version_cell)
    elif version_cell is not None and pk.cell is not version_cell:
        pk.invalidate(version_cell)         # a new owner (a second FlatAdam over the same network)
    return pk


def _packed(w, dgrad, B, Hs, Ws, stride, ph, pw, up):
    if up or not PK_ENABLED:
        return None
    pk = getattr(w, "_mogan_pk", None)
    if pk is None:
        return None
    return pk.pointer(dgrad, B, Hs, Ws, stride, ph, pw)


def conv2d_forward(x, w, stride, ph, pw, up):
    B, Cin, Hs, Ws = x.shape
    Cout, _, KH, KW = w.shape
    wp = _packed(w, 0, B, Hs, Ws, stride, ph, pw, up)
    if wp is not None:
        OH, OW = conv_out_hw(Hs, Ws, KH, KW, stride, ph, pw, 0)
        y = torch.empty((B, Cout, OH, OW), dtype=torch.float32, device=x.device)
        wsp, wsn = workspace(x.device)
        call("mogan_conv2d_fwd_pk", ptr(x), wp, ptr(y), B, Cin, Hs, Ws, Cout, KH, KW, stride, ph, pw, wsp, wsn, stream_ptr())
        PK_STATS["fwd"] += 1
        return y
    if _is_upconv(w.shape, stride, ph, pw, up):
        y = torch.empty((B, Cout, 2 * Hs, 2 * Ws), dtype=torch.float32, device=x.device)
        wsp, wsn = workspace(x.device)
        pk = getattr(w, "_mogan_pk", None)
        if pk is not None and WINO_PREP and UPCONV_OWNED:     # the owner's K = T w T^t (and filter image) of this weight version
            k4, img = pk.upconv_pointers(0, B, Hs, Ws)
            call("mogan_conv2d_dgrad_wp", ptr(x), k4, img, ptr(y), B, Cout, 2 * Hs, 2 * Ws, Cin, 4, 4, 2, 1, 1, 0, wsp, wsn, stream_ptr())
            return y
        call("mogan_upconv3x3_fwd", ptr(x), ptr(w), ptr(y), B, Cin, Hs, Ws, Cout, wsp, wsn, stream_ptr())
        return y
    OH, OW = conv_out_hw(Hs, Ws, KH, KW, stride, ph, pw, up)
    y = torch.empty((B, Cout, OH, OW), dtype=torch.float32, device=x.device)
    wsp, wsn = workspace(x.device)
    wprep = _wino_prep_ptr(w, 0, B, Hs, Ws, stride, ph, pw, up) if _prep_kind(KH, KW, stride, up) else None
    if wprep is not None:        # the owner's prepared Winograd filter image of this weight version (no transform launch here)
        call("mogan_conv2d_fwd_wp", ptr(x), ptr(w), wprep, ptr(y), B, Cin, Hs, Ws, Cout, KH, KW, stride, ph, pw, up,
             wsp, wsn, stream_ptr())
        return y
    call("mogan_conv2d_fwd", ptr(x), ptr(w), ptr(y), B, Cin, Hs, Ws, Cout, KH, KW, stride, ph, pw, up,
         wsp, wsn, stream_ptr())
    return y


def conv2d_dgrad(dy, w, x_shape, stride, ph, pw, up):
    B, Cin, Hs, Ws = x_shape
    Cout, _, KH, KW = w.shape
    wsp, wsn = workspace(dy.device)
    wp = _packed(w, 1, B, Hs, Ws, stride, ph, pw, up)
    if wp is not None:
        dx = torch.empty((B, Cin, Hs, Ws), dtype=torch.float32, device=dy.device)
        call("mogan_conv2d_dgrad_pk", ptr(dy), wp, ptr(dx), B, Cin, Hs, Ws, Cout, KH, KW, stride, ph, pw, wsp, wsn, stream_ptr())
        PK_STATS["dgrad"] += 1
        return dx
    if _is_upconv(w.shape, stride, ph, pw, up):          # the gradient comes out at the source resolution
        dx = torch.empty((B, Cin, Hs, Ws), dtype=torch.float32, device=dy.device)
        pk = getattr(w, "_mogan_pk", None)
        if pk is not None and WINO_PREP and UPCONV_OWNED:
            k4, img = pk.upconv_pointers(1, B, Hs, Ws)
            call("mogan_conv2d_fwd_wp", ptr(dy), k4, img, ptr(dx), B, Cout, 2 * Hs, 2 * Ws, Cin, 4, 4, 2, 1, 1, 0, wsp, wsn, stream_ptr())
            return dx
        call("mogan_upconv3x3_dgrad", ptr(dy), ptr(w), ptr(dx), B, Cin, Hs, Ws, Cout, wsp, wsn, stream_ptr())
        return dx
    du = torch.empty((B, Cin, Hs << up, Ws << up), dtype=torch.float32, device=dy.device)
    wprep = _wino_prep_ptr(w, 1, B, Hs, Ws, stride, ph, pw, up) if _prep_kind(KH, KW, stride, up) else None
    if wprep is not None:
        call("mogan_conv2d_dgrad_wp", ptr(dy), ptr(w), wprep, ptr(du), B, Cin, Hs, Ws, Cout, KH, KW, stride, ph, pw, up,
             wsp, wsn, stream_ptr())
    else:
        call("mogan_conv2d_dgrad", ptr(dy), ptr(w), ptr(du), B, Cin, Hs, Ws, Cout, KH, KW, stride, ph, pw, up,
             wsp, wsn, stream_ptr())
    if not up:
        return du
    dx = torch.empty((B, Cin, Hs, Ws), dtype=torch.float32, device=dy.device)
    call("mogan_down2_sum", ptr(du), ptr(dx), B * Cin, Hs, Ws, stream_ptr())
    return dx


def conv2d_wgrad(dy, x, w_shape, stride, ph, pw, up, out=None, accumulate=False):
    B, Cin, Hs, Ws = x.shape
    Cout, _, KH, KW = w_shape
    wsp, wsn = workspace(dy.device)
    dw = out if out is not None else torch.empty(w_shape, dtype=torch.float32, device=dy.device)
    if PK_ENABLED and PK_WGRAD and not up:
        key = (B, Cin, Hs, Ws, Cout, KH, KW, stride, ph, pw, wsn)
        e = _pk_wgrad_elig.get(key)
        if e is None:
            e = _pk_wgrad_elig[key] = bool(lib.load().mogan_pk_wgrad_eligible(B, Cin, Hs, Ws, Cout, KH, KW, stride, ph, pw, wsn))
        if e:
            call("mogan_conv2d_wgrad_pk", ptr(dy), ptr(x), ptr(dw), B, Cin, Hs, Ws, Cout, KH, KW, stride, ph, pw,
                 1 if accumulate else 0, wsp, wsn, stream_ptr())
            PK_STATS["wgrad"] = PK_STATS.get("wgrad", 0) + 1
            return dw
    if _is_upconv(w_shape, stride, ph, pw, up):
        call("mogan_upconv3x3_wgrad", ptr(dy), ptr(x), ptr(dw), B, Cin, Hs, Ws, Cout, 1 if accumulate else 0, wsp, wsn,
             stream_ptr())
        return dw
    call("mogan_conv2d_wgrad", ptr(dy), ptr(x), ptr(dw), B, Cin, Hs, Ws, Cout, KH, KW, stride, ph, pw, up,
         1 if accumulate else 0, wsp, wsn, stream_ptr())
    return dw


class Conv2dFn(torch.autograd.Function):
    """y = conv2d(upsample2x?(x), w) (+ bias).  model.py:35-55,587,598-609,626,664-677."""

    @staticmethod
    def forward(ctx, x, w, bias, stride, ph, pw, up):
        x, w = _c(x), _c(w)
        y = conv2d_forward(x, w, stride, ph, pw, up)
        if bias is not None:
            call("mogan_bias_add", ptr(y), ptr(_c(bias)), y.shape[0], y.shape[1], y.shape[2] * y.shape[3],
                 stream_ptr())
        ctx.save_for_backward(x, w)
        ctx.bias_ref = bias
        ctx.geom = (stride, ph, pw, up, bias is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        stride, ph, pw, up, has_bias = ctx.geom
        dy = _c(dy)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = conv2d_dgrad(dy, w, x.shape, stride, ph, pw, up)
        if ctx.needs_input_grad[1]:
            g = _grad_buf(w)
            if g is not None:
                _wgrad_accumulate(dy, x, w, (stride, ph, pw, up), g)
            else:
                dw = conv2d_wgrad(dy, x, w.shape, stride, ph, pw, up)
        if has_bias and ctx.needs_input_grad[2]:
            g = _grad_buf(ctx.bias_ref)
            db = g if g is not None else torch.empty(dy.shape[1], dtype=torch.float32, device=dy.device)
            call("mogan_bias_grad", ptr(dy), ptr(db), dy.shape[0], dy.shape[1], dy.shape[2] * dy.shape[3],
                 1 if g is not None else 0, stream_ptr())
            if g is not None:
                db = None
                _grad_hit(g)
        return dx, dw, db, None, None, None, None


class ConvAffineReluFn(torch.autograd.Function):
    """z = relu(scale[c] * conv2d(x, w) + shift[c]) in one launch (the affine + ReLU ride in the conv epilogue or in its
    split-K reduction): BasicConv2d of the frozen eval-mode Inception trunk (model.py:258-299).  Saves x, w and the
    OUTPUT z; backward: g = dz * scale * (z > 0), then the ordinary data / weight gradients of the conv."""

    @staticmethod
    def forward(ctx, x, w, scale, shift, stride, ph, pw):
        x, w = _c(x), _c(w)
        B, Cin, Hs, Ws = x.shape
        Cout, _, KH, KW = w.shape
        OH, OW = conv_out_hw(Hs, Ws, KH, KW, stride, ph, pw, 0)
        z = torch.empty((B, Cout, OH, OW), dtype=torch.float32, device=x.device)
        wsp, wsn = workspace(x.device)
        call("mogan_conv2d_affine_fwd", ptr(x), ptr(w), ptr(scale), ptr(shift), ptr(z), B, Cin, Hs, Ws, Cout, KH, KW,
             stride, ph, pw, 1, wsp, wsn, stream_ptr())
        ctx.save_for_backward(x, w, z, scale)
        ctx.geom = (stride, ph, pw)
        return z

    @staticmethod
    def backward(ctx, dz):
        x, w, z, scale = ctx.saved_tensors
        stride, ph, pw = ctx.geom
        dz = _c(dz)
        g = torch.empty_like(z)
        call("mogan_affine_relu_bwd_out", ptr(z), ptr(dz), ptr(scale), ptr(g), z.shape[0], z.shape[1],
             z.shape[2] * z.shape[3], stream_ptr())
        dx = conv2d_dgrad(g, w, x.shape, stride, ph, pw, 0) if ctx.needs_input_grad[0] else None
        dw = conv2d_wgrad(g, x, w.shape, stride, ph, pw, 0) if ctx.needs_input_grad[1] else None
        return dx, dw, None, None, None, None, None


class ConvLReLUFn(torch.autograd.Function):
    """z = LeakyReLU(conv2d(x, w)) with the activation in the convolution's epilogue (mogan_conv2d_lrelu_fwd): the first layer
    of every discriminator (model.py:597-598, 660-661).  Saves x, w and the OUTPUT z; backward: g = dz * (z > 0 ? 1 : slope)
    (z has the pre-activation's sign), then the ordinary data / weight gradients."""

    @staticmethod
    def forward(ctx, x, w, stride, ph, pw, slope):
        x, w = _c(x), _c(w)
        B, Cin, Hs, Ws = x.shape
        Cout, _, KH, KW = w.shape
        OH, OW = conv_out_hw(Hs, Ws, KH, KW, stride, ph, pw, 0)
        z = torch.empty((B, Cout, OH, OW), dtype=torch.float32, device=x.device)
        wsp, wsn = workspace(x.device)
        rc = lib.load().mogan_conv2d_lrelu_fwd(ptr(x), ptr(w), ptr(z), B, Cin, Hs, Ws, Cout, KH, KW, stride, ph, pw, slope,
                                               wsp, wsn, stream_ptr())
        if rc == 1:                                        # not a geometry for the fused epilogue
            z = conv2d_forward(x, w, stride, ph, pw, 0)
            call("mogan_act_fwd", ptr(z), ptr(z), B, Cout, OH * OW, ACT_LRELU, slope, stream_ptr())
        elif rc != 0:
            raise lib.MoganHipError("mogan_conv2d_lrelu_fwd failed: %s" % lib._ERRORS.get(rc, rc))
        if ACT_TRACE is not None:
            _trace(ACT_LRELU, z, TRACE_GROUPS)
        ctx.save_for_backward(x, w, z)
        ctx.cfg = (stride, ph, pw, slope)
        return z

    @staticmethod
    def backward(ctx, dz):
        x, w, z = ctx.saved_tensors
        stride, ph, pw, slope = ctx.cfg
        g = torch.empty_like(z)
        call("mogan_act_bwd", ptr(z), ptr(_c(dz)), ptr(g), z.shape[0], z.shape[1], z.shape[2] * z.shape[3], ACT_LRELU, slope,
             stream_ptr())
        dx = conv2d_dgrad(g, w, x.shape, stride, ph, pw, 0) if ctx.needs_input_grad[0] else None
        dw = None
        if ctx.needs_input_grad[1]:
            gb = _grad_buf(w)
            if gb is not None:
                _wgrad_accumulate(g, x, w, (stride, ph, pw, 0), gb)
            else:
                dw = conv2d_wgrad(g, x, w.shape, stride, ph, pw, 0)
        return dx, dw, None, None, None, None


class LogitsHeadFn(torch.autograd.Function):
    """p = sigmoid(conv(x, w) + bias).view(-1) for a convolution whose filter covers the whole map (D_GET_LOGITS.outlogits,
    model.py:626-627, 640-641): one launch forward, one backward (mogan_logits_head_*)."""

    @staticmethod
    def forward(ctx, x, w, bias):
        x, w = _c(x), _c(w)
        B, Cout, K = x.shape[0], w.shape[0], w[0].numel()
        p = torch.empty((B, Cout, 1, 1), dtype=torch.float32, device=x.device)
        call("mogan_logits_head_fwd", ptr(x), ptr(w), ptr(_c(bias)) if bias is not None else None, ptr(p), B, K, Cout,
             stream_ptr())
        ctx.save_for_backward(x, w, p)
        ctx.bias_ref = bias
        return p

    @staticmethod
    def backward(ctx, dp):
        x, w, p = ctx.saved_tensors
        bias = ctx.bias_ref
        B, Cout, K = x.shape[0], w.shape[0], w[0].numel()
        dp = _c(dp)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        want_w = ctx.needs_input_grad[1]
        want_b = bias is not None and ctx.needs_input_grad[2]
        gw = _grad_buf(w) if want_w else None
        gb = _grad_buf(bias) if want_b else None
        # one accumulate flag for both: direct only when every wanted gradient has its buffer
        direct = (want_w or want_b) and (not want_w or gw is not None) and (not want_b or gb is not None)
        dw = gw if direct else (torch.empty_like(w) if want_w else None)
        db = (gb if direct else torch.empty_like(bias)) if want_b else None
        call("mogan_logits_head_bwd", ptr(dp), ptr(p), ptr(x), ptr(w), ptr(dx), ptr(dw), ptr(db), B, K, Cout,
             1 if direct else 0, stream_ptr())
        if direct:
            if gw is not None:
                _grad_hit(gw)
            if gb is not None:
                _grad_hit(gb)
            dw = db = None
        return dx, dw, db


def logits_head(x, w, bias):
    return LogitsHeadFn.apply(x, w, bias)


def logits_head_ok(x, conv):
    """conv + Sigmoid as the fused head: the filter covers the whole (unpadded) map, <= 4 logits, K a multiple of 4"""
    w = conv.weight
    ph, pw = conv.padding if isinstance(conv.padding, tuple) else (conv.padding, conv.padding)
    if not (x.dim() == 4 and ph == 0 and pw == 0 and w.shape[2] == x.shape[2] and w.shape[3] == x.shape[3] and w.shape[0] <= 4
            and w[0].numel() % 4 == 0 and x.shape[1] == w.shape[1]):
        return False
    # the kernels read x and w as 16-byte quads: a dense view whose storage offset is not a multiple of four floats (a batch
    # slice of an odd-sized tensor) takes the convolution + sigmoid path instead of failing with MOGAN_ERR_SHAPE
    # (a non-contiguous operand is copied to a fresh, aligned tensor by the Function)
    return (not x.is_contiguous() or x.data_ptr() % 16 == 0) and (not w.is_contiguous() or w.data_ptr() % 16 == 0)


def conv2d_lrelu(x, w, stride, padding, slope=0.2):
    ph, pw = (padding, padding) if isinstance(padding, int) else padding
    return ConvLReLUFn.apply(x, w, int(stride), int(ph), int(pw), float(slope))


def conv2d_affine_relu(x, w, scale, shift, stride=1, padding=0):
    ph, pw = (padding, padding) if isinstance(padding, int) else padding
    return ConvAffineReluFn.apply(x, w, scale, shift, int(stride), int(ph), int(pw))


def conv2d(x, w, bias=None, stride=1, padding=0, up=False):
    ph, pw = (padding, padding) if isinstance(padding, int) else padding
    return Conv2dFn.apply(x, w, bias, int(stride), int(ph), int(pw), 1 if up else 0)


# ------------------------------------------------------------------------------- deep block: conv + BN + activation
DEEP_STATS = {"fwd": 0, "bwd": 0, "panel_hits": 0}
DEEP_ENABLED = True       # 0: packed GEMMs, but BatchNorm / activation as separate launches
_deep_elig = {}


def pk_debug_force(take_all, cfg=-1, split=0):
    """test hook (mogan_pk_debug_force) + the host-side eligibility caches it invalidates"""
    lib.load().mogan_pk_debug_force(int(take_all), int(cfg), int(split))
    _deep_elig.clear()
    _pk_wgrad_elig.clear()


def deep_block_eligible(x, w, stride, ph, pw, act, groups=1):
    """conv -> BatchNorm(train) -> act as the fused deep block (csrc/mogan_pgemm.hip): the weight has packed copies, both
    directions of the convolution take the packed path and the output map is small enough for the one-block-per-8-channels
    tail kernels.  groups: BatchNorm calls the batch stands for (see deep_conv_bn_act)."""
    if not (PK_ENABLED and DEEP_ENABLED) or getattr(w, "_mogan_pk", None) is None or x.dim() != 4:
        return False
    B, Cin, Hs, Ws = x.shape
    Cout, _, KH, KW = w.shape
    key = (B, Cin, Hs, Ws, Cout, KH, KW, stride, ph, pw, act, groups)
    e = _deep_elig.get(key)
    if e is None:
        e = _deep_elig[key] = bool(lib.load().mogan_deep_block_eligible(B, Cin, Hs, Ws, Cout, KH, KW, stride, ph, pw, act,
                                                                        groups))
    if e:
        # one weight used with two convolution geometries has packed copies for the first one only (WeightPacks.pointer
        # returns None for the other): such a call takes the unfused path
        pk = w._mogan_pk
        for d in (0, 1):
            slot = pk.slots.get(d)
            if slot is not None and slot.geom != (stride, ph, pw):
                return False
    return e


class DeepConvBNActFn(torch.autograd.Function):
    """z = act(BatchNorm2d_train(conv2d(x, w))) for the deep discriminator layers (model.py:575-613: downBlock,
    Block3x3_leakRelu; 616-642: jointConv) in two launches forward (packed-weight GEMM, tail) and two + the weight gradient
    backward.  The output carries the pixel panel of z for the next deep block (attribute _mogan_panel).  groups = 2: the batch
    is [real; fake] of a discriminator update (miscc/losses.py:136-174) -- one convolution, BatchNorm statistics per half."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, running_mean, running_var, act, slope, eps, momentum, stride, ph, pw, groups):
        x, gamma, beta = _c(x), _c(gamma), _c(beta)
        B, Cin, Hs, Ws = x.shape
        Cout, _, KH, KW = w.shape
        OH, OW = conv_out_hw(Hs, Ws, KH, KW, stride, ph, pw, 0)
        dev = x.device
        pk = w._mogan_pk
        wp = pk.pointer(0, B, Hs, Ws, stride, ph, pw)
        if wp is None:          # (deep_block_eligible checks both directions; a NULL panel must never reach the kernel)
            raise lib.MoganHipError("deep block: no packed forward copy of this weight for geometry %r" % ((stride, ph, pw),))
        f32 = dict(dtype=torch.float32, device=dev)
        y = torch.empty((B, Cout, OH, OW), **f32)
        z = torch.empty((B, Cout, OH, OW), **f32)
        stats = torch.empty((2, groups, Cout), **f32)
        zpanel = torch.empty(int(lib.load().mogan_pk_panel_bytes(B, Cout, OH * OW)), dtype=torch.uint8, device=dev)
        xp = getattr(x, "_mogan_panel", None)
        if xp is not None and (xp[1] != x.data_ptr() or xp[2] != x._version):
            xp = None                                    # not the panel of these values
        if xp is not None:
            DEEP_STATS["panel_hits"] += 1
        wsp, wsn = workspace(dev)
        if BN_DEFER is not None:
            if groups != 1:
                raise lib.MoganHipError("deferred running statistics: one BatchNorm call per launch only")
            BN_DEFER.append((stats[0, 0], stats[1, 0], B * OH * OW, running_mean, running_var, eps, momentum))
            running_mean = running_var = None
        call("mogan_deep_conv_bn_act_fwd", ptr(x), ptr(xp[0]) if xp is not None else None, wp, ptr(gamma), ptr(beta),
             ptr(running_mean), ptr(running_var), ptr(y), ptr(stats), ptr(z), ptr(zpanel), B, Cin, Hs, Ws, Cout, KH, KW,
             stride, ph, pw, eps, momentum, act, slope, groups, wsp, wsn, stream_ptr())
        DEEP_STATS["fwd"] += 1
        if ACT_TRACE is not None and act in (ACT_RELU, ACT_LRELU):
            _trace(act, z, groups)
        ctx.save_for_backward(x, w, y, stats, gamma, beta)
        ctx.cfg = (act, slope, stride, ph, pw, groups)
        z._mogan_panel = (zpanel, z.data_ptr(), z._version)
        return z

    @staticmethod
    def backward(ctx, dz):
        x, w, y, stats, gamma, beta = ctx.saved_tensors
        act, slope, stride, ph, pw, groups = ctx.cfg
        dz = _c(dz)
        B, Cin, Hs, Ws = x.shape
        Cout, _, KH, KW = w.shape
        dev = x.device
        dy = torch.empty_like(y)
        want_dx = ctx.needs_input_grad[0]
        dx = torch.empty(x.shape, dtype=torch.float32, device=dev) if want_dx else None
        wpd = w._mogan_pk.pointer(1, B, Hs, Ws, stride, ph, pw) if want_dx else None
        if want_dx and wpd is None:
            raise lib.MoganHipError("deep block: no packed data-gradient copy of this weight for geometry %r" % ((stride, ph, pw),))
        gg, gb = _grad_buf(gamma), _grad_buf(beta)
        want_gb = ctx.needs_input_grad[2] or ctx.needs_input_grad[3]
        direct = gg is not None and gb is not None and ctx.needs_input_grad[2] and ctx.needs_input_grad[3]
        dg = db = None
        if direct:
            pg, pb = gg, gb
        elif want_gb:
            dgb = torch.empty((2, Cout), dtype=torch.float32, device=dev)
            pg, pb = dgb[0], dgb[1]
        else:
            pg = pb = None
        wsp, wsn = workspace(dev)
        call("mogan_deep_conv_bn_act_bwd", ptr(dz), ptr(y), ptr(stats), ptr(gamma), ptr(beta), wpd, ptr(dy), ptr(pg), ptr(pb),
             1 if direct else 0, ptr(dx), B, Cin, Hs, Ws, Cout, KH, KW, stride, ph, pw, act, slope, groups, wsp, wsn,
             stream_ptr())
        DEEP_STATS["bwd"] += 1
        if direct:
            _grad_hit(gg)
            _grad_hit(gb)
        elif want_gb:
            dg, db = pg, pb
        dw = None
        if ctx.needs_input_grad[1]:
            g = _grad_buf(w)
            if g is not None:
                _wgrad_accumulate(dy, x, w, (stride, ph, pw, 0), g)
            else:
                dw = conv2d_wgrad(dy, x, w.shape, stride, ph, pw, 0)
        return (dx, dw, dg, db) + (None,) * 10


def deep_conv_bn_act(x, w, gamma, beta, running_mean, running_var, act, slope, eps, momentum, stride, ph, pw, groups=1):
    return DeepConvBNActFn.apply(x, w, gamma, beta, running_mean, running_var, int(act), float(slope), float(eps),
                                 float(momentum), int(stride), int(ph), int(pw), int(groups))


# ------------------------------------------------------------------------------- strided bmm / linear
def bmm_raw(a, b, out, accumulate=False):
    """out[z] (+)= a[z] @ b[z] for 3-D strided views (no copies)."""
    Z_, M, K = a.shape
    N = b.shape[2]
    wsp, wsn = workspace(a.device)
    call("mogan_bmm", ptr(a), ptr(b), ptr(out), Z_, M, N, K,
         a.stride(0), a.stride(1), a.stride(2), b.stride(0), b.stride(1), b.stride(2),
         out.stride(0), out.stride(1), out.stride(2), 1 if accumulate else 0, wsp, wsn, stream_ptr())
    return out


class BmmFn(torch.autograd.Function):
    """(Z,M,K) x (Z,K,N) -> (Z,M,N); inputs may be arbitrary strided views (torch.bmm call sites of
    GlobalAttention.py:46,66)."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = a.float(), b.float()
        out = torch.empty((a.shape[0], a.shape[1], b.shape[2]), dtype=torch.float32, device=a.device)
        bmm_raw(a, b, out)
        ctx.save_for_backward(a, b)
        return out

    @staticmethod
    def backward(ctx, dout):
        a, b = ctx.saved_tensors
        dout = _c(dout)
        da = db = None
        if ctx.needs_input_grad[0]:
            da = torch.empty(a.shape, dtype=torch.float32, device=a.device)
            bmm_raw(dout, b.transpose(1, 2), da)
        if ctx.needs_input_grad[1]:
            db = torch.empty(b.shape, dtype=torch.float32, device=a.device)
            bmm_raw(a.transpose(1, 2), dout, db)
        return da, db


def bmm(a, b):
    return BmmFn.apply(a, b)


class LinearFn(torch.autograd.Function):
    """y = x @ w.T (+ bias); nn.Linear at model.py:324,365,371."""

    @staticmethod
    def forward(ctx, x, w, bias):
        x, w = _c(x), _c(w)
        y = torch.empty((x.shape[0], w.shape[0]), dtype=torch.float32, device=x.device)
        bmm_raw(x.unsqueeze(0), w.t().unsqueeze(0), y.unsqueeze(0))
        if bias is not None:
            call("mogan_bias_add", ptr(y), ptr(_c(bias)), y.shape[0], y.shape[1], 1, stream_ptr())
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        ctx.bias_ref = bias
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = _c(dy)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
            bmm_raw(dy.unsqueeze(0), w.unsqueeze(0), dx.unsqueeze(0))
        if ctx.needs_input_grad[1]:
            g = _grad_buf(w)
            if g is not None:
                bmm_raw(dy.t().unsqueeze(0), x.unsqueeze(0), g.unsqueeze(0), accumulate=True)
                _grad_hit(g)
            else:
                dw = torch.empty(w.shape, dtype=torch.float32, device=x.device)
                bmm_raw(dy.t().unsqueeze(0), x.unsqueeze(0), dw.unsqueeze(0))
        if ctx.has_bias and ctx.needs_input_grad[2]:
            g = _grad_buf(ctx.bias_ref)
            db = g if g is not None else torch.empty(dy.shape[1], dtype=torch.float32, device=dy.device)
            call("mogan_bias_grad", ptr(dy), ptr(db), dy.shape[0], dy.shape[1], 1, 1 if g is not None else 0,
                 stream_ptr())
            if g is not None:
                db = None
                _grad_hit(g)
        return dx, dw, db


def linear(x, w, bias=None):
    return LinearFn.apply(x, w, bias)


# ------------------------------------------------------------------------------- batch norm (+act)
def _bchw(x):
    if x.dim() == 2:
        return x.shape[0], x.shape[1], 1
    return x.shape[0], x.shape[1], x[0, 0].numel()


class BNActFn(torch.autograd.Function):
    """`groups` training-mode BatchNorm1d/2d calls fused with GLU / LeakyReLU / ReLU on the groups of B images of one
    (groups*B, C, ...) tensor (model.py:52-54,72-80,96-101,366-373,577-611).  Every group has its own batch statistics and updates
    the running statistics in place like nn.BatchNorm does (momentum 0.1, unbiased variance), group after group.  groups == 1 is the
    plain call, which may add a residual; groups > 1 are the per-object calls of the object pathways (model.py:395-407, 662-672;
    SURVEY F11) and the [real; fake] batch of a discriminator update (miscc/losses.py:136-174).
    Launches: where bn_groups_ok, all groups in ONE launch each way.  Otherwise the entry points of the plain call once per group on
    the group's slice of x / y (the groups are contiguous: no copies, no concatenation): small maps (<= 4096 values per channel)
    take ONE launch (a block per channel reduces, finalises and applies), larger ones two (partial sums; apply with the reduction
    of the partial sums folded in: per wave, an xor-butterfly, no barrier -- round 2's version of that fold, every block
    re-reducing behind a barrier, was 3 % slower in the step and dropped; this one is +0.3 %), planes whose size is not a
    multiple of 4 three."""

    @staticmethod
    def forward(ctx, x, gamma, beta, residual, running_mean, running_var, act, slope, eps, momentum, groups):
        x, gamma, beta = _c(x), _c(gamma), _c(beta)
        N, C, HW = _bchw(x)
        B = N // groups
        dev = x.device
        stats = torch.empty((2, groups, C), dtype=torch.float32, device=dev)
        Cy = C // 2 if act == ACT_GLU else C
        y = torch.empty((N, Cy) + tuple(x.shape[2:]), dtype=torch.float32, device=dev)
        one = bn_groups_ok(x, groups)
        if BN_DEFER is not None:
            if groups > 1:
                raise lib.MoganHipError("deferred running statistics: one BatchNorm call per launch only")
            BN_DEFER.append((stats[0, 0], stats[1, 0], B * HW, running_mean, running_var, eps, momentum))
            running_mean = running_var = None
        if one:
            call("mogan_bn_act_grouped_fwd", ptr(x), ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var), ptr(stats[0]),
                 ptr(stats[1]), ptr(y), groups, B, C, HW, act, slope, eps, momentum, stream_ptr())
        else:
            need = lib.bn_ws_bytes(B, C, HW)
            wsp, wsn = workspace(dev)
            if need > wsn:
                raise lib.MoganHipError("workspace too small for bn (%d > %d)" % (need, wsn))
            res = _c(residual) if residual is not None else None
            for g in range(groups):
                call("mogan_bn_act_fwd_fused", ptr(x[g * B:(g + 1) * B]), ptr(gamma), ptr(beta), ptr(res), ptr(running_mean),
                     ptr(running_var), ptr(stats[0, g]), ptr(stats[1, g]), ptr(y[g * B:(g + 1) * B]), B, C, HW, act, slope, eps,
                     momentum, wsp, wsn, stream_ptr())
        if ACT_TRACE is not None and act in (ACT_RELU, ACT_LRELU):
            _trace(act, y, groups)                       # (one entry per reference call, in call order)
        ctx.save_for_backward(x, gamma, beta, stats)
        ctx.cfg = (act, slope, groups, one, residual is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, beta, stats = ctx.saved_tensors
        act, slope, groups, one, has_res = ctx.cfg
        dy = _c(dy)
        N, C, HW = _bchw(x)
        B = N // groups
        dx = torch.empty_like(x)
        gg, gb = _grad_buf(gamma), _grad_buf(beta)
        direct = gg is not None and gb is not None and ctx.needs_input_grad[1] and ctx.needs_input_grad[2]
        loop_adds = groups > 1 and not one                   # (the per-group calls accumulate: into zeros, if into a buffer of ours)
        if direct:
            dg, db = gg, gb
        else:
            dgb = (torch.zeros if loop_adds else torch.empty)((2, C), dtype=torch.float32, device=x.device)
            dg, db = dgb[0], dgb[1]
        accumulate = 1 if direct or loop_adds else 0
        if one:
            call("mogan_bn_act_grouped_bwd", ptr(x), ptr(dy), ptr(stats[0]), ptr(stats[1]), ptr(gamma), ptr(beta), ptr(dx),
                 ptr(dg), ptr(db), groups, B, C, HW, act, slope, accumulate, stream_ptr())
        else:
            wsp, wsn = workspace(x.device)
            for g in range(groups):
                call("mogan_bn_act_bwd", ptr(x[g * B:(g + 1) * B]), ptr(dy[g * B:(g + 1) * B]), ptr(stats[0, g]), ptr(stats[1, g]),
                     ptr(gamma), ptr(beta), ptr(dx[g * B:(g + 1) * B]), ptr(dg), ptr(db), B, C, HW, act, slope, accumulate, wsp,
                     wsn, stream_ptr())
        if direct:
            _grad_hit(gg)
            _grad_hit(gb)
            dg = db = None
        return dx, dg, db, (dy if has_res else None), None, None, None, None, None, None, None


def bn_groups_ok(x, groups):
    """can `groups` BatchNorm calls on this (groups*B, C, ...) tensor go out as ONE launch (B*HW <= 4096 values per channel)?
    (bn_act(groups=...) itself takes any size: larger maps run the two-launch kernels per group, in place)"""
    N, C, HW = _bchw(x)
    return groups > 1 and N % groups == 0 and bool(lib.load().mogan_bn_act_grouped_eligible(groups, N // groups, C, HW))


def bn_act(x, gamma, beta, running_mean, running_var, act=ACT_NONE, slope=0.2, residual=None, eps=1e-5,
           momentum=0.1, groups=1):
    assert groups == 1 or residual is None
    return BNActFn.apply(x, gamma, beta, residual, running_mean, running_var, act, float(slope), float(eps), float(momentum),
                         int(groups))


class AffineActFn(torch.autograd.Function):
    """Eval-mode BN (running statistics folded into scale/shift) + activation; only dx is produced
    (frozen Inception trunk of CNN_ENCODER, model.py:218-219,227-242)."""

    @staticmethod
    def forward(ctx, x, scale, shift, act, slope):
        x = _c(x)
        B, C, HW = _bchw(x)
        y = torch.empty_like(x)
        call("mogan_affine_act_fwd", ptr(x), ptr(scale), ptr(shift), ptr(y), B, C, HW, act, slope, stream_ptr())
        ctx.save_for_backward(x, scale, shift)
        ctx.cfg = (act, slope)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, scale, shift = ctx.saved_tensors
        act, slope = ctx.cfg
        B, C, HW = _bchw(x)
        dx = torch.empty_like(x)
        call("mogan_affine_act_bwd", ptr(x), ptr(_c(dy)), ptr(scale), ptr(shift), ptr(dx), B, C, HW, act, slope,
             stream_ptr())
        return dx, None, None, None, None


def affine_act(x, scale, shift, act=ACT_RELU, slope=0.0):
    return AffineActFn.apply(x, scale, shift, act, float(slope))


# ------------------------------------------------------------------------------- activations
class ActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, act, slope):
        x = _c(x)
        B, C, HW = _bchw(x)
        Cy = C // 2 if act == ACT_GLU else C
        y = torch.empty((B, Cy) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
        call("mogan_act_fwd", ptr(x), ptr(y), B, C, HW, act, slope, stream_ptr())
        if ACT_TRACE is not None and act in (ACT_RELU, ACT_LRELU):
            ACT_TRACE.append((act, y))
        ctx.save_for_backward(x)
        ctx.cfg = (act, slope)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        act, slope = ctx.cfg
        B, C, HW = _bchw(x)
        dx = torch.empty_like(x)
        call("mogan_act_bwd", ptr(x), ptr(_c(dy)), ptr(dx), B, C, HW, act, slope, stream_ptr())
        return dx, None, None


def act(x, kind, slope=0.2):
    return ActFn.apply(x, kind, float(slope))


def glu(x):
    return ActFn.apply(x, ACT_GLU, 0.0)


class AddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a, b = _c(a), _c(b)
        y = torch.empty_like(a)
        call("mogan_add", ptr(a), ptr(b), ptr(y), a.numel(), stream_ptr())
        return y

    @staticmethod
    def backward(ctx, dy):
        return dy, dy


def add(a, b):
    return AddFn.apply(a, b)


class GroupSumFn(torch.autograd.Function):
    """(G*B, ...) -> (B, ...): x_0 + x_1 + ... over the G groups of B samples, in that order (model.py:113,406,671)."""

    @staticmethod
    def forward(ctx, x, G):
        x = _c(x)
        y = torch.empty((x.shape[0] // G,) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
        call("mogan_group_sum", ptr(x), ptr(y), y.numel(), G, stream_ptr())
        ctx.G = G
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _c(dy)
        dx = torch.empty((dy.shape[0] * ctx.G,) + tuple(dy.shape[1:]), dtype=torch.float32, device=dy.device)
        call("mogan_group_bcast", ptr(dy), ptr(dx), dy.numel(), ctx.G, stream_ptr())
        return dx, None


def group_sum(x, G):
    return GroupSumFn.apply(x, int(G))


# ------------------------------------------------------------------------------- softmax
class SoftmaxFn(torch.autograd.Function):
    """softmax(scale * x) over `dim`, optionally restricted to the first lens[...] entries of each
    column (DAMSM: captions of different lengths).  GlobalAttention.py:50,58."""

    @staticmethod
    def forward(ctx, x, dim, scale, lens):
        x = _c(x)
        dim = dim % x.dim()
        outer = 1
        for s in x.shape[:dim]:
            outer *= s
        inner = 1
        for s in x.shape[dim + 1:]:
            inner *= s
        L = x.shape[dim]
        y = torch.empty_like(x)
        call("mogan_softmax_fwd", ptr(x), ptr(y), ptr(lens), outer, L, inner, scale, stream_ptr())
        ctx.save_for_backward(y)
        ctx.lens = lens
        ctx.cfg = (outer, L, inner, scale)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        outer, L, inner, scale = ctx.cfg
        dx = torch.empty_like(y)
        call("mogan_softmax_bwd", ptr(y), ptr(_c(dy)), ptr(dx), ptr(ctx.lens), outer, L, inner, scale, stream_ptr())
        return dx, None, None, None


def softmax(x, dim, scale=1.0, lens=None):
    return SoftmaxFn.apply(x, dim, float(scale), lens)


# ------------------------------------------------------------------------------- spatial transformer
class STNFn(torch.autograd.Function):
    """model.py:17-21 (affine_grid + grid_sample, bilinear, zeros)."""

    @staticmethod
    def forward(ctx, x, theta, Hout, Wout, align_corners):
        x, theta = _c(x), _c(theta)
        B, C, Hin, Win = x.shape
        y = torch.empty((B, C, Hout, Wout), dtype=torch.float32, device=x.device)
        call("mogan_stn_fwd", ptr(x), ptr(theta), ptr(y), B, C, Hin, Win, Hout, Wout, align_corners, stream_ptr())
        ctx.save_for_backward(theta)
        ctx.cfg = (B, C, Hin, Win, Hout, Wout, align_corners)
        return y

    @staticmethod
    def backward(ctx, dy):
        (theta,) = ctx.saved_tensors
        B, C, Hin, Win, Hout, Wout, ac = ctx.cfg
        dx = torch.empty((B, C, Hin, Win), dtype=torch.float32, device=dy.device)
        call("mogan_stn_bwd", ptr(_c(dy)), ptr(theta), ptr(dx), B, C, Hin, Win, Hout, Wout, ac, stream_ptr())
        return dx, None, None, None, None


def stn(x, theta, size, align_corners=False):
    return STNFn.apply(x, theta, int(size[2]), int(size[3]), 1 if align_corners else 0)


class STNSharedFn(torch.autograd.Function):
    """stn() whose source is shared between the objects or constant over the plane, without the materialised copies
    (include/mogan_hip.h: mogan_stn_*_ex): x (xB, C, Hin, Win) read by sample b as image b % xB, or -- plane -- x (xB, C), the
    label vector the reference repeats over Hin x Win first (model.py:109-111, 663-665).  theta (B', G, 2, 3) in the loader's
    order when theta_G = G (samples are object-major), else (N, 2, 3)."""

    @staticmethod
    def forward(ctx, x, theta, N, Hin, Win, Hout, Wout, align_corners, plane, theta_G):
        x, theta = _c(x), _c(theta)
        xB, C = x.shape[0], x.shape[1]
        y = torch.empty((N, C, Hout, Wout), dtype=torch.float32, device=x.device)
        call("mogan_stn_fwd_ex", ptr(x), ptr(theta), ptr(y), N, C, Hin, Win, Hout, Wout, align_corners, xB, plane, theta_G,
             stream_ptr())
        ctx.save_for_backward(theta)
        ctx.cfg = (N, C, Hin, Win, Hout, Wout, align_corners, xB, plane, theta_G, tuple(x.shape))
        return y

    @staticmethod
    def backward(ctx, dy):
        (theta,) = ctx.saved_tensors
        N, C, Hin, Win, Hout, Wout, ac, xB, plane, theta_G, xshape = ctx.cfg
        dx = torch.empty(xshape, dtype=torch.float32, device=dy.device)
        call("mogan_stn_bwd_ex", ptr(_c(dy)), ptr(theta), ptr(dx), N, C, Hin, Win, Hout, Wout, ac, xB, plane, theta_G,
             stream_ptr())
        return (dx,) + (None,) * 9


def stn_shared(x, theta, N, in_hw, out_hw, align_corners=False, plane=False, theta_G=0):
    return STNSharedFn.apply(x, theta, int(N), int(in_hw[0]), int(in_hw[1]), int(out_hw[0]), int(out_hw[1]),
                             1 if align_corners else 0, 1 if plane else 0, int(theta_G))


# ------------------------------------------------------------------------------- channel concat with broadcast sources
class CatFn(torch.autograd.Function):
    """torch.cat(parts, 1) where a part may be a code repeated over the plane, one tensor repeated for every object, or the
    per-object slices of a (B, G, C) tensor in the object-major batch -- one launch each way (mogan_concat_fwd / _bwd; model.py:
    400-401, 418, 457, 633-634, 666, 703).  meta[i] = (C, rows, sb, sg, bcast) of part i."""

    @staticmethod
    def forward(ctx, meta, N, spatial, *parts):
        import ctypes
        parts = [_c(t) for t in parts]
        n = len(parts)
        HW = 1
        for d in spatial:
            HW *= d
        Ctot = sum(m[0] for m in meta)
        dst = torch.empty((N, Ctot) + tuple(spatial), dtype=torch.float32, device=parts[0].device)
        arrs = _cat_arrays(meta, [t.data_ptr() for t in parts])
        call("mogan_concat_fwd", *arrs, n, ptr(dst), N, HW, stream_ptr())
        ctx.cfg = (meta, N, HW, [tuple(t.shape) for t in parts])
        return dst

    @staticmethod
    def backward(ctx, ddst):
        meta, N, HW, shapes = ctx.cfg
        ddst = _c(ddst)
        grads = [torch.empty(shp, dtype=torch.float32, device=ddst.device) if ctx.needs_input_grad[3 + i] else None
                 for i, shp in enumerate(shapes)]
        if any(g is not None for g in grads):
            arrs = _cat_arrays(meta, [g.data_ptr() if g is not None else None for g in grads])
            call("mogan_concat_bwd", ptr(ddst), *arrs, len(shapes), N, HW, stream_ptr())
        return (None, None, None) + tuple(grads)


def _cat_arrays(meta, pointers):
    import ctypes
    n = len(meta)
    pp = (ctypes.c_void_p * n)(*pointers)
    cc = (ctypes.c_int * n)(*[m[0] for m in meta])
    rr = (ctypes.c_int * n)(*[m[1] for m in meta])
    sb = (ctypes.c_longlong * n)(*[m[2] for m in meta])
    sg = (ctypes.c_longlong * n)(*[m[3] for m in meta])
    bc = (ctypes.c_int * n)(*[m[4] for m in meta])
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)
    return cast(pp), cast(cc), cast(rr), cast(sb), cast(sg), cast(bc)


def cat_channels(parts, N, spatial=()):
    """parts: list of (tensor, mode); mode = "full" (N, C, *spatial) | "plane" (N, C) | ("rep", G) (N/G, C, *spatial) repeated for
    G objects | ("rep_plane", G) (N/G, C) | ("obj", G) (B, G, C, *spatial), batch n = g B + b | ("obj_plane", G) (B, G, C).
    Returns the (N, sum C, *spatial) concatenation."""
    HW = 1
    for d in spatial:
        HW *= int(d)
    meta, ts = [], []
    for t, mode in parts:
        kind, G = (mode, 1) if isinstance(mode, str) else mode
        if kind == "full":
            C = t.shape[1]; m = (C, N, C * HW, 0, 0)
        elif kind == "plane":
            C = t.shape[1]; m = (C, N, C, 0, 1)
        elif kind == "rep":
            C = t.shape[1]; m = (C, N // G, C * HW, 0, 0)
        elif kind == "rep_plane":
            C = t.shape[1]; m = (C, N // G, C, 0, 1)
        elif kind == "obj":
            C = t.shape[2]; m = (C, N // G, G * C * HW, C * HW, 0)
        elif kind == "obj_plane":
            C = t.shape[2]; m = (C, N // G, G * C, C, 1)
        else:
            raise ValueError(mode)
        want = {"full": N, "plane": N, "rep": N // G, "rep_plane": N // G, "obj": N // G, "obj_plane": N // G}[kind]
        lead = 3 if kind.startswith("obj") else 2                 # (batch[, object], channel) in front of the plane
        tail = () if kind.endswith("plane") else tuple(int(d) for d in spatial)
        # the kernels index every part with the destination's plane size: a part whose trailing dims differ would be read out
        # of bounds where torch.cat raises a shape error
        if (t.shape[0] != want or (kind.startswith("obj") and t.shape[1] != G) or t.dim() != lead + len(tail)
                or tuple(t.shape[lead:]) != tail):
            raise lib.MoganHipError("cat_channels: part of shape %r does not fit mode %r at N = %d, plane %r"
                                    % (tuple(t.shape), mode, N, tuple(spatial)))
        meta.append(m)
        ts.append(t)
    if len(ts) > 4:
        raise lib.MoganHipError("cat_channels: at most 4 parts")
    return CatFn.apply(tuple(meta), int(N), tuple(int(d) for d in spatial), *ts)


def bbox_to_theta(bbox):
    bbox = _c(bbox).view(-1, 4)
    n = bbox.shape[0]
    th = torch.empty((n, 2, 3), dtype=torch.float32, device=bbox.device)
    thi = torch.empty((n, 2, 3), dtype=torch.float32, device=bbox.device)
    call("mogan_bbox_to_theta", ptr(bbox), ptr(th), ptr(thi), n, stream_ptr())
    return th, thi


# ------------------------------------------------------------------------------- word attention
class AttnFn(torch.autograd.Function):
    """GlobalAttention.py:96-121 after conv_context. h (B,idf,Q), src (B,idf,T), mask (B,T) uint8."""

    @staticmethod
    def forward(ctx, h, src, mask, mask_mode):
        h, src = _c(h), _c(src)
        B, idf, Q = h.shape
        T = src.shape[2]
        wc = torch.empty((B, idf, Q), dtype=torch.float32, device=h.device)
        attn = torch.empty((B, T, Q), dtype=torch.float32, device=h.device)
        call("mogan_attn_fwd", ptr(h), ptr(src), ptr(mask), ptr(wc), ptr(attn), B, idf, Q, T, mask_mode,
             stream_ptr())
        ctx.save_for_backward(h, src, attn)
        return wc, attn

    @staticmethod
    def backward(ctx, dwc, dattn):
        h, src, attn = ctx.saved_tensors
        B, idf, Q = h.shape
        T = src.shape[2]
        dwc = _c(dwc)
        dattn = _c(dattn) if dattn is not None else None
        dh = torch.empty_like(h)
        dscore = torch.empty_like(attn)
        call("mogan_attn_bwd", ptr(src), ptr(attn), ptr(dwc), ptr(dattn), ptr(dh), ptr(dscore), B, idf, Q, T,
             stream_ptr())
        dsrc = None
        if ctx.needs_input_grad[1]:
            dsrc = torch.empty_like(src)
            bmm_raw(h, dscore.transpose(1, 2), dsrc)                    # (B,idf,Q) x (B,Q,T)
            bmm_raw(dwc, attn.transpose(1, 2), dsrc, accumulate=True)
        return dh, dsrc, None, None


def attention(h, src, mask=None, mask_mode=0):
    if mask is not None:
        mask = mask.to(torch.uint8).contiguous()
    return AttnFn.apply(h, src, mask, mask_mode)


# ------------------------------------------------------------------------------- losses
class BCEFn(torch.autograd.Function):
    """nn.BCELoss()(p, const target) (miscc/losses.py:158-168,198-201)."""

    @staticmethod
    def forward(ctx, p, target):
        p = _c(p).view(-1)
        loss = torch.empty(1, dtype=torch.float32, device=p.device)
        call("mogan_bce_fwd", ptr(p), target, 1.0, ptr(loss), p.numel(), 0, stream_ptr())
        ctx.save_for_backward(p)
        ctx.target = target
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        (p,) = ctx.saved_tensors
        dp = torch.empty_like(p)
        call("mogan_bce_bwd", ptr(p), ctx.target, 1.0, ptr(_c(g).view(1)), ptr(dp), p.numel(), stream_ptr())
        return dp, None


def bce(p, target):
    return BCEFn.apply(p, float(target))


class BCELogitsFn(torch.autograd.Function):
    """nn.BCEWithLogitsLoss()(x, const target) (code/coco/stackgan/miscc/utils.py:73,114)."""

    @staticmethod
    def forward(ctx, x, target):
        x = _c(x).view(-1)
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        call("mogan_bce_logits_fwd", ptr(x), target, 1.0, ptr(loss), x.numel(), 0, stream_ptr())
        ctx.save_for_backward(x)
        ctx.target = target
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        dx = torch.empty_like(x)
        call("mogan_bce_logits_bwd", ptr(x), ctx.target, 1.0, ptr(_c(g).view(1)), ptr(dx), x.numel(), stream_ptr())
        return dx, None


def bce_with_logits(x, target):
    return BCELogitsFn.apply(x, float(target))


class KLFn(torch.autograd.Function):
    """KL_loss (miscc/losses.py:230-234)."""

    @staticmethod
    def forward(ctx, mu, logvar):
        mu, logvar = _c(mu), _c(logvar)
        loss = torch.empty(1, dtype=torch.float32, device=mu.device)
        call("mogan_kl_fwd", ptr(mu), ptr(logvar), ptr(loss), mu.numel(), stream_ptr())
        ctx.save_for_backward(mu, logvar)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        mu, logvar = ctx.saved_tensors
        dmu, dlv = torch.empty_like(mu), torch.empty_like(logvar)
        call("mogan_kl_bwd", ptr(mu), ptr(logvar), ptr(_c(g).view(1)), ptr(dmu), ptr(dlv), mu.numel(), stream_ptr())
        return dmu, dlv


def kl_loss(mu, logvar):
    return KLFn.apply(mu, logvar)


class ReparamFn(torch.autograd.Function):
    """CA_NET.reparametrize (model.py:333-340)."""

    @staticmethod
    def forward(ctx, mu, logvar, eps):
        mu, logvar, eps = _c(mu), _c(logvar), _c(eps)
        c = torch.empty_like(mu)
        call("mogan_reparam_fwd", ptr(mu), ptr(logvar), ptr(eps), ptr(c), mu.numel(), stream_ptr())
        ctx.save_for_backward(logvar, eps)
        return c

    @staticmethod
    def backward(ctx, dc):
        logvar, eps = ctx.saved_tensors
        dmu, dlv = torch.empty_like(logvar), torch.empty_like(logvar)
        call("mogan_reparam_bwd", ptr(logvar), ptr(eps), ptr(_c(dc)), ptr(dmu), ptr(dlv), logvar.numel(), stream_ptr())
        return dmu, dlv, None


def reparam(mu, logvar, eps):
    return ReparamFn.apply(mu, logvar, eps)


# ------------------------------------------------------------------------------- DAMSM matching losses
def _scalar(device):
    return torch.empty((), dtype=torch.float32, device=device)


def _g_ptr(g):
    """Pointer of a 0-dim upstream gradient (None -> NULL: that output did not take part in the loss)."""
    return ptr(_c(g)) if g is not None else None


class _PairCE:
    """Shared tail of the word and the sentence loss: the two cross-entropies over a (B,B) similarity matrix."""

    @staticmethod
    def forward(ctx, sim, labels, mask):
        R = sim.shape[0]
        dev = sim.device
        prow, pcol = torch.empty_like(sim), torch.empty_like(sim)
        nll = torch.empty(2 * R, dtype=torch.float32, device=dev)
        out2 = torch.empty(2, dtype=torch.float32, device=dev)
        call("mogan_damsm_ce_fwd", ptr(sim), ptr(labels), ptr(mask), R, sim.shape[1], ptr(prow), ptr(pcol), ptr(nll),
             ptr(out2), stream_ptr())
        ctx.ce = (prow, pcol, labels)
        return out2[0], out2[1]

    @staticmethod
    def backward(ctx, g0, g1):
        prow, pcol, labels = ctx.ce
        dsim = torch.empty_like(prow)
        call("mogan_damsm_ce_bwd", ptr(prow), ptr(pcol), ptr(labels), _g_ptr(g0), _g_ptr(g1), prow.shape[0], prow.shape[1],
             ptr(dsim), stream_ptr())
        return dsim


class DamsmWordsFn(torch.autograd.Function):
    """words_loss for all (image, caption) pairs (miscc/losses.py:62-132, GlobalAttention.py:31-69) -> (loss0, loss1,
    attention a2 (B,Bc,T,S)).  Gradients: the region features, and -- when they ask for one (DAMSM pre-training) -- the word
    embeddings (mogan_damsm_words_bwd_text + one mogan_bmm per image for the path through the attention scores)."""

    @staticmethod
    def forward(ctx, feat, words, lens, labels, mask, g1, g2, g3):
        feat, words = _c(feat), _c(words)
        B, C = feat.shape[0], feat.shape[1]
        S = feat[0, 0].numel()
        Bc, T = words.shape[0], words.shape[2]
        dev = feat.device
        f32 = dict(dtype=torch.float32, device=dev)
        sim = torch.empty((B, Bc), **f32)
        a1, a2 = torch.empty((B, Bc, S, T), **f32), torch.empty((B, Bc, T, S), **f32)
        wc, wt = torch.empty((B, C, Bc, T), **f32), torch.empty((C, Bc, T), **f32)
        call("mogan_damsm_words_fwd", ptr(feat), ptr(words), ptr(lens), B, Bc, C, S, T, g1, g2, g3, ptr(sim), ptr(a1),
             ptr(a2), ptr(wc), ptr(wt), stream_ptr())
        l0, l1 = _PairCE.forward(ctx, sim, labels, mask)
        ctx.save_for_backward(feat, words, a1, a2, wc, wt)
        ctx.cfg = (lens, g1, g2, g3)
        ctx.mark_non_differentiable(a2)
        return l0, l1, a2

    @staticmethod
    def backward(ctx, gl0, gl1, _ga2):
        feat, words, a1, a2, wc, wt = ctx.saved_tensors
        lens, g1, g2, g3 = ctx.cfg
        B, C = feat.shape[0], feat.shape[1]
        S = feat[0, 0].numel()
        Bc, T = words.shape[0], words.shape[2]
        dsim = _PairCE.backward(ctx, gl0, gl1)
        dwc = torch.empty_like(wc)
        dst = torch.empty_like(a2)
        call("mogan_damsm_words_bwd", ptr(feat), ptr(words), ptr(lens), ptr(a1), ptr(a2), ptr(wc), ptr(dsim), B, Bc, C, S, T,
             g1, g2, g3, ptr(dwc), ptr(dst), stream_ptr())
        dfeat = dwords = None
        if ctx.needs_input_grad[0]:
            dfeat = torch.empty_like(feat)
            out = dfeat.view(B, C, S)
            bmm_raw(dwc.view(B, C, Bc * T), a2.view(B, Bc * T, S), out)
            bmm_raw(wt.view(1, C, Bc * T).expand(B, C, Bc * T), dst.view(B, Bc * T, S), out, accumulate=True)
        if ctx.needs_input_grad[1]:
            dwords = torch.empty_like(words)
            call("mogan_damsm_words_bwd_text", ptr(words), ptr(lens), ptr(wc), ptr(dsim), B, Bc, C, T, g2, g3, ptr(dwords),
                 stream_ptr())
            fv = feat.view(B, C, S)
            for b in range(B):          # dwords[i] (C,T) += ctx[b] (C,S) . dscore_t[b,i] (T,S)^T, the images in index order
                bmm_raw(fv[b:b + 1].expand(Bc, C, S), dst[b].transpose(1, 2), dwords, accumulate=True)
        return dfeat, dwords, None, None, None, None, None, None


def damsm_words(feat, words, lens, labels, mask, gamma1, gamma2, gamma3):
    return DamsmWordsFn.apply(feat, words, lens, labels, mask, float(gamma1), float(gamma2), float(gamma3))


class DamsmSentFn(torch.autograd.Function):
    """sent_loss (miscc/losses.py:20-59) -> (loss0, loss1).  Gradients: the cnn code, and the sentence code when it asks for
    one (mogan_damsm_sent_bwd_text)."""

    @staticmethod
    def forward(ctx, cnn, rnn, labels, mask, g3, eps):
        cnn, rnn = _c(cnn), _c(rnn)
        B, C, Bc = cnn.shape[0], cnn.shape[1], rnn.shape[0]
        sim = torch.empty((B, Bc), dtype=torch.float32, device=cnn.device)
        call("mogan_damsm_sent_fwd", ptr(cnn), ptr(rnn), B, Bc, C, g3, eps, ptr(sim), stream_ptr())
        l0, l1 = _PairCE.forward(ctx, sim, labels, mask)
        ctx.save_for_backward(cnn, rnn)
        ctx.cfg = (g3, eps)
        return l0, l1

    @staticmethod
    def backward(ctx, gl0, gl1):
        cnn, rnn = ctx.saved_tensors
        g3, eps = ctx.cfg
        dsim = _PairCE.backward(ctx, gl0, gl1)
        dcnn = drnn = None
        if ctx.needs_input_grad[0]:
            dcnn = torch.empty_like(cnn)
            call("mogan_damsm_sent_bwd", ptr(cnn), ptr(rnn), ptr(dsim), cnn.shape[0], rnn.shape[0], cnn.shape[1], g3, eps,
                 ptr(dcnn), stream_ptr())
        if ctx.needs_input_grad[1]:
            drnn = torch.empty_like(rnn)
            call("mogan_damsm_sent_bwd_text", ptr(cnn), ptr(rnn), ptr(dsim), cnn.shape[0], rnn.shape[0], cnn.shape[1], g3, eps,
                 ptr(drnn), stream_ptr())
        return dcnn, drnn, None, None, None, None


def damsm_sent(cnn, rnn, labels, mask, gamma3, eps=1e-8):
    return DamsmSentFn.apply(cnn, rnn, labels, mask, float(gamma3), float(eps))


def retrieval_rank(code, pos, bank, idx, eps=1e-8, want_scores=False):
    """R-precision ranking in ONE launch (mogan_retrieval_rank): for every query q the cosine of the image code code[q] (Q, C) with
    its own sentence code pos[q] (candidate 0) and with the bank rows idx[q, :] (Q, Rn) of bank (N, C); rank[q] (int32) = how many
    mismatched candidates score strictly higher than the match (0 = retrieved first; a tie counts for the match).  No gradient.
    idx: an int32 device tensor (entries outside [0, N) are clamped by the kernel), or a host array (numpy), which is checked
    against [0, N) here -- IndexError -- and uploaded.  Returns rank, or (rank, score (Q, Rn + 1)) with want_scores."""
    import numpy as np
    code, pos, bank = _c(code.detach()), _c(pos.detach()), _c(bank.detach())
    if code.dim() != 2 or pos.shape != code.shape or bank.dim() != 2 or bank.shape[1] != code.shape[1]:
        raise ValueError("retrieval_rank: code (Q, C), pos (Q, C), bank (N, C) expected, got %s, %s, %s"
                         % (tuple(code.shape), tuple(pos.shape), tuple(bank.shape)))
    Q, C, N = code.shape[0], code.shape[1], bank.shape[0]
    if isinstance(idx, np.ndarray):
        if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= N):
            raise IndexError("retrieval_rank: idx holds rows outside [0, %d): min %d, max %d" % (N, idx.min(), idx.max()))
        ptr(code)                                            # (a host tensor raises here, before anything is uploaded)
        idx = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).to(code.device)
    if idx.dtype != torch.int32 or idx.dim() != 2 or idx.shape[0] != Q:
        raise ValueError("retrieval_rank: idx must be int32 (Q, Rn), got %s %s" % (idx.dtype, tuple(idx.shape)))
    if not (pos.device == bank.device == idx.device == code.device):
        raise ValueError("retrieval_rank: code, pos, bank and idx must be on one device")
    idx = idx if idx.is_contiguous() else idx.contiguous()
    rank = torch.empty((Q,), dtype=torch.int32, device=code.device)
    score = torch.empty((Q, idx.shape[1] + 1), dtype=torch.float32, device=code.device) if want_scores else None
    call("mogan_retrieval_rank", ptr(code), ptr(pos), ptr(bank), ptr(idx), Q, idx.shape[1], C, N, float(eps), ptr(score),
         ptr(rank), stream_ptr())
    return (rank, score) if want_scores else rank


def feature_moments(codes):
    """fp64 mean (D,) and covariance (D, D) -- numpy.cov(rowvar=False), divisor N - 1 -- of fp32 codes (N, D) on the device, in two
    launches (mogan_col_mean_f64, mogan_cov_f64: fp64 MFMA, fixed summation order, cov bitwise symmetric).  No gradient.  Nothing is
    converted or copied for the caller: a wrong dtype or rank, N < 2 or a non-contiguous input is a ValueError."""
    if not torch.is_tensor(codes) or codes.dtype != torch.float32:
        raise ValueError("feature_moments: fp32 codes expected, got %s" % (getattr(codes, "dtype", type(codes)),))
    if codes.dim() != 2:
        raise ValueError("feature_moments: codes (N, D) expected, got %s" % (tuple(codes.shape),))
    N, D = codes.shape
    if N < 2 or D < 1:
        raise ValueError("feature_moments: at least 2 codes of at least 1 feature expected, got %s" % (tuple(codes.shape),))
    if not codes.is_contiguous():
        raise ValueError("feature_moments: contiguous codes expected (strides %s)" % (tuple(codes.stride()),))
    codes = codes.detach()
    x = ptr(codes)
    mean = torch.empty((D,), dtype=torch.float64, device=codes.device)
    cov = torch.empty((D, D), dtype=torch.float64, device=codes.device)
    call("mogan_col_mean_f64", x, N, D, ptr(mean), stream_ptr())
    call("mogan_cov_f64", x, ptr(mean), N, D, ptr(cov), stream_ptr())
    return mean, cov


def poly_mmd_sums(x, y, ix, iy, gamma=None, coef0=1.0):
    """The three sums per subset pair that the kernel Inception distance is formed from (mogan_poly3_mmd_f64: fp64 MFMA, fixed
    summation order, no kernel matrix written): for fp32 codes x (Nx, D), y (Ny, D) and int32 tables ix, iy (S, s), under
    k(a, b) = (gamma <a, b> + coef0)^3 with gamma = 1 / D by default, sums (S, 3) fp64 on the device =
    [sum_{i != j} k(x_ix[k,i], x_ix[k,j]), sum_{i != j} k(y_iy[k,i], y_iy[k,j]), sum_{i,j} k(x_ix[k,i], y_iy[k,j])].
    No gradient.  Nothing is converted or copied for the caller: a wrong dtype or rank, a non-contiguous input, codes on different
    devices or of different widths are a ValueError.  ix, iy: int32 device tensors (entries outside [0, N) are clamped by the
    kernel), or host arrays (numpy), which are checked against [0, N) here -- IndexError -- and uploaded."""
    import numpy as np
    for name, t in (("x", x), ("y", y)):
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise ValueError("poly_mmd_sums: fp32 codes expected, %s is %s" % (name, getattr(t, "dtype", type(t))))
        if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError("poly_mmd_sums: codes (N, D) expected, %s is %s" % (name, tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError("poly_mmd_sums: contiguous codes expected (%s has strides %s)" % (name, tuple(t.stride())))
    if x.shape[1] != y.shape[1]:
        raise ValueError("poly_mmd_sums: x and y differ in width: %s, %s" % (tuple(x.shape), tuple(y.shape)))
    if x.device != y.device:
        raise ValueError("poly_mmd_sums: x and y must be on one device (%s, %s)" % (x.device, y.device))
    x, y = x.detach(), y.detach()
    D = x.shape[1]
    tables = []
    for name, idx, N in (("ix", ix, x.shape[0]), ("iy", iy, y.shape[0])):
        if isinstance(idx, np.ndarray):
            if idx.ndim != 2 or not np.issubdtype(idx.dtype, np.integer):
                raise ValueError("poly_mmd_sums: %s must be an integer (S, s) table, got %s %s" % (name, idx.dtype, idx.shape))
            if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= N):
                raise IndexError("poly_mmd_sums: %s holds rows outside [0, %d): min %d, max %d" % (name, N, idx.min(), idx.max()))
            ptr(x)                                           # (a host tensor raises here, before anything is uploaded)
            idx = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).to(x.device)
        if not torch.is_tensor(idx) or idx.dtype != torch.int32 or idx.dim() != 2:
            raise ValueError("poly_mmd_sums: %s must be int32 (S, s), got %s %s"
                             % (name, getattr(idx, "dtype", type(idx)), tuple(getattr(idx, "shape", ()))))
        if idx.device != x.device:
            raise ValueError("poly_mmd_sums: %s must be on the codes' device (%s, %s)" % (name, idx.device, x.device))
        tables.append(idx if idx.is_contiguous() else idx.contiguous())
    ix, iy = tables
    if ix.shape != iy.shape or ix.shape[0] < 1 or ix.shape[1] < 2:
        raise ValueError("poly_mmd_sums: ix and iy must share one shape (S >= 1, s >= 2), got %s, %s" % (tuple(ix.shape), tuple(iy.shape)))
    S, s = ix.shape
    gamma = 1.0 / D if gamma is None else float(gamma)
    px, py = ptr(x), ptr(y)
    need = int(lib.load().mogan_poly3_mmd_ws_bytes(S, s))
    ws, ws_bytes = workspace(x.device)
    own = None
    if ws_bytes < need:                                       # larger than the shared scratch: a tensor of its own
        own = torch.empty(max(need, 8), dtype=torch.uint8, device=x.device)
        ws, ws_bytes = own.data_ptr(), own.numel()
    sums = torch.empty((S, 3), dtype=torch.float64, device=x.device)
    call("mogan_poly3_mmd_f64", px, x.shape[0], py, y.shape[0], D, ptr(ix), ptr(iy), S, s, gamma, float(coef0), ptr(sums), ws,
         ws_bytes, stream_ptr())
    if own is not None:
        own.record_stream(torch.cuda.current_stream(x.device))
    return sums


def _codes(who, pairs):
    """the contract of the fp64 score ops for their fp32 code matrices: dtype, rank, contiguity, one device, one width"""
    for name, t in pairs:
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise ValueError("%s: fp32 codes expected, %s is %s" % (who, name, getattr(t, "dtype", type(t))))
        if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError("%s: codes (N, D) expected, %s is %s" % (who, name, tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError("%s: contiguous codes expected (%s has strides %s)" % (who, name, tuple(t.stride())))
        if t.shape[1] != pairs[0][1].shape[1]:
            raise ValueError("%s: the codes differ in width: %s, %s" % (who, tuple(pairs[0][1].shape), tuple(t.shape)))
        if t.device != pairs[0][1].device:
            raise ValueError("%s: the codes must be on one device (%s, %s)" % (who, pairs[0][1].device, t.device))


def _scratch(device, need):
    """(pointer, bytes, owner): the shared workspace where it is large enough, else a tensor of its own (to be record_stream'ed)"""
    ws, ws_bytes = workspace(device)
    if ws_bytes >= need:
        return ws, ws_bytes, None
    own = torch.empty(max(need, 8), dtype=torch.uint8, device=device)
    return own.data_ptr(), own.numel(), own


def knn_sqdist(x, K):
    """The K smallest squared Euclidean distances from every row of fp32 codes x (N, D) to the OTHER rows (by position: a duplicate
    elsewhere is a neighbour at distance 0), ascending: (N, K) fp64 on the device (mogan_knn_sqdist_f64: fp64 MFMA, no distance
    matrix written, a distance's bits depend on the two rows only, same bits on every call).  1 <= K <= min(8, N - 1).  No gradient.
    Nothing is converted or copied for the caller: a wrong dtype or rank, a non-contiguous input, a K out of range are a ValueError."""
    _codes("knn_sqdist", (("x", x),))
    K = int(K)
    N, D = x.shape
    if K < 1 or K > 8 or K > N - 1:
        raise ValueError("knn_sqdist: 1 <= K <= min(8, N - 1) expected, got K = %d for %d rows" % (K, N))
    x = x.detach()
    px = ptr(x)
    ws, ws_bytes, own = _scratch(x.device, int(lib.load().mogan_knn_sqdist_ws_bytes(N, K)))
    out = torch.empty((N, K), dtype=torch.float64, device=x.device)
    call("mogan_knn_sqdist_f64", px, N, D, K, ptr(out), ws, ws_bytes, stream_ptr())
    if own is not None:
        own.record_stream(torch.cuda.current_stream(x.device))
    return out


def knn_cross(q, p, K):
    """For every row of fp32 queries q (M, D) its K nearest rows of fp32 codes p (N, D): (d2 (M, K) fp64, idx (M, K) int32) on the
    device, ascending by squared Euclidean distance, equal bits by position -- the lexicographic order of (d2, i)
    (mogan_knn_cross_f64; the distances are knn_sqdist's and ball_counts', bit for bit).  1 <= K <= min(8, N).  No gradient.
    Nothing is converted or copied for the caller: a wrong dtype or rank, a width mismatch, a non-contiguous input, another device,
    a K out of range are a ValueError."""
    _codes("knn_cross", (("q", q), ("p", p)))
    K = int(K)
    M, N, D = q.shape[0], p.shape[0], q.shape[1]
    if K < 1 or K > 8 or K > N:
        raise ValueError("knn_cross: 1 <= K <= min(8, N) expected, got K = %d for %d rows of p" % (K, N))
    q, p = q.detach(), p.detach()
    pq, pp = ptr(q), ptr(p)
    ws, ws_bytes, own = _scratch(q.device, int(lib.load().mogan_knn_cross_ws_bytes(M, N, K)))
    d2 = torch.empty((M, K), dtype=torch.float64, device=q.device)
    idx = torch.empty((M, K), dtype=torch.int32, device=q.device)
    call("mogan_knn_cross_f64", pq, M, pp, N, D, K, ptr(d2), ptr(idx), ws, ws_bytes, stream_ptr())
    if own is not None:
        own.record_stream(torch.cuda.current_stream(q.device))
    return d2, idx


def knn_label(q, qlabel, p, plabel, K):
    """knn_cross with an int32 label per row (mogan_knn_label_f64): (d2 (M, K) fp64, idx (M, K) int32, same_d2 (M) fp64, same_idx (M)
    int32, other_d2 (M) fp64, other_idx (M) int32) on the device.  d2 / idx are knn_cross's bit for bit; same_* is the first pair
    under the same order (distance, equal bits by position) among the rows of p whose label equals the query's, other_* among the
    rows whose label differs; an empty set gives +inf and 2^31 - 1.  Labels are arbitrary int32.  No gradient.  Nothing is converted
    or copied for the caller: knn_cross's checks, and labels that are not int32, dense, on the codes' device, of length M and N are
    a ValueError."""
    _codes("knn_label", (("q", q), ("p", p)))
    K = int(K)
    M, N, D = q.shape[0], p.shape[0], q.shape[1]
    if K < 1 or K > 8 or K > N:
        raise ValueError("knn_label: 1 <= K <= min(8, N) expected, got K = %d for %d rows of p" % (K, N))
    for name, t, n in (("qlabel", qlabel, M), ("plabel", plabel, N)):
        if not torch.is_tensor(t) or t.dtype != torch.int32:
            raise ValueError("knn_label: int32 labels expected, %s is %s" % (name, getattr(t, "dtype", type(t))))
        if t.dim() != 1 or t.shape[0] != n or not t.is_contiguous():
            raise ValueError("knn_label: dense labels (%d,) expected, %s is %s with strides %s" % (n, name, tuple(t.shape),
                                                                                                tuple(t.stride())))
        if t.device != q.device:
            raise ValueError("knn_label: the labels must be on the codes' device (%s, %s is on %s)" % (q.device, name, t.device))
    q, p = q.detach(), p.detach()
    pq, pp = ptr(q), ptr(p)
    ws, ws_bytes, own = _scratch(q.device, int(lib.load().mogan_knn_label_ws_bytes(M, N, K)))
    d2 = torch.empty((M, K), dtype=torch.float64, device=q.device)
    idx = torch.empty((M, K), dtype=torch.int32, device=q.device)
    same_d2, other_d2 = (torch.empty((M,), dtype=torch.float64, device=q.device) for _ in range(2))
    same_idx, other_idx = (torch.empty((M,), dtype=torch.int32, device=q.device) for _ in range(2))
    call("mogan_knn_label_f64", pq, ptr(qlabel), M, pp, ptr(plabel), N, D, K, ptr(d2), ptr(idx), ptr(same_d2), ptr(same_idx),
         ptr(other_d2), ptr(other_idx), ws, ws_bytes, stream_ptr())
    if own is not None:
        own.record_stream(torch.cuda.current_stream(q.device))
    return d2, idx, same_d2, same_idx, other_d2, other_idx


SOFTMAX_HEAD_MAX_CLASSES = 1 << 20
SOFTMAX_HEAD_MAX_SPLITS = 65535


def softmax_head_sums(x, w, bias, splits=1, want_lse=False):
    """The sums the Inception Score is formed from (mogan_softmax_head_f64: fp64 MFMA, fixed summation order, no (row, class) matrix
    written): for fp32 codes x (n, D), a head w (C, D) and bias (C), with z = x w^T + bias, p = softmax(z) per row and the rows cut
    into `splits` contiguous splits [floor(s n / S), floor((s + 1) n / S)): (row_h (n) = sum_y p log p, psum (S, C) = sum of p over
    each split's rows), both fp64 on the device; with want_lse (row_lse (n), row_h, psum).  A row's figures depend on the row and the
    head only; psum[s] is bit for bit that of the S = 1 call on the split's rows.  No gradient.  Nothing is converted or copied for
    the caller: a wrong dtype or rank, a non-contiguous input, another device, a width mismatch, splits outside 1..min(n, 65535) or
    more than 2^20 classes are a ValueError."""
    _codes("softmax_head_sums", (("x", x), ("w", w)))
    if not torch.is_tensor(bias) or bias.dtype != torch.float32 or bias.dim() != 1 or bias.shape[0] != w.shape[0] or \
            not bias.is_contiguous():
        raise ValueError("softmax_head_sums: a dense fp32 bias (%d,) expected, got %s %s"
                         % (w.shape[0], getattr(bias, "dtype", type(bias)), tuple(getattr(bias, "shape", ()))))
    if bias.device != x.device:
        raise ValueError("softmax_head_sums: the bias must be on the codes' device (%s, %s)" % (x.device, bias.device))
    n, D, C, S = x.shape[0], x.shape[1], w.shape[0], int(splits)
    if S < 1 or S > min(n, SOFTMAX_HEAD_MAX_SPLITS) or C > SOFTMAX_HEAD_MAX_CLASSES:
        raise ValueError("softmax_head_sums: 1 <= splits <= min(n, %d) and at most %d classes expected, got splits = %d for %d "
                         "rows, %d classes" % (SOFTMAX_HEAD_MAX_SPLITS, SOFTMAX_HEAD_MAX_CLASSES, S, n, C))
    x, w, bias = x.detach(), w.detach(), bias.detach()
    px, pw, pb = ptr(x), ptr(w), ptr(bias)
    ws, ws_bytes, own = _scratch(x.device, int(lib.load().mogan_softmax_head_ws_bytes(n, C, S)))
    row_lse = torch.empty((n,), dtype=torch.float64, device=x.device) if want_lse else None
    row_h = torch.empty((n,), dtype=torch.float64, device=x.device)
    psum = torch.empty((S, C), dtype=torch.float64, device=x.device)
    call("mogan_softmax_head_f64", px, n, D, pw, pb, C, S, ptr(row_lse), ptr(row_h), ptr(psum), ws, ws_bytes, stream_ptr())
    if own is not None:
        own.record_stream(torch.cuda.current_stream(x.device))
    return (row_lse, row_h, psum) if want_lse else (row_h, psum)


def ball_counts(q, p, r2, side="support"):
    """count (M, R) int32 on the device, count[j, c] = #{ i : d2(q_j, p_i) <= r2[., c] } for fp32 queries q (M, D), fp32 support
    points p (N, D) and fp64 squared radii r2 (mogan_ball_count_f64; the distances are knn_sqdist's, bit for bit).  side
    "support": the radius is the support point's, r2 (N, R) or (N,); side "query": the query's, r2 (M, R) or (M,).  1 <= R <= 4.
    No gradient.  Nothing is converted or copied for the caller: a wrong dtype or rank, a width or length mismatch, a
    non-contiguous input, another device, R > 4, another `side` are a ValueError."""
    _codes("ball_counts", (("q", q), ("p", p)))
    if side not in ("support", "query"):
        raise ValueError("ball_counts: side must be 'support' or 'query', got %r" % (side,))
    if not torch.is_tensor(r2) or r2.dtype != torch.float64:
        raise ValueError("ball_counts: fp64 radii expected, r2 is %s" % (getattr(r2, "dtype", type(r2)),))
    if r2.dim() not in (1, 2):
        raise ValueError("ball_counts: radii (rows, R) or (rows,) expected, r2 is %s" % (tuple(r2.shape),))
    M, N, D = q.shape[0], p.shape[0], q.shape[1]
    rows = N if side == "support" else M
    R = 1 if r2.dim() == 1 else int(r2.shape[1])
    if r2.shape[0] != rows or R < 1 or R > 4:
        raise ValueError("ball_counts: side %r needs radii (%d, 1..4), r2 is %s" % (side, rows, tuple(r2.shape)))
    if not r2.is_contiguous():
        raise ValueError("ball_counts: contiguous radii expected (r2 has strides %s)" % (tuple(r2.stride()),))
    if r2.device != q.device:
        raise ValueError("ball_counts: r2 must be on the codes' device (%s, %s)" % (r2.device, q.device))
    q, p, r2 = q.detach(), p.detach(), r2.detach()
    pq, pp, pr = ptr(q), ptr(p), ptr(r2)
    ws, ws_bytes, own = _scratch(q.device, int(lib.load().mogan_ball_count_ws_bytes(M, N, R)))
    count = torch.empty((M, R), dtype=torch.int32, device=q.device)
    call("mogan_ball_count_f64", pq, M, pp, N, D, pr, R, 0 if side == "support" else 1, ptr(count), ws, ws_bytes, stream_ptr())
    if own is not None:
        own.record_stream(torch.cuda.current_stream(q.device))
    return count


def _dense_f32(who, name, t, ndim):
    """the contract of the sliced-Wasserstein ops for an fp32 tensor: dtype, rank, contiguity (nothing is converted)"""
    if not torch.is_tensor(t) or t.dtype != torch.float32:
        raise ValueError("%s: fp32 expected, %s is %s" % (who, name, getattr(t, "dtype", type(t))))
    if t.dim() != ndim or min(t.shape) < 1:
        raise ValueError("%s: %s must have %d non-empty dimensions, got %s" % (who, name, ndim, tuple(t.shape)))
    if not t.is_contiguous():
        raise ValueError("%s: contiguous tensors expected (%s has strides %s)" % (who, name, tuple(t.stride())))
    return t.detach()


def _plane(who, x):
    x = _dense_f32(who, "x", x, 3)
    NC, H, W = x.shape
    if H < 4 or W < 4 or H % 2 or W % 2 or x.numel() > 2 ** 31 - 1:
        raise ValueError("%s: x (N C, H, W) with even H, W >= 4 and fewer than 2^31 elements expected, got %s" % (who, tuple(x.shape)))
    return x, NC, H, W


def pyr_down(x):
    """One step down the Gaussian pyramid of DESIGN.md section 9g (mogan_pyr_down): fp32 x (N C, H, W) -> (N C, H / 2, W / 2) under
    the 5 x 5 filter (1, 4, 6, 4, 1)^2 / 256 with mirrored indices (the edge sample not repeated).  H and W even and >= 4.  No
    gradient.  Nothing is converted or copied for the caller: a wrong dtype, rank, contiguity or size is a ValueError."""
    x, NC, H, W = _plane("pyr_down", x)
    px = ptr(x)
    out = torch.empty((NC, H // 2, W // 2), dtype=torch.float32, device=x.device)
    call("mogan_pyr_down", px, NC, H, W, ptr(out), stream_ptr())
    return out


def lap_residual(x, down):
    """One level of the Laplacian pyramid in one launch (mogan_lap_residual): x - pyr_up(down) for fp32 x (N C, H, W) and
    down (N C, H / 2, W / 2); pyr_up is pyr_down's filter times 4 over the zero-inserted image, which is never formed.  No gradient.
    Nothing is converted or copied for the caller: a wrong dtype, rank, contiguity, device or size is a ValueError."""
    x, NC, H, W = _plane("lap_residual", x)
    down = _dense_f32("lap_residual", "down", down, 3)
    if tuple(down.shape) != (NC, H // 2, W // 2):
        raise ValueError("lap_residual: down must be %s for x %s, got %s" % ((NC, H // 2, W // 2), tuple(x.shape), tuple(down.shape)))
    if down.device != x.device:
        raise ValueError("lap_residual: x and down must be on one device (%s, %s)" % (x.device, down.device))
    px, pd = ptr(x), ptr(down)
    out = torch.empty_like(x)
    call("mogan_lap_residual", px, pd, NC, H, W, ptr(out), stream_ptr())
    return out


def swd_gather(level, centres, desc, row0):
    """Writes rows [row0, row0 + R) of the descriptor buffer desc (rows_total, 49 C) fp32: row r = the 7 x 7 neighbourhood of
    (cy, cx) in image `image` of the fp32 level (N, C, H, W), all channels, in (channel, y, x) order (mogan_swd_gather; a copy).
    centres (R, 3) = (image, cy, cx) per row: a host array (numpy integers), checked here -- image in [0, N), cy in [3, H - 3),
    cx in [3, W - 3), else a ValueError -- and uploaded; or an int32 device tensor, which the kernel clamps into the level.  C in 1..4,
    H and W >= 7.  Returns desc.  No gradient; nothing is converted or copied for the caller."""
    import numpy as np
    level = _dense_f32("swd_gather", "level", level, 4)
    given, desc = desc, _dense_f32("swd_gather", "desc", desc, 2)
    N, C, H, W = level.shape
    if C > 4 or H < 7 or W < 7 or level.numel() > 2 ** 31 - 1:
        raise ValueError("swd_gather: level (N, 1..4, >= 7, >= 7) with fewer than 2^31 elements expected, got %s" % (tuple(level.shape),))
    if desc.shape[1] != 49 * C or desc.shape[0] > 2 ** 31 - 1:
        raise ValueError("swd_gather: desc must be (rows, %d) for %d channels, got %s" % (49 * C, C, tuple(desc.shape)))
    if desc.device != level.device:
        raise ValueError("swd_gather: level and desc must be on one device (%s, %s)" % (level.device, desc.device))
    if isinstance(centres, np.ndarray):
        if centres.ndim != 2 or centres.shape[1] != 3 or centres.shape[0] < 1 or not np.issubdtype(centres.dtype, np.integer):
            raise ValueError("swd_gather: centres must be an integer (R, 3) table, got %s %s" % (centres.dtype, centres.shape))
        lo, hi = centres.min(axis=0), centres.max(axis=0)
        if lo[0] < 0 or hi[0] >= N or lo[1] < 3 or hi[1] >= H - 3 or lo[2] < 3 or hi[2] >= W - 3:
            raise ValueError("swd_gather: centres outside image [0, %d), cy [3, %d), cx [3, %d): min %s, max %s"
                             % (N, H - 3, W - 3, lo.tolist(), hi.tolist()))
    host = centres if isinstance(centres, np.ndarray) else None
    if host is None and (not torch.is_tensor(centres) or centres.dtype != torch.int32 or centres.dim() != 2 or centres.shape[1] != 3
                         or centres.shape[0] < 1 or not centres.is_contiguous()):
        raise ValueError("swd_gather: centres must be contiguous int32 (R, 3), got %s %s"
                         % (getattr(centres, "dtype", type(centres)), tuple(getattr(centres, "shape", ()))))
    if host is None and centres.device != level.device:
        raise ValueError("swd_gather: centres must be on the level's device (%s, %s)" % (centres.device, level.device))
    R, row0 = int(centres.shape[0]), int(row0)
    if row0 < 0 or row0 + R > desc.shape[0]:
        raise ValueError("swd_gather: rows [%d, %d) do not fit a buffer of %d rows" % (row0, row0 + R, desc.shape[0]))
    if host is not None:
        ptr(level)                                           # (a host tensor raises here, before anything is uploaded)
        centres = torch.from_numpy(np.ascontiguousarray(host, dtype=np.int32)).to(level.device)
    call("mogan_swd_gather", ptr(level), N, C, H, W, ptr(centres), R, ptr(desc), row0, desc.shape[0], stream_ptr())
    return given


def _descriptors(who, desc):
    desc = _dense_f32(who, "desc", desc, 2)
    rows, K = desc.shape
    if K % 49 or K // 49 > 4 or rows > 2 ** 31 - 1:
        raise ValueError("%s: descriptors (rows, 49 C) with C in 1..4 expected, got %s" % (who, tuple(desc.shape)))
    return desc, rows, K // 49


def swd_moments(desc):
    """(C, 2) fp64 on the device: mean and population standard deviation per channel of fp32 descriptors (rows, 49 C), over all rows
    and the 49 positions of the channel (mogan_swd_moments_f64: two passes, fp64 sums in a fixed order).  A constant channel has a
    standard deviation of exactly 0.  No gradient; nothing is converted or copied for the caller."""
    desc, rows, C = _descriptors("swd_moments", desc)
    pd = ptr(desc)
    ws, ws_bytes, own = _scratch(desc.device, int(lib.load().mogan_swd_moments_ws_bytes(rows, C)))
    mom = torch.empty((C, 2), dtype=torch.float64, device=desc.device)
    call("mogan_swd_moments_f64", pd, rows, C, ptr(mom), ws, ws_bytes, stream_ptr())
    if own is not None:
        own.record_stream(torch.cuda.current_stream(desc.device))
    return mom


def swd_project(desc, moments, dirs):
    """Projections (D, rows) fp32 of the standardised descriptors onto the directions: desc (rows, K = 49 C) fp32, moments (C, 2)
    fp64 (swd_moments), dirs (K, D) fp32, 1 <= D <= 1024 (mogan_swd_project: every value standardised in fp64 and rounded once, the
    product on the matrix pipe; a projection's bits depend on its row and direction only).  A direction's projections are
    contiguous.  No gradient; nothing is converted or copied for the caller."""
    desc, rows, C = _descriptors("swd_project", desc)
    dirs = _dense_f32("swd_project", "dirs", dirs, 2)
    if not torch.is_tensor(moments) or moments.dtype != torch.float64 or tuple(moments.shape) != (C, 2) or not moments.is_contiguous():
        raise ValueError("swd_project: contiguous fp64 moments (%d, 2) expected, got %s %s"
                         % (C, getattr(moments, "dtype", type(moments)), tuple(getattr(moments, "shape", ()))))
    if dirs.shape[0] != 49 * C or dirs.shape[1] > 1024:
        raise ValueError("swd_project: dirs (%d, 1..1024) expected, got %s" % (49 * C, tuple(dirs.shape)))
    if not (moments.device == dirs.device == desc.device):
        raise ValueError("swd_project: desc, moments and dirs must be on one device")
    D = int(dirs.shape[1])
    pd, pm, pv = ptr(desc), ptr(moments.detach()), ptr(dirs)
    out = torch.empty((D, rows), dtype=torch.float32, device=desc.device)
    call("mogan_swd_project", pd, rows, C, pm, pv, D, ptr(out), stream_ptr())
    return out


def swd_absdiff(a, b):
    """(D,) fp64 on the device: sum over r of |a[d, r] - b[d, r]| for two fp32 (D, rows) matrices, D <= 1024, in fp64 and a fixed
    order (mogan_swd_absdiff_f64).  No gradient; nothing is converted or copied for the caller."""
    a = _dense_f32("swd_absdiff", "a", a, 2)
    b = _dense_f32("swd_absdiff", "b", b, 2)
    if a.shape != b.shape or a.shape[0] > 1024 or a.shape[1] > 2 ** 31 - 1:
        raise ValueError("swd_absdiff: two (D <= 1024, rows) matrices of one shape expected, got %s, %s" % (tuple(a.shape), tuple(b.shape)))
    if a.device != b.device:
        raise ValueError("swd_absdiff: a and b must be on one device (%s, %s)" % (a.device, b.device))
    pa, pb = ptr(a), ptr(b)
    out = torch.empty((a.shape[0],), dtype=torch.float64, device=a.device)
    call("mogan_swd_absdiff_f64", pa, pb, a.shape[1], a.shape[0], ptr(out), stream_ptr())
    return out


def avg_down2(x):
    """The aligned 2 x 2 mean of DESIGN.md section 9h (mogan_avg_down2): fp32 x (N C, H, W) -> (N C, H / 2, W / 2),
    ((x00 + x01) + (x10 + x11)) / 4.  H and W even.  No gradient.  Nothing is converted or copied for the caller: a wrong dtype,
    rank, contiguity or size is a ValueError."""
    x = _dense_f32("avg_down2", "x", x, 3)
    NC, H, W = x.shape
    if H % 2 or W % 2 or x.numel() > 2 ** 31 - 1:
        raise ValueError("avg_down2: x (N C, H, W) with even H, W and fewer than 2^31 elements expected, got %s" % (tuple(x.shape),))
    px = ptr(x)
    out = torch.empty((NC, H // 2, W // 2), dtype=torch.float32, device=x.device)
    call("mogan_avg_down2", px, NC, H, W, ptr(out), stream_ptr())
    return out


def ssim_level(a, b, window, maps=False):
    """One scale of the structural similarity of P pairs of images (mogan_ssim_level_f64; attngan/msssim.py has the definition):
    fp32 a, b (P, C, S, S) with C in 1..4 and the fp32 window (n,), n <= min(11, S), on their device -> terms (P, 2) fp64 on the
    device, (mean ssim, mean cs) of every pair over its channels and its (S - n + 1)^2 valid positions; with maps=True
    (terms, ssim_map, cs_map), the maps (P, C, S - n + 1, S - n + 1) fp32.  A bit copy gives 1.0 exactly, exchanging a and b gives
    the same bits, and so does a second call.  No gradient.  Nothing is converted or copied for the caller: a wrong dtype, rank,
    device, contiguity or size is a ValueError."""
    a = _dense_f32("ssim_level", "a", a, 4)
    b = _dense_f32("ssim_level", "b", b, 4)
    window = _dense_f32("ssim_level", "window", window, 1)
    P, C, S, n = a.shape[0], a.shape[1], a.shape[2], window.shape[0]
    if a.shape != b.shape:
        raise ValueError("ssim_level: a and b must have one shape, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    if C > 4 or S < 2 or a.shape[3] != S or a.numel() > 2 ** 31 - 1:
        raise ValueError("ssim_level: pairs (P, 1..4, S, S) with S >= 2 and fewer than 2^31 elements expected, got %s" % (tuple(a.shape),))
    if n > min(11, S):
        raise ValueError("ssim_level: a window of at most min(11, S = %d) taps expected, got %d" % (S, n))
    if not (a.device == b.device == window.device):
        raise ValueError("ssim_level: a, b and the window must be on one device (%s, %s, %s)" % (a.device, b.device, window.device))
    pa, pb, pw = ptr(a), ptr(b), ptr(window)
    ws, ws_bytes, own = _scratch(a.device, int(lib.load().mogan_ssim_level_ws_bytes(P, C, S, n)))
    terms = torch.empty((P, 2), dtype=torch.float64, device=a.device)
    M = S - n + 1
    ssim_map = torch.empty((P, C, M, M), dtype=torch.float32, device=a.device) if maps else None
    cs_map = torch.empty((P, C, M, M), dtype=torch.float32, device=a.device) if maps else None
    call("mogan_ssim_level_f64", pa, pb, P, C, S, pw, n, ptr(terms), ptr(ssim_map), ptr(cs_map), ws, ws_bytes, stream_ptr())
    if own is not None:
        own.record_stream(torch.cuda.current_stream(a.device))
    return (terms, ssim_map, cs_map) if maps else terms


def roi_resize(x, boxes, image_index, OH, OW, out=None):
    """Crop, compaction and edge-clamped bilinear resize of a ragged list of boxes in one launch (mogan_roi_resize; DESIGN.md section
    9i): fp32 x (B, C, H, W) on the device with C in 1..4; boxes (R, 4) fp32, relative (x, y, w, h), and image_index (R) int32 or
    int64 are HOST tensors -- checked here, then uploaded -- -> (R, C, OH, OW) fp32 on x's device, row r the box boxes[r] of image
    image_index[r].  A box with w <= 0 or h <= 0 gives zeros.  `out`, where given, is a dense (R, C, OH, OW) fp32 tensor on x's device
    (rows of a larger buffer, for one) and is returned.  R = 0 returns an empty tensor without a launch.  No gradient.  Nothing is
    converted or copied for the caller: a wrong type, dtype, rank, stride or device, an index outside [0, B) and a box value that is
    not finite are a ValueError."""
    x = _dense_f32("roi_resize", "x", x, 4)
    B, C, H, W = x.shape
    OH, OW = int(OH), int(OW)
    if C > 4 or x.numel() > 2 ** 31 - 1 or OH < 1 or OW < 1:
        raise ValueError("roi_resize: x (B, 1..4, H, W) with fewer than 2^31 elements and OH, OW >= 1 expected, got %s -> (%d, %d)"
                         % (tuple(x.shape), OH, OW))
    for name, t, dtypes, ndim in (("boxes", boxes, (torch.float32,), 2), ("image_index", image_index, (torch.int32, torch.int64), 1)):
        if not torch.is_tensor(t) or t.dtype not in dtypes or t.device.type != "cpu":
            raise ValueError("roi_resize: %s must be a host tensor of %s, got %s %s" % (
                name, " or ".join(str(d) for d in dtypes), getattr(t, "dtype", type(t)), getattr(t, "device", "")))
        if t.dim() != ndim or not t.is_contiguous():
            raise ValueError("roi_resize: %s must be a contiguous tensor of %d dimensions, got %s with strides %s"
                             % (name, ndim, tuple(t.shape), tuple(t.stride())))
    R = image_index.shape[0]
    if tuple(boxes.shape) != (R, 4):
        raise ValueError("roi_resize: boxes (R, 4) for image_index (R,) expected, got %s and %s" % (tuple(boxes.shape), (R,)))
    if x.device.type == "meta":
        raise ValueError("roi_resize: x is a meta tensor")
    if R * C * OH * OW > 2 ** 31 - 1:
        raise ValueError("roi_resize: (%d, %d, %d, %d) has 2^31 elements or more" % (R, C, OH, OW))
    if R and (int(image_index.min()) < 0 or int(image_index.max()) >= B):
        raise ValueError("roi_resize: image_index holds images outside [0, %d): min %d, max %d"
                         % (B, int(image_index.min()), int(image_index.max())))
    if not bool(torch.isfinite(boxes).all()):
        raise ValueError("roi_resize: a box value is not finite")
    if out is not None:
        if (not torch.is_tensor(out) or out.dtype != torch.float32 or tuple(out.shape) != (R, C, OH, OW) or not out.is_contiguous()
                or out.device != x.device):
            raise ValueError("roi_resize: out must be a dense fp32 %s tensor on %s, got %s %s on %s"
                             % ((R, C, OH, OW), x.device, getattr(out, "dtype", type(out)), tuple(getattr(out, "shape", ())),
                                getattr(out, "device", "")))
    px = ptr(x)                                                # (a host tensor raises here, before anything is uploaded)
    if out is None:
        out = torch.empty((R, C, OH, OW), dtype=torch.float32, device=x.device)
    if R:
        # one upload for both: the boxes' bits and the index behind them, 20 bytes per object
        both = torch.cat([boxes.view(torch.int32).view(-1), image_index.to(torch.int32)]).to(x.device)
        call("mogan_roi_resize", px, B, C, H, W, ptr(both), ptr(both) + 16 * R, R, ptr(out), OH, OW, stream_ptr())
    return out


def box_shift_sums(a, b, edit, others):
    """The sums of the layout-shift score in one launch (mogan_box_shift_sums_f64; attngan/layoutshift.py has
    the definition): fp32 a, b (P, C, S, S) on one device with C in 1..4 and S in 2..1024 -- a generated under the data's layout, b
    under the edit; edit (P, 6) int32 = (x0, y0, x1, y1, dx, dy) and others (P, G, 4) int32 = (x0, y0, x1, y1), G in 0..8, are HOST
    tensors -- checked here, then uploaded -- -> (sums (P, 7) fp64, counts (P, 5) int32) on a's device.  No gradient.  Nothing is
    converted or copied for the caller: a wrong type, dtype, rank, stride or device is a ValueError, and so is a bad rectangle: an
    edit rectangle that is empty or not inside the image, or whose copy shifted by (dx, dy) is not inside it."""
    a = _dense_f32("box_shift_sums", "a", a, 4)
    b = _dense_f32("box_shift_sums", "b", b, 4)
    P, C, S, S2 = a.shape
    if tuple(b.shape) != tuple(a.shape) or b.device != a.device:
        raise ValueError("box_shift_sums: a and b must have one shape and one device, got %s on %s and %s on %s"
                         % (tuple(a.shape), a.device, tuple(b.shape), b.device))
    if S != S2 or C > 4 or S < 2 or S > 1024 or a.numel() > 2 ** 31 - 1:
        raise ValueError("box_shift_sums: a (P, 1..4, S, S) with S in 2..1024 and fewer than 2^31 elements expected, got %s"
                         % (tuple(a.shape),))
    for name, t, ndim in (("edit", edit, 2), ("others", others, 3)):
        if not torch.is_tensor(t) or t.dtype != torch.int32 or t.device.type != "cpu":
            raise ValueError("box_shift_sums: %s must be a host tensor of torch.int32, got %s %s"
                             % (name, getattr(t, "dtype", type(t)), getattr(t, "device", "")))
        if t.dim() != ndim or not t.is_contiguous():
            raise ValueError("box_shift_sums: %s must be a contiguous tensor of %d dimensions, got %s with strides %s"
                             % (name, ndim, tuple(t.shape), tuple(t.stride())))
    if tuple(edit.shape) != (P, 6) or others.shape[0] != P or others.shape[2] != 4 or others.shape[1] > 8:
        raise ValueError("box_shift_sums: edit (%d, 6) and others (%d, 0..8, 4) expected, got %s and %s"
                         % (P, P, tuple(edit.shape), tuple(others.shape)))
    if a.device.type == "meta":
        raise ValueError("box_shift_sums: a is a meta tensor")
    # the legality of an edit row, as attngan/layoutshift._row_ok (the oracle) and the kernel's own guard (csrc/mogan_layout.hip) state it
    e = edit.to(torch.int64)
    x0, y0, x1, y1, dx, dy = (e[:, k] for k in range(6))
    bad = ~((x0 >= 0) & (y0 >= 0) & (x1 > x0) & (y1 > y0) & (x1 <= S) & (y1 <= S)
            & (x0 + dx >= 0) & (y0 + dy >= 0) & (x1 + dx <= S) & (y1 + dy <= S))
    if bool(bad.any()):
        r = int(bad.nonzero()[0])
        raise ValueError("box_shift_sums: edit row %d, rectangle (%d, %d, %d, %d) moved by (%d, %d), is empty or leaves the %d x %d "
                         "image" % ((r,) + tuple(int(v) for v in edit[r]) + (S, S)))
    G = int(others.shape[1])
    pa, pb = ptr(a), ptr(b)                                    # (a host tensor raises here, before anything is uploaded)
    both = torch.cat([edit.reshape(-1), others.reshape(-1)]).to(a.device)       # one upload: 24 + 16 G bytes per pair
    sums = torch.empty((P, 7), dtype=torch.float64, device=a.device)
    counts = torch.empty((P, 5), dtype=torch.int32, device=a.device)
    call("mogan_box_shift_sums_f64", pa, pb, P, C, S, ptr(both), (ptr(both) + 24 * P) if G else None, G, ptr(sums), ptr(counts),
         stream_ptr())
    return sums, counts


def _attn_maps(who, attn, cap_lens):
    """the checks the two attention-sheet ops share: attn (B, 1..32, att, att) fp32 with att in 2..128, cap_lens (B) a HOST int32
    tensor with every length in 1..T -> (attn detached, B, T, att)"""
    attn = _dense_f32(who, "attn", attn, 4)
    B, T, att, att2 = attn.shape
    if att != att2 or att < 2 or att > 128 or T > 32 or attn.numel() > 2 ** 31 - 1:
        raise ValueError("%s: attn (B, 1..32, att, att) with att in 2..128 and fewer than 2^31 elements expected, got %s"
                         % (who, tuple(attn.shape)))
    if not torch.is_tensor(cap_lens) or cap_lens.dtype != torch.int32 or cap_lens.device.type != "cpu":
        raise ValueError("%s: cap_lens must be a host tensor of torch.int32, got %s %s"
                         % (who, getattr(cap_lens, "dtype", type(cap_lens)), getattr(cap_lens, "device", "")))
    if cap_lens.dim() != 1 or cap_lens.shape[0] != B or not cap_lens.is_contiguous():
        raise ValueError("%s: cap_lens must be a contiguous (%d,) tensor, got %s with strides %s"
                         % (who, B, tuple(cap_lens.shape), tuple(cap_lens.stride())))
    if int(cap_lens.min()) < 1 or int(cap_lens.max()) > T:
        raise ValueError("%s: every caption length must lie in 1..%d, got %d..%d" % (who, T, int(cap_lens.min()), int(cap_lens.max())))
    if attn.device.type == "meta":
        raise ValueError("%s: attn is a meta tensor" % who)
    return attn, B, T, att


def attn_conf(attn, cap_lens):
    """The thresholded attention mass per word, the quantity the attention sheets' top-K choice sorts by (mogan_attn_conf_f64;
    DESIGN.md section 9p; attngan/attnsheet.py has the definition): fp32 attn (B, T, att, att) on the device with T <= 32 and att in
    2..128; cap_lens (B) a HOST int32 tensor, every length in 1..T -- checked here, then uploaded -- -> conf (B, T) fp64 on attn's
    device, conf[b, t] = sum a [a > 4 / len_b] for t < len_b and 0 otherwise.  No gradient.  Nothing is converted or copied for the
    caller: a wrong type, dtype, rank, stride, device or range is a ValueError."""
    attn, B, T, att = _attn_maps("attn_conf", attn, cap_lens)
    pa = ptr(attn)                                             # (a host tensor raises here, before anything is uploaded)
    lens = cap_lens.to(attn.device)
    conf = torch.empty((B, T), dtype=torch.float64, device=attn.device)
    call("mogan_attn_conf_f64", pa, ptr(lens), B, T, att, ptr(conf), stream_ptr())
    return conf


def attn_sheet(attn, cap_lens, img, table, pick, alpha=180):
    """The attention sheets of the picked (sample, word) pairs in one launch (mogan_attn_sheet_f64; DESIGN.md section 9p;
    attngan/attnsheet.py has the definition): fp32 attn (B, T, att, att) and img (B, 3, vis, vis) and the fp64 table (vis, att) of
    attnsheet.table on one device, vis a multiple of att and <= 256; cap_lens (B) and pick (P, 2) = (sample, word) are HOST int32
    tensors -- checked here, then uploaded -- -> (sheet (P, vis, vis, 3) uint8, stats (P, 2) fp64 = (lo, hi), flags (P) int32) on
    attn's device.  No gradient.  Nothing is converted or copied for the caller: a wrong type, dtype, rank, stride, device or range
    is a ValueError, and so is a pick outside the batch or at or past its caption's length."""
    attn, B, T, att = _attn_maps("attn_sheet", attn, cap_lens)
    img = _dense_f32("attn_sheet", "img", img, 4)
    if not torch.is_tensor(table) or table.dtype != torch.float64 or table.dim() != 2 or not table.is_contiguous():
        raise ValueError("attn_sheet: table must be a contiguous fp64 (vis, %d) tensor, got %s %s"
                         % (att, getattr(table, "dtype", type(table)), tuple(getattr(table, "shape", ()))))
    vis = int(table.shape[0])
    if table.shape[1] != att or vis < att or vis > 256 or vis % att:
        raise ValueError("attn_sheet: table (vis, %d) with vis a multiple of %d and <= 256 expected, got %s" % (att, att, tuple(table.shape)))
    if tuple(img.shape) != (B, 3, vis, vis):
        raise ValueError("attn_sheet: img %s expected, got %s" % ((B, 3, vis, vis), tuple(img.shape)))
    if img.device != attn.device or table.device != attn.device:
        raise ValueError("attn_sheet: attn, img and table must be on one device (%s, %s, %s)" % (attn.device, img.device, table.device))
    if not torch.is_tensor(pick) or pick.dtype != torch.int32 or pick.device.type != "cpu":
        raise ValueError("attn_sheet: pick must be a host tensor of torch.int32, got %s %s"
                         % (getattr(pick, "dtype", type(pick)), getattr(pick, "device", "")))
    if pick.dim() != 2 or pick.shape[0] < 1 or pick.shape[1] != 2 or not pick.is_contiguous():
        raise ValueError("attn_sheet: pick must be a contiguous (P >= 1, 2) tensor, got %s with strides %s"
                         % (tuple(pick.shape), tuple(pick.stride())))
    alpha = int(alpha)
    if alpha < 0 or alpha > 255:
        raise ValueError("attn_sheet: alpha in 0..255 expected, got %d" % alpha)
    P = int(pick.shape[0])
    if 3 * P * vis * vis > 2 ** 31 - 1 or img.numel() > 2 ** 31 - 1:
        raise ValueError("attn_sheet: (%d, %d, %d, 3) has 2^31 elements or more" % (max(P, B), vis, vis))
    # the legality of a pick, as attnsheet.pick_ok (the oracle) and the kernel's own guard (csrc/mogan_attn_sheet.hip) state it
    s, w = pick[:, 0].to(torch.int64), pick[:, 1].to(torch.int64)
    bad = ~((s >= 0) & (s < B) & (w >= 0) & (w < T))
    bad |= w >= cap_lens.to(torch.int64)[s.clamp(0, B - 1)]
    if bool(bad.any()):
        r = int(bad.nonzero()[0])
        raise ValueError("attn_sheet: pick row %d, (sample %d, word %d), is outside the batch of %d or at or past its caption's length"
                         % (r, int(pick[r, 0]), int(pick[r, 1]), B))
    pa, pi, pt = ptr(attn), ptr(img), ptr(table)               # (a host tensor raises here, before anything is uploaded)
    both = torch.cat([cap_lens, pick.reshape(-1)]).to(attn.device)              # one upload: 4 B + 8 P bytes
    sheet = torch.empty((P, vis, vis, 3), dtype=torch.uint8, device=attn.device)
    stats = torch.empty((P, 2), dtype=torch.float64, device=attn.device)
    flags = torch.empty((P,), dtype=torch.int32, device=attn.device)
    call("mogan_attn_sheet_f64", pa, ptr(both), pi, pt, ptr(both) + 4 * B, P, B, T, att, vis, alpha, ptr(sheet), ptr(stats),
         ptr(flags), stream_ptr())
    return sheet, stats, flags


_twiddles = {}


def twiddle_table(S):
    """The S / 2 pairs (cos, -sin)(2 pi k / S) of mogan_radial_power_f64 as a (S / 2, 2) fp64 numpy array: numpy's cos and sin of
    the fp64 angle 2 pi k / S.  The device takes them as they are, so a CPU oracle can start from the same constants."""
    import numpy as np
    ang = 2.0 * np.pi * np.arange(int(S) // 2, dtype=np.float64) / float(S)
    return np.ascontiguousarray(np.stack([np.cos(ang), -np.sin(ang)], axis=1))


def radial_power(x, weight, window, bins, n_bins, out=None):
    """Per image the sums of |F|^2 over the bins of a table (mogan_radial_power_f64; attngan/spectrum.py has the definition): fp32 x
    (B, C, S, S) with C in 1..4 and S a power of two in [8, 256], fp32 weight (C,), fp32 window (S,) or None (all ones), int32 bins
    (S, S / 2 + 1) over the half plane v in [0, S / 2] (an entry < 0 or >= n_bins leaves its frequency out), all on x's device ->
    (B, n_bins) fp64 on the device, out[b, k] = sum over the table's members of bin k of m(v) |F_b[u, v]|^2, F the unnormalised DFT of
    (sum_c weight[c] x[b, c]) window[i] window[j], m = 1 for v in {0, S / 2} and 2 otherwise.  fp64 after the loads; the same bits on
    every call, a row's bits depend on its image only, a zero image gives exactly 0.0.  `out`, where given, is a dense (B, n_bins)
    fp64 tensor on x's device (rows of a larger buffer, for one) and is returned.  The twiddle table is built once per (S, device).
    No gradient.  Nothing is converted or copied for the caller: a wrong dtype, rank, device, contiguity or size is a ValueError."""
    x = _dense_f32("radial_power", "x", x, 4)
    weight = _dense_f32("radial_power", "weight", weight, 1)
    if window is not None:
        window = _dense_f32("radial_power", "window", window, 1)
    B, C, S, n_bins = x.shape[0], x.shape[1], x.shape[2], int(n_bins)
    if C > 4 or x.shape[3] != S or S < 8 or S > 256 or S & (S - 1) or x.numel() > 2 ** 31 - 1:
        raise ValueError("radial_power: x (B, 1..4, S, S) with S a power of two in [8, 256] and fewer than 2^31 elements expected, "
                         "got %s" % (tuple(x.shape),))
    if weight.shape[0] != C:
        raise ValueError("radial_power: one weight per channel expected, got %d for %d channels" % (weight.shape[0], C))
    if window is not None and window.shape[0] != S:
        raise ValueError("radial_power: a window of S = %d values expected, got %d" % (S, window.shape[0]))
    if (not torch.is_tensor(bins) or bins.dtype != torch.int32 or tuple(bins.shape) != (S, S // 2 + 1) or not bins.is_contiguous()):
        raise ValueError("radial_power: bins must be a contiguous int32 (%d, %d) table, got %s %s"
                         % (S, S // 2 + 1, getattr(bins, "dtype", type(bins)), tuple(getattr(bins, "shape", ()))))
    if not 1 <= n_bins <= 256:
        raise ValueError("radial_power: 1 <= n_bins <= 256 expected, got %d" % n_bins)
    for name, t in (("weight", weight), ("window", window), ("bins", bins), ("out", out if torch.is_tensor(out) else None)):
        if t is not None and t.device != x.device:
            raise ValueError("radial_power: x and %s must be on one device (%s, %s)" % (name, x.device, t.device))
    if x.device.type == "meta":
        raise ValueError("radial_power: x is a meta tensor")
    if out is not None:
        if not torch.is_tensor(out) or out.dtype != torch.float64 or tuple(out.shape) != (B, n_bins) or not out.is_contiguous():
            raise ValueError("radial_power: out must be a dense fp64 %s tensor, got %s %s"
                             % ((B, n_bins), getattr(out, "dtype", type(out)), tuple(getattr(out, "shape", ()))))
    px, pw, pn, pb = ptr(x), ptr(weight), ptr(window), ptr(bins.detach())      # (a host tensor raises here, before any upload)
    key = (S, x.device)
    tw = _twiddles.get(key)
    if tw is None:
        tw = _twiddles[key] = torch.from_numpy(twiddle_table(S)).to(x.device)
    ws, ws_bytes, own = _scratch(x.device, int(lib.load().mogan_radial_power_ws_bytes(B, S)))
    if out is None:
        out = torch.empty((B, n_bins), dtype=torch.float64, device=x.device)
    call("mogan_radial_power_f64", px, B, C, S, pw, pn, ptr(tw), pb, n_bins, ptr(out), ws, ws_bytes, stream_ptr())
    if own is not None:
        own.record_stream(torch.cuda.current_stream(x.device))
    return out


class ScalarSumFn(torch.autograd.Function):
    """sum_k w_k * x_k over up to 8 zero-dim device scalars in ONE launch (forward) / one launch (backward): the loss sums
    of miscc/losses.py:169-174,203,221 and trainer.py:330 otherwise cost a chain of 0-dim aten kernels each way."""

    @staticmethod
    def forward(ctx, weights, *xs):
        import ctypes
        n = len(xs)
        xs = [_c(x) for x in xs]
        out = _scalar(xs[0].device)
        pin = (ctypes.c_void_p * n)(*[x.data_ptr() for x in xs])
        pw = (ctypes.c_float * n)(*weights)
        call("mogan_scalar_sum", ctypes.cast(pin, ctypes.c_void_p), ctypes.cast(pw, ctypes.c_void_p), n, ptr(out),
             stream_ptr())
        ctx.weights = weights
        return out

    @staticmethod
    def backward(ctx, g):
        import ctypes
        idx = [k for k in range(len(ctx.weights)) if ctx.needs_input_grad[1 + k]]
        if not idx:
            return (None,) * (1 + len(ctx.weights))
        g = _c(g)
        outs = [_scalar(g.device) for _ in idx]
        n = len(idx)
        pout = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
        pw = (ctypes.c_float * n)(*[ctx.weights[k] for k in idx])
        call("mogan_scalar_scale", ptr(g), ctypes.cast(pw, ctypes.c_void_p), n, ctypes.cast(pout, ctypes.c_void_p),
             stream_ptr())
        grads = [None] * len(ctx.weights)
        for k, o in zip(idx, outs):
            grads[k] = o
        return (None,) + tuple(grads)


def scalar_sum(xs, weights=None):
    """sum_k weights[k] * xs[k] of zero-dim fp32 device tensors (len <= 8; longer lists are summed in chunks)."""
    xs = list(xs)
    weights = [1.0] * len(xs) if weights is None else [float(w) for w in weights]
    while len(xs) > 8:
        head = ScalarSumFn.apply(tuple(weights[:8]), *xs[:8])
        xs, weights = [head] + xs[8:], [1.0] + weights[8:]
    return ScalarSumFn.apply(tuple(weights), *xs)


# ------------------------------------------------------------------------------- pooling / resize
class PoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kind, k, s, pad, OH, OW):
        x = _c(x)
        B, C, H, W = x.shape
        if kind == "max":
            oh, ow = (H - k) // s + 1, (W - k) // s + 1
            y = torch.empty((B, C, oh, ow), dtype=torch.float32, device=x.device)
            idx = torch.empty((B, C, oh, ow), dtype=torch.uint8, device=x.device)
            call("mogan_maxpool_fwd", ptr(x), ptr(y), ptr(idx), B * C, H, W, k, s, stream_ptr())
            ctx.save_for_backward(idx)
        elif kind == "avg":
            oh, ow = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
            y = torch.empty((B, C, oh, ow), dtype=torch.float32, device=x.device)
            call("mogan_avgpool_fwd", ptr(x), ptr(y), B * C, H, W, k, s, pad, stream_ptr())
        else:
            y = torch.empty((B, C, OH, OW), dtype=torch.float32, device=x.device)
            call("mogan_bilinear_fwd", ptr(x), ptr(y), B * C, H, W, OH, OW, stream_ptr())
        ctx.cfg = (kind, k, s, pad, OH, OW, tuple(x.shape))
        return y

    @staticmethod
    def backward(ctx, dy):
        kind, k, s, pad, OH, OW, shp = ctx.cfg
        B, C, H, W = shp
        dy = _c(dy)
        dx = torch.empty(shp, dtype=torch.float32, device=dy.device)
        if kind == "max":
            (idx,) = ctx.saved_tensors
            call("mogan_maxpool_bwd", ptr(idx), ptr(dy), ptr(dx), B * C, H, W, k, s, stream_ptr())
        elif kind == "avg":
            call("mogan_avgpool_bwd", ptr(dy), ptr(dx), B * C, H, W, k, s, pad, stream_ptr())
        else:
            call("mogan_bilinear_bwd", ptr(dy), ptr(dx), B * C, H, W, OH, OW, stream_ptr())
        return dx, None, None, None, None, None, None


def max_pool2d(x, k, s):
    return PoolFn.apply(x, "max", k, s, 0, 0, 0)


def avg_pool2d(x, k, s=None, pad=0):
    return PoolFn.apply(x, "avg", k, s or k, pad, 0, 0)


def bilinear_resize(x, OH, OW):
    return PoolFn.apply(x, "bilinear", 0, 0, 0, OH, OW)


# ------------------------------------------------------------------------------- optimizer
def adam_step(p, g, m, v, ema, lr, beta1, beta2, eps, step=0, dev_state=None, eps_mode=0, grad_scale=1.0,
              ema_decay=0.999):
    """In-place fused Adam (+EMA) over flat fp32 buckets (trainer.py:137-148,341-342)."""
    call("mogan_adam_step", ptr(p), ptr(g), ptr(m), ptr(v), ptr(ema), p.numel(), lr, beta1, beta2, eps, step,
         ptr(dev_state), eps_mode, grad_scale, ema_decay, stream_ptr())


def adam_prep(dev_state, lr, beta1, beta2, eps_mode=0):
    """advance the device-resident step count once: what adam_apply / adam_pack_both launches of this step then read"""
    call("mogan_adam_prep", ptr(dev_state), lr, beta1, beta2, eps_mode, stream_ptr())


def adam_apply(p, g, m, v, ema, beta1, beta2, eps, dev_state, eps_mode=0, grad_scale=1.0, ema_decay=0.999):
    """adam_step's element pass over one range of a bucket, with the step size adam_prep left in dev_state"""
    call("mogan_adam_apply", ptr(p), ptr(g), ptr(m), ptr(v), ptr(ema), p.numel(), beta1, beta2, eps, ptr(dev_state), eps_mode,
         grad_scale, ema_decay, stream_ptr())


def adam_pack_both(pk, p, g, m, v, ema, lr, beta1, beta2, eps, step=0, dev_state=None, eps_mode=0, grad_scale=1.0,
                   ema_decay=0.999, zero_g=True):
    """The Adam (+EMA) step of ONE deep convolution weight and both of its packed copies in one pass over it
    (mogan_pk_adam_pack_both); p, g, m, v, ema: the weight's ranges of the flat buckets, pk: its WeightPacks with both panels in
    use for one geometry.  The caller stamps the panels current (_stamp) behind its last launch."""
    Cout, Cin, KH, KW = pk.w.shape
    s0, s1 = pk.slots[0], pk.slots[1]
    stride, ph, pw = s0.geom
    call("mogan_pk_adam_pack_both", ptr(p), ptr(g), ptr(m), ptr(v), ptr(ema), s0.buf.data_ptr(), s1.buf.data_ptr(), Cout, Cin, KH,
         KW, stride, ph, pw, lr, beta1, beta2, eps, step, ptr(dev_state), eps_mode, grad_scale, ema_decay, 1 if zero_g else 0,
         stream_ptr())
    PK_STATS["adam_packs"] = PK_STATS.get("adam_packs", 0) + 1


# ------------------------------------------------------------------------------- text encoder (csrc/mogan_rnn.hip)
# PK_STATS counts the calls per cell: lstm_fused / gru_fused (eval), lstm_train_fused / gru_train_fused (training)
def _rnn_encoder_args(captions, lens, emb_weight, rnn, states):
    """What both text-encoder paths need checked before a pointer reaches the kernels: the module is the one-layer bidirectional
    nn.LSTM or nn.GRU with 128 units per direction, `states` is the cell's tuple of initial states ((h0, c0) or (h0,), each a
    tensor or None), the sizes are inside the kernels' limits, and every tensor (the embedding table and the initial states
    included) is float32, dense, on the captions' device and of the expected shape.
    Returns (B, T, V, E, H, Tmax, lens, ws, cell) with cell = 'lstm' or 'gru', or None (the caller keeps the stock modules)."""
    cell = "lstm" if isinstance(rnn, torch.nn.LSTM) else "gru" if isinstance(rnn, torch.nn.GRU) else None
    if (cell is None or len(states) != (2 if cell == "lstm" else 1) or rnn.num_layers != 1 or not rnn.bidirectional
            or not rnn.batch_first or rnn.hidden_size != 128 or not rnn.bias or getattr(rnn, "proj_size", 0)):
        return None
    H = rnn.hidden_size
    if captions.dim() != 2 or emb_weight.dim() != 2:
        return None
    B, T = captions.shape
    V, E = emb_weight.shape
    lens = [int(v) for v in lens]
    Tmax = max(lens) if lens else 0
    if (len(lens) != B or B > 64 or Tmax < 1 or Tmax > 32 or Tmax > T or E > 320 or E % 4 or min(lens) < 0
            or captions.dtype != torch.int64 or rnn.input_size != E):
        return None
    ws = [rnn.weight_ih_l0, rnn.weight_ih_l0_reverse, rnn.weight_hh_l0, rnn.weight_hh_l0_reverse,
          rnn.bias_ih_l0, rnn.bias_ih_l0_reverse, rnn.bias_hh_l0, rnn.bias_hh_l0_reverse]
    dev = captions.device
    if any(w.dtype != torch.float32 or not w.is_contiguous() or w.data_ptr() % 16 or w.device != dev for w in ws):
        return None
    if emb_weight.dtype != torch.float32 or not emb_weight.is_contiguous() or emb_weight.device != dev:
        return None
    for st in states:
        if st is not None and (st.dtype != torch.float32 or st.device != dev or tuple(st.shape) != (2, B, H)):
            return None
    return B, T, V, E, H, Tmax, lens, ws, cell


def _ptr_pairs(ws):
    import ctypes
    P2 = ctypes.c_void_p * 2
    arr = [P2(ws[2 * i].data_ptr(), ws[2 * i + 1].data_ptr()) for i in range(len(ws) // 2)]
    return arr, [ctypes.cast(a, ctypes.c_void_p) for a in arr]


def rnn_encoder_forward(captions, lens, emb_weight, rnn, states):
    """Embedding + one-layer bidirectional LSTM or GRU over packed captions, eval mode, no gradient, as ONE launch
    (mogan_lstm_encoder_fwd / mogan_gru_encoder_fwd); `rnn` is the nn.LSTM / nn.GRU whose parameters are used, `states` its
    initial states (h0, c0) / (h0,).  Returns (words (B, 2H, Tmax), sent (B, 2H)) or None where the kernel does not cover the
    module (then the caller keeps the stock path)."""
    import ctypes
    args = _rnn_encoder_args(captions, lens, emb_weight, rnn, states)
    if args is None:
        return None
    B, T, V, E, H, Tmax, lens, ws, cell = args
    dev = captions.device
    cap = captions if captions.is_contiguous() else captions.contiguous()
    words = torch.empty((B, 2 * H, Tmax), dtype=torch.float32, device=dev)
    sent = torch.empty((B, 2 * H), dtype=torch.float32, device=dev)
    keep, arr = _ptr_pairs(ws)
    lens_c = (ctypes.c_int * B)(*lens)
    states = [_c(st) if st is not None else None for st in states]
    call("mogan_%s_encoder_fwd" % cell, cap.data_ptr(), ctypes.cast(lens_c, ctypes.c_void_p), emb_weight.data_ptr(),
         arr[0], arr[1], arr[2], arr[3], *[ptr(st) for st in states], words.data_ptr(), sent.data_ptr(), B, T, Tmax, V, E, H,
         stream_ptr())
    PK_STATS[cell + "_fused"] = PK_STATS.get(cell + "_fused", 0) + 1
    return words, sent


class RnnEncoderFn(torch.autograd.Function):
    """The text encoder under training (csrc/mogan_rnn.hip): mogan_{lstm,gru}_encoder_train_fwd forward; backward =
    mogan_{lstm,gru}_encoder_bwd (BPTT -> the input-side and hidden-side pre-activation gate gradients dgi / dgh and the bias
    gradients dbi / dbh), the weight gradients as mogan_bmm GEMMs over the dense (B * Tmax) axis (dgi against x and W_ih, dgh
    against hprev), mogan_embedding_bwd for the table.  The GRU's two sides differ (the n block of the hidden side carries the
    factor r); the LSTM is the case dgi is dgh, dbi is dbh.  `aux` is the cell's own saved tensor: c_t (LSTM) or hn (GRU).
    Differentiable inputs: the embedding table and the eight parameters (w_ih, w_ih_reverse, w_hh, w_hh_reverse, b_ih,
    b_ih_reverse, b_hh, b_hh_reverse); the initial states get none."""

    @staticmethod
    def forward(ctx, cell, cap, lens, states, keep_mask, scale, emb_weight, *ws):
        import ctypes
        B, T = cap.shape
        V, E = emb_weight.shape
        H, Tmax = 128, max(lens)
        G = (4 if cell == "lstm" else 3) * H
        dev = cap.device
        f32 = dict(dtype=torch.float32, device=dev)
        words, sent = torch.empty((B, 2 * H, Tmax), **f32), torch.empty((B, 2 * H), **f32)
        x = torch.empty((B, Tmax, E), **f32)
        gates, aux = torch.empty((2, B, Tmax, G), **f32), torch.empty((2, B, Tmax, H), **f32)
        hprev = torch.empty((2, B, Tmax, H), **f32)
        keep, arr = _ptr_pairs(ws)
        lens_c = (ctypes.c_int * B)(*lens)
        call("mogan_%s_encoder_train_fwd" % cell, cap.data_ptr(), ctypes.cast(lens_c, ctypes.c_void_p), emb_weight.data_ptr(),
             arr[0], arr[1], arr[2], arr[3], *[ptr(st) for st in states], ptr(keep_mask), float(scale), ptr(words), ptr(sent),
             ptr(x), ptr(gates), ptr(aux), ptr(hprev), B, T, Tmax, V, E, H, stream_ptr())
        ctx.save_for_backward(x, gates, aux, hprev, ws[0], ws[1], ws[2], ws[3])
        ctx.aux = (cell, cap, lens, states, keep_mask, float(scale), emb_weight)
        return words, sent

    @staticmethod
    def backward(ctx, dwords, dsent):
        import ctypes
        x, gates, aux, hprev, wih0, wih1, whh0, whh1 = ctx.saved_tensors
        cell, cap, lens, states, keep_mask, scale, emb_weight = ctx.aux
        B, Tmax, E = x.shape
        T = cap.shape[1]
        H, G = 128, gates.shape[3]
        f32 = dict(dtype=torch.float32, device=x.device)
        dwords = _c(dwords) if dwords is not None else None
        dsent = _c(dsent) if dsent is not None else None
        dgi, dbi = torch.empty((2, B, Tmax, G), **f32), torch.empty((2, G), **f32)
        keep, arr = _ptr_pairs([whh0, whh1])
        lens_c = (ctypes.c_int * B)(*lens)
        lens_p = ctypes.cast(lens_c, ctypes.c_void_p)
        if cell == "lstm":
            dgh, dbh = dgi, dbi
            call("mogan_lstm_encoder_bwd", ptr(dwords), ptr(dsent), lens_p, ptr(gates), ptr(aux), ptr(hprev), ptr(states[1]),
                 arr[0], ptr(dgi), ptr(dbi), B, Tmax, H, stream_ptr())
        else:
            dgh, dbh = torch.empty((2, B, Tmax, G), **f32), torch.empty((2, G), **f32)
            call("mogan_gru_encoder_bwd", ptr(dwords), ptr(dsent), lens_p, ptr(gates), ptr(aux), ptr(hprev), arr[0],
                 ptr(dgi), ptr(dgh), ptr(dbi), ptr(dbh), B, Tmax, H, stream_ptr())
        need = ctx.needs_input_grad[6:]
        BT = B * Tmax
        demb = dwih = dwhh = None
        if need[1] or need[2]:
            dwih = torch.empty((2, G, E), **f32)
            bmm_raw(dgi.view(2, BT, G).transpose(1, 2), x.view(1, BT, E).expand(2, BT, E), dwih)
        if need[3] or need[4]:
            dwhh = torch.empty((2, G, H), **f32)
            bmm_raw(dgh.view(2, BT, G).transpose(1, 2), hprev.view(2, BT, H), dwhh)
        if need[0]:
            dx = torch.empty((1, BT, E), **f32)
            bmm_raw(dgi[0].view(1, BT, G), wih0.view(1, G, E), dx)
            bmm_raw(dgi[1].view(1, BT, G), wih1.view(1, G, E), dx, accumulate=True)
            gbuf = _grad_buf(emb_weight)             # the optimizer's (zeroed) gradient bucket: added to in place
            into = gbuf if gbuf is not None else torch.zeros_like(emb_weight)
            call("mogan_embedding_bwd", cap.data_ptr(), lens_p, ptr(dx), ptr(keep_mask), scale, ptr(into), B, T, Tmax,
                 emb_weight.shape[0], E, stream_ptr())
            if gbuf is not None:
                _grad_hit(gbuf)
            else:
                demb = into
        pick = lambda t, d, on: t[d] if (t is not None and on) else None
        return (None, None, None, None, None, None, demb, pick(dwih, 0, need[1]), pick(dwih, 1, need[2]),
                pick(dwhh, 0, need[3]), pick(dwhh, 1, need[4]), dbi[0] if need[5] else None, dbi[1] if need[6] else None,
                dbh[0] if need[7] else None, dbh[1] if need[8] else None)


def rnn_encoder_train(captions, lens, emb_weight, rnn, states, keep_mask=None, scale=1.0):
    """Embedding (+ dropout through `keep_mask` (B, T, E) uint8 and `scale`) + one-layer bidirectional LSTM or GRU over packed
    captions WITH gradients for the embedding table and the module's parameters (RnnEncoderFn).  Returns (words (B, 2H, Tmax),
    sent (B, 2H)) or None where the kernels do not cover the module."""
    args = _rnn_encoder_args(captions, lens, emb_weight, rnn, states)
    if args is None:
        return None
    B, T, V, E, H, Tmax, lens, ws, cell = args
    if keep_mask is not None:
        if keep_mask.dtype != torch.uint8 or keep_mask.device != captions.device or tuple(keep_mask.shape) != (B, T, E):
            return None
        keep_mask = keep_mask.contiguous()
    cap = captions if captions.is_contiguous() else captions.contiguous()
    states = tuple(_c(st.detach()) if st is not None else None for st in states)
    out = RnnEncoderFn.apply(cell, cap, lens, states, keep_mask, float(scale), emb_weight, *ws)
    PK_STATS[cell + "_train_fused"] = PK_STATS.get(cell + "_train_fused", 0) + 1
    return out
