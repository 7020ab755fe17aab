"""The ReLU and max-pool decisions a HIP run of the frozen Inception trunk made, in the form the fp64 oracle's hooks take
(oracle/inception_oracle.py: RELU_MASKS keyed by torchvision layer name, POOL_ARGMAX keyed by pool site).  A plain helper
module for the GPU tests.

ReLU mask = post-ReLU output > 0: exactly the test the backward's `relu_of` / tail `mask` makes.  Max-pool decisions: the
kernel's own idx bytes where a tape keeps them (FrozenTrunk, and the stem of PanelTrunk), else the first maximum of the
GPU's fp32 pool input recomputed on the CPU (the kernel's rule)."""
import contextlib

import torch

from oracle import inception_oracle as IO

POOL_SITE = {64: "pool1", 192: "pool2", 288: "Mixed_6a.pool", 768: "Mixed_7a.pool"}     # by pooled channels


def tape_decisions(tp, masks, pools):
    """decisions of a FrozenTrunk tape (_Tape): every convolution and max-pool it planned a backward for"""
    for levels in tp.bwd_levels:
        for level in levels:
            for op in level:
                if op.kind == "conv":
                    parts = [op.y.t[:, op.y.c0:op.y.c0 + op.y.C]]
                    if op.y2 is not None:
                        parts.append(op.y2.t[:, op.y2.c0:op.y2.c0 + op.y2.C])
                    out = torch.cat(parts, 1)
                    assert out.shape[1] == sum(op.fc.couts)
                    for n, o in zip(op.fc.names, out.split(op.fc.couts, 1)):
                        masks[n] = (o > 0).cpu()
                elif op.kind == "maxpool":
                    pools[POOL_SITE[op.x.C]] = op.idx.cpu()


@contextlib.contextmanager
def recording(monkeypatch):
    """while active, every forward tail member of a PanelTrunk block is recorded: yields a list that receives
    (layer name, _PS output slice)"""
    from mogan_amd.attngan import inception
    rec = []
    fwd = inception.PanelTrunk._fwd

    def _fwd(raw, fc, i, out, box=0):
        rec.append((fc.names[i], out))
        return fwd(raw, fc, i, out, box)
    with monkeypatch.context() as m:
        m.setattr(inception.PanelTrunk, "_fwd", staticmethod(_fwd))
        yield rec


def panel_decisions(rec, masks):
    for name, out in rec:
        masks[name] = (out.t.f32[:, out.c0:out.c0 + out.n] > 0).cpu()


def decisions(trunk, tapes, rec=None):
    """({layer: mask}, {pool site: window offsets}) of one forward of `trunk` (FrozenTrunk or PanelTrunk; `rec` = what
    `recording` collected during a PanelTrunk forward).  Call after the forward has finished on the GPU."""
    torch.cuda.synchronize()
    masks, pools = {}, {}
    if isinstance(tapes, tuple):                     # PanelTrunk: (stem tape, panel tape)
        tp, pt = tapes
        tape_decisions(tp, masks, pools)
        panel_decisions(rec, masks)
        for (name, kind, _), (X, _, _) in zip(trunk.blocks, pt.chain):
            if kind in ("InceptionB", "InceptionD"):
                pools[name + ".pool"] = IO.pool_offsets(X.f32.cpu())
    else:
        tape_decisions(tapes, masks, pools)
    assert len(masks) == 94 and len(pools) == 4, (len(masks), sorted(pools))
    return masks, pools


@contextlib.contextmanager
def imposed(masks, pools):
    """the oracle evaluates with these decisions; yields the FLIPS record"""
    flips = {}
    IO.RELU_MASKS, IO.POOL_ARGMAX, IO.FLIPS = masks, pools, flips
    try:
        yield flips
    finally:
        IO.RELU_MASKS = IO.POOL_ARGMAX = IO.FLIPS = None


def flip_summary(flips):
    """(imposed decisions that differ from the oracle's own, worst distance to the kink relative to the site's rms)"""
    n = sum(v[0] for v in flips.values())
    worst = max((v[2] / v[3] for v in flips.values() if v[0]), default=0.0)
    return n, worst
