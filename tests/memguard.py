"""Memory-contract checks for kernels that write channel slices of larger tensors (a plain helper module, not a conftest).

Every output slice lives in a parent tensor, and the parent in a flat buffer with guard bands on both sides.  Before the call
everything outside the slice holds SENTINEL bits, the slice holds POISON (write mode: a NaN no kernel computes) or a finite
base (accumulate mode).  After the call `Guarded.check` verifies
  * nothing outside the slice changed (bitwise -- band, the parent's other channels, other images);
  * no element of the slice still holds POISON (every element was written);
  * the slice equals the expected values (within the caller's tolerance, or bitwise).
`Frozen` snapshots an input and verifies it bitwise unchanged; `poison_` fills a workspace.  Poison is data, never an address:
the bands lie inside the test's own allocation.  Works on CPU and GPU tensors alike.
"""
import torch

SENTINEL = 0x7FA5A5A5        # fp32 bits outside the slice (a NaN)
POISON = 0xFFC0DEAD - (1 << 32)   # fp32 bits inside a slice in write mode (0xFFC0DEAD, a negative NaN), as int32
SENTINEL_U8, POISON_U8 = 0xA5, 0xFF
BAND = 1024                  # guard elements on each side of the parent


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.uint8)


def poison_(t):
    """fill t (fp32 or uint8) with the POISON pattern"""
    if t.dtype == torch.float32:
        _bits(t).fill_(POISON)
    else:
        t.view(torch.uint8).fill_(POISON_U8)
    return t


class Guarded:
    """`shape` parent (fp32 or uint8) inside a guard-banded buffer; `view` = parent[index] is the slice under test.
    base: None = write mode (slice poisoned), else a tensor broadcastable to the slice (accumulate mode)."""

    def __init__(self, shape, index, device, dtype=torch.float32, base=None, band=BAND):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.empty(n + 2 * band, dtype=dtype, device=device)
        _bits(self.buf).fill_(SENTINEL if dtype == torch.float32 else SENTINEL_U8)
        self.parent = self.buf[band:band + n].view(shape)
        self.view = self.parent[index]
        if base is None:
            poison_(self.view)
        else:
            self.view.copy_(base)
        self.base = None if base is None else self.view.clone()
        self.inside = torch.zeros(self.buf.shape, dtype=torch.bool, device=device)
        self.inside[band:band + n].view(shape)[index] = True
        self.before = _bits(self.buf).clone()
        self.dtype = dtype

    @property
    def ptr(self):
        return self.view.data_ptr()

    @property
    def bstride(self):
        return self.parent.stride(0)

    def reset(self):
        """the state before the call again (poison or base, sentinels outside), for a second call into the same buffer"""
        _bits(self.buf).copy_(self.before)

    def untouched(self):
        """whether every element, inside and outside the slice, still holds what it held before the call (a declined call)"""
        return bool((_bits(self.buf) == self.before).all())

    def problems(self, expect=None, atol=None, exact=False, written=True):
        """list of violated contract items (empty = all fine); expect: the slice's expected values (fp64 or exact);
        written=False: no "never written" item (a byte image whose bytes may equal the poison pattern, or that has padding)"""
        out = []
        bits = _bits(self.buf)
        outside = (bits != self.before) & ~self.inside
        if bool(outside.any()):
            pos = torch.nonzero(outside).flatten()
            out.append("%d elements outside the slice changed (first at buffer index %d, last %d)"
                       % (pos.numel(), int(pos[0]), int(pos[-1])))
        vb = _bits(self.view)
        pz = (vb == (POISON if self.dtype == torch.float32 else POISON_U8))
        if written and self.base is None and bool(pz.any()):
            out.append("%d slice elements never written (first at %s)" % (int(pz.sum()), tuple(torch.nonzero(pz)[0].tolist())))
        if expect is not None:
            got = self.view.cpu()
            exp = expect.cpu()
            if exact:
                bad = _bits(got.contiguous()) != _bits(exp.to(got.dtype).contiguous())
            else:
                err = (got.double() - exp.double()).abs()
                bad = ~(err <= atol.cpu().double() if torch.is_tensor(atol) else err <= atol)
            if bool(bad.any()):
                i = tuple(torch.nonzero(bad)[0].tolist())
                out.append("%d slice elements off the expected values (first at %s: got %r, want %r)"
                           % (int(bad.sum()), i, float(got[i]), float(exp[i])))
        return out

    def check(self, expect=None, atol=None, exact=False, what="", written=True):
        p = self.problems(expect, atol, exact, written)
        assert not p, "%s: %s" % (what, "; ".join(p))


class Frozen:
    """an input whose bits must not change"""

    def __init__(self, t):
        self.t, self.snap = t, _bits(t.contiguous()).clone()

    def check(self, what=""):
        assert torch.equal(_bits(self.t.contiguous()), self.snap), "%s: an input was modified" % what


class Banded:
    """a freshly allocated tensor for code under test: payload poisoned (fp32 POISON / uint8 POISON_U8), `band` SENTINEL
    elements on both sides; `intact()` tells whether the bands are untouched"""

    def __init__(self, shape, dtype, device, band=BAND):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.empty(n + 2 * band, dtype=dtype, device=device)
        _bits(self.buf).fill_(SENTINEL if dtype == torch.float32 else SENTINEL_U8)
        self.t = poison_(self.buf[band:band + n]).view(shape)
        self.band = band

    def intact(self):
        b = _bits(self.buf)
        s = SENTINEL if self.buf.dtype == torch.float32 else SENTINEL_U8
        return bool((b[:self.band] == s).all()) and bool((b[b.numel() - self.band:] == s).all())
