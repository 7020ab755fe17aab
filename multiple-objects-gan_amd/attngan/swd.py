"""Host side of the sliced Wasserstein distance between real and generated images (Karras et al., "Progressive Growing of GANs for
Improved Quality, Stability, and Variation", 2018, section 5 and metrics/sliced_wasserstein.py of their code; DESIGN.md section 9g;
the reference repository has no code for it).  The score reads the images themselves, at every scale of a Laplacian pyramid: it
needs no network, works at any channel count, and its per-level figures tell "coarse layout wrong" from "fine texture wrong".

The definition, in this project's words:

  Levels.      L = [S, S / 2, ..., min_res] for square S x S images; S / min_res must be a power of two (min_res 16: 256 .. 16 are
               five levels, 64 .. 16 three).
  Pyramid.     g0 = the image, fp32 as it comes in [-1, 1] -- NOT quantised to 8 bits as Karras does; the standardisation below
               removes scale and offset.  g(i+1) = pyr_down(g(i)); level i of the Laplacian pyramid is g(i) - pyr_up(g(i+1)), the
               last level is the last g itself.
                 pyr_down(x)[oy, ox] = sum_{dy, dx = -2..2} w[dy] w[dx] x[m(2 oy + dy, H), m(2 ox + dx, W)],  w = (1, 4, 6, 4, 1) / 16,
               the mirror rule leaves the edge sample out: m(i, n) = -i for i < 0, 2 n - 2 - i for i >= n.  pyr_up(x) is the same
               filter times 4 over the zero-inserted image z of size 2h x 2w (z[2y, 2x] = x[y, x], zero elsewhere) under the same
               mirror rule on z's indices; a mirrored index on an odd row or column contributes zero.  (The index rule equals
               scipy.ndimage.convolve(mode='mirror'), which Karras's code calls.)
  Descriptors. Per image and level `patches` (128) 7 x 7 neighbourhoods over all C channels, their centres uniform in
               [3, size - 3) in each axis; a descriptor is a row of C 49 values in (channel, y, x) order.
  Standardise. Per level and side every channel has its mean subtracted and is divided by its population standard deviation, both
               over all rows and the 49 positions of that channel.  A constant channel has no SWD: ValueError.
  Distance.    Per repeat (4): `dirs` (128) Gaussian directions of length C 49, normalised to unit length; both sides projected
               onto them; every direction's projections sorted; the mean over rows and directions of |sorted real - sorted fake|.
               The level's figure is the mean over the repeats times 1000; the score is the mean over the levels.
               Both sides hold the same number of rows.

The draw order is a contract (tests/test_swd_reference_cpu.py holds it):

  real-side centres   np.random.RandomState(seed)      per batch; per level from the finest down; all x, then all y
                                                       (randint(3, size - 3, B patches) each); draw j belongs to image j // patches
  fake-side centres   np.random.RandomState(seed + 1)  the same order
  directions          np.random.RandomState(seed + 2)  per level from the finest down; per repeat randn(C 49, dirs) in fp64,
                                                       normalised in fp64, rounded once to fp32
so the real side never depends on whether a fake side is computed.

The device does the work (hip/ops: pyr_down, lap_residual, swd_gather, swd_moments, swd_project, swd_absdiff; torch.sort in
between -- keys only, so the score's bits do not depend on which correct sort runs); this module draws, keeps the descriptor buffers
and forms the figures.  Descriptor memory is rows C 49 4 bytes per level and side, rows = images x patches: 2.26 GB per level and
side at 30 000 images of 3 channels, 22.6 GB for five levels and two sides.  `levels`, `draw_centres`, `draw_directions` and
`figure_from_sums` need no GPU.
"""
import math

import numpy as np

PATCH = 7
HALF = PATCH // 2
VALUES = PATCH * PATCH          # per channel and descriptor


def levels(size, min_res=16):
    """[size, size / 2, ..., min_res]; ValueError unless min_res >= 7 (a level must hold a 7 x 7 neighbourhood), size >= min_res
    and size / min_res is a power of two"""
    size, min_res = int(size), int(min_res)
    if min_res < PATCH:
        raise ValueError("swd: min_res = %d is smaller than a %d x %d neighbourhood" % (min_res, PATCH, PATCH))
    if size < min_res or size % min_res:
        raise ValueError("swd: image size %d is not min_res = %d times a power of two" % (size, min_res))
    q = size // min_res
    if q & (q - 1):
        raise ValueError("swd: image size %d is not min_res = %d times a power of two" % (size, min_res))
    out = []
    while size >= min_res:
        out.append(size)
        size //= 2
    return out


def draw_centres(rng, sizes, batch, patches):
    """One batch's centres for one side from that side's RandomState: per level of `sizes` (finest first) all x, then all y.
    Returns one int32 (batch patches, 3) table (image, cy, cx) per level; draw j belongs to image j // patches."""
    n = int(batch) * int(patches)
    image = (np.arange(n) // int(patches)).astype(np.int32)
    out = []
    for size in sizes:
        cx = rng.randint(HALF, size - HALF, n)
        cy = rng.randint(HALF, size - HALF, n)
        out.append(np.stack([image, cy.astype(np.int32), cx.astype(np.int32)], axis=1))
    return out


def check_centres(centres, batch, size):
    """ValueError unless the (R, 3) table keeps image in [0, batch) and both coordinates in [3, size - 3)"""
    c = np.asarray(centres)
    if c.ndim != 2 or c.shape[1] != 3 or c.shape[0] < 1 or not np.issubdtype(c.dtype, np.integer):
        raise ValueError("swd: centres must be an integer (R, 3) table, got %s %s" % (c.dtype, c.shape))
    lo, hi = c.min(axis=0), c.max(axis=0)
    if lo[0] < 0 or hi[0] >= batch or min(lo[1], lo[2]) < HALF or max(hi[1], hi[2]) >= size - HALF:
        raise ValueError("swd: centres outside image [0, %d), coordinates [%d, %d) at level %d: min %s, max %s"
                         % (batch, HALF, size - HALF, size, lo.tolist(), hi.tolist()))
    return c


def draw_directions(rng, channels, dirs):
    """One repeat's directions from the directions' RandomState: randn(C 49, dirs) in fp64, every column normalised to unit length in
    fp64, rounded once to fp32: (C 49, dirs) fp32, C-contiguous"""
    d = rng.randn(int(channels) * VALUES, int(dirs))
    d = d / np.sqrt(np.sum(np.square(d), axis=0, keepdims=True))
    return np.ascontiguousarray(d.astype(np.float32))


def figure_from_sums(sums, rows):
    """A level's figure from sums (repeats, dirs) fp64, sums[t, d] = sum over the rows of |sorted real - sorted fake| of direction d
    in repeat t: the mean over rows and directions per repeat (one exactly rounded sum, one division), the mean over the repeats,
    times 1000.  A python float."""
    s = np.asarray(sums, dtype=np.float64)
    if s.ndim != 2 or s.shape[0] < 1 or s.shape[1] < 1 or int(rows) < 1:
        raise ValueError("figure_from_sums: sums (repeats, dirs) and rows >= 1 expected, got %s, rows = %s" % (s.shape, rows))
    if not np.isfinite(s).all() or s.min() < 0:
        raise ValueError("figure_from_sums: a sum of absolute differences is negative or not finite")
    per_repeat = [math.fsum(row.tolist()) / (float(rows) * s.shape[1]) for row in s]
    return math.fsum(per_repeat) / len(per_repeat) * 1000.0


def check_moments(moments, level, side):
    """ValueError where a channel of a level has a zero or non-finite standard deviation (a constant channel has no SWD)"""
    m = np.asarray(moments, dtype=np.float64)
    for c in range(m.shape[0]):
        if not np.isfinite(m[c]).all() or not m[c, 1] > 0:
            raise ValueError("swd: level %d, channel %d of the %s images has mean %r and standard deviation %r -- a constant "
                             "channel has no sliced Wasserstein distance" % (level, c, side, m[c, 0], m[c, 1]))
    return m


def descriptor_bytes(n_levels, rows, channels):
    """bytes of the descriptor buffers of both sides"""
    return 2 * int(n_levels) * int(rows) * int(channels) * VALUES * 4


class SlicedWasserstein:
    """The score over a stream of batches.  size: the images' side; channels: 1 or 3; rows: descriptor rows per level and side the
    buffers are allocated for (images x patches); add(real_batch, fake_batch) takes two fp32 (B, C, size, size) device tensors,
    builds both Laplacian pyramids and gathers `patches` descriptors per image and level into the buffers; result() runs moments ->
    per repeat project, sort, absdiff -> figures and returns {"swd", "levels", "per_level", "rows"}.  Depends on nothing of any
    tree's model or config."""

    def __init__(self, size, channels, rows, patches=128, dirs=128, repeats=4, min_res=16, seed=100, device="cuda"):
        import torch
        self.sizes = levels(size, min_res)
        self.size, self.channels, self.rows = int(size), int(channels), int(rows)
        self.patches, self.dirs, self.repeats, self.seed = int(patches), int(dirs), int(repeats), int(seed)
        if self.channels not in (1, 3):
            raise ValueError("swd: 1 or 3 channels expected, got %d" % self.channels)
        if self.patches < 1 or self.repeats < 1 or not 1 <= self.dirs <= 1024:
            raise ValueError("swd: patches >= 1, repeats >= 1 and 1 <= dirs <= 1024 expected, got %d, %d, %d"
                             % (self.patches, self.repeats, self.dirs))
        if self.rows < 1 or self.rows % self.patches:
            raise ValueError("swd: rows = %d is not a positive multiple of patches = %d" % (self.rows, self.patches))
        self.device = torch.device(device)
        self.bytes = descriptor_bytes(len(self.sizes), self.rows, self.channels)
        K = self.channels * VALUES
        self.desc = {side: [torch.empty((self.rows, K), dtype=torch.float32, device=self.device) for _ in self.sizes]
                     for side in ("real", "fake")}
        self.rng = {"real": np.random.RandomState(self.seed), "fake": np.random.RandomState(self.seed + 1)}
        self.n = 0                                             # rows filled per level and side
        self.params = {"seed": self.seed, "patches": self.patches, "dirs": self.dirs, "repeats": self.repeats,
                       "min_res": self.sizes[-1]}                  # what it was made under: a shared pass's hand-over check compares it

    def pyramid(self, batch):
        """the Laplacian levels of an fp32 (B, C, size, size) batch, finest first, each (B, C, s, s)"""
        from ..hip import ops
        B, C = batch.shape[0], batch.shape[1]
        g = batch.view(B * C, self.size, self.size)
        out = []
        for s in self.sizes[:-1]:
            down = ops.pyr_down(g)
            out.append(ops.lap_residual(g, down).view(B, C, s, s))
            g = down
        out.append(g.view(B, C, self.sizes[-1], self.sizes[-1]))
        return out

    def add(self, real_batch, fake_batch, centres=None):
        """Both batches' descriptors into the buffers.  centres: None (drawn from the two sides' streams), or
        {"real": [...], "fake": [...]} with one (B patches, 3) table per level, which are checked and no stream is advanced."""
        import torch
        from ..hip import ops
        want = None
        for name, t in (("real_batch", real_batch), ("fake_batch", fake_batch)):
            if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 4 or not t.is_contiguous():
                raise ValueError("swd: %s must be a contiguous fp32 (B, C, S, S) tensor, got %s %s"
                                 % (name, getattr(t, "dtype", type(t)), tuple(getattr(t, "shape", ()))))
            if tuple(t.shape[1:]) != (self.channels, self.size, self.size) or t.shape[0] < 1:
                raise ValueError("swd: %s must be (B, %d, %d, %d), got %s" % (name, self.channels, self.size, self.size, tuple(t.shape)))
            if t.device != self.device and (t.device.type != self.device.type or self.device.index is not None):
                raise ValueError("swd: %s is on %s, the buffers are on %s" % (name, t.device, self.device))
            want = want or tuple(t.shape)
            if tuple(t.shape) != want:
                raise ValueError("swd: both sides must hold the same number of images, got %s and %s" % (want, tuple(t.shape)))
        B = want[0]
        R = B * self.patches
        if self.n + R > self.rows:
            raise ValueError("swd: %d more rows do not fit buffers of %d rows of which %d are filled" % (R, self.rows, self.n))
        for side, batch in (("real", real_batch), ("fake", fake_batch)):
            if centres is None:
                tables = draw_centres(self.rng[side], self.sizes, B, self.patches)
            else:
                tables = centres[side]
                if len(tables) != len(self.sizes) or any(len(t) != R for t in tables):
                    raise ValueError("swd: one (%d, 3) table of centres per level expected for the %s side" % (R, side))
            tables = [check_centres(t, B, s) for t, s in zip(tables, self.sizes)]
            for level, table, desc in zip(self.pyramid(batch.detach()), tables, self.desc[side]):
                ops.swd_gather(level, table, desc, self.n)
        self.n += R

    def sink(self, real, fake, take):
        """the (real, fake, take) callable of pool_codes' image_sink"""
        self.add(real[:take].float().contiguous(), fake[:take].float().contiguous())

    def result(self):
        import torch
        from ..hip import ops
        if self.n < 1:
            raise ValueError("swd: no images were added")
        rng = np.random.RandomState(self.seed + 2)
        per_level = []
        for size, real, fake in zip(self.sizes, self.desc["real"], self.desc["fake"]):
            real, fake = real[:self.n], fake[:self.n]
            mom = {"real": ops.swd_moments(real), "fake": ops.swd_moments(fake)}
            host = torch.stack([mom["real"], mom["fake"]]).cpu().numpy()          # 2 x 2 C doubles: the level's first read-back
            check_moments(host[0], size, "real")
            check_moments(host[1], size, "generated")
            sums = []
            for _ in range(self.repeats):
                d = torch.from_numpy(draw_directions(rng, self.channels, self.dirs)).to(self.device)
                pr = torch.sort(ops.swd_project(real, mom["real"], d), dim=-1).values
                pf = torch.sort(ops.swd_project(fake, mom["fake"], d), dim=-1).values
                sums.append(ops.swd_absdiff(pr, pf))
                del pr, pf
            per_level.append(figure_from_sums(torch.stack(sums).cpu().numpy(), self.n))      # ... and its second
        return {"swd": math.fsum(per_level) / len(per_level), "levels": list(self.sizes), "per_level": per_level, "rows": self.n}
