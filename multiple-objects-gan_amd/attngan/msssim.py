"""Host side of the multi-scale structural similarity between pairs of images (Wang, Simoncelli & Bovik, "Multi-scale structural
similarity for image quality assessment", 2003; used as a diversity score for GANs by Odena et al., "Conditional Image Synthesis with
Auxiliary Classifier GANs", 2017, and reported next to SWD by Karras et al. 2018; the reference repository has
no code for it).  The score reads the images themselves: it needs no network, works at any channel count and at 64 x 64.  A HIGH
mean over pairs means images that are alike: a generator that ignores its noise scores 1 on pairs that share their conditioning.

The definition, in this project's words, for two fp32 images a, b of shape (C, S, S) in [-1, 1]:

  Scales.      L = `scales` (5) levels of side S, S / 2, ..., S / 2^(L-1); S must be divisible by 2^(L-1) and the coarsest side
               must be >= 4 (256: 256 .. 16; 64: 64 .. 4).  The next level is the aligned 2 x 2 mean of the level above,
               ((x00 + x01) + (x10 + x11)) / 4.
  Window.      n = min(11, side) taps, sigma = 1.5 n / 11 (the shrink rule of the TF msssim.py that Odena and Karras used);
               g[k] ~ exp(-(k - (n - 1) / 2)^2 / (2 sigma^2)), normalised in fp64 and rounded ONCE to fp32.  Separable, applied at
               valid positions only: (side - n + 1)^2 per channel.  The host computes it and hands it to the kernel, so a test's
               oracle and the kernel share its bits.
  Values.      The image is not quantised to 8 bits (as with SWD).  d = 127.5 x is the CENTRED value, mu = 127.5 + G*d;
               s_aa = G*(d_a d_a) - (G*d_a)^2, likewise s_bb, s_ab = G*(d_a d_b) - (G*d_a)(G*d_b): the variance terms are
               formed on the centred values (in fp32 the uncentred 0..255 form loses two decimal digits to cancellation).
               C1 = 6.5025, C2 = 58.5225;
                 cs   = (2 s_ab + C2) / ((s_aa + s_bb) + C2)
                 l    = (2 (mu_a mu_b) + C1) / ((mu_a mu_a + mu_b mu_b) + C1)
                 ssim = l cs
  Level terms. (mean ssim, mean cs) over all channels and valid positions.
  Score.       prod_{j < L-1} max(cs_j, 0)^w_j  x  max(ssim_{L-1}, 0)^w_{L-1},  w = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333) as it
               stands for L = 5; for L < 5 the first L weights divided by their sum.  A negative level mean is clamped to 0 where
               the published code would give NaN: the pair scores 0 and is counted as `clamped`.  The score is formed on the host
               in fp64 from the terms (score_from_terms).

Two properties hold bit for bit (the kernel writes numerator and denominator without contraction, 2 (x y) against x x + y y):
a pair of bit-identical images has ssim = cs = 1.0 exactly at every level, and exchanging a and b gives the same bits.  The same
inputs give the same bits on every call.

The device does the work (hip/ops.ssim_level, one launch per level for all pairs of a batch plus one that finishes the sums;
hip/ops.avg_down2 between the levels); this module keeps the windows and the terms and forms the figures.  `scales_of`, `window`
and `score_from_terms` need no GPU.
"""
import math

import numpy as np

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
TAPS = 11
SIGMA = 1.5
C1, C2 = 6.5025, 58.5225        # (0.01 * 255)^2, (0.03 * 255)^2


def scales_of(size, scales=5):
    """[size, size / 2, ..., size / 2^(scales - 1)]; ValueError unless 1 <= scales <= 5, size is divisible by 2^(scales - 1) and
    the coarsest side is at least 4"""
    size, scales = int(size), int(scales)
    if not 1 <= scales <= len(WEIGHTS):
        raise ValueError("msssim: 1 to %d scales expected, got %d" % (len(WEIGHTS), scales))
    step = 1 << (scales - 1)
    if size < 1 or size % step or size // step < 4:
        raise ValueError("msssim: an image side of %d does not give %d scales (it must be a multiple of %d and at least %d)"
                         % (size, scales, step, 4 * step))
    return [size >> j for j in range(scales)]


def window(side):
    """The level's separable window: n = min(11, side) taps, sigma = 1.5 n / 11, normalised in fp64, rounded once to fp32"""
    side = int(side)
    if side < 1:
        raise ValueError("msssim: a level of side %d has no window" % side)
    n = min(TAPS, side)
    sigma = SIGMA * n / TAPS
    k = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
    g = np.exp(-(k * k) / (2.0 * sigma * sigma))
    return np.ascontiguousarray((g / g.sum()).astype(np.float32))


def weights_of(scales):
    """the first `scales` of the five published exponents; divided by their sum where there are fewer than five"""
    w = np.asarray(WEIGHTS[:int(scales)], dtype=np.float64)
    return w if len(w) == len(WEIGHTS) else w / w.sum()


def score_from_terms(terms):
    """terms (..., L, 2) fp64 = (mean ssim, mean cs) per level, finest first -> (score, clamped) of shape (...): the product of
    max(cs_j, 0)^w_j over the first L - 1 levels and max(ssim_{L-1}, 0)^w_{L-1}, in fp64; clamped is True where a level mean that
    enters the product is negative (the score is then 0)."""
    t = np.asarray(terms, dtype=np.float64)
    if t.ndim < 2 or t.shape[-1] != 2 or not 1 <= t.shape[-2] <= len(WEIGHTS):
        raise ValueError("score_from_terms: terms (..., 1..%d levels, 2) expected, got %s" % (len(WEIGHTS), t.shape))
    if not np.isfinite(t).all():
        raise ValueError("score_from_terms: a level term is not finite")
    used = np.concatenate([t[..., :-1, 1], t[..., -1:, 0]], axis=-1)              # cs of every level but the last, ssim of the last
    clamped = (used < 0).any(axis=-1)
    score = np.prod(np.power(np.maximum(used, 0.0), weights_of(t.shape[-2])), axis=-1)
    return score, clamped


class PairSimilarity:
    """The score over a stream of batches of pairs.  size: the images' side; channels: 1..4; pairs: how many pairs the term buffer
    is allocated for; add(a_batch, b_batch) takes two fp32 (B, C, size, size) device tensors -- row j of one is paired with row j
    of the other --, runs all levels and appends the (B, L, 2) fp64 terms to the buffer on the device (nothing is read back);
    result() reads the buffer back once and returns {"mean", "std" (population), "cs" and "ssim" (per-level means), "levels",
    "pairs", "clamped"}.  Depends on nothing of any tree's model or config."""

    def __init__(self, size, channels, pairs, scales=5, device="cuda"):
        import torch
        self.sizes = scales_of(size, scales)
        self.size, self.channels, self.pairs, self.scales = int(size), int(channels), int(pairs), int(scales)
        if not 1 <= self.channels <= 4:
            raise ValueError("msssim: 1 to 4 channels expected, got %d" % self.channels)
        if self.pairs < 1:
            raise ValueError("msssim: room for one pair at least expected, got %d" % self.pairs)
        self.device = torch.device(device)
        self.windows = [torch.from_numpy(window(s)).to(self.device) for s in self.sizes]
        self.terms = torch.empty((self.pairs, len(self.sizes), 2), dtype=torch.float64, device=self.device)
        self.n = 0                                             # pairs added

    def add(self, a_batch, b_batch):
        import torch
        from ..hip import ops
        want = None
        for name, t in (("a_batch", a_batch), ("b_batch", b_batch)):
            if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 4 or not t.is_contiguous():
                raise ValueError("msssim: %s must be a contiguous fp32 (B, C, S, S) tensor, got %s %s"
                                 % (name, getattr(t, "dtype", type(t)), tuple(getattr(t, "shape", ()))))
            if tuple(t.shape[1:]) != (self.channels, self.size, self.size) or t.shape[0] < 1:
                raise ValueError("msssim: %s must be (B, %d, %d, %d), got %s" % (name, self.channels, self.size, self.size, tuple(t.shape)))
            if t.device != self.device and (t.device.type != self.device.type or self.device.index is not None):
                raise ValueError("msssim: %s is on %s, the buffer is on %s" % (name, t.device, self.device))
            want = want or tuple(t.shape)
            if tuple(t.shape) != want:
                raise ValueError("msssim: both sides must hold the same number of images, got %s and %s" % (want, tuple(t.shape)))
        B = want[0]
        if self.n + B > self.pairs:
            raise ValueError("msssim: %d more pairs do not fit a buffer of %d pairs of which %d are filled" % (B, self.pairs, self.n))
        a, b = a_batch.detach(), b_batch.detach()
        for j, (s, win) in enumerate(zip(self.sizes, self.windows)):
            self.terms[self.n:self.n + B, j] = ops.ssim_level(a, b, win)
            if j + 1 < len(self.sizes):
                a = ops.avg_down2(a.view(B * self.channels, s, s)).view(B, self.channels, s // 2, s // 2)
                b = ops.avg_down2(b.view(B * self.channels, s, s)).view(B, self.channels, s // 2, s // 2)
        self.n += B

    def result(self):
        if self.n < 1:
            raise ValueError("msssim: no pairs were added")
        terms = self.terms[:self.n].cpu().numpy()              # the one read-back
        score, clamped = score_from_terms(terms)
        mean = math.fsum(score.tolist()) / self.n
        std = math.sqrt(math.fsum(((score - mean) ** 2).tolist()) / self.n)
        per_level = [[math.fsum(terms[:, j, t].tolist()) / self.n for j in range(len(self.sizes))] for t in (0, 1)]
        return {"mean": mean, "std": std, "ssim": per_level[0], "cs": per_level[1], "levels": list(self.sizes), "pairs": self.n,
                "clamped": int(clamped.sum())}


class PairFigures:
    """The figures of a pass over real and generated images, one PairSimilarity each under `figures`: "real" and "generated" --
    within a batch, of the `take` leading images, row j is paired with row j + take // 2 for j < take // 2 -- and, with
    `same_caption`, "same_caption": every generated image against a second one for the same conditioning.  images: how many images
    the pass will see at most.  `sink` is the (real, fake, take) callable of pool_codes' image_sink, `resample_sink` the (fake,
    fake_again, take) callable of its resample_sink (None without `same_caption`); `seed` is kept for the hand-over check only."""

    def __init__(self, size, channels, images, scales=5, same_caption=True, seed=100, device="cuda"):
        self.seed, self.scales, self.same_caption = int(seed), int(scales), bool(same_caption)
        self.params = {"seed": self.seed, "scales": self.scales, "same_caption": self.same_caption}      # for the hand-over check
        self.figures = {name: PairSimilarity(size, channels, max(1, int(images) // 2), scales, device) for name in ("real", "generated")}
        if self.same_caption:
            self.figures["same_caption"] = PairSimilarity(size, channels, int(images), scales, device)
        else:
            self.resample_sink = None                          # the pass then generates no second image

    def sink(self, real, fake, take):
        half = take // 2
        if half:
            for name, t in (("real", real), ("generated", fake)):
                t = t[:2 * half].float()
                self.figures[name].add(t[:half].contiguous(), t[half:].contiguous())

    def resample_sink(self, fake, fake_again, take):
        self.figures["same_caption"].add(fake[:take].float().contiguous(), fake_again[:take].float().contiguous())
