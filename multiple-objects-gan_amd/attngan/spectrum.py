"""Host side of the radial power spectrum of real and generated images (the azimuthally averaged power spectrum of Durall et al.,
"Watch your Up-Convolution", 2020; Dzanic et al., "Fourier Spectrum Discrepancies in Deep Network Generated Images", 2020; Schwarz et
al., "On the Frequency Bias of Generative Models", 2021; the spectrum plots of Karras et al., "Alias-Free Generative Adversarial
Networks", 2021; the reference repository has no code for it).  The score reads the images themselves, in the
frequency domain: it needs no network, works at 64 x 64, and says AT WHICH PERIOD a generator built from nearest-neighbour
upsamplings and 3 x 3 convolutions leaves its grids and checkerboards.

The definition, in this project's words, for fp32 images x of shape (B, C, S, S) in [-1, 1], S a power of two in [8, 256]:

  Plane.       y = sum_c weight[c] x[c]: (0.299, 0.587, 0.114) for C = 3, (1) for C = 1 (`channel_weights`), rounded once to fp32.
  Window.      y[i][j] w[i] w[j] before the transform; the default is the periodic Hann window 0.5 - 0.5 cos(2 pi i / S), formed in
               fp64 and rounded once to fp32 (`hann`); `window` None or "none" means all ones.  The host builds the vector and hands
               it to the kernel, so a test's oracle and the kernel share its bits.
  Transform.   F[u, v] = sum_ij y w w exp(-2 pi i (u i + v j) / S), unnormalised, fp64.
  Bins.        Signed frequencies fu = u for u <= S / 2, else u - S; fv likewise.  bin(u, v) = floor(sqrt(fu^2 + fv^2) + 1 / 2), in
               integer arithmetic: the r with (2 r - 1)^2 <= 4 (fu^2 + fv^2) < (2 r + 1)^2.  Bins run from 0 to bin(S / 2, S / 2);
               the corners beyond the Nyquist circle are kept -- the period-2 checkerboard lives at (S / 2, S / 2) -- so bins beyond
               S / 2 cover partial rings only.  `radial_bins` gives the table over the half plane v in [0, S / 2] and the FULL-plane
               count per bin.
  Profile.     p[k] = (sum_{bin(u, v) = k} |F[u, v]|^2) / (count[k] sum_ij (w[i] w[j])^2): a white-noise image of unit variance has
               expectation 1 in every bin.
  Side.        P[k] = the mean of p[k] over a side's images; dB[k] = 10 log10 P[k].  A bin whose P is 0 on either side is left out
               of every figure and listed as `empty_bins`.
  Figures      over k >= 1, d[k] = dB_fake[k] - dB_real[k]:
               lsd_db      sqrt(mean_k d[k]^2), the log-spectral distance;
               hf_db       10 log10 (sum_{k > S/4} count[k] P_fake[k] / sum_{k > S/4} count[k] P_real[k]): positive = too much
                           fine-scale power (noise, grids), negative = too little (blur);
               slope_real, slope_fake   the least-squares slope of dB[k] against log10 k over 1 <= k <= S / 2, dB per decade;
               peak        the bin with the largest |d[k]|, d there, and its period S / k in pixels;
               and the vectors profile_real_db, profile_fake_db, excess_db (= d) and count.

The device does the transform and the sums per bin (hip/ops.radial_power: fp64, the same bits for an image whatever batch it arrives
in, no 2-D spectrum stored); this module builds the window and the table, keeps the per-image sums and forms the figures.  The score
draws nothing.  `channel_weights`, `hann`, `radial_bins`, `window_energy` and `figures` need no GPU.
"""
import math

import numpy as np

LUMA = (0.299, 0.587, 0.114)
S_MIN, S_MAX = 8, 256
WINDOWS = ("hann", "none")


def check_size(size):
    size = int(size)
    if size < S_MIN or size > S_MAX or size & (size - 1):
        raise ValueError("spectrum: an image side that is a power of two in [%d, %d] expected, got %d" % (S_MIN, S_MAX, size))
    return size


def channel_weights(channels):
    """the fp32 weights of the plane: the luminance of 3 channels, the channel itself for 1; ValueError otherwise"""
    channels = int(channels)
    if channels == 3:
        return np.asarray(LUMA, dtype=np.float32)
    if channels == 1:
        return np.ones(1, dtype=np.float32)
    raise ValueError("spectrum: 1 or 3 channels expected, got %d" % channels)


def window_name(window):
    """'hann' or 'none' for 'hann', 'none' and None; ValueError otherwise"""
    name = "none" if window is None else window
    if name not in WINDOWS:
        raise ValueError("spectrum: window must be one of %s (or None), got %r" % (WINDOWS, window))
    return name


def hann(size):
    """the periodic Hann window 0.5 - 0.5 cos(2 pi i / S), formed in fp64 and rounded once to fp32"""
    size = check_size(size)
    i = np.arange(size, dtype=np.float64)
    return np.ascontiguousarray((0.5 - 0.5 * np.cos(2.0 * np.pi * i / size)).astype(np.float32))


def make_window(window, size):
    """the fp32 vector of a window's name, None for 'none'"""
    return hann(size) if window_name(window) == "hann" else None


def window_energy(window, size):
    """sum_ij (w[i] w[j])^2 = (sum_i w[i]^2)^2 in fp64 from the fp32 vector; S^2 for no window"""
    if window is None:
        return float(check_size(size)) ** 2
    w = np.asarray(window, dtype=np.float64)
    if w.shape != (check_size(size),):
        raise ValueError("spectrum: a window of %d values expected, got %s" % (size, w.shape))
    return float(math.fsum((w * w).tolist()) ** 2)


def bin_of(fu, fv):
    """floor(sqrt(fu^2 + fv^2) + 1 / 2) for integer arrays, in integer arithmetic"""
    q = 4 * (np.asarray(fu, dtype=np.int64) ** 2 + np.asarray(fv, dtype=np.int64) ** 2)
    r = (np.sqrt(q.astype(np.float64)) / 2.0 + 0.5).astype(np.int64)        # a first guess, off by one at the most
    r = np.where((r > 0) & ((2 * r - 1) ** 2 > q), r - 1, r)
    r = np.where((2 * r + 1) ** 2 <= q, r + 1, r)
    assert bool((((2 * r - 1) ** 2 <= q) | (r == 0)).all()) and bool(((2 * r + 1) ** 2 > q).all())
    return r


def radial_bins(size):
    """(table, count): the int32 (S, S / 2 + 1) table of bin(u, v) over the half plane v in [0, S / 2], and the int64 count of the
    FULL plane's members per bin, bins 0 .. bin(S / 2, S / 2)"""
    size = check_size(size)
    u = np.arange(size, dtype=np.int64)
    f = np.where(u <= size // 2, u, u - size)
    full = bin_of(f[:, None], f[None, :])
    count = np.bincount(full.ravel(), minlength=int(full[size // 2, size // 2]) + 1)
    return np.ascontiguousarray(full[:, :size // 2 + 1].astype(np.int32)), count.astype(np.int64)


def profiles(sums, count, energy):
    """p (N, n_bins) fp64 from the per-image sums of |F|^2 per bin: sums / (count energy)"""
    s = np.asarray(sums, dtype=np.float64)
    c = np.asarray(count, dtype=np.float64)
    if s.ndim != 2 or s.shape[0] < 1 or c.shape != (s.shape[1],) or not c.min() > 0 or not float(energy) > 0:
        raise ValueError("spectrum: sums (images, bins), a positive count per bin and a positive window energy expected, got %s, %s, %r"
                         % (s.shape, c.shape, energy))
    if not np.isfinite(s).all() or s.min() < 0:
        raise ValueError("spectrum: a sum of |F|^2 is negative or not finite")
    return s / (c * float(energy))


def side_profile(p):
    """P[k]: the mean over the images, one exactly rounded sum and one division per bin"""
    p = np.asarray(p, dtype=np.float64)
    return np.array([math.fsum(p[:, k].tolist()) / p.shape[0] for k in range(p.shape[1])], dtype=np.float64)


def _slope(db, ks):
    """least-squares slope of db[k] against log10 k over the bins ks; None for fewer than two"""
    if len(ks) < 2:
        return None
    xs = np.log10(np.asarray(ks, dtype=np.float64))
    ys = np.asarray([db[k] for k in ks], dtype=np.float64)
    xm, ym = xs.mean(), ys.mean()
    return float(((xs - xm) * (ys - ym)).sum() / ((xs - xm) ** 2).sum())


def figures(P_real, P_fake, count, size):
    """The figures of the definition from the two side profiles: a dict of python values that json can hold (an empty bin's dB
    entries are None).  ValueError where no bin k >= 1 holds power on both sides."""
    size = check_size(size)
    pr, pf = np.asarray(P_real, dtype=np.float64), np.asarray(P_fake, dtype=np.float64)
    cnt = np.asarray(count, dtype=np.int64)
    if pr.ndim != 1 or pr.shape != pf.shape or cnt.shape != pr.shape or len(pr) < 2:
        raise ValueError("spectrum: two profiles and a count of one length >= 2 expected, got %s, %s, %s" % (pr.shape, pf.shape, cnt.shape))
    if not (np.isfinite(pr).all() and np.isfinite(pf).all()) or min(pr.min(), pf.min()) < 0:
        raise ValueError("spectrum: a profile value is negative or not finite")
    n = len(pr)
    empty = [k for k in range(n) if not (pr[k] > 0 and pf[k] > 0)]
    gone = set(empty)
    db_r = [None if not pr[k] > 0 else 10.0 * math.log10(pr[k]) for k in range(n)]
    db_f = [None if not pf[k] > 0 else 10.0 * math.log10(pf[k]) for k in range(n)]
    d = [None if k in gone else db_f[k] - db_r[k] for k in range(n)]
    ks = [k for k in range(1, n) if k not in gone]
    if not ks:
        raise ValueError("spectrum: no bin k >= 1 holds power on both sides")
    lsd = math.sqrt(math.fsum(d[k] * d[k] for k in ks) / len(ks))
    high = [k for k in ks if k > size // 4]
    hf = None
    if high:
        hf = 10.0 * math.log10(math.fsum(float(cnt[k]) * pf[k] for k in high) / math.fsum(float(cnt[k]) * pr[k] for k in high))
    low = [k for k in ks if k <= size // 2]
    at = max(ks, key=lambda k: (abs(d[k]), -k))                    # the lowest bin among equals
    return {"lsd_db": lsd, "hf_db": hf, "slope_real": _slope(db_r, low), "slope_fake": _slope(db_f, low),
            "peak": {"bin": int(at), "excess_db": d[at], "period": float(size) / at},
            "profile_real_db": db_r, "profile_fake_db": db_f, "excess_db": d, "count": [int(c) for c in cnt],
            "empty_bins": empty}


class RadialSpectrum:
    """The score over a stream of batches.  size: the images' side; channels: 1 or 3; images: how many images per side the buffers
    are allocated for; window: 'hann' (default), 'none' or None; seed: kept, with the window's name, for the hand-over check of a
    shared pass -- the score draws nothing.  add(real_batch, fake_batch) takes two fp32 (B, C, size, size) device tensors and makes
    one device call per side, which writes the batch's (B, n_bins) fp64 sums into the side's preallocated (images, n_bins) buffer
    (8 n_bins bytes per image and side: 44 MB per side at 30 000 images of 256 x 256); result() reads both buffers back once and
    returns the figures with "n".  Depends on nothing of any tree's model or config."""

    def __init__(self, size, channels, images, window="hann", device="cuda", seed=100):
        import torch
        self.size, self.channels, self.images, self.seed = check_size(size), int(channels), int(images), int(seed)
        weight = channel_weights(self.channels)
        self.window = window_name(window)
        self.params = {"seed": self.seed, "window": self.window}     # what it was made under: the hand-over check compares it
        if self.images < 1:
            raise ValueError("spectrum: room for one image at least expected, got %d" % self.images)
        win = make_window(self.window, self.size)
        table, self.count = radial_bins(self.size)
        self.n_bins = len(self.count)
        self.energy = window_energy(win, self.size)
        self.device = torch.device(device)
        self.weight = torch.from_numpy(weight).to(self.device)
        self.win = None if win is None else torch.from_numpy(win).to(self.device)
        self.table = torch.from_numpy(table).to(self.device)
        self.sums = {side: torch.empty((self.images, self.n_bins), dtype=torch.float64, device=self.device)
                     for side in ("real", "fake")}
        self.n = 0                                             # images added per side

    def add(self, real_batch, fake_batch):
        import torch
        from ..hip import ops
        want = None
        for name, t in (("real_batch", real_batch), ("fake_batch", fake_batch)):
            if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 4 or not t.is_contiguous():
                raise ValueError("spectrum: %s must be a contiguous fp32 (B, C, S, S) tensor, got %s %s"
                                 % (name, getattr(t, "dtype", type(t)), tuple(getattr(t, "shape", ()))))
            if tuple(t.shape[1:]) != (self.channels, self.size, self.size) or t.shape[0] < 1:
                raise ValueError("spectrum: %s must be (B, %d, %d, %d), got %s"
                                 % (name, self.channels, self.size, self.size, tuple(t.shape)))
            if t.device != self.device and (t.device.type != self.device.type or self.device.index is not None):
                raise ValueError("spectrum: %s is on %s, the buffers are on %s" % (name, t.device, self.device))
            want = want or tuple(t.shape)
            if tuple(t.shape) != want:
                raise ValueError("spectrum: both sides must hold the same number of images, got %s and %s" % (want, tuple(t.shape)))
        B = want[0]
        if self.n + B > self.images:
            raise ValueError("spectrum: %d more images do not fit buffers of %d images of which %d are filled" % (B, self.images, self.n))
        for side, batch in (("real", real_batch), ("fake", fake_batch)):
            ops.radial_power(batch.detach(), self.weight, self.win, self.table, self.n_bins, out=self.sums[side][self.n:self.n + B])
        self.n += B

    def sink(self, real, fake, take):
        """the (real, fake, take) callable of pool_codes' image_sink"""
        self.add(real[:take].float().contiguous(), fake[:take].float().contiguous())

    def result(self):
        import torch
        if self.n < 1:
            raise ValueError("spectrum: no images were added")
        both = torch.stack([self.sums["real"][:self.n], self.sums["fake"][:self.n]]).cpu().numpy()       # the one read-back
        P = [side_profile(profiles(s, self.count, self.energy)) for s in both]
        return dict(figures(P[0], P[1], self.count, self.size), n=self.n)
