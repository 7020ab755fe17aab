"""Host side of the Frechet distance between two sets of Inception pool codes (the reference repository has
no code for it).

Two sets of (N, 2048) pooled trunk codes (CNN_ENCODER.pool_code) are summarised by their fp64 mean and covariance -- on the device,
hip/ops.feature_moments -- and compared as Gaussians:

    d = |mu1 - mu2|^2 + Tr S1 + Tr S2 - 2 Tr (S1 S2)^(1/2)

  * `frechet_distance`  the distance and its four terms, in fp64 on the host, from two symmetric eigen-decompositions;
  * `trunk_digest`      which trunk weights produced a set of codes;
  * `FeatureStats`      mean, covariance, count and digest of one set, saved as an .npz and refused for another trunk;
  * `NeighbourBank`     the codes themselves of a split's real images, with their dataset positions, saved and refused likewise.
Nothing in this module's logic needs a GPU.
"""
import hashlib

import numpy as np
import torch


def _f64(t):
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float64))
    return t.detach().to(device="cpu", dtype=torch.float64)


def frechet_distance(mu1, S1, mu2, S2):
    """(distance, terms): terms = {"mean_sq": |mu1 - mu2|^2, "tr_s1": Tr S1, "tr_s2": Tr S2, "tr_sqrt": Tr (S1 S2)^(1/2)} and
    distance = mean_sq + tr_s1 + tr_s2 - 2 tr_sqrt, python floats.

    (S1 S2) has the eigenvalues of the symmetric positive semi-definite R S2 R with R = S1^(1/2), so the last term is
    sum_i sqrt(max(lambda_i, 0)) over the eigenvalues of R S2 R (symmetrised), and R comes from torch.linalg.eigh of S1 with negative
    eigenvalues clamped to 0: no complex arithmetic, no general matrix square root, well defined for rank-deficient covariances."""
    mu1, S1, mu2, S2 = _f64(mu1), _f64(S1), _f64(mu2), _f64(S2)
    D = mu1.numel()
    if mu1.dim() != 1 or mu2.shape != mu1.shape or tuple(S1.shape) != (D, D) or tuple(S2.shape) != (D, D):
        raise ValueError("frechet_distance: mu (D,), S (D, D) twice expected, got %s, %s, %s, %s"
                         % (tuple(mu1.shape), tuple(S1.shape), tuple(mu2.shape), tuple(S2.shape)))
    w, V = torch.linalg.eigh((S1 + S1.t()) * 0.5)
    R = (V * w.clamp_min(0.0).sqrt()) @ V.t()
    M = R @ ((S2 + S2.t()) * 0.5) @ R
    lam = torch.linalg.eigvalsh((M + M.t()) * 0.5)
    diff = mu1 - mu2
    terms = {"mean_sq": float(diff.dot(diff)), "tr_s1": float(torch.trace(S1)), "tr_s2": float(torch.trace(S2)),
             "tr_sqrt": float(lam.clamp_min(0.0).sqrt().sum())}
    return terms["mean_sq"] + terms["tr_s1"] + terms["tr_s2"] - 2.0 * terms["tr_sqrt"], terms


def trunk_digest(encoder):
    """SHA-256 (hex) over the parameters and buffers of the encoder's Inception trunk -- everything in its state_dict but the two
    DAMSM heads -- in state_dict order: name, dtype, shape and bytes of each entry.  Under another trunk variant than the default
    (CNN_ENCODER.trunk_variant) a line naming it is hashed first: the same weights run as two networks give two digests, so
    statistics, banks and heads of one are refused under the other"""
    heads = tuple(getattr(encoder, "HEADS", ()))
    h = hashlib.sha256()
    variant = getattr(encoder, "trunk_variant", "torchvision")
    if variant != "torchvision":
        h.update(("trunk_variant %s\n" % variant).encode())
    for name, t in encoder.state_dict().items():
        if name.split(".")[0] in heads:
            continue
        a = t.detach().cpu().contiguous().numpy()
        h.update(("%s %s %s\n" % (name, a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


class FeatureStats:
    """fp64 mean (D,) and covariance (D, D) of `n` codes under the trunk `trunk_digest` (host tensors)"""

    def __init__(self, mean, cov, n, trunk_digest):
        self.mean, self.cov, self.n, self.trunk_digest = _f64(mean), _f64(cov), int(n), str(trunk_digest)
        D = self.mean.numel()
        if self.mean.dim() != 1 or tuple(self.cov.shape) != (D, D):
            raise ValueError("FeatureStats: mean (D,), cov (D, D) expected, got %s, %s" % (tuple(self.mean.shape), tuple(self.cov.shape)))

    def save(self, path):
        with open(path, "wb") as f:                           # (a file object: numpy appends no suffix of its own)
            np.savez(f, mean=self.mean.numpy(), cov=self.cov.numpy(), n=np.int64(self.n), trunk_digest=np.str_(self.trunk_digest))

    @classmethod
    def load(cls, path, trunk_digest, D):
        """the statistics of `path`; ValueError where they were taken under another trunk or at another feature width"""
        with np.load(path, allow_pickle=False) as z:
            mean, cov, n, digest = z["mean"], z["cov"], int(z["n"]), str(z["trunk_digest"])
        if mean.dtype != np.float64 or cov.dtype != np.float64:
            raise ValueError("%s: fp64 statistics expected, found %s / %s" % (path, mean.dtype, cov.dtype))
        if digest != str(trunk_digest):
            raise ValueError("%s was computed under another Inception trunk (digest %s..., this encoder's is %s...): statistics of "
                             "different trunks cannot be compared" % (path, digest[:12], str(trunk_digest)[:12]))
        if mean.shape != (D,) or cov.shape != (D, D):
            raise ValueError("%s holds statistics of %s features, this encoder has %d" % (path, mean.shape, D))
        return cls(mean, cov, n, digest)


def is_external_stats(path):
    """whether `path` is a TTUR / pytorch-fid statistics file: an .npz holding exactly `mu` and `sigma`"""
    try:
        with np.load(path, allow_pickle=False) as z:
            return set(z.files) == {"mu", "sigma"}
    except (OSError, ValueError):
        return False


def load_external_stats(path, D):
    """(mu (D,), sigma (D, D)), fp64 host tensors, of a TTUR / pytorch-fid statistics file.  ValueError naming the file and the
    fault where the arrays are not D wide, not finite or sigma is not symmetric.  Which network and protocol the file was computed
    under cannot be checked; such a file is never written here."""
    with np.load(path, allow_pickle=False) as z:
        if set(z.files) != {"mu", "sigma"}:
            raise ValueError("%s: exactly mu and sigma expected, found %s" % (path, sorted(z.files)))
        mu, sigma = z["mu"], z["sigma"]
    for name, a in (("mu", mu), ("sigma", sigma)):
        if a.dtype.kind not in "fiu":
            raise ValueError("%s: %s is %s, numbers expected" % (path, name, a.dtype))
    mu, sigma = np.asarray(mu, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    if mu.shape != (D,) or sigma.shape != (D, D):
        raise ValueError("%s: width -- mu %s and sigma %s, this encoder's codes are %d wide" % (path, mu.shape, sigma.shape, D))
    if not np.isfinite(mu).all() or not np.isfinite(sigma).all():
        raise ValueError("%s: non-finite values in %s" % (path, "mu" if not np.isfinite(mu).all() else "sigma"))
    asym = float(np.abs(sigma - sigma.T).max())
    if asym > 1e-6 * max(float(np.abs(sigma).max()), 1e-300):
        raise ValueError("%s: sigma is not symmetric (max |sigma - sigma^T| = %.3e)" % (path, asym))
    return _f64(mu), _f64(sigma)


class NeighbourBank:
    """fp32 pool codes (n, D) of a split's real images under the trunk `trunk_digest`, with the dataset positions (n,) their rows
    stand for and the split's name: what the memorisation figures search for nearest neighbours (host
    arrays)"""

    def __init__(self, codes, positions, trunk_digest, split):
        if torch.is_tensor(codes):
            codes = codes.detach().cpu().numpy()
        self.codes = np.ascontiguousarray(codes)
        self.positions = np.ascontiguousarray(np.asarray(positions), dtype=np.int64)
        self.trunk_digest, self.split = str(trunk_digest), str(split)
        if self.codes.dtype != np.float32 or self.codes.ndim != 2 or self.codes.shape[0] < 1 or self.codes.shape[1] < 1:
            raise ValueError("NeighbourBank: fp32 codes (n, D) expected, got %s %s" % (self.codes.dtype, self.codes.shape))
        if self.positions.shape != (self.codes.shape[0],):
            raise ValueError("NeighbourBank: one dataset position per code expected, got %s for %d codes"
                             % (self.positions.shape, self.codes.shape[0]))

    def __len__(self):
        return int(self.codes.shape[0])

    def save(self, path):
        with open(path, "wb") as f:
            np.savez(f, codes=self.codes, positions=self.positions, trunk_digest=np.str_(self.trunk_digest),
                     split=np.str_(self.split))

    @classmethod
    def load(cls, path, trunk_digest, D):
        """the bank of `path`; ValueError where it was taken under another trunk or at another feature width"""
        with np.load(path, allow_pickle=False) as z:
            codes, positions, digest, split = z["codes"], z["positions"], str(z["trunk_digest"]), str(z["split"])
        if codes.dtype != np.float32:
            raise ValueError("%s: fp32 codes expected, found %s" % (path, codes.dtype))
        if digest != str(trunk_digest):
            raise ValueError("%s was computed under another Inception trunk (digest %s..., this encoder's is %s...): codes of "
                             "different trunks cannot be compared" % (path, digest[:12], str(trunk_digest)[:12]))
        if codes.ndim != 2 or codes.shape[1] != D:
            raise ValueError("%s holds codes of shape %s, this encoder has %d features" % (path, codes.shape, D))
        return cls(codes, positions, digest, split)
