"""The attention sheet of a generated image: the definition and its numpy oracle.

What `miscc/vis.build_super_images2` draws per word -- the word's attention map thresholded, upscaled bilinearly, smoothed by a
Gaussian, normalised by its own minimum and maximum, quantised to 8 bits and pasted over the image through a constant mask -- is
restated here so that a device kernel can be held against it byte for byte.  The upscaling and the smoothing are linear and
separable, so together they are ONE table M (vis x att), built once on the host (`table`), and the smoothed map is M A M^T.

Inputs: attn (B, T, att, att) fp32 >= 0, cap_lens (B), img (B, 3, vis, vis) fp32 in [-1, 1], M (vis, att) fp64, pick (P, 2) =
(sample, word) pairs, alpha (the mask, 180 in the reference).

  1. conf[b, t] = sum a [a > 4 / len_b] in fp64 for t < len_b, 0 otherwise (`conf_numpy`): the reference's conf_score without the
     factor 3 of its repeated channels -- the order of the words is the same.
  2. A = a [a > 2 / len_b];  S = M A M^T in fp64.
  3. lo = min S, hi = max S, v = (S - lo) / (hi - lo) * 255, q = floor(v) as u8 (the reference's np.uint8).  hi == lo: q = 0
     everywhere, flag FLAT (the reference divides 0 by 0 there).  A non-finite value in S: q = 0, stats (0, 0), flag NONFINITE.
  4. the image's byte: floor(((x + 1) / 2) * 255) clamped to 0..255, formed in fp32 with the roundings of vis._to_uint8_range.
  5. Pillow's paste(map, mask=alpha) per channel in integer arithmetic (`blend_u8`).
A pick outside the batch, or a word at or past its caption's length, gets a zero sheet, zero stats and flag NEVER.

Both thresholds are compared in fp32, as numpy compares an fp32 map with a Python float: t = fp32(2 / len) and 2 t.
numpy and torch (for `table` only); no GPU."""
import numpy as np

ALPHA = 180
OK, FLAT, NONFINITE, NEVER = 0, 1, 2, 3
ATT_MIN, ATT_MAX, VIS_MAX, T_MAX = 2, 128, 256, 32


def table(att, up, sigma=20.0):
    """M (att * up, att) fp64: F.interpolate(mode="linear", align_corners=False) by `up`, then scipy's gaussian_filter1d(sigma,
    mode="reflect"), both applied to the identity.  up == 1 gives the identity exactly (the reference skips the expansion there).
    Every entry is >= 0 and every row sums to 1 within rounding."""
    att, up = int(att), int(up)
    if att < 1 or up < 1:
        raise ValueError("table: att >= 1 and up >= 1 expected, got %d and %d" % (att, up))
    eye = np.eye(att, dtype=np.float64)
    if up == 1:
        return eye
    import torch
    import torch.nn.functional as F
    from scipy import ndimage
    lin = F.interpolate(torch.from_numpy(eye)[None], scale_factor=up, mode="linear", align_corners=False)[0].numpy().T
    return np.ascontiguousarray(ndimage.gaussian_filter1d(lin, sigma=float(sigma), axis=0, mode="reflect"))


def thresholds(length):
    """(2 / len, 4 / len) as the fp32 values a map is compared against"""
    t = np.float32(2.0 / float(length))
    return t, np.float32(2.0) * t


def conf_numpy(attn, cap_lens):
    """step 1 -> (B, T) fp64"""
    attn = np.asarray(attn)
    assert attn.dtype == np.float32 and attn.ndim == 4
    B, T = attn.shape[:2]
    out = np.zeros((B, T), dtype=np.float64)
    for b in range(B):
        n = int(cap_lens[b])
        if n < 1:
            continue
        t4 = thresholds(n)[1]
        for t in range(min(n, T)):
            a = attn[b, t]
            out[b, t] = np.sum(a.astype(np.float64) * (a > t4))
    return out


def image_u8(img):
    """step 4: (..., vis, vis) fp32 -> u8 with the fp32 roundings of ((x + 1) / 2 * 255) and numpy's truncation"""
    x = np.asarray(img)
    assert x.dtype == np.float32
    f = (x + np.float32(1)) / np.float32(2) * np.float32(255)
    f = np.where(f >= 0, np.minimum(f, np.float32(255)), np.float32(0))            # a NaN becomes 0
    return f.astype(np.uint8)


def blend_u8(image, q, alpha=ALPHA):
    """step 5: Pillow's paste through a constant mask, (image (255 - alpha) + q alpha) / 255 in its rounding"""
    t = image.astype(np.int64) * (255 - int(alpha)) + q.astype(np.int64) * int(alpha) + 128
    return (((t >> 8) + t) >> 8).astype(np.uint8)


def smooth_numpy(attn, cap_lens, M, b, t):
    """step 2 for one legal pick -> S (vis, vis) fp64"""
    a = np.asarray(attn)[b, t]
    A = a.astype(np.float64) * (a > thresholds(int(cap_lens[b]))[0])
    return M @ A @ M.T


def level_numpy(S):
    """step 3 -> (v fp64 or None, q u8, lo, hi, flag)"""
    if not np.isfinite(S).all():
        return None, np.zeros(S.shape, dtype=np.uint8), 0.0, 0.0, NONFINITE
    lo, hi = float(S.min()), float(S.max())
    if hi == lo:
        return None, np.zeros(S.shape, dtype=np.uint8), lo, hi, FLAT
    v = (S - lo) / (hi - lo) * 255
    return v, np.floor(v).astype(np.uint8), lo, hi, OK


def pick_ok(pick_row, cap_lens, B, T):
    b, t = int(pick_row[0]), int(pick_row[1])
    return 0 <= b < B and 0 <= t < T and t < int(cap_lens[b])


def sheet_numpy(attn, cap_lens, img, M, pick, alpha=ALPHA, want_v=False):
    """steps 2-5 -> (sheet (P, vis, vis, 3) u8, stats (P, 2) fp64, flags (P) int32[, v: list of (vis, vis) fp64 or None])"""
    attn, img, M = np.asarray(attn), np.asarray(img), np.asarray(M)
    assert attn.dtype == np.float32 and img.dtype == np.float32 and M.dtype == np.float64
    B, T, att = attn.shape[:3]
    vis = M.shape[0]
    assert M.shape == (vis, att) and img.shape == (B, 3, vis, vis) and attn.shape[3] == att
    pick = np.asarray(pick).reshape(-1, 2)
    P = pick.shape[0]
    sheet = np.zeros((P, vis, vis, 3), dtype=np.uint8)
    stats = np.zeros((P, 2), dtype=np.float64)
    flags = np.zeros((P,), dtype=np.int32)
    vs = []
    for p in range(P):
        if not pick_ok(pick[p], cap_lens, B, T):
            flags[p] = NEVER
            vs.append(None)
            continue
        b, t = int(pick[p, 0]), int(pick[p, 1])
        v, q, lo, hi, flag = level_numpy(smooth_numpy(attn, cap_lens, M, b, t))
        stats[p] = (lo, hi)
        flags[p] = flag
        vs.append(v)
        sheet[p] = blend_u8(image_u8(img[b]).transpose(1, 2, 0), q[:, :, None], alpha)
    return (sheet, stats, flags, vs) if want_v else (sheet, stats, flags)


def top_words(conf_row, length, topk):
    """the reference's choice: np.argsort(conf)[::-1][:topk] over the caption's words"""
    return [int(k) for k in np.argsort(np.asarray(conf_row)[:int(length)])[::-1][:int(topk)]]
