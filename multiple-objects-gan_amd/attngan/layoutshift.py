"""Host side of the layout-shift score (the reference repository has no code for it; the paper shows the
property in its moved-box figures only).  Every score of sections 9c-9m generates at the DATA's boxes; a generator that paints each
caption's or class's typical layout passes all of them and may still not respond when a box is moved.  This one generates every
image twice from the same noise, text and labels -- A under the data's layout, B with ONE box moved -- and measures whether the
object travelled with its box and whether anything else changed.  It depends on nothing of any tree's model or config.

The definition, in this project's words:

  Objects.     An image's objects are scenefid.object_list's: the boxes (x, y, w, h), relative, with w > 0, h > 0 and
               min(w, h) * S >= min_side pixels, S the images' side.
  Rectangle.   A box's pixel rectangle [x0, x1) x [y0, y1) at side S, in fp64 from the fp32 box (pixel_rect):
                   x0 = clamp(floor(x S + 1/2), 0, S - 1)        x1 = clamp(floor((x + w) S + 1/2), x0 + 1, S)        y likewise.
  Edit.        Image i of the pass, counted globally, draws from numpy.random.default_rng([seed, i]) (draw_edit), so its edit
               depends neither on the batch size nor on num_samples: one slot, uniformly among the image's objects; then one integer
               offset (dx, dy), uniformly among the offsets that keep the rectangle inside the image and have
               max(|dx|, |dy|) >= min_shift (pixels; S / 8 by default), enumerated dy-major (dy ascending, within it dx ascending).
               An image with no object is `no_objects`, one whose drawn object has no feasible offset `immovable`: both are left out
               and counted.  The moved box is (x + dx / S, y + dy / S, w, h), each sum in fp64 and rounded once to fp32; its
               rectangle IS the old rectangle plus (dx, dy), not a recomputation.
  Classes.     Of a pair's pixels, disjoint: 0 old rectangle only; 1 new rectangle only; 2 both; 3 outside both and inside the
               rectangle of another object of the image; 4 the rest.
  Sums.        A the image under the data's layout, B under the edit, delta = (dx, dy); fp64 after the fp32 loads:
                   s[k], k = 0..4   sum over class k and all channels of (A - B)^2
                   s[5] "moved"     sum over the old rectangle of (A[p] - B[p + delta])^2
                   s[6] "baseline"  sum over the old rectangle of (A[p] - A[p + delta])^2
                   count[k]         pixels of class k
               hip/ops.box_shift_sums on the device, one launch per batch; sums_numpy here is its oracle.
  Figures.     follow = 1 - moved / baseline per pair: 1 -- the object travelled with its box, 0 -- the generator ignored the edit.
               A pair with baseline == 0 is `flat`, left out of follow and counted.  locality = (s0 + s1 + s2) / sum_k s[k], next
               to area_share = (c0 + c1 + c2) / S^2, its chance level.  A pair with sum_k s[k] == 0 is `unchanged`: left out of
               locality and counted, its follow is 0.  change[k]: the mean squared change per pixel and channel of class k, over
               the pairs that have pixels of it.  spill_others and spill_background: class 3's and class 4's mean squared change
               per pixel divided by that of the three box classes together, over the pairs where both exist and the latter is not 0.
               Every figure is mean +- population std over its pairs with the integer count beside it.  most_ignored: the `show`
               pairs of lowest follow (the earlier pair first among equals) with image position, key, slot, rectangle and offset.

pixel_rect, draw_edit, classes_numpy, sums_numpy and figures need no GPU.  ShiftResponse is the accumulator a pass fills: of it only
`sums` (hip/ops.box_shift_sums unless the caller hands another over, sums_numpy for one) needs the device.
"""
import math

import numpy as np

N_SUMS, N_CLASSES = 7, 5
MAX_OTHERS = 8
CLASS_NAMES = ("old_only", "new_only", "both", "others", "rest")


def default_min_shift(size):
    return max(1, int(size) // 8)


def pixel_rect(box, size):
    """(x0, y0, x1, y1) of the fp32 box (x, y, w, h) at side `size`: fp64 arithmetic on the fp32 values, the rounding of the
    module's docstring; never empty, always inside the image"""
    S = int(size)
    x, y, w, h = (float(np.float32(v)) for v in box)

    def axis(lo, ext):
        p0 = min(max(int(math.floor(lo * S + 0.5)), 0), S - 1)
        p1 = min(max(int(math.floor((lo + ext) * S + 0.5)), p0 + 1), S)
        return p0, p1
    (x0, x1), (y0, y1) = axis(x, w), axis(y, h)
    return x0, y0, x1, y1


def feasible_offsets(rect, size, min_shift):
    """the integer offsets (dx, dy) that keep `rect` inside the image with max(|dx|, |dy|) >= min_shift, dy-major"""
    x0, y0, x1, y1 = rect
    S, m = int(size), int(min_shift)
    return [(dx, dy) for dy in range(-y0, S - y1 + 1) for dx in range(-x0, S - x1 + 1) if max(abs(dx), abs(dy)) >= m]


def objects_of(boxes, size, min_side=1):
    """the slots of one image's objects, boxes (G, 4) fp32: scenefid.object_list's rule, asked slot by slot"""
    import torch
    from .scenefid import object_list
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(boxes, dtype=np.float32).reshape(-1, 1, 4)))
    return [int(g) for g in object_list(t, t.shape[0], size, min_side)[0]]


def draw_edit(boxes, size, seed, i, min_shift=None, min_side=1):
    """The edit of image `i` (its global position in the pass) with boxes (G, 4) fp32: "no_objects", "immovable", or a dict with
    "slot", "rect" (x0, y0, x1, y1), "offset" (dx, dy), "box" -- the moved box, (4,) fp32 -- and "others", the rectangles of the
    image's other objects in slot order."""
    S = int(size)
    m = default_min_shift(S) if min_shift is None else int(min_shift)
    if m < 1:
        raise ValueError("layoutshift: min_shift must be 1 pixel at least, got %d" % m)
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    slots = objects_of(boxes, S, min_side)
    if not slots:
        return "no_objects"
    rng = np.random.default_rng([int(seed), int(i)])
    slot = slots[int(rng.integers(len(slots)))]
    rect = pixel_rect(boxes[slot], S)
    offsets = feasible_offsets(rect, S, m)
    if not offsets:
        return "immovable"
    dx, dy = offsets[int(rng.integers(len(offsets)))]
    x, y, w, h = boxes[slot]
    moved = np.array([np.float32(float(x) + dx / float(S)), np.float32(float(y) + dy / float(S)), w, h], dtype=np.float32)
    return {"slot": slot, "rect": rect, "offset": (dx, dy), "box": moved,
            "others": [pixel_rect(boxes[g], S) for g in slots if g != slot]}


def _row_ok(e, S):
    """the legality of an edit row: the rule hip/ops.box_shift_sums raises on and the kernel of csrc/mogan_layout.hip answers with zeros"""
    x0, y0, x1, y1, dx, dy = (int(v) for v in e)
    return (x0 >= 0 and y0 >= 0 and x1 > x0 and y1 > y0 and x1 <= S and y1 <= S
            and x0 + dx >= 0 and y0 + dy >= 0 and x1 + dx <= S and y1 + dy <= S)


def classes_numpy(size, edit, others=()):
    """(S, S) int8: the class of every pixel under the edit row (x0, y0, x1, y1, dx, dy) and the other objects' rectangles"""
    S = int(size)
    x0, y0, x1, y1, dx, dy = (int(v) for v in edit)
    yy, xx = np.mgrid[0:S, 0:S]
    old = (xx >= x0) & (xx < x1) & (yy >= y0) & (yy < y1)
    new = (xx >= x0 + dx) & (xx < x1 + dx) & (yy >= y0 + dy) & (yy < y1 + dy)
    other = np.zeros((S, S), dtype=bool)
    for r in np.asarray(others, dtype=np.int64).reshape(-1, 4):
        if r[2] > r[0]:
            other |= (xx >= r[0]) & (xx < r[2]) & (yy >= r[1]) & (yy < r[3])
    cls = np.full((S, S), 4, dtype=np.int8)
    cls[other] = 3
    cls[old & ~new] = 0
    cls[new & ~old] = 1
    cls[old & new] = 2
    return cls


def sums_numpy(a, b, edit, others=None):
    """The oracle of hip/ops.box_shift_sums: a, b (P, C, S, S) fp32, edit (P, 6) and others (P, G, 4) integers (arrays or host
    tensors) -> (sums (P, 7) fp64, counts (P, 5) int32), numpy.  A row the device would answer with zeros gets zeros."""
    def host(t):
        return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    a, b, edit = host(a), host(b), host(edit).astype(np.int64)
    if a.dtype != np.float32 or b.dtype != np.float32 or a.ndim != 4 or a.shape != b.shape or a.shape[2] != a.shape[3]:
        raise ValueError("layoutshift: fp32 a and b of one shape (P, C, S, S) expected")
    P, C, S, _ = a.shape
    others = np.zeros((P, 0, 4), dtype=np.int64) if others is None else host(others).astype(np.int64)
    if edit.shape != (P, 6) or others.ndim != 3 or others.shape[0] != P or others.shape[2] != 4:
        raise ValueError("layoutshift: edit (P, 6) and others (P, G, 4) expected")
    sums = np.zeros((P, N_SUMS), dtype=np.float64)
    counts = np.zeros((P, N_CLASSES), dtype=np.int32)
    for p in range(P):
        if not _row_ok(edit[p], S):
            continue
        x0, y0, x1, y1, dx, dy = (int(v) for v in edit[p])
        A, B = a[p].astype(np.float64), b[p].astype(np.float64)
        cls = classes_numpy(S, edit[p], others[p])
        d2 = ((A - B) ** 2).sum(axis=0)
        for k in range(N_CLASSES):
            sums[p, k] = d2[cls == k].sum()
            counts[p, k] = int((cls == k).sum())
        old = A[:, y0:y1, x0:x1]
        sums[p, 5] = ((old - B[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx]) ** 2).sum()
        sums[p, 6] = ((old - A[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx]) ** 2).sum()
    return sums, counts


def follow_of(sums):
    """follow per pair of sums (n, 7): 1 - moved / baseline; 0 for an unchanged pair; NaN for a flat one"""
    s = np.asarray(sums, dtype=np.float64).reshape(-1, N_SUMS)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(s[:, :5].sum(axis=1) == 0, 0.0, 1.0 - s[:, 5] / s[:, 6])
    return np.where(s[:, 6] == 0, np.nan, f)


def _stat(values):
    v = np.asarray(values, dtype=np.float64)
    if v.size == 0:
        return {"mean": None, "std": None, "n": 0}
    return {"mean": float(v.mean()), "std": float(v.std()), "n": int(v.size)}


def figures(sums, counts, size, channels, show=16, info=None):
    """The figures of the module's docstring from sums (n, 7) fp64 and counts (n, 5): a dict of {"mean", "std", "n"} entries with
    the integer counts "n_pairs", "flat", "unchanged" and the list "most_ignored".  info: per pair a dict of what is known about it
    (image position, key, slot, rectangle, offset), copied into its most_ignored entry."""
    s = np.asarray(sums, dtype=np.float64).reshape(-1, N_SUMS)
    c = np.asarray(counts, dtype=np.int64).reshape(-1, N_CLASSES)
    n, S, C = s.shape[0], int(size), int(channels)
    if c.shape[0] != n or (info is not None and len(info) != n):
        raise ValueError("layoutshift: sums, counts and info must list the same pairs")
    if not np.isfinite(s).all() or (s < 0).any() or (c < 0).any():
        raise ValueError("layoutshift: a sum is negative or not finite")
    total = s[:, :5].sum(axis=1)
    unchanged, flat = total == 0, s[:, 6] == 0
    follow = follow_of(s)
    with np.errstate(divide="ignore", invalid="ignore"):
        locality = s[:, :3].sum(axis=1) / total
        change = s[:, :5] / (c[:, :5] * float(C))
        boxes_px = c[:, :3].sum(axis=1)
        box_mean = s[:, :3].sum(axis=1) / boxes_px
        spill = [(s[:, k] / c[:, k]) / box_mean for k in (3, 4)]
    out = {"n_pairs": int(n), "flat": int(flat.sum()), "unchanged": int(unchanged.sum()),
           "follow": _stat(follow[~flat]), "locality": _stat(locality[~unchanged]),
           "area_share": _stat(boxes_px / float(S * S)),
           "change": {CLASS_NAMES[k]: _stat(change[c[:, k] > 0, k]) for k in range(N_CLASSES)}}
    for name, k, v in (("spill_others", 3, spill[0]), ("spill_background", 4, spill[1])):
        out[name] = _stat(v[(c[:, k] > 0) & (boxes_px > 0) & (s[:, :3].sum(axis=1) > 0)])
    rows = [r for r in np.argsort(np.where(flat, np.inf, follow), kind="stable").tolist() if not flat[r]][:max(0, int(show))]
    out["most_ignored"] = [dict({} if info is None else info[r], pair=int(r), follow=float(follow[r])) for r in rows]
    return out


def _boxed(img, rect):
    """(S, S, 3) u8 of a (C, S, S) u8 image with the one-pixel white outline of the pixel rectangle"""
    t = np.repeat(img, 3, axis=0) if img.shape[0] == 1 else img[:3]
    t = np.ascontiguousarray(t.transpose(1, 2, 0)).copy()
    x0, y0, x1, y1 = rect
    t[y0, x0:x1] = t[y1 - 1, x0:x1] = 255
    t[y0:y1, x0] = t[y0:y1, x1 - 1] = 255
    return t


def layout_grid(save_dir, kept, info):
    """layout_grid.png: one row [A with the old box | B with the new box | |A - B|] per entry (follow, pair, A u8, B u8) of `kept`,
    lowest follow first; info[pair] holds the pair's rectangle and offset.  Returns the file's name."""
    from PIL import Image
    rows = []
    for _, pair, a, b in sorted(kept, key=lambda v: (v[0], v[1])):
        x0, y0, x1, y1 = info[pair]["rect"]
        dx, dy = info[pair]["offset"]
        diff = np.abs(a.astype(np.int16) - b.astype(np.int16)).astype(np.uint8)
        diff = np.repeat(diff, 3, axis=0) if diff.shape[0] == 1 else diff[:3]
        rows.append(np.concatenate([_boxed(a, (x0, y0, x1, y1)), _boxed(b, (x0 + dx, y0 + dy, x1 + dx, y1 + dy)),
                                    diff.transpose(1, 2, 0)], axis=1))
    Image.fromarray(np.concatenate(rows, axis=0)).save('%s/layout_grid.png' % save_dir)
    return "layout_grid.png"


class ShiftResponse:
    """The score over a stream of batches.  size, channels: the images'; rows: the images the pass will see at most; min_shift:
    pixels, None for size / 8; `sums(a, b, edit, others)` -> (sums, counts): hip/ops.box_shift_sums unless the caller hands another
    over (sums_numpy, for one).  Per batch: `edits(boxes, take)` makes the edit table of the `take` leading images of host fp32 boxes
    (B, G, 4) -- the images are counted from the accumulator's own position, nothing is recorded yet --; the caller generates the
    second batch under the moved boxes table["moved"]; `add(a, b, edit, others, take)` scores the table's pairs out of the two batches
    (B, C, S, S) on the device, keeps the (n, 7) fp64 sums and (n, 5) counts on the device and counts the images.  result() reads
    them back once.  keep > 0: after every batch its sums are read back as well, and the `keep` pairs of lowest follow so far stay
    on the host as u8 images (`kept`): what layout_grid.png is drawn from."""

    def __init__(self, size, channels, rows, min_shift=None, min_side=1, seed=100, device="cuda", sums=None, keep=0):
        import torch
        self.size, self.channels, self.rows = int(size), int(channels), int(rows)
        if self.size < 2 or self.size > 1024 or not 1 <= self.channels <= 4 or self.rows < 1:
            raise ValueError("layoutshift: size in 2..1024, channels in 1..4 and rows >= 1 expected, got %d, %d, %d"
                             % (self.size, self.channels, self.rows))
        self.min_shift = default_min_shift(self.size) if min_shift is None else int(min_shift)
        if self.min_shift < 1:
            raise ValueError("layoutshift: min_shift must be 1 pixel at least, got %d" % self.min_shift)
        self.min_side, self.seed, self.device, self.sums = float(min_side), int(seed), torch.device(device), sums
        if not 0 <= self.min_side < float("inf"):
            raise ValueError("layoutshift: min_side must be a finite number of pixels, 0 at least, got %r" % (min_side,))
        self.n_images = self.no_objects = self.immovable = 0
        self._sums, self._counts, self.info = [], [], []
        self.keep, self.kept = max(0, int(keep)), []               # (follow, pair, A u8, B u8) of the `keep` lowest so far

    @property
    def n(self):
        return len(self.info)

    def edits(self, boxes, take):
        """The edit table of a batch, a dict of host tensors: "row" (n,) int64, the images of the batch that have a pair; "slot" (n,)
        int64; "edit" (n, 6) int32; "others" (n, G - 1, 4) int32, absent ones (0, 0, 0, 0); "moved" (n, 4) fp32, the moved boxes;
        "boxes" (B, G, 4) fp32, the batch's boxes with the moved ones in their slots and every other value's bits kept; "no_objects" and
        "immovable", the images of the `take` left out."""
        import torch
        if not torch.is_tensor(boxes) or boxes.dim() != 3 or boxes.shape[2] != 4 or boxes.dtype != torch.float32 or boxes.is_cuda:
            raise ValueError("layoutshift: host fp32 boxes (B, G, 4) expected, got %s" % (tuple(getattr(boxes, "shape", ())) or type(boxes),))
        B, G = int(boxes.shape[0]), int(boxes.shape[1])
        take = max(0, min(int(take), B))
        if G - 1 > MAX_OTHERS:
            raise ValueError("layoutshift: %d boxes per image, %d at the most" % (G, MAX_OTHERS + 1))
        if self.n_images + take > self.rows:
            raise ValueError("layoutshift: %d more images do not fit an accumulator for %d of which %d are in"
                             % (take, self.rows, self.n_images))
        host = boxes.numpy()
        edited = boxes.clone()
        row, slot, edit, others, moved, left = [], [], [], [], [], {"no_objects": 0, "immovable": 0}
        for j in range(take):
            e = draw_edit(host[j], self.size, self.seed, self.n_images + j, self.min_shift, self.min_side)
            if isinstance(e, str):
                left[e] += 1
                continue
            row.append(j)
            slot.append(e["slot"])
            edit.append(list(e["rect"]) + list(e["offset"]))
            others.append([list(r) for r in e["others"]] + [[0, 0, 0, 0]] * (G - 1 - len(e["others"])))
            moved.append(e["box"])
            edited[j, e["slot"]] = torch.from_numpy(e["box"])
        n = len(row)
        return {"row": torch.tensor(row, dtype=torch.int64), "slot": torch.tensor(slot, dtype=torch.int64),
                "edit": torch.tensor(edit, dtype=torch.int32).reshape(n, 6),
                "others": torch.tensor(others, dtype=torch.int32).reshape(n, max(0, G - 1), 4),
                "moved": torch.from_numpy(np.asarray(moved, dtype=np.float32).reshape(n, 4)), "boxes": edited,
                "no_objects": left["no_objects"], "immovable": left["immovable"], "first": self.n_images, "take": take}

    def add(self, a, b, edit, others=None, take=None, keys=None):
        """Scores a batch: a, b (B, C, S, S) fp32 on the device, the batch under the data's layout and under `edit`, the table
        edits() made for it (`others` and `take` default to the table's); keys: the batch's dataset keys, for most_ignored.
        Returns (sums, counts) of the batch's pairs, on the device (None where the batch has none)."""
        import torch
        if edit["first"] != self.n_images:
            raise ValueError("layoutshift: the edit table was made at image %d, the accumulator stands at %d"
                             % (edit["first"], self.n_images))
        others = edit["others"] if others is None else others
        take = edit["take"] if take is None else int(take)
        if take != edit["take"]:
            raise ValueError("layoutshift: the edit table covers %d images, not %d" % (edit["take"], take))
        for name, t in (("a", a), ("b", b)):
            if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 4:
                raise ValueError("layoutshift: %s must be an fp32 (B, C, S, S) tensor, got %s %s"
                                 % (name, getattr(t, "dtype", type(t)), tuple(getattr(t, "shape", ()))))
            if tuple(t.shape[1:]) != (self.channels, self.size, self.size) or t.shape[0] < take or t.shape != a.shape:
                raise ValueError("layoutshift: %s must be (>= %d, %d, %d, %d), got %s"
                                 % (name, take, self.channels, self.size, self.size, tuple(t.shape)))
        if self.sums is None:
            from ..hip import ops
            self.sums = ops.box_shift_sums
        got = None
        rows = edit["row"]
        if len(rows):
            at = rows.to(a.device)
            got = self.sums(a.detach()[at].contiguous(), b.detach()[at].contiguous(), edit["edit"], others)
            self._sums.append(torch.as_tensor(got[0]))
            self._counts.append(torch.as_tensor(got[1]))
            for k, j in enumerate(rows.tolist()):
                e = [int(v) for v in edit["edit"][k]]
                self.info.append({"image": self.n_images + j, "key": None if keys is None else str(keys[j]),
                                  "slot": int(edit["slot"][k]), "rect": e[:4], "offset": e[4:]})
            if self.keep:
                self._keep(torch.as_tensor(got[0]).cpu().numpy(), a.detach()[at], b.detach()[at])
        self.n_images += take
        self.no_objects += edit["no_objects"]
        self.immovable += edit["immovable"]
        return got

    def _keep(self, s, a, b):
        first = self.n - s.shape[0]
        f = follow_of(s)
        new = [(float(f[k]), first + k, k) for k in range(s.shape[0]) if np.isfinite(f[k])]
        best = sorted([(v[0], v[1], None) for v in self.kept] + new)[:self.keep]
        old = {v[1]: v for v in self.kept}
        u8 = lambda t: t.float().add(1.0).mul(127.5).clamp(0, 255).byte().cpu().numpy()
        self.kept = [old[pair] if k is None else (fo, pair, u8(a[k]), u8(b[k])) for fo, pair, k in best]

    def raw(self):
        """(sums (n, 7) fp64, counts (n, 5) int64) of every pair so far, numpy: the one read-back"""
        import torch
        if not self._sums:
            return np.zeros((0, N_SUMS)), np.zeros((0, N_CLASSES), dtype=np.int64)
        both = torch.cat([torch.cat(self._sums).double(), torch.cat(self._counts).double()], dim=1).cpu().numpy()
        return both[:, :N_SUMS], both[:, N_SUMS:].astype(np.int64)             # counts <= 2^20 are exact in fp64

    def result(self, show=16):
        if self.n < 1:
            raise ValueError("layoutshift: no pair was added (%d images: %d without objects, %d immovable)"
                             % (self.n_images, self.no_objects, self.immovable))
        s, c = self.raw()
        out = figures(s, c, self.size, self.channels, show, self.info)
        out.update({"n_images": self.n_images, "no_objects": self.no_objects, "immovable": self.immovable,
                    "min_shift": self.min_shift, "min_side": self.min_side})
        return out
