"""Host side of object accuracy by nearest labelled training crops (the reference repository has no code for
it): does the object at the box have the identity that was asked for?  That is the question of the paper's Multi-MNIST and CLEVR
experiments, and the one score the StackGAN-family trees (multi-mnist, clevr, coco stage I / II) can have without a trunk, a
detector or any weights: the judge is the training set itself.

The definition, in this project's words:

  Objects.   A slot of an image's layout is an object when w > 0, h > 0 and min(w, h) * size >= min_side pixels (size: the tree's
             resolution, 64 or 256; min_side = 1 by default).  The boxes are the DATA's, read from the batch's matrices `tm` by
             attngan/scenefid.boxes_from_theta; the objects of a pass are listed in image order, then slot order
             (attngan/scenefid.object_list).
  Class.     From the slot's row of label_one_hot (classes_of):
                 mnist   argmax of 10
                 clevr   argmax(label[:4]) * 9 + argmax(label[4:]), 36 classes, as sampling.sample_clevr reads shape and colour
                 coco    argmax of 81; class 80 is "no label": the slot is left out and counted as `unlabelled`
  Crop.      hip/ops.roi_resize of the box to side x side (16 by default) over all C channels, flattened to a row of D = C side^2.
  Bank.      The crops and classes of the TRAIN split's real images, in dataset order, the first bank_size images.
  Queries.   Two sets against the same bank: the GENERATED images' crops, at the data's boxes of the evaluation split and with the
             classes the generator was given, and the evaluation split's REAL crops at the same boxes -- the data's own ceiling:
             what a nearest-crop judge gives unseen real objects.
  Distances. Squared Euclidean distances of rows, hip/ops.knn_label: per query the K nearest bank rows (K = 5 by default) under the
             order `before` (distance, equal bits by position), and the first bank row under that order of the query's OWN class
             (`same`) and of ANY OTHER class (`other`); an empty set is (+inf, NO_ROW = 2^31 - 1).
  Vote.      Among a query's K listed neighbours the class with most members wins; on a tie the class whose first member comes
             earliest in the list.

The figures, each an integer count with its ratio, for one set of queries (figures):

  accuracy            the vote equals the asked class
  accuracy_1nn        before(same, other): the nearest bank row is of the asked class (the K = 1 vote, from the label lists)
  accuracy_per_class  the mean of the per-class accuracies over the classes that have a query, plus the table class -> (right, n)
  accuracy_per_image  the mean over the images that have an object of the share of the image's objects that are right
  margin              the mean over queries of (sqrt d_other - sqrt d_same) / (sqrt d_other + sqrt d_same), in [-1, 1]: +1 the
                      object sits on a training crop of its class, -1 on one of another class, 0 half way.  A query where either
                      distance is infinite (its class, or every other class, is not in the bank), or both are 0, has no margin:
                      it is left out and counted (margin_left_out).

`most_wrong` lists the `show` queries with the smallest margin, ties by row; for that ranking a query without a margin takes the
limit: -1 where d_same is infinite and d_other is not, +1 where only d_other is infinite, 0 otherwise.

Every figure depends on `side`, K and the bank: a larger bank lies closer to everything.  Comparable at equal settings only.
Pure numpy; nothing here needs a GPU.
"""
import numpy as np

NO_ROW = 2147483647        # the position of an empty set, as mogan_knn_label_f64 writes it
CLASSES = {"mnist": 10, "clevr": 36, "coco": 80}
COCO_NO_LABEL = 80


def classes_of(tree, label_one_hot):
    """(..., L) one-hot rows -> (...) int64 classes by the tree's rule; a coco row whose argmax is 80 gives -1 (unlabelled)"""
    lab = np.asarray(label_one_hot)
    want = {"mnist": 10, "clevr": 13, "coco": 81}
    if tree not in want:
        raise ValueError("classes_of: tree must be one of mnist, clevr, coco, got %r" % (tree,))
    if lab.ndim < 1 or lab.shape[-1] != want[tree]:
        raise ValueError("classes_of: %s labels have %d entries, got shape %s" % (tree, want[tree], lab.shape))
    if tree == "clevr":
        return lab[..., :4].argmax(-1).astype(np.int64) * 9 + lab[..., 4:].argmax(-1).astype(np.int64)
    cls = lab.argmax(-1).astype(np.int64)
    if tree == "coco":
        cls[cls == COCO_NO_LABEL] = -1
    return cls


def before(v, i, w, j):
    """(v, i) comes before (w, j): by distance, equal distances by position -- the device's order, elementwise"""
    v, i, w, j = np.asarray(v, np.float64), np.asarray(i, np.int64), np.asarray(w, np.float64), np.asarray(j, np.int64)
    return (v < w) | ((v == w) & (i < j))


def vote(neighbour_classes):
    """(M, K) classes of every query's listed neighbours, nearest first -> (M,) int64 the winning class: most members, on a tie the
    class whose first member comes earliest.  A negative entry is an empty slot and votes for nothing; a query whose slots are all
    empty gets -1."""
    nc = np.asarray(neighbour_classes)
    if nc.ndim != 2 or nc.shape[1] < 1 or not np.issubdtype(nc.dtype, np.integer):
        raise ValueError("vote: integer classes (M, K) expected, got %s %s" % (nc.dtype, nc.shape))
    out = np.full((nc.shape[0],), -1, dtype=np.int64)
    for r, row in enumerate(nc):
        best, count = -1, 0
        for c in row:                                          # in list order: a later class must have MORE members to win
            if c >= 0:
                n = int((row == c).sum())
                if n > count:
                    best, count = int(c), n
        out[r] = best
    return out


def margins(same_d2, other_d2):
    """(margin (M,) fp64 with NaN where a query has none, has (M,) bool)"""
    s, o = np.asarray(same_d2, np.float64), np.asarray(other_d2, np.float64)
    if s.shape != o.shape or s.ndim != 1:
        raise ValueError("margins: two vectors of one length expected, got %s and %s" % (s.shape, o.shape))
    if np.isnan(s).any() or np.isnan(o).any() or (s < 0).any() or (o < 0).any():
        raise ValueError("margins: NaN or negative distances")
    has = np.isfinite(s) & np.isfinite(o) & ~((s == 0) & (o == 0))
    rs, ro = np.sqrt(np.where(has, s, 1.0)), np.sqrt(np.where(has, o, 1.0))
    return np.where(has, (ro - rs) / np.where(has, ro + rs, 1.0), np.nan), has


def _ranking_margin(same_d2, other_d2):
    m, has = margins(same_d2, other_d2)
    s, o = np.asarray(same_d2, np.float64), np.asarray(other_d2, np.float64)
    limit = np.where(np.isinf(s) & ~np.isinf(o), -1.0, np.where(np.isinf(o) & ~np.isinf(s), 1.0, 0.0))
    return np.where(has, m, limit)


def _checked(asked, neighbour_classes, same_d2, same_idx, other_d2, other_idx, image):
    asked, image = np.asarray(asked), np.asarray(image)
    n = asked.shape[0] if asked.ndim == 1 else -1
    if n < 1 or not np.issubdtype(asked.dtype, np.integer) or (asked < 0).any():
        raise ValueError("objaccuracy: a non-empty vector of classes >= 0 expected, got %s %s" % (asked.dtype, asked.shape))
    if image.shape != (n,) or not np.issubdtype(image.dtype, np.integer):
        raise ValueError("objaccuracy: one image index per query expected, got %s %s" % (image.dtype, image.shape))
    for name, a in (("same_d2", same_d2), ("same_idx", same_idx), ("other_d2", other_d2), ("other_idx", other_idx)):
        if np.asarray(a).shape != (n,):
            raise ValueError("objaccuracy: %s must have shape (%d,), got %s" % (name, n, np.asarray(a).shape))
    if np.asarray(neighbour_classes).shape[:1] != (n,):
        raise ValueError("objaccuracy: one row of neighbour classes per query expected")
    return asked.astype(np.int64), image.astype(np.int64)


def right(asked, neighbour_classes):
    """(M,) bool: the vote equals the asked class"""
    return vote(neighbour_classes) == np.asarray(asked, np.int64)


def figures(asked, neighbour_classes, same_d2, same_idx, other_d2, other_idx, image):
    """The figures of one set of queries (module docstring).  asked (M,) the queries' classes; neighbour_classes (M, K) the classes
    of the K listed bank rows (-1 for an empty slot); same_* / other_* (M,) the label lists; image (M,) the image each query is an
    object of."""
    asked, image = _checked(asked, neighbour_classes, same_d2, same_idx, other_d2, other_idx, image)
    n = int(asked.size)
    ok = right(asked, neighbour_classes)
    one = before(same_d2, same_idx, other_d2, other_idx)
    table = {}
    for c in np.unique(asked):
        of = asked == c
        table[int(c)] = [int(ok[of].sum()), int(of.sum())]
    per_class = float(np.mean([r / m for r, m in table.values()]))
    shares = [float(ok[image == i].mean()) for i in np.unique(image)]
    m, has = margins(same_d2, other_d2)
    return {"n": n, "right": int(ok.sum()), "accuracy": int(ok.sum()) / n,
            "right_1nn": int(one.sum()), "accuracy_1nn": int(one.sum()) / n,
            "classes": len(table), "accuracy_per_class": per_class, "per_class": {str(c): v for c, v in sorted(table.items())},
            "images": len(shares), "accuracy_per_image": float(np.mean(shares)),
            "margin_n": int(has.sum()), "margin_left_out": n - int(has.sum()),
            "margin": float(m[has].mean()) if has.any() else None}


def most_wrong(same_d2, other_d2, show):
    """(rows (m,) int64, margin (m,) fp64), m = min(show, M): the queries with the smallest margin, ascending, ties by row; a
    query without a margin is ranked at its limit (module docstring) and reported with NaN"""
    show = int(show)
    if show < 0:
        raise ValueError("most_wrong: show >= 0 expected, got %d" % show)
    key = _ranking_margin(same_d2, other_d2)
    rows = np.argsort(key, kind="stable")[:show].astype(np.int64)
    return rows, margins(same_d2, other_d2)[0][rows]
