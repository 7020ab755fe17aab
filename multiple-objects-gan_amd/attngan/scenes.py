"""Scene files: captions, boxes and labels a user wrote, checked and turned into what a layout-conditioned generator takes
(DESIGN.md section 9p).  Pure Python and numpy, no GPU, nothing of coco-attngan beyond the vocabulary and the limits it is handed.

A file is JSON: {"scenes": [scene, ...]},
    scene = {"name", "caption", "objects": [{"label", "box": [x, y, w, h]}, ...], "samples"?, "sweep"?: {"object", "to": [x, y], "steps"}}

  caption   lower-cased, its tokens are re's \\w+, each reduced to its ASCII characters; a token the vocabulary does not hold is dropped
            and listed; the rest is cut to `words_num` words, and the record says so.  No known word: an error.
  box       relative (x, y, w, h), w, h > 0, the rectangle inside [0, 1]^2; at most `max_objects` objects, absent slots are -1 as in
            the data
  label     an int in 0..n_classes - 2 (the one-hot's last index is the absent slot's), or, with a class-name list, a name of it
  name      usable as a directory name ([A-Za-z0-9._-], not starting with a dot), unique in the file
  samples   1..64 images of the scene under different noise (the file's default where absent)
  sweep     object `object` walks linearly from its own (x, y) to `to` in `steps` (2..32) steps, step 0 being its own position; the
            box must stay inside the image at `to`
Every violation is a ValueError that names the scene and the field."""
import json
import re

import numpy as np

MAX_OBJECTS = 3
SAMPLES_MAX, STEPS_MIN, STEPS_MAX = 64, 2, 32
_NAME = re.compile(r"^[A-Za-z0-9_-][A-Za-z0-9._-]*$")
_SCENE_KEYS = {"name", "caption", "objects", "samples", "sweep"}


class Scene(object):
    """a checked scene: name, tokens (word indices), words, dropped, truncated, boxes (max_objects, 4) float32 with -1 rows for absent
    slots, labels (max_objects,) int64 with -1, n_objects, samples, sweep (None or dict(object, to, steps)), index, seed"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def sweep_boxes(self):
        """(steps, 4) float32: the swept object's box at every step; step 0 is its own box, bit for bit"""
        s = self.sweep
        x, y, w, h = (float(v) for v in self.boxes[s["object"]])
        out = np.empty((s["steps"], 4), dtype=np.float32)
        for k in range(s["steps"]):
            f = k / float(s["steps"] - 1)
            out[k] = (x + (s["to"][0] - x) * f, y + (s["to"][1] - y) * f, w, h)
        out[0] = self.boxes[s["object"]]
        return out

    def drawn_boxes(self):
        """the boxes as they are drawn: the data's clamp (datasets.crop_imgs: x + w > 0.999 -> w = 1 - x - 0.001) keeps the far edge
        on the last pixel at most; the generator sees the boxes as written"""
        out = self.boxes.copy()
        for k in range(self.n_objects):
            out[k] = clamp_box(out[k])
        return out

    def pixel_boxes(self, size):
        """[[x, y, w, h], ...] of the present objects in pixels of a size x size image, by evaluate.draw_bbox_lines' rule"""
        return [[int(size * float(v)) for v in box] for box in self.drawn_boxes()[:self.n_objects]]


def clamp_box(box):
    x, y, w, h = (float(v) for v in box)
    if x + w > 0.999:
        w = 1.0 - x - 0.001
    if y + h > 0.999:
        h = 1.0 - y - 0.001
    return np.array([x, y, w, h], dtype=np.float32)


def scene_seed(seed, index):
    """the seed of scene `index`'s own device generator"""
    return int(np.random.SeedSequence([int(seed), int(index)]).generate_state(1)[0])


def tokenize(caption):
    """lower-cased \\w+ tokens, each reduced to its ASCII characters (empty ones dropped)"""
    out = []
    for tok in re.findall(r"\w+", caption.lower()):
        tok = tok.encode("ascii", "ignore").decode("ascii")
        if tok:
            out.append(tok)
    return out


def read_classes(path):
    """one class name per line -> list of names; blank lines are an error, so that a line number is a label"""
    with open(path) as f:
        names = [line.strip() for line in f.read().splitlines()]
    if not names or any(not n for n in names) or len(set(names)) != len(names):
        raise ValueError("class file %s: one non-empty, unique class name per line expected" % path)
    return names


def _fail(scene, field, what):
    raise ValueError("scene %s, %s: %s" % (scene, field, what))


def _number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool) and np.isfinite(v)


def _integer(v):
    return isinstance(v, int) and not isinstance(v, bool)


def _box(who, field, box):
    if not isinstance(box, (list, tuple)) or len(box) != 4 or not all(_number(v) for v in box):
        _fail(who, field, "four finite numbers (x, y, w, h) expected, got %r" % (box,))
    x, y, w, h = (float(v) for v in box)
    if not (w > 0 and h > 0):
        _fail(who, field, "w and h must be positive, got %r" % (box,))
    if not (x >= 0 and y >= 0 and x + w <= 1 and y + h <= 1):
        _fail(who, field, "the rectangle must lie inside [0, 1]^2, got %r" % (box,))
    return x, y, w, h


def check_scene(raw, index, wordtoix, words_num, n_classes, samples=4, classes=None, seed=100, max_objects=MAX_OBJECTS):
    """one entry of the file's list -> Scene"""
    who = "#%d" % index
    if not isinstance(raw, dict):
        _fail(who, "scene", "an object expected, got %s" % type(raw).__name__)
    name = raw.get("name")
    if not isinstance(name, str) or not _NAME.match(name) or len(name) > 100:
        _fail(who, "name", "a directory name of [A-Za-z0-9._-] that does not start with a dot expected, got %r" % (name,))
    who = "%r" % name
    unknown = sorted(set(raw) - _SCENE_KEYS)
    if unknown:
        _fail(who, unknown[0], "unknown field")
    caption = raw.get("caption")
    if not isinstance(caption, str):
        _fail(who, "caption", "a string expected, got %r" % (caption,))
    words, dropped = [], []
    for tok in tokenize(caption):
        (words if tok in wordtoix and int(wordtoix[tok]) != 0 else dropped).append(tok)
    if not words:
        _fail(who, "caption", "no word of %r is in the vocabulary" % caption)
    truncated = len(words) > int(words_num)
    words = words[:int(words_num)]
    objects = raw.get("objects")
    if not isinstance(objects, list) or not 1 <= len(objects) <= max_objects:
        _fail(who, "objects", "a list of 1..%d objects expected" % max_objects)
    boxes = np.full((max_objects, 4), -1.0, dtype=np.float32)
    labels = np.full((max_objects,), -1, dtype=np.int64)
    written = []                                                     # as Python floats: the sweep's end is checked as the boxes are
    for k, obj in enumerate(objects):
        if not isinstance(obj, dict) or set(obj) != {"label", "box"}:
            _fail(who, "objects[%d]" % k, "an object with exactly the fields label and box expected")
        written.append(_box(who, "objects[%d].box" % k, obj["box"]))
        boxes[k] = written[k]
        label = obj["label"]
        if isinstance(label, str):
            if classes is None:
                _fail(who, "objects[%d].label" % k, "the name %r needs a class-name file" % label)
            if label not in classes:
                _fail(who, "objects[%d].label" % k, "%r is not a name of the class file" % label)
            label = classes.index(label)
        if not _integer(label) or not 0 <= label <= int(n_classes) - 2:
            _fail(who, "objects[%d].label" % k, "an int in 0..%d expected, got %r" % (int(n_classes) - 2, obj["label"]))
        labels[k] = label
    n = raw.get("samples", samples)
    if not _integer(n) or not 1 <= n <= SAMPLES_MAX:
        _fail(who, "samples", "an int in 1..%d expected, got %r" % (SAMPLES_MAX, n))
    sweep = raw.get("sweep")
    if sweep is not None:
        if not isinstance(sweep, dict) or set(sweep) != {"object", "to", "steps"}:
            _fail(who, "sweep", "an object with exactly the fields object, to and steps expected")
        if not _integer(sweep["object"]) or not 0 <= sweep["object"] < len(objects):
            _fail(who, "sweep.object", "an index into the scene's %d objects expected, got %r" % (len(objects), sweep["object"]))
        if not _integer(sweep["steps"]) or not STEPS_MIN <= sweep["steps"] <= STEPS_MAX:
            _fail(who, "sweep.steps", "an int in %d..%d expected, got %r" % (STEPS_MIN, STEPS_MAX, sweep["steps"]))
        to = sweep["to"]
        if not isinstance(to, (list, tuple)) or len(to) != 2 or not all(_number(v) for v in to):
            _fail(who, "sweep.to", "two finite numbers (x, y) expected, got %r" % (to,))
        w, h = written[sweep["object"]][2:]
        if not (to[0] >= 0 and to[1] >= 0 and to[0] + w <= 1 and to[1] + h <= 1):
            _fail(who, "sweep.to", "the swept box (w %g, h %g) must stay inside the image at %r" % (w, h, to))
        sweep = {"object": int(sweep["object"]), "to": [float(to[0]), float(to[1])], "steps": int(sweep["steps"])}
    return Scene(name=name, caption=caption, words=words, tokens=[int(wordtoix[w]) for w in words], dropped=dropped, truncated=truncated,
                 boxes=boxes, labels=labels, n_objects=len(objects), samples=int(n), sweep=sweep, index=index,
                 seed=scene_seed(seed, index))


def check_file(doc, wordtoix, words_num, n_classes, samples=4, classes=None, seed=100, max_objects=MAX_OBJECTS):
    """the parsed JSON document -> [Scene, ...] in the file's order"""
    if not isinstance(doc, dict) or set(doc) != {"scenes"} or not isinstance(doc["scenes"], list) or not doc["scenes"]:
        raise ValueError('scene file: {"scenes": [ ... ]} with one scene at least expected')
    if not _integer(samples) or not 1 <= samples <= SAMPLES_MAX:
        raise ValueError("scene file: the default for samples must be an int in 1..%d, got %r" % (SAMPLES_MAX, samples))
    out, seen = [], set()
    for index, raw in enumerate(doc["scenes"]):
        scene = check_scene(raw, index, wordtoix, words_num, n_classes, samples, classes, seed, max_objects)
        if scene.name in seen:
            _fail("%r" % scene.name, "name", "used twice in the file")
        seen.add(scene.name)
        out.append(scene)
    return out


def load(path, wordtoix, words_num, n_classes, samples=4, classes=None, seed=100, max_objects=MAX_OBJECTS):
    with open(path) as f:
        try:
            doc = json.load(f)
        except ValueError as e:
            raise ValueError("scene file %s is not JSON: %s" % (path, e))
    return check_file(doc, wordtoix, words_num, n_classes, samples, classes, seed, max_objects)


def vocabulary(dataset):
    """word -> index of a dataset: its `wordtoix` where it has one, else its `ixtoword` inverted (the synthetic set's w1, w2, ...)"""
    w = getattr(dataset, "wordtoix", None)
    if w is None:
        w = {word: ix for ix, word in dataset.ixtoword.items()}
    return w
