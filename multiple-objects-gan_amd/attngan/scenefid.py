"""Host side of the object-level Frechet distance (Sylvain et al., "Object-centric image generation from layouts", 2021, call it
SceneFID; the reference repository has no code for it).  Every score of sections 9c-9h looks at the whole
image; this one looks at the OBJECTS: whether the generator put something plausible at the box it was given.  A checkpoint whose
object pathway has died keeps its FID while the global pathway paints a believable scene, and loses this figure.

The definition, in this project's words:

  Objects.     The generator is conditioned on up to three labelled boxes per caption, relative (x, y, w, h), the data set's
               convention; an absent object is (-1, -1, -1, -1).  The boxes are the DATA's on both sides: the real image and the
               image generated for the same caption, boxes and labels are cut at the same ground-truth boxes.  An object counts
               when w > 0, h > 0 and min(w, h) * size >= min_side pixels (size = 256, the tree's final resolution; min_side = 1 by
               default).  The pass has the boxes as the matrices `tm` of compute_transformation_matrix,
               [[w, 0, 2 (x + w / 2) - 1], [0, h, 2 (y + h / 2) - 1]]; boxes_from_theta inverts them in fp32: w = t00, h = t11,
               x = (t02 + 1) / 2 - w / 2, y = (t12 + 1) / 2 - h / 2 (within 4 * 2^-24 of the data set's box; w and h exactly).
  Order.       The objects of a pass are listed in image order, then slot order (object_list); row k of the real codes and row k
               of the generated codes are the same object.
  Crop.        Every object is cut out and resized to the trunk's 299 x 299 input in one step, hip/ops.roi_resize: per axis, in
               fp32 with one rounding per operation,
                   p0 = x * W          pl = w * W          scale = pl / 299
                   src(j) = p0 + ((j + 0.5) * scale - 0.5)      clamped to [0, W - 1]
                   i0 = floor(src)     i1 = min(i0 + 1, W - 1)  l = src - i0
               and the value is the bilinear blend of the four taps -- the pixel rule of bilinear_resize, the trunk's own first step
               (the full box (0, 0, 1, 1) is that resize), with the edge pixel repeated where a tap falls outside: a box at the
               image's edge keeps its brightness, nothing is padded with zeros.
  Codes.       The crops go through CNN_ENCODER.pool_code of TRAIN.NET_E's image encoder, the pooled 2048 vector the Frechet
               distance of section 9d is defined on.
  Score.       fid.frechet_distance of the fp64 mean and covariance (hip/ops.feature_moments) of the real objects' codes and of
               the generated objects' codes.  As with section 9d it is SceneFID in torchvision's Inception-v3 if the trunk holds
               ImageNet weights and a distance in random convolutional features otherwise; with fewer objects than features the
               covariances are rank-deficient and the figure is only comparable at equal n.

`boxes_from_theta` and `object_list` need no GPU.  `ObjectCodes` is the accumulator a pass over the data loader fills
(CheckpointEvaluation.pool_codes' object_sink); of it only the crop (`resize`, hip/ops.roi_resize unless the caller hands another
over) and the encoder need the device.
"""
import torch

TRUNK_SIZE = 299           # the Inception trunk's input side
MAX_OBJECTS = 3            # boxes per caption


def boxes_from_theta(tm):
    """(B, G, 2, 3) matrices of compute_transformation_matrix -> (B, G, 4) fp32 boxes (x, y, w, h) on tm's device: w = t00, h = t11,
    x = (t02 + 1) / 2 - w / 2, y likewise.  An absent object (w = -1) comes back with w < 0."""
    if not torch.is_tensor(tm) or tm.dim() != 4 or tuple(tm.shape[2:]) != (2, 3):
        raise ValueError("boxes_from_theta: matrices (B, G, 2, 3) expected, got %s" % (tuple(getattr(tm, "shape", ())) or type(tm),))
    tm = tm.detach().float()
    w, h = tm[:, :, 0, 0], tm[:, :, 1, 1]
    x = (tm[:, :, 0, 2] + 1.0) / 2.0 - w / 2.0
    y = (tm[:, :, 1, 2] + 1.0) / 2.0 - h / 2.0
    return torch.stack([x, y, w, h], dim=2)


def object_list(boxes, take, size, min_side=1):
    """The objects of the `take` leading images of host boxes (B, G, 4), in image order then slot order: every box with w > 0,
    h > 0 and min(w, h) * size >= min_side pixels.  Returns (image_index (R,) int32, boxes (R, 4) fp32), host tensors."""
    if not torch.is_tensor(boxes) or boxes.dim() != 3 or boxes.shape[2] != 4 or boxes.dtype != torch.float32 or boxes.is_cuda:
        raise ValueError("object_list: host fp32 boxes (B, G, 4) expected, got %s" % (tuple(getattr(boxes, "shape", ())) or type(boxes),))
    b = boxes[:max(0, int(take))]
    w, h = b[:, :, 2], b[:, :, 3]
    keep = (w > 0) & (h > 0) & (torch.minimum(w, h) * float(size) >= float(min_side))
    where = keep.nonzero()                                     # row-major: image, then slot
    return where[:, 0].to(torch.int32).contiguous(), b[keep].contiguous()


class ObjectCodes:
    """The pool codes of the objects of a stream of batches, real and generated.  rows: the images the pass will see at most;
    chunk: the loader's batch size, the ONE batch shape the frozen trunk sees; size: the images' side; `sink(real, fake, tm, take,
    image_encoder)` is pool_codes' object_sink: it reads back `tm` (tiny, and the price of knowing how many objects there are),
    lists the batch's objects, has `resize` write the real and the generated crops into two zero-initialised staging batches
    (chunk, 3, 299, 299) -- splitting the list where a batch fills -- and runs image_encoder.pool_code on a staging batch only when
    it is full; the codes go to two device buffers (rows * max_objects, D), allocated at the first batch.  `finish()` runs the partly
    filled last batch whole, its unused rows zeroed, and keeps its leading rows.  `n` objects and `n_images` images are in;
    `image` and `box` list the objects in global image order (host)."""

    def __init__(self, rows, chunk, size, min_side=1, seed=100, device="cuda", max_objects=MAX_OBJECTS, resize=None):
        self.rows, self.chunk, self.size, self.max_objects = int(rows), int(chunk), int(size), int(max_objects)
        if self.rows < 1 or self.chunk < 1 or self.size < 1 or self.max_objects < 1:
            raise ValueError("scenefid: rows, chunk, size and max_objects >= 1 expected, got %d, %d, %d, %d"
                             % (self.rows, self.chunk, self.size, self.max_objects))
        self.min_side, self.seed, self.device = float(min_side), int(seed), torch.device(device)
        self.params = {"seed": self.seed, "min_side": self.min_side}      # what it was made under: the hand-over check compares it
        self.resize = resize
        self.stage = {k: torch.zeros((self.chunk, 3, TRUNK_SIZE, TRUNK_SIZE), dtype=torch.float32, device=self.device)
                      for k in ("real", "fake")}
        self.codes = None                                      # {"real", "fake"}: (rows * max_objects, D), at the first batch
        self.fill = self.n = self.n_images = 0                 # staged objects; objects with codes; images seen
        self.encoder = None
        self.image, self.box = [], []

    def _resize(self, x, boxes, index, out):
        if self.resize is None:
            from ..hip import ops
            self.resize = ops.roi_resize
        self.resize(x, boxes, index, TRUNK_SIZE, TRUNK_SIZE, out=out)

    def _flush(self):
        """the staged objects' codes: the trunk on both staging batches at the full chunk size, the leading `fill` rows kept"""
        for k in ("real", "fake"):
            self.codes[k][self.n:self.n + self.fill] = self.encoder.pool_code(self.stage[k])[:self.fill]
        self.n += self.fill
        self.fill = 0

    def sink(self, real, fake, tm, take, image_encoder):
        if self.n_images + int(take) > self.rows:
            raise ValueError("scenefid: %d more images do not fit an accumulator for %d of which %d are in"
                             % (take, self.rows, self.n_images))
        if tm.shape[1] > self.max_objects:
            raise ValueError("scenefid: %d boxes per image, the accumulator has room for %d" % (tm.shape[1], self.max_objects))
        self.encoder = image_encoder
        if self.codes is None:
            D = int(image_encoder.emb_cnn_code.weight.shape[1])             # 2048: the pooled code's width
            self.codes = {k: torch.empty((self.rows * self.max_objects, D), dtype=torch.float32, device=self.device)
                          for k in ("real", "fake")}
        index, boxes = object_list(boxes_from_theta(tm.cpu()), take, self.size, self.min_side)    # the one read-back per batch
        self.image.append(index.to(torch.int64) + self.n_images)
        self.box.append(boxes)
        self.n_images += int(take)
        real, fake = real.detach().float().contiguous(), fake.detach().float().contiguous()
        pos, R = 0, int(index.shape[0])
        while pos < R:
            k = min(self.chunk - self.fill, R - pos)
            for name, x in (("real", real), ("fake", fake)):
                self._resize(x, boxes[pos:pos + k], index[pos:pos + k], self.stage[name][self.fill:self.fill + k])
            self.fill += k
            pos += k
            if self.fill == self.chunk:
                self._flush()

    def finish(self):
        """the codes of what is still staged (the last batch is run whole, rows past the staged objects zeroed); then
        (real codes, fake codes), the `n` filled rows of the device buffers"""
        if self.fill:
            for k in ("real", "fake"):
                self.stage[k][self.fill:].zero_()
            self._flush()
        if self.codes is None:
            return None, None
        return self.codes["real"][:self.n], self.codes["fake"][:self.n]

    def objects(self):
        """(image (n,) int64 in global image order, box (n, 4) fp32): the objects in the order of the codes' rows (host)"""
        if not self.image:
            return torch.zeros((0,), dtype=torch.int64), torch.zeros((0, 4), dtype=torch.float32)
        return torch.cat(self.image), torch.cat(self.box)
