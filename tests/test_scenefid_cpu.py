"""The host side of the object-level Frechet distance (attngan/scenefid.py) without a GPU: boxes_from_theta against the boxes that
made the matrices, object_list's order, `take` and `min_side`, the accumulator's splitting of an object list across its staging
batches (the crop and the encoder are stand-ins on the CPU: ObjectCodes needs the device for nothing else), and main.py's
arguments."""
import numpy as np
import pytest
import torch

import scenefid_cases as S
from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import scenefid as SF, synthetic  # noqa: E402
from mogan_amd.attngan.miscc.utils import compute_transformation_matrix  # noqa: E402


def _theta(boxes):
    """(B, G, 4) boxes -> (B, G, 2, 3), as the data set makes them"""
    B, G = boxes.shape[:2]
    return compute_transformation_matrix(torch.from_numpy(boxes).view(-1, 4)).view(B, G, 2, 3)


def test_boxes_from_theta_gives_the_boxes_back():
    boxes, _ = synthetic.make_bboxes(np.random.RandomState(11), 440)               # 2 or 3 of 3 slots present per image
    assert boxes.shape == (440, 3, 4) and (boxes[:, :, 2] < 0).any()
    got = SF.boxes_from_theta(_theta(boxes)).numpy()
    assert got.dtype == np.float32 and got.shape == boxes.shape
    present = boxes[:, :, 2] > 0
    assert int(present.sum()) >= 1000
    err = float(np.abs(got[present].astype(np.float64) - boxes[present]).max())
    print("boxes_from_theta: %.3e off the boxes (bound %.3e)" % (err, 4 * S.EPS))
    assert err <= 4 * S.EPS
    assert np.array_equal(got[:, :, 2:], boxes[:, :, 2:])                           # w and h are the matrix's own entries
    assert (got[~present][:, 2] < 0).all() and (got[~present][:, 3] < 0).all()
    for bad in (torch.zeros(3, 2, 3), torch.zeros(2, 3, 3, 2), np.zeros((2, 3, 2, 3))):
        with pytest.raises(ValueError):
            SF.boxes_from_theta(bad)


def test_object_list_order_take_and_min_side():
    A = S.ABSENT
    boxes = torch.tensor([[(0.1, 0.1, 0.5, 0.5), A, (0.2, 0.2, 0.25, 0.125)],
                          [A, A, A],
                          [(0.3, 0.3, 0.01, 0.5), (0.0, 0.0, 1.0, 1.0), (0.5, 0.5, 0.0, 0.5)],
                          [(0.4, 0.4, 0.5, 0.003), A, (0.6, 0.6, 0.25, 0.25)]], dtype=torch.float32)
    index, kept = SF.object_list(boxes, 4, 256)
    assert index.dtype == torch.int32 and kept.dtype == torch.float32 and kept.is_contiguous()
    assert index.tolist() == [0, 0, 2, 2, 3]                                       # image order, then slot order; w = 0 is absent
    assert torch.equal(kept, torch.stack([boxes[0, 0], boxes[0, 2], boxes[2, 0], boxes[2, 1], boxes[3, 2]]))
    index, kept = SF.object_list(boxes, 3, 256)                                    # the leading images only
    assert index.tolist() == [0, 0, 2, 2]
    index, kept = SF.object_list(boxes, 4, 256, min_side=3)                        # 0.01 * 256 = 2.56 pixels: out
    assert index.tolist() == [0, 0, 2, 3] and torch.equal(kept[2], boxes[2, 1])
    index, kept = SF.object_list(boxes, 4, 256, min_side=32)                       # min(w, h) * 256 = 32 stays
    assert index.tolist() == [0, 0, 2, 3] and torch.equal(kept[1], boxes[0, 2])
    index, kept = SF.object_list(boxes, 4, 256, min_side=33)
    assert index.tolist() == [0, 2, 3]
    index, kept = SF.object_list(boxes, 4, 256, min_side=0)                        # the 0.768-pixel box counts, w = 0 never does
    assert index.tolist() == [0, 0, 2, 2, 3, 3]
    index, kept = SF.object_list(boxes, 0, 256)
    assert tuple(index.shape) == (0,) and tuple(kept.shape) == (0, 4)
    for bad in (boxes.double(), boxes[0], boxes.numpy(), boxes[:, :, :3]):
        with pytest.raises(ValueError):
            SF.object_list(bad, 4, 256)


class _Encoder(torch.nn.Module):
    """a stand-in for CNN_ENCODER: the `code` of a crop is its first D values; it records the batch shapes it is run at"""
    D = 5

    def __init__(self):
        super().__init__()
        self.emb_cnn_code = torch.nn.Linear(self.D, 2)
        self.seen = []

    def pool_code(self, x):
        self.seen.append(tuple(x.shape))
        return x.flatten(1)[:, :self.D].clone()


def _mark(x, boxes, index, OH, OW, out=None):
    """a stand-in for ops.roi_resize: the crop of object (image i, box b) is filled with x[i, 0, 0, 0] + b.x"""
    assert out is not None and tuple(out.shape) == (len(index), 3, OH, OW) and out.is_contiguous()
    assert index.dtype == torch.int32 and boxes.dtype == torch.float32 and tuple(boxes.shape) == (len(index), 4)
    for r in range(len(index)):
        out[r] = x[int(index[r]), 0, 0, 0] + boxes[r, 0]
    return out


def test_the_accumulator_splits_an_object_list_across_staging_batches():
    rng = np.random.RandomState(4)
    boxes, _ = synthetic.make_bboxes(rng, 10)
    boxes = boxes.reshape(5, 2, 3, 4)                                              # five batches of two images
    enc = _Encoder()
    acc = SF.ObjectCodes(rows=9, chunk=4, size=256, device="cpu", resize=_mark)    # the pass stops after nine images
    assert all(tuple(t.shape) == (4, 3, 299, 299) and not t.any() for t in acc.stage.values())
    want_real, want_fake, want_image, want_box = [], [], [], []
    for b in range(5):
        real = torch.full((2, 3, 256, 256), 10.0 * b) + torch.arange(2.0).view(2, 1, 1, 1)
        fake = -real
        take = 2 if b < 4 else 1
        acc.sink(real, fake, _theta(boxes[b]), take, enc)
        for i in range(take):
            for g in range(3):
                if boxes[b, i, g, 2] > 0:
                    x = SF.boxes_from_theta(_theta(boxes[b]))[i, g, 0]
                    want_real.append(float(real[i, 0, 0, 0] + x))
                    want_fake.append(float(fake[i, 0, 0, 0] + x))
                    want_image.append(2 * b + i)
                    want_box.append(boxes[b, i, g])
    n = len(want_real)
    assert n > 16 and n % 4                                                        # several batches, and a partly filled last one
    full = n // 4
    assert acc.n == 4 * full and acc.fill == n % 4 and acc.n_images == 9 and len(enc.seen) == 2 * full
    real, fake = acc.finish()
    assert acc.n == n and acc.fill == 0 and len(enc.seen) == 2 * (full + 1)
    assert set(enc.seen) == {(4, 3, 299, 299)}                                     # the trunk sees one batch shape for the whole pass
    assert not acc.stage["real"][n % 4:].any() and not acc.stage["fake"][n % 4:].any()     # the last batch's unused rows are zero
    assert tuple(real.shape) == (n, _Encoder.D) == tuple(fake.shape)
    assert torch.equal(real, torch.tensor(want_real).view(n, 1).expand(n, _Encoder.D))
    assert torch.equal(fake, torch.tensor(want_fake).view(n, 1).expand(n, _Encoder.D))
    image, box = acc.objects()
    assert image.tolist() == want_image and image.dtype == torch.int64
    assert float((box - torch.from_numpy(np.stack(want_box))).abs().max()) <= 4 * S.EPS
    assert acc.finish()[0].data_ptr() == real.data_ptr() and len(enc.seen) == 2 * (full + 1)    # nothing left to run
    with pytest.raises(ValueError, match="do not fit"):
        acc.sink(torch.zeros(2, 3, 256, 256), torch.zeros(2, 3, 256, 256), _theta(boxes[0]), 1, enc)


def test_main_takes_scene_fid_alone_and_in_the_group_and_not_with_sampling():
    from mogan_amd.attngan import main as entry
    args = entry.parse_args(["--scene_fid"])
    assert args.scene_fid and args.scene_fid_min_side == 1 and not args.fid
    args = entry.parse_args(["--scene_fid", "--scene_fid_min_side", "8", "--fid", "--kid", "--prdc", "--swd", "--msssim"])
    assert args.scene_fid and args.scene_fid_min_side == 8 and args.fid and args.kid and args.prdc and args.swd and args.msssim
    assert not entry.parse_args([]).scene_fid
    for other in ("--sampling", "--r_precision"):
        with pytest.raises(SystemExit):
            entry.parse_args(["--scene_fid", other])


def test_pool_codes_wants_the_trunk_for_an_object_sink():
    from mogan_amd.attngan.evaluate import CheckpointEvaluation
    with pytest.raises(ValueError, match="object_sink"):
        CheckpointEvaluation().pool_codes("test", object_sink=lambda *a: None, trunk=False)
