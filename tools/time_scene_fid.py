"""The object crop of the object-level Frechet distance (attngan/scenefid.py; csrc/mogan_roi.hip) at the real workload -- ops.roi_resize
for 48 objects of 16 images of 3 x 256 x 256 to 299 x 299, host-side checks and the upload of boxes and index included -- against the
stock route of the same process: ops.stn_shared for all 16 x 3 slots (zero padding, absent objects as images of their own) plus
index_select of the present rows.  Hip events around every call, 8 warm-up calls and the median of 30 per path, the two paths
alternating call by call in one process.  A record, not a gate: the project's kernel is the path whichever way it comes out.
Also measured: the share of the crop in one scene_fid() batch of 16 captions next to the trunk -- ObjectCodes.sink with an encoder
that does nothing (the read-back of tm, the object list and the crops of both sides), and CNN_ENCODER.pool_code on one staging
batch (16, 3, 299, 299), of which the batch's 48 objects need three per side.
python tools/time_scene_fid.py [--out profiles/scene_fid_timing.json]"""
import argparse, json, os, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mogan_loader; mogan_loader.load()
from mogan_amd.attngan import scenefid as SF
from mogan_amd.hip import ops
ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=16)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--warmup", type=int, default=8)
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--out", default="")
args = ap.parse_args()
assert torch.cuda.is_available(), "a timing needs the GPU"
dev = torch.device("cuda")
B, S, G, T = args.images, args.size, SF.MAX_OBJECTS, SF.TRUNK_SIZE
rng = np.random.RandomState(5)
# every slot present: 48 objects of 16 images, boxes as the synthetic data set draws them
xy, wh = rng.uniform(0.0, 0.5, (B, G, 2)), rng.uniform(0.1, 0.5, (B, G, 2))
host_boxes = torch.from_numpy(np.concatenate([xy, wh], axis=2).astype(np.float32))
from mogan_amd.attngan.miscc.utils import compute_transformation_matrix
tm = compute_transformation_matrix(host_boxes.view(-1, 4)).view(B, G, 2, 3).to(dev)
index, boxes = SF.object_list(host_boxes, B, S)
R = int(index.shape[0])
gen = torch.Generator(device=dev).manual_seed(5)
real = torch.rand((B, 3, S, S), device=dev, generator=gen) * 2 - 1
fake = torch.rand((B, 3, S, S), device=dev, generator=gen) * 2 - 1
present = (index.long() + B * torch.arange(G).repeat(B)[:R]).to(dev)     # row of (image, slot) in stn_shared's object-major batch
out = torch.empty((R, 3, T, T), device=dev)


def timed(fn):
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record(); res = fn(); e1.record()
    return res, (e0, e1)


def kernel_crop():
    return ops.roi_resize(real, boxes, index, T, T, out=out)


def stock_crop():
    return ops.stn_shared(real, tm, B * G, (S, S), (T, T), theta_G=G).index_select(0, present)


def median_us(events):
    return statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in events)


PATHS = {"kernel": kernel_crop, "stock": stock_crop}
events = {name: [] for name in PATHS}
with torch.no_grad():
    for r in range(args.warmup + args.calls):
        for name, fn in PATHS.items():
            _, ev = timed(fn)
            if r >= args.warmup:
                events[name].append(ev)
torch.cuda.synchronize()
us = {name: [e0.elapsed_time(e1) * 1e3 for e0, e1 in events[name]] for name in PATHS}
result = {"method": "hip events around every call; %d warm-up calls and the median of %d per path, the two paths alternating call by "
                    "call in one process; microseconds" % (args.warmup, args.calls),
          "device": torch.cuda.get_device_name(0),
          "workload": {"images": B, "size": S, "objects": R, "out": T},
          "kernel_us": round(statistics.median(us["kernel"]), 1), "kernel_min_us": round(min(us["kernel"]), 1),
          "kernel_max_us": round(max(us["kernel"]), 1),
          "stock_us": round(statistics.median(us["stock"]), 1), "stock_min_us": round(min(us["stock"]), 1),
          "stock_max_us": round(max(us["stock"]), 1),
          "stock_route": "ops.stn_shared over %d slots, then index_select of the %d present rows" % (B * G, R)}
result["stock_over_kernel"] = round(result["stock_us"] / result["kernel_us"], 3)
need = R * 3 * T * T * 4                                          # what the crop has to write; it reads less
result["bytes_the_crop_writes"] = need
result["kernel_TB_per_s_of_those_bytes"] = round(need / result["kernel_us"] / 1e6, 3)
print(json.dumps(result), flush=True)

# ------------------------------------------------------------------------------------------------ the share of one scene_fid() batch
from mogan_amd.attngan import model
from mogan_amd.attngan.miscc.config import cfg, set_coco_train_defaults
set_coco_train_defaults()
torch.manual_seed(3)
enc = model.CNN_ENCODER(cfg.TEXT.EMBEDDING_DIM)
for p in enc.parameters():
    p.requires_grad = False
enc = enc.to(dev).eval()


class NoTrunk:
    """the encoder's place in ObjectCodes.sink without its work"""
    emb_cnn_code = enc.emb_cnn_code
    codes = torch.zeros((B, 2048), device=dev)

    def pool_code(self, x):
        return self.codes


acc = SF.ObjectCodes(B, B, S, device=dev)
idle = NoTrunk()


def crops():
    acc.fill = acc.n = acc.n_images = 0
    acc.image, acc.box = [], []
    acc.sink(real, fake, tm, B, idle)


def trunk():
    return enc.pool_code(acc.stage["real"])


share = {"crops": [], "trunk": []}
with torch.no_grad():
    for r in range(args.warmup + args.calls):
        for name, fn in (("crops", crops), ("trunk", trunk)):
            _, ev = timed(fn)
            if r >= args.warmup:
                share[name].append(ev)
torch.cuda.synchronize()
cr, tr = median_us(share["crops"]), median_us(share["trunk"])
runs = 2 * -(-R // B)
result["batch_share"] = {"captions": B, "objects": R, "encoder": "coco_train widths, random init, eval mode, frozen",
                         "crops_of_both_sides_us": round(cr, 1), "one_trunk_run_at_the_batch_size_us": round(tr, 1),
                         "trunk_runs_for_the_batch": runs,
                         "crop_share_of_crops_plus_trunk": round(cr / (cr + runs * tr), 4)}
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
