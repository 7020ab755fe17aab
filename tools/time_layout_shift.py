"""Layout-shift sums (attngan/layoutshift.py; csrc/mogan_layout.hip) at the real workload -- ShiftResponse.add for 16 pairs of
3 x 256 x 256 images, one launch -- against the same sums formed by stock torch ops on the device without a host synchronisation:
batched class masks by comparison and torch.where, the squared difference in fp64, one masked reduction per class, and the two sums
over the old rectangle against copies of b and of a rolled by -delta (reductions whose bits depend on the batch shape).
Hip events around every call, 8 warm-up calls and the median of 30 per path, the paths alternating call by call in one process.  A
record, not a gate: no speed target was set -- what the kernel is there for is the bit contracts of include/mogan_hip.h.  The torch
formulation lives only here.
Also measured: the two generator forwards of a batch (coco_train widths, 16 captions), next to which the scoring runs.
python tools/time_layout_shift.py [--out profiles/layout_shift_timing.json]"""
import argparse, json, os, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mogan_loader; mogan_loader.load()
from mogan_amd.attngan import layoutshift as LS
ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=16, help="image pairs per add()")
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--warmup", type=int, default=8)
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--out", default="")
args = ap.parse_args()
assert torch.cuda.is_available(), "a timing needs the GPU"
dev = torch.device("cuda")
B, C, S, G = args.pairs, 3, args.size, 3
g = torch.Generator(device=dev).manual_seed(5)
a = torch.rand((B, C, S, S), device=dev, generator=g) * 2 - 1
b = (0.5 * a + 0.5 * (torch.rand((B, C, S, S), device=dev, generator=g) * 2 - 1)).contiguous()
rng = np.random.RandomState(5)
boxes = np.zeros((B, G, 4), dtype=np.float32)
boxes[:, :, :2] = rng.uniform(0.0, 0.5, (B, G, 2))
boxes[:, :, 2:] = rng.uniform(0.1, 0.5, (B, G, 2))
boxes = torch.from_numpy(boxes)
acc = LS.ShiftResponse(S, C, B, None, 1, 5, dev)
table = acc.edits(boxes, B)
assert len(table["row"]) == B
edit, others = table["edit"].numpy(), table["others"].numpy()


def timed(fn):
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record(); out = fn(); e1.record()
    return out, (e0, e1)


def kernel_add():
    acc.n_images, acc.info, acc._sums, acc._counts = 0, [], [], []
    return acc.add(a, b, table)[0]


# the tables on the device, once, outside the timed region: the torch path never reads a value back or asks for a mask's size
edit_d = torch.from_numpy(edit).to(dev).long()
others_d = torch.from_numpy(others).to(dev).long()
yy = torch.arange(S, device=dev).view(1, S, 1)
xx = torch.arange(S, device=dev).view(1, 1, S)
shifts = [(-int(e[5]), -int(e[4])) for e in edit]                  # host integers, known before the call


def inside(r):
    """(B, S, S) bool of rectangles r (B, 4)"""
    return ((xx >= r[:, 0].view(-1, 1, 1)) & (xx < r[:, 2].view(-1, 1, 1))
            & (yy >= r[:, 1].view(-1, 1, 1)) & (yy < r[:, 3].view(-1, 1, 1)))


def torch_add():
    """the same sums in stock torch without a host synchronisation: batched masks by comparison, torch.where for the classes, one
    masked reduction per class, and the two sums over the old rectangle against copies of b and of a rolled by -delta"""
    a64, b64 = a.double(), b.double()
    d2 = ((a64 - b64) ** 2).sum(dim=1)
    old = inside(edit_d[:, :4])
    new = inside(edit_d[:, :4] + edit_d[:, 4:6].repeat(1, 2))
    other = torch.zeros_like(old)
    for g in range(others_d.shape[1]):
        r = others_d[:, g]
        other |= inside(r) & (r[:, 2] > r[:, 0]).view(-1, 1, 1)
    four = torch.where(other, 3, 4)
    cls = torch.where(old & new, 2, torch.where(old, 0, torch.where(new, 1, four)))
    out = torch.empty((B, 7), dtype=torch.float64, device=dev)
    for k in range(5):
        out[:, k] = (d2 * (cls == k)).sum(dim=(1, 2))
    b_at = torch.stack([torch.roll(b64[p], shifts[p], dims=(1, 2)) for p in range(B)])
    a_at = torch.stack([torch.roll(a64[p], shifts[p], dims=(1, 2)) for p in range(B)])
    m = old.unsqueeze(1)
    out[:, 5] = (((a64 - b_at) ** 2) * m).sum(dim=(1, 2, 3))
    out[:, 6] = (((a64 - a_at) ** 2) * m).sum(dim=(1, 2, 3))
    return out


from mogan_amd.attngan import model, synthetic
from mogan_amd.attngan.evaluate import moved_matrices
from mogan_amd.attngan.miscc.config import cfg, set_coco_train_defaults
from mogan_amd.attngan.miscc.utils import weights_init
set_coco_train_defaults()
torch.manual_seed(3)
netG = model.G_NET()
netG.apply(weights_init)
netG = netG.to(dev).eval()
bt = synthetic.to_device(synthetic.make_batch(B, words_num=cfg.TEXT.WORDS_NUM, nef=cfg.TEXT.EMBEDDING_DIM, seed=3), dev)
tmi_b = moved_matrices(bt["tmi"], table)


def forwards():
    with torch.no_grad():
        for tmi in (bt["tmi"], tmi_b):
            netG(bt["z"], bt["sent_emb"], bt["words_embs"], bt["mask"], tmi, bt["label_one_hot"], eps=bt["eps"])


def op_alone():
    from mogan_amd.hip import ops
    return ops.box_shift_sums(a, b, table["edit"], table["others"])[0]


PATHS = {"kernel": kernel_add, "op_alone": op_alone, "torch": torch_add, "two_forwards": forwards}
events = {name: [] for name in PATHS}
sums = {}
for r in range(args.warmup + args.calls):
    for name, fn in PATHS.items():
        out, ev = timed(fn)
        if r >= args.warmup:
            events[name].append(ev)
        sums[name] = out
torch.cuda.synchronize()
us = {name: [e0.elapsed_time(e1) * 1e3 for e0, e1 in events[name]] for name in PATHS}
med = {name: statistics.median(v) for name, v in us.items()}
result = {"method": "hip events around every call; %d warm-up calls and the median of %d per path, the paths alternating call "
                    "by call in one process; microseconds.  kernel: ShiftResponse.add -- the gather of the pairs' rows, one upload of "
                    "the tables, one launch.  op_alone: ops.box_shift_sums on the whole batch -- the upload and the launch.  torch: the "
                    "same sums from stock torch ops, batched, with no host synchronisation.  two_forwards: the generator's two forwards "
                    "of the batch (coco_train widths, random init, eval mode), which the scoring runs next to" % (args.warmup, args.calls),
          "device": torch.cuda.get_device_name(0),
          "workload": {"pairs": B, "channels": C, "size": S, "others_per_pair": G - 1}}
for name in PATHS:
    result[name + "_us"] = round(med[name], 1)
    result[name + "_min_us"] = round(min(us[name]), 1)
    result[name + "_max_us"] = round(max(us[name]), 1)
result["torch_over_kernel"] = round(med["torch"] / med["kernel"], 3)
result["scoring_share_of_two_forwards_plus_scoring"] = round(med["kernel"] / (med["kernel"] + med["two_forwards"]), 5)
result["largest_relative_difference_of_a_sum_between_the_paths"] = float(
    ((sums["kernel"] - sums["torch"]).abs() / sums["torch"].clamp_min(1e-300)).max())
need = 2 * B * C * S * S * 4
result["bytes_the_images_hold"] = need
result["kernel_TB_per_s_of_those_bytes"] = round(need / med["kernel"] / 1e6, 3)
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
