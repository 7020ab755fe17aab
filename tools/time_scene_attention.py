"""Attention sheets (attngan/attnsheet.py; csrc/mogan_attn_sheet.hip) at the scene mode's workload -- 16 images, the top 5 of 12 words,
at both attention stages (64 -> 256 and 128 -> 256) -- against
  (i)  the host path, miscc/vis.build_super_images2 on the same maps and images (wall clock, one call per stage: it takes seconds), and
  (ii) the same stages formed by stock torch ops on the device: the threshold, two fp64 matmuls with the same table, amin / amax,
       the quantisation and the integer blend, batched over the picks, with no host synchronisation.
Hip events around every device call, 8 warm-up calls and the median of 30 per path, the paths alternating call by call in one process.
A record, not a gate: no speed target was set -- what the kernel is there for is the one-launch read-out and the bit contracts of
include/mogan_hip.h.  The torch formulation lives only here.
Also measured: the generator's forward of the 16 images (coco_train widths), next to which the sheets are made.
python tools/time_scene_attention.py [--out profiles/scene_attention_timing.json]"""
import argparse, json, os, statistics, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mogan_loader; mogan_loader.load()
from mogan_amd.attngan import attnsheet as AS
from mogan_amd.attngan.miscc import vis
from mogan_amd.hip import ops
ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=16)
ap.add_argument("--words", type=int, default=12)
ap.add_argument("--topk", type=int, default=5)
ap.add_argument("--warmup", type=int, default=8)
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--no_host", action="store_true", help="leave the host path out (it takes most of the run)")
ap.add_argument("--out", default="")
args = ap.parse_args()
assert torch.cuda.is_available(), "a timing needs the GPU"
dev = torch.device("cuda")
B, T, K, VIS = args.images, args.words, args.topk, 256
g = torch.Generator(device=dev).manual_seed(5)
img = (torch.rand((B, 3, VIS, VIS), device=dev, generator=g) * 2 - 1).contiguous()
lens = torch.full((B,), T, dtype=torch.int32)
stage = {}
for att in (64, 128):
    attn = torch.softmax(torch.randn((B, T, att, att), device=dev, generator=g) * 2, dim=1).contiguous()
    M = torch.from_numpy(AS.table(att, VIS // att)).to(dev)
    conf = ops.attn_conf(attn, lens).cpu().numpy()
    pick = torch.tensor([(s, w) for s in range(B) for w in AS.top_words(conf[s], T, K)], dtype=torch.int32)
    stage[att] = (attn, M, pick, pick.to(dev).long())


def timed(fn):
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record(); out = fn(); e1.record()
    return out, (e0, e1)


def kernel(att):
    attn, M, pick, _ = stage[att]
    return lambda: ops.attn_sheet(attn, lens, img, M, pick, AS.ALPHA)[0]


def conf_op(att):
    return lambda: ops.attn_conf(stage[att][0], lens)


t2 = float(AS.thresholds(T)[0])


def torch_path(att):
    attn, M, _, pick = stage[att]

    def run():
        a = attn[pick[:, 0], pick[:, 1]]
        A = (a * (a > t2)).double()
        S = M @ A @ M.t()
        lo, hi = S.amin(dim=(1, 2), keepdim=True), S.amax(dim=(1, 2), keepdim=True)
        q = ((S - lo) / (hi - lo) * 255).floor().to(torch.int32)
        image = ((img + 1) / 2 * 255).clamp(0, 255).to(torch.int32).permute(0, 2, 3, 1)[pick[:, 0]]
        t = image * (255 - AS.ALPHA) + q.unsqueeze(-1) * AS.ALPHA + 128
        return (((t >> 8) + t) >> 8).to(torch.uint8)
    return run


from mogan_amd.attngan import model, synthetic
from mogan_amd.attngan.miscc.config import cfg, set_coco_train_defaults
from mogan_amd.attngan.miscc.utils import weights_init
set_coco_train_defaults()
torch.manual_seed(3)
netG = model.G_NET()
netG.apply(weights_init)
netG = netG.to(dev).eval()
bt = synthetic.to_device(synthetic.make_batch(B, words_num=cfg.TEXT.WORDS_NUM, nef=cfg.TEXT.EMBEDDING_DIM, seed=3), dev)


def forward():
    with torch.no_grad():
        return netG(bt["z"], bt["sent_emb"], bt["words_embs"], bt["mask"], bt["tmi"], bt["label_one_hot"], eps=bt["eps"])[0][-1]


PATHS = {"forward": forward}
for att in (64, 128):
    PATHS.update({"kernel_%d" % att: kernel(att), "conf_%d" % att: conf_op(att), "torch_%d" % att: torch_path(att)})
events = {name: [] for name in PATHS}
last = {}
for r in range(args.warmup + args.calls):
    for name, fn in PATHS.items():
        out, ev = timed(fn)
        if r >= args.warmup:
            events[name].append(ev)
        last[name] = out
torch.cuda.synchronize()
us = {name: [e0.elapsed_time(e1) * 1e3 for e0, e1 in events[name]] for name in PATHS}
med = {name: statistics.median(v) for name, v in us.items()}
result = {"method": "hip events around every device call; %d warm-up calls and the median of %d per path, the paths alternating call by "
                    "call in one process; microseconds.  kernel_<att>: ops.attn_sheet for all picks of the stage -- one upload of the "
                    "lengths and picks, one launch.  conf_<att>: ops.attn_conf, what the top-K choice reads.  torch_<att>: the same "
                    "stages from stock torch ops (threshold, two fp64 matmuls with the same table, amin / amax, quantisation, integer "
                    "blend), batched over the picks, no host synchronisation.  host_<att>: miscc/vis.build_super_images2 on the same "
                    "maps and images, ONE call per stage by the wall clock -- it smooths all %d words of every image, as the reference "
                    "does, before it keeps the top %d.  forward: the generator's forward of the %d images (coco_train widths, random "
                    "init, eval mode)" % (args.warmup, args.calls, T, K, B),
          "device": torch.cuda.get_device_name(0),
          "workload": {"images": B, "words": T, "topk": K, "picks_per_stage": B * K, "vis": VIS, "stages": [64, 128]}}
for name in PATHS:
    result[name + "_us"] = round(med[name], 1)
    result[name + "_min_us"] = round(min(us[name]), 1)
    result[name + "_max_us"] = round(max(us[name]), 1)
for att in (64, 128):
    result["torch_over_kernel_%d" % att] = round(med["torch_%d" % att] / med["kernel_%d" % att], 3)
    d = (last["kernel_%d" % att].to(torch.int32) - last["torch_%d" % att].to(torch.int32)).abs()
    result["bytes_that_differ_between_kernel_and_torch_%d" % att] = int((d > 0).sum())
    result["largest_byte_difference_%d" % att] = int(d.max())
    # 2 FMA-flops per term: U = M A per strip and S = U M^T, walked twice
    flops = 2 * 2 * B * K * VIS * att * (att + VIS)
    result["kernel_fp64_TFLOPs_%d" % att] = round(flops / med["kernel_%d" % att] / 1e6, 3)
both = med["kernel_64"] + med["kernel_128"] + med["conf_64"] + med["conf_128"]
result["sheets_us_both_stages_with_conf"] = round(both, 1)
result["sheets_share_of_forward_plus_sheets"] = round(both / (both + med["forward"]), 5)
if not args.no_host:
    caps = torch.arange(1, T + 1)[None].repeat(B, 1)
    ixtoword = {i: "w%d" % i for i in range(T + 1)}
    host_img = img.cpu()
    for att in (64, 128):
        maps = [m for m in stage[att][0].cpu()]
        t0 = time.perf_counter()
        drawn = vis.build_super_images2(host_img, caps, lens.numpy(), ixtoword, maps, att, VIS, topK=K)[0]
        result["host_%d_us" % att] = round((time.perf_counter() - t0) * 1e6, 1)
        result["host_over_kernel_%d" % att] = round(result["host_%d_us" % att] / med["kernel_%d" % att], 1)
        sheet = last["kernel_%d" % att].cpu().numpy().reshape(B, K, VIS, VIS, 3)
        host = np.stack([np.stack([drawn[s * (vis.FONT_MAX + VIS) + vis.FONT_MAX:(s + 1) * (vis.FONT_MAX + VIS), i * (VIS + 2):i * (VIS + 2) + VIS]
                                   for i in range(K)]) for s in range(B)])
        result["bytes_that_differ_between_kernel_and_host_%d" % att] = int((sheet != host).sum())
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
