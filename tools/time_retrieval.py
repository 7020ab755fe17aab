"""R-precision's ranking step (mogan_retrieval_rank, csrc/mogan_damsm.hip) against a stock-torch formulation of the same function
(gather the candidates, norms, bmm, compare), and the share of one condGANTrainer.r_precision batch that the retrieval step takes.
Method of tools/time_text.py: hip events, --warmup calls, then --iters timed calls of each path, the two paths alternating in one
process; medians.  The stock formulation lives only here.
python tools/time_retrieval.py [--out profiles/retrieval_timing.json] [--no-batch]"""
import argparse, json, os, statistics, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mogan_loader; mogan_loader.load()
from mogan_amd.hip import ops
ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--warmup", type=int, default=8)
ap.add_argument("--out", default="")
ap.add_argument("--no-batch", action="store_true", help="skip the share of a whole r_precision batch")
args = ap.parse_args()
dev = torch.device("cuda")


def stock(code, pos, bank, idx, eps=1e-8):
    cand = torch.cat([pos[:, None, :], bank[idx.long()]], 1)                       # (Q, Rn + 1, C) in memory
    w12 = torch.bmm(cand, code[:, :, None]).squeeze(2)
    s = w12 / (torch.norm(code, 2, 1)[:, None] * torch.norm(cand, 2, 2)).clamp(min=eps)
    return (s[:, 1:] > s[:, :1]).sum(1).int()


def timed(fn):
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


result = {"method": "hip events around one call, %d warm-up calls, %d timed calls per path, paths alternating in one process, "
                    "medians in microseconds" % (args.warmup, args.iters), "device": torch.cuda.get_device_name(0), "shapes": []}
for Q, Rn, C, N in ((16, 99, 256, 200000), (64, 99, 256, 200000)):
    g = torch.Generator(device=dev).manual_seed(Q)
    code, pos = torch.randn(Q, C, device=dev, generator=g), torch.randn(Q, C, device=dev, generator=g)
    bank = torch.randn(N, C, device=dev, generator=g)
    idx = torch.randint(0, N, (Q, Rn), device=dev, generator=g, dtype=torch.int32)
    paths = {"kernel": lambda: ops.retrieval_rank(code, pos, bank, idx), "stock_torch": lambda: stock(code, pos, bank, idx)}
    differ = int((paths["kernel"]() != paths["stock_torch"]()).sum())               # (a near-tie may fall differently in two fp32 orders)
    for _ in range(args.warmup):
        for fn in paths.values(): fn()
    torch.cuda.synchronize()
    us = {k: [] for k in paths}
    for _ in range(args.iters):
        for k, fn in paths.items(): us[k].append(timed(fn))
    row = {"Q": Q, "Rn": Rn, "C": C, "N": N, "ranks_that_differ_between_the_paths": differ}
    row.update({k + "_us": round(statistics.median(v), 2) for k, v in us.items()})
    row.update({k + "_min_us": round(min(v), 2) for k, v in us.items()})
    result["shapes"].append(row)
    print(row, flush=True)

if not args.no_batch:
    # one r_precision batch at the coco widths, B = 16, random-init networks: text encoder, eval generator, image encoder, then the
    # retrieval step (draw_mismatched on the host over a 200 000-caption index, upload, the kernel); wall clock, synchronised
    from mogan_amd.attngan import model
    from mogan_amd.attngan.miscc.config import cfg, set_coco_train_defaults
    from mogan_amd.attngan.retrieval import draw_mismatched
    from mogan_amd.attngan import synthetic
    set_coco_train_defaults()
    B, T, N = 16, cfg.TEXT.WORDS_NUM, 200000
    torch.manual_seed(0)
    with torch.no_grad():
        text = model.RNN_ENCODER(27297, nhidden=cfg.TEXT.EMBEDDING_DIM).to(dev).eval()
        image = model.CNN_ENCODER(cfg.TEXT.EMBEDDING_DIM).to(dev).eval()
        for p in image.parameters(): p.requires_grad = False
        netG = model.G_NET().to(dev).eval()
        bt = synthetic.to_device(synthetic.make_batch(B, words_num=T, nef=cfg.TEXT.EMBEDDING_DIM, seed=1, text="tokens"), dev)
        bank = torch.randn(N, cfg.TEXT.EMBEDDING_DIM, device=dev)
        image_index = np.arange(N) // 5
        rng = np.random.RandomState(0)
        lens = bt["cap_lens"].cpu()

        def batch():
            t0 = time.perf_counter()
            words, sent = text(bt["captions"], lens, text.init_hidden(B))
            fake = netG(bt["z"], sent.contiguous(), words.contiguous(), bt["mask"][:, :words.size(2)], bt["tmi"], bt["label_one_hot"],
                        eps=bt["eps"])[0][-1]
            code = image(fake)[1]
            torch.cuda.synchronize(); t1 = time.perf_counter()
            idx = draw_mismatched(image_index, rng.randint(0, N // 5, B), 99, rng)
            t2 = time.perf_counter()
            ops.retrieval_rank(code, sent, bank, idx)
            torch.cuda.synchronize(); t3 = time.perf_counter()
            return (t3 - t0) * 1e3, (t3 - t1) * 1e3, (t2 - t1) * 1e3
        for _ in range(3): batch()
        runs = [batch() for _ in range(10)]
    tot, ret, draw = (statistics.median(r[k] for r in runs) for k in range(3))
    result["batch"] = {"B": B, "bank_rows": N, "batch_ms": round(tot, 3), "retrieval_step_ms": round(ret, 3),
                       "of_which_host_draw_ms": round(draw, 3), "retrieval_share": round(ret / tot, 4),
                       "note": "wall clock, synchronised after the image encoder and after the kernel; 3 warm-up batches, median of 10"}
    print(result["batch"], flush=True)
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
