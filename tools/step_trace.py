"""Which launches does a train step queue, in which host order, on which stream?  The reduced-width engine of tests/test_model_gpu.py,
three steps per launch mode, with hip/lib.call (and the name hip/ops.py imported), torch.cuda.CUDAGraph.replay and
torch.distributed.all_reduce wrapped: each records (name, index of the current stream in first-seen order of the mode).  Prints per mode
and step the length and a SHA-1 of the sequence ("all": host order over all streams) and of the per-stream sub-sequences ("per_stream").
Evidence for a change of the step's schedule that must not move a launch: run it on both commits and compare the lines.  `--rccl` adds the
data-parallel modes on a one-rank RCCL group (the collectives' place in each stream's order); `--json FILE` also writes the digests."""
import hashlib, json, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import det_fill_state, load_pkg
from standin import StandInEncoder
load_pkg()
from mogan_amd.attngan import model, synthetic
from mogan_amd.attngan.miscc.config import cfg
from mogan_amd.attngan.trainer import TrainEngine
from mogan_amd.hip import lib, ops

rccl = "--rccl" in sys.argv
DEV = torch.device("cuda", 0)
torch.cuda.set_device(DEV)
cfg.GAN.GF_DIM, cfg.GAN.DF_DIM, cfg.GAN.R_NUM, cfg.GAN.Z_DIM = 4, 4, 2, 100
cfg.TEXT.EMBEDDING_DIM, cfg.TEXT.WORDS_NUM, cfg.TREE.BRANCH_NUM = 16, 5, 3
cfg.TRAIN.GENERATOR_LR = cfg.TRAIN.DISCRIMINATOR_LR = 2e-4

trace, seen = [], {}


def note(name):
    s = torch.cuda.current_stream().cuda_stream
    trace.append((name, seen.setdefault(s, len(seen))))


def wrap(fn, name_of):
    def wrapped(*a, **k):
        note(name_of(a))
        return fn(*a, **k)
    return wrapped


lib.call = ops.call = wrap(lib.call, lambda a: a[0])
torch.cuda.CUDAGraph.replay = wrap(torch.cuda.CUDAGraph.replay, lambda a: "graph.replay")
torch.distributed.all_reduce = wrap(torch.distributed.all_reduce, lambda a: "all_reduce[%d]" % a[0].numel())


def sha(seq):
    return hashlib.sha1(repr(seq).encode()).hexdigest()[:16]


def build():
    G = model.G_NET()
    det_fill_state(G, "G.")
    Ds = []
    for i, cls in enumerate((model.D_NET64, model.D_NET128, model.D_NET256)):
        D = cls()
        det_fill_state(D, "D%d." % i)
        Ds.append(D.to(DEV).train())
    enc = StandInEncoder(16)
    det_fill_state(enc, "ENC.")
    for p in enc.parameters():
        p.requires_grad = False
    return enc.to(DEV).eval(), G.to(DEV).train(), Ds


# mode: (branch_graphs, g_graphs, g_fwd_only, inputs_ready, multi_stream, distributed)
MODES = [("eager multi-stream", (False, False, False, False, True, False)),
         ("eager, inputs_ready", (False, False, False, True, True, False)),
         ("branch graphs, eager generator", (True, False, False, True, True, False)),
         ("branch graphs, forward graph", (True, True, True, True, True, False)),
         ("branch graphs, forward and backward graphs", (True, True, False, True, True, False)),
         ("single-stream", (False, False, False, False, False, False))]
if rccl:
    import torch.distributed as dist
    os.environ["MOGAN_FORCE_DIST"] = "1"
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % (29300 + os.getpid() % 500), rank=0, world_size=1)
    MODES += [("one-rank RCCL, eager", (False, False, False, True, True, True)),
              ("one-rank RCCL, branch graphs, forward graph", (True, True, True, True, True, True))]

report = {}
for name, (bgr, gg, fwd, ready, ms, dp) in MODES:
    enc, G, Ds = build()
    eng = TrainEngine(None, enc, G, Ds, distributed=dp, use_graph=False, branch_graphs=bgr)
    eng.g_graphs, eng.g_fwd_only, eng.multi_stream = gg, fwd, ms
    seen.clear()
    rows = []
    for step in range(3):
        bt = synthetic.to_device(synthetic.make_batch(4, words_num=5, nef=16, seed=100 + step), DEV)
        if ready:
            torch.cuda.synchronize()
            bt["inputs_ready"] = torch.cuda.Event()
            bt["inputs_ready"].record()
        del trace[:]
        eng.step(bt)
        torch.cuda.synchronize()
        per = {}
        for n, s in trace:
            per.setdefault(s, []).append(n)
        rows.append({"launches": len(trace), "all": sha(trace), "per_stream": sha(sorted(per.values()))})
        print("%-44s step %d: %5d launches on %2d streams, all %s, per_stream %s"
              % (name, step, len(trace), len(per), rows[-1]["all"], rows[-1]["per_stream"]), flush=True)
    report[name] = rows
    eng.close()
if rccl:
    dist.destroy_process_group()
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        json.dump(report, f, indent=1)
