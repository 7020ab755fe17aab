"""-m gpu: (1) the HIP Inception-v3 trunk (CNN_ENCODER) against its torch-CPU restatement
(oracle/inception_oracle.py; the Inception arithmetic is unpinned by the reference),
forward and input-gradient; (2) the drop-in entry point: main.py -> condGANTrainer.train() on synthetic
batches for two iterations, checkpoint written in the reference's format."""
import glob
import os

import numpy as np
import pytest
import torch

from helpers import ROOT, load_pkg

load_pkg()
from mogan_amd.attngan.miscc.config import cfg  # noqa: E402
from oracle import inception_oracle as IO  # noqa: E402

pytestmark = pytest.mark.gpu


def test_cnn_encoder_vs_cpu_restatement(monkeypatch):
    from mogan_amd.attngan import model
    cfg.TRAIN.FLAG, cfg.TEXT.EMBEDDING_DIM = True, 32
    torch.manual_seed(3)
    enc = model.CNN_ENCODER(32)
    # non-trivial eval-mode BN statistics
    for m in enc.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.05); m.running_var.uniform_(0.8, 1.2); m.weight.data.uniform_(0.9, 1.1)
            m.bias.data.normal_(0, 0.05)
    enc.eval()
    sd = {k: v.detach().clone().double() for k, v in enc.state_dict().items()}
    x = (torch.rand(2, 3, 256, 256) * 2 - 1).requires_grad_(True)
    gf, gc = torch.randn(2, 32, 17, 17), torch.randn(2, 32)
    f_ref, c_ref = IO.cnn_encoder(sd, x.double())
    ((f_ref * gf.double()).sum() + (c_ref * gc.double()).sum()).backward()
    enc = enc.cuda()
    xd = x.detach().cuda().requires_grad_(True)
    f, c = enc(xd)
    ((f * gf.cuda()).sum() + (c * gc.cuda()).sum()).backward()
    rel = lambda a, b: float((a.detach().cpu().double() - b.detach()).norm() / b.detach().norm())
    assert tuple(f.shape) == (2, 32, 17, 17) and tuple(c.shape) == (2, 32)
    assert rel(f, f_ref) < 2e-5, rel(f, f_ref)
    assert rel(c, c_ref) < 2e-5, rel(c, c_ref)
    # input gradient: 94 convs deep with ReLU / max-pool kinks -- torch-CPU fp32 vs fp64 of this very restatement
    # already differ by 9.9e-3 rel-L2 on these inputs (decisions that flip at the fp32 noise floor), so that is the scale
    assert rel(xd.grad, x.grad) < 3e-2, rel(xd.grad, x.grad)
    # the train step's path: frozen encoder -> explicit forward / backward over the folded, grouped trunk
    # (inception.FrozenTrunk: grouped 1x1 convolutions, outputs written into the concatenated tensors, ReLU backward fused
    # into the data gradients) -- same checks, plus agreement with the module-by-module evaluation above
    from mogan_amd.attngan import inception
    assert inception.FAST_TRUNK
    for p_ in enc.parameters():
        p_.requires_grad = False
    assert enc._frozen()
    xf = x.detach().cuda().requires_grad_(True)
    import inception_decisions as D
    runs, fwd = [], inception.PanelTrunk.forward

    def recorded(self, x299):
        out = fwd(self, x299)
        runs.append((self, out[0]))
        return out
    with D.recording(monkeypatch) as rec, monkeypatch.context() as m:
        m.setattr(inception.PanelTrunk, "forward", recorded)
        f2, c2 = enc(xf)
    ((f2 * gf.cuda()).sum() + (c2 * gc.cuda()).sum()).backward()
    torch.cuda.synchronize()
    assert rel(f2, f_ref) < 2e-5 and rel(c2, c_ref) < 2e-5, (rel(f2, f_ref), rel(c2, c_ref))
    assert rel(f2, f.detach().cpu().double()) < 2e-6, rel(f2, f.detach().cpu().double())
    assert rel(xf.grad, x.grad) < 3e-2, rel(xf.grad, x.grad)
    print("frozen trunk: features vs fp64 %.1e, vs module path %.1e; image gradient vs fp64 %.1e (module path %.1e), vs module "
          "path %.1e" % (rel(f2, f_ref), rel(f2, f.detach().cpu().double()), rel(xf.grad, x.grad), rel(xd.grad, x.grad),
                         rel(xf.grad, xd.grad.detach().cpu().double())))
    # the same with the trunk's own ReLU / max-pool decisions imposed on the fp64 oracle: fp32 rounding is all that is left
    (trunk, tapes), = runs
    dec = D.decisions(trunk, tapes, rec)
    xm = x.detach().double().requires_grad_(True)
    with D.imposed(*dec) as flips:
        f_m, c_m = IO.cnn_encoder(sd, xm)
        ((f_m * gf.double()).sum() + (c_m * gc.double()).sum()).backward()
    n, worst = D.flip_summary(flips)
    print("frozen trunk, matched decisions: image gradient vs fp64 %.2e (%d flips, worst |pre| / rms %.1e)"
          % (rel(xf.grad, xm.grad), n, worst))
    assert rel(f2, f_m) < 2e-5 and rel(c2, c_m) < 2e-5, (rel(f2, f_m), rel(c2, c_m))
    assert rel(xf.grad, xm.grad) < 5e-5, rel(xf.grad, xm.grad)          # measured 9.2e-6 (31 flips)
    assert worst <= 1e-4, flips                                           # measured 1.1e-5


def test_main_trains_on_synthetic_and_checkpoints(tmp_path):
    from mogan_amd.attngan import main as entry
    yml = tmp_path / "tiny.yml"
    yml.write_text("CONFIG_NAME: 'tiny'\nDATASET_NAME: 'coco'\nWORKERS: 0\nTREE: {BRANCH_NUM: 3}\n"
                   "GAN: {DF_DIM: 8, GF_DIM: 8, Z_DIM: 100, R_NUM: 1}\n"
                   "TEXT: {EMBEDDING_DIM: 32, CAPTIONS_PER_IMAGE: 5, WORDS_NUM: 6}\n"
                   "TRAIN: {FLAG: True, BATCH_SIZE: 4, MAX_EPOCH: 1, SNAPSHOT_INTERVAL: 1, NET_E: ''}\n")
    out = tmp_path / "out"
    entry.main(["--cfg", str(yml), "--synthetic", "8", "--manualSeed", "7", "--output_dir", str(out)])
    ckpts = sorted(glob.glob(os.path.join(str(out), "Model", "checkpoint_*.pth")))
    assert ckpts, "no checkpoint written"
    sd = torch.load(ckpts[-1], map_location="cpu", weights_only=False)
    assert set(sd) == {"epoch", "netG", "optimG", "netD", "optimD"} and len(sd["netD"]) == 3
    assert "h_net1.upsample1.1.weight" in sd["netG"] and "COND_DNET.jointConv.0.weight" in sd["netD"][2]
    assert all(torch.isfinite(v).all() for v in sd["netG"].values() if v.is_floating_point())
    nbt = sd["netG"]["h_net1.fc.1.num_batches_tracked"]
    assert int(nbt) == 2                                   # two iterations, one BN call each


def test_train_writes_attention_grids(tmp_path):
    """trainer.py:206-248,335-346: with >= 8 samples per batch the first iteration of an epoch writes the attention grids
    of the two attention stages (G_average_<epoch>_<i>.png) and the DAMSM word-region attention (D_average_<epoch>.png),
    generated by the EMA weights."""
    from PIL import Image
    from mogan_amd.attngan import main as entry
    yml = tmp_path / "tiny.yml"
    yml.write_text("CONFIG_NAME: 'tiny'\nDATASET_NAME: 'coco'\nWORKERS: 0\nTREE: {BRANCH_NUM: 3}\n"
                   "GAN: {DF_DIM: 8, GF_DIM: 8, Z_DIM: 100, R_NUM: 1}\n"
                   "TEXT: {EMBEDDING_DIM: 32, CAPTIONS_PER_IMAGE: 5, WORDS_NUM: 6}\n"
                   "TRAIN: {FLAG: True, BATCH_SIZE: 8, MAX_EPOCH: 1, SNAPSHOT_INTERVAL: 1, NET_E: ''}\n")
    out = tmp_path / "out"
    entry.main(["--cfg", str(yml), "--synthetic", "8", "--manualSeed", "7", "--output_dir", str(out)])
    T, FONT = 6, 50
    for i, vis in ((0, 128), (1, 256)):
        im = Image.open(os.path.join(str(out), "Image", "G_average_0_%d.png" % i))
        assert im.size == ((T + 2) * (vis + 2), 8 * (FONT + 2 * vis))
    im = Image.open(os.path.join(str(out), "Image", "D_average_0.png"))
    assert im.size == ((T + 2) * (17 * 16 + 2), 8 * (FONT + 2 * 17 * 16))
    assert np.asarray(im).std() > 0


def test_sampling_from_a_checkpoint(tmp_path):
    """trainer.py:387-470: train one epoch, then load the checkpoint's (EMA) generator in eval mode and write one
    256x256 image per caption."""
    from PIL import Image
    from mogan_amd.attngan import main as entry
    from mogan_amd.attngan.datasets import SyntheticTextDataset
    from mogan_amd.attngan.miscc.config import cfg
    from mogan_amd.attngan.trainer import condGANTrainer
    yml = tmp_path / "tiny.yml"
    yml.write_text("CONFIG_NAME: 'tiny'\nDATASET_NAME: 'coco'\nWORKERS: 0\nTREE: {BRANCH_NUM: 3}\n"
                   "GAN: {DF_DIM: 8, GF_DIM: 8, Z_DIM: 100, R_NUM: 1}\n"
                   "TEXT: {EMBEDDING_DIM: 32, CAPTIONS_PER_IMAGE: 5, WORDS_NUM: 6}\n"
                   "TRAIN: {FLAG: True, BATCH_SIZE: 4, MAX_EPOCH: 1, SNAPSHOT_INTERVAL: 1, NET_E: ''}\n")
    out = tmp_path / "out"
    entry.main(["--cfg", str(yml), "--synthetic", "8", "--manualSeed", "7", "--output_dir", str(out)])
    ckpt = sorted(glob.glob(os.path.join(str(out), "Model", "checkpoint_*.pth")))[-1]
    cfg.TRAIN.NET_G, cfg.TRAIN.NET_E = ckpt, ''
    ds = SyntheticTextDataset(length=4, n_words=100)
    dl = torch.utils.data.DataLoader(ds, batch_size=4, drop_last=True, shuffle=False)
    algo = condGANTrainer(str(out), dl, 100, ds.ixtoword, resume=False)
    written = algo.sampling("valid")
    cfg.TRAIN.NET_G = ''
    assert len(written) == 4 and all(os.path.isfile(p) for p in written)
    im = np.asarray(Image.open(written[0]))
    assert im.shape == (256, 256, 3) and im.dtype == np.uint8 and im.std() > 0


def test_sample_rows_from_a_checkpoint_via_main(tmp_path):
    """trainer.py:474-579 / main.py:117-158: TRAIN.FLAG False + B_VALIDATION runs sample(): one PNG per batch, a row of
    [real | 9 generated] 256x256 images (make_grid padding 2, nrow 10) named after the caption, boxes drawn white."""
    from PIL import Image
    from mogan_amd.attngan import main as entry
    from mogan_amd.attngan.miscc.config import cfg
    yml = tmp_path / "tiny.yml"
    body = ("CONFIG_NAME: 'tiny'\nDATASET_NAME: 'coco'\nWORKERS: 0\nTREE: {BRANCH_NUM: 3}\n"
            "GAN: {DF_DIM: 8, GF_DIM: 8, Z_DIM: 100, R_NUM: 1}\n"
            "TEXT: {EMBEDDING_DIM: 32, CAPTIONS_PER_IMAGE: 5, WORDS_NUM: 6}\n")
    yml.write_text(body + "TRAIN: {FLAG: True, BATCH_SIZE: 4, MAX_EPOCH: 1, SNAPSHOT_INTERVAL: 1, NET_E: ''}\n")
    out = tmp_path / "out"
    entry.main(["--cfg", str(yml), "--synthetic", "8", "--manualSeed", "7", "--output_dir", str(out)])
    ckpt = sorted(glob.glob(os.path.join(str(out), "Model", "checkpoint_*.pth")))[-1]
    ev = tmp_path / "eval.yml"
    ev.write_text(body + "B_VALIDATION: True\nTRAIN: {FLAG: False, BATCH_SIZE: 4, NET_G: '%s', NET_E: ''}\n" % ckpt)
    try:
        entry.main(["--cfg", str(ev), "--synthetic", "12", "--manualSeed", "7", "--output_dir", str(out)])
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.FLAG, cfg.B_VALIDATION = '', True, False
    files = sorted(glob.glob(ckpt[:-4] + "_valid/*.png"))
    assert len(files) == 3                                  # 12 samples / batch 4, drop_last
    for f in files:
        name = os.path.basename(f)
        assert name.rsplit("_", 1)[1] in ("0.png", "1.png", "2.png") and name.startswith("w")      # 'w<ix> w<ix> ..._<step>'
        im = np.asarray(Image.open(f))
        assert im.shape == (256 + 4, 10 * 258 + 2, 3) and im.dtype == np.uint8
        tiles = [im[2:258, 2 + 258 * k: 258 + 258 * k] for k in range(10)]
        assert all(t.std() > 0 for t in tiles)
        assert any(np.abs(tiles[1].astype(int) - tiles[k].astype(int)).max() > 0 for k in range(2, 10))   # nine noises
        # the same white rectangle on every tile: value 1 is the maximum before normalisation; torchvision 0.2.1 divides
        # by (max - min + 1e-5) and truncates, so "white" is 254
        assert im.max() == 254
        white = [(t == 254).all(axis=2) for t in tiles]
        assert white[0].sum() >= 50 and all((white[0] & w).sum() >= 0.9 * white[0].sum() for w in white[1:])


def test_sample_rows_directly(tmp_path):
    """condGANTrainer.sample() on the tiny evaluation set-up (tests/eval_setup.py), without main.py: the files it returns, their
    names and directory, one row of 1 + 9 images each, the boxes drawn on request only, and the same bytes under the same seed."""
    from PIL import Image
    from eval_setup import tiny_checkpoint, trainer
    from mogan_amd.attngan.datasets import prepare_data
    from mogan_amd.attngan.evaluate import caption_sentence
    cfg, ev, ckpt = tiny_checkpoint(tmp_path)
    try:
        algo = trainer(tmp_path, length=8, eval=True)

        def run(draw_bbox):
            torch.manual_seed(5)
            files = algo.sample("test", num_samples=2, draw_bbox=draw_bbox)
            return files, [open(f, "rb").read() for f in files]
        files, boxed = run(True)
        assert len(files) == 2 and all(os.path.isfile(f) for f in files)
        for step, (f, data) in enumerate(zip(files, algo.data_loader)):
            captions = prepare_data(data, "cuda", eval=True)[1]
            sentence = caption_sentence(captions[0].cpu().numpy(), algo.ixtoword)
            assert sentence and os.path.basename(f) == "%s_%d.png" % (sentence, step)
            assert os.path.dirname(f) == ckpt[:-4] + "_valid"
            width, height = Image.open(f).size
            pad = (height - 256) // 2                              # one row: 256 pixels and the grid's padding above and below
            assert pad >= 0 and height == 256 + 2 * pad and width == 10 * (256 + pad) + pad
        again, boxed_again = run(True)
        assert again == files and boxed_again == boxed
        plain_files, plain = run(False)
        assert plain_files == files and all(a != b for a, b in zip(plain, boxed))
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.FLAG = '', True


def test_bench_two_ranks_control_flow():
    """`python bench.py --gpus 2 ... --full` as ONE plain command: bench.py re-executes itself under torch.distributed.run (2 ranks,
    the way the driver launches N>1 and what train.sh:25-29 hands to data_parallel in the reference) -- on this 1-GPU box
    both ranks share cuda:0 and the process group is gloo (MOGAN_ONE_GPU / MOGAN_DIST_BACKEND), which exercises everything
    but RCCL itself: matched collectives on every rank in the warm-up, the timed steps AND the roofline leg, the MAX
    over ranks, one JSON line from rank 0."""
    import json
    import subprocess
    import sys
    env = dict(os.environ, MOGAN_ONE_GPU="1", MOGAN_DIST_BACKEND="gloo", MOGAN_FAST_INIT="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--full", "--no-cpu-baseline"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 0 and len(lines) == 1, out.stderr[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 32 and d["scaling"] == "weak"
    assert "roofline" in d and "cpu_baseline" not in d and d["value"] > 0
    # the data-parallel diagnosis of the line: both launch modes measured in the one invocation, the better one reported,
    # and per gradient bucket its bytes, the time of its collectives and the time its consumer was held
    dp = d["dp"]
    assert dp["world_size_seen"] == 2 and dp["backend"] == "gloo" and set(dp["modes"]) == {"branch_graphs", "eager"}
    assert dp["mode_reported"] in dp["modes"] and abs(d["value"] - max(m["value"] for m in dp["modes"].values())) < 1e-6
    sizes = {"G": 69.7e6, "D64": 58.9e6, "D128": 171e6, "D256": 643e6}               # SURVEY section 8(e), bytes
    for mode, m in dp["modes"].items():
        assert set(m["buckets"]) == set(sizes), (mode, m["buckets"])
        for name, b in m["buckets"].items():
            assert abs(b["bytes_per_step"] - sizes[name]) <= 0.02 * sizes[name], (mode, name, b)
            assert b["collectives_per_step"] >= 1 and b["allreduce_ms"] > 0 and b["exposed_ms"] >= 0
    assert "hipGraphs" in dp["modes"]["branch_graphs"]["launch"] and dp["modes"]["eager"]["launch"].startswith("eager")


@pytest.mark.parametrize("parallel", [False, True])
def test_graphed_encoder_matches_eager(parallel, monkeypatch):
    """The train engine replays the frozen encoder as a hipGraph pair (optionally with the Mixed-block branches captured
    on parallel streams, inception._parallel): same kernels, so outputs and the image gradient must be identical to
    the eager, single-stream evaluation."""
    from mogan_amd.attngan import inception
    from mogan_amd.attngan.model import CNN_ENCODER
    monkeypatch.setattr(inception, "PARALLEL_BRANCHES", parallel)
    cfg.TRAIN.FLAG = True
    torch.manual_seed(3)
    enc = CNN_ENCODER(32).to("cuda").eval()
    for p in enc.parameters():
        p.requires_grad = False
    x = (torch.rand(2, 3, 256, 256, device="cuda") * 2 - 1)
    gf, gc = torch.randn(2, 32, 17, 17, device="cuda"), torch.randn(2, 32, device="cuda")
    xe = x.clone().requires_grad_(True)
    f, c = enc(xe)
    torch.autograd.backward((f, c), (gf, gc))
    graphed = torch.cuda.make_graphed_callables(enc, (torch.zeros_like(x).requires_grad_(True),))
    for _ in range(2):                                   # replay twice: static buffers are reused
        xg = x.clone().requires_grad_(True)
        f2, c2 = graphed(xg)
        torch.autograd.backward((f2, c2), (gf, gc))
        torch.cuda.synchronize()
        assert torch.equal(f2, f) and torch.equal(c2, c)
        assert torch.allclose(xg.grad, xe.grad, rtol=0, atol=0) or float((xg.grad - xe.grad).abs().max()) < 1e-6 * float(xe.grad.abs().max())


def test_resume_restores_optimizer_state_and_missing_files_raise(tmp_path):
    """trainer.py:137-159 (optimizer state is reloaded on resume) and ADVICE round 1: a wrong DAMSM path or an empty --resume
    directory must raise instead of silently training from random encoders / from scratch."""
    from mogan_amd.attngan import main as entry
    from mogan_amd.attngan.datasets import SyntheticTextDataset
    from mogan_amd.attngan.trainer import TrainEngine, condGANTrainer
    yml = tmp_path / "tiny.yml"
    yml.write_text("CONFIG_NAME: 'tiny'\nDATASET_NAME: 'coco'\nWORKERS: 0\nTREE: {BRANCH_NUM: 3}\n"
                   "GAN: {DF_DIM: 8, GF_DIM: 8, Z_DIM: 100, R_NUM: 1}\n"
                   "TEXT: {EMBEDDING_DIM: 32, CAPTIONS_PER_IMAGE: 5, WORDS_NUM: 6}\n"
                   "TRAIN: {FLAG: True, BATCH_SIZE: 4, MAX_EPOCH: 1, SNAPSHOT_INTERVAL: 1, NET_E: ''}\n")
    out = tmp_path / "out"
    entry.main(["--cfg", str(yml), "--synthetic", "8", "--manualSeed", "7", "--output_dir", str(out)])
    ckpt = sorted(glob.glob(os.path.join(str(out), "Model", "checkpoint_*.pth")))[-1]
    sd = torch.load(ckpt, map_location="cpu", weights_only=False)
    assert set(sd["optimG"]) == {"state", "param_groups"} and float(sd["optimG"]["state"][0]["step"]) == 2.0
    ds = SyntheticTextDataset(8, n_words=100, seed=7)
    dl = torch.utils.data.DataLoader(ds, batch_size=4, drop_last=True)
    algo = condGANTrainer(str(out), dl, 100, ds.ixtoword, resume=str(out))
    te, ie, G, Ds, epoch = algo.build_models()
    assert epoch == 1
    algo.engine = TrainEngine(te, ie, G, Ds)
    optG, optDs = algo.define_optimizers(G, Ds)
    assert float(optG.state[0]) == 2.0 and all(float(o.state[0]) == 2.0 for o in optDs)
    m0 = sd["optimD"][2]["state"][0]["exp_avg"]
    assert torch.equal(optDs[2].m[:m0.numel()].view_as(m0).cpu(), m0) and float(optDs[2].m.abs().sum()) > 0
    # missing files
    empty = tmp_path / "empty"
    algo2 = condGANTrainer(str(empty), dl, 100, ds.ixtoword, resume=str(empty))
    with pytest.raises(FileNotFoundError):
        algo2.build_models()
    cfg.TRAIN.NET_E = str(tmp_path / "no_such_dir" / "text_encoder100.pth")
    try:
        with pytest.raises(FileNotFoundError):
            condGANTrainer(str(out), dl, 100, ds.ixtoword, resume='').build_models()
    finally:
        cfg.TRAIN.NET_E = ''


def _encoder_with_statistics(seed, dim=32):
    from mogan_amd.attngan import model
    cfg.TRAIN.FLAG, cfg.TEXT.EMBEDDING_DIM = True, dim
    torch.manual_seed(seed)
    enc = model.CNN_ENCODER(dim)
    for m in enc.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.05); m.running_var.uniform_(0.8, 1.2); m.weight.data.uniform_(0.9, 1.1)
            m.bias.data.normal_(0, 0.05)
    return enc.eval().cuda()


def test_panel_trunk_blocks_against_the_module_path():
    """inception.PanelTrunk (packed filters, pixel panels, grouped GEMM + tail launches; the pool branch evaluated as 1x1 conv ->
    average pool) block by block against the module-by-module evaluation under autograd, on inputs with exact zeros (the ReLU
    mask of the block input is part of the block's backward).  A ReLU decision that flips at the fp32 noise floor moves a block's
    input gradient by ~2e-4 rel-L2; everything else agrees to fp32 rounding."""
    from mogan_amd.attngan import inception
    enc = _encoder_with_statistics(5)
    pk = inception.PanelTrunk(enc)
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    dims = {"Mixed_5b": (192, 35), "Mixed_5c": (256, 35), "Mixed_5d": (288, 35), "Mixed_6a": (288, 35), "Mixed_6b": (768, 17),
            "Mixed_6c": (768, 17), "Mixed_6d": (768, 17), "Mixed_6e": (768, 17), "Mixed_7a": (768, 17), "Mixed_7b": (1280, 8),
            "Mixed_7c": (2048, 8)}
    B, tight = 3, 0
    for name, kind, fcs in pk.blocks:
        C, H = dims[name]
        x = torch.relu(torch.randn(B, C, H, H, device="cuda"))
        xr = x.clone().requires_grad_(True)
        y = getattr(enc, name)(xr)
        g = torch.randn_like(y)
        (y * g).sum().backward()
        pt = inception._PTape(B, x.device)
        X = inception._PT(B, x.device, [C], H, H, f32=x.clone())
        pt.tail([dict(srcs=[inception._f32src(X.sl(0))], out=X.sl(0), f32=False)])
        O, bwd = pk._block(pt, kind, fcs, X)
        dO = pt.grad(O)
        pt.tail([dict(srcs=[(g.data_ptr(), g.stride(0), 0, 1)], out=dO.whole(), mask=O.whole())])
        dO.written = True
        dX = pt.grad(X)
        bwd(dO, dX)
        torch.cuda.synchronize()
        ey, eg = rel(O.f32, y.detach()), rel(dX.f32, xr.grad * (x > 0))
        assert ey < 5e-6, (name, ey)
        assert eg < 3e-3, (name, eg)
        tight += eg < 5e-6
    assert tight >= 8, tight


def test_panel_trunk_against_the_grouped_trunk():
    """whole frozen trunk, both forms (FrozenTrunk: implicit GEMM on fp32 NCHW; PanelTrunk): outputs to fp32 rounding, image
    gradient within what flipped ReLU / max-pool decisions leave (torch fp32 vs fp64 of the restatement differ by 1e-2 there)"""
    from mogan_amd.attngan import inception
    enc = _encoder_with_statistics(7)
    B = 3
    x = torch.rand(B, 3, 299, 299, device="cuda") * 2 - 1
    gf, gl = torch.randn(B, 768, 17, 17, device="cuda"), torch.randn(B, 2048, 8, 8, device="cuda")
    ft, pk = inception.FrozenTrunk(enc), inception.PanelTrunk(enc)
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    tp, f0, l0 = ft.forward(x)
    g0 = ft.backward(tp, gf, gl)
    tapes, f1, l1 = pk.forward(x)
    g1 = pk.backward(tapes, gf, gl)
    assert rel(f1, f0) < 5e-6 and rel(l1, l0) < 5e-6, (rel(f1, f0), rel(l1, l0))
    assert rel(g1, g0) < 2e-2, rel(g1, g0)
    # one output's gradient absent (None -> zeros), as autograd hands it over when only one output is used
    tapes, _, _ = pk.forward(x)
    g2 = pk.backward(tapes, gf, None)
    tp, _, _ = ft.forward(x)
    g3 = ft.backward(tp, gf, None)
    assert rel(g2, g3) < 2e-2, rel(g2, g3)
