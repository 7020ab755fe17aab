"""-m gpu: all eight checkpoint scores of attngan/evaluate.SCORES from ONE pass (CheckpointEvaluation.run_scores through main.py) on
the 12-image synthetic split: every file byte-equal to the same flag run alone, the generator and the trunk run as often and at the
batch sizes they ran at before the scores were put into one table, and run_scores called directly returns what the methods return."""
import os
import shutil

import pytest
import torch

from eval_setup import tiny_checkpoint as _tiny_checkpoint
from helpers import load_pkg

load_pkg()
from mogan_amd.attngan.evaluate import SCORES  # noqa: E402

pytestmark = pytest.mark.gpu

# How often the generator (G_NET.forward) and the trunk (CNN_ENCODER.pool_code) run, every call at the batch size 4: measured ONCE, with
# the wrappers below and the flags below, on the commit before run_scores existed (main.py's hand-written shared block; ccdcdd1), and
# recorded with the files' digests in profiles/eval_scores_refactor_ab.json.  All eight, the bank not yet on disk: 3 batches and
# their 3 resampled ones; 3 real + 3 generated batches, 16 batches of object crops, 3 batches of the training bank.  Alone: the
# object crops and the generated images only (scene_fid), no trunk (swd, msssim, spectrum), both sides (the others; the bank loaded).
CALLS_TOGETHER = (6, 25)
CALLS_ALONE = {"scene_fid": (3, 19), "swd": (3, 0), "msssim": (6, 0), "spectrum": (3, 0), "fid": (3, 6), "kid": (3, 6), "prdc": (3, 6),
               "memorisation": (3, 6)}


def _files(valid):
    return {name: open(os.path.join(valid, name), "rb").read() for name in sorted(os.listdir(valid))}


def test_all_eight_scores_in_one_pass_keep_their_bytes_and_the_passes_their_calls(tmp_path, monkeypatch):
    from mogan_amd.attngan import main as entry
    from mogan_amd.attngan import model
    from mogan_amd.attngan.datasets import SyntheticTextDataset
    from mogan_amd.attngan.trainer import condGANTrainer
    cfg, ev, ckpt = _tiny_checkpoint(tmp_path)
    calls = {"netG": [], "pool_code": []}
    forward, pool_code = model.G_NET.forward, model.CNN_ENCODER.pool_code

    def counted_forward(self, noise, *args, **kw):
        calls["netG"].append(int(noise.shape[0]))
        return forward(self, noise, *args, **kw)

    def counted_pool_code(self, x):
        calls["pool_code"].append(int(x.shape[0]))
        return pool_code(self, x)
    monkeypatch.setattr(model.G_NET, "forward", counted_forward)
    monkeypatch.setattr(model.CNN_ENCODER, "pool_code", counted_pool_code)

    def counted():
        got = (len(calls["netG"]), len(calls["pool_code"]))
        assert set(calls["netG"]) | set(calls["pool_code"]) <= {4}
        del calls["netG"][:], calls["pool_code"][:]
        return got
    try:
        base = ["--cfg", str(ev), "--synthetic", "12", "--manualSeed", "7", "--output_dir", str(tmp_path), "--swd_patches", "16",
                "--swd_dirs", "16", "--swd_repeats", "2", "--msssim_scales", "3", "--nn_k", "2", "--nn_show", "3",
                "--nn_bank", str(tmp_path / "bank.npz")]
        valid = os.path.join(ckpt[:-4], "valid")
        entry.main(base + ["--" + name for name in SCORES])
        assert counted() == CALLS_TOGETHER
        together = _files(valid)
        assert sorted(together) == sorted([name + ".json" for name in SCORES] + ["nn_grid.png"])
        for name in SCORES:
            shutil.rmtree(valid)
            entry.main(base + ["--" + name])
            assert counted() == CALLS_ALONE[name], name
            alone = _files(valid)
            assert sorted(alone) == [name + ".json"] + ["nn_grid.png"] * (name == "memorisation"), name
            for n, data in alone.items():
                assert data == together[n], "%s differs between --%s alone and all eight flags" % (n, name)
        # run_scores directly, on the trainer main.py builds: an images score and a codes score from one pass
        ds = SyntheticTextDataset(12, seed=7, eval=False)
        dl = torch.utils.data.DataLoader(ds, batch_size=cfg.TRAIN.BATCH_SIZE, drop_last=True, shuffle=True, num_workers=0)
        algo = condGANTrainer(str(tmp_path), dl, ds.n_words, ds.ixtoword, '', distributed=False)
        both = algo.run_scores("test", {"spectrum": dict(window="hann"), "fid": {}}, seed=7)
        assert counted() == (3, 6) and list(both) == ["spectrum", "fid"]
        assert {n: _files(valid)[n] for n in ("spectrum.json", "fid.json")} == {n: together[n] for n in ("spectrum.json", "fid.json")}
        assert both == {"spectrum": algo.spectrum("test", seed=7, window="hann"), "fid": algo.fid("test", seed=7)}
        assert counted() == (6, 6)
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.FLAG = '', True
