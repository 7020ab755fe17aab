"""-m gpu: the trunk variant "fid"  on the device.

Trunk level: a random-init CNN_ENCODER with non-trivial BatchNorm statistics on two 64 x 64 images, the Mixed_6e map and the pool code
against the fp64 restatement of tests/trunk_variant_cases.py (which takes no arithmetic from the code under test and is tied to the
pinned oracle by tests/test_trunk_variant_cpu.py) with rel-L2 < 2e-5 -- the figure test_cnn_encoder_vs_cpu_restatement holds for the
torchvision trunk --, more than 100 times that away from the torchvision run of the same weights, the same bits from two calls, and
the default variant's bits unchanged by a round trip through the other one (the cache key).

End to end, on eval_setup's tiny checkpoint under a synthetic trunk file: main.py --trunk F --trunk_variant fid for the scores on
pool codes, the JSON's variant key and digest, the same bytes twice, today's key set without the flag, the Inception Score under the
file's head, a NET_E whose pair holds another trunk, statistics files of one variant refused under the other, and published mu / sigma
statistics as the real side."""
import json
import os

import numpy as np
import pytest
import torch

import trunk_variant_cases as V
from eval_setup import tiny_checkpoint as _tiny_checkpoint
from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import fid as FID  # noqa: E402
from mogan_amd.attngan import inception, model  # noqa: E402
from mogan_amd.attngan.datasets import SyntheticTextDataset  # noqa: E402

pytestmark = pytest.mark.gpu
FID_KEYS = {"fid", "mean_sq", "tr_s1", "tr_s2", "tr_sqrt", "n_real", "n_fake", "trunk_digest", "seed", "NET_G", "NET_E", "note"}


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def test_the_fid_trunk_against_its_fp64_restatement_and_apart_from_torchvisions():
    ref = V.references()
    enc = V.encoder().cuda()
    x = V.images().cuda()
    with torch.no_grad():
        tv = [t.clone() for t in enc._trunk_walk(x)]
        enc.set_trunk_variant("fid")
        got = [t.clone() for t in enc._trunk_walk(x)]
        again = [t.clone() for t in enc._trunk_walk(x)]
        trunk = enc._frozen_trunk
        assert isinstance(trunk, inception.PanelTrunk) and trunk.variant == "fid" and trunk.box == 2
        assert [n for n, _, f in trunk.blocks if "pool" in f] == ["Mixed_7c"]
        enc.set_trunk_variant("torchvision")
        back = [t.clone() for t in enc._trunk_walk(x)]
    torch.cuda.synchronize()
    assert tuple(got[0].shape) == (2, 768, 17, 17) and tuple(got[1].shape) == (2, 2048)
    for i, what in enumerate(("Mixed_6e map", "pool code")):
        rel, rel_tv = V.rel_l2(got[i], ref["fid"][i]), V.rel_l2(tv[i], ref["torchvision"][i])
        apart = V.rel_l2(got[i], tv[i].cpu().double())
        print("%s: fid against fp64 rel-L2 %.2e (torchvision's %.2e), fid against the torchvision run %.2e"
              % (what, rel, rel_tv, apart))
        assert rel < V.TOL, (what, rel)
        assert rel_tv < V.TOL, (what, rel_tv)
        assert apart > V.APART, (what, apart)
        assert torch.equal(_bits(got[i]), _bits(again[i])), what + ": two calls differ"
        assert torch.equal(_bits(tv[i]), _bits(back[i])), what + ": the default changed after a round trip through the variant"


def test_a_variant_tape_has_no_backward():
    enc = V.encoder().cuda().set_trunk_variant("fid")
    trunk = inception.PanelTrunk(enc, "fid")
    with torch.no_grad():
        tapes, feats, last = trunk.forward(torch.zeros(1, 3, 299, 299, device="cuda"))
    with pytest.raises(RuntimeError, match="forward only"):
        trunk.backward(tapes, None, torch.zeros_like(last))
    with pytest.raises(ValueError, match="unknown trunk variant"):
        inception.PanelTrunk(enc, "tf")


# ------------------------------------------------------------------------------------------------------------------- end to end
def _main_trainer(tmp_path, trunk=None, variant=None, seed=7, length=12):
    """the trainer main.py builds for --synthetic 12 --manualSeed 7 under the tiny config"""
    from mogan_amd.attngan.miscc.config import cfg
    from mogan_amd.attngan.trainer import condGANTrainer
    ds = SyntheticTextDataset(length, seed=seed, eval=False)
    dl = torch.utils.data.DataLoader(ds, batch_size=cfg.TRAIN.BATCH_SIZE, drop_last=True, shuffle=True, num_workers=0)
    extra = {"trunk": trunk} if trunk else {}
    if variant:
        extra["trunk_variant"] = variant
    return condGANTrainer(str(tmp_path), dl, ds.n_words, ds.ixtoword, '', distributed=False, **extra)


def test_fid_and_kid_through_main_under_the_variant(tmp_path, capsys):
    from mogan_amd.attngan import main as entry
    cfg, ev, ckpt = _tiny_checkpoint(tmp_path)
    trunk = str(tmp_path / "trunk.pth")
    V.trunk_file(trunk)
    stats = {v: str(tmp_path / ("stats_%s.npz" % v)) for v in V.VARIANTS}
    try:
        base = ["--cfg", str(ev), "--synthetic", "12", "--manualSeed", "7", "--output_dir", str(tmp_path), "--fid", "--kid",
                "--kid_subsets", "4", "--kid_subset_size", "6", "--trunk", trunk]
        paths = {k: os.path.join(ckpt[:-4], "valid", k + ".json") for k in ("fid", "kid")}
        entry.main(base + ["--trunk_variant", "fid", "--fid_stats", stats["fid"]])
        first = {k: open(p, "rb").read() for k, p in paths.items()}
        out = {k: json.loads(v) for k, v in first.items()}
        # the codes of a pass of the caller's own, from an encoder set to the variant: the digest and the codes themselves
        algo = _main_trainer(tmp_path, trunk, "fid")
        seen = []
        handed = algo.pool_codes("test", seed=7, image_sink=lambda r, f, take: seen.append((r[:take].clone(), f[:take].clone())))
        kept = cfg.TRAIN.FLAG
        cfg.TRAIN.FLAG = True
        enc = model.CNN_ENCODER(32)
        cfg.TRAIN.FLAG = kept
        enc.load_trunk_file(trunk)
        for p_ in enc.parameters():
            p_.requires_grad = False
        enc = enc.cuda().eval().set_trunk_variant("fid")
        assert FID.trunk_digest(enc) == handed["trunk_digest"]
        for k in ("fid", "kid"):
            assert out[k]["trunk_variant"] == "fid" and out[k]["trunk_digest"] == handed["trunk_digest"], k
            for word in ("published FID Inception network", "not quantised to 8 bits", "resize"):
                assert word in out[k]["note"], (k, word)
        assert set(out["fid"]) == FID_KEYS | {"trunk_variant"}
        plain_enc = _main_trainer(tmp_path, trunk)._load_seeded(7)[2]
        assert plain_enc.trunk_variant == "torchvision" and FID.trunk_digest(plain_enc) != handed["trunk_digest"]
        assert len(seen) == 3 and handed["n"] == 12
        with torch.no_grad():
            for i, side in enumerate(("real", "fake")):
                want = torch.cat([enc.pool_code(batch[i]) for batch in seen])
                assert torch.equal(_bits(handed[side][:12]), _bits(want)), "the %s codes are not pool_code's under the variant" % side
        # the handed-over codes write the same bytes, and so does a second run
        for p in paths.values():
            os.remove(p)
        algo.fid("test", seed=7, codes=handed, stats_path=stats["fid"])
        assert open(paths["fid"], "rb").read() == first["fid"]
        entry.main(base + ["--trunk_variant", "fid", "--fid_stats", stats["fid"]])
        assert {k: open(p, "rb").read() for k, p in paths.items()} == first
        # without the flag: today's key set, another digest, other figures -- and the other variant's statistics are refused
        entry.main(base + ["--fid_stats", stats["torchvision"]])
        tv = json.load(open(paths["fid"]))
        assert set(tv) == FID_KEYS and tv["trunk_digest"] != out["fid"]["trunk_digest"] and tv["fid"] != out["fid"]["fid"]
        assert "trunk_variant" not in json.load(open(paths["kid"]))
        with pytest.raises(ValueError, match="another Inception trunk"):
            entry.main(base + ["--fid_stats", stats["fid"]])
        with pytest.raises(ValueError, match="another Inception trunk"):
            entry.main(base + ["--trunk_variant", "fid", "--fid_stats", stats["torchvision"]])
        # published statistics (mu, sigma): the real side under "fid" only, never written
        own = FID.FeatureStats.load(stats["fid"], out["fid"]["trunk_digest"], 2048)
        mu, sigma = own.mean, own.cov
        ext = str(tmp_path / "published.npz")
        with open(ext, "wb") as f:
            np.savez(f, mu=mu.numpy(), sigma=sigma.numpy())
        before = open(ext, "rb").read()
        got = algo.fid("test", seed=7, codes=handed, stats_path=ext)
        assert got["real_stats"] == "external" and got["n_real"] is None and got["n_fake"] == 12 and "unverified" in got["note"]
        assert got["fid"] == out["fid"]["fid"] and open(ext, "rb").read() == before
        assert json.load(open(paths["fid"]))["n_real"] is None
        with pytest.raises(ValueError, match="--trunk_variant fid only"):
            _main_trainer(tmp_path, trunk).fid("test", seed=7, stats_path=ext)
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.FLAG = '', True


def test_inception_score_under_the_variant_takes_the_files_head(tmp_path):
    from mogan_amd.attngan import inception_score as IS
    from mogan_amd.attngan import main as entry
    cfg, ev, ckpt = _tiny_checkpoint(tmp_path)
    trunk = str(tmp_path / "trunk.pth")
    w, b = V.trunk_file(trunk)
    try:
        entry.main(["--cfg", str(ev), "--synthetic", "12", "--manualSeed", "7", "--output_dir", str(tmp_path), "--inception_score",
                    "--trunk", trunk, "--trunk_variant", "fid", "--is_splits", "3"])
        out = json.load(open(os.path.join(ckpt[:-4], "valid", "inception_score.json")))
        assert out["trunk_variant"] == "fid" and out["classes"] == 7 and out["head"] == trunk
        assert out["head_digest"] == IS.head_digest(w, b) and "published FID Inception network" in out["note"]
        assert "not verified" not in out["note"]                                # the file's own trunk, under the variant's digest
        algo = _main_trainer(tmp_path, trunk, "fid")
        handed = algo.pool_codes("test", seed=7, want_real=False)
        assert out["trunk_digest"] == handed["trunk_digest"]
        path = os.path.join(ckpt[:-4], "valid", "inception_score.json")
        first = open(path, "rb").read()
        os.remove(path)
        algo.inception_score("test", seed=7, splits=3, codes=handed)           # the variant's codes handed over: the same bytes
        assert open(path, "rb").read() == first
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.FLAG = '', True


def test_beside_a_net_e_of_another_trunk_the_variant_runs_and_the_images_stay(tmp_path):
    cfg, ev, ckpt = _tiny_checkpoint(tmp_path)
    trunk = str(tmp_path / "trunk.pth")
    V.trunk_file(trunk)
    try:
        torch.manual_seed(51)
        torch.save(model.RNN_ENCODER(_main_trainer(tmp_path).n_words, nhidden=32).state_dict(), str(tmp_path / "text_encoder9.pth"))
        pair = _main_trainer(tmp_path)._new_image_encoder()
        torch.save(pair.state_dict(), str(tmp_path / "image_encoder9.pth"))
        cfg.TRAIN.NET_E = str(tmp_path / "text_encoder9.pth")
        seen = {}

        def sink(name):
            seen[name] = []
            return lambda r, f, take: seen[name].append(f[:take].clone())
        with pytest.raises(ValueError, match="one pass runs under one trunk"):
            _main_trainer(tmp_path, trunk).pool_codes("test", seed=7)
        under = _main_trainer(tmp_path, trunk, "fid").pool_codes("test", seed=7, image_sink=sink("fid"))
        plain = _main_trainer(tmp_path).pool_codes("test", seed=7, image_sink=sink("plain"))
        ours, theirs = torch.cat(seen["fid"]), torch.cat(seen["plain"])
        assert tuple(ours.shape) == (12, 3, 256, 256) and torch.equal(_bits(ours), _bits(theirs))
        assert under["trunk_digest"] != plain["trunk_digest"] and not torch.equal(under["fake"], plain["fake"])
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.NET_E, cfg.TRAIN.FLAG = '', '', True
