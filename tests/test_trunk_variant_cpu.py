"""The trunk variant "fid"  where no GPU is needed: the attribute and its refusals, the digest's recipe, the
command line's refusals, the tail's new rejections (answered by the host before any HIP call), the reader of published mu / sigma
statistics, and the fp64 restatement the GPU tests compare with -- tied to the pinned oracle in its "torchvision" form and shown to
tell the two networks apart on the GPU test's own seeds."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

import trunk_variant_cases as V
from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import fid as F  # noqa: E402
from mogan_amd.attngan import inception, model  # noqa: E402
from mogan_amd.hip import lib  # noqa: E402


@pytest.fixture(scope="module")
def enc():
    return V.encoder()


def test_set_trunk_variant_and_its_refusals(enc):
    assert model.CNN_ENCODER.trunk_variant == "torchvision" and enc.trunk_variant == "torchvision"
    assert "trunk_variant" not in enc.state_dict() and inception.VARIANTS == ("torchvision", "fid")
    with pytest.raises(ValueError, match="tf"):
        enc.set_trunk_variant("tf")
    assert enc.trunk_variant == "torchvision"
    x = torch.zeros(1, 3, 8, 8)
    enc.set_trunk_variant("fid")
    try:
        assert enc._frozen()
        with torch.enable_grad(), pytest.raises(RuntimeError, match="forward only"):
            enc._trunk_walk(x.clone().requires_grad_(True))                     # a gradient is asked for
        enc.train()
        with torch.no_grad(), pytest.raises(RuntimeError, match="frozen fast path"):
            enc._trunk_walk(x)                                                  # not _frozen(): training mode
        enc.eval()
        p = enc.Mixed_7c.branch_pool.conv.weight
        p.requires_grad = True
        with torch.no_grad(), pytest.raises(RuntimeError, match="frozen fast path"):
            enc.pool_code(x)                                                    # not _frozen(): a trunk parameter asks for a gradient
        p.requires_grad = False
    finally:
        enc.eval()
        enc.set_trunk_variant("torchvision")


def test_the_other_trunks_say_that_they_do_not_know_the_variant(enc, monkeypatch):
    """FrozenTrunk (PANEL_TRUNK False) raises before it builds or launches anything; an unknown name never reaches a trunk"""
    monkeypatch.setattr(inception, "PANEL_TRUNK", False)
    enc.set_trunk_variant("fid")
    try:
        with pytest.raises(RuntimeError, match="panel trunk only"):
            inception.frozen_trunk(enc, torch.zeros(1, 3, 299, 299))
    finally:
        enc.set_trunk_variant("torchvision")


def _recipe(encoder, first=b""):
    h = hashlib.sha256()
    h.update(first)
    for name, t in encoder.state_dict().items():
        if name.split(".")[0] in ("emb_features", "emb_cnn_code"):
            continue
        a = t.detach().cpu().contiguous().numpy()
        h.update(("%s %s %s\n" % (name, a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def test_the_digest_is_the_documented_recipe_and_names_another_variant(enc):
    default = F.trunk_digest(enc)
    assert default == _recipe(enc)
    enc.set_trunk_variant("fid")
    try:
        other = F.trunk_digest(enc)
    finally:
        enc.set_trunk_variant("torchvision")
    assert other != default and other == _recipe(enc, b"trunk_variant fid\n")
    assert F.trunk_digest(enc) == default


def test_the_command_line_refuses(capsys):
    from mogan_amd.attngan import main as entry
    for argv, word in ((["--fid", "--trunk_variant", "fid"], "--trunk"),
                       (["--r_precision", "--trunk", "f.pth", "--trunk_variant", "fid"], "--r_precision"),
                       (["--sampling", "--trunk", "f.pth", "--trunk_variant", "fid"], "pool codes"),
                       (["--fid", "--trunk", "f.pth", "--trunk_variant", "tf"], "invalid choice")):
        with pytest.raises(SystemExit) as e:
            entry.parse_args(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv
    args = entry.parse_args(["--fid", "--kid", "--trunk", "f.pth", "--trunk_variant", "fid"])
    assert args.trunk_variant == "fid" and entry.parse_args(["--fid"]).trunk_variant == "torchvision"
    from mogan_amd.attngan import pretrain_DAMSM as P
    with pytest.raises(SystemExit):
        P.parse_args(["--trunk_variant", "fid"])                                # DAMSM pre-training has no such flag
    capsys.readouterr()


def test_the_trainer_refuses_a_variant_without_a_file_and_r_precision_under_it(tmp_path):
    from mogan_amd.attngan.evaluate import CheckpointEvaluation
    from mogan_amd.attngan.miscc.config import cfg
    from mogan_amd.attngan.trainer import condGANTrainer
    with pytest.raises(ValueError, match="needs `trunk`"):
        condGANTrainer(str(tmp_path), [], 10, {}, '', trunk_variant="fid")
    with pytest.raises(ValueError, match="unknown trunk variant"):
        condGANTrainer(str(tmp_path), [], 10, {}, '', trunk="f.pth", trunk_variant="tf")

    class Evaluation(CheckpointEvaluation):
        trunk_path, trunk_variant = "f.pth", "fid"
    kept = cfg.TRAIN.NET_G
    cfg.TRAIN.NET_G = str(tmp_path / "netG.pth")
    try:
        with pytest.raises(ValueError, match="DAMSM heads"):
            Evaluation().r_precision("test")
    finally:
        cfg.TRAIN.NET_G = kept


def test_beside_a_net_e_the_variant_replaces_the_pairs_trunk(tmp_path, capsys):
    """the default refuses a file of another trunk beside NET_E's pair; "fid" loads the pair (its draws and file errors stay), then
    the file's trunk over it, and sets the variant; a 1008-way head under the default prints one line naming the flag"""
    from mogan_amd.attngan.evaluate import CheckpointEvaluation
    from mogan_amd.attngan.miscc.config import cfg

    class Evaluation(CheckpointEvaluation):
        device = torch.device("cpu")

        def __init__(self, trunk_path=None, variant=None):
            self.trunk_path = trunk_path
            if variant:
                self.trunk_variant = variant

    torch.manual_seed(5)
    pair = Evaluation()._new_image_encoder()
    torch.manual_seed(6)
    other = model.CNN_ENCODER(256)
    state = dict(inception.trunk_entries(other))
    state.update({"fc.weight": torch.zeros(1008, 2048), "fc.bias": torch.zeros(1008)})
    another = str(tmp_path / "pt_inception.pth")
    torch.save(state, another)
    torch.save({}, str(tmp_path / "text_encoder100.pth"))
    torch.save(pair.state_dict(), str(tmp_path / "image_encoder100.pth"))
    kept = cfg.TRAIN.NET_E
    try:
        cfg.TRAIN.NET_E = str(tmp_path / "text_encoder100.pth")
        with pytest.raises(ValueError, match="one pass runs under one trunk"):
            Evaluation(another)._load_image_encoder()
        torch.manual_seed(9)
        plain = Evaluation()._load_image_encoder()
        after = torch.get_rng_state()
        torch.manual_seed(9)
        capsys.readouterr()
        loaded = Evaluation(another, "fid")._load_image_encoder()
        assert "--trunk_variant fid" not in capsys.readouterr().out
        assert torch.equal(torch.get_rng_state(), after)                        # the draws of a seeded pass stay
        assert loaded.trunk_variant == "fid" and plain.trunk_variant == "torchvision"
        other.set_trunk_variant("fid")
        assert F.trunk_digest(loaded) == F.trunk_digest(other) != F.trunk_digest(plain)
        for k in ("emb_features.weight", "emb_cnn_code.weight", "emb_cnn_code.bias"):
            assert torch.equal(loaded.state_dict()[k], pair.state_dict()[k]), k
        (tmp_path / "image_encoder100.pth").unlink()
        with pytest.raises(FileNotFoundError):                                  # the pair's file errors stay
            Evaluation(another, "fid")._load_image_encoder()
        # the default variant without a NET_E: the file loads as ever, and one line names the flag
        cfg.TRAIN.NET_E = ''
        ev = Evaluation(another)
        capsys.readouterr()
        ev._load_image_encoder()
        ev._load_image_encoder()
        text = capsys.readouterr().out
        assert text.count("--trunk_variant fid") == 1 and "1008" in text
    finally:
        cfg.TRAIN.NET_E = kept


# ---------------------------------------------------------------------------------------------- the tail's rejections, on the host
PTR = 256          # non-null, never dereferenced: every case below is answered before any HIP call


def _tail(box, nsrc=1, nsplit=1):
    a = lib.TailArgs()
    for j in range(nsrc):
        a.src[j], a.src_bs[j], a.src_slab[j], a.src_nsplit[j] = PTR, 40 * 64, 3 * 40 * 64, nsplit
    a.nsrc, a.B, a.n, a.H, a.W, a.box, a.dst, a.dst_bs = nsrc, 3, 40, 8, 8, box, PTR, 40 * 64
    arr = (lib.TailArgs * 1)(a)
    return lib.load().mogan_panel_tail_group(1, ctypes.cast(arr, ctypes.c_void_p), ctypes.c_void_p(None))


@pytest.mark.parametrize("case", [(4, 1, 1), (-1, 1, 1), (7, 1, 1), (3, 2, 1), (3, 1, 2), (3, 3, 1)],
                         ids=lambda c: "box%d_src%d_slabs%d" % c)
def test_the_tail_rejects_before_any_launch(case):
    assert _tail(*case) == -1                                                   # MOGAN_ERR_SHAPE


# ------------------------------------------------------------------------------------------- published real-side statistics (mu, sigma)
def _npz(path, **arrays):
    with open(path, "wb") as f:
        np.savez(f, **arrays)
    return str(path)


def test_the_reader_of_published_statistics(tmp_path):
    rng = np.random.RandomState(4)
    D = 6
    a = rng.standard_normal((D, D))
    mu, sigma = rng.standard_normal(D).astype(np.float32), (a @ a.T).astype(np.float32)
    sigma = (sigma + sigma.T) / 2
    good = _npz(tmp_path / "good.npz", mu=mu, sigma=sigma)
    assert F.is_external_stats(good)
    m, s = F.load_external_stats(good, D)
    assert m.dtype == s.dtype == torch.float64 and tuple(m.shape) == (D,) and tuple(s.shape) == (D, D)
    assert np.array_equal(m.numpy(), mu.astype(np.float64)) and np.array_equal(s.numpy(), sigma.astype(np.float64))
    # the project's own format is not such a file, nor is one with a third array
    own = str(tmp_path / "own.npz")
    F.FeatureStats(m, s, 5, "0" * 64).save(own)
    assert not F.is_external_stats(own) and not F.is_external_stats(str(tmp_path / "missing.npz"))
    extra = _npz(tmp_path / "extra.npz", mu=mu, sigma=sigma, n=np.int64(3))
    assert not F.is_external_stats(extra)
    with pytest.raises(ValueError, match="extra.npz.*exactly mu and sigma"):
        F.load_external_stats(extra, D)
    bad = sigma.copy()
    bad[0, 1] += 0.5
    nan = mu.copy()
    nan[2] = np.nan
    inf = sigma.copy()
    inf[1, 1] = np.inf
    for name, arrays, D_, word in (("width", dict(mu=mu, sigma=sigma), D + 1, "width"),
                                   ("shape", dict(mu=mu, sigma=sigma[:, :4]), D, "width"),
                                   ("nan", dict(mu=nan, sigma=sigma), D, "non-finite values in mu"),
                                   ("inf", dict(mu=mu, sigma=inf), D, "non-finite values in sigma"),
                                   ("asym", dict(mu=mu, sigma=bad), D, "not symmetric"),
                                   ("text", dict(mu=np.array(["a"] * D), sigma=sigma), D, "numbers expected")):
        path = _npz(tmp_path / (name + ".npz"), **arrays)
        with pytest.raises(ValueError, match="%s.npz.*%s" % (name, word)):
            F.load_external_stats(path, D_)


# ------------------------------------------------------------------------------------------------------- the fp64 restatement
def test_the_restatement_is_the_pinned_oracle_in_its_torchvision_form(enc):
    from oracle import inception_oracle as IO
    sd = {k: v.detach().clone().double() for k, v in enc.state_dict().items()}
    x = V.images(1, 64, seed=5).double()
    with torch.no_grad():
        feat, code = V.restated(sd, x, "torchvision")
        f_ref, c_ref = IO.cnn_encoder(sd, x)
        want_f = torch.nn.functional.conv2d(feat, sd["emb_features.weight"])
        want_c = torch.nn.functional.linear(code, sd["emb_cnn_code.weight"], sd["emb_cnn_code.bias"])
        # and the trunk itself, not only what the heads let through
        t_feat, t_last = IO.trunk(sd, torch.nn.functional.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False))
    figures = [V.rel_l2(want_f, f_ref), V.rel_l2(want_c, c_ref), V.rel_l2(feat, t_feat), V.rel_l2(code, t_last.mean(dim=(2, 3)))]
    print("restatement against the oracle, rel-L2: %s" % ", ".join("%.2e" % f for f in figures))
    assert max(figures) < 1e-12, figures                                        # fp64 rounding over 94 layers


def test_the_two_networks_are_far_apart_on_the_gpu_tests_seeds():
    ref = V.references()
    for i, what in enumerate(("Mixed_6e map", "pool code")):
        apart = V.rel_l2(ref["fid"][i], ref["torchvision"][i])
        print("%s: fid against torchvision rel-L2 %.3e = %.0f x the GPU tolerance %.0e" % (what, apart, apart / V.TOL, V.TOL))
        assert apart >= V.APART, (what, apart)
