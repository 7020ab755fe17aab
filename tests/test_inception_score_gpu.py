"""-m gpu: the Inception Score end to end -- on eval_setup's tiny checkpoint over 12 synthetic images, under a
synthetic trunk file in torchvision's layout with a head of 7 classes, through attngan/main.py and directly: the JSON against the numpy
definition on the codes read back, the same bytes from a second run and from handed-over codes, the real side, the lowering of the
splits, the head's errors, and the generated images under --trunk bit for bit those without it.

The tolerance of the definition's comparison is inception_score_cases.score_bounds -- the kernel's bound carried through to log IS --
for both sides; no bound here comes from the code under test."""
import json
import os

import numpy as np
import pytest
import torch

import inception_score_cases as C
from eval_setup import tiny_checkpoint as _tiny_checkpoint
from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import inception_score as IS  # noqa: E402
from mogan_amd.attngan.datasets import SyntheticTextDataset  # noqa: E402

pytestmark = pytest.mark.gpu
CLASSES = 7
KEYS = {"inception_score", "inception_score_std", "per_split", "inception_score_all", "splits", "classes", "head_digest", "head",
        "n_real", "n_fake", "trunk_digest", "seed", "NET_G", "NET_E", "note"}


def _main_trainer(tmp_path, trunk=None, seed=7, length=12):
    """the trainer main.py builds for --synthetic 12 --manualSeed 7 under the tiny config"""
    from mogan_amd.attngan.miscc.config import cfg
    from mogan_amd.attngan.trainer import condGANTrainer
    ds = SyntheticTextDataset(length, seed=seed, eval=False)
    dl = torch.utils.data.DataLoader(ds, batch_size=cfg.TRAIN.BATCH_SIZE, drop_last=True, shuffle=True, num_workers=0)
    extra = {"trunk": trunk} if trunk else {}
    return condGANTrainer(str(tmp_path), dl, ds.n_words, ds.ixtoword, '', distributed=False, **extra)


def _files(tmp_path):
    """a trunk file in torchvision's layout with a head of CLASSES classes, the same head alone, another trunk with the same head,
    and the trunk without any head: (paths, weight, bias)"""
    from mogan_amd.attngan import inception, model
    rng = np.random.RandomState(31)
    w = torch.from_numpy((rng.standard_normal((CLASSES, 2048)) * 0.05).astype(np.float32))
    b = torch.from_numpy((rng.standard_normal(CLASSES) * 0.5).astype(np.float32))
    paths = {k: str(tmp_path / ("%s.pth" % k)) for k in ("trunk", "head_only", "other_trunk", "headless")}
    for name, seed in (("trunk", 41), ("other_trunk", 42)):
        torch.manual_seed(seed)
        state = {k: v.clone() for k, v in inception.trunk_entries(model.CNN_ENCODER(256)).items()}
        if name == "trunk":
            torch.save(dict(state), paths["headless"])
        state.update({"fc.weight": w, "fc.bias": b, "AuxLogits.fc.bias": torch.zeros(CLASSES),
                      "Conv2d_1a_3x3.bn.num_batches_tracked": torch.tensor(3)})
        torch.save(state, paths[name])
    torch.save({"fc.weight": w, "fc.bias": b}, paths["head_only"])
    return paths, w.numpy(), b.numpy()


def _tolerances(codes, w, b, S):
    """(per split (S,), all rows) absolute tolerances of IS_s against the numpy definition on `codes`"""
    lse, h, p = IS.row_sums(codes, w, b)
    z = codes.astype(np.float64) @ w.astype(np.float64).T + b.astype(np.float64)
    A, R = C.logit_scale(codes, w, b), z.max(axis=1) - z.min(axis=1)
    n, D = codes.shape
    out = []
    for splits in (S, 1):
        psum = IS.split_sums(p, n, splits)
        figures = np.array(IS.from_sums(h, psum, n)["per_split"])
        out.append(C.BOTH_SIDES * C.score_bounds(D, w.shape[0], A, R, lse, h, psum, splits) * figures)
    return out[0], float(out[1][0])


def _marginal_bound(codes, w, b):
    """the relative bound, for both sides, of the all-row marginal psum / n of `codes`"""
    lse, h, p = IS.row_sums(codes, w, b)
    z = codes.astype(np.float64) @ w.astype(np.float64).T + b.astype(np.float64)
    psum = IS.split_sums(p, codes.shape[0], 1)
    bound = C.bounds(codes.shape[1], w.shape[0], C.logit_scale(codes, w, b), z.max(axis=1) - z.min(axis=1), lse, h, psum, 1)["psum"]
    return C.BOTH_SIDES * float((bound / psum).max()) + C.U


def _against_the_definition(out, codes, w, b, S):
    want = IS.score(codes, w, b, S)
    per_split, whole = _tolerances(codes, w, b, S)
    assert out["splits"] == want["splits"] == S and len(out["per_split"]) == S
    worst = 0.0
    for got, ref, tol in zip(out["per_split"], want["per_split"], per_split):
        worst = max(worst, abs(got - ref) / tol)
        assert abs(got - ref) <= tol, (got, ref, tol)
    tol = float(per_split.max())
    assert abs(out["inception_score"] - want["inception_score"]) <= tol
    assert abs(out["inception_score_std"] - want["inception_score_std"]) <= 2 * tol        # a standard deviation is 1-Lipschitz per value
    assert abs(out["inception_score_all"] - want["inception_score_all"]) <= whole
    worst = max(worst, abs(out["inception_score_all"] - want["inception_score_all"]) / whole)
    print("the figures use %.4f of their tolerance at the most (per split %.3e)" % (worst, tol))


def test_inception_score_through_main_directly_and_from_handed_over_codes(tmp_path, capsys):
    from mogan_amd.attngan import main as entry
    cfg, ev, ckpt = _tiny_checkpoint(tmp_path)
    paths, w, b = _files(tmp_path)
    try:
        base = ["--cfg", str(ev), "--synthetic", "12", "--manualSeed", "7", "--output_dir", str(tmp_path), "--inception_score",
                "--trunk", paths["trunk"], "--is_splits", "3", "--is_real"]
        path = os.path.join(ckpt[:-4], "valid", "inception_score.json")
        entry.main(base)                                                                     # 1: through main.py
        first = open(path, "rb").read()
        os.remove(path)
        capsys.readouterr()
        algo = _main_trainer(tmp_path, paths["trunk"])
        out, codes = algo.inception_score("test", seed=7, splits=3, real=True, return_codes=True)        # 2: directly -- the same bytes
        text = capsys.readouterr().out
        assert open(path, "rb").read() == first and json.loads(first) == json.loads(json.dumps(out))
        assert "Inception Score (12 generated images, 7 classes, 3 splits): " in text and "inception_score.json" in text
        assert set(out) == KEYS | {"real", "kl_marginals"}
        assert (out["classes"], out["seed"], out["NET_G"], out["NET_E"], out["n_fake"], out["n_real"]) == (CLASSES, 7, ckpt, '', 12, 12)
        assert out["head"] == paths["trunk"] and out["head_digest"] == IS.head_digest(w, b) and len(out["trunk_digest"]) == 64
        for word in ("torchvision", "TF-ported", "1000 outputs", "1008", "trunk_digest", "head_digest"):
            assert word in out["note"], word
        assert "not verified" not in out["note"] and "lowered" not in out["note"]
        fake, real = codes["fake"].numpy(), codes["real"].numpy()
        assert fake.shape == real.shape == (12, 2048) and fake.dtype == np.float32
        assert 1.0 <= out["inception_score_all"] <= CLASSES and all(1.0 <= v <= CLASSES for v in out["per_split"])
        _against_the_definition(out, fake, w, b, 3)
        _against_the_definition(out["real"], real, w, b, 3)
        assert set(out["real"]) == {"inception_score", "inception_score_std", "per_split", "inception_score_all", "splits"}
        pf, pr = (IS.row_sums(c, w, b)[2].sum(axis=0, keepdims=True) for c in (fake, real))
        kl = IS.kl_marginals(pf, 12, pr, 12)
        # KL(a || b) moves by at most sum |da| (|log a / b| + 1) + sum a |db| / b <= r (sum a |log a / b| + 2), r the marginals' relative bound
        r = max(_marginal_bound(c, w, b) for c in (fake, real))
        a_, b_ = pf[0] / 12, pr[0] / 12
        assert abs(out["kl_marginals"] - kl) <= r * (float((a_ * np.abs(np.log(a_) - np.log(b_))).sum()) + 2.0) + 16 * C.U

        # 3: one pass of the caller's own, under the trunk file: its codes handed over write the same bytes; the images of the
        # pass are, bit for bit, those of a pass without the file
        seen = {True: [], False: []}
        algo = _main_trainer(tmp_path, paths["trunk"])
        handed = algo.pool_codes("test", seed=7, image_sink=lambda r, f, take: seen[True].append(f[:take].clone()))
        os.remove(path)
        again = algo.inception_score("test", seed=7, splits=3, real=True, codes=handed)
        assert open(path, "rb").read() == first and json.loads(json.dumps(again)) == json.loads(first)
        plain = _main_trainer(tmp_path)
        other = plain.pool_codes("test", seed=7, want_real=False, image_sink=lambda r, f, take: seen[False].append(f[:take].clone()))
        ours, theirs = torch.cat(seen[True]), torch.cat(seen[False])
        assert tuple(ours.shape) == (12, 3, 256, 256) and torch.equal(ours.view(torch.int32), theirs.view(torch.int32))
        assert other["trunk_digest"] != handed["trunk_digest"] == out["trunk_digest"]
        assert not torch.equal(other["fake"], handed["fake"])                                # and the file's trunk did run

        # the splits are lowered where there are fewer images; without --is_real there is no real side
        low = algo.inception_score("test", seed=7, splits=20, codes=handed)
        assert low["splits"] == 12 and len(low["per_split"]) == 12 and "splits lowered from 20 to 12" in low["note"]
        assert set(low) == KEYS and low["n_real"] == 0
        _against_the_definition(low, fake, w, b, 12)
        assert all(abs(v - 1.0) <= 1e-12 for v in low["per_split"])                          # a split of one image: KL = 0
        # a head alone: accepted, and the note says it was not verified; the same figures
        alone = algo.inception_score("test", seed=7, splits=3, real=True, codes=handed, head_path=paths["head_only"])
        assert "not verified" in alone["note"] and alone["head"] == paths["head_only"] and alone["head_digest"] == out["head_digest"]
        assert alone["per_split"] == out["per_split"] and alone["real"] == out["real"]
        # the head's errors: of another trunk; none anywhere; codes of another seed; no real side in the codes
        with pytest.raises(ValueError, match="head of another trunk"):
            algo.inception_score("test", seed=7, codes=handed, head_path=paths["other_trunk"])
        with pytest.raises(ValueError, match="head of another trunk"):
            plain.inception_score("test", seed=7, codes=other, head_path=paths["trunk"])
        with pytest.raises(ValueError, match="no head"):
            plain.inception_score("test", seed=7, codes=other)
        with pytest.raises(ValueError, match="no head"):
            _main_trainer(tmp_path, paths["headless"]).inception_score("test", seed=7, codes=handed)
        with pytest.raises(ValueError, match="no head"):
            algo.inception_score("test", seed=7, codes=handed, head_path=paths["headless"])
        with pytest.raises(ValueError, match="seed"):
            algo.inception_score("test", seed=8, codes=handed)
        with pytest.raises(ValueError, match="no real side"):
            plain.inception_score("test", seed=7, codes=other, real=True, head_path=paths["head_only"])
        assert open(path, "rb").read() != first                                              # (the head-alone run wrote last)
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.FLAG = '', True


def test_a_non_finite_code_is_named(tmp_path):
    cfg, ev, ckpt = _tiny_checkpoint(tmp_path)
    try:
        rng = np.random.RandomState(2)
        head = str(tmp_path / "head.pth")
        torch.save({"fc.weight": torch.from_numpy(rng.standard_normal((3, 2048)).astype(np.float32)), "fc.bias": torch.zeros(3)}, head)
        algo = _main_trainer(tmp_path)
        fake = torch.from_numpy(rng.uniform(0, 1, (12, 2048)).astype(np.float32)).cuda()
        fake[5, 100] = float("nan")
        codes = {"real": None, "fake": fake, "n": 12, "trunk_digest": "0" * 64, "seed": 7}
        with pytest.raises(ValueError, match="row 5 of the generated codes"):
            algo.inception_score("test", seed=7, codes=codes, head_path=head)
        fake[5, 100] = 0.5
        out = algo.inception_score("test", seed=7, codes=codes, head_path=head, splits=2)
        _against_the_definition(out, fake.cpu().numpy(), *[t.numpy() for t in torch.load(head).values()], 2)
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.FLAG = '', True
