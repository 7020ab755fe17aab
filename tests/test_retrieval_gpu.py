"""-m gpu: R-precision on the device -- mogan_retrieval_rank through ctypes in guard-banded, poisoned memory against the fp64 oracle
(tests/retrieval_cases.py: cases, seeds, TOL and the gap condition), the tie rule bit for bit, the extremes, the index clamp; then
SentenceBank.build against the stock-module text encoder, condGANTrainer.r_precision end to end (directly and through main.py) and
DAMSMEngine.retrieval.  No bound here comes from the code under test."""
import json
import os

import numpy as np
import pytest
import torch

import memguard as MG
import retrieval_cases as K
from eval_setup import tiny_checkpoint as _tiny_checkpoint, trainer as _trainer
from helpers import load_pkg

load_pkg()
from mogan_amd.hip import lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FULL = (slice(None),)
SHAPES = list(K.CASES)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


class Run:
    """one problem in guarded memory: inputs with bands (bitwise frozen), score and rank poisoned inside bands"""

    def __init__(self, code, pos, bank, idx, with_score=True):
        self.Q, self.C = code.shape
        self.N, self.Rn = bank.shape[0], idx.shape[1]
        self.ins = [MG.Guarded(tuple(t.shape), FULL, DEV, base=t.to(DEV)) for t in (code, pos, bank)]
        ib = torch.full((idx.numel() + 2 * MG.BAND,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        self.idx_buf, self.idx_snap = ib, None
        self.idx = ib[MG.BAND:MG.BAND + idx.numel()].view(idx.shape)
        self.idx.copy_(idx.to(DEV))
        self.idx_snap = ib.clone()
        self.score = MG.Guarded((self.Q, self.Rn + 1), FULL, DEV) if with_score else None
        self.rank = MG.Guarded((self.Q,), FULL, DEV)            # int32 ranks in an fp32-typed guarded buffer: same 4 bytes

    def call(self, eps=K.EPS):
        rc = lib.load().mogan_retrieval_rank(self.ins[0].ptr, self.ins[1].ptr, self.ins[2].ptr, self.idx.data_ptr(), self.Q, self.Rn,
                                             self.C, self.N, eps, self.score.ptr if self.score else None, self.rank.ptr,
                                             lib.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def ranks(self):
        return self.rank.view.view(torch.int32).cpu().long()

    def scores(self):
        return self.score.view.cpu()

    def check_memory(self, what):
        """every output element written, nothing outside the outputs changed, inputs bitwise as they were"""
        self.rank.check(what=what + " rank")
        if self.score:
            self.score.check(what=what + " score")
        for g, name in zip(self.ins, ("code", "pos", "bank")):
            assert g.untouched(), "%s: %s or its bands were modified" % (what, name)
        assert torch.equal(self.idx_buf, self.idx_snap), "%s: idx or its bands were modified" % what


# ------------------------------------------------------------------------------------------------- 1: the kernel, per element
@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_scores_and_ranks_against_fp64_in_guarded_memory(shape):
    ref = K.reference(shape)
    assert K.gap(ref["score"]) >= K.GAP, "the seeded inputs have a near-tie: rank equality would mean nothing"
    run = Run(*ref["in"])
    assert run.call() == 0
    err = float((run.scores().double() - ref["score"]).abs().max())
    print("%s: max |score - fp64| %.3e (TOL %.2e)" % (shape, err, K.TOL))
    run.score.check(ref["score"], atol=K.TOL, what="score %s" % (shape,))
    run.check_memory(str(shape))
    assert torch.equal(run.ranks(), ref["rank"])
    # the same inputs give the same bits on every call
    s1, r1 = _bits(run.score.view).clone(), _bits(run.rank.view).clone()
    run.score.reset()
    run.rank.reset()
    assert run.call() == 0
    assert torch.equal(_bits(run.score.view), s1) and torch.equal(_bits(run.rank.view), r1)
    run.check_memory("%s, second call" % (shape,))
    # score = NULL: the same ranks
    lean = Run(*ref["in"], with_score=False)
    assert lean.call() == 0
    lean.check_memory("%s, no score" % (shape,))
    assert torch.equal(_bits(lean.rank.view), r1)


def test_op_matches_the_entry_point_and_checks_a_host_idx():
    shape = (5, 99, 300, 130)
    ref = K.reference(shape)
    code, pos, bank, idx = ref["in"]
    rank, score = ops.retrieval_rank(code.to(DEV), pos.to(DEV), bank.to(DEV), idx.to(DEV), want_scores=True)
    assert rank.dtype == torch.int32 and tuple(rank.shape) == (5,) and tuple(score.shape) == (5, 100)
    assert torch.equal(rank.cpu().long(), ref["rank"]) and float((score.cpu().double() - ref["score"]).abs().max()) <= K.TOL
    again = ops.retrieval_rank(code.to(DEV), pos.to(DEV), bank.to(DEV), idx.numpy())             # host idx: checked, uploaded
    assert torch.equal(again, rank)
    bad = idx.numpy().copy()
    bad[3, 7] = 130
    with pytest.raises(IndexError):
        ops.retrieval_rank(code.to(DEV), pos.to(DEV), bank.to(DEV), bad)
    with pytest.raises(ValueError):
        ops.retrieval_rank(code.to(DEV), pos.to(DEV), bank.to(DEV), idx.long().to(DEV))


# ------------------------------------------------------------------------------------------------- 2: the tie rule, bitwise
@pytest.mark.parametrize("shape", [(3, 9, 70, 11), (2, 99, 256, 40), (2, 5, 1, 6)], ids=str)
def test_tie_rule_bitwise(shape):
    """a bank row that is a bit copy of pos[q], listed at r = 1, 4, 5 and Rn (several stripes and wave positions), gets the match's
    score bits and does not raise the rank; the same bank row listed twice gets equal bits"""
    Q, Rn, C, N = shape
    code, pos, bank, idx = K.make_inputs(shape, 11)
    q = Q - 1
    bank[2] = pos[q]
    for r in (1, 4, 5, Rn):
        idx[q, r - 1] = 2
    idx[0, 1], idx[0, Rn - 2] = 3, 3                      # one mismatched row twice, in another query
    _, base = K.oracle(code, pos, bank, idx)
    run = Run(code, pos, bank, idx)
    assert run.call() == 0
    run.check_memory("tie %s" % (shape,))
    sb = _bits(run.score.view).cpu()
    for r in (1, 4, 5, Rn):
        assert int(sb[q, r]) == int(sb[q, 0]), "copy of pos at r = %d: %r vs %r" % (r, float(run.scores()[q, r]), float(run.scores()[q, 0]))
    assert int(sb[0, 2]) == int(sb[0, Rn - 1])
    # the copies do not count: the rank is that of the other candidates alone (fp64, ties for the match)
    others = [r for r in range(1, Rn + 1) if int(idx[q, r - 1]) != 2]
    s64, _ = K.oracle(code, pos, bank, idx)
    if C > 1 and others:
        assert float((s64[q, others] - s64[q, 0]).abs().min()) >= K.GAP
        assert int(run.ranks()[q]) == int((s64[q, others] > s64[q, 0]).sum()) == int(base[q])


def test_pure_tie_gives_rank_zero():
    """(1, 1, 1, 1) with the bank row a copy of pos: both scores are the same +-1, rank 0"""
    for v, c in ((0.37, 1.9), (-2.5, 0.004), (1e-3, -7.0)):
        code, pos, bank = torch.tensor([[c]]), torch.tensor([[v]]), torch.tensor([[v]])
        run = Run(code, pos, bank, torch.zeros(1, 1, dtype=torch.int32))
        assert run.call() == 0
        run.check_memory("pure tie")
        s = run.scores()
        # x v / (sqrt(x x) sqrt(v v)): six roundings, the two under a square root count half -- within 6 x 2^-24 of +-1
        assert int(_bits(s)[0, 0]) == int(_bits(s)[0, 1]) and abs(abs(float(s[0, 0])) - 1.0) <= 7 * 2.0 ** -24
        assert run.ranks().tolist() == [0]


# ------------------------------------------------------------------------------------------------- 3: extremes
def test_extremes():
    shape = (6, 37, 100, 50)
    Q, Rn, C, N = shape
    code, pos, bank, idx = K.make_inputs(shape, 2)
    run = Run(code, code.clone(), bank, idx)               # the match is the image code itself: cosine 1, first everywhere
    assert run.call() == 0
    assert run.ranks().tolist() == [0] * Q and float((run.scores()[:, 0] - 1.0).abs().max()) <= K.TOL
    run = Run(code, -code, bank, idx)                       # ... its negative: cosine -1, last everywhere
    assert run.call() == 0
    assert run.ranks().tolist() == [Rn] * Q and float((run.scores()[:, 0] + 1.0).abs().max()) <= K.TOL
    # an all-zero pos row: 0 / max(0, eps) = 0 through the clamp, no NaN, the oracle's rank
    pos = pos.clone()
    pos[1] = 0.0
    s64, r64 = K.oracle(code, pos, bank, idx)
    assert float(s64[1, 0]) == 0.0 and K.gap(s64) >= K.GAP
    run = Run(code, pos, bank, idx)
    assert run.call() == 0
    run.check_memory("zero pos row")
    got = run.scores()
    assert bool(torch.isfinite(got).all()) and float(got[1, 0]) == 0.0
    run.score.check(s64, atol=K.TOL, what="zero pos row")
    assert torch.equal(run.ranks(), r64)
    # an all-zero bank row and an all-zero code row as well
    bank = bank.clone()
    bank[int(idx[0, 0])] = 0.0
    code = code.clone()
    code[2] = 0.0
    s64, r64 = K.oracle(code, pos, bank, idx)
    run = Run(code, pos, bank, idx)
    assert run.call() == 0
    got = run.scores()
    assert bool(torch.isfinite(got).all()) and float(got[0, 1]) == 0.0 and float(got[2].abs().max()) == 0.0
    run.score.check(s64, atol=K.TOL, what="zero rows")
    assert int(run.ranks()[2]) == 0                         # every score of the zero query is 0: all tie with the match


# ------------------------------------------------------------------------------------------------- 4: the clamp
def test_idx_is_clamped_with_the_bank_inside_guard_bands():
    shape = (4, 12, 33, 9)
    Q, Rn, C, N = shape
    code, pos, bank, idx = K.make_inputs(shape, 5)
    wild, tame = idx.clone(), idx.clone()
    for (q, r), (w, t) in {(0, 0): (-1, 0), (1, 5): (N, N - 1), (3, 11): (-1, 0), (2, 2): (N, N - 1)}.items():
        wild[q, r], tame[q, r] = w, t
    a, b = Run(code, pos, bank, wild), Run(code, pos, bank, tame)
    assert a.call() == 0 and b.call() == 0
    a.check_memory("clamped idx")
    assert torch.equal(_bits(a.score.view), _bits(b.score.view)) and torch.equal(a.ranks(), b.ranks())
    s64, r64 = K.oracle(code, pos, bank, wild)              # the oracle clamps the same way
    a.score.check(s64, atol=K.TOL, what="clamped idx")


# ------------------------------------------------------------------------------------------------- 5: the bank on the device
def _mixed_captions(n=37, longest=18, seed=4):
    rng = np.random.RandomState(seed)
    lens = rng.randint(1, longest + 1, n)
    lens[:3] = (1, longest, 12)
    return [rng.randint(1, 300, k).tolist() for k in lens]


def test_sentence_bank_against_the_stock_modules():
    """37 captions of 1..18 tokens (TEXT.WORDS_NUM 12: the long ones keep a seeded subset), chunk 16, on the one-launch text
    encoder against the stock nn.Embedding / nn.LSTM path of the same module: within 5e-6, test_text_encoder_as_one_launch's
    bound; the rows do not depend on the chunk"""
    from mogan_amd.attngan import model, retrieval as R
    from mogan_amd.attngan.miscc.config import cfg
    cfg.RNN_TYPE = 'LSTM'
    torch.manual_seed(8)
    enc = model.RNN_ENCODER(300, nhidden=256).to(DEV).eval()
    caps = _mixed_captions()
    image_index = np.arange(len(caps)) // 5
    n0 = ops.PK_STATS.get("lstm_fused", 0)
    bank = R.SentenceBank.build(enc, caps, image_index, 12, seed=3, chunk=16)
    assert ops.PK_STATS.get("lstm_fused", 0) == n0 + 3 and tuple(bank.bank.shape) == (37, 256) and bank.bank.is_cuda
    model.RNN_ENCODER.FUSED = False
    try:
        stock = R.SentenceBank.build(enc, caps, image_index, 12, seed=3, chunk=16)
    finally:
        model.RNN_ENCODER.FUSED = True
    assert ops.PK_STATS.get("lstm_fused", 0) == n0 + 3
    assert float((bank.bank - stock.bank).abs().max()) <= 5e-6
    # row i is caption i: against the module on each caption alone, in caption order with the same seeded subsets
    rng = np.random.RandomState(3)
    with torch.no_grad():
        for i, cap in enumerate(caps):
            k = R.fit_caption(cap, 12, rng)
            if i % 6 == 0:
                tok = torch.zeros(1, 12, dtype=torch.int64)
                tok[0, :len(k)] = torch.from_numpy(k)
                _, one = enc(tok.to(DEV), torch.tensor([len(k)]), enc.init_hidden(1))
                assert float((bank.bank[i] - one[0]).abs().max()) <= 5e-6, i
    for chunk in (1024, 5):
        other = R.SentenceBank.build(enc, caps, image_index, 12, seed=3, chunk=chunk)
        assert float((other.bank - bank.bank).abs().max()) <= 5e-6, chunk


# ------------------------------------------------------------------------------------------------- 6: end to end
def test_r_precision_end_to_end(tmp_path):
    cfg, ev, ckpt = _tiny_checkpoint(tmp_path)
    try:
        algo = _trainer(tmp_path)
        out, t = algo.r_precision("test", n_mismatched=5, seed=100, return_codes=True)
        path = os.path.join(ckpt[:-4], "valid", "r_precision.json")
        assert os.path.isfile(path) and json.load(open(path)) == out
        assert set(out) == {"r_precision", "mean", "std", "n", "folds", "n_mismatched", "seed", "real", "NET_G", "NET_E"}
        assert out["n"] == 12 and out["folds"] == 10 and out["n_mismatched"] == 5 and out["seed"] == 100 and out["real"] is False
        assert out["NET_G"] == ckpt and out["NET_E"] == '' and 0.0 <= out["r_precision"] <= 1.0
        assert tuple(t["code"].shape) == (12, 32) == tuple(t["pos"].shape) and tuple(t["idx"].shape) == (12, 5)
        assert tuple(t["bank"].shape) == (12, 32) and t["rank"].dtype == torch.int32
        for row in t["idx"].tolist():
            assert len(set(row)) == 5 and all(0 <= r < 12 for r in row)
        s64, r64 = K.oracle(t["code"], t["pos"], t["bank"], t["idx"])
        print("end to end: gap %.2e, ranks %s" % (K.gap(s64), t["rank"].tolist()))
        assert K.gap(s64) >= K.GAP
        assert torch.equal(t["rank"].long(), r64)
        assert out["r_precision"] == pytest.approx(float((r64 == 0).double().mean()))
        out2, t2 = algo.r_precision("test", n_mismatched=5, seed=100, return_codes=True)        # same seed, same ranks
        assert torch.equal(t2["rank"], t["rank"]) and torch.equal(t2["idx"], t["idx"]) and out2 == out
        out3, t3 = algo.r_precision("test", n_mismatched=5, seed=101, return_codes=True)        # another seed, another table
        assert not torch.equal(t3["idx"], t["idx"])
        real, tr = algo.r_precision("test", n_mismatched=5, seed=100, real=True, return_codes=True)
        assert real["real"] is True and real["n"] == 12 and json.load(open(path)) == real
        s64r, r64r = K.oracle(tr["code"], tr["pos"], tr["bank"], tr["idx"])
        print("real images: gap %.2e, ranks %s" % (K.gap(s64r), tr["rank"].tolist()))
        if K.gap(s64r) >= K.GAP:                                   # (asked of the generated run above; here only where it holds)
            assert torch.equal(tr["rank"].long(), r64r)
        assert not torch.equal(tr["code"], t["code"])
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.FLAG = '', True


def test_main_r_precision_on_synthetic(tmp_path):
    from mogan_amd.attngan import main as entry
    cfg, ev, ckpt = _tiny_checkpoint(tmp_path)
    try:
        entry.main(["--cfg", str(ev), "--synthetic", "12", "--manualSeed", "7", "--output_dir", str(tmp_path), "--r_precision"])
        path = os.path.join(ckpt[:-4], "valid", "r_precision.json")
        out = json.load(open(path))
        # 12 synthetic samples, one caption each: 11 captions of other images, fewer than the protocol's 99 -- recorded as such
        assert out["n"] == 12 and out["n_mismatched"] == 11 and out["seed"] == 7 and out["real"] is False
        assert 0.0 <= out["r_precision"] <= 1.0
        entry.main(["--cfg", str(ev), "--synthetic", "12", "--manualSeed", "7", "--output_dir", str(tmp_path), "--r_precision",
                    "--real"])
        assert json.load(open(path))["real"] is True
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.FLAG = '', True


def test_r_precision_needs_the_encoder_pair(tmp_path):
    """TRAIN.NET_E names a text encoder whose image_encoder twin is missing: FileNotFoundError, as build_models raises"""
    from mogan_amd.attngan import model
    cfg, ev, ckpt = _tiny_checkpoint(tmp_path)
    try:
        te = str(tmp_path / "text_encoder0.pth")
        torch.save(model.RNN_ENCODER(100, nhidden=32).state_dict(), te)
        cfg.TRAIN.NET_E = te
        with pytest.raises(FileNotFoundError):
            _trainer(tmp_path, length=4, seed=0).r_precision("test", n_mismatched=2)
    finally:
        cfg.TRAIN.NET_G, cfg.TRAIN.NET_E, cfg.TRAIN.FLAG = '', '', True


# ------------------------------------------------------------------------------------------------- 7: DAMSM pre-training
def test_damsm_engine_retrieval(tmp_path, capsys):
    from mogan_amd.attngan import model, pretrain_DAMSM as PD
    from mogan_amd.attngan.datasets import SyntheticTextDataset
    from mogan_amd.attngan.miscc.config import cfg
    yml = tmp_path / "damsm.yml"
    yml.write_text("CONFIG_NAME: 'damsm'\nDATASET_NAME: 'coco'\nWORKERS: 0\nRNN_TYPE: 'LSTM'\nTREE: {BRANCH_NUM: 1, BASE_SIZE: 64}\n"
                   "TEXT: {EMBEDDING_DIM: 32, CAPTIONS_PER_IMAGE: 5, WORDS_NUM: 12}\n"
                   "TRAIN: {FLAG: True, BATCH_SIZE: 4, MAX_EPOCH: 1, SNAPSHOT_INTERVAL: 1, NET_E: '', ENCODER_LR: 0.002}\n")
    PD.cfg_from_file(str(yml))
    torch.manual_seed(7)
    ds = SyntheticTextDataset(length=8, seed=3)
    text, image = model.RNN_ENCODER(ds.n_words, nhidden=32), model.CNN_ENCODER(32)
    eng = PD.DAMSMEngine(text.to(DEV), image.to(DEV))
    dl = torch.utils.data.DataLoader(ds, batch_size=4, drop_last=True, shuffle=False)
    assert eng.text_encoder.training
    rp = eng.retrieval(dl, ds, n_mismatched=5, seed=1)
    assert isinstance(rp, float) and 0.0 <= rp <= 1.0 and rp * 8 == round(rp * 8)
    assert eng.text_encoder.training and not eng.image_encoder.training
    assert eng.retrieval(dl, ds, n_mismatched=5, seed=1) == rp
    eng.text_encoder.eval()
    eng.retrieval(dl, ds, n_mismatched=5, seed=1)
    assert not eng.text_encoder.training
    eng.text_encoder.train()
    capsys.readouterr()
    assert eng.retrieval(dl, ds) is None                     # 7 captions of other images, 99 asked for: skipped, with a note
    assert "R-precision skipped" in capsys.readouterr().out and eng.text_encoder.training
    cfg.TREE.BRANCH_NUM = 3
