"""The set-up the end-to-end tests of condGANTrainer's evaluation methods share (tests/test_retrieval_gpu.py, test_fid_gpu.py,
test_kid_gpu.py, test_prdc_gpu.py and the sample() test of test_encoder_trainer_gpu.py): a tiny evaluation config, a checkpoint of
a random-init generator at its widths, and a trainer over a small synthetic split.  A test restores cfg.TRAIN.NET_G = '' and
cfg.TRAIN.FLAG = True when it is done."""
import torch

TINY = ("CONFIG_NAME: 'tiny'\nDATASET_NAME: 'coco'\nWORKERS: 0\nRNN_TYPE: 'LSTM'\nTREE: {BRANCH_NUM: 3, BASE_SIZE: 64}\n"
        "GAN: {DF_DIM: 8, GF_DIM: 8, Z_DIM: 100, R_NUM: 1}\n"
        "TEXT: {EMBEDDING_DIM: 32, CAPTIONS_PER_IMAGE: 5, WORDS_NUM: 6}\n")


def tiny_checkpoint(tmp_path):
    """writes and loads the evaluation yml (TRAIN.NET_G: the checkpoint, NET_E: '') and saves the checkpoint: (cfg, yml, checkpoint)"""
    from mogan_amd.attngan import model
    from mogan_amd.attngan.miscc.config import cfg, cfg_from_file
    from mogan_amd.attngan.miscc.utils import weights_init
    ckpt = str(tmp_path / "netG_tiny.pth")
    ev = tmp_path / "eval.yml"
    ev.write_text(TINY + "TRAIN: {FLAG: False, BATCH_SIZE: 4, NET_G: '%s', NET_E: ''}\n" % ckpt)
    cfg_from_file(str(ev))
    torch.manual_seed(21)
    netG = model.G_NET()
    netG.apply(weights_init)
    torch.save({"netG": netG.state_dict()}, ckpt)
    return cfg, ev, ckpt


def trainer(tmp_path, length=12, seed=7, **dataset_kw):
    """condGANTrainer over `length` synthetic samples of a 100-word vocabulary in batches of 4; call it after tiny_checkpoint
    (the dataset takes its image sizes from the config)"""
    from mogan_amd.attngan.datasets import SyntheticTextDataset
    from mogan_amd.attngan.trainer import condGANTrainer
    ds = SyntheticTextDataset(length=length, n_words=100, seed=seed, **dataset_kw)
    dl = torch.utils.data.DataLoader(ds, batch_size=4, drop_last=True, shuffle=False)
    return condGANTrainer(str(tmp_path), dl, 100, ds.ixtoword, resume=False)
