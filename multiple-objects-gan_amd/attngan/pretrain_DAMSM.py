"""DAMSM pre-training: trains the text encoder (embedding + bi-LSTM, or bi-GRU with `RNN_TYPE: 'GRU'` in the yml) and the image encoder's two heads against the word /
sentence matching losses, i.e. produces the `text_encoder%d.pth` / `image_encoder%d.pth` pair that TRAIN.NET_E names.

The reference repository holds no such script (its users download the pair from the AttnGAN project); the recipe is AttnGAN's,
as the config keys imply: loss = w_loss0 + w_loss1 + s_loss0 + s_loss1, one Adam (0.5, 0.999) at TRAIN.ENCODER_LR over the text
encoder and the heads, the text encoder's gradient norm clipped to TRAIN.RNN_GRAD_CLIP, the learning rate * 0.98 per epoch with
a floor of ENCODER_LR / 10, the Inception trunk frozen (eval mode).

Same flags as main.py (--cfg --gpu --manualSeed --data_dir --output_dir ...); `--synthetic N` trains on N generated batches per
epoch when the COCO pickles are not present.  One process, one GPU.  Both values of RNN_TYPE train on the HIP path
(csrc/mogan_rnn.hip).  Not built: data-parallel pre-training, training the Inception trunk, hipGraph
capture of this step."""
import argparse
import datetime
import os
import pprint
import random
import sys
import time

import numpy as np
import torch

if __package__ in (None, ""):
    sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.realpath(__file__)), "..", "..")))
    import mogan_loader
    mogan_loader.load()
    from mogan_amd.attngan.miscc.config import cfg, cfg_from_file
    from mogan_amd.attngan.miscc import losses as L
    from mogan_amd.attngan.datasets import SyntheticTextDataset, TextDataset
    from mogan_amd.attngan.model import CNN_ENCODER, RNN_ENCODER
    from mogan_amd.attngan.trainer import FlatAdam
    from mogan_amd.attngan import inception
    from mogan_amd.hip import lib as hiplib, ops
else:
    from .miscc.config import cfg, cfg_from_file
    from .miscc import losses as L
    from .datasets import SyntheticTextDataset, TextDataset
    from .model import CNN_ENCODER, RNN_ENCODER
    from .trainer import FlatAdam
    from . import inception
    from ..hip import lib as hiplib, ops

LR_DECAY = 0.98


def prepare_batch(data, device):
    """(images of the last branch, captions, caption lengths, class ids) of a TextDataset batch, sorted by falling caption length
    (pack_padded_sequence's order, as datasets.prepare_data does).  The lengths stay on the host: the kernels take them there."""
    imgs, captions, cap_lens, class_ids = data[0], data[1], data[2], data[3]
    lens, order = torch.sort(cap_lens, 0, True)
    return (imgs[-1][order].to(device, non_blocking=True), captions[order].squeeze(-1).to(device), lens,
            class_ids[order].numpy())


class DAMSMEngine:
    """The two encoders and ONE FlatAdam over what is trained: the text encoder's nine tensors (LSTM or GRU: their count and
    sizes are taken from the module, not assumed) and the image encoder's heads (emb_features 1x1 convolution, emb_cnn_code
    linear).  The trunk is frozen and stays in eval mode (the fast frozen trunk)."""

    def __init__(self, text_encoder, image_encoder, lr=None, clip=None):
        self.text_encoder, self.image_encoder = text_encoder, image_encoder
        self.base_lr = float(cfg.TRAIN.ENCODER_LR if lr is None else lr)
        self.clip = float(cfg.TRAIN.RNN_GRAD_CLIP if clip is None else clip)
        for p in text_encoder.parameters():
            p.requires_grad = True
        for p in image_encoder.parameters():
            p.requires_grad = False
        for name in image_encoder.HEADS:
            for p in getattr(image_encoder, name).parameters():
                p.requires_grad = True
        text_encoder.train()
        image_encoder.eval()
        self.nets = torch.nn.ModuleList([text_encoder, image_encoder])
        self.opt = FlatAdam(self.nets, self.base_lr)
        # the text encoder's parameters come first in the flat buckets: its gradient is one slice (the alignment gaps are zeros)
        n_text = len(list(text_encoder.parameters()))
        self.n_text = self.opt.offsets[n_text] if n_text < len(self.opt.offsets) else self.opt.numel
        self.device = self.opt.p.device
        self._labels = {}

    # ------------------------------------------------------------------------------------------------------------ pieces
    def trunk(self, imgs):
        """images (B, 3, h, w) -> (17 x 17 x 768 map, pooled 2048 code) of the frozen trunk, no gradient"""
        enc = self.image_encoder
        with torch.no_grad():
            x = ops.bilinear_resize(imgs, 299, 299)
            feat, last = inception.frozen_trunk(enc, x)
            return feat, ops.avg_pool2d(last, 8).view(last.size(0), -1)

    def _labels_for(self, B):
        if B not in self._labels:
            self._labels[B] = torch.arange(B, device=self.device)
        return self._labels[B]

    def _losses(self, feat768, code2048, captions, cap_lens, class_ids, drop_mask=None):
        B = captions.shape[0]
        enc = self.image_encoder
        feats, code = enc.emb_features(feat768), enc.emb_cnn_code(code2048)
        words, sent = self.text_encoder(captions, cap_lens, self.text_encoder.init_hidden(B), drop_mask=drop_mask)
        labels = self._labels_for(B)
        w0, w1, _ = L.words_loss(feats, words, labels, cap_lens, class_ids, B)
        s0, s1 = L.sent_loss(code, sent, labels, class_ids, B)
        return w0, w1, s0, s1

    # -------------------------------------------------------------------------------------------------------------- step
    def step_from_features(self, feat768, code2048, captions, cap_lens, class_ids, drop_mask=None):
        """heads -> text encoder -> the four losses -> backward -> clip the text encoder's gradient -> Adam.
        Returns (w_loss0, w_loss1, s_loss0, s_loss1, the text gradient's norm before clipping) as device scalars; nothing in
        here waits for the device."""
        self.opt.zero_grad()
        w0, w1, s0, s1 = self._losses(feat768, code2048, captions, cap_lens, class_ids, drop_mask)
        ops.scalar_sum([w0, w1, s0, s1]).backward()
        g = self.opt.g[:self.n_text]
        norm = torch.linalg.vector_norm(g)                       # clip_grad_norm_: g *= min(1, clip / (norm + 1e-6))
        g.mul_(torch.clamp(self.clip / (norm + 1e-6), max=1.0))
        self.opt.step()
        return w0.detach(), w1.detach(), s0.detach(), s1.detach(), norm

    def step(self, batch):
        """batch = (images, captions, cap_lens (host), class_ids) as prepare_batch returns them"""
        imgs, captions, cap_lens, class_ids = batch
        feat, code = self.trunk(imgs)
        return self.step_from_features(feat, code, captions, cap_lens, class_ids)

    def evaluate(self, loader):
        """mean of the four losses over the loader, eval mode, no gradients"""
        was = self.text_encoder.training
        self.text_encoder.eval()
        tot, n = torch.zeros(4, device=self.device), 0
        try:
            with torch.no_grad():
                for data in loader:
                    imgs, captions, cap_lens, class_ids = prepare_batch(data, self.device)
                    feat, code = self.trunk(imgs)
                    tot += torch.stack(self._losses(feat, code, captions, cap_lens, class_ids))
                    n += 1
        finally:
            self.text_encoder.train(was)
        return [float(v) / max(n, 1) for v in tot.tolist()]

    def retrieval(self, loader, dataset, n_mismatched=99, seed=0):
        """R-precision of the REAL images of `loader` under the two encoders as they are now (attngan/retrieval.py, DESIGN.md
        section 9c): every caption of `dataset` encoded once, each image's code ranked against its batch caption and
        `n_mismatched` captions of other images (hip/ops.retrieval_rank).  Eval mode, no gradients, one read-back; the text
        encoder is left in the mode it was found in.  None, with a note, when the split has too few captions of other images."""
        from .retrieval import SentenceBank, dataset_captions, draw_mismatched, eligible, fold_stats
        captions, image_index, keys = dataset_captions(dataset)
        if not eligible(image_index, n_mismatched):
            print('R-precision skipped: the validation split has fewer than %d captions of other images' % n_mismatched)
            return None
        was = self.text_encoder.training
        self.text_encoder.eval()
        rng, ranks = np.random.RandomState(seed), []
        try:
            bank = SentenceBank.build(self.text_encoder, captions, image_index, cfg.TEXT.WORDS_NUM, seed,
                                      key_to_image={k: i for i, k in enumerate(keys)})
            with torch.no_grad():
                for data in loader:
                    lens, order = torch.sort(data[2], 0, True)
                    batch_keys = [data[4][i] for i in order.tolist()]
                    caps = data[1][order].squeeze(-1).to(self.device)
                    _, code2048 = self.trunk(data[0][-1][order].to(self.device, non_blocking=True))
                    code = self.image_encoder.emb_cnn_code(code2048)
                    _, sent = self.text_encoder(caps, lens, self.text_encoder.init_hidden(caps.shape[0]))
                    idx = draw_mismatched(bank.image_index, bank.images_of(batch_keys), n_mismatched, rng)
                    ranks.append(ops.retrieval_rank(code, sent, bank.bank, idx))
        finally:
            self.text_encoder.train(was)
        if not ranks:
            return None
        return fold_stats(torch.cat(ranks).cpu().numpy(), 1)["r_precision"]

    def decay_lr(self):
        """once per epoch: * 0.98, floored at ENCODER_LR / 10"""
        self.opt.lr = max(self.opt.lr * LR_DECAY, self.base_lr / 10.0)
        return self.opt.lr

    def save(self, model_dir, epoch):
        """plain state_dicts with the reference's keys: what condGANTrainer.build_models loads through TRAIN.NET_E"""
        os.makedirs(model_dir, exist_ok=True)
        paths = []
        for net, name in ((self.text_encoder, "text_encoder"), (self.image_encoder, "image_encoder")):
            sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
            paths.append(os.path.join(model_dir, "%s%d.pth" % (name, epoch)))
            torch.save(sd, paths[-1])
        return paths


def build_encoders(n_words, device, trunk=None):
    """`trunk`: a torchvision inception_v3 file (or an image_encoder checkpoint) whose Inception trunk replaces the random-init one
    -- after construction, so the draws from torch's global generator are those of a run without it -- and after NET_E's pair."""
    text_encoder = RNN_ENCODER(n_words, nhidden=cfg.TEXT.EMBEDDING_DIM)
    image_encoder = CNN_ENCODER(cfg.TEXT.EMBEDDING_DIM, pretrained=False)
    if cfg.TRAIN.NET_E != '':                                   # continue from an earlier pair
        img_path = cfg.TRAIN.NET_E.replace('text_encoder', 'image_encoder')
        text_encoder.load_state_dict(torch.load(cfg.TRAIN.NET_E, map_location='cpu'))
        image_encoder.load_state_dict(torch.load(img_path, map_location='cpu'))
        print('Load text / image encoder from:', cfg.TRAIN.NET_E, img_path)
    if trunk:
        image_encoder.load_trunk_file(trunk)
    return text_encoder.to(device), image_encoder.to(device)


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='Train the DAMSM text / image encoders')
    parser.add_argument('--cfg', dest='cfg_file', help='optional config file', default='cfg/DAMSM/coco.yml', type=str)
    parser.add_argument('--gpu', dest='gpu_id', type=str, default='0')
    parser.add_argument('--data_dir', dest='data_dir', type=str, default='')
    parser.add_argument('--manualSeed', type=int, help='manual seed')
    parser.add_argument('--synthetic', type=int, default=0, help='train on N generated batches per epoch instead of COCO')
    parser.add_argument('--max_epoch', type=int, default=None)
    parser.add_argument('--batch_size', type=int, default=None)
    parser.add_argument('--output_dir', type=str, default='')
    parser.add_argument('--trunk', type=str, default=None, metavar='PATH',
                        help='start the frozen Inception trunk from this file instead of a random one: torchvision\'s '
                             'inception_v3_google-*.pth (old or new layout), or any image_encoder*.pth, of which the trunk is read')
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    if args.cfg_file is not None:
        cfg_from_file(args.cfg_file)
    cfg.GPU_ID = args.gpu_id
    if args.data_dir != '':
        cfg.DATA_DIR = args.data_dir
    if args.max_epoch is not None:
        cfg.TRAIN.MAX_EPOCH = args.max_epoch
    if args.batch_size is not None:
        cfg.TRAIN.BATCH_SIZE = args.batch_size
    if not torch.cuda.is_initialized():
        hiplib.configure_hw_queues()
        torch.cuda.set_device(int(str(args.gpu_id).split(",")[0]))
    device = torch.device("cuda", torch.cuda.current_device())
    print('Using config:')
    pprint.pprint(cfg)
    if args.manualSeed is None:
        args.manualSeed = random.randint(1, 10000)
    random.seed(args.manualSeed)
    np.random.seed(args.manualSeed)
    torch.manual_seed(args.manualSeed)
    stamp = datetime.datetime.now().strftime('%Y_%m_%d_%H_%M_%S')
    output_dir = args.output_dir or '../../../output/%s_%s_%s' % (cfg.DATASET_NAME, cfg.CONFIG_NAME, stamp)
    model_dir = os.path.join(output_dir, 'Model')
    B = cfg.TRAIN.BATCH_SIZE
    if args.synthetic > 0:
        dataset = SyntheticTextDataset(args.synthetic * B, seed=args.manualSeed)
        dataset_val = SyntheticTextDataset(B, seed=args.manualSeed + 1)
    else:
        dataset = TextDataset(cfg.DATA_DIR, cfg.IMG_DIR, 'train', base_size=cfg.TREE.BASE_SIZE)
        dataset_val = TextDataset(cfg.DATA_DIR, cfg.IMG_DIR, 'test', base_size=cfg.TREE.BASE_SIZE)
    workers = 0 if args.synthetic else int(cfg.WORKERS)
    loader = torch.utils.data.DataLoader(dataset, batch_size=B, drop_last=True, shuffle=True, num_workers=workers)
    loader_val = torch.utils.data.DataLoader(dataset_val, batch_size=B, drop_last=True, shuffle=False, num_workers=workers)
    text_encoder, image_encoder = build_encoders(dataset.n_words, device, trunk=args.trunk)
    engine = DAMSMEngine(text_encoder, image_encoder)
    interval = max(1, int(cfg.TRAIN.SNAPSHOT_INTERVAL))
    epoch = -1
    for epoch in range(cfg.TRAIN.MAX_EPOCH):
        t0, tot, n = time.time(), torch.zeros(5, device=device), 0
        for data in loader:
            tot += torch.stack(engine.step(prepare_batch(data, device)))
            n += 1
        w0, w1, s0, s1, norm = [float(v) / max(n, 1) for v in tot.tolist()]       # one read-back per epoch
        val = engine.evaluate(loader_val)
        print('| epoch %3d | %d batches | %.1f s | lr %.6f | w_loss %.4f %.4f | s_loss %.4f %.4f | |g| %.3f | valid w %.4f %.4f '
              's %.4f %.4f' % (epoch, n, time.time() - t0, engine.opt.lr, w0, w1, s0, s1, norm, val[0], val[1], val[2], val[3]))
        rp = engine.retrieval(loader_val, dataset_val, seed=args.manualSeed)
        if rp is not None:
            print('| epoch %3d | valid R-precision %.4f (real images, 99 mismatched captions)' % (epoch, rp))
        engine.decay_lr()
        if epoch % interval == 0 or epoch == cfg.TRAIN.MAX_EPOCH - 1:
            print('Save encoders to:', ', '.join(engine.save(model_dir, epoch)))
    return engine


if __name__ == "__main__":
    main()
