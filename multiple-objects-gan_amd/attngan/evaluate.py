"""coco-attngan checkpoint evaluation (mirror of code/coco/attngan/trainer.py:387-579, plus the scores of DESIGN.md sections 9c-9k).

`CheckpointEvaluation` is the base of `trainer.condGANTrainer` that holds every path which reads a finished checkpoint instead of
training one: `sampling` / `sample` (images), `r_precision`, and `pool_codes`, the one pass over the data loader, with the eight scores
of the table `SCORES` that can share it.  It needs `self.device`, `self.data_loader`, `self.n_words` and `self.ixtoword` of the trainer
and nothing of the train step.  What these paths have in common is written once here: the NET_G guard and the save-directory rule
(`net_g_missing`, `eval_save_dir`), the text side of a batch (`encode_text`), the seeded generation whose draw order the tests rely on
(`generate_seeded`), the keys every score's JSON shares (`write_score`) and what the scores on the pooled codes do around their own
device calls (`PooledCodes`, `trunk_note`).

How scores share a pass is written once too (`SCORES`, `shared_pass`, `run_scores`, `fed`): a new score costs its
method, one row of `SCORES` and -- where it reads the images -- an accumulator with `sink`, optionally `resample_sink`, and `params`.

`layout_shift` is a mode of its own as `r_precision` is: it generates every image a second time under an edited
layout (`draw_noise`, `generate_from`, `moved_matrices`), which no shared pass does.

`inception_score` is a mode of its own too: it needs a classifier head from a file (`score_head`), which no row of
`SCORES` does, and reads the pooled codes through `PooledCodes` as the table's "codes" scores do.  A trainer's `trunk_path`, where set,
makes `_load_image_encoder` load the Inception trunk from a torchvision file after the encoder's construction.

`scenes` is the one path whose captions and layouts do not come from the data loader: it draws the scenes of a
file the user wrote (attngan/scenes.py) and the attention sheets of their words (`attention_sheets`; attngan/attnsheet.py)."""
import json
import os
from collections import namedtuple

import numpy as np
import torch

from ..hip import ops
from .miscc.config import cfg
from .miscc.utils import mkdir_p, weights_init
from .model import CNN_ENCODER, G_NET, RNN_ENCODER


def draw_bbox_lines(data_img, boxes, imsize):
    """trainer.py:556-566: white (value 1) one-pixel rectangles of the relative boxes (x, y, w, h) on every image of
    the row; pixel coordinates are int(imsize * v) of each value SEPARATELY, w and h are capped at imsize - 1, the first
    absent box (x <= -1) ends the loop."""
    for idx in range(boxes.shape[0]):
        x, y, w, h = tuple(int(imsize * float(v)) for v in boxes[idx])
        w = imsize - 1 if w > imsize - 1 else w
        h = imsize - 1 if h > imsize - 1 else h
        if x <= -1:
            break
        data_img[:, :, y, x:x + w] = 1
        data_img[:, :, y:y + h, x] = 1
        data_img[:, :, y + h, x:x + w] = 1
        data_img[:, :, y:y + h, x + w] = 1
    return data_img


def caption_sentence(cap, ixtoword):
    """trainer.py:569-576: the words of a zero-terminated caption joined by blanks, non-ASCII characters dropped."""
    words = []
    for ix in cap:
        if int(ix) == 0:
            break
        words.append(ixtoword[int(ix)].encode('ascii', 'ignore').decode('ascii'))
    return " ".join(words)


def net_g_missing(what='model NET_G'):
    """The guard of every evaluation path: True, with the reference's message, where TRAIN.NET_G names no checkpoint
    (`what` keeps the reference's wording of trainer.py:389 for sampling())."""
    if cfg.TRAIN.NET_G == '':
        print('Error: the path for %s is not found!' % what)
        return True
    return False


def eval_save_dir(split_dir, sep='/'):
    """<NET_G minus .pth>/<split> of the evaluation paths ('test' reads the 'valid' split), created; sample() joins the
    two with '_' as the reference does (trainer.py:508)"""
    if split_dir == 'test':
        split_dir = 'valid'
    save_dir = cfg.TRAIN.NET_G[:cfg.TRAIN.NET_G.rfind('.pth')] + sep + split_dir
    mkdir_p(save_dir)
    return save_dir


def write_json(save_dir, name, out):
    with open('%s/%s.json' % (save_dir, name), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)


def write_score(split_dir, who, out, seed, note):
    """adds the keys every score's JSON shares to `out`, writes <save directory>/<who>.json and returns the directory"""
    out.update({"seed": int(seed), "NET_G": cfg.TRAIN.NET_G, "NET_E": cfg.TRAIN.NET_E, "note": note})
    save_dir = eval_save_dir(split_dir)
    write_json(save_dir, who, out)
    return save_dir


# The scores that can share one pass, in the order a shared pass finishes them (memorisation last: its grid re-reads training
# images).  name: the method and main.py's flag.  takes, also the keyword of the hand-over: "codes" -- both sides' pooled codes;
# "objects" -- the images, their boxes and the trunk, not the real images' own codes; "images" -- the images only.  factory: the method
# that makes the accumulator from (num_samples, seed) and the score's keywords `params`; a "codes" row's rides in the codes.
Score = namedtuple("Score", "name takes factory params")
SCORES = {s.name: s for s in (
    Score("scene_fid", "objects", "scene_fid_objects", ("min_side",)),
    Score("swd", "images", "swd_images", ("patches", "dirs", "repeats", "min_res")),
    Score("msssim", "images", "msssim_images", ("scales", "same_caption")),
    Score("spectrum", "images", "spectrum_images", ("window",)),
    Score("fid", "codes", None, ()),
    Score("kid", "codes", None, ()),
    Score("prdc", "codes", None, ()),
    Score("memorisation", "codes", "thumbnails", ("show",)))}


def fan_out(sinks):
    """one callable that hands a batch to every sink of one kind, in order; None for none"""
    def every(*batch):
        for sink in sinks:
            sink(*batch)
    return every if sinks else None


def encode_text(text_encoder, captions, cap_lens):
    """The text side of one batch (trainer.py:431-437): (words_embs, sent_emb, mask), both embeddings contiguous, the
    mask of the padding words cut to the word count the encoder returned.  Call it under torch.no_grad()."""
    hidden = text_encoder.init_hidden(captions.shape[0])
    words_embs, sent_emb = text_encoder(captions, cap_lens.cpu(), hidden)
    mask = (captions == 0)
    if mask.size(1) > words_embs.size(2):
        mask = mask[:, :words_embs.size(2)]
    return words_embs.contiguous(), sent_emb.contiguous(), mask


def generate_seeded(netG, gen, words_embs, sent_emb, mask, tmi, label_one_hot):
    """One 256x256 image per caption from the seeded device generator `gen`: `noise` (B, Z_DIM) is drawn first, then the
    conditioning noise `eps` (B, CONDITION_DIM) -- the order is a contract, r_precision and pool_codes see the same images
    under the same seed."""
    noise, eps = draw_noise(gen, sent_emb)
    return generate_from(netG, noise, eps, words_embs, sent_emb, mask, tmi, label_one_hot)


def draw_noise(gen, sent_emb):
    """generate_seeded's draws, in its order: (noise (B, Z_DIM), eps (B, CONDITION_DIM)) on sent_emb's device"""
    B = sent_emb.shape[0]
    noise = torch.randn(B, cfg.GAN.Z_DIM, device=sent_emb.device, generator=gen)
    eps = torch.randn(B, cfg.GAN.CONDITION_DIM, device=sent_emb.device, generator=gen)
    return noise, eps


def generate_from(netG, noise, eps, words_embs, sent_emb, mask, tmi, label_one_hot):
    """generate_seeded's generator call under given draws: layout_shift() calls it twice with one pair of draws and two layouts"""
    fake_imgs, _, _, _ = netG(noise, sent_emb, words_embs, mask, tmi, label_one_hot, eps=eps)
    return fake_imgs[-1]


def moved_matrices(tmi, table, boxes=None):
    """`tmi` (B, G, 2, 3) with the matrix of every moved slot of the edit table (layoutshift.ShiftResponse.edits) replaced by that
    of its moved box (hip/ops.bbox_to_theta; `boxes` (n, 4) where they are not the table's own); every other slot keeps its bits"""
    boxes = table["moved"] if boxes is None else boxes
    out = tmi.clone()
    if len(table["row"]):
        inv = ops.bbox_to_theta(boxes.to(tmi.device).float().contiguous())[1]
        out[table["row"].to(tmi.device), table["slot"].to(tmi.device)] = inv.to(tmi.dtype)
    return out


FID_NETWORK_NOTE = ("the trunk's weights are run as the published FID Inception network (trunk_variant fid: the PyTorch port of the 2015 "
                    "TensorFlow graph, pt_inception-2015-12-05 -- the pool branches of Mixed_5b..7b average the taps inside the "
                    "map, Mixed_7c's takes their maximum), so with that network's weights file the codes are the published kind; "
                    "the protocol remains this project's: fp32 images that are not quantised to 8 bits, and this data "
                    "pipeline's resize.")


def trainer_variant(trainer):
    """the trunk variant a trainer's passes run under (main.py --trunk_variant): "torchvision" unless it says otherwise"""
    return getattr(trainer, "trunk_variant", None) or "torchvision"


def trunk_note(what, figure, unit, variant="torchvision"):
    """the note of fid.json / kid.json / prdc.json: what the score is under an ImageNet trunk and under a random-init one"""
    if variant != "torchvision":
        return ("%s of Inception pool codes under the trunk file's weights: %s  %s under that network if the file holds its "
                "weights, %s in other features -- comparable between checkpoints under this trunk_digest only -- if it does not."
                % (what, FID_NETWORK_NOTE, figure, unit))
    return ("%s of Inception pool codes under the trunk of NET_E's image encoder: %s under torchvision's "
            "Inception-v3 if that trunk holds ImageNet weights (published figures mostly use the TF-ported network), %s "
            "in random convolutional features -- comparable between checkpoints under this trunk only -- if it is random-init."
            % (what, figure, unit))


class PooledCodes:
    """What fid(), kid() and prdc() do around their own device calls: the codes of one pass (pool_codes; or the `codes` a
    caller hands over, checked against `seed`) cut to their `n` filled rows as `real` / `fake`, the save directory, the JSON
    with the keys the three files share, and the return_codes result.  `want_real` is pool_codes' argument; where the
    real side is wanted and handed-over codes hold none, that is a ValueError (`or_else` ends its message)."""

    def __init__(self, trainer, who, split_dir, num_samples, seed, codes, want_real=True, or_else=""):
        if codes is None:
            codes = trainer.pool_codes(split_dir, num_samples, seed, want_real)
        else:
            if int(codes["seed"]) != int(seed):
                raise ValueError("%s: the codes were taken under seed %d, not %d" % (who, codes["seed"], seed))
            if callable(want_real):
                want_real = want_real(codes["trunk_digest"], int(codes["fake"].shape[1]))
            if not want_real:
                codes = dict(codes, real=None)
            elif codes["real"] is None:
                raise ValueError("%s: the codes handed over hold no real side%s" % (who, or_else))
        self.who, self.seed, self.n, self.digest, self.split_dir = who, int(seed), codes["n"], codes["trunk_digest"], split_dir
        self.variant = trainer_variant(trainer)
        self.real = None if codes["real"] is None else codes["real"][:self.n]
        self.fake = codes["fake"][:self.n]
        self.save_dir = eval_save_dir(split_dir)

    def write(self, out, n_real, n_fake, note):
        """adds the common keys to `out`, writes <save_dir>/<who>.json and returns `out`"""
        out.update({"n_real": None if n_real is None else int(n_real), "n_fake": int(n_fake), "trunk_digest": self.digest})
        if self.variant != "torchvision":                      # the default's files keep their key set
            out["trunk_variant"] = self.variant
        write_score(self.split_dir, self.who, out, self.seed, note)
        return out

    def result(self, out, return_codes):
        if return_codes:
            return out, {"real": None if self.real is None else self.real.cpu(), "fake": self.fake.cpu()}
        return out


THUMB = 64                   # side of the thumbnails of nn_grid.png
BANK_SEED_STEP = 1           # a synthetic split's training bank: a second synthetic set, under the split's seed plus this


class Thumbnails:
    """u8 THUMB x THUMB thumbnails of a pass's generated images on the host, in the pass's order (12 KB per image): `sink` is the
    (real, fake, take) callable of pool_codes' image_sink and halves the generated images with hip/ops.avg_down2 -- the aligned
    2 x 2 mean, twice for 256 x 256 -- until they are THUMB wide.  memorisation() shows its most suspicious rows from it."""

    def __init__(self):
        self.rows = []

    def sink(self, real, fake, take):
        t = fake[:take].float().contiguous()
        B, C, H, W = t.shape
        t = t.view(B * C, H, W)
        while t.shape[-1] > THUMB and t.shape[-1] % 2 == 0 and t.shape[-2] % 2 == 0:
            t = ops.avg_down2(t)
        self.rows.append(t.view(B, C, t.shape[-2], t.shape[-1]).add(1.0).mul(127.5).clamp(0, 255).byte().cpu())

    def __len__(self):
        return sum(int(r.shape[0]) for r in self.rows)

    def images(self, rows):
        """(len(rows), 3, h, w) u8, numpy"""
        every = torch.cat(self.rows)
        return every[torch.as_tensor(np.asarray(rows, dtype=np.int64))].numpy()


def thumbnail_u8(img):
    """a (3, H, W) image in [-1, 1] (host) as (3, h, w) u8 with h, w <= THUMB where H, W are THUMB times a power of two: the mean
    over aligned squares"""
    a = np.asarray(img, dtype=np.float32)
    while a.shape[-1] > THUMB and a.shape[-1] % 2 == 0 and a.shape[-2] % 2 == 0:
        a = ((a[:, 0::2, 0::2] + a[:, 0::2, 1::2]) + (a[:, 1::2, 0::2] + a[:, 1::2, 1::2])) / np.float32(4)
    return np.clip((a + 1.0) * 127.5, 0, 255).astype(np.uint8)


class CheckpointEvaluation(object):
    """The evaluation methods of condGANTrainer (reference trainer.py:387-579 and DESIGN.md sections 9c-9j)."""

    def _load_eval_models(self):
        """The two checkpoints of the evaluation paths (trainer.py:397-417, 483-505): EMA generator from
        cfg.TRAIN.NET_G["netG"], DAMSM text encoder from cfg.TRAIN.NET_E, both in eval mode."""
        netG = G_NET()
        netG.apply(weights_init)
        sd = torch.load(cfg.TRAIN.NET_G, map_location='cpu')
        netG.load_state_dict(sd["netG"])
        print('Load G from: ', cfg.TRAIN.NET_G)
        netG = netG.to(self.device).eval()
        text_encoder = RNN_ENCODER(self.n_words, nhidden=cfg.TEXT.EMBEDDING_DIM)
        if cfg.TRAIN.NET_E != '':
            text_encoder.load_state_dict(torch.load(cfg.TRAIN.NET_E, map_location='cpu'))
            print('Load text encoder from:', cfg.TRAIN.NET_E)
        return netG, text_encoder.to(self.device).eval()

    def _new_image_encoder(self):
        """A random-init image encoder on the host, heads TEXT.EMBEDDING_DIM wide as in training (outside training the reference's
        constructor fixes them at 256, model.py:213, which is the same thing for the published pairs only).  Its construction
        draws from torch's global generator: the state it leaves behind is the one every seeded pass shuffles its loader under."""
        nef = cfg.TEXT.EMBEDDING_DIM
        image_encoder = CNN_ENCODER(nef, pretrained=False)
        if image_encoder.nef != nef:
            image_encoder.nef = nef
            image_encoder.emb_features = type(image_encoder.emb_features)(768, nef, kernel_size=1, stride=1, padding=0, bias=False)
            image_encoder.emb_cnn_code = type(image_encoder.emb_cnn_code)(2048, nef)
            image_encoder.init_trainable_weights()
        return image_encoder

    def _load_image_encoder(self):
        """The image encoder that TRAIN.NET_E's text encoder was trained with: the `image_encoder` twin of its path, by
        build_models' rule and with its error, frozen, on the device, in eval mode."""
        image_encoder = self._host_image_encoder()
        for p in image_encoder.parameters():
            p.requires_grad = False
        return image_encoder.to(self.device).eval()

    def _state_file(self, path):
        """the state dict in `path`; a method that has read the file already for its own ends (inception_score(): the head) leaves it
        in `_state_read` for the length of its pass, so one file is read once"""
        from .inception import read_state_file
        read = getattr(self, "_state_read", None)
        return read[1] if read is not None and read[0] == path else read_state_file(path)

    def _host_image_encoder(self):
        """_load_image_encoder's encoder on the host, weights and buffers as the pass will run them: constructed, NET_E's image
        encoder loaded, then the trunk of the trainer's `trunk_path`"""
        image_encoder = self._new_image_encoder()
        if cfg.TRAIN.NET_E != '':
            img_path = cfg.TRAIN.NET_E.replace('text_encoder', 'image_encoder')
            for path in (cfg.TRAIN.NET_E, img_path):
                if not os.path.isfile(path):
                    raise FileNotFoundError("DAMSM encoder checkpoint not found: %s (cwd %s)" % (path, os.getcwd()))
            image_encoder.load_state_dict(torch.load(img_path, map_location='cpu'))
            print('Load image encoder from:', img_path)
        trunk_path = getattr(self, "trunk_path", None)
        if trunk_path:
            # after the construction, whose draws every seeded pass shuffles its loader behind (_load_seeded): the images of a pass
            # under a trunk file are those of the pass without it.  One pass runs under one trunk: beside NET_E's pair the file
            # must hold that pair's trunk.
            from .fid import trunk_digest
            from .inception import load_trunk_state
            variant = trainer_variant(self)
            own = trunk_digest(image_encoder) if cfg.TRAIN.NET_E != '' and variant == "torchvision" else None
            state = self._state_file(trunk_path)
            load_trunk_state(image_encoder, state, trunk_path)
            print('Load Inception trunk from:', trunk_path)
            if variant != "torchvision":
                # the pool-code scores touch no DAMSM head: beside NET_E's pair the file's trunk REPLACES that pair's (the check
                # below is the default variant's), and the weights run as the variant's network
                image_encoder.set_trunk_variant(variant)
            elif "fc.weight" in state and state["fc.weight"].dim() == 2 and state["fc.weight"].shape[0] == 1008 \
                    and not getattr(self, "_said_fid_file", False):
                self._said_fid_file = True                     # once per trainer: a score may build its encoder twice
                print("%s has a 1008-way head: it looks like the published FID Inception network's file, which runs as that network "
                      "under --trunk_variant fid; this pass runs its weights with torchvision's pooling" % trunk_path)
            if own is not None and trunk_digest(image_encoder) != own:
                raise ValueError("--trunk %s holds another Inception trunk (digest %s...) than NET_E's image encoder (%s...): one "
                                 "pass runs under one trunk" % (trunk_path, trunk_digest(image_encoder)[:12], own[:12]))
        return image_encoder

    def _load_seeded(self, seed, trunk=True):
        """The networks of the seeded paths under torch.manual_seed(seed) (which fixes the random-init encoders of an empty
        NET_E) and the device generator the noise comes from: (netG, text_encoder, image_encoder, generator).  trunk=False: no
        image encoder (None) -- no checkpoint of it is read, nothing of it reaches the device or runs; its random initialisation
        alone is still drawn on the host and dropped, because a shuffling loader takes its order from the global generator's state
        after it: a pass without the trunk sees the batches, and so the generated images, of a pass with it."""
        torch.manual_seed(seed)
        netG, text_encoder = self._load_eval_models()
        if trunk:
            image_encoder = self._load_image_encoder()
        else:
            image_encoder = None
            self._new_image_encoder()
        gen = torch.Generator(device=self.device)
        gen.manual_seed(seed)
        return netG, text_encoder, image_encoder, gen

    def sampling(self, split_dir, num_samples=30000):
        """trainer.py:387-470: load cfg.TRAIN.NET_G (EMA generator of a checkpoint) and cfg.TRAIN.NET_E (DAMSM text
        encoder), generate one 256x256 image per caption of the data loader with netG.eval() and save it as
        <NET_G minus .pth>/<split>/single/<key>_s<batch index>.png"""
        from PIL import Image
        from .datasets import prepare_data
        if net_g_missing('morels'):
            return None
        netG, text_encoder = self._load_eval_models()
        save_dir = eval_save_dir(split_dir)
        written = []
        for step, data in enumerate(self.data_loader, 0):
            if step >= num_samples:
                break
            imgs, captions, cap_lens, class_ids, keys, (tm, tmi), label_one_hot = prepare_data(data, self.device)
            B = captions.shape[0]
            with torch.no_grad():
                words_embs, sent_emb, mask = encode_text(text_encoder, captions, cap_lens)
                noise = torch.randn(B, cfg.GAN.Z_DIM, device=self.device)
                fake_imgs, _, _, _ = netG(noise, sent_emb, words_embs, mask, tmi, label_one_hot)
            out = fake_imgs[-1].add(1.0).mul(127.5).clamp(0, 255).byte().permute(0, 2, 3, 1).cpu().numpy()
            for j in range(B):
                s_tmp = '%s/single/%s' % (save_dir, keys[j])
                mkdir_p(s_tmp[:s_tmp.rfind('/')] if '/' in keys[j] else '%s/single' % save_dir)
                fullpath = '%s_s%d.png' % (s_tmp, step)
                Image.fromarray(out[j]).save(fullpath)
                written.append(fullpath)
        return written

    def r_precision(self, split_dir, num_samples=30000, n_mismatched=99, folds=10, seed=100, real=False, return_codes=False):
        """R-precision of the checkpoint TRAIN.NET_G under the DAMSM pair TRAIN.NET_E: one 256x256 image per
        caption of the data loader (EMA generator, eval mode, seeded noise) -- or, with real=True, the real 256x256 image: the
        ceiling the encoder pair allows --, its image code ranked against its own caption and `n_mismatched` captions of other
        images of the split (hip/ops.retrieval_rank, one launch per batch; the ranks stay on the device until the end).
        `seed` fixes the noise, the mismatched draws, the bank's long-caption subsets and, with an empty NET_E, the random-init
        encoders.  A split with fewer than `n_mismatched` captions of other images is ranked against as many as it has.
        Writes <NET_G minus .pth>/<split>/r_precision.json and returns its content; with return_codes also a dict of host
        tensors: the image codes "code", "pos", "idx", the ranks "rank" and the "bank" the rows of idx point into."""
        from .datasets import prepare_data
        from .retrieval import SentenceBank, draw_mismatched, fold_stats
        if net_g_missing():
            return None
        if trainer_variant(self) != "torchvision":
            raise ValueError("r_precision: the score runs the DAMSM heads on torchvision's trunk; the trunk variant %r serves the "
                             "scores on pool codes only" % trainer_variant(self))
        netG, text_encoder, image_encoder, gen = self._load_seeded(seed)
        save_dir = eval_save_dir(split_dir)
        bank = SentenceBank.from_dataset(text_encoder, self.data_loader.dataset, cfg.TEXT.WORDS_NUM, seed)
        usable = len(bank) - int(np.bincount(bank.image_index).max())       # captions of other images, for the fullest image
        if usable < 1:
            raise ValueError("r_precision: the split holds no caption of another image to rank against")
        if n_mismatched > usable:
            print("R-precision: the split has %d captions of other images per query, not %d -- ranking against %d (a smaller "
                  "candidate set gives a HIGHER figure; the JSON records it)" % (usable, n_mismatched, usable))
            n_mismatched = usable
        rng = np.random.RandomState(seed)
        ranks, codes, poss, idxs, n = [], [], [], [], 0
        for data in self.data_loader:
            if n >= num_samples:
                break
            imgs, captions, cap_lens, class_ids, keys, (tm, tmi), label_one_hot = prepare_data(data, self.device)
            with torch.no_grad():
                words_embs, sent_emb, mask = encode_text(text_encoder, captions, cap_lens)
                img = imgs[-1] if real else generate_seeded(netG, gen, words_embs, sent_emb, mask, tmi, label_one_hot)
                code = image_encoder(img)[1]
                idx = draw_mismatched(bank.image_index, bank.images_of(keys), n_mismatched, rng)
                ranks.append(ops.retrieval_rank(code, sent_emb, bank.bank, idx))
            if return_codes:
                codes.append(code); poss.append(sent_emb); idxs.append(torch.from_numpy(idx))
            n += captions.shape[0]
        if not ranks:
            raise ValueError("r_precision: the data loader gave no batch")
        rank = torch.cat(ranks)[:num_samples].cpu()                      # the one read-back
        out = fold_stats(rank.numpy(), folds)
        out.update({"n_mismatched": int(n_mismatched), "seed": int(seed), "real": bool(real), "NET_G": cfg.TRAIN.NET_G,
                    "NET_E": cfg.TRAIN.NET_E})
        write_json(save_dir, "r_precision", out)
        print("R-precision (%s images, %d queries, %d mismatched): %.4f, folds %.4f +- %.4f -> %s/r_precision.json"
              % ("real" if real else "generated", out["n"], n_mismatched, out["r_precision"], out["mean"], out["std"], save_dir))
        if return_codes:
            k = rank.numel()
            return out, {"code": torch.cat(codes)[:k].cpu(), "pos": torch.cat(poss)[:k].cpu(), "idx": torch.cat(idxs)[:k],
                         "rank": rank, "bank": bank.bank.cpu()}
        return out

    def pool_codes(self, split_dir, num_samples=30000, seed=100, want_real=True, image_sink=None, trunk=True, resample_sink=None,
                   object_sink=None, generate=None):
        """The one pass over the data loader that the scores share: the real 256x256 image and one generated 256x256 image per
        caption (EMA generator, eval mode, noise from the seeded device generator exactly as r_precision draws it) go through
        CNN_ENCODER.pool_code; the codes stay on the device in two preallocated (num_samples, 2048) fp32 buffers.  `want_real`
        False leaves the real images out of the trunk; it may also be a callable (trunk digest, code width) -> bool, asked once the
        image encoder is loaded and before the pass (fid() decides there whether a statistics file replaces the real side).
        `split_dir` names the split the data loader was built for; the pass itself reads the loader only.
        Returns a dict: "real" (None where not wanted) and "fake", the device buffers, of which the first "n" rows are filled;
        "trunk_digest"; the "seed" the pass ran under.  None, with fid()'s message, where TRAIN.NET_G is empty.
        `image_sink`, where given, is called once per batch with (real, fake, take): the real and the generated 256x256 images of
        the batch on the device and the number of leading images that count (swd() gathers its descriptors there).  trunk=False
        leaves the image encoder out altogether -- not loaded, not run; "real", "fake" and "trunk_digest" are then None -- and the
        images, their order and "n" are those of a pass with it.
        `resample_sink`, where given, makes the pass generate a SECOND image per caption right after the batch's first one -- the
        same text, boxes and labels, noise and then eps (generate_seeded's order) from a device generator of its own seeded
        `seed` + 1 -- and is called with (fake, fake_again, take) (msssim() scores how much the noise changes there).  The first
        generator's draws, and so the images every other score sees, are those of a pass without it.
        `object_sink`, where given, is called once per batch with (real, fake, tm, take, image_encoder): the images as for
        `image_sink`, the batch's box matrices `tm` (B, 3, 2, 3) on the device and the pass's image encoder (scene_fid() cuts the
        objects out there and runs the trunk on them).  It needs the trunk: ValueError with trunk=False.  It draws nothing, so
        every other score's images and codes are those of a pass without it.
        `generate`, where given, makes a batch's image in generate_seeded's place: it is called with (netG, gen, words_embs, sent_emb,
        mask, tm, tmi, label_one_hot, keys, take) and owes the pass generate_seeded's draws and image (layout_shift() generates a
        second image from the same draws there)."""
        from .datasets import prepare_data
        from .fid import trunk_digest
        if object_sink is not None and not trunk:
            raise ValueError("pool_codes: an object_sink needs the image encoder, trunk=False leaves it out")
        if net_g_missing():
            return None
        netG, text_encoder, image_encoder, gen = self._load_seeded(seed, trunk)
        rows = self.pass_shape(num_samples)[1]
        digest = fake_codes = real_codes = None
        if trunk:
            D = int(image_encoder.emb_cnn_code.weight.shape[1])             # 2048: the pooled code's width
            digest = trunk_digest(image_encoder)
            if callable(want_real):
                want_real = want_real(digest, D)
            fake_codes = torch.empty((rows, D), dtype=torch.float32, device=self.device)
            real_codes = torch.empty((rows, D), dtype=torch.float32, device=self.device) if want_real else None
        gen_again = None
        if resample_sink is not None:
            gen_again = torch.Generator(device=self.device)
            gen_again.manual_seed(int(seed) + 1)
        n = 0
        for data in self.data_loader:
            if n >= rows:
                break
            imgs, captions, cap_lens, class_ids, keys, (tm, tmi), label_one_hot = prepare_data(data, self.device)
            take = min(captions.shape[0], rows - n)
            with torch.no_grad():
                words_embs, sent_emb, mask = encode_text(text_encoder, captions, cap_lens)
                if generate is None:
                    fake = generate_seeded(netG, gen, words_embs, sent_emb, mask, tmi, label_one_hot)
                else:
                    fake = generate(netG, gen, words_embs, sent_emb, mask, tm, tmi, label_one_hot, keys, take)
                if resample_sink is not None:
                    resample_sink(fake, generate_seeded(netG, gen_again, words_embs, sent_emb, mask, tmi, label_one_hot), take)
                if trunk:
                    fake_codes[n:n + take] = image_encoder.pool_code(fake)[:take]
                    if real_codes is not None:
                        real_codes[n:n + take] = image_encoder.pool_code(imgs[-1])[:take]
                if image_sink is not None:
                    image_sink(imgs[-1], fake, take)
                if object_sink is not None:
                    object_sink(imgs[-1], fake, tm, take, image_encoder)
            n += take
        return {"real": real_codes, "fake": fake_codes, "n": n, "trunk_digest": digest, "seed": int(seed)}

    def pass_shape(self, num_samples):
        """(size, images) of a pass: the side of the tree's final resolution and how many images the pass will see at most"""
        return cfg.TREE.BASE_SIZE << (cfg.TREE.BRANCH_NUM - 1), max(1, min(int(num_samples), len(self.data_loader.dataset)))

    def shared_pass(self, split_dir, num_samples, seed, accs):
        """pool_codes for the scores `accs` names (score -> its accumulator or None), every keyword derived from SCORES: the trunk runs
        where a score takes codes or objects, on the real images where one takes codes; the sinks are composed per kind in table order"""
        takes = {SCORES[name].takes for name in accs}
        made = [(SCORES[name].takes == "objects", accs[name]) for name in SCORES if accs.get(name) is not None]
        return self.pool_codes(
            split_dir, num_samples, seed, want_real="codes" in takes, trunk=bool(takes & {"codes", "objects"}),
            image_sink=fan_out([acc.sink for boxes, acc in made if not boxes]),
            object_sink=fan_out([acc.sink for boxes, acc in made if boxes]),
            resample_sink=fan_out([acc.resample_sink for _, acc in made if getattr(acc, "resample_sink", None) is not None]))

    def fed(self, who, split_dir, num_samples, acc, **params):
        """The hand-over rule of the scores with an accumulator: `acc` None -- the score's factory makes one under `params` and a pass of
        the score's own feeds it; else a pass the caller shared has fed it, and it must have been made under `params`.  Returns it."""
        if acc is None:
            acc = getattr(self, SCORES[who].factory)(num_samples, **params)
            self.shared_pass(split_dir, num_samples, params["seed"], {who: acc})
        elif acc.params != params:
            raise ValueError("%s: the accumulator handed over was made under other parameters (%s) = %s"
                             % (who, ", ".join(acc.params), tuple(acc.params.values())))
        return acc

    def run_scores(self, split_dir, asked, num_samples=30000, seed=100):
        """The scores `asked` names (score -> its own keyword arguments) from ONE pass: the accumulators are made, shared_pass runs once,
        each score finishes in table order from what it is handed.  One score alone runs its own method without a hand-over (fid() may
        then keep the real images out of the trunk, swd(), msssim() and spectrum() load no image encoder).  Returns score -> result."""
        if not asked or set(asked) - set(SCORES):
            raise ValueError("run_scores: one score at least of %s expected, got %s" % (list(SCORES), list(asked)))
        if len(asked) == 1:
            (name, kw), = asked.items()
            return {name: getattr(self, name)(split_dir, num_samples, seed, **kw)}
        if net_g_missing():
            return None
        accs = {}
        for row in (SCORES[name] for name in SCORES if name in asked):
            kw = {k: asked[row.name][k] for k in row.params if k in asked[row.name]}
            accs[row.name] = row.factory and getattr(self, row.factory)(num_samples, seed, **kw)
        codes = self.shared_pass(split_dir, num_samples, seed, accs)
        out = {}
        for name, acc in accs.items():
            takes = SCORES[name].takes
            handed = acc if takes != "codes" else codes if acc is None else dict(codes, thumbnails=acc)
            out[name] = getattr(self, name)(split_dir, num_samples, seed, **dict(asked[name], **{takes: handed}))
        return out

    def fid(self, split_dir, num_samples=30000, seed=100, stats_path=None, return_codes=False, codes=None):
        """Frechet distance between real and generated images of the checkpoint TRAIN.NET_G in the Inception pool codes of
        TRAIN.NET_E's image encoder: the codes of ONE pass over the data loader (pool_codes; or the `codes`
        a caller hands over from a pass of its own, which kid() can share) stay on the device, their
        fp64 mean and covariance come from hip/ops.feature_moments after the loop and the distance from fid.frechet_distance on
        the host.  With `stats_path` the real side is loaded from that file when it exists and was taken under the same trunk
        (the real images then skip the trunk), and computed and saved there otherwise.  With a trunk that holds torchvision's
        ImageNet weights the figure is FID under torchvision's Inception-v3; with a random-init trunk it is a Frechet distance in
        random convolutional features, comparable between checkpoints under the same trunk only.
        Writes <NET_G minus .pth>/<split>/fid.json and returns its content; with return_codes also a dict of the two code matrices
        on the host, "real" (None where the real side was loaded) and "fake"."""
        from .fid import FeatureStats, frechet_distance, is_external_stats, load_external_stats
        if net_g_missing():
            return None
        loaded = []
        variant = trainer_variant(self)

        def want_real(digest, D):
            if stats_path is not None and os.path.isfile(stats_path):
                if is_external_stats(stats_path):
                    # a TTUR / pytorch-fid file (mu, sigma): read under the published network only, never written
                    if variant != "fid":
                        raise ValueError("%s holds published statistics (mu, sigma): they are accepted under --trunk_variant fid only"
                                         % stats_path)
                    mu, sigma = load_external_stats(stats_path, D)
                    loaded.append(FeatureStats(mu, sigma, 0, "external"))
                    print('Load published real-image statistics from: %s (network and protocol unverified)' % stats_path)
                else:
                    loaded.append(FeatureStats.load(stats_path, digest, D))     # ValueError for another trunk's file
                    print('Load real-image statistics from: %s (%d images)' % (stats_path, loaded[0].n))
            return not loaded
        c = PooledCodes(self, "fid", split_dir, num_samples, seed, codes, want_real, " and there is no statistics file")
        n, D = c.n, int(c.fake.shape[1])
        if n < 2:
            raise ValueError("fid: the data loader gave %d images; a covariance needs two at least" % n)
        fake_stats = FeatureStats(*[t.cpu() for t in ops.feature_moments(c.fake)], n, c.digest)
        if loaded:
            real_stats = loaded[0]
        else:
            real_stats = FeatureStats(*[t.cpu() for t in ops.feature_moments(c.real)], n, c.digest)
            if stats_path is not None:
                real_stats.save(stats_path)
                print('Save real-image statistics to: %s' % stats_path)
        dist, terms = frechet_distance(real_stats.mean, real_stats.cov, fake_stats.mean, fake_stats.cov)
        external = bool(loaded) and loaded[0].trunk_digest == "external"
        few = fake_stats.n if external else min(real_stats.n, fake_stats.n)
        note = trunk_note("Frechet distance", "FID", "a distance", variant)
        if external:
            note += (" The real side is the published statistics file %s: the network and the protocol it was computed under are "
                     "unverified, and the number of its images is unknown." % stats_path)
        if few < D:
            note += (" n = %d < %d features: the covariances are rank-deficient, so the figure is biased and only comparable "
                     "at equal n." % (few, D))
            print("FID: %d images for %d features -- the covariances are rank-deficient, the figure is biased and only comparable "
                  "at equal n (the JSON records it)" % (few, D))
        out = c.write(dict(terms, fid=dist, **({"real_stats": "external"} if external else {})),
                      None if external else real_stats.n, fake_stats.n, note)
        print("FID (%s real, %d generated images): %.4f = |dmu|^2 %.4f + Tr S_real %.4f + Tr S_fake %.4f - 2 x %.4f -> %s/fid.json"
              % (out["n_real"], out["n_fake"], dist, terms["mean_sq"], terms["tr_s1"], terms["tr_s2"], terms["tr_sqrt"], c.save_dir))
        return c.result(out, return_codes)

    def kid(self, split_dir, num_samples=30000, seed=100, subsets=100, subset_size=1000, codes=None, return_codes=False):
        """Kernel Inception distance between real and generated images of the checkpoint TRAIN.NET_G in the Inception pool codes
        of TRAIN.NET_E's image encoder: the unbiased estimate of the squared maximum mean discrepancy under
        k(a, b) = (<a, b> / D + 1)^3, averaged over `subsets` random subset pairs of `subset_size` codes each (kid.draw_subsets
        under `seed`; the size is lowered to the number of images where there are fewer).  The codes are those of fid() -- ONE
        pass over the data loader (pool_codes), or the `codes` a caller hands over from a pass of its own -- and stay on the device;
        the three sums per subset pair come from hip/ops.poly_mmd_sums in one call, the figure from kid.kid_from_sums on the host.
        Unlike the Frechet distance the estimator has no bias that depends on n; it may be negative.  The real images always go
        through the trunk.  Writes <NET_G minus .pth>/<split>/kid.json and returns its content; with return_codes also a dict of
        the two code matrices on the host, "real" and "fake"."""
        from . import kid as KID
        if net_g_missing():
            return None
        c = PooledCodes(self, "kid", split_dir, num_samples, seed, codes)
        n, D = c.n, int(c.fake.shape[1])
        s = KID.subset_size(n, n, subset_size)
        ix, iy = KID.draw_subsets(n, n, subsets, s, seed)
        gamma = 1.0 / D
        sums = ops.poly_mmd_sums(c.real, c.fake, ix, iy, gamma=gamma, coef0=KID.COEF0).cpu().numpy()   # the one read-back
        mean, std, _ = KID.kid_from_sums(sums, s)
        note = trunk_note("Kernel Inception distance (unbiased MMD^2 under the cubic polynomial kernel, mean over subset pairs)",
                          "KID", "a distance", c.variant)
        if s < int(subset_size):
            note += (" subset_size lowered from %d to %d: there are only %d images per side." % (subset_size, s, n))
            print("KID: %d images per side -- subsets of %d codes instead of %d (the JSON records it)" % (n, s, subset_size))
        out = c.write({"kid": mean, "kid_std": std, "subsets": int(subsets), "subset_size": int(s), "gamma": gamma,
                       "coef0": float(KID.COEF0), "degree": int(KID.DEGREE)}, n, n, note)
        print("KID (%d real, %d generated images; %d subset pairs of %d): %.6f +- %.6f -> %s/kid.json"
              % (n, n, out["subsets"], s, mean, std, c.save_dir))
        return c.result(out, return_codes)

    def prdc(self, split_dir, num_samples=30000, seed=100, k_pr=3, k_dc=5, codes=None, return_codes=False):
        """Improved precision / recall (k_pr nearest neighbours) and density / coverage (k_dc) between real and generated images of
        the checkpoint TRAIN.NET_G in the Inception pool codes of TRAIN.NET_E's image encoder (attngan/prdc.py
        has the definitions): where the Frechet distance and KID give one number, these tell a generator whose images are sharp but
        alike (precision high, recall low) from one whose images are varied but poor.  The codes are those of fid() -- ONE pass over
        the data loader (pool_codes), or the `codes` a caller hands over from a pass of its own -- and stay on the device: two
        calls of hip/ops.knn_sqdist give every code's radii inside its own set, three of hip/ops.ball_counts the memberships
        between the sets, and the counts are read back once; the k's are lowered to n - 1 where there are fewer images.  All four
        figures depend on n.  The real images always go through the trunk.  Writes <NET_G minus .pth>/<split>/prdc.json and
        returns its content; with return_codes also a dict of the two code matrices on the host, "real" and "fake"."""
        from . import prdc as PRDC
        if net_g_missing():
            return None
        c = PooledCodes(self, "prdc", split_dir, num_samples, seed, codes)
        n, real_codes, fake_codes = c.n, c.real, c.fake
        if n < 2:
            raise ValueError("prdc: the data loader gave %d images; a nearest neighbour needs two at least" % n)
        kp, kd = PRDC.neighbours(n, n, k_pr, k_dc)
        real_r2 = ops.knn_sqdist(real_codes, max(kp, kd))                                  # every real code's radii, both k's
        fake_r2 = ops.knn_sqdist(fake_codes, kp)
        fake_in_real = ops.ball_counts(fake_codes, real_codes, real_r2[:, [kp - 1, kd - 1]].contiguous(), "support")
        real_in_fake = ops.ball_counts(real_codes, fake_codes, fake_r2[:, kp - 1].contiguous(), "support")
        real_own = ops.ball_counts(real_codes, fake_codes, real_r2[:, kd - 1].contiguous(), "query")
        counts = torch.cat([fake_in_real, real_in_fake, real_own], dim=1).cpu().numpy()      # (n, 4): the one read-back
        scores = PRDC.scores_from_counts(counts[:, 0:2], counts[:, 2], counts[:, 3], kd)
        note = trunk_note("Improved precision / recall (k_pr nearest neighbours) and density / coverage (k_dc)",
                          "the published scores", "scores", c.variant)
        note += " All four figures depend on the number of images and are comparable at equal n only."
        for name, asked, k in (("k_pr", k_pr, kp), ("k_dc", k_dc, kd)):
            if k < int(asked):
                note += (" %s lowered from %d to %d: there are only %d images per side." % (name, asked, k, n))
                print("PRDC: %d images per side -- %s = %d instead of %d (the JSON records it)" % (n, name, k, asked))
        out = c.write(dict(scores, k_pr=int(kp), k_dc=int(kd)), n, n, note)
        print("PRDC (%d real, %d generated images; k = %d / %d): precision %.4f recall %.4f density %.4f coverage %.4f -> %s/prdc.json"
              % (n, n, kp, kd, out["precision"], out["recall"], out["density"], out["coverage"], c.save_dir))
        return c.result(out, return_codes)

    def swd_images(self, num_samples=30000, seed=100, patches=128, dirs=128, repeats=4, min_res=16):
        """The accumulator swd() fills: attngan/swd.SlicedWasserstein for the tree's final resolution and as many images as the
        pass will see, whose `sink` is the (real, fake, take) callable pool_codes' image_sink wants.  A caller that shares one pass
        between swd() and other scores makes it first and hands it to both (run_scores)."""
        from .swd import SlicedWasserstein
        size, images = self.pass_shape(num_samples)
        acc = SlicedWasserstein(size, 3, images * int(patches), patches, dirs, repeats, min_res, seed, self.device)
        print("SWD: %.2f GB of descriptors on the device (%d levels x 2 sides x %d rows x %d values, fp32)"
              % (acc.bytes / 1e9, len(acc.sizes), acc.rows, acc.desc["real"][0].shape[1]))
        return acc

    def swd(self, split_dir, num_samples=30000, seed=100, patches=128, dirs=128, repeats=4, min_res=16, images=None):
        """Sliced Wasserstein distance (Karras et al. 2018; attngan/swd.py has the definition and the draw
        order) between the real 256x256 images and one generated image per caption of the checkpoint TRAIN.NET_G -- exactly the
        images pool_codes and r_precision see under `seed` -- at every level of a Laplacian pyramid from 256 down to `min_res`.
        The score reads the images themselves: it needs no image encoder, and pool_codes runs without one (trunk=False) unless
        the caller shares a pass: `images` is then the accumulator of swd_images() whose sink that pass has fed.  Pyramid,
        descriptors, moments, projections and the reduction run in hip/ops; the sort is torch.sort.  Writes
        <NET_G minus .pth>/<split>/swd.json and returns its content."""
        if net_g_missing():
            return None
        images = self.fed("swd", split_dir, num_samples, images, seed=int(seed), patches=int(patches), dirs=int(dirs),
                          repeats=int(repeats), min_res=int(min_res))
        if images.n < 1:
            raise ValueError("swd: the data loader gave no batch")
        res = images.result()
        n = images.n // images.patches
        out = {"swd": res["swd"], "levels": res["levels"], "per_level": res["per_level"], "patches": images.patches,
               "dirs": images.dirs, "repeats": images.repeats, "n_real": n, "n_fake": n}
        save_dir = write_score(
            split_dir, "swd", out, seed,
            "Sliced Wasserstein distance x 1000 between Laplacian-pyramid descriptors (7x7 neighbourhoods) of the real "
            "and the generated images, per level and averaged: trunk-free -- no image encoder is involved, the figure "
            "does not depend on any encoder weights.  It depends on the number of descriptors per image (patches = "
            "%d), on dirs, repeats and the seed, and is comparable under equal settings only.  The images enter as "
            "fp32 in [-1, 1], not quantised to 8 bits as in Karras et al.'s code." % images.patches)
        print("SWD (%d real, %d generated images; %d patches, %d directions, %d repeats): %.4f = mean of %s at levels %s -> %s/swd.json"
              % (n, n, images.patches, images.dirs, images.repeats, out["swd"], ["%.4f" % v for v in out["per_level"]],
                 out["levels"], save_dir))
        return out

    def msssim_images(self, num_samples=30000, seed=100, scales=5, same_caption=True):
        """The accumulator msssim() fills, as swd_images() is swd()'s: attngan/msssim.PairFigures for the tree's final resolution and as
        many pairs as the pass can give"""
        from .msssim import PairFigures
        size, images = self.pass_shape(num_samples)
        return PairFigures(size, 3, images, scales, same_caption, seed, self.device)

    def msssim(self, split_dir, num_samples=30000, seed=100, scales=5, same_caption=True, images=None):
        """Multi-scale structural similarity between PAIRS of images (Wang et al. 2003 as Odena et al. 2017 use it; DESIGN.md section
        9h; attngan/msssim.py has the definition), the trunk-free score for variation: "real", pairs of real 256x256 images -- the
        data's own figure, the floor a generator should reach; "generated", the same pairs of the images pool_codes and
        r_precision see under `seed` -- higher than "real" means less varied than the data; and, with `same_caption`,
        "same_caption": every caption's image against a second image for the same text, boxes and labels under fresh z and
        conditioning noise (pool_codes' resample_sink) -- a value near 1 means the generator ignores its noise, which no score
        that draws one image per caption can see.  No image encoder is involved, and pool_codes runs without one (trunk=False)
        unless the caller shares a pass: `images` is then the accumulator of msssim_images() whose sinks that pass has fed.
        Every level's filtering and sums run in hip/ops.ssim_level; the terms are read back once per figure.  Writes
        <NET_G minus .pth>/<split>/msssim.json and returns its content."""
        if net_g_missing():
            return None
        images = self.fed("msssim", split_dir, num_samples, images, seed=int(seed), scales=int(scales), same_caption=bool(same_caption))
        if any(f.n < 1 for f in images.figures.values()):
            raise ValueError("msssim: the data loader gave no pair of images")
        out = {}
        for name, f in images.figures.items():
            res = f.result()
            out[name] = {"mean": res["mean"], "std": res["std"], "ssim": res["ssim"], "cs": res["cs"], "pairs": res["pairs"],
                         "clamped": res["clamped"]}
        out.update({"levels": list(images.figures["real"].sizes), "scales": images.scales})
        save_dir = write_score(
            split_dir, "msssim", out, seed,
            "Multi-scale structural similarity between pairs of images, mean and population standard deviation over "
            "the pairs, with the per-level means of ssim and cs: trunk-free -- no image encoder is involved.  "
            "HIGHER means LESS varied.  real / generated: within a batch row j against row j + take // 2; the "
            "batches are sorted by caption length, so a pair's captions are of similar length.  same_caption: "
            "two images for one caption, boxes and labels under independent noise; near 1 means the generator "
            "ignores its noise.  A pair with a negative level mean scores 0 and is counted as clamped.  The images "
            "enter as fp32 in [-1, 1], not quantised to 8 bits.")
        print("MS-SSIM (%d scales; mean +- std over pairs): %s -> %s/msssim.json"
              % (images.scales, ", ".join("%s %.4f +- %.4f (%d pairs)" % (k, out[k]["mean"], out[k]["std"], out[k]["pairs"])
                                          for k in ("real", "generated", "same_caption") if k in out), save_dir))
        return out

    def spectrum_images(self, num_samples=30000, seed=100, window="hann"):
        """The accumulator spectrum() fills, as swd_images() is swd()'s: attngan/spectrum.RadialSpectrum for the tree's final resolution
        and as many images as the pass will see"""
        from .spectrum import RadialSpectrum
        size, images = self.pass_shape(num_samples)
        return RadialSpectrum(size, 3, images, window, self.device, seed=seed)

    def spectrum(self, split_dir, num_samples=30000, seed=100, window="hann", images=None):
        """Radial power spectrum (the azimuthally averaged power spectrum of Durall et al. 2020, Dzanic et al. 2020, Schwarz et al.
        2021; attngan/spectrum.py has the definition) of the real 256x256 images against one generated image per
        caption of the checkpoint TRAIN.NET_G -- exactly the images pool_codes and r_precision see under `seed`: the one score that
        looks at the images in the frequency domain, where the generator's nearest-neighbour upsamplings leave grids and
        checkerboards of period 2, 4 and 8 that a random-init trunk can miss and SWD cannot place.  It reads the images
        themselves: no image encoder is involved, and pool_codes runs without one (trunk=False) unless the caller shares a pass:
        `images` is then the accumulator of spectrum_images() whose sink that pass has fed.  The transform and the sums per bin
        run in hip/ops.radial_power, one call per side and batch, fp64; the per-image sums are read back once.  The score draws
        nothing.  Writes <NET_G minus .pth>/<split>/spectrum.json and returns its content."""
        from .spectrum import window_name
        if net_g_missing():
            return None
        images = self.fed("spectrum", split_dir, num_samples, images, seed=int(seed), window=window_name(window))
        if images.n < 1:
            raise ValueError("spectrum: the data loader gave no batch")
        out = images.result()
        n = out.pop("n")
        out.update({"size": images.size, "window": images.window, "n_real": n, "n_fake": n})
        save_dir = write_score(
            split_dir, "spectrum", out, seed,
            "Radial (azimuthally averaged) power spectrum of the luminance of the real and the generated images, in dB "
            "per bin of integer radius, with the log-spectral distance lsd_db, the ratio of the power above a "
            "quarter of the sampling frequency hf_db (positive: too much fine-scale power -- noise, grids; negative: "
            "blur), the spectral slopes and the bin of the largest excess with its period in pixels: trunk-free -- "
            "no image encoder is involved.  Every figure depends on the window (%s) and is comparable under the "
            "same window only.  The images enter as fp32 in [-1, 1], not quantised to 8 bits.  Bins beyond S / 2 "
            "cover partial rings only (the corners of the frequency square; the period-2 checkerboard is the last "
            "bin)." % images.window)
        def shown(v, form):                                     # a figure none of whose bins holds power is None
            return "n/a" if v is None else form % v
        print("Spectrum (%d real, %d generated images; window %s): LSD %.4f dB, HF %s dB, slopes %s / %s dB per decade, peak "
              "%+.2f dB at bin %d (period %.2f px) -> %s/spectrum.json"
              % (n, n, images.window, out["lsd_db"], shown(out["hf_db"], "%+.4f"), shown(out["slope_real"], "%.2f"),
                 shown(out["slope_fake"], "%.2f"), out["peak"]["excess_db"], out["peak"]["bin"], out["peak"]["period"], save_dir))
        return out

    def scene_fid_objects(self, num_samples=30000, seed=100, min_side=1):
        """The accumulator scene_fid() fills: attngan/scenefid.ObjectCodes for the tree's final resolution, as many images as the
        pass will see and the loader's batch size as the one batch shape the trunk runs at, whose `sink` is the (real, fake, tm, take,
        image_encoder) callable of pool_codes' object_sink; shared as swd_images() is"""
        from .scenefid import ObjectCodes
        size, images = self.pass_shape(num_samples)
        return ObjectCodes(images, int(self.data_loader.batch_size), size, min_side, seed, self.device)

    def scene_fid(self, split_dir, num_samples=30000, seed=100, min_side=1, objects=None, return_codes=False):
        """Object-level Frechet distance (SceneFID, Sylvain et al. 2021; attngan/scenefid.py has the
        definition) of the checkpoint TRAIN.NET_G: every object of the data -- a box with w, h > 0 whose shorter side is at least
        `min_side` pixels -- is cut at its ground-truth box out of the real 256x256 image and out of the image generated for the same
        caption, boxes and labels (exactly the images pool_codes and r_precision see under `seed`), resized to the trunk's 299x299
        input in the same launch (hip/ops.roi_resize) and sent through CNN_ENCODER.pool_code of TRAIN.NET_E's image encoder; the
        figure is fid()'s distance over the objects' codes (hip/ops.feature_moments, fid.frechet_distance).  It moves where the
        whole-image scores cannot: when the generator paints a believable scene and nothing plausible at the boxes.  ONE pass over
        the data loader (pool_codes), unless the caller shares one: `objects` is then the accumulator of scene_fid_objects() whose
        sink that pass has fed.  Writes <NET_G minus .pth>/<split>/scene_fid.json and returns its content; with return_codes also a
        dict of host tensors: the code matrices "real" and "fake" and the objects their rows stand for, "image" (in global image
        order) and "box"."""
        from .fid import frechet_distance, trunk_digest
        if net_g_missing():
            return None
        objects = self.fed("scene_fid", split_dir, num_samples, objects, seed=int(seed), min_side=float(min_side))
        real, fake = objects.finish()
        n = objects.n
        if n < 2:
            raise ValueError("scene_fid: the data loader gave %d objects; a covariance needs two at least" % n)
        D = int(real.shape[1])
        digest = trunk_digest(objects.encoder)
        stats = [[t.cpu() for t in ops.feature_moments(codes)] for codes in (real, fake)]
        dist, terms = frechet_distance(stats[0][0], stats[0][1], stats[1][0], stats[1][1])
        note = trunk_note("Object-level Frechet distance (SceneFID: every object cut at its box and resized to the trunk's input)",
                          "SceneFID", "a distance", trainer_variant(self))
        note += (" The boxes are the data's on both sides: the real and the generated image of a caption are cut at the same "
                 "ground-truth boxes; a box counts when its shorter side is at least min_side pixels.")
        if n < D:
            note += (" n = %d < %d features: the covariances are rank-deficient, so the figure is biased and only comparable "
                     "at equal n." % (n, D))
            print("SceneFID: %d objects for %d features -- the covariances are rank-deficient, the figure is biased and only "
                  "comparable at equal n (the JSON records it)" % (n, D))
        out = dict(terms, scene_fid=dist)
        out.update({"n_objects": int(n), "n_images": int(objects.n_images), "min_side": objects.min_side, "trunk_digest": digest})
        if trainer_variant(self) != "torchvision":
            out["trunk_variant"] = trainer_variant(self)
        save_dir = write_score(split_dir, "scene_fid", out, seed, note)
        print("SceneFID (%d objects of %d images, real and generated): %.4f = |dmu|^2 %.4f + Tr S_real %.4f + Tr S_fake %.4f - 2 x %.4f "
              "-> %s/scene_fid.json" % (n, objects.n_images, dist, terms["mean_sq"], terms["tr_s1"], terms["tr_s2"], terms["tr_sqrt"],
                                        save_dir))
        if return_codes:
            image, box = objects.objects()
            return out, {"real": real.cpu(), "fake": fake.cpu(), "image": image, "box": box}
        return out

    def score_head(self, head_path=None):
        """The classifier head of inception_score(): (weight (C, D), bias (C), the file's state dict, its path) from `head_path`, or
        from the trainer's trunk file where none is given.  ValueError where there is no such file or it holds no fc.weight /
        fc.bias: a random head is never drawn."""
        from . import inception_score as IS
        path = head_path or getattr(self, "trunk_path", None)
        if not path:
            raise ValueError("inception_score: no head -- the score needs a file with fc.weight (C, D) and fc.bias (C), --is_head or a "
                             "--trunk file that holds them (torchvision's inception_v3 file does); a random head is never drawn")
        state = self._state_file(path)
        head = IS.read_head(state, path)
        if head is None:
            raise ValueError("inception_score: no head -- %s holds no fc.weight / fc.bias; a random head is never drawn" % path)
        return head[0], head[1], state, path

    def head_trunk_digest(self, state, where):
        """fid.trunk_digest of the pass's own image encoder (_host_image_encoder: constructed, NET_E, the trunk file) after the trunk
        that the state dict `state` holds is loaded over it (ValueError where it holds it in part only): equal to the pass's digest
        exactly when every trunk parameter and buffer of `state` has the pass's bits.  BatchNorm's step counters, which the digest
        covers too, stay the pass's own, so they decide nothing.  The global generator's state is put back."""
        from .fid import trunk_digest
        from .inception import load_trunk_state
        kept = torch.get_rng_state()
        try:
            encoder = self._host_image_encoder()
        finally:
            torch.set_rng_state(kept)
        load_trunk_state(encoder, state, where)
        return trunk_digest(encoder)

    def inception_score(self, split_dir, num_samples=30000, seed=100, head_path=None, splits=10, real=False, codes=None,
                        return_codes=False):
        """Inception Score (Salimans et al. 2016; attngan/inception_score.py has the definition) of the checkpoint
        TRAIN.NET_G: the softmax of a classifier head over the Inception pool codes of one generated image per caption -- exactly the
        images and codes fid() sees under `seed` --, exp of the mean KL(p_i || mean p) over `splits` contiguous splits of the pass
        (lowered to the number of images where there are fewer), their mean and population standard deviation, and the figure over
        all rows.  The head: `fc.weight` (C, D) / `fc.bias` (C) of `head_path`, by default of the trainer's trunk file
        (main.py --trunk); where that file holds a trunk as well it must be the pass's, bit for bit ("head of another trunk").
        With real=True the same figures for the real images under "real" -- the ceiling the data itself gets -- and kl_marginals =
        KL(mean p of the generated || mean p of the real images).  A mode of its own, not a row of SCORES.  ONE pass over the data
        loader (pool_codes), or the `codes` a caller hands over; the codes stay on the device, hip/ops.softmax_head_sums gives
        sum_y p log p per row and the sum of p per split in one call per side without the (image, class) matrix ever being formed,
        one read-back per side, and the figures are finished on the host by math.fsum.  Writes
        <NET_G minus .pth>/<split>/inception_score.json and returns its content; with return_codes also a dict of the two code
        matrices on the host, "real" (None unless real) and "fake"."""
        from . import inception_score as IS
        from .inception import holds_trunk_keys
        if net_g_missing():
            return None
        weight, bias, state, head_file = self.score_head(head_path)
        verified = holds_trunk_keys(state)

        def want_real(digest, D):
            if weight.shape[1] != D:
                raise ValueError("inception_score: the head of %s is %d wide, the pool codes %d" % (head_file, weight.shape[1], D))
            if verified and self.head_trunk_digest(state, head_file) != digest:
                raise ValueError("inception_score: head of another trunk -- %s holds an Inception trunk beside its head, and it is not "
                                 "the one this pass runs under (digest %s...)" % (head_file, str(digest)[:12]))
            return bool(real)
        self._state_read = (head_file, state)                  # the pass's own loader reads the same file where it is the trunk file
        try:
            c = PooledCodes(self, "inception_score", split_dir, num_samples, seed, codes, want_real, " and real=True asks for it")
        finally:
            del self._state_read
            state = None                                       # 100 MB that nothing below needs
        n = c.n
        if n < 1:
            raise ValueError("inception_score: the data loader gave no batch")
        S = IS.effective_splits(n, splits)
        w, b = torch.from_numpy(weight).to(self.device), torch.from_numpy(bias).to(self.device)
        sides = {}
        for side, x in (("fake", c.fake), ("real", c.real)):
            if x is None:
                continue
            row_h, psum = ops.softmax_head_sums(x.contiguous(), w, b, S)
            back = torch.cat([row_h, psum.flatten()]).cpu().numpy()                       # the one read-back of a side
            row_h, psum = back[:n], back[n:].reshape(S, -1)
            bad = np.flatnonzero(~np.isfinite(row_h))
            if bad.size:
                raise ValueError("inception_score: row %d of the %s codes gives a non-finite sum (%r): non-finite codes or head"
                                 % (int(bad[0]), "generated" if side == "fake" else side, float(row_h[bad[0]])))
            sides[side] = (IS.finish(row_h, psum, n), psum)
        out = dict(sides["fake"][0])
        if "real" in sides:
            out["real"] = sides["real"][0]
            out["kl_marginals"] = IS.kl_marginals(IS.all_rows(sides["fake"][1]), n, IS.all_rows(sides["real"][1]), n)
        out.update({"classes": int(weight.shape[0]), "head_digest": IS.head_digest(weight, bias), "head": head_file})
        note = ("Inception Score: exp of the mean KL(p(y|x) || p(y)) of a classifier head over Inception pool codes, per contiguous "
                "split of the pass, mean and population standard deviation over the splits, and over all rows "
                "(inception_score_all).  Under torchvision's ImageNet Inception-v3 weights -- trunk and fc head -- this is the score "
                "under torchvision's network, not the TF-ported one of the published figures, and with 1000 outputs against its "
                "1008; under any other trunk or head it is comparable between checkpoints under the same trunk_digest and "
                "head_digest only.  The figure depends on the number of images per split.")
        if c.variant != "torchvision":
            note = ("Inception Score: exp of the mean KL(p(y|x) || p(y)) of a classifier head over Inception pool codes, per "
                    "contiguous split of the pass, mean and population standard deviation over the splits, and over all rows "
                    "(inception_score_all).  " + FID_NETWORK_NOTE[0].upper() + FID_NETWORK_NOTE[1:] + "  The head is the file's "
                    "own (1008 outputs in the published file); under any other weights the figure is comparable between "
                    "checkpoints under the same trunk_digest and head_digest only.  The figure depends on the number of images "
                    "per split.")
        if not verified:
            note += " The head file holds no trunk: the head was not verified against the trunk the codes were taken under."
        if S < int(splits):
            note += " splits lowered from %d to %d: there are only %d images." % (splits, S, n)
            print("Inception Score: %d images -- %d splits instead of %d (the JSON records it)" % (n, S, splits))
        out = c.write(out, n if "real" in sides else 0, n, note)
        print("Inception Score (%d generated images, %d classes, %d splits): %.4f +- %.4f, all rows %.4f%s -> %s/inception_score.json"
              % (n, out["classes"], S, out["inception_score"], out["inception_score_std"], out["inception_score_all"],
                 "" if "real" not in sides else "; real images %.4f +- %.4f, KL of the marginals %.6f"
                 % (out["real"]["inception_score"], out["real"]["inception_score_std"], out["kl_marginals"]), c.save_dir))
        return c.result(out, return_codes)

    def layout_shift(self, split_dir, num_samples=30000, seed=100, min_shift=None, min_side=1, show=16, image_sink=None):
        """Layout control of the checkpoint TRAIN.NET_G by moving ONE box (attngan/layoutshift.py has the
        definition): every caption's image is generated twice from the same noise, eps, text and labels -- A under the data's `tmi`,
        bit for bit the image every other score sees under `seed`, and B under `tmi` with only the moved slot's matrix replaced --
        and hip/ops.box_shift_sums gives, per pair in one launch per batch, how much changed inside the old and the new rectangle,
        in the other objects and in the rest, and whether the old rectangle's content is found again at the new place (follow = 1)
        or stayed where it was (follow = 0).  A mode of its own as r_precision() is, not a row of SCORES: it generates a second
        image under another layout.  No image encoder is loaded.  `image_sink`, where given, is called once per batch with
        (A, B, edit table, take).  Writes <NET_G minus .pth>/<split>/layout_shift.json and, where show > 0, layout_grid.png -- one row
        [A with the old box | B with the new box | |A - B|] per pair of most_ignored -- and returns the JSON's content."""
        from .layoutshift import ShiftResponse, layout_grid
        from .scenefid import boxes_from_theta
        if net_g_missing():
            return None
        size, rows = self.pass_shape(num_samples)
        acc = ShiftResponse(size, 3, rows, min_shift, min_side, seed, self.device, keep=show)

        def pair(netG, gen, words_embs, sent_emb, mask, tm, tmi, label_one_hot, keys, take):
            noise, eps = draw_noise(gen, sent_emb)
            a = generate_from(netG, noise, eps, words_embs, sent_emb, mask, tmi, label_one_hot)
            table = acc.edits(boxes_from_theta(tm.cpu()), take)                    # the one read-back of the layout
            b = generate_from(netG, noise, eps, words_embs, sent_emb, mask, moved_matrices(tmi, table), label_one_hot)
            acc.add(a.float(), b.float(), table, keys=keys)
            if image_sink is not None:
                image_sink(a, b, table, take)
            return a
        self.pool_codes(split_dir, num_samples, seed, want_real=False, trunk=False, generate=pair)
        out = acc.result(show)
        out.update({"size": size, "show": len(out["most_ignored"]), "grid": None})
        save_dir = eval_save_dir(split_dir)
        if acc.kept:
            out["grid"] = layout_grid(save_dir, acc.kept, acc.info)
        write_score(
            split_dir, "layout_shift", out, seed,
            "Layout control by moving one box: every image is generated twice from the same noise, text and labels, under the data's "
            "layout (A) and with one object's box moved by at least min_shift pixels (B).  follow = 1 - moved / baseline over the old "
            "rectangle: 1 -- the object travelled with its box, 0 -- the edit was ignored.  locality: the share of the squared change "
            "that lies inside the old and the new rectangle; area_share is its chance level.  spill_others / spill_background: the "
            "mean squared change per pixel in the other objects' rectangles / in the rest, over that of the box pixels.  mean +- "
            "population std over the pairs; flat (baseline 0), unchanged (B == A), no_objects and immovable are counted.  The images "
            "enter as fp32 in [-1, 1], not quantised to 8 bits.  Every figure depends on min_shift and min_side.")
        f, loc = out["follow"], out["locality"]
        shown = lambda v: "n/a" if v["mean"] is None else "%.4f +- %.4f (%d)" % (v["mean"], v["std"], v["n"])
        print("Layout shift (%d pairs of %d images; %d without objects, %d immovable, %d unchanged, %d flat; min_shift %d px): follow "
              "%s, locality %s at area share %s -> %s/layout_shift.json%s"
              % (out["n_pairs"], out["n_images"], out["no_objects"], out["immovable"], out["unchanged"], out["flat"], out["min_shift"],
                 shown(f), shown(loc), shown(out["area_share"]), save_dir, "" if out["grid"] is None else " and %s" % out["grid"]))
        return out

    def _sheet_table(self, att, vis):
        """attnsheet.table(att, vis / att) on the device, built once per shape"""
        from .attnsheet import table
        cache = self.__dict__.setdefault("_sheet_tables", {})
        if (att, vis) not in cache:
            cache[(att, vis)] = torch.from_numpy(table(att, vis // att)).to(self.device)
        return cache[(att, vis)]

    def attention_sheets(self, fake_imgs, att_maps, captions, topk=5, vis_size=256):
        """The attention sheets of one generator batch whose captions all have captions.shape[1] words: per
        attention stage k one launch of ops.attn_conf, the reference's top-K choice on the host, one launch of ops.attn_sheet for
        every picked (sample, word) of the batch over fake_imgs[k + 1] -- brought to vis_size by F.interpolate on the device where
        smaller, as miscc/vis does on the host -- and the caption strip of vis.drawCaption on top.
        -> (sheets[k][sample]: uint8 (FONT_MAX + vis, K (vis + 2), 3), records[k][sample]: dict(words, conf, lo, hi, flag))"""
        import torch.nn.functional as F
        from .attnsheet import ALPHA, top_words
        from .miscc import vis
        n, T = captions.shape
        lens = torch.full((n,), T, dtype=torch.int32)
        strip = np.ones([n * vis.FONT_MAX, T * (vis_size + 2), 3], dtype=np.uint8)
        strip = np.asarray(vis.drawCaption(strip, captions, self.ixtoword, vis_size, off1=0)[0]).astype(np.uint8)
        pad = np.zeros((vis_size, 2, 3), dtype=np.uint8)
        sheets, records = [], []
        for k, attn in enumerate(att_maps):
            attn = attn.detach().float().contiguous()
            img = fake_imgs[k + 1].detach().float()
            if img.shape[-1] != vis_size:
                img = F.interpolate(img, size=(vis_size, vis_size), mode='bilinear', align_corners=False)
            conf = ops.attn_conf(attn, lens).cpu().numpy()
            order = [top_words(conf[s], T, topk) for s in range(n)]
            pick = torch.tensor([(s, w) for s in range(n) for w in order[s]], dtype=torch.int32)
            sheet, stats, flags = ops.attn_sheet(attn, lens, img.contiguous(), self._sheet_table(attn.shape[-1], vis_size), pick, ALPHA)
            sheet, stats, flags = sheet.cpu().numpy(), stats.cpu().numpy(), flags.cpu().numpy()
            K = len(order[0])
            sheets.append([])
            records.append([])
            for s in range(n):
                txt = [strip[s * vis.FONT_MAX:(s + 1) * vis.FONT_MAX, w * (vis_size + 2):(w + 1) * (vis_size + 2)] for w in order[s]]
                row = [np.concatenate([sheet[s * K + i], pad], 1) for i in range(K)]
                sheets[k].append(np.concatenate([np.concatenate(txt, 1), np.concatenate(row, 1)], 0))
                records[k].append({"words": order[s], "conf": [float(conf[s, w]) for w in order[s]],
                                   "lo": [float(v) for v in stats[s * K:(s + 1) * K, 0]], "hi": [float(v) for v in stats[s * K:(s + 1) * K, 1]],
                                   "flag": [int(v) for v in flags[s * K:(s + 1) * K]]})
        return sheets, records

    def scenes(self, path, seed=100, samples=4, topk=5, attention=True, classes=None, image_sink=None):
        """Images from written scenes (attngan/scenes.py has the file's rules): for every scene of the JSON
        file `path` -- a caption, up to three boxes with labels -- `samples` images of TRAIN.NET_G under the scene's own seeded
        generator, each scene a generator batch of its own, so a scene's images do not depend on what else the file holds; where the
        scene asks for a sweep, sample 0's draws again with only the swept slot's matrix replaced, in batches of the samples' shape,
        step 0 being sample 0 itself.  The data loader's dataset gives the vocabulary only.  Writes <NET_G minus .pth>/scenes/<name>/
        s<k>_g<stage>.png, s<k>_a<stage>.png (the attention sheets, where `attention`), samples.png and sweep.png, and the record
        scenes.json beside the scene directories; returns the record.  `image_sink`, where given, is called once per scene with
        (scene, the three stages' images, the attention maps, the sweep's 256 x 256 images or None).  The file is checked before any checkpoint is read."""
        import torch.nn.functional as F
        from PIL import Image
        from . import scenes as SC
        from . import synthetic
        if net_g_missing():
            return None
        topk = int(topk)
        if not 1 <= topk <= 8:
            raise ValueError("scenes: topk must be in 1..8, got %d" % topk)
        if attention and cfg.TEXT.WORDS_NUM > 32:
            raise ValueError("scenes: attention sheets take captions of 32 words at the most, TEXT.WORDS_NUM is %d" % cfg.TEXT.WORDS_NUM)
        todo = SC.load(path, SC.vocabulary(self.data_loader.dataset), cfg.TEXT.WORDS_NUM, synthetic.N_CLASSES, samples, classes, seed)
        netG, text_encoder, _, _ = self._load_seeded(seed, trunk=False)
        root = eval_save_dir('scenes')
        u8 = lambda t: t.add(1.0).mul(127.5).clamp(0, 255).byte().permute(0, 2, 3, 1).cpu().numpy()       # sampling()'s rule
        shown = lambda t: t if t.shape[-1] == 256 else F.interpolate(t, size=(256, 256), mode='nearest')
        record = []
        for sc in todo:
            save_dir = '%s/%s' % (root, sc.name)
            mkdir_p(save_dir)
            n, T = sc.samples, len(sc.tokens)
            gen = torch.Generator(device=self.device)
            gen.manual_seed(sc.seed)
            captions = torch.tensor([sc.tokens] * n, dtype=torch.int64, device=self.device)
            with torch.no_grad():
                words_embs, sent_emb, mask = encode_text(text_encoder, captions, torch.full((n,), T, dtype=torch.int64, device=self.device))
                noise, eps = draw_noise(gen, sent_emb)
                tmi = ops.bbox_to_theta(torch.from_numpy(sc.boxes).to(self.device))[1][None].repeat(n, 1, 1, 1)
                label = synthetic.one_hot_labels(sc.labels)[None].repeat(n, 1, 1).to(self.device)
                fake_imgs, att_maps, _, _ = netG(noise, sent_emb, words_embs, mask, tmi, label, eps=eps)
                stages = [u8(t) for t in fake_imgs]
                for k in range(n):
                    for g, st in enumerate(stages):
                        Image.fromarray(st[k]).save('%s/s%d_g%d.png' % (save_dir, k, g))
                entry = {"name": sc.name, "caption": sc.caption, "words": sc.words, "tokens": sc.tokens, "dropped": sc.dropped,
                         "truncated": sc.truncated, "boxes_px": sc.pixel_boxes(256), "labels": [int(v) for v in sc.labels[:sc.n_objects]],
                         "seed": sc.seed, "samples": n, "sweep": sc.sweep, "sheets": []}
                if attention:
                    sheets, recs = self.attention_sheets(fake_imgs, att_maps, captions, topk)
                    for k in range(n):
                        for a in range(len(sheets)):
                            Image.fromarray(sheets[a][k]).save('%s/s%d_a%d.png' % (save_dir, k, a))
                            entry["sheets"].append(dict(recs[a][k], sample=k, stage=a))
                drawn = torch.from_numpy(sc.drawn_boxes())
                layout = draw_bbox_lines(torch.full((n, 3, 256, 256), -1.0, device=self.device), drawn, 256)
                rows = [layout] + [draw_bbox_lines(shown(t.float()).clone(), drawn, 256) for t in fake_imgs]
                Image.fromarray(np.concatenate([np.concatenate(list(r), 0) for r in map(u8, rows)], 1)).save('%s/samples.png' % save_dir)
                swept = None
                if sc.sweep is not None:
                    path_boxes = torch.from_numpy(sc.sweep_boxes())
                    steps, slot = path_boxes.shape[0], sc.sweep["object"]
                    first = lambda t: t[:1].repeat((n,) + (1,) * (t.dim() - 1))
                    out = []
                    for at in range(0, steps, n):
                        rows = list(range(at, min(at + n, steps)))
                        table = {"row": torch.arange(len(rows)), "slot": torch.full((len(rows),), slot, dtype=torch.int64)}
                        out.append(generate_from(netG, first(noise), first(eps), words_embs, sent_emb, mask,
                                                 moved_matrices(tmi, table, path_boxes[rows]), label)[:len(rows)])
                    swept = torch.cat(out)
                    strip = swept.float().clone()
                    for k in range(steps):
                        draw_bbox_lines(strip[k:k + 1], torch.from_numpy(SC.clamp_box(path_boxes[k].numpy()))[None], 256)
                    Image.fromarray(np.concatenate(list(u8(strip)), 1)).save('%s/sweep.png' % save_dir)
            if image_sink is not None:
                image_sink(sc, fake_imgs, att_maps, swept)
            record.append(entry)
        out = {"scenes": record, "file": str(path), "topk": topk, "attention": bool(attention)}
        write_score('scenes', "scenes", out, seed,
                    "Images of TRAIN.NET_G from written scenes: per scene `samples` images under the scene's own seed (s<k>_g<stage>.png, "
                    "samples.png: layout | 64 | 128 | 256), the attention sheets of the two attention stages (s<k>_a<stage>.png: the top-K "
                    "words by thresholded attention mass conf, each word's map thresholded at 2 / len, upscaled, smoothed and normalised "
                    "by its own lo and hi, pasted over the stage's image; flag 1: a flat map, 2: a non-finite one) and, where asked for, "
                    "one object walked across the image under sample 0's noise (sweep.png).")
        print("Scenes (%d scenes, %d images%s) -> %s" % (len(todo), sum(sc.samples for sc in todo),
                                                       ", attention sheets of the top %d words" % topk if attention else "", root))
        return out

    def train_split(self):
        """(dataset, name): the TRAIN split next to the data loader's evaluation split, what memorisation() searches -- for a
        TextDataset the 'train' split of the same directories; for a SyntheticTextDataset a second synthetic set of the same
        length and vocabulary under a seed of its own (the split's plus BANK_SEED_STEP), named 'synthetic-train'"""
        from .datasets import SyntheticTextDataset, TextDataset
        ds = self.data_loader.dataset
        if isinstance(ds, SyntheticTextDataset):
            return SyntheticTextDataset(ds.length, ds.n_words, seed=ds.seed + BANK_SEED_STEP), "synthetic-train"
        if isinstance(ds, TextDataset):
            return TextDataset(ds.data_dir, ds.img_dir, 'train', base_size=cfg.TREE.BASE_SIZE), "train"
        raise ValueError("memorisation: no train split is known for a %s; hand a bank over" % type(ds).__name__)

    @staticmethod
    def dataset_key(dataset, position):
        """the key of a dataset's sample without reading its image"""
        names = getattr(dataset, "filenames", None)
        return str(names[position]) if names is not None else 'synthetic_%06d' % position

    def neighbour_bank(self, seed=100, bank_size=None, digest=None):
        """fid.NeighbourBank of the train split (train_split): the pool codes of its first `bank_size` real images (all where
        None), in dataset order, under the image encoder a pass under `seed` runs -- loaded as _load_seeded loads it, so a
        random-init trunk of an empty NET_E is the pass's too; `digest`, where given, is checked against it.  No generator runs
        and no caption is encoded.  The trunk sees the loader's batch size only: the last batch is filled up with zeros.  The
        global generators' states are put back, so a pass that follows shuffles and crops as it would have without this call."""
        from .fid import NeighbourBank, trunk_digest
        dataset, name = self.train_split()
        rows = len(dataset) if bank_size is None else max(1, min(int(bank_size), len(dataset)))
        states = torch.get_rng_state(), np.random.get_state()
        try:
            image_encoder = self._load_seeded(seed)[2]
            own = trunk_digest(image_encoder)
            if digest is not None and own != digest:
                raise ValueError("memorisation: the bank's trunk (digest %s...) is not the pass's (%s...)" % (own[:12], digest[:12]))
            chunk = int(self.data_loader.batch_size)
            loader = torch.utils.data.DataLoader(torch.utils.data.Subset(dataset, range(rows)), batch_size=chunk, shuffle=False,
                                                 num_workers=int(self.data_loader.num_workers))
            D = int(image_encoder.emb_cnn_code.weight.shape[1])
            codes = torch.empty((rows, D), dtype=torch.float32, device=self.device)
            n = 0
            for batch in loader:
                img = batch[0][-1].to(self.device)
                take = int(img.shape[0])
                if take < chunk:
                    img = torch.cat([img, img.new_zeros((chunk - take,) + tuple(img.shape[1:]))])
                with torch.no_grad():
                    codes[n:n + take] = image_encoder.pool_code(img)[:take]
                n += take
        finally:
            torch.set_rng_state(states[0])
            np.random.set_state(states[1])
        return NeighbourBank(codes.cpu(), np.arange(rows), own, name)

    def thumbnails(self, num_samples=30000, seed=100, show=16):
        """The accumulator memorisation() draws its grid from: a Thumbnails, or None where no row is shown"""
        return Thumbnails() if int(show) > 0 else None

    def memorisation(self, split_dir, num_samples=30000, seed=100, bank_path=None, bank_size=None, k=5, show=16, codes=None,
                     bank=None, return_codes=False):
        """Is the checkpoint TRAIN.NET_G reproducing its TRAINING images?  (attngan/memorisation.py has the
        definitions.)  Every other score compares the generated images with the evaluation split's or with each other, and a
        generator that has memorised the training set scores well on all of them.  Here the Inception pool codes of TRAIN.NET_E's
        image encoder are searched in a bank T of the TRAIN split's real images: `authenticity`, the share of generated images that
        are not closer to their nearest training image than that image's own nearest training neighbour, next to the same share of
        the evaluation split's real images (`authenticity_heldout`, the data's own value); `copying`, the Mann-Whitney statistic of
        the generated images' nearest-bank distances against the held-out real images' (0.5: as far from the training set as
        unseen real images; towards 1: closer); and the `show` most suspicious generated images with their `k` nearest training
        images, listed in the JSON and drawn as nn_grid.png, rows of [generated | its k nearest training images] at 64 x 64.
        The generated and the held-out codes are those of fid() -- ONE pass over the data loader (pool_codes, whose image_sink
        keeps the thumbnails), or the `codes` a caller hands over from a pass of its own (with a Thumbnails under "thumbnails" where
        the grid is wanted).  The bank: `bank`, a fid.NeighbourBank, where given; else `bank_path` when that file exists and was
        taken under the same trunk (ValueError for another trunk's); else neighbour_bank(), saved to `bank_path` where given.
        `bank_size` cuts it to its first rows.  On the device: hip/ops.knn_sqdist(T, 1), hip/ops.knn_cross(F, T, k),
        hip/ops.knn_cross(H, T, 1), one read-back; k is lowered to the bank's size where that is smaller.  All figures depend on the
        bank's size.  Writes <NET_G minus .pth>/<split>/memorisation.json (and nn_grid.png) and returns the JSON's content; with
        return_codes also a dict of host tensors: the code matrices "real", "fake" and "bank"."""
        from . import memorisation as MEM
        from .fid import NeighbourBank
        if net_g_missing():
            return None
        k, show = int(k), int(show)
        if k < 1 or k > 8 or show < 0:
            raise ValueError("memorisation: 1 <= k <= 8 and show >= 0 expected, got k = %d, show = %d" % (k, show))
        if codes is None:
            thumbs = self.thumbnails(show=show)
            codes = dict(self.shared_pass(split_dir, num_samples, seed, {"memorisation": thumbs}), thumbnails=thumbs)
        c = PooledCodes(self, "memorisation", split_dir, num_samples, seed, codes)
        thumbs = codes.get("thumbnails") if show > 0 else None
        n, D = c.n, int(c.fake.shape[1])
        if n < 1:
            raise ValueError("memorisation: the data loader gave no batch")
        if bank is None:
            if bank_path is not None and os.path.isfile(bank_path):
                bank = NeighbourBank.load(bank_path, c.digest, D)             # ValueError for another trunk's file
                print('Load the training bank from: %s (%d images of split %s)' % (bank_path, len(bank), bank.split))
            else:
                bank = self.neighbour_bank(seed, bank_size, c.digest)
                if bank_path is not None:
                    bank.save(bank_path)
                    print('Save the training bank to: %s' % bank_path)
        elif bank.trunk_digest != c.digest or bank.codes.shape[1] != D:
            raise ValueError("memorisation: the bank handed over was computed under another Inception trunk (digest %s..., the "
                             "codes' is %s...) or at another width" % (bank.trunk_digest[:12], str(c.digest)[:12]))
        bank_codes, positions = bank.codes, bank.positions
        if bank_size is not None and len(bank) > int(bank_size):
            bank_codes, positions = bank_codes[:max(1, int(bank_size))], positions[:max(1, int(bank_size))]
        n_bank = int(bank_codes.shape[0])
        if n_bank < 2:
            raise ValueError("memorisation: a bank of %d image has no nearest other image; two at least" % n_bank)
        kk = min(k, n_bank)
        T = torch.tensor(bank_codes).to(self.device)
        nn_bank = ops.knn_sqdist(T, 1)                                      # every training image's own nearest training neighbour
        d2_f, idx_f = ops.knn_cross(c.fake.contiguous(), T, kk)
        d2_h, idx_h = ops.knn_cross(c.real.contiguous(), T, 1)
        back = torch.cat([t.double().flatten() for t in (d2_f, idx_f, d2_h, idx_h, nn_bank)]).cpu().numpy()    # the one read-back
        cut = np.cumsum([0, n * kk, n * kk, n, n, n_bank])
        d2_f, idx_f, d2_h, idx_h, nn_bank = (back[cut[i]:cut[i + 1]] for i in range(5))
        d2_f, idx_f = d2_f.reshape(n, kk), idx_f.reshape(n, kk).astype(np.int64)
        idx_h = idx_h.astype(np.int64)
        out = MEM.scores(d2_f[:, 0], idx_f[:, 0], d2_h, idx_h, nn_bank)
        rows, ratio = MEM.most_suspicious(d2_f[:, 0], idx_f[:, 0], nn_bank, show)
        bank_dataset = None
        suspicious = []
        for r, x in zip(rows.tolist(), ratio.tolist()):
            at = positions[idx_f[r]].tolist()
            entry = {"row": r, "ratio": x, "d2": d2_f[r].tolist(), "nn_bank_d2": float(nn_bank[idx_f[r, 0]]),
                     "bank_rows": idx_f[r].tolist(), "bank_positions": at}
            if bank.split in ("train", "synthetic-train"):
                if bank_dataset is None:
                    bank_dataset = self.train_split()[0]
                entry["bank_keys"] = [self.dataset_key(bank_dataset, p) for p in at]
            suspicious.append(entry)
        grid = None
        if thumbs is not None and len(rows) and bank_dataset is not None and len(thumbs) >= n:
            grid = self._nn_grid(c.save_dir, thumbs.images(rows), [e["bank_positions"] for e in suspicious], bank_dataset)
        note = trunk_note("Nearest training neighbours (authenticity: the share of generated images not closer to their nearest "
                          "training image than that image's own nearest training neighbour, authenticity_heldout: the same share "
                          "of the evaluation split's real images; copying: the Mann-Whitney statistic of the generated images' "
                          "distances to the training set against the held-out real images', 0.5 = as far as unseen real images, "
                          "towards 1 = closer)", "the papers' figures", "figures", c.variant)
        note += " Every figure depends on n_bank: comparable at equal bank only."
        if bank.split == "synthetic-train":
            note += " Synthetic data: the bank is a second synthetic set with a seed of its own, not a split of real images."
        if kk < k:
            note += " k lowered from %d to %d: the bank holds only %d images." % (k, kk, n_bank)
            print("Memorisation: a bank of %d images -- k = %d instead of %d (the JSON records it)" % (n_bank, kk, k))
        out.update({"n_bank": n_bank, "k": int(kk), "bank_path": bank_path, "bank_split": bank.split, "show": len(suspicious),
                    "most_suspicious": suspicious, "grid": grid})
        out = c.write(out, n, n, note)
        print("Memorisation (%d generated, %d held-out real images against %d training images; k = %d): authenticity %.4f "
              "(held-out %.4f) copying %.4f -> %s/memorisation.json%s"
              % (n, n, n_bank, kk, out["authenticity"], out["authenticity_heldout"], out["copying"], c.save_dir,
                 "" if grid is None else " and %s" % grid))
        if return_codes:
            out, both = c.result(out, True)
            return out, dict(both, bank=torch.tensor(bank_codes))
        return out

    @staticmethod
    def _nn_grid(save_dir, generated, bank_positions, bank_dataset):
        """nn_grid.png: one row per entry, [generated | the training images at its bank positions], THUMB x THUMB each; the
        training images are re-read from the bank's dataset by position.  Returns the file's name."""
        from PIL import Image
        k = max(len(p) for p in bank_positions)
        h, w = generated.shape[-2], generated.shape[-1]
        sheet = np.zeros((len(bank_positions) * h, (1 + k) * w, 3), dtype=np.uint8)
        for r, at in enumerate(bank_positions):
            sheet[r * h:(r + 1) * h, 0:w] = generated[r].transpose(1, 2, 0)
            for j, p in enumerate(at):
                tile = thumbnail_u8(bank_dataset[int(p)][0][-1].numpy())
                sheet[r * h:r * h + tile.shape[1], (1 + j) * w:(1 + j) * w + tile.shape[2]] = tile.transpose(1, 2, 0)
        Image.fromarray(sheet).save('%s/nn_grid.png' % save_dir)
        return "nn_grid.png"

    def sample(self, split_dir, num_samples=25, draw_bbox=False):
        """trainer.py:474-579 (what main.py:158 runs for B_VALIDATION): for the first `num_samples` batches of an
        eval-mode loader take the FIRST sample of the sorted batch, generate nine 256x256 images for its caption /
        boxes / labels from nine noise vectors with netG.eval(), and save one row [real | 9 fakes] (boxes drawn as white
        lines when draw_bbox) as <NET_G minus .pth>_<split>/<caption>_<step>.png."""
        from .datasets import prepare_data
        from ..stackgan.logging_utils import save_image
        if net_g_missing():
            return None
        netG, text_encoder = self._load_eval_models()
        save_dir = eval_save_dir(split_dir, sep='_')
        imsize, nrep = cfg.TREE.BASE_SIZE << (cfg.TREE.BRANCH_NUM - 1), 9
        written, step = [], 0
        for step, data in enumerate(self.data_loader, 0):
            if step >= num_samples:
                break
            imgs, captions, cap_lens, class_ids, keys, (tm, tmi), label_one_hot, bbox = \
                prepare_data(data, self.device, eval=True)
            with torch.no_grad():
                def row0(t):                                  # the first sample of the batch, nine times
                    return t[0:1].repeat(nrep, *[1] * (t.dim() - 1)).contiguous()
                words_embs, sent_emb, mask = (row0(t) for t in encode_text(text_encoder, captions, cap_lens))
                noise = torch.randn(nrep, cfg.GAN.Z_DIM, device=self.device)
                fake_imgs, _, _, _ = netG(noise, sent_emb, words_embs, mask, row0(tmi), row0(label_one_hot))
            data_img = torch.zeros(1 + nrep, 3, imsize, imsize)
            data_img[0] = imgs[-1][0].cpu()
            data_img[1:] = fake_imgs[-1].float().cpu()
            if draw_bbox:
                draw_bbox_lines(data_img, np.asarray(bbox[0]), imsize)
            sentence = caption_sentence(captions[0].cpu().numpy(), self.ixtoword)
            fullpath = '{}/{}_{}.png'.format(save_dir, sentence, step)
            save_image(data_img, fullpath, nrow=1 + nrep, normalize=True)
            written.append(fullpath)
        print("Saved {} files to {}".format(len(written), save_dir))
        return written
