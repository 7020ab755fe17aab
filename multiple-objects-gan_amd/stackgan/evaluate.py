"""Checkpoint evaluation of the StackGAN-family trees (multi-mnist, clevr, coco stage I / II; the reference
trees can train and draw sample grids, and nothing else): ONE pass over the evaluation loader serves all the asked scores --

  object_accuracy   object accuracy by nearest labelled training crops (stackgan/objaccuracy.py has the definition): the
                    accumulator ObjectCrops here, hip/ops.roi_resize for the crops, hip/ops.knn_label for the search
  swd, msssim,      the trunk-free image scores of sections 9g / 9h / 9k, their accumulators as they are
  spectrum          (attngan/swd.SlicedWasserstein, attngan/msssim.PairFigures, attngan/spectrum.RadialSpectrum) at the tree's
                    size (64, or 256 for stage II) and channels (1 for multi-mnist), fed through their sink(real, fake, take)

-- each written to <NET_G minus .pth>/<split>/<score>.json with the seed, NET_G, the settings and a note.

The pass.  Batches come from the tree's prepare_batch; the checkpoint cfg.NET_G is loaded by load_network_stageI / II; the
generator runs in eval mode under no_grad through engine.generate, the train step's own call.  Noise: z, then eps (the trees
with text), then eps_s1 (stage II) from ONE seeded device torch.Generator, in that order -- a contract: the images do not depend
on which scores are asked.  msssim's same_caption ("same layout, labels and text, fresh noise") draws from a second generator
seeded seed + 1.  A file holds the bytes of its score run alone.

`FamilyEvaluation.layout_shift` (attngan/layoutshift.py has the definition) is a mode of its own, not a row of
SCORES: a pass that generates every image twice from one set of draws, under the data's layout and with one box moved.
"""
import json
import os

import numpy as np
import torch

from ..attngan.miscc.utils import mkdir_p
from ..attngan.scenefid import boxes_from_theta, object_list
from . import objaccuracy as OA
from .engine import generate

SCORES = ("object_accuracy", "swd", "msssim", "spectrum")      # the order a pass finishes them in
BANK_SEED_STEP = 1000003   # a synthetic split's bank: a second synthetic set, under the split's seed plus this (item i is drawn
                           # under seed + i, so the step is larger than any set: the two sets share no item)


def asked_scores(args):
    """score -> its keyword arguments, for the score flags `args` (main_base.parse_args) holds, in SCORES order"""
    kw = {"object_accuracy": dict(k=args.oa_k, side=args.oa_side, min_side=args.oa_min_side, bank_size=args.oa_bank_size,
                                  show=args.oa_show),
          "swd": dict(patches=args.swd_patches, dirs=args.swd_dirs, repeats=args.swd_repeats, min_res=args.swd_min_res),
          "msssim": dict(scales=args.msssim_scales, same_caption=not args.msssim_no_resample),
          "spectrum": dict(window=args.spectrum_window)}
    return {name: kw[name] for name in SCORES if getattr(args, name)}


def generate_seeded(netG, variant, stage, cfg, b, gen):
    """One image per item of the prepared batch `b` under noise from the seeded device generator `gen`: z (B, Z_DIM), then for the
    trees with text eps (B, CONDITION_DIM), then in stage II eps_s1 (B, CONDITION_DIM) -- the order is a contract.  `b` keeps its
    own fields: the draws go into a copy."""
    return generate(netG, variant, stage, draw_noise(variant, stage, cfg, b, gen))[0]


def draw_noise(variant, stage, cfg, b, gen):
    """generate_seeded's draws, in its order, in a copy of the prepared batch `b`: layout_shift() generates twice from one copy"""
    B, dev = b["real_imgs"].shape[0], b["real_imgs"].device
    b = dict(b, z=torch.randn(B, cfg.Z_DIM, device=dev, generator=gen))
    if variant.text:
        b["eps"] = torch.randn(B, cfg.GAN.CONDITION_DIM, device=dev, generator=gen)
        if stage == 2:
            b["eps_s1"] = torch.randn(B, cfg.GAN.CONDITION_DIM, device=dev, generator=gen)
    return b


def object_slots(boxes, take, size, min_side=1):
    """(image (R,) int64, slot (R,) int64, boxes (R, 4) fp32) of the objects of the `take` leading images of host boxes (B, G, 4), in
    image order then slot order.  What an object is stays scenefid.object_list's rule: it is asked slot by slot."""
    B, G = boxes.shape[0], boxes.shape[1]
    keep = torch.zeros((max(0, min(int(take), B)), G), dtype=torch.bool)
    for g in range(G):
        keep[object_list(boxes[:, g:g + 1].contiguous(), take, size, min_side)[0].long(), g] = True
    where = keep.nonzero()
    index, listed = object_list(boxes, take, size, min_side)
    assert torch.equal(index.long(), where[:, 0])
    return where[:, 0].contiguous(), where[:, 1].contiguous(), listed


class ObjectCrops:
    """The crops and classes of the objects of a stream of batches, real and generated (scenefid.ObjectCodes without the trunk).
    tree: mnist, clevr or coco (objaccuracy.classes_of); rows: the images the pass will see at most; size / channels: the images';
    side: the crops'.  `sink(real, fake, tm, label_one_hot, take)` reads `tm` and the labels back in ONE transfer, lists the batch's
    objects, leaves the unlabelled ones out (coco's class 80) and has hip/ops.roi_resize write both sides' crops into two device
    buffers (rows * max_objects, channels * side^2), allocated at the first batch.  `n` objects of `n_images` images are in;
    `classes`, `image`, `slot`, `box` list them in the order of the crops' rows (host)."""

    def __init__(self, tree, rows, size, channels, max_objects, side=16, min_side=1, device="cuda", resize=None, both=True):
        self.tree, self.rows, self.size, self.channels = tree, int(rows), int(size), int(channels)
        if tree not in OA.CLASSES:
            raise ValueError("objaccuracy: tree must be one of %s, got %r" % (sorted(OA.CLASSES), tree))
        self.max_objects, self.side, self.min_side = int(max_objects), int(side), float(min_side)
        if min(self.rows, self.size, self.channels, self.max_objects, self.side) < 1:
            raise ValueError("objaccuracy: rows, size, channels, max_objects and side >= 1 expected")
        self.device, self.resize, self.sides = torch.device(device), resize, ("real", "fake") if both else ("real",)
        self.D = self.channels * self.side * self.side
        self.crops = None
        self.n = self.n_images = self.unlabelled = 0
        self._classes, self._image, self._slot, self._box = [], [], [], []

    def sink(self, real, fake, tm, label_one_hot, take):
        take = int(take)
        if self.n_images + take > self.rows:
            raise ValueError("objaccuracy: %d more images do not fit an accumulator for %d of which %d are in"
                             % (take, self.rows, self.n_images))
        B, G = tm.shape[0], tm.shape[1]
        if G > self.max_objects:
            raise ValueError("objaccuracy: %d boxes per image, the accumulator has room for %d" % (G, self.max_objects))
        if self.resize is None:
            from ..hip import ops
            self.resize = ops.roi_resize
        if self.crops is None:
            self.crops = {k: torch.empty((self.rows * self.max_objects, self.D), dtype=torch.float32, device=self.device)
                          for k in self.sides}
        host = torch.cat([tm.detach().float().reshape(B, G, 6), label_one_hot.detach().float().reshape(B, G, -1)], dim=2).cpu()
        boxes = boxes_from_theta(host[:, :, :6].reshape(B, G, 2, 3).contiguous())                     # the one read-back
        image, slot, listed = object_slots(boxes, take, self.size, self.min_side)
        classes = torch.from_numpy(OA.classes_of(self.tree, host[:, :, 6:].numpy()))[image, slot]
        labelled = classes >= 0
        self.unlabelled += int((~labelled).sum())
        image, slot, listed, classes = image[labelled], slot[labelled], listed[labelled].contiguous(), classes[labelled]
        R = int(image.shape[0])
        for k, x in (("real", real), ("fake", fake)):
            if k in self.sides and R:
                out = self.crops[k][self.n:self.n + R].view(R, self.channels, self.side, self.side)
                self.resize(x.detach().float().contiguous(), listed, image.contiguous(), self.side, self.side, out=out)
        self._classes.append(classes)
        self._image.append(image + self.n_images)
        self._slot.append(slot)
        self._box.append(listed)
        self.n += R
        self.n_images += take

    def finish(self):
        """{"real", "fake"}: the (n, D) filled rows of the device buffers (None before the first batch)"""
        return {k: (None if self.crops is None else self.crops[k][:self.n]) for k in self.sides}

    def objects(self):
        """(classes (n,) int64, image (n,) int64 in global image order, slot (n,) int64, box (n, 4) fp32), host tensors"""
        if not self._classes:
            z = torch.zeros((0,), dtype=torch.int64)
            return z, z, z, torch.zeros((0, 4), dtype=torch.float32)
        return torch.cat(self._classes), torch.cat(self._image), torch.cat(self._slot), torch.cat(self._box)


def dataset_key(dataset, position):
    """the key of a dataset's item without reading its image"""
    names = getattr(dataset, "filenames", None)
    return os.path.basename(str(names[position])) if names is not None else 'synthetic_%06d' % position


def search(queries, asked, bank, bank_classes, k):
    """hip/ops.knn_label of device crops `queries` (M, D) with host classes `asked` against the device bank: a dict of host numpy
    arrays, d2 (M, k), idx (M, k), neighbour_classes (M, k), same_d2, same_idx, other_d2, other_idx (M,); one read-back"""
    from ..hip import ops
    dev = queries.device
    out = ops.knn_label(queries.contiguous(), torch.as_tensor(asked, dtype=torch.int32).to(dev), bank,
                        torch.as_tensor(bank_classes, dtype=torch.int32).to(dev), k)
    M = int(queries.shape[0])
    back = torch.cat([t.double().flatten() for t in out]).cpu().numpy()            # positions < 2^31 are exact in fp64
    cut = np.cumsum([0, M * k, M * k, M, M, M, M])
    d2, idx, sd, si, od, oi = (back[cut[i]:cut[i + 1]] for i in range(6))
    idx = idx.reshape(M, k).astype(np.int64)
    classes = np.asarray(bank_classes, dtype=np.int64)
    nbr = np.where(idx < len(classes), classes[np.minimum(idx, len(classes) - 1)], -1)
    return {"d2": d2.reshape(M, k), "idx": idx, "neighbour_classes": nbr, "same_d2": sd, "same_idx": si.astype(np.int64),
            "other_d2": od, "other_idx": oi.astype(np.int64)}


def figures_of(found, asked, image):
    return OA.figures(asked, found["neighbour_classes"], found["same_d2"], found["same_idx"], found["other_d2"], found["other_idx"],
                      image)


def _u8(crop, channels, side):
    a = np.asarray(crop, dtype=np.float32).reshape(channels, side, side)
    a = np.clip((a + 1.0) * 127.5, 0, 255).astype(np.uint8)
    return np.repeat(a, 3, axis=0).transpose(1, 2, 0) if channels == 1 else a.transpose(1, 2, 0)


def oa_grid(save_dir, rows, channels, side):
    """oa_grid.png: one row per entry of `rows`, a list of crops (D,) in [-1, 1] or None (an empty tile):
    [generated crop | nearest of the asked class | nearest of another class | the K neighbours].  Returns the file's name."""
    from PIL import Image
    width = max(len(r) for r in rows)
    sheet = np.zeros((len(rows) * side, width * side, 3), dtype=np.uint8)
    for r, tiles in enumerate(rows):
        for j, t in enumerate(tiles):
            if t is not None:
                sheet[r * side:(r + 1) * side, j * side:(j + 1) * side] = _u8(t, channels, side)
    Image.fromarray(sheet).save('%s/oa_grid.png' % save_dir)
    return "oa_grid.png"


class FamilyEvaluation:
    """The scores of one checkpoint of a family tree.  trainer: the tree's GANTrainer (cfg, model, tree, device, prepare_batch, the
    network loaders); loader: the evaluation split's, unshuffled; split: its name; bank: (dataset, name) of the train split, or None
    where object accuracy is not asked; `synthetic`: the data is synthetic, and the JSON says so."""

    def __init__(self, trainer, stage, loader, split, bank=None, synthetic=False):
        self.trainer, self.cfg, self.stage, self.loader, self.split = trainer, trainer.cfg, int(stage), loader, split
        self.variant, self.device = trainer.model.VARIANT, trainer.device
        self.bank, self.synthetic = bank, bool(synthetic)
        self.size, self.channels = (256 if self.stage == 2 else 64), self.variant.img_ch

    # ------------------------------------------------------------------------------------------ the pass
    def save_dir(self):
        net_g = self.cfg.NET_G
        d = net_g[:net_g.rfind('.pth')] + '/' + self.split
        mkdir_p(d)
        return d

    def images(self, num_samples):
        return max(1, min(int(num_samples), len(self.loader.dataset)))

    def load_generator(self):
        nets = self.trainer.load_network_stageI() if self.stage == 1 else self.trainer.load_network_stageII()
        return None if nets is None else nets[0].eval()

    def one_pass(self, num_samples, seed, image_sinks=(), resample_sinks=(), object_sinks=(), generate=None):
        """real and generated images of the loader's first `num_samples` items to the sinks: image_sinks (real, fake, take),
        resample_sinks (fake, fake_again, take), object_sinks (real, fake, tm, label_one_hot, take) with the matrices of the boxes at
        the images' own size.  `generate`, where given, makes a batch's image in generate_seeded's place: it is called with (netG,
        prepared batch, the seeded generator, take, images before the batch) and owes the pass generate_seeded's draws and image
        (layout_shift() generates a second image from the same draws there).  Returns the number of images."""
        netG = self.load_generator()
        if netG is None:
            raise ValueError("evaluate: the generator could not be loaded (cfg.NET_G = %r)" % (self.cfg.NET_G,))
        gen = torch.Generator(device=self.device)
        gen.manual_seed(int(seed))
        gen_again = None
        if resample_sinks:
            gen_again = torch.Generator(device=self.device)
            gen_again.manual_seed(int(seed) + 1)
        rows, n = self.images(num_samples), 0
        for data in self.loader:
            if n >= rows:
                break
            b = self.trainer.prepare_batch(data, self.stage)
            take = min(int(b["real_imgs"].shape[0]), rows - n)
            with torch.no_grad():
                if generate is None:
                    fake = generate_seeded(netG, self.variant, self.stage, self.cfg, b, gen)
                else:
                    fake = generate(netG, b, gen, take, n)
                for sink in resample_sinks:
                    sink(fake, generate_seeded(netG, self.variant, self.stage, self.cfg, b, gen_again), take)
                for sink in image_sinks:
                    sink(b["real_imgs"], fake, take)
                for sink in object_sinks:
                    sink(b["real_imgs"], fake, b["tm_s2"] if self.stage == 2 else b["tm"], b["label_one_hot"], take)
            n += take
        return n

    # ------------------------------------------------------------------------------------------ the accumulators
    def make(self, name, num_samples, seed, kw):
        images = self.images(num_samples)
        if name == "swd":
            from ..attngan.swd import SlicedWasserstein
            return SlicedWasserstein(self.size, self.channels, images * int(kw["patches"]), kw["patches"], kw["dirs"], kw["repeats"],
                                     kw["min_res"], seed, self.device)
        if name == "msssim":
            from ..attngan.msssim import PairFigures
            return PairFigures(self.size, self.channels, images, kw["scales"], kw["same_caption"], seed, self.device)
        if name == "spectrum":
            from ..attngan.spectrum import RadialSpectrum
            return RadialSpectrum(self.size, self.channels, images, kw["window"], self.device, seed=seed)
        return ObjectCrops(self.trainer.tree, images, self.size, self.channels, self.variant.max_objects, kw["side"], kw["min_side"],
                           self.device)

    def run_scores(self, asked, num_samples=30000, seed=100, return_crops=False):
        """The scores `asked` names (score -> its keyword arguments) from ONE pass, finished in SCORES order: score -> the content
        of its JSON.  With return_crops the object-accuracy entry is (content, crops): the host crops and classes of the pass."""
        if not asked or set(asked) - set(SCORES):
            raise ValueError("run_scores: one score at least of %s expected, got %s" % (list(SCORES), list(asked)))
        if self.cfg.NET_G == '':
            print('Error: the path for model NET_G is not found!')
            return None
        accs = {name: self.make(name, num_samples, seed, asked[name]) for name in SCORES if name in asked}
        n = self.one_pass(
            num_samples, seed,
            image_sinks=[accs[name].sink for name in ("swd", "msssim", "spectrum") if name in accs],
            resample_sinks=[accs["msssim"].resample_sink] if "msssim" in accs and accs["msssim"].resample_sink is not None else [],
            object_sinks=[accs["object_accuracy"].sink] if "object_accuracy" in accs else [])
        if n < 1:
            raise ValueError("evaluate: the data loader gave no batch")
        out = {}
        for name, acc in accs.items():
            out[name] = getattr(self, name)(acc, n, seed, **dict(asked[name], **({"return_crops": return_crops}
                                                                                 if name == "object_accuracy" else {})))
        return out

    def write(self, name, out, seed, note):
        out.update({"seed": int(seed), "NET_G": self.cfg.NET_G, "tree": self.variant.name, "stage": self.stage, "size": self.size,
                    "channels": self.channels, "split": self.split, "note": note})
        d = self.save_dir()
        with open('%s/%s.json' % (d, name), 'w') as f:
            json.dump(out, f, indent=1, sort_keys=True)
        return d

    # ------------------------------------------------------------------------------------------ the image scores
    def swd(self, acc, n, seed, **kw):
        res = acc.result()
        out = {"swd": res["swd"], "levels": res["levels"], "per_level": res["per_level"], "patches": acc.patches, "dirs": acc.dirs,
               "repeats": acc.repeats, "n_real": n, "n_fake": n}
        d = self.write("swd", out, seed,
                       "Sliced Wasserstein distance x 1000 between Laplacian-pyramid descriptors (7x7 neighbourhoods) of the real and "
                       "the generated images, per level and averaged: trunk-free.  It depends on the number of descriptors per image "
                       "(patches = %d), on dirs, repeats and the seed, and is comparable under equal settings only.  The images enter "
                       "as fp32 in [-1, 1], not quantised to 8 bits." % acc.patches)
        print("SWD (%d real, %d generated %dx%d images): %.4f = mean of %s at levels %s -> %s/swd.json"
              % (n, n, self.size, self.size, out["swd"], ["%.4f" % v for v in out["per_level"]], out["levels"], d))
        return out

    def msssim(self, acc, n, seed, **kw):
        if any(f.n < 1 for f in acc.figures.values()):
            raise ValueError("msssim: the data loader gave no pair of images")
        out = {}
        for name, f in acc.figures.items():
            res = f.result()
            out[name] = {k: res[k] for k in ("mean", "std", "ssim", "cs", "pairs", "clamped")}
        out.update({"levels": list(acc.figures["real"].sizes), "scales": acc.scales})
        d = self.write("msssim", out, seed,
                       "Multi-scale structural similarity between pairs of images, mean and population standard deviation over the "
                       "pairs, with the per-level means of ssim and cs: trunk-free.  HIGHER means LESS varied.  real / generated: "
                       "within a batch row j against row j + take // 2.  same_caption: two images for one layout, labels and text "
                       "under independent noise (a second generator seeded seed + 1); near 1 means the generator ignores its noise.  "
                       "A pair with a negative level mean scores 0 and is counted as clamped.  The images enter as fp32 in [-1, 1].")
        print("MS-SSIM (%d scales; mean +- std over pairs): %s -> %s/msssim.json"
              % (acc.scales, ", ".join("%s %.4f +- %.4f (%d pairs)" % (k, out[k]["mean"], out[k]["std"], out[k]["pairs"])
                                       for k in ("real", "generated", "same_caption") if k in out), d))
        return out

    def spectrum(self, acc, n, seed, **kw):
        out = acc.result()
        m = out.pop("n")
        out.update({"window": acc.window, "n_real": m, "n_fake": m})
        d = self.write("spectrum", out, seed,
                       "Radial (azimuthally averaged) power spectrum of the luminance of the real and the generated images, in dB per "
                       "bin of integer radius, with the log-spectral distance lsd_db, the high-frequency excess hf_db, the spectral "
                       "slopes and the bin of the largest excess with its period in pixels: trunk-free.  Every figure depends on the "
                       "window (%s) and is comparable under the same window only.  The images enter as fp32 in [-1, 1]." % acc.window)
        print("Spectrum (%d real, %d generated %dx%d images; window %s): LSD %.4f dB -> %s/spectrum.json"
              % (m, m, self.size, self.size, acc.window, out["lsd_db"], d))
        return out

    # ------------------------------------------------------------------------------------------ layout shift
    def layout_shift(self, num_samples=30000, seed=100, min_shift=None, min_side=1, show=16, image_sink=None):
        """Layout control by moving ONE box (attngan/layoutshift.py has the definition): every item's image is
        generated twice from the same z / eps / eps_s1, labels and text -- A under the data's matrices, the image every score of
        run_scores sees under `seed`, and B with only the moved slot's inverse matrix replaced -- and hip/ops.box_shift_sums scores
        the pairs, one launch per batch.  Stage II moves both box sets by the same relative offset and scores the 256 x 256 image at
        the stage-II boxes.  A mode of its own, not a row of SCORES.  `image_sink`, where given, is called once per batch with
        (A, B, edit table, take).  Writes layout_shift.json and, where show > 0, layout_grid.png; returns the JSON's content."""
        from ..attngan.evaluate import moved_matrices
        from ..attngan.layoutshift import ShiftResponse, layout_grid
        if self.cfg.NET_G == '':
            print('Error: the path for model NET_G is not found!')
            return None
        acc = ShiftResponse(self.size, self.channels, self.images(num_samples), min_shift, min_side, seed, self.device, keep=show)
        scored = "tm_s2" if self.stage == 2 else "tm"

        def pair(netG, b, gen, take, first):
            b = draw_noise(self.variant, self.stage, self.cfg, b, gen)
            a = generate(netG, self.variant, self.stage, b)[0]
            table = acc.edits(boxes_from_theta(b[scored].cpu()), take)                # the one read-back of the layout
            edited = dict(b)
            if self.stage == 2:
                # the stage-I boxes travel by the same RELATIVE offset: (dx, dy) / 256, rounded once to fp32
                moved = boxes_from_theta(b["tm"].cpu())[table["row"], table["slot"]].double()
                moved[:, :2] += table["edit"][:, 4:6].double() / float(self.size)
                edited["tmi"] = moved_matrices(b["tmi"], table, moved.float())
                edited["tmi_s2"] = moved_matrices(b["tmi_s2"], table)
            else:
                edited["tmi"] = moved_matrices(b["tmi"], table)
            again = generate(netG, self.variant, self.stage, edited)[0]
            acc.add(a.float(), again.float(), table,
                    keys=[dataset_key(self.loader.dataset, first + j) for j in range(int(a.shape[0]))])
            if image_sink is not None:
                image_sink(a, again, table, take)
            return a
        self.one_pass(num_samples, seed, generate=pair)
        out = acc.result(show)
        out.update({"show": len(out["most_ignored"]), "grid": None})
        d = self.save_dir()
        if acc.kept:
            out["grid"] = layout_grid(d, acc.kept, acc.info)
        note = ("Layout control by moving one box: every image is generated twice from the same noise, labels and text, under the "
                "data's layout (A) and with one object's box moved by at least min_shift pixels (B).  follow = 1 - moved / baseline "
                "over the old rectangle: 1 -- the object travelled with its box, 0 -- the edit was ignored.  locality: the share of the "
                "squared change inside the old and the new rectangle; area_share is its chance level.  spill_others / "
                "spill_background: the mean squared change per pixel in the other objects' rectangles / in the rest, over that of the "
                "box pixels.  mean +- population std over the pairs; flat, unchanged, no_objects and immovable are counted.  Every "
                "figure depends on min_shift and min_side.")
        if self.synthetic:
            note += " Synthetic data."
        self.write("layout_shift", out, seed, note)
        shown = lambda v: "n/a" if v["mean"] is None else "%.4f +- %.4f (%d)" % (v["mean"], v["std"], v["n"])
        print("Layout shift (%d pairs of %d %dx%d images; %d without objects, %d immovable, %d unchanged, %d flat; min_shift %d px): "
              "follow %s, locality %s at area share %s -> %s/layout_shift.json%s"
              % (out["n_pairs"], out["n_images"], self.size, self.size, out["no_objects"], out["immovable"], out["unchanged"],
                 out["flat"], out["min_shift"], shown(out["follow"]), shown(out["locality"]), shown(out["area_share"]), d,
                 "" if out["grid"] is None else " and %s" % out["grid"]))
        return out

    # ------------------------------------------------------------------------------------------ object accuracy
    def bank_crops(self, side, min_side, bank_size=None):
        """(crops (N, D) on the device, classes (N,), image (N,), box (N, 4), dataset, images read): the labelled objects of the first `bank_size`
        real images of the bank's dataset (all where None), in dataset order.  No generator runs.  The global generators' states are
        put back, so nothing a pass draws depends on this call."""
        import random
        dataset = self.bank[0]
        rows = len(dataset) if bank_size is None else max(1, min(int(bank_size), len(dataset)))
        states = torch.get_rng_state(), np.random.get_state(), random.getstate()
        try:
            loader = torch.utils.data.DataLoader(torch.utils.data.Subset(dataset, range(rows)), batch_size=int(self.loader.batch_size),
                                                 shuffle=False, num_workers=int(self.loader.num_workers))
            acc = ObjectCrops(self.trainer.tree, rows, self.size, self.channels, self.variant.max_objects, side, min_side, self.device,
                              both=False)
            for data in loader:
                b = self.trainer.prepare_batch(data, self.stage)
                acc.sink(b["real_imgs"], None, b["tm_s2"] if self.stage == 2 else b["tm"], b["label_one_hot"], b["real_imgs"].shape[0])
        finally:
            torch.set_rng_state(states[0])
            np.random.set_state(states[1])
            random.setstate(states[2])
        classes, image, slot, box = acc.objects()
        return acc.finish()["real"], classes.numpy(), image.numpy(), box.numpy(), dataset, rows

    def object_accuracy(self, acc, n, seed, k=5, side=16, min_side=1, bank_size=None, show=16, return_crops=False):
        """Object accuracy by nearest labelled training crops (stackgan/objaccuracy.py has the definition) from the accumulator a pass
        has fed: both query sets against the bank of the train split, hip/ops.knn_label twice, two read-backs.  k is lowered to the
        bank's size where that is smaller, and the JSON records it.  Writes object_accuracy.json (and oa_grid.png where show > 0)."""
        k, show = int(k), int(show)
        if k < 1 or k > 8 or show < 0:
            raise ValueError("object_accuracy: 1 <= k <= 8 and show >= 0 expected, got k = %d, show = %d" % (k, show))
        if self.bank is None:
            raise ValueError("object_accuracy: no train split to build the bank from")
        if acc.n < 1:
            raise ValueError("object_accuracy: the pass saw no labelled object")
        crops = acc.finish()
        asked, image, slot, box = (t.numpy() for t in acc.objects())
        bank, bank_classes, bank_image, bank_box, dataset, bank_rows = self.bank_crops(acc.side, acc.min_side, bank_size)
        n_bank = 0 if bank is None else int(bank.shape[0])
        if n_bank < 1:
            raise ValueError("object_accuracy: the bank holds no labelled object")
        kk = min(k, n_bank)
        found = {name: search(crops[name], asked, bank, bank_classes, kk) for name in ("fake", "real")}
        out = {"generated": figures_of(found["fake"], asked, image), "real": figures_of(found["real"], asked, image)}
        rows, margin = OA.most_wrong(found["fake"]["same_d2"], found["fake"]["other_d2"], show)
        voted = OA.vote(found["fake"]["neighbour_classes"])
        f = found["fake"]

        def at(position):
            p = int(position)
            return None if p == OA.NO_ROW else {"bank_row": p, "image": int(bank_image[p]), "key": dataset_key(dataset, int(bank_image[p])),
                                                "class": int(bank_classes[p])}
        listing = []
        for r, m in zip(rows.tolist(), margin.tolist()):
            listing.append({"row": r, "image": int(image[r]), "slot": int(slot[r]), "box": [float(v) for v in box[r]],
                            "asked": int(asked[r]), "voted": int(voted[r]), "margin": None if np.isnan(m) else m,
                            "d2": f["d2"][r].tolist(), "neighbours": [at(p) for p in f["idx"][r]],
                            "same": at(f["same_idx"][r]), "same_d2": float(f["same_d2"][r]) if np.isfinite(f["same_d2"][r]) else None,
                            "other": at(f["other_idx"][r]),
                            "other_d2": float(f["other_d2"][r]) if np.isfinite(f["other_d2"][r]) else None})
        d = self.save_dir()
        grid = None
        if listing:
            host_fake, host_bank = crops["fake"].cpu().numpy(), bank.cpu().numpy()
            tiles = [[host_fake[e["row"]]] + [None if p is None else host_bank[p["bank_row"]]
                                              for p in [e["same"], e["other"]] + e["neighbours"]] for e in listing]
            grid = oa_grid(d, tiles, self.channels, acc.side)
        note = ("Object accuracy by nearest labelled training crops: every object of the evaluation split is cut at the data's box out "
                "of the generated image (generated) and out of the real image (real: the data's own ceiling), resized to side x side "
                "and searched among the crops of the train split's objects; accuracy: the vote of the k nearest crops equals the "
                "class the generator was given; accuracy_1nn: the nearest crop is of that class; margin: the mean of (sqrt d_other - "
                "sqrt d_same) / (sqrt d_other + sqrt d_same).  No trunk, no weights: the judge is the training set.  Every figure "
                "depends on side (%d), k (%d) and the bank (%d objects of %d images): comparable at equal settings only."
                % (acc.side, kk, n_bank, bank_rows))
        if self.synthetic:
            note += " Synthetic data: the bank is a second synthetic set with a seed of its own, not a split of real images."
        if kk < k:
            note += " k lowered from %d to %d: the bank holds only %d objects." % (k, kk, n_bank)
        out.update({"k": kk, "side": acc.side, "min_side": acc.min_side, "D": acc.D, "n_images": n, "n_objects": int(acc.n),
                    "unlabelled": int(acc.unlabelled), "n_bank": n_bank, "n_bank_images": bank_rows,
                    "bank_split": self.bank[1], "classes": OA.CLASSES[acc.tree], "show": len(listing), "most_wrong": listing,
                    "grid": grid})
        self.write("object_accuracy", out, seed, note)
        g, r = out["generated"], out["real"]
        print("Object accuracy (%d objects of %d images against %d training crops; k = %d, side = %d): generated %.4f (1-NN %.4f, "
              "margin %s), real %.4f (1-NN %.4f) -> %s/object_accuracy.json%s"
              % (acc.n, n, n_bank, kk, acc.side, g["accuracy"], g["accuracy_1nn"],
                 "n/a" if g["margin"] is None else "%+.4f" % g["margin"], r["accuracy"], r["accuracy_1nn"], d,
                 "" if grid is None else " and %s" % grid))
        if return_crops:
            return out, {"fake": crops["fake"].cpu(), "real": crops["real"].cpu(), "bank": bank.cpu(), "asked": asked, "image": image,
                         "bank_classes": bank_classes}
        return out
