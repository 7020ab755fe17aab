"""Shared entry point of the three StackGAN-style trees (code/coco/stackgan/main.py, code/clevr/main.py,
code/multi-mnist/main.py): --cfg / --gpu / --data_dir / --manualSeed as in the reference -- real data through ..datasets' TextDatasets when
TRAIN.FLAG, `sample` from the checkpoint cfg.NET_G otherwise -- plus --synthetic N (train on N synthetic items: there are no
datasets on the GPU box), --max_epoch, --batch_size, --output_dir, --graph.  With TRAIN.FLAG False and any of --object_accuracy
--swd --msssim --spectrum the checkpoint is SCORED instead of sampled: one pass over the evaluation split (the 'test' split, or N
synthetic items) serves all the asked scores (stackgan/evaluate.py); --layout_shift, a mode of its own, scores
the checkpoint's layout control by moving one box.  Each tree's
main.py binds its own cfg / trainer to `run`."""
import argparse
import datetime
import os
import pprint
import random

import torch

from . import datasets
from .datasets_synth import SyntheticDataset


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='Train a GAN network')
    parser.add_argument('--cfg', dest='cfg_file', help='optional config file', default=None, type=str)
    parser.add_argument('--gpu', dest='gpu_id', type=str, default='0')
    parser.add_argument('--data_dir', dest='data_dir', type=str, default='')
    parser.add_argument('--manualSeed', type=int, help='manual seed')
    parser.add_argument('--synthetic', type=int, default=0)
    parser.add_argument('--max_epoch', type=int, default=None)
    parser.add_argument('--batch_size', type=int, default=None)
    parser.add_argument('--output_dir', type=str, default=None)
    parser.add_argument('--graph', action='store_true')
    scores = 'evaluation (TRAIN.FLAG False): '
    parser.add_argument('--object_accuracy', action='store_true',
                        help=scores + 'object accuracy by nearest labelled training crops: every object of the evaluation split cut at '
                             'its box out of the generated and out of the real image and searched among the train split\'s object crops '
                             '-> <NET_G minus .pth>/<split>/object_accuracy.json and oa_grid.png; all score flags together take one pass')
    parser.add_argument('--oa_k', type=int, default=5, metavar='K', help='with --object_accuracy: neighbours that vote (1..8)')
    parser.add_argument('--oa_side', type=int, default=16, metavar='S', help='with --object_accuracy: the crops are resized to S x S')
    parser.add_argument('--oa_min_side', type=float, default=1, metavar='PX',
                        help='with --object_accuracy: leave out boxes whose shorter side is below PX pixels')
    parser.add_argument('--oa_bank_size', type=int, default=None, metavar='N',
                        help='with --object_accuracy: the bank is the first N images of the train split (all by default)')
    parser.add_argument('--oa_show', type=int, default=16, metavar='M',
                        help='with --object_accuracy: the M generated objects with the smallest margin are listed and drawn')
    parser.add_argument('--swd', action='store_true', help=scores + 'sliced Wasserstein distance -> swd.json')
    parser.add_argument('--swd_patches', type=int, default=128, metavar='N', help='with --swd: 7x7 descriptors per image and level')
    parser.add_argument('--swd_dirs', type=int, default=128, metavar='N', help='with --swd: random directions per repeat (1..1024)')
    parser.add_argument('--swd_repeats', type=int, default=4, metavar='N', help='with --swd: repeats of the random projection')
    parser.add_argument('--swd_min_res', type=int, default=16, metavar='S', help='with --swd: the coarsest pyramid level')
    parser.add_argument('--msssim', action='store_true', help=scores + 'multi-scale structural similarity of pairs -> msssim.json')
    parser.add_argument('--msssim_scales', type=int, default=5, metavar='N', help='with --msssim: number of scales (1..5)')
    parser.add_argument('--msssim_no_resample', action='store_true',
                        help='with --msssim: leave the second image per item, and so the same_caption figure, out')
    parser.add_argument('--spectrum', action='store_true', help=scores + 'radial power spectrum -> spectrum.json')
    parser.add_argument('--spectrum_window', type=str, default='hann', choices=('hann', 'none'),
                        help='with --spectrum: the window applied before the transform')
    parser.add_argument('--layout_shift', action='store_true',
                        help=scores + 'layout control by moving ONE box: every image generated twice from the same noise, labels and '
                             'text, under the data\'s layout and with one object\'s box moved -> layout_shift.json and layout_grid.png; '
                             'a mode of its own: not together with any score flag')
    parser.add_argument('--ls_min_shift', type=int, default=None, metavar='PX',
                        help='with --layout_shift: the box moves by PX pixels at least along one axis (an eighth of the side by default)')
    parser.add_argument('--ls_min_side', type=float, default=1, metavar='PX',
                        help='with --layout_shift: leave out boxes whose shorter side is below PX pixels')
    parser.add_argument('--ls_show', type=int, default=16, metavar='N',
                        help='with --layout_shift: the N pairs that followed the edit least are listed and drawn (0: no layout_grid.png)')
    parser.add_argument('--num_samples', type=int, default=30000, metavar='N', help='with a score flag: images scored at most')
    args = parser.parse_args(argv)
    for name in ('object_accuracy', 'swd', 'msssim', 'spectrum'):
        if getattr(args, name) and args.layout_shift:
            parser.error('--%s cannot be combined with --layout_shift' % name)
    if args.ls_show < 0 or (args.ls_min_shift is not None and args.ls_min_shift < 1):
        parser.error('--ls_show must not be negative and --ls_min_shift must be 1 at least')
    if not 0 <= args.ls_min_side < float('inf'):                      # NaN fails both comparisons
        parser.error('--ls_min_side must be a finite number of pixels, 0 at least')
    return args


def evaluation_datasets(tree, cfg, stage, args, want_bank):
    """(evaluation dataset, split name, (bank dataset, name) or None) for a scoring run: the 'test' split and, for the bank, the
    'train' split without crop or flip, each image resized to the tree's size; under --synthetic N two synthetic sets, the bank's
    under a seed of its own"""
    from .evaluate import BANK_SEED_STEP
    imsize = 256 if stage == 2 else 64
    if args.synthetic:
        text_dim = cfg.TEXT.DIMENSION if "TEXT" in cfg else 0
        ds = SyntheticDataset(tree, stage, args.synthetic, seed=args.manualSeed, text_dim=text_dim)
        bank = SyntheticDataset(tree, stage, args.synthetic, seed=args.manualSeed + BANK_SEED_STEP, text_dim=text_dim)
        return ds, "synthetic", ((bank, "synthetic-train") if want_bank else None)

    def split(name):
        if tree == "coco":
            return datasets.CocoTextDataset(cfg.DATA_DIR, cfg.IMG_DIR, split=name, imsize=imsize,
                                            transform=datasets.image_transform(imsize), crop=False, stage=stage, fixed=True)
        if tree == "clevr":
            return datasets.ClevrTextDataset(cfg.DATA_DIR, split=name, imsize=64, transform=datasets.image_transform(), flip=False)
        return datasets.MnistTextDataset(cfg.DATA_DIR, split=name, imsize=64, transform=datasets.image_transform(), crop=False)
    return split("test"), "test", ((split("train"), "train") if want_bank else None)


def score(tree, cfg, stage, trainer_cls, args, asked, output_dir):
    """TRAIN.FLAG False with score flags: one pass over the evaluation split for all of `asked` (stackgan/evaluate.py)"""
    from .evaluate import FamilyEvaluation
    dataset, split, bank = evaluation_datasets(tree, cfg, stage, args, "object_accuracy" in asked)
    assert len(dataset) > 0
    workers = 0 if args.synthetic else int(cfg.get("WORKERS", 0))
    loader = torch.utils.data.DataLoader(dataset, batch_size=cfg.TRAIN.BATCH_SIZE, drop_last=False, shuffle=False, num_workers=workers)
    algo = trainer_cls(output_dir, use_graph=False)
    algo.evaluation = FamilyEvaluation(algo, stage, loader, split, bank, synthetic=bool(args.synthetic))
    if args.layout_shift:
        algo.scores = {"layout_shift": algo.evaluation.layout_shift(args.num_samples, args.manualSeed, args.ls_min_shift,
                                                                    args.ls_min_side, args.ls_show)}
    else:
        algo.scores = algo.evaluation.run_scores(asked, num_samples=args.num_samples, seed=args.manualSeed)
    return algo


def run(tree, cfg, cfg_from_file, trainer_cls, argv=None):
    args = parse_args(argv)
    if args.cfg_file is not None:
        cfg_from_file(args.cfg_file)
    if args.gpu_id != -1:
        cfg.GPU_ID = args.gpu_id
    if args.data_dir != '':
        cfg.DATA_DIR = args.data_dir
    if args.max_epoch is not None:
        cfg.TRAIN.MAX_EPOCH = args.max_epoch
    if args.batch_size is not None:
        cfg.TRAIN.BATCH_SIZE = args.batch_size
    print('Using config:')
    pprint.pprint(cfg)
    if args.manualSeed is None:
        args.manualSeed = random.randint(1, 10000)
    random.seed(args.manualSeed)
    torch.manual_seed(args.manualSeed)
    torch.cuda.manual_seed_all(args.manualSeed)
    timestamp = datetime.datetime.now().strftime('%Y_%m_%d_%H_%M_%S')
    output_dir = args.output_dir or '../../../output/%s_%s_%s' % (cfg.DATASET_NAME, cfg.CONFIG_NAME, timestamp)
    stage = int(cfg.get("STAGE", 1))
    from .evaluate import asked_scores
    asked = asked_scores(args)
    if (asked or args.layout_shift) and not cfg.TRAIN.FLAG:            # scoring a checkpoint (cfg.NET_G)
        return score(tree, cfg, stage, trainer_cls, args, asked, output_dir)
    if not cfg.TRAIN.FLAG:                                             # sampling from a checkpoint (cfg.NET_G)
        algo = trainer_cls(output_dir, use_graph=False)
        if tree == "coco":                                             # S/main.py:98-100
            algo.sample('%s/test/' % cfg.DATA_DIR, num_samples=25, stage=stage, draw_bbox=True)
        elif tree == "clevr":                                          # C/main.py:91-101
            ds = datasets.ClevrTextDataset(cfg.DATA_DIR, split="test", imsize=64, transform=datasets.image_transform())
            dl = torch.utils.data.DataLoader(ds, batch_size=1, drop_last=True, shuffle=True, num_workers=int(cfg.WORKERS))
            algo.sample(dl, num_samples=25, draw_bbox=True)
        else:                                                          # M/main.py:91-93
            algo.sample(os.path.join(cfg.DATA_DIR, "test"), num_samples=25, draw_bbox=True)
        return algo
    os.makedirs(output_dir, exist_ok=True)
    if args.synthetic:
        dataset = SyntheticDataset(tree, stage, args.synthetic, seed=args.manualSeed,
                                   text_dim=cfg.TEXT.DIMENSION if "TEXT" in cfg else 0)
    elif tree == "coco":                                               # S/main.py:77-90
        resize, imsize = (76, 64) if stage == 1 else (268, 256)
        dataset = datasets.CocoTextDataset(cfg.DATA_DIR, cfg.IMG_DIR, split="train", imsize=imsize,
                                           transform=datasets.image_transform(resize), crop=True, stage=stage)
    elif tree == "clevr":                                              # C/main.py:80-85
        dataset = datasets.ClevrTextDataset(cfg.DATA_DIR, split="train", imsize=64, transform=datasets.image_transform())
    else:                                                              # M/main.py:77-83
        dataset = datasets.MnistTextDataset(cfg.DATA_DIR, split="train", imsize=64, transform=datasets.image_transform(),
                                            crop=True)
    assert len(dataset) > 0
    workers = 0 if args.synthetic else int(cfg.get("WORKERS", 0))
    dataloader = torch.utils.data.DataLoader(dataset, batch_size=cfg.TRAIN.BATCH_SIZE, drop_last=True, shuffle=True,
                                             num_workers=workers)
    algo = trainer_cls(output_dir, use_graph=args.graph)
    algo.train(dataloader, stage)
    return algo
