"""Entry point of the coco-attngan variant (mirror of code/coco/attngan/main.py): same flags
(--cfg --gpu --resume --data_dir --manualSeed), plus --synthetic N to train on generated batches when the
COCO pickles are not present.  One process per GPU: launch with
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 main.py --cfg cfg/coco_train.yml
(`--gpu` is kept for compatibility; the device comes from LOCAL_RANK).

Evaluation (TRAIN.FLAG False): every score of evaluate.SCORES has a flag of its name, `asked_scores` maps the flags to each score's
keywords, and CheckpointEvaluation.run_scores gives any number of them from one pass.  A new score adds its flags and its entry there.
--layout_shift (CheckpointEvaluation.layout_shift) and --inception_score (CheckpointEvaluation.inception_score) are modes of their own
beside --sampling and --r_precision, and so is --scenes FILE (CheckpointEvaluation.scenes): images from captions, boxes and labels the
user wrote.  --trunk PATH loads the image encoder's Inception trunk from a torchvision file; --trunk_variant fid runs such a file's
weights as the published FID Inception network."""
import argparse
import datetime
import os
import pprint
import random
import sys

import numpy as np
import torch
import torch.distributed as dist

if __package__ in (None, ""):
    sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.realpath(__file__)), "..", "..")))
    import mogan_loader
    mogan_loader.load()
    from mogan_amd.attngan.miscc.config import cfg, cfg_from_file
    from mogan_amd.attngan.datasets import SyntheticTextDataset, TextDataset
    from mogan_amd.attngan.evaluate import SCORES
    from mogan_amd.attngan.trainer import condGANTrainer as trainer
    from mogan_amd.hip import lib as hiplib
else:
    from .miscc.config import cfg, cfg_from_file
    from .datasets import SyntheticTextDataset, TextDataset
    from .evaluate import SCORES
    from .trainer import condGANTrainer as trainer
    from ..hip import lib as hiplib


POOL_CODE_MODES = ('fid', 'kid', 'prdc', 'scene_fid', 'memorisation', 'inception_score')     # what --trunk_variant serves


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='Train a AttnGAN network')
    parser.add_argument('--cfg', dest='cfg_file', help='optional config file', default='cfg/coco_train.yml', type=str)
    parser.add_argument('--gpu', dest='gpu_id', type=str, default='0')
    parser.add_argument('--resume', dest='resume', type=str, default='')
    parser.add_argument('--data_dir', dest='data_dir', type=str, default='')
    parser.add_argument('--manualSeed', type=int, help='manual seed')
    parser.add_argument('--synthetic', type=int, default=0, help='train on N generated samples instead of COCO')
    parser.add_argument('--max_epoch', type=int, default=None)
    parser.add_argument('--batch_size', type=int, default=None, help='per-GPU minibatch')
    parser.add_argument('--output_dir', type=str, default='')
    parser.add_argument('--device_feeder', action='store_true',
                        help='real data: workers only decode + resize the JPEGs; crop / flip / multi-scale / normalise run '
                             'on the GPU (attngan/feeder.py, bit-identical images, 5x less PCIe traffic)')
    parser.add_argument('--sampling', action='store_true',
                        help='evaluation (TRAIN.FLAG False): one image per caption of the whole split (sampling()) '
                             'instead of the 25 rows of sample()')
    parser.add_argument('--r_precision', action='store_true',
                        help='evaluation (TRAIN.FLAG False): R-precision of TRAIN.NET_G under the DAMSM pair TRAIN.NET_E over the '
                             'split (condGANTrainer.r_precision) -> <NET_G minus .pth>/<split>/r_precision.json')
    parser.add_argument('--real', action='store_true',
                        help='with --r_precision: score the real images instead of generated ones (the ceiling of the encoder pair)')
    parser.add_argument('--fid', action='store_true',
                        help='evaluation (TRAIN.FLAG False): Frechet distance between the Inception pool codes of the real images and of '
                             'TRAIN.NET_G\'s images under the trunk of TRAIN.NET_E\'s image encoder (condGANTrainer.fid) -> '
                             '<NET_G minus .pth>/<split>/fid.json; not together with --sampling or --r_precision')
    parser.add_argument('--fid_stats', type=str, default=None, metavar='PATH',
                        help='with --fid: the real images\' statistics as an .npz -- loaded when it exists and was taken under the same '
                             'trunk, computed and saved there otherwise')
    parser.add_argument('--kid', action='store_true',
                        help='evaluation (TRAIN.FLAG False): kernel Inception distance between the same pool codes (condGANTrainer.kid: '
                             'unbiased, no dependence on the number of images) -> <NET_G minus .pth>/<split>/kid.json; with --fid both '
                             'scores come from one pass; not together with --sampling or --r_precision')
    parser.add_argument('--kid_subsets', type=int, default=100, metavar='N', help='with --kid: number of random subset pairs')
    parser.add_argument('--kid_subset_size', type=int, default=1000, metavar='N',
                        help='with --kid: codes per subset (lowered to the number of images where there are fewer)')
    parser.add_argument('--prdc', action='store_true',
                        help='evaluation (TRAIN.FLAG False): improved precision / recall and density / coverage between the same pool '
                             'codes (condGANTrainer.prdc: "collapsed" and "sloppy" told apart) -> <NET_G minus .pth>/<split>/prdc.json; '
                             'any of --fid --kid --prdc together take one pass; not together with --sampling or --r_precision')
    parser.add_argument('--prdc_k_pr', type=int, default=3, metavar='K', help='with --prdc: neighbours of precision / recall (1..8)')
    parser.add_argument('--prdc_k_dc', type=int, default=5, metavar='K', help='with --prdc: neighbours of density / coverage (1..8)')
    parser.add_argument('--swd', action='store_true',
                        help='evaluation (TRAIN.FLAG False): sliced Wasserstein distance between Laplacian-pyramid descriptors of the '
                             'real and the generated images themselves (condGANTrainer.swd: no image encoder involved, one figure per '
                             'pyramid level) -> <NET_G minus .pth>/<split>/swd.json; with any of --fid --kid --prdc all take one pass; '
                             'not together with --sampling or --r_precision')
    parser.add_argument('--swd_patches', type=int, default=128, metavar='N', help='with --swd: 7x7 descriptors per image and level')
    parser.add_argument('--swd_dirs', type=int, default=128, metavar='N', help='with --swd: random directions per repeat (1..1024)')
    parser.add_argument('--swd_repeats', type=int, default=4, metavar='N', help='with --swd: repeats of the random projection')
    parser.add_argument('--swd_min_res', type=int, default=16, metavar='S',
                        help='with --swd: the coarsest pyramid level (256 / S must be a power of two)')
    parser.add_argument('--msssim', action='store_true',
                        help='evaluation (TRAIN.FLAG False): multi-scale structural similarity between pairs of real images, the same '
                             'pairs of generated images, and two images per caption under independent noise (condGANTrainer.msssim: '
                             'no image encoder involved; higher = less varied) -> <NET_G minus .pth>/<split>/msssim.json; with any of '
                             '--fid --kid --prdc --swd all take one pass; not together with --sampling or --r_precision')
    parser.add_argument('--msssim_scales', type=int, default=5, metavar='N', help='with --msssim: number of scales (1..5)')
    parser.add_argument('--msssim_no_resample', action='store_true',
                        help='with --msssim: leave the second image per caption, and so the same_caption figure, out')
    parser.add_argument('--spectrum', action='store_true',
                        help='evaluation (TRAIN.FLAG False): radial power spectrum of the real against the generated images '
                             '(condGANTrainer.spectrum: no image encoder involved; the log-spectral distance, the high-frequency '
                             'excess, the spectral slopes and the period of the largest excess -- the grids and checkerboards of the '
                             'up-convolutions) -> <NET_G minus .pth>/<split>/spectrum.json; with any of --fid --kid --prdc --swd '
                             '--msssim --scene_fid --memorisation all take one pass; not together with --sampling or --r_precision')
    parser.add_argument('--spectrum_window', type=str, default='hann', choices=('hann', 'none'),
                        help='with --spectrum: the window applied before the transform (every figure depends on it)')
    parser.add_argument('--scene_fid', action='store_true',
                        help='evaluation (TRAIN.FLAG False): object-level Frechet distance (SceneFID) -- every object of the data cut '
                             'at its box out of the real and out of the generated image, resized to the trunk\'s input and scored as '
                             '--fid scores whole images (condGANTrainer.scene_fid) -> <NET_G minus .pth>/<split>/scene_fid.json; with '
                             'any of --fid --kid --prdc --swd --msssim all take one pass; not together with --sampling or --r_precision')
    parser.add_argument('--scene_fid_min_side', type=float, default=1, metavar='PX',
                        help='with --scene_fid: leave out boxes whose shorter side is below PX pixels of the 256x256 image')
    parser.add_argument('--memorisation', action='store_true',
                        help='evaluation (TRAIN.FLAG False): is the generator reproducing its TRAINING images?  The pool codes of the '
                             'generated and of the split\'s real images against their nearest neighbours in a bank of the train '
                             'split\'s real images (condGANTrainer.memorisation: authenticity, its held-out value, copying, and the '
                             'most suspicious images next to their nearest training images) -> <NET_G minus .pth>/<split>/'
                             'memorisation.json and nn_grid.png; with any of --fid --kid --prdc --swd --msssim --scene_fid all take '
                             'one pass; not together with --sampling or --r_precision')
    parser.add_argument('--nn_bank', type=str, default=None, metavar='PATH',
                        help='with --memorisation: the training bank as an .npz -- loaded when it exists and was taken under the same '
                             'trunk, computed and saved there otherwise')
    parser.add_argument('--nn_bank_size', type=int, default=None, metavar='N',
                        help='with --memorisation: the first N training images only (every figure depends on the bank\'s size)')
    parser.add_argument('--nn_k', type=int, default=5, metavar='K', help='with --memorisation: training neighbours listed and drawn per image (1..8)')
    parser.add_argument('--nn_show', type=int, default=16, metavar='M',
                        help='with --memorisation: the M most suspicious generated images are listed and drawn (0: no nn_grid.png)')
    parser.add_argument('--layout_shift', action='store_true',
                        help='evaluation (TRAIN.FLAG False): layout control by moving ONE box -- every image generated twice from the '
                             'same noise, text and labels, under the data\'s layout and with one object\'s box moved; does the object '
                             'travel with its box (follow), and does anything else change (locality, spill)?  '
                             '(condGANTrainer.layout_shift: no image encoder involved) -> <NET_G minus .pth>/<split>/layout_shift.json '
                             'and layout_grid.png; a mode of its own: not together with --sampling, --r_precision or any score flag')
    parser.add_argument('--ls_min_shift', type=int, default=None, metavar='PX',
                        help='with --layout_shift: the box moves by PX pixels at least along one axis (an eighth of the side by default)')
    parser.add_argument('--ls_min_side', type=float, default=1, metavar='PX',
                        help='with --layout_shift: leave out boxes whose shorter side is below PX pixels')
    parser.add_argument('--ls_show', type=int, default=16, metavar='N',
                        help='with --layout_shift: the N pairs that followed the edit least are listed and drawn (0: no layout_grid.png)')
    parser.add_argument('--trunk', type=str, default=None, metavar='PATH',
                        help='evaluation (TRAIN.FLAG False): load the image encoder\'s Inception trunk from this file -- torchvision\'s '
                             'inception_v3_google-*.pth (old or new layout) or any image_encoder*.pth -- so that with NET_E: \'\' the '
                             'scores on pool codes run under ImageNet features; the generated images are those of a pass without it; '
                             'beside a NET_E the file must hold that pair\'s trunk')
    parser.add_argument('--trunk_variant', type=str, default='torchvision', choices=('torchvision', 'fid'),
                        help='with --trunk: the network the file\'s weights are run as -- torchvision\'s Inception-v3, or fid: the '
                             'published FID Inception network (pt_inception-2015-12-05-*.pth, the PyTorch port of the 2015 TensorFlow '
                             'graph; other pooling in the Mixed blocks\' pool branches), for --fid --kid --prdc --scene_fid '
                             '--memorisation --inception_score; beside a NET_E the file\'s trunk then replaces that pair\'s; not '
                             'together with --r_precision')
    parser.add_argument('--inception_score', action='store_true',
                        help='evaluation (TRAIN.FLAG False): Inception Score of TRAIN.NET_G\'s images -- the softmax of a classifier '
                             'head over their Inception pool codes (condGANTrainer.inception_score) -> <NET_G minus .pth>/<split>/'
                             'inception_score.json; a mode of its own: not together with --sampling, --r_precision, --layout_shift or '
                             'any score flag')
    parser.add_argument('--is_head', type=str, default=None, metavar='PATH',
                        help='with --inception_score: the file with the head, fc.weight (C, D) and fc.bias (C); by default the '
                             '--trunk file.  A trunk in the same file must be the one the pass runs under')
    parser.add_argument('--is_splits', type=int, default=10, metavar='N',
                        help='with --inception_score: contiguous splits of the pass (lowered to the number of images where fewer)')
    parser.add_argument('--is_real', action='store_true',
                        help='with --inception_score: the same figures for the real images (the ceiling the data gets) and the KL '
                             'divergence between the two marginals')
    parser.add_argument('--scenes', type=str, default=None, metavar='FILE',
                        help='evaluation (TRAIN.FLAG False): images of TRAIN.NET_G from written scenes -- a JSON file {"scenes": [{"name", '
                             '"caption", "objects": [{"label", "box": [x, y, w, h]}], "samples"?, "sweep"?: {"object", "to": [x, y], '
                             '"steps"}}]} (attngan/scenes.py; condGANTrainer.scenes) -> <NET_G minus .pth>/scenes/<name>/ with the three '
                             'stages of every sample, the attention sheets of the top words, samples.png and sweep.png, and scenes.json; '
                             'a mode of its own: not together with --sampling, --r_precision, --layout_shift, --inception_score or any '
                             'score flag')
    parser.add_argument('--scene_samples', type=int, default=4, metavar='N', help='with --scenes: images per scene where the scene does not say (1..64)')
    parser.add_argument('--scene_topk', type=int, default=5, metavar='K', help='with --scenes: words per attention sheet (1..8)')
    parser.add_argument('--scene_no_attention', action='store_true', help='with --scenes: write no attention sheets')
    parser.add_argument('--scene_classes', type=str, default=None, metavar='FILE',
                        help='with --scenes: one class name per line; a label may then be a name of this file')
    args = parser.parse_args(argv)
    for name in list(SCORES) + ['layout_shift', 'inception_score', 'scenes']:
        if getattr(args, name) and (args.sampling or args.r_precision):
            parser.error('--%s cannot be combined with --sampling or --r_precision' % name)
    for name in list(SCORES) + ['layout_shift', 'inception_score']:
        if getattr(args, name) and args.scenes:
            parser.error('--%s cannot be combined with --scenes' % name)
    if not 1 <= args.scene_samples <= 64 or not 1 <= args.scene_topk <= 8:
        parser.error('--scene_samples must be in 1..64 and --scene_topk in 1..8')
    for name in SCORES:
        if getattr(args, name) and args.layout_shift:
            parser.error('--%s cannot be combined with --layout_shift' % name)
    for name in list(SCORES) + ['layout_shift']:
        if getattr(args, name) and args.inception_score:
            parser.error('--%s cannot be combined with --inception_score' % name)
    if args.trunk_variant != 'torchvision':
        if not args.trunk:
            parser.error('--trunk_variant %s runs the weights of a file: it needs --trunk' % args.trunk_variant)
        if args.r_precision:
            parser.error('--trunk_variant %s cannot be combined with --r_precision: that score runs the DAMSM heads' % args.trunk_variant)
        if not any(getattr(args, name) for name in POOL_CODE_MODES):
            parser.error('--trunk_variant %s serves the modes that read pool codes: one of %s'
                         % (args.trunk_variant, ' '.join('--' + name for name in POOL_CODE_MODES)))
    if args.is_splits < 1:
        parser.error('--is_splits must be 1 at least')
    if args.ls_show < 0 or (args.ls_min_shift is not None and args.ls_min_shift < 1):
        parser.error('--ls_show must not be negative and --ls_min_shift must be 1 at least')
    if not 0 <= args.ls_min_side < float('inf'):                      # NaN fails both comparisons
        parser.error('--ls_min_side must be a finite number of pixels, 0 at least')
    if not 1 <= args.nn_k <= 8:
        parser.error('--nn_k must be in 1..8')
    if args.nn_show < 0 or (args.nn_bank_size is not None and args.nn_bank_size < 2):
        parser.error('--nn_show must not be negative and --nn_bank_size must be 2 at least')
    return args


def asked_scores(args):
    """score -> that score's own keyword arguments, for the scores of evaluate.SCORES whose flag is set, in the table's order"""
    every = {"scene_fid": dict(min_side=args.scene_fid_min_side),
             "swd": dict(patches=args.swd_patches, dirs=args.swd_dirs, repeats=args.swd_repeats, min_res=args.swd_min_res),
             "msssim": dict(scales=args.msssim_scales, same_caption=not args.msssim_no_resample),
             "spectrum": dict(window=args.spectrum_window),
             "fid": dict(stats_path=args.fid_stats),
             "kid": dict(subsets=args.kid_subsets, subset_size=args.kid_subset_size),
             "prdc": dict(k_pr=args.prdc_k_pr, k_dc=args.prdc_k_dc),
             "memorisation": dict(bank_path=args.nn_bank, bank_size=args.nn_bank_size, k=args.nn_k, show=args.nn_show)}
    return {name: every[name] for name in SCORES if getattr(args, name)}


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
    if args.trunk and cfg.TRAIN.FLAG:
        raise SystemExit("--trunk is an evaluation flag (TRAIN.FLAG False): training takes its image encoder from TRAIN.NET_E, and "
                         "pretrain_DAMSM.py --trunk starts a DAMSM pair from the file")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if cfg.TRAIN.FLAG and not torch.cuda.is_initialized():
        # the eager multi-stream step: 4 hardware queues, and the engine's streams created / bound to them in their fixed order
        # before RCCL creates its own (hip/lib.py "hardware queues", trainer.create_engine_streams)
        hiplib.configure_hw_queues()
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        hiplib.reserve_hw_queues()
        from .trainer import create_engine_streams
        create_engine_streams()
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("TORCH_NCCL_HIGH_PRIORITY", "1")       # RCCL's stream on its own priority queue (see bench.py)
        dist.init_process_group("nccl", rank=rank, world_size=world)
    if rank == 0:
        print('Using config:')
        pprint.pprint(cfg)
    if args.manualSeed is None:
        args.manualSeed = 100 if not cfg.TRAIN.FLAG else random.randint(1, 10000)
    stamp = datetime.datetime.now().strftime('%Y_%m_%d_%H_%M_%S')
    if world > 1:
        # ONE seed and ONE output directory for the job: rank 0 draws them (each rank's `random` is unseeded, so the
        # draws would differ), everybody else takes rank 0's
        shared = [args.manualSeed, stamp]
        dist.broadcast_object_list(shared, src=0)
        args.manualSeed, stamp = shared
    random.seed(args.manualSeed + rank)
    np.random.seed(args.manualSeed + rank)
    # common torch seed for the weight initialisation (the engine additionally broadcasts rank 0's weights, buffers and
    # optimizer state: TrainEngine.sync_replicas); condGANTrainer.train() re-seeds per rank afterwards for z / eps
    torch.manual_seed(args.manualSeed)
    if args.resume == '':
        output_dir = args.output_dir or '../../../output/%s_%s_%s' % (cfg.DATASET_NAME, cfg.CONFIG_NAME, stamp)
    else:
        output_dir = args.resume
    # main.py:117-121: evaluation reads the test split and the dataset hands the scaled boxes along
    split_dir, evaluate = ('train', False) if cfg.TRAIN.FLAG else ('test', True)
    asked = asked_scores(args)
    with_bbox = evaluate and not (args.sampling or args.r_precision or asked or args.layout_shift or args.inception_score or args.scenes)
    if args.synthetic > 0:
        dataset = SyntheticTextDataset(args.synthetic, seed=args.manualSeed, eval=with_bbox)   # one dataset, partitioned below
    else:
        dataset = TextDataset(cfg.DATA_DIR, cfg.IMG_DIR, split_dir, base_size=cfg.TREE.BASE_SIZE, eval=with_bbox,
                              raw=args.device_feeder and cfg.TRAIN.FLAG)
    assert dataset
    sampler = None
    if world > 1 and cfg.TRAIN.FLAG:
        # every rank trains on its own 1/world partition of each epoch (same permutation seed on all ranks, re-drawn per
        # epoch through sampler.set_epoch in condGANTrainer.train)
        sampler = torch.utils.data.distributed.DistributedSampler(dataset, num_replicas=world, rank=rank, shuffle=True,
                                                                  seed=int(args.manualSeed), drop_last=True)
    loader = torch.utils.data.DataLoader(dataset, batch_size=cfg.TRAIN.BATCH_SIZE, drop_last=True,
                                         shuffle=sampler is None, sampler=sampler,
                                         num_workers=min(int(cfg.WORKERS), 8 if args.synthetic else int(cfg.WORKERS)))
    # the trunk file reaches the trainer only where the flag is given: a trainer without the keyword serves every other run
    extra = {'trunk': args.trunk} if args.trunk else {}
    if args.trunk_variant != 'torchvision':
        extra['trunk_variant'] = args.trunk_variant
    algo = trainer(output_dir, loader, dataset.n_words, dataset.ixtoword, args.resume, distributed=world > 1, **extra)
    if cfg.TRAIN.FLAG:
        algo.train()
    elif args.sampling:
        algo.sampling(split_dir)                  # main.py:157 (commented alternative): the whole validation split
    elif args.r_precision:
        algo.r_precision(split_dir, seed=args.manualSeed, real=args.real)
    elif args.layout_shift:
        algo.layout_shift(split_dir, seed=args.manualSeed, min_shift=args.ls_min_shift, min_side=args.ls_min_side, show=args.ls_show)
    elif args.inception_score:
        algo.inception_score(split_dir, seed=args.manualSeed, head_path=args.is_head, splits=args.is_splits, real=args.is_real)
    elif args.scenes:
        from .scenes import read_classes
        algo.scenes(args.scenes, seed=args.manualSeed, samples=args.scene_samples, topk=args.scene_topk,
                    attention=not args.scene_no_attention, classes=read_classes(args.scene_classes) if args.scene_classes else None)
    elif asked:
        # any number of scores from ONE pass over the loader (evaluate.SCORES says what each takes from it); one score alone runs
        # its own method, which may then leave out what a shared pass needs (the trunk, the real images' codes)
        algo.run_scores(split_dir, asked, seed=args.manualSeed)
    elif cfg.B_VALIDATION:
        algo.sample(split_dir, num_samples=25, draw_bbox=True)                      # main.py:158
    else:
        # main.py:160 gen_example: not callable in the reference (it passes num_samples to a two-argument function and
        # trainer.gen_example calls G_NET without boxes and labels); --scenes is this project's form of it
        raise SystemExit("custom captions come from a scene file: --scenes FILE (or set B_VALIDATION: True)")
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
