"""What the tests of the trunk variants share: a plain helper module, not a conftest.

  * `restated(sd, x, variant)`: the whole trunk walk -- bilinear resize to 299, Conv2d_1a .. Mixed_7c, the 8 x 8 mean -- written out
    with plain torch functions in the dtype of its arguments (fp64 in the tests), for "torchvision" and for "fid".  It takes no
    arithmetic from the code under test; its "torchvision" form is tied to oracle/inception_oracle.py by a CPU test.
  * the pool branch's references for the kernel tests: `valid_mean` (fp64 avg_pool2d(count_include_pad=False), and the sum of the
    taps' magnitudes over their number, which the derived bound scales with).
  * the encoder, the inputs and the references of the trunk-level tests, computed once per process.
"""
import functools

import torch
import torch.nn.functional as F

VARIANTS = ("torchvision", "fid")
TOL = 2e-5                   # rel-L2 of the HIP trunk against the fp64 restatement: the figure test_cnn_encoder_vs_cpu_restatement holds
APART = 100 * TOL            # the two variants must differ by this at least, or the GPU test could not tell them apart
U = 2.0 ** -24               # unit roundoff of fp32
# mode 2 of the tail: every tap passes through at most 7 fp32 additions -- 2 in its row's sum, 2 more into the slab's sum (the first
# row is added to zero, exactly), and 3 where a second slab follows -- and the sum through one division: 8 roundings, each relative
# to a partial sum that sum |taps| bounds.  10 u sum |taps| / count leaves the second-order terms room.
MEAN_BOUND = 10 * U


def _cbr(sd, p, x, stride=1, pad=0):
    """BasicConv2d in eval mode: convolution, BatchNorm (eps 1e-3) from its running statistics, ReLU"""
    y = F.conv2d(x, sd[p + ".conv.weight"], None, stride, pad)
    inv = (sd[p + ".bn.running_var"] + 1e-3).rsqrt() * sd[p + ".bn.weight"]
    y = (y - sd[p + ".bn.running_mean"].view(1, -1, 1, 1)) * inv.view(1, -1, 1, 1) + sd[p + ".bn.bias"].view(1, -1, 1, 1)
    return y.clamp_min(0)


def _pool(x, variant, last=False):
    """the pool branch's pooling: the one place where the two networks differ"""
    if variant == "torchvision":
        return F.avg_pool2d(x, 3, 1, 1)
    if last:
        return F.max_pool2d(x, 3, 1, 1)
    return F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)


def _chain(sd, p, x, layers):
    for name, stride, pad in layers:
        x = _cbr(sd, p + "." + name, x, stride, pad)
    return x


def _mixed_a(sd, p, x, variant):
    return torch.cat([_cbr(sd, p + ".branch1x1", x),
                      _chain(sd, p, x, [("branch5x5_1", 1, 0), ("branch5x5_2", 1, 2)]),
                      _chain(sd, p, x, [("branch3x3dbl_1", 1, 0), ("branch3x3dbl_2", 1, 1), ("branch3x3dbl_3", 1, 1)]),
                      _cbr(sd, p + ".branch_pool", _pool(x, variant))], 1)


def _mixed_b(sd, p, x, variant):
    return torch.cat([_cbr(sd, p + ".branch3x3", x, 2),
                      _chain(sd, p, x, [("branch3x3dbl_1", 1, 0), ("branch3x3dbl_2", 1, 1), ("branch3x3dbl_3", 2, 0)]),
                      F.max_pool2d(x, 3, 2)], 1)


def _mixed_c(sd, p, x, variant):
    return torch.cat([_cbr(sd, p + ".branch1x1", x),
                      _chain(sd, p, x, [("branch7x7_1", 1, 0), ("branch7x7_2", 1, (0, 3)), ("branch7x7_3", 1, (3, 0))]),
                      _chain(sd, p, x, [("branch7x7dbl_1", 1, 0), ("branch7x7dbl_2", 1, (3, 0)), ("branch7x7dbl_3", 1, (0, 3)),
                                        ("branch7x7dbl_4", 1, (3, 0)), ("branch7x7dbl_5", 1, (0, 3))]),
                      _cbr(sd, p + ".branch_pool", _pool(x, variant))], 1)


def _mixed_d(sd, p, x, variant):
    return torch.cat([_chain(sd, p, x, [("branch3x3_1", 1, 0), ("branch3x3_2", 2, 0)]),
                      _chain(sd, p, x, [("branch7x7x3_1", 1, 0), ("branch7x7x3_2", 1, (0, 3)), ("branch7x7x3_3", 1, (3, 0)),
                                        ("branch7x7x3_4", 2, 0)]),
                      F.max_pool2d(x, 3, 2)], 1)


def _mixed_e(sd, p, x, variant, last=False):
    a = _cbr(sd, p + ".branch3x3_1", x)
    d = _chain(sd, p, x, [("branch3x3dbl_1", 1, 0), ("branch3x3dbl_2", 1, 1)])
    return torch.cat([_cbr(sd, p + ".branch1x1", x),
                      _cbr(sd, p + ".branch3x3_2a", a, 1, (0, 1)), _cbr(sd, p + ".branch3x3_2b", a, 1, (1, 0)),
                      _cbr(sd, p + ".branch3x3dbl_3a", d, 1, (0, 1)), _cbr(sd, p + ".branch3x3dbl_3b", d, 1, (1, 0)),
                      _cbr(sd, p + ".branch_pool", _pool(x, variant, last))], 1)


def restated(sd, x, variant):
    """images (B, 3, H, W) in [-1, 1] -> (the Mixed_6e map (B, 768, 17, 17), the pool code (B, 2048)) of the network `variant`"""
    assert variant in VARIANTS
    x = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False)
    x = _cbr(sd, "Conv2d_2b_3x3", _cbr(sd, "Conv2d_2a_3x3", _cbr(sd, "Conv2d_1a_3x3", x, 2)), 1, 1)
    x = F.max_pool2d(x, 3, 2)
    x = _cbr(sd, "Conv2d_4a_3x3", _cbr(sd, "Conv2d_3b_1x1", x))
    x = F.max_pool2d(x, 3, 2)
    for name in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
        x = _mixed_a(sd, name, x, variant)
    x = _mixed_b(sd, "Mixed_6a", x, variant)
    for name in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
        x = _mixed_c(sd, name, x, variant)
    feat = x
    x = _mixed_d(sd, "Mixed_7a", x, variant)
    x = _mixed_e(sd, "Mixed_7b", x, variant)
    x = _mixed_e(sd, "Mixed_7c", x, variant, last=True)
    return feat, x.mean(dim=(2, 3))


def rel_l2(got, want):
    return float((got.detach().cpu().double() - want.detach().cpu().double()).norm() / want.detach().cpu().double().norm())


# ------------------------------------------------------------------------------------------------------------ the trunk-level case
ENCODER_SEED, INPUT_SEED = 3, 17


def encoder(seed=ENCODER_SEED, nef=32):
    """a random-init CNN_ENCODER on the host with non-trivial eval-mode BatchNorm statistics (as test_cnn_encoder_vs_cpu_restatement
    sets them), frozen, in eval mode"""
    from mogan_amd.attngan import model
    from mogan_amd.attngan.miscc.config import cfg
    kept = cfg.TRAIN.FLAG
    cfg.TRAIN.FLAG = True
    try:
        torch.manual_seed(seed)
        enc = model.CNN_ENCODER(nef)
    finally:
        cfg.TRAIN.FLAG = kept
    for m in enc.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.05)
            m.running_var.uniform_(0.8, 1.2)
            m.weight.data.uniform_(0.9, 1.1)
            m.bias.data.normal_(0, 0.05)
    for p in enc.parameters():
        p.requires_grad = False
    return enc.eval()


def images(B=2, size=64, seed=INPUT_SEED):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, 3, size, size, generator=g) * 2 - 1


@functools.lru_cache(maxsize=None)
def references(B=2, size=64):
    """{variant: (Mixed_6e map, pool code)} in fp64 for encoder() on images(B, size); computed once, never modified"""
    sd = {k: v.detach().clone().double() for k, v in encoder().state_dict().items()}
    x = images(B, size).double()
    with torch.no_grad():
        return {v: restated(sd, x, v) for v in VARIANTS}


# ------------------------------------------------------------------------------------------------------- the kernel-level references
def valid_mean(slabs64):
    """(fp64 avg_pool2d(sum of the slabs, 3, 1, 1, count_include_pad=False), sum over every slab's taps of |tap| / count per
    element) of fp64 slabs (S, B, C, H, W)"""
    return (F.avg_pool2d(slabs64.sum(0), 3, 1, 1, count_include_pad=False),
            F.avg_pool2d(slabs64.abs().sum(0), 3, 1, 1, count_include_pad=False))


def trunk_file(path, seed=41, classes=7, head_seed=31):
    """a synthetic trunk file with torchvision's key names and a head of `classes` classes, as the published files are laid out:
    (weight, bias) of the head as numpy arrays"""
    import numpy as np
    from mogan_amd.attngan import inception, model
    rng = np.random.RandomState(head_seed)
    w = torch.from_numpy((rng.standard_normal((classes, 2048)) * 0.05).astype(np.float32))
    b = torch.from_numpy((rng.standard_normal(classes) * 0.5).astype(np.float32))
    torch.manual_seed(seed)
    state = {k: v.clone() for k, v in inception.trunk_entries(model.CNN_ENCODER(256)).items()}
    state.update({"fc.weight": w, "fc.bias": b})
    torch.save(state, path)
    return w.numpy(), b.numpy()
