"""CPU oracle for the CNN_ENCODER trunk (reference: code/coco/attngan/model.py:207-313, which wraps
torchvision.models.inception_v3 -- torchvision==0.2.1, requirements.txt:31, NOT vendored under
/root/reference and not installed here).  PARITY UNPINNED for the Inception arithmetic: there is no
reference implementation or fixture to check against, so this is a functional torch-CPU restatement
of the published architecture (Szegedy et al., "Rethinking the Inception Architecture for Computer
Vision", 2015; torchvision layer names) that the HIP trunk is compared with.  What is downstream of
it (emb_features, emb_cnn_code, words_loss, sent_loss) IS pinned by tests/golden/losses.npz.
TEST INFRASTRUCTURE ONLY (tests/, smoke(), bench.py cpu_baseline).

The encoder is frozen and in eval mode in the train step (trainer.py:62-66): BN uses running stats.
`sd` is a state_dict with torchvision key names (e.g. Mixed_5b.branch1x1.conv.weight).
"""
import torch
import torch.nn.functional as F


RELU_MASKS = None    # test hook: {layer name (torchvision prefix, e.g. "Mixed_5b.branch1x1"): bool tensor}, see _relu
POOL_ARGMAX = None   # test hook: {pool site ("pool1", "pool2", "Mixed_6a.pool", "Mixed_7a.pool"): window offsets}, see _maxpool
FLIPS = None         # test hook: a dict that receives, per hooked decision site, (imposed decisions that differ from the
#                      oracle's own, decisions, largest |pre-activation| (ReLU) or max - chosen value (pool) among them, rms of
#                      the site's input)


def _flip(site, diff, dist, x):
    if FLIPS is not None:
        n = int(diff.sum())
        FLIPS[site] = (n, diff.numel(), float(dist[diff].max()) if n else 0.0, float(x.detach().pow(2).mean().sqrt()))


def _relu(p, x):
    """F.relu.  Test hook: when RELU_MASKS holds layer p, the decision of every element is taken from there (the decisions the
    checked implementation made) instead of from x itself -- the value and the gradient of the SAME piecewise-linear function
    at the checked run's kink sides; pre-activations within fp32 noise of the kink otherwise flip a few decisions per layer
    and move the input gradient by up to ~1e-2 through the 94 layers."""
    m = RELU_MASKS.get(p) if RELU_MASKS is not None else None
    if m is None:
        return F.relu(x)
    assert m.shape == x.shape and m.dtype == torch.bool, (p, tuple(m.shape), tuple(x.shape), m.dtype)
    _flip(p, m != (x.detach() > 0), x.detach().abs(), x)
    return torch.where(m, x, torch.zeros((), dtype=x.dtype))


def _maxpool(site, x):
    """F.max_pool2d(x, 3, 2).  Test hook: when POOL_ARGMAX holds the site, each window takes the element at the given offset
    a * 3 + b (uint8 / integer tensor shaped like the output; the rule of the kernels and of torch-CPU is the first maximum)
    instead of its own maximum; the gradient goes to that element."""
    a = POOL_ARGMAX.get(site) if POOL_ARGMAX is not None else None
    if a is None:
        return F.max_pool2d(x, 3, 2)
    B, C, H, W = x.shape
    OH, OW = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    a = a.long()
    assert tuple(a.shape) == (B, C, OH, OW) and int(a.min()) >= 0 and int(a.max()) < 9, (site, tuple(a.shape))
    oy = torch.arange(OH).view(OH, 1) * 2
    ox = torch.arange(OW).view(1, OW) * 2
    flat = ((oy + a // 3) * W + ox + a % 3).reshape(B, C, -1)        # input position of the chosen element
    y = torch.gather(x.reshape(B, C, H * W), 2, flat).reshape(B, C, OH, OW)
    own = F.max_pool2d(x.detach(), 3, 2)
    _flip(site, y.detach() != own, own - y.detach(), x)
    return y


def pool_offsets(x):
    """window offset a * 3 + b of the first maximum of every 3x3 / stride-2 window of x (the rule of torch-CPU and of the
    kernels) -- the form POOL_ARGMAX takes"""
    B, C, H, W = x.shape
    _, i = F.max_pool2d(x, 3, 2, return_indices=True)
    OH, OW = i.shape[2], i.shape[3]
    a = i // W - torch.arange(OH, device=x.device).view(OH, 1) * 2
    b = i % W - torch.arange(OW, device=x.device).view(1, OW) * 2
    return (a * 3 + b).to(torch.uint8)


def _bc(sd, p, x, stride=1, padding=0):
    """BasicConv2d: conv(bias=False) -> BN(eps=1e-3, eval) -> ReLU."""
    x = F.conv2d(x, sd[p + ".conv.weight"], None, stride, padding)
    x = F.batch_norm(x, sd[p + ".bn.running_mean"], sd[p + ".bn.running_var"], sd[p + ".bn.weight"],
                     sd[p + ".bn.bias"], False, 0.0, 0.001)
    return _relu(p, x)


def _a(sd, p, x):
    b1 = _bc(sd, p + ".branch1x1", x)
    b5 = _bc(sd, p + ".branch5x5_2", _bc(sd, p + ".branch5x5_1", x), 1, 2)
    b3 = _bc(sd, p + ".branch3x3dbl_1", x)
    b3 = _bc(sd, p + ".branch3x3dbl_3", _bc(sd, p + ".branch3x3dbl_2", b3, 1, 1), 1, 1)
    bp = _bc(sd, p + ".branch_pool", F.avg_pool2d(x, 3, 1, 1))
    return torch.cat([b1, b5, b3, bp], 1)


def _b(sd, p, x):
    b3 = _bc(sd, p + ".branch3x3", x, 2)
    bd = _bc(sd, p + ".branch3x3dbl_2", _bc(sd, p + ".branch3x3dbl_1", x), 1, 1)
    bd = _bc(sd, p + ".branch3x3dbl_3", bd, 2)
    return torch.cat([b3, bd, _maxpool(p + ".pool", x)], 1)


def _c(sd, p, x):
    b1 = _bc(sd, p + ".branch1x1", x)
    b7 = _bc(sd, p + ".branch7x7_1", x)
    b7 = _bc(sd, p + ".branch7x7_2", b7, 1, (0, 3))
    b7 = _bc(sd, p + ".branch7x7_3", b7, 1, (3, 0))
    bd = _bc(sd, p + ".branch7x7dbl_1", x)
    for n, pad in (("2", (3, 0)), ("3", (0, 3)), ("4", (3, 0)), ("5", (0, 3))):
        bd = _bc(sd, p + ".branch7x7dbl_" + n, bd, 1, pad)
    bp = _bc(sd, p + ".branch_pool", F.avg_pool2d(x, 3, 1, 1))
    return torch.cat([b1, b7, bd, bp], 1)


def _d(sd, p, x):
    b3 = _bc(sd, p + ".branch3x3_2", _bc(sd, p + ".branch3x3_1", x), 2)
    b7 = _bc(sd, p + ".branch7x7x3_1", x)
    b7 = _bc(sd, p + ".branch7x7x3_2", b7, 1, (0, 3))
    b7 = _bc(sd, p + ".branch7x7x3_3", b7, 1, (3, 0))
    b7 = _bc(sd, p + ".branch7x7x3_4", b7, 2)
    return torch.cat([b3, b7, _maxpool(p + ".pool", x)], 1)


def _e(sd, p, x):
    b1 = _bc(sd, p + ".branch1x1", x)
    b3 = _bc(sd, p + ".branch3x3_1", x)
    b3 = torch.cat([_bc(sd, p + ".branch3x3_2a", b3, 1, (0, 1)), _bc(sd, p + ".branch3x3_2b", b3, 1, (1, 0))], 1)
    bd = _bc(sd, p + ".branch3x3dbl_2", _bc(sd, p + ".branch3x3dbl_1", x), 1, 1)
    bd = torch.cat([_bc(sd, p + ".branch3x3dbl_3a", bd, 1, (0, 1)), _bc(sd, p + ".branch3x3dbl_3b", bd, 1, (1, 0))], 1)
    bp = _bc(sd, p + ".branch_pool", F.avg_pool2d(x, 3, 1, 1))
    return torch.cat([b1, b3, bd, bp], 1)


def trunk(sd, x299):
    """Conv2d_1a_3x3 .. Mixed_7c on a (B,3,299,299) image -> (Mixed_6e output (B,768,17,17), Mixed_7c output (B,2048,8,8))."""
    x = _bc(sd, "Conv2d_1a_3x3", x299, 2)
    x = _bc(sd, "Conv2d_2a_3x3", x)
    x = _bc(sd, "Conv2d_2b_3x3", x, 1, 1)
    x = _maxpool("pool1", x)
    x = _bc(sd, "Conv2d_3b_1x1", x)
    x = _bc(sd, "Conv2d_4a_3x3", x)
    x = _maxpool("pool2", x)
    for n in ("5b", "5c", "5d"):
        x = _a(sd, "Mixed_" + n, x)
    x = _b(sd, "Mixed_6a", x)
    for n in ("6b", "6c", "6d", "6e"):
        x = _c(sd, "Mixed_" + n, x)
    feat = x
    x = _d(sd, "Mixed_7a", x)
    x = _e(sd, "Mixed_7b", x)
    x = _e(sd, "Mixed_7c", x)
    return feat, x


BLOCKS = {"Mixed_5b": _a, "Mixed_5c": _a, "Mixed_5d": _a, "Mixed_6a": _b, "Mixed_6b": _c, "Mixed_6c": _c, "Mixed_6d": _c,
          "Mixed_6e": _c, "Mixed_7a": _d, "Mixed_7b": _e, "Mixed_7c": _e}


def block(sd, name, x):
    """one Mixed block of the trunk"""
    return BLOCKS[name](sd, name, x)


def cnn_encoder(sd, x):
    """model.py:252-313 -> (regions (B,nef,17,17), code (B,nef))."""
    x = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False)
    feat, x = trunk(sd, x)
    x = F.avg_pool2d(x, 8).reshape(x.shape[0], -1)
    code = F.linear(x, sd["emb_cnn_code.weight"], sd["emb_cnn_code.bias"])
    return F.conv2d(feat, sd["emb_features.weight"]), code
