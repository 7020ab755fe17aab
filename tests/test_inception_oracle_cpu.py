"""The decision hooks of the fp64 Inception oracle (oracle/inception_oracle.py: RELU_MASKS, POOL_ARGMAX, FLIPS), on the CPU.

The GPU tests impose the ReLU and max-pool decisions of a HIP run on the oracle; that is only sound if (1) the hooked oracle
with its OWN decisions is the unhooked oracle, bit for bit, and (2) the decisions of an fp32 run of the same arithmetic
differ from the fp64 ones only at elements within rounding of a kink."""
import pytest
import torch

from helpers import load_pkg

load_pkg()
from oracle import inception_oracle as IO  # noqa: E402

# an imposed decision that differs from the oracle's own must lie this close to its kink, relative to the rms of the
# site's input (fp32 forward error of the trunk is ~1e-6 of the rms)
KINK_REL = 1e-4


def trunk_state(seed):
    """random trunk weights (He-normal, as attngan.inception.init_trunk) with non-trivial eval-mode BN statistics"""
    from mogan_amd.attngan import inception
    g = torch.Generator().manual_seed(seed)
    sd = {}
    enc = torch.nn.Module()
    for name, make in inception.TRUNK:
        enc.add_module(name, make())
    for k, v in enc.state_dict().items():
        if k.endswith("num_batches_tracked"):
            continue
        if k.endswith("conv.weight"):
            sd[k] = torch.randn(v.shape, generator=g) * (2.0 / v[0].numel()) ** 0.5
        elif k.endswith("running_mean"):
            sd[k] = torch.randn(v.shape, generator=g) * 0.05
        elif k.endswith("running_var"):
            sd[k] = torch.rand(v.shape, generator=g) * 0.4 + 0.8
        elif k.endswith("bn.weight"):
            sd[k] = torch.rand(v.shape, generator=g) * 0.2 + 0.9
        else:
            sd[k] = torch.randn(v.shape, generator=g) * 0.05
    return {k: v.double() for k, v in sd.items()}


def record_decisions(monkeypatch):
    """run the oracle recording its own decisions: ({layer: mask}, {pool site: window offsets})"""
    masks, pools = {}, {}
    relu, maxpool = IO._relu, IO._maxpool

    def rec_relu(p, x):
        masks[p] = (x.detach() > 0).clone()
        return relu(p, x)

    def rec_pool(site, x):
        pools[site] = IO.pool_offsets(x.detach())
        return maxpool(site, x)
    monkeypatch.setattr(IO, "_relu", rec_relu)
    monkeypatch.setattr(IO, "_maxpool", rec_pool)
    return masks, pools


def run(sd, x, gf, gl):
    x = x.clone().requires_grad_(True)
    f, last = IO.trunk(sd, x)
    gx, = torch.autograd.grad((f * gf).sum() + (last * gl).sum(), x)
    return f.detach(), last.detach(), gx


@pytest.fixture(autouse=True)
def _unhook():
    yield
    IO.RELU_MASKS = IO.POOL_ARGMAX = IO.FLIPS = None


def test_own_decisions_reproduce_the_oracle_bitwise(monkeypatch):
    sd = trunk_state(1)
    torch.manual_seed(0)
    x = torch.rand(1, 3, 139, 139, dtype=torch.float64) * 2 - 1
    f0, l0, _ = run(sd, x, 0, 0)                          # shapes only
    gf, gl = torch.randn_like(f0), torch.randn_like(l0)
    f0, l0, g0 = run(sd, x, gf, gl)
    with monkeypatch.context() as m:
        masks, pools = record_decisions(m)
        run(sd, x, gf, gl)
    assert len(masks) == 94 and set(pools) == {"pool1", "pool2", "Mixed_6a.pool", "Mixed_7a.pool"}
    IO.RELU_MASKS, IO.POOL_ARGMAX, IO.FLIPS = masks, pools, {}
    f1, l1, g1 = run(sd, x, gf, gl)
    assert torch.equal(f1, f0) and torch.equal(l1, l0) and torch.equal(g1, g0)
    assert len(IO.FLIPS) == 98 and all(v[0] == 0 for v in IO.FLIPS.values())
    # a decision imposed against the oracle's own is reported, and changes the result
    p = "Mixed_5b.branch1x1"
    IO.RELU_MASKS = dict(masks, **{p: ~masks[p]})
    IO.FLIPS = {}
    f2, _, _ = run(sd, x, gf, gl)
    assert IO.FLIPS[p][0] == masks[p].numel() and not torch.equal(f2, f0)


def test_fp32_decisions_flip_only_at_kinks(monkeypatch):
    sd = trunk_state(2)
    torch.manual_seed(1)
    x = torch.rand(1, 3, 299, 299, dtype=torch.float64) * 2 - 1
    sd32 = {k: v.float() for k, v in sd.items()}
    f0, l0, _ = run(sd, x, 0, 0)
    gf, gl = torch.randn_like(f0), torch.randn_like(l0)
    with monkeypatch.context() as m:
        masks, pools = record_decisions(m)
        f32, l32, g32 = run(sd32, x.float(), gf.float(), gl.float())
    _, _, g_own = run(sd, x, gf, gl)
    IO.RELU_MASKS, IO.POOL_ARGMAX, IO.FLIPS = masks, pools, {}
    f1, l1, g1 = run(sd, x, gf, gl)
    rel = lambda a, b: float((a.double() - b).norm() / b.norm())
    flips = sum(v[0] for v in IO.FLIPS.values())
    worst = max(v[2] / v[3] for v in IO.FLIPS.values())
    print("fp32 CPU decisions on fp64: %d flips, worst |pre| / rms %.1e; image gradient vs fp64: own decisions %.1e, matched %.1e"
          % (flips, worst, rel(g32, g_own), rel(g32, g1)))
    assert worst <= KINK_REL, {k: v for k, v in IO.FLIPS.items() if v[0]}
    assert rel(f32, f1) < 5e-6 and rel(l32, l1) < 5e-6
    # with the decisions matched, what is left of the image-gradient difference is fp32 rounding
    assert rel(g32, g1) < 1e-5, rel(g32, g1)
