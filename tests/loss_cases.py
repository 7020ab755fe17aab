"""Tables, inputs, fp64 references and per-element bounds of the entry points at the end of the train step, as include/mogan_hip.h
declares them -- mogan_logits_head_fwd / _bwd, mogan_bce_fwd / _bwd, mogan_bce_logits_fwd / _bwd, mogan_kl_fwd / _bwd,
mogan_reparam_fwd / _bwd, mogan_damsm_words_fwd / _bwd, mogan_damsm_ce_fwd / _bwd, mogan_damsm_sent_fwd / _bwd, mogan_scalar_sum /
_scale and mogan_adam_step (a plain helper module, not a conftest, like tests/pathway_cases.py).
tests/test_loss_entry_points_gpu.py runs the tables through the C ABI under tests/memguard.py;
tests/test_loss_reference_cpu.py keeps the references equal to the package's fp64 oracle, derives the TOL constants below from fp32
CPU evaluations and asserts the path coverage; tests/test_loss_rejections_cpu.py holds what the host refuses before a launch.
Nothing here needs a GPU or the library.

Paths, restated from the words of include/mogan_hip.h and the heads of csrc/mogan_damsm.hip / csrc/mogan_elem.hip /
csrc/mogan_smallc.hip (not read from the library):
    words           one workgroup of 320 threads (5 waves) per (image b, caption i); the word loops are unrolled over TT = 8, 12, 16, 24
                    or 32 slots (the smallest that holds T), slots past T re-read slot T - 1; the channel loop of the scores takes 8
                    channels at a time with the next 8 in flight (a second prefetch only while 16 more remain) and the rest one by
                    one; forward: the weighted context holds S <= 320 regions in registers and loops beyond; backward: a thread
                    takes the regions tid and tid + 320 (S <= 640).  LDS: (C T + T (S + 1) + 1088) floats <= 64 KB
    cross-entropies one block of 256 threads per row and per column, thread k takes the entries k, k + 256, ...
    sentence        one block per image; wave w takes the captions w, w + 4, ...; lanes stride the channels by 64
    logits head     one block of 256 threads per (b, co): thread k takes the float4 k, k + 256, ... in four chains
    bce / kl        one block of 256 threads, thread k takes the elements k, k + 256, ...; then six shuffle steps and four partial sums
    adam            one float4 per thread; the last one is ragged when n % 4 != 0 and moves element by element

Bounds.  |got - fp64| <= TOL[kind] * S + FLOOR per element, as in pathway_cases: S is first order in what an fp32 evaluation can
lose, in units of one rounding -- the sum of the absolute values of the terms that enter the element, times the condition of its last
nonlinear step.  FLOOR = 2^-126 (fp32's smallest normal number) stands wherever S > 0: a value below it may be flushed or lose
bits to gradual underflow (a sigmoid of -100), and no bound in units of the value's own roundings sees that.  S == 0 implies an exact
zero (every slot at t >= cap_lens[i], a masked probability, a gradient through a saturated sigmoid).
  sigmoid     p = 1 / (1 + e), e = exp(-z): e carries S_z + 2 + |z| roundings of its own size (__expf is v_exp_f32 of the
              fp32-rounded product with log2(e), pathway_cases), dp / de = -p^2, and the sum and the reciprocal round once each:
              S_p = p (1 - p) (S_z + 2 + |z|) + 2 p
  softmax     pathway_cases' model: p_k (A_k + sum_u p_u A_u + adds + 2), A_k = (roundings of the score) + 2 + 2 |arg_k|
  sums        a sum of n terms in a fixed tree: sum_i S_term_i + (additions of the longest chain) * sum_i |term_i|; dot products
              of the words / sentence kernels: sum |a||b|, the factor left to TOL as in conv_cases
  quotients   relative losses add: sqrt halves what its argument lost and rounds once
  the words backward takes a1, a2 and wc as fp32 INPUTS (the reference's, rounded), as pathway_cases' attention backward takes attn
Each S formula stands beside its reference below.
"""
import functools
import math

import numpy as np
import torch

from helpers import det_array
from pathway_cases import EPS32, TOL_CEILING, _exp32

f32 = np.float32
FLOOR = 2.0 ** -126
GAMMAS = (4.0, 5.0, 10.0)             # gamma1, gamma2, gamma3 (cfg.TRAIN.SMOOTH)
F64 = torch.float64

# Per-element tolerances: 4 x the largest err / S of the fp32 CPU evaluations over every row of the tables below
# (tests/test_loss_reference_cpu.py measures them, asserts the factor 4 and the ceiling, and prints the figures).  Measured, in units
# of 2^-24 (restatement of the kernel's formula in numpy fp32, operand order kept / torch's own fp32 CPU evaluation where torch has
# the operation):
#     p 0.442 / 0.515   head_dx 0.569 / 0.569   head_dw 0.580 / 0.580   head_db 0.228 / 0.228   bce 0.141 / 0.185
#     bce_dp 0.530 / 0.445   bcel 0.111 / 0.141   bcel_dx 0.726 / 0.726   kl 0.068 / 0.041   kl_dmu 0.632 / 0.632
#     kl_dlv 0.744 / 0.731   c 0.896 / 0.874   rp_dlv 0.637 / 0.420   sim 0.011 / 0.010   a1 1.689 / 1.591
#     a2 0.494 / 0.494   wc 0.088 / 0.110   dwc 0.242   dscore_t 0.031   prow 0.664 / 0.397
#     pcol 0.622 / 0.953   ce 0.405 / 0.159   ce_dsim 0.798   ssim 0.619 / 1.120   dcnn 0.512 / 0.460
#     sum 0.262 / 0.262   adam_p 0.995 / 0.995   adam_m 0.325 / 0.325   adam_v 0.647 / 0.647   adam_ema 0.642 / 0.642
MEASURED_UNITS = {
    "p": 0.52, "head_dx": 0.57, "head_dw": 0.58, "head_db": 0.23, "bce": 0.19, "bce_dp": 0.53, "bcel": 0.15, "bcel_dx": 0.73,
    "kl": 0.07, "kl_dmu": 0.64, "kl_dlv": 0.75, "c": 0.90, "rp_dlv": 0.64, "sim": 0.02, "a1": 1.69, "a2": 0.50,
    "wc": 0.11, "dwc": 0.25, "dscore_t": 0.04, "prow": 0.67, "pcol": 0.96, "ce": 0.41, "ce_dsim": 0.80, "ssim": 1.12,
    "dcnn": 0.52, "sum": 0.27, "adam_p": 1.00, "adam_m": 0.33, "adam_v": 0.65, "adam_ema": 0.65,
}
MEASURED = {k: v * EPS32 for k, v in MEASURED_UNITS.items()}
TOL = {k: min(4 * v, TOL_CEILING) for k, v in MEASURED.items()}
# the whole-tensor figures tests/test_kernels_gpu.py holds for these operations, asserted beside the bounds: rel-L2 1e-6 for the
# losses and what feeds them, 2e-5 for the DAMSM gradients, 2e-6 (max-abs) for the attention maps a2; 1e-6 (max-abs) for Adam at |p| ~ 3.
# a1 and wc -- a softmax over the words of a channel dot product and the context it weights -- have no figure there: theirs is pathway_cases'
# for the same two operations of the word attention (REL["attn"], REL["wc"])
REL = {"p": 1e-6, "head_dx": 1e-6, "head_dw": 1e-6, "head_db": 1e-6, "bce": 1e-6, "bce_dp": 1e-6, "bcel": 1e-6, "bcel_dx": 1e-6,
       "kl": 1e-6, "kl_dmu": 1e-6, "kl_dlv": 1e-6, "c": 1e-6, "rp_dlv": 1e-6, "sim": 1e-6, "a1": 5e-6, "a2": 2e-6, "wc": 5e-6,
       "dwc": 2e-5, "dscore_t": 2e-5, "prow": 2e-6, "pcol": 2e-6, "ce": 1e-6, "ce_dsim": 2e-5, "ssim": 1e-6, "dcnn": 2e-5, "sum": 1e-6,
       "adam_p": 1e-6, "adam_m": 1e-6, "adam_v": 1e-6, "adam_ema": 1e-6}
# kinds whose REL figure is a max-abs one (the attention maps' is max-abs in tests/test_kernels_gpu.py too)
ABSOLUTE = {"adam_p", "adam_m", "adam_v", "adam_ema", "a2"}


def T(name, shape, scale=1.0, shift=0.0):
    return torch.from_numpy(det_array(name, shape, scale, shift))


def bound(kind, S):
    """the per-element bound of an output kind: TOL * S, plus FLOOR wherever S > 0"""
    S = S.double()
    return TOL[kind] * S + FLOOR * (S > 0)


def figure(kind, got, ref):
    """the whole-tensor figure REL[kind] is asked of: rel-L2, or max-abs for the kinds of ABSOLUTE; inf where got is not finite"""
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    fin = torch.isfinite(ref)
    if not bool(torch.isfinite(got[fin]).all()):
        return float("inf")
    d = (got - ref)[fin]
    return float(d.abs().max()) if kind in ABSOLUTE else float(d.norm() / (ref[fin].norm() + 1e-30))


def _chain(n):
    """additions of the longest chain of a 256-thread block sum over n terms: the thread's own, six shuffle steps, four partials"""
    return (n + 255) // 256 + 6 + 3


def _sig(z):
    return torch.sigmoid(z)


def _butterfly(lanes, width=64):
    """xor-shuffle sum over the last axis (width lanes), fp32, the kernels' order: o = width / 2, ..., 1"""
    o = width // 2
    idx = np.arange(width)
    while o > 0:
        lanes = lanes + lanes[..., idx ^ o]
        o >>= 1
    return lanes[..., 0]


def _shfl_down_sum(lanes):
    """__shfl_down sum over 64 lanes (last axis): lane 0 of v += down(v, o), o = 32, ..., 1 (lanes past the end keep their own)"""
    o = 32
    while o > 0:
        sh = np.concatenate([lanes[..., o:], lanes[..., 64 - o:]], -1)
        lanes = lanes + sh
        o >>= 1
    return lanes[..., 0]


def _fn32(fn, x):
    """logf / expf / log1pf as one rounding of the fp64 function: the same bits on every machine (numpy's own fp32 routines differ
    between its SIMD builds), and as valid an fp32 evaluation as the device's"""
    with np.errstate(all="ignore"):
        return fn(np.asarray(x, np.float64)).astype(f32)


def _block_sum(terms):
    """block_sum_f of csrc/mogan_elem.hip over a 1-D fp32 array: thread k sums k, k + 256, ... in order, each wave by shuffles,
    then sh[0] + sh[1] + sh[2] + sh[3]"""
    n = terms.shape[0]
    acc = np.zeros(256, f32)
    for i0 in range(0, n, 256):
        k = min(256, n - i0)
        acc[:k] = acc[:k] + terms[i0:i0 + k]
    w = _shfl_down_sum(acc.reshape(4, 64))
    return ((w[0] + w[1]) + w[2]) + w[3]


# ================================================================================================================ logits head
HEAD_ROWS = [(1, 4, 1), (15, 32, 1), (5, 1028, 3), (16, 12288, 1), (3, 72, 4)]
HEAD_SATURATED = (15, 32, 1)          # images 0 and 1 of this row have z = +110 and -110: p is exactly 1 and exactly 0


@functools.lru_cache(maxsize=None)
def head_case(B, K, Cout, with_bias=True):
    tag = "%s" % ((B, K, Cout),)
    x, w = T("hdx" + tag, (B, K)), T("hdw" + tag, (Cout, K), 1.0 / math.sqrt(K))
    bias = T("hdb" + tag, (Cout,), 0.1) if with_bias else None
    if (B, K, Cout) == HEAD_SATURATED:
        u = w[0] / float(w[0].double().pow(2).sum())
        x[0], x[1] = 110.0 * u, -110.0 * u
    dp = T("hdg" + tag, (B, Cout))
    base_w, base_b = T("hdbw" + tag, (Cout, K)), T("hdbb" + tag, (Cout,))
    xd, wd = x.double(), w.double()
    z = xd @ wd.t() + (bias.double() if with_bias else 0.0)
    S_z = xd.abs() @ wd.abs().t() + (bias.double().abs() if with_bias else 0.0)
    p = _sig(z)
    q = _sig(-z)                                                 # 1 - p without the cancellation
    ref, S = {"p": p}, {"p": p * q * (S_z + 2 + z.abs()) + 2 * p}
    # backward from dp and the fp32 p the kernel receives: dz = dp p (1 - p), three roundings
    pin = p.float()
    pq = pin.double()
    dz = dp.double() * pq * (1 - pq)
    ref["dx"], S["dx"] = dz @ wd, (3 + Cout) * (dz.abs() @ wd.abs())
    ref["dw"], S["dw"] = dz.t() @ xd, (3 + B) * (dz.abs().t() @ xd.abs())
    ref["db"], S["db"] = dz.sum(0), (3 + B) * dz.abs().sum(0)
    for k, base in (("dw", base_w), ("db", base_b)):             # accumulate = 1: one more addition
        ref[k + "+"] = ref[k] + base.double()
        S[k + "+"] = S[k] + ref[k].abs() + ref[k + "+"].abs()
    return dict(x=x, w=w, bias=bias, dp=dp, p_in=pin, base_w=base_w, base_b=base_b, z=z, ref=ref, S=S)


def restate_head_fp32(x, w, bias, dp, p_in, base_w, base_b):
    """logits_head_fwd_kernel / _bwd_kernel in numpy fp32, chains and order kept (one rounding per multiply and per add)"""
    B, K = x.shape
    Cout = w.shape[0]
    p = np.zeros((B, Cout), f32)
    for co in range(Cout):
        prod = (x * w[co][None]).reshape(B, K // 4, 4)           # (B, float4 index, component)
        acc = np.zeros((B, 256, 4), f32)
        for k0 in range(0, K // 4, 256):
            k = min(256, K // 4 - k0)
            acc[:, :k] = acc[:, :k] + prod[:, k0:k0 + k]
        a = (acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3])
        part = _shfl_down_sum(a.reshape(B, 4, 64))
        z = (part[:, 0] + part[:, 1]) + (part[:, 2] + part[:, 3]) + (bias[co] if bias is not None else f32(0))
        with np.errstate(all="ignore"):
            p[:, co] = f32(1) / (f32(1) + _exp32(-z))
    dz = dp * p_in * (f32(1) - p_in)
    dx = np.zeros((B, K), f32)
    for co in range(Cout):
        dx = dz[:, co, None] * w[co][None] + dx
    dw, db = np.zeros((Cout, K), f32), np.zeros(Cout, f32)
    for b in range(B):
        dw = dz[b][:, None] * x[b][None] + dw
        db = db + dz[b]
    out = {"p": p, "dx": dx, "dw": dw, "db": db, "dw+": base_w + dw, "db+": base_b + db}
    assert all(v.dtype == f32 for v in out.values())
    return out


# ========================================================================================================= elementwise losses
ELEM_N = (1, 63, 64, 65, 255, 256, 257, 1600, 4099)
TARGETS = (0.0, 1.0, 0.3)
WEIGHTS = (1.0, 0.5)
GOUT = 1.7
BASE = 0.8125                       # what the accumulating forward adds onto (of the losses' sign: no cancellation)
BCE_SPECIAL = (0.0, 1.0, 1e-13, 1.0 - 6e-8, 3e-20)
BCEL_SPECIAL = (0.0, 1e-4, -1e-4, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0)
LV_SPECIAL = (0.0, -0.0, 10.0, -10.0)


def _with_special(t, special, at=0):
    k = max(0, min(len(special), t.numel() - at))
    t[at:at + k] = torch.tensor(special[:k], dtype=torch.float32)
    return t


@functools.lru_cache(maxsize=None)
def elem_inputs(n):
    p = _with_special(torch.sigmoid(T("elp%d" % n, (n,), 2.0)), BCE_SPECIAL)
    x = _with_special(T("elx%d" % n, (n,), 3.0), BCEL_SPECIAL)
    mu = T("elm%d" % n, (n,), 0.5)
    # (from element 1 on: alone at n = 1, lv = 0 makes the KL scalar the cancellation 1 - mu^2 - 1, of which no fp32 evaluation
    # has the whole-tensor figure; in company the sum is larger than what the term loses)
    lv = _with_special(T("ell%d" % n, (n,), 4.0).clamp(-10, 10), LV_SPECIAL, at=1)
    eps, dc = T("ele%d" % n, (n,)), T("eld%d" % n, (n,))
    return dict(p=p, x=x, mu=mu, lv=lv, eps=eps, dc=dc)


def _mean_loss(term, S_term, weight, n, accumulate):
    """loss = (base +) weight * sum / n with S: the terms' own losses, the block sum's chain, the two scalings, the addition"""
    s, a = term.sum(), term.abs().sum()
    val = weight * s / n
    S = abs(weight) / n * (S_term.sum() + _chain(n) * a) + 2 * val.abs()
    if accumulate:
        S = S + val.abs() + (val + BASE).abs()
        val = val + BASE
    return val.reshape(1), S.reshape(1)


@functools.lru_cache(maxsize=None)
def bce_case(n, target, weight, accumulate):
    """mogan_bce_fwd / _bwd: -(t max(log p, -100) + (1 - t) max(log(1 - p), -100)); backward (p - t) / max(p (1 - p), 1e-12).
    t is the fp32 value the entry receives.  S: a log loses one rounding of its size and one of its argument's ((1 - p) rounds:
    an absolute 1); the two products and the sum round; the backward is a chain of eight roundings of its own size"""
    p = elem_inputs(n)["p"].double()
    t = float(f32(target))
    lp, l1p = torch.log(p).clamp_min(-100), torch.log1p(-p).clamp_min(-100)
    term = -(t * lp + (1 - t) * l1p)
    S_term = abs(t) * (lp.abs() + 1) + abs(1 - t) * (l1p.abs() + 1) + 2 * ((t * lp).abs() + ((1 - t) * l1p).abs())
    loss, S_loss = _mean_loss(term, S_term, weight, n, accumulate)
    dp = GOUT * weight * ((p - t) / ((1 - p) * p).clamp_min(float(f32(1e-12)))) / n
    return dict(ref={"bce": loss, "bce_dp": dp}, S={"bce": S_loss, "bce_dp": 8 * dp.abs()})


@functools.lru_cache(maxsize=None)
def bcel_case(n, target, weight, accumulate):
    """mogan_bce_logits_fwd / _bwd: max(x, 0) - x t + log1p(exp(-|x|)); backward sigmoid(x) - t.  S: e = exp(-|x|) carries 2 + |x|
    roundings, d log1p(e) = e / (1 + e); the three terms and their two sums round"""
    x = elem_inputs(n)["x"].double()
    t = float(f32(target))
    e = torch.exp(-x.abs())
    l = torch.log1p(e)
    term = x.clamp_min(0) - x * t + l
    S_term = (x * t).abs() + e / (1 + e) * (2 + x.abs()) + l + 2 * (x.clamp_min(0) + (x * t).abs() + l)
    loss, S_loss = _mean_loss(term, S_term, weight, n, accumulate)
    sg = _sig(x)
    k = abs(GOUT * weight / n)
    dx = GOUT * weight * (sg - t) / n
    S_dx = k * (sg * _sig(-x) * (2 + x.abs()) + 2 * sg + (sg - t).abs()) + 3 * dx.abs()
    return dict(ref={"bcel": loss, "bcel_dx": dx}, S={"bcel": S_loss, "bcel_dx": S_dx})


@functools.lru_cache(maxsize=None)
def kl_case(n):
    """mogan_kl_fwd / _bwd and mogan_reparam_fwd / _bwd.  E = exp(lv) carries 2 + |lv| roundings (__expf), exp(lv / 2) one more
    for the product with 0.5 (exact, counted all the same)"""
    d = elem_inputs(n)
    mu, lv, eps, dc = (d[k].double() for k in ("mu", "lv", "eps", "dc"))
    E = torch.exp(lv)
    term = 1 + lv - mu * mu - E
    S_term = E * (2 + lv.abs()) + mu * mu + 3 * (1 + lv.abs() + mu * mu + E)
    s, a = term.sum(), term.abs().sum()
    kl = (-0.5 * s / n).reshape(1)
    S_kl = (0.5 / n * (S_term.sum() + _chain(n) * a) + 2 * kl.abs()).reshape(1)
    g = GOUT * -0.5 / n
    dmu, dlv = g * (-2 * mu), g * (1 - E)
    H = torch.exp(0.5 * lv)
    c = eps * H + mu
    rdlv = dc * eps * 0.5 * H
    ref = {"kl": kl, "kl_dmu": dmu, "kl_dlv": dlv, "c": c, "rp_dlv": rdlv}
    S = {"kl": S_kl, "kl_dmu": 3 * dmu.abs(), "kl_dlv": abs(g) * (E * (2 + lv.abs()) + (1 - E).abs()) + 2 * dlv.abs(),
         "c": (eps * H).abs() * (3 + 0.5 * lv.abs()) + c.abs(), "rp_dlv": rdlv.abs() * (5 + 0.5 * lv.abs())}
    return dict(ref=ref, S=S)


def restate_elem_fp32(n, target, weight, accumulate):
    """the elementwise kernels in numpy fp32, operation order kept, one rounding per operation (logf / expf / log1pf: _fn32)"""
    d = {k: v.numpy() for k, v in elem_inputs(n).items()}
    t, w, one, nn = f32(target), f32(weight), f32(1), f32(n)
    g, base = f32(GOUT), f32(BASE)
    fin = lambda s: (base if accumulate else f32(0)) + w * s / nn
    out = {}
    with np.errstate(all="ignore"):
        p = d["p"]
        lp, l1p = np.maximum(_fn32(np.log, p), f32(-100)), np.maximum(_fn32(np.log, one - p), f32(-100))
        out["bce"] = np.array([fin(-_block_sum(t * lp + (one - t) * l1p))], f32)         # (s -= term: the negated sum, exactly)
        out["bce_dp"] = g * w * ((p - t) / np.maximum((one - p) * p, f32(1e-12))) / nn
        x = d["x"]
        out["bcel"] = np.array([fin(_block_sum(np.maximum(x, f32(0)) - x * t + _fn32(np.log1p, _fn32(np.exp, -np.abs(x)))))], f32)
        out["bcel_dx"] = g * w * (one / (one + _fn32(np.exp, -x)) - t) / nn
        mu, lv, eps, dc = d["mu"], d["lv"], d["eps"], d["dc"]
        out["kl"] = np.array([f32(-0.5) * _block_sum(one + lv - mu * mu - _exp32(lv)) / nn], f32)
        gk = g * f32(-0.5) / nn
        out["kl_dmu"], out["kl_dlv"] = gk * (f32(-2) * mu), gk * (one - _exp32(lv))
        H = _exp32(f32(0.5) * lv)
        out["c"], out["rp_dlv"] = eps * H + mu, dc * eps * f32(0.5) * H
    assert all(v.dtype == f32 for v in out.values())
    return out


# ====================================================================================================================== words
LENS_KINDS = ("full", "ragged", "zero", "over")
WORDS_ROWS = [(2, 2, 10, 9, T_, "ragged") for T_ in (1, 8, 9, 12, 13, 16, 17, 24, 25, 32)]
WORDS_ROWS += [(2, 2, C, 36, 5, "full") for C in (1, 7, 8, 15, 16, 23)]
WORDS_ROWS += [(2, 2, 10, S_, 5, "full") for S_ in (1, 63, 64, 65, 289, 320, 321, 640)]
WORDS_ROWS += [(3, 5, 10, 36, 7, "ragged"), (5, 2, 10, 36, 7, "ragged")]
WORDS_LDS_EDGE = (1, 2, 188, 289, 32, "full")
WORDS_ROWS += [WORDS_LDS_EDGE]
WORDS_ROWS += [(2, 3, 10, 36, 7, k) for k in LENS_KINDS]
WORDS_ROWS += [(2, 2, 256, 289, 12, "ragged")]
CHAIN_ROW = (5, 5, 32, 36, 7)         # B = Bc, C, S, T of the row that runs words -> ce -> words backward with the bmm pair


def words_tt(T_):
    """the instantiation that takes T words"""
    return next(tt for tt in (8, 12, 16, 24, 32) if T_ <= tt)


def words_channel_loop(C):
    """which shapes of the channel loop a C reaches: nothing but the one-by-one tail (C < 8), eights followed by a tail (C % 8),
    eights without a second prefetch (8 <= C < 16), eights with one (C >= 16)"""
    tags = set()
    if C < 8:
        tags.add("C < 8")
    if C >= 8 and C % 8:
        tags.add("eights and tail")
    if 8 <= C < 16:
        tags.add("no second prefetch")
    if C >= 16:
        tags.add("second prefetch")
    return tags


def words_s_regime(S_):
    """(forward, backward): the weighted context in registers or in the loop; one region per thread or two"""
    return ("registers" if S_ <= 320 else "loop", "one region" if S_ <= 320 else "two regions")


def words_rel_applies(C):
    """whether the whole-tensor figures REL["dwc"] / REL["dscore_t"] can be asked of a backward call.  With one channel every
    cosine is +1 or -1 whatever the context is: the gradient through it is identically zero, dwc = k1 w + k2 wc is the difference
    of two equal products and what any fp32 evaluation returns is their rounding -- the numpy restatement has 5e+8 relative to
    the fp64 value (tests/test_loss_reference_cpu.py asserts it: the exemption is needed, not convenient).  The C = 1 call is
    held to the per-element bound, which knows the size of the two products, and to the memory contract"""
    return C > 1


def words_lds_bytes(C, S_, T_):
    return (C * T_ + T_ * (S_ + 1) + 1088) * 4


def words_lens(Bc, T_, kind):
    """int32 (Bc): full; ragged -- descending from T to one caption of length 1; zero -- the same with a last caption of length 0;
    over -- T + 3 and -2 (they clamp to T and 0), the others T - 1"""
    if kind == "full":
        l = [T_] * Bc
    elif kind in ("ragged", "zero"):
        l = [max(1, int(round(T_ - (T_ - 1) * i / max(1, Bc - 1)))) for i in range(Bc)]
        l[-1] = 1 if kind == "ragged" else 0
    else:
        l = [T_ + 3, -2] + [max(1, T_ - 1)] * (Bc - 2)
    return torch.tensor(l, dtype=torch.int32)


def lens_clamps(lens, T_):
    l = lens.numpy()
    return {"zero": bool((l == 0).any()), "above": bool((l > T_).any()), "negative": bool((l < 0).any()),
            "one": bool((l == 1).any()), "ragged": bool(((l > 0) & (l < T_)).any())}


def words_forward(ctx, words, lens, gammas=GAMMAS, dtype=F64):
    """the words similarity of miscc/losses.py:62-132 + GlobalAttention.py:31-69 for all pairs, in torch at `dtype`:
    ctx (B, C, S), words (Bc, C, T), lens (Bc) -> dict of sim (B, Bc), a1 (B, Bc, S, T), a2 (B, Bc, T, S), wc (B, C, Bc, T), wt
    (C, Bc, T) and the intermediates the scales need.  Only the valid words enter; a caption of length 0 has sim = -inf"""
    g1, g2, g3 = gammas
    B, C, S_ = ctx.shape
    Bc, _, T_ = words.shape
    n = lens.long().clamp(0, T_)
    valid = torch.arange(T_)[None] < n[:, None]                                          # (Bc, T)
    w = torch.where(valid[:, None, :], words, torch.zeros((), dtype=words.dtype)).to(dtype)
    x = ctx.to(dtype)
    score = torch.einsum("bcs,ict->bist", x, w)
    off = ~valid[None, :, None, :].expand(B, Bc, S_, T_)
    sm = score.masked_fill(off, -float("inf"))
    m1 = sm.max(3, keepdim=True).values
    m1 = torch.where(torch.isfinite(m1), m1, torch.zeros_like(m1))
    arg1 = (sm - m1).masked_fill(off, 0.0)
    e1 = torch.where(off, torch.zeros_like(score), torch.exp(arg1))
    tiny = torch.finfo(dtype).tiny                                                       # (an empty caption: 0 / tiny = 0)
    a1 = e1 / e1.sum(3, keepdim=True).clamp_min(tiny)
    a1t = a1.transpose(2, 3)                                                             # (B, Bc, T, S)
    arg2 = g1 * a1t - (g1 * a1t).max(3, keepdim=True).values
    offt = off.transpose(2, 3)
    e2 = torch.where(offt, torch.zeros_like(arg2), torch.exp(arg2))
    a2 = e2 / e2.sum(3, keepdim=True).clamp_min(tiny)
    wc = torch.einsum("bcs,bits->bcit", x, a2)
    wi = w.permute(1, 0, 2)[None]                                                        # (1, C, Bc, T)
    d, a, w2 = (wc * wi).sum(1), (wc * wc).sum(1), (wi * wi).sum(1).expand(B, Bc, T_)
    den = (a.sqrt() * w2.sqrt()).clamp_min(float(f32(1e-8)))
    cos = d / den
    e = torch.where(valid[None], torch.exp(g2 * cos), torch.zeros_like(cos))
    Z = e.sum(2)
    sim = g3 * torch.log(Z)
    return dict(sim=sim, a1=a1, a2=a2, wc=wc, wt=w.permute(1, 0, 2).contiguous(), score=score, arg1=arg1, arg2=arg2, d=d, a=a, w2=w2,
                den=den, cos=cos, e=e, Z=Z, valid=valid, w=w, off=off)


def words_reference(ctx, words, lens, dsim, gammas=GAMMAS):
    """fp64 reference and S of mogan_damsm_words_fwd and, from the rounded a1 / a2 / wc the backward receives, of _bwd"""
    g1, g2, g3 = gammas
    B, C, S_ = ctx.shape
    Bc, _, T_ = words.shape
    r = words_forward(ctx, words, lens, gammas)
    x, w, valid, off = ctx.double(), r["w"], r["valid"], r["off"]
    xa, wa = x.abs(), w.abs()
    Ti = valid.sum(1).double()[None, :, None, None]
    # a1: the attention model of pathway_cases over the valid words
    S_sc = torch.einsum("bcs,ict->bist", xa, wa)
    A1 = torch.where(off, torch.zeros_like(S_sc), S_sc + 2 + 2 * r["arg1"].abs())
    a1 = r["a1"]
    S_a1 = a1 * (A1 + (a1 * A1).sum(3, keepdim=True) + Ti + 2)
    # a2: softmax over the regions of gamma1 a1 -- the argument inherits gamma1 S_a1 and is formed as in pathway_cases' softmax
    a2 = r["a2"]
    a1t, S_a1t, offt = a1.transpose(2, 3), S_a1.transpose(2, 3), off.transpose(2, 3)
    m2 = (g1 * a1t).max(3, keepdim=True).values
    A2 = torch.where(offt, torch.zeros_like(a2), g1 * S_a1t + (g1 * a1t).abs() + m2.abs() + 2 + r["arg2"].abs())
    S_a2 = a2 * (A2 + (a2 * A2).sum(3, keepdim=True) + (S_ + 63) // 64 + 6 + 2)
    S_wc = torch.einsum("bcs,bits->bcit", xa, S_a2 + a2)
    wc = r["wc"]
    wi, wia = w.permute(1, 0, 2)[None], wa.permute(1, 0, 2)[None]
    # the cosine: d = <wc, w>, a = |wc|^2, w2 = |w|^2; den = sqrt(a) sqrt(w2) loses half of a's and of w2's loss and rounds 3 times
    S_d = (S_wc * wia + (wc * wi).abs()).sum(1)
    S_aa = (2 * wc.abs() * S_wc + wc * wc).sum(1)
    a, den, cos, e, Z = r["a"], r["den"], r["cos"], r["e"], r["Z"]
    live = valid[None].expand(B, Bc, T_)
    safe = lambda t: torch.where(live, t, torch.ones_like(t))
    rel_den = 0.5 * S_aa / safe(a) + 3.5
    S_cos = torch.where(live, S_d / den + cos.abs() * (rel_den + 1), torch.zeros_like(cos))
    E = g2 * S_cos + 2 + 2 * (g2 * cos).abs()
    Zs = Z.clamp_min(1e-300)
    sim = r["sim"]
    S_sim = abs(g3) * ((e * E).sum(2) / Zs + 6 + torch.log(Zs).abs()) + torch.where(torch.isfinite(sim), sim.abs(), torch.zeros_like(sim))
    S_sim = torch.where(torch.isfinite(sim), S_sim, torch.zeros_like(S_sim))               # a -inf is compared as such
    ref = {k: r[k] for k in ("sim", "a1", "a2", "wc", "wt")}
    S = {"sim": S_sim, "a1": S_a1, "a2": S_a2, "wc": S_wc}
    # ---- backward, from fp32 inputs: the cosines again from wc_in and w, then dwc = k1 w + k2 wc and the two softmax backwards
    a1i, a2i, wci = a1.float().double(), a2.float().double(), wc.float().double()
    g = dsim.double()[:, :, None]
    d, aa = (wci * wi).sum(1), (wci * wci).sum(1)
    S_d2 = (wci * wi).abs().sum(1)
    w2 = r["w2"]
    den = (aa.sqrt() * w2.sqrt()).clamp_min(float(f32(1e-8)))
    assert bool((den[live] > 1e-6).all()), "a cosine of the table sits on the 1e-8 clamp"
    cos = d / den
    S_cos = torch.where(live, S_d2 / den + 5 * cos.abs(), torch.zeros_like(cos))
    e = torch.where(live, torch.exp(g2 * cos), torch.zeros_like(cos))
    E = g2 * S_cos + 2 + 2 * (g2 * cos).abs()
    z = e.sum(2, keepdim=True).clamp_min(1e-300)
    dcos = g * g3 * g2 * e / z
    S_dcos = dcos.abs() * (E + (e * E).sum(2, keepdim=True) / z + 5 + 4)
    k1 = dcos / den
    S_k1 = S_dcos / den + 5 * k1.abs()
    k2 = -dcos * cos / safe(aa)
    S_k2 = (S_dcos * cos.abs() + dcos.abs() * S_cos) / safe(aa) + 3 * k2.abs()
    dwc = k1[:, None] * wi + k2[:, None] * wci                                           # (B, C, Bc, T)
    S_dwc = S_k1[:, None] * wia + S_k2[:, None] * wci.abs() + 2 * ((k1[:, None] * wi).abs() + (k2[:, None] * wci).abs())
    da = torch.einsum("bcit,bcs->bits", dwc, x)
    S_da = torch.einsum("bcit,bcs->bits", S_dwc + dwc.abs(), xa)
    rd = (a2i * da).sum(3, keepdim=True)
    S_rd = (a2i * (S_da + 2 * da.abs())).sum(3, keepdim=True)
    da1 = g1 * a2i * (da - rd)                                                           # (B, Bc, T, S)
    S_da1 = abs(g1) * a2i * (S_da + S_rd + da.abs() + rd.abs()) + 2 * da1.abs()
    a1it = a1i.transpose(2, 3)
    inner = (a1it * da1).sum(2, keepdim=True)
    S_in = (a1it * (S_da1 + 2 * da1.abs())).sum(2, keepdim=True)
    ds = a1it * (da1 - inner)
    ref["dwc"], S["dwc"] = dwc, S_dwc
    ref["dscore_t"], S["dscore_t"] = ds, a1it * (S_da1 + S_in + da1.abs() + inner.abs()) + ds.abs()
    return ref, S


def words_inputs(B, Bc, C, S_, T_, kind):
    tag = "%s" % ((B, Bc, C, S_, T_),)
    ctx, words = T("wdx" + tag, (B, C, S_)), T("wdw" + tag, (Bc, C, T_), 0.3)
    lens = words_lens(Bc, T_, kind)
    valid = torch.arange(T_)[None] < lens.long().clamp(0, T_)[:, None]
    words = torch.where(valid[:, None, :], words, torch.full((), float("nan")))          # the padded slots hold NaN
    return ctx, words, lens, T("wdg" + tag, (B, Bc))


@functools.lru_cache(maxsize=None)
def words_case(B, Bc, C, S_, T_, kind):
    ctx, words, lens, dsim = words_inputs(B, Bc, C, S_, T_, kind)
    ref, S = words_reference(ctx, words, lens, dsim)
    sav = {k: ref[k].float() for k in ("a1", "a2", "wc")}
    return dict(ctx=ctx, words=words, lens=lens, dsim=dsim, saved=sav, ref=ref, S=S)


def restate_words_fp32(ctx, words, lens, dsim, a1_in, a2_in, wc_in, gammas=GAMMAS):
    """damsm_words_fwd_kernel / damsm_words_bwd_kernel in numpy fp32: the channel, word, lane and wave sums in the kernels' order,
    one rounding per multiply and per add (the kernels' fmaf rounds once: an equally valid evaluation).  numpy fp32 arrays as the
    entry takes them (padded word slots zeroed: the kernels read none of them into a result)"""
    g1, g2, g3 = (f32(v) for v in gammas)
    B, C, S_ = ctx.shape
    Bc, _, T_ = words.shape
    n = np.clip(lens.astype(np.int64), 0, T_)
    valid = np.arange(T_)[None] < n[:, None]                                             # (Bc, T)
    w = np.where(valid[:, None, :], words, f32(0)).astype(f32)
    one, zero = f32(1), f32(0)
    NW = 5
    with np.errstate(all="ignore"):
        acc = np.zeros((B, Bc, S_, T_), f32)
        for c in range(C):
            acc = ctx[:, None, c, :, None] * w[None, :, c, None, :] + acc
        vt = valid[None, :, None, :]
        m = np.where(vt, acc, f32(-np.inf)).max(3, keepdims=True)
        e = np.where(vt, _exp32(acc - m), zero)
        z = np.zeros((B, Bc, S_, 1), f32)
        for t in range(T_):
            z = z + e[..., t:t + 1]
        a1 = np.where(vt, e * (one / z), zero).astype(f32)
        # softmax over the regions: lanes along s
        K = (S_ + 63) // 64
        row = a1.transpose(0, 1, 3, 2)                                                   # (B, Bc, T, S)
        vr = valid[None, :, :, None]
        rg = row * g1
        m2 = rg.max(3, keepdims=True)
        e2 = np.where(vr, _exp32(rg - m2), zero)
        pad = np.zeros((B, Bc, T_, K * 64), f32)
        pad[..., :S_] = e2
        lanes = np.zeros((B, Bc, T_, 64), f32)
        for k in range(K):
            lanes = lanes + pad[..., 64 * k:64 * k + 64]
        z2 = _butterfly(lanes)[..., None]
        a2 = np.where(vr, e2 * (one / z2), zero).astype(f32)
        # weighted context: lanes along s, then the butterfly; the per-word sums by wave (channels w, w + 5, ...), then over waves
        a2p = np.zeros((B, Bc, T_, K * 64), f32)
        a2p[..., :S_] = a2
        xp = np.zeros((B, C, K * 64), f32)
        xp[..., :S_] = ctx
        wc = np.zeros((B, C, Bc, T_), f32)
        for c in range(C):
            pl = np.zeros((B, Bc, T_, 64), f32)
            for k in range(K):
                pl = xp[:, None, None, c, 64 * k:64 * k + 64] * a2p[..., 64 * k:64 * k + 64] + pl
            wc[:, c] = np.where(valid[None], _butterfly(pl), zero)
        red = np.zeros((3, NW, B, Bc, T_), f32)
        for c in range(C):
            v, wv = wc[:, c], w[None, :, c, :]
            q = c % NW
            red[0, q] = v * wv + red[0, q]; red[1, q] = v * v + red[1, q]; red[2, q] = wv * wv + red[2, q]
        tot = np.zeros((3, B, Bc, T_), f32)
        for q in range(NW):
            tot = tot + red[:, q]
        cosv = tot[0] / np.maximum(np.sqrt(tot[1]) * np.sqrt(tot[2]), f32(1e-8))
        ee = np.where(valid[None], _exp32(g2 * cosv), zero)
        l64 = np.zeros((B, Bc, 64), f32)
        l64[..., :T_] = ee
        sim = (_fn32(np.log, _butterfly(l64)) * g3).astype(f32)
        # ---- backward from the saved fp32 tensors
        NP = 10
        red = np.zeros((3, NP, B, Bc, T_), f32)
        for c in range(C):
            v, wv = wc_in[:, c], w[None, :, c, :]
            q = c % NP
            red[0, q] = v * wv + red[0, q]; red[1, q] = v * v + red[1, q]; red[2, q] = wv * wv + red[2, q]
        tot = np.zeros((3, B, Bc, T_), f32)
        for q in range(NP):
            tot = tot + red[:, q]
        d, a, w2 = tot
        den = np.sqrt(a) * np.sqrt(w2)
        clamped = den < f32(1e-8)
        cosv = d / np.maximum(den, f32(1e-8))
        ee = np.where(valid[None], _exp32(g2 * cosv), zero)
        l32 = np.zeros((B, Bc, 32), f32)
        l32[..., :T_] = ee
        zz = _butterfly(l32, 32)[..., None]
        g = dsim[:, :, None]
        dcos = np.where(valid[None], g * g3 * g2 * ee / zz, zero)
        k1 = dcos / np.maximum(den, f32(1e-8))
        k2 = np.where(clamped | (a <= 0), zero, -dcos * cosv / a)
        wi = w.transpose(1, 0, 2)[None]                                                  # (1, C, Bc, T)
        dwc = np.where(valid[None, None], k1[:, None] * wi + k2[:, None] * wc_in, zero).astype(f32)
        da = np.zeros((B, Bc, T_, S_), f32)
        for c in range(C):
            da = ctx[:, None, None, c, :] * dwc[:, c, :, :, None] + da
        prod = np.zeros((B, Bc, T_, K * 64), f32)
        prod[..., :S_] = np.where(vr, a2_in * da, zero)
        lanes = np.zeros((B, Bc, T_, 64), f32)
        for k in range(K):
            lanes = lanes + prod[..., 64 * k:64 * k + 64]
        rd = _butterfly(lanes)[..., None]
        da1 = np.where(vr, g1 * a2_in * (da - rd), zero)                                 # (B, Bc, T, S)
        a1t = a1_in.transpose(0, 1, 3, 2)
        inner = np.zeros((B, Bc, 1, S_), f32)
        for t in range(T_):
            inner = a1t[:, :, t:t + 1] * da1[:, :, t:t + 1] + inner
        ds = np.where(vr, a1t * (da1 - inner), zero).astype(f32)
    out = {"sim": sim, "a1": a1, "a2": a2, "wc": wc, "dwc": dwc, "dscore_t": ds}
    assert all(v.dtype == f32 for v in out.values())
    return out


# ============================================================================================================ cross-entropies
CE_R = (1, 2, 5, 63, 64, 65, 256, 257)
CE_ROWS = [(R, mk, lk) for R in CE_R for mk in (None, "same") for lk in ("arange", "perm")] + [(5, mk, "clamp") for mk in (None, "same")]
CE_G = ((1.3, 0.7), (1.3, None), (None, 0.7), (None, None))            # g0, g1 of the backward: both, each NULL in turn, both NULL


def ce_labels(R, kind):
    """int64 (R): arange; a permutation; arange with one label equal to R and one -1 (they clamp to R - 1 and 0)"""
    lab = torch.arange(R, dtype=torch.int64)
    if kind == "perm":
        lab = torch.from_numpy(np.random.RandomState(R).permutation(R).astype(np.int64))
    if kind == "clamp":
        lab[1], lab[3] = R, -1
    return lab


def ce_mask(R, lab):
    """uint8 (R, R): pairs of a class off the diagonal, never a row's or a column's own label (classes of two, r // 2; below
    R = 8 two classes, r % 2, so that pairs are left once the labels are cleared)"""
    c = torch.arange(R) // 2 if R >= 8 else torch.arange(R) % 2
    m = (c[:, None] == c[None, :]) & ~torch.eye(R, dtype=torch.bool)
    l = lab.clamp(0, R - 1)
    m[torch.arange(R), l] = False
    m[l, torch.arange(R)] = False
    return m.to(torch.uint8)


def _ce_axis(s, off, lab, dim):
    """softmax and NLL along `dim` of the masked scores; entry [k] of the NLL is row k (dim 1) or column k (dim 0)"""
    R = s.shape[0]
    sm = s.masked_fill(off, -float("inf"))
    m = sm.max(dim, keepdim=True).values
    arg = (sm - m).masked_fill(off, 0.0)
    e = torch.where(off, torch.zeros_like(s), torch.exp(arg))
    z = e.sum(dim, keepdim=True)
    p = e / z
    A = torch.where(off, torch.zeros_like(s), 2 + 2 * arg.abs())
    pA = (p * A).sum(dim, keepdim=True)
    S_p = p * (A + pA + _chain(R) + 2)
    idx = lab.clamp(0, R - 1)
    ar = torch.arange(R)
    al = arg[ar, idx] if dim == 1 else arg[idx, ar]
    lz = torch.log(z).reshape(R)
    nll = -(al - lz)
    S_nll = 2 * al.abs() + pA.reshape(R) + _chain(R) + lz.abs() + nll.abs()
    return p, S_p, nll, S_nll


def ce_reference(sim, lab, mask, prow_in=None, pcol_in=None):
    """fp64 reference and S of mogan_damsm_ce_fwd (prow, pcol, nll (2R), out2) and, from the fp32 prow / pcol it receives, of _bwd
    for every (g0, g1) of CE_G.  Masked entries of sim (NaN in the tables) are not read"""
    R = sim.shape[0]
    off = torch.zeros(R, R, dtype=torch.bool) if mask is None else mask.bool()
    s = torch.where(off, torch.zeros((), dtype=F64), sim.double())
    prow, S_prow, nr, S_nr = _ce_axis(s, off, lab, 1)
    pcol, S_pcol, nc, S_nc = _ce_axis(s, off, lab, 0)
    nll, S_nll = torch.cat([nr, nc]), torch.cat([S_nr, S_nc])
    out2 = torch.stack([nr.mean(), nc.mean()])
    S_out = torch.stack([S_nr.mean() + (_chain(R) + 2) * nr.abs().mean(), S_nc.mean() + (_chain(R) + 2) * nc.abs().mean()])
    ref = {"prow": prow, "pcol": pcol, "nll": nll, "out2": out2}
    S = {"prow": S_prow, "pcol": S_pcol, "nll": S_nll, "out2": S_out}
    pr = prow if isinstance(prow_in, str) else (prow.float() if prow_in is None else prow_in).double()          # ("exact": the exact ones)
    pc = pcol if isinstance(pcol_in, str) else (pcol.float() if pcol_in is None else pcol_in).double()
    idx = lab.clamp(0, R - 1)
    hot_r = torch.zeros(R, R, dtype=F64)
    hot_r[torch.arange(R), idx] = 1
    hot_c = torch.zeros(R, R, dtype=F64)
    hot_c[idx, torch.arange(R)] = 1
    for g0, g1 in CE_G:
        a = (g0 or 0.0) * (pr - hot_r) / R
        b = (g1 or 0.0) * (pc - hot_c) / R
        ref[("dsim", g0, g1)], S[("dsim", g0, g1)] = a + b, 3 * a.abs() + 3 * b.abs() + (a + b).abs()
    return ref, S


@functools.lru_cache(maxsize=None)
def ce_case(R, mask_kind, label_kind):
    lab = ce_labels(R, label_kind)
    mask = None if mask_kind is None else ce_mask(R, lab)
    sim = T("cesim%d" % R, (R, R), 3.0)
    if mask is not None:
        sim = torch.where(mask.bool(), torch.full((), float("nan")), sim)
    ref, S = ce_reference(sim, lab, mask)
    return dict(sim=sim, lab=lab, mask=mask, prow_in=ref["prow"].float(), pcol_in=ref["pcol"].float(), ref=ref, S=S)


def restate_ce_fp32(sim, lab, mask, prow_in, pcol_in):
    """damsm_ce_fwd_kernel / _finish_kernel / _bwd_kernel in numpy fp32, order kept"""
    R = sim.shape[0]
    off = np.zeros((R, R), bool) if mask is None else mask.astype(bool)
    idx = np.clip(lab, 0, R - 1)
    one, zero = f32(1), f32(0)
    out = {}
    nll = []
    with np.errstate(all="ignore"):
        for name, s, o in (("prow", sim, off), ("pcol", sim.T, off.T)):           # rows of s are the softmax axis
            sm = np.where(o, f32(-np.inf), np.where(o, zero, s))
            m = sm.max(1, keepdims=True)
            e = np.where(o, zero, _exp32(sm - m))
            z = np.array([_block_sum(e[r]) for r in range(R)], f32)[:, None]     # (wave_sum by xor here: the same pairs)
            p = e / z
            out[name] = p if name == "prow" else p.T.copy()
            lz = _fn32(np.log, z[:, 0])
            nll.append(-(sm[np.arange(R), idx] - m[:, 0] - lz))
        out["nll"] = np.concatenate(nll).astype(f32)
        out["out2"] = np.array([_block_sum(nll[0]) / f32(R), _block_sum(nll[1]) / f32(R)], f32)
        hot_r = np.zeros((R, R), f32); hot_r[np.arange(R), idx] = 1
        hot_c = np.zeros((R, R), f32); hot_c[idx, np.arange(R)] = 1
        for g0, g1 in CE_G:
            a = f32(g0) * (prow_in - hot_r) / f32(R) if g0 is not None else np.zeros((R, R), f32)
            b = f32(g1) * (pcol_in - hot_c) / f32(R) if g1 is not None else np.zeros((R, R), f32)
            out[("dsim", g0, g1)] = a + b
    assert all(v.dtype == f32 for v in out.values())
    return out


# ============================================================================================================= sentence loss
SENT_SHAPES = [(1, 1, 1), (3, 5, 10), (5, 3, 63), (2, 2, 64), (2, 2, 65), (4, 4, 256), (2, 9, 300)]
SENT_EPS = (1e-8, 0.5)
# (B, Bc, C, kind, eps): plain; tiny -- image 1 is 1e-10 of a plain one, |cnn_b| |rnn_i| < eps for both eps; zero -- image 0 is all zeros
SENT_ROWS = [s + ("plain", e) for s in SENT_SHAPES for e in SENT_EPS] + [(3, 5, 10, k, e) for k in ("tiny", "zero") for e in SENT_EPS]


def sent_reference(cnn, rnn, dsim, eps, g3=GAMMAS[2]):
    """sim[b, i] = g3 <cnn_b, rnn_i> / max(|cnn_b| |rnn_i|, eps) and dcnn.  S: the dot product sum |x||r| (factor to TOL); a norm
    loses 0.5 + 1, the product of two norms 4 in all; clamped, the denominator is the constant"""
    x, r, g = cnn.double(), rnn.double(), dsim.double() * g3
    ep = float(f32(eps))
    d, S_d = x @ r.t(), x.abs() @ r.abs().t()
    n0s = (x * x).sum(1, keepdim=True)
    n0, n1 = n0s.sqrt(), (r * r).sum(1, keepdim=True).sqrt().t()
    den0 = n0 * n1
    cl = den0 < ep
    den = den0.clamp_min(ep)
    rel = torch.where(cl, torch.zeros_like(den), torch.full_like(den, 4.0))
    sim = d / den * g3
    ref, S = {"ssim": sim}, {"ssim": g3 / den * S_d + sim.abs() * (rel + 2)}
    k1 = g / den
    S_k1 = k1.abs() * (rel + 2)
    ok = (~cl) & (n0s > 0)
    dn = torch.where(ok, den * n0s, torch.ones_like(den))
    k2 = torch.where(ok, -g * d / dn, torch.zeros_like(den))
    S_k2 = torch.where(ok, g.abs() * S_d / dn + 9 * k2.abs(), torch.zeros_like(den))
    self_ = k2.sum(1, keepdim=True)
    ref["dcnn"] = k1 @ r + self_ * x
    S["dcnn"] = S_k1 @ r.abs() + k1.abs() @ r.abs() + x.abs() * (S_k2.sum(1, keepdim=True) + k2.abs().sum(1, keepdim=True)) \
        + (self_ * x).abs() + ref["dcnn"].abs()
    ref["margin"] = float(((den0 - ep).abs() / ep).min())
    ref["clamped"] = cl
    return ref, S


@functools.lru_cache(maxsize=None)
def sent_case(B, Bc, C, kind, eps):
    tag = "%s" % ((B, Bc, C),)
    cnn, rnn, dsim = T("sncnn" + tag, (B, C)), T("snrnn" + tag, (Bc, C)), T("sng" + tag, (B, Bc))
    if kind == "tiny":
        cnn[1] = cnn[1] * 1e-10
    if kind == "zero":
        cnn[0] = 0.0
    ref, S = sent_reference(cnn, rnn, dsim, eps)
    return dict(cnn=cnn, rnn=rnn, dsim=dsim, ref=ref, S=S)


def restate_sent_fp32(cnn, rnn, dsim, eps, g3=GAMMAS[2]):
    """damsm_sent_fwd_kernel / _bwd_kernel in numpy fp32: lanes stride the channels by 64, then the butterfly; order kept"""
    B, C = cnn.shape
    Bc = rnn.shape[0]
    K = (C + 63) // 64
    g3, ep, zero = f32(g3), f32(eps), f32(0)

    def lanesum(v):                                                  # v (..., C) products -> the wave's sum
        pad = np.zeros(v.shape[:-1] + (K * 64,), f32)
        pad[..., :C] = v
        lanes = np.zeros(v.shape[:-1] + (64,), f32)
        for k in range(K):
            lanes = lanes + pad[..., 64 * k:64 * k + 64]
        return _butterfly(lanes)
    with np.errstate(all="ignore"):
        n0s = lanesum(cnn * cnn)[:, None]
        n0 = np.sqrt(n0s)
        d = lanesum(cnn[:, None, :] * rnn[None])
        n1 = np.sqrt(lanesum(rnn * rnn))[None]
        den = n0 * n1
        sim = d / np.maximum(den, ep) * g3
        g = dsim * g3
        cl = den < ep
        k1 = np.where(cl, g / ep, g / den)
        k2 = np.where(cl | ~(n0s > 0), zero, -g * d / (den * n0s)).astype(f32)
        acc, self_ = np.zeros((B, C), f32), np.zeros((B, 1), f32)
        for i in range(Bc):
            acc = k1[:, i:i + 1] * rnn[i][None] + acc
            self_ = self_ + k2[:, i:i + 1]
        dcnn = acc + self_ * cnn
    out = {"ssim": sim.astype(f32), "dcnn": dcnn.astype(f32)}
    assert all(v.dtype == f32 for v in out.values())
    return out


# ================================================================================================================ scalar sums
SUM_N = tuple(range(1, 9))
SUM_W = (1.3, 0.7, 2.0, 0.5, 0.0, -1.0, -0.25, 3.0)


@functools.lru_cache(maxsize=None)
def sum_case(n):
    v = T("sumv%d" % n, (n,), 2.0)
    w = torch.tensor(SUM_W[:n], dtype=torch.float32)
    terms = w.double() * v.double()
    return dict(v=v, w=w, ref=terms.sum().reshape(1), S=((n + 1) * terms.abs().sum()).reshape(1))


def restate_sum_fp32(v, w):
    s = f32(0)
    for k in range(len(v)):
        s = s + w[k] * v[k]
    return np.array([s], f32)


# ======================================================================================================================= adam
ADAM_N = (1, 3, 4, 5, 6, 1023, 1024, 1027, 10007)          # (6: the one tail of two elements)
ADAM_STEPS = (1, 2, 1000)
ADAM_HYPER = dict(lr=2e-4, beta1=0.5, beta2=0.999, eps=1e-8, ema_decay=0.999)
# (n, ema?, eps_mode, grad_scale, step): every (ema, eps_mode, grad_scale) at every n, the step through the argument in rotation
ADAM_ROWS = [(n, ema, em, gs, ADAM_STEPS[(i + 2 * ema + em + int(gs != 1.0)) % 3]) for i, n in enumerate(ADAM_N) for ema in (1, 0) for em in (0, 1)
             for gs in (1.0, 0.125)]
ADAM_ZERO_ROW = (5, 1, 0, 1.0, 1)          # with g = 0 and v = 0: denom = eps
ADAM_DEV_ROWS = [(n, ema, em, gs) for n in (5, 1027) for ema in (1, 0) for em, gs in ((0, 1.0), (1, 0.125))]


def adam_tail(n):
    """elements of the ragged last float4 (0: none)"""
    return n % 4


def _hyper(as_given):
    """the hyper-parameters as fp64: the fp32 values the entry receives, or (as_given) python's own -- what the oracle takes"""
    return {k: (float(v) if as_given else float(f32(v))) for k, v in ADAM_HYPER.items()}


def adam_corrections(step, eps_mode, as_given=False):
    """(step size, 1 / sqrt(1 - b2^t)) in fp64"""
    h = _hyper(as_given)
    lr, b1, b2 = h["lr"], h["beta1"], h["beta2"]
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    return (lr / bc1 if eps_mode == 0 else lr * math.sqrt(bc2) / bc1), 1.0 / math.sqrt(bc2)


@functools.lru_cache(maxsize=None)
def adam_inputs(n, zero=False):
    # |p| and |ema| below 4, the domain of the max-abs figure REL["adam_*"] (one rounding at 4 is a quarter of it already)
    p, g, m = T("adp%d" % n, (n,)).clamp(-3.5, 3.5), T("adg%d" % n, (n,), 0.01), T("adm%d" % n, (n,), 0.01)
    # v goes with m as in a run, |m| <= sqrt(v): the update stays a few lr and p' in p's binade
    v = m * m * (1 + T("adv%d" % n, (n,)).abs()) + 1e-10
    ema = T("ade%d" % n, (n,)).clamp(-3.5, 3.5)
    if zero:            # denom = eps: m of eps' size, so that the update stays one
        g, v, m = torch.zeros(n), torch.zeros(n), m * 1e-8
    return dict(p=p, g=g, m=m, v=v, ema=ema)


def adam_reference(d, eps_mode, grad_scale, step, as_given=False):
    """one step in fp64 from fp32 inputs and fp32 hyper-parameters.  S per element: every product and sum rounds; the root halves
    what v lost; p' = p - step_size * (m' / denom) rounds at the size of p'"""
    h = _hyper(as_given)
    b1, b2, eps, dec = h["beta1"], h["beta2"], h["eps"], h["ema_decay"]
    ss, isb = adam_corrections(step, eps_mode, as_given)
    p, g, m, v, ema = (d[k].double() for k in ("p", "g", "m", "v", "ema"))
    gg = g * float(f32(grad_scale))
    t1, t2 = m * b1, (1 - b1) * gg
    m2 = t1 + t2
    S_m = 2 * (t1.abs() + t2.abs()) + t2.abs() + m2.abs()
    u1, u2 = v * b2, (1 - b2) * gg * gg
    v2 = u1 + u2
    S_v = 2 * (u1 + u2) + 3 * u2 + v2
    rt = v2.sqrt()
    rts = torch.where(rt > 0, rt, torch.ones_like(rt))
    S_rt = 0.5 * S_v / rts + rt
    if eps_mode == 0:
        den, S_den = rt * isb + eps, isb * (S_rt + 2 * rt)
    else:
        den, S_den = rt + eps, S_rt
    S_den = S_den + den
    q = m2 / den
    S_q = S_m / den + q.abs() * S_den / den + q.abs()
    upd = ss * q
    p2 = p - upd
    S_p = ss * S_q + 2 * upd.abs() + p2.abs()
    e1, e2 = ema * dec, (1 - dec) * p2
    ref = {"adam_p": p2, "adam_m": m2, "adam_v": v2, "adam_ema": e1 + e2}
    S = {"adam_p": S_p, "adam_m": S_m, "adam_v": S_v, "adam_ema": 2 * (e1.abs() + e2.abs()) + (1 - dec) * S_p + e2.abs() + (e1 + e2).abs()}
    return ref, S


def restate_adam_fp32(d, eps_mode, grad_scale, step):
    """adam_kernel in numpy fp32, operation order kept; the step size and 1 / sqrt(1 - b2^t) as the host forms them (fp64 -> fp32)"""
    h = {k: f32(v) for k, v in ADAM_HYPER.items()}
    b1, b2, eps, dec, one = h["beta1"], h["beta2"], h["eps"], h["ema_decay"], f32(1)
    bc1, bc2 = 1.0 - float(b1) ** step, 1.0 - float(b2) ** step
    lr = float(h["lr"])
    ss = f32(lr / bc1) if eps_mode == 0 else f32(lr * math.sqrt(bc2) / bc1)
    isb = f32(1.0 / math.sqrt(bc2))
    p, g, m, v, ema = (d[k].numpy() for k in ("p", "g", "m", "v", "ema"))
    gg = g * f32(grad_scale)
    m2 = m * b1 + (one - b1) * gg
    v2 = v * b2 + (one - b2) * gg * gg
    den = np.sqrt(v2) * isb + eps if eps_mode == 0 else np.sqrt(v2) + eps
    p2 = p - ss * (m2 / den)
    out = {"adam_p": p2, "adam_m": m2, "adam_v": v2, "adam_ema": ema * dec + (one - dec) * p2}
    assert all(x.dtype == f32 for x in out.values())
    return out
