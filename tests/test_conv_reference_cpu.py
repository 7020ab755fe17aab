"""The per-element tolerances of tests/test_conv_entry_points_gpu.py are set against references, not against the kernels: this
file measures the references themselves on every case of the convolution tables (tests/conv_cases.py) and asserts that each stays
within a QUARTER of the constant the GPU file imports.

Measure: max over the elements of |reference - fp64| / S, S = the same convolution / gradient over the absolute values of both
operands in fp64 (conv_cases.references), inputs from helpers.det_array as in the GPU tests.

  torch's fp32 CPU convolution, data gradient and weight gradient (F.conv2d, torch.nn.grad.conv2d_input / conv2d_weight), over
  CONV_CASES, UP_CASES, PK_CASES and PK_WGRAD_CASES -- the bound of the small-channel, stem, direct, implicit-GEMM, up-convolution
  and packed kernels.  Largest figures (x86-64, oneDNN; the largest of runs with 1, 4, 8 and 16 threads, which move the data and
  weight gradient figures by up to 3 % and the case they fall on):
      forward          2.68e-7   CONV_CASES (2, 3, 64, 96, 40, (4, 4), 2, (1, 1), 0)       -> TOL["fwd"]   = 4 x = 1.1e-6
      data gradient    3.01e-7   CONV_CASES (2, 192, 32, 32, 96, (4, 4), 2, (1, 1), 0)     -> TOL["dgrad"] = 4 x = 1.3e-6
      weight gradient  4.60e-7   CONV_CASES (16, 256, 8, 8, 192, (4, 4), 2, (1, 1), 0)     -> TOL["wgrad"] = 4 x = 1.9e-6
  a plain fp32 emulation of Winograd F(2x2,3x3) from the textbook matrices (conv_cases.wino_fwd / wino_dgrad / wino_wgrad: fp32
  transforms, fp32 products and sums), over the cases the dispatch hands to the Winograd kernels (conv_cases.wino_geometry) -- the
  bound of wino3_fwd_kernel, its 16-wave form and wino_wgrad_kernel.  Largest figures:
      forward          1.65e-7   CONV_CASES (2, 32, 8, 32, 64, (3, 3), 1, (1, 1), 0)       -> TOL_WINO["fwd"]   = 4 x = 6.7e-7
      data gradient    2.76e-7   CONV_CASES (2, 80, 29, 63, 96, (3, 3), 1, (0, 0), 0)      -> TOL_WINO["dgrad"] = 4 x = 1.2e-6
      weight gradient  2.47e-7   CONV_CASES (2, 256, 16, 16, 64, (3, 3), 1, (1, 1), 0)     -> TOL_WINO["wgrad"] = 4 x = 1.0e-6
  (4 x the figure, rounded up to two digits.)  The factor 4 is what a right kernel may do differently from the reference: another
  summation order (tiles, split-K slabs), the dropped terms of the split-bf16 products (<= 2^-23 |a b|, csrc/mogan_mma.h), one more
  rounding of the pre-summed filters K = T w T^t of the up-convolution.  The emulation is also checked in fp64 against the direct
  convolution (it is the same function to 1e-12), so that its fp32 error is the algorithm's and not a mistake in the matrices.

Every run prints the figures it measured (pytest -s shows them)."""
import pytest
import torch

import conv_cases as C

TABLES = ([("conv", c) for c in C.CONV_CASES] + [("up", c) for c in C.UP_CASES] + [("pk", c) for c in C.PK_CASES]
          + [("pw", c) for c in C.PK_WGRAD_CASES])


@pytest.fixture(scope="module", autouse=True)
def _four_threads():
    """the fp32 figures depend (in the last digit) on how the CPU library splits its sums over threads: measured with 4"""
    n = torch.get_num_threads()
    torch.set_num_threads(4)
    yield
    torch.set_num_threads(n)


def _inputs(kind, case):
    if kind == "conv":
        return C.conv_inputs(case), case
    if kind == "up":
        return C.up_inputs(case), C.as_conv_case(case, "up")
    return C.pk_inputs(case, wgrad=kind == "pw"), C.as_conv_case(case, "pk")


def _ratio(got, ref, S):
    return float(((got.double() - ref).abs() / S.clamp_min(1e-300)).max())


def test_constants_are_below_the_projects_ceiling():
    for t in list(C.TOL.values()) + list(C.TOL_WINO.values()):
        assert 0 < t <= C.TOL_CEILING


def test_fp32_cpu_convolutions_stay_within_a_quarter_of_tol():
    worst = {}
    for kind, case in TABLES:
        (x, w, g), (B, Cin, H, W, Cout, k, s, pad, up) = _inputs(kind, case)
        ref, S = C.references(x, w, g, s, pad, up)
        got = C.conv_all(x, w, g, s, pad, up)
        for d, key in (("fwd", "y"), ("dgrad", "dxu"), ("dgrad", "dx"), ("wgrad", "dw")):
            r = _ratio(got[key], ref[key], S[key])
            if r > worst.get(d, (0.0, None))[0]:
                worst[d] = (r, (kind, case))
            assert r <= C.TOL[d] / 4, "fp32 CPU %s of %s %s: err / S = %.3e > TOL / 4 = %.3e" % (d, kind, case, r, C.TOL[d] / 4)
    for d, (r, c) in sorted(worst.items()):
        print("fp32 CPU %-5s largest err / S = %.3e (TOL / 4 = %.3e) at %s" % (d, r, C.TOL[d] / 4, c))


def test_winograd_emulation_is_the_convolution_and_stays_within_a_quarter_of_tol_wino():
    worst, n = {}, [0, 0, 0]
    for case in C.CONV_CASES:
        fwd, dgrad, wgrad = C.wino_geometry(case)
        if not (fwd or dgrad or wgrad):
            continue
        x, w, g = C.conv_inputs(case)
        B, Cin, H, W, Cout, k, s, pad, up = case
        ref, S = C.references(x, w, g, s, pad, up)
        runs = []
        if fwd:
            runs.append(("fwd", "y", lambda dt: C.wino_fwd(x.to(dt), w.to(dt), pad[0])))
        if dgrad:
            runs.append(("dgrad", "dxu", lambda dt: C.wino_dgrad(g.to(dt), w.to(dt), pad[0])))
        if wgrad:
            runs.append(("wgrad", "dw", lambda dt: C.wino_wgrad(x.to(dt), g.to(dt))))
        for d, key, fn in runs:
            n[("fwd", "dgrad", "wgrad").index(d)] += 1
            assert _ratio(fn(torch.float64), ref[key], S[key]) <= 1e-12, "the emulation (%s) is not the convolution: %s" % (d, case)
            r = _ratio(fn(torch.float32), ref[key], S[key])
            if r > worst.get(d, (0.0, None))[0]:
                worst[d] = (r, case)
            assert r <= C.TOL_WINO[d] / 4, "Winograd emulation %s of %s: err / S = %.3e > TOL_WINO / 4 = %.3e" % (
                d, case, r, C.TOL_WINO[d] / 4)
    assert min(n) >= 5, "too few Winograd geometries in CONV_CASES (fwd, dgrad, wgrad): %s" % n
    for d, (r, c) in sorted(worst.items()):
        print("Winograd emulation %-5s largest err / S = %.3e (TOL_WINO / 4 = %.3e) at %s" % (d, r, C.TOL_WINO[d] / 4, c))
