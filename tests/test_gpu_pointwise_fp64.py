"""GPU: the kernels AROUND the convolutions -- scalar losses, InstanceNorm, element-wise helpers, Adam -- against plain
float64 references (tests/ref64.py, themselves checked against the fp32 oracle by tests/test_ref64.py), on every
dispatch path of their launchers.  Run on the MI355X box:  python -m pytest tests/test_gpu_pointwise_fp64.py -m gpu -q

Tolerances.  The project's bars (header of tests/test_gpu_ops.py): BAR = 1e-4 of the tensor's maximum for fp32 results
and for the scalar losses, BAR_GRAD = 1e-3 for long-reduction gradients (the NCC gradient: three box passes over win^nd
terms each); the InstanceNorm gradient keeps the 3e-4 of test_instnorm.  Where the INPUT makes the operation itself
ill-conditioned in fp32 (flat-background NCC, InstanceNorm of a constant plane or with mean >> std, full-size reductions,
Adam over 200 steps) the bound is `max(bar, 2 x error of the fp32 CPU oracle / plain fp32 torch against the same float64
reference on the same input)`, computed in the test by bounded(); 2 x is the README's convention and covers another valid
fp32 summation order.  bounded() refuses an input whose bound would exceed 10 x the bar (nothing would be tested), and
tests/test_ref64.py checks that on the CPU for every such input of this module.  Every comparison lands in
tests.test_gpu_ops.MARGINS (DFMIR_MARGINS_OUT writes the table: profiles/r07_pointwise_margins.txt).

Launcher branch -> test id (csrc/losses.hip; `fwd` / `bwd` name the kernels a case runs):
  dfmir_flow_smooth_fwd_p
    flow_smooth_fwd_v4_k<16>            test_flow_smoothness_l2[v4-tpr16_*], [rows3-lt8_v4-tpr16_*], [degenerate cases with W % 4 == 0]
    flow_smooth_fwd_v4_k<32>            test_flow_smoothness_l2[v4-tpr32_*]
    flow_smooth_fwd_v4_k<64>            test_flow_smoothness_l2[v4-tpr64_*], [rows6-lt8_*], [2d-256x256-b16_*], test_flow_smoothness_full_size_value
    flow_smooth_fwd_k<false> (W > 256)  test_flow_smoothness_l2[scalar-W260_*]
    flow_smooth_fwd_k<false> (W % 4)    test_flow_smoothness_l2[scalar-Wmod4_*]
    flow_smooth_fwd_k<true>  (L1)       test_flow_smoothness_l1[*]
  dfmir_flow_smooth_bwd_p
    flow_smooth_bwd_march_k             test_flow_smoothness_l2[*_bwd-march]
    flow_smooth_bwd_v4_k<16|32|64>      test_flow_smoothness_l2[*_bwd-v4-tpr16|32|64*] (D < 8, H < FS_RY, 2-D)
    flow_smooth_bwd_k<unsigned>         test_flow_smoothness_l2[scalar-*_bwd-scalar]
    flow_smooth_bwd_k<unsigned, L1>     test_flow_smoothness_l1[*]
    flow_smooth_bwd_k<long long>        test_flow_smoothness_backward_64bit_index[bwd-scalar-int64]  (2^31 elements; the
    flow_smooth_bwd_k<long long, L1>    ...[bwd-scalar-int64-l1]               float64 reference is formed on the device, in chunks)
  dfmir_ncc_fwd_m / ncc_prod_boxw_launch / box_axis_launch
    ncc_prod_boxwh_k + box_axis_march_k (D)       test_ncc[3d-win9_*]  (1 / 2 / 3 segments of 36 planes: D35, D36, D37, D80)
    ncc_prod_boxw_k + box_axis_k (H, D)           test_ncc[3d-win5_*], [3d-win3_*]
    ncc_prod_boxw_x4_k + box_axis_march_k (H)     test_ncc[2d-win9_boxw-x4_*], [3d-win9_D1-one-plane*]
    ncc_prod_boxw_k (r = 4, W % 4 or W < 8)       test_ncc[2d-win9_boxw-generic_*], [2d-win9_W6*]
    ncc_prod_boxw_k + box_axis_k (r != 4)         test_ncc[2d-win7_*]
    ncc_cc_reduce_k / ncc_fin_k with `part` (ordered partial sums), modes 0 / 1, masked / not: all of the above.  Their
    atomic form (part == NULL) is unreachable: dfmir_ncc_fwd_m passes part whenever 5 N >= 2 * workgroups, which holds for
    every N >= 1, so no test runs it
  dfmir_ncc_bwd_m
    ncc_fields_boxwh_k + ncc_boxd_combine_k       test_ncc[3d-win9_*] (D > 1)
    ncc_fields_k + box_axis_x4_k (W) + box_axis_march_k (H) + ncc_combine_k       test_ncc[2d-win9_boxw-x4_*], [3d-win9_D1-one-plane*]
    ncc_fields_k + box_axis_k (W: W % 4 or W < 8) + box_axis_march_k (H)          test_ncc[2d-win9_boxw-generic_*], [2d-win9_W6*]
    ncc_fields_k + box_axis_k x 2 or 3 + ncc_combine_k                            test_ncc[2d-win7_*], [3d-win5_*], [3d-win3_*]
"""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ref64 as R
from tests.golden import common as C
from tests.test_gpu_ops import MARGINS, close, near, ops  # noqa: F401  (ops: the module-scoped fixture)

pytestmark = pytest.mark.gpu

DEV = "cuda"
BAR, BAR_GRAD, BAR_IN_DX = 1e-4, 1e-3, 3e-4


def _test_id():
    return os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]


def _f64(t):
    return t.detach().to(torch.float64).cpu() if torch.is_tensor(t) else torch.as_tensor(t, dtype=torch.float64)


def oracle_bound(ref, oracle, bar, floor=0.0, where=None):
    """(bound, oracle error, scale): bound = max(bar, 2 x max |oracle - ref| / scale), scale = max(max |ref|, floor)."""
    r, o = _f64(ref), _f64(oracle)
    if where is not None:
        r, o = r[where], o[where]
    scale = max(float(r.abs().max()) if r.numel() else 0.0, floor, 1e-30)
    oerr = float((o - r).abs().max()) / scale if r.numel() else 0.0
    return max(bar, 2.0 * oerr), oerr, scale


def bounded(got, ref, bar, what, oracle=None, floor=0.0, where=None):
    """max |got - ref| <= bound * max(max |ref|, floor); bound = bar, or with `oracle` (the fp32 CPU result on the same input)
    max(bar, 2 x the oracle's own error) -- never above 10 x bar: such an input tests nothing and must be replaced.
    `where` (bool tensor) restricts the comparison.  Both figures go to MARGINS."""
    g, r = _f64(got), _f64(ref)
    assert g.shape == r.shape, "%s: shape %s vs %s" % (what, tuple(g.shape), tuple(r.shape))
    assert bool(torch.isfinite(g).all()), "%s: non-finite values" % what
    if where is not None:
        g, r = g[where], r[where]
    bound, scale = bar, max(float(r.abs().max()) if r.numel() else 0.0, floor, 1e-30)
    if oracle is not None:
        bound, oerr, scale = oracle_bound(ref, oracle, bar, floor, where)
        assert bound <= 10 * bar, "%s: the fp32 oracle itself is off by %.2e (bar %.0e): input too ill-conditioned" % (what, oerr, bar)
        MARGINS.append((_test_id(), what + " [fp32 oracle vs fp64]", oerr, bound))
    err = float((g - r).abs().max()) / scale if r.numel() else 0.0
    MARGINS.append((_test_id(), what, err, bound))
    assert err <= bound, "%s: rel err %.3e > %.3e (scale %.3e)" % (what, err, bound, scale)


# ===================================================================================== 1. flow smoothness
# (id, shape): id = forward kernel _ backward kernel of dfmir_flow_smooth_fwd_p / _bwd_p (FS_RY = 8)
FLOW_L2 = [
    ("v4-tpr16_rows567_bwd-march", (1, 3, 9, 21, 64)),
    ("v4-tpr32_rows570_bwd-march", (1, 3, 10, 19, 100)),
    ("v4-tpr64_W252_rows264_bwd-march", (1, 3, 8, 11, 252)),
    ("v4-tpr64_W256_batch2_bwd-march", (2, 3, 9, 13, 256)),
    ("rows6-lt8_v4-tpr64_bwd-v4-tpr64", (1, 1, 2, 3, 256)),
    ("rows3-lt8_v4-tpr16_2d_bwd-v4-tpr16", (1, 1, 3, 40)),
    ("rows13_v4-tpr32_2d_bwd-v4-tpr32", (1, 1, 13, 128)),
    ("scalar-W260_rb2_bwd-scalar", (1, 3, 9, 100, 260)),
    ("scalar-Wmod4_bwd-scalar", (2, 3, 9, 12, 37)),
    ("2d-256x256-b16_v4-tpr64_bwd-v4-tpr64", (16, 2, 256, 256)),
    ("3d-D5-lt8_v4-tpr16_bwd-v4-tpr16", (1, 3, 5, 24, 64)),
    ("3d-D4-lt8_v4-tpr32_bwd-v4-tpr32", (2, 3, 4, 16, 128)),
    ("3d-H6-ltFS_RY_v4-tpr64_bwd-v4-tpr64", (1, 3, 12, 6, 200)),
]
FLOW_L1 = [
    ("l1-scalar_3d_W64", (1, 3, 9, 21, 64)),
    ("l1-scalar_2d_rows2800-rb2_Wmod4", (2, 2, 700, 37)),
    ("l1-scalar_3d_W260", (1, 3, 5, 6, 260)),
]


def _flow_case(ops, shape, penalty, seed=611):
    flow = C.randn(seed, *shape) * 1.5
    fr = flow.double().requires_grad_()
    lr = R.grad_loss(fr, penalty)
    (lr * 3.0).backward()
    fg = flow.clone().to(DEV).requires_grad_()
    lg = ops.flow_smoothness(fg, penalty)
    (lg * 3.0).backward()                                      # upstream gradient 3, not 1
    return lg, fg.grad, lr, fr.grad


@pytest.mark.parametrize("shape", [c[1] for c in FLOW_L2], ids=[c[0] for c in FLOW_L2])
def test_flow_smoothness_l2(ops, shape):
    """Grad_Loss / smooothing_loss, penalty 'l2': value and gradient against float64 on every kernel of the launchers."""
    lg, dg, lr, dr = _flow_case(ops, shape, 'l2')
    near(lg, lr, BAR, "smooth l2 value")
    close(dg, dr, rtol=BAR, atol=0.0, what="smooth l2 gradient")


@pytest.mark.parametrize("shape", [c[1] for c in FLOW_L1], ids=[c[0] for c in FLOW_L1])
def test_flow_smoothness_l1(ops, shape):
    """penalty 'l1' (row-walking forward kernel, scalar backward kernel with sgn): value and gradient against float64.  The
    gradient is a sum of signs of fp32 differences, which carry the sign of the exact differences."""
    lg, dg, lr, dr = _flow_case(ops, shape, 'l1')
    near(lg, lr, BAR, "smooth l1 value")
    close(dg, dr, rtol=BAR, atol=0.0, what="smooth l1 gradient")


def test_flow_smoothness_full_size_value(ops):
    """One 1x3x160x192x224 field (flow_smooth_fwd_v4_k<64>, 512 workgroups over the 8 XCDs, 12 rows per thread): the VALUE
    against float64 (the gradient there is pinned bit-wise by test_flow_smoothness_backward_marching_kernel's kernel pair).
    A full-size reduction: bound from plain fp32 torch on the same field."""
    flow = C.randn(612, 1, 3, 160, 192, 224)
    lr = R.grad_loss(flow, 'l2')
    lo = R.grad_loss(flow, 'l2', dtype=torch.float32)
    lg = ops.flow_smoothness(flow.to(DEV), 'l2')
    bounded(lg, lr, BAR, "smooth l2 full-size value", oracle=lo)


@pytest.mark.parametrize("shape", [(1, 2, 6, 5, 1), (1, 2, 6, 8, 1), (2, 2, 1, 9), (2, 2, 1, 8), (1, 2, 7, 1), (1, 3, 4, 1, 12),
                                   (1, 3, 1, 6, 8)],
                         ids=["3d-W1", "3d-W1-H8", "2d-H1-W9", "2d-H1-W8-v4", "2d-W1", "3d-H1-W12-v4", "3d-D1-one-plane"])
@pytest.mark.parametrize("penalty", ['l2', 'l1'])
def test_flow_smoothness_degenerate_axes(ops, shape, penalty):
    """An axis of extent 1 has no forward differences; torch's mean over the empty difference is NaN, so the reference
    gives NaN.  The mirror (documented at dfmir_amd.losses.Grad_Loss): such an axis contributes 0 to value and gradient and
    the divisor stays the number of axes, except that a 3-D field of one plane is the 2-D field it is (divisor 2)."""
    from dfmir_amd.losses import Grad_Loss
    assert "Degenerate axes" in Grad_Loss.__doc__ and "contributes 0" in Grad_Loss.__doc__
    flow = C.randn(613, *shape) * 1.5
    assert bool(torch.isnan(R.grad_loss(flow, penalty)))                      # the reference's answer
    fr = flow.double().requires_grad_()
    if len(shape) == 5 and shape[2] == 1:
        lr = R.grad_loss(fr[:, :, 0], penalty, skip_empty=True)               # one plane: a 2-D field
    else:
        lr = R.grad_loss(fr, penalty, skip_empty=True)
    (lr * 3.0).backward()
    fg = flow.clone().to(DEV).requires_grad_()
    lg = Grad_Loss(dim=len(shape) - 2, penalty=penalty)(fg)
    (lg * 3.0).backward()
    near(lg, lr, BAR, "smooth %s degenerate value" % penalty)
    close(fg.grad, fr.grad, rtol=BAR, atol=0.0, what="smooth %s degenerate gradient" % penalty)


@pytest.mark.parametrize("penalty", ['l2', 'l1'], ids=["bwd-scalar-int64", "bwd-scalar-int64-l1"])
def test_flow_smoothness_backward_64bit_index(ops, penalty):
    """flow_smooth_bwd_k<long long> / <long long, L1>: a 2-D field of 2 x 32769 x 32771 = 2 147 844 198 elements (>= 2^31,
    W odd, so both launchers take their scalar kernels; 8.6 GB, and as much for the gradient).  The field is a seeded
    257-row block repeated down the image, each repetition scaled by an exactly representable factor.  A float64 reference
    of that size does not fit a host, so it is formed ON THE DEVICE by plain torch in float64, 2048 rows (plus one halo
    row each side) at a time: the value from the differences of the chunk's own rows, the gradient of its rows by
    autograd on the chunk's share of the loss.  Every element is compared, the last rows of plane 1 -- flat index above
    2^31 -- included."""
    Cc, H, W, RB = 2, 32769, 32771, 257
    assert Cc * H * W >= 2 ** 31
    base = C.randn(619, Cc, RB, W).to(DEV)
    rows = torch.arange(H, device=DEV)
    flow = (base[:, rows % RB] * (1.0 + (rows // RB).float() / 128.0)[None, :, None])[None].contiguous()
    del base
    fg = flow.requires_grad_()
    lg = ops.flow_smoothness(fg, penalty)
    (lg * 3.0).backward()
    pen = (lambda d: d * d) if penalty == 'l2' else (lambda d: d.abs())
    cw, ch = float(Cc * H * (W - 1)), float(Cc * (H - 1) * W)
    val = torch.zeros((), device=DEV, dtype=torch.float64)
    err = ref_max = 0.0
    for r0 in range(0, H, 2048):
        r1 = min(H, r0 + 2048)
        a, b = max(r0 - 1, 0), min(r1 + 1, H)
        f = flow.detach()[:, :, a:b].double().requires_grad_()
        dx, dy = f[..., 1:] - f[..., :-1], f[:, :, 1:] - f[:, :, :-1]
        (3.0 * (pen(dx).sum() / cw + pen(dy).sum() / ch) / 2.0).backward()
        g = f.grad[:, :, r0 - a:r0 - a + (r1 - r0)]
        err = max(err, float((fg.grad[:, :, r0:r1].double() - g).abs().max()))
        ref_max = max(ref_max, float(g.abs().max()))
        with torch.no_grad():                                    # the chunk's own rows: dx of r0 .. r1 - 1, dy of the pairs (h, h + 1)
            val += pen(dx[:, :, r0 - a:r0 - a + (r1 - r0)]).sum() / cw + pen(dy[:, :, r0 - a:r0 - a + (min(r1, H - 1) - r0)]).sum() / ch
        del f, dx, dy, g
    near(lg, float(val) / 2.0, BAR, "smooth %s value, 2^31 elements" % penalty)
    MARGINS.append((_test_id(), "smooth %s gradient, 2^31 elements" % penalty, err / ref_max, BAR))
    assert bool(torch.isfinite(fg.grad[0, 1, -8:]).all()) and err <= BAR * ref_max, (err, ref_max)
    del flow, fg
    torch.cuda.empty_cache()


def test_grad_loss_mask_and_loss_mult(ops):
    """Grad_Loss with `mask=` (ops.mul in front) and loss_mult (ops.scale behind), 2-D and 3-D, both penalties."""
    from dfmir_amd.losses import Grad_Loss
    for nd, shape in ((2, (2, 2, 33, 52)), (3, (1, 3, 9, 10, 36))):
        flow = C.randn(614 + nd, *shape)
        mask = (C.rand(616 + nd, shape[0], 1, *shape[2:]) > 0.3).float()
        for penalty in ('l2', 'l1'):
            fr = flow.double().requires_grad_()
            lr = R.grad_loss(fr, penalty, mask=mask, loss_mult=2.5)
            (lr * 3.0).backward()
            fg = flow.clone().to(DEV).requires_grad_()
            lg = Grad_Loss(dim=nd, penalty=penalty, loss_mult=2.5)(fg, mask=mask.to(DEV))
            (lg * 3.0).backward()
            near(lg, lr, BAR, "masked Grad_Loss %s %d-D value" % (penalty, nd))
            close(fg.grad, fr.grad, rtol=BAR, atol=0.0, what="masked Grad_Loss %s %d-D gradient" % (penalty, nd))


# ================================================================================================== 2. NCC
def smooth_field(seed, shape, div=6):
    """A smooth [0, 1] field: seeded low-resolution noise, linearly interpolated to `shape` = (B, 1, *spatial)."""
    sp = shape[2:]
    lo = C.rand(seed, shape[0], 1, *[max(2, s // div) for s in sp])
    return F.interpolate(lo, size=sp, mode='bilinear' if len(sp) == 2 else 'trilinear', align_corners=True)


def phantom_pair(seed, shape, family):
    """A smooth blob (an ellipsoid, ~40 % of the voxels) on a CONSTANT background, and a second image of it, shifted and
    re-shaded.  family '01': intensities on [0, 1], background 0.1 (not representable in binary); '11': on [-1, 1] with
    the -1 background of tests.golden.common.image_pair."""
    sp = shape[2:]
    nd = len(sp)
    a = 0.914 if nd == 3 else 0.714                               # 4/3 pi a^3 / 8 = pi a^2 / 4 = 0.4
    grids = torch.meshgrid(*[torch.arange(s, dtype=torch.float32) for s in sp], indexing='ij')

    def inside(shift):                                            # shift: voxels along the last axis
        r2 = sum(((g - (s - 1) / 2.0 - (shift if i == nd - 1 else 0.0)) / (a * s / 2.0)) ** 2
                 for i, (g, s) in enumerate(zip(grids, sp)))
        return (r2 < 1.0)[None, None].expand(shape)
    lo, hi, bg = (0.2, 1.0, 0.1) if family == '01' else (-0.8, 1.0, -1.0)
    t1, t2 = smooth_field(seed, shape), smooth_field(seed + 1, shape)
    I = torch.where(inside(0.0), lo + (hi - lo) * t1, torch.full(shape, bg))
    J = torch.where(inside(1.0), lo + (hi - lo) * (0.7 * t1 + 0.3 * t2), torch.full(shape, bg))
    return I.contiguous(), J.contiguous()


def noise_pair(seed, shape):
    I = C.rand(seed, *shape)
    return I, 0.6 * I + 0.4 * C.rand(seed + 1, *shape)


# (id, shape, win, family, masked, reduction).  Family '01' (background 0.1) sits on the shapes where the fp32 oracle's own dI
# stays within 10 x BAR_GRAD of float64: on volumes with large flat corners (35x40x70 win 9, 14x20x37 win 5) the oracle is
# off by 3.6e-2 / 6.3e-2 of max |dI| and two valid fp32 summation orders differ by 100 x -- nothing to test; those shapes
# carry family '11' (measured by tests/test_ref64.py::test_phantom_ncc_inputs_are_testable).  Family '11' alone would not do:
# -1 is representable, its window sums are exact and the variance terms cancel to exactly 0.  So the 0.1 background also
# runs on a volume of 2 x 2 ragged 32 x 64 tiles (16x36x66, win 9) and on the win 5 3-D path (10x12x37), where fewer windows
# are entirely flat and the oracle's dI stays within 1.1e-4 of float64.
NCC_CASES = [
    ("3d-win9_boxwh-ragged-tiles_D35-1seg_batch2_Wmod4", (2, 1, 35, 40, 70), 9, "noise", False, "neg_sqrt_mean"),
    ("3d-win9_boxwh-ragged-tiles_D35-1seg_batch2_Wmod4_phantom11_masked", (2, 1, 35, 40, 70), 9, "11", True, "neg_sqrt_mean"),
    ("3d-win9_D36-1seg_phantom11_neg-mean", (1, 1, 36, 33, 65), 9, "11", False, "neg_mean"),
    ("3d-win9_D37-2seg_masked", (1, 1, 37, 20, 24), 9, "noise", True, "neg_sqrt_mean"),
    ("3d-win9_D80-3seg_phantom01", (1, 1, 80, 20, 24), 9, "01", False, "neg_sqrt_mean"),
    ("3d-win9_tiles3x3-ragged_neg-mean", (1, 1, 6, 70, 150), 9, "noise", False, "neg_mean"),
    ("3d-win9_tiles2x2-ragged_phantom01_masked", (1, 1, 16, 36, 66), 9, "01", True, "neg_sqrt_mean"),
    ("3d-win9_W6-lt8", (1, 1, 12, 20, 6), 9, "noise", False, "neg_sqrt_mean"),
    ("3d-win9_H5-lt-window_masked", (1, 1, 12, 5, 40), 9, "noise", True, "neg_sqrt_mean"),
    ("3d-win9_D1-one-plane", (1, 1, 1, 40, 72), 9, "noise", False, "neg_sqrt_mean"),
    ("3d-win9_D1-one-plane_batch2_phantom01_masked_neg-mean", (2, 1, 1, 33, 32), 9, "01", True, "neg_mean"),
    ("3d-win5_box-axis_Wmod4", (1, 1, 14, 20, 37), 5, "noise", False, "neg_sqrt_mean"),
    ("3d-win5_box-axis_phantom11_masked", (1, 1, 14, 20, 37), 5, "11", True, "neg_sqrt_mean"),
    ("3d-win5_box-axis_phantom01", (1, 1, 10, 12, 37), 5, "01", False, "neg_sqrt_mean"),
    ("3d-win3_box-axis_batch2_neg-mean", (2, 1, 9, 33, 16), 3, "noise", False, "neg_mean"),
    ("2d-win9_boxw-x4_H-march_batch2", (2, 1, 70, 152), 9, "noise", False, "neg_sqrt_mean"),
    ("2d-win9_boxw-x4_H-march_phantom11_masked", (2, 1, 70, 152), 9, "11", True, "neg_sqrt_mean"),
    ("2d-win9_boxw-generic_Wmod4_phantom01", (1, 1, 40, 70), 9, "01", False, "neg_sqrt_mean"),
    ("2d-win7_box-axis_batch2_masked_neg-mean", (2, 1, 33, 50), 7, "noise", True, "neg_mean"),
    ("2d-win7_box-axis_phantom01", (1, 1, 33, 50), 7, "01", False, "neg_sqrt_mean"),
    ("2d-win9_W6-lt8", (1, 1, 30, 6), 9, "noise", False, "neg_sqrt_mean"),
    ("2d-win9_H5-lt-window", (1, 1, 5, 40), 9, "noise", False, "neg_mean"),
    ("3d-win9_full-size-160x192x224", (1, 1, 160, 192, 224), 9, "noise", False, "neg_sqrt_mean"),
]
NCC_UPSTREAM = 1.7


def ncc_inputs(case):
    _, shape, win, family, masked, reduction = case
    I, J = noise_pair(621, shape) if family == "noise" else phantom_pair(623, shape, family)
    mask = (C.rand(625, *shape) > 0.3).float() if masked else None
    return I, J, mask


def ncc_fp32_oracle(case, I, J, mask):
    """(loss, dI) of the fp32 yardstick: the CPU oracle (oracle/dfmir_oracle.py, a conv with win^nd taps) where that is
    affordable and has the form asked for, else the plain fp32 restatement of tests/ref64.py (separable 9-term sums)."""
    from oracle import dfmir_oracle as O
    _, shape, win, family, masked, reduction = case
    Io = I.clone().requires_grad_()
    if I.numel() * win ** (len(shape) - 2) <= 3e7 and not (masked and reduction == "neg_mean"):
        lo = O.ncc_loss(Io, J, win, 1e-5, mask) if reduction == "neg_sqrt_mean" else O.vxm_ncc_loss(J, Io, win)
    else:
        lo = R.ncc_loss(Io, J, win, 1e-5, mask, reduction, dtype=torch.float32)
    (lo * NCC_UPSTREAM).backward()
    return lo.detach(), Io.grad


@pytest.mark.parametrize("case", NCC_CASES, ids=[c[0] for c in NCC_CASES])
def test_ncc(ops, case):
    """Windowed NCC through losses.NCC_Loss ('neg_sqrt_mean') / voxelmorph.losses.NCC ('neg_mean') and ops.ncc_loss: value
    and dI against float64.  Phantom inputs (flat background: the variance terms cancel to round-off, which eps then
    divides) take the bound from the fp32 oracle's own error on the same input."""
    from dfmir_amd import losses as L
    from dfmir_amd import voxelmorph as V
    _, shape, win, family, masked, reduction = case
    nd = len(shape) - 2
    I, J, mask = ncc_inputs(case)
    Ir = I.double().requires_grad_()
    lr = R.ncc_loss(Ir, J, win, 1e-5, mask, reduction)
    (lr * NCC_UPSTREAM).backward()
    Jg, mg = J.to(DEV), (mask.to(DEV) if masked else None)
    Ig = I.clone().to(DEV).requires_grad_()
    if reduction == "neg_sqrt_mean":
        lg = L.NCC_Loss(DEV, kernel_var=[win] * nd, kernel_type='mean')(Ig, Jg, mask=mg)
    elif not masked:
        lg = V.losses.NCC([win] * nd).loss(Jg, Ig)
    else:
        lg = ops.ncc_loss(Ig, Jg, win, 1e-5, mask=mg, reduction=reduction)
    (lg * NCC_UPSTREAM).backward()
    # bit-identical by design: the forward adds per-workgroup partial sums in a fixed order (no atomics; see the docstring
    # of this module).  A reduction whose result depends on the order of arrival would need a tolerance here.
    direct = ops.ncc_loss(I.to(DEV), Jg, win, 1e-5, mask=mg, reduction=reduction)
    assert float(direct) == float(lg), "ops.ncc_loss and the loss class disagree"
    if family == "noise":
        bounded(lg, lr, BAR, "ncc value")
        bounded(Ig.grad, Ir.grad, BAR_GRAD, "ncc dI")
    else:
        lo, dIo = ncc_fp32_oracle(case, I, J, mask)
        bounded(lg, lr, BAR, "ncc value (phantom)", oracle=lo)
        bounded(Ig.grad, Ir.grad, BAR_GRAD, "ncc dI (phantom)", oracle=dIo)


def _misaligned(t):
    """The same values, contiguous, on the device, 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, device=DEV, dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def test_misaligned_inputs_take_the_scalar_kernels(ops):
    """The float4 kernels are chosen by shape AND by 16-byte pointer alignment: the same shapes on a base pointer 4 bytes off
    must fall back to the scalar kernels (flow_smooth_fwd_k / _bwd_k<unsigned>, ncc_prod_boxw_k) and give the same answers."""
    flow = C.randn(618, 1, 3, 9, 21, 64) * 1.5
    fr = flow.double().requires_grad_()
    lr = R.grad_loss(fr, 'l2')
    (lr * 3.0).backward()
    fg = _misaligned(flow).requires_grad_()
    lg = ops.flow_smoothness(fg, 'l2')
    (lg * 3.0).backward()
    near(lg, lr, BAR, "smooth l2 value, misaligned field")
    close(fg.grad, fr.grad, rtol=BAR, atol=0.0, what="smooth l2 gradient, misaligned field")
    I, J = noise_pair(619, (2, 1, 70, 152))
    Ir = I.double().requires_grad_()
    nr = R.ncc_loss(Ir, J, 9)
    (nr * NCC_UPSTREAM).backward()
    Ig = _misaligned(I).requires_grad_()
    ng = ops.ncc_loss(Ig, _misaligned(J), 9, 1e-5)
    (ng * NCC_UPSTREAM).backward()
    bounded(ng, nr, BAR, "ncc value, misaligned images")
    bounded(Ig.grad, Ir.grad, BAR_GRAD, "ncc dI, misaligned images")


# ============================================================================================ 3. masked L1
def l1_pair(seed, n):
    """[-1, 1] values with ~40 % of each image at the -1 background (so the > -0.95 mask is non-trivial)."""
    a, b = C.rand(seed, n) * 2 - 1, C.rand(seed + 1, n) * 2 - 1
    a = torch.where(C.rand(seed + 2, n) < 0.4, torch.full_like(a, -1.0), a)
    b = torch.where(C.rand(seed + 3, n) < 0.4, torch.full_like(b, -1.0), b)
    return a, b


L1_SIZES = [1, 1023, 1025, 128 * 1024 + 7, 16 * 256 * 256, 4096 * 256 + 1029]


@pytest.mark.parametrize("explicit", [False, True], ids=["threshold-mask", "explicit-mask"])
@pytest.mark.parametrize("n", L1_SIZES, ids=["n1", "n1023", "n1025", "n128x1024+7-fwd-two-grid-passes", "n16x256x256-bench-batch",
                                              "n4096x256+1029-bwd-two-grid-passes"])
def test_masked_l1(ops, n, explicit):
    """sum(|a - b| m) / sum(m): value and both gradients against float64.  The forward runs at most 128 workgroups of 1024
    threads, so n > 131072 takes a second pass of the grid-stride loop and n % 1024 != 0 leaves a ragged tail; the backward
    runs at most 4096 workgroups of 256, so only the last size takes its second pass.  The mask
    count is an fp32 sum of ones: per-thread and per-workgroup counts stay far below 2^24 and are exact, and the atomic
    total is exact up to 2^24 = 16 777 216 masked elements; the largest n the plugin reaches is the bench batch
    16 x 256 x 256 = 2^20 (tested here), a mask count above 2^24 is not."""
    if n == 16 * 256 * 256:
        a, b = C.image_pair(631, 16, 256, 256)
    elif n == 1:
        a, b = torch.tensor([0.3]), torch.tensor([-0.2])
    else:
        a, b = l1_pair(632, n)
    mask = (C.rand(636, *a.shape) > 0.45) if explicit else None
    ar, br = a.double().requires_grad_(), b.double().requires_grad_()
    lr = R.masked_l1(ar, br, mask=mask, thr=None if explicit else -0.95)
    (lr * 3.0).backward()
    from oracle import dfmir_oracle as O
    mo = mask.float() if explicit else R.threshold_mask(a, b, -0.95).float()
    lo = O.masked_l1(a, b, mo)                                  # fp32 CPU oracle: the yardstick of the full-size sums
    ag, bg = a.clone().to(DEV).requires_grad_(), b.clone().to(DEV).requires_grad_()
    lg = ops.masked_l1(ag, bg, mask.to(DEV) if explicit else None, -0.95)
    (lg * 3.0).backward()
    bounded(lg, lr, BAR, "masked l1 value", oracle=lo)
    near(lg._df_mask_sum, float(mo.sum()), 0.0, "masked l1 mask count (exact)")
    close(ag.grad, ar.grad, rtol=BAR, atol=0.0, what="masked l1 da")
    close(bg.grad, br.grad, rtol=BAR, atol=0.0, what="masked l1 db")


@pytest.mark.parametrize("explicit", [False, True], ids=["threshold-mask", "explicit-mask"])
def test_masked_l1_empty_mask_and_ties(ops, explicit):
    """All masked out -> exactly 0 and an exactly zero gradient; a == b inside the mask -> gradient exactly 0 there."""
    n = 128 * 1024 + 7
    a, b = l1_pair(637, n)
    if explicit:
        empty = torch.zeros(n, dtype=torch.bool).to(DEV)
        ag, bg = a.clone().to(DEV).requires_grad_(), b.clone().to(DEV).requires_grad_()
    else:
        empty = None                                             # nothing above the threshold
        ag, bg = (a * 0.01 - 0.97).to(DEV).requires_grad_(), (b * 0.01 - 0.97).to(DEV).requires_grad_()
    l = ops.masked_l1(ag, bg, empty, -0.95)
    (l * 3.0).backward()
    assert float(l) == 0.0 and float(ag.grad.abs().max()) == 0.0 and float(bg.grad.abs().max()) == 0.0
    tie = torch.zeros(n, dtype=torch.bool)
    tie[::3] = True
    a2 = torch.where(tie, b, a)                                  # ties, inside the mask wherever b > -0.95
    mask = (C.rand(638, n) > 0.45) if explicit else None
    m = mask if explicit else R.threshold_mask(a2, b, -0.95)
    assert int((tie & m).sum()) > 1000
    ar, br = a2.double().requires_grad_(), b.double().requires_grad_()
    (R.masked_l1(ar, br, mask=mask, thr=None if explicit else -0.95) * 3.0).backward()
    ag, bg = a2.clone().to(DEV).requires_grad_(), b.clone().to(DEV).requires_grad_()
    (ops.masked_l1(ag, bg, mask.to(DEV) if explicit else None, -0.95) * 3.0).backward()
    assert float(ag.grad.cpu()[tie].abs().max()) == 0.0 and float(bg.grad.cpu()[tie].abs().max()) == 0.0
    assert float(ar.grad[tie].abs().max()) == 0.0
    close(ag.grad, ar.grad, rtol=BAR, atol=0.0, what="masked l1 da with ties")
    close(bg.grad, br.grad, rtol=BAR, atol=0.0, what="masked l1 db with ties")


# ========================================================================================= 4. InstanceNorm
IN_PLANES = [(5, 5, "generic-scalar"), (9, 11, "generic-scalar"), (100, 100, "generic-float4"), (64, 64, "reg-256x4"),
             (128, 128, "reg-256x16"), (256, 256, "reg-1024x16")]
IN_FAMILIES = ["randn", "constant", "offset1e3", "tiny1e-6", "one-constant-channel"]
IN_CONST = 0.1                                                   # not representable in binary


def in_input(family, H, W, seed=641):
    shape = (2, 3, H, W)
    z = C.randn(seed, *shape)
    if family == "randn":
        return z * 2 + 0.7
    if family == "constant":
        return torch.full(shape, IN_CONST)
    if family == "offset1e3":
        return z + 1e3
    if family == "tiny1e-6":
        return z * 1e-6
    x = z * 2 + 0.7
    x[:, 1] = IN_CONST                                           # channel 1 of both images constant, the others randn
    return x


def in_reference(x, res, relu, cot, down=False):
    """float64 (y, mean, rstd, dx, dres, xhat) and the plain fp32 torch (y, dx): F.instance_norm -> relu -> + res, as the
    oracle's generator composes them; down: followed by the anti-aliased Downsample."""
    xr = x.double().requires_grad_()
    rr = res.double().requires_grad_() if res is not None else None
    y, mean, rstd = R.instance_norm(xr, rr, relu, 1e-5)
    xhat = ((x.double().reshape(mean.numel(), -1) - mean.detach()[:, None]) * rstd.detach()[:, None]).reshape(x.shape)
    if down:
        y = R.blur_down(y)
    (y * cot.double()).sum().backward()
    xo = x.clone().requires_grad_()
    yo = F.instance_norm(xo, eps=1e-5)
    if relu:
        yo = F.relu(yo)
    if res is not None:
        yo = yo + res
    if down:
        yo = R.blur_down(yo)
    (yo * cot).sum().backward()
    return dict(y=y.detach(), mean=mean.detach(), rstd=rstd.detach(), dx=xr.grad, dres=rr.grad if rr is not None else None,
                xhat=xhat, y32=yo.detach(), dx32=xo.grad)


def in_floor(family):
    """Scale floor of the y / z comparison.  Only on an all-constant tensor: its reference is exactly 0 (without a residual)
    and the error is then taken on the unit scale a normalised plane has.  Every other family, the 1e-6 one (max |y| ~ 1e-3:
    var << eps) included, is compared relative to its own maximum."""
    return 1.0 if family == "constant" else 0.0


def in_mean_unit(x, ref):
    """Per plane, the unit the saved mean's error is measured in: the plane's own standard deviation (an error of the mean
    is an equal shift of every x - mean), or sqrt(var + eps) = 1 / rstd on a constant plane, whose deviation is 0."""
    std = x.double().reshape(ref["mean"].numel(), -1).std(1, unbiased=False)
    return torch.where(std > 0, std, 1.0 / ref["rstd"])


def backward_capturing_dx(x, fn, cot):
    """Run fn on a NON-leaf copy of x and back-propagate cot; returns (output, leaf, the dx tensor the op's backward
    returned).  A leaf's .grad is a copy that loses the range-probe tag; the hook sees the op's own tensor."""
    leaf = x.clone().to(DEV).requires_grad_()
    xin, cap = leaf * 1.0, []
    xin.register_hook(cap.append)
    out = fn(xin)
    return out, leaf, cap, lambda: (out * cot.to(DEV)).sum().backward()


def in_dx_where(family, relu, ref):
    """Elements whose dx is DEFINED in fp32.  With ReLU the gradient gate is xhat > 0: on a constant plane xhat is 0 in exact
    arithmetic and +-round-off in fp32, so the gate is undecidable there (dx is only required to be finite); with
    mean >> std the same holds for the few elements with |xhat| below the fp32 resolution of x - mean (1e-3 here: ulp(1e3)
    = 6e-5 on a unit-variance plane, x 16 of margin)."""
    if not relu:
        return None
    if family == "constant":
        return torch.zeros_like(ref["xhat"], dtype=torch.bool)
    if family == "one-constant-channel":
        w = torch.ones_like(ref["xhat"], dtype=torch.bool)
        w[:, 1] = False
        return w
    if family == "offset1e3":
        return ref["xhat"].abs() > 1e-3
    return None


def check_probe(ops, t, what, source_max=None, slack=0.0):
    """The range probe the op publishes for the next conv: present (ops.amax_of would otherwise measure a fresh absmax and
    the check be trivial), at least the true maximum of the tensor and at most that maximum x (1 + 1e-6).  source_max: the
    fused IN + ReLU + Downsample publishes the maximum of relu(IN(x)) BEFORE the blur (a bound on its convex combinations,
    not their maximum); the upper limit is then that float64 maximum x (1 + BAR), plus `slack` where that maximum is 0 by
    construction (a constant plane)."""
    tag = getattr(t, "_df_amax", None)
    assert tag is not None and ops._amax_ok(t, tag), "%s: the op did not tag its output with a range probe" % what
    probe, true = float(ops.amax_of(t).max()), float(t.detach().abs().max())
    if source_max is None:
        assert probe >= true and probe <= true * (1 + 1e-6), (what, probe, true)
    else:
        assert probe >= true and probe <= source_max * (1 + BAR) + slack, (what, probe, true, source_max)


@pytest.mark.parametrize("relu,res", [(False, True), (True, False)], ids=["res", "relu"])
@pytest.mark.parametrize("family", IN_FAMILIES)
@pytest.mark.parametrize("plane", IN_PLANES, ids=["%dx%d-%s" % p for p in IN_PLANES])
def test_instance_norm(ops, plane, family, relu, res):
    """ops.instance_norm: y, dx, dres, the saved mean / rstd and the published range probe against float64, per kernel
    (generic scalar / float4, the three register kernels) and input family, each relative to its own maximum (in_floor: the
    all-constant tensor, whose reference is 0, on the unit scale).  The range probes of y and of dx must be tight."""
    H, W, _ = plane
    x = in_input(family, H, W)
    r = C.randn(642, *x.shape) if res else None
    cot = C.randn(643, *x.shape)
    ref = in_reference(x, r, relu, cot)
    hard = family in ("constant", "offset1e3", "one-constant-channel")
    rg = r.clone().to(DEV).requires_grad_() if res else None
    yg, xg, cap, run_backward = backward_capturing_dx(x, lambda t: ops.instance_norm(t, rg, relu, 1e-5), cot)
    check_probe(ops, yg, "instance_norm y")
    _, mean_g, rstd_g = yg.grad_fn.saved_tensors
    mean_g, rstd_g = mean_g.clone(), rstd_g.clone()
    run_backward()
    check_probe(ops, cap[0], "instance_norm dx")
    assert torch.equal(cap[0], xg.grad)
    assert bool(torch.isfinite(yg).all()) and bool(torch.isfinite(xg.grad).all()), "non-finite output or gradient"
    bounded(yg, ref["y"], BAR, "IN y", oracle=ref["y32"] if hard else None, floor=in_floor(family))
    # the saved statistics: the mean's error in units of the plane's own standard deviation (in_mean_unit), rstd relative
    xo, unit = x.reshape(6, -1), in_mean_unit(x, ref)
    bounded((mean_g.cpu().double() - ref["mean"]) / unit, torch.zeros(6), BAR, "IN saved mean (in sigmas)",
            oracle=(xo.mean(1).double() - ref["mean"]) / unit if hard else None, floor=1.0)
    bounded(rstd_g, ref["rstd"], BAR, "IN saved rstd",
            oracle=1.0 / torch.sqrt(xo.var(1, unbiased=False) + 1e-5) if hard else None)
    where = in_dx_where(family, relu, ref)
    if where is None or bool(where.any()):
        bounded(xg.grad, ref["dx"], BAR_IN_DX, "IN dx", oracle=ref["dx32"] if hard else None, where=where)
    if res:
        bounded(rg.grad, ref["dres"], BAR, "IN dres")


@pytest.mark.parametrize("family", IN_FAMILIES)
@pytest.mark.parametrize("H", [128, 256])
def test_instance_norm_relu_blur_down(ops, H, family):
    """The fused InstanceNorm + ReLU + Downsample (128^2 and 256^2 planes): z, dx, the saved statistics and the range probes
    against float64 on every input family (dx where it is defined, see in_dx_where; finite everywhere).  The probe of z is
    the maximum of relu(IN(x)) BEFORE the blur, so it bounds max |z| without being tight (check_probe, source_max); the probe
    of dx is tight."""
    x = in_input(family, H, H, seed=645)
    assert ops.in_relu_blurdown_ok(x.to(DEV))
    cot = C.randn(646, 2, 3, H // 2, H // 2)
    ref = in_reference(x, None, True, cot, down=True)
    hard = family in ("constant", "offset1e3", "one-constant-channel")
    zg, xg, cap, run_backward = backward_capturing_dx(x, ops.instance_norm_relu_blur_down, cot)
    check_probe(ops, zg, "instance_norm_relu_blur_down z", source_max=float(ref["xhat"].clamp(min=0).max()),
                slack=BAR if family == "constant" else 0.0)
    _, mean_g, rstd_g = zg.grad_fn.saved_tensors
    mean_g, rstd_g = mean_g.clone(), rstd_g.clone()
    run_backward()
    check_probe(ops, cap[0], "instance_norm_relu_blur_down dx")
    assert torch.equal(cap[0], xg.grad)
    assert bool(torch.isfinite(zg).all()) and bool(torch.isfinite(xg.grad).all()), "non-finite output or gradient"
    bounded(zg, ref["y"], BAR, "IN+ReLU+blur z", oracle=ref["y32"] if hard else None, floor=in_floor(family))
    xo, unit = x.reshape(6, -1), in_mean_unit(x, ref)
    bounded((mean_g.cpu().double() - ref["mean"]) / unit, torch.zeros(6), BAR, "IN+ReLU+blur saved mean (in sigmas)",
            oracle=(xo.mean(1).double() - ref["mean"]) / unit if hard else None, floor=1.0)
    bounded(rstd_g, ref["rstd"], BAR, "IN+ReLU+blur saved rstd",
            oracle=1.0 / torch.sqrt(xo.var(1, unbiased=False) + 1e-5) if hard else None)
    where = in_dx_where(family, True, ref)
    if where is None or bool(where.any()):
        bounded(xg.grad, ref["dx"], BAR_IN_DX, "IN+ReLU+blur dx", oracle=ref["dx32"] if hard else None, where=where)


# ================================================================================================= 5. Adam
# dfmir_adam_step launches df_grid(n, 256, 8192): one pass of the grid covers 8192 x 256 = 2 097 152 elements.  The arena
# below has 2 106 315 (odd; no parameter's size is a multiple of 4), so 9 163 elements are updated in a second pass.
ADAM_SHAPES = [(1031, 2039), (4099,), (7,)]
ADAM_N = sum(int(np.prod(s)) for s in ADAM_SHAPES)
ADAM_STEPS, ADAM_LR = 200, 2e-4
assert ADAM_N > 8192 * 256 and ADAM_N % 4 != 0


def adam_grad(t, A, B):
    """Gradient of step t (0-based): a rotating mix of two seeded fields whose scale grows by 1e3 over the run."""
    s = 1e-2 * 10.0 ** (3.0 * t / (ADAM_STEPS - 1))
    return (A * float(np.cos(0.37 * t)) + B * float(np.sin(0.37 * t))) * s


@functools.lru_cache(maxsize=None)
def adam_reference(betas):
    """float64 Adam and fp32 torch.optim.Adam (the oracle) over the ADAM_STEPS gradients, from the same fp32 start."""
    p0 = C.randn(651, ADAM_N) * 0.05
    A, B = C.randn(652, ADAM_N), C.randn(653, ADAM_N)
    ref = R.Adam(p0, ADAM_LR, betas)
    po = p0.clone().requires_grad_()
    opt = torch.optim.Adam([po], lr=ADAM_LR, betas=betas)
    for t in range(ADAM_STEPS):
        g = adam_grad(t, A, B)
        ref.step(g)
        po.grad = g
        opt.step()
    st = opt.state[po]
    return p0, A, B, ref, (po.detach(), st['exp_avg'], st['exp_avg_sq'])


def adam_compare(p0, p, m, v, ref, orc):
    po, mo, vo = orc
    bounded(p.cpu().double() - p0.double(), ref.p - p0.double(), BAR, "adam update p_t - p_0", oracle=po.double() - p0.double())
    bounded(m, ref.m, BAR, "adam exp_avg", oracle=mo)
    bounded(v, ref.v, BAR, "adam exp_avg_sq", oracle=vo)


@pytest.mark.parametrize("grad_scale", [1.0, 1.0 / 16], ids=["gs1", "gs1over16"])
def test_flat_adam_200_steps(ops, grad_scale):
    """FlatAdam (betas (0.5, 0.999), the training default) over 200 steps: the UPDATE p_t - p_0 and both moments, each
    relative to its own maximum, against float64 Adam.  With grad_scale = 1/16 the gradients arrive 16 x larger, so the
    reference is the same."""
    from dfmir_amd.optim import FlatAdam
    betas = (0.5, 0.999)
    p0, A, B, ref, orc = adam_reference(betas)
    ps, off = [], 0
    for s in ADAM_SHAPES:
        k = int(np.prod(s))
        ps.append(torch.nn.Parameter(p0[off:off + k].view(s).clone().to(DEV)))
        off += k
    opt = FlatAdam(ps, lr=ADAM_LR, betas=betas)
    opt.grad_scale = grad_scale
    Ag, Bg = A.to(DEV), B.to(DEV)
    for t in range(ADAM_STEPS):
        opt.zero_grad()
        opt.flat_g.copy_(adam_grad(t, Ag, Bg) / grad_scale)
        opt.step()
    assert ps[1].data_ptr() == opt.flat_p[int(np.prod(ADAM_SHAPES[0])):].data_ptr()
    adam_compare(p0, torch.cat([p.detach().reshape(-1) for p in ps]), opt.exp_avg, opt.exp_avg_sq, ref, orc)


@pytest.mark.parametrize("grad_scale", [1.0, 1.0 / 16], ids=["gs1", "gs1over16"])
def test_adam_step_200_steps(ops, grad_scale):
    """ops.adam_step itself with betas (0.9, 0.999) (torch's default: bc1 still matters after 40 steps, bc2 = 1 - 0.999^t
    grows from 1e-3 to 0.18 over the run), same arena, same comparisons."""
    betas = (0.9, 0.999)
    p0, A, B, ref, orc = adam_reference(betas)
    p = p0.clone().to(DEV)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    Ag, Bg = A.to(DEV), B.to(DEV)
    for t in range(ADAM_STEPS):
        g = adam_grad(t, Ag, Bg) / grad_scale
        ops.adam_step(p, g, m, v, ADAM_LR, betas[0], betas[1], 1e-8, t + 1, grad_scale)
    adam_compare(p0, p, m, v, ref, orc)


# ============================================================================================== 6. helpers
HELPER_SIZES = [1, 255, 257, (1 << 20) + 3]
MUL_SIZES = HELPER_SIZES + [8192 * 256 + 259]                    # mul_k: at most 8192 workgroups of 256 -> a second grid pass


@pytest.mark.parametrize("n", MUL_SIZES)
def test_mul_scale(ops, n):
    """ops.mul (mul_k, both gradients) and ops.scale: values and gradients against float64."""
    a, b, cot = C.randn(661, n), C.randn(662, n) * 3 + 1, C.randn(663, n)
    ag, bg = a.clone().to(DEV).requires_grad_(), b.clone().to(DEV).requires_grad_()
    y = ops.mul(ag, bg)
    (y * cot.to(DEV)).sum().backward()
    close(y, a.double() * b.double(), rtol=BAR, atol=0.0, what="mul")
    close(ag.grad, cot.double() * b.double(), rtol=BAR, atol=0.0, what="mul da")
    close(bg.grad, cot.double() * a.double(), rtol=BAR, atol=0.0, what="mul db")
    sg = a.clone().to(DEV).requires_grad_()
    z = ops.scale(sg, -2.5)
    (z * cot.to(DEV)).sum().backward()
    close(z, a.double() * -2.5, rtol=BAR, atol=0.0, what="scale")
    close(sg.grad, cot.double() * -2.5, rtol=BAR, atol=0.0, what="scale dx")


@pytest.mark.parametrize("offset", [0.0, 1e3], ids=["zero-mean", "offset1e3"])
@pytest.mark.parametrize("n", HELPER_SIZES)
def test_mean(ops, n, offset):
    """ops.mean (sum_scaled_k forward, fill_from_scalar_k backward): value and gradient against float64; with a common
    offset of 1e3 the fp32 sum runs at 1e3 x the magnitude of the signal (bound from plain fp32 torch on the same input)."""
    x = C.randn(664, n) + offset
    xg = x.clone().to(DEV).requires_grad_()
    y = ops.mean(xg)
    (y * 3.0).backward()
    bounded(y, x.double().mean(), BAR, "mean", oracle=x.mean() if offset else None)
    close(xg.grad, torch.full((n,), 3.0 / n, dtype=torch.float64), rtol=BAR, atol=0.0, what="mean dx")
