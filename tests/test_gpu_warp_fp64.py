"""ops.warp, ops.vecint_step and ops.resize_linear (dfmir_amd/csrc/warp.hip, warp_win.hip) against the plain float64
restatements of tests/ref64.py (checked on the CPU by tests/test_ref64.py), value and gradients, on every branch of their
launchers.  Run on the MI355X box:  python -m pytest tests/test_gpu_warp_fp64.py -m gpu -q ; the tests without the gpu mark
check the inputs (lattice distances, exclusion caps, the nearest ties, the chain's clearance, the resize bounds).  Shapes, input
builders and CPU evaluators live in tests/warp_cases.py, which the CPU module and scripts/warp_margins.py share.

Launcher branch -> test id.  "windowed" = W % 4 == 0 (tiles 8 x 8 x 32 / 64 x 32, windows 12 x 12 x 40 / 68 x 40, the grid
rounded up to 8 workgroups, win_tile's remap over the XCDs), "scalar" = the one-voxel-per-thread kernels.  Both are built on
the cell of dfmir_amd/csrc/lin_cell.h (lin_cell, lin_value, lin_flow_grad, lin_cw, lin_voxel_fwd / lin_voxel_bwd).
    lin_cell's guard / win_prologue's clamp   test_warp_far_and_non_finite_flow[*]: NaN, inf and +-1e30 displacements
  dfmir_warp3d_fwd / dfmir_warp2d_fwd
    warp_win_fwd_k<3|2>, mode 0               test_warp_vs_restatement[3d-win-* | 2d-win-*]: tile counts 1 (7 of 8 workgroups idle),
                                              4, 6 (3 z tiles), 8 ragged, 12 with a batch, 27; one voxel short / past per axis
      lin_voxel_fwd<*, int> inside it         ... the lattice and far families (far: almost every voxel)
      add_identity = 1                        test_vecint_step_vs_restatement[*-win-*], test_vecint_seven_steps[*-win-*]
    warp_fwd_k<3|2>, mode 0                   test_warp_vs_restatement[3d-sca-* | 2d-sca-*] (255 / 256 / 258 voxels: one block)
      add_identity = 1                        test_vecint_step_vs_restatement[*-sca-*], test_vecint_seven_steps[*-sca-*]
    warp_fwd_k<3|2>, mode 1                   test_warp_nearest_vs_restatement[*] (every shape: mode 1 never takes the window),
                                              test_warp_nearest_ties_go_to_the_even_voxel
      mode 1 with add_identity = 1            unreachable: ops passes add_identity only from VecIntStepFn, with mode 0
    win_eligible refusing a W % 4 == 0 shape  a volume of 2^31 bytes or 2^30 tiles: not run; test_ref64.py pins the host logic
  dfmir_warp3d_bwd / dfmir_warp2d_bwd
    warp_win_bwd_k<3|2>, dsrc == NULL         test_warp_vs_restatement[*-win-*] (the flow-only backward of WarpFn)
    warp_win_bwd_k, dsrc, LDS + atomics       test_warp_vs_restatement[*-win-*] (ops._warp_bwd into a zeroed buffer)
    warp_win_bwd_k, need_own                  test_vecint_step_vs_restatement[*-win-*] (ops._warp_bwd(dout, v, v, zeros, None, 1, 1))
      lin_voxel_bwd<*, int> inside it         ... the lattice / far families, vi-6
    warp_bwd_k<3|2>, dsrc == NULL             test_warp_vs_restatement[*-sca-*] (flow only)
    warp_bwd_k<3|2>, dsrc, dflow              test_warp_vs_restatement[*-sca-*] (src and flow require gradients)
    ..., dsrc, dflow == NULL                  test_warp_vs_restatement[*-sca-*] (src alone requires a gradient)
    ..., add_identity = flow_into_src = 1     test_vecint_step_vs_restatement[*-sca-*], test_vecint_seven_steps[*-sca-*]
  dfmir_warp_bwd_own
    warp_win_bwd_own_k + warp_win_gather_k    test_warp_vs_restatement[*-win-*] (src.requires_grad), test_warp_dsrc_scales_by_powers_of_two
    warp_win_slow_k, plain                    ... the lattice / far families
    own term (add_identity, flow_into_src)    test_vecint_step_vs_restatement[*-win-*], test_vecint_seven_steps[*-win-*]
    warp_win_slow_k with the own term         ... the lattice family and vi-6 (the own cell leaves the window)
    dflow == NULL without flow_into_src       test_warp_vs_restatement[*-win-*] (src alone requires a gradient: phase A and the d(flow)
                                              stores are skipped, warp_win_slow_k hands lin_voxel_bwd a null dflow)
  dfmir_resize_fwd
    resize_rows_fwd_k                         test_resize_vs_restatement[6x10x12-12x20x24], [12x20x24-6x10x12], [1x8-1x16], [5x1x8-5x1x16]
      its second grid pass (> 20480 rows)     test_resize_vs_restatement[24x30x4-48x75x8]
    resize_fwd_v4_k<unsigned>                 test_resize_vs_restatement[3x5-24x40] (Wi % 4), [2x2x1-4x4x8], [5x6x516-5x6x1032] (Wi > 512)
    resize_fwd_v4_k<long long>                unreachable here: 2^34 outputs
    resize_fwd_k                              test_resize_vs_restatement[7x9x13-3x4x6], [9x37-23x50], [4x300-4x1], [5x8-5x18], [5x8-5x19]; its 64-bit decode needs
                                              2^31 outputs
    a misaligned x or y                       not run (the launchers guard it; no misaligned input is added)
  dfmir_resize_bwd_sep
    resize_w_bwd_tab_k                        [6x10x12-12x20x24], [12x20x24-6x10x12], [7x9x13-3x4x6], [9x37-23x50], [1x8-1x16], [5x1x8-5x1x16],
                                              [24x30x4-48x75x8] (at most 4 non-zero candidates per input), [5x8-5x18] (2 / scale = 4.86: 5
                                              candidates, the most the host rule lets through; the sixth slot of the table is never filled)
    resize_w_bwd4_k<unsigned>                 [5x8-5x19] (2 / scale = 5.14: the first ratio the table refuses), [3x8-24x40] (13 candidates),
                                              [4x300-4x1] (scale 0), [5x6x516-5x6x1032]
    resize_axis_bwd_k<1> as the W pass        [3x5-24x40], [2x2x1-4x4x8] (Wi = 1: scale 0)
    resize_axis_bwd_k<4> (H, D passes)        every case with Wi % 4 == 0
    resize_axis_bwd_k<1> (H, D passes)        every other case
    the <long long> forms of the three        unreachable here: 2^32 threads
  dfmir_resize_bwd (exported; ResizeFn never takes it: dfmir_resize_bwd_ws_floats is positive for every valid size)
    resize_bwd_k, windows < 8 candidates      test_resize_one_pass_adjoint[7x9x13-3x4x6]
    resize_bwd_k, the general loop            test_resize_one_pass_adjoint[3x8-24x40]; its 64-bit decode needs 2^31 inputs

Inputs.  src is seeded noise in [-2, 2] of the case's channel count, the upstream gradient seeded noise in [-1, 1].  Flows:
`lattice` (tests/test_invcons.py) k + f, k integer-valued in [-3, 3], f in [0.05, 0.95]: every sample point at least 0.05 from
a cell boundary, fast and slow voxels mixed in a tile, many taps outside; `far` the same with k in [-40, 40]; `smooth`
sinusoids of amplitude 2 and wavelength >= 12; `bulk` = smooth + (5.3, -4.6, 9.2) voxels (2-D: the last two).  d(flow) is
piecewise constant in the sample position, so on smooth and bulk it leaves out the voxels with a sample coordinate within
EXCLUDE_WITHIN of an integer, at most EXCLUDE_CAP of a case (asserted below, on the CPU); value and d(src) are continuous and
compared in full.  VecInt: `vi-0.25`, `vi-1`, `vi-6` = smooth at those amplitudes, and lattice; dv carries the same d(flow)
term and leaves out the same voxels.  The seven chained steps run behind ops.scale(v, 1 / 128) on `chain` = 0.5 + smooth at
amplitude 0.3: a kink met at one step spreads through the later ones and a velocity that crosses zero puts x + v / 128 right
beside the integer x, so no exclusion would do; with every component in [0.2, 0.8] each step's displacement stays inside
(0.001, 0.5) and no sample coordinate of any step comes within CHAIN_CLEAR = 1e-3 of an integer (asserted on the CPU) -- fp32
and float64 take the same cell everywhere.  That field never leaves its own cell, so `chain-neg` runs beside it: 3 + smooth
at amplitude 0.4, the sign alternating over the channels (-, +, -): magnitudes in [2.6, 3.4] halve to (1.3, 1.7), (0.65, 0.85),
(0.32, 0.43), ... at the steps before the last, all clear of the integers by the same CHAIN_CLEAR (asserted likewise); the last
steps sample one and two cells away, on either side, and leave the volume at both faces.  Nearest mode: lattice with f in
[0.05, 0.45] or [0.55, 0.95] (no tie), and a case with every sample point on k + 0.5 against a hand-written table.

Tolerances (profiles/warp_margins.txt; the rule of tests/test_compose.py).  Every comparison with a restatement is bounded by
FACTOR = 4 x the error of the same definition evaluated by torch in fp32 on the CPU against float64, on these inputs: the
maximum over the case set, per family and quantity, each as relative 2-norm and as max-abs over max.  scripts/warp_margins.py
measures them and the kernels' own errors beside them; no bound comes from those, and the fixed-point d(src) paths get no
allowance of their own.  Resize: the fp32 error grows with the width (scale * o is rounded),
so the bound is per case max(16 x 2^-24, 4 x error of fp32 F.interpolate on the CPU against the restatement) of the
maximum, for the value and, against autograd of the same, the adjoint; a case whose bound exceeds BAR = 1e-4 is refused.
The resize inputs are plain noise, except beyond RF_MAXW = 512 input columns (resize_input says why).
All comparisons go to tests.test_gpu_ops.MARGINS."""
import os

import pytest
import torch
import torch.nn.functional as F

from tests import ref64 as R
from tests import test_invcons as T
from tests.test_gpu_ops import MARGINS
from tests.warp_cases import (BULK, CHAIN_FAMILIES, CHAIN_SHAPES, CHAIN_STEPS, SHAPES, SLOW_TAPS_INSIDE, VI_AMP, VI_FAMILIES,  # noqa: F401
                              VI_SHAPES, WARP_FAMILIES, _seed, flow_field, nearest_ties, noise, rel_errors, vecint_eval, warp_eval)

DEV = "cuda"
FACTOR = 4.0
BAR = 1e-4
EXCLUDE_WITHIN, EXCLUDE_CAP = T.EXCLUDE_WITHIN, T.EXCLUDE_CAP
CHAIN_CLEAR = 1e-3
F32 = torch.float32

# profiles/warp_margins.txt, rows "max" of the fp32 CPU columns.
# ops.warp: (value 2-norm, value max, d(src) 2-norm, d(src) max, d(flow) 2-norm, d(flow) max)
FP32_WARP = {"lattice": (3.45e-06, 9.20e-06, 3.44e-06, 4.92e-06, 2.44e-06, 6.29e-06),
             "smooth": (3.41e-06, 1.12e-05, 3.40e-06, 4.34e-06, 2.38e-06, 5.15e-06),
             "bulk": (3.37e-06, 9.00e-06, 3.38e-06, 5.26e-06, 2.42e-06, 4.28e-06),
             "far": (3.62e-06, 1.15e-05, 3.62e-06, 4.23e-06, 2.58e-06, 4.26e-06)}
# ops.vecint_step: (value 2-norm, value max, dv 2-norm, dv max)
FP32_VECINT = {"vi-0.25": (3.86e-07, 2.96e-06, 1.38e-06, 5.46e-06), "vi-1": (3.29e-07, 3.06e-06, 1.46e-06, 5.25e-06),
               "vi-6": (4.15e-07, 2.25e-06, 1.56e-06, 1.80e-06), "lattice": (1.69e-06, 5.33e-06, 2.37e-06, 5.42e-06)}
# seven chained steps behind the 1 / 128 scale: (value 2-norm, value max, dv 2-norm, dv max)
FP32_CHAIN = {"chain": (1.93e-07, 2.02e-06, 1.66e-06, 3.37e-06), "chain-neg": (7.75e-08, 3.53e-07, 1.49e-06, 2.52e-06)}
BOUND_WARP = {k: tuple(FACTOR * e for e in v) for k, v in FP32_WARP.items()}
BOUND_VECINT = {k: tuple(FACTOR * e for e in v) for k, v in FP32_VECINT.items()}
BOUND_CHAIN = {k: tuple(FACTOR * e for e in v) for k, v in FP32_CHAIN.items()}

# resize: (input spatial size, output spatial size)
RESIZE_CASES = [((6, 10, 12), (12, 20, 24)), ((12, 20, 24), (6, 10, 12)), ((7, 9, 13), (3, 4, 6)), ((9, 37), (23, 50)),
                ((3, 8), (24, 40)), ((3, 5), (24, 40)), ((5, 8), (5, 18)), ((5, 8), (5, 19)), ((4, 300), (4, 1)), ((1, 8), (1, 16)), ((5, 1, 8), (5, 1, 16)),
                ((2, 2, 1), (4, 4, 8)), ((5, 6, 516), (5, 6, 1032)), ((24, 30, 4), (48, 75, 8))]
ONE_PASS_CASES = [((7, 9, 13), (3, 4, 6)), ((3, 8), (24, 40))]
RESIZE_MULTS = (0.5, 2.0, -1.5)
RESIZE_FLOOR = 16.0 * 2.0 ** -24


def _kind(shape):
    return "%dd-%s" % (len(shape) - 2, "win" if shape[-1] % 4 == 0 else "sca")


def _id(shape):
    return _kind(shape) + "-" + T._id(shape)


def _rid(case):
    return "-".join("x".join(str(n) for n in sp) for sp in case)


def _test_id():
    return os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]


# ------------------------------------------------------------------------------------------ cases
_REF = {}


def warp_case(shape, family):
    """(src, flow, g, (out64, dsrc64, dflow64), keep) of a warp case, computed once and shared"""
    key = ("warp", shape, family)
    if key not in _REF:
        seed = _seed(shape, family)
        src, flow, g = noise(seed + 5, shape, 2.0), flow_field(shape, family), noise(seed + 6, shape, 1.0)
        keep = T.du_keep(flow) if family in ("smooth", "bulk") else None
        _REF[key] = (src, flow, g, warp_eval(src, flow, g), keep)
    return _REF[key]


def vecint_case(shape, family):
    """(v, g, (out64, dv64), keep) of a VecInt case"""
    key = ("vecint", shape, family)
    if key not in _REF:
        v, g = flow_field(shape, family), noise(_seed(shape, family) + 6, shape, 1.0)
        _REF[key] = (v, g, vecint_eval(v, g), None if family == "lattice" else T.du_keep(v))
    return _REF[key]


def chain_case(shape, family="chain"):
    """(v, g, (out64, dv64), the sample points of the seven float64 steps)"""
    key = (family, shape)
    if key not in _REF:
        v, g = flow_field(shape, family), noise(_seed(shape, family) + 6, shape, 1.0)
        coords = []
        _REF[key] = (v, g, vecint_eval(v, g, steps=CHAIN_STEPS, pre=1.0 / 128, coords=coords), coords)
    return _REF[key]


def warp_errors(got, ref, keep):
    return rel_errors(got[0], ref[0]) + rel_errors(got[1], ref[1]) + rel_errors(got[2], ref[2], keep)


def vecint_errors(got, ref, keep):
    return rel_errors(got[0], ref[0]) + rel_errors(got[1], ref[1], keep)


def resize_input(case):
    """(x fp32 [2, 3, *in], cotangent fp32 [2, 3, *out]): noise in [-2, 2] and [-1, 1].  Beyond 512 input columns (the widest the
    row and table kernels take) fp32 rounds scale = (in - 1) / (out - 1) by 3e-8 of itself, which moves the sample point of
    output column o by o times that, up to 3e-5 of a voxel at the far end: the value by that times the local slope, and an
    input's gradient by that times the cotangent wherever its candidates do not pair off left and right.  For plain noise
    4 x the fp32 yardstick then lies above BAR.  There, and only there, x is noise on an offset, [1.75, 2.25] (an eighth of
    the slope over the maximum), and the cotangent is [0.9, 1.1] times a ramp that falls from 1 at column 0 to 1 / 4 at the
    last, so that o times the cotangent peaks at a third of what a flat one reaches.  A wrong weight or index still moves
    either result by a multiple of the noise."""
    i = RESIZE_CASES.index(case)
    if case[0][-1] > 512:
        ramp = 1.0 - 0.75 * torch.arange(case[1][-1], dtype=torch.float32) / (case[1][-1] - 1)
        return 2.0 + noise(5000 + 7 * i, (2, 3) + case[0], 0.25), (1.0 + noise(5001 + 7 * i, (2, 3) + case[1], 0.1)) * ramp
    return noise(5000 + 7 * i, (2, 3) + case[0], 2.0), noise(5001 + 7 * i, (2, 3) + case[1], 1.0)


def resize_eval(x, cot, out_sp, mult, how):
    """(y, dx) on the CPU: how = 'ref' the float64 restatement, 'f32' F.interpolate(align_corners=True) in fp32"""
    a = x.detach().cpu().to(torch.float64 if how == "ref" else F32).requires_grad_()
    if how == "ref":
        y = R.resize_linear(a, out_sp, mult)
    else:
        y = mult * F.interpolate(a, size=out_sp, mode="trilinear" if len(out_sp) == 3 else "bilinear", align_corners=True)
    (y * cot.to(y.dtype)).sum().backward()
    return y.detach(), a.grad


def resize_case(case, mult):
    """(x, cot, (y64, dx64), (bound of y, bound of dx)): max(floor, FACTOR x the fp32 CPU error), of the maximum"""
    key = ("resize", case, mult)
    if key not in _REF:
        x, cot = resize_input(case)
        ref, f32 = resize_eval(x, cot, case[1], mult, "ref"), resize_eval(x, cot, case[1], mult, "f32")
        _REF[key] = (x, cot, ref, tuple(max(RESIZE_FLOOR, FACTOR * rel_errors(f32[k], ref[k])[1]) for k in (0, 1)))
    return _REF[key]


# ------------------------------------------------------------------------------------------ CPU tier: the inputs
def _sample_points(flow):
    return T._grid(flow.shape[2:], torch.float64)[None] + flow.double()


def test_lattice_families_keep_their_distance_and_many_points_leave_the_volume():
    for shape in SHAPES:
        for family in ("lattice", "far", "nearest"):
            f = _sample_points(flow_field(shape, family))
            assert float((f - torch.round(f)).abs().min()) >= 0.05 - 1e-5, (shape, family)
            if family == "nearest":                                   # ... and from the ties
                assert float((f - torch.floor(f) - 0.5).abs().min()) >= 0.05 - 1e-5, shape
            vol = torch.tensor(shape[2:], dtype=torch.float64).reshape((1, -1) + (1,) * (len(shape) - 2))
            outside = float(((f < 0) | (f > vol - 1)).any(1).double().mean())
            assert outside > 0.02, (shape, family, outside)
    for shape in VI_SHAPES:
        assert torch.equal(flow_field(shape, "lattice"), vecint_case(shape, "lattice")[0])


def test_smooth_families_stay_under_the_exclusion_cap():
    worst = 0.0
    for shape in SHAPES:
        for family in ("smooth", "bulk") + (("vi-0.25", "vi-1", "vi-6") if shape in VI_SHAPES else ()):
            u = flow_field(shape, family)
            nd = len(shape) - 2
            off = torch.tensor(BULK[-nd:]).reshape((1, nd) + (1,) * nd) if family == "bulk" else 0.0
            amp = VI_AMP.get(family, 2.0)
            assert float((u - off).abs().max()) <= amp + 1e-5, (shape, family)
            left_out = 1.0 - float(T.du_keep(u).double().mean())
            worst = max(worst, left_out)
            assert left_out <= EXCLUDE_CAP, (shape, family, left_out)
    print("largest share left out of a d(flow) comparison: %.4f" % worst)


def test_chain_sample_points_clear_every_cell_boundary():
    for shape in CHAIN_SHAPES:
        for family in CHAIN_FAMILIES:
            v, _, (out, _), coords = chain_case(shape, family)
            lo, hi = (0.2, 0.8) if family == "chain" else (2.6, 3.4)
            assert len(coords) == CHAIN_STEPS and lo - 1e-6 <= float(v.abs().min()) and float(v.abs().max()) <= hi + 1e-6
            assert bool((v > 0).all()) == (family == "chain") and bool((v[:, 0] < 0).all()) == (family == "chain-neg")
            clear = min(float((f - torch.round(f)).abs().min()) for f in coords)
            assert clear > CHAIN_CLEAR, (shape, family, clear)
            assert float(out.abs().max()) > 0.5                       # the integrated field is a real displacement
            if family == "chain-neg":                                 # the last step samples beyond the neighbouring cell
                assert float((coords[-1] - T._grid(v.shape[2:], torch.float64)[None]).abs().max()) > 1.0


def test_nearest_tie_table_is_what_the_restatement_computes():
    for nd in (2, 3):
        src, flow, want = nearest_ties(nd)
        f = _sample_points(flow)
        assert bool(((f - torch.floor(f)) == 0.5).all())
        for dtype in (torch.float64, F32):
            assert torch.equal(R.warp(src, flow, mode="nearest", dtype=dtype).float(), want)
        assert float(want.abs().max()) > 0.0 and float((want == 0).float().mean()) > 0.3


@pytest.mark.parametrize("case", RESIZE_CASES, ids=_rid)
def test_resize_bounds_test_something(case):
    for mult in RESIZE_MULTS:
        x, cot, ref, bounds = resize_case(case, mult)
        assert ref[0].shape[2:] == case[1] and float(ref[0].abs().max()) > 0.0 and float(ref[1].abs().max()) > 0.0
        assert max(bounds) <= BAR, (case, mult, bounds)


def test_fp32_constants_equal_the_rows_of_the_margins_file():
    """The constants above against the rows "max" of the fp32 CPU columns of profiles/warp_margins.txt as committed (the file
    itself is what scripts/warp_margins.py writes; nothing is recomputed here)."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "warp_margins.txt")
    rows = {}
    for line in open(path):
        parts = line.split("|")
        head = parts[0].split()
        if len(parts) >= 2 and len(head) == 3 and head[1] == "max":
            rows[(head[0], head[2])] = tuple(float(x) for x in parts[1].split())
    for fam, want in FP32_WARP.items():
        assert rows[("warp", fam)] == want, fam
    for fam, want in FP32_VECINT.items():
        assert rows[("vecint", fam)] == want, fam
    for fam, want in FP32_CHAIN.items():
        assert rows[("chain", fam)] == want, fam
    assert all(e > 0.0 for d in (FP32_WARP, FP32_VECINT, FP32_CHAIN) for v in d.values() for e in v)


# ------------------------------------------------------------------------------------------ GPU tier
def _check(what, errs, bounds, names):
    print("%s: %s" % (what, "  ".join("%s %.3e (%.1e)" % (n, e, b) for n, e, b in zip(names, errs, bounds))))
    for n, e, b in zip(names, errs, bounds):
        MARGINS.append((_test_id(), "%s %s" % (what, n), e, b))
    assert all(e <= b for e, b in zip(errs, bounds)), (what, [(n, e, b) for n, e, b in zip(names, errs, bounds) if not e <= b])


WARP_NAMES = ("value l2", "value max", "dsrc l2", "dsrc max", "dflow l2", "dflow max")
VI_NAMES = ("value l2", "value max", "dv l2", "dv max")


def gpu_warp(src, flow, g, want_src=True, mode="bilinear", want_flow=True):
    """(out, d(src) or None, d(flow) or None) of ops.warp"""
    from dfmir_amd import ops
    a, b = src.to(DEV).requires_grad_(want_src), flow.to(DEV).requires_grad_(want_flow)
    out = ops.warp(a, b, mode)
    out.backward(g.to(DEV))
    torch.cuda.synchronize()
    assert want_flow or b.grad is None
    return out.detach().cpu(), (a.grad.cpu() if want_src else None), (b.grad.cpu() if want_flow else None)


def gpu_warp_atomic(src, flow, g, own=0):
    """(d(src), d(flow) or None) of ops._warp_bwd into a zeroed buffer; own = 1: the VecInt form (flow's gradient into d(src))"""
    from dfmir_amd import ops
    s, f, d = src.to(DEV), flow.to(DEV), g.to(DEV)
    dsrc = torch.zeros_like(s)
    dflow = None if own else torch.empty_like(f)
    ops._warp_bwd(d, s, s if own else f, dsrc, dflow, own, own)
    torch.cuda.synchronize()
    return dsrc.cpu(), None if own else dflow.cpu()


def gpu_vecint(v, g, steps=1, pre=None):
    from dfmir_amd import ops
    a = v.to(DEV).requires_grad_()
    x = a if pre is None else ops.scale(a, pre)
    for _ in range(steps):
        x = ops.vecint_step(x)
    x.backward(g.to(DEV))
    torch.cuda.synchronize()
    return x.detach().cpu(), a.grad.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_warp_vs_restatement(shape):
    """Value, d(src) and d(flow) through every backward form (both gradients, flow only, src only, on the windowed shapes the
    LDS-atomic kernel too), and what must repeat itself bit for bit: d(flow) everywhere, d(src) of the owner-gather path on
    lattice (SLOW_TAPS_INSIDE: on smooth), with or without d(flow) -- the scalar shapes' d(src) is a sum of float atomics."""
    windowed = shape[-1] % 4 == 0
    for family in WARP_FAMILIES:
        src, flow, g, ref, keep = warp_case(shape, family)
        what = "%s [%s]" % (_id(shape), family)
        full = gpu_warp(src, flow, g)
        assert all(bool(torch.isfinite(t).all()) for t in full), what
        _check(what + (" owner-gather" if windowed else " scalar"), warp_errors(full, ref, keep), BOUND_WARP[family], WARP_NAMES)
        only = gpu_warp(src, flow, g, want_src=False)
        assert torch.equal(only[0], full[0])
        _check(what + " flow only", rel_errors(only[2], ref[2], keep), BOUND_WARP[family][4:], WARP_NAMES[4:])
        if windowed:
            dsrc, dflow = gpu_warp_atomic(src, flow, g)
            _check(what + " LDS atomics", rel_errors(dsrc, ref[1]) + rel_errors(dflow, ref[2], keep), BOUND_WARP[family][2:],
                   WARP_NAMES[2:])
        alone = gpu_warp(src, flow, g, want_flow=False)                # d(src) alone: dflow == NULL beside dsrc
        assert torch.equal(alone[0], full[0]) and bool(torch.isfinite(alone[1]).all()), what
        _check(what + " src only", rel_errors(alone[1], ref[1]), BOUND_WARP[family][2:4], WARP_NAMES[2:4])
        again = gpu_warp(src, flow, g)
        assert torch.equal(again[0], full[0]) and torch.equal(again[2], full[2]), what
        assert torch.equal(gpu_warp(src, flow, g, want_src=False)[2], only[2]), what
        if windowed and family == ("smooth" if shape in SLOW_TAPS_INSIDE else "lattice"):
            assert torch.equal(again[1], full[1]), what + ": d(src) of the owner-gather path must repeat itself"
            assert torch.equal(alone[1], full[1]), what + ": d(src) alone must be the d(src) of the full backward"


@pytest.mark.gpu
@pytest.mark.parametrize("shape", VI_SHAPES, ids=_id)
def test_vecint_step_vs_restatement(shape):
    windowed = shape[-1] % 4 == 0
    for family in VI_FAMILIES:
        v, g, ref, keep = vecint_case(shape, family)
        what = "vecint %s [%s]" % (_id(shape), family)
        got = gpu_vecint(v, g)
        assert all(bool(torch.isfinite(t).all()) for t in got), what
        _check(what, vecint_errors(got, ref, keep), BOUND_VECINT[family], VI_NAMES)
        if windowed:
            dv, _ = gpu_warp_atomic(v, v, g, own=1)
            _check(what + " LDS atomics", rel_errors(dv, ref[1], keep), BOUND_VECINT[family][2:], VI_NAMES[2:])
            if family != "lattice" and family != "vi-6":            # no voxel on the slow list: fixed-point sums alone
                assert torch.equal(gpu_vecint(v, g)[1], got[1]), what


@pytest.mark.gpu
@pytest.mark.parametrize("shape", CHAIN_SHAPES, ids=_id)
def test_vecint_seven_steps(shape):
    for family in CHAIN_FAMILIES:
        v, g, ref, _ = chain_case(shape, family)
        got = gpu_vecint(v, g, steps=CHAIN_STEPS, pre=1.0 / 128)
        assert all(bool(torch.isfinite(t).all()) for t in got), family
        _check("7 steps %s [%s]" % (_id(shape), family), vecint_errors(got, ref, None), BOUND_CHAIN[family], VI_NAMES)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_warp_nearest_vs_restatement(shape):
    from dfmir_amd._lib import DfmirHipError
    from dfmir_amd import ops
    seed = _seed(shape, "nearest")
    src, flow, g = noise(seed + 5, shape, 2.0), flow_field(shape, "nearest"), noise(seed + 6, shape, 1.0)
    want = R.warp(src, flow, mode="nearest").float()
    assert float((want == 0).float().mean()) > 0.02 and float(want.abs().max()) > 0.0
    out, _, dflow = gpu_warp(src, flow, g, want_src=False, mode="nearest")
    assert torch.equal(out, want)
    assert dflow.shape == flow.shape and float(dflow.abs().max()) == 0.0
    a = src.to(DEV).requires_grad_()
    out = ops.warp(a, flow.to(DEV), "nearest")
    with pytest.raises(DfmirHipError, match="nearest"):
        out.backward(g.to(DEV))


@pytest.mark.gpu
@pytest.mark.parametrize("nd", [2, 3], ids=["2d", "3d"])
def test_warp_nearest_ties_go_to_the_even_voxel(nd):
    src, flow, want = nearest_ties(nd)
    assert torch.equal(gpu_warp(src, flow, torch.ones_like(src), want_src=False, mode="nearest")[0], want)


def _shifted(src, s):
    """src(x + s), 0 where x + s leaves the volume; s integers"""
    out = src
    for a, sa in enumerate(s):
        ax, n = 2 + a, src.shape[2 + a]
        idx = torch.arange(n) + sa
        ok = ((idx >= 0) & (idx < n)).to(src.dtype).reshape([-1 if d == ax else 1 for d in range(src.dim())])
        out = out.index_select(ax, idx.clamp(0, n - 1)) * ok
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 3, 8, 9, 36), (1, 3, 7, 9, 13), (1, 2, 65, 36), (1, 3, 17, 23)], ids=_id)
def test_warp_exact_identities(shape):
    nd = len(shape) - 2
    src, g = noise(91, shape, 2.0), noise(92, shape, 1.0)
    fs = (shape[0], nd) + shape[2:]
    assert torch.equal(gpu_warp(src, torch.zeros(fs), g)[0], src)
    for s in ((1, -2, 3), (-3, 0, -1), (0, 5, -11)):
        s = s[-nd:]
        flow = torch.tensor(s, dtype=F32).reshape((1, nd) + (1,) * nd).expand(fs).contiguous()
        want = _shifted(src, s)
        assert float(want.abs().max()) > 0.0 and bool((want == 0).any())
        assert torch.equal(gpu_warp(src, flow, g)[0], want), s
    for far in (1e6, -1e6):
        for axis in range(nd):
            flow = noise(93, fs, 1.0)
            flow[:, axis] += far
            for want_src in (True, False):
                out, dsrc, dflow = gpu_warp(src, flow, g, want_src=want_src)
                assert float(out.abs().max()) == 0.0 and float(dflow.abs().max()) == 0.0, (far, axis)
                assert dsrc is None or float(dsrc.abs().max()) == 0.0, (far, axis)


FAR_VALUES = (float("nan"), float("inf"), 1e30, -1e30)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 2, 8, 8, 32), (1, 2, 5, 6, 9), (1, 2, 64, 32), (1, 2, 7, 9)], ids=_id)
def test_warp_far_and_non_finite_flow(shape):
    """A smooth flow with twelve voxels overwritten, one component each, by NaN, +inf, +1e30 and -1e30: the displacements
    that no int holds.  From the zero-padding definition: a NaN or infinite coordinate has NaN weights, so the output
    there is NaN; at +-1e30 the weights are 0 and 1 and every corner lies outside, so the output is exactly 0; no other
    output voxel reads the flow of these twelve, so the rest stays within the smooth bound of the float64 restatement of
    the untouched flow; d(flow) is finite wherever the flow is.  d(src) is finite everywhere: a voxel with no corner inside
    the volume scatters to no cell, and the guarded cell gives these twelve none (the unguarded convert took NaN to cell 0,
    whose NaN weights then reached d(src); autograd through the restatement yields NaN there too, from 0 x NaN, so d(src)
    is not compared with it).  Both backward forms run (with and without d(src)), and on the windowed shapes the LDS-atomic
    kernel.  One windowed tile and one scalar block per dimension."""
    nd = len(shape) - 2
    seed = 9100 + sum(shape)
    src, g, flow0 = noise(seed, shape, 2.0), noise(seed + 1, shape, 1.0), flow_field(shape, "smooth", seed + 2)
    vox = flow0[0, 0].numel()
    flow = flow0.clone()
    touched = torch.zeros(shape[2:], dtype=torch.bool)
    for i in range(12):
        at = (i * 7919 + 3) % vox
        assert not bool(touched.view(-1)[at])
        touched.view(-1)[at] = True
        flow[0, i % nd].view(-1)[at] = FAR_VALUES[i % 4]
    bad = ~torch.isfinite(flow).all(1, keepdim=True)                   # NaN and inf voxels
    far = touched[None, None] & ~bad                                   # +-1e30
    assert int(bad.sum()) == 6 and int(far.sum()) == 6
    ref = R.warp(src.double(), flow0.double())
    rest = ~touched[None, None].expand_as(src)
    for want_src in (True, False):
        out, dsrc, dflow = gpu_warp(src, flow, g, want_src=want_src)
        what = "far flow %s%s" % (_id(shape), "" if want_src else " flow only")
        assert bool(torch.isnan(out[bad.expand_as(out)]).all()), what
        assert bool((out[far.expand_as(out)] == 0).all()), what
        _check(what, rel_errors(torch.where(rest, out, torch.zeros(())), ref, rest.double()), BOUND_WARP["smooth"][:2],
               WARP_NAMES[:2])
        assert bool(torch.isfinite(dflow[(~bad).expand_as(dflow)]).all()), what
        assert dsrc is None or bool(torch.isfinite(dsrc).all()), what
    if shape[-1] % 4 == 0:
        dsrc, dflow = gpu_warp_atomic(src, flow, g)
        assert bool(torch.isfinite(dsrc).all()) and bool(torch.isfinite(dflow[(~bad).expand_as(dflow)]).all()), shape


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 3, 8, 9, 36), (2, 2, 9, 11)], ids=_id)
def test_warp_non_contiguous_inputs_give_the_bits_of_their_copies(shape):
    from dfmir_amd import ops
    nd = len(shape) - 2
    src, flow, g, ref, _ = warp_case(shape, "lattice")
    want = gpu_warp(src, flow, g)
    big_s = torch.zeros((shape[0], 2 * shape[1]) + shape[2:], device=DEV)
    big_f = torch.zeros((shape[0], 2 * nd) + shape[2:], device=DEV)
    big_s[:, ::2], big_f[:, 1::2] = src.to(DEV), flow.to(DEV)
    a, b = big_s[:, ::2].requires_grad_(), big_f[:, 1::2].requires_grad_()
    assert not a.is_contiguous() and not b.is_contiguous()
    out = ops.warp(a, b)
    ga, gb = torch.autograd.grad(out, (a, b), g.to(DEV))
    assert torch.equal(out.detach().cpu(), want[0]) and torch.equal(gb.cpu(), want[2])
    if shape[-1] % 4 == 0:
        assert torch.equal(ga.cpu(), want[1])
    else:           # float atomics: no two runs need agree to the bit, so the copy is no yardstick; the restatement is
        _check("non-contiguous %s" % _id(shape), rel_errors(ga, ref[1]), BOUND_WARP["lattice"][2:4], WARP_NAMES[2:4])
    if shape[1] == nd:
        v, gv = flow_field(shape, "vi-1"), g
        big_f[:, 1::2] = v.to(DEV)
        c = big_f[:, 1::2].requires_grad_()
        y = ops.vecint_step(c)
        assert torch.equal(y.detach().cpu(), gpu_vecint(v, gv)[0])


@pytest.mark.gpu
def test_warp_dsrc_scales_by_powers_of_two():
    """dout times 2^40 and 2^-40: d(src) of the owner-gather path and d(flow) are the unscaled results times that factor, bit
    for bit -- the fixed-point scale is a power of two taken from the tile's sum of |g| (the +-90 clamp is far away)."""
    shape = (1, 3, 9, 9, 36)
    src, flow, g, _, _ = warp_case(shape, "lattice")
    base = gpu_warp(src, flow, g)
    for k in (40, -40):
        got = gpu_warp(src, flow, g * 2.0 ** k)
        assert torch.equal(got[1], base[1] * 2.0 ** k) and torch.equal(got[2], base[2] * 2.0 ** k), k
    v, gv, _, _ = vecint_case(shape, "vi-1")
    base = gpu_vecint(v, gv)
    for k in (40, -40):
        assert torch.equal(gpu_vecint(v, gv * 2.0 ** k)[1], base[1] * 2.0 ** k), k


def gpu_resize(x, cot, out_sp, mult):
    from dfmir_amd import ops
    a = x.to(DEV).requires_grad_()
    y = ops.resize_linear(a, out_sp, mult)
    y.backward(cot.to(DEV))
    torch.cuda.synchronize()
    return y.detach().cpu(), a.grad.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("case", RESIZE_CASES, ids=_rid)
def test_resize_vs_restatement(case):
    for mult in RESIZE_MULTS:
        x, cot, ref, bounds = resize_case(case, mult)
        assert max(bounds) <= BAR, (case, mult, bounds)
        got = gpu_resize(x, cot, case[1], mult)
        assert got[0].shape == ref[0].shape and all(bool(torch.isfinite(t).all()) for t in got)
        _check("resize %s x %g" % (_rid(case), mult), (rel_errors(got[0], ref[0])[1], rel_errors(got[1], ref[1])[1]), bounds,
               ("value max", "dx max"))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ONE_PASS_CASES, ids=_rid)
def test_resize_one_pass_adjoint(case):
    """dfmir_resize_bwd, the one-pass gather adjoint that stays exported, called as ResizeFn calls the separable one."""
    import dfmir_amd
    from dfmir_amd import ops
    from dfmir_amd._lib import check
    isp, osp = ((1,) * (3 - len(sp)) + sp for sp in case)
    for mult in RESIZE_MULTS:
        x, cot, ref, bounds = resize_case(case, mult)
        dy = cot.to(DEV)
        dx = torch.full(x.shape, float("nan"), device=DEV)
        check(dfmir_amd.lib().dfmir_resize_bwd(ops._p(dy), ops._p(dx), x.shape[0] * x.shape[1], *isp, *osp, mult, ops._st()))
        torch.cuda.synchronize()
        _check("one-pass adjoint %s x %g" % (_rid(case), mult), (rel_errors(dx, ref[1])[1],), bounds[1:], ("dx max",))
