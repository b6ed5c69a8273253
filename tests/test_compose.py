"""ops.compose_flows / ops.invert_flow (build-defined, dfmir_amd/csrc/compose.hip) and what infer builds on them
(infer.invert_flow, infer.pull_back_label, refine_flow(update='compose')): the C ABI and the argument checks (CPU); a float64
restatement with explicit floor / gather indexing (ic_residual of tests/test_invcons.py: c = u + v(x + u) is that residual),
checked on the CPU against an independent F.grid_sample(align_corners=True, padding_mode='zeros') composition and against the
documented adjoint formulas; a float64 restatement of the fixed-point iteration, whose convergence on the cases the GPU tests
use is asserted on the CPU; and on the GPU the kernels against both.

Which launch each GPU shape reaches.  The kernels tile as invcons.hip's do (they share flow_sample.h): one workgroup owns
256 * VPT consecutive voxels of one sample, VPT = 4 (16-byte accesses through LDS) when W % 4 == 0 and the streamed pointers
are 16-byte aligned -- u and out for compose_fwd_k, u, g and du for compose_bwd_k, init and w for invert_k -- else 1.  So the
shape list is that of tests/test_invcons.py:
  <3-D, VPT 1>  (2,3,3,4,5); (1,3,5,6,7); (1,3,13,17,19) 17 workgroups; (1,3,3,5,17) 255 voxels; (1,3,8,16,2) 256;
                (1,3,2,3,43) 258; the misaligned view of (1,3,4,4,64); the non-contiguous (1,3,13,17,19)
  <3-D, VPT 4>  (1,3,4,4,64) 1024 voxels; (1,3,3,3,260) 3 workgroups; (1,3,3,5,68) 1020; (1,3,3,43,8) 1032;
                windowed (1,3,12,14,16); the 16^3 refinement
  <2-D, VPT 1>  (2,2,3,3); (2,2,9,11); (1,2,37,41) 6 workgroups; (1,2,15,17) 255; (1,2,128,2) 256; (1,2,6,43) 258; the
                misaligned view of (1,2,16,64); the non-contiguous (2,2,9,11); windowed (2,2,25,27)
  <2-D, VPT 4>  (1,2,5,300) 2 workgroups; (1,2,15,68) 1020; (1,2,16,64) 1024; (1,2,257,4) 1028; windowed (1,2,24,28), (1,2,5,300)
dv: the VPT 4 shapes hand g to the owner-gather warp adjoint (compose_bwd_k then runs for du alone, and not at all when only
dv is wanted); the VPT 1 shapes and the misaligned views take cmp_zero_k, cmp_absmax_k, compose_bwd_k with its 64-bit
fixed-point scatter and cmp_cvt_k.  inv_fin_k runs after every invert_k.

Inputs.  `lattice` and `smooth` are the families of tests/test_invcons.py (lattice: every sample point at least 0.05 from a
cell boundary, many outside the volume; smooth: sinusoids of wavelength >= 12 voxels, v a noisy near-inverse of u; for du on
smooth the voxels with a sample coordinate within 1e-4 of an integer are left out, at most 1 % per case, asserted on the CPU).
`windowed`, for the inversion: three sinusoids per channel of total amplitude 1.5 voxels and wavelength >= 12 voxels, times the
half-sine envelope prod_a sin(pi (i_a + 0.5) / n_a): the field vanishes at the border, where zero padding would otherwise stall
the iteration at rms ~ 0.1.  test_windowed_cases_converge_in_float64 asserts rms_20 < 1e-6 and a non-increasing rms_k, k <= 10,
for each windowed case: the condition under which the 20-iteration GPU comparisons mean anything.  Thin volumes converge too
slowly for that and serve the single-step test only.

Tolerances (profiles/compose_margins.txt, the rule of profiles/invcons_margins.txt): every comparison with the restatement is
bounded by 4x the error of the SAME definition evaluated by torch in fp32 on the CPU against float64, on these inputs: the
maxima over the case set, per family and per quantity -- a field in relative 2-norm and as max-abs over max, a statistic
relative.  scripts/compose_margins.py measures them and, beside them, the kernels' own errors when a device is there; no bound
is taken from those.  The 4x covers the other summation order of a GPU reduction and interpolation.  The residual history is
compared as max(stat_k, floor): below the floor a residual is rounding error alone; the floor is itself such an error, so it is
4x the statistic the fp32 CPU evaluation ends with (rms_20, max_20), per case.  The label flip share allowed is 4x the
share the fp32 CPU evaluation flips against the float64 inverse (nearest-neighbour ties flip with 1e-7 of coordinate error)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ref64
from tests import test_invcons as T
from tests import test_refine as R
from tests.golden import common as C
from tests.test_invcons import ic_residual

DEV = "cuda"
FACTOR = 4.0
FAMILIES = ("lattice", "smooth")
SHAPES_3D = [(2, 3, 3, 4, 5), (1, 3, 5, 6, 7), (1, 3, 13, 17, 19), (1, 3, 4, 4, 64), (1, 3, 3, 3, 260)]
SHAPES_2D = [(2, 2, 3, 3), (2, 2, 9, 11), (1, 2, 37, 41), (1, 2, 5, 300)]
SHAPES_EDGE = [(1, 3, 3, 5, 17), (1, 3, 8, 16, 2), (1, 3, 2, 3, 43), (1, 3, 3, 5, 68), (1, 3, 3, 43, 8),
               (1, 2, 15, 17), (1, 2, 128, 2), (1, 2, 6, 43), (1, 2, 15, 68), (1, 2, 16, 64), (1, 2, 257, 4)]
SHAPES = SHAPES_3D + SHAPES_2D + SHAPES_EDGE
WINDOWED = [(1, 3, 12, 14, 16), (1, 2, 24, 28), (1, 2, 5, 300), (2, 2, 25, 27)]
ITERS = 20
TOL = 1e-3
EXCLUDE_CAP = T.EXCLUDE_CAP

# profiles/compose_margins.txt, rows "max" of the fp32 CPU columns.
# compose_flows: (value 2-norm, value max, du 2-norm, du max, dv 2-norm, dv max)
FP32_COMPOSE = {"lattice": (2.15e-06, 7.14e-06, 5.05e-06, 1.91e-05, 7.80e-06, 1.10e-05),
                "smooth": (3.22e-06, 1.19e-05, 1.02e-06, 4.38e-06, 7.87e-06, 1.49e-05)}
# invert_flow, one step from noise on the lattice fields: (w 2-norm, w max, rms_0, max_0, rms_1, max_1)
FP32_STEP = (7.22e-06, 2.04e-05, 1.36e-07, 5.97e-07, 3.16e-07, 1.36e-05)
# invert_flow, 20 iterations on the windowed fields: (w 2-norm, w max, clipped history rms, clipped history max)
FP32_CONVERGED = (7.09e-07, 1.35e-06, 8.44e-02, 1.88e-01)
# rows "floor": what the fp32 CPU evaluation ends with per windowed case, (rms_20, max_20)
FP32_FLOOR = {(1, 3, 12, 14, 16): (3.62e-08, 2.98e-07), (1, 2, 24, 28): (4.81e-08, 4.89e-07),
              (1, 2, 5, 300): (1.95e-07, 2.76e-06), (2, 2, 25, 27): (7.99e-08, 5.79e-07)}
# infer.pull_back_label under the windowed 3-D flow: the share of voxels whose label the fp32 CPU evaluation flips
FP32_FLIPS = 0.0
# refine_flow(update='compose'), five iterations at 16^3: the flow, (2-norm, max)
FP32_REFINE = (1.42e-07, 1.80e-06)

BOUND_COMPOSE = {k: tuple(FACTOR * e for e in v) for k, v in FP32_COMPOSE.items()}
BOUND_STEP = tuple(FACTOR * e for e in FP32_STEP)
BOUND_CONVERGED = tuple(FACTOR * e for e in FP32_CONVERGED)
FLOOR = {k: tuple(FACTOR * e for e in v) for k, v in FP32_FLOOR.items()}
BOUND_FLIPS = FACTOR * FP32_FLIPS
BOUND_REFINE = tuple(FACTOR * e for e in FP32_REFINE)

_id = T._id


# ------------------------------------------------------------------------------------------ restatement
def compose_ref(u, v, g, dtype=torch.float64):
    """(c, du, dv) on the CPU in `dtype` (float64: the restatement; float32: the yardstick): c = u + v(x + u(x)) with explicit
    floor / gather indexing and its gradients for the incoming gradient g, by autograd."""
    a = u.detach().cpu().to(dtype).requires_grad_()
    b = v.detach().cpu().to(dtype).requires_grad_()
    c = ic_residual(a, b)
    (c * g.detach().cpu().to(dtype)).sum().backward()
    return c.detach(), a.grad, b.grad


def compose_grid_sample(u, v):
    """The same composition from F.grid_sample: normalised coordinates, align_corners=True, zero padding.  Shares no code
    with ic_residual."""
    nd = u.dim() - 2
    vol = tuple(u.shape[2:])
    f = T._grid(vol, u.dtype)[None] + u
    grid = torch.stack([2.0 * f[:, a] / (vol[a] - 1) - 1.0 for a in range(nd)][::-1], -1)
    return u + F.grid_sample(v, grid, mode='bilinear', padding_mode='zeros', align_corners=True)


def compose_adjoint(u, v, g):
    """(du, dv) by the documented formulas: du_c = g_c + sum_c' g_c' d_c v_c', d_c = corner differences with zero-padded
    corners as zeros; dv = the interpolation's transpose applied to g."""
    B, nd = u.shape[:2]
    S = math.prod(u.shape[2:])
    vf = v.reshape(B, nd, S)
    du = g.clone()
    dv = torch.zeros(B, nd, S, dtype=u.dtype)
    for flat, valid, w, bits in T._corners(u):
        idx = flat.reshape(B, 1, S).expand(B, nd, S)
        val = torch.gather(vf, 2, idx).reshape(u.shape) * valid.to(u.dtype)[:, None]
        for c in range(nd):
            others = torch.ones_like(w[:, 0])
            for a in range(nd):
                if a != c:
                    others = others * w[:, a]
            du[:, c] += (1.0 if bits[c] else -1.0) * others * (g * val).sum(1)
        dv.scatter_add_(2, idx, (g * (w.prod(1) * valid.to(u.dtype))[:, None]).reshape(B, nd, S))
    return du, dv.reshape(u.shape)


def _stats(r):
    """[B,2]: (sqrt(sum over voxels and channels of r^2 / S), max |r_c|) per sample"""
    B = r.shape[0]
    S = math.prod(r.shape[2:])
    return torch.stack([(r.reshape(B, -1) ** 2).sum(1).div(S).sqrt(), r.reshape(B, -1).abs().max(1).values], 1)


def invert_ref(u, iters, tol=0.0, init=None, dtype=torch.float64):
    """(w, history [iters + 1, B, 2]) of the fixed-point iteration on the CPU in `dtype`: r_k = w_k + u(x + w_k), w_{k+1} =
    w_k - r_k where max_c |r_k,c| > tol (a voxel that has stopped keeps its w, and so its r)."""
    uu = u.detach().cpu().to(dtype)
    w = torch.zeros_like(uu) if init is None else init.detach().cpu().to(dtype).clone()
    tol = float(np.float32(tol))                         # the kernel takes tol as a float
    hist = []
    for k in range(iters + 1):
        r = ic_residual(w, uu)
        hist.append(_stats(r))
        if k < iters:
            go = r.abs().max(1, keepdim=True).values > tol
            w = torch.where(go, w - r, w)
    return w, torch.stack(hist, 0)


def nearest_pull(label, w):
    """label(y + w(y)) with the nearest voxel (ties to even, as nearbyint) and 0 outside the volume, on the CPU in w's
    dtype: what SpatialTransformer(mode='nearest') computes."""
    B = w.shape[0]
    vol = tuple(w.shape[2:])
    nd = len(vol)
    f = T._grid(vol, w.dtype)[None] + w
    idx = torch.round(f).long()
    flat = torch.zeros((B,) + vol, dtype=torch.long)
    valid = torch.ones((B,) + vol, dtype=torch.bool)
    for a in range(nd):
        valid &= (idx[:, a] >= 0) & (idx[:, a] < vol[a])
        flat += idx[:, a].clamp(0, vol[a] - 1) * math.prod(vol[a + 1:])
    out = torch.gather(label.reshape(B, -1).float(), 1, flat.reshape(B, -1)).reshape((B, 1) + vol)
    return out * valid[:, None].float()


# ------------------------------------------------------------------------------------------ inputs
def fields(shape, family):
    """(u, v, g) fp32 of a composition case: the pair of tests/test_invcons.py and a random incoming gradient in [-1, 1]"""
    u, v = T.fields(shape, family)
    return u, v, C.rand(700 + 13 * SHAPES.index(shape), *shape) * 2.0 - 1.0


def step_fields(shape):
    """(u, init) fp32 of a single-step inversion case: the lattice u and noise of amplitude 2"""
    return T.fields(shape, "lattice")[0], (C.rand(800 + 13 * SHAPES.index(shape), *shape) * 2.0 - 1.0) * 2.0


def windowed(shape):
    """u fp32: three sinusoids per channel, total amplitude 1.5 voxels, wavelength >= 12 voxels, times the half-sine envelope"""
    vol = shape[2:]
    env = torch.ones(vol, dtype=torch.float64)
    for a, n in enumerate(vol):
        s = torch.sin(math.pi * (torch.arange(n, dtype=torch.float64) + 0.5) / n)
        env = env * s.reshape([-1 if i == a else 1 for i in range(len(vol))])
    return (0.75 * T._sinusoids(shape, 900 + 17 * WINDOWED.index(shape)) * env).float()


def label_blocks(vol, margin=3):
    """[1,1,*vol] fp32 label map: blocks of 3 x 3 (x 3) voxels with labels 1 .. 5, background 0 within `margin` of the border"""
    g = T._grid(vol, torch.float64)
    lab = (sum(torch.div(g[a], 3, rounding_mode='floor') * (a + 2) for a in range(len(vol))) % 5 + 1)
    inside = torch.ones(vol, dtype=torch.bool)
    for a, n in enumerate(vol):
        inside &= (g[a] >= margin) & (g[a] < n - margin)
    return (lab * inside)[None, None].float()


REFINE_VOL = (16, 16, 16)
REFINE_KW = dict(grid_downsize=2, iters=5, lr=0.02, lam=0.05, regularizer='diffusion')
REFINE_SPAN = (0.2, 0.8)


def refine_input():
    """(moving, fixed, flow0) fp32 at 16^3: five Gaussian blobs; the starting flow 0.5 + a smooth field of amplitude 0.15 per
    component, `true` = that + another smooth field of amplitude 0.15, fixed = moving warped by `true` in float64.  With
    lr = 0.02 five Adam steps move a component by at most 0.1, so every component of every flow_k stays inside REFINE_SPAN
    (asserted on the CPU): no sample point x + flow_k(x) of the similarity comes near a lattice point, where its gradient --
    piecewise constant in the position, with jumps as large as the image's second differences -- would take another cell in
    fp32 than in float64 and send the Adam iterates apart.  (Measured on a pair whose flow crossed lattice points: one voxel
    3e-6 from one changed a gradient component by 3e-3 of the largest and the flow after five steps by 2e-5, for either
    `update`.)  The correction up(delta) itself crosses zero, where compose_flows' du has its kink; the jump there is the second
    difference of the smooth starting flow, 0.15 (2 pi / 12)^2 = 0.04 of one voxel's second term, far below the bound."""
    vol = REFINE_VOL
    g = T._grid(vol, torch.float64)
    ctr = C.rand(171, 5, 3).double() * 0.5 + 0.25
    sig = 2.0 + 1.0 * C.rand(172, 5).double()
    moving = torch.zeros(vol, dtype=torch.float64)
    for i in range(5):
        d2 = sum((g[a] - ctr[i, a] * (vol[a] - 1)) ** 2 for a in range(3))
        moving = moving + torch.exp(-d2 / (2.0 * sig[i] ** 2))
    moving = moving[None, None]
    flow0 = 0.5 + 0.075 * T._sinusoids((1, 3) + vol, 173)
    true = flow0 + 0.075 * T._sinusoids((1, 3) + vol, 175)
    f = g[None] + true
    grid = torch.stack([2.0 * f[:, a] / (vol[a] - 1) - 1.0 for a in range(3)][::-1], -1)
    fixed = F.grid_sample(moving, grid, mode='bilinear', padding_mode='zeros', align_corners=True)
    return moving.float(), fixed.float(), flow0.float()


def refine_compose_ref(moving, fixed, flow0, dtype=torch.float64, grid_downsize=2, iters=5, lr=0.1, lam=0.05,
                       betas=(0.9, 0.999), **_):
    """refine_flow(update='compose', features='intensity', the diffusion penalty) restated on the CPU in `dtype`:
    flow_k = up(delta_k) + flow0(x + up(delta_k)(x)).  (flow, history [iters + 1, 2], (the smallest, the largest component of
    any flow_k))."""
    M, Fx, f0 = (t.detach().cpu().to(dtype) for t in (moving, fixed, flow0))
    vol = tuple(M.shape[2:])
    nd = len(vol)
    opt = ref64.Adam(torch.zeros((M.shape[0], nd) + tuple(n // grid_downsize for n in vol)), lr, betas, 1e-8, dtype=dtype)
    up = lambda d: F.interpolate(d, size=vol, mode='trilinear' if nd == 3 else 'bilinear', align_corners=True)
    hist = torch.zeros(iters + 1, 2, dtype=dtype)
    lo, hi = float('inf'), -float('inf')
    for k in range(iters + 1):
        d = opt.p.clone().requires_grad_(k < iters)
        flow = ic_residual(up(d), f0)
        lo, hi = min(lo, float(flow.detach().min())), max(hi, float(flow.detach().max()))
        sim = R.ssd_grid_sample(M, Fx, flow)[0]
        reg = ref64.grad_loss(flow, 'l2', dtype=dtype)
        hist[k, 0], hist[k, 1] = sim.detach(), reg.detach()
        if k < iters:
            (g,) = torch.autograd.grad(sim + lam * reg, d)
            opt.step(g)
    return flow.detach(), hist, (lo, hi)


# ------------------------------------------------------------------------------------------ errors (shared with the script)
def field_errors(got, ref, keep=None):
    """(relative 2-norm error, max-abs error over max) of a field against the restatement's, over the kept voxels"""
    return T.rel_errors(got, ref, keep)


def stat_errors(got, ref):
    """relative errors of a [B,2] statistics row, the worst over the samples: (rms, max)"""
    g, r = got.detach().cpu().double(), ref.double()
    e = ((g - r).abs() / r.abs()).max(0).values
    return float(e[0]), float(e[1])


def history_errors(got, ref, floor):
    """relative errors of max(stat_k, floor) over a [K,B,2] history, the worst over k and the samples: (rms, max)"""
    fl = torch.tensor(floor, dtype=torch.float64)
    g, r = torch.maximum(got.detach().cpu().double(), fl), torch.maximum(ref.double(), fl)
    e = ((g - r).abs() / r).reshape(-1, 2).max(0).values
    return float(e[0]), float(e[1])


def compose_errors(got, ref, keep):
    """(value 2-norm, value max, du 2-norm, du max, dv 2-norm, dv max); du over the kept voxels"""
    return field_errors(got[0], ref[0]) + field_errors(got[1], ref[1], keep) + field_errors(got[2], ref[2])


_REF = {}


def compose_reference(shape, family):
    """(u, v, g, (c64, du64, dv64), keep) of a case, computed once and shared"""
    key = ("compose", shape, family)
    if key not in _REF:
        u, v, g = fields(shape, family)
        _REF[key] = (u, v, g, compose_ref(u, v, g), T.du_keep(u) if family == "smooth" else None)
    return _REF[key]


def step_reference(shape):
    """(u, init, (w64, history64)) of a single-step case"""
    key = ("step", shape)
    if key not in _REF:
        u, init = step_fields(shape)
        _REF[key] = (u, init, invert_ref(u, 1, init=init))
    return _REF[key]


def windowed_reference(shape):
    """(u, (w64, history64)) of a converged case"""
    key = ("windowed", shape)
    if key not in _REF:
        u = windowed(shape)
        _REF[key] = (u, invert_ref(u, ITERS))
    return _REF[key]


def refine_reference():
    """((moving, fixed, flow0), (flow64, history64, span64))"""
    if "refine" not in _REF:
        inp = refine_input()
        _REF["refine"] = (inp, refine_compose_ref(*inp, **REFINE_KW))
    return _REF["refine"]


def _gpu_compose(u, v, g, need_v=True):
    from dfmir_amd import ops
    a, b = u.to(DEV).requires_grad_(), v.to(DEV).requires_grad_(need_v)
    c = ops.compose_flows(a, b)
    c.backward(g.to(DEV))
    torch.cuda.synchronize()
    return c.detach().cpu(), a.grad.cpu(), None if b.grad is None else b.grad.cpu()


def _gpu_invert(u, **kw):
    from dfmir_amd import ops
    if kw.get("init") is not None:
        kw["init"] = kw["init"].to(DEV)
    w, stats = ops.invert_flow(u.to(DEV), **kw)
    torch.cuda.synchronize()
    return w.cpu(), stats.cpu()


def _check(e, bound, what):
    print("%s: %s" % (what, "  ".join("%.3e (bound %.1e)" % p for p in zip(e, bound))))
    assert all(x <= y for x, y in zip(e, bound)), (what, e, bound)


# ------------------------------------------------------------------------------------------ CPU tier
NEW_SYMBOLS = ("dfmir_compose_fwd", "dfmir_compose_bwd_ws_floats", "dfmir_compose_bwd", "dfmir_flow_invert_ws_floats",
               "dfmir_flow_invert")


def test_compose_symbols_in_header_exports_and_ctypes_table():
    import dfmir_amd
    from dfmir_amd import _lib, infer, ops
    from tests.test_abi import REPO, header_symbols
    h = ctypes.CDLL(dfmir_amd.LIB_PATH)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "dfmir_hip.h")).read(), flags=re.S)
    for s in NEW_SYMBOLS:
        assert s in header_symbols() and s in _lib.exported_symbols() and hasattr(h, s), s
        params = re.search(r"\b%s\s*\(([^)]*)\)" % s, text).group(1)
        assert len(params.split(",")) == len(_lib._SIGS[s]), s            # the arity of the declaration and of the table
    lib = dfmir_amd.lib()
    assert lib.dfmir_abi_version() == 14
    assert lib.dfmir_compose_bwd_ws_floats(3, 2, 4, 5, 6) == 2 * 2 * 3 * 120 + 2       # a 64-bit sum per element, one for max |g|
    assert lib.dfmir_compose_bwd_ws_floats(2, 2, 999, 3, 3) == 2 * 2 * 2 * 9 + 2        # nd == 2: D is not read
    assert lib.dfmir_flow_invert_ws_floats(3, 1, 16, 16, 16, 20, 0) == 3 * 16           # a double and an unsigned per 256 voxels
    assert lib.dfmir_flow_invert_ws_floats(3, 2, 16, 16, 16, 20, 1) == 3 * 21 * 2 * 16  # ... and per iteration with history
    for name in ("ComposeFlowsFn", "compose_flows", "invert_flow"):
        assert hasattr(ops, name), name
    assert hasattr(infer, "invert_flow") and hasattr(infer, "pull_back_label")
    assert ops.INVERT_MAX_ITERS == 64


def test_compose_bad_arguments_are_invalid_without_a_device():
    import dfmir_amd
    lib = dfmir_amd.lib()
    for bad in T.BAD_DIMS:
        assert lib.dfmir_compose_bwd_ws_floats(*bad) == -1 and lib.dfmir_flow_invert_ws_floats(*bad, 20, 1) == -1, bad
    assert lib.dfmir_flow_invert_ws_floats(3, 1, 8, 8, 8, 65, 0) == -1 and lib.dfmir_flow_invert_ws_floats(3, 1, 8, 8, 8, -1, 0) == -1
    buf = (ctypes.c_double * 64)()                      # host memory: an argument the checks refuse is never dereferenced
    p = ctypes.cast(buf, ctypes.c_void_p)

    def refused(rc, what):
        assert rc != 0 and b"invalid argument" in lib.dfmir_last_error(), what

    for bad in T.BAD_DIMS:
        nd, dims = bad[0], bad[1:]
        refused(lib.dfmir_compose_fwd(nd, p, p, p, *dims, None), bad)
        refused(lib.dfmir_compose_bwd(nd, p, p, p, p, p, p, *dims, None), bad)
        refused(lib.dfmir_flow_invert(nd, p, p, p, p, p, *dims, 20, 0.0, 1, None), bad)
    good = (1, 8, 8, 8)
    for hole in range(3):                               # a NULL pointer in every position
        args = [p] * 3
        args[hole] = None
        refused(lib.dfmir_compose_fwd(3, *args, *good, None), hole)
    for args in ((None, p, p, p, p, p), (p, None, p, p, p, p), (p, p, None, p, p, p), (p, p, p, None, None, p),
                 (p, p, p, p, p, None)):                # no gradient wanted at all; dv without scratch
        refused(lib.dfmir_compose_bwd(3, *args, *good, None), args)
    for args in ((None, p, p, p, p), (p, p, None, p, p), (p, p, p, None, p), (p, p, p, p, None)):     # init alone is optional
        refused(lib.dfmir_flow_invert(3, *args, *good, 20, 0.0, 0, None), args)
    for iters, tol in ((-1, 0.0), (65, 0.0), (20, -1e-3), (20, float('inf')), (20, float('nan'))):
        refused(lib.dfmir_flow_invert(3, p, p, p, p, p, *good, iters, tol, 0, None), (iters, tol))


def test_compose_and_invert_reject_bad_arguments_before_any_launch():
    from dfmir_amd import infer, ops
    from dfmir_amd._lib import DfmirHipError
    u = torch.rand(1, 3, 8, 8, 8)
    calls = (lambda a, b: ops.compose_flows(a, b), lambda a, b: ops.compose_flows(b, a), lambda a, b: ops.invert_flow(a, init=b),
             lambda a, b: ops.invert_flow(b, init=a))
    for fn in calls:
        with pytest.raises(ValueError, match="tensor"):
            fn(u, None if fn in calls[:2] else 3.0)
        with pytest.raises(ValueError, match="field"):
            fn(u, torch.rand(3, 8, 8))
        with pytest.raises(ValueError, match="mismatch"):
            fn(u, torch.rand(1, 3, 8, 8, 9))
        with pytest.raises(ValueError, match="mismatch"):
            fn(u, torch.rand(2, 3, 8, 8, 8))
        with pytest.raises(ValueError, match="channels"):
            fn(torch.rand(1, 2, 8, 8, 8), torch.rand(1, 2, 8, 8, 8))
        with pytest.raises(ValueError, match="channels"):
            fn(torch.rand(1, 3, 8, 8), torch.rand(1, 3, 8, 8))
        with pytest.raises(ValueError, match="extent"):
            fn(torch.rand(1, 3, 8, 1, 8), torch.rand(1, 3, 8, 1, 8))
        with pytest.raises(ValueError, match="extent"):
            fn(torch.rand(1, 2, 8, 1), torch.rand(1, 2, 8, 1))
        with pytest.raises(DfmirHipError, match="fp32"):
            fn(u.double(), u.double())
        with pytest.raises(DfmirHipError, match="no CPU fallback"):
            fn(u, u)
    with pytest.raises(ValueError, match="tensor"):
        ops.invert_flow([[0.0]])
    with pytest.raises(ValueError, match="field"):
        ops.invert_flow(torch.rand(8, 8))
    with pytest.raises(ValueError, match="channels"):
        ops.invert_flow(torch.rand(1, 3, 8, 8))
    with pytest.raises(ValueError, match="extent"):
        ops.invert_flow(torch.rand(1, 2, 1, 8))
    for iters in (-1, 65, 2.0, True, None, "3"):
        with pytest.raises(ValueError, match="iters"):
            ops.invert_flow(u, iters=iters)
        with pytest.raises(ValueError, match="iters"):
            infer.invert_flow(u, iters=iters)
        with pytest.raises(ValueError, match="iters"):
            infer.pull_back_label(u[:, :1], u, iters=iters)
    for tol in (-1e-3, float('inf'), float('nan'), None, "x"):
        with pytest.raises(ValueError, match="tol"):
            ops.invert_flow(u, tol=tol)
        with pytest.raises(ValueError, match="tol"):
            infer.invert_flow(u, tol=tol)
    with pytest.raises(DfmirHipError, match="no CPU fallback"):
        ops.invert_flow(u, iters=0)
    a = torch.rand(1, 1, 8, 8, 8)
    for bad in ('sum', None, 0, 'Compose'):
        with pytest.raises(ValueError, match="update"):
            infer.refine_flow(a, a, u, lam=0.1, lr=0.1, update=bad)


CPU_SHAPES = [(2, 3, 5, 6, 7), (1, 3, 3, 4, 9), (2, 2, 9, 11), (1, 2, 2, 2)]


@pytest.mark.parametrize("shape", CPU_SHAPES, ids=_id)
@pytest.mark.parametrize("family", FAMILIES)
def test_restatement_equals_the_grid_sample_composition_and_the_adjoint_formulas(shape, family):
    """Gradients against grid_sample's on the lattice family only (no sample point near a cell boundary, where the
    normalised-coordinate round trip may pick the other cell: du is piecewise constant in the position)."""
    u, v = (t.double() for t in T.fields(shape, family, seed=71))
    g = C.rand(73, *shape).double() * 2.0 - 1.0
    c, du, dv = compose_ref(u, v, g)
    a, b = u.clone().requires_grad_(), v.clone().requires_grad_()
    cg = compose_grid_sample(a, b)
    (cg * g).sum().backward()
    assert float((cg.detach() - c).abs().max()) <= 1e-12 * float(c.abs().max())
    assert float((b.grad - dv).abs().max()) <= 1e-12 * float(dv.abs().max())
    if family == "lattice":
        assert float((a.grad - du).abs().max()) <= 1e-12 * float(du.abs().max())
    fu, fv = compose_adjoint(u, v, g)
    assert float((fu - du).abs().max()) <= 1e-12 * float(du.abs().max())
    assert float((fv - dv).abs().max()) <= 1e-12 * float(dv.abs().max())
    w, hist = invert_ref(u, 1, init=v)                      # one step of the iteration is a composition
    assert torch.equal(w, v - ic_residual(v, u)) and torch.equal(hist[0], _stats(ic_residual(v, u)))
    assert float((w + compose_grid_sample(v, u) - v).abs().max()) <= 1e-12 * float(u.abs().max())


def test_smooth_seeds_stay_under_the_exclusion_cap():
    for shape in SHAPES:
        u = fields(shape, "smooth")[0]
        assert 1.0 - float(T.du_keep(u).double().mean()) <= EXCLUDE_CAP, shape


@pytest.mark.parametrize("shape", WINDOWED, ids=_id)
def test_windowed_cases_converge_in_float64(shape):
    u, (w, hist) = windowed_reference(shape)
    assert float(u.abs().max()) <= 1.5 and tuple(hist.shape) == (ITERS + 1, shape[0], 2)
    rms = hist[:, :, 0]
    print("%s: rms_k %s" % (_id(shape), " ".join("%.1e" % float(x) for x in rms.max(1).values)))
    assert float(rms[ITERS].max()) < 1e-6
    assert bool((rms[1:11] <= rms[:10]).all())
    border = 0.75 * 2.0 * math.sin(math.pi * 0.5 / shape[2])                # the envelope's value in the outermost voxel
    assert float(u[:, :, 0].abs().max()) <= border + 1e-6
    # with a tolerance every voxel ends at or below it, or has used all its updates; the statistics say the same
    wt, ht = invert_ref(u, ITERS, tol=TOL)
    assert float(ht[ITERS, :, 1].max()) <= TOL and not torch.equal(wt, w)


def test_label_blocks_and_the_integer_shift_inverse():
    """The float64 iteration on a constant integer flow s: w = -s wherever x - s stays inside, and B's labels pulled back are
    A's in the interior."""
    vol, s = (12, 14, 16), (2.0, -1.0, 3.0)
    lab = label_blocks(vol)
    assert sorted(set(lab.flatten().tolist())) == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0] and float(lab[..., :3, :, :].abs().max()) == 0.0
    u = torch.tensor(s, dtype=torch.float64).reshape(1, 3, 1, 1, 1).expand(1, 3, *vol).contiguous()
    w, _ = invert_ref(u, ITERS)
    inner = (slice(None), slice(None), slice(3, -3), slice(3, -3), slice(3, -3))
    assert torch.equal(w[inner], -u[inner])
    lab_b = nearest_pull(lab, u)                               # A's labels carried onto B by the flow
    assert torch.equal(nearest_pull(lab_b, w)[inner], lab[inner])


def test_windowed_labels_move_and_the_refinement_restatement_reduces_the_similarity():
    """The inputs of the label and refinement tests do what those tests need, in float64."""
    shape = WINDOWED[0]
    lab = label_blocks(shape[2:])
    moved = float((nearest_pull(lab, windowed_reference(shape)[1][0]) != lab).float().mean())
    assert moved > 0.02, moved
    (moving, fixed, flow0), (flow64, hist64, span) = refine_reference()
    print("similarity %s; components of flow_k in [%.3f, %.3f]; the flow moved by up to %.3f"
          % (" ".join("%.4e" % float(x) for x in hist64[:, 0]), span[0], span[1], float((flow64 - flow0.double()).abs().max())))
    assert REFINE_SPAN[0] <= span[0] and span[1] <= REFINE_SPAN[1]            # no sample point near a lattice point, ever
    assert float(hist64[5, 0]) < float(hist64[0, 0]) and float((flow64 - flow0.double()).abs().max()) > 0.05


# ------------------------------------------------------------------------------------------ GPU tier
@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_compose_flows_value_and_gradients_vs_restatement(shape):
    for family in FAMILIES:
        u, v, g, ref, keep = compose_reference(shape, family)
        got = _gpu_compose(u, v, g)
        assert all(bool(torch.isfinite(t).all()) for t in got)
        _check(compose_errors(got, ref, keep), BOUND_COMPOSE[family], "%s [%s]" % (_id(shape), family))
        only_u = _gpu_compose(u, v, g, need_v=False)           # v needs no gradient: dv is None and du the same bits
        assert only_u[2] is None and torch.equal(only_u[0], got[0]) and torch.equal(only_u[1], got[1])


@pytest.mark.gpu
def test_compose_flows_gradient_to_v_only():
    from dfmir_amd import ops
    for shape in ((1, 3, 5, 6, 7), (1, 3, 4, 4, 64)):           # the scatter; the owner-gather adjoint without compose_bwd_k
        u, v, g, _, _ = compose_reference(shape, "lattice")
        want = _gpu_compose(u, v, g)
        b = v.to(DEV).requires_grad_()
        (dv,) = torch.autograd.grad(ops.compose_flows(u.to(DEV), b), b, g.to(DEV))
        assert torch.equal(dv.cpu(), want[2])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 3, 3, 4, 5), (1, 3, 13, 17, 19), (1, 3, 3, 3, 260), (2, 2, 9, 11), (1, 2, 5, 300)], ids=_id)
def test_compose_flows_identities(shape):
    from dfmir_amd import ops
    u, v, _, ref, _ = compose_reference(shape, "lattice")
    a, b, z = u.to(DEV), v.to(DEV), torch.zeros(shape, device=DEV)
    assert torch.equal(ops.compose_flows(a, z), a) and torch.equal(ops.compose_flows(z, b), b)
    k = torch.round(u)                                          # integer-valued: u plus the shifted v, zeros where it leaves
    want = k + nearest_pull_field(v, k)
    assert torch.equal(ops.compose_flows(k.to(DEV), b).cpu(), want)
    c = ops.compose_flows(a, b)
    bound = BOUND_COMPOSE["lattice"]
    _check(field_errors(a + ops.warp(b, a), c.cpu()), bound[:2], "u + warp(v, u) " + _id(shape))
    _check(field_errors(ops.vecint_step(b), ops.compose_flows(b, b).cpu()), bound[:2], "vecint_step " + _id(shape))
    ic, ms = float(ops.inverse_consistency(a, b)), float(c.double().square().mean())
    _check((abs(ic - ms) / ms,), bound[1:2], "inverse_consistency against mean(c^2) " + _id(shape))


def nearest_pull_field(v, k):
    """v(x + k(x)) channel by channel for an integer-valued k: the shifted v, zeros outside the volume"""
    return torch.cat([nearest_pull(v[:, c:c + 1].contiguous(), k) for c in range(v.shape[1])], 1)


def _misaligned(t):
    """a contiguous device copy of t that starts 4 bytes past a 16-byte boundary"""
    off = torch.empty(t.numel() + 1, device=DEV)[1:].view(t.shape)
    off.copy_(t)
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    return off


@pytest.mark.gpu
def test_compose_flows_non_contiguous_and_misaligned_inputs():
    from dfmir_amd import ops
    for shape, perm in (((1, 3, 13, 17, 19), (0, 1, 4, 3, 2)), ((2, 2, 9, 11), (0, 1, 3, 2))):
        u, v, g, _, _ = compose_reference(shape, "lattice")
        want = _gpu_compose(u, v, g)
        nu = u.permute(*perm).contiguous().to(DEV).permute(*perm).requires_grad_()
        nv = v.permute(*perm).contiguous().to(DEV).permute(*perm).requires_grad_()
        ng = g.permute(*perm).contiguous().to(DEV).permute(*perm)
        assert not nu.is_contiguous() and not nv.is_contiguous() and not ng.is_contiguous()
        c = ops.compose_flows(nu, nv)
        c.backward(ng)
        assert torch.equal(c.detach().cpu(), want[0]) and torch.equal(nu.grad.cpu(), want[1]) and torch.equal(nv.grad.cpu(), want[2])
        w, st = ops.invert_flow(nu.detach(), iters=1, init=nv.detach())
        w2, st2 = _gpu_invert(u, iters=1, init=v)
        assert torch.equal(w.cpu(), w2) and torch.equal(st.cpu(), st2)
    # W % 4 == 0 but u starts 4 bytes off a 16-byte boundary: the scalar launches and the fixed-point dv.  The same arithmetic
    # per voxel: value and du to the bit
    for shape in ((1, 3, 4, 4, 64), (1, 2, 16, 64)):
        u, v, g, ref, keep = compose_reference(shape, "lattice")
        want = _gpu_compose(u, v, g)
        x, y = _misaligned(u).requires_grad_(), v.to(DEV).requires_grad_()
        c = ops.compose_flows(x, y)
        gx, gy = torch.autograd.grad(c, (x, y), g.to(DEV))
        torch.cuda.synchronize()
        _check(compose_errors((c.detach().cpu(), gx.cpu(), gy.cpu()), ref, keep), BOUND_COMPOSE["lattice"], "misaligned " + _id(shape))
        assert torch.equal(c.detach().cpu(), want[0]) and torch.equal(gx.cpu(), want[1])
        u, init, (w64, h64) = step_reference(shape)
        w, st = ops.invert_flow(u.to(DEV), iters=1, init=_misaligned(init), history=True)
        w2, st2 = _gpu_invert(u, iters=1, init=init, history=True)
        assert torch.equal(w.cpu(), w2)
        _check(stat_errors(st[0].cpu(), h64[0]) + stat_errors(st[1].cpu(), h64[1]), BOUND_STEP[2:], "misaligned step " + _id(shape))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 3, 4, 4, 64), (1, 2, 5, 300)], ids=_id)
def test_compose_flows_fixed_point_dv_on_vector_shapes(shape):
    """DFMIR_INVCONS_FIXED64 on aligned W % 4 == 0 shapes: the VPT = 4 launch of compose_bwd_k with its own scatter."""
    from dfmir_amd import _lib
    u, v, g, ref, keep = compose_reference(shape, "lattice")
    want = _gpu_compose(u, v, g)
    _lib.set_option("DFMIR_INVCONS_FIXED64", "1")
    try:
        got = _gpu_compose(u, v, g)
        _check(compose_errors(got, ref, keep), BOUND_COMPOSE["lattice"], "fixed-point dv " + _id(shape))
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert torch.equal(_gpu_compose(u, v, g)[2], got[2])
    finally:
        _lib.set_option("DFMIR_INVCONS_FIXED64", None)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_invert_flow_single_step_vs_restatement(shape):
    u, init, (w64, h64) = step_reference(shape)
    w, hist = _gpu_invert(u, iters=1, init=init, history=True)
    assert tuple(hist.shape) == (2, shape[0], 2) and bool(torch.isfinite(w).all())
    e = field_errors(w, w64) + stat_errors(hist[0], h64[0]) + stat_errors(hist[1], h64[1])
    _check(e, BOUND_STEP, "step " + _id(shape))
    w0, st0 = _gpu_invert(u, iters=0, init=init)                # no update: init back, and the statistics of r_0
    assert torch.equal(w0, init) and torch.equal(st0, hist[0])
    wz, stz = _gpu_invert(u, iters=0)                           # no init: zeros, r_0 = u
    assert float(wz.abs().max()) == 0.0
    _check(stat_errors(stz, _stats(u.double())), BOUND_STEP[2:4], "r_0 = u " + _id(shape))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", WINDOWED, ids=_id)
def test_invert_flow_converged_vs_restatement(shape):
    from dfmir_amd import ops
    u, (w64, h64) = windowed_reference(shape)
    w, hist = _gpu_invert(u, iters=ITERS, history=True)
    print("%s: rms_k %s" % (_id(shape), " ".join("%.1e" % float(x) for x in hist[:, :, 0].max(1).values)))
    e = field_errors(w, w64) + history_errors(hist, h64, FLOOR[shape])
    _check(e, BOUND_CONVERGED, "converged " + _id(shape))
    w2, last = _gpu_invert(u, iters=ITERS)
    assert torch.equal(w2, w) and torch.equal(last, hist[-1])    # history=False: the same flow, the statistics of r_iters
    # tol: every voxel ends with max_c |r_c| <= tol, or did all its updates (then it is the tol = 0 voxel, bit for bit:
    # each voxel iterates on its own)
    wt, ht = _gpu_invert(u, iters=ITERS, tol=TOL, history=True)
    r = ops.compose_flows(wt.to(DEV), u.to(DEV)).cpu()
    small = r.abs().max(1, keepdim=True).values <= float(np.float32(TOL))
    same = (wt == w).all(1, keepdim=True)
    assert bool((small | same).all()) and 0.0 < float(small.float().mean())
    assert float(ht[-1, :, 1].max()) <= float(np.float32(TOL)) and not torch.equal(wt, w)
    # restart: init = w and no iteration returns w; its statistics are those the first call ended with
    w3, st3 = _gpu_invert(u, iters=0, init=w)
    assert torch.equal(w3, w) and torch.equal(st3, last)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 3, 13, 17, 19), (1, 3, 3, 3, 260), (1, 2, 37, 41), (1, 2, 5, 300)],
                         ids=["3d", "3d-vec", "2d", "2d-vec"])
def test_compose_and_invert_bit_reproducible(shape):
    for family in FAMILIES:
        u, v, g, _, _ = compose_reference(shape, family)
        r0, r1 = _gpu_compose(u, v, g), _gpu_compose(u, v, g)
        assert all(torch.equal(x, y) for x, y in zip(r0, r1)), family
    u, init, _ = step_reference(shape)
    for kw in (dict(iters=3, init=init, history=True), dict(iters=ITERS, tol=TOL), dict(iters=5, history=True)):
        r0, r1 = _gpu_invert(u * 0.25, **kw), _gpu_invert(u * 0.25, **kw)
        assert torch.equal(r0[0], r1[0]) and torch.equal(r0[1], r1[1]), sorted(kw)


@pytest.mark.gpu
def test_infer_invert_flow_reports_the_inverse_and_its_residuals():
    from dfmir_amd import infer, ops
    shape = WINDOWED[0]
    u, (w64, h64) = windowed_reference(shape)
    flow = u.to(DEV)
    out = infer.invert_flow(flow, iters=ITERS)
    assert sorted(out) == ["history", "inverse", "residual", "residual_max", "roundtrip"]
    assert tuple(out["inverse"].shape) == shape and tuple(out["history"].shape) == (ITERS + 1, 1, 2)
    assert all(tuple(out[k].shape) == (1,) for k in ("residual", "residual_max", "roundtrip"))
    assert torch.equal(out["residual"], out["history"][-1, :, 0]) and torch.equal(out["residual_max"], out["history"][-1, :, 1])
    assert torch.equal(out["inverse"], ops.invert_flow(flow, iters=ITERS)[0])
    assert torch.equal(out["roundtrip"], infer.inverse_consistency_error(flow, out["inverse"]))
    # the residual is the inverse-consistency error of (inverse, flow): the same quantity from the other kernel
    other = float(infer.inverse_consistency_error(out["inverse"], flow))
    assert abs(float(out["residual"]) - other) <= 1e-6 * other + FLOOR[shape][0]
    print("residual %.3e, max %.3e, roundtrip %.3e" % tuple(float(out[k]) for k in ("residual", "residual_max", "roundtrip")))


@pytest.mark.gpu
def test_pull_back_label_integer_shift_and_windowed_flow():
    from dfmir_amd import infer
    from dfmir_amd.voxelmorph import SpatialTransformer
    vol, s = (12, 14, 16), (2.0, -1.0, 3.0)
    lab = label_blocks(vol)
    u = torch.tensor(s).reshape(1, 3, 1, 1, 1).expand(1, 3, *vol).contiguous()
    st = SpatialTransformer(vol, mode='nearest').to(DEV)
    lab_b = st(lab.to(DEV), u.to(DEV))                          # A's labels carried onto B
    assert torch.equal(lab_b.cpu(), nearest_pull(lab, u))
    out = infer.pull_back_label(lab_b, u.to(DEV), iters=ITERS)
    assert sorted(out) == ["inverse", "label", "residual", "residual_max"]
    inner = (slice(None), slice(None), slice(3, -3), slice(3, -3), slice(3, -3))
    assert torch.equal(out["inverse"].cpu()[inner], -u[inner]) and torch.equal(out["label"].cpu()[inner], lab[inner])
    assert tuple(out["label"].shape) == (1, 1) + vol and tuple(out["residual"].shape) == (1,)
    # a windowed flow: against nearest sampling under the float64 inverse
    shape = WINDOWED[0]
    flow, (w64, _) = windowed_reference(shape)
    out = infer.pull_back_label(lab.to(DEV), flow.to(DEV), iters=ITERS)
    want = nearest_pull(lab, w64)
    assert torch.equal(out["label"], st(lab.to(DEV), out["inverse"]))
    share = float((out["label"].cpu() != want).float().mean())
    moved = float((want != lab).float().mean())
    print("labels that differ from the float64 pull-back: %.3e of the voxels (bound %.1e); %.3f moved at all"
          % (share, BOUND_FLIPS, moved))
    assert share <= BOUND_FLIPS
    assert float(out["residual_max"]) <= FLOOR[shape][1]


@pytest.mark.gpu
def test_refine_flow_update_compose():
    from dfmir_amd import infer, ops
    (moving, fixed, flow0), (flow64, hist64, _) = refine_reference()
    mv, fx, f0 = moving.to(DEV), fixed.to(DEV), flow0.to(DEV)
    kw = dict(features='intensity', **REFINE_KW)
    add0, cmp0 = infer.refine_flow(mv, fx, None, **kw), infer.refine_flow(mv, fx, None, update='compose', **kw)
    for k in ("flow", "warped", "history"):                     # no starting flow: the same computation
        assert torch.equal(add0[k], cmp0[k]), k
    add, cmp = infer.refine_flow(mv, fx, f0, update='add', **kw), infer.refine_flow(mv, fx, f0, update='compose', **kw)
    assert torch.equal(add["history"][0], cmp["history"][0])    # delta = 0: compose_flows(0, flow0) is flow0
    assert torch.equal(cmp["history"][0, 0], ops.warp_ssd(mv, fx, f0))
    assert not torch.equal(add["flow"], cmp["flow"]) and torch.equal(cmp["warped"], ops.warp(mv, cmp["flow"]))
    hist = cmp["history"].cpu().double()
    print("similarity %s (fp64 loop %s)" % (" ".join("%.4e" % float(x) for x in hist[:, 0]),
                                            " ".join("%.4e" % float(x) for x in hist64[:, 0])))
    assert float(hist[5, 0]) < float(hist[0, 0]) and float(hist64[5, 0]) < float(hist64[0, 0])
    _check(field_errors(cmp["flow"], flow64), BOUND_REFINE, "refine_flow(update='compose')")
