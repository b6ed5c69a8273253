"""Shapes, seeded inputs and CPU evaluators shared by tests/test_gpu_warp_fp64.py (which explains them), tests/test_ref64.py
and scripts/warp_margins.py.  Imports nothing that needs a device or the GPU test modules."""
import itertools

import torch

from tests import ref64 as R
from tests import test_invcons as T
from tests.golden import common as C

WIN_3D = [(1, 1, 8, 8, 32), (1, 2, 7, 7, 28), (1, 3, 9, 9, 36), (3, 3, 8, 9, 36), (1, 5, 17, 8, 64), (1, 3, 5, 6, 4)]
SCA_3D = [(1, 3, 7, 9, 13), (2, 1, 5, 6, 7), (1, 3, 3, 5, 17), (1, 3, 8, 16, 2), (1, 3, 2, 3, 43)]
WIN_2D = [(1, 2, 64, 32), (1, 1, 63, 28), (1, 2, 65, 36), (3, 2, 130, 68)]
SCA_2D = [(2, 2, 9, 11), (1, 3, 17, 23), (1, 2, 15, 17), (1, 2, 6, 43)]
SHAPES = WIN_3D + SCA_3D + WIN_2D + SCA_2D
VI_SHAPES = [s for s in SHAPES if s[1] == len(s) - 2]
CHAIN_SHAPES = [(1, 3, 9, 9, 36), (1, 3, 7, 9, 13), (1, 2, 64, 32), (1, 2, 15, 17)]
CHAIN_STEPS = 7
CHAIN_FAMILIES = ("chain", "chain-neg")
# Run-to-run bit equality of the owner-gather d(src) is asked for on lattice on every windowed shape.  On these two it is
# checked on smooth instead: a departure from that wording.  An extent of more than one tile (17 planes, 130 rows) lets a
# lattice tap lie inside the volume but outside its tile's window; such voxels are listed for warp_win_slow_k, which adds
# with float atomics, so their sum depends on the order.  On the other windowed shapes every tap inside the volume is inside
# the window and lattice is checked.
SLOW_TAPS_INSIDE = [(1, 5, 17, 8, 64), (3, 2, 130, 68)]
WARP_FAMILIES = ("lattice", "smooth", "bulk", "far")
VI_FAMILIES = ("vi-0.25", "vi-1", "vi-6", "lattice")
VI_AMP = {"vi-0.25": 0.25, "vi-1": 1.0, "vi-6": 6.0}
BULK = (5.3, -4.6, 9.2)



def _seed(shape, family):
    return 3000 + 97 * SHAPES.index(shape) + 11 * (WARP_FAMILIES + VI_FAMILIES + ("nearest", "chain", "chain-neg")).index(family)


def flow_field(shape, family, seed=None):
    """[B, nd, *vol] fp32 of a case"""
    nd = len(shape) - 2
    fs = (shape[0], nd) + tuple(shape[2:])
    seed = _seed(shape, family) if seed is None else seed
    if family == "lattice":
        return T.fields(fs, "lattice", seed)[0]
    if family in ("far", "nearest"):
        half = 40 if family == "far" else 3
        k = torch.floor(C.rand(seed, *fs).double() * (2 * half + 1)).clamp(0, 2 * half) - half
        f = C.rand(seed + 1, *fs).double()
        f = 0.05 + 0.9 * f if family == "far" else 0.05 + 0.4 * f + 0.5 * (C.rand(seed + 3, *fs) > 0.5).double()
        return (k + f).float()
    u = T._sinusoids(fs, seed)
    if family == "bulk":
        u = u + torch.tensor(BULK[-nd:], dtype=torch.float64).reshape((1, nd) + (1,) * nd)
    elif family == "chain":
        u = 0.5 + u * 0.15
    elif family == "chain-neg":                       # 3 + 0.4 * sinusoids, the sign alternating over the channels from -
        sign = torch.tensor([-1.0, 1.0, -1.0][:nd], dtype=torch.float64).reshape((1, nd) + (1,) * nd)
        u = sign * (3.0 + u * 0.2)
    elif family != "smooth":
        u = u * (VI_AMP[family] / 2.0)
    return u.float()


def noise(seed, shape, amp):
    return ((C.rand(seed, *shape).double() * 2.0 - 1.0) * amp).float()


def rel_errors(got, ref, keep=None):
    """(relative 2-norm error, max-abs error over max) over the kept voxels; an all-zero reference wants an all-zero result"""
    g, r = got.detach().cpu().double(), ref.double()
    if keep is not None:
        g, r = g * keep, r * keep
    if float(r.abs().max()) == 0.0:
        return (0.0, 0.0) if float(g.abs().max()) == 0.0 else (float("inf"), float("inf"))
    return float((g - r).norm() / r.norm()), float((g - r).abs().max() / r.abs().max())


def warp_eval(src, flow, g, dtype=torch.float64):
    """(out, d(src), d(flow)) of R.warp on the CPU in `dtype`, for the upstream gradient g"""
    a = src.detach().cpu().to(dtype).requires_grad_()
    b = flow.detach().cpu().to(dtype).requires_grad_()
    out = R.warp(a, b, dtype=dtype)
    (out * g.detach().cpu().to(dtype)).sum().backward()
    return out.detach(), a.grad, b.grad


def vecint_eval(v, g, dtype=torch.float64, steps=1, pre=1.0, coords=None):
    """(out, dv) of `steps` chained R.vecint_step on pre * v, on the CPU in `dtype`; coords collects each step's sample points"""
    a = v.detach().cpu().to(dtype).requires_grad_()
    x = a * pre if pre != 1.0 else a
    for _ in range(steps):
        if coords is not None:
            coords.append((T._grid(x.shape[2:], dtype)[None] + x.detach()).double())
        x = R.vecint_step(x, dtype=dtype)
    (x * g.detach().cpu().to(dtype)).sum().backward()
    return x.detach(), a.grad


def nearest_ties(nd):
    """(src, flow, expected) with every sample point on k + 0.5.  Along each axis of extent 6 voxel i samples TIE_AT[i], which
    nearbyint takes to TIE_TO[i] (halves to the even integer; -0.5 -> -0 = voxel 0; 6 is outside: 0)."""
    TIE_AT = (-0.5, 0.5, 1.5, 2.5, 4.5, 5.5)
    TIE_TO = (0, 0, 2, 2, 4, 6)
    vol = (6,) * nd
    src = noise(77 + nd, (2, 2) + vol, 2.0)
    at = torch.tensor(TIE_AT, dtype=torch.float64)
    flow = torch.stack([(at - torch.arange(6.0, dtype=torch.float64)).reshape([-1 if d == a else 1 for d in range(nd)]).expand(vol)
                        for a in range(nd)], 0)[None].expand((2, nd) + vol).contiguous().float()
    want = torch.zeros_like(src)
    for pos in itertools.product(range(6), repeat=nd):
        to = tuple(TIE_TO[i] for i in pos)
        if max(to) < 6:
            want[(slice(None), slice(None)) + pos] = src[(slice(None), slice(None)) + to]
    return src, flow, want
