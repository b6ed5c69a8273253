"""InverseConsistency_Loss / ops.inverse_consistency (build-defined, dfmir_amd/csrc/invcons.hip): the C ABI and the argument
checks (CPU), a float64 restatement of the definition written with explicit floor / gather indexing, checked on the CPU
against an independent F.grid_sample(align_corners=True, padding_mode='zeros') composition and against the documented adjoint
formulas, and on the GPU against the kernels: value, du and dv, one-way and symmetric, on shapes around every launch
variant and workgroup edge, exact identities, a non-contiguous and a misaligned input, run-to-run bit-reproducibility,
infer.inverse_consistency_error and Registration3DModel(symmetric=True, inverse_consistency=w) eager and captured.

Which launch each GPU shape reaches (dfmir_invcons_fwd and dfmir_invcons_bwd select alike: <ND, VPT> of ic_fwd_k / ic_bwd_k;
VPT = 4 (16-byte loads of u, stores of du) when W % 4 == 0 and u (and du) are 16-byte aligned, else 1).  A workgroup owns
256 * VPT consecutive voxels of one sample in memory order: the kernels have ONE tile extent, along the flattened volume, and
no z chunk, so "-1, 0, +1 along each axis" is the voxel count of a sample around one workgroup -- 255 / 256 / 258 voxels for
VPT = 1 (257 is prime: no volume with every extent >= 2 has it) and, in steps of a 16-byte quad, 1020 / 1024 / 1028 for
VPT = 4 in 2-D; 1028 = 4 x 257 has no 3-D volume with W % 4 == 0, where the next one up is 1032.
  <3-D, VPT 1>  (2,3,3,4,5); (1,3,5,6,7); (1,3,13,17,19) 17 workgroups; (1,3,4,9,70) 10; (1,3,3,5,17) 255 voxels;
                (1,3,8,16,2) 256; (1,3,2,3,43) 258; the misaligned view of (1,3,4,4,64)
  <3-D, VPT 4>  (1,3,4,4,64) 1024 voxels; (1,3,3,3,260) 3 workgroups; (1,3,3,5,68) 1020; (1,3,3,43,8) 1032; the 16^3 model
  <2-D, VPT 1>  (2,2,3,3); (2,2,9,11); (1,2,37,41) 6 workgroups; (1,2,15,17) 255; (1,2,128,2) 256; (1,2,6,43) 258; the
                misaligned view of (1,2,16,64)
  <2-D, VPT 4>  (1,2,5,300) 2 workgroups; (1,2,15,68) 1020; (1,2,16,64) 1024; (1,2,257,4) 1028; the 32^2 model
ic_fin_k runs after every forward.  dv: the VPT 4 launches hand k r to the owner-gather warp adjoint (warp_win_bwd_own_k,
warp_win_gather_k, warp_win_slow_k), the VPT 1 launches scatter 64-bit fixed-point sums (ic_zero_k and ic_cvt_k around
ic_bwd_k); the misaligned views take the second way on shapes that otherwise take the first, and so does
test_invcons_fixed_point_dv_on_vector_shapes, which sets DFMIR_INVCONS_FIXED64 on VPT 4 launches.

Bit-reproducibility: the value (double slots added in a fixed order) and du (a gather) are bit-identical from run to run on
every shape.  dv is bit-identical wherever ops.warp's backward is (W % 4 == 0: the same kernels; all but voxels displaced
past the tiles around their own, none in these inputs) and, unlike it, on the other shapes too (integer sums do not depend
on the order of the adds).  test_invcons_bit_reproducible runs both ways.

Inputs come in two seeded families.  `lattice`: u = k + f, k integer-valued in [-3, 3], f uniform in [0.05, 0.95], v noise of
amplitude 2 -- every sample point lies at least 0.05 from a cell boundary (du has no kink nearby), many border voxels sample
outside the volume, nothing is excluded from any comparison.  `smooth`: u = three sinusoids of total amplitude 2 and
wavelength >= 12 voxels, v = -u plus 10 % noise, a realistic near-inverse pair; value and dv are continuous in the sample
position and are compared in full, du is piecewise constant in it, so for du only the voxels with a sample coordinate within
1e-4 of an integer on any axis are left out (at most 1 % per case: checked below on the CPU).

Tolerances (profiles/invcons_margins.txt): every comparison with the restatement is bounded by 4x the error of the SAME
definition evaluated by torch in fp32 on the CPU against the float64 restatement, on these inputs -- the maxima over the case
set, per family: the loss (relative), each gradient in relative 2-norm and as max-abs over max.  scripts/invcons_margins.py
measures them, and the kernels' own errors beside them."""
import ctypes
import itertools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import step3d
from tests.golden import common as C

DEV = "cuda"
FACTOR = 4.0
# profiles/invcons_margins.txt, rows "max" of the fp32 CPU columns: (loss, du 2-norm, du max, dv 2-norm, dv max)
FP32_ERR = {"lattice": (1.22e-07, 5.72e-06, 1.59e-05, 8.20e-06, 1.48e-05), "smooth": (3.77e-07, 3.75e-06, 1.03e-05, 7.02e-06, 1.83e-05)}
BOUND = {k: tuple(FACTOR * e for e in v) for k, v in FP32_ERR.items()}
FAMILIES = ("lattice", "smooth")

SHAPES_3D = [(2, 3, 3, 4, 5), (1, 3, 5, 6, 7), (1, 3, 13, 17, 19), (1, 3, 4, 9, 70), (1, 3, 4, 4, 64), (1, 3, 3, 3, 260)]
SHAPES_2D = [(2, 2, 3, 3), (2, 2, 9, 11), (1, 2, 37, 41), (1, 2, 5, 300)]
WG_SCALAR, WG_VECTOR = 256, 1024             # voxels of a workgroup: IC_T * VPT of invcons.hip
SHAPES_EDGE = [(1, 3, 3, 5, 17), (1, 3, 8, 16, 2), (1, 3, 2, 3, 43),          # 255, 256, 258 voxels, VPT 1
               (1, 3, 3, 5, 68), (1, 3, 3, 43, 8),                            # 1020, 1032 voxels, VPT 4 (1024: above)
               (1, 2, 15, 17), (1, 2, 128, 2), (1, 2, 6, 43),
               (1, 2, 15, 68), (1, 2, 16, 64), (1, 2, 257, 4)]                 # 1020, 1024, 1028 voxels, VPT 4
SHAPES = SHAPES_3D + SHAPES_2D + SHAPES_EDGE
EXCLUDE_WITHIN, EXCLUDE_CAP = 1e-4, 0.01


def _id(shape):
    return "x".join(str(v) for v in shape)


# ------------------------------------------------------------------------------------------ restatement
def _grid(vol, dtype):
    return torch.stack(torch.meshgrid(*[torch.arange(n, dtype=dtype) for n in vol], indexing='ij'), 0)


def _corners(u):
    """Per corner of the cell around x + u(x): (flat index into a channel of v, clamped; validity [B,*vol]; per-axis
    weights [B,nd,*vol]; the corner's bits).  Plain floor and integer arithmetic, in u's dtype."""
    B, nd = u.shape[:2]
    vol = tuple(u.shape[2:])
    f = _grid(vol, u.dtype)[None] + u
    i0 = torch.floor(f.detach())
    w1 = f - i0
    w = (1.0 - w1, w1)
    i0 = i0.long()
    strides = [math.prod(vol[a + 1:]) for a in range(nd)]
    for bits in itertools.product((0, 1), repeat=nd):
        flat = torch.zeros((B,) + vol, dtype=torch.long)
        valid = torch.ones((B,) + vol, dtype=torch.bool)
        for a in range(nd):
            ia = i0[:, a] + bits[a]
            valid &= (ia >= 0) & (ia < vol[a])
            flat += ia.clamp(0, vol[a] - 1) * strides[a]
        yield flat, valid, torch.stack([w[bits[a]][:, a] for a in range(nd)], 1), bits


def ic_residual(u, v):
    """r = u + v(x + u(x)) with explicit floor / gather indexing; corners outside the volume read as 0.  Differentiable."""
    B, nd = u.shape[:2]
    S = math.prod(u.shape[2:])
    vf = v.reshape(B, nd, S)
    r = u
    for flat, valid, w, _ in _corners(u):
        val = torch.gather(vf, 2, flat.reshape(B, 1, S).expand(B, nd, S)).reshape(u.shape)
        r = r + (w.prod(1) * valid.to(u.dtype))[:, None] * val
    return r


def ic_ref(u, v, symmetric=False):
    """IC(u, v), the mean of r^2 over all elements (symmetric: 0.5 (IC(u, v) + IC(v, u))), in the inputs' dtype."""
    loss = (ic_residual(u, v) ** 2).mean()
    if symmetric:
        loss = 0.5 * (loss + (ic_residual(v, u) ** 2).mean())
    return loss


def ic_loss_ref(u, v, symmetric=False, dtype=torch.float64):
    """(loss, du, dv) on the CPU in `dtype` (float64: the restatement; float32: the yardstick)."""
    a = u.detach().cpu().to(dtype).requires_grad_()
    b = v.detach().cpu().to(dtype).requires_grad_()
    loss = ic_ref(a, b, symmetric)
    loss.backward()
    return float(loss.detach()), a.grad, b.grad


def ic_grid_sample(u, v):
    """The same loss from F.grid_sample: normalised coordinates, align_corners=True, zero padding.  Shares no code with
    ic_residual."""
    nd = u.dim() - 2
    vol = tuple(u.shape[2:])
    f = _grid(vol, u.dtype)[None] + u
    norm = [2.0 * f[:, a] / (vol[a] - 1) - 1.0 for a in range(nd)]
    grid = torch.stack(norm[::-1], -1)                       # last axis: x, y(, z)
    warped = F.grid_sample(v, grid, mode='bilinear', padding_mode='zeros', align_corners=True)
    return ((u + warped) ** 2).mean()


def ic_adjoint(u, v):
    """(du, dv) by the documented formulas, k = 2 / (B nd S): du_c = k (r_c + sum_c' r_c' d_c v_c'), d_c = corner differences
    with zero-padded corners as zeros; dv = the interpolation's transpose applied to k r."""
    B, nd = u.shape[:2]
    S = math.prod(u.shape[2:])
    k = 2.0 / (B * nd * S)
    r = ic_residual(u, v).detach()
    vf = v.reshape(B, nd, S)
    du = k * r.clone()
    dv = torch.zeros(B, nd, S, dtype=u.dtype)
    for flat, valid, w, bits in _corners(u):
        val = torch.gather(vf, 2, flat.reshape(B, 1, S).expand(B, nd, S)).reshape(u.shape) * valid.to(u.dtype)[:, None]
        for c in range(nd):
            others = torch.ones_like(w[:, 0])
            for a in range(nd):
                if a != c:
                    others = others * w[:, a]
            du[:, c] += k * (1.0 if bits[c] else -1.0) * others * (r * val).sum(1)
        contrib = k * r * (w.prod(1) * valid.to(u.dtype))[:, None]
        dv.scatter_add_(2, flat.reshape(B, 1, S).expand(B, nd, S), contrib.reshape(B, nd, S))
    return du, dv.reshape(u.shape)


# ------------------------------------------------------------------------------------------ inputs
def _sinusoids(shape, seed):
    """Per (b, c) three sinusoids (2 / 3) sin(2 pi f . p + phase), every |f_a| <= 1 / 12; frequencies and phases seeded."""
    B, Cn = shape[:2]
    nd = len(shape) - 2
    f = (C.rand(seed, B, Cn, 3, nd).double() * 2.0 - 1.0) / 12.0
    ph = C.rand(seed + 1, B, Cn, 3).double() * 2.0 * math.pi
    arg = torch.einsum('bcka,a...->bck...', f, _grid(shape[2:], torch.float64)) * 2.0 * math.pi
    return (2.0 / 3.0 * torch.sin(arg + ph.reshape((B, Cn, 3) + (1,) * nd))).sum(2)


def fields(shape, family, seed=500):
    """(u, v) fp32 of a case."""
    seed = seed + 13 * SHAPES.index(shape) if shape in SHAPES else seed
    if family == "lattice":
        k = torch.floor(C.rand(seed, *shape).double() * 7.0).clamp(0, 6) - 3.0
        f = 0.05 + 0.9 * C.rand(seed + 1, *shape).double()
        u = (k + f).float()
        v = ((C.rand(seed + 2, *shape).double() * 2.0 - 1.0) * 2.0).float()
    else:
        u = _sinusoids(shape, seed).float()
        v = (-u.double() + 0.2 * (C.rand(seed + 2, *shape).double() * 2.0 - 1.0)).float()
    return u, v


def du_keep(u):
    """[B,1,*vol] mask of the voxels whose sample point x + u(x) stays more than EXCLUDE_WITHIN from an integer on every
    axis: where du is compared (smooth family)."""
    f = _grid(u.shape[2:], torch.float64)[None] + u.double()
    return ((f - torch.round(f)).abs() > EXCLUDE_WITHIN).all(1, keepdim=True)


def rel_errors(got, ref, keep=None):
    """(relative 2-norm error, max-abs error over max) of a gradient, over the kept voxels."""
    g, r = got.detach().cpu().double(), ref.double()
    if keep is not None:
        g, r = g * keep, r * keep
    return float((g - r).norm() / r.norm()), float((g - r).abs().max() / r.abs().max())


def all_errors(got, ref, keeps):
    """(loss, du 2-norm, du max, dv 2-norm, dv max) of (loss, du, dv) against the restatement's."""
    return ((abs(float(got[0]) - ref[0]) / abs(ref[0]),) + rel_errors(got[1], ref[1], keeps[0])
            + rel_errors(got[2], ref[2], keeps[1]))


_REF = {}


def reference(shape, family, symmetric=False):
    """(u, v, (loss64, du64, dv64), (keep_u, keep_v)) of a case, computed once and shared."""
    key = (shape, family, symmetric)
    if key not in _REF:
        u, v = fields(shape, family)
        keeps = (None, None)
        if family == "smooth":                    # symmetric: each field is also the sampling one of the other direction
            keeps = (du_keep(u), du_keep(v) if symmetric else None)
        _REF[key] = (u, v, ic_loss_ref(u, v, symmetric), keeps)
    return _REF[key]


def _gpu(u, v, symmetric=False):
    from dfmir_amd import ops
    a, b = u.to(DEV).requires_grad_(), v.to(DEV).requires_grad_()
    loss = ops.inverse_consistency(a, b, symmetric=symmetric)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), a.grad.cpu(), b.grad.cpu()


def _check(got, ref, keeps, family, what):
    e = all_errors(got, ref, keeps)
    b = BOUND[family]
    print("%s [%s]: loss %.3e (bound %.1e)  du l2 %.3e (%.1e) max %.3e (%.1e)  dv l2 %.3e (%.1e) max %.3e (%.1e)"
          % ((what, family) + tuple(x for p in zip(e, b) for x in p)))
    assert bool(torch.isfinite(got[1]).all()) and bool(torch.isfinite(got[2]).all()), what
    assert all(x <= y for x, y in zip(e, b)), (what, family, e)


# ------------------------------------------------------------------------------------------ CPU tier
def test_invcons_symbols_in_header_exports_and_ctypes_table():
    import dfmir_amd
    from dfmir_amd import _lib, infer, losses, ops
    from tests.test_abi import header_symbols
    h = ctypes.CDLL(dfmir_amd.LIB_PATH)
    for s in ("dfmir_invcons_ws_floats", "dfmir_invcons_fwd", "dfmir_invcons_bwd_ws_floats", "dfmir_invcons_bwd"):
        assert s in header_symbols() and s in _lib.exported_symbols() and hasattr(h, s), s
    lib = dfmir_amd.lib()
    assert lib.dfmir_abi_version() == 14
    assert lib.dfmir_invcons_ws_floats(3, 1, 16, 16, 16) == 3 * 16          # a double and an unsigned per 256 voxels
    assert lib.dfmir_invcons_ws_floats(2, 2, 999, 3, 3) == 3 * 2 * 1        # nd == 2: D is not read
    assert lib.dfmir_invcons_bwd_ws_floats(3, 2, 4, 5, 6) == 2 * 2 * 3 * 120
    for name in ("InverseConsistencyFn", "inverse_consistency", "inverse_consistency_per_sample"):
        assert hasattr(ops, name), name
    assert hasattr(losses, "InverseConsistency_Loss") and hasattr(infer, "inverse_consistency_error")
    crit = losses.InverseConsistency_Loss(dim=2, loss_mult=0.5)
    assert crit.name == 'ic' and crit.symmetric and crit.loss_mult == 0.5 and crit.dim == 2
    with pytest.raises(ValueError, match="dim"):
        losses.InverseConsistency_Loss(dim=4)


BAD_DIMS = ((1, 1, 8, 8, 8), (4, 1, 8, 8, 8), (3, 0, 8, 8, 8), (3, 1, 1, 8, 8), (3, 1, 8, 1, 8), (3, 1, 8, 8, 1), (2, 1, 1, 1, 8),
            (2, 1, 1, 8, 1), (3, 1, 1024, 1024, 1024))                # (nd, B, D, H, W)


def test_invcons_bad_arguments_are_invalid_without_a_device():
    import dfmir_amd
    lib = dfmir_amd.lib()
    for bad in BAD_DIMS:
        assert lib.dfmir_invcons_ws_floats(*bad) == -1 and lib.dfmir_invcons_bwd_ws_floats(*bad) == -1, bad
    buf = (ctypes.c_double * 64)()                      # host memory: an argument the checks refuse is never dereferenced
    p = ctypes.cast(buf, ctypes.c_void_p)
    for bad in BAD_DIMS:
        nd, dims = bad[0], bad[1:]
        assert lib.dfmir_invcons_fwd(nd, p, p, p, p, p, p, *dims, None) != 0, bad
        assert b"invalid argument" in lib.dfmir_last_error()
        assert lib.dfmir_invcons_bwd(nd, p, p, p, p, p, p, p, *dims, None) != 0, bad
        assert b"invalid argument" in lib.dfmir_last_error()
    good = (1, 8, 8, 8)
    for hole in range(6):                               # a NULL pointer in every position
        args = [p] * 6
        args[hole] = None
        assert lib.dfmir_invcons_fwd(3, *args, *good, None) != 0, hole
        assert b"invalid argument" in lib.dfmir_last_error()
    for args in ((None, p, p, p, p, p, p), (p, None, p, p, p, p, p), (p, p, None, p, p, p, p), (p, p, p, None, p, p, p),
                 (p, p, p, p, None, None, p), (p, p, p, p, p, p, None)):      # no gradient wanted at all; dv without scratch
        assert lib.dfmir_invcons_bwd(3, *args, *good, None) != 0, args
        assert b"invalid argument" in lib.dfmir_last_error()


def test_inverse_consistency_rejects_bad_arguments_before_any_launch():
    from dfmir_amd import infer, ops
    from dfmir_amd._lib import DfmirHipError
    from dfmir_amd.losses import InverseConsistency_Loss
    u = torch.rand(1, 3, 8, 8, 8)
    for fn in (ops.inverse_consistency, ops.inverse_consistency_per_sample):
        with pytest.raises(DfmirHipError, match="mismatch"):
            fn(u, torch.rand(1, 3, 8, 8, 9))
        with pytest.raises(DfmirHipError, match="mismatch"):
            fn(u, torch.rand(2, 3, 8, 8, 8))
        with pytest.raises(DfmirHipError, match="channels"):
            fn(torch.rand(1, 2, 8, 8, 8), torch.rand(1, 2, 8, 8, 8))
        with pytest.raises(DfmirHipError, match="channels"):
            fn(torch.rand(1, 3, 8, 8), torch.rand(1, 3, 8, 8))
        with pytest.raises(DfmirHipError, match="fp32"):
            fn(u.double(), u.double())
        with pytest.raises(DfmirHipError, match="fp32"):
            fn(u, u.half())
        with pytest.raises(DfmirHipError, match="no CPU fallback"):
            fn(u, u)
    with pytest.raises(ValueError, match="2-D field"):
        InverseConsistency_Loss(dim=3)(torch.rand(1, 2, 8, 8), torch.rand(1, 2, 8, 8))
    with pytest.raises(ValueError, match="anisotropic"):
        infer.inverse_consistency_error(u, u, spacing=(1.0, 1.0, 2.5))
    with pytest.raises(ValueError, match="positive"):
        infer.inverse_consistency_error(u, u, spacing=(1.0, 1.0))


def test_registration3d_symmetric_arguments():
    from dfmir_amd.losses import InverseConsistency_Loss
    from dfmir_amd.registration3d import Registration3DModel
    with pytest.raises(ValueError, match="symmetric=True"):
        Registration3DModel((8, 8, 8), device="cpu", inverse_consistency=1.0, symmetric=False)
    with pytest.raises(ValueError, match=">= 0"):
        Registration3DModel((8, 8, 8), device="cpu", inverse_consistency=-1.0, symmetric=True)
    m = Registration3DModel((8, 8, 8), device="cpu")
    assert m.netR.skip_unused_target and not m.symmetric and m._outputs == ('regA', 'flow', 'loss_ncc', 'loss_grad')
    m = Registration3DModel((8, 8, 8), device="cpu", symmetric=True)
    assert not m.netR.skip_unused_target and m._outputs == ('regA', 'flow', 'loss_ncc', 'loss_grad', 'regB', 'neg_flow')
    m = Registration3DModel((16, 16), device="cpu", symmetric=True, inverse_consistency=0.1, similarity='mind')
    assert isinstance(m.criterionIC, InverseConsistency_Loss) and m.criterionIC.dim == 2 and m.criterionIC.symmetric
    assert m._outputs[-3:] == ('regB', 'neg_flow', 'loss_ic') and m.ic_weight == 0.1


def test_vxmdense_returns_what_it_returned_without_the_keyword(monkeypatch):
    """The lengths of the returned tuples, with the kernels stubbed out (a CPU test: only the plumbing runs)."""
    from dfmir_amd import voxelmorph as V
    net = V.VxmDense((8, 8), [[2], [2, 2]], int_steps=2, bidir=True)
    flow = torch.full((1, 2, 8, 8), 0.5)
    monkeypatch.setattr(V.ops, "upcat_channels", lambda a, b: torch.cat([a, b], 1))
    monkeypatch.setattr(V.ops, "scale", lambda x, m: x * m)
    net.unet_model.forward = lambda x: x
    net.flow.forward = lambda x: flow
    net.resize = net.fullsize = None
    net.integrate.forward = lambda x, scale_folded=False: x
    net.transformer.forward = lambda src, fl: src
    a = torch.rand(1, 1, 8, 8)
    assert len(net.forward(a, a)) == 3 and len(net.forward(a, a, registration=True)) == 2
    out = net.forward(a, a, return_neg_flow=True)
    assert len(out) == 4 and out[3] is not None and torch.equal(out[3], -out[2])
    assert len(net.forward(a, a, registration=True, return_neg_flow=True)) == 2
    net.skip_unused_target = True
    out = net.forward(a, a, return_neg_flow=True)
    assert len(out) == 4 and out[1] is None and out[3] is None
    net.bidir = False
    assert len(net.forward(a, a)) == 2 and len(net.forward(a, a, return_neg_flow=True)) == 2


CPU_SHAPES = [(2, 3, 5, 6, 7), (1, 3, 3, 4, 9), (2, 2, 9, 11), (1, 2, 2, 2)]


@pytest.mark.parametrize("shape", CPU_SHAPES, ids=_id)
@pytest.mark.parametrize("family", FAMILIES)
def test_restatement_equals_the_grid_sample_composition_and_the_adjoint_formulas(shape, family):
    """Gradients against grid_sample's on the lattice family only: there no sample point lies near a cell boundary, where
    the normalised-coordinate round trip may pick the other cell (du is piecewise constant in the position)."""
    u, v = (t.double() for t in fields(shape, family, seed=71))
    loss, du, dv = ic_loss_ref(u, v)
    a, b = u.clone().requires_grad_(), v.clone().requires_grad_()
    lg = ic_grid_sample(a, b)
    lg.backward()
    assert loss > 0.0
    assert abs(float(lg.detach()) - loss) <= 1e-12 * loss
    assert float((b.grad - dv).abs().max()) <= 1e-12 * float(dv.abs().max())
    if family == "lattice":
        assert float((a.grad - du).abs().max()) <= 1e-12 * float(du.abs().max())
    fu, fv = ic_adjoint(u, v)
    assert float((fu - du).abs().max()) <= 1e-12 * float(du.abs().max())
    assert float((fv - dv).abs().max()) <= 1e-12 * float(dv.abs().max())
    ls = ic_loss_ref(u, v, symmetric=True)
    lr = ic_loss_ref(v, u)
    assert abs(ls[0] - 0.5 * (loss + lr[0])) <= 1e-14 * ls[0]
    assert float((ls[1] - 0.5 * (du + lr[2])).abs().max()) <= 1e-14 * float(du.abs().max())


def test_lattice_points_keep_their_distance_and_many_leave_the_volume():
    for shape in SHAPES:
        u, _ = fields(shape, "lattice")
        f = _grid(shape[2:], torch.float64)[None] + u.double()
        assert float((f - torch.round(f)).abs().min()) >= 0.05 - 1e-5, shape
        vol = torch.tensor(shape[2:], dtype=torch.float64).reshape((1, -1) + (1,) * (len(shape) - 2))
        outside = ((f < 0) | (f > vol - 1)).any(1)
        assert float(outside.double().mean()) > 0.05, shape


def test_smooth_seeds_stay_under_the_exclusion_cap():
    for shape in SHAPES:
        u, v = fields(shape, "smooth")
        assert float(u.abs().max()) <= 2.0 and float((u + v).abs().max()) <= 0.2 + 1e-6
        for t in (u, v):
            assert 1.0 - float(du_keep(t).double().mean()) <= EXCLUDE_CAP, shape


# ------------------------------------------------------------------------------------------ GPU tier
@pytest.mark.gpu
@pytest.mark.parametrize("symmetric", [False, True], ids=["oneway", "symmetric"])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_invcons_value_and_gradients_vs_restatement(shape, symmetric):
    for family in FAMILIES:
        u, v, ref, keeps = reference(shape, family, symmetric)
        _check(_gpu(u, v, symmetric), ref, keeps, family, _id(shape))


def _shifted_out(vol, s):
    """Number of voxels x of the volume whose x + s leaves it."""
    inside = 1
    for n, sa in zip(vol, s):
        inside *= max(n - abs(sa), 0)
    return math.prod(vol) - inside


@pytest.mark.gpu
@pytest.mark.parametrize("vol,s", [((6, 9, 70), (1, -2, 3)), ((5, 6, 64), (0, 0, -1)), ((4, 4, 8), (-4, 1, 1)), ((5, 68), (2, -3)),
                                   ((9, 11), (0, 1))], ids=["3d", "3d-vec", "3d-all-out", "2d-vec", "2d"])
def test_invcons_integer_shifts_count_the_voxels_that_leave(vol, s):
    nd = len(vol)
    u = torch.tensor(s, dtype=torch.float32).reshape((1, nd) + (1,) * nd).expand((2, nd) + vol).contiguous()
    loss, du, dv = _gpu(u, -u)
    S = math.prod(vol)
    want = np.float32(_shifted_out(vol, s) * float(sum(x * x for x in s)) / (nd * S))
    assert np.float32(float(loss)) == want, (float(loss), want)
    from dfmir_amd import ops
    per = ops.inverse_consistency_per_sample(u.to(DEV), (-u).to(DEV)).cpu()
    assert per.shape == (2,) and all(np.float32(float(p)) == want for p in per)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 3, 5, 6, 7), (1, 3, 4, 4, 64), (2, 2, 9, 11), (1, 2, 5, 300)], ids=_id)
def test_invcons_zero_fields_and_a_zero_second_field(shape):
    z = torch.zeros(shape)
    for symmetric in (False, True):
        loss, du, dv = _gpu(z, z, symmetric)
        assert float(loss) == 0.0 and float(du.abs().max()) == 0.0 and float(dv.abs().max()) == 0.0
    u = fields(shape, "lattice")[0]
    loss = float(_gpu(u, z)[0])
    want = float((u.double() ** 2).mean())
    err = abs(loss - want) / want
    print("IC(u, 0) against mean(u^2): %.3e (bound %.1e)" % (err, BOUND["lattice"][0]))
    assert err <= BOUND["lattice"][0]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 3, 3, 4, 5), (1, 3, 3, 3, 260), (2, 2, 9, 11), (1, 2, 5, 300)], ids=_id)
def test_invcons_symmetric_is_the_mean_of_the_two_directions_and_per_sample_averages(shape):
    from dfmir_amd import ops
    from dfmir_amd.losses import InverseConsistency_Loss
    u, v, ref, _ = reference(shape, "lattice")
    ab, ba, sym = _gpu(u, v), _gpu(v, u), _gpu(u, v, True)
    assert torch.equal(sym[0], (ab[0] + ba[0]) * 0.5)
    for got, want in ((sym[1], 0.5 * ab[1] + 0.5 * ba[2]), (sym[2], 0.5 * ab[2] + 0.5 * ba[1])):
        assert float((got - want).abs().max()) <= 1e-6 * float(want.abs().max())
    per = ops.inverse_consistency_per_sample(u.to(DEV), v.to(DEV))
    assert per.shape == (shape[0],) and not per.requires_grad
    assert abs(float(per.double().mean()) - float(ab[0])) <= 1e-6 * float(ab[0])
    per64 = (ic_residual(u.double(), v.double()) ** 2).flatten(1).mean(1)
    assert float(((per.cpu().double() - per64) / per64).abs().max()) <= BOUND["lattice"][0]
    nd = len(shape) - 2
    a, b = u.to(DEV).requires_grad_(), v.to(DEV).requires_grad_()
    loss = InverseConsistency_Loss(dim=nd, loss_mult=0.25)(a, b)
    loss.backward()
    assert abs(float(loss) - 0.25 * float(sym[0])) <= 1e-6 * float(sym[0])
    assert float((a.grad.cpu() - 0.25 * sym[1]).abs().max()) <= 1e-6 * float(sym[1].abs().max())
    plain = InverseConsistency_Loss(dim=nd, symmetric=False)(u.to(DEV), v.to(DEV))
    assert torch.equal(plain.cpu(), ab[0])


@pytest.mark.gpu
def test_invcons_gradient_to_one_field_only():
    from dfmir_amd import ops
    u, v, _, _ = reference((1, 3, 5, 6, 7), "lattice")
    want = _gpu(u, v)
    a = u.to(DEV).requires_grad_()
    (g,) = torch.autograd.grad(ops.inverse_consistency(a, v.to(DEV)), a)
    assert torch.equal(g.cpu(), want[1])
    b = v.to(DEV).requires_grad_()
    (g,) = torch.autograd.grad(ops.inverse_consistency(u.to(DEV), b), b)
    assert torch.equal(g.cpu(), want[2])


@pytest.mark.gpu
def test_invcons_non_contiguous_and_misaligned_inputs():
    from dfmir_amd import ops
    u, v, _, _ = reference((1, 3, 13, 17, 19), "lattice")
    want = _gpu(u, v)
    perm = (0, 1, 4, 3, 2)
    nu = u.permute(*perm).contiguous().to(DEV).permute(*perm).requires_grad_()
    nv = v.permute(*perm).contiguous().to(DEV).permute(*perm).requires_grad_()
    assert not nu.is_contiguous() and not nv.is_contiguous()
    loss = ops.inverse_consistency(nu, nv)
    loss.backward()
    assert torch.equal(loss.cpu(), want[0]) and torch.equal(nu.grad.cpu(), want[1]) and torch.equal(nv.grad.cpu(), want[2])
    # W % 4 == 0 but u starts 4 bytes off a 16-byte boundary: the scalar launch and the fixed-point dv.  The same arithmetic
    # per voxel (du to the bit); the value is summed over other workgroups and may differ in its last bit
    for shape in ((1, 3, 4, 4, 64), (1, 2, 16, 64)):
        u, v, ref, keeps = reference(shape, "lattice")
        want = _gpu(u, v)
        base = torch.empty(u.numel() + 1, device=DEV)
        off = base[1:].view(shape)
        off.copy_(u)
        assert off.is_contiguous() and off.data_ptr() % 16 == 4
        x, y = off.requires_grad_(), v.to(DEV).requires_grad_()
        loss = ops.inverse_consistency(x, y)
        gx, gy = torch.autograd.grad(loss, (x, y))
        torch.cuda.synchronize()
        _check((loss.detach().cpu(), gx.cpu(), gy.cpu()), ref, keeps, "lattice", "misaligned " + _id(shape))
        assert torch.equal(gx.cpu(), want[1])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 3, 4, 4, 64), (1, 3, 3, 3, 260), (1, 2, 5, 300), (1, 2, 257, 4)], ids=_id)
def test_invcons_fixed_point_dv_on_vector_shapes(shape):
    """DFMIR_INVCONS_FIXED64 on aligned W % 4 == 0 shapes: the VPT = 4 launch of ic_bwd_k with its own 64-bit fixed-point
    scatter for dv instead of the owner-gather warp adjoint.  Value and du come from the same arithmetic (to the bit); dv
    meets the same bounds and repeats itself."""
    from dfmir_amd import _lib
    want = {f: _gpu(*reference(shape, f)[:2]) for f in FAMILIES}
    _lib.set_option("DFMIR_INVCONS_FIXED64", "1")
    try:
        for family in FAMILIES:
            u, v, ref, keeps = reference(shape, family)
            got = _gpu(u, v)
            _check(got, ref, keeps, family, "fixed-point dv " + _id(shape))
            assert torch.equal(got[0], want[family][0]) and torch.equal(got[1], want[family][1])
            assert torch.equal(_gpu(u, v)[2], got[2])
    finally:
        _lib.set_option("DFMIR_INVCONS_FIXED64", None)


@pytest.mark.gpu
@pytest.mark.parametrize("vol", [(4, 5, 6), (3, 4, 8), (3, 8), (5, 7)], ids=_id)
def test_invcons_sample_points_exactly_on_the_padding_cell(vol):
    """Integer-valued u that puts border voxels at coordinate exactly -1 or n - 1 + 1 = n: the value and dv see weight 0 or
    a zero corner there (dv is exactly 0), du still has the corner-difference term (v[0] - 0) of the documented adjoint.
    u = -1 - x along one axis sends every voxel to -1, u = n - x to n (a whole cell outside: nothing is read).  v is the
    lattice family's noise and every sample point an integer in fp32 and float64 alike: that family's bounds."""
    nd = len(vol)
    shape = (1, nd) + vol
    v = ((C.rand(901, *shape).double() * 2.0 - 1.0) * 2.0).float()
    for axis in range(nd):
        for target in (-1.0, float(vol[axis])):
            u = torch.zeros(shape)
            u[:, axis] = target - _grid(vol, torch.float32)[axis]
            ref = ic_loss_ref(u, v)
            fu, fv = ic_adjoint(u.double(), v.double())
            assert float((fu - ref[1]).abs().max()) <= 1e-12 * float(ref[1].abs().max())
            if target < 0:
                assert float((ref[1] - 2.0 * u.double() / u.numel()).abs().max()) > 0.0       # the corner term is there
            got = _gpu(u, v)
            assert float(ref[2].abs().max()) == 0.0 and float(got[2].abs().max()) == 0.0     # every weight on v is 0
            e = (abs(float(got[0]) - ref[0]) / ref[0],) + rel_errors(got[1], ref[1])
            print("axis %d at %g of %s: loss %.3e  du l2 %.3e max %.3e" % ((axis, target, _id(shape)) + e))
            assert all(x <= y for x, y in zip(e, BOUND["lattice"][:3])), (axis, target, e)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 3, 13, 17, 19), (1, 3, 3, 3, 260), (1, 2, 37, 41), (1, 2, 5, 300)],
                         ids=["3d", "3d-vec", "2d", "2d-vec"])
def test_invcons_bit_reproducible(shape):
    for family in FAMILIES:
        u, v, _, _ = reference(shape, family)
        for symmetric in (False, True):
            r0, r1 = _gpu(u, v, symmetric), _gpu(u, v, symmetric)
            assert all(torch.equal(x, y) for x, y in zip(r0, r1)), (family, symmetric)


@pytest.mark.gpu
def test_inverse_consistency_error_on_a_hand_checked_case():
    """u = (3, 4) everywhere and v = 0: r = u, |r| = 5 at every voxel.  u = (0, 2), v = (0, -2) on 4 x 8: the two last columns
    sample outside the volume and keep |r| = 2, the others return exactly: RMS = sqrt(8 * 4 / 32) = 1."""
    from dfmir_amd import infer
    u = torch.tensor([3.0, 4.0]).reshape(1, 2, 1, 1).expand(2, 2, 6, 8).contiguous().to(DEV)
    z = torch.zeros_like(u)
    assert torch.equal(infer.inverse_consistency_error(u, z).cpu(), torch.tensor([5.0, 5.0]))
    assert torch.equal(infer.inverse_consistency_error(u, z, spacing=2.0).cpu(), torch.tensor([10.0, 10.0]))
    assert torch.equal(infer.inverse_consistency_error(u, z, spacing=(0.5, 0.5)).cpu(), torch.tensor([2.5, 2.5]))
    w = torch.tensor([0.0, 2.0]).reshape(1, 2, 1, 1).expand(1, 2, 4, 8).contiguous().to(DEV)
    assert torch.equal(infer.inverse_consistency_error(w, -w).cpu(), torch.tensor([1.0]))
    with pytest.raises(ValueError, match="anisotropic"):
        infer.inverse_consistency_error(u, z, spacing=(1.0, 2.0))


# ------------------------------------------------------------------------------------------ model
MODEL_CASES = [((16, 16, 16), 'ncc'), ((32, 32), 'mind')]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,similarity", MODEL_CASES, ids=["3d-ncc", "2d-mind"])
def test_registration3d_symmetric_ic_step_matches_restatement(shape, similarity):
    """Two eager steps: finite losses, 'ic' present and equal to the restatement on the model's own pair of fields (neither
    family: the bound is the larger of the two loss bounds)."""
    m, A, B = step3d.step_model(shape, similarity, symmetric=True, inverse_consistency=0.1)
    for _ in range(2):
        m.set_input({"A": A, "B": B})
        m.optimize_parameters()
        torch.cuda.synchronize()
        got = m.get_current_losses()
        assert sorted(got) == sorted(["grad", "ic", similarity]) and all(math.isfinite(x) for x in got.values()), got
        assert m.regB.shape == B.shape and m.neg_flow.shape == m.flow.shape
        ref = ic_loss_ref(m.flow, m.neg_flow, symmetric=True)[0]
        err = abs(got["ic"] - ref) / abs(ref)
        bound = max(BOUND["lattice"][0], BOUND["smooth"][0])
        print("step loss_ic %.4e: %.3e (bound %.1e)" % (got["ic"], err, bound))
        assert ref > 0.0 and err <= bound
    assert float(m.optimizer_R.flat_g.abs().max()) > 0.0


@pytest.mark.gpu
def test_registration3d_symmetric_nmi_with_seg_labels():
    """symmetric=True with similarity='nmi' and seg_labels, two eager steps at 16^3: every loss is there and finite, and
    'nmi' is 0.5 (NMI(real_B, y_source) + NMI(real_A, y_target)) -- the second term's argument order mirrors the first --
    evaluated again on the step's own outputs by the same kernels (fp32 sums of the same numbers: 1e-6)."""
    from tests.test_dice import SEG_LABELS, _seg_pair
    shape = (16, 16, 16)
    m, A, B = step3d.step_model(shape, 'nmi', symmetric=True, inverse_consistency=0.1, seg_labels=SEG_LABELS, seg_weight=0.7)
    A_seg, B_seg = (x.to(DEV) for x in _seg_pair(shape, 143))
    for _ in range(2):
        m.set_input({"A": A, "B": B, "A_seg": A_seg, "B_seg": B_seg})
        m.optimize_parameters()
        torch.cuda.synchronize()
        got = m.get_current_losses()
        assert sorted(got) == ["dice", "grad", "ic", "nmi"] and all(math.isfinite(x) for x in got.values()), got
        with torch.no_grad():
            want = 0.5 * (float(m.criterionNMI(B, m.regA.detach())) + float(m.criterionNMI(A, m.regB.detach())))
        assert abs(got["nmi"] - want) <= 1e-6 * abs(want), (got["nmi"], want)
        assert got["ic"] > 0.0 and m.neg_flow.shape == m.flow.shape
    assert float(m.optimizer_R.flat_g.abs().max()) > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("shape,similarity", MODEL_CASES, ids=["3d-ncc", "2d-mind"])
def test_registration3d_symmetric_ic_captured_step_matches_eager(shape, similarity):
    """symmetric=True, inverse_consistency=0.1 under capture_step=True: a replayed step equals the same step enqueued eagerly
    (the pattern and the tolerances of test_bending.py's captured-step test), for two steps."""
    m, A, B = step3d.step_model(shape, similarity, capture=True, symmetric=True, inverse_consistency=0.1)
    m.parallelize()
    step3d.assert_replay_matches_eager(m, {"A": A, "B": B}, ["grad", "ic", similarity],
                                       extra=(("regB", 1e-6), ("neg_flow", 1e-5)))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,similarity", MODEL_CASES, ids=["3d-ncc", "2d-mind"])
def test_registration3d_defaults_reproduce_the_one_directional_step(shape, similarity):
    """symmetric=False, inverse_consistency=0.0 spelled out against a model built without them: the first step's losses and
    the parameter arena after it, bit for bit (weight gradients summed in fixed point, so a step repeats itself)."""
    from dfmir_amd import ops
    was = ops.deterministic_wgrad()
    try:
        res = []
        for kw in ({}, dict(symmetric=False, inverse_consistency=0.0)):
            m, A, B = step3d.step_model(shape, similarity, deterministic_wgrad=True, **kw)
            m.set_input({"A": A, "B": B})
            m.optimize_parameters()
            torch.cuda.synchronize()
            assert not hasattr(m, "regB") and not hasattr(m, "loss_ic")
            res.append((m.get_current_losses(), m.optimizer_R.flat_p.clone()))
    finally:
        ops.set_deterministic_wgrad(was)
    assert res[0][0] == res[1][0] and sorted(res[0][0]) == sorted(["grad", similarity])
    assert torch.equal(res[0][1], res[1][1])
