"""JacobianDet_Loss / ops.jacobian_penalty, ops.jacobian_determinant, ops.jacobian_stats and infer.flow_regularity
(build-defined fold penalty, determinant map and regularity statistics, dfmir_amd/csrc/jacdet.hip): the C ABI and the
argument checks (CPU), a float64 restatement of the definition written with slicing, checked on the CPU against an
independent route (conv{2,3}d with [-0.5, 0, 0.5] kernels, torch.linalg.det on the stacked matrices, the documented
adjoint formula with cofactors from det * inverse^T) and on exactly representable affine fields, and on the GPU against
the kernels: value and gradient, map and statistics on shapes around the border and tile cases, exact identities on
affine fields, mask / loss_mult, a non-contiguous and a misaligned input, run-to-run bit-reproducibility,
refine_flow(fold_weight=...) and Registration3DModel(fold_weight=...) eager and captured.

Which launch each GPU shape reaches (the four entry points select alike: <ND3, VEC> of jac_fwd_k<., ., MODE> /
jac_bwd_k; ND3 = a 3-D field, VEC = W % 4 == 0 and a 16-byte aligned field; the tile is 8 (y) x 64 (x), a z chunk 16 planes):
  <3-D, scalar>  (2,3,3,3,3) one voxel of Omega; (1,3,5,6,7); (2,3,13,17,19) three tiles along y, border 1 and 2;
                 (1,3,4,9,70) two tiles along y and x; (1,3,4,H,6) H = 7, 8, 9; (1,3,4,4,W) W = 63, 65; (6,9,70); the
                 misaligned view
  <3-D, vector>  (1,3,3,3,260) five tiles along x; (1,3,D,5,8) D = 15, 16, 17 (one / one / two z chunks); (1,3,4,4,64);
                 the refine_flow volume (12,14,16); the 16^3 model steps
  <2-D, scalar>  (2,2,3,3); (2,2,9,11); (1,2,37,41) border 1 and 2; (1,2,H,10) H = 7, 8, 9; (1,2,5,W) W = 63, 65; the
                 misaligned view
  <2-D, vector>  (1,2,5,300); (1,2,5,64); (5,68); the refine_flow plane (20,24); the 16^2 model step
df_slot_mean_k (common.h) runs after every penalty forward, jac_stats_fin_k after every statistics call.

Inputs come in two seeded families, generated in float64 and cast to fp32: per channel three sinusoids of wavelength 12
to 24 voxels per axis whose amplitudes add up to 3 voxels (`fold`: 5-25 % of the voxels fold, det J from about -1.9
to 7.5) or to 0.5 (`mild`: none does, and every determinant stays above 0.5, so a mild field checks that the three penalties and their gradients are exactly
0).  Conditions on the inputs, asserted on the float64 restatement before the GPU is looked at (input_conditions):
  C1  no voxel of Omega has |d64| < 1e-4 (the fp32 determinant lies within 2e-6 of the float64 one on these fields), so the
      GPU count of d <= 0 must equal the float64 count exactly and the power = 1 gradient does not sit on the hinge; every
      `fold` case has a voxel with d64 <= -0.1 (the losses with eps = 0 are then no rounding noise of a fold that barely
      is one), and at least 5 % folded and 5 % unfolded voxels where Omega has more than 200 voxels;
  C2  d64 + log_offset >= 0.1 where the log statistics are compared (`mild` with offset 0, `fold` with offset 3).
Tolerances (profiles/jacobian_margins.txt): every comparison with the restatement is bounded by 4x the error of the SAME
definition evaluated by torch in fp32 on the CPU against the float64 restatement, on these inputs -- the maxima over the
case set, per family.  scripts/jacobian_margins.py measures them, and the kernels' own errors beside them."""
import ctypes
import fractions
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

from tests.golden import common as C
from tests.test_bending import rel_errors

DEV = "cuda"
FACTOR = 4.0
GUARD = 1e-4
# profiles/jacobian_margins.txt, rows "max" of the fp32 CPU columns: loss (relative), gradient 2-norm, gradient max-abs over
# max; then absolute: the map, min d, max d, mean d, mean l, std l.  (fold mean l and std l: torch's fp32 sums came out
# differently on two CPUs, the file's notes give both figures and the smaller one stands here.  The mild penalty entries are
# 0 and unused: every penalty of a mild field is exactly 0, which the tests assert as such.)
FP32_ERR = {"fold": (6.02e-07, 5.57e-07, 8.88e-07, 8.77e-07, 9.49e-08, 4.20e-07, 1.35e-07, 1.73e-07, 1.61e-08),
            "mild": (0.0, 0.0, 0.0, 3.26e-07, 1.32e-07, 1.60e-07, 1.67e-07, 8.31e-08, 1.52e-08)}
BOUND = {k: tuple(FACTOR * e for e in v) for k, v in FP32_ERR.items()}
FAMILIES = ("fold", "mild")
AMPLITUDE = {"fold": 3.0, "mild": 0.5}
LOG_OFFSET = {"fold": 3.0, "mild": 0.0}
COMBOS = ((2, 0.0), (2, 0.5), (1, 0.0))          # (power, eps)

TILE_Y, TILE_X, CHUNK_Z = 8, 64, 16          # TY, TX, ZC of csrc/stencil_tile.h
SHAPES_3D = ([(2, 3, 3, 3, 3), (1, 3, 5, 6, 7), (2, 3, 13, 17, 19), (1, 3, 4, 9, 70), (1, 3, 3, 3, 260)] +
             [(1, 3, d, 5, 8) for d in (CHUNK_Z - 1, CHUNK_Z, CHUNK_Z + 1)] +
             [(1, 3, 4, h, 6) for h in (TILE_Y - 1, TILE_Y, TILE_Y + 1)] +
             [(1, 3, 4, 4, w) for w in (TILE_X - 1, TILE_X, TILE_X + 1)])
SHAPES_2D = ([(2, 2, 3, 3), (2, 2, 9, 11), (1, 2, 37, 41), (1, 2, 5, 300)] +
             [(1, 2, h, 10) for h in (TILE_Y - 1, TILE_Y, TILE_Y + 1)] +
             [(1, 2, 5, w) for w in (TILE_X - 1, TILE_X, TILE_X + 1)])
SHAPES = SHAPES_3D + SHAPES_2D
MID = ((2, 3, 13, 17, 19), (1, 2, 37, 41))
CASES = [(s, 1) for s in SHAPES] + [(s, 2) for s in MID]          # (shape, border)
# one seed per shape, the first of 300 + 11 i + 1000 k at which C1 and C2 hold (input_conditions asserts them)
SEEDS = (21300, 311, 1322, 333, 1344, 5355, 1366, 1377, 2388, 399, 1410, 3421, 432, 443,
         3454, 465, 1476, 487, 1498, 4509, 6520, 531, 5542, 553)
assert len(SEEDS) == len(SHAPES)


def _id(case):
    return "x".join(str(v) for v in case[0]) + "-b%d" % case[1]


# ------------------------------------------------------------------------------------------ restatement
def jacdet_ref(u, border=1):
    """d = det(I + central differences of u) on Omega_border, [B,*omega], with slicing, in u's dtype, differentiable."""
    nd, m, sp = u.dim() - 2, border, tuple(u.shape[2:])
    assert u.shape[1] == nd and all(n >= 2 * m + 1 for n in sp)

    def at(a, b, s):
        return u[(slice(None), a) + tuple(slice(m + (s if i == b else 0), n - m + (s if i == b else 0)) for i, n in enumerate(sp))]

    J = [[(at(a, b, 1) - at(a, b, -1)) / 2.0 + (1.0 if a == b else 0.0) for b in range(nd)] for a in range(nd)]
    if nd == 2:
        return J[0][0] * J[1][1] - J[0][1] * J[1][0]
    return (J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) + J[0][1] * (J[1][2] * J[2][0] - J[1][0] * J[2][2])
            + J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]))


def penalty_ref(u, eps=0.0, power=2, border=1):
    """mean over (B, Omega) of max(0, eps - d)^power; the hinge has derivative 0 at d == eps."""
    e = eps - jacdet_ref(u, border)
    e = torch.where(e > 0, e, torch.zeros_like(e))
    return (e * e if power == 2 else e).mean()


def penalty_loss_ref(u, eps, power, border, dtype=torch.float64):
    """(loss, dL/du) of the definition on the CPU in `dtype` (float64: the restatement; float32: the yardstick)."""
    x = u.detach().cpu().to(dtype).requires_grad_()
    loss = penalty_ref(x, eps, power, border)
    loss.backward()
    return float(loss.detach()), x.grad


def stats_ref(u, border=1, log_offset=0.0, log_floor=1e-9):
    """[B,6] in u's dtype: count of d <= 0, min, max, mean of d, mean and population std (numpy's default) of l."""
    d = jacdet_ref(u, border).reshape(u.shape[0], -1)
    l = torch.log(torch.clamp(d + log_offset, min=log_floor))
    return torch.stack([(d <= 0).to(d.dtype).sum(1), d.min(1).values, d.max(1).values, d.mean(1), l.mean(1),
                        l.std(1, unbiased=False)], 1)


def detmap_ref(u, border=1):
    """[B,1,*vol]: d on Omega, 1 outside."""
    out = torch.ones((u.shape[0],) + tuple(u.shape[2:]), dtype=u.dtype)
    out[(slice(None),) + tuple(slice(border, n - border) for n in u.shape[2:])] = jacdet_ref(u, border)
    return out[:, None]


def jacdet_conv(u, border=1):
    """(d, J) from stock conv ops and torch.linalg.det: every difference a [-0.5, 0, 0.5] kernel embedded in a 3^nd one,
    so a valid convolution lands on Omega_1; J is [B,*omega,nd,nd].  Shares no code with jacdet_ref."""
    nd, B, sp = u.dim() - 2, u.shape[0], tuple(u.shape[2:])
    conv = F.conv3d if nd == 3 else F.conv2d
    x = u.reshape((B * nd, 1) + sp)
    d1 = torch.tensor([-0.5, 0.0, 0.5], dtype=u.dtype)
    mid = torch.tensor([0.0, 1.0, 0.0], dtype=u.dtype)
    crop = (slice(None), slice(None)) + tuple(slice(border - 1, n - 2 - (border - 1)) for n in sp)
    cols = []
    for b in range(nd):
        k = None
        for i in range(nd):
            v = d1 if i == b else mid
            k = v if k is None else torch.tensordot(k, v, dims=0)
        g = conv(x, k[None, None])
        cols.append(g.reshape((B, nd) + tuple(g.shape[2:]))[crop])
    J = torch.stack(cols, -1).movedim(1, -2) + torch.eye(nd, dtype=u.dtype)
    return torch.linalg.det(J), J


def penalty_adjoint(u, eps=0.0, power=2, border=1):
    """dL/du by the documented formula: W = psi'(d) cof(J) on Omega, extended by 0, pushed back through the transposed
    central differences.  The cofactors come from d * inverse(J)^T, not from the written-out minors."""
    nd, sp, m = u.dim() - 2, tuple(u.shape[2:]), border
    d, J = jacdet_conv(u, border)
    cof = d[..., None, None] * torch.linalg.inv(J).transpose(-1, -2)
    e = torch.clamp(eps - d, min=0.0)
    dpsi = -2.0 * e if power == 2 else -(e > 0).to(u.dtype)
    Wm = dpsi[..., None, None] * cof
    inner = (slice(None),) + tuple(slice(m, n - m) for n in sp)

    def shifted(U, b, s):
        """p -> U(p + s e_b), zero where p + s e_b leaves the volume."""
        P = F.pad(U, tuple(v for _ in range(nd) for v in (1, 1)))
        return P[(slice(None),) + tuple(slice(1 + (s if i == b else 0), 1 + (s if i == b else 0) + n) for i, n in enumerate(sp))]

    g = torch.zeros_like(u)
    for a in range(nd):
        for b in range(nd):
            Wab = torch.zeros((u.shape[0],) + sp, dtype=u.dtype)
            Wab[inner] = Wm[..., a, b]
            g[:, a] += shifted(Wab, b, -1) - shifted(Wab, b, 1)
    return g / (2.0 * d.numel())


def sin_field(shape, seed, amplitude):
    """Per (b, channel) the sum of three sinusoids (amplitude / 3) sin(2 pi f . p + phase): |f_a| = 1 / wavelength with a
    wavelength in [12, 24] voxels and a random sign per axis, frequencies and phases seeded.  float64."""
    B, Cn = shape[:2]
    nd = len(shape) - 2
    lam = 12.0 + 12.0 * C.rand(seed, B, Cn, 3, nd).double()
    sign = torch.where(C.rand(seed + 1, B, Cn, 3, nd) < 0.5, -1.0, 1.0).double()
    ph = C.rand(seed + 2, B, Cn, 3).double() * 2.0 * math.pi
    grid = torch.stack(torch.meshgrid(*[torch.arange(n, dtype=torch.float64) for n in shape[2:]], indexing='ij'), 0)
    arg = torch.einsum('bcka,a...->bck...', sign / lam, grid) * 2.0 * math.pi + ph.reshape((B, Cn, 3) + (1,) * nd)
    return (amplitude / 3.0) * torch.sin(arg).sum(2)


def field(shape, family, seed=None):
    """The fp32 field of a shape and family; a shape of the case set has its own seed."""
    seed = SEEDS[SHAPES.index(shape)] if seed is None else seed
    return sin_field(shape, seed + (0 if family == "fold" else 5), AMPLITUDE[family]).float()


_REF = {}


def reference(case, family):
    """dict(u, d [B,*omega] float64, map, stats [B,6] with the family's log offset) of a case, computed once and shared."""
    key = (case, family)
    if key not in _REF:
        shape, border = case
        u = field(shape, family)
        x = u.double()
        _REF[key] = dict(u=u, d=jacdet_ref(x, border), map=detmap_ref(x, border),
                         stats=stats_ref(x, border, LOG_OFFSET[family]))
    return _REF[key]


def penalty_reference(case, family, combo):
    """(loss64, grad64) of a case under (power, eps), computed once and shared."""
    key = (case, family, combo)
    if key not in _REF:
        _REF[key] = penalty_loss_ref(reference(case, family)["u"], combo[1], combo[0], case[1])
    return _REF[key]


def input_conditions(case, family):
    """C1 and C2 on the float64 restatement (module docstring); returns the folded fraction."""
    d = reference(case, family)["d"]
    folded = float((d <= 0).double().mean())
    assert float(d.abs().min()) >= GUARD, ("C1", _id(case), family, float(d.abs().min()))
    assert float(d.min()) + LOG_OFFSET[family] >= 0.1, ("C2", _id(case), family, float(d.min()))
    if family == "mild":                 # every d64 clears 0.5 as well: all three penalties of a mild field are exactly 0
        assert folded == 0.0 and float(d.min()) >= 0.5 + GUARD, (_id(case), float(d.min()))
    else:
        assert float(d.min()) <= -0.1, ("no fold of depth 0.1", _id(case), float(d.min()))
        if d.numel() > 200:
            assert 0.05 <= folded <= 0.95, (_id(case), folded)
    return folded


def _gpu(u, eps=0.0, power=2, border=1):
    from dfmir_amd import ops
    x = u.to(DEV).requires_grad_()
    loss = ops.jacobian_penalty(x, eps, power, border)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), x.grad.cpu()


def _check(got, ref, family, what):
    el, l2, mx = rel_errors(got[0], got[1], ref[0], ref[1])
    b = BOUND[family]
    print("%s [%s]: loss %.3e (bound %.1e)  grad l2 %.3e (%.1e)  grad max %.3e (%.1e)" % (what, family, el, b[0], l2, b[1], mx, b[2]))
    assert bool(torch.isfinite(got[1]).all()), what
    assert el <= b[0] and l2 <= b[1] and mx <= b[2], (what, family, el, l2, mx)


def stat_errors(got, ref):
    """Absolute errors of (min d, max d, mean d, mean l, std l) between two [B,6] tables, the maxima over the samples."""
    return tuple(float((got[:, k].double() - ref[:, k].double()).abs().max()) for k in range(1, 6))


# ------------------------------------------------------------------------------------------ CPU tier
SYMBOLS = ("dfmir_jacdet_ws_floats", "dfmir_jacdet_fwd", "dfmir_jacdet_bwd", "dfmir_jacdet_map", "dfmir_jacdet_stats")


def test_jacdet_symbols_in_header_exports_and_ctypes_table():
    import dfmir_amd
    from dfmir_amd import _lib
    from tests.test_abi import header_symbols
    h = ctypes.CDLL(dfmir_amd.LIB_PATH)
    for s in SYMBOLS:
        assert s in header_symbols() and s in _lib.exported_symbols() and hasattr(h, s), s
    lib = dfmir_amd.lib()
    assert lib.dfmir_abi_version() == 14
    ws = lib.dfmir_jacdet_ws_floats                                  # 7 doubles per (sample, chunk, tile)
    assert ws(3, 1, 16, 16, 16) == 14 * 1 * 1 * 2 * 1
    assert ws(2, 2, 1, 9, 65) == 14 * 2 * 1 * 2 * 2 and ws(2, 2, 999, 9, 65) == ws(2, 2, 1, 9, 65)      # D is not read in 2-D
    assert ws(3, 1, 17, 3, 3) == 14 * 2
    for bad in ((4, 1, 8, 8, 8), (1, 1, 8, 8, 8), (3, 1, 2, 8, 8), (3, 1, 8, 2, 8), (3, 1, 8, 8, 2), (2, 1, 1, 8, 2), (2, 1, 1, 2, 8),
                (3, 0, 8, 8, 8), (3, 1, 1024, 1024, 1024), (2, 1, 1, 32768, 32768)):
        assert ws(*bad) == -1, bad


def _refused(lib, p, which=("fwd", "bwd", "map", "stats"), nd=3, dims=(1, 8, 8, 8), border=1, eps=0.0, power=2, off=0.0,
             floor=1e-9):
    """Every entry point of `which` returns "invalid argument" on this argument set."""
    calls = dict(fwd=lambda: lib.dfmir_jacdet_fwd(nd, p, p, p, *dims, border, eps, power, None),
                 bwd=lambda: lib.dfmir_jacdet_bwd(nd, p, p, p, *dims, border, eps, power, None),
                 map=lambda: lib.dfmir_jacdet_map(nd, p, p, *dims, border, None),
                 stats=lambda: lib.dfmir_jacdet_stats(nd, p, p, p, *dims, border, off, floor, None))
    return all(calls[name]() != 0 and b"invalid argument" in lib.dfmir_last_error() for name in which)


def test_jacdet_bad_arguments_are_invalid_without_a_device():
    import dfmir_amd
    lib = dfmir_amd.lib()
    assert _refused(lib, None)
    buf = (ctypes.c_double * 64)()                      # host memory: an argument the checks refuse is never dereferenced
    p = ctypes.cast(buf, ctypes.c_void_p)
    nan, inf = float('nan'), float('inf')
    for kw in (dict(nd=1), dict(nd=4), dict(dims=(1, 2, 8, 8)), dict(dims=(1, 8, 8, 2)), dict(nd=2, dims=(1, 1, 8, 2)),
               dict(dims=(1, 8, 8, 4), border=2), dict(border=0), dict(border=-1), dict(dims=(0, 8, 8, 8)),
               dict(dims=(1, 1024, 1024, 1024)), dict(nd=2, dims=(1, 1, 32768, 32768))):
        assert _refused(lib, p, **kw), kw
    for kw in (dict(power=0), dict(power=3), dict(eps=-1.0), dict(eps=nan), dict(eps=inf)):
        assert _refused(lib, p, ("fwd", "bwd"), **kw), kw
    for kw in (dict(off=-1.0), dict(off=nan), dict(off=inf), dict(floor=0.0), dict(floor=-1.0), dict(floor=nan), dict(floor=inf)):
        assert _refused(lib, p, ("stats",), **kw), kw


def test_jacobian_rejects_bad_arguments_before_any_launch():
    from dfmir_amd import infer, ops
    from dfmir_amd._lib import DfmirHipError
    from dfmir_amd.losses import JacobianDet_Loss
    x = torch.rand(1, 3, 8, 8, 8)
    calls = (ops.jacobian_penalty, ops.jacobian_determinant, ops.jacobian_stats, infer.flow_regularity,
             lambda t, **kw: JacobianDet_Loss(dim=t.dim() - 2, **kw)(t))
    for fn in calls[:4]:
        with pytest.raises(ValueError, match="displacement field"):
            fn(torch.rand(1, 2, 8))
    for fn in calls:
        with pytest.raises(ValueError, match="refused, not reinterpreted"):
            fn(torch.rand(1, 3, 1, 8, 8))
        with pytest.raises(ValueError, match="channels"):
            fn(torch.rand(1, 3, 8, 8))
        for shape in ((1, 3, 2, 8, 8), (1, 3, 8, 2, 8), (1, 3, 8, 8, 2), (1, 2, 8, 2)):
            with pytest.raises(ValueError, match="2 \\* border \\+ 1"):
                fn(torch.rand(*shape))
        with pytest.raises(ValueError, match="2 \\* border \\+ 1"):
            fn(torch.rand(1, 3, 8, 8, 4), border=2)
        for bad in (0, -1, 1.0, True, "1"):
            with pytest.raises(ValueError, match="border"):
                fn(x, border=bad)
        with pytest.raises(ValueError, match="2\\^31"):
            fn(torch.empty(1, 3, 1024, 1024, 1024, device="meta"))
        with pytest.raises(DfmirHipError, match="no CPU fallback"):
            fn(x)
        with pytest.raises(DfmirHipError, match="no CPU fallback"):
            fn(torch.rand(2, 2, 9, 11), border=2)
    for kw in (dict(power=3), dict(power=0), dict(power=True), dict(eps=-0.1), dict(eps=float('nan')), dict(eps=float('inf')),
               dict(eps="0")):
        with pytest.raises(ValueError, match="power|eps"):
            ops.jacobian_penalty(x, **kw)
        with pytest.raises(ValueError, match="power|eps"):
            JacobianDet_Loss(dim=3, **kw)
    for kw in (dict(log_offset=-1.0), dict(log_offset=float('nan')), dict(log_floor=0.0), dict(log_floor=-1e-9),
               dict(log_floor=float('inf'))):
        with pytest.raises(ValueError, match="log_offset|log_floor"):
            ops.jacobian_stats(x, **kw)
    with pytest.raises(ValueError, match="log_offset"):
        infer.flow_regularity(x, log_offset=-3.0)
    with pytest.raises(ValueError, match="dim"):
        JacobianDet_Loss(dim=4)
    with pytest.raises(ValueError, match="2-D field"):
        JacobianDet_Loss(dim=3)(torch.rand(1, 2, 8, 8))
    crit = JacobianDet_Loss(dim=2, eps=0.5, power=1, border=2, loss_mult=0.5)
    assert (crit.name, crit.dim, crit.eps, crit.power, crit.border, crit.loss_mult) == ('jacdet', 2, 0.5, 1, 2, 0.5)
    d = JacobianDet_Loss()
    assert (d.dim, d.eps, d.power, d.border, d.loss_mult) == (3, 0.0, 2, 1, None)


def test_refine_flow_rejects_bad_fold_arguments_before_any_launch():
    from dfmir_amd import infer
    img = torch.rand(1, 1, 8, 8, 8)
    for bad in (-1.0, float('nan'), float('inf'), "1", True):
        with pytest.raises(ValueError, match="fold_weight"):
            infer.refine_flow(img, img, lam=0.0, lr=0.1, features='intensity', fold_weight=bad)
    with pytest.raises(ValueError, match="power"):
        infer.refine_flow(img, img, lam=0.0, lr=0.1, features='intensity', fold_weight=1.0, fold_power=3)
    with pytest.raises(ValueError, match="eps"):
        infer.refine_flow(img, img, lam=0.0, lr=0.1, features='intensity', fold_weight=1.0, fold_eps=-1.0)
    small = torch.rand(1, 1, 2, 8, 8)
    with pytest.raises(ValueError, match="at least 3"):
        infer.refine_flow(small, small, lam=0.0, lr=0.1, features='intensity', grid_downsize=1, fold_weight=1.0)


def test_registration3d_constructs_with_a_fold_term_last():
    from dfmir_amd.losses import JacobianDet_Loss
    from dfmir_amd.registration3d import Registration3DModel
    plain = Registration3DModel((8, 8, 8), device="cpu")
    assert [k for k, _, _ in plain._terms] == ['ncc', 'grad'] and 'loss_fold' not in plain._outputs
    assert plain._outputs == ('regA', 'flow', 'loss_ncc', 'loss_grad') and not hasattr(plain, 'criterionFold')
    m = Registration3DModel((8, 8, 8), device="cpu", fold_weight=0.1)
    assert m._outputs[-1] == 'loss_fold' and m._outputs[:-1] == plain._outputs
    assert [(k, w) for k, w, _ in m._terms] == [('ncc', 1), ('grad', 1.0), ('fold', 0.1)]
    assert isinstance(m.criterionFold, JacobianDet_Loss) and (m.criterionFold.dim, m.criterionFold.eps, m.criterionFold.power) == (3, 0.0, 2)
    m2 = Registration3DModel((8, 8), device="cpu", similarity='mind', symmetric=True, inverse_consistency=0.5, seg_labels=[1, 2],
                             seg_weight=1.0, fold_weight=2.0, fold_eps=1.0, fold_power=1)
    assert [k for k, _, _ in m2._terms] == ['mind', 'grad', 'ic', 'dice', 'fold'] and m2._outputs[-1] == 'loss_fold'
    assert (m2.criterionFold.dim, m2.criterionFold.eps, m2.criterionFold.power) == (2, 1.0, 1)
    for bad in (-0.5, float('nan'), float('inf')):
        with pytest.raises(ValueError, match="fold_weight"):
            Registration3DModel((8, 8, 8), device="cpu", fold_weight=bad)
    with pytest.raises(ValueError, match="power"):
        Registration3DModel((8, 8, 8), device="cpu", fold_weight=1.0, fold_power=3)


@pytest.mark.parametrize("shape", [(2, 3, 5, 6, 7), (1, 3, 3, 3, 9), (2, 2, 9, 11), (1, 2, 3, 3), (1, 3, 7, 6, 8)],
                         ids=["3d", "3d-thin", "2d", "2d-one", "3d-b2"])
@pytest.mark.parametrize("combo", COMBOS, ids=["p2e0", "p2e05", "p1e0"])
@pytest.mark.parametrize("family", FAMILIES)
def test_restatement_equals_the_conv_composition_and_the_adjoint_formula(shape, combo, family):
    power, eps = combo
    border = 2 if shape == (1, 3, 7, 6, 8) else 1
    u = field(shape, family, seed=44).double()
    d = jacdet_ref(u, border)
    dc, _ = jacdet_conv(u, border)
    assert d.shape == dc.shape and float((d - dc).abs().max()) <= 1e-12 * float(d.abs().max())
    assert float((eps - d).abs().min()) >= GUARD                # (the three routes place the hinge alike)
    loss, g = penalty_loss_ref(u, eps, power, border)
    e = torch.clamp(eps - dc, min=0.0)
    lc = float((e * e if power == 2 else e).mean())
    assert abs(lc - loss) <= 1e-12 * max(loss, 1e-300)
    ga = penalty_adjoint(u, eps, power, border)
    gmax = float(g.abs().max())
    assert float((ga - g).abs().max()) <= 1e-12 * gmax
    if family == "fold" and d.numel() > 100:
        assert loss > 0.0 and gmax > 0.0
    s = stats_ref(u, border, 3.0)
    l = torch.log(torch.clamp(dc + 3.0, min=1e-9)).reshape(u.shape[0], -1).numpy()
    assert abs(float(s[0, 5]) - float(l[0].std())) <= 1e-12 and abs(float(s[0, 4]) - float(l[0].mean())) <= 1e-12


def _affine_field(vol, A):
    """u = A x on the grid of `vol` (float64): channel a = sum_b A[a][b] p_b."""
    g = torch.meshgrid(*[torch.arange(n, dtype=torch.float64) for n in vol], indexing='ij')
    return torch.stack([sum(float(A[a][b]) * g[b] for b in range(len(vol))) for a in range(len(vol))], 0)[None]


def _det_fraction(M):
    """The Leibniz determinant of a small matrix of Fractions."""
    n, tot = len(M), fractions.Fraction(0)
    for perm in itertools.permutations(range(n)):
        sign = (-1) ** sum(perm[i] > perm[j] for i in range(n) for j in range(i + 1, n))
        term = fractions.Fraction(sign)
        for i in range(n):
            term *= M[i][perm[i]]
        tot += term
    return tot


DYADIC = (((-2, 0, 0), (0, 0, 0), (0, 0, 0)), ((0.5, 0.25, 0), (0, -0.5, 1), (0.125, 0, 1)),
          ((0, 1, 0), (-1, 0, 0.5), (2, 0, -2.5)), ((0.5, -0.75), (1.25, -2)), ((0, -1), (1, 0)))


@pytest.mark.parametrize("A", DYADIC, ids=lambda A: "%dd" % len(A))
def test_restatement_is_exact_on_dyadic_affine_fields(A):
    nd = len(A)
    want = float(_det_fraction([[fractions.Fraction(A[a][b]) + (1 if a == b else 0) for b in range(nd)] for a in range(nd)]))
    for border in (1, 2):
        d = jacdet_ref(_affine_field((6, 7, 9)[-nd:], A), border)
        assert d.numel() > 0 and bool((d == want).all()), (A, want)
        assert float(jacdet_conv(_affine_field((6, 7, 9)[-nd:], A), border)[0].sub(want).abs().max()) <= 1e-14 * max(1.0, abs(want))


def test_input_families_meet_their_conditions():
    """C1 and C2 on every case (the GPU tests assert them again where they lean on them)."""
    for case in CASES:
        for family in FAMILIES:
            input_conditions(case, family)


# ------------------------------------------------------------------------------------------ GPU tier
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_jacobian_penalty_value_and_gradient_vs_restatement(case):
    shape, border = case
    for family in FAMILIES:
        input_conditions(case, family)
        u = reference(case, family)["u"]
        for power, eps in COMBOS:
            got = _gpu(u, eps, power, border)
            if family == "mild" and eps == 0.0:
                assert float(got[0]) == 0.0 and float(got[1].abs().max()) == 0.0, (power, eps)
                continue
            ref = penalty_reference(case, family, (power, eps))
            if ref[0] == 0.0:               # mild under eps = 0.5: every d64 clears the hinge by the guard band, exact zeros
                assert family == "mild" and float((reference(case, family)["d"] - eps).min()) >= GUARD
                assert float(got[0]) == 0.0 and float(got[1].abs().max()) == 0.0, (power, eps)
                continue
            _check(got, ref, family, "%s p%d eps%.1f" % (_id(case), power, eps))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_jacobian_map_and_statistics_vs_restatement(case):
    from dfmir_amd import infer, ops
    shape, border = case
    vol = tuple(shape[2:])
    for family in FAMILIES:
        input_conditions(case, family)
        ref = reference(case, family)
        b = BOUND[family]
        x = ref["u"].to(DEV)
        dm = ops.jacobian_determinant(x, border).cpu()
        assert dm.shape == (shape[0], 1) + vol and dm.dtype == torch.float32
        outside = torch.ones((shape[0], 1) + vol, dtype=torch.bool)
        outside[(slice(None), slice(None)) + tuple(slice(border, n - border) for n in vol)] = False
        assert bool((dm[outside] == 1.0).all())
        emap = float((dm.double() - ref["map"]).abs().max())
        st = ops.jacobian_stats(x, border, LOG_OFFSET[family]).cpu()
        assert st.shape == (shape[0], 6) and st.dtype == torch.float64
        errs = stat_errors(st, ref["stats"])
        print("%s [%s]: map %.3e (bound %.1e)  min %.3e max %.3e mean %.3e meanl %.3e stdl %.3e (bounds %s)"
              % ((_id(case), family, emap, b[3]) + errs + (" ".join("%.1e" % v for v in b[4:]),)))
        assert emap <= b[3]
        assert torch.equal(st[:, 0], ref["stats"][:, 0]), (st[:, 0], ref["stats"][:, 0])          # exact under C1
        assert all(e <= bb for e, bb in zip(errs, b[4:])), (family, errs)
        # the minimum and the maximum are values of the map
        om = dm[~outside].reshape(shape[0], -1).double()
        assert torch.equal(st[:, 1], om.min(1).values) and torch.equal(st[:, 2], om.max(1).values)
        reg = infer.flow_regularity(x, border, LOG_OFFSET[family])
        assert sorted(reg) == ['detmap', 'folded', 'folded_count', 'max', 'mean', 'min', 'sdlogj']
        assert torch.equal(reg['detmap'].cpu(), dm) and torch.equal(reg['folded_count'].cpu(), st[:, 0])
        assert torch.allclose(reg['folded'].cpu(), st[:, 0] / om.shape[1], rtol=1e-15, atol=0.0)     # (a device division)
        assert torch.equal(reg['sdlogj'].cpu(), st[:, 5])
        assert torch.equal(reg['min'].cpu(), st[:, 1]) and torch.equal(reg['max'].cpu(), st[:, 2]) and torch.equal(reg['mean'].cpu(), st[:, 3])
        if shape[0] == 2 and om.shape[1] > 1:               # per sample: two different fields give two different rows
            assert not torch.equal(st[0], st[1])
            one = ops.jacobian_stats(x[1:], border, LOG_OFFSET[family]).cpu()
            assert torch.equal(one[0], st[1])


def _affine32(vol, A):
    return _affine_field(vol, A).float()


@pytest.mark.gpu
@pytest.mark.parametrize("vol", [(6, 9, 70), (5, 68)], ids=["3d", "2d"])
def test_jacobian_exact_identities_on_affine_fields(vol):
    from dfmir_amd import ops
    nd = len(vol)
    zero = torch.zeros((1, nd) + vol)
    for border in (1, 2):
        omega = math.prod(n - 2 * border for n in vol)
        assert bool((ops.jacobian_determinant(zero.to(DEV), border) == 1.0).all())
        for power, eps in ((2, 0.0), (1, 0.0), (2, 1.5), (1, 1.5), (2, 1.0)):
            loss, grad = _gpu(zero, eps, power, border)
            assert float(loss) == max(0.0, eps - 1.0) ** power
            assert eps > 1.0 or float(grad.abs().max()) == 0.0          # (an active penalty pulls at the border of Omega)
        st = ops.jacobian_stats(zero.to(DEV), border).cpu()
        assert st.tolist() == [[0.0, 1.0, 1.0, 1.0, 0.0, 0.0]]
        for axis in range(nd):                              # a reflection along one axis: d == -1 on Omega
            A = [[-2.0 if a == b == axis else 0.0 for b in range(nd)] for a in range(nd)]
            u = _affine32(vol, A)
            dm = ops.jacobian_determinant(u.to(DEV), border).cpu()
            inner = (slice(None), slice(None)) + tuple(slice(border, n - border) for n in vol)
            assert bool((dm[inner] == -1.0).all()) and float(dm.sum()) == float(math.prod(vol) - 2 * omega)
            assert float(_gpu(u, 0.0, 1, border)[0]) == 1.0
            st = ops.jacobian_stats(u.to(DEV), border).cpu()[0].tolist()
            assert st[:4] == [float(omega), -1.0, -1.0, -1.0] and st[5] == 0.0, st
            assert abs(st[4] - math.log(1e-9)) <= 4.0 * 2.0 ** -52 * abs(math.log(1e-9)), st[4]
            st3 = ops.jacobian_stats(u.to(DEV), border, 3.0).cpu()[0].tolist()
            assert st3[5] == 0.0 and abs(st3[4] - math.log(2.0)) <= 4.0 * 2.0 ** -52


@pytest.mark.gpu
@pytest.mark.parametrize("vol", [(6, 9, 70), (5, 68)], ids=["3d", "2d"])
@pytest.mark.parametrize("border", [1, 2])
def test_jacobian_gradient_on_an_affine_field_lives_at_the_border(vol, border):
    """d and the cofactors are constant on Omega, so the two W terms of every voxel farther than border + 1 from the
    boundary cancel exactly; a wrong Omega indicator in the adjoint leaves a gradient there (or none at the border)."""
    nd = len(vol)
    A = DYADIC[2] if nd == 3 else DYADIC[3]                 # det(I + A) < 0: the penalty is active everywhere
    u = _affine32(vol, A)
    for power, eps in COMBOS:
        loss64, g64 = penalty_loss_ref(u, eps, power, border)
        got = _gpu(u, eps, power, border)
        _check(got, (loss64, g64), "fold", "affine %s b%d p%d eps%.1f" % (vol, border, power, eps))
        assert float(g64.abs().max()) > 0.0
        far = (slice(None), slice(None)) + tuple(slice(border + 1, n - border - 1) for n in vol)
        if border == 1:                                     # (with border 2 these volumes have no such voxel)
            assert got[1][far].numel() > 0 and float(got[1][far].abs().max()) == 0.0
            assert float(g64[far].abs().max()) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("shape", MID, ids=["3d", "2d"])
def test_jacobian_loss_mask_and_loss_mult(shape):
    from dfmir_amd.losses import JacobianDet_Loss
    nd = len(shape) - 2
    u = reference((shape, 1), "fold")["u"]
    mask = (C.rand(77, *((shape[0], 1) + shape[2:])) > 0.3).float()
    x = u.to(DEV).requires_grad_()
    loss = JacobianDet_Loss(dim=nd, eps=0.5, power=2, loss_mult=0.25)(x, mask=mask)
    loss.backward()
    torch.cuda.synchronize()
    xr = u.double().requires_grad_()
    lr = 0.25 * penalty_ref(xr * mask.double(), 0.5, 2)
    lr.backward()
    _check((loss.detach().cpu(), x.grad.cpu()), (float(lr.detach()), xr.grad), "fold", "mask + loss_mult")
    plain = JacobianDet_Loss(dim=nd, eps=0.5, power=2)(u.to(DEV))
    assert torch.equal(plain.cpu(), _gpu(u, 0.5, 2)[0])
    b2 = JacobianDet_Loss(dim=nd, eps=0.5, power=1, border=2)(u.to(DEV))
    assert torch.equal(b2.cpu(), _gpu(u, 0.5, 1, 2)[0])


def _all_outputs(x, border=1):
    """(loss, gradient, map, statistics) of a device field that requires grad."""
    from dfmir_amd import ops
    loss = ops.jacobian_penalty(x, 0.5, 2, border)
    (g,) = torch.autograd.grad(loss, x)
    return loss.detach().cpu(), g.cpu(), ops.jacobian_determinant(x, border).cpu(), ops.jacobian_stats(x, border, 3.0).cpu()


@pytest.mark.gpu
def test_jacobian_non_contiguous_and_misaligned_inputs():
    for shape in MID:
        u = reference((shape, 1), "fold")["u"]
        want = _all_outputs(u.to(DEV).requires_grad_())
        perm = [0, 1] + list(range(len(shape) - 1, 1, -1))                # memory with the spatial axes reversed
        nc = u.permute(*perm).contiguous().to(DEV).permute(*perm).requires_grad_()
        assert not nc.is_contiguous() and nc.shape == u.shape
        assert all(torch.equal(a, b) for a, b in zip(_all_outputs(nc), want))
        cl = u.movedim(1, -1).contiguous().to(DEV).movedim(-1, 1).requires_grad_()      # channels last in memory
        assert not cl.is_contiguous() and cl.shape == u.shape
        assert all(torch.equal(a, b) for a, b in zip(_all_outputs(cl), want))
    # W % 4 == 0 but the field starts 4 bytes off a 16-byte boundary: the scalar staging path, the same bits
    for shape in ((1, 3, 4, 4, 64), (1, 2, 5, 64)):
        v = reference((shape, 1), "fold")["u"]
        want = _all_outputs(v.to(DEV).requires_grad_())
        base = torch.empty(v.numel() + 1, device=DEV)
        off = base[1:].view(shape)
        off.copy_(v)
        assert off.is_contiguous() and off.data_ptr() % 16 == 4
        assert all(torch.equal(a, b) for a, b in zip(_all_outputs(off.requires_grad_()), want))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 3, 13, 17, 19), (1, 3, 17, 5, 8), (1, 2, 37, 41), (1, 2, 5, 300)],
                         ids=["3d", "3d-vec", "2d", "2d-vec"])
def test_jacobian_bit_reproducible(shape):
    u = reference((shape, 1), "fold")["u"]
    r0, r1 = _all_outputs(u.to(DEV).requires_grad_()), _all_outputs(u.to(DEV).requires_grad_())
    assert all(torch.equal(a, b) for a, b in zip(r0, r1))


REFINE = dict(features='intensity', lam=0.0, grid_downsize=2, lr=0.1)
# a quarter of the voxels of these two fields fold (penalty 0.030 / 0.048); a float64 CPU emulation of the loop below (Adam on
# the coarse grid, align-corners linear upsampling) brought the penalty below 1e-6 and the folded share below 0.5 %
REFINE_SEED = {(12, 14, 16): 287, (20, 24): 136}


@pytest.mark.gpu
@pytest.mark.parametrize("vol", [(12, 14, 16), (20, 24)], ids=["3d", "2d"])
def test_refine_flow_fold_weight(vol):
    """fold_weight = 0 changes nothing; with a constant image on both sides (zeros: a sample outside the volume reads the
    same value, so the similarity has no gradient anywhere) and lam = 0 the fold penalty alone drives the descent."""
    from dfmir_amd import infer, ops
    nd = len(vol)
    flow = field((1, nd) + vol, "fold", seed=REFINE_SEED[vol]).to(DEV)
    img = torch.zeros((1, 1) + vol, device=DEV)
    A, B = (t.to(DEV) for t in (C.rand(5, 1, 1, *vol), C.rand(6, 1, 1, *vol)))
    r0 = infer.refine_flow(A, B, flow, iters=3, **REFINE)
    r1 = infer.refine_flow(A, B, flow, iters=3, fold_weight=0.0, fold_eps=0.5, fold_power=1, **REFINE)
    assert 'fold_history' not in r1 and sorted(r0) == sorted(r1)
    assert torch.equal(r0['flow'], r1['flow']) and torch.equal(r0['history'], r1['history'])
    before = infer.flow_regularity(flow)
    res = infer.refine_flow(img, img, flow, iters=30, fold_weight=1.0, fold_power=2, **REFINE)
    fh = res['fold_history']
    assert fh.shape == (31,) and fh.device == flow.device and res['history'].shape == (31, 2)
    assert torch.equal(fh[0], ops.jacobian_penalty(flow)) and torch.equal(fh[-1], ops.jacobian_penalty(res['flow']))
    after = infer.flow_regularity(res['flow'])
    print("fold penalty %.4g -> %.4g, folded %.4f -> %.4f" % (float(fh[0]), float(fh[-1]), float(before['folded']), float(after['folded'])))
    assert float(fh[0]) > 0.0 and float(fh[-1]) <= 0.5 * float(fh[0])
    assert float(after['folded_count']) < float(before['folded_count'])


def _model_step(shape):
    from tests import step3d
    m, A, B = step3d.step_model(shape, 'ncc', fold_weight=0.5, fold_eps=1.0, fold_power=2)
    m.set_input({"A": A, "B": B})
    m.optimize_parameters()
    torch.cuda.synchronize()
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(16, 16, 16), (16, 16)], ids=["3d", "2d"])
def test_registration3d_fold_step_matches_restatement(shape):
    """eps = 1 makes the term non-zero for any non-trivial flow.  The flow of a network is neither family; the bound is
    the larger of the two loss bounds."""
    m = _model_step(shape)
    got = m.get_current_losses()
    assert sorted(got) == ["fold", "grad", "ncc"] and list(got)[-1] == "fold"
    ref = float(penalty_ref(m.flow.detach().cpu().double(), 1.0, 2))
    err = abs(got["fold"] - ref) / abs(ref)
    bound = max(BOUND["fold"][0], BOUND["mild"][0])
    print("step loss_fold %.4g: %.3e (bound %.1e)" % (ref, err, bound))
    assert ref > 0.0 and got["fold"] > 0.0 and err <= bound
    assert float(m.optimizer_R.flat_g.abs().max()) > 0.0


@pytest.mark.gpu
def test_registration3d_fold_captured_step_matches_eager():
    """fold_weight > 0 (with similarity='mind') under capture_step=True: a replayed step equals the same step enqueued
    eagerly (the pattern and the tolerances of test_mind.py's captured-step test)."""
    from tests import step3d
    m, A, B = step3d.step_model((16, 16, 16), 'mind', capture=True, fold_weight=0.5, fold_eps=1.0, fold_power=2)
    m.parallelize()
    step3d.assert_replay_matches_eager(m, {"A": A, "B": B}, ["fold", "grad", "mind"])
