"""Discrete displacement search (build-defined, dfmir_amd/csrc/dsearch.hip): ops.pool_features, ops.ssd_cost_volume,
ops.cost_argmin, ops.box_smooth_flow and infer.convex_init built on them.  CPU: the C ABI and the argument checks; float64
restatements of the four definitions written with explicit padding and slicing over the displacement loop, a second one of
the cost volume through F.unfold (2-D), and a self-check of the sign convention on a planted integer shift.  GPU: the kernels
against the restatements.

The displacement index k enumerates d_k in {-r .. r}^nd in row-major order (dz,) dy, dx, -r first: `mesh` below.

Which launch each GPU case (B,C,*vol), g, r reaches (ds_cost_k<ND, CP>, CP = C rounded up to 4; a workgroup owns a 32 x 8
in-plane tile of one z-plane and one dz, and stages the whole (2r + 1)-row window of dy at once wherever it fits 64 KB of LDS):
  (2,4,9,13)      g 1 r 2   <2, 4>   odd extents, one partial tile in x, two tiles in y (the second with one live row)
  (1,5,12,20)     g 2 r 3   <2, 8>   C no multiple of 4; pooled to 6 x 10: smaller than one tile both ways, the window (7) wider
                                     than the volume in y (6)
  (1,3,40,36)     g 1 r 8   <2, 4>   the largest 2-D radius, 2 x 5 tiles
  (1,16,12,34)    g 1 r 8   <2, 16>  the one combination whose window is staged in TWO chunks of dy (9 + 8 rows), two tiles each way
  (2,12,8,12,24)  g 2 r 2   <3, 12>  the MIND channel count, B = 2, pooled to 4 x 6 x 12
  (1,1,5,7,9)     g 1 r 1   <3, 4>   C = 1, odd extents
  (1,3,7,11,13)   g 3 r 1   <3, 4>   the pooling remainder dropped on every axis, 2 x 3 x 4 coarse voxels
  (1,16,6,20,36)  g 1 r 4   <3, 16>  the largest 3-D radius and channel count, 2 x 3 tiles
ds_pool_k runs for every case (g = 1: as the packing copy inside ssd_cost_volume as well), ds_argmin_k<ND> and ds_smooth_k<ND>
on every pooled volume with and without `soft`.  (1,16,12,34) is not in the issue's table: it is added for the chunked stage.

Tolerances (profiles/dsearch_margins.txt, measured by scripts/dsearch_margins.py on this case set): pooling, cost volume and
box mean are bounded by 4x the error of the SAME definition evaluated by torch in fp32 on the CPU against float64 on these
inputs (noise in [-1, 1]; integer-valued fields for the box mean) -- max-abs over max and relative 2-norm, each the maximum over
the case set.  The argmin on synthetic costs is exact (small integers, soft in halves, coeff in {0, 0.25, 1}: every quantity
is exact in fp32); on real costs the pick must lie within tau = 2 (cost bound x max |cost| + coeff x fp32 eps x (2r)^2 x nd) of
the float64 minimum at EVERY voxel -- no index equality, no exclusions (near-ties are common on such inputs).

The planted end-to-end cases: features cut from one larger noise volume so that mov(x + g t) == fix(x).  Where X + t lies
inside the coarse volume cost(t) is exactly 0 and the plain argmin is t; elsewhere the pick is arbitrary, the first box mean
carries that one voxel inwards, and every round of the alternation one more (a coupled argmin can leave t wherever soft is not
t, and the box mean spreads it): `coarse` is asserted at the coarse voxels at least r + 1 + len(coeffs) from every face, the
issue's margin, with its coeffs = (0.003, 1.0), g, r, t, channel counts and thresholds.  That margin is 6 (7 in 2-D) and
leaves NO voxel at the issue's volumes, 16 x 24 x 32 and 24 x 40 (8 x 12 x 16 and 12 x 20 coarse voxels; the tighter per-face
bound max(0, +-t_a) + 1 + len(coeffs) still leaves none in z), where the end-to-end assertions would hold of nothing and the
"zero flow is above 0.1" one could not hold at all; the volumes are therefore grown to the smallest multiples of 4 with an
interior two voxels wide, 28 x 28 x 32 and 32 x 40.  The plain-argmin self-check of the sign convention runs at the issue's
volumes as well."""
import ctypes
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import ref64
from tests.golden import common as C

DEV = "cuda"
FACTOR = 4.0
# profiles/dsearch_margins.txt, rows "max" of the fp32 CPU columns: (max-abs over max, relative 2-norm)
FP32_ERR = {"pool": (1.55e-07, 7.69e-08), "cost": (1.99e-07, 6.64e-08), "smooth": (3.97e-08, 2.60e-08)}
BOUND = {k: tuple(FACTOR * e for e in v) for k, v in FP32_ERR.items()}
EPS32 = float(torch.finfo(torch.float32).eps)

# ((B,C,*vol), g, r)
CASES = [((2, 4, 9, 13), 1, 2), ((1, 5, 12, 20), 2, 3), ((1, 3, 40, 36), 1, 8), ((1, 16, 12, 34), 1, 8),
         ((2, 12, 8, 12, 24), 2, 2), ((1, 1, 5, 7, 9), 1, 1), ((1, 3, 7, 11, 13), 3, 1), ((1, 16, 6, 20, 36), 1, 4)]
# (shape, g, r, t, coeffs) of the planted end-to-end cases
PLANTED = [((1, 12, 28, 28, 32), 2, 3, (2, -1, 3), (0.003, 1.0)), ((2, 4, 32, 40), 2, 4, (-3, 2), (0.003, 1.0))]
# the issue's volumes: the plain-argmin self-check only (module docstring)
PLANTED_SMALL = [((1, 12, 16, 24, 32), 2, 3, (2, -1, 3), None), ((2, 4, 24, 40), 2, 4, (-3, 2), None)]
REFINE_KW = dict(grid_downsize=2, iters=30, lr=0.1, lam=0.05, regularizer='diffusion')


def _id(case):
    return "x".join(str(v) for v in case[0]) + "-g%d-r%d" % (case[1], case[2])


# ------------------------------------------------------------------------------------------ restatements
def mesh(nd, r, dtype=torch.float64):
    """[K, nd]: d_k in row-major order (dz,) dy, dx, -r first."""
    return torch.tensor(list(itertools.product(range(-r, r + 1), repeat=nd)), dtype=dtype)


def pool_ref(x, g):
    """[B,C,*vol] -> [B,C,*(vol // g)]: the mean over g^nd windows at stride g, the far remainder dropped; in x's dtype."""
    sp = [n // g for n in x.shape[2:]]
    x = x[(slice(None), slice(None)) + tuple(slice(0, n * g) for n in sp)]
    shape = list(x.shape[:2])
    for n in sp:
        shape += [n, g]
    return x.reshape(shape).mean(tuple(range(3, 3 + 2 * len(sp), 2)))


def cost_ref(fix, mov, r):
    """[B,K,*vol]: mean_c (fix(x) - mov(x + d_k))^2 with mov zero-padded by r, one slice per displacement; in fix's dtype."""
    nd = fix.dim() - 2
    vol = fix.shape[2:]
    pm = F.pad(mov, (r, r) * nd)
    out = []
    for d in itertools.product(range(-r, r + 1), repeat=nd):
        sl = (slice(None), slice(None)) + tuple(slice(r + d[a], r + d[a] + vol[a]) for a in range(nd))
        out.append(((fix - pm[sl]) ** 2).mean(1))
    return torch.stack(out, 1)


def cost_ref_unfold(fix, mov, r):
    """The same through F.unfold (2-D): every shifted copy of mov as a column block."""
    B, Cn, H, W = fix.shape
    n = 2 * r + 1
    cols = F.unfold(mov, kernel_size=n, padding=r).reshape(B, Cn, n * n, H, W)
    return ((fix[:, :, None] - cols) ** 2).mean(1)


def coupled_ref(cost, r, soft=None, coeff=0.0):
    """[B,K,*vol] float64: cost + coeff sum_a (d_k[a] - soft[a])^2."""
    nd = cost.dim() - 2
    J = cost.double()
    if soft is not None:
        m = mesh(nd, r).reshape((1, -1, nd) + (1,) * nd)
        J = J + coeff * ((m - soft.double()[:, None]) ** 2).sum(2)
    return J


def argmin_ref(cost, r, soft=None, coeff=0.0):
    """(idx [B,*vol] int64, disp [B,nd,*vol] float64): the LOWEST k among the minimisers."""
    nd = cost.dim() - 2
    J = coupled_ref(cost, r, soft, coeff)
    K = J.shape[1]
    ks = torch.arange(K).reshape((1, K) + (1,) * nd).expand_as(J)
    idx = torch.where(J == J.min(1, keepdim=True).values, ks, torch.full_like(ks, K)).min(1).values
    disp = mesh(nd, r)[idx].movedim(-1, 1)
    return idx, disp


def smooth_ref(disp):
    """[B,nd,*vol]: the sum over the 3^nd neighbours (zero-padded) divided by the number of them inside the volume."""
    nd = disp.dim() - 2
    vol = disp.shape[2:]
    pd, pc = F.pad(disp, (1, 1) * nd), F.pad(torch.ones_like(disp), (1, 1) * nd)
    s, c = torch.zeros_like(disp), torch.zeros_like(disp)
    for d in itertools.product((0, 1, 2), repeat=nd):
        sl = (slice(None), slice(None)) + tuple(slice(d[a], d[a] + vol[a]) for a in range(nd))
        s, c = s + pd[sl], c + pc[sl]
    return s / c


def convex_ref(Mm, Mf, g, r, coeffs, dtype=torch.float64):
    """infer.convex_init on a feature pair restated on the CPU: dict(flow, coarse, idx)."""
    mov_p, fix_p = pool_ref(Mm.to(dtype), g), pool_ref(Mf.to(dtype), g)
    cost = cost_ref(fix_p, mov_p, r)
    idx, disp = argmin_ref(cost, r)
    soft = smooth_ref(disp.to(dtype))
    for c in coeffs:
        idx, disp = argmin_ref(cost, r, soft, c)
        soft = smooth_ref(disp.to(dtype))
    return dict(flow=ref64.resize_linear(soft, tuple(Mm.shape[2:]), mult=float(g), dtype=dtype), coarse=soft, idx=idx)


def errs(got, ref):
    """(max-abs over max, relative 2-norm) against the float64 restatement."""
    g, r = got.detach().cpu().double(), ref.double()
    return float((g - r).abs().max() / r.abs().max()), float((g - r).norm() / r.norm())


# ------------------------------------------------------------------------------------------ inputs and shared references
def features(case):
    """(mov, fix) fp32 noise in [-1, 1] of a case."""
    shape = case[0]
    seed = 1300 + 19 * CASES.index(case)
    return C.rand(seed, *shape) * 2 - 1, C.rand(seed + 1, *shape) * 2 - 1


_REF = {}


def reference(case):
    """dict of a case, computed once and shared (never modified): mov, fix (fp32), pooled64 = (mov, fix) pooled in float64,
    P = (mov, fix) pooled and rounded to fp32 -- the cost volume's inputs on both sides -- and cost64 = cost_ref of P."""
    key = _id(case)
    if key not in _REF:
        mov, fix = features(case)
        g, r = case[1], case[2]
        p64 = (pool_ref(mov.double(), g), pool_ref(fix.double(), g))
        P = (p64[0].float(), p64[1].float())
        _REF[key] = dict(mov=mov, fix=fix, pooled64=p64, P=P, cost64=cost_ref(P[1].double(), P[0].double(), r))
    return _REF[key]


def synthetic(case, seed=0):
    """(cost [B,K,*pooled vol] of small integers in [0, 7], soft [B,nd,*pooled vol] in halves within [-r, r]) fp32."""
    shape, g, r = case
    sp = tuple(n // g for n in shape[2:])
    nd = len(sp)
    s = 1700 + 23 * CASES.index(case) + seed
    cost = torch.floor(C.rand(s, shape[0], (2 * r + 1) ** nd, *sp) * 8.0).clamp(0, 7)
    soft = torch.floor(C.rand(s + 1, shape[0], nd, *sp) * (4 * r + 1)).clamp(0, 4 * r) * 0.5 - r
    return cost, soft


def integer_field(case):
    """[B,nd,*pooled vol] fp32, integers in [-r, r]: what cost_argmin hands to the box mean."""
    shape, g, r = case
    sp = tuple(n // g for n in shape[2:])
    return torch.floor(C.rand(1900 + CASES.index(case), shape[0], len(sp), *sp) * (2 * r + 1)).clamp(0, 2 * r) - r


def planted(spec):
    """(mov, fix) fp32 [B,C,*vol] cut from one noise volume so that mov(x + g t) == fix(x) wherever both are inside."""
    shape, g, r, t, _ = spec
    vol = shape[2:]
    m = g * max(abs(v) for v in t)
    big = C.rand(2100 + len(vol), shape[0], shape[1], *[n + 2 * m for n in vol]) * 2 - 1
    cut = lambda off: big[(slice(None), slice(None)) + tuple(slice(m + off[a], m + off[a] + vol[a]) for a in range(len(vol)))]
    return cut([-g * v for v in t]).contiguous(), cut([0] * len(vol)).contiguous()


def planted_interior(which):
    """(coarse mask [*coarse vol], fine mask [1,1,*vol]) bool: the coarse voxels at least r + 1 + len(coeffs) from every
    face, and the fine voxels whose aligned-corner interpolation reads coarse voxels of that set alone."""
    shape, g, r, t, coeffs = PLANTED[which]
    vol = shape[2:]
    margin = r + 1 + len(coeffs)
    cm, fm = [], []
    for a, n in enumerate(vol):
        nc = n // g
        ok = torch.zeros(nc, dtype=torch.bool)
        ok[margin: nc - margin] = True
        c = torch.arange(n, dtype=torch.float64) * (nc - 1) / (n - 1)
        i0 = torch.floor(c).long().clamp(0, nc - 1)
        i1 = (i0 + 1).clamp(max=nc - 1)
        cm.append(ok)
        fm.append(ok[i0] & ok[i1])
    outer = lambda vs: math.prod([v.reshape([-1 if b == a else 1 for b in range(len(vs))]).long() for a, v in enumerate(vs)]).bool()
    return outer(cm), outer(fm)[None, None]


def masked_ssd64(mov, fix, flow, mask):
    from tests.test_refine import ssd_grid_sample
    return float(ssd_grid_sample(mov.double(), fix.double(), flow.double().cpu(), mask.double())[0])


_PLANTED = {}


def planted_reference(which):
    """(mov, fix, convex_ref(..) in float64), computed once and shared."""
    if which not in _PLANTED:
        _, g, r, _, coeffs = PLANTED[which]
        mov, fix = planted(PLANTED[which])
        _PLANTED[which] = (mov, fix, convex_ref(mov, fix, g, r, coeffs))
    return _PLANTED[which]


# ------------------------------------------------------------------------------------------ CPU tier
def _searchable(spec):
    """The case lies inside what the ops accept: the restatements below speak about the same window the kernels search."""
    from dfmir_amd import ops
    shape, g, r = spec[:3]
    assert 1 <= r <= ops.DSEARCH_MAX_RADIUS[len(shape) - 2] and min(n // g for n in shape[2:]) >= 2 and 1 <= shape[1] <= 16


def test_dsearch_symbols_in_header_exports_and_ctypes_table_and_null_pointers_refused():
    import dfmir_amd
    from dfmir_amd import _lib, infer, ops
    from tests.test_abi import header_symbols
    h = ctypes.CDLL(dfmir_amd.LIB_PATH)
    for s in ("dfmir_dsearch_pool", "dfmir_dsearch_cost", "dfmir_dsearch_argmin", "dfmir_dsearch_smooth"):
        assert s in header_symbols() and s in _lib.exported_symbols() and hasattr(h, s), s
    lib = dfmir_amd.lib()
    assert lib.dfmir_abi_version() == 14
    one = ctypes.c_void_p(16)                         # a non-null, aligned address that is never dereferenced: refused first
    calls = [lambda: lib.dfmir_dsearch_pool(3, None, None, None, 1, 4, 8, 8, 8, 2, None),
             lambda: lib.dfmir_dsearch_pool(3, one, None, None, 1, 4, 8, 8, 8, 2, None),          # neither output
             lambda: lib.dfmir_dsearch_pool(3, one, one, None, 1, 4, 8, 8, 8, 5, None),           # pooled extent 1
             lambda: lib.dfmir_dsearch_pool(3, one, one, None, 1, 17, 8, 8, 8, 2, None),
             lambda: lib.dfmir_dsearch_pool(3, one, one, None, 1, 4, 8, 8, 8, 0, None),
             lambda: lib.dfmir_dsearch_cost(3, None, None, None, 1, 4, 8, 8, 8, 2, None),
             lambda: lib.dfmir_dsearch_cost(3, one, one, one, 1, 4, 8, 8, 8, 5, None),            # r above 4 in 3-D
             lambda: lib.dfmir_dsearch_cost(2, one, one, one, 1, 4, 1, 8, 8, 9, None),            # r above 8 in 2-D
             lambda: lib.dfmir_dsearch_cost(3, one, one, one, 1, 4, 8, 8, 8, 0, None),
             lambda: lib.dfmir_dsearch_cost(4, one, one, one, 1, 4, 8, 8, 8, 1, None),
             lambda: lib.dfmir_dsearch_cost(3, one, one, one, 1, 4, 256, 256, 256, 4, None),      # B K S >= 2^31
             lambda: lib.dfmir_dsearch_cost(3, one, ctypes.c_void_p(20), one, 1, 4, 8, 8, 8, 1, None),   # misaligned
             lambda: lib.dfmir_dsearch_argmin(3, None, None, 0.0, None, None, 1, 8, 8, 8, 2, None),
             lambda: lib.dfmir_dsearch_argmin(3, one, None, -1.0, one, one, 1, 8, 8, 8, 2, None),
             lambda: lib.dfmir_dsearch_argmin(3, one, None, float('nan'), one, one, 1, 8, 8, 8, 2, None),
             lambda: lib.dfmir_dsearch_argmin(3, one, None, float('inf'), one, one, 1, 8, 8, 8, 2, None),
             lambda: lib.dfmir_dsearch_argmin(3, one, None, 0.0, one, one, 1, 1, 8, 8, 2, None),   # extent < 2
             lambda: lib.dfmir_dsearch_smooth(3, None, None, 1, 8, 8, 8, None),
             lambda: lib.dfmir_dsearch_smooth(3, one, one, 1, 8, 8, 8, None),                      # in place
             lambda: lib.dfmir_dsearch_smooth(2, one, ctypes.c_void_p(32), 0, 1, 8, 8, None)]
    for i, call in enumerate(calls):
        assert call() != 0, i
        assert b"invalid argument" in lib.dfmir_last_error(), i
    assert ops.DSEARCH_MAX_RADIUS == {2: 8, 3: 4}
    for name in ("pool_features", "ssd_cost_volume", "cost_argmin", "box_smooth_flow"):
        assert hasattr(ops, name), name
    assert hasattr(infer, "convex_init")
    assert infer.CONVEX_COEFFS == (0.003, 0.01, 0.03, 0.1, 0.3, 1.0)


def test_dsearch_argument_checks_raise_before_the_device_is_asked_for():
    from dfmir_amd import infer, ops
    from dfmir_amd._lib import DfmirHipError
    z = torch.zeros
    # pool_features
    for g in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="g must be an integer >= 1"):
            ops.pool_features(z(1, 4, 8, 8), g)
    with pytest.raises(ValueError, match="pooled extent"):
        ops.pool_features(z(1, 4, 8, 3), 2)
    with pytest.raises(ValueError, match="1 to 16 channels, got 17"):
        ops.pool_features(z(1, 17, 8, 8), 2)
    with pytest.raises(ValueError, match="fp32"):
        ops.pool_features(z(1, 4, 8, 8).double(), 2)
    with pytest.raises(ValueError, match=r"\[B,C,H,W\] or \[B,C,D,H,W\]"):
        ops.pool_features(z(4, 8, 8), 2)
    with pytest.raises(ValueError, match="2\\^31"):
        ops.pool_features(z(1, 16, 1, 1, 1).expand(1, 16, 512, 512, 512), 2)
    with pytest.raises(ValueError, match="requires grad"):
        ops.pool_features(z(1, 4, 8, 8).requires_grad_(), 2)
    with pytest.raises(DfmirHipError, match="no CPU fallback"):
        ops.pool_features(z(1, 4, 8, 8), 2)
    # ssd_cost_volume
    with pytest.raises(ValueError, match="differ in shape"):
        ops.ssd_cost_volume(z(1, 4, 8, 8), z(1, 4, 8, 9), 2)
    with pytest.raises(ValueError, match="differ in shape"):
        ops.ssd_cost_volume(z(1, 4, 8, 8), None, 2)
    for r, shape in ((0, (1, 4, 8, 8)), (9, (1, 4, 8, 8)), (5, (1, 4, 8, 8, 8)), (2.0, (1, 4, 8, 8)), (True, (1, 4, 8, 8))):
        with pytest.raises(ValueError, match="radius must be an integer"):
            ops.ssd_cost_volume(z(*shape), z(*shape), r)
    with pytest.raises(ValueError, match="1 to 16 channels, got 0"):
        ops.ssd_cost_volume(z(1, 0, 8, 8), z(1, 0, 8, 8), 2)
    with pytest.raises(ValueError, match="fp32"):
        ops.ssd_cost_volume(z(1, 4, 8, 8).half(), z(1, 4, 8, 8).half(), 2)
    with pytest.raises(ValueError, match="extent >= 2"):
        ops.ssd_cost_volume(z(1, 4, 1, 8), z(1, 4, 1, 8), 2)
    big = z(1, 4, 1, 1, 1).expand(1, 4, 160, 192, 224)
    with pytest.raises(ValueError, match="cost volume .* 2\\^31"):
        ops.ssd_cost_volume(big, big, 4)                                            # 729 x 6.9 M
    for which in range(2):
        args = [z(1, 4, 8, 8), z(1, 4, 8, 8)]
        args[which].requires_grad_()
        with pytest.raises(ValueError, match="requires grad"):
            ops.ssd_cost_volume(*args, 2)
    with pytest.raises(DfmirHipError, match="no CPU fallback"):
        ops.ssd_cost_volume(z(1, 4, 8, 8), z(1, 4, 8, 8), 2)
    # cost_argmin
    with pytest.raises(ValueError, match="must have 25 channels"):
        ops.cost_argmin(z(1, 24, 8, 8), 2)
    with pytest.raises(ValueError, match="must have 27 channels"):
        ops.cost_argmin(z(1, 9, 8, 8, 8), 1)
    with pytest.raises(ValueError, match="radius must be an integer"):
        ops.cost_argmin(z(1, 25, 8, 8), 0)
    with pytest.raises(ValueError, match=r"\[B,K,H,W\] or \[B,K,D,H,W\]"):
        ops.cost_argmin(z(25, 8, 8), 2)
    with pytest.raises(ValueError, match="soft must be"):
        ops.cost_argmin(z(1, 25, 8, 8), 2, soft=z(1, 3, 8, 8))
    with pytest.raises(ValueError, match="soft must be"):
        ops.cost_argmin(z(1, 25, 8, 8), 2, soft=z(1, 2, 8, 9))
    with pytest.raises(ValueError, match="fp32"):
        ops.cost_argmin(z(1, 25, 8, 8), 2, soft=z(1, 2, 8, 8).double())
    with pytest.raises(ValueError, match="fp32"):
        ops.cost_argmin(z(1, 25, 8, 8).double(), 2)
    for bad in (-0.1, float('inf'), float('nan'), "x", None):
        with pytest.raises(ValueError, match="coeff must be a finite number >= 0"):
            ops.cost_argmin(z(1, 25, 8, 8), 2, soft=z(1, 2, 8, 8), coeff=bad)
    with pytest.raises(ValueError, match="requires grad"):
        ops.cost_argmin(z(1, 25, 8, 8).requires_grad_(), 2)
    with pytest.raises(DfmirHipError, match="no CPU fallback"):
        ops.cost_argmin(z(1, 25, 8, 8), 2, soft=z(1, 2, 8, 8), coeff=0.5)
    # box_smooth_flow
    with pytest.raises(ValueError, match="must have 2 channels"):
        ops.box_smooth_flow(z(1, 3, 8, 8))
    with pytest.raises(ValueError, match="extent >= 2"):
        ops.box_smooth_flow(z(1, 3, 1, 8, 8))
    with pytest.raises(ValueError, match="fp32"):
        ops.box_smooth_flow(z(1, 2, 8, 8).double())
    with pytest.raises(ValueError, match=r"\[B,.,H,W\]"):
        ops.box_smooth_flow(z(2, 8, 8))
    with pytest.raises(DfmirHipError, match="no CPU fallback"):
        ops.box_smooth_flow(z(1, 2, 8, 8))
    # convex_init
    a = z(1, 1, 16, 16)
    with pytest.raises(ValueError, match="one shape"):
        infer.convex_init(a, z(1, 1, 16, 17))
    with pytest.raises(ValueError, match="grid_sp must be an integer >= 1"):
        infer.convex_init(a, a, grid_sp=0)
    with pytest.raises(ValueError, match="search grid"):
        infer.convex_init(a, a, grid_sp=16)
    for hw in (0, 9, 1.0):
        with pytest.raises(ValueError, match="disp_hw must be an integer"):
            infer.convex_init(a, a, disp_hw=hw)
    with pytest.raises(ValueError, match="disp_hw must be an integer"):
        infer.convex_init(z(1, 1, 16, 16, 16), z(1, 1, 16, 16, 16), disp_hw=5)
    for bad in ((0.1, -1.0), (float('nan'),), 3.0, ("a",)):
        with pytest.raises(ValueError, match="coeffs must be"):
            infer.convex_init(a, a, coeffs=bad)
    with pytest.raises(ValueError, match="features must be"):
        infer.convex_init(a, a, features='ssc')
    with pytest.raises(ValueError, match="single-channel"):
        infer.convex_init(z(1, 2, 16, 16), z(1, 2, 16, 16), features='intensity')
    with pytest.raises(ValueError, match="feature tensors"):
        infer.convex_init(a, a, features=(z(1, 4, 16, 16), z(1, 4, 16, 15)))
    with pytest.raises(DfmirHipError, match="no CPU fallback"):
        infer.convex_init(a, a, features='intensity')


def test_mesh_order_and_unfold_restatement_agrees_with_the_slicing_one():
    assert mesh(2, 1).tolist() == [[-1, -1], [-1, 0], [-1, 1], [0, -1], [0, 0], [0, 1], [1, -1], [1, 0], [1, 1]]
    m = mesh(3, 2)
    assert m.shape == (125, 3) and m[0].tolist() == [-2, -2, -2] and m[1].tolist() == [-2, -2, -1] and m[5].tolist() == [-2, -1, -2]
    for case in CASES:
        _searchable(case)
        if len(case[0]) == 4:
            P = reference(case)["P"]
            a, b = reference(case)["cost64"], cost_ref_unfold(P[1].double(), P[0].double(), case[2])
            assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-14, _id(case)


@pytest.mark.parametrize("spec", PLANTED_SMALL + PLANTED, ids=_id)
def test_restated_argmin_has_the_sign_convention_of_the_flow(spec):
    """With mov(x + g t) == fix(x) the restated plain argmin is t, at cost exactly 0, at every coarse voxel at least r from
    every face (where every sample of the window is inside)."""
    shape, g, r, t, _ = spec
    _searchable(spec)
    mov, fix = planted(spec)
    nd = len(t)
    cost = cost_ref(pool_ref(fix.double(), g), pool_ref(mov.double(), g), r)
    idx, disp = argmin_ref(cost, r)
    inner = (slice(None),) + tuple(slice(r, n // g - r) for n in shape[2:])
    k_t = sum((t[a] + r) * (2 * r + 1) ** (nd - 1 - a) for a in range(nd))
    assert idx[inner].numel() > 0 and bool((idx[inner] == k_t).all())
    assert float(cost[:, k_t][inner].abs().max()) == 0.0
    for a in range(nd):
        assert bool((disp[:, a][inner] == t[a]).all())


@pytest.mark.parametrize("which", range(len(PLANTED)))
def test_restated_search_recovers_a_planted_shift(which):
    """In float64: the alternation returns t on the interior; the resized flow registers the pair exactly where a zero flow
    does not; and a local descent started from zero does not get there."""
    from tests.test_refine import refine_ref
    shape, g, r, t, coeffs = PLANTED[which]
    _searchable(PLANTED[which])
    mov, fix, out = planted_reference(which)
    nd = len(t)
    cmask, fmask = planted_interior(which)
    assert int(cmask.sum()) > 0 and int(fmask.sum()) > 0
    want = torch.tensor(t, dtype=torch.float64).reshape((1, nd) + (1,) * nd)
    assert float(((out["coarse"] - want).abs() * cmask).max()) <= 1e-6
    assert masked_ssd64(mov, fix, out["flow"], fmask) < 1e-10
    assert masked_ssd64(mov, fix, torch.zeros_like(out["flow"]), fmask) > 0.1
    flow, _ = refine_ref(mov, fix, **REFINE_KW)
    assert masked_ssd64(mov, fix, flow, fmask) > 0.1


# ------------------------------------------------------------------------------------------ GPU tier
def _check(what, got, ref, kind):
    e, b = errs(got, ref), BOUND[kind]
    print("%s: max-abs/max %.3e (bound %.1e)  l2 %.3e (bound %.1e)" % (what, e[0], b[0], e[1], b[1]))
    assert bool(torch.isfinite(got).all()), what
    assert e[0] <= b[0] and e[1] <= b[1], (what, e, b)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_pool_features_matches_fp64(case):
    from dfmir_amd import ops
    ref = reference(case)
    for name, p64 in zip(("mov", "fix"), ref["pooled64"]):
        got = ops.pool_features(ref[name].to(DEV), case[1])
        assert got.shape == p64.shape and got.is_contiguous()
        if case[1] == 1:
            assert torch.equal(got.cpu(), ref[name])
        _check("pool %s %s" % (_id(case), name), got, p64, "pool")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_cost_volume_matches_fp64_and_outside_samples_tie_exactly(case):
    from dfmir_amd import ops
    ref = reference(case)
    r = case[2]
    mov_p, fix_p = ref["P"]
    cost = ops.ssd_cost_volume(fix_p.to(DEV), mov_p.to(DEV), r)
    assert cost.shape == ref["cost64"].shape and cost.is_contiguous()
    _check("cost %s" % _id(case), cost, ref["cost64"], "cost")
    # every k whose sample lies outside the volume has the same bits, at every voxel
    vol = mov_p.shape[2:]
    nd = len(vol)
    pos = torch.stack(torch.meshgrid(*[torch.arange(n) for n in vol], indexing='ij'), 0)[None] \
        + mesh(nd, r, torch.long).reshape((-1, nd) + (1,) * nd)
    outside = torch.zeros(pos.shape[:1] + tuple(vol), dtype=torch.bool)
    for a in range(nd):
        outside |= (pos[:, a] < 0) | (pos[:, a] >= vol[a])
    c = cost.cpu()
    inf = torch.full_like(c, float('inf'))
    lo = torch.where(outside[None], c, inf).min(1).values
    hi = torch.where(outside[None], c, -inf).max(1).values
    some = outside.any(0)[None].expand_as(lo)
    assert int(some.sum()) > 0
    assert torch.equal(lo[some], hi[some])
    assert torch.equal(lo[some], ops.ssd_cost_volume(fix_p.to(DEV), torch.zeros_like(mov_p).to(DEV), r).cpu()[:, 0][some])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_cost_argmin_is_exact_on_integer_costs(case):
    from dfmir_amd import ops
    r = case[2]
    cost, soft = synthetic(case)
    nd = cost.dim() - 2
    m32 = mesh(nd, r, torch.float32)
    for sf, coeff in ((None, 0.0), (soft, 0.0), (soft, 0.25), (soft, 1.0)):
        idx, disp = ops.cost_argmin(cost.to(DEV), r, None if sf is None else sf.to(DEV), coeff)
        want, _ = argmin_ref(cost, r, sf, coeff)
        assert idx.dtype == torch.int32 and idx.shape == want.shape and disp.shape == (cost.shape[0], nd) + tuple(cost.shape[2:])
        assert torch.equal(idx.cpu().long(), want), (_id(case), coeff, int((idx.cpu().long() != want).sum()))
        assert torch.equal(disp.cpu(), m32[idx.cpu().long()].movedim(-1, 1))
    # a NaN is never selected; where every value is NaN the result is index 0
    bad = cost.clone()
    bad[:, ::2] = float('nan')
    bad.reshape(bad.shape[0], bad.shape[1], -1)[0, :, 0] = float('nan')
    idx, _ = ops.cost_argmin(bad.to(DEV), r)
    flat = idx.cpu().reshape(idx.shape[0], -1).long()
    assert int(flat[0, 0]) == 0
    assert bool((flat.reshape(-1)[1:] % 2 == 1).all())
    want, _ = argmin_ref(torch.where(torch.isnan(bad), torch.full_like(bad, float('inf')), bad), r)
    assert torch.equal(flat.reshape(-1)[1:], want.reshape(-1)[1:])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_cost_argmin_on_real_costs_picks_within_the_rounding_of_the_minimum(case):
    from dfmir_amd import ops
    ref = reference(case)
    r = case[2]
    mov_p, fix_p = ref["P"]
    nd = mov_p.dim() - 2
    cost = ops.ssd_cost_volume(fix_p.to(DEV), mov_p.to(DEV), r)
    soft = (C.rand(2300 + CASES.index(case), mov_p.shape[0], nd, *mov_p.shape[2:]) * 2 - 1) * r
    for sf, coeff in ((None, 0.0), (soft, 0.0), (soft, 0.003), (soft, 1.0)):
        idx, _ = ops.cost_argmin(cost, r, None if sf is None else sf.to(DEV), coeff)
        J = coupled_ref(ref["cost64"], r, sf, coeff)
        gap = J.gather(1, idx.cpu().long()[:, None])[:, 0] - J.min(1).values
        tau = 2.0 * (BOUND["cost"][0] * float(ref["cost64"].abs().max()) + coeff * EPS32 * (2 * r) ** 2 * nd)
        print("argmin %s coeff %g: worst gap %.3e (tau %.3e), %d of %d picks differ from the float64 argmin"
              % (_id(case), coeff, float(gap.max()), tau, int((idx.cpu().long() != argmin_ref(ref["cost64"], r, sf, coeff)[0]).sum()),
                 idx.numel()))
        assert bool((idx >= 0).all()) and bool((idx < cost.shape[1]).all())
        assert float(gap.max()) <= tau, (_id(case), coeff, float(gap.max()), tau)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_box_smooth_flow_matches_fp64_and_keeps_a_constant_field(case):
    from dfmir_amd import ops
    d = integer_field(case)
    got = ops.box_smooth_flow(d.to(DEV))
    _check("smooth %s" % _id(case), got, smooth_ref(d.double()), "smooth")
    const = torch.empty_like(d)
    for a in range(d.shape[1]):
        const[:, a] = float(a + 1) * (-1.0) ** a               # 1, -2(, 3)
    assert torch.equal(ops.box_smooth_flow(const.to(DEV)).cpu(), const)          # faces, edges and corners included


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(len(PLANTED)))
def test_convex_init_recovers_a_planted_shift_that_refine_flow_alone_does_not(which):
    from dfmir_amd import infer, ops
    shape, g, r, t, coeffs = PLANTED[which]
    mov, fix, ref = planted_reference(which)
    nd = len(t)
    img = torch.zeros((shape[0], 1) + tuple(shape[2:]), device=DEV)
    pair = (mov.to(DEV), fix.to(DEV))
    out = infer.convex_init(img, img, features=pair, grid_sp=g, disp_hw=r, coeffs=coeffs)
    cmask, fmask = planted_interior(which)
    want = torch.tensor(t, dtype=torch.float32).reshape((1, nd) + (1,) * nd)
    assert out["coarse"].shape == ref["coarse"].shape and out["flow"].shape == (shape[0], nd) + tuple(shape[2:])
    assert out["idx"].dtype == torch.int32 and out["idx"].shape == ref["idx"].shape
    assert float(((out["coarse"].cpu() - want).abs() * cmask).max()) <= 1e-6
    m = fmask.to(DEV).float()
    sim = float(ops.warp_ssd(pair[0], pair[1], out["flow"], mask=m))
    sim0 = float(ops.warp_ssd(pair[0], pair[1], torch.zeros_like(out["flow"]), mask=m))
    local = infer.refine_flow(img, img, None, features=pair, **REFINE_KW)
    sim_local = float(ops.warp_ssd(pair[0], pair[1], local["flow"], mask=m))
    print("planted %s: masked similarity %.3e with convex_init, %.3f with a zero flow, %.3f after refine_flow from zero"
          % (_id(PLANTED[which][:3]), sim, sim0, sim_local))
    assert sim < 1e-10
    assert sim0 > 0.1
    assert sim_local > 0.1


@pytest.mark.gpu
def test_convex_init_is_bit_reproducible_and_resolves_its_features():
    from dfmir_amd import infer
    shape, g, r, t, coeffs = PLANTED[0]
    mov, fix = planted(PLANTED[0])
    img = torch.zeros((shape[0], 1) + tuple(shape[2:]), device=DEV)
    pair = (mov.to(DEV), fix.to(DEV))
    a = infer.convex_init(img, img, features=pair, grid_sp=g, disp_hw=r)
    b = infer.convex_init(img, img, features=pair, grid_sp=g, disp_hw=r)
    assert torch.equal(a["idx"], b["idx"]) and torch.equal(a["flow"], b["flow"]) and torch.equal(a["coarse"], b["coarse"])
    # 'intensity' is the feature pair of the images themselves; 'mind' runs end to end
    A, Bx = mov[:, :1].contiguous().to(DEV), fix[:, :1].contiguous().to(DEV)
    c = infer.convex_init(A, Bx, features='intensity', grid_sp=2, disp_hw=2, coeffs=(0.1,))
    d = infer.convex_init(img, img, features=(A, Bx), grid_sp=2, disp_hw=2, coeffs=(0.1,))
    assert torch.equal(c["flow"], d["flow"]) and torch.equal(c["idx"], d["idx"])
    e = infer.convex_init(A, Bx, grid_sp=4, disp_hw=2)
    assert e["flow"].shape == (1, 3) + tuple(shape[2:]) and bool(torch.isfinite(e["flow"]).all())
    assert float(e["coarse"].abs().max()) <= 2.0
