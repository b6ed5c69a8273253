"""BendingEnergy_Loss / ops.bending_energy (build-defined second-order flow regulariser, dfmir_amd/csrc/bend.hip): the C ABI
and the argument checks (CPU), a float64 restatement of the definition written with slicing, checked on the CPU against an
independent conv{2,3}d composition ([1,-2,1] and outer([-1,0,1],[-1,0,1])/4 stencils) and against the documented adjoint
formula, and on the GPU against the kernels: value and gradient on shapes around the border and tile cases with and
without voxel spacing, exact identities on integer-valued fields, mask / loss_mult, a non-contiguous and a misaligned
input, run-to-run bit-reproducibility and Registration3DModel(regularizer='bending') eager and captured.

Which launch each GPU shape reaches (dfmir_bend_fwd and dfmir_bend_bwd select alike: <ND3, VEC> of bend_fwd_k /
bend_bwd_k; ND3 = D > 1, VEC = W % 4 == 0 and a 16-byte aligned field; the tile is 8 (y) x 64 (x), a z chunk 16 planes):
  <3-D, scalar>  (2,3,3,3,3) one voxel of Omega; (1,3,5,6,7); (2,3,13,17,19) three tiles along y;
                 (1,2,4,9,70) two tiles along y and x; (1,1,4,H,6) H = 7, 8, 9; (1,1,4,4,W) W = 63, 65; the misaligned view
  <3-D, vector>  (1,1,3,3,260) five tiles along x; (1,1,D,5,8) D = 15, 16, 17 (one / one / two z chunks); (1,1,4,4,64);
                 the 16^3 model steps
  <2-D, scalar>  (1,3,1,20,33), the one-plane volume; (2,2,3,3); (2,2,9,11); (1,2,37,41); (1,1,H,10) H = 7, 8, 9;
                 (1,1,5,W) W = 63, 65
  <2-D, vector>  (1,2,5,300); (1,1,5,64)
df_slot_mean_k (common.h) runs after every forward.

Inputs come in two families: `noise` (a seeded box-smoothed part plus 30 % uniform noise, as test_mind.mind_inputs) and
`smooth` (three seeded sinusoids of amplitude 2 and wavelength >= 12 voxels: a realistic flow, where the second
differences cancel).  Tolerances (profiles/bending_margins.txt): every comparison with the restatement is bounded by 4x the
error of the SAME definition evaluated by torch in fp32 on the CPU against the float64 restatement, on these inputs -- the
maxima over the case set, per family: the loss (relative), the gradient in relative 2-norm and as max-abs over max.
scripts/bending_margins.py measures them, and the kernels' own errors beside them."""
import ctypes
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

from tests.golden import common as C

DEV = "cuda"
FACTOR = 4.0
# profiles/bending_margins.txt, row "max" of the fp32 CPU columns: (loss, gradient 2-norm, gradient max-abs over max)
FP32_ERR = {"noise": (1.67e-07, 9.65e-08, 1.48e-07), "smooth": (3.39e-07, 1.08e-06, 1.89e-06)}
BOUND = {k: tuple(FACTOR * e for e in v) for k, v in FP32_ERR.items()}
FAMILIES = ("noise", "smooth")

SHAPES_3D = [(2, 3, 3, 3, 3), (1, 3, 5, 6, 7), (2, 3, 13, 17, 19), (1, 3, 1, 20, 33), (1, 2, 4, 9, 70), (1, 1, 3, 3, 260)]
SHAPES_2D = [(2, 2, 3, 3), (2, 2, 9, 11), (1, 2, 37, 41), (1, 2, 5, 300)]
TILE_Y, TILE_X, CHUNK_Z = 8, 64, 16          # TY, TX, ZC of csrc/stencil_tile.h
SHAPES_TILE = ([(1, 1, d, 5, 8) for d in (CHUNK_Z - 1, CHUNK_Z, CHUNK_Z + 1)] +
               [(1, 1, 4, h, 6) for h in (TILE_Y - 1, TILE_Y, TILE_Y + 1)] +
               [(1, 1, 4, 4, w) for w in (TILE_X - 1, TILE_X, TILE_X + 1)] +
               [(1, 1, h, 10) for h in (TILE_Y - 1, TILE_Y, TILE_Y + 1)] +
               [(1, 1, 5, w) for w in (TILE_X - 1, TILE_X, TILE_X + 1)])
SHAPES = SHAPES_3D + SHAPES_2D + SHAPES_TILE
SPACING = (1.5, 1.0, 0.75)
CASES = [(s, sp) for s in SHAPES for sp in (False, True)]


def _spacing(shape, spaced):
    """None, or SPACING cut to the rank; the one-plane volume takes all three entries (the first is ignored)."""
    if not spaced:
        return None
    return SPACING if len(shape) == 5 else SPACING[1:]


def _id(case):
    return "x".join(str(v) for v in case[0]) + ("-spaced" if case[1] else "-unit")


# ------------------------------------------------------------------------------------------ restatement
def bending_ref(u, spacing=None):
    """The definition with slicing, in u's dtype, differentiable.  u [B,C,*vol]; a one-plane volume is its 2-D field."""
    if u.dim() == 5 and u.shape[2] == 1:
        u = u[:, :, 0]
        spacing = None if spacing is None else tuple(spacing)[-2:]
    nd = u.dim() - 2
    h = (1.0,) * nd if spacing is None else tuple(float(v) for v in spacing)
    assert len(h) == nd and all(n >= 3 for n in u.shape[2:])

    def at(off):
        return u[(slice(None), slice(None)) + tuple(slice(1 + o, n - 1 + o) for o, n in zip(off, u.shape[2:]))]

    def e(a, s=1):
        return tuple(s if i == a else 0 for i in range(nd))

    def add(p, q):
        return tuple(i + j for i, j in zip(p, q))

    c = at((0,) * nd)
    tot = 0.0
    for a in range(nd):
        uaa = (at(e(a)) - 2.0 * c + at(e(a, -1))) / h[a] ** 2
        tot = tot + uaa ** 2
    for a, b in itertools.combinations(range(nd), 2):
        uab = (at(add(e(a), e(b))) - at(add(e(a), e(b, -1))) - at(add(e(a, -1), e(b))) + at(add(e(a, -1), e(b, -1)))) / (4.0 * h[a] * h[b])
        tot = tot + 2.0 * uab ** 2
    return tot.sum() / tot.numel()


def bending_loss_ref(u, spacing=None, dtype=torch.float64):
    """(loss, dL/du) of the definition on the CPU in `dtype` (float64: the restatement; float32: the yardstick)."""
    x = u.detach().cpu().to(dtype).requires_grad_()
    loss = bending_ref(x, spacing)
    loss.backward()
    return float(loss.detach()), x.grad


def bending_conv(u, spacing=None):
    """The same energy from stock conv ops: every stencil embedded in a 3^nd kernel, so a valid convolution lands on Omega.
    Shares no code with bending_ref."""
    nd = u.dim() - 2
    h = [1.0] * nd if spacing is None else [float(v) for v in spacing]
    conv = F.conv3d if nd == 3 else F.conv2d
    x = u.reshape((-1, 1) + tuple(u.shape[2:]))
    d2 = torch.tensor([1.0, -2.0, 1.0], dtype=u.dtype)
    d1 = torch.tensor([-1.0, 0.0, 1.0], dtype=u.dtype)
    mid = torch.tensor([0.0, 1.0, 0.0], dtype=u.dtype)
    tot = 0.0
    for a in range(nd):
        k = None
        for i in range(nd):
            v = d2 if i == a else mid
            k = v if k is None else torch.tensordot(k, v, dims=0)
        tot = tot + (conv(x, k[None, None]) / h[a] ** 2) ** 2
    for a in range(nd):
        for b in range(a + 1, nd):
            k = None
            for i in range(nd):
                v = d1 if i in (a, b) else mid
                k = v if k is None else torch.tensordot(k, v, dims=0)
            tot = tot + 2.0 * (conv(x, k[None, None] / 4.0) / (h[a] * h[b])) ** 2
    return tot.mean()


def bending_adjoint(u, spacing=None):
    """dL/du by the documented adjoint formula: the derivative values on Omega, extended by 0, pushed back through the
    transposed stencils."""
    nd = u.dim() - 2
    h = (1.0,) * nd if spacing is None else tuple(float(v) for v in spacing)
    sp = tuple(u.shape[2:])
    inner = (slice(None), slice(None)) + tuple(slice(1, n - 1) for n in sp)

    def at(t, off):
        return t[(slice(None), slice(None)) + tuple(slice(1 + o, n - 1 + o) for o, n in zip(off, sp))]

    def shifted(U, off):
        """p -> U(p + off), zero where p + off leaves the volume (U itself is zero outside Omega)."""
        P = F.pad(U, tuple(v for _ in range(nd) for v in (1, 1)))
        return P[(slice(None), slice(None)) + tuple(slice(1 + o, 1 + o + n) for o, n in zip(off, sp))]

    def e(a, s=1):
        return tuple(s if i == a else 0 for i in range(nd))

    def add(p, q):
        return tuple(i + j for i, j in zip(p, q))

    N = u.shape[0] * u.shape[1] * math.prod(n - 2 for n in sp)
    g = torch.zeros_like(u)
    for a in range(nd):
        U = torch.zeros_like(u)
        U[inner] = (at(u, e(a)) - 2.0 * at(u, e(a, 0)) + at(u, e(a, -1))) / h[a] ** 2
        g = g + (shifted(U, e(a, -1)) - 2.0 * U + shifted(U, e(a))) / h[a] ** 2
    for a, b in itertools.combinations(range(nd), 2):
        U = torch.zeros_like(u)
        U[inner] = (at(u, add(e(a), e(b))) - at(u, add(e(a), e(b, -1))) - at(u, add(e(a, -1), e(b)))
                    + at(u, add(e(a, -1), e(b, -1)))) / (4.0 * h[a] * h[b])
        g = g + 2.0 * (shifted(U, add(e(a, -1), e(b, -1))) - shifted(U, add(e(a, -1), e(b)))
                       - shifted(U, add(e(a), e(b, -1))) + shifted(U, add(e(a), e(b)))) / (4.0 * h[a] * h[b])
    return 2.0 / N * g


def _take(x, dim, off):
    n = x.shape[dim]
    return x.index_select(dim, (torch.arange(n) + off).clamp(0, n - 1))


def noise_field(shape, seed):
    """0.7 * normalised(5-wide box-smoothed uniform noise) + 0.3 * uniform noise (seeded), as test_mind.mind_inputs."""
    x = C.rand(seed, *shape).double()
    sm = x
    for ax in range(len(shape) - 2):
        sm = sum(_take(sm, 2 + ax, t) for t in range(-2, 3)) / 5.0
    sm = (sm - sm.min()) / (sm.max() - sm.min())
    return (0.7 * sm + 0.3 * C.rand(seed + 100, *shape).double()).float()


def smooth_field(shape, seed):
    """Per (b, c) the sum of three sinusoids 2 sin(2 pi f . p + phase): every |f_a| <= 1 / 12 (wavelength >= 12 voxels),
    frequencies and phases seeded."""
    B, Cn = shape[:2]
    nd = len(shape) - 2
    f = (C.rand(seed, B, Cn, 3, nd).double() * 2.0 - 1.0) / 12.0
    ph = C.rand(seed + 1, B, Cn, 3).double() * 2.0 * math.pi
    grid = torch.stack(torch.meshgrid(*[torch.arange(n, dtype=torch.float64) for n in shape[2:]], indexing='ij'), 0)
    arg = torch.einsum('bcka,a...->bck...', f, grid) * 2.0 * math.pi + ph.reshape((B, Cn, 3) + (1,) * nd)
    return (2.0 * torch.sin(arg)).sum(2).float()


def field(shape, family, seed=300):
    seed = seed + 11 * SHAPES.index(shape) if shape in SHAPES else seed
    return noise_field(shape, seed) if family == "noise" else smooth_field(shape, seed)


def rel_errors(loss, grad, loss64, grad64):
    """(relative error of the loss, relative 2-norm error of the gradient, its max-abs error over max)."""
    g, g64 = grad.detach().cpu().double(), grad64.double()
    return (abs(float(loss) - loss64) / abs(loss64), float((g - g64).norm() / g64.norm()),
            float((g - g64).abs().max() / g64.abs().max()))


_REF = {}


def reference(case, family):
    """(u, loss64, grad64) of a case, computed once and shared."""
    key = (case, family)
    if key not in _REF:
        shape, spaced = case
        u = field(shape, family)
        _REF[key] = (u,) + bending_loss_ref(u, _spacing(shape, spaced))
    return _REF[key]


def _gpu(u, spacing=None):
    from dfmir_amd import ops
    x = u.to(DEV).requires_grad_()
    loss = ops.bending_energy(x, spacing)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), x.grad.cpu()


def _check(got, ref, family, what):
    el, l2, mx = rel_errors(got[0], got[1], ref[0], ref[1])
    b = BOUND[family]
    print("%s [%s]: loss %.3e (bound %.1e)  grad l2 %.3e (%.1e)  grad max %.3e (%.1e)" % (what, family, el, b[0], l2, b[1], mx, b[2]))
    assert bool(torch.isfinite(got[1]).all()), what
    assert el <= b[0] and l2 <= b[1] and mx <= b[2], (what, family, el, l2, mx)


# ------------------------------------------------------------------------------------------ CPU tier
def test_bend_symbols_in_header_exports_and_ctypes_table():
    import dfmir_amd
    from dfmir_amd import _lib
    from tests.test_abi import header_symbols
    h = ctypes.CDLL(dfmir_amd.LIB_PATH)
    for s in ("dfmir_bend_ws_floats", "dfmir_bend_fwd", "dfmir_bend_bwd"):
        assert s in header_symbols() and s in _lib.exported_symbols() and hasattr(h, s), s
    lib = dfmir_amd.lib()
    assert lib.dfmir_abi_version() == 14
    assert lib.dfmir_bend_ws_floats(1, 3, 16, 16, 16) == 2 * 3 * 1 * 2 * 1          # a double per (plane, chunk, tile)
    assert lib.dfmir_bend_ws_floats(2, 2, 1, 9, 65) == 2 * 4 * 1 * 2 * 2
    assert lib.dfmir_bend_ws_floats(1, 1, 17, 3, 3) == 2 * 2
    for bad in ((1, 1, 2, 8, 8), (1, 1, 8, 2, 8), (1, 1, 8, 8, 2), (1, 1, 1, 8, 1), (0, 1, 8, 8, 8), (1, 0, 8, 8, 8),
                (1, 1, 2048, 1024, 1024)):
        assert lib.dfmir_bend_ws_floats(*bad) == -1, bad


def test_bend_bad_arguments_are_invalid_without_a_device():
    import dfmir_amd
    lib = dfmir_amd.lib()
    assert lib.dfmir_bend_fwd(None, None, None, 1, 3, 8, 8, 8, 1.0, 1.0, 1.0, None) != 0
    assert b"invalid argument" in lib.dfmir_last_error()
    assert lib.dfmir_bend_bwd(None, None, None, 1, 3, 8, 8, 8, 1.0, 1.0, 1.0, None) != 0
    assert b"invalid argument" in lib.dfmir_last_error()
    buf = (ctypes.c_double * 64)()                      # host memory: an argument the checks refuse is never dereferenced
    p = ctypes.cast(buf, ctypes.c_void_p)
    for dims, h in (((1, 3, 2, 8, 8), (1.0, 1.0, 1.0)), ((1, 3, 8, 8, 2), (1.0, 1.0, 1.0)), ((1, 3, 8, 8, 8), (0.0, 1.0, 1.0)),
                    ((1, 3, 8, 8, 8), (1.0, -1.0, 1.0)), ((1, 3, 8, 8, 8), (1.0, 1.0, float('nan'))),
                    ((1, 3, 8, 8, 8), (1.0, float('inf'), 1.0)), ((1, 1, 2048, 1024, 1024), (1.0, 1.0, 1.0))):
        assert lib.dfmir_bend_fwd(p, p, p, *dims, *h, None) != 0, (dims, h)
        assert b"invalid argument" in lib.dfmir_last_error()
        assert lib.dfmir_bend_bwd(p, p, p, *dims, *h, None) != 0, (dims, h)
        assert b"invalid argument" in lib.dfmir_last_error()


def test_bending_rejects_bad_arguments_before_any_launch():
    from dfmir_amd import ops
    from dfmir_amd._lib import DfmirHipError
    from dfmir_amd.losses import BendingEnergy_Loss
    x = torch.rand(1, 3, 8, 8, 8)
    for bad in ((1.0, 1.0), (1.0, 1.0, 0.0), (1.0, -2.0, 1.0), (1.0, float('nan'), 1.0), (1.0, float('inf'), 1.0), 2.0, "111",
                (1.0, "a", 1.0), (True, 1.0, 1.0)):
        with pytest.raises(ValueError, match="spacing"):
            BendingEnergy_Loss(dim=3, spacing=bad)
        with pytest.raises(ValueError, match="spacing"):
            ops.bending_energy(x, bad)
    with pytest.raises(ValueError, match="spacing"):
        BendingEnergy_Loss(dim=2, spacing=(1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="dim"):
        BendingEnergy_Loss(dim=4)
    with pytest.raises(ValueError, match="2-D field"):
        BendingEnergy_Loss(dim=3)(torch.rand(1, 2, 8, 8))
    with pytest.raises(ValueError, match="dims"):
        ops.bending_energy(torch.rand(1, 2, 8))
    for shape in ((1, 3, 2, 8, 8), (1, 3, 8, 2, 8), (1, 3, 8, 8, 2), (1, 3, 1, 8, 2)):
        with pytest.raises(ValueError, match="at least 3"):
            ops.bending_energy(torch.rand(*shape))
        with pytest.raises(ValueError, match="at least 3"):
            BendingEnergy_Loss(dim=3)(torch.rand(*shape), mask=torch.ones(*shape))
    with pytest.raises(ValueError, match="at least 3"):
        BendingEnergy_Loss(dim=2)(torch.rand(1, 2, 2, 8))
    with pytest.raises(ValueError, match="2\\^31"):
        ops.bending_energy(torch.empty(1, 1, 2048, 1024, 1024, device="meta"))
    with pytest.raises(DfmirHipError, match="no CPU fallback"):
        ops.bending_energy(x)
    with pytest.raises(DfmirHipError, match="no CPU fallback"):
        BendingEnergy_Loss(dim=3, spacing=(1.5, 1.0, 0.75))(x)
    with pytest.raises(DfmirHipError, match="no CPU fallback"):
        ops.bending_energy(torch.rand(1, 3, 1, 8, 8), (1.0, 0.75))        # the one-plane volume takes 2 entries or 3
    crit = BendingEnergy_Loss(dim=3, spacing=[2, 1.0, 0.5], loss_mult=0.5)
    assert crit.name == 'bending' and crit.spacing == (2.0, 1.0, 0.5) and crit.loss_mult == 0.5
    assert BendingEnergy_Loss(dim=2).spacing == (1.0, 1.0)


def test_registration3d_constructs_with_bending_and_rejects_unknown():
    from dfmir_amd.losses import BendingEnergy_Loss, Grad_Loss
    from dfmir_amd.registration3d import Registration3DModel
    m = Registration3DModel((8, 8, 8), device="cpu", regularizer="bending", spacing=(1.5, 1.0, 0.75))
    assert isinstance(m.criterionGrad, BendingEnergy_Loss) and m.criterionGrad.spacing == (1.5, 1.0, 0.75)
    assert 'loss_bending' in m._outputs and 'loss_grad' not in m._outputs
    m2 = Registration3DModel((8, 8), device="cpu", regularizer="bending")
    assert isinstance(m2.criterionGrad, BendingEnergy_Loss) and m2.criterionGrad.dim == 2 and 'loss_bending' in m2._outputs
    m3 = Registration3DModel((8, 8, 8), device="cpu")
    assert isinstance(m3.criterionGrad, Grad_Loss) and m3.regularizer == 'diffusion' and 'loss_grad' in m3._outputs
    with pytest.raises(ValueError, match="'diffusion' or 'bending'"):
        Registration3DModel((8, 8, 8), device="cpu", regularizer="elastic")
    with pytest.raises(ValueError, match="spacing"):
        Registration3DModel((8, 8, 8), device="cpu", regularizer="bending", spacing=(1.0, 1.0))


@pytest.mark.parametrize("shape", [(2, 3, 5, 6, 7), (1, 2, 3, 3, 9), (2, 2, 9, 11), (1, 1, 3, 3)], ids=["3d", "3d-thin", "2d", "2d-one"])
@pytest.mark.parametrize("spaced", [False, True], ids=["unit", "spaced"])
@pytest.mark.parametrize("family", FAMILIES)
def test_restatement_equals_the_conv_composition_and_the_adjoint_formula(shape, spaced, family):
    u = field(shape, family, seed=41).double()
    sp = _spacing(shape, spaced)
    loss, g = bending_loss_ref(u, sp)
    x = u.clone().requires_grad_()
    lc = bending_conv(x, sp)
    lc.backward()
    assert loss > 0.0
    assert abs(float(lc.detach()) - loss) <= 1e-13 * loss
    gmax = float(g.abs().max())
    assert float((x.grad - g).abs().max()) <= 1e-13 * gmax
    assert float((bending_adjoint(u, sp) - g).abs().max()) <= 1e-13 * gmax


def test_restatement_takes_a_one_plane_volume_as_its_2d_field():
    u = field((1, 3, 1, 20, 33), "noise").double()
    l3, g3 = bending_loss_ref(u, SPACING)
    l2, g2 = bending_loss_ref(u[:, :, 0], SPACING[1:])
    assert l3 == l2 and torch.equal(g3[:, :, 0], g2)


# ------------------------------------------------------------------------------------------ GPU tier
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_bending_value_and_gradient_vs_restatement(case):
    shape, spaced = case
    for family in FAMILIES:
        u, loss64, g64 = reference(case, family)
        _check(_gpu(u, _spacing(shape, spaced)), (loss64, g64), family, _id(case))


def _grid(shape):
    return torch.meshgrid(*[torch.arange(n, dtype=torch.float32) for n in shape], indexing='ij')


@pytest.mark.gpu
@pytest.mark.parametrize("vol", [(6, 9, 70), (5, 68)], ids=["3d", "2d"])
def test_bending_exact_identities_on_integer_fields(vol):
    g = _grid(vol)
    x, y = g[-1], g[-2]
    affine = 2.0 * x + 3.0 * y - (g[0] if len(vol) == 3 else 0.0) + 5.0
    u = torch.stack([affine, -affine + 7.0], 0)[None]
    loss, grad = _gpu(u)
    assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0
    loss, grad = _gpu(u, SPACING[-len(vol):])
    assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0
    lsq = float(_gpu((x * x)[None, None])[0])           # u_xx = 2 everywhere on Omega, every other term 0
    assert abs(lsq - 4.0) <= 1e-6 * 4.0, lsq
    lxy = float(_gpu((x * y)[None, None])[0])           # u_yx = 1: e = 2 u_yx^2
    assert abs(lxy - 2.0) <= 1e-6 * 2.0, lxy


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 3, 13, 17, 19), (1, 2, 37, 41)], ids=["3d", "2d"])
def test_bending_spacing_two_gives_a_sixteenth(shape):
    u, loss64, _ = reference((shape, False), "noise")
    l1 = float(_gpu(u)[0])
    l2 = float(_gpu(u, (2.0,) * (len(shape) - 2))[0])
    err = abs(l2 - l1 / 16.0) / (l1 / 16.0)
    print("spacing 2: %.3e (bound %.1e)" % (err, BOUND["noise"][0]))
    assert err <= BOUND["noise"][0]
    assert abs(l2 - loss64 / 16.0) <= BOUND["noise"][0] * loss64 / 16.0


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 3, 13, 17, 19), (1, 2, 37, 41)], ids=["3d", "2d"])
def test_bending_loss_mask_and_loss_mult(shape):
    from dfmir_amd.losses import BendingEnergy_Loss
    nd = len(shape) - 2
    u = reference((shape, True), "noise")[0]
    mask = (C.rand(77, *((shape[0], 1) + shape[2:])) > 0.3).float()
    sp = _spacing(shape, True)
    x = u.to(DEV).requires_grad_()
    loss = BendingEnergy_Loss(dim=nd, spacing=sp, loss_mult=0.25)(x, mask=mask)
    loss.backward()
    torch.cuda.synchronize()
    xr = u.double().requires_grad_()
    lr = 0.25 * bending_ref(xr * mask.double(), sp)
    lr.backward()
    _check((loss.detach().cpu(), x.grad.cpu()), (float(lr.detach()), xr.grad), "noise", "mask + loss_mult")
    plain = BendingEnergy_Loss(dim=nd, spacing=sp)(u.to(DEV))
    assert torch.equal(plain.cpu(), _gpu(u, sp)[0])


@pytest.mark.gpu
def test_bending_non_contiguous_and_misaligned_inputs():
    from dfmir_amd import ops
    u = reference(((2, 3, 13, 17, 19), False), "noise")[0]
    want = _gpu(u)
    nc = u.permute(0, 1, 4, 3, 2).contiguous().to(DEV).permute(0, 1, 4, 3, 2).requires_grad_()
    assert not nc.is_contiguous()
    loss = ops.bending_energy(nc)
    loss.backward()
    assert torch.equal(loss.cpu(), want[0]) and torch.equal(nc.grad.cpu(), want[1])
    # W % 4 == 0 but the field starts 4 bytes off a 16-byte boundary: the scalar staging path, the same bits
    for shape in ((1, 1, 4, 4, 64), (1, 1, 5, 64)):
        v = reference((shape, False), "noise")[0]
        want = _gpu(v)
        base = torch.empty(v.numel() + 1, device=DEV)
        off = base[1:].view(shape)
        off.copy_(v)
        assert off.is_contiguous() and off.data_ptr() % 16 == 4
        x = off.requires_grad_()
        loss = ops.bending_energy(x)
        (g,) = torch.autograd.grad(loss, x)
        assert torch.equal(loss.cpu(), want[0]) and torch.equal(g.cpu(), want[1])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 3, 13, 17, 19), (1, 1, 17, 5, 8), (1, 2, 37, 41), (1, 2, 5, 300)],
                         ids=["3d", "3d-vec", "2d", "2d-vec"])
def test_bending_bit_reproducible(shape):
    u = reference((shape, True), "noise")[0]
    sp = _spacing(shape, True)
    r0, r1 = _gpu(u, sp), _gpu(u, sp)
    assert torch.equal(r0[0], r1[0]) and torch.equal(r0[1], r1[1])


def _step_model(capture, similarity):
    from tests import step3d
    return step3d.step_model((16, 16, 16), similarity, capture=capture, regularizer='bending', spacing=SPACING)


@pytest.mark.gpu
def test_registration3d_bending_step_matches_restatement():
    """The flow of a network is neither family; the bound is the larger of the two loss bounds."""
    m, A, B = _step_model(False, 'ncc')
    m.set_input({"A": A, "B": B})
    m.optimize_parameters()
    torch.cuda.synchronize()
    got = m.get_current_losses()
    assert sorted(got) == ["bending", "ncc"]
    ref = bending_loss_ref(m.flow, SPACING)[0]
    err = abs(got["bending"] - ref) / abs(ref)
    bound = max(BOUND["noise"][0], BOUND["smooth"][0])
    print("step loss_bending: %.3e (bound %.1e)" % (err, bound))
    assert ref > 0.0 and err <= bound
    assert float(m.optimizer_R.flat_g.abs().max()) > 0.0


@pytest.mark.gpu
def test_registration3d_bending_captured_step_matches_eager():
    """regularizer='bending' (with similarity='mind') under capture_step=True: a replayed step equals the same step
    enqueued eagerly (the pattern and the tolerances of test_mind.py's captured-step test)."""
    from tests import step3d
    m, A, B = _step_model(True, 'mind')
    m.parallelize()
    step3d.assert_replay_matches_eager(m, {"A": A, "B": B}, ["bending", "mind"])
