"""ops.bspline_flow (build-defined, dfmir_amd/csrc/bspline.hip), the cubic B-spline free-form deformation, and
infer.refine_flow(parametrisation='bspline') built on it: the C ABI and the argument checks (CPU); two float64 restatements of
the definition -- the gather form (per axis y[x] = sum_l B_l(t) c[q + l], q = x // s, t = (x % s) / s) and the depthwise
conv_transpose with the separable kernel k[(3 - l) s + r] = B_l(r / s) cropped to [3 s, 3 s + n) -- checked against each other
and for partition of unity, linear precision and the adjoint identity on the CPU; a float64 restatement of the refinement loop
with the B-spline in place of the linear interpolation; and on the GPU the kernels against all of it.

Which launch each GPU case reaches.  Forward, bs_fwd_k<ND, VEC>: a workgroup owns a 32 x 32 in-plane tile of one plane and, in
3-D, one cell of z (the s_z slices that share four control planes); VEC = 16-byte stores when W % 4 == 0.  Backward: bs_bwd_x_k
(a workgroup stages min(8, 8192 // padded W) whole rows of dy, a wave per row, 64 voxels and then 64 control columns of the row
at a time), then bs_bwd_axis_k along y and, in 3-D, along z (one thread per output).
  (2,2,9,13) s 2        <2, scalar>; one partial tile; 36 rows: the fifth row group is partial; dead last row and column
  (2,2,8,16) s 4        <2, VEC>
  (1,2,40,36) s 8       <2, VEC>; 2 x 2 tiles, the far ones partial
  (1,3,7,11,13) s 3     <3, scalar>; three cells of z, the last one cut short by the volume (one slice of three)
  (2,3,5,6,8) s 1       <3, VEC>; every cell is one slice, weights (1/6, 4/6, 1/6, 0), every last control point dead
  (1,3,16,20,24) s 4    <3, VEC>; the refinement volume
  (1,3,3,4,5) s 4       <3, scalar>; one cell, cut short on every axis; m = (4,4,5)
  (1,3,6,10,16) s 1,2,4 <3, VEC>; per-axis spacing
  (1,1,4,40,72) s 8     <3, VEC>; C = 1; 2 x 3 tiles; rows of 72: a wave of bs_bwd_x_k stages its row in two rounds
Added for paths the issue's set leaves unreached (the precedent of tests/test_dsearch.py):
  (1,1,2,1024) s 8      padded W = 1055: bs_bwd_x_k sizes its workgroup for 7 rows instead of 8 (the case has two rows: two
                        waves take one each); m_x = 131: three rounds of control columns per row; 32 tiles along x

Inputs: ctrl and dy are seeded noise in [-1, 1].

Tolerances (profiles/bspline_margins.txt): every comparison with the float64 restatement is bounded by FACTOR = 4 times the error
of the SAME definition (the gather form) evaluated by torch in fp32 on the CPU against float64 on the same inputs -- the maxima
over the case set of max-abs over max and of the relative 2-norm, forward and adjoint (the adjoint of the fp32 evaluation by
autograd).  scripts/bspline_margins.py measures them, the kernels' own errors beside them, and the same pair of figures for the
final similarity of the 40-iteration loop."""
import ctypes
import inspect

import pytest
import torch
import torch.nn.functional as F

from tests import ref64
from tests import test_refine as R
from tests.golden import common as C

DEV = "cuda"
FACTOR = 4.0
# profiles/bspline_margins.txt, row "max" of the fp32 CPU columns: (max-abs over max, relative 2-norm)
FP32_FWD = (2.44e-07, 1.49e-07)
FP32_ADJ = (1.75e-07, 1.54e-07)
# the final similarity of the 40-iteration B-spline loop at spacing 4: |fp32 CPU - fp64| / fp64 (profiles/bspline_margins.txt)
REFINE_FP32_GAP = 2.19e-03
BOUND_FWD = tuple(FACTOR * e for e in FP32_FWD)
BOUND_ADJ = tuple(FACTOR * e for e in FP32_ADJ)

CASES = [((2, 2, 9, 13), 2), ((2, 2, 8, 16), 4), ((1, 2, 40, 36), 8), ((1, 3, 7, 11, 13), 3), ((2, 3, 5, 6, 8), 1),
         ((1, 3, 16, 20, 24), 4), ((1, 3, 3, 4, 5), 4), ((1, 3, 6, 10, 16), (1, 2, 4)), ((1, 1, 4, 40, 72), 8),
         ((1, 1, 2, 1024), 8)]
CONTROL = [(8, 10), (5, 7), (8, 8), (6, 7, 8), (8, 9, 11), (7, 8, 9), (4, 4, 5), (9, 8, 7), (4, 8, 12), (4, 131)]
SPACING = 4
BSPLINE_KW = dict(R.REFINE_KW, grid_downsize=SPACING)


def _id(case):
    shape, stride = case
    st = "".join(str(s) for s in stride) if isinstance(stride, tuple) else str(stride)
    return "x".join(str(v) for v in shape) + "-s" + st


def strides(case):
    shape, stride = case
    return stride if isinstance(stride, tuple) else (stride,) * (len(shape) - 2)


# ------------------------------------------------------------------------------------------ restatements
def control_shape(vol, stride):
    return tuple((n - 1) // s + 4 for n, s in zip(vol, stride))


def basis(t):
    """[4, len(t)]: the uniform cubic B-spline basis B_0 .. B_3 at t, in t's dtype"""
    return torch.stack([(1 - t) ** 3 / 6, (3 * t ** 3 - 6 * t ** 2 + 4) / 6, (-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / 6, t ** 3 / 6])


def expand_gather(ctrl, vol, stride):
    """The definition, gather form, in ctrl's dtype: axis after axis, y[x] = sum_l B_l(t(x)) c[q(x) + l].  Differentiable."""
    y = ctrl
    for a, (n, s) in enumerate(zip(vol, stride)):
        x = torch.arange(n)
        q, t = x // s, (x % s).to(ctrl.dtype) / s
        B = basis(t)
        shape = [1] * y.dim()
        shape[2 + a] = n
        y = sum(B[l].reshape(shape) * y.index_select(2 + a, q + l) for l in range(4))
    return y


def expand_conv_transpose(ctrl, vol, stride):
    """The same field as a depthwise conv_transpose with stride s of the separable kernel k_a[(3 - l) s_a + r] = B_l(r / s_a),
    cropped to [3 s_a, 3 s_a + n_a)."""
    nd, Cn = len(vol), ctrl.shape[1]
    ks = []
    for s in stride:
        B = basis(torch.arange(s, dtype=ctrl.dtype) / s)                    # [4, s]
        ks.append(torch.stack([B[3 - i] for i in range(4)]).reshape(-1))    # position (3 - l) s + r
    k = ks[0]
    for a in range(1, nd):
        k = k[..., None] * ks[a].reshape((1,) * a + (-1,))
    w = k[None, None].expand((Cn, 1) + tuple(k.shape)).contiguous()
    full = (F.conv_transpose3d if nd == 3 else F.conv_transpose2d)(ctrl, w, stride=tuple(stride), groups=Cn)
    for a, (n, s) in enumerate(zip(vol, stride)):
        full = full.narrow(2 + a, 3 * s, n)
    return full


def inputs(case):
    """(ctrl, dy) fp32 noise in [-1, 1] of a case"""
    shape, _ = case
    seed = 1300 + 19 * CASES.index(case)
    m = control_shape(shape[2:], strides(case))
    return C.rand(seed, *(tuple(shape[:2]) + m)) * 2 - 1, C.rand(seed + 1, *shape) * 2 - 1


def evaluate(case, ctrl, dy, dtype):
    """(y, dctrl) of the gather form on the CPU in `dtype` (float64: the restatement; float32: the yardstick), the adjoint by
    autograd"""
    c = ctrl.detach().cpu().to(dtype).requires_grad_()
    y = expand_gather(c, case[0][2:], strides(case))
    (g,) = torch.autograd.grad(y, c, dy.detach().cpu().to(dtype))
    return y.detach(), g


_REF = {}


def reference(case):
    """((ctrl, dy), (y64, dctrl64)) of a case, computed once and shared"""
    if case not in _REF:
        inp = inputs(case)
        _REF[case] = (inp, evaluate(case, inp[0], inp[1], torch.float64))
    return _REF[case]


def errors(got, ref):
    """(max-abs over max, relative 2-norm) of a tensor against the restatement's"""
    g, r = got.detach().cpu().double(), ref.double()
    return float((g - r).abs().max() / r.abs().max()), float((g - r).norm() / r.norm())


def _gpu(case, ctrl, dy):
    from dfmir_amd import ops
    c = ctrl.to(DEV).requires_grad_()
    y = ops.bspline_flow(c, case[0][2:], case[1])
    (g,) = torch.autograd.grad(y, c, dy.to(DEV))
    torch.cuda.synchronize()
    return y.detach(), g


def bspline_refine_ref(moving, fixed, dtype=torch.float64, grid_downsize=SPACING, iters=40, lr=0.1, lam=0.05,
                       betas=(0.9, 0.999), **_):
    """The loop of infer.refine_flow(parametrisation='bspline') restated on the CPU in `dtype` (flow = None, features =
    'intensity', the diffusion penalty): tests.test_refine.refine_ref with the gather form in place of F.interpolate.
    Returns (flow [1,nd,*vol], history [iters + 1, 2])."""
    M, Fx = moving.detach().cpu().to(dtype), fixed.detach().cpu().to(dtype)
    vol = tuple(M.shape[2:])
    nd = len(vol)
    st = (grid_downsize,) * nd
    opt = ref64.Adam(torch.zeros((M.shape[0], nd) + control_shape(vol, st)), lr, betas, 1e-8, dtype=dtype)
    hist = torch.zeros(iters + 1, 2, dtype=dtype)
    for k in range(iters + 1):
        d = opt.p.clone().requires_grad_(k < iters)
        flow = expand_gather(d, vol, st)
        sim = R.ssd_grid_sample(M, Fx, flow)[0]
        reg = ref64.grad_loss(flow, 'l2', dtype=dtype)
        hist[k, 0], hist[k, 1] = sim.detach(), reg.detach()
        if k < iters:
            (g,) = torch.autograd.grad(sim + lam * reg, d)
            opt.step(g)
    return flow.detach(), hist


_REFINE = {}


def refine_reference():
    """((moving, fixed, true), (flow64, history64)) of the B-spline loop at spacing 4, computed once and shared"""
    if not _REFINE:
        inp = R.refine_input()
        _REFINE["r"] = (inp, bspline_refine_ref(inp[0], inp[1], **BSPLINE_KW))
    return _REFINE["r"]


# ------------------------------------------------------------------------------------------ CPU tier
def test_bspline_symbols_in_header_exports_and_ctypes_table():
    import dfmir_amd
    from dfmir_amd import _lib, ops
    from tests.test_abi import header_symbols
    h = ctypes.CDLL(dfmir_amd.LIB_PATH)
    for s, nargs in (("dfmir_bspline_fwd", 11), ("dfmir_bspline_bwd_ws_floats", 8), ("dfmir_bspline_bwd", 12)):
        assert s in header_symbols() and s in _lib.exported_symbols() and hasattr(h, s), s
        assert len(_lib._SIGS[s]) == nargs, s
    lib = dfmir_amd.lib()
    assert lib.dfmir_abi_version() == 14
    # the two intermediates: planes D H m_x and planes D m_y m_x, each rounded up to 4 floats; 2-D has the first alone
    assert lib.dfmir_bspline_bwd_ws_floats(3, 3, 16, 20, 24, 4, 4, 4) == 3 * 16 * 20 * 9 + 3 * 16 * 8 * 9
    assert lib.dfmir_bspline_bwd_ws_floats(2, 4, 999, 9, 13, 999, 2, 2) == 4 * 9 * 10    # nd == 2: D and sz are not read
    for bad in ((1, 1, 8, 8, 8, 2, 2, 2), (3, 0, 8, 8, 8, 2, 2, 2), (3, 1, 0, 8, 8, 2, 2, 2), (3, 1, 8, 8, 8, 0, 2, 2),
                (3, 1, 8, 8, 8, 2, 9, 2), (3, 65536, 8, 8, 8, 2, 2, 2), (3, 1, 2048, 2048, 2048, 2, 2, 2),
                (3, 1, 260, 260, 260, 1, 1, 1), (2, 1, 1, 4, 7945, 1, 2, 2)):
        assert lib.dfmir_bspline_bwd_ws_floats(*bad) == -1, bad
    assert lib.dfmir_bspline_bwd_ws_floats(2, 1, 1, 4, 7944, 1, 2, 2) > 0
    assert lib.dfmir_bspline_fwd(3, None, None, 1, 8, 8, 8, 2, 2, 2, None) != 0
    assert b"invalid argument" in lib.dfmir_last_error()
    assert lib.dfmir_bspline_bwd(3, None, None, 1, 8, 8, 8, 2, 2, 2, None, None) != 0
    for name in ("BSplineFn", "bspline_flow", "bspline_control_shape"):
        assert hasattr(ops, name), name
    assert ops.BSPLINE_MAX_STRIDE == 8


def test_bspline_control_shape_on_the_case_set():
    from dfmir_amd import ops
    for case, want in zip(CASES, CONTROL):
        assert ops.bspline_control_shape(case[0][2:], case[1]) == want, case
        assert control_shape(case[0][2:], strides(case)) == want, case
    assert ops.bspline_control_shape([5, 6], (1, 8)) == (8, 4)
    assert ops.bspline_control_shape(torch.Size([1, 1, 1]), 8) == (4, 4, 4)


def test_bspline_flow_argument_checks_raise_before_the_device_is_asked_for():
    """Every call here is made with CPU tensors: a check that came after the device was asked for would raise DfmirHipError
    ("no CPU fallback") instead."""
    from dfmir_amd import ops
    z = torch.zeros
    for bad in (0, 9, True, 2.0, "2", None, (2, 2), (2, 2, 2, 2), (2, 0, 2), (2, True, 2), [2, 2.0, 2]):
        with pytest.raises(ValueError, match="stride"):
            ops.bspline_flow(z(1, 3, 5, 5, 5), (4, 4, 4), bad)
        with pytest.raises(ValueError, match="stride"):
            ops.bspline_control_shape((4, 4, 4), bad)
    for bad in ((4, 4, 4, 4), (4,), (4, 0, 4), (4, 4.0, 4), 4, None, (4, True, 4)):
        with pytest.raises(ValueError, match="vol"):
            ops.bspline_flow(z(1, 3, 5, 5, 5), bad, 2)
        with pytest.raises(ValueError, match="vol"):
            ops.bspline_control_shape(bad, 2)
    with pytest.raises(ValueError, match="stride"):
        ops.bspline_flow(z(1, 2, 5, 5), (4, 4, 4), (2, 2))                 # a 2-D stride with a 3-D volume: the volume decides
    with pytest.raises(ValueError, match="fp32"):
        ops.bspline_flow(z(1, 3, 5, 5, 5, dtype=torch.float64), (4, 4, 4), 2)
    with pytest.raises(ValueError, match="fp32"):
        ops.bspline_flow(z(1, 3, 5, 5, 5, dtype=torch.float16), (4, 4, 4), 2)
    with pytest.raises(ValueError, match="fp32"):
        ops.bspline_flow([[0.0]], (4, 4, 4), 2)
    for shape in ((1, 3, 5, 5, 6), (1, 3, 5, 5), (3, 5, 5, 5), (1, 3, 4, 4, 4), (0, 3, 5, 5, 5), (1, 0, 5, 5, 5)):
        with pytest.raises(ValueError, match="control grid"):
            ops.bspline_flow(z(*shape), (4, 4, 4), 2)
    with pytest.raises(ValueError, match="control grid"):
        ops.bspline_flow(z(1, 3, 5, 5, 5), (4, 4, 4), (2, 2, 1))


def test_refine_flow_parametrisation_argument_checks():
    from dfmir_amd import infer
    z = torch.zeros(1, 1, 8, 8, 8)
    kw = dict(features='intensity', lam=0.05, lr=0.1)
    with pytest.raises(ValueError, match="parametrisation"):
        infer.refine_flow(z, z, parametrisation='cubic', **kw)
    for bad in (9, 0, True, (2, 2), 2.0, (2, 2, 9)):
        with pytest.raises(ValueError, match="grid_downsize"):
            infer.refine_flow(z, z, parametrisation='bspline', grid_downsize=bad, **kw)
    with pytest.raises(ValueError, match="grid_downsize"):
        infer.refine_flow(z, z, parametrisation='linear', grid_downsize=(2, 2, 2), **kw)     # a tuple is B-spline only
    sig = inspect.signature(infer.refine_flow)
    positional = [n for n, p in sig.parameters.items() if p.kind is not inspect.Parameter.KEYWORD_ONLY]
    assert positional == ["moving", "fixed", "flow"]
    assert sig.parameters["parametrisation"].default == 'linear'
    assert sig.parameters["parametrisation"].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["grid_downsize"].default == 2 and sig.parameters["update"].default == 'add'


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_restatements_agree_and_reproduce_constants(case):
    """float64: gather form == conv_transpose form to 1e-12; a constant grid gives the constant (partition of unity)."""
    shape, _ = case
    vol, st = shape[2:], strides(case)
    ctrl = inputs(case)[0].double()
    a, b = expand_gather(ctrl, vol, st), expand_conv_transpose(ctrl, vol, st)
    assert tuple(a.shape) == tuple(shape) and tuple(b.shape) == tuple(shape)
    assert float((a - b).abs().max()) <= 1e-12
    const = expand_gather(torch.full_like(ctrl, 0.75), vol, st)
    assert float((const - 0.75).abs().max()) <= 1e-12


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_restatement_has_linear_precision(case):
    """ctrl[j] = alpha s (j - 1) along one axis (the control points' own coordinates, scaled) gives y = alpha x along it."""
    shape, _ = case
    vol, st = shape[2:], strides(case)
    m = control_shape(vol, st)
    alpha = 0.37
    for a in range(len(vol)):
        view = [1] * (2 + len(vol))
        view[2 + a] = m[a]
        ctrl = (alpha * st[a] * (torch.arange(m[a], dtype=torch.float64) - 1)).reshape(view).expand((1, 1) + m)
        y = expand_gather(ctrl, vol, st)
        view[2 + a] = vol[a]
        want = (alpha * torch.arange(vol[a], dtype=torch.float64)).reshape(view).expand((1, 1) + tuple(vol))
        assert float((y - want).abs().max()) <= 1e-12 * max(1.0, alpha * vol[a])


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_restatement_adjoint_identity_and_dead_control_points(case):
    """float64: <B c, y> = <c, B^T y> with B^T from autograd; where (n - 1) % s == 0 the last control slab's gradient is 0."""
    (ctrl, dy), (y64, g64) = reference(case)
    lhs, rhs = float((y64 * dy.double()).sum()), float((ctrl.double() * g64).sum())
    assert abs(lhs - rhs) <= 1e-12 * float(y64.norm() * dy.double().norm())
    for a, (n, s) in enumerate(zip(case[0][2:], strides(case))):
        if (n - 1) % s == 0:
            slab = g64.select(2 + a, g64.shape[2 + a] - 1)
            assert torch.equal(slab, torch.zeros_like(slab)), (case, a)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_adjoint_identity_inputs_have_no_accidental_cancellation(case):
    """The input property the device's adjoint-identity test rests on, in float64: <B c, y> of the seeded noise is at least
    1 / 512 of |B c| |y| (the cases measure 1 / 12 to 1 / 401; noise gives about 1 / sqrt(voxels))."""
    (ctrl, dy), (y64, g64) = reference(case)
    lhs, scale = float((y64 * dy.double()).sum()), float(y64.norm() * dy.double().norm())
    print("%s: <B c, y> %.6e, |B c| |y| / |<B c, y>| = %.1f" % (_id(case), lhs, scale / abs(lhs)))
    assert abs(lhs) * 512.0 >= scale


def test_bspline_loop_restatement_beats_the_linear_loop():
    """The float64 B-spline loop on the blob pair at spacing 4 ends with lower similarity and flow error than it starts with
    (7.26e-3 -> 9.0e-5; 1.220 -> 1.053 voxels) and with lower final similarity than the linear loop of tests/test_refine.py at
    the same spacing (1.89e-4); profiles/bspline_margins.txt records the figures."""
    (moving, fixed, true), (flow, hist) = refine_reference()
    lin_flow, lin_hist = R.refine_ref(moving, fixed, **BSPLINE_KW)
    before, after = R.flow_error(torch.zeros_like(true), true), R.flow_error(flow, true)
    print("B-spline: similarity %.4e -> %.4e, flow error %.4f -> %.4f; linear: similarity -> %.4e, flow error -> %.4f"
          % (float(hist[0, 0]), float(hist[-1, 0]), before, after, float(lin_hist[-1, 0]), R.flow_error(lin_flow, true)))
    assert float(hist[0, 1]) == 0.0 and float(hist[0, 0]) == float(lin_hist[0, 0])
    assert float(hist[-1, 0]) < float(hist[0, 0])
    assert after < before
    assert float(hist[-1, 0]) < float(lin_hist[-1, 0])


# ------------------------------------------------------------------------------------------ GPU tier
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_bspline_flow_matches_fp64(case):
    (ctrl, dy), (y64, g64) = reference(case)
    y, g = _gpu(case, ctrl, dy)
    ef, ea = errors(y, y64), errors(g, g64)
    print("%s: forward max %.3e l2 %.3e (bounds %.1e %.1e); adjoint max %.3e l2 %.3e (bounds %.1e %.1e)"
          % ((_id(case),) + ef + BOUND_FWD + ea + BOUND_ADJ))
    assert tuple(y.shape) == tuple(case[0]) and tuple(g.shape) == tuple(ctrl.shape)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(g).all())
    assert ef[0] <= BOUND_FWD[0] and ef[1] <= BOUND_FWD[1], (case, ef)
    assert ea[0] <= BOUND_ADJ[0] and ea[1] <= BOUND_ADJ[1], (case, ea)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_bspline_dead_control_points_and_zero_grid(case):
    """Exactly zero: the gradient of a last control slab that only meets B_3(0) = 0, and the field of a zero grid (+0.0 bit for
    bit: refine_flow's "iteration 0 evaluates `flow` itself" rests on it)."""
    from dfmir_amd import ops
    ctrl, dy = inputs(case)
    _, g = _gpu(case, ctrl, dy)
    for a, (n, s) in enumerate(zip(case[0][2:], strides(case))):
        if (n - 1) % s == 0:
            slab = g.select(2 + a, g.shape[2 + a] - 1)
            assert torch.equal(slab, torch.zeros_like(slab)), (case, a)
    y = ops.bspline_flow(torch.zeros_like(ctrl).to(DEV), case[0][2:], case[1])
    assert not y.view(torch.int32).any()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_bspline_adjoint_identity_on_the_device(case):
    """<fwd(c), y> and <c, bwd(y)> of the device's own outputs, both accumulated in float64 on the host, agree to 2 x (forward
    bound + adjoint bound), the 2-norm bounds, relative to the inner product itself.  An inner product of noise is a small
    share of |fwd(c)| |y| (about 1 / sqrt(voxels)), so an accidental cancellation would make the relative figure meaningless:
    test_adjoint_identity_inputs_have_no_accidental_cancellation asserts on the CPU that no case has one; the bound is not
    widened for it."""
    ctrl, dy = inputs(case)
    y, g = _gpu(case, ctrl, dy)
    y, g, c, d = y.cpu().double(), g.cpu().double(), ctrl.double(), dy.double()
    lhs, rhs = float((y * d).sum()), float((c * g).sum())
    bound = 2.0 * (BOUND_FWD[1] + BOUND_ADJ[1])
    print("%s: <fwd c, y> %.9e  <c, bwd y> %.9e  relative %.3e (bound %.1e)"
          % (_id(case), lhs, rhs, abs(lhs - rhs) / abs(lhs), bound))
    assert abs(lhs - rhs) <= bound * abs(lhs)


@pytest.mark.gpu
def test_bspline_flow_refuses_at_the_forward_what_the_backward_cannot_do():
    """W = 7945 is one past what bs_bwd_x_k stages: a grid that needs a gradient is refused when the field is formed, not at
    backward time; without a gradient the forward runs (249 tiles along x, scalar stores) and matches float64."""
    from dfmir_amd import ops
    from dfmir_amd._lib import DfmirHipError
    vol, st = (2, 7945), 8
    ctrl = C.rand(1421, 1, 1, *ops.bspline_control_shape(vol, st)) * 2 - 1
    with pytest.raises(DfmirHipError, match="backward"):
        ops.bspline_flow(ctrl.to(DEV).requires_grad_(), vol, st)
    y = ops.bspline_flow(ctrl.to(DEV), vol, st)
    e = errors(y, expand_gather(ctrl.double(), vol, (st, st)))
    assert e[0] <= BOUND_FWD[0] and e[1] <= BOUND_FWD[1], e


@pytest.mark.gpu
def test_bspline_is_bit_reproducible():
    for case in (CASES[5], CASES[0]):
        ctrl, dy = inputs(case)
        a, b = _gpu(case, ctrl, dy), _gpu(case, ctrl, dy)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.gpu
def test_bspline_planes_are_independent_and_layout_does_not_matter():
    from dfmir_amd import ops
    vol, st = (7, 11, 13), 3
    m = ops.bspline_control_shape(vol, st)
    ctrl = (C.rand(1411, 2, 3, *m) * 2 - 1).to(DEV)
    dy = (C.rand(1412, 2, 3, *vol) * 2 - 1).to(DEV)
    case = ((2, 3) + vol, st)
    y, g = _gpu(case, ctrl, dy)
    halves = [_gpu(((1, 3) + vol, st), ctrl[b:b + 1].contiguous(), dy[b:b + 1].contiguous()) for b in range(2)]
    assert torch.equal(y, torch.cat([h[0] for h in halves])) and torch.equal(g, torch.cat([h[1] for h in halves]))
    # non-contiguous ctrl and dy: channel-last storage, and a slice of a wider tensor
    last = lambda t: t.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)
    c_nc, d_nc = last(ctrl), last(dy)
    assert not c_nc.is_contiguous() and not d_nc.is_contiguous()
    y2, g2 = _gpu(case, c_nc, d_nc)
    assert torch.equal(y, y2) and torch.equal(g, g2)
    wide = torch.zeros(2, 3, m[0], m[1], m[2] + 3, device=DEV)
    wide[..., 1:1 + m[2]] = ctrl
    y3, g3 = _gpu(case, wide[..., 1:1 + m[2]], dy)
    assert torch.equal(y, y3) and torch.equal(g, g3)


@pytest.mark.gpu
def test_refine_flow_bspline_follows_the_fp64_loop():
    """The start is flow=None, so no sample point is planted near a lattice point (where the similarity's gradient has a kink
    and a rounding error can pick the other side); the bound is 4x the fp32 CPU loop's own gap.  Measured: a gap of 7.6e-3
    against the bound of 8.8e-3 (profiles/bspline_margins.txt)."""
    from dfmir_amd import infer, ops
    (moving, fixed, true), (flow64, hist64) = refine_reference()
    mv, fx = moving.to(DEV), fixed.to(DEV)
    out = infer.refine_flow(mv, fx, features='intensity', parametrisation='bspline', **BSPLINE_KW)
    assert sorted(out) == ["control", "flow", "history", "warped"]
    hist = out['history'].cpu().double()
    zero = torch.zeros(1, 3, *R.REFINE_VOL, device=DEV)
    assert tuple(hist.shape) == (41, 2) and out['history'].is_cuda
    assert torch.equal(out['history'][0, 0], ops.warp_ssd(mv, fx, zero))           # iteration 0 evaluates flow0 itself
    assert torch.equal(out['history'][40, 0], ops.warp_ssd(mv, fx, out['flow']))
    assert torch.equal(out['warped'], ops.warp(mv, out['flow']))
    assert tuple(out['control'].shape) == (1, 3) + ops.bspline_control_shape(R.REFINE_VOL, SPACING) == (1, 3, 7, 8, 9)
    assert torch.equal(out['flow'], ops.bspline_flow(out['control'], R.REFINE_VOL, SPACING))
    before, after = R.flow_error(zero, true), R.flow_error(out['flow'], true)
    gap = abs(float(hist[40, 0]) - float(hist64[40, 0])) / float(hist64[40, 0])
    print("similarity %.6e -> %.6e (fp64 loop %.6e -> %.6e, relative gap %.3e, bound %.1e); flow error %.4f -> %.4f"
          % (float(hist[0, 0]), float(hist[40, 0]), float(hist64[0, 0]), float(hist64[40, 0]), gap,
             FACTOR * REFINE_FP32_GAP, before, after))
    assert float(hist[40, 0]) < float(hist[0, 0])
    assert after < before
    assert gap <= FACTOR * REFINE_FP32_GAP


@pytest.mark.gpu
def test_refine_flow_bspline_options():
    from dfmir_amd import infer, ops
    moving, fixed, _ = R.refine_input()
    mv, fx = moving.to(DEV), fixed.to(DEV)
    kw = dict(features='intensity', lam=0.05, lr=0.1, parametrisation='bspline', grid_downsize=SPACING)
    flow0 = ((C.rand(77, 1, 3, *R.REFINE_VOL) * 2 - 1) * 0.7).to(DEV)
    out = infer.refine_flow(mv, fx, flow0, iters=0, **kw)
    assert torch.equal(out['flow'], flow0) and out['flow'].data_ptr() != flow0.data_ptr()      # bit for bit, a copy
    assert tuple(out['history'].shape) == (1, 2) and torch.equal(out['history'][0, 0], ops.warp_ssd(mv, fx, flow0))
    assert tuple(out['control'].shape) == (1, 3, 7, 8, 9) and not out['control'].any()
    for update in ('add', 'compose'):
        out = infer.refine_flow(mv, fx, flow0, iters=2, update=update, **kw)
        assert torch.equal(out['history'][0, 0], ops.warp_ssd(mv, fx, flow0)), update
        assert bool(torch.isfinite(out['history']).all()) and bool(torch.isfinite(out['flow']).all())
    finite = lambda o: bool(torch.isfinite(o['history']).all()) and bool(torch.isfinite(o['flow']).all())
    # 2-D with MIND features at 32 x 32; per-axis spacing in 3-D; the bending penalty; a volume below one control cell
    a2, b2 = mv[:, :, 8, :16, :16].repeat(1, 1, 2, 2).contiguous(), fx[:, :, 8, :16, :16].repeat(1, 1, 2, 2).contiguous()
    out = infer.refine_flow(a2, b2, features='mind', iters=3, lam=0.05, lr=0.1, parametrisation='bspline', grid_downsize=4)
    assert tuple(out['flow'].shape) == (1, 2, 32, 32) and tuple(out['control'].shape) == (1, 2, 11, 11) and finite(out)
    out = infer.refine_flow(mv, fx, iters=3, **dict(kw, grid_downsize=(2, 4, 4)))
    assert tuple(out['control'].shape) == (1, 3, 11, 8, 9) and finite(out)
    out = infer.refine_flow(mv, fx, iters=3, regularizer='bending', spacing=(2.0, 1.0, 1.0), **kw)
    assert finite(out)
    out = infer.refine_flow(mv[:, :, :3, :4, :5].contiguous(), fx[:, :, :3, :4, :5].contiguous(), iters=2, **kw)
    assert tuple(out['control'].shape) == (1, 3, 4, 4, 5) and finite(out)


@pytest.mark.gpu
def test_refine_flow_linear_is_untouched_by_the_keyword():
    from dfmir_amd import infer
    moving, fixed, _ = R.refine_input()
    mv, fx = moving.to(DEV), fixed.to(DEV)
    flow0 = ((C.rand(77, 1, 3, *R.REFINE_VOL) * 2 - 1) * 0.7).to(DEV)
    kw = dict(features='intensity', iters=5, lam=0.05, lr=0.1)
    a = infer.refine_flow(mv, fx, flow0, **kw)
    b = infer.refine_flow(mv, fx, flow0, parametrisation='linear', **kw)
    assert sorted(a) == sorted(b) == ["flow", "history", "warped"]
    for k in a:
        assert torch.equal(a[k], b[k]), k
