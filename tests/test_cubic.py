"""Cubic B-spline resampling (build-defined, dfmir_amd/csrc/cubic.hip): ops.spline_prefilter, ops.warp_cubic, ops.warp(mode='cubic'),
infer.resample and the interp= keyword of the solvers.

The definition, restated here in float64 with torch ops (so that autograd gives d(flow)):
  refl(i), an axis of extent n: n == 1: 0; else j = i mod (2 n - 2), j if j < n else 2 n - 2 - j (the whole-sample mirror
  d c b | a b c d | c b a, at any distance).
  prefilter c = P s, per axis: (c[refl(i - 1)] + 4 c[i] + c[refl(i + 1)]) / 6 = s[i], solved by the two-sweep recursion with
  z = sqrt(3) - 2:  c+[0] = sum_{k < 2 n - 2} z^k s[refl(k)] / (1 - z^(2 n - 2)),  c+[k] = s[k] + z c+[k - 1],
  c-[n - 1] = z / (z^2 - 1) (c+[n - 1] + z c+[n - 2]),  c-[k] = z (c-[k + 1] - c+[k]),  c = 6 c-;  n == 1: c = s.
  sampling at p = x + flow(x), per axis i = floor(p), t = p - i:  w0 = (1 - t)^3 / 6, w1 = (3 t^3 - 6 t^2 + 4) / 6,
  w2 = (-3 t^3 + 3 t^2 + 3 t + 1) / 6, w3 = t^3 / 6;  out = sum over the 4^nd taps of prod_a w_ka(t_a) c[refl(i_a - 1 + k_a)];
  a position that is not finite or has |p| >= 2^24 on any axis gives 0 and a zero gradient.
CPU: the argument checks; the restatement against scipy.ndimage (spline_filter and map_coordinates, order 3, mode 'mirror'),
against itself (interpolation, constants, d(flow) against central differences, continuity of d(flow) across a cell face, the
weights' sums).  GPU: the kernels against the restatement and run to run.

Which launch each GPU shape reaches.  dfmir_spline_prefilter: cb_tile_k<TH, XF, VEC> -- XF = the x axis is filtered (W > 1: a
32 x 64 tile with an x halo, else 64 x 64), VEC = 16-byte accesses (row length % 4 == 0 and aligned pointers); 3-D runs it per
plane over (y, x) and again as the z pass on the view [B C][D][H W]:
  (2,2,9,13)      <32, XF, scalar>, one tile                        (2,2,8,16)     <32, XF, VEC>
  (1,3,1,7,9)     D = 1: the (y, x) pass alone, nothing through tmp  (1,2,3,1,8)    H = 1: y passed through, then the z pass
  (1,1,2,3)       extents 2 and 3: the reflection repeats 16 and 8 times inside the halo
  (1,3,3,7,9)     every halo wider than its axis; <32, XF, scalar> then the z pass <64, no XF, scalar> (H W = 63)
  (1,16,2,6,8)    <32, XF, VEC> then the z pass <64, no XF, VEC> (H W = 48)
  (1,2,300,260)   10 x 5 tiles, partial tiles on both axes
  (1,3,40,70,72)  3 x 2 tiles per plane, and a z pass over 5040 columns = 79 tiles
  and, on (2,3,6,10,12): a non-contiguous input (copied) and an input that starts 4 bytes off a 16-byte boundary (the scalar
  launch on a shape that otherwise takes the 16-byte one).
dfmir_warp_cubic_fwd / _bwd_flow: cw_k<ND, BWD>, one thread per voxel, 256 per workgroup, with a per-voxel choice between the
interior taps and the reflected ones:  <2-D> (2,4,9,13), (2,4,8,16)   <3-D> (2,3,5,12,24), (1,5,2,6,8) (D = 2: no voxel is
interior), (2,1,3,7,9) C = 1, and (1,2,40,70,72): 788 workgroups, mostly interior.

Flows, a different one per sample (tests/test_affine.py's thetas, turned into dense fp32 fields as tests/test_demons.py does):
`zero`; `lattice` = smooth, offsets near integer + 0.5; `shifted` = the same pushed a third of the x extent, a third of the points
past a face; `outside` = twice the extent on every axis; `far` = 20 times the extent: the reflection wraps many times;
`integer` = the lattice flow rounded, with the identity part removed: p lands exactly on voxels, t = 0; `bad` = the lattice flow
with one NaN and one 3e7 entry in sample 0: those two voxels must come out as exactly 0 with a zero gradient, and every other
voxel exactly as in `lattice`.  Images are noise in [-1, 1].  No case is skipped or masked: the value is C2 in p and the
gradient C1, so a float64-against-fp32 disagreement on floor(p) changes nothing beyond rounding.

Tolerances (profiles/cubic_margins.txt, profiles/cubic_margins_cpu.txt): every kernel-against-float64 comparison is bounded by
4x the error of the SAME restatement evaluated by torch in fp32 on the CPU against float64, on these inputs, the maximum over
the case set per quantity (prefilter, forward, d(flow)), over the small shapes and over the large ones separately; fields in
relative 2-norm and as max-abs over max.  scripts/cubic_margins.py measures them, with the kernels' own errors beside them;
the smaller figure of the two files stands below."""
import math

import pytest
import torch

from tests import test_affine as TA
from tests.golden import common as C

DEV = "cuda"
FACTOR = 4.0
# rows "max" of the fp32 CPU columns: the smaller of profiles/cubic_margins.txt and profiles/cubic_margins_cpu.txt per quantity
FP32_ERR = {"prefilter": {"small": {"l2": 1.12e-07, "max": 2.04e-07}, "large": {"l2": 9.87e-08, "max": 2.37e-07}},
            "forward": {"small": {"l2": 2.95e-05, "max": 5.79e-05}, "large": {"l2": 4.52e-06, "max": 7.53e-06}},
            "dflow": {"small": {"l2": 2.50e-05, "max": 5.04e-05}, "large": {"l2": 4.02e-06, "max": 7.31e-06}}}

PREFILTER_SHAPES = [(2, 2, 9, 13), (2, 2, 8, 16), (1, 3, 1, 7, 9), (1, 2, 3, 1, 8), (1, 1, 2, 3), (1, 3, 3, 7, 9), (1, 16, 2, 6, 8),
                    (1, 2, 300, 260), (1, 3, 40, 70, 72)]
STRIDED_SHAPE = (2, 3, 6, 10, 12)
WARP_SHAPES = [(2, 4, 9, 13), (2, 4, 8, 16), (2, 3, 5, 12, 24), (1, 5, 2, 6, 8), (2, 1, 3, 7, 9), (1, 2, 40, 70, 72)]
KINDS = ("zero", "lattice", "shifted", "outside", "far", "integer", "bad")
PMAX = 2.0 ** 24


def group_of(shape):
    return "large" if math.prod(shape) > 100000 else "small"


def _id(v):
    return "x".join(str(n) for n in v)


def field_errors(got, ref):
    l2, mx = TA._l2_max(got, ref)
    return {"l2": l2, "max": mx}


# ------------------------------------------------------------------------------------------ restatement
def refl(i, n):
    """refl(i) for an integer tensor i and an axis of extent n."""
    if n == 1:
        return torch.zeros_like(i)
    per = 2 * n - 2
    j = torch.remainder(i, per)
    return torch.where(j < n, j, per - j)


def prefilter_line_ref(s):
    """The recursion along the LAST axis of s, in s's dtype."""
    n = s.shape[-1]
    if n == 1:
        return s.clone()
    z = torch.tensor(math.sqrt(3.0) - 2.0, dtype=s.dtype)
    k = torch.arange(2 * n - 2)
    zk = z ** k.to(s.dtype)
    cp = [(s[..., refl(k, n)] * zk).sum(-1) / (1.0 - z ** (2 * n - 2))]
    for i in range(1, n):
        cp.append(s[..., i] + z * cp[-1])
    cm = [None] * n
    cm[n - 1] = z / (z * z - 1.0) * (cp[n - 1] + z * cp[n - 2])
    for i in range(n - 2, -1, -1):
        cm[i] = z * (cm[i + 1] - cp[i])
    return 6.0 * torch.stack(cm, -1)


def prefilter_ref(x, dtype=torch.float64):
    """ops.spline_prefilter on the CPU in `dtype`: the recursion along every axis in turn."""
    y = x.detach().cpu().to(dtype)
    for a in range(2, y.dim()):
        y = prefilter_line_ref(y.movedim(a, -1)).movedim(-1, a)
    return y.contiguous()


def weights_ref(t):
    """(w [4, ...], w' [4, ...]) at t."""
    u = 1.0 - t
    w = torch.stack([u ** 3 / 6.0, (3.0 * t ** 3 - 6.0 * t ** 2 + 4.0) / 6.0, (-3.0 * t ** 3 + 3.0 * t ** 2 + 3.0 * t + 1.0) / 6.0,
                     t ** 3 / 6.0])
    dw = torch.stack([-u ** 2 / 2.0, (3.0 * t ** 2 - 4.0 * t) / 2.0, (-3.0 * t ** 2 + 2.0 * t + 1.0) / 2.0, t ** 2 / 2.0])
    return w, dw


def sample_ref(coef, p):
    """The spline of the coefficients coef [B,C,*vol] at the positions p [B,nd,*vol] (in coef's dtype; differentiable in p)."""
    B, Cn = coef.shape[:2]
    vol = tuple(coef.shape[2:])
    nd = len(vol)
    bad = (~torch.isfinite(p) | (p.abs() >= PMAX)).any(1, keepdim=True)
    p = torch.where(bad, torch.zeros_like(p), p)
    fl = torch.floor(p.detach())
    t = p - fl
    i0 = fl.long() - 1
    w = [weights_ref(t[:, a])[0] for a in range(nd)]                                # [4,B,*vol] per axis
    idx = [[refl(i0[:, a] + k, vol[a]) for k in range(4)] for a in range(nd)]
    strides = [math.prod(vol[a + 1:]) for a in range(nd)]
    flat = coef.reshape(B, Cn, -1)
    out = torch.zeros_like(coef)
    taps = [(k,) for k in range(4)]
    for _ in range(nd - 1):
        taps = [tp + (k,) for tp in taps for k in range(4)]
    for tp in taps:
        lin = sum(idx[a][tp[a]] * strides[a] for a in range(nd)).reshape(B, 1, -1).expand(B, Cn, -1)
        wt = w[0][tp[0]]
        for a in range(1, nd):
            wt = wt * w[a][tp[a]]
        out = out + wt[:, None] * flat.gather(2, lin).reshape(coef.shape)
    return torch.where(bad, torch.zeros_like(out), out)


def warp_cubic_ref(src, flow, dtype=torch.float64, prefiltered=False):
    """ops.warp_cubic on the CPU in `dtype`; differentiable in `flow` when it requires grad (pass it in `dtype` then)."""
    coef = src.detach().cpu().to(dtype) if prefiltered else prefilter_ref(src, dtype)
    f = flow if flow.requires_grad else flow.detach().cpu().to(dtype)
    return sample_ref(coef, TA._grid(tuple(src.shape[2:]), dtype)[None] + f)


def warp_cubic_ref_grad(src, flow, dout, dtype=torch.float64):
    """(out, dflow) of the restatement in `dtype`, dflow by autograd."""
    f = flow.detach().cpu().to(dtype).requires_grad_()
    out = warp_cubic_ref(src, f, dtype)
    (g,) = torch.autograd.grad((out * dout.to(dtype)).sum(), f)
    return out.detach(), g


# ------------------------------------------------------------------------------------------ inputs
def image(shape, seed=2300):
    return C.rand(seed + sum(shape), *shape) * 2 - 1


def warp_flow(shape, kind):
    """The fp32 flow [B,nd,*vol] of a warp case (see the module docstring)."""
    B, vol = shape[0], tuple(shape[2:])
    nd = len(vol)
    seed = 2500 + 13 * WARP_SHAPES.index(shape)
    if kind == "zero":
        return torch.zeros(B, nd, *vol)
    if kind == "far":
        th = TA.thetas(shape, "outside", seed).double()
        th[:, :, nd] = torch.tensor([[(20.0 + b) * n + 0.5 for n in vol] for b in range(B)], dtype=torch.float64)
        return TA.affine_flow_ref(th, vol).float()
    if kind in ("integer", "bad"):
        flow = TA.affine_flow_ref(TA.thetas(shape, "lattice", seed).double(), vol).float()
        if kind == "integer":
            return torch.round(flow)
        flat = flow.reshape(B, nd, -1)
        S = flat.shape[2]
        flat[0, 0, S // 3] = float('nan')
        flat[0, nd - 1, (2 * S) // 3] = 3.0e7
        return flow
    return TA.affine_flow_ref(TA.thetas(shape, kind, seed).double(), vol).float()


def bad_voxels(shape):
    S = math.prod(shape[2:])
    return [S // 3, (2 * S) // 3]


def warp_inputs(shape, kind):
    """(src, flow, dout) fp32 of a warp case."""
    return image(shape), warp_flow(shape, kind), C.rand(2700 + sum(shape), *shape) * 2 - 1


_REF = {}


def warp_reference(shape, kind):
    """((src, flow, dout), (out, dflow) in float64), computed once."""
    key = (shape, kind)
    if key not in _REF:
        inp = warp_inputs(shape, kind)
        _REF[key] = (inp, warp_cubic_ref_grad(*inp))
    return _REF[key]


def prefilter_reference(shape):
    key = ("prefilter", shape)
    if key not in _REF:
        x = image(shape)
        _REF[key] = (x, prefilter_ref(x))
    return _REF[key]


# ------------------------------------------------------------------------------------------ CPU tier
def test_value_errors_are_raised_before_any_launch():
    from dfmir_amd import infer, ops
    E = pytest.raises(ValueError)
    x = torch.zeros(2, 3, 8, 12)
    flow = torch.zeros(2, 2, 8, 12)
    with E: ops.spline_prefilter(None)
    with E: ops.spline_prefilter(x[0])
    with E: ops.spline_prefilter(x.double())
    with E: ops.spline_prefilter(torch.zeros(2, 0, 8, 12))
    with E: ops.spline_prefilter(torch.zeros(2, 3, 0, 12))
    with E: ops.spline_prefilter(x.clone().requires_grad_())
    with pytest.raises(Exception, match="no CPU fallback"): ops.spline_prefilter(x)
    with pytest.raises(Exception, match="no CPU fallback"): ops.spline_prefilter(torch.zeros(1, 1, 1, 5))      # extent 1 is legal
    for fn in (ops.warp_cubic, lambda s, f: ops.warp(s, f, mode='cubic')):
        with E: fn(None, flow)
        with E: fn(x, None)
        with E: fn(x[0], flow)
        with E: fn(x.double(), flow)
        with E: fn(x, flow.double())
        with E: fn(x, flow[:, :1])
        with E: fn(x, flow[:1])
        with E: fn(x, flow[:, :, :4])
        with E: fn(x, torch.zeros(2, 3, 8, 12))
        with E: fn(torch.zeros(2, 0, 8, 12), flow)
        with E: fn(torch.zeros(2, 3, 2, 8, 12), flow)
        with pytest.raises(Exception, match="no CPU fallback"): fn(x, flow)
    with E: ops.warp_cubic(x, flow, prefiltered=1)
    with E: ops.warp_cubic(x, flow, prefiltered="yes")
    im, fx = torch.zeros(2, 1, 8, 12), torch.zeros(2, 1, 8, 12)
    for bad in ('nearest', 'bicubic', 'Cubic', 3, None, True):
        with E: infer.refine_flow(im, fx, features='intensity', lam=0.1, lr=0.1, iters=1, interp=bad)
        with E: infer.demons_flow(im, fx, features='intensity', iters=1, interp=bad)
        with E: infer.affine_init(im, fx, features='intensity', iters=1, interp=bad)
        with E: infer.resample(im, flow, interp=bad)
    with E: infer.resample(None, flow)
    with E: infer.resample(im, flow[:, :1])
    for interp in infer.INTERPS:
        with pytest.raises(Exception, match="no CPU fallback"): infer.resample(im, flow, interp=interp)
        with pytest.raises(Exception, match="no CPU fallback"): infer.demons_flow(im, fx, features='intensity', iters=1, interp=interp)


def test_restatement_matches_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    import numpy as np
    for n in (1, 2, 3, 5, 17, 64):
        s = (C.rand(90 + n, 3, n).double() * 2 - 1)
        want = ndi.spline_filter1d(s.numpy(), order=3, axis=-1, mode='mirror')
        assert float((prefilter_line_ref(s) - torch.from_numpy(want)).abs().max()) <= 1e-13, n
    for shape in ((1, 1, 7, 9), (1, 1, 2, 3), (1, 1, 3, 5, 4), (1, 1, 1, 6, 1)):
        x = image(shape).double()
        want = ndi.spline_filter(x[0, 0].numpy(), order=3, mode='mirror')
        coef = prefilter_ref(x)
        assert float((coef[0, 0] - torch.from_numpy(want)).abs().max()) <= 1e-13, shape
        vol = shape[2:]
        pts = torch.stack([C.rand(77 + a, 200).double() * (n + 32.0) - 12.0 for a, n in enumerate(vol)])         # [-12, n + 20]
        pts[:, :5] = torch.round(pts[:, :5])                                              # on the lattice too
        want = ndi.map_coordinates(x[0, 0].numpy(), pts.numpy(), order=3, mode='mirror')
        got = torch.stack([_sample_points(coef, pts[:, i]) for i in range(200)])
        assert float((got - torch.from_numpy(np.asarray(want))).abs().max()) <= 1e-12, shape


def _sample_points(coef, pt):
    """The spline of coef [1,1,*vol] at ONE position pt [nd]: sample_ref on a flow that sends voxel 0 there."""
    vol = tuple(coef.shape[2:])
    flow = torch.zeros((1, len(vol)) + vol, dtype=coef.dtype)
    flow[(0, slice(None)) + (0,) * len(vol)] = pt
    return sample_ref(coef, TA._grid(vol, coef.dtype)[None] * 0 + flow)[(0, 0) + (0,) * len(vol)]


def test_restatement_interpolates_keeps_constants_and_weights_sum():
    for shape in PREFILTER_SHAPES[:7] + WARP_SHAPES[:5]:
        x = image(shape).double()
        zero = torch.zeros((shape[0], len(shape) - 2) + tuple(shape[2:]), dtype=torch.float64)
        assert float((warp_cubic_ref(x, zero) - x).abs().max()) <= 1e-12, shape                 # the interpolation property
        const = torch.full(shape, 0.75, dtype=torch.float64)
        assert float((prefilter_ref(const) - 0.75).abs().max()) <= 1e-13
        if shape in WARP_SHAPES:
            out = warp_cubic_ref(const, warp_flow(shape, "shifted"))
            assert float((out - 0.75).abs().max()) <= 1e-13
        # the defining equation, per axis
        c = prefilter_ref(x)
        back = c
        for a in range(2, len(shape)):
            n = shape[a]
            i = torch.arange(n)
            m = back.movedim(a, -1)
            back = ((m[..., refl(i - 1, n)] + 4.0 * m + m[..., refl(i + 1, n)]) / 6.0 if n > 1 else m).movedim(-1, a)
        assert float((back - x).abs().max()) <= 1e-12, shape
    t = torch.linspace(0.0, 1.0, 101, dtype=torch.float64)
    w, dw = weights_ref(t)
    assert float((w.sum(0) - 1.0).abs().max()) <= 1e-15 and float(dw.sum(0).abs().max()) <= 1e-15
    assert float(w.min()) >= 0.0
    tt = t.clone().requires_grad_()
    for k in range(4):                                                                        # w' is the derivative of w
        (g,) = torch.autograd.grad(weights_ref(tt)[0][k].sum(), tt)
        assert float((g - dw[k]).abs().max()) <= 1e-15
    bad = warp_cubic_ref(image((1, 2, 6, 7)), torch.full((1, 2, 6, 7), float('inf')))
    assert float(bad.abs().max()) == 0.0
    # the spline is not confined to the range of src: it overshoots at an edge
    step = torch.zeros(1, 1, 1, 12, dtype=torch.float64)
    step[..., 6:] = 1.0
    over = warp_cubic_ref(step, torch.full((1, 2, 1, 12), 0.5, dtype=torch.float64))
    assert float(over.max()) > 1.0 and float(over.min()) < 0.0


@pytest.mark.parametrize("shape", WARP_SHAPES[:5], ids=_id)
def test_restated_gradient_matches_central_differences_and_is_continuous(shape):
    nd = len(shape) - 2
    for kind in ("lattice", "shifted", "far"):
        (src, flow, dout), (out, g) = warp_reference(shape, kind)
        h = 1e-5
        for a in range(nd):
            e = torch.zeros_like(flow, dtype=torch.float64)
            e[:, a] = h
            hi = warp_cubic_ref(src, flow.double() + e)
            lo = warp_cubic_ref(src, flow.double() - e)
            fd = ((hi - lo) * dout.double()).sum(1) / (2 * h)
            assert float((fd - g[:, a]).abs().max()) <= 1e-8 * max(1.0, float(g.abs().max())), (shape, kind, a)
    # across a cell face: positions k - 1e-9 and k + 1e-9 give gradients that agree to 1e-7
    (src, flow, dout), _ = warp_reference(shape, "integer")
    below = warp_cubic_ref_grad(src, flow.double() - 1e-9, dout)[1]
    above = warp_cubic_ref_grad(src, flow.double() + 1e-9, dout)[1]
    assert float((below - above).abs().max()) <= 1e-7
    vol = tuple(shape[2:])
    p = TA._grid(vol, torch.float64)[None] + flow.double()
    assert bool((torch.floor(p - 1e-9) == torch.floor(p + 1e-9) - 1).all())                   # the two sides ARE different cells
    _, (_, gbad) = warp_reference(shape, "bad")
    flat = gbad.reshape(shape[0], nd, -1)
    assert float(flat[0, :, bad_voxels(shape)].abs().max()) == 0.0 and bool(torch.isfinite(gbad).all())


# ------------------------------------------------------------------------------------------ GPU tier
def _bounded(errs, what, bound, factor=FACTOR):
    print("%s: " % what + "  ".join("%s %.3e (bound %.1e)" % (k, v, factor * bound[k]) for k, v in errs.items()))
    assert all(v <= factor * bound[k] for k, v in errs.items()), (what, errs)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _gpu_prefilter(x):
    from dfmir_amd import ops
    y = ops.spline_prefilter(x.to(DEV))
    assert y.is_contiguous() and y.dtype == torch.float32 and not y.requires_grad and y.shape == x.shape
    return y.cpu()


def _gpu_warp(src, flow, dout, prefiltered=False):
    """(out, dflow) of ops.warp_cubic on the device, back on the CPU."""
    from dfmir_amd import ops
    f = flow.to(DEV).requires_grad_()
    s = src.to(DEV)
    out = ops.warp_cubic(ops.spline_prefilter(s) if prefiltered else s, f, prefiltered=prefiltered)
    (g,) = torch.autograd.grad(out, f, dout.to(DEV))
    assert out.dtype == g.dtype == torch.float32 and out.shape == src.shape and g.shape == flow.shape
    return out.detach().cpu(), g.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", PREFILTER_SHAPES, ids=_id)
def test_spline_prefilter_matches_float64_and_is_reproducible(shape):
    x, ref = prefilter_reference(shape)
    y = _gpu_prefilter(x)
    assert bool(torch.isfinite(y).all())
    _bounded(field_errors(y, ref), "spline_prefilter %s" % _id(shape), FP32_ERR["prefilter"][group_of(shape)])
    assert torch.equal(y, _gpu_prefilter(x))
    if len(shape) == 5 and 1 in shape[2:]:                                    # an axis of extent 1 passes through bit for bit:
        a = 2 + shape[2:].index(1)                                            # the result is the 2-D one of the other two axes
        assert torch.equal(_bits(y.squeeze(a)), _bits(_gpu_prefilter(x.squeeze(a))))


@pytest.mark.gpu
def test_spline_prefilter_extent_one_bits_strided_and_misaligned_inputs():
    from dfmir_amd import ops
    odd = torch.tensor([0.0, -0.0, float('inf'), -1.5, 1e-42], device=DEV)
    for shape in ((1, 5, 1, 1), (1, 5, 1, 1, 1)):                             # every axis of extent 1: the bits as they stand
        x = odd.reshape(shape)
        assert torch.equal(_bits(ops.spline_prefilter(x)), _bits(x))
    line = (C.rand(7, 1, 2, 1, 9) * 2 - 1).to(DEV)                             # H = 1: the result is the x filter alone, and the
    col = line.reshape(1, 2, 9, 1)                                            # same numbers whichever axis carries them
    assert torch.equal(ops.spline_prefilter(line).reshape(-1), ops.spline_prefilter(col).reshape(-1))
    vol3 = line.reshape(1, 2, 1, 1, 9)
    assert torch.equal(ops.spline_prefilter(vol3).reshape(-1), ops.spline_prefilter(line).reshape(-1))
    zcol = line.reshape(1, 2, 9, 1, 1)                                        # the z pass alone
    assert torch.equal(ops.spline_prefilter(zcol).reshape(-1), ops.spline_prefilter(line).reshape(-1))
    shape = STRIDED_SHAPE
    x = image(shape)
    ref = prefilter_ref(x)
    bound = FP32_ERR["prefilter"]["small"]
    full = _gpu_prefilter(x)
    _bounded(field_errors(full, ref), "contiguous", bound)
    strided = x.to(DEV).permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
    assert not strided.is_contiguous()
    assert torch.equal(ops.spline_prefilter(strided).cpu(), full)
    base = torch.empty(x.numel() + 1, device=DEV)
    off = base[1:].view(shape).copy_(x.to(DEV))
    assert off.data_ptr() % 16 == 4
    got = ops.spline_prefilter(off).cpu()
    _bounded(field_errors(got, ref), "misaligned", bound)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", WARP_SHAPES, ids=_id)
def test_warp_cubic_matches_float64_and_is_reproducible(shape, kind):
    from dfmir_amd import ops
    from dfmir_amd._lib import DfmirHipError
    from dfmir_amd.voxelmorph import SpatialTransformer
    (src, flow, dout), (ref_out, ref_g) = warp_reference(shape, kind)
    grp = group_of(shape)
    what = "%s %s" % (_id(shape), kind)
    out, g = _gpu_warp(src, flow, dout)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(g).all()), what
    _bounded(field_errors(out, ref_out), "warp_cubic forward " + what, FP32_ERR["forward"][grp])
    _bounded(field_errors(g, ref_g), "warp_cubic d(flow) " + what, FP32_ERR["dflow"][grp])
    again = _gpu_warp(src, flow, dout)
    assert torch.equal(out, again[0]) and torch.equal(g, again[1]), what
    pre = _gpu_warp(src, flow, dout, prefiltered=True)
    assert torch.equal(_bits(out), _bits(pre[0])) and torch.equal(_bits(g), _bits(pre[1])), what
    s, f = src.to(DEV), flow.to(DEV)
    assert torch.equal(_bits(ops.warp(s, f, mode='cubic').cpu()), _bits(out))
    assert torch.equal(_bits(SpatialTransformer(shape[2:], mode='cubic').to(DEV)(s, f).cpu()), _bits(out))
    for mode, code in (("bilinear", 0), ("nearest", 1)):                        # the other modes did not move
        assert torch.equal(_bits(ops.warp(s, f, mode=mode)), _bits(ops._warp_fwd(s, f, code, 0))), mode
    if kind == "zero":                                                         # the interpolation property, in fp32
        assert float((out - src).abs().max()) <= FACTOR * FP32_ERR["forward"][grp]["max"] * float(ref_out.abs().max())
    if kind == "bad":
        nd = len(shape) - 2
        vox = bad_voxels(shape)
        assert float(out.reshape(shape[0], shape[1], -1)[0, :, vox].abs().max()) == 0.0
        assert float(g.reshape(shape[0], nd, -1)[0, :, vox].abs().max()) == 0.0
        lat_out, lat_g = _gpu_warp(src, warp_flow(shape, "lattice"), dout)      # every other voxel: unaffected
        keep = torch.ones(math.prod(shape[2:]), dtype=torch.bool)
        keep[vox] = False
        assert torch.equal(out.reshape(shape[0], shape[1], -1)[..., keep], lat_out.reshape(shape[0], shape[1], -1)[..., keep])
        assert torch.equal(g.reshape(shape[0], nd, -1)[..., keep], lat_g.reshape(shape[0], nd, -1)[..., keep])
        assert torch.equal(out[1:], lat_out[1:])
    sg = src.to(DEV).requires_grad_()
    with pytest.raises(DfmirHipError):
        ops.warp_cubic(sg, f).sum().backward()


@pytest.mark.gpu
def test_interp_keyword_changes_only_the_warped_image():
    from dfmir_amd import infer, ops
    mov, fix, _ = TA.recovery_fixture((24, 32))
    mov, fix = mov.float().to(DEV), fix.float().to(DEV)
    assert tuple(mov.shape) == (1, 1, 24, 32)
    calls = {"refine_flow": (infer.refine_flow, dict(features='intensity', lam=0.05, lr=0.1, iters=1)),
             "demons_flow": (infer.demons_flow, dict(features='intensity', levels=(2, 1), iters=1)),
             "affine_init": (infer.affine_init, dict(features='intensity', levels=(2, 1), iters=1))}
    for name, (fn, kw) in calls.items():
        lin = fn(mov, fix, **kw)
        default = fn(mov, fix, interp='linear', **kw)
        cub = fn(mov, fix, interp='cubic', **kw)
        assert sorted(lin) == sorted(cub)
        for k in lin:
            assert torch.equal(lin[k], default[k]), (name, k)
            if k != 'warped':
                assert torch.equal(lin[k], cub[k]), (name, k)                  # flow, history, ...: bit-identical
        assert torch.equal(lin['warped'], ops.warp(mov, lin['flow'])), name
        assert torch.equal(cub['warped'], ops.warp_cubic(mov, cub['flow'])), name
        assert torch.equal(infer.resample(mov, cub['flow']), cub['warped']), name
        assert torch.equal(infer.resample(mov, cub['flow'], interp='cubic'), cub['warped']), name
        assert torch.equal(infer.resample(mov, cub['flow'], interp='linear'), lin['warped']), name
        assert not cub['warped'].requires_grad
