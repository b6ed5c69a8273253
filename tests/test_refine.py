"""WarpedSSD_Loss / ops.warp_ssd (build-defined, dfmir_amd/csrc/warpssd.hip) and infer.refine_flow, the instance optimisation
built on it: the C ABI and the argument checks (CPU); a float64 restatement of the definition -- the value from
F.grid_sample(align_corners=True, padding_mode='zeros') followed by the (masked) mean, the flow gradient from the documented
closed form written out with corner differences -- checked on the CPU against autograd through grid_sample; a float64
restatement of the refinement loop; and on the GPU the kernels against both.

Which launch each GPU shape reaches (dfmir_warp_ssd_fwd_grad: <ND, VPT, PACKED> of ws_fwd_k; VPT = 4, 16-byte accesses of
phi, F and the gradient, when W % 4 == 0 and the pointers are aligned, else 1; a workgroup owns 256 * VPT consecutive voxels
of one sample; channels pass in groups of four):
  <2-D, VPT 1>  (2,4,9,13)           <2-D, VPT 4>  (2,4,8,16)
  <3-D, VPT 4>  (2,12,5,12,24) 1440 voxels = 2 workgroups per sample, three channel groups; (1,5,2,6,8) C = 5: a second group
                with one live channel
  <3-D, VPT 1>  (2,1,3,7,9) C = 1
Every case runs on the packed gather and, under DFMIR_WARPSSD_PLANAR, on the channel-major one.  ws_fin_k runs after every
forward, ws_bwd_k in every backward, ws_pack_k once per case.

Inputs come in two seeded families.  `lattice`: phi = k + f, k integer-valued in [-3, 3], f uniform in [0.05, 0.95]: every
sample point lies at least 0.05 from a cell boundary (the gradient has no kink nearby and the normalised-coordinate round trip
of grid_sample cannot pick the other cell), and the integer part pushes samples past every face of every volume here.
`integer`: phi = k exactly, samples ON the lattice, where the gradient is one-sided: only the values are compared.  M and F are
noise in [-1, 1].  Masks: none, `partial` (float weights, zero on a third of the voxels) and `zero`.

Tolerances (profiles/refine_margins.txt): every comparison with the restatement is bounded by 4x the error of the SAME
definition evaluated by torch in fp32 on the CPU against float64, on these inputs -- the maxima over the case set, per family:
the loss and L_b (relative), the gradient in relative 2-norm and as max-abs over max.  scripts/refine_margins.py measures them,
the kernels' own errors beside them, and the same pair of figures for the final similarity of the refinement loop."""
import ctypes
import inspect
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import ref64
from tests.golden import common as C

DEV = "cuda"
FACTOR = 4.0
# profiles/refine_margins.txt, rows "max" of the fp32 CPU columns: (loss, L_b, dflow 2-norm, dflow max)
FP32_ERR = {"lattice": (1.11e-07, 1.36e-07, 8.82e-07, 1.17e-06), "integer": (1.10e-07, 1.47e-07, None, None)}
BOUND = {k: tuple(None if e is None else FACTOR * e for e in v) for k, v in FP32_ERR.items()}
# the final similarity of the 40-iteration loop below: |fp32 CPU - fp64| / fp64 (profiles/refine_margins.txt)
REFINE_FP32_GAP = 3.18e-03
FAMILIES = ("lattice", "integer")
MASKS = ("none", "partial", "zero")
PATHS = ("packed", "planar")
SHAPES = [(2, 4, 9, 13), (2, 4, 8, 16), (2, 12, 5, 12, 24), (2, 1, 3, 7, 9), (1, 5, 2, 6, 8)]


def _id(shape):
    return "x".join(str(v) for v in shape)


# ------------------------------------------------------------------------------------------ restatement
def _grid(vol, dtype):
    return torch.stack(torch.meshgrid(*[torch.arange(n, dtype=dtype) for n in vol], indexing='ij'), 0)


def _reduce(e2c, mask):
    """(L, L_b [B]) of e2c = mean_c e^2 [B,1,*vol]: the plain mean, or sum m e2c / sum m with 0 for an empty mask."""
    B = e2c.shape[0]
    if mask is None:
        per = e2c.reshape(B, -1).mean(1)
        return per.mean(), per
    m = mask.to(e2c.dtype).expand_as(e2c)
    num, den = (m * e2c).reshape(B, -1).sum(1), m.reshape(B, -1).sum(1)
    safe = lambda n, d: n / d if float(d) > 0 else n * 0.0
    return safe(num.sum(), den.sum()), torch.stack([safe(num[b], den[b]) for b in range(B)])


def ssd_grid_sample(M, Fx, phi, mask=None):
    """(L, L_b) from F.grid_sample: normalised coordinates, align_corners=True, zero padding, then the (masked) mean.
    Differentiable in phi."""
    nd = phi.shape[1]
    vol = tuple(phi.shape[2:])
    f = _grid(vol, phi.dtype)[None] + phi
    norm = [2.0 * f[:, a] / (vol[a] - 1) - 1.0 for a in range(nd)]
    grid = torch.stack(norm[::-1], -1)                       # last axis: x, y(, z)
    warped = F.grid_sample(M, grid, mode='bilinear', padding_mode='zeros', align_corners=True)
    return _reduce(((warped - Fx) ** 2).mean(1, keepdim=True), mask)


def ssd_closed_form(M, Fx, phi, mask=None):
    """(L, L_b, dL/dphi) by the documented formulas with explicit floor / gather indexing, in phi's dtype:
    dL/dphi_d = k sum_c e_c d_d M_c, d_d = corner differences (+ upper, - lower along d, times the other axes' weights),
    zero-padded corners taking part as zeros; k = 2 / (B C S), masked 2 m / (C sum m)."""
    B, nd = phi.shape[:2]
    Cn = M.shape[1]
    vol = tuple(phi.shape[2:])
    S = math.prod(vol)
    f = _grid(vol, phi.dtype)[None] + phi
    i0 = torch.floor(f)
    w1 = f - i0
    w = (1.0 - w1, w1)
    i0 = i0.long()
    strides = [math.prod(vol[a + 1:]) for a in range(nd)]
    Mf = M.reshape(B, Cn, S)
    val = torch.zeros_like(M)
    dM = [torch.zeros_like(M) for _ in range(nd)]
    for bits in itertools.product((0, 1), repeat=nd):
        flat = torch.zeros((B,) + vol, dtype=torch.long)
        valid = torch.ones((B,) + vol, dtype=torch.bool)
        for a in range(nd):
            ia = i0[:, a] + bits[a]
            valid &= (ia >= 0) & (ia < vol[a])
            flat += ia.clamp(0, vol[a] - 1) * strides[a]
        v = torch.gather(Mf, 2, flat.reshape(B, 1, S).expand(B, Cn, S)).reshape(M.shape) * valid.to(M.dtype)[:, None]
        wa = [w[bits[a]][:, a] for a in range(nd)]
        val = val + math.prod(wa[1:], start=wa[0])[:, None] * v
        for d in range(nd):
            others = torch.ones_like(wa[0])
            for a in range(nd):
                if a != d:
                    others = others * wa[a]
            dM[d] = dM[d] + (1.0 if bits[d] else -1.0) * others[:, None] * v
    e = val - Fx
    loss, per = _reduce((e ** 2).mean(1, keepdim=True), mask)
    if mask is None:
        k = torch.full((B, 1) + vol, 2.0 / (B * Cn * S), dtype=phi.dtype)
    else:
        m = mask.to(phi.dtype).expand((B, 1) + vol)
        k = 2.0 * m / (Cn * m.sum()) if float(m.sum()) > 0 else m * 0.0
    dphi = torch.stack([(e * dM[d]).sum(1) for d in range(nd)], 1) * k
    return loss, per, dphi


def ssd_ref(M, Fx, phi, mask=None, dtype=torch.float64):
    """(L, L_b, dL/dphi) on the CPU in `dtype` (float64: the restatement; float32: the yardstick): the value from
    grid_sample and the (masked) mean, the gradient from the closed form."""
    a, b, p = (t.detach().cpu().to(dtype) for t in (M, Fx, phi))
    m = None if mask is None else mask.detach().cpu().to(dtype)
    loss, per = ssd_grid_sample(a, b, p, m)
    return loss, per, ssd_closed_form(a, b, p, m)[2]


# ------------------------------------------------------------------------------------------ inputs
def inputs(shape, family, mask="none", seed=900):
    """(M, F, phi, mask or None) fp32 of a case."""
    seed = seed + 17 * SHAPES.index(shape) if shape in SHAPES else seed
    B, vol = shape[0], tuple(shape[2:])
    nd = len(vol)
    M = C.rand(seed, *shape) * 2 - 1
    Fx = C.rand(seed + 1, *shape) * 2 - 1
    k = torch.floor(C.rand(seed + 2, B, nd, *vol).double() * 7.0).clamp(0, 6) - 3.0
    if family == "lattice":
        k = k + 0.05 + 0.9 * C.rand(seed + 3, B, nd, *vol).double()
    m = None
    if mask == "partial":
        m = C.rand(seed + 4, B, 1, *vol)
        m = torch.where(m < 1.0 / 3.0, torch.zeros_like(m), m)
    elif mask == "zero":
        m = torch.zeros(B, 1, *vol)
    return M, Fx, k.float(), m


def errors(got, ref, values_only=False):
    """(loss, L_b, dflow 2-norm, dflow max) of (L, L_b, dflow) against the restatement's; None where not compared."""
    rel = lambda g, r: float(((g.detach().cpu().double() - r.double()).abs() / r.double().abs()).max())
    out = [rel(got[0].reshape(1), ref[0].reshape(1)), rel(got[1], ref[1])]
    if values_only:
        return tuple(out) + (None, None)
    g, r = got[2].detach().cpu().double(), ref[2].double()
    return tuple(out) + (float((g - r).norm() / r.norm()), float((g - r).abs().max() / r.abs().max()))


_REF = {}


def reference(shape, family, mask):
    """((M, F, phi, m), (L64, L_b64, dflow64)) of a case, computed once and shared."""
    key = (shape, family, mask)
    if key not in _REF:
        inp = inputs(shape, family, mask)
        _REF[key] = (inp, ssd_ref(*inp))
    return _REF[key]


class planar_path(object):
    """DFMIR_WARPSSD_PLANAR for the duration of a block (a process-global option: always unset again)."""

    def __init__(self, path):
        self.on = path == "planar"

    def __enter__(self):
        from dfmir_amd import _lib
        if self.on:
            _lib.set_option("DFMIR_WARPSSD_PLANAR", "1")

    def __exit__(self, *a):
        from dfmir_amd import _lib
        if self.on:
            _lib.set_option("DFMIR_WARPSSD_PLANAR", None)


def _gpu(M, Fx, phi, mask, path="packed", gout=1.0):
    from dfmir_amd import ops
    with planar_path(path):
        p = phi.to(DEV).requires_grad_()
        m = None if mask is None else mask.to(DEV)
        h = ops.pack_features(M.to(DEV))
        loss = ops.warp_ssd(h, Fx.to(DEV), p, m)
        (loss * gout).backward()
        per = ops.warp_ssd_per_sample(h, Fx.to(DEV), p.detach(), m)
        torch.cuda.synchronize()
    return loss.detach().cpu(), per.cpu(), p.grad.cpu()


def _check(got, ref, family, what):
    e = errors(got, ref, values_only=family == "integer")
    b = BOUND[family]
    print("%s [%s]: " % (what, family) + "  ".join("%s %.3e (bound %.1e)" % (n, x, y) for n, x, y in
                                                     zip(("loss", "L_b", "dflow l2", "dflow max"), e, b) if x is not None))
    assert bool(torch.isfinite(got[2]).all()), what
    assert all(x <= y for x, y in zip(e, b) if x is not None), (what, family, e)


# ------------------------------------------------------------------------------------------ the refinement input and loop
REFINE_VOL = (16, 20, 24)
REFINE_KW = dict(grid_downsize=2, iters=40, lr=0.1, lam=0.05, regularizer='diffusion')


def refine_input():
    """(moving, fixed, true) fp32: one channel of six Gaussian blobs [1,1,16,20,24]; `true` a smooth sinusoidal field of
    amplitude 1.5 voxels per component; fixed = moving warped by it (float64 grid_sample), so `true` registers the pair."""
    vol = REFINE_VOL
    g = _grid(vol, torch.float64)
    ctr = C.rand(71, 6, 3).double() * 0.6 + 0.2
    sig = 2.0 + 1.5 * C.rand(72, 6).double()
    moving = torch.zeros(vol, dtype=torch.float64)
    for i in range(6):
        d2 = sum((g[a] - ctr[i, a] * (vol[a] - 1)) ** 2 for a in range(3))
        moving = moving + torch.exp(-d2 / (2.0 * sig[i] ** 2))
    moving = moving[None, None]
    ph = [0.3, 1.1, 2.0]
    true = torch.stack([1.5 * torch.sin(2 * math.pi * g[(a + 1) % 3] / vol[(a + 1) % 3] + ph[a])
                        * torch.cos(math.pi * g[(a + 2) % 3] / vol[(a + 2) % 3]) for a in range(3)], 0)[None]
    f = g[None] + true
    grid = torch.stack([2.0 * f[:, a] / (vol[a] - 1) - 1.0 for a in range(3)][::-1], -1)
    fixed = F.grid_sample(moving, grid, mode='bilinear', padding_mode='zeros', align_corners=True)
    return moving.float(), fixed.float(), true.float()


def flow_error(flow, true):
    """mean over the voxels of |flow - true|_2, in voxels"""
    return float((flow.detach().cpu().double() - true.double()).square().sum(1).sqrt().mean())


def refine_ref(moving, fixed, dtype=torch.float64, grid_downsize=2, iters=40, lr=0.1, lam=0.05, betas=(0.9, 0.999), **_):
    """The refinement loop of infer.refine_flow restated on the CPU in `dtype` (flow = None, features = 'intensity', the
    diffusion penalty): (flow [1,nd,*vol], history [iters + 1, 2])."""
    M, Fx = moving.detach().cpu().to(dtype), fixed.detach().cpu().to(dtype)
    vol = tuple(M.shape[2:])
    nd = len(vol)
    opt = ref64.Adam(torch.zeros((M.shape[0], nd) + tuple(n // grid_downsize for n in vol)), lr, betas, 1e-8, dtype=dtype)
    up = lambda d: F.interpolate(d, size=vol, mode='trilinear' if nd == 3 else 'bilinear', align_corners=True)
    hist = torch.zeros(iters + 1, 2, dtype=dtype)
    for k in range(iters + 1):
        d = opt.p.clone().requires_grad_(k < iters)
        flow = up(d)
        sim = ssd_grid_sample(M, Fx, flow)[0]
        reg = ref64.grad_loss(flow, 'l2', dtype=dtype)
        hist[k, 0], hist[k, 1] = sim.detach(), reg.detach()
        if k < iters:
            (g,) = torch.autograd.grad(sim + lam * reg, d)
            opt.step(g)
    return flow.detach(), hist


_REFINE = {}


def refine_reference():
    """((moving, fixed, true), (flow64, history64)), computed once and shared."""
    if not _REFINE:
        inp = refine_input()
        _REFINE["r"] = (inp, refine_ref(inp[0], inp[1], **REFINE_KW))
    return _REFINE["r"]


# ------------------------------------------------------------------------------------------ CPU tier
def test_warp_ssd_symbols_in_header_exports_and_ctypes_table():
    import dfmir_amd
    from dfmir_amd import _lib, infer, losses, ops
    from tests.test_abi import header_symbols
    h = ctypes.CDLL(dfmir_amd.LIB_PATH)
    for s in ("dfmir_warp_ssd_ws_floats", "dfmir_warp_ssd_pack", "dfmir_warp_ssd_fwd", "dfmir_warp_ssd_fwd_grad",
              "dfmir_warp_ssd_bwd"):
        assert s in header_symbols() and s in _lib.exported_symbols() and hasattr(h, s), s
    lib = dfmir_amd.lib()
    assert lib.dfmir_abi_version() == 14
    assert lib.dfmir_warp_ssd_ws_floats(3, 1, 12, 16, 16, 16) == 4 * 16      # two doubles per 256 voxels
    assert lib.dfmir_warp_ssd_ws_floats(2, 2, 4, 999, 3, 3) == 4 * 2 * 1     # nd == 2: D is not read
    for bad in ((1, 1, 4, 8, 8, 8), (3, 0, 4, 8, 8, 8), (3, 1, 0, 8, 8, 8), (3, 1, 17, 8, 8, 8), (3, 1, 4, 1, 8, 8),
                (2, 1, 4, 1, 8, 1), (3, 1, 4, 1024, 1024, 1024), (3, 1, 1, 1024, 1024, 1024)):
        assert lib.dfmir_warp_ssd_ws_floats(*bad) == -1, bad
    assert lib.dfmir_warp_ssd_fwd_grad(3, None, None, None, None, None, None, None, None, None, None, 1, 4, 8, 8, 8, None) != 0
    assert b"invalid argument" in lib.dfmir_last_error()
    for name in ("WarpSSDFn", "warp_ssd", "warp_ssd_per_sample", "pack_features", "PackedFeatures"):
        assert hasattr(ops, name), name
    for name in ("refine_flow", "register_volume", "register_pair_refined"):
        assert hasattr(infer, name), name
    crit = losses.WarpedSSD_Loss(dim=2, loss_mult=0.5)
    assert crit.name == 'warped_ssd' and crit.loss_mult == 0.5 and crit.dim == 2
    with pytest.raises(ValueError, match="dim"):
        losses.WarpedSSD_Loss(dim=4)
    with pytest.raises(ValueError, match="3-D field"):
        crit(torch.zeros(1, 1, 4, 4, 4), torch.zeros(1, 1, 4, 4, 4), torch.zeros(1, 3, 4, 4, 4))
    assert inspect.signature(ops.adam_step).parameters["bump"].default is True


def test_warp_ssd_argument_checks_raise_before_the_device_is_asked_for():
    from dfmir_amd import ops
    from dfmir_amd._lib import DfmirHipError
    z = torch.zeros
    for fn in (ops.warp_ssd, ops.warp_ssd_per_sample):
        with pytest.raises(ValueError, match=r"\[B,C,H,W\] or \[B,C,D,H,W\]"):
            fn(z(2, 4, 8), z(2, 4, 8), z(2, 1, 8))                                  # bad rank
        with pytest.raises(ValueError, match="1 to 16 channels, got 0"):
            fn(z(2, 0, 8, 8), z(2, 0, 8, 8), z(2, 2, 8, 8))
        with pytest.raises(ValueError, match="1 to 16 channels, got 17"):
            fn(z(2, 17, 8, 8), z(2, 17, 8, 8), z(2, 2, 8, 8))
        with pytest.raises(ValueError, match="differ in shape"):
            fn(z(2, 4, 8, 8), z(2, 4, 8, 9), z(2, 2, 8, 8))
        with pytest.raises(ValueError, match="flow of"):
            fn(z(2, 4, 8, 8), z(2, 4, 8, 8), z(2, 3, 8, 8))                         # a 2-D pair with a 3-channel flow
        with pytest.raises(ValueError, match="flow of"):
            fn(z(2, 4, 6, 8, 8), z(2, 4, 6, 8, 8), z(2, 3, 6, 8, 9))
        with pytest.raises(ValueError, match="fp32"):
            fn(z(2, 4, 8, 8).double(), z(2, 4, 8, 8).double(), z(2, 2, 8, 8))
        with pytest.raises(ValueError, match="fp32"):
            fn(z(2, 4, 8, 8), z(2, 4, 8, 8), z(2, 2, 8, 8).double())
        with pytest.raises(ValueError, match="extent >= 2"):
            fn(z(2, 4, 1, 8), z(2, 4, 1, 8), z(2, 2, 1, 8))
        with pytest.raises(ValueError, match="does not broadcast"):
            fn(z(2, 4, 8, 8), z(2, 4, 8, 8), z(2, 2, 8, 8), mask=z(2, 1, 8, 7))
        with pytest.raises(ValueError, match="2\\^31"):
            fn(z(1, 16, 1, 1, 1).expand(1, 16, 512, 512, 512), z(1, 16, 1, 1, 1).expand(1, 16, 512, 512, 512),
               z(1, 3, 1, 1, 1).expand(1, 3, 512, 512, 512))
        for which in range(3):                      # no gradient to the features or the mask: refused, never dropped
            args = [z(2, 4, 8, 8), z(2, 4, 8, 8), z(2, 1, 8, 8)]
            args[which].requires_grad_()
            with pytest.raises(ValueError, match="requires grad"):
                fn(args[0], args[1], z(2, 2, 8, 8), mask=args[2])
        with pytest.raises(DfmirHipError, match="no CPU fallback"):                 # a good call, but on the CPU
            fn(z(2, 4, 8, 8), z(2, 4, 8, 8), z(2, 2, 8, 8), mask=z(2, 1, 8, 8))
    with pytest.raises(ValueError, match=r"\[B,C,H,W\] or \[B,C,D,H,W\]"):
        ops.pack_features(z(4, 8, 8))
    with pytest.raises(ValueError, match="got 0"):
        ops.pack_features(z(1, 0, 8, 8))
    with pytest.raises(ValueError, match="got 17"):
        ops.pack_features(z(1, 17, 8, 8))
    with pytest.raises(ValueError, match="fp32"):
        ops.pack_features(z(1, 4, 8, 8).half())
    with pytest.raises(ValueError, match="requires grad"):
        ops.pack_features(z(1, 4, 8, 8).requires_grad_())
    with pytest.raises(DfmirHipError, match="no CPU fallback"):
        ops.pack_features(z(1, 4, 8, 8))
    bad = ops.PackedFeatures(z(1, 8, 8, 8), z(1, 4, 8, 8), (1, 4, 8, 8))            # Cp = 8 for C = 4: not pack_features'
    with pytest.raises(ValueError, match="not a handle"):
        ops.warp_ssd(bad, z(1, 4, 8, 8), z(1, 2, 8, 8))


def test_refine_flow_argument_checks():
    from dfmir_amd import infer
    z = torch.zeros
    kw = dict(lam=0.1, lr=0.1)
    with pytest.raises(ValueError, match="coarse grid"):
        infer.refine_flow(z(1, 1, 3, 8, 8), z(1, 1, 3, 8, 8), **kw)                  # 3 // 2 = 1
    with pytest.raises(ValueError, match="coarse grid"):
        infer.refine_flow(z(1, 1, 8, 8), z(1, 1, 8, 8), grid_downsize=8, **kw)
    with pytest.raises(ValueError, match="one shape"):
        infer.refine_flow(z(1, 1, 8, 8), z(1, 1, 8, 9), **kw)
    with pytest.raises(ValueError, match="one shape"):
        infer.refine_flow(z(1, 8, 8), z(1, 8, 8), **kw)
    with pytest.raises(ValueError, match="flow must be"):
        infer.refine_flow(z(1, 1, 8, 8), z(1, 1, 8, 8), z(1, 3, 8, 8), **kw)
    with pytest.raises(ValueError, match="features must be"):
        infer.refine_flow(z(1, 1, 8, 8), z(1, 1, 8, 8), features='ncc', **kw)
    with pytest.raises(ValueError, match="feature tensors"):
        infer.refine_flow(z(1, 1, 8, 8), z(1, 1, 8, 8), features=(z(1, 4, 8, 8), z(1, 4, 8, 9)), **kw)
    with pytest.raises(ValueError, match="regularizer"):
        infer.refine_flow(z(1, 1, 8, 8), z(1, 1, 8, 8), regularizer='tv', **kw)
    with pytest.raises(ValueError, match="iters"):
        infer.refine_flow(z(1, 1, 8, 8), z(1, 1, 8, 8), iters=-1, **kw)
    with pytest.raises(TypeError):
        infer.refine_flow(z(1, 1, 8, 8), z(1, 1, 8, 8))                              # lam and lr have no default
    with pytest.raises(ValueError, match="refine must be"):
        infer.register_volume(None, {}, refine=0.1)
    ps = inspect.signature(infer.refine_flow).parameters
    assert [n for n, p in ps.items() if p.kind == p.POSITIONAL_OR_KEYWORD] == ["moving", "fixed", "flow"]
    assert ps["grid_downsize"].default == 2 and ps["iters"].default == 50 and ps["betas"].default == (0.9, 0.999)
    assert ps["features"].default == 'mind' and ps["regularizer"].default == 'diffusion'


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_closed_form_equals_autograd_through_grid_sample(shape, mask):
    """float64, lattice family (fractional parts in [0.05, 0.95]): the closed-form value and gradient equal grid_sample's
    value and autograd's gradient to 1e-12 (relative to the largest entry)."""
    M, Fx, phi, m = (None if t is None else t.double() for t in inputs(shape, "lattice", mask))
    p = phi.clone().requires_grad_()
    loss, per = ssd_grid_sample(M, Fx, p, m)
    (g,) = torch.autograd.grad(loss, p)
    l2, per2, d2 = ssd_closed_form(M, Fx, phi, m)
    assert abs(float(loss.detach()) - float(l2)) <= 1e-12 * max(abs(float(loss.detach())), 1e-300)
    assert float((per - per2).abs().max()) <= 1e-12 * max(float(per.abs().max()), 1e-300)
    if mask == "zero":
        assert float(loss.detach()) == 0.0 and not g.any() and not d2.any()
    else:
        assert float((g - d2).abs().max()) <= 1e-12 * float(g.abs().max())
        frac = (phi - torch.floor(phi))
        assert 0.05 - 1e-6 <= float(frac.min()) and float(frac.max()) <= 0.95 + 1e-6
        f = _grid(shape[2:], torch.float64)[None] + phi
        for a, n in enumerate(shape[2:]):            # samples leave the volume through both faces of every axis
            assert float(f[:, a].min()) < -1.0 and float(f[:, a].max()) > n


def test_refinement_loop_restatement_reduces_similarity_and_flow_error():
    """The float64 loop on the blob pair: the similarity falls by more than a factor of 10 (7.26e-3 -> 6.47e-5) and the mean
    flow error against the true field falls (1.220 -> 1.092 voxels: the blobs leave flat regions where the field cannot be
    observed); profiles/refine_margins.txt records the figures, in fp64 and in fp32 (0.3 % apart in the final similarity)."""
    (moving, fixed, true), (flow, hist) = refine_reference()
    assert tuple(moving.shape) == (1, 1) + REFINE_VOL and abs(float(true.abs().max()) - 1.5) < 0.1
    before, after = flow_error(torch.zeros_like(true), true), flow_error(flow, true)
    print("similarity %.4e -> %.4e, flow error %.4f -> %.4f" % (float(hist[0, 0]), float(hist[-1, 0]), before, after))
    assert float(hist[0, 1]) == 0.0
    assert float(hist[-1, 0]) < 0.1 * float(hist[0, 0])
    assert after < 0.95 * before


# ------------------------------------------------------------------------------------------ GPU tier
@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_warp_ssd_matches_fp64(shape, family, mask, path):
    inp, ref = reference(shape, family, mask)
    got = _gpu(*inp, path=path)
    if mask == "zero":                                   # decided on the device: exactly 0, gradient included
        assert float(got[0]) == 0.0 and not got[1].any() and not got[2].any()
        return
    _check(got, ref, family, "%s %s %s" % (_id(shape), mask, path))


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=_id)
def test_warp_ssd_gout_scales_the_gradient(shape, path):
    inp, ref = reference(shape, "lattice", "partial")
    got = _gpu(*inp, path=path, gout=-2.5)
    _check(got, (ref[0], ref[1], -2.5 * ref[2]), "lattice", "%s gout -2.5 %s" % (_id(shape), path))


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_warp_ssd_agrees_with_warp_then_mse(shape, path):
    """The fused op against the composition it replaces, ops.mse_loss(ops.warp(M, phi), F), value and dflow."""
    from dfmir_amd import ops
    M, Fx, phi, _ = inputs(shape, "lattice")
    got = _gpu(M, Fx, phi, None, path=path)
    p = phi.to(DEV).requires_grad_()
    loss = ops.mse_loss(Fx.to(DEV), ops.warp(M.to(DEV), p))
    loss.backward()
    torch.cuda.synchronize()
    per = got[1]                                         # (the composition has no per-sample form)
    _check(got, (loss.detach().cpu(), per, p.grad.cpu()), "lattice", "%s vs warp+mse %s" % (_id(shape), path))


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_warp_ssd_is_bit_reproducible(path):
    for shape, mask in ((SHAPES[2], "partial"), (SHAPES[0], "none")):
        inp = inputs(shape, "lattice", mask)
        a, b = _gpu(*inp, path=path), _gpu(*inp, path=path)
        for x, y in zip(a, b):
            assert torch.equal(x, y)


@pytest.mark.gpu
def test_warp_ssd_refuses_gradients_to_features_and_mask_and_packs_per_call():
    from dfmir_amd import ops
    M, Fx, phi, m = (t.to(DEV) for t in inputs(SHAPES[0], "lattice", "partial"))
    for which in range(3):
        args = [M.clone(), Fx.clone(), m.clone()]
        args[which].requires_grad_()
        with pytest.raises(ValueError, match="requires grad"):
            ops.warp_ssd(args[0], args[1], phi, args[2])
    h = ops.pack_features(M)
    assert tuple(h.packed.shape) == (2, 9, 13, 4) and h.shape == tuple(M.shape)
    assert torch.equal(h.packed.permute(0, 3, 1, 2), M)
    h5 = ops.pack_features(inputs(SHAPES[4], "lattice")[0].to(DEV))
    assert tuple(h5.packed.shape) == (1, 2, 6, 8, 8) and not h5.packed[..., 5:].any()
    assert torch.equal(ops.warp_ssd(M, Fx, phi, m), ops.warp_ssd(h, Fx, phi, m))      # a tensor is packed per call
    with torch.no_grad():
        assert torch.equal(ops.warp_ssd(h, Fx, phi, m), ops.warp_ssd(h, Fx, phi.clone().requires_grad_(), m).detach())
    from dfmir_amd.losses import WarpedSSD_Loss
    assert torch.equal(WarpedSSD_Loss(dim=2, loss_mult=2.0)(h, Fx, phi, mask=m), 2.0 * ops.warp_ssd(h, Fx, phi, m))


@pytest.mark.gpu
def test_refine_flow_follows_the_fp64_loop():
    from dfmir_amd import infer, ops
    (moving, fixed, true), (flow64, hist64) = refine_reference()
    mv, fx = moving.to(DEV), fixed.to(DEV)
    out = infer.refine_flow(mv, fx, features='intensity', **REFINE_KW)
    hist = out['history'].cpu().double()
    zero = torch.zeros(1, 3, *REFINE_VOL, device=DEV)
    assert tuple(hist.shape) == (41, 2) and out['history'].is_cuda
    assert torch.equal(out['history'][0, 0], ops.warp_ssd(mv, fx, zero))           # iteration 0 evaluates flow0 itself
    assert torch.equal(out['history'][40, 0], ops.warp_ssd(mv, fx, out['flow']))
    assert torch.equal(out['warped'], ops.warp(mv, out['flow']))
    before, after = flow_error(zero, true), flow_error(out['flow'], true)
    gap = abs(float(hist[40, 0]) - float(hist64[40, 0])) / float(hist64[40, 0])
    print("similarity %.6e -> %.6e (fp64 loop %.6e -> %.6e, relative gap %.3e, bound %.1e); flow error %.4f -> %.4f"
          % (float(hist[0, 0]), float(hist[40, 0]), float(hist64[0, 0]), float(hist64[40, 0]), gap,
             FACTOR * REFINE_FP32_GAP, before, after))
    assert float(hist[40, 0]) < float(hist[0, 0])
    assert gap <= FACTOR * REFINE_FP32_GAP
    assert after < before


@pytest.mark.gpu
def test_refine_flow_options():
    from dfmir_amd import infer, ops
    moving, fixed, _ = refine_input()
    mv, fx = moving.to(DEV), fixed.to(DEV)
    flow0 = ((C.rand(77, 1, 3, *REFINE_VOL) * 2 - 1) * 0.7).to(DEV)
    out = infer.refine_flow(mv, fx, flow0, features='intensity', iters=0, lam=0.05, lr=0.1)
    assert torch.equal(out['flow'], flow0) and out['flow'].data_ptr() != flow0.data_ptr()      # bit for bit, a copy
    assert tuple(out['history'].shape) == (1, 2) and torch.equal(out['history'][0, 0], ops.warp_ssd(mv, fx, flow0))
    out = infer.refine_flow(mv, fx, flow0, features='intensity', iters=2, lam=0.05, lr=0.1)
    assert torch.equal(out['history'][0, 0], ops.warp_ssd(mv, fx, flow0))
    # MIND features, 3-D (12 channels) and 2-D at 32 x 32 (4 channels); the bending penalty; user features; a mask
    out = infer.refine_flow(mv, fx, iters=3, lam=0.05, lr=0.1, regularizer='bending', spacing=(2.0, 1.0, 1.0))
    assert bool(torch.isfinite(out['history']).all()) and bool(torch.isfinite(out['flow']).all())
    a2, b2 = mv[:, :, 8, :16, :16].repeat(1, 1, 2, 2).contiguous(), fx[:, :, 8, :16, :16].repeat(1, 1, 2, 2).contiguous()
    out = infer.refine_flow(a2, b2, features='mind', iters=3, lam=0.05, lr=0.1)
    assert tuple(out['flow'].shape) == (1, 2, 32, 32) and tuple(out['warped'].shape) == (1, 1, 32, 32)
    assert bool(torch.isfinite(out['history']).all()) and bool(torch.isfinite(out['flow']).all())
    feats = (torch.cat([mv, mv * mv], 1), torch.cat([fx, fx * fx], 1))
    mask = (C.rand(78, 1, 1, *REFINE_VOL) > 0.3).float().to(DEV)
    out = infer.refine_flow(mv, fx, features=feats, mask=mask, iters=3, lam=0.05, lr=0.1)
    assert torch.equal(out['history'][0, 0], ops.warp_ssd(feats[0], feats[1], torch.zeros_like(flow0), mask))
    assert bool(torch.isfinite(out['history']).all()) and bool(torch.isfinite(out['flow']).all())


@pytest.mark.gpu
def test_refine_flow_leaves_the_weights_epoch_alone():
    """A flow is no conv weight: the loop's Adam steps must not invalidate packed weights (ops.adam_step(bump=False))."""
    from dfmir_amd import infer, ops
    moving, fixed, _ = refine_input()
    calls = []
    orig = ops.bump_weights_epoch
    ops.bump_weights_epoch = lambda: calls.append(1)
    try:
        infer.refine_flow(moving.to(DEV), fixed.to(DEV), features='intensity', iters=2, lam=0.05, lr=0.1)
        assert not calls
        p = torch.zeros(8, device=DEV)
        ops.adam_step(p, torch.ones(8, device=DEV), torch.zeros(8, device=DEV), torch.zeros(8, device=DEV), 0.1, 0.9, 0.999,
                      1e-8, 1)
        assert calls == [1]                              # the default keeps today's behaviour
    finally:
        ops.bump_weights_epoch = orig


@pytest.mark.gpu
def test_register_volume_with_and_without_refine():
    from dfmir_amd import infer
    from dfmir_amd.registration3d import Registration3DModel
    torch.manual_seed(5)
    model = Registration3DModel((16, 16, 16), device=DEV)
    moving, fixed, _ = refine_input()
    data = {"A": moving[:, :, :, :16, :16].contiguous(), "B": fixed[:, :, :, :16, :16].contiguous()}
    out = infer.register_volume(model, data)
    assert sorted(out) == ["flow", "warped_A"]
    with torch.no_grad():
        want = model.netR(model.real_A, model.real_B, registration=True)
    assert torch.equal(out["flow"], want[1]) and torch.equal(out["warped_A"], want[0])
    ref = infer.register_volume(model, data, refine=dict(features='intensity', iters=3, lam=0.05, lr=0.1))
    assert sorted(ref) == ["flow", "history", "refined_A", "refined_flow", "warped_A"]
    assert torch.equal(ref["flow"], out["flow"]) and tuple(ref["history"].shape) == (4, 2)
    assert tuple(ref["refined_flow"].shape) == (1, 3, 16, 16, 16) and tuple(ref["refined_A"].shape) == (1, 1, 16, 16, 16)
    assert bool(torch.isfinite(ref["history"]).all()) and bool(torch.isfinite(ref["refined_flow"]).all())


@pytest.mark.gpu
def test_register_pair_keys_are_unchanged_and_the_refined_form_adds_three():
    from dfmir_amd import infer, ops

    class _Stub(object):                     # the slice of REGISTRATIONModel that register_pair touches
        def __init__(self, flow):
            self._flow = flow
            self.netG = lambda x: x
            self.netR = lambda a, b, registration=False: (ops.warp(a, self._flow), self._flow)

        def set_input(self, data):
            self.real_A, self.real_B = data["A"].to(DEV), data["B"].to(DEV)

        def forward(self):
            self.fake_B = self.idt_B = self.real_A

    moving, fixed, _ = refine_input()
    data = {"A": moving[:, :, 8].contiguous(), "B": fixed[:, :, 8].contiguous()}
    flow = ((C.rand(79, 1, 2, 20, 24) * 2 - 1) * 0.5).to(DEV)
    plain = infer.register_pair(_Stub(flow), data)
    assert sorted(plain) == ["fake_B", "flow", "idt_B", "translated_B", "warped_A"]
    out = infer.register_pair_refined(_Stub(flow), data, dict(features='intensity', iters=2, lam=0.05, lr=0.1))
    assert sorted(out) == sorted(list(plain) + ["refined_flow", "refined_A", "history"])
    for k in plain:
        assert torch.equal(out[k], plain[k]), k
    assert tuple(out["refined_flow"].shape) == (1, 2, 20, 24) and tuple(out["history"].shape) == (3, 2)
