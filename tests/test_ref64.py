"""CPU: the float64 references of tests/ref64.py against the fp32 oracle (oracle/dfmir_oracle.py, the project's restatement
of the reference) and plain torch, values and autograd gradients, on small seeded inputs -- this is where the references
the GPU tests trust are themselves verified.  Agreement is to fp32 round-off of the ORACLE: 2e-5 on scalars, 1e-4 of the
maximum on gradients, 1e-3 on the NCC gradient (the oracle's conv over win^nd taps in fp32).

The warp, VecInt and resize restatements are compared with the oracle's functions evaluated in float64 (1e-11: the oracle's
round trip through normalised coordinates), with the documented adjoint formulas and with F.interpolate; the two host-only
size functions that choose the warp and resize backward forms are checked at their boundaries through ctypes.

conv_weight_grad / conv_bias_grad (the tap-by-tap contraction, both evaluation orders, the up-cat operand) are compared with
float64 autograd through F.conv2d / F.conv3d.

The tests after those evaluate, with the oracle alone, the ill-conditioned inputs of tests/test_gpu_pointwise_fp64.py: the bound
`max(bar, 2 x oracle error)` they lead to must stay within 10 x the bar, else the input tests nothing."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import dfmir_oracle as O
from tests import ref64 as R
from tests.golden import common as C


def rel(got, ref):
    got, ref = got.detach().double(), ref.detach().double()
    assert got.shape == ref.shape
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def val_and_grads(fn, *xs, dtype=None):
    xs = [(x.to(dtype) if dtype else x.clone()).requires_grad_() for x in xs]
    l = fn(*xs)
    (l * 3.0).backward()
    return [l] + [x.grad for x in xs]


@pytest.mark.parametrize("n", [1, 37, 1000])
def test_masked_l1(n):
    a, b = C.rand(11, n) * 2 - 1, C.rand(12, n) * 2 - 1
    a[::3] = -1.0
    mask = (a > -0.95) | (b > -0.95)
    ref = val_and_grads(lambda x, y: O.masked_l1(x, y, mask.float()), a, b)
    for got in (val_and_grads(lambda x, y: R.masked_l1(x, y, thr=-0.95), a, b, dtype=torch.float64),
                val_and_grads(lambda x, y: R.masked_l1(x, y, mask=mask), a, b, dtype=torch.float64)):
        assert rel(got[0], ref[0]) <= 2e-5
        assert rel(got[1], ref[1]) <= 1e-4 and rel(got[2], ref[2]) <= 1e-4
    assert float(R.masked_l1(a, b, mask=torch.zeros(n))) == 0.0 == float(O.masked_l1(a, b, torch.zeros(n)))
    assert rel(R.masked_l1(a, b), O.masked_l1(a, b, None)) <= 2e-5


@pytest.mark.parametrize("shape", [(2, 2, 18, 22), (1, 3, 7, 9, 11)], ids=["2d", "3d"])
@pytest.mark.parametrize("penalty", ["l2", "l1"])
def test_grad_loss(shape, penalty):
    f = C.randn(13, *shape) * 1.5
    mask = (C.rand(14, shape[0], 1, *shape[2:]) > 0.3).float()
    for kw in (dict(), dict(mask=mask, loss_mult=2.5)):
        ref = val_and_grads(lambda x: O.grad_loss(x, penalty, **kw), f)
        got = val_and_grads(lambda x: R.grad_loss(x, penalty, **kw), f, dtype=torch.float64)
        assert rel(got[0], ref[0]) <= 2e-5 and rel(got[1], ref[1]) <= 1e-4
    if len(shape) == 4 and penalty == "l2":
        assert rel(R.grad_loss(f, "l2"), O.smoothing_loss(f)) <= 2e-5
    # an axis of extent 1: NaN like torch; skip_empty: the axis contributes 0 and the divisor stays the number of axes
    g = f[..., :1]
    assert bool(torch.isnan(R.grad_loss(g, penalty))) and bool(torch.isnan(O.grad_loss(g, penalty)))
    nd = len(shape) - 2
    assert rel(R.grad_loss(g, penalty, skip_empty=True) * nd, R.grad_loss(g[..., 0], penalty) * (nd - 1)) <= 1e-12


@pytest.mark.parametrize("shape,win", [((2, 1, 24, 28), 9), ((1, 1, 20, 13), 7), ((1, 1, 5, 30), 9), ((1, 1, 12, 14, 16), 9),
                                       ((2, 1, 7, 10, 11), 5), ((1, 1, 6, 9, 8), 3), ((1, 1, 1, 12, 14), 9)])
def test_ncc(shape, win):
    I = C.rand(15, *shape)
    J = 0.6 * I + 0.4 * C.rand(16, *shape)
    mask = (C.rand(17, *shape) > 0.35).float()
    cc = O.ncc_map(I, J, win)
    for method in ("cumsum", "shift"):
        assert rel(R.ncc_map(I, J, win, method=method), cc) <= 1e-4
    assert rel(R.ncc_map(I, J, win, dtype=torch.float32), cc) <= 1e-4          # the plain fp32 restatement
    assert rel(R.box_sum(I.double(), win, range(2, I.dim()), "cumsum"), R.box_sum(I.double(), win, range(2, I.dim()), "shift")) <= 1e-13
    for kw, ofn in ((dict(), lambda x: O.ncc_loss(x, J, win)),
                    (dict(mask=mask), lambda x: O.ncc_loss(x, J, win, mask=mask)),
                    (dict(reduction="neg_mean"), lambda x: O.vxm_ncc_loss(J, x, win))):
        ref = val_and_grads(ofn, I)
        got = val_and_grads(lambda x: R.ncc_loss(x, J, win, **kw), I, dtype=torch.float64)
        assert rel(got[0], ref[0]) <= 2e-5 and rel(got[1], ref[1]) <= 1e-3, kw
        g32 = val_and_grads(lambda x: R.ncc_loss(x, J, win, dtype=torch.float32, **kw), I)
        assert rel(g32[0], ref[0]) <= 2e-5 and rel(g32[1], ref[1]) <= 1e-3, kw
    assert rel(R.vxm_ncc_loss(J, I, win), O.vxm_ncc_loss(J, I, win)) <= 2e-5
    assert float(R.ncc_loss(I, J, win, mask=torch.zeros(shape))) == 0.0 == float(O.ncc_loss(I, J, win, mask=torch.zeros(shape)))


@pytest.mark.parametrize("shape,relu,res", [((2, 3, 5, 5), False, False), ((2, 3, 9, 11), True, True), ((1, 2, 16, 16), True, False),
                                            ((1, 2, 16, 16), False, True)])
def test_instance_norm(shape, relu, res):
    x, r, cot = C.randn(18, *shape) * 2 + 0.7, (C.randn(19, *shape) if res else None), C.randn(20, *shape)

    def torch_in(x_, r_=None):
        y = F.instance_norm(x_, eps=1e-5)
        y = F.relu(y) if relu else y
        return ((y + r_ if res else y) * cot.to(x_.dtype)).sum()

    def ref_in(x_, r_=None):
        return (R.instance_norm(x_, r_, relu, 1e-5)[0] * cot.double()).sum()
    args = (x, r) if res else (x,)
    ref, got = val_and_grads(torch_in, *args), val_and_grads(ref_in, *args, dtype=torch.float64)
    for g, o in zip(got[1:], ref[1:]):
        assert rel(g, o) <= 1e-4
    y, mean, rstd = R.instance_norm(x, r, relu)
    yo = F.relu(F.instance_norm(x, eps=1e-5)) if relu else F.instance_norm(x, eps=1e-5)
    assert rel(y, yo + r if res else yo) <= 2e-5
    xf = x.double().reshape(mean.numel(), -1)
    assert rel(mean, xf.mean(1)) <= 1e-12 and rel(rstd, 1 / torch.sqrt(xf.var(1, unbiased=False) + 1e-5)) <= 1e-12
    # the Downsample of the fused kernel's reference against the oracle's module
    assert rel(R.blur_down(y), O.BlurDown(shape[1])(y.float())) <= 2e-5 or shape[2] < 3


@pytest.mark.parametrize("betas", [(0.5, 0.999), (0.9, 0.999)])
def test_adam(betas):
    p0 = C.randn(21, 1001)
    ref = R.Adam(p0, 2e-4, betas)
    p64, p32 = p0.double().requires_grad_(), p0.clone().requires_grad_()
    o64, o32 = torch.optim.Adam([p64], lr=2e-4, betas=betas), torch.optim.Adam([p32], lr=2e-4, betas=betas)
    for t in range(12):
        g = C.randn(30 + t, 1001) * (0.1 + t)
        ref.step(g)
        p64.grad, p32.grad = g.double(), g.clone()
        o64.step(); o32.step()
    assert rel(ref.p - p0.double(), p64 - p0.double()) <= 1e-12          # torch's own Adam in float64: the same rule
    assert rel(ref.m, o64.state[p64]['exp_avg']) <= 1e-12 and rel(ref.v, o64.state[p64]['exp_avg_sq']) <= 1e-12
    assert rel(ref.p - p0.double(), p32 - p0) <= 1e-3                    # fp32: p ~ 3 moves by ~2e-3, 1 ulp(p) = 1e-4 of that
    assert rel(ref.m, o32.state[p32]['exp_avg']) <= 2e-5 and rel(ref.v, o32.state[p32]['exp_avg_sq']) <= 2e-5


# ------------------------------------------------------------------------------------------------------------------------
# the ill-conditioned inputs of the GPU module, with the oracle alone
def _gpu_module():
    from tests import test_gpu_pointwise_fp64 as G
    return G


def _phantom_cases():
    return [c for c in _gpu_module().NCC_CASES if c[3] != "noise"]


@pytest.mark.parametrize("case", _phantom_cases(), ids=[c[0] for c in _phantom_cases()])
def test_phantom_ncc_inputs_are_testable(case):
    G = _gpu_module()
    I, J, mask = G.ncc_inputs(case)
    fg = float(((I - I.flatten()[0]).abs() > 1e-6).float().mean())
    if min(case[1][2:]) > 4:
        assert 0.3 <= fg <= 0.5, "phantom foreground %.2f, wanted about 40 %%" % fg
    Ir = I.double().requires_grad_()
    lr = R.ncc_loss(Ir, J, case[2], 1e-5, mask, case[5])
    (lr * G.NCC_UPSTREAM).backward()
    lo, dIo = G.ncc_fp32_oracle(case, I, J, mask)
    assert G.oracle_bound(lr, lo, G.BAR)[0] <= 10 * G.BAR
    assert G.oracle_bound(Ir.grad, dIo, G.BAR_GRAD)[0] <= 10 * G.BAR_GRAD
    assert float(lr.detach()) < -0.05                                            # a real similarity, not a vanishing one


@pytest.mark.parametrize("family", ["constant", "offset1e3", "one-constant-channel"])
@pytest.mark.parametrize("plane", [(5, 5), (9, 11), (100, 100), (64, 64), (128, 128), (256, 256)], ids=lambda p: "%dx%d" % p)
def test_hard_instance_norm_inputs_are_testable(plane, family):
    G = _gpu_module()
    H, W = plane
    x, cot = G.in_input(family, H, W), C.randn(643, 2, 3, H, W)
    for relu, res in ((False, True), (True, False)):
        ref = G.in_reference(x, C.randn(642, *x.shape) if res else None, relu, cot)
        assert G.oracle_bound(ref["y"], ref["y32"], G.BAR, floor=G.in_floor(family))[0] <= 10 * G.BAR
        where = G.in_dx_where(family, relu, ref)
        if where is None or bool(where.any()):
            assert G.oracle_bound(ref["dx"], ref["dx32"], G.BAR_IN_DX, where=where)[0] <= 10 * G.BAR_IN_DX
    if H in (128, 256):
        ref = G.in_reference(G.in_input(family, H, H, seed=645), None, True, C.randn(646, 2, 3, H // 2, H // 2), down=True)
        assert G.oracle_bound(ref["y"], ref["y32"], G.BAR, floor=G.in_floor(family))[0] <= 10 * G.BAR
        where = G.in_dx_where(family, True, ref)
        if bool(where.any()):
            assert G.oracle_bound(ref["dx"], ref["dx32"], G.BAR_IN_DX, where=where)[0] <= 10 * G.BAR_IN_DX


def test_full_size_reduction_inputs_are_testable():
    G = _gpu_module()
    a, b = C.image_pair(631, 16, 256, 256)
    m = R.threshold_mask(a, b, -0.95).float()
    assert G.oracle_bound(R.masked_l1(a, b, thr=-0.95), O.masked_l1(a, b, m), G.BAR)[0] <= 10 * G.BAR
    x = C.randn(664, (1 << 20) + 3) + 1e3
    assert G.oracle_bound(x.double().mean(), x.mean(), G.BAR)[0] <= 10 * G.BAR


def test_ncc_volume_flag_matches_the_header():
    """ops.NCC_VOLUME mirrors DFMIR_NCC_VOLUME of include/dfmir_hip.h."""
    import os
    import re
    from dfmir_amd import ops
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dfmir_hip.h")).read()
    assert int(re.search(r"#define\s+DFMIR_NCC_VOLUME\s+(\d+)", text).group(1)) == ops.NCC_VOLUME


# ------------------------------------------------------------------------------------------------------------------------
# warp, VecInt, resize
WARP_CPU_SHAPES = [(2, 3, 5, 6, 7), (1, 1, 3, 4, 9), (2, 2, 9, 11), (1, 4, 6, 7)]


def _warp_module():
    from tests import warp_cases as W
    return W


def warp_adjoint(src, flow, g):
    """(d(src), d(flow)) of sum(g * warp(src, flow)) by the documented formulas: d(src) = the interpolation's transpose applied to
    g; d(flow)_a = sum over channels and corners of g * (+-1 along a) * the other axes' weights * the corner's value, corners
    outside the volume as zeros."""
    from tests.test_invcons import _corners
    B, Cn = src.shape[:2]
    nd = flow.shape[1]
    S = math.prod(src.shape[2:])
    sf = src.reshape(B, Cn, S)
    dsrc = torch.zeros(B, Cn, S, dtype=src.dtype)
    dflow = torch.zeros_like(flow)
    for flat, valid, w, bits in _corners(flow):
        idx = flat.reshape(B, 1, S).expand(B, Cn, S)
        ok = valid.to(src.dtype)
        val = torch.gather(sf, 2, idx).reshape(src.shape) * ok[:, None]
        for a in range(nd):
            others = torch.ones_like(w[:, 0])
            for b in range(nd):
                if b != a:
                    others = others * w[:, b]
            dflow[:, a] += (1.0 if bits[a] else -1.0) * others * (g * val).sum(1)
        dsrc.scatter_add_(2, idx, (g * (w.prod(1) * ok)[:, None]).reshape(B, Cn, S))
    return dsrc.reshape(src.shape), dflow


@pytest.mark.parametrize("shape", WARP_CPU_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
@pytest.mark.parametrize("family", ["lattice", "smooth"])
def test_warp_against_the_oracle_in_float64_and_the_adjoint_formulas(shape, family):
    """d(flow) against grid_sample's on the lattice family only: elsewhere a sample point may lie so close to a cell boundary
    that the normalised-coordinate round trip takes the other cell."""
    W = _warp_module()
    src, flow, g = (t.double() for t in (W.noise(41, shape, 2.0), W.flow_field(shape, family, seed=43), W.noise(47, shape, 1.0)))
    out, dsrc, dflow = W.warp_eval(src, flow, g)
    a, b = src.clone().requires_grad_(), flow.clone().requires_grad_()
    ref = O.spatial_transform(a, b)
    (ref * g).sum().backward()
    assert ref.dtype == torch.float64 and float(out.abs().max()) > 0.0
    assert rel(out, ref) <= 1e-11 and rel(dsrc, a.grad) <= 1e-11
    if family == "lattice":
        assert rel(dflow, b.grad) <= 1e-11
    fs, ff = warp_adjoint(src, flow, g)
    assert rel(fs, dsrc) <= 1e-13 and rel(ff, dflow) <= 1e-13
    assert rel(R.warp(src, flow, add_identity=True), ref + src) <= 1e-11
    if shape[1] == len(shape) - 2:                                  # C = nd: ic_residual is this warp plus the flow
        from tests.test_invcons import ic_residual
        assert rel(ic_residual(flow, src), flow + R.warp(src, flow)) <= 1e-14
    near = W.flow_field(shape, "nearest", seed=53).double()
    assert torch.equal(R.warp(src, near, mode="nearest"), O.spatial_transform(src, near, mode="nearest"))
    assert rel(R.warp(src.float(), flow.float(), dtype=torch.float32), out) <= 1e-4      # dtype=float32: the fp32 yardstick


@pytest.mark.parametrize("shape", [(1, 3, 5, 6, 7), (2, 2, 9, 11)], ids=["3d", "2d"])
def test_vecint_against_the_oracle_in_float64(shape):
    W = _warp_module()
    g = W.noise(59, shape, 1.0).double()
    for family in ("chain", "lattice"):          # chain: seven steps behind 1 / 128; lattice: one step (d(flow) on the lattice only)
        v = W.flow_field(shape, family, seed=61).double()
        steps = 7 if family == "chain" else 1
        out, dv = W.vecint_eval(v, g, steps=steps, pre=1.0 / 2 ** steps)
        a = v.clone().requires_grad_()
        ref = O.vec_int(a, steps)
        (ref * g).sum().backward()
        assert rel(out, ref) <= 1e-11 and rel(dv, a.grad) <= 1e-11, family
    v = W.flow_field(shape, "lattice", seed=61).double()
    fs, ff = warp_adjoint(v, v, g)
    assert rel(g + fs + ff, W.vecint_eval(v, g)[1]) <= 1e-13
    assert torch.equal(R.vecint_step(v), v + R.warp(v, v))


@pytest.mark.parametrize("isp,osp", [((6, 10, 12), (12, 20, 24)), ((12, 20, 24), (6, 10, 12)), ((7, 9, 13), (3, 4, 6)), ((9, 37), (23, 50)),
                                     ((3, 5), (24, 40)), ((4, 30), (4, 1)), ((5, 1, 8), (5, 1, 16)), ((2, 2, 1), (4, 4, 8))],
                         ids=lambda sp: "x".join(str(v) for v in sp))
def test_resize_against_interpolate_and_the_oracle_in_float64(isp, osp):
    x, cot = C.randn(67, 2, 3, *isp).double(), C.randn(68, 2, 3, *osp).double()
    mode = "trilinear" if len(isp) == 3 else "bilinear"
    for mult in (0.5, 2.0, -1.5):
        got = val_and_grads(lambda t: (R.resize_linear(t, osp, mult) * cot).sum(), x)
        ref = val_and_grads(lambda t: (mult * F.interpolate(t, size=osp, mode=mode, align_corners=True) * cot).sum(), x)
        assert rel(R.resize_linear(x, osp, mult), mult * F.interpolate(x, size=osp, mode=mode, align_corners=True)) <= 1e-13
        assert rel(got[1], ref[1]) <= 1e-13
    if all(o == 2 * i for i, o in zip(isp, osp)):
        assert rel(R.resize_linear(x, osp, 2.0), O.resize_transform(x, 0.5)) <= 1e-13
    if all(i == 2 * o for i, o in zip(isp, osp)):
        assert rel(R.resize_linear(x, osp, 0.5), O.resize_transform(x, 2.0)) <= 1e-13
    assert R.resize_linear(x.float(), osp).dtype == torch.float64 and R.resize_linear(x, osp, dtype=torch.float32).dtype == torch.float32


def _own_eligible(nd, B, C_, D, H, W):
    """What dfmir_warp_bwd_own_ws_floats documents: the owner-gather backward takes a shape when W % 4 == 0, a sample's flow
    stays below 2^31 bytes, the voxel count below 2^31 and the tile count (tiles 8 x 8 x 32 / 64 x 32) below 2^30."""
    D = D if nd == 3 else 1
    ty, tz = (8, 8) if nd == 3 else (64, 1)
    tiles = -(-W // 32) * -(-H // ty) * -(-D // tz) * B
    return W % 4 == 0 and D * H * W * nd * 4 < 2 ** 31 and B * D * H * W < 2 ** 31 and tiles < 2 ** 30


def test_warp_and_resize_size_functions_at_their_boundaries():
    """No tensor is allocated: both functions are host arithmetic."""
    import dfmir_amd
    lib = dfmir_amd.lib()
    own = lib.dfmir_warp_bwd_own_ws_floats
    cases = [(3, 1, 1, 8, 8, 32), (3, 1, 1, 8, 8, 30), (3, 1, 1, 8, 8, 31), (3, 1, 1, 8, 8, 33), (3, 1, 1, 8, 8, 4), (2, 1, 2, 1, 64, 32),
             (2, 3, 2, 999, 130, 68), (2, 1, 2, 1, 9, 11), (3, 2, 5, 1, 1, 4),
             # a sample's flow at 2^31 bytes: 3-D D H W < 2^31 / 12, 2-D H W < 2^28
             (3, 1, 1, 1, 1, 178956968), (3, 1, 1, 1, 1, 178956972), (3, 1, 1, 2, 2, 44739240), (3, 1, 1, 2, 2, 44739244),
             (2, 1, 2, 1, 1, 268435452), (2, 1, 2, 1, 1, 268435456), (2, 1, 2, 1, 4096, 65532), (2, 1, 2, 1, 4096, 65536),
             # the voxel count at 2^31
             (2, 15, 2, 1, 1, 1 << 27), (2, 16, 2, 1, 1, 1 << 27), (3, 31, 3, 4, 4096, 4096), (3, 32, 3, 4, 4096, 4096),
             (2, (1 << 29) - 1, 2, 1, 1, 4), (2, 1 << 29, 2, 1, 1, 4), (3, (1 << 29) - 1, 3, 1, 1, 4), (3, 1 << 29, 3, 1, 1, 4)]
    seen = set()
    for c in cases:
        want = _own_eligible(*c)
        seen.add(want)
        assert (own(*c) > 0) == want, (c, own(*c))
        assert own(*c) >= 0
    assert seen == {True, False}
    # (a tile holds at least 4 voxels of a W % 4 == 0 volume, so below 2^31 voxels the tile count stays below 2^29: the fourth
    # condition never decides alone)
    T_, Cn = 2 * 2 * 2 * 3, 5                                        # (3, 5, 9, 9, 36): 8 ragged tiles per sample
    assert own(3, 3, Cn, 9, 9, 36) == ((8 * T_ + 2048 * T_ + 3) & ~3) + T_ * Cn * 12 * 12 * 40
    assert own(2, 1, 2, 77, 65, 36) == ((8 * 4 + 2048 * 4 + 3) & ~3) + 4 * 2 * 68 * 40          # 2-D: D is not read
    for bad in ((1, 1, 1, 8, 8, 32), (4, 1, 1, 8, 8, 32), (3, 0, 1, 8, 8, 32), (3, 1, 0, 8, 8, 32), (3, 1, 1, 0, 8, 32),
                (3, 1, 1, 8, 0, 32), (3, 1, 1, 8, 8, 0), (2, 1, 1, 8, 8, -4)):
        assert own(*bad) == -1, bad
    buf = (ctypes.c_float * 64)()                      # host memory: a refused call never dereferences it
    p = ctypes.cast(buf, ctypes.c_void_p)
    for c in ((3, 1, 1, 8, 8, 30), (3, 1, 1, 1, 1, 178956972), (2, 16, 2, 1, 1, 1 << 27)):
        nd, dims = c[0], c[1:]
        assert lib.dfmir_warp_bwd_own(nd, p, p, p, p, p, *dims, 0, 0, p, None) != 0, c
        assert b"invalid argument" in lib.dfmir_last_error()
    ws = lib.dfmir_resize_bwd_ws_floats
    assert ws(6, 5, 6, 7, 10, 12, 14) == 6 * 10 * 12 * 7 + 6 * 10 * 6 * 7             # planes Do Ho Wi + planes Do Hi Wi
    assert ws(1, 1, 1, 1, 1, 1, 1) == 2 and ws(2, 1, 4, 300, 1, 4, 1) == 2 * 4 * 300 * 2
    assert ws(3, 1024, 1024, 1024, 2048, 2048, 2048) == 3 * 2048 * 2048 * 1024 + 3 * 2048 * 1024 * 1024    # past 2^32: 64-bit
    for hole in range(7):                               # positive for every valid size, 0 for any other: ResizeFn takes
        for v in (0, -1):                               # the separable adjoint whenever the count is positive
            args = [2, 3, 4, 5, 6, 7, 8]
            args[hole] = v
            assert ws(*args) == 0, args


# ------------------------------------------------------------------------------------------------------------------------
# PatchNCE path
def _nce_module():
    from tests import test_gpu_patchnce_fp64 as G
    return G


@pytest.mark.parametrize("shape", [(37, 1), (50, 3), (20, 24), (5, 300)], ids=lambda s: "rows%d-C%d" % s)
def test_l2_normalize(shape):
    x, dy = C.randn(901, *shape), C.randn(902, *shape)
    ref = val_and_grads(lambda t: (O.l2_normalize(t) * dy).sum(), x)
    got = val_and_grads(lambda t: (R.l2_normalize(t) * dy.double()).sum(), x, dtype=torch.float64)
    assert rel(R.l2_normalize(x), O.l2_normalize(x)) <= 2e-5
    if shape[1] > 1:                                                 # (C = 1: dx is a pure cancellation, the fp32 oracle 1e-2 off)
        assert rel(got[1], ref[1]) <= 1e-4
    # the written-out gradient is autograd's wherever autograd has one, at any eps
    for eps in (1e-7, 1e-3):
        xd = x.double().requires_grad_()
        ((xd / (xd.pow(2).sum(1, keepdim=True).sqrt() + eps)) * dy.double()).sum().backward()
        # (C = 1: two terms of size |dy| / n cancel to |dy| eps / n^2, a factor n / eps ~ 1e7 that float64 round-off rides on)
        assert rel(R.l2_normalize_grad(x, dy, eps), xd.grad) <= (1e-12 if shape[1] > 1 else 1e-8)
    # a zero row: y = 0, dx = dy / eps (defined, where autograd through sqrt has NaN)
    x[2] = 0.0
    xd = x.double().requires_grad_()
    y = R.l2_normalize(xd, 1e-3)
    (y * dy.double()).sum().backward()
    assert bool((y[2] == 0).all()) and torch.equal(xd.grad[2], dy[2].double() / 1e-3) and bool(torch.isfinite(xd.grad).all())
    assert R.l2_normalize(x, dtype=torch.float32).dtype == torch.float32


@pytest.mark.parametrize("cfg", [(32, 24, 2, 0.07), (16, 3, 3, 1.0), (48, 64, 1, 0.07), (16, 1, 2, 0.01)],
                         ids=lambda c: "R%d-C%d-G%d-T%g" % c)
def test_patchnce_rows(cfg):
    Rr, Cn, G, T = cfg
    q, k = O.l2_normalize(C.randn(903, Rr * G, Cn)), O.l2_normalize(C.randn(904, Rr * G, Cn))
    cot = C.randn(905, Rr * G)
    ref = val_and_grads(lambda t: (O.patchnce_loss(t, k, G, T) * cot).sum(), q)
    got = val_and_grads(lambda t: (R.patchnce_rows(t, k, G, T) * cot.double()).sum(), q, dtype=torch.float64)
    assert rel(R.patchnce_rows(q, k, G, T), O.patchnce_loss(q, k, G, T)) <= 2e-5
    assert rel(got[1], ref[1]) <= 1e-4
    assert rel(R.patchnce_rows(q, k, 1, T), O.patchnce_loss(q, k, G, T, all_negatives=True)) <= 2e-5
    # the oracle itself evaluated in float64: the same function to round-off
    assert rel(R.patchnce_rows(q, k, G, T), O.patchnce_loss(q.double(), k.double(), G, T)) <= 1e-12
    kd = k.double().requires_grad_()                                  # no gradient reaches k
    assert torch.autograd.grad(R.patchnce_rows(q.double().requires_grad_(), kd, G, T).sum(), kd, allow_unused=True)[0] is None


def test_patch_gather_and_head_against_the_patch_sampler():
    B, Cn, H, W, P, nc = 2, 5, 6, 7, 9, 8
    feat = C.randn(906, B, Cn, H, W)
    ids = C.patch_ids(3, 0, H * W, P)
    plain = O.PatchSampler(nc, False)
    assert rel(R.l2_normalize(R.patch_gather(feat, ids)), plain([feat], P, [ids])[0][0]) <= 2e-5
    smp = O.PatchSampler(nc, True)
    smp.create_mlp([feat])
    with torch.no_grad():
        for i, p_ in enumerate(smp.mlp_0.parameters()):
            p_.copy_(C.randn(907 + i, *p_.shape) * 0.5)
    cot = C.randn(911, B * P, nc)
    fo = feat.clone().requires_grad_()
    (smp([fo], P, [ids])[0][0] * cot).sum().backward()
    leaves = [t.detach().double().requires_grad_() for t in [feat] + list(smp.mlp_0.parameters())]
    y = R.nce_head(leaves[0], ids, *leaves[1:])
    (y * cot.double()).sum().backward()
    assert rel(y, smp([feat], P, [ids])[0][0]) <= 2e-5
    for a, b in zip([t.grad for t in leaves], [fo.grad] + [p_.grad for p_ in smp.mlp_0.parameters()]):
        assert rel(a, b) <= 1e-4
    # grouped ids and the adjoint: <gather(f), d> == <f, adjoint(d)>, repeated ids accumulate
    G, Bper = 3, 2
    f = C.randn(912, G * Bper, Cn, H, W).double()
    gids = torch.stack([C.patch_ids(4 + g, 0, H * W, P) for g in range(G)])
    gids[1, 4] = gids[1, 0]
    rows = R.patch_gather(f, gids, G)
    for b in range(G * Bper):
        assert torch.equal(rows[b * P:(b + 1) * P], f[b].reshape(Cn, -1)[:, gids[b // Bper]].t())
    d = C.randn(913, G * Bper * P, Cn).double()
    adj = R.patch_gather_adjoint(d, gids, G, f.shape)
    assert abs(float((rows * d).sum() - (f * adj).sum())) <= 1e-12 * float(d.abs().sum())
    pos = int(gids[1, 0])
    assert torch.equal(adj[2, :, pos // W, pos % W], d[2 * P + 0] + d[2 * P + 4])


def test_segment_means_and_scalar_combine():
    rows = C.randn(914, 5, 3 * 257).double()
    ref = sum(rows[l].reshape(3, 257).mean(1) for l in range(5)) * -0.3
    assert rel(R.segment_means(rows, 3, -0.3), ref) <= 1e-14
    M, xs = C.randn(915, 4, 3), [C.randn(916 + i, 1).double() for i in range(3)]
    assert rel(R.scalar_combine(M.tolist(), xs), M.double() @ torch.cat(xs)) <= 1e-14


def _nce_variants(G):
    for case in G.VARIANT_SHAPES:
        for variant in ("plain", "correlated", "ties", "unnormalised", "zero-row"):
            for T in ((1.0, 0.01, G.T0) if variant == "plain" else (G.T0,)):
                yield case, variant, T


def test_patchnce_gpu_inputs_are_testable():
    """Every shape of the GPU module's table and every well-conditioned variant: the fp32 oracle sits a factor 10 inside the bars
    in the sharp metrics (so the bars stand on their own there); the correlated keys give float64 row losses in [0.05, 1]; the
    unnormalised input, compared through bounded(oracle=...), stays under the 10 x bar cap."""
    G = _nce_module()
    worst = [0.0, 0.0]
    cases = [(c, "plain", G.T0, 700) for c in G.NCE_CASES] + [v + (720,) for v in _nce_variants(G)]    # the GPU tests' seeds
    for (name, Rr, Cn, Gr), variant, T, seed in cases:
        q, k, cot = G.nce_inputs(Rr, Cn, Gr, variant, seed=seed)
        lr, dqr = G.nce_reference(q, k, cot, Gr, T)
        lo, dqo = G.nce_oracle(q, k, cot, Gr, T)
        if variant == "correlated":
            assert 0.05 <= float(lr.min()) and float(lr.max()) <= 1.0, (name, float(lr.min()), float(lr.max()))
        if variant in G.ILL_VARIANTS:
            assert G.oracle_bound(lr, lo, G.BAR)[0] <= 10 * G.BAR, name
            assert G.oracle_bound(dqr, dqo, G.BAR_DQ)[0] <= 10 * G.BAR_DQ, name
        else:
            worst[0], worst[1] = max(worst[0], G.rows_err(lo, lr)), max(worst[1], G.per_row_err(dqo, dqr))
            assert G.rows_err(lo, lr) <= G.BAR / 10 and G.per_row_err(dqo, dqr) <= G.BAR_DQ / 10, (name, variant, T)
        assert bool((dqr[cot == 0] == 0).all())
    assert worst[0] > 0.0 and worst[1] > 0.0


@pytest.mark.parametrize("route,P,all_neg", _nce_module().ROUTES,
                         ids=["%s-P%d-%s" % (r, P, "allneg" if a else "perimage") for r, P, a in _nce_module().ROUTES])
def test_host_route_inputs_are_testable(route, P, all_neg):
    """The end-to-end routes compare their gradients through bounded(oracle=...): the oracle in fp32 against itself in float64,
    on the GPU test's inputs and a seeded id draw of the same size, stays under the cap."""
    G = _nce_module()
    fq, fk, params, nc = G.route_inputs(route)
    Pn = min(P, 256)
    ids = C.patch_ids(7, 0, 256, Pn)
    cot = G.route_cot(2 * Pn)
    ref = G.route_oracle(route, fq, fk, params, nc, ids, all_neg, cot, torch.float64)
    o32 = G.route_oracle(route, fq, fk, params, nc, ids, all_neg, cot, torch.float32)
    assert G.rows_err(o32[0], ref[0]) <= G.BAR / 10
    for r, o, bar in zip(ref[1:], o32[1:], (G.BAR_DFEAT, G.BAR_DQ, G.BAR_DQ, G.BAR_DQ, G.BAR_DQ)):
        assert G.oracle_bound(r, o, bar)[0] <= 10 * bar


def test_l2norm_gpu_inputs_are_testable():
    """ops.l2norm_rows' cases: plain fp32 torch stays far inside the bar in the per-row metric at every shape, scale and eps
    with C > 1; at C = 1 against the scale the GPU test uses."""
    G = _nce_module()
    for (Cn, rows) in G.L2_SHAPES:
        for scale in (1.0, 1e-6, 1e15):
            for eps in (1e-7, 1e-3):
                x, dy = G.l2_inputs(Cn, rows, scale)
                yr, dxr = R.l2_normalize(x, eps), R.l2_normalize_grad(x, dy, eps)
                yo, dxo = R.l2_normalize(x, eps, dtype=torch.float32), R.l2_normalize_grad(x, dy, eps, dtype=torch.float32)
                assert G.per_row_err(yo, yr) <= G.BAR / 10
                if Cn == 1:
                    floor = float(dy.abs().max()) / (float(x.abs().min()) + eps)
                    assert G.oracle_bound(dxr, dxo, G.BAR, floor=floor)[1] <= G.BAR / 10
                else:
                    assert G.per_row_err(dxo, dxr) <= G.BAR / 10, (Cn, rows, scale, eps)


# ------------------------------------------------------------------- convolution weight / bias gradients
def _conv_autograd(x, dy, Cout, K, stride, pad, reflect):
    """dW, db of float64 autograd through F.conv2d / F.conv3d with a bias (the weights' values play no part)."""
    nd = x.dim() - 2
    conv = F.conv2d if nd == 2 else F.conv3d
    w = torch.zeros((Cout, x.shape[1]) + (K,) * nd, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(Cout, dtype=torch.float64, requires_grad=True)
    xd = x.double()
    if reflect:
        y = conv(F.pad(xd, (pad,) * (2 * nd), mode="reflect"), w, b, stride=stride)
    else:
        y = conv(xd, w, b, stride=stride, padding=pad)
    (y * dy.double()).sum().backward()
    return w.grad, b.grad


WG_CASES = [  # nd, Cin, Cout, K, stride, pad, reflect, N, spatial
    (2, 3, 5, 1, 1, 0, False, 2, (7, 9)), (2, 3, 5, 1, 2, 0, False, 2, (7, 9)),
    (2, 4, 3, 3, 1, 1, False, 2, (9, 13)), (2, 4, 3, 3, 1, 1, True, 2, (9, 13)),
    (2, 4, 3, 3, 2, 1, False, 1, (15, 17)), (2, 4, 3, 3, 2, 1, True, 1, (16, 10)),
    (2, 1, 6, 7, 1, 3, True, 2, (11, 12)), (2, 2, 3, 7, 1, 3, False, 1, (9, 20)), (2, 2, 3, 7, 2, 3, True, 1, (13, 12)),
    (3, 3, 4, 3, 1, 1, False, 2, (5, 7, 9)), (3, 3, 4, 3, 1, 1, True, 1, (5, 7, 9)),
    (3, 2, 5, 3, 2, 1, False, 1, (9, 11, 13)), (3, 2, 5, 3, 2, 1, True, 1, (8, 6, 10)),
    (3, 3, 2, 1, 1, 0, False, 1, (4, 5, 6)), (3, 2, 2, 7, 1, 3, False, 1, (7, 8, 9)), (3, 1, 2, 7, 2, 3, True, 1, (8, 9, 7)),
]


@pytest.mark.parametrize("cfg", WG_CASES, ids=[str(c) for c in WG_CASES])
@pytest.mark.parametrize("order", ["matmul", "chunk64"])
def test_conv_weight_and_bias_grad(cfg, order):
    nd, Cin, Cout, K, stride, pad, reflect, N, sp = cfg
    x = C.randn(501, N, Cin, *sp)
    out = tuple((n + 2 * pad - K) // stride + 1 for n in sp)
    dy = C.randn(502, N, Cout, *out)
    dw_ref, db_ref = _conv_autograd(x, dy, Cout, K, stride, pad, reflect)
    dw = R.conv_weight_grad(x, dy, K, stride, pad, 1 if reflect else 0, order=order)
    assert dw.dtype == torch.float64 and rel(dw, dw_ref) <= 1e-13
    assert rel(R.conv_bias_grad(dy, order=order), db_ref) <= 1e-13
    # the fp32 restatement is the same sum at fp32 round-off
    assert rel(R.conv_weight_grad(x, dy, K, stride, pad, 1 if reflect else 0, torch.float32, order), dw_ref) <= 2e-5
    assert rel(R.conv_bias_grad(dy, torch.float32, order), db_ref) <= 2e-5


def test_conv_weight_grad_of_a_2d_layer_given_as_5d():
    """[N, C, 1, H, W] with K = (1, 3, 3), pad = (0, 1, 1): the form the GPU tests hand to ops.conv_wgrad_raw."""
    x, dy = C.randn(503, 2, 3, 8, 10), C.randn(504, 2, 4, 8, 10)
    for mode in (0, 1):
        a = R.conv_weight_grad(x, dy, 3, 1, 1, mode)
        b = R.conv_weight_grad(x.unsqueeze(2), dy.unsqueeze(2), (1, 3, 3), 1, (0, 1, 1), mode)
        assert torch.equal(a, b[:, :, 0])


@pytest.mark.parametrize("order", ["matmul", "chunk64"])
def test_conv_weight_grad_upcat_form(order):
    a, b = C.randn(505, 2, 8, 3, 4, 4), C.randn(506, 2, 3, 6, 8, 8)
    dy = C.randn(507, 2, 5, 6, 8, 8)
    xcat = torch.cat([F.interpolate(a, scale_factor=2, mode="nearest"), b], 1)
    assert torch.equal(R.upcat(a, b), xcat)
    dw_ref, _ = _conv_autograd(xcat, dy, 5, 3, 1, 1, False)
    assert rel(R.conv_weight_grad((a, b), dy, 3, 1, 1, 0, order=order), dw_ref) <= 1e-13


def test_conv_weight_grad_orders_differ_in_fp32_only():
    """The two evaluation orders are the same numbers in float64 (to its round-off) and two different roundings in fp32."""
    x, dy = C.randn(508, 2, 6, 24, 40), C.randn(509, 2, 7, 24, 40)
    d64 = [R.conv_weight_grad(x, dy, 3, 1, 1, 0, order=o) for o in ("matmul", "chunk64")]
    d32 = [R.conv_weight_grad(x, dy, 3, 1, 1, 0, torch.float32, o) for o in ("matmul", "chunk64")]
    assert rel(d64[0], d64[1]) <= 1e-13
    assert not torch.equal(d32[0], d32[1]) and rel(d32[0], d32[1]) <= 1e-5
