"""MIND_Loss / ops.mind_descriptor (build-defined MIND-SSC, dfmir_amd/csrc/mind.hip): the C ABI and the argument checks
(CPU), a float64 restatement of the definition written from its formulas (index_select with clamped indices, explicit
first-index argmin routing, detached mu), checked on the CPU against plain autograd of the textbook composition, and on the
GPU against the kernels: descriptor, loss and both gradients on shapes around the tile and border cases, clamped regions
with ties in the min, masks, structural identities, run-to-run bit-reproducibility and Registration3DModel(similarity='mind')
eager and captured.

Tolerances (profiles/mind_margins.txt): the bound of every comparison with the restatement is 4x the error of the SAME
definition evaluated by torch in fp32 on the CPU against the float64 restatement, on these inputs -- the maxima over the
case set: 1.03e-7 relative on the loss, 5.63e-6 on a gradient in relative 2-norm, 1.04e-5 as max-abs over max, 5.74e-6 on
the descriptor (max-abs over max).  scripts/mind_margins.py measures them, and the kernels' own errors beside them."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests.golden import common as C

DEV = "cuda"
FACTOR = 4.0
FP32_ERR_LOSS, FP32_ERR_GRAD_L2, FP32_ERR_GRAD_MAX, FP32_ERR_DESC = 1.03e-7, 5.63e-6, 1.04e-5, 5.74e-6   # profiles/mind_margins.txt
B_LOSS, B_L2, B_MAX, B_DESC = (FACTOR * e for e in (FP32_ERR_LOSS, FP32_ERR_GRAD_L2, FP32_ERR_GRAD_MAX, FP32_ERR_DESC))

SHAPES = [(2, 1, 5, 6, 7), (1, 1, 3, 2, 70), (2, 1, 13, 17, 19), (1, 1, 1, 20, 33), (1, 1, 6, 10, 35),
          (2, 1, 9, 11), (1, 1, 3, 70), (2, 1, 37, 41)]
CASES = [(s, 2, 2) for s in SHAPES] + [(s, r, d) for s in ((2, 1, 13, 17, 19), (2, 1, 37, 41)) for r, d in ((1, 1), (3, 2))]


def _id(case):
    return "x".join(str(v) for v in case[0]) + "-r%dd%d" % case[1:]


# ------------------------------------------------------------------------------------------ restatement
def channels(nd):
    """The documented channel order: pairs p < q of the neighbours n = 2 * axis + (0: -d, 1: +d) on different axes."""
    return [(p, q) for p in range(2 * nd) for q in range(p + 1, 2 * nd) if p // 2 != q // 2]


def _take(x, dim, off):
    n = x.shape[dim]
    return x.index_select(dim, (torch.arange(n) + off).clamp(0, n - 1))


def mind_ref(I, r=2, d=2, info=None):
    """M [B,C,*vol] of I [B,1,*vol] in I's dtype on the CPU, differentiable; mu detached, the min routed to the first
    minimal channel, nothing through V where it is clamped.  info (a dict) receives the clamped fractions."""
    nd = I.dim() - 2
    nb = [_take(I, 2 + n // 2, d if n & 1 else -d) for n in range(2 * nd)]
    Ds = []
    for p, q in channels(nd):
        s = (nb[p] - nb[q]) ** 2
        for ax in range(nd):
            acc = _take(s, 2 + ax, -r)
            for t in range(-r + 1, r + 1):
                acc = acc + _take(s, 2 + ax, t)
            s = acc
        Ds.append(s * (1.0 / (2 * r + 1) ** nd))
    Dm = torch.cat(Ds, 1)
    is_min = Dm.detach() == Dm.detach().min(1, keepdim=True).values
    first = is_min & (is_min.to(torch.int64).cumsum(1) == 1)
    m = Dm - (Dm * first.to(Dm.dtype)).sum(1, keepdim=True)
    V = m.mean(1, keepdim=True)
    mu = V.detach().mean()
    lo, hi = 0.001 * mu, 1000.0 * mu
    Vc = torch.where(V.detach() < lo, lo.expand_as(V), torch.where(V.detach() > hi, hi.expand_as(V), V))
    if info is not None:
        info["low"] = float((V.detach() < lo).double().mean())
        info["high"] = float((V.detach() > hi).double().mean())
        info["ties"] = float((is_min.sum(1) > 1).double().mean())
    return torch.exp(-m / Vc)


def mind_loss_ref(a, b, r=2, d=2, mask=None, dtype=torch.float64, info=None):
    """(loss, d/da, d/db) of the definition on the CPU in `dtype` (float64: the restatement; float32: the yardstick)."""
    x = a.detach().cpu().to(dtype).requires_grad_()
    y = b.detach().cpu().to(dtype).requires_grad_()
    ia, ib = ({}, {}) if info is not None else (None, None)
    Ma, Mb = mind_ref(x, r, d, ia), mind_ref(y, r, d, ib)
    if info is not None:
        info["a"], info["b"] = ia, ib
    sq = (Ma - Mb) ** 2
    if mask is None:
        loss = sq.mean()
    else:
        w = mask.detach().cpu().to(dtype).expand_as(x)
        if float(w.sum()) == 0.0:
            return 0.0, torch.zeros_like(x), torch.zeros_like(y)
        loss = (w * sq.mean(1, keepdim=True)).sum() / w.sum()
    loss.backward()
    return float(loss.detach()), x.grad, y.grad


def mind_textbook(I, r, d):
    """The textbook composition with stock torch ops (replicate padding, avg_pool, min, clamp): shares no code with mind_ref."""
    nd = I.dim() - 2
    pad = lambda x, n: F.pad(x, (n,) * (2 * nd), mode='replicate')
    Ip = pad(I, d)
    sp = I.shape[2:]

    def shifted(n):
        sl = [slice(None), slice(None)] + [slice(d, d + e) for e in sp]
        ax = n // 2
        o = d + (d if n & 1 else -d)
        sl[2 + ax] = slice(o, o + sp[ax])
        return Ip[tuple(sl)]

    pool = F.avg_pool3d if nd == 3 else F.avg_pool2d
    Dm = torch.cat([pool(pad((shifted(p) - shifted(q)) ** 2, r), 2 * r + 1, stride=1) for p, q in channels(nd)], 1)
    m = Dm - Dm.min(1, keepdim=True).values
    V = m.mean(1, keepdim=True)
    mu = V.mean().detach()
    return torch.exp(-m / V.clamp(min=0.001 * mu, max=1000.0 * mu))


def mind_inputs(shape, seed):
    """0.7 * normalised(5-wide box-smoothed uniform noise) + 0.3 * uniform noise, twice (seeded)."""
    out = []
    for s in (seed, seed + 1):
        x = C.rand(s, *shape).double()
        sm = x
        for ax in range(len(shape) - 2):
            sm = sum(_take(sm, 2 + ax, t) for t in range(-2, 3)) / 5.0
        sm = (sm - sm.min()) / (sm.max() - sm.min())
        out.append((0.7 * sm + 0.3 * C.rand(s + 100, *shape).double()).float())
    return out


def rel_errors(loss, grads, loss64, grads64):
    """(relative error of the loss, worst relative 2-norm error of the gradients, worst max-abs over max)."""
    el = abs(float(loss) - loss64) / abs(loss64)
    l2 = mx = 0.0
    for g, g64 in zip(grads, grads64):
        g, g64 = g.detach().cpu().double(), g64.double()
        l2 = max(l2, float((g - g64).norm() / g64.norm()))
        mx = max(mx, float((g - g64).abs().max() / g64.abs().max()))
    return el, l2, mx


_REF = {}


def reference(case, seed=500):
    """(a, b, loss64, da64, db64, info) of a case, computed once and shared."""
    if case not in _REF:
        shape, r, d = case
        a, b = mind_inputs(shape, seed + 7 * SHAPES.index(shape))
        info = {}
        loss, da, db = mind_loss_ref(a, b, r, d, info=info)
        _REF[case] = (a, b, loss, da, db, info)
    return _REF[case]


def clamped_pair():
    """(1,1,9,12,14): `a` with the columns x < 5 set to 0, `b` with the last five rows (y >= 7) set to 0.25.  A voxel sits on
    the low bound when its whole support lies in the flat band, which takes r + d + 1 = 5 flat positions from the border:
    7 % of `a` (x = 0) and 8 % of `b` (y = 11).  With four flat rows (y >= 8) the restatement clamps no voxel of `b` at all,
    so the band is five rows wide here.  Ties in the min occur throughout the flat parts."""
    a, b = mind_inputs((1, 1, 9, 12, 14), 900)
    a[..., :5] = 0.0
    b[..., 7:, :] = 0.25
    return a, b


def _gpu_loss(a, b, r=2, d=2, mask=None):
    from dfmir_amd import ops
    x, y = a.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
    loss = ops.mind_loss(x, y, r, d, mask=None if mask is None else mask.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), x.grad.cpu(), y.grad.cpu()


def _check(got, ref, what):
    el, l2, mx = rel_errors(got[0], got[1:], ref[0], ref[1:])
    print("%s: loss %.3e (bound %.1e)  grad l2 %.3e (%.1e)  grad max %.3e (%.1e)" % (what, el, B_LOSS, l2, B_L2, mx, B_MAX))
    assert all(bool(torch.isfinite(g).all()) for g in got[1:]), what
    assert el <= B_LOSS and l2 <= B_L2 and mx <= B_MAX, (what, el, l2, mx)


# ------------------------------------------------------------------------------------------ CPU tier
def test_mind_symbols_in_header_exports_and_ctypes_table():
    import dfmir_amd
    from dfmir_amd import _lib
    from tests.test_abi import header_symbols
    h = ctypes.CDLL(dfmir_amd.LIB_PATH)
    for s in ("dfmir_mind_ws_floats", "dfmir_mind_desc", "dfmir_mind_fwd", "dfmir_mind_bwd"):
        assert s in header_symbols() and s in _lib.exported_symbols() and hasattr(h, s), s
    lib = dfmir_amd.lib()
    assert lib.dfmir_abi_version() == 14
    assert lib.dfmir_mind_ws_floats(3, 1, 8, 8, 8, 2, 2, 0) > 2 * 12 * 512
    assert lib.dfmir_mind_ws_floats(3, 1, 8, 8, 8, 2, 2, 1) == 2 * 12 * 512
    assert lib.dfmir_mind_ws_floats(2, 2, 1, 8, 8, 4, 4, 1) == 2 * 2 * 4 * 64
    for bad in ((4, 1, 8, 8, 8, 2, 2, 0), (2, 1, 2, 8, 8, 2, 2, 0), (3, 1, 8, 8, 8, 0, 2, 0), (3, 1, 8, 8, 8, 2, 5, 0),
                (3, 0, 8, 8, 8, 2, 2, 0), (3, 1, 8, 8, 8, 2, 2, 2)):
        assert lib.dfmir_mind_ws_floats(*bad) == -1, bad


def test_mind_null_arguments_are_invalid_without_a_device():
    import dfmir_amd
    lib = dfmir_amd.lib()
    assert lib.dfmir_mind_desc(None, 3, 1, 8, 8, 8, 2, 2, None, None, None) != 0
    assert b"invalid argument" in lib.dfmir_last_error()
    assert lib.dfmir_mind_fwd(None, None, None, 3, 1, 8, 8, 8, 2, 2, None, None, None) != 0
    assert b"invalid argument" in lib.dfmir_last_error()
    assert lib.dfmir_mind_bwd(None, None, None, 3, 1, 8, 8, 8, 2, 2, None, None, None, None, None, None) != 0
    assert b"invalid argument" in lib.dfmir_last_error()


def test_mind_loss_rejects_bad_arguments_before_any_launch():
    from dfmir_amd import ops
    from dfmir_amd._lib import DfmirHipError
    from dfmir_amd.losses import MIND_Loss
    x = torch.rand(1, 1, 8, 8, 8)
    with pytest.raises(ValueError, match="radius"):
        MIND_Loss(radius=0)
    with pytest.raises(ValueError, match="dilation"):
        MIND_Loss(dilation=5)
    with pytest.raises(ValueError, match="dilation"):
        ops.mind_loss(x, x, dilation=5)
    with pytest.raises(ValueError, match="single-channel"):
        MIND_Loss()(torch.rand(1, 2, 8, 8), torch.rand(1, 2, 8, 8))
    with pytest.raises(ValueError, match="dims"):
        ops.mind_descriptor(torch.rand(1, 1, 8))
    with pytest.raises(DfmirHipError, match="no CPU fallback"):
        MIND_Loss()(x, x)
    with pytest.raises(DfmirHipError, match="no CPU fallback"):
        ops.mind_descriptor(x)
    crit = MIND_Loss(radius=3, dilation=1)
    assert crit.name == 'mind' and (crit.radius, crit.dilation) == (3, 1)


def test_registration3d_constructs_with_mind_and_still_rejects_unknown():
    from dfmir_amd.losses import MIND_Loss
    from dfmir_amd.registration3d import Registration3DModel
    m = Registration3DModel((8, 8, 8), device="cpu", similarity="mind", mind_radius=1, mind_dilation=3)
    assert isinstance(m.criterionMIND, MIND_Loss) and (m.criterionMIND.radius, m.criterionMIND.dilation) == (1, 3)
    assert 'loss_mind' in m._outputs
    m2 = Registration3DModel((8, 8), device="cpu", similarity="mind")
    assert m2.criterionGrad.dim == 2
    with pytest.raises(ValueError, match="'ncc', 'nmi' or 'mind'"):
        Registration3DModel((8, 8, 8), device="cpu", similarity="mi")


def test_mind_channel_order_is_the_documented_one():
    assert channels(3) == [(0, 2), (0, 3), (0, 4), (0, 5), (1, 2), (1, 3), (1, 4), (1, 5), (2, 4), (2, 5), (3, 4), (3, 5)]
    assert channels(2) == [(0, 2), (0, 3), (1, 2), (1, 3)]


@pytest.mark.parametrize("shape", [(2, 1, 5, 6, 7), (1, 1, 1, 20, 33), (2, 1, 9, 11)], ids=["3d", "plane", "2d"])
def test_restatement_equals_autograd_of_the_textbook_formula(shape):
    """On inputs that clamp no voxel and tie no minimum the three build-defined points do not act: the restatement's
    descriptor, loss and gradients are those of plain autograd through stock torch ops."""
    a, b = mind_inputs(shape, 500 + 7 * SHAPES.index(shape))
    info = {}
    loss, da, db = mind_loss_ref(a, b, info=info)
    assert info["a"]["low"] == info["a"]["high"] == info["b"]["low"] == info["b"]["high"] == 0.0
    if shape[2:] != (1, 20, 33):        # (one plane: the channels (0,n) and (1,n) coincide, so either routing of the tie
        assert info["a"]["ties"] == info["b"]["ties"] == 0.0       # gives the same gradient)
    assert 0.05 < loss < 0.4
    x, y = a.double().requires_grad_(), b.double().requires_grad_()
    Mx = mind_textbook(x, 2, 2)
    assert Mx.shape[1] == (12 if len(shape) == 5 else 4)
    tl = ((Mx - mind_textbook(y, 2, 2)) ** 2).mean()
    tl.backward()
    assert float((Mx.detach() - mind_ref(a.double())).abs().max()) <= 1e-14
    assert abs(float(tl.detach()) - loss) <= 1e-14 * loss
    for g, t in ((da, x.grad), (db, y.grad)):
        assert float((g - t).abs().max()) <= 1e-13 * float(t.abs().max())


def test_restatement_clamps_and_ties_on_the_flat_pair():
    a, b = clamped_pair()
    info = {}
    loss, da, db = mind_loss_ref(a, b, info=info)
    assert info["a"]["low"] > 0.05 and info["b"]["low"] > 0.05, info
    assert info["a"]["high"] == 0.0 and info["b"]["high"] == 0.0
    assert info["a"]["ties"] > 0.0 and info["b"]["ties"] > 0.0
    assert bool(torch.isfinite(da).all()) and bool(torch.isfinite(db).all()) and loss > 0.0


# ------------------------------------------------------------------------------------------ GPU tier
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_mind_descriptor_loss_and_gradients_vs_restatement(case):
    from dfmir_amd import ops
    shape, r, d = case
    a, b, loss64, da64, db64, info = reference(case)
    assert info["a"]["low"] == info["a"]["high"] == info["b"]["low"] == info["b"]["high"] == 0.0
    M = ops.mind_descriptor(a.to(DEV), r, d).cpu()
    M64 = mind_ref(a.double(), r, d)
    assert M.shape == M64.shape and M.shape[1] == (12 if len(shape) == 5 else 4)
    em = float((M.double() - M64).abs().max() / M64.abs().max())
    print("%s: descriptor max %.3e (bound %.1e)" % (_id(case), em, B_DESC))
    assert em <= B_DESC, em
    _check(_gpu_loss(a, b, r, d), (loss64, da64, db64), _id(case))


@pytest.mark.gpu
def test_mind_clamped_regions_and_min_ties():
    a, b = clamped_pair()
    info = {}
    ref = mind_loss_ref(a, b, info=info)
    assert info["a"]["low"] > 0.05 and info["b"]["low"] > 0.05 and info["a"]["ties"] > 0.0 and info["b"]["ties"] > 0.0
    _check(_gpu_loss(a, b), ref, "clamped")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["broadcast", "binary", "empty"])
def test_mind_mask(kind):
    case = ((2, 1, 13, 17, 19), 2, 2)
    a, b = reference(case)[:2]
    if kind == "broadcast":
        mask = C.rand(77, 1, 1, 13, 17, 19)
    elif kind == "binary":
        mask = (C.rand(78, 2, 1, 13, 17, 19) > 0.4).float()
    else:
        mask = torch.zeros(2, 1, 13, 17, 19)
    got = _gpu_loss(a, b, mask=mask)
    if kind == "empty":
        assert float(got[0]) == 0.0 and float(got[1].abs().max()) == 0.0 and float(got[2].abs().max()) == 0.0
        assert not bool(torch.isnan(got[1]).any()) and not bool(torch.isnan(got[2]).any())
        return
    _check(got, mind_loss_ref(a, b, mask=mask), "mask " + kind)


@pytest.mark.gpu
def test_mind_structure():
    from dfmir_amd import ops
    case = ((2, 1, 13, 17, 19), 2, 2)
    a, b = reference(case)[:2]
    l0, g0, g1 = _gpu_loss(a, a.clone())
    assert float(l0) == 0.0 and float(g0.abs().max()) == 0.0 and float(g1.abs().max()) == 0.0
    lab, dab_a, dab_b = _gpu_loss(a, b)
    lba, dba_b, dba_a = _gpu_loss(b, a)
    assert torch.equal(lab, lba) and torch.equal(dab_a, dba_a) and torch.equal(dab_b, dba_b)
    # contrast invariance: the descriptor of alpha I + beta is the descriptor of I
    M = ops.mind_descriptor(a.to(DEV)).cpu().double()
    M2 = ops.mind_descriptor((-3.0 * a + 0.4).to(DEV)).cpu().double()
    err = float((M - M2).abs().max() / M.abs().max())
    print("contrast invariance: %.3e (bound %.1e)" % (err, B_DESC))
    assert err <= B_DESC


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 1, 13, 17, 19), (2, 1, 37, 41)], ids=["3d", "2d"])
def test_mind_bit_reproducible(shape):
    a, b = reference((shape, 2, 2))[:2]
    r0, r1 = _gpu_loss(a, b), _gpu_loss(a, b)
    for x, y in zip(r0, r1):
        assert torch.equal(x, y)


def _step_model(capture):
    from tests import step3d
    return step3d.step_model((16, 16, 16), 'mind', capture=capture)


@pytest.mark.gpu
def test_registration3d_mind_step_matches_restatement():
    m, A, B = _step_model(False)
    m.set_input({"A": A, "B": B})
    m.optimize_parameters()
    torch.cuda.synchronize()
    got = m.get_current_losses()
    assert sorted(got) == ["grad", "mind"]
    ref = mind_loss_ref(m.regA, m.real_B)[0]
    err = abs(got["mind"] - ref) / abs(ref)
    print("step loss_mind: %.3e (bound %.1e)" % (err, B_LOSS))
    assert err <= B_LOSS
    assert float(m.optimizer_R.flat_g.abs().max()) > 0.0


@pytest.mark.gpu
def test_registration3d_mind_captured_step_matches_eager():
    """similarity='mind' under capture_step=True: a replayed step equals the same step enqueued eagerly (the pattern of
    test_nmi.py's captured-step test)."""
    from tests import step3d
    m, A, B = _step_model(True)
    m.parallelize()
    step3d.assert_replay_matches_eager(m, {"A": A, "B": B}, ["grad", "mind"])
