"""GradField_Loss / ops.gradfield_loss / ops.gradfield_normals (build-defined normalised-gradient-field distance,
dfmir_amd/csrc/gradfield.hip): the C ABI and the argument checks (CPU), a float64 restatement of the definition written from
its formulas (index_select with clamped indices, detached eps), checked on the CPU against plain autograd through
F.pad(mode='replicate') and slicing, and on the GPU against the kernels: loss, both gradients and the field on shapes that
cross a tile edge, leave a partial tile, hit both clamps on one voxel, take the scalar-load path or one more plane than a z
chunk (of 4, 8 or 16 planes by the size of the grid), each with eps='auto', a given pair and 'auto' under an anisotropic spacing; masks, one-sided gradients,
contrast invariance, the argument swap, a constant image, run-to-run bit-reproducibility and
Registration3DModel(similarity='gradfield') eager, captured and symmetric.

Tolerances (profiles/gradfield_margins.txt): the bound of every comparison with the restatement is 4x the error of the SAME
definition evaluated by torch in fp32 on the CPU against the float64 restatement, on these inputs -- the maxima over the
case set: 1.21e-7 relative on the loss, 5.14e-7 on a gradient in relative 2-norm, 6.83e-7 as max-abs over max, 1.62e-7 on
the field (max-abs over max) -- floored at 1e-6 (about 8 ulp of fp32: below that a comparison measures summation order).
scripts/gradfield_margins.py measures them, and the kernels' own errors beside them."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests.golden import common as C
from tests.test_mind import _take, mind_inputs

DEV = "cuda"
FACTOR, FLOOR = 4.0, 1e-6
FP32_ERR_LOSS, FP32_ERR_GRAD_L2, FP32_ERR_GRAD_MAX, FP32_ERR_FIELD = 1.21e-7, 5.14e-7, 6.83e-7, 1.62e-7   # profiles/gradfield_margins.txt
B_LOSS, B_L2, B_MAX, B_FIELD = (max(FACTOR * e, FLOOR) for e in (FP32_ERR_LOSS, FP32_ERR_GRAD_L2, FP32_ERR_GRAD_MAX,
                                                                FP32_ERR_FIELD))

SHAPES = [(2, 1, 5, 6, 7), (1, 1, 3, 2, 70), (2, 1, 13, 17, 19), (1, 1, 1, 20, 33), (1, 1, 2, 1, 5), (1, 1, 6, 10, 67),
          (1, 1, 17, 9, 68), (2, 1, 9, 11), (1, 1, 3, 70), (2, 1, 37, 41), (1, 1, 1, 9),
          (384, 1, 17, 2, 5), (256, 1, 17, 2, 5)]        # (the last two: enough workgroups for z chunks of 16 and of 8)
EPS_PAIR = (0.05, 0.02)


def _spacing(shape):
    return (2.5, 1.0, 0.8) if len(shape) == 5 else (2.5, 0.8)


# (shape, eps, spacing, related)
CASES = [(s, e, sp(s), False) for s in SHAPES for e, sp in (('auto', lambda s: None), (EPS_PAIR, lambda s: None),
                                                            ('auto', _spacing))]
CASES += [((2, 1, 13, 17, 19), EPS_PAIR, None, True), ((2, 1, 13, 17, 19), 'auto', None, True),
          ((2, 1, 37, 41), EPS_PAIR, None, True)]


def _id(case):
    shape, eps, spacing, related = case
    return "x".join(str(v) for v in shape) + ("-auto" if eps == 'auto' else "-pair") + ("-aniso" if spacing else "") + \
        ("-related" if related else "")


# ------------------------------------------------------------------------------------------ restatement
def grad_ref(I, spacing=None):
    """[g_a(I)] over the axes (z,) y, x: the clamped central differences over 2 h_a."""
    nd = I.dim() - 2
    h = (1.0,) * nd if spacing is None else spacing
    return [(_take(I, 2 + ax, 1) - _take(I, 2 + ax, -1)) / (2.0 * h[ax]) for ax in range(nd)]


def eps_ref(g, eps, eta, which):
    """eps of one image from its gradient list: the given value, or eta * mean |g| (detached)."""
    if eps == 'auto':
        return eta * sum(c.detach() ** 2 for c in g).sqrt().mean()
    return torch.tensor(float(eps[which] if isinstance(eps, (tuple, list)) else eps), dtype=g[0].dtype)


def field_ref(I, eps='auto', eta=1.0, spacing=None):
    """n(I) [B,nd,*vol] in I's dtype on the CPU; 0 where |g|^2 + eps^2 == 0."""
    g = grad_ref(I, spacing)
    d = sum(c ** 2 for c in g) + eps_ref(g, eps, eta, 0) ** 2
    r = torch.where(d > 0, torch.where(d > 0, d, torch.ones_like(d)).rsqrt(), torch.zeros_like(d))
    return torch.cat([c * r for c in g], 1)


def similarity_ref(x, y, eps='auto', eta=1.0, spacing=None):
    """s [B,1,*vol]: dot^2 / (D_A D_B), 0 (with no gradient) where D_A D_B == 0."""
    ga, gb = grad_ref(x, spacing), grad_ref(y, spacing)
    dot = sum(p * q for p, q in zip(ga, gb))
    prod = (sum(p ** 2 for p in ga) + eps_ref(ga, eps, eta, 0) ** 2) * (sum(q ** 2 for q in gb) + eps_ref(gb, eps, eta, 1) ** 2)
    ok = prod > 0
    return torch.where(ok, dot ** 2 / torch.where(ok, prod, torch.ones_like(prod)), torch.zeros_like(prod))


def gradfield_loss_ref(a, b, eps='auto', eta=1.0, spacing=None, mask=None, dtype=torch.float64):
    """(loss, d/da, d/db) of the definition on the CPU in `dtype` (float64: the restatement; float32: the yardstick)."""
    x = a.detach().cpu().to(dtype).requires_grad_()
    y = b.detach().cpu().to(dtype).requires_grad_()
    one_minus_s = 1.0 - similarity_ref(x, y, eps, eta, spacing)
    if mask is None:
        loss = one_minus_s.mean()
    else:
        w = mask.detach().cpu().to(dtype).expand_as(x)
        if float(w.sum()) == 0.0:
            return 0.0, torch.zeros_like(x), torch.zeros_like(y)
        loss = (w * one_minus_s).sum() / w.sum()
    loss.backward()
    return float(loss.detach()), x.grad, y.grad


def gradfield_textbook(x, y, eta=1.0):
    """The loss with 'auto' eps and unit spacing from stock torch ops (replicate padding and slicing): shares no code with
    the restatement."""
    nd = x.dim() - 2

    def grads(I):
        P = F.pad(I, (1, 1) * nd, mode='replicate')
        out = []
        for ax in range(nd):
            hi = [slice(None), slice(None)] + [slice(1, 1 + n) for n in I.shape[2:]]
            lo = list(hi)
            hi[2 + ax] = slice(2, 2 + I.shape[2 + ax])
            lo[2 + ax] = slice(0, I.shape[2 + ax])
            out.append((P[tuple(hi)] - P[tuple(lo)]) / 2.0)
        return torch.stack(out, 0)

    ga, gb = grads(x), grads(y)
    ea, eb = (eta * g.detach().norm(dim=0).mean() for g in (ga, gb))
    s = (ga * gb).sum(0) ** 2 / (((ga ** 2).sum(0) + ea ** 2) * ((gb ** 2).sum(0) + eb ** 2))
    return (1.0 - s).mean()


def inputs(case, seed=900):
    """The two images of a case: test_mind.mind_inputs (seeded), or the related pair b = 1 - a^2 + 0.05 noise."""
    shape, _, _, related = case
    a, b = mind_inputs(shape, seed + 7 * SHAPES.index(shape))
    if related:
        b = (1.0 - a.double() ** 2 + 0.05 * C.rand(seed + 300, *shape).double()).float()
    return a, b


def rel_errors(loss, grads, loss64, grads64):
    """(relative error of the loss, worst relative 2-norm error of the gradients, worst max-abs over max)."""
    el = abs(float(loss) - loss64) / abs(loss64)
    l2 = mx = 0.0
    for g, g64 in zip(grads, grads64):
        g, g64 = g.detach().cpu().double(), g64.double()
        l2 = max(l2, float((g - g64).norm() / g64.norm()))
        mx = max(mx, float((g - g64).abs().max() / g64.abs().max()))
    return el, l2, mx


def field_error(f, f64):
    return float((f.detach().cpu().double() - f64).abs().max() / f64.abs().max())


_REF = {}


def reference(case):
    """(a, b, loss64, da64, db64) of a case, computed once and shared."""
    if case not in _REF:
        a, b = inputs(case)
        _REF[case] = (a, b) + gradfield_loss_ref(a, b, case[1], 1.0, case[2])
    return _REF[case]


def _gpu_loss(a, b, eps='auto', eta=1.0, spacing=None, mask=None, grad=(True, True)):
    from dfmir_amd import ops
    x, y = a.to(DEV).requires_grad_(grad[0]), b.to(DEV).requires_grad_(grad[1])
    loss = ops.gradfield_loss(x, y, eps, eta, spacing, mask=None if mask is None else mask.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), None if x.grad is None else x.grad.cpu(), None if y.grad is None else y.grad.cpu()


def _check(got, ref, what):
    el, l2, mx = rel_errors(got[0], got[1:], ref[0], ref[1:])
    print("%s: loss %.3e (bound %.1e)  grad l2 %.3e (%.1e)  grad max %.3e (%.1e)" % (what, el, B_LOSS, l2, B_L2, mx, B_MAX))
    assert all(bool(torch.isfinite(g).all()) for g in got[1:]), what
    assert el <= B_LOSS and l2 <= B_L2 and mx <= B_MAX, (what, el, l2, mx)


BIG = ((2, 1, 13, 17, 19), 'auto', None, False)


# ------------------------------------------------------------------------------------------ CPU tier
def test_gradfield_symbols_in_header_exports_and_ctypes_table():
    import dfmir_amd
    from dfmir_amd import _lib
    from tests.test_abi import header_symbols
    h = ctypes.CDLL(dfmir_amd.LIB_PATH)
    for s in ("dfmir_gradfield_ws_floats", "dfmir_gradfield_fwd", "dfmir_gradfield_bwd", "dfmir_gradfield_field"):
        assert s in header_symbols() and s in _lib.exported_symbols() and hasattr(h, s), s
    lib = dfmir_amd.lib()
    assert lib.dfmir_abi_version() == 14
    # two double slots per workgroup behind a head of four doubles; a workgroup owns an 8 x 64 tile of 16 planes, of 8 or 4
    # while that leaves fewer than 768 workgroups
    assert lib.dfmir_gradfield_ws_floats(3, 1, 256, 512, 512) == 2 * (4 + 2 * 16 * 64 * 8)
    assert lib.dfmir_gradfield_ws_floats(3, 1, 128, 128, 256) == 2 * (4 + 2 * 16 * 16 * 4)
    assert lib.dfmir_gradfield_ws_floats(3, 1, 8, 8, 8) == 2 * (4 + 2 * 2)
    assert lib.dfmir_gradfield_ws_floats(3, 2, 17, 9, 65) == 2 * (4 + 2 * 2 * 5 * 2 * 2)
    assert lib.dfmir_gradfield_ws_floats(2, 3, 1, 1, 1) == 2 * (4 + 2 * 3)
    assert lib.dfmir_gradfield_ws_floats(3, 1, 1, 20, 33) > 0
    for bad in ((4, 1, 8, 8, 8), (1, 1, 1, 1, 8), (2, 1, 2, 8, 8), (3, 0, 8, 8, 8), (3, 1, 8, 0, 8), (3, 1, 2048, 1024, 1024)):
        assert lib.dfmir_gradfield_ws_floats(*bad) == -1, bad


def test_gradfield_null_and_bad_arguments_are_invalid_without_a_device():
    import dfmir_amd
    lib = dfmir_amd.lib()
    one = ctypes.c_void_p(8)            # (a non-NULL, aligned pointer that is never dereferenced: every call is refused)
    assert lib.dfmir_gradfield_fwd(None, None, None, 3, 1, 8, 8, 8, 1.0, 1.0, 1.0, 1, 1.0, 0.0, 0.0, None, None, None) != 0
    assert b"invalid argument" in lib.dfmir_last_error()
    assert lib.dfmir_gradfield_bwd(None, None, None, None, None, None, None, 3, 1, 8, 8, 8, 1.0, 1.0, 1.0, None) != 0
    assert b"invalid argument" in lib.dfmir_last_error()
    assert lib.dfmir_gradfield_field(None, 3, 1, 8, 8, 8, 1.0, 1.0, 1.0, 1, 1.0, 0.0, None, None, None) != 0
    assert b"invalid argument" in lib.dfmir_last_error()
    for args in ((3, 1, 8, 8, 8, 1.0, 1.0, 0.0, 1, 1.0, 0.0, 0.0),             # a spacing of 0
                 (3, 1, 8, 8, 8, 1.0, 1.0, 1.0, 1, 0.0, 0.0, 0.0),             # auto with eta = 0
                 (3, 1, 8, 8, 8, 1.0, 1.0, 1.0, 0, 1.0, 0.1, -0.1),            # a negative eps
                 (3, 1, 8, 8, 8, 1.0, 1.0, 1.0, 0, 1.0, float('nan'), 0.1),
                 (2, 1, 2, 8, 8, 1.0, 1.0, 1.0, 1, 1.0, 0.0, 0.0)):            # nd = 2 with two planes
        assert lib.dfmir_gradfield_fwd(one, one, None, *args, one, one, None) != 0, args
        assert b"invalid argument" in lib.dfmir_last_error()
    assert lib.dfmir_gradfield_bwd(one, one, None, one, one, None, None, 3, 1, 8, 8, 8, 1.0, 1.0, 1.0, None) != 0   # no output
    assert b"invalid argument" in lib.dfmir_last_error()


def test_gradfield_rejects_bad_arguments_before_any_launch():
    from dfmir_amd import ops
    from dfmir_amd._lib import DfmirHipError
    from dfmir_amd.losses import GradField_Loss
    x = torch.rand(1, 1, 8, 8, 8)
    for bad in (0.0, -1.0, 'automatic', (0.1,), (0.1, 0.0), float('nan'), True):
        with pytest.raises(ValueError, match="eps"):
            GradField_Loss(eps=bad)
        with pytest.raises(ValueError, match="eps"):
            ops.gradfield_loss(x, x, eps=bad)
    with pytest.raises(ValueError, match="eps"):
        ops.gradfield_normals(x, eps=(0.1, 0.1))
    with pytest.raises(ValueError, match="eta"):
        GradField_Loss(eta=0.0)
    with pytest.raises(ValueError, match="eta"):
        ops.gradfield_loss(x, x, eta=-2.0)
    with pytest.raises(ValueError, match="spacing"):
        ops.gradfield_loss(x, x, spacing=(1.0, 1.0))
    with pytest.raises(ValueError, match="spacing"):
        ops.gradfield_loss(x, x, spacing=(1.0, 0.0, 1.0))
    with pytest.raises(ValueError, match="spacing"):
        GradField_Loss(dim=2, spacing=(1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="dim"):
        GradField_Loss(dim=4)
    with pytest.raises(ValueError, match="2-D images"):
        GradField_Loss(dim=3)(x[0], x[0])
    with pytest.raises(ValueError, match="single-channel"):
        GradField_Loss()(torch.rand(1, 2, 8, 8), torch.rand(1, 2, 8, 8))
    with pytest.raises(ValueError, match="dims"):
        ops.gradfield_normals(torch.rand(1, 1, 8))
    with pytest.raises(ValueError, match="differ in shape"):
        ops.gradfield_loss(x, torch.rand(1, 1, 8, 8, 9))
    with pytest.raises(DfmirHipError, match="fp32 tensors only"):
        ops.gradfield_loss(x.double(), x.double())
    with pytest.raises(DfmirHipError, match="fp32 tensors only"):
        ops.gradfield_normals(x.half())
    with pytest.raises(DfmirHipError, match="no CPU fallback"):
        GradField_Loss()(x, x)
    with pytest.raises(DfmirHipError, match="no CPU fallback"):
        ops.gradfield_normals(x)
    crit = GradField_Loss(eps=(0.1, 0.2), eta=2.0, dim=3, spacing=(2.0, 1.0, 1.0))
    assert crit.name == 'gradfield' and crit.eps == (0.1, 0.2) and crit.spacing == (2.0, 1.0, 1.0)


def test_registration3d_constructs_with_gradfield_and_still_rejects_unknown():
    from dfmir_amd.losses import GradField_Loss
    from dfmir_amd.registration3d import Registration3DModel
    m = Registration3DModel((8, 8, 8), device="cpu", similarity="gradfield", gradfield_eps=(0.1, 0.2), gradfield_eta=2.0,
                            spacing=(2.0, 1.0, 1.0))
    assert isinstance(m.criterionGradField, GradField_Loss)
    assert (m.criterionGradField.eps, m.criterionGradField.eta, m.criterionGradField.dim) == ((0.1, 0.2), 2.0, 3)
    assert m.criterionGradField.spacing == (2.0, 1.0, 1.0)
    assert 'loss_gradfield' in m._outputs
    m2 = Registration3DModel((8, 8), device="cpu", similarity="gradfield")
    assert m2.criterionGradField.dim == 2 and m2.criterionGradField.eps == 'auto'
    with pytest.raises(ValueError, match="'ncc', 'nmi' or 'mind'"):
        Registration3DModel((8, 8, 8), device="cpu", similarity="mi")
    with pytest.raises(ValueError, match="eps"):
        Registration3DModel((8, 8, 8), device="cpu", similarity="gradfield", gradfield_eps=0.0)


@pytest.mark.parametrize("shape", [(2, 1, 5, 6, 7), (1, 1, 1, 20, 33), (2, 1, 9, 11)], ids=["3d", "plane", "2d"])
def test_restatement_equals_autograd_of_the_textbook_formula(shape):
    a, b = inputs((shape, 'auto', None, False))
    loss, da, db = gradfield_loss_ref(a, b)
    assert 0.3 < loss < 1.0
    x, y = a.double().requires_grad_(), b.double().requires_grad_()
    tl = gradfield_textbook(x, y)
    tl.backward()
    assert abs(float(tl.detach()) - loss) <= 1e-13 * loss
    for g, t in ((da, x.grad), (db, y.grad)):
        assert float((g - t).abs().max()) <= 1e-13 * float(t.abs().max())


def test_restatement_is_contrast_invariant_with_auto_eps():
    a, b = inputs(BIG)
    loss, da, db = gradfield_loss_ref(a, b)
    l2, da2, db2 = gradfield_loss_ref(-3.0 * a.double() + 0.4, b)
    assert abs(l2 - loss) <= 1e-12 * loss
    assert float((da2 * -3.0 - da).abs().max()) <= 1e-12 * float(da.abs().max())
    assert float((db2 - db).abs().max()) <= 1e-12 * float(db.abs().max())
    # not so with a given eps
    assert abs(gradfield_loss_ref(-3.0 * a.double() + 0.4, b, EPS_PAIR)[0] - gradfield_loss_ref(a, b, EPS_PAIR)[0]) > 1e-3


def test_restatement_related_pair_has_large_similarity():
    """b = 1 - a^2 + 0.05 noise: inverted contrast, parallel edges.  With the small given eps the loss falls below 0.5 (the
    unrelated pairs of the same shapes: 0.75 and 0.70); 'auto' (eps = the mean edge strength) damps s to about a quarter on
    a typical edge, and the loss falls from 0.93 to 0.75."""
    for case in CASES:
        if case[3]:
            loss, unrelated = reference(case)[2], reference(case[:3] + (False,))[2]
            assert loss < (0.5 if case[1] == EPS_PAIR else 0.8) and loss < unrelated - 0.15, (_id(case), loss, unrelated)


def test_restatement_constant_image_gives_loss_one_and_zero_gradients():
    a, b = inputs(BIG)
    for const in (torch.full_like(a, 0.3), torch.zeros_like(a)):
        loss, da, db = gradfield_loss_ref(const, b)
        assert loss == 1.0
        assert bool(torch.isfinite(da).all()) and bool(torch.isfinite(db).all())
        assert float(da.abs().max()) == 0.0 and float(db.abs().max()) == 0.0
        assert float(field_ref(const.double()).abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ GPU tier
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_gradfield_loss_gradients_and_field_vs_restatement(case):
    from dfmir_amd import ops
    shape, eps, spacing, _ = case
    a, b, loss64, da64, db64 = reference(case)
    feps = eps if eps == 'auto' else eps[0]
    f = ops.gradfield_normals(a.to(DEV), feps, 1.0, spacing).cpu()
    f64 = field_ref(a.double(), feps, 1.0, spacing)
    assert f.shape == f64.shape and f.shape[1] == len(shape) - 2
    ef = field_error(f, f64)
    print("%s: field max %.3e (bound %.1e)" % (_id(case), ef, B_FIELD))
    assert bool(torch.isfinite(f).all()) and ef <= B_FIELD, ef
    _check(_gpu_loss(a, b, eps, 1.0, spacing), (loss64, da64, db64), _id(case))


@pytest.mark.gpu
@pytest.mark.parametrize("kind,shape", [("broadcast", (2, 1, 13, 17, 19)), ("binary", (2, 1, 13, 17, 19)),
                                        ("empty", (2, 1, 13, 17, 19)), ("broadcast", (1, 1, 17, 9, 68)),
                                        ("binary", (2, 1, 37, 41))])
def test_gradfield_mask(kind, shape):
    a, b = reference((shape, 'auto', None, False))[:2]
    if kind == "broadcast":
        mask = C.rand(77, *((1, 1) + shape[2:]))
    elif kind == "binary":
        mask = (C.rand(78, *shape) > 0.4).float()
    else:
        mask = torch.zeros(*shape)
    got = _gpu_loss(a, b, mask=mask)
    if kind == "empty":
        assert float(got[0]) == 0.0 and float(got[1].abs().max()) == 0.0 and float(got[2].abs().max()) == 0.0
        assert not bool(torch.isnan(got[1]).any()) and not bool(torch.isnan(got[2]).any())
        return
    _check(got, gradfield_loss_ref(a, b, mask=mask), "mask %s %s" % (kind, shape))


@pytest.mark.gpu
def test_gradfield_only_one_input_requires_grad():
    a, b = reference(BIG)[:2]
    both = _gpu_loss(a, b)
    la, ga, none_b = _gpu_loss(a, b, grad=(True, False))
    lb, none_a, gb = _gpu_loss(a, b, grad=(False, True))
    assert none_a is None and none_b is None
    assert torch.equal(la, both[0]) and torch.equal(lb, both[0])
    assert torch.equal(ga, both[1]) and torch.equal(gb, both[2])


@pytest.mark.gpu
def test_gradfield_contrast_invariance_through_the_kernels():
    """-3 a + 0.40625 with `a` rounded to multiples of 2^-10: the transform is exact in fp32, so the kernels see exactly the
    transformed image and the result is held to the restatement of the ORIGINAL pair with the bounds of every other case."""
    a, b = reference(BIG)[:2]
    a = (a * 1024.0).round() / 1024.0
    a2 = -3.0 * a + 0.40625
    assert torch.equal(a2.double(), -3.0 * a.double() + 0.40625)
    ref = gradfield_loss_ref(a, b)
    loss, da2, db2 = _gpu_loss(a2, b)
    _check((loss, da2.double() * -3.0, db2), ref, "contrast invariance")


@pytest.mark.gpu
def test_gradfield_swapping_the_images_with_their_eps_swaps_the_gradients():
    case = ((2, 1, 13, 17, 19), EPS_PAIR, None, False)
    a, b, loss64, da64, db64 = reference(case)
    lba, dba_b, dba_a = _gpu_loss(b, a, (EPS_PAIR[1], EPS_PAIR[0]))
    _check((lba, dba_a, dba_b), (loss64, da64, db64), "swapped")


@pytest.mark.gpu
def test_gradfield_constant_image():
    from dfmir_amd import ops
    a, b = reference(BIG)[:2]
    const = torch.full_like(a, 0.3)
    for pair in ((const, b), (b, const), (const, const)):
        loss, g0, g1 = _gpu_loss(*pair)
        assert float(loss) == 1.0
        for g in (g0, g1):
            assert bool(torch.isfinite(g).all()) and float(g.abs().max()) == 0.0
    f = ops.gradfield_normals(const.to(DEV)).cpu()
    assert bool(torch.isfinite(f).all()) and float(f.abs().max()) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 1, 13, 17, 19), (1, 1, 17, 9, 68), (2, 1, 37, 41)], ids=["3d", "3d-vec", "2d"])
def test_gradfield_bit_reproducible(shape):
    from dfmir_amd import ops
    a, b = reference((shape, 'auto', None, False))[:2]
    r0, r1 = _gpu_loss(a, b), _gpu_loss(a, b)
    for x, y in zip(r0, r1):
        assert torch.equal(x, y)
    assert torch.equal(ops.gradfield_normals(a.to(DEV)), ops.gradfield_normals(a.to(DEV)))


def _step_model(capture, **kw):
    from tests import step3d
    return step3d.step_model((16, 16, 16), 'gradfield', capture=capture, **kw)


@pytest.mark.gpu
def test_registration3d_gradfield_step_matches_restatement():
    m, A, B = _step_model(False)
    m.set_input({"A": A, "B": B})
    m.optimize_parameters()
    torch.cuda.synchronize()
    got = m.get_current_losses()
    assert sorted(got) == ["grad", "gradfield"]
    ref = gradfield_loss_ref(m.regA, m.real_B)[0]
    err = abs(got["gradfield"] - ref) / abs(ref)
    print("step loss_gradfield: %.3e (bound %.1e)" % (err, B_LOSS))
    assert err <= B_LOSS
    assert float(m.optimizer_R.flat_g.abs().max()) > 0.0


@pytest.mark.gpu
def test_registration3d_gradfield_symmetric_step_is_the_mean_of_both_directions():
    m, A, B = _step_model(False, symmetric=True)
    m.set_input({"A": A, "B": B})
    m.optimize_parameters()
    torch.cuda.synchronize()
    got = m.get_current_losses()["gradfield"]
    ref = 0.5 * (gradfield_loss_ref(m.regA, m.real_B)[0] + gradfield_loss_ref(m.regB, m.real_A)[0])
    err = abs(got - ref) / abs(ref)
    print("symmetric step loss_gradfield: %.3e (bound %.1e)" % (err, B_LOSS))
    assert err <= B_LOSS


@pytest.mark.gpu
def test_registration3d_gradfield_captured_step_matches_eager():
    """similarity='gradfield' under capture_step=True: a replayed step equals the same step enqueued eagerly."""
    from tests import step3d
    m, A, B = _step_model(True)
    m.parallelize()
    step3d.assert_replay_matches_eager(m, {"A": A, "B": B}, ["grad", "gradfield"])
