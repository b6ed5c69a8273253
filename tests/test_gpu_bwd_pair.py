"""GPU: the backward of a 2-D 3x3 layer as ONE launch (dfmir_conv3x3_bwd_pair, csrc/conv3x3s.hip conv3x3_bwd_pair_k) against the
same backward as two launches (DFMIR_NO_BWD_PAIR=1) on the same inputs.

Every case first asserts through ops.last_backward_paired() that the pair was really taken: a silent fallback fails the test.
The shapes are the smallest the library still routes to the kernels the pair carries.  Its conditions (conv3x3s.hip: cs_plan,
split_fwd_geom_ok, ws_setup): the data gradient needs > 32 produced and >= 16 reduced channels and a spatial size that fills
>= 85 % of its 8 x 32 (more than 64 produced channels) or 16 x 32 tiles; the weight gradient needs >= 64 channels on both
sides, H even and W a multiple of 16.

  case 1   64 -> 128, zero pad, N = 2, 16 x 32.  Data gradient: 64 produced channels = the 16 x 32 tile form, short K (128 = 8
           chunks), two tiles (nb & 7 != 0: plain grid, no XCD mapping).  Weight gradient: 128 output channels = the plain role
           assignment, 4 pixel splits per (ci, co) tile.
  case 2   128 -> 64, zero pad, N = 8, 16 x 32.  Data gradient: 128 produced channels = the 8 x 32 tile form, 16 tiles
           (nb & 7 == 0: the 1-D XCD-mapped grid, the one whose index offsets must stay multiples of 8).  Weight gradient: 64
           output channels under 128 input channels = the swapped-roles form with its transposed store, db from the X operand.
  case 3   256 -> 256, reflect pad, N = 2, 8 x 32, with a skip gradient.  Data gradient: two cout slices on a 2-D grid, the
           ring fold and `res` in its epilogue.  Weight gradient: db, 2 pixel splits.
  case 4   128 -> 128, zero pad, N = 1, 8 x 32.  runs_total = 8 = one pixel split per (ci, co) tile: one atomic add per
           gradient element, so dW must be BIT-equal as well (db: see test_case4_bias_gradient_is_bit_equal).

Bounds.  dX (with the skip gradient and the ring folded in) is bit-equal in every case and order.  dW / db of cases 1-3 (a) meet
the bound of the existing split parity test against float64, tests/test_gpu_ops.py::test_conv3x3_split_dynamic_range -- max
error <= 2e-5 of the reference's largest magnitude, reference = torch's float64 convolution on the CPU (tests/ref64.py holds no
convolution), inputs made the way that test makes them: C.randn tensors, the weights divided by 24 -- and (b) differ from a
two-launch result by no more than twice what two-launch runs differ from each other on these inputs (measured here: the
largest difference between any two of four two-launch runs).
"""
import pytest
import torch
import torch.nn.functional as F

from tests.golden import common as C

pytestmark = pytest.mark.gpu

DEV = "cuda"

CASES = {
    # name: (Cin, Cout, reflect, N, H, W, skip gradient, dW / db bit-equal)
    "c1_64to128_zero": (64, 128, False, 2, 16, 32, False, False),
    "c2_128to64_zero_swap": (128, 64, False, 8, 16, 32, False, False),
    "c3_256to256_reflect_skip": (256, 256, True, 2, 8, 32, True, False),
    "c4_128to128_one_split": (128, 128, False, 1, 8, 32, False, True),
}
ORDERS = (0, 1, 2)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dfmir_amd import ops as _ops
    return _ops


def _set(**kv):
    from dfmir_amd import _lib
    for k, v in kv.items():
        _lib.set_option(k, v)


@pytest.fixture(autouse=True)
def _options_restored():
    yield
    _set(DFMIR_NO_BWD_PAIR=None, DFMIR_BWD_PAIR=None, DFMIR_BWD_PAIR_ORDER=None)


def _inputs(name):
    Cin, Cout, reflect, N, H, W, skip, _ = CASES[name]
    seed = 900 + 10 * list(CASES).index(name)
    x = C.randn(seed, N, Cin, H, W)
    w = C.randn(seed + 1, Cout, Cin, 3, 3) / 24.0
    b = C.randn(seed + 2, Cout) * 0.1
    cot = C.randn(seed + 3, N, Cout, H, W)
    cskip = C.randn(seed + 4, N, Cin, H, W) if skip else None
    return x, w, b, cot, cskip


def _backward(ops, name, inp):
    """One forward + backward of the layer through ops.conv; (dx, dw, db, paired)."""
    _, _, reflect, _, _, _, skip, _ = CASES[name]
    x, w, b, cot, cskip = inp
    xg, wg, bg = (t.clone().to(DEV).requires_grad_() for t in (x, w, b))
    out = ops.conv(xg, wg, bg, None, 1, 1, 1 if reflect else 0, 0, 0.0, skip=skip)
    loss = ((out[0] * cot.to(DEV)).sum() + (out[1] * cskip.to(DEV)).sum()) if skip else (out * cot.to(DEV)).sum()
    loss.backward()
    paired = ops.last_backward_paired()
    torch.cuda.synchronize()
    return xg.grad.detach(), wg.grad.detach(), bg.grad.detach(), paired


def _ref64(name, inp):
    _, _, reflect, _, _, _, skip, _ = CASES[name]
    x, w, b, cot, cskip = inp
    xd, wd, bd = (t.double().requires_grad_() for t in (x, w, b))
    y = F.conv2d(F.pad(xd, (1, 1, 1, 1), mode="reflect"), wd, bd) if reflect else F.conv2d(xd, wd, bd, padding=1)
    loss = (y * cot.double()).sum() + ((xd * cskip.double()).sum() if skip else 0.0)
    loss.backward()
    return xd.grad, wd.grad, bd.grad


_RUNS = {}


def _runs(ops, name):
    """Per case, computed once and shared: the inputs, the float64 reference, four two-launch backwards and the pair in each
    of the three orders."""
    if name not in _RUNS:
        inp = _inputs(name)
        r = {"ref": _ref64(name, inp), "two": [], "pair": {}}
        _set(DFMIR_NO_BWD_PAIR="1")
        for _ in range(4):
            r["two"].append(_backward(ops, name, inp))
        _set(DFMIR_NO_BWD_PAIR=None, DFMIR_BWD_PAIR="1")
        for o in ORDERS:
            _set(DFMIR_BWD_PAIR_ORDER=str(o))
            r["pair"][o] = _backward(ops, name, inp)
        _set(DFMIR_BWD_PAIR=None, DFMIR_BWD_PAIR_ORDER=None)
        _RUNS[name] = r
    return _RUNS[name]


def _maxdiff(a, b):
    return float((a.double() - b.double()).abs().max())


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", list(CASES))
def test_pair_equals_two_launches(ops, name, order):
    r = _runs(ops, name)
    for run in r["two"]:
        assert not run[3], "DFMIR_NO_BWD_PAIR=1 must give two launches"
    dx, dw, db, paired = r["pair"][order]
    assert paired, "%s: the backward did not take the pair kernel (silent fallback)" % name
    dx2, dw2, db2, _ = r["two"][0]
    assert torch.equal(dx, dx2), "%s order %d: dX differs from the two-launch dX by %.3e" % (name, order, _maxdiff(dx, dx2))
    if CASES[name][7]:
        print("%s order %d: dW vs two launches %.3e" % (name, order, _maxdiff(dw, dw2)))
        assert torch.equal(dw, dw2), "dW differs by %.3e with one atomic add per element" % _maxdiff(dw, dw2)
        return                                                   # db of this case: test_case4_bias_gradient_is_bit_equal
    _, dw64, db64 = r["ref"]
    for got, two, ref, what in ((dw, 1, dw64, "dW"), (db, 2, db64, "db")):
        scale = float(ref.abs().max())
        err = _maxdiff(got.cpu(), ref)
        spread = max(_maxdiff(r["two"][i][two], r["two"][j][two]) for i in range(4) for j in range(i))
        d = _maxdiff(got, r["two"][0][two])
        print("%s order %d %s: err vs fp64 %.3e (bound %.3e), vs two launches %.3e (two-launch spread %.3e)"
              % (name, order, what, err, 2e-5 * scale, d, spread))
        assert torch.isfinite(got).all(), what
        assert err <= 2e-5 * scale, "%s: max err %.3e vs scale %.3e" % (what, err, scale)
        assert d <= 2.0 * spread, "%s: differs from the two-launch result by %.3e, two-launch runs by %.3e" % (what, d, spread)


@pytest.mark.parametrize("order", ORDERS)
def test_case4_bias_gradient_is_bit_equal(ops, order):
    """Case 4, db: one workgroup owns each output channel and its single global add lands on zeros, so db is bit-equal as
    well.  (That needs the in-workgroup part of the sum to be order-stable: conv3x3_wgrad_split2_k used to add a channel's four
    per-thread partial sums with LDS atomics in arrival order, and four two-launch runs then differed from EACH OTHER by up to
    3.815e-06, 1-2 ulp of |db| ~ 30; they now meet in a fixed order.)"""
    name = "c4_128to128_one_split"
    r = _runs(ops, name)
    db, paired = r["pair"][order][2], r["pair"][order][3]
    assert paired
    db2 = r["two"][0][2]
    spread = max(_maxdiff(r["two"][i][2], r["two"][j][2]) for i in range(4) for j in range(i))
    print("%s order %d: db vs two launches %.3e (two-launch runs among themselves: %.3e)" % (name, order, _maxdiff(db, db2), spread))
    assert torch.equal(db, db2), "db differs by %.3e (two-launch runs among themselves: %.3e)" % (_maxdiff(db, db2), spread)


def test_deterministic_mode_is_not_paired(ops):
    name = "c1_64to128_zero"
    inp = _inputs(name)
    _set(DFMIR_BWD_PAIR="1")
    ops.set_deterministic_wgrad(True)
    try:
        dx, dw, db, paired = _backward(ops, name, inp)
        _set(DFMIR_NO_BWD_PAIR="1")
        dx2, dw2, db2, paired2 = _backward(ops, name, inp)
    finally:
        ops.set_deterministic_wgrad(False)
    assert not paired and not paired2
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2) and torch.equal(db, db2)
    assert torch.equal(dx, _runs(ops, name)["two"][0][0])


def test_conv_profiler_keeps_the_launches_separate(ops):
    name = "c3_256to256_reflect_skip"
    inp = _inputs(name)
    kinds = []

    def prof(kind, flops, launch):
        kinds.append(kind)
        launch()

    _set(DFMIR_BWD_PAIR="1")
    ops.set_conv_profiler(prof)
    try:
        dx, dw, db, paired = _backward(ops, name, inp)
    finally:
        ops.set_conv_profiler(None)
    assert not paired
    assert "conv3x3_L" in kinds and "wgrad3x3_L" in kinds, kinds        # forward + dgrad, and the weight gradient, each timed
    r = _runs(ops, name)
    assert torch.equal(dx, r["two"][0][0])
    _, dw64, db64 = r["ref"]
    assert _maxdiff(dw.cpu(), dw64) <= 2e-5 * float(dw64.abs().max())
    assert _maxdiff(db.cpu(), db64) <= 2e-5 * float(db64.abs().max())
