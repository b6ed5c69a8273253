"""Every weight- and bias-gradient kernel, in both accumulation modes (fp32 atomics | ops.set_deterministic_wgrad: 64-bit fixed
point, include/dfmir_hip.h "Deterministic weight gradients"), against the float64 restatements conv_weight_grad /
conv_bias_grad of tests/ref64.py (checked on the CPU by tests/test_ref64.py).  Run on the MI355X box:
python -m pytest tests/test_gpu_wgrad_fp64.py -m gpu -q ; the tests without the gpu mark admit the cases (yardstick, fixed-point
grid, planned kernel) and run anywhere.  Cases, inputs and CPU evaluators: tests/wgrad_cases.py, shared with
scripts/wgrad_margins.py.

Launch site (every line of `grep df_acc\\|df_det_fx csrc/`) -> test id, with the condition of the source that the shape meets.
All ids are test_wgrad_branch[<mode>-<id>] unless another test is named; <mode> = atomic | deterministic.
  conv.hip  conv_wgrad_impl, after df_conv3x3_split_wgrad_try, df_conv3x3_wgrad_try, df_conv3x3_small_wgrad_try, df_conv3d_wgrad_try
    conv_wgrad_mfma_k<2,2,2,2,16>  Cout > 64       mfma-c136: 130 -> 136 at 7 x 9 (H W = 63 is no multiple of 32, which the LDS
                                                   kernel needs; at 8 x 8 that kernel takes the layer)
    conv_wgrad_mfma_k<4,1,1,2,16>  32 < Cout <= 64 mfma-c40: 8 -> 40 at 9 x 13 (Cout < 64: not the LDS kernel; > 16: not the small one)
    conv_wgrad_mfma_k<4,1,1,1,32>  Cout <= 32      mfma-c16-reflect: 16 -> 16 at 12 x 20 x 2 (4 tiles < 32: the small-channel kernel
                                                   refuses), mfma-c32-stride2; with three-deep taps: c3d-generic-w17 (40 -> 12 at
                                                   6 x 7 x 17: W % 4 != 0 refuses both 3-D kernels), 1x1-refused
    conv1x1_wgrad_k                                1x1-72to49 (three images, last chunk 32 of 64), 1x1-8to136 (two chunks);
                                                   refusal under DFMIR_NO_1X1_WGRAD: 1x1-refused
    bias_grad_k, 64 threads (S < 4096)             test_bias_grad[*-b64-scalar] (S % 4 != 0), [*-b64-quad]; and db of every case below
    bias_grad_k, 256 threads (S >= 4096)           test_bias_grad[*-b256-quad] (S = 4096), [*-b256-scalar]
    bias_grad_k, nsplit = 2                        test_bias_grad[*-bsplit2-quad] (S = 65540), [*-bsplit2-scalar] (65541)
    the 2 GiB batch split of conv_wgrad_impl       unreachable at test size (a tensor of 2^31 bytes)
  conv3x3.hip
    conv3x3_wgrad_k<2,2>  64 <= Cout < 128         lds-40to64 (no probes, Cin >= 32, H W % 32 == 0, W = 32)
    conv3x3_wgrad_k<1,4>  Cout >= 128              lds-40to128-narrow (W = 16 < 32 divides 32; reflect)
    conv3x3_small_wgrad_k                          small-34to16 (44 x 70 x 2: 36 tiles >= 32, ragged rows and columns), small-16to2,
                                                   small-48to12-reflect
  conv3x3s.hip  ws_setup's `which` (probes given; H even, W % 16 == 0, Cin, Cout >= 64)
    1  conv3x3_wgrad_split2_k, swapped roles       s1-swap-160to64 (Cout == 64 < Cin, zero padding); body: conv3x3s_w2_body.inc:270
    2  conv3x3_wgrad_split2_k                      s2-64to128, s2-64to128-pmax, s2-72to136-reflect-pmax; conv3x3s_w2_body.inc:283
    3  conv3x3_wgrad_split_k<2,64>                 s3-64to64, s3-160to64-reflect-pmax (reflect: no swap); conv3x3s.hip:1079
    4  conv3x3_wgrad_split_k<3,128>                s4-bf16-64to128 (DFMIR_CONV_SPLIT=b)
    5  conv3x3_wgrad_split_k<3,64>                 s5-bf16-72to64-pmax
    with / without dy_pmax                         the -pmax cases / the others (the swapped form drops dy_pmax)
  taps.hip
    conv7x7_c1_wgrad_k, dW (:358) and db (:359)    test_stem7_backward[*] through ops.conv_taps -> Stem7Fn (its only caller); the
                                                   db site runs in the default mode only, Stem7Fn hands it NULL in the other
  conv3d.hip  df_conv3d_wgrad_try (no probes, Cout <= 32, W % 4 == 0)
    conv3d_wgrad16_k<2,8>                          c3d-34to32 (two channel groups of 17)
    conv3d_wgrad16_k<1,14>                         c3d-32to12 (one group of 32 channels: 54 row tiles, Cout <= 16)
    conv3d_wgrad16_k<1,8>                          c3d-18to16 (31 row tiles; batch 2, ragged columns)
    conv3d_wgrad16_k<2,14>                         c3d-32to32
  conv3dsw.hip  conv3d_split_wgrad_impl (probes; 8 <= Cin <= 128, W % 4 == 0)
    conv3d_wgrad_tr_k<.,false,false>  32 rows      sw-34to32 (5 chunks: two workgroup rows)
    conv3d_wgrad_tr_k<2,true,false>   plane pairs  sw-pair-40to12 (6 x 7 x 16; at W = 17 the layer is c3d-generic-w17)
    swapped roles (Cout < 8)                       sw-swapped-16to3 (756 voxels < 1024: not the flow-head kernel)
    <.,false,true> up-cat operand                  sw-upcat-16+2to32, test_upcat_conv3d_backward[*]
    <.,true,true> up-cat operand, plane pairs      sw-upcat-8+3to16-pair (batch 2)
  conv3dwm.hip  conv3d_wgrad_march_k               wm-march (32 -> 16, 5 x 27 x 36 = 4860 voxels >= 4096; ragged columns)
  conv3duw.hip  df_conv3d_upwgrad_launch (ops._UPWGRAD_MIN_VOX at 0: the parity-class kernels at a test-sized volume)
    conv3d_upwgrad4_k<false> (:690)                uw-4wave-32+16to32 (its 16 skip channels go through the conv3dsw.hip rows form)
    conv3d_upwgrad4_k<true>, skip pair (:690, :699) uw-fused-32+2to32 (batch 2; db rides in it in the default mode only)
    conv3d_upwgrad_k, two waves per SIMD (:287)    uw-8wave-32+16to32 (DFMIR_UPWGRAD_8WAVE)
    conv3d_upwgrad_fold_k / _foldb_k               all three (integer adds in deterministic mode)
  conv3dt.hip
    conv3d_s2c2_wgrad_k (:409)                     t-s2c2-2to16
    conv3d_flow_wgrad_k (:590, db :598)            t-flow-16to2 (Cin 16, Cout <= 4, 2 x 1024 voxels)
  conv3ds2.hip  conv3d_s2_wgrad_k (:412, db :424)  s2m-16to32 (15 x 17 x 21 -> 792 output voxels > 512; at 9 x 11 x 13 the layer is
                                                   below S2_MIN_VOX and generic), test_conv_backward_end_to_end[*-s2m-16to32]
  losses.hip  det_scale_k, det_final_k             every deterministic id; the scale rule: test_wgrad_edges[deterministic-*]
  ops.py glue: conv_wgrad_raw (out=, db with dW, db = None to fused kernels): every test_wgrad_branch[deterministic-*];
    bias_grad: test_bias_grad; Stem7Fn.backward: test_stem7_backward; ConvFn / UpCatConv3dFn: the two end-to-end tests

Tolerances.  No number comes from the kernels under test, and deterministic mode has no allowance of its own.
  kind fp32 (the kernel multiplies in fp32): FACTOR = 4 x FP32_YARD, the larger error of the two fp32 CPU evaluation orders of
  the restatement against float64 on these inputs, maximum per family (2-D dW, 3-D dW, db) and metric; measured by
  scripts/wgrad_margins.py into profiles/wgrad_margins.txt (the rule of tests/test_compose.py: room for another summation
  order, not for a dropped term).
  kind split (fp16 / bf16 pairs): the figures the project asserts for them -- 1e-5 per output channel (SPLIT_L2) and 2e-5 of the
  maximum (SPLIT_MAX); on the dynamic-range edges 2e-5 of the maximum alone; on the channel spread without per-plane maxima
  the documented degradation (2e-4 per channel, 2e-6 on the larger half).
  Admission (CPU, test_case_admission): per case the yardstick stays within the family constant and the float64 reference put
  onto the documented fixed-point grid stays within a quarter of the bound.
All comparisons go to tests.test_gpu_ops.MARGINS.

The fixed-point scale.  Before this module the scale came from the fp32 product count * max(max|x|, 1) * max|dy|
(tests/wgrad_cases.py det_shifts(rule="product")).  test_the_product_rule_fails_admission keeps on the CPU what that did:
small_x (x ~ 1e-20) quantises every weight gradient to zero (relative error 1), big_bound (x ~ 1e19, dy ~ 1e16; the bound
overflows fp32, the result ~ 1e36 does not) overflows the 64-bit slots.  The GPU run on the earlier library measured the
same (profiles/wgrad_margins.txt, "before"); with the rule of include/dfmir_hip.h both meet the bounds of the default mode."""
import contextlib
import ctypes
import os

import pytest
import torch

from tests import wgrad_cases as WC
from tests.test_gpu_ops import MARGINS
from tests.wgrad_cases import BIAS_CASES, BY_ID, CASES, DYNAMIC_RANGE, EDGE_RUNS, STEM7

DEV = "cuda"
FACTOR = 4.0
# profiles/wgrad_margins.txt, rows "max": (largest per-output-channel relative 2-norm, max-abs over max) of the fp32 CPU restatement
FP32_YARD = {"2d": (4.69e-07, 6.44e-07), "3d": (3.30e-07, 6.30e-07), "bias": (9.14e-07, 9.14e-07)}
SPLIT_L2, SPLIT_MAX = 1e-5, 2e-5
SPREAD_L2_ALL, SPREAD_L2_LARGER_HALF = 2e-4, 2e-6
MODES = ("atomic", "deterministic")
gpu = pytest.mark.gpu


def bounds(c, what, edge=None):
    """(bound on the largest per-channel relative 2-norm error or None = not asserted, bound on max-abs over max)."""
    if c["kind"] == "fp32":
        y = FP32_YARD["bias" if what == "db" else "%dd" % c["nd"]]
        return FACTOR * y[0], FACTOR * y[1]
    if edge in DYNAMIC_RANGE:
        return None, SPLIT_MAX
    if edge == "spread" and not c["pmax"] and what == "dW":
        return SPREAD_L2_ALL, SPLIT_MAX
    return SPLIT_L2, SPLIT_MAX


def _test_id():
    return os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]


def check(mode, key, what, got, ref, bnd):
    """Record, print (DFMIR_WGRAD_PRINT=1: the lines scripts/wgrad_margins.py --measured reads) and assert both metrics."""
    l2, mx = WC.rel_errors(got, ref)
    if os.environ.get("DFMIR_WGRAD_PRINT"):
        print("WGRAD %s %s %s l2=%.3e max=%.3e bounds %s %.3e" % (mode, key, what, l2, mx, bnd[0], bnd[1]), flush=True)
    if bnd[0] is not None:
        MARGINS.append((_test_id(), what + " per-channel 2-norm", l2, bnd[0]))
    MARGINS.append((_test_id(), what + " max over max", mx, bnd[1]))
    assert (bnd[0] is None or l2 <= bnd[0]) and mx <= bnd[1], \
        "%s %s %s: per-channel 2-norm %.3e (bound %s), max over max %.3e (bound %.3e)" % (mode, key, what, l2, bnd[0], mx, bnd[1])


# ------------------------------------------------------------------------------------------------ CPU: admission
def _geom(c):
    from dfmir_amd.ops import DfConvGeom
    K3, p3, sp3, out3 = WC.geometry(c)
    return DfConvGeom(c["N"], c["Cin"], c["Cout"], *sp3, *out3, *K3, c["stride"], 1, *p3, 1 if c["reflect"] else 0, 0, 0.0)


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_planned_kernel(c):
    """ops._plan_conv_wgrad (host code only) answers what the table says, and the library's own predicates agree."""
    from dfmir_amd import ops
    g = _geom(c)
    parts = None
    if c["parts"]:
        _, _, sp3, _ = WC.geometry(c)
        parts = (torch.zeros(1, c["parts"], *(n // 2 for n in sp3)), torch.zeros(1, c["Cin"] - c["parts"], *sp3))
    old = ops._UPWGRAD_MIN_VOX
    ops._UPWGRAD_MIN_VOX = 0 if c["upw"] else old
    try:
        assert ops._plan_conv_wgrad(g, WC.geometry(c)[0], c["probes"], parts) == c["plan"]
    finally:
        ops._UPWGRAD_MIN_VOX = old
    if c["id"] == "wm-march":
        assert ops.lib().dfmir_conv3d_wgrad_is_march(ctypes.byref(g)) == 1
    if c["id"] in ("sw-34to32", "sw-pair-40to12", "c3d-generic-w17"):
        assert ops.lib().dfmir_conv3d_wgrad_is_march(ctypes.byref(g)) == 0


ADMIT = [(c["id"], None) for c in CASES] + [(STEM7["id"], None)] + EDGE_RUNS


def _case(cid):
    return STEM7 if cid == STEM7["id"] else BY_ID[cid]


def _grid_errors(c, x, dy, ref, rule):
    sw, sb = WC.det_shifts(WC.count(c), WC.operand_max(x), float(dy.abs().max()), rule)
    return (WC.rel_errors(WC.quantise(ref[0], sw), ref[0]), WC.rel_errors(WC.quantise(ref[1], sb).view(-1, 1), ref[1].view(-1, 1)))


@pytest.mark.parametrize("cid,edge", ADMIT, ids=["%s-%s" % (a, e) if e else a for a, e in ADMIT])
def test_case_admission(cid, edge):
    """The yardstick of the case stays within its family constant (fp32 kinds), and the float64 reference alone, rounded onto
    the fixed-point grid of include/dfmir_hip.h and to fp32, within a quarter of each bound."""
    c = _case(cid)
    x, dy = WC.inputs(c, edge)
    ref = WC.reference(c, x, dy)
    assert float(ref[0].abs().max()) < WC.FP32_MAX and float(ref[1].abs().max()) < WC.FP32_MAX
    if edge == "big_bound":
        assert WC.count(c) * WC.operand_max(x) * float(dy.abs().max()) > WC.FP32_MAX
    if edge in ("zero_input", "zero_dy"):
        gw, gb = _grid_errors(c, x, dy, ref, "documented")
        assert gw == (0.0, 0.0) and float(ref[0].abs().max()) == 0.0
        assert gb == (0.0, 0.0) or edge == "zero_input"
        return
    if c["kind"] == "fp32":
        ew, eb, _ = WC.yardstick(c, x, dy, ref)
        for e, fam in ((ew, "%dd" % c["nd"]), (eb, "bias")):
            assert e[0] <= FP32_YARD[fam][0] * 1.005 and e[1] <= FP32_YARD[fam][1] * 1.005, (fam, e)   # (the constants carry 3 digits)
    gw, gb = _grid_errors(c, x, dy, ref, "documented")
    for g_, what in ((gw, "dW"), (gb, "db")):
        b = bounds(c, what, edge)
        assert (b[0] is None or g_[0] <= b[0] / 4) and g_[1] <= b[1] / 4, (what, g_, b)


BIAS_SCALES = [(g, "%g" % g) for g in WC.BIAS_SCALES + (0.0,)]


@pytest.mark.parametrize("bid,N,Cc,S", BIAS_CASES, ids=[b[0] for b in BIAS_CASES])
@pytest.mark.parametrize("gs", [g for g, _ in BIAS_SCALES if g], ids=[i for g, i in BIAS_SCALES if g])
def test_bias_case_admission(gs, bid, N, Cc, S):
    """The same for the bias cases: ops.bias_grad hands dy over as both operands, the db slots take the scale of count * max|dy|."""
    dy = WC.bias_input(N, Cc, S, gs)
    ref = WC.R.conv_bias_grad(dy).view(-1, 1)
    e = (0.0, 0.0)
    for o in WC.ORDERS:
        e = tuple(max(p, q) for p, q in zip(e, WC.rel_errors(WC.R.conv_bias_grad(dy, WC.F32, o).view(-1, 1), ref)))
    assert e[0] <= FP32_YARD["bias"][0] * 1.005 and e[1] <= FP32_YARD["bias"][1] * 1.005, e
    ay = float(dy.abs().max())
    g_ = WC.rel_errors(WC.quantise(ref, WC.det_shifts(N * S, ay, ay)[1]), ref)
    assert g_[0] <= FACTOR * FP32_YARD["bias"][0] / 4 and g_[1] <= FACTOR * FP32_YARD["bias"][1] / 4, g_
    if gs == 1e30:       # the earlier rule squared max|dy| into the bound, which overflowed: every sum past its slot
        assert WC.rel_errors(WC.quantise(ref, WC.det_shifts(N * S, ay, ay, "product")[1]), ref)[1] >= 1.0


@pytest.mark.parametrize("host,edge", [(h, e) for h, e in EDGE_RUNS if e in ("small_x", "big_bound")])
def test_the_product_rule_fails_admission(host, edge):
    """What the scale count * max(max|x|, 1) * max|dy|, formed in fp32, does to the two cases: not admitted (see the module
    docstring) -- the reason the scale is built from the factors' exponents, without the floor."""
    c = BY_ID[host]
    x, dy = WC.inputs(c, edge)
    gw, _ = _grid_errors(c, x, dy, WC.reference(c, x, dy), "product")
    assert gw[1] > bounds(c, "dW", edge)[1], gw
    assert gw[1] >= 1.0                                  # every weight gradient zero (small_x) or past the slot (big_bound)


# ------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dfmir_amd import ops as _ops
    return _ops


@contextlib.contextmanager
def scope(ops, mode, c=None):
    """The accumulation mode, the case's library options and the parity-class threshold, all restored on the way out."""
    from dfmir_amd._lib import set_option
    was, was_vox = ops.deterministic_wgrad(), ops._UPWGRAD_MIN_VOX
    ops.set_deterministic_wgrad(mode == "deterministic")
    try:
        if c is not None:
            for k, v in c["opts"]:
                set_option(k, v)
            if c["upw"]:
                ops._UPWGRAD_MIN_VOX = 0
        yield
    finally:
        ops.set_deterministic_wgrad(was)
        ops._UPWGRAD_MIN_VOX = was_vox
        if c is not None:
            for k, _ in c["opts"]:
                set_option(k, None)


class Raw(object):
    """One case on the device: operands, probes where the path takes them, and the call through ops.conv_wgrad_raw."""

    def __init__(self, ops, c, x, dy):
        self.ops, self.c = ops, c
        self.parts = tuple(t.to(DEV) for t in x) if c["parts"] else None
        self.x = None if c["parts"] else x.to(DEV)
        self.dy = dy.to(DEV)
        self.xa = self.da = self.pm = None
        if c["probes"]:
            ops_in = torch.cat([t.flatten() for t in self.parts]) if c["parts"] else self.x
            self.xa, self.da = ops.absmax(ops_in).clone(), ops.absmax(self.dy).clone()
        if c["pmax"]:
            self.pm = self.dy.abs().amax(dim=(2, 3, 4)).contiguous()              # [N, Cout] plane maxima
        self.K3, self.p3, _, _ = WC.geometry(c)
        self.shape = (c["Cout"], c["Cin"]) + self.K3

    def __call__(self, out=None, db=None):
        c, ops = self.c, self.ops
        db = torch.zeros(c["Cout"], device=DEV) if db is None else db
        dwt = ops.conv_wgrad_raw(self.x, self.dy, self.K3, c["stride"], self.p3, 1 if c["reflect"] else 0, out=out, x_amax=self.xa,
                                 dy_amax=self.da, db=db, dy_pmax=self.pm, parts=self.parts)
        return dwt, ops.weight_unpack(dwt, self.shape), db


def _deterministic_properties(run, dwt, db):
    """Deterministic mode: a second run is bit-identical; out= / db onto pre-filled buffers = the buffers + a fresh result, to
    the rounding of one fp32 add."""
    dwt2, _, db2 = run()
    assert torch.equal(dwt, dwt2) and torch.equal(db, db2), "two deterministic runs differ"
    g = torch.Generator().manual_seed(77)
    scale_w, scale_b = float(dwt.abs().max()), float(db.abs().max())
    pre_w = (torch.randn(dwt.shape, generator=g) * scale_w).to(DEV)
    pre_b = (torch.randn(db.shape, generator=g) * scale_b).to(DEV)
    acc_w, _, acc_b = run(out=pre_w.clone(), db=pre_b.clone())
    for acc, pre, fresh, what in ((acc_w, pre_w, dwt, "out="), (acc_b, pre_b, db, "db")):
        want = pre.double() + fresh.double()
        tol = 2.0 ** -24 * want.abs() + 1e-45                                     # half an ulp of the sum
        assert bool(((acc.double() - want).abs() <= tol * 1.0000001).all()), "%s does not accumulate" % what


@gpu
@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
@pytest.mark.parametrize("mode", MODES)
def test_wgrad_branch(ops, mode, c):
    x, dy = WC.inputs(c)
    ref = WC.reference(c, x, dy)
    with scope(ops, mode, c):
        from dfmir_amd.ops import _plan_conv_wgrad
        run = Raw(ops, c, x, dy)
        assert _plan_conv_wgrad(_geom(c), run.K3, c["probes"], run.parts) == c["plan"]
        dwt, dw, db = run()
        if mode == "deterministic":
            _deterministic_properties(run, dwt, db)
    check(mode, c["id"], "dW", dw, ref[0], bounds(c, "dW"))
    check(mode, c["id"], "db", db.view(-1, 1), ref[1].view(-1, 1), bounds(c, "db"))


@gpu
@pytest.mark.parametrize("host,edge", EDGE_RUNS, ids=["%s-%s" % he for he in EDGE_RUNS])
@pytest.mark.parametrize("mode", MODES)
def test_wgrad_edges(ops, mode, host, edge):
    c = BY_ID[host]
    x, dy = WC.inputs(c, edge)
    ref = WC.reference(c, x, dy)
    with scope(ops, mode, c):
        run = Raw(ops, c, x, dy)
        dwt, dw, db = run()
        if mode == "deterministic":
            dwt2, _, db2 = run()
            assert torch.equal(dwt, dwt2) and torch.equal(db, db2), "two deterministic runs differ"
    key = "%s+%s" % (host, edge)
    if edge in ("zero_input", "zero_dy"):
        assert float(dw.abs().max()) == 0.0, "dW of a zero operand is not exactly zero"
        if edge == "zero_dy":
            assert float(db.abs().max()) == 0.0
            return
    else:
        check(mode, key, "dW", dw, ref[0], bounds(c, "dW", edge))
        if edge == "spread" and c["kind"] == "split" and not c["pmax"]:
            h = c["Cout"] // 2
            l2 = WC.rel_errors(dw[:h], ref[0][:h])[0]
            MARGINS.append((_test_id(), "dW per-channel 2-norm, larger half", l2, SPREAD_L2_LARGER_HALF))
            assert l2 <= SPREAD_L2_LARGER_HALF, l2
    check(mode, key, "db", db.view(-1, 1), ref[1].view(-1, 1), bounds(c, "db", edge))


@gpu
@pytest.mark.parametrize("bid,N,Cc,S", BIAS_CASES, ids=[b[0] for b in BIAS_CASES])
@pytest.mark.parametrize("gs", [g for g, _ in BIAS_SCALES], ids=[i for _, i in BIAS_SCALES])
@pytest.mark.parametrize("mode", MODES)
def test_bias_grad(ops, mode, gs, bid, N, Cc, S):
    dy = WC.bias_input(N, Cc, S, gs)
    ref = WC.R.conv_bias_grad(dy)
    bnd = (FACTOR * FP32_YARD["bias"][0], FACTOR * FP32_YARD["bias"][1])
    dyg = dy.to(DEV)
    pre = (torch.arange(Cc, dtype=torch.float32) - 1.0).to(DEV) * float(ref.abs().max())
    with scope(ops, mode):
        db = torch.zeros(Cc, device=DEV)
        ops.bias_grad(dyg, db)
        db2 = torch.zeros(Cc, device=DEV)
        acc = pre.clone()
        if mode == "deterministic":
            ops.bias_grad(dyg, db2)
            ops.bias_grad(dyg, acc)
    if gs == 0.0:
        assert float(db.abs().max()) == 0.0
        return
    check(mode, "%s@%g" % (bid, gs), "db", db.view(-1, 1), ref.view(-1, 1), bnd)
    if mode == "deterministic":
        assert torch.equal(db, db2)
        want = pre.double() + db.double()
        assert bool(((acc.double() - want).abs() <= 2.0 ** -24 * want.abs() * 1.0000001 + 1e-45).all())


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_stem7_backward(ops, mode):
    """ops.conv_taps on a single-channel image takes Stem7Fn: dW and db of conv7x7_c1_wgrad_k (deterministic mode: db from the
    bias pass, the kernel is handed NULL)."""
    c = STEM7
    x, dy = WC.inputs(c)
    ref = WC.reference(c, x, dy)

    def run():
        w = torch.zeros(c["Cout"], 1, 7, 7, device=DEV, requires_grad=True)
        b = torch.zeros(c["Cout"], device=DEV, requires_grad=True)
        y = ops.conv_taps(x[:, :, 0].to(DEV), w, b, 3, 1)
        y.backward(dy[:, :, 0].to(DEV))
        return w.grad, b.grad

    with scope(ops, mode):
        dw, db = run()
        if mode == "deterministic":
            dw2, db2 = run()
            assert torch.equal(dw, dw2) and torch.equal(db, db2)
    check(mode, c["id"], "dW", dw.unsqueeze(2), ref[0], bounds(c, "dW"))
    check(mode, c["id"], "db", db.view(-1, 1), ref[1].view(-1, 1), bounds(c, "db"))


@gpu
@pytest.mark.parametrize("cid", ["mfma-c16-reflect", "s2m-16to32"])
@pytest.mark.parametrize("mode", MODES)
def test_conv_backward_end_to_end(ops, mode, cid):
    """ops.conv -> ConvFn.backward -> conv_wgrad_raw with db: a kernel whose db is a pass of its own, and one that fuses db
    (conv3ds2.hip) and is handed NULL in deterministic mode."""
    c = BY_ID[cid]
    x, dy = WC.inputs(c)
    ref = WC.reference(c, x, dy)
    sq = (lambda t: t[:, :, 0]) if c["nd"] == 2 else (lambda t: t)

    def run():
        w = torch.zeros((c["Cout"], c["Cin"]) + (c["K"],) * c["nd"], device=DEV, requires_grad=True)
        b = torch.zeros(c["Cout"], device=DEV, requires_grad=True)
        y = ops.conv(sq(x).to(DEV), w, b, None, c["stride"], c["pad"], 1 if c["reflect"] else 0, 0, 0.0)
        y.backward(sq(dy).to(DEV))
        return w.grad, b.grad

    with scope(ops, mode):
        dw, db = run()
        if mode == "deterministic":
            dw2, db2 = run()
            assert torch.equal(dw, dw2) and torch.equal(db, db2)
    check(mode, "e2e-" + cid, "dW", dw.reshape(ref[0].shape), ref[0], bounds(c, "dW"))
    check(mode, "e2e-" + cid, "db", db.view(-1, 1), ref[1].view(-1, 1), bounds(c, "db"))


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_upcat_conv3d_backward(ops, mode):
    """ops.upcat_conv3d -> UpCatConv3dFn.backward: dW, db over cat(nearest_up2(a), b), which the library never builds."""
    c = BY_ID["sw-upcat-16+2to32"]
    (a, b), dy = WC.inputs(c)
    ref = WC.reference(c, (a, b), dy)

    def run():
        w = torch.zeros(c["Cout"], c["Cin"], 3, 3, 3, device=DEV, requires_grad=True)
        bias = torch.zeros(c["Cout"], device=DEV, requires_grad=True)
        ag, bg = a.to(DEV).requires_grad_(), b.to(DEV)     # d(a) wanted, d(b) not: the backward hands conv_wgrad_raw the parts
        assert ops.upcat_conv3d_ok(ag, bg, w)
        y = ops.upcat_conv3d(ag, bg, w, bias, None, 0, 0.0)
        y.backward(dy.to(DEV))
        return w.grad, bias.grad

    with scope(ops, mode):
        dw, db = run()
        if mode == "deterministic":
            dw2, db2 = run()
            assert torch.equal(dw, dw2) and torch.equal(db, db2)
    check(mode, "e2e-upcat", "dW", dw, ref[0], bounds(c, "dW"))
    check(mode, "e2e-upcat", "db", db.view(-1, 1), ref[1].view(-1, 1), bounds(c, "db"))
