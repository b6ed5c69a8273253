"""Cases, seeded inputs and CPU evaluators of the weight- and bias-gradient tests: shared by tests/test_gpu_wgrad_fp64.py (its
GPU comparisons and its CPU admission tests) and scripts/wgrad_margins.py.  Nothing here needs a GPU.

A case is one launcher branch (the table in tests/test_gpu_wgrad_fp64.py says which condition of the source each shape
meets).  Inputs: x seeded N(0, 1) * xs; dy seeded (N(0, 1) + 0.5) * gs, optionally times a per-output-channel magnitude --
the mean keeps every bias gradient (0.5 * count against a noise of sqrt(count)) well conditioned, so that a relative error
per channel means something; it changes nothing for dW, whose terms x * dy stay zero-mean."""
import math
import zlib

import torch

from tests import ref64 as R
from tests.golden import common as C

F32, F64 = torch.float32, torch.float64
ORDERS = ("matmul", "chunk64")


def case(id, nd, Cin, Cout, K, stride, pad, reflect, N, sp, kind, plan="generic", probes=False, pmax=False, opts=(), parts=None,
         upw=False):
    """kind: 'fp32' (the kernel multiplies in fp32) | 'split' (fp16 / bf16 pairs).  plan: what ops._plan_conv_wgrad must answer.
    probes / pmax: the range probes / per-plane maxima of dY are handed over.  opts: library options set around the call.
    parts = Ca: the operand is cat(nearest_up2(a), b) with Ca up-sampled channels (sp = the FULL resolution); upw: with
    ops._UPWGRAD_MIN_VOX at 0 (the parity-class kernel at a test-sized volume)."""
    return dict(id=id, nd=nd, Cin=Cin, Cout=Cout, K=K, stride=stride, pad=pad, reflect=reflect, N=N, sp=tuple(sp), kind=kind,
                plan=plan, probes=probes, pmax=pmax, opts=tuple(opts), parts=parts, upw=upw)


BF16 = (("DFMIR_CONV_SPLIT", "b"),)
CASES = [
    # ---- 2-D, csrc/conv.hip: the generic implicit-GEMM kernel and the 1x1 streaming GEMM
    case("mfma-c136", 2, 130, 136, 3, 1, 1, False, 1, (7, 9), "fp32"),
    case("mfma-c40", 2, 8, 40, 3, 1, 1, False, 2, (9, 13), "fp32"),
    case("mfma-c16-reflect", 2, 16, 16, 3, 1, 1, True, 2, (12, 20), "fp32"),
    case("mfma-c32-stride2", 2, 16, 32, 3, 2, 1, False, 2, (15, 17), "fp32"),
    case("1x1-72to49", 2, 72, 49, 1, 1, 0, False, 3, (20, 24), "fp32"),
    case("1x1-8to136", 2, 8, 136, 1, 1, 0, False, 1, (8, 16), "fp32"),
    case("1x1-refused", 2, 72, 49, 1, 1, 0, False, 3, (20, 24), "fp32", opts=(("DFMIR_NO_1X1_WGRAD", "1"),)),
    # ---- 2-D, csrc/conv3x3.hip: the LDS kernel (two tilings) and the small-channel kernel
    case("lds-40to64", 2, 40, 64, 3, 1, 1, False, 2, (16, 32), "fp32"),
    case("lds-40to128-narrow", 2, 40, 128, 3, 1, 1, True, 1, (8, 16), "fp32"),
    case("small-34to16", 2, 34, 16, 3, 1, 1, False, 2, (44, 70), "fp32"),
    case("small-16to2", 2, 16, 2, 3, 1, 1, False, 4, (40, 70), "fp32"),
    case("small-48to12-reflect", 2, 48, 12, 3, 1, 1, True, 2, (64, 64), "fp32"),
    # ---- 2-D, csrc/conv3x3s.hip (+ conv3x3s_w2_body.inc): every `which` of ws_setup
    case("s1-swap-160to64", 2, 160, 64, 3, 1, 1, False, 1, (6, 16), "split", probes=True),
    case("s2-64to128", 2, 64, 128, 3, 1, 1, False, 2, (16, 32), "split", probes=True),
    case("s2-64to128-pmax", 2, 64, 128, 3, 1, 1, False, 2, (16, 32), "split", probes=True, pmax=True),
    case("s2-72to136-reflect-pmax", 2, 72, 136, 3, 1, 1, True, 2, (10, 48), "split", probes=True, pmax=True),
    case("s3-64to64", 2, 64, 64, 3, 1, 1, False, 1, (6, 16), "split", probes=True),
    case("s3-160to64-reflect-pmax", 2, 160, 64, 3, 1, 1, True, 1, (6, 16), "split", probes=True, pmax=True),
    case("s4-bf16-64to128", 2, 64, 128, 3, 1, 1, False, 1, (6, 16), "split", probes=True, opts=BF16),
    case("s5-bf16-72to64-pmax", 2, 72, 64, 3, 1, 1, True, 1, (6, 16), "split", probes=True, pmax=True, opts=BF16),
    # ---- 3-D
    case("c3d-34to32", 3, 34, 32, 3, 1, 1, False, 1, (4, 8, 16), "fp32"),
    case("c3d-32to12", 3, 32, 12, 3, 1, 1, False, 1, (3, 6, 8), "fp32"),
    case("c3d-18to16", 3, 18, 16, 3, 1, 1, False, 2, (2, 5, 20), "fp32"),
    case("c3d-32to32", 3, 32, 32, 3, 1, 1, False, 1, (3, 4, 16), "fp32"),
    case("c3d-generic-w17", 3, 40, 12, 3, 1, 1, False, 1, (6, 7, 17), "fp32", probes=True),
    case("sw-34to32", 3, 34, 32, 3, 1, 1, False, 1, (6, 10, 12), "split", "split3d", probes=True),
    case("sw-pair-40to12", 3, 40, 12, 3, 1, 1, False, 1, (6, 7, 16), "split", "split3d", probes=True),
    case("sw-swapped-16to3", 3, 16, 3, 3, 1, 1, False, 1, (7, 9, 12), "split", "split3d", probes=True),
    case("sw-upcat-16+2to32", 3, 18, 32, 3, 1, 1, False, 1, (6, 10, 16), "split", "split_upcat", probes=True, parts=16),
    case("sw-upcat-8+3to16-pair", 3, 11, 16, 3, 1, 1, False, 2, (4, 8, 8), "split", "split_upcat", probes=True, parts=8),
    case("wm-march", 3, 32, 16, 3, 1, 1, False, 1, (5, 27, 36), "split", "split3d", probes=True),
    case("uw-fused-32+2to32", 3, 34, 32, 3, 1, 1, False, 2, (6, 10, 16), "split", "upwgrad", probes=True, parts=32, upw=True),
    case("uw-4wave-32+16to32", 3, 48, 32, 3, 1, 1, False, 1, (8, 12, 16), "split", "upwgrad", probes=True, parts=32, upw=True),
    case("uw-8wave-32+16to32", 3, 48, 32, 3, 1, 1, False, 1, (8, 12, 16), "split", "upwgrad", probes=True, parts=32, upw=True,
         opts=(("DFMIR_UPWGRAD_8WAVE", "1"),)),
    case("t-s2c2-2to16", 3, 2, 16, 3, 2, 1, False, 1, (12, 10, 16), "fp32", "s2c2"),
    case("t-flow-16to2", 3, 16, 2, 3, 1, 1, False, 2, (4, 8, 32), "split", "split3d", probes=True),
    case("s2m-16to32", 3, 16, 32, 3, 2, 1, False, 1, (15, 17, 21), "fp32", "s2m"),
]
BY_ID = {c["id"]: c for c in CASES}

# the 7x7 stem (csrc/taps.hip conv7x7_c1_wgrad_k: dW and, in the default mode, db at its two df_acc sites); driven through
# ops.conv_taps -> Stem7Fn, which is its only caller
STEM7 = case("stem7-1to64", 2, 1, 64, 7, 1, 3, True, 2, (20, 24), "fp32", plan=None)

# bias_grad_k (csrc/conv.hip bias_grad_launch): (id, N, C, S)
BIAS_CASES = [("b64-scalar", 2, 5, 117), ("b64-quad", 2, 5, 480), ("b256-quad", 1, 3, 4096), ("b256-scalar", 2, 3, 4099),
              ("bsplit2-quad", 1, 1, 65540), ("bsplit2-scalar", 1, 1, 65541)]
BIAS_SCALES = (1.0, 1e-30, 1e30)          # of dy; the GPU test adds an all-zero dy

# Edge families: id -> (xs, gs, per-channel spread of dy).  The first four are those of
# tests/test_gpu_ops.py::test_conv3x3_split_dynamic_range; small_x, big_bound are the two suspected defects of the fixed-point
# scale; spread is that of test_conv3x3_split_channel_magnitude_spread.
EDGES = {"tiny": (1e-12, 1e-14, False), "huge": (3e9, 7e5, False), "denormal_grads": (1.0, 1e-30, False),
         "zero_input": (0.0, 1.0, False), "small_x": (1e-20, 1.0, False), "big_bound": (1e19, 1e16, False),
         "spread": (1.0, 1.0, True), "zero_dy": (1.0, 0.0, False)}
DYNAMIC_RANGE = ("tiny", "huge", "denormal_grads", "small_x", "big_bound")
# hosts: one split and one fp32 kernel in 2-D, one of each in 3-D
EDGE_HOSTS = ("s2-64to128", "s2-64to128-pmax", "lds-40to64", "sw-34to32", "c3d-34to32")
EDGE_RUNS = [(h, e) for h in EDGE_HOSTS for e in EDGES]
FP32_MAX = 3.4028234663852886e38


def geometry(c):
    """(K3, pad3, sp3, out3): the layer as the 5-D call sees it (a 2-D layer has depth 1, K = (1, k, k), pad = (0, p, p))."""
    K, p, s = c["K"], c["pad"], c["stride"]
    K3 = (K,) * 3 if c["nd"] == 3 else (1, K, K)
    p3 = (p,) * 3 if c["nd"] == 3 else (0, p, p)
    sp3 = c["sp"] if c["nd"] == 3 else (1,) + c["sp"]
    out3 = tuple((n + 2 * q - k) // s + 1 for n, q, k in zip(sp3, p3, K3))
    return K3, p3, sp3, out3


def count(c):
    return c["N"] * math.prod(geometry(c)[3])


def inputs(c, edge=None):
    """(x or (a, b), dy), fp32, 5-D.  x is the materialised operand unless the case has parts."""
    xs, gs, spread = EDGES[edge] if edge else (1.0, 1.0, False)
    _, _, sp3, out3 = geometry(c)
    seed = 9000 + 4 * (zlib.crc32(c["id"].encode()) % 100000)       # (a case keeps its inputs when the list changes)
    dy = (C.randn(seed + 2, c["N"], c["Cout"], *out3) + 0.5) * gs
    if spread:
        dy = dy * torch.logspace(0, -6, c["Cout"]).view(1, -1, 1, 1, 1)
    if c["parts"]:
        Ca = c["parts"]
        a = C.randn(seed, c["N"], Ca, *(n // 2 for n in sp3)) * xs
        b = C.randn(seed + 1, c["N"], c["Cin"] - Ca, *sp3) * xs
        return (a.contiguous(), b.contiguous()), dy.contiguous()
    return (C.randn(seed, c["N"], c["Cin"], *sp3) * xs).contiguous(), dy.contiguous()


def bias_input(N, Cc, S, gs=1.0):
    return ((C.randn(9900 + S % 97, N, Cc, S) + 0.5) * gs).contiguous()


def reference(c, x, dy, dtype=F64, order="matmul"):
    """(dW [Cout, Cin, *K3], db [Cout]) of tests/ref64.py in `dtype`."""
    K3, p3, _, _ = geometry(c)
    return (R.conv_weight_grad(x, dy, K3, c["stride"], p3, 1 if c["reflect"] else 0, dtype, order),
            R.conv_bias_grad(dy, dtype, order))


def rel_errors(got, ref):
    """(largest per-output-channel relative 2-norm error, max-abs error over max |ref|) of got against ref [Cout, ...], in
    float64.  A channel (or tensor) whose reference is all zero must be all zero: its error is 0 then, inf otherwise."""
    got, ref = got.detach().to(F64).cpu().flatten(1), ref.detach().to(F64).cpu().flatten(1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not bool(torch.isfinite(got).all()):
        return float("inf"), float("inf")
    d, n = (got - ref).norm(dim=1), ref.norm(dim=1)
    l2 = torch.where(n > 0, d / n.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))
    m = float(ref.abs().max())
    e = float((got - ref).abs().max())
    return float(l2.max()), (e / m if m > 0 else (0.0 if e == 0 else float("inf")))


def yardstick(c, x, dy, ref=None):
    """The fp32 CPU restatement against float64 on these inputs: the larger error of the two evaluation orders, per metric:
    ((dW l2, dW max), (db l2, db max)), plus the float64 reference."""
    ref = ref or reference(c, x, dy)
    ew = eb = (0.0, 0.0)
    for o in ORDERS:
        w32, b32 = reference(c, x, dy, F32, o)
        ew = tuple(max(p, q) for p, q in zip(ew, rel_errors(w32, ref[0])))
        eb = tuple(max(p, q) for p, q in zip(eb, rel_errors(b32.view(-1, 1), ref[1].view(-1, 1))))
    return ew, eb, ref


# ------------------------------------------------------------------ the fixed-point grid of include/dfmir_hip.h
def _e(f):
    return math.frexp(f)[1]


def det_shifts(cnt, ax, ay, rule="documented"):
    """(shift of the dW slots, shift of the db slots): scale = 2^shift.  'documented': include/dfmir_hip.h, "Deterministic
    weight gradients" -- 61 minus the sum of the frexp exponents of count, max|x|, max|dy| (db: of count, max|dy|), 61 when a
    factor is zero, clamped to [-126, 126].  'product': the earlier rule, kept to show what it does to the small-input and
    overflowing-bound cases: one shift for both from the fp32 product count * max(max|x|, 1) * max|dy|, 61 when that
    product is zero or beyond 3e38, clamped to [-120, 120]."""
    f32 = lambda v: float(torch.tensor(v, dtype=F32))
    cnt, ax, ay = f32(cnt), f32(ax), f32(ay)
    if rule == "product":
        B = f32(f32(cnt * max(ax, 1.0)) * ay) if ay > 0 else 0.0
        sh = 61 - (_e(B) if 0.0 < B < 3.0e38 else 0)
        sh = max(-120, min(120, sh))
        return sh, sh
    sw = 61 if (ax == 0 or ay == 0) else 61 - (_e(cnt) + _e(ax) + _e(ay))
    sb = 61 if ay == 0 else 61 - (_e(cnt) + _e(ay))
    return max(-126, min(126, sw)), max(-126, min(126, sb))


def quantise(ref, shift):
    """The float64 reference put through the fixed-point path: rounded to a multiple of 2^-shift as a 64-bit integer (a value
    that does not fit the slot comes out non-finite here; on the device it saturates or wraps), converted back, rounded to fp32."""
    v = torch.round(ref.to(F64) * 2.0 ** shift)
    v = torch.where(v.abs() < 2.0 ** 63, v, torch.full_like(v, float("nan")))
    return (v * 2.0 ** -shift).to(F32)


def operand_max(x):
    return max(float(t.abs().max()) for t in (x if isinstance(x, tuple) else (x,)))
