"""GPU: the contrastive path -- csrc/patchnce.hip, the head / loss algebra of csrc/nce_head.hip and their glue in ops.py -- against
the plain float64 references of tests/ref64.py (themselves checked against the fp32 oracle by tests/test_ref64.py), on every
dispatch path of the launchers.  Run on the MI355X box:  python -m pytest tests/test_gpu_patchnce_fp64.py -m gpu -q

Tolerances.  The project's bars: BAR = 1e-4 for loss rows, normalised rows and the head's output, BAR_DQ = 3e-4 for dq, dx and
the head's weight and bias gradients, BAR_DFEAT = 1e-3 for d(feat) through the head.  Loss rows are compared ELEMENT-wise,
|got_i - ref_i| <= bar * max(|ref_i|, 1e-2 max |ref|) (rows_near); dq / dx per ROW in the 2-norm against the reference row's
norm, floored at 1e-2 of the largest row norm (per_row); rows with a zero cotangent must come back exactly zero.  The fp32
oracle is 7e-8 .. 6e-7 from float64 on every well-conditioned input here, so those bars hold without help.  Ill-conditioned
inputs (unnormalised rows: logits in the thousands; the weight gradients behind an L2 normalisation, which cancel) take
bounded(..., oracle=the fp32 CPU result on the same input): max(bar, 2 x the oracle's own error), refused above 10 x bar;
tests/test_ref64.py proves on the CPU that each of them stays under that cap.  No bound comes from a kernel's own error.
Every comparison lands in tests.test_gpu_ops.MARGINS (DFMIR_MARGINS_OUT writes the table: profiles/r08_patchnce_margins.txt).

Launcher branch -> kernel -> test id
  dfmir_patchnce_fwd (csrc/patchnce.hip)
    R == 256, C <= 256, C % 32 == 0     patchnce_fwd_mfma_k         test_patchnce_rows[mfma-*]  (C 32: one chunk; 96: three; 256: eight)
    else, 16 C + 80 floats <= 64 KB     patchnce_fwd_k, one jb pass  test_patchnce_rows[mixed-*], [scalar-R256-*], [scalar-R64-C1], [scalar-R16-*], [scalar-R48-*]
                                        second jb pass, 16 of 256    test_patchnce_rows[scalar-R272-C20-G1]
                                        two full jb passes           test_patchnce_rows[scalar-R512-C64-G1]
                                        C = 1019 (the LDS limit)     test_patchnce_forward_width_limit
    C >= 1020 / R % 16 / rows % G       refused, nothing written     test_patchnce_forward_width_limit, test_patchnce_refusals_write_nothing
  dfmir_patchnce_bwd
    R == 256, C <= 256, C % 16 == 0     patchnce_bwd_mfma_k         test_patchnce_rows[mfma-*] (ntile 2, 6, 16), [mixed-*] (ntile 1, 3, 15:
                                                                    `ct < ntile` leaves waves / tiles empty in all but C = 256; the
                                                                    zero it feeds goes into accumulators the store guard drops, so
                                                                    no value depends on it.  Which of the two backward kernels
                                                                    ran is not observable either: at C % 32 == 16 the scalar kernel
                                                                    returns the SAME BITS -- both chain fp32 FMAs over j in order)
    else, C <= 330                      patchnce_bwd_k, ncp = 1      test_patchnce_rows[scalar-*] with C <= 256 (R 16 .. 512: `j < R` in the
                                                                    last 32-column tile at R = 16, 48, 272)
                                        ncp = 2                      test_patchnce_rows[scalar-R16-C257], [scalar-R16-C300-G2], [scalar-R16-C330]
    C > 330                             refused                      test_patchnce_gradient_width_is_refused_before_the_forward (ops refuses
                                                                    ahead of the forward; the launcher's own check is called there too)
  dfmir_l2norm_fwd / _bwd               l2norm_fwd_k / l2norm_bwd_k  test_l2norm_rows[*] (C < 16: idle channel groups; rows % 16: ragged tile),
                                        n == 0                       test_l2norm_zero_row, test_fused_head_bias_corners[dead-relu-b2-zero]
  dfmir_patch_gather_fwd_g              patch_gather_fwd_k           test_patch_gather_forward_exact[*], test_patch_gather_backward_*
  dfmir_patch_gather_fwd                patch_gather_fwd_k, bpg = B  test_patch_gather_ungrouped_entry_points
  dfmir_patch_gather_fwd_multi          patch_gather_multi_k         test_patch_gather_forward_exact[*] (G sources)
  dfmir_patch_gather_bwd_g              patch_gather_bwd_k<true>     test_patch_gather_backward_distinct_exact, test_fork_tap_repeated_and_distinct_ids[distinct-*], test_probe_upkeep[g-*]
  dfmir_patch_gather_bwd_gp             <true> + pmax                test_probe_upkeep[gp-*]  (ops.py takes it when the incoming gradient carries a plane-maxima tag)
  dfmir_patch_gather_bwd_any            <false> (atomics)            test_patch_gather_backward_repeated_ids, test_fused_head_repeated_ids,
                                                                    test_fork_tap_repeated_and_distinct_ids[repeated-*], test_probe_upkeep[any-*]
  dfmir_patch_gather_bwd / _bwd_amax    <false> / <true>, bpg = B    test_patch_gather_ungrouped_entry_points (ops.py calls neither)
    the 64-bit index form of patch_gather_bwd_k (B C P >= 2^31 - 1) is NOT run: its rows buffer alone is 8.6 GB, and with
    P <= 1024 from the id generator it needs two million feature planes -- no option reaches it
  dfmir_nce_head_fwd (csrc/nce_head.hip) nce_head_fwd_k              test_fused_head[*] (C 1 .. 256: K padded to 16 with C = 1, 2, 15, 17, 255; odd C:
                                                                    the unpaired last row; rows 8 / 32 / 33 / 100: only, full, ragged last tile),
                                                                    test_fused_head_group_limit (G = 8, G = 9 refused), test_fused_head_bias_corners
  dfmir_segment_means_fwd / _bwd        segment_means_k / _bwd_k     test_segment_means[*] (seg 1, 255, 256, 257, 1000), test_nce_terms_two_kernels
  dfmir_scalar_combine_fwd / _bwd       scalar_combine_k / _bwd_k    test_scalar_combine_limits_and_shapes (8 x 8; 9 refused)
  ops.py glue: ids_distinct routing, TapForkFn's stash, PatchSampleF / PatchNCELoss: the tests above and test_host_routes[*];
  ids_distinct's tag and cache rules run on the CPU (tests/test_host_logic.py).
"""
import ctypes
import math
import types

import pytest
import torch

from tests import ref64 as R
from tests.golden import common as C
from tests.test_gpu_ops import MARGINS, close, near, ops  # noqa: F401  (ops: the module-scoped fixture)
from tests.test_gpu_pointwise_fp64 import _f64, _test_id, bounded, oracle_bound  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda"
BAR, BAR_DQ, BAR_DFEAT = 1e-4, 3e-4, 1e-3
T0 = 0.07


# ============================================================================================== comparisons
def rows_err(got, ref):
    """max_i |got_i - ref_i| / max(|ref_i|, 1e-2 max |ref|)."""
    g, r = _f64(got), _f64(ref)
    scale = torch.clamp(r.abs(), min=max(1e-2 * float(r.abs().max()), 1e-300))
    return float(((g - r).abs() / scale).max())


def rows_near(got, ref, bar, what):
    g, r = _f64(got), _f64(ref)
    assert g.shape == r.shape, "%s: shape %s vs %s" % (what, tuple(g.shape), tuple(r.shape))
    assert bool(torch.isfinite(g).all()), "%s: non-finite values" % what
    err = rows_err(g, r)
    MARGINS.append((_test_id(), what, err, bar))
    assert err <= bar, "%s: element-wise rel err %.3e > %.1e" % (what, err, bar)


def per_row_err(got, ref):
    """max over rows of ||got_r - ref_r||_2 / max(||ref_r||_2, 1e-2 max_r ||ref_r||_2); rows along dim 0."""
    g, r = _f64(got), _f64(ref)
    rn = r.norm(dim=1)
    scale = torch.clamp(rn, min=max(1e-2 * float(rn.max()), 1e-300))
    return float(((g - r).norm(dim=1) / scale).max())


def per_row(got, ref, bar, what, zero_rows=None):
    g, r = _f64(got), _f64(ref)
    assert g.shape == r.shape, "%s: shape %s vs %s" % (what, tuple(g.shape), tuple(r.shape))
    assert bool(torch.isfinite(g).all()), "%s: non-finite values" % what
    if zero_rows is not None:
        assert bool((g[zero_rows] == 0).all()), "%s: a row with zero cotangent is not exactly zero" % what
    err = per_row_err(g, r)
    MARGINS.append((_test_id(), what, err, bar))
    assert err <= bar, "%s: per-row rel err %.3e > %.1e" % (what, err, bar)


def exact(got, ref, what):
    g, r = got.detach().cpu(), ref.detach().cpu()
    assert g.shape == r.shape and g.dtype == r.dtype, what
    MARGINS.append((_test_id(), what + " (bit-exact)", float((g.double() - r.double()).abs().max()), 0.0))
    assert torch.equal(g, r), "%s: not bit-equal (max diff %.3e)" % (what, float((g.double() - r.double()).abs().max()))


# ============================================================================================== 1. fused InfoNCE
def l2rows(x, eps=1e-7):
    return x / (x.pow(2).sum(1, keepdim=True).sqrt() + eps)


def nce_inputs(Rr, Cn, G, variant="plain", seed=700):
    """(q, k, cotangent) as fp32 [rows, C] / [rows]; the cotangent holds zeros (every 5th row) and negative entries.
    plain: independent normalised rows.  correlated: k_i = normalise(q_i + s_i noise_i), the s_i iterated in float64 until
    row i's loss sits at its own target, log-uniform in [0.07, 0.8].  ties: keys 2m and 2m + 1 identical (tied logits, at the
    row maximum for the pair's own rows).  unnormalised: 3 x raw normal rows -- logits in the thousands, the -10 fill no
    longer the minimum.  zero-row: query row 3 all zero."""
    rows = Rr * G
    q, k = C.randn(seed, rows, Cn), C.randn(seed + 1, rows, Cn)
    if variant == "unnormalised":
        q, k = 3.0 * q, 3.0 * k
    else:
        q, k = l2rows(q), l2rows(k)
    if variant == "correlated":
        target = 0.07 * (0.8 / 0.07) ** C.rand(seed + 3, rows).double()
        noise, ls = k.double(), torch.zeros(rows, dtype=torch.float64)
        for _ in range(40):
            kk = l2rows(q.double() + ls.exp()[:, None] * noise)
            ls = (ls + 0.25 * torch.log(target / R.patchnce_rows(q, kk, G, T0))).clamp(-4.0, 3.0)
        k = kk.float()
    elif variant == "ties":
        k[1::2] = k[0::2]
    elif variant == "zero-row":
        q[3] = 0.0
    cot = C.randn(seed + 2, rows)
    cot[::5] = 0.0
    return q, k, cot


def nce_reference(q, k, cot, G, T, dtype=torch.float64):
    qr = q.to(dtype).requires_grad_()
    l = R.patchnce_rows(qr, k, G, T, dtype)
    (l * cot.to(dtype)).sum().backward()
    return l.detach(), qr.grad


def nce_oracle(q, k, cot, G, T):
    """The fp32 CPU oracle (bmm + cross-entropy) on the same input."""
    from oracle import dfmir_oracle as O
    qr = q.clone().requires_grad_()
    l = O.patchnce_loss(qr, k, G, T)
    (l * cot).sum().backward()
    return l.detach(), qr.grad


def nce_gpu(ops, q, k, cot, G, T, transposed_view=False):
    """loss rows and dq [rows, C] from ops.patchnce_rows on channel-major [C, rows] tensors; transposed_view: q goes in as the
    non-contiguous .t() of a [rows, C] leaf, and the gradient is read in that leaf's layout."""
    if transposed_view:
        leaf = q.clone().to(DEV).requires_grad_()
        qg = leaf.t()
        assert not qg.is_contiguous()
    else:
        leaf = q.t().contiguous().to(DEV).requires_grad_()
        qg = leaf
    lg = ops.patchnce_rows(qg, k.t().contiguous().to(DEV), G, T)
    (lg * cot.to(DEV)).sum().backward()
    return lg.detach(), (leaf.grad if transposed_view else leaf.grad.t())


# (id, R, C, G): the route is decided by dfmir_patchnce_fwd (R == 256, C % 32 == 0) and _bwd (R == 256, C % 16 == 0)
NCE_CASES = [
    ("mfma-R256-C32-G1", 256, 32, 1),           # ntile = 2: three waves own no tile
    ("mfma-R256-C96-G3", 256, 96, 3),           # ntile = 6: wave 1 half full
    ("mfma-R256-C256-G2", 256, 256, 2),         # full width
    ("mixed-R256-C16-G2", 256, 16, 2),          # scalar forward, matrix-core backward
    ("mixed-R256-C48-G1", 256, 48, 1),
    ("mixed-R256-C240-G1", 256, 240, 1),
    ("scalar-R256-C24-G2", 256, 24, 2),
    ("scalar-R256-C3-G1", 256, 3, 1),
    ("scalar-R64-C1", 64, 1, 2),
    ("scalar-R16-C300-G2", 16, 300, 2),         # one 16-row tile is the whole group; ncp = 2
    ("scalar-R48-C3-G2", 48, 3, 2),
    ("scalar-R272-C20-G1", 272, 20, 1),         # second jb pass of 16 of 256 columns
    ("scalar-R512-C64-G1", 512, 64, 1),         # all negatives from a minibatch of two images
    ("scalar-R16-C257", 16, 257, 3),
    ("scalar-R16-C330", 16, 330, 1),            # the backward's LDS limit
]
VARIANT_SHAPES = [("mfma-R256-C96-G3", 256, 96, 3), ("scalar-R272-C20-G1", 272, 20, 1)]
ILL_VARIANTS = ("unnormalised",)                 # compared through bounded(oracle=...); tests/test_ref64.py checks the cap


def _check_nce(ops, q, k, cot, G, T, tag, ill=False, transposed_view=False):
    lr, dqr = nce_reference(q, k, cot, G, T)
    lg, dqg = nce_gpu(ops, q, k, cot, G, T, transposed_view)
    zero = cot == 0
    if ill:
        lo, dqo = nce_oracle(q, k, cot, G, T)
        bounded(lg, lr, BAR, "nce loss rows " + tag, oracle=lo)
        bounded(dqg, dqr, BAR_DQ, "nce dq " + tag, oracle=dqo)
        assert bool((dqg.cpu()[zero] == 0).all())
    else:
        rows_near(lg, lr, BAR, "nce loss rows " + tag)
        per_row(dqg, dqr, BAR_DQ, "nce dq " + tag, zero_rows=zero)


@pytest.mark.parametrize("case", NCE_CASES, ids=[c[0] for c in NCE_CASES])
def test_patchnce_rows(ops, case):
    """Loss rows and dq of ops.patchnce_rows against float64 on every launcher branch (the table in the module docstring)."""
    _, Rr, Cn, G = case
    q, k, cot = nce_inputs(Rr, Cn, G)
    _check_nce(ops, q, k, cot, G, T0, "plain")


@pytest.mark.parametrize("variant", ["T1.0", "T0.01", "correlated", "ties", "unnormalised", "zero-row", "transposed-view"])
@pytest.mark.parametrize("case", VARIANT_SHAPES, ids=[c[0] for c in VARIANT_SHAPES])
def test_patchnce_conditioning(ops, case, variant):
    """Temperatures 1 and 0.01, keys correlated with the queries (float64 row losses in [0.05, 1]), tied keys, unnormalised rows
    (the max shift matters), an all-zero query row, q as a transposed view: one matrix-core and one scalar shape each."""
    _, Rr, Cn, G = case
    T = {"T1.0": 1.0, "T0.01": 0.01}.get(variant, T0)
    q, k, cot = nce_inputs(Rr, Cn, G, variant if variant in ("correlated", "ties", "unnormalised", "zero-row") else "plain", seed=720)
    if variant == "correlated":
        lr = R.patchnce_rows(q, k, G, T0)
        assert 0.05 <= float(lr.min()) and float(lr.max()) <= 1.0
    _check_nce(ops, q, k, cot, G, T, variant, ill=variant in ILL_VARIANTS, transposed_view=variant == "transposed-view")


def test_patchnce_forward_width_limit(ops):
    """The scalar forward holds 16 C + 80 floats of LDS: C = 1019 runs (forward alone, R = 16) and matches float64, C = 1020
    raises."""
    from dfmir_amd import DfmirHipError
    q, k, cot = nce_inputs(16, 1019, 2, seed=730)
    lg = ops.patchnce_rows(q.t().contiguous().to(DEV), k.t().contiguous().to(DEV), 2, T0)
    rows_near(lg, R.patchnce_rows(q, k, 2, T0), BAR, "nce loss rows C=1019")
    q, k, _ = nce_inputs(16, 1020, 1, seed=731)
    with pytest.raises(DfmirHipError):
        ops.patchnce_rows(q.t().contiguous().to(DEV), k.t().contiguous().to(DEV), 1, T0)


@pytest.mark.parametrize("Cn", [331, 1019])
def test_patchnce_gradient_width_is_refused_before_the_forward(ops, Cn):
    """The backward kernels take C <= 330 (matrix-core form: C <= 256).  A wider q that needs a gradient is refused by
    PatchNCEFn.forward / NCETermsFn.forward -- not in the middle of autograd -- while the same q detached still gets its loss;
    dfmir_patchnce_bwd itself refuses such a width without touching dq."""
    from dfmir_amd import DfmirHipError
    from dfmir_amd._lib import lib
    assert ops.PATCHNCE_BWD_MAX_C == 330
    q, k, _ = nce_inputs(16, Cn, 1, seed=732)
    qg, kg = q.t().contiguous().to(DEV), k.t().contiguous().to(DEV)
    with pytest.raises(DfmirHipError, match="no gradient kernel"):
        ops.patchnce_rows(qg.clone().requires_grad_(), kg, 1, T0)
    with pytest.raises(DfmirHipError, match="no gradient kernel"):
        ops.nce_terms([qg.clone().requires_grad_()], [kg], 1, T0, 1.0, 1)
    rows_near(ops.patchnce_rows(qg, kg, 1, T0), R.patchnce_rows(q, k, 1, T0), BAR, "nce loss rows, q detached")
    near(ops.nce_terms([qg], [kg], 1, T0, 1.0, 1)[0], R.patchnce_rows(q, k, 1, T0).mean(), BAR, "nce term, q detached")
    dq = torch.full((Cn, 16), 7.0, device=DEV)
    probs, dl = torch.rand(16, 17, device=DEV), torch.ones(16, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib().dfmir_patchnce_bwd(vp(dl), vp(probs), vp(kg), vp(dq), 16, Cn, 1, T0, st) != 0
    torch.cuda.synchronize()
    assert bool((dq == 7.0).all())


def test_patchnce_refusals_write_nothing(ops):
    """R % 16 != 0 and rows % groups != 0 raise DfmirHipError (through ops) and leave loss, probs and dq as they were (through
    the C entry points on sentinel-filled buffers)."""
    from dfmir_amd import DfmirHipError
    from dfmir_amd._lib import lib
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    for rows, G in ((40, 1), (48, 5), (96, 4)):                     # R = 40; 48 rows in 5 groups; R = 24
        q, k = torch.randn(8, rows, device=DEV), torch.randn(8, rows, device=DEV)
        with pytest.raises(DfmirHipError):
            ops.patchnce_rows(q, k, G, T0)
        with pytest.raises(DfmirHipError):
            ops.nce_terms([q], [k], G, T0, 1.0, 1)
        loss, probs = torch.full((rows,), 7.0, device=DEV), torch.full((rows, rows + 1), 7.0, device=DEV)
        dq = torch.full((8, rows), 7.0, device=DEV)
        assert lib().dfmir_patchnce_fwd(vp(q), vp(k), vp(loss), vp(probs), rows, 8, G, T0, st) != 0
        assert lib().dfmir_patchnce_bwd(vp(loss), vp(probs), vp(k), vp(dq), rows, 8, G, T0, st) != 0
        torch.cuda.synchronize()
        assert bool((loss == 7.0).all()) and bool((probs == 7.0).all()) and bool((dq == 7.0).all())


# ============================================================================================== 2. l2norm_rows
L2_SHAPES = [(1, 37), (3, 50), (15, 16), (16, 17), (17, 33), (256, 40), (300, 5)]      # (C, rows)


def l2_inputs(Cn, rows, scale, seed=740):
    return C.randn(seed, rows, Cn) * scale, C.randn(seed + 1, rows, Cn)


@pytest.mark.parametrize("eps", [1e-7, 1e-3], ids=["eps1e-7", "eps1e-3"])
@pytest.mark.parametrize("scale", [1.0, 1e-6, 1e15], ids=["x1", "x1e-6", "x1e15"])
@pytest.mark.parametrize("shape", L2_SHAPES, ids=["C%d-rows%d" % s for s in L2_SHAPES])
def test_l2norm_rows(ops, shape, scale, eps):
    """y and dx of ops.l2norm_rows against float64: channel counts around the 16 channel groups, ragged 16-row tiles, inputs
    of size 1e-6 (eps = 1e-7 a tenth of the norm) and 1e15.  At C = 1 dx = dy eps / (|x| + eps)^2 is what is left of two
    cancelling terms of size |dy| / (|x| + eps): that is the scale it is compared against."""
    Cn, rows = shape
    x, dy = l2_inputs(Cn, rows, scale)
    xr = x.double().requires_grad_()
    yr = R.l2_normalize(xr, eps)
    (yr * dy.double()).sum().backward()
    xg = x.t().contiguous().to(DEV).requires_grad_()
    yg = ops.l2norm_rows(xg, eps)
    (yg * dy.t().contiguous().to(DEV)).sum().backward()
    per_row(yg.t(), yr, BAR, "l2norm y")
    if Cn == 1:
        floor = float(dy.abs().max()) / (float(x.abs().min()) + eps)
        bounded(xg.grad.t(), xr.grad, BAR, "l2norm dx (C = 1, against |dy| / (|x| + eps))", floor=floor)
    else:
        per_row(xg.grad.t(), xr.grad, BAR, "l2norm dx")


def test_l2norm_zero_row(ops):
    """A zero row: y == 0 and dx == dy / eps, as ref64.l2_normalize_grad defines it (autograd through sqrt would give NaN); its
    neighbours in the same 16-row tile are unaffected."""
    eps = 1e-7
    x, dy = l2_inputs(24, 20, 1.0, seed=745)
    x[7] = 0.0
    yr = R.l2_normalize(x, eps)
    dxr = R.l2_normalize_grad(x, dy, eps)
    assert bool((yr[7] == 0).all()) and bool((dxr[7] == dy[7].double() / eps).all())
    xg = x.t().contiguous().to(DEV).requires_grad_()
    yg = ops.l2norm_rows(xg, eps)
    (yg * dy.t().contiguous().to(DEV)).sum().backward()
    assert bool((yg[:, 7] == 0).all())
    others = torch.arange(20) != 7
    per_row(yg.t()[others], yr[others], BAR, "l2norm y beside a zero row")
    per_row(xg.grad.t()[others], dxr[others], BAR, "l2norm dx beside a zero row")
    close(xg.grad[:, 7], dxr[7], rtol=1e-6, atol=0.0, what="l2norm dx of the zero row (dy / eps)")


# ============================================================================================== 3. gather
def make_ids(seed, G, P, S, repeats=False, dtype=torch.int64):
    """[G, P] ids, every row its own draw, 0 and S - 1 present in each; repeats: positions 2, 3 and P - 1 repeat position 0 / 1."""
    rows = []
    for g in range(G):
        perm = torch.randperm(S - 2, generator=C.gen(seed + g))[:P - 2] + 1
        row = torch.cat([perm, torch.tensor([0, S - 1])])[torch.randperm(P, generator=C.gen(seed + 50 + g))]
        if repeats:
            row[2], row[3], row[P - 1] = row[0], row[0], row[1]
        rows.append(row)
    return torch.stack(rows).to(dtype)


GATHER_CASES = [
    # id, G, Bper, C, spatial, P, ids dtype, channels_last
    ("G1-2d", 1, 2, 5, (7, 9), 16, torch.int64, False),
    ("G3-2d-rows-differ", 3, 2, 4, (6, 5), 12, torch.int64, False),
    ("G1-3d", 1, 2, 3, (3, 4, 5), 20, torch.int64, False),
    ("G3-P-equals-S", 3, 2, 2, (4, 4), 16, torch.int64, False),
    ("G1-int32-ids", 1, 2, 5, (7, 9), 16, torch.int32, False),
    ("G3-channels-last", 3, 2, 6, (5, 7), 10, torch.int64, True),
]


@pytest.mark.parametrize("case", GATHER_CASES, ids=[c[0] for c in GATHER_CASES])
def test_patch_gather_forward_exact(ops, case):
    """ops.patch_gather and ops.patch_gather_multi are bit-exact against indexing: G 1 and 3 with two images per group, id rows
    that differ (a wrong group-to-row mapping shows), a 3-D feature, ids 0 and S - 1, P == S, int32 ids, channels-last input."""
    _, G, Bper, Cn, sp, P, idt, cl = case
    B, S = G * Bper, math.prod(sp)
    feat = C.randn(750, B, Cn, *sp)
    ids = make_ids(751, G, P, S, dtype=idt)
    assert G == 1 or not torch.equal(ids[0], ids[1])
    ref = R.patch_gather(feat, ids, G, dtype=torch.float32)          # [B P, C]
    fg = feat.to(DEV)
    if cl:
        fg = fg.contiguous(memory_format=torch.channels_last)
        assert not fg.is_contiguous()
    exact(ops.patch_gather(fg, ids.to(DEV), G).t(), ref, "gather")
    exact(ops.patch_gather(fg, ids[0].to(DEV) if G == 1 else ids.to(DEV), G).t(), ref, "gather, 1-D ids" if G == 1 else "gather again")
    srcs = [fg[g * Bper:(g + 1) * Bper] for g in range(G)]
    exact(ops.patch_gather_multi(srcs, ids.to(DEV)).t(), ref, "gather multi")


def _gather_grad(ops, feat, ids, G, cot):
    fg = feat.clone().to(DEV).requires_grad_()
    rows = ops.patch_gather(fg, ids.to(DEV), G)
    (rows * cot.t().contiguous().to(DEV)).sum().backward()
    return fg.grad


@pytest.mark.parametrize("case", GATHER_CASES[:4], ids=[c[0] for c in GATHER_CASES[:4]])
def test_patch_gather_backward_distinct_exact(ops, case):
    """Distinct ids (the plain-store scatter): every element of d(feat) is one value of the cotangent or zero -- bit-exact
    against the float64 adjoint rounded to fp32."""
    _, G, Bper, Cn, sp, P, idt, _ = case
    B, S = G * Bper, math.prod(sp)
    feat, cot = C.randn(752, B, Cn, *sp), C.randn(753, B * P, Cn)
    ids = make_ids(751, G, P, S)
    assert ops.ids_distinct(ids.to(DEV), G)
    exact(_gather_grad(ops, feat, ids, G, cot), R.patch_gather_adjoint(cot, ids, G, feat.shape).float(), "gather adjoint, distinct ids")


def test_patch_gather_same_id_in_two_groups_is_distinct(ops):
    """The same position in two different groups lands in different images: still the plain-store form, still exact."""
    G, Bper, Cn, sp, P = 2, 2, 3, (4, 5), 6
    ids = torch.tensor([[0, 19, 7, 3, 11, 5], [5, 7, 0, 19, 2, 3]])
    assert ops.ids_distinct(ids.to(DEV), G) and not ops.ids_distinct(ids.reshape(-1).to(DEV), 1)
    feat, cot = C.randn(754, G * Bper, Cn, *sp), C.randn(755, G * Bper * P, Cn)
    exact(_gather_grad(ops, feat, ids, G, cot), R.patch_gather_adjoint(cot, ids, G, feat.shape).float(), "gather adjoint, shared ids")


def test_patch_gather_backward_repeated_ids(ops):
    """Ids repeated INSIDE a group go through ids_distinct to the accumulating scatter: d(feat) is the float64 adjoint, with the
    repeated positions summed."""
    G, Bper, Cn, sp, P = 3, 2, 5, (6, 5), 12
    ids = make_ids(756, G, P, math.prod(sp), repeats=True)
    assert not ops.ids_distinct(ids.to(DEV), G)
    feat, cot = C.randn(757, G * Bper, Cn, *sp), C.randn(758, G * Bper * P, Cn)
    ref = R.patch_gather_adjoint(cot, ids, G, feat.shape)
    assert float((ref != 0).sum()) < G * Bper * P * Cn              # positions really were summed
    bounded(_gather_grad(ops, feat, ids, G, cot), ref, BAR, "gather adjoint, repeated ids")


@pytest.mark.parametrize("main_used", [True, False], ids=["main-used", "main-unused"])
@pytest.mark.parametrize("repeats", [True, False], ids=["repeated-ids", "distinct-ids"])
def test_fork_tap_repeated_and_distinct_ids(ops, repeats, main_used):
    """ops.fork_tap: the sampled rows' gradient is scattered by TapForkFn.backward into the gradient of `main` (or into zeros when
    `main` is unused), with repeated ids through the accumulating kernel and distinct ones through the plain-store one."""
    G, Bper, Cn, sp, P = 2, 2, 4, (6, 6), 10
    B = G * Bper
    ids = make_ids(760, G, P, math.prod(sp), repeats=repeats)
    feat, cot, w = C.randn(761, B, Cn, *sp), C.randn(762, B * P, Cn), C.randn(763, B, Cn, *sp)
    ref = R.patch_gather_adjoint(cot, ids, G, feat.shape) + (w.double() if main_used else 0.0)
    leaf = feat.clone().to(DEV).requires_grad_()
    main, tap = ops.fork_tap(leaf * 1.0)
    assert hasattr(tap, "_df_tap_stash")
    loss = (ops.patch_gather(tap, ids.to(DEV), G) * cot.t().contiguous().to(DEV)).sum()
    if main_used:
        loss = loss + (main * w.to(DEV)).sum()
    loss.backward()
    if repeats:
        bounded(leaf.grad, ref, BAR, "fork_tap d(feat), repeated ids")
    else:
        exact(leaf.grad, (ref.float() if not main_used else (R.patch_gather_adjoint(cot, ids, G, feat.shape).float() + w)),
              "fork_tap d(feat), distinct ids")


def test_patch_gather_ungrouped_entry_points(ops):
    """dfmir_patch_gather_fwd / _bwd / _bwd_amax (one id row for the whole batch; ops.py goes through the grouped forms):
    gather exact, the atomic scatter with repeated ids and the plain one with distinct ids against the float64 adjoint."""
    from dfmir_amd._lib import lib
    B, Cn, sp, P = 3, 5, (5, 6), 9
    S = math.prod(sp)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    feat, cot = C.randn(764, B, Cn, *sp), C.randn(765, B * P, Cn)
    for repeats in (False, True):
        ids = make_ids(766, 1, P, S, repeats=repeats)
        fg, ig = feat.to(DEV), ids.to(DEV)
        out = torch.empty(Cn, B * P, device=DEV)
        assert lib().dfmir_patch_gather_fwd(vp(fg), vp(ig), vp(out), B, Cn, S, P, st) == 0
        exact(out.t(), R.patch_gather(feat, ids, 1, dtype=torch.float32), "ungrouped gather")
        ref = R.patch_gather_adjoint(cot, ids, 1, feat.shape)
        d, cd = torch.zeros(B, Cn, *sp, device=DEV), cot.t().contiguous().to(DEV)
        assert lib().dfmir_patch_gather_bwd(vp(cd), vp(ig), vp(d), B, Cn, S, P, st) == 0
        bounded(d, ref, BAR, "ungrouped atomic scatter")
        if not repeats:
            d2, amax = torch.zeros(B, Cn, *sp, device=DEV), torch.zeros(64, device=DEV)
            assert lib().dfmir_patch_gather_bwd_amax(vp(cd), vp(ig), vp(d2), B, Cn, S, P, vp(amax), st) == 0
            exact(d2, ref.float(), "ungrouped plain scatter")
            _check_probes(d2, amax, None, torch.zeros(64), None, ref.abs(), "ungrouped amax")


# ============================================================================================== 4. probe upkeep
def _slot_max(plane_max, slots=64):
    """[B C] plane maxima -> [slots] slot maxima, slot = plane index & (slots - 1)."""
    out = torch.zeros(slots, dtype=plane_max.dtype)
    for bc in range(plane_max.numel()):
        out[bc & (slots - 1)] = torch.maximum(out[bc & (slots - 1)], plane_max[bc])
    return out


def _check_probes(dfeat, amax, pmax, amax0, pmax0, wrote_abs, what):
    """Validity of the range probes after a scatter: every amax slot >= the maximum of its planes, every pmax[bc] >= its
    plane's maximum; neither above max(old value, the largest |value| the scatter wrote into its planes) (wrote_abs: per
    element, zero where nothing was written)."""
    d = dfeat.detach().cpu()
    BC = d.shape[0] * d.shape[1]
    plane = d.abs().reshape(BC, -1).max(1).values
    wrote = wrote_abs.float().reshape(BC, -1).max(1).values * (1.0 + 1e-6)       # float64 sum -> the fp32 value written
    a = amax.detach().cpu()
    assert bool((a >= _slot_max(plane)).all()), "%s: an amax slot is below the maximum of its planes" % what
    assert bool((a <= torch.maximum(amax0, _slot_max(wrote))).all()), "%s: an amax slot was raised beyond what was written" % what
    if pmax is not None:
        p = pmax.detach().cpu()
        assert bool((p >= plane).all()), "%s: a pmax entry is below its plane's maximum" % what
        assert bool((p <= torch.maximum(pmax0, wrote)).all()), "%s: a pmax entry was raised beyond what was written" % what


@pytest.mark.parametrize("Cn", [5, 48], ids=["BC10-own-slots", "BC96-shared-slots"])
@pytest.mark.parametrize("form", ["g", "gp", "any", "any-repeats"])
def test_probe_upkeep(ops, form, Cn):
    """dfmir_patch_gather_bwd_g / _gp / _any called as ops.py calls them, into a gradient that already holds values and
    carries its range probes (amax: 64 slot maxima, slot = plane & 63; pmax: plane maxima): afterwards d(feat) is the
    float64 sum and the probes are still upper bounds -- and not looser than what the scatter wrote.  The cotangent is ten
    times the resident gradient, so slots MUST rise; a NaN in the cotangent turns its slot (and plane) into +inf.  Validity of
    an upper bound only: the fp16-split weight gradient scales its input by these probes and overflows on one that is too small."""
    from dfmir_amd._lib import lib
    assert ops.PROBE_SLOTS == 64
    G, Bper, sp, P = 2, 1, (6, 7), 11
    B, S = G * Bper, math.prod(sp)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    ids = make_ids(770, G, P, S, repeats=form == "any-repeats")
    d0, cot = C.randn(771, B, Cn, *sp), C.randn(772, B * P, Cn) * 10.0
    pmax0 = d0.abs().reshape(B * Cn, -1).max(1).values
    amax0 = _slot_max(pmax0)
    adj = R.patch_gather_adjoint(cot, ids, G, d0.shape)
    ref = d0.double() + adj
    # the largest |value| any thread can have written at an element: the final sum, or (atomics over repeats) a partial one
    wrote = torch.where(adj != 0, d0.double().abs() + R.patch_gather_adjoint(cot.abs(), ids, G, d0.shape), torch.zeros_like(adj)) \
        if form == "any-repeats" else torch.where(adj != 0, ref.abs(), torch.zeros_like(adj))
    for nan_at in (None, (P + 4, 2)):                              # (row of image 1, channel 2) -> plane 1 * Cn + 2
        cg = cot.clone()
        if nan_at is not None:
            cg[nan_at] = float("nan")
        d, amax, pmax = d0.clone().to(DEV), amax0.clone().to(DEV), pmax0.clone().to(DEV)
        cgd, idd = cg.t().contiguous().to(DEV), ids.to(DEV)         # named: the raw pointers must outlive the call
        args = (vp(cgd), vp(idd), vp(d), B, Cn, S, P, G)
        if form == "g":
            rc, pm = lib().dfmir_patch_gather_bwd_g(*args, vp(amax), st), None
        elif form == "gp":
            rc, pm = lib().dfmir_patch_gather_bwd_gp(*args, vp(amax), vp(pmax), st), pmax
        else:
            rc, pm = lib().dfmir_patch_gather_bwd_any(*args, vp(amax), vp(pmax), st), pmax
        assert rc == 0
        torch.cuda.synchronize()
        if nan_at is None:
            if form == "any-repeats":
                bounded(d, ref, BAR, "probed scatter d(feat)")
            else:
                exact(d, ref.float(), "probed scatter d(feat)")     # one fp32 add per element: the rounded float64 sum
            _check_probes(d, amax, pm, amax0, pmax0, wrote, "probes after " + form)
            assert bool((amax.cpu() > amax0).any()), "no slot rose: the case does not exercise the upkeep"
        else:
            bc = 1 * Cn + 2
            assert float(amax[bc & 63]) == float("inf")
            if pm is not None:
                assert float(pm[bc]) == float("inf")
                assert bool(torch.isfinite(pm.cpu()[torch.arange(B * Cn) != bc]).all())


# ============================================================================================== 5. fused head
def head_modules(Cn, seed, b1_shift=None, b2_zero=False):
    """Linear(C, 256), Linear(256, 256) on the device with seeded weights; the same values as fp32 CPU tensors."""
    from dfmir_amd import networks as N
    w1, b1 = C.randn(seed, 256, Cn) / math.sqrt(Cn), C.randn(seed + 1, 256) * 0.3
    w2, b2 = C.randn(seed + 2, 256, 256) / 16.0, C.randn(seed + 3, 256) * 0.3
    if b1_shift is not None:
        b1 = b1 + b1_shift
    if b2_zero:
        b2 = torch.zeros(256)
    m0, m2 = N.Linear(Cn, 256).to(DEV), N.Linear(256, 256).to(DEV)
    with torch.no_grad():
        m0.weight.copy_(w1), m0.bias.copy_(b1), m2.weight.copy_(w2), m2.bias.copy_(b2)
    return m0, m2, (w1, b1, w2, b2)


def head_reference(feat, ids, G, params, cot, eps=1e-7, dtype=torch.float64):
    leaves = [t.to(dtype).requires_grad_() for t in (feat,) + tuple(params)]
    y = R.nce_head(leaves[0], ids, *leaves[1:], eps=eps, groups=G, dtype=dtype)
    (y * cot.to(dtype)).sum().backward()
    return [y.detach()] + [t.grad for t in leaves]


HEAD_NAMES = ("out", "dfeat", "dw1", "db1", "dw2", "db2")
HEAD_BARS = (BAR, BAR_DFEAT, BAR_DQ, BAR_DQ, BAR_DQ, BAR_DQ)


def head_gpu(ops, feat, ids, m0, m2, cot, eps=1e-7):
    fg = feat.clone().to(DEV).requires_grad_()
    for m in (m0, m2):
        m.weight.grad = m.bias.grad = None
    y = ops.nce_head(fg, ids.to(DEV), m0, m2, eps)
    (y * cot.t().contiguous().to(DEV)).sum().backward()
    return [y.detach().t(), fg.grad, m0.weight.grad, m0.bias.grad, m2.weight.grad, m2.bias.grad]


HEAD_CASES = [
    # id, C, G, Bper, P, spatial
    ("C1-rows8", 1, 1, 1, 8, (3, 4)),
    ("C2-rows32", 2, 1, 2, 16, (5, 5)),
    ("C15-rows33", 15, 1, 1, 33, (6, 6)),
    ("C16-rows100", 16, 1, 2, 50, (8, 8)),
    ("C17-G3-Bper2-rows96", 17, 3, 2, 16, (5, 5)),
    ("C255-rows33", 255, 1, 1, 33, (6, 6)),
    ("C256-G2-rows100", 256, 2, 1, 50, (8, 8)),
    ("C16-G8-rows32", 16, 8, 1, 4, (3, 3)),
]


@pytest.mark.parametrize("case", HEAD_CASES, ids=[c[0] for c in HEAD_CASES])
def test_fused_head(ops, case):
    """ops.nce_head -- output and d(feat), dw1, db1, dw2, db2 -- against float64, and ops.nce_head_multi bit-equal to it: channel
    counts around the K padding (multiples of 16) and the row pairing, 8 / 32 / 33 / 100 rows (the only tile partial, full,
    ragged last tile), up to 8 groups with distinct id rows, ids 0 and S - 1."""
    _, Cn, G, Bper, P, sp = case
    B, S = G * Bper, math.prod(sp)
    feat, cot = C.randn(780, B, Cn, *sp), C.randn(781, B * P, 256)
    ids = make_ids(782, G, P, S)
    m0, m2, params = head_modules(Cn, 783)
    assert ops.nce_head_ok(Cn, 256, True)
    ref = head_reference(feat, ids, G, params, cot)
    got = head_gpu(ops, feat, ids, m0, m2, cot)
    per_row(got[0], ref[0], BAR, "head out")
    for g, r, nm, bar in list(zip(got, ref, HEAD_NAMES, HEAD_BARS))[1:]:
        bounded(g, r, bar, "head " + nm)
    srcs = [feat[g * Bper:(g + 1) * Bper].contiguous().to(DEV) for g in range(G)]
    exact(ops.nce_head_multi(srcs, ids.to(DEV), m0, m2).t(), got[0], "multi-source head vs query head")


def test_fused_head_group_limit(ops):
    """G = 9 groups: refused (the launch carries 8 source pointers); G = 8 is test_fused_head[C16-G8-rows32]."""
    from dfmir_amd import DfmirHipError
    m0, m2, _ = head_modules(4, 784)
    feat, ids = C.randn(785, 9, 4, 3, 3).to(DEV), make_ids(786, 9, 4, 9).to(DEV)
    with pytest.raises(DfmirHipError):
        ops.nce_head(feat, ids, m0, m2)
    with pytest.raises(DfmirHipError):
        ops.nce_head_multi([feat[g:g + 1].contiguous() for g in range(9)], ids, m0, m2)


@pytest.mark.parametrize("b2_zero", [False, True], ids=["dead-relu", "dead-relu-b2-zero"])
def test_fused_head_bias_corners(ops, b2_zero):
    """b1 strongly negative: the ReLU is dead for every row, the output is normalise(b2) and only db2 is non-zero.  With b2 = 0 on
    top the pre-normalisation row is zero: out == 0 and db2 = sum of dout / eps, everything finite."""
    Cn, G, Bper, P, sp = 17, 1, 2, 20, (5, 5)
    feat, cot = C.randn(787, G * Bper, Cn, *sp), C.randn(788, G * Bper * P, 256)
    ids = make_ids(789, G, P, math.prod(sp))
    m0, m2, params = head_modules(Cn, 790, b1_shift=-100.0, b2_zero=b2_zero)
    ref = head_reference(feat, ids, G, params, cot)
    assert float(ref[1].abs().max()) == 0.0 and float(ref[4].abs().max()) == 0.0 and float(ref[5].abs().max()) > 0.0
    got = head_gpu(ops, feat, ids, m0, m2, cot)
    if b2_zero:
        assert bool((ref[0] == 0).all()) and bool((got[0] == 0).all())
    else:
        per_row(got[0], ref[0], BAR, "head out, dead ReLU")
    for g, r, nm, bar in list(zip(got, ref, HEAD_NAMES, HEAD_BARS))[1:]:
        bounded(g, r, bar, "head %s, dead ReLU" % nm)               # zero references: exactly zero back


def test_fused_head_repeated_ids(ops):
    """Repeated ids through ops.nce_head: ids_distinct routes d(feat) to the accumulating scatter."""
    Cn, G, Bper, P, sp = 16, 2, 2, 12, (5, 5)
    feat, cot = C.randn(791, G * Bper, Cn, *sp), C.randn(792, G * Bper * P, 256)
    ids = make_ids(793, G, P, math.prod(sp), repeats=True)
    assert not ops.ids_distinct(ids.to(DEV), G)
    m0, m2, params = head_modules(Cn, 794)
    ref = head_reference(feat, ids, G, params, cot)
    got = head_gpu(ops, feat, ids, m0, m2, cot)
    per_row(got[0], ref[0], BAR, "head out, repeated ids")
    bounded(got[1], ref[1], BAR_DFEAT, "head dfeat, repeated ids")


# ============================================================================================== 6. loss algebra
def test_nce_terms_two_kernels(ops):
    """ops.nce_terms over a C = 256 layer (matrix-core kernels) and a C = 24 layer (scalar kernels) at R = 256 in one call: both
    write their rows into the shared buffer; per-row losses, the per-term sums and both dq against float64."""
    n_terms, B, P, lam = 2, 1, 256, 0.25
    G, Cs = n_terms * B, (256, 24)
    ins = [nce_inputs(P, Cn, G, seed=800 + 10 * l) for l, Cn in enumerate(Cs)]
    w = torch.tensor([0.75, -1.5])
    qr = [q.double().requires_grad_() for q, _, _ in ins]
    rows_r = torch.stack([R.patchnce_rows(qr[l], ins[l][1], G, T0) for l in range(2)])
    out_r = R.segment_means(rows_r, n_terms, lam / 2)
    (out_r * w.double()).sum().backward()
    qg = [q.t().contiguous().to(DEV).requires_grad_() for q, _, _ in ins]
    out = ops.nce_terms(qg, [k.t().contiguous().to(DEV) for _, k, _ in ins], G, T0, lam / 2, n_terms)
    rows_near(out.grad_fn.rows_buf, rows_r, BAR, "nce_terms row buffer")
    rows_near(out, out_r, BAR, "nce_terms per-term losses")
    (out * w.to(DEV)).sum().backward()
    for l in range(2):
        per_row(qg[l].grad.t(), qr[l].grad, BAR_DQ, "nce_terms dq, layer C=%d" % Cs[l])


@pytest.mark.parametrize("seg", [1, 255, 256, 257, 1000])
def test_segment_means(ops, seg):
    """dfmir_segment_means_fwd / _bwd: L in {1, 5} layers, T in {1, 3} terms, a negative scale; segments of one element, one
    short of / exactly / one past the 256 threads, and several strides."""
    from dfmir_amd._lib import lib
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    for L in (1, 5):
        for T in (1, 3):
            scale = -0.3 / L
            rows, g = C.randn(810 + L + T, L, T * seg) + 0.5, C.randn(815, T)
            rr = rows.double().requires_grad_()
            ref = R.segment_means(rr, T, scale)
            (ref * g.double()).sum().backward()
            out, drows, rd, gd = torch.empty(T, device=DEV), torch.empty(L, T * seg, device=DEV), rows.to(DEV), g.to(DEV)
            assert lib().dfmir_segment_means_fwd(vp(rd), vp(out), L, T, seg, scale, st) == 0
            assert lib().dfmir_segment_means_bwd(vp(gd), vp(drows), L, T, seg, scale, st) == 0
            tag = "L%d T%d" % (L, T)
            bounded(out, ref, BAR, "segment means " + tag)
            rows_near(drows, rr.grad, BAR, "segment means gradient " + tag)


def test_scalar_combine_limits_and_shapes(ops):
    """ops.scalar_combine: 8 inputs x 8 outputs run, 9 of either raise; a one-element input of shape (1,) gets its gradient in
    that shape, a 0-dim one in its own."""
    from dfmir_amd import DfmirHipError
    M = (C.randn(820, 8, 8)).tolist()
    vals, g = C.randn(821, 8), C.randn(822, 8)
    xs = [(vals[i].reshape(1) if i % 2 else vals[i].reshape(())).clone().to(DEV).requires_grad_() for i in range(8)]
    out = ops.scalar_combine(M, xs)
    xr = [v.double().requires_grad_() for v in vals]
    ref = R.scalar_combine(M, xr)
    (ref * g.double()).sum().backward()
    bounded(out, ref, BAR, "scalar combine 8 x 8")
    (out * g.to(DEV)).sum().backward()
    for i, x in enumerate(xs):
        assert tuple(x.grad.shape) == ((1,) if i % 2 else ())
    bounded(torch.stack([x.grad.reshape(()) for x in xs]), torch.stack([x.grad for x in xr]), BAR, "scalar combine gradient")
    with pytest.raises(DfmirHipError):
        ops.scalar_combine(C.randn(823, 8, 9).tolist(), xs + [xs[0]])
    with pytest.raises(DfmirHipError):
        ops.scalar_combine(C.randn(824, 9, 8).tolist(), xs)


# ============================================================================================== 7. host routes, end to end
ROUTES = [(r, P, a) for r in ("no-mlp", "mlp256-fused", "mlp128-unfused") for P in (300, 64) for a in (False, True)]
ROUTE_C = {"no-mlp": 24, "mlp256-fused": 32, "mlp128-unfused": 32}


def route_inputs(route, seed=830):
    """Two 16 x 16 feature maps of two images (query side, key side), the MLP's seeded weights (None without MLP), a cotangent."""
    Cn = ROUTE_C[route]
    nc = {"no-mlp": Cn, "mlp256-fused": 256, "mlp128-unfused": 128}[route]
    fq, fk = C.randn(seed, 2, Cn, 16, 16), C.randn(seed + 1, 2, Cn, 16, 16)
    params = None
    if route != "no-mlp":
        params = (C.randn(seed + 2, nc, Cn) / math.sqrt(Cn), C.randn(seed + 3, nc) * 0.3,
                  C.randn(seed + 4, nc, nc) / math.sqrt(nc), C.randn(seed + 5, nc) * 0.3)
    return fq, fk, params, nc


def route_oracle(route, fq, fk, params, nc, ids, all_neg, cot, dtype):
    """The oracle's PatchSampler + patchnce_loss in `dtype`: loss rows, d(fq) and the MLP's parameter gradients."""
    from oracle import dfmir_oracle as O
    smp = O.PatchSampler(nc, route != "no-mlp")
    f = fq.to(dtype).requires_grad_()
    if params is not None:
        smp.create_mlp([fq])
        with torch.no_grad():
            for p_, v in zip(smp.mlp_0.parameters(), params):
                p_.copy_(v)
        smp = smp.to(dtype)
    q, _ = smp([f], 64, [ids])
    with torch.no_grad():
        k, _ = smp([fk.to(dtype)], 64, [ids])
    l = O.patchnce_loss(q[0], k[0], 2, T0, all_neg)
    (l * cot.to(dtype)).sum().backward()
    return [l.detach(), f.grad] + ([p_.grad for p_ in smp.mlp_0.parameters()] if params is not None else [])


def route_cot(rows):
    cot = C.randn(840, rows)
    cot[::5] = 0.0
    return cot


@pytest.mark.parametrize("route,P,all_neg", ROUTES, ids=["%s-P%d-%s" % (r, P, "allneg" if a else "perimage") for r, P, a in ROUTES])
def test_host_routes(ops, route, P, all_neg):
    """networks.PatchSampleF + patchnce.PatchNCELoss against the oracle's PatchSampler + patchnce_loss in float64, same weights
    and ids: without MLP, with the fused head (nc = 256), with gather + project (nc = 128); num_patches above S (P = S = 256) and
    64; negatives per image and from the whole minibatch.  The ids are the sampler's own draw.  Loss rows element-wise; the
    gradients of the features and of the MLP through bounded() with the fp32 oracle (sums behind a normalisation cancel)."""
    from dfmir_amd import networks as N
    from dfmir_amd.patchnce import PatchNCELoss
    fq, fk, params, nc = route_inputs(route)
    netF = N.PatchSampleF(use_mlp=route != "no-mlp", init_type='normal', init_gain=0.02, gpu_ids=[0], nc=nc)
    fg, kg = fq.clone().to(DEV).requires_grad_(), fk.to(DEV)
    if params is not None:
        netF.create_mlp([fg])
        with torch.no_grad():
            for p_, v in zip(netF.mlp_0.parameters(), params):
                p_.copy_(v)
    _, idl = netF([kg], P, None)                                   # the sampler's own draw: randperm(S)[:min(P, S)]
    ids = idl[0]
    Pn = min(P, 256)
    assert ids.shape == (Pn,) and ops.ids_distinct(ids)
    if route == "mlp256-fused":
        assert ops.nce_head_ok(fg.shape[1], nc, True)
        q = netF.sample_project(0, fg, ids).t()
        with torch.no_grad():
            k = netF.sample_project_multi(0, [kg], ids.view(1, -1)).t()
    else:
        q = netF([fg], P, [ids])[0][0]
        with torch.no_grad():
            k = netF([kg], P, [ids])[0][0]
    opt = types.SimpleNamespace(nce_includes_all_negatives_from_minibatch=all_neg, batch_size=2, nce_T=T0)
    loss = PatchNCELoss(opt)(q, k)
    cot = route_cot(2 * Pn)
    (loss * cot.to(DEV)).sum().backward()
    got = [loss.detach(), fg.grad] + ([p_.grad for p_ in netF.mlp_0.parameters()] if params is not None else [])
    ref = route_oracle(route, fq, fk, params, nc, ids.cpu(), all_neg, cot, torch.float64)
    o32 = route_oracle(route, fq, fk, params, nc, ids.cpu(), all_neg, cot, torch.float32)
    rows_near(got[0], ref[0], BAR, "route loss rows")
    names = ("dfeat", "dw1", "db1", "dw2", "db2")
    bars = (BAR_DFEAT, BAR_DQ, BAR_DQ, BAR_DQ, BAR_DQ)
    for g, r, o, nm, bar in zip(got[1:], ref[1:], o32[1:], names, bars):
        bounded(g, r, bar, "route " + nm, oracle=o)
