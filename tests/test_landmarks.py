"""Landmark_Loss / ops.landmark_loss / ops.landmark_distances / ops.warp_points / infer.landmark_error (build-defined,
dfmir_amd/csrc/landmark.hip): the C ABI and the argument checks (CPU), a float64 restatement of the definition written with
explicit floor / clamp / gather indexing, checked on the CPU against an independent F.grid_sample(flow, points,
align_corners=True) composition and against the closed-form adjoint, and on the GPU against the kernels: value, d table,
mapped points and dflow for both penalties, isotropic and anisotropic spacing, with and without weights; the invalid kinds, an
all-invalid call, d = 0 under 'tre', exact zeros away from the landmarks, run-to-run bit-reproducibility, non-contiguous
inputs, infer.landmark_error and Registration3DModel(landmark_weight=...) eager and captured.

Sizes of the kernels: LM_T = 256 threads per workgroup = landmarks per workgroup (lm_fwd_k, lm_prep_k, lm_bwd_k) = landmarks
per LDS tile of the backward's owner-gather (dfmir_amd/csrc/landmark.hip); a sample of K landmarks takes ceil(K / 256) workgroups, and each of them walks
ceil(K / 256) tiles.  So K runs over 1, 255 / 256 / 257 (one tile short of full, full, two tiles with one landmark in the
second), 513 (three tiles) and 4096 (the maximum, 16 tiles, once); B = 2 at K = 257 has a sample boundary between workgroups.
The kernels have no tile along the volume: a landmark reads and writes the 2^nd corners of its own cell only, so the volumes
vary the strides, the upper faces and the one-cell volume 2 x 2 (x 2), where every landmark collides with every other.

Landmark sets (`landmarks`): every K >= 48 carries, in seeded positions spread over the index range, random interior points,
points on integer coordinates, points at 0 and exactly at S - 1 on each axis (and both extreme corners), 8 landmarks in one
cell plus 4 at one identical position in that cell (12 in the cell: the collision path), 6 in the cells next to it (shared
faces, edges and corners), and one of each invalid kind (outside by 1e-3 below 0 and above S - 1, a NaN fixed coordinate, a
NaN and an infinite moving coordinate, and -- with weights -- weight 0).  K > 256 repeats the identical position at the
first and the last index, so a collision spans tiles.  K = 1 is one interior point.

The 'tre' gradient r / d is ill-conditioned as d -> 0, so every moving point is placed at the float64 mapped position plus
an offset o with 0.5 <= |o| <= 3 voxels; the smallest spacing entry used is 0.7, so d >= 0.35 >= 0.25 voxel for every valid
landmark -- asserted on the CPU (`reference`) before anything is compared.  d = 0 exactly is a test of its own.  Nothing is
excluded from any comparison: value and gradient are continuous in the point position (no derivative with respect to the
points is taken); NaN entries are compared as a pattern.

Tolerances (profiles/landmark_margins.txt): every comparison with the restatement is bounded by 4x the error of the SAME
definition evaluated by torch in fp32 on the CPU against the float64 restatement, on this very case set -- the maxima over
the cases: the loss (relative), d and the mapped points (max-abs), dflow (relative 2-norm, and max-abs over max).
scripts/landmark_margins.py measures them, and the kernels' own errors beside them."""
import ctypes
import itertools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import step3d
from tests.golden import common as C

DEV = "cuda"
FACTOR = 4.0
# profiles/landmark_margins.txt, row "max" of the fp32 CPU columns: (loss rel, d max-abs, mapped max-abs, dflow 2-norm, dflow max)
FP32_ERR = (4.69e-07, 3.28e-06, 2.01e-06, 8.14e-07, 1.13e-06)
BOUND = tuple(FACTOR * e for e in FP32_ERR)
LM_T = 256                                   # landmarks per workgroup and per LDS tile (landmark.hip)
MAX_K = 4096
MIN_D = 0.25

VOLS_3D = [(2, 3, 3, 4, 5), (1, 3, 13, 17, 19), (1, 3, 2, 2, 2)]
VOLS_2D = [(2, 2, 9, 11), (1, 2, 37, 41), (1, 2, 2, 2)]
ANISO = {3: (2.5, 1.0, 0.7), 2: (0.7, 1.6)}
# (flow shape, K)
CASES = ([(s, 1) for s in VOLS_3D + VOLS_2D] + [(s, 64) for s in VOLS_3D + VOLS_2D]
         + [((1, 3, 13, 17, 19), k) for k in (LM_T - 1, LM_T, LM_T + 1)]
         + [((2, 2, 9, 11), k) for k in (LM_T - 1, LM_T, LM_T + 1)]
         + [((2, 3, 3, 4, 5), LM_T + 1), ((1, 2, 37, 41), 2 * LM_T + 1), ((1, 3, 13, 17, 19), MAX_K)])
# (penalty, anisotropic spacing, weights): both penalties, both spacings, with and without weights
VARIANTS = [('l2', False, False), ('l2', True, True), ('tre', False, True), ('tre', True, False)]


def _id(case):
    return "x".join(str(v) for v in case[0]) + "-K%d" % case[1]


def _vid(v):
    return "%s-%s-%s" % (v[0], "aniso" if v[1] else "iso", "w" if v[2] else "now")


# ------------------------------------------------------------------------------------------ restatement
def lm_terms(flow, q, p, w, h, dtype=torch.float64):
    """The definition, term by term, in `dtype` on the CPU: dict(valid [B,K] bool, i0 [B,K,nd] long, w1 [B,K,nd], m [B,K,nd],
    r [B,K,nd], d [B,K], wv [B,K] = w where valid else 0).  Explicit floor / clamp / gather indexing; invalid rows are
    computed at q = p = 0 and masked by the caller.  Differentiable with respect to `flow`; d has derivative 0 at d = 0."""
    B, nd = flow.shape[:2]
    vol = tuple(flow.shape[2:])
    S = math.prod(vol)
    K = q.shape[1]
    q, p = q.to(dtype), p.to(dtype)
    wt = torch.ones(B, K, dtype=dtype) if w is None else w.to(dtype)
    valid = (wt > 0) & torch.isfinite(q).all(-1) & torch.isfinite(p).all(-1)
    for a in range(nd):
        valid = valid & (q[..., a] >= 0) & (q[..., a] <= vol[a] - 1)
    qs = torch.where(valid[..., None], q, torch.zeros_like(q))
    ps = torch.where(valid[..., None], p, torch.zeros_like(p))
    i0 = torch.stack([torch.clamp(torch.floor(qs[..., a]), max=vol[a] - 2) for a in range(nd)], -1)
    w1 = qs - i0
    i0 = i0.long()
    strides = [math.prod(vol[a + 1:]) for a in range(nd)]
    ff = flow.to(dtype).reshape(B, nd, S)
    u = torch.zeros(B, K, nd, dtype=dtype)
    for bits in itertools.product((0, 1), repeat=nd):                       # corners in ascending order, x the lowest bit
        flat = sum((i0[..., a] + bits[a]) * strides[a] for a in range(nd))
        cw = w1[..., 0] if bits[0] else 1.0 - w1[..., 0]
        for a in range(1, nd):
            cw = cw * (w1[..., a] if bits[a] else 1.0 - w1[..., a])
        val = torch.gather(ff, 2, flat[:, None, :].expand(B, nd, K))          # [B,nd,K]
        u = u + cw[..., None] * val.transpose(1, 2)
    m = qs + u
    hh = torch.tensor(h, dtype=dtype)
    r = hh * (m - ps)
    d2 = r[..., 0] * r[..., 0]
    for a in range(1, nd):
        d2 = d2 + r[..., a] * r[..., a]
    pos = d2 > 0
    d = torch.where(pos, torch.sqrt(torch.where(pos, d2, torch.ones_like(d2))), torch.zeros_like(d2))
    return dict(valid=valid, i0=i0, w1=w1, m=m, r=r, d=d, d2=d2, wv=torch.where(valid, wt, torch.zeros_like(wt)))


def lm_ref(flow, q, p, w=None, h=None, penalty='l2', dtype=torch.float64):
    """(loss, d [B,K] with NaN for invalid landmarks, mapped [B,K,nd] with NaN rows, per_sample [B], dflow) of the
    definition in `dtype` on the CPU (float64: the restatement; float32: the yardstick); dflow by autograd."""
    nd = flow.shape[1]
    h = (1.0,) * nd if h is None else tuple(h)
    f = flow.detach().cpu().to(dtype).requires_grad_()
    t = lm_terms(f, q.cpu(), p.cpu(), None if w is None else w.cpu(), h, dtype)
    wv, valid = t['wv'], t['valid']
    wsum = wv.sum()
    pen = t['d2'] if penalty == 'l2' else t['d']
    loss = (wv * pen).sum() / wsum if float(wsum) > 0 else f.sum() * 0.0
    loss.backward()
    nan = torch.full((), float('nan'), dtype=dtype)
    d = torch.where(valid, t['d'].detach(), nan)
    m = torch.where(valid[..., None], t['m'].detach(), nan)
    ws = wv.sum(1)
    per = torch.where(ws > 0, (wv * t['d'].detach()).sum(1) / torch.where(ws > 0, ws, torch.ones_like(ws)), nan)
    return float(loss.detach()), d, m, per, f.grad


def lm_adjoint(flow, q, p, w, h, penalty):
    """dflow by the documented closed form, float64: dflow[b, a, corner] += (w / Wsum) dl/dr_a h_a cornerweight, dl/dr_a =
    2 r_a ('l2') or r_a / d ('tre', 0 at d = 0).  An explicit loop over the landmarks: shares no code with autograd."""
    B, nd = flow.shape[:2]
    vol = tuple(flow.shape[2:])
    t = lm_terms(flow.double(), q, p, w, h)
    wsum = float(t['wv'].sum())
    out = torch.zeros(flow.shape, dtype=torch.float64)
    if wsum == 0.0:
        return out
    for b in range(B):
        for k in range(q.shape[1]):
            if not bool(t['valid'][b, k]):
                continue
            d = float(t['d'][b, k])
            for a in range(nd):
                ra = float(t['r'][b, k, a])
                dl = 2.0 * ra if penalty == 'l2' else (ra / d if d > 0 else 0.0)
                g = float(t['wv'][b, k]) / wsum * dl * h[a]
                for bits in itertools.product((0, 1), repeat=nd):
                    cw = 1.0
                    for c in range(nd):
                        w1 = float(t['w1'][b, k, c])
                        cw *= w1 if bits[c] else 1.0 - w1
                    idx = (b, a) + tuple(int(t['i0'][b, k, c]) + bits[c] for c in range(nd))
                    out[idx] += g * cw
    return out


def lm_grid_sample(flow, q):
    """q + flow(q) from F.grid_sample: normalised coordinates, align_corners=True.  Shares no code with lm_terms; for
    in-volume points."""
    B, nd = flow.shape[:2]
    vol = tuple(flow.shape[2:])
    norm = [2.0 * q[..., a] / (vol[a] - 1) - 1.0 for a in range(nd)]
    grid = torch.stack(norm[::-1], -1).reshape((B,) + (1,) * (nd - 1) + (q.shape[1], nd))      # last axis: x, y(, z)
    u = F.grid_sample(flow, grid, mode='bilinear', padding_mode='border', align_corners=True)
    return q + u.reshape(B, nd, q.shape[1]).transpose(1, 2)


# ------------------------------------------------------------------------------------------ inputs
def make_flow(shape, seed):
    return ((C.rand(seed, *shape).double() * 2.0 - 1.0) * 2.0).float()


INVALID_KINDS = ("below", "above", "q-nan", "p-nan", "p-inf", "w-zero")


def landmarks(shape, K, weights, seed=900):
    """(q, p_offset, w, invalid [B,K] bool, tags) of a case: fixed points, the offsets that the moving points get from the
    mapped positions (`reference` adds them), the weights (None without) and which entries are invalid by construction."""
    B, nd = shape[:2]
    vol = shape[2:]
    top = torch.tensor([n - 1 for n in vol], dtype=torch.float64)
    q = C.rand(seed, B, K, nd).double() * top * 0.999                          # random interior points
    direction = C.randn(seed + 1, B, K, nd).double()
    direction = direction / direction.norm(dim=-1, keepdim=True)
    off = direction * (0.5 + 2.5 * C.rand(seed + 2, B, K, 1).double())           # 0.5 <= |o| <= 3
    w = (0.5 + 1.5 * C.rand(seed + 3, B, K)).float() if weights else None
    invalid = torch.zeros(B, K, dtype=torch.bool)
    tags = {}
    if K >= 48:
        for b in range(B):
            ends = [0, K - 1] if K > LM_T else []
            slots = [i for i in torch.randperm(K, generator=C.gen(seed + 10 + b)).tolist() if i not in ends]
            take = lambda n: [slots.pop() for _ in range(n)]
            ii = take(8)                                                       # integer coordinates
            q[b, ii] = torch.floor(C.rand(seed + 20 + b, 8, nd).double() * (top + 1)).clamp(max=top)
            ff = take(2 * nd + 2)                                              # 0 and exactly S - 1 on each axis, both corners
            for a in range(nd):
                q[b, ff[2 * a], a] = 0.0
                q[b, ff[2 * a + 1], a] = top[a]
            q[b, ff[2 * nd]] = 0.0
            q[b, ff[2 * nd + 1]] = top
            cell = torch.floor(C.rand(seed + 30 + b, nd).double() * (top - 1).clamp(min=0)).clamp(min=0)
            cc = take(8)                                                       # 8 in one cell
            q[b, cc] = cell + 0.05 + 0.9 * C.rand(seed + 40 + b, 8, nd).double()
            same = take(4)                                                     # 4 at one identical position in that cell
            q[b, same] = cell + torch.tensor([0.25, 0.5, 0.75][:nd], dtype=torch.float64)
            for e in ends:                                                     # ... and at the first and the last index
                q[b, e] = q[b, same[0]]
                same.append(e)
            nb = take(6)                                                       # the cells around it
            shift = torch.floor(C.rand(seed + 50 + b, 6, nd).double() * 3.0) - 1.0
            q[b, nb] = ((cell + shift).clamp(min=0) + 0.05 + 0.9 * C.rand(seed + 60 + b, 6, nd).double()).clamp(max=top)
            bad = take(len(INVALID_KINDS))
            a0 = b % nd
            q[b, bad[0], a0] = -1e-3
            q[b, bad[1], a0] = float(np.float32(top[a0]) + np.float32(1e-3))
            q[b, bad[2], (a0 + 1) % nd] = float('nan')
            invalid[b, bad[:5]] = True
            if weights:
                w[b, bad[5]] = 0.0
                invalid[b, bad[5]] = True
            tags[b] = dict(integer=ii, faces=ff, cell=cc, same=same, near=nb, bad=bad)
    return q.float(), off, w, invalid, tags


_REF = {}


def inputs(case, weights):
    """(flow, q, p, w, invalid) fp32 of a case: p = the float64 mapped position of q + the offset, then the two invalid
    moving coordinates."""
    key = (case, weights)
    if key not in _REF:
        shape, K = case
        B, nd = shape[:2]
        flow = make_flow(shape, 700 + 7 * CASES.index(case) if case in CASES else 699)
        q, off, w, invalid, tags = landmarks(shape, K, weights)
        t = lm_terms(flow, q, torch.zeros_like(q), None, (1.0,) * nd)
        p = (t['m'] + off).float()
        for b, tg in tags.items():
            p[b, tg['bad'][3], 0] = float('nan')
            p[b, tg['bad'][4], nd - 1] = float('inf')
        _REF[key] = (flow, q, p, w, invalid, tags)
    return _REF[key]


def spacing_of(nd, aniso):
    return ANISO[nd] if aniso else None


def reference(case, variant):
    """(flow, q, p, w, h, (loss64, d64, m64, per64, dflow64)) of a case and variant, computed once and shared.  Asserts that
    every valid landmark lies at d >= MIN_D and that the invalid ones are the ones built as such."""
    penalty, aniso, weights = variant
    key = (case, variant)
    if key not in _REF:
        flow, q, p, w, invalid, _ = inputs(case, weights)
        h = spacing_of(flow.shape[1], aniso)
        ref = lm_ref(flow, q, p, w, h, penalty)
        assert torch.equal(torch.isnan(ref[1]), invalid), case
        assert float(ref[1][~invalid].min()) >= MIN_D, (case, float(ref[1][~invalid].min()))
        _REF[key] = (flow, q, p, w, h, ref)
    return _REF[key]


def errors(got, ref):
    """(loss rel, d max-abs, mapped max-abs, dflow relative 2-norm, dflow max-abs over max) of (loss, d, m, per, dflow)
    against the restatement's; the NaN patterns of d and the mapped points must agree exactly."""
    loss, d, m, _, df = got
    d, m, df = d.detach().cpu().double(), m.detach().cpu().double(), df.detach().cpu().double()
    assert torch.equal(torch.isnan(d), torch.isnan(ref[1])) and torch.equal(torch.isnan(m), torch.isnan(ref[2]))
    assert bool(torch.isfinite(df).all())
    ok = ~torch.isnan(ref[1])
    return (abs(float(loss) - ref[0]) / abs(ref[0]), float((d - ref[1])[ok].abs().max()),
            float((m - ref[2])[ok].abs().max()), float((df - ref[4]).norm() / ref[4].norm()),
            float((df - ref[4]).abs().max() / ref[4].abs().max()))


def _gpu(flow, q, p, w, h, penalty):
    """(loss, d, mapped, per_sample, dflow) from the kernels."""
    from dfmir_amd import ops
    f = flow.to(DEV).requires_grad_()
    qd, pd = q.to(DEV), p.to(DEV)
    wd = None if w is None else w.to(DEV)
    loss = ops.landmark_loss(f, qd, pd, wd, h, penalty)
    loss.backward()
    d, per = ops.landmark_distances(f.detach(), qd, pd, wd, h)
    m = ops.warp_points(qd, f.detach())
    torch.cuda.synchronize()
    # warp_points decides by q alone: it also maps a point whose partner or weight makes the PAIR invalid; those rows are NaN
    # in the restatement (test_landmark_invalid_kinds_give_nan_rows_and_no_gradient checks warp_points' own pattern)
    m = torch.where(torch.isnan(d)[..., None], torch.full_like(m, float('nan')), m)
    return loss.detach().cpu(), d.cpu(), m.cpu(), per.cpu(), f.grad.cpu()


# ------------------------------------------------------------------------------------------ CPU tier
SYMS = ("dfmir_landmark_ws_floats", "dfmir_landmark_fwd", "dfmir_landmark_bwd")


def test_landmark_symbols_in_header_exports_and_ctypes_table():
    import dfmir_amd
    from dfmir_amd import _lib, infer, losses, ops
    from dfmir_amd.registration3d import Registration3DModel
    from tests.test_abi import header_symbols
    h = ctypes.CDLL(dfmir_amd.LIB_PATH)
    for s in SYMS:
        assert s in header_symbols() and s in _lib.exported_symbols() and hasattr(h, s) and s in _lib._SIGS, s
    lib = dfmir_amd.lib()
    assert lib.dfmir_abi_version() == 14
    assert lib.dfmir_landmark_ws_floats(3, 1, 1, 16, 16, 16) == 10 * LM_T    # 1 + 3 nd words per landmark, whole tiles
    assert lib.dfmir_landmark_ws_floats(3, 2, LM_T + 1, 16, 16, 16) == 10 * LM_T * 2 * 2
    assert lib.dfmir_landmark_ws_floats(2, 3, MAX_K, 999, 3, 3) == 7 * LM_T * 3 * 16   # nd == 2: D is not read
    for name in ("LandmarkFn", "landmark_loss", "landmark_distances", "warp_points"):
        assert hasattr(ops, name), name
    assert ops.LANDMARK_MAX_K == MAX_K
    assert hasattr(losses, "Landmark_Loss") and hasattr(infer, "landmark_error")
    crit = losses.Landmark_Loss(dim=2, penalty='tre', spacing=(0.5, 2.0), loss_mult=0.5)
    assert crit.name == 'landmark' and crit.penalty == 'tre' and crit.spacing == (0.5, 2.0) and crit.loss_mult == 0.5
    assert losses.Landmark_Loss().spacing == (1.0, 1.0, 1.0) and losses.Landmark_Loss().penalty == 'l2'
    with pytest.raises(ValueError, match="dim"):
        losses.Landmark_Loss(dim=4)
    with pytest.raises(ValueError, match="penalty"):
        losses.Landmark_Loss(penalty='l1')
    with pytest.raises(ValueError, match="spacing"):
        losses.Landmark_Loss(dim=3, spacing=(1.0, 1.0))
    m = Registration3DModel((8, 8, 8), device="cpu")
    assert m.landmark_weight == 0.0 and m._outputs == ('regA', 'flow', 'loss_ncc', 'loss_grad')
    m = Registration3DModel((8, 8), device="cpu", landmark_weight=0.5, landmark_penalty='tre', spacing=(2.0, 1.0))
    assert m._outputs[-1] == 'loss_landmark' and m.criterionLandmark.penalty == 'tre' and m.criterionLandmark.dim == 2
    assert m.criterionLandmark.spacing == (2.0, 1.0)
    with pytest.raises(ValueError, match=">= 0"):
        Registration3DModel((8, 8, 8), device="cpu", landmark_weight=-1.0)
    with pytest.raises(ValueError, match="penalty"):
        Registration3DModel((8, 8, 8), device="cpu", landmark_weight=1.0, landmark_penalty='huber')
    x = torch.zeros(1, 1, 8, 8)
    with pytest.raises(KeyError, match="A_pts"):
        m.set_input({"A": x, "B": x, "B_pts": torch.zeros(1, 4, 2)})
    with pytest.raises(KeyError, match="B_pts"):
        m.set_input({"A": x, "B": x, "A_pts": torch.zeros(1, 4, 2)})
    m.set_input({"A": x, "B": x, "A_pts": torch.zeros(1, 4, 2), "B_pts": torch.ones(1, 4, 2)})
    assert m.pts_w is None and float(m.pts_B.sum()) == 8.0 and float(m.pts_A.sum()) == 0.0


# (nd, B, K, D, H, W, hz, hy, hx, penalty)
GOOD = (3, 1, 8, 8, 8, 8, 1.0, 1.0, 1.0, 0)
BAD_ARGS = [(1, 1, 8, 8, 8, 8, 1.0, 1.0, 1.0, 0), (4, 1, 8, 8, 8, 8, 1.0, 1.0, 1.0, 0), (3, 0, 8, 8, 8, 8, 1.0, 1.0, 1.0, 0),
            (3, 1, 0, 8, 8, 8, 1.0, 1.0, 1.0, 0), (3, 1, MAX_K + 1, 8, 8, 8, 1.0, 1.0, 1.0, 0),
            (3, 1, 8, 1, 8, 8, 1.0, 1.0, 1.0, 0), (3, 1, 8, 8, 1, 8, 1.0, 1.0, 1.0, 0), (3, 1, 8, 8, 8, 1, 1.0, 1.0, 1.0, 0),
            (2, 1, 8, 1, 1, 8, 1.0, 1.0, 1.0, 0), (2, 1, 8, 1, 8, 1, 1.0, 1.0, 1.0, 0),
            (3, 1, 8, 1024, 1024, 1024, 1.0, 1.0, 1.0, 0), (3, 1, 8, 8, 8, 8, 0.0, 1.0, 1.0, 0),
            (3, 1, 8, 8, 8, 8, 1.0, -1.0, 1.0, 0), (3, 1, 8, 8, 8, 8, 1.0, 1.0, float('inf'), 0),
            (3, 1, 8, 8, 8, 8, 1.0, float('nan'), 1.0, 0), (2, 1, 8, 1, 8, 8, 1.0, 1.0, 0.0, 0),
            (3, 1, 8, 8, 8, 8, 1.0, 1.0, 1.0, 2), (3, 1, 8, 8, 8, 8, 1.0, 1.0, 1.0, -1)]


def test_landmark_bad_arguments_are_invalid_without_a_device():
    import dfmir_amd
    lib = dfmir_amd.lib()
    for bad in BAD_ARGS[:11]:
        assert lib.dfmir_landmark_ws_floats(*bad[:6]) == -1, bad
    buf = (ctypes.c_double * 64)()                      # host memory: an argument the checks refuse is never dereferenced
    p = ctypes.cast(buf, ctypes.c_void_p)
    for bad in BAD_ARGS:
        assert lib.dfmir_landmark_fwd(bad[0], *([p] * 10), *bad[1:], None) != 0, bad
        assert b"invalid argument" in lib.dfmir_last_error()
        assert lib.dfmir_landmark_fwd(bad[0], *([None] * 10), *bad[1:], None) != 0, bad
        assert b"invalid argument" in lib.dfmir_last_error()
        assert lib.dfmir_landmark_bwd(bad[0], *([p] * 8), *bad[1:], None) != 0, bad
        assert b"invalid argument" in lib.dfmir_last_error()
        assert lib.dfmir_landmark_bwd(bad[0], *([None] * 8), *bad[1:], None) != 0, bad
        assert b"invalid argument" in lib.dfmir_last_error()
    # forward pointers: flow, fixed_pts, moving_pts, weight, ws, mapped, d, per_sample, loss, wsum.  weight and mapped may be
    # NULL; without moving_pts the call only maps and needs `mapped`
    for hole in (0, 1, 4, 6, 7, 8, 9):
        args = [p] * 10
        args[hole] = None
        assert lib.dfmir_landmark_fwd(GOOD[0], *args, *GOOD[1:], None) != 0, hole
        assert b"invalid argument" in lib.dfmir_last_error()
    args = [p] * 10
    args[2] = args[5] = None
    assert lib.dfmir_landmark_fwd(GOOD[0], *args, *GOOD[1:], None) != 0
    assert b"invalid argument" in lib.dfmir_last_error()
    odd = ctypes.c_void_p(p.value + 4)                  # ws must be 8-byte aligned
    assert lib.dfmir_landmark_fwd(GOOD[0], p, p, p, p, odd, p, p, p, p, p, *GOOD[1:], None) != 0
    assert b"invalid argument" in lib.dfmir_last_error()
    # backward pointers: flow, fixed_pts, moving_pts, weight, gout, wsum, dflow, ws: all but weight
    for hole in (0, 1, 2, 4, 5, 6, 7):
        args = [p] * 8
        args[hole] = None
        assert lib.dfmir_landmark_bwd(GOOD[0], *args, *GOOD[1:], None) != 0, hole
        assert b"invalid argument" in lib.dfmir_last_error()


def test_landmark_ops_reject_bad_arguments_before_any_launch():
    from dfmir_amd import infer, ops
    from dfmir_amd._lib import DfmirHipError
    from dfmir_amd.losses import Landmark_Loss
    f = torch.rand(2, 3, 8, 8, 8)
    q = torch.rand(2, 5, 3)
    for fn in (ops.landmark_loss, ops.landmark_distances):
        with pytest.raises(DfmirHipError, match="mismatch"):
            fn(f, torch.rand(1, 5, 3), torch.rand(1, 5, 3))                   # batch
        with pytest.raises(DfmirHipError, match="mismatch"):
            fn(f, torch.rand(2, 5, 2), torch.rand(2, 5, 2))                   # nd
        with pytest.raises(DfmirHipError, match="mismatch"):
            fn(f, q, torch.rand(2, 6, 3))                                     # the two sets differ
        with pytest.raises(DfmirHipError, match="mismatch"):
            fn(f, q, q, torch.rand(2, 4))                                     # weight
        with pytest.raises(DfmirHipError, match="channels"):
            fn(torch.rand(2, 2, 8, 8, 8), q, q)
        with pytest.raises(DfmirHipError, match="fp32"):
            fn(f.double(), q, q)
        with pytest.raises(DfmirHipError, match="fp32"):
            fn(f, q.double(), q.double())
        with pytest.raises(DfmirHipError, match="fp32"):
            fn(f, q, q.half())
        with pytest.raises(DfmirHipError, match="fp32"):
            fn(f, q, q, torch.ones(2, 5, dtype=torch.float64))
        with pytest.raises(DfmirHipError, match="K must"):
            fn(f, torch.rand(2, 0, 3), torch.rand(2, 0, 3))
        with pytest.raises(DfmirHipError, match="K must"):
            fn(f, torch.rand(2, MAX_K + 1, 3), torch.rand(2, MAX_K + 1, 3))
        for bad in ((1.0, 1.0), (1.0, 0.0, 1.0), (1.0, float('nan'), 1.0), "abc", 2.0):
            with pytest.raises(ValueError, match="spacing"):
                fn(f, q, q, None, bad)
        with pytest.raises(DfmirHipError, match="no CPU fallback"):
            fn(f, q, q)
    with pytest.raises(ValueError, match="penalty"):
        ops.landmark_loss(f, q, q, penalty='l1')
    with pytest.raises(DfmirHipError, match="mismatch"):
        ops.warp_points(torch.rand(2, 5, 2), f)
    with pytest.raises(DfmirHipError, match="no CPU fallback"):
        ops.warp_points(q, f)
    with pytest.raises(ValueError, match="2-D field"):
        Landmark_Loss(dim=3)(torch.rand(1, 2, 8, 8), torch.rand(1, 4, 2), torch.rand(1, 4, 2))
    with pytest.raises(DfmirHipError, match="no CPU fallback"):
        Landmark_Loss(dim=3, penalty='tre')(f, q, q)
    with pytest.raises(ValueError, match="spacing"):
        infer.landmark_error(f, q, q, spacing=(1.0, 1.0))
    with pytest.raises(DfmirHipError, match="no CPU fallback"):
        infer.landmark_error(f, q, q)


CPU_CASES = [((2, 3, 3, 4, 5), 64), ((1, 3, 2, 2, 2), 64), ((2, 2, 9, 11), 64), ((1, 2, 2, 2), 64), ((1, 3, 13, 17, 19), 1)]


@pytest.mark.parametrize("case", CPU_CASES, ids=_id)
@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
def test_restatement_equals_the_grid_sample_composition_and_the_closed_form_adjoint(case, variant):
    penalty = variant[0]
    flow, q, p, w, h, ref = reference(case, variant)
    nd = flow.shape[1]
    hh = (1.0,) * nd if h is None else h
    ok = ~torch.isnan(ref[1])
    qs = torch.where(ok[..., None], q, torch.zeros_like(q)).double()
    m = lm_grid_sample(flow.double(), qs)
    assert float((m - ref[2])[ok].abs().max()) <= 1e-12 * float(ref[2][ok].abs().max())
    d = ((m - p.double()) * torch.tensor(hh, dtype=torch.float64)).norm(dim=-1)
    assert float((d - ref[1])[ok].abs().max()) <= 1e-12 * float(ref[1][ok].max())
    wv = torch.where(ok, torch.ones_like(d) if w is None else w.double(), torch.zeros_like(d))
    loss = float((wv * torch.where(ok, d, torch.zeros_like(d)) ** (2 if penalty == 'l2' else 1)).sum() / wv.sum())
    assert ref[0] > 0.0 and abs(loss - ref[0]) <= 1e-12 * ref[0]
    adj = lm_adjoint(flow, q, p, w, hh, penalty)
    assert float(ref[4].abs().max()) > 0.0
    assert float((adj - ref[4]).abs().max()) <= 1e-12 * float(ref[4].abs().max())


def test_restatement_edge_semantics():
    """Upper-face points read the last cell with weight 1 on its upper corner; Wsum = 0 gives 0 and a zero gradient; d = 0
    under 'tre' has a zero derivative."""
    flow = make_flow((1, 3, 3, 4, 5), 31)
    top = torch.tensor([[[2.0, 3.0, 4.0], [2.0, 1.5, 4.0], [0.0, 3.0, 0.0]]])
    t = lm_terms(flow, top, torch.zeros_like(top), None, (1.0, 1.0, 1.0))
    assert t['i0'][0].tolist() == [[1, 2, 3], [1, 1, 3], [0, 2, 0]] and t['w1'][0].tolist() == [[1, 1, 1], [1, 0.5, 1], [0, 1, 0]]
    assert torch.equal(t['m'][0, 0], top[0, 0].double() + flow[0, :, 2, 3, 4].double())
    assert torch.equal(t['m'][0, 2], top[0, 2].double() + flow[0, :, 0, 3, 0].double())
    want = top[0, 1].double() + 0.5 * (flow[0, :, 2, 1, 4].double() + flow[0, :, 2, 2, 4].double())
    assert float((t['m'][0, 1] - want).abs().max()) <= 1e-15
    p = torch.rand(1, 3, 3)
    for bad_q, bad_p, bad_w in ((top + 5.0, p, None), (top, p * float('nan'), None), (top, p, torch.zeros(1, 3))):
        for penalty in ('l2', 'tre'):
            loss, d, m, per, df = lm_ref(flow, bad_q, bad_p, bad_w, None, penalty)
            assert loss == 0.0 and float(df.abs().max()) == 0.0 and bool(torch.isnan(d).all()) and bool(torch.isnan(per).all())
    q = torch.tensor([[[0.5, 1.25, 2.0], [1.0, 1.0, 1.0]]])
    m = lm_terms(flow, q, torch.zeros_like(q), None, (1.0, 1.0, 1.0))['m']
    pp = m.clone()
    pp[0, 1] += 1.0
    loss, d, _, _, df = lm_ref(flow, q, pp, None, None, 'tre')
    assert float(d[0, 0]) == 0.0 and bool(torch.isfinite(df).all())
    only = lm_ref(flow, q[:, 1:], pp[:, 1:], None, None, 'tre')[4] * 0.5          # the landmark at d = 0 adds nothing
    assert float((df - only).abs().max()) <= 1e-15


def test_comparison_sets_hold_what_they_promise():
    """Every valid landmark at d >= 0.25 voxel (`reference` asserts it for every variant), the invalid kinds present, 12
    landmarks in one cell with 4 at one position, points on both faces of every axis."""
    for case in CASES:
        for variant in VARIANTS:
            if case[1] == MAX_K and variant != VARIANTS[1]:
                continue
            reference(case, variant)
        shape, K = case
        if K < 48:
            continue
        flow, q, p, w, invalid, tags = inputs(case, True)
        nd = shape[1]
        t = lm_terms(flow, q, p, w, (1.0,) * nd)
        for b, tg in tags.items():
            assert int(invalid[b].sum()) == len(INVALID_KINDS)
            cells = t['i0'][b, tg['cell'] + tg['same'][:4]]
            assert bool((cells == cells[0]).all()) and bool((q[b, tg['same']] == q[b, tg['same'][0]]).all())
            assert bool((q[b, tg['integer']] == torch.floor(q[b, tg['integer']])).all())
            for a in range(nd):
                assert float(q[b, tg['faces'][2 * a], a]) == 0.0 and float(q[b, tg['faces'][2 * a + 1], a]) == shape[2 + a] - 1
            if K > LM_T:
                assert 0 in tg['same'] and K - 1 in tg['same']


# ------------------------------------------------------------------------------------------ GPU tier
def _check(got, ref, what):
    e = errors(got, ref)
    print("%s: loss %.3e (bound %.1e)  d %.3e (%.1e)  mapped %.3e (%.1e)  dflow l2 %.3e (%.1e) max %.3e (%.1e)"
          % ((what,) + tuple(x for pr in zip(e, BOUND) for x in pr)))
    # per-sample mean: a convex combination of the d's (summed in double) rounded once to fp32
    per, per64 = got[3].double(), ref[3]
    assert torch.equal(torch.isnan(per), torch.isnan(per64))
    okp = ~torch.isnan(per64)
    assert bool(((per - per64)[okp].abs() <= BOUND[1] + 2.0 ** -23 * per64[okp].abs()).all()), what
    assert all(x <= y for x, y in zip(e, BOUND)), (what, e)
    # exactly zero wherever no valid landmark touches
    assert float(got[4][ref[4] == 0].abs().max() if bool((ref[4] == 0).any()) else 0.0) == 0.0, what


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if c[1] != MAX_K], ids=_id)
def test_landmark_value_table_points_and_gradient_vs_restatement(case):
    for variant in VARIANTS:
        flow, q, p, w, h, ref = reference(case, variant)
        _check(_gpu(flow, q, p, w, h, variant[0]), ref, _id(case) + " " + _vid(variant))


@pytest.mark.gpu
def test_landmark_maximum_k():
    case, variant = CASES[-1], VARIANTS[1]
    assert case[1] == MAX_K
    flow, q, p, w, h, ref = reference(case, variant)
    _check(_gpu(flow, q, p, w, h, variant[0]), ref, _id(case) + " " + _vid(variant))


@pytest.mark.gpu
@pytest.mark.parametrize("case", [((2, 3, 3, 4, 5), 64), ((2, 2, 9, 11), LM_T + 1)], ids=_id)
def test_landmark_invalid_kinds_give_nan_rows_and_no_gradient(case):
    """The invalid entries have NaN in d and a NaN row in the mapped points, the others are finite; the loss and dflow equal,
    bit for bit, those of the call with the invalid entries' weights set to 0 and their coordinates replaced by an
    in-volume point: they add to no sum and touch no voxel."""
    from dfmir_amd import ops
    for penalty in ('l2', 'tre'):
        flow, q, p, w, invalid, tags = inputs(case, True)
        got = _gpu(flow, q, p, w, None, penalty)
        assert torch.equal(torch.isnan(got[1]), invalid)
        assert torch.equal(torch.isnan(got[2]).all(-1), invalid) and torch.equal(torch.isnan(got[2]).any(-1), invalid)
        q2 = torch.where(invalid[..., None], torch.full_like(q, 0.5), q)
        p2 = torch.where(invalid[..., None], torch.zeros_like(p), p)
        w2 = torch.where(invalid, torch.zeros_like(w), w)
        clean = _gpu(flow, q2, p2, w2, None, penalty)
        assert torch.equal(got[0], clean[0]) and torch.equal(got[4], clean[4]) and torch.equal(got[3], clean[3])
        assert torch.equal(got[1][~invalid], clean[1][~invalid])
        # warp_points maps by q alone: a NaN or out-of-volume q gives a NaN row, the others (a bad p, weight 0) are mapped
        m = ops.warp_points(q.to(DEV), flow.to(DEV)).cpu()
        bad_q = ~(torch.isfinite(q).all(-1) & (q >= 0).all(-1) & (q <= torch.tensor(case[0][2:]) - 1).all(-1))
        assert torch.equal(torch.isnan(m).all(-1), bad_q) and torch.equal(torch.isnan(m).any(-1), bad_q)
        assert int(bad_q.sum()) == 3 * case[0][0] and not m.requires_grad


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 3, 3, 4, 5), (1, 2, 9, 11)], ids=lambda s: "x".join(map(str, s)))
def test_landmark_all_invalid_call_is_exactly_zero(shape):
    from dfmir_amd import infer, ops
    B, nd = shape[:2]
    flow = make_flow(shape, 41)
    q = C.rand(42, B, 5, nd) * 1.5
    p = C.rand(43, B, 5, nd)
    top = torch.tensor(shape[2:], dtype=torch.float32)
    for bq, bp, bw in ((q + top, p, None), (q, p * float('nan'), None), (q, p, torch.zeros(B, 5)),
                       (q * float('nan'), p, torch.ones(B, 5)), (q, p, -torch.ones(B, 5))):
        for penalty in ('l2', 'tre'):
            loss, d, m, per, df = _gpu(flow, bq, bp, bw, None, penalty)
            assert float(loss) == 0.0 and float(df.abs().max()) == 0.0 and df.shape == flow.shape
            assert bool(torch.isnan(d).all()) and bool(torch.isnan(per).all())
    out = infer.landmark_error(flow.to(DEV), (q + top).to(DEV), p.to(DEV))
    assert all(bool(torch.isnan(v).all()) for v in out.values())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 3, 13, 17, 19), (2, 2, 9, 11)], ids=lambda s: "x".join(map(str, s)))
def test_landmark_tre_at_zero_distance_has_a_finite_zero_gradient(shape):
    """p = m exactly (the kernel's own mapped positions): d = 0 to the bit, the loss is 0 and dflow is 0 and finite
    everywhere.  Then a mix, half of the landmarks at d = 0 and half one voxel off: the d = 0 half counts in Wsum and adds
    nothing to dflow, which is half the float64 gradient of the other half alone (the float64 restatement of the whole set
    cannot serve: there the first half lies at d ~ 1e-7, not 0, with a gradient of full size)."""
    from dfmir_amd import ops
    B, nd = shape[:2]
    flow = make_flow(shape, 51).to(DEV)
    q = (C.rand(52, B, 40, nd) * (torch.tensor(shape[2:], dtype=torch.float32) - 1)).to(DEV)
    m = ops.warp_points(q, flow)
    f = flow.clone().requires_grad_()
    loss = ops.landmark_loss(f, q, m, penalty='tre')
    loss.backward()
    d, per = ops.landmark_distances(flow, q, m)
    assert float(loss.detach()) == 0.0 and float(d.abs().max()) == 0.0 and float(per.abs().max()) == 0.0
    assert bool(torch.isfinite(f.grad).all()) and float(f.grad.abs().max()) == 0.0
    # a mix: the first 20 at d = 0, the others one voxel off along x: only the others' cells get a gradient
    p = m.clone()
    p[:, 20:, nd - 1] += 1.0
    f = flow.clone().requires_grad_()
    ops.landmark_loss(f, q, p, penalty='tre').backward()
    assert bool(torch.isfinite(f.grad).all())
    only = lm_ref(flow.cpu(), q.cpu()[:, 20:], p.cpu()[:, 20:], None, None, 'tre')[4] * 0.5
    got = f.grad.cpu().double()
    assert float((got - only).abs().max()) <= BOUND[4] * float(only.abs().max()), float((got - only).abs().max())
    assert float(got[only == 0].abs().max()) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("case", [((1, 3, 13, 17, 19), LM_T + 1), ((1, 3, 2, 2, 2), 64), ((2, 2, 9, 11), LM_T + 1),
                                  ((1, 2, 37, 41), 2 * LM_T + 1)], ids=_id)
def test_landmark_bit_reproducible_on_the_collision_sets(case):
    """Three runs of forward and backward on sets with 12 landmarks in one cell, 4 (6 across tiles) at one position and the
    cells around it -- in the 2 x 2 x 2 volume every landmark shares its cell with all the others."""
    for variant in VARIANTS:
        flow, q, p, w, h, _ = reference(case, variant)
        runs = [_gpu(flow, q, p, w, h, variant[0]) for _ in range(3)]
        for r in runs[1:]:
            assert all(torch.equal(torch.nan_to_num(x, nan=-7.0), torch.nan_to_num(y, nan=-7.0)) for x, y in zip(runs[0], r)), variant


@pytest.mark.gpu
def test_landmark_non_contiguous_flow_and_points():
    from dfmir_amd import ops
    case, variant = ((1, 3, 13, 17, 19), 64), VARIANTS[1]
    flow, q, p, w, h, ref = reference(case, variant)
    want = _gpu(flow, q, p, w, h, variant[0])
    perm = (0, 1, 4, 3, 2)
    nf = flow.permute(*perm).contiguous().to(DEV).permute(*perm).requires_grad_()
    nq = q.transpose(1, 2).contiguous().to(DEV).transpose(1, 2)
    npt = torch.stack([p, p], -1).to(DEV)[..., 0]
    nw = torch.stack([w, w], -1).to(DEV)[..., 1]
    assert not nf.is_contiguous() and not nq.is_contiguous() and not npt.is_contiguous() and not nw.is_contiguous()
    loss = ops.landmark_loss(nf, nq, npt, nw, h, variant[0])
    loss.backward()
    d, per = ops.landmark_distances(nf.detach(), nq, npt, nw, h)
    assert torch.equal(loss.detach().cpu(), want[0]) and torch.equal(nf.grad.cpu(), want[4])
    assert torch.equal(torch.nan_to_num(d.cpu(), nan=-7.0), torch.nan_to_num(want[1], nan=-7.0)) and torch.equal(per.cpu(), want[3])
    m = ops.warp_points(nq, nf.detach()).cpu()
    ok = ~torch.isnan(want[2])
    assert torch.equal(m[ok], want[2][ok])
    # dflow written entirely whatever the buffer held, and 16-byte misaligned: the scalar zero fill
    import dfmir_amd
    lib = dfmir_amd.lib()
    f = flow.to(DEV)
    qd, pd, wd = q.to(DEV), p.to(DEV), w.to(DEV)
    hz, hy, hx = h
    out = torch.empty(2, device=DEV)
    ws = torch.empty(int(lib.dfmir_landmark_ws_floats(3, 1, 64, 13, 17, 19)), device=DEV)
    dd, pp = torch.empty(1, 64, device=DEV), torch.empty(1, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.dfmir_landmark_fwd(3, vp(f), vp(qd), vp(pd), vp(wd), vp(ws), None, vp(dd), vp(pp), vp(out), vp(out[1:]), 1, 64,
                                  13, 17, 19, hz, hy, hx, 0, st) == 0
    base = torch.full((f.numel() + 1,), 7.0, device=DEV)
    off = base[1:]
    assert off.data_ptr() % 16 == 4
    g = torch.ones(1, device=DEV)
    assert lib.dfmir_landmark_bwd(3, vp(f), vp(qd), vp(pd), vp(wd), vp(g), vp(out[1:]), vp(off), vp(ws), 1, 64, 13, 17, 19, hz, hy,
                                  hx, 0, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(off.view(flow.shape).cpu(), want[4]) and float(base[0]) == 7.0


@pytest.mark.gpu
def test_landmark_loss_class_scales_and_upstream_gradient():
    from dfmir_amd import ops
    from dfmir_amd.losses import Landmark_Loss
    case, variant = ((2, 2, 9, 11), 64), VARIANTS[3]
    flow, q, p, w, h, ref = reference(case, variant)
    want = _gpu(flow, q, p, w, h, 'tre')
    f = flow.to(DEV).requires_grad_()
    loss = Landmark_Loss(dim=2, penalty='tre', spacing=h, loss_mult=0.25)(f, q.to(DEV), p.to(DEV))
    (loss * 3.0).backward()
    assert abs(float(loss) - 0.25 * float(want[0])) <= 1e-6 * float(want[0])
    assert float((f.grad.cpu() - 0.75 * want[4]).abs().max()) <= 1e-6 * float(want[4].abs().max())
    assert not ops.landmark_distances(f, q.to(DEV), p.to(DEV))[0].requires_grad


@pytest.mark.gpu
def test_landmark_error_agrees_with_distances_and_numpy():
    from dfmir_amd import infer, ops
    for case, variant in ((((2, 3, 3, 4, 5), 64), VARIANTS[1]), (((2, 2, 9, 11), 64), VARIANTS[0])):
        flow, q, p, w, h, ref = reference(case, variant)
        fd, qd, pd = flow.to(DEV), q.to(DEV), p.to(DEV)
        wd = None if w is None else w.to(DEV)
        out = infer.landmark_error(fd, qd, pd, spacing=h, weight=wd)
        d, per = ops.landmark_distances(fd, qd, pd, wd, h)
        assert sorted(out) == ["initial", "mean", "tre"]
        nn = lambda t: torch.nan_to_num(t.cpu(), nan=-7.0)
        assert torch.equal(nn(out["tre"]), nn(d)) and torch.equal(nn(out["mean"]), nn(per))
        hh = np.ones(flow.shape[1], np.float32) if h is None else np.asarray(h, np.float32)
        with np.errstate(invalid='ignore', over='ignore'):
            init = np.sqrt((((q.numpy() - p.numpy()) * hh) ** 2).sum(-1))
        init[np.isnan(d.cpu().numpy())] = np.nan
        got = out["initial"].cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(init))
        ok = ~np.isnan(init)
        # two fp32 evaluations of sqrt(sum((q - p)^2 h^2)): six roundings of half an ulp each on either side
        assert np.abs(got[ok] - init[ok]).max() <= 8 * 2.0 ** -23 * init[ok].max()


# ------------------------------------------------------------------------------------------ model
MODEL_CASES = [((16, 16, 16), 'ncc'), ((32, 32), 'mind')]


def _model_points(shape, K=24, seed=820):
    nd = len(shape)
    top = torch.tensor([n - 1 for n in shape], dtype=torch.float32)
    b_pts = C.rand(seed, 1, K, nd) * top
    a_pts = (b_pts + (C.rand(seed + 1, 1, K, nd) * 2.0 - 1.0) * 2.0).clamp(min=0.0).minimum(top)
    b_pts[0, 3, 0] = -0.5                                  # one outside the volume, one padding entry
    w = torch.ones(1, K)
    w[0, 5] = 0.0
    return a_pts, b_pts, w


@pytest.mark.gpu
@pytest.mark.parametrize("shape,similarity", MODEL_CASES, ids=["3d-ncc", "2d-mind"])
def test_registration3d_landmark_step_eager_and_captured(shape, similarity):
    """Four steps of Registration3DModel(landmark_weight=1.0), eager against capture_step=True (two eager steps, the capture,
    two replays): the same losses at every step and the same parameters after the fourth, within the tolerances that
    test_invcons.py's captured-step test uses for a replayed against an eager step (losses 1e-5 relative; its loosest
    tensor bound, 5e-5 of the maximum, for the parameters).  Weight gradients are summed in fixed point, so an eager step
    repeats itself.  'landmark' is in the losses and equals the restatement on the model's own flow; a missing key raises."""
    from dfmir_amd import ops
    a_pts, b_pts, w = _model_points(shape)
    data = lambda A, B: {"A": A, "B": B, "A_pts": a_pts, "B_pts": b_pts, "pts_weight": w}
    was = ops.deterministic_wgrad()
    try:
        res = []
        for capture in (False, True):
            m, A, B = step3d.step_model(shape, similarity, capture=capture, deterministic_wgrad=True, landmark_weight=1.0,
                                  landmark_penalty='tre')
            with pytest.raises(KeyError, match="B_pts"):
                m.set_input({"A": A, "B": B, "A_pts": a_pts})
            losses = []
            for _ in range(4):
                m.set_input(data(A, B))
                m.optimize_parameters()
                torch.cuda.synchronize()
                losses.append(m.get_current_losses())
            assert (m._graph['graph'] is not None) == capture
            assert sorted(losses[-1]) == sorted(["grad", "landmark", similarity])
            ref = lm_ref(m.flow.detach().cpu(), b_pts, a_pts, w, None, 'tre')[0]
            err = abs(losses[-1]["landmark"] - ref) / ref
            print("step loss_landmark %.4e: %.3e (bound %.1e)" % (losses[-1]["landmark"], err, BOUND[0]))
            assert ref > 0.0 and err <= BOUND[0]
            res.append((losses, m.optimizer_R.flat_p.clone()))
    finally:
        ops.set_deterministic_wgrad(was)
    for le, lc in zip(res[0][0], res[1][0]):
        for k in le:
            assert math.isfinite(lc[k]) and abs(lc[k] - le[k]) <= 1e-5 * max(abs(le[k]), 1e-8), (k, lc[k], le[k])
    err, pmax = float((res[0][1] - res[1][1]).abs().max()), float(res[0][1].abs().max())
    print("parameters after 4 steps, eager against captured: %.3e of max %.3e" % (err, pmax))
    assert err <= 5e-5 * pmax + 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("shape,similarity", MODEL_CASES, ids=["3d-ncc", "2d-mind"])
def test_registration3d_landmark_symmetric_adds_the_reverse_term(shape, similarity):
    from dfmir_amd import ops
    a_pts, b_pts, w = _model_points(shape)
    sp = (1.5, 1.0, 0.8)[:len(shape)]
    m, A, B = step3d.step_model(shape, similarity, symmetric=True, landmark_weight=0.5, spacing=sp)
    for _ in range(2):
        m.set_input({"A": A, "B": B, "A_pts": a_pts, "B_pts": b_pts, "pts_weight": w})
        m.optimize_parameters()
        torch.cuda.synchronize()
        got = m.get_current_losses()
        assert sorted(got) == sorted(["grad", "landmark", similarity]) and all(math.isfinite(x) for x in got.values()), got
        ad, bd, wd = a_pts.to(DEV), b_pts.to(DEV), w.to(DEV)
        fwd = float(ops.landmark_loss(m.flow.detach(), bd, ad, wd, sp))
        rev = float(ops.landmark_loss(m.neg_flow.detach(), ad, bd, wd, sp))
        assert fwd > 0.0 and rev > 0.0 and abs(fwd - rev) > 1e-3 * fwd
        assert abs(got["landmark"] - 0.5 * (fwd + rev)) <= 1e-6 * (fwd + rev)
        ref = 0.5 * (lm_ref(m.flow.detach().cpu(), b_pts, a_pts, w, sp)[0] + lm_ref(m.neg_flow.detach().cpu(), a_pts, b_pts, w, sp)[0])
        assert abs(got["landmark"] - ref) <= BOUND[0] * ref
    assert float(m.optimizer_R.flat_g.abs().max()) > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("shape,similarity", MODEL_CASES, ids=["3d-ncc", "2d-mind"])
def test_registration3d_landmark_defaults_reproduce_the_step(shape, similarity):
    """landmark_weight=0.0, landmark_penalty='l2' spelled out against a model built without them: the first step's losses
    and the parameter arena after it, bit for bit; landmark keys in the data are ignored."""
    from dfmir_amd import ops
    a_pts, b_pts, w = _model_points(shape)
    was = ops.deterministic_wgrad()
    try:
        res = []
        for kw in ({}, dict(landmark_weight=0.0, landmark_penalty='l2')):
            m, A, B = step3d.step_model(shape, similarity, deterministic_wgrad=True, **kw)
            m.set_input({"A": A, "B": B, "A_pts": a_pts, "B_pts": b_pts} if kw else {"A": A, "B": B})
            m.optimize_parameters()
            torch.cuda.synchronize()
            assert not hasattr(m, "loss_landmark")
            res.append((m.get_current_losses(), m.optimizer_R.flat_p.clone()))
    finally:
        ops.set_deterministic_wgrad(was)
    assert res[0][0] == res[1][0] and sorted(res[0][0]) == sorted(["grad", similarity])
    assert torch.equal(res[0][1], res[1][1])
