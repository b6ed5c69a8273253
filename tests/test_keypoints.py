"""Keypoint detection and sparse matching: ops.foerstner_response / ops.local_maxima / ops.select_keypoints /
ops.keypoint_cost / ops.keypoint_argmin / infer.keypoint_init (build-defined, dfmir_amd/csrc/keypoints.hip).  CPU: float64
restatements of the five definitions in plain torch / numpy, written from the formulas of the ops' docstrings, checked against
scipy.ndimage where it states the same thing (maximum_filter on distinct values; gaussian_filter in the interior, where the
renormalised faces play no part); every argument check; select_keypoints' ordering, ties and padding.  GPU: the kernels
against the restatements.

Sizes of the kernels and why each shape is there:
  kp_prod_k   the stencil tile: 8 x 64 voxels of (y, x), chunks of 16 planes along z, halo 1.  (2,1,5,6,7) B = 2 and odd
              extents; (1,1,2,2,2) the one-cell volume, every voxel on two faces per axis; (1,1,13,17,19) several tile rows;
              (2,1,9,11) / (1,1,37,41) the 2-D kernel; (1,1,17,9,65) and (1,1,17,65) cross the tile (and the z chunk) by one
              voxel in every axis.  The Gaussian between the two kernels is dfmir_gauss_smooth itself (tests/test_gauss.py);
              sigma 0 (the copy), 1.5 (the default, radius 5) and 5 (radius 15, above the smallest extent of every 3-D shape).
  kp_nms_k    tiles 4 x 8 x 32 (3-D, radius <= 6), 4 x 4 x 16 (3-D, radius 7, 8), 16 x 64 (2-D), halo = radius.  The shapes
              above again: 2 x 2 x 2 and 5 x 6 x 7 are smaller than the window at radius 8, 17 x 9 x 65 crosses all three tiles
              by one voxel (17 = 4 * 4 + 1, 9 = 8 + 1 = 2 * 4 + 1, 65 = 2 * 32 + 1 = 4 * 16 + 1), 17 x 65 the 2-D one.
  kp_cost_k   256 threads, JPT = 1, 3, 6, 12 or 20 displacements per thread: D = 9 and 27 (JPT 1), 49 and 125 (1), 343 (3:
              radius 3), 1089 (6: 2-D radius 16), 4913 (20: 3-D radius 8); the channel group G < C with and without a
              remainder (C = 12 and C = 16 at E = 37: two stages of 6; 6 + 6 + 4), G = C elsewhere; the 2 x 2 x 2 volume lies
              inside every window.
  kp_argmin_k one wave per row, four rows per workgroup: K = 1 and 65 (a partial last workgroup); D from 9 (most lanes idle)
              to 4913 (77 values per lane); ties planted at j = 0, 63, 64, 65 and D - 1 straddle the lane and the trip boundary.

Tolerances, PER CASE (profiles/keypoints_margins.txt lists them beside the kernels' own errors): e32 = the max-abs error of the
same definition evaluated by torch in fp32 on the CPU against the float64 restatement (the response's determinant in double in
both, as the op defines it).  The kernel's max-abs error is bounded by 4 e32 + 4 * 2^-23 max|reference|: the factor 4 is the
project's usual margin over the fp32 CPU evaluation (tests/test_tps.py, tests/test_landmarks.py), the floor keeps a case whose
fp32 evaluation happens to be exact from a zero bound.  NMS and argmin are exact: no tolerance.
With sigma = 0 the 3-D tensor is a single outer product, of rank one: determinant and trace of the adjugate are both rounding
residue, the response is noise of the order of |g|^2 in any precision, e32 equals max|reference| and the bound exceeds every
signal -- those six response cases assert finiteness and little else.  What sigma = 0 can check is checked apart, and exactly:
test_products_bitwise compares the product planes of dfmir_keypoint_products bit for bit with the fp32 CPU evaluation
(difference, true division by 2 h, product: three correctly rounded operations, no contraction).

End to end.  Exact shift: both cuts of one smooth noise volume, so the cost at the true displacement is exactly 0 for every
keypoint whose reads stay inside (the mask keeps the others out) and positive elsewhere; the coupling can only confirm it.
Smooth deformation, seed 7: the float64 restatement of the pipeline from keypoint_cost on, fed the GPU's keypoints and features;
a keypoint may be left out only where the restatement's two best penalised costs lie closer than twice the case's cost bound,
and at most 5 % may be (profiles/keypoints_margins.txt records the share found, and at how many keypoints the restatement's
own fp32 evaluation picks another index)."""
import functools
import itertools
import math

import numpy as np
import pytest
import torch

import dfmir_amd
from dfmir_amd import infer, ops
from dfmir_amd._lib import DfmirHipError

DEV = "cuda"
F64 = torch.float64
F32 = torch.float32
FACTOR = 4.0
FLOOR = 4.0 * 2.0 ** -23
ANISO = {3: (2.5, 1.0, 0.7), 2: (0.7, 1.6)}


# ------------------------------------------------------------------------------------------ restatements
def ref_gauss(x, sigma, dtype):
    """ops.gaussian_smooth's definition on the trailing nd axes of x [B,C,*vol]: weights rounded to fp32, renormalised faces."""
    x = x.to(dtype)
    r = int(math.ceil(3.0 * sigma))
    if r == 0:
        return x
    w = [float(np.float32(math.exp(-k * k / (2.0 * sigma * sigma)))) for k in range(r + 1)]
    for axis in range(x.dim() - 1, 1, -1):                                   # x, y, then z
        n = x.shape[axis]
        num = torch.zeros_like(x)
        den = torch.zeros(n, dtype=dtype)
        for k in range(-r, r + 1):
            lo, hi = max(0, -k), min(n, n - k)
            if lo >= hi:
                continue
            num.narrow(axis, lo, hi - lo).add_(x.narrow(axis, lo + k, hi - lo) * w[abs(k)])
            den[lo:hi] += w[abs(k)]
        shape = [1] * x.dim()
        shape[axis] = n
        x = num / den.view(shape)
    return x


def ref_response(I, sigma, h, dtype=F64):
    """R [B,1,*vol] float64: gradient, products and Gaussian in `dtype`, the determinant ratio in double."""
    nd = I.dim() - 2
    I = I.to(dtype)
    g = []
    for a in range(nd):
        ax = a + 2
        n = I.shape[ax]
        ip = torch.arange(n).add(1).clamp(max=n - 1)
        im = torch.arange(n).sub(1).clamp(min=0)
        two_h = torch.tensor([2.0 * float(np.float32(h[a]))], dtype=dtype)    # one element: a true division, no reciprocal
        g.append((I.index_select(ax, ip) - I.index_select(ax, im)) / two_h)
    T = {}
    for a in range(nd):
        for b in range(a, nd):
            T[a, b] = ref_gauss(g[a] * g[b], sigma, dtype).to(F64)
    if nd == 3:
        a, b, c, d, e, f = T[0, 0], T[0, 1], T[0, 2], T[1, 1], T[1, 2], T[2, 2]
        A00, A11, A22 = d * f - e * e, a * f - c * c, a * d - b * b
        det = a * A00 - b * (b * f - c * e) + c * (b * e - c * d)
        tr = (A00 + A11) + A22
    else:
        a, b, c = T[0, 0], T[0, 1], T[1, 1]
        det, tr = a * c - b * b, a + c
    fin = torch.stack([torch.isfinite(t) for t in T.values()]).all(0)
    ok = fin & (tr > 0)
    R = torch.where(ok, det / torch.where(ok, tr, torch.ones_like(tr)), torch.zeros_like(tr))
    R = torch.where(torch.isfinite(R), R, torch.zeros_like(R))
    return R.to(F32).to(F64)                                                 # rounded once, as the op returns it


def ref_nms(R, radius, mask=None, threshold=0.0):
    """numpy [B,1,*vol] float32 -> float32: the selection rule, offset by offset."""
    R = np.asarray(R, dtype=np.float32)
    vol = R.shape[2:]
    nd = len(vol)
    v = np.where(np.isnan(R), -np.inf, R).astype(np.float32)
    pad = np.pad(v, [(0, 0), (0, 0)] + [(radius, radius)] * nd, constant_values=-np.inf)
    sel = v > np.float32(threshold)
    if mask is not None:
        sel &= np.asarray(mask) != 0
    for d in itertools.product(range(-radius, radius + 1), repeat=nd):
        if not any(d):
            continue
        sl = (slice(None), slice(None)) + tuple(slice(radius + da, radius + da + n) for da, n in zip(d, vol))
        o = pad[sl]
        before = d < (0,) * nd                                               # lexicographic = the lower linear index
        sel &= ~((o > v) | ((o == v) & before))
    return np.where(sel, R, np.float32(0)).astype(np.float32)


def ref_select(peaks, K):
    """numpy: (pts [B,K,nd], weight [B,K]) by an explicit stable ordering."""
    B = peaks.shape[0]
    vol = peaks.shape[2:]
    nd = len(vol)
    pts = np.full((B, K, nd), np.nan, dtype=np.float32)
    wt = np.zeros((B, K), dtype=np.float32)
    for b in range(B):
        flat = peaks[b, 0].reshape(-1)
        cand = [(-float(flat[i]), i) for i in range(flat.size) if flat[i] > 0]
        cand.sort()
        for k, (nv, i) in enumerate(cand[:K]):
            pts[b, k] = np.unravel_index(i, vol)
            wt[b, k] = -nv
    return pts, wt


def ref_cost(fix, mov, pts, radius, step, patch, dtype=F64):
    """[B,K,D] in `dtype`: zero-padded volumes, one keypoint and one channel at a time."""
    B, C = fix.shape[:2]
    vol = tuple(fix.shape[2:])
    nd = len(vol)
    K = pts.shape[1]
    n, pw = 2 * radius + 1, 2 * patch + 1
    R0 = radius * step + patch
    padf = torch.nn.functional.pad(fix.to(dtype), (R0, R0) * nd)
    padm = torch.nn.functional.pad(mov.to(dtype), (R0, R0) * nd)
    out = torch.full((B, K, n ** nd), float('nan'), dtype=dtype)
    q = torch.round(pts)                                                     # ties to even
    for b in range(B):
        for k in range(K):
            if not torch.isfinite(pts[b, k]).all():
                continue
            qq = [int(v) for v in q[b, k]]
            if any(c < 0 or c >= s for c, s in zip(qq, vol)):
                continue
            acc = torch.zeros((n,) * nd, dtype=dtype)
            for c in range(C):
                # the fixed patch around q and the moving region around q (padded coordinates: q + R0 is the centre)
                fp = padf[b, c][tuple(slice(v + R0 - patch, v + R0 + patch + 1) for v in qq)]
                reg = padm[b, c][tuple(slice(v, v + 2 * R0 + 1) for v in qq)]
                for a in range(nd):
                    reg = reg.unfold(a, pw, 1)                               # [E-pw+1]*nd + [pw]*nd
                reg = reg[tuple(slice(None, None, step) for _ in range(nd))]  # [n]*nd + [pw]*nd
                acc += (fp - reg).square().sum(tuple(range(nd, 2 * nd)))
            out[b, k] = (acc / (C * pw ** nd)).reshape(-1)
    return out


def ref_argmin(cost, radius, step, nd, prior=None, coeff=0.0):
    """float64: (idx [B,K] int64, disp [B,K,nd], best, second) -- the two smallest finite penalised values per row."""
    n = 2 * radius + 1
    d = torch.stack(torch.meshgrid(*[torch.arange(-radius, radius + 1, dtype=F64)] * nd, indexing='ij'), -1).reshape(-1, nd)
    pen = cost.to(F64)
    if prior is not None:
        pen = pen + coeff * (step * d[None, None] - prior.to(F64)[:, :, None, :]).square().sum(-1)
    pen = torch.where(torch.isfinite(pen), pen, torch.full_like(pen, float('inf')))
    srt = torch.sort(pen, dim=2, stable=True)
    idx = srt.indices[..., 0]
    found = torch.isfinite(srt.values[..., 0])
    idx = torch.where(found, idx, torch.zeros_like(idx))
    disp = torch.where(found[..., None], step * d[idx], torch.full((1,), float('nan'), dtype=F64))
    return idx, disp, srt.values[..., 0], srt.values[..., 1]


def ref_tps_points(handle, pts):
    """The spline of a float64 ops.tps_fit handle (CPU) at pts [B,M,nd], float64 (ops.tps_fit states the definition)."""
    coef, ctrl = handle.coef.to(F64), handle.ctrl.to(F64)
    sc = torch.tensor(handle.scale, dtype=F64)
    K, nd = ctrl.shape[1], ctrl.shape[2]
    xh, qh = pts.to(F64) * sc, ctrl * sc
    s = (xh[:, :, None, :] - qh[:, None, :, :]).square().sum(-1)
    if nd == 3:
        phi = -s.sqrt()
    else:
        phi = torch.where(s > 0, 0.5 * s * torch.log(torch.where(s > 0, s, torch.ones_like(s))), torch.zeros_like(s))
    return phi @ coef[:, :K] + coef[:, K:K + 1] + xh @ coef[:, K + 1:]


def ref_coupling(cost, q, w, vol, radius, step, coeffs, smoothing, spacing=None):
    """The coupling loop of infer.keypoint_init in float64 on the CPU -> the list of (idx, disp, best, second) per argmin."""
    nd = len(vol)
    steps = [ref_argmin(cost, radius, step, nd)]
    q64 = q.to(F64)
    for c in coeffs:
        disp = steps[-1][1]
        handle = ops.tps_fit(q, (q64 + disp).to(F32), vol, spacing, smoothing, w)
        prior = ref_tps_points(handle, q64)                                  # a displacement; NaN for a padding point
        steps.append(ref_argmin(cost, radius, step, nd, prior, c))
    return steps


def smooth_noise(shape, seed, sigma=2.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g, dtype=F64)
    x = ref_gauss(x, sigma, F64)
    return (x / x.abs().max()).to(F32)


def image(shape, seed):
    """A seeded image with structure at several scales: smooth noise plus a little white noise."""
    g = torch.Generator().manual_seed(seed + 1000)
    return (smooth_noise(shape, seed, 1.5) + 0.05 * torch.randn(shape, generator=g)).to(F32)


# ------------------------------------------------------------------------------------------ cases
RESP_SHAPES = [(2, 1, 5, 6, 7), (1, 1, 2, 2, 2), (1, 1, 13, 17, 19), (2, 1, 9, 11), (1, 1, 37, 41), (1, 1, 17, 9, 65),
               (1, 1, 17, 65)]
RESP_CASES = [(s, sig, an) for s in RESP_SHAPES for sig in (0.0, 1.5, 5.0) for an in (False, True)]


def _rid(c):
    return "x".join(str(v) for v in c[0]) + "-sig%g-%s" % (c[1], "aniso" if c[2] else "iso")


@functools.lru_cache(maxsize=None)
def resp_case(shape, sigma, aniso):
    nd = len(shape) - 2
    I = image(shape, 11 + len(shape) + shape[-1])
    h = ANISO[nd] if aniso else (1.0,) * nd
    ref = ref_response(I, sigma, h, F64)
    e32 = float((ref_response(I, sigma, h, F32) - ref).abs().max())
    return I, h, ref, e32


# (feature shape, K, radius, step, patch)
COST_CASES = [
    ((2, 3, 9, 10, 11), 65, 1, 1, 0),
    ((1, 12, 13, 17, 19), 5, 8, 2, 2),
    ((1, 1, 2, 2, 2), 12, 2, 1, 3),
    ((1, 16, 7, 9, 8), 3, 8, 2, 2),
    ((1, 16, 6, 7, 9), 64, 1, 1, 3),
    ((1, 4, 5, 6, 7), 1, 8, 1, 0),
    ((1, 5, 9, 8, 7), 63, 3, 2, 1),
    ((2, 4, 11, 13), 64, 16, 1, 0),
    ((1, 3, 37, 41), 63, 1, 2, 3),
    ((1, 12, 9, 11), 65, 3, 2, 2),
    ((1, 16, 37, 41), 1, 16, 2, 3),
    ((1, 1, 2, 2), 12, 2, 2, 1),
]


def _cid(c):
    return "x".join(str(v) for v in c[0]) + "-K%d-r%d-s%d-p%d" % c[1:]


def special_points(vol):
    """Corners, faces, .5 coordinates (ties to even, both ways), and rows that must come back NaN."""
    nd = len(vol)
    top = [float(n - 1) for n in vol]
    mid = [float(n // 2) for n in vol]
    rows = [[0.0] * nd, top,
            [float('nan')] + mid[1:], mid[:-1] + [float('inf')], [-1.0] + mid[1:], mid[:-1] + [float(vol[-1])],
            [0.0] + top[1:], mid[:1] + [0.0] * (nd - 1), top[:1] + mid[1:],
            [0.5] * nd,                                  # -> 0
            [min(1.5, t) for t in top],                  # -> 2 where the volume has it, else the top face
            [t - 0.5 for t in top],                      # -> the even one of top - 1, top
            [-0.5] + mid[1:],                            # -> -0: inside
            [t + 0.5 for t in top]]                      # -> top (inside) or top + 1 (outside), by parity
    return torch.tensor(rows, dtype=F32)


@functools.lru_cache(maxsize=None)
def cost_case(shape, K, radius, step, patch):
    vol = shape[2:]
    g = torch.Generator().manual_seed(shape[1] * 100 + K)
    fix = torch.randn(shape, generator=g, dtype=F32)
    mov = (0.5 * fix + torch.randn(shape, generator=g, dtype=F32)).contiguous()
    pts = torch.rand((shape[0], K, len(vol)), generator=g, dtype=F32) * torch.tensor([n - 1 for n in vol], dtype=F32)
    sp = special_points(vol)
    if K >= 12:
        m = min(K - 1, len(sp))
        pts[-1, 1:1 + m] = sp[:m]
    ref = ref_cost(fix, mov, pts, radius, step, patch, F64)
    r32 = ref_cost(fix, mov, pts, radius, step, patch, F32).to(F64)
    live = torch.isfinite(ref)
    e32 = float((r32 - ref)[live].abs().max())
    return fix, mov, pts, ref, e32


def cost_bound(ref, e32):
    return FACTOR * e32 + FLOOR * float(ref[torch.isfinite(ref)].abs().max())


# (nd, radius) of D = 9, 25, 27, 1089, 4913
ARG_CASES = [(2, 1), (2, 2), (3, 1), (2, 16), (3, 8)]


@functools.lru_cache(maxsize=None)
def argmin_case(nd, radius, K):
    """Integer-valued cost rows with planted ties, NaN entries and all-NaN rows; a dyadic prior."""
    D = (2 * radius + 1) ** nd
    g = torch.Generator().manual_seed(D + K)
    cost = torch.randint(10, 50, (2, K, D), generator=g).to(F32)
    spots = [j for j in (0, 63, 64, 65, D - 1) if j < D]
    for t in range(2 * K):
        b, k = t % 2, t // 2                                                 # every row of both samples, another pair each
        pair = [spots[t % len(spots)], spots[(t // len(spots) + t + 1) % len(spots)]]
        cost[b, k, pair] = 1.0                                               # a tie (or one minimum) at lane-boundary positions
        if k % 5 == 3:
            cost[b, k, min(pair)] = float('nan')                             # the lower of the pair drops out
        if k % 7 == 4:
            cost[1 - b, k, ::3] = float('nan')
    if K > 1:
        cost[0, K - 1] = float('nan')                                        # an all-NaN row (K = 1 keeps its planted rows)
    if K > 2:
        cost[1, 1] = float('inf')                                            # a row without a finite entry
    prior = torch.randint(-4 * radius, 4 * radius + 1, (2, K, nd), generator=g).to(F32) / 4.0
    return cost, prior


def _noise_pair(vol, shift, seed):
    """fixed, moving [1,1,*vol] cut from one smooth noise volume so that fixed(x) = moving(x + shift) wherever both lie inside."""
    m = max(abs(s) for s in shift)
    big = smooth_noise((1, 1) + tuple(n + 2 * m for n in vol), seed, 1.5)
    fixed = big[(0, 0) + tuple(slice(m, m + n) for n in vol)]
    moving = big[(0, 0) + tuple(slice(m - s, m - s + n) for s, n in zip(shift, vol))]
    return moving[None, None].contiguous(), fixed[None, None].contiguous()


# (vol, shift, search_radius, search_step, patch, nms_radius, K, seed)
SHIFT_CASES = [((40, 44, 48), (4, -6, 2), 3, 2, 2, 2, 64, 3), ((64, 72), (-4, 6), 4, 2, 2, 2, 32, 5)]
SHIFT_SIGMA = 1.0


def band_mask(vol, band):
    m = torch.zeros((1, 1) + tuple(vol), dtype=F32)
    m[(0, 0) + tuple(slice(band, n - band) for n in vol)] = 1.0
    return m


# ------------------------------------------------------------------------------------------ CPU tier
def test_restatement_nms_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    g = np.random.default_rng(0)
    for vol, r in (((7, 9, 8), 1), ((7, 9, 8), 2), ((23, 19), 3), ((5, 4), 8)):
        R = g.permutation(int(np.prod(vol))).astype(np.float32).reshape((1, 1) + vol) + 1.0     # distinct, positive
        want = np.where(ndi.maximum_filter(R[0, 0], size=2 * r + 1, mode='constant', cval=-np.inf) == R[0, 0], R[0, 0], 0)
        assert np.array_equal(ref_nms(R, r)[0, 0], want)


def test_restatement_gauss_against_scipy_interior():
    ndi = pytest.importorskip("scipy.ndimage")
    x = torch.randn(1, 1, 21, 23, 25, dtype=F64, generator=torch.Generator().manual_seed(1))
    sigma, r = 1.5, 5
    got = ref_gauss(x, sigma, F64)[0, 0].numpy()
    want = ndi.gaussian_filter(x[0, 0].numpy(), sigma, truncate=3.0, mode='constant')
    inner = (slice(r, -r),) * 3
    # the restatement's weights are rounded to fp32 (part of the op's definition): 2^-24 relative per weight
    assert np.abs(got[inner] - want[inner]).max() <= 4 * 2.0 ** -24 * np.abs(want).max()


def test_restatement_response_properties():
    # a constant image and a pure ramp have a singular structure tensor: the response is exactly 0
    c = torch.full((1, 1, 6, 7, 8), 3.0)
    assert float(ref_response(c, 1.5, (1.0,) * 3).abs().max()) == 0.0
    ramp = torch.arange(8.0).view(1, 1, 1, 8).expand(1, 1, 7, 8).contiguous()
    assert float(ref_response(ramp, 0.0, (1.0, 1.0)).abs().max()) == 0.0
    # an isotropic blob responds at its flanks and the response scales with the squared gradient: R(2 I) = 4 R(I)
    I = image((1, 1, 9, 10, 11), 2)
    a, b = ref_response(I, 1.5, (1.0,) * 3), ref_response(2 * I, 1.5, (1.0,) * 3)
    assert float(a.max()) > 0 and torch.allclose(b, 4 * a, rtol=1e-6, atol=0)


def test_restatement_cost_against_brute_force():
    g = torch.Generator().manual_seed(4)
    fix, mov = torch.randn(1, 2, 5, 6, generator=g), torch.randn(1, 2, 5, 6, generator=g)
    pts = torch.tensor([[[0.0, 5.0], [2.5, 3.5], [4.0, 0.0]]])
    r, step, patch = 2, 2, 1
    got = ref_cost(fix, mov, pts, r, step, patch)

    def rd(t, c, y, x):
        return float(t[0, c, y, x]) if 0 <= y < 5 and 0 <= x < 6 else 0.0
    for k, (qy, qx) in enumerate(((0, 5), (2, 4), (4, 0))):
        j = 0
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                s = sum((rd(fix, c, qy + oy, qx + ox) - rd(mov, c, qy + oy + step * dy, qx + ox + step * dx)) ** 2
                        for c in range(2) for oy in (-1, 0, 1) for ox in (-1, 0, 1)) / 18.0
                assert abs(float(got[0, k, j]) - s) <= 1e-12 * max(s, 1.0)
                j += 1


def test_select_keypoints_order_ties_padding():
    p = torch.zeros(2, 1, 3, 4, 5)
    p[0, 0, 2, 3, 4] = 7.0
    p[0, 0, 0, 1, 2] = 7.0                   # a tie: the lower linear index first
    p[0, 0, 1, 0, 0] = 9.0
    p[0, 0, 1, 1, 1] = -2.0                  # negative, NaN and zero entries are no peaks
    p[0, 0, 2, 0, 0] = float('nan')
    p[1, 0, 0, 0, 3] = 1.0
    pts, w = ops.select_keypoints(p, 4)
    assert pts.dtype == F32 and w.dtype == F32 and tuple(pts.shape) == (2, 4, 3) and tuple(w.shape) == (2, 4)
    assert w.tolist() == [[9.0, 7.0, 7.0, 0.0], [1.0, 0.0, 0.0, 0.0]]
    assert pts[0, :3].tolist() == [[1.0, 0.0, 0.0], [0.0, 1.0, 2.0], [2.0, 3.0, 4.0]]
    assert pts[1, 0].tolist() == [0.0, 0.0, 3.0]
    assert torch.isnan(pts[0, 3]).all() and torch.isnan(pts[1, 1:]).all()
    # K above the number of voxels pads as well; 2-D; against the explicit ordering
    g = torch.Generator().manual_seed(0)
    q = torch.randint(0, 4, (2, 1, 5, 6), generator=g).to(F32)             # many ties, many zeros
    for K in (1, 7, 30, 64):
        pts, w = ops.select_keypoints(q, K)
        rp, rw = ref_select(q.numpy(), K)
        assert np.array_equal(w.numpy(), rw) and np.array_equal(pts.numpy(), rp, equal_nan=True)


def _raises(fn, *a, **k):
    with pytest.raises(ValueError):
        fn(*a, **k)


def test_value_errors_response_nms_select():
    I = torch.zeros(1, 1, 4, 5, 6)
    for bad in (torch.zeros(1, 2, 4, 5, 6), torch.zeros(4, 5, 6), torch.zeros(1, 1, 1, 5, 6), I.double(), "x",
                torch.zeros(1, 1, 4, 5, 6, requires_grad=True)):
        _raises(ops.foerstner_response, bad)
        _raises(ops.local_maxima, bad, 1)
    for sig in (-1.0, float('nan'), float('inf'), (1.0, 1.0), 6.0, "a"):
        _raises(ops.foerstner_response, I, sig)
    for sp in ((1.0, 1.0), (1.0, 0.0, 1.0), (1.0, -1.0, 1.0), (1.0, float('nan'), 1.0), "abc", 2.0):
        _raises(ops.foerstner_response, I, 1.5, sp)
    for r in (0, 9, 1.0, True, None):
        _raises(ops.local_maxima, I, r)
    for m in (torch.zeros(1, 1, 4, 5, 5), torch.zeros(1, 4, 5, 6), I.double(), "m"):
        _raises(ops.local_maxima, I, 1, m)
    for t in (float('nan'), float('inf'), -float('inf'), "0", None, True, 1e39):
        _raises(ops.local_maxima, I, 1, None, t)
    with pytest.raises(DfmirHipError, match="no CPU fallback"):
        ops.foerstner_response(I)
    with pytest.raises(DfmirHipError, match="no CPU fallback"):
        ops.local_maxima(I, 1)
    for bad in (torch.zeros(1, 2, 4, 5), torch.zeros(4, 5), torch.zeros(1, 1, 4, 5, dtype=torch.int32), None):
        _raises(ops.select_keypoints, bad, 4)
    for K in (0, -1, ops.LANDMARK_MAX_K + 1, 2.0, True):
        _raises(ops.select_keypoints, torch.zeros(1, 1, 4, 5), K)


def test_value_errors_cost_argmin():
    f3, f2 = torch.zeros(1, 3, 4, 5, 6), torch.zeros(1, 3, 5, 6)
    p3, p2 = torch.zeros(1, 7, 3), torch.zeros(1, 7, 2)
    for fix, mov in ((torch.zeros(1, 17, 4, 5, 6),) * 2, (f3, torch.zeros(1, 3, 4, 5, 7)), (f3.double(),) * 2, (f3, "m"),
                     (torch.zeros(1, 3, 1, 5, 6),) * 2, (torch.zeros(3, 4, 5),) * 2,
                     (torch.zeros(1, 3, 4, 5, 6, requires_grad=True), f3), (f3, torch.zeros(1, 3, 4, 5, 6, requires_grad=True))):
        _raises(ops.keypoint_cost, fix, mov, p3, 1)
    for pts in (p2, torch.zeros(2, 7, 3), torch.zeros(7, 3), torch.zeros(1, 0, 3), p3.double(), None,
                torch.zeros(1, 7, 3, requires_grad=True)):
        _raises(ops.keypoint_cost, f3, f3, pts, 1)
    for r in (0, 9, 1.0, True):
        _raises(ops.keypoint_cost, f3, f3, p3, r)
    for r in (0, 17):
        _raises(ops.keypoint_cost, f2, f2, p2, r)
    for s in (0, 5, 1.0, True):
        _raises(ops.keypoint_cost, f3, f3, p3, 1, s)
    for p in (-1, 4, 1.0, True):
        _raises(ops.keypoint_cost, f3, f3, p3, 1, 1, p)
    assert ops.KEYPOINT_MAX_EXTENT == 96 and ops.KEYPOINT_MAX_RADIUS == {2: 16, 3: 8}
    assert (ops.KEYPOINT_NMS_MAX_RADIUS, ops.KEYPOINT_MAX_STEP, ops.KEYPOINT_MAX_PATCH) == (8, 4, 3)
    _raises(ops.keypoint_cost, f2, f2, p2, 16, 3, 0)                        # E = 97: beyond the staged extent, no fallback
    _raises(ops.keypoint_cost, f2, f2, p2, 12, 4, 3)                        # E = 103
    big = torch.zeros(1, 1, 2, 2, 2).expand(110, 1, 2, 2, 2)
    _raises(ops.keypoint_cost, big, big, torch.zeros(1, 4096, 3).expand(110, 4096, 3), 8)      # B K D >= 2^31
    with pytest.raises(DfmirHipError, match="no CPU fallback"):
        ops.keypoint_cost(f3, f3, p3, 1)

    c3, c2 = torch.zeros(1, 7, 27), torch.zeros(1, 7, 9)
    for cost in (torch.zeros(7, 27), torch.zeros(1, 0, 27), c3.double(), "c", torch.zeros(1, 7, 27, requires_grad=True),
                 torch.zeros(1, 7, 26)):
        _raises(ops.keypoint_argmin, cost, 1)
    for r in (0, 2, 9, 1.0, True):
        _raises(ops.keypoint_argmin, c3, r)
    _raises(ops.keypoint_argmin, torch.zeros(1, 1, 35 ** 2), 17)
    for s in (0, 5, 1.0, True):
        _raises(ops.keypoint_argmin, c3, 1, s)
    for pr in (p2, torch.zeros(1, 6, 3), torch.zeros(7, 3), p3.double(), "p", torch.zeros(1, 7, 3, requires_grad=True)):
        _raises(ops.keypoint_argmin, c3, 1, 1, pr)
    _raises(ops.keypoint_argmin, c2, 1, 1, p3)
    for co in (-1.0, float('nan'), float('inf'), "x", None):
        _raises(ops.keypoint_argmin, c3, 1, 1, p3, co)
    with pytest.raises(DfmirHipError, match="no CPU fallback"):
        ops.keypoint_argmin(c3, 1)
    with pytest.raises(DfmirHipError, match="no CPU fallback"):
        ops.keypoint_argmin(c2, 1, 2, p2, 0.5)


def test_value_errors_keypoint_init():
    a = torch.zeros(1, 1, 8, 9, 10)
    ki = infer.keypoint_init
    _raises(ki, a, torch.zeros(1, 1, 8, 9, 11))
    _raises(ki, a, "b")
    _raises(ki, torch.zeros(8, 9, 10), torch.zeros(8, 9, 10))
    _raises(ki, a, a, interp='nearest')
    _raises(ki, a, a, features='sift')
    _raises(ki, torch.zeros(1, 2, 8, 9, 10), torch.zeros(1, 2, 8, 9, 10))
    _raises(ki, torch.zeros(1, 2, 8, 9, 10), torch.zeros(1, 2, 8, 9, 10), features=(a, a))
    _raises(ki, a, a, features=(a, torch.zeros(1, 1, 8, 9, 11)))
    for kw in (dict(num_keypoints=0), dict(num_keypoints=4097), dict(mask=torch.zeros(1, 1, 8, 9, 10, dtype=F64)),
               dict(mask=torch.zeros(1, 1, 8, 9, 10, requires_grad=True)), dict(num_keypoints=8.0), dict(sigma=-1.0), dict(sigma=6.0),
               dict(nms_radius=0), dict(nms_radius=9), dict(mask=torch.zeros(1, 1, 8, 9, 11)), dict(mask="m"),
               dict(threshold=float('nan')), dict(threshold="t"), dict(search_radius=0), dict(search_radius=9),
               dict(search_step=0), dict(search_step=5), dict(patch=-1), dict(patch=4), dict(coeffs=(0.1, -1.0)),
               dict(coeffs=(float('inf'),)), dict(coeffs=3.0), dict(coeffs=("a",)), dict(smoothing=-1.0),
               dict(smoothing=float('nan')), dict(smoothing="s"), dict(spacing=(1.0, 1.0)), dict(spacing=(1.0, 0.0, 1.0))):
        _raises(ki, a, a, features='intensity', **kw)
    b = torch.zeros(1, 1, 9, 10)
    _raises(ki, b, b, features='intensity', search_radius=17)
    _raises(ki, b, b, features='intensity', search_radius=16, search_step=3, patch=0)          # E = 97
    with pytest.raises(DfmirHipError, match="no CPU fallback"):
        ki(a, a, features='intensity')


@pytest.mark.parametrize("case", SHIFT_CASES, ids=lambda c: "x".join(str(v) for v in c[0]))
def test_shift_seed_yields_keypoints_cpu(case):
    """The chosen seeds give the exact-shift test its nd + 1 keypoints, and more: by the restatement, without a GPU."""
    vol, shift, r, step, patch, nms_r, K, seed = case
    moving, fixed = _noise_pair(vol, shift, seed)
    sl = tuple(slice(max(0, -s), min(n, n - s)) for s, n in zip(shift, vol))
    assert torch.equal(fixed[(0, 0) + sl], moving[(0, 0) + tuple(slice(a.start + s, a.stop + s) for a, s in zip(sl, shift))])
    R = ref_response(fixed, SHIFT_SIGMA, (1.0,) * len(vol)).to(F32).numpy()
    peaks = ref_nms(R, nms_r, band_mask(vol, r * step + patch).numpy(), 0.0)
    assert int((peaks > 0).sum()) >= 2 * (len(vol) + 1)


# ------------------------------------------------------------------------------------------ GPU tier
gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("case", RESP_CASES, ids=_rid)
def test_response_against_restatement(case):
    I, h, ref, e32 = resp_case(*case)
    got = ops.foerstner_response(I.to(DEV), case[1], None if not case[2] else h).cpu().to(F64)
    assert got.shape == ref.shape
    err = float((got - ref).abs().max())
    bound = FACTOR * e32 + FLOOR * float(ref.abs().max())
    print("response %s: err %.3e e32 %.3e bound %.3e max|R| %.3e" % (_rid(case), err, e32, bound, float(ref.abs().max())))
    assert torch.isfinite(got).all() and err <= bound


@gpu
@pytest.mark.parametrize("shape", RESP_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("aniso", (False, True), ids=("iso", "aniso"))
def test_products_bitwise(shape, aniso):
    """The product planes (what sigma = 0 hands to the response kernel) against the fp32 CPU evaluation, bit for bit."""
    from dfmir_amd._lib import check, lib
    nd = len(shape) - 2
    I = image(shape, 11 + len(shape) + shape[-1])
    h = ANISO[nd] if aniso else (1.0,) * nd
    g = []
    for a in range(nd):
        n = shape[a + 2]
        ip, im = torch.arange(n).add(1).clamp(max=n - 1), torch.arange(n).sub(1).clamp(min=0)
        two_h = torch.tensor([2.0 * float(np.float32(h[a]))], dtype=F32)
        g.append((I.index_select(a + 2, ip) - I.index_select(a + 2, im)) / two_h)
    want = torch.cat([g[a] * g[b] for a in range(nd) for b in range(a, nd)], 1)
    x = I.to(DEV)
    got = torch.empty(want.shape, device=DEV, dtype=F32)
    D, H, W = (1,) * (3 - nd) + tuple(shape[2:])
    hz, hy, hx = (1.0,) * (3 - nd) + tuple(h)
    check(lib().dfmir_keypoint_products(nd, ops._p(x), ops._p(got), shape[0], D, H, W, hz, hy, hx, ops._st()))
    assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))


@gpu
def test_response_nonfinite_and_repeat():
    I = image((1, 1, 9, 10, 11), 5).clone()
    I[0, 0, 4, 5, 6] = float('nan')
    I[0, 0, 0, 0, 0] = float('inf')
    x = I.to(DEV)
    R = ops.foerstner_response(x, 1.5)
    assert torch.isfinite(R).all()                                           # 0 where anything is non-finite
    assert float(R[0, 0, 4, 5, 6]) == 0.0 and float(R[0, 0, 0, 0, 0]) == 0.0
    assert torch.equal(R, ops.foerstner_response(x, 1.5))
    with pytest.raises(ValueError):
        ops.foerstner_response(x.requires_grad_(True))


def nms_inputs():
    """(name, R numpy [B,1,*vol], mask or None, threshold)"""
    out = []
    g = np.random.default_rng(3)
    for shape in RESP_SHAPES:
        vol = shape[2:]
        R = g.integers(0, 6, size=shape).astype(np.float32)                  # integer values: plateaus everywhere
        planted = R.copy()
        sl = (0, 0) + tuple(slice(n // 3, n // 3 + 3) for n in vol)
        planted[sl] = 9.0                                                    # a 3^nd plateau of the maximum
        out.append(("int-" + "x".join(map(str, shape)), planted, None, 0.0))
        out.append(("thr-" + "x".join(map(str, shape)), planted, None, 5.0))  # a value that is present: strict >
        m = (g.random(shape) > 0.3).astype(np.float32)
        out.append(("mask-" + "x".join(map(str, shape)), planted, m, 0.0))
        out.append(("const-" + "x".join(map(str, shape)), np.full(shape, 2.0, dtype=np.float32), None, 0.0))
        real = g.standard_normal(shape).astype(np.float32)
        real[(0, 0) + tuple(n // 2 for n in vol)] = np.nan
        real[(0, 0) + (0,) * len(vol)] = np.nan
        real[(0, 0) + tuple(n - 1 for n in vol)] = np.inf
        out.append(("nan-" + "x".join(map(str, shape)), real, None, -0.5))
    return out


NMS_INPUTS = nms_inputs()


@gpu
@pytest.mark.parametrize("radius", (1, 2, 8))
def test_nms_bit_exact(radius):
    for name, R, m, thr in NMS_INPUTS:
        want = ref_nms(R, radius, m, thr)
        got = ops.local_maxima(torch.from_numpy(R).to(DEV), radius, None if m is None else torch.from_numpy(m).to(DEV), thr)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), (name, radius)
        if name.startswith("const"):                                         # exactly the voxel of lowest index survives
            flat = got.cpu().numpy().reshape(R.shape[0], -1)
            assert (flat[:, 0] == 2.0).all() and (flat[:, 1:] == 0.0).all()


@gpu
@pytest.mark.parametrize("case", COST_CASES, ids=_cid)
def test_cost_against_restatement(case):
    fix, mov, pts, ref, e32 = cost_case(*case)
    got = ops.keypoint_cost(fix.to(DEV), mov.to(DEV), pts.to(DEV), *case[2:])
    again = ops.keypoint_cost(fix.to(DEV), mov.to(DEV), pts.to(DEV), *case[2:])
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))       # bit-identical from run to run
    got = got.cpu().to(F64)
    live = torch.isfinite(ref)
    assert torch.equal(torch.isnan(got), ~live)                              # NaN rows: where the restatement has them
    if case[1] >= 12:
        assert int((~live).all(2).sum()) >= 4                                # the special points did produce NaN rows
    err = float((got - ref)[live].abs().max())
    bound = cost_bound(ref, e32)
    print("cost %s: err %.3e e32 %.3e bound %.3e max %.3e" % (_cid(case), err, e32, bound, float(ref[live].abs().max())))
    assert err <= bound


@gpu
def test_cost_outside_reads_tie_bitwise():
    """Displacements whose moving reads all fall outside the volume give one bit pattern: sum fix^2 / (C P) in one order."""
    g = torch.Generator().manual_seed(9)
    fix, mov = torch.randn(1, 5, 4, 4, 4, generator=g), torch.randn(1, 5, 4, 4, 4, generator=g)
    pts = torch.tensor([[[1.0, 2.0, 1.0]]])
    r, step, patch = 8, 2, 1
    c = ops.keypoint_cost(fix.to(DEV), mov.to(DEV), pts.to(DEV), r, step, patch).cpu()[0, 0].view(17, 17, 17)
    far = c[0].reshape(-1)                                                   # dz = -8: 16 voxels below a 4-voxel volume
    assert (far.view(torch.int32) == far.view(torch.int32)[0]).all()
    assert torch.equal(c[-1].reshape(-1).view(torch.int32), far.view(torch.int32))


@gpu
@pytest.mark.parametrize("K", (1, 65))
@pytest.mark.parametrize("nd,radius", ARG_CASES)
def test_argmin_exact(nd, radius, K):
    cost, prior = argmin_case(nd, radius, K)
    cd = cost.to(DEV)
    for step, pr, coeff in ((1, None, 0.0), (2, prior, 0.0), (1, prior, 0.25), (2, prior, 0.5)):
        idx, disp = ops.keypoint_argmin(cd, radius, step, None if pr is None else pr.to(DEV), coeff)
        ri, rd, _, _ = ref_argmin(cost, radius, step, nd, pr, coeff)
        assert idx.dtype == torch.int32 and tuple(idx.shape) == (2, K) and tuple(disp.shape) == (2, K, nd)
        assert torch.equal(idx.cpu().long(), ri), (step, coeff)
        assert torch.equal(torch.isnan(disp.cpu()), torch.isnan(rd))
        assert torch.equal(torch.nan_to_num(disp.cpu().to(F64), nan=-99.0), torch.nan_to_num(rd, nan=-99.0))
    if K > 1:
        assert torch.isnan(disp[0, K - 1]).all() and int(idx[0, K - 1]) == 0  # the all-NaN row


@gpu
@pytest.mark.parametrize("case", SHIFT_CASES, ids=lambda c: "x".join(str(v) for v in c[0]))
def test_exact_shift_recovery(case):
    vol, shift, r, step, patch, nms_r, K, seed = case
    nd = len(vol)
    mv, fx = _noise_pair(vol, shift, seed)
    moving, fixed = mv.to(DEV), fx.to(DEV)
    mask = band_mask(vol, r * step + patch).to(DEV)
    s = torch.tensor(shift, dtype=F32, device=DEV)
    coeffs, lam = infer.CONVEX_COEFFS, 1e-3
    # the pipeline op by op: the plain argmin and every coupling step return the shift exactly
    q, w = ops.select_keypoints(ops.local_maxima(ops.foerstner_response(fixed, SHIFT_SIGMA), nms_r, mask, 0.0), K)
    valid = w > 0
    assert int(valid.sum()) >= nd + 1
    cost = ops.keypoint_cost(fixed, moving, q, r, step, patch)
    idx, disp = ops.keypoint_argmin(cost, r, step)
    assert torch.equal(disp[valid], s.expand_as(disp)[valid]) and torch.isnan(disp[~valid]).all()
    for c in coeffs:
        prior = ops.tps_points(ops.tps_fit(q, q + disp, vol, None, lam, w), q)
        idx, disp = ops.keypoint_argmin(cost, r, step, prior, c)
        assert torch.equal(disp[valid], s.expand_as(disp)[valid]), c
    out = infer.keypoint_init(moving, fixed, features='intensity', num_keypoints=K, sigma=SHIFT_SIGMA, nms_radius=nms_r,
                              mask=mask, threshold=0.0, search_radius=r, search_step=step, patch=patch, smoothing=lam)
    assert torch.equal(out['fixed_pts'].isnan(), q.isnan()) and torch.equal(out['fixed_pts'][valid], q[valid])
    assert torch.equal(out['weight'], w) and torch.equal(out['idx'], idx)
    assert torch.equal(out['moving_pts'][valid], (q + s)[valid])
    ref = infer.landmark_init(moving, fixed, q, q + s, smoothing=lam, weight=w)
    for name in ('flow', 'warped', 'tre'):
        assert torch.equal(out[name].view(torch.int32), ref[name].view(torch.int32)), name
    # the flow is the shift, and the warped image the fixed one, wherever the moving image has the voxel
    assert float((out['flow'] - s.view(1, nd, *([1] * nd))).abs().max()) < 1e-3


DEFORM = dict(vol=(32, 36, 40), seed=7, amp=5.0, K=64, sigma=1.5, nms_radius=2, search_radius=4, search_step=2, patch=2,
              smoothing=1e-3)


def deform_pair(vol, seed, amp):
    """fixed [1,1,*vol] and the sinusoidal field u [1,3,*vol] (|u_a| <= amp) with moving = ops.warp(fixed, u)."""
    fixed = image((1, 1) + vol, seed)
    zz, yy, xx = torch.meshgrid(*[torch.arange(n, dtype=F64) / (n - 1) for n in vol], indexing='ij')
    g = torch.Generator().manual_seed(seed)
    ph = torch.rand(3, 3, generator=g, dtype=F64) * 2 * math.pi
    u = torch.stack([amp * torch.sin(2 * math.pi * zz * 0.5 + ph[a, 0]) * torch.cos(math.pi * yy + ph[a, 1])
                     * torch.cos(math.pi * xx * 0.7 + ph[a, 2]) for a in range(3)])[None]
    return fixed, u.to(F32)


@gpu
def test_smooth_deformation_against_restatement():
    P = DEFORM
    vol, r, step, patch = P['vol'], P['search_radius'], P['search_step'], P['patch']
    fixed, u = deform_pair(vol, P['seed'], P['amp'])
    fixed, u = fixed.to(DEV), u.to(DEV)
    moving = ops.warp(fixed, u)
    Mm, Mf = ops.mind_descriptor(moving, 2, 2), ops.mind_descriptor(fixed, 2, 2)
    out = infer.keypoint_init(moving, fixed, features=(Mm, Mf), num_keypoints=P['K'], sigma=P['sigma'],
                              nms_radius=P['nms_radius'], search_radius=r, search_step=step, patch=patch,
                              smoothing=P['smoothing'])
    q, w = out['fixed_pts'].cpu(), out['weight'].cpu()
    valid = w > 0
    assert int(valid.sum()) >= 16
    # the restatement from keypoint_cost on, on the GPU's keypoints and features
    fm, ff = Mm.cpu(), Mf.cpu()
    rc = ref_cost(ff, fm, q, r, step, patch, F64)
    e32 = float((ref_cost(ff, fm, q, r, step, patch, F32).to(F64) - rc)[torch.isfinite(rc)].abs().max())
    bound = cost_bound(rc, e32)
    steps = ref_coupling(rc, q, w, vol, r, step, infer.CONVEX_COEFFS, P['smoothing'])
    ri, rd, best, second = steps[-1]
    close = (second - best) < 2 * bound
    share = float((close & valid).sum()) / float(valid.sum())
    print("deformation: %d keypoints, cost bound %.3e, left out %.1f %%" % (int(valid.sum()), bound, 100 * share))
    assert share <= 0.05
    keep = valid & ~close
    assert torch.equal(out['idx'].cpu().long()[keep], ri[keep])
    assert torch.equal(out['moving_pts'].cpu().to(F64)[keep], (q.to(F64) + rd)[keep])
    assert torch.isnan(out['moving_pts'].cpu()[~valid]).all()
