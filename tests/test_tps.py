"""Thin-plate-spline landmark interpolation: ops.tps_fit / ops.tps_flow / ops.tps_points / infer.landmark_init (build-defined,
dfmir_amd/csrc/tps.hip).  CPU: a float64 restatement of the definition in plain torch (explicit per-axis differences, the
system solved on the VALID SUBSET of the points, so the padding rule of ops.tps_fit is checked against something that never
forms a padded row), checked against scipy.interpolate.RBFInterpolator and against ops.tps_fit; the interpolation property;
every argument check.  GPU: the kernels against the restatement.

Sizes of the kernels: TPS_T = 256 threads per workgroup = control points per LDS chunk of the forward = voxels per LDS tile
and control points per workgroup of the adjoint; TPS_V = 4 voxels (points) per thread of the forward along x.  So K runs over
nd + 1 (the smallest legal: a pure affine fit), 255 / 256 / 257 (a chunk short of full, full, two chunks with one point in the
second), 513 (three chunks) and 4096 (the maximum, once, with smoothing > 0); B = 2 at K = 257 has a sample boundary between
chunks.  The volumes have x extents 5, 19, 2, 11, 41, 2 -- none a multiple of 4, one smaller than 4 -- the one-cell volume and
odd strides; both spacings.  The adjoint's slabs: 2048 / (control blocks * B) of them, at least one tile each, so those volumes
give 1 to 17 slabs of ONE tile, the last one partial; two more cases (B = 16, 25 x 26 x 27 and 129 x 131, K = 257) give slabs of
two tiles, which no volume of the list above reaches.

Point sets (all seeded, positions uniform in the volume): 'smooth' = a product of sinusoids of the normalised position,
amplitude 3 voxels; 'noisy' = smooth + 0.3 voxel of noise, fitted with smoothing > 0; 'rough' = independent noise, sigma 2;
'pad' = smooth with weight-0, NaN and infinite entries; 'affine' = p = A q + t.

Tolerances, PER CASE (profiles/tps_margins.txt lists them beside the kernels' own errors): e32 = the error of the same
definition evaluated by torch in fp32 on the CPU, coefficients rounded to fp32, against the float64 restatement.  The kernel's
max-abs flow error is bounded by 4 e32 + 4 * 2^-23 max|u|, dcoef by the same rule in relative 2-norm.  The fp32 error runs
over four decades between a smooth and a rough set, so one maximum over the cases would let a kernel wrong by 1e-3 pass every
smooth one.  The factor 4 is the project's usual margin over the fp32 CPU evaluation (tests/test_landmarks.py); the floor keeps
the affine case from a zero bound."""
import functools
import math

import pytest
import torch

import dfmir_amd
from dfmir_amd import infer, ops
from dfmir_amd._lib import DfmirHipError

DEV = "cuda"
FACTOR = 4.0
FLOOR = 4.0 * 2.0 ** -23
TPS_T = 256                                  # control points per LDS chunk of tps_fwd_k, voxels per tile of tps_bwd_k (tps.hip)
TPS_V = 4                                    # voxels per thread of tps_fwd_k
MAX_K = 4096
F64 = torch.float64

ANISO = {3: (2.5, 1.0, 0.7), 2: (0.7, 1.6)}
VOLS = {3: [(2, 3, 3, 4, 5), (1, 3, 13, 17, 19), (1, 3, 2, 2, 2)], 2: [(2, 2, 9, 11), (1, 2, 37, 41), (1, 2, 2, 2)]}
BIG = {3: (1, 3, 13, 17, 19), 2: (1, 2, 37, 41)}
LAM = 1e-3


def _cases():
    """(flow shape, K, kind, anisotropic, smoothing)"""
    out = []
    for nd in (3, 2):
        for i, s in enumerate(VOLS[nd]):
            out.append((s, nd + 1, 'smooth', bool(i & 1), 0.0))
            out.append((s, TPS_T + 1, 'smooth', not (i & 1), 0.0))             # (B = 2 on the first volume of each nd)
        out.append((BIG[nd], TPS_T - 1, 'noisy', False, LAM))
        out.append((BIG[nd], TPS_T, 'rough', True, 0.0))
        out.append((BIG[nd], 2 * TPS_T + 1, 'smooth', True, 0.0))
        out.append((BIG[nd], TPS_T + 1, 'pad', False, 0.0))
        out.append((VOLS[nd][0], 64, 'pad', True, LAM))
        out.append((BIG[nd], TPS_T + 1, 'affine', nd == 3, 0.0))
    out.append((BIG[3], MAX_K, 'noisy', False, 1e-2))
    # slabs of the adjoint with MORE than one tile: 2 control blocks * 16 samples leave 64 slabs for > 64 * 256 voxels
    out.append(((16, 3, 25, 26, 27), TPS_T + 1, 'smooth', False, 0.0))
    out.append(((16, 2, 129, 131), TPS_T + 1, 'smooth', True, 0.0))
    return out


CASES = _cases()


def _id(case):
    return "x".join(str(v) for v in case[0]) + "-K%d-%s-%s-lam%g" % (case[1], case[2], "aniso" if case[3] else "iso", case[4])


# ------------------------------------------------------------------------------------------ restatement
def scale_of(vol, h):
    L = max(ha * (n - 1) for ha, n in zip(h, vol))
    return [ha / L for ha in h]


def phi_of_s(s, nd):
    """phi as a function of s = r^2: -sqrt(s) in 3-D, 1/2 s log s with phi(0) = 0 in 2-D."""
    if nd == 3:
        return -torch.sqrt(s)
    pos = s > 0
    return torch.where(pos, 0.5 * s * torch.log(torch.where(pos, s, torch.ones_like(s))), torch.zeros_like(s))


def sqdist(x, y):
    """[N,nd], [K,nd] -> [N,K]: the squared distances, axis by axis."""
    s = None
    for a in range(x.shape[1]):
        d = x[:, a, None] - y[None, :, a]
        s = d * d if s is None else s + d * d
    return s


def valid_of(q, p, w):
    v = torch.isfinite(q).all(-1) & torch.isfinite(p).all(-1)
    return v if w is None else v & (w != 0)


def ref_fit(q, p, vol, h, lam=0.0, w=None):
    """The float64 coefficients [B,K+nd+1,nd] and the normalised control positions [B,K,nd] (0 for a padding entry) of the
    definition, on the CPU: per sample the system of the valid points alone.  Differentiable with respect to p."""
    B, K, nd = q.shape
    sc = torch.tensor(scale_of(vol, h), dtype=F64)
    valid = valid_of(q, p, w)
    coefs, qhs = [], []
    for b in range(B):
        idx = valid[b].nonzero()[:, 0]
        n = len(idx)
        qv = q[b, idx].to(F64) * sc
        d = p[b, idx].to(F64) - q[b, idx].to(F64)
        M = torch.zeros(n + nd + 1, n + nd + 1, dtype=F64)
        M[:n, :n] = phi_of_s(sqdist(qv, qv), nd)
        if lam:
            M[:n, :n] += torch.diag(lam / (torch.ones(n, dtype=F64) if w is None else w[b, idx].to(F64)))
        P = torch.cat([torch.ones(n, 1, dtype=F64), qv], 1)
        M[:n, n:] = P
        M[n:, :n] = P.t()
        c = torch.linalg.solve(M, torch.cat([d, torch.zeros(nd + 1, nd, dtype=F64)], 0))
        rows = torch.zeros(K, n, dtype=F64)
        rows[idx, torch.arange(n)] = 1.0
        coefs.append(torch.cat([rows @ c[:n], c[n:]], 0))
        qhs.append(rows @ qv)
    return torch.stack(coefs), torch.stack(qhs)


def ref_eval(coef, qh, xh):
    """u [B,N,nd] at normalised positions xh [B,N,nd] (or [N,nd] for every sample), in the dtype of coef."""
    B, K, nd = qh.shape
    out = []
    for b in range(B):
        x = xh if xh.dim() == 2 else xh[b]
        out.append(phi_of_s(sqdist(x, qh[b]), nd) @ coef[b, :K] + coef[b, K] + x @ coef[b, K + 1:])
    return torch.stack(out)


def grid_of(vol, dtype=F64):
    ax = [torch.arange(n, dtype=dtype) for n in vol]
    return torch.stack(torch.meshgrid(*ax, indexing='ij'), -1).reshape(-1, len(vol))


def as_flow(u, vol):
    return u.transpose(1, 2).reshape(u.shape[0], len(vol), *vol)


def eval_at(coef, q_ctrl, pts, vol, h, dtype):
    """The definition at voxel positions pts ([N,nd] or [B,N,nd]) in `dtype` (float64: the restatement; float32 with coef
    rounded to fp32: the yardstick): normalised coordinates formed in that dtype too.  q_ctrl: sanitised voxel positions."""
    sc = torch.tensor(scale_of(vol, h), dtype=dtype)
    return ref_eval(coef.to(dtype), q_ctrl.to(dtype) * sc, pts.to(dtype) * sc)


# ------------------------------------------------------------------------------------------ point sets
def make_points(case, seed=None):
    """(q, p, w) of a case: [B,K,nd] fp32 voxel coordinates, w [B,K] or None."""
    shape, K, kind, aniso, lam = case
    B, nd = shape[:2]
    vol = shape[2:]
    gen = torch.Generator().manual_seed(1000 + CASES.index(case) if seed is None else seed)
    ext = torch.tensor([n - 1 for n in vol], dtype=torch.float32)
    q = torch.rand(B, K, nd, generator=gen) * ext
    qn = q / ext
    if kind == 'affine':
        q, A, t = affine_draw(case)
        return q, q @ A.t() + t, None
    if kind == 'rough':
        d = 2.0 * torch.randn(B, K, nd, generator=gen)
    else:
        f = 0.5 + 1.5 * torch.rand(nd, nd, generator=gen)
        ph = 6.283 * torch.rand(nd, nd, generator=gen)
        d = 3.0 * torch.sin(6.283 * qn[..., None, :] * f + ph).prod(-1)
        if kind == 'noisy':
            d = d + 0.3 * torch.randn(B, K, nd, generator=gen)
    p = q + d
    w = None
    if kind == 'pad':
        w = 0.5 + torch.rand(B, K, generator=gen)
        step = max(K // 8, 5)
        w[:, 1::step] = 0.0
        q[:, 2::step, 0] = float('nan')
        p[:, 3::step, nd - 1] = float('nan')
        p[:, 4::step, 0] = float('inf')
    return q, p, w


def affine_draw(case):
    """(q, A, t) of an 'affine' case with p = q A^T + t EXACT in fp32: distinct q on the lattice of eighths of a voxel, A - I in
    sixteenths, t in eighths, so every product and partial sum is representable.  (With p merely rounded to fp32 the set is
    affine only to 2^-24 |p|, and the weights interpolate that noise: 1e-5 instead of 0.)"""
    shape, K = case[0], case[1]
    B, nd = shape[:2]
    vol = shape[2:]
    gen = torch.Generator().manual_seed(1000 + CASES.index(case))
    lat = tuple(8 * (n - 1) + 1 for n in vol)
    q = torch.stack([torch.stack(torch.unravel_index(torch.randperm(math.prod(lat), generator=gen)[:K], lat), -1)
                     for _ in range(B)]).float() / 8
    A = torch.eye(nd) + torch.round(1.6 * torch.randn(nd, nd, generator=gen)) / 16
    t = torch.round(8 * torch.randn(nd, generator=gen)) / 8
    return q, A, t


def affine_of(case):
    return affine_draw(case)[1:]


class Ref:
    pass


@functools.lru_cache(maxsize=None)
def reference(case):
    """Everything the tests of one case share, computed once on the CPU and never written to: the points, the float64
    restatement (coefficients, flow, the spline at the control points and at random points, dcoef of a fixed g by autograd)
    and the fp32 yardsticks e32 of each."""
    shape, K, kind, aniso, lam = case
    B, nd = shape[:2]
    vol = tuple(shape[2:])
    h = ANISO[nd] if aniso else (1.0,) * nd
    r = Ref()
    r.vol, r.h, r.nd, r.B, r.K, r.lam = vol, h, nd, B, K, lam
    r.q, r.p, r.w = make_points(case)
    gen = torch.Generator().manual_seed(77 + CASES.index(case))
    with torch.no_grad():
        r.coef, _ = ref_fit(r.q, r.p, vol, h, lam, r.w)
    valid = valid_of(r.q, r.p, r.w)
    r.qs = torch.where(valid[..., None], r.q, torch.zeros_like(r.q))
    r.valid = valid
    ext = torch.tensor([n - 1 for n in vol], dtype=torch.float32)
    r.rand = (torch.rand(B, 37, nd, generator=gen) * 1.2 - 0.1) * ext          # some outside the volume
    r.g = torch.randn(B, nd, *vol, generator=gen)
    grid = grid_of(vol)
    gflat = r.g.reshape(B, nd, -1).transpose(1, 2)
    res = {}
    for dtype in (F64, torch.float32):
        c = r.coef.to(dtype).requires_grad_()
        u = eval_at(c, r.qs, grid, vol, h, dtype)
        dc, = torch.autograd.grad((u * gflat.to(dtype)).sum(), c)
        with torch.no_grad():
            res[dtype] = (as_flow(u.detach(), vol), eval_at(c, r.qs, r.qs, vol, h, dtype), eval_at(c, r.qs, r.rand, vol, h, dtype), dc)
    r.flow, r.at_ctrl, r.at_rand, r.dcoef = res[F64]
    f32 = res[torch.float32]
    r.umax = float(r.flow.abs().max())
    r.e32 = {
        'flow': float((f32[0].double() - r.flow).abs().max()),
        'ctrl': float((f32[1].double() - r.at_ctrl).abs().max()),
        'rand': float((f32[2].double() - r.at_rand).abs().max()),
        'dcoef': float((f32[3].double() - r.dcoef).norm() / r.dcoef.norm()),
    }
    r.bound = {
        'flow': FACTOR * r.e32['flow'] + FLOOR * r.umax,
        'ctrl': FACTOR * r.e32['ctrl'] + FLOOR * float(r.at_ctrl.abs().max()),
        'rand': FACTOR * r.e32['rand'] + FLOOR * float(r.at_rand.abs().max()),
        'dcoef': FACTOR * r.e32['dcoef'] + FLOOR,
    }
    return r


def gpu_fit(r):
    w = None if r.w is None else r.w.to(DEV)
    return ops.tps_fit(r.q.to(DEV), r.p.to(DEV), r.vol, r.h if r.h != (1.0,) * r.nd else None, r.lam, w)


# ------------------------------------------------------------------------------------------ CPU tier
def test_abi_refuses_bad_arguments_without_a_launch():
    h = dfmir_amd.lib()
    assert h.dfmir_tps_ws_bytes(3, 1, 257, 13, 17, 19) > 0
    assert h.dfmir_tps_ws_bytes(3, 2, 64, 3, 4, 5) % 8 == 0
    for bad in ((4, 1, 8, 4, 4, 4), (3, 0, 8, 4, 4, 4), (3, 1, 0, 4, 4, 4), (3, 1, MAX_K + 1, 4, 4, 4), (3, 1, 8, 1, 4, 4),
                (2, 1, 8, 1, 1, 4), (3, 1, 8, 1024, 1024, 1024), (3, 65536, 8, 2, 2, 2)):
        assert h.dfmir_tps_ws_bytes(*bad) == -1, bad
    assert h.dfmir_tps_fwd(3, None, None, None, None, 1, 8, 0, 4, 4, 4, 1.0, 1.0, 1.0, None) != 0
    assert b"invalid argument" in h.dfmir_last_error()
    assert h.dfmir_tps_bwd_coef(3, None, None, None, None, 1, 8, 4, 4, 4, 1.0, 1.0, 1.0, None) != 0
    assert b"invalid argument" in h.dfmir_last_error()


@pytest.mark.parametrize("nd", [3, 2])
def test_restatement_and_fit_match_scipy(nd):
    """The restatement reproduces scipy's RBFInterpolator (kernel 'linear' in 3-D, 'thin_plate_spline' in 2-D, degree 1) in
    the normalised coordinates, with and without smoothing; ops.tps_fit (here on CPU tensors: it is plain torch) returns the
    restatement's coefficients.  Bounds: both sides solve one float64 system whose condition number stays below 1e8 (the
    probe of the definition), so they agree to 1e8 * 2^-53 ~ 1e-8 of the displacements' size."""
    interp = pytest.importorskip("scipy.interpolate")
    for case in [c for c in CASES if c[0][1] == nd and c[2] in ('smooth', 'noisy', 'rough') and 64 <= c[1] <= 2 * TPS_T + 1]:
        shape, K, kind, aniso, lam = case
        vol = tuple(shape[2:])
        h = ANISO[nd] if aniso else (1.0,) * nd
        q, p, _ = make_points(case)
        coef, qh = ref_fit(q, p, vol, h, lam)
        x = torch.rand(200, nd, dtype=F64, generator=torch.Generator().manual_seed(5))
        mine = ref_eval(coef, qh, x)
        fit = ops.tps_fit(q, p, vol, h, lam)
        assert fit.coef.dtype == F64 and tuple(fit.coef.shape) == (shape[0], K + nd + 1, nd)
        assert fit.scale == pytest.approx(scale_of(vol, h), rel=1e-15)
        theirs = ref_eval(fit.coef, qh, x)
        dmax = float((p - q).abs().max())
        for b in range(shape[0]):
            sp = interp.RBFInterpolator(qh[b].numpy(), (p[b].double() - q[b].double()).numpy(),
                                        kernel='linear' if nd == 3 else 'thin_plate_spline', degree=1, smoothing=lam)
            want = torch.from_numpy(sp(x.numpy()))
            assert float((mine[b] - want).abs().max()) <= 1e-8 * dmax, (_id(case), b)
            assert float((theirs[b] - want).abs().max()) <= 1e-8 * dmax, (_id(case), b)


@pytest.mark.parametrize("nd", [3, 2])
def test_interpolation_property_and_padding_on_the_cpu(nd):
    """smoothing = 0: u(q_k) = d_k at every valid point, with ops.tps_fit's coefficients evaluated by the restatement; a
    padding entry has a zero coefficient and a zero control position, and the fit equals the fit of the valid subset."""
    case = next(c for c in CASES if c[0][1] == nd and c[2] == 'pad' and c[4] == 0.0)
    shape, K, kind, aniso, lam = case
    vol = tuple(shape[2:])
    h = (1.0,) * nd
    q, p, w = make_points(case)
    fit = ops.tps_fit(q, p, vol, None, 0.0, w)
    valid = valid_of(q, p, w)
    assert 0 < int((~valid).sum()) < K
    assert bool((fit.coef[:, :K][~valid] == 0).all()) and bool((fit.ctrl[~valid] == 0).all())
    assert torch.equal(fit.ctrl[valid], q[valid])
    u = eval_at(fit.coef, fit.ctrl, fit.ctrl, vol, h, F64)
    d = (p.double() - q.double())[valid]
    assert float((u[valid] - d).abs().max()) <= 1e-8 * float(d.abs().max())
    coef, _ = ref_fit(q, p, vol, h, 0.0, w)
    assert float((fit.coef - coef).abs().max()) <= 1e-8 * float(coef.abs().max())
    assert float(fit.coef[:, :K].sum(1).abs().max()) <= 1e-8 * float(coef.abs().max())       # P^T w = 0, the row of ones


def test_fit_is_differentiable_in_moving_pts_on_the_cpu():
    case = next(c for c in CASES if c[2] == 'noisy' and c[0][1] == 2)
    q, p, _ = make_points(case)
    vol = tuple(case[0][2:])
    p1 = p.clone().requires_grad_()
    c = ops.tps_fit(q, p1, vol, None, case[4]).coef
    g = torch.randn(c.shape, dtype=F64, generator=torch.Generator().manual_seed(3))
    (c * g).sum().backward()
    p2 = p.clone().requires_grad_()
    c2, _ = ref_fit(q, p2, vol, (1.0, 1.0), case[4])
    (c2 * g).sum().backward()
    assert float((p1.grad - p2.grad).norm()) <= 1e-6 * float(p2.grad.norm())    # (the gradients themselves are fp32)


def test_argument_checks_raise_before_any_launch():
    q = torch.rand(2, 8, 3) * 3
    p = q + 0.5
    vol = (4, 5, 6)
    with pytest.raises(ValueError, match="K must lie"):
        ops.tps_fit(q[:, :3], p[:, :3], vol)
    with pytest.raises(ValueError, match="K must lie"):
        ops.tps_fit(torch.zeros(1, MAX_K + 1, 3), torch.zeros(1, MAX_K + 1, 3), vol)
    with pytest.raises(ValueError, match="vol must be"):
        ops.tps_fit(q, p, (4, 5, 1))
    with pytest.raises(ValueError, match="vol must be"):
        ops.tps_fit(q, p, 7)
    with pytest.raises(DfmirHipError, match="points mismatch"):
        ops.tps_fit(q, p, (4, 5))
    with pytest.raises(DfmirHipError, match="points mismatch"):
        ops.tps_fit(q, p[:, :7], vol)
    with pytest.raises(DfmirHipError, match="fp32 tensors only"):
        ops.tps_fit(q.double(), p, vol)
    with pytest.raises(DfmirHipError, match="weight mismatch"):
        ops.tps_fit(q, p, vol, weight=torch.ones(2, 7))
    with pytest.raises(DfmirHipError, match="must be \\[B,K,nd\\] tensors"):
        ops.tps_fit(q.numpy(), p, vol)
    with pytest.raises(ValueError, match="spacing"):
        ops.tps_fit(q, p, vol, spacing=(1.0, 1.0))
    with pytest.raises(ValueError, match="spacing"):
        ops.tps_fit(q, p, vol, spacing=(1.0, -1.0, 1.0))
    for bad in (-1.0, float('nan'), float('inf'), "1", True):
        with pytest.raises(ValueError, match="smoothing"):
            ops.tps_fit(q, p, vol, smoothing=bad)
    with pytest.raises(ValueError, match="weight must hold"):
        ops.tps_fit(q, p, vol, weight=-torch.ones(2, 8))
    with pytest.raises(ValueError, match="weight must hold"):
        ops.tps_fit(q, p, vol, weight=torch.full((2, 8), float('nan')))
    # singular systems: coincident points without smoothing, too few valid points, points on one plane
    qq = q.clone()
    qq[:, 1] = qq[:, 0]
    with pytest.raises(ValueError, match="singular"):
        ops.tps_fit(qq, p, vol)
    assert ops.tps_fit(qq, p, vol, smoothing=0.1).coef.isfinite().all()
    w = torch.zeros(2, 8)
    w[:, :3] = 1.0
    with pytest.raises(ValueError, match="singular"):
        ops.tps_fit(q, p, vol, weight=w)
    flat = q.clone()
    flat[..., 0] = 1.0
    with pytest.raises(ValueError, match="singular"):
        ops.tps_fit(flat, p, vol)
    # the evaluation ops: a CPU handle has no kernel to run on; bad coef / points raise first
    fit = ops.tps_fit(q, p, vol)
    with pytest.raises(DfmirHipError, match="no CPU fallback"):
        ops.tps_flow(fit)
    with pytest.raises(DfmirHipError, match="no CPU fallback"):
        ops.tps_points(fit, q)
    with pytest.raises(ValueError, match="needs handle="):
        ops.tps_flow(fit.coef)
    with pytest.raises(ValueError, match="either a handle"):
        ops.tps_flow(fit, handle=fit)
    with pytest.raises(DfmirHipError, match="coef mismatch"):
        ops.tps_flow(fit.coef[:, :-1], handle=fit)
    with pytest.raises(DfmirHipError, match="coef must be float64"):
        ops.tps_flow(fit.coef.float(), handle=fit)
    with pytest.raises(ValueError, match="handle must be"):
        ops.tps_points(fit.coef, q)
    with pytest.raises(ValueError, match="interp"):
        infer.landmark_init(torch.zeros(2, 1, *vol), torch.zeros(2, 1, *vol), q, p, interp='nearest')
    with pytest.raises(ValueError, match="one shape"):
        infer.landmark_init(torch.zeros(2, 1, *vol), torch.zeros(2, 1, 4, 5, 7), q, p)
    with pytest.raises(ValueError, match="samples of images"):
        infer.landmark_init(torch.zeros(1, 1, *vol), torch.zeros(1, 1, *vol), q, p)


@pytest.mark.gpu
def test_point_argument_checks_on_a_device_handle():
    q = torch.rand(2, 8, 3, device=DEV) * 3
    fit = ops.tps_fit(q, q + 0.5, (4, 5, 6))
    for bad in (q[:1], q[..., :2], q[:, :0], q.double(), q.cpu()):
        with pytest.raises(DfmirHipError):
            ops.tps_points(fit, bad)
    with pytest.raises(DfmirHipError, match="coef on"):
        ops.tps_flow(fit.coef.cpu(), handle=fit)


# ------------------------------------------------------------------------------------------ GPU tier
def report(case, what, err, bound, e32):
    print("tps-margin %s %s err=%.3e bound=%.3e e32=%.3e" % (_id(case), what, err, bound, e32))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_flow_and_points_match_the_restatement(case):
    r = reference(case)
    fit = gpu_fit(r)
    flow = ops.tps_flow(fit)
    assert flow.dtype == torch.float32 and tuple(flow.shape) == tuple(case[0])
    got = {'flow': flow, 'ctrl': ops.tps_points(fit, fit.ctrl), 'rand': ops.tps_points(fit, r.rand.to(DEV))}
    want = {'flow': r.flow, 'ctrl': r.at_ctrl, 'rand': r.at_rand}
    errs = {k: float((got[k].double().cpu() - want[k]).abs().max()) for k in got}
    for k in got:
        report(case, k, errs[k], r.bound[k], r.e32[k])
    assert torch.equal(fit.ctrl.cpu(), r.qs)
    assert bool((fit.coef[:, :r.K][~r.valid.to(DEV)] == 0).all())
    for k in got:
        assert errs[k] <= r.bound[k], (k, errs[k], r.bound[k])
    if r.lam == 0.0:                         # interpolation: u(q_k) = d_k at the valid points
        d = (r.p.double() - r.q.double())[r.valid]
        assert float((got['ctrl'].double().cpu()[r.valid] - d).abs().max()) <= r.bound['ctrl']


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_dcoef_matches_autograd_and_the_dot_product_identity(case):
    r = reference(case)
    fit = gpu_fit(r)
    coef = r.coef.to(DEV).requires_grad_()
    flow = ops.tps_flow(coef, handle=fit)
    g = r.g.to(DEV)
    dcoef, = torch.autograd.grad(flow, coef, g)
    assert dcoef.dtype == F64 and dcoef.shape == coef.shape
    err = float((dcoef.cpu() - r.dcoef).norm() / r.dcoef.norm())
    report(case, 'dcoef', err, r.bound['dcoef'], r.e32['dcoef'])
    assert err <= r.bound['dcoef']
    # <tps_flow(c), g> = <c, bwd(g)> for an arbitrary c: both sides see the same fp32 basis values and add in float64, so
    # they differ by the one fp32 rounding of each flow element, at most 2^-24 |u| |g| each
    c = torch.randn(coef.shape, dtype=F64, generator=torch.Generator().manual_seed(9)).to(DEV)
    u = ops.tps_flow(c, handle=fit).double()
    lhs = float((u * g.double()).sum())
    rhs = float((c * dcoef).sum())
    assert abs(lhs - rhs) <= 2.0 ** -23 * float((u.abs() * g.double().abs()).sum()), (lhs, rhs)


@pytest.mark.gpu
@pytest.mark.parametrize("nd", [3, 2])
def test_padding_matches_the_fit_of_the_valid_subset(nd):
    """The same flow from the padded set and from its valid points alone (K differs, so chunks and order differ)."""
    case = next(c for c in CASES if c[0][1] == nd and c[2] == 'pad' and c[0][0] == 1)
    r = reference(case)
    keep = r.valid[0]
    sub = ops.tps_fit(r.q[:, keep].to(DEV), r.p[:, keep].to(DEV), r.vol, None, r.lam, r.w[:, keep].to(DEV))
    a, b = ops.tps_flow(gpu_fit(r)), ops.tps_flow(sub)
    assert float((b.double().cpu() - r.flow).abs().max()) <= r.bound['flow']
    assert float((a.double() - b.double()).abs().max()) <= r.bound['flow']


@pytest.mark.gpu
@pytest.mark.parametrize("nd", [3, 2])
def test_affine_set_has_no_weights_and_gives_the_affine_flow(nd):
    case = next(c for c in CASES if c[0][1] == nd and c[2] == 'affine')
    r = reference(case)
    fit = gpu_fit(r)
    dmax = float((r.p - r.q).abs().max())
    assert float(fit.coef[:, :r.K].abs().max()) <= 1e-9 * dmax
    A, t = affine_of(case)
    c = torch.tensor([(n - 1) / 2 for n in r.vol])
    theta = torch.cat([A, (A @ c + t - c)[:, None]], 1)[None].to(DEV)        # p = A q + t in ops.affine_flow's centred form
    want = ops.affine_flow(theta.contiguous(), r.vol)
    assert float((ops.tps_flow(fit) - want).abs().max()) <= r.bound['flow']


@pytest.mark.gpu
@pytest.mark.parametrize("nd", [3, 2])
def test_gradient_reaches_moving_pts_through_the_fit(nd):
    """d <tps_flow(tps_fit(q, p)), g> / dp against the restatement's autograd gradient, relative 2-norm; the yardstick e32 is
    the same chain with the evaluation in fp32 (the solve stays float64 on both sides, as in ops.tps_fit)."""
    case = next(c for c in CASES if c[0][1] == nd and c[2] == 'noisy' and c[1] < MAX_K)
    r = reference(case)
    grid = grid_of(r.vol)
    gflat = r.g.reshape(r.B, nd, -1).transpose(1, 2)
    grads = {}
    for dtype in (F64, torch.float32):
        p = r.p.clone().requires_grad_()
        coef, _ = ref_fit(r.q, p, r.vol, r.h, r.lam)
        (eval_at(coef, r.qs, grid, r.vol, r.h, dtype) * gflat.to(dtype)).sum().backward()
        grads[dtype] = p.grad.double()
    e32 = float((grads[torch.float32] - grads[F64]).norm() / grads[F64].norm())
    p = r.p.to(DEV).requires_grad_()
    fit = ops.tps_fit(r.q.to(DEV), p, r.vol, None, r.lam)
    (ops.tps_flow(fit) * r.g.to(DEV)).sum().backward()
    err = float((p.grad.double().cpu() - grads[F64]).norm() / grads[F64].norm())
    report(case, 'dp', err, FACTOR * e32 + FLOOR, e32)
    assert err <= FACTOR * e32 + FLOOR


@pytest.mark.gpu
def test_bit_identical_from_run_to_run_and_non_contiguous_inputs():
    for nd in (3, 2):
        case = next(c for c in CASES if c[0][1] == nd and c[1] == 2 * TPS_T + 1)
        r = reference(case)
        q, p = r.q.to(DEV), r.p.to(DEV)
        fit = ops.tps_fit(q, p, r.vol, r.h, r.lam)
        g = r.g.to(DEV)
        runs = []
        for _ in range(2):
            c = fit.coef.detach().clone().requires_grad_()
            flow = ops.tps_flow(c, handle=fit)
            dc, = torch.autograd.grad(flow, c, g)
            runs.append((flow, dc, ops.tps_points(fit, r.rand.to(DEV))))
        for a, b in zip(*runs):
            assert torch.equal(a, b)
        # non-contiguous points, coef, g and query points: the same bits
        qn = q.transpose(1, 2).contiguous().transpose(1, 2)
        pn = torch.stack([p, p], -1)[..., 0]
        assert not qn.is_contiguous() and not pn.is_contiguous()
        fit2 = ops.tps_fit(qn, pn, r.vol, r.h, r.lam)
        assert torch.equal(fit2.coef, fit.coef) and fit2.ctrl.is_contiguous()
        cn = torch.stack([fit.coef.detach(), fit.coef.detach()], -1)[..., 0].requires_grad_()
        gn = g.transpose(2, 3).contiguous().transpose(2, 3)
        assert not cn.is_contiguous() and not gn.is_contiguous()
        flow = ops.tps_flow(cn, handle=fit)
        dc, = torch.autograd.grad(flow, cn, gn)
        rn = torch.stack([r.rand.to(DEV)] * 2, -1)[..., 1]
        assert torch.equal(flow, runs[0][0]) and torch.equal(dc, runs[0][1])
        assert torch.equal(ops.tps_points(fit, rn), runs[0][2])


@pytest.mark.gpu
@pytest.mark.parametrize("nd", [3, 2])
def test_landmark_init(nd):
    """infer.landmark_init at smoothing 0 with the fixed points on voxels (there the landmark kernel's linear sample of the
    flow is the flow's own value): tre = |h (q + u(q) - p)| is the flow's error at q, bounded by the flow bound, plus the fp32
    roundings of q + u and of the difference, at most 2^-23 of the largest coordinate, per axis; sqrt(nd) max h over the axes.
    Its flow goes through refine_flow(iters = 0) bit for bit, and its coef evaluates to its flow."""
    case = next(c for c in CASES if c[0] == BIG[nd] and c[2] == 'smooth' and c[1] == 2 * TPS_T + 1)
    vol, K = tuple(BIG[nd][2:]), 200
    gen = torch.Generator().manual_seed(11)
    flat = torch.randperm(math.prod(vol), generator=gen)[:K]
    q = torch.stack(torch.unravel_index(flat, vol), -1).float()[None]
    qn = q / torch.tensor([n - 1 for n in vol])
    p = q + 3.0 * torch.sin(5.0 * qn + torch.arange(nd)).flip(-1)
    mov = torch.rand(1, 1, *vol, generator=gen).to(DEV)
    fix = torch.rand(1, 1, *vol, generator=gen).to(DEV)
    h = ANISO[nd]
    out = infer.landmark_init(mov, fix, q.to(DEV), p.to(DEV), spacing=h)
    assert sorted(out) == ['coef', 'flow', 'tre', 'warped']
    assert tuple(out['flow'].shape) == (1, nd) + vol and tuple(out['tre'].shape) == (1, K) and out['coef'].dtype == F64
    coef, _ = ref_fit(q, p, vol, h)
    grid = grid_of(vol)
    want = as_flow(eval_at(coef, q, grid, vol, h, F64), vol)
    e32 = float((as_flow(eval_at(coef, q, grid, vol, h, torch.float32), vol).double() - want).abs().max())
    bound = FACTOR * e32 + FLOOR * float(want.abs().max())
    assert float((out['flow'].double().cpu() - want).abs().max()) <= bound
    tre_bound = math.sqrt(nd) * max(h) * (bound + 2.0 ** -23 * float(max(q.abs().max(), p.abs().max())))
    report(case, 'tre', float(out['tre'].max()), tre_bound, e32)
    assert float(out['tre'].max()) <= tre_bound
    assert torch.equal(out['warped'], ops.warp(mov, out['flow']))
    same = infer.refine_flow(mov, fix, out['flow'], features='intensity', lam=0.1, lr=0.1, iters=0)
    assert torch.equal(same['flow'], out['flow'])
    cub = infer.landmark_init(mov, fix, q.to(DEV), p.to(DEV), spacing=h, interp='cubic')
    assert torch.equal(cub['flow'], out['flow']) and torch.equal(cub['warped'], ops.warp_cubic(mov, out['flow']))
