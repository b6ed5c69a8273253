"""Affine pre-alignment (build-defined, dfmir_amd/csrc/affine.hip): ops.affine_flow, ops.affine_ssd, ops.affine_ssd_system,
ops.affine_lm_step and infer.affine_init.  CPU: the C ABI and the argument checks; a float64 restatement of the definitions --
the flow and its adjoint by einsum, the value from F.grid_sample(align_corners=True, padding_mode='zeros') on y(x) followed by
the (masked) mean, g and H from the documented closed form with explicit floor / gather corner differences, the
Levenberg-Marquardt loop as infer.affine_init states it -- checked against itself (g against autograd through grid_sample, H
against sum J J^T of per-voxel Jacobians, the closed-form value against grid_sample's) and on recovery fixtures.  GPU: the
kernels against the restatement, against the shipped ops.warp_ssd at ops.affine_flow(theta), and run to run.

Which launch each GPU shape reaches (dfmir_affine_system: af_sys_k<ND, FULL>, FULL = the whole system for affine_ssd_system,
gradient-only for affine_ssd; a workgroup of 256 threads walks chunks of 256 voxels, a sample has min(1024, ceil(S / 1024))
workgroups; channels pass in groups of four.  dfmir_affine_flow: af_flow_k<ND, V>, V = 4 -- 16-byte stores -- when W % 4 == 0):
  <2-D, V 1>  (2,4,9,13)             <2-D, V 4>  (2,4,8,16)
  <3-D, V 4>  (2,12,5,12,24) 1440 voxels = 2 workgroups per sample, three channel groups; (1,5,2,6,8) C = 5: a second group
              with one live channel
  <3-D, V 1>  (2,1,3,7,9) C = 1
  <2-D, V 4>  (1,1,1028,1024) 1052672 voxels > 1024 workgroups x 1024 voxels: the walk over the chunks wraps, and the last
              workgroups take one chunk less than the first
af_fin_k runs after every system, af_flow_bwd_k / af_flow_fin_k in every backward of affine_flow, af_lm_k in the step test and
in affine_init.

Thetas, a different one per sample (`kinds`): `identity` (sample 0; sample 1 takes a lattice theta), `lattice` = a generic
near-identity matrix, |(A - I) q| <= 0.4 over the volume, with a translation of integer + 0.5 per axis, so that every sample
point lies at least 0.05 from a cell face (asserted) -- the gradient has no kink nearby and fp32 cannot pick another cell;
`shifted` = the same with a translation of a third of the x extent, which pushes a third of the points past a face; `outside`
= a translation of twice the extent on every axis: no corner is inside (the guard path: L_b = mean F^2, g = 0, H = 0).  M and F
are noise in [-1, 1].  Masks: none, `partial` (float weights, zero on a third of the voxels) and `zero`.

Tolerances (profiles/affine_margins.txt, profiles/affine_margins_cpu.txt): every kernel-against-float64 comparison is bounded by 4x the error of the SAME
definition evaluated by torch in fp32 on the CPU against float64, on these inputs, the maximum over the case set per quantity
(over the five small shapes and over the large one separately: fp32 coordinates of a thousand voxels carry another error than
those of ten): values relative, gradients and H in relative 2-norm and as max-abs over max, the flow absolute.  scripts/affine_margins.py
measures them, with the kernels' own errors beside them.  affine_ssd against warp_ssd compares two fp32 kernels: 2x that bound.
The theta affine_init recovers is bounded by 4x the gap between the fp32 CPU restatement of the whole loop and float64."""
import ctypes
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

from tests.golden import common as C

DEV = "cuda"
FACTOR = 4.0
# rows "max" of the fp32 CPU columns, over the five small shapes and over the large one.  The fp32 figures depend on the host
# (torch orders its sums by the thread count), so two runs are recorded: profiles/affine_margins.txt (a host with the device:
# the kernels' errors stand beside) and profiles/affine_margins_cpu.txt (a host without one).  Per quantity the SMALLER of the
# two stands here.
GROUPS = ("small", "large")
FP32_ERR = {"small": {"flow": 5.45e-06, "dtheta_l2": 1.40e-07, "dtheta_max": 2.25e-07, "L": 1.56e-07, "Lb": 1.89e-07,
                      "gb_l2": 7.31e-07, "gb_max": 8.86e-07, "g_l2": 7.31e-07, "g_max": 7.85e-07, "H_l2": 4.00e-07, "H_max": 3.72e-07},
            "large": {"flow": 1.83e-04, "dtheta_l2": 3.09e-06, "dtheta_max": 3.79e-06, "L": 3.82e-06, "Lb": 3.82e-06,
                      "gb_l2": 1.05e-04, "gb_max": 1.52e-04, "g_l2": 1.05e-04, "g_max": 1.52e-04, "H_l2": 1.60e-05, "H_max": 2.04e-05}}
BOUND = {grp: {k: FACTOR * v for k, v in e.items()} for grp, e in FP32_ERR.items()}
# max |theta(fp32 CPU loop) - theta(float64 loop)| over the two recovery fixtures: 6.146e-08 in profiles/affine_margins.txt,
# 1.211e-07 in profiles/affine_margins_cpu.txt
THETA_FP32_GAP = 6.146e-08
SHAPES = [(2, 4, 9, 13), (2, 4, 8, 16), (2, 12, 5, 12, 24), (2, 1, 3, 7, 9), (1, 5, 2, 6, 8), (1, 1, 1028, 1024)]
KINDS = ("identity", "lattice", "shifted", "outside")
MASKS = ("none", "partial", "zero")
FORMS = ("packed", "plain")


def group_of(shape):
    return "large" if math.prod(shape[2:]) > 100000 else "small"


def _id(shape):
    return "x".join(str(v) for v in shape)


# ------------------------------------------------------------------------------------------ restatement
def _grid(vol, dtype):
    return torch.stack(torch.meshgrid(*[torch.arange(n, dtype=dtype) for n in vol], indexing='ij'), 0)


def _centre(vol, dtype):
    return torch.tensor([(n - 1) / 2.0 for n in vol], dtype=dtype).reshape((len(vol),) + (1,) * len(vol))


def qe_of(vol, dtype):
    """q(x) = (x - c, 1) as [nd + 1, *vol]."""
    return torch.cat([_grid(vol, dtype) - _centre(vol, dtype), torch.ones((1,) + tuple(vol), dtype=dtype)], 0)


def affine_flow_ref(theta, vol):
    """flow[b,a,x] = y_a(x) - x_a, y = c + A (x - c) + t, in theta's dtype."""
    y = torch.einsum('baj,j...->ba...', theta, qe_of(vol, theta.dtype)) + _centre(vol, theta.dtype)[None]
    return y - _grid(vol, theta.dtype)[None]


def affine_flow_adjoint_ref(dflow):
    """dtheta[b,a,j] = sum_x dflow[b,a,x] q_j(x)."""
    return torch.einsum('ba...,j...->baj', dflow, qe_of(tuple(dflow.shape[2:]), dflow.dtype))


def _reduce(e2c, mask):
    """(L, L_b [B]) of e2c = mean_c e^2 [B,1,*vol]: the plain mean, or sum m e2c / sum m with 0 for an empty mask."""
    B = e2c.shape[0]
    if mask is None:
        per = e2c.reshape(B, -1).mean(1)
        return per.mean(), per
    m = mask.to(e2c.dtype).expand_as(e2c)
    num, den = (m * e2c).reshape(B, -1).sum(1), m.reshape(B, -1).sum(1)
    safe = lambda n, d: n / d if float(d) > 0 else n * 0.0
    return safe(num.sum(), den.sum()), torch.stack([safe(num[b], den[b]) for b in range(B)])


def ssd_grid_sample(M, Fx, phi, mask=None):
    """(L, L_b) of a flow from F.grid_sample: normalised coordinates, align_corners=True, zero padding, then the (masked)
    mean -- the restatement of ops.warp_ssd.  Differentiable in phi."""
    nd = phi.shape[1]
    vol = tuple(phi.shape[2:])
    f = _grid(vol, phi.dtype)[None] + phi
    norm = [2.0 * f[:, a] / (vol[a] - 1) - 1.0 for a in range(nd)]
    grid = torch.stack(norm[::-1], -1)
    warped = F.grid_sample(M, grid, mode='bilinear', padding_mode='zeros', align_corners=True)
    return _reduce(((warped - Fx) ** 2).mean(1, keepdim=True), mask)


def sample_closed(M, f):
    """(M(f) [B,C,*vol], dM [B,C,nd,*vol]) at the sample points f [B,nd,*vol] with explicit floor / gather indexing: the
    interpolant in the cell floor() selects and its derivative -- corner differences (+ upper, - lower along d, times the other
    axes' weights), zero-padded corners taking part as zeros."""
    B, nd = f.shape[:2]
    Cn = M.shape[1]
    vol = tuple(f.shape[2:])
    S = math.prod(vol)
    i0 = torch.floor(f)
    w1 = f - i0
    w = (1.0 - w1, w1)
    i0 = i0.clamp(-4, max(vol) + 4).long()                      # (far-away points: every corner outside either way)
    strides = [math.prod(vol[a + 1:]) for a in range(nd)]
    Mf = M.reshape(B, Cn, S)
    val = torch.zeros_like(M)
    dM = [torch.zeros_like(M) for _ in range(nd)]
    for bits in itertools.product((0, 1), repeat=nd):
        flat = torch.zeros((B,) + vol, dtype=torch.long)
        valid = torch.ones((B,) + vol, dtype=torch.bool)
        for a in range(nd):
            ia = i0[:, a] + bits[a]
            valid &= (ia >= 0) & (ia < vol[a])
            flat += ia.clamp(0, vol[a] - 1) * strides[a]
        v = torch.gather(Mf, 2, flat.reshape(B, 1, S).expand(B, Cn, S)).reshape(M.shape) * valid.to(M.dtype)[:, None]
        wa = [w[bits[a]][:, a] for a in range(nd)]
        val = val + math.prod(wa[1:], start=wa[0])[:, None] * v
        for d in range(nd):
            others = torch.ones_like(wa[0])
            for a in range(nd):
                if a != d:
                    others = others * wa[a]
            dM[d] = dM[d] + (1.0 if bits[d] else -1.0) * others[:, None] * v
    return val, torch.stack(dM, 2)


def system_ref(M, Fx, theta, mask=None, dtype=torch.float64):
    """dict(L, Lb [B], gb [B,nd,nd+1] = dL/dtheta, g [B,P], H [B,P,P], val) on the CPU in `dtype` (float64: the restatement;
    float32: the yardstick): the values from grid_sample on y(x) and the (masked) mean; g and H from the closed form,
        g_b = (2 / (C N_b)) sum_x m r (x) q,   H_b = (2 / (C N_b)) sum_x m G (x) (q q^T),   r = sum_c e_c dM_c,  G = sum_c dM_c dM_c^T
    and gb_b = g_b N_b / sum_b N_b; all 0 where the weights sum to 0.  val: the closed form's own L_b."""
    M, Fx, theta = (t.detach().cpu().to(dtype) for t in (M, Fx, theta))
    m = None if mask is None else mask.detach().cpu().to(dtype)
    B, Cn = M.shape[:2]
    vol = tuple(M.shape[2:])
    nd, S = len(vol), math.prod(vol)
    P = nd * (nd + 1)
    flow = affine_flow_ref(theta, vol)
    L, Lb = ssd_grid_sample(M, Fx, flow, m)
    val, dM = sample_closed(M, _grid(vol, dtype)[None] + flow)
    e = val - Fx
    mw = (torch.ones((B, 1) + vol, dtype=dtype) if m is None else m.expand((B, 1) + vol)).reshape(B, 1, S)
    N = mw.sum((1, 2))
    r = (e[:, :, None] * dM).sum(1).reshape(B, nd, S)
    G = torch.einsum('bca...,bcd...->bad...', dM, dM).reshape(B, nd * nd, S)
    qe = qe_of(vol, dtype).reshape(nd + 1, S)
    qq = (qe[:, None] * qe[None]).reshape((nd + 1) ** 2, S)
    sc = torch.where(N > 0, 2.0 / (Cn * N.clamp_min(1e-300)), torch.zeros_like(N))
    g = sc[:, None, None] * ((mw * r) @ qe.T)                                                  # [B,nd,nd+1]
    H = sc[:, None, None] * ((mw * G) @ qq.T)                                                  # [B,(a,d),(i,j)]
    H = H.reshape(B, nd, nd, nd + 1, nd + 1).permute(0, 1, 3, 2, 4).reshape(B, P, P)
    Nall = N.sum()
    gb = g * (N / Nall)[:, None, None] if float(Nall) > 0 else g * 0.0
    valb = torch.where(N > 0, (mw * (e ** 2).mean(1).reshape(B, 1, S)).sum((1, 2)) / N.clamp_min(1e-300), torch.zeros_like(N))
    return dict(L=L, Lb=Lb, gb=gb, g=g.reshape(B, P), H=H, val=valb)


def _free(nd, dof):
    P = nd * (nd + 1)
    return list(range(P)) if dof == 'affine' else [a * (nd + 1) + nd for a in range(nd)]


def lm_solve_ref(g, H, mu, free):
    """(d [P] with zeros off `free`, singular): (H[f,f] + mu diag H[f,f]) d = -g[f] by Cholesky in float64; a pivot <= 0 or not
    finite gives d = 0 and singular."""
    n = len(free)
    A = [[float(H[free[i], free[j]]) for j in range(n)] for i in range(n)]
    for i in range(n):
        A[i][i] += mu * A[i][i]
    Lc = [[0.0] * n for _ in range(n)]
    d = [0.0] * len(g)
    for i in range(n):
        for j in range(i + 1):
            s = A[i][j] - sum(Lc[i][c] * Lc[j][c] for c in range(j))
            if i == j:
                if not (s > 0.0) or not math.isfinite(s):
                    return d, True
                Lc[i][i] = math.sqrt(s)
            else:
                Lc[i][j] = s / Lc[j][j]
    z = [0.0] * n
    for i in range(n):
        z[i] = (-float(g[free[i]]) - sum(Lc[i][c] * z[c] for c in range(i))) / Lc[i][i]
    for i in reversed(range(n)):
        z[i] = (z[i] - sum(Lc[c][i] * z[c] for c in range(i + 1, n))) / Lc[i][i]
    for i in range(n):
        d[free[i]] = z[i]
    return d, False


def lm_step_ref(L, g, H, st, k, nd, dof, mu_up, mu_down, theta_dtype):
    """One step of the loop for ONE sample, in place on st = dict(acc [P], trial [P], L_acc, mu, g, H); returns the history row.
    theta_dtype: what the thetas are rounded to (float64: the restatement; float32: what the kernel stores)."""
    L = float(L)
    ok = math.isfinite(L) and L <= st['L_acc']
    if ok:
        st['acc'], st['L_acc'], st['g'], st['H'] = st['trial'].clone(), L, g.clone(), H.clone()
        if k > 0:
            st['mu'] = max(st['mu'] * mu_down, 1e-12)
    else:
        st['mu'] = min(st['mu'] * mu_up, 1e12)
    d, singular = lm_solve_ref(st['g'], st['H'], st['mu'], _free(nd, dof))
    trial = st['acc'].double().clone()
    for i in _free(nd, dof):
        trial[i] = trial[i] + d[i]
    st['trial'] = trial.to(theta_dtype)
    return [L, st['L_acc'], st['mu'], 1.0 if ok else 0.0, 1.0 if singular else 0.0]


def _pool(t, s):
    if s == 1:
        return t
    return (F.avg_pool3d if t.dim() == 5 else F.avg_pool2d)(t, s, s)


def affine_init_ref(Mm, Mf, mask=None, theta=None, dof='affine', levels=(4, 2, 1), iters=10, mu0=1e-3, mu_up=10.0, mu_down=0.1,
                    dtype=torch.float64, theta_dtype=torch.float64):
    """(theta [B,nd,nd+1], history [sum iters, B, 5]) of infer.affine_init's loop on feature tensors, on the CPU: the system in
    `dtype`, the solve in float64, the thetas kept in `theta_dtype`."""
    B, nd = Mm.shape[0], Mm.dim() - 2
    P = nd * (nd + 1)
    iters = (iters,) * len(levels) if isinstance(iters, int) else tuple(iters)
    th = (torch.eye(nd, nd + 1, dtype=theta_dtype).repeat(B, 1, 1) if theta is None else theta.to(theta_dtype).clone())
    hist = []
    for s, n in zip(levels, iters):
        if n == 0:
            continue
        Lm, Lf, Lk = _pool(Mm.to(dtype), s), _pool(Mf.to(dtype), s), None if mask is None else _pool(mask.to(dtype), s)
        th = th.clone()
        th[:, :, nd] = th[:, :, nd] / s
        sts = [dict(acc=th[b].reshape(P).clone(), trial=th[b].reshape(P).clone(), L_acc=float('inf'), mu=float(mu0),
                    g=torch.zeros(P, dtype=torch.float64), H=torch.zeros(P, P, dtype=torch.float64)) for b in range(B)]
        for k in range(n):
            trial = torch.stack([st['trial'] for st in sts]).reshape(B, nd, nd + 1)
            sy = system_ref(Lm, Lf, trial, Lk, dtype=dtype)
            hist.append([lm_step_ref(sy['Lb'][b].double(), sy['g'][b].double(), sy['H'][b].double(), sts[b], k, nd, dof, mu_up,
                                     mu_down, theta_dtype) for b in range(B)])
        th = torch.stack([st['acc'] for st in sts]).reshape(B, nd, nd + 1).clone()
        th[:, :, nd] = th[:, :, nd] * s
    return th, torch.tensor(hist, dtype=torch.float64).reshape(-1, B, 5)


# ------------------------------------------------------------------------------------------ inputs
def thetas(shape, kind, seed):
    """[B,nd,nd+1] fp32 of a case (see the module docstring); every sample its own."""
    B, vol = shape[0], tuple(shape[2:])
    nd = len(vol)
    qmax = torch.tensor([(n - 1) / 2.0 for n in vol], dtype=torch.float64)
    out = []
    for b in range(B):
        u = C.rand(seed + 31 * b, nd, nd).double()
        sign = torch.where(C.rand(seed + 31 * b + 1, nd, nd) < 0.5, -1.0, 1.0).double()
        E = sign * (0.5 + 0.5 * u) * 0.4 / (nd * qmax[None, :])           # sum_j |E_aj| qmax_j <= 0.4
        k = torch.floor(C.rand(seed + 31 * b + 2, nd).double() * 5.0) - 2.0
        t = k + 0.5
        if kind == "identity" and b == 0:
            E, t = E * 0.0, t * 0.0
        if kind == "shifted":
            t[nd - 1] = float(vol[nd - 1] // 3 + (vol[nd - 1] // 2 if b else 0)) + 0.5
        if kind == "outside":
            t = torch.tensor([(2.0 + b) * n + 0.5 for n in vol], dtype=torch.float64)
        out.append(torch.cat([torch.eye(nd, dtype=torch.float64) + E, t[:, None]], 1))
    return torch.stack(out).float()


def inputs(shape, kind, mask="none", seed=1300):
    """(M, F, theta, mask or None) fp32 of a case."""
    seed = seed + 19 * SHAPES.index(shape) if shape in SHAPES else seed
    B, vol = shape[0], tuple(shape[2:])
    M = C.rand(seed, *shape) * 2 - 1
    Fx = C.rand(seed + 1, *shape) * 2 - 1
    m = None
    if mask == "partial":
        m = C.rand(seed + 4, B, 1, *vol)
        m = torch.where(m < 1.0 / 3.0, torch.zeros_like(m), m)
    elif mask == "zero":
        m = torch.zeros(B, 1, *vol)
    return M, Fx, thetas(shape, kind, seed + 7), m


def face_distance(theta, vol):
    """min over the sample points of the distance to the nearest cell face (0 for a point on the lattice), in float64."""
    f = _grid(vol, torch.float64)[None] + affine_flow_ref(theta.double(), vol)
    fr = f - torch.floor(f)
    return float(torch.minimum(fr, 1.0 - fr).min())


def _rel(got, ref):
    got, ref = got.detach().cpu().double().reshape(-1), ref.detach().cpu().double().reshape(-1)
    live = ref != 0
    if not bool(live.all()):
        assert bool((got[~live] == 0).all()), "a value whose restatement is exactly 0 must be exactly 0"
    return float(((got - ref)[live].abs() / ref[live].abs()).max()) if bool(live.any()) else 0.0


def _l2_max(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    if float(ref.abs().max()) == 0.0:
        assert float(got.abs().max()) == 0.0, "a tensor whose restatement is exactly 0 must be exactly 0"
        return 0.0, 0.0
    return float((got - ref).norm() / ref.norm()), float((got - ref).abs().max() / ref.abs().max())


def system_errors(got, ref):
    """dict of the errors of (L, Lb, gb, g, H) against the restatement's."""
    out = dict(L=_rel(got['L'].reshape(1), ref['L'].reshape(1)), Lb=_rel(got['Lb'], ref['Lb']))
    for k in ("gb", "g", "H"):
        out[k + "_l2"], out[k + "_max"] = _l2_max(got[k], ref[k])
    return out


def dflow_of(shape, seed=1700):
    B, vol = shape[0], tuple(shape[2:])
    return C.rand(seed + SHAPES.index(shape), B, len(vol), *vol) * 2 - 1


def flow_errors(flow, dtheta, theta, shape):
    """dict(flow, dtheta_l2, dtheta_max) of a flow and of the adjoint of dflow_of(shape) against float64."""
    vol = tuple(shape[2:])
    ref = affine_flow_ref(theta.double(), vol)
    l2, mx = _l2_max(dtheta, affine_flow_adjoint_ref(dflow_of(shape).double()))
    return dict(flow=float((flow.detach().cpu().double() - ref).abs().max()), dtheta_l2=l2, dtheta_max=mx)


_REF = {}


def reference(shape, kind, mask):
    """((M, F, theta, m), system_ref in float64) of a case, computed once and shared."""
    key = (shape, kind, mask)
    if key not in _REF:
        inp = inputs(shape, kind, mask)
        _REF[key] = (inp, system_ref(*inp))
    return _REF[key]


# ------------------------------------------------------------------------------------------ the recovery fixtures
RECOVERY_VOLS = ((24, 32), (12, 16, 20))
RECOVERY_SEED = {2: 41, 3: 43}


def blobs(vol, seed, n=6):
    """A seeded sum of n Gaussian blobs [1,1,*vol] in float64: sigma in [2, 5] voxels, centres in the middle half."""
    nd = len(vol)
    g = _grid(vol, torch.float64)
    ctr = (0.25 + 0.5 * C.rand(seed, n, nd).double()) * (torch.tensor(vol, dtype=torch.float64) - 1.0)
    sig = 2.0 + 3.0 * C.rand(seed + 1, n).double()
    amp = 0.5 + 0.5 * C.rand(seed + 2, n).double()
    img = torch.zeros(vol, dtype=torch.float64)
    for i in range(n):
        d2 = sum((g[a] - ctr[i, a]) ** 2 for a in range(nd))
        img = img + amp[i] * torch.exp(-0.5 * d2 / sig[i] ** 2)
    return img[None, None]


def true_theta(nd, seed):
    """theta* [1,nd,nd+1] float64: rotation <= 6 degrees, scale within +-5 %, shear <= 0.04, |t| <= 2 voxels."""
    u = C.rand(seed, 16).double() * 2 - 1
    if nd == 2:
        a = math.radians(6.0) * float(u[0])
        R = torch.tensor([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]], dtype=torch.float64)
    else:
        R = torch.eye(3, dtype=torch.float64)
        for i, (p, q) in enumerate(((0, 1), (0, 2), (1, 2))):
            a = math.radians(6.0 / math.sqrt(3.0)) * float(u[i])
            Ri = torch.eye(3, dtype=torch.float64)
            Ri[p, p], Ri[p, q], Ri[q, p], Ri[q, q] = math.cos(a), -math.sin(a), math.sin(a), math.cos(a)
            R = R @ Ri
    Sc = torch.diag(1.0 + 0.05 * u[3:3 + nd])
    Sh = torch.eye(nd, dtype=torch.float64)
    for i, (p, q) in enumerate(itertools.combinations(range(nd), 2)):
        Sh[p, q] = 0.04 * float(u[6 + i])
    t = 2.0 * u[9:9 + nd]
    return torch.cat([R @ Sc @ Sh, t[:, None]], 1)[None]


def sample_at(img, theta):
    """img sampled at y_theta(x) (float64 grid_sample, zero padding)."""
    vol = tuple(img.shape[2:])
    f = _grid(vol, img.dtype)[None] + affine_flow_ref(theta.to(img.dtype), vol)
    grid = torch.stack([2.0 * f[:, a] / (vol[a] - 1) - 1.0 for a in range(len(vol))][::-1], -1)
    return F.grid_sample(img, grid.expand(img.shape[0], *grid.shape[1:]), mode='bilinear', padding_mode='zeros', align_corners=True)


_FIX = {}


def recovery_fixture(vol):
    """(moving, fixed, theta*) in float64: fixed = moving sampled at y_theta*(x)."""
    if vol not in _FIX:
        nd = len(vol)
        moving = blobs(vol, RECOVERY_SEED[nd])
        star = true_theta(nd, RECOVERY_SEED[nd] + 5)
        _FIX[vol] = (moving, sample_at(moving, star), star)
    return _FIX[vol]


# ------------------------------------------------------------------------------------------ CPU tier
def test_abi_rows_load_and_refuse_bad_arguments_without_a_device():
    import dfmir_amd
    h = dfmir_amd.lib()
    assert h.dfmir_abi_version() == 14
    assert h.dfmir_affine_ws_floats(3, 1, 160, 192, 224) > 0 and h.dfmir_affine_ws_floats(2, 2, 1, 9, 13) > 0
    for bad in ((4, 1, 4, 4, 4), (1, 1, 4, 4, 4), (3, 0, 4, 4, 4), (3, 1, 1, 4, 4), (2, 1, 1, 1, 4), (3, 1, 4, 4, 1),
                (3, 1, 1024, 1024, 1024)):
        assert h.dfmir_affine_ws_floats(*bad) == -1, bad
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.c_void_p(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16)          # aligned host memory: never launched on

    def refused(rc):
        assert rc != 0 and b"invalid argument" in h.dfmir_last_error()

    refused(h.dfmir_affine_flow(3, None, p, 1, 4, 4, 4, None))
    refused(h.dfmir_affine_flow(3, p, None, 1, 4, 4, 4, None))
    for nd, B, D, H, W in ((4, 1, 4, 4, 4), (3, 0, 4, 4, 4), (3, 1, 1, 4, 4), (2, 1, 1, 1, 4), (3, 2, 1024, 1024, 512)):
        refused(h.dfmir_affine_flow(nd, p, p, B, D, H, W, None))
        refused(h.dfmir_affine_flow_bwd(nd, p, p, p, B, D, H, W, None))
        refused(h.dfmir_affine_system(nd, p, p, p, None, p, p, 1, B, 4, D, H, W, None))
    refused(h.dfmir_affine_flow_bwd(3, p, None, p, 1, 4, 4, 4, None))
    for Cn in (0, 17):
        refused(h.dfmir_affine_system(3, p, p, p, None, p, p, 1, 1, Cn, 4, 4, 4, None))
    for args in ((None, p, p, p, p), (p, None, p, p, p), (p, p, None, p, p), (p, p, p, None, p), (p, p, p, p, None)):
        refused(h.dfmir_affine_system(3, args[0], args[1], args[2], None, args[3], args[4], 0, 1, 4, 4, 4, 4, None))
    ok = (3, p, p, p, p, p, p, p, 1, 0, 0, 10.0, 0.1, None)
    for i, v in ((0, 4), (1, None), (4, None), (7, None), (8, 0), (9, -1), (11, 1.0), (12, 0.0), (12, 1.5)):
        a = list(ok)
        a[i] = v
        refused(h.dfmir_affine_lm_step(*a))


def test_value_errors_are_raised_before_any_launch():
    from dfmir_amd import infer, losses, ops
    mov, fix = torch.zeros(2, 1, 8, 12), torch.zeros(2, 1, 8, 12)
    th = torch.eye(2, 3).repeat(2, 1, 1)
    E = pytest.raises(ValueError)
    with E: ops.affine_flow(th, (8,))
    with E: ops.affine_flow(th, (1, 8))
    with E: ops.affine_flow(th, (8, 8, 8))
    with E: ops.affine_flow(th.double(), (8, 8))
    with E: ops.affine_flow(th[0], (8, 8))
    with E: ops.affine_flow(th, (8, 2.0))
    with E: ops.affine_flow(torch.zeros(2, 3, 4), (1 << 10, 1 << 10, 1 << 10))
    with E: ops.affine_identity(0, 2, "cpu")
    with E: ops.affine_identity(1, 4, "cpu")
    assert torch.equal(ops.affine_identity(2, 2, "cpu"), th)
    for fn in (ops.affine_ssd, ops.affine_ssd_system):
        with E: fn(mov, fix, th[:1])
        with E: fn(mov, fix, th.double())
        with E: fn(mov, fix, torch.zeros(2, 3, 4))
        with E: fn(mov, fix[:, :, :4], th)
        with E: fn(torch.zeros(2, 17, 8, 12), torch.zeros(2, 17, 8, 12), th)
        with E: fn(mov, fix.double(), th)
        with E: fn(mov.clone().requires_grad_(), fix, th)
        with E: fn(mov, fix.clone().requires_grad_(), th)
        with E: fn(mov, fix, th, mask=torch.ones(2, 1, 8, 12).requires_grad_())
        with E: fn(mov, fix, th, mask=torch.ones(2, 1, 8, 5))
        with E: fn(mov[0], fix[0], th)
    flow = torch.zeros(2, 2, 8, 12)
    for fn in (ops.warp_ssd, ops.warp_ssd_per_sample):                    # the shipped op's own contract, which shares the checks
        with E: fn(mov, fix, None)
        with E: fn(mov, fix, flow.double())
        with E: fn(mov, fix[:, :, :4], flow)
    with E: losses.AffineSSD_Loss(dim=4)
    with E: losses.AffineSSD_Loss(dim=3)(mov, fix, th)
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64)
    good = (f64(2), f64(2, 6), f64(2, 6, 6), th.clone(), th.clone(), f64(2, 44), f64(2, 5), 0)
    for i, v in ((0, f64(3)), (1, f64(2, 6).float()), (2, f64(2, 6, 5)), (3, th.double()), (5, f64(2, 43)), (6, f64(2, 4)),
                 (7, -1), (7, 1.0)):
        a = list(good)
        a[i] = v
        with E: ops.affine_lm_step(*a)
    with E: ops.affine_lm_step(*good, dof='rigid')
    with E: ops.affine_lm_step(*good, mu_up=1.0)
    with E: ops.affine_lm_step(*good, mu_down=0.0)
    kw = dict(features='intensity')
    with E: infer.affine_init(mov, fix[:1], **kw)
    with E: infer.affine_init(mov[0], fix[0], **kw)
    with E: infer.affine_init(mov, fix, features='ncc')
    with E: infer.affine_init(mov.repeat(1, 2, 1, 1), fix.repeat(1, 2, 1, 1), **kw)
    with E: infer.affine_init(mov, fix, dof='rigid', **kw)
    with E: infer.affine_init(mov, fix, theta=th[:1], **kw)
    with E: infer.affine_init(mov, fix, theta=th.double(), **kw)
    with E: infer.affine_init(mov, fix, levels=(8,), **kw)                 # 8 // 8 = 1 < 2
    with E: infer.affine_init(mov, fix, levels=(0,), **kw)
    with E: infer.affine_init(mov, fix, levels=(2.0,), **kw)
    with E: infer.affine_init(mov, fix, levels=(), **kw)
    with E: infer.affine_init(mov, fix, levels=(2, 1), iters=(3,), **kw)
    with E: infer.affine_init(mov, fix, iters=-1, **kw)
    with E: infer.affine_init(mov, fix, iters=2.0, **kw)
    for bad in (dict(mu0=0.0), dict(mu0=float('nan')), dict(mu0=float('inf')), dict(mu_up=1.0), dict(mu_up=float('inf')),
                dict(mu_down=0.0), dict(mu_down=1.5), dict(mu_down=float('nan'))):
        with E: infer.affine_init(mov, fix, **kw, **bad)


@pytest.mark.parametrize("shape", SHAPES[:5], ids=_id)
def test_restated_gradient_matches_autograd_through_grid_sample(shape):
    """g (and gb) from the closed form against autograd through grid_sample on y(x), on the lattice thetas (no sample within
    0.05 of a cell face); the closed form's own value against grid_sample's; the flow's adjoint against autograd."""
    for mask in ("none", "partial"):
        (M, Fx, theta, m), ref = reference(shape, "lattice", mask)
        vol = tuple(shape[2:])
        assert face_distance(theta, vol) >= 0.05
        th = theta.double().requires_grad_()
        md = None if m is None else m.double()
        L, Lb = ssd_grid_sample(M.double(), Fx.double(), affine_flow_ref(th, vol), md)
        (gb,) = torch.autograd.grad(L, th, retain_graph=True)
        assert torch.allclose(gb, ref['gb'], rtol=1e-9, atol=1e-13)
        g = torch.stack([torch.autograd.grad(Lb[b], th, retain_graph=True)[0][b] for b in range(shape[0])])
        assert torch.allclose(g.reshape(shape[0], -1), ref['g'], rtol=1e-9, atol=1e-13)
        assert torch.allclose(ref['val'], ref['Lb'], rtol=1e-11, atol=0)
        d = dflow_of(shape).double()
        (dt,) = torch.autograd.grad((affine_flow_ref(th, vol) * d).sum(), th)
        assert torch.allclose(dt, affine_flow_adjoint_ref(d), rtol=1e-12, atol=1e-12)


def test_restated_H_is_symmetric_psd_and_the_sum_of_J_JT():
    shape = (2, 1, 3, 7, 9)
    for mask in ("none", "partial"):
        (M, Fx, theta, m), ref = reference(shape, "lattice", mask)
        B, Cn = shape[:2]
        vol = tuple(shape[2:])
        nd, S = len(vol), math.prod(vol)
        H = ref['H']
        assert float((H - H.transpose(1, 2)).abs().max()) <= 1e-15 * float(H.abs().max())
        assert float(torch.linalg.eigvalsh(H).min()) >= -1e-12 * float(H.abs().max())
        f = _grid(vol, torch.float64)[None] + affine_flow_ref(theta.double(), vol)
        _, dM = sample_closed(M.double(), f)
        qe = qe_of(vol, torch.float64).reshape(nd + 1, S)
        mw = torch.ones(B, S, dtype=torch.float64) if m is None else m.double().reshape(B, S)
        for b in range(B):
            want = torch.zeros(nd * (nd + 1), nd * (nd + 1), dtype=torch.float64)
            for c in range(Cn):
                for x in range(S):
                    J = (dM[b, c].reshape(nd, S)[:, x, None] * qe[None, :, x]).reshape(-1)      # d e_c(x) / d theta, (a, j)
                    want += mw[b, x] * J[:, None] * J[None]
            assert torch.allclose(H[b], want * 2.0 / (Cn * mw[b].sum()), rtol=1e-10, atol=1e-14)


@pytest.mark.parametrize("vol", RECOVERY_VOLS, ids=_id)
def test_restated_loop_recovers_theta(vol):
    """One level of stride 1, the default mu schedule, intensity features: max |theta - theta*| < 1e-6 within 8 evaluations."""
    moving, fixed, star = recovery_fixture(vol)
    th, hist = affine_init_ref(moving, fixed, levels=(1,), iters=8)
    print("max |theta - theta*| = %.3e, L: %s" % (float((th - star).abs().max()), ["%.2e" % v for v in hist[:, 0, 0].tolist()]))
    assert float((th - star).abs().max()) < 1e-6
    acc = hist[:, 0, 1]
    assert bool((acc[1:] <= acc[:-1]).all())


@pytest.mark.parametrize("vol", RECOVERY_VOLS, ids=_id)
def test_restated_loop_two_levels_and_translation(vol):
    """Levels (2, 1) recover the same theta*; dof='translation' on a pure shift recovers t and leaves A bit-identical."""
    moving, fixed, star = recovery_fixture(vol)
    th, _ = affine_init_ref(moving, fixed, levels=(2, 1), iters=8)
    assert float((th - star).abs().max()) < 1e-6
    nd = len(vol)
    shift = torch.eye(nd, nd + 1, dtype=torch.float64)[None].clone()
    shift[0, :, nd] = torch.tensor([1.3, -0.7, 0.9][:nd], dtype=torch.float64)
    th, _ = affine_init_ref(moving, sample_at(moving, shift), dof='translation', levels=(1,), iters=8)
    assert torch.equal(th[:, :, :nd], shift[:, :, :nd])
    assert float((th - shift).abs().max()) < 1e-6


# ------------------------------------------------------------------------------------------ GPU tier
def _gpu_flow(theta, shape):
    """(flow, dtheta of dflow_of(shape)) from ops.affine_flow."""
    from dfmir_amd import ops
    th = theta.to(DEV).requires_grad_()
    flow = ops.affine_flow(th, tuple(shape[2:]))
    flow.backward(dflow_of(shape).to(DEV))
    return flow.detach().cpu(), th.grad.cpu()


def _gpu_system(M, Fx, theta, m, form):
    """dict(L, Lb, gb, g, H) from ops.affine_ssd (+ backward) and ops.affine_ssd_system, and the same (L, gb) from the shipped
    ops.warp_ssd at ops.affine_flow(theta)."""
    from dfmir_amd import ops
    mov = ops.pack_features(M.to(DEV)) if form == "packed" else M.to(DEV)
    Fd, md = Fx.to(DEV), None if m is None else m.to(DEV)
    th = theta.to(DEV).requires_grad_()
    L = ops.affine_ssd(mov, Fd, th, md)
    L.backward()
    Lb, g, H = ops.affine_ssd_system(mov, Fd, th.detach(), md)
    th2 = theta.to(DEV).requires_grad_()
    L2 = ops.warp_ssd(mov, Fd, ops.affine_flow(th2, tuple(M.shape[2:])), md)
    L2.backward()
    torch.cuda.synchronize()
    assert L.dtype == torch.float32 and Lb.dtype == g.dtype == H.dtype == torch.float64 and not g.requires_grad
    return (dict(L=L.detach().cpu(), Lb=Lb.cpu(), gb=th.grad.cpu(), g=g.cpu(), H=H.cpu()),
            dict(L=L2.detach().cpu(), gb=th2.grad.cpu()))


def _bounded(errs, what, shape, factor=1.0):
    bound = BOUND[group_of(shape)]
    print("%s: " % what + "  ".join("%s %.3e (bound %.1e)" % (k, v, factor * bound[k]) for k, v in errs.items()))
    assert all(v <= factor * bound[k] for k, v in errs.items()), (what, errs)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_affine_flow_matches_float64_and_is_reproducible(shape, kind):
    theta = thetas(shape, kind, 1300 + 19 * SHAPES.index(shape) + 7)
    flow, dtheta = _gpu_flow(theta, shape)
    assert bool(torch.isfinite(flow).all()) and bool(torch.isfinite(dtheta).all())
    _bounded(flow_errors(flow, dtheta, theta, shape), "affine_flow %s %s" % (_id(shape), kind), shape)
    again = _gpu_flow(theta, shape)
    assert torch.equal(flow, again[0]) and torch.equal(dtheta, again[1])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_affine_ssd_and_system_match_float64_warp_ssd_and_are_reproducible(shape, kind):
    """affine_ssd's value and dtheta, affine_ssd_system's L_b, g and H against float64; affine_ssd against the shipped
    warp_ssd at affine_flow(theta) and its autograd gradient; every output bit-identical on a second run; the packed handle
    and a plain tensor as `mov` give the same bits."""
    for mask in MASKS:
        (M, Fx, theta, m), ref = reference(shape, kind, mask)
        if kind != "identity":
            assert face_distance(theta, tuple(shape[2:])) >= 0.05
        what = "%s %s %s" % (_id(shape), kind, mask)
        got, ws = _gpu_system(M, Fx, theta, m, "packed")
        for v in got.values():
            assert bool(torch.isfinite(v).all()), what
        _bounded(system_errors(got, ref), "system " + what, shape)
        pair = dict(L=_rel(got['L'].reshape(1), ws['L'].reshape(1)))
        pair["gb_l2"], pair["gb_max"] = _l2_max(got['gb'], ws['gb'])
        _bounded(pair, "affine_ssd against warp_ssd " + what, shape, factor=2.0)
        for form in FORMS:
            again, _ = _gpu_system(M, Fx, theta, m, form)
            assert all(torch.equal(got[k], again[k]) for k in got), (what, form)
        if kind == "outside" or mask == "zero":
            assert float(got['g'].abs().max()) == 0.0 and float(got['H'].abs().max()) == 0.0 and float(got['gb'].abs().max()) == 0.0
        if mask == "zero":
            assert float(got['L']) == 0.0 and float(got['Lb'].abs().max()) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("dof", ("affine", "translation"))
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]], ids=_id)
def test_lm_step_matches_the_float64_solve_of_the_same_system(shape, dof):
    """af_lm_k on a (L, g, H) that is FED IN (the float64 restatement's), three steps: accept at k = 0, accept or reject at
    k = 1 by a doctored L, a NaN L (rejected, solved from the kept system) and the guard row (H = 0: singular, trial = theta_acc).  Both sides solve in float64, so they agree far
    below an fp32 ulp: the trial may differ by the rounding to fp32 alone (one ulp of max(1, |theta|))."""
    from dfmir_amd import ops
    (M, Fx, theta, m), ref = reference(shape, "lattice", "none")
    B, nd = shape[0], len(shape) - 2
    P = nd * (nd + 1)
    acc, trial = theta.to(DEV).clone(), theta.to(DEV).clone()
    state = ops.affine_lm_state(B, nd, 1e-3, DEV)
    sts = [dict(acc=theta[b].reshape(P).clone(), trial=theta[b].reshape(P).clone(), L_acc=float('inf'), mu=1e-3,
                g=torch.zeros(P, dtype=torch.float64), H=torch.zeros(P, P, dtype=torch.float64)) for b in range(B)]
    steps = [(ref['Lb'], ref['g'], ref['H']),
             (ref['Lb'] * torch.tensor([0.5, 2.0][:B], dtype=torch.float64), ref['g'] * 0.5, ref['H'] * 1.5),
             (ref['Lb'] * float('nan'), ref['g'], ref['H']),
             (ref['Lb'] * 0.25, ref['g'], ref['H'] * 0.0)]
    for k, (L, g, H) in enumerate(steps):
        hist = torch.empty(B, 5, device=DEV, dtype=torch.float64)
        ops.affine_lm_step(L.to(DEV), g.to(DEV), H.to(DEV), acc, trial, state, hist, k, dof)
        want = [lm_step_ref(L[b], g[b], H[b], sts[b], k, nd, dof, 10.0, 0.1, torch.float32) for b in range(B)]
        hist = hist.cpu()
        for b in range(B):
            assert hist[b, 3:].tolist() == want[b][3:], (k, b)
            for i in range(3):
                a, w = float(hist[b, i]), want[b][i]
                assert (math.isnan(a) and math.isnan(w)) or abs(a - w) <= 1e-14 * abs(w), (k, b, i, a, w)
            assert torch.equal(acc[b].cpu().reshape(P), sts[b]['acc'].float())
            tol = 2.0 ** -23 * sts[b]['trial'].abs().clamp_min(1.0).double()
            assert bool(((trial[b].cpu().reshape(P).double() - sts[b]['trial'].double()).abs() <= tol).all()), (k, b)
            fixed_par = [i for i in range(P) if i not in _free(nd, dof)]
            assert torch.equal(trial[b].cpu().reshape(P)[fixed_par], theta[b].reshape(P)[fixed_par])
            sts[b]['trial'] = trial[b].cpu().reshape(P).clone()          # (go on from the kernel's own rounding)
    assert hist[:, 4].tolist() == [1.0] * B and hist[:, 3].tolist() == [1.0] * B and torch.equal(trial, acc)     # the guard row


@pytest.mark.gpu
@pytest.mark.parametrize("vol", RECOVERY_VOLS, ids=_id)
def test_affine_init_recovers_theta_and_keeps_its_contract(vol):
    from dfmir_amd import infer, ops
    moving, fixed, star = recovery_fixture(vol)
    nd = len(vol)
    mov, fix = moving.float().repeat(2, 1, 1, *([1] * (nd - 1))), fixed.float().repeat(2, 1, 1, *([1] * (nd - 1)))
    ref, _ = affine_init_ref(mov[:1], fix[:1], levels=(1,), iters=8)
    out = infer.affine_init(mov.to(DEV), fix.to(DEV), features='intensity', levels=(1,), iters=8)
    again = infer.affine_init(mov.to(DEV), fix.to(DEV), features='intensity', levels=(1,), iters=8)
    th, hist = out['theta'].cpu(), out['history'].cpu()
    gap = float((th.double() - ref).abs().max())
    print("max |theta - theta(float64 loop)| = %.3e (bound %.1e), against theta*: %.3e"
          % (gap, FACTOR * THETA_FP32_GAP, float((th.double() - star).abs().max())))
    assert gap <= FACTOR * THETA_FP32_GAP
    assert torch.equal(th[0], th[1])
    for k in ("theta", "flow", "warped", "history"):
        assert torch.equal(out[k], again[k]), k
    assert tuple(hist.shape) == (8, 2, 5) and hist.dtype == torch.float64
    acc = hist[:, :, 1]
    assert bool((acc[1:] <= acc[:-1]).all())
    prev = torch.cat([torch.full((1, 2), float('inf'), dtype=torch.float64), acc[:-1]])
    assert torch.equal(hist[:, :, 3], (hist[:, :, 0] <= prev).double())
    assert torch.equal(torch.where(hist[:, :, 3] > 0, hist[:, :, 0], prev), acc)
    assert torch.equal(out['flow'], ops.affine_flow(out['theta'], vol))
    assert torch.equal(out['warped'], ops.warp(mov.to(DEV), out['flow']))
    # levels (2, 1), 6 evaluations each, intensity features and a mask of ones: the pooling of features and mask and the
    # t / s, s t hand-over between levels.  The float64 loop's 1e-6 condition for two levels is the CPU tier's; the bound here is
    # for the wiring: a wrong hand-over or centre shows as an error of (s - 1) / 2 = 0.5 voxel in t or of order 1e-2 in A, the
    # fp32 evaluation as 1e-7 (profiles/affine_margins.txt), and 1e-3 lies between the two
    multi = infer.affine_init(mov.to(DEV), fix.to(DEV), features='intensity', levels=(2, 1), iters=(6, 6),
                              mask=torch.ones(1, 1, *vol, device=DEV))
    hm = multi['history'].cpu()
    assert tuple(hm.shape) == (12, 2, 5)
    for lv in (hm[:6, :, 1], hm[6:, :, 1]):
        assert bool((lv[1:] <= lv[:-1]).all())
    assert float((multi['theta'].cpu().double() - star).abs().max()) < 1e-3


@pytest.mark.gpu
def test_affine_init_guards_translation_and_iters_zero():
    from dfmir_amd import infer, ops
    vol = RECOVERY_VOLS[0]
    moving, fixed, _ = recovery_fixture(vol)
    mov, fix = moving.float().to(DEV), fixed.float().to(DEV)
    start = thetas((1, 1) + vol, "lattice", 5).to(DEV)
    out = infer.affine_init(mov, fix, features='intensity', theta=start, iters=0)
    assert torch.equal(out['theta'], start) and tuple(out['history'].shape) == (0, 1, 5)
    assert torch.equal(out['flow'], ops.affine_flow(start, vol))
    out = infer.affine_init(mov, fix, features='intensity', theta=start, levels=(2, 1), iters=(0, 0))
    assert torch.equal(out['theta'], start)
    strided = torch.empty(1, 3, 2, device=DEV).transpose(1, 2).copy_(start)          # a start that is not contiguous
    assert not strided.is_contiguous()
    a, b = (infer.affine_init(mov, fix, features='intensity', theta=t, levels=(1,), iters=2) for t in (start, strided))
    assert torch.equal(a['theta'], b['theta']) and torch.equal(a['history'], b['history'])
    # translation only: A keeps its starting value bit for bit and a pure shift is found (1e-3: as for the two-level run above,
    # between the fp32 evaluation's 1e-7 and the 0.1 voxel or more of a column that is not free or not updated)
    shift = torch.eye(2, 3, dtype=torch.float64)[None].clone()
    shift[0, :, 2] = torch.tensor([1.3, -0.7], dtype=torch.float64)
    out = infer.affine_init(mov, sample_at(moving, shift).float().to(DEV), features='intensity', dof='translation', levels=(1,),
                            iters=8)
    th = out['theta'].cpu()
    assert torch.equal(th[:, :, :2], torch.eye(2)[None])
    assert float((th.double() - shift).abs().max()) < 1e-3
    # a zero mask and a start that samples nothing: everything is 0, the solver flags the row and theta stays
    for kw in (dict(mask=torch.zeros(1, 1, *vol, device=DEV), theta=start),
               dict(theta=thetas((1, 1) + vol, "outside", 5).to(DEV))):
        out = infer.affine_init(mov, fix, features='intensity', levels=(1,), iters=3, **kw)
        h = out['history'].cpu()
        assert torch.equal(out['theta'], kw['theta'])
        assert h[:, :, 4].tolist() == [[1.0]] * 3 and bool(torch.isfinite(out['flow']).all())
    out = infer.affine_init(mov, fix, levels=(2,), iters=2)                      # the MIND default, pooled
    assert bool(torch.isfinite(out['theta']).all()) and tuple(out['history'].shape) == (2, 1, 5)
    from dfmir_amd.losses import AffineSSD_Loss
    assert torch.equal(AffineSSD_Loss(dim=2)(mov, fix, start), ops.affine_ssd(mov, fix, start))
