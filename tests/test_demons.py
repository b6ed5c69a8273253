"""The demons solver (build-defined, dfmir_amd/csrc/gauss.hip and demons.hip): ops.gaussian_smooth, ops.demons_force and
infer.demons_flow.  CPU: the argument checks; a float64 restatement of the definitions -- the Gaussian as the per-axis F.conv of
the tensor divided by the same F.conv of ones, the force from explicit floor / gather sampling (tests/test_affine.py's
sample_closed) with torch.linalg.solve per voxel, the driver's loop as infer.demons_flow states it with F.avg_pool,
F.interpolate(align_corners=True) * mult and F.grid_sample -- checked against itself (the C = 1 closed form, J against autograd
through grid_sample, the step bound, the guards, L against mean (warped - F)^2) and on two recovery fixtures.  GPU: the kernels
against the restatement, against the shipped ops.warp_ssd, and run to run.

Which launch each GPU shape reaches.  dfmir_gauss_smooth: gs_tile_k<TH, XF, VEC> -- XF = the x axis is filtered (a 32 x 64 tile
with an x halo, else 64 x 64), VEC = 16-byte accesses (row length % 4 == 0 and aligned pointers); 3-D runs it per plane over
(y, x) and again as the z pass on the view [B C][D][H W]:
  (2,2,9,13) sigma (1, 2)             <32, XF, scalar>, one tile            (2,2,8,16) sigma 1.5        <32, XF, VEC>
  (2,3,5,12,24) sigma (0, 1.5, 0.7)   <32, XF, VEC> alone: the z pass is skipped, nothing goes through tmp
  (1,3,3,7,9) sigma 4                 r = 12 on every axis, every window wider than its axis; <32, XF, scalar> then the z pass
                                      <64, no XF, scalar> (H W = 63)
  (1,16,2,6,8) sigma 1                <32, XF, VEC> then the z pass <64, no XF, VEC> (H W = 48)
  (1,1,64,64) sigma 16 / 3            r = 16 = ops.GAUSS_MAX_RADIUS, two tiles along y
  (1,2,300,260) sigma 2.5             r = 8: 10 x 5 tiles, partial tiles on both axes
  (1,3,40,70,72) sigma 2.5            3 x 2 tiles per plane, and a z pass over 5040 columns = 79 tiles, 40 rows in one tile
  and, on (2,3,6,10,12): sigma (1.2, 0, 0) (the z pass alone), a non-contiguous input (copied) and an input that starts 4 bytes
  off a 16-byte boundary (the scalar launch on a shape that otherwise takes the 16-byte one).
dfmir_demons_force: dm_fwd_k<ND, VPT>, VPT = 4 -- 16-byte accesses of the flow, F and d -- when W % 4 == 0 (the staging is
ws_fwd_k's, a workgroup owns 256 VPT voxels; the launch does not walk chunks, so tests/test_affine.py's large shape adds no path):
  <2-D, 1> (2,4,9,13)    <2-D, 4> (2,4,8,16)    <3-D, 4> (2,12,5,12,24) 1440 voxels = 2 workgroups per sample, three channel
  groups; (1,5,2,6,8) C = 5: a second group with one live channel    <3-D, 1> (2,1,3,7,9) C = 1
ws_fin_k (without its scale output) runs after every force.

Flows of the force cases, a different one per sample (tests/test_affine.py's thetas, turned into dense fp32 fields): `zero`;
`lattice` = smooth, offsets near integer + 0.5, every sample point at least 0.05 from a cell face (asserted on the fp32 field);
`shifted` = the same pushed a third of the x extent, which puts a third of the points past a face; `outside` = twice the extent on
every axis: no corner is inside, d must be exactly 0 and L_b the mean of F^2.  M and F are noise in [-1, 1].  Masks: none, `partial`
(float weights, zero on a third of the voxels) and `zero`.

Tolerances (profiles/demons_margins.txt, profiles/demons_margins_cpu.txt): every kernel-against-float64 comparison is bounded by
4x the error of the SAME definition evaluated by torch in fp32 on the CPU against float64, on these inputs, the maximum over the
case set per quantity (over the small shapes and over the large ones separately): fields in relative 2-norm and as max-abs over
max, values relative.  scripts/demons_margins.py measures them, with the kernels' own errors beside them.  L against warp_ssd
compares two fp32 kernels: 2x that bound.  The flow and the history of infer.demons_flow are bounded by 4x the gap between the
fp32 CPU restatement of the whole loop and float64, per fixture and variant."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import test_affine as TA
from tests.golden import common as C

DEV = "cuda"
FACTOR = 4.0
# rows "max" of the fp32 CPU columns.  The fp32 figures depend on the host (torch orders its sums by the thread count), so two
# runs are recorded: profiles/demons_margins.txt (a host with the device: the kernels' errors stand beside) and
# profiles/demons_margins_cpu.txt (a host without one).  Per quantity the SMALLER of the two stands here.
FP32_ERR = {"gauss": {"small": {"l2": 1.66e-07, "max": 3.30e-07}, "large": {"l2": 1.70e-07, "max": 2.95e-07}},
            "force": {"small": {"d_l2": 5.50e-06, "d_max": 2.78e-05, "L": 1.56e-07, "Lb": 1.78e-07}}}
# max |flow(fp32 CPU loop) - flow(float64 loop)| in voxels and max relative gap of the history, per (fixture, variant): the
# smaller of the two files' figures
LOOP_FP32_GAP = {("2d", "compose"): {"flow": 1.17e-05, "history": 2.39e-06}, ("3d", "compose"): {"flow": 4.28e-05, "history": 1.75e-06},
                 ("2d", "add"): {"flow": 8.05e-06, "history": 2.87e-06}, ("2d", "diffeomorphic"): {"flow": 1.44e-05, "history": 1.64e-06}}

GAUSS_CASES = [((2, 2, 9, 13), (1.0, 2.0)), ((2, 2, 8, 16), 1.5), ((2, 3, 5, 12, 24), (0.0, 1.5, 0.7)), ((1, 3, 3, 7, 9), 4.0),
               ((1, 16, 2, 6, 8), 1.0), ((1, 1, 64, 64), 16.0 / 3.0), ((1, 2, 300, 260), 2.5), ((1, 3, 40, 70, 72), 2.5)]
FORCE_SHAPES = TA.SHAPES[:5]
KINDS = ("zero", "lattice", "shifted", "outside")
MASKS = TA.MASKS
MAX_STEP = 2.0


def group_of(shape):
    return "large" if math.prod(shape) > 100000 else "small"


def _id(v):
    return "x".join(str(n) for n in v)


# ------------------------------------------------------------------------------------------ restatement: the Gaussian
def _sigmas(sigma, nd):
    return (float(sigma),) * nd if isinstance(sigma, (int, float)) else tuple(float(s) for s in sigma)


def gauss_weights(sigma, truncate=3.0):
    """(r, w [2 r + 1] float64): r = ceil(truncate * sigma), w[k] = exp(-k^2 / (2 sigma^2))."""
    r = int(math.ceil(truncate * sigma))
    return r, torch.tensor([math.exp(-k * k / (2.0 * sigma * sigma)) if k else 1.0 for k in range(-r, r + 1)], dtype=torch.float64)


def gauss_ref(x, sigma, truncate=3.0, dtype=torch.float64):
    """ops.gaussian_smooth on the CPU in `dtype`: per axis, F.conv1d of the tensor (zero padding) divided by the same
    F.conv1d of ones; the weights are the fp32 roundings of the float64 values, as the kernel receives them."""
    nd = x.dim() - 2
    y = x.detach().cpu().to(dtype)
    for a, sg in enumerate(_sigmas(sigma, nd)):
        if sg == 0.0:
            continue
        r, w = gauss_weights(sg, truncate)
        w = w.float().to(dtype).reshape(1, 1, -1)
        t = y.movedim(2 + a, -1)
        shp = t.shape
        rows = t.reshape(-1, 1, shp[-1])
        num = F.conv1d(rows, w, padding=r)
        den = F.conv1d(torch.ones(1, 1, shp[-1], dtype=dtype), w, padding=r)
        y = (num / den).reshape(shp).movedim(-1, 2 + a)
    return y.contiguous()


def gauss_input(shape, seed=2100):
    return C.rand(seed + sum(shape), *shape) * 2 - 1


def field_errors(got, ref, prefix=""):
    l2, mx = TA._l2_max(got, ref)
    return {prefix + "l2": l2, prefix + "max": mx}


# ------------------------------------------------------------------------------------------ restatement: the force
def demons_force_ref(M, Fx, phi, mask=None, max_step=MAX_STEP, dtype=torch.float64):
    """dict(d [B,nd,*vol], L, Lb [B], J [B,C,nd,*vol], val [B,C,*vol]) of ops.demons_force on the CPU in `dtype`: explicit floor /
    gather sampling, then per voxel d = -(H + (s / max_step^2) I)^-1 g by torch.linalg.solve; d = 0 where g is exactly 0, where
    the mask weight is <= 0 and where a component of the solution is not finite (fp32: e^2 can underflow where e J does not)."""
    M, Fx, phi = (t.detach().cpu().to(dtype) for t in (M, Fx, phi))
    m = None if mask is None else mask.detach().cpu().to(dtype)
    B, Cn = M.shape[:2]
    vol = tuple(M.shape[2:])
    nd = len(vol)
    val, J = TA.sample_closed(M, TA._grid(vol, dtype)[None] + phi)
    e = val - Fx
    s = (e ** 2).mean(1)                                                          # [B,*vol]
    g = (e[:, :, None] * J).mean(1)                                               # [B,nd,*vol]
    H = torch.einsum('bca...,bcd...->bad...', J, J) / Cn                          # [B,nd,nd,*vol]
    gl = g.movedim(1, -1)                                                         # [B,*vol,nd]
    Hl = H.movedim(1, -1).movedim(1, -1)                                          # [B,*vol,nd,nd]
    live = (gl != 0).any(-1)
    if m is not None:
        live = live & (m.expand((B, 1) + vol)[:, 0] > 0)
    eye = torch.eye(nd, dtype=dtype)
    A = Hl + (s / max_step ** 2)[..., None, None] * eye
    A = torch.where(live[..., None, None], A, eye.expand_as(A))
    d = -torch.linalg.solve_ex(A, gl[..., None])[0][..., 0]                       # (no error on a singular matrix: inf / NaN)
    live = live & torch.isfinite(d).all(-1)                                       # a result that is not finite: the vector is 0
    d = torch.where(live[..., None], d, torch.zeros_like(d)).movedim(-1, 1).contiguous()
    L, Lb = TA._reduce(s[:, None], m)
    return dict(d=d, L=L, Lb=Lb, J=J, val=val)


def force_flow(shape, kind, seed):
    """The fp32 flow [B,nd,*vol] of a force case (see the module docstring)."""
    B, vol = shape[0], tuple(shape[2:])
    if kind == "zero":
        return torch.zeros(B, len(vol), *vol)
    return TA.affine_flow_ref(TA.thetas(shape, kind, seed).double(), vol).float()


def force_inputs(shape, kind, mask="none"):
    """(M, F, flow, mask or None) fp32 of a force case: tests/test_affine.py's features and masks."""
    M, Fx, _, m = TA.inputs(shape, "lattice", mask)
    return M, Fx, force_flow(shape, kind, 1300 + 19 * TA.SHAPES.index(shape) + 7), m


def face_distance(phi):
    f = TA._grid(tuple(phi.shape[2:]), torch.float64)[None] + phi.double()
    fr = f - torch.floor(f)
    return float(torch.minimum(fr, 1.0 - fr).min())


def force_errors(got, ref):
    out = field_errors(got['d'], ref['d'], "d_")
    out["L"] = TA._rel(got['L'].reshape(1), ref['L'].reshape(1))
    out["Lb"] = TA._rel(got['Lb'], ref['Lb'])
    return out


_REF = {}


def force_reference(shape, kind, mask):
    key = (shape, kind, mask)
    if key not in _REF:
        inp = force_inputs(shape, kind, mask)
        _REF[key] = (inp, demons_force_ref(*inp))
    return _REF[key]


# ------------------------------------------------------------------------------------------ restatement: the driver
def warp_ref(src, flow):
    """src(x + flow(x)): grid_sample, align_corners, zero padding."""
    vol = tuple(flow.shape[2:])
    f = TA._grid(vol, flow.dtype)[None] + flow
    grid = torch.stack([2.0 * f[:, a] / (vol[a] - 1) - 1.0 for a in range(len(vol))][::-1], -1)
    return F.grid_sample(src, grid, mode='bilinear', padding_mode='zeros', align_corners=True)


def resize_ref(u, vol, mult):
    return F.interpolate(u, size=vol, mode='bilinear' if len(vol) == 2 else 'trilinear', align_corners=True) * mult


def demons_flow_ref(Mm, Mf, flow=None, mask=None, levels=(4, 2, 1), iters=10, max_step=2.0, sigma_fluid=1.0, sigma_diffusion=1.0,
                    update='compose', diffeomorphic=False, exp_steps=4, dtype=torch.float64):
    """dict(flow, history, energy0, energy) of infer.demons_flow's loop on feature tensors, on the CPU in `dtype`."""
    Mm, Mf = Mm.detach().cpu().to(dtype), Mf.detach().cpu().to(dtype)
    mask = None if mask is None else mask.detach().cpu().to(dtype).expand((Mm.shape[0], 1) + tuple(Mm.shape[2:]))
    B, vol = Mm.shape[0], tuple(Mm.shape[2:])
    nd = len(vol)
    iters = (iters,) * len(levels) if isinstance(iters, int) else tuple(iters)
    u = torch.zeros((B, nd) + vol, dtype=dtype) if flow is None else flow.detach().cpu().to(dtype).clone()
    energy0 = TA.ssd_grid_sample(Mm, Mf, u, mask)[0]
    hist, s_prev = [], 1
    for s, n in zip(levels, iters):
        if n == 0:
            continue
        Lm, Lf, Lk = TA._pool(Mm, s), TA._pool(Mf, s), None if mask is None else TA._pool(mask, s)
        lvol = tuple(Lm.shape[2:])
        if s != s_prev or tuple(u.shape[2:]) != lvol:
            u = resize_ref(u, lvol, float(s_prev) / float(s))
        for _ in range(n):
            r = demons_force_ref(Lm, Lf, u, Lk, max_step, dtype)
            hist.append(r['L'])
            d = r['d']
            if sigma_fluid > 0:
                d = gauss_ref(d, sigma_fluid, dtype=dtype)
            if diffeomorphic:
                d = d * (2.0 ** -exp_steps)
                for _ in range(exp_steps):
                    d = d + warp_ref(d, d)
            u = d + warp_ref(u, d) if update == 'compose' else u + d
            if sigma_diffusion > 0:
                u = gauss_ref(u, sigma_diffusion, dtype=dtype)
        s_prev = s
    if s_prev != 1:
        u = resize_ref(u, vol, float(s_prev))
    return dict(flow=u, history=torch.stack(hist) if hist else torch.zeros(0, dtype=dtype), energy0=energy0,
                energy=TA.ssd_grid_sample(Mm, Mf, u, mask)[0])


FIXTURES = {"2d": dict(vol=(24, 32), amp=2.0, iters=(3, 3), seed=61), "3d": dict(vol=(12, 16, 20), amp=1.5, iters=(6, 6), seed=67)}
FIXTURE_KW = dict(levels=(2, 1), max_step=2.0, sigma_fluid=1.0, sigma_diffusion=1.0, update='compose')
VARIANTS = {"compose": {}, "add": dict(update='add'), "diffeomorphic": dict(diffeomorphic=True, exp_steps=4)}


def blobs(vol, seed, n=6):
    """The moving image [1,1,*vol] in float64: n seeded Gaussian blobs, centres in the middle 60 % of the volume, widths 0.08 to
    0.18 of the smallest extent, amplitudes 0.5 to 1.5."""
    nd = len(vol)
    g = TA._grid(vol, torch.float64)
    ctr = (0.2 + 0.6 * C.rand(seed, n, nd).double()) * (torch.tensor(vol, dtype=torch.float64) - 1.0)
    sig = (0.08 + 0.10 * C.rand(seed + 1, n).double()) * min(vol)
    amp = 0.5 + 1.0 * C.rand(seed + 2, n).double()
    img = torch.zeros(vol, dtype=torch.float64)
    for i in range(n):
        d2 = sum((g[a] - ctr[i, a]) ** 2 for a in range(nd))
        img = img + amp[i] * torch.exp(-0.5 * d2 / sig[i] ** 2)
    return img[None, None]


def true_field(vol, amp):
    """true_a = amp sin(2 pi x_b / n_b) sin(pi x_a / (n_a - 1)), b = a + 1 mod nd: [1,nd,*vol] float64, zero on axis a's faces."""
    nd = len(vol)
    g = TA._grid(vol, torch.float64)
    return torch.stack([amp * torch.sin(2 * math.pi * g[(a + 1) % nd] / vol[(a + 1) % nd]) * torch.sin(math.pi * g[a] / (vol[a] - 1))
                        for a in range(nd)])[None]


_FIX = {}


def fixture(name):
    """(moving, fixed) fp32 [1,1,*vol]: fixed = moving warped by the true field, formed in float64."""
    if name not in _FIX:
        f = FIXTURES[name]
        moving = blobs(f['vol'], f['seed'])
        _FIX[name] = (moving.float(), warp_ref(moving, true_field(f['vol'], f['amp'])).float())
    return _FIX[name]


_LOOP = {}


def loop_reference(name, variant, dtype=torch.float64):
    key = (name, variant, dtype)
    if key not in _LOOP:
        mov, fix = fixture(name)
        _LOOP[key] = demons_flow_ref(mov, fix, iters=FIXTURES[name]['iters'], dtype=dtype, **{**FIXTURE_KW, **VARIANTS[variant]})
    return _LOOP[key]


def loop_errors(got, ref):
    """dict(flow = max |flow - ref| in voxels, history = max relative gap)."""
    return dict(flow=float((got['flow'].detach().cpu().double() - ref['flow'].double()).abs().max()),
                history=TA._rel(got['history'], ref['history']))


# ------------------------------------------------------------------------------------------ CPU tier
def test_abi_rows_refuse_bad_arguments_without_a_device():
    import ctypes
    import dfmir_amd
    h = dfmir_amd.lib()
    assert h.dfmir_demons_ws_floats(3, 1, 12, 160, 192, 224) > 0 and h.dfmir_demons_ws_floats(2, 2, 4, 1, 9, 13) > 0
    for bad in ((4, 1, 4, 4, 4, 4), (3, 0, 4, 4, 4, 4), (3, 1, 17, 4, 4, 4), (3, 1, 4, 1, 4, 4), (3, 1, 16, 1024, 1024, 1024)):
        assert h.dfmir_demons_ws_floats(*bad) == -1, bad
    buf = ctypes.create_string_buffer(4096)
    base = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16                  # aligned host memory: never launched on
    p, q, t = (ctypes.c_void_p(base + 1024 * i) for i in range(3))

    def refused(rc):
        assert rc != 0 and b"invalid argument" in h.dfmir_last_error()

    ok = [2, p, q, None, 4, 1, 8, 8, 1.0, 1.0, 1.0, 3.0, None]
    for i, v in ((0, 4), (1, None), (2, None), (2, p), (4, 0), (6, 1), (7, 1), (10, -1.0), (10, float('nan')), (10, float('inf')),
                 (11, 0.0), (11, float('inf')), (10, 6.0)):
        a = list(ok)
        a[i] = v
        refused(h.dfmir_gauss_smooth(*a))
    refused(h.dfmir_gauss_smooth(3, p, q, None, 1, 4, 4, 4, 1.0, 1.0, 1.0, 3.0, None))       # both passes and no tmp
    refused(h.dfmir_gauss_smooth(3, p, q, p, 1, 4, 4, 4, 1.0, 1.0, 1.0, 3.0, None))
    refused(h.dfmir_gauss_smooth(3, p, q, t, 1, 1, 4, 4, 1.0, 1.0, 1.0, 3.0, None))
    ok = [3, p, p, p, None, p, p, p, q, 2.0, 1, 4, 4, 4, 4, None]
    for i, v in ((0, 1), (1, None), (2, None), (3, None), (5, None), (6, None), (7, None), (8, None), (8, p), (9, 0.0),
                 (9, float('inf')), (9, float('nan')), (10, 0), (11, 0), (11, 17), (12, 1), (14, 1)):
        a = list(ok)
        a[i] = v
        refused(h.dfmir_demons_force(*a))


def test_value_errors_are_raised_before_any_launch():
    from dfmir_amd import infer, ops
    E = pytest.raises(ValueError)
    x = torch.zeros(2, 3, 8, 12)
    assert ops.GAUSS_MAX_RADIUS == 16
    with E: ops.gaussian_smooth(x, -1.0)
    with E: ops.gaussian_smooth(x, float('nan'))
    with E: ops.gaussian_smooth(x, float('inf'))
    with E: ops.gaussian_smooth(x, (1.0,))
    with E: ops.gaussian_smooth(x, (1.0, 1.0, 1.0))
    with E: ops.gaussian_smooth(x, (1.0, -0.5))
    with E: ops.gaussian_smooth(x, "1")
    with E: ops.gaussian_smooth(x, True)
    with E: ops.gaussian_smooth(x, 1.0, truncate=0.0)
    with E: ops.gaussian_smooth(x, 1.0, truncate=float('inf'))
    with E: ops.gaussian_smooth(x, 1.0, truncate=float('nan'))
    with E: ops.gaussian_smooth(x, 6.0)                                   # ceil(18) > 16
    with E: ops.gaussian_smooth(x, (1.0, 4.0), truncate=4.5)
    with E: ops.gaussian_smooth(x.double(), 1.0)
    with E: ops.gaussian_smooth(x[0], 1.0)
    with E: ops.gaussian_smooth(torch.zeros(2, 3, 1, 12), 1.0)
    with E: ops.gaussian_smooth(torch.zeros(2, 0, 8, 12), 1.0)
    with E: ops.gaussian_smooth(x.clone().requires_grad_(), 1.0)
    with E: ops.gaussian_smooth(None, 1.0)
    with pytest.raises(Exception, match="no CPU fallback"): ops.gaussian_smooth(x, 16.0 / 3.0)
    mov, fix, flow = torch.zeros(2, 4, 8, 12), torch.zeros(2, 4, 8, 12), torch.zeros(2, 2, 8, 12)
    for ms in (0.0, -1.0, float('inf'), float('nan'), "2", True):
        with E: ops.demons_force(mov, fix, flow, max_step=ms)
    with E: ops.demons_force(mov, fix, None)
    with E: ops.demons_force(None, fix, flow)
    with E: ops.demons_force(mov, fix, flow.double())
    with E: ops.demons_force(mov, fix, flow[:, :1])
    with E: ops.demons_force(mov, fix[:, :, :4], flow)
    with E: ops.demons_force(torch.zeros(2, 17, 8, 12), torch.zeros(2, 17, 8, 12), flow)
    with E: ops.demons_force(mov, fix.double(), flow)
    with E: ops.demons_force(mov.clone().requires_grad_(), fix, flow)
    with E: ops.demons_force(mov, fix.clone().requires_grad_(), flow)
    with E: ops.demons_force(mov, fix, flow.clone().requires_grad_())
    with E: ops.demons_force(mov, fix, flow, mask=torch.ones(2, 1, 8, 12).requires_grad_())
    with E: ops.demons_force(mov, fix, flow, mask=torch.ones(2, 1, 8, 5))
    with pytest.raises(Exception, match="no CPU fallback"): ops.demons_force(mov, fix, flow)
    im, fx = torch.zeros(2, 1, 8, 12), torch.zeros(2, 1, 8, 12)
    kw = dict(features='intensity')
    with E: infer.demons_flow(im, fx, update='replace', **kw)
    with E: infer.demons_flow(im, fx, diffeomorphic=1, **kw)
    for bad in (-1, 9, 2.0, True):
        with E: infer.demons_flow(im, fx, exp_steps=bad, **kw)
    for name in ("sigma_fluid", "sigma_diffusion"):
        for bad in (-0.5, float('nan'), float('inf'), 5.5, "1"):          # ceil(3 * 5.5) = 17 > 16
            with E: infer.demons_flow(im, fx, **{name: bad}, **kw)
    for bad in (0.0, -2.0, float('inf'), float('nan')):
        with E: infer.demons_flow(im, fx, max_step=bad, **kw)
    with E: infer.demons_flow(im, fx, torch.zeros(2, 2, 8, 11), **kw)
    with E: infer.demons_flow(im, fx, torch.zeros(2, 2, 8, 12).double(), **kw)
    # everything affine_init refuses
    with E: infer.demons_flow(im, fx[:1], **kw)
    with E: infer.demons_flow(im[0], fx[0], **kw)
    with E: infer.demons_flow(im, fx, features='ncc')
    with E: infer.demons_flow(im.repeat(1, 2, 1, 1), fx.repeat(1, 2, 1, 1), **kw)
    with E: infer.demons_flow(im, fx, features=(im, fx[:, :, :4]))
    with E: infer.demons_flow(im, fx, levels=(8,), **kw)                  # 8 // 8 = 1 < 2
    with E: infer.demons_flow(im, fx, levels=(0,), **kw)
    with E: infer.demons_flow(im, fx, levels=(2.0,), **kw)
    with E: infer.demons_flow(im, fx, levels=(), **kw)
    with E: infer.demons_flow(im, fx, levels=(2, 1), iters=(3,), **kw)
    with E: infer.demons_flow(im, fx, iters=-1, **kw)
    with E: infer.demons_flow(im, fx, iters=2.0, **kw)
    with E: infer.demons_flow(im, fx, mask=torch.ones(2, 1, 8, 5), **kw)
    with E: infer.demons_flow(im, fx, mask=1.0, **kw)
    with pytest.raises(Exception, match="no CPU fallback"): infer.demons_flow(im, fx, **kw)


def test_restated_gaussian_keeps_constants_and_handles_zero_sigma_and_short_axes():
    for shape, sigma in GAUSS_CASES[:6]:
        nd = len(shape) - 2
        const = torch.full(shape, 0.75, dtype=torch.float64)
        assert float((gauss_ref(const, sigma) - 0.75).abs().max()) <= 1e-14
        x = gauss_input(shape)
        assert torch.equal(gauss_ref(x, 0.0), x.double())
        assert gauss_ref(x, sigma).shape == x.shape
        sg = _sigmas(sigma, nd)[-1]                                       # the definition itself, on one line along x
        r, w = gauss_weights(sg)
        w = w.float().double()
        line = gauss_ref(x, (0.0,) * (nd - 1) + (sg,))[0, 0].reshape(-1, shape[-1])[0]
        src = x.double()[0, 0].reshape(-1, shape[-1])[0]
        for i in range(shape[-1]):
            ks = [k for k in range(-r, r + 1) if 0 <= i + k < shape[-1]]
            want = sum(w[k + r] * src[i + k] for k in ks) / sum(w[k + r] for k in ks)
            assert abs(float(line[i]) - float(want)) <= 1e-14
    shape, sigma = GAUSS_CASES[3]                                        # r = 12 against extents 3, 7, 9
    assert all(gauss_weights(s)[0] > n for s, n in zip(_sigmas(sigma, 3), shape[2:]))


@pytest.mark.parametrize("shape", FORCE_SHAPES, ids=_id)
def test_restated_force_closed_form_jacobian_bound_and_guards(shape):
    B, Cn = shape[:2]
    vol = tuple(shape[2:])
    for kind in KINDS:
        for mask in ("none", "partial"):
            (M, Fx, phi, m), ref = force_reference(shape, kind, mask)
            d = ref['d']
            assert bool(torch.isfinite(d).all())
            assert float(d.norm(dim=1).max()) <= MAX_STEP / 2 * (1 + 1e-12)
            warped = warp_ref(M.double(), phi.double())
            assert torch.allclose(ref['val'], warped, rtol=1e-11, atol=1e-13)
            L, Lb = TA._reduce(((warped - Fx.double()) ** 2).mean(1, keepdim=True), None if m is None else m.double())
            assert torch.allclose(ref['L'], L, rtol=1e-11, atol=0) and torch.allclose(ref['Lb'], Lb, rtol=1e-11, atol=0)
            if m is not None:
                assert float(d.abs().amax(1)[m[:, 0] <= 0].max()) == 0.0
            if kind == "outside":
                assert float(d.abs().max()) == 0.0
                assert torch.allclose(ref['Lb'], TA._reduce((Fx.double() ** 2).mean(1, keepdim=True), None if m is None else m.double())[1],
                                      rtol=1e-12, atol=0)
            if Cn == 1:                                                   # Thirion's force with Vercauteren's step bound
                e = (ref['val'] - Fx.double())[:, 0]
                J = ref['J'][:, 0]
                want = -e[:, None] * J / ((J ** 2).sum(1) + e ** 2 / MAX_STEP ** 2).clamp_min(1e-300)[:, None]
                if m is not None:
                    want = want * (m > 0).double()
                assert torch.allclose(d, want, rtol=1e-9, atol=1e-14)
    (M, Fx, phi, m), ref = force_reference(shape, "lattice", "none")
    assert face_distance(phi) >= 0.05
    p = phi.double().requires_grad_()
    J = torch.zeros_like(ref['J'])
    warped = warp_ref(M.double(), p)
    for c in range(Cn):
        (gc,) = torch.autograd.grad(warped[:, c].sum(), p, retain_graph=True)
        J[:, c] = gc
    assert torch.allclose(J, ref['J'], rtol=1e-9, atol=1e-12)
    zero = demons_force_ref(M, Fx, phi, torch.zeros(B, 1, *vol))
    assert float(zero['d'].abs().max()) == 0.0 and float(zero['L']) == 0.0


@pytest.mark.parametrize("name", sorted(FIXTURES), ids=str)
def test_restated_loop_reduces_the_energy(name):
    """Levels (2, 1), both sigmas 1, max_step 2, 'compose', intensity features: energy <= 0.25 energy0 in float64."""
    out = loop_reference(name, "compose")
    print("%s: energy0 %.3e -> energy %.3e, ratio %.4f; history %s" % (name, float(out['energy0']), float(out['energy']),
          float(out['energy'] / out['energy0']), ["%.2e" % v for v in out['history'].tolist()]))
    assert tuple(out['history'].shape) == (sum(FIXTURES[name]['iters']),)
    assert float(out['energy']) <= 0.25 * float(out['energy0'])
    mov, fix = fixture(name)
    none = demons_flow_ref(mov, fix, iters=0, **FIXTURE_KW)
    assert float(none['flow'].abs().max()) == 0.0 and float(none['energy']) == float(none['energy0'])


def test_restated_variants_run_and_reduce_the_energy():
    for variant in ("add", "diffeomorphic"):
        out = loop_reference("2d", variant)
        print("2d %s: ratio %.4f" % (variant, float(out['energy'] / out['energy0'])))
        assert float(out['energy']) < float(out['energy0']) and bool(torch.isfinite(out['flow']).all())


# ------------------------------------------------------------------------------------------ GPU tier
def _bounded(errs, what, bound, factor=FACTOR):
    print("%s: " % what + "  ".join("%s %.3e (bound %.1e)" % (k, v, factor * bound[k]) for k, v in errs.items()))
    assert all(v <= factor * bound[k] for k, v in errs.items()), (what, errs)


def _gpu_gauss(x, sigma):
    from dfmir_amd import ops
    y = ops.gaussian_smooth(x.to(DEV), sigma)
    assert y.is_contiguous() and y.dtype == torch.float32 and not y.requires_grad
    return y.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("case", GAUSS_CASES, ids=lambda c: _id(c[0]))
def test_gaussian_smooth_matches_float64_and_is_reproducible(case):
    shape, sigma = case
    x = gauss_input(shape)
    y = _gpu_gauss(x, sigma)
    assert bool(torch.isfinite(y).all())
    _bounded(field_errors(y, gauss_ref(x, sigma)), "gaussian_smooth %s" % _id(shape), FP32_ERR["gauss"][group_of(shape)])
    assert torch.equal(y, _gpu_gauss(x, sigma))
    const = torch.full(shape, 0.75)
    # a constant comes back constant: per axis two sums of at most 2 r + 1 = 33 terms and a division, each within (2 r + 3) u
    assert float((_gpu_gauss(const, sigma) - 0.75).abs().max()) <= (len(shape) - 2) * 35 * 2.0 ** -24
    assert torch.equal(_gpu_gauss(x, 0.0), x)


@pytest.mark.gpu
def test_gaussian_smooth_single_pass_strided_and_misaligned_inputs():
    from dfmir_amd import ops
    shape = (2, 3, 6, 10, 12)
    x = gauss_input(shape)
    bound = FP32_ERR["gauss"]["small"]
    y = _gpu_gauss(x, (1.2, 0.0, 0.0))                                   # the z pass alone
    _bounded(field_errors(y, gauss_ref(x, (1.2, 0.0, 0.0))), "z alone", bound)
    full = _gpu_gauss(x, 1.2)
    _bounded(field_errors(full, gauss_ref(x, 1.2)), "contiguous", bound)
    strided = x.to(DEV).permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
    assert not strided.is_contiguous()
    assert torch.equal(ops.gaussian_smooth(strided, 1.2).cpu(), full)
    base = torch.empty(x.numel() + 1, device=DEV)
    off = base[1:].view(shape).copy_(x.to(DEV))
    assert off.data_ptr() % 16 == 4
    got = ops.gaussian_smooth(off, 1.2).cpu()
    _bounded(field_errors(got, gauss_ref(x, 1.2)), "misaligned", bound)
    zero_sig = torch.tensor([0.0, -0.0, float('inf'), -1.5], device=DEV).repeat(2, 1, 2, 1)      # sigma 0 copies the bits
    assert torch.equal(ops.gaussian_smooth(zero_sig, 0.0).view(torch.int32), zero_sig.view(torch.int32))


def _gpu_force(M, Fx, phi, m, form):
    from dfmir_amd import ops
    mov = ops.pack_features(M.to(DEV)) if form == "packed" else M.to(DEV)
    md = None if m is None else m.to(DEV)
    d, L, Lb = ops.demons_force(mov, Fx.to(DEV), phi.to(DEV), md, MAX_STEP)
    Lw = ops.warp_ssd(mov, Fx.to(DEV), phi.to(DEV), md)
    torch.cuda.synchronize()
    assert d.dtype == L.dtype == Lb.dtype == torch.float32 and not d.requires_grad and tuple(d.shape) == tuple(phi.shape)
    return dict(d=d.cpu(), L=L.cpu(), Lb=Lb.cpu()), Lw.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", FORCE_SHAPES, ids=_id)
def test_demons_force_matches_float64_warp_ssd_and_is_reproducible(shape, kind):
    bound = FP32_ERR["force"]["small"]
    for mask in MASKS:
        (M, Fx, phi, m), ref = force_reference(shape, kind, mask)
        if kind == "lattice":
            assert face_distance(phi) >= 0.05
        what = "%s %s %s" % (_id(shape), kind, mask)
        got, Lw = _gpu_force(M, Fx, phi, m, "packed")
        for v in got.values():
            assert bool(torch.isfinite(v).all()), what
        _bounded(force_errors(got, ref), "demons_force " + what, bound)
        _bounded(dict(L=TA._rel(got['L'].reshape(1), Lw.reshape(1))), "L against warp_ssd " + what, bound, factor=2.0 * FACTOR)
        assert float(got['d'].norm(dim=1).max()) <= MAX_STEP / 2 * (1 + 1e-5)
        for form in ("packed", "plain"):
            again, _ = _gpu_force(M, Fx, phi, m, form)
            assert all(torch.equal(got[k], again[k]) for k in got), (what, form)
        if kind == "outside" or mask == "zero":
            assert float(got['d'].abs().max()) == 0.0 and not bool(torch.signbit(got['d']).any())
        if mask == "zero":
            assert float(got['L']) == 0.0 and float(got['Lb'].abs().max()) == 0.0
        elif kind == "outside":
            want = TA._reduce((Fx.double() ** 2).mean(1, keepdim=True), None if m is None else m.double())[1]
            assert TA._rel(got['Lb'], want) <= FACTOR * bound["Lb"]
        if m is not None:
            assert float(got['d'].abs().amax(1)[m[:, 0] <= 0].max()) == 0.0


def _gpu_loop(name, variant, **extra):
    from dfmir_amd import infer
    mov, fix = fixture(name)
    kw = {**FIXTURE_KW, **VARIANTS[variant], **extra}
    kw.setdefault("iters", FIXTURES[name]['iters'])
    return infer.demons_flow(mov.to(DEV), fix.to(DEV), features='intensity', **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name,variant", [("2d", "compose"), ("3d", "compose"), ("2d", "add"), ("2d", "diffeomorphic")])
def test_demons_flow_matches_the_float64_loop(name, variant):
    from dfmir_amd import ops
    ref = loop_reference(name, variant)
    out = _gpu_loop(name, variant)
    n = sum(FIXTURES[name]['iters'])
    assert tuple(out['history'].shape) == (n,) and out['history'].dtype == torch.float32
    assert out['energy0'].dim() == 0 and out['energy'].dim() == 0 and not out['flow'].requires_grad
    e0, e1 = float(out['energy0']), float(out['energy'])
    print("%s %s: energy0 %.3e -> %.3e, ratio %.4f (float64 loop %.4f)" % (name, variant, e0, e1, e1 / e0,
                                                                         float(ref['energy'] / ref['energy0'])))
    if variant == "compose":
        assert e1 <= 0.25 * e0
    _bounded(loop_errors(out, ref), "demons_flow %s %s" % (name, variant), LOOP_FP32_GAP[(name, variant)])
    mov, fix = fixture(name)
    assert torch.equal(out['warped'], ops.warp(mov.to(DEV), out['flow']))
    assert torch.equal(out['energy'], ops.warp_ssd(mov.to(DEV), fix.to(DEV), out['flow']))
    again = _gpu_loop(name, variant)
    for k in ("flow", "warped", "history", "energy0", "energy"):
        assert torch.equal(out[k], again[k]), k


@pytest.mark.gpu
def test_demons_flow_iters_zero_default_start_mask_and_mind():
    from dfmir_amd import infer
    mov, fix = (t.to(DEV) for t in fixture("2d"))
    vol = FIXTURES["2d"]['vol']
    start = (C.rand(5, 1, 2, *vol) - 0.5).to(DEV)
    kw = dict(features='intensity', levels=(2, 1))
    out = infer.demons_flow(mov, fix, start, iters=0, **kw)
    assert torch.equal(out['flow'], start) and tuple(out['history'].shape) == (0,) and torch.equal(out['energy'], out['energy0'])
    out = infer.demons_flow(mov, fix, iters=(0, 0), **kw)
    assert float(out['flow'].abs().max()) == 0.0 and not bool(torch.signbit(out['flow']).any())
    a = infer.demons_flow(mov, fix, iters=2, **kw)
    b = infer.demons_flow(mov, fix, torch.zeros(1, 2, *vol, device=DEV), iters=2, **kw)
    assert torch.equal(a['flow'], b['flow']) and torch.equal(a['history'], b['history'])
    ones = infer.demons_flow(mov, fix, iters=2, mask=torch.ones(1, 1, *vol, device=DEV), **kw)      # the mask's pooling: ones stay ones
    assert torch.equal(ones['flow'], a['flow']) and torch.equal(ones['history'], a['history'])
    none = infer.demons_flow(mov, fix, start, iters=2, mask=torch.zeros(1, 1, *vol, device=DEV), sigma_diffusion=0.0, **kw)
    assert float(none['history'].abs().max()) == 0.0 and float(none['energy']) == 0.0
    out = infer.demons_flow(mov, fix, levels=(2,), iters=2)               # the MIND default, pooled, then back to the volume
    assert bool(torch.isfinite(out['flow']).all()) and tuple(out['flow'].shape) == (1, 2) + vol
