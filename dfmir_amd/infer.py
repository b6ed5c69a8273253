"""Inference path (reference test.py:37-90): translate B, register A onto B, and
warp a label map with nearest-neighbour sampling -- all on the HIP device (the reference moves the label
warp to the CPU, test.py:80-81)."""
import torch

from . import ops
from .losses import BendingEnergy_Loss, Grad_Loss, JacobianDet_Loss
from .voxelmorph import SpatialTransformer


def _check_features(what, features, moving, nd, B, vol):
    """The `features` argument of refine_flow / convex_init: 'mind', 'intensity' or a pair of [B,C,*vol] tensors."""
    if isinstance(features, str):
        if features not in ('mind', 'intensity'):
            raise ValueError("%s: features must be 'mind', 'intensity' or a pair of tensors, got %r" % (what, features))
        if moving.shape[1] != 1:
            raise ValueError("%s: features=%r needs single-channel images, got %d channels" % (what, features, moving.shape[1]))
    else:
        try:
            Mm, Mf = features
        except (TypeError, ValueError):
            raise ValueError("%s: features must be 'mind', 'intensity' or a pair of [B,C,*vol] tensors" % what)
        for t in (Mm, Mf):
            if not torch.is_tensor(t) or t.dim() != nd + 2 or (int(t.shape[0]),) + tuple(t.shape[2:]) != (B,) + vol:
                raise ValueError("%s: the feature tensors must be [B,C,*vol] over the images' volume %s" % (what, vol))


def _resolve_features(features, moving, fixed, mind_radius, mind_dilation):
    """(moving features, fixed features) of a checked `features` argument, detached."""
    if isinstance(features, str) and features == 'mind':
        return (ops.mind_descriptor(moving, mind_radius, mind_dilation), ops.mind_descriptor(fixed, mind_radius, mind_dilation))
    if isinstance(features, str):
        return moving.detach(), fixed.detach()
    Mm, Mf = features
    return Mm.detach(), Mf.detach()


INTERPS = ('linear', 'cubic')


def _check_interp(what, interp):
    if not isinstance(interp, str) or interp not in INTERPS:
        raise ValueError("%s: interp must be 'linear' or 'cubic', got %r" % (what, interp))


def _final_warp(moving, flow, interp):
    """The `warped` a solver returns: ops.warp (bi-/trilinear, zero padding) or ops.warp_cubic (cubic B-spline, mirror)."""
    return ops.warp_cubic(moving, flow) if interp == 'cubic' else ops.warp(moving, flow)


@torch.no_grad()
def resample(moving, flow, interp='cubic'):
    """The moving image through a flow that a solver found, in one call: interp 'cubic' = ops.warp_cubic(moving, flow) --
    third-order B-spline interpolation with mirror extension, which may overshoot the range of `moving` at edges -- or
    'linear' = ops.warp(moving, flow), bi-/trilinear with zero padding.  moving [B,C,*vol] fp32, flow [B,nd,*vol] in voxels;
    no gradient is recorded.  ValueError on any other interp and on what the op refuses."""
    _check_interp("resample", interp)
    if not torch.is_tensor(moving) or not torch.is_tensor(flow):
        raise ValueError("resample: moving and flow must be tensors")
    return _final_warp(moving.detach(), flow.detach(), interp)


def refine_flow(moving, fixed, flow=None, *, features='mind', mind_radius=2, mind_dilation=2, mask=None,
                regularizer='diffusion', lam, spacing=None, grid_downsize=2, iters=50, lr, betas=(0.9, 0.999),
                update='add', parametrisation='linear', fold_weight=0.0, fold_eps=0.0, fold_power=2, interp='linear'):
    """Instance optimisation: `iters` Adam iterations on the displacement field of ONE pair (build-defined), the step
    between a network's flow and the reported number.  Returns dict(flow, warped, history).

    moving, fixed: [B,1,*vol] fp32 images, 2-D or 3-D; flow: the starting field [B,nd,*vol] in voxels (ops.warp's
    convention), None = zeros.  features: 'mind' = ops.mind_descriptor(., mind_radius, mind_dilation) of both images (12
    channels in 3-D, 4 in 2-D), 'intensity' = the images themselves, or a pair (moving features, fixed features) of
    [B,C,*vol] tensors, 1 <= C <= 16.  The unknown is a residual delta [B,nd,*(vol // grid_downsize)], zero at the start:

        flow_k = flow + ops.resize_linear(delta_k, vol)                     (iteration 0 evaluates `flow` itself)
        J_k    = ops.warp_ssd(Mm, Mf, flow_k, mask) + lam * R(flow_k)        R = Grad_Loss('l2') ('diffusion') or
                                                                             BendingEnergy_Loss(spacing) ('bending')
        delta_{k+1} = Adam(lr, betas, eps 1e-8)(delta_k, dJ_k / d delta)     (ops.adam_step)

    The moving features are packed once (ops.pack_features).  history: a device tensor [iters + 1, 2] of (similarity,
    regulariser) at flow_0 .. flow_iters; the returned flow is flow_iters (with iters = 0: `flow` bit for bit) and warped =
    ops.warp(moving, flow).  Nothing in the loop syncs with the host.  ValueError on an unknown option, on shapes that
    disagree and on a coarse dimension < 2.

    update: how the correction meets the starting flow.  'add' (the default) is the sum above.  'compose' combines the two as
    deformations do: flow_k = ops.compose_flows(ops.resize_linear(delta_k, vol), flow) = up + flow(x + up(x)) -- the correction
    is applied in the fixed image's frame and then the starting flow, so warp(moving, flow_k) = warp(warp(moving, flow), up).
    With flow=None the two are the same computation (bit-identical results); iteration 0 evaluates `flow` itself either way
    (compose_flows(0, flow) is flow bit for bit).  ValueError on any other value.

    parametrisation: what `delta` is.  'linear' (the default) is the coarse grid above, interpolated linearly.  'bspline' makes
    it the control grid of a cubic B-spline free-form deformation: grid_downsize is then the control spacing in voxels, an
    int or nd ints in [1, ops.BSPLINE_MAX_STRIDE]; delta is [B,nd,*ops.bspline_control_shape(vol, grid_downsize)], zero at
    the start; ops.bspline_flow(delta_k, vol, grid_downsize) stands where ops.resize_linear(delta_k, vol) does above, under
    both values of `update` (a zero grid expands to +0.0, so iteration 0 still evaluates `flow` itself); there is no lower
    limit on the volume (one smaller than a control cell is legal); and the returned dict gains 'control', the final delta.
    Everything else is the same loop.  ValueError on any other value.

    fold_weight: a weight >= 0 on the fold penalty (build-defined: losses.JacobianDet_Loss).  0.0 (the default) launches
    nothing more and the result is bit-identical to a call without the keyword.  With fold_weight > 0, J_k gains
    fold_weight * ops.jacobian_penalty(flow_k, fold_eps, fold_power) and the returned dict gains 'fold_history', a device
    tensor [iters + 1] of that penalty (unweighted) at flow_0 .. flow_iters; `history` keeps its two columns.  ValueError on
    a negative or non-finite weight and on a fold_eps / fold_power that ops.jacobian_penalty refuses.

    interp: how the returned `warped` is sampled, and nothing else: 'linear' (the default) = ops.warp(moving, flow), 'cubic'
    = ops.warp_cubic(moving, flow) (mirror extension, may overshoot).  The loop's SSD kernel samples linearly either way, so
    flow and history do not depend on it.  ValueError on any other value."""
    what = "refine_flow"
    _check_interp(what, interp)
    if isinstance(fold_weight, bool) or not isinstance(fold_weight, (int, float)) or not 0.0 <= fold_weight < float('inf'):
        raise ValueError("%s: fold_weight must be a finite weight >= 0, got %r" % (what, fold_weight))
    fold = float(fold_weight) > 0.0
    if update not in ('add', 'compose'):
        raise ValueError("%s: update must be 'add' or 'compose', got %r" % (what, update))
    if parametrisation not in ('linear', 'bspline'):
        raise ValueError("%s: parametrisation must be 'linear' or 'bspline', got %r" % (what, parametrisation))
    if not (torch.is_tensor(moving) and torch.is_tensor(fixed)) or moving.dim() not in (4, 5) \
            or tuple(moving.shape) != tuple(fixed.shape):
        raise ValueError("%s: moving and fixed must be two [B,1,*vol] tensors of one shape" % what)
    nd = moving.dim() - 2
    B, vol = int(moving.shape[0]), tuple(int(n) for n in moving.shape[2:])
    if parametrisation == 'bspline':
        try:
            coarse = ops.bspline_control_shape(vol, grid_downsize)
        except ValueError:
            raise ValueError("%s: with parametrisation='bspline' grid_downsize must be an integer in [1, %d] or %d of them, "
                             "got %r" % (what, ops.BSPLINE_MAX_STRIDE, nd, grid_downsize)) from None
    else:
        if isinstance(grid_downsize, bool) or not isinstance(grid_downsize, int) or grid_downsize < 1:
            raise ValueError("%s: grid_downsize must be an integer >= 1, got %r" % (what, grid_downsize))
        coarse = tuple(n // grid_downsize for n in vol)
        if min(coarse) < 2:
            raise ValueError("%s: every dimension of the coarse grid %s = %s // %d must be >= 2"
                             % (what, coarse, vol, grid_downsize))
    if isinstance(iters, bool) or not isinstance(iters, int) or iters < 0:
        raise ValueError("%s: iters must be an integer >= 0, got %r" % (what, iters))
    if regularizer not in ('diffusion', 'bending'):
        raise ValueError("%s: regularizer must be 'diffusion' or 'bending', got %r" % (what, regularizer))
    if flow is not None and (not torch.is_tensor(flow) or tuple(flow.shape) != (B, nd) + vol):
        raise ValueError("%s: flow must be [B,%d,*vol] = %s" % (what, nd, (B, nd) + vol))
    _check_features(what, features, moving, nd, B, vol)
    reg = Grad_Loss(dim=nd, penalty='l2') if regularizer == 'diffusion' else BendingEnergy_Loss(dim=nd, spacing=spacing)
    if fold:
        if min(vol) < 3:
            raise ValueError("%s: fold_weight > 0 needs a volume of at least 3 voxels per axis, got %s" % (what, vol))
        jd = JacobianDet_Loss(dim=nd, eps=fold_eps, power=fold_power)      # (a bad fold_eps / fold_power raises here)
    with torch.no_grad():
        Mm, Mf = _resolve_features(features, moving, fixed, mind_radius, mind_dilation)
        handle = ops.pack_features(Mm)
        flow0 = None if flow is None else flow.detach()
        delta = ops.zeros((B, nd) + coarse, handle.packed.device)
        m, v = ops.zeros_like(delta), ops.zeros_like(delta)
        history = torch.empty((iters + 1, 2), device=delta.device, dtype=torch.float32)
        fold_history = torch.empty((iters + 1,), device=delta.device, dtype=torch.float32) if fold else None

    def flow_of(d):
        up = ops.bspline_flow(d, vol, grid_downsize) if parametrisation == 'bspline' else ops.resize_linear(d, vol)
        if flow0 is None:
            return up
        return ops.compose_flows(up, flow0) if update == 'compose' else flow0 + up

    for k in range(iters):
        d = delta.detach().requires_grad_(True)
        with torch.enable_grad():
            flow_k = flow_of(d)
            sim = ops.warp_ssd(handle, Mf, flow_k, mask)
            r = reg(flow_k)
            total = sim + r * float(lam)
            if fold:
                f = jd(flow_k)
                total = total + f * float(fold_weight)
            (g,) = torch.autograd.grad(total, d)
        with torch.no_grad():
            history[k, 0], history[k, 1] = sim.detach(), r.detach()
            if fold:
                fold_history[k] = f.detach()
            ops.adam_step(delta, g, m, v, lr, betas[0], betas[1], 1e-8, k + 1, bump=False)
    with torch.no_grad():
        if iters == 0:
            out = ops.zeros((B, nd) + vol, delta.device) if flow0 is None else flow0.clone()
        else:
            out = flow_of(delta)
        history[iters, 0] = ops.warp_ssd(handle, Mf, out, mask)
        history[iters, 1] = reg(out)
        if fold:
            fold_history[iters] = jd(out)
        warped = _final_warp(moving, out, interp)
    res = dict(flow=out, warped=warped, history=history)
    if fold:
        res['fold_history'] = fold_history
    if parametrisation == 'bspline':
        res['control'] = delta
    return res


CONVEX_COEFFS = (0.003, 0.01, 0.03, 0.1, 0.3, 1.0)


@torch.no_grad()
def convex_init(moving, fixed, *, features='mind', mind_radius=2, mind_dilation=2, grid_sp=4, disp_hw=3,
                coeffs=CONVEX_COEFFS):
    """Discrete displacement search with coupled-convex regularisation (build-defined), the first stage of the two-stage
    scheme whose second stage is refine_flow: it has no gradient to get stuck on, so it captures displacements of up to
    grid_sp * disp_hw voxels that a local descent started from zero cannot.  Returns dict(flow, coarse, idx).

    moving, fixed: [B,1,*vol] fp32 images, 2-D or 3-D; features as in refine_flow: 'mind' = ops.mind_descriptor(.,
    mind_radius, mind_dilation) of both images, 'intensity' = the images themselves, or a pair (moving features, fixed
    features) of [B,C,*vol] tensors, 1 <= C <= 16.  grid_sp: an integer >= 1, the stride of the search grid; disp_hw: the
    half width of the search window in coarse voxels, an integer in 1..ops.DSEARCH_MAX_RADIUS[nd] (8 in 2-D, 4 in 3-D);
    coeffs: the coupling coefficients, finite floats >= 0, in the order they are applied.

        mov_p, fix_p = ops.pool_features(., grid_sp)                        both sides, [B,C,*(vol // grid_sp)]
        cost   = ops.ssd_cost_volume(fix_p, mov_p, disp_hw)                 [B,(2 disp_hw + 1)^nd,*(vol // grid_sp)]
        soft_0 = ops.box_smooth_flow(ops.cost_argmin(cost, disp_hw)[1])
        soft   <- ops.box_smooth_flow(ops.cost_argmin(cost, disp_hw, soft, coeff)[1])        for each coeff in coeffs
        coarse = the last soft, in COARSE voxels;  idx = the index field of the last argmin, int32 [B,*(vol // grid_sp)]
        flow   = ops.resize_linear(coarse, vol, mult=grid_sp)               fine voxels, ops.warp's convention

    so `flow` is ready for refine_flow(moving, fixed, flow, ..., update='compose').  Nothing here syncs with the host, and
    every output is bit-identical from run to run.

    Where the field lands: the stride-g pooling puts coarse sample i at fine coordinate g i + (g - 1) / 2, while
    ops.resize_linear aligns corners, so the field lands up to (g - 1) / 2 voxels from where it was estimated -- the same
    approximation refine_flow makes for its coarse `delta`.  The box mean divides by the in-volume count
    (ops.box_smooth_flow), where the published code divides by 3^nd.

    The default `coeffs` are the numbers of the published coupled-convex schedule.  The cost here is a channel MEAN and the
    displacements are in coarse voxels, so their scale is not the published one, and nobody has measured registration
    quality with them.

    ValueError before any launch on images that are not two [B,1,*vol] tensors of one shape (any channel count with a
    feature pair), an unknown `features`, a grid_sp that is not an integer >= 1 or leaves a coarse extent < 2, a disp_hw
    outside its range and a coefficient that is negative or not finite."""
    what = "convex_init"
    if not (torch.is_tensor(moving) and torch.is_tensor(fixed)) or moving.dim() not in (4, 5) \
            or tuple(moving.shape) != tuple(fixed.shape):
        raise ValueError("%s: moving and fixed must be two [B,1,*vol] tensors of one shape" % what)
    nd = moving.dim() - 2
    B, vol = int(moving.shape[0]), tuple(int(n) for n in moving.shape[2:])
    if isinstance(grid_sp, bool) or not isinstance(grid_sp, int) or grid_sp < 1:
        raise ValueError("%s: grid_sp must be an integer >= 1, got %r" % (what, grid_sp))
    if min(n // grid_sp for n in vol) < 2:
        raise ValueError("%s: every dimension of the search grid %s // %d must be >= 2" % (what, vol, grid_sp))
    if isinstance(disp_hw, bool) or not isinstance(disp_hw, int) or not 1 <= disp_hw <= ops.DSEARCH_MAX_RADIUS[nd]:
        raise ValueError("%s: disp_hw must be an integer in [1, %d] in %d-D, got %r"
                         % (what, ops.DSEARCH_MAX_RADIUS[nd], nd, disp_hw))
    try:
        coeffs = tuple(float(c) for c in coeffs)
    except (TypeError, ValueError):
        raise ValueError("%s: coeffs must be a sequence of finite numbers >= 0, got %r" % (what, coeffs))
    if not all(0.0 <= c < float('inf') for c in coeffs):
        raise ValueError("%s: coeffs must be a sequence of finite numbers >= 0, got %r" % (what, coeffs))
    _check_features(what, features, moving, nd, B, vol)
    Mm, Mf = _resolve_features(features, moving, fixed, mind_radius, mind_dilation)
    mov_p, fix_p = ops.pool_features(Mm, grid_sp), ops.pool_features(Mf, grid_sp)
    cost = ops.ssd_cost_volume(fix_p, mov_p, disp_hw)
    idx, disp = ops.cost_argmin(cost, disp_hw)
    soft = ops.box_smooth_flow(disp)
    for c in coeffs:
        idx, disp = ops.cost_argmin(cost, disp_hw, soft, c)
        soft = ops.box_smooth_flow(disp)
    return dict(flow=ops.resize_linear(soft, vol, mult=float(grid_sp)), coarse=soft, idx=idx)


def _finite_number(x):
    return not isinstance(x, bool) and isinstance(x, (int, float)) and float('-inf') < x < float('inf')


@torch.no_grad()
def affine_init(moving, fixed, *, features='mind', mind_radius=2, mind_dilation=2, mask=None, theta=None, dof='affine',
                levels=(4, 2, 1), iters=10, mu0=1e-3, mu_up=10.0, mu_down=0.1, interp='linear'):
    """Affine pre-alignment (build-defined): a multi-level Levenberg-Marquardt fit of one affine transform per sample to the
    SSD of features, the global stage in front of convex_init and refine_flow, which only look as far as a search window or
    a descent from the start reaches.  Returns dict(theta, flow, warped, history).

    moving, fixed: [B,1,*vol] fp32 images, 2-D or 3-D; features as in refine_flow: 'mind' = ops.mind_descriptor(.,
    mind_radius, mind_dilation) of both images, 'intensity' = the images themselves, or a pair (moving features, fixed
    features) of [B,C,*vol] tensors, 1 <= C <= 16.  mask: float weights that broadcast to [B,1,*vol], or None.  theta: the
    start, [B,nd,nd+1] fp32 in ops.affine_flow's convention ([A | t], centred voxel coordinates), None = identity.  dof:
    'affine' (all P = nd (nd + 1) parameters are free) or 'translation' (only the t column; A keeps its starting value bit for
    bit).  levels: pooling strides, integers >= 1, applied in order; iters: evaluations per level, an int or one per level.

    A level of stride s works on ops.pool_features(., s) of both feature sets (and of the mask, as a 1-channel feature; s = 1
    takes them as they are), the moving side packed once.  Its theta is [A | t / s] and its result goes back as [A | s t]; the
    centres are the level's own (n_l - 1) / 2.  When s does not divide an extent the pooled grid's centre sits (n mod s) / 2
    fine voxels from the fine centre: an approximation the later levels absorb.  The loop of one level, per sample and all on
    the device (ops.affine_ssd_system, ops.affine_lm_step), starts from theta_acc = trial = the level's start, L_acc = +inf,
    mu = mu0 (both reset at each level: the similarity changes):

        for k in 0 .. iters - 1:
            (L, g, H) = ops.affine_ssd_system at trial
            L finite and L <= L_acc:  accept -- theta_acc = trial, L_acc = L, (g_acc, H_acc) = (g, H); k > 0: mu = max(mu mu_down, 1e-12)
            otherwise:                reject -- mu = min(mu mu_up, 1e12)
            solve (H_acc[f,f] + mu diag(H_acc[f,f])) d = -g_acc[f] over the free parameters f, Cholesky in fp64;
                  a pivot <= 0 or not finite: d = 0 and the row's 'singular' flag is set
            trial = theta_acc + d
            history[row + k, b] = (L, L_acc, mu, accepted, singular)
        the level's result: theta_acc

    history: a float64 device tensor [sum iters, B, 5].  flow = ops.affine_flow(theta, vol) and warped = ops.warp(moving,
    flow); with iters = 0 everywhere theta is the start bit for bit.  Nothing syncs with the host.  The staged pipeline this
    opens: aff = affine_init(mov, fix); cv = convex_init(aff['warped'], fix); flow0 = ops.compose_flows(cv['flow'],
    aff['flow']); refine_flow(mov, fix, flow0, update='compose', ...).

    ValueError before any launch on images that are not two [B,1,*vol] tensors of one shape (any channel count with a feature
    pair), an unknown `features` or `dof`, a theta of the wrong shape or dtype, levels that are not integers >= 1 or leave an
    extent < 2, iters that are not integers >= 0 or disagree with levels in length, and mu0 <= 0, mu_up <= 1 or mu_down outside
    (0, 1] (or any of them not finite), and an interp other than 'linear' or 'cubic'.

    interp: how the returned `warped` is sampled, and nothing else: 'linear' (the default) = ops.warp(moving, flow), 'cubic'
    = ops.warp_cubic(moving, flow) (mirror extension, may overshoot); theta, flow and history do not depend on it."""
    what = "affine_init"
    _check_interp(what, interp)
    if not (torch.is_tensor(moving) and torch.is_tensor(fixed)) or moving.dim() not in (4, 5) \
            or tuple(moving.shape) != tuple(fixed.shape):
        raise ValueError("%s: moving and fixed must be two [B,1,*vol] tensors of one shape" % what)
    nd = moving.dim() - 2
    B, vol = int(moving.shape[0]), tuple(int(n) for n in moving.shape[2:])
    if dof not in ('affine', 'translation'):
        raise ValueError("%s: dof must be 'affine' or 'translation', got %r" % (what, dof))
    try:
        levels = tuple(levels)
    except TypeError:
        raise ValueError("%s: levels must be a sequence of integers >= 1, got %r" % (what, levels)) from None
    if not levels or any(isinstance(s, bool) or not isinstance(s, int) or s < 1 for s in levels):
        raise ValueError("%s: levels must be a non-empty sequence of integers >= 1, got %r" % (what, levels))
    for s in levels:
        if min(n // s for n in vol) < 2:
            raise ValueError("%s: every extent of a level must be >= 2, got %s // %d" % (what, vol, s))
    if isinstance(iters, int) and not isinstance(iters, bool):
        iters = (iters,) * len(levels)
    try:
        iters = tuple(iters)
    except TypeError:
        raise ValueError("%s: iters must be an integer >= 0 or one per level, got %r" % (what, iters)) from None
    if len(iters) != len(levels) or any(isinstance(n, bool) or not isinstance(n, int) or n < 0 for n in iters):
        raise ValueError("%s: iters must be an integer >= 0 or one per level (%d), got %r" % (what, len(levels), iters))
    if not (_finite_number(mu0) and _finite_number(mu_up) and _finite_number(mu_down)) \
            or not (mu0 > 0 and mu_up > 1 and 0 < mu_down <= 1):
        raise ValueError("%s: mu0 must be > 0, mu_up > 1 and mu_down in (0, 1], all finite; got %r, %r, %r"
                         % (what, mu0, mu_up, mu_down))
    if theta is not None:
        if not torch.is_tensor(theta) or tuple(theta.shape) != (B, nd, nd + 1) or theta.dtype != torch.float32:
            raise ValueError("%s: theta must be an fp32 tensor [B,%d,%d] = %s" % (what, nd, nd + 1, (B, nd, nd + 1)))
    _check_features(what, features, moving, nd, B, vol)
    if mask is not None:
        if not torch.is_tensor(mask):
            raise ValueError("%s: mask must be a tensor" % what)
        try:
            mask = mask.expand((B, 1) + vol)
        except RuntimeError:
            raise ValueError("%s: mask %s does not broadcast to %s" % (what, tuple(mask.shape), (B, 1) + vol)) from None
    Mm, Mf = _resolve_features(features, moving, fixed, mind_radius, mind_dilation)
    dev = Mm.device
    if mask is not None:
        mask = mask.detach().to(device=dev, dtype=torch.float32).contiguous()
    th = ops.affine_identity(B, nd, dev) if theta is None else theta.detach().to(dev).clone(memory_format=torch.contiguous_format)
    P = nd * (nd + 1)
    history = torch.empty((sum(iters), B, 5), device=dev, dtype=torch.float64)
    row = 0
    for s, n in zip(levels, iters):
        if n == 0:
            continue
        if s == 1:
            Lm, Lf, Lk = Mm, Mf, mask
        else:
            Lm, Lf = ops.pool_features(Mm, s), ops.pool_features(Mf, s)
            Lk = None if mask is None else ops.pool_features(mask, s)
        geom, h, Lf, _, Lk = ops._affine_ssd_args(Lm, Lf, th, Lk, what)
        acc = th.clone()
        acc[:, :, nd] /= float(s)
        trial = acc.clone()
        state = ops.affine_lm_state(B, nd, mu0, dev)
        for k in range(n):
            out = ops._affine_system_launch(geom, h, Lf, trial, Lk, True)
            o = 1 + B + B * P
            ops.affine_lm_step(out[1:1 + B], out[o:o + B * P].view(B, P), out[o + B * P:].view(B, P, P), acc, trial, state,
                               history[row + k], k, dof, mu_up, mu_down)
        row += n
        th = acc
        th[:, :, nd] *= float(s)
    flow = ops.affine_flow(th, vol)
    return dict(theta=th, flow=flow, warped=_final_warp(moving, flow, interp), history=history)


@torch.no_grad()
def demons_flow(moving, fixed, flow=None, *, features='mind', mind_radius=2, mind_dilation=2, mask=None,
                levels=(4, 2, 1), iters=10, max_step=2.0, sigma_fluid=1.0, sigma_diffusion=1.0,
                update='compose', diffeomorphic=False, exp_steps=4, interp='linear'):
    """The demons iteration (build-defined): a second-order dense solver on the feature SSD, coarse to fine -- a per-voxel
    Gauss-Newton step (ops.demons_force) regularised by Gaussian smoothing of the update (fluid) and of the field
    (diffusion), with no backward pass, no optimiser state and no learning rate.  Returns dict(flow, warped, history, energy0,
    energy).

    moving, fixed: [B,1,*vol] fp32 images, 2-D or 3-D; flow: the starting field [B,nd,*vol] in voxels (ops.warp's
    convention), None = zeros.  features as in refine_flow: 'mind' = ops.mind_descriptor(., mind_radius, mind_dilation) of
    both images, 'intensity' = the images themselves, or a pair (moving features, fixed features) of [B,C,*vol] tensors,
    1 <= C <= 16.  mask: float weights that broadcast to [B,1,*vol], or None.  levels: pooling strides, integers >= 1, applied
    in order; iters: iterations per level, an int or one per level (a level with 0 iterations is skipped).

    A level of stride s works on ops.pool_features(., s) of both feature sets (and of the mask, as a 1-channel feature; s = 1
    takes them as they are), the moving side packed once.  Its field is u = ops.resize_linear(previous, vol // s,
    mult=s_prev / s) -- the first level starts from `flow` with s_prev = 1; a field that already has the level's shape and
    stride is taken as it is -- and each iteration is

        d, L, _ = ops.demons_force(h, Lf, u, Lk, max_step)        history[row] = L   (the energy at the u the force saw)
        d = ops.gaussian_smooth(d, sigma_fluid)                    skipped when sigma_fluid == 0
        diffeomorphic:  d = d * 2^-exp_steps, then exp_steps times d = ops.vecint_step(d)      (d <- exp(d))
        u = ops.compose_flows(d, u)     'compose': u <- d + u(x + d), the correction applied in the fixed image's frame
            or u + d                    'add'
        u = ops.gaussian_smooth(u, sigma_diffusion)                skipped when sigma_diffusion == 0

    The sigmas and max_step are in the level's own voxels.  After the last level the field goes to `vol` with
    ops.resize_linear(u, vol, mult=s_last), skipped when s_last == 1.  history: a device tensor [sum iters]; energy0 and
    energy: ops.warp_ssd on the full-resolution features (and the mask) at the input flow and at the result, as device
    scalars; warped = ops.warp(moving, flow).  With iters = 0 everywhere `flow` is the input bit for bit (or zeros).  Nothing
    syncs with the host and nothing records a gradient.

    Where the field lands: when s does not divide an extent the pooled grid's centre sits (n mod s) / 2 fine voxels from the
    fine centre, and the stride-s pooling puts coarse sample i at fine coordinate s i + (s - 1) / 2 while ops.resize_linear
    aligns corners: an approximation the later levels absorb (affine_init's and convex_init's).

    Where the stage sits: after affine_init and convex_init, composed as refine_flow's docstring shows -- aff =
    affine_init(mov, fix); cv = convex_init(aff['warped'], fix); flow0 = ops.compose_flows(cv['flow'], aff['flow']);
    demons_flow(mov, fix, flow0) -- or on a network's flow with levels=(1,).

    Out of scope: symmetric (ESM) forces that average in the gradient of the fixed features, a gradient of
    ops.gaussian_smooth, and the wiring into register_volume / register_pair_refined.

    ValueError before any launch on everything affine_init refuses for its images, features, mask, levels and iters, a flow
    that is not [B,nd,*vol] fp32, an unknown `update`, a `diffeomorphic` that is not a bool, an exp_steps that is not an
    integer in 0..8, a max_step that is not finite and > 0, a sigma that is negative or not finite and a sigma whose radius
    ceil(3 sigma) exceeds ops.GAUSS_MAX_RADIUS, and an interp other than 'linear' or 'cubic'.

    interp: how the returned `warped` is sampled, and nothing else: 'linear' (the default) = ops.warp(moving, flow), 'cubic'
    = ops.warp_cubic(moving, flow) (mirror extension, may overshoot); flow, history and the energies do not depend on it."""
    what = "demons_flow"
    _check_interp(what, interp)
    if not (torch.is_tensor(moving) and torch.is_tensor(fixed)) or moving.dim() not in (4, 5) \
            or tuple(moving.shape) != tuple(fixed.shape):
        raise ValueError("%s: moving and fixed must be two [B,1,*vol] tensors of one shape" % what)
    nd = moving.dim() - 2
    B, vol = int(moving.shape[0]), tuple(int(n) for n in moving.shape[2:])
    if update not in ('add', 'compose'):
        raise ValueError("%s: update must be 'add' or 'compose', got %r" % (what, update))
    if not isinstance(diffeomorphic, bool):
        raise ValueError("%s: diffeomorphic must be a bool, got %r" % (what, diffeomorphic))
    if isinstance(exp_steps, bool) or not isinstance(exp_steps, int) or not 0 <= exp_steps <= 8:
        raise ValueError("%s: exp_steps must be an integer in 0..8, got %r" % (what, exp_steps))
    if not _finite_number(max_step) or not max_step > 0:
        raise ValueError("%s: max_step must be a finite number > 0, got %r" % (what, max_step))
    for name, sg in (("sigma_fluid", sigma_fluid), ("sigma_diffusion", sigma_diffusion)):
        if not _finite_number(sg) or sg < 0:
            raise ValueError("%s: %s must be a finite number >= 0, got %r" % (what, name, sg))
        ops.gauss_radii(sg, 3.0, nd, "%s: %s" % (what, name))
    try:
        levels = tuple(levels)
    except TypeError:
        raise ValueError("%s: levels must be a sequence of integers >= 1, got %r" % (what, levels)) from None
    if not levels or any(isinstance(s, bool) or not isinstance(s, int) or s < 1 for s in levels):
        raise ValueError("%s: levels must be a non-empty sequence of integers >= 1, got %r" % (what, levels))
    for s in levels:
        if min(n // s for n in vol) < 2:
            raise ValueError("%s: every extent of a level must be >= 2, got %s // %d" % (what, vol, s))
    if isinstance(iters, int) and not isinstance(iters, bool):
        iters = (iters,) * len(levels)
    try:
        iters = tuple(iters)
    except TypeError:
        raise ValueError("%s: iters must be an integer >= 0 or one per level, got %r" % (what, iters)) from None
    if len(iters) != len(levels) or any(isinstance(n, bool) or not isinstance(n, int) or n < 0 for n in iters):
        raise ValueError("%s: iters must be an integer >= 0 or one per level (%d), got %r" % (what, len(levels), iters))
    if flow is not None and (not torch.is_tensor(flow) or tuple(flow.shape) != (B, nd) + vol or flow.dtype != torch.float32):
        raise ValueError("%s: flow must be an fp32 tensor [B,%d,*vol] = %s" % (what, nd, (B, nd) + vol))
    _check_features(what, features, moving, nd, B, vol)
    if mask is not None:
        if not torch.is_tensor(mask):
            raise ValueError("%s: mask must be a tensor" % what)
        try:
            mask = mask.expand((B, 1) + vol)
        except RuntimeError:
            raise ValueError("%s: mask %s does not broadcast to %s" % (what, tuple(mask.shape), (B, 1) + vol)) from None
    Mm, Mf = _resolve_features(features, moving, fixed, mind_radius, mind_dilation)
    full = ops.pack_features(Mm)
    dev = full.packed.device
    if mask is not None:
        mask = mask.detach().to(device=dev, dtype=torch.float32).contiguous()
    flow0 = ops.zeros((B, nd) + vol, dev) if flow is None else flow.detach().to(dev).clone(memory_format=torch.contiguous_format)
    history = torch.empty((sum(iters),), device=dev, dtype=torch.float32)
    energy0 = ops.warp_ssd(full, Mf, flow0, mask)
    u, s_prev, row = flow0, 1, 0
    for s, n in zip(levels, iters):
        if n == 0:
            continue
        if s == 1:
            h, Lf, Lk = full, Mf, mask
        else:
            h, Lf = ops.pack_features(ops.pool_features(Mm, s)), ops.pool_features(Mf, s)
            Lk = None if mask is None else ops.pool_features(mask, s)
        lvol = tuple(m // s for m in vol)
        if s != s_prev or tuple(u.shape[2:]) != lvol:
            u = ops.resize_linear(u, lvol, mult=float(s_prev) / float(s))
        for k in range(n):
            d, L, _ = ops.demons_force(h, Lf, u, Lk, max_step)
            history[row + k] = L
            if sigma_fluid > 0:
                d = ops.gaussian_smooth(d, sigma_fluid)
            if diffeomorphic:
                d = d * (2.0 ** -exp_steps)
                for _ in range(exp_steps):
                    d = ops.vecint_step(d)
            u = ops.compose_flows(d, u) if update == 'compose' else u + d
            if sigma_diffusion > 0:
                u = ops.gaussian_smooth(u, sigma_diffusion)
        row += n
        s_prev = s
    if s_prev != 1:
        u = ops.resize_linear(u, vol, mult=float(s_prev))
    return dict(flow=u, warped=_final_warp(moving, u, interp), history=history, energy0=energy0,
                energy=ops.warp_ssd(full, Mf, u, mask))


def _refine_kwargs(refine, what):
    if not isinstance(refine, dict):
        raise ValueError("%s: refine must be None or a dict of refine_flow keywords, got %s" % (what, type(refine).__name__))
    return refine


@torch.no_grad()
def register_volume(model, data, refine=None):
    """The inference entry of Registration3DModel: register data['A'] onto data['B'].  Returns dict(warped_A, flow) of
    netR(real_A, real_B, registration=True); with refine = a dict of refine_flow keywords (lam and lr at least) the flow is
    then refined on this pair and 'refined_flow', 'refined_A' (real_A warped by it) and 'history' are added.  The dict may
    carry any refine_flow keyword, parametrisation='bspline' among them."""
    if refine is not None:
        _refine_kwargs(refine, "register_volume")
    model.set_input(data)
    warped_A, flow = model.netR(model.real_A, model.real_B, registration=True)
    out = dict(warped_A=warped_A, flow=flow)
    if refine is not None:
        res = refine_flow(model.real_A, model.real_B, flow, **refine)
        out.update(refined_flow=res['flow'], refined_A=res['warped'], history=res['history'])
    return out


@torch.no_grad()
def register_pair(model, data, label=None, fixed_label=None, labels=None):
    """Returns dict(fake_B, idt_B, translated_B, warped_A, flow[, warped_label][, dice]).

    model: a REGISTRATIONModel (train or test mode); data: {'A','B','A_paths','B_paths'};
    label: optional [B,1,H,W] tensor warped with mode='nearest' by the same flow (test.py:80-81);
    fixed_label, labels (with `label`; all three or none take effect): `label` and `fixed_label` are then integer label
    maps of A and B and `labels` the label values to score -> 'dice', the [B,K] hard-Dice table of A's label warped with
    nearest-neighbour sampling against B's label, under the same flow that produces 'warped_label'
    (ops.warp_dice, mode='nearest')."""
    model.set_input(data)
    model.forward()                                        # model.test() without the visuals hook
    translated_B = model.netG(model.real_B)                # test.py:77
    warped_A, flow = model.netR(model.real_A, model.real_B, registration=True)   # test.py:78
    out = dict(fake_B=model.fake_B, idt_B=model.idt_B, translated_B=translated_B, warped_A=warped_A, flow=flow)
    if label is not None:
        st = SpatialTransformer(tuple(flow.shape[2:]), mode='nearest').to(flow.device)
        out['warped_label'] = st(label.to(flow.device).float(), flow)
        if fixed_label is not None and labels is not None:
            mov = ops.as_label_map(label.to(flow.device))
            fix = ops.as_label_map(fixed_label.to(flow.device))
            out['dice'] = ops.warp_dice(mov, fix, flow.detach(), labels, mode='nearest')[1]
    return out


@torch.no_grad()
def register_pair_refined(model, data, refine, label=None, fixed_label=None, labels=None):
    """register_pair followed by instance optimisation of its flow: register_pair's own dict (every key as it is, 'warped_label'
    and 'dice' those of the network's flow) plus 'refined_flow', 'refined_A' and 'history' of refine_flow(real_A, real_B,
    flow, **refine); refine = a dict of refine_flow keywords (lam and lr at least; parametrisation='bspline' is accepted like
    any other).  A function of its own because register_pair's signature is pinned."""
    _refine_kwargs(refine, "register_pair_refined")
    out = register_pair(model, data, label, fixed_label, labels)
    res = refine_flow(model.real_A, model.real_B, out['flow'], **refine)
    out.update(refined_flow=res['flow'], refined_A=res['warped'], history=res['history'])
    return out


@torch.no_grad()
def score_labels(warped_label, fixed_label, labels, percentile=100.0, surface=False):
    """Hausdorff scores of a warped label map (register_pair's 'warped_label', label ids warped with mode='nearest')
    against the fixed one: dict(hd[B,K], directed[2,B,K], mean[2,B,K]) in voxels per listed label value
    (ops.label_hausdorff; direction 0 is warped -> fixed).  Maps that are not uint8 go through ops.as_label_map."""
    dev = warped_label.device
    a = warped_label if warped_label.dtype == torch.uint8 else ops.as_label_map(warped_label)
    fixed_label = fixed_label.to(dev)
    b = fixed_label if fixed_label.dtype == torch.uint8 else ops.as_label_map(fixed_label)
    hd, directed, mean, _ = ops.label_hausdorff(a, b, labels, percentile, surface)
    return dict(hd=hd, directed=directed, mean=mean)


@torch.no_grad()
def inverse_consistency_error(flow_ab, flow_ba, spacing=None):
    """The invertibility diagnostic of a registration: per sample, the RMS over the voxels of |r|, r(x) = flow_ab(x) +
    flow_ba(x + flow_ab(x)) -- how far a point lands from where it started after going there and back.  A [B] tensor,
    sqrt(nd * IC_b) of ops.inverse_consistency_per_sample, in voxels; with an isotropic `spacing` (one positive number,
    or a sequence of nd equal ones) in physical units.  An anisotropic spacing raises: the kernel sums the squared
    components of r with equal weights, so a per-axis scale cannot be applied to the sum afterwards."""
    nd = flow_ab.dim() - 2
    h = 1.0
    if spacing is not None:
        try:                                      # a number (a 0-dim tensor or numpy scalar too), or a sequence of nd
            sp = torch.as_tensor(spacing, dtype=torch.float64).cpu()
        except (TypeError, ValueError, RuntimeError):
            raise ValueError("inverse_consistency_error: spacing must be %d positive finite numbers, got %r" % (nd, spacing))
        vals = [float(sp)] * nd if sp.dim() == 0 else sp.flatten().tolist()
        if len(vals) != nd or not all(0.0 < s < float('inf') for s in vals):
            raise ValueError("inverse_consistency_error: spacing must be %d positive finite numbers, got %r" % (nd, spacing))
        if any(s != vals[0] for s in vals):
            raise ValueError("inverse_consistency_error: anisotropic spacing %r is not supported: the per-sample sum adds "
                             "the squared components of r with equal weights, so a per-axis scale cannot be applied to it "
                             "afterwards; resample the fields to isotropic voxels or scale their channels first"
                             % (spacing,))
        h = vals[0]
    ic = ops.inverse_consistency_per_sample(flow_ab, flow_ba)
    return torch.sqrt(ic * float(nd)) * h


@torch.no_grad()
def invert_flow(flow, iters=20, tol=0.0):
    """The inverse of a registration's flow by fixed-point iteration (ops.invert_flow, which states the definition and where
    the iteration converges): register_pair / register_volume map A onto B, the inverse carries what lives in B's space --
    labels, landmarks -- back into A's.  Returns dict(inverse [B,nd,*vol]; residual [B] = the RMS over the voxels of |r|, r =
    inverse + flow(x + inverse(x)), in voxels; residual_max [B] = max |r_c|; history [iters + 1, B, 2] = (rms, max) of every
    iteration; roundtrip [B] = inverse_consistency_error(flow, inverse), the OTHER direction flow + inverse(x + flow(x)),
    which the iteration does not drive to zero by itself: a diagnostic).  A residual that stays large says the flow is no
    contraction somewhere, typically at the volume border (zero padding) or where it folds."""
    inverse, history = ops.invert_flow(flow, iters=iters, tol=tol, history=True)
    return dict(inverse=inverse, residual=history[-1, :, 0].clone(), residual_max=history[-1, :, 1].clone(), history=history,
                roundtrip=inverse_consistency_error(flow, inverse))


@torch.no_grad()
def flow_regularity(flow, border=1, log_offset=0.0):
    """The regularity of a deformation, the number reported beside Dice / HD95 / TRE: where phi = x + flow folds and how far
    its volume change spreads.  flow: [B,nd,*vol] fp32 in voxels (ops.warp's convention).  With d = det J, J = I + the central
    differences of the flow, on Omega = the voxels at least `border` away from every face (the definition:
    losses.JacobianDet_Loss), returns dict(folded [B] = the fraction of Omega with d <= 0, folded_count [B], min [B], max
    [B], mean [B] of d, sdlogj [B] = the population standard deviation of log(max(d + log_offset, 1e-9)), all float64;
    detmap [B,1,*vol] fp32 = d on Omega and exactly 1.0 outside).  flow_regularity(flow, border=2, log_offset=3.0) gives the
    Learn2Reg numbers (SDlogJ of the determinant shifted by 3 and clipped, two voxels cropped per face); the defaults give
    the plain log on the largest domain the central differences allow.  The determinant does not depend on the voxel
    spacing, so there is no spacing argument.  This is the check behind invert_flow's remark that a residual which stays
    large typically means a fold."""
    stats = ops.jacobian_stats(flow, border, log_offset)
    omega = 1
    for n in flow.shape[2:]:
        omega *= int(n) - 2 * int(border)
    return dict(folded=stats[:, 0] / float(omega), folded_count=stats[:, 0].clone(), min=stats[:, 1].clone(),
                max=stats[:, 2].clone(), mean=stats[:, 3].clone(), sdlogj=stats[:, 5].clone(),
                detmap=ops.jacobian_determinant(flow, border))


@torch.no_grad()
def pull_back_label(fixed_label, flow, iters=20, tol=0.0):
    """Carry B's label map into A's space: `flow` registers A onto B (warped_A(x) = A(x + flow(x)), x in B's grid), so B's
    labels are sampled with nearest-neighbour interpolation under the INVERSE flow (ops.invert_flow(flow, iters, tol)):
    label(y) = fixed_label(y + inverse(y)), y in A's grid, by SpatialTransformer(mode='nearest').  fixed_label: [B,1,*vol], any
    dtype that converts to float exactly.  Returns dict(label (fp32), inverse, residual [B], residual_max [B]) -- the
    residuals of the inversion as infer.invert_flow reports them: check them before trusting the labels."""
    inverse, stats = ops.invert_flow(flow, iters=iters, tol=tol)
    st = SpatialTransformer(tuple(flow.shape[2:]), mode='nearest').to(flow.device)
    label = st(fixed_label.to(flow.device).float(), inverse)
    return dict(label=label, inverse=inverse, residual=stats[:, 0].clone(), residual_max=stats[:, 1].clone())


@torch.no_grad()
def landmark_error(flow, fixed_pts, moving_pts, spacing=None, weight=None):
    """The target registration error of corresponding landmarks, the headline number of multi-modal registration:
    dict(tre [B,K], initial [B,K], mean [B]).  `tre` = |h * (q + flow(q) - p)| per landmark from the landmark kernel
    (ops.landmark_distances; q = fixed_pts, p = moving_pts [B,K,nd] in voxel coordinates, axis order (z,) y, x as the flow's
    channels, h = `spacing`, nd positive numbers, None = 1: anisotropic spacing is applied per axis), NaN for an invalid
    landmark (weight 0, a non-finite coordinate, q outside the volume); `initial` = |h * (q - p)|, the error before
    registration, with the same NaN pattern; `mean` = per sample the weighted mean of `tre` over its valid landmarks (NaN
    without one).  The definition: losses.Landmark_Loss."""
    tre, mean = ops.landmark_distances(flow, fixed_pts, moving_pts, weight, spacing)
    nd = flow.dim() - 2
    h = torch.tensor(ops.bending_spacing(spacing, (nd,), "landmark_error"), dtype=torch.float32, device=tre.device)
    initial = ((fixed_pts - moving_pts) * h).square().sum(2).sqrt()
    initial = torch.where(torch.isnan(tre), tre, initial)
    return dict(tre=tre, initial=initial, mean=mean)


@torch.no_grad()
def landmark_init(moving, fixed, fixed_pts, moving_pts, *, spacing=None, smoothing=0.0, weight=None, interp='linear'):
    """Stage 0 of the inference pipeline for a pair with corresponding keypoints (annotated, detected or predicted): the
    thin-plate-spline flow through them (build-defined; the definition: ops.tps_fit).  Returns dict(flow, warped, coef, tre).

    moving, fixed: [B,C,*vol] fp32 images of one shape, 2-D or 3-D (`fixed` gives the grid; only `moving` is sampled);
    fixed_pts q, moving_pts p: [B,K,nd] fp32 voxel coordinates, axis order (z,) y, x, nd + 1 <= K <= ops.LANDMARK_MAX_K;
    spacing: nd positive numbers (None = 1); smoothing: lambda >= 0, 0 interpolates (flow(q_k) = p_k - q_k); weight: [B,K]
    or None, 0 marks a padding entry, as does a non-finite coordinate.

        flow   = ops.tps_flow(ops.tps_fit(q, p, vol, spacing, smoothing, weight))     [B,nd,*vol], ops.warp's convention
        warped = ops.warp(moving, flow) (interp 'linear') or ops.warp_cubic(moving, flow) ('cubic')
        coef   = the float64 coefficients [B,K+nd+1,nd] = [w; a_0; A] of the fit
        tre    = ops.landmark_distances(flow, q, p, weight, spacing)[0]               [B,K], NaN for an invalid landmark

    The flow feeds the solvers directly: refine_flow(moving, fixed, flow), demons_flow(moving, fixed, flow).  The fit syncs
    with the host once.  No gradient is recorded (for a loss through the interpolant use ops.tps_fit and ops.tps_flow).
    ValueError on an unknown interp, images that are not two tensors of one [B,C,*vol] shape, and whatever ops.tps_fit
    refuses (a singular system included)."""
    what = "landmark_init"
    _check_interp(what, interp)
    if not (torch.is_tensor(moving) and torch.is_tensor(fixed)) or moving.dim() not in (4, 5) \
            or tuple(moving.shape) != tuple(fixed.shape):
        raise ValueError("%s: moving and fixed must be two [B,C,*vol] tensors of one shape" % what)
    vol = tuple(int(n) for n in moving.shape[2:])
    if torch.is_tensor(fixed_pts) and fixed_pts.dim() == 3 and int(fixed_pts.shape[0]) != int(moving.shape[0]):
        raise ValueError("%s: %d samples of images, %d of points" % (what, int(moving.shape[0]), int(fixed_pts.shape[0])))
    fixed_pts = fixed_pts.detach() if torch.is_tensor(fixed_pts) else fixed_pts
    moving_pts = moving_pts.detach() if torch.is_tensor(moving_pts) else moving_pts
    handle = ops.tps_fit(fixed_pts, moving_pts, vol, spacing, smoothing, weight)
    flow = ops.tps_flow(handle)
    tre = ops.landmark_distances(flow, fixed_pts, moving_pts, weight, spacing)[0]
    return dict(flow=flow, warped=_final_warp(moving.detach(), flow, interp), coef=handle.coef, tre=tre)


@torch.no_grad()
def keypoint_init(moving, fixed, *, features='mind', mind_radius=2, mind_dilation=2, num_keypoints=2048, sigma=1.5,
                  nms_radius=3, mask=None, threshold=0.0, search_radius=8, search_step=2, patch=2, coeffs=CONVEX_COEFFS,
                  smoothing=1e-3, spacing=None, interp='linear'):
    """Stage 0 of the inference pipeline for a pair WITHOUT annotated keypoints (build-defined): detect distinctive points of
    the fixed image, search a wide window around each one only, regularise the sparse displacements against a thin-plate
    spline and interpolate -- the sparse answer to motion beyond convex_init's dense window (search_radius * search_step
    voxels per axis, 16 at the defaults).  Returns dict(flow, warped, fixed_pts, moving_pts, weight, idx, tre).

    moving, fixed: [B,1,*vol] fp32 images of one shape, 2-D or 3-D; features as in convex_init ('mind', 'intensity' or a pair
    (moving features, fixed features) of [B,C,*vol] tensors, 1 <= C <= 16); num_keypoints: K in 1..ops.LANDMARK_MAX_K;
    sigma, spacing: ops.foerstner_response's; nms_radius, mask, threshold: ops.local_maxima's; search_radius, search_step, patch:
    ops.keypoint_cost's radius, step and patch (search_radius is clamped by nothing: 1..8 in 3-D, 1..16 in 2-D, the default 8
    suits 3-D); coeffs: the coupling coefficients, finite floats >= 0, in the order they are applied; smoothing: the lambda
    of every ops.tps_fit; interp: the final warp, as landmark_init.

        q, w  = ops.select_keypoints(ops.local_maxima(ops.foerstner_response(fixed, sigma, spacing), nms_radius, mask,
                                                      threshold), num_keypoints)
        cost  = ops.keypoint_cost(Mf, Mm, q, search_radius, search_step, patch)          Mf, Mm: the fixed / moving features
        disp  = ops.keypoint_argmin(cost, search_radius, search_step)[1]
        for c in coeffs:
            prior     = ops.tps_points(ops.tps_fit(q, q + disp, vol, spacing, smoothing, w), q)
            idx, disp = ops.keypoint_argmin(cost, search_radius, search_step, prior, c)
        p = q + disp

    (ops.tps_points returns the spline's DISPLACEMENT at the points, which is the prior; nothing is subtracted.)
        flow, warped, tre  exactly as landmark_init(moving, fixed, q, p, spacing=spacing, smoothing=smoothing, weight=w,
                                                    interp=interp) returns them

    fixed_pts = q, moving_pts = p [B,K,nd], weight = w [B,K] (the response at the keypoint; 0 and NaN coordinates mark the
    padding of a sample with fewer than K peaks), idx = the index field of the last argmin, int32 [B,K].

    Each ops.tps_fit syncs with the host once: len(coeffs) + 1 syncs per call; nothing else does.  Fewer than nd + 1 valid
    keypoints in a sample surfaces as ops.tps_fit's ValueError (the spline system is singular).

    The default `coeffs` are the numbers of the published coupled-convex schedule and `smoothing` is a borrowed number too:
    the cost here is a mean over channels and patch, the displacements are in voxels and the prior is a spline, not a box
    mean, so their scale is not the published one, and nobody has measured registration quality with them.

    ValueError before any launch on an unknown interp, images that are not two [B,1,*vol] tensors of one shape (any channel
    count with a feature pair), an unknown `features`, and every parameter the ops above refuse (num_keypoints, sigma,
    spacing, nms_radius, mask, threshold, search_radius, search_step, patch, the staged extent, a coefficient that is
    negative or not finite, smoothing)."""
    what = "keypoint_init"
    _check_interp(what, interp)
    if not (torch.is_tensor(moving) and torch.is_tensor(fixed)) or moving.dim() not in (4, 5) \
            or tuple(moving.shape) != tuple(fixed.shape):
        raise ValueError("%s: moving and fixed must be two [B,1,*vol] tensors of one shape" % what)
    nd = moving.dim() - 2
    B, vol = int(moving.shape[0]), tuple(int(n) for n in moving.shape[2:])
    _check_features(what, features, moving, nd, B, vol)
    if fixed.shape[1] != 1:
        raise ValueError("%s: the keypoints are detected on a single-channel fixed image, got %d channels" % (what, fixed.shape[1]))
    ops._keypoint_int(num_keypoints, 1, ops.LANDMARK_MAX_K, what, "num_keypoints")
    ops.bending_spacing(spacing, (nd,), what)
    ops.gauss_radii(sigma, 3.0, nd, what)
    ops._keypoint_int(nms_radius, 1, ops.KEYPOINT_NMS_MAX_RADIUS, what, "nms_radius")
    if mask is not None and (not torch.is_tensor(mask) or tuple(mask.shape) != tuple(fixed.shape)
                             or mask.dtype != torch.float32 or mask.requires_grad):
        raise ValueError("%s: mask must be an fp32 tensor [B,1,*vol] = %s that does not require grad" % (what, tuple(fixed.shape)))
    for name, t in (("moving", moving), ("fixed", fixed)):
        if t.dtype != torch.float32:
            raise ValueError("%s: fp32 tensors only (%s is %s)" % (what, name, t.dtype))
    if not _finite_number(threshold):
        raise ValueError("%s: threshold must be a finite number, got %r" % (what, threshold))
    ops._keypoint_window(search_radius, search_step, nd, what)
    ops._keypoint_int(patch, 0, ops.KEYPOINT_MAX_PATCH, what, "patch")
    if 2 * (search_radius * search_step + patch) + 1 > ops.KEYPOINT_MAX_EXTENT:
        raise ValueError("%s: the staged extent 2 (search_radius search_step + patch) + 1 exceeds ops.KEYPOINT_MAX_EXTENT = %d"
                         % (what, ops.KEYPOINT_MAX_EXTENT))
    try:
        coeffs = tuple(float(c) for c in coeffs)
    except (TypeError, ValueError):
        raise ValueError("%s: coeffs must be a sequence of finite numbers >= 0, got %r" % (what, coeffs))
    if not all(0.0 <= c < float('inf') for c in coeffs):
        raise ValueError("%s: coeffs must be a sequence of finite numbers >= 0, got %r" % (what, coeffs))
    if not _finite_number(smoothing) or smoothing < 0:
        raise ValueError("%s: smoothing must be a finite number >= 0, got %r" % (what, smoothing))
    Mm, Mf = _resolve_features(features, moving, fixed, mind_radius, mind_dilation)
    peaks = ops.local_maxima(ops.foerstner_response(fixed.detach(), sigma, spacing), nms_radius, mask, threshold)
    q, w = ops.select_keypoints(peaks, num_keypoints)
    cost = ops.keypoint_cost(Mf, Mm, q, search_radius, search_step, patch)
    idx, disp = ops.keypoint_argmin(cost, search_radius, search_step)
    for c in coeffs:
        prior = ops.tps_points(ops.tps_fit(q, q + disp, vol, spacing, smoothing, w), q)
        idx, disp = ops.keypoint_argmin(cost, search_radius, search_step, prior, c)
    p = q + disp
    res = landmark_init(moving, fixed, q, p, spacing=spacing, smoothing=smoothing, weight=w, interp=interp)
    return dict(flow=res['flow'], warped=res['warped'], fixed_pts=q, moving_pts=p, weight=w, idx=idx, tre=res['tre'])
