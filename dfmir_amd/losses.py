"""Registration losses with the reference's interfaces: `smooothing_loss`
(models/registration_model.py:25-32), `NCC_Loss` / `Grad_Loss` / `NMI_Loss` (util/losses.py:81-348) and vxm `NCC` / `MSE` /
`Dice` / `Grad` (models/voxelmorph/torchvoxelmorph/losses.py:7-117; also reachable as `dfmir_amd.voxelmorph.losses`), each
one fused HIP reduction (dfmir_amd.ops); `BendingEnergy_Loss` (build-defined) is the second-order flow regulariser; `JacobianDet_Loss` (build-defined) is the fold penalty of a flow; `MIND_Loss` (build-defined) is the MIND-SSC multi-modal similarity; `GradField_Loss` (build-defined) is the normalised-gradient-field multi-modal similarity; `LabelDice` (build-defined) is the Dice of label maps under a flow.  `HausdorffDistance`
(util/loss_metrics.py:105-132) and `LabelHausdorff` (build-defined) are evaluation metrics on the HIP distance transform."""
import numpy as np
import torch

from . import ops


def smooothing_loss(y_pred):
    """(mean(dx^2) + mean(dy^2)) / 2 of a 2-D flow [B,2,H,W] (sic, three o's)."""
    return ops.flow_smoothness(y_pred)


class _Loss(object):
    def __init__(self, name=None, *args, **kwargs):
        self.name = name

    def __call__(self, *args, **kwargs):
        return self.forward(*args, **kwargs)


class Grad_Loss(_Loss):
    """util/losses.py:81-130: mean over axes of mean(|forward difference|) ('l1', i.e. any penalty other than 'l2' in the
    reference) or of its square ('l2'); `mask=` multiplies the field first (:119-121); `loss_mult` scales the result.
    Degenerate axes: an axis of extent 1 has no forward differences and the reference's mean over nothing is NaN; here such
    an axis contributes 0 (value and gradient) and the divisor stays the number of axes -- except a 3-D field of ONE plane
    ([B,C,1,H,W]), which is taken as the 2-D field it is: mean over H and W only, divided by 2."""

    def __init__(self, dim=2, penalty='l2', name=None, loss_mult=None, *args, **kwargs):
        super().__init__(name=name or 'gradient')
        assert dim in [2, 3]
        self.dim, self.penalty, self.loss_mult = dim, penalty, loss_mult

    def forward(self, prediction, *args, **kwargs):
        if prediction.dim() - 2 != self.dim:
            raise ValueError("Grad_Loss(dim=%d) got a %d-D field" % (self.dim, prediction.dim() - 2))
        if 'mask' in kwargs:
            m = kwargs['mask'].to(device=prediction.device, dtype=torch.float32).expand_as(prediction).contiguous()
            prediction = ops.mul(prediction, m)
        loss = ops.flow_smoothness(prediction, 'l2' if self.penalty == 'l2' else 'l1')
        if self.loss_mult is not None:
            loss = ops.scale(loss.view(1), self.loss_mult).view(())
        return loss


class BendingEnergy_Loss(_Loss):
    """Build-defined (the reference's regulariser, util/losses.py:81-130, is first-order only): the bending energy of a
    field, the second-order companion of Grad_Loss -- it charges nothing for an affine motion.
    `BendingEnergy_Loss(dim, spacing)(prediction, mask=...)`, Grad_Loss's calling convention.

    Field u [B,C,*vol], fp32, nd = `dim` spatial axes a in the order (z,) y, x with extents n_a; any C >= 1; `spacing` =
    the voxel spacing h_a > 0 in that order (None = 1).  Omega = the voxels whose whole 3^nd neighbourhood lies inside the
    volume, 1 <= p_a <= n_a - 2 on every axis.  For p in Omega:

        u_aa(p) = (u(p+e_a) - 2 u(p) + u(p-e_a)) / h_a^2
        u_ab(p) = (u(p+e_a+e_b) - u(p+e_a-e_b) - u(p-e_a+e_b) + u(p-e_a-e_b)) / (4 h_a h_b),   a < b
        e(p)    = sum_a u_aa(p)^2 + 2 sum_{a<b} u_ab(p)^2
        loss    = sum over (b, c, p in Omega) of e / N,   N = B C |Omega|

    The gradient is the exact adjoint; with U = a derivative value extended by 0 outside Omega:

        dL/du(p) = (2 / N) [ sum_a (U_aa(p-e_a) - 2 U_aa(p) + U_aa(p+e_a)) / h_a^2
                   + 2 sum_{a<b} (U_ab(p-e_a-e_b) - U_ab(p-e_a+e_b) - U_ab(p+e_a-e_b) + U_ab(p+e_a+e_b)) / (4 h_a h_b) ]

    A volume of one plane [B,C,1,H,W] is the 2-D field it is, as for Grad_Loss: the terms run over y and x, the first
    spacing entry is ignored.  Any other axis shorter than 3 leaves Omega empty and raises a ValueError before anything
    is launched.  `mask=` multiplies the field first, `loss_mult` scales the result.  Bit-identical from run to run;
    capturable (ops.bending_energy; dfmir_amd/csrc/bend.hip)."""

    def __init__(self, dim=3, spacing=None, name=None, loss_mult=None, *args, **kwargs):
        super().__init__(name=name or 'bending')
        if dim not in (2, 3):
            raise ValueError("BendingEnergy_Loss: dim must be 2 or 3, got %r" % (dim,))
        self.dim, self.loss_mult = dim, loss_mult
        self.spacing = ops.bending_spacing(spacing, (dim,), "BendingEnergy_Loss")

    def forward(self, prediction, *args, **kwargs):
        if prediction.dim() - 2 != self.dim:
            raise ValueError("BendingEnergy_Loss(dim=%d) got a %d-D field" % (self.dim, prediction.dim() - 2))
        ops.bending_geom(prediction, self.spacing, "BendingEnergy_Loss")      # (a bad shape raises before the mask is applied)
        if 'mask' in kwargs:
            m = kwargs['mask'].to(device=prediction.device, dtype=torch.float32).expand_as(prediction).contiguous()
            prediction = ops.mul(prediction, m)
        loss = ops.bending_energy(prediction, self.spacing)
        if self.loss_mult is not None:
            loss = ops.scale(loss.view(1), self.loss_mult).view(())
        return loss


class JacobianDet_Loss(_Loss):
    """Build-defined (the reference has no Jacobian code): the fold penalty of a displacement field.  Grad_Loss,
    BendingEnergy_Loss and InverseConsistency_Loss charge roughness; this one charges a fold as such.
    `JacobianDet_Loss(dim, eps, power, border)(prediction, mask=...)`, Grad_Loss's calling convention.

    Field u [B,nd,*vol], fp32, nd = `dim` = 2 or 3.  Channel a is the displacement in voxels along axis a, in the order
    (z,) y, x (ops.warp's convention); phi(x) = x + u(x).  `border` = m >= 1 (an integer); Omega_m = the voxels with
    m <= p_a <= n_a - 1 - m on every axis (m = 1 is BendingEnergy_Loss's Omega; Learn2Reg's evaluation crops 2).  For p in
    Omega_m:

        J_ab(p) = delta_ab + (u_a(p + e_b) - u_a(p - e_b)) / 2          central differences
        d(p)    = det J(p)                                              2x2 or 3x3, written out
        psi(d)  = max(0, eps - d)^power                                 power 1 or 2, eps >= 0 finite
        loss    = sum over (b, p in Omega_m) of psi(d(p)) / N,   N = B |Omega_m|

    The determinant does not depend on the voxel spacing: in physical units J_phys = H J H^-1 with H = diag(h), which has
    the same determinant.  That is why there is no `spacing` argument.

    The gradient is the exact adjoint; with W_ab(p) = psi'(d(p)) cof(J(p))_ab on Omega_m and 0 outside, cof = the cofactor
    matrix dd/dJ_ab, psi'(d) = -power max(0, eps - d)^(power - 1) (power 1: -1 where d < eps and 0 otherwise, 0 at d == eps):

        dL/du_a(q) = (1 / 2N) sum_b [ W_ab(q - e_b) - W_ab(q + e_b) ]

    The channel count must be nd: a one-plane volume [B,3,1,H,W] is refused, not reinterpreted.  An axis shorter than
    2 m + 1 leaves Omega_m empty and raises a ValueError before anything is launched.  `mask=` multiplies the field first,
    `loss_mult` scales the result.  Bit-identical from run to run; capturable (ops.jacobian_penalty;
    dfmir_amd/csrc/jacdet.hip).  The map and the statistics of d: ops.jacobian_determinant, ops.jacobian_stats,
    infer.flow_regularity."""

    def __init__(self, dim=3, eps=0.0, power=2, border=1, name=None, loss_mult=None, *args, **kwargs):
        super().__init__(name=name or 'jacdet')
        if dim not in (2, 3):
            raise ValueError("JacobianDet_Loss: dim must be 2 or 3, got %r" % (dim,))
        if isinstance(power, bool) or power not in (1, 2):
            raise ValueError("JacobianDet_Loss: power must be 1 or 2, got %r" % (power,))
        if isinstance(border, bool) or not isinstance(border, (int, np.integer)) or border < 1:
            raise ValueError("JacobianDet_Loss: border must be an integer >= 1, got %r" % (border,))
        self.dim, self.power, self.border, self.loss_mult = dim, int(power), int(border), loss_mult
        self.eps = ops._finite_ge0("JacobianDet_Loss", "eps", eps)

    def forward(self, prediction, *args, **kwargs):
        if torch.is_tensor(prediction) and prediction.dim() - 2 != self.dim:
            raise ValueError("JacobianDet_Loss(dim=%d) got a %d-D field" % (self.dim, prediction.dim() - 2))
        ops._jacobian_geom(prediction, self.border, "JacobianDet_Loss")    # (a bad argument raises before the mask is applied)
        if 'mask' in kwargs:
            m = kwargs['mask'].to(device=prediction.device, dtype=torch.float32).expand_as(prediction).contiguous()
            prediction = ops.mul(prediction, m)
        loss = ops.jacobian_penalty(prediction, self.eps, self.power, self.border)
        if self.loss_mult is not None:
            loss = ops.scale(loss.view(1), self.loss_mult).view(())
        return loss


class NCC_Loss(_Loss):
    """util/losses.py:132-261: -sqrt(mean(cc)) of the windowed correlation; with `mask` -sqrt(sum(cc * mask) / sum(mask))
    (:257-261; an empty mask gives 0 -- as a device scalar, the reference returns `torch.tensor(0)` after a host sync).
    kernel_type 'mean': a win^nd box, win = kernel_var (default [9] * nd).  'gaussian' (:153-181): sigma = kernel_var[0]
    (default 3, a positive integer <= 10; the other entries are ignored, as in the reference), K = 3 sigma + ((3 sigma + 1)
    mod 2) taps per axis, weights c * g(dy) * g(dx) with g(d) = exp(-(d - (K-1)/2)^2 / (2 sigma^2)) and c = 1 /
    (2.506628274631 sigma), NOT normalised: win_size = sum of the weights.  The reference builds that 2-D window only and
    its conv3d call fails on a 5-D tensor; the 3-D form here is build-defined: c * g(dz) * g(dy) * g(dx), same c and K,
    zero padding on all three axes, win_size = c * (sum g)^3 -- also for a one-plane volume [B,1,1,H,W], where only the
    centre z-tap meets data.  'linear' raises NotImplementedError, as in the reference."""

    def __init__(self, device, kernel_var=None, name=None, kernel_type='mean', eps=1e-5, *args, **kwargs):
        super().__init__(name=name or 'ncc')
        assert kernel_type in ['mean', 'gaussian', 'linear']
        if kernel_type == 'linear':
            raise NotImplementedError("Linear kernel for NCC still not implemented")
        if kernel_type == 'gaussian':
            ops.ncc_gauss_window(3 if kernel_var is None else kernel_var[0])      # (a bad sigma raises here)
        self.device, self.kernel_var, self.kernel_type, self.eps = device, kernel_var, kernel_type, eps

    def forward(self, prediction, target, mask=None, *args, **kwargs):
        if self.kernel_type == 'gaussian':
            sigma = 3 if self.kernel_var is None else self.kernel_var[0]
            return ops.ncc_loss(prediction, target, eps=self.eps, mask=mask, kernel='gaussian', sigma=sigma)
        nd = prediction.dim() - 2
        kv = self.kernel_var if self.kernel_var is not None else [9] * nd
        if len(set(kv)) != 1 or len(kv) != nd:
            raise NotImplementedError("NCC window must be cubic and match the tensor rank")
        return ops.ncc_loss(prediction, target, int(kv[0]), self.eps, mask=mask)


class NMI_Loss(_Loss):
    """util/losses.py:263-348: soft-binned (Parzen) mutual information of two images (Guo; Dalca et al., MedIA 2019),
    returned as -MI with shape (1,).  sigma = mean(diff(bin_centers)) * sigma_ratio; the centers need not be uniform
    (2 to 64 of them).  Both inputs are clamped to [0, max_clip] first -- data in [-1, 1] loses its negative half, as in
    the reference -- and every voxel of the batch and channels goes into ONE histogram.  crop_background=True counts only
    the voxels where `mask` > 1e-4 (any mask that broadcasts to the inputs); the reference's mask-less crop (a box filter
    over y_true) fails there with a RuntimeError, and raises a ValueError here.  An empty selection gives NaN.  Gradients
    go to both y_true and y_pred; the bin centers are constants and get none (`vol_bin_centers.requires_grad` is kept for
    the reference's attribute, but nothing flows into it).  `patch_size` is stored and unused, as in the reference.
    One HIP forward (dfmir_nmi_fwd) and one backward (dfmir_nmi_bwd)."""

    def __init__(self, bin_centers, device='cpu', sigma_ratio=0.5, max_clip=1, crop_background=False, patch_size=1,
                 name='nmi'):
        super().__init__(name=name)
        self.max_clip = max_clip
        self.patch_size = patch_size
        self.crop_background = crop_background
        self.bin_centers = [float(c) for c in np.asarray(bin_centers, dtype=np.float64).reshape(-1)]
        self.num_bins = len(self.bin_centers)
        if not 2 <= self.num_bins <= 64:
            raise ValueError("NMI_Loss supports 2 to 64 bin centers (got %d)" % self.num_bins)
        self.sigma_ratio = sigma_ratio
        self.sigma = np.mean(np.diff(self.bin_centers)) * sigma_ratio
        self.preterm = 1 / (2 * np.square(self.sigma))
        self.vol_bin_centers = torch.tensor(self.bin_centers, requires_grad=True, device=device, dtype=torch.float32)

    def __call__(self, y_true, y_pred, mask=None, padding_size=15, **kwargs):
        if self.crop_background and mask is None:
            raise ValueError("NMI_Loss(crop_background=True) needs a mask: the reference's mask-less crop does not run "
                             "(util/losses.py:298-310 passes conv%dd a stride list of the wrong length)" % (y_true.dim() - 2))
        return ops.nmi_loss(y_true, y_pred, self.bin_centers, self.sigma_ratio, float(self.max_clip),
                            mask=mask if self.crop_background else None)

    forward = __call__


class MIND_Loss(_Loss):
    """Build-defined (the reference ships no MIND): the MIND-SSC similarity of Heinrich et al. (MICCAI 2013), a local,
    contrast-invariant self-similarity descriptor compared voxel-wise with an L2 loss -- the multi-modal companion of the
    mono-modal NCC_Loss and the global NMI_Loss.  `MIND_Loss(radius, dilation)(prediction, target, mask=None)`.

    Inputs [B,1,*vol], fp32, 2-D or 3-D (nd axes); radius r and dilation d in 1..4; clamp = replicate the border per axis
    and per sample.  Neighbours n = 2 * axis + (0: -d, 1: +d) over the axes in the order (z,) y, x; channels = the pairs
    p < q of neighbours on different axes, in lexicographic order: C = 12 in 3-D -- (0,2) (0,3) (0,4) (0,5) (1,2) (1,3)
    (1,4) (1,5) (2,4) (2,5) (3,4) (3,5) -- and C = 4 in 2-D -- (0,2) (0,3) (1,2) (1,3) of -y, +y, -x, +x.  Per sample:

        s_k(y) = (I(clamp(y + p_k)) - I(clamp(y + q_k)))^2
        D_k(x) = (2r+1)^-nd * sum over t in [-r,r]^nd of s_k(clamp(x + t))    (x + t is clamped first, the shifts clamp again)
        m_k = D_k - min_j D_j,   V = mean_k m_k,   mu = mean of V over the whole tensor (batch included)
        Vc = min(max(V, 0.001 mu), 1000 mu),   M_k = exp(-m_k / Vc)  in (0, 1]

    A volume of one plane [B,1,1,H,W] keeps the 3-D definition with 12 channels (the z shifts clamp onto the plane).
    Loss: the mean over (B, C, voxels) of (M_pred - M_target)^2; with `mask` (anything that broadcasts to [B,1,*vol], float
    weights) sum mask * mean_k (.)^2 / sum mask, and 0 (a device scalar, no host sync) for an empty mask.  Gradients go to
    both images.  Three build-defined points: mu is a constant in the backward (both clamp bounds are detached); min sends
    its gradient to the FIRST minimal channel in the order above; a constant image has mu = 0, the formula is 0 / 0 there
    and the loss is NaN (no epsilon is added).  Where V is clamped nothing flows through V; everything else is the exact
    chain rule.  Bit-identical from run to run; capturable (ops.mind_loss; dfmir_amd/csrc/mind.hip)."""

    def __init__(self, radius=2, dilation=2, name='mind', *args, **kwargs):
        super().__init__(name=name)
        for what, v in (("radius", radius), ("dilation", dilation)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= 4:
                raise ValueError("MIND_Loss: %s must be an integer in 1..4, got %r" % (what, v))
        self.radius, self.dilation = int(radius), int(dilation)

    def forward(self, prediction, target, mask=None, *args, **kwargs):
        return ops.mind_loss(prediction, target, self.radius, self.dilation, mask=mask)


class GradField_Loss(_Loss):
    """Build-defined (the reference ships no such loss): the normalised-gradient-field distance of Haber & Modersitzki
    (MICCAI 2006).  It rewards image edges that are parallel or anti-parallel, whatever the contrast: the purely local
    multi-modal companion of MIND_Loss (wider capture range) and the global NMI_Loss.
    `GradField_Loss(eps, eta, dim, spacing)(prediction, target, mask=None)`.

    Images A, B [B,1,*vol], fp32, 2-D or 3-D; axes a in the order (z,) y, x of extent n_a with the voxel spacing h_a > 0
    (`spacing`, None = 1).  A volume of one plane [B,1,1,H,W] is legal and keeps three axes.  Per sample and axis, with
    replicate clamping:

        g_a(I)(x) = ( I(min(x_a + 1, n_a - 1)) - I(max(x_a - 1, 0)) ) / (2 h_a)

    -- half a one-sided difference on the border, 0 on an axis of extent 1 -- and

        dot = <g(A), g(B)>,   D_A = |g(A)|^2 + eps_A^2,   D_B = |g(B)|^2 + eps_B^2
        s(x) = dot^2 / (D_A D_B)  in [0, 1),   s = 0 with no gradient where D_A D_B == 0
        loss = mean over (B, voxels) of (1 - s)

    With `mask` (anything that broadcasts to [B,1,*vol], used as float weights) the loss is sum mask (1 - s) / sum mask;
    an empty mask gives 0 (a device scalar, no host sync) and zero gradients.

    `eps`: a positive float (both images), a pair (eps_A, eps_B) of positive floats, or 'auto' (default): eps_I = eta *
    the mean over the whole tensor (batch included) of |g(I)|_2 with eta > 0 (default 1) -- the usual automatic edge
    parameter, formed on the device in double in a fixed order and A CONSTANT IN THE BACKWARD (as mu is in MIND_Loss).
    With 'auto' the loss is invariant under I -> alpha I + beta for any alpha != 0; a constant image gets eps = 0, hence
    s = 0, loss 1 and a zero gradient.  No NaN anywhere.

    Gradients go to both images.  With w(x) = 1 / N, or mask(x) / sum mask, times the upstream gradient:

        G^A(x) = dL/dg(A)(x) = -2 w dot / (D_A D_B) * ( g(B) - (dot / D_A) g(A) )       (G^B: the mirror expression)
        dI(y)  = sum_a (1 / 2 h_a) * (   [y_a >= 1] G_a(y - e_a)     + [y_a == n_a - 1] G_a(y)
                                       - [y_a <= n_a - 2] G_a(y + e_a) - [y_a == 0] G_a(y) )

    the exact adjoint of the clamped difference (on an axis of extent 1 the terms cancel to 0).  `dim` (None = either)
    pins the number of spatial axes.  Bit-identical from run to run; capturable (ops.gradfield_loss;
    dfmir_amd/csrc/gradfield.hip)."""

    def __init__(self, eps='auto', eta=1.0, dim=None, spacing=None, name='gradfield', *args, **kwargs):
        super().__init__(name=name)
        if dim not in (None, 2, 3):
            raise ValueError("GradField_Loss: dim must be None, 2 or 3, got %r" % (dim,))
        ops.gradfield_eps(eps, eta, "GradField_Loss")
        self.eps, self.eta, self.dim = eps, eta, dim
        self.spacing = None if spacing is None else ops.bending_spacing(spacing, (2, 3) if dim is None else (dim,),
                                                                        "GradField_Loss")

    def forward(self, prediction, target, mask=None, *args, **kwargs):
        if self.dim is not None and prediction.dim() - 2 != self.dim:
            raise ValueError("GradField_Loss(dim=%d) got %d-D images" % (self.dim, prediction.dim() - 2))
        return ops.gradfield_loss(prediction, target, self.eps, self.eta, self.spacing, mask=mask)


class NCC(object):
    """vxm `NCC(win).loss(y_true, y_pred)` = -mean(cc) (models/voxelmorph/torchvoxelmorph/losses.py:7-67; eps 1e-5; the
    reference builds its filter with `.to("cuda")`, here the tensors' own device).  cc is symmetric in its arguments;
    the gradient goes to y_pred."""

    def __init__(self, win=None):
        self.win = win

    def loss(self, y_true, y_pred):
        nd = y_true.dim() - 2
        win = [9] * nd if self.win is None else list(self.win)
        if len(set(win)) != 1 or len(win) != nd:
            raise NotImplementedError("NCC window must be cubic and match the tensor rank")
        return ops.ncc_loss(y_pred, y_true, int(win[0]), 1e-5, reduction='neg_mean')


class Grad(object):
    """vxm `Grad(penalty, loss_mult).loss(_, y_pred)` (models/voxelmorph/torchvoxelmorph/losses.py:93-117): 3-D fields only
    (the reference indexes five axes); penalty 'l1' (default) or 'l2'."""

    def __init__(self, penalty='l1', loss_mult=None):
        self.penalty = penalty
        self.loss_mult = loss_mult

    def loss(self, _, y_pred):
        if y_pred.dim() != 5:
            raise IndexError("vxm Grad.loss indexes [B, C, D, H, W] fields (got %d dims)" % y_pred.dim())
        grad = ops.flow_smoothness(y_pred, 'l2' if self.penalty == 'l2' else 'l1')
        if self.loss_mult is not None:
            grad = ops.scale(grad.view(1), self.loss_mult).view(())
        return grad


class InverseConsistency_Loss(_Loss):
    """Build-defined (the reference has no such term): how far the composition of two displacement fields is from the
    identity.  `InverseConsistency_Loss(dim, symmetric)(flow_ab, flow_ba)`.

    u, v [B,nd,*vol], nd = `dim` = 2 or 3, fp32; channel i displaces axis i in voxels, in the order (z,) y, x, exactly as
    ops.warp reads a flow.

        r(x)    = u(x) + v(x + u(x))        v sampled (bi/tri)linearly, corners outside the volume read as 0:
                                            r = u + ops.warp(v, u), element for element
        IC(u,v) = mean over all B*nd*S elements of r^2          (S = voxels per sample)

    A voxel whose sample point leaves the volume contributes |u|^2 (zero padding): the warp's own convention, and one that
    does not reward pushing points out of the volume.  The gradients are the exact adjoint; with k = 2 gout / (B nd S):

        dIC/du_c(x) = k ( r_c(x) + sum_c' r_c'(x) d_c v_c'(x + u(x)) )
        dIC/dv      = the transpose of the interpolation applied to k r (a scatter to the up to 2^nd corners)

    where d_c is the derivative of the multilinear interpolant as the warp backward forms it: corner differences, with
    zero-padded corners taking part as zeros.  symmetric=True (default): 0.5 * (IC(u, v) + IC(v, u)).  `loss_mult` scales
    the result.  The value and dIC/du are bit-identical from run to run on every shape, dIC/dv wherever ops.warp's backward
    is (W % 4 == 0) and on the shapes where that is not (see ops.inverse_consistency); capturable
    (dfmir_amd/csrc/invcons.hip)."""

    def __init__(self, dim=3, symmetric=True, name=None, loss_mult=None, *args, **kwargs):
        super().__init__(name=name or 'ic')
        if dim not in (2, 3):
            raise ValueError("InverseConsistency_Loss: dim must be 2 or 3, got %r" % (dim,))
        self.dim, self.symmetric, self.loss_mult = dim, bool(symmetric), loss_mult

    def forward(self, flow_ab, flow_ba, *args, **kwargs):
        if flow_ab.dim() - 2 != self.dim:
            raise ValueError("InverseConsistency_Loss(dim=%d) got a %d-D field" % (self.dim, flow_ab.dim() - 2))
        loss = ops.inverse_consistency(flow_ab, flow_ba, symmetric=self.symmetric)
        if self.loss_mult is not None:
            loss = ops.scale(loss.view(1), self.loss_mult).view(())
        return loss


class WarpedSSD_Loss(_Loss):
    """Build-defined (the reference has no such term): the SSD between fixed-image features and warped moving-image
    features, the data term of instance optimisation (infer.refine_flow), value and flow gradient in one fused pass.
    `WarpedSSD_Loss(dim)(moving_features, fixed_features, flow, mask=None)`.

    M, F [B,C,*vol], fp32, nd = `dim` = 2 or 3, 1 <= C <= 16 (M may be the handle of ops.pack_features(M): the voxel-major
    copy the gather reads, made once per loop); phi [B,nd,*vol] a displacement in voxels, channel d displacing axis d in
    the order (z,) y, x, exactly as ops.warp reads a flow.

        e_c(x) = M_c(x + phi(x)) - F_c(x)      M sampled (bi/tri)linearly, align_corners=True, corners outside the volume
                                               read as 0: e = ops.warp(M, phi) - F, element for element
        L      = mean over (B, C, voxels) of e^2
        with `mask` m (float weights that broadcast to [B,1,*vol]):  L = sum m * mean_c e^2 / sum m,  0 for an empty mask
        (a device scalar, no host sync); per sample (ops.warp_ssd_per_sample) the same over sample b alone

        dL/dphi_d(x) = k(x) sum_c e_c(x) d_d M_c(x + phi(x)),   k = 2 gout / (B C S), masked 2 gout m(x) / (C sum m)

    where d_d is the derivative of the multilinear interpolant in the cell floor() selects: corner differences, with
    zero-padded corners taking part as zeros.  Gradients go to phi ONLY: features or a mask that require grad raise a
    ValueError instead of being dropped silently.  `loss_mult` scales the result.  Bit-identical from run to run;
    capturable (ops.warp_ssd; dfmir_amd/csrc/warpssd.hip)."""

    def __init__(self, dim=3, name=None, loss_mult=None, *args, **kwargs):
        super().__init__(name=name or 'warped_ssd')
        if dim not in (2, 3):
            raise ValueError("WarpedSSD_Loss: dim must be 2 or 3, got %r" % (dim,))
        self.dim, self.loss_mult = dim, loss_mult

    def forward(self, moving_features, fixed_features, flow, mask=None, *args, **kwargs):
        if flow.dim() - 2 != self.dim:
            raise ValueError("WarpedSSD_Loss(dim=%d) got a %d-D field" % (self.dim, flow.dim() - 2))
        loss = ops.warp_ssd(moving_features, fixed_features, flow, mask=mask)
        if self.loss_mult is not None:
            loss = ops.scale(loss.view(1), self.loss_mult).view(())
        return loss


class AffineSSD_Loss(_Loss):
    """Build-defined (the reference has no affine stage): the SSD between fixed-image features and moving-image features
    under an affine transform, the data term of affine pre-alignment (infer.affine_init), value and gradient to the
    transform's parameters in one fused pass.  `AffineSSD_Loss(dim)(moving_features, fixed_features, theta, mask=None)`.

    M, F [B,C,*vol] as for WarpedSSD_Loss (M may be the handle of ops.pack_features(M)); theta [B,nd,nd+1] fp32 = [A | t] in
    centred voxel coordinates, axis order (z,) y, x (ops.affine_flow): with c_a = (n_a - 1) / 2,

        y(x) = c + A (x - c) + t          L = WarpedSSD_Loss(dim)(M, F, phi, mask)  at  phi(x) = y(x) - x  by definition

    -- the same sampling, mean, masked form and 0 for an empty mask -- without the flow tensor or a per-voxel gradient:
    dL/dtheta[b,a,j] = sum_x dL/dphi_a(x) q_j(x), q = (x - c, 1), is added in double inside the pass.  Gradients go to theta
    ONLY: features or a mask that require grad raise a ValueError.  Bit-identical from run to run (ops.affine_ssd;
    dfmir_amd/csrc/affine.hip)."""

    def __init__(self, dim=3, name=None, *args, **kwargs):
        super().__init__(name=name or 'affine_ssd')
        if dim not in (2, 3):
            raise ValueError("AffineSSD_Loss: dim must be 2 or 3, got %r" % (dim,))
        self.dim = dim

    def forward(self, moving_features, fixed_features, theta, mask=None, *args, **kwargs):
        if not torch.is_tensor(theta) or theta.dim() != 3 or theta.shape[1] != self.dim:
            raise ValueError("AffineSSD_Loss(dim=%d) needs a theta [B,%d,%d]" % (self.dim, self.dim, self.dim + 1))
        return ops.affine_ssd(moving_features, fixed_features, theta, mask=mask)


class Landmark_Loss(_Loss):
    """Build-defined (the reference has no landmark code): the registration error of corresponding landmarks carried
    through a displacement field, the keypoint supervision of multi-modal registration.
    `Landmark_Loss(dim, penalty, spacing)(flow, fixed_pts, moving_pts, weight=None)`.

    flow u [B,nd,*vol], nd = `dim` = 2 or 3, fp32, read exactly as ops.warp reads it: channel a displaces axis a in voxels,
    in the order (z,) y, x, and warped(x) = moving(x + u(x)) with x in the fixed image's grid -- so a point q of the FIXED
    image corresponds to q + u(q) in the MOVING image.  fixed_pts q and moving_pts p: [B,K,nd] fp32 voxel coordinates, axis
    order as the flow's channels, 1 <= K <= 4096; weight w [B,K] fp32 (None = all ones; 0 marks a padding entry, so samples
    with different landmark counts share one K); `spacing` = nd positive finite numbers h (None = 1), applied per axis.
    With S_a the extent of axis a, per landmark:

        m_bk = q + u_b(q)         u_b sampled (bi/tri)linearly at q in the cell i0_a = min(floor(q_a), S_a - 2): a point on
                                  the upper face q_a = S_a - 1 reads the last cell with weight 1 on its upper corner
        r_bk = h * (m_bk - p),    d_bk = |r_bk|_2, the target registration error (TRE) of that landmark
        valid: w > 0, every coordinate of q and p finite, 0 <= q_a <= S_a - 1 on every axis

    An invalid landmark contributes to no sum and gets no gradient (its d is NaN in ops.landmark_distances).  Over the whole
    call, with Wsum the sum of w over the valid landmarks:

        penalty='l2':   loss = sum w d^2 / Wsum
        penalty='tre':  loss = sum w d / Wsum          (the derivative at d = 0 is defined as 0)
        Wsum = 0 (no valid landmark): loss 0 and an all-zero gradient, not NaN

    The gradient goes to the flow only: dflow[b, a, corner] += gout * (w / Wsum) * dl/dr_a * h_a * cornerweight, dl/dr_a =
    2 r_a ('l2') or r_a / d ('tre'); zeros at every voxel no valid landmark touches.  `loss_mult` scales the result.  Value
    and gradient are bit-identical from run to run, landmarks in one cell or at one position included; validity is decided
    on the device, so the call captures into a hipGraph (ops.landmark_loss; dfmir_amd/csrc/landmark.hip)."""

    def __init__(self, dim=3, penalty='l2', spacing=None, name=None, loss_mult=None, *args, **kwargs):
        super().__init__(name=name or 'landmark')
        if dim not in (2, 3):
            raise ValueError("Landmark_Loss: dim must be 2 or 3, got %r" % (dim,))
        if penalty not in ops.LANDMARK_PENALTIES:
            raise ValueError("Landmark_Loss: penalty must be 'l2' or 'tre', got %r" % (penalty,))
        self.dim, self.penalty, self.loss_mult = dim, penalty, loss_mult
        self.spacing = ops.bending_spacing(spacing, (dim,), "Landmark_Loss")

    def forward(self, flow, fixed_pts, moving_pts, weight=None, *args, **kwargs):
        if flow.dim() - 2 != self.dim:
            raise ValueError("Landmark_Loss(dim=%d) got a %d-D field" % (self.dim, flow.dim() - 2))
        loss = ops.landmark_loss(flow, fixed_pts, moving_pts, weight, self.spacing, self.penalty)
        if self.loss_mult is not None:
            loss = ops.scale(loss.view(1), self.loss_mult).view(())
        return loss


class MSE(object):
    """vxm `MSE().loss(y_true, y_pred)` = mean((y_true - y_pred)^2) (models/voxelmorph/torchvoxelmorph/losses.py:70-76);
    gradients to both arguments."""

    def loss(self, y_true, y_pred):
        return ops.mse_loss(y_true, y_pred)


class Dice(object):
    """vxm `Dice().loss(y_true, y_pred)` = -mean_{b,c} 2 sum(t p) / clamp(sum(t + p), min=1e-5) over float tensors
    [B,C,*vol] -- soft segmentations or one-hot label maps (models/voxelmorph/torchvoxelmorph/losses.py:79-90); gradients
    to both arguments.  For integer label maps under a flow use `LabelDice`, which never forms the one-hot tensors."""

    def loss(self, y_true, y_pred):
        return ops.dice_loss(y_true, y_pred)


class LabelDice(object):
    """Build-defined (the reference ships the pieces, not the composition): the segmentation term of semi-supervised
    VoxelMorph on integer label maps.  `LabelDice(labels, mode).loss(fixed_label, moving_label, flow)` equals

        Dice().loss(one_hot(fixed_label)[:, labels], SpatialTransformer(size, mode)(one_hot(moving_label)[:, labels], flow))

    with one_hot over the label VALUES as channels (float), i.e. -mean over (batch, listed label) of
    2 sum(t p) / clamp(sum(t + p), min=1e-5); a listed label present in neither map scores 0 and still counts in the mean,
    values that are not listed are not scored.  One fused HIP forward and one backward (ops.warp_dice): the one-hot
    tensors are never formed.  labels: 1..64 distinct integers in [0, 255]; the maps: uint8 [B,1,*vol] (anything else goes
    through ops.as_label_map, which may sync with the host -- convert once where the inputs are set).  mode 'bilinear'
    gives a gradient to `flow` only; 'nearest' is the hard Dice of the label warp of test.py:80-81 and has none.
    `.scores` holds the last [B,K] Dice table (detached)."""

    def __init__(self, labels, mode='bilinear'):
        self.labels = list(ops._dice_labels(labels))
        if mode not in ('bilinear', 'nearest'):
            raise ValueError("LabelDice mode must be 'bilinear' or 'nearest', got %r" % (mode,))
        self.mode = mode
        self.scores = None

    def loss(self, fixed_label, moving_label, flow):
        if fixed_label.dtype != torch.uint8:
            fixed_label = ops.as_label_map(fixed_label)
        if moving_label.dtype != torch.uint8:
            moving_label = ops.as_label_map(moving_label)
        loss, self.scores = ops.warp_dice(moving_label, fixed_label, flow, self.labels, self.mode)
        return loss


class HausdorffDistance(object):
    """util/loss_metrics.py:105-132: `HausdorffDistance().compute(pred, target)`, the Hausdorff distance in voxels of the
    two binary masks `pred > 0.5` and `target > 0.5` ([B,1,*vol], 2-D or 3-D): the largest distance from a voxel of one
    mask to the nearest voxel of the other, +inf when either mask is empty.  The reference copies both tensors to the host
    and runs scipy's distance transform; here the exact integer transform and the reduction are HIP kernels
    (ops.label_hausdorff) and nothing leaves the device.  Returns a [B] tensor.  For B = 1 that is the reference's value.
    Build-defined divergence for B > 1: the reference hands the whole [B,1,*vol] array to scipy, so the batch axis counts
    as a spatial axis and masks of different samples are measured against each other (a batch whose sample 0 holds only
    `pred` and whose sample 1 holds only `target` gives a finite distance there); here every sample is scored on its own."""

    def compute(self, pred, target):
        assert (
            pred.shape[1] == 1 and target.shape[1] == 1
        ), "Only binary channel supported"
        a = (pred > 0.5).to(torch.uint8)
        b = (target > 0.5).to(torch.uint8)
        return ops.label_hausdorff(a, b, [1], mean=False)[0][:, 0]


class LabelHausdorff(object):
    """Build-defined: the Hausdorff distance of two integer label maps per label value, the evaluation-side companion of
    `LabelDice`.  `LabelHausdorff(labels, percentile, surface).compute(a_label, b_label)` returns hd[B,K] in voxels: per
    listed label the larger of the two directed distances, each the `percentile` (nearest rank; 100 = the maximum, 95 =
    HD95) of the distances from the voxels of one map's label to the nearest voxel of the other's; surface=True measures
    between the border voxels instead.  A label that either map lacks scores +inf.  labels: 1..64 distinct integers in
    [0, 255]; the maps: uint8 [B,1,*vol] (anything else goes through ops.as_label_map, which may sync with the host).
    `.directed` and `.mean` hold the last call's [2,B,K] tables (direction 0: a -> b).  No gradients."""

    def __init__(self, labels, percentile=100.0, surface=False):
        self.labels = list(ops._dice_labels(labels))
        ops._hd_percentile(percentile)
        self.percentile, self.surface = float(percentile), bool(surface)
        self.directed = self.mean = None

    def compute(self, a_label, b_label):
        if a_label.dtype != torch.uint8:
            a_label = ops.as_label_map(a_label)
        if b_label.dtype != torch.uint8:
            b_label = ops.as_label_map(b_label)
        hd, self.directed, self.mean, _ = ops.label_hausdorff(a_label, b_label, self.labels, self.percentile, self.surface)
        return hd
