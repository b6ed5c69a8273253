"""Inference path (reference test.py:37-90): translate B, register A onto B, and
warp a label map with nearest-neighbour sampling -- all on the HIP device (the reference moves the label
warp to the CPU, test.py:80-81)."""
import torch

from . import ops
from .voxelmorph import SpatialTransformer


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
