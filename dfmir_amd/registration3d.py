"""3-D registration step for BASELINE configs 4/5.

The reference has no 3-D entry point (`vol_shape = (crop_size, crop_size)` is hard-wired,
models/registration_model.py:97); SURVEY.md section 8 row A13 defines the composition from the pieces the
reference does ship: `VxmDense(ndims=3, int_steps=7, bidir=True)`
(models/voxelmorph/torchvoxelmorph/networks.py:1028-1145) + `NCC_Loss(kernel_var=[9,9,9], 'mean')`
(util/losses.py:132-261; ncc_kernel='gaussian' swaps in its Gaussian window) + lambda * `Grad_Loss(dim=3, 'l2')` (util/losses.py:81-130), Adam(2e-4,
(0.5, 0.999)).  Oracle counterpart: oracle/dfmir_oracle.py::Registration3DStep.  similarity='nmi' swaps the NCC term for
`NMI_Loss` (util/losses.py:263-348), the reference's multi-modal similarity; similarity='mind' for the build-defined MIND-SSC loss (`MIND_Loss`), similarity='gradfield' for the build-defined
normalised-gradient-field distance (`GradField_Loss`).  seg_labels / seg_weight add the segmentation
term of semi-supervised VoxelMorph: seg_weight * Dice of the fixed label map against the moving one warped by the flow
(`losses.LabelDice`).  regularizer='bending' swaps the diffusion penalty for the build-defined second-order
`BendingEnergy_Loss`.  symmetric=True trains both directions of the bidir network (the similarity is charged both ways);
inverse_consistency=w adds w * the build-defined `InverseConsistency_Loss` of the two integrated fields.
landmark_weight=w adds w * the build-defined `Landmark_Loss` of corresponding keypoints carried through the flow.
fold_weight=w adds w * the build-defined `JacobianDet_Loss`, the penalty on folds (det J <= fold_eps) of the forward flow.
"""
from types import SimpleNamespace

import numpy as np
import torch

from . import distributed as dfdist
from . import ops
from .losses import (BendingEnergy_Loss, Grad_Loss, GradField_Loss, InverseConsistency_Loss, JacobianDet_Loss, LabelDice,
                     Landmark_Loss, MIND_Loss, NCC_Loss, NMI_Loss)
from .optim import FlatAdam
from .voxelmorph import VxmDense


class Registration3DModel(object):
    def __init__(self, shape, features=None, lam=1.0, lr=2e-4, betas=(0.5, 0.999), win=9, device="cuda",
                 capture_step=False, deterministic_wgrad=None, similarity='ncc', nmi_bins=None, nmi_max_clip=1.0,
                 seg_labels=None, seg_weight=0.0, ncc_kernel='mean', ncc_sigma=3, mind_radius=2, mind_dilation=2,
                 regularizer='diffusion', spacing=None, symmetric=False, inverse_consistency=0.0, landmark_weight=0.0,
                 landmark_penalty='l2', fold_weight=0.0, fold_eps=0.0, fold_power=2, gradfield_eps='auto',
                 gradfield_eta=1.0):
        """similarity: 'ncc' (default: NCC_Loss with a `win`^3 window, or with ncc_kernel='gaussian' the Gaussian window of
        sigma = ncc_sigma, whose 3-D form is build-defined: see NCC_Loss; `win` is then unused) or 'nmi': NMI_Loss(real_B, warped real_A) with the
        bin centers `nmi_bins` (None = 32 uniform centers on [0, nmi_max_clip]) and max_clip = nmi_max_clip.  NMI clamps
        both images to [0, nmi_max_clip] first, as the reference does: data in [-1, 1] loses its negative half (nothing is
        rescaled here).  The loss key is then 'nmi' instead of 'ncc'.  similarity='mind': MIND_Loss(mind_radius,
        mind_dilation)(warped real_A, real_B), the local multi-modal similarity (build-defined: see MIND_Loss), for 2-D and
        3-D shapes; the loss key is 'mind'.  similarity='gradfield': GradField_Loss(gradfield_eps, gradfield_eta,
        dim=len(shape), spacing=spacing)(warped real_A, real_B), the normalised-gradient-field distance (build-defined: see
        GradField_Loss; eps 'auto', a positive float or a pair), the purely local multi-modal term for fine alignment and
        for pairs with inverted contrast, for 2-D and 3-D shapes; the loss key is 'gradfield'.
        seg_labels (a list of 1..64 label values in [0, 255]; None = no segmentation term): `set_input` then also takes
        data['A_seg'] and data['B_seg'], integer label maps [B,1,*shape] of the moving and the fixed image, and the step
        adds seg_weight * LabelDice(seg_labels).loss(B_seg, A_seg, flow); `get_current_losses()` gains 'dice'.
        regularizer: 'diffusion' (default: Grad_Loss(penalty='l2'), loss key 'grad') or 'bending': lam *
        BendingEnergy_Loss(dim=len(shape), spacing=spacing)(flow), the second-order penalty that charges nothing for an
        affine motion (build-defined: see BendingEnergy_Loss), for 2-D and 3-D shapes; `spacing` is the voxel spacing in
        the order (z,) y, x (None = 1) and is read by the bending energy, by the landmark term and by similarity='gradfield'.  The loss key is then
        'bending' instead of 'grad'.
        symmetric (build-defined, VoxelMorph's own bidirectional training; default False = the one-directional step): the
        target branch of the bidir network is computed and the similarity becomes 0.5 * (sim(y_source, real_B) +
        sim(y_target, real_A)) under the similarity's own loss key ('nmi' mirrors its argument order: NMI(real_A,
        y_target)); `regB` (real_B warped onto real_A) and `neg_flow` become outputs.  The regulariser stays on the forward
        flow and the segmentation term one-directional.
        inverse_consistency = w > 0 (needs symmetric=True, ValueError otherwise): adds w * InverseConsistency_Loss(
        symmetric=True)(flow, neg_flow), how far the two integrated fields are from being inverses of each other
        (build-defined: see InverseConsistency_Loss), for 2-D and 3-D shapes; `get_current_losses()` gains 'ic'.
        landmark_weight = w > 0 (default 0 = no landmark term): `set_input` then also takes data['A_pts'] (landmarks of
        the moving image A) and data['B_pts'] (the corresponding landmarks of the fixed image B), [B,K,nd] fp32 voxel
        coordinates in the order (z,) y, x, and optionally data['pts_weight'] [B,K] (0 marks a padding entry), and the
        step adds w * Landmark_Loss(penalty=landmark_penalty, spacing=spacing)(flow, B_pts, A_pts, pts_weight)
        (build-defined: see Landmark_Loss; landmark_penalty 'l2' or 'tre'), for 2-D and 3-D shapes; with symmetric=True
        the term is 0.5 * (L(flow, B_pts, A_pts) + L(neg_flow, A_pts, B_pts)); `get_current_losses()` gains 'landmark'.
        Which landmarks count is decided on the device, so the captured step needs no host check.
        fold_weight = w > 0 (default 0 = no fold term, nothing about the model changes): the step adds w *
        JacobianDet_Loss(dim=len(shape), eps=fold_eps, power=fold_power)(flow), the mean over the interior voxels of
        max(0, fold_eps - det J)^fold_power with J = I + the central differences of the flow (build-defined: see
        JacobianDet_Loss), for 2-D and 3-D shapes, as the LAST term; `get_current_losses()` gains 'fold'.  It stays on the
        forward flow under symmetric=True, as the regulariser does.
        capture_step (build-defined, as REGISTRATIONModel's opt.capture_step): after two eager steps forward +
        losses + backward are captured into ONE hipGraph and replayed; Adam and the gradient all-reduce stay eager.
        Small volumes are host-bound otherwise (128^3: 3.7 ms of Python / autograd / ctypes per 5.2 ms step)."""
        self.device = torch.device(device)
        if deterministic_wgrad is not None:     # (process-global switch of dfmir_amd.ops, as REGISTRATIONModel's opt.deterministic_wgrad)
            ops.set_deterministic_wgrad(deterministic_wgrad)
        self.netR = VxmDense(tuple(shape), features, int_steps=7, bidir=True).to(self.device)
        self.symmetric, self.ic_weight = bool(symmetric), float(inverse_consistency)
        if not self.ic_weight >= 0.0:
            raise ValueError("inverse_consistency must be a weight >= 0, got %r" % (inverse_consistency,))
        if self.ic_weight > 0.0 and not self.symmetric:
            raise ValueError("inverse_consistency > 0 needs symmetric=True: the one-directional step never computes the "
                             "backward field")
        self.netR.skip_unused_target = not self.symmetric      # the one-directional step reads (y_source, flow) only
        self.optimizer_R = FlatAdam(self.netR.parameters(), lr=lr, betas=betas)
        if similarity not in ('ncc', 'nmi', 'mind', 'gradfield'):
            raise ValueError("similarity must be 'ncc', 'nmi' or 'mind', or 'gradfield', got %r" % (similarity,))
        if ncc_kernel not in ('mean', 'gaussian'):
            raise ValueError("ncc_kernel must be 'mean' or 'gaussian', got %r" % (ncc_kernel,))
        self.similarity = similarity
        symmetric = self.symmetric

        def sym(fwd, rev):      # a term that symmetric=True charges both ways: its forward value, rev() the mirrored one
            return (fwd + rev()) * 0.5 if symmetric else fwd

        if similarity == 'ncc':
            kernel_var = [win if ncc_kernel == 'mean' else ncc_sigma] * len(shape)
            ncc = self.criterionNCC = NCC_Loss(self.device, kernel_var=kernel_var, kernel_type=ncc_kernel)
            sim = lambda s: sym(ncc(s.y_source, s.real_B), lambda: ncc(s.y_target, s.real_A))
        elif similarity == 'mind':
            mind = self.criterionMIND = MIND_Loss(radius=mind_radius, dilation=mind_dilation)
            sim = lambda s: sym(mind(s.y_source, s.real_B), lambda: mind(s.y_target, s.real_A))
        elif similarity == 'gradfield':
            gf = self.criterionGradField = GradField_Loss(eps=gradfield_eps, eta=gradfield_eta, dim=len(shape),
                                                          spacing=spacing)
            sim = lambda s: sym(gf(s.y_source, s.real_B), lambda: gf(s.y_target, s.real_A))
        else:
            bins = np.linspace(0.0, nmi_max_clip, 32) if nmi_bins is None else nmi_bins
            nmi = self.criterionNMI = NMI_Loss(bins, device=self.device, max_clip=nmi_max_clip)
            sim = lambda s: sym(nmi(s.real_B, s.y_source), lambda: nmi(s.real_A, s.y_target))
        if regularizer not in ('diffusion', 'bending'):
            raise ValueError("regularizer must be 'diffusion' or 'bending', got %r" % (regularizer,))
        self.regularizer = regularizer
        # The step's loss, one entry per term: (key, weight, fn) in the order the terms are added up.  fn(step) is the
        # term's scalar from the step's tensors: y_source, y_target, flow, neg_flow and the inputs named in self._inputs.
        # The first term opens the total as it is, every later one adds term * weight.  `reg` is criterionGrad, which is
        # constructed last (below).  The outputs and get_current_losses() follow from this table; the captured step takes
        # its static buffers from self._inputs (attribute names; pts_w may hold None).
        self._terms = [(similarity, 1, sim), ('bending' if regularizer == 'bending' else 'grad', lam, lambda s: reg(s.flow))]
        self._inputs = ('real_A', 'real_B')
        if self.ic_weight > 0.0:
            ic = self.criterionIC = InverseConsistency_Loss(dim=len(shape), symmetric=True)
            self._terms.append(('ic', self.ic_weight, lambda s: ic(s.flow, s.neg_flow)))
        self.landmark_weight = float(landmark_weight)
        if not self.landmark_weight >= 0.0:
            raise ValueError("landmark_weight must be a weight >= 0, got %r" % (landmark_weight,))
        self.pts_A = self.pts_B = self.pts_w = None
        if self.landmark_weight > 0.0:
            lmk = self.criterionLandmark = Landmark_Loss(dim=len(shape), penalty=landmark_penalty, spacing=spacing)
            self._terms.append(('landmark', self.landmark_weight,
                                lambda s: sym(lmk(s.flow, s.pts_B, s.pts_A, s.pts_w),
                                              lambda: lmk(s.neg_flow, s.pts_A, s.pts_B, s.pts_w))))
            self._inputs += ('pts_A', 'pts_B', 'pts_w')
        self.seg_labels, self.seg_weight = seg_labels, float(seg_weight)
        self.seg_A = self.seg_B = None
        if seg_labels is not None:
            dice = self.criterionDice = LabelDice(seg_labels)
            self.seg_labels = dice.labels
            self._terms.append(('dice', self.seg_weight, lambda s: dice.loss(s.seg_B, s.seg_A, s.flow)))
            self._inputs += ('seg_A', 'seg_B')
        self.fold_weight = float(fold_weight)
        if not 0.0 <= self.fold_weight < float('inf'):
            raise ValueError("fold_weight must be a finite weight >= 0, got %r" % (fold_weight,))
        if self.fold_weight > 0.0:
            jd = self.criterionFold = JacobianDet_Loss(dim=len(shape), eps=fold_eps, power=fold_power)
            self._terms.append(('fold', self.fold_weight, lambda s: jd(s.flow)))
        if regularizer == 'bending':
            reg = self.criterionGrad = BendingEnergy_Loss(dim=len(shape), spacing=spacing)
        else:
            reg = self.criterionGrad = Grad_Loss(dim=len(shape), penalty='l2')
        self.lam = lam
        keys = tuple('loss_' + k for k, _, _ in self._terms)
        self._outputs = ('regA', 'flow') + keys[:2] + (('regB', 'neg_flow') if symmetric else ()) + keys[2:]
        self._ddp = False
        self.capture_step = bool(capture_step) and self.device.type == "cuda"
        self._graph = {'eager_steps': 0, 'graph': None, 'shape': None, 'force_eager': False,
                       'stream': torch.cuda.Stream(device=self.device) if self.capture_step else None}

    def parallelize(self):
        self._ddp = dfdist.is_distributed()
        if self._ddp:
            dfdist.broadcast_arena(self.optimizer_R.flat_p, src=0)
            self.optimizer_R.grad_scale = 1.0 / dfdist.world_size()

    def set_input(self, data):
        self.real_A = data['A'].to(self.device, non_blocking=True)
        self.real_B = data['B'].to(self.device, non_blocking=True)
        if self.seg_labels is not None:
            for k in ('A_seg', 'B_seg'):
                if k not in data:
                    raise KeyError("Registration3DModel(seg_labels=...) needs data[%r]: an integer label map" % k)
            # (the range check of as_label_map may sync with the host: here, outside any captured region)
            self.seg_A = ops.as_label_map(data['A_seg'].to(self.device, non_blocking=True))
            self.seg_B = ops.as_label_map(data['B_seg'].to(self.device, non_blocking=True))
        if self.landmark_weight > 0.0:
            for k in ('A_pts', 'B_pts'):
                if k not in data:
                    raise KeyError("Registration3DModel(landmark_weight=...) needs data[%r]: [B,K,nd] landmark coordinates"
                                   % k)
            self.pts_A = data['A_pts'].to(self.device, non_blocking=True)
            self.pts_B = data['B_pts'].to(self.device, non_blocking=True)
            w = data.get('pts_weight')
            self.pts_w = None if w is None else w.to(self.device, non_blocking=True)

    def _forward_backward(self):
        if self.symmetric:
            y_source, y_target, flow, neg_flow = self.netR(self.real_A, self.real_B, return_neg_flow=True)
            self.regB, self.neg_flow = y_target, neg_flow
        else:
            (y_source, y_target, flow), neg_flow = self.netR(self.real_A, self.real_B), None
        self.regA, self.flow = y_source, flow
        self.optimizer_R.zero_grad()
        step = SimpleNamespace(y_source=y_source, y_target=y_target, flow=flow, neg_flow=neg_flow,
                               **{k: getattr(self, k) for k in self._inputs})
        total = None
        for key, weight, fn in self._terms:
            term = fn(step)
            setattr(self, 'loss_' + key, term)
            total = term if total is None else total + term * weight
        with ops.deferred_weight_grads():
            total.backward()

    def _apply_updates(self):
        if self._ddp:
            dfdist.allreduce_arenas([self.optimizer_R.flat_g])
        self.optimizer_R.step()

    def optimize_parameters(self):
        if not self.capture_step:
            self._forward_backward()
            return self._apply_updates()
        # The protocol of REGISTRATIONModel._optimize_parameters_graphed: every step of a capturing model runs on ONE
        # side stream (autograd binds a parameter's AccumulateGrad node to the stream of its first use), inputs live in
        # static buffers, the outputs are the capture's tensors; a change of shape or arena re-captures.
        st = self._graph
        side, cur = st['stream'], torch.cuda.current_stream()
        inputs = {k: getattr(self, k) for k in self._inputs}
        shape = tuple(None if t is None else tuple(t.shape) for t in inputs.values()) + (
            self.optimizer_R.flat_p.data_ptr(), self.optimizer_R.flat_g.data_ptr())
        if st['graph'] is not None and st['shape'] != shape:
            st.update(graph=None, eager_steps=0)
        if st['force_eager'] or (st['graph'] is None and st['eager_steps'] < 2):
            st['eager_steps'] += 1
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                self._forward_backward()
            cur.wait_stream(side)
            return self._apply_updates()
        if st['graph'] is None:
            st['inputs'] = {k: None if t is None else t.clone() for k, t in inputs.items()}
            vars(self).update(st['inputs'])
            for k in self._outputs:                                       # drop the previous step's autograd graph
                v = getattr(self, k, None)
                if torch.is_tensor(v) and v.grad_fn is not None:
                    setattr(self, k, v.detach())
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            ops.begin_graph_capture()
            try:
                with torch.cuda.graph(graph, stream=side):
                    self._forward_backward()
            finally:
                ops.end_graph_capture()
            st['outputs'] = {k: getattr(self, k) for k in self._outputs}
            st.update(graph=graph, shape=shape)
        else:
            for k, buf in st['inputs'].items():
                if buf is not None and inputs[k] is not buf:
                    buf.copy_(inputs[k], non_blocking=True)
            vars(self).update(st['outputs'])
            vars(self).update(st['inputs'])
        st['graph'].replay()
        self._apply_updates()

    def get_current_losses(self):
        return {k: float(getattr(self, 'loss_' + k).detach()) for k, _, _ in self._terms}
