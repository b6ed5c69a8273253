"""GPU parity at module / whole-step level: the host mirror (dfmir_amd.networks / voxelmorph /
registration_model) on the HIP kernels against (a) the golden vectors captured from the reference
and (b) the CPU oracle on the same seeded weights and inputs.  Tolerance 1e-4 relative on outputs
(north_star), 1e-3 on gradients that pass through long reductions / many layers.
"""
import numpy as np
import pytest
import torch

from tests.golden import common as C
from tests.test_gpu_ops import DEV, close, near

pytestmark = pytest.mark.gpu

# element-wise bound on the three north_star outputs at full size (floor: 1e-6 of the tensor's maximum); measured values are
# printed by the tests that use it and kept in profiles/r05_elementwise_error.txt
ELEM_RTOL = 8e-3
# the six losses of a full-size (256 x 256, ngf 64) step against the fp32 CPU oracle; measured values: profiles/r06_parity_margins.txt
LOSS_RTOL_FULL = 1e-3


@pytest.fixture(scope="module")
def O():
    from oracle import dfmir_oracle
    return dfmir_oracle


def _load(dst, src_module):
    """Copy an oracle module's weights into the HIP mirror (same state_dict keys; `grid` buffers
    exist only on the HIP side for checkpoint compatibility)."""
    missing, unexpected = dst.load_state_dict(src_module.state_dict(), strict=False)
    assert not unexpected, unexpected
    assert all(k.endswith(".grid") for k in missing), missing
    from dfmir_amd import ops
    ops.bump_weights_epoch()


def test_resblock_golden(golden, O):
    from dfmir_amd import networks as N
    g = golden("resblock.npz")
    torch.manual_seed(41)
    ob = O.ResBlock(16)
    assert C.state_checksum(ob) == str(g["wsum"])
    hb = N.ResnetBlock(16, 'reflect', N.get_norm_layer('instance'), False, True).to(DEV)
    _load(hb, ob)
    x = C.randn(42, 2, 16, 10, 14).to(DEV).requires_grad_()
    y = hb(x)
    (y * C.randn(43, *y.shape).to(DEV)).sum().backward()
    close(y, g["out"], what="out"); close(x.grad, g["dx"], rtol=3e-4, what="dx")
    close(hb.conv_block[1].weight.grad, g["dw1"], rtol=1e-3, what="dw1")
    close(hb.conv_block[1].bias.grad, g["db1"], rtol=1e-3, atol=1e-4, what="db1")
    close(hb.conv_block[5].weight.grad, g["dw5"], rtol=1e-3, what="dw5")
    close(hb.conv_block[5].bias.grad, g["db5"], rtol=1e-3, atol=1e-4, what="db5")


def test_generator_golden(golden, O):
    from dfmir_amd import networks as N
    from tests.test_oracle_golden import make_tiny_generator
    g = golden("generator.npz")
    og = make_tiny_generator()
    assert C.state_checksum(og) == str(g["wsum"])
    hg = N.define_G(1, 1, 8, 'resnet_9blocks', 'instance', False, 'xavier', 0.02, False, False, [0], None)
    assert sorted(hg.state_dict().keys()) == sorted(og.state_dict().keys())
    _load(hg, og)
    x = C.image_pair(52, 2, 64, 64)[0].to(DEV).requires_grad_()
    y, feats = hg(x, [0, 4, 8, 12, 16], encode_only=False)
    fc = [C.randn(54 + i, *f.shape).to(DEV) for i, f in enumerate(feats)]
    ((y * C.randn(53, *y.shape).to(DEV)).sum() + sum((f * c).sum() for f, c in zip(feats, fc))).backward()
    close(y, g["out"], what="gen out")
    for i, f in enumerate(feats):
        close(f, g["feat%d" % i], what="feat%d" % i)
    close(x.grad, g["dx"], rtol=1e-3, what="gen dx")
    for k, p in hg.named_parameters():
        if k.endswith(".bias") and k != "model.30.bias":
            continue  # a bias in front of InstanceNorm has an exactly-zero true gradient: both sides are rounding noise
        ref = float(g["gnorm_" + k.replace(".", "_")])
        assert abs(float(p.grad.norm()) - ref) <= 2e-3 * max(ref, 1e-6), (k, float(p.grad.norm()), ref)
    enc = hg(x.detach(), [0, 4, 8, 12, 16], encode_only=True)
    assert len(enc) == 5
    close(enc[4], g["feat4"], what="encode_only feat4")
    close(hg(x.detach()), g["out"], what="plain forward")


def test_patch_sampler_golden(golden, O):
    from dfmir_amd import networks as N
    from dfmir_amd.patchnce import PatchNCELoss
    from dfmir_amd.options import default_options
    from dfmir_amd import ops
    from tests.test_oracle_golden import make_patch_sampler
    g = golden("patchnce.npz")
    opf, feats = make_patch_sampler()
    hpf = N.PatchSampleF(use_mlp=True, init_type='xavier', init_gain=0.02, nc=32, gpu_ids=[0])
    hpf.create_mlp([f.to(DEV) for f in feats])
    _load(hpf, opf)
    ids = [C.patch_ids(0, i, f.shape[2] * f.shape[3], 48).to(DEV) for i, f in enumerate(feats)]
    fq = [f.clone().to(DEV).requires_grad_() for f in feats]
    fk = [C.randn(65 + i, *f.shape).to(DEV) for i, f in enumerate(feats)]
    kpool, _ = hpf(fk, 48, ids)
    qpool, rid = hpf(fq, 48, ids)
    assert qpool[1].shape == (2 * 48, 32)
    crit = PatchNCELoss(default_options(batch_size=2))
    tot = 0
    for i, (q, k) in enumerate(zip(qpool, kpool)):
        l = crit(q, k)
        close(l, g["loss%d" % i], what="nce loss %d" % i)
        close(q, g["q%d" % i], what="q%d" % i)
        tot = tot + ops.mean(l)
    tot.backward()
    for i, f in enumerate(fq):
        close(f.grad, g["dfeat%d" % i], rtol=1e-3, what="dfeat%d" % i)
    for k_, p in hpf.named_parameters():
        close(p.grad, g["dparam_" + k_.replace(".", "_")], rtol=1e-3, atol=1e-5, what=k_)


@pytest.mark.parametrize("tag", ["2d", "3d"])
def test_vxm_golden(golden, O, tag):
    from dfmir_amd import voxelmorph as V
    from tests.test_oracle_golden import make_vxm
    g = golden("vxm.npz")
    ov, shp = make_vxm(tag)
    feats_ = O.PLUGIN_UNET_FEATURES if tag == "2d" else None
    hv = V.VxmDense(shp, feats_, int_steps=7, bidir=True).to(DEV)
    _load(hv, ov)
    B = 2 if tag == "2d" else 1
    s_ = C.rand(83, B, 1, *shp).to(DEV).requires_grad_()
    t_ = C.rand(84, B, 1, *shp).to(DEV)
    ys, yt, fl = hv(s_, t_)
    ((ys * C.randn(85, *ys.shape).to(DEV)).sum() + (fl * (C.randn(86, *fl.shape) * 0.1).to(DEV)).sum()).backward()
    close(fl, g["flow_" + tag], what="flow"); close(ys, g["ys_" + tag], what="ys"); close(yt, g["yt_" + tag], what="yt")
    close(s_.grad, g["dsrc_" + tag], rtol=1e-3, what="dsrc")
    close(hv.flow.weight.grad, g["gflow_w_" + tag], rtol=1e-3, what="dflow.w")
    close(hv.unet_model.downarm[0].main.weight.grad, g["gdown0_w_" + tag], rtol=1e-3, what="ddown0.w")
    close(hv.unet_model.uparm[1].main.weight.grad, g["gup1_w_" + tag], rtol=1e-3, what="dup1.w")
    y2, f2 = hv(s_.detach(), t_, registration=True)
    close(y2, g["reg_ys_" + tag], what="registration=True")


def _hip_model_from_oracle(st, size, B, ngf, **opt_kw):
    from dfmir_amd.options import default_options
    from dfmir_amd.registration_model import REGISTRATIONModel
    opt = default_options(batch_size=B, crop_size=size, load_size=size, ngf=ngf, gpu_ids=[0],
                          checkpoints_dir="/tmp/dfmir_ckpt", name="t", **opt_kw)
    model = REGISTRATIONModel(opt)
    _load(model.netG, st.netG)
    _load(model.netR, st.netR)
    return model, opt


class PinnedIds(object):
    """model.patch_id_source for the DEFAULT (batched, device-side) NCE path with the fixture's ids: set t of a call
    with n_sets sets = C.patch_ids(call + t, layer, S, P), `call` advancing as the reference's netF calls do (0, 1 =
    data-dependent init; 2, 3, 4 = step 0; ...).  graph_safe: one static device buffer per (sizes, n_sets, P), filled in
    place; inside a capture nothing is copied -- the owner calls prefill() before every step that may replay."""
    graph_safe = True
    distinct = True          # randperm prefixes

    def __init__(self, device=None):
        self.call = 0
        self.bufs = {}
        self.device = device or DEV
        self.filled = False

    def _ids(self, sizes, n_sets, P):
        ids = torch.stack([torch.stack([C.patch_ids(self.call + t, l, S, P) for t in range(n_sets)])
                           for l, S in enumerate(sizes)])
        self.call += n_sets
        return ids

    def prefill(self, sizes, n_sets, P):
        key = (tuple(int(s) for s in sizes), int(n_sets), int(P))
        ids = self._ids(sizes, n_sets, P)
        if key not in self.bufs:
            self.bufs[key] = ids.to(self.device)
        else:
            self.bufs[key].copy_(ids)
        self.filled = True

    def __call__(self, sizes, n_sets, P):
        key = (tuple(int(s) for s in sizes), int(n_sets), int(P))
        if not self.filled:       # not prefilled: fresh tensors (an earlier call's ids may be saved for its backward)
            assert not torch.cuda.is_current_stream_capturing(), "prefill() before a step that is captured"
            return self._ids(sizes, n_sets, P).to(self.device)
        self.filled = False
        return self.bufs[key]


def nce_sizes(size):
    """H*W of the five tapped layers (0, 4, 8, 12, 16) of ResnetGenerator at size x size."""
    return [(size + 6) ** 2, size ** 2, (size // 2) ** 2, (size // 4) ** 2, (size // 4) ** 2]


@pytest.mark.parametrize("flip", [True, False], ids=["mirrored", "not-mirrored"])
@pytest.mark.parametrize("stacked", [True, False], ids=["stacked-queries", "per-term"])
def test_fastcut_step_vs_oracle(O, flip, stacked):
    """The FastCUT branch of the plugin (registration_model.py:63-67,188-191,241-242): nce_idt False, lambda_NCE 10,
    flip_equivariance -- the generator sees the batch mirrored along W with probability 1/2 (forced here through the
    `flip_draw` hook on both sides) and every NCE term mirrors its query features back.  Two whole steps against the
    oracle: losses, the three outputs, every arena's gradient; the two-term stacked query pass and the per-term calls."""
    size, B, ngf = 64, 2, 8
    torch.manual_seed(5)
    st = O.RegistrationStep(size, B, ngf=ngf, lambda_NCE=10.0, nce_idt=False, flip_equivariance=True)
    st.flip_draw = lambda: flip
    with torch.no_grad():
        st.netR.flow.weight.mul_(1e5)
    st.ids_hook = lambda c, feats: [C.patch_ids(c, i, f.shape[2] * f.shape[3], 256) for i, f in enumerate(feats)]
    A0, B0 = C.image_pair(7, B, size, size)
    st.data_dependent_initialize(A0, B0)
    with torch.no_grad():
        for p in st.netF.parameters():
            if p.dim() == 1:
                p.add_(0.01)
    model, opt = _hip_model_from_oracle(st, size, B, ngf, nce_idt=False, lambda_NCE=10.0, flip_equivariance=True,
                                        batch_query_passes=stacked)
    assert 'NCE_Y' not in model.loss_names
    model.flip_draw = lambda: flip
    model.patch_id_source = PinnedIds()
    model.data_dependent_initialize({"A": A0, "B": B0, "A_paths": [""] * B, "B_paths": [""] * B})
    _load(model.netF, st.netF)
    model.setup(opt)
    model.parallelize()
    for it in range(2):
        A_, B_ = C.image_pair(20 + 2 * it, B, size, size)
        ref = st.step(A_, B_)
        model.set_input({"A": A_, "B": B_, "A_paths": [""] * B, "B_paths": [""] * B})
        model.optimize_parameters()
        assert model.flipped_for_equivariance == flip and st.flipped == flip
        ls = model.get_current_losses()
        for k in ("G", "NCE", "R", "smooth", "local"):
            near(ls[k], ref[k], 3e-4 * (it + 1), "loss %s step %d" % (k, it))
        if it == 0:
            close(model.fake_B, st.fake_B, what="fake_B"); close(model.registered, st.registered, what="registered")
            close(model.pos_flow, st.flow, what="pos_flow"); close(model.regA, st.regA, what="regA")
    if flip:       # the mirrored pass really differs: the translated image is the mirror image of the un-mirrored run's
        assert float((model.fake_B - torch.flip(model.fake_B, [3])).abs().max()) > 1e-3


def test_all_negatives_step_vs_oracle_and_netF_sample(O, golden):
    """opt.nce_includes_all_negatives_from_minibatch (models/patchnce.py:32-38: the whole minibatch is ONE group of
    negatives) through the model's default stacked path -- two whole steps against the oracle (losses, outputs, gradient
    arenas) -- and `--netF sample` (models/networks.py:280-281): the reference builds `torch.optim.Adam` over PatchSampleF's
    empty parameter list in data_dependent_initialize (registration_model.py:134-135) and raises; the mirror raises the same
    error (fixture edges.npz records the reference's message)."""
    size, B, ngf = 64, 2, 8
    torch.manual_seed(6)
    st = O.RegistrationStep(size, B, ngf=ngf, nce_all_negatives=True)
    with torch.no_grad():
        st.netR.flow.weight.mul_(1e5)
    st.ids_hook = lambda c, feats: [C.patch_ids(c, i, f.shape[2] * f.shape[3], 256) for i, f in enumerate(feats)]
    A0, B0 = C.image_pair(9, B, size, size)
    st.data_dependent_initialize(A0, B0)
    with torch.no_grad():
        for p in st.netF.parameters():
            if p.dim() == 1:
                p.add_(0.01)
    model, opt = _hip_model_from_oracle(st, size, B, ngf, nce_includes_all_negatives_from_minibatch=True)
    model.patch_id_source = PinnedIds()
    data = {"A": A0, "B": B0, "A_paths": [""] * B, "B_paths": [""] * B}
    model.data_dependent_initialize(data)
    _load(model.netF, st.netF)
    model.setup(opt)
    model.parallelize()
    for it in range(2):
        A_, B_ = C.image_pair(30 + 2 * it, B, size, size)
        ref = st.step(A_, B_)
        model.set_input({"A": A_, "B": B_, "A_paths": [""] * B, "B_paths": [""] * B})
        model.optimize_parameters()
        assert model._nce_on_device
        ls = model.get_current_losses()
        for k, v in ref.items():
            near(ls[k], v, 3e-4 * (it + 1), "loss %s step %d" % (k, it))
        if it == 0:
            close(model.fake_B, st.fake_B, what="fake_B"); close(model.registered, st.registered, what="registered")
            close(model.pos_flow, st.flow, what="pos_flow")
            for nm, o_, net in (("G", model.optimizer_G, st.netG), ("F", model.optimizer_F, st.netF), ("R", model.optimizer_R, st.netR)):
                # (the oracle's .grad after its step: Adam does not modify them)
                ref_g = torch.cat([p.grad.reshape(-1) for p in net.parameters()])
                got_g = o_.flat_g.cpu()
                rel = float((got_g - ref_g).norm() / ref_g.norm())
                # (F: sums behind the L2 normalisation, cancellation-dominated -- 1.6e-3 measured here; at full size the
                # fp32 CPU oracle itself is 2.8e-3 from an fp64 run on the same rows, test_full_size_gradients_vs_fp64_oracle)
                assert rel <= (4e-3 if nm == "F" else 1e-3), (nm, rel)
    # --netF sample
    g = golden("edges.npz")
    from dfmir_amd.options import default_options
    from dfmir_amd.registration_model import REGISTRATIONModel
    opt2 = default_options(batch_size=B, crop_size=size, load_size=size, ngf=ngf, gpu_ids=[0], netF='sample',
                           checkpoints_dir="/tmp/dfmir_ckpt", name="t")
    m2 = REGISTRATIONModel(opt2)
    with pytest.raises(ValueError) as ei:
        m2.data_dependent_initialize(data)
    assert "ValueError: %s" % ei.value == str(g["netF_sample_optimizer_error"])


@pytest.mark.parametrize("capture", [False, True])
def test_whole_step_golden_default_path(golden, O, capture):
    """Fixture S1 (the reference's own three train steps) through the DEFAULT production path -- device-side batched
    NCE head, stacked query passes, scalar_combine; with capture=True the third step is a hipGraph replay -- ids pinned
    through model.patch_id_source, no netF.forward wrap, no per-term fallback."""
    from tests.test_oracle_golden import make_step
    g = golden("step.npz")
    st, size, B = make_step()
    model, opt = _hip_model_from_oracle(st, size, B, 8)
    opt.capture_step = capture
    src = model.patch_id_source = PinnedIds()
    model.set_dvf_image(torch.from_numpy(g["dvf_image"]))
    A0, B0 = C.image_pair(93, B, size, size)
    model.data_dependent_initialize({"A": A0, "B": B0, "A_paths": [""] * B, "B_paths": [""] * B})
    assert src.call == 2
    _load(model.netF, st.netF)
    model.setup(opt)
    model.parallelize()
    for it in range(3):
        A_, B_ = C.image_pair(100 + 2 * it, B, size, size)
        src.prefill(nce_sizes(size), 3, opt.num_patches)
        model.set_input({"A": A_, "B": B_, "A_paths": [""] * B, "B_paths": [""] * B})
        model.optimize_parameters()
        assert model._nce_on_device and 'forward' not in vars(model.netF)
        ls = model.get_current_losses()
        got = np.array([ls[k] for k in ("G", "NCE", "R", "smooth", "local", "NCE_Y")])
        np.testing.assert_allclose(got, g["losses_%d" % it], rtol=3e-4 * (it + 1), atol=1e-6, err_msg="step %d" % it)
        if it == 0:
            close(model.fake_B, g["fake_B"], what="fake_B"); close(model.registered, g["registered"], what="registered")
            close(model.regA, g["regA"], what="regA"); close(model.idt_B, g["idt_B"], what="idt_B")
            close(model.pos_flow, g["pos_flow"], what="pos_flow")      # the deformation field, against the reference's own
            close(model.dvf, g["dvf"], what="dvf")
            for nm, o_ in (("G", model.optimizer_G), ("F", model.optimizer_F), ("R", model.optimizer_R)):
                n2 = float(o_.flat_g.double().pow(2).sum().sqrt())
                ref = float(g["gradnorm_" + nm])
                assert abs(n2 - ref) <= 2e-3 * ref, (nm, n2, ref)
    assert src.call == 2 + 9
    if capture:
        assert model._graph['graph'] is not None, "the third step must have been a hipGraph replay"


def test_trajectory_drift_vs_fp64_oracle(O):
    """Parity over an optimizer TRAJECTORY: five consecutive train steps (fresh image pair each step, patch ids pinned, three
    Adam updates per step; steps 3.. are replays of one captured hipGraph) of the default production path, next to the CPU
    oracle in fp32 AND in fp64 from the same weights.  Early training with Adam is a sensitive system (updates of size lr
    whatever the gradient's size, and every ReLU / mask decision that sits on a rounding boundary changes one image's
    gradient by 0.1-3 %: scripts/diag/diag_dfake.py shows such flips in the fp32 oracle as well as in the HIP path, in different
    images): the fp32 oracle itself leaves the fp64 trajectory -- 1e-4 relative at step 3, 1.4 % at the loss spike of step 5.
    So the bound is the sum of the drift the reference-generated three-step fixture S1 allows (3e-4 x (step + 1) relative) and
    3x the fp32 oracle's own distance from the fp64 trajectory at that step (round 6, five runs: every loss of every step
    inside the S1 floor alone, worst |HIP - fp64| = 0.75 of it at step 5 -- the second term is head-room for the run-to-run
    noise of the weight gradients' float atomics through Adam; it was 12x until round 5.  Round 4 had measured HIP 1.0e-3 at
    step 3 where fp32 has 1.4e-4, 5 % at step 5 where fp32 has 1.4 %; scripts/diag/diag_first_update.py, diag_gen_grads.py, diag_nce_precision.py and
    diag_nce_term.py put the generator, the NCE head and a single NCE term in isolation at 1.2-2x fp32 PyTorch's error)."""
    size, B, steps = 64, 2, 5          # up to, not into, the oracle's own loss spike at step 5 (fp32 vs fp64: 1.4 % there)

    def make(double):
        torch.manual_seed(11)
        st = O.RegistrationStep(size, B, ngf=8)
        with torch.no_grad():
            st.netR.flow.weight.mul_(1e5)                  # a flow field that moves pixels (the init is N(0, 1e-5))
        st.ids_hook = lambda c, feats: [C.patch_ids(c, i, f.shape[2] * f.shape[3], 256) for i, f in enumerate(feats)]
        A0, B0 = C.image_pair(7, B, size, size)
        st.data_dependent_initialize(A0, B0)
        with torch.no_grad():
            for p in st.netF.parameters():
                if p.dim() == 1:
                    p.add_(0.01)                           # biases off zero: Normalize's gradient is regular on both sides
        if double:
            for m in (st.netG, st.netF, st.netR):
                m.double()                                 # in place: the optimizers keep their parameter objects
        return st, A0, B0

    s64, _, _ = make(True)
    st, A0, B0 = make(False)
    model, opt = _hip_model_from_oracle(st, size, B, 8)
    opt.capture_step = True
    src = model.patch_id_source = PinnedIds()
    model.data_dependent_initialize({"A": A0, "B": B0, "A_paths": [""] * B, "B_paths": [""] * B})
    _load(model.netF, st.netF)
    model.setup(opt)
    model.parallelize()
    worst, worst_floor, rows = 0.0, 0.0, []
    for it in range(steps):
        A_, B_ = C.image_pair(300 + 2 * it, B, size, size)
        r32 = st.step(A_, B_)
        r64 = s64.step(A_.double(), B_.double())
        src.prefill(nce_sizes(size), 3, opt.num_patches)
        model.set_input({"A": A_, "B": B_, "A_paths": [""] * B, "B_paths": [""] * B})
        model.optimize_parameters()
        got = model.get_current_losses()
        for k, v in r64.items():
            e_hip, e_32 = abs(got[k] - v), abs(r32[k] - v)
            floor = 3e-4 * (it + 1) * max(abs(v), 1e-3)
            worst = max(worst, (e_hip - floor) / max(e_32, 1e-12) if e_hip > floor else 0.0)
            worst_floor = max(worst_floor, e_hip / floor)
            rows.append((it, k, got[k], r32[k], v))
            assert e_hip <= 3.0 * e_32 + floor, "step %d loss %s: HIP %.6f fp32 oracle %.6f fp64 oracle %.6f" % (it, k, got[k], r32[k], v)
    assert model._graph['graph'] is not None, "steps 3.. must have been hipGraph replays"
    print("\n  trajectory: worst (|HIP - fp64| - floor) / |fp32 - fp64| over %d steps x 6 losses = %.1f; worst |HIP - fp64| / floor = %.2f"
          % (steps, worst, worst_floor))
    for it, k, a, b, c in rows:
        if k in ("G", "R"):
            print("    step %d %-3s HIP %.6f  fp32 %.6f  fp64 %.6f" % (it, k, a, b, c))


def test_whole_step_golden(golden, O):
    """Config 1 geometry (64x64, batch 2): 3 consecutive train steps against the reference's own
    losses / outputs (fixture S1), patch ids pinned."""
    from tests.test_oracle_golden import make_step
    g = golden("step.npz")
    st, size, B = make_step()          # oracle with the fixture's seeded weights (post data-dependent init)
    assert C.multi_state_checksum((st.netG, st.netF, st.netR)) == str(g["wsum"])
    model, opt = _hip_model_from_oracle(st, size, B, 8)
    call = [0]
    base_forward = model.netF.forward

    def netF_forward(feats, num_patches=64, patch_ids=None):
        if patch_ids is None:
            patch_ids = [C.patch_ids(call[0], i, f.shape[2] * f.shape[3], 256).to(DEV) for i, f in enumerate(feats)]
            call[0] += 1
        return base_forward(feats, num_patches, patch_ids)

    model.netF.forward = netF_forward
    model.set_dvf_image(torch.from_numpy(g["dvf_image"]))     # the decoded ./deform256.jpg window the reference warped
    A0, B0 = C.image_pair(93, B, size, size)
    model.data_dependent_initialize({"A": A0, "B": B0, "A_paths": [""] * B, "B_paths": [""] * B})
    _load(model.netF, st.netF)
    model.setup(opt)
    model.parallelize()
    for it in range(3):
        A_, B_ = C.image_pair(100 + 2 * it, B, size, size)
        model.set_input({"A": A_, "B": B_, "A_paths": [""] * B, "B_paths": [""] * B})
        model.optimize_parameters()
        ls = model.get_current_losses()
        got = np.array([ls[k] for k in ("G", "NCE", "R", "smooth", "local", "NCE_Y")])
        np.testing.assert_allclose(got, g["losses_%d" % it], rtol=3e-4 * (it + 1), atol=1e-6, err_msg="step %d" % it)
        if it == 0:
            close(model.fake_B, g["fake_B"], what="fake_B"); close(model.registered, g["registered"], what="registered")
            close(model.regA, g["regA"], what="regA"); close(model.idt_B, g["idt_B"], what="idt_B")
            close(model.pos_flow, g["pos_flow"], what="pos_flow")      # the deformation field, against the reference's own
            close(model.dvf, g["dvf"], what="dvf")                # row A12, against the reference's own visual
            for nm, o_ in (("G", model.optimizer_G), ("F", model.optimizer_F), ("R", model.optimizer_R)):
                n2 = float(o_.flat_g.double().pow(2).sum().sqrt())
                ref = float(g["gradnorm_" + nm])
                assert abs(n2 - ref) <= 2e-3 * ref, (nm, n2, ref)
    vis = model.get_current_visuals()
    assert list(vis.keys()) == ['real_A', 'fake_B', 'real_B', 'dvf', 'registered', 'regA', 'idt_B']
    assert vis['dvf'].shape == (B, 3, size, size)


def test_key_feature_reuse_is_bit_identical(O):
    """forward() taps the key-side encoder features instead of re-running the encoder three times
    (registration_model.py:244): losses, gradients and updated weights must not change by one bit."""
    from tests.test_oracle_golden import make_step
    res = []
    for reuse in (True, False):
        st, size, B = make_step()
        model, opt = _hip_model_from_oracle(st, size, B, 8)
        opt.reuse_key_features = reuse
        base_forward = model.netF.forward
        call = [0]

        def netF_forward(feats, num_patches=64, patch_ids=None, base_forward=base_forward, call=call):
            if patch_ids is None:
                patch_ids = [C.patch_ids(call[0], i, f.shape[2] * f.shape[3], 256).to(DEV) for i, f in enumerate(feats)]
                call[0] += 1
            return base_forward(feats, num_patches, patch_ids)

        model.netF.forward = netF_forward
        A0, B0 = C.image_pair(93, B, size, size)
        model.data_dependent_initialize({"A": A0, "B": B0, "A_paths": [""] * B, "B_paths": [""] * B})
        _load(model.netF, st.netF)
        model.setup(opt)
        model.parallelize()
        A_, B_ = C.image_pair(100, B, size, size)
        model.set_input({"A": A_, "B": B_, "A_paths": [""] * B, "B_paths": [""] * B})
        model.optimize_parameters()
        assert (model._key_feats is not None) == reuse
        res.append(([v for v in model.get_current_losses().values()], [o_.flat_g.clone() for o_ in model.optimizers]))
        if reuse:   # the tapped activations are the encoder's, bit for bit (forward kernels hold no atomics)
            with torch.no_grad():
                model.forward()   # re-tap with the weights as they are now
                for owner, feats in model._key_feats:
                    again = model.netG(owner, model.nce_layers, encode_only=True)
                    assert len(again) == len(feats)
                    for f0, f1 in zip(feats, again):
                        assert torch.equal(f0, f1)
    # the step's losses are identical; its gradients differ only by the float-atomic ordering noise of the
    # warp backward (one step only: Adam's g/sqrt(v) turns that noise into lr-sized differences later)
    np.testing.assert_allclose(res[0][0], res[1][0], rtol=1e-6)   # loss sums reduce through float atomics
    for a, b in zip(res[0][1], res[1][1]):
        assert float((a - b).norm()) <= 1e-5 * float(b.norm())


def test_stacked_query_passes_match_sequential(O):
    """The three NCE terms' query batches through ONE encoder pass (stacked along the batch, grouped patch ids) give
    the losses and gradients of the reference's three passes (registration_model.py:213-253, 163)."""
    from tests.test_oracle_golden import make_step
    res = []
    for stacked in (True, False):
        st, size, B = make_step()
        model, opt = _hip_model_from_oracle(st, size, B, 8)
        opt.batch_query_passes = stacked
        base_forward = model.netF.forward
        call = [0]

        def netF_forward(feats, num_patches=64, patch_ids=None, base_forward=base_forward, call=call):
            if patch_ids is None:
                patch_ids = [C.patch_ids(call[0], i, f.shape[2] * f.shape[3], 256).to(DEV) for i, f in enumerate(feats)]
                call[0] += 1
            return base_forward(feats, num_patches, patch_ids)

        model.netF.forward = netF_forward
        A0, B0 = C.image_pair(93, B, size, size)
        model.data_dependent_initialize({"A": A0, "B": B0, "A_paths": [""] * B, "B_paths": [""] * B})
        _load(model.netF, st.netF)
        model.setup(opt)
        model.parallelize()
        A_, B_ = C.image_pair(100, B, size, size)
        model.set_input({"A": A_, "B": B_, "A_paths": [""] * B, "B_paths": [""] * B})
        model.optimize_parameters()
        res.append(([v for v in model.get_current_losses().values()], [o_.flat_g.clone() for o_ in model.optimizers]))
    np.testing.assert_allclose(res[0][0], res[1][0], rtol=2e-6)
    for a, b in zip(res[0][1], res[1][1]):
        assert float((a - b).norm()) <= 2e-5 * float(b.norm())


def test_graph_captured_step_matches_eager(O):
    """opt.capture_step: two eager steps, then the step is captured as one hipGraph and replayed.  Every replayed step
    is checked against the SAME step enqueued eagerly from the same state (weights, Adam moments, patch-id generator
    restored in between): same kernels on the same data, so losses, outputs and gradient arenas agree to the noise of
    the float atomics.  (Two independent training runs cannot be compared this tightly: Adam turns that noise into
    lr-sized steps on ill-conditioned weights, and lr = 2e-4 is 10 % of a weight's standard deviation here.)"""
    from dfmir_amd import ops
    from tests.test_oracle_golden import make_step
    st, size, B = make_step()
    model, opt = _hip_model_from_oracle(st, size, B, 8)
    opt.capture_step = True
    ids_state = ops.seed_patch_ids(4242, DEV)
    A0, B0 = C.image_pair(93, B, size, size)
    base_forward = model.netF.forward
    model.netF.forward = lambda feats, num_patches=64, patch_ids=None, bf=base_forward: bf(
        feats, num_patches, patch_ids if patch_ids is not None else
        [C.patch_ids(0, i, f.shape[2] * f.shape[3], 256).to(DEV) for i, f in enumerate(feats)])
    model.data_dependent_initialize({"A": A0, "B": B0, "A_paths": [""] * B, "B_paths": [""] * B})
    del model.netF.forward
    _load(model.netF, st.netF)
    model.setup(opt)
    model.parallelize()

    def snapshot():
        return ([(o_.flat_p.clone(), o_.exp_avg.clone(), o_.exp_avg_sq.clone(), o_._steps) for o_ in model.optimizers],
                ids_state.clone())

    def restore(snap):
        for o_, (p, m, v, n) in zip(model.optimizers, snap[0]):
            o_.flat_p.copy_(p); o_.exp_avg.copy_(m); o_.exp_avg_sq.copy_(v); o_._steps = n
        ids_state.copy_(snap[1])
        ops.bump_weights_epoch()

    def observe():
        return (list(model.get_current_losses().values()), model.fake_B.clone(), model.registered.clone(), model.dvf.clone(),
                [o_.flat_g.clone() for o_ in model.optimizers], [o_.flat_p.clone() for o_ in model.optimizers])

    prev_fake = None
    for it in range(6):
        A_, B_ = C.image_pair(200 + 2 * it, B, size, size)
        data = {"A": A_.to(DEV), "B": B_.to(DEV), "A_paths": [""] * B, "B_paths": [""] * B}
        snap = snapshot()
        model._graph_state()['force_eager'] = True
        model.set_input(data)
        model.optimize_parameters()
        ref = observe()
        model._graph_state()['force_eager'] = False
        restore(snap)
        model.set_input(data)
        model.optimize_parameters()
        got = observe()
        if it >= 2:
            assert model._graph['graph'] is not None          # captured on the third step, replayed from then on
        np.testing.assert_allclose(got[0], ref[0], rtol=1e-5, atol=1e-9, err_msg="losses, step %d" % it)
        close(got[1], ref[1], rtol=1e-6, what="fake_B step %d" % it)
        close(got[2], ref[2], rtol=1e-6, what="registered step %d" % it)
        close(got[3], ref[3], rtol=1e-6, what="dvf step %d" % it)
        gscale = max(float(g.norm()) for g in ref[4])
        for nm, a, b in zip("GRF", got[4], ref[4]):
            assert float((a - b).norm()) <= 2e-5 * float(b.norm()) + 2e-6 * gscale, (it, nm)
        if prev_fake is not None:
            assert not torch.equal(got[1], prev_fake)          # replays see new inputs and new weights
        prev_fake = got[1]
    assert model._graph['eager_steps'] >= 2


def test_failed_capture_falls_back_to_a_correct_eager_step(O):
    """A capture that raises has recorded the batched weight re-pack and the probe pool's zero fill without running them
    while the host caches were updated as if they had run (round-3 advisor finding): the eager step that follows must
    invalidate them.  The third step's capture is made to raise after all of the step has been recorded; that step and
    the next are compared with the same steps of a forced-eager run from the same state."""
    import warnings
    from dfmir_amd import ops
    from tests.test_oracle_golden import make_step
    st, size, B = make_step()
    model, opt = _hip_model_from_oracle(st, size, B, 8)
    opt.capture_step = True
    # deterministic weight gradients: with fp32 atomics the two runs differ by summation order, step 3's round-off goes
    # through Adam and PatchNCE's softmax (T = 0.07), and step 4's gradients have been seen 9.5e-4 of their norm apart
    # (1 of 3 full-suite runs) -- too close to what a stale weight pack would do.  In fixed point the comparison is sharp.
    ops.set_deterministic_wgrad(True)
    try:
        _failed_capture_body(O, ops, st, size, B, model, opt, make_step)
    finally:
        ops.set_deterministic_wgrad(False)


def _failed_capture_body(O, ops, st, size, B, model, opt, make_step):
    import warnings
    ids_state = ops.seed_patch_ids(777, DEV)
    A0, B0 = C.image_pair(93, B, size, size)
    base_forward = model.netF.forward
    model.netF.forward = lambda feats, num_patches=64, patch_ids=None, bf=base_forward: bf(
        feats, num_patches, patch_ids if patch_ids is not None else
        [C.patch_ids(0, i, f.shape[2] * f.shape[3], 256).to(DEV) for i, f in enumerate(feats)])
    model.data_dependent_initialize({"A": A0, "B": B0, "A_paths": [""] * B, "B_paths": [""] * B})
    del model.netF.forward
    _load(model.netF, st.netF)
    model.setup(opt)
    model.parallelize()
    batches = []
    for it in range(4):
        A_, B_ = C.image_pair(300 + 2 * it, B, size, size)
        batches.append({"A": A_.to(DEV), "B": B_.to(DEV), "A_paths": [""] * B, "B_paths": [""] * B})

    def run(data):
        model.set_input(data)
        model.optimize_parameters()
        torch.cuda.synchronize()
        return (list(model.get_current_losses().values()), model.fake_B.clone(), model.registered.clone(),
                [o_.flat_g.clone() for o_ in model.optimizers], [o_.flat_p.clone() for o_ in model.optimizers])

    for it in range(2):
        run(batches[it])
    snap = ([(o_.flat_p.clone(), o_.exp_avg.clone(), o_.exp_avg_sq.clone(), o_._steps) for o_ in model.optimizers],
            ids_state.clone())
    # reference: steps 3 and 4 enqueued eagerly
    model._graph_state()['force_eager'] = True
    ref = [run(batches[2]), run(batches[3])]
    model._graph_state()['force_eager'] = False
    for o_, (p_, m_, v_, n_) in zip(model.optimizers, snap[0]):
        o_.flat_p.copy_(p_); o_.exp_avg.copy_(m_); o_.exp_avg_sq.copy_(v_); o_._steps = n_
    ids_state.copy_(snap[1])
    ops.bump_weights_epoch()
    # now the capture of step 3 records everything and then raises
    real_fb = model._forward_backward

    def failing_fb():
        real_fb()
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("injected capture failure")
    model._forward_backward = failing_fb
    real_pieces = model._step_pieces                     # the staged step (default): its last piece raises while it is captured

    def failing_pieces():
        ps = real_pieces()
        name, sk, fn, after = ps[-1]

        def fin():
            fn()
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("injected capture failure")
        return ps[:-1] + [(name, sk, fin, after)]
    model._step_pieces = failing_pieces
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = [run(batches[2])]
    assert any("capturing the train step failed" in str(x.message) for x in w)
    assert model._graph['force_eager'] and model._graph['graph'] is None
    got.append(run(batches[3]))
    for k, (g_, r_) in enumerate(zip(got, ref)):
        np.testing.assert_allclose(g_[0], r_[0], rtol=1e-5, atol=1e-9, err_msg="losses, step %d" % (k + 3))
        close(g_[1], r_[1], rtol=1e-6, what="fake_B step %d" % (k + 3))
        close(g_[2], r_[2], rtol=1e-6, what="registered step %d" % (k + 3))
        gscale = max(float(x.norm()) for x in r_[3])
        # step 4 starts from weights that already differ by the float-atomic round-off of step 3's weight gradients through
        # Adam (see below): its gradients differ by up to 4e-5 of their norm (2 of 30 runs exceeded the step-3 bound);
        # a stale packed weight or a garbage probe pool is a 1e-2 .. 1 effect
        gtol = 2e-5 if k == 0 else 1e-4
        for nm, a, b in zip("GRF", g_[3], r_[3]):
            err = float((a - b).norm())
            assert err <= gtol * float(b.norm()) + 0.1 * gtol * gscale, (k, nm)
            # ... and in fixed point the fallback's gradients are the eager run's, bit for bit (6 of 6 runs)
            assert torch.equal(a, b), "step %d: gradient arena %s differs from the eager run by %.3e" % (k + 3, nm, err)
        if k == 0:
            # weights after step 3's Adam update: round-off of the weight gradients' float atomics becomes lr-sized
            # differences on elements whose gradient is at round-off level (0.4 % of the update's norm measured); stale
            # packed weights or a garbage probe pool would be a different step altogether
            for nm, a, b in zip("GRF", g_[4], r_[4]):
                assert float((a - b).norm()) <= 2e-3 * float(b.norm()), (k, nm)


class FixedIds(object):
    """model.patch_id_source that returns the SAME id sets at every call (the device generator advances per draw)."""
    graph_safe = False
    distinct = True

    def __call__(self, sizes, n_sets, P):
        return torch.stack([torch.stack([C.patch_ids(7 + t, l, S, P) for t in range(n_sets)]) for l, S in enumerate(sizes)]).to(DEV)


@pytest.mark.parametrize("cfg", [(64, 2, 8), (256, 16, 64)], ids=["64-b2-ngf8", "256-b16-ngf64(configs[1])"])
def test_deterministic_weight_gradients(cfg):
    """opt.deterministic_wgrad (build-defined): every weight / bias gradient accumulated as 64-bit fixed-point integers
    (include/dfmir_hip.h "Deterministic weight gradients").  Forward + backward twice from the same weights, inputs and
    patch ids: the three gradient arenas are BIT-identical (SHA-1), and within round-off of the default float-atomic path."""
    import hashlib
    from dfmir_amd import ops
    from dfmir_amd.options import default_options
    from dfmir_amd.registration_model import REGISTRATIONModel
    size, B, ngf = cfg
    res = {}
    try:
        for det in (True, False):
            torch.manual_seed(17)
            opt = default_options(batch_size=B, crop_size=size, load_size=size, ngf=ngf, gpu_ids=[0], deterministic_wgrad=det,
                                  checkpoints_dir="/tmp/dfmir_ckpt", name="det")
            model = REGISTRATIONModel(opt)
            assert ops._DET["on"] == det
            with torch.no_grad():
                model.netR.flow.weight.mul_(1e5)
            model.patch_id_source = FixedIds()
            A0, B0 = C.image_pair(61, B, size, size)
            data = {"A": A0.to(DEV), "B": B0.to(DEV), "A_paths": [""] * B, "B_paths": [""] * B}
            model.data_dependent_initialize(data)
            model.setup(opt)
            model.parallelize()
            runs = []
            for _ in range(2):
                model.set_input(data)
                model._forward_backward()
                torch.cuda.synchronize()
                runs.append([o_.flat_g.clone() for o_ in model.optimizers])
            res[det] = runs
            del model
    finally:
        ops.set_deterministic_wgrad(False)
    sha = lambda t: hashlib.sha1(t.cpu().numpy().tobytes()).hexdigest()
    for nm, a, b in zip("GRF", res[True][0], res[True][1]):
        assert float(a.abs().sum()) > 0
        assert sha(a) == sha(b), "arena %s differs between two deterministic runs" % nm
    for nm, a, b in zip("GRF", res[True][0], res[False][0]):
        assert float((a - b).norm()) <= 2e-5 * float(b.norm()), (nm, float((a - b).norm() / b.norm()))


def test_deterministic_weight_gradients_3d():
    """The same for the 3-D step (every 3-D weight-gradient kernel: tiled, plane-pair, marching, parity-class, first level,
    flow head; NCC's reduction in index order): two backward passes from one state give bit-identical arenas."""
    import hashlib
    from dfmir_amd import ops
    from dfmir_amd.registration3d import Registration3DModel
    res = {}
    try:
        for shape, feats in (((32, 64, 64), None), ((64, 64, 64), "plugin")):
            from oracle import dfmir_oracle as O_
            for det in (True, False):
                torch.manual_seed(23)
                m = Registration3DModel(shape, O_.PLUGIN_UNET_FEATURES if feats else None, device=DEV, deterministic_wgrad=det)
                with torch.no_grad():
                    m.netR.flow.weight.mul_(3e4)
                A = C.rand(31, 1, 1, *shape).to(DEV)
                B = (0.5 * A + 0.5 * C.rand(41, 1, 1, *shape).to(DEV))
                runs = []
                for _ in range(2):
                    m.set_input({"A": A, "B": B})
                    m._forward_backward()
                    torch.cuda.synchronize()
                    runs.append(m.optimizer_R.flat_g.clone())
                res[(shape, det)] = runs
            a, b = res[(shape, True)]
            assert float(a.abs().sum()) > 0
            assert hashlib.sha1(a.cpu().numpy().tobytes()).hexdigest() == hashlib.sha1(b.cpu().numpy().tobytes()).hexdigest(), shape
            c = res[(shape, False)][0]
            assert float((a - c).norm()) <= 2e-5 * float(c.norm()), (shape, float((a - c).norm() / c.norm()))
    finally:
        ops.set_deterministic_wgrad(False)


def _full_size_oracle(O, B, double=False):
    """256x256, ngf 64 oracle step state with seeded weights, pinned ids, a non-vacuous flow head; optionally fp64."""
    size = 256
    torch.manual_seed(7)
    st = O.RegistrationStep(size, B, ngf=64)
    with torch.no_grad():
        st.netR.flow.weight.mul_(1e5)
        st.netR.flow.bias.copy_(C.randn(8, 2) * 1.0)
    st.ids_hook = lambda c, feats: [C.patch_ids(c, i, f.shape[2] * f.shape[3], 256) for i, f in enumerate(feats)]
    A0, B0 = C.image_pair(9, B, size, size)
    st.data_dependent_initialize(A0, B0)
    with torch.no_grad():
        for p in st.netF.parameters():
            if p.dim() == 1:
                p.add_(0.01)
    if double:
        for net in (st.netG, st.netF, st.netR):
            net.double()
        mk = lambda net: torch.optim.Adam(net.parameters(), lr=st.lr, betas=st.betas)
        st.opt_G, st.opt_R, st.opt_F = mk(st.netG), mk(st.netR), mk(st.netF)
    return st, size, A0, B0


def _full_size_hip(st, size, B, A0, B0, default_path=False):
    model, opt = _hip_model_from_oracle(st, size, B, 64)
    if default_path:       # the production NCE head (batched, device-side), ids pinned through the model's hook
        model.patch_id_source = PinnedIds()
        paths = [""] * B
        model.data_dependent_initialize({"A": A0, "B": B0, "A_paths": paths, "B_paths": paths})
        _load(model.netF, st.netF)
        model.setup(opt)
        return model
    call = [0]
    base_forward = model.netF.forward

    def netF_forward(feats, num_patches=64, patch_ids=None):
        if patch_ids is None:
            patch_ids = [C.patch_ids(call[0], i, f.shape[2] * f.shape[3], 256).to(DEV) for i, f in enumerate(feats)]
            call[0] += 1
        return base_forward(feats, num_patches, patch_ids)

    model.netF.forward = netF_forward
    paths = [""] * B
    model.data_dependent_initialize({"A": A0, "B": B0, "A_paths": paths, "B_paths": paths})
    _load(model.netF, st.netF)
    model.setup(opt)
    return model


def test_config0_geometry_at_full_width(O):
    """BASELINE configs[0] -- 64 x 64 pairs, batch 2 -- at the generator's real width (ngf 64: 16 x 16 maps with 256
    channels through the flat-run `pp` kernel, the NCE head on 4 x 4 ... 64 x 64 feature maps with P = 256 of S = 256
    positions at the deepest layers), one whole step against the oracle."""
    size, B, ngf = 64, 2, 64
    torch.manual_seed(13)
    st = O.RegistrationStep(size, B, ngf=ngf)
    with torch.no_grad():
        st.netR.flow.weight.mul_(1e5)
    st.ids_hook = lambda c, feats: [C.patch_ids(c, i, f.shape[2] * f.shape[3], 256) for i, f in enumerate(feats)]
    A0, B0 = C.image_pair(15, B, size, size)
    st.data_dependent_initialize(A0, B0)
    with torch.no_grad():
        for p in st.netF.parameters():
            if p.dim() == 1:
                p.add_(0.01)
    model, opt = _hip_model_from_oracle(st, size, B, ngf)
    model.patch_id_source = PinnedIds()
    model.data_dependent_initialize({"A": A0, "B": B0, "A_paths": [""] * B, "B_paths": [""] * B})
    _load(model.netF, st.netF)
    model.setup(opt)
    model.parallelize()
    A_, B_ = C.image_pair(17, B, size, size)
    ref = st.step(A_, B_)
    model.set_input({"A": A_, "B": B_, "A_paths": [""] * B, "B_paths": [""] * B})
    model.optimize_parameters()
    ls = model.get_current_losses()
    close(model.fake_B, st.fake_B, what="fake_B"); close(model.regA, st.regA, what="regA")
    close(model.registered, st.registered, what="registered"); close(model.pos_flow, st.flow, what="pos_flow")
    for k in ("G", "NCE", "R", "smooth", "local", "NCE_Y"):
        near(ls[k], ref[k], LOSS_RTOL_FULL, "loss " + k)


@pytest.mark.parametrize("default_path", [False, True], ids=["per-term-keys", "default-batched-head"])
def test_full_size_step_vs_oracle(O, default_path, capsys):
    """256x256, ngf=64 (BASELINE configs[1] geometry) at batch 2: one step of the HIP path against the oracle on
    identical seeded weights -- outputs within 1e-4 relative, losses within 1e-3.  Both NCE-head routes: the per-term
    key calls a wrapped netF.forward selects, and the default batched device-side head (ids through patch_id_source)."""
    B = 2
    st, size, A0, B0 = _full_size_oracle(O, B)
    model = _full_size_hip(st, size, B, A0, B0, default_path)
    A_, B_ = C.image_pair(11, B, size, size)
    ref = st.step(A_, B_)
    model.set_input({"A": A_, "B": B_, "A_paths": [""] * B, "B_paths": [""] * B})
    model.optimize_parameters()
    ls = model.get_current_losses()
    # the three outputs north_star names -- translated image, deformation field, warped moving image -- norm-wise AND
    # element-wise (99.9 % of the elements within ELEM_RTOL of max(|ref_i|, 1e-6 max|ref|), every element within 1: see
    # tests/test_gpu_ops.py::close); the other tensors norm-wise
    close(model.fake_B, st.fake_B, what="fake_B", elem_rtol=ELEM_RTOL); close(model.regA, st.regA, what="regA")
    close(model.registered, st.registered, what="registered", elem_rtol=ELEM_RTOL); close(model.idt_B, st.idt_B, what="idt_B")
    close(model.pos_flow, st.flow, what="pos_flow", elem_rtol=ELEM_RTOL)
    with capsys.disabled():
        from tests.test_gpu_ops import ELEMENTWISE
        for row in ELEMENTWISE[-3:]:
            print("\n  %-10s norm-wise %.2e   element-wise max %.2e  99.9%% %.2e  median %.2e" % row, end="")
    for k in ("G", "NCE", "R", "smooth", "local", "NCE_Y"):
        near(ls[k], ref[k], LOSS_RTOL_FULL, "loss " + k)
    moved = (model.netG.state_dict()["model.12.conv_block.1.weight"].cpu() - st.netG.state_dict()["model.12.conv_block.1.weight"]).abs().max()
    assert float(moved) <= 2.0 * 2e-4 * 1.001   # both took one Adam step of size <= lr


def test_full_size_gradients_vs_fp64_oracle(O, capsys):
    """The step's gradients at 256x256, ngf 64 (batch 1), arbitrated by an fp64 run of the oracle: the HIP path's
    distance to the fp64 gradient is compared with the fp32 CPU oracle's own distance to it, parameter by parameter.
    A ~60-op-deep fp32 backward differs from fp64 wherever a ReLU / mask decision sits on a rounding boundary, so
    the yardstick is what plain fp32 PyTorch achieves, not zero.  (Replaces a 2e-2 / cos 0.9995 comparison between
    the two fp32 implementations.)"""
    B = 1
    st32, size, A0, B0 = _full_size_oracle(O, B)
    st64, _, _, _ = _full_size_oracle(O, B, double=True)
    model = _full_size_hip(st32, size, B, A0, B0)
    A_, B_ = C.image_pair(11, B, size, size)
    st32.step(A_, B_)
    st64.step(A_.double(), B_.double())
    model.set_input({"A": A_, "B": B_, "A_paths": [""], "B_paths": [""]})
    model.optimize_parameters()
    rows = []
    fmax = max(float(p.grad.abs().max()) for p in st64.netF.parameters())
    for tag, n32, n64, nh in (("G", st32.netG, st64.netG, model.netG), ("R", st32.netR, st64.netR, model.netR),
                              ("F", st32.netF, st64.netF, model.netF)):
        for (k, p32), (_, p64), (k2, ph) in zip(n32.named_parameters(), n64.named_parameters(), nh.named_parameters()):
            assert k == k2
            if tag == "G" and k.endswith(".bias") and k != "model.30.bias":
                continue  # zero true gradient (bias in front of InstanceNorm)
            if tag == "F" and float(p64.grad.abs().max()) <= 1e-3 * fmax:
                continue  # cancellation-dominated sums behind the L2 normalisation
            g64 = p64.grad.flatten()
            e_cpu = float((p32.grad.double().flatten() - g64).norm() / g64.norm())
            e_hip = float((ph.grad.detach().cpu().double().flatten() - g64).norm() / g64.norm())
            rows.append((e_hip, e_cpu, tag + "." + k))
    worst = sorted(rows, key=lambda r: -r[0] / (r[1] + 1e-12))[:8] + sorted(rows, reverse=True)[:8]
    with capsys.disabled():
        print("\n  rel. L2 error vs the fp64 gradient (HIP, fp32 CPU oracle): worst ratios, then worst absolute")
        for e_hip, e_cpu, k in worst:
            print("    %-44s %.2e   %.2e" % (k, e_hip, e_cpu))
    # What the per-layer ratio measures (round 4, profiles/r04_relu_flips.txt, r04_wgrad_precision.txt, r04_forward_error.txt):
    # a gradient's distance to fp64 is set by the handful of ReLU decisions behind InstanceNorm that land on the other
    # side of zero -- 12 of 18.9 M on the HIP path, 8 for fp32 PyTorch, in different layers: ONE flip moves the weight
    # gradient of the conv in front of it by ~1 / sqrt(2 M) = 7e-4, the size of every entry in this table.  The per-layer
    # ratio is therefore a lottery with a few tickets per layer (model.19.conv_block.1: 3 flips HIP vs 0 CPU -> 5.7x;
    # model.14.conv_block.1: 0 vs 3 -> 0.5x), and it does NOT depend on the operand split: DFMIR_CONV_FP32=1 (exact fp32
    # products) and DFMIR_NO_CH_SCALE give the same table.  What is systematic is a factor ~2 in the forward activations'
    # distance to fp64 (one fp32 accumulation chain over K = 2304 per output: 5e-7 per conv against mkldnn's blocked
    # 1.7e-7), hence ~1.5x the flips.  Bounds: the GEOMETRIC MEAN of the ratio over G's layers within 2.2x of fp32
    # PyTorch (measured 1.8), every single layer within 6x (its lottery) and within 3x of the worst error fp32 PyTorch
    # itself shows on any layer of the same network (HIP's worst: 2.7e-3, PyTorch's: 2.8e-3).
    g_rows = [(e_hip, e_cpu) for e_hip, e_cpu, k in rows if k.startswith("G.")]
    gmean = float(np.exp(np.mean([np.log((eh + 1e-12) / (ec + 1e-12)) for eh, ec in g_rows])))
    with capsys.disabled():
        print("    geometric mean of HIP : fp32-CPU over G's layers: %.2f" % gmean)
    assert gmean <= 2.2, gmean          # measured 1.6 (round 6) .. 1.8 (round 4)
    worst_cpu = {t: max(ec for eh, ec, k in rows if k.startswith(t)) for t in ("G.", "R.", "F.")}
    for e_hip, e_cpu, k in rows:
        assert e_hip <= 6.0 * e_cpu + 2e-5, "%s: HIP %.3e vs fp64, fp32 CPU oracle %.3e" % (k, e_hip, e_cpu)
        # (G and R only: F's rows that survive the filter above are still cancellation-dominated sums behind the L2
        # normalisation -- mlp_1.2.weight, filtered, is 389 % / 210 % off for HIP / fp32 PyTorch -- and carry the forward
        # error of fake_B, the END of G's 25-conv chain, amplified; they are held by the 6x rule and the absolute bound)
        if not k.startswith("F."):
            assert e_hip <= 3.0 * worst_cpu[k[:2]] + 2e-5, "%s: HIP %.3e vs fp64, worst fp32 CPU layer %.3e" % (k, e_hip, worst_cpu[k[:2]])
        assert e_hip <= (3.5e-2 if k.startswith("F.") else 8e-3), "%s: HIP %.3e vs fp64" % (k, e_hip)


def test_registration_net_on_a_second_stream_changes_nothing(O):
    """opt.overlap_registration (build-defined, default on): netR's forward and backward run on a second HIP stream beside
    the generator's -- as single-stream pieces with one autograd call per loss group and stream (opt.staged_step, default
    on: registration_model._step_pieces) or as one two-stream forward / one backward.  Two steps each way and on ONE stream
    from identical states: same losses, outputs and gradient arenas (up to the summation order of the weight gradients'
    float atomics)."""
    from tests.test_oracle_golden import make_step
    res = []
    for overlap, staged in ((True, True), (True, False), (False, False)):
        st, size, B = make_step()
        model, opt = _hip_model_from_oracle(st, size, B, 8)
        opt.overlap_registration, opt.staged_step = overlap, staged
        model.patch_id_source = PinnedIds()
        A0, B0 = C.image_pair(93, B, size, size)
        model.data_dependent_initialize({"A": A0, "B": B0, "A_paths": [""] * B, "B_paths": [""] * B})
        _load(model.netF, st.netF)
        model.setup(opt)
        assert model._overlap_registration() == overlap and model._staged_ok() == staged
        out = []
        for it in range(2):
            A_, B_ = C.image_pair(100 + it, B, size, size)
            model.set_input({"A": A_, "B": B_, "A_paths": [""] * B, "B_paths": [""] * B})
            model.optimize_parameters()
            torch.cuda.synchronize()
            out.append(([v for v in model.get_current_losses().values()], model.fake_B.clone(), model.registered.clone(),
                        model.regA.clone(), [o_.flat_g.clone() for o_ in model.optimizers]))
        res.append(out)
    for which in (0, 1):
        for it, (a, b) in enumerate(zip(res[which], res[2])):
            # step 0 starts from identical weights; step 1 from weights one Adam update apart by at most lr wherever a gradient
            # element sits at round-off level (Adam's first update is lr * g / |g|)
            tol = 1e-6 if it == 0 else 2e-4
            np.testing.assert_allclose(a[0], b[0], rtol=1e-5 if it == 0 else 2e-3, atol=1e-9)
            for x, y in zip(a[1:4], b[1:4]):
                close(x, y, rtol=tol, what="outputs, step %d" % it)
            if it == 0:
                gscale = max(float(g.norm()) for g in b[4])
                for nm, x, y in zip("GRF", a[4], b[4]):
                    assert float((x - y).norm()) <= 2e-5 * float(y.norm()) + 2e-6 * gscale, (which, nm)


def test_batch16_step_vs_oracle(O, capsys):
    """BASELINE configs[1] as quoted -- 256x256, ngf 64, batch 16 -- one whole step (forward, losses, backward, Adam)
    against the CPU oracle on identical weights, inputs and patch ids: outputs within 1e-4 relative, losses within 1e-3,
    every parameter gradient of G and R within the fp32-vs-fp32 distance measured at batch 1 against an fp64 arbiter
    (test_full_size_gradients_vs_fp64_oracle)."""
    B = 16
    st, size, A0, B0 = _full_size_oracle(O, B)
    model = _full_size_hip(st, size, B, A0, B0, default_path=True)
    A_, B_ = C.image_pair(11, B, size, size)
    ref = st.step(A_, B_)
    model.set_input({"A": A_, "B": B_, "A_paths": [""] * B, "B_paths": [""] * B})
    model.optimize_parameters()
    ls = model.get_current_losses()
    # the three outputs north_star names -- translated image, deformation field, warped moving image -- norm-wise AND
    # element-wise (99.9 % of the elements within ELEM_RTOL of max(|ref_i|, 1e-6 max|ref|), every element within 1: see
    # tests/test_gpu_ops.py::close); the other tensors norm-wise
    close(model.fake_B, st.fake_B, what="fake_B", elem_rtol=ELEM_RTOL); close(model.regA, st.regA, what="regA")
    close(model.registered, st.registered, what="registered", elem_rtol=ELEM_RTOL); close(model.idt_B, st.idt_B, what="idt_B")
    close(model.pos_flow, st.flow, what="pos_flow", elem_rtol=ELEM_RTOL)
    with capsys.disabled():
        from tests.test_gpu_ops import ELEMENTWISE
        for row in ELEMENTWISE[-3:]:
            print("\n  %-10s norm-wise %.2e   element-wise max %.2e  99.9%% %.2e  median %.2e" % row, end="")
    for k in ("G", "NCE", "R", "smooth", "local", "NCE_Y"):
        near(ls[k], ref[k], LOSS_RTOL_FULL, "loss " + k)
    rows = []
    for tag, n32, nh in (("G", st.netG, model.netG), ("R", st.netR, model.netR)):
        for (k, p32), (k2, ph) in zip(n32.named_parameters(), nh.named_parameters()):
            assert k == k2
            if tag == "G" and k.endswith(".bias") and k != "model.30.bias":
                continue  # zero true gradient (bias in front of InstanceNorm)
            g = p32.grad.double().flatten()
            rows.append((float((ph.grad.detach().cpu().double().flatten() - g).norm() / g.norm()), tag + "." + k))
    with capsys.disabled():
        print("\n  batch 16: rel. L2 distance of the HIP gradients to the fp32 CPU oracle's, worst 6")
        for e, k in sorted(rows, reverse=True)[:6]:
            print("    %-44s %.2e" % (k, e))
    for e, k in rows:      # measured (MI355X, rounds 3 - 6): worst 2.8e-4 .. 2.95e-4 (G.model.1.weight, the deepest backward)
        from tests.test_gpu_ops import MARGINS
        MARGINS.append(("tests/test_gpu_models.py::test_batch16_step_vs_oracle", "grad " + k, e, 4e-4))
        assert e <= 4e-4, "%s: %.3e" % (k, e)


def test_batch16_equals_per_sample_runs(O):
    """BASELINE configs[1] at its own batch: every kernel on the path is per-sample, so fake_B[i], regA[i], flow[i] and
    registered[i] of a batch-16 forward equal the batch-1 results sample by sample (up to the split convs' per-tensor
    power-of-two scale, which depends on the batch maximum)."""
    from dfmir_amd.options import default_options
    from dfmir_amd.registration_model import REGISTRATIONModel
    size, B = 256, 16
    torch.manual_seed(5)
    model = REGISTRATIONModel(default_options(batch_size=B, crop_size=size, load_size=size, ngf=64, gpu_ids=[0],
                                              checkpoints_dir="/tmp/dfmir_ckpt", name="b16"))
    with torch.no_grad():
        model.netR.flow.weight.mul_(1e5)
    A, Bm = C.image_pair(21, B, size, size)
    A, Bm = A.to(DEV), Bm.to(DEV)
    with torch.no_grad():
        def run(a, b):
            model.set_input({"A": a, "B": b, "A_paths": [""] * a.shape[0], "B_paths": [""] * a.shape[0]})
            model.forward()
            ys, yt, flow = model.netR(model.real_A, model.real_B)
            return model.fake_B.clone(), model.idt_B.clone(), ys, flow, model.spatialTransformer(model.fake_B, flow)
        full = run(A, Bm)
        for i in (0, 7, 15):
            one = run(A[i:i + 1], Bm[i:i + 1])
            for nm, f, o in zip(("fake_B", "idt_B", "regA", "flow", "registered"), full, one):
                close(f[i:i + 1], o, rtol=1e-5, what="%s[%d]" % (nm, i))


@pytest.mark.parametrize("shape,plugin", [((32, 32, 32), False), ((64, 64, 64), True), ((128, 128, 128), True),
                                          ((160, 192, 224), False)],
                         ids=["32", "64-plugin", "128-plugin(configs[3])", "160x192x224(configs[4] shard)"])
def test_registration3d_step_vs_oracle(O, shape, plugin):
    """The 3-D step (VxmDense 3-D + NCC[9,9,9] + Grad l2): two consecutive steps against the oracle, up to BASELINE's own
    sizes (configs[3] = 128^3 with the plugin's features; one GPU's volume of configs[4])."""
    from dfmir_amd.registration3d import Registration3DModel
    feats = O.PLUGIN_UNET_FEATURES if plugin else None
    torch.manual_seed(21)
    st = O.Registration3DStep(shape, feats)
    with torch.no_grad():
        st.netR.flow.weight.mul_(3e4)
    model = Registration3DModel(shape, feats, device=DEV)
    _load(model.netR, st.netR)
    for it in range(2):
        A = C.rand(31 + it, 1, 1, *shape)
        B = 0.5 * A + 0.5 * C.rand(41 + it, 1, 1, *shape)
        ref = st.step(A, B)
        model.set_input({"A": A, "B": B})
        model.optimize_parameters()
        got = model.get_current_losses()
        if it == 0:
            close(model.flow, st.flow, what="flow"); close(model.regA, st.ys, what="warped")
            for (k, po), (k2, ph) in zip(st.netR.named_parameters(), model.netR.named_parameters()):
                close(ph.grad, po.grad, rtol=2e-3, atol=1e-9, what="grad " + k)    # measured worst 9.0e-4 (profiles/r06_parity_margins.txt)
        for k in ("ncc", "grad"):
            near(got[k], ref[k], 1e-3, "3-D loss %s step %d" % (k, it), floor=1e-7)


def test_skipping_the_unused_target_branch_changes_nothing(O):
    """VxmDense.skip_unused_target (build-defined): without the discarded warp(target, -flow) output the
    outputs the step reads (y_source, flow) are bit-identical and the parameter gradients equal to atomic-order round-off."""
    from dfmir_amd.voxelmorph import VxmDense
    shape = (16, 16, 32)
    torch.manual_seed(3)
    net = VxmDense(shape, None, int_steps=7, bidir=True).to(DEV)
    with torch.no_grad():
        net.flow.weight.mul_(3e4)
    A = C.rand(31, 1, 1, *shape).to(DEV)
    B = C.rand(41, 1, 1, *shape).to(DEV)
    res = []
    for skip in (False, True):
        net.skip_unused_target = skip
        net.zero_grad()
        ys, yt, fl = net(A, B)
        (ys.sum() + (fl * fl).sum()).backward()
        assert (yt is None) == skip
        res.append((ys.detach().clone(), fl.detach().clone(), [p.grad.clone() for p in net.parameters()]))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    for g0, g1 in zip(res[0][2], res[1][2]):          # (weight gradients sum through float atomics: equal to round-off)
        close(g0, g1, rtol=1e-5, atol=1e-9, what="parameter gradient")
    net.skip_unused_target = True
    y2, f2 = net(A, B, registration=True)            # the inference form is untouched
    assert y2.shape == A.shape and f2.shape[1] == 3


def test_probe_audit_full_steps():
    """DFMIR_PROBE_AUDIT: every fp16x2-split launch of a 256x256 ngf-64 train step and of a 64^3 3-D step is handed a
    range probe that bounds the true max |t| of its operand (inherited probes included: blur outputs, upcat, sampled-
    feature scatters, dgrad epilogues, per-plane dY maxima) -- also with a 1e4x outlier pixel in the input, where a stale
    or under-estimating probe would overflow fp16 to inf."""
    from dfmir_amd import ops
    from dfmir_amd.options import default_options
    from dfmir_amd.registration3d import Registration3DModel
    from dfmir_amd.registration_model import REGISTRATIONModel
    size, B = 256, 1
    log = ops.set_probe_audit(True)
    try:
        opt = default_options(batch_size=B, crop_size=size, load_size=size, ngf=64, gpu_ids=[0],
                              checkpoints_dir="/tmp/dfmir_ckpt", name="audit", dvf_image="synthetic")
        torch.manual_seed(5)
        model = REGISTRATIONModel(opt)
        with torch.no_grad():
            model.netR.flow.weight.mul_(1e5)             # a non-identity field: warps produce new values
        A0, B0 = C.image_pair(9, B, size, size)
        paths = [""] * B
        model.data_dependent_initialize({"A": A0, "B": B0, "A_paths": paths, "B_paths": paths})
        model.setup(opt)
        for it in range(2):
            A_, B_ = C.image_pair(11 + it, B, size, size)
            if it == 1:
                A_[0, 0, 100, 77] = 1e4                  # one outlier pixel, 1e4 x the data range
                B_[0, 0, 31, 200] = -1e4
            model.set_input({"A": A_, "B": B_, "A_paths": paths, "B_paths": paths})
            model.optimize_parameters()
            ls = model.get_current_losses()
            assert all(v == v and abs(v) < 1e30 for v in ls.values()), ls
            assert bool(torch.isfinite(model.fake_B).all())
            for o_ in model.optimizers:
                assert bool(torch.isfinite(o_.flat_g).all())
        n2d = len(log)
        assert n2d > 150, n2d                            # ~90 split forward/dgrad launches + wgrads per step, 2 steps
        shape = (64, 64, 64)
        torch.manual_seed(6)
        m3 = Registration3DModel(shape, None, device=DEV)
        with torch.no_grad():
            m3.netR.flow.weight.mul_(3e4)
        for it in range(2):
            A = C.rand(31 + it, 1, 1, *shape)
            Bv = 0.5 * A + 0.5 * C.rand(41 + it, 1, 1, *shape)
            if it == 1:
                A[0, 0, 10, 20, 30] = 1e4
            m3.set_input({"A": A, "B": Bv})
            m3.optimize_parameters()
            assert bool(torch.isfinite(m3.optimizer_R.flat_g).all())
        assert len(log) - n2d > 30, len(log) - n2d
        # the audit really saw inherited probes that are loose upper bounds (probe > true max), never below
        assert all(pv >= tv for _, pv, tv in log if tv == tv)
        assert any(pv > tv * 1.0001 for _, pv, tv in log)
    finally:
        ops.set_probe_audit(False)


# ------------------------------------------------------------------ full-size, size-independent properties
@pytest.mark.parametrize("cfg", [(256, 256, 64, 32, True), (64, 128, 256, 16, False), (128, 64, 256, 16, False),
                                 (256, 128, 128, 16, False)],
                         ids=["res256@64x32", "64to128@256x16", "128to64@256x16", "256to128@128x16"])
def test_full_size_conv_adjoint_and_linearity(cfg):
    """BASELINE configs[1] layer shapes at the bench's batch: the kernels must satisfy the identities a convolution
    satisfies at any size --  <conv(x,w), g> = <x, dgrad(g)> = <w, wgrad(x,g)>  and linearity in w -- to fp32
    round-off of the (fp64-accumulated) inner products.  Exercises the split fp16x2 forward, dgrad and wgrad
    kernels on the exact launch geometries of the measured step."""
    from dfmir_amd import ops
    Cin, Cout, H, N, reflect = cfg
    x = C.randn(101, 1, Cin, H, H).to(DEV).expand(N, -1, -1, -1).contiguous()
    x = (x * torch.linspace(0.5, 1.5, N, device=DEV).view(N, 1, 1, 1)).requires_grad_()
    w = (C.randn(102, Cout, Cin, 3, 3) / (Cin * 9) ** 0.5).to(DEV).requires_grad_()
    g = C.randn(103, 1, Cout, H, H).to(DEV).expand(N, -1, -1, -1).contiguous()
    y = ops.conv(x, w, None, None, 1, 1, 1 if reflect else 0, 0, 0.0)
    (y * g).sum().backward()
    dot = lambda a, b: float((a.double() * b.double()).sum())
    yg, xdx, wdw = dot(y, g), dot(x, x.grad), dot(w, w.grad)
    scale = float(y.double().norm() * g.double().norm())
    assert abs(yg - xdx) <= 2e-6 * scale, (yg, xdx, scale)
    assert abs(yg - wdw) <= 2e-6 * scale, (yg, wdw, scale)
    with torch.no_grad():
        w2 = (C.randn(104, Cout, Cin, 3, 3) / (Cin * 9) ** 0.5).to(DEV)
        y2 = ops.conv(x, w2, None, None, 1, 1, 1 if reflect else 0, 0, 0.0)
        y12 = ops.conv(x, w.detach() + w2, None, None, 1, 1, 1 if reflect else 0, 0, 0.0)
        err = float((y12 - (y + y2)).abs().max())
        assert err <= 2e-5 * float(y12.abs().max()), err


@pytest.mark.parametrize("cfg", [(34, 32, (160, 192, 224)), (32, 16, (160, 192, 224)), (16, 3, (160, 192, 224)),
                                 (48, 32, (80, 96, 112)), (34, 16, (128, 128, 128)), (48, 32, (64, 64, 64))],
                         ids=["34to32@big", "32to16@big", "16to3@big", "48to32@half", "34to16@128", "48to32@64"])
def test_full_size_conv3d_adjoint_and_linearity(cfg):
    """BASELINE configs[3] / [4] layer shapes (VxmDense 3-D, plugin features at 128^3, default features at
    160x192x224, batch 1): the 3x3x3 forward, dgrad and wgrad kernels (conv3d_mfma16_k / conv3d_wgrad16_k) satisfy
    <conv(x,w), g> = <x, dgrad(g)> = <w, wgrad(x,g)>  and linearity in w to fp32 round-off of the fp64-accumulated
    inner products -- size-independent identities at sizes no CPU oracle finishes."""
    from dfmir_amd import ops
    Cin, Cout, sp = cfg
    lo = tuple(s // 8 for s in sp)
    up = lambda t: torch.nn.functional.interpolate(t, size=sp, mode="trilinear", align_corners=True)
    x = (up(C.randn(121, 1, Cin, *lo).to(DEV)) + 0.05 * torch.randn(1, Cin, *sp, device=DEV,
         generator=torch.Generator(device=DEV).manual_seed(122))).requires_grad_()
    w = (C.randn(123, Cout, Cin, 3, 3, 3) / (Cin * 27) ** 0.5).to(DEV).requires_grad_()
    g = up(C.randn(124, 1, Cout, *lo).to(DEV)) + 0.05 * torch.randn(1, Cout, *sp, device=DEV,
                                                                  generator=torch.Generator(device=DEV).manual_seed(125))
    y = ops.conv(x, w, None, None, 1, 1, 0, 0, 0.0)
    (y * g).sum().backward()
    dot = lambda a, b: float((a.double() * b.double()).sum())
    yg, xdx, wdw = dot(y, g), dot(x, x.grad), dot(w, w.grad)
    scale = float(y.double().norm() * g.double().norm())
    assert abs(yg - xdx) <= 2e-6 * scale, (yg, xdx, scale)
    assert abs(yg - wdw) <= 2e-6 * scale, (yg, wdw, scale)
    with torch.no_grad():
        w2 = (C.randn(126, Cout, Cin, 3, 3, 3) / (Cin * 27) ** 0.5).to(DEV)
        y12 = ops.conv(x, w.detach() + w2, None, None, 1, 1, 0, 0, 0.0)
        y12 -= y
        y12 -= ops.conv(x, w2, None, None, 1, 1, 0, 0, 0.0)
        assert float(y12.abs().max()) <= 2e-5 * float(y.abs().max()), float(y12.abs().max())


def test_registration3d_captured_step_matches_eager():
    """Registration3DModel(capture_step=True): a replayed step equals the same step enqueued eagerly from the same
    restored state (weights, Adam moments) -- losses, outputs and the gradient arena."""
    from dfmir_amd.registration3d import Registration3DModel
    from tests import step3d
    shape = (32, 32, 32)
    torch.manual_seed(0)
    m = Registration3DModel(shape, None, capture_step=True, device=DEV)
    A = C.randn(141, 1, 1, *shape).to(DEV).clamp(-1, 1)
    B = (0.5 * A + 0.5 * C.randn(142, 1, 1, *shape).to(DEV)).clamp(-1, 1)
    step3d.assert_replay_matches_eager(m, {"A": A, "B": B}, ["grad", "ncc"])


def test_full_size_warp_properties():
    """160x192x224 (BASELINE configs[4] geometry): zero displacement is the identity, an integer shift moves
    voxels exactly, and the warp is linear in src with d(src) as its adjoint."""
    from dfmir_amd import ops
    shp = (1, 1, 160, 192, 224)
    src = C.randn(111, 1, 1, 40, 48, 56).to(DEV)
    src = torch.nn.functional.interpolate(src, size=shp[2:], mode="trilinear", align_corners=True).requires_grad_()
    zero = torch.zeros(1, 3, *shp[2:], device=DEV)
    assert torch.equal(ops.warp(src.detach(), zero), src.detach())
    shift = zero.clone(); shift[:, 2] = 3.0
    ys = ops.warp(src.detach(), shift)
    assert torch.equal(ys[..., :-3], src.detach()[..., 3:]) and float(ys[..., -3:].abs().max()) == 0.0
    coarse = C.randn(112, 1, 3, 5, 6, 7).to(DEV)
    flow = torch.nn.functional.interpolate(coarse, size=shp[2:], mode="trilinear", align_corners=True)
    g = C.randn(113, 1, 1, 40, 48, 56).to(DEV)
    g = torch.nn.functional.interpolate(g, size=shp[2:], mode="nearest")
    y = ops.warp(src, flow)
    (y * g).sum().backward()
    dot = lambda a, b: float((a.double() * b.double()).sum())
    lhs, rhs = dot(y, g), dot(src, src.grad)
    assert abs(lhs - rhs) <= 2e-6 * float(y.double().norm() * g.double().norm()), (lhs, rhs)
