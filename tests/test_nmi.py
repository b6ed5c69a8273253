"""NMI_Loss (util/losses.py:263-348) on the HIP kernels of dfmir_amd/csrc/nmi.hip: the C ABI and the argument checks
(CPU), the reference's own losses and gradients (tests/golden/nmi.npz), a float64 restatement of the formula at the full
3-D size, run-to-run bit-reproducibility, and Registration3DModel(similarity='nmi') against the oracle step."""
import os

import numpy as np
import pytest
import torch

from tests.golden import common as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


# ------------------------------------------------------------------------------------------ float64 restatement
def nmi_ref64(y_true, y_pred, centers, sigma_ratio=0.5, max_clip=1.0, mask=None, chunk=1 << 17):
    """(-MI, d/dy_true, d/dy_pred) in float64 on the CPU, written from the formula (not from the reference's code):
    w_k(x) = exp(-(x - c_k)^2 / (2 sigma^2)) / sum_k ..., x clamped to [0, max_clip]; P = sum_v w(y_pred) w(y_true)^T / V,
    p_true / p_pred the mean weights, MI = sum P log(P / (p_pred p_true^T + 1e-5) + 1e-5).  Voxels are streamed in chunks;
    the gradient is autograd through the per-chunk sums, seeded with dMI/d(P, p_true, p_pred) of the small problem."""
    c = torch.tensor(np.asarray(centers, np.float64))
    sigma = float(np.mean(np.diff(np.asarray(centers, np.float64)))) * sigma_ratio
    k = 1.0 / (2.0 * sigma * sigma)
    t = y_true.detach().cpu().double().reshape(-1)
    p = y_pred.detach().cpu().double().reshape(-1)
    if mask is None:
        sel = torch.ones_like(t)
    else:
        sel = (mask.detach().cpu().double().expand(y_true.shape).reshape(-1) > 1e-4).double()

    def weights(x):
        w = torch.exp(-k * (x.clamp(0.0, max_clip)[:, None] - c[None, :]) ** 2)
        return w / w.sum(1, keepdim=True)

    nb = c.numel()
    P = torch.zeros(nb, nb, dtype=torch.float64)
    st = torch.zeros(nb, dtype=torch.float64)
    sp = torch.zeros(nb, dtype=torch.float64)
    with torch.no_grad():
        for s in range(0, t.numel(), chunk):
            m = sel[s:s + chunk, None]
            wt, wp = weights(t[s:s + chunk]) * m, weights(p[s:s + chunk]) * m
            P += wp.T @ wt
            st += wt.sum(0)
            sp += wp.sum(0)
    V = float(sel.sum())
    dt, dp = torch.empty_like(t), torch.empty_like(p)
    with torch.enable_grad():                  # (also when called from an autograd Function's forward)
        P_, pt_, pp_ = (x.div(V).requires_grad_() for x in (P, st, sp))
        mi = (P_ * torch.log(P_ / (pp_[:, None] * pt_[None, :] + 1e-5) + 1e-5)).sum()
        mi.backward()
        gP, gt, gp = P_.grad, pt_.grad, pp_.grad
        for s in range(0, t.numel(), chunk):
            xt = t[s:s + chunk].clone().requires_grad_()
            xp = p[s:s + chunk].clone().requires_grad_()
            m = sel[s:s + chunk, None]
            wt, wp = weights(xt) * m, weights(xp) * m
            f = ((wp.T @ wt) * gP).sum() + (wt.sum(0) * gt).sum() + (wp.sum(0) * gp).sum()
            (f / V).backward()
            dt[s:s + chunk], dp[s:s + chunk] = -xt.grad, -xp.grad
    return -float(mi.detach()), dt.view(y_true.shape), dp.view(y_pred.shape)


class _RefNMIFn(torch.autograd.Function):
    """nmi_ref64 as an autograd node of a float32 graph (the oracle step's similarity term)."""

    @staticmethod
    def forward(ctx, y_true, y_pred, centers, max_clip):
        loss, dt, dp = nmi_ref64(y_true, y_pred, centers, 0.5, max_clip)
        ctx.save_for_backward(dt.float(), dp.float())
        return torch.tensor([loss], dtype=torch.float32)

    @staticmethod
    def backward(ctx, g):
        dt, dp = ctx.saved_tensors
        return dt * g, dp * g, None, None


# ------------------------------------------------------------------------------------------ CPU tier
def test_nmi_symbols_in_header_exports_and_ctypes_table():
    import ctypes
    import dfmir_amd
    from dfmir_amd import _lib
    from tests.test_abi import header_symbols
    names = ("dfmir_nmi_ws_floats", "dfmir_nmi_fwd", "dfmir_nmi_bwd")
    h = ctypes.CDLL(dfmir_amd.LIB_PATH)
    for s in names:
        assert s in header_symbols() and s in _lib.exported_symbols() and hasattr(h, s), s
    lib = dfmir_amd.lib()
    assert lib.dfmir_nmi_ws_floats(1000, 65) == -1 and lib.dfmir_nmi_ws_floats(1000, 1) == -1
    assert lib.dfmir_nmi_ws_floats(1000, 32) > 32 * 32 and lib.dfmir_nmi_ws_floats(1 << 24, 64) > 64 * 64 * 2
    # bad arguments fail without touching a device
    assert lib.dfmir_nmi_fwd(None, None, None, None, 32, 1.0, 1.0, 10, None, None, None) != 0
    assert b"invalid argument" in lib.dfmir_last_error()


def test_nmi_loss_rejects_bad_arguments_before_any_launch():
    from dfmir_amd import ops
    from dfmir_amd._lib import DfmirHipError
    from dfmir_amd.losses import NMI_Loss
    x = torch.rand(1, 1, 8, 8)
    with pytest.raises(ValueError, match="2 to 64"):
        NMI_Loss(np.linspace(0, 1, 65))
    with pytest.raises(DfmirHipError, match="2 to 64"):
        ops.nmi_loss(x, x, np.linspace(0, 1, 65))
    with pytest.raises(ValueError, match="needs a mask"):
        NMI_Loss(np.linspace(0, 1, 16), crop_background=True)(x, x)
    with pytest.raises(DfmirHipError, match="no CPU fallback"):
        NMI_Loss(np.linspace(0, 1, 16))(x, x)
    l = NMI_Loss([0.0, 0.25, 1.0], sigma_ratio=0.5, patch_size=3)
    assert l.num_bins == 3 and l.patch_size == 3 and abs(l.sigma - 0.25) < 1e-15 and abs(l.preterm - 8.0) < 1e-12


def test_registration3d_rejects_unknown_similarity():
    from dfmir_amd.registration3d import Registration3DModel
    with pytest.raises(ValueError, match="similarity"):
        Registration3DModel((8, 8, 8), device="cpu", similarity="mi")


# ------------------------------------------------------------------------------------------ GPU: fixture
def _golden_cases(golden):
    g = golden("nmi.npz")
    return g, [str(t) for t in g["cases"]]


def _run(g, tag):
    from dfmir_amd.losses import NMI_Loss
    ratio, maxc, crop = (float(v) for v in g[tag + "_params"])
    yt = torch.from_numpy(g[tag + "_true"]).to(DEV).requires_grad_()
    yp = torch.from_numpy(g[tag + "_pred"]).to(DEV).requires_grad_()
    crit = NMI_Loss(g[tag + "_centers"], device=DEV, sigma_ratio=ratio, max_clip=maxc, crop_background=bool(crop))
    mask = torch.from_numpy(g[tag + "_mask"]).to(DEV) if crop else None
    loss = crit(yt, yp, mask=mask)
    loss.backward()
    return loss, yt, yp, mask, maxc


@pytest.mark.gpu
def test_nmi_golden(golden):
    """Every case of nmi.npz: the loss (shape (1,)) and the gradients of both arguments against the reference."""
    from tests.test_gpu_ops import close
    g, tags = _golden_cases(golden)
    for tag in tags:
        loss, yt, yp, _, _ = _run(g, tag)
        assert loss.shape == (1,), loss.shape
        # bounds: 2x the worst measured on the MI355X (1.6e-7 loss, 5.7e-7 gradients; test_losses_golden's NCC bars are
        # 1e-4 / 1e-3)
        close(loss, g[tag + "_loss"], rtol=3e-7, atol=0, what=tag + " loss")
        close(yt.grad, g[tag + "_dtrue"], rtol=1.1e-6, atol=0, what=tag + " d y_true")
        close(yp.grad, g[tag + "_dpred"], rtol=1.1e-6, atol=0, what=tag + " d y_pred")


@pytest.mark.gpu
def test_nmi_gradient_is_zero_outside_the_clamp_and_the_mask(golden):
    g, tags = _golden_cases(golden)
    for tag in tags:
        _, yt, yp, mask, maxc = _run(g, tag)
        for x in (yt, yp):
            cut = (x.detach() < 0) | (x.detach() > maxc)
            if mask is not None:
                cut |= ~(mask.expand_as(x) > 1e-4)
            assert bool(cut.any()) and float(x.grad[cut].abs().max()) == 0.0, tag
            assert float(x.grad[~cut].abs().max()) > 0.0, tag
        on_bounds = (yt.detach() == 0) | (yt.detach() == maxc)
        if mask is None:                              # torch.clamp's gradient passes on the bounds themselves
            assert bool(on_bounds.any()) and float(yt.grad[on_bounds].abs().max()) > 0.0, tag


@pytest.mark.gpu
def test_nmi_batch_is_one_histogram():
    """B = 2 gives the value and gradients of the two images stacked into one (the reference flattens the batch)."""
    from dfmir_amd.losses import NMI_Loss
    crit = NMI_Loss(np.linspace(0, 1, 32), device=DEV)
    a, b = C.rand(5, 2, 1, 20, 24).to(DEV), C.rand(6, 2, 1, 20, 24).to(DEV)
    a1, b1 = a.clone().requires_grad_(), b.clone().requires_grad_()
    l1 = crit(a1, b1)
    l1.backward()
    a2 = torch.cat([a[0:1], a[1:2]], 2).requires_grad_()
    b2 = torch.cat([b[0:1], b[1:2]], 2).requires_grad_()
    l2 = crit(a2, b2)
    l2.backward()
    assert torch.equal(l1, l2)
    assert torch.equal(a1.grad, torch.cat([a2.grad[:, :, :20], a2.grad[:, :, 20:]], 0))
    assert torch.equal(b1.grad, torch.cat([b2.grad[:, :, :20], b2.grad[:, :, 20:]], 0))


@pytest.mark.gpu
def test_nmi_empty_selection_is_nan():
    from dfmir_amd.losses import NMI_Loss
    crit = NMI_Loss(np.linspace(0, 1, 16), device=DEV, crop_background=True)
    x = C.rand(7, 1, 1, 8, 8).to(DEV).requires_grad_()
    loss = crit(x, x, mask=torch.zeros(1, 1, 8, 8, device=DEV))
    loss.backward()
    assert bool(torch.isnan(loss).all()) and float(x.grad.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ GPU: full size
@pytest.mark.gpu
def test_nmi_full_size_vs_float64_and_bit_reproducible():
    """160 x 192 x 224, nb = 64, against the float64 restatement; forward and backward bit-identical across runs."""
    from dfmir_amd import ops
    from tests.test_gpu_ops import close, near
    shp = (1, 1, 160, 192, 224)
    centers = np.linspace(0.0, 1.0, 64)
    a = C.rand(81, *shp) * 1.1 - 0.05
    b = (0.5 * a + 0.5 * C.rand(82, *shp)) * 1.1 - 0.05
    runs = []
    for _ in range(2):
        x, y = a.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
        loss = ops.nmi_loss(x, y, centers)
        loss.backward()
        torch.cuda.synchronize()
        runs.append((loss.detach().cpu(), x.grad.cpu(), y.grad.cpu()))
    for r0, r1 in zip(runs[0], runs[1]):
        assert torch.equal(r0, r1)
    ref, dt, dp = nmi_ref64(a, b, centers)
    # bounds: 2x the worst measured on the MI355X (9.6e-8 loss, 2.9e-6 gradients)
    near(float(runs[0][0]), ref, 1.9e-7, "full-size loss")
    close(runs[0][1], dt, rtol=5.5e-6, atol=0, what="full-size d y_true")
    close(runs[0][2], dp, rtol=5.5e-6, atol=0, what="full-size d y_pred")


# ------------------------------------------------------------------------------------------ GPU: the 3-D model
def _nmi_oracle_step(O):
    class NMIRegistration3DStep(O.Registration3DStep):
        """The oracle's 3-D step with NMI_Loss(real_B, warped) (32 uniform centers on [0, 1]) in place of NCC."""

        def step(self, A, B):
            ys, yt, flow = self.netR(A, B)
            self.opt.zero_grad()
            l_sim = _RefNMIFn.apply(B, ys, np.linspace(0.0, 1.0, 32), 1.0)
            l_reg = O.grad_loss_l2(flow)
            (l_sim + self.lam * l_reg).sum().backward()
            self.opt.step()
            self.ys, self.flow = ys, flow
            return dict(nmi=float(l_sim.detach()), grad=float(l_reg.detach()))
    return NMIRegistration3DStep


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(32, 32, 32), (128, 128, 128)], ids=["32", "128"])
def test_registration3d_nmi_step_vs_oracle(shape):
    from oracle import dfmir_oracle as O
    from dfmir_amd.registration3d import Registration3DModel
    from tests.test_gpu_models import _load
    from tests.test_gpu_ops import close, near
    torch.manual_seed(21)
    st = _nmi_oracle_step(O)(shape)
    with torch.no_grad():
        st.netR.flow.weight.mul_(3e4)
    model = Registration3DModel(shape, device=DEV, similarity='nmi')
    _load(model.netR, st.netR)
    for it in range(2):
        A = C.rand(31 + it, 1, 1, *shape)
        B = 0.5 * A + 0.5 * C.rand(41 + it, 1, 1, *shape)
        ref = st.step(A, B)
        model.set_input({"A": A, "B": B})
        model.optimize_parameters()
        got = model.get_current_losses()
        assert sorted(got) == ["grad", "nmi"]
        if it == 0:
            close(model.flow, st.flow, what="flow"); close(model.regA, st.ys, what="warped")
            for (k, po), (k2, ph) in zip(st.netR.named_parameters(), model.netR.named_parameters()):
                close(ph.grad, po.grad, rtol=2e-3, atol=1e-9, what="grad " + k)
        for k in ("nmi", "grad"):
            near(got[k], ref[k], 1e-3, "3-D loss %s step %d" % (k, it), floor=1e-7)


@pytest.mark.gpu
def test_registration3d_nmi_captured_step_matches_eager():
    """similarity='nmi' under capture_step=True: a replayed step equals the same step enqueued eagerly."""
    from dfmir_amd.registration3d import Registration3DModel
    from tests import step3d
    shape = (32, 32, 32)
    torch.manual_seed(0)
    m = Registration3DModel(shape, None, capture_step=True, device=DEV, similarity='nmi')
    m.parallelize()
    A = C.rand(141, 1, 1, *shape).to(DEV)
    B = (0.5 * A + 0.5 * C.rand(142, 1, 1, *shape).to(DEV))
    step3d.assert_replay_matches_eager(m, {"A": A, "B": B}, ["grad", "nmi"])
