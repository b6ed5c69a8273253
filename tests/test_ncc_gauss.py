"""NCC_Loss(kernel_type='gaussian') (util/losses.py:145-261) on the HIP kernels of dfmir_amd/csrc/losses.hip: the C ABI and
the argument checks (CPU), the reference's own losses and gradients (tests/golden/ncc_gauss.npz, 2-D: the reference's
window is 2-D only), a float64 restatement of the formulas for the 2-D cases and the build-defined 3-D window, run-to-run
bit-reproducibility, and Registration3DModel(ncc_kernel='gaussian') eager and captured.

Tolerances: the fixture stores how far the reference's own fp32 CPU evaluation lies from the float64 restatement, per
case and as maxima (`ref_fp32_err_loss`: relative error of the loss, over all cases; `ref_fp32_err_grad`: |g - g64| / |g64|
in the 2-norm, over the well-conditioned cases).  The kernels get 4x those values: the separable evaluation rounds one
intermediate per axis more than the reference's single K^2-term sum and adds in another order, while the cancellation in
I_var = I2_sum - u * I_sum amplifies both alike.  `half_const` is the one ill-conditioned case: over its constant half
I_var is fp32 cancellation noise of the size of eps / J_var, the reference's own gradient is off by 1.5e-3 (the others:
2.6e-7 .. 1.3e-6), and its gradient is bounded by 4x ITS OWN entry -- that figure bounds no other case."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.golden import common as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
FACTOR = 4.0


# ------------------------------------------------------------------------------------------ float64 restatement
def gauss_window64(sigma, nd):
    """(window [K]*nd, K) in float64: c * g (x) ... (x) g, g(d) = exp(-(d - (K-1)/2)^2 / (2 sigma^2)), c = 1 / (2.506628274631 sigma)."""
    K = 3 * sigma + (3 * sigma + 1) % 2
    d = torch.arange(K, dtype=torch.float64) - (K - 1) / 2.0
    g = torch.exp(-d * d / (2.0 * sigma * sigma))
    w = g
    for _ in range(nd - 1):
        w = w[..., None] * g
    return w / (2.506628274631 * sigma), K


def ncc_gauss_ref64(I, J, sigma, mask=None, eps=1e-5, reduction='neg_sqrt_mean'):
    """(loss, d loss / d I) in float64 on the CPU, written from the formulas: local sums = zero-padded convolutions with the
    window, u = sum / win_size, cc = cross^2 / (I_var J_var + eps); -sqrt(mean cc), with a mask -sqrt(sum(cc m) / sum(m))
    (0 for an empty mask); 'neg_mean' is -mean(cc) resp. -sum(cc m) / sum(m).  sum(m) is the sum of the mask AS GIVEN: one
    that broadcasts over the batch counts once there and B times in sum(cc m), as in the reference (util/losses.py:260-261)."""
    nd = I.dim() - 2
    w, K = gauss_window64(sigma, nd)
    wn = w.sum()
    conv = F.conv2d if nd == 2 else F.conv3d
    x = I.detach().cpu().double().requires_grad_()
    y = J.detach().cpu().double()
    S = lambda t: conv(t, w[None, None], padding=K // 2)
    Is, Js, I2, J2, IJ = S(x), S(y), S(x * x), S(y * y), S(x * y)
    uI, uJ = Is / wn, Js / wn
    cross = IJ - uJ * Is - uI * Js + uI * uJ * wn
    Iv = I2 - 2 * uI * Is + uI * uI * wn
    Jv = J2 - 2 * uJ * Js + uJ * uJ * wn
    cc = cross * cross / (Iv * Jv + eps)
    if mask is None:
        m = cc.mean()
    else:
        mk = mask.detach().cpu().double()
        if float(mk.sum()) == 0.0:
            return 0.0, torch.zeros_like(x)
        m = (cc * mk).sum() / mk.sum()
    loss = -torch.sqrt(m) if reduction == 'neg_sqrt_mean' else -m
    loss.backward()
    return float(loss.detach()), x.grad


def rel_errors(loss, grad, loss64, grad64):
    """(relative error of the loss, norm-wise relative error of the gradient) against float64 values."""
    g, g64 = torch.as_tensor(np.asarray(grad)).double().reshape(-1), torch.as_tensor(np.asarray(grad64)).double().reshape(-1)
    return abs(float(loss) - float(loss64)) / abs(float(loss64)), float((g - g64).norm() / g64.norm())


def _bounds(g, tag=None):
    """(loss bound, gradient bound): 4x the reference's fp32 error -- of the ill-conditioned case itself for its gradient."""
    eg = float(g["ref_fp32_err_grad"])
    if tag == "half_const":
        eg = float(g["ref_fp32_err_grad_case"][[str(t) for t in g["cases"]].index(tag)])
        assert eg > 100 * float(g["ref_fp32_err_grad"])         # (what makes it the special case)
    return FACTOR * float(g["ref_fp32_err_loss"]), FACTOR * eg


# ------------------------------------------------------------------------------------------ CPU tier
def test_ncc_gauss_symbols_in_header_exports_and_ctypes_table():
    import dfmir_amd
    from dfmir_amd import _lib
    from tests.test_abi import header_symbols
    h = ctypes.CDLL(dfmir_amd.LIB_PATH)
    for s in ("dfmir_ncc_gauss_fwd", "dfmir_ncc_gauss_bwd"):
        assert s in header_symbols() and s in _lib.exported_symbols() and hasattr(h, s), s
    assert dfmir_amd.lib().dfmir_abi_version() == 14


def test_ncc_gauss_entry_points_reject_bad_arguments_before_any_launch():
    import dfmir_amd
    from dfmir_amd import ops
    lib = dfmir_amd.lib()
    taps, K, c = ops.ncc_gauss_window(3)
    t = (ctypes.c_float * 31)(*taps)
    p = ctypes.c_void_p(64)                      # never dereferenced: every call below fails its argument check

    def fwd(I=p, taps=t, K=K, c=c, mode=0, B=1):
        return lib.dfmir_ncc_gauss_fwd(I, p, None, mode, p, p, p, p, B, 1, 8, 8, taps, K, c, 1e-5, None)

    def bwd(dI=p, taps=t, K=K, c=c, mode=0):
        return lib.dfmir_ncc_gauss_bwd(p, p, None, mode, p, p, p, p, p, dI, 1, 1, 8, 8, taps, K, c, 1e-5, None)

    for call in (fwd, bwd):
        bad = [dict(taps=None), dict(K=8), dict(K=1), dict(K=33), dict(c=0.0), dict(c=-1.0), dict(mode=2), dict(mode=8)]
        bad.append(dict(I=None) if call is fwd else dict(dI=None))
        for kw in bad:
            assert call(**kw) != 0, kw
            assert b"invalid argument" in lib.dfmir_last_error(), kw
    assert fwd(B=0) != 0


def test_ncc_loss_gaussian_constructs_and_checks_sigma():
    from dfmir_amd import ops
    from dfmir_amd._lib import DfmirHipError
    from dfmir_amd.losses import NCC_Loss
    crit = NCC_Loss('cpu', kernel_type='gaussian')
    assert crit.kernel_type == 'gaussian' and crit.kernel_var is None and crit.name == 'ncc'
    NCC_Loss('cpu', kernel_type='gaussian', kernel_var=[10, 7])           # only kernel_var[0] is read, as in the reference
    with pytest.raises(NotImplementedError):
        NCC_Loss('cpu', kernel_type='linear')
    for bad in (0, -3, 11, 2.5, 3.0, '3', True):
        with pytest.raises(ValueError, match="sigma"):
            NCC_Loss('cpu', kernel_type='gaussian', kernel_var=[bad, bad])
        with pytest.raises(ValueError, match="sigma"):
            ops.ncc_loss(torch.rand(1, 1, 8, 8), torch.rand(1, 1, 8, 8), kernel='gaussian', sigma=bad)
    with pytest.raises(ValueError, match="kernel"):
        ops.ncc_loss(torch.rand(1, 1, 8, 8), torch.rand(1, 1, 8, 8), kernel='linear')
    with pytest.raises(DfmirHipError, match="no CPU fallback"):          # the kernels are the only path
        crit(torch.rand(1, 1, 8, 8), torch.rand(1, 1, 8, 8))
    assert [ops.ncc_gauss_window(s)[1] for s in (1, 2, 3, 4, 5, 10)] == [3, 7, 9, 13, 15, 31]


def test_ncc_gauss_host_taps_reproduce_the_reference_window_sum(golden):
    """c * (sum g)^2 of the host tap builder against the reference's own fp32 `torch.sum(filt)`, sigma = 1..5.  The
    reference rounds each of its K^2 weights to fp32 (its exp and products: a few ulp each, <= 4 * 2^-24 relative, and the
    same sign is not guaranteed, so they bound the sum's relative error alike) and adds them in fp32 (<= (K^2 - 1) * 2^-24
    relative for positive terms): (K^2 + 3) * 2^-24 in all."""
    from dfmir_amd import ops
    g = golden("ncc_gauss.npz")
    sums = g["ref_sum_filt"]
    assert sums.dtype == np.float32 and list(g["ref_sum_filt_sigma"]) == [1, 2, 3, 4, 5]
    for sigma, ref in zip((1, 2, 3, 4, 5), sums):
        taps, K, c = ops.ncc_gauss_window(sigma)
        assert taps.dtype == np.float32 and len(taps) == K and taps[K // 2] == 1.0 and np.array_equal(taps, taps[::-1])
        got = c * float(taps.astype(np.float64).sum()) ** 2
        assert abs(got - float(ref)) <= (K * K + 3) * 2.0 ** -24 * float(ref), (sigma, got, float(ref))
    assert abs(float(sums[2]) - 5.668127) < 1e-6


def test_registration_models_reject_an_unknown_ncc_kernel():
    from dfmir_amd.options import default_options
    from dfmir_amd.registration3d import Registration3DModel
    with pytest.raises(ValueError, match="ncc_kernel"):
        Registration3DModel((8, 8, 8), device='cpu', ncc_kernel='box')
    m = Registration3DModel((8, 8, 8), device='cpu', ncc_kernel='gaussian', ncc_sigma=2)
    assert m.criterionNCC.kernel_type == 'gaussian' and m.criterionNCC.kernel_var[0] == 2
    assert Registration3DModel((8, 8, 8), device='cpu').criterionNCC.kernel_type == 'mean'
    opt = default_options()
    assert opt.ncc_kernel_type == 'mean' and opt.ncc_sigma == 3


def test_registration_model_reads_the_ncc_kernel_options():
    """REGISTRATIONModel constructs its NCC criterion from opt.ncc_kernel_type / opt.ncc_sigma (it never calls it, as the
    reference never calls its own); options without the two keys give the mean window."""
    from dfmir_amd.options import default_options
    from dfmir_amd.registration_model import REGISTRATIONModel
    small = dict(gpu_ids=[], crop_size=32, load_size=32, ngf=8)
    m = REGISTRATIONModel(default_options(ncc_kernel_type='gaussian', ncc_sigma=2, **small))
    assert m.criterionNCC.kernel_type == 'gaussian' and m.criterionNCC.kernel_var == [2, 2]
    with pytest.raises(ValueError, match="ncc_kernel_type"):
        REGISTRATIONModel(default_options(ncc_kernel_type='box', **small))
    with pytest.raises(ValueError, match="sigma"):
        REGISTRATIONModel(default_options(ncc_kernel_type='gaussian', ncc_sigma=11, **small))
    opt = default_options(**small)
    del opt.ncc_kernel_type, opt.ncc_sigma
    crit = REGISTRATIONModel(opt).criterionNCC
    assert crit.kernel_type == 'mean' and crit.kernel_var == [9, 9]


# ------------------------------------------------------------------------------------------ GPU: fixture
def _run(I, J, sigma, mask=None, reduction='neg_sqrt_mean'):
    from dfmir_amd import ops
    x = I.to(DEV).requires_grad_()
    loss = ops.ncc_loss(x, J.to(DEV), mask=None if mask is None else mask.to(DEV), reduction=reduction, kernel='gaussian',
                        sigma=sigma)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), x.grad.cpu()


def _case(g, tag):
    I, J = torch.from_numpy(g[tag + "_pred"]), torch.from_numpy(g[tag + "_target"])
    mask = torch.from_numpy(g[tag + "_mask"]) if tag + "_mask" in g.files else None
    return I, J, int(g[tag + "_sigma"]), mask


@pytest.fixture(scope="module")
def fixture_runs(golden):
    """Every fixture case once: (inputs, the kernels' loss and gradient, the float64 restatement's)."""
    g = golden("ncc_gauss.npz")
    runs = {}
    for tag in (str(t) for t in g["cases"]):
        I, J, sigma, mask = _case(g, tag)
        runs[tag] = ((I, J, sigma, mask), _run(I, J, sigma, mask), ncc_gauss_ref64(I, J, sigma, mask))
    return g, runs


@pytest.mark.gpu
def test_ncc_gauss_golden(fixture_runs):
    """Every case of ncc_gauss.npz through NCC_Loss's path against the reference's own loss and d / d prediction."""
    from dfmir_amd.losses import NCC_Loss
    g, runs = fixture_runs
    for tag, ((I, J, sigma, mask), (loss, grad), _) in runs.items():
        bl, bg = _bounds(g, tag)
        x = I.to(DEV).requires_grad_()
        l2 = NCC_Loss(DEV, kernel_var=[sigma, sigma], kernel_type='gaussian')(x, J.to(DEV), mask=None if mask is None else mask.to(DEV))
        l2.backward()
        assert torch.equal(l2.detach().cpu(), loss) and torch.equal(x.grad.cpu(), grad), tag      # = ops.ncc_loss, bit for bit
        ref_l, ref_g = float(g[tag + "_loss"]), g[tag + "_dpred"]
        if mask is not None and float(mask.sum()) == 0.0:
            assert float(loss) == 0.0 and ref_l == 0.0 and float(grad.abs().max()) == 0.0, tag
            continue
        el, eg = rel_errors(loss, grad, ref_l, ref_g)
        print("golden %-10s loss %.3e (<= %.3e)  grad %.3e (<= %.3e)" % (tag, el, bl, eg, bg))
        assert el <= bl and eg <= bg, (tag, el, bl, eg, bg)


@pytest.mark.gpu
def test_ncc_gauss_2d_vs_float64(fixture_runs):
    g, runs = fixture_runs
    for tag, (inp, (loss, grad), (l64, g64)) in runs.items():
        bl, bg = _bounds(g, tag)
        if l64 == 0.0:
            assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0, tag
            continue
        el, eg = rel_errors(loss, grad, l64, g64)
        print("fp64   %-10s loss %.3e (<= %.3e)  grad %.3e (<= %.3e)" % (tag, el, bl, eg, bg))
        assert el <= bl and eg <= bg, (tag, el, bl, eg, bg)


def _pair(seed, shape):
    J = C.rand(seed, *shape)
    return 0.6 * C.rand(seed + 1, *shape) + 0.4 * J, J


CASES_3D = [("d10", (1, 1, 10, 12, 14), 3, False, 'neg_sqrt_mean'),          # D close to K
            ("d5_b2", (2, 1, 5, 9, 11), 3, False, 'neg_sqrt_mean'),            # D < K, batch 2
            ("one_plane", (1, 1, 1, 12, 14), 3, False, 'neg_sqrt_mean'),       # keeps the 3-D window and win_size
            ("s2_mask", (1, 1, 10, 12, 14), 2, True, 'neg_sqrt_mean'),         # the per-axis path, masked
            ("s2_mask_mean", (1, 1, 10, 12, 14), 2, True, 'neg_mean')]


@pytest.mark.gpu
@pytest.mark.parametrize("tag,shape,sigma,masked,reduction", CASES_3D, ids=[c[0] for c in CASES_3D])
def test_ncc_gauss_3d_vs_float64(golden, tag, shape, sigma, masked, reduction):
    """The build-defined 3-D window c * g (x) g (x) g against its float64 restatement (F.conv3d in double)."""
    bl, bg = _bounds(golden("ncc_gauss.npz"))
    I, J = _pair(300 + 10 * len(tag), shape)
    mask = (C.rand(77, *shape) > 0.4).float() if masked else None
    loss, grad = _run(I, J, sigma, mask, reduction)
    l64, g64 = ncc_gauss_ref64(I, J, sigma, mask, reduction=reduction)
    el, eg = rel_errors(loss, grad, l64, g64)
    print("fp64   %-12s loss %.3e (<= %.3e)  grad %.3e (<= %.3e)" % (tag, el, bl, eg, bg))
    assert el <= bl and eg <= bg, (tag, el, bl, eg, bg)
    if tag == "one_plane":                       # not the 2-D image's loss: win_size is the full 3-D sum
        l2d, _ = _run(I[:, :, 0], J[:, :, 0], sigma)
        assert abs(float(l2d) - float(loss)) > 1e-3 * abs(float(loss))


@pytest.mark.gpu
@pytest.mark.parametrize("reduction", ['neg_sqrt_mean', 'neg_mean'])
@pytest.mark.parametrize("shape,mshape", [((2, 1, 24, 20), (1, 1, 24, 20)), ((3, 1, 6, 9, 11), (1, 1, 6, 9, 11))], ids=["2d", "3d"])
def test_ncc_gauss_broadcast_mask_normalises_by_its_own_sum(golden, shape, mshape, reduction):
    """A mask broadcast r-fold over the batch: sum(cc m) runs over the batch, sum(m) over the mask as given
    (util/losses.py:260-261) -- sqrt(r) resp. r times the loss over the expanded mask, in the value and in the gradient."""
    bl, bg = _bounds(golden("ncc_gauss.npz"))
    I, J = _pair(431, shape)
    mask = (C.rand(79, *mshape) > 0.4).float()
    loss, grad = _run(I, J, 3, mask, reduction)
    l64, g64 = ncc_gauss_ref64(I, J, 3, mask, reduction=reduction)
    el, eg = rel_errors(loss, grad, l64, g64)
    print("fp64   bcast %-13s %s loss %.3e (<= %.3e)  grad %.3e (<= %.3e)" % (reduction, "x".join(map(str, shape)), el, bl, eg, bg))
    assert el <= bl and eg <= bg, (el, bl, eg, bg)
    full, _ = _run(I, J, 3, mask.expand(shape).contiguous(), reduction)
    r = float(shape[0])
    assert abs(float(loss) / float(full) - (r if reduction == 'neg_mean' else r ** 0.5)) < 1e-6


@pytest.mark.gpu
def test_ncc_gauss_is_bit_reproducible():
    for shape, sigma in (((2, 1, 33, 70), 3), ((2, 1, 33, 70), 2), ((1, 1, 10, 12, 14), 3), ((1, 1, 10, 12, 14), 1)):
        I, J = _pair(401, shape)
        mask = (C.rand(78, *shape) > 0.4).float()
        for m in (None, mask):
            a, b = _run(I, J, sigma, m), _run(I, J, sigma, m)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (shape, sigma)
            assert float(a[0]) < 0.0 and float(a[1].abs().max()) > 0.0


# ------------------------------------------------------------------------------------------ GPU: the 3-D model
def _volumes(shape):
    A = C.rand(141, 1, 1, *shape)
    return A, 0.5 * A + 0.5 * C.rand(142, 1, 1, *shape)


@pytest.mark.gpu
def test_registration3d_gaussian_step_and_unchanged_default(golden):
    """The 'ncc' loss of a Gaussian step is the float64 restatement on the model's own warped image; ncc_kernel='mean' is
    the model without the argument."""
    from dfmir_amd.registration3d import Registration3DModel
    shape = (16, 16, 16)
    A, B = _volumes(shape)

    def first_step(**kw):
        torch.manual_seed(0)
        m = Registration3DModel(shape, None, device=DEV, **kw)
        with torch.no_grad():
            m.netR.flow.weight.mul_(3e4)           # a flow of voxels, not of 1e-5 voxels
        m.set_input({"A": A, "B": B}); m.optimize_parameters()
        torch.cuda.synchronize()
        return m, m.get_current_losses()

    m, got = first_step(ncc_kernel='gaussian')
    assert sorted(got) == ["grad", "ncc"] and float(m.flow.abs().max()) > 1e-3
    l64, _ = ncc_gauss_ref64(m.regA, B, 3)
    bl, _ = _bounds(golden("ncc_gauss.npz"))
    err = abs(got["ncc"] - l64) / abs(l64)
    print("model  16^3 step-one loss %.3e (<= %.3e)" % (err, bl))
    assert err <= bl, (got["ncc"], l64, err, bl)
    _, default = first_step()
    _, mean = first_step(ncc_kernel='mean')
    assert default == mean and abs(default["ncc"] - got["ncc"]) > 1e-4


@pytest.mark.gpu
def test_registration3d_gaussian_captured_step_matches_eager():
    """ncc_kernel='gaussian' under capture_step=True, by the criterion of test_registration3d_captured_step_matches_eager:
    two eager steps, the capture, then each replayed step equals the same step enqueued eagerly from the restored state."""
    from dfmir_amd.registration3d import Registration3DModel
    from tests import step3d
    shape = (16, 16, 16)
    torch.manual_seed(0)
    m = Registration3DModel(shape, None, capture_step=True, device=DEV, ncc_kernel='gaussian')
    A, B = (t.to(DEV) for t in _volumes(shape))
    refs = step3d.assert_replay_matches_eager(m, {"A": A, "B": B}, ["grad", "ncc"])
    assert all(r["ncc"] < 0.0 for r in refs)
