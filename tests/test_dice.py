"""Label-map Dice under a flow (dfmir_amd/csrc/dice.hip: ops.warp_dice, losses.LabelDice), the dense vxm Dice / MSE, and
Registration3DModel(seg_labels=..., seg_weight=...): the C ABI and the argument checks (CPU), the reference's own losses
and gradients (tests/golden/dice.npz), the one-hot composition the tree could already run, a float64 restatement of the
formula at the full 3-D size, run-to-run bit-reproducibility, and the 3-D model against the oracle step.

Bounds of the GPU comparisons: at most 2x the worst error measured on the MI355X (profiles/dice_parity_margins.txt), under
the ceilings test_losses_golden uses for NCC (1e-4 on a loss, 1e-3 on a gradient)."""
import inspect
import os

import numpy as np
import pytest
import torch

from tests.golden import common as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
NAMES = ("dfmir_warp_dice_ws_floats", "dfmir_warp_dice_fwd", "dfmir_warp_dice_bwd", "dfmir_dice_ws_floats",
         "dfmir_dice_fwd", "dfmir_dice_bwd", "dfmir_mse_ws_floats", "dfmir_mse_fwd", "dfmir_mse_bwd")


# ------------------------------------------------------------------------------------------ float64 restatement
def warp_dice_ref64(mov, fix, flow, labels, mode="bilinear", chunk=1 << 20, want_grad=True):
    """(loss, dice[B,K], d loss / d flow) in float64 on the CPU, written from the formulas (not from the reference's code):
    p = x + flow(x) -- taken as the fp32 sum, the one rounding the kernel makes, so the cell is the same --, its 2^nd corners
    c_k with the multi-linear weights w_k (0 outside the volume);
    T[b,l] = sum_x sum_k w_k [mov(c_k) = l][fix(x) = l], S[b,l] = sum_x sum_k w_k [mov(c_k) = l], N[b,l] = #{fix(x) = l},
    dice = 2 T / max(N + S, 1e-5), loss = -mean dice; d loss / d flow_a(x) = sum_k dw_k/dp_a (gT[m_k][m_k = fix(x)] + gS[m_k])
    with gT = -2 / (bottom B K), gS = 2 T / (bottom^2 B K) where the clamp is inactive.  Voxels are streamed in chunks."""
    B, vol = flow.shape[0], tuple(flow.shape[2:])
    nd, K, S = len(vol), len(labels), int(np.prod(vol))
    table = torch.full((256,), K, dtype=torch.long)          # slot K: not scored
    for i, l in enumerate(labels):
        table[int(l)] = i
    mslot = table[mov.detach().cpu().long().reshape(B, S)]
    fslot = table[fix.detach().cpu().long().reshape(B, S)]
    fl = flow.detach().cpu().float().reshape(B, nd, S)
    strides = [int(np.prod(vol[a + 1:])) for a in range(nd)]

    def cells(b, s0, s1):
        """per corner: (linear index, valid, weight, [d weight / d p_a])"""
        idx = torch.arange(s0, s1)
        out, rem = [], idx
        for a in range(nd):
            out.append((rem // strides[a]).float())
            rem = rem % strides[a]
        p = torch.stack([(out[a] + fl[b, a, s0:s1]).double() for a in range(nd)])       # fp32 sum, then float64
        if mode == "nearest":
            c = torch.round(p).long()                                                    # half to even, as nearbyintf
            valid = torch.ones(s1 - s0, dtype=torch.bool)
            lin = torch.zeros(s1 - s0, dtype=torch.long)
            for a in range(nd):
                valid &= (c[a] >= 0) & (c[a] < vol[a])
                lin += c[a].clamp(0, vol[a] - 1) * strides[a]
            yield lin, valid, torch.ones(s1 - s0, dtype=torch.float64), None
            return
        p0 = torch.floor(p)
        w1 = p - p0
        c0 = p0.long()
        for k in range(1 << nd):
            offs = [(k >> (nd - 1 - a)) & 1 for a in range(nd)]
            valid = torch.ones(s1 - s0, dtype=torch.bool)
            lin = torch.zeros(s1 - s0, dtype=torch.long)
            fac = []
            for a in range(nd):
                ca = c0[a] + offs[a]
                valid &= (ca >= 0) & (ca < vol[a])
                lin += ca.clamp(0, vol[a] - 1) * strides[a]
                fac.append(w1[a] if offs[a] else 1.0 - w1[a])
            w = fac[0].clone()
            for a in range(1, nd):
                w = w * fac[a]
            dw = []
            for a in range(nd):
                d = torch.full_like(w, 1.0 if offs[a] else -1.0)
                for a2 in range(nd):
                    if a2 != a:
                        d = d * fac[a2]
                dw.append(d)
            yield lin, valid, w, dw

    T = torch.zeros(B, K + 1, dtype=torch.float64)
    Ssum = torch.zeros(B, K + 1, dtype=torch.float64)
    N = torch.zeros(B, K + 1, dtype=torch.float64)
    for b in range(B):
        N[b] = torch.bincount(fslot[b], minlength=K + 1).double()
        for s0 in range(0, S, chunk):
            s1 = min(S, s0 + chunk)
            f = fslot[b, s0:s1]
            for lin, valid, w, _ in cells(b, s0, s1):
                m = torch.where(valid, mslot[b][lin], torch.full_like(lin, K))
                Ssum[b].index_add_(0, m, w)
                T[b].index_add_(0, m, w * (m == f))
    T, Ssum, N = T[:, :K], Ssum[:, :K], N[:, :K]
    bs = N + Ssum
    active = bs >= 1e-5
    bottom = torch.where(active, bs, torch.full_like(bs, 1e-5))
    dice = 2 * T / bottom
    loss = -float(dice.mean())
    if not want_grad or mode == "nearest":
        return loss, dice, None
    zero = torch.zeros(B, 1, dtype=torch.float64)
    gT = torch.cat([-2.0 / bottom / (B * K), zero], 1)
    gS = torch.cat([torch.where(active, 2 * T / bottom ** 2 / (B * K), torch.zeros_like(T)), zero], 1)
    dflow = torch.zeros(B, nd, S, dtype=torch.float64)
    for b in range(B):
        for s0 in range(0, S, chunk):
            s1 = min(S, s0 + chunk)
            f = fslot[b, s0:s1]
            for lin, valid, w, dw in cells(b, s0, s1):
                m = torch.where(valid, mslot[b][lin], torch.full_like(lin, K))
                G = gT[b][m] * (m == f) + gS[b][m]
                for a in range(nd):
                    dflow[b, a, s0:s1] += dw[a] * G
    return loss, dice, dflow.view(flow.shape)


def one_hot(x, labels):
    return torch.cat([(x == int(l)).float() for l in labels], 1)


def blocky_labels(seed, B, vol, nvals, block):
    coarse = [-(-s // block) for s in vol]
    x = (C.rand(seed, B, 1, *coarse) * nvals).long().clamp_(max=nvals - 1)
    for ax in range(len(vol)):
        x = x.repeat_interleave(block, dim=2 + ax)
    return x[(slice(None), slice(None)) + tuple(slice(0, s) for s in vol)].to(torch.uint8).contiguous()


# ------------------------------------------------------------------------------------------ CPU tier
def test_dice_symbols_in_header_exports_and_ctypes_table():
    import ctypes
    import dfmir_amd
    from dfmir_amd import _lib
    from tests.test_abi import header_symbols
    h = ctypes.CDLL(dfmir_amd.LIB_PATH)
    for s in NAMES:
        assert s in header_symbols() and s in _lib.exported_symbols() and hasattr(h, s), s
    assert dfmir_amd.lib().dfmir_abi_version() == 14


def test_dice_workspace_queries_and_bad_arguments_touch_no_device():
    import dfmir_amd
    lib = dfmir_amd.lib()
    q = lib.dfmir_warp_dice_ws_floats
    for bad in ((4, 1, 8, 4, 4, 4), (1, 1, 8, 4, 4, 4), (3, 0, 8, 4, 4, 4), (3, 1, 0, 4, 4, 4), (3, 1, 65, 4, 4, 4),
                (3, 1, 8, 0, 4, 4), (3, 1, 8, 4, -1, 4), (3, 1, 8, 4, 4, 0), (2, 1, 8, 2, 4, 4), (3, 1, 8, 2048, 2048, 1024)):
        assert q(*bad) == -1, bad
    assert q(3, 1, 35, 160, 192, 224) >= 2 * 3 * 35 and q(2, 2, 1, 1, 24, 21) >= 2 * 2 * 3
    assert q(3, 1, 64, 160, 192, 224) * 4 < 4 << 20              # partial slots stay a few MB at most
    assert lib.dfmir_dice_ws_floats(0, 10) == -1 and lib.dfmir_dice_ws_floats(3, 0) == -1
    assert lib.dfmir_dice_ws_floats(35, 1 << 22) >= 35 * 4
    assert lib.dfmir_mse_ws_floats(0) == -1 and lib.dfmir_mse_ws_floats(1000) >= 2
    for rc in (lib.dfmir_warp_dice_fwd(3, None, None, None, None, 8, 1, 4, 4, 4, 0, None, None, None, None, None),
               lib.dfmir_warp_dice_bwd(3, None, None, None, None, 8, 1, 4, 4, 4, None, None, None, None),
               lib.dfmir_dice_fwd(None, None, 2, 10, None, None, None),
               lib.dfmir_dice_bwd(None, None, 2, 10, None, None, None, None, None),
               lib.dfmir_mse_fwd(None, None, 10, None, None, None),
               lib.dfmir_mse_bwd(None, None, 10, None, None, None, None)):
        assert rc != 0
        assert b"invalid argument" in lib.dfmir_last_error()


def test_warp_dice_rejects_bad_arguments_before_any_launch():
    from dfmir_amd import ops
    from dfmir_amd._lib import DfmirHipError
    from dfmir_amd.losses import Dice, LabelDice, MSE
    mov = torch.zeros(1, 1, 8, 8, dtype=torch.uint8)
    flow = torch.zeros(1, 2, 8, 8)
    with pytest.raises(DfmirHipError, match="no CPU fallback"):
        ops.warp_dice(mov, mov, flow, [1, 2])
    with pytest.raises(DfmirHipError, match="do not match"):
        ops.warp_dice(mov, torch.zeros(1, 1, 8, 9, dtype=torch.uint8), flow, [1, 2])
    with pytest.raises(DfmirHipError, match="do not match"):
        ops.warp_dice(torch.zeros(2, 1, 8, 8, dtype=torch.uint8), mov, flow, [1, 2])
    with pytest.raises(DfmirHipError, match="nd = 2 or 3"):
        ops.warp_dice(mov, mov, torch.zeros(1, 3, 8, 8), [1])
    with pytest.raises(DfmirHipError, match="1 to 64"):
        ops.warp_dice(mov, mov, flow, list(range(65)))
    with pytest.raises(DfmirHipError, match="1 to 64"):
        ops.warp_dice(mov, mov, flow, [])
    with pytest.raises(DfmirHipError, match="duplicate"):
        ops.warp_dice(mov, mov, flow, [1, 2, 1])
    for bad in ([256], [-1], [1.5]):
        with pytest.raises(DfmirHipError, match=r"\[0, 255\]"):
            ops.warp_dice(mov, mov, flow, bad)
    with pytest.raises(DfmirHipError, match="uint8"):
        ops.warp_dice(mov.long(), mov, flow, [1])
    with pytest.raises(DfmirHipError, match="mode"):
        ops.warp_dice(mov, mov, flow, [1], mode="cubic")
    with pytest.raises(DfmirHipError, match="nearest"):
        ops.warp_dice(mov, mov, flow.clone().requires_grad_(), [1], mode="nearest")
    with pytest.raises(DfmirHipError, match="duplicate"):
        LabelDice([3, 3])
    with pytest.raises(ValueError, match="mode"):
        LabelDice([1], mode="cubic")
    crit = LabelDice(np.arange(1, 5))
    assert crit.labels == [1, 2, 3, 4] and crit.mode == "bilinear" and crit.scores is None
    with pytest.raises(DfmirHipError, match="no CPU fallback"):
        crit.loss(mov, mov.long(), flow)
    x = torch.rand(1, 2, 8, 8)
    for fn in (ops.dice_loss, ops.mse_loss, Dice().loss, MSE().loss):
        with pytest.raises(DfmirHipError, match="no CPU fallback"):
            fn(x, x)
        with pytest.raises(DfmirHipError, match="one shape"):
            fn(x, x[:, :1])
    from dfmir_amd.voxelmorph import losses as vxm_losses
    assert vxm_losses.Dice is Dice and vxm_losses.MSE is MSE


def test_as_label_map_checks_range_and_dtype():
    from dfmir_amd import ops
    from dfmir_amd._lib import DfmirHipError
    for t in (torch.tensor([[0, 3, 255]]), torch.tensor([[0, 3, 255]], dtype=torch.int16), torch.tensor([[0.0, 3.0, 255.0]]),
              torch.tensor([[0, 3, 255]], dtype=torch.uint8).t(), torch.tensor([True, False])):
        u = ops.as_label_map(t)
        assert u.dtype == torch.uint8 and u.is_contiguous() and u.device == t.device
        assert torch.equal(u.long(), t.long())
    for bad in (torch.tensor([0, 256]), torch.tensor([-1, 3]), torch.tensor([0.5, 1.0]), torch.tensor([float("nan")]),
                torch.tensor([1.0, 300.0])):
        with pytest.raises(DfmirHipError):
            ops.as_label_map(bad)
    with pytest.raises(DfmirHipError):
        ops.as_label_map([1, 2])


def test_registration3d_seg_arguments_cpu():
    from dfmir_amd._lib import DfmirHipError
    from dfmir_amd.registration3d import Registration3DModel
    with pytest.raises(DfmirHipError, match="duplicate"):
        Registration3DModel((8, 8, 8), device="cpu", seg_labels=[1, 1])
    with pytest.raises(DfmirHipError, match="1 to 64"):
        Registration3DModel((8, 8, 8), device="cpu", seg_labels=list(range(70)))
    m = Registration3DModel((8, 8, 8), device="cpu", seg_labels=[1, 2], seg_weight=0.5)
    A = torch.rand(1, 1, 8, 8, 8)
    seg = torch.zeros(1, 1, 8, 8, 8, dtype=torch.long)
    with pytest.raises(KeyError, match="A_seg"):
        m.set_input({"A": A, "B": A})
    with pytest.raises(KeyError, match="B_seg"):
        m.set_input({"A": A, "B": A, "A_seg": seg})
    with pytest.raises(DfmirHipError, match=r"\[0, 255\]"):
        m.set_input({"A": A, "B": A, "A_seg": seg + 300, "B_seg": seg})
    m.set_input({"A": A, "B": A, "A_seg": seg, "B_seg": seg.float()})
    assert m.seg_A.dtype == torch.uint8 and m.seg_B.dtype == torch.uint8
    plain = Registration3DModel((8, 8, 8), device="cpu")
    assert plain.seg_labels is None and plain._outputs == ('regA', 'flow', 'loss_ncc', 'loss_grad')
    plain.set_input({"A": A, "B": A})                                 # no segmentation asked for, none needed


def test_register_pair_signature_is_backwards_compatible():
    from dfmir_amd.infer import register_pair
    ps = list(inspect.signature(register_pair).parameters.values())
    assert [p.name for p in ps] == ["model", "data", "label", "fixed_label", "labels"]
    assert [p.default for p in ps[2:]] == [None, None, None]
    from dfmir_amd import test as driver
    assert driver.parse(["--dataroot", "x"]).fixed_label_dir is None
    assert driver.parse(["--dataroot", "x", "--fixed_label_dir", "trainB_label"]).fixed_label_dir == "trainB_label"


# Bounds: 2x the worst relative error measured on the MI355X per tensor class (profiles/dice_parity_margins.txt; the kernels
# are bit-reproducible, so the measured figures repeat).  The ceilings are 1e-4 (loss) and 1e-3 (gradient).
LOSS_RTOL = 3.0e-7           # measured 1.52e-7 (2d_b1_k1_w4)
TABLE_RTOL = 5.4e-7          # measured 2.74e-7 (3d_b2_k64_w4)
DFLOW_RTOL = 3.9e-6          # measured 1.98e-6 (2d_b1_k1_w4; the reference's own fp32 d(flow) is 1.9e-6 off float64 there)
DENSE_LOSS_RTOL = 2.2e-7     # measured 1.12e-7
DENSE_GRAD_RTOL = 4.7e-7     # measured 2.38e-7
FULL_LOSS_RTOL = 5.5e-7      # measured 2.80e-7 (K = 64)
FULL_TABLE_RTOL = 1.4e-7     # measured 7.40e-8
FULL_DFLOW_RTOL = 4.5e-7     # measured 2.27e-7
COMP_LOSS_RTOL = 1.7e-7      # measured 8.70e-8
COMP_DFLOW_RTOL = 4.9e-7     # measured 2.48e-7


# ------------------------------------------------------------------------------------------ GPU: fixture
def _case(g, tag):
    mov = torch.from_numpy(g[tag + "_mov"]).to(DEV)
    fix = torch.from_numpy(g[tag + "_fix"]).to(DEV)
    flow = torch.from_numpy(g[tag + "_flow"]).to(DEV)
    return mov, fix, flow, [int(v) for v in g[tag + "_labels"]], "nearest" if int(g[tag + "_mode"]) else "bilinear"


@pytest.mark.gpu
def test_warp_dice_golden(golden):
    """Every label case of dice.npz: loss, dice table and d(flow) -- every element -- against the reference's one-hot
    composition (SpatialTransformer + Dice, autograd through both)."""
    from dfmir_amd.losses import LabelDice
    from tests.test_gpu_ops import close
    g = golden("dice.npz")
    for tag in [str(t) for t in g["cases"]]:
        mov, fix, flow, labels, mode = _case(g, tag)
        flow.requires_grad_(mode == "bilinear")
        crit = LabelDice(labels, mode=mode)
        loss = crit.loss(fix, mov, flow)
        assert loss.shape == () and crit.scores.shape == (flow.shape[0], len(labels)) and not crit.scores.requires_grad
        close(loss, g[tag + "_loss"], rtol=LOSS_RTOL, atol=0, what=tag + " loss")
        close(crit.scores, g[tag + "_dice"], rtol=TABLE_RTOL, atol=0, what=tag + " dice table")
        if mode == "bilinear":
            loss.backward()
            close(flow.grad, g[tag + "_dflow"], rtol=DFLOW_RTOL, atol=0, what=tag + " d flow")
        else:
            assert not loss.requires_grad


@pytest.mark.gpu
def test_dense_dice_and_mse_golden(golden):
    """vxm Dice / MSE of float tensors against the reference: the loss and the gradients of both arguments (one channel is
    empty in both tensors: the clamp of the denominator is active there)."""
    from dfmir_amd.losses import Dice, MSE
    from tests.test_gpu_ops import close
    g = golden("dice.npz")
    for tag in [str(t) for t in g["dense_cases"]]:
        for name, crit in (("dice", Dice()), ("mse", MSE())):
            t = torch.from_numpy(g[tag + "_true"]).to(DEV).requires_grad_()
            p = torch.from_numpy(g[tag + "_pred"]).to(DEV).requires_grad_()
            loss = crit.loss(t, p)
            loss.backward()
            assert loss.shape == ()
            close(loss, g["%s_%s_loss" % (tag, name)], rtol=DENSE_LOSS_RTOL, atol=0, what="%s %s loss" % (tag, name))
            close(t.grad, g["%s_%s_dtrue" % (tag, name)], rtol=DENSE_GRAD_RTOL, atol=0, what="%s %s d y_true" % (tag, name))
            close(p.grad, g["%s_%s_dpred" % (tag, name)], rtol=DENSE_GRAD_RTOL, atol=0, what="%s %s d y_pred" % (tag, name))
            # a gradient to one argument only
            t2 = torch.from_numpy(g[tag + "_true"]).to(DEV)
            p2 = torch.from_numpy(g[tag + "_pred"]).to(DEV).requires_grad_()
            crit.loss(t2, p2).backward()
            assert torch.equal(p2.grad, p.grad) and t2.grad is None


@pytest.mark.gpu
def test_warp_dice_equals_the_one_hot_composition():
    """ops.warp of the one-hot moving map followed by the dense Dice -- what the tree could already compose -- against the
    fused kernels at 64^3 with K = 35: loss and d(flow)."""
    from dfmir_amd import ops
    from tests.test_gpu_ops import close
    vol, labels = (64, 64, 64), list(range(1, 36))
    mov = blocky_labels(501, 1, vol, 40, 4).to(DEV)
    fix = torch.where(C.rand(503, 1, 1, *vol).to(DEV) < 0.6, mov, blocky_labels(502, 1, vol, 40, 4).to(DEV))
    flow0 = ((C.rand(504, 1, 3, *vol) * 2 - 1) * 3.0).to(DEV)
    flow = flow0.clone().requires_grad_()
    loss, table = ops.warp_dice(mov, fix, flow, labels)
    loss.backward()
    flow2 = flow0.clone().requires_grad_()
    warped = ops.warp(one_hot(mov, labels), flow2)
    loss2 = ops.dice_loss(one_hot(fix, labels), warped)
    loss2.backward()
    close(loss, loss2, rtol=COMP_LOSS_RTOL, atol=0, what="composition loss")
    close(flow.grad, flow2.grad, rtol=COMP_DFLOW_RTOL, atol=0, what="composition d flow")
    assert float(flow.grad.abs().max()) > 0


@pytest.mark.gpu
def test_warp_dice_gradient_is_zero_where_no_corner_is_scored(golden):
    """d(flow) is exactly 0 at voxels whose 2^nd corners are all unscored or outside the volume, and not elsewhere."""
    from dfmir_amd import ops
    g = golden("dice.npz")
    seen = 0
    for tag in [str(t) for t in g["cases"]]:
        mov, fix, flow, labels, mode = _case(g, tag)
        if mode != "bilinear":
            continue
        flow.requires_grad_()
        ops.warp_dice(mov, fix, flow, labels)[0].backward()
        nd, vol = flow.shape[1], tuple(flow.shape[2:])
        scored = torch.zeros(256, dtype=torch.bool, device=DEV)
        scored[torch.tensor(labels, device=DEV)] = True
        grid = torch.stack(torch.meshgrid([torch.arange(s, device=DEV, dtype=torch.float32) for s in vol], indexing="ij"))[None]
        p0 = torch.floor(grid + flow.detach()).long()
        dead = torch.ones((flow.shape[0],) + vol, dtype=torch.bool, device=DEV)
        for k in range(1 << nd):
            c = [p0[:, a] + ((k >> a) & 1) for a in range(nd)]
            valid = torch.ones_like(dead)
            for a in range(nd):
                valid &= (c[a] >= 0) & (c[a] < vol[a])
            idx = tuple(c[a].clamp(0, vol[a] - 1) for a in range(nd))
            for b in range(flow.shape[0]):
                lab = mov[b, 0][tuple(i[b] for i in idx)].long()
                dead[b] &= ~(valid[b] & scored[lab])
        dead = dead[:, None].expand_as(flow)
        assert bool(dead.any()), tag
        assert float(flow.grad[dead].abs().max()) == 0.0, tag
        assert float(flow.grad[~dead].abs().max()) > 0.0, tag
        seen += 1
    assert seen >= 4


@pytest.mark.gpu
def test_warp_dice_nearest_is_the_hard_dice_of_the_label_warp():
    """mode='nearest' against the hard Dice computed from SpatialTransformer(mode='nearest') of the tree on the same flow."""
    from dfmir_amd import ops
    from dfmir_amd.voxelmorph import SpatialTransformer
    for vol in ((40, 36, 44), (33, 27)):
        B, labels = 2, [1, 2, 3, 5, 8, 13]
        mov = blocky_labels(511, B, vol, 10, 3).to(DEV)
        fix = torch.where(C.rand(513, B, 1, *vol).to(DEV) < 0.6, mov, blocky_labels(512, B, vol, 10, 3).to(DEV))
        flow = ((C.rand(514, B, len(vol), *vol) * 2 - 1) * 4.0).to(DEV)
        loss, table = ops.warp_dice(mov, fix, flow, labels, mode="nearest")
        assert not loss.requires_grad
        # a background of 0 would be what the zero padding warps in: shift the values so that padding is its own value
        warped = SpatialTransformer(vol, mode="nearest").to(DEV)(mov.float() + 1.0, flow) - 1.0
        axes = tuple(range(2, 2 + len(vol)))
        t, p = one_hot(fix, labels).double(), one_hot(warped, labels).double()
        ref = 2 * (t * p).sum(axes) / torch.clamp((t + p).sum(axes), min=1e-5)
        assert float((table.double() - ref).abs().max()) <= 1e-6 * float(ref.abs().max()), (vol, table, ref)
        assert abs(float(loss) + float(ref.mean())) <= 1e-6 * abs(float(ref.mean()))


# ------------------------------------------------------------------------------------------ GPU: full size
@pytest.mark.gpu
@pytest.mark.parametrize("K", [35, 64])
def test_warp_dice_full_size_vs_float64_and_bit_reproducible(K):
    """1 x 160 x 192 x 224 against the float64 restatement (every voxel); loss, table and d(flow) bit-identical across runs."""
    from dfmir_amd import ops
    from tests.test_gpu_ops import close, near
    vol = (160, 192, 224)
    labels = list(range(1, K + 1))
    mov = blocky_labels(521, 1, vol, K + 6, 8)
    fix = torch.where(C.rand(523, 1, 1, *vol) < 0.7, mov, blocky_labels(522, 1, vol, K + 6, 8))
    flow0 = (C.rand(524, 1, 3, *vol) * 2 - 1) * 3.0
    runs = []
    for _ in range(2):
        flow = flow0.to(DEV).requires_grad_()
        loss, table = ops.warp_dice(mov.to(DEV), fix.to(DEV), flow, labels)
        loss.backward()
        torch.cuda.synchronize()
        runs.append((loss.detach().cpu(), table.cpu(), flow.grad.cpu()))
    for r0, r1 in zip(runs[0], runs[1]):
        assert torch.equal(r0, r1)
    ref_loss, ref_table, ref_dflow = warp_dice_ref64(mov, fix, flow0, labels)
    near(float(runs[0][0]), ref_loss, FULL_LOSS_RTOL, "full-size loss K=%d" % K)
    close(runs[0][1], ref_table, rtol=FULL_TABLE_RTOL, atol=0, what="full-size dice table K=%d" % K)
    close(runs[0][2], ref_dflow, rtol=FULL_DFLOW_RTOL, atol=0, what="full-size d flow K=%d" % K)


# ------------------------------------------------------------------------------------------ GPU: the 3-D model
SEG_LABELS = [1, 2, 3, 4]
SEG_WEIGHT = 0.7


def _seg_pair(shape, seed):
    a = blocky_labels(seed, 1, shape, 6, 4)
    b = torch.where(C.rand(seed + 2, 1, 1, *shape) < 0.7, a, blocky_labels(seed + 1, 1, shape, 6, 4))
    return a, b


def _dice_oracle_step(O):
    class DiceRegistration3DStep(O.Registration3DStep):
        """The oracle's 3-D step plus SEG_WEIGHT * Dice(one_hot(B_seg), warp(one_hot(A_seg), flow)) in torch ops."""

        def step(self, A, B, A_seg, B_seg):
            ys, yt, flow = self.netR(A, B)
            self.opt.zero_grad()
            l_sim = O.ncc_loss(ys, B, self.win)
            l_reg = O.grad_loss_l2(flow)
            t = one_hot(B_seg, SEG_LABELS)
            p = O.spatial_transform(one_hot(A_seg, SEG_LABELS), flow)
            l_dice = -torch.mean(2 * (t * p).sum(dim=(2, 3, 4)) / torch.clamp((t + p).sum(dim=(2, 3, 4)), min=1e-5))
            (l_sim + self.lam * l_reg + SEG_WEIGHT * l_dice).backward()
            self.opt.step()
            self.ys, self.flow = ys, flow
            return dict(ncc=float(l_sim.detach()), grad=float(l_reg.detach()), dice=float(l_dice.detach()))
    return DiceRegistration3DStep


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(32, 32, 32), (128, 128, 128)], ids=["32", "128"])
def test_registration3d_dice_step_vs_oracle(shape):
    from oracle import dfmir_oracle as O
    from dfmir_amd.registration3d import Registration3DModel
    from tests.test_gpu_models import _load
    from tests.test_gpu_ops import close, near
    torch.manual_seed(21)
    st = _dice_oracle_step(O)(shape)
    with torch.no_grad():
        st.netR.flow.weight.mul_(3e4)
    model = Registration3DModel(shape, device=DEV, seg_labels=SEG_LABELS, seg_weight=SEG_WEIGHT)
    _load(model.netR, st.netR)
    for it in range(2):
        A = C.rand(31 + it, 1, 1, *shape)
        B = 0.5 * A + 0.5 * C.rand(41 + it, 1, 1, *shape)
        A_seg, B_seg = _seg_pair(shape, 61 + 10 * it)
        ref = st.step(A, B, A_seg, B_seg)
        model.set_input({"A": A, "B": B, "A_seg": A_seg.long(), "B_seg": B_seg})
        model.optimize_parameters()
        got = model.get_current_losses()
        assert sorted(got) == ["dice", "grad", "ncc"]
        if it == 0:
            close(model.flow, st.flow, what="flow"); close(model.regA, st.ys, what="warped")
            for (k, po), (k2, ph) in zip(st.netR.named_parameters(), model.netR.named_parameters()):
                close(ph.grad, po.grad, rtol=2e-3, atol=1e-9, what="grad " + k)
        for k in ("ncc", "grad", "dice"):
            near(got[k], ref[k], 1e-3, "3-D loss %s step %d" % (k, it), floor=1e-7)


@pytest.mark.gpu
def test_registration3d_dice_captured_step_matches_eager():
    """seg_labels under capture_step=True: a replayed step equals the same step enqueued eagerly; a changed label shape
    re-captures."""
    from dfmir_amd.registration3d import Registration3DModel
    from tests import step3d
    shape = (32, 32, 32)
    torch.manual_seed(0)
    m = Registration3DModel(shape, None, capture_step=True, device=DEV, seg_labels=SEG_LABELS, seg_weight=SEG_WEIGHT)
    m.parallelize()
    A = C.rand(141, 1, 1, *shape).to(DEV)
    B = (0.5 * A + 0.5 * C.rand(142, 1, 1, *shape).to(DEV))
    A_seg, B_seg = (x.to(DEV) for x in _seg_pair(shape, 143))
    data = {"A": A, "B": B, "A_seg": A_seg, "B_seg": B_seg}
    for _ in range(3):                                    # two eager steps, then the capture: the label maps are its buffers
        m.set_input(data); m.optimize_parameters()
    assert m._graph['graph'] is not None
    assert m.seg_A is m._graph['inputs']['seg_A'] and m.seg_B is m._graph['inputs']['seg_B']
    step3d.assert_replay_matches_eager(m, data, ["dice", "grad", "ncc"])


@pytest.mark.gpu
def test_registration3d_without_seg_labels_is_bit_identical():
    """seg_labels=None (the default) against a model constructed without the new arguments: the same parameters, bit for
    bit, after two steps (deterministic weight gradients, so that the comparison means something)."""
    from dfmir_amd import ops
    from dfmir_amd.registration3d import Registration3DModel
    shape = (32, 32, 32)
    A = C.rand(151, 1, 1, *shape).to(DEV)
    B = (0.5 * A + 0.5 * C.rand(152, 1, 1, *shape).to(DEV))
    params = []
    try:
        for kw in ({}, {"seg_labels": None, "seg_weight": 0.0}, {"seg_labels": None, "seg_weight": 3.0}):
            torch.manual_seed(5)
            m = Registration3DModel(shape, device=DEV, deterministic_wgrad=True, **kw)
            with torch.no_grad():
                m.netR.flow.weight.mul_(3e4)
            ops.bump_weights_epoch()
            for _ in range(2):
                m.set_input({"A": A, "B": B})
                m.optimize_parameters()
            torch.cuda.synchronize()
            assert sorted(m.get_current_losses()) == ["grad", "ncc"]
            params.append(m.optimizer_R.flat_p.clone())
    finally:
        ops.set_deterministic_wgrad(False)
    assert float(params[0].abs().sum()) > 0
    assert torch.equal(params[0], params[1]) and torch.equal(params[0], params[2])


@pytest.mark.gpu
def test_register_pair_scores_the_label_warp(golden):
    """register_pair(..., label, fixed_label, labels): 'dice' is the nearest-mode table under the flow that produced
    'warped_label'; without the new arguments the result has no such key."""
    from dfmir_amd import ops
    from dfmir_amd.infer import register_pair

    class _Stub(object):                     # the slice of REGISTRATIONModel that register_pair touches
        def __init__(self, flow):
            self._flow = flow
            self.netG = lambda x: x
            self.netR = lambda a, b, registration=False: (ops.warp(a, self._flow), self._flow)

        def set_input(self, data):
            self.real_A, self.real_B = data["A"].to(DEV), data["B"].to(DEV)

        def forward(self):
            self.fake_B = self.idt_B = self.real_A

    vol, labels = (33, 28), [1, 2, 3]
    mov, fix = blocky_labels(531, 1, vol, 5, 3), blocky_labels(532, 1, vol, 5, 3)
    flow = ((C.rand(533, 1, 2, *vol) * 2 - 1) * 2.0).to(DEV)
    data = {"A": C.rand(534, 1, 1, *vol), "B": C.rand(535, 1, 1, *vol)}
    old = register_pair(_Stub(flow), data, mov.float())
    assert "dice" not in old and "warped_label" in old
    new = register_pair(_Stub(flow), data, mov.float(), fixed_label=fix.long(), labels=labels)
    assert torch.equal(new["warped_label"], old["warped_label"]) and new["dice"].shape == (1, 3)
    assert torch.equal(new["dice"], ops.warp_dice(mov.to(DEV), fix.to(DEV), flow, labels, mode="nearest")[1])
