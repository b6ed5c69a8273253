"""Plain float64 references (torch, CPU) of the operations around the convolutions: masked L1, flow smoothness
(Grad_Loss), windowed NCC, InstanceNorm (+ReLU, +residual), Adam, the displacement-field warp, the VecInt step, the linear
resize, the PatchNCE path (patch gather, L2 normalisation, the MLP head, InfoNCE rows, the loss algebra) and the weight and
bias gradients of a convolution.  TEST
infrastructure, written from the formulas in the docstrings of oracle/dfmir_oracle.py and the kernels' comments;
tests/test_ref64.py checks each one against the fp32 oracle on small inputs, the GPU tests (tests/test_gpu_pointwise_fp64.py,
tests/test_gpu_warp_fp64.py, tests/test_gpu_patchnce_fp64.py, tests/test_gpu_wgrad_fp64.py) compare the HIP kernels with them.

Every function takes tensors of any float dtype and computes in `dtype` (float64 by default); gradients come from
autograd on the returned value.  `dtype=torch.float32` turns a function into a plain fp32 restatement (another valid
summation order), which the GPU tests use as the fp32 yardstick where the fp32 oracle itself is too slow.
"""
import math

import torch
import torch.nn.functional as F


def _t(x, dtype):
    return x if x.dtype == dtype else x.to(dtype)


# ------------------------------------------------------------------------------------------------ masked L1
def threshold_mask(a, b, thr):
    """(a > thr) | (b > thr) with thr rounded to fp32 first: the images are fp32 and so is the kernel's threshold."""
    t = float(torch.tensor(thr, dtype=torch.float32))
    return (a > t) | (b > t)


def masked_l1(a, b, mask=None, thr=None, dtype=torch.float64):
    """sum(|a - b| * m) / sum(m), 0 when sum(m) == 0; m = `mask` (any dtype, non-zero = 1) or the threshold mask
    (a > thr) | (b > thr); without both: mean |a - b|."""
    a, b = _t(a, dtype), _t(b, dtype)
    d = (a - b).abs()
    if mask is None and thr is None:
        return d.mean()
    m = (mask != 0) if mask is not None else threshold_mask(a.detach(), b.detach(), thr)
    m = m.expand_as(d).to(dtype)
    n = m.sum()
    if float(n) == 0.0:
        return (d * 0).sum()
    return (d * m).sum() / n


# ------------------------------------------------------------------------------------------- flow smoothness
def grad_loss(flow, penalty='l2', mask=None, loss_mult=None, skip_empty=False, dtype=torch.float64):
    """mean over the spatial axes of mean(|forward difference|^p), p = 2 ('l2') or 1 ('l1'), of a field [B, C, *spatial]
    (2-D or 3-D); `mask` multiplies the field first, `loss_mult` the result.  An axis of extent 1 has no differences: the
    mean over nothing is NaN, as in torch -- unless skip_empty, where such an axis contributes 0 and the divisor stays the
    number of axes."""
    f = _t(flow, dtype)
    if mask is not None:
        f = f * _t(mask, dtype)
    nd = f.dim() - 2
    tot = 0.0
    for ax in range(2, 2 + nd):
        n = f.shape[ax]
        if n == 1 and skip_empty:
            continue
        d = f.narrow(ax, 1, n - 1) - f.narrow(ax, 0, n - 1)
        tot = tot + ((d * d) if penalty == 'l2' else d.abs()).mean()
    tot = tot / float(nd)
    return tot if loss_mult is None else tot * loss_mult


# ------------------------------------------------------------------------------------------------------ NCC
def box_sum(x, win, axes, method='cumsum'):
    """Zero-padded box sums of odd width `win` along `axes`, one axis after the other.  'cumsum': difference of two
    entries of the running sum (cost independent of win; for float64); 'shift': the plain sum of the win shifted copies."""
    assert win % 2 == 1
    r = win // 2
    for ax in axes:
        L = x.shape[ax]
        pad = [0, 0] * (x.dim() - 1 - ax)
        if method == 'cumsum':
            c = F.pad(x, pad + [r + 1, r]).cumsum(ax)             # c[k] = sum of x[.. k - r - 1]
            x = c.narrow(ax, 2 * r + 1, L) - c.narrow(ax, 0, L)   # x[i - r] + ... + x[i + r]
        else:
            xp = F.pad(x, pad + [r, r])
            acc = xp.narrow(ax, 0, L)
            for d in range(1, win):
                acc = acc + xp.narrow(ax, d, L)
            x = acc
    return x


def ncc_map(I, J, win=9, eps=1e-5, dtype=torch.float64, method=None):
    """cc = cross^2 / (Iv * Jv + eps) over a win^nd box, zero padded: with the box sums Is, Js, I2s, J2s, IJs, n = win^nd,
    uI = Is / n, uJ = Js / n:  cross = IJs - uJ Is - uI Js + uI uJ n,  Iv = I2s - 2 uI Is + uI^2 n,  Jv likewise."""
    I, J = _t(I, dtype), _t(J, dtype)
    method = method or ('cumsum' if dtype == torch.float64 else 'shift')
    axes = list(range(2, I.dim()))
    bs = lambda t: box_sum(t, win, axes, method)
    Is, Js, I2s, J2s, IJs = bs(I), bs(J), bs(I * I), bs(J * J), bs(I * J)
    n = float(win) ** len(axes)
    uI, uJ = Is / n, Js / n
    cross = IJs - uJ * Is - uI * Js + uI * uJ * n
    Iv = I2s - 2 * uI * Is + uI * uI * n
    Jv = J2s - 2 * uJ * Js + uJ * uJ * n
    return cross * cross / (Iv * Jv + eps)


def ncc_loss(I, J, win=9, eps=1e-5, mask=None, reduction='neg_sqrt_mean', dtype=torch.float64, method=None):
    """'neg_sqrt_mean': -sqrt(mean(cc)) (NCC_Loss), 'neg_mean': -mean(cc) (vxm NCC); with a mask the mean is
    sum(cc * mask) / sum(mask), and the loss is 0 when the mask is empty."""
    cc = ncc_map(I, J, win, eps, dtype, method)
    if mask is None:
        m = cc.mean()
    else:
        mk = _t(mask, dtype).expand_as(cc)
        if float(mk.sum()) == 0.0:
            return (cc * 0).sum()
        m = (cc * mk).sum() / mk.sum()
    return -torch.sqrt(m) if reduction == 'neg_sqrt_mean' else -m


def vxm_ncc_loss(y_true, y_pred, win=9, dtype=torch.float64):
    """-mean(cc), eps 1e-5 (cc is symmetric in its arguments)."""
    return ncc_loss(y_pred, y_true, win, 1e-5, None, 'neg_mean', dtype)


# --------------------------------------------------------------------------------------------- InstanceNorm
def instance_norm(x, res=None, relu=False, eps=1e-5, dtype=torch.float64):
    """y = (x - mean) * rstd per (n, c) plane, mean / biased variance over the plane, rstd = 1 / sqrt(var + eps); then
    ReLU, then + res.  Returns (y, mean, rstd), the statistics as [N * C]."""
    x = _t(x, dtype)
    xf = x.reshape(x.shape[0] * x.shape[1], -1)
    mean = xf.mean(1)
    var = ((xf - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = ((xf - mean[:, None]) * rstd[:, None]).reshape(x.shape)
    if relu:
        y = torch.relu(y)
    if res is not None:
        y = y + _t(res, dtype)
    return y, mean, rstd


def blur_down(y):
    """Reflect pad 1, [1 2 1]^2 / 16, stride 2, per channel (the anti-aliased Downsample)."""
    f = torch.tensor([1.0, 2.0, 1.0], dtype=y.dtype)
    k = (f[:, None] * f[None, :] / 16.0)[None, None].repeat(y.shape[1], 1, 1, 1)
    return F.conv2d(F.pad(y, (1, 1, 1, 1), mode="reflect"), k, stride=2, groups=y.shape[1])


# ----------------------------------------------------------------------------------------------------- Adam
class Adam(object):
    """Adam without weight decay on one tensor, in `dtype`:  m = b1 m + (1 - b1) g,  v = b2 v + (1 - b2) g^2,
    p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)."""

    def __init__(self, p, lr, betas, eps=1e-8, dtype=torch.float64):
        self.p = p.detach().to(dtype).clone()
        self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.lr, self.b1, self.b2, self.eps, self.t, self.dtype = lr, betas[0], betas[1], eps, 0, dtype

    def step(self, g):
        g = g.to(self.dtype)
        self.t += 1
        self.m.mul_(self.b1).add_(g, alpha=1 - self.b1)
        self.v.mul_(self.b2).addcmul_(g, g, value=1 - self.b2)
        bc1, bc2 = 1 - self.b1 ** self.t, 1 - self.b2 ** self.t
        den = self.v.sqrt().div_(bc2 ** 0.5).add_(self.eps)
        self.p.addcdiv_(self.m, den, value=-self.lr / bc1)


# ------------------------------------------------------------------------------------- warp, VecInt, resize
def warp(src, flow, mode='bilinear', add_identity=False, dtype=torch.float64):
    """out_c(x) = src_c sampled at x + flow(x), flow in voxels, [B, C, *vol] and [B, nd, *vol], any C.  'bilinear': the 2^nd
    corners of the cell around the sample point (plain floor), weights the products of the per-axis distances, a corner
    outside the volume reads 0 -- explicit floor / gather indexing on tests.test_invcons._corners, of which ic_residual is the
    case C = nd, add_identity on flow itself.  'nearest': the voxel nearest to the sample point, halves to the even one
    (torch.round, the kernels' nearbyintf), 0 outside; no gradient to flow.  add_identity adds src(x)."""
    from tests.test_invcons import _corners, _grid
    src, flow = _t(src, dtype), _t(flow, dtype)
    B, Cn = src.shape[:2]
    vol = tuple(src.shape[2:])
    S = math.prod(vol)
    sf = src.reshape(B, Cn, S)
    pick = lambda flat: torch.gather(sf, 2, flat.reshape(B, 1, S).expand(B, Cn, S)).reshape(src.shape)
    if mode == 'nearest':
        idx = torch.round((_grid(vol, dtype)[None] + flow).detach()).long()
        flat = torch.zeros((B,) + vol, dtype=torch.long)
        valid = torch.ones((B,) + vol, dtype=torch.bool)
        for a in range(len(vol)):
            valid &= (idx[:, a] >= 0) & (idx[:, a] < vol[a])
            flat += idx[:, a].clamp(0, vol[a] - 1) * math.prod(vol[a + 1:])
        out = pick(flat) * valid.to(dtype)[:, None]
    else:
        out = 0.0
        for flat, valid, w, _ in _corners(flow):
            out = out + (w.prod(1) * valid.to(dtype))[:, None] * pick(flat)
    return out + src if add_identity else out


def vecint_step(v, dtype=torch.float64):
    """v + warp(v, v): one scaling-and-squaring step."""
    v = _t(v, dtype)
    return warp(v, v, add_identity=True, dtype=dtype)


def resize_linear(x, out_sp, mult=1.0, dtype=torch.float64):
    """mult * the (bi | tri)linear resize of [B, C, *in_sp] to out_sp with aligned corners: along every axis output o reads
    the source coordinate c = o (in - 1) / (out - 1) (0 when out == 1), i.e. (1 - l) x[i0] + l x[i1] with i0 = floor(c),
    i1 = min(i0 + 1, in - 1), l = c - i0.  Explicit indices and weights, one axis after the other."""
    y = _t(x, dtype)
    for a, n_out in enumerate(out_sp):
        ax = 2 + a
        n_in = y.shape[ax]
        o = torch.arange(n_out, dtype=dtype)
        c = o * (n_in - 1) / (n_out - 1) if n_out > 1 else torch.zeros(n_out, dtype=dtype)
        i0 = torch.floor(c).clamp(0, n_in - 1)
        l = (c - i0).reshape([-1 if d == ax else 1 for d in range(y.dim())])
        i0 = i0.long()
        i1 = (i0 + 1).clamp(max=n_in - 1)
        y = (1.0 - l) * y.index_select(ax, i0) + l * y.index_select(ax, i1)
    return y * mult


# ------------------------------------------------------------------------------------------------- PatchNCE
def l2_normalize_grad(x, dy, eps=1e-7, dtype=torch.float64):
    """dx of y = x / (n + eps), n = sqrt(sum_c x^2), rows [rows, C]:  dx = dy / (n + eps) - x (dy . x) / (n (n + eps)^2),
    the second term 0 where n == 0 (a zero row: y = 0, dx = dy / eps).  Autograd through sqrt gives NaN there, so the
    zero row is DEFINED here, as l2norm_bwd_k defines it."""
    x, dy = _t(x, dtype), _t(dy, dtype)
    n = x.pow(2).sum(1, keepdim=True).sqrt()
    dot = (dy * x).sum(1, keepdim=True)
    safe = torch.where(n > 0, n, torch.ones_like(n))
    k2 = torch.where(n > 0, dot / (n + eps) / (n + eps) / safe, torch.zeros_like(n))     # (this order: no n^3 to overflow in fp32)
    return dy / (n + eps) - x * k2


class _L2Normalize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, eps):
        ctx.save_for_backward(x)
        ctx.eps = eps
        return x / (x.pow(2).sum(1, keepdim=True).sqrt() + eps)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return l2_normalize_grad(x, dy, ctx.eps, x.dtype), None


def l2_normalize(x, eps=1e-7, dtype=torch.float64):
    """x / (sqrt(sum_c x^2) + eps) on [rows, C]; the gradient is l2_normalize_grad (written out, not autograd's)."""
    return _L2Normalize.apply(_t(x, dtype), float(eps))


def patchnce_rows(q, k, groups, T, dtype=torch.float64):
    """Per-row InfoNCE loss of q, k [rows, C]; consecutive groups of R = rows / groups rows share negatives.  Logits
    q . k^T within a group, the diagonal replaced by -10, the positive logit q_i . k_i prepended, all divided by T;
    loss_i = logsumexp(row i) - positive_i, with an explicit max shift.  k is detached: the gradient flows to q only."""
    q, k = _t(q, dtype), _t(k, dtype).detach()
    rows, Cn = q.shape
    R = rows // groups
    assert R * groups == rows
    qg, kg = q.reshape(groups, R, Cn), k.reshape(groups, R, Cn)
    pos = (qg * kg).sum(2, keepdim=True)
    neg = torch.matmul(qg, kg.transpose(1, 2)).masked_fill(torch.eye(R, dtype=torch.bool)[None], -10.0)
    z = torch.cat([pos, neg], 2) / T
    m = z.detach().max(2, keepdim=True).values
    lse = m[..., 0] + torch.log(torch.exp(z - m).sum(2))
    return (lse - z[..., 0]).reshape(rows)


def _ids2(ids, groups):
    return ids.reshape(int(groups), -1).long()


def patch_gather(feat, ids, groups=1, dtype=torch.float64):
    """feat [B, C, *sp], ids [G, P] (or [P], G = 1) -> rows [B * P, C]: row b * P + p is feat[b, :, ids[b // (B / G), p]]
    over the flattened spatial positions."""
    f = _t(feat, dtype)
    B, Cn = f.shape[:2]
    ids = _ids2(ids, groups)
    bpg = B // ids.shape[0]
    ff = f.reshape(B, Cn, -1)
    return torch.cat([ff[b][:, ids[b // bpg]].t() for b in range(B)], 0)


def patch_gather_adjoint(drows, ids, groups, shape, dtype=torch.float64):
    """The adjoint of patch_gather: drows [B * P, C] scattered into zeros of `shape` by index_add_; repeated ids accumulate."""
    d = _t(drows, dtype)
    B, Cn = shape[:2]
    ids = _ids2(ids, groups)
    P, bpg = ids.shape[1], B // ids.shape[0]
    out = torch.zeros(B, Cn, math.prod(shape[2:]), dtype=dtype)
    for b in range(B):
        out[b].index_add_(1, ids[b // bpg], d[b * P:(b + 1) * P].t())
    return out.reshape(shape)


def nce_head(feat, ids, w1, b1, w2, b2, eps=1e-7, groups=1, dtype=torch.float64):
    """gather -> relu(x W1^T + b1) -> W2^T + b2 -> l2_normalize: rows [B * P, nc]; w1 [nc, C], w2 [nc, nc] (Linear layout)."""
    x = patch_gather(feat, ids, groups, dtype)
    h = torch.relu(x @ _t(w1, dtype).t() + _t(b1, dtype))
    return l2_normalize(h @ _t(w2, dtype).t() + _t(b2, dtype), eps, dtype)


def segment_means(rows, n_terms, scale, dtype=torch.float64):
    """out[t] = scale * sum_l mean(rows[l, t * seg : (t + 1) * seg]) for rows [L, T * seg]."""
    r = _t(rows, dtype)
    L = r.shape[0]
    return scale * r.reshape(L, int(n_terms), -1).mean(2).sum(0)


def scalar_combine(M, xs, dtype=torch.float64):
    """out[j] = sum_i M[j][i] x_i for one-element tensors x_i."""
    Mt = torch.as_tensor(M, dtype=torch.float32).to(dtype)         # the coefficients reach the kernel as fp32
    return Mt @ torch.stack([_t(x, dtype).reshape(()) for x in xs])


# ----------------------------------------------------------------------- convolution weight / bias gradients
def nearest_up2(a):
    """Every voxel of [N, C, *sp] repeated twice along every spatial axis (nearest-neighbour up-sampling by 2)."""
    for ax in range(2, a.dim()):
        a = a.repeat_interleave(2, dim=ax)
    return a


def upcat(a, b):
    """cat(nearest_up2(a), b) over the channels, built explicitly (the operand ops.upcat_conv3d never builds)."""
    return torch.cat([nearest_up2(a), b], 1)


def _per_axis(v, nd):
    v = tuple(int(e) for e in v) if isinstance(v, (tuple, list)) else (int(v),) * nd
    assert len(v) == nd, (v, nd)
    return v


def pad_by_index(x, pad, pad_mode):
    """x [N, C, *sp] padded by pad[a] on both sides of spatial axis a: pad_mode 0 = zeros, 1 = reflect without the edge
    (index -i reads i, index n - 1 + i reads n - 1 - i).  Explicit index arithmetic, not F.pad."""
    for a, p in enumerate(pad):
        if p == 0:
            continue
        ax, n = 2 + a, x.shape[2 + a]
        if pad_mode == 0:
            shp = list(x.shape)
            shp[ax] = n + 2 * p
            xp = torch.zeros(shp, dtype=x.dtype)
            xp.narrow(ax, p, n).copy_(x)
            x = xp
        else:
            assert p <= n - 1, "reflect padding needs pad < extent"
            i = torch.arange(-p, n + p).abs()
            i = torch.where(i > n - 1, 2 * (n - 1) - i, i)
            x = x.index_select(ax, i)
    return x


def _contract(A, Bm, order):
    """A [Cin, P], Bm [Cout, P] -> [Cout, Cin] = sum over P.  'matmul': one matrix product; 'chunk64': a running sum over
    chunks of 64 positions (every chunk a product of its own, added to the accumulator in position order)."""
    if order == "matmul":
        return Bm @ A.t()
    assert order == "chunk64", order
    P = A.shape[1]
    acc = torch.zeros(Bm.shape[0], A.shape[0], dtype=A.dtype)
    nfull = P // 64
    if nfull:
        part = torch.bmm(Bm[:, :nfull * 64].reshape(Bm.shape[0], nfull, 64).transpose(0, 1),
                         A[:, :nfull * 64].reshape(A.shape[0], nfull, 64).permute(1, 2, 0))
        for i in range(nfull):
            acc = acc + part[i]
    if P > nfull * 64:
        acc = acc + Bm[:, nfull * 64:] @ A[:, nfull * 64:].t()
    return acc


def conv_weight_grad(x, dy, K, stride, pad, pad_mode, dtype=torch.float64, order="matmul"):
    """dW [Cout, Cin, *K] of y = conv(x, W), stride `stride`, padding `pad` (zeros: pad_mode 0, reflect: 1), from the
    definition:  dW[co, ci, t] = sum over (n, o) of xp[n, ci, stride * o + t] * dy[n, co, o]  with xp the padded input and o
    the output positions -- for every tap t the strided slice of xp contracted with dy over batch and positions.  x, dy
    [N, C, *sp] with 2 or 3 spatial axes (a 2-D layer may come as [N, C, 1, H, W] with K = (1, k, k), pad = (0, p, p)); K
    and pad an int or one per axis.  x = (a, b): the operand is cat(nearest_up2(a), b), built here.  `order`: how the fp32
    restatement (dtype=torch.float32) sums -- 'matmul' or 'chunk64', see _contract; two valid orders, so that neither
    flatters the yardstick."""
    if isinstance(x, (tuple, list)):
        x = upcat(_t(x[0], dtype), _t(x[1], dtype))
    x, dy = _t(x, dtype), _t(dy, dtype)
    nd = x.dim() - 2
    K, pad = _per_axis(K, nd), _per_axis(pad, nd)
    out_sp = tuple(dy.shape[2:])
    for a in range(nd):
        assert out_sp[a] == (x.shape[2 + a] + 2 * pad[a] - K[a]) // stride + 1, (a, out_sp, tuple(x.shape), K, pad, stride)
    xp = pad_by_index(x, pad, pad_mode)
    Cin, Cout = x.shape[1], dy.shape[1]
    Bm = dy.transpose(0, 1).reshape(Cout, -1)
    dw = torch.zeros((Cout, Cin) + K, dtype=dtype)
    taps = [()]
    for k in K:
        taps = [t + (i,) for t in taps for i in range(k)]
    for t in taps:
        sl = xp
        for a in range(nd):
            sl = sl.narrow(2 + a, t[a], stride * (out_sp[a] - 1) + 1)
            if stride > 1:
                sl = sl.index_select(2 + a, torch.arange(0, sl.shape[2 + a], stride))
        dw[(slice(None), slice(None)) + t] = _contract(sl.transpose(0, 1).reshape(Cin, -1), Bm, order)
    return dw


def conv_bias_grad(dy, dtype=torch.float64, order="matmul"):
    """db [Cout] = sum of dy [N, Cout, *sp] over batch and positions; order as in conv_weight_grad ('matmul': torch's sum)."""
    Bm = _t(dy, dtype).transpose(0, 1).reshape(dy.shape[1], -1)
    if order == "matmul":
        return Bm.sum(1)
    return _contract(torch.ones(1, Bm.shape[1], dtype=dtype), Bm, order)[:, 0]
