"""Generator of tests/golden/ncc_gauss.npz -- the reference's NCC_Loss(kernel_type='gaussian') (util/losses.py:145-261) on
seeded 2-D inputs (its window is 2-D only: conv3d fails on it): the loss and d / d prediction.  Runs only where the
reference checkout (make_golden.REF) exists; imports the reference itself with the shims of make_golden.py and records
INPUTS-BY-SEED + the reference's own outputs, per case <tag>:

  <tag>_pred, <tag>_target, [<tag>_mask]   inputs: target J = rand, prediction I = 0.6 rand + 0.4 J
  <tag>_sigma                              kernel_var[0]
  <tag>_loss, <tag>_dpred                  the loss and its gradient (0 and zeros for an empty mask: the reference returns
                                           a constant there)

and, for the tests' tolerances and the host tap builder:

  ref_fp32_err_loss_case, _grad_case       how far these fp32 CPU results lie from the float64 restatement of
                                           tests/test_ncc_gauss.py, one entry per case in the order of `cases`: relative
                                           error of the loss, |g - g64| / |g64| (2-norm) of the gradient
  ref_fp32_err_loss                        the maximum of the former over all cases
  ref_fp32_err_grad                        the maximum of the latter over the WELL-CONDITIONED cases, i.e. all but
                                           `half_const`: where I_var ~ 0 the denominator I_var J_var + eps is eps plus
                                           fp32 cancellation noise and the reference's own gradient is off by 1.5e-3,
                                           a thousand times the other cases' error; that case is bounded by its own entry
  ref_sum_filt, ref_sum_filt_sigma         the reference's own fp32 torch.sum(filt) for sigma = 1..5

    python tests/golden/make_golden_ncc_gauss.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from tests.golden import common as C                      # noqa: E402
from tests.golden import make_golden as MG                # noqa: E402
from tests.test_ncc_gauss import ncc_gauss_ref64, rel_errors   # noqa: E402


def cases():
    """(tag, shape, sigma, mask or None, left half of the prediction constant)"""
    m = (C.rand(73, 1, 1, 24, 20) > 0.4).float()                # [1,1,H,W] against B = 2
    return [
        ("b2", (2, 1, 24, 20), 3, None, False),                 # the window must not bleed across batch items
        ("small", (1, 1, 7, 5), 3, None, False),                # smaller than the 9-wide window in both axes
        ("odd", (1, 1, 33, 70), 3, None, False),                # odd sizes, W % 4 != 0, one past the 32 x 64 tile in each axis
        ("sigma1", (2, 1, 24, 20), 1, None, False),             # K = 3
        ("sigma2", (2, 1, 24, 20), 2, None, False),             # K = 7
        ("sigma5", (2, 1, 24, 20), 5, None, False),             # K = 15
        ("mask", (2, 1, 24, 20), 3, m, False),
        ("mask_zero", (2, 1, 24, 20), 3, torch.zeros(1, 1, 24, 20), False),
        ("half_const", (1, 1, 24, 20), 3, None, True),          # I_var ~ 0 against eps
    ]


def main():
    MG.install_shims()
    from util.losses import NCC_Loss as RefNCC
    npy = MG.npy
    out = {}
    errs_l, errs_g = [], []
    for i, (tag, shape, sigma, mask, half) in enumerate(cases()):
        J = C.rand(500 + 10 * i, *shape)
        I = 0.6 * C.rand(505 + 10 * i, *shape) + 0.4 * J
        if half:
            I[..., :shape[-1] // 2] = 0.37
        I = I.requires_grad_()
        crit = RefNCC('cpu', kernel_var=[sigma, sigma], kernel_type='gaussian')
        loss = crit(I, J) if mask is None else crit(I, J, mask=mask)
        if loss.requires_grad:
            loss.backward()
            grad = I.grad
            l64, g64 = ncc_gauss_ref64(I, J, sigma, mask)
            el, eg = rel_errors(loss.detach(), grad, l64, g64)
        else:                                                   # the empty mask: `torch.tensor(0)`
            assert float(loss) == 0.0
            grad, el, eg = torch.zeros_like(I), 0.0, 0.0
        errs_l.append(el)
        errs_g.append(eg)
        out.update({tag + "_pred": npy(I), tag + "_target": npy(J), tag + "_sigma": np.int64(sigma),
                    tag + "_loss": np.float32(float(loss)), tag + "_dpred": npy(grad)})
        if mask is not None:
            out[tag + "_mask"] = npy(mask)
        print("%-11s loss %-12.8f fp32 vs fp64: loss %.3e grad %.3e" % (tag, float(loss), el, eg))
    sums = [float(torch.sum(RefNCC('cpu', kernel_type='gaussian')._get_kernel('gaussian', [s, s]))) for s in range(1, 6)]
    out["ref_sum_filt"] = np.array(sums, np.float32)
    out["ref_sum_filt_sigma"] = np.arange(1, 6)
    tags = [c[0] for c in cases()]
    worst_l = max(errs_l)
    worst_g = max(e for t, e in zip(tags, errs_g) if t != "half_const")
    out["ref_fp32_err_loss_case"], out["ref_fp32_err_grad_case"] = np.array(errs_l), np.array(errs_g)
    out["ref_fp32_err_loss"], out["ref_fp32_err_grad"] = np.float64(worst_l), np.float64(worst_g)
    out["cases"] = np.array(tags)
    print("sum(filt)", sums, " worst fp32 error: loss %.3e grad %.3e (well-conditioned cases)" % (worst_l, worst_g))
    MG.HERE = HERE
    MG.save("ncc_gauss.npz", **out)


if __name__ == "__main__":
    main()
