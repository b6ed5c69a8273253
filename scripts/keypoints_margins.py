"""profiles/keypoints_margins.txt: per case of tests/test_keypoints.py the error e32 of the definition evaluated by torch in
fp32 on the CPU against the float64 restatement, the bound the tests derive from it (4 e32 + 4 * 2^-23 max|reference|) and -- with
a GPU -- the kernels' own errors beside them; for the smooth-deformation case the share of keypoints the comparison leaves out,
the same share for the restatement's own fp32 evaluation, and the restatement's mean TRE against the true field before and after.

    python scripts/keypoints_margins.py [--out profiles/keypoints_margins.txt]

The CPU columns need no GPU; without one the kernel columns read "-" and the deformation block is left out (its features are
the MIND kernels')."""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from dfmir_amd import infer, ops  # noqa: E402
from tests import test_keypoints as T  # noqa: E402


def row(name, e32, bound, ke):
    return "%-44s %10.3e %10.3e %10s %8s" % (name, e32, bound, "-" if ke is None else "%.3e" % ke,
                                             "-" if ke is None else "%.3f" % (ke / bound))


def deformation(lines):
    P = T.DEFORM
    vol, r, step, patch = P['vol'], P['search_radius'], P['search_step'], P['patch']
    fixed, u = T.deform_pair(vol, P['seed'], P['amp'])
    fixed, ud = fixed.to(T.DEV), u.to(T.DEV)
    moving = ops.warp(fixed, ud)
    Mm, Mf = ops.mind_descriptor(moving, 2, 2), ops.mind_descriptor(fixed, 2, 2)
    out = infer.keypoint_init(moving, fixed, features=(Mm, Mf), num_keypoints=P['K'], sigma=P['sigma'],
                              nms_radius=P['nms_radius'], search_radius=r, search_step=step, patch=patch,
                              smoothing=P['smoothing'])
    q, w = out['fixed_pts'].cpu(), out['weight'].cpu()
    valid = w > 0
    fm, ff = Mm.cpu(), Mf.cpu()
    rc = T.ref_cost(ff, fm, q, r, step, patch, T.F64)
    r32 = T.ref_cost(ff, fm, q, r, step, patch, T.F32)
    e32 = float((r32.to(T.F64) - rc)[torch.isfinite(rc)].abs().max())
    bound = T.cost_bound(rc, e32)
    steps = T.ref_coupling(rc, q, w, vol, r, step, infer.CONVEX_COEFFS, P['smoothing'])
    ri, rd, best, second = steps[-1]
    close = (second - best) < 2 * bound
    s32 = T.ref_coupling(r32.to(T.F64), q, w, vol, r, step, infer.CONVEX_COEFFS, P['smoothing'])[-1]
    differ32 = (s32[0] != ri) & valid
    # the true correspondence of q: the y with y + u(y) = q (moving = warp(fixed, u)), by fixed-point iteration on the field
    qv = q[valid][None].to(T.DEV)
    y = qv.clone()
    top = torch.tensor([n - 1.0 for n in vol], device=T.DEV)
    for _ in range(50):
        yc = torch.minimum(y.clamp(min=0), top)                      # the field is read inside the volume
        y = qv - (ops.warp_points(yc, ud) - yc)
    y = y[0].cpu().to(T.F64)
    before = (q[valid].to(T.F64) - y).norm(dim=1).mean()
    after = (q[valid].to(T.F64) + rd[valid] - y).norm(dim=1).mean()
    gk = (out['idx'].cpu().long() != ri) & valid
    lines += ["# smooth deformation %s, amplitude %g, seed %d, MIND features, K = %d (valid %d), search %d x %d, patch %d:"
              % ("x".join(map(str, vol)), P['amp'], P['seed'], P['K'], int(valid.sum()), r, step, patch),
              "#   cost bound of the case %.3e (e32 %.3e); keypoints whose two best penalised costs lie within twice the bound: "
              "%d of %d = %.2f %% (the test allows 5 %%)" % (bound, e32, int((close & valid).sum()), int(valid.sum()),
                                                           100.0 * float((close & valid).sum()) / float(valid.sum())),
              "#   the restatement's own fp32 evaluation picks another index at %d keypoints; the kernels at %d"
              % (int(differ32.sum()), int(gk.sum())),
              "#   restatement's mean TRE against the true field: %.3f voxels before, %.3f after (not asserted)"
              % (float(before), float(after))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "keypoints_margins.txt"))
    args = ap.parse_args()
    gpu = torch.cuda.is_available()
    lines = ["# keypoint kernels (dfmir_amd/csrc/keypoints.hip) against the float64 restatements of tests/test_keypoints.py",
             "# e32 = the same definition in fp32 on the CPU; bound = 4 e32 + 4 * 2^-23 max|reference|; max-abs errors;",
             "# kernel = ops.foerstner_response / ops.keypoint_cost on %s" % (torch.cuda.get_device_name(0) if gpu else "- (no GPU)"),
             "# (ops.local_maxima and ops.keypoint_argmin are compared bit for bit: no margin)",
             "%-44s %10s %10s %10s %8s" % ("case", "e32", "bound", "kernel", "k/bound")]
    worst = 0.0
    for case in T.RESP_CASES:
        I, h, ref, e32 = T.resp_case(*case)
        bound = T.FACTOR * e32 + T.FLOOR * float(ref.abs().max())
        ke = None
        if gpu:
            got = ops.foerstner_response(I.to(T.DEV), case[1], h if case[2] else None).cpu().to(T.F64)
            ke = float((got - ref).abs().max())
            worst = max(worst, ke / bound if bound > 0 else 0.0)
        lines.append(row("response " + T._rid(case), e32, bound, ke))
    for case in T.COST_CASES:
        fix, mov, pts, ref, e32 = T.cost_case(*case)
        bound = T.cost_bound(ref, e32)
        ke = None
        if gpu:
            got = ops.keypoint_cost(fix.to(T.DEV), mov.to(T.DEV), pts.to(T.DEV), *case[2:]).cpu().to(T.F64)
            ke = float((got - ref)[torch.isfinite(ref)].abs().max())
            worst = max(worst, ke / bound)
        lines.append(row("cost " + T._cid(case), e32, bound, ke))
    if gpu:
        lines.append("# worst kernel / bound: %.3f" % worst)
        deformation(lines)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
