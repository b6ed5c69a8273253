"""profiles/hausdorff_timing.txt: ops.label_hausdorff on the device (one event pair per call, median of 5 after 2 warm-up
calls) at [1,1,256,256] with K = 4 and [1,1,160,192,224] with K = 35, and the reference's path (scipy's
distance_transform_edt, util/loss_metrics.py:105-132) on the host of the same machine where scipy is installed; the two are
checked against each other on the labels the host ran.

    python scripts/bench_hausdorff.py [--out FILE] [--tiny]"""
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tests.test_hausdorff import blocky_labels            # noqa: E402

OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
TINY = "--tiny" in sys.argv
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def maps(vol, nvals, block, shift):
    a = blocky_labels(900, 1, vol, nvals, block)
    b = torch.roll(a, shifts=shift, dims=tuple(range(2, 2 + len(vol))))
    return a, b


def time_gpu(a, b, labels, **kw):
    from dfmir_amd import ops
    for _ in range(2):
        out = ops.label_hausdorff(a, b, labels, **kw)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
    ev[0].record()
    for i in range(5):
        out = ops.label_hausdorff(a, b, labels, **kw)
        ev[i + 1].record()
    torch.cuda.synchronize()
    ts = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(5))
    return ts[2], ts[0], ts[4], out


def scipy_ref(a, b, labels):
    """The reference's hd_distance per label on the host: (seconds, hd per label)."""
    try:
        from scipy.ndimage import distance_transform_edt as edt
    except ImportError:
        return None, None
    a, b = a[0, 0].numpy(), b[0, 0].numpy()
    t0 = time.perf_counter()
    hd = []
    for l in labels:
        x, y = a == l, b == l
        if not x.any() or not y.any():
            hd.append(np.inf)
            continue
        hd.append(max(edt(~y)[x].max(), edt(~x)[y].max()))
    return time.perf_counter() - t0, hd


def main():
    gpu = torch.cuda.is_available()
    say("label_hausdorff timing; device: %s" % (torch.cuda.get_device_name(0) if gpu else "none (rehearsal)"))
    cases = [("[1,1,256,256] K=4", (256, 256), 4, 16, (3, -2), 4),
             ("[1,1,160,192,224] K=35", (160, 192, 224), 35, 8, (2, -3, 1), 3)]
    if TINY:
        cases = [("tiny 2-D", (20, 24), 4, 4, (1, -1), 4), ("tiny 3-D", (6, 10, 12), 5, 3, (1, 0, -1), 3)]
    for name, vol, K, block, shift, nref in cases:
        a, b = maps(vol, K + 2, block, shift)
        labels = list(range(1, K + 1))
        say("%s  (labels 1..%d of blocky maps, block %d, b = a rolled by %s)" % (name, K, block, (shift,)))
        got = None
        if gpu:
            ad, bd = a.cuda(), b.cuda()
            for what, kw in (("percentile 100", {}), ("percentile 100, mean=False", {"mean": False}),
                             ("percentile 95, surface", {"percentile": 95.0, "surface": True})):
                med, lo, hi, out = time_gpu(ad, bd, labels, **kw)
                say("  device  %-28s median %9.3f ms  (min %9.3f  max %9.3f, 5 calls)" % (what, med, lo, hi))
                if not kw:
                    got = out[0][0].cpu().numpy()
        sec, hd = scipy_ref(a, b, labels[:nref])
        if sec is None:
            say("  host    scipy is not installed on this machine: the reference's path was not measured")
        else:
            say("  host    reference path (scipy distance_transform_edt, both directions), %d labels: %9.1f ms = %9.1f ms per label"
                " -> about %9.1f ms for K=%d" % (nref, 1e3 * sec, 1e3 * sec / nref, 1e3 * sec / nref * K, K))
            if got is not None:
                ok = all(np.float32(h) == g or abs(np.float32(h) - g) <= np.spacing(np.float32(h)) for h, g in zip(hd, got))
                say("  device hd equals the host's on those labels (one fp32 ulp): %s" % ok)
    if OUT:
        with open(OUT, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
