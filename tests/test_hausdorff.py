"""Hausdorff distance of label maps on the HIP distance transform (dfmir_amd/csrc/edt.hip: ops.label_edt_sq,
ops.label_hausdorff, losses.HausdorffDistance / LabelHausdorff, infer.score_labels): the C ABI and the argument checks
(CPU), the reference's own values (tests/golden/hausdorff.npz, util/loss_metrics.py:105-132 on scipy), and a pure-numpy
restatement -- the separable integer transform d[i] = min_j(prev[j] + (i - j)^2) per axis, the border predicate, the
nearest-rank percentile and a float64 mean -- that the kernels must equal EXACTLY: the squared distances are integers.

The only inexact comparisons: sqrt of an exactly represented integer against the reference's float64 sqrt rounded to fp32
(one fp32 ulp), and the mean distance, a float64 sum rounded to fp32 (rtol 1e-6 >= 8 fp32 ulps; the float64 sums themselves
differ by ~1e-16 per term)."""
import inspect
import os

import numpy as np
import pytest
import torch

from tests.golden import common as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
INF = 1 << 29
NAMES = ("dfmir_label_hausdorff_ws_bytes", "dfmir_label_edt_sq", "dfmir_label_hausdorff")
FIXTURE_CASES = ("overlap", "disjoint", "identical", "corners", "empty_pred", "ring_disc")


# ------------------------------------------------------------------------------------------ numpy restatement
def edt_sq_np(mask):
    """Exact squared distance to the nearest True voxel of `mask` (any rank), int32; INF where mask is empty."""
    d = np.where(mask, 0, INF).astype(np.int64)
    for ax in range(d.ndim):
        n = d.shape[ax]
        prev = np.moveaxis(d, ax, 0)
        out = np.empty_like(prev)
        j = np.arange(n).reshape((n,) + (1,) * (prev.ndim - 1))
        for i in range(n):
            out[i] = np.min(prev + (i - j) ** 2, axis=0)
        d = np.moveaxis(np.minimum(out, INF), 0, ax)
    return d.astype(np.int32)


def border_np(mask):
    """Set voxels with a face neighbour outside the set or outside the volume; a 3-D array of one plane is a 2-D image."""
    m = np.asarray(mask, dtype=bool)
    one_plane = m.ndim == 3 and m.shape[0] == 1
    if one_plane:
        m = m[0]
    p = np.pad(m, 1, constant_values=False)
    inner = m.copy()
    for ax in range(m.ndim):
        for off in (0, 2):
            sl = tuple(slice(off, off + m.shape[a]) if a == ax else slice(1, 1 + m.shape[a]) for a in range(m.ndim))
            inner &= p[sl]
    b = m & ~inner
    return b[None] if one_plane else b


def nearest_rank(d2, qm):
    """The smallest value whose cumulative count reaches r = max(1, ceil(qm n / 100000)); qm = percentile * 1000."""
    s = np.sort(np.asarray(d2).reshape(-1))
    r = max(1, -((-int(qm) * int(s.size)) // 100000))
    return int(s[r - 1])


def hausdorff_np(a, b, qm=100000, surface=False):
    """One sample, one label: (hd, directed[2], mean[2], d2[2]) of the boolean arrays a, b (direction 0: a -> b)."""
    a, b = np.asarray(a, dtype=bool), np.asarray(b, dtype=bool)
    if surface:
        a, b = border_np(a), border_np(b)
    if not a.any() or not b.any():
        return np.inf, [np.inf, np.inf], [np.inf, np.inf], [INF, INF]
    directed, mean, d2 = [], [], []
    for src, tgt in ((a, b), (b, a)):
        v = edt_sq_np(tgt)[src]
        q = nearest_rank(v, qm)
        d2.append(q)
        directed.append(float(np.sqrt(np.float64(q))))
        mean.append(float(np.sqrt(v.astype(np.float64)).mean()))
    return max(directed), directed, mean, d2


def hausdorff_table_np(a, b, labels, qm=100000, surface=False):
    """(hd[B,K], directed[2,B,K], mean[2,B,K], d2[2,B,K]) of uint8 label maps [B,1,*vol]."""
    B, K = a.shape[0], len(labels)
    hd, di, me, d2 = np.zeros((B, K)), np.zeros((2, B, K)), np.zeros((2, B, K)), np.zeros((2, B, K), np.int64)
    for bi in range(B):
        for k, l in enumerate(labels):
            h, d, m, q = hausdorff_np(a[bi, 0] == l, b[bi, 0] == l, qm, surface)
            hd[bi, k], di[:, bi, k], me[:, bi, k], d2[:, bi, k] = h, d, m, q
    return hd, di, me, d2


def blocky_labels(seed, B, vol, nvals, block):
    coarse = [-(-s // block) for s in vol]
    x = (C.rand(seed, B, 1, *coarse) * nvals).long().clamp_(max=nvals - 1)
    for ax in range(len(vol)):
        x = x.repeat_interleave(block, dim=2 + ax)
    return x[(slice(None), slice(None)) + tuple(slice(0, s) for s in vol)].to(torch.uint8).contiguous()


def ulp32(x):
    return float(np.spacing(np.float32(x)))


# ------------------------------------------------------------------------------------------ CPU tier
def test_restatement_reproduces_every_fixture_value(golden):
    g = golden("hausdorff.npz")
    seen_inf = 0
    for nd in (2, 3):
        for case in FIXTURE_CASES:
            tag = "%dd_%s" % (nd, case)
            ref = float(g[tag + "_hd"])
            hd, _, _, d2 = hausdorff_np(g[tag + "_pred"][0, 0] > 0, g[tag + "_target"][0, 0] > 0)
            if np.isinf(ref):
                assert np.isinf(hd) and d2 == [INF, INF], tag
                seen_inf += 1
            else:
                assert int(np.rint(np.float64(ref) ** 2)) == max(d2), (tag, ref, d2)
        vol = g["%dd_corners_pred" % nd].shape[2:]
        assert int(np.rint(float(g["%dd_corners_hd" % nd]) ** 2)) == sum((n - 1) ** 2 for n in vol)
        assert float(g["%dd_identical_hd" % nd]) == 0.0
    assert seen_inf == 2
    # the documented divergence: the reference measures across the batch axis, every sample on its own gives inf
    assert np.isfinite(float(g["mix_ref_hd"]))
    for bi in range(2):
        assert np.isinf(hausdorff_np(g["mix_pred"][bi, 0] > 0, g["mix_target"][bi, 0] > 0)[0])


def test_restatement_equals_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for seed, vol in ((1, (7, 33, 70)), (2, (1, 40, 65)), (3, (5, 9, 13)), (4, (37, 70))):
        m = (C.rand(seed, *vol) < 0.02).numpy()
        m[..., 3, :] = False
        ref = ndi.distance_transform_edt(~m)
        assert np.array_equal(np.rint(ref ** 2).astype(np.int64), edt_sq_np(m).astype(np.int64)), vol
        blob = blocky_labels(10 + seed, 1, vol, 2, 3)[0, 0].numpy() > 0
        sq = blob[0] if blob.ndim == 3 and blob.shape[0] == 1 else blob
        er = ndi.binary_erosion(sq, ndi.generate_binary_structure(sq.ndim, 1), border_value=0)
        assert np.array_equal(border_np(blob).reshape(sq.shape), sq & ~er), vol
    assert edt_sq_np(np.zeros((4, 5), bool)).min() == INF
    assert nearest_rank([5, 1, 3, 2, 4], 50000) == 3 and nearest_rank([5, 1, 3, 2, 4], 100000) == 5
    assert nearest_rank([5, 1, 3, 2, 4], 1) == 1 and nearest_rank([5, 1, 3, 2, 4], 60001) == 4


def test_hausdorff_symbols_in_header_exports_and_ctypes_table():
    import ctypes
    import dfmir_amd
    from dfmir_amd import _lib, ops
    from tests.test_abi import header_symbols
    h = ctypes.CDLL(dfmir_amd.LIB_PATH)
    for s in NAMES:
        assert s in header_symbols() and s in _lib.exported_symbols() and hasattr(h, s), s
    assert dfmir_amd.lib().dfmir_abi_version() == 14
    text = open(os.path.join(REPO, "include", "dfmir_hip.h")).read()
    assert "#define DFMIR_EDT_SQ_INF (1 << 29)" in text and ops.EDT_SQ_INF == INF
    assert "#define DFMIR_HD_SURFACE %d" % ops.HD_SURFACE in text


def test_hausdorff_workspace_query_and_bad_arguments_touch_no_device():
    import dfmir_amd
    lib = dfmir_amd.lib()
    q = lib.dfmir_label_hausdorff_ws_bytes
    for bad in ((4, 1, 1, 4, 4, 4), (1, 1, 1, 4, 4, 4), (3, 0, 1, 4, 4, 4), (3, 1, 0, 4, 4, 4), (3, 1, 65, 4, 4, 4),
                (3, 1, 1, 0, 4, 4), (3, 1, 1, 4, -1, 4), (2, 1, 1, 2, 4, 4), (3, 1, 1, 257, 4, 4), (3, 1, 1, 4, 257, 4),
                (2, 1, 1, 1, 4, 257), (3, 70000, 1, 4, 4, 4)):
        assert q(*bad) == -1, bad
    S, bins = 160 * 192 * 224, 159 ** 2 + 191 ** 2 + 223 ** 2 + 1
    full = q(3, 1, 35, 160, 192, 224)
    assert full == 4 * 2 * 4 * (S + 2 + bins) == 223768768
    assert q(3, 1, 64, 160, 192, 224) == full and q(3, 1, 4, 160, 192, 224) == full        # one chunk, whatever K
    assert q(3, 1, 1, 160, 192, 224) == full // 4
    assert q(2, 1, 4, 1, 256, 256) > 0 and q(3, 2, 5, 256, 256, 256) > 0
    for rc in (lib.dfmir_label_edt_sq(3, None, 1, 0, 1, 4, 4, 4, None, None),
               lib.dfmir_label_hausdorff(3, None, None, None, 1, 1, 4, 4, 4, 100000, 0, None, None, None, None, None, None)):
        assert rc != 0
        assert b"invalid argument" in lib.dfmir_last_error()


def test_label_hausdorff_rejects_bad_arguments_before_any_launch():
    from dfmir_amd import ops
    from dfmir_amd._lib import DfmirHipError
    from dfmir_amd.losses import HausdorffDistance, LabelHausdorff
    m = torch.zeros(1, 1, 8, 8, dtype=torch.uint8)
    with pytest.raises(DfmirHipError, match="no CPU fallback"):
        ops.label_hausdorff(m, m, [1, 2])
    with pytest.raises(DfmirHipError, match="no CPU fallback"):
        ops.label_edt_sq(m, 1)
    with pytest.raises(DfmirHipError, match="do not match"):
        ops.label_hausdorff(m, torch.zeros(1, 1, 8, 9, dtype=torch.uint8), [1])
    with pytest.raises(DfmirHipError, match=r"\[B,1,\*vol\]"):
        ops.label_hausdorff(torch.zeros(1, 2, 8, 8, dtype=torch.uint8), m, [1])
    with pytest.raises(DfmirHipError, match=r"\[B,1,\*vol\]"):
        ops.label_edt_sq(torch.zeros(8, 8, dtype=torch.uint8), 1)
    with pytest.raises(DfmirHipError, match="uint8"):
        ops.label_hausdorff(m.long(), m, [1])
    with pytest.raises(DfmirHipError, match="uint8"):
        ops.label_edt_sq(m.float(), 1)
    with pytest.raises(DfmirHipError, match="1 to 64"):
        ops.label_hausdorff(m, m, list(range(65)))
    with pytest.raises(DfmirHipError, match="1 to 64"):
        ops.label_hausdorff(m, m, [])
    with pytest.raises(DfmirHipError, match="duplicate"):
        ops.label_hausdorff(m, m, [1, 2, 1])
    for bad in ([256], [-1], [1.5]):
        with pytest.raises(DfmirHipError, match=r"\[0, 255\]"):
            ops.label_hausdorff(m, m, bad)
    for bad in (256, -1, 1.5, True):
        with pytest.raises(DfmirHipError, match=r"\[0, 255\]"):
            ops.label_edt_sq(m, bad)
    for bad in (0, 0.0, -5, 100.001, 101, 95.0005, float("nan"), float("inf"), "x"):
        with pytest.raises(DfmirHipError, match="percentile"):
            ops.label_hausdorff(m, m, [1], percentile=bad)
        with pytest.raises(DfmirHipError, match="percentile"):
            LabelHausdorff([1], percentile=bad)
    for ok, qm in ((100, 100000), (95, 95000), (0.001, 1), (99.999, 99999), (12.5, 12500)):
        assert ops._hd_percentile(ok) == qm
    big = torch.zeros(1, 1, 4, 257, dtype=torch.uint8)
    with pytest.raises(DfmirHipError, match="unsupported shape"):            # from the workspace query: no device is touched
        ops.label_hausdorff(big, big, [1])
    with pytest.raises(DfmirHipError, match="unsupported shape"):
        ops.label_edt_sq(torch.zeros(1, 1, 300, 4, 4, dtype=torch.uint8), 1)
    with pytest.raises(DfmirHipError, match="duplicate"):
        LabelHausdorff([3, 3])
    crit = LabelHausdorff(np.arange(1, 5), percentile=95, surface=True)
    assert crit.labels == [1, 2, 3, 4] and crit.percentile == 95.0 and crit.surface is True
    assert crit.directed is None and crit.mean is None
    with pytest.raises(DfmirHipError, match="no CPU fallback"):
        crit.compute(m, m.long())
    with pytest.raises(AssertionError, match="Only binary channel supported"):
        HausdorffDistance().compute(torch.zeros(1, 2, 8, 8), torch.zeros(1, 1, 8, 8))
    with pytest.raises(DfmirHipError, match="no CPU fallback"):
        HausdorffDistance().compute(torch.zeros(1, 1, 8, 8), torch.zeros(1, 1, 8, 8))


def test_hausdorff_option_parses_and_signatures_are_unchanged():
    from dfmir_amd import test as driver
    from dfmir_amd.infer import register_pair, score_labels
    base = vars(driver.parse(["--dataroot", "x"]))
    assert base.pop("hausdorff") is None
    with_q = vars(driver.parse(["--dataroot", "x", "--hausdorff", "95", "--fixed_label_dir", "trainB_label"]))
    assert with_q.pop("hausdorff") == 95.0 and with_q.pop("fixed_label_dir") == "trainB_label"
    assert base.pop("fixed_label_dir") is None and with_q == base               # nothing else moves
    ps = list(inspect.signature(register_pair).parameters.values())
    assert [p.name for p in ps] == ["model", "data", "label", "fixed_label", "labels"]
    assert [p.default for p in ps[2:]] == [None, None, None]
    ps = list(inspect.signature(score_labels).parameters.values())
    assert [p.name for p in ps] == ["warped_label", "fixed_label", "labels", "percentile", "surface"]
    assert [p.default for p in ps[3:]] == [100.0, False]


# ------------------------------------------------------------------------------------------ GPU tier
def _sparse_set(seed, shape):
    """A sparse random set over [B,1,*vol] with whole rows and whole planes empty."""
    m = (C.rand(seed, *shape) < (0.01 if int(np.prod(shape)) > 2000 else 0.1))
    if shape[-2] > 2:
        m[..., 2, :] = False                               # a whole row of every plane
    m[..., 5:9, :] = False
    if len(shape) == 5 and shape[2] > 2:
        m[:, :, 1] = False                                 # a whole plane
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 1, 37, 70), (2, 1, 5, 33, 70), (1, 1, 1, 40, 65), (1, 1, 9, 1, 13), (1, 1, 256, 256)],
                         ids=["2d_37x70", "3d_b2_5x33x70", "one_plane_40x65", "3d_9x1x13", "2d_256x256"])
def test_label_edt_sq_is_exact(shape):
    """ops.label_edt_sq against the restatement, bit for bit: a sparse set with empty rows and planes, one corner voxel
    (the largest d2), the empty set (all sentinel) and the full set (all 0), each with and without `surface`; the one-plane
    volume also equals the 2-D call.  256 x 256 is the largest supported line (a 64 KiB tile)."""
    from dfmir_amd import ops
    vol = shape[2:]
    corner = torch.zeros(shape, dtype=torch.bool)
    corner[(slice(None), 0) + (0,) * len(vol)] = True
    inputs = {"sparse": _sparse_set(7, shape), "corner": corner, "empty": torch.zeros(shape, dtype=torch.bool),
              "full": torch.ones(shape, dtype=torch.bool)}
    assert bool(inputs["sparse"].any())
    if shape[-1] == 256:
        del inputs["full"]
    for name, m in inputs.items():
        lab = (m.to(torch.uint8) * 7 + (~m).to(torch.uint8) * 2).contiguous()      # the set is value 7 among 2s
        for surface in (False, True):
            got = ops.label_edt_sq(lab.to(DEV), 7, surface=surface)
            assert got.dtype == torch.int32 and tuple(got.shape) == (shape[0],) + tuple(vol)
            for bi in range(shape[0]):
                s = m[bi, 0].numpy()
                ref = edt_sq_np(border_np(s) if surface else s)
                assert np.array_equal(got[bi].cpu().numpy(), ref), (name, surface, bi)
            if name == "corner":
                assert int(got.max()) == sum((n - 1) ** 2 for n in vol)
            if name == "empty":
                assert int(got.min()) == INF == int(got.max())
            if len(vol) == 3 and vol[0] == 1:
                assert torch.equal(got[:, 0], ops.label_edt_sq(lab[:, :, 0].contiguous().to(DEV), 7, surface=surface))


@pytest.mark.gpu
def test_hausdorff_distance_reproduces_the_reference(golden):
    """HausdorffDistance.compute on every B = 1 fixture case: d2 equals rint(ref^2) exactly, the fp32 value lies within
    one fp32 ulp of the reference's (sqrt of an exactly represented integer), inf equals inf."""
    from dfmir_amd import ops
    from dfmir_amd.losses import HausdorffDistance
    g = golden("hausdorff.npz")
    for nd in (2, 3):
        for case in FIXTURE_CASES:
            tag = "%dd_%s" % (nd, case)
            pred = torch.from_numpy(g[tag + "_pred"]).float().to(DEV) * 0.9 + 0.05         # 0.05 / 0.95 around the threshold
            target = torch.from_numpy(g[tag + "_target"]).float().to(DEV)
            ref = float(g[tag + "_hd"])
            got = HausdorffDistance().compute(pred, target)
            assert tuple(got.shape) == (1,) and got.dtype == torch.float32
            d2 = ops.label_hausdorff((pred > 0.5).to(torch.uint8), (target > 0.5).to(torch.uint8), [1])[3]
            print(tag, "ref", ref, "got", float(got[0]), "d2", d2.flatten().tolist())
            if np.isinf(ref):
                assert float(got[0]) == float("inf") and d2.flatten().tolist() == [INF, INF], tag
            else:
                assert int(d2.max()) == int(np.rint(np.float64(ref) ** 2)), tag
                assert abs(float(got[0]) - ref) <= ulp32(ref), (tag, float(got[0]), ref)


@pytest.mark.gpu
def test_hausdorff_scores_every_sample_on_its_own(golden):
    """The batch-mixing case (sample 0 holds only pred, sample 1 only target; the reference answers a finite distance
    across the batch axis) gives [inf, inf]; every sample of a B = 3 stack equals its own B = 1 call bit for bit."""
    from dfmir_amd import ops
    from dfmir_amd.losses import HausdorffDistance
    g = golden("hausdorff.npz")
    got = HausdorffDistance().compute(torch.from_numpy(g["mix_pred"]).float().to(DEV),
                                      torch.from_numpy(g["mix_target"]).float().to(DEV))
    assert got.tolist() == [float("inf"), float("inf")]
    vol = (6, 34, 66)
    a, b = blocky_labels(601, 3, vol, 3, 5).to(DEV), blocky_labels(602, 3, vol, 3, 5).to(DEV)
    b[2] = 0                                                # label 1 is missing from sample 2 of b
    whole = ops.label_hausdorff(a, b, [1, 2], percentile=95)
    assert bool(torch.isinf(whole[0][2, 0])) and bool(torch.isfinite(whole[0][:2]).all())
    for bi in range(3):
        one = ops.label_hausdorff(a[bi:bi + 1].contiguous(), b[bi:bi + 1].contiguous(), [1, 2], percentile=95)
        assert torch.equal(whole[0][bi:bi + 1], one[0])
        for w, o in zip(whole[1:], one[1:]):
            assert torch.equal(w[:, bi:bi + 1], o)


@pytest.mark.gpu
def test_label_hausdorff_multi_label():
    """K = 5 on [2,1,6,34,66]: a listed label absent from both maps and one present in `a` only give inf, unlisted values
    are ignored, the table equals K single-label calls bit for bit and follows the order of `labels`; K = 64 on
    [1,1,4,20,70] crosses the label-chunk boundary."""
    from dfmir_amd import ops
    vol = (6, 34, 66)
    a, b = blocky_labels(611, 2, vol, 6, 4), blocky_labels(612, 2, vol, 6, 4)        # values 0..5
    a[a == 5] = 9                                           # 9: in a only; 5: in b only (unlisted); 200: in neither
    labels = [3, 200, 1, 9, 2]
    a, b = a.to(DEV), b.to(DEV)
    got = ops.label_hausdorff(a, b, labels, percentile=90)
    assert tuple(got[0].shape) == (2, 5) and all(tuple(t.shape) == (2, 2, 5) for t in got[1:])
    assert got[0].dtype == got[1].dtype == got[2].dtype == torch.float32 and got[3].dtype == torch.int32
    for k in (1, 3):
        assert bool(torch.isinf(got[0][:, k]).all()) and bool(torch.isinf(got[1][:, :, k]).all())
        assert bool(torch.isinf(got[2][:, :, k]).all()) and bool((got[3][:, :, k] == INF).all())
    for k in (0, 2, 4):
        assert bool(torch.isfinite(got[0][:, k]).all())
    ref = hausdorff_table_np(a.cpu().numpy(), b.cpu().numpy(), labels, 90000)
    assert np.array_equal(got[3].cpu().numpy(), ref[3])
    for k, l in enumerate(labels):
        one = ops.label_hausdorff(a, b, [l], percentile=90)
        assert torch.equal(got[0][:, k:k + 1], one[0])
        for w, o in zip(got[1:], one[1:]):
            assert torch.equal(w[:, :, k:k + 1], o)
    swapped = ops.label_hausdorff(a, b, labels[::-1], percentile=90)
    assert torch.equal(swapped[0], got[0].flip(1)) and torch.equal(swapped[3], got[3].flip(2))
    vol = (4, 20, 70)
    a, b = blocky_labels(613, 1, vol, 70, 3).to(DEV), blocky_labels(614, 1, vol, 70, 3).to(DEV)
    labels = list(range(1, 65))
    got = ops.label_hausdorff(a, b, labels)
    assert int((got[3] < INF).sum()) > 64                  # most labels are present in both maps
    for k, l in enumerate(labels):
        one = ops.label_hausdorff(a, b, [l])
        assert torch.equal(got[0][:, k:k + 1], one[0])
        for w, o in zip(got[1:], one[1:]):
            assert torch.equal(w[:, :, k:k + 1], o)


def _ring_disc(vol):
    """target: a ring (shell) around the centre; pred: a small disc (ball) at the centre -- the largest distance pred ->
    target is at the centre of the disc, an interior voxel."""
    grid = np.meshgrid(*[np.arange(n) - (n - 1) // 2 for n in vol], indexing="ij")
    r2 = sum(x.astype(np.int64) ** 2 for x in grid)
    return (r2 <= 9)[None, None], ((r2 >= 49) & (r2 <= 72))[None, None]


@pytest.mark.gpu
def test_label_hausdorff_percentile_and_mean():
    """Percentile 95 and 50: d2 equals the restatement exactly, directed is its square root, the mean lies within rtol
    1e-6 of the float64 mean; with more than 95 % of the source voxels inside the other set d2 at 95 is 0."""
    from dfmir_amd import ops
    vol = (6, 34, 66)
    a, b = blocky_labels(621, 2, vol, 3, 6), blocky_labels(622, 2, vol, 3, 6)
    labels = [1, 2]
    for q in (95.0, 50.0, 100.0):
        got = ops.label_hausdorff(a.to(DEV), b.to(DEV), labels, percentile=q)
        ref = hausdorff_table_np(a.numpy(), b.numpy(), labels, int(round(q * 1000)))
        assert np.array_equal(got[3].cpu().numpy(), ref[3]), q
        assert np.array_equal(got[1].cpu().numpy(), np.sqrt(ref[3].astype(np.float64)).astype(np.float32)), q
        assert np.array_equal(got[0].cpu().numpy(), got[1].cpu().numpy().max(0)), q
        err = np.abs(got[2].cpu().numpy().astype(np.float64) - ref[2])
        print("percentile", q, "mean rel err", (err / ref[2]).max())
        assert (err <= 1e-6 * ref[2]).all(), (q, err)
    # a = b plus a thin sliver: > 95 % of a's voxels lie in b
    b1 = torch.zeros(1, 1, 40, 65, dtype=torch.uint8)
    b1[..., 5:35, 10:50] = 1
    a1 = b1.clone()
    a1[..., 5:35, 50:52] = 1                                # 60 of 1260 voxels outside b
    got = ops.label_hausdorff(a1.to(DEV), b1.to(DEV), [1], percentile=95)
    ref = hausdorff_table_np(a1.numpy(), b1.numpy(), [1], 95000)
    assert got[3].flatten().tolist() == [0, 0] == ref[3].flatten().tolist()
    assert float(got[0]) == 0.0 and float(got[2][0, 0, 0]) > 0.0 and float(got[2][1, 0, 0]) == 0.0
    full = ops.label_hausdorff(a1.to(DEV), b1.to(DEV), [1])
    assert full[3].flatten().tolist() == [4, 0]
    # mean=False: the same hd / directed / d2, no mean
    lean = ops.label_hausdorff(a1.to(DEV), b1.to(DEV), [1], mean=False)
    assert lean[2] is None and all(torch.equal(x, y) for x, y in zip((lean[0], lean[1], lean[3]), (full[0], full[1], full[3])))


@pytest.mark.gpu
@pytest.mark.parametrize("vol", [(37, 70), (21, 33, 70), (1, 37, 70)], ids=["2d", "3d", "one_plane"])
def test_label_hausdorff_surface(vol):
    """surface=True at percentile 100 and 95 against the restatement on the ring / disc case, where the border-to-border
    distance differs from the set-to-set one."""
    from dfmir_amd import ops
    pred, target = _ring_disc(vol)
    a = torch.from_numpy(pred.astype(np.uint8)).to(DEV)
    b = torch.from_numpy(target.astype(np.uint8)).to(DEV)
    plain = ops.label_hausdorff(a, b, [1])
    assert plain[3].flatten().tolist() == hausdorff_table_np(pred, target, [1])[3].flatten().tolist()
    for q in (100.0, 95.0):
        got = ops.label_hausdorff(a, b, [1], percentile=q, surface=True)
        ref = hausdorff_table_np(pred, target, [1], int(round(q * 1000)), surface=True)
        assert np.array_equal(got[3].cpu().numpy(), ref[3]), (q, got[3], ref[3])
        err = np.abs(got[2].cpu().numpy().astype(np.float64) - ref[2])
        assert (err <= 1e-6 * ref[2]).all(), (q, err)
        if q == 100.0:
            assert int(got[3][0, 0, 0]) < int(plain[3][0, 0, 0])      # the centre of the disc no longer counts


@pytest.mark.gpu
def test_label_hausdorff_is_bit_reproducible():
    from dfmir_amd import ops
    vol = (6, 34, 66)
    a, b = blocky_labels(631, 2, vol, 4, 5).to(DEV), blocky_labels(632, 2, vol, 4, 5).to(DEV)
    for kw in ({}, {"percentile": 95.0, "surface": True}):
        r0 = [t.clone() for t in ops.label_hausdorff(a, b, [1, 2, 3], **kw)]
        r1 = ops.label_hausdorff(a, b, [1, 2, 3], **kw)
        torch.cuda.synchronize()
        for x, y in zip(r0, r1):
            assert torch.equal(x, y)


@pytest.mark.gpu
def test_score_labels_scores_the_nearest_warped_ids():
    """infer.score_labels on register_pair's nearest-warped label ids equals ops.label_hausdorff on those ids against the
    fixed ids; LabelHausdorff keeps the directed and mean tables."""
    from dfmir_amd import ops
    from dfmir_amd.infer import register_pair, score_labels
    from dfmir_amd.losses import LabelHausdorff

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
    out = register_pair(_Stub(flow), data, mov.float())
    got = score_labels(out["warped_label"], fix.long(), labels, percentile=95.0)
    assert sorted(got) == ["directed", "hd", "mean"]
    warped = ops.as_label_map(out["warped_label"])
    ref = ops.label_hausdorff(warped, fix.to(DEV), labels, percentile=95.0)
    assert torch.equal(got["hd"], ref[0]) and torch.equal(got["directed"], ref[1]) and torch.equal(got["mean"], ref[2])
    assert bool(torch.isfinite(got["hd"]).all()) and float(got["hd"].max()) > 0
    crit = LabelHausdorff(labels, percentile=95.0)
    assert torch.equal(crit.compute(out["warped_label"], fix.to(DEV).long()), ref[0])
    assert torch.equal(crit.directed, ref[1]) and torch.equal(crit.mean, ref[2])
