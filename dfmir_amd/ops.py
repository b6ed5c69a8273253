"""torch.autograd.Function wrappers over the C ABI of libdfmir_hip.so.

Every op here launches hand-written gfx950 kernels on torch's *current* HIP stream with raw device
pointers; torch is used only for memory, streams and the autograd tape.  There is no CPU or
eager-PyTorch fallback: a non-CUDA tensor raises.
"""
import collections
import ctypes
import functools
import math
import os

import numpy as np
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ._lib import DfConvGeom, DfmirHipError, check, lib

_VP = ctypes.c_void_p


def _p(t):
    return None if t is None else _VP(t.data_ptr())


def _st():
    return _VP(torch.cuda.current_stream().cuda_stream)


def _need(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise DfmirHipError("dfmir_amd ops run only on the HIP device (got a %s tensor); "
                                "there is no CPU fallback" % t.device)
        if t.dtype not in (torch.float32, torch.int64, torch.bool, torch.uint8):
            raise DfmirHipError("unsupported dtype %s" % t.dtype)


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


def zero_(t):
    """t.zero_() as a kernel launch.  torch zeroes contiguous tensors with hipMemsetAsync, which a captured step turns
    into hipGraph memset nodes; those are not reliably ordered with neighbouring kernel nodes on ROCm 7.2
    (scripts/graph_probe.py memset_order), so nothing on the step path uses torch.zeros / zero_ / zeros_like."""
    if t.numel():
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32):
            raise DfmirHipError("ops.zero_: contiguous fp32 device tensors only")
        check(lib().dfmir_fill_zero(_p(t), t.numel(), _st()))
    return t


def zeros(shape, device):
    return zero_(torch.empty(shape, device=device, dtype=torch.float32))


def zeros_like(t):
    return zero_(torch.empty_like(t, memory_format=torch.contiguous_format))


def _env_on(name):
    """A/B switch from the environment, read at import: on unless unset, "" or "0" (the semantics of the library's own
    DfOptFlag, include/dfmir_hip.h "Options").  These Python-side switches select host-side call paths and are
    ENVIRONMENT-ONLY: dfmir_set_option() after import changes the C side alone."""
    v = os.environ.get(name)
    return v is not None and v not in ("", "0")


# ------------------------------------------------------------------------------------------------
# raw launches
# ------------------------------------------------------------------------------------------------
# conv_raw / conv_wgrad_raw go in three steps: _plan_conv_* picks the kernel (the one place that asks the library's *_ok
# queries and reads the A/B switches), _launch_conv_* issues it, _conv_*_label names it for the profiler below.
# Optional launch profiler (bench.py): called as prof(kind, flops, launch) where launch() issues
# the kernel; lets the bench bracket the dominant kernel with HIP events on the launch stream.
_CONV_PROFILER = [None]


def set_conv_profiler(fn):
    _CONV_PROFILER[0] = fn


# Range probes (max |t|) of the fp16x2 split kernels (csrc/conv3x3s.hip).  Slots come zero-initialised from
# a pool (one fill per 4096 probes).  A producer that computes the maximum as a by-product (InstanceNorm
# forward / backward) tags its output tensor with it; `amax_of` reuses the tag while the tensor is unmodified.
PROBE_SLOTS = 64          # DFMIR_PROBE_SLOTS: floats of an InstanceNorm by-product probe
_AMAX_POOL = {"buf": None, "next": 0, "gen": 0}


def amax_slot(device, n=1):
    """n floats of zero-initialised device memory (a probe = n partial maxima)."""
    pool = _AMAX_POOL
    if pool["buf"] is None or pool["next"] + n > pool["buf"].numel() or pool["buf"].device != device:
        if pool.get("capturing") and pool["buf"] is not None:
            raise DfmirHipError("probe pool exhausted inside a graph capture (a replay would not re-zero the new pool)")
        pool["buf"] = zeros(max(1 << 18, n), device)
        pool["next"] = 0
    i = pool["next"]
    pool["next"] = i + n
    return pool["buf"][i:i + n]


def prepare_step(device):
    """What a step triggers lazily on first use and every stream of the step then relies on -- the batched re-pack of all
    weights after an optimizer step, a probe pool with room for a whole step -- done NOW, on the current stream: a step
    that forks work onto a second stream (registration_model._forward_backward) calls this before the fork."""
    ep = weights_epoch()
    if _PACKS["epoch"] != ep and _PACKS["entries"]:
        _repack_all(ep)
    pool = _AMAX_POOL
    if pool["buf"] is None or pool["buf"].device != device:
        amax_slot(device, 0)
    elif pool["next"] + (1 << 16) > pool["buf"].numel() and not pool.get("capturing"):
        pool["buf"] = zeros(1 << 18, device)
        pool["next"] = 0


def begin_graph_capture():
    """Called right before a hipGraph capture of the step: probe slots handed out during the capture must be zeroed by
    the graph itself at every replay, so the pool is re-created (allocation + zero fill) inside the capture."""
    _AMAX_POOL["buf"] = None
    _AMAX_POOL["capturing"] = True


def end_graph_capture():
    _AMAX_POOL["capturing"] = False


def invalidate_after_failed_capture():
    """A capture that raised has RECORDED launches without running them, while the host-side caches were updated as if
    they had run: the batched weight re-pack (and the 3-D split workspaces derived from it) is marked current for this
    weights epoch, and the probe pool handed out during the capture was allocated and zero-filled only by the dead graph.
    Forget both: the next eager step re-packs every weight, re-splits every 3-D workspace and starts a fresh, really
    zeroed probe pool."""
    _AMAX_POOL["buf"] = None
    _AMAX_POOL["capturing"] = False
    _AMAX_POOL["gen"] += 1                                         # tags that point into the dead capture's pool expire
    _PACKS["epoch"] = None
    _PACKS["key"] = _WS3D["key"] = None                           # job tables uploaded inside the capture never arrived
    for j_ in _JOBS_BY_GROUP.values():
        j_["key"] = None
    for e in _PACKS["entries"].values():
        e["epoch"] = None
    for e in _WS3D["entries"].values():
        w = e["ref"]()
        cache = getattr(w, "_df_ws3d", None) if w is not None else None
        if cache is not None and e["key"] in cache:
            cache[e["key"]] = (None, cache[e["key"]][1])          # generation None never matches: re-split in place


def absmax(t):
    out = amax_slot(t.device)
    check(lib().dfmir_absmax(_p(t), t.numel(), _p(out), _st()))
    return out


def tag_amax(t, slot):
    t._df_amax = (slot, t._version, t.data_ptr(), _AMAX_POOL["gen"])
    return t


def _amax_ok(t, tag):
    """The tag still describes t (same version, same storage) AND its slot comes from a probe pool that really ran: a
    capture that failed hands out slots of a graph-private pool that no launch ever filled (invalidate_after_failed_capture
    bumps the pool generation)."""
    return tag[1] == t._version and tag[2] == t.data_ptr() and tag[3] == _AMAX_POOL["gen"]


def amax_of(t):
    tag = getattr(t, "_df_amax", None)
    if tag is not None and _amax_ok(t, tag):
        return tag[0]
    return absmax(t)


_NO_SPLIT3D = _env_on("DFMIR_CONV3D_FP32") or _env_on("DFMIR_CONV_FP32")

# Probe audit (DFMIR_PROBE_AUDIT=1 or set_probe_audit(True); debugging / test mode, one device sync per conv launch).
# The fp16x2 split scales a tensor by its range PROBE, and probes are inherited (blur outputs, nearest_up2 + cat,
# sampled-feature scatters, dgrad epilogues); a probe below the true maximum would overflow fp16 silently.  In audit
# mode every split launch first measures the true max |t| of each operand with dfmir_absmax and raises if the probe
# it was handed is smaller (per-plane dY maxima of the weight gradient included).
_PROBE_AUDIT = {"on": _env_on("DFMIR_PROBE_AUDIT"), "log": []}


def set_probe_audit(on):
    _PROBE_AUDIT["on"] = bool(on)
    _PROBE_AUDIT["log"] = []
    return _PROBE_AUDIT["log"]


def _audit_probe(t, probe, what, plane_max=None):
    true = torch.zeros(1, device=t.device, dtype=torch.float32)
    tc = _c(t)
    check(lib().dfmir_absmax(_p(tc), tc.numel(), _p(true), _st()))
    pv, tv = float(probe.max()), float(true)
    _PROBE_AUDIT["log"].append((what, pv, tv))
    if tv == tv and not pv >= tv:
        raise DfmirHipError("probe audit: %s has max|t| = %.6g but its range probe says %.6g" % (what, tv, pv))
    if plane_max is not None:                 # per-(n, c) maxima of dY (split weight gradient)
        pm = tc.reshape(plane_max.numel(), -1).abs().amax(dim=1)
        bad = (plane_max.reshape(-1) < pm)
        if bool(bad.any()):
            i = int(bad.nonzero()[0])
            raise DfmirHipError("probe audit: %s plane %d has max %.6g but its per-plane probe says %.6g"
                                % (what, i, float(pm[i]), float(plane_max.reshape(-1)[i])))


def _wants_amax(K, stride, dil, Di, Cin, Cout):
    """Shapes the split kernels take (the C side decides, asked by _plan_conv_fwd / _plan_conv_wgrad; this only avoids useless
    probes): 2-D 3x3 with more than 32 output channels (csrc/conv3x3s.hip), 3-D 3x3x3 with at least 8 channels on both sides
    (csrc/conv3ds.hip; their weight gradient: csrc/conv3dsw.hip)."""
    if tuple(K) == (3, 3, 3):   # Cout < 8 (the flow conv): only its weight gradient is split (swapped operand roles)
        return stride == 1 and dil == 1 and Di > 1 and Cin >= 8 and Cout >= 1 and not _NO_SPLIT3D
    return tuple(K) == (1, 3, 3) and stride == 1 and dil == 1 and Di == 1 and Cout > 32 and Cin >= 16


# A/B switches of the conv paths, from the environment at import; tests assign to them later: read them at call time
_NO_TINY3D = _env_on("DFMIR_CONV3D_NO_TINY")  # A/B switch: the flow head on the split kernels
_NO_TINYVOL = _env_on("DFMIR_NO_TINYVOL")     # A/B switch (also read by the library): no conv_tinyvol_k
_NO_S2 = _env_on("DFMIR_CONV3D_NO_S2")        # A/B switch: the stride-2 encoder levels on the generic gather kernels
_NO_FLOW_MARCH = _env_on("DFMIR_CONV3D_NO_FLOW_MARCH")  # A/B switch: the flow head's forward on the fp32-FMA kernel
_NO_ACTGRAD = _env_on("DFMIR_NO_ACTGRAD")     # A/B switch: LeakyReLU backward always as its own pass
_NO_RES = _env_on("DFMIR_NO_RES")       # A/B switch: residual added by a separate kernel
_NO_CH_SCALE = _env_on("DFMIR_NO_CH_SCALE")   # A/B switch: one dY scale per tensor in the split wgrad
_LAST_ACTGRAD = [False]     # did the last conv_raw() apply an activation derivative in its epilogue?


def _size_label(c, small=True):     # channel class in the bench profiler's kinds (the weight gradient has no "small")
    return "L" if c > 64 else ("M" if c > 32 else ("S" if c > 4 or not small else "small"))


def _call_profiler(prof, launch, kind, flops, issued):
    if issued is not None and getattr(prof, "accepts_issued", False):
        prof(kind, flops, launch, issued)
    else:
        prof(kind, flops, launch)


_ConvFwdPlan = collections.namedtuple("_ConvFwdPlan", "kernel cout_used act_src fuse_res tiling")


def _plan_conv_fwd(g, K, probe, res, ring, cout_used, no_bias, act_src):
    """Which forward kernel takes the layer g: flow_march | tiny3d | s2c2 | s2m | s2d | march3d | split3d | res2d | generic.
    Pure: no launch, no allocation; asks the library's *_ok queries in a fixed order, each only while its answer matters.
    cout_used, act_src: what the caller asked for where that kernel does it, else None; fuse_res: the residual goes into the
    epilogue; tiling: the split tiling ("split" / "march") that took the layer, or None -- the label counts its issued products
    even under a stride-2 kernel, which launches ahead of it (the real library never accepts a layer for both)."""
    L, gp = lib(), ctypes.byref(g)
    N, Cin, Cout, Wi, stride, dil, act = g.N, g.Cin, g.Cout, g.Wi, g.stride, g.dil, g.act
    yshape, vol = (N, Cout, g.Do, g.Ho, g.Wo), g.Do * g.Ho * g.Wo
    if res is not None or ring is not None:       # only the 2-D 3x3 epilogue folds them in; otherwise a separate add
        fuse_res = bool(res is not None and not _NO_RES and probe and res.is_contiguous() and tuple(res.shape) == yshape
                        and L.dfmir_conv3x3_res_ok(gp))
        return _ConvFwdPlan("res2d" if (fuse_res or ring is not None) else "generic", None, None, fuse_res, None)
    if tuple(K) != (3, 3, 3):
        return _ConvFwdPlan("generic", None, None, False, None)
    # the flow head / its data gradient (16 -> 3, 3 -> 16): plain fp32 FMAs (csrc/conv3dt.hip)
    tiny = not _NO_TINY3D and (cout_used is None or cout_used == Cout) and bool(L.dfmir_conv3d_tiny_ok(gp))
    # ... the head itself on the z-marching kernel's FLOW form when the volume is large enough for it (csrc/conv3dm.hip)
    flow = (tiny and Cin == 16 and Cout == 3 and act == 0 and act_src is None and probe and not _NO_FLOW_MARCH
            and Wi % 4 == 0 and bool(L.dfmir_conv3d_march_ok(gp)))
    # the first encoder level (2 -> 16, stride 2) from an LDS-staged patch (csrc/conv3dt.hip)
    s2c2 = not tiny and stride == 2 and Cin == 2 and not _NO_TINY3D and cout_used is None and bool(L.dfmir_conv3d_s2c2_ok(gp))
    # the deeper stride-2 encoder levels and their data gradients (fp32 MFMA from LDS-staged patches: csrc/conv3ds2.hip)
    plain = cout_used is None and act_src is None and not _NO_S2
    s2m = plain and not s2c2 and stride == 2 and dil == 1 and bool(L.dfmir_conv3d_s2_ok(gp))
    s2d = plain and stride == 1 and dil == 2 and no_bias and act == 0 and bool(L.dfmir_conv3d_s2_dgrad_ok(gp))
    split = not tiny and not s2c2 and probe and bool(L.dfmir_conv3d_split_ok(gp))
    # <= 512 output voxels per image (the deepest levels of the 6-level U-Net: 8^3, 4^3, 2^3): a split launch costs its
    # 45-80 us of prologue whatever the volume; conv_tinyvol_k (behind dfmir_conv_fwd_scaled) takes 20-30
    if split and cout_used is None and not _NO_TINYVOL and Cout <= 64 and vol <= 512 and N * vol <= 8192:
        split = False
    if not split:
        cout_used = None                                     # only the split 3-D kernel computes a channel subset
    # the full-resolution layers with Cin x Cout <= 512: the z-marching kernel (csrc/conv3dm.hip)
    march = split and (cout_used is None or cout_used == Cout) and Wi % 4 == 0 and bool(L.dfmir_conv3d_march_ok(gp))
    if act_src is not None and not ((split or tiny) and act == 0 and tuple(act_src.shape) == yshape and act_src.is_contiguous()):
        act_src = None                                       # ... and only these epilogues apply an activation derivative
    kernel = ("flow_march" if flow else "tiny3d" if tiny else "s2c2" if s2c2 else "s2m" if s2m else "s2d" if s2d
              else "march3d" if march else "split3d" if split else "generic")
    return _ConvFwdPlan(kernel, cout_used, act_src, False, "march" if march else "split" if split else None)


def _launch_probed(y, call):
    """Issue a kernel that leaves the range probe of y for the next layer: call(pointer to a fresh probe)."""
    slot = amax_slot(y.device, PROBE_SLOTS)
    check(call(_p(slot)))
    tag_amax(y, slot)              # survives as is when y is a backward result (dgrad) ...
    _LAST_CONV_AMAX[0] = slot      # ... and is re-attached by conv() to the tensor Function.apply returns


def _launch_conv_fwd(plan, g, x5, x_amax, w_tcc, bias, y, res, ring, act_slope):
    L, gp, k = lib(), ctypes.byref(g), plan.kernel
    x, w, b, yp, src, slope = _p(x5), _p(w_tcc), _p(bias), _p(y), _p(plan.act_src), float(act_slope)
    xa, xa_n = _p(x_amax), 0 if x_amax is None else x_amax.numel()
    if k in ("flow_march", "march3d"):                        # (the FLOW form has no activation derivative: src is None)
        slope = slope if k == "march3d" else 0.0
        _launch_probed(y, lambda slot: L.dfmir_conv3d_march_fwd(gp, x, xa, xa_n, w, b, yp, slot, src, slope, _st()))
    elif k == "tiny3d":
        _launch_probed(y, lambda slot: L.dfmir_conv3d_tiny_fwd(gp, x, w, b, yp, slot, src, slope, _st()))
    elif k in ("s2c2", "s2m"):
        fn = L.dfmir_conv3d_s2c2_fwd if k == "s2c2" else L.dfmir_conv3d_s2_fwd
        _launch_probed(y, lambda slot: fn(gp, x, w, b, yp, slot, _st()))
    elif k == "s2d":
        check(L.dfmir_conv3d_s2_dgrad(gp, x, w, yp, _st()))
    elif k == "split3d":
        # fp16x2 split form on the 16-bit matrix pipe.  The split weights are kept per packed-weight buffer and re-made only when
        # it was re-packed (generation and cache live ON the persistent buffer's tensor object: a temporary packing has neither)
        Cin, Cout = g.Cin, g.Cout
        cu = Cout if plan.cout_used is None else plan.cout_used
        pair_ = L.dfmir_conv3d_split_is_pair(cu)
        ws, need_ = _ws_cached(w_tcc, (Cin, Cout, cu), L.dfmir_conv3d_split_ws_floats(Cin, Cout), x5.device,
                               job=(0, Cin, cu if pair_ else Cout, pair_, Cin, 0, 0))
        w, ws = (w if need_ else None), _p(ws)
        if plan.act_src is not None:   # dgrad into the output of a LeakyReLU: the epilogue applies its derivative (csrc/conv3ds.hip)
            _launch_probed(y, lambda slot: L.dfmir_conv3d_split_fwd_actgrad(gp, x, xa, xa_n, w, ws, b, yp, slot, cu, src, slope, _st()))
        else:
            _launch_probed(y, lambda slot: L.dfmir_conv3d_split_fwd_sub(gp, x, xa, xa_n, w, ws, b, yp, slot, cu, _st()))
    elif k == "res2d":
        check(L.dfmir_conv3x3_fwd_scaled_res(gp, x, xa, xa_n, w, b, _p(res) if plan.fuse_res else None,
                                             *((_p(ring[0]), ring[1]) if ring is not None else (None, 0)), yp, _st()))
    else:
        check(L.dfmir_conv_fwd_scaled(gp, x, xa, xa_n, w, b, yp, _st()))
    if res is not None and not plan.fuse_res:
        y.add_(res.reshape(y.shape))


def _conv_fwd_label(plan, g):
    """(kind, flops, issued or None) of the launch for the bench profiler (bench.py keys on the kind strings)."""
    N, Cin, Cout, dil = g.N, g.Cin, g.Cout, g.dil
    K, pad = (g.KD, g.KH, g.KW), (g.pd, g.ph, g.pw)
    flops = 2.0 * N * Cout * g.Do * g.Ho * g.Wo * Cin * K[0] * K[1] * K[2] / (dil ** 3 if K[0] > 1 else dil ** 2)
    size = _size_label(Cout)
    is3x3 = K == (1, 3, 3) and g.stride == 1 and dil == 1 and g.Di == 1 and pad[1] == pad[2] and pad[1] in (1, 2) and Cout > 4
    is3d = (K == (3, 3, 3) and g.stride == 1 and dil == 1 and pad == (1, 1, 1) and g.pad_mode == 0
            and not (Cout <= 4 and Cin < 8))              # what csrc/conv3d.hip::df_conv3d_fwd_try takes
    kind = ("conv3dt_" if plan.kernel in ("flow_march", "tiny3d", "s2c2", "s2m", "s2d") else "conv3x3_" if is3x3
            else ("conv3ds_" if plan.tiling else "conv3d_") if is3d else "conv_mfma_") + size
    if not plan.tiling:
        return kind, flops, None
    # 16-bit products the kernel ISSUES per algorithmic MAC: 3 (a0b0 + a0b1 + a1b0) x the padding of its tiling --
    # taps 27 -> 28 (plane-pair rows: 27 -> 36 taps'), input channels to whole chunks of 8, output channels to 32 rows
    cu = Cout if plan.cout_used is None else plan.cout_used
    form_ = lib().dfmir_conv3d_split_is_pair(cu)      # 0: 32 rows, 1: plane pairs (36 taps'), 2: 16 rows
    pad_k = (36.0 if form_ == 1 else 28.0) / 27.0 * (8.0 * ((Cin + 7) // 8)) / Cin
    pad_m = (16.0 / cu) if form_ else (32.0 * ((cu + 31) // 32)) / cu
    if plan.tiling == "march":                        # no padded rows; 16 -> 16 walks 10 tap slots per 9 taps
        pad_k, pad_m = ((10.0 / 9.0) if (Cin == 16 and Cout == 16) else 1.0), 1.0
    return kind, flops * cu / Cout, 3.0 * pad_k * pad_m * flops * cu / Cout


def conv_raw(x5, w_tcc, bias, Cout, K, stride, pad, dil, pad_mode, act, slope, out_sp, x_amax=None, res=None, ring=None,
             cout_used=None, act_src=None, act_slope=0.0):
    """res (optional, shape of the output): y = act(conv + bias) + res, inside the kernel's epilogue where the
    library has one (dfmir_conv3x3_res_ok), else by a separate add.  ring = (buffer, row length) of
    dfmir_conv3x3_reflect_ring: folded in by the same epilogue (the caller checked dfmir_conv3x3_res_ok)."""
    N, Cin, Di, Hi, Wi = x5.shape
    y = torch.empty((N, Cout) + tuple(out_sp), device=x5.device, dtype=torch.float32)
    g = DfConvGeom(N, Cin, Cout, Di, Hi, Wi, out_sp[0], out_sp[1], out_sp[2], K[0], K[1], K[2],
                   stride, dil, pad[0], pad[1], pad[2], pad_mode, act, float(slope))
    plan = _plan_conv_fwd(g, K, x_amax is not None, res, ring, cout_used, bias is None, act_src)
    _LAST_ACTGRAD[0] = plan.act_src is not None
    if _PROBE_AUDIT["on"] and x_amax is not None:
        _audit_probe(x5, x_amax, "conv input %s -> %d ch, k=%s" % (tuple(x5.shape), Cout, tuple(K)))
    launch = functools.partial(_launch_conv_fwd, plan, g, x5, x_amax, w_tcc, bias, y, res, ring, act_slope)
    prof = _CONV_PROFILER[0]
    if prof is None:
        launch()
    else:
        _call_profiler(prof, launch, *_conv_fwd_label(plan, g))
    return y


def _tag_ok(t, tag):
    return tag is not None and tag[-2] == t._version and tag[-1] == t.data_ptr()


# dfmir_conv3d_upwgrad below this many low-resolution voxels per image: the direct kernel over both parts.  With MORE than two
# skip channels their share runs on the direct kernel anyway and the split only pays at the largest volumes
# (profiles/r05_bench_upwgrad.txt: 48 -> 32 at 80x96x112 0.32 vs 0.29 ms); two skip channels ride in the same launch.
_UPWGRAD_MIN_VOX = int(os.environ.get("DFMIR_UPWGRAD_MIN_VOX", "400000"))
_UPWGRAD_MIN_VOX_FUSED = 50000
_UPWGRAD_WS = {}


def _upwgrad_ws(device):
    """64 accumulator tiles of dfmir_conv3d_upwgrad: one buffer per (device, stream) -- the call zeroes it, fills it and
    folds it on the caller's stream, so launches of one stream may share it."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _UPWGRAD_WS.get(key)
    if ws is None:
        ws = _UPWGRAD_WS[key] = torch.zeros(int(lib().dfmir_conv3d_upwgrad_ws_floats()), device=device)
    return ws


# Deterministic weight gradients (opt.deterministic_wgrad -> set_deterministic_wgrad; build-defined).  The weight- and
# bias-gradient kernels split their reduction over workgroups and meet in fp32 atomics: every run rounds in a different
# order (2 of 30 runs of one test exceeded a 4e-5 bound on step 4's gradients because of it).  In this mode each
# gradient launch accumulates 64-bit fixed-point integers into a per-call scratch (include/dfmir_hip.h "Deterministic
# weight gradients") -- integer addition is associative -- and a finaliser adds the converted sums to the real target: two
# runs of a step from the same state give bit-identical gradient arenas.  Cost: one zero-fill, one scale launch and one
# finaliser per gradient launch, and the bias gradients as their own pass over dY.
_DET = {"on": _env_on("DFMIR_DETERMINISTIC_WGRAD")}


def set_deterministic_wgrad(on):
    _DET["on"] = bool(on)


def deterministic_wgrad():
    return _DET["on"]


class _DetAcc(object):
    def __init__(self, n_dw, n_db, count, x, x_amax, dy, dy_amax):
        head = int(lib().dfmir_det_head_floats())
        self.n_dw, self.n_db = int(n_dw), int(n_db)
        self.scr = torch.empty(head + 2 * (self.n_dw + self.n_db), device=dy.device, dtype=torch.float32)
        check(lib().dfmir_det_begin(_p(self.scr), self.n_dw + self.n_db, _p(x), 0 if x is None else x.numel(), _p(x_amax),
                                    0 if x_amax is None else x_amax.numel(), _p(dy), dy.numel(), _p(dy_amax),
                                    0 if dy_amax is None else dy_amax.numel(), float(count), _st()))
        self.dw = self.scr[head:head + 2 * self.n_dw]              # the entry points see 8-byte slots behind this pointer
        self.db = self.scr[head + 2 * self.n_dw:] if self.n_db else None

    def end(self, dw_out, db_out):
        check(lib().dfmir_det_end(_p(self.scr), _p(dw_out), self.n_dw, _p(db_out), self.n_db if db_out is not None else 0, _st()))

    def abort(self):
        check(lib().dfmir_det_end(_p(self.scr), None, 0, None, 0, _st()))


def bias_grad(dy5, db):
    """db[c] += sum over (n, voxels) of dy5[n, c] (accumulates); deterministic mode: through the fixed-point scratch."""
    N, C = dy5.shape[0], dy5.shape[1]
    S = dy5.numel() // (N * C)
    if not _DET["on"]:
        check(lib().dfmir_bias_grad(_p(dy5), _p(db), N, C, S, _st()))
        return
    acc = _DetAcc(0, C, N * S, dy5, None, dy5, None)         # (x plays no part: the bound is count * max|dy|)
    try:
        check(lib().dfmir_bias_grad(_p(dy5), _p(acc.db), N, C, S, _st()))
    except BaseException:
        acc.abort()
        raise
    acc.end(None, db)


_WGRAD_SPLIT = ("upwgrad", "split_upcat", "split3d")      # the kernels behind dfmir_conv3d_split_wgrad_ok


def _plan_conv_wgrad(g, K, probed, parts):
    """Which weight-gradient kernel takes the layer g: s2c2 | s2m | upwgrad | split_upcat | split3d | generic.  Pure, like
    _plan_conv_fwd; probed = the caller has the range probes of both operands."""
    L, gp = lib(), ctypes.byref(g)
    k3 = tuple(K) == (3, 3, 3)
    split = probed and k3 and bool(L.dfmir_conv3d_split_wgrad_ok(gp))
    if parts is not None:
        if not split:
            raise DfmirHipError("conv_wgrad_raw(parts=...) needs the split 3-D weight-gradient kernel")
        # the up-sampled channels in parity classes (csrc/conv3duw.hip) where the volume fills the chip
        min_vox = min(_UPWGRAD_MIN_VOX, _UPWGRAD_MIN_VOX_FUSED) if parts[1].shape[1] == 2 else _UPWGRAD_MIN_VOX
        upw = parts[0][0, 0].numel() >= min_vox and L.dfmir_conv3d_upwgrad_ok(gp, parts[0].shape[1])
        return "upwgrad" if upw else "split_upcat"
    if k3 and g.stride == 2:
        if g.Cin == 2 and not _NO_TINY3D and L.dfmir_conv3d_s2c2_ok(gp):
            return "s2c2"
        if not _NO_S2 and L.dfmir_conv3d_s2_ok(gp):
            return "s2m"
    return "split3d" if split else "generic"


def _launch_conv_wgrad(kernel, g, x5, dy5, x_amax, dy_amax, dy_pmax, parts, dw, db):
    L, gp = lib(), ctypes.byref(g)
    x, dy, dwp, dbp = _p(x5), _p(dy5), _p(dw), _p(db)
    xa, xa_n = _p(x_amax), 0 if x_amax is None else x_amax.numel()
    ya, ya_n = _p(dy_amax), 0 if dy_amax is None else dy_amax.numel()
    if kernel == "s2c2":
        if db is not None:
            check(L.dfmir_bias_grad(dy, dbp, dy5.shape[0], g.Cout, g.Do * g.Ho * g.Wo, _st()))   # accumulates
        check(L.dfmir_conv3d_s2c2_wgrad(gp, x, dy, dwp, _st()))
    elif kernel == "s2m":
        check(L.dfmir_conv3d_s2_wgrad(gp, x, dy, dwp, dbp, _st()))   # db fused
    elif kernel in ("upwgrad", "split_upcat"):
        args = (gp, _p(parts[0]), _p(parts[1]), parts[0].shape[1], xa, xa_n, dy, ya, ya_n, dwp, dbp)
        check(L.dfmir_conv3d_upwgrad(*args, _p(_upwgrad_ws(dy5.device)), _st()) if kernel == "upwgrad"
              else L.dfmir_conv3d_split_wgrad_upcat(*args, _st()))
    elif kernel == "split3d":
        check(L.dfmir_conv3d_split_wgrad_db(gp, x, xa, xa_n, dy, ya, ya_n, dwp, dbp, _st()))   # db fused
    else:
        pm = dy_pmax if (dy_pmax is not None and dy_pmax.numel() == g.N * g.Cout and dy_amax is not None) else None
        check(L.dfmir_conv_wgrad_scaled_ch(gp, x, xa, xa_n, dy, ya, ya_n, _p(pm), dwp, dbp, _st()))


def _conv_wgrad_label(kernel, g, x5, dy5, parts, want_issued):
    """(kind, flops, issued or None) of the launch for the bench profiler; want_issued: the profiler takes the issued
    products (the parity-class kernel has a kind of its own only then)."""
    Cin, Cout, Wi = g.Cin, g.Cout, g.Wi
    K, pad = (g.KD, g.KH, g.KW), (g.pd, g.ph, g.pw)
    size = _size_label(Cout, small=False)
    flops = 2.0 * g.N * Cout * g.Do * g.Ho * g.Wo * Cin * (K[0] * K[1] * K[2])
    split = kernel in _WGRAD_SPLIT
    is3x3 = (K == (1, 3, 3) and g.stride == 1 and g.Di == 1 and pad[1] == 1 and pad[2] == 1 and Cout >= 64 and Cin >= 32
             and (g.Hi * Wi) % 32 == 0 and Wi % 32 == 0)
    is3d = (K == (3, 3, 3) and g.stride == 1 and pad == (1, 1, 1) and g.pad_mode == 0 and Cout <= 32
            and Wi % 4 == 0)                              # csrc/conv3d.hip::df_conv3d_wgrad_try
    kind = ("wgrad3dt_S" if kernel in ("s2c2", "s2m") else
            ("wgrad3x3_" if is3x3 else (("wgrad3ds_" if split else "wgrad3d_") if is3d else "conv_wgrad_")) + size)
    if not (split and is3d and want_issued):
        return kind, flops, None
    # 16-bit products the kernel ISSUES per algorithmic MAC (cf. _conv_fwd_label): 3 x the padding of its tiling
    if kernel == "upwgrad":     # parity classes: 8 / 27 of the up-sampled share, 32 columns; fused skip pair: 54 -> 64 rows
        Ca_, Cb_ = parts[0].shape[1], parts[1].shape[1]
        skip_ = (64.0 / 54.0) if Cb_ == 2 else (28.0 / 27.0) * (8.0 * ((Cb_ + 7) // 8)) / Cb_
        pad_ = ((8.0 / 27.0) * Ca_ + skip_ * Cb_) / Cin * (32.0 / Cout)
        kind = "wgrad3dup_" + size
    elif Cout < 8:          # the flow head: roles swapped, rows = (tap, co of a chunk of 8), columns = ci of 32
        pad_ = (28.0 / 27.0) * (8.0 / Cout) * (32.0 / Cin)
    elif parts is None and lib().dfmir_conv3d_wgrad_is_march_at(ctypes.byref(g), _p(x5), _p(dy5)):   # 14 tiles of two taps for 27
        pad_ = 28.0 / 27.0
    elif Cout <= 16:        # plane-pair columns: 36 taps' of 27, 16 columns per plane
        pad_ = (36.0 / 27.0) * (8.0 * ((Cin + 7) // 8)) / Cin * (16.0 / Cout)
    else:
        pad_ = (28.0 / 27.0) * (8.0 * ((Cin + 7) // 8)) / Cin * (32.0 / Cout)
    return kind, flops, 3.0 * pad_ * flops


def conv_wgrad_raw(x5, dy5, K, stride, pad, pad_mode, out=None, x_amax=None, dy_amax=None, db=None, dy_pmax=None,
                   parts=None):
    """dW in the tap-major packing; `out` (same packing) is accumulated into when given.  parts = (a, b): the operand is
    cat(nearest_up2(a), b), never built (x5 is None; the caller checked upcat_wgrad_ok)."""
    if parts is not None:
        x5 = parts[1]
    N, Cin, Di, Hi, Wi = x5.shape
    if parts is not None:
        Cin += parts[0].shape[1]
    _, Cout, Do, Ho, Wo = dy5.shape
    dw = zeros((K[0] * K[1] * K[2], Cin, Cout), x5.device) if out is None else out
    g = DfConvGeom(N, Cin, Cout, Di, Hi, Wi, Do, Ho, Wo, K[0], K[1], K[2], stride, 1, pad[0], pad[1],
                   pad[2], pad_mode, 0, 0.0)
    kernel = _plan_conv_wgrad(g, K, x_amax is not None and dy_amax is not None, parts)
    if _PROBE_AUDIT["on"]:
        if x_amax is not None:
            for t_ in (parts if parts is not None else (x5,)):
                _audit_probe(t_, x_amax, "wgrad x %s" % (tuple(t_.shape),))
        if dy_amax is not None:
            pm_ = dy_pmax if (dy_pmax is not None and dy_pmax.numel() == N * Cout and kernel not in _WGRAD_SPLIT) else None
            _audit_probe(dy5, dy_amax, "wgrad dY %s" % (tuple(dy5.shape),), plane_max=pm_)
    # deterministic mode: the kernels add 64-bit fixed-point sums into a scratch, never a bias gradient (its own pass below)
    det = _DetAcc(dw.numel(), Cout if db is not None else 0, N * Do * Ho * Wo, x5 if parts is None else None, x_amax,
                  dy5, dy_amax) if _DET["on"] else None
    launch = functools.partial(_launch_conv_wgrad, kernel, g, x5, dy5, x_amax, dy_amax, dy_pmax, parts,
                               *((dw, db) if det is None else (det.dw, None)))
    if det is not None:
        try:
            launch()
            if db is not None:
                check(lib().dfmir_bias_grad(_p(dy5), _p(det.db), dy5.shape[0], Cout, Do * Ho * Wo, _st()))
        except BaseException:
            det.abort()
            raise
        det.end(dw, db)
        return dw
    prof = _CONV_PROFILER[0]
    if prof is None:
        launch()
    else:
        _call_profiler(prof, launch, *_conv_wgrad_label(kernel, g, x5, dy5, parts, getattr(prof, "accepts_issued", False)))
    return dw


def weight_pack(w, mode):
    Cout, Cin = w.shape[0], w.shape[1]
    T = w.numel() // (Cout * Cin)
    out = torch.empty(lib().dfmir_weight_pack_floats(Cout, Cin, T), device=w.device, dtype=torch.float32)
    check(lib().dfmir_weight_pack(_p(_c(w)), _p(out), Cout, Cin, T, mode, _st()))
    return out


# Packed weights are kept per (module, mode) in persistent buffers.  All weights change together (the optimizer step
# bumps the weights epoch), so the first request after a bump re-packs EVERY registered buffer whose parameter is still
# in place with one batched call (2 launches instead of ~170 per train step).
_PACKS = {"epoch": None, "entries": {}, "key": None, "descs": None, "dev": None}
def _bump_gen(buf):
    """Generation of a persistent packed-weight buffer (bumped whenever it is re-packed): keys what is derived from it."""
    buf._df_gen = getattr(buf, "_df_gen", 0) + 1
_KEEP_TABLES = []     # device job tables are never freed (a few KB each; see _repack_all / _flush_deferred)


def packed_weight(owner, w3, mode):
    """Packed form of owner's weight (w3 = the parameter viewed [Cout, Cin, T...]) for mode 0 (forward) / 1 (dgrad).
    The buffer of an (owner, mode) pair is allocated once and refreshed IN PLACE for as long as the parameter keeps its
    address and shape -- a captured hipGraph holds the buffer's address, and an in-place change of the weights through
    torch (load_state_dict, a test restoring a snapshot) must not move it."""
    import weakref
    ents = _PACKS["entries"]
    key = (id(owner), mode)
    ep = weights_epoch()
    place = (w3.data_ptr(), tuple(w3.shape), w3.device)
    ent = ents.get(key)
    if ent is not None and (ent["ref"]() is not owner or ent["place"] != place):
        ent = None
    if ent is None:
        buf = weight_pack(w3, mode)
        _bump_gen(buf)
        ents[key] = {"ref": weakref.ref(owner), "place": place, "version": w3._version, "epoch": ep, "buf": buf,
                     "w": w3.detach(), "mode": mode}
        _PACKS["key"] = None
        return buf
    if ent["version"] != w3._version:            # modified in place through torch since the last pack
        ent["version"] = w3._version
        ent["epoch"] = None
    if ent["epoch"] != ep and _PACKS["epoch"] != ep:
        _repack_all(ep)
    if ent["epoch"] == ep:
        return ent["buf"]
    # the batched pass did not cover it (it ran before this entry existed / before the in-place change): refresh
    Cout, Cin = w3.shape[0], w3.shape[1]
    check(lib().dfmir_weight_pack(_p(_c(w3)), _p(ent["buf"]), Cout, Cin, w3.numel() // (Cout * Cin), mode, _st()))
    _bump_gen(ent["buf"])
    ent["epoch"] = ep
    return ent["buf"]


def _repack_all(ep):
    import numpy as np
    ents = _PACKS["entries"]
    for k in [k for k, e in ents.items() if e["ref"]() is None]:
        del ents[k]
        _PACKS["key"] = None
    live = [e for e in ents.values() if e["place"][0] == e["w"].data_ptr() and e["w"].is_contiguous()]
    _PACKS["epoch"] = ep
    if not live:
        return
    dev = live[0]["w"].device
    live = [e for e in live if e["w"].device == dev]
    key = tuple((e["w"].data_ptr(), e["buf"].data_ptr(), e["mode"]) for e in live)
    upload = 0
    if _PACKS["key"] != key:
        tab = np.zeros((len(live), 4), dtype=np.int64)             # struct DfPackJob = 2 pointers + 4 ints
        for i, e in enumerate(live):
            Cout, Cin = int(e["w"].shape[0]), int(e["w"].shape[1])
            T = e["w"].numel() // (Cout * Cin)
            tab[i, 0], tab[i, 1] = e["w"].data_ptr(), e["buf"].data_ptr()
            tab[i, 2] = Cout | (Cin << 32)
            tab[i, 3] = T | (e["mode"] << 32)
        _PACKS["descs"] = tab
        _PACKS["dev"] = torch.empty(len(live) * 8, device=dev, dtype=torch.int64)   # 64 B per job
        _KEEP_TABLES.append(_PACKS["dev"])       # a captured hipGraph may hold the address of an earlier table
        _PACKS["key"] = key
        upload = 1
    check(lib().dfmir_weight_pack_batch(_PACKS["descs"].ctypes.data, len(live), _p(_PACKS["dev"]), upload, _st()))
    for e in live:
        e["epoch"] = ep
        e["version"] = e["w"]._version
        _bump_gen(e["buf"])
    _resplit_all_3d(dev)


def weight_unpack(g_tcc, shape):
    Cout, Cin = shape[0], shape[1]
    T = g_tcc.numel() // (Cout * Cin)
    out = torch.empty(shape, device=g_tcc.device, dtype=torch.float32)
    check(lib().dfmir_weight_unpack(_p(g_tcc), _p(out), Cout, Cin, T, _st()))
    return out


# A global "weights epoch": the fused Adam kernel updates parameters through raw pointers, which
# torch's version counters cannot see; packed-weight caches are keyed on (version, epoch).
_EPOCH = [0]


def bump_weights_epoch():
    _EPOCH[0] += 1


# Deferred weight gradients.  A train step back-propagates through the same conv modules several times
# (G once, its encoder three more times for the NCE terms).  Inside `with deferred_weight_grads():` the
# wgrad kernels of all those passes accumulate into ONE persistent tap-major buffer per module and the
# bias gradients straight into `bias.grad`; the buffers are unpacked into `weight.grad` once, on exit.
# Without it every pass pays a zero-fill, an unpack and an autograd `add` per parameter (~900 tiny launches).
_DEFER = {"on": False, "pending": {}}


class deferred_weight_grads:
    def __enter__(self):
        _DEFER["on"] = True
        return self

    def __exit__(self, *exc):
        _DEFER["on"] = False
        pending, _DEFER["pending"] = _DEFER["pending"], {}
        if exc[0] is None and pending:
            _flush_deferred(list(pending.values()))
        elif pending:
            # backward raised: the accumulators hold partial sums that only the flush kernel would clear; a caller
            # that catches the error and goes on (skip-batch / OOM-retry loops) must not inherit them
            for _, buf, _ in pending.values():
                zero_(buf)
        return False


def begin_deferred():
    """deferred_weight_grads as two calls, for a backward that runs in several pieces (registration_model's staged step:
    the pieces are separate autograd calls on two streams, captured into separate hipGraphs): begin_deferred() before the
    first piece, end_deferred() -- the one flush -- after the last, on a stream that has waited for all of them."""
    _DEFER["on"] = True


def end_deferred(failed=False):
    _DEFER["on"] = False
    pending, _DEFER["pending"] = _DEFER["pending"], {}
    if not pending:
        return
    if failed:
        for _, buf, _ in pending.values():
            zero_(buf)
    else:
        _flush_deferred(list(pending.values()))


_JOBS = {"key": None, "dev": None, "max": 0}
_JOBS_BY_GROUP = {"all": _JOBS}


def flush_deferred_subset(owner_ids, group):
    """Flush NOW the deferred accumulators of the modules in `owner_ids` (ids) whose weight gradients are final -- a
    gradient bucket that leaves for its all-reduce before backward has finished (registration_model._bucket_ready).
    `group` names the job table (one device table per group: a captured step holds it by address)."""
    pend = _DEFER["pending"]
    items = [pend.pop(i) for i in list(pend.keys()) if i in owner_ids]
    if items:
        _flush_deferred(items, group)
    return len(items)


def _flush_deferred(items, group="all"):
    """grad += unpack(accumulator); accumulator = 0 for every deferred conv, one launch (the job table is uploaded
    once and reused while the same buffers come back, i.e. every step after the first)."""
    import numpy as np
    _JOBS = _JOBS_BY_GROUP.setdefault(group, {"key": None, "dev": None, "max": 0})
    key = tuple((buf.data_ptr(), owner.weight.grad.data_ptr(), tuple(shape)) for owner, buf, shape in items)
    if _JOBS["key"] != key:
        tab = np.zeros((len(items), 4), dtype=np.int64)            # struct DfUnpackJob = 2 pointers + 4 ints
        mx = 0
        for i, (owner, buf, shape) in enumerate(items):
            Cout, Cin = int(shape[0]), int(shape[1])
            T = buf.numel() // (Cout * Cin)
            tab[i, 0], tab[i, 1] = buf.data_ptr(), owner.weight.grad.data_ptr()
            tab[i, 2] = Cout | (Cin << 32)
            tab[i, 3] = T
            mx = max(mx, Cout * Cin * T)
        _JOBS["dev"] = torch.from_numpy(tab).to(items[0][1].device)
        _KEEP_TABLES.append(_JOBS["dev"])
        _JOBS["key"], _JOBS["max"] = key, mx
    check(lib().dfmir_weight_unpack_add_batch(_p(_JOBS["dev"]), len(items), _JOBS["max"], _st()))


def _deferred_buffer(owner, T, Cin, Cout, shape, device):
    buf = getattr(owner, "_dw_tcc", None)
    if buf is None or buf.shape != (T, Cin, Cout) or buf.device != device:
        buf = zeros((T, Cin, Cout), device)
        owner._dw_tcc = buf
    _DEFER["pending"][id(owner)] = (owner, buf, shape)
    return buf


def weights_epoch():
    return _EPOCH[0]


# ------------------------------------------------------------------------------------------------
# convolution
# ------------------------------------------------------------------------------------------------
class ConvFn(Function):
    """y = act(conv(x, w) + b).  `owner` supplies cached packed weights (owner.packed(mode))."""

    @staticmethod
    def forward(ctx, x, weight, bias, owner, stride, pad, pad_mode, act, slope, skip=False):
        # skip=True (reflect-padded stride-1 convs): also return x itself as a second output for a residual
        # branch, so that backward receives that branch's gradient and sums it inside the halo-fold kernel
        # (ResnetBlock: out = x + conv_block(x), models/networks.py:1219-1221) instead of autograd's add kernel.
        _need(x, weight, bias)
        nd = x.dim() - 2
        x5 = _c(x) if nd == 3 else _c(x).unsqueeze(2)
        K = tuple(weight.shape[2:]) if nd == 3 else (1,) + tuple(weight.shape[2:])
        p3 = (pad,) * 3 if nd == 3 else (0, pad, pad)
        sp = x5.shape[2:]
        out_sp = tuple((sp[i] + 2 * p3[i] - K[i]) // stride + 1 for i in range(3))
        w_tcc = owner.packed(0) if owner is not None else weight_pack(weight, 0)
        x_amax = None
        if _wants_amax(K, stride, 1, x5.shape[2], x5.shape[1], weight.shape[0]):
            x_amax = amax_of(x) if x.is_contiguous() else absmax(x5)
        y5 = conv_raw(x5, w_tcc, bias, weight.shape[0], K, stride, p3, 1, pad_mode, act, slope, out_sp, x_amax)
        ctx.x_amax = x_amax
        # trailing input channels that need no gradient (cat([up2(a), b]) with b = the network's input images)
        ctx.dead_tail = int(getattr(x, "_df_nograd_tail", 0))
        # x = the output of a LeakyReLU ConvBlock that feeds nothing but this conv (declared by the caller, conv(sole=True)):
        # this conv's dgrad can then return the gradient w.r.t. that block's PRE-activation (see backward)
        ta = getattr(x, "_df_act_sole", None)
        ctx.in_act = (ta[0], ta[1]) if (_tag_ok(x, ta) and x.is_contiguous() and not _NO_ACTGRAD) else None
        ctx.cfg = (nd, K, stride, p3, pad_mode, act, slope, owner)
        ctx.save_for_backward(x5, weight, y5 if act else None)
        ctx.has_bias = bias is not None
        ctx.skip = bool(skip)
        y = y5 if nd == 3 else y5.squeeze(2)
        if skip:
            if not (stride == 1 and pad_mode == 1 and x.is_contiguous()):
                raise DfmirHipError("conv(skip=True) is the reflect-padded stride-1 case on a contiguous input")
            ctx.set_materialize_grads(False)
            return y, x.view_as(x)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy, dskip=None):
        if dy is None:              # only the skip output was used downstream
            return (dskip,) + (None,) * 9
        x5, weight, y5 = ctx.saved_tensors
        dx, dw, db = _conv_backward_impl(ctx, dy, dskip, x5, weight, y5)
        return dx, dw, db, None, None, None, None, None, None, None


def _conv_backward_impl(ctx, dy, dskip, x5, weight, y5):
    """Backward of y = act(conv(x5, weight) + bias) for a ctx-like object carrying cfg, x_amax, dead_tail, in_act,
    has_bias, needs_input_grad (x, weight, bias); returns (dx, dw, db).  Shared by ConvFn and UpCatConv3dFn."""
    nd, K, stride, p3, pad_mode, act, slope, owner = ctx.cfg
    dy5 = _c(dy) if nd == 3 else _c(dy).unsqueeze(2)
    Cout, Cin = weight.shape[0], weight.shape[1]
    want_probe = _wants_amax(K, stride, 1, dy5.shape[2], Cout, Cin) or ctx.x_amax is not None
    dy_amax = None
    if act and _tag_ok(dy, getattr(dy, "_df_premasked", None)) and dy.is_contiguous():
        pass      # the producing dgrad already multiplied by this activation's derivative (and left the range probe)
    elif act:
        dpre = torch.empty_like(dy5)
        if want_probe and nd == 3 and not ((dy5.data_ptr() | y5.data_ptr() | dpre.data_ptr()) & 15):
            # the activation's backward leaves the range probe of what it writes (3-D tensors are 0.1-1 GB: a
            # separate absmax pass would cost 10 % of the dgrad it serves)
            dy_amax = amax_slot(dy5.device, PROBE_SLOTS)
            check(lib().dfmir_act_bwd_amax(_p(dy5), _p(y5), _p(dpre), dy5.numel(), act, float(slope), _p(dy_amax), _st()))
        else:
            check(lib().dfmir_act_bwd(_p(dy5), _p(y5), _p(dpre), dy5.numel(), act, float(slope), _st()))
        dy5 = dpre
    dx = dw = db = None
    # dY feeds the dgrad conv (as its input) and the wgrad: one range probe for both
    if want_probe and dy_amax is None:
        dy_amax = amax_of(dy) if (dy.is_contiguous() and (not act or dy5.data_ptr() == dy.data_ptr())) else absmax(dy5)
    _LAST_BWD_PAIRED[0] = False
    both = _conv_backward_pair(ctx, dy, dskip, dy5, dy_amax, x5, weight)
    if both is not None:
        return both
    if ctx.needs_input_grad[0]:
        wd = owner.packed(1) if owner is not None else weight_pack(weight, 1)
        in_sp = tuple(x5.shape[2:])
        gf = None
        if stride == 1 and pad_mode == 1 and dy_amax is not None:
            gf = DfConvGeom(x5.shape[0], Cin, Cout, 1, in_sp[1], in_sp[2], 1, in_sp[1], in_sp[2], K[0], K[1], K[2],
                            1, 1, p3[0], p3[1], p3[2], 1, 0, 0.0)
            gd = DfConvGeom(x5.shape[0], Cout, Cin, 1, in_sp[1], in_sp[2], 1, in_sp[1], in_sp[2], K[0], K[1], K[2],
                            1, 1, p3[0], p3[1], p3[2], 0, 0, 0.0)      # the zero-padded dgrad as a conv
            if not (lib().dfmir_conv3x3_reflect_ring_ok(ctypes.byref(gf))
                    and lib().dfmir_conv3x3_res_ok(ctypes.byref(gd))):
                gf = None
        if gf is not None:
            # the one-pixel ring of the padded frame first (four 1-D convolutions of dY's border lines, into a
            # compact buffer), then the frame's interior = the zero-padded "same" dgrad on full tiles, whose
            # epilogue folds the ring (and the skip branch's gradient) in   (csrc/conv3x3s.hip)
            rl = lib().dfmir_conv3x3_reflect_ring_len(ctypes.byref(gf))
            ringbuf = torch.empty(x5.shape[0] * 4 * Cin * rl, device=dy5.device, dtype=torch.float32)
            ctag = getattr(dy, "_df_cols", None)
            cols = ctag[0] if (ctag is not None and ctag[1] == dy._version and ctag[2] == dy.data_ptr()
                               and dy.is_contiguous() and not act) else None
            check(lib().dfmir_conv3x3_reflect_ring(ctypes.byref(gf), _p(dy5), _p(cols), _p(dy_amax), dy_amax.numel(),
                                                   _p(wd), _p(ringbuf), _st()))
            res5 = None
            if dskip is not None:
                res5 = _c(dskip) if nd == 3 else _c(dskip).unsqueeze(2)
                dskip = None
            dx5 = conv_raw(dy5, wd, None, Cin, K, 1, p3, 1, 0, 0, 0.0, in_sp, dy_amax, res=res5, ring=(ringbuf, rl))
        elif stride == 1 and pad_mode == 1:
            # full correlation onto the reflect-padded frame, then fold the halo back
            padp = tuple(K[i] - 1 for i in range(3))
            out_sp = tuple(in_sp[i] + 2 * p3[i] for i in range(3))
            dxp = conv_raw(dy5, wd, None, Cin, K, 1, padp, 1, 0, 0, 0.0, out_sp, dy_amax)
            if p3[0] != 0 or p3[1] != p3[2]:
                raise DfmirHipError("reflect padding is 2-D, symmetric only")
            dx5 = torch.empty_like(x5)
            if dskip is not None:
                check(lib().dfmir_reflect_pad2d_bwd_add(_p(dxp), _p(_c(dskip)), _p(dx5), x5.shape[0] * Cin,
                                                        in_sp[1], in_sp[2], p3[1], _st()))
                dskip = None
            else:
                check(lib().dfmir_reflect_pad2d_bwd(_p(dxp), _p(dx5), x5.shape[0] * Cin, in_sp[1], in_sp[2],
                                                    p3[1], _st()))
        else:
            padp = tuple(K[i] - 1 - p3[i] for i in range(3))
            used = Cin - ctx.dead_tail if (ctx.dead_tail and stride == 1) else None
            ia = ctx.in_act if (stride == 1 and nd == 3) else None
            dx5 = conv_raw(dy5, wd, None, Cin, K, 1, padp, stride, 0, 0, 0.0, in_sp, dy_amax, cout_used=used,
                           act_src=x5 if ia else None, act_slope=ia[1] if ia else 0.0)
            if ia and _LAST_ACTGRAD[0]:
                dx5._df_premasked = (dx5._version, dx5.data_ptr())
        dx = dx5 if nd == 3 else dx5.squeeze(2)
    if dskip is not None:       # not folded in above (x needs no conv-path gradient, or non-reflect dgrad)
        dx = dskip if dx is None else dx + dskip
    defer = (_DEFER["on"] and owner is not None and getattr(owner, "weight", None) is not None
             and owner.weight.grad is not None and owner.weight.grad.is_contiguous())
    # bias gradient target: straight into bias.grad when deferring, else a fresh buffer (returned to autograd);
    # it rides along with the wgrad call (which reads dY anyway) when there is one
    db_buf = None
    if ctx.has_bias and ctx.needs_input_grad[2]:
        bg = getattr(owner, "bias", None).grad if defer and getattr(owner, "bias", None) is not None else None
        if bg is not None and bg.is_contiguous():
            db_buf = bg
        else:
            db = db_buf = zeros(Cout, dy5.device)
    if ctx.needs_input_grad[1]:
        ptag = getattr(dy, "_df_pmax", None) if not act else None     # per-plane maxima of dY (InstanceNorm backward)
        dy_pmax = ptag[0] if (ptag is not None and ptag[1] == dy._version and ptag[2] == dy.data_ptr()
                              and dy.is_contiguous() and not _NO_CH_SCALE) else None
        parts = getattr(ctx, "x_parts", None)
        if defer:
            T = K[0] * K[1] * K[2]
            conv_wgrad_raw(x5, dy5, K, stride, p3, pad_mode,
                           out=_deferred_buffer(owner, T, Cin, Cout, tuple(weight.shape), dy5.device),
                           x_amax=ctx.x_amax, dy_amax=dy_amax, db=db_buf, dy_pmax=dy_pmax, parts=parts)
        else:
            dwt = conv_wgrad_raw(x5, dy5, K, stride, p3, pad_mode, x_amax=ctx.x_amax, dy_amax=dy_amax, db=db_buf,
                                 dy_pmax=dy_pmax, parts=parts)
            dw = weight_unpack(dwt, tuple(weight.shape))
    elif db_buf is not None:
        bias_grad(dy5, db_buf)                                                           # accumulates
    return dx, dw, db


_LAST_BWD_PAIRED = [False]


def last_backward_paired():
    """Did the LAST conv backward issue its data gradient and its weight gradient as one launch (dfmir_conv3x3_bwd_pair)?"""
    return _LAST_BWD_PAIRED[0]


def _plan_conv_bwd_pair(gd, gw, K, res, ring):
    """Does the backward of the 2-D 3x3 layer gw (gd = its data gradient as a convolution of dY) go out as ONE launch?  Pure,
    like the two planners it asks: both must leave the layer to the library's own 2-D dispatch (with the residual, if any,
    in the epilogue), the library must say that this dispatch ends on the kernels the pair kernel carries, weight gradients
    must not be in deterministic mode, and no conv profiler may be installed -- bench.py --full keeps timing the two kernels
    per kind.  (The probe audit reads each operand between the launches: separate, too.)"""
    if _CONV_PROFILER[0] is not None or _DET["on"] or _PROBE_AUDIT["on"]:
        return False
    fwd = _plan_conv_fwd(gd, K, True, res, ring, None, True, None)
    if fwd.kernel not in ("res2d", "generic") or (res is not None and not fwd.fuse_res):
        return False
    if _plan_conv_wgrad(gw, K, True, None) != "generic":
        return False
    return bool(lib().dfmir_conv3x3_bwd_pair_ok(ctypes.byref(gd), ctypes.byref(gw)))


def _conv_backward_pair(ctx, dy, dskip, dy5, dy_amax, x5, weight):
    """The dgrad + wgrad part of _conv_backward_impl as one launch where _plan_conv_bwd_pair allows it: (dx, dw, db), or
    None -- nothing launched -- when the backward goes the two-launch way.  dy5 = the gradient w.r.t. the pre-activation."""
    nd, K, stride, p3, pad_mode, act, _, owner = ctx.cfg
    if not (nd == 2 and tuple(K) == (1, 3, 3) and stride == 1 and tuple(p3) == (0, 1, 1) and ctx.needs_input_grad[0]
            and ctx.needs_input_grad[1] and ctx.x_amax is not None and dy_amax is not None
            and getattr(ctx, "x_parts", None) is None and not ctx.dead_tail):
        return None
    if pad_mode == 0 and dskip is not None:
        return None
    L = lib()
    Cout, Cin = weight.shape[0], weight.shape[1]
    N, H, W = x5.shape[0], x5.shape[3], x5.shape[4]
    gw = DfConvGeom(N, Cin, Cout, 1, H, W, 1, H, W, 1, 3, 3, 1, 1, 0, 1, 1, pad_mode, 0, 0.0)
    gd = DfConvGeom(N, Cout, Cin, 1, H, W, 1, H, W, 1, 3, 3, 1, 1, 0, 1, 1, 0, 0, 0.0)   # the zero-padded dgrad as a conv
    res5 = None
    if pad_mode == 1:       # reflect: the ring of the padded frame by its own kernel, folded in by the dgrad's epilogue
        if not (L.dfmir_conv3x3_reflect_ring_ok(ctypes.byref(gw)) and L.dfmir_conv3x3_res_ok(ctypes.byref(gd))):
            return None
        if dskip is not None:
            res5 = _c(dskip).unsqueeze(2)
    if not _plan_conv_bwd_pair(gd, gw, K, res5, (None, 0) if pad_mode == 1 else None):
        return None
    wd = owner.packed(1) if owner is not None else weight_pack(weight, 1)
    ringbuf, rl = None, 0
    if pad_mode == 1:
        rl = L.dfmir_conv3x3_reflect_ring_len(ctypes.byref(gw))
        ringbuf = torch.empty(N * 4 * Cin * rl, device=dy5.device, dtype=torch.float32)
        ctag = getattr(dy, "_df_cols", None)
        cols = ctag[0] if (ctag is not None and ctag[1] == dy._version and ctag[2] == dy.data_ptr()
                           and dy.is_contiguous() and not act) else None
        check(L.dfmir_conv3x3_reflect_ring(ctypes.byref(gw), _p(dy5), _p(cols), _p(dy_amax), dy_amax.numel(), _p(wd),
                                           _p(ringbuf), _st()))
    # the weight / bias gradient targets, as in _conv_backward_impl
    defer = (_DEFER["on"] and owner is not None and getattr(owner, "weight", None) is not None
             and owner.weight.grad is not None and owner.weight.grad.is_contiguous())
    db = db_buf = None
    if ctx.has_bias and ctx.needs_input_grad[2]:
        bg = getattr(owner, "bias", None).grad if defer and getattr(owner, "bias", None) is not None else None
        if bg is not None and bg.is_contiguous():
            db_buf = bg
        else:
            db = db_buf = zeros(Cout, dy5.device)
    ptag = getattr(dy, "_df_pmax", None) if not act else None
    pm = ptag[0] if (ptag is not None and ptag[1] == dy._version and ptag[2] == dy.data_ptr() and dy.is_contiguous()
                     and not _NO_CH_SCALE and ptag[0].numel() == N * Cout) else None
    dwt = (_deferred_buffer(owner, 9, Cin, Cout, tuple(weight.shape), dy5.device) if defer
           else zeros((9, Cin, Cout), dy5.device))
    dx5 = torch.empty((N, Cin, 1, H, W), device=dy5.device, dtype=torch.float32)
    paired = ctypes.c_int(0)
    check(L.dfmir_conv3x3_bwd_pair(ctypes.byref(gd), ctypes.byref(gw), _p(dy5), _p(dy_amax), dy_amax.numel(), _p(pm), _p(wd),
                                   _p(res5), _p(ringbuf), rl, _p(dx5), _p(x5), _p(ctx.x_amax), ctx.x_amax.numel(), _p(dwt),
                                   _p(db_buf), ctypes.byref(paired), _st()))
    _LAST_BWD_PAIRED[0] = bool(paired.value)
    _LAST_ACTGRAD[0] = False
    return dx5.squeeze(2), (None if defer else weight_unpack(dwt, tuple(weight.shape))), db


_LAST_CONV_AMAX = [None]


def conv(x, weight, bias=None, owner=None, stride=1, pad=0, pad_mode=0, act=0, slope=0.0, skip=False, sole=False):
    """sole=True: the caller guarantees that the returned tensor feeds exactly ONE consumer (the next conv of a chain);
    with a LeakyReLU epilogue that consumer's dgrad may then fold this activation's backward into its own epilogue."""
    _LAST_CONV_AMAX[0] = None
    out = ConvFn.apply(x, weight, bias, owner, stride, pad, pad_mode, act, slope, skip)
    if _LAST_CONV_AMAX[0] is not None and not skip:
        tag_amax(out, _LAST_CONV_AMAX[0])
        _LAST_CONV_AMAX[0] = None
    if sole and act == 1 and not skip and x.dim() == 5:
        out._df_act_sole = (act, float(slope), out._version, out.data_ptr())
    return out


# ------------------------------------------------------------------------------------------------
# 7x7 convolutions as tap-stack / tap-sum + 1x1 GEMM
# ------------------------------------------------------------------------------------------------
class TapStackFn(Function):
    """x [N,C,H,W] -> S [N, C*K*K, H, W],  S[c*T+tap][p] = x[c][map(p + tap - pad)]."""

    @staticmethod
    def forward(ctx, x, K, pad, pad_mode):
        _need(x)
        x = _c(x)
        N, C, H, W = x.shape
        s = torch.empty((N, C * K * K, H, W), device=x.device, dtype=torch.float32)
        check(lib().dfmir_tapstack_fwd(_p(x), _p(s), N, C, H, W, K, pad, pad_mode, _st()))
        ctx.meta = (N, C, H, W, K, pad, pad_mode)
        return s

    @staticmethod
    @once_differentiable
    def backward(ctx, ds):
        N, C, H, W, K, pad, pad_mode = ctx.meta
        ds = _c(ds)
        dx = torch.empty((N, C, H, W), device=ds.device, dtype=torch.float32)
        check(lib().dfmir_tapstack_bwd(_p(ds), _p(dx), N, C, H, W, K, pad, pad_mode, _st()))
        return dx, None, None, None


class TapSumFn(Function):
    """Z [N, C*K*K, H, W] -> y [N,C,H,W] = act(bias + sum_tap Z[c*T+tap][map(p + tap - pad)])."""

    @staticmethod
    def forward(ctx, z, bias, C, K, pad, pad_mode, act, slope):
        _need(z, bias)
        z = _c(z)
        N, CT, H, W = z.shape
        y = torch.empty((N, C, H, W), device=z.device, dtype=torch.float32)
        check(lib().dfmir_tapsum_fwd(_p(z), _p(bias), _p(y), N, C, H, W, H, W, K, pad, pad_mode, act, float(slope), _st()))
        ctx.meta = (N, C, H, W, K, pad, pad_mode, act, float(slope))
        ctx.save_for_backward(y if act else None)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        N, C, H, W, K, pad, pad_mode, act, slope = ctx.meta
        (y,) = ctx.saved_tensors
        dy = _c(dy)
        if act:
            dpre = torch.empty_like(dy)
            check(lib().dfmir_act_bwd(_p(dy), _p(y), _p(dpre), dy.numel(), act, slope, _st()))
            dy = dpre
        dz = db = None
        if ctx.needs_input_grad[0]:
            dz = torch.empty((N, C * K * K, H, W), device=dy.device, dtype=torch.float32)
            check(lib().dfmir_tapsum_bwd(_p(dy), _p(dz), N, C, H, W, H, W, K, pad, pad_mode, _st()))
        if ctx.has_bias and ctx.needs_input_grad[1]:
            db = zeros(C, dy.device)
            bias_grad(dy.view(N, C, H * W), db)
        return dz, db, None, None, None, None, None, None


class Stem7Fn(Function):
    """7x7 conv of a single-channel image (Cout <= 64, pad 3) straight from the image (csrc/taps.hip), not through
    the 49-plane tap stack.  Backward: dW, db by the direct kernel; dx (only when the image needs a gradient) through
    the tap-stack adjoint."""

    @staticmethod
    def forward(ctx, x, weight, bias, pad_mode):
        _need(x, weight, bias)
        x = _c(x)
        N, _, H, W = x.shape
        Cout = weight.shape[0]
        y = torch.empty((N, Cout, H, W), device=x.device, dtype=torch.float32)
        check(lib().dfmir_conv7x7_c1_fwd(_p(x), _p(_c(weight)), _p(bias), _p(y), N, H, W, Cout, pad_mode, _st()))
        ctx.save_for_backward(x, weight)
        ctx.pad_mode = pad_mode
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = _c(dy)
        N, _, H, W = x.shape
        Cout = weight.shape[0]
        dx = dw = db = None
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dwb = zeros(Cout * 49 + Cout, dy.device)
            dbp = dwb[Cout * 49:] if ctx.has_bias else None
            if _DET["on"]:
                det = _DetAcc(Cout * 49, Cout if ctx.has_bias else 0, N * H * W, x, None, dy, None)
                try:
                    check(lib().dfmir_conv7x7_c1_wgrad(_p(x), _p(dy), _p(det.dw), None, N, H, W, Cout, ctx.pad_mode, _st()))
                    if ctx.has_bias:
                        check(lib().dfmir_bias_grad(_p(dy), _p(det.db), N, Cout, H * W, _st()))
                except BaseException:
                    det.abort()
                    raise
                det.end(dwb, dbp)
            else:
                check(lib().dfmir_conv7x7_c1_wgrad(_p(x), _p(dy), _p(dwb), _p(dbp), N, H, W, Cout, ctx.pad_mode, _st()))
            dw = dwb[:Cout * 49].view(Cout, 1, 7, 7)
            db = dbp if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        if ctx.needs_input_grad[0]:
            wd = weight_pack(weight.detach().view(Cout, 49, 1), 1)
            ds = conv_raw(dy.unsqueeze(2), wd, None, 49, (1, 1, 1), 1, (0, 0, 0), 1, 0, 0, 0.0, (1, H, W))
            dx = torch.empty_like(x)
            check(lib().dfmir_tapstack_bwd(_p(ds), _p(dx), N, 1, H, W, 7, 3, ctx.pad_mode, _st()))
        return dx, dw, db, None


def conv_taps(x, weight, bias, pad, pad_mode, act=0, slope=0.0):
    """KxK conv with Cin == 1 or Cout <= 4 as a 1x1 GEMM over K*K tap planes (see csrc/taps.hip)."""
    Cout, Cin, K = weight.shape[0], weight.shape[1], weight.shape[2]
    T = K * K
    if Cin == 1 and K == 7 and pad == 3 and Cout <= 64 and act == 0 and x.dim() == 4:
        return Stem7Fn.apply(x, weight, bias, pad_mode)
    if Cin == 1:
        s = TapStackFn.apply(x, K, pad, pad_mode)
        return conv(s, weight.view(Cout, T, 1, 1), bias, None, 1, 0, 0, act, slope)
    wz = weight.view(Cout, Cin, T).permute(0, 2, 1).reshape(Cout * T, Cin, 1, 1)   # [c*T+tap][ci]
    z = conv(x, wz, None, None, 1, 0, 0, 0, 0.0)
    return TapSumFn.apply(z, bias, Cout, K, pad, pad_mode, act, slope)


# ------------------------------------------------------------------------------------------------
# InstanceNorm (+ReLU, +residual)
# ------------------------------------------------------------------------------------------------
class InstNormFn(Function):
    @staticmethod
    def forward(ctx, x, res, relu, eps):
        _need(x, res)
        x = _c(x)
        planes = x.shape[0] * x.shape[1]
        S = x.numel() // planes
        y = torch.empty_like(x)
        mean = torch.empty(planes, device=x.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        r = _c(res) if res is not None else None
        slot = amax_slot(x.device, PROBE_SLOTS)
        check(lib().dfmir_instnorm_fwd(_p(x), _p(r), _p(y), _p(mean), _p(rstd), planes, S, float(eps),
                                       int(relu), _p(slot), _st()))
        _LAST_AMAX[0] = slot
        ctx.save_for_backward(x, mean, rstd)
        ctx.relu = int(relu)
        ctx.has_res = res is not None
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, mean, rstd = ctx.saved_tensors
        dy = _c(dy)
        planes = x.shape[0] * x.shape[1]
        S = x.numel() // planes
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            slot = amax_slot(x.device, PROBE_SLOTS)
            W = x.shape[-1]
            want_cols = x.dim() == 4 and W <= 94 and S // W <= 94 and lib().dfmir_instnorm_bwd_cols_ok(S, W)   # ring-kernel sizes
            # first / last column of dx on the side: the dgrad of a reflect-padded conv reads them (ring kernel)
            cols = torch.empty(planes * 2 * (S // W), device=x.device, dtype=torch.float32) if want_cols else None
            if x.dim() == 4 and lib().dfmir_instnorm_bwd_pmax_ok(S):
                # + the maximum of every (n, c) plane: per-output-channel dY scales for the split weight gradient
                pmax = torch.empty(planes, device=x.device, dtype=torch.float32)
                check(lib().dfmir_instnorm_bwd_pmax(_p(dy), _p(x), _p(mean), _p(rstd), _p(dx), planes, S, ctx.relu,
                                                    _p(slot), _p(cols), W if want_cols else 0, _p(pmax), _st()))
                dx._df_pmax = (pmax, dx._version, dx.data_ptr())
            elif want_cols:
                check(lib().dfmir_instnorm_bwd_cols(_p(dy), _p(x), _p(mean), _p(rstd), _p(dx), planes, S, ctx.relu,
                                                    _p(slot), _p(cols), W, _st()))
            else:
                check(lib().dfmir_instnorm_bwd(_p(dy), _p(x), _p(mean), _p(rstd), _p(dx), planes, S, ctx.relu,
                                               _p(slot), _st()))
            if want_cols:
                dx._df_cols = (cols, dx._version, dx.data_ptr())
            tag_amax(dx, slot)
        dres = dy if (ctx.has_res and ctx.needs_input_grad[1]) else None
        return dx, dres, None, None


_LAST_AMAX = [None]


def instance_norm(x, res=None, relu=False, eps=1e-5):
    y = InstNormFn.apply(x, res, relu, eps)
    return tag_amax(y, _LAST_AMAX[0])


class InstNormReluBlurDownFn(Function):
    """Downsample(ReLU(InstanceNorm2d(x))) in one pass per plane (csrc/norm_resample.hip in_relu_blurdown_*): the
    full-resolution normalised tensor is never written -- it feeds only the blur and no backward needs it."""

    @staticmethod
    def forward(ctx, x, eps):
        _need(x)
        x = _c(x)
        N, C, H, W = x.shape
        planes = N * C
        z = torch.empty((N, C, H // 2, W // 2), device=x.device, dtype=torch.float32)
        mean = torch.empty(planes, device=x.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        slot = amax_slot(x.device, PROBE_SLOTS)
        check(lib().dfmir_in_relu_blurdown_fwd(_p(x), _p(z), _p(mean), _p(rstd), planes, H, W, float(eps), _p(slot), _st()))
        _LAST_AMAX[0] = slot
        ctx.save_for_backward(x, mean, rstd)
        return z

    @staticmethod
    @once_differentiable
    def backward(ctx, dz):
        x, mean, rstd = ctx.saved_tensors
        dz = _c(dz)
        N, C, H, W = x.shape
        dx = torch.empty_like(x)
        slot = amax_slot(x.device, PROBE_SLOTS)
        pmax = torch.empty(N * C, device=x.device, dtype=torch.float32)
        check(lib().dfmir_in_relu_blurdown_bwd(_p(dz), _p(x), _p(mean), _p(rstd), _p(dx), N * C, H, W, _p(slot), _p(pmax),
                                               _st()))
        dx._df_pmax = (pmax, dx._version, dx.data_ptr())
        tag_amax(dx, slot)
        return dx, None


def in_relu_blurdown_ok(x):
    return (x.dim() == 4 and x.is_cuda and x.dtype == torch.float32
            and bool(lib().dfmir_in_relu_blurdown_ok(int(x.shape[2]), int(x.shape[3]))))


def instance_norm_relu_blur_down(x, eps=1e-5):
    z = InstNormReluBlurDownFn.apply(x, eps)
    return tag_amax(z, _LAST_AMAX[0])


# ------------------------------------------------------------------------------------------------
# plane-wise resampling
# ------------------------------------------------------------------------------------------------
def _plane_op(fwd_name, bwd_name, out_hw):
    class _Fn(Function):
        @staticmethod
        def forward(ctx, x, *extra):
            _need(x)
            x = _c(x)
            N, C, H, W = x.shape
            Ho, Wo = out_hw(H, W, *extra)
            y = torch.empty((N, C, Ho, Wo), device=x.device, dtype=torch.float32)
            check(getattr(lib(), fwd_name)(_p(x), _p(y), N * C, H, W, *extra, _st()))
            ctx.shape = (N, C, H, W)
            ctx.extra = extra
            return y

        @staticmethod
        @once_differentiable
        def backward(ctx, dy):
            N, C, H, W = ctx.shape
            dy = _c(dy)
            dx = torch.empty((N, C, H, W), device=dy.device, dtype=torch.float32)
            check(getattr(lib(), bwd_name)(_p(dy), _p(dx), N * C, H, W, *ctx.extra, _st()))
            return (dx,) + (None,) * len(ctx.extra)

    _Fn.__name__ = fwd_name
    return _Fn


BlurDownFn = _plane_op("dfmir_blur_down_fwd", "dfmir_blur_down_bwd",
                       lambda H, W: ((H - 1) // 2 + 1, (W - 1) // 2 + 1))
BlurUpFn = _plane_op("dfmir_blur_up_fwd", "dfmir_blur_up_bwd", lambda H, W: (2 * H, 2 * W))
ReflectPadFn = _plane_op("dfmir_reflect_pad2d_fwd", "dfmir_reflect_pad2d_bwd",
                         lambda H, W, p: (H + 2 * p, W + 2 * p))


def _bound_from(y, x):
    """y is a convex combination of x's values (the [1,2,1] blurs: non-negative taps summing to 1 per output), so
    max|x| bounds max|y|: x's range probe serves y's split conversion (no standalone absmax launch)."""
    tag = getattr(x, "_df_amax", None)
    if tag is not None and _amax_ok(x, tag):
        tag_amax(y, tag[0])
    return y


def blur_down(x):
    return _bound_from(BlurDownFn.apply(x), x)


def blur_up(x):
    return _bound_from(BlurUpFn.apply(x), x)


def reflect_pad2d(x, p):
    return ReflectPadFn.apply(x, int(p))


class UpCatFn(Function):
    """cat([nearest_up2(a), b], dim=1)  (torchvoxelmorph/networks.py:97-100)."""

    @staticmethod
    def forward(ctx, a, b):
        _need(a, b)
        a, b = _c(a), _c(b)
        nd = a.dim() - 2
        N, Ca = a.shape[0], a.shape[1]
        Cb = b.shape[1]
        Da, Ha, Wa = (a.shape[2:] if nd == 3 else (1,) + tuple(a.shape[2:]))
        sd = 2 if nd == 3 else 1
        exp = (Da * sd, Ha * 2, Wa * 2) if nd == 3 else (Ha * 2, Wa * 2)
        if tuple(b.shape[2:]) != tuple(exp):
            raise DfmirHipError("upcat: skip tensor %s does not match upsampled %s" % (tuple(b.shape), exp))
        y = torch.empty((N, Ca + Cb) + tuple(b.shape[2:]), device=a.device, dtype=torch.float32)
        check(lib().dfmir_upcat_fwd(_p(a), _p(b), _p(y), N, Ca, Cb, Da, Ha, Wa, sd, _st()))
        ctx.meta = (a.shape, b.shape, N, Ca, Cb, Da, Ha, Wa, sd)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        ash, bsh, N, Ca, Cb, Da, Ha, Wa, sd = ctx.meta
        dy = _c(dy)
        da = torch.empty(ash, device=dy.device, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        db = torch.empty(bsh, device=dy.device, dtype=torch.float32) if ctx.needs_input_grad[1] else None
        if da is not None or db is not None:   # (the skip part of dy may be unwritten when it needs no gradient)
            check(lib().dfmir_upcat_bwd(_p(dy), _p(da), _p(db), N, Ca, Cb, Da, Ha, Wa, sd, _st()))
        return da, db


def _valid_amax(t):
    tag = getattr(t, "_df_amax", None)
    if tag is not None and _amax_ok(t, tag) and tag[0].numel() == PROBE_SLOTS:
        return tag[0]
    return None


def _probe64(t):
    """A PROBE_SLOTS-wide range probe of t by a standalone pass (slot 0 = max |t|, the rest stay 0); tags t."""
    slot = amax_slot(t.device, PROBE_SLOTS)
    tc = _c(t)
    check(lib().dfmir_absmax(_p(tc), tc.numel(), _p(slot), _st()))
    if tc.data_ptr() == t.data_ptr():
        tag_amax(t, slot)
    return slot


def upcat(a, b):
    y = UpCatFn.apply(a, b)
    if torch.is_grad_enabled() and a.requires_grad and not b.requires_grad:
        y._df_nograd_tail = int(b.shape[1])    # the consumer conv's dgrad skips these channels (ConvFn)
    pa, pb = _valid_amax(a), _valid_amax(b)
    if a.dim() == 5 and not _NO_SPLIT3D:
        # 3-D: the consumer is a split conv that needs the range of y.  A part without a probe (skip tensors made by the
        # stride-2 convs, the 2-channel input) is measured on its own: 1/17 .. 1/3 of a pass over the concatenation
        pa = _probe64(a) if pa is None else pa
        pb = _probe64(b) if pb is None else pb
    if pa is not None and pb is not None:      # nearest up-sampling + concatenation create no new values
        slot = amax_slot(y.device, PROBE_SLOTS)
        check(lib().dfmir_probe_merge(_p(pa), _p(pb), _p(slot), _st()))
        tag_amax(y, slot)
    return y


# Registry of the split-weight workspaces of persistent packed buffers: after the batched re-pack of an optimizer step
# (_repack_all) every registered split is re-made by ONE launch (dfmir_conv3d_wsplit_batch) instead of one launch per
# layer and mode at its first use.
_WS3D = {"entries": {}, "key": None, "dev": None}


def _ws3d_register(w_tcc, key, ws, job):
    """job = (kind, K, M, pair, Ktot, koff, Cb) as dfmir_conv3d_wsplit_batch reads them."""
    import weakref
    _WS3D["entries"][(id(w_tcc), key)] = {"ref": weakref.ref(w_tcc), "key": key, "ws": ws, "job": job}
    _WS3D["key"] = None


def _resplit_all_3d(dev):
    import numpy as np
    ents = _WS3D["entries"]
    for k_ in [k_ for k_, e in ents.items() if e["ref"]() is None]:
        del ents[k_]
        _WS3D["key"] = None
    live = [e for e in ents.values() if e["ws"].device == dev and getattr(e["ref"](), "_df_gen", None) is not None]
    if not live:
        return
    key = tuple((e["ref"]().data_ptr(), e["ws"].data_ptr()) + tuple(e["job"]) for e in live)
    if _WS3D["key"] != key:
        tab = np.zeros((len(live), 7), dtype=np.int64)
        for i, e in enumerate(live):
            kind, K, M, pair, Ktot, koff, Cb = e["job"]
            tab[i, 0] = e["ref"]().data_ptr()
            tab[i, 1] = e["ws"].data_ptr()
            tab[i, 2] = e["ws"].data_ptr() + 4 * (e["ws"].numel() - 4)
            tab[i, 3] = kind | (K << 32)
            tab[i, 4] = M | (pair << 32)
            tab[i, 5] = Ktot | (koff << 32)
            tab[i, 6] = Cb
        _WS3D["dev"] = torch.from_numpy(tab).to(dev)
        _KEEP_TABLES.append(_WS3D["dev"])
        _WS3D["key"] = key
    check(lib().dfmir_conv3d_wsplit_batch(_p(_WS3D["dev"]), len(live), _st()))
    for e in live:
        w_tcc = e["ref"]()
        w_tcc._df_ws3d[e["key"]] = (w_tcc._df_gen, e["ws"])


def _ws_cached(w_tcc, key, floats, device, job=None):
    """(ws, needs_split): a per-(packed-weight buffer, key) workspace for split weights, re-made only when the packed
    buffer was re-packed (its generation changed).  A temporary packing (no generation) gets a fresh workspace."""
    gen = getattr(w_tcc, "_df_gen", None)
    cache = getattr(w_tcc, "_df_ws3d", None) if gen is not None else None
    ent = cache.get(key) if cache is not None else None
    if ent is not None and ent[0] == gen:
        return ent[1], False
    ws = ent[1] if ent is not None else torch.empty(floats, device=device, dtype=torch.float32)   # in place: graphs hold it
    if gen is not None:
        if cache is None:
            cache = w_tcc._df_ws3d = {}
        cache[key] = (gen, ws)
        if ent is None and job is not None:
            _ws3d_register(w_tcc, key, ws, job)
    return ws, True


class _Ctx(object):
    pass


class UpCatConv3dFn(Function):
    """y = act(conv3x3x3(cat([nearest_up2(a), b], 1), weight) + bias)  (torchvoxelmorph/networks.py:64,97-100 + the next
    ConvBlock, :1506-1521) without the up-sampled / concatenated tensor in the forward pass: the up-sampled channels
    through the parity-class form (8 of the 27 products, csrc/conv3ds.hip conv3d_up_phase_k), the skip channels
    through the split kernel whose epilogue adds both, the bias and the activation.  Backward: the concatenation is
    materialised there (for the weight gradient's operand) and the existing dgrad / wgrad / pooling kernels run."""

    @staticmethod
    def forward(ctx, a, b, weight, bias, owner, act, slope):
        _need(a, b, weight, bias)
        a, b = _c(a), _c(b)
        N, Ca, D, H, W = a.shape
        Cb = b.shape[1]
        Cout = weight.shape[0]
        if tuple(b.shape[2:]) != (2 * D, 2 * H, 2 * W) or weight.shape[1] != Ca + Cb:
            raise DfmirHipError("upcat_conv3d: a %s, b %s, weight %s do not fit" % (tuple(a.shape), tuple(b.shape), tuple(weight.shape)))
        w_tcc = owner.packed(0) if owner is not None else weight_pack(weight, 0)
        pa = _valid_amax(a)
        pa = _probe64(a) if pa is None else pa
        pb = _valid_amax(b)
        pb = _probe64(b) if pb is None else pb
        y = torch.empty((N, Cout, 2 * D, 2 * H, 2 * W), device=a.device, dtype=torch.float32)
        g = DfConvGeom(N, Cb, Cout, 2 * D, 2 * H, 2 * W, 2 * D, 2 * H, 2 * W, 3, 3, 3, 1, 1, 1, 1, 1, 0, act, float(slope))
        fused = Cb <= 2 and act in (0, 1)
        ws_up, split_up = _ws_cached(w_tcc, ("up", Ca, Cout, Cb if fused else 0), lib().dfmir_conv3d_up_ws_floats(Ca, Cout),
                                     a.device, job=(1, Ca, Cout, 0, Ca + Cb, 0, Cb if fused else 0))
        ws_sk, split_sk = (None, False) if fused else \
            _ws_cached(w_tcc, ("skip", Ca, Cb, Cout), lib().dfmir_conv3d_split_ws_floats(Cb, Cout), a.device,
                       job=(0, Cb, Cout, lib().dfmir_conv3d_split_is_pair(Cout), Ca + Cb, Ca, 0))
        slot = amax_slot(a.device, PROBE_SLOTS)
        if _PROBE_AUDIT["on"]:
            _audit_probe(a, pa, "upcat conv a %s" % (tuple(a.shape),))
            _audit_probe(b, pb, "upcat conv b %s" % (tuple(b.shape),))

        def launch_fused():
            check(lib().dfmir_conv3d_up_skip2_fwd(_p(a), _p(pa), pa.numel(), _p(b), _p(pb), pb.numel(), Cb,
                                                  _p(w_tcc) if split_up else None, _p(ws_up), _p(bias), _p(y), _p(slot),
                                                  N, Ca, Cout, D, H, W, act, float(slope), _st()))

        def launch_up():
            check(lib().dfmir_conv3d_up_fwd(_p(a), _p(pa), pa.numel(), _p(w_tcc) if split_up else None, Ca + Cb, _p(ws_up),
                                            _p(y), N, Ca, Cout, D, H, W, _st()))

        def launch_skip():
            check(lib().dfmir_conv3d_split_fwd_add(ctypes.byref(g), _p(b), _p(pb), pb.numel(), _p(w_tcc) if split_sk else None,
                                                   Ca + Cb, Ca, _p(ws_sk), _p(bias), _p(y), _p(slot), _st()))

        prof = _CONV_PROFILER[0]
        vox = 8.0 * N * D * H * W
        size = _size_label(Cout)
        if fused:
            if prof is None:
                launch_fused()
            else:
                prof("conv3dup_" + size, 2.0 * vox * Cout * (Ca + Cb) * 27, launch_fused)   # reference-equivalent FLOPs
        elif prof is None:
            launch_up()
            launch_skip()
        else:
            prof("conv3dup_" + size, 2.0 * vox * Cout * Ca * 27, launch_up)        # reference-equivalent FLOPs (27 taps)
            prof("conv3ds_" + size, 2.0 * vox * Cout * Cb * 27, launch_skip)
        _LAST_CONV_AMAX[0] = slot
        ctx.save_for_backward(a, b, weight, y if act else None)
        ctx.probes = (pa, pb)
        ctx.cfg = (3, (3, 3, 3), 1, (1, 1, 1), 0, act, slope, owner)
        ctx.has_bias = bias is not None
        ta = getattr(a, "_df_act_sole", None)          # a = the output of a LeakyReLU ConvBlock feeding only this layer
        ctx.a_act = (ta[0], ta[1]) if (_tag_ok(a, ta) and not _NO_ACTGRAD) else None
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        a, b, weight, y = ctx.saved_tensors
        N, Ca, D, H, W = a.shape
        Cb = b.shape[1]
        Cout = weight.shape[0]
        nd, K, stride, p3, pad_mode, act, slope, owner = ctx.cfg
        dy = _c(dy)
        # gradient w.r.t. the conv's result (LeakyReLU backward, unless the consumer's dgrad epilogue already applied it)
        if act and not _tag_ok(dy, getattr(dy, "_df_premasked", None)):
            dpre = torch.empty_like(dy)
            if not ((dy.data_ptr() | y.data_ptr() | dpre.data_ptr()) & 15):
                slot = amax_slot(dy.device, PROBE_SLOTS)
                check(lib().dfmir_act_bwd_amax(_p(dy), _p(y), _p(dpre), dy.numel(), act, float(slope), _p(slot), _st()))
                tag_amax(dpre, slot)
            else:
                check(lib().dfmir_act_bwd(_p(dy), _p(y), _p(dpre), dy.numel(), act, float(slope), _st()))
            dy = dpre
        need_a, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        up_dgrad = need_a and not need_b and Cout % 8 == 0
        xp = amax_slot(a.device, PROBE_SLOTS)
        check(lib().dfmir_probe_merge(_p(ctx.probes[0]), _p(ctx.probes[1]), _p(xp), _st()))
        c = _Ctx()
        gfull = DfConvGeom(N, Ca + Cb, Cout, 2 * D, 2 * H, 2 * W, 2 * D, 2 * H, 2 * W, 3, 3, 3, 1, 1, 1, 1, 1, 0, 0, 0.0)
        gather = (up_dgrad and W % 4 == 0 and ctx.needs_input_grad[2]
                  and bool(lib().dfmir_conv3d_split_wgrad_ok(ctypes.byref(gfull))) and Cout >= 8)
        if gather:
            # the weight gradient stages its operand patch from a (at half the coordinates) and b: no concatenation
            x = None
            c.x_parts = (a, b)
        else:
            # the concatenation, for the weight gradient's operand (and the dgrad's reference shape)
            x = torch.empty((N, Ca + Cb) + tuple(b.shape[2:]), device=a.device, dtype=torch.float32)
            check(lib().dfmir_upcat_fwd(_p(a), _p(b), _p(x), N, Ca, Cb, D, H, W, 2, _st()))
        c.cfg, c.x_amax, c.has_bias = (nd, K, stride, p3, pad_mode, 0, 0.0, owner), xp, ctx.has_bias
        c.dead_tail = 0 if need_b else Cb
        c.in_act = None
        c.needs_input_grad = ((need_a or need_b) and not up_dgrad, ctx.needs_input_grad[2], ctx.needs_input_grad[3])
        dx, dw, dbias = _conv_backward_impl(c, dy, None, x, weight, None)
        da = db = None
        if up_dgrad:
            # d(a) directly at low resolution: the sum pool of nearest_up2's adjoint composed with the dgrad is a 4x4x4
            # stride-2 conv of dy, run in parity classes (csrc/conv3ds.hip conv3d_up_dgrad_k)
            w_tcc = owner.packed(0) if owner is not None else weight_pack(weight, 0)
            ws, split = _ws_cached(w_tcc, ("updgrad", Ca, Cout), lib().dfmir_conv3d_up_dgrad_ws_floats(Ca, Cout), a.device,
                                   job=(2, Ca, Cout, 0, Ca + Cb, 0, 0))
            dya = amax_of(dy)
            if _PROBE_AUDIT["on"]:
                _audit_probe(dy, dya, "upcat conv dY %s" % (tuple(dy.shape),))
            da = torch.empty_like(a)
            slot = amax_slot(a.device, PROBE_SLOTS)
            ia = ctx.a_act

            def launch():
                check(lib().dfmir_conv3d_up_dgrad(_p(dy), _p(dya), dya.numel(), _p(w_tcc) if split else None, Ca + Cb, _p(ws),
                                                  _p(da), _p(slot), _p(a) if ia else None, float(ia[1]) if ia else 0.0,
                                                  N, Ca, Cout, D, H, W, _st()))
            prof = _CONV_PROFILER[0]
            if prof is None:
                launch()
            else:
                size = _size_label(Ca)
                prof("conv3dup_" + size, 2.0 * 8.0 * N * D * H * W * Cout * Ca * 27, launch)     # reference-equivalent FLOPs
            tag_amax(da, slot)
            if ia:
                da._df_premasked = (da._version, da.data_ptr())
        elif dx is not None:
            dx = _c(dx)
            da = torch.empty_like(a) if need_a else None
            db = torch.empty_like(b) if need_b else None
            if da is not None or db is not None:
                check(lib().dfmir_upcat_bwd(_p(dx), _p(da), _p(db), N, Ca, Cb, D, H, W, 2, _st()))
        return da, db, dw, dbias, None, None, None


def upcat_conv3d_ok(a, b, weight):
    if _NO_SPLIT3D or a.dim() != 5 or not (a.is_cuda and b.is_cuda):
        return False
    N, Ca, D, H, W = a.shape
    return (tuple(weight.shape[2:]) == (3, 3, 3) and tuple(b.shape[2:]) == (2 * D, 2 * H, 2 * W)
            and bool(lib().dfmir_conv3d_up_ok(N, Ca, int(weight.shape[0]), D, H, W)))


def upcat_conv3d(a, b, weight, bias, owner, act=0, slope=0.0, sole=False):
    """The next ConvBlock applied to cat([nearest_up2(a), b], 1); see UpCatConv3dFn."""
    _LAST_CONV_AMAX[0] = None
    out = UpCatConv3dFn.apply(a, b, weight, bias, owner, act, slope)
    if _LAST_CONV_AMAX[0] is not None:
        tag_amax(out, _LAST_CONV_AMAX[0])
        _LAST_CONV_AMAX[0] = None
    if sole and act == 1:
        out._df_act_sole = (act, float(slope), out._version, out.data_ptr())
    return out


class CatChannelsFn(Function):
    """torch.cat([a, b], dim=1) for same-shape-but-channels tensors."""

    @staticmethod
    def forward(ctx, a, b):
        _need(a, b)
        a, b = _c(a), _c(b)
        if a.shape[0] != b.shape[0] or a.shape[2:] != b.shape[2:]:
            raise DfmirHipError("cat: shapes %s / %s differ outside dim 1" % (tuple(a.shape), tuple(b.shape)))
        N = a.shape[0]
        SA, SB = a.numel() // N, b.numel() // N
        y = torch.empty((N, a.shape[1] + b.shape[1]) + tuple(a.shape[2:]), device=a.device, dtype=torch.float32)
        check(lib().dfmir_cat_channels_fwd(_p(a), _p(b), _p(y), N, SA, SB, _st()))
        ctx.meta = (a.shape, b.shape, N, SA, SB)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        ash, bsh, N, SA, SB = ctx.meta
        dy = _c(dy)
        da = torch.empty(ash, device=dy.device, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        db = torch.empty(bsh, device=dy.device, dtype=torch.float32) if ctx.needs_input_grad[1] else None
        if da is not None or db is not None:
            check(lib().dfmir_cat_channels_bwd(_p(dy), _p(da), _p(db), N, SA, SB, _st()))
        return da, db


def upcat_channels(a, b):
    return CatChannelsFn.apply(a, b)


class CatBatchFn(Function):
    """torch.cat([a, b], dim=0) (registration_model.py:187) as one copy launch."""

    @staticmethod
    def forward(ctx, a, b):
        _need(a, b)
        a, b = _c(a), _c(b)
        if a.shape[1:] != b.shape[1:]:
            raise DfmirHipError("cat_batch: shapes %s / %s differ outside dim 0" % (tuple(a.shape), tuple(b.shape)))
        y = torch.empty((a.shape[0] + b.shape[0],) + tuple(a.shape[1:]), device=a.device, dtype=torch.float32)
        check(lib().dfmir_cat_channels_fwd(_p(a), _p(b), _p(y), 1, a.numel(), b.numel(), _st()))
        ctx.meta = (a.shape, b.shape)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        ash, bsh = ctx.meta
        dy = _c(dy)
        na = 1
        for s in ash:
            na *= s
        da = dy[:ash[0]] if ctx.needs_input_grad[0] else None
        db = dy[ash[0]:] if ctx.needs_input_grad[1] else None
        return da, db


def cat_batch(a, b):
    return CatBatchFn.apply(a, b)


class ScaleFn(Function):
    @staticmethod
    def forward(ctx, x, mult):
        _need(x)
        x = _c(x)
        y = torch.empty_like(x)
        check(lib().dfmir_scale(_p(x), _p(y), x.numel(), float(mult), _st()))
        ctx.mult = float(mult)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        dy = _c(dy)
        dx = torch.empty_like(dy)
        check(lib().dfmir_scale(_p(dy), _p(dx), dy.numel(), ctx.mult, _st()))
        return dx, None


def scale(x, mult):
    return ScaleFn.apply(x, mult)


# ------------------------------------------------------------------------------------------------
# warps
# ------------------------------------------------------------------------------------------------
def _warp_fwd(src, flow, mode, add_identity):
    nd = src.dim() - 2
    out = torch.empty_like(src)
    if nd == 2:
        B, C, H, W = src.shape
        check(lib().dfmir_warp2d_fwd(_p(src), _p(flow), _p(out), B, C, H, W, mode, add_identity, _st()))
    else:
        B, C, D, H, W = src.shape
        check(lib().dfmir_warp3d_fwd(_p(src), _p(flow), _p(out), B, C, D, H, W, mode, add_identity, _st()))
    return out


def _warp_bwd(dout, src, flow, dsrc, dflow, add_identity, into_src):
    nd = src.dim() - 2
    if nd == 2:
        B, C, H, W = src.shape
        check(lib().dfmir_warp2d_bwd(_p(dout), _p(src), _p(flow), _p(dsrc), _p(dflow), B, C, H, W,
                                     add_identity, into_src, _st()))
    else:
        B, C, D, H, W = src.shape
        check(lib().dfmir_warp3d_bwd(_p(dout), _p(src), _p(flow), _p(dsrc), _p(dflow), B, C, D, H, W,
                                     add_identity, into_src, _st()))


_WARP_ATOMIC = _env_on("DFMIR_WARP_ATOMIC")     # A/B switch: d(src) through global atomics


def _warp_bwd_dsrc(dout, src, flow, dflow, add_identity, into_src):
    """Backward of a warp that needs d(src): the atomic-free, bit-reproducible owner-gather kernels where the shape is
    eligible (W % 4 == 0), else the scatter with global atomics into a zeroed buffer.  Returns d(src)."""
    nd = src.dim() - 2
    B, C = src.shape[0], src.shape[1]
    D, H, W = (src.shape[2:] if nd == 3 else (1,) + tuple(src.shape[2:]))
    n = 0 if _WARP_ATOMIC else lib().dfmir_warp_bwd_own_ws_floats(nd, B, C, D, H, W)
    if n > 0:
        dsrc = torch.empty_like(src)
        ws = torch.empty(n, device=src.device, dtype=torch.float32)
        check(lib().dfmir_warp_bwd_own(nd, _p(dout), _p(src), _p(flow), _p(dsrc), _p(dflow), B, C, D, H, W, add_identity,
                                       into_src, _p(ws), _st()))
        return dsrc
    dsrc = zeros_like(src)
    _warp_bwd(dout, src, flow, dsrc, dflow, add_identity, into_src)
    return dsrc


class WarpFn(Function):
    @staticmethod
    def forward(ctx, src, flow, mode):
        _need(src, flow)
        src, flow = _c(src), _c(flow)
        nd = src.dim() - 2
        if flow.shape[1] != nd or flow.shape[0] != src.shape[0] or flow.shape[2:] != src.shape[2:]:
            raise DfmirHipError("warp: src %s / flow %s mismatch (expected grid and input to have same "
                                "batch size and spatial shape)" % (tuple(src.shape), tuple(flow.shape)))
        ctx.save_for_backward(src, flow)
        ctx.mode = mode
        return _warp_fwd(src, flow, mode, 0)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        src, flow = ctx.saved_tensors
        dout = _c(dout)
        dflow = None
        if ctx.needs_input_grad[1]:
            dflow = zeros_like(flow) if ctx.mode == 1 else torch.empty_like(flow)
        if ctx.mode == 1:
            if ctx.needs_input_grad[0]:
                raise DfmirHipError("nearest-mode warp backward is not implemented (inference only)")
            return None, dflow, None
        if ctx.needs_input_grad[0]:
            return _warp_bwd_dsrc(dout, src, flow, dflow, 0, 0), dflow, None
        _warp_bwd(dout, src, flow, None, dflow, 0, 0)
        return None, dflow, None


def warp(src, flow, mode="bilinear"):
    """src(x + flow(x)): mode 'nearest' for labels, 'cubic' = ops.warp_cubic (third-order B-spline, MIRROR extension where
    the linear mode pads with zeros), any other string the bi-/trilinear warp."""
    if mode == "cubic":
        return warp_cubic(src, flow)
    return WarpFn.apply(src, flow, 1 if mode == "nearest" else 0)


def _cubic_image(x, what, name):
    """(nd, D, H, W) of a [B,C,*vol] fp32 image of the cubic ops after its checks (ValueError: nothing is launched)."""
    if not torch.is_tensor(x) or x.dim() not in (4, 5):
        raise ValueError("%s: %s must be a [B,C,H,W] or [B,C,D,H,W] tensor, got %s"
                         % (what, name, tuple(x.shape) if torch.is_tensor(x) else type(x).__name__))
    if min(x.shape) < 1:
        raise ValueError("%s: %s needs B >= 1, C >= 1 and every extent >= 1, got %s" % (what, name, tuple(x.shape)))
    if x.dtype != torch.float32:
        raise ValueError("%s: fp32 tensors only (%s is %s)" % (what, name, x.dtype))
    if x.numel() >= 2 ** 31:
        raise ValueError("%s: %s %s has 2^31 or more elements" % (what, name, tuple(x.shape)))
    nd = x.dim() - 2
    D, H, W = (int(n) for n in (x.shape[2:] if nd == 3 else (1,) + tuple(x.shape[2:])))
    return nd, D, H, W


def _spline_prefilter(x, nd, D, H, W):
    out = torch.empty_like(x)
    tmp = torch.empty_like(x) if nd == 3 and D > 1 and (H > 1 or W > 1) else None
    check(lib().dfmir_spline_prefilter(nd, _p(x), _p(out), _p(tmp), int(x.shape[0]) * int(x.shape[1]), D, H, W, _st()))
    return out


@torch.no_grad()
def spline_prefilter(x):
    """The coefficients of the interpolating cubic B-spline of an image (build-defined): x [B,C,*vol] fp32, 2-D or 3-D,
    every extent >= 1; returns c of the same shape.  With refl the whole-sample mirror d c b | a b c d | c b a -- for an
    axis of extent n > 1, j = i mod (2 n - 2), refl(i) = j if j < n else 2 n - 2 - j; refl(i) = 0 for n == 1 -- c solves,
    along every axis in turn (the axes commute),

        (c[refl(i - 1)] + 4 c[i] + c[refl(i + 1)]) / 6 = s[i]

    which is scipy.ndimage.spline_filter(order=3, mode='mirror').  The kernel evaluates the exact inverse as the FIR
    c[i] = sum_{|k| <= 16} sqrt(3) z^|k| s[refl(i + k)], z = sqrt(3) - 2 (the tail is below 8e-10 max |s|); an axis of extent 1 is
    left alone bit for bit.  max |c| is about 2.3 max |s| for noise.  2-D is one launch, 3-D the (y, x) pass and a z pass
    (dfmir_amd/csrc/cubic.hip).  Bit-identical from run to run; nothing syncs with the host.  No gradient: an input that
    requires grad raises.  ValueError before any launch on a rank other than 4 or 5, an empty axis, a dtype other than fp32,
    2^31 or more elements and a tensor that requires grad; a CPU tensor raises the usual "no CPU fallback" error."""
    what = "spline_prefilter"
    nd, D, H, W = _cubic_image(x, what, "x")
    if x.requires_grad:
        raise ValueError("%s: x requires grad, but the op has no gradient (detach it)" % what)
    _need(x)
    return _spline_prefilter(_c(x), nd, D, H, W)


class WarpCubicFn(Function):
    """dfmir_warp_cubic_fwd / _bwd_flow on the prefiltered coefficients; the gradient goes to the flow only."""

    @staticmethod
    def forward(ctx, src, flow, prefiltered, geom):
        nd, D, H, W = geom
        src, flow = _c(src.detach()), _c(flow.detach())
        coef = src if prefiltered else _spline_prefilter(src, nd, D, H, W)
        B, C = int(src.shape[0]), int(src.shape[1])
        out = torch.empty_like(coef)
        check(lib().dfmir_warp_cubic_fwd(nd, _p(coef), _p(flow), _p(out), B, C, D, H, W, _st()))
        ctx.save_for_backward(coef, flow)
        ctx.geom = geom
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        if ctx.needs_input_grad[0]:
            raise DfmirHipError("warp_cubic: the gradient to src is not implemented (d(flow) only; detach src)")
        if not ctx.needs_input_grad[1]:
            return None, None, None, None
        coef, flow = ctx.saved_tensors
        nd, D, H, W = ctx.geom
        dflow = torch.empty_like(flow)
        check(lib().dfmir_warp_cubic_bwd_flow(nd, _p(_c(dout)), _p(coef), _p(flow), _p(dflow), int(coef.shape[0]),
                                              int(coef.shape[1]), D, H, W, _st()))
        return None, dflow, None, None


def warp_cubic(src, flow, prefiltered=False):
    """src(x + flow(x)) by third-order (cubic) B-spline interpolation (build-defined): src [B,C,*vol] fp32, 2-D or 3-D; flow
    [B,nd,*vol] in voxels, ops.warp's convention (channel a displaces axis a, p = x + flow(x)).  The image is first turned
    into spline coefficients c = ops.spline_prefilter(src) -- pass them yourself with prefiltered=True to warp one image
    many times -- and then, per axis, i = floor(p), t = p - i,

        w0 = (1 - t)^3 / 6    w1 = (3 t^3 - 6 t^2 + 4) / 6    w2 = (-3 t^3 + 3 t^2 + 3 t + 1) / 6    w3 = t^3 / 6
        out(x) = sum over the 4^nd taps of  prod_a w_ka(t_a) * c[refl(i_a - 1 + k_a)]

    with refl the whole-sample mirror of ops.spline_prefilter, applied at ANY distance outside the volume: exactly
    scipy.ndimage.map_coordinates(src, p, order=3, mode='mirror').  This DIVERGES ON PURPOSE from the linear and nearest
    modes of ops.warp, which pad with zeros: a point far outside reads a mirrored copy of the image, not 0.  The spline
    interpolates (zero flow returns src up to rounding) but is not confined to the range of src: it OVERSHOOTS at edges,
    and nothing clamps.  A position that is not finite, or has |p| >= 2^24 on any axis, gives out = 0 and a zero gradient.
    Gradient: to the flow only, dflow[b,a,x] = sum_c dout[b,c,x] d out[b,c,x] / d p_a with the derivative weights
    w0' = -(1 - t)^2 / 2, w1' = (3 t^2 - 4 t) / 2, w2' = (-3 t^2 + 2 t + 1) / 2, w3' = t^2 / 2 on axis a -- continuous across cell
    faces, unlike the linear warp's.  A src that requires grad raises DfmirHipError in the backward, as the nearest mode
    does.  One thread per voxel, no atomics: value and gradient are bit-identical from run to run; nothing syncs with the
    host.  ValueError before any launch on a rank other than 4 or 5, an empty axis, a flow that is not [B,nd,*vol], a dtype
    other than fp32, tensors on different devices, 2^31 or more elements and a prefiltered that is not a bool; a CPU tensor
    raises the usual "no CPU fallback" error."""
    what = "warp_cubic"
    if not isinstance(prefiltered, bool):
        raise ValueError("%s: prefiltered must be a bool, got %r" % (what, prefiltered))
    geom = _cubic_image(src, what, "src")
    nd = geom[0]
    want = (int(src.shape[0]), nd) + tuple(src.shape[2:])
    if not torch.is_tensor(flow) or tuple(flow.shape) != want:
        raise ValueError("%s: the flow of a %s image is [B,%d,*vol] = %s, got %s"
                         % (what, tuple(src.shape), nd, want, tuple(flow.shape) if torch.is_tensor(flow) else type(flow).__name__))
    if flow.dtype != torch.float32:
        raise ValueError("%s: fp32 tensors only (flow is %s)" % (what, flow.dtype))
    if flow.numel() >= 2 ** 31:
        raise ValueError("%s: flow %s has 2^31 or more elements" % (what, tuple(flow.shape)))
    if flow.device != src.device:
        raise ValueError("%s: src is on %s, flow on %s" % (what, src.device, flow.device))
    _need(src, flow)
    return WarpCubicFn.apply(src, flow, prefiltered, geom)


class VecIntStepFn(Function):
    """v -> v + warp(v, v)   (one scaling-and-squaring step, layers.py:66-67)."""

    @staticmethod
    def forward(ctx, v):
        _need(v)
        v = _c(v)
        ctx.save_for_backward(v)
        return _warp_fwd(v, v, 0, 1)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        (v,) = ctx.saved_tensors
        dout = _c(dout)
        return _warp_bwd_dsrc(dout, v, v, None, 1, 1)


def vecint_step(v):
    return VecIntStepFn.apply(v)


class ResizeFn(Function):
    @staticmethod
    def forward(ctx, x, out_sp, mult):
        _need(x)
        x = _c(x)
        nd = x.dim() - 2
        isp = tuple(x.shape[2:]) if nd == 3 else (1,) + tuple(x.shape[2:])
        osp = tuple(out_sp) if nd == 3 else (1,) + tuple(out_sp)
        planes = x.shape[0] * x.shape[1]
        y = torch.empty(tuple(x.shape[:2]) + tuple(out_sp), device=x.device, dtype=torch.float32)
        check(lib().dfmir_resize_fwd(_p(x), _p(y), planes, isp[0], isp[1], isp[2], osp[0], osp[1], osp[2],
                                     float(mult), _st()))
        ctx.meta = (x.shape, planes, isp, osp, float(mult))
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        xs, planes, isp, osp, mult = ctx.meta
        dy = _c(dy)
        dx = torch.empty(xs, device=dy.device, dtype=torch.float32)
        n = lib().dfmir_resize_bwd_ws_floats(planes, isp[0], isp[1], isp[2], osp[0], osp[1], osp[2])
        if n > 0:
            ws = torch.empty(n + 4, device=dy.device, dtype=torch.float32)
            check(lib().dfmir_resize_bwd_sep(_p(dy), _p(dx), planes, isp[0], isp[1], isp[2], osp[0], osp[1], osp[2],
                                             mult, _p(ws), _st()))
        else:
            check(lib().dfmir_resize_bwd(_p(dy), _p(dx), planes, isp[0], isp[1], isp[2], osp[0], osp[1], osp[2],
                                         mult, _st()))
        return dx, None, None


def resize_linear(x, out_sp, mult=1.0):
    return ResizeFn.apply(x, tuple(int(s) for s in out_sp), mult)


BSPLINE_MAX_STRIDE = 8                             # dfmir_amd/csrc/bspline.hip: what the weight tables are sized for


def _bspline_geometry(vol, stride, what):
    """(vol, stride) as tuples of nd ints, checked: nd = 2 or 3, every extent >= 1, every stride an integer in
    [1, BSPLINE_MAX_STRIDE] (a bool is no integer)."""
    is_int = lambda v: isinstance(v, int) and not isinstance(v, bool)
    if not isinstance(vol, (tuple, list, torch.Size)) or len(vol) not in (2, 3) \
            or not all(is_int(n) and n >= 1 for n in vol):
        raise ValueError("%s: vol must be 2 or 3 integer extents >= 1, got %r" % (what, vol))
    nd = len(vol)
    st = (stride,) * nd if is_int(stride) else stride
    if not isinstance(st, (tuple, list)) or len(st) != nd \
            or not all(is_int(s) and 1 <= s <= BSPLINE_MAX_STRIDE for s in st):
        raise ValueError("%s: stride must be an integer in [1, %d] or %d of them, got %r"
                         % (what, BSPLINE_MAX_STRIDE, nd, stride))
    return tuple(int(n) for n in vol), tuple(st)


def bspline_control_shape(vol, stride):
    """The control grid of a cubic B-spline deformation over a volume `vol` (nd ints) at control spacing `stride` (an int or
    nd ints in [1, 8]): m_a = (n_a - 1) // s_a + 4 points per axis, point j at voxel coordinate s_a (j - 1) -- one point
    before the first voxel and enough after the last."""
    vol, st = _bspline_geometry(vol, stride, "bspline_control_shape")
    return tuple((n - 1) // s + 4 for n, s in zip(vol, st))


class BSplineFn(Function):
    @staticmethod
    def forward(ctx, ctrl, vol, st):
        _need(ctrl)
        ctrl = _c(ctrl)
        nd = len(vol)
        planes = ctrl.shape[0] * ctrl.shape[1]
        geom = ((1,) + vol if nd == 2 else vol) + ((1,) + st if nd == 2 else st)
        ws = lib().dfmir_bspline_bwd_ws_floats(nd, planes, *geom) if ctx.needs_input_grad[0] else 0
        if ws < 0:
            raise DfmirHipError("bspline_flow: the backward refuses the field %s (W > 7944 or more than 65535 * 256 control "
                                "points per plane); detach ctrl if no gradient is wanted" % (tuple(ctrl.shape[:2]) + vol,))
        y = torch.empty(tuple(ctrl.shape[:2]) + vol, device=ctrl.device, dtype=torch.float32)
        check(lib().dfmir_bspline_fwd(nd, _p(ctrl), _p(y), planes, *geom, _st()))
        ctx.meta = (tuple(ctrl.shape), nd, planes, geom, ws)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        shape, nd, planes, geom, n = ctx.meta
        dy = _c(dy)
        dctrl = torch.empty(shape, device=dy.device, dtype=torch.float32)
        ws = torch.empty(n + 4, device=dy.device, dtype=torch.float32)
        check(lib().dfmir_bspline_bwd(nd, _p(dy), _p(dctrl), planes, *geom, _p(ws), _st()))
        return dctrl, None, None


def bspline_flow(ctrl, vol, stride):
    """The dense field of a cubic B-spline control grid, the free-form deformation of Rueckert et al. 1999 (build-defined,
    dfmir_amd/csrc/bspline.hip).  ctrl: [B,C,*m] fp32, any C >= 1, m = bspline_control_shape(vol, stride); vol: nd = 2 or 3
    ints; stride: the control spacing in voxels, an int or nd ints in [1, BSPLINE_MAX_STRIDE].  Returns [B,C,*vol]:

        y[b,c,x] = sum over l in {0,1,2,3}^nd of prod_a B_{l_a}(t_a) ctrl[b,c,q + l],   q_a = x_a // s_a, t_a = (x_a % s_a) / s_a
        B_0 = (1-t)^3 / 6   B_1 = (3t^3 - 6t^2 + 4) / 6   B_2 = (-3t^3 + 3t^2 + 3t + 1) / 6   B_3 = t^3 / 6

    which is a depthwise conv_transpose of ctrl with stride s and the separable kernel k_a[(3 - l) s_a + r] = B_l(r / s_a),
    cropped to [3 s_a, 3 s_a + n_a) on every axis.  The B*C planes are independent.  A zero grid gives +0.0 everywhere.  The
    gradient goes to ctrl only (once differentiable): the adjoint in gather form, no atomics, bit-identical from run to run;
    where (n_a - 1) % s_a == 0 the last control point of that axis only meets B_3(0) = 0 and its gradient is exactly 0.
    ValueError, before the library or the device is touched, on a bad vol or stride and on a ctrl that is not fp32 or not of
    the control shape.  The backward handles W <= 7944 and at most 65535 * 256 control points per plane: a ctrl that requires
    grad beyond that raises DfmirHipError at the forward; without a gradient the forward has neither limit."""
    what = "bspline_flow"
    vol, st = _bspline_geometry(vol, stride, what)
    m = tuple((n - 1) // s + 4 for n, s in zip(vol, st))
    if not torch.is_tensor(ctrl) or ctrl.dtype != torch.float32:
        raise ValueError("%s: ctrl must be an fp32 tensor, got %s" % (what, getattr(ctrl, 'dtype', type(ctrl).__name__)))
    if ctrl.dim() != len(vol) + 2 or tuple(ctrl.shape[2:]) != m or ctrl.shape[0] < 1 or ctrl.shape[1] < 1:
        raise ValueError("%s: ctrl must be [B,C,*%s], the control grid of volume %s at stride %s, got %s"
                         % (what, m, vol, st, tuple(ctrl.shape)))
    return BSplineFn.apply(ctrl, vol, st)


# ------------------------------------------------------------------------------------------------
# PatchNCE
# ------------------------------------------------------------------------------------------------
class TapForkFn(Function):
    """feat -> (main, tap): two aliases of a feature map that is tapped for PatchNCE sampling AND feeds the next
    layer.  The sampled rows' gradient is a scatter of a few hundred positions per plane; returned densely
    (zeros + scatter) autograd would then sum two full-size tensors.  `patch_gather` on `tap` instead parks
    (d rows, ids) in `stash` and returns no gradient; this node's backward scatters them into the next layer's
    gradient in place (or into zeros if `main` received none)."""

    @staticmethod
    def forward(ctx, feat, stash):
        ctx.stash = stash
        ctx.shape = tuple(feat.shape)
        ctx.set_materialize_grads(False)
        return feat.view_as(feat), feat.view_as(feat)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_main, g_tap):
        stash = ctx.stash
        g = g_main
        if stash:
            if g is None:
                g = zeros(ctx.shape, stash[0][0].device)
            elif not g.is_contiguous():
                g = g.contiguous()
            atag = getattr(g, "_df_amax", None)
            if atag is not None and not _amax_ok(g, atag):
                atag = None
            ptag = getattr(g, "_df_pmax", None)
            if ptag is not None and not (ptag[1] == g._version and ptag[2] == g.data_ptr()):
                ptag = None
            for dout, ids, (shape, B, C, S, Pn, G, distinct) in stash:
                if atag is not None and atag[0].numel() != PROBE_SLOTS:
                    atag = None
                if ptag is not None and (atag is None or ptag[0].numel() != B * C):
                    ptag = None
                # with a probe: keep g's range probes (from the InstanceNorm backward that produced it) valid
                if not distinct:          # caller-supplied ids with repeats: accumulate with atomics
                    check(lib().dfmir_patch_gather_bwd_any(_p(dout), _p(ids), _p(g), B, C, S, Pn, G,
                                                           _p(atag[0]) if atag is not None else None,
                                                           _p(ptag[0]) if ptag is not None else None, _st()))
                elif ptag is not None:
                    check(lib().dfmir_patch_gather_bwd_gp(_p(dout), _p(ids), _p(g), B, C, S, Pn, G, _p(atag[0]),
                                                          _p(ptag[0]), _st()))
                else:
                    check(lib().dfmir_patch_gather_bwd_g(_p(dout), _p(ids), _p(g), B, C, S, Pn, G,
                                                         _p(atag[0]) if atag is not None else None, _st()))
            del stash[:]
            # modified through the raw pointer: tags that were not maintained would be stale
            stale = ["_df_cols"]
            if atag is None:
                stale.append("_df_amax")
            if ptag is None:
                stale.append("_df_pmax")
            for tag in stale:
                if hasattr(g, tag):
                    delattr(g, tag)
        if g_tap is not None:                    # a dense gradient on the tap (some other use of it)
            g = g_tap if g is None else g + g_tap
        return g, None


def fork_tap(feat):
    """(main, tap) for a tapped feature that also feeds the next layer; see TapForkFn.  Without grad: (feat, feat)."""
    if not (torch.is_grad_enabled() and feat.requires_grad and feat.is_contiguous()):
        return feat, feat
    stash = []
    main, tap = TapForkFn.apply(feat, stash)
    tap._df_tap_stash = stash
    tag = getattr(feat, "_df_amax", None)
    if tag is not None and _amax_ok(feat, tag):
        tag_amax(main, tag[0])
        tag_amax(tap, tag[0])
    return main, tap


class PatchGatherFn(Function):
    """feat [B,C,*sp], ids int64 [P] (or [G,P]: image b uses row b // (B/G)) -> channel-major rows [C, B*P]."""

    @staticmethod
    def forward(ctx, feat, ids, groups=1, distinct=True):
        ids = _c(ids.to(torch.int64))            # (int32 ids are welcome: widened before the dtype check)
        _need(feat, ids)
        ctx.stash = getattr(feat, "_df_tap_stash", None) if feat.is_contiguous() else None
        feat = _c(feat)
        B, C = feat.shape[0], feat.shape[1]
        S = feat.numel() // (B * C)
        G = int(groups)
        if ids.numel() % G or B % G:
            raise DfmirHipError("patch_gather: ids [G,P] with G dividing the batch")
        Pn = ids.numel() // G
        out = torch.empty((C, B * Pn), device=feat.device, dtype=torch.float32)
        check(lib().dfmir_patch_gather_fwd_g(_p(feat), _p(ids), _p(out), B, C, S, Pn, G, _st()))
        ctx.save_for_backward(ids)
        ctx.meta = (feat.shape, B, C, S, Pn, G, bool(distinct))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        (ids,) = ctx.saved_tensors
        shape, B, C, S, Pn, G, distinct = ctx.meta
        dout = _c(dout)
        if ctx.stash is not None:                # collected by TapForkFn.backward, which runs after this node
            ctx.stash.append((dout, ids, ctx.meta))
            return None, None, None, None
        dfeat = zeros(shape, dout.device)
        if distinct:
            check(lib().dfmir_patch_gather_bwd_g(_p(dout), _p(ids), _p(dfeat), B, C, S, Pn, G, None, _st()))
        else:
            check(lib().dfmir_patch_gather_bwd_any(_p(dout), _p(ids), _p(dfeat), B, C, S, Pn, G, None, None, _st()))
        return dfeat, None, None, None


def mark_distinct(ids):
    """Tag an id tensor as a P-subset per group (what torch.randperm / dfmir_patch_ids_draw yield)."""
    ids._df_distinct = (ids._version, ids.data_ptr())
    return ids


def ids_distinct(ids, groups=1):
    """Are the ids of every group pairwise distinct?  Generated ids carry the tag of mark_distinct; a caller-supplied
    tensor (PatchSampleF.forward(patch_ids=...), model.patch_id_source) is checked on the host ONCE per tensor state
    (one device sync).  The non-atomic scatter of patch_gather's backward is a data race on repeated ids, so those go
    through the accumulating kernel instead."""
    tag = getattr(ids, "_df_distinct", None)
    if tag is not None and tag == (ids._version, ids.data_ptr()):
        return True
    # the verdict lives ON the tensor object (an address + version key does not identify content: a fresh tensor per
    # step usually gets the allocator's previous address with version 0)
    key = (ids._version, ids.data_ptr(), int(groups))
    seen = getattr(ids, "_df_distinct_checked", None)
    if seen is not None and seen[0] == key:
        return seen[1]
    if ids.is_cuda and torch.cuda.is_current_stream_capturing():    # (a host tensor: no device to ask, nothing captured)
        return False                          # no host round trip inside a capture: take the safe (atomic) form
    srt = torch.sort(ids.reshape(int(groups), -1), dim=1).values
    hit = bool((srt[:, 1:] != srt[:, :-1]).all()) if srt.shape[1] > 1 else True
    ids._df_distinct_checked = (key, hit)
    return hit


def patch_gather(feat, ids, groups=1):
    distinct = ids_distinct(ids, groups) if (torch.is_grad_enabled() and feat.requires_grad) else True
    return PatchGatherFn.apply(feat, ids, groups, distinct)


class L2NormFn(Function):
    """x [C, rows] -> x / (||x||_2 over C + eps)   (networks.py:499-502)."""

    @staticmethod
    def forward(ctx, x, eps):
        _need(x)
        x = _c(x)
        C, rows = x.shape
        y = torch.empty_like(x)
        nrm = torch.empty(rows, device=x.device, dtype=torch.float32)
        check(lib().dfmir_l2norm_fwd(_p(x), _p(y), _p(nrm), C, rows, float(eps), _st()))
        ctx.save_for_backward(x, nrm)
        ctx.eps = float(eps)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, nrm = ctx.saved_tensors
        dy = _c(dy)
        dx = torch.empty_like(x)
        check(lib().dfmir_l2norm_bwd(_p(dy), _p(x), _p(nrm), _p(dx), x.shape[0], x.shape[1], ctx.eps, _st()))
        return dx, None


def l2norm_rows(x, eps=1e-7):
    return L2NormFn.apply(x, eps)


PATCHNCE_BWD_MAX_C = 330     # NCE_BWD_CMAX of csrc/patchnce.hip: the scalar backward's key tile in 64 KB of LDS


def _patchnce_need_bwd(C, what):
    """The forward takes rows of up to 1019 channels, dfmir_patchnce_bwd only C <= 330 (its matrix-core form C <= 256).
    Refuse BEFORE the forward when q wants a gradient the library cannot compute, instead of raising in the middle of
    autograd."""
    if C > PATCHNCE_BWD_MAX_C:
        raise DfmirHipError("%s: no gradient kernel for %d channels (the backward takes C <= %d); detach q for the "
                            "loss value alone" % (what, C, PATCHNCE_BWD_MAX_C))


class PatchNCEFn(Function):
    """q, k [C, rows] -> per-row InfoNCE loss [rows]; gradient flows to q only (k is detached,
    patchnce.py:17)."""

    @staticmethod
    def forward(ctx, q, k, groups, T):
        _need(q, k)
        q, k = _c(q), _c(k)
        C, rows = q.shape
        if rows % groups != 0:
            raise DfmirHipError("patchnce: rows %d not divisible by groups %d" % (rows, groups))
        R = rows // groups
        if ctx.needs_input_grad[0]:
            _patchnce_need_bwd(C, "patchnce")
        loss = torch.empty(rows, device=q.device, dtype=torch.float32)
        probs = torch.empty((rows, R + 1), device=q.device, dtype=torch.float32)
        check(lib().dfmir_patchnce_fwd(_p(q), _p(k), _p(loss), _p(probs), rows, C, groups, float(T), _st()))
        ctx.save_for_backward(probs, k)
        ctx.meta = (rows, C, groups, float(T))
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, dloss):
        probs, k = ctx.saved_tensors
        rows, C, groups, T = ctx.meta
        dloss = _c(dloss)
        dq = torch.empty_like(k)
        check(lib().dfmir_patchnce_bwd(_p(dloss), _p(probs), _p(k), _p(dq), rows, C, groups, T, _st()))
        return dq, None, None, None


def patchnce_rows(q, k, groups, T):
    return PatchNCEFn.apply(q, k, groups, T)


class NCETermsFn(Function):
    """Per-row NCE losses of L layers and T stacked terms -> the T per-term losses
    scale * sum_l mean(rows_l[t])  (registration_model.py:247-253 for every term at once).  q[l], k[l]: channel-major
    [C, T*seg]; one PatchNCE launch per layer writes into one [L, T*seg] buffer, one launch reduces it."""

    @staticmethod
    def forward(ctx, groups, temp, scale, n_terms, *qk):
        L = len(qk) // 2
        qs = [_c(t) for t in qk[:L]]
        ks = [_c(t) for t in qk[L:]]
        _need(*qs)
        _need(*ks)
        for l in range(L):
            if ctx.needs_input_grad[4 + l]:
                _patchnce_need_bwd(qs[l].shape[0], "nce_terms")
        rows = qs[0].shape[1]
        if rows % n_terms or rows % groups:
            raise DfmirHipError("nce_terms: %d rows, %d terms, %d groups" % (rows, n_terms, groups))
        seg = rows // n_terms
        R = rows // groups
        dev = qs[0].device
        buf = torch.empty((L, rows), device=dev, dtype=torch.float32)
        probs = []
        for l in range(L):
            C = qs[l].shape[0]
            pr = torch.empty((rows, R + 1), device=dev, dtype=torch.float32)
            check(lib().dfmir_patchnce_fwd(_p(qs[l]), _p(ks[l]), _VP(buf.data_ptr() + 4 * l * rows), _p(pr), rows, C,
                                           groups, float(temp), _st()))
            probs.append(pr)
        out = torch.empty(n_terms, device=dev, dtype=torch.float32)
        check(lib().dfmir_segment_means_fwd(_p(buf), _p(out), L, n_terms, seg, float(scale), _st()))
        ctx.save_for_backward(*(probs + ks))
        ctx.meta = (L, rows, seg, groups, float(temp), float(scale), n_terms, [q.shape[0] for q in qs])
        ctx.rows_buf = buf            # kept for inspection (tests read the per-row losses)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        L, rows, seg, groups, temp, scale, n_terms, Cs = ctx.meta
        saved = ctx.saved_tensors
        probs, ks = saved[:L], saved[L:]
        g = _c(g)
        drows = torch.empty((L, rows), device=g.device, dtype=torch.float32)
        check(lib().dfmir_segment_means_bwd(_p(g), _p(drows), L, n_terms, seg, scale, _st()))
        dqs = []
        for l in range(L):
            dq = torch.empty_like(ks[l])
            check(lib().dfmir_patchnce_bwd(_VP(drows.data_ptr() + 4 * l * rows), _p(probs[l]), _p(ks[l]), _p(dq), rows,
                                           Cs[l], groups, temp, _st()))
            dqs.append(dq)
        return (None, None, None, None) + tuple(dqs) + (None,) * L


def nce_terms(qs, ks, groups, temp, scale, n_terms):
    """qs, ks: lists (per layer) of channel-major [C, T*seg] rows -> tensor [n_terms] of per-term losses."""
    return NCETermsFn.apply(int(groups), temp, scale, int(n_terms), *(list(qs) + [k.detach() for k in ks]))


class ScalarCombineFn(Function):
    """out[j] = sum_i M[j][i] * in_i for 0-dim device scalars in_i (one launch; gradients are M^T g)."""

    @staticmethod
    def forward(ctx, M, *ins):
        import numpy as np
        _need(*ins)
        n_in, n_out = len(ins), len(M)
        Mh = np.ascontiguousarray(np.asarray(M, dtype=np.float32).reshape(n_out, n_in))
        ptrs = (ctypes.c_void_p * n_in)(*[t.data_ptr() for t in ins])
        out = torch.empty(n_out, device=ins[0].device, dtype=torch.float32)
        check(lib().dfmir_scalar_combine_fwd(ptrs, n_in, Mh.ctypes.data, n_out, _p(out), _st()))
        ctx.M = Mh
        ctx.shapes = [tuple(t.shape) for t in ins]
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        g = _c(g)
        n_out, n_in = ctx.M.shape
        din = torch.empty(n_in, device=g.device, dtype=torch.float32)
        check(lib().dfmir_scalar_combine_bwd(_p(g), n_in, ctx.M.ctypes.data, n_out, _p(din), _st()))
        return (None,) + tuple(din[i].view(ctx.shapes[i]) for i in range(n_in))


def scalar_combine(M, ins):
    """M: n_out rows of n_in coefficients; ins: device scalars (0-dim or 1-element tensors) -> tensor [n_out]."""
    return ScalarCombineFn.apply(M, *ins)


# device-side patch-id generator state: {seed, draw counter, finished-workgroup counter}
_IDS_STATE = {}


def _cuda_device(device):
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise DfmirHipError("patch ids are drawn on the HIP device, not on %s" % device)
    return torch.device("cuda", torch.cuda.current_device() if device.index is None else device.index)


def seed_patch_ids(seed, device=None):
    """(Re)seed the device patch-id generator (default seed: torch's initial_seed at first use).  The state tensor is
    updated in place once it exists: a captured hipGraph holds its address."""
    device = _cuda_device(device)
    new = torch.tensor([int(seed) & 0x7FFFFFFFFFFFFFFF, 0, 0], dtype=torch.int64)
    st = _IDS_STATE.get(device)
    if st is None:
        st = _IDS_STATE[device] = new.to(device)
    else:
        st.copy_(new)
    return st


def draw_patch_ids(sizes, n_sets, P, device):
    """[n_layers, n_sets, P] int64: for each layer l and set t a uniformly random P-subset of [0, sizes[l])
    (PatchSampleF's torch.randperm(S)[:P], models/networks.py:609-610), all in ONE launch, no host round trip."""
    device = _cuda_device(device)
    st = _IDS_STATE.get(device)
    if st is None:
        st = seed_patch_ids(torch.initial_seed(), device)
    L = len(sizes)
    out = torch.empty((L, n_sets, P), device=device, dtype=torch.int64)
    sz = (ctypes.c_longlong * L)(*[int(s) for s in sizes])
    check(lib().dfmir_patch_ids_draw(_p(st), sz, L, int(n_sets), int(P), _p(out), _st()))
    return mark_distinct(out)


def patch_gather_multi(srcs, ids):
    """srcs: G tensors [Bper, C, *sp] (no gradient: the detached key side); ids [G, P] -> [C, G*Bper*P]."""
    _need(*srcs)
    ids = _c(ids.to(torch.int64))
    _need(ids)
    G = len(srcs)
    srcs = [_c(s) for s in srcs]
    Bper, C = srcs[0].shape[0], srcs[0].shape[1]
    S = srcs[0].numel() // (Bper * C)
    for s_ in srcs:
        if tuple(s_.shape) != tuple(srcs[0].shape):
            raise DfmirHipError("patch_gather_multi: sources differ in shape")
    if ids.dim() != 2 or ids.shape[0] != G:
        raise DfmirHipError("patch_gather_multi: ids must be [G, P]")
    Pn = ids.shape[1]
    out = torch.empty((C, G * Bper * Pn), device=srcs[0].device, dtype=torch.float32)
    ptrs = (ctypes.c_void_p * G)(*[s_.data_ptr() for s_ in srcs])
    check(lib().dfmir_patch_gather_fwd_multi(ptrs, G, _p(ids), _p(out), Bper, C, S, Pn, _st()))
    return out


def nce_head_ok(C, nc, use_mlp):
    return use_mlp and nc == 256 and 1 <= C <= 256


def _nce_head_launch(ptrs, G, ids, mlp0, mlp2, Bper, C, S, Pn, eps, device, save):
    rows = G * Bper * Pn
    out = torch.empty((256, rows), device=device, dtype=torch.float32)
    nrm = xs = hs = ypre = None
    if save:
        nrm = torch.empty(rows, device=device, dtype=torch.float32)
        xs = torch.empty((C, rows), device=device, dtype=torch.float32)
        hs = torch.empty((256, rows), device=device, dtype=torch.float32)
        ypre = torch.empty((256, rows), device=device, dtype=torch.float32)
    arr = (ctypes.c_void_p * G)(*ptrs)
    check(lib().dfmir_nce_head_fwd(arr, G, _p(ids), _p(mlp0.packed(0)), _p(mlp0.bias), _p(mlp2.packed(0)), _p(mlp2.bias),
                                   _p(out), _p(nrm), _p(xs), _p(hs), _p(ypre), Bper, C, S, Pn, float(eps), _st()))
    return out, nrm, xs, hs, ypre


def nce_head_multi(srcs, ids, mlp0, mlp2, eps=1e-7):
    """Key side (no gradient): G source tensors [Bper, C, *sp], ids [G, P] -> L2-normalised projections [256, G*Bper*P]."""
    _need(*srcs)
    srcs = [_c(s_) for s_ in srcs]
    Bper, C = srcs[0].shape[0], srcs[0].shape[1]
    S = srcs[0].numel() // (Bper * C)
    ids = _c(ids.to(torch.int64))
    _need(ids)
    out, _, _, _, _ = _nce_head_launch([s_.data_ptr() for s_ in srcs], len(srcs), ids, mlp0, mlp2, Bper, C, S, ids.shape[1], eps,
                                       srcs[0].device, False)
    return out


class NceHeadFn(Function):
    """Query side: feat [B, C, *sp] (the G terms' images stacked along the batch), ids [G, P] -> [256, B*P]; the backward
    runs the chain the unfused modules would run (l2norm, the two Linear layers' dgrad / wgrad / bias gradients, the
    sampled-feature scatter) on the intermediates the fused forward saved."""

    @staticmethod
    def forward(ctx, feat, ids, w1, b1, w2, b2, mlp0, mlp2, eps, distinct):
        ids = _c(ids.to(torch.int64))
        _need(feat, ids)
        ctx.stash = getattr(feat, "_df_tap_stash", None) if feat.is_contiguous() else None
        feat = _c(feat)
        G, Pn = ids.shape
        B, C = feat.shape[0], feat.shape[1]
        if B % G:
            raise DfmirHipError("nce_head: ids [G,P] with G dividing the batch")
        Bper = B // G
        S = feat.numel() // (B * C)
        base = feat.data_ptr()
        ptrs = [base + 4 * g * Bper * C * S for g in range(G)]
        out, nrm, xs, hs, ypre = _nce_head_launch(ptrs, G, ids, mlp0, mlp2, Bper, C, S, Pn, eps, feat.device, True)
        ctx.save_for_backward(ids, nrm, xs, hs, ypre, w1, w2)
        ctx.meta = (tuple(feat.shape), B, C, S, Pn, G, bool(distinct), float(eps))
        ctx.mods = (mlp0, mlp2)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        ids, nrm, xs, hs, ypre, w1, w2 = ctx.saved_tensors
        shape, B, C, S, Pn, G, distinct, eps = ctx.meta
        mlp0, mlp2 = ctx.mods
        rows = B * Pn
        dout = _c(dout)
        dy = torch.empty_like(ypre)
        check(lib().dfmir_l2norm_bwd(_p(dout), _p(ypre), _p(nrm), _p(dy), 256, rows, eps, _st()))
        # Linear(256, 256): y = W2 h + b2
        c2 = _Ctx()
        c2.cfg, c2.x_amax, c2.dead_tail, c2.in_act, c2.has_bias = (2, (1, 1, 1), 1, (0, 0, 0), 0, 0, 0.0, mlp2), None, 0, None, True
        c2.needs_input_grad = (True, ctx.needs_input_grad[4], ctx.needs_input_grad[5])
        dh, dw2, db2 = _conv_backward_impl(c2, dy.view(1, 256, 1, rows), None, hs.view(1, 256, 1, 1, rows),
                                           w2.view(256, 256, 1, 1), None)
        # Linear(C, 256) + ReLU: h = relu(W1 x + b1)
        c1 = _Ctx()
        c1.cfg, c1.x_amax, c1.dead_tail, c1.in_act, c1.has_bias = (2, (1, 1, 1), 1, (0, 0, 0), 0, 1, 0.0, mlp0), None, 0, None, True
        c1.needs_input_grad = (ctx.needs_input_grad[0], ctx.needs_input_grad[2], ctx.needs_input_grad[3])
        dx, dw1, db1 = _conv_backward_impl(c1, dh, None, xs.view(1, C, 1, 1, rows), w1.view(256, C, 1, 1),
                                           hs.view(1, 256, 1, 1, rows))
        dfeat = None
        if dx is not None:
            dxr = _c(dx).view(C, rows)
            meta = (shape, B, C, S, Pn, G, distinct)
            if ctx.stash is not None:
                ctx.stash.append((dxr, ids, meta))
            else:
                dfeat = zeros(shape, dxr.device)
                if distinct:
                    check(lib().dfmir_patch_gather_bwd_g(_p(dxr), _p(ids), _p(dfeat), B, C, S, Pn, G, None, _st()))
                else:
                    check(lib().dfmir_patch_gather_bwd_any(_p(dxr), _p(ids), _p(dfeat), B, C, S, Pn, G, None, None, _st()))
        dw1 = dw1.view(256, C) if dw1 is not None else None          # the Linear parameters are [out, in]
        dw2 = dw2.view(256, 256) if dw2 is not None else None
        return dfeat, None, dw1, db1, dw2, db2, None, None, None, None


def nce_head(feat, ids, mlp0, mlp2, eps=1e-7):
    """Query side with gradient; see NceHeadFn."""
    groups = ids.shape[0] if ids.dim() == 2 else 1
    ids2 = ids if ids.dim() == 2 else ids.view(1, -1)
    distinct = ids_distinct(ids, groups) if (torch.is_grad_enabled() and feat.requires_grad) else True
    return NceHeadFn.apply(feat, ids2, mlp0.weight, mlp0.bias, mlp2.weight, mlp2.bias, mlp0, mlp2, eps, distinct)


# ------------------------------------------------------------------------------------------------
# scalar losses
# ------------------------------------------------------------------------------------------------
_LAST_L1_WS = [None]


class MaskedL1Fn(Function):
    @staticmethod
    def forward(ctx, a, b, mask, thr):
        _need(a, b, mask)
        a, b = _c(a), _c(b)
        m = None
        if mask is not None:
            m = _c(mask.to(torch.bool))
            if m.shape != a.shape:
                m = _c(m.expand_as(a))
        ws = torch.empty(8, device=a.device, dtype=torch.float32)
        out = torch.empty((), device=a.device, dtype=torch.float32)
        check(lib().dfmir_masked_l1_fwd(_p(a), _p(b), _p(m), float(thr), _p(ws), _p(out), a.numel(), _st()))
        _LAST_L1_WS[0] = ws
        ctx.save_for_backward(a, b, m, ws)
        ctx.thr = float(thr)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        a, b, m, ws = ctx.saved_tensors
        g = _c(g)
        da = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        db = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        if da is not None or db is not None:
            check(lib().dfmir_masked_l1_bwd(_p(a), _p(b), _p(m), ctx.thr, _p(ws), _p(g), _p(da), _p(db),
                                            a.numel(), _st()))
        return da, db, None, None


def masked_l1(a, b, mask=None, thr=-0.95):
    """sum(|a-b|*m)/sum(m); m = mask if given else (a>thr)|(b>thr).  The result carries `_df_mask_sum` = sum(m) (a
    0-dim view of the kernel's workspace) for the global-batch normalisation of the data-parallel form."""
    out = MaskedL1Fn.apply(a, b, mask, thr)
    out._df_mask_sum = _LAST_L1_WS[0][1]
    return out


class FlowSmoothFn(Function):
    @staticmethod
    def forward(ctx, flow, penalty=2):
        _need(flow)
        flow = _c(flow)
        nd = flow.dim() - 2
        B, C = flow.shape[0], flow.shape[1]
        D, H, W = flow.shape[2:] if nd == 3 else (1,) + tuple(flow.shape[2:])
        ws = torch.empty(int(lib().dfmir_flow_smooth_ws_floats()), device=flow.device, dtype=torch.float32)
        out = torch.empty((), device=flow.device, dtype=torch.float32)
        if penalty == 2:
            check(lib().dfmir_flow_smooth_fwd(_p(flow), _p(ws), _p(out), B, C, D, H, W, _st()))
        else:
            check(lib().dfmir_flow_smooth_fwd_p(_p(flow), _p(ws), _p(out), B, C, D, H, W, int(penalty), _st()))
        ctx.save_for_backward(flow)
        ctx.meta = (B, C, D, H, W, int(penalty))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (flow,) = ctx.saved_tensors
        B, C, D, H, W, penalty = ctx.meta
        g = _c(g)
        df = torch.empty_like(flow)
        if penalty == 2:
            check(lib().dfmir_flow_smooth_bwd(_p(flow), _p(g), _p(df), B, C, D, H, W, _st()))
        else:
            check(lib().dfmir_flow_smooth_bwd_p(_p(flow), _p(g), _p(df), B, C, D, H, W, penalty, _st()))
        return df, None


def flow_smoothness(flow, penalty='l2'):
    """mean over axes of mean(|forward difference|^p): smooothing_loss (registration_model.py:25-32), Grad_Loss
    (util/losses.py:81-130) and vxm Grad (torchvoxelmorph/losses.py:93-117); penalty 'l2' (p = 2) or 'l1' (p = 1)."""
    if penalty not in ('l1', 'l2'):
        raise DfmirHipError("gradient penalty must be 'l1' or 'l2', got %r" % (penalty,))
    return FlowSmoothFn.apply(flow, 2 if penalty == 'l2' else 1)


def bending_spacing(spacing, lengths, what):
    """The voxel spacing of a bending energy as a tuple of floats: None = all ones (of lengths[0] entries), otherwise a
    sequence of positive finite numbers whose length is one of `lengths` (ValueError otherwise)."""
    if spacing is None:
        return (1.0,) * lengths[0]
    try:
        vals = tuple(spacing)
    except TypeError:
        vals = None
    if vals is None or isinstance(spacing, str) or len(vals) not in lengths:
        raise ValueError("%s: spacing must be a sequence of %s numbers, got %r"
                         % (what, " or ".join(str(n) for n in lengths), spacing))
    for v in vals:
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) \
                or not np.isfinite(v) or not 0.0 < float(np.float32(v)) < float('inf'):
            raise ValueError("%s: spacing must hold positive finite numbers, got %r" % (what, spacing))
    return tuple(float(v) for v in vals)


def bending_geom(flow, spacing, what):
    """(B, C, D, H, W, hz, hy, hx) of a bending-energy input after the argument checks (ValueError: nothing is launched).
    A 5-D field of one plane is the 2-D field it is: its spacing has 2 entries, or 3 with the first ignored."""
    if flow.dim() not in (4, 5):
        raise ValueError("%s: expects a [B,C,H,W] or [B,C,D,H,W] field, got %d dims" % (what, flow.dim()))
    nd = flow.dim() - 2
    B, C = int(flow.shape[0]), int(flow.shape[1])
    D, H, W = (int(v) for v in (flow.shape[2:] if nd == 3 else (1,) + tuple(flow.shape[2:])))
    if B < 1 or C < 1:
        raise ValueError("%s: empty tensor %s" % (what, tuple(flow.shape)))
    short = [n for n in ((H, W) if D == 1 else (D, H, W)) if n < 3]
    if short:
        raise ValueError("%s: every axis needs an extent of at least 3 (a voxel with its whole 3^nd neighbourhood inside "
                         "the volume), got %s" % (what, tuple(flow.shape[2:])))
    if B * C * D * H * W >= 2 ** 31:
        raise ValueError("%s: fields of 2^31 and more elements are not supported, got %s" % (what, tuple(flow.shape)))
    sp = bending_spacing(spacing, (2,) if nd == 2 else ((2, 3) if D == 1 else (3,)), what)
    hz, hy, hx = sp if len(sp) == 3 else (1.0,) + sp
    return B, C, D, H, W, hz, hy, hx


class BendingEnergyFn(Function):
    """dfmir_bend_fwd / _bwd: the forward keeps the field alone, the backward re-forms the second differences in LDS."""

    @staticmethod
    def forward(ctx, flow, geom):
        flow = _c(flow)
        B, C, D, H, W, hz, hy, hx = geom
        ws = torch.empty(int(lib().dfmir_bend_ws_floats(B, C, D, H, W)), device=flow.device, dtype=torch.float32)
        out = torch.empty((), device=flow.device, dtype=torch.float32)
        check(lib().dfmir_bend_fwd(_p(flow), _p(ws), _p(out), B, C, D, H, W, hz, hy, hx, _st()))
        ctx.save_for_backward(flow)
        ctx.meta = geom
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (flow,) = ctx.saved_tensors
        B, C, D, H, W, hz, hy, hx = ctx.meta
        g = _c(g)
        df = torch.empty_like(flow)
        check(lib().dfmir_bend_bwd(_p(flow), _p(g), _p(df), B, C, D, H, W, hz, hy, hx, _st()))
        return df, None


def bending_energy(flow, spacing=None):
    """Bending energy of a field [B,C,*vol] (2-D or 3-D, any C >= 1; build-defined, the definition: losses.
    BendingEnergy_Loss): the mean over (B, C, Omega) of sum_a u_aa^2 + 2 sum_{a<b} u_ab^2 with central second differences
    divided by the voxel spacing (`spacing`, one positive number per axis in the order (z,) y, x; None = 1), Omega = the
    voxels whose whole 3^nd neighbourhood lies in the volume.  A [B,C,1,H,W] field is the 2-D field it is (spacing of 2
    entries, or 3 with the first ignored).  ValueError before any launch on a bad rank or spacing, on an axis shorter
    than 3 and on 2^31 or more elements; a CPU tensor raises the usual "no CPU fallback" error."""
    geom = bending_geom(flow, spacing, "bending_energy")
    _need(flow)
    if flow.dtype != torch.float32:
        raise DfmirHipError("bending_energy: fp32 tensors only (got %s)" % flow.dtype)
    return BendingEnergyFn.apply(flow, geom)


def _jacobian_geom(flow, border, what):
    """(nd, B, D, H, W, border) of a Jacobian-determinant input after the argument checks: ValueError on a bad rank, channel
    count, border, extent or size (nothing is launched), then the usual errors for a CPU tensor and a dtype other than fp32."""
    if not torch.is_tensor(flow) or flow.dim() not in (4, 5):
        raise ValueError("%s: expects a [B,2,H,W] or [B,3,D,H,W] displacement field, got %s"
                         % (what, "%d dims" % flow.dim() if torch.is_tensor(flow) else type(flow).__name__))
    nd = flow.dim() - 2
    if int(flow.shape[1]) != nd:
        raise ValueError("%s: a %d-D field needs %d channels, one displacement per axis, got %s"
                         % (what, nd, nd, tuple(flow.shape)))
    if isinstance(border, bool) or not isinstance(border, (int, np.integer)) or border < 1:
        raise ValueError("%s: border must be an integer >= 1, got %r" % (what, border))
    border = int(border)
    B = int(flow.shape[0])
    D, H, W = (int(v) for v in (flow.shape[2:] if nd == 3 else (1,) + tuple(flow.shape[2:])))
    if B < 1:
        raise ValueError("%s: empty tensor %s" % (what, tuple(flow.shape)))
    if min(int(n) for n in flow.shape[2:]) < 2 * border + 1:
        raise ValueError("%s: every axis needs an extent of at least 2 * border + 1 = %d, got %s%s"
                         % (what, 2 * border + 1, tuple(flow.shape[2:]),
                            " (a one-plane volume [B,3,1,H,W] is refused, not reinterpreted as a 2-D field: pass "
                            "flow[:, 1:, 0])" if nd == 3 and D == 1 else ""))
    if B * nd * D * H * W >= 2 ** 31:
        raise ValueError("%s: fields of 2^31 and more elements are not supported, got %s" % (what, tuple(flow.shape)))
    _need(flow)
    if flow.dtype != torch.float32:
        raise DfmirHipError("%s: fp32 tensors only (got %s)" % (what, flow.dtype))
    return nd, B, D, H, W, border


def _jacobian_ws(flow, geom):
    nd, B, D, H, W, _ = geom
    return torch.empty(int(lib().dfmir_jacdet_ws_floats(nd, B, D, H, W)), device=flow.device, dtype=torch.float32)


def _finite_ge0(what, name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or v < 0:
        raise ValueError("%s: %s must be a finite number >= 0, got %r" % (what, name, v))
    return float(v)


class JacobianPenaltyFn(Function):
    """dfmir_jacdet_fwd / _bwd: the forward keeps the field alone, the backward re-forms the cofactors in LDS."""

    @staticmethod
    def forward(ctx, flow, geom, eps, power):
        flow = _c(flow)
        nd, B, D, H, W, border = geom
        ws = _jacobian_ws(flow, geom)
        out = torch.empty((), device=flow.device, dtype=torch.float32)
        check(lib().dfmir_jacdet_fwd(nd, _p(flow), _p(ws), _p(out), B, D, H, W, border, eps, power, _st()))
        ctx.save_for_backward(flow)
        ctx.meta = (geom, eps, power)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (flow,) = ctx.saved_tensors
        (nd, B, D, H, W, border), eps, power = ctx.meta
        g = _c(g)
        df = torch.empty_like(flow)
        check(lib().dfmir_jacdet_bwd(nd, _p(flow), _p(g), _p(df), B, D, H, W, border, eps, power, _st()))
        return df, None, None, None


def jacobian_penalty(flow, eps=0.0, power=2, border=1):
    """The fold penalty of a displacement field [B,nd,*vol] (2-D or 3-D, fp32; build-defined, the definition:
    losses.JacobianDet_Loss): the mean over (B, Omega) of max(0, eps - det J)^power, J = I + the central differences of the
    field, Omega = the voxels at least `border` away from every face; power 1 or 2, eps >= 0.  A scalar with the exact
    adjoint as its gradient.  No spacing argument: the determinant does not depend on the voxel spacing (J_phys = H J
    H^-1).  ValueError before any launch on a bad rank, a channel count other than nd (a [B,3,1,H,W] field is refused),
    an axis shorter than 2 border + 1, 2^31 or more elements, a bad eps, power or border; a CPU tensor raises the usual
    "no CPU fallback" error."""
    what = "jacobian_penalty"
    if isinstance(power, bool) or power not in (1, 2):
        raise ValueError("%s: power must be 1 or 2, got %r" % (what, power))
    eps = _finite_ge0(what, "eps", eps)
    geom = _jacobian_geom(flow, border, what)
    return JacobianPenaltyFn.apply(flow, geom, eps, int(power))


def jacobian_determinant(flow, border=1):
    """det J of phi = x + flow, J = I + the central differences of the field [B,nd,*vol] (ops.warp's convention: channel a
    displaces axis a in voxels, order (z,) y, x): a map [B,1,*vol] that holds the determinant on Omega (the voxels at
    least `border` away from every face) and exactly 1.0, the identity's value, outside, so a plot needs no mask.  Not
    differentiable (ops.jacobian_penalty is).  The determinant does not depend on the voxel spacing, so there is no
    spacing argument.  Argument checks as ops.jacobian_penalty."""
    nd, B, D, H, W, border = _jacobian_geom(flow, border, "jacobian_determinant")
    flow = _c(flow.detach())
    out = torch.empty((B, 1) + tuple(flow.shape[2:]), device=flow.device, dtype=torch.float32)
    check(lib().dfmir_jacdet_map(nd, _p(flow), _p(out), B, D, H, W, border, _st()))
    return out


def jacobian_stats(flow, border=1, log_offset=0.0, log_floor=1e-9):
    """Regularity statistics of a displacement field [B,nd,*vol], per sample over Omega (the voxels at least `border` away
    from every face): a float64 tensor [B,6] of (the count of det J <= 0, min, max and mean of det J, mean and population
    standard deviation of l = log(max(det J + log_offset, log_floor))).  border=2, log_offset=3 is the Learn2Reg
    convention for SDlogJ.  The sums are taken in double in a fixed order.  The determinant does not depend on the voxel
    spacing, so there is no spacing argument.  Argument checks as ops.jacobian_penalty; log_offset >= 0 and log_floor > 0,
    both finite."""
    what = "jacobian_stats"
    log_offset = _finite_ge0(what, "log_offset", log_offset)
    if _finite_ge0(what, "log_floor", log_floor) == 0.0:
        raise ValueError("%s: log_floor must be a finite number > 0, got %r" % (what, log_floor))
    geom = _jacobian_geom(flow, border, what)
    nd, B, D, H, W, border = geom
    flow = _c(flow.detach())
    out = torch.empty((B, 6), device=flow.device, dtype=torch.float64)
    check(lib().dfmir_jacdet_stats(nd, _p(flow), _p(_jacobian_ws(flow, geom)), _p(out), B, D, H, W, border, log_offset,
                                   float(log_floor), _st()))
    return out


def _invcons_geom(u, v, what):
    """(nd, B, D, H, W) of an inverse-consistency pair after the argument checks (nothing is launched on a bad one)."""
    if u.dim() not in (4, 5) or tuple(u.shape) != tuple(v.shape):
        raise DfmirHipError("%s: u %s / v %s mismatch (expected two [B,nd,*vol] fields of one shape)"
                            % (what, tuple(u.shape), tuple(v.shape)))
    nd = u.dim() - 2
    if u.shape[1] != nd:
        raise DfmirHipError("%s: a %d-D field needs %d channels, got %s" % (what, nd, nd, tuple(u.shape)))
    if u.dtype != torch.float32 or v.dtype != torch.float32:
        raise DfmirHipError("%s: fp32 tensors only (got %s, %s)" % (what, u.dtype, v.dtype))
    if u.device != v.device:
        raise DfmirHipError("%s: u on %s, v on %s" % (what, u.device, v.device))
    _need(u, v)
    B = int(u.shape[0])
    D, H, W = (int(n) for n in (u.shape[2:] if nd == 3 else (1,) + tuple(u.shape[2:])))
    if lib().dfmir_invcons_ws_floats(nd, B, D, H, W) < 0:
        raise DfmirHipError("%s: needs B >= 1, every extent >= 2 and fewer than 2^31 elements, got %s"
                            % (what, tuple(u.shape)))
    return nd, B, D, H, W


def _invcons_fwd(u, v, geom):
    """[B + 2] floats: IC per sample, their mean, max |r_c| (the backward's fixed-point range)."""
    nd, B, D, H, W = geom
    ws = torch.empty(int(lib().dfmir_invcons_ws_floats(nd, B, D, H, W)), device=u.device, dtype=torch.float32)
    out = torch.empty(B + 2, device=u.device, dtype=torch.float32)
    check(lib().dfmir_invcons_fwd(nd, _p(u), _p(v), _p(ws), _p(out), _p(out[B:]), _p(out[B + 1:]), B, D, H, W, _st()))
    return out


class InverseConsistencyFn(Function):
    """dfmir_invcons_fwd / _bwd: the forward keeps the two fields and max |r_c|, the backward recomputes r."""

    @staticmethod
    def forward(ctx, u, v, geom):
        u, v = _c(u), _c(v)
        out = _invcons_fwd(u, v, geom)
        ctx.save_for_backward(u, v, out)
        ctx.meta = geom
        return out[geom[1]].clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        u, v, out = ctx.saved_tensors
        nd, B, D, H, W = ctx.meta
        g = _c(g)
        du = torch.empty_like(u) if ctx.needs_input_grad[0] else None
        dv = ws = None
        if ctx.needs_input_grad[1]:
            dv = torch.empty_like(v)
            ws = torch.empty(int(lib().dfmir_invcons_bwd_ws_floats(nd, B, D, H, W)), device=u.device, dtype=torch.float32)
        if du is not None or dv is not None:
            check(lib().dfmir_invcons_bwd(nd, _p(u), _p(v), _p(g), _p(out[B + 1:]), _p(du), _p(dv), _p(ws), B, D, H, W,
                                          _st()))
        return du, dv, None


def inverse_consistency(u, v, symmetric=False):
    """Inverse-consistency loss of two displacement fields [B,nd,*vol] (nd = 2 or 3, fp32; build-defined, the definition:
    losses.InverseConsistency_Loss): IC(u, v) = the mean over all B * nd * S elements of r^2, r = u + ops.warp(v, u)
    element for element (v sampled (bi/tri)linearly at x + u(x), corners outside the volume read as 0).  symmetric=True:
    0.5 * (IC(u, v) + IC(v, u)), two calls of the same kernels.  One fused forward and one backward per direction; r is
    never stored.  Gradients to both fields, the exact adjoint.  The value and du are bit-identical from run to run on
    every shape.  dv is bit-identical from run to run wherever ops.warp's backward is -- W % 4 == 0: the same owner-gather
    adjoint, all but voxels displaced past the neighbouring tiles -- and, unlike it, on every other shape too (W % 4 != 0
    or a misaligned view: 64-bit fixed-point sums, several times slower; dfmir_amd/csrc/invcons.hip).  Raises before any launch on fields of
    different shapes, a channel count other than nd, a dtype other than fp32, an extent < 2 and 2^31 or more elements; a
    CPU tensor raises the usual "no CPU fallback" error."""
    geom = _invcons_geom(u, v, "inverse_consistency")
    loss = InverseConsistencyFn.apply(u, v, geom)
    if symmetric:
        loss = (loss + InverseConsistencyFn.apply(v, u, geom)) * 0.5
    return loss


@torch.no_grad()
def inverse_consistency_per_sample(u, v):
    """IC(u, v) per sample, a [B] tensor without gradient: the mean of r^2 over the nd * S elements of each sample (for
    evaluation; their mean is inverse_consistency(u, v))."""
    geom = _invcons_geom(u, v, "inverse_consistency_per_sample")
    return _invcons_fwd(_c(u), _c(v), geom)[:geom[1]].clone()


INVERT_MAX_ITERS = 64                        # INV_MAX_ITERS of dfmir_amd/csrc/compose.hip: one LDS slot per iteration


def _flow_geom(fields, what):
    """(nd, B, D, H, W) of one or more displacement fields [B,nd,*vol] of one shape after the argument checks (ValueError:
    nothing is launched on a bad one).  `fields`: (name, tensor) pairs."""
    name0, u = fields[0]
    for name, t in fields:
        if not torch.is_tensor(t):
            raise ValueError("%s: %s must be a [B,nd,*vol] tensor, got %s" % (what, name, type(t).__name__))
        if t.dim() not in (4, 5):
            raise ValueError("%s: %s must be a [B,2,H,W] or [B,3,D,H,W] field, got %s" % (what, name, tuple(t.shape)))
    nd = u.dim() - 2
    if u.shape[1] != nd:
        raise ValueError("%s: a %d-D field needs %d channels, got %s %s" % (what, nd, nd, name0, tuple(u.shape)))
    for name, t in fields[1:]:
        if tuple(t.shape) != tuple(u.shape):
            raise ValueError("%s: %s %s / %s %s mismatch (expected [B,nd,*vol] fields of one shape)"
                             % (what, name0, tuple(u.shape), name, tuple(t.shape)))
    if min(int(n) for n in u.shape[2:]) < 2:
        raise ValueError("%s: every extent must be >= 2, got %s" % (what, tuple(u.shape)))
    for name, t in fields:
        if t.dtype != torch.float32:
            raise DfmirHipError("%s: fp32 tensors only (%s is %s)" % (what, name, t.dtype))
        if t.device != u.device:
            raise DfmirHipError("%s: %s on %s, %s on %s" % (what, name0, u.device, name, t.device))
    _need(*[t for _, t in fields])
    B = int(u.shape[0])
    D, H, W = (int(n) for n in (u.shape[2:] if nd == 3 else (1,) + tuple(u.shape[2:])))
    if lib().dfmir_compose_bwd_ws_floats(nd, B, D, H, W) < 0:
        raise ValueError("%s: needs B >= 1 and fewer than 2^31 elements, got %s" % (what, tuple(u.shape)))
    return nd, B, D, H, W


class ComposeFlowsFn(Function):
    """dfmir_compose_fwd / _bwd: the forward keeps the two fields, the backward gathers v again."""

    @staticmethod
    def forward(ctx, u, v, geom):
        u, v = _c(u), _c(v)
        nd, B, D, H, W = geom
        out = torch.empty_like(u)
        check(lib().dfmir_compose_fwd(nd, _p(u), _p(v), _p(out), B, D, H, W, _st()))
        ctx.save_for_backward(u, v)
        ctx.meta = geom
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        u, v = ctx.saved_tensors
        nd, B, D, H, W = ctx.meta
        g = _c(g)
        du = torch.empty_like(u) if ctx.needs_input_grad[0] else None
        dv = ws = None
        if ctx.needs_input_grad[1]:                   # the dv pass is not launched for a v that needs no gradient
            dv = torch.empty_like(v)
            ws = torch.empty(int(lib().dfmir_compose_bwd_ws_floats(nd, B, D, H, W)), device=u.device, dtype=torch.float32)
        if du is not None or dv is not None:
            check(lib().dfmir_compose_bwd(nd, _p(u), _p(v), _p(g), _p(du), _p(dv), _p(ws), B, D, H, W, _st()))
        return du, dv, None


def compose_flows(u, v):
    """Composition of two displacement fields [B,nd,*vol] (nd = 2 or 3, fp32, in voxels, channel order (z,) y, x;
    build-defined): c(x) = u(x) + v(x + u(x)), v sampled (bi/tri)linearly at x + u(x) with corners outside the volume read
    as 0 -- ops.warp's convention, c = u + ops.warp(v, u) element for element in one launch and without the warped tensor.
    Then warp(src, c) is warp(warp(src, v), u) in the continuum: u is the warp applied LAST.  Differentiable in both:
    du_c = g_c + sum_c' g_c' d_c v_c'(x + u) (d_c: corner differences, padded corners as zeros), dv = the transpose of the
    interpolation applied to g; a gradient is computed only for the input that needs one.  The value and du are
    bit-identical from run to run on every shape, dv exactly where ops.inverse_consistency's is (W % 4 == 0 and aligned:
    the owner-gather adjoint of ops.warp's backward; elsewhere 64-bit fixed-point sums, slower; dfmir_amd/csrc/compose.hip).
    Non-contiguous inputs are copied, misaligned ones take the scalar launch.  ValueError before any launch on a non-tensor,
    a rank other than 4 or 5, a channel count other than nd, shapes that disagree, an extent < 2 and 2^31 or more elements; a
    CPU tensor raises the usual "no CPU fallback" error."""
    geom = _flow_geom((("u", u), ("v", v)), "compose_flows")
    return ComposeFlowsFn.apply(u, v, geom)


@torch.no_grad()
def invert_flow(u, iters=20, tol=0.0, init=None, history=False):
    """Fixed-point inverse of a displacement field [B,nd,*vol] (fp32, in voxels; build-defined): the w with
    compose_flows(w, u) = 0, i.e. warp(warp(src, u), w) = src in the continuum.  From w_0 = `init` (None = zeros):

        r_k(x)  = w_k(x) + u(x + w_k(x))         = compose_flows(w_k, u), the residual
        w_{k+1} = w_k - r_k                      = -u(x + w_k(x)) up to rounding

    for `iters` iterations (an int in [0, 64]); a voxel stops updating once max_c |r_k,c| <= tol (tol = 0, the default: every
    voxel does exactly `iters` updates).  Returns (w, stats): w = w_iters, and stats = a device tensor [B, 2] of (rms, max) of
    r_iters per sample -- rms = sqrt(sum |r|^2 / S), the RMS over the voxels of the vector length, the quantity
    infer.inverse_consistency_error reports; max = max |r_c| -- or, with history=True, [iters + 1, B, 2] for r_0 .. r_iters.
    iters = 0 returns `init` (or zeros) and the statistics of r_0.  All iterations run in ONE launch with w in registers
    (every voxel iterates on its own: it reads its own w and a gather of u); nothing syncs with the host, there is no
    autograd through it, and w and stats are bit-identical from run to run.

    Where it stands: the iteration converges where u is a contraction (Lipschitz constant < 1, i.e. |grad u| < 1: any
    diffeomorphic field of moderate strain).  At the volume border the zero padding makes u drop to 0 within one cell, so a
    field that is not small at the border does not converge there -- read the returned residual.  ValueError before any
    launch as compose_flows, and on iters not an int in [0, 64] and a negative or non-finite tol."""
    fields = (("u", u),) if init is None else (("u", u), ("init", init))
    what = "invert_flow"
    for name, t in fields:                            # the tensor checks that need no library call come before the scalars'
        if not torch.is_tensor(t):
            raise ValueError("%s: %s must be a [B,nd,*vol] tensor, got %s" % (what, name, type(t).__name__))
    if isinstance(iters, bool) or not isinstance(iters, int) or not 0 <= iters <= INVERT_MAX_ITERS:
        raise ValueError("%s: iters must be an integer in [0, %d], got %r" % (what, INVERT_MAX_ITERS, iters))
    try:
        tol = float(tol)
    except (TypeError, ValueError):
        raise ValueError("%s: tol must be a finite number >= 0, got %r" % (what, tol))
    if not 0.0 <= tol < float('inf'):
        raise ValueError("%s: tol must be a finite number >= 0, got %r" % (what, tol))
    nd, B, D, H, W = _flow_geom(fields, what)
    u = _c(u.detach())
    init = None if init is None else _c(init.detach())
    hist = 1 if history else 0
    w = torch.empty_like(u)
    stats = torch.empty((iters + 1, B, 2) if history else (B, 2), device=u.device, dtype=torch.float32)
    ws = torch.empty(int(lib().dfmir_flow_invert_ws_floats(nd, B, D, H, W, iters, hist)), device=u.device, dtype=torch.float32)
    check(lib().dfmir_flow_invert(nd, _p(u), _p(init), _p(w), _p(stats), _p(ws), B, D, H, W, iters, tol, hist, _st()))
    return w, stats


WARP_SSD_MAX_C = 16

# What ops.pack_features returns: `packed` [B,*vol,Cp] voxel-major (Cp = C rounded up to 4, zeros in the padding channels),
# `planar` the contiguous [B,C,*vol] tensor it was made from (the DFMIR_WARPSSD_PLANAR gather reads it), `shape` = planar's.
PackedFeatures = collections.namedtuple("PackedFeatures", "packed planar shape")


def _features_geom(M, what, name="mov"):
    """(nd, B, C, D, H, W) of a [B,C,*vol] feature tensor after the argument checks (ValueError: nothing is launched)."""
    if not torch.is_tensor(M) or M.dim() not in (4, 5):
        raise ValueError("%s: %s must be a [B,C,H,W] or [B,C,D,H,W] tensor, got %s"
                         % (what, name, tuple(M.shape) if torch.is_tensor(M) else type(M).__name__))
    nd = M.dim() - 2
    B, C = int(M.shape[0]), int(M.shape[1])
    if not 1 <= C <= WARP_SSD_MAX_C:
        raise ValueError("%s: %s needs 1 to %d channels, got %d" % (what, name, WARP_SSD_MAX_C, C))
    D, H, W = (int(n) for n in (M.shape[2:] if nd == 3 else (1,) + tuple(M.shape[2:])))
    if B < 1 or min(M.shape[2:]) < 2:
        raise ValueError("%s: %s needs B >= 1 and every extent >= 2, got %s" % (what, name, tuple(M.shape)))
    if M.dtype != torch.float32:
        raise ValueError("%s: fp32 tensors only (%s is %s)" % (what, name, M.dtype))
    if B * ((C + 3) // 4 * 4) * D * H * W >= 2 ** 31 or B * nd * D * H * W >= 2 ** 31:
        raise ValueError("%s: %s %s has 2^31 or more elements (packed)" % (what, name, tuple(M.shape)))
    if M.requires_grad:
        raise ValueError("%s: %s requires grad, but the op has no gradient to the features (detach it)" % (what, name))
    return nd, B, C, D, H, W


def pack_features(M):
    """The moving-side features of ops.warp_ssd laid out for its gather: M [B,C,*vol] (fp32, 1 <= C <= 16, 2-D or 3-D) ->
    PackedFeatures(packed [B,*vol,Cp], planar, shape), Cp = C rounded up to 4.  Made once for as many warp_ssd calls as the
    features live (a refinement loop).  ValueError on a bad rank, channel count, extent < 2, dtype, 2^31 or more elements
    or a tensor that requires grad; a CPU tensor raises the usual "no CPU fallback" error."""
    nd, B, C, D, H, W = _features_geom(M, "pack_features", "M")
    _need(M)
    M = _c(M)
    packed = torch.empty((B,) + tuple(M.shape[2:]) + ((C + 3) // 4 * 4,), device=M.device, dtype=torch.float32)
    check(lib().dfmir_warp_ssd_pack(nd, _p(M), _p(packed), B, C, D, H, W, _st()))
    return PackedFeatures(packed, M, tuple(M.shape))


def _ssd_features_args(mov, fix, what):
    """(packed, shape, geom) of the feature pair of a warp_ssd / affine_ssd call after its checks (ValueError: nothing is
    launched): `mov` a [B,C,*vol] tensor or a handle of ops.pack_features, `fix` a tensor of the same shape."""
    packed = isinstance(mov, PackedFeatures)
    if packed:
        shape = tuple(mov.shape)
        geom = _features_geom(mov.planar, what)
        if tuple(mov.planar.shape) != shape or tuple(mov.packed.shape) != (shape[0],) + shape[2:] + ((shape[1] + 3) // 4 * 4,):
            raise ValueError("%s: mov is not a handle ops.pack_features made" % what)
    else:
        geom = _features_geom(mov, what)
        shape = tuple(mov.shape)
    if not torch.is_tensor(fix) or tuple(fix.shape) != shape:
        raise ValueError("%s: mov %s / fix %s differ in shape" % (what, shape, tuple(fix.shape) if torch.is_tensor(fix) else fix))
    _features_geom(fix, what, "fix")
    return packed, shape, geom


def _warp_ssd_args(mov, fix, flow, mask, what):
    """(geom, handle, fix, flow, mask [B,1,*vol] or None) of a warp_ssd call after the argument checks; a [B,C,*vol] `mov`
    is packed here.  Everything a CPU tensor can get wrong raises ValueError before the device is asked for."""
    packed, shape, geom = _ssd_features_args(mov, fix, what)
    nd, B = geom[0], geom[1]
    if not torch.is_tensor(flow) or tuple(flow.shape) != (B, nd) + shape[2:]:
        raise ValueError("%s: the flow of %s features is [B,%d,*vol] = %s, got %s"
                         % (what, shape, nd, (B, nd) + shape[2:], tuple(flow.shape) if torch.is_tensor(flow) else flow))
    if flow.dtype != torch.float32:
        raise ValueError("%s: fp32 tensors only (flow is %s)" % (what, flow.dtype))
    return _ssd_pair_args(mov, packed, fix, flow, mask, shape, geom, what)


def _ssd_pair_args(mov, packed, fix, flow, mask, shape, geom, what):
    """The part of _warp_ssd_args that does not look at the flow beyond its device; `flow` may be any device tensor that says
    where the call runs (ops.affine_ssd passes its theta)."""
    B = geom[1]
    if mask is not None:
        if not torch.is_tensor(mask):
            raise ValueError("%s: mask must be a tensor" % what)
        if mask.requires_grad:
            raise ValueError("%s: mask requires grad, but the op has no gradient to the mask (detach it)" % what)
        try:
            mask = mask.expand((B, 1) + shape[2:])
        except RuntimeError:
            raise ValueError("%s: mask %s does not broadcast to %s" % (what, tuple(mask.shape), (B, 1) + shape[2:]))
    _need(mov.packed if packed else mov, fix, flow)
    if mask is not None:
        mask = mask.to(device=flow.device, dtype=torch.float32).contiguous()
    return geom, (mov if packed else pack_features(mov)), _c(fix), _c(flow), mask


def _warp_ssd_launch(geom, h, fix, flow, mask, unit):
    """[B + 2] floats: L_b per sample, L, and the factor the unit gradient is still to be multiplied with."""
    nd, B, C, D, H, W = geom
    ws = torch.empty(int(lib().dfmir_warp_ssd_ws_floats(nd, B, C, D, H, W)), device=flow.device, dtype=torch.float32)
    out = torch.empty(B + 2, device=flow.device, dtype=torch.float32)
    if unit is None:
        check(lib().dfmir_warp_ssd_fwd(nd, _p(h.packed), _p(h.planar), _p(fix), _p(flow), _p(mask), _p(ws), _p(out),
                                       _p(out[B:]), _p(out[B + 1:]), B, C, D, H, W, _st()))
    else:
        check(lib().dfmir_warp_ssd_fwd_grad(nd, _p(h.packed), _p(h.planar), _p(fix), _p(flow), _p(mask), _p(ws), _p(out),
                                            _p(out[B:]), _p(out[B + 1:]), _p(unit), B, C, D, H, W, _st()))
    return out


class WarpSSDFn(Function):
    """dfmir_warp_ssd_fwd_grad / _bwd: the forward's one pass leaves the unit gradient, the backward scales it by gout."""

    @staticmethod
    def forward(ctx, flow, geom, h, fix, mask):
        unit = torch.empty_like(flow) if ctx.needs_input_grad[0] else None
        out = _warp_ssd_launch(geom, h, fix, flow, mask, unit)
        if unit is not None:
            ctx.save_for_backward(unit, out)
        ctx.B = geom[1]
        return out[geom[1]].clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        unit, out = ctx.saved_tensors
        dflow = torch.empty_like(unit)
        check(lib().dfmir_warp_ssd_bwd(_p(unit), _p(_c(g)), _p(out[ctx.B + 1:]), _p(dflow), unit.numel(), _st()))
        return dflow, None, None, None, None


def warp_ssd(mov, fix, flow, mask=None):
    """The SSD between fixed-image features and warped moving-image features, the data term of instance optimisation
    (build-defined; the definition: losses.WarpedSSD_Loss): the mean over (B, C, voxels) of (mov_c(x + flow(x)) - fix_c(x))^2,
    or with `mask` (float weights that broadcast to [B,1,*vol]) sum mask * mean_c (.)^2 / sum mask -- 0 for an empty mask, as
    a device scalar without a host sync.  mov: [B,C,*vol] (packed per call) or the handle of ops.pack_features(mov); fix:
    [B,C,*vol]; flow: [B,nd,*vol] in voxels, ops.warp's convention.  One fused pass, no warped tensor; the gradient goes to
    the flow ONLY: a `mov`, `fix` or `mask` that requires grad raises.  Bit-identical from run to run.  ValueError before
    any launch on a bad rank, C outside 1..16, shapes that disagree, a dtype other than fp32, an extent < 2 and 2^31 or
    more elements; a CPU tensor raises the usual "no CPU fallback" error."""
    geom, h, fix, flow_c, mask = _warp_ssd_args(mov, fix, flow, mask, "warp_ssd")
    return WarpSSDFn.apply(flow_c, geom, h, fix, mask)


@torch.no_grad()
def warp_ssd_per_sample(mov, fix, flow, mask=None):
    """warp_ssd per sample, a [B] tensor without gradient: sample b's own (masked) mean, 0 where its mask is empty."""
    geom, h, fix, flow_c, mask = _warp_ssd_args(mov, fix, flow, mask, "warp_ssd_per_sample")
    return _warp_ssd_launch(geom, h, fix, flow_c, mask, None)[:geom[1]].clone()


def affine_identity(B, nd, device):
    """The identity transform [B,nd,nd+1] fp32 = [I | 0] on `device` (the convention: ops.affine_flow)."""
    if isinstance(B, bool) or not isinstance(B, int) or B < 1 or nd not in (2, 3):
        raise ValueError("affine_identity: B must be an integer >= 1 and nd 2 or 3, got B = %r, nd = %r" % (B, nd))
    return torch.eye(nd, nd + 1, dtype=torch.float32, device=device).repeat(B, 1, 1)


def _affine_theta(theta, B, nd, what):
    """theta [B,nd,nd+1] fp32 of an affine op after the argument checks (ValueError: nothing is launched)."""
    if not torch.is_tensor(theta) or tuple(theta.shape) != (B, nd, nd + 1):
        raise ValueError("%s: theta must be [B,%d,%d] = %s, got %s"
                         % (what, nd, nd + 1, (B, nd, nd + 1), tuple(theta.shape) if torch.is_tensor(theta) else theta))
    if theta.dtype != torch.float32:
        raise ValueError("%s: fp32 tensors only (theta is %s)" % (what, theta.dtype))


def _affine_vol(vol, B, what):
    """(nd, D, H, W) of the volume an affine flow is made for."""
    try:
        vol = tuple(vol)
    except TypeError:
        raise ValueError("%s: vol must be 2 or 3 extents, got %r" % (what, vol)) from None
    if len(vol) not in (2, 3) or any(isinstance(n, bool) or not isinstance(n, int) or n < 2 for n in vol):
        raise ValueError("%s: vol must be 2 or 3 integer extents >= 2, got %r" % (what, vol))
    nd = len(vol)
    D, H, W = vol if nd == 3 else (1,) + vol
    if B * 4 * D * H * W >= 2 ** 31:
        raise ValueError("%s: a flow [%d,%d,*%s] is too large (2^31 or more elements with four channels)" % (what, B, nd, vol))
    return nd, D, H, W


class AffineFlowFn(Function):
    """dfmir_affine_flow / _flow_bwd."""

    @staticmethod
    def forward(ctx, theta, geom):
        nd, B, D, H, W = geom
        flow = torch.empty((B, nd) + ((D, H, W) if nd == 3 else (H, W)), device=theta.device, dtype=torch.float32)
        check(lib().dfmir_affine_flow(nd, _p(theta), _p(flow), B, D, H, W, _st()))
        ctx.geom = geom
        return flow

    @staticmethod
    @once_differentiable
    def backward(ctx, dflow):
        nd, B, D, H, W = ctx.geom
        dflow = _c(dflow)
        ws = torch.empty(int(lib().dfmir_affine_ws_floats(nd, B, D, H, W)), device=dflow.device, dtype=torch.float32)
        dtheta = torch.empty((B, nd, nd + 1), device=dflow.device, dtype=torch.float32)
        check(lib().dfmir_affine_flow_bwd(nd, _p(dflow), _p(ws), _p(dtheta), B, D, H, W, _st()))
        return dtheta, None


def affine_flow(theta, vol):
    """The dense displacement field of an affine transform (build-defined): theta [B,nd,nd+1] fp32 = [A | t] in CENTRED voxel
    coordinates, axis order (z,) y, x; vol = the nd extents.  With c_a = (n_a - 1) / 2 and q(x) = (x - c, 1):

        y(x) = c + A (x - c) + t         flow[b,a,x] = y_a(x) - x_a = sum_j (A - I)_aj (x - c)_j + t_a        [B,nd,*vol]

    in ops.warp's convention, so ops.warp(moving, flow), ops.compose_flows, ops.warp_dice and the landmark ops take it as it
    is.  Identity is [I | 0] (ops.affine_identity).  Centring makes A the same matrix on every pooled level of a volume (only
    t scales) and keeps the normal matrix of a fit conditioned.  Differentiable in theta: dtheta[b,a,j] = sum_x dflow[b,a,x]
    q_j(x), added in double in two fixed-order stages without atomics -- bit-identical from run to run.  ValueError before any
    launch on a theta that is not [B,nd,nd+1] fp32, extents that are not integers >= 2 and 2^31 or more elements; a CPU tensor
    raises the usual "no CPU fallback" error."""
    what = "affine_flow"
    if not torch.is_tensor(theta) or theta.dim() != 3 or int(theta.shape[0]) < 1:
        raise ValueError("%s: theta must be a [B,nd,nd+1] tensor, got %s"
                         % (what, tuple(theta.shape) if torch.is_tensor(theta) else type(theta).__name__))
    B = int(theta.shape[0])
    nd, D, H, W = _affine_vol(vol, B, what)
    _affine_theta(theta, B, nd, what)
    _need(theta)
    return AffineFlowFn.apply(_c(theta), (nd, B, D, H, W))


def _affine_ssd_args(mov, fix, theta, mask, what):
    """(geom, handle, fix, theta, mask) of an affine_ssd / affine_ssd_system call after the argument checks: warp_ssd's own
    for the features and the mask, and theta's, which stands where warp_ssd's flow does."""
    if not isinstance(mov, PackedFeatures) and not torch.is_tensor(mov):
        raise ValueError("%s: mov must be a [B,C,*vol] tensor or a handle of ops.pack_features" % what)
    packed, shape, geom = _ssd_features_args(mov, fix, what)
    _affine_theta(theta, geom[1], geom[0], what)
    return _ssd_pair_args(mov, packed, fix, theta, mask, shape, geom, what)


def _affine_system_launch(geom, h, fix, theta, mask, full):
    """dfmir_affine_system: the double buffer [L, L_b [B], gb [B,P], g [B,P] (, H [B,P,P])]."""
    nd, B, C, D, H, W = geom
    P = nd * (nd + 1)
    ws = torch.empty(int(lib().dfmir_affine_ws_floats(nd, B, D, H, W)), device=theta.device, dtype=torch.float32)
    out = torch.empty(1 + B + 2 * B * P + (B * P * P if full else 0), device=theta.device, dtype=torch.float64)
    check(lib().dfmir_affine_system(nd, _p(h.packed), _p(fix), _p(theta), _p(mask), _p(ws), _p(out), 1 if full else 0,
                                    B, C, D, H, W, _st()))
    return out


class AffineSSDFn(Function):
    """dfmir_affine_system in gradient-only mode: the forward's one pass leaves dL/dtheta, the backward scales it by gout."""

    @staticmethod
    def forward(ctx, theta, geom, h, fix, mask):
        nd, B = geom[0], geom[1]
        out = _affine_system_launch(geom, h, fix, theta, mask, False)
        ctx.save_for_backward(out[1 + B:1 + B + B * nd * (nd + 1)])
        ctx.shape = (B, nd, nd + 1)
        return out[0].to(torch.float32)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (gb,) = ctx.saved_tensors
        return (gb * g.to(torch.float64)).to(torch.float32).reshape(ctx.shape), None, None, None, None


def affine_ssd(mov, fix, theta, mask=None):
    """The SSD between fixed-image features and moving-image features under an affine transform (build-defined; the
    definition: losses.AffineSSD_Loss): by definition ops.warp_ssd(mov, fix, ops.affine_flow(theta, vol), mask) -- the same
    mean over (B, C, voxels), the same masked form sum m mean_c e^2 / sum m, 0 for an empty mask -- as a device scalar, from
    ONE fused pass that reads no flow and writes no per-voxel gradient (dfmir_amd/csrc/affine.hip: the moving features are
    sampled in the cell warp_ssd selects, with its guards).  mov: [B,C,*vol] (packed per call) or the handle of
    ops.pack_features(mov), 1 <= C <= 16; fix: [B,C,*vol]; theta: [B,nd,nd+1] fp32, ops.affine_flow's convention.  The
    gradient goes to theta ONLY (sums in double, a fixed order: bit-identical from run to run); a `mov`, `fix` or `mask`
    that requires grad raises.  ValueError before any launch on what ops.warp_ssd refuses and on a theta of the wrong shape
    or dtype; a CPU tensor raises the usual "no CPU fallback" error."""
    geom, h, fix, theta_c, mask = _affine_ssd_args(mov, fix, theta, mask, "affine_ssd")
    return AffineSSDFn.apply(theta_c, geom, h, fix, mask)


@torch.no_grad()
def affine_ssd_system(mov, fix, theta, mask=None):
    """The affine SSD per sample with its gradient and Gauss-Newton matrix (build-defined), arguments as ops.affine_ssd:
    (L_b [B], g [B,P], H [B,P,P]) as float64 device tensors without gradient, P = nd (nd + 1) parameters flattened row-major
    (a, j).  Per voxel, with y = y_theta(x) and q = (x - c, 1) (ops.affine_flow):

        e_c = M_c(y) - F_c      r = sum_c e_c dM_c(y)  (nd)      G = sum_c dM_c dM_c^T  (nd x nd)      N_b = sum_x m  (S unmasked)
        L_b = sum_x m mean_c e^2 / N_b
        g_b = (2 / (C N_b)) sum_x m r (x) q          = dL_b / dtheta_b exactly
        H_b = (2 / (C N_b)) sum_x m G (x) (q q^T)    the Gauss-Newton matrix of L_b, symmetric positive semi-definite

    all 0 for N_b = 0.  dM is the derivative of the interpolant in the cell floor() selects: corner differences, zero-padded
    corners taking part as zeros (warp_ssd's).  One pass over the voxels, sums in double in a fixed order."""
    geom, h, fix, theta_c, mask = _affine_ssd_args(mov, fix, theta, mask, "affine_ssd_system")
    nd, B = geom[0], geom[1]
    P = nd * (nd + 1)
    out = _affine_system_launch(geom, h, fix, theta_c, mask, True)
    o = 1 + B + B * P
    return out[1:1 + B].clone(), out[o:o + B * P].reshape(B, P).clone(), out[o + B * P:].reshape(B, P, P).clone()


def affine_lm_state(B, nd, mu0, device):
    """The state of ops.affine_lm_step at the start of a level: [B, 2 + P + P P] float64 = (L_acc = +inf, mu = mu0, g_acc = 0,
    H_acc = 0) per sample."""
    P = nd * (nd + 1)
    state = torch.empty((B, 2 + P + P * P), dtype=torch.float64, device=device)
    state[:, 0] = float('inf')
    state[:, 1] = float(mu0)
    state[:, 2:] = 0.0
    return state


@torch.no_grad()
def affine_lm_step(L, g, H, theta_acc, trial, state, hist, k, dof='affine', mu_up=10.0, mu_down=0.1):
    """One Levenberg-Marquardt step of infer.affine_init per sample, on the device and in place (dfmir_affine_lm_step): (L
    [B], g [B,P], H [B,P,P]) float64 = the system AT `trial`; theta_acc, trial [B,nd,nd+1] fp32; state from
    ops.affine_lm_state; hist [B,5] float64 receives (L, L_acc, mu, accepted, singular); k = the evaluation's index within
    its level.  L finite and L <= L_acc accepts the trial (and for k > 0 mu = max(mu mu_down, 1e-12)), anything else rejects it
    (mu = min(mu mu_up, 1e12)); then (H_acc[f,f] + mu diag H_acc[f,f]) d = -g_acc[f] over the free parameters (dof 'affine':
    all; 'translation': the t column) by Cholesky in fp64 -- a pivot <= 0 or not finite gives d = 0 and the singular flag --
    and trial = theta_acc + d.  Nothing syncs with the host."""
    what = "affine_lm_step"
    if dof not in ('affine', 'translation'):
        raise ValueError("%s: dof must be 'affine' or 'translation', got %r" % (what, dof))
    if not torch.is_tensor(theta_acc) or theta_acc.dim() != 3:
        raise ValueError("%s: theta_acc must be [B,nd,nd+1]" % what)
    B, nd = int(theta_acc.shape[0]), int(theta_acc.shape[1])
    if nd not in (2, 3):
        raise ValueError("%s: theta_acc must be [B,nd,nd+1] with nd 2 or 3, got %s" % (what, tuple(theta_acc.shape)))
    P = nd * (nd + 1)
    _affine_theta(theta_acc, B, nd, what)
    _affine_theta(trial, B, nd, what)
    for t, shape, name in ((L, (B,), "L"), (g, (B, P), "g"), (H, (B, P, P), "H"), (state, (B, 2 + P + P * P), "state"),
                           (hist, (B, 5), "hist")):
        if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != torch.float64:
            raise ValueError("%s: %s must be a float64 tensor %s" % (what, name, shape))
    if isinstance(k, bool) or not isinstance(k, int) or k < 0:
        raise ValueError("%s: k must be an integer >= 0, got %r" % (what, k))
    if not (mu_up > 1.0 and 0.0 < mu_down <= 1.0 and mu_up < float('inf')):
        raise ValueError("%s: mu_up must be finite and > 1, mu_down in (0, 1], got %r, %r" % (what, mu_up, mu_down))
    for t in (L, g, H, theta_acc, trial, state, hist):
        if not t.is_cuda:
            raise DfmirHipError("dfmir_amd ops run only on the HIP device (got a %s tensor); there is no CPU fallback" % t.device)
        if not t.is_contiguous():
            raise ValueError("%s: contiguous tensors only (the step works in place)" % what)
    check(lib().dfmir_affine_lm_step(nd, _p(L), _p(g), _p(H), _p(theta_acc), _p(trial), _p(state), _p(hist), B, k,
                                     1 if dof == 'translation' else 0, float(mu_up), float(mu_down), _st()))


DSEARCH_MAX_RADIUS = {2: 8, 3: 4}           # dfmir_amd/csrc/dsearch.hip: what the cost kernel's staged window is sized for
# dfmir_amd/csrc/keypoints.hip (the DFMIR_KEYPOINT_* of include/dfmir_hip.h): the limits of ops.local_maxima, ops.keypoint_cost
# and ops.keypoint_argmin.  KEYPOINT_MAX_EXTENT bounds the staged extent E = 2 (radius step + patch) + 1 of the search region:
# one plane of E^2 floats beside the largest fixed patch in 64 KB of LDS.
KEYPOINT_NMS_MAX_RADIUS = 8
KEYPOINT_MAX_RADIUS = {2: 16, 3: 8}
KEYPOINT_MAX_STEP = 4
KEYPOINT_MAX_PATCH = 3
KEYPOINT_MAX_EXTENT = 96


def _dsearch_radius(radius, nd, what):
    if isinstance(radius, bool) or not isinstance(radius, int) or not 1 <= radius <= DSEARCH_MAX_RADIUS[nd]:
        raise ValueError("%s: radius must be an integer in [1, %d] for %d-D features, got %r"
                         % (what, DSEARCH_MAX_RADIUS[nd], nd, radius))
    return radius


def _dsearch_pool(M, geom, g, planar, packed):
    """dfmir_dsearch_pool of a checked [B,C,*vol] tensor: (planar [B,C,*(vol // g)] or None, packed [B,*(vol // g),Cp] or
    None)."""
    nd, B, C, D, H, W = geom
    _need(M)
    M = _c(M)
    sp = tuple(int(n) // g for n in M.shape[2:])
    out = torch.empty((B, C) + sp, device=M.device, dtype=torch.float32) if planar else None
    pk = torch.empty((B,) + sp + ((C + 3) // 4 * 4,), device=M.device, dtype=torch.float32) if packed else None
    check(lib().dfmir_dsearch_pool(nd, _p(M), _p(out), _p(pk), B, C, D, H, W, g, _st()))
    return out, pk


@torch.no_grad()
def pool_features(M, g):
    """Average pooling of features onto a search grid (build-defined): M [B,C,*vol] (fp32, 1 <= C <= 16, 2-D or 3-D) ->
    [B,C,*(vol // g)], out[b,c,X] = the mean of M[b,c,g X + {0 .. g-1}^nd] -- window g^nd, stride g, the remainder at the far
    faces dropped (F.avg_pool with kernel = stride = g).  Coarse sample i therefore sits at fine coordinate g i + (g - 1) / 2.
    The window is added in double in a fixed order and rounded once; g = 1 copies.  No gradient.  ValueError before any launch
    on a g that is not an integer >= 1, a pooled extent < 2, and what ops.pack_features refuses (rank, C outside 1..16, dtype,
    2^31 or more elements, a tensor that requires grad); a CPU tensor raises the usual "no CPU fallback" error."""
    what = "pool_features"
    geom = _features_geom(M, what, "M")
    if isinstance(g, bool) or not isinstance(g, int) or g < 1:
        raise ValueError("%s: g must be an integer >= 1, got %r" % (what, g))
    if min(int(n) // g for n in M.shape[2:]) < 2:
        raise ValueError("%s: every pooled extent must be >= 2, got %s // %d" % (what, tuple(M.shape[2:]), g))
    return _dsearch_pool(M, geom, g, True, False)[0]


@torch.no_grad()
def ssd_cost_volume(fix, mov, radius):
    """The SSD cost volume of a discrete displacement search (build-defined): fix, mov [B,C,*vol] features that already live
    on the search grid (fp32, 1 <= C <= 16, 2-D or 3-D, one shape) -> cost [B,K,*vol], K = (2 radius + 1)^nd,

        cost[b,k,x] = (1/C) sum_c (fix[b,c,x] - mov[b,c,x + d_k])^2         mov reads 0 outside the volume (ops.warp's padding)

    where k enumerates the displacements d_k in {-radius .. radius}^nd in row-major order (dz,) dy, dx with -radius first; d_k
    is in voxels of this grid and in the flow's channel order, so the minimiser is a flow in ops.warp's convention.  The
    channels are added in one order for every k: displacements whose sample lies outside the volume tie bit for bit.  Both
    sides are packed voxel-major once, then one launch writes every cost once (dfmir_amd/csrc/dsearch.hip); bit-identical
    from run to run.  No gradient: an input that requires grad raises.  ValueError before any launch on shapes that
    disagree, a radius that is not an integer in 1..DSEARCH_MAX_RADIUS[nd] (8 in 2-D, 4 in 3-D), B K S >= 2^31, B > 65535 and what
    ops.pack_features refuses; a CPU tensor raises the usual "no CPU fallback" error."""
    what = "ssd_cost_volume"
    geom = _features_geom(fix, what, "fix")
    if not torch.is_tensor(mov) or tuple(mov.shape) != tuple(fix.shape):
        raise ValueError("%s: fix %s / mov %s differ in shape"
                         % (what, tuple(fix.shape), tuple(mov.shape) if torch.is_tensor(mov) else mov))
    _features_geom(mov, what, "mov")
    nd, B, C, D, H, W = geom
    r = _dsearch_radius(radius, nd, what)
    K = (2 * r + 1) ** nd
    if B * K * D * H * W >= 2 ** 31:
        raise ValueError("%s: the cost volume [%d,%d,*%s] has 2^31 or more elements" % (what, B, K, tuple(fix.shape[2:])))
    if B > 65535:
        raise ValueError("%s: B must be <= 65535, got %s" % (what, tuple(fix.shape)))
    if mov.device != fix.device:
        raise DfmirHipError("%s: fix on %s, mov on %s" % (what, fix.device, mov.device))
    fp = _dsearch_pool(fix, geom, 1, False, True)[1]
    mp = _dsearch_pool(mov, geom, 1, False, True)[1]
    cost = torch.empty((B, K) + tuple(fix.shape[2:]), device=fix.device, dtype=torch.float32)
    check(lib().dfmir_dsearch_cost(nd, _p(fp), _p(mp), _p(cost), B, C, D, H, W, r, _st()))
    return cost


def _dsearch_field(t, what, name, chan=None):
    """(nd, B, D, H, W) of a [B,chan,*vol] fp32 tensor (chan None: nd channels) after the checks a CPU tensor can fail."""
    if not torch.is_tensor(t) or t.dim() not in (4, 5):
        raise ValueError("%s: %s must be a [B,.,H,W] or [B,.,D,H,W] tensor, got %s"
                         % (what, name, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
    nd = t.dim() - 2
    if t.shape[1] != (nd if chan is None else chan(nd)):
        raise ValueError("%s: %s %s must have %d channels" % (what, name, tuple(t.shape), nd if chan is None else chan(nd)))
    if t.shape[0] < 1 or min(t.shape[2:]) < 2:
        raise ValueError("%s: %s needs B >= 1 and every extent >= 2, got %s" % (what, name, tuple(t.shape)))
    if t.dtype != torch.float32:
        raise ValueError("%s: fp32 tensors only (%s is %s)" % (what, name, t.dtype))
    if t.numel() >= 2 ** 31:
        raise ValueError("%s: %s %s has 2^31 or more elements" % (what, name, tuple(t.shape)))
    if t.requires_grad:
        raise ValueError("%s: %s requires grad, but the op has no gradient (detach it)" % (what, name))
    D, H, W = (int(n) for n in (t.shape[2:] if nd == 3 else (1,) + tuple(t.shape[2:])))
    return nd, int(t.shape[0]), D, H, W


@torch.no_grad()
def cost_argmin(cost, radius, soft=None, coeff=0.0):
    """The coupled argmin of a displacement cost volume (build-defined) -> (idx int32 [B,*vol], disp fp32 [B,nd,*vol]):

        idx[b,x] = argmin_k ( cost[b,k,x] + coeff * sum_a (d_k[a] - soft[b,a,x])^2 ),        disp[b,a,x] = d_idx[a]

    cost: [B,K,*vol] as ops.ssd_cost_volume lays it out, K = (2 radius + 1)^nd; soft: a field [B,nd,*vol] in voxels, None =
    the plain argmin (coeff is then not read); coeff: a finite float >= 0.  The LOWEST k wins a tie (a strict < walking k
    upwards); a NaN is never selected, and where every value is NaN the result is index 0.  One thread per voxel reads the
    cost volume once.  ValueError before any launch on a radius outside 1..DSEARCH_MAX_RADIUS[nd], a channel count other than
    K, a soft of another shape, a coeff that is negative or not finite, 2^31 or more elements, a dtype other than fp32 and a
    tensor that requires grad; a CPU tensor raises the usual "no CPU fallback" error."""
    what = "cost_argmin"
    if not torch.is_tensor(cost) or cost.dim() not in (4, 5):
        raise ValueError("%s: cost must be a [B,K,H,W] or [B,K,D,H,W] tensor, got %s"
                         % (what, tuple(cost.shape) if torch.is_tensor(cost) else type(cost).__name__))
    r = _dsearch_radius(radius, cost.dim() - 2, what)
    nd, B, D, H, W = _dsearch_field(cost, what, "cost", chan=lambda n: (2 * r + 1) ** n)
    vol = tuple(cost.shape[2:])
    if soft is not None:
        if not torch.is_tensor(soft) or tuple(soft.shape) != (B, nd) + vol:
            raise ValueError("%s: soft must be [B,nd,*vol] = %s, got %s"
                             % (what, (B, nd) + vol, tuple(soft.shape) if torch.is_tensor(soft) else type(soft).__name__))
        _dsearch_field(soft, what, "soft")
    try:
        coeff = float(coeff)
    except (TypeError, ValueError):
        raise ValueError("%s: coeff must be a finite number >= 0, got %r" % (what, coeff))
    if not 0.0 <= coeff < float('inf'):
        raise ValueError("%s: coeff must be a finite number >= 0, got %r" % (what, coeff))
    _need(cost, soft)
    if soft is not None and soft.device != cost.device:
        raise DfmirHipError("%s: cost on %s, soft on %s" % (what, cost.device, soft.device))
    cost = _c(cost)
    soft = None if soft is None else _c(soft)
    idx = torch.empty((B,) + vol, device=cost.device, dtype=torch.int32)
    disp = torch.empty((B, nd) + vol, device=cost.device, dtype=torch.float32)
    check(lib().dfmir_dsearch_argmin(nd, _p(cost), _p(soft), coeff, _p(idx), _p(disp), B, D, H, W, r, _st()))
    return idx, disp


@torch.no_grad()
def box_smooth_flow(disp):
    """The 3^nd box mean of a field [B,nd,*vol] (fp32, 2-D or 3-D; build-defined): out[b,a,x] = the mean of disp[b,a,.] over
    those of the 3^nd neighbours of x (x included) that lie inside the volume -- the divisor is the in-volume count
    (F.avg_pool(3, stride 1, padding 1, count_include_pad=False)).  A stated divergence: the published coupled-convex code
    divides by 3^nd everywhere and so pulls the field towards zero at the faces; here a constant field comes back constant.
    No gradient.  ValueError before any launch on a rank other than 4 or 5, a channel count other than nd, an extent < 2, a
    dtype other than fp32, 2^31 or more elements and a tensor that requires grad; a CPU tensor raises the usual "no CPU
    fallback" error."""
    nd, B, D, H, W = _dsearch_field(disp, "box_smooth_flow", "disp")
    _need(disp)
    disp = _c(disp)
    out = torch.empty_like(disp)
    check(lib().dfmir_dsearch_smooth(nd, _p(disp), _p(out), B, D, H, W, _st()))
    return out


GAUSS_MAX_RADIUS = 16      # DFMIR_GAUSS_MAX_RADIUS (include/dfmir_hip.h): the halo dfmir_amd/csrc/gauss.hip sizes its LDS tile for


def gauss_radii(sigma, truncate, nd, what):
    """((sigma_a) per axis as floats, (r_a) per axis) of a gaussian_smooth call after the checks on `sigma` and `truncate`
    (ValueError: nothing is launched): r_a = ceil(truncate * sigma_a) <= GAUSS_MAX_RADIUS."""
    def number(v):
        return not isinstance(v, bool) and isinstance(v, (int, float)) and 0.0 <= v < float('inf')
    if number(sigma):
        sig = (float(sigma),) * nd
    else:
        try:
            sig = tuple(sigma)
        except TypeError:
            sig = None
        if sig is None or len(sig) != nd or not all(number(v) for v in sig):
            raise ValueError("%s: sigma must be a finite number >= 0 or %d of them, got %r" % (what, nd, sigma))
        sig = tuple(float(v) for v in sig)
    if isinstance(truncate, bool) or not isinstance(truncate, (int, float)) or not 0.0 < truncate < float('inf'):
        raise ValueError("%s: truncate must be a finite number > 0, got %r" % (what, truncate))
    radii = tuple(int(min(math.ceil(float(truncate) * s), GAUSS_MAX_RADIUS + 1)) for s in sig)
    if max(radii) > GAUSS_MAX_RADIUS:
        raise ValueError("%s: the radius ceil(truncate * sigma) must be <= GAUSS_MAX_RADIUS = %d, got sigma %r, truncate %r"
                         % (what, GAUSS_MAX_RADIUS, sigma, truncate))
    return sig, radii


@torch.no_grad()
def gaussian_smooth(x, sigma, truncate=3.0):
    """Gaussian smoothing of a field or a feature volume (build-defined): x [B,C,*vol] fp32, 2-D or 3-D, any C >= 1; sigma: a
    finite float >= 0 in voxels, or nd of them in axis order (z,) y, x; truncate: finite and > 0.  Per axis a,
    r_a = ceil(truncate * sigma_a) and w_a[k] = exp(-k^2 / (2 sigma_a^2)) for |k| <= r_a (formed in double, rounded to fp32);
    the filter is separable and RENORMALISED AT THE FACES,

        out(i) = sum_k w[k] in(i + k) [i + k inside] / sum_k w[k] [i + k inside]                  along each axis

    so a constant comes back constant -- ops.box_smooth_flow's convention, and the reason the filter is not zero padding.
    sigma_a == 0 leaves that axis alone, and with every sigma 0 the result equals the input bit for bit.  An extent smaller
    than the window is legal (the whole axis then lies inside every window); r_a <= GAUSS_MAX_RADIUS = 16, what the kernel's
    LDS tile is sized for.  2-D is one launch (tile and halo in LDS, both axes filtered there); 3-D is the (y, x) pass per
    plane and a z pass, two reads and two writes of the tensor (dfmir_amd/csrc/gauss.hip).  Bit-identical from run to run;
    nothing syncs with the host.  No gradient, in the manner of ops.box_smooth_flow: an input that requires grad raises.
    ValueError before any launch on a rank other than 4 or 5, C < 1, an extent < 2, a dtype other than fp32, 2^31 or more
    elements, a tensor that requires grad, a sigma that is negative, not finite or not 1 or nd numbers, a truncate that is
    not finite and > 0 and a radius above GAUSS_MAX_RADIUS; a CPU tensor raises the usual "no CPU fallback" error."""
    what = "gaussian_smooth"
    if not torch.is_tensor(x) or x.dim() not in (4, 5):
        raise ValueError("%s: x must be a [B,C,H,W] or [B,C,D,H,W] tensor, got %s"
                         % (what, tuple(x.shape) if torch.is_tensor(x) else type(x).__name__))
    nd = x.dim() - 2
    if x.shape[0] < 1 or x.shape[1] < 1 or min(x.shape[2:]) < 2:
        raise ValueError("%s: x needs B >= 1, C >= 1 and every extent >= 2, got %s" % (what, tuple(x.shape)))
    if x.dtype != torch.float32:
        raise ValueError("%s: fp32 tensors only (x is %s)" % (what, x.dtype))
    if x.numel() >= 2 ** 31:
        raise ValueError("%s: x %s has 2^31 or more elements" % (what, tuple(x.shape)))
    if x.requires_grad:
        raise ValueError("%s: x requires grad, but the op has no gradient (detach it)" % what)
    sig, radii = gauss_radii(sigma, truncate, nd, what)
    _need(x)
    x = _c(x)
    D, H, W = (int(n) for n in (x.shape[2:] if nd == 3 else (1,) + tuple(x.shape[2:])))
    sz, sy, sx = sig if nd == 3 else (0.0,) + sig
    out = torch.empty_like(x)
    two = nd == 3 and radii[0] > 0 and max(radii[1:]) > 0
    tmp = torch.empty_like(x) if two else None
    check(lib().dfmir_gauss_smooth(nd, _p(x), _p(out), _p(tmp), int(x.shape[0]) * int(x.shape[1]), D, H, W, sz, sy, sx,
                                   float(truncate), _st()))
    return out


@torch.no_grad()
def demons_force(mov, fix, flow, mask=None, max_step=2.0):
    """The demons force (build-defined): a per-voxel Gauss-Newton step on the feature SSD that ops.warp_ssd and
    ops.affine_ssd_system use.  mov: a [B,C,*vol] feature tensor (packed per call) or the handle of ops.pack_features(mov);
    fix, flow, mask: exactly as ops.warp_ssd takes them (1 <= C <= 16, 2-D or 3-D, flow [B,nd,*vol] in voxels, mask float
    weights that broadcast to [B,1,*vol]); max_step: finite and > 0, in voxels.  Per voxel x, with p = x + flow(x):

        m_c = M_c(p)        J_c = the derivative of the interpolant in the cell floor() selects: corner differences, padded
                            corners as zeros (warp_ssd's)                   e_c = m_c - F_c(x)
        s = (1/C) sum_c e_c^2          g = (1/C) sum_c e_c J_c  (nd)          H = (1/C) sum_c J_c J_c^T  (nd x nd)
        d(x) = -(H + (s / max_step^2) I)^-1 g

    With C = 1 this is Thirion's force with Vercauteren's step bound, -e J / (|J|^2 + e^2 / max_step^2); for any C
    |d(x)| <= max_step / 2.  Where g is exactly zero (that includes points with no corner inside the volume) d = +0 without a
    division; elsewhere the system is solved in closed form, and if a component is not finite the vector is 0.  A mask weight
    <= 0 gives d(x) = 0; a positive weight leaves d as it is and weights only the energy.  Returns (d [B,nd,*vol], L, L_b [B]):
    L and L_b are the (masked) mean of s with warp_ssd's reduction, as device tensors.  One fused gather pass, no warped
    tensor; everything is bit-identical from run to run; nothing syncs with the host.  No gradient: a `mov`, `fix`, `flow` or
    `mask` that requires grad raises.  ValueError before any launch on what ops.warp_ssd refuses and on a max_step that is
    not finite and > 0; a CPU tensor raises the usual "no CPU fallback" error."""
    what = "demons_force"
    if isinstance(max_step, bool) or not isinstance(max_step, (int, float)) or not 0.0 < max_step < float('inf'):
        raise ValueError("%s: max_step must be a finite number > 0, got %r" % (what, max_step))
    if not isinstance(mov, PackedFeatures) and not torch.is_tensor(mov):
        raise ValueError("%s: mov must be a [B,C,*vol] tensor or a handle of ops.pack_features" % what)
    if torch.is_tensor(flow) and flow.requires_grad:
        raise ValueError("%s: flow requires grad, but the op has no gradient (detach it)" % what)
    geom, h, fix, flow_c, mask = _warp_ssd_args(mov, fix, flow, mask, what)
    nd, B, C, D, H, W = geom
    ws = torch.empty(int(lib().dfmir_demons_ws_floats(nd, B, C, D, H, W)), device=flow_c.device, dtype=torch.float32)
    out = torch.empty(B + 1, device=flow_c.device, dtype=torch.float32)
    d = torch.empty_like(flow_c)
    check(lib().dfmir_demons_force(nd, _p(h.packed), _p(fix), _p(flow_c), _p(mask), _p(ws), _p(out), _p(out[B:]), _p(d),
                                   float(max_step), B, C, D, H, W, _st()))
    return d, out[B].clone(), out[:B].clone()


LANDMARK_PENALTIES = {'l2': 0, 'tre': 1}
LANDMARK_MAX_K = 4096


def _landmark_geom(flow, fixed_pts, moving_pts, weight, spacing, what):
    """(nd, B, K, D, H, W, hz, hy, hx) of a landmark call after the argument checks (nothing is launched on a bad one).
    moving_pts and weight may be None."""
    if flow.dim() not in (4, 5):
        raise DfmirHipError("%s: expects a [B,nd,*vol] flow, got %d dims" % (what, flow.dim()))
    nd = flow.dim() - 2
    if flow.shape[1] != nd:
        raise DfmirHipError("%s: a %d-D flow needs %d channels, got %s" % (what, nd, nd, tuple(flow.shape)))
    B = int(flow.shape[0])
    for name, t in (("fixed_pts", fixed_pts), ("moving_pts", moving_pts)):
        if t is None:
            continue
        if t.dim() != 3 or int(t.shape[0]) != B or int(t.shape[2]) != nd or tuple(t.shape) != tuple(fixed_pts.shape):
            raise DfmirHipError("%s: %s %s mismatch (expected [B,K,nd] = [%d,K,%d] points for a flow %s, both sets of one "
                                "shape)" % (what, name, tuple(t.shape), B, nd, tuple(flow.shape)))
    K = int(fixed_pts.shape[1])
    if weight is not None and tuple(weight.shape) != (B, K):
        raise DfmirHipError("%s: weight %s mismatch (expected [B,K] = [%d,%d])" % (what, tuple(weight.shape), B, K))
    for name, t in (("flow", flow), ("fixed_pts", fixed_pts), ("moving_pts", moving_pts), ("weight", weight)):
        if t is not None and t.dtype != torch.float32:
            raise DfmirHipError("%s: fp32 tensors only (%s is %s)" % (what, name, t.dtype))
    if not 1 <= K <= LANDMARK_MAX_K:
        raise DfmirHipError("%s: K must lie in [1, %d], got %d landmarks" % (what, LANDMARK_MAX_K, K))
    hs = bending_spacing(spacing, (nd,), what)
    hz, hy, hx = hs if nd == 3 else (1.0,) + hs
    for t in (fixed_pts, moving_pts, weight):
        if t is not None and t.device != flow.device:
            raise DfmirHipError("%s: flow on %s, points on %s" % (what, flow.device, t.device))
    _need(flow, fixed_pts, moving_pts, weight)
    D, H, W = (int(n) for n in (flow.shape[2:] if nd == 3 else (1,) + tuple(flow.shape[2:])))
    if lib().dfmir_landmark_ws_floats(nd, B, K, D, H, W) < 0:
        raise DfmirHipError("%s: needs B >= 1, every extent >= 2 and fewer than 2^31 flow elements, got %s"
                            % (what, tuple(flow.shape)))
    return nd, B, K, D, H, W, hz, hy, hx


def _landmark_fwd(flow, fixed_pts, moving_pts, weight, geom, penalty, want_mapped=False):
    """(out [2] = loss, Wsum; d [B,K]; per_sample [B]; mapped [B,K,nd] or None) of contiguous inputs."""
    nd, B, K, D, H, W, hz, hy, hx = geom
    dev = flow.device
    ws = torch.empty(int(lib().dfmir_landmark_ws_floats(nd, B, K, D, H, W)), device=dev, dtype=torch.float32)
    out = torch.empty(2, device=dev, dtype=torch.float32)
    d = torch.empty((B, K), device=dev, dtype=torch.float32)
    per = torch.empty(B, device=dev, dtype=torch.float32)
    mapped = torch.empty((B, K, nd), device=dev, dtype=torch.float32) if want_mapped else None
    check(lib().dfmir_landmark_fwd(nd, _p(flow), _p(fixed_pts), _p(moving_pts), _p(weight), _p(ws), _p(mapped), _p(d), _p(per),
                                   _p(out), _p(out[1:]), B, K, D, H, W, hz, hy, hx, penalty, _st()))
    return out, d, per, mapped


class LandmarkFn(Function):
    """dfmir_landmark_fwd / _bwd: the forward keeps the flow, the points and Wsum; the backward recomputes the residuals."""

    @staticmethod
    def forward(ctx, flow, fixed_pts, moving_pts, weight, geom, penalty):
        flow, fixed_pts, moving_pts = _c(flow), _c(fixed_pts), _c(moving_pts)
        weight = None if weight is None else _c(weight)
        out = _landmark_fwd(flow, fixed_pts, moving_pts, weight, geom, penalty)[0]
        ctx.save_for_backward(flow, fixed_pts, moving_pts, weight, out)
        ctx.meta = (geom, penalty)
        return out[0].clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        flow, fixed_pts, moving_pts, weight, out = ctx.saved_tensors
        (nd, B, K, D, H, W, hz, hy, hx), penalty = ctx.meta
        g = _c(g)
        dflow = torch.empty_like(flow)
        ws = torch.empty(int(lib().dfmir_landmark_ws_floats(nd, B, K, D, H, W)), device=flow.device, dtype=torch.float32)
        check(lib().dfmir_landmark_bwd(nd, _p(flow), _p(fixed_pts), _p(moving_pts), _p(weight), _p(g), _p(out[1:]), _p(dflow),
                                       _p(ws), B, K, D, H, W, hz, hy, hx, penalty, _st()))
        return dflow, None, None, None, None, None


def landmark_loss(flow, fixed_pts, moving_pts, weight=None, spacing=None, penalty='l2'):
    """Landmark loss of a flow [B,nd,*vol] (nd = 2 or 3, fp32; build-defined, the definition: losses.Landmark_Loss) against K
    pairs of corresponding points per sample: fixed_pts q and moving_pts p [B,K,nd] in voxel coordinates, axis order as the
    flow's channels ((z,) y, x); weight [B,K] (None = 1; 0 marks a padding entry); spacing = nd positive numbers (None = 1).
    m = q + flow(q) (sampled (bi/tri)linearly), d = |spacing * (m - p)|; penalty 'l2': sum w d^2 / Wsum, 'tre': sum w d /
    Wsum over the valid landmarks (w > 0, finite coordinates, q inside the volume), Wsum their sum of w; no valid landmark:
    0 with a zero gradient.  A scalar with a gradient to `flow` only; value and gradient are bit-identical from run to run
    (dfmir_amd/csrc/landmark.hip).  Raises before any launch on mismatched batch or nd, a dtype other than fp32, K outside
    [1, 4096], a bad spacing (ValueError) and an unknown penalty (ValueError); a CPU tensor raises the usual "no CPU
    fallback" error."""
    if penalty not in LANDMARK_PENALTIES:
        raise ValueError("landmark_loss: penalty must be 'l2' or 'tre', got %r" % (penalty,))
    if moving_pts is None:
        raise DfmirHipError("landmark_loss: moving_pts is required")
    geom = _landmark_geom(flow, fixed_pts, moving_pts, weight, spacing, "landmark_loss")
    return LandmarkFn.apply(flow, fixed_pts, moving_pts, weight, geom, LANDMARK_PENALTIES[penalty])


@torch.no_grad()
def landmark_distances(flow, fixed_pts, moving_pts, weight=None, spacing=None):
    """(d [B,K], per_sample [B]) without gradient: the target registration error d = |spacing * (q + flow(q) - p)| of every
    landmark (NaN for an invalid one) and per sample the weighted mean of d over its valid landmarks (NaN without one).
    Arguments and checks as landmark_loss."""
    if moving_pts is None:
        raise DfmirHipError("landmark_distances: moving_pts is required")
    geom = _landmark_geom(flow, fixed_pts, moving_pts, weight, spacing, "landmark_distances")
    weight = None if weight is None else _c(weight)
    _, d, per, _ = _landmark_fwd(_c(flow), _c(fixed_pts), _c(moving_pts), weight, geom, 0)
    return d, per


@torch.no_grad()
def warp_points(points, flow):
    """Points [B,K,nd] of the fixed image carried into the moving image by a flow [B,nd,*vol]: q + flow(q), the flow sampled
    (bi/tri)linearly, [B,K,nd] without gradient.  A point with a non-finite coordinate or outside [0, S_a - 1] on an axis
    gives a NaN row.  The same kernel as landmark_loss, the same checks."""
    geom = _landmark_geom(flow, points, None, None, None, "warp_points")
    return _landmark_fwd(_c(flow), _c(points), None, None, geom, 0, want_mapped=True)[3]


class TPSHandle:
    """What ops.tps_fit returns: coef [B,K+nd+1,nd] float64 = [w (K rows); a_0; A (nd rows)] (it carries the autograd graph to
    moving_pts when those require grad), ctrl [B,K,nd] fp32 = the sanitised control positions in voxels (a padding entry is
    0), scale = the nd factors h_a / L as Python floats, vol = the nd extents, nd."""
    __slots__ = ("coef", "ctrl", "scale", "vol", "nd")

    def __init__(self, coef, ctrl, scale, vol):
        self.coef, self.ctrl, self.scale, self.vol, self.nd = coef, ctrl, tuple(scale), tuple(vol), len(vol)


def tps_scale(vol, spacing=None, what="tps_scale"):
    """The nd factors h_a / L, L = max_a h_a (S_a - 1), that take voxel coordinates of a volume `vol` to the normalised
    coordinates of the thin-plate spline ops (part of their definition: ops.tps_fit)."""
    try:
        vol = tuple(vol)
    except TypeError:
        raise ValueError("%s: vol must be 2 or 3 extents, got %r" % (what, vol)) from None
    if len(vol) not in (2, 3) or any(isinstance(n, bool) or not isinstance(n, int) or n < 2 for n in vol):
        raise ValueError("%s: vol must be 2 or 3 integer extents >= 2, got %r" % (what, vol))
    h = bending_spacing(spacing, (len(vol),), what)
    L = max(ha * (n - 1) for ha, n in zip(h, vol))
    return tuple(ha / L for ha in h)


def tps_fit(fixed_pts, moving_pts, vol, spacing=None, smoothing=0.0, weight=None):
    """Fit the thin-plate / polyharmonic spline through K pairs of corresponding points (build-defined) and return a
    TPSHandle for ops.tps_flow / ops.tps_points.  fixed_pts q, moving_pts p: [B,K,nd] fp32 voxel coordinates, nd = 2 or 3,
    axis order as a flow's channels ((z,) y, x), nd + 1 <= K <= LANDMARK_MAX_K; vol: the nd extents S_a >= 2; spacing: nd
    positive numbers h (None = 1); smoothing: lambda >= 0; weight omega: [B,K] fp32 or None (= 1).

    The target displacement is d_k = p_k - q_k in voxels, ops.warp's convention (warped(x) = moving(x + u(x)), so u(q_k) =
    d_k).  Basis functions live in NORMALISED coordinates xh_a = h_a x_a / L, L = max_a h_a (S_a - 1) -- part of the
    definition: analytically the interpolant is the same, but the float64 system of 1024 points in a 256^2 image has condition
    number 2e14 in voxel coordinates and 1e8 in normalised ones.  The flow is

        u(x) = a_0 + A^T xh + sum_k w_k phi(|xh - qh_k|)       phi(r) = -r (3-D),  r^2 log r with phi(0) = 0 (2-D)

    and coef = [w; a_0; A] solves (Phi + diag(lambda / omega_k)) w + P a = d, P^T w = 0 with Phi_jk = phi(|qh_j - qh_k|), P =
    [1, qh].  With weight=None that is scipy.interpolate.RBFInterpolator(qh, d, kernel='linear' | 'thin_plate_spline',
    degree=1, smoothing=lambda).  lambda = 0 interpolates: u(q_k) = d_k; an affinely related point set gives w = 0.

    An entry with omega = 0, or with a non-finite coordinate in q or p, is padding: its row and column of the system are the
    identity's, its right-hand side and its row of P are zero, so its coefficient is exactly 0, and its position in `ctrl` is
    0.  A NaN or negative weight raises.

    The system is assembled and solved in float64 with torch on the points' device (pairwise squared distances axis by axis,
    torch.linalg.solve_ex): no kernel of this library runs, so CPU tensors are served too (ops.tps_flow then refuses them).
    One host sync reads the solver's `info` and a rank test of P (the smallest eigenvalue of P^T P above 1e-12 of the largest).  The right-hand side is p - q in differentiable torch ops with q detached: autograd reaches moving_pts
    through the returned coef; no gradient is defined for the control positions q or for the weight.  ValueError on K
    outside [nd + 1, LANDMARK_MAX_K], a bad vol, spacing, smoothing or weight, and when the solve fails (info != 0) or returns
    a non-finite coefficient: coincident points with smoothing = 0, fewer than nd + 1 valid points, or valid points that lie
    on one line (plane); DfmirHipError on shapes or dtypes that disagree."""
    what = "tps_fit"
    if not torch.is_tensor(fixed_pts) or not torch.is_tensor(moving_pts):
        raise DfmirHipError("%s: fixed_pts and moving_pts must be [B,K,nd] tensors" % what)
    scale = tps_scale(vol, spacing, what)
    vol = tuple(vol)
    nd = len(vol)
    if fixed_pts.dim() != 3 or int(fixed_pts.shape[2]) != nd or int(fixed_pts.shape[0]) < 1 \
            or tuple(moving_pts.shape) != tuple(fixed_pts.shape):
        raise DfmirHipError("%s: points mismatch (expected two [B,K,%d] sets of one shape for a volume %s, got %s and %s)"
                            % (what, nd, vol, tuple(fixed_pts.shape), tuple(moving_pts.shape)))
    B, K = int(fixed_pts.shape[0]), int(fixed_pts.shape[1])
    if weight is not None and (not torch.is_tensor(weight) or tuple(weight.shape) != (B, K)):
        raise DfmirHipError("%s: weight mismatch (expected [B,K] = [%d,%d])" % (what, B, K))
    for name, t in (("fixed_pts", fixed_pts), ("moving_pts", moving_pts), ("weight", weight)):
        if t is not None and t.dtype != torch.float32:
            raise DfmirHipError("%s: fp32 tensors only (%s is %s)" % (what, name, t.dtype))
        if t is not None and t.device != fixed_pts.device:
            raise DfmirHipError("%s: fixed_pts on %s, %s on %s" % (what, fixed_pts.device, name, t.device))
    if not nd + 1 <= K <= LANDMARK_MAX_K:
        raise ValueError("%s: K must lie in [%d, %d], got %d landmarks" % (what, nd + 1, LANDMARK_MAX_K, K))
    if isinstance(smoothing, bool) or not isinstance(smoothing, (int, float)) or not 0.0 <= smoothing < float('inf'):
        raise ValueError("%s: smoothing must be a finite number >= 0, got %r" % (what, smoothing))
    dev, f64 = fixed_pts.device, torch.float64
    with torch.no_grad():
        q = fixed_pts.detach().to(f64)
        valid = torch.isfinite(q).all(-1) & torch.isfinite(moving_pts.detach()).all(-1)
        om = None
        if weight is not None:
            om = weight.detach().to(f64)
            valid = valid & (om != 0)
        v = valid.to(f64)
        q = torch.where(valid[..., None], q, torch.zeros_like(q))
        qh = q * torch.tensor(scale, dtype=f64, device=dev)
        # squared distances axis by axis: exact zeros on the diagonal, none of the cancellation of the matmul form of
        # torch.cdist (whose exact mode refuses K = 4096 on the device: its grid exceeds the launch limit)
        s = torch.zeros((B, K, K), dtype=f64, device=dev)
        for a in range(nd):
            s += (qh[:, :, None, a] - qh[:, None, :, a]).square()
        if nd == 3:
            phi = -s.sqrt()
        else:
            phi = torch.where(s > 0, 0.5 * s * torch.log(torch.where(s > 0, s, torch.ones_like(s))), torch.zeros_like(s))
        R = K + nd + 1
        A = torch.zeros((B, R, R), dtype=f64, device=dev)
        A[:, :K, :K] = phi * (v[:, :, None] * v[:, None, :])
        diag = 1.0 - v                                                     # identity rows of the padding entries
        if smoothing > 0.0:
            diag = diag + float(smoothing) * v / (torch.where(valid, om, torch.ones_like(v)) if om is not None else 1.0)
        A[:, :K, :K] += torch.diag_embed(diag)
        Pm = torch.cat([torch.ones_like(qh[..., :1]), qh], -1) * v[..., None]
        A[:, :K, K:] = Pm
        A[:, K:, :K] = Pm.transpose(1, 2)
    d = torch.where(valid[..., None], moving_pts.to(f64) - q, torch.zeros_like(q))
    rhs = torch.cat([d, torch.zeros((B, nd + 1, nd), dtype=f64, device=dev)], 1)
    coef, info = torch.linalg.solve_ex(A, rhs)
    with torch.no_grad():
        bad_w = torch.zeros((), dtype=torch.bool, device=dev) if om is None else ~(om >= 0).all()
        # fewer than nd + 1 valid points, or all of them on one line (plane): P has no full column rank, which an LU in
        # floating point need not notice -- the Gram matrix of P's columns shows it
        ev = torch.linalg.eigvalsh(Pm.transpose(1, 2) @ Pm)
        few = (valid.sum(1) < nd + 1).any() | ~(ev[:, 0] > 1e-12 * ev[:, -1]).all()
        flags = torch.stack([(info != 0).any() | few, ~torch.isfinite(coef).all(), bad_w]).tolist()    # the one host sync
    if flags[2]:
        raise ValueError("%s: weight must hold numbers >= 0 (0 marks a padding entry)" % what)
    if flags[0] or flags[1]:
        raise ValueError("%s: the spline system is singular (coincident points with smoothing = 0, fewer than %d valid points, "
                         "or valid points on one %s)" % (what, nd + 1, "line" if nd == 2 else "plane"))
    return TPSHandle(coef, q.to(torch.float32).contiguous(), scale, vol)


def _tps_args(handle_or_coef, handle, what):
    """(coef, handle, B, K) of a tps_flow / tps_points call after the argument checks (nothing is launched on a bad one)."""
    if isinstance(handle_or_coef, TPSHandle):
        if handle is not None:
            raise ValueError("%s: give either a handle, or a coef tensor and handle=" % what)
        handle = handle_or_coef
        coef = handle.coef
    else:
        coef = handle_or_coef
        if not isinstance(handle, TPSHandle):
            raise ValueError("%s: a coef tensor needs handle= the TPSHandle of ops.tps_fit whose control points it weights" % what)
    ctrl = handle.ctrl
    B, K, nd = (int(n) for n in ctrl.shape)
    if not torch.is_tensor(coef) or tuple(coef.shape) != (B, K + nd + 1, nd):
        raise DfmirHipError("%s: coef mismatch (expected [B,K+nd+1,nd] = %s, got %s)"
                            % (what, (B, K + nd + 1, nd), tuple(coef.shape) if torch.is_tensor(coef) else type(coef).__name__))
    if coef.dtype != torch.float64:
        raise DfmirHipError("%s: coef must be float64 (got %s)" % (what, coef.dtype))
    if coef.device != ctrl.device:
        raise DfmirHipError("%s: coef on %s, control points on %s" % (what, coef.device, ctrl.device))
    _need(ctrl)
    return coef, handle, B, K


def _tps_zyx(nd, vals, fill):
    return tuple(vals) if nd == 3 else (fill,) + tuple(vals)


class TpsFlowFn(Function):
    """dfmir_tps_fwd / dfmir_tps_bwd_coef."""

    @staticmethod
    def forward(ctx, coef, ctrl, vol, scale):
        nd = len(vol)
        B, K = int(ctrl.shape[0]), int(ctrl.shape[1])
        coef = _c(coef)
        flow = torch.empty((B, nd) + vol, device=ctrl.device, dtype=torch.float32)
        check(lib().dfmir_tps_fwd(nd, _p(coef), _p(ctrl), None, _p(flow), B, K, 0, *_tps_zyx(nd, vol, 1),
                                  *_tps_zyx(nd, scale, 1.0), _st()))
        ctx.save_for_backward(ctrl)
        ctx.meta = (nd, B, K, vol, scale)
        return flow

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        ctrl, = ctx.saved_tensors
        nd, B, K, vol, scale = ctx.meta
        g = _c(g)
        dhw = _tps_zyx(nd, vol, 1)
        ws = torch.empty(int(lib().dfmir_tps_ws_bytes(nd, B, K, *dhw)) // 8, device=g.device, dtype=torch.float64)
        dcoef = torch.empty((B, K + nd + 1, nd), device=g.device, dtype=torch.float64)
        check(lib().dfmir_tps_bwd_coef(nd, _p(ctrl), _p(g), _p(dcoef), _p(ws), B, K, *dhw, *_tps_zyx(nd, scale, 1.0), _st()))
        return dcoef, None, None, None


def tps_flow(handle_or_coef, handle=None):
    """The dense flow [B,nd,*vol] fp32 of a thin-plate spline (build-defined; the definition: ops.tps_fit): u at every voxel
    of the handle's volume, in ops.warp's convention.  tps_flow(handle) evaluates the handle's own coefficients; tps_flow(coef,
    handle=handle) evaluates a float64 tensor coef [B,K+nd+1,nd] on the handle's control points, scale and volume.  Basis
    values are fp32, their products with the coefficients and the sum over the control points float64, rounded once
    (dfmir_amd/csrc/tps.hip).  Differentiable in coef (once): dcoef[k] = sum_x phi(|xh - qh_k|) g(x), da_0 = sum g, dA = sum
    xh g^T in float64 without atomics -- through the handle's coef the gradient reaches the moving_pts of ops.tps_fit.  No
    gradient is defined for the control positions.  Forward and backward are bit-identical from run to run.  Raises before
    any launch on a coef that is not float64 [B,K+nd+1,nd] on the control points' device and on a volume of 2^31 or more flow
    elements; a CPU handle raises the usual "no CPU fallback" error."""
    what = "tps_flow"
    coef, handle, B, K = _tps_args(handle_or_coef, handle, what)
    if lib().dfmir_tps_ws_bytes(handle.nd, B, K, *_tps_zyx(handle.nd, handle.vol, 1)) < 0:
        raise DfmirHipError("%s: needs B <= 65535 and fewer than 2^31 flow elements, got B = %d, vol %s" % (what, B, handle.vol))
    return TpsFlowFn.apply(coef, handle.ctrl, handle.vol, handle.scale)


@torch.no_grad()
def tps_points(handle, points):
    """The spline of a TPSHandle at M arbitrary points: points [B,M,nd] fp32 voxel coordinates (inside the volume or not) ->
    [B,M,nd] fp32 displacements u(points), the kernel of ops.tps_flow with another position source.  No gradient.  A point
    with a non-finite coordinate gives a non-finite row.  Raises before any launch on a shape or dtype that disagrees; a CPU
    tensor raises the usual "no CPU fallback" error."""
    what = "tps_points"
    if not isinstance(handle, TPSHandle):
        raise ValueError("%s: handle must be the TPSHandle of ops.tps_fit" % what)
    coef, handle, B, K = _tps_args(handle, None, what)
    nd = handle.nd
    if not torch.is_tensor(points) or points.dim() != 3 or int(points.shape[0]) != B or int(points.shape[2]) != nd \
            or int(points.shape[1]) < 1:
        raise DfmirHipError("%s: points mismatch (expected [B,M,nd] = [%d,M,%d] with M >= 1, got %s)"
                            % (what, B, nd, tuple(points.shape) if torch.is_tensor(points) else type(points).__name__))
    if points.dtype != torch.float32:
        raise DfmirHipError("%s: fp32 tensors only (points is %s)" % (what, points.dtype))
    if points.device != handle.ctrl.device:
        raise DfmirHipError("%s: points on %s, control points on %s" % (what, points.device, handle.ctrl.device))
    M = int(points.shape[1])
    if B > 65535 or B * M * nd >= 2 ** 31:
        raise DfmirHipError("%s: needs B <= 65535 and fewer than 2^31 coordinates, got %s" % (what, tuple(points.shape)))
    points = _c(points)
    out = torch.empty((B, M, nd), device=points.device, dtype=torch.float32)
    check(lib().dfmir_tps_fwd(nd, _p(_c(coef.detach())), _p(handle.ctrl), _p(points), _p(out), B, K, M, 2, 2, 2,
                              *_tps_zyx(nd, handle.scale, 1.0), _st()))
    return out


def _keypoint_image(t, what, name, planes=1):
    """(nd, B, D, H, W) of a [B,1,*vol] fp32 tensor after the checks a CPU tensor can fail (ValueError: nothing is launched);
    `planes` = the most planes per voxel a kernel of the call forms from it."""
    if not torch.is_tensor(t) or t.dim() not in (4, 5) or t.shape[1] != 1:
        raise ValueError("%s: %s must be a [B,1,H,W] or [B,1,D,H,W] tensor, got %s"
                         % (what, name, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
    nd = t.dim() - 2
    if t.shape[0] < 1 or min(t.shape[2:]) < 2:
        raise ValueError("%s: %s needs B >= 1 and every extent >= 2, got %s" % (what, name, tuple(t.shape)))
    if t.dtype != torch.float32:
        raise ValueError("%s: fp32 tensors only (%s is %s)" % (what, name, t.dtype))
    if t.numel() * planes >= 2 ** 31:
        raise ValueError("%s: %s %s has 2^31 or more elements (times %d planes)" % (what, name, tuple(t.shape), planes))
    if t.requires_grad:
        raise ValueError("%s: %s requires grad, but the op has no gradient (detach it)" % (what, name))
    D, H, W = (int(n) for n in (t.shape[2:] if nd == 3 else (1,) + tuple(t.shape[2:])))
    return nd, int(t.shape[0]), D, H, W


def _keypoint_int(v, lo, hi, what, name):
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
        raise ValueError("%s: %s must be an integer in [%d, %d], got %r" % (what, name, lo, hi, v))
    return v


@torch.no_grad()
def foerstner_response(I, sigma=1.5, spacing=None):
    """The Foerstner structure-tensor response of an image (build-defined), the distinctiveness that keypoints are picked by:
    I [B,1,*vol] fp32, 2-D or 3-D -> R [B,1,*vol].  Axis order (z,) y, x; S_a the extents.

        g_a(x) = (I(min(x_a + 1, S_a - 1)) - I(max(x_a - 1, 0))) / (2 h_a)        h = `spacing`: nd positive numbers, None = 1
        T_ab   = ops.gaussian_smooth(g_a g_b, sigma)                             nd (nd + 1) / 2 planes, fp32, renormalised at
                                                                                 the faces: that op's definition exactly
        R      = det(T) / trace(adj(T))   ( = 1 / trace(T^-1); in 2-D det / trace)

    R is formed in DOUBLE from the fp32 planes and rounded once (the determinant of a near-singular T cancels), and is 0
    where the denominator is not > 0 or anything is non-finite.  One kernel forms the products (a thread writes all planes
    of its voxel from a staged tile), dfmir_gauss_smooth filters them, one kernel forms the response
    (dfmir_amd/csrc/keypoints.hip).  Bit-identical from run to run; nothing syncs with the host.  No gradient: an input that
    requires grad raises.  ValueError before any launch on a tensor that is not [B,1,*vol] fp32 with every extent >= 2, 2^31
    or more elements in the stack of planes, a bad spacing (ops.bending_spacing) and what ops.gaussian_smooth refuses of
    sigma; a CPU tensor raises the usual "no CPU fallback" error."""
    what = "foerstner_response"
    nd, B, D, H, W = _keypoint_image(I, what, "I", planes=6 if torch.is_tensor(I) and I.dim() == 5 else 3)
    hs = bending_spacing(spacing, (nd,), what)
    hz, hy, hx = hs if nd == 3 else (1.0,) + hs
    gauss_radii(sigma, 3.0, nd, what)
    _need(I)
    I = _c(I)
    vol = tuple(I.shape[2:])
    prod = torch.empty((B, nd * (nd + 1) // 2) + vol, device=I.device, dtype=torch.float32)
    check(lib().dfmir_keypoint_products(nd, _p(I), _p(prod), B, D, H, W, hz, hy, hx, _st()))
    T = gaussian_smooth(prod, sigma)
    R = torch.empty((B, 1) + vol, device=I.device, dtype=torch.float32)
    check(lib().dfmir_keypoint_response(nd, _p(T), _p(R), B, D, H, W, _st()))
    return R


@torch.no_grad()
def local_maxima(R, radius, mask=None, threshold=0.0):
    """Non-maximum suppression of a response map (build-defined): R [B,1,*vol] fp32, 2-D or 3-D -> [B,1,*vol] holding R(x)
    where x is selected and 0 elsewhere.  x is selected iff R(x) > threshold, mask(x) != 0 (mask: [B,1,*vol] fp32 or None) and
    for every other y of the (2 radius + 1)^nd window clipped to the volume R(y) < R(x), or R(y) == R(x) and y has the HIGHER
    linear index -- the lowest index wins a plateau.  A NaN is never selected, and as a neighbour it compares as -inf; the mask
    does not remove a voxel as a competitor.  radius: an integer in 1..KEYPOINT_NMS_MAX_RADIUS (8); threshold: a finite number.
    One launch, tile plus halo in LDS and a direct walk of the window (dfmir_amd/csrc/keypoints.hip).  Bit-identical from run
    to run; nothing syncs with the host; no gradient.  ValueError before any launch on tensors that are not [B,1,*vol] fp32 of
    one shape with every extent >= 2, 2^31 or more elements, a tensor that requires grad, a radius outside its range and a
    threshold that is not finite; a CPU tensor raises the usual "no CPU fallback" error."""
    what = "local_maxima"
    nd, B, D, H, W = _keypoint_image(R, what, "R")
    r = _keypoint_int(radius, 1, KEYPOINT_NMS_MAX_RADIUS, what, "radius")
    if mask is not None:
        if not torch.is_tensor(mask) or tuple(mask.shape) != tuple(R.shape):
            raise ValueError("%s: mask must be [B,1,*vol] = %s, got %s"
                             % (what, tuple(R.shape), tuple(mask.shape) if torch.is_tensor(mask) else type(mask).__name__))
        _keypoint_image(mask, what, "mask")
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)) \
            or not abs(float(threshold)) <= float(np.finfo(np.float32).max):
        raise ValueError("%s: threshold must be a finite number, got %r" % (what, threshold))
    _need(R, mask)
    if mask is not None and mask.device != R.device:
        raise DfmirHipError("%s: R on %s, mask on %s" % (what, R.device, mask.device))
    R = _c(R)
    mask = None if mask is None else _c(mask)
    out = torch.empty_like(R)
    check(lib().dfmir_keypoint_nms(nd, _p(R), _p(mask), _p(out), B, D, H, W, r, float(threshold), _st()))
    return out


@torch.no_grad()
def select_keypoints(peaks, K):
    """The K strongest peaks of a suppressed response map as points (plain torch, plumbing only; it runs wherever `peaks`
    lives): peaks [B,1,*vol], 2-D or 3-D, as ops.local_maxima returns it -> (pts [B,K,nd] fp32 voxel coordinates in axis order
    (z,) y, x, weight [B,K] fp32 = the peaks' values).  Per sample the K largest POSITIVE entries in descending order, ties
    broken by the lower linear index (a stable sort; torch.topk leaves the order of ties undefined).  A sample with fewer
    positive entries is padded with NaN coordinates and weight 0, the padding ops.tps_fit honours.  K: an integer in
    1..LANDMARK_MAX_K.  Nothing syncs with the host.  ValueError on a tensor that is not [B,1,*vol] floating point and on a K
    outside its range."""
    what = "select_keypoints"
    if not torch.is_tensor(peaks) or peaks.dim() not in (4, 5) or peaks.shape[1] != 1 or not peaks.is_floating_point() \
            or peaks.shape[0] < 1 or min(peaks.shape[2:]) < 1:
        raise ValueError("%s: peaks must be a floating-point [B,1,H,W] or [B,1,D,H,W] tensor, got %s"
                         % (what, tuple(peaks.shape) if torch.is_tensor(peaks) else type(peaks).__name__))
    K = _keypoint_int(K, 1, LANDMARK_MAX_K, what, "K")
    B, vol = int(peaks.shape[0]), tuple(int(n) for n in peaks.shape[2:])
    flat = peaks.detach().reshape(B, -1).to(torch.float32)
    flat = torch.where(flat > 0, flat, torch.zeros_like(flat))         # a NaN or a negative entry is no peak
    val, lin = torch.sort(flat, dim=1, descending=True, stable=True)
    val, lin = val[:, :K], lin[:, :K]
    if val.shape[1] < K:
        pad = K - val.shape[1]
        val = torch.cat([val, val.new_zeros((B, pad))], 1)
        lin = torch.cat([lin, lin.new_zeros((B, pad))], 1)
    coords = []
    for n in reversed(vol):
        coords.append(lin % n)
        lin = torch.div(lin, n, rounding_mode='floor')
    pts = torch.stack(coords[::-1], -1).to(torch.float32)
    pts = torch.where((val > 0)[..., None], pts, torch.full_like(pts, float('nan')))
    return pts.contiguous(), val.contiguous()


def _keypoint_window(radius, step, nd, what):
    r = _keypoint_int(radius, 1, KEYPOINT_MAX_RADIUS[nd], what, "radius (%d-D)" % nd)
    return r, _keypoint_int(step, 1, KEYPOINT_MAX_STEP, what, "step")


def _keypoint_points(t, what, name, B, nd, K=None):
    if not torch.is_tensor(t) or t.dim() != 3 or int(t.shape[0]) != B or int(t.shape[2]) != nd or int(t.shape[1]) < 1 \
            or (K is not None and int(t.shape[1]) != K):
        raise ValueError("%s: %s must be [B,K,nd] = [%d,%s,%d] with K >= 1, got %s"
                         % (what, name, B, "K" if K is None else K, nd, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
    if t.dtype != torch.float32:
        raise ValueError("%s: fp32 tensors only (%s is %s)" % (what, name, t.dtype))
    if t.requires_grad:
        raise ValueError("%s: %s requires grad, but the op has no gradient (detach it)" % (what, name))
    return int(t.shape[1])


@torch.no_grad()
def keypoint_cost(fix, mov, pts, radius, step=1, patch=1):
    """The windowed patch SSD around K points, the cost rows of a sparse displacement search (build-defined): fix, mov
    [B,C,*vol] features (fp32, 1 <= C <= 16, 2-D or 3-D, one shape), pts [B,K,nd] fp32 voxel coordinates in axis order (z,) y,
    x, as ops.landmark_distances takes them -> cost [B,K,D], D = (2 radius + 1)^nd.  With q_k = rint(pts[b,k]) (ties to even)
    and P = (2 patch + 1)^nd,

        cost[b,k,j] = 1/(C P) * sum_c sum_{o in {-patch..patch}^nd} ( fix[b,c,q+o] - mov[b,c,q+o+step*d_j] )^2

    both sides reading 0 outside the volume; j enumerates d_j in {-radius .. radius}^nd in row-major order (dz,) dy, dx with
    -radius first, exactly as ops.ssd_cost_volume does.  A row is all NaN where a coordinate of the point is non-finite or q_k
    lies outside the volume.  Precision: the difference is fp32, its square and the sum are float64 in one fixed order for
    every j, scaled in float64 and rounded once -- displacements whose reads all fall outside the volume tie bit for bit.
    One workgroup per keypoint stages the fixed patch and, plane by plane, the moving search region in LDS
    (dfmir_amd/csrc/keypoints.hip).  Bit-identical from run to run; nothing syncs with the host; no gradient.

    Limits: radius 1..KEYPOINT_MAX_RADIUS[nd] (16 in 2-D, 8 in 3-D), step 1..KEYPOINT_MAX_STEP (4), patch
    0..KEYPOINT_MAX_PATCH (3), the staged extent E = 2 (radius step + patch) + 1 <= KEYPOINT_MAX_EXTENT (96) -- a call beyond
    it raises, there is no unstaged path --, B K D < 2^31, B <= 65535.  ValueError before any launch on these, on shapes that
    disagree, and on what ops.pack_features refuses of the features (rank, C outside 1..16, dtype, 2^31 or more elements, a
    tensor that requires grad); a CPU tensor raises the usual "no CPU fallback" error."""
    what = "keypoint_cost"
    geom = _features_geom(fix, what, "fix")
    if not torch.is_tensor(mov) or tuple(mov.shape) != tuple(fix.shape):
        raise ValueError("%s: fix %s / mov %s differ in shape"
                         % (what, tuple(fix.shape), tuple(mov.shape) if torch.is_tensor(mov) else mov))
    _features_geom(mov, what, "mov")
    nd, B, C, D, H, W = geom
    K = _keypoint_points(pts, what, "pts", B, nd)
    r, step = _keypoint_window(radius, step, nd, what)
    patch = _keypoint_int(patch, 0, KEYPOINT_MAX_PATCH, what, "patch")
    E = 2 * (r * step + patch) + 1
    if E > KEYPOINT_MAX_EXTENT:
        raise ValueError("%s: the staged extent 2 (radius step + patch) + 1 = %d exceeds KEYPOINT_MAX_EXTENT = %d"
                         % (what, E, KEYPOINT_MAX_EXTENT))
    Dn = (2 * r + 1) ** nd
    if B * K * Dn >= 2 ** 31:
        raise ValueError("%s: the cost rows [%d,%d,%d] have 2^31 or more elements" % (what, B, K, Dn))
    if B > 65535:
        raise ValueError("%s: B must be <= 65535, got %s" % (what, tuple(fix.shape)))
    _need(fix, mov, pts)
    if mov.device != fix.device or pts.device != fix.device:
        raise DfmirHipError("%s: fix on %s, mov on %s, pts on %s" % (what, fix.device, mov.device, pts.device))
    fix, mov, pts = _c(fix), _c(mov), _c(pts)
    cost = torch.empty((B, K, Dn), device=fix.device, dtype=torch.float32)
    check(lib().dfmir_keypoint_cost(nd, _p(fix), _p(mov), _p(pts), _p(cost), B, C, K, D, H, W, r, step, patch, _st()))
    return cost


@torch.no_grad()
def keypoint_argmin(cost, radius, step=1, prior=None, coeff=0.0):
    """The sparse coupled argmin over each keypoint's cost row (build-defined) -> (idx int32 [B,K], disp fp32 [B,K,nd]):

        idx[b,k] = argmin_j ( cost[b,k,j] + coeff * sum_a (step*d_j[a] - prior[b,k,a])^2 ),        disp[b,k] = step * d_idx

    cost: [B,K,D] as ops.keypoint_cost lays it out, D = (2 radius + 1)^nd with nd = 2 or 3 (prior's last extent; without a
    prior the one nd whose D matches, 3-D first); prior: [B,K,nd] fp32 in voxels, None = the plain argmin (coeff is then not
    read); coeff: a finite float >= 0.  The lowest j wins a tie; only finite penalised values compete, so a NaN (or infinite)
    entry is never selected, and a row without a finite entry gives idx 0 and disp NaN -- q + disp is then a padding point for
    ops.tps_fit.  One wave per keypoint; the cross-lane reduction carries (value, j).  The squares are added in the order (z,)
    y, x in fp32.  Nothing syncs with the host; no gradient.  ValueError before any launch on a cost that is not [B,K,D] fp32,
    a radius or step outside KEYPOINT_MAX_RADIUS[nd] / KEYPOINT_MAX_STEP, a D that is no (2 radius + 1)^nd, a prior of another
    shape, a coeff that is negative or not finite, 2^31 or more elements and a tensor that requires grad; a CPU tensor raises
    the usual "no CPU fallback" error."""
    what = "keypoint_argmin"
    if not torch.is_tensor(cost) or cost.dim() != 3 or cost.shape[0] < 1 or cost.shape[1] < 1:
        raise ValueError("%s: cost must be a [B,K,D] tensor, got %s"
                         % (what, tuple(cost.shape) if torch.is_tensor(cost) else type(cost).__name__))
    if cost.dtype != torch.float32:
        raise ValueError("%s: fp32 tensors only (cost is %s)" % (what, cost.dtype))
    if cost.requires_grad:
        raise ValueError("%s: cost requires grad, but the op has no gradient (detach it)" % what)
    if cost.numel() >= 2 ** 31:
        raise ValueError("%s: cost %s has 2^31 or more elements" % (what, tuple(cost.shape)))
    B, K, Dn = (int(n) for n in cost.shape)
    if isinstance(radius, bool) or not isinstance(radius, int) or radius < 1:
        raise ValueError("%s: radius must be an integer >= 1, got %r" % (what, radius))
    if prior is not None:
        if not torch.is_tensor(prior) or prior.dim() != 3 or int(prior.shape[2]) not in (2, 3):
            raise ValueError("%s: prior must be [B,K,nd], got %s"
                             % (what, tuple(prior.shape) if torch.is_tensor(prior) else type(prior).__name__))
        nd = int(prior.shape[2])
        _keypoint_points(prior, what, "prior", B, nd, K)
    else:
        nd = 3 if (2 * radius + 1) ** 3 == Dn else 2
    r, step = _keypoint_window(radius, step, nd, what)
    if (2 * r + 1) ** nd != Dn:
        raise ValueError("%s: cost %s must have (2 radius + 1)^nd = %d entries per row" % (what, tuple(cost.shape), (2 * r + 1) ** nd))
    try:
        coeff = float(coeff)
    except (TypeError, ValueError):
        raise ValueError("%s: coeff must be a finite number >= 0, got %r" % (what, coeff))
    if not 0.0 <= coeff < float('inf'):
        raise ValueError("%s: coeff must be a finite number >= 0, got %r" % (what, coeff))
    _need(cost, prior)
    if prior is not None and prior.device != cost.device:
        raise DfmirHipError("%s: cost on %s, prior on %s" % (what, cost.device, prior.device))
    cost = _c(cost)
    prior = None if prior is None else _c(prior)
    idx = torch.empty((B, K), device=cost.device, dtype=torch.int32)
    disp = torch.empty((B, K, nd), device=cost.device, dtype=torch.float32)
    check(lib().dfmir_keypoint_argmin(nd, _p(cost), _p(prior), coeff, _p(idx), _p(disp), B * K, r, step, _st()))
    return idx, disp


class MulFn(Function):
    """a * b element-wise, same shapes (`prediction * mask`, util/losses.py:120-121)."""

    @staticmethod
    def forward(ctx, a, b):
        _need(a, b)
        a, b = _c(a), _c(b)
        if a.shape != b.shape or a.dtype != torch.float32 or b.dtype != torch.float32:
            raise DfmirHipError("ops.mul: fp32 tensors of one shape (got %s, %s)" % (tuple(a.shape), tuple(b.shape)))
        out = torch.empty_like(a)
        check(lib().dfmir_mul(_p(a), _p(b), _p(out), a.numel(), _st()))
        ctx.save_for_backward(a if ctx.needs_input_grad[1] else None, b if ctx.needs_input_grad[0] else None)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = _c(g)
        da = db = None
        if ctx.needs_input_grad[0]:
            da = torch.empty_like(g)
            check(lib().dfmir_mul(_p(g), _p(b), _p(da), g.numel(), _st()))
        if ctx.needs_input_grad[1]:
            db = torch.empty_like(g)
            check(lib().dfmir_mul(_p(g), _p(a), _p(db), g.numel(), _st()))
        return da, db


def mul(a, b):
    return MulFn.apply(a, b)


NCC_VOLUME = 4            # DFMIR_NCC_VOLUME (include/dfmir_hip.h): mode flag of dfmir_ncc_fwd_m / _bwd_m


def ncc_gauss_window(sigma):
    """(taps, K, c) of NCC_Loss's Gaussian window (util/losses.py:153-181): K = 3 sigma + ((3 sigma + 1) mod 2) taps
    g(d) = exp(-(d - (K-1)/2)^2 / (2 sigma^2)), formed in float64 and rounded to fp32, and c = 1 / (2.506628274631 sigma).
    The window is c * g (x) g [(x) g], not normalised.  sigma: a positive integer <= 10 (K <= 31)."""
    if isinstance(sigma, bool) or not isinstance(sigma, (int, np.integer)) or not 1 <= sigma <= 10:
        raise ValueError("NCC Gaussian window: sigma must be a positive integer <= 10, got %r" % (sigma,))
    sigma = int(sigma)
    K = 3 * sigma + (3 * sigma + 1) % 2
    d = np.arange(K, dtype=np.float64) - (K - 1) / 2.0
    return np.exp(-d * d / (2.0 * sigma * sigma)).astype(np.float32), K, 1.0 / (2.506628274631 * sigma)


class NCCFn(Function):
    """Windowed NCC; gradient w.r.t. the prediction I only (J is the fixed target).  `win`: an odd int = the win^nd mean
    window, or the (taps, K, c) of ncc_gauss_window = the Gaussian one (dfmir_ncc_gauss_fwd / _bwd).
    mode 0: -sqrt(mean(cc)) (NCC_Loss, util/losses.py:248-256), with a mask -sqrt(sum(cc * mask) / sum(mask)) and 0 for
    an empty mask (:257-261); mode 1: -mean(cc) (vxm NCC.loss, torchvoxelmorph/losses.py:67)."""

    @staticmethod
    def forward(ctx, I, J, win, eps, mask=None, mode=0):
        _need(I, J, mask)
        I, J = _c(I), _c(J)
        if I.shape[1] != 1:
            raise DfmirHipError("NCC expects single-channel volumes")
        if mask is not None and (mask.dtype != torch.float32 or mask.shape != I.shape or not mask.is_contiguous()):
            raise DfmirHipError("NCC mask: a contiguous fp32 tensor of the volumes' shape")
        nd = I.dim() - 2
        B = I.shape[0]
        D, H, W = I.shape[2:] if nd == 3 else (1,) + tuple(I.shape[2:])
        if nd == 3 and D == 1:
            mode = int(mode) | NCC_VOLUME  # a one-plane VOLUME keeps the win^3 window of the reference's conv3d
        N = I.numel()
        sums = torch.empty(5 * N, device=I.device, dtype=torch.float32)
        tmp2 = torch.empty(5 * N, device=I.device, dtype=torch.float32)
        ws = torch.empty(8, device=I.device, dtype=torch.float32)
        out = torch.empty((), device=I.device, dtype=torch.float32)
        if isinstance(win, tuple):
            taps, K, c = win
            win = (np.ascontiguousarray(taps, dtype=np.float32), int(K), float(c))
            check(lib().dfmir_ncc_gauss_fwd(_p(I), _p(J), _p(mask), int(mode), _p(sums), _p(tmp2), _p(ws), _p(out), B, D, H, W,
                                            win[0].ctypes.data, win[1], win[2], float(eps), _st()))
        elif mask is None and mode == 0:
            check(lib().dfmir_ncc_fwd(_p(I), _p(J), _p(sums), _p(tmp2), _p(ws), _p(out), B, D, H, W, int(win),
                                      float(eps), _st()))
        else:
            check(lib().dfmir_ncc_fwd_m(_p(I), _p(J), _p(mask), int(mode), _p(sums), _p(tmp2), _p(ws), _p(out), B, D, H, W,
                                        int(win), float(eps), _st()))
        ctx.save_for_backward(I, J, sums, ws, mask)
        ctx.meta = (B, D, H, W, win if isinstance(win, tuple) else int(win), float(eps), int(mode))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        I, J, sums, ws, mask = ctx.saved_tensors
        B, D, H, W, win, eps, mode = ctx.meta
        g = _c(g)
        N = I.numel()
        t1 = torch.empty(3 * N, device=I.device, dtype=torch.float32)
        t2 = torch.empty(3 * N, device=I.device, dtype=torch.float32)
        dI = torch.empty_like(I)
        if isinstance(win, tuple):
            check(lib().dfmir_ncc_gauss_bwd(_p(I), _p(J), _p(mask), mode, _p(sums), _p(t1), _p(t2), _p(ws), _p(g), _p(dI),
                                            B, D, H, W, win[0].ctypes.data, win[1], win[2], eps, _st()))
        elif mask is None and mode == 0:
            check(lib().dfmir_ncc_bwd(_p(I), _p(J), _p(sums), _p(t1), _p(t2), _p(ws), _p(g), _p(dI), B, D, H, W,
                                      win, eps, _st()))
        else:
            check(lib().dfmir_ncc_bwd_m(_p(I), _p(J), _p(mask), mode, _p(sums), _p(t1), _p(t2), _p(ws), _p(g), _p(dI),
                                        B, D, H, W, win, eps, _st()))
        return dI, None, None, None, None, None


def ncc_loss(I, J, win=9, eps=1e-5, mask=None, reduction='neg_sqrt_mean', kernel='mean', sigma=None):
    """reduction 'neg_sqrt_mean' (NCC_Loss) or 'neg_mean' (vxm NCC); mask: any tensor that broadcasts to I's shape
    (bool / byte / float: the reference multiplies cc by it, util/losses.py:261).  The window counts win^nd positions by the
    tensors' RANK: a volume of one plane [B,1,1,H,W] keeps win^3, as the reference's conv3d does.
    kernel 'mean': the win^nd box; 'gaussian': the window of ncc_gauss_window(sigma) (sigma None = 3; `win` is not read),
    whose 3-D form c * g (x) g (x) g is build-defined.  There a mask that is broadcast r-fold normalises by
    its own sum, as the reference's `1 / torch.sum(mask)` does (util/losses.py:260): the loss is sqrt(r) (neg_mean: r) times
    the one over the expanded mask, which is what the 'mean' kernel keeps returning."""
    if kernel == 'gaussian':
        win = ncc_gauss_window(3 if sigma is None else sigma)
    elif kernel != 'mean':
        raise ValueError("NCC kernel must be 'mean' or 'gaussian', got %r" % (kernel,))
    mode = {'neg_sqrt_mean': 0, 'neg_mean': 1}[reduction]
    r = 1
    if mask is not None:
        r = I.numel() // mask.numel() if kernel == 'gaussian' else 1
        mask = mask.to(device=I.device, dtype=torch.float32).expand_as(I).contiguous()
    loss = NCCFn.apply(I, J, win, eps, mask, mode)
    return loss if r == 1 else scale(loss.view(1), float(r) if mode else float(r) ** 0.5).view(())


class NMIFn(Function):
    """-MI of one soft-binned joint histogram over every voxel of y_true and y_pred (NMI_Loss, util/losses.py:263-348);
    result shape (1,).  Gradients go to both inputs; `centers` (a device tensor) is a constant and gets none."""

    @staticmethod
    def forward(ctx, y_true, y_pred, centers, preterm, max_clip, mask=None):
        _need(y_true, y_pred, centers, mask)
        y_true, y_pred = _c(y_true), _c(y_pred)
        if y_true.shape != y_pred.shape or y_true.dtype != torch.float32 or y_pred.dtype != torch.float32:
            raise DfmirHipError("NMI: fp32 tensors of one shape (got %s, %s)" % (tuple(y_true.shape), tuple(y_pred.shape)))
        if mask is not None and (mask.dtype != torch.float32 or mask.shape != y_true.shape or not mask.is_contiguous()):
            raise DfmirHipError("NMI mask: a contiguous fp32 tensor of the inputs' shape")
        nb, n = centers.numel(), y_true.numel()
        ws = torch.empty(int(lib().dfmir_nmi_ws_floats(n, nb)), device=y_true.device, dtype=torch.float32)
        out = torch.empty(1, device=y_true.device, dtype=torch.float32)
        check(lib().dfmir_nmi_fwd(_p(y_true), _p(y_pred), _p(mask), _p(centers), nb, float(preterm), float(max_clip), n,
                                  _p(ws), _p(out), _st()))
        ctx.save_for_backward(y_true, y_pred, centers, mask, ws)
        ctx.meta = (nb, float(preterm), float(max_clip), n)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        y_true, y_pred, centers, mask, ws = ctx.saved_tensors
        nb, preterm, max_clip, n = ctx.meta
        g = _c(g)
        dt = torch.empty_like(y_true) if ctx.needs_input_grad[0] else None
        dp = torch.empty_like(y_pred) if ctx.needs_input_grad[1] else None
        if dt is not None or dp is not None:
            check(lib().dfmir_nmi_bwd(_p(y_true), _p(y_pred), _p(mask), _p(centers), nb, preterm, max_clip, n, _p(ws),
                                      _p(g), _p(dt), _p(dp), _st()))
        return dt, dp, None, None, None, None


_NMI_CENTERS = {}


def nmi_preterm(centers, sigma_ratio=0.5):
    """1 / (2 sigma^2), sigma = mean(diff(centers)) * sigma_ratio, in float64 as the reference (util/losses.py:284-285)."""
    import numpy as np
    c = np.asarray(centers, dtype=np.float64).reshape(-1)
    if not 2 <= c.size <= 64:
        raise DfmirHipError("NMI supports 2 to 64 bin centers (got %d)" % c.size)
    sigma = np.mean(np.diff(c)) * sigma_ratio
    return float(1.0 / (2.0 * np.square(sigma)))


def nmi_centers(centers, device):
    """The bin centers as a float32 device tensor, uploaded once per (values, device) and reused (also inside a captured
    step, which cannot upload)."""
    import numpy as np
    vals = tuple(float(v) for v in np.asarray(centers, dtype=np.float64).reshape(-1))
    key = (vals, torch.device(device))
    t = _NMI_CENTERS.get(key)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            raise DfmirHipError("NMI: bin centers must be uploaded before a graph capture (run one eager step first)")
        t = _NMI_CENTERS[key] = torch.tensor(vals, dtype=torch.float32, device=device)
    return t


def nmi_loss(y_true, y_pred, centers, sigma_ratio=0.5, max_clip=1.0, mask=None):
    """-MI of NMI_Loss (util/losses.py:263-348): both inputs clamped to [0, max_clip], the whole tensor (batch and
    channels) one histogram; `centers`: 2..64 host floats (a list / array; any spacing).  mask (crop_background): any
    tensor that broadcasts to the inputs' shape; voxels with mask > 1e-4 count.  Returns shape (1,)."""
    preterm = nmi_preterm(centers, sigma_ratio)
    _need(y_true, y_pred, mask)
    c = nmi_centers(centers, y_true.device)
    if mask is not None:
        mask = mask.to(device=y_true.device, dtype=torch.float32).expand_as(y_true).contiguous()
    return NMIFn.apply(y_true, y_pred, c, preterm, float(max_clip), mask)


def _mind_geom(I, radius, dilation, what):
    """(nd, B, D, H, W, C) of a MIND input after the argument checks (ValueError: nothing is launched)."""
    for name, v in (("radius", radius), ("dilation", dilation)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= 4:
            raise ValueError("%s: %s must be an integer in 1..4, got %r" % (what, name, v))
    if I.dim() not in (4, 5):
        raise ValueError("%s: expects [B,1,H,W] or [B,1,D,H,W] tensors, got %d dims" % (what, I.dim()))
    if I.shape[1] != 1:
        raise ValueError("%s: expects single-channel images, got %d channels" % (what, I.shape[1]))
    if I.numel() == 0:
        raise ValueError("%s: empty tensor %s" % (what, tuple(I.shape)))
    nd = I.dim() - 2
    D, H, W = I.shape[2:] if nd == 3 else (1,) + tuple(I.shape[2:])
    return nd, int(I.shape[0]), int(D), int(H), int(W), 12 if nd == 3 else 4


def _mind_ws(geom, r, d, which, device):
    nd, B, D, H, W, _ = geom
    n = int(lib().dfmir_mind_ws_floats(nd, B, D, H, W, r, d, which))
    if n < 0:
        raise DfmirHipError("MIND: unsupported shape %s" % ((B, D, H, W),))
    return torch.empty(n, device=device, dtype=torch.float32)


def mind_descriptor(I, radius=2, dilation=2):
    """The MIND-SSC descriptor M [B,C,*vol] of I [B,1,*vol] (C = 12 in 3-D, 4 in 2-D; the definition and the channel order:
    losses.MIND_Loss).  No gradient: for inspection and tests."""
    geom = _mind_geom(I, radius, dilation, "mind_descriptor")
    _need(I)
    if I.dtype != torch.float32:
        raise DfmirHipError("MIND: fp32 tensors only (got %s)" % I.dtype)
    I = _c(I.detach())
    nd, B, D, H, W, C = geom
    ws = _mind_ws(geom, int(radius), int(dilation), 0, I.device)
    out = torch.empty((B, C) + tuple(I.shape[2:]), device=I.device, dtype=torch.float32)
    check(lib().dfmir_mind_desc(_p(I), nd, B, D, H, W, int(radius), int(dilation), _p(ws), _p(out), _st()))
    return out


class MINDFn(Function):
    """L2 loss of the MIND-SSC descriptors of two images (dfmir_mind_fwd / _bwd); gradients to both.  The workspace that
    lives until the backward holds m = D - min D of both images (C floats per voxel and image)."""

    @staticmethod
    def forward(ctx, a, b, radius, dilation, mask=None):
        a, b = _c(a), _c(b)
        geom = _mind_geom(a, radius, dilation, "mind_loss")
        nd, B, D, H, W, _ = geom
        ws = _mind_ws(geom, radius, dilation, 0, a.device)
        out = torch.empty((), device=a.device, dtype=torch.float32)
        check(lib().dfmir_mind_fwd(_p(a), _p(b), _p(mask), nd, B, D, H, W, radius, dilation, _p(ws), _p(out), _st()))
        ctx.save_for_backward(a, b, mask, ws)
        ctx.meta = (geom, radius, dilation)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        a, b, mask, ws = ctx.saved_tensors
        geom, radius, dilation = ctx.meta
        nd, B, D, H, W, _ = geom
        g = _c(g)
        da = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        db = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        if da is not None or db is not None:
            tmp = _mind_ws(geom, radius, dilation, 1, a.device)
            check(lib().dfmir_mind_bwd(_p(a), _p(b), _p(mask), nd, B, D, H, W, radius, dilation, _p(ws), _p(tmp), _p(g),
                                       _p(da), _p(db), _st()))
        return da, db, None, None, None


def mind_loss(a, b, radius=2, dilation=2, mask=None):
    """MIND-SSC loss of two single-channel images [B,1,*vol] (2-D or 3-D; the definition: losses.MIND_Loss): the mean over
    (B, C, voxels) of (M_a - M_b)^2, or with `mask` (anything that broadcasts to [B,1,*vol], used as float weights)
    sum mask * mean_k (M_a - M_b)^2 / sum mask -- 0 for an empty mask, as a device scalar without a host sync.  Gradients go
    to both images.  ValueError on a bad radius / dilation (1..4 each), rank or channel count; a CPU tensor raises the
    usual "no CPU fallback" error."""
    _mind_geom(a, radius, dilation, "mind_loss")
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError("mind_loss: the two images differ in shape (%s, %s)" % (tuple(a.shape), tuple(b.shape)))
    _need(a, b)
    if a.dtype != torch.float32 or b.dtype != torch.float32:
        raise DfmirHipError("MIND: fp32 tensors only (got %s, %s)" % (a.dtype, b.dtype))
    if mask is not None:
        mask = mask.to(device=a.device, dtype=torch.float32).expand_as(a).contiguous()
    return MINDFn.apply(a, b, int(radius), int(dilation), mask)


def _gradfield_geom(I, spacing, what):
    """(nd, B, D, H, W, hz, hy, hx) of a gradient-field input after the argument checks (ValueError: nothing is launched)."""
    if not torch.is_tensor(I) or I.dim() not in (4, 5):
        raise ValueError("%s: expects [B,1,H,W] or [B,1,D,H,W] tensors, got %s" %
                         (what, "%d dims" % I.dim() if torch.is_tensor(I) else type(I).__name__))
    if I.shape[1] != 1:
        raise ValueError("%s: expects single-channel images, got %d channels" % (what, I.shape[1]))
    if I.numel() == 0:
        raise ValueError("%s: empty tensor %s" % (what, tuple(I.shape)))
    if I.numel() >= 2 ** 31:
        raise ValueError("%s: images of 2^31 and more voxels are not supported, got %s" % (what, tuple(I.shape)))
    nd = I.dim() - 2
    sp = bending_spacing(spacing, (nd,), what)
    hz, hy, hx = sp if nd == 3 else (1.0,) + sp
    D, H, W = (int(v) for v in (I.shape[2:] if nd == 3 else (1,) + tuple(I.shape[2:])))
    return nd, int(I.shape[0]), D, H, W, hz, hy, hx


def _gradfield_pos(v, what, name):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) \
            or not np.isfinite(v) or not 0.0 < float(v) <= 3.0e38:
        raise ValueError("%s: %s must be a positive finite number, got %r" % (what, name, v))
    return float(v)


def gradfield_eps(eps, eta, what, pair=True):
    """(auto, eta, eps_A, eps_B) of the `eps` / `eta` arguments of the gradient-field term: eps = 'auto' (eta > 0 is then
    read), a positive float or, with `pair`, a pair of positive floats.  ValueError otherwise."""
    if isinstance(eps, str):
        if eps != 'auto':
            raise ValueError("%s: eps must be 'auto', a positive number%s, got %r"
                             % (what, " or a pair of them" if pair else "", eps))
        return 1, _gradfield_pos(eta, what, "eta"), 0.0, 0.0
    if pair and isinstance(eps, (tuple, list)):
        if len(eps) != 2:
            raise ValueError("%s: eps must be 'auto', a positive number or a pair of them, got %r" % (what, eps))
        return 0, 0.0, _gradfield_pos(eps[0], what, "eps"), _gradfield_pos(eps[1], what, "eps")
    e = _gradfield_pos(eps, what, "eps")
    return 0, 0.0, e, e


def _gradfield_ws(geom, device):
    n = int(lib().dfmir_gradfield_ws_floats(*geom[:5]))
    if n < 0:
        raise DfmirHipError("gradfield: unsupported shape %s" % (geom[1:5],))
    return torch.empty(n, device=device, dtype=torch.float32)


class GradFieldFn(Function):
    """dfmir_gradfield_fwd / _bwd; gradients to both images.  The workspace that lives until the backward holds eps_A,
    eps_B and the sum of the mask at its head."""

    @staticmethod
    def forward(ctx, a, b, geom, eps, mask=None):
        a, b = _c(a), _c(b)
        ws = _gradfield_ws(geom, a.device)
        out = torch.empty((), device=a.device, dtype=torch.float32)
        check(lib().dfmir_gradfield_fwd(_p(a), _p(b), _p(mask), *geom, *eps, _p(ws), _p(out), _st()))
        ctx.save_for_backward(a, b, mask, ws)
        ctx.meta = geom
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        a, b, mask, ws = ctx.saved_tensors
        g = _c(g)
        da = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        db = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        if da is not None or db is not None:
            check(lib().dfmir_gradfield_bwd(_p(a), _p(b), _p(mask), _p(g), _p(ws), _p(da), _p(db), *ctx.meta, _st()))
        return da, db, None, None, None


def gradfield_loss(a, b, eps='auto', eta=1.0, spacing=None, mask=None):
    """Normalised-gradient-field distance of two single-channel images [B,1,*vol] (2-D or 3-D; the definition:
    losses.GradField_Loss): the mean over (B, voxels) of 1 - <g(a), g(b)>^2 / ((|g(a)|^2 + eps_a^2) (|g(b)|^2 + eps_b^2))
    with the clamped central differences g divided by the voxel spacing (`spacing`, one positive number per axis in the
    order (z,) y, x; None = 1); with `mask` (anything that broadcasts to [B,1,*vol], used as float weights)
    sum mask (1 - s) / sum mask -- 0 for an empty mask, as a device scalar without a host sync.  eps: 'auto' (eta * the
    mean gradient magnitude of each image, a constant in the backward), a positive float, or a pair (eps_a, eps_b).
    Gradients go to both images.  ValueError before any launch on a bad rank, channel count, shape mismatch, eps, eta or
    spacing; a CPU tensor raises the usual "no CPU fallback" error."""
    geom = _gradfield_geom(a, spacing, "gradfield_loss")
    if not torch.is_tensor(b) or tuple(a.shape) != tuple(b.shape):
        raise ValueError("gradfield_loss: the two images differ in shape (%s, %s)"
                         % (tuple(a.shape), tuple(b.shape) if torch.is_tensor(b) else type(b).__name__))
    e = gradfield_eps(eps, eta, "gradfield_loss")
    if a.dtype != torch.float32 or b.dtype != torch.float32:
        raise DfmirHipError("gradfield_loss: fp32 tensors only (got %s, %s)" % (a.dtype, b.dtype))
    _need(a, b)
    if mask is not None:
        mask = mask.to(device=a.device, dtype=torch.float32).expand_as(a).contiguous()
    return GradFieldFn.apply(a, b, geom, e, mask)


def gradfield_normals(I, eps='auto', eta=1.0, spacing=None):
    """The normalised gradient field n(I) = g(I) / sqrt(|g(I)|^2 + eps^2) [B,nd,*vol] of I [B,1,*vol], channels in the order
    (z,) y, x (the definition: losses.GradField_Loss; eps: 'auto' or one positive float).  No gradient: for inspection and
    tests."""
    geom = _gradfield_geom(I, spacing, "gradfield_normals")
    auto, eta, e, _ = gradfield_eps(eps, eta, "gradfield_normals", pair=False)
    if I.dtype != torch.float32:
        raise DfmirHipError("gradfield_normals: fp32 tensors only (got %s)" % I.dtype)
    _need(I)
    I = _c(I.detach())
    ws = _gradfield_ws(geom, I.device)
    out = torch.empty((geom[1], geom[0]) + tuple(I.shape[2:]), device=I.device, dtype=torch.float32)
    check(lib().dfmir_gradfield_field(_p(I), *geom, auto, eta, e, _p(ws), _p(out), _st()))
    return out


def as_label_map(t):
    """An integer label map as the contiguous uint8 tensor the Dice kernels read, on the tensor's own device: any integer
    dtype, bool, or a float tensor with integral values; every value must lie in [0, 255].  The range check reads the
    extrema back (a host sync), so call it where inputs are set, never inside a captured region."""
    if not torch.is_tensor(t):
        raise DfmirHipError("as_label_map: a tensor is required (got %s)" % type(t).__name__)
    if t.dtype == torch.uint8:
        return _c(t)
    if t.dtype == torch.bool:
        return _c(t.to(torch.uint8))
    if t.is_complex():
        raise DfmirHipError("as_label_map: unsupported dtype %s" % t.dtype)
    if t.numel():
        lo, hi = t.min().item(), t.max().item()
        if not (lo >= 0 and hi <= 255):           # (also catches NaN)
            raise DfmirHipError("as_label_map: label values must lie in [0, 255] (got %s .. %s)" % (lo, hi))
        if t.is_floating_point() and not bool((t == t.round()).all()):
            raise DfmirHipError("as_label_map: a float label map must hold integral values")
    return _c(t.to(torch.uint8))


_DICE_STATE = {}


def _dice_labels(labels):
    try:
        vals = [v for v in (labels.tolist() if hasattr(labels, "tolist") else list(labels))]
    except TypeError:
        raise DfmirHipError("warp_dice: labels must be a list of label values")
    if not 1 <= len(vals) <= 64:
        raise DfmirHipError("warp_dice scores 1 to 64 labels (got %d)" % len(vals))
    for v in vals:
        if isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= 255:
            raise DfmirHipError("warp_dice: label values must be integers in [0, 255] (got %r)" % (v,))
    vals = tuple(int(v) for v in vals)
    if len(set(vals)) != len(vals):
        raise DfmirHipError("warp_dice: duplicate label values in %r" % (vals,))
    return vals


def _dice_state(vals, shape, nd, device):
    """(value -> slot table, workspace) on the device, made once per (labels, shape, device) and reused: a captured step
    neither uploads nor allocates."""
    key = (vals, tuple(shape), torch.device(device))
    st = _DICE_STATE.get(key)
    if st is None:
        if torch.cuda.is_current_stream_capturing():
            raise DfmirHipError("warp_dice: the label table must be uploaded before a graph capture (run one eager step first)")
        table = [255] * 256
        for i, v in enumerate(vals):
            table[v] = i
        B = shape[0]
        D, H, W = (shape[2:] if nd == 3 else (1,) + tuple(shape[2:]))
        n = int(lib().dfmir_warp_dice_ws_floats(nd, B, len(vals), D, H, W))
        if n <= 0:
            raise DfmirHipError("warp_dice: unsupported shape %s" % (tuple(shape),))
        st = _DICE_STATE[key] = (torch.tensor(table, dtype=torch.uint8, device=device),
                                 torch.empty(n, device=device, dtype=torch.float32))
    return st


class WarpDiceFn(Function):
    """(loss, dice[B,K]) of a fixed label map against a moving label map warped by `flow` (dfmir_warp_dice_fwd); the
    gradient goes to `flow` only."""

    @staticmethod
    def forward(ctx, mov, fix, flow, table, ws, K, mode):
        nd = flow.dim() - 2
        B = flow.shape[0]
        D, H, W = (flow.shape[2:] if nd == 3 else (1,) + tuple(flow.shape[2:]))
        dev = flow.device
        loss = torch.empty((), device=dev, dtype=torch.float32)
        dice = torch.empty(B, K, device=dev, dtype=torch.float32)
        seeds = torch.empty(2, B, K, device=dev, dtype=torch.float32)
        check(lib().dfmir_warp_dice_fwd(nd, _p(mov), _p(fix), _p(flow), _p(table), K, B, D, H, W, mode, _p(ws), _p(loss),
                                        _p(dice), _p(seeds), _st()))
        ctx.save_for_backward(mov, fix, flow, table, seeds)
        ctx.meta = (nd, K, B, D, H, W)
        ctx.mark_non_differentiable(dice)
        return loss, dice

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _gdice):
        mov, fix, flow, table, seeds = ctx.saved_tensors
        nd, K, B, D, H, W = ctx.meta
        if not ctx.needs_input_grad[2]:
            return (None,) * 7
        g = _c(g)
        dflow = torch.empty_like(flow)
        check(lib().dfmir_warp_dice_bwd(nd, _p(mov), _p(fix), _p(flow), _p(table), K, B, D, H, W, _p(seeds), _p(g),
                                        _p(dflow), _st()))
        return None, None, dflow, None, None, None, None


def warp_dice(mov, fix, flow, labels, mode='bilinear'):
    """Dice of the FIXED label map `fix` against the MOVING label map `mov` warped by `flow`, over the label values
    `labels` (1..64 distinct integers in [0, 255]; values of the maps that are not listed are not scored):
    Dice().loss(one_hot(fix)[:, labels], SpatialTransformer(one_hot(mov)[:, labels], flow)) of the reference, without the
    one-hot tensors.  mov / fix: uint8 [B,1,*vol] (ops.as_label_map), flow: fp32 [B,nd,*vol].  Returns (loss, dice[B,K]).
    mode 'bilinear' (multi-linear weights; gradient to flow) or 'nearest' (the hard Dice of the label warp of
    test.py:80-81; no gradient).  Never syncs with the host."""
    vals = _dice_labels(labels)
    if mode not in ('bilinear', 'nearest'):
        raise DfmirHipError("warp_dice: mode must be 'bilinear' or 'nearest' (got %r)" % (mode,))
    nd = flow.dim() - 2
    if nd not in (2, 3) or flow.shape[1] != nd:
        raise DfmirHipError("warp_dice: flow must be [B,nd,*vol] with nd = 2 or 3 (got %s)" % (tuple(flow.shape),))
    want = (flow.shape[0], 1) + tuple(flow.shape[2:])
    if tuple(mov.shape) != want or tuple(fix.shape) != want:
        raise DfmirHipError("warp_dice: label maps %s / %s do not match the flow %s (expected %s)"
                            % (tuple(mov.shape), tuple(fix.shape), tuple(flow.shape), want))
    if mov.dtype != torch.uint8 or fix.dtype != torch.uint8 or flow.dtype != torch.float32:
        raise DfmirHipError("warp_dice: uint8 label maps (ops.as_label_map) and an fp32 flow (got %s, %s, %s)"
                            % (mov.dtype, fix.dtype, flow.dtype))
    if mode == 'nearest' and flow.requires_grad:
        raise DfmirHipError("warp_dice: mode='nearest' has no gradient; detach the flow")
    _need(mov, fix, flow)
    table, ws = _dice_state(vals, flow.shape, nd, flow.device)
    return WarpDiceFn.apply(_c(mov), _c(fix), _c(flow), table, ws, len(vals), 1 if mode == 'nearest' else 0)


EDT_SQ_INF = 1 << 29          # DFMIR_EDT_SQ_INF: "no voxel of the set in this batch element"
HD_SURFACE = 1                # DFMIR_HD_SURFACE
_HD_WS = {}


def _label_vol(t, what):
    """(nd, B, D, H, W) of a uint8 label map [B,1,*vol]."""
    if not torch.is_tensor(t) or t.dim() not in (4, 5) or t.shape[1] != 1:
        raise DfmirHipError("%s: label maps are [B,1,*vol] tensors with 2 or 3 spatial axes (got %s)"
                            % (what, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
    if t.dtype != torch.uint8:
        raise DfmirHipError("%s: uint8 label maps (ops.as_label_map) (got %s)" % (what, t.dtype))
    nd = t.dim() - 2
    D, H, W = (t.shape[2:] if nd == 3 else (1,) + tuple(t.shape[2:]))
    return nd, int(t.shape[0]), int(D), int(H), int(W)


def _hd_ws(nd, B, K, D, H, W, device, what):
    """The scratch of the distance passes, made once per (label count, shape, device) and reused; an unsupported shape
    raises here, before anything is launched."""
    n = int(lib().dfmir_label_hausdorff_ws_bytes(nd, B, K, D, H, W))
    if n <= 0:
        raise DfmirHipError("%s: unsupported shape %s (every axis must lie in 1..256)" % (what, (B, D, H, W)))
    if device is None:
        return None
    key = (nd, B, min(K, 4), D, H, W, torch.device(device))
    ws = _HD_WS.get(key)
    if ws is None:
        if torch.cuda.is_current_stream_capturing():
            raise DfmirHipError("%s: the scratch must be allocated before a graph capture (run one eager call first)" % what)
        ws = _HD_WS[key] = torch.empty(n // 4, device=device, dtype=torch.int32)
    return ws


def label_edt_sq(label_map, value, surface=False):
    """Exact squared Euclidean distance transform: int32 [B,*vol], min over voxels y of the same batch element with
    label_map(y) == value of |x - y|^2, EDT_SQ_INF where there is none.  surface=True: distances to the BORDER voxels of
    that set (set voxels with a face neighbour outside the set or outside the volume; a volume of one plane counts the
    in-plane neighbours only).  label_map: uint8 [B,1,*vol], every axis <= 256.  Never syncs with the host."""
    if isinstance(value, bool) or int(value) != value or not 0 <= int(value) <= 255:
        raise DfmirHipError("label_edt_sq: the label value must be an integer in [0, 255] (got %r)" % (value,))
    nd, B, D, H, W = _label_vol(label_map, "label_edt_sq")
    _hd_ws(nd, B, 1, D, H, W, None, "label_edt_sq")
    _need(label_map)
    m = _c(label_map)
    out = torch.empty((B,) + tuple(m.shape[2:]), device=m.device, dtype=torch.int32)
    check(lib().dfmir_label_edt_sq(nd, _p(m), int(value), 1 if surface else 0, B, D, H, W, _p(out), _st()))
    return out


def _hd_percentile(percentile):
    """percentile in (0, 100], a multiple of 0.001 -> thousandths as an integer."""
    try:
        q = float(percentile)
    except (TypeError, ValueError):
        raise DfmirHipError("label_hausdorff: percentile must be a number (got %r)" % (percentile,))
    qm = int(round(1000.0 * q)) if q == q and abs(q) < 1e9 else 0
    if not (0.0 < q <= 100.0) or qm < 1 or abs(1000.0 * q - qm) > 1e-6:
        raise DfmirHipError("label_hausdorff: percentile must lie in (0, 100] and be a multiple of 0.001 (got %r)"
                            % (percentile,))
    return qm


def label_hausdorff(a, b, labels, percentile=100.0, surface=False, mean=True):
    """Hausdorff distance of two label maps per batch element and label value, in voxels, on the exact distance
    transform (dfmir_label_hausdorff) -- the reference's HausdorffDistance (util/loss_metrics.py:105-132) without the host.
    a / b: uint8 [B,1,*vol] (ops.as_label_map) of equal shape, every axis <= 256; labels: 1..64 distinct integers in
    [0, 255].  Returns (hd[B,K] fp32, directed[2,B,K] fp32, mean[2,B,K] fp32, d2[2,B,K] int32): direction 0 is a -> b (over
    the voxels of a's set, the distance to b's set), 1 the converse; d2 is the `percentile` of the squared distances by
    nearest rank (100: the maximum), directed its square root, mean the mean distance, hd the larger directed value.
    A label that either map lacks gives +inf (d2: EDT_SQ_INF).  surface=True measures between the border voxels of the
    sets.  mean=False skips the mean (and, at percentile 100, the histogram it needs) and returns None in its place.
    Never syncs with the host."""
    vals = _dice_labels(labels)
    qm = _hd_percentile(percentile)
    nd, B, D, H, W = _label_vol(a, "label_hausdorff")
    _label_vol(b, "label_hausdorff")
    if tuple(a.shape) != tuple(b.shape):
        raise DfmirHipError("label_hausdorff: label maps %s / %s do not match" % (tuple(a.shape), tuple(b.shape)))
    K = len(vals)
    _hd_ws(nd, B, K, D, H, W, None, "label_hausdorff")
    _need(a, b)
    a, b = _c(a), _c(b)
    ws = _hd_ws(nd, B, K, D, H, W, a.device, "label_hausdorff")
    dev = a.device
    hd = torch.empty(B, K, device=dev, dtype=torch.float32)
    directed = torch.empty(2, B, K, device=dev, dtype=torch.float32)
    mean_t = torch.empty(2, B, K, device=dev, dtype=torch.float32) if mean else None
    d2 = torch.empty(2, B, K, device=dev, dtype=torch.int32)
    host_vals = (ctypes.c_ubyte * K)(*vals)
    check(lib().dfmir_label_hausdorff(nd, _p(a), _p(b), ctypes.cast(host_vals, ctypes.c_void_p), K, B, D, H, W, qm,
                                      HD_SURFACE if surface else 0, _p(ws), _p(hd), _p(directed), _p(mean_t), _p(d2),
                                      _st()))
    return hd, directed, mean_t, d2


def _dense_pair(y_true, y_pred, what):
    if y_true.shape != y_pred.shape or y_true.dtype != torch.float32 or y_pred.dtype != torch.float32:
        raise DfmirHipError("%s: fp32 tensors of one shape (got %s %s, %s %s)"
                            % (what, tuple(y_true.shape), y_true.dtype, tuple(y_pred.shape), y_pred.dtype))
    _need(y_true, y_pred)
    return _c(y_true), _c(y_pred)


class DiceFn(Function):
    """vxm Dice of float tensors [B,C,*vol] (dfmir_dice_fwd / _bwd); gradients to both arguments."""

    @staticmethod
    def forward(ctx, y_true, y_pred):
        y_true, y_pred = _dense_pair(y_true, y_pred, "Dice")
        if y_true.dim() < 3:
            raise DfmirHipError("Dice: [B,C,*vol] tensors (got %s)" % (tuple(y_true.shape),))
        planes = y_true.shape[0] * y_true.shape[1]
        S = y_true.numel() // max(planes, 1)
        n = int(lib().dfmir_dice_ws_floats(planes, S))
        if n <= 0:
            raise DfmirHipError("Dice: unsupported shape %s" % (tuple(y_true.shape),))
        ws = torch.empty(n, device=y_true.device, dtype=torch.float32)
        out = torch.empty((), device=y_true.device, dtype=torch.float32)
        check(lib().dfmir_dice_fwd(_p(y_true), _p(y_pred), planes, S, _p(ws), _p(out), _st()))
        ctx.save_for_backward(y_true, y_pred, ws)
        ctx.meta = (planes, S)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        y_true, y_pred, ws = ctx.saved_tensors
        planes, S = ctx.meta
        dt = torch.empty_like(y_true) if ctx.needs_input_grad[0] else None
        dp = torch.empty_like(y_pred) if ctx.needs_input_grad[1] else None
        if dt is not None or dp is not None:
            check(lib().dfmir_dice_bwd(_p(y_true), _p(y_pred), planes, S, _p(ws), _p(_c(g)), _p(dt), _p(dp), _st()))
        return dt, dp


def dice_loss(y_true, y_pred):
    """-mean_{b,c} 2 sum(t p) / max(sum(t + p), 1e-5): vxm `Dice().loss` (torchvoxelmorph/losses.py:79-90)."""
    return DiceFn.apply(y_true, y_pred)


class MSEFn(Function):
    """mean((t - p)^2) (dfmir_mse_fwd / _bwd); gradients to both arguments."""

    @staticmethod
    def forward(ctx, y_true, y_pred):
        y_true, y_pred = _dense_pair(y_true, y_pred, "MSE")
        n = y_true.numel()
        nws = int(lib().dfmir_mse_ws_floats(n))
        if nws <= 0:
            raise DfmirHipError("MSE: empty tensors")
        ws = torch.empty(nws, device=y_true.device, dtype=torch.float32)
        out = torch.empty((), device=y_true.device, dtype=torch.float32)
        check(lib().dfmir_mse_fwd(_p(y_true), _p(y_pred), n, _p(ws), _p(out), _st()))
        ctx.save_for_backward(y_true, y_pred)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        y_true, y_pred = ctx.saved_tensors
        dt = torch.empty_like(y_true) if ctx.needs_input_grad[0] else None
        dp = torch.empty_like(y_pred) if ctx.needs_input_grad[1] else None
        if dt is not None or dp is not None:
            check(lib().dfmir_mse_bwd(_p(y_true), _p(y_pred), y_true.numel(), _p(_c(g)), _p(dt), _p(dp), _st()))
        return dt, dp


def mse_loss(y_true, y_pred):
    """mean((y_true - y_pred)^2): vxm `MSE().loss` (torchvoxelmorph/losses.py:70-76)."""
    return MSEFn.apply(y_true, y_pred)


class MeanFn(Function):
    @staticmethod
    def forward(ctx, x):
        _need(x)
        x = _c(x)
        out = torch.empty((), device=x.device, dtype=torch.float32)
        check(lib().dfmir_sum_scaled(_p(x), _p(out), x.numel(), 1.0 / x.numel(), _st()))
        ctx.shape = x.shape
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        g = _c(g)
        n = 1
        for s in ctx.shape:
            n *= s
        dx = torch.empty(ctx.shape, device=g.device, dtype=torch.float32)
        check(lib().dfmir_fill_from_scalar(_p(g), _p(dx), n, 1.0 / n, _st()))
        return dx


def mean(x):
    return MeanFn.apply(x)


def adam_step(p, g, m, v, lr, beta1, beta2, eps, step, grad_scale=1.0, bump=True):
    """One Adam update of p in place (dfmir_adam_step).  bump=False: p is no conv weight (the flow of infer.refine_flow), so
    the packed weights derived from the parameters stay valid and the weights epoch is left alone."""
    _need(p, g, m, v)
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    check(lib().dfmir_adam_step(_p(p), _p(g), _p(m), _p(v), p.numel(), float(lr), float(beta1), float(beta2),
                                float(eps), float(bc1), float(bc2), float(grad_scale), _st()))
    if bump:
        bump_weights_epoch()
