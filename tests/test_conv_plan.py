"""Characterization of the kernel selection of ops.conv_raw / ops.conv_wgrad_raw against tests/golden/conv_plan.json.

Runs on a CPU: the library is a stand-in whose answers to the ten selection queries are INPUTS of each case, so the table
depends neither on the built library nor on the machine.  Every other dfmir_* call is recorded (name, ints and floats by
value, pointers as None / "p", a byref geometry as "g" when its 20 fields are the ones the case implies, else spelled
out) and returns 0; a row leaves out what is None, False or 0.  The table was recorded from the ops.py
of the commit it names (tests/golden/make_golden_conv_plan.py) and holds for any later ops.py: which entry point a layer
reaches with which arguments, how many queries that took (at most the recorded number), what the bench profiler is told
(kind, flops, issued -- bit-equal), and the side effects on _LAST_ACTGRAD, _LAST_CONV_AMAX, the probe tag and the
un-fused residual add.

Besides the five names the stand-in replaces on the module (lib, _st, amax_slot, _ws_cached, zeros), _upwgrad_ws is
replaced too: it asks torch for the current HIP stream, which a CPU run does not have.
"""
import ctypes
import hashlib
import json
import os

import pytest
import torch

from dfmir_amd import DfmirHipError
from dfmir_amd import ops
from dfmir_amd._lib import DfConvGeom

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plan.json")

QUERY = {"res": "dfmir_conv3x3_res_ok", "tiny": "dfmir_conv3d_tiny_ok", "march": "dfmir_conv3d_march_ok",
         "s2c2": "dfmir_conv3d_s2c2_ok", "s2": "dfmir_conv3d_s2_ok", "s2d": "dfmir_conv3d_s2_dgrad_ok",
         "split": "dfmir_conv3d_split_ok", "splitw": "dfmir_conv3d_split_wgrad_ok", "upw": "dfmir_conv3d_upwgrad_ok",
         "marchw": "dfmir_conv3d_wgrad_is_march_at"}
FWD_QUERIES = ("res", "tiny", "march", "s2c2", "s2", "s2d", "split")
WGRAD_QUERIES = ("splitw", "upw", "s2c2", "s2", "marchw")
SWITCHES = ("_NO_TINY3D", "_NO_TINYVOL", "_NO_S2", "_NO_FLOW_MARCH", "_NO_RES")
FWD_ENTRIES = ("dfmir_conv3d_march_fwd", "dfmir_conv3d_tiny_fwd", "dfmir_conv3d_s2c2_fwd", "dfmir_conv3d_s2_fwd",
               "dfmir_conv3d_s2_dgrad", "dfmir_conv3d_split_fwd_actgrad", "dfmir_conv3d_split_fwd_sub",
               "dfmir_conv3x3_fwd_scaled_res", "dfmir_conv_fwd_scaled")
WGRAD_ENTRIES = ("dfmir_conv3d_s2c2_wgrad", "dfmir_conv3d_s2_wgrad", "dfmir_conv3d_upwgrad",
                 "dfmir_conv3d_split_wgrad_upcat", "dfmir_conv3d_split_wgrad_db", "dfmir_conv_wgrad_scaled_ch",
                 "dfmir_det_begin", "dfmir_det_end")
_BYREF = type(ctypes.byref(DfConvGeom()))


class FakeLib(object):
    """The stand-in library of one case: `yes` = the short names (QUERY) of the selection queries it answers with 1."""

    def __init__(self, yes, pair, geom):
        self.yes = frozenset(QUERY[q] for q in yes)
        self.pair, self.geom, self.queries, self.calls = pair, geom, 0, []

    def __getattr__(self, name):
        if not name.startswith("dfmir_"):
            raise AttributeError(name)
        if name in QUERY.values():
            def fn(*args):
                self.queries += 1
                return 1 if name in self.yes else 0
        elif name == "dfmir_conv3d_split_is_pair":
            def fn(cu):
                return self.pair
        elif name.endswith("_floats"):
            def fn(*args):
                return 16
        else:
            def fn(*args):
                self.calls.append([name] + [self._arg(a) for a in args])
                return 0
        return fn


    def _arg(self, a):
        if isinstance(a, _BYREF):                 # "g" = the 20 fields the case implies (_geom); any others are spelled out
            got = [getattr(a._obj, f) for f, _ in DfConvGeom._fields_]
            return "g" if got == self.geom else got
        if isinstance(a, ctypes.c_void_p):
            return "p" if a.value else None
        if a is None or isinstance(a, (int, float)):
            return a
        raise TypeError("unexpected argument %r" % (a,))


def _geom(case):
    """The DfConvGeom fields a case implies (the weight gradient: dil 1, act 0, slope 0)."""
    fwd = case["id"][0] == "f"
    slope = ctypes.c_float(0.2 if fwd and case["act"] else 0.0).value
    return list((case["N"],) + case["ch"] + case["isp"] + _out_sp(case["isp"], case["stride"]) + case["K"]
                + (case["stride"], case["dil"] if fwd else 1) + case["pad"] + (case["pad_mode"], case["act"] if fwd else 0, slope))


class Prof(object):
    accepts_issued = True

    def __init__(self):
        self.log = []

    def __call__(self, kind, flops, launch, issued=None):
        self.log.append([kind, flops, issued])
        launch()


def _patched(mp, case, fake, prof):
    ws = torch.zeros(16)
    mp.setattr(ops, "lib", lambda: fake)
    mp.setattr(ops, "_st", lambda: None)
    mp.setattr(ops, "amax_slot", lambda device, n=1: torch.zeros(max(n, 1)))
    mp.setattr(ops, "_ws_cached", lambda *a, **k: (ws, True))
    mp.setattr(ops, "zeros", lambda shape, device: torch.zeros(shape))
    mp.setattr(ops, "_upwgrad_ws", lambda device: ws)
    for s in SWITCHES:
        mp.setattr(ops, s, s in case["flags"])
    mp.setattr(ops, "_UPWGRAD_MIN_VOX", case.get("min_vox", 400000))
    mp.setattr(ops, "_CONV_PROFILER", [prof])
    mp.setitem(ops._DET, "on", bool(case.get("det")))
    mp.setitem(ops._PROBE_AUDIT, "on", False)
    mp.setattr(ops, "_LAST_CONV_AMAX", [None])
    mp.setattr(ops, "_LAST_ACTGRAD", [None])


def _out_sp(isp, stride):
    return tuple((n - 1) // stride + 1 for n in isp)      # "same" padding p = dil (K - 1) / 2


def _like(kind, shape):
    """None / a tensor of `shape` / one of another shape with as many elements / the right shape, not contiguous."""
    if kind is None:
        return None
    if kind == "ok":
        return torch.zeros(shape)
    if kind == "bad":
        return torch.zeros((shape[0] * shape[1],) + tuple(shape[2:]))
    assert kind == "nc"
    return torch.zeros(tuple(shape[:3]) + (shape[4], shape[3])).transpose(3, 4)


def _case_id(kind, c, maker):
    """`kind`, the arguments that differ from the maker's defaults, [the switches flipped] [the queries answered yes]."""
    names = maker.__code__.co_varnames[:maker.__code__.co_argcount]
    words = [kind]
    for name, default in zip(names, maker.__defaults__):
        v = c[name]
        if name in ("flags", "yes", "pad") or v == default:
            continue
        words.append(name + "=" + ("x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)))
    if c["pad"] != tuple(c.get("dil", 1) * (k - 1) // 2 for k in c["K"]):
        words.append("pad=" + "x".join(str(i) for i in c["pad"]))
    return " ".join(words + ["[%s]" % ",".join(f[4:] for f in c["flags"]), "[%s]" % ",".join(c["yes"])])


# ---------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------
def fwd_case(K=(3, 3, 3), stride=1, dil=1, ch=(16, 16), isp=(4, 8, 8), N=1, probe=True, res=None, ring=False, cu=None,
             act_src=None, bias=True, act=0, flags=(), yes=(), pair=0, pad=None, pad_mode=0):
    if K[0] == 1 and K != (1, 1, 1):
        isp = (1,) + tuple(isp[1:])
    c = dict(K=tuple(K), stride=stride, dil=dil, ch=tuple(ch), isp=tuple(isp), N=N, probe=probe, res=res, ring=ring, cu=cu,
             act_src=act_src, bias=bias, act=act, flags=tuple(flags), yes=tuple(yes), pair=pair,
             pad=tuple(pad) if pad else tuple(dil * (k - 1) // 2 for k in K), pad_mode=pad_mode)
    c["id"] = _case_id("f", c, fwd_case)
    return c


def run_fwd(case, with_prof):
    Cin, Cout = case["ch"]
    N, K, stride = case["N"], case["K"], case["stride"]
    out_sp = _out_sp(case["isp"], stride)
    yshape = (N, Cout) + out_sp
    fake, prof = FakeLib(case["yes"], case["pair"], _geom(case)), (Prof() if with_prof else None)
    with pytest.MonkeyPatch.context() as mp:
        _patched(mp, case, fake, prof)
        y = ops.conv_raw(torch.empty((N, Cin) + case["isp"]), torch.empty(K[0] * K[1] * K[2] * Cin * Cout),
                         torch.zeros(Cout) if case["bias"] else None, Cout, K, stride, case["pad"], case["dil"],
                         case["pad_mode"], case["act"], 0.2 if case["act"] else 0.0, out_sp,
                         torch.zeros(ops.PROBE_SLOTS) if case["probe"] else None, res=_like(case["res"], yshape),
                         ring=(torch.zeros(8), 5) if case["ring"] else None, cout_used=case["cu"],
                         act_src=_like(case["act_src"], yshape), act_slope=0.2 if case["act_src"] else 0.0)
        assert tuple(y.shape) == yshape
        return {"calls": fake.calls, "queries": fake.queries, "prof": prof.log if with_prof else None,
                "amax_tag": hasattr(y, "_df_amax"), "last_amax": ops._LAST_CONV_AMAX[0] is not None,
                "actgrad": ops._LAST_ACTGRAD[0], "version": y._version}


FWD_YES = [(), FWD_QUERIES] + [(q,) for q in FWD_QUERIES] + [("tiny", "march"), ("split", "march"), ("s2c2", "s2"),
                                                             ("split", "tiny")]
CHANNELS = [(16, 3), (2, 16), (16, 16), (32, 64), (64, 128), (48, 32)]


def fwd_cases():
    cs = []
    # every library answer on every channel pair, below and above 512 output voxels
    for ch in CHANNELS:
        for isp in ((4, 8, 8), (8, 8, 12)):
            for yes in FWD_YES:
                cs.append(fwd_case(ch=ch, isp=isp, yes=yes))
    # kernel shape, stride and dilation
    for K in ((3, 3, 3), (1, 3, 3), (1, 1, 1)):
        for stride in (1, 2):
            for dil in (1, 2):
                for ch in ((2, 16), (32, 64)):
                    for yes in ((), FWD_QUERIES, ("s2c2",), ("s2",), ("s2d",), ("split",), ("s2c2", "s2")) if K[0] == 3 else ((), FWD_QUERIES):
                        for bias in ((True, False) if dil == 2 else (True,)):         # (the stride-2 dgrad has no bias)
                            cs.append(fwd_case(K=K, stride=stride, dil=dil, ch=ch, yes=yes, bias=bias))
    # each switch against the layers it moves: the flow head, the stride-2 encoder levels, a deep level, a 2-D residual
    layers = [dict(ch=(16, 3)), dict(ch=(3, 16), act_src="ok"), dict(ch=(2, 16), stride=2), dict(ch=(32, 64), stride=2),
              dict(ch=(64, 32), dil=2, bias=False), dict(ch=(16, 16)), dict(ch=(16, 16), isp=(8, 8, 12)),
              dict(K=(1, 3, 3), ch=(64, 128), res="ok")]
    for flags in [()] + [(s,) for s in SWITCHES]:
        for yes in (FWD_QUERIES, ("tiny", "march"), ("split", "march"), ("s2c2", "s2"), ("s2d", "split")):
            for kw in layers:
                cs.append(fwd_case(flags=flags, yes=yes, **kw))
    # the caller's arguments, one at a time and in the pairs the code combines
    variants = [dict(probe=False), dict(res="ok"), dict(res="bad"), dict(res="nc"), dict(ring=True), dict(ring=True, res="ok"),
                dict(cu=-1), dict(cu=0), dict(cu=-1, act_src="ok"), dict(act_src="ok"), dict(act_src="bad"),
                dict(act_src="nc"), dict(act_src="ok", act=1), dict(act_src="ok", probe=False), dict(bias=False),
                dict(act=1), dict(res="ok", probe=False), dict(isp=(4, 8, 10)), dict(isp=(4, 8, 10), act_src="ok")]
    for yes in ((), FWD_QUERIES, ("split", "march"), ("tiny",)):
        for ch in ((16, 3), (16, 16), (32, 64)):
            for v in variants:
                v = dict(v)
                if "cu" in v:                                 # a channel subset (-1) or all of them given explicitly (0)
                    v["cu"] = ch[1] + v["cu"] if ch[1] + v["cu"] > 0 else 1
                cs.append(fwd_case(ch=ch, yes=yes, **v))
    # the 2-D residual / ring epilogue and the 3x3 label
    for ch in ((64, 128), (48, 32), (16, 3)):
        for yes in ((), ("res",)):
            for v in (dict(), dict(res="ok"), dict(res="bad"), dict(res="nc"), dict(ring=True), dict(ring=True, res="ok"),
                      dict(ring=True, res="bad"), dict(res="ok", probe=False), dict(pad_mode=1), dict(pad=(0, 2, 2)),
                      dict(pad=(0, 1, 2)), dict(res="ok", act=1)):
                cs.append(fwd_case(K=(1, 3, 3), ch=ch, isp=(1, 8, 12), yes=yes, **v))
    # the tiny-volume rule: both sides of 512 voxels per image, of N x voxels = 8192 and of 64 output channels
    for ch in ((16, 16), (32, 64), (64, 128)):
        for isp, N in (((4, 8, 8), 1), ((4, 8, 8), 32), ((4, 8, 8), 33), ((8, 8, 8), 1), ((8, 8, 8), 16), ((8, 8, 8), 17),
                       ((8, 8, 10), 1), ((8, 8, 12), 1)):
            for cu in (None, ch[1] - 8):
                for flags in ((), ("_NO_TINYVOL",)):
                    for yes in (("split", "march"),):
                        cs.append(fwd_case(ch=ch, isp=isp, N=N, cu=cu, flags=flags, yes=yes))
    # the issued-product factors: the three forms of the split tiling, with and without a channel subset
    for pair in (0, 1, 2):
        for ch in ((16, 16), (12, 16), (48, 32)):
            for cu in (None, ch[1] - 8):
                for yes in ((("split",), ("split", "march")) if ch == (16, 16) else (("split",),)):
                    cs.append(fwd_case(ch=ch, isp=(8, 8, 12), cu=cu, pair=pair, yes=yes))
    return _unique(cs)


# ---------------------------------------------------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------------------------------------------------
def wgrad_case(K=(3, 3, 3), stride=1, ch=(16, 16), isp=(4, 8, 8), N=1, probes="xy", db=True, pmax=False, parts=None,
               min_vox=400000, det=False, out=False, flags=(), yes=(), pad_mode=0):
    if K[0] == 1 and K != (1, 1, 1):
        isp = (1,) + tuple(isp[1:])
    c = dict(K=tuple(K), stride=stride, ch=tuple(ch), isp=tuple(isp), N=N, probes=probes, db=db, pmax=pmax, parts=parts,
             min_vox=min_vox, det=det, out=out, flags=tuple(flags), yes=tuple(yes), pair=0,
             pad=tuple((k - 1) // 2 for k in K), pad_mode=pad_mode)
    c["id"] = _case_id("w", c, wgrad_case)
    return c


def run_wgrad(case, with_prof):
    Cin, Cout = case["ch"]
    N, K, stride = case["N"], case["K"], case["stride"]
    isp = case["isp"]
    T = K[0] * K[1] * K[2]
    fake, prof = FakeLib(case["yes"], 0, _geom(case)), (Prof() if with_prof else None)
    x5 = parts = None
    if case["parts"] is not None:                             # the operand is cat(nearest_up2(a), b), b with `parts` channels
        parts = (torch.empty((N, Cin - case["parts"]) + tuple(n // 2 for n in isp)), torch.empty((N, case["parts"]) + isp))
    else:
        x5 = torch.empty((N, Cin) + isp)
    out = torch.zeros((T, Cin, Cout)) if case["out"] else None
    raised = None
    with pytest.MonkeyPatch.context() as mp:
        _patched(mp, case, fake, prof)
        try:
            dw = ops.conv_wgrad_raw(x5, torch.empty((N, Cout) + _out_sp(isp, stride)), K, stride, case["pad"],
                                    case["pad_mode"], out=out,
                                    x_amax=torch.zeros(ops.PROBE_SLOTS) if "x" in case["probes"] else None,
                                    dy_amax=torch.zeros(ops.PROBE_SLOTS) if "y" in case["probes"] else None,
                                    db=torch.zeros(Cout) if case["db"] else None,
                                    dy_pmax=torch.zeros(N * Cout) if case["pmax"] else None, parts=parts)
            assert tuple(dw.shape) == (T, Cin, Cout) and (out is None or dw is out)
        except DfmirHipError:
            raised = "DfmirHipError"
    return {"calls": fake.calls, "queries": fake.queries, "prof": prof.log if with_prof else None, "raised": raised}


WGRAD_YES = [(), WGRAD_QUERIES, ("splitw",), ("s2c2",), ("s2",), ("s2c2", "s2"), ("splitw", "marchw"), ("splitw", "upw")]


def wgrad_cases():
    cs = []
    for ch in CHANNELS:
        for stride in (1, 2):
            for isp in ((4, 8, 8), (4, 8, 10)) if stride == 1 else ((4, 8, 8),):
                for yes in WGRAD_YES:
                    cs.append(wgrad_case(ch=ch, stride=stride, isp=isp, yes=yes))
            for K, isp in (((1, 3, 3), (1, 8, 32)), ((1, 3, 3), (1, 8, 8)), ((1, 1, 1), (4, 8, 8))):
                for yes in (WGRAD_QUERIES,):
                    cs.append(wgrad_case(K=K, ch=ch, stride=stride, isp=isp, yes=yes))
    # which probes the caller has
    for ch in ((16, 3), (16, 16), (64, 128)):
        for probes in ("", "x", "y"):
            for pmax, yes in ((False, ()), (True, WGRAD_QUERIES)):
                cs.append(wgrad_case(ch=ch, probes=probes, pmax=pmax, yes=yes))
    # bias gradient, per-plane maxima, the accumulation target and the deterministic mode on every kernel
    layers = [dict(ch=(16, 16), yes=("splitw",)), dict(ch=(16, 16), yes=("splitw", "marchw")), dict(ch=(16, 3), yes=("splitw",)),
              dict(ch=(2, 16), stride=2, yes=("s2c2",)), dict(ch=(32, 64), stride=2, yes=("s2",)), dict(ch=(48, 32)),
              dict(K=(1, 3, 3), ch=(64, 128), isp=(1, 8, 32)), dict(ch=(32, 64), pad_mode=1, yes=("splitw",))]
    for kw in layers:
        for db, pmax, det, out in ((False, False, False, False), (True, False, False, True), (False, True, False, True),
                                   (True, True, True, False), (False, False, True, True), (True, True, False, False)):
            cs.append(wgrad_case(db=db, pmax=pmax, det=det, out=out, **kw))
    # the two switches the weight gradient reads
    for flags in ((), ("_NO_TINY3D",), ("_NO_S2",)):
        for kw in (dict(ch=(2, 16), stride=2), dict(ch=(32, 64), stride=2), dict(ch=(2, 16))):
            for yes in (WGRAD_QUERIES, ("s2c2", "s2")):
                cs.append(wgrad_case(flags=flags, yes=yes, det=(yes == WGRAD_QUERIES), **kw))
    # parts: 2 skip channels (the fused threshold) and more; a = 2 x 4 x 4 = 32 low-resolution voxels per image
    for ch, nb in (((18, 16), 2), ((48, 32), 16), ((18, 4), 2), ((40, 64), 8)):
        for min_vox in (10, 32, 33, 400000):
            for yes in ((), ("upw",), ("splitw",), ("splitw", "upw")):
                for db, det in ((True, False), (False, True)) if min_vox in (32, 33) else ((True, False),):
                    cs.append(wgrad_case(ch=ch, parts=nb, min_vox=min_vox, yes=yes, db=db, det=det))
    return _unique(cs)


def _unique(cases):
    seen, out = set(), []
    for c in cases:
        if c["id"] not in seen:
            seen.add(c["id"])
            out.append(c)
    return out


def record(case):
    """The table's row of one case: the run without a profiler, plus what a profiler is told and the queries its label
    costs.  A profiler only brackets the launch: everything else must be the same in both runs."""
    run = run_fwd if case["id"][0] == "f" else run_wgrad
    plain, profd = run(case, False), run(case, True)
    for k in plain:
        if k not in ("prof", "queries"):
            assert plain[k] == profd[k], (case["id"], k)
    row = dict(plain, prof=profd["prof"], queries=[plain["queries"], profd["queries"]])
    return json.loads(json.dumps({k: v for k, v in row.items() if v not in (None, False, 0)}))   # (absent = None / False / 0)


def dumps(row):
    return json.dumps(row, sort_keys=True, separators=(",", ":"))


def ids_digest(cases):
    return hashlib.sha1("\n".join(c["id"] for c in cases).encode()).hexdigest()


# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table():
    """The file holds every distinct row once (`records`) and, per case in the order of the case list, its index (`rows`);
    `cases` is the SHA-1 of the case ids, so a changed case list cannot be read against the old indices."""
    with open(GOLDEN) as f:
        t = json.load(f)
    cases = fwd_cases() + wgrad_cases()
    assert t["cases"] == ids_digest(cases) and len(t["rows"]) == len(cases)
    return {"recorded_from": t["recorded_from"], "rows": {c["id"]: t["records"][i] for c, i in zip(cases, t["rows"])}}


@pytest.fixture(scope="module")
def rows():
    return {c["id"]: record(c) for c in fwd_cases() + wgrad_cases()}


def test_table_covers_exactly_the_case_list(table, rows):
    assert len(table["recorded_from"]) == 40
    assert list(table["rows"].keys()) == list(rows.keys())


def test_selection_launch_and_label_equal_the_recorded_table(table, rows):
    bad = []
    for cid, row in rows.items():
        gold = table["rows"][cid]
        got = dict(row, queries=gold["queries"])              # the queries are bounded below, everything else is equal
        if dumps(got) != dumps(gold):
            bad.append("%s\n  recorded %s\n  got      %s" % (cid, dumps(gold), dumps(got)))
    assert not bad, "%d of %d cases differ:\n%s" % (len(bad), len(rows), "\n".join(bad[:5]))


def test_no_more_library_queries_than_recorded(table, rows):
    more = [(cid, row["queries"], table["rows"][cid]["queries"]) for cid, row in rows.items()
            if any(a > b for a, b in zip(row["queries"], table["rows"][cid]["queries"]))]
    assert not more, more[:5]


def test_table_reaches_every_launch_entry_point(table):
    seen = set(call[0] for row in table["rows"].values() for call in row["calls"])
    assert seen >= set(FWD_ENTRIES + WGRAD_ENTRIES), set(FWD_ENTRIES + WGRAD_ENTRIES) - seen
    kinds = set(p[0] for row in table["rows"].values() for p in row.get("prof", ()))
    assert kinds >= {"conv3x3_L", "conv3ds_S", "conv3d_S", "conv_mfma_M", "conv3dt_small", "conv3dt_S", "wgrad3dt_S",
                     "wgrad3x3_L", "wgrad3ds_S", "wgrad3d_S", "conv_wgrad_M", "wgrad3dup_S"}, kinds


@pytest.mark.parametrize("switch", SWITCHES)
def test_every_switch_changes_some_row(table, switch):
    tag = "[%s]" % switch[4:]
    moved = [cid for cid, row in table["rows"].items()
             if tag in cid and cid.replace(tag, "[]", 1) in table["rows"]
             and dumps(dict(row, queries=0)) != dumps(dict(table["rows"][cid.replace(tag, "[]", 1)], queries=0))]
    assert moved, switch


def test_parts_without_the_split_wgrad_raise_and_nothing_else_does(table):
    raising = [cid for cid, row in table["rows"].items() if row.get("raised")]
    expect = [c["id"] for c in wgrad_cases() if c["parts"] is not None and "splitw" not in c["yes"]]
    assert expect and raising == expect
    assert all(table["rows"][cid]["raised"] == "DfmirHipError" and not table["rows"][cid]["calls"] for cid in raising)
