"""What the tools/probes/*_diag.py scripts share: their common flags, the QU30 workload they time on, the one timing loop,
the two-round bookkeeping, the rate annotation and the record's way out.  A probe keeps its docstring and bytes model,
its objects, the functions it times and its derived ratios."""
import json
import os
import sys
from functools import cached_property

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import omega_amd as oa  # noqa: E402
from omega_amd.meshgen import planar_hex  # noqa: E402

PEAK_TBS = 8.0
LAYER = 50.0  # m: the calm fields' layer thickness, and the bottom depth per level that goes with it
FLAGS = {"nx": int, "levels": int, "tracers": int, "nsub": int, "dt": float, "iters": int, "warmup": int, "local_order": str}


def add_common_args(ap, only_kernels=False, **defaults):
    """--nx --levels --tracers --nsub --dt --iters --warmup --local-order: a probe has those it gives a default for,
    and --out; only_kernels: --only-kernel and --only-kernels, one flag in two spellings (documents quote both)"""
    for name, kind in FLAGS.items():
        if name in defaults:
            ap.add_argument("--" + name.replace("_", "-"), type=kind, default=defaults.pop(name))
    assert not defaults, defaults
    if only_kernels:
        ap.add_argument("--only-kernel", "--only-kernels", dest="only_kernels", action="store_true")
    ap.add_argument("--out", default="")


def active_levels(lo, hi):
    return int(np.sum(np.where((lo >= 0) & (lo <= hi), hi - lo + 1, 0)))


class Qu30Rig:
    """The planar hexagon mesh of a.nx x a.nx cells at 30 km on one rank (halo 3), a.levels levels, a.tracers tracers
    (2 without the flag), with OceanState, Tracers, VertCoord and a Stream (.stream), from default_rng(2026).  The random
    draws come in one order -- layer ranges, thickness, velocity, tracers -- and what a probe draws afterwards from .rng
    follows.

      bottom   None (the mesh's default depth), "layers" (LAYER * levels) or a depth in m
      ragged   surface-attached layer ranges, the bottoms spread over the levels with a deep-ocean mode at 60 %; False:
               full columns, and nothing is drawn for them
      fields   "calm": thickness LAYER +- 1e-3, velocity +- 1e-3, on both time levels; "rough": thickness in (1, 50),
               velocity +- 0.05 (u="zero": none, and nothing is drawn), on time level 0 alone
      tracers  "uniform": all in (-1, 1); "stratified": T falling and S rising with depth under noise across the cells,
               the rest in (-1, 1); ((lo, hi), (lo, hi)): T and S uniform in these ranges, the rest in (-1, 1)
      ref_thickness   RefLayerThickness of the VertCoord set to LAYER
    reset() puts the fields back on their time levels."""

    def __init__(self, a, bottom=None, ragged=True, fields="calm", u="noise", tracers="uniform", ref_thickness=False):
        self.a = a
        self.K = K = a.levels
        self.NT = NT = getattr(a, "tracers", 2)
        self.P = oa.level_pitch(K)
        oa.device_init(0)
        depth = {} if bottom is None else {"bottom_depth": LAYER * K if bottom == "layers" else bottom}
        self.g = g = planar_hex(a.nx, a.nx, 30.0e3, **depth)
        n = int(g["nCells"])
        self.rng = rng = np.random.default_rng(2026)
        self.ranges = ()
        if ragged:
            self.ranges = (np.ones(n, np.int32), np.where(rng.random(n) < 0.6, K, rng.integers(5, K + 1, n)).astype(np.int32))
        self.decomp = oa.Decomp(oa.GlobalMesh(g), 1, 0, 3, local_order=getattr(a, "local_order", "global"))
        self.mesh = mesh = oa.HorzMesh(self.decomp, K)
        self.ns, self.nes, self.nc, self.ne = mesh.NCellsSize, mesh.NEdgesSize, mesh.NCellsAll, mesh.NEdgesAll
        ns, nes = self.ns, self.nes
        self.state = oa.OceanState(mesh, None, K, 2)
        self.tracers = oa.Tracers(mesh, None, K, NT, 2)
        if fields == "calm":
            self.h0, self.u0 = LAYER + rng.uniform(-1.0e-3, 1.0e-3, (ns, K)), rng.uniform(-1.0e-3, 1.0e-3, (nes, K))
        else:
            self.h0 = rng.uniform(1.0, 50.0, (ns, K))
            self.u0 = np.zeros((nes, K)) if u == "zero" else rng.uniform(-0.05, 0.05, (nes, K))
        self.time_levels = (0, 1) if fields == "calm" else (0,)
        if tracers == "uniform":
            self.tr0 = rng.uniform(-1.0, 1.0, (NT, ns, K))
        else:
            if tracers == "stratified":
                k = np.arange(K)[None, None, :]
                ts = [20.0 - 0.2 * k + rng.uniform(-0.5, 0.5, (1, ns, K)), 34.0 + 0.02 * k + rng.uniform(-0.1, 0.1, (1, ns, K))]
            else:
                ts = [rng.uniform(lo, hi, (1, ns, K)) for lo, hi in tracers]
            self.tr0 = np.concatenate(ts + [rng.uniform(-1.0, 1.0, (NT - 2, ns, K))])  # (an empty draw takes nothing)
        self.reset()
        self.vc = oa.VertCoord(mesh, K, 1026.0, "Uniform", *self.ranges, decomp=self.decomp)
        if ref_thickness:
            self.vc.set("RefLayerThickness", np.full((ns, K), LAYER))

    @cached_property
    def stream(self):
        """made when first asked for: a probe asks where its records' processes made theirs, after its own objects, so
        that the order of allocations, and with it where the arrays lie, stays what it was"""
        return oa.Stream()

    def reset(self):
        for lvl in self.time_levels:
            self.state.copy_to_device(self.h0, self.u0, lvl)
            self.tracers.copy_to_device(self.tr0, lvl)

    @property
    def active_cell_levels(self):
        return active_levels(self.vc.get("MinLayerCell")[: self.nc], self.vc.get("MaxLayerCell")[: self.nc])

    @property
    def active_edge_levels(self):
        return active_levels(self.vc.get("MinLayerEdgeBot")[: self.ne], self.vc.get("MaxLayerEdgeTop")[: self.ne])

    def time(self, fns, iters=None, warmup=None, **kw):
        """timed() on the rig's stream, a.iters rounds after a.warmup unless told otherwise"""
        return timed(self.stream, fns, self.a.iters if iters is None else iters,
                     self.a.warmup if warmup is None else warmup, **kw)

    def tendencies(self, cfg, count=1):
        """the AuxiliaryState and `count` Tendencies of a config"""
        aux = oa.AuxiliaryState(self.mesh, None, self.K, self.NT)
        aux.set_options(cfg.FluxThicknessUpwind, cfg.FluxTracerUpwind, cfg.WindInterpIsotropic)
        return (aux,) + tuple(oa.Tendencies(self.mesh, self.K, self.NT, cfg) for _ in range(count))


def timed(stream, fns, iters, warmup, before_each=None, before=None, every=0, successive=False, device=oa):
    """One dict of ms_median / ms_min / ms_max / ms_p25 / ms_p75 per fn.  After `warmup` untimed rounds come `iters`
    timed ones; in a round every fn is called once, in order, between an event pair of its own on `stream`: the fns
    alternate in one loop, and a number is the device time of the call, not of the gap before it.  before_each runs ahead
    of every call, outside its pair.  before runs ahead of round 0 and of every `every`-th round after it (0: of round 0
    alone), on a drained device.  Stream and device are drained before the first pair and after the last.
    successive (one fn, nothing run in between): one event after each call and one ahead of the first, a number being
    the span between two of them, the gap before the launch included -- column_diag.py and tridiag_diag.py, whose
    records were taken so (profiles/EXPERIMENTS.md).
    device: what gives Event() and device_synchronize() (omega_amd)."""
    def drain():
        stream.synchronize()
        device.device_synchronize()

    for _ in range(warmup):
        for fn in fns:
            if before_each:
                before_each()
            fn()
    drain()
    if successive:
        assert len(fns) == 1 and not before_each and not before
        evs = [device.Event() for _ in range(iters + 1)]
        evs[0].record(stream)
        for e in evs[1:]:
            fns[0]()
            e.record(stream)
        pairs = [[span] for span in zip(evs, evs[1:])]
    else:
        pairs = [[(device.Event(), device.Event()) for _ in fns] for _ in range(iters)]
        for r, row in enumerate(pairs):
            if before and (r == 0 or (every and r % every == 0)):
                drain()
                before()
            for fn, (e0, e1) in zip(fns, row):
                if before_each:
                    before_each()
                e0.record(stream)
                fn()
                e1.record(stream)
    drain()
    out = []
    for j in range(len(fns)):
        per = np.array([row[j][0].elapsed_ms(row[j][1]) for row in pairs])
        out.append({"ms_median": float(np.median(per)), "ms_min": float(per.min()), "ms_max": float(per.max()),
                    "ms_p25": float(np.percentile(per, 25)), "ms_p75": float(np.percentile(per, 75))})
    return out


def twice(calls, names, time_round):
    """Every case twice: time_round() -> one entry per name, kept as calls[<name>_1] and calls[<name>_2].  -> names"""
    for rnd in ("1", "2"):
        for name, t in zip(names, time_round()):
            calls[f"{name}_{rnd}"] = t
    return list(names)


def summarise(calls, keys):
    """<key>_ms: the mean of the two rounds' medians; <key>_spread_ms: their difference, the run's own spread"""
    s = {}
    for key in keys:
        m1, m2 = calls[key + "_1"]["ms_median"], calls[key + "_2"]["ms_median"]
        s[key + "_ms"], s[key + "_spread_ms"] = 0.5 * (m1 + m2), abs(m1 - m2)
    return s


def with_rate(t, nbytes):
    """the bytes model's rate at the median, and its share of the HBM peak"""
    t["algorithmic_GB"] = nbytes / 1.0e9
    t["TBs"] = t["algorithmic_GB"] / t["ms_median"]
    t["share_of_8TBs"] = t["TBs"] / PEAK_TBS
    return t


def emit(res, out=""):
    """the record as one JSON line on stdout, and in `out` when given"""
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")
