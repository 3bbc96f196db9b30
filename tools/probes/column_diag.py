"""The fused column pass (VertCoord::computeColumn) against the four launches it replaces (computePressure ->
Eos::computeSpecVol -> computeZHeight -> computeGeopotential), timed with device events at QU30 size:
462 400 cells x 80 levels, TEOS-10, realistic random layer ranges.  Prints one JSON line (ms per call, algorithmic
bytes, share of 8 TB/s) and writes it to --out when given.

   python tools/probes/column_diag.py [--nx 680] [--levels 80] [--iters 50] [--warmup 10] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import omega_amd as oa  # noqa: E402
from omega_amd.meshgen import planar_hex  # noqa: E402

PEAK_TBS = 8.0
BYTES_FUSED = 72      # per cell-level: reads h, T, S; writes PInt, PMid, SpecVol, ZInt, ZMid, GeoMid
BYTES_SEQUENCE = 104  # pressure 24 + specific volume 32 + z-height 32 + geopotential 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=680)
    ap.add_argument("--levels", type=int, default=80)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--eos", default="teos10")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    K = a.levels
    oa.device_init(0)
    g = planar_hex(a.nx, a.nx, 30.0e3)
    n = int(g["nCells"])
    rng = np.random.default_rng(2026)
    # realistic ranges: surface-attached columns, bottoms spread over the levels with a deep-ocean mode
    min_level = np.ones(n, np.int32)
    max_level = np.where(rng.random(n) < 0.6, K, rng.integers(5, K + 1, n)).astype(np.int32)
    gm = oa.GlobalMesh(g)
    decomp = oa.Decomp(gm, 1, 0, 3)
    mesh = oa.HorzMesh(decomp, K)
    ns = mesh.NCellsSize
    state = oa.OceanState(mesh, None, K, 2)
    tracers = oa.Tracers(mesh, None, K, 2, 2)
    state.copy_to_device(rng.uniform(1.0, 50.0, (ns, K)), np.zeros((mesh.NEdgesSize, K)), 0)
    tracers.copy_to_device(np.stack([rng.uniform(-2.0, 30.0, (ns, K)), rng.uniform(30.0, 38.0, (ns, K))]), 0)
    vc = oa.VertCoord(mesh, K, 1026.0, "Uniform", min_level, max_level, decomp=decomp)
    eos = oa.Eos(mesh, K, a.eos)
    ps, tidal, sal = (oa.DeviceBuffer(rng.uniform(-1.0, 1.0, ns)) for _ in range(3))
    stream = oa.Stream()
    hp = state.device_ptr(0)
    tp, sp = oa.tracer_rows_ptr(tracers, 0), oa.tracer_rows_ptr(tracers, 1)
    pmid, svp = vc.device_ptr("PressureMid"), eos.device_ptr("SpecVol")

    def fused():
        vc.compute_column(state, tracers, eos, ps.ptr, tidal.ptr, sal.ptr, stream=stream)

    def sequence():
        vc.compute_pressure(hp, ps.ptr, stream=stream)
        eos.compute_spec_vol(tp, sp, pmid, p_scale=1.0e-4, stream=stream)
        vc.compute_zheight(hp, svp, stream=stream)
        vc.compute_geopotential(tidal.ptr, sal.ptr, stream=stream)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        stream.synchronize()
        evs = [oa.Event() for _ in range(a.iters + 1)]
        evs[0].record(stream)
        for i in range(a.iters):
            fn()
            evs[i + 1].record(stream)
        stream.synchronize()
        per = np.array([evs[i].elapsed_ms(evs[i + 1]) for i in range(a.iters)])
        return float(np.median(per)), float(per.min()), float(per.max())

    cell_levels = mesh.NCellsAll * K
    res = {"probe": "column_diag", "cells": mesh.NCellsAll, "levels": K, "eos": a.eos, "iters": a.iters,
           "active_fraction": float(np.mean(max_level - min_level + 1) / K)}
    # alternate the two twice: a drift of the clock shows up as a difference between the rounds
    for rnd in (0, 1):
        for name, fn, b in (("fused", fused, BYTES_FUSED), ("sequence", sequence, BYTES_SEQUENCE)):
            med, lo, hi = timed(fn)
            gb = cell_levels * b / 1.0e9
            res[f"{name}_r{rnd}"] = {"ms_median": med, "ms_min": lo, "ms_max": hi, "algorithmic_GB": gb,
                                     "TBs": gb / med, "share_of_8TBs": gb / med / PEAK_TBS}
    res["fused_over_sequence"] = res["fused_r1"]["ms_median"] / res["sequence_r1"]["ms_median"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
