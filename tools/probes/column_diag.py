"""The fused column pass (VertCoord::computeColumn) against the four launches it replaces (computePressure ->
Eos::computeSpecVol -> computeZHeight -> computeGeopotential), timed with device events at QU30 size:
462 400 cells x 80 levels, TEOS-10, realistic random layer ranges.  Prints one JSON line (ms per call, algorithmic
bytes, share of 8 TB/s) and writes it to --out when given.

   python tools/probes/column_diag.py [--nx 680] [--levels 80] [--iters 50] [--warmup 10] [--out FILE]
"""
import argparse

import numpy as np
from probe_rig import Qu30Rig, add_common_args, emit, oa, with_rate

BYTES_FUSED = 72      # per cell-level: reads h, T, S; writes PInt, PMid, SpecVol, ZInt, ZMid, GeoMid
BYTES_SEQUENCE = 104  # pressure 24 + specific volume 32 + z-height 32 + geopotential 16


def main(argv=None):
    ap = argparse.ArgumentParser()
    add_common_args(ap, nx=680, levels=80, iters=50, warmup=10)
    ap.add_argument("--eos", default="teos10")
    a = ap.parse_args(argv)
    # realistic ranges: surface-attached columns, bottoms spread over the levels with a deep-ocean mode
    w = Qu30Rig(a, fields="rough", u="zero", tracers=((-2.0, 30.0), (30.0, 38.0)))
    K, state, tracers, vc = w.K, w.state, w.tracers, w.vc
    eos = oa.Eos(w.mesh, K, a.eos)
    ps, tidal, sal = (oa.DeviceBuffer(w.rng.uniform(-1.0, 1.0, w.ns)) for _ in range(3))
    stream = w.stream
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

    min_level, max_level = w.ranges
    res = {"probe": "column_diag", "cells": w.nc, "levels": K, "eos": a.eos, "iters": a.iters,
           "active_fraction": float(np.mean(max_level - min_level + 1) / K)}
    # alternate the two twice: a drift of the clock shows up as a difference between the rounds
    for rnd in (0, 1):
        for name, fn, b in (("fused", fused, BYTES_FUSED), ("sequence", sequence, BYTES_SEQUENCE)):
            res[f"{name}_r{rnd}"] = with_rate(w.time([fn], successive=True)[0], w.nc * K * b)
    res["fused_over_sequence"] = res["fused_r1"]["ms_median"] / res["sequence_r1"]["ms_median"]
    emit(res, a.out)


if __name__ == "__main__":
    main()
