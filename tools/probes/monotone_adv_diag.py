"""MonotoneAdv::addTracerTend (MonotoneAdv.h) at QU30 size, timed with device events: the workload of
tools/probes/transport_diag.py (462 400 cells x 80 levels in k-d order, surface-attached layer ranges, 6 tracers).
Alternated in one process, each as the median of --iters after --warmup, every case timed twice (the difference of the
two medians is its own run-to-run spread):
  transport_centred_1 / _2     compute_transport_tendencies with the Tendencies' own centred advection term (the path
                               without this class)
  transport_no_adv_mono_1 / _2 the same call with TracerHorzAdvTendencyEnable off, followed by add_tracers
  mono_only_1 / _2             add_tracers alone (two launches)
  step_plain_1 / _2            one Split-Explicit step at --nsub, nothing attached
  step_mono_1 / _2             one Split-Explicit step with the MonotoneAdv attached (and the advection term off)
Prints one JSON line and writes it to --out.

Bytes model per cell-level of a hexagon mesh (3 edge rows per cell), 8 B values, every row counted once per launch:
  pass 1   reads hOld, hNew, 3 u: 40; per tracer reads phi, writes ScaleIn and ScaleOut: 24
  pass 2   reads hOld, 3 u: 32; per tracer reads phi, ScaleIn, ScaleOut, reads and writes Tend: 40
  -> 72 + 64 NT for the call; the transport call it follows is 40 + 40 NT with the hyperdiffusion term on
     (tools/probes/transport_diag.py), with or without its advection term.

   python tools/probes/monotone_adv_diag.py [--nx 680] [--levels 80] [--tracers 6] [--nsub 30] [--dt 600] [--iters 50]
          [--warmup 10] [--local-order kd] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=680)
    ap.add_argument("--levels", type=int, default=80)
    ap.add_argument("--tracers", type=int, default=6)
    ap.add_argument("--nsub", type=int, default=30)
    ap.add_argument("--dt", type=float, default=600.0)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--local-order", default="kd")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    K, NT = a.levels, a.tracers
    oa.device_init(0)
    layer = 50.0
    g = planar_hex(a.nx, a.nx, 30.0e3, bottom_depth=layer * K)
    n = int(g["nCells"])
    rng = np.random.default_rng(2026)
    min_level = np.ones(n, np.int32)
    max_level = np.where(rng.random(n) < 0.6, K, rng.integers(5, K + 1, n)).astype(np.int32)
    decomp = oa.Decomp(oa.GlobalMesh(g), 1, 0, 3, local_order=a.local_order)
    mesh = oa.HorzMesh(decomp, K)
    ns, nes = mesh.NCellsSize, mesh.NEdgesSize
    state = oa.OceanState(mesh, None, K, 2)
    tracers = oa.Tracers(mesh, None, K, NT, 2)
    h0, u0 = layer + rng.uniform(-1.0e-3, 1.0e-3, (ns, K)), rng.uniform(-1.0e-3, 1.0e-3, (nes, K))
    tr0 = rng.uniform(-1.0, 1.0, (NT, ns, K))

    def reset():
        for lvl in (0, 1):
            state.copy_to_device(h0, u0, lvl)
            tracers.copy_to_device(tr0, lvl)

    reset()
    vc = oa.VertCoord(mesh, K, 1026.0, "Uniform", min_level, max_level, decomp=decomp)
    bm = oa.BarotropicMode(mesh, vc)
    cfg = oa.default_config()
    aux = oa.AuxiliaryState(mesh, None, K, NT)
    aux.set_options(cfg.FluxThicknessUpwind, cfg.FluxTracerUpwind, cfg.WindInterpIsotropic)
    tend = oa.Tendencies(mesh, K, NT, cfg)
    tend_no_adv = oa.Tendencies(mesh, K, NT, oa.default_config(TracerHorzAdvTendencyEnable=0))
    mono = oa.MonotoneAdv(mesh, K, NT, bool(cfg.FluxThicknessUpwind))
    stream = oa.Stream()
    nc = mesh.NCellsAll
    h_old, h_new, u_new = state.device_ptr(0, 0), state.device_ptr(0, 1), state.device_ptr(1, 1)

    def timed(fn, before=None, every=0):
        for _ in range(a.warmup):
            fn()
        stream.synchronize()
        evs = [[oa.Event() for _ in range(2)] for _ in range(a.iters)]
        for i, (e0, e1) in enumerate(evs):
            if before and (i == 0 or (every and i % every == 0)):
                stream.synchronize()
                before()
            e0.record(stream)
            fn()
            e1.record(stream)
        stream.synchronize()
        per = np.array([e0.elapsed_ms(e1) for e0, e1 in evs])
        return {"ms_median": float(np.median(per)), "ms_min": float(per.min()), "ms_max": float(per.max())}

    def centred():
        tend.compute_transport_tendencies(state, aux, tracers, 0, 0, 1, stream=stream)

    def mono_only():
        mono.add_tracers(tend_no_adv.device_ptr(2)[0], h_old, h_new, u_new, tracers.device_ptr(0), NT, a.dt, stream=stream)

    def no_adv_mono():
        tend_no_adv.compute_transport_tendencies(state, aux, tracers, 0, 0, 1, stream=stream)
        mono_only()

    hyper = bool(cfg.TracerHyperDiffTendencyEnable)
    cell_levels = nc * K
    transport_bytes = cell_levels * (40 + (40 if hyper else 16) * NT)
    mono_bytes = cell_levels * (72 + 64 * NT)
    res = {"probe": "monotone_adv_diag", "ncells": nc, "nedges": mesh.NEdgesAll, "levels": K, "tracers": NT, "nsub": a.nsub,
           "dt": a.dt, "local_order": a.local_order, "iters": a.iters, "warmup": a.warmup, "peak_TBs": PEAK_TBS,
           "tracer_hyperdiffusion": hyper, "bytes_per_cell_level": {"mono": 72 + 64 * NT, "transport": 40 + (40 if hyper else 16) * NT},
           "calls": {}}
    c = res["calls"]
    for rnd in ("1", "2"):
        c["transport_centred_" + rnd] = timed(centred)
        c["transport_no_adv_mono_" + rnd] = timed(no_adv_mono)
        c["mono_only_" + rnd] = timed(mono_only)
    for name, nb in (("transport_centred", transport_bytes), ("transport_no_adv_mono", transport_bytes + mono_bytes),
                     ("mono_only", mono_bytes)):
        for rnd in ("_1", "_2"):
            t = c[name + rnd]
            t["algorithmic_GB"] = nb / 1.0e9
            t["TBs"] = t["algorithmic_GB"] / t["ms_median"]
            t["share_of_8TBs"] = t["TBs"] / PEAK_TBS
    # whole steps (the calm start again every 5 steps, as in transport_diag.py)
    plain = oa.TimeStepper("Split-Explicit", a.dt, tend, aux, mesh, None, tracers)
    plain.attach_barotropic(bm, a.nsub)
    limited = oa.TimeStepper("Split-Explicit", a.dt, tend_no_adv, aux, mesh, None, tracers)
    limited.attach_barotropic(bm, a.nsub)
    limited.attach_monotone_adv(mono)
    for rnd in ("1", "2"):
        c["step_plain_" + rnd] = timed(lambda: plain.do_step(state, stream=stream), before=reset, every=5)
        c["step_mono_" + rnd] = timed(lambda: limited.do_step(state, stream=stream), before=reset, every=5)
    stream.synchronize()
    si = mono.get("ScaleIn")[:, :nc]
    res["scale_in_finite"] = bool(np.isfinite(si).all())
    res["scale_in_limited_fraction"] = float((si < 1.0).mean())

    def mean(name):
        return 0.5 * (c[name + "_1"]["ms_median"] + c[name + "_2"]["ms_median"])

    def spread(name):
        return abs(c[name + "_1"]["ms_median"] - c[name + "_2"]["ms_median"])

    res["summary"] = {k + "_ms": mean(k) for k in ("transport_centred", "transport_no_adv_mono", "mono_only", "step_plain", "step_mono")}
    res["summary"].update({k + "_spread_ms": spread(k) for k in ("transport_centred", "transport_no_adv_mono", "mono_only", "step_plain", "step_mono")})
    s = res["summary"]
    s["limited_over_centred_transport"] = s["transport_no_adv_mono_ms"] / s["transport_centred_ms"]
    s["step_mono_over_step_plain"] = s["step_mono_ms"] / s["step_plain_ms"]
    s["mono_only_TBs"] = mono_bytes / 1.0e9 / s["mono_only_ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f_:
            f_.write(line + "\n")


if __name__ == "__main__":
    main()
