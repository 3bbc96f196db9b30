"""SplitExplicitStepper (SplitExplicitStepper.h) timed with device events at QU30 size: the workload of
tools/probes/barotropic_diag.py (462 400 cells x 80 levels in k-d order, surface-attached layer ranges, 6 tracers) from a
calm state.  Times, each as the median of --iters in one process: the three BarotropicMode calls of the step
(computeResidualForcing, transportVelocity, advanceVelocity), the two reference-structured group calls of steps 6 and 7
with their updates, one Split-Explicit step at --nsub, one stage-fused RungeKutta4 step and one fused RHS evaluation.
Prints one JSON line and writes it to --out.

Bytes models (`active` = the edge-levels of the ranges, `other` = the remaining edge-levels below K):
  residual forcing   the forcing sweep, 8 B per active edge-level + 8 B per active cell-level, + per edge 12 B x MaxEdges2
                     of tables + 52 B (mask, cells, 1/dc, slot count, mean read, forcing written)
  transport          16 B per active edge-level (BclVelocity read, u written) + 16 B per other (u read, u written) + 16 B
                     per edge
  advance            24 B per active edge-level (BclVelocity and the tendency read, u written) + 24 B per other (u and the
                     tendency read, u written) + 16 B per edge

   python tools/probes/split_explicit_diag.py [--nx 680] [--levels 80] [--nsub 30] [--dt 600] [--iters 50] [--warmup 10]
          [--local-order kd] [--out FILE]
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
    stream = oa.Stream()
    pitch = oa.level_pitch(K)

    lo, hi = vc.get("MinLayerCell")[: mesh.NCellsAll], vc.get("MaxLayerCell")[: mesh.NCellsAll]
    cactive = int(np.sum(np.where((lo >= 0) & (lo <= hi), hi - lo + 1, 0)))
    elo, ehi = vc.get("MinLayerEdgeBot")[: mesh.NEdgesAll], vc.get("MaxLayerEdgeTop")[: mesh.NEdgesAll]
    eactive = int(np.sum(np.where((elo >= 0) & (elo <= ehi), ehi - elo + 1, 0)))
    nc, ne, me2 = mesh.NCellsAll, mesh.NEdgesAll, mesh.MaxEdges2
    other = ne * K - eactive
    nbytes = {"residual_forcing": 8 * eactive + 8 * cactive + ne * (12 * me2 + 52),
              "transport": 16 * eactive + 16 * other + 16 * ne, "advance": 24 * eactive + 24 * other + 16 * ne}

    def timed(fn, before=None, every=0):
        """`before` runs after the warm-up and then before every `every`-th timed call (0: only once), outside the
        event pairs"""
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

    res = {"probe": "split_explicit_diag", "ncells": nc, "nedges": ne, "levels": K, "tracers": NT, "nsub": a.nsub,
           "dt": a.dt, "local_order": a.local_order, "active_cell_levels": cactive, "active_edge_levels": eactive,
           "iters": a.iters, "peak_TBs": PEAK_TBS, "calls": {}}
    rhs = timed(lambda: tend.compute_all_tendencies(state, aux, tracers, stream=stream))
    res["calls"]["rhs_fused"] = rhs
    # the three calls, on the fields one step leaves behind
    dt = oa.coeff_seconds(1.0, a.dt)
    hp, up, un = state.device_ptr(0, 0), state.device_ptr(1, 0), state.device_ptr(1, 1)
    vt = tend.device_ptr(1)[0]
    bm.split_velocity(hp, up, with_ssh=True, stream=stream)
    calls = {"residual_forcing": lambda: bm.compute_residual_forcing(hp, vt, stream=stream),
             "transport": lambda: bm.transport_velocity(up, un, stream=stream),
             "advance": lambda: bm.advance_velocity(up, vt, dt, un, stream=stream)}
    for name, fn in calls.items():
        t = timed(fn)
        t["algorithmic_GB"] = nbytes[name] / 1.0e9
        t["TBs"] = t["algorithmic_GB"] / t["ms_median"]
        t["share_of_8TBs"] = t["TBs"] / PEAK_TBS
        res["calls"][name] = t
    # steps 6 and 7 of the step: the reference-structured group calls with their updates
    res["calls"]["thickness_group"] = timed(lambda: tend.compute_thickness_tendencies(state, aux, 0, 1, stream=stream))
    res["calls"]["tracer_group"] = timed(lambda: tend.compute_tracer_tendencies(state, aux, tracers, 0, 0, 1, stream=stream))
    res["calls"]["subcycle"] = timed(lambda: bm.subcycle(a.nsub, dt / a.nsub, stream=stream),
                                     before=lambda: (bm.set("SSH", np.zeros(ns)), bm.set("BtrVelocity", np.zeros(nes))))
    # whole steps
    se = oa.TimeStepper("Split-Explicit", a.dt, tend, aux, mesh, None, tracers)
    se.attach_barotropic(bm, a.nsub)
    # (the calm start again every 5 steps: one forward evaluation per long step does not hold the layers' own gravity
    # waves of this workload, which has no layered pressure force, for 60 steps)
    res["calls"]["split_explicit_step"] = timed(lambda: se.do_step(state, stream=stream), before=reset, every=5)
    h, u = state.copy_to_host(0)
    res["state_finite_after_split_explicit_steps"] = bool(np.isfinite(h[:nc]).all() and np.isfinite(u[:ne]).all())
    res["max_abs_u_after_split_explicit_steps"] = float(np.abs(u[:ne]).max())
    rk = oa.TimeStepper("RungeKutta4", a.dt, tend, aux, mesh, None, tracers)
    res["calls"]["rk4_step"] = timed(lambda: rk.do_step(state, stream=stream), before=reset, every=5)
    c, r = res["calls"], rhs["ms_median"]
    for t in c.values():
        t["fraction_of_rhs"] = t["ms_median"] / r
    step = c["split_explicit_step"]["ms_median"]
    groups = c["thickness_group"]["ms_median"] + c["tracer_group"]["ms_median"]
    res["summary"] = {"step_over_rhs": step / r, "step_over_rk4_step": step / c["rk4_step"]["ms_median"],
                      "share_of_step_1": r / step, "share_of_group_calls": groups / step,
                      "share_of_subcycle": c["subcycle"]["ms_median"] / step,
                      # a velocity-only + thickness/tracer-only fused pair costs at least one fused RHS between them
                      "upper_bound_saving_of_a_fused_pair_ms": groups,
                      "step_with_a_fused_pair_at_best_over_rhs": (step - groups) / r}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
