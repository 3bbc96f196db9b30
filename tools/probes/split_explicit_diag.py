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

import numpy as np
from probe_rig import PEAK_TBS, Qu30Rig, add_common_args, emit, oa, with_rate


def main(argv=None):
    ap = argparse.ArgumentParser()
    add_common_args(ap, nx=680, levels=80, tracers=6, nsub=30, dt=600.0, iters=50, warmup=10, local_order="kd")
    a = ap.parse_args(argv)
    w = Qu30Rig(a, bottom="layers")
    K, NT, mesh, ns, nes, state, tracers, vc = w.K, w.NT, w.mesh, w.ns, w.nes, w.state, w.tracers, w.vc
    bm = oa.BarotropicMode(mesh, vc)
    aux, tend = w.tendencies(oa.default_config())
    stream = w.stream

    cactive = w.active_cell_levels
    eactive = w.active_edge_levels
    nc, ne, me2 = mesh.NCellsAll, mesh.NEdgesAll, mesh.MaxEdges2
    other = ne * K - eactive
    nbytes = {"residual_forcing": 8 * eactive + 8 * cactive + ne * (12 * me2 + 52),
              "transport": 16 * eactive + 16 * other + 16 * ne, "advance": 24 * eactive + 24 * other + 16 * ne}

    res = {"probe": "split_explicit_diag", "ncells": nc, "nedges": ne, "levels": K, "tracers": NT, "nsub": a.nsub,
           "dt": a.dt, "local_order": a.local_order, "active_cell_levels": cactive, "active_edge_levels": eactive,
           "iters": a.iters, "peak_TBs": PEAK_TBS, "calls": {}}
    rhs = w.time([lambda: tend.compute_all_tendencies(state, aux, tracers, stream=stream)])[0]
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
        res["calls"][name] = with_rate(w.time([fn])[0], nbytes[name])
    # steps 6 and 7 of the step: the reference-structured group calls with their updates
    res["calls"]["thickness_group"] = w.time([lambda: tend.compute_thickness_tendencies(state, aux, 0, 1, stream=stream)])[0]
    res["calls"]["tracer_group"] = w.time([lambda: tend.compute_tracer_tendencies(state, aux, tracers, 0, 0, 1, stream=stream)])[0]
    res["calls"]["subcycle"] = w.time([lambda: bm.subcycle(a.nsub, dt / a.nsub, stream=stream)],
                                       before=lambda: (bm.set("SSH", np.zeros(ns)), bm.set("BtrVelocity", np.zeros(nes))))[0]
    # whole steps
    se = oa.TimeStepper("Split-Explicit", a.dt, tend, aux, mesh, None, tracers)
    se.attach_barotropic(bm, a.nsub)
    # (the calm start again every 5 steps: one forward evaluation per long step does not hold the layers' own gravity
    # waves of this workload, which has no layered pressure force, for 60 steps)
    res["calls"]["split_explicit_step"] = w.time([lambda: se.do_step(state, stream=stream)], before=w.reset, every=5)[0]
    h, u = state.copy_to_host(0)
    res["state_finite_after_split_explicit_steps"] = bool(np.isfinite(h[:nc]).all() and np.isfinite(u[:ne]).all())
    res["max_abs_u_after_split_explicit_steps"] = float(np.abs(u[:ne]).max())
    rk = oa.TimeStepper("RungeKutta4", a.dt, tend, aux, mesh, None, tracers)
    res["calls"]["rk4_step"] = w.time([lambda: rk.do_step(state, stream=stream)], before=w.reset, every=5)[0]
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
    emit(res, a.out)


if __name__ == "__main__":
    main()
