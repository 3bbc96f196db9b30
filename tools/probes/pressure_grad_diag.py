"""PressureGrad (PressureGrad.h) timed with device events at QU30 size: 462 400 cells x 80 levels in k-d order,
surface-attached layer ranges as in tools/probes/vert_mix_diag.py.  Times the pressure-gradient kernel alone, the
column pass alone, and -- alternating in one loop, in the same process -- the plain RHS (SSH gradient off), the layered
RHS (column pass + RHS + term: computeAllTendencies with the PressureGrad attached) and one RK4 step of each (plain:
stage updates fused; layered: stage updates as separate kernels).  Prints one JSON line and writes it to --out.

Algorithmic bytes of the term: 24 B per cell-level (PressureMid, GeopotentialMid, SpecVol, each row fetched once)
+ 16 B per active edge-level (the tendency read and written); on a hexagon mesh ~ 72 B per cell-level.

   python tools/probes/pressure_grad_diag.py [--nx 680] [--levels 80] [--tracers 6] [--iters 50] [--warmup 10]
          [--local-order kd] [--only-kernel] [--out FILE]
(--only-kernel: just the kernel, a few launches: the form to run under rocprofv3 --pmc or --kernel-trace.)
"""
import argparse

import numpy as np
from probe_rig import PEAK_TBS, Qu30Rig, add_common_args, emit, oa, with_rate


def main(argv=None):
    ap = argparse.ArgumentParser()
    add_common_args(ap, only_kernels=True, nx=680, levels=80, tracers=6, iters=50, warmup=10, local_order="kd")
    a = ap.parse_args(argv)
    w = Qu30Rig(a, fields="rough", tracers=((-2.0, 30.0), (30.0, 38.0)))
    K, NT, mesh, nes, state, tracers, vc = w.K, w.NT, w.mesh, w.nes, w.state, w.tracers, w.vc
    eos = oa.Eos(mesh, K, "teos10")
    pg = oa.PressureGrad(mesh, vc, eos)
    stream = w.stream
    hp, trp = state.device_ptr(0, 0), tracers.device_ptr(0)
    pg.update_column(hp, trp, NT, stream=stream)
    stream.synchronize()
    scratch = oa.DeviceBuffer(np.zeros((nes, oa.level_pitch(K))))

    eactive = w.active_edge_levels
    cell_levels = mesh.NCellsAll * K
    term_bytes = 24 * cell_levels + 16 * eactive
    res = {"probe": "pressure_grad_diag", "ncells": mesh.NCellsAll, "nedges": mesh.NEdgesAll, "levels": K, "tracers": NT,
           "local_order": a.local_order, "active_edge_levels": eactive, "iters": a.iters, "peak_TBs": PEAK_TBS,
           "term_algorithmic_GB": term_bytes / 1.0e9, "term_B_per_cell_level": term_bytes / cell_levels, "calls": {}}

    def term():
        pg.compute(scratch.ptr, stream=stream)

    if a.only_kernels:
        for _ in range(a.iters):
            term()
        stream.synchronize()
        emit(res)
        return

    res["calls"]["pressure_grad"] = with_rate(w.time([term])[0], term_bytes)
    res["calls"]["column_pass"] = with_rate(w.time([lambda: pg.update_column(hp, trp, NT, stream=stream)])[0], 72 * cell_levels)

    # the RHS with and without the layered term, same state, same process, alternating
    aux, plain, layered = w.tendencies(oa.default_config(SSHTendencyEnable=0), 2)
    layered.attach_pressure_grad(pg)
    rhs = w.time([lambda: plain.compute_all_tendencies(state, aux, tracers, stream=stream),
                 lambda: layered.compute_all_tendencies(state, aux, tracers, stream=stream)])
    res["calls"]["rhs_plain"], res["calls"]["rhs_layered"] = rhs
    res["rhs_layered_over_plain"] = rhs[1]["ms_median"] / rhs[0]["ms_median"]
    # one RK4 step of each (a small step from the same start every time would need a state copy: the steps run on, the
    # fields stay smooth for the few steps timed)
    st_plain = oa.TimeStepper("RungeKutta4", 1.0, plain, aux, mesh, None, tracers)
    st_layered = oa.TimeStepper("RungeKutta4", 1.0, layered, aux, mesh, None, tracers)
    steps = w.time([lambda: st_plain.do_step(state, stream=stream), lambda: st_layered.do_step(state, stream=stream)],
                    iters=max(a.iters // 5, 4), warmup=2)
    res["calls"]["rk4_step_plain_stage_fused"], res["calls"]["rk4_step_layered_unfused"] = steps
    res["rk4_layered_over_plain"] = steps[1]["ms_median"] / steps[0]["ms_median"]
    h, _ = state.copy_to_host(0)
    res["state_finite_after_steps"] = bool(np.isfinite(h[: mesh.NCellsAll]).all())
    emit(res, a.out)


if __name__ == "__main__":
    main()
