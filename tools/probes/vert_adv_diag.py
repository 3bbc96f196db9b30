"""VertAdv (VertAdv.h) timed with device events at QU30 size: 462 400 cells x 80 levels x 6 tracers in k-d order,
surface-attached layer ranges as in tools/probes/pressure_grad_diag.py.  Times each launch alone (median of --iters) and
-- alternating in one loop, in the same process -- the plain RHS against the RHS with the VertAdv attached, and one RK4
step of each (plain: stage updates fused; attached: stage updates as separate kernels).  Prints one JSON line and writes
it to --out.

Algorithmic bytes (VertAdv.h), on the active cell-levels / edge-levels of the ranges:
  transport 24 B per cell-level, transport + thickness 32 B, thickness alone 24 B,
  tracers (16 + 24 NT) B per cell-level, velocity 16 B per cell-level + 24 B per edge-level.

   python tools/probes/vert_adv_diag.py [--nx 680] [--levels 80] [--tracers 6] [--iters 50] [--warmup 10]
          [--local-order kd] [--only-kernels] [--out FILE]
(--only-kernels: just the launches, a few times: the form to run under rocprofv3 --pmc or --kernel-trace.)
"""
import argparse

import numpy as np
from probe_rig import PEAK_TBS, Qu30Rig, add_common_args, emit, oa, with_rate


def main(argv=None):
    ap = argparse.ArgumentParser()
    add_common_args(ap, only_kernels=True, nx=680, levels=80, tracers=6, iters=50, warmup=10, local_order="kd")
    a = ap.parse_args(argv)
    w = Qu30Rig(a, fields="rough")
    K, NT, mesh, ns, nes, state, tracers, vc, rng = w.K, w.NT, w.mesh, w.ns, w.nes, w.state, w.tracers, w.vc, w.rng
    vc.set("RefLayerThickness", rng.uniform(1.0, 50.0, (ns, K)))
    va = oa.VertAdv(mesh, vc, 2)
    stream = w.stream
    hp, up, trp = state.device_ptr(0, 0), state.device_ptr(1, 0), tracers.device_ptr(0)
    pitch = oa.level_pitch(K)
    d = oa.DeviceBuffer(np.pad(rng.uniform(-1.0e-6, 1.0e-6, (ns, K)), ((0, 0), (0, pitch - K))))
    tt = oa.DeviceBuffer(np.zeros((NT, ns, pitch)))
    ut = oa.DeviceBuffer(np.zeros((nes, pitch)))

    cactive = w.active_cell_levels
    eactive = w.active_edge_levels
    nbytes = {"transport": 24 * cactive, "transport_and_thickness": 32 * cactive, "thickness": 24 * cactive,
              "tracers": (16 + 24 * NT) * cactive, "velocity": 16 * cactive + 24 * eactive}
    calls = {"transport": lambda: va.compute_transport(d.ptr, stream=stream),
             "transport_and_thickness": lambda: va.compute_transport(d.ptr, add_thickness=True, stream=stream),
             "thickness": lambda: va.add_thickness(d.ptr, stream=stream),
             "tracers": lambda: va.add_tracers(tt.ptr, hp, trp, NT, stream=stream),
             "velocity": lambda: va.add_velocity(ut.ptr, hp, up, stream=stream)}
    res = {"probe": "vert_adv_diag", "ncells": mesh.NCellsAll, "nedges": mesh.NEdgesAll, "levels": K, "tracers": NT,
           "local_order": a.local_order, "active_cell_levels": cactive, "active_edge_levels": eactive, "iters": a.iters,
           "peak_TBs": PEAK_TBS, "calls": {}}

    if a.only_kernels:
        for _ in range(a.iters):
            for fn in calls.values():
                fn()
        stream.synchronize()
        emit(res)
        return

    for name, fn in calls.items():
        res["calls"][name] = with_rate(w.time([fn])[0], nbytes[name])

    # the RHS with and without the terms, same state, same process, alternating
    aux, plain, attached = w.tendencies(oa.default_config(), 2)
    attached.attach_vert_adv(va)
    rhs = w.time([lambda: plain.compute_all_tendencies(state, aux, tracers, stream=stream),
                 lambda: attached.compute_all_tendencies(state, aux, tracers, stream=stream)])
    res["calls"]["rhs_plain"], res["calls"]["rhs_attached"] = rhs
    res["rhs_attached_over_plain"] = rhs[1]["ms_median"] / rhs[0]["ms_median"]
    st_plain = oa.TimeStepper("RungeKutta4", 1.0, plain, aux, mesh, None, tracers)
    st_attached = oa.TimeStepper("RungeKutta4", 1.0, attached, aux, mesh, None, tracers)
    steps = w.time([lambda: st_plain.do_step(state, stream=stream), lambda: st_attached.do_step(state, stream=stream)],
                    iters=max(a.iters // 5, 4), warmup=2)
    res["calls"]["rk4_step_plain_stage_fused"], res["calls"]["rk4_step_attached_unfused"] = steps
    res["rk4_attached_over_plain"] = steps[1]["ms_median"] / steps[0]["ms_median"]
    h, _ = state.copy_to_host(0)
    res["state_finite_after_steps"] = bool(np.isfinite(h[: mesh.NCellsAll]).all())
    emit(res, a.out)


if __name__ == "__main__":
    main()
