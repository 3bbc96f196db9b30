"""The forced implicit solves of VertMix (VertMix.h) timed with device events at QU30 size: 462 400 cells x 80 levels x
6 tracers in k-d order, surface-attached layer ranges as in tools/probes/vert_adv_diag.py.  In one process and one
alternating loop it times the unforced launch, the forced launch and the unforced launch again (median of --iters
each), for the tracer solve and for the velocity solve: the second unforced series gives the run-to-run spread the
forced launch is judged against.  Then one VertMixStep.apply, and one RK4 step with and without the stepper hook
(PressureGrad and VertAdv attached in both, so both run the plain stage sequence).  Prints one JSON line and writes it
to --out.

The forced launch adds, per column, two 8-byte reads and a sqrt on one lane and nothing per level: the expectation is
parity with the unforced launch within that spread.

   python tools/probes/vert_mix_forcing_diag.py [--nx 680] [--levels 80] [--tracers 6] [--iters 50] [--warmup 10]
          [--local-order kd] [--only-kernels] [--out FILE]
(--only-kernels: just the four solves, a few times: the form to run under rocprofv3 --kernel-trace.)
"""
import argparse

import numpy as np
from probe_rig import Qu30Rig, add_common_args, emit, oa


def main(argv=None):
    ap = argparse.ArgumentParser()
    add_common_args(ap, only_kernels=True, nx=680, levels=80, tracers=6, iters=50, warmup=10, local_order="kd")
    a = ap.parse_args(argv)
    w = Qu30Rig(a, fields="rough", tracers=((2.0, 20.0), (33.0, 36.0)))
    K, NT, mesh, ns, nes, state, tracers, vc, rng = w.K, w.NT, w.mesh, w.ns, w.nes, w.state, w.tracers, w.vc, w.rng
    vc.set("RefLayerThickness", rng.uniform(1.0, 50.0, (ns, K)))
    eos = oa.Eos(mesh, K, "teos10")
    vm = oa.VertMix(mesh, vc)
    step = oa.VertMixStep(mesh, vm, vc, eos, NT)
    step.set("NormalStressEdge", rng.uniform(-0.2, 0.2, nes))
    step.set("SurfaceTracerFlux", rng.uniform(-1.0e-6, 1.0e-6, (NT, ns)))
    step.set_boundary(2.5e-3, 1.0e-6, True)
    stream = w.stream
    hp, up, trp = state.device_ptr(0, 0), state.device_ptr(1, 0), tracers.device_ptr(0)
    dt = 600.0
    step.apply(hp, up, trp, dt, stream=stream)  # coefficients and the tangential velocity in place
    stream.synchronize()
    flux, stress, ut = (step.device_ptr(k) for k in ("SurfaceTracerFlux", "NormalStressEdge", "TangentialVelocity"))
    calls = {"tracers_unforced": lambda: vm.apply_tracers(hp, trp, NT, dt, stream=stream),
             "tracers_forced": lambda: vm.apply_tracers(hp, trp, NT, dt, stream=stream, surface_flux=flux),
             "velocity_unforced": lambda: vm.apply_velocity(hp, up, dt, stream=stream),
             "velocity_forced": lambda: vm.apply_velocity(hp, up, dt, stream=stream, boundary=(2.5e-3, 1.0e-6),
                                                          stress=stress, ut=ut)}
    res = {"probe": "vert_mix_forcing_diag", "ncells": mesh.NCellsAll, "nedges": mesh.NEdgesAll, "levels": K,
           "tracers": NT, "local_order": a.local_order, "iters": a.iters, "calls": {}}

    if a.only_kernels:
        for _ in range(a.iters):
            for fn in calls.values():
                fn()
        stream.synchronize()
        emit(res)
        return

    def quartiles_too(fns, **kw):
        return [dict(t, ms_q1=t["ms_p25"], ms_q3=t["ms_p75"]) for t in w.time(fns, **kw)]  # (this probe's names for the quartiles)

    for kind in ("tracers", "velocity"):
        un, fo, un2 = quartiles_too([calls[kind + "_unforced"], calls[kind + "_forced"], calls[kind + "_unforced"]])
        res["calls"][kind + "_unforced"], res["calls"][kind + "_forced"], res["calls"][kind + "_unforced_again"] = un, fo, un2
        res[kind + "_forced_over_unforced"] = fo["ms_median"] / un["ms_median"]
        res[kind + "_unforced_again_over_unforced"] = un2["ms_median"] / un["ms_median"]
        res[kind + "_unforced_iqr_over_median"] = (un["ms_q3"] - un["ms_q1"]) / un["ms_median"]

    w.reset()
    res["calls"]["vert_mix_step_apply"] = quartiles_too([lambda: step.apply(hp, up, trp, dt, stream=stream)])[0]

    # one RK4 step with and without the hook; the layered terms attached in both, so both run the plain stage sequence
    aux, tend = w.tendencies(oa.default_config(SSHTendencyEnable=0))
    pg, va = oa.PressureGrad(mesh, vc, eos), oa.VertAdv(mesh, vc, 2)
    tend.attach_vert_adv(va)
    tend.attach_pressure_grad(pg)
    w.reset()
    plain = oa.TimeStepper("RungeKutta4", 1.0, tend, aux, mesh, None, tracers)
    hooked = oa.TimeStepper("RungeKutta4", 1.0, tend, aux, mesh, None, tracers)
    hooked.attach_vert_mix(step)
    steps = quartiles_too([lambda: plain.do_step(state, stream=stream), lambda: hooked.do_step(state, stream=stream)],
                  iters=max(a.iters // 5, 4), warmup=2)
    res["calls"]["rk4_step_plain"], res["calls"]["rk4_step_with_hook"] = steps
    res["rk4_hook_over_plain"] = steps[1]["ms_median"] / steps[0]["ms_median"]
    h, _ = state.copy_to_host(0)
    res["state_finite_after_steps"] = bool(np.isfinite(h[: mesh.NCellsAll]).all())
    emit(res, a.out)


if __name__ == "__main__":
    main()
