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
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import omega_amd as oa  # noqa: E402
from omega_amd.meshgen import planar_hex  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=680)
    ap.add_argument("--levels", type=int, default=80)
    ap.add_argument("--tracers", type=int, default=6)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--local-order", default="kd")
    ap.add_argument("--only-kernels", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    K, NT = a.levels, a.tracers
    oa.device_init(0)
    g = planar_hex(a.nx, a.nx, 30.0e3)
    n = int(g["nCells"])
    rng = np.random.default_rng(2026)
    min_level = np.ones(n, np.int32)
    max_level = np.where(rng.random(n) < 0.6, K, rng.integers(5, K + 1, n)).astype(np.int32)
    gm = oa.GlobalMesh(g)
    decomp = oa.Decomp(gm, 1, 0, 3, local_order=a.local_order)
    mesh = oa.HorzMesh(decomp, K)
    ns, nes = mesh.NCellsSize, mesh.NEdgesSize
    state = oa.OceanState(mesh, None, K, 2)
    tracers = oa.Tracers(mesh, None, K, NT, 2)
    h0, u0 = rng.uniform(1.0, 50.0, (ns, K)), rng.uniform(-0.05, 0.05, (nes, K))
    tr0 = np.concatenate([rng.uniform(2.0, 20.0, (1, ns, K)), rng.uniform(33.0, 36.0, (1, ns, K)),
                          rng.uniform(-1.0, 1.0, (NT - 2, ns, K))])
    state.copy_to_device(h0, u0, 0)
    tracers.copy_to_device(tr0, 0)
    vc = oa.VertCoord(mesh, K, 1026.0, "Uniform", min_level, max_level, decomp=decomp)
    vc.set("RefLayerThickness", rng.uniform(1.0, 50.0, (ns, K)))
    eos = oa.Eos(mesh, K, "teos10")
    vm = oa.VertMix(mesh, vc)
    step = oa.VertMixStep(mesh, vm, vc, eos, NT)
    step.set("NormalStressEdge", rng.uniform(-0.2, 0.2, nes))
    step.set("SurfaceTracerFlux", rng.uniform(-1.0e-6, 1.0e-6, (NT, ns)))
    step.set_boundary(2.5e-3, 1.0e-6, True)
    stream = oa.Stream()
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
        print(json.dumps(res))
        return

    def timed(fns):
        """median / quartiles / min / max ms of each fn, the fns alternating in one loop"""
        for _ in range(a.warmup):
            for fn in fns:
                fn()
        stream.synchronize()
        evs = [[oa.Event() for _ in range(2)] for _ in range(a.iters * len(fns))]
        i = 0
        for _ in range(a.iters):
            for fn in fns:
                evs[i][0].record(stream)
                fn()
                evs[i][1].record(stream)
                i += 1
        stream.synchronize()
        out = []
        for j in range(len(fns)):
            per = np.array([evs[r * len(fns) + j][0].elapsed_ms(evs[r * len(fns) + j][1]) for r in range(a.iters)])
            q1, med, q3 = np.percentile(per, [25, 50, 75])
            out.append({"ms_median": float(med), "ms_q1": float(q1), "ms_q3": float(q3), "ms_min": float(per.min()),
                        "ms_max": float(per.max())})
        return out

    for kind in ("tracers", "velocity"):
        un, fo, un2 = timed([calls[kind + "_unforced"], calls[kind + "_forced"], calls[kind + "_unforced"]])
        res["calls"][kind + "_unforced"], res["calls"][kind + "_forced"], res["calls"][kind + "_unforced_again"] = un, fo, un2
        res[kind + "_forced_over_unforced"] = fo["ms_median"] / un["ms_median"]
        res[kind + "_unforced_again_over_unforced"] = un2["ms_median"] / un["ms_median"]
        res[kind + "_unforced_iqr_over_median"] = (un["ms_q3"] - un["ms_q1"]) / un["ms_median"]

    state.copy_to_device(h0, u0, 0)
    tracers.copy_to_device(tr0, 0)
    res["calls"]["vert_mix_step_apply"] = timed([lambda: step.apply(hp, up, trp, dt, stream=stream)])[0]

    # one RK4 step with and without the hook; the layered terms attached in both, so both run the plain stage sequence
    cfg = oa.default_config(SSHTendencyEnable=0)
    aux = oa.AuxiliaryState(mesh, None, K, NT)
    aux.set_options(cfg.FluxThicknessUpwind, cfg.FluxTracerUpwind, cfg.WindInterpIsotropic)
    tend = oa.Tendencies(mesh, K, NT, cfg)
    pg, va = oa.PressureGrad(mesh, vc, eos), oa.VertAdv(mesh, vc, 2)
    tend.attach_vert_adv(va)
    tend.attach_pressure_grad(pg)
    state.copy_to_device(h0, u0, 0)
    tracers.copy_to_device(tr0, 0)
    plain = oa.TimeStepper("RungeKutta4", 1.0, tend, aux, mesh, None, tracers)
    hooked = oa.TimeStepper("RungeKutta4", 1.0, tend, aux, mesh, None, tracers)
    hooked.attach_vert_mix(step)
    a.iters, a.warmup = max(a.iters // 5, 4), 2
    steps = timed([lambda: plain.do_step(state, stream=stream), lambda: hooked.do_step(state, stream=stream)])
    res["calls"]["rk4_step_plain"], res["calls"]["rk4_step_with_hook"] = steps
    res["rk4_hook_over_plain"] = steps[1]["ms_median"] / steps[0]["ms_median"]
    h, _ = state.copy_to_host(0)
    res["state_finite_after_steps"] = bool(np.isfinite(h[: mesh.NCellsAll]).all())
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
