"""Redi (Redi.h) timed with device events at QU30 size: 462 400 cells x 80 levels in k-d order, 2 tracers,
surface-attached layer ranges as in tools/probes/gm_diag.py.  Times the three launches -- the slope, the tracer tendency,
the S.S diffusivity (with a VertDiff to add to) -- and, alternating in the same loop, a yardstick from the code without
this class next to each: GentMcWilliams::computeBolusVelocity without Transport (the same edge-column geometry on the
same cell arrays plus the thickness, two arrays written and a PCR solve) for the slope, the centred
MonotoneAdv::addTracerTend at the same tracer count (two launches) for the tendency, and the displaced column pass.
Then whole Split-Explicit steps with a VertMixStep attached, with and without the closure, alternating.  Prints one JSON
line and writes it to --out.

Algorithmic bytes (8 B values, every row counted once per launch, a hexagon mesh: 3 edge rows per cell):
  slope        24 B per cell-level (SpecVol, SpecVolDisplaced, ZMid) + 8 B per active edge-level (SlopeInterface written)
  tendency     16 B per cell-level (h, ZMid) + 8 B per edge-level (SlopeInterface) + 24 B per tracer and cell-level (phi
               read, Tend read and written)
  diffusivity  8 B per edge-level + 24 B per cell-level (VertDiffusivity written, VertDiff read and written)
  bolus        32 B per cell-level + 16 B per active edge-level (no Transport)

   python tools/probes/redi_diag.py [--nx 680] [--levels 80] [--tracers 2] [--nsub 30] [--dt 600] [--iters 50]
          [--warmup 10] [--local-order kd] [--only-kernels] [--no-steps] [--out FILE]
(--only-kernels: just the three launches, --iters times: the form to run under rocprofv3 --pmc or --kernel-trace.)
"""
import argparse

import numpy as np
from probe_rig import PEAK_TBS, Qu30Rig, add_common_args, emit, oa, summarise, twice, with_rate


def main(argv=None):
    ap = argparse.ArgumentParser()
    add_common_args(ap, only_kernels=True, nx=680, levels=80, tracers=2, nsub=30, dt=600.0, iters=50, warmup=10, local_order="kd")
    ap.add_argument("--no-steps", action="store_true")
    a = ap.parse_args(argv)
    # a stable column (T falls, S rises with depth) with noise across the cells: fronts for the closure to act on
    w = Qu30Rig(a, bottom="layers", tracers="stratified")
    K, NT, P, mesh, ns, nc, state, tracers, vc = w.K, w.NT, w.P, w.mesh, w.ns, w.nc, w.state, w.tracers, w.vc
    eos = oa.Eos(mesh, K, "teos10")
    redi = oa.Redi(mesh, vc, eos, NT)
    gm = oa.GentMcWilliams(mesh, vc, eos)
    mono = oa.MonotoneAdv(mesh, K, NT)
    stream = w.stream
    hp, h1, u1, trp = state.device_ptr(0, 0), state.device_ptr(0, 1), state.device_ptr(1, 1), tracers.device_ptr(0)
    redi.update_column(hp, trp, NT, stream=stream)
    stream.synchronize()
    tend_buf = oa.DeviceBuffer(np.zeros((NT, ns, P)))
    vert_diff = oa.DeviceBuffer(np.zeros((ns, P)))

    eactive = w.active_edge_levels
    cl = nc * K
    nbytes = {"slope": 24 * cl + 8 * eactive, "tracer_tend": (16 + 24 * NT) * cl + 8 * eactive,
              "vert_diffusivity": 24 * cl + 8 * eactive, "bolus_velocity_no_transport": 32 * cl + 16 * eactive,
              "mono_centred": (72 + 64 * NT) * cl}
    res = {"probe": "redi_diag", "ncells": nc, "nedges": mesh.NEdgesAll, "levels": K, "tracers": NT, "nsub": a.nsub,
           "dt": a.dt, "local_order": a.local_order, "active_edge_levels": eactive, "iters": a.iters, "warmup": a.warmup,
           "peak_TBs": PEAK_TBS, "calls": {}}

    def slope():
        redi.compute_slope(hp, stream=stream)

    def bolus():
        gm.compute(hp, None, stream=stream)

    def tracer_tend():
        redi.add_tracer_tend(tend_buf.ptr, hp, trp, NT, stream=stream)

    def mono_centred():
        mono.add_tracers(tend_buf.ptr, hp, h1, u1, trp, NT, a.dt, stream=stream)

    def vert_diffusivity():
        redi.compute_vert_diffusivity(vert_diff.ptr, stream=stream)

    def column():
        redi.update_column(hp, trp, NT, stream=stream)

    if a.only_kernels:
        for _ in range(a.iters):
            slope()
            tracer_tend()
            vert_diffusivity()
        stream.synchronize()
        emit(res)
        return

    names = ("slope", "bolus_velocity_no_transport", "tracer_tend", "mono_centred", "vert_diffusivity")
    fns = (slope, bolus, tracer_tend, mono_centred, vert_diffusivity, column)
    c = res["calls"]
    keys = twice(c, names + ("column_pass_displaced",), lambda: w.time(fns))
    for name, t in c.items():
        if name[:-2] in nbytes:
            with_rate(t, nbytes[name[:-2]])
    stream.synchronize()
    s_dev = redi.get("SlopeInterface")[: mesh.NEdgesAll]
    res["slope_finite"], res["slope_max_abs"] = bool(np.isfinite(s_dev).all()), float(np.abs(s_dev).max())
    res["slope_clipped_fraction"] = float((np.abs(s_dev) == 0.01).sum() / max(eactive, 1))
    del s_dev
    res["redi_launches_so_far"] = redi.launch_count()  # three per round of the loop: one per call

    if not a.no_steps:
        aux, tend = w.tendencies(oa.default_config())
        bm = oa.BarotropicMode(mesh, vc)
        vm = oa.VertMix(mesh, vc)
        mix_plain, mix_redi = oa.VertMixStep(mesh, vm, vc, eos, NT), oa.VertMixStep(mesh, vm, vc, eos, NT)
        mix_redi.attach_redi(redi)
        steppers = []
        for mix, closure in ((mix_plain, False), (mix_redi, True)):
            st = oa.TimeStepper("Split-Explicit", a.dt, tend, aux, mesh, None, tracers)
            st.attach_barotropic(bm, a.nsub)
            st.attach_vert_mix(mix)
            if closure:
                st.attach_redi(redi)
            steppers.append(st)
        step_fns = [lambda st=st: st.do_step(state, stream=stream) for st in steppers]
        keys += twice(c, ("step_vert_mix", "step_vert_mix_redi"), lambda: w.time(step_fns, before=w.reset, every=5))
        stream.synchronize()
        oa.device_synchronize()
        res["step_state_finite"] = bool(np.isfinite(tracers.copy_to_host(0)[:, :nc]).all())
    s = res["summary"] = summarise(c, keys)
    s["slope_over_bolus_velocity"] = s["slope_ms"] / s["bolus_velocity_no_transport_ms"]
    s["tracer_tend_over_mono_centred"] = s["tracer_tend_ms"] / s["mono_centred_ms"]
    if not a.no_steps:
        s["step_redi_over_step_plain"] = s["step_vert_mix_redi_ms"] / s["step_vert_mix_ms"]
        s["step_redi_minus_step_plain_ms"] = s["step_vert_mix_redi_ms"] - s["step_vert_mix_ms"]
    emit(res, a.out)


if __name__ == "__main__":
    main()
