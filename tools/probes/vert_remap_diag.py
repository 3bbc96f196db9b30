"""VertRemap (VertRemap.h) timed with device events at QU30 size: 462 400 cells x 80 levels in k-d order, 6 tracers,
surface-attached layer ranges as in tools/probes/redi_diag.py.  For each order (PCM, PLM, PPM) it times remap -- three
launches -- from a thickness that is the reference thickness perturbed layer-wise by up to +-30 % (restored on the device
before every call, outside the timed span: the first remap leaves h on the target, and a second one from there would
find every layer whole), the orders alternating in one loop.  Then whole Split-Explicit steps without and with the remap
attached (PPM), alternating: the step without it is the step of the code before this class, launch for launch.  Prints
one JSON line and writes it to --out.

Algorithmic bytes of remap (8 B values, every row counted once per launch, a hexagon mesh: 3 edge rows per cell):
  target + tracers  24 B per cell-level (h, Ref read, target written) + 16 B per tracer and cell-level (in place)
  velocity          16 B per cell-level (h, target, each row once) + 16 B per active edge-level (u in place)
  adoption          16 B per cell-level (target read, h written)

   python tools/probes/vert_remap_diag.py [--nx 680] [--levels 80] [--tracers 6] [--nsub 30] [--dt 600] [--iters 20]
          [--warmup 5] [--local-order kd] [--only-kernels] [--no-steps] [--plain-step-only] [--out FILE]
(--only-kernels: just remap at each order, --iters times: the form to run under rocprofv3 --pmc or --kernel-trace.
--plain-step-only: nothing but the step without the remap, and no call into the class: the form that also runs on a
library built from the code before it, OMEGA_AMD_LIB=<that library>, to compare the two builds in alternating processes.)
"""
import argparse
import os

import numpy as np
from probe_rig import LAYER, PEAK_TBS, Qu30Rig, add_common_args, emit, oa, summarise, twice, with_rate

ORDER_NAMES = {1: "pcm", 2: "plm", 3: "ppm"}


def main(argv=None):
    ap = argparse.ArgumentParser()
    add_common_args(ap, only_kernels=True, nx=680, levels=80, tracers=6, nsub=30, dt=600.0, iters=20, warmup=5, local_order="kd")
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--plain-step-only", action="store_true")
    a = ap.parse_args(argv)
    w = Qu30Rig(a, bottom="layers", tracers="stratified", ref_thickness=True)
    K, NT, P, mesh, ns, nc, state, tracers, vc = w.K, w.NT, w.P, w.mesh, w.ns, w.nc, w.state, w.tracers, w.vc
    remaps = {} if a.plain_step_only else {o: oa.VertRemap(mesh, vc, NT, o) for o in (1, 2, 3)}
    stream = w.stream
    # the scratch level 1 of the state and the tracers is what the calls work on; the perturbed thickness is kept aside
    h1, u1, tr1 = state.device_ptr(0, 1), state.device_ptr(1, 1), tracers.device_ptr(1)
    pad = np.zeros((ns, P))
    pad[:, :K] = LAYER * w.rng.uniform(0.7, 1.3, (ns, K))
    h_rough = oa.DeviceBuffer(pad)
    del pad

    def roughen():  # h1 = h_rough, on the device (out = in + 0 * tend)
        oa.update_by_tend(h1, h_rough.ptr, h_rough.ptr, 0.0, ns, P, stream.h.value)

    eactive = w.active_edge_levels
    cl = nc * K
    nbytes = (24 + 16 * NT) * cl + (16 * cl + 16 * eactive) + 16 * cl
    res = {"probe": "vert_remap_diag", "ncells": nc, "nedges": mesh.NEdgesAll, "levels": K, "tracers": NT, "nsub": a.nsub,
           "dt": a.dt, "local_order": a.local_order, "active_edge_levels": eactive, "iters": a.iters, "warmup": a.warmup,
           "peak_TBs": PEAK_TBS, "remap_algorithmic_GB": nbytes / 1.0e9, "calls": {}}

    def remap(order):
        remaps[order].remap(h1, u1, tr1, NT, stream=stream)

    if a.only_kernels:
        for _ in range(a.iters):
            for o in (1, 2, 3):
                roughen()
                remap(o)
        stream.synchronize()
        oa.device_synchronize()
        emit(res)
        return

    c = res["calls"]
    keys = []
    if not a.plain_step_only:
        fns = [lambda o=o: remap(o) for o in (1, 2, 3)]
        keys = twice(c, [f"remap_{v}" for v in ORDER_NAMES.values()], lambda: w.time(fns, before_each=roughen))
        for t in c.values():
            with_rate(t, nbytes)
        res["launches_per_remap"] = remaps[3].launch_count() / (2 * (a.iters + a.warmup))
        oa.device_synchronize()
        res["remap_state_finite"] = bool(np.isfinite(tracers.copy_to_host(1)[:, :nc]).all())

    if not a.no_steps:
        aux, tend = w.tendencies(oa.default_config())
        bm = oa.BarotropicMode(mesh, vc)
        steppers = []
        for attached in ((False,) if a.plain_step_only else (False, True)):
            st = oa.TimeStepper("Split-Explicit", a.dt, tend, aux, mesh, None, tracers)
            st.attach_barotropic(bm, a.nsub)
            if attached:
                st.attach_vert_remap(remaps[3])
            steppers.append(st)
        step_fns = [lambda st=st: st.do_step(state, stream=stream) for st in steppers]
        keys += twice(c, ("step", "step_vert_remap")[: len(step_fns)], lambda: w.time(step_fns, before=w.reset, every=5))
        oa.device_synchronize()
        res["step_state_finite"] = bool(np.isfinite(tracers.copy_to_host(0)[:, :nc]).all())
    s = res["summary"] = summarise(c, keys)
    for v in ORDER_NAMES.values():
        if f"remap_{v}_ms" in s:
            s[f"remap_{v}_share_of_8TBs"] = res["remap_algorithmic_GB"] / s[f"remap_{v}_ms"] / PEAK_TBS
    res["library"] = os.path.basename(oa.LIB_PATH)
    if not a.no_steps and not a.plain_step_only:
        s["step_vert_remap_minus_step_ms"] = s["step_vert_remap_ms"] - s["step_ms"]
        s["step_vert_remap_over_step"] = s["step_vert_remap_ms"] / s["step_ms"]
    emit(res, a.out)


if __name__ == "__main__":
    main()
