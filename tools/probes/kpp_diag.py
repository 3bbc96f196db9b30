"""Kpp (Kpp.h) timed with device events at QU30 size: 462 400 cells x 80 levels in k-d order, 6 tracers, surface-attached
layer ranges, a stratified column under rough velocities, us in [0, 0.02] and Bf in [-2e-7, 1e-7] per cell.  Times
Kpp::compute and Kpp::applyNonLocalTracerFlux and, alternating in the same loop, the launch of the code without this
class that does the same edge gather over the same rows: VertMix::computeVertMix (it also rewrites what compute changed
of VertDiff / VertVisc, so every round starts from the same coefficients).  Every case is timed twice for the run's own
spread.  Prints one JSON line and writes it to --out.

Algorithmic bytes (8 B values, every row counted once per launch, a hexagon mesh: 3 edge rows per cell):
  compute      24 B per active cell-level (N2, ZMid, ZInterface) + 16 B per active edge-level (Un, Ut) + 16 B per
               cell-level written (BulkRichardson, NonLocalShape: every entry of every row) + 16 B per interface inside
               the boundary layer (VertDiff, VertVisc)
  non_local    16 B per active cell-level (h, NonLocalShape) + 16 B per tracer and active cell-level (phi read, written)
  vert_mix     16 B per active cell-level (N2, ZMid) + 16 B per active edge-level + 16 B per cell-level written

   python tools/probes/kpp_diag.py [--nx 680] [--levels 80] [--tracers 6] [--iters 50] [--warmup 10]
          [--local-order kd] [--only-kernels] [--out FILE]
(--only-kernels: just the two launches, --iters times: the form to run under rocprofv3 --pmc or --kernel-trace.)
"""
import argparse

import numpy as np
from probe_rig import PEAK_TBS, Qu30Rig, add_common_args, emit, oa, summarise, twice, with_rate


def main(argv=None):
    ap = argparse.ArgumentParser()
    add_common_args(ap, only_kernels=True, nx=680, levels=80, tracers=6, dt=600.0, iters=50, warmup=10, local_order="kd")
    a = ap.parse_args(argv)
    w = Qu30Rig(a, bottom="layers", fields="rough", tracers="stratified")
    K, NT, mesh, ns, nc, state, tracers, vc = w.K, w.NT, w.mesh, w.ns, w.nc, w.state, w.tracers, w.vc
    eos = oa.Eos(mesh, K, "teos10")
    vm = oa.VertMix(mesh, vc)
    kpp = oa.Kpp(mesh, vc, vm)
    us, bf = w.rng.uniform(0.0, 0.02, ns), w.rng.uniform(-2.0e-7, 1.0e-7, ns)
    kpp.set("FrictionVelocity", us)
    kpp.set("SurfaceBuoyancyFlux", bf)
    flux = oa.DeviceBuffer(w.rng.uniform(-1.0e-4, 1.0e-4, (NT, ns)))
    stream = w.stream
    hp, up, trp = state.device_ptr(0, 0), state.device_ptr(1, 0), tracers.device_ptr(0)
    vc.compute_column(state, tracers, eos, kdisp=1, stream=stream)
    vm.compute_bvf(eos, stream=stream)
    stream.synchronize()
    pad = np.zeros((w.nes, w.P))
    pad[:, :K] = oa.HorzOperators(mesh).tangential_recon(w.u0)
    ut = oa.DeviceBuffer(pad)
    del pad
    oa.device_synchronize()

    def vert_mix():
        vm.compute(up, ut.ptr, stream=stream)

    def compute():
        kpp.compute(up, ut.ptr, stream=stream)

    def non_local():
        kpp.apply_non_local(hp, trp, NT, a.dt, surface_flux=flux.ptr, stream=stream)

    res = {"probe": "kpp_diag", "ncells": nc, "nedges": mesh.NEdgesAll, "levels": K, "tracers": NT, "dt": a.dt,
           "local_order": a.local_order, "iters": a.iters, "warmup": a.warmup, "peak_TBs": PEAK_TBS, "calls": {}}
    if a.only_kernels:
        for _ in range(a.iters):
            vert_mix()
            compute()
            non_local()
        stream.synchronize()
        emit(res)
        return

    vert_mix()
    compute()
    stream.synchronize()
    oa.device_synchronize()
    hbl, kb = kpp.get("BoundaryLayerDepth")[:nc], kpp.get("BoundaryLayerIndex")[:nc]
    lo, hi = vc.get("MinLayerCell")[:nc], vc.get("MaxLayerCell")[:nc]
    shape = kpp.get("NonLocalShape")[:nc]
    inside = int(np.sum(np.clip(kb - lo - 1, 0, None)))  # interfaces KMin < K < kb: an upper count of those inside
    res.update(hbl_mean_m=float(hbl.mean()), hbl_max_m=float(hbl.max()), hbl_finite=bool(np.isfinite(hbl).all()),
               index_mean_levels=float((kb - lo).mean()), no_crossing_fraction=float((kb == hi + 1).mean()),
               unstable_fraction=float((bf[:nc] < 0.0).mean()), shape_max=float(shape.max()), interfaces_inside=inside)
    del shape
    cl, ecl, all_cl = w.active_cell_levels, w.active_edge_levels, ns * K
    res.update(active_cell_levels=cl, active_edge_levels=ecl)
    nbytes = {"compute": 24 * cl + 16 * ecl + 16 * all_cl + 16 * inside, "non_local": (16 + 16 * NT) * cl,
              "vert_mix": 16 * cl + 16 * ecl + 16 * all_cl}
    c = res["calls"]
    keys = twice(c, ("vert_mix", "compute", "non_local"),
                 lambda: w.time((vert_mix, compute, non_local), before=w.reset, every=10))
    for name, t in c.items():
        with_rate(t, nbytes[name[:-2]])
    res["kpp_launches_so_far"] = kpp.launch_count()  # two per round of the loop: one per call
    s = res["summary"] = summarise(c, keys)
    s["compute_over_vert_mix"] = s["compute_ms"] / s["vert_mix_ms"]
    s["compute_bytes_over_vert_mix_bytes"] = nbytes["compute"] / nbytes["vert_mix"]
    emit(res, a.out)


if __name__ == "__main__":
    main()
