"""BarotropicMode (BarotropicMode.h) timed with device events at QU30 size: 462 400 cells x 80 levels in k-d order,
surface-attached layer ranges as in tools/probes/vert_adv_diag.py.  Times, each as the median of --iters, the split
launch (alone and with the SSH in the same launch), computeForcing, recombine and subcycle(--nsub), and -- in the same
process -- one fused RHS evaluation to set them against.  Prints one JSON line and writes it to --out.

Bytes models (BarotropicMode.h; `active` = the levels of the ranges):
  split            algorithmic 16 B per active edge-level (u read, BclVelocity written) + 8 B per active cell-level (h,
                   each row ideally once); as issued 32 B per active edge-level (h of both cells per edge)
  split + SSH      + 8 B per active cell-level (h once more, by the cell half of the launch)
  forcing          8 B per active edge-level + 8 B per active cell-level (issued: 24 B per active edge-level)
  recombine        16 B per active edge-level
  one sub-step     tables and fields each once: per cell 16 B x MaxEdges + 36 B, per edge 12 B x MaxEdges2 + 68 B
                   (the gathered SSH / BottomDepth / BtrVelocity values are shared between neighbouring threads)

   python tools/probes/barotropic_diag.py [--nx 680] [--levels 80] [--nsub 30] [--iters 50] [--warmup 10]
          [--local-order kd] [--only-kernels] [--out FILE]
(--only-kernels: just the launches, a few times: the form to run under rocprofv3 --pmc or --kernel-trace.)
"""
import argparse

import numpy as np
from probe_rig import PEAK_TBS, Qu30Rig, add_common_args, emit, oa, with_rate


def main(argv=None):
    ap = argparse.ArgumentParser()
    add_common_args(ap, only_kernels=True, nx=680, levels=80, tracers=6, nsub=30, iters=50, warmup=10, local_order="kd")
    ap.add_argument("--dt-btr", type=float, default=20.0)
    a = ap.parse_args(argv)
    w = Qu30Rig(a, bottom=4000.0, fields="rough")
    K, mesh, ns, nes, state, tracers, vc, rng = w.K, w.mesh, w.ns, w.nes, w.state, w.tracers, w.vc, w.rng
    bm = oa.BarotropicMode(mesh, vc)
    stream = w.stream
    hp, up = state.device_ptr(0, 0), state.device_ptr(1, 0)
    pitch = oa.level_pitch(K)
    ut = oa.DeviceBuffer(np.pad(rng.uniform(-1.0e-6, 1.0e-6, (nes, K)), ((0, 0), (0, pitch - K))))
    ur = oa.DeviceBuffer(np.zeros((nes, pitch)))

    cactive = w.active_cell_levels
    eactive = w.active_edge_levels
    nc, ne, me, me2 = mesh.NCellsAll, mesh.NEdgesAll, mesh.MaxEdges, mesh.MaxEdges2
    substep = nc * (16 * me + 36) + ne * (12 * me2 + 68)
    nbytes = {"split": 16 * eactive + 8 * cactive, "split_and_ssh": 16 * eactive + 16 * cactive,
              "forcing": 8 * eactive + 8 * cactive, "recombine": 16 * eactive,
              "subcycle": a.nsub * substep + 24 * ne}
    issued = {"split": 32 * eactive, "split_and_ssh": 32 * eactive + 8 * cactive, "forcing": 24 * eactive}

    def reset():
        """a calm 2-D state to sub-cycle from: it is stepped a.nsub * iterations times in all"""
        bm.set("SSH", np.zeros(ns)), bm.set("BtrVelocity", np.zeros(nes)), bm.set("BtrForcing", np.full(nes, 1.0e-9))

    calls = {"split": lambda: bm.split_velocity(hp, up, stream=stream),
             "split_and_ssh": lambda: bm.split_velocity(hp, up, with_ssh=True, stream=stream),
             "forcing": lambda: bm.compute_forcing(hp, ut.ptr, stream=stream),
             "recombine": lambda: bm.recombine(ur.ptr, stream=stream),
             "subcycle": lambda: bm.subcycle(a.nsub, a.dt_btr, stream=stream)}
    res = {"probe": "barotropic_diag", "ncells": nc, "nedges": ne, "levels": K, "nsub": a.nsub,
           "local_order": a.local_order, "active_cell_levels": cactive, "active_edge_levels": eactive, "iters": a.iters,
           "max_edges": me, "max_edges2": me2, "peak_TBs": PEAK_TBS, "calls": {}}
    reset()

    if a.only_kernels:
        for _ in range(a.iters):
            for fn in calls.values():
                fn()
        stream.synchronize()
        emit(res)
        return

    aux, tend = w.tendencies(oa.default_config())
    rhs = w.time([lambda: tend.compute_all_tendencies(state, aux, tracers, stream=stream)])[0]
    res["calls"]["rhs_fused"] = rhs
    for name, fn in calls.items():
        if name == "subcycle":
            reset()
        t = with_rate(w.time([fn])[0], nbytes[name])
        if name in issued:
            t["issued_GB"] = issued[name] / 1.0e9
            t["issued_TBs"] = t["issued_GB"] / t["ms_median"]
        t["fraction_of_rhs"] = t["ms_median"] / rhs["ms_median"]
        res["calls"][name] = t
    res["calls"]["subcycle"]["us_per_substep"] = 1.0e3 * res["calls"]["subcycle"]["ms_median"] / a.nsub
    res["state_finite_after_subcycles"] = bool(np.isfinite(bm.get("SSH")[:nc]).all() and
                                                np.isfinite(bm.get("BtrVelocity")[:ne]).all())
    emit(res, a.out)


if __name__ == "__main__":
    main()
