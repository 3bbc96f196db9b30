"""VertMix (VertMix.h) timed with device events at QU30 size: 462 400 cells x 80 levels, 6 tracers, surface-attached
layer ranges as in tools/probes/column_diag.py.  Times N^2, the coefficients, the tracer pass and the velocity pass,
and compares the tracer pass with NT separate PCR diffusion launches (PCRDiffusionSolver on pre-assembled G, H, X of
the same [NCells][80] shape), the two alternating in one loop.  The tracer pass is timed on the surface-attached ranges
and on full columns (every level active: the same rows as the separate launches).  Prints one JSON line and writes
it to --out when given.

Algorithmic bytes (each array touched once):
  N^2          32 B per cell-level (SpecVol, SpecVolDisplaced, ZMid read; N^2 written)
  coefficients 32 B per cell-level (N^2, ZMid read; VertVisc, VertDiff written) + 16 B per edge-level (Un, Ut read)
  tracer pass  16 B + 16 B per tracer per active cell-level (h, VertDiff read; phi read and written): 112 B at NT = 6
  velocity     16 B per active edge-level (u read and written) + 16 B per cell-level (h, VertVisc read)
  separate     32 B per row per launch (G, H, X read; X written)

   python tools/probes/vert_mix_diag.py [--nx 680] [--levels 80] [--tracers 6] [--iters 50] [--warmup 10] [--out FILE]
"""
import argparse

import numpy as np
from probe_rig import PEAK_TBS, Qu30Rig, active_levels, add_common_args, emit, oa, with_rate


def main(argv=None):
    ap = argparse.ArgumentParser()
    add_common_args(ap, nx=680, levels=80, tracers=6, iters=50, warmup=10)
    a = ap.parse_args(argv)
    w = Qu30Rig(a, fields="rough", tracers=((-2.0, 30.0), (30.0, 38.0)))
    K, NT, P, mesh, nes, state, tracers, vc, rng = w.K, w.NT, w.P, w.mesh, w.nes, w.state, w.tracers, w.vc, w.rng
    nown, eown, h = mesh.NCellsOwned, mesh.NEdgesOwned, w.h0
    vc_full = oa.VertCoord(mesh, K, 1026.0, "Uniform")
    eos = oa.Eos(mesh, K, "teos10")
    vc.compute_column(state, tracers, eos, kdisp=1)
    vm = oa.VertMix(mesh, vc)
    vm_full = oa.VertMix(mesh, vc_full)
    ut = oa.DeviceBuffer(np.pad(rng.uniform(-0.05, 0.05, (nes, K)), ((0, 0), (0, P - K))))
    stream = w.stream
    hp, up, trp = state.device_ptr(0, 0), state.device_ptr(1, 0), tracers.device_ptr(0)
    vm.compute_bvf(eos, stream=stream)
    vm.compute(up, ut.ptr, stream=stream)
    vm_full.compute_bvf(eos, stream=stream)
    vm_full.compute(up, ut.ptr, stream=stream)
    stream.synchronize()
    # the separate launches' pre-assembled columns: full [NCellsOwned][K] systems, NT right-hand sides
    kd = vm_full.get("VertDiff")[:nown]
    hh = h[:nown]
    gg = np.zeros((nown, K))
    gg[:, :-1] = (kd[:, 1:] * 1800.0) / ((hh[:, 1:] + hh[:, :-1]) / 2)
    sep = {"g": oa.DeviceBuffer(gg), "h": oa.DeviceBuffer(np.ascontiguousarray(hh))}
    xs = [oa.DeviceBuffer(hh * rng.uniform(-1.0, 1.0, (nown, K))) for _ in range(NT)]
    del gg, kd

    def separate():
        for x in xs:
            oa.tridiag_diff_solve(sep["g"].ptr, sep["h"].ptr, x.ptr, "pcr", stream=stream, nbatch=nown, nrow=K)

    calls = {
        "bvf": lambda: vm.compute_bvf(eos, stream=stream),
        "coefficients": lambda: vm.compute(up, ut.ptr, stream=stream),
        "tracer_pass": lambda: vm.apply_tracers(hp, trp, NT, 1800.0, stream=stream),
        "tracer_pass_full_columns": lambda: vm_full.apply_tracers(hp, trp, NT, 1800.0, stream=stream),
        "velocity_pass": lambda: vm.apply_velocity(hp, up, 1800.0, stream=stream),
        "separate_pcr_x%d" % NT: separate,
    }

    # (the owned elements: the rows of the separate launches)
    active = active_levels(vc.get("MinLayerCell")[:nown], vc.get("MaxLayerCell")[:nown])
    eactive = active_levels(vc.get("MinLayerEdgeBot")[:eown], vc.get("MaxLayerEdgeTop")[:eown])
    cl, el = mesh.NCellsAll * K, mesh.NEdgesAll * K
    gb = {"bvf": 32 * cl, "coefficients": 32 * cl + 16 * el, "tracer_pass": (16 + 16 * NT) * active,
          "tracer_pass_full_columns": (16 + 16 * NT) * nown * K, "velocity_pass": 16 * eactive + 16 * cl,
          "separate_pcr_x%d" % NT: 32 * nown * K * NT}
    res = {"probe": "vert_mix_diag", "ncells": mesh.NCellsAll, "nedges": mesh.NEdgesAll, "levels": K, "tracers": NT,
           "active_cell_levels": active, "active_edge_levels": eactive, "iters": a.iters, "peak_TBs": PEAK_TBS,
           "calls": {}}
    names = list(calls)
    groups = [["bvf"], ["coefficients"], ["velocity_pass"],
              ["tracer_pass", "tracer_pass_full_columns", "separate_pcr_x%d" % NT]]
    for grp in groups:
        for name, t in zip(grp, w.time([calls[x] for x in grp])):
            res["calls"][name] = with_rate(t, gb[name])
    assert set(res["calls"]) == set(names)
    sepn = "separate_pcr_x%d" % NT
    res["full_columns_over_separate"] = res["calls"]["tracer_pass_full_columns"]["ms_median"] / \
        res["calls"][sepn]["ms_median"]
    res["tracer_pass_over_separate"] = res["calls"]["tracer_pass"]["ms_median"] / res["calls"][sepn]["ms_median"]
    emit(res, a.out)


if __name__ == "__main__":
    main()
