"""GentMcWilliams (GentMcWilliams.h) timed with device events at QU30 size: 462 400 cells x 80 levels in k-d order,
surface-attached layer ranges as in tools/probes/vert_mix_diag.py.  Times the bolus-velocity launch (with Transport),
the column pass with the displaced volume, the two together (step 5b of the split-explicit step) and, alternating in the
same loop, the yardsticks: VertMix::applyVelocityVertMix (the same edge-column PCR geometry on fewer bytes) and one
fused momentum RHS (Tendencies::computeMomentumTendencies, step 1 of the split-explicit step).  Prints one JSON line
and writes it to --out.

Algorithmic bytes of the launch: 32 B per cell-level (thickness, SpecVol, SpecVolDisplaced, ZMid, each row fetched once)
+ 32 B per active edge-level (BolusVelocity and StreamFunction written, Transport read and written); on a hexagon mesh
~ 128 B per cell-level.  applyVelocityVertMix: 16 B per cell-level + 16 B per active edge-level.

   python tools/probes/gm_diag.py [--nx 680] [--levels 80] [--tracers 2] [--iters 50] [--warmup 10]
          [--local-order kd] [--only-kernel] [--out FILE]
(--only-kernel: just the launch, a few times: the form to run under rocprofv3 --pmc or --kernel-trace.)
"""
import argparse

import numpy as np
from probe_rig import PEAK_TBS, Qu30Rig, add_common_args, emit, oa, with_rate


def main(argv=None):
    ap = argparse.ArgumentParser()
    add_common_args(ap, only_kernels=True, nx=680, levels=80, tracers=2, iters=50, warmup=10, local_order="kd")
    a = ap.parse_args(argv)
    # a stable column (T falls, S rises with depth) with noise across the cells: fronts for the closure to act on
    w = Qu30Rig(a, fields="rough", tracers="stratified")
    K, NT, mesh, nes, state, tracers, vc = w.K, w.NT, w.mesh, w.nes, w.state, w.tracers, w.vc
    eos = oa.Eos(mesh, K, "teos10")
    gm = oa.GentMcWilliams(mesh, vc, eos)
    stream = w.stream
    hp, up, trp = state.device_ptr(0, 0), state.device_ptr(1, 0), tracers.device_ptr(0)
    gm.update_column(hp, trp, NT, stream=stream)
    stream.synchronize()
    transport = oa.DeviceBuffer(np.zeros((nes, oa.level_pitch(K))))

    eactive = w.active_edge_levels
    cell_levels = w.nc * K
    gm_bytes = 32 * cell_levels + 32 * eactive
    mix_bytes = 16 * cell_levels + 16 * eactive
    res = {"probe": "gm_diag", "ncells": mesh.NCellsAll, "nedges": mesh.NEdgesAll, "levels": K, "tracers": NT,
           "local_order": a.local_order, "active_edge_levels": eactive, "iters": a.iters, "peak_TBs": PEAK_TBS,
           "gm_algorithmic_GB": gm_bytes / 1.0e9, "gm_B_per_cell_level": gm_bytes / cell_levels, "calls": {}}

    def bolus():
        gm.compute(hp, transport.ptr, stream=stream)

    def column():
        gm.update_column(hp, trp, NT, stream=stream)

    def step5b():
        column()
        bolus()

    if a.only_kernels:
        for _ in range(a.iters):
            bolus()
        stream.synchronize()
        emit(res)
        return

    # the yardstick: the implicit velocity mixing on the same columns (coefficients from the same stratification)
    vm = oa.VertMix(mesh, vc)
    vm.compute_bvf(eos, stream=stream)
    vm.compute(up, up, stream=stream)
    mixed = oa.DeviceBuffer(np.zeros((nes, oa.level_pitch(K))))

    def velocity_mix():
        vm.apply_velocity(hp, mixed.ptr, 600.0, stream=stream)

    aux, tend = w.tendencies(oa.default_config())

    def rhs():
        tend.compute_momentum_tendencies(state, aux, tracers, stream=stream)

    t_bolus, t_mix, t_col, t_5b, t_rhs = w.time([bolus, velocity_mix, column, step5b, rhs])
    with_rate(t_bolus, gm_bytes)
    with_rate(t_mix, mix_bytes)
    res["calls"].update(bolus_velocity=t_bolus, velocity_vert_mix=t_mix, column_pass_displaced=t_col, step_5b=t_5b,
                        momentum_rhs=t_rhs)
    res["bolus_over_velocity_vert_mix"] = t_bolus["ms_median"] / t_mix["ms_median"]
    res["step_5b_over_momentum_rhs"] = t_5b["ms_median"] / t_rhs["ms_median"]
    u = gm.get("BolusVelocity")[: mesh.NEdgesAll]
    res["bolus_finite"], res["bolus_max_abs"] = bool(np.isfinite(u).all()), float(np.abs(u).max())
    emit(res, a.out)


if __name__ == "__main__":
    main()
