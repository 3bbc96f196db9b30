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
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import omega_amd as oa  # noqa: E402
from omega_amd.meshgen import planar_hex  # noqa: E402

PEAK_TBS = 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=680)
    ap.add_argument("--levels", type=int, default=80)
    ap.add_argument("--tracers", type=int, default=2)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--local-order", default="kd")
    ap.add_argument("--only-kernel", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    K, NT = a.levels, a.tracers
    oa.device_init(0)
    g = planar_hex(a.nx, a.nx, 30.0e3)
    n = int(g["nCells"])
    rng = np.random.default_rng(2026)
    min_level = np.ones(n, np.int32)
    max_level = np.where(rng.random(n) < 0.6, K, rng.integers(5, K + 1, n)).astype(np.int32)
    gmesh = oa.GlobalMesh(g)
    decomp = oa.Decomp(gmesh, 1, 0, 3, local_order=a.local_order)
    mesh = oa.HorzMesh(decomp, K)
    ns, nes = mesh.NCellsSize, mesh.NEdgesSize
    state = oa.OceanState(mesh, None, K, 2)
    tracers = oa.Tracers(mesh, None, K, NT, 2)
    state.copy_to_device(rng.uniform(1.0, 50.0, (ns, K)), rng.uniform(-0.05, 0.05, (nes, K)), 0)
    # a stable column (T falls, S rises with depth) with noise across the cells: fronts for the closure to act on
    k = np.arange(K)[None, None, :]
    tr = np.concatenate([20.0 - 0.2 * k + rng.uniform(-0.5, 0.5, (1, ns, K)), 34.0 + 0.02 * k + rng.uniform(-0.1, 0.1, (1, ns, K)),
                         rng.uniform(-1.0, 1.0, (NT - 2, ns, K))])
    tracers.copy_to_device(tr, 0)
    del tr
    vc = oa.VertCoord(mesh, K, 1026.0, "Uniform", min_level, max_level, decomp=decomp)
    eos = oa.Eos(mesh, K, "teos10")
    gm = oa.GentMcWilliams(mesh, vc, eos)
    stream = oa.Stream()
    hp, up, trp = state.device_ptr(0, 0), state.device_ptr(1, 0), tracers.device_ptr(0)
    gm.update_column(hp, trp, NT, stream=stream)
    stream.synchronize()
    transport = oa.DeviceBuffer(np.zeros((nes, oa.level_pitch(K))))

    elo, ehi = vc.get("MinLayerEdgeBot")[: mesh.NEdgesAll], vc.get("MaxLayerEdgeTop")[: mesh.NEdgesAll]
    eactive = int(np.sum(np.where((elo >= 0) & (elo <= ehi), ehi - elo + 1, 0)))
    cell_levels = mesh.NCellsAll * K
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

    if a.only_kernel:
        for _ in range(a.iters):
            bolus()
        stream.synchronize()
        print(json.dumps(res))
        return

    def timed(fns):
        """median / min / max ms of each fn, the fns alternating in one loop"""
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
            out.append({"ms_median": float(np.median(per)), "ms_min": float(per.min()), "ms_max": float(per.max())})
        return out

    # the yardstick: the implicit velocity mixing on the same columns (coefficients from the same stratification)
    vm = oa.VertMix(mesh, vc)
    vm.compute_bvf(eos, stream=stream)
    vm.compute(up, up, stream=stream)
    mixed = oa.DeviceBuffer(np.zeros((nes, oa.level_pitch(K))))

    def velocity_mix():
        vm.apply_velocity(hp, mixed.ptr, 600.0, stream=stream)

    cfg = oa.default_config()
    aux = oa.AuxiliaryState(mesh, None, K, NT)
    aux.set_options(cfg.FluxThicknessUpwind, cfg.FluxTracerUpwind, cfg.WindInterpIsotropic)
    tend = oa.Tendencies(mesh, K, NT, cfg)

    def rhs():
        tend.compute_momentum_tendencies(state, aux, tracers, stream=stream)

    t_bolus, t_mix, t_col, t_5b, t_rhs = timed([bolus, velocity_mix, column, step5b, rhs])
    for t, nbytes in ((t_bolus, gm_bytes), (t_mix, mix_bytes)):
        t["algorithmic_GB"] = nbytes / 1.0e9
        t["TBs"] = t["algorithmic_GB"] / t["ms_median"]
        t["share_of_8TBs"] = t["TBs"] / PEAK_TBS
    res["calls"].update(bolus_velocity=t_bolus, velocity_vert_mix=t_mix, column_pass_displaced=t_col, step_5b=t_5b,
                        momentum_rhs=t_rhs)
    res["bolus_over_velocity_vert_mix"] = t_bolus["ms_median"] / t_mix["ms_median"]
    res["step_5b_over_momentum_rhs"] = t_5b["ms_median"] / t_rhs["ms_median"]
    u = gm.get("BolusVelocity")[: mesh.NEdgesAll]
    res["bolus_finite"], res["bolus_max_abs"] = bool(np.isfinite(u).all()), float(np.abs(u).max())
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
