"""PressureGrad (PressureGrad.h) timed with device events at QU30 size: 462 400 cells x 80 levels in k-d order,
surface-attached layer ranges as in tools/probes/vert_mix_diag.py.  Times the pressure-gradient kernel alone, the
column pass alone, and -- alternating in one loop, in the same process -- the plain RHS (SSH gradient off), the layered
RHS (column pass + RHS + term: computeAllTendencies with the PressureGrad attached) and one RK4 step of each (plain:
stage updates fused; layered: stage updates as separate kernels).  Prints one JSON line and writes it to --out.

Algorithmic bytes of the term: 24 B per cell-level (PressureMid, GeopotentialMid, SpecVol, each row fetched once)
+ 16 B per active edge-level (the tendency read and written); on a hexagon mesh ~ 72 B per cell-level.

   python tools/probes/pressure_grad_diag.py [--nx 680] [--levels 80] [--tracers 6] [--iters 50] [--warmup 10]
          [--local-order kd] [--only-kernel] [--out FILE]
(--only-kernel: just the kernel, a few launches: the form to run under rocprofv3 --pmc or --kernel-trace.)
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
    ap.add_argument("--tracers", type=int, default=6)
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
    gm = oa.GlobalMesh(g)
    decomp = oa.Decomp(gm, 1, 0, 3, local_order=a.local_order)
    mesh = oa.HorzMesh(decomp, K)
    ns, nes = mesh.NCellsSize, mesh.NEdgesSize
    state = oa.OceanState(mesh, None, K, 2)
    tracers = oa.Tracers(mesh, None, K, NT, 2)
    state.copy_to_device(rng.uniform(1.0, 50.0, (ns, K)), rng.uniform(-0.05, 0.05, (nes, K)), 0)
    tr = np.concatenate([rng.uniform(-2.0, 30.0, (1, ns, K)), rng.uniform(30.0, 38.0, (1, ns, K)),
                         rng.uniform(-1.0, 1.0, (NT - 2, ns, K))])
    tracers.copy_to_device(tr, 0)
    del tr
    vc = oa.VertCoord(mesh, K, 1026.0, "Uniform", min_level, max_level, decomp=decomp)
    eos = oa.Eos(mesh, K, "teos10")
    pg = oa.PressureGrad(mesh, vc, eos)
    stream = oa.Stream()
    hp, trp = state.device_ptr(0, 0), tracers.device_ptr(0)
    pg.update_column(hp, trp, NT, stream=stream)
    stream.synchronize()
    scratch = oa.DeviceBuffer(np.zeros((nes, oa.level_pitch(K))))

    elo, ehi = vc.get("MinLayerEdgeBot")[: mesh.NEdgesAll], vc.get("MaxLayerEdgeTop")[: mesh.NEdgesAll]
    eactive = int(np.sum(np.where((elo >= 0) & (elo <= ehi), ehi - elo + 1, 0)))
    cell_levels = mesh.NCellsAll * K
    term_bytes = 24 * cell_levels + 16 * eactive
    res = {"probe": "pressure_grad_diag", "ncells": mesh.NCellsAll, "nedges": mesh.NEdgesAll, "levels": K, "tracers": NT,
           "local_order": a.local_order, "active_edge_levels": eactive, "iters": a.iters, "peak_TBs": PEAK_TBS,
           "term_algorithmic_GB": term_bytes / 1.0e9, "term_B_per_cell_level": term_bytes / cell_levels, "calls": {}}

    def term():
        pg.compute(scratch.ptr, stream=stream)

    if a.only_kernel:
        for _ in range(a.iters):
            term()
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

    t = timed([term])[0]
    t["algorithmic_GB"] = term_bytes / 1.0e9
    t["TBs"] = t["algorithmic_GB"] / t["ms_median"]
    t["share_of_8TBs"] = t["TBs"] / PEAK_TBS
    res["calls"]["pressure_grad"] = t
    t = timed([lambda: pg.update_column(hp, trp, NT, stream=stream)])[0]
    t["algorithmic_GB"] = 72 * cell_levels / 1.0e9
    t["TBs"] = t["algorithmic_GB"] / t["ms_median"]
    res["calls"]["column_pass"] = t

    # the RHS with and without the layered term, same state, same process, alternating
    cfg = oa.default_config(SSHTendencyEnable=0)
    aux = oa.AuxiliaryState(mesh, None, K, NT)
    aux.set_options(cfg.FluxThicknessUpwind, cfg.FluxTracerUpwind, cfg.WindInterpIsotropic)
    plain = oa.Tendencies(mesh, K, NT, cfg)
    layered = oa.Tendencies(mesh, K, NT, cfg)
    layered.attach_pressure_grad(pg)
    rhs = timed([lambda: plain.compute_all_tendencies(state, aux, tracers, stream=stream),
                 lambda: layered.compute_all_tendencies(state, aux, tracers, stream=stream)])
    res["calls"]["rhs_plain"], res["calls"]["rhs_layered"] = rhs
    res["rhs_layered_over_plain"] = rhs[1]["ms_median"] / rhs[0]["ms_median"]
    # one RK4 step of each (a small step from the same start every time would need a state copy: the steps run on, the
    # fields stay smooth for the few steps timed)
    a.iters, a.warmup = max(a.iters // 5, 4), 2
    st_plain = oa.TimeStepper("RungeKutta4", 1.0, plain, aux, mesh, None, tracers)
    st_layered = oa.TimeStepper("RungeKutta4", 1.0, layered, aux, mesh, None, tracers)
    steps = timed([lambda: st_plain.do_step(state, stream=stream), lambda: st_layered.do_step(state, stream=stream)])
    res["calls"]["rk4_step_plain_stage_fused"], res["calls"]["rk4_step_layered_unfused"] = steps
    res["rk4_layered_over_plain"] = steps[1]["ms_median"] / steps[0]["ms_median"]
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
