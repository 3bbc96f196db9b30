"""VertAdv (VertAdv.h) timed with device events at QU30 size: 462 400 cells x 80 levels x 6 tracers in k-d order,
surface-attached layer ranges as in tools/probes/pressure_grad_diag.py.  Times each launch alone (median of --iters) and
-- alternating in one loop, in the same process -- the plain RHS against the RHS with the VertAdv attached, and one RK4
step of each (plain: stage updates fused; attached: stage updates as separate kernels).  Prints one JSON line and writes
it to --out.

Algorithmic bytes (VertAdv.h), on the active cell-levels / edge-levels of the ranges:
  transport 24 B per cell-level, transport + thickness 32 B, thickness alone 24 B,
  tracers (16 + 24 NT) B per cell-level, velocity 16 B per cell-level + 24 B per edge-level.

   python tools/probes/vert_adv_diag.py [--nx 680] [--levels 80] [--tracers 6] [--iters 50] [--warmup 10]
          [--local-order kd] [--only-kernels] [--out FILE]
(--only-kernels: just the launches, a few times: the form to run under rocprofv3 --pmc or --kernel-trace.)
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
    state.copy_to_device(rng.uniform(1.0, 50.0, (ns, K)), rng.uniform(-0.05, 0.05, (nes, K)), 0)
    tracers.copy_to_device(rng.uniform(-1.0, 1.0, (NT, ns, K)), 0)
    vc = oa.VertCoord(mesh, K, 1026.0, "Uniform", min_level, max_level, decomp=decomp)
    vc.set("RefLayerThickness", rng.uniform(1.0, 50.0, (ns, K)))
    va = oa.VertAdv(mesh, vc, 2)
    stream = oa.Stream()
    hp, up, trp = state.device_ptr(0, 0), state.device_ptr(1, 0), tracers.device_ptr(0)
    pitch = oa.level_pitch(K)
    d = oa.DeviceBuffer(np.pad(rng.uniform(-1.0e-6, 1.0e-6, (ns, K)), ((0, 0), (0, pitch - K))))
    tt = oa.DeviceBuffer(np.zeros((NT, ns, pitch)))
    ut = oa.DeviceBuffer(np.zeros((nes, pitch)))

    lo, hi = vc.get("MinLayerCell")[: mesh.NCellsAll], vc.get("MaxLayerCell")[: mesh.NCellsAll]
    cactive = int(np.sum(np.where((lo >= 0) & (lo <= hi), hi - lo + 1, 0)))
    elo, ehi = vc.get("MinLayerEdgeBot")[: mesh.NEdgesAll], vc.get("MaxLayerEdgeTop")[: mesh.NEdgesAll]
    eactive = int(np.sum(np.where((elo >= 0) & (elo <= ehi), ehi - elo + 1, 0)))
    nbytes = {"transport": 24 * cactive, "transport_and_thickness": 32 * cactive, "thickness": 24 * cactive,
              "tracers": (16 + 24 * NT) * cactive, "velocity": 16 * cactive + 24 * eactive}
    calls = {"transport": lambda: va.compute_transport(d.ptr, stream=stream),
             "transport_and_thickness": lambda: va.compute_transport(d.ptr, add_thickness=True, stream=stream),
             "thickness": lambda: va.add_thickness(d.ptr, stream=stream),
             "tracers": lambda: va.add_tracers(tt.ptr, hp, trp, NT, stream=stream),
             "velocity": lambda: va.add_velocity(ut.ptr, hp, up, stream=stream)}
    res = {"probe": "vert_adv_diag", "ncells": mesh.NCellsAll, "nedges": mesh.NEdgesAll, "levels": K, "tracers": NT,
           "local_order": a.local_order, "active_cell_levels": cactive, "active_edge_levels": eactive, "iters": a.iters,
           "peak_TBs": PEAK_TBS, "calls": {}}

    if a.only_kernels:
        for _ in range(a.iters):
            for fn in calls.values():
                fn()
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

    for name, fn in calls.items():
        t = timed([fn])[0]
        t["algorithmic_GB"] = nbytes[name] / 1.0e9
        t["TBs"] = t["algorithmic_GB"] / t["ms_median"]
        t["share_of_8TBs"] = t["TBs"] / PEAK_TBS
        res["calls"][name] = t

    # the RHS with and without the terms, same state, same process, alternating
    cfg = oa.default_config()
    aux = oa.AuxiliaryState(mesh, None, K, NT)
    aux.set_options(cfg.FluxThicknessUpwind, cfg.FluxTracerUpwind, cfg.WindInterpIsotropic)
    plain = oa.Tendencies(mesh, K, NT, cfg)
    attached = oa.Tendencies(mesh, K, NT, cfg)
    attached.attach_vert_adv(va)
    rhs = timed([lambda: plain.compute_all_tendencies(state, aux, tracers, stream=stream),
                 lambda: attached.compute_all_tendencies(state, aux, tracers, stream=stream)])
    res["calls"]["rhs_plain"], res["calls"]["rhs_attached"] = rhs
    res["rhs_attached_over_plain"] = rhs[1]["ms_median"] / rhs[0]["ms_median"]
    a.iters, a.warmup = max(a.iters // 5, 4), 2
    st_plain = oa.TimeStepper("RungeKutta4", 1.0, plain, aux, mesh, None, tracers)
    st_attached = oa.TimeStepper("RungeKutta4", 1.0, attached, aux, mesh, None, tracers)
    steps = timed([lambda: st_plain.do_step(state, stream=stream), lambda: st_attached.do_step(state, stream=stream)])
    res["calls"]["rk4_step_plain_stage_fused"], res["calls"]["rk4_step_attached_unfused"] = steps
    res["rk4_attached_over_plain"] = steps[1]["ms_median"] / steps[0]["ms_median"]
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
