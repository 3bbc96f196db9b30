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
    ap.add_argument("--nsub", type=int, default=30)
    ap.add_argument("--dt-btr", type=float, default=20.0)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--local-order", default="kd")
    ap.add_argument("--only-kernels", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    K, NT = a.levels, a.tracers
    oa.device_init(0)
    g = planar_hex(a.nx, a.nx, 30.0e3, bottom_depth=4000.0)
    n = int(g["nCells"])
    rng = np.random.default_rng(2026)
    min_level = np.ones(n, np.int32)
    max_level = np.where(rng.random(n) < 0.6, K, rng.integers(5, K + 1, n)).astype(np.int32)
    decomp = oa.Decomp(oa.GlobalMesh(g), 1, 0, 3, local_order=a.local_order)
    mesh = oa.HorzMesh(decomp, K)
    ns, nes = mesh.NCellsSize, mesh.NEdgesSize
    state = oa.OceanState(mesh, None, K, 2)
    tracers = oa.Tracers(mesh, None, K, NT, 2)
    state.copy_to_device(rng.uniform(1.0, 50.0, (ns, K)), rng.uniform(-0.05, 0.05, (nes, K)), 0)
    tracers.copy_to_device(rng.uniform(-1.0, 1.0, (NT, ns, K)), 0)
    vc = oa.VertCoord(mesh, K, 1026.0, "Uniform", min_level, max_level, decomp=decomp)
    bm = oa.BarotropicMode(mesh, vc)
    stream = oa.Stream()
    hp, up = state.device_ptr(0, 0), state.device_ptr(1, 0)
    pitch = oa.level_pitch(K)
    ut = oa.DeviceBuffer(np.pad(rng.uniform(-1.0e-6, 1.0e-6, (nes, K)), ((0, 0), (0, pitch - K))))
    ur = oa.DeviceBuffer(np.zeros((nes, pitch)))

    lo, hi = vc.get("MinLayerCell")[: mesh.NCellsAll], vc.get("MaxLayerCell")[: mesh.NCellsAll]
    cactive = int(np.sum(np.where((lo >= 0) & (lo <= hi), hi - lo + 1, 0)))
    elo, ehi = vc.get("MinLayerEdgeBot")[: mesh.NEdgesAll], vc.get("MaxLayerEdgeTop")[: mesh.NEdgesAll]
    eactive = int(np.sum(np.where((elo >= 0) & (elo <= ehi), ehi - elo + 1, 0)))
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
        print(json.dumps(res))
        return

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        stream.synchronize()
        evs = [[oa.Event() for _ in range(2)] for _ in range(a.iters)]
        for e0, e1 in evs:
            e0.record(stream)
            fn()
            e1.record(stream)
        stream.synchronize()
        per = np.array([e0.elapsed_ms(e1) for e0, e1 in evs])
        return {"ms_median": float(np.median(per)), "ms_min": float(per.min()), "ms_max": float(per.max())}

    cfg = oa.default_config()
    aux = oa.AuxiliaryState(mesh, None, K, NT)
    aux.set_options(cfg.FluxThicknessUpwind, cfg.FluxTracerUpwind, cfg.WindInterpIsotropic)
    tend = oa.Tendencies(mesh, K, NT, cfg)
    rhs = timed(lambda: tend.compute_all_tendencies(state, aux, tracers, stream=stream))
    res["calls"]["rhs_fused"] = rhs
    for name, fn in calls.items():
        if name == "subcycle":
            reset()
        t = timed(fn)
        t["algorithmic_GB"] = nbytes[name] / 1.0e9
        t["TBs"] = t["algorithmic_GB"] / t["ms_median"]
        t["share_of_8TBs"] = t["TBs"] / PEAK_TBS
        if name in issued:
            t["issued_GB"] = issued[name] / 1.0e9
            t["issued_TBs"] = t["issued_GB"] / t["ms_median"]
        t["fraction_of_rhs"] = t["ms_median"] / rhs["ms_median"]
        res["calls"][name] = t
    res["calls"]["subcycle"]["us_per_substep"] = 1.0e3 * res["calls"]["subcycle"]["ms_median"] / a.nsub
    res["state_finite_after_subcycles"] = bool(np.isfinite(bm.get("SSH")[:nc]).all() and
                                                np.isfinite(bm.get("BtrVelocity")[:ne]).all())
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
