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
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    K, NT = a.levels, a.tracers
    P = oa.level_pitch(K)
    oa.device_init(0)
    g = planar_hex(a.nx, a.nx, 30.0e3)
    n = int(g["nCells"])
    rng = np.random.default_rng(2026)
    min_level = np.ones(n, np.int32)
    max_level = np.where(rng.random(n) < 0.6, K, rng.integers(5, K + 1, n)).astype(np.int32)
    gm = oa.GlobalMesh(g)
    decomp = oa.Decomp(gm, 1, 0, 3)
    mesh = oa.HorzMesh(decomp, K)
    ns, nes, nown, eown = mesh.NCellsSize, mesh.NEdgesSize, mesh.NCellsOwned, mesh.NEdgesOwned
    state = oa.OceanState(mesh, None, K, 2)
    tracers = oa.Tracers(mesh, None, K, NT, 2)
    h = rng.uniform(1.0, 50.0, (ns, K))
    state.copy_to_device(h, rng.uniform(-0.05, 0.05, (nes, K)), 0)
    tr = np.concatenate([rng.uniform(-2.0, 30.0, (1, ns, K)), rng.uniform(30.0, 38.0, (1, ns, K)),
                         rng.uniform(-1.0, 1.0, (NT - 2, ns, K))])
    tracers.copy_to_device(tr, 0)
    del tr
    vc = oa.VertCoord(mesh, K, 1026.0, "Uniform", min_level, max_level, decomp=decomp)
    vc_full = oa.VertCoord(mesh, K, 1026.0, "Uniform")
    eos = oa.Eos(mesh, K, "teos10")
    vc.compute_column(state, tracers, eos, kdisp=1)
    vm = oa.VertMix(mesh, vc)
    vm_full = oa.VertMix(mesh, vc_full)
    ut = oa.DeviceBuffer(np.pad(rng.uniform(-0.05, 0.05, (nes, K)), ((0, 0), (0, P - K))))
    stream = oa.Stream()
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

    lo, hi = vc.get("MinLayerCell")[:nown], vc.get("MaxLayerCell")[:nown]
    active = int(np.sum(hi - lo + 1))
    elo, ehi = vc.get("MinLayerEdgeBot")[:eown], vc.get("MaxLayerEdgeTop")[:eown]
    eactive = int(np.sum(np.where((elo >= 0) & (elo <= ehi), ehi - elo + 1, 0)))
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
        for name, t in zip(grp, timed([calls[x] for x in grp])):
            t["algorithmic_GB"] = gb[name] / 1.0e9
            t["TBs"] = t["algorithmic_GB"] / t["ms_median"]
            t["share_of_8TBs"] = t["TBs"] / PEAK_TBS
            res["calls"][name] = t
    assert set(res["calls"]) == set(names)
    sepn = "separate_pcr_x%d" % NT
    res["full_columns_over_separate"] = res["calls"]["tracer_pass_full_columns"]["ms_median"] / \
        res["calls"][sepn]["ms_median"]
    res["tracer_pass_over_separate"] = res["calls"]["tracer_pass"]["ms_median"] / res["calls"][sepn]["ms_median"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
