"""Tendencies::computeTransportTendencies (Tendencies.h) against the two group calls it replaces, timed with device
events at QU30 size: the workload of tools/probes/split_explicit_diag.py (462 400 cells x 80 levels in k-d order,
surface-attached layer ranges, 6 tracers).  Alternated in one process, each as the median of --iters after --warmup:
  group_pair_1, group_pair_2   compute_thickness_tendencies + compute_tracer_tendencies (five launches), timed twice:
                               the difference of the two medians is the pair's own run-to-run spread
  fused_transport              compute_transport_tendencies (two launches)
  split_explicit_step_groups / split_explicit_step_fused
                               one Split-Explicit step at --nsub with set_fused_transport(False) / (True)
  rhs_fused                    one fused RHS evaluation, the unit the step's cost is quoted in
Prints one JSON line and writes it to --out.

Bytes model per cell-level of a hexagon mesh (6 edges per cell shared by two cells: 3 edge rows per cell), 8 B values:
  fused, hyperdiffusion on    launch 1 reads h, 3 u, NT tracers, writes the thickness tendency, NT tendencies and NT del2:
                              40 + 24 NT; launch 2 reads NT del2 and updates NT tendencies in place (counted once):
                              16 NT more -> 40 + 40 NT (48 NT with the reload and the second store counted apart)
  fused, hyperdiffusion off   40 + 16 NT
  the five group launches     192 + 96 NT (the edge-located intermediates written and read back, 3 edge rows per cell each)

   python tools/probes/transport_diag.py [--nx 680] [--levels 80] [--tracers 6] [--nsub 30] [--dt 600] [--iters 50]
          [--warmup 10] [--local-order kd] [--out FILE]
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
    ap.add_argument("--dt", type=float, default=600.0)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--local-order", default="kd")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    K, NT = a.levels, a.tracers
    oa.device_init(0)
    layer = 50.0
    g = planar_hex(a.nx, a.nx, 30.0e3, bottom_depth=layer * K)
    n = int(g["nCells"])
    rng = np.random.default_rng(2026)
    min_level = np.ones(n, np.int32)
    max_level = np.where(rng.random(n) < 0.6, K, rng.integers(5, K + 1, n)).astype(np.int32)
    decomp = oa.Decomp(oa.GlobalMesh(g), 1, 0, 3, local_order=a.local_order)
    mesh = oa.HorzMesh(decomp, K)
    ns, nes = mesh.NCellsSize, mesh.NEdgesSize
    state = oa.OceanState(mesh, None, K, 2)
    tracers = oa.Tracers(mesh, None, K, NT, 2)
    h0, u0 = layer + rng.uniform(-1.0e-3, 1.0e-3, (ns, K)), rng.uniform(-1.0e-3, 1.0e-3, (nes, K))
    tr0 = rng.uniform(-1.0, 1.0, (NT, ns, K))

    def reset():
        for lvl in (0, 1):
            state.copy_to_device(h0, u0, lvl)
            tracers.copy_to_device(tr0, lvl)

    reset()
    vc = oa.VertCoord(mesh, K, 1026.0, "Uniform", min_level, max_level, decomp=decomp)
    bm = oa.BarotropicMode(mesh, vc)
    cfg = oa.default_config()
    aux = oa.AuxiliaryState(mesh, None, K, NT)
    aux.set_options(cfg.FluxThicknessUpwind, cfg.FluxTracerUpwind, cfg.WindInterpIsotropic)
    tend = oa.Tendencies(mesh, K, NT, cfg)
    stream = oa.Stream()
    nc = mesh.NCellsAll

    def timed(fn, before=None, every=0):
        for _ in range(a.warmup):
            fn()
        stream.synchronize()
        evs = [[oa.Event() for _ in range(2)] for _ in range(a.iters)]
        for i, (e0, e1) in enumerate(evs):
            if before and (i == 0 or (every and i % every == 0)):
                stream.synchronize()
                before()
            e0.record(stream)
            fn()
            e1.record(stream)
        stream.synchronize()
        per = np.array([e0.elapsed_ms(e1) for e0, e1 in evs])
        return {"ms_median": float(np.median(per)), "ms_min": float(per.min()), "ms_max": float(per.max())}

    def group_pair():
        tend.compute_thickness_tendencies(state, aux, 0, 1, stream=stream)
        tend.compute_tracer_tendencies(state, aux, tracers, 0, 0, 1, stream=stream)

    def fused():
        tend.compute_transport_tendencies(state, aux, tracers, 0, 0, 1, stream=stream)

    hyper = bool(cfg.TracerHyperDiffTendencyEnable)
    cell_levels = nc * K
    nbytes = {"fused": cell_levels * (40 + (40 if hyper else 16) * NT), "groups": cell_levels * (192 + 96 * NT)}
    res = {"probe": "transport_diag", "ncells": nc, "nedges": mesh.NEdgesAll, "levels": K, "tracers": NT, "nsub": a.nsub,
           "dt": a.dt, "local_order": a.local_order, "iters": a.iters, "warmup": a.warmup, "peak_TBs": PEAK_TBS,
           "tracer_hyperdiffusion": hyper, "calls": {}}
    c = res["calls"]
    c["rhs_fused"] = timed(lambda: tend.compute_all_tendencies(state, aux, tracers, stream=stream))
    c["group_pair_1"] = timed(group_pair)
    c["fused_transport"] = timed(fused)
    c["group_pair_2"] = timed(group_pair)
    for name, key in (("group_pair_1", "groups"), ("group_pair_2", "groups"), ("fused_transport", "fused")):
        c[name]["algorithmic_GB"] = nbytes[key] / 1.0e9
        c[name]["TBs"] = c[name]["algorithmic_GB"] / c[name]["ms_median"]
        c[name]["share_of_8TBs"] = c[name]["TBs"] / PEAK_TBS
    # same bits on the timed workload: the last fused call against the last pair
    group_pair()
    stream.synchronize()
    ref = (tend.get(0)[:nc].copy(), tend.get(2)[:, :nc].copy())
    fused()
    stream.synchronize()
    res["fused_equals_group_pair_bitwise"] = bool(np.array_equal(ref[0].view(np.uint64), tend.get(0)[:nc].view(np.uint64)) and
                                                  np.array_equal(ref[1].view(np.uint64), tend.get(2)[:, :nc].view(np.uint64)))
    # whole steps (the calm start again every 5 steps, as in split_explicit_diag.py)
    se = oa.TimeStepper("Split-Explicit", a.dt, tend, aux, mesh, None, tracers)
    se.attach_barotropic(bm, a.nsub)
    for name, on in (("split_explicit_step_groups", False), ("split_explicit_step_fused", True)):
        se.set_fused_transport(on)
        c[name] = timed(lambda: se.do_step(state, stream=stream), before=reset, every=5)
    r = c["rhs_fused"]["ms_median"]
    for t in c.values():
        t["fraction_of_rhs"] = t["ms_median"] / r
    pair = 0.5 * (c["group_pair_1"]["ms_median"] + c["group_pair_2"]["ms_median"])
    spread = abs(c["group_pair_1"]["ms_median"] - c["group_pair_2"]["ms_median"])
    f = c["fused_transport"]["ms_median"]
    res["summary"] = {"group_pair_ms": pair, "group_pair_spread_ms": spread, "fused_ms": f, "fused_over_group_pair": f / pair,
                      "saving_ms": pair - f, "faster_by_more_than_the_spread": bool(pair - f > spread),
                      "bytes_model_fused_over_groups": nbytes["fused"] / nbytes["groups"],
                      "step_groups_over_rhs": c["split_explicit_step_groups"]["ms_median"] / r,
                      "step_fused_over_rhs": c["split_explicit_step_fused"]["ms_median"] / r}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f_:
            f_.write(line + "\n")


if __name__ == "__main__":
    main()
