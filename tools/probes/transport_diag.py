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

import numpy as np
from probe_rig import PEAK_TBS, Qu30Rig, add_common_args, emit, oa, summarise, with_rate


def main(argv=None):
    ap = argparse.ArgumentParser()
    add_common_args(ap, nx=680, levels=80, tracers=6, nsub=30, dt=600.0, iters=50, warmup=10, local_order="kd")
    a = ap.parse_args(argv)
    w = Qu30Rig(a, bottom="layers")
    K, NT, mesh, nc, state, tracers, vc = w.K, w.NT, w.mesh, w.nc, w.state, w.tracers, w.vc
    bm = oa.BarotropicMode(mesh, vc)
    cfg = oa.default_config()
    aux, tend = w.tendencies(cfg)
    stream = w.stream

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
    c["rhs_fused"] = w.time([lambda: tend.compute_all_tendencies(state, aux, tracers, stream=stream)])[0]
    c["group_pair_1"] = w.time([group_pair])[0]
    c["fused_transport"] = w.time([fused])[0]
    c["group_pair_2"] = w.time([group_pair])[0]
    for name, key in (("group_pair_1", "groups"), ("group_pair_2", "groups"), ("fused_transport", "fused")):
        with_rate(c[name], nbytes[key])
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
        c[name] = w.time([lambda: se.do_step(state, stream=stream)], before=w.reset, every=5)[0]
    r = c["rhs_fused"]["ms_median"]
    for t in c.values():
        t["fraction_of_rhs"] = t["ms_median"] / r
    s = res["summary"] = summarise(c, ["group_pair"])
    pair, spread, f = s["group_pair_ms"], s["group_pair_spread_ms"], c["fused_transport"]["ms_median"]
    s.update({"fused_ms": f, "fused_over_group_pair": f / pair, "saving_ms": pair - f,
              "faster_by_more_than_the_spread": bool(pair - f > spread),
              "bytes_model_fused_over_groups": nbytes["fused"] / nbytes["groups"],
              "step_groups_over_rhs": c["split_explicit_step_groups"]["ms_median"] / r,
              "step_fused_over_rhs": c["split_explicit_step_fused"]["ms_median"] / r})
    emit(res, a.out)


if __name__ == "__main__":
    main()
