"""Tendencies::computeMomentumTendencies and Tendencies::computeTransportTendenciesAndUpdate (Tendencies.h) against the
paths they replace, timed with device events at QU30 size: the workload of tools/probes/split_explicit_diag.py and
tools/probes/transport_diag.py (462 400 cells x 80 levels in k-d order, surface-attached layer ranges, 6 tracers).
Alternated in one process, each as the median of --iters after --warmup:
  rhs_fused                    one fused RHS evaluation (compute_all_tendencies), the unit the step's cost is quoted in
  momentum_rhs                 compute_momentum_tendencies (the fused RHS without its tracer half)
  sequence_1, sequence_2       compute_transport_tendencies + update_by_tend + update_tracers_by_tend: the path the folded
                               call replaces, which stays in the library, timed before and after the new calls: the
                               difference of the two medians is its own run-to-run spread
  transport_alone              compute_transport_tendencies, so that the update pair's share of the sequence is known
  folded_keep, folded_drop     compute_transport_tendencies_and_update with KeepTendencies on / off
  step_<momentum>_<fold>       one Split-Explicit step at --nsub under each combination of set_momentum_rhs and
                               set_folded_updates (fused transport on); step_off_off is timed twice, first and last: the
                               difference is the step's own spread
Records bitwise equality of the paths on the timed workload.  Prints one JSON line and writes it to --out.

Bytes model per cell-level of a hexagon mesh (3 edge rows per cell), 8 B values, hyperdiffusion on:
  transport call               40 + 40 NT      (transport_diag.py)
  the two update kernels       24 + (24 NT + 16): h, tendency, new h; per tracer the tracer, its tendency and the new one,
                               plus both thicknesses
  folded, tendencies kept      transport + 8 (the new thickness, launch 1; the cell's own thickness is among the rows it
                               gathers anyway) + 16 + 16 NT (launch 2: both thicknesses, per tracer the tracer at the own
                               cell and the new one) = transport + 24 + 16 NT; with the hyperdiffusion term off the tracer
                               update is in launch 1 and costs the new tracers only: transport + 8 + 8 NT
  folded, tendencies dropped   8 + 8 NT less: the thickness tendency and the final tracer tendency are not stored

   python tools/probes/momentum_update_diag.py [--nx 680] [--levels 80] [--tracers 6] [--nsub 30] [--dt 600] [--iters 50]
          [--warmup 10] [--local-order kd] [--hyperdiff 1] [--out FILE]
"""
import argparse

import numpy as np
from probe_rig import PEAK_TBS, Qu30Rig, add_common_args, emit, oa, summarise, with_rate


def main(argv=None):
    ap = argparse.ArgumentParser()
    add_common_args(ap, nx=680, levels=80, tracers=6, nsub=30, dt=600.0, iters=50, warmup=10, local_order="kd")
    ap.add_argument("--hyperdiff", type=int, default=1, help="TracerHyperDiffTendencyEnable: 0 puts the tracer update in launch 1")
    a = ap.parse_args(argv)
    w = Qu30Rig(a, bottom="layers")
    K, NT, mesh, ns, state, tracers, vc, reset = w.K, w.NT, w.mesh, w.ns, w.state, w.tracers, w.vc, w.reset
    bm = oa.BarotropicMode(mesh, vc)
    cfg = oa.default_config(TracerHyperDiffTendencyEnable=a.hyperdiff)
    aux, tend = w.tendencies(cfg)
    stream = w.stream
    nc, ne, pitch = w.nc, w.ne, w.P
    coeff = oa.coeff_seconds(1.0, a.dt)
    h_cur, h_next = state.device_ptr(0, 0), state.device_ptr(0, 1)
    tr_cur, tr_next = tracers.device_ptr(0), tracers.device_ptr(1)
    h_tend, tr_tend = tend.device_ptr(0)[0], tend.device_ptr(2)[0]
    sh = stream.h.value  # (the raw-pointer update calls take the stream as an address)

    def rhs():
        tend.compute_all_tendencies(state, aux, tracers, stream=stream)

    def momentum():
        tend.compute_momentum_tendencies(state, aux, tracers, stream=stream)

    def transport():
        tend.compute_transport_tendencies(state, aux, tracers, 0, 0, 1, stream=stream)

    def sequence():
        transport()
        oa.update_by_tend(h_next, h_cur, h_tend, coeff, nc, pitch, sh)
        oa.update_tracers_by_tend(tr_next, tr_cur, h_next, h_cur, tr_tend, coeff, NT, nc, ns, pitch, sh)

    def folded(keep):
        tend.compute_transport_tendencies_and_update(state, aux, tracers, 0, 0, 1, 1, 1, coeff, keep, stream=stream)

    hyper = bool(cfg.TracerHyperDiffTendencyEnable)
    cl = nc * K
    b_transport = 40 + (40 if hyper else 16) * NT
    nbytes = {"transport": cl * b_transport, "sequence": cl * (b_transport + 24 + 24 * NT + 16),
              "folded_keep": cl * (b_transport + ((24 + 16 * NT) if hyper else (8 + 8 * NT))),
              "folded_drop": cl * (b_transport + ((24 + 16 * NT) if hyper else (8 + 8 * NT)) - 8 - 8 * NT)}
    res = {"probe": "momentum_update_diag", "ncells": nc, "nedges": ne, "levels": K, "tracers": NT, "nsub": a.nsub,
           "dt": a.dt, "coeff": coeff, "local_order": a.local_order, "iters": a.iters, "warmup": a.warmup,
           "peak_TBs": PEAK_TBS, "tracer_hyperdiffusion": hyper, "calls": {}}
    c = res["calls"]
    c["rhs_fused"] = w.time([rhs])[0]
    c["momentum_rhs"] = w.time([momentum])[0]
    c["sequence_1"] = w.time([sequence])[0]
    c["transport_alone"] = w.time([transport])[0]
    c["folded_keep"] = w.time([lambda: folded(True)])[0]
    c["folded_drop"] = w.time([lambda: folded(False)])[0]
    c["sequence_2"] = w.time([sequence])[0]
    for name, key in (("sequence_1", "sequence"), ("sequence_2", "sequence"), ("transport_alone", "transport"),
                      ("folded_keep", "folded_keep"), ("folded_drop", "folded_drop")):
        with_rate(c[name], nbytes[key])

    # ---- the same bits on the timed workload
    def same(x, y):
        return bool(np.array_equal(x.view(np.uint64), y.view(np.uint64)))

    eq = res["bitwise"] = {}
    rhs()
    stream.synchronize()
    ref_u, ref_h = tend.get(1)[:ne].copy(), tend.get(0)[:nc].copy()
    momentum()
    stream.synchronize()
    eq["momentum_equals_rhs_velocity_tend"] = same(ref_u, tend.get(1)[:ne])
    eq["momentum_equals_rhs_thickness_tend"] = same(ref_h, tend.get(0)[:nc])
    sequence()
    stream.synchronize()
    want = (state.copy_to_host(1)[0][:nc].copy(), tracers.copy_to_host(1)[:, :nc].copy(), tend.get(0)[:nc].copy(),
            tend.get(2)[:, :nc].copy())
    for keep in (True, False):
        state.copy_to_device(w.h0, w.u0, 1)
        tracers.copy_to_device(w.tr0, 1)
        folded(keep)
        stream.synchronize()
        tag = "keep" if keep else "drop"
        eq[f"folded_{tag}_thickness"] = same(want[0], state.copy_to_host(1)[0][:nc])
        eq[f"folded_{tag}_tracers"] = same(want[1], tracers.copy_to_host(1)[:, :nc])
        if keep:
            eq["folded_keep_thickness_tend"] = same(want[2], tend.get(0)[:nc])
            eq["folded_keep_tracer_tend"] = same(want[3], tend.get(2)[:, :nc])

    # ---- whole steps (the calm start again every 5 steps, as in split_explicit_diag.py)
    se = oa.TimeStepper("Split-Explicit", a.dt, tend, aux, mesh, None, tracers)
    se.attach_barotropic(bm, a.nsub)
    se.set_fused_transport(True)
    combos = (("step_off_off", False, False), ("step_on_off", True, False), ("step_off_on", False, True),
              ("step_on_on", True, True), ("step_off_off_again", False, False))
    finals = {}
    for name, mom, fold in combos:
        se.set_momentum_rhs(mom)
        se.set_folded_updates(fold)
        c[name] = w.time([lambda: se.do_step(state, stream=stream)], before=reset, every=5)[0]
        reset()
        for _ in range(3):
            se.do_step(state, stream=stream)
        stream.synchronize()
        h, u = state.copy_to_host(0)
        finals[name] = (h[:nc].copy(), u[:ne].copy(), tracers.copy_to_host(0)[:, :nc].copy())
    base = finals["step_off_off"]
    eq["steps_equal_both_switches_off"] = {name: all(same(x, y) for x, y in zip(base, f)) for name, f in finals.items()}
    r = c["rhs_fused"]["ms_median"]
    for t in c.values():
        t["fraction_of_rhs"] = t["ms_median"] / r
    seq, seq_spread = summarise(c, ["sequence"]).values()
    step = 0.5 * (c["step_off_off"]["ms_median"] + c["step_off_off_again"]["ms_median"])
    step_spread = abs(c["step_off_off"]["ms_median"] - c["step_off_off_again"]["ms_median"])
    s = res["summary"] = {"rhs_ms": r, "momentum_ms": c["momentum_rhs"]["ms_median"],
                          "momentum_saving_ms": r - c["momentum_rhs"]["ms_median"],
                          "sequence_ms": seq, "sequence_spread_ms": seq_spread,
                          "update_pair_ms": seq - c["transport_alone"]["ms_median"],
                          "folded_keep_ms": c["folded_keep"]["ms_median"], "folded_drop_ms": c["folded_drop"]["ms_median"],
                          "folded_keep_saving_ms": seq - c["folded_keep"]["ms_median"],
                          "folded_drop_saving_ms": seq - c["folded_drop"]["ms_median"],
                          "step_both_off_ms": step, "step_spread_ms": step_spread}
    for name in ("step_on_off", "step_off_on", "step_on_on"):
        s[name + "_saving_ms"] = step - c[name]["ms_median"]
        s[name + "_faster_by_more_than_the_spread"] = bool(step - c[name]["ms_median"] > step_spread)
    s["all_bitwise_equal"] = bool(all(v if isinstance(v, bool) else all(v.values()) for v in eq.values()))
    emit(res, a.out)


if __name__ == "__main__":
    main()
