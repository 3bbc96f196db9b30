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
    ap.add_argument("--hyperdiff", type=int, default=1, help="TracerHyperDiffTendencyEnable: 0 puts the tracer update in launch 1")
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
    cfg = oa.default_config(TracerHyperDiffTendencyEnable=a.hyperdiff)
    aux = oa.AuxiliaryState(mesh, None, K, NT)
    aux.set_options(cfg.FluxThicknessUpwind, cfg.FluxTracerUpwind, cfg.WindInterpIsotropic)
    tend = oa.Tendencies(mesh, K, NT, cfg)
    stream = oa.Stream()
    nc, ne, pitch = mesh.NCellsAll, mesh.NEdgesAll, oa.level_pitch(K)
    coeff = oa.coeff_seconds(1.0, a.dt)
    h_cur, h_next = state.device_ptr(0, 0), state.device_ptr(0, 1)
    tr_cur, tr_next = tracers.device_ptr(0), tracers.device_ptr(1)
    h_tend, tr_tend = tend.device_ptr(0)[0], tend.device_ptr(2)[0]
    sh = stream.h.value  # (the raw-pointer update calls take the stream as an address)

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
    c["rhs_fused"] = timed(rhs)
    c["momentum_rhs"] = timed(momentum)
    c["sequence_1"] = timed(sequence)
    c["transport_alone"] = timed(transport)
    c["folded_keep"] = timed(lambda: folded(True))
    c["folded_drop"] = timed(lambda: folded(False))
    c["sequence_2"] = timed(sequence)
    for name, key in (("sequence_1", "sequence"), ("sequence_2", "sequence"), ("transport_alone", "transport"),
                      ("folded_keep", "folded_keep"), ("folded_drop", "folded_drop")):
        c[name]["algorithmic_GB"] = nbytes[key] / 1.0e9
        c[name]["TBs"] = c[name]["algorithmic_GB"] / c[name]["ms_median"]
        c[name]["share_of_8TBs"] = c[name]["TBs"] / PEAK_TBS

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
        state.copy_to_device(h0, u0, 1)
        tracers.copy_to_device(tr0, 1)
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
        c[name] = timed(lambda: se.do_step(state, stream=stream), before=reset, every=5)
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
    seq = 0.5 * (c["sequence_1"]["ms_median"] + c["sequence_2"]["ms_median"])
    seq_spread = abs(c["sequence_1"]["ms_median"] - c["sequence_2"]["ms_median"])
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
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f_:
            f_.write(line + "\n")


if __name__ == "__main__":
    main()
