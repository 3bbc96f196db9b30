"""MonotoneAdv::addTracerTend with the high-order horizontal flux (MonotoneAdv.h, setHorzOrder) against the centred
form, at QU30 size, timed with device events: the workload of tools/probes/monotone_adv_diag.py (462 400 cells x 80
levels in k-d order, 6 tracers), one MonotoneAdv object switched between the orders, so that order 2 is the parent's
path in the same binary.  Alternated in one process, each as the median of --iters after --warmup, every case timed
twice (the difference of the two medians is its own run-to-run spread):
  order2_1 / _2, order3_1 / _2, order4_1 / _2                add_tracers alone at each order (2, 3 and 3 launches)
  step_order2_1 / _2, step_order3_.., step_order4_..         one attached Split-Explicit step at --nsub at each order
Prints one JSON line and writes it to --out.
(--only-kernels: add_tracers alone at orders 2 and 4, --iters times each and nothing else: the form to run under
rocprofv3 --kernel-trace, which tells the launches apart.)

Bytes model per cell-level of a hexagon mesh, 8 B values, every row counted once per launch:
  order 2      pass 1 40 + 24 NT, pass 2 32 + 40 NT                            72 + 64 NT
  order 3, 4   pass 0 32 NT, pass 1 40 + 48 NT, pass 2 32 + 64 NT              72 + 144 NT
Hess is NT*3 rows per cell: 5.3 GB at this size with 6 tracers.

   python tools/probes/monotone_adv_ho_diag.py [--nx 680] [--levels 80] [--tracers 6] [--nsub 30] [--dt 600] [--iters 50]
          [--warmup 10] [--local-order kd] [--only-kernels] [--no-steps] [--out FILE]
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
ORDERS = (2, 3, 4)


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
    ap.add_argument("--only-kernels", action="store_true")
    ap.add_argument("--no-steps", action="store_true", help="the calls alone: no Split-Explicit step is timed")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    K, NT = a.levels, a.tracers
    oa.device_init(0)
    layer = 50.0
    g = planar_hex(a.nx, a.nx, 30.0e3, bottom_depth=layer * K)
    rng = np.random.default_rng(2026)
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
    vc = oa.VertCoord(mesh, K, 1026.0, "Uniform", decomp=decomp)
    vc.set("RefLayerThickness", np.full((ns, K), layer))
    bm = oa.BarotropicMode(mesh, vc)
    cfg = oa.default_config(TracerHorzAdvTendencyEnable=0)
    aux = oa.AuxiliaryState(mesh, None, K, NT)
    aux.set_options(cfg.FluxThicknessUpwind, cfg.FluxTracerUpwind, cfg.WindInterpIsotropic)
    tend = oa.Tendencies(mesh, K, NT, cfg)
    mono = oa.MonotoneAdv(mesh, K, NT, bool(cfg.FluxThicknessUpwind))
    geo = dict(x_period=float(g["x_period"]), y_period=float(g["y_period"]))

    def set_order(order):
        mono.set_horz_order(order, 0.25, **geo)

    stream = oa.Stream()
    nc = mesh.NCellsAll
    h_old, h_new, u_new = state.device_ptr(0, 0), state.device_ptr(0, 1), state.device_ptr(1, 1)
    tr_ptr, tend_ptr = tracers.device_ptr(0), tend.device_ptr(2)[0]

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

    def call():
        mono.add_tracers(tend_ptr, h_old, h_new, u_new, tr_ptr, NT, a.dt, stream=stream)

    per_level = {2: 72 + 64 * NT, 3: 72 + 144 * NT, 4: 72 + 144 * NT}
    res = {"probe": "monotone_adv_ho_diag", "ncells": nc, "nedges": mesh.NEdgesAll, "levels": K, "tracers": NT,
           "nsub": a.nsub, "dt": a.dt, "local_order": a.local_order, "iters": a.iters, "warmup": a.warmup,
           "peak_TBs": PEAK_TBS, "bytes_per_cell_level": {f"order{o}": b for o, b in per_level.items()},
           "hess_GB": NT * 3 * ns * oa.level_pitch(K) * 8 / 1.0e9, "calls": {}}
    c = res["calls"]
    tend.compute_transport_tendencies(state, aux, tracers, 0, 0, 1, stream=stream)  # h[1] of the calls
    oa.update_by_tend(h_new, h_old, tend.device_ptr(0)[0], a.dt, nc, oa.level_pitch(K))
    stream.synchronize()
    oa.device_synchronize()
    if a.only_kernels:
        for order in (2, 4):
            set_order(order)
            for _ in range(a.iters):
                call()
            stream.synchronize()
        return
    for rnd in ("1", "2"):
        for order in ORDERS:
            set_order(order)
            before = mono.launch_count()
            t = c[f"order{order}_{rnd}"] = timed(call)
            t["launches_per_call"] = (mono.launch_count() - before) / (a.iters + a.warmup)
            t["algorithmic_GB"] = nc * K * per_level[order] / 1.0e9
            t["TBs"] = t["algorithmic_GB"] / t["ms_median"]
            t["share_of_8TBs"] = t["TBs"] / PEAK_TBS
    res["fit_cell_fraction"] = float(mono.get("FitCell")[:nc].mean())
    keys = [f"order{o}" for o in ORDERS]
    if not a.no_steps:
        st = oa.TimeStepper("Split-Explicit", a.dt, tend, aux, mesh, None, tracers)
        st.attach_barotropic(bm, a.nsub)
        st.attach_monotone_adv(mono)
        for rnd in ("1", "2"):
            for order in ORDERS:
                set_order(order)
                c[f"step_order{order}_{rnd}"] = timed(lambda: st.do_step(state, stream=stream), before=reset, every=5)
        stream.synchronize()
        keys += [f"step_order{o}" for o in ORDERS]
    si = mono.get("ScaleIn")[:, :nc]
    res["scale_in_finite"] = bool(np.isfinite(si).all())
    res["scale_in_limited_fraction"] = float((si < 1.0).mean())
    s = res["summary"] = {}
    for k in keys:
        s[k + "_ms"] = 0.5 * (c[k + "_1"]["ms_median"] + c[k + "_2"]["ms_median"])
        s[k + "_spread_ms"] = abs(c[k + "_1"]["ms_median"] - c[k + "_2"]["ms_median"])
    for o in (3, 4):
        s[f"order{o}_over_order2"] = s[f"order{o}_ms"] / s["order2_ms"]
        if not a.no_steps:
            s[f"step_order{o}_over_step_order2"] = s[f"step_order{o}_ms"] / s["step_order2_ms"]
        s[f"order{o}_TBs"] = nc * K * per_level[o] / 1.0e9 / s[f"order{o}_ms"]
    s["order2_TBs"] = nc * K * per_level[2] / 1.0e9 / s["order2_ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f_:
            f_.write(line + "\n")


if __name__ == "__main__":
    main()
