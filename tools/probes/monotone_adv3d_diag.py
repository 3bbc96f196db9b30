"""The 3-D form of MonotoneAdv::addTracerTend (MonotoneAdv.h, attachVertAdv) against the path it replaces, at QU30 size,
timed with device events: the workload of tools/probes/monotone_adv_diag.py (462 400 cells x 80 levels in k-d order,
surface-attached layer ranges, 6 tracers) with a z-star VertAdv of order 2 on the Tendencies, whose own horizontal
tracer advection is off.  Alternated in one process, each as the median of --iters after --warmup, every case timed
twice (the difference of the two medians is its own run-to-run spread):
  parent_1 / _2      compute_transport_tendencies with the VertAdv's tracer term on (its unlimited order-2 flux, a launch
                     of its own) followed by the 2-D add_tracers
  limited3d_1 / _2   the same call with the tracer term off (VertAdv.set_tracer_term) followed by the 3-D add_tracers
  mono2d_only, mono3d_only, vert_tracer_only     the pieces: add_tracers alone either way, VertAdv.add_tracers alone
  step_parent, step_limited3d                    one Split-Explicit step at --nsub either way
Prints one JSON line and writes it to --out.
(--only-kernels: add_tracers alone either way, --iters times each and nothing else: the form to run under
rocprofv3 --kernel-trace, which tells the two launches apart.)

Bytes model per cell-level of a hexagon mesh, 8 B values, the rows of a cell's own column counted once per launch:
  2-D   pass 1 40 + 24 NT, pass 2 32 + 40 NT                       (monotone_adv_diag.py)
  3-D   pass 1 48 + 24 NT, pass 2 40 + 40 NT: VerticalTransport in each, and 8 B per cell per launch for the range
  VertAdv's tracer term: 16 + 24 NT (h, VerticalTransport; per tracer phi, Tend read and written)
  -> the new path moves 16 B more in add_tracers and drops 16 + 24 NT.

   python tools/probes/monotone_adv3d_diag.py [--nx 680] [--levels 80] [--tracers 6] [--nsub 30] [--dt 600] [--iters 50]
          [--warmup 10] [--local-order kd] [--only-kernels] [--out FILE]
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
CASES = ("parent", "limited3d", "mono2d_only", "mono3d_only", "vert_tracer_only")
STEPS = ("step_parent", "step_limited3d")


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
    vc.set("RefLayerThickness", np.full((ns, K), layer))
    bm = oa.BarotropicMode(mesh, vc)
    cfg = oa.default_config(TracerHorzAdvTendencyEnable=0)
    aux = oa.AuxiliaryState(mesh, None, K, NT)
    aux.set_options(cfg.FluxThicknessUpwind, cfg.FluxTracerUpwind, cfg.WindInterpIsotropic)
    tend = oa.Tendencies(mesh, K, NT, cfg)
    va = oa.VertAdv(mesh, vc, 2)
    tend.attach_vert_adv(va)
    mono2 = oa.MonotoneAdv(mesh, K, NT, bool(cfg.FluxThicknessUpwind))
    mono3 = oa.MonotoneAdv(mesh, K, NT, bool(cfg.FluxThicknessUpwind))
    mono3.attach_vert_adv(va)
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

    def transport():
        tend.compute_transport_tendencies(state, aux, tracers, 0, 0, 1, stream=stream)

    def mono2d_only():
        mono2.add_tracers(tend_ptr, h_old, h_new, u_new, tr_ptr, NT, a.dt, stream=stream)

    def mono3d_only():
        mono3.add_tracers(tend_ptr, h_old, h_new, u_new, tr_ptr, NT, a.dt, stream=stream)

    def vert_tracer_only():
        va.add_tracers(tend_ptr, h_old, tr_ptr, NT, stream=stream)

    def parent():
        transport()
        mono2d_only()

    def limited3d():
        transport()
        mono3d_only()

    fns = {"parent": parent, "limited3d": limited3d, "mono2d_only": mono2d_only, "mono3d_only": mono3d_only,
           "vert_tracer_only": vert_tracer_only}
    term_on = {"parent": True, "limited3d": False}
    hyper = bool(cfg.TracerHyperDiffTendencyEnable)
    per_level = {"transport": 40 + (40 if hyper else 16) * NT + 32, "vert_tracer_only": 16 + 24 * NT,
                 "mono2d_only": 72 + 64 * NT, "mono3d_only": 88 + 64 * NT}
    per_level["parent"] = per_level["transport"] + per_level["vert_tracer_only"] + per_level["mono2d_only"]
    per_level["limited3d"] = per_level["transport"] + per_level["mono3d_only"]
    res = {"probe": "monotone_adv3d_diag", "ncells": nc, "nedges": mesh.NEdgesAll, "levels": K, "tracers": NT,
           "nsub": a.nsub, "dt": a.dt, "local_order": a.local_order, "iters": a.iters, "warmup": a.warmup,
           "peak_TBs": PEAK_TBS, "tracer_hyperdiffusion": hyper, "bytes_per_cell_level": per_level, "calls": {}}
    c = res["calls"]
    transport()  # VerticalTransport and h[1] of the pieces
    oa.update_by_tend(h_new, h_old, tend.device_ptr(0)[0], a.dt, nc, oa.level_pitch(K))
    stream.synchronize()
    oa.device_synchronize()
    if a.only_kernels:
        for _ in range(a.iters):
            mono2d_only()
            mono3d_only()
        stream.synchronize()
        return
    for rnd in ("1", "2"):
        for name in CASES:
            va.set_tracer_term(term_on.get(name, True))
            c[f"{name}_{rnd}"] = timed(fns[name])
    for name in CASES:
        for rnd in ("_1", "_2"):
            t = c[name + rnd]
            t["algorithmic_GB"] = nc * K * per_level[name] / 1.0e9
            t["TBs"] = t["algorithmic_GB"] / t["ms_median"]
            t["share_of_8TBs"] = t["TBs"] / PEAK_TBS
    # whole steps (the calm start again every 5 steps, as in monotone_adv_diag.py)
    steppers = {}
    for name, mono, on in (("step_parent", mono2, True), ("step_limited3d", mono3, False)):
        st = oa.TimeStepper("Split-Explicit", a.dt, tend, aux, mesh, None, tracers)
        st.attach_barotropic(bm, a.nsub)
        va.set_tracer_term(on)
        st.attach_monotone_adv(mono)
        steppers[name] = (st, on)
    for rnd in ("1", "2"):
        for name in STEPS:
            st, on = steppers[name]
            va.set_tracer_term(on)
            c[f"{name}_{rnd}"] = timed(lambda: st.do_step(state, stream=stream), before=reset, every=5)
    stream.synchronize()
    si = mono3.get("ScaleIn")[:, :nc]
    res["scale_in_finite"] = bool(np.isfinite(si).all())
    res["scale_in_limited_fraction"] = float((si < 1.0).mean())
    res["max_abs_vertical_transport"] = float(np.abs(va.get("VerticalTransport")[:nc]).max())
    s = res["summary"] = {}
    for k in CASES + STEPS:
        s[k + "_ms"] = 0.5 * (c[k + "_1"]["ms_median"] + c[k + "_2"]["ms_median"])
        s[k + "_spread_ms"] = abs(c[k + "_1"]["ms_median"] - c[k + "_2"]["ms_median"])
    s["limited3d_over_parent"] = s["limited3d_ms"] / s["parent_ms"]
    s["step_limited3d_over_step_parent"] = s["step_limited3d_ms"] / s["step_parent_ms"]
    s["mono3d_over_mono2d"] = s["mono3d_only_ms"] / s["mono2d_only_ms"]
    s["mono3d_only_TBs"] = nc * K * per_level["mono3d_only"] / 1.0e9 / s["mono3d_only_ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f_:
            f_.write(line + "\n")


if __name__ == "__main__":
    main()
