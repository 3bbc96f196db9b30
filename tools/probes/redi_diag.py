"""Redi (Redi.h) timed with device events at QU30 size: 462 400 cells x 80 levels in k-d order, 2 tracers,
surface-attached layer ranges as in tools/probes/gm_diag.py.  Times the three launches -- the slope, the tracer tendency,
the S.S diffusivity (with a VertDiff to add to) -- and, alternating in the same loop, a yardstick from the code without
this class next to each: GentMcWilliams::computeBolusVelocity without Transport (the same edge-column geometry on the
same cell arrays plus the thickness, two arrays written and a PCR solve) for the slope, the centred
MonotoneAdv::addTracerTend at the same tracer count (two launches) for the tendency, and the displaced column pass.
Then whole Split-Explicit steps with a VertMixStep attached, with and without the closure, alternating.  Prints one JSON
line and writes it to --out.

Algorithmic bytes (8 B values, every row counted once per launch, a hexagon mesh: 3 edge rows per cell):
  slope        24 B per cell-level (SpecVol, SpecVolDisplaced, ZMid) + 8 B per active edge-level (SlopeInterface written)
  tendency     16 B per cell-level (h, ZMid) + 8 B per edge-level (SlopeInterface) + 24 B per tracer and cell-level (phi
               read, Tend read and written)
  diffusivity  8 B per edge-level + 24 B per cell-level (VertDiffusivity written, VertDiff read and written)
  bolus        32 B per cell-level + 16 B per active edge-level (no Transport)

   python tools/probes/redi_diag.py [--nx 680] [--levels 80] [--tracers 2] [--nsub 30] [--dt 600] [--iters 50]
          [--warmup 10] [--local-order kd] [--only-kernels] [--no-steps] [--out FILE]
(--only-kernels: just the three launches, --iters times: the form to run under rocprofv3 --pmc or --kernel-trace.)
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
    ap.add_argument("--tracers", type=int, default=2)
    ap.add_argument("--nsub", type=int, default=30)
    ap.add_argument("--dt", type=float, default=600.0)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--local-order", default="kd")
    ap.add_argument("--only-kernels", action="store_true")
    ap.add_argument("--no-steps", action="store_true")
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
    ns, nes, nc = mesh.NCellsSize, mesh.NEdgesSize, mesh.NCellsAll
    state = oa.OceanState(mesh, None, K, 2)
    tracers = oa.Tracers(mesh, None, K, NT, 2)
    h0, u0 = layer + rng.uniform(-1.0e-3, 1.0e-3, (ns, K)), rng.uniform(-1.0e-3, 1.0e-3, (nes, K))
    # a stable column (T falls, S rises with depth) with noise across the cells: fronts for the closure to act on
    k = np.arange(K)[None, None, :]
    tr0 = np.concatenate([20.0 - 0.2 * k + rng.uniform(-0.5, 0.5, (1, ns, K)), 34.0 + 0.02 * k + rng.uniform(-0.1, 0.1, (1, ns, K)),
                          rng.uniform(-1.0, 1.0, (NT - 2, ns, K))])

    def reset():
        for lvl in (0, 1):
            state.copy_to_device(h0, u0, lvl)
            tracers.copy_to_device(tr0, lvl)

    reset()
    vc = oa.VertCoord(mesh, K, 1026.0, "Uniform", min_level, max_level, decomp=decomp)
    eos = oa.Eos(mesh, K, "teos10")
    redi = oa.Redi(mesh, vc, eos, NT)
    gm = oa.GentMcWilliams(mesh, vc, eos)
    mono = oa.MonotoneAdv(mesh, K, NT)
    stream = oa.Stream()
    hp, h1, u1, trp = state.device_ptr(0, 0), state.device_ptr(0, 1), state.device_ptr(1, 1), tracers.device_ptr(0)
    redi.update_column(hp, trp, NT, stream=stream)
    stream.synchronize()
    P = oa.level_pitch(K)
    tend_buf = oa.DeviceBuffer(np.zeros((NT, ns, P)))
    vert_diff = oa.DeviceBuffer(np.zeros((ns, P)))

    elo, ehi = vc.get("MinLayerEdgeBot")[: mesh.NEdgesAll], vc.get("MaxLayerEdgeTop")[: mesh.NEdgesAll]
    eactive = int(np.sum(np.where((elo >= 0) & (elo <= ehi), ehi - elo + 1, 0)))
    cl = nc * K
    nbytes = {"slope": 24 * cl + 8 * eactive, "tracer_tend": (16 + 24 * NT) * cl + 8 * eactive,
              "vert_diffusivity": 24 * cl + 8 * eactive, "bolus_velocity_no_transport": 32 * cl + 16 * eactive,
              "mono_centred": (72 + 64 * NT) * cl}
    res = {"probe": "redi_diag", "ncells": nc, "nedges": mesh.NEdgesAll, "levels": K, "tracers": NT, "nsub": a.nsub,
           "dt": a.dt, "local_order": a.local_order, "active_edge_levels": eactive, "iters": a.iters, "warmup": a.warmup,
           "peak_TBs": PEAK_TBS, "calls": {}}

    def slope():
        redi.compute_slope(hp, stream=stream)

    def bolus():
        gm.compute(hp, None, stream=stream)

    def tracer_tend():
        redi.add_tracer_tend(tend_buf.ptr, hp, trp, NT, stream=stream)

    def mono_centred():
        mono.add_tracers(tend_buf.ptr, hp, h1, u1, trp, NT, a.dt, stream=stream)

    def vert_diffusivity():
        redi.compute_vert_diffusivity(vert_diff.ptr, stream=stream)

    def column():
        redi.update_column(hp, trp, NT, stream=stream)

    if a.only_kernels:
        for _ in range(a.iters):
            slope()
            tracer_tend()
            vert_diffusivity()
        stream.synchronize()
        print(json.dumps(res))
        return

    def timed(fns, before=None, every=0):
        """median / min / max ms of each fn, the fns alternating in one loop"""
        for _ in range(a.warmup):
            for fn in fns:
                fn()
        stream.synchronize()
        evs = [[oa.Event() for _ in range(2)] for _ in range(a.iters * len(fns))]
        i = 0
        for r in range(a.iters):
            if before and r % every == 0:
                stream.synchronize()
                before()
            for fn in fns:
                evs[i][0].record(stream)
                fn()
                evs[i][1].record(stream)
                i += 1
        stream.synchronize()
        out = []
        for j in range(len(fns)):
            per = np.array([evs[r * len(fns) + j][0].elapsed_ms(evs[r * len(fns) + j][1]) for r in range(a.iters)])
            out.append({"ms_median": float(np.median(per)), "ms_min": float(per.min()), "ms_max": float(per.max()),
                        "ms_p25": float(np.percentile(per, 25)), "ms_p75": float(np.percentile(per, 75))})
        return out

    names = ("slope", "bolus_velocity_no_transport", "tracer_tend", "mono_centred", "vert_diffusivity")
    fns = (slope, bolus, tracer_tend, mono_centred, vert_diffusivity, column)
    c = res["calls"]
    for rnd in ("1", "2"):  # every case twice: the difference of the two medians is the run's own spread
        ts = timed(fns)
        for name, t in zip(names + ("column_pass_displaced",), ts):
            if name in nbytes:
                t["algorithmic_GB"] = nbytes[name] / 1.0e9
                t["TBs"] = t["algorithmic_GB"] / t["ms_median"]
                t["share_of_8TBs"] = t["TBs"] / PEAK_TBS
            c[f"{name}_{rnd}"] = t
    stream.synchronize()
    s_dev = redi.get("SlopeInterface")[: mesh.NEdgesAll]
    res["slope_finite"], res["slope_max_abs"] = bool(np.isfinite(s_dev).all()), float(np.abs(s_dev).max())
    res["slope_clipped_fraction"] = float((np.abs(s_dev) == 0.01).sum() / max(eactive, 1))
    del s_dev
    res["redi_launches_so_far"] = redi.launch_count()  # three per round of the loop: one per call

    keys = list(names) + ["column_pass_displaced"]
    if not a.no_steps:
        cfg = oa.default_config()
        aux = oa.AuxiliaryState(mesh, None, K, NT)
        aux.set_options(cfg.FluxThicknessUpwind, cfg.FluxTracerUpwind, cfg.WindInterpIsotropic)
        tend = oa.Tendencies(mesh, K, NT, cfg)
        bm = oa.BarotropicMode(mesh, vc)
        vm = oa.VertMix(mesh, vc)
        mix_plain, mix_redi = oa.VertMixStep(mesh, vm, vc, eos, NT), oa.VertMixStep(mesh, vm, vc, eos, NT)
        mix_redi.attach_redi(redi)
        steppers = []
        for mix, closure in ((mix_plain, False), (mix_redi, True)):
            st = oa.TimeStepper("Split-Explicit", a.dt, tend, aux, mesh, None, tracers)
            st.attach_barotropic(bm, a.nsub)
            st.attach_vert_mix(mix)
            if closure:
                st.attach_redi(redi)
            steppers.append(st)
        step_fns = [lambda st=st: st.do_step(state, stream=stream) for st in steppers]
        for rnd in ("1", "2"):
            for name, t in zip(("step_vert_mix", "step_vert_mix_redi"), timed(step_fns, before=reset, every=5)):
                c[f"{name}_{rnd}"] = t
        stream.synchronize()
        oa.device_synchronize()
        res["step_state_finite"] = bool(np.isfinite(tracers.copy_to_host(0)[:, :nc]).all())
        keys += ["step_vert_mix", "step_vert_mix_redi"]
    s = res["summary"] = {}
    for key in keys:
        s[key + "_ms"] = 0.5 * (c[key + "_1"]["ms_median"] + c[key + "_2"]["ms_median"])
        s[key + "_spread_ms"] = abs(c[key + "_1"]["ms_median"] - c[key + "_2"]["ms_median"])
    s["slope_over_bolus_velocity"] = s["slope_ms"] / s["bolus_velocity_no_transport_ms"]
    s["tracer_tend_over_mono_centred"] = s["tracer_tend_ms"] / s["mono_centred_ms"]
    if not a.no_steps:
        s["step_redi_over_step_plain"] = s["step_vert_mix_redi_ms"] / s["step_vert_mix_ms"]
        s["step_redi_minus_step_plain_ms"] = s["step_vert_mix_redi_ms"] - s["step_vert_mix_ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
