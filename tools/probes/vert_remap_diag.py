"""VertRemap (VertRemap.h) timed with device events at QU30 size: 462 400 cells x 80 levels in k-d order, 6 tracers,
surface-attached layer ranges as in tools/probes/redi_diag.py.  For each order (PCM, PLM, PPM) it times remap -- three
launches -- from a thickness that is the reference thickness perturbed layer-wise by up to +-30 % (restored on the device
before every call, outside the timed span: the first remap leaves h on the target, and a second one from there would
find every layer whole), the orders alternating in one loop.  Then whole Split-Explicit steps without and with the remap
attached (PPM), alternating: the step without it is the step of the code before this class, launch for launch.  Prints
one JSON line and writes it to --out.

Algorithmic bytes of remap (8 B values, every row counted once per launch, a hexagon mesh: 3 edge rows per cell):
  target + tracers  24 B per cell-level (h, Ref read, target written) + 16 B per tracer and cell-level (in place)
  velocity          16 B per cell-level (h, target, each row once) + 16 B per active edge-level (u in place)
  adoption          16 B per cell-level (target read, h written)

   python tools/probes/vert_remap_diag.py [--nx 680] [--levels 80] [--tracers 6] [--nsub 30] [--dt 600] [--iters 20]
          [--warmup 5] [--local-order kd] [--only-kernels] [--no-steps] [--plain-step-only] [--out FILE]
(--only-kernels: just remap at each order, --iters times: the form to run under rocprofv3 --pmc or --kernel-trace.
--plain-step-only: nothing but the step without the remap, and no call into the class: the form that also runs on a
library built from the code before it, OMEGA_AMD_LIB=<that library>, to compare the two builds in alternating processes.)
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
ORDER_NAMES = {1: "pcm", 2: "plm", 3: "ppm"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=680)
    ap.add_argument("--levels", type=int, default=80)
    ap.add_argument("--tracers", type=int, default=6)
    ap.add_argument("--nsub", type=int, default=30)
    ap.add_argument("--dt", type=float, default=600.0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--local-order", default="kd")
    ap.add_argument("--only-kernels", action="store_true")
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--plain-step-only", action="store_true")
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
    P = oa.level_pitch(K)
    state = oa.OceanState(mesh, None, K, 2)
    tracers = oa.Tracers(mesh, None, K, NT, 2)
    h0, u0 = layer + rng.uniform(-1.0e-3, 1.0e-3, (ns, K)), rng.uniform(-1.0e-3, 1.0e-3, (nes, K))
    k = np.arange(K)[None, None, :]
    tr0 = np.concatenate([20.0 - 0.2 * k + rng.uniform(-0.5, 0.5, (1, ns, K)), 34.0 + 0.02 * k + rng.uniform(-0.1, 0.1, (1, ns, K)),
                          rng.uniform(-1.0, 1.0, (NT - 2, ns, K))])

    def reset():
        for lvl in (0, 1):
            state.copy_to_device(h0, u0, lvl)
            tracers.copy_to_device(tr0, lvl)

    reset()
    vc = oa.VertCoord(mesh, K, 1026.0, "Uniform", min_level, max_level, decomp=decomp)
    vc.set("RefLayerThickness", np.full((ns, K), layer))
    remaps = {} if a.plain_step_only else {o: oa.VertRemap(mesh, vc, NT, o) for o in (1, 2, 3)}
    stream = oa.Stream()
    # the scratch level 1 of the state and the tracers is what the calls work on; the perturbed thickness is kept aside
    h1, u1, tr1 = state.device_ptr(0, 1), state.device_ptr(1, 1), tracers.device_ptr(1)
    pad = np.zeros((ns, P))
    pad[:, :K] = layer * rng.uniform(0.7, 1.3, (ns, K))
    h_rough = oa.DeviceBuffer(pad)
    del pad

    def roughen():  # h1 = h_rough, on the device (out = in + 0 * tend)
        oa.update_by_tend(h1, h_rough.ptr, h_rough.ptr, 0.0, ns, P, stream.h.value)

    elo, ehi = vc.get("MinLayerEdgeBot")[: mesh.NEdgesAll], vc.get("MaxLayerEdgeTop")[: mesh.NEdgesAll]
    eactive = int(np.sum(np.where((elo >= 0) & (elo <= ehi), ehi - elo + 1, 0)))
    cl = nc * K
    nbytes = (24 + 16 * NT) * cl + (16 * cl + 16 * eactive) + 16 * cl
    res = {"probe": "vert_remap_diag", "ncells": nc, "nedges": mesh.NEdgesAll, "levels": K, "tracers": NT, "nsub": a.nsub,
           "dt": a.dt, "local_order": a.local_order, "active_edge_levels": eactive, "iters": a.iters, "warmup": a.warmup,
           "peak_TBs": PEAK_TBS, "remap_algorithmic_GB": nbytes / 1.0e9, "calls": {}}

    def remap(order):
        remaps[order].remap(h1, u1, tr1, NT, stream=stream)

    if a.only_kernels:
        for _ in range(a.iters):
            for o in (1, 2, 3):
                roughen()
                remap(o)
        stream.synchronize()
        oa.device_synchronize()
        print(json.dumps(res))
        return

    def timed(fns, before_each=None, before=None, every=0):
        """median / min / max ms of each fn, the fns alternating in one loop; before_each runs ahead of every call,
        outside its timed span"""
        for _ in range(a.warmup):
            for fn in fns:
                if before_each:
                    before_each()
                fn()
        stream.synchronize()
        oa.device_synchronize()
        evs = [[oa.Event() for _ in range(2)] for _ in range(a.iters * len(fns))]
        i = 0
        for r in range(a.iters):
            if before and r % every == 0:
                stream.synchronize()
                oa.device_synchronize()
                before()
            for fn in fns:
                if before_each:
                    before_each()
                evs[i][0].record(stream)
                fn()
                evs[i][1].record(stream)
                i += 1
        stream.synchronize()
        oa.device_synchronize()
        out = []
        for j in range(len(fns)):
            per = np.array([evs[r * len(fns) + j][0].elapsed_ms(evs[r * len(fns) + j][1]) for r in range(a.iters)])
            out.append({"ms_median": float(np.median(per)), "ms_min": float(per.min()), "ms_max": float(per.max()),
                        "ms_p25": float(np.percentile(per, 25)), "ms_p75": float(np.percentile(per, 75))})
        return out

    c = res["calls"]
    keys = []
    if not a.plain_step_only:
        fns = [lambda o=o: remap(o) for o in (1, 2, 3)]
        for rnd in ("1", "2"):  # every case twice: the difference of the two medians is the run's own spread
            for o, t in zip((1, 2, 3), timed(fns, before_each=roughen)):
                t["TBs"] = res["remap_algorithmic_GB"] / t["ms_median"]
                t["share_of_8TBs"] = t["TBs"] / PEAK_TBS
                c[f"remap_{ORDER_NAMES[o]}_{rnd}"] = t
        res["launches_per_remap"] = remaps[3].launch_count() / (2 * (a.iters + a.warmup))
        oa.device_synchronize()
        res["remap_state_finite"] = bool(np.isfinite(tracers.copy_to_host(1)[:, :nc]).all())
        keys = [f"remap_{v}" for v in ORDER_NAMES.values()]

    if not a.no_steps:
        cfg = oa.default_config()
        aux = oa.AuxiliaryState(mesh, None, K, NT)
        aux.set_options(cfg.FluxThicknessUpwind, cfg.FluxTracerUpwind, cfg.WindInterpIsotropic)
        tend = oa.Tendencies(mesh, K, NT, cfg)
        bm = oa.BarotropicMode(mesh, vc)
        steppers = []
        for attached in ((False,) if a.plain_step_only else (False, True)):
            st = oa.TimeStepper("Split-Explicit", a.dt, tend, aux, mesh, None, tracers)
            st.attach_barotropic(bm, a.nsub)
            if attached:
                st.attach_vert_remap(remaps[3])
            steppers.append(st)
        step_fns = [lambda st=st: st.do_step(state, stream=stream) for st in steppers]
        for rnd in ("1", "2"):
            for name, t in zip(("step", "step_vert_remap")[: len(step_fns)], timed(step_fns, before=reset, every=5)):
                c[f"{name}_{rnd}"] = t
        oa.device_synchronize()
        res["step_state_finite"] = bool(np.isfinite(tracers.copy_to_host(0)[:, :nc]).all())
        keys += ["step", "step_vert_remap"][: len(step_fns)]
    s = res["summary"] = {}
    for key in keys:
        s[key + "_ms"] = 0.5 * (c[key + "_1"]["ms_median"] + c[key + "_2"]["ms_median"])
        s[key + "_spread_ms"] = abs(c[key + "_1"]["ms_median"] - c[key + "_2"]["ms_median"])
    for v in ORDER_NAMES.values():
        if f"remap_{v}_ms" in s:
            s[f"remap_{v}_share_of_8TBs"] = res["remap_algorithmic_GB"] / s[f"remap_{v}_ms"] / PEAK_TBS
    res["library"] = os.path.basename(oa.LIB_PATH)
    if not a.no_steps and not a.plain_step_only:
        s["step_vert_remap_minus_step_ms"] = s["step_vert_remap_ms"] - s["step_ms"]
        s["step_vert_remap_over_step"] = s["step_vert_remap_ms"] / s["step_ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
