"""MonotoneAdv::addTracerTend (MonotoneAdv.h) at QU30 size, timed with device events, in one of three forms (--form):
the workload of tools/probes/transport_diag.py (462 400 cells x 80 levels in k-d order, 6 tracers).  The cases of a form
are alternated in one process, each as the median of --iters after --warmup, every case timed twice (the difference of
the two medians is its own run-to-run spread): first the calls, then whole Split-Explicit steps at --nsub.  Prints one
JSON line ("probe" names the form) and writes it to --out.

--form 2d ("monotone_adv_diag"; surface-attached layer ranges): the call against the Tendencies' own centred term
  transport_centred_1 / _2     compute_transport_tendencies with the Tendencies' own centred advection term (the path
                               without this class)
  transport_no_adv_mono_1 / _2 the same call with TracerHorzAdvTendencyEnable off, followed by add_tracers
  mono_only_1 / _2             add_tracers alone (two launches)
  step_plain_1 / _2            one Split-Explicit step, nothing attached
  step_mono_1 / _2             one Split-Explicit step with the MonotoneAdv attached (and the advection term off)

--form 3d ("monotone_adv3d_diag"; the same ranges, a z-star VertAdv of order 2 on the Tendencies, whose own horizontal
tracer advection is off): the 3-D form (attachVertAdv) against the path it replaces
  parent_1 / _2      compute_transport_tendencies with the VertAdv's tracer term on (its unlimited order-2 flux, a launch
                     of its own) followed by the 2-D add_tracers
  limited3d_1 / _2   the same call with the tracer term off (VertAdv.set_tracer_term) followed by the 3-D add_tracers
  mono2d_only, mono3d_only, vert_tracer_only     the pieces: add_tracers alone either way, VertAdv.add_tracers alone
  step_parent, step_limited3d                    one Split-Explicit step either way

--form ho ("monotone_adv_ho_diag"; full columns): the high-order horizontal flux (setHorzOrder) against the centred
form, one MonotoneAdv object switched between the orders, so that order 2 is the parent's path in the same binary
  order2_1 / _2, order3_1 / _2, order4_1 / _2                add_tracers alone at each order (2, 3 and 3 launches)
  step_order2_1 / _2, step_order3_.., step_order4_..         one attached Split-Explicit step at each order

--only-kernels (3d, ho): add_tracers alone -- either way, or at orders 2 and 4 -- --iters times each and nothing else:
the form to run under rocprofv3 --kernel-trace, which tells the launches apart.  --no-steps (ho): the calls alone.

Bytes model per cell-level of a hexagon mesh (3 edge rows per cell), 8 B values, every row counted once per launch:
  2-D     pass 1 reads hOld, hNew, 3 u: 40; per tracer reads phi, writes ScaleIn and ScaleOut: 24
          pass 2 reads hOld, 3 u: 32; per tracer reads phi, ScaleIn, ScaleOut, reads and writes Tend: 40
          -> 72 + 64 NT for the call; the transport call it follows is 40 + 40 NT with the hyperdiffusion term on
             (tools/probes/transport_diag.py), with or without its advection term.
  3-D     pass 1 48 + 24 NT, pass 2 40 + 40 NT: VerticalTransport in each, and 8 B per cell per launch for the range
          VertAdv's tracer term: 16 + 24 NT (h, VerticalTransport; per tracer phi, Tend read and written)
          -> the new path moves 16 B more in add_tracers and drops 16 + 24 NT.
  order 3, 4   pass 0 32 NT, pass 1 40 + 48 NT, pass 2 32 + 64 NT: 72 + 144 NT.  Hess is NT*3 rows per cell: 5.3 GB at
          this size with 6 tracers.

   python tools/probes/monotone_adv_diag.py [--form 2d|3d|ho] [--nx 680] [--levels 80] [--tracers 6] [--nsub 30]
          [--dt 600] [--iters 50] [--warmup 10] [--local-order kd] [--only-kernels] [--no-steps] [--out FILE]
"""
import argparse
from types import SimpleNamespace

import numpy as np
from probe_rig import PEAK_TBS, Qu30Rig, add_common_args, emit, oa, summarise, with_rate


def workload(a, ragged, ref_thickness, **config):
    """the rig and the Tendencies (of default_config(**config)) every form times on"""
    w = Qu30Rig(a, bottom="layers", ragged=ragged, ref_thickness=ref_thickness)
    w.bm = oa.BarotropicMode(w.mesh, w.vc)
    w.cfg = oa.default_config(**config)
    w.aux, w.tend = w.tendencies(w.cfg)
    w.hyper = bool(w.cfg.TracerHyperDiffTendencyEnable)
    w.stream  # (made here, after the Tendencies)
    w.h_old, w.h_new, w.u_new = w.state.device_ptr(0, 0), w.state.device_ptr(0, 1), w.state.device_ptr(1, 1)
    w.tr_ptr, w.tend_ptr = w.tracers.device_ptr(0), w.tend.device_ptr(2)[0]
    return w


def new_mono(w):
    return oa.MonotoneAdv(w.mesh, w.K, w.NT, bool(w.cfg.FluxThicknessUpwind))


def add_tracers(w, mono, tend_ptr):
    mono.add_tracers(tend_ptr, w.h_old, w.h_new, w.u_new, w.tr_ptr, w.NT, w.a.dt, stream=w.stream)


def transport(w, tend):
    tend.compute_transport_tendencies(w.state, w.aux, w.tracers, 0, 0, 1, stream=w.stream)


def stepper(w, tend, mono=None):
    st = oa.TimeStepper("Split-Explicit", w.a.dt, tend, w.aux, w.mesh, None, w.tracers)
    st.attach_barotropic(w.bm, w.a.nsub)
    if mono is not None:
        st.attach_monotone_adv(mono)
    return st


def take_h_new(w):
    """h[1] of the calls (and VerticalTransport, with a VertAdv): one transport call and its thickness update"""
    transport(w, w.tend)
    oa.update_by_tend(w.h_new, w.h_old, w.tend.device_ptr(0)[0], w.a.dt, w.nc, oa.level_pitch(w.K))
    w.stream.synchronize()
    oa.device_synchronize()


# A form gives: probe, w, header (its entries of the record before "calls"), mono (whose ScaleIn is reported),
# calls [(name, fn, bytes per cell-level, setup or None)], steps() -> [(name, stepper, setup or None)] (built after the
# calls are timed), derive(summary), and optionally prepare(), only_kernels(), extras(record).  A setup runs
# before its case is timed and may return a function that adds to the case's entry afterwards.

def form_2d(a):
    w = workload(a, ragged=True, ref_thickness=False)
    NT = w.NT
    tend_no_adv = oa.Tendencies(w.mesh, w.K, NT, oa.default_config(TracerHorzAdvTendencyEnable=0))
    mono = new_mono(w)
    per = {"mono": 72 + 64 * NT, "transport": 40 + (40 if w.hyper else 16) * NT}

    def mono_only():  # (the address is looked up inside the timed call: so was r18 recorded)
        add_tracers(w, mono, tend_no_adv.device_ptr(2)[0])

    def no_adv_mono():
        transport(w, tend_no_adv)
        mono_only()

    def derive(s):
        s["limited_over_centred_transport"] = s["transport_no_adv_mono_ms"] / s["transport_centred_ms"]
        s["step_mono_over_step_plain"] = s["step_mono_ms"] / s["step_plain_ms"]
        s["mono_only_TBs"] = w.nc * w.K * per["mono"] / 1.0e9 / s["mono_only_ms"]

    return SimpleNamespace(
        probe="monotone_adv_diag", w=w, mono=mono, derive=derive,
        header={"tracer_hyperdiffusion": w.hyper, "bytes_per_cell_level": per},
        calls=[("transport_centred", lambda: transport(w, w.tend), per["transport"], None),
               ("transport_no_adv_mono", no_adv_mono, per["transport"] + per["mono"], None),
               ("mono_only", mono_only, per["mono"], None)],
        steps=lambda: [("step_plain", stepper(w, w.tend), None), ("step_mono", stepper(w, tend_no_adv, mono), None)])


def form_3d(a):
    w = workload(a, ragged=True, ref_thickness=True, TracerHorzAdvTendencyEnable=0)
    NT = w.NT
    va = oa.VertAdv(w.mesh, w.vc, 2)
    w.tend.attach_vert_adv(va)
    mono2, mono3 = new_mono(w), new_mono(w)
    mono3.attach_vert_adv(va)
    per = {"transport": 40 + (40 if w.hyper else 16) * NT + 32, "vert_tracer_only": 16 + 24 * NT,
           "mono2d_only": 72 + 64 * NT, "mono3d_only": 88 + 64 * NT}
    per["parent"] = per["transport"] + per["vert_tracer_only"] + per["mono2d_only"]
    per["limited3d"] = per["transport"] + per["mono3d_only"]

    def mono2d_only():
        add_tracers(w, mono2, w.tend_ptr)

    def mono3d_only():
        add_tracers(w, mono3, w.tend_ptr)

    def vert_tracer_only():
        va.add_tracers(w.tend_ptr, w.h_old, w.tr_ptr, NT, stream=w.stream)

    def parent():
        transport(w, w.tend)
        mono2d_only()

    def limited3d():
        transport(w, w.tend)
        mono3d_only()

    def term(on):
        return lambda: va.set_tracer_term(on)

    def steps():
        out = []
        for name, mono, on in (("step_parent", mono2, True), ("step_limited3d", mono3, False)):
            va.set_tracer_term(on)
            out.append((name, stepper(w, w.tend, mono), term(on)))
        return out

    def only_kernels():
        for _ in range(a.iters):
            mono2d_only()
            mono3d_only()

    def extras(res):
        res["max_abs_vertical_transport"] = float(np.abs(va.get("VerticalTransport")[: w.nc]).max())

    def derive(s):
        s["limited3d_over_parent"] = s["limited3d_ms"] / s["parent_ms"]
        s["step_limited3d_over_step_parent"] = s["step_limited3d_ms"] / s["step_parent_ms"]
        s["mono3d_over_mono2d"] = s["mono3d_only_ms"] / s["mono2d_only_ms"]
        s["mono3d_only_TBs"] = w.nc * w.K * per["mono3d_only"] / 1.0e9 / s["mono3d_only_ms"]

    return SimpleNamespace(
        probe="monotone_adv3d_diag", w=w, mono=mono3, derive=derive, steps=steps, prepare=lambda: take_h_new(w),
        only_kernels=only_kernels, extras=extras,
        header={"tracer_hyperdiffusion": w.hyper, "bytes_per_cell_level": per},
        calls=[("parent", parent, per["parent"], term(True)), ("limited3d", limited3d, per["limited3d"], term(False)),
               ("mono2d_only", mono2d_only, per["mono2d_only"], term(True)),
               ("mono3d_only", mono3d_only, per["mono3d_only"], term(True)),
               ("vert_tracer_only", vert_tracer_only, per["vert_tracer_only"], term(True))])


def form_ho(a):
    w = workload(a, ragged=False, ref_thickness=True, TracerHorzAdvTendencyEnable=0)
    NT, orders = w.NT, (2, 3, 4)
    mono = new_mono(w)
    geo = dict(x_period=float(w.g["x_period"]), y_period=float(w.g["y_period"]))
    per = {2: 72 + 64 * NT, 3: 72 + 144 * NT, 4: 72 + 144 * NT}

    def set_order(order):
        mono.set_horz_order(order, 0.25, **geo)

    def call():
        add_tracers(w, mono, w.tend_ptr)

    def counted(order):
        def setup():
            set_order(order)
            before = mono.launch_count()
            return lambda t: t.update(launches_per_call=(mono.launch_count() - before) / (a.iters + a.warmup))
        return setup

    def steps():
        st = stepper(w, w.tend, mono)
        return [(f"step_order{o}", st, lambda o=o: set_order(o)) for o in orders]

    def only_kernels():
        for order in (2, 4):
            set_order(order)
            for _ in range(a.iters):
                call()
            w.stream.synchronize()

    def extras(res):
        res["fit_cell_fraction"] = float(mono.get("FitCell")[: w.nc].mean())

    def derive(s):
        for o in (3, 4):
            s[f"order{o}_over_order2"] = s[f"order{o}_ms"] / s["order2_ms"]
            if not a.no_steps:
                s[f"step_order{o}_over_step_order2"] = s[f"step_order{o}_ms"] / s["step_order2_ms"]
        for o in orders:
            s[f"order{o}_TBs"] = w.nc * w.K * per[o] / 1.0e9 / s[f"order{o}_ms"]

    return SimpleNamespace(
        probe="monotone_adv_ho_diag", w=w, mono=mono, derive=derive, steps=steps, prepare=lambda: take_h_new(w),
        only_kernels=only_kernels, extras=extras,
        header={"bytes_per_cell_level": {f"order{o}": b for o, b in per.items()},
                "hess_GB": NT * 3 * w.ns * oa.level_pitch(w.K) * 8 / 1.0e9},
        calls=[(f"order{o}", call, per[o], counted(o)) for o in orders])


FORMS = {"2d": form_2d, "3d": form_3d, "ho": form_ho}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--form", choices=tuple(FORMS), default="2d")
    add_common_args(ap, only_kernels=True, nx=680, levels=80, tracers=6, nsub=30, dt=600.0, iters=50, warmup=10, local_order="kd")
    ap.add_argument("--no-steps", action="store_true", help="the calls alone: no Split-Explicit step is timed")
    a = ap.parse_args(argv)
    if (a.only_kernels and a.form == "2d") or (a.no_steps and a.form != "ho"):
        ap.error(f"--form {a.form} has no such mode")
    form = FORMS[a.form](a)
    w = form.w
    stream, nc, K = w.stream, w.nc, w.K

    res = {"probe": form.probe, "ncells": nc, "nedges": w.mesh.NEdgesAll, "levels": K, "tracers": w.NT, "nsub": a.nsub,
           "dt": a.dt, "local_order": a.local_order, "iters": a.iters, "warmup": a.warmup, "peak_TBs": PEAK_TBS,
           **form.header, "calls": {}}
    c = res["calls"]
    if hasattr(form, "prepare"):
        form.prepare()
    if a.only_kernels:
        form.only_kernels()
        stream.synchronize()
        return

    def rounds(cases, time_one):
        for rnd in ("1", "2"):
            for name, what, nbytes, setup in cases:
                finish = setup() if setup else None
                t = c[f"{name}_{rnd}"] = time_one(what)
                if finish:
                    finish(t)
                if nbytes:
                    with_rate(t, nc * K * nbytes)
        return [name for name, *_ in cases]

    keys = rounds(form.calls, lambda fn: w.time([fn])[0])
    if not a.no_steps:
        # whole steps (the calm start again every 5 steps, as in transport_diag.py)
        keys += rounds([(name, st, 0, setup) for name, st, setup in form.steps()],
                       lambda st: w.time([lambda: st.do_step(w.state, stream=stream)], before=w.reset, every=5)[0])
        stream.synchronize()
    si = form.mono.get("ScaleIn")[:, :nc]
    res["scale_in_finite"] = bool(np.isfinite(si).all())
    res["scale_in_limited_fraction"] = float((si < 1.0).mean())
    if hasattr(form, "extras"):
        form.extras(res)
    s = res["summary"] = summarise(c, keys)
    form.derive(s)
    emit(res, a.out)


if __name__ == "__main__":
    main()
