"""The four batched tridiagonal solvers (TriDiagSolvers.h), timed with device events: QU30 size (462 400 systems x
K = 80, and x K = 60 in level arrays of pitch 64) and the reference's perf sizes (NRow 64 x NBatch 500 .. 10000).
Prints one JSON line (ms per call, algorithmic bytes, share of 8 TB/s) and writes it to --out when given.
Algorithmic bytes per row: 40 for the general form (DL, D, DU, X read, X written), 32 for the diffusion form.

   python tools/probes/tridiag_diag.py [--iters 50] [--warmup 10] [--sizes qu30_k80,...] [--out FILE]
"""
import argparse

import numpy as np
from probe_rig import PEAK_TBS, add_common_args, emit, oa, timed, with_rate

BYTES = {"general": 40, "diffusion": 32}
SOLVERS = [("general", "pcr"), ("diffusion", "pcr"), ("general", "thomas"), ("diffusion", "thomas")]
SIZES = [("qu30_k80", 462400, 80, 80), ("qu30_k60_p64", 462400, 60, 64)] + \
        [(f"ref_{nb}x64", nb, 64, 64) for nb in (500, 1000, 5000, 10000)]


def main(argv=None):
    ap = argparse.ArgumentParser()
    add_common_args(ap, iters=50, warmup=10)
    ap.add_argument("--sizes", default="", help="comma-separated case names (default: all)")
    a = ap.parse_args(argv)
    only = set(filter(None, a.sizes.split(",")))
    oa.device_init(0)
    rng = np.random.default_rng(2026)
    stream = oa.Stream()
    res = {"probe": "tridiag_diag", "iters": a.iters, "peak_TBs": PEAK_TBS, "cases": {}}
    for name, nb, n, pitch in SIZES:
        if only and name not in only:
            continue
        # a diagonally dominant general system and a diffusion system; each solve overwrites X in place, so the
        # timed calls solve ever new right-hand sides (|A^-1| <= 1 general, <= 2 diffusion: no overflow in 60 calls)
        dl = rng.uniform(-1.0, 1.0, (nb, pitch))
        du = rng.uniform(-1.0, 1.0, (nb, pitch))
        d = rng.uniform(3.0, 4.0, (nb, pitch))
        dl[:, 0], du[:, n - 1] = 0.0, 0.0
        g = rng.uniform(0.0, 2.0, (nb, pitch))
        g[:, n - 1] = 0.0
        h = rng.uniform(0.5, 1.5, (nb, pitch))
        x = rng.uniform(-1.0, 1.0, (nb, pitch))
        bufs = {k: oa.DeviceBuffer(v) for k, v in dict(dl=dl, d=d, du=du, g=g, h=h, x=x).items()}
        p = {k: b.ptr for k, b in bufs.items()}
        case = {"nbatch": nb, "nrow": n, "row_pitch": pitch}
        for form, algo in SOLVERS:
            if form == "general":
                def fn():
                    oa.tridiag_solve(p["dl"], p["d"], p["du"], p["x"], algorithm=algo, stream=stream, nbatch=nb,
                                     nrow=n, row_pitch=pitch)
            else:
                def fn():
                    oa.tridiag_diff_solve(p["g"], p["h"], p["x"], algorithm=algo, stream=stream, nbatch=nb, nrow=n,
                                          row_pitch=pitch)
            case[f"{algo}_{form}"] = with_rate(timed(stream, [fn], a.iters, a.warmup, successive=True)[0], nb * n * BYTES[form])
        res["cases"][name] = case
        del bufs
    emit(res, a.out)


if __name__ == "__main__":
    main()
