"""bench.py --gpus N started plainly (no torch.distributed.run around it) launches its own rank processes.
CPU part: without a GPU every rank fails loudly (the product path has no CPU fallback), the parent relays that and exits
non-zero; the parent itself never loads libomega_amd.  The GPU rehearsal is tests/test_00_multirank_gpu.py."""
import ast
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCH_VARS = ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "OMEGA_BENCH_LAUNCHER")


def test_module_level_of_bench_loads_no_native_library():
    """Nothing at module level imports omega_amd / torch / the oracle: argument parsing and the launcher come first."""
    tree = ast.parse(open(os.path.join(ROOT, "bench.py")).read())
    mods = set()
    for node in tree.body:
        if isinstance(node, ast.Import):
            mods.update(a.name.split(".")[0] for a in node.names)
        elif isinstance(node, ast.ImportFrom):
            mods.add((node.module or "").split(".")[0])
    assert not (mods & {"omega_amd", "torch", "oracle"}), mods


def test_plain_invocation_with_two_gpus_starts_two_ranks_and_reports_their_failure():
    import omega_amd as oa
    if oa.device_count() > 0:
        pytest.skip("a GPU is visible: the GPU suite runs the real rehearsal")
    env = {k: v for k, v in os.environ.items() if k not in LAUNCH_VARS}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "small", "--steps", "1",
                        "--warmup", "0", "--no-cpu-baseline"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    err = r.stderr.decode()
    assert r.returncode != 0
    assert r.stdout.decode().strip() == ""                 # no record: nothing was measured
    assert "launch with torch.distributed.run" not in err  # (round 4's answer)
    assert err.count("no HIP device visible") >= 2, err[-2000:]      # both ranks ran and failed loudly
    assert "[bench launcher] rank exit codes" in err


def test_world_size_mismatch_is_refused():
    env = dict({k: v for k, v in os.environ.items() if k not in LAUNCH_VARS}, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--workload", "small"], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE = 2" in r.stderr.decode()


def test_tool_scripts_parse():
    """tools/*.sh are only ever run on the GPU box: at least their syntax is checked here."""
    import glob
    for f in sorted(glob.glob(os.path.join(ROOT, "tools", "*.sh"))):
        r = subprocess.run(["bash", "-n", f], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, (f, r.stderr.decode())


def test_live_traffic_degrades_to_a_reason(monkeypatch):
    """bench.live_traffic (roofline.traffic measured inside the run through two rocprofv3 --pmc child runs) must never
    take the measurement down with it: under a profiler it declines, and where the child runs cannot succeed (no GPU
    here) it returns the reason instead of raising."""
    import bench
    args = bench.parse_args(["--workload", "small"])
    monkeypatch.setenv("ROCPROFILER_TEST_MARK", "1")
    out, why = bench.live_traffic(args)
    assert out is None and "profiler" in why
    monkeypatch.delenv("ROCPROFILER_TEST_MARK")
    import omega_amd as oa
    if oa.device_count() == 0:
        out, why = bench.live_traffic(args)
        assert out is None and isinstance(why, str) and why


def test_dump_outputs_is_refused_for_several_ranks():
    env = {k: v for k, v in os.environ.items() if k not in LAUNCH_VARS}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "small", "--dump-outputs",
                        os.path.join(ROOT, "never_written")], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=120)
    assert r.returncode != 0 and "--gpus 1" in r.stderr.decode()
    assert r.stdout.decode().strip() == "" and not os.path.exists(os.path.join(ROOT, "never_written"))


class _GlobalTend:
    """Stands in for omega_amd.Tendencies in bench.dump_outputs: global [n, K] arrays handed out in a decomposition's
    local row order."""

    def __init__(self, decomp, mesh, h, u, tr):
        self.K, self.NT = h.shape[1], tr.shape[0]
        c = np.asarray(decomp.get_array("CellID")[: mesh.NCellsOwned]) - 1
        e = np.asarray(decomp.get_array("EdgeID")[: mesh.NEdgesOwned]) - 1
        self.arrays = (h[c], u[e], tr[:, c])

    def get(self, which):
        return self.arrays[which]


def _dump(tmp, g, local_order, h, u, tr):
    import bench
    oa = bench.oa
    decomp = oa.Decomp(oa.GlobalMesh(g), 1, 0, 3, cell_task=None, local_order=local_order)
    mesh = oa.HorzMesh(decomp, h.shape[1], host_only=True)
    bench.dump_outputs(str(tmp), g, decomp, mesh, _GlobalTend(decomp, mesh, h, u, tr))
    return {n: np.load(os.path.join(str(tmp), n + ".npy")) for n in ("layer_thickness_tend", "normal_velocity_tend", "tracer_tend")}


def test_dumped_outputs_are_a_fixed_sample_in_global_order(tmp_path):
    """--dump-outputs: float64, rows of a seeded sample of global ids in ascending order, whatever local numbering the
    library chose, and below 64 MB in all for every workload."""
    import bench
    bench.load_library()
    from omega_amd.meshgen import synthetic_state_rows
    g = bench.workload_mesh("small_coast")
    K, NT = 7, 3
    h, u, tr = synthetic_state_rows(g, K, NT, np.arange(g["nCells"]), np.arange(g["nEdges"]))
    a = _dump(tmp_path / "kd", g, "kd", h, u, tr)
    b = _dump(tmp_path / "global", g, "global", h, u, tr)
    for name in a:
        assert a[name].dtype == np.float64 and np.array_equal(a[name], b[name]), name
    n = min(bench.DUMP_ROWS, g["nCells"])
    assert a["layer_thickness_tend"].shape == (n, K) and a["tracer_tend"].shape == (NT, n, K)
    assert a["normal_velocity_tend"].shape == (min(bench.DUMP_ROWS, g["nEdges"]), K)
    rows = [int(np.flatnonzero((h == r).all(axis=1))[0]) for r in a["layer_thickness_tend"][:50]]
    assert rows == sorted(rows) and len(set(rows)) == 50
    assert np.array_equal(a["tracer_tend"], tr[:, [int(np.flatnonzero((h == r).all(axis=1))[0]) for r in a["layer_thickness_tend"]]])
    for wl, (_, _, _, levels, ntr, _) in bench.WORKLOADS.items():
        rows = min(bench.DUMP_ROWS, bench.DUMP_BYTES // (8 * levels * (2 + ntr)))
        assert 0 < rows * 8 * levels * (2 + ntr) <= 64 << 20, wl


@pytest.mark.gpu
def test_plain_run_measures_the_headline_and_dumps_what_it_computed(tmp_path):
    """A plain `bench.py --gpus 1` run: the headline record without the --full parts, and --dump-outputs writes the
    tendencies of the timed path, equal to the CPU oracle's on the global mesh bit for bit."""
    import json
    import bench
    from oracle import oracle as O
    from omega_amd.meshgen import synthetic_state_rows
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "small", "--steps", "3",
                        "--warmup", "1", "--dump-outputs", str(out)], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = r.stdout.decode().strip().splitlines()
    assert len(lines) == 1, lines
    rec = json.loads(lines[0])
    assert rec["metric"] == "tendency_cell_level_updates_per_sec" and rec["unit"] == "cell-level-updates/s"
    assert rec["higher_is_better"] is True and rec["dtype"] == "f64" and rec["steps"] == 3 and rec["warmup"] == 1
    assert rec["ms_per_step"] > 0 and abs(rec["value"] - rec["config"]["cells"] * rec["config"]["levels"] / (rec["ms_per_step"] * 1e-3)) < 1e-6 * rec["value"]
    assert rec["config"]["full"] is False
    assert rec["sypd"] is None and rec["roofline"] is None and rec["cpu_baseline"] is None and rec["realistic"] is None
    bench.load_library()
    g = bench.workload_mesh("small")
    K, NT = bench.WORKLOADS["small"][3:5]
    h, u, tr = synthetic_state_rows(g, K, NT, np.arange(g["nCells"]), np.arange(g["nEdges"]))
    if "boundaryEdge" in g:
        u[np.asarray(g["boundaryEdge"]) != 0] = 0.0
    pad = lambda a: np.concatenate([a, np.zeros(a.shape[:-2] + (1, K))], axis=-2)   # noqa: E731  (the zero sentinel row)
    hT, uT, trT = O.Oracle(O.Mesh.single_rank(g, K), NT).compute_all_tendencies(pad(h), pad(u), pad(tr))
    ref = _dump(tmp_path / "oracle", g, "global", hT[: g["nCells"]], uT[: g["nEdges"]], trT[:, : g["nCells"]])
    for name, want in ref.items():
        got = np.load(os.path.join(str(out), name + ".npy"))
        assert got.dtype == np.float64 and np.isfinite(got).all() and np.abs(got).max() > 0, name
        assert np.array_equal(got, want), (name, float(np.abs(got - want).max()))
