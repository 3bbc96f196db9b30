"""tools/probes/probe_rig.py and the counter condenser of tools/summarise_profile.py without a device: the timing loop
on a fake stream and event pair driven by a counter, the two-round arithmetic, the rate fields, the condenser on CSVs
written here, and every *_diag.py up to its argument parser."""
import csv
import glob
import importlib
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBES = os.path.join(ROOT, "tools", "probes")
if PROBES not in sys.path:
    sys.path.insert(0, PROBES)
import probe_rig  # noqa: E402
from tools import summarise_profile  # noqa: E402


class FakeDevice:
    """A clock that only the calls move, and a log of everything that happens.  fn j takes 10 (j + 1) + (its call
    count) % 4 ticks; before_each takes 100 and before 1000, so either inside a pair would show in the statistics."""

    def __init__(self, nfn):
        self.t, self.log, self.ncalls = 0.0, [], [0] * nfn
        self.stream = SimpleNamespace(synchronize=lambda: self.log.append("stream_sync"))
        self.fns = [lambda j=j: self.call(j) for j in range(nfn)]

    def call(self, j):
        d = 10.0 * (j + 1) + self.ncalls[j] % 4
        self.ncalls[j] += 1
        self.t += d
        self.log.append(("call", j, d))

    def before_each(self):
        self.t += 100.0
        self.log.append("before_each")

    def before(self):
        self.t += 1000.0
        self.log.append("before")

    def device_synchronize(self):
        self.log.append("device_sync")

    def Event(self):
        dev = self

        class Event:
            def record(self, stream):
                assert stream is dev.stream
                self.t = dev.t
                dev.log.append("record")

            def elapsed_ms(self, other):
                return other.t - self.t
        return Event()


def run(nfn, iters, warmup, **kw):
    dev = FakeDevice(nfn)
    kw = {k: getattr(dev, k) if k.startswith("before") else v for k, v in kw.items()}
    return dev, probe_rig.timed(dev.stream, dev.fns, iters, warmup, device=dev, **kw)


def pairs_of(log):
    """[(index of the first record, fn, duration)] of every record-call-record run in the log"""
    out = []
    for i in range(len(log) - 2):
        if log[i] == "record" and isinstance(log[i + 1], tuple) and log[i + 2] == "record":
            out.append((i, log[i + 1][1], log[i + 1][2]))
    return out


def test_timed_alternates_and_keeps_the_warmup_outside():
    dev, out = run(3, 4, 2)
    log = dev.log
    first = log.index("record")
    assert log[:first] == [("call", j, 10.0 * (j + 1) + r) for r in range(2) for j in range(3)] + ["stream_sync", "device_sync"]
    pairs = pairs_of(log)
    assert [j for _, j, _ in pairs] == [0, 1, 2] * 4                       # four pairs each, alternating
    assert log.count("record") == 2 * 12 and sum(isinstance(x, tuple) for x in log) == 6 + 12   # and no call outside one
    assert log[-2:] == ["stream_sync", "device_sync"] and log.count("device_sync") == 2
    for j in range(3):
        per = np.array([d for _, k, d in pairs if k == j])
        assert len(per) == 4
        want = {"ms_median": np.median(per), "ms_min": per.min(), "ms_max": per.max(), "ms_p25": np.percentile(per, 25),
                "ms_p75": np.percentile(per, 75)}
        assert out[j] == {k: float(v) for k, v in want.items()}


def test_timed_before_each_runs_ahead_of_every_call_outside_its_pair():
    dev, out = run(2, 3, 1, before_each=True)
    log = dev.log
    assert log.count("before_each") == 2 * (1 + 3)
    for i, x in enumerate(log):
        if isinstance(x, tuple):    # a warm-up call directly after it, a timed one after it and the first record
            assert log[i - 1] == "before_each" or (log[i - 1] == "record" and log[i - 2] == "before_each")
    for i, _, _ in pairs_of(log):
        assert log[i + 1] != "before_each" and log[i - 1] == "before_each"
    assert out[0]["ms_max"] < 100.0 and out[1]["ms_max"] < 100.0


@pytest.mark.parametrize("every,rounds", [(0, [0]), (2, [0, 2, 4]), (5, [0]), (1, [0, 1, 2, 3, 4])])
def test_timed_before_runs_at_every_th_round_and_once_when_every_is_0(every, rounds):
    dev, out = run(2, 5, 1, before=True, every=every)
    log = dev.log
    at = [sum(isinstance(x, tuple) for x in log[:i]) for i, x in enumerate(log) if x == "before"]
    assert at == [2 * 1 + 2 * r for r in rounds]                           # timed calls done before it: 2 per round
    for i, x in enumerate(log):
        if x == "before":                                                  # on a drained device, outside every pair
            assert log[i - 2: i] == ["stream_sync", "device_sync"] and log[i + 1] == "record"
    assert out[0]["ms_max"] < 1000.0


def test_timed_successive_spans_run_from_event_to_event():
    dev, out = run(1, 4, 2, successive=True)
    first = dev.log.index("record")
    assert dev.log[first:] == ["record"] + [x for r in range(2, 6) for x in (("call", 0, 10.0 + r % 4), "record")] + \
        ["stream_sync", "device_sync"]
    per = np.array([10.0 + r % 4 for r in range(2, 6)])
    assert out == [{"ms_median": float(np.median(per)), "ms_min": per.min(), "ms_max": per.max(),
                    "ms_p25": float(np.percentile(per, 25)), "ms_p75": float(np.percentile(per, 75))}]


def test_summarise_and_with_rate():
    calls = {"a_1": {"ms_median": 2.0}, "a_2": {"ms_median": 2.5}, "b_1": {"ms_median": 7.0}, "b_2": {"ms_median": 4.0},
             "c": {"ms_median": 1.0}}
    assert probe_rig.summarise(calls, ["a", "b"]) == {"a_ms": 2.25, "a_spread_ms": 0.5, "b_ms": 5.5, "b_spread_ms": 3.0}
    t = {"ms_median": 0.5, "ms_min": 0.4}
    assert probe_rig.with_rate(t, 2.0e9) is t
    assert t == {"ms_median": 0.5, "ms_min": 0.4, "algorithmic_GB": 2.0, "TBs": 4.0, "share_of_8TBs": 0.5}
    assert probe_rig.PEAK_TBS == 8.0
    rounds, kept = iter([[{"n": 1}, {"m": 1}], [{"n": 2}, {"m": 2}]]), {}
    assert probe_rig.twice(kept, ("x", "y"), lambda: next(rounds)) == ["x", "y"]
    assert kept == {"x_1": {"n": 1}, "y_1": {"m": 1}, "x_2": {"n": 2}, "y_2": {"m": 2}}


def test_emit(tmp_path, capsys):
    out = tmp_path / "sub" / "r.json"
    probe_rig.emit({"a": 1, "b": {"c": 2.5}}, str(out))
    line = capsys.readouterr().out
    assert line == '{"a": 1, "b": {"c": 2.5}}\n' and out.read_text() == line
    probe_rig.emit({"a": 1})
    assert capsys.readouterr().out == '{"a": 1}\n'


def write_csv(path, cols, rows):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(cols)
        w.writerows(rows)


def test_condense_kernels(tmp_path, capsys):
    """columns as rocprofv3 writes them; two kernels, betaKernel absent from the write pass"""
    d, tag = str(tmp_path), "t"
    alpha, beta = "void OMEGA::alphaKernel<6>(double*, int)", "OMEGA::betaKernel(double const*)"
    cols = ["Dispatch_Id", "Kernel_Name", "Counter_Name", "Counter_Value"]
    write_csv(f"{d}/{tag}_pmc_fetch/host/1_counter_collection.csv", cols,
              [[1, alpha, "FETCH_SIZE", 100.0], [2, beta, "FETCH_SIZE", 7.0], [3, alpha, "FETCH_SIZE", 300.0], [4, "other", "FETCH_SIZE", 1.0]])
    write_csv(f"{d}/{tag}_pmc_write/host/1_counter_collection.csv", cols,
              [[1, alpha, "WRITE_SIZE", 50.0], [1, alpha, "TCC_HIT_sum", 9.0], [1, alpha, "TCC_MISS_sum", 3.0], [2, alpha, "WRITE_SIZE", 70.0]])
    write_csv(f"{d}/{tag}_trace/host/1_kernel_stats.csv", ["Name", "Calls", "AverageNs"],
              [[alpha, 20, 1500.0], [beta, 20, 900.0], ["other", 1, 1.0]])
    res = summarise_profile.condense_kernels(d, tag, "a note", ["alphaKernel", "betaKernel"])
    printed = json.loads(capsys.readouterr().out)
    with open(f"{d}/{tag}_counters_qu30.json") as f:
        assert json.load(f) == res == printed
    assert list(res) == ["_note", "kernels"] and res["_note"] == "a note" and list(res["kernels"]) == ["alphaKernel", "betaKernel"]
    a, b = res["kernels"]["alphaKernel"], res["kernels"]["betaKernel"]
    assert a["launches_sampled"] == {"FETCH_SIZE": 2, "WRITE_SIZE": 2, "TCC_HIT_sum": 1, "TCC_MISS_sum": 1}
    assert a["counters_mean"] == {"FETCH_SIZE": 200.0, "WRITE_SIZE": 60.0, "TCC_HIT_sum": 9.0, "TCC_MISS_sum": 3.0}
    assert a["fetch_bytes_per_launch_x2"] == 200.0 * 2 * 1024 and a["write_bytes_per_launch"] == 60.0 * 1024
    assert a["hbm_bytes_per_launch"] == 200.0 * 2 * 1024 + 60.0 * 1024
    assert a["kernel_stats"] == [{"Name": alpha, "Calls": "20", "AverageNs": "1500.0"}]       # matched by substring
    assert b["launches_sampled"] == {"FETCH_SIZE": 1} and b["counters_mean"] == {"FETCH_SIZE": 7.0}
    assert not {"fetch_bytes_per_launch_x2", "write_bytes_per_launch", "hbm_bytes_per_launch"} & set(b)
    assert b["kernel_stats"] == [{"Name": beta, "Calls": "20", "AverageNs": "900.0"}]
    assert set(a) == {"launches_sampled", "counters_mean", "fetch_bytes_per_launch_x2", "write_bytes_per_launch",
                      "hbm_bytes_per_launch", "kernel_stats"}
    flat = summarise_profile.condense_kernels(d, tag, "a note", ["alphaKernel"], flat=True)
    assert flat == {"_note": "a note", **a}
    # the reader the bench summary uses is the same one, keyed by the short name
    assert dict(summarise_profile.counters(f"{d}/{tag}_pmc_fetch")["alphaKernel<6>"]) == {"FETCH_SIZE": [100.0, 300.0]}


@pytest.mark.parametrize("script", sorted(os.path.basename(f) for f in glob.glob(os.path.join(PROBES, "*_diag.py"))))
def test_probe_imports_and_parses_its_arguments(script, capsys):
    """without touching a device: a probe left half-converted fails here"""
    mod = importlib.import_module(script[:-3])
    with pytest.raises(SystemExit) as e:
        mod.main(["--help"])
    assert e.value.code == 0
    usage = capsys.readouterr().out
    assert "--iters" in usage and "--warmup" in usage and "--out" in usage
    src = open(os.path.join(PROBES, script)).read()
    assert "def timed" not in src and "PEAK_TBS =" not in src and "json.dumps" not in src
