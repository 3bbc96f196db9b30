"""VertMix on the GPU: N^2, the mixing coefficients and the implicit tracer and velocity solves equal the NumPy
restatement of the contract (tests/vert_mix_reference.py) bit for bit, on NaN-filled outputs and NaN-seeded entries
the solves must not touch; the merged tracer pass equals the existing PCR diffusion solver tracer by tracer; a 2-part
decomposition gives the 1-part values; the null-stream and stream forms agree; no call allocates."""
import numpy as np
import pytest

import omega_amd as oa
from tests import column_reference as CR
from tests import tridiag_reference as TR
from tests import vert_mix_reference as R
from tests.meshes import named_mesh
from tests.vert_fixtures import MIX_NT, MIX_OUT, Mix, same as _same

pytestmark = pytest.mark.gpu

NT = MIX_NT
DT = 1800.0
OUT = MIX_OUT


@pytest.fixture(scope="module", autouse=True)
def _device():
    oa.device_init(0)


CASES = [("hex24x20", 80, "teos10"), ("hex24x20", 60, "linear"), ("fib700_coast_ragged", 37, "teos10"),
         ("fib700_coast_ragged", 80, "linear")]


@pytest.mark.parametrize("mesh,K,eos_kind", CASES)
def test_bvf_and_coefficients_bit_exact(mesh, K, eos_kind):
    x = Mix(named_mesh(mesh), K, eos_kind)
    x.compute()
    n2 = x.expected_bvf()
    _same(x.vm.get("BruntVaisalaFreqSq"), n2, "BruntVaisalaFreqSq")
    assert (n2 > 0).any() and (n2 < 0).any()  # both stable and unstable interfaces
    visc, diff = x.expected_coefficients(x.un, x.ut, n2)
    _same(x.vm.get("VertVisc"), visc, "VertVisc")
    _same(x.vm.get("VertDiff"), diff, "VertDiff")
    # the caller's N^2 instead of the object's own
    other = n2 * 0.5 - 1.0e-5
    x.vm.compute(x.un, x.ut, bvf=other)
    oa.device_synchronize()
    visc, diff = x.expected_coefficients(x.un, x.ut, other)
    _same(x.vm.get("VertVisc"), visc, "VertVisc (caller's N2)")
    _same(x.vm.get("VertDiff"), diff, "VertDiff (caller's N2)")


SWITCHES = [dict(EnableShearMix=False, EnableConvectiveMix=False), dict(EnableShearMix=True, EnableConvectiveMix=False),
            dict(EnableShearMix=False, EnableConvectiveMix=True), dict(EnableShearMix=True, EnableConvectiveMix=True),
            dict(BackgroundViscosity=3.0e-4, BackgroundDiffusivity=2.0e-6, ShearNuZero=0.01, ShearAlpha=7.0,
                 ConvectiveDiffusivity=0.5, ConvectiveTriggerBVF=1.0e-6),
            dict(ShearExponent=3.0), dict(ShearExponent=1.0)]


@pytest.mark.parametrize("cfg", SWITCHES)
def test_switches_and_parameters_bit_exact(cfg):
    x = Mix(named_mesh("fib700_coast_ragged"), 60, "teos10", **cfg)
    x.compute()
    n2 = x.expected_bvf()
    visc, diff = x.expected_coefficients(x.un, x.ut, n2)
    _same(x.vm.get("VertVisc"), visc, "VertVisc")
    _same(x.vm.get("VertDiff"), diff, "VertDiff")


def test_non_integer_exponent_within_4_ulp():
    x = Mix(named_mesh("hex24x20"), 37, "teos10", ShearExponent=1.5)
    x.compute()
    visc, diff = x.expected_coefficients(x.un, x.ut, x.expected_bvf())
    for name, want in (("VertVisc", visc), ("VertDiff", diff)):
        got = x.vm.get(name)
        assert np.all(np.abs(got - want) <= 4 * np.spacing(np.abs(want))), name


def test_tangential_velocity_from_tangential_recon():
    x = Mix(named_mesh("fib700_coast_ragged"), 80, "teos10")
    ut = oa.HorzOperators(x.mesh).tangential_recon(x.un)
    x.compute(ut=ut)
    visc, diff = x.expected_coefficients(x.un, ut, x.expected_bvf())
    _same(x.vm.get("VertVisc"), visc, "VertVisc")
    _same(x.vm.get("VertDiff"), diff, "VertDiff")


@pytest.mark.parametrize("mesh,K,ntracers", [("hex24x20", 80, 1), ("hex24x20", 60, 3), ("fib700_coast_ragged", 37, 6),
                                             ("fib700_coast_ragged", 80, 6), ("hex24x20", 37, 37)])
def test_tracer_solve_bit_exact(mesh, K, ntracers):
    x = Mix(named_mesh(mesh), K, "teos10", ntracers=max(ntracers, 2))
    x.compute()
    t0, t1 = x.seeded_tracers()
    x.vm.apply_tracers(x.state.device_ptr(0, 0), x.tracers.device_ptr(0), ntracers, DT)
    oa.device_synchronize()
    want = R.tracer_mix(x.h, x.vm.get("VertDiff"), t0, ntracers, DT, x.lo, x.hi, x.n_own)
    _same(x.tracers.copy_to_host(0), want, "tracers (level 0)")
    _same(x.tracers.copy_to_host(1), t1, "tracers (level 1)")
    assert not np.array_equal(want[:ntracers], t0[:ntracers], equal_nan=True)  # the solve changed something


@pytest.mark.parametrize("mesh,K", [("hex24x20", 80), ("fib700_coast_ragged", 60), ("fib700_coast_ragged", 37)])
def test_velocity_solve_bit_exact(mesh, K):
    x = Mix(named_mesh(mesh), K, "linear")
    x.compute()
    u0, u1, lo, hi = x.seeded_velocity()
    x.vm.apply_velocity(x.state.device_ptr(0, 0), x.state.device_ptr(1, 0), DT)
    oa.device_synchronize()
    want = R.velocity_mix(x.h, x.vm.get("VertVisc"), u0, DT, x.mesh.get_array("CellsOnEdge"), lo, hi, x.e_own)
    _, got0 = x.state.copy_to_host(0)
    _, got1 = x.state.copy_to_host(1)
    _same(got0, want, "normal velocity (level 0)")
    _same(got1, u1, "normal velocity (level 1)")
    empty = ~((lo[: x.e_own] >= 0) & (lo[: x.e_own] <= hi[: x.e_own]) & (hi[: x.e_own] < K))
    if "coast" in mesh:
        assert empty.any()  # edges with a land neighbour are left alone


@pytest.mark.parametrize("K", [80, 37])
def test_merged_pass_equals_separate_pcr_solves(K):
    x = Mix(named_mesh("hex24x20"), K, "teos10", full=True)
    x.compute()
    t0 = x.tr.copy()
    x.tracers.copy_to_device(t0, 0)
    x.vm.apply_tracers(x.state.device_ptr(0, 0), x.tracers.device_ptr(0), NT, DT)
    oa.device_synchronize()
    got = x.tracers.copy_to_host(0)
    n = x.n_own
    kd = x.vm.get("VertDiff")[:n]
    for t in range(NT):
        g, hh, xx = R.assemble(x.h[:n], kd, t0[t, :n], DT)
        sep = oa.tridiag_diff_solve(g, hh, xx, "pcr")
        assert np.array_equal(got[t, :n], sep), f"tracer {t}"
        assert np.array_equal(sep, TR.pcr_diff(g, hh, xx))


@pytest.mark.parametrize("mesh,K", [("hex24x20", 37), ("fib700_coast_ragged", 80)])
def test_two_part_decomposition_matches_one_part(mesh, K):
    g = named_mesh(mesh)

    def run(nparts, rank):
        x = Mix(g, K, "teos10", nparts=nparts, rank=rank)
        x.compute()
        x.tracers.copy_to_device(x.tr, 0)
        x.vm.apply_tracers(x.state.device_ptr(0, 0), x.tracers.device_ptr(0), NT, DT)
        x.vm.apply_velocity(x.state.device_ptr(0, 0), x.state.device_ptr(1, 0), DT)
        oa.device_synchronize()
        out = {name: x.vm.get(name) for name in OUT}
        out["tracers"] = x.tracers.copy_to_host(0)
        out["u"] = x.state.copy_to_host(0)[1]
        return x, out

    one, ref = run(1, 0)
    cell1 = {int(c): i for i, c in enumerate(one.cid[: one.n_all])}
    edge1 = {int(e): i for i, e in enumerate(one.eid[: one.e_all])}
    for rank in (0, 1):
        x, got = run(2, rank)
        ci = np.array([cell1[int(c)] for c in x.cid[: x.n_own]])
        ei = np.array([edge1[int(e)] for e in x.eid[: x.e_own]])
        for name in OUT:
            _same(got[name][: x.n_own], ref[name][ci], f"{name} rank {rank}")
        _same(got["tracers"][:, : x.n_own], ref["tracers"][:, ci], f"tracers rank {rank}")
        _same(got["u"][: x.e_own], ref["u"][ei], f"u rank {rank}")


def test_stream_and_null_stream_forms_agree():
    g = named_mesh("fib700_coast_ragged")
    a, b = Mix(g, 60, "teos10"), Mix(g, 60, "teos10")
    s = oa.Stream()
    for x, st in ((a, None), (b, s)):
        x.vm.compute_bvf(x.eos, stream=st)
        x.vm.compute(x.un, x.ut, stream=st)
        x.vm.apply_tracers(x.state.device_ptr(0, 0), x.tracers.device_ptr(0), NT, DT, stream=st)
        x.vm.apply_velocity(x.state.device_ptr(0, 0), x.state.device_ptr(1, 0), DT, stream=st)
        if st is not None:
            st.synchronize()
        oa.device_synchronize()
    for name in OUT:
        _same(b.vm.get(name), a.vm.get(name), name)
    _same(b.tracers.copy_to_host(0), a.tracers.copy_to_host(0), "tracers")
    _same(b.state.copy_to_host(0)[1], a.state.copy_to_host(0)[1], "u")


def test_no_allocation_across_compute_and_apply():
    x = Mix(named_mesh("hex24x20"), 80, "teos10")
    ut = oa.DeviceBuffer(np.pad(x.ut, ((0, 0), (0, oa.level_pitch(80) - 80))))
    hp, up = x.state.device_ptr(0, 0), x.state.device_ptr(1, 0)
    s = oa.Stream()
    oa.device_synchronize()
    before = oa.device_resource_count()
    for _ in range(3):
        x.vm.compute_bvf(x.eos, stream=s)
        x.vm.compute(up, ut.ptr, bvf=x.vm.device_ptr("BruntVaisalaFreqSq"), stream=s)
        x.vm.apply_tracers(hp, x.tracers.device_ptr(0), NT, DT, stream=s)
        x.vm.apply_velocity(hp, up, DT, stream=s)
    s.synchronize()
    assert oa.device_resource_count() == before
