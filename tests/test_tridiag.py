"""The NumPy restatement of the tridiagonal solvers (tests/tridiag_reference.py) against the reference's known answers
(components/omega/test/base/TriDiagSolversTest.cpp): the correctness sweep, the manufactured-solution convergence
rate and the stability test.  CPU only; tests/test_tridiag_gpu.py holds the library to this restatement bit for bit."""
import math

import numpy as np
import pytest

from tests import tridiag_reference as R

NBATCH = (1, 2, 4, 5, 11, 33, 102)
NROW = (3, 4, 5, 6, 11, 17, 64, 100)


@pytest.mark.parametrize("algo", ["pcr", "thomas"])
def test_correctness_sweep(algo):
    """TriDiagSolversTest.cpp:15-119,476-497: max |x - solve(A x)| <= 1e-12, both forms"""
    for nb in NBATCH:
        for n in NROW:
            dl, d, du, x, ax = R.correctness_system(nb, n)
            assert np.max(np.abs(R.GENERAL[algo](dl, d, du, ax) - x)) <= 1e-12, (nb, n)
            g, h, x, ax = R.diffusion_correctness_system(nb, n)
            assert np.max(np.abs(R.DIFFUSION[algo](g, h, ax) - x)) <= 1e-12, (nb, n)


def test_inputs_are_not_modified():
    dl, d, du, x, ax = R.correctness_system(3, 17)
    g, h, _, _ = R.diffusion_correctness_system(3, 17)
    keep = [a.copy() for a in (dl, d, du, ax, g, h)]
    for f in R.GENERAL.values():
        f(dl, d, du, ax)
    for f in R.DIFFUSION.values():
        f(g, h, ax)
    for a, b in zip((dl, d, du, ax, g, h), keep):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 60, 63, 64, 65, 80, 129])
def test_pcr_solves_random_diagonally_dominant_systems(n):
    """PCR's level loop, index clamps and final 2x2 / 1x1 step give the solution at every size, NRow = 1 included
    (the 1x1 solve the contract defines there)"""
    rng = np.random.default_rng(n)
    nb = 7
    dl, du = rng.uniform(-1, 1, (nb, n)), rng.uniform(-1, 1, (nb, n))
    dl[:, 0], du[:, -1] = 0, 0
    d = 3 + rng.uniform(0, 1, (nb, n))
    x = rng.uniform(-1, 1, (nb, n))
    a = np.zeros((nb, n, n))
    for i in range(nb):
        a[i] = np.diag(d[i]) + np.diag(dl[i, 1:], -1) + np.diag(du[i, :-1], 1)
    want = np.linalg.solve(a, x[..., None])[..., 0]
    assert np.allclose(R.pcr(dl, d, du, x), want, rtol=0, atol=1e-13)
    assert np.allclose(R.thomas(dl, d, du, x), want, rtol=0, atol=1e-13)
    g, h = rng.uniform(0, 2, (nb, n)), rng.uniform(0.5, 1.5, (nb, n))
    g[:, -1] = 0
    gm = np.concatenate([np.zeros((nb, 1)), g[:, :-1]], axis=1)
    for i in range(nb):
        a[i] = np.diag(h[i] + gm[i] + g[i]) - np.diag(g[i, :-1], -1) - np.diag(g[i, :-1], 1)
    want = np.linalg.solve(a, x[..., None])[..., 0]
    assert np.allclose(R.pcr_diff(g, h, x), want, rtol=0, atol=1e-13)
    assert np.allclose(R.thomas_diff(g, h, x), want, rtol=0, atol=1e-13)


def test_pcr_levels():
    assert [R.pcr_levels(n) for n in (2, 3, 4, 5, 60, 64, 65, 80, 1024)] == [1, 2, 2, 3, 6, 6, 7, 7, 10]
    for n in range(2, 1025):
        assert R.pcr_levels(n) == math.ceil(math.log2(n))


@pytest.mark.parametrize("algo", ["pcr", "thomas"])
def test_diffusion_manufactured_solution(algo):
    """TriDiagSolversTest.cpp:122-268: rate 2 +- 0.1 and L2(200) <= 2e-5"""
    e100 = R.diff_manufactured(100, R.DIFFUSION[algo])
    e200 = R.diff_manufactured(200, R.DIFFUSION[algo])
    rate = math.log2(e100 / e200)
    assert abs(rate - 2) <= 0.1, rate
    assert e200 <= 2e-5, e200


@pytest.mark.parametrize("algo", ["pcr", "thomas"])
def test_diffusion_stability(algo):
    """TriDiagSolversTest.cpp:270-474: at 1e2 the general and diffusion solvers agree (isApprox RTol 1e-3); at 1e14
    the general solver gives NaN and the diffusion solver stays finite"""
    gen, dif = R.GENERAL[algo], R.DIFFUSION[algo]
    small_g = R.diffusion_stability(True, 1e2, gen)
    small_d = R.diffusion_stability(False, 1e2, dif)
    assert R.is_approx(small_g, small_d, 1e-3), (small_g, small_d)
    assert math.isnan(R.diffusion_stability(True, 1e14, gen))
    assert not math.isnan(R.diffusion_stability(False, 1e14, dif))
