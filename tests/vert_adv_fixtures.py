"""Inputs shared by the VertAdv tests (CPU: tests/test_vert_adv.py, GPU: tests/test_vert_adv_gpu.py): the random
thickness tendency and reference thickness on top of tests.vert_fixtures.mix_inputs (layer ranges with land and
KMin > 0), and the condition every such fixture must meet -- a transport of both signs."""
import numpy as np

from tests import vert_adv_reference as VR
from tests.vert_fixtures import mix_inputs

SEED = 7


def adv_inputs(g, K, nt, seed=SEED):
    """mix_inputs plus `d` (the horizontal thickness tendency, m/s, both signs) and `ref` (RefLayerThickness), global
    order"""
    G = mix_inputs(g, K, seed, False, max(nt, 2))
    G["tr"] = G["tr"][:nt]
    rng = np.random.default_rng(seed + 1000)
    n = int(g["nCells"])
    G["d"] = rng.uniform(-1.0e-3, 1.0e-3, (n, K))
    G["ref"] = rng.uniform(1.0, 30.0, (n, K))
    return G


def sign_fractions(wt, lo, hi, n_all):
    """(fraction positive, fraction negative, count) of VerticalTransport on the interior interfaces KMin < K <= KMax"""
    m = VR.interior_mask(lo, hi, n_all, wt.shape[1])
    v = wt[:n_all][m]
    if v.size == 0:
        return 0.0, 0.0, 0
    return float((v > 0.0).mean()), float((v < 0.0).mean()), int(v.size)


def assert_both_signs(wt, lo, hi, n_all):
    """the fixture condition: at least a quarter of the active interior interfaces positive and a quarter negative
    (vacuous where no column has an interior interface, e.g. one level)"""
    pos, neg, cnt = sign_fractions(wt, lo, hi, n_all)
    if cnt:
        assert pos >= 0.25 and neg >= 0.25, f"transport is one-sided: {pos:.2f} positive, {neg:.2f} negative of {cnt}"
    return cnt
