"""Shared by the VertAdv tests (CPU: tests/test_vert_adv.py, GPU: tests/test_vert_adv_gpu.py,
tests/test_vert_adv_shapes_gpu.py): the random thickness tendency and reference thickness on top of
tests.vert_fixtures.mix_inputs (layer ranges with land and KMin > 0), the condition every such fixture must meet -- a
transport of both signs -- and the rig, host-only or on a device."""
import numpy as np

import omega_amd as oa
from tests import column_reference as CR
from tests import vert_adv_reference as VR
from tests.rank_rig import RankRig
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


class AdvRig(RankRig):
    """One rank's mesh with the inputs of adv_inputs (or `G`) in local order; `full`: every column runs from the top
    to the bottom.  With `device` also VertCoord, OceanState, Tracers and VertAdv (both flux orders) -- with `config`
    AuxiliaryState and Tendencies too."""

    def __init__(self, g, K, nt=2, nparts=1, rank=0, weights="Uniform", config=None, G=None, full=False, device=True):
        super().__init__(g, K, nparts, rank, device=device)
        self.nt = nt
        m = self.mesh
        G = self.G = adv_inputs(g, K, nt) if G is None else G
        if full:
            G["min_level"][:], G["max_level"][:] = 1, K
        self.d, self.ref, self.h = (self.cells(G[k]) for k in ("d", "ref", "h"))
        self.tr, self.u = self.cells(G["tr"]), self.edges(G["un"])
        self.w = CR.movement_weights(weights, K)
        self.layers(G["min_level"], G["max_level"], weights=weights)
        self.coe = m.get_array("CellsOnEdge")
        self.mask = np.ascontiguousarray(m.get_array("EdgeMask")[:, 0])
        if not device:
            return
        self.vc.set("RefLayerThickness", self.seeded(self.ref))  # NaN outside every column's range
        assert np.array_equal(self.vc.get("VertCoordMovementWeights"), self.w)
        self.state = oa.OceanState(m, None, K, 2)
        self.tracers = oa.Tracers(m, None, K, nt, 2)
        self.state.copy_to_device(self.h, self.u, 0)
        self.tracers.copy_to_device(self.tr, 0)
        self.va = {o: oa.VertAdv(m, self.vc, o) for o in (2, 1)}
        for va in self.va.values():
            assert np.all(va.get("VerticalTransport") == 0.0)  # zero at construction
        if config is not None:
            cfg = oa.default_config(**config)
            self.aux = oa.AuxiliaryState(m, None, K, nt)
            self.aux.set_options(cfg.FluxThicknessUpwind, cfg.FluxTracerUpwind, cfg.WindInterpIsotropic)
            self.tend = oa.Tendencies(m, K, nt, cfg)

    def transport(self, d=None, ref=None):
        """the restated transport of `d` (default: the rig's) into zeros"""
        wt = np.zeros((self.n_size, self.K))
        return VR.vertical_transport(self.d if d is None else d, self.ref if ref is None else ref, self.w, self.lo,
                                     self.hi, self.n_all, wt)

    def want_transport(self, d):
        """the restated transport of `d` on the NaN-seeded reference thickness, into NaN"""
        return VR.vertical_transport(d, self.seeded(self.ref), self.w, self.lo, self.hi, self.n_all,
                                     np.full((self.n_size, self.K), np.nan))

    def poison_transport(self, order=2):
        oa.copy_to_device(self.va[order].device_ptr("VerticalTransport"),
                          np.full((self.n_size, oa.level_pitch(self.K)), np.nan))

    def transport_padded(self, order=2):
        return self.raw(self.va[order].device_ptr("VerticalTransport"), (self.n_size, oa.level_pitch(self.K)))
