"""The inputs and the rig of the Kpp tests: columns with a mixed layer drawn per column on the layer ranges of
tests.vert_fixtures.mix_inputs (land, KMin > 0, single layers), in local order, with the restatement
(tests/kpp_reference.py) evaluated on them.  The rig works without a device (host-only mesh: the restatement alone) and
with one (VertCoord, VertMix and Kpp on the same inputs)."""
import numpy as np

import omega_amd as oa
from tests import kpp_reference as KR
from tests.rank_rig import RankRig, raw
from tests.vert_fixtures import level_pitch, mix_inputs

NT = 3
OUT2 = ("BulkRichardson", "NonLocalShape")
VALUES = ("BoundaryLayerDepth", "BulkRichardson", "NonLocalShape", "VertDiff", "VertVisc")


def kpp_inputs(g, K, seed):
    """Global inputs: the layer ranges and tracers of mix_inputs; h in 2 .. 12 m and the heights that follow from it;
    N2 in [-2e-9, 1e-8] down to a level drawn per column and in [1e-6, 6e-5] below it; edge velocities whose
    differences reach 0.2 m/s; us in [0, 0.02] with every 9th cell exactly 0; Bf in [-2e-7, 1e-7] with every 11th cell
    exactly 0; seeded coefficients and a surface flux for every tracer"""
    G = mix_inputs(g, K, seed, nt=NT)
    n, ne = int(g["nCells"]), int(g["nEdges"])
    rng = np.random.default_rng(seed + 1000)
    h = rng.uniform(2.0, 12.0, (n, K))
    zint = rng.uniform(-0.5, 0.5, (n, 1)) - np.concatenate([np.zeros((n, 1)), np.cumsum(h, axis=1)], axis=1)
    lo, hi = G["min_level"].astype(np.int64) - 1, G["max_level"].astype(np.int64) - 1
    base = lo + rng.integers(0, K + 1, n) % (np.maximum(hi - lo + 1, 1) + 1)  # lo .. hi+1
    k = np.arange(K)[None, :]
    n2 = np.where(k <= base[:, None], rng.uniform(-2.0e-9, 1.0e-8, (n, K)), rng.uniform(1.0e-6, 6.0e-5, (n, K)))
    n2[k == lo[:, None]] = 0.0  # as VertMix leaves the top interface
    us, bf = rng.uniform(0.0, 0.02, n), rng.uniform(-2.0e-7, 1.0e-7, n)
    us[::9], bf[::11] = 0.0, 0.0
    G.update(h=h, zint=zint, zmid=0.5 * (zint[:, :-1] + zint[:, 1:]), n2=n2,
             un=rng.uniform(-0.1, 0.1, (ne, K)), ut=rng.uniform(-0.1, 0.1, (ne, K)), us=us, bf=bf,
             vd=rng.uniform(1.0e-5, 1.0e-2, (n, K)), vv=rng.uniform(1.0e-4, 1.0e-2, (n, K)),
             flux=rng.uniform(-1.0e-4, 1.0e-4, (NT, n)))
    return G


class KppRig(RankRig):
    """One rank's inputs in local order -- the cell arrays NaN outside what the contract reads (ZMid and N2 outside
    KMin .. KMax, ZInterface outside KMin .. KMax+1, the seeded VertDiff / VertVisc outside the interfaces) -- and, with
    a device, a VertCoord, a VertMix and a Kpp on them."""

    def __init__(self, g, K, seed=7, device=True, vmix_cfg=None, nparts=1, rank=0, **cfg):
        super().__init__(g, K, nparts, rank, device=device)
        self.P = level_pitch(K)
        G = self.G = kpp_inputs(g, K, seed)
        self.layers(G["min_level"], G["max_level"])
        self.cfg = KR.config(**cfg)
        self.h, self.tr = self.cells(G["h"], np.nan), self.cells(G["tr"], np.nan)
        self.un, self.ut = self.edges(G["un"]), self.edges(G["ut"])
        self.us, self.bf = self.cells(G["us"]), self.cells(G["bf"])
        self.flux = self.cells(G["flux"].T).T.copy()
        self.n2, self.zmid = self.seeded(self.cells(G["n2"])), self.seeded(self.cells(G["zmid"]))
        zi = self.cells(G["zint"])
        self.zint = np.full(zi.shape, np.nan)
        below = np.zeros((self.n_size, K + 1), bool)
        below[:, :K] |= self.active
        below[:, 1:] |= self.active
        self.zint[below] = zi[below]
        self.faces = self.active.copy()
        self.faces[np.arange(self.n_size), np.clip(self.lo, 0, K - 1)] = False  # KMin < K <= KMax
        self.vd = np.where(self.faces, self.cells(G["vd"]), np.nan)
        self.vv = np.where(self.faces, self.cells(G["vv"]), np.nan)
        m = self.mesh
        self.tables = (m.get_array("NEdgesOnCell"), m.get_array("EdgesOnCell"), m.get_array("DcEdge"),
                       m.get_array("DvEdge"), m.get_array("AreaCell"))
        self.bg_visc, self.bg_diff = 1.0e-4, 1.0e-5  # VertMixConfig's defaults
        if vmix_cfg:
            self.bg_visc = vmix_cfg.get("BackgroundViscosity", self.bg_visc)
            self.bg_diff = vmix_cfg.get("BackgroundDiffusivity", self.bg_diff)
        self.consts = KR.constants(self.cfg)
        if device:
            self.vm = oa.VertMix(m, self.vc, **(vmix_cfg or {}))
            self.kpp = oa.Kpp(m, self.vc, self.vm, **cfg)
            self.kpp.set("FrictionVelocity", self.us)
            self.kpp.set("SurfaceBuoyancyFlux", self.bf)
            # the restatement takes the two constants as the library formed them: NonLocalCoeff holds a cbrt, and the
            # host's and NumPy's need not round alike
            vt, nl = self.kpp.constants()
            assert vt == self.consts[0] and abs(nl - self.consts[1]) <= 4.0 * np.spacing(nl)
            self.consts = (vt, nl)

    def expected(self, **over):
        """the restatement on the rig's inputs (any of them replaced by keyword)"""
        a = dict(un=self.un, ut=self.ut, n2=self.n2, zmid=self.zmid, zint=self.zint, vd=self.vd, vv=self.vv, us=self.us,
                 bf=self.bf)
        a.update(over)
        return KR.compute(a["un"], a["ut"], a["n2"], a["zmid"], a["zint"], a["vd"], a["vv"], a["us"], a["bf"], self.lo,
                          self.hi, self.n_all, *self.tables, self.bg_visc, self.bg_diff, *self.consts, self.cfg)

    # ---- with a device
    def poison(self):
        """the four outputs NaN (the index: a pattern no column has), padding and sentinel row included"""
        k = self.kpp
        for name in OUT2:
            oa.copy_to_device(k.device_ptr(name), np.full((self.n_size, self.P), np.nan))
        k.set("BoundaryLayerDepth", np.full(self.n_size, np.nan))
        k.set("BoundaryLayerIndex", np.full(self.n_size, -77, np.int32))

    def sync(self, stream=None):
        if stream is not None:
            stream.synchronize()
        oa.device_synchronize()

    def compute_arrays(self, stream=None, **over):
        """the array form on NaN-padded device copies; returns the device's (VertDiff, VertVisc) with their padding"""
        a = dict(un=self.un, ut=self.ut, n2=self.n2, zmid=self.zmid, zint=self.zint, vd=self.vd, vv=self.vv)
        a.update(over)
        bufs = {n: self.dev(a[n]) for n in ("un", "ut", "n2", "zmid", "vd", "vv")}
        pad = np.full((self.n_size, level_pitch(self.K + 1)), np.nan)
        pad[:, : self.K + 1] = a["zint"]
        bz = oa.DeviceBuffer(pad)
        self.kpp.compute(bufs["un"].ptr, bufs["ut"].ptr, bufs["n2"].ptr, bufs["zmid"].ptr, bz.ptr, bufs["vd"].ptr,
                         bufs["vv"].ptr, stream=stream)
        self.sync(stream)
        return bufs["vd"].to_host(), bufs["vv"].to_host()

    def outputs(self):
        """the four arrays of the object as the device holds them (padding included for the level arrays)"""
        k = self.kpp
        out = {name: raw(k.device_ptr(name), (self.n_size, self.P)) for name in OUT2}
        out["BoundaryLayerDepth"], out["BoundaryLayerIndex"] = k.get("BoundaryLayerDepth"), k.get("BoundaryLayerIndex")
        return out
