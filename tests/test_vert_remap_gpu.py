"""VertRemap on the GPU: each of the four calls equals the NumPy restatement of the contract
(tests/vert_remap_reference.py) bit for bit on NaN-seeded arrays -- entries outside the ranges, land, the sentinel row and
the row padding are NaN and must stay so -- for the three orders, at every layer count at which a launch changes shape;
remap equals the four calls in three launches; the stream forms agree and tracer planes beyond NTracers are left alone;
the refusals that need a device; attached to the split-explicit stepper a step equals the unattached step followed by
remap by hand, allocates nothing, keeps a uniform tracer uniform, and detaching restores the unattached bits."""
import numpy as np
import pytest

import omega_amd as oa
from tests import column_reference as CR
from tests import vert_remap_reference as VR
from tests.column_reference import RHO0
from tests.meshes import named_mesh
from tests.rank_rig import RankRig, raw
from tests.split_explicit_fixtures import StepRig
from tests.vert_fixtures import level_pitch, lds_pitch, mix_inputs, same as _same

pytestmark = pytest.mark.gpu

NT, MAX_TRACERS = 2, 3
ORDERS = (1, 2, 3)
MESHES = ("hex24x20", "fib300_coast_ragged")
LDS_BYTES = 65536


def remap_tile(K):
    """vertRemapColumnTile (kernels/VertRemapKernels.hip), restated: the largest of 16, 8, 4, 2 columns per workgroup
    whose LDS -- per column five level rows of the odd pitch, two interface rows of the odd pitch of P + 1, two scalars
    and four ints -- fits 64 KiB; None: refused"""
    P = level_pitch(K)
    per_column = 5 * lds_pitch(P) + 2 * lds_pitch(P + 1) + 4
    for tile in (16, 8, 4, 2):
        if tile * per_column * 8 <= LDS_BYTES:
            return tile
    return None


def remap_limit():
    K = 1
    while remap_tile(K + 1) is not None:
        K += 1
    return K


def _tile_changes():
    """the layer counts on both sides of every change of the tile"""
    out, K = [], 1
    while remap_tile(K + 1) is not None:
        if remap_tile(K + 1) != remap_tile(K):
            out += [K, K + 1]
        K += 1
    return out


LIMIT = remap_limit()
# the short columns where the boundary rules meet; 15, 16, 17: an odd row pitch (rows off 16 bytes, one level per lane in
# the adoption), the first padded pitch; every change of the tile; the longest column
SMALL = (1, 2, 3, 4, 15, 16, 17)
LEVELS = tuple(sorted(set(SMALL) | set(_tile_changes()) | {LIMIT}))
CASES = [(m, K) for K in LEVELS for i, m in enumerate(MESHES) if K <= 64 or i == LEVELS.index(K) % 2]


@pytest.fixture(scope="module", autouse=True)
def _device():
    oa.device_init(0)


class Rig(RankRig):
    """One rank's VertCoord on global inputs (tests.vert_fixtures.mix_inputs: layer ranges with land, KMin > 0, single
    layers) in local order, a random reference thickness, and the thickness: the reference scaled column-wise by 0.8 ..
    1.25 and perturbed layer-wise by up to +-30 %.  Host-only (device = False) it still restates everything."""

    def __init__(self, g, K, seed=7, device=True):
        super().__init__(g, K, device=device)
        self.P = level_pitch(K)
        G = mix_inputs(g, K, seed, nt=MAX_TRACERS)
        rng = np.random.default_rng(seed + 200)
        n = int(g["nCells"])
        ref = rng.uniform(1.0, 30.0, (n, K))
        h = ref * rng.uniform(0.8, 1.25, (n, 1)) * rng.uniform(0.7, 1.3, (n, K))
        self.ref, self.h0 = self.cells(ref), self.cells(h)
        self.tr0, self.u0 = self.cells(G["tr"]), self.edges(G["un"])
        self.layers(G["min_level"], G["max_level"])
        self.w = CR.movement_weights("Uniform", K)
        self.coe = self.mesh.get_array("CellsOnEdge")
        if device:
            self.vc.set("RefLayerThickness", self.ref)
        self.h, self.tr, self.u = self.seeded(self.h0), self.seeded(self.tr0), self.seeded(self.u0, edge=True)
        self._want = {}

    def want(self, order):
        """the four calls restated, each on what the one before left: target, tracers, u, h, and the overlap counts of
        the cell and edge columns; computed once per order"""
        if order not in self._want:
            tgt = np.full((self.n_size, self.K), np.nan)
            VR.compute_target(self.h, self.ref, self.w, self.lo, self.hi, self.n_all, tgt)
            ci, ei = {}, {}
            tr = VR.remap_tracers(self.h, tgt, self.tr.copy(), NT, self.lo, self.hi, self.n_all, order, ci)
            u = VR.remap_velocity(self.h, tgt, self.u.copy(), self.coe, self.lo_e, self.hi_e, self.e_all, self.n_size,
                                  order, ei)
            h = VR.adopt_target(self.h.copy(), tgt, self.lo, self.hi, self.n_all)
            self._want[order] = dict(target=tgt, tr=tr, u=u, h=h, cell_span=ci.get("span"), edge_span=ei.get("span"))
        return self._want[order]

    def buffers(self):
        return self.dev(self.h), self.dev(self.u), self.dev(self.tr)

    def remap_object(self, order):
        vr = oa.VertRemap(self.mesh, self.vc, MAX_TRACERS, order)
        self.poison(vr)
        return vr

    def poison(self, vr):
        oa.copy_to_device(vr.device_ptr("LayerThicknessTarget"), np.full((self.n_size, self.P), np.nan))

    def target(self, vr):
        return raw(vr.device_ptr("LayerThicknessTarget"), (self.n_size, self.P))


def test_the_levels_cover_the_launch_rules():
    assert LIMIT == oa.VertRemap.max_layers() and remap_tile(LIMIT) == 2 and remap_tile(LIMIT + 1) is None
    assert {remap_tile(K) for K in LEVELS} == {16, 8, 4, 2}
    changes = _tile_changes()
    assert len(changes) == 6 and set(changes) <= set(LEVELS)
    assert [remap_tile(K) for K in changes] == [16, 8, 8, 4, 4, 2]
    assert {1, 2, 3, 4, LIMIT} <= set(LEVELS)
    assert level_pitch(15) % 2 == 1 and level_pitch(17) == 32  # unaligned rows; padded rows
    assert {m for m, K in CASES} == set(MESHES) and {K for m, K in CASES} == set(LEVELS)


@pytest.mark.parametrize("mesh,K", CASES)
def test_bit_exact_on_nan_seeded_arrays(mesh, K):
    x = Rig(named_mesh(mesh), K)
    n, ne = x.n_all, x.e_all
    assert (x.lo[:n] > x.hi[:n]).any() or (x.hi[:n] < 0).any()  # land
    assert (x.lo[:n] == x.hi[:n]).any()                          # single-layer columns
    if K > 2:
        assert (x.lo[:n] > 0).any()                              # KMin > 0
    assert (x.e_active[:ne].sum(axis=1) == 0).any()              # edges left alone
    for order in ORDERS:
        w = x.want(order)
        assert np.isfinite(w["target"][x.active]).all() and (w["target"][x.active] > 0.0).all()
        assert np.isfinite(w["tr"][:NT][:, x.active]).all() and np.isfinite(w["u"][x.e_active]).all()
        vr = x.remap_object(order)
        hb, ub, tb = x.buffers()
        before = vr.launch_count()
        vr.compute_target(hb.ptr)
        oa.device_synchronize()
        _same(x.target(vr), x.padded(w["target"]), f"order {order}: LayerThicknessTarget")
        vr.remap_tracers(hb.ptr, tb.ptr, NT)
        oa.device_synchronize()
        _same(tb.to_host(), x.padded(w["tr"]), f"order {order}: Tracers")  # (plane 2 among them: left alone)
        vr.remap_velocity(hb.ptr, ub.ptr)
        oa.device_synchronize()
        _same(ub.to_host(), x.padded(w["u"]), f"order {order}: NormalVelocity")
        _same(hb.to_host(), x.padded(x.h), f"order {order}: LayerThickness is an input so far")
        vr.adopt_target(hb.ptr)
        oa.device_synchronize()
        _same(hb.to_host(), x.padded(w["h"]), f"order {order}: LayerThickness")
        assert vr.launch_count() == before + 4  # one launch each
        # the one call: the same bits, three launches at most
        x.poison(vr)
        h2, u2, t2 = x.buffers()
        vr.remap(h2.ptr, u2.ptr, t2.ptr, NT)
        oa.device_synchronize()
        assert vr.launch_count() - (before + 4) <= 3
        for name, got, want in (("LayerThickness", h2, hb), ("NormalVelocity", u2, ub), ("Tracers", t2, tb)):
            _same(got.to_host(), want.to_host(), f"order {order}: remap against the four calls: {name}")
        _same(x.target(vr), x.padded(w["target"]), f"order {order}: remap: LayerThicknessTarget")
    # the case is what it is there for: the orders differ, and a target layer overlaps one, two, three and more cells
    if K >= 4:
        assert not np.array_equal(x.want(1)["tr"], x.want(2)["tr"], equal_nan=True)
        assert not np.array_equal(x.want(2)["tr"], x.want(3)["tr"], equal_nan=True)
        assert not np.array_equal(x.want(2)["u"], x.want(3)["u"], equal_nan=True)
    if K >= 15:
        for kind in ("cell_span", "edge_span"):
            spans = set(np.unique(x.want(3)[kind]).tolist())
            assert {1, 2, 3} <= spans, (kind, spans)
    if K >= 64:  # on edges the two totals differ: layers past the source's bottom have no width
        assert (x.want(3)["edge_span"] == 0).any() and not (x.want(3)["cell_span"] == 0).any()


@pytest.mark.parametrize("mesh,K,order", [("fib300_coast_ragged", 17, 3), ("hex24x20", 5, 2)])
def test_the_stream_forms_agree_and_other_planes_are_left_alone(mesh, K, order):
    """the null stream (what the object-`Stream` forms of VertRemap.h forward to by default: they are inline calls of the
    stream forms with the object's `Stream`) against a stream of the caller's, the four calls against the one"""
    x = Rig(named_mesh(mesh), K)
    vr = x.remap_object(order)
    s = oa.Stream()
    outs = []
    for stream in (None, s):
        x.poison(vr)
        hb, ub, tb = x.buffers()
        vr.compute_target(hb.ptr, stream=stream)
        vr.remap_tracers(hb.ptr, tb.ptr, 1, stream=stream)  # one plane of three
        vr.remap_velocity(hb.ptr, ub.ptr, stream=stream)
        vr.adopt_target(hb.ptr, stream=stream)
        if stream is not None:
            stream.synchronize()
        oa.device_synchronize()
        outs.append((x.target(vr), hb.to_host(), ub.to_host(), tb.to_host()))
        x.poison(vr)
        hb, ub, tb = x.buffers()
        vr.remap(hb.ptr, ub.ptr, tb.ptr, 1, stream=stream)
        if stream is not None:
            stream.synchronize()
        oa.device_synchronize()
        outs.append((x.target(vr), hb.to_host(), ub.to_host(), tb.to_host()))
    for o in outs[1:]:
        for name, got, want in zip(("LayerThicknessTarget", "LayerThickness", "NormalVelocity", "Tracers"), o, outs[0]):
            _same(got, want, name)
    tr = outs[0][3]
    _same(tr[1:], x.padded(x.tr)[1:], "planes beyond NTracers")
    _same(tr[0], x.padded(x.want(order)["tr"])[0], "the one plane")
    assert not np.array_equal(tr[0], x.padded(x.tr)[0], equal_nan=True)
    # no tracers: the target, the velocity and the thickness all the same, no plane touched; the numpy forms
    x.poison(vr)
    hb, ub, tb = x.buffers()
    vr.remap(hb.ptr, ub.ptr, None, 0)
    oa.device_synchronize()
    _same(hb.to_host(), outs[0][1], "LayerThickness without tracers")
    _same(ub.to_host(), outs[0][2], "NormalVelocity without tracers")
    h, u, t = vr.remap(np.nan_to_num(x.h, nan=1.0), np.nan_to_num(x.u), np.nan_to_num(x.tr[:NT]), NT)
    w = x.want(order)
    _same(h[x.active], w["h"][x.active], "LayerThickness (numpy form)")
    _same(t[:, x.active], w["tr"][:NT][:, x.active], "Tracers (numpy form)")
    _same(u[x.e_active], w["u"][x.e_active], "NormalVelocity (numpy form)")
    before = tb.to_host()
    for nt in (-1, MAX_TRACERS + 1):  # refused before anything is launched
        with pytest.raises(oa.OmegaAmdError, match="NTracers"):
            vr.remap_tracers(hb.ptr, tb.ptr, nt)
        with pytest.raises(oa.OmegaAmdError, match="NTracers"):
            vr.remap(hb.ptr, ub.ptr, tb.ptr, nt)
    oa.device_synchronize()
    _same(tb.to_host(), before, "Tracers after the refused calls")


def test_refusals_on_a_device():
    K = 8
    x, y = Rig(named_mesh("hex24x20"), K), Rig(named_mesh("hex24x20"), K)
    with pytest.raises(oa.OmegaAmdError, match="VertCoord is NULL"):
        oa.VertRemap(x.mesh, None, 2)
    with pytest.raises(oa.OmegaAmdError, match="another mesh"):
        oa.VertRemap(x.mesh, y.vc, 2)
    with pytest.raises(oa.OmegaAmdError, match="another layer count"):
        oa.VertRemap(x.mesh, oa.VertCoord(x.mesh, K - 1, RHO0, "Uniform"), 2)
    for order in (0, 4, -1):
        with pytest.raises(oa.OmegaAmdError, match="Order"):
            oa.VertRemap(x.mesh, x.vc, 2, order)
    with pytest.raises(oa.OmegaAmdError, match="MaxTracers"):
        oa.VertRemap(x.mesh, x.vc, -1)
    vr = oa.VertRemap(x.mesh, x.vc, 0)  # no tracers is a count
    assert np.all(x.target(vr) == 0.0)  # zero at construction, padding and sentinel row included
    with pytest.raises(oa.OmegaAmdError, match="no array named"):
        vr.get("NoSuchArray")
    # columns too long for the LDS tile: the message names the limit
    decomp = oa.Decomp(oa.GlobalMesh(named_mesh("hex24x20")), 1, 0, 3)
    m = oa.HorzMesh(decomp, LIMIT + 1)
    with pytest.raises(oa.OmegaAmdError, match=f"NVertLayers <= {LIMIT}"):
        oa.VertRemap(m, oa.VertCoord(m, LIMIT + 1, RHO0, "Uniform", decomp=decomp), 2)


# ---------------------------------------------------------------------------------------------------------------------
# attached to the split-explicit stepper
# ---------------------------------------------------------------------------------------------------------------------
STEP_K, NSUB, STEP_DT = 5, 3, 20.0


def step_rig(attached=False, uniform=None):
    """tests.split_explicit_fixtures.StepRig on hex24x20 (RefLayerThickness 10, h in 8 .. 12) with nothing on the
    Tendencies (attached: a PressureGrad and a VertAdv); uniform: tracer 1 is that value everywhere"""
    x = StepRig(K=STEP_K, attached=attached, g=named_mesh("hex24x20"))
    if uniform is not None:
        x.tr[1, : x.p.mesh.NCellsAll] = uniform
        x.load()
    return x


def by_hand(x, vr):
    """VertRemap::remap on the current time level of the rig, through the public call"""
    st = x.p.state
    vr.remap(st.device_ptr(0, 0), st.device_ptr(1, 0), x.p.tracers.device_ptr(0), x.nt)
    oa.device_synchronize()


@pytest.mark.parametrize("order", ORDERS)
def test_step_equals_the_unattached_step_then_remap(order):
    a, b, c = step_rig(), step_rig(), step_rig()
    vra, vrb = (oa.VertRemap(r.p.mesh, r.vc, r.nt, order) for r in (a, b))
    st = a.stepper("Split-Explicit", STEP_DT, NSUB)
    st.attach_vert_remap(vra)
    st.do_step(a.p.state)
    oa.device_synchronize()
    before, launches = oa.device_resource_count(), vra.launch_count()
    st.do_step(a.p.state)
    oa.device_synchronize()
    assert oa.device_resource_count() == before  # a step with the remap attached allocates nothing
    assert vra.launch_count() - launches <= 3
    stb, stc = b.stepper("Split-Explicit", STEP_DT, NSUB), c.stepper("Split-Explicit", STEP_DT, NSUB)
    for _ in range(2):
        stb.do_step(b.p.state)
        oa.device_synchronize()
        by_hand(b, vrb)
        stc.do_step(c.p.state)
    plain = c.result()
    for name, got, want, other in zip(("h", "u", "tracers"), a.result(), b.result(), plain):
        assert np.all(np.isfinite(got)), name
        _same(got, want, f"{name}: the stepper against the step and the remap by hand")
        assert not np.array_equal(got, other), f"{name}: the remap moves it"
    _same(vra.get("LayerThicknessTarget"), vrb.get("LayerThicknessTarget"), "LayerThicknessTarget")
    n = a.p.mesh.NCellsAll
    _same(a.result()[0][:n], vra.get("LayerThicknessTarget")[:n], "h is the target")
    # z-star with a uniform reference: every layer of a column has the same thickness, and the column total is the
    # Lagrangian step's
    h = a.result()[0][:n]
    assert np.allclose(h, h[:, :1], rtol=1e-14) and not np.allclose(plain[0][:n], plain[0][:n, :1], rtol=1e-3)
    # detached: the unattached bits
    d = step_rig()
    std = d.stepper("Split-Explicit", STEP_DT, NSUB)
    vrd = oa.VertRemap(d.p.mesh, d.vc, d.nt, order)
    std.attach_vert_remap(vrd)
    std.attach_vert_remap(None)
    for _ in range(2):
        std.do_step(d.p.state)
    for name, got, want in zip(("h", "u", "tracers"), d.result(), plain):
        _same(got, want, f"{name}: detached against unattached")
    assert vrd.launch_count() == 0 and np.all(vrd.get("LayerThicknessTarget") == 0.0)


@pytest.mark.parametrize("order", ORDERS)
def test_a_uniform_tracer_stays_uniform(order):
    x = step_rig(uniform=1.0)
    vr = oa.VertRemap(x.p.mesh, x.vc, x.nt, order)
    st = x.stepper("Split-Explicit", STEP_DT, NSUB)
    st.attach_vert_remap(vr)
    for _ in range(3):
        st.do_step(x.p.state)
    h, u, tr = x.result()
    n = x.p.mesh.NCellsAll
    assert np.all(tr[1, :n] == 1.0)  # bit for bit
    assert np.all(np.isfinite(tr[0, :n])) and not np.array_equal(tr[0, :n], x.tr[0, :n])
    assert vr.launch_count() == 9


def test_attachment_refusals():
    x = step_rig(attached=True)  # a VertAdv on the Tendencies
    m = x.p.mesh
    vr = oa.VertRemap(m, x.vc, x.nt)
    st = x.stepper("Split-Explicit", STEP_DT, NSUB)
    base = x.result()
    with pytest.raises(oa.OmegaAmdError, match="a VertAdv is attached to the Tendencies"):
        st.attach_vert_remap(vr)
    with pytest.raises(oa.OmegaAmdError, match="Split-Explicit"):
        x.stepper("RungeKutta4", STEP_DT).attach_vert_remap(vr)
    y = step_rig()
    sty = y.stepper("Split-Explicit", STEP_DT, NSUB)
    with pytest.raises(oa.OmegaAmdError, match="another mesh or layer count"):
        sty.attach_vert_remap(vr)
    with pytest.raises(oa.OmegaAmdError, match="MaxTracers = 1"):
        sty.attach_vert_remap(oa.VertRemap(y.p.mesh, y.vc, 1))
    vry = oa.VertRemap(y.p.mesh, y.vc, y.nt)
    sty.attach_vert_remap(vry)
    va = oa.VertAdv(y.p.mesh, y.vc, 2)
    y.p.tend.attach_vert_adv(va)  # checked again in every step
    with pytest.raises(oa.OmegaAmdError, match="a VertAdv is attached to the Tendencies"):
        sty.do_step(y.p.state)
    y.p.tend.attach_vert_adv(None)
    sty.do_step(y.p.state)
    assert vry.launch_count() == 3
    for got, want in zip(x.result(), base):
        _same(got, want, "a refused attachment leaves the state alone")
