"""MESH and SPLINE of the particle VM on the device (lmx_particles_set_mesh_source / _set_spline) against
tests/particle_source_oracle.py: every channel value in [0, count), every count and every slice row in [0, count) bit for bit, the guards
untouched. A comparison leaves out exactly two things: the rows between count and the next multiple of four, and the outputs behind a
whole-chunk program that a SPLINE without a spline ended."""
import numpy as np
import pytest

from tests import particle_asm as A
from tests import particle_source_oracle as S
from tests import ribbon_oracle as R
from tests.particle_asm import CH, REG, LIT, LIT_BITS, SYS, OUT
from tests.test_gpu_particles import GUARD, assert_bits, table, u32

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
NAN = 0x7FC00000
NEG_ZERO = 0x80000000


# ---- models: a mesh, its skin and the palettes of a pose -------------------------------------------------------------------------------
class Model:
    """A skinned model on the device's skinning module: n_bones bones, n_verts vertices, one skin instance per pose."""

    def __init__(self, ctx, n_verts, n_bones, n_poses=1, seed=0, skin_edit=None):
        from lumixengine_amd import api, scenes

        self.sk = api.Skinning(ctx)
        self.sk.setMode(True)
        skel = scenes.skeleton(n_bones, seed=40 + seed)
        self.verts, self.skin = scenes.skinned_mesh(n_verts, n_bones, seed=60 + seed)
        if skin_edit is not None: skin_edit(self.skin)
        own = self.skin.copy()
        own["indices"] = np.clip(own["indices"], 0, n_bones - 1)  # the skinning module's own copy: it skins every vertex, ours only some
        model = self.sk.addModel(skel["parents"], skel["bind"], skel["first_nonroot"])
        mesh = self.sk.addMesh(self.verts, own)
        self.n_bones, self.n_poses = n_bones, n_poses
        self.sk.setInstances([model] * n_poses, [mesh] * n_poses)

    def pose(self, seed):
        """uploads the poses of `seed`, runs the skinning; no host wait"""
        from lumixengine_amd import scenes

        pos, rot = scenes.relative_poses(self.n_poses, self.n_bones, seed=seed)
        self.sk.uploadPoses(pos.reshape(-1, 3), rot.reshape(-1, 4))
        self.sk.run()

    def palette(self, instance=0):
        return self.sk.readPalette(instance)["columns"].copy()


def plain_mesh(n, seed=1):
    return np.random.default_rng(seed).uniform(-4.0, 4.0, size=(n, 3)).astype(np.float32)


class Pair:
    """The device object and the oracle world over the same programs and sources. decl[si] = dict(mesh=(positions, skin) | None,
    skin_instance, bones, spline) or None for a system that declares nothing; `sources[si]` is the oracle's view of the same."""

    def __init__(self, ctx, systems, capacities, decl, sources, seed=0, options=None):
        from lumixengine_amd import api

        self.ps = api.ParticleSystems(ctx)
        self.world = S.make_world(systems, capacities, sources, options, seed)
        self.meshes = {}
        for si, progs in enumerate(systems):
            assert self.ps.addSystem(len(progs), 0) == si
            self.declare(si, decl[si])
            for ei, p in enumerate(progs):
                p.set_on(self.ps, si, ei)
                if options is not None and options[si][ei] is not None: options[si][ei].set_on(self.ps, si, ei)
                else: self.ps.reserve(si, ei, capacities if isinstance(capacities, int) else capacities[si][ei])
        self.ps.setSeed(seed)

    def declare(self, si, d):
        if d is None: return
        if "mesh" in d:
            mesh = NONE
            if d["mesh"] is not None:
                key = id(d["mesh"][0])  # shared between systems: uploaded once
                if key not in self.meshes: self.meshes[key] = self.ps.addMesh(*d["mesh"])
                mesh = self.meshes[key]
            self.ps.setMeshSource(si, mesh, d.get("skin_instance", NONE), 1 if d.get("bones") else 0)
        if "spline" in d: self.ps.setSpline(si, d["spline"])

    def step(self, dt, check=True, **kw):
        self.ps.update(dt)
        self.ps.fill()
        self.world.step(dt)
        if check: self.check(**kw)

    def check(self, outputs_upto=None):
        """outputs_upto[g]: only the first so many outputs of every row are compared (a program that a missing spline ended)"""
        counts = self.ps.counts()
        slices, frame = self.ps.readSlices()
        want = self.world.fill()
        offset, g = 0, 0
        for si, sy in enumerate(self.world.systems):
            for ei, em in enumerate(sy.emitters):
                c = counts[g]
                assert (int(c["particles"]), int(c["emit_index"]), int(c["overflow"]), int(c["killed"])) == (em.count, em.emit_index, em.overflow, em.killed), (si, ei)
                got = self.ps.readChannels(si, ei, em.p.channels)
                ribbon = getattr(em, "is_ribbon", False)
                if ribbon:
                    L = em.opts.max_ribbon_length
                    for r, rb in enumerate(em.ribbons):
                        assert_bits(got[:, r * L:r * L + rb.length], em.ch[:, r * L:r * L + rb.length], f"ribbon {r} of system {si} emitter {ei}")
                else:
                    assert_bits(got[:, :em.count], em.ch[:, :em.count], f"channels of system {si} emitter {ei}")
                assert np.all(u32(got[:, em.capacity:]) == GUARD), (si, ei, "channel guard written")
                out, n = want[g]
                s = slices[g]
                assert (int(s["offset"]), int(s["bytes"]), int(s["particles"])) == (offset, out.nbytes, n), (si, ei)
                nout = em.p.outputs
                rows = frame[offset // 4: offset // 4 + n * nout].reshape(n, nout)
                upto = nout if outputs_upto is None else outputs_upto[g]
                assert_bits(rows[:, :upto], out[:n * nout].reshape(n, nout)[:, :upto], f"slice of system {si} emitter {ei}")
                offset += out.nbytes
                g += 1
        assert np.all(u32(frame[-64:]) == GUARD), "frame guard written"

    def close(self):
        self.ps.close()


def run(ctx, systems, capacities, decl, sources, dts=(0.25,), **kw):
    p = Pair(ctx, systems, capacities, decl, sources, **kw)
    try:
        for dt in dts: p.step(dt)
    finally:
        p.close()
    return p


def unskinned(n, seed=1):
    """(device declaration, oracle source) of a model without bones"""
    m = plain_mesh(n, seed)
    return dict(mesh=(m, None)), S.Source(mesh=m)


def skinned(model, instance=0, palette=None):
    return (dict(mesh=(model.verts, model.skin), skin_instance=instance, bones=True),
            S.Source(mesh=model.verts, skin=model.skin, has_bones=True, palette=model.palette(instance) if palette is None else palette))


def xyz_emit(index_ops, nch=5):
    """emit program: channel 0 = the index (by `index_ops`), channels 1..3 = the vertex, channel 4 = a marker written behind the MESHes"""
    return index_ops + [A.mesh(CH(1), CH(0), 0), A.mesh(CH(2), CH(0), 1), A.mesh(CH(3), CH(0), 2), A.mov(CH(4), LIT(7.0))]


OUT5 = [A.mov(OUT(k), CH(k)) for k in range(5)]


# ---- vertices and draws -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_verts", [1, 2, 63, 64, 65, 1025])
def test_drawn_vertex_of_an_unskinned_mesh(gpu_ctx, n_verts):
    """A negative index draws float(r % n): the drawn index is read back (it is written to its channel), the three components follow it; the
    second MESH of the program finds the index already drawn. Twice with one seed: the same bytes."""
    d, s = unskinned(n_verts)
    p = A.Program([], xyz_emit([A.mov(CH(0), LIT(-1.0))]), OUT5, channels=5, outputs=5, init_emit_count=70)
    got = []
    for _ in range(2):
        pair = run(gpu_ctx, [[p]], 72, [d], [s], seed=11)
        em = pair.world.systems[0].emitters[0]
        got.append(em.ch[:, :em.count].copy())
        idx = em.ch[0, :em.count]
        assert np.all((idx >= 0) & (idx < n_verts) & (idx == np.floor(idx)))
        if n_verts >= 63: assert len(np.unique(idx)) > 20
    assert np.array_equal(u32(got[0]), u32(got[1]))


def test_two_mesh_instructions_draw_differently(gpu_ctx):
    d, s = unskinned(1025)
    emit = [A.mov(CH(0), LIT(-1.0)), A.mov(CH(1), LIT(-3.5)), A.mesh(CH(2), CH(0), 0), A.mesh(CH(3), CH(1), 0)]
    p = A.Program([], emit, [A.mov(OUT(0), CH(2))], channels=4, outputs=1, init_emit_count=64)
    pair = run(gpu_ctx, [[p]], 64, [d], [s], seed=5)
    ch = pair.world.systems[0].emitters[0].ch
    assert np.count_nonzero(ch[0, :64] != ch[1, :64]) > 50


def test_index_handed_in(gpu_ctx):
    """k + 0.49 and k + 0.5 (u32(index + 0.5f)), n - 1, n (vertex 0), -0.0 (no draw), NaN (no draw, vertex 0), and a LITERAL index"""
    n = 65
    d, s = unskinned(n)
    values = [0.0, 3.49, 3.5, 62.49, 62.5, float(n - 1), float(n), NEG_ZERO, NAN, 1.0e10, 4294967296.0, 63.5, 64.49]
    emit = table(CH(0), values) + [A.mesh(CH(1), CH(0), 0), A.mesh(CH(2), CH(0), 1), A.mesh(CH(3), CH(0), 2), A.mesh(CH(4), LIT(17.0), 1)]
    p = A.Program([], emit, OUT5, channels=5, registers=2, outputs=5, init_emit_count=len(values))
    pair = run(gpu_ctx, [[p]], 16, [d], [s])
    ch = pair.world.systems[0].emitters[0].ch
    m = s.mesh
    assert_bits(ch[0, :len(values)], np.array([v if not isinstance(v, int) else np.uint32(v).view(np.float32) for v in values], np.float32), "an index that is not negative is not written")
    assert ch[1, 1] == m[3, 0] and ch[1, 2] == m[4, 0] and ch[1, 6] == m[0, 0] and ch[1, 7] == m[0, 0] and ch[1, 8] == m[0, 0] and ch[4, 0] == m[17, 1]


# ---- skin -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bones", [1, 3, 196])
def test_skinned_vertex(gpu_ctx, n_bones):
    """Every subindex against the whole evalVertexPose; weights with zeros; a bone index past the pose (bone 0)."""
    def edit(skin):
        skin["weights"][5] = [1.0, 0.0, 0.0, 0.0]
        skin["weights"][6] = [0.0, 0.5, 0.0, 0.5]
        skin["indices"][7] = [n_bones, 0, n_bones + 7, 32767]

    model = Model(gpu_ctx, 67, n_bones, skin_edit=edit)
    model.pose(7)
    d, s = skinned(model)
    emit = xyz_emit([A.mov(CH(0), SYS(A.EMIT_INDEX))])
    p = A.Program([], emit, OUT5, channels=5, outputs=5, init_emit_count=67)
    pair = run(gpu_ctx, [[p]], 68, [d], [s])
    ch = pair.world.systems[0].emitters[0].ch
    assert np.all(ch[4, :67] == 7.0) and np.all(np.isfinite(ch[1:4, :67]))


def test_bones_without_a_pose_and_no_model(gpu_ctx):
    """Bones and no pose: the index is drawn and written, dst is not, the run ends (the marker behind the MESH is not written). No model:
    the instruction in front of the MESH ran, the one behind it did not."""
    model = Model(gpu_ctx, 10, 3)
    model.pose(3)
    emit = [A.mov(CH(1), LIT(5.0)), A.mov(CH(0), LIT(-1.0)), A.mesh(CH(2), CH(0), 0), A.mov(CH(3), LIT(9.0))]
    p = A.Program([], emit, [A.mov(OUT(k), CH(k)) for k in range(4)], channels=4, outputs=4, init_emit_count=9)
    no_pose = (dict(mesh=(model.verts, model.skin), skin_instance=NONE, bones=True), S.Source(mesh=model.verts, skin=model.skin, has_bones=True))
    no_model = (dict(mesh=None), S.Source())
    pair = run(gpu_ctx, [[p], [p]], 12, [no_pose[0], no_model[0]], [no_pose[1], no_model[1]], seed=2)
    a, b = (sy.emitters[0].ch for sy in pair.world.systems)
    assert np.all(a[1, :9] == 5.0) and np.all(a[0, :9] >= 0) and np.all(a[2, :9] == 0) and np.all(a[3, :9] == 0)
    assert np.all(b[1, :9] == 5.0) and np.all(b[0, :9] == -1.0) and np.all(b[3, :9] == 0)


def test_pose_follows_the_stream(gpu_ctx):
    """lmx_skin_run with pose A, step; pose B, step; nothing waits in between: each step's values follow its pose."""
    model = Model(gpu_ctx, 40, 5)
    model.pose(100); pal_a = model.palette()
    model.pose(101); pal_b = model.palette()
    assert not np.array_equal(pal_a, pal_b)
    d, s = skinned(model, palette=pal_a)
    update = [A.lt(REG(0), LIT(-1.0), CH(0)), A.sub(REG(0), LIT(0.0), REG(0)), A.cmp(REG(0), [A.mesh(CH(1), CH(0), 0), A.mesh(CH(2), CH(0), 1), A.mesh(CH(3), CH(0), 2)])]
    p = A.Program(update, [A.mov(CH(0), SYS(A.EMIT_INDEX))], OUT5, channels=5, registers=1, outputs=5, init_emit_count=40)
    pair = Pair(gpu_ctx, [[p]], 40, [d], [s])
    try:
        model.pose(100)
        pair.ps.update(0.1)
        model.pose(101)
        pair.ps.update(0.1)
        pair.world.step(0.1)
        first = pair.world.systems[0].emitters[0].ch.copy()
        s.palette = pal_b
        pair.world.step(0.1)
        assert not np.array_equal(first[1:4], pair.world.systems[0].emitters[0].ch[1:4])
        pair.ps.fill()
        pair.check()
    finally:
        pair.close()


# ---- lanes and edges --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("burst", [1, 255, 256, 257])
def test_mesh_in_the_emit_program(gpu_ctx, burst):
    """first-frame bursts around the emit kernel's block of 256, then a rate emission"""
    model = Model(gpu_ctx, 130, 3, n_poses=2)
    model.pose(9)
    (d0, s0), (d1, s1) = skinned(model, 0), skinned(model, 1)  # two systems on one model: one mesh on the device, a pose each
    p = A.Program([], xyz_emit([A.mov(CH(0), LIT(-2.0))]), OUT5, channels=5, outputs=5, init_emit_count=burst, emit_per_second=40.0)
    pair = run(gpu_ctx, [[p], [p]], burst + 24, [d0, d1], [s0, s1], dts=(0.25, 0.25), seed=3)
    assert len(pair.meshes) == 1


SIGN = [A.sub(REG(0), LIT(0.0), LIT(1.0))]  # a condition whose sign bit is set


@pytest.mark.parametrize("n", [1023, 1024, 1025])
@pytest.mark.parametrize("killing", [False, True, "index written by the MESH alone"])
def test_mesh_in_an_update_block(gpu_ctx, n, killing):
    """A CMP block that re-reads the vertex over the chunk edge; `killing`: the block also kills every fifth particle and writes the MESH
    destination and index channels (the snapshot of the killing block and the kill replay take both from the write mask). In the last
    variant nothing but the MESH's draw writes the index channel (negative since the emission): a killed slot must take the index its
    survivor had BEFORE the block, which only a write mask that holds the index gives."""
    d, s = unskinned(65)
    alone = killing not in (False, True)
    body = ([] if alone else [A.mov(CH(0), LIT(-1.0))]) + [A.mesh(CH(1), CH(0), 0), A.mesh(CH(2), CH(0), 2)]
    if killing: body += [A.mod(REG(1), CH(3), LIT(5.0)), A.lt(REG(1), REG(1), LIT(0.5)), A.cmp(REG(1), [A.KILL])]
    emit = [A.mov(CH(3), SYS(A.EMIT_INDEX))] + ([A.mov(CH(0), LIT(-1.0))] if alone else [])
    p = A.Program(SIGN + [A.cmp(REG(0), body)], emit, [A.mov(OUT(k), CH(k)) for k in range(4)], channels=4, registers=2, outputs=4, init_emit_count=n)
    pair = run(gpu_ctx, [[p]], n + 3, [d], [s], dts=(0.1, 0.1), seed=8)
    if alone: assert np.any(pair.world.systems[0].emitters[0].ch[0, :n // 2] == -1.0)  # survivors moved into killed slots before their own turn


def test_mesh_in_both_arms_of_a_cmp_else(gpu_ctx):
    d, s = unskinned(64)
    update = [A.mov(REG(1), LIT(2.0)), A.mod(REG(0), CH(3), REG(1)), A.sub(REG(0), LIT(0.5), REG(0)),
              A.cmp_else(REG(0), [A.mesh(CH(1), CH(3), 0)], [A.mov(CH(0), LIT(-1.0)), A.mesh(CH(1), CH(0), 1), A.mesh(CH(2), CH(0), 2)])]
    p = A.Program(update, [A.mov(CH(3), SYS(A.EMIT_INDEX))], [A.mov(OUT(k), CH(k)) for k in range(4)], channels=4, registers=2, outputs=4, init_emit_count=70)
    run(gpu_ctx, [[p]], 72, [d], [s], seed=4)


def test_mesh_in_a_sub_emission_target(gpu_ctx):
    model = Model(gpu_ctx, 33, 3)
    model.pose(12)
    d, s = skinned(model)
    parent = A.Program(SIGN + [A.cmp(REG(0), [A.emit(1, [A.mov(OUT(0), CH(0))])])], [A.mov(CH(0), SYS(A.EMIT_INDEX))], [A.mov(OUT(0), CH(0))], channels=1,
                       registers=1, outputs=1, init_emit_count=5)
    child = A.Program([], [A.mov(CH(0), REG(0)), A.mov(CH(4), LIT(-1.0)), A.mesh(CH(1), CH(0), 0), A.mesh(CH(2), CH(4), 1), A.mesh(CH(3), CH(4), 2)], OUT5,
                      channels=5, outputs=5, emit_inputs=1, init_emit_count=3)
    run(gpu_ctx, [[parent, child]], [[8, 64]], [d], [s], dts=(0.1, 0.1), seed=6)


def test_ribbon_emitter_with_mesh_and_spline(gpu_ctx):
    """MESH in a ribbon emitter's emit program, SPLINE in its output program"""
    m = plain_mesh(50)
    pts = np.random.default_rng(3).uniform(-2, 2, size=(5, 3)).astype(np.float32)
    d, s = dict(mesh=(m, None), spline=pts), S.Source(mesh=m, spline=pts)
    emit = [A.mov(CH(0), LIT(-1.0)), A.mesh(CH(1), CH(0), 1), A.mul(CH(2), SYS(A.EMIT_INDEX), LIT(0.07))]
    p = A.Program([A.add(CH(2), CH(2), SYS(A.TIME_DELTA))], emit, [A.mov(OUT(0), CH(1)), A.spline(OUT(1), CH(2), 0), A.spline(OUT(2), CH(2), 2)], channels=3, outputs=3,
                  init_emit_count=3, emit_per_second=20.0)
    opts = R.Options(max_ribbons=3, max_ribbon_length=8, init_ribbons_count=2)
    run(gpu_ctx, [[p]], 0, [d], [s], dts=(0.1, 0.2, 0.2), seed=9, options=[[opts]])


# ---- spline -----------------------------------------------------------------------------------------------------------------------------
def spline_ts(n_points):
    """0, 1, every segment boundary and its two neighbours in ulps, negative, > 1, 1e10, -0.0, NaN"""
    ts = [0.0, 1.0, -0.25, -1.0, -3.0, 1.5, 1.0e10, NEG_ZERO, NAN, 0.3, 0.77]
    for k in range(1, n_points - 1):
        b = np.float32(k) / np.float32(n_points - 2)
        ts += [float(np.nextafter(b, np.float32(-1))), float(b), float(np.nextafter(b, np.float32(2)))]
    return ts


@pytest.mark.parametrize("n_points", [3, 4, 7])
def test_spline_scalar_and_whole_chunk(gpu_ctx, n_points):
    """every subindex, the scalar form (in a block, into channels) and the whole-chunk form (into outputs) on the same inputs"""
    pts = np.random.default_rng(n_points).uniform(-5, 5, size=(n_points, 3)).astype(np.float32)
    ts = spline_ts(n_points)
    update = SIGN + [A.cmp(REG(0), [A.spline(CH(1 + k), CH(0), k) for k in range(3)])]
    output = [A.spline(OUT(k), CH(0), k) for k in range(3)] + [A.mov(OUT(3 + k), CH(1 + k)) for k in range(3)]
    p = A.Program(update, table(CH(0), ts), output, channels=4, registers=2, outputs=6, init_emit_count=len(ts))
    pair = run(gpu_ctx, [[p]], len(ts), [dict(spline=pts)], [S.Source(spline=pts)])
    out, n = pair.world.fill()[0]
    rows = out[:n * 6].reshape(n, 6)
    assert_bits(rows[:, :3], rows[:, 3:], "the scalar and the whole-chunk form agree")


def test_no_spline(gpu_ctx):
    """Scalar: the run ends (the instruction behind the SPLINE does not run). Whole-chunk: the program ends; only the outputs written
    before the instruction are compared."""
    update = SIGN + [A.cmp(REG(0), [A.mov(CH(1), LIT(2.0)), A.spline(CH(2), CH(0), 1), A.mov(CH(3), LIT(4.0))])]
    output = [A.mov(OUT(0), CH(1)), A.spline(OUT(1), CH(0), 0), A.mov(OUT(2), CH(3))]
    p = A.Program(update, [A.mov(CH(0), LIT(0.5))], output, channels=4, registers=1, outputs=3, init_emit_count=6)
    pair = Pair(gpu_ctx, [[p]], 8, [dict(spline=None)], [S.Source()])
    try:
        pair.step(0.1, outputs_upto=[1])
        ch = pair.world.systems[0].emitters[0].ch
        assert np.all(ch[1, :6] == 2.0) and np.all(ch[2, :6] == 0) and np.all(ch[3, :6] == 0)
    finally:
        pair.close()


def test_spline_replaced_between_two_fills(gpu_ctx):
    a = np.random.default_rng(1).uniform(-5, 5, size=(4, 3)).astype(np.float32)
    b = np.random.default_rng(2).uniform(-5, 5, size=(6, 3)).astype(np.float32)
    p = A.Program([], [A.mul(CH(0), SYS(A.EMIT_INDEX), LIT(0.11))], [A.spline(OUT(k), CH(0), k) for k in range(3)], channels=1, outputs=3, init_emit_count=10)
    src = S.Source(spline=a)
    pair = Pair(gpu_ctx, [[p]], 12, [dict(spline=a)], [src])
    try:
        pair.step(0.1)
        first = pair.world.fill()[0][0].copy()
        pair.ps.setSpline(0, b)
        src.spline = b
        pair.ps.fill()
        pair.check()
        assert not np.array_equal(first, pair.world.fill()[0][0])
        counts = pair.ps.counts()
        assert int(counts[0]["particles"]) == 10  # no new layout, no reset
    finally:
        pair.close()


# ---- refusals and bookkeeping -----------------------------------------------------------------------------------------------------------
def code_of(fn):
    from lumixengine_amd import api

    with pytest.raises(api.LumixError) as e:
        fn()
    return e.value.code


OK_PROG = A.Program([], [A.mov(CH(0), LIT(-1.0)), A.mesh(CH(1), CH(0), 0)], [A.spline(OUT(0), CH(0), 1)], channels=2, outputs=1, init_emit_count=4)
INVALID, UNSUPPORTED, INVALID_ARGUMENT, NOT_BUILT = 8, 9, 1, 6  # LMX_ERR_*


def test_refusals_leave_the_object_usable(gpu_ctx):
    from lumixengine_amd import api

    m = plain_mesh(9)
    pts = np.zeros((3, 3), np.float32)
    ps = api.ParticleSystems(gpu_ctx)
    try:
        assert ps.addSystem(1, 1) == 0 and ps.addSystem(1, 0) == 1
        # the undeclared system still answers LMX_ERR_UNSUPPORTED, for MESH and for SPLINE on their own
        assert code_of(lambda: OK_PROG.set_on(ps, 1, 0)) == UNSUPPORTED
        ps.setSpline(1, None)
        assert code_of(lambda: OK_PROG.set_on(ps, 1, 0)) == UNSUPPORTED  # MESH still undeclared
        # lmx_particles_set_mesh_source / _set_spline / _add_mesh
        mesh = ps.addMesh(m)
        assert code_of(lambda: ps.setMeshSource(0, mesh, NONE, 1)) == INVALID_ARGUMENT      # bones, and the mesh carries no skin
        assert code_of(lambda: ps.setMeshSource(0, mesh + 1, NONE, 0)) == INVALID_ARGUMENT  # no such mesh
        assert code_of(lambda: ps.setMeshSource(0, mesh, NONE, 2)) == INVALID_ARGUMENT      # unknown flag
        assert code_of(lambda: ps.setMeshSource(7, mesh, NONE, 0)) == INVALID_ARGUMENT
        assert code_of(lambda: ps.setSpline(0, pts[:1])) == INVALID_ARGUMENT
        assert code_of(lambda: ps.setSpline(0, pts[:2])) == INVALID_ARGUMENT
        assert code_of(lambda: ps.setSpline(7, pts)) == INVALID_ARGUMENT
        assert code_of(lambda: ps.addMesh(np.zeros((0, 3), np.float32))) == INVALID_ARGUMENT
        assert code_of(lambda: OK_PROG.set_on(ps, 0, 0)) == UNSUPPORTED  # a refused declaration is no declaration
        ps.setMeshSource(0, mesh, NONE, 0)
        ps.setSpline(0, pts)
        # the decoder's refusals
        def prog(update=(), emit=(), output=(), **kw):
            return A.Program(list(update), list(emit), list(output), channels=2, registers=1, outputs=1, **kw)

        invalid = [prog(emit=[A.mesh(CH(0), CH(1), 3)]), prog(emit=[A.spline(CH(0), CH(1), 3)]), prog(output=[A.spline(OUT(0), CH(1), 255)]),
                   prog(emit=[A.mesh(CH(0), A.GLOB(0), 0)]), prog(emit=[A.mesh(CH(0), SYS(A.EMIT_INDEX), 0)]), prog(emit=[A.mesh(CH(0), LIT(-1.0), 0)]),
                   prog(emit=[A.mesh(LIT(0.0), CH(1), 0)]), prog(emit=[A.mesh(CH(2), CH(1), 0)]), prog(emit=[A.spline(CH(0), CH(2), 0)]),
                   prog(output=[A.spline(OUT(0), LIT(0.5), 0)]), prog(output=[A.spline(OUT(1), CH(0), 0)])]
        for k, p in enumerate(invalid):
            assert code_of(lambda: p.set_on(ps, 0, 0)) == INVALID, k
        unsupported = [prog(update=[A.mesh(CH(0), CH(1), 0)]), prog(output=[A.mesh(OUT(0), CH(1), 0)]), prog(update=[A.spline(CH(0), CH(1), 0)]),
                       prog(update=[A.spline(REG(0), CH(1), 0)]),
                       prog(update=SIGN + [A.cmp(REG(0), [A.emit(0, [A.mesh(OUT(0), CH(1), 0)])])]),
                       prog(update=SIGN + [A.cmp(REG(0), [A.emit(0, [A.spline(OUT(0), CH(1), 0)])])])]
        for k, p in enumerate(unsupported):
            assert code_of(lambda: p.set_on(ps, 0, 0)) == UNSUPPORTED, k
        # a skin instance past the skinning module's: LMX_ERR_NOT_BUILT from the step, and the step after a good declaration runs
        OK_PROG.set_on(ps, 0, 0)
        ps.reserve(0, 0, 8)
        A.Program([], [], [A.mov(OUT(0), CH(0))]).set_on(ps, 1, 0)
        ps.reserve(1, 0, 4)
        ps.setMeshSource(0, mesh, 1 << 20, 0)
        assert code_of(lambda: ps.update(0.1)) == NOT_BUILT
        assert code_of(lambda: ps.fill()) == NOT_BUILT
        model = Model(gpu_ctx, 4, 2)  # new skin instances and no lmx_skin_run yet: there is no palette to read
        ps.setMeshSource(0, mesh, 0, 0)
        assert code_of(lambda: ps.update(0.1)) == NOT_BUILT
        model.pose(1)
        ps.update(0.1)
        ps.fill()
        assert int(ps.counts()[0]["particles"]) == 4  # the refused steps emitted nothing
        got = ps.readChannels(0, 0, 2)
        assert np.all(got[0, :4] >= 0) and np.all(u32(got[:, 8:]) == GUARD)
    finally:
        ps.close()


def test_clear_meshes_with_a_source_still_bound(gpu_ctx):
    """the source that named a mesh has none afterwards: the run ends at the MESH; a mesh added and bound again is read"""
    d, s = unskinned(20)
    emit = [A.mov(CH(0), LIT(-1.0)), A.mesh(CH(1), CH(0), 0), A.mov(CH(2), LIT(1.0))]
    p = A.Program([], emit, [A.mov(OUT(k), CH(k)) for k in range(3)], channels=3, outputs=3, init_emit_count=3, emit_per_second=30.0)
    pair = Pair(gpu_ctx, [[p]], 32, [d], [s])
    try:
        pair.step(0.1)
        pair.ps.clearMeshes()
        mesh, s.mesh = s.mesh, None
        pair.step(0.1)
        assert np.all(pair.world.systems[0].emitters[0].ch[2, 6:9] == 0)  # the three particles of this step's rate emission
        again = pair.ps.addMesh(mesh[::-1].copy())
        pair.ps.setMeshSource(0, again, NONE, 0)
        s.mesh = mesh[::-1].copy()
        pair.step(0.1)
    finally:
        pair.close()
