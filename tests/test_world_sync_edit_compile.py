"""lumixengine_amd/host/world_sync.h with WorldSync::edit - World::destroyEntity / createEntity / setParent of a frame handed over as one
batch of the reference's own EntityRef / EntityPtr / Transform values - against the reference's REAL headers under
-DLMX_WITH_LUMIX_HEADERS, and mi355_plugin.cpp's queue in front of it: Mi355Module binds World::entityCreated / entityDestroyed to its
queue, re-parents through Mi355Module::setParent, and update() sends the frame's batch. Syntax-only, as tests/test_plugin_compile.py;
skipped where the reference tree is absent. (tests/test_gpu_world_sync_edit_run.py RUNS WorldSync::edit against the oracles.)"""
import os
import subprocess

from tests.test_plugin_compile import FLAGS, HOST, REF, ROOT, ref_src  # noqa: F401 - ref_src is the fixture

USE = ('#include "world_sync.h"\n'
       "bool use(Lumix::WorldSync& sync, Lumix::World& world, Lumix::EntityRef doomed, Lumix::EntityPtr parent) {\n"
       "\tconst Lumix::EntityRef made = world.createEntity(Lumix::DVec3(1, 2, 3), Lumix::Quat::IDENTITY);\n"
       "\tconst Lumix::Transform tr = world.getTransform(made);\n"
       "\tworld.setParent(parent, made);\n"
       "\tworld.destroyEntity(doomed);\n"
       "\tconst Lumix::EntityPtr none = Lumix::INVALID_ENTITY;\n"
       "\tbool ok = sync.edit(&doomed, 1, &made, &tr, 1, &parent, &made, 1);\n"
       "\tok = ok && sync.edit(nullptr, 0, nullptr, nullptr, 0, &none, &made, 1) && sync.entityCount() > (Lumix::u32)made.index;\n"
       "\tsync.setTransform(made, tr);\n"
       "\treturn ok && sync.propagate();\n"
       "}\n")

USE_PLUGIN = ('#include "mi355_plugin.cpp"\n'
              "void use(Lumix::Mi355Module& module, Lumix::World& world, Lumix::EntityPtr parent) {\n"
              "\tconst Lumix::EntityRef made = world.createEntity(Lumix::DVec3(1, 2, 3), Lumix::Quat::IDENTITY); // -> Mi355Module::onEntityCreated\n"
              "\tmodule.setParent(parent, made);\n"
              "\tmodule.setParent(Lumix::INVALID_ENTITY, made);\n"
              "\tworld.destroyEntity(made); // -> Mi355Module::onEntityDestroyed\n"
              "\tmodule.update(1.f / 60);\n"
              "\tmodule.markDirty();\n"
              "}\n")


def test_plugin_queue_compiles_against_reference_headers(ref_src, tmp_path):  # noqa: F811
    tu = tmp_path / "plugin_queue_tu.cpp"
    tu.write_text(USE_PLUGIN)
    cmd = ["g++"] + FLAGS + ["-I" + ref_src, "-I" + os.path.join(REF, "external"), "-I" + os.path.join(ROOT, "include"), "-I" + HOST, str(tu)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    src = open(os.path.join(HOST, "mi355_plugin.cpp")).read()
    assert "entityCreated().bind<&Mi355Module::onEntityCreated>" in src and "entityDestroyed().bind<&Mi355Module::onEntityDestroyed>" in src
    assert "m_queue.apply(*m_sync, m_world)" in src, "update() sends the queue through WorldSync::edit (world_edit_queue.h)"


def test_world_sync_edit_compiles_against_reference_headers(ref_src, tmp_path):  # noqa: F811
    tu = tmp_path / "world_sync_edit_tu.cpp"
    tu.write_text(USE)
    cmd = ["g++"] + FLAGS + ["-I" + ref_src, "-I" + os.path.join(REF, "external"), "-I" + os.path.join(ROOT, "include"), "-I" + HOST, str(tu)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
