// run_world_sync_edit.cpp — drives WorldSync (lumixengine_amd/host/world_sync.h) through a scenario of staged writes, structural edits
// (WorldSync::edit: World::destroyEntity / createEntity / setParent of a frame as one batch) and propagations, the way mi355_plugin.cpp's
// module does - also with the batch folded from a frame's delegate calls by WorldEditQueue, as the module folds it -, and writes out what the mirror holds after every DUMP. tests/test_gpu_world_sync_edit_run.py writes the scenario and
// compares the dumps with the oracle's world.
//   run_world_sync_edit <scenario> <output>
#include "adapter_run.h"
#include "world_edit_queue.h"
#include "world_sync.h"

using namespace Lumix;
using namespace adapter_run;

enum Op : uint32_t { EDIT = 1, WRITE = 2, PROPAGATE = 3, DUMP = 4, QUEUE = 5 };

// the World after a frame of structural calls, as WorldEditQueue::apply asks it: the compat World plus the validity of every index
struct FrameWorld : World {
	std::vector<uint32_t> valid;
	bool hasEntity(EntityRef e) const { return e.index >= 0 && e.index < (i32)valid.size() && valid[e.index] != 0; }
};

int main(int argc, char** argv) {
	Reader in;
	Writer out;
	if (argc < 3 || !in.open(argv[1]) || !out.open(argv[2])) return EXIT_USAGE;
	LmxContext* ctx = nullptr;
	if (lmx_ctx_create(0, &ctx) != LMX_OK) { fprintf(stderr, "no device: %s\n", lmx_last_error(nullptr)); return EXIT_NO_DEVICE; }
	int rc = 0;
	{
		World world;
		const uint32_t n = in.get<uint32_t>();
		world.transforms = in.arr<Transform>(n);
		world.locals = in.arr<Transform>(n);
		world.parents = in.arr<i32>(n);
		WorldSync sync(ctx);
		if (!sync.build(world)) { fprintf(stderr, "WorldSync::build: %s\n", sync.lastError()); rc = EXIT_STEP; }
		while (rc == 0 && !in.done()) {
			const uint32_t op = in.get<uint32_t>();
			switch (op) {
				case EDIT: {
					const std::vector<i32> destroyed = in.arr<i32>(in.get<uint32_t>());
					const std::vector<i32> created = in.arr<i32>(in.get<uint32_t>());
					const std::vector<Transform> created_tr = in.arr<Transform>(created.size());
					const uint32_t n_reparented = in.get<uint32_t>();
					const std::vector<i32> parents = in.arr<i32>(n_reparented), children = in.arr<i32>(n_reparented);
					const bool want = in.get<uint32_t>() != 0;
					std::vector<EntityRef> d, c, k;
					std::vector<EntityPtr> p;
					for (i32 e : destroyed) d.push_back(EntityRef{e});
					for (i32 e : created) c.push_back(EntityRef{e});
					for (i32 e : children) k.push_back(EntityRef{e});
					for (i32 e : parents) p.push_back(EntityPtr{e});
					expect(sync.edit(d.data(), (u32)d.size(), c.data(), created_tr.data(), (u32)c.size(), p.data(), k.data(), (u32)k.size()), want, op, "edit", sync.lastError());
					break;
				}
				case QUEUE: { // a frame's delegate calls in order (0 created, 1 destroyed, 2 re-parented), then the World they left
					WorldEditQueue queue;
					const uint32_t n_events = in.get<uint32_t>();
					for (uint32_t i = 0; i < n_events; ++i) {
						const uint32_t kind = in.get<uint32_t>();
						const EntityRef e{in.get<i32>()};
						if (kind == 0) queue.created(e);
						else if (kind == 1) queue.destroyed(e);
						else queue.reparented(e);
					}
					FrameWorld after;
					const uint32_t count = in.get<uint32_t>();
					after.transforms = in.arr<Transform>(count);
					after.parents = in.arr<i32>(count);
					after.valid = in.arr<uint32_t>(count);
					const bool want = in.get<uint32_t>() != 0;
					expect(queue.apply(sync, after), want, op, "WorldEditQueue::apply", sync.lastError());
					expect(queue.empty(), true, op, "the queue is empty after apply", "");
					break;
				}
				case WRITE: {
					const uint32_t count = in.get<uint32_t>();
					const std::vector<i32> entity = in.arr<i32>(count);
					const std::vector<Transform> tr = in.arr<Transform>(count);
					const std::vector<uint32_t> world_space = in.arr<uint32_t>(count);
					for (uint32_t i = 0; i < count; ++i) {
						if (world_space[i]) sync.setTransform(EntityRef{entity[i]}, tr[i]);
						else sync.setLocalTransform(EntityRef{entity[i]}, tr[i]);
					}
					break;
				}
				case PROPAGATE: expect(sync.propagate(), true, op, "propagate", sync.lastError()); break;
				case DUMP: {
					const u32 count = sync.entityCount();
					std::vector<Transform> tr(count), local(count), moved_tr;
					std::vector<int32_t> moved;
					expect(sync.readTransforms(tr.data(), count) && sync.readLocalTransforms(local.data(), count), true, op, "read", sync.lastError());
					expect(sync.readMoved(moved, moved_tr), true, op, "readMoved", sync.lastError());
					out.counted(tr, count);
					out.arr(local.data(), count);
					out.counted(moved, moved.size());
					break;
				}
				default: fprintf(stderr, "scenario: unknown op %u\n", op); rc = EXIT_SCENARIO;
			}
		}
	}
	lmx_ctx_destroy(ctx);
	out.close();
	if (rc == 0) printf("world sync edit ok\n");
	return rc;
}
