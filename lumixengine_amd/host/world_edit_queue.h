// world_edit_queue.h — a frame's structural changes of a World (entityCreated / entityDestroyed delegates, re-parentings) folded into
// ONE batch for WorldSync::edit. The World holds the outcome, so the batch states outcomes, not the calls:
//   * an index is DESTROYED when the entity the mirror knows under it was destroyed, whatever happened to the index afterwards
//     (World::destroyEntity announces every descendant too, children first, world.cpp:524-529; an entity created this frame and
//     destroyed again never reaches the mirror);
//   * it is CREATED when an entity created this frame lives under it now, with the world transform it has now;
//   * a re-parented entity that still lives gets the parent it has now, in the order of the last re-parenting per entity.
// The batch applies in World's order - destroys, creates, re-parentings. A chain of re-parentings whose shortened form closes a cycle on
// the way is refused by the mirror: the caller then rebuilds it.
#pragma once

#include <vector>

#include "world_sync.h"

namespace Lumix {

struct WorldEditQueue {
	void created(EntityRef e) { m_events.push_back(Event{CREATED, e}); }
	void destroyed(EntityRef e) { m_events.push_back(Event{DESTROYED, e}); }
	void reparented(EntityRef e) { m_events.push_back(Event{REPARENTED, e}); }
	bool empty() const { return m_events.empty(); }
	void clear() { m_events.clear(); }

	// WorldT: hasEntity(EntityRef), getParent(EntityRef), getTransforms() - the World, or a test's stand-in. Empties the queue.
	template <typename WorldT> bool apply(WorldSync& sync, const WorldT& world) {
		enum : u8 { SEEN = 1, DESTROY = 2, CREATE = 4, MOVED = 8, KNOWN = 16 };
		m_destroyed.clear();
		m_created.clear();
		m_created_tr.clear();
		m_children.clear();
		m_parents.clear();
		u32 top = sync.entityCount();
		for (const Event& ev : m_events) top = (u32)ev.entity.index >= top ? (u32)ev.entity.index + 1 : top;
		m_state.assign(top, 0);
		for (const Event& ev : m_events) {
			u8& st = m_state[ev.entity.index];
			// the first event of an index says whether the mirror knows an entity under it: anything but CREATED means it does
			if (!(st & SEEN) && ev.kind != CREATED) st |= KNOWN;
			if (ev.kind == DESTROYED) {
				if (st & KNOWN) st |= DESTROY;
				st &= (u8)~(CREATE | MOVED);
			} else {
				st |= ev.kind == CREATED ? CREATE : MOVED;
			}
			st |= SEEN;
		}
		const Transform* transforms = world.getTransforms();
		for (u32 i = 0; i < top; ++i) {
			const u8 st = m_state[i];
			const EntityRef e{(i32)i};
			if (st & DESTROY) m_destroyed.push_back(e);
			if ((st & CREATE) && world.hasEntity(e)) {
				m_created.push_back(e);
				m_created_tr.push_back(transforms[i]);
			}
		}
		for (size_t k = m_events.size(); k-- > 0;) { // the last re-parenting of every entity that still lives, ...
			const Event& ev = m_events[k];
			u8& st = m_state[ev.entity.index];
			if (ev.kind != REPARENTED || !(st & MOVED)) continue;
			st &= (u8)~MOVED;
			if (!world.hasEntity(ev.entity)) continue;
			m_children.push_back(ev.entity);
			m_parents.push_back(world.getParent(ev.entity));
		}
		for (size_t a = 0, b = m_children.size(); a + 1 < b; ++a, --b) { // ... in call order
			const EntityRef c = m_children[a];
			m_children[a] = m_children[b - 1];
			m_children[b - 1] = c;
			const EntityPtr p = m_parents[a];
			m_parents[a] = m_parents[b - 1];
			m_parents[b - 1] = p;
		}
		m_events.clear();
		return sync.edit(m_destroyed.data(), (u32)m_destroyed.size(), m_created.data(), m_created_tr.data(), (u32)m_created.size(), m_parents.data(), m_children.data(),
			(u32)m_children.size());
	}

private:
	enum Kind : u8 { CREATED, DESTROYED, REPARENTED };
	struct Event { Kind kind; EntityRef entity; };
	std::vector<Event> m_events;
	std::vector<u8> m_state; // per entity index, while the events are folded
	std::vector<EntityRef> m_destroyed, m_created, m_children;
	std::vector<EntityPtr> m_parents;
	std::vector<Transform> m_created_tr;
};

} // namespace Lumix
