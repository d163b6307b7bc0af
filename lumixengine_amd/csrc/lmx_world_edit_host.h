// lmx_world_edit_host.h — the host's side of lmx_world_edit: what it knows of the hierarchy without asking the device, and the check
// of a batch against it. Plain C++ (no HIP): tests/cpp/world_edit_host.cpp drives it alone under the sanitizers.
//
// The mirror is three 4-byte words per entity: `parent`, and two stamps that answer "is this entity alive" in O(depth) although
// destroying an entity takes its whole subtree along (the host never walks DOWN a tree: it has no child lists).
//   born[e]   - the edit that created e (1: the build), 0 once e itself was destroyed
//   linked[e] - the edit that last set parent[e]
// e is alive when none of its ancestors a (e included) has born[a] == 0 or was born after its child's link to it was made (it was
// destroyed and created again since, so the child went down with its first life). `parent` of a dead entity is stale until the index
// is created again.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <unordered_map>
#include <vector>

namespace lmx {

struct WorldEditMirror {
	std::vector<int32_t> parent; // by entity, -1 for roots
	std::vector<uint32_t> born, linked;
	uint32_t stamp = 1;
	uint32_t n() const { return (uint32_t)parent.size(); }

	void reset(const int32_t* p, uint32_t count) {
		parent.assign(p, p + count);
		born.assign(count, 1u);
		linked.assign(count, 1u);
		stamp = 1;
	}
	bool alive(int32_t e) const {
		if (e < 0 || (uint32_t)e >= n()) return false;
		for (int32_t a = e;;) {
			if (!born[a]) return false;
			const int32_t p = parent[a];
			if (p < 0) return true;
			if (born[p] > linked[a]) return false;
			a = p;
		}
	}
	// parent[] and 0 / 1 liveness as a fresh build would state them: dead entities are roots
	void resolve(std::vector<int32_t>* parent_out, std::vector<uint8_t>* alive_out) const {
		parent_out->assign(n(), -1);
		alive_out->assign(n(), 0);
		for (uint32_t e = 0; e < n(); ++e) {
			(*alive_out)[e] = alive((int32_t)e) ? 1 : 0;
			if ((*alive_out)[e]) (*parent_out)[e] = parent[e];
		}
	}
};

constexpr int32_t WORLD_EDIT_MAX_ENTITY = 1 << 28; // create_entity beyond this is refused (the range would grow to it)

struct WorldEditBatch {
	uint32_t n_destroy = 0, n_create = 0, n_reparent = 0;
	const int32_t* destroy_entity = nullptr;
	const int32_t* create_entity = nullptr;
	const int32_t* new_parent = nullptr;
	const int32_t* child = nullptr;
};

// What a batch changed in the mirror, for taking it back: world_edit_check_apply fills it, world_edit_rollback applies it (a refused
// batch inside the check; an accepted one when a later step of lmx_world_edit fails).
struct WorldEditUndo {
	struct Entry { int32_t e, parent; uint32_t born, linked; };
	std::vector<Entry> log;
	uint32_t n_before = 0, stamp_before = 0;
};
inline void world_edit_rollback(WorldEditMirror& m, const WorldEditUndo& u) {
	for (size_t k = u.log.size(); k-- > 0;) {
		const WorldEditUndo::Entry& x = u.log[k];
		if ((uint32_t)x.e >= u.n_before) continue;
		m.parent[x.e] = x.parent; m.born[x.e] = x.born; m.linked[x.e] = x.linked;
	}
	m.parent.resize(u.n_before); m.born.resize(u.n_before); m.linked.resize(u.n_before);
	m.stamp = u.stamp_before;
}

// Applies the batch to the mirror in World's order - every destroy, every create, the re-parentings in list order - checking each
// step against the state the steps before it left: range, liveness, duplicate creates, cycles. Returns nullptr and leaves the batch
// applied, or a message and the mirror exactly as it was. *which = the index of the offending list entry.
// reparent_child / reparent_parent: every re-parented child once, with its LAST parent of the list (what the device has to write).
// undo_out (optional): how to take an ACCEPTED batch back (world_edit_rollback).
inline const char* world_edit_check_apply(WorldEditMirror& m, const WorldEditBatch& b, std::vector<int32_t>* reparent_child, std::vector<int32_t>* reparent_parent,
	uint32_t* which, WorldEditUndo* undo_out = nullptr) {
	WorldEditUndo local_undo;
	WorldEditUndo& undo = undo_out ? *undo_out : local_undo;
	undo.log.clear();
	undo.n_before = m.n();
	undo.stamp_before = m.stamp;
	const uint32_t n_before = undo.n_before;
	auto touch = [&](int32_t e) { undo.log.push_back(WorldEditUndo::Entry{e, m.parent[e], m.born[e], m.linked[e]}); };
	auto refuse = [&](const char* why, uint32_t i) {
		world_edit_rollback(m, undo);
		undo.log.clear();
		*which = i;
		return why;
	};
	if ((b.n_destroy && !b.destroy_entity) || (b.n_create && !b.create_entity) || (b.n_reparent && (!b.new_parent || !b.child))) return refuse("null input array", 0);
	if (m.stamp == 0xffffffffu) { // the stamps wrapped: restate the mirror with fresh ones (alive entities keep their links, dead ones are dead roots)
		std::vector<int32_t> p;
		std::vector<uint8_t> a;
		m.resolve(&p, &a);
		m.parent.swap(p);
		for (uint32_t e = 0; e < m.n(); ++e) { m.born[e] = a[e]; m.linked[e] = 1; }
		m.stamp = 1;
		return world_edit_check_apply(m, b, reparent_child, reparent_parent, which, undo_out); // (no undo of the restatement: it states the same world)
	}
	const uint32_t now = ++m.stamp;
	// destroyEntity: alive before the call (a listed descendant of a listed entity is)
	for (uint32_t i = 0; i < b.n_destroy; ++i)
		if (!m.alive(b.destroy_entity[i])) return refuse("destroy_entity: not a live entity", i);
	for (uint32_t i = 0; i < b.n_destroy; ++i) {
		const int32_t e = b.destroy_entity[i];
		if (!m.born[e]) continue; // listed twice
		touch(e);
		m.born[e] = 0;
	}
	// createEntity: a dead index, or one beyond the range (the indices in between stay dead)
	for (uint32_t i = 0; i < b.n_create; ++i) {
		const int32_t e = b.create_entity[i];
		if (e < 0 || e >= WORLD_EDIT_MAX_ENTITY) return refuse("create_entity: out of range", i);
		if ((uint32_t)e >= m.n()) {
			m.parent.resize((size_t)e + 1, -1);
			m.born.resize((size_t)e + 1, 0u);
			m.linked.resize((size_t)e + 1, now);
		} else if (m.alive(e)) {
			return refuse("create_entity: the entity is alive (or listed twice)", i);
		}
		if ((uint32_t)e < n_before) touch(e);
		m.parent[e] = -1;
		m.born[e] = now;
		m.linked[e] = now;
	}
	// setParent, in list order
	for (uint32_t i = 0; i < b.n_reparent; ++i) {
		const int32_t c = b.child[i], p = b.new_parent[i];
		if (!m.alive(c)) return refuse("child: not a live entity", i);
		if (p >= 0 && !m.alive(p)) return refuse("new_parent: not a live entity", i);
		for (int32_t a = p; a >= 0; a = m.parent[a]) // "Hierarchy can not contain a cycle." (world.cpp:621-626)
			if (a == c) return refuse("re-parenting would close a cycle", i);
		if ((uint32_t)c < n_before) touch(c);
		m.parent[c] = p < 0 ? -1 : p;
		m.linked[c] = now;
	}
	reparent_child->clear();
	reparent_parent->clear();
	if (b.n_reparent) {
		std::unordered_map<int32_t, uint32_t> last;
		for (uint32_t i = 0; i < b.n_reparent; ++i) last[b.child[i]] = i;
		for (uint32_t i = 0; i < b.n_reparent; ++i)
			if (last[b.child[i]] == i) {
				reparent_child->push_back(b.child[i]);
				reparent_parent->push_back(b.new_parent[i] < 0 ? -1 : b.new_parent[i]);
			}
	}
	return nullptr;
}

} // namespace lmx
