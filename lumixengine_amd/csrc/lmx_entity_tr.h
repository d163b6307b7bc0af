// lmx_entity_tr.h — World::getTransforms()[e] as the device passes read it (draw_kernels.hip, cluster_kernels.hip): the array
// lmx_draw_set_transforms uploaded, or the propagated world hierarchy in place through slot_of_entity. An entity neither covers
// reads as zero. `D` is the pass's device struct: it carries tr / n_tr and wpx .. wsz / slot_of_entity / n_world under these names.
#pragma once

#include "lmx_kernels.h"

namespace lmx {

struct DrawTr { double px, py, pz; uint32_t rot[4]; uint32_t scale[3]; };

__device__ __forceinline__ DrawTr load_uploaded(const LmxTransform* t, uint32_t n, uint32_t e) {
	DrawTr r;
	r.px = r.py = r.pz = 0.0;
	r.rot[0] = r.rot[1] = r.rot[2] = r.rot[3] = 0;
	r.scale[0] = r.scale[1] = r.scale[2] = 0;
	if (t && e < n) {
		const LmxTransform* p = t + e;
		r.px = p->pos[0]; r.py = p->pos[1]; r.pz = p->pos[2];
		const uint32_t* w = reinterpret_cast<const uint32_t*>(p->rot);
		for (int k = 0; k < 4; ++k) r.rot[k] = w[k];
		for (int k = 0; k < 3; ++k) r.scale[k] = w[4 + k];
	}
	return r;
}
// transforms[e]: the uploaded array, or the propagated world in place
template <typename D> __device__ __forceinline__ DrawTr load_tr(const D& d, uint32_t e) {
	if (d.tr) return load_uploaded(d.tr, d.n_tr, e);
	DrawTr r = load_uploaded(nullptr, 0, 0);
	if (e < d.n_world) {
		const int32_t slot = d.slot_of_entity[e];
		if (slot >= 0) {
			r.px = d.wpx[slot]; r.py = d.wpy[slot]; r.pz = d.wpz[slot];
			const uint4 q = reinterpret_cast<const uint4*>(d.wrot)[slot];
			r.rot[0] = q.x; r.rot[1] = q.y; r.rot[2] = q.z; r.rot[3] = q.w;
			r.scale[0] = __float_as_uint(d.wsx[slot]); r.scale[1] = __float_as_uint(d.wsy[slot]); r.scale[2] = __float_as_uint(d.wsz[slot]);
		}
	}
	return r;
}

} // namespace lmx
