// animcomp_kernels.hip — the animation clip writer on the device (ModelImporter::writeAnimations, renderer/editor/model_importer.cpp:1508-1754)
// for a batch of clips. The arithmetic is lmx_animcomp.h's, shared with the host; FMA-free (-ffp-contract=off). No kernel uses scratch.
//
// Keys are the ABI's 28-byte records, sample-major and bones-minor: a clip is a matrix of n_samples rows of n_bones * 7 floats, a column is
// one channel of one bone. Both passes over the keys walk rows with consecutive lanes on consecutive floats.
//
//   k_animcomp_ranges  one workgroup per (clip, chunk of AC_RANGE_SAMPLES samples). A thread folds one column over a run of samples in sample
//                      order; a clip of few bones puts 256 / columns threads on each column, each on its own run of the chunk, and joins
//                      their folds in run order in LDS. The fold is the reference's (the earlier sample stays on a tie), a join of runs in
//                      order is the same fold, so the sign of a zero minimum is the sequential one. One partial per (chunk, column).
//   k_animcomp_layout  one workgroup per clip, one thread per bone: joins the bone's partials in chunk order, derives its bit sizes and what
//                      it refuses the clip with, then two block scans (lmx_wave.h) give every bone its place in the four tables and its
//                      offset_bits; writes the records in bone order, the pack's tracks and the clip's info.
//   k_animcomp_pack    one workgroup per run of groups of 32 frames of one stream of one clip. 32 frames are frame_size_bits dwords whatever
//                      the frame size: the group is cleared in LDS, every (frame, track) entry is packed by one thread and set with up to
//                      three LDS atomic ORs (an entry of 57 bits at bit 31 spans three dwords), and the group goes out as whole dwords,
//                      consecutive lanes on consecutive dwords. The last, short group writes its zero tail. ORs commute: the bytes are the
//                      same from run to run, and no global atomic touches a stream.
#include <hip/hip_runtime.h>

#include "lmx_animcomp.h"
#include "lmx_wave.h"

namespace lmx {

namespace {

// column j of the clip's rows s0 .. s1 - 1, in sample order
__device__ __forceinline__ AcRange fold_column(const float* __restrict__ rows, uint32_t width, uint32_t j, uint32_t s0, uint32_t s1, const float* __restrict__ bind) {
	AcRange r = ac_range_identity();
	const uint32_t bone = j / 7u, ch = j - bone * 7u;
	if (ch < 3) {
		const float at = bind[3 * bone + ch];
		for (uint32_t s = s0; s < s1; ++s) ac_range_add_pos(r, rows[(size_t)s * width + j], at);
	} else {
		for (uint32_t s = s0; s < s1; ++s) ac_range_add(r, rows[(size_t)s * width + j]);
	}
	return r;
}

__global__ __launch_bounds__(AC_BLOCK) void k_animcomp_ranges(AcBatch B, const AcRangeItem* __restrict__ items) {
	__shared__ AcRange s_part[AC_BLOCK];
	const uint32_t tid = threadIdx.x;
	const AcRangeItem it = items[blockIdx.x];
	const AcClip c = B.clips[it.clip];
	const uint32_t width = c.n_bones * 7u, s0 = it.chunk * AC_RANGE_SAMPLES;
	const uint32_t s1 = c.n_samples - s0 < AC_RANGE_SAMPLES ? c.n_samples : s0 + AC_RANGE_SAMPLES;
	const float* __restrict__ rows = B.keys + c.key_off * 7u;
	const float* __restrict__ bind = B.bind + 3 * (size_t)c.bone_off;
	AcRange* __restrict__ out = B.partials + c.part_off + (size_t)it.chunk * width;
	if (width * 2u <= AC_BLOCK) { // (block-uniform) several threads per column, each on its own run of the chunk's samples
		const uint32_t runs = AC_BLOCK / width, per = (s1 - s0 + runs - 1) / runs;
		const uint32_t run = tid / width, j = tid - run * width;
		AcRange r = ac_range_identity();
		if (run < runs) {
			const uint32_t a = s0 + run * per, b = a + per < s1 ? a + per : s1;
			r = fold_column(rows, width, j, a, b, bind); // (a >= s1: an empty run)
		}
		s_part[tid] = r;
		__syncthreads();
		if (tid < width) {
			for (uint32_t k = 1; k < runs; ++k) ac_range_join(r, s_part[k * width + tid]);
			out[tid] = r;
		}
	} else {
		for (uint32_t j = tid; j < width; j += AC_BLOCK) out[j] = fold_column(rows, width, j, s0, s1, bind);
	}
}

__global__ __launch_bounds__(AC_BLOCK) void k_animcomp_layout(AcBatch B) {
	__shared__ uint32_t s_wave[AC_BLOCK / 64];
	__shared__ uint32_t s_code;
	const uint32_t tid = threadIdx.x, clip = blockIdx.x;
	const AcClip c = B.clips[clip];
	const uint32_t width = c.n_bones * 7u, chunks = (c.n_samples + AC_RANGE_SAMPLES - 1) / AC_RANGE_SAMPLES;
	const uint32_t clip_code = ac_clip_code(c.n_samples, c.t_error, c.r_error);
	if (tid == 0) s_code = clip_code ? clip_code : 0xffffffffu;
	__syncthreads();
	const bool keyed = !clip_code && tid < c.n_bones && B.has_keys[c.bone_off + tid] != 0;
	AcRange r[7];
	AcBone L;
	L.t_kind = L.r_kind = AC_NONE;
	L.t_entry = L.r_entry = 0;
	if (keyed) {
		const AcRange* __restrict__ part = B.partials + c.part_off + tid * 7u;
#pragma unroll
		for (int ch = 0; ch < 7; ++ch) r[ch] = part[ch];
		for (uint32_t k = 1; k < chunks; ++k) {
#pragma unroll
			for (int ch = 0; ch < 7; ++ch) ac_range_join(r[ch], part[(size_t)k * width + ch]);
		}
		const float* bind = B.bind + 3 * (size_t)(c.bone_off + tid);
		const float at[3] = {bind[0], bind[1], bind[2]};
		L = ac_bone_layout(r, at, c.t_error, c.r_error);
		if (L.code) atomicMin(&s_code, L.code);
	}
	// a bone's place in each of the four tables (four counts of at most 196 in one word) and its two offsets (two sums below 2^16)
	const uint32_t kinds = (L.t_kind == AC_CONST ? 1u : 0u) | (L.t_kind == AC_ANIMATED ? 1u << 8 : 0u) | (L.r_kind == AC_CONST ? 1u << 16 : 0u) | (L.r_kind == AC_ANIMATED ? 1u << 24 : 0u);
	const uint32_t entries = (L.t_kind == AC_ANIMATED ? L.t_entry : 0u) | (L.r_kind == AC_ANIMATED ? L.r_entry << 16 : 0u);
	uint32_t all_kinds, all_entries;
	const uint32_t place = block_scan<true>(kinds, AC_BLOCK / 64, 0u, s_wave, &all_kinds, Sum());
	const uint32_t offsets = block_scan<true>(entries, AC_BLOCK / 64, 0u, s_wave, &all_entries, Sum()); // (the first scan's barriers order s_code too)
	uint32_t code = s_code == 0xffffffffu ? 0u : s_code;
	const uint32_t t_frame = all_entries & 0xffffu, r_frame = all_entries >> 16;
	if (!code && (t_frame > AC_MAX_FRAME_BITS || r_frame > AC_MAX_FRAME_BITS)) code = LMX_ANIMCOMP_FRAME_BITS; // (never with 196 bones of 57 bits)
	if (tid == 0) {
		LmxAnimCompInfo info;
		memset(&info, 0, sizeof(info));
		info.frame_count = c.n_samples ? c.n_samples - 1 : 0;
		info.status = code;
		if (!code) {
			info.n_const_translations = all_kinds & 0xffu, info.n_translations = (all_kinds >> 8) & 0xffu;
			info.n_const_rotations = (all_kinds >> 16) & 0xffu, info.n_rotations = all_kinds >> 24;
			info.translations_frame_size_bits = t_frame, info.rotations_frame_size_bits = r_frame;
			info.translation_stream_size = ((uint64_t)t_frame * c.n_samples + 7) / 8;
			info.rotation_stream_size = ((uint64_t)r_frame * c.n_samples + 7) / 8;
		}
		B.infos[clip] = info;
	}
	if (code || !keyed) return;
	const float* __restrict__ first = B.keys + (c.key_off * 7u + tid * 7u);
	if (L.t_kind == AC_CONST) {
		LmxAnimConstTranslation rec;
		rec.value[0] = first[0], rec.value[1] = first[1], rec.value[2] = first[2];
		rec.bone_index = (uint16_t)tid, rec._pad = 0;
		B.ct[c.bone_off + (place & 0xffu)] = rec;
	} else if (L.t_kind == AC_ANIMATED) {
		const uint32_t at = c.bone_off + ((place >> 8) & 0xffu);
		LmxAnimTranslationTrack rec;
		AcTrack track;
		ac_translation_records(r, L, tid, offsets & 0xffffu, &rec, &track);
		B.tt[at] = rec;
		B.t_tracks[at] = track;
	}
	if (L.r_kind == AC_CONST) {
		LmxAnimConstRotation rec;
		rec.value[0] = first[3], rec.value[1] = first[4], rec.value[2] = first[5], rec.value[3] = first[6];
		rec.bone_index = (uint16_t)tid, rec._pad = 0;
		B.cr[c.bone_off + ((place >> 16) & 0xffu)] = rec;
	} else if (L.r_kind == AC_ANIMATED) {
		const uint32_t at = c.bone_off + (place >> 24);
		LmxAnimRotationTrack rec;
		AcTrack track;
		ac_rotation_records(r, L, tid, offsets >> 16, &rec, &track);
		B.rt[at] = rec;
		B.r_tracks[at] = track;
	}
}

__global__ __launch_bounds__(AC_BLOCK) void k_animcomp_pack(AcBatch B, const AcPackItem* __restrict__ items, uint32_t* __restrict__ t_stream, uint32_t* __restrict__ r_stream) {
	__shared__ uint32_t s_words[AC_GROUP_WORDS];
	const uint32_t tid = threadIdx.x;
	const AcPackItem it = items[blockIdx.x];
	const AcClip c = B.clips[it.clip];
	const LmxAnimCompInfo info = B.infos[it.clip];
	const bool rotation = it.rotation != 0;
	const uint32_t n_tracks = rotation ? info.n_rotations : info.n_translations;
	const uint32_t frame_bits = rotation ? info.rotations_frame_size_bits : info.translations_frame_size_bits;
	if (info.status || n_tracks == 0 || frame_bits == 0 || frame_bits > AC_GROUP_WORDS) return; // (block-uniform; the host makes no such item)
	const AcTrack* __restrict__ tracks = (rotation ? B.r_tracks : B.t_tracks) + c.bone_off;
	const float* __restrict__ rows = B.keys + c.key_off * 7u + (rotation ? 3u : 0u);
	uint32_t* __restrict__ out = (rotation ? r_stream : t_stream) + it.out_word;
	const uint64_t total_words = ((uint64_t)frame_bits * c.n_samples + 31) / 32;
	for (uint32_t g = it.group0; g < it.group0 + it.n_groups; ++g) {
		const uint32_t f0 = g * AC_GROUP_FRAMES;
		if (f0 >= c.n_samples) break;
		for (uint32_t w = tid; w < frame_bits; w += AC_BLOCK) s_words[w] = 0;
		__syncthreads();
		const uint32_t frames = c.n_samples - f0 < AC_GROUP_FRAMES ? c.n_samples - f0 : AC_GROUP_FRAMES;
		for (uint32_t e = tid; e < frames * n_tracks; e += AC_BLOCK) {
			const uint32_t f = e / n_tracks, k = e - f * n_tracks;
			const AcTrack t = tracks[k];
			const float* key = rows + ((size_t)(f0 + f) * c.n_bones + t.bone) * 7u;
			const uint64_t v = rotation ? ac_pack_rotation(key, t) : ac_pack_translation(key, t);
			const uint32_t at = f * frame_bits + t.offset_bits, w = at >> 5, sh = at & 31u;
			const uint32_t lo = (uint32_t)(v << sh), mid = (uint32_t)(v >> (32u - sh)), hi = sh ? (uint32_t)(v >> (64u - sh)) : 0u;
			if (lo) atomicOr(&s_words[w], lo);
			if (mid && w + 1 < frame_bits) atomicOr(&s_words[w + 1], mid);
			if (hi && w + 2 < frame_bits) atomicOr(&s_words[w + 2], hi);
		}
		__syncthreads();
		// (a thread stores the words it clears: no barrier is needed before the next group's clear)
		for (uint32_t w = tid; w < frame_bits; w += AC_BLOCK) {
			const uint64_t gw = (uint64_t)g * frame_bits + w;
			if (gw < total_words) out[gw] = s_words[w];
		}
	}
}

} // namespace

hipError_t launch_animcomp_ranges(hipStream_t s, const AcBatch& batch, const AcRangeItem* items, uint32_t n_items) {
	if (!batch.clips || !batch.keys || !batch.bind || !batch.partials || (n_items && !items)) return hipErrorInvalidValue;
	if (n_items == 0) return hipSuccess; // (every clip without samples)
	hipLaunchKernelGGL(k_animcomp_ranges, dim3(n_items), dim3(AC_BLOCK), 0, s, batch, items);
	return hipGetLastError();
}

hipError_t launch_animcomp_layout(hipStream_t s, const AcBatch& batch, uint32_t n_clips) {
	if (!batch.clips || !batch.keys || !batch.bind || !batch.has_keys || !batch.partials || !batch.infos || !batch.ct || !batch.tt || !batch.cr || !batch.rt || !batch.t_tracks || !batch.r_tracks || n_clips == 0)
		return hipErrorInvalidValue;
	hipLaunchKernelGGL(k_animcomp_layout, dim3(n_clips), dim3(AC_BLOCK), 0, s, batch);
	return hipGetLastError();
}

hipError_t launch_animcomp_pack(hipStream_t s, const AcBatch& batch, const AcPackItem* items, uint32_t n_items, uint32_t* t_stream, uint32_t* r_stream) {
	if (n_items == 0) return hipSuccess; // (no animated track in the batch)
	if (!batch.clips || !batch.keys || !batch.infos || !batch.t_tracks || !batch.r_tracks || !items || !t_stream || !r_stream) return hipErrorInvalidValue;
	hipLaunchKernelGGL(k_animcomp_pack, dim3(n_items), dim3(AC_BLOCK), 0, s, batch, items, t_stream, r_stream);
	return hipGetLastError();
}

} // namespace lmx
