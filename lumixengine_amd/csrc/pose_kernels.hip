// pose_kernels.hip — PoseProcessor (renderer/pipeline.cpp:3730-3787) on the device: the model instances lmx_keys_run handed over are
// packed back to back into the frame's transient dual-quaternion buffer (offset += pose->count * sizeof(DualQuat)), every instance's part
// is filled as computeSkeletonDualQuats fills it (:2680-2745: toDualQuat(absolute pose[b] * inverse bind[b]), skin_dual_quat of lmx_math.h,
// FMA-free) and pose->slice {bindless handle, byte offset} lands in the entity-indexed tables k_draw_encode writes into the skinned records.
//
// The list and its length stay on the device: every launch has a FIXED grid whose blocks / waves stride over the list, nothing is sized
// from a read-back. Three steps:
//   k_pose_sizes    entity -> skin instance -> n_bones per list entry (one 16-byte record each), the bytes of every block's part of the list
//   k_pose_offsets  exclusive prefix of 32 * n_bones in list order (block scan with carry, the blocks' bases from the sums of step 1) on top
//                   of the frame's cursor; the slice tables by entity; cursor and counters (one non-returning atomic per block and counter)
//   k_pose_dual_quats  one WAVE per listed instance, one lane per bone: 12 + 16 B of pose, 12 + 16 B of inverse bind in, 32 B out. A
//                   skeleton's bones are consecutive in the pose arrays and in the slice, so a wave's loads and its stores are contiguous
//                   runs without a search in the prefix (a flat bone index needs one per lane); a skeleton under 64 bones leaves lanes idle,
//                   which costs issue slots of a kernel that waits for memory.
// Sums saturate at 2^32 - 1: a slice that would start or end there lies past any buffer (its size is checked against 32-bit offsets).
#include "lmx_kernels.h"
#include "lmx_wave.h"

namespace lmx {

namespace {

constexpr uint32_t POSE_NONE = 0xffffffffu;

// block b's part of the list (list_length(d) entries): whole tiles of POSE_BLOCK entries
__device__ __forceinline__ uint32_t part_length(uint32_t n) {
	const uint32_t per = (n + POSE_GRID - 1) / POSE_GRID;
	return (per + POSE_BLOCK - 1) / POSE_BLOCK * POSE_BLOCK;
}

// Exclusive saturating prefix of v in thread order; *total = the block's sum. s_wave: one word per wave.
__device__ __forceinline__ uint32_t block_scan_sum(uint32_t v, uint32_t* s_wave, uint32_t* total) {
	return block_scan<true>(v, POSE_BLOCK / 64, 0u, s_wave, total, SatAdd());
}

// Step 1. entries[i] = {entity, first bone in the pose arrays, n_bones, first bone of the model's inverse bind}; y = POSE_NONE: no skin instance.
__global__ __launch_bounds__(POSE_BLOCK) void k_pose_sizes(PosesDevice d) {
	__shared__ uint32_t s_wave[POSE_BLOCK / 64];
	const uint32_t n = list_length(d), per = part_length(n);
	const uint32_t begin = blockIdx.x * per, end = begin + per < n ? begin + per : n; // (list_cap <= 2^31: no wrap)
	uint32_t bytes = 0;
	for (uint32_t base = begin; base < end; base += POSE_BLOCK) {
		const uint32_t i = base + threadIdx.x;
		if (i >= end) continue;
		const int32_t e = d.list[i];
		int32_t si = -1;
		if (e >= 0 && (uint32_t)e < d.n_entities) si = d.skin_of_entity[e];
		uint4 rec = make_uint4((uint32_t)e, POSE_NONE, 0u, 0u);
		if (si >= 0 && (uint32_t)si < d.n_inst) {
			const SkinInstance& in = d.inst[si];
			rec.y = in.bone_offset; rec.z = in.n_bones; rec.w = in.model_offset;
			bytes = sat_add(bytes, in.n_bones * POSE_BONE_BYTES);
		}
		d.entries[i] = rec;
	}
	uint32_t total;
	(void)block_scan_sum(bytes, s_wave, &total);
	if (threadIdx.x == 0) {
		d.block_sum[blockIdx.x] = total;
		// the cursor this run starts from, set aside: step 2's blocks read it while their first one already advances the cursor itself
		if (blockIdx.x == 0) d.state[POSES_BASE] = d.state[POSES_BYTES];
	}
}

// Step 2.
__global__ __launch_bounds__(POSE_BLOCK) void k_pose_offsets(PosesDevice d) {
	__shared__ uint32_t s_wave[POSE_BLOCK / 64];
	__shared__ uint32_t s_base;
	static_assert(POSE_GRID == POSE_BLOCK, "one thread per block sum");
	const uint32_t n = list_length(d), per = part_length(n);
	const uint32_t begin = blockIdx.x * per, end = begin + per < n ? begin + per : n;
	uint32_t total;
	const uint32_t before = block_scan_sum(d.block_sum[threadIdx.x], s_wave, &total);
	if (threadIdx.x == blockIdx.x) s_base = sat_add(d.state[POSES_BASE], before);
	__syncthreads();
	uint32_t carry = s_base;
	uint32_t taken = 0, taken_bytes = 0, skipped = 0, overflow = 0; // this thread's entries
	for (uint32_t base = begin; base < end; base += POSE_BLOCK) { // (block-uniform bounds: every thread takes every barrier)
		const uint32_t i = base + threadIdx.x;
		uint4 rec = make_uint4(0u, POSE_NONE, 0u, 0u);
		if (i < end) rec = d.entries[i];
		const bool skinned = rec.y != POSE_NONE;
		const uint32_t size = skinned ? rec.z * POSE_BONE_BYTES : 0u;
		uint32_t tile;
		const uint32_t start = sat_add(carry, block_scan_sum(size, s_wave, &tile));
		carry = sat_add(carry, tile);
		if (i >= end) continue;
		if (!skinned) {
			++skipped;
			continue;
		}
		if (sat_add(start, size) > d.cap_bytes) { // the reservation would pass the end: nothing is written, and nothing behind it fits either
			overflow = 1;
			d.entries[i].y = POSE_NONE;
			continue;
		}
		d.entries[i].x = start;
		if (rec.x < d.n_table) { // pose->slice of the entity (pipeline.cpp:3176-3180)
			d.bones_handle[rec.x] = d.handle;
			d.bones_offset[rec.x] = d.base_offset + start;
		}
		++taken;
		taken_bytes += size;
	}
	uint32_t n_taken, n_bytes, n_skipped, any_overflow; // (the accepted bytes of a run fit the buffer: no saturation)
	(void)block_scan_sum(taken, s_wave, &n_taken);
	(void)block_scan_sum(taken_bytes, s_wave, &n_bytes);
	(void)block_scan_sum(skipped, s_wave, &n_skipped);
	(void)block_scan_sum(overflow, s_wave, &any_overflow);
	if (threadIdx.x == 0) { // results nobody waits for: the adds return nothing
		if (n_taken) (void)atomicAdd(&d.state[POSES_INSTANCES], n_taken);
		if (n_bytes) (void)atomicAdd(&d.state[POSES_BYTES], n_bytes);
		if (n_skipped) (void)atomicAdd(&d.state[POSES_SKIPPED], n_skipped);
		if (any_overflow) (void)atomicOr(&d.state[POSES_OVERFLOW], 1u);
	}
}

// Step 3. A lane's two 16-byte stores are the 32 contiguous bytes of its bone's DualQuat {r, d} (core/math.h:257-260).
__global__ __launch_bounds__(POSE_BLOCK) void k_pose_dual_quats(PosesDevice d) {
	const uint32_t n = list_length(d);
	const uint32_t lane = threadIdx.x & 63u, n_waves = gridDim.x * (POSE_BLOCK / 64);
	for (uint32_t i = blockIdx.x * (POSE_BLOCK / 64) + (threadIdx.x >> 6); i < n; i += n_waves) {
		const uint4 rec = d.entries[i]; // wave-uniform
		if (rec.y == POSE_NONE) continue;
		float4* out = d.dual_quats + (rec.x >> 4);
		for (uint32_t b = lane; b < rec.z; b += 64) {
			const float* pp = d.pose_pos + ((size_t)rec.y + b) * 3;
			const float* ip = d.inv_pos + ((size_t)rec.w + b) * 3;
			const float4 pr = d.pose_rot[(size_t)rec.y + b], ir = d.inv_rot[(size_t)rec.w + b];
			const DualQ dq = skin_dual_quat(V3{pp[0], pp[1], pp[2]}, Q4{pr.x, pr.y, pr.z, pr.w}, V3{ip[0], ip[1], ip[2]}, Q4{ir.x, ir.y, ir.z, ir.w});
			out[2 * b] = make_float4(dq.r.x, dq.r.y, dq.r.z, dq.r.w);
			out[2 * b + 1] = make_float4(dq.d.x, dq.d.y, dq.d.z, dq.d.w);
		}
	}
}

} // namespace

hipError_t launch_pose_slices(hipStream_t s, const PosesDevice& d) {
	hipLaunchKernelGGL(k_pose_sizes, dim3(POSE_GRID), dim3(POSE_BLOCK), 0, s, d);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(k_pose_offsets, dim3(POSE_GRID), dim3(POSE_BLOCK), 0, s, d);
	return hipGetLastError();
}

hipError_t launch_pose_dual_quats(hipStream_t s, const PosesDevice& d) {
	hipLaunchKernelGGL(k_pose_dual_quats, dim3(POSE_DQ_GRID), dim3(POSE_BLOCK), 0, s, d);
	return hipGetLastError();
}

} // namespace lmx
