// Table-gradient scatter, PER-CORNER RECORD LISTS (rounds 2-3): the workspace path of fp16 dL/dy (ngp_fox.py) and of every level table the record regions
// (hash_bwd_regions.h) cannot take.  Launched by launch_percorner (hash_encode.hip).
#pragma once
#include "hash_bwd_common.h"

// ---------------------------------------------------------------------------------------------------------------- binned scatter (every level of up to 2^19 entries)
// (Rounds 1-2 scattered through an owner-computes scan - every slice owner re-deriving every sample's indices, VALU-bound at ~0.45 ms per 2^18-sample batch; deleted in
// round 5.)  With a workspace the levels take this two-phase path:
//   A  records: the eight (entry, weight*gradient) contributions of a (sample, level) are computed ONCE and appended to the record list of the bin the
//      entry lives in (64 bins per level).  Slots are handed out by an LDS histogram per workgroup plus ONE global integer atomic per
//      (workgroup, bin) — ~10^5 global atomics per batch instead of 3*10^7.
//        k_bin_records       (fine levels)   one thread per (sample, level);
//        k_bin_records_runs  (coarse levels, **r2b**) one thread per EIGHT CONSECUTIVE samples: the samples of a ray are consecutive in the batch and a cell of a
//                            level with res <= 300 is 3-40 marching steps long, so the thread sums the runs that share a cell in registers and emits one set of
//                            eight records per run - 2.2 instead of 10 levels' worth of records on the ngp_base.py batch, and the dense levels (whose whole
//                            table is a few thousand entries hit by 2 M contributions) fit the same machinery: no owner-computes scan, no partial slabs.
//   B  k_bin_accumulate: one workgroup per bin streams its records (coalesced reads) into 64-bit INTEGER accumulators in LDS
//      (ds_add_u64: 16.6 cycles per wave instruction vs 194 for ds_add_f32) and writes the bin's entries of the gradient with plain stores.
// A record is a 16-bit slot inside the bin plus the contribution, kept as two streams (structure of arrays: 2 + 4 bytes for fp16 gradients on the fine levels,
// 2 + 8 for fp32 and for every run record - the 8-byte {u32 index, half2} records of round 1 moved a third more bytes).
//   fp16 dL/dy, fine levels: the contribution is stored as fp16 after scaling by the power of two that maps the level's max |dL/dy| into [2^13, 2^14): every
//     fp16 value is a multiple of 2^-24, so value * 2^24 is an exact integer < 2^39 and the sum of up to 2^21 records cannot overflow 63 bits.  Each contribution
//     is rounded once (2^-11 relative, like the `(__half)(grad*weight)` of HashEncode.h:345).
//   fp32 records (fp32 dL/dy - ngp_base.py - and all run records): converted to fixed point at 2^38 / max|dL/dy| (a 64-bit sum per feature): fp32-exact for every
//     contribution within 2^-14 of the level's largest, and still 2^-10-relative 14 binades further down.
// In both cases the accumulation itself is EXACT and order-independent => bit-reproducible gradients (the reference's atomics round after every add, in
// random order; the run sums are fp32 sums in sample order inside one thread: deterministic too).  A bin that overflows its record capacity (pathological
// clustering) spills to one shared list that the bin's owner scans before it writes - no float atomics anywhere, still deterministic, just slow in that corner.
// (The bins' constants, BinPlan, LevelSel and SpillEntry are shared with the region path: hash_bwd_common.h.)

// entry -> (bin, slot inside the bin).  A full 2^19-entry hashed level: bin = the entry's 8192-entry slice (pseudo-random entries: balanced; contiguous write-out).
// Any smaller level (the dense levels, small hashed tables): groups of 8 entries are dealt round-robin to the 64 bins, so the spatially coherent dense indices
// (x + y*res + z*res^2: a batch lives in a few z-slabs) spread evenly as well.
__device__ __forceinline__ uint32_t bin_of(uint32_t e, bool il) { return il ? (e >> 3) & 63u : e >> BIN_BITS; }
__device__ __forceinline__ uint32_t local_of(uint32_t e, bool il) { return il ? ((e >> 9) << 3) | (e & 7u) : e & (BIN_ENTRIES - 1u); }
__device__ __forceinline__ uint32_t entry_of(uint32_t bin, uint32_t local, bool il) { return il ? ((local >> 3) << 9) | (bin << 3) | (local & 7u) : (bin << BIN_BITS) | local; }
// record streams of (binned level hl, bin): every level owns 64 * cap * 8 bytes of the value area whatever its record type
// (cap = capacity of ONE sub-list; list = bin * CUR_SUBS + sub)
template <typename RV> __device__ __forceinline__ RV *rec_val_at(void *base, uint32_t hl, uint32_t list, uint32_t cap) {
	return reinterpret_cast<RV *>(reinterpret_cast<char *>(base) + (size_t)hl * BINS_PER_LEVEL * CUR_SUBS * cap * 8u) + (size_t)list * cap;
}
__device__ __forceinline__ uint16_t *rec_idx_at(uint16_t *base, uint32_t hl, uint32_t list, uint32_t cap) { return base + ((size_t)hl * BINS_PER_LEVEL * CUR_SUBS + list) * cap; }
// Reading a bin back: its eight sub-lists laid end to end in units of K records (`groups`) plus the < K leftover records of every sub-list (`tails`).
struct SubLists { uint32_t cnt[CUR_SUBS], gstart[CUR_SUBS + 1], tstart[CUR_SUBS + 1]; bool over; };
__device__ __forceinline__ SubLists sub_lists(const uint32_t *__restrict__ cur /* the bin's CUR_SUBS cursors */, uint32_t cap, uint32_t K) {
	SubLists m; m.over = false; m.gstart[0] = 0u; m.tstart[0] = 0u;
#pragma unroll
	for (uint32_t k = 0; k < CUR_SUBS; ++k) {
		const uint32_t raw = cur[k];
		m.over |= raw > cap;
		m.cnt[k] = min(raw, cap);
		m.gstart[k + 1] = m.gstart[k] + m.cnt[k] / K;
		m.tstart[k + 1] = m.tstart[k] + m.cnt[k] % K;
	}
	return m;
}
// flat group index r -> index into the bin's sub-list layout in units of K records (sub-list k begins k * gcap groups in); static indexing only (the tables stay in registers)
__device__ __forceinline__ uint32_t sub_group(const SubLists &m, uint32_t r, uint32_t gcap) {
	uint32_t k = 0, s0 = 0;
#pragma unroll
	for (uint32_t j = 1; j < CUR_SUBS; ++j) if (r >= m.gstart[j]) { k = j; s0 = m.gstart[j]; }
	return k * gcap + (r - s0);
}
// flat leftover index t -> record index in the bin's sub-list layout (sub-list k begins k * cap records in, its leftovers follow its cnt / K * K grouped records)
__device__ __forceinline__ uint32_t sub_tail(const SubLists &m, uint32_t t, uint32_t cap, uint32_t K) {
	uint32_t k = 0, s0 = 0, full = m.cnt[0] / K * K;
#pragma unroll
	for (uint32_t j = 1; j < CUR_SUBS; ++j) if (t >= m.tstart[j]) { k = j; s0 = m.tstart[j]; full = m.cnt[j] / K * K; }
	return k * cap + full + (t - s0);
}

// Records are staged in LDS grouped by bin and written out run by run: a wave then stores 64 consecutive records (full lines) instead of 64
// scattered words.  The scattered version was bound by the L2 request rate (2.4e7 partial-line writes ~ one per clock per channel), not by bytes.
template <typename T> struct RecVal;
template <> struct RecVal<__half> { using type = __half2; };
template <> struct RecVal<float> { using type = float2; };
// 512 samples per workgroup: 33 KiB (fp16) / 49 KiB (fp32) of LDS, so 3-4 workgroups share a CU and one workgroup's serial phases (loads -> LDS histogram -> the
// wave-0 reservation with its global atomics -> staging -> copy-out, five barriers) hide behind the others'.  With 1024 samples (99 KiB for fp32: one workgroup
// per CU) the fp32 pass took 185 us for 230 MB of records.
#define BIN_WG 512u
template <typename T> constexpr uint32_t bin_stage_bytes() { return BIN_WG * 8u * (uint32_t)(sizeof(typename RecVal<T>::type) + 4u) + 3u * BINS_PER_LEVEL * 4u; }

// wave 0 of a record workgroup, one bin per lane: reserves the workgroup's records of every bin with ONE global atomic on the bin's cursor (base[bin] = its first slot in the
// bin's list) and takes the exclusive prefix of the counts (loff[bin] = where the bin's records begin in the LDS staging area)
__device__ __forceinline__ void reserve_and_prefix(const uint32_t *cnt, uint32_t *base, uint32_t *loff, uint32_t *cursors, uint32_t hl, uint32_t sub) {
	if (threadIdx.x < BINS_PER_LEVEL) {
		const uint32_t c = cnt[threadIdx.x];
		base[threadIdx.x] = c ? atomicAdd(&cursors[(hl * BINS_PER_LEVEL + threadIdx.x) * CUR_SUBS + sub], c) : 0u;
		uint32_t x = c;
#pragma unroll
		for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(x, o); if ((int)threadIdx.x >= o) x += y; }
		loff[threadIdx.x] = x - c;
	}
}

template <typename T, int LAYOUT>
__global__ __launch_bounds__(BIN_WG) void k_bin_records(uint32_t n, const float *__restrict__ pos, uint32_t stride, const T *__restrict__ dLdy, LevelTable lt, BinPlan bp, LevelSel sel,
                                                      const uint32_t *__restrict__ absmax_bits, uint32_t *__restrict__ cursors, void *__restrict__ rec_val,
                                                      uint16_t *__restrict__ rec_idx, uint32_t *__restrict__ spill_count, SpillEntry *__restrict__ spill,
                                                      const uint32_t *__restrict__ n_valid) {
	using P = typename Pair<T>::type;
	using RV = typename RecVal<T>::type;
	extern __shared__ __attribute__((aligned(16))) uint32_t bin_smem[];
	RV *stage_val = reinterpret_cast<RV *>(bin_smem);                                   // [4096] contributions, grouped by bin
	uint32_t *stage_idx = bin_smem + BIN_WG * 8u * (sizeof(RV) / 4u);                     // [4096] level-wide entry indices
	uint32_t *cnt = stage_idx + BIN_WG * 8u, *base = cnt + BINS_PER_LEVEL, *loff = base + BINS_PER_LEVEL;
	const uint32_t hl = sel.hl[blockIdx.y], level = bp.level[hl], sub = blockIdx.x % CUR_SUBS;
	const uint32_t size = lt.v[4 * level + 1], res = lt.v[4 * level + 2];
	const float scale = __uint_as_float(lt.v[4 * level + 3]);
	const bool dense = level_is_dense(size, res), il = size < BIN_LEVEL_MAX;
	const uint32_t amax = level_absmax(absmax_bits, level);
	const float vs = sizeof(T) == 2 ? bin_scale(amax) : (amax ? 1.0f : 0.f);       // fp32 records are stored unscaled
	const uint32_t lim = valid_count(n, n_valid);
	if (vs == 0.f || blockIdx.x * BIN_WG >= lim) return;                // uniform exit
	if (threadIdx.x < BINS_PER_LEVEL) cnt[threadIdx.x] = 0;
	__syncthreads();
	const uint32_t i = blockIdx.x * BIN_WG + threadIdx.x;
	const P *dy = reinterpret_cast<const P *>(dLdy);
	uint32_t idx[8], rank[8]; RV val[8];
	bool live = false;
	if (i < lim) {
		const float2 g2 = to_f2(load_dy<LAYOUT>(dy, n, level, i));
		live = (g2.x != 0.f || g2.y != 0.f);
		if (live) {
			const Corner c = locate(pos, stride, i, scale);
			cell_entries(size, res, dense, c.g[0], c.g[1], c.g[2], idx);
			const float gx = g2.x * vs, gy = g2.y * vs;
#pragma unroll
			for (uint32_t q = 0; q < 8; ++q) {
				const float w = ((q & 1u) ? c.w[0] : 1 - c.w[0]) * ((q & 2u) ? c.w[1] : 1 - c.w[1]) * ((q & 4u) ? c.w[2] : 1 - c.w[2]);
				from_f2(val[q], make_float2(gx * w, gy * w));
				rank[q] = atomicAdd(&cnt[bin_of(idx[q], il)], 1u);
			}
		}
	}
	__syncthreads();
	reserve_and_prefix(cnt, base, loff, cursors, hl, sub);
	__syncthreads();
	if (live) {
#pragma unroll
		for (uint32_t q = 0; q < 8; ++q) {
			const uint32_t slot = loff[bin_of(idx[q], il)] + rank[q];
			stage_val[slot] = val[q]; stage_idx[slot] = idx[q];
		}
	}
	__syncthreads();
	const uint32_t total = loff[BINS_PER_LEVEL - 1] + cnt[BINS_PER_LEVEL - 1];
	for (uint32_t p = threadIdx.x; p < total; p += BIN_WG) {
		const uint32_t e = stage_idx[p];
		const RV v = stage_val[p];
		const uint32_t bin = bin_of(e, il), slot = base[bin] + (p - loff[bin]);
		if (slot < bp.cap) {
			rec_val_at<RV>(rec_val, hl, bin * CUR_SUBS + sub, bp.cap)[slot] = v; rec_idx_at(rec_idx, hl, bin * CUR_SUBS + sub, bp.cap)[slot] = (uint16_t)local_of(e, il);
		} else {                                                        // bin full (pathological clustering): the shared spill list, scanned by the bin's owner
			const uint32_t k = atomicAdd(spill_count, 1u);
			if (k < bp.spill_cap) { const float2 f = to_f2(v); spill[k] = SpillEntry{(hl << 19) | e, f.x, f.y}; }
		}
	}
}

// Coarse levels: the run-combining core (hash_bwd_common.h: run_load, run_sweep) over this path's 64 bins - COUNT, the cursor reservation, PLACE.  Up to RUN_STAGE
// records are staged in LDS and leave as full lines; whatever exceeds that (scattered positions only) is stored to its reserved slot directly.
#define RUN_STAGE 3072u
static uint32_t run_stage_bytes(uint32_t stage) { return stage * 12u + 4u * BINS_PER_LEVEL * 4u; }

template <typename T, int LAYOUT, int OCC /* waves per SIMD the register budget is held to: 4 = natural (114 VGPRs), 5 = all 1280 workgroups of a 2^18-sample batch resident at once (probe) */>
__global__ __launch_bounds__(RUN_WG, OCC) void k_bin_records_runs(uint32_t n, const float *__restrict__ pos, uint32_t stride, const T *__restrict__ dLdy, LevelTable lt, BinPlan bp, LevelSel sel,
                                                           const uint32_t *__restrict__ absmax_bits, uint32_t *__restrict__ cursors, void *__restrict__ rec_val,
                                                           uint16_t *__restrict__ rec_idx, uint32_t *__restrict__ spill_count, SpillEntry *__restrict__ spill,
                                                           const uint32_t *__restrict__ n_valid, uint32_t stage /* records of LDS staging */, TailJobs tj) {
	extern __shared__ __attribute__((aligned(16))) uint32_t bin_smem[];
	const uint32_t by = blockIdx.y;
	if (tj.do_reduce) tail_reduce_share(tj, reinterpret_cast<float *>(bin_smem), by * gridDim.x + blockIdx.x, gridDim.x * gridDim.y);      // (r6, mlp_tail.h) this workgroup's 8 columns of the MLP weight-gradient slabs (+ the two packs' sweep)
	float2 *stage_val = reinterpret_cast<float2 *>(bin_smem);                             // [stage]
	uint32_t *stage_idx = bin_smem + stage * 2u;                                          // [stage] level-wide entry indices
	uint32_t *cnt = stage_idx + stage, *base = cnt + BINS_PER_LEVEL, *loff = base + BINS_PER_LEVEL, *cnt2 = loff + BINS_PER_LEVEL;
	const uint32_t hl = sel.hl[by], level = bp.level[hl], sub = blockIdx.x % CUR_SUBS;
	const uint32_t size = lt.v[4 * level + 1], res = lt.v[4 * level + 2];
	const float scale = __uint_as_float(lt.v[4 * level + 3]);
	const bool dense = level_is_dense(size, res), il = size < BIN_LEVEL_MAX;
	const uint32_t lim = valid_count(n, n_valid);
	if (level_absmax(absmax_bits, level) == 0u || blockIdx.x * RUN_WG * RUN_K >= lim) return;          // uniform exit
	if (threadIdx.x < BINS_PER_LEVEL) { cnt[threadIdx.x] = 0; cnt2[threadIdx.x] = 0; }
	__syncthreads();
	const uint32_t first = (blockIdx.x * RUN_WG + threadIdx.x) * RUN_K;
	RunSamples<false> rs;                                                                 // (cell and fraction kept per sample: the form this kernel was tuned with - see DESIGN.md for the open experiment)
	run_load<T, LAYOUT>(rs, n, pos, stride, dLdy, level, scale, first, lim);
	run_sweep(rs, size, res, dense, [&](uint32_t e, float, float) { atomicAdd(&cnt[bin_of(e, il)], 1u); });
	__syncthreads();
	reserve_and_prefix(cnt, base, loff, cursors, hl, sub);
	__syncthreads();
	const uint32_t cap = bp.cap;
	auto store = [&](uint32_t e, uint32_t bin, uint32_t slot, float2 v) {
		if (slot < cap) { rec_val_at<float2>(rec_val, hl, bin * CUR_SUBS + sub, cap)[slot] = v; rec_idx_at(rec_idx, hl, bin * CUR_SUBS + sub, cap)[slot] = (uint16_t)local_of(e, il); }
		else { const uint32_t k = atomicAdd(spill_count, 1u); if (k < bp.spill_cap) spill[k] = SpillEntry{(hl << 19) | e, v.x, v.y}; }
	};
	run_sweep(rs, size, res, dense, [&](uint32_t e, float x, float y) {
		const uint32_t bin = bin_of(e, il), rank = atomicAdd(&cnt2[bin], 1u), p = loff[bin] + rank;
		if (p < stage) { stage_val[p] = make_float2(x, y); stage_idx[p] = e; }
		else store(e, bin, base[bin] + rank, make_float2(x, y));
	});
	__syncthreads();
	const uint32_t total = min(loff[BINS_PER_LEVEL - 1] + cnt[BINS_PER_LEVEL - 1], stage);
	for (uint32_t p = threadIdx.x; p < total; p += RUN_WG) {
		const uint32_t e = stage_idx[p];
		const uint32_t bin = bin_of(e, il);
		store(e, bin, base[bin] + (p - loff[bin]), stage_val[p]);
	}
}

template <typename G, typename RV, bool ADAM>
__global__ __launch_bounds__(1024) void k_bin_accumulate(LevelTable lt, BinPlan bp, LevelSel sel, const uint32_t *__restrict__ absmax_bits, const uint32_t *__restrict__ cursors,
                                                         void *__restrict__ rec_val_base, uint16_t *__restrict__ rec_idx_base, const uint32_t *__restrict__ spill_count,
                                                         const SpillEntry *__restrict__ spill, G *__restrict__ grad, int overwrite, AdamRide ar) {
	extern __shared__ __attribute__((aligned(16))) unsigned long long iacc[];   // [BIN_ENTRIES][2] 64-bit fixed point
	using GP = typename Pair<G>::type;
	constexpr bool F32 = sizeof(RV) == 8;
	const uint32_t hl = sel.hl[blockIdx.x / BINS_PER_LEVEL], bin = blockIdx.x % BINS_PER_LEVEL, level = bp.level[hl];
	const uint32_t size = lt.v[4 * level + 1];
	const bool il = size < BIN_LEVEL_MAX;
	// slots of this bin that are entries of the level (interleaved: groups bin, bin + 64, ... of the level's ceil(size / 8) groups)
	const uint32_t groups_all = (size + 7u) >> 3;
	const uint32_t n_local = il ? (groups_all > bin ? ((groups_all - bin + 63u) >> 6) << 3 : 0u) : BIN_ENTRIES;
	const uint32_t amax = level_absmax(absmax_bits, level);
	float s32 = 0.f, inv;
	if (F32) {
		const float m = __uint_as_float(amax);
		if (m > 0.f && m < 3.0e38f) { int ex; frexpf(m, &ex); s32 = ldexpf(1.0f, 38 - ex); }
		inv = s32 > 0.f ? 1.0f / s32 : 0.f;
	} else {
		const float vs = bin_scale(amax);
		s32 = vs;                                                            // (only its zero-ness is used on this path)
		inv = vs > 0.f ? 1.0f / (vs * 16777216.0f) : 0.f;
	}
	constexpr uint32_t K = 8;
	const SubLists sl = sub_lists(cursors + (hl * BINS_PER_LEVEL + bin) * CUR_SUBS, bp.cap, K);
	const uint32_t count = sl.gstart[CUR_SUBS] * K + sl.tstart[CUR_SUBS];
	GP *dst = reinterpret_cast<GP *>(grad) + lt.v[4 * level];
	float2 *P2 = nullptr, *M2 = nullptr, *V2 = nullptr; __half2 *H2 = nullptr;     // ADAM: the level's parameters, moments and fp16 shadow as pairs
	if (ADAM) {
		P2 = reinterpret_cast<float2 *>(ar.p) + lt.v[4 * level]; M2 = reinterpret_cast<float2 *>(ar.m) + lt.v[4 * level]; V2 = reinterpret_cast<float2 *>(ar.v) + lt.v[4 * level];
		if (ar.p_half) H2 = reinterpret_cast<__half2 *>(ar.p_half) + lt.v[4 * level];
	}
	auto sweep_store = [&](uint32_t t, float2 p, float2 m, float2 v, float gx, float gy) {
		adam_ride_update(p.x, m.x, v.x, gx, ar); adam_ride_update(p.y, m.y, v.y, gy, ar);
		P2[t] = p; M2[t] = m; V2[t] = v;
		if (H2) H2[t] = __floats2half2_rn(p.x, p.y);
	};
	if (s32 == 0.f || count == 0) {                                      // nothing to add: an accumulating destination is left alone, an overwritten one gets its zeros
		if (ADAM) {                                                         // ... and the sweep sees a zero gradient
			for (uint32_t e = threadIdx.x; e < n_local; e += 1024) { const uint32_t t = entry_of(bin, e, il); if (t < size) sweep_store(t, P2[t], M2[t], V2[t], 0.f, 0.f); }
		} else if (overwrite) {
			GP zv; from_f2(zv, make_float2(0.f, 0.f));
			for (uint32_t e = threadIdx.x; e < n_local; e += 1024) { const uint32_t t = entry_of(bin, e, il); if (t < size) dst[t] = zv; }
		}
		return;
	}
	for (uint32_t e = threadIdx.x; e < n_local * 2; e += 1024) iacc[e] = 0ull;
	__syncthreads();
	const RV *rec_val = rec_val_at<RV>(rec_val_base, hl, bin * CUR_SUBS, bp.cap);  // cap % 8 == 0: both streams of every sub-list start 16-byte aligned; sub-list k begins k * cap records further
	const uint16_t *rec_idx = rec_idx_at(rec_idx_base, hl, bin * CUR_SUBS, bp.cap);
	// Consecutive records of a bin come from neighbouring samples of a ray, which often still share a cell (a run that was split between two threads of the
	// record pass; a fine level's cell that is two steps long): a wavefront's 64 lanes would hit a handful of entries, and same-address ds_add_u64 serialise.  So
	// every thread takes K = 8 CONSECUTIVE records, sums runs of equal entries in registers (exact: the sums are integers) and issues one pair of LDS atomics per
	// run; neighbouring lanes are then 8 records apart.  Two trips (64 / 32 + 16 bytes per thread each) are in flight.
	struct alignas(16) VK { RV v[K]; };
	struct alignas(16) IK { uint16_t i[K]; };
	const VK *pv = reinterpret_cast<const VK *>(rec_val);
	const IK *pi = reinterpret_cast<const IK *>(rec_idx);
	const uint32_t groups = sl.gstart[CUR_SUBS], gcap = bp.cap / K;
	auto grp = [&](uint32_t r) { return sub_group(sl, r, gcap); };     // group r of the bin -> its place in the sub-list layout
	auto add_fixed = [&](uint32_t local, long long ix, long long iy) {
		__hip_atomic_fetch_add(&iacc[2 * local], (unsigned long long)ix, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
		__hip_atomic_fetch_add(&iacc[2 * local + 1], (unsigned long long)iy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
	};
	auto add = [&](uint32_t local, RV v) { long long ix, iy; rec_to_fixed(v, s32, ix, iy); add_fixed(local, ix, iy); };
	auto run_add = [&](const VK &x, const IK &k) {
		uint32_t cur = k.i[0]; long long sx, sy; rec_to_fixed(x.v[0], s32, sx, sy);
#pragma unroll
		for (uint32_t q = 1; q < K; ++q) {
			long long ix, iy; rec_to_fixed(x.v[q], s32, ix, iy);
			if (k.i[q] == cur) { sx += ix; sy += iy; }
			else { add_fixed(cur, sx, sy); cur = k.i[q]; sx = ix; sy = iy; }
		}
		add_fixed(cur, sx, sy);
	};
	uint32_t r = threadIdx.x;
	for (; r + 1024 < groups; r += 2 * 1024) {
		const uint32_t a0 = grp(r), a1 = grp(r + 1024);
		const VK x0 = pv[a0], x1 = pv[a1]; const IK k0 = pi[a0], k1 = pi[a1];
		run_add(x0, k0); run_add(x1, k1);
	}
	for (; r < groups; r += 1024) { const uint32_t a0 = grp(r); const VK x = pv[a0]; const IK k = pi[a0]; run_add(x, k); }
	if (threadIdx.x < sl.tstart[CUR_SUBS]) {                             // the < K leftover records of every sub-list
		const uint32_t t = sub_tail(sl, threadIdx.x, bp.cap, K);
		add(rec_idx[t], rec_val[t]);
	}
	if (sl.over) {                                                        // a sub-list of this bin overflowed: its surplus records are somewhere in the shared spill list
		const uint32_t ns = min(*spill_count, bp.spill_cap);
		for (uint32_t t = threadIdx.x; t < ns; t += 1024) {
			const SpillEntry se = spill[t];
			const uint32_t e = se.key & (BIN_LEVEL_MAX - 1u);
			if ((se.key >> 19) == hl && bin_of(e, il) == bin) { RV v; from_f2(v, make_float2(se.x, se.y)); add(local_of(e, il), v); }
		}
	}
	__syncthreads();
	if (ADAM) {
		static_assert(BIN_ENTRIES == 8u * 1024u, "eight entries per thread");
		float2 rp[8], rm[8], rv[8];                                         // this thread's eight entries (the write-out's own assignment): all loads first
#pragma unroll
		for (uint32_t k = 0; k < 8; ++k) {
			const uint32_t e = threadIdx.x + k * 1024, t = e < n_local ? entry_of(bin, e, il) : ~0u;
			rp[k] = rm[k] = rv[k] = make_float2(0.f, 0.f);
			if (t < size) { rp[k] = P2[t]; rm[k] = M2[t]; rv[k] = V2[t]; }
		}
#pragma unroll
		for (uint32_t k = 0; k < 8; ++k) {
			const uint32_t e = threadIdx.x + k * 1024, t = e < n_local ? entry_of(bin, e, il) : ~0u;
			if (!(t < size)) continue;
			const long long sx = (long long)iacc[2 * e], sy = (long long)iacc[2 * e + 1];
			sweep_store(t, rp[k], rm[k], rv[k], (float)sx * inv, (float)sy * inv);
		}
		return;
	}
	for (uint32_t e0 = 0; e0 < n_local; e0 += 8u * 1024u) {                // (a full bin: one trip, all eight read-modify-write loads in flight)
		GP oldv[8]; uint32_t tgt[8];
#pragma unroll
		for (uint32_t k = 0; k < 8; ++k) {
			const uint32_t e = e0 + threadIdx.x + k * 1024;
			tgt[k] = e < n_local ? entry_of(bin, e, il) : ~0u;
			if (tgt[k] >= size) tgt[k] = ~0u;
			if (!overwrite && tgt[k] != ~0u) oldv[k] = dst[tgt[k]];
		}
#pragma unroll
		for (uint32_t k = 0; k < 8; ++k) {
			if (tgt[k] == ~0u) continue;
			const uint32_t e = e0 + threadIdx.x + k * 1024;
			const long long sx = (long long)iacc[2 * e], sy = (long long)iacc[2 * e + 1];
			float2 v = make_float2((float)sx * inv, (float)sy * inv);
			if (!overwrite) { if (sx == 0 && sy == 0) continue; const float2 old = to_f2(oldv[k]); v.x += old.x; v.y += old.y; }
			GP o; from_f2(o, v);
			dst[tgt[k]] = o;
		}
	}
}
