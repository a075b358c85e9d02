// Table-gradient scatter, RECORD REGIONS (round 4): the workspace path of fp32 dL/dy into an fp32 gradient (ngp_base.py) - no global atomic of any kind, one accumulate
// kernel for all levels.  Launched by launch_regions (hash_encode.hip).
#pragma once
#include "hash_bwd_common.h"

// ---------------------------------------------------------------------------------------------------------------- edge records (r4): the fine hashed levels, fp32
// Round 3's fine levels wrote eight 10-byte records per (sample, level) - 124 MB out and back in for the six fine levels of the ngp_base.py table - through lists whose
// slots were handed out by one returning global atomic per (workgroup, bin).  Two things were wrong with that, both measured this round (profiles/r04_scatter_probes.md):
//   * the ATOMICS, not the bytes, set the record kernels' duration: returning device-scope atomics retire at ~8 G/s chip-wide whatever their addresses (eight cursors
//     per bin changed nothing), so the 196 k / 393 k reservations of a 2^18-sample batch cost 25 / 50 us of k_bin_pairs' 52 / 78 us (1024- / 512-sample workgroups);
//     the stores themselves cost 9 us, and the plain append pattern without atomics runs at 5-6 TB/s (tools/microbench_stream.py);
//   * the eight contributions of a cell share most of their bits.
// So: NO global atomics and half the bytes.
//   * The hash is x ^ y*P1 ^ z*P2 masked to 19 bits and x + 1 <= res <= 2048 touches bits 0..11 only: the two x-neighbours of a cell edge ALWAYS fall into the same
//     4096-entry slice of the level.  Bins are 4096 entries (128 per level) and ONE record carries the edge: {a = g.x*(wy*wz), b = g.y*(wy*wz), fx, slot0 | slot1 << 12},
//     16 bytes for two contributions (a*(1-fx), b*(1-fx) -> slot0; a*fx, b*fx -> slot1; the accumulate kernel multiplies: three roundings per contribution like the
//     reference's ((wx*wy)*wz)*g, in another order - each within 3 * 2^-24 of the exact product, up to 4 ulp apart (tests/test_host_cpu.py), far inside what the reference's float atomics scatter around the exact sum;
//     the accumulation itself stays exact, 64-bit integers).
//   * Every record workgroup owns a REGION of the record area (4 x its samples records): it sorts its edge records by bin in LDS (histogram, prefix, staging - as before)
//     and writes the staged block out as it is - one contiguous, fully coalesced 64 KiB store stream - plus the 129 bin offsets inside its region (u16).  Nothing is
//     reserved, nothing can overflow, the layout is deterministic.
//   * The accumulate workgroup of (level, bin) walks the W regions: eight lanes per region read that region's segment of the bin (offset table -> start, length;
//     32 records on average = one 64-byte quad of records per lane), neighbours that name the same edge are summed in registers, four LDS atomics per distinct edge.
//     64 KiB of accumulators: two workgroups per CU, one's write-out and start-up hide behind the other's record stream.
// Levels: hashed, 2^19 entries, run-combining limit < res <= 2048, fp32 dL/dy and gradient.  Everything else keeps the per-corner records (hash_bwd_percorner.h).
#define PAIR_BIN_BITS 12u
#define PAIR_BIN_ENTRIES (1u << PAIR_BIN_BITS)
#define PAIR_BINS 128u
#define PAIR_RES_MAX 2048u
#define PAIR_OFFS (PAIR_BINS + 2u)                                     // u16 offsets per region: 128 bin starts, the total, one pad (rows stay 4-byte aligned)
static_assert(PAIR_BIN_ENTRIES * PAIR_BINS == BIN_LEVEL_MAX, "the edge-record path covers the full 2^19-entry levels");
struct alignas(16) PairRec { float a, b, fx; uint32_t loc; };
#define PAIR_STAGE_RECORDS 4096u                                       // LDS staging of a record workgroup = its region: 1024 samples x 4 edge records | 512 samples x 8 single records
static uint32_t pair_stage_bytes() { return PAIR_STAGE_RECORDS * 16u + (2u * PAIR_BINS + 4u) * 4u; }
__host__ __device__ static inline uint32_t pair_region_records() { return PAIR_STAGE_RECORDS + 4u; }     // + 4: slack behind the last segment

// wave 0 of a record workgroup, two bins per lane: the exclusive prefix of the 128 bin counts = the bin offsets inside the workgroup's region, to LDS (loff[PAIR_BINS] = the
// total) and, as u16, to the region's row of the offset table (a region holds at most 16384 records < 2^16)
__device__ __forceinline__ void region_offsets(const uint32_t *cnt, uint32_t *loff, uint16_t *my_off) {
	if (threadIdx.x < 64u) {
		const uint32_t b0 = 2u * threadIdx.x, c0 = cnt[b0], c1 = cnt[b0 + 1u];
		uint32_t x = c0 + c1;
#pragma unroll
		for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(x, o); if ((int)threadIdx.x >= o) x += y; }
		const uint32_t e0 = x - (c0 + c1);
		loff[b0] = e0; loff[b0 + 1u] = e0 + c0;
		reinterpret_cast<uint32_t *>(my_off)[threadIdx.x] = e0 | ((e0 + c0) << 16);
		if (threadIdx.x == 63u) { loff[PAIR_BINS] = x; reinterpret_cast<uint32_t *>(my_off)[64] = x; }
	}
}

// S samples per workgroup = one region.  Levels beyond res 2048 (aabb_scale > 1: ngp_fox.py's 2353 .. 8192) cannot pair their x-neighbours - x + 1 reaches into the
// bin bits - so they emit eight SINGLE records per sample in the same format (fx = 0, both slots the same entry: the second contribution is an exact zero and is
// skipped); S = 512 then.  T = type of dL/dy (fp16 configuration: the contributions are formed in fp32 from the fp16 gradient - at least as accurate as the fp16
// records of the per-corner path).
template <typename T, int LAYOUT, uint32_t S>
__global__ __launch_bounds__(S) void k_bin_pairs(uint32_t n, const float *__restrict__ pos, uint32_t stride, const T *__restrict__ dLdy, LevelTable lt, BinPlan bp, LevelSel sel,
                                                 const uint32_t *__restrict__ absmax_bits, PairRec *__restrict__ prec, uint16_t *__restrict__ poff,
                                                 uint32_t *__restrict__ spill_count, SpillEntry *__restrict__ spill, const uint32_t *__restrict__ n_valid, TailJobs tj) {
	using P = typename Pair<T>::type;
	extern __shared__ __attribute__((aligned(16))) uint32_t bin_smem[];
	const uint32_t po = blockIdx.y;
	if (tj.do_sweep) tail_pack_share(tj, po * gridDim.x + blockIdx.x, gridDim.x * gridDim.y);      // (r6, mlp_tail.h) this workgroup's 32 slots of the MLP fragment buffer, from the pack the run kernel's launch has swept
	PairRec *stage = reinterpret_cast<PairRec *>(bin_smem);                                   // [PAIR_STAGE_RECORDS] records, grouped by bin
	uint32_t *cnt = bin_smem + PAIR_STAGE_RECORDS * 4u, *loff = cnt + PAIR_BINS;             // loff[PAIR_BINS] = total
	const uint32_t hl = sel.hl[po], level = bp.level[hl];
	const uint32_t mask = lt.v[4 * level + 1] - 1u;
	const bool split = lt.v[4 * level + 2] > PAIR_RES_MAX;                                    // (uniform; the host launches S = 512 when any level of the launch is split)
	const float scale = __uint_as_float(lt.v[4 * level + 3]);
	const size_t region = (size_t)po * gridDim.x + blockIdx.x;
	uint16_t *my_off = poff + region * PAIR_OFFS;
	const uint32_t lim = valid_count(n, n_valid);
	if (level_absmax(absmax_bits, level) == 0u || blockIdx.x * S >= lim || (split && S * 8u > PAIR_STAGE_RECORDS)) {   // uniform exit: an empty region
		if (threadIdx.x < PAIR_OFFS) my_off[threadIdx.x] = 0;
		return;
	}
	if (threadIdx.x < PAIR_BINS) cnt[threadIdx.x] = 0;
	__syncthreads();
	const uint32_t i = blockIdx.x * S + threadIdx.x;
	const P *dy = reinterpret_cast<const P *>(dLdy);
	float2 g2 = make_float2(0.f, 0.f);
	Corner c;
	uint32_t h[4], rank[8];
	bool live = false;
	if (i < lim) {
		g2 = to_f2(load_dy<LAYOUT>(dy, n, level, i));
		live = (g2.x != 0.f || g2.y != 0.f);
		if (live) {
			c = locate(pos, stride, i, scale);
			const uint32_t ty0 = c.g[1] * 19349663u, tz0 = c.g[2] * 83492791u;
#pragma unroll
			for (uint32_t q = 0; q < 4; ++q) {                                // q = (y corner, z corner), HashEncode.h:68-94
				h[q] = (ty0 + ((q & 1u) ? 19349663u : 0u)) ^ (tz0 + ((q & 2u) ? 83492791u : 0u));
				const uint32_t i0 = (c.g[0] ^ h[q]) & mask, i1 = ((c.g[0] + 1u) ^ h[q]) & mask;
				if (split) { rank[2 * q] = atomicAdd(&cnt[i0 >> PAIR_BIN_BITS], 1u); rank[2 * q + 1] = atomicAdd(&cnt[i1 >> PAIR_BIN_BITS], 1u); }
				// (edge levels: positions outside the unit cube can carry x + 1 into the bin bits: that edge goes to the spill list as two contributions, rank = ~0)
				else rank[2 * q] = ((i0 ^ i1) >> PAIR_BIN_BITS) ? ~0u : atomicAdd(&cnt[i0 >> PAIR_BIN_BITS], 1u);
			}
		}
	}
	__syncthreads();
	region_offsets(cnt, loff, my_off);
	__syncthreads();
	if (live) {
#pragma unroll
		for (uint32_t q = 0; q < 4; ++q) {
			const float wy = (q & 1u) ? c.w[1] : 1 - c.w[1], wz = (q & 2u) ? c.w[2] : 1 - c.w[2];
			const uint32_t i0 = (c.g[0] ^ h[q]) & mask, i1 = ((c.g[0] + 1u) ^ h[q]) & mask;
			if (split) {
				const float w0 = ((1 - c.w[0]) * wy) * wz, w1 = (c.w[0] * wy) * wz;             // the reference's x, y, z multiplication order
				const uint32_t l0 = i0 & (PAIR_BIN_ENTRIES - 1u), l1 = i1 & (PAIR_BIN_ENTRIES - 1u);
				stage[loff[i0 >> PAIR_BIN_BITS] + rank[2 * q]] = PairRec{g2.x * w0, g2.y * w0, 0.f, l0 | (l0 << PAIR_BIN_BITS)};
				stage[loff[i1 >> PAIR_BIN_BITS] + rank[2 * q + 1]] = PairRec{g2.x * w1, g2.y * w1, 0.f, l1 | (l1 << PAIR_BIN_BITS)};
				continue;
			}
			const float wyz = wy * wz;
			const float a = g2.x * wyz, b = g2.y * wyz;
			if (rank[2 * q] != ~0u) {
				stage[loff[i0 >> PAIR_BIN_BITS] + rank[2 * q]] = PairRec{a, b, c.w[0], (i0 & (PAIR_BIN_ENTRIES - 1u)) | ((i1 & (PAIR_BIN_ENTRIES - 1u)) << PAIR_BIN_BITS)};
			} else {
				const uint32_t k = atomicAdd(spill_count, 2u);
				const float w0 = 1 - c.w[0];
				if (k + 1u < bp.spill_cap) { spill[k] = SpillEntry{(hl << 19) | i0, a * w0, b * w0}; spill[k + 1u] = SpillEntry{(hl << 19) | i1, a * c.w[0], b * c.w[0]}; }
			}
		}
	}
	__syncthreads();
	const uint32_t total = loff[PAIR_BINS];
	PairRec *out = prec + region * pair_region_records();
#ifdef NGP_PROBE_SCATTER                                                                      // timing experiment (tools/probe_scatter.py builds it): no record stores - results WRONG
	if (total != 0x7fffffffu) return;
#endif
	for (uint32_t p = threadIdx.x; p < total; p += S) out[p] = stage[p];
}

// ---- run records without atomics (r4): the coarse levels of the fp32 path.  The run-combining core (hash_bwd_common.h: run_load, run_sweep) with the edge kernel's
// layout: a region per record workgroup (its run records sorted by bin, 12 bytes each {x, y, slot}; the bin offsets beside them), 128 bins of 4096 entries like the edge
// levels - so that ONE accumulate kernel serves every level.  Entries of a level smaller than 2^19 are dealt to the bins in interleaved groups of eight (the spatially
// coherent dense indices spread evenly), as the per-corner path does with 64 bins.
struct RunRec { float x, y; uint32_t loc; };
#define RUN2_OFFS (PAIR_BINS + 2u)
static_assert(RUN2_OFFS == PAIR_OFFS && PAIR_BINS == 128u, "region_offsets: one wave, two bins per lane, 65 words per row of either offset table");
__host__ __device__ static inline uint32_t run2_region_records() { return RUN_WG * RUN_K * 8u + 4u; }
#define RUN2_STAGE 2048u                                                 // staged run records per workgroup of the region path (x 12 B + tables = 26 KiB: five workgroups per CU with room to spare; round 4: 54 -> 43 us)
static uint32_t run2_stage_bytes(uint32_t stage) { return stage * 12u + (3u * PAIR_BINS + 4u) * 4u; }
__host__ __device__ __forceinline__ uint32_t bin2_of(uint32_t e, bool il) { return il ? (e >> 3) & (PAIR_BINS - 1u) : e >> PAIR_BIN_BITS; }
__host__ __device__ __forceinline__ uint32_t local2_of(uint32_t e, bool il) { return il ? ((e >> 10) << 3) | (e & 7u) : e & (PAIR_BIN_ENTRIES - 1u); }
__host__ __device__ __forceinline__ uint32_t entry2_of(uint32_t bin, uint32_t local, bool il) { return il ? ((local >> 3) << 10) | (bin << 3) | (local & 7u) : (bin << PAIR_BIN_BITS) | local; }

// (r7) timing build -DNGP_PROBE_CLOCK (tools/probe_hash_bwd_phases.py): thread 0 of every workgroup of k_bin_runs2 (K = 0) and k_bin_accumulate2 (K = 1) stamps the 100 MHz
// wall clock at its phase boundaries; results are unchanged, the build is never the product
#ifdef NGP_PROBE_CLOCK
#define PROBE_CLOCK_WGS 4096u
#define PROBE_CLOCK_SLOTS 8u
__device__ unsigned long long g_probe_clock[2][PROBE_CLOCK_WGS][PROBE_CLOCK_SLOTS];
#define PROBE_TICK(K, WG, I) do { if (threadIdx.x == 0 && (WG) < PROBE_CLOCK_WGS) g_probe_clock[K][WG][I] = wall_clock64(); } while (0)
NGP_API int ngp_x_probe_clock(unsigned long long *out_host, int clear) {
	hipError_t e = hipDeviceSynchronize();
	if (e == hipSuccess && out_host) e = hipMemcpyFromSymbol(out_host, HIP_SYMBOL(g_probe_clock), sizeof(g_probe_clock));
	if (e == hipSuccess && clear) { void *d = nullptr; e = hipGetSymbolAddress(&d, HIP_SYMBOL(g_probe_clock)); if (e == hipSuccess) e = hipMemset(d, 0, sizeof(g_probe_clock)); }
	return (int)e;
}
#else
#define PROBE_TICK(K, WG, I) do {} while (0)
#endif

// (r7, profiles/r07_hash_bwd_stage.md) V2: (a) all 1280 workgroups start together and every one of them began with its unit of the MLP tail - two dependent rounds of loads,
// 6.4 us in which the whole GPU waited; now the odd workgroups carry their unit at their END, so one half's latency lies under the other half's sweeps.  (b) the thread keeps
// p = pos * scale + 0.5 (24 registers) and takes cell and fraction from it in each sweep instead of keeping both (48): nothing spills at five waves per SIMD.  Same records.
template <typename T, int LAYOUT, int OCC, bool V2 = false>
__global__ __launch_bounds__(RUN_WG, OCC) void k_bin_runs2(uint32_t n, const float *__restrict__ pos, uint32_t stride, const T *__restrict__ dLdy, LevelTable lt, BinPlan bp, LevelSel sel,
                                                         const uint32_t *__restrict__ absmax_bits, RunRec *__restrict__ rrec, uint16_t *__restrict__ roff,
                                                         const uint32_t *__restrict__ n_valid, uint32_t stage /* records of LDS staging */, TailJobs tj) {
	extern __shared__ __attribute__((aligned(16))) uint32_t bin_smem[];
	const uint32_t ro = blockIdx.y;
	PROBE_TICK(0, ro * gridDim.x + blockIdx.x, 0);
	const bool tail_last = V2 && tj.do_reduce && ((ro * gridDim.x + blockIdx.x) & 1u);
	if (tj.do_reduce && !tail_last) tail_reduce_share(tj, reinterpret_cast<float *>(bin_smem), ro * gridDim.x + blockIdx.x, gridDim.x * gridDim.y);      // (r6, mlp_tail.h) this workgroup's 8 columns of the MLP weight-gradient slabs (+ their parameters' sweep)
	PROBE_TICK(0, ro * gridDim.x + blockIdx.x, 1);
	RunRec *stage_rec = reinterpret_cast<RunRec *>(bin_smem);                              // [stage]
	uint32_t *cnt = bin_smem + stage * 3u, *loff = cnt + PAIR_BINS, *cnt2 = loff + PAIR_BINS + 2u;   // loff[PAIR_BINS] = total
	const uint32_t hl = sel.hl[ro], level = bp.level[hl];
	const uint32_t size = lt.v[4 * level + 1], res = lt.v[4 * level + 2];
	const float scale = __uint_as_float(lt.v[4 * level + 3]);
	const bool dense = level_is_dense(size, res), il = size < BIN_LEVEL_MAX;
	const size_t region = (size_t)ro * gridDim.x + blockIdx.x;
	uint16_t *my_off = roff + region * RUN2_OFFS;
	const uint32_t lim = valid_count(n, n_valid);
	if (level_absmax(absmax_bits, level) == 0u || blockIdx.x * RUN_WG * RUN_K >= lim) {        // uniform exit: an empty region
		if (threadIdx.x < RUN2_OFFS) my_off[threadIdx.x] = 0;
		if (tail_last) tail_reduce_share(tj, reinterpret_cast<float *>(bin_smem), ro * gridDim.x + blockIdx.x, gridDim.x * gridDim.y);
		return;
	}
	if (threadIdx.x < PAIR_BINS) { cnt[threadIdx.x] = 0; cnt2[threadIdx.x] = 0; }
	__syncthreads();
	const uint32_t first = (blockIdx.x * RUN_WG + threadIdx.x) * RUN_K;
	RunSamples<V2> rs;                                                                    // V2: rs.pp = pos * scale + 0.5; cell and fraction are taken from it in the sweeps
	run_load<T, LAYOUT>(rs, n, pos, stride, dLdy, level, scale, first, lim);
	PROBE_TICK(0, (uint32_t)region, 2);
	run_sweep(rs, size, res, dense, [&](uint32_t e, float, float) { atomicAdd(&cnt[bin2_of(e, il)], 1u); });
	__syncthreads();
	PROBE_TICK(0, (uint32_t)region, 3);
	if constexpr (V2) {                                                         // the second sweep takes cell and fraction from rs.pp AGAIN: values of the first kept alive across the passes are what spilled
#pragma unroll
		for (uint32_t k = 0; k < RUN_K; ++k)
#pragma unroll
			for (int d = 0; d < 3; ++d) asm volatile("" : "+v"(rs.pp[k][d]));
	}
	region_offsets(cnt, loff, my_off);
	__syncthreads();
	PROBE_TICK(0, (uint32_t)region, 4);
	RunRec *out = rrec + region * run2_region_records();
	run_sweep(rs, size, res, dense, [&](uint32_t e, float x, float y) {
		const uint32_t bin = bin2_of(e, il), p = loff[bin] + atomicAdd(&cnt2[bin], 1u);
		const RunRec r{x, y, local2_of(e, il)};
		if (p < stage) stage_rec[p] = r; else out[p] = r;                      // beyond the staging area (scattered positions only): straight to its place in the region
	});
	__syncthreads();
	PROBE_TICK(0, (uint32_t)region, 5);
	const uint32_t total = min(loff[PAIR_BINS], stage);
#ifdef NGP_PROBE_SCATTER                                                                  // timing experiment: no record stores from the staging area - results WRONG
	if (total != 0x7fffffffu) return;
#endif
	for (uint32_t p = threadIdx.x; p < total; p += RUN_WG) out[p] = stage_rec[p];
	PROBE_TICK(0, (uint32_t)region, 6);
	if (tail_last) {                                                            // (the staging area is the unit's scratch: every thread has copied its records out)
		__syncthreads();
		tail_reduce_share(tj, reinterpret_cast<float *>(bin_smem), ro * gridDim.x + blockIdx.x, gridDim.x * gridDim.y);
		PROBE_TICK(0, (uint32_t)region, 7);
	}
}

// ---- ONE accumulate kernel for every level of the fp32 path: a workgroup per (level, 4096-entry bin), 64 KiB of 64-bit accumulators (two workgroups per CU).  It walks
// the record regions of its level: LANES lanes per region read the region's segment of the bin (offset table -> start, length) with consecutive lanes on consecutive
// records (full lines), I records per lane in flight, U regions per thread.  Unit order: edge levels first (the heavier units), then the run levels.
#define ACC2_WG 512u
#define ACC2_RB 512u                                                     // regions per block of the gather (= threads: one region per thread when the segment table is built)
#define ACC2_MAPN 1024u
#define ACC2_LDS_EXTRA ((2u * (ACC2_RB + 1u) + 16u) * 4u + ACC2_MAPN * 8u)
struct Acc2Plan { uint32_t n_pair, n_run, pair_regions, pair_region_records, run_regions, run_region_records, probe; };
static_assert(ACC2_RB == ACC2_WG, "gather_flat builds one segment-table row per thread");
// The records of one (level, bin) lie in n_regions segments (one per record workgroup).  Per block of ACC2_RB regions: segment table (start, length) -> exclusive prefix P in LDS ->
// the segments laid end to end as ONE flat list that the threads walk densely (thread t takes flat records t, t + 512, ...; eight loads in flight): consecutive lanes read
// consecutive records of a segment (full lines) and every lane has work - eight lanes per segment with a fixed number of slots left half of them idle, and the kernel was
// bound by exactly that (k_bin_accumulate2 90 us).  flat index -> segment: a map with one entry per 2^shift flat records (the segment holding the first of them), then a
// short forward walk over P.
// this thread's row of the segment table of (level, bin): region w0 + threadIdx.x -> {length, index of the segment's first record}
__device__ __forceinline__ uint2 segment_row(const uint16_t *__restrict__ offs, uint32_t level_ord, uint32_t n_regions, uint32_t region_records, uint32_t offs_per_region, uint32_t bin, uint32_t w0) {
	if (w0 + threadIdx.x >= n_regions) return make_uint2(0u, 0u);
	const size_t region = (size_t)level_ord * n_regions + w0 + threadIdx.x;
	const uint32_t o = *reinterpret_cast<const uint32_t *>(offs + region * offs_per_region + (bin & ~1u));        // offsets of bins 2k, 2k+1 in one word
	const uint32_t o2 = *reinterpret_cast<const uint32_t *>(offs + region * offs_per_region + (bin & ~1u) + 2u);  // ... of 2k+2 (or the total)
	const uint32_t q0 = (bin & 1u) ? o >> 16 : o & 0xffffu, q1 = (bin & 1u) ? o2 & 0xffffu : o >> 16;
	return make_uint2(q1 - q0, (uint32_t)(region * region_records) + q0);
}
template <typename Rec> __device__ __forceinline__ Rec nt_ld_rec(const Rec *p) {
	uint32_t w[sizeof(Rec) / 4];
#pragma unroll
	for (uint32_t k = 0; k < sizeof(Rec) / 4; ++k) w[k] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(p) + k);
	Rec r; __builtin_memcpy(&r, w, sizeof(Rec)); return r;
}
template <uint32_t B /* records in flight per thread */, typename Rec, typename F>
__device__ __forceinline__ void gather_flat(const Rec *__restrict__ recs, const uint16_t *__restrict__ offs, uint32_t level_ord, uint32_t n_regions, uint32_t region_records,
                                            uint32_t offs_per_region, uint32_t bin, uint32_t *__restrict__ lds, uint32_t probe /* timing experiments: 1 = records loaded, not processed; 2 = not loaded */,
                                            uint2 row0 /* segment_row(..., 0), loaded by the caller ahead of time */, F process) {
	uint32_t sink = 0;
	uint2 *seg = reinterpret_cast<uint2 *>(lds);                           // [RB + 1] per segment: {flat index of its END, start - flat index of its beginning}: one 8-byte read answers "is f mine" and "where is it"
	uint32_t *wsum = lds + 2u * (ACC2_RB + 1u);                            // per-wave totals[8 (+8 spare)]
	uint2 *map = reinterpret_cast<uint2 *>(wsum + 16u);                    // [ACC2_MAPN] per 2^shift flat records: the seg entry of the segment holding the first of them, its index in the top 9 bits of .x
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	for (uint32_t w0 = 0; w0 < n_regions; w0 += ACC2_RB) {
		const uint2 row = w0 == 0 ? row0 : segment_row(offs, level_ord, n_regions, region_records, offs_per_region, bin, w0);
		const uint32_t len = row.x, st = row.y;
		uint32_t inc = len;                                                 // inclusive prefix over the workgroup's 512 lengths
#pragma unroll
		for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(inc, o); if ((int)lane >= o) inc += y; }
		if (lane == 63u) wsum[wave] = inc;
		__syncthreads();
		uint32_t base = 0, T = 0;
#pragma unroll
		for (uint32_t k = 0; k < ACC2_WG / 64u; ++k) { const uint32_t v = wsum[k]; base += k < wave ? v : 0u; T += v; }
		const uint32_t p0 = base + inc - len;
		seg[threadIdx.x] = make_uint2(p0 + len, st - p0);
		if (threadIdx.x == ACC2_RB - 1u) seg[ACC2_RB] = make_uint2(0xffffffffu, 0u);     // sentinel: the forward walk stops here
		uint32_t shift = 3;
		while ((T >> shift) >= ACC2_MAPN) ++shift;
		if (T >> 23) { T = (1u << 23) - 1u; }                               // (cannot happen below 8 M records per bin; keeps the packed entries well-formed)
		if (len) { const uint32_t G = 1u << shift; for (uint32_t g = (p0 + G - 1u) >> shift; (g << shift) < p0 + len; ++g) map[g] = make_uint2((p0 + len) | (threadIdx.x << 23), st - p0); }   // (T < 2^23: 8 M records of one bin)
		__syncthreads();
		for (uint32_t f0 = threadIdx.x; f0 < T; f0 += ACC2_WG * B) {
			Rec x[B];
#pragma unroll
			for (uint32_t b = 0; b < B; ++b) {
				const uint32_t f = f0 + b * ACC2_WG;
				if (f < T) {
					uint2 e = map[f >> shift];
					uint32_t w = e.x >> 23; e.x &= 0x7fffffu;
					while (f >= e.x) e = seg[++w];                          // (rarely: f lies up to 2^shift - 1 records behind the mapped one; empty segments end where they begin: skipped)
#ifndef ACC2_NO_NT
					if (!(probe & 2u)) x[b] = nt_ld_rec(recs + e.y + f);
#else
					if (!(probe & 2u)) x[b] = recs[e.y + f];
#endif
				}
			}
#pragma unroll
			for (uint32_t b = 0; b < B; ++b) if (f0 + b * ACC2_WG < T) { if (probe & 1u) sink ^= reinterpret_cast<const uint32_t *>(&x[b])[0]; else process(x[b]); }
		}
		__syncthreads();                                                    // the tables are rebuilt for the next block of regions
	}
	if (sink == 0x9e3779b9u) lds[0] = sink;                                 // (keeps the probe's loads alive)
}

// (r6) The table's Adam + EMA sweep can RIDE in this kernel (ADAM = true, fp32 table on one GPU with backward and sweep in one ngp_train_step call): a unit owns its
// 4096 entries exclusively and holds their finished gradient sums in LDS, so the thread that would store a gradient pair applies optim.hip's adam_ema_update to the
// parameter instead - the same arithmetic on the same float, hence the same bits as the separate k_adam_ema launch (test_fused_launches_of_the_native_step_change_no_bit).
// The gradient itself is never written (48.8 MB out + 48.8 MB back in per iteration saved, one launch less), and the sweep's HBM streams run beside the other resident
// workgroups' LDS-atomic phases: 103 us for both jobs against 70 + 49 us as two launches (+3.7 % it/s, profiles/r06l_ab_variants.txt).  Requesting the unit's p, m, v
// BEFORE the record gather (48 registers per thread held across it, six to eight records in flight) was measured too and is slower than loading them here: 110 - 114 us.
// the moments and the records are touched once per iteration: as non-temporal accesses they leave the caches to the table the next forward gathers from
// (profiles/r06m_ab_variants.txt: every kernel of the step 0-2 us shorter, +0.2 % it/s - inside the noise of a pair, consistent over both; -DACC2_NO_NT builds the plain accesses)
typedef float f4v_nt __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 nt_ld4(const float4 *p) { const f4v_nt v = __builtin_nontemporal_load(reinterpret_cast<const f4v_nt *>(p)); return make_float4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ void nt_st4(float4 *p, float4 v) { const f4v_nt t = {v.x, v.y, v.z, v.w}; __builtin_nontemporal_store(t, reinterpret_cast<f4v_nt *>(p)); }
#ifndef ACC2_NO_NT
#define MV_LD(ptr) nt_ld4(ptr)
#define MV_ST(ptr, val) nt_st4((ptr), (val))
#else
#define MV_LD(ptr) (*(ptr))
#define MV_ST(ptr, val) (*(ptr) = (val))
#endif
template <typename G, bool ADAM>
__global__ __launch_bounds__(ACC2_WG, 4) void k_bin_accumulate2(LevelTable lt, BinPlan bp, LevelSel sel_pair, LevelSel sel_run, Acc2Plan ap, const uint32_t *__restrict__ absmax_bits,
                                                               const PairRec *__restrict__ prec, const uint16_t *__restrict__ poff, const RunRec *__restrict__ rrec, const uint16_t *__restrict__ roff,
                                                               const uint32_t *__restrict__ spill_count, const SpillEntry *__restrict__ spill, G *__restrict__ grad, int overwrite, AdamRide ar) {
	extern __shared__ __attribute__((aligned(16))) unsigned long long iacc[];   // [PAIR_BIN_ENTRIES][2] 64-bit fixed point
	using GP = typename Pair<G>::type;
	uint32_t *tables = reinterpret_cast<uint32_t *>(iacc + 2u * PAIR_BIN_ENTRIES);        // gather_flat's segment tables, behind the accumulators
	// one unit = one (level, bin) per workgroup, two workgroups per CU.  (A persistent variant - resident workgroups drawing units from a queue - was measured in round 4
	// and dropped: profiles/r04_scatter_probes.md.)
	const uint32_t n_units = (ap.n_pair + ap.n_run) * PAIR_BINS;
	const uint32_t u_this = blockIdx.x;
	if (u_this >= n_units) return;
	PROBE_TICK(1, blockIdx.x, 0);
	{
		const bool pr0 = u_this < ap.n_pair * PAIR_BINS;
		const uint32_t v0 = pr0 ? u_this : u_this - ap.n_pair * PAIR_BINS;
		const uint2 row0 = pr0 ? segment_row(poff, v0 / PAIR_BINS, ap.pair_regions, ap.pair_region_records, PAIR_OFFS, v0 % PAIR_BINS, 0u)
		                       : segment_row(roff, v0 / PAIR_BINS, ap.run_regions, ap.run_region_records, RUN2_OFFS, v0 % PAIR_BINS, 0u);
	const bool is_pair = u_this < ap.n_pair * PAIR_BINS;
	const uint32_t unit = is_pair ? u_this : u_this - ap.n_pair * PAIR_BINS;
	const uint32_t ord = unit / PAIR_BINS, bin = unit % PAIR_BINS, hl = is_pair ? sel_pair.hl[ord] : sel_run.hl[ord], level = bp.level[hl];
	const uint32_t size = lt.v[4 * level + 1];
	const bool il = size < BIN_LEVEL_MAX;
	// slots of this bin that are entries of the level (interleaved: groups bin, bin + 128, ... of the level's ceil(size / 8) groups)
	const uint32_t groups_all = (size + 7u) >> 3;
	const uint32_t n_local = il ? (groups_all > bin ? ((groups_all - bin + PAIR_BINS - 1u) / PAIR_BINS) << 3 : 0u) : PAIR_BIN_ENTRIES;
	const uint32_t amax = level_absmax(absmax_bits, level);
	float s32 = 0.f;
	{ const float m = __uint_as_float(amax); if (m > 0.f && m < 3.0e38f) { int ex; frexpf(m, &ex); s32 = ldexpf(1.0f, 38 - ex); } }
	const float inv = s32 > 0.f ? 1.0f / s32 : 0.f;
	const uint32_t ns = is_pair ? min(*spill_count, bp.spill_cap) : 0u;
	GP *dst = reinterpret_cast<GP *>(grad) + lt.v[4 * level];
#ifndef ACC2_RECORDS_IN_FLIGHT
#define ACC2_RECORDS_IN_FLIGHT 8u
#endif
	constexpr uint32_t ACC2_B = ACC2_RECORDS_IN_FLIGHT;                    // records in flight per thread
	float2 *P2 = nullptr, *M2 = nullptr, *V2 = nullptr;                  // ADAM: the level's parameters and moments as pairs
	if (ADAM) { P2 = reinterpret_cast<float2 *>(ar.p) + lt.v[4 * level]; M2 = reinterpret_cast<float2 *>(ar.m) + lt.v[4 * level]; V2 = reinterpret_cast<float2 *>(ar.v) + lt.v[4 * level]; }
	if (s32 == 0.f) {                                                     // the level has no gradient: an accumulating destination is left alone, an overwritten one gets its zeros
		if (ADAM) {                                                         // ... and the sweep sees a zero gradient (the moments decay, the parameter follows them)
			for (uint32_t e = threadIdx.x; e < n_local; e += ACC2_WG) {
				const uint32_t t = entry2_of(bin, e, il);
				if (t >= size) continue;
				float2 p = P2[t], m = M2[t], v = V2[t];
				adam_ride_update(p.x, m.x, v.x, 0.f, ar); adam_ride_update(p.y, m.y, v.y, 0.f, ar);
				P2[t] = p; M2[t] = m; V2[t] = v;
			}
		} else if (overwrite) {
			GP zv; from_f2(zv, make_float2(0.f, 0.f));
			for (uint32_t e = threadIdx.x; e < n_local; e += ACC2_WG) { const uint32_t t = entry2_of(bin, e, il); if (t < size) dst[t] = zv; }
		}
		return;                                                             // (uniform)
	}
	for (uint32_t e = threadIdx.x; e < n_local; e += ACC2_WG) { iacc[2 * e] = 0ull; iacc[2 * e + 1] = 0ull; }
	__syncthreads();
	PROBE_TICK(1, blockIdx.x, 1);
#ifdef NGP_PROBE_ACC_U32_CARRY
	// diagnosis build (tools/probe_acc_carry.sh): the 64-bit sum as two 32-bit LDS atomics with carry instead of ds_add_u64 - the low word's returning add
	// tells the one thread whose add wrapped it, which adds the carry to the high word; adds commute, so the final sum is the same integer.  Same results, slower; never the product.
	auto add64 = [&](unsigned long long *p, unsigned long long v) {
		uint32_t *w = reinterpret_cast<uint32_t *>(p);
		const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
		const uint32_t old = __hip_atomic_fetch_add(w, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
		const uint32_t up = hi + (uint32_t)((uint32_t)(old + lo) < old);
		if (up) __hip_atomic_fetch_add(w + 1, up, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
	};
#else
	auto add64 = [&](unsigned long long *p, unsigned long long v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
#endif
	auto add_fixed = [&](uint32_t local, long long ix, long long iy) {
		if ((ix | iy) == 0) return;
		add64(&iacc[2 * local], (unsigned long long)ix);
		add64(&iacc[2 * local + 1], (unsigned long long)iy);
	};
	if (is_pair) {
		gather_flat<ACC2_B>(prec, poff, ord, ap.pair_regions, ap.pair_region_records, PAIR_OFFS, bin, tables, ap.probe, row0, [&](const PairRec &r) {
			const float w0 = 1 - r.fx;
			add_fixed(r.loc & (PAIR_BIN_ENTRIES - 1u), fixed_rn(r.a * w0, s32), fixed_rn(r.b * w0, s32));
			add_fixed((r.loc >> PAIR_BIN_BITS) & (PAIR_BIN_ENTRIES - 1u), fixed_rn(r.a * r.fx, s32), fixed_rn(r.b * r.fx, s32));
		});
		for (uint32_t t = threadIdx.x; t < ns; t += ACC2_WG) {             // out-of-cube edges (normally ns == 0)
			const SpillEntry se = spill[t];
			const uint32_t e = se.key & (BIN_LEVEL_MAX - 1u);
			if ((se.key >> 19) == hl && (e >> PAIR_BIN_BITS) == bin) add_fixed(e & (PAIR_BIN_ENTRIES - 1u), __float2ll_rn(se.x * s32), __float2ll_rn(se.y * s32));
		}
	} else {
		gather_flat<ACC2_B>(rrec, roff, ord, ap.run_regions, ap.run_region_records, RUN2_OFFS, bin, tables, ap.probe, row0, [&](const RunRec &r) {
			add_fixed(r.loc, fixed_rn(r.x, s32), fixed_rn(r.y, s32));
		});
	}
#ifdef ACC2_PMV_BEFORE_BARRIER
	// (A/B build) a full bin's p, m, v requested by each thread as soon as IT has processed its records - the loads then travel while the workgroup waits at the barrier for its
	// slowest wavefront - instead of after the barrier
	float4 rp[4], rm[4], rv[4];
	if (ADAM && !il) {
		const float4 *Pq = reinterpret_cast<const float4 *>(P2 + (bin << PAIR_BIN_BITS)), *Mq = reinterpret_cast<const float4 *>(M2 + (bin << PAIR_BIN_BITS)), *Vq = reinterpret_cast<const float4 *>(V2 + (bin << PAIR_BIN_BITS));
#pragma unroll
		for (uint32_t k = 0; k < 4u; ++k) { const uint32_t q = threadIdx.x + k * ACC2_WG; rp[k] = Pq[q]; rm[k] = MV_LD(Mq + q); rv[k] = MV_LD(Vq + q); }
	}
#endif
	PROBE_TICK(1, blockIdx.x, 2);
	__syncthreads();
	PROBE_TICK(1, blockIdx.x, 3);
	if (ADAM) {                                                           // the sweep instead of the gradient store: same entries per thread as below; all of a thread's loads first
		static_assert(PAIR_BIN_ENTRIES == 8u * ACC2_WG, "eight entries per thread");
		if (!il) {
			float4 *Pq = reinterpret_cast<float4 *>(P2 + (bin << PAIR_BIN_BITS)), *Mq = reinterpret_cast<float4 *>(M2 + (bin << PAIR_BIN_BITS)), *Vq = reinterpret_cast<float4 *>(V2 + (bin << PAIR_BIN_BITS));
#ifndef ACC2_PMV_BEFORE_BARRIER
			float4 rp[4], rm[4], rv[4];
#pragma unroll
			for (uint32_t k = 0; k < 4u; ++k) { const uint32_t q = threadIdx.x + k * ACC2_WG; rp[k] = Pq[q]; rm[k] = MV_LD(Mq + q); rv[k] = MV_LD(Vq + q); }
#endif
#pragma unroll
			for (uint32_t k = 0; k < 4u; ++k) {
				const uint32_t q = threadIdx.x + k * ACC2_WG, e = 2u * q;
				const long long s0 = (long long)iacc[2 * e], s1 = (long long)iacc[2 * e + 1], s2 = (long long)iacc[2 * e + 2], s3 = (long long)iacc[2 * e + 3];
				float4 p = rp[k], m = rm[k], v = rv[k];
				adam_ride_update(p.x, m.x, v.x, (float)s0 * inv, ar); adam_ride_update(p.y, m.y, v.y, (float)s1 * inv, ar);
				adam_ride_update(p.z, m.z, v.z, (float)s2 * inv, ar); adam_ride_update(p.w, m.w, v.w, (float)s3 * inv, ar);
				Pq[q] = p; MV_ST(Mq + q, m); MV_ST(Vq + q, v);
			}
		} else {
			float2 rp[8], rm[8], rv[8];
#pragma unroll
			for (uint32_t k = 0; k < 8u; ++k) {
				const uint32_t e = threadIdx.x + k * ACC2_WG, t = entry2_of(bin, e, il);
				rp[k] = rm[k] = rv[k] = make_float2(0.f, 0.f);
				if (e < n_local && t < size) { rp[k] = P2[t]; rm[k] = M2[t]; rv[k] = V2[t]; }
			}
#pragma unroll
			for (uint32_t k = 0; k < 8u; ++k) {
				const uint32_t e = threadIdx.x + k * ACC2_WG, t = entry2_of(bin, e, il);
				if (!(e < n_local && t < size)) continue;
				const long long sx = (long long)iacc[2 * e], sy = (long long)iacc[2 * e + 1];
				float2 p = rp[k], m = rm[k], v = rv[k];
				adam_ride_update(p.x, m.x, v.x, (float)sx * inv, ar); adam_ride_update(p.y, m.y, v.y, (float)sy * inv, ar);
				P2[t] = p; M2[t] = m; V2[t] = v;
			}
		}
	} else if (!il) {                                                     // a full bin: contiguous, two entries (16 bytes of fp32 gradient) per thread and trip
		GP *d = dst + (bin << PAIR_BIN_BITS);
		for (uint32_t e = 2u * threadIdx.x; e < PAIR_BIN_ENTRIES; e += 2u * ACC2_WG) {
			const long long s0 = (long long)iacc[2 * e], s1 = (long long)iacc[2 * e + 1], s2 = (long long)iacc[2 * e + 2], s3 = (long long)iacc[2 * e + 3];
			float2 v0 = make_float2((float)s0 * inv, (float)s1 * inv), v1 = make_float2((float)s2 * inv, (float)s3 * inv);
			if (!overwrite) {
				if ((s0 | s1 | s2 | s3) == 0) continue;
				const float2 o0 = to_f2(d[e]), o1 = to_f2(d[e + 1]);
				v0.x += o0.x; v0.y += o0.y; v1.x += o1.x; v1.y += o1.y;
			}
			GP w0, w1; from_f2(w0, v0); from_f2(w1, v1);
			if (sizeof(GP) == 8) *reinterpret_cast<float4 *>(d + e) = make_float4(v0.x, v0.y, v1.x, v1.y);
			else { d[e] = w0; d[e + 1] = w1; }
		}
	} else {
		for (uint32_t e = threadIdx.x; e < n_local; e += ACC2_WG) {
			const uint32_t t = entry2_of(bin, e, il);
			if (t >= size) continue;
			const long long sx = (long long)iacc[2 * e], sy = (long long)iacc[2 * e + 1];
			float2 v = make_float2((float)sx * inv, (float)sy * inv);
			if (!overwrite) { if (sx == 0 && sy == 0) continue; const float2 old = to_f2(dst[t]); v.x += old.x; v.y += old.y; }
			GP o; from_f2(o, v);
			dst[t] = o;
		}
	}
	PROBE_TICK(1, blockIdx.x, 4);
	}
}
