// (r10) The forward gather of the RUN levels (res <= RUN_RES_MAX, the levels the backward run-combines): one thread per RUN_K consecutive samples, the eight corners of a
// cell gathered ONCE per run of samples that share it.  The samples of a ray are consecutive in the batch and a cell of such a level is 3-40 marching steps long, so
// k_hash_fwd_x2's eight gathers per (sample, level) mostly fetch what the neighbouring sample has just fetched; the texture path does not merge equal addresses of
// different lanes, let alone of different instructions - that was the premise.  MEASURED (profiles/r10_hash_fwd.md): it is not so.  k_hash_fwd_x2 takes 2.3 us for every
// run level of a training batch whatever its resolution, table size or run length - the bound there is the 131 k short wavefronts' instructions, not their gathers - and
// this kernel takes 2.3 - 4.2 us (two waves per SIMD at 208 - 248 VGPRs; a wavefront executes sample k's index arithmetic and loads whenever ANY lane opens a run at k); on
// the Morton-ordered refresh set, where the finer run levels have no runs to share, 9 - 37 us per level against 7 - 20.  So it stays behind NGP_HASH_FWD_RUNS=1, off by
// default, with its tests.  fp32 table only.  Included by hash_encode.hip (one translation unit), behind its fp-contract pragma; this header also holds the forward's
// block maps (sel_block, block_to_level_chunk_paired).
//
// A thread: loads its window's positions (one 96-byte block when it can), marks the samples that OPEN a run (the first one, and every
// one whose cell differs from its predecessor's), issues the eight gathers of EVERY opened run before the first use - up to 64 loads in flight per lane, one memory round
// trip per window however many runs it holds; only the lanes that open a run at sample k take part in sample k's loads - and then interpolates sample after sample with the
// corners of the run it belongs to.  Same table entries (grid_index), same weights, same order of the eight terms as k_hash_fwd: no output bit differs.
// A run that crosses a window is fetched once per window, the compromise the backward makes.
#pragma once
#include "hash_bwd_common.h"

#define FWD_RUN_WG 64u                                                // one wavefront per workgroup: a level's 512-sample units spread evenly over the CUs of its XCDs
#define FWD_RUN_SPAN (FWD_RUN_WG * RUN_K)                             // samples per workgroup and trip

// The levels one forward launch works on, and its blockIdx -> (level, chunk) map: the launch's units (level-major, nblk chunks per level) are dealt to the eight XCDs in
// contiguous eighths - block b runs on XCD b % 8 - so a level's table slice is served by the L2 of one XCD, two when an eighth boundary cuts the level, and every XCD has
// the same number of units whatever the number of levels (6 fine and 10 run levels with the bench table: 0.75 and 1.25 levels per XCD).
struct FwdSel { uint32_t level[16]; uint32_t m; };
__device__ __forceinline__ bool sel_block(const FwdSel &sel, uint32_t nblk, uint32_t &level, uint32_t &chunk) {
	const uint32_t units = sel.m * nblk, per = (units + 7u) >> 3;
	const uint32_t u = (blockIdx.x & 7u) * per + (blockIdx.x >> 3);
	if (u >= units) return false;
	const uint32_t li = u / nblk;
	chunk = u - li * nblk;
	level = sel.level[li];
	return true;
}

// All sixteen levels in one launch, the XCDs in PAIRS (k_hash_fwd_x2's default map for the fp32 table): XCD x and XCD 7 - x share the four levels 15 - p, 8 + p, 7 - p and
// p (p = min(x, 7 - x)), finest first, one taking the even chunks of each and the other the odd ones.  block_to_level_chunk hands XCD x the levels 15 - x and x whole, and
// a level costs the more the finer it is - a 2^18-sample training batch: 2.3 us at full machine width for every level up to res 300, 2.6 - 5.3 us for res 407 - 2048
// (profiles/r10_hash_fwd.md) - so XCD 0 (levels 15 and 0) is busy for 7.6 us x 8 = 60.6 us, which IS the launch's time, while XCD 7 (levels 8 and 7) idles after
// 4.5 us x 8.  The four levels of a pair sum to 12.1, 11.8, 11.6 and 11.3 us: 48 us at best, 50.6 measured.  A level's table slice is then served by two L2s instead
// of one; groups of four and of all eight XCDs balance better on paper and measured slower (53 - 54 us; the refresh query +5 % with all eight).  In closed form: the launch
// has 131 k wavefronts of 32 samples, and a map that cost a few hundred scalar instructions per wavefront cost 20 us.  Speed only, never results: every (level, chunk) has
// exactly one workgroup under either map.  Needs 32 * ceil(nblk / 2) workgroups.
__device__ __forceinline__ bool block_to_level_chunk_paired(uint32_t nblk, uint32_t &level, uint32_t &chunk) {
	const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3, per = (nblk + 1u) >> 1;
	const uint32_t p = xcd < 4u ? xcd : 7u - xcd, phase = slot / per;
	level = (phase & 1u) ? 8u - 8u * (phase >> 1) + p : 15u - 8u * (phase >> 1) - p;       // 15 - p, 8 + p, 7 - p, p
	chunk = 2u * (slot - phase * per) + (xcd >> 2);
	return phase < 4u && chunk < nblk;
}

// The positions of a whole window (first % RUN_K == 0, stride 3, 16-byte aligned base) as one 96-byte block, and of one sample at any stride.  run_load
// (hash_bwd_common.h) has the same two loads interleaved with its gradient loads; calling these from there was tried and changed the code of all eight backward run
// kernels (register allocation), so the backward keeps its text and the forward has its own.
__device__ __forceinline__ void run_pos_wide(const float *pos, uint32_t first, float (&px)[RUN_K][3]) {
	const float4 *p4 = reinterpret_cast<const float4 *>(pos + (size_t)first * 3);
	float4 v[6];
#pragma unroll
	for (int r = 0; r < 6; ++r) v[r] = p4[r];
	const float *f = reinterpret_cast<const float *>(v);
#pragma unroll
	for (uint32_t k = 0; k < RUN_K; ++k) { px[k][0] = f[3 * k]; px[k][1] = f[3 * k + 1]; px[k][2] = f[3 * k + 2]; }
}
__device__ __forceinline__ void run_pos_one(const float *pos, uint32_t stride, uint32_t i, float (&px)[3]) {
	px[0] = pos[(size_t)i * stride]; px[1] = pos[(size_t)i * stride + 1]; px[2] = pos[(size_t)i * stride + 2];
}

// wide: bit 0 = the positions can be read as 16-byte words (stride 3, 16-byte aligned base), bit 1 = a window's eight SOA feature pairs are 64 aligned contiguous bytes
template <typename T, int LAYOUT>
__global__ __launch_bounds__(FWD_RUN_WG) void k_hash_fwd_runs(uint32_t n, const float *__restrict__ pos, uint32_t stride, const T *__restrict__ table, LevelTable lt,
                                                              T *__restrict__ out, uint32_t nblk, const uint32_t *__restrict__ n_valid, FwdSel sel, uint32_t wide) {
	static_assert(sizeof(T) == 4, "the run forward reads the fp32 table; the fp16 table keeps k_hash_fwd's pair loads");
	uint32_t level, chunk;
	if (!sel_block(sel, nblk, level, chunk)) return;
	const uint32_t lim = valid_count(n, n_valid);
	const uint32_t off = lt.v[4 * level], size = lt.v[4 * level + 1], res = lt.v[4 * level + 2];
	const float scale = __uint_as_float(lt.v[4 * level + 3]);
	const bool dense = level_is_dense(size, res);
	const float2 *tab = reinterpret_cast<const float2 *>(table) + off;
	float2 *o = reinterpret_cast<float2 *>(out);
	// nblk is capped by the host: a workgroup takes chunks chunk, chunk + nblk, ... of its level (64-bit: n may be close to 2^32)
	for (uint64_t base = (uint64_t)chunk * FWD_RUN_SPAN; base < lim; base += (uint64_t)nblk * FWD_RUN_SPAN) {
		const uint64_t first64 = base + threadIdx.x * RUN_K;
		if (first64 >= lim) continue;
		const uint32_t first = (uint32_t)first64, live = min(lim - first, RUN_K);      // rows from lim on are neither read nor written
		const bool whole = live == RUN_K;
		float p[RUN_K][3];
		if (whole && (wide & 1u)) run_pos_wide(pos, first, p);
		else {
#pragma unroll
			for (uint32_t k = 0; k < RUN_K; ++k) {
				if (k < live) run_pos_one(pos, stride, first + k, p[k]);
				else p[k][0] = p[k][1] = p[k][2] = 0.f;
			}
		}
#pragma unroll
		for (uint32_t k = 0; k < RUN_K; ++k)
#pragma unroll
			for (int d = 0; d < 3; ++d) p[k][d] = p[k][d] * scale + 0.5f;               // pos_fract, HashEncode.h:106-115 (locate)
		// every run's gathers, issued before the first use
		float2 v[RUN_K][8];
		bool open[RUN_K];
		uint32_t prev[3] = {0u, 0u, 0u};
#pragma unroll
		for (uint32_t k = 0; k < RUN_K; ++k) {
			uint32_t c[3];
#pragma unroll
			for (int d = 0; d < 3; ++d) c[d] = (uint32_t)(int)floorf(p[k][d]);
			open[k] = k < live && (k == 0 || c[0] != prev[0] || c[1] != prev[1] || c[2] != prev[2]);
#pragma unroll
			for (int d = 0; d < 3; ++d) prev[d] = c[d];
#pragma unroll
			for (uint32_t q = 0; q < 8; ++q) v[k][q] = make_float2(0.f, 0.f);
			if (open[k]) {
#pragma unroll
				for (uint32_t q = 0; q < 8; ++q) v[k][q] = tab[grid_index(size, res, dense, c[0] + (q & 1u), c[1] + ((q >> 1) & 1u), c[2] + (q >> 2))];   // corner q = x + 2 y + 4 z
			}
		}
		// every sample with its own weights and the corners of its run
		float2 cur[8], r[RUN_K];
#pragma unroll
		for (uint32_t q = 0; q < 8; ++q) cur[q] = make_float2(0.f, 0.f);
#pragma unroll
		for (uint32_t k = 0; k < RUN_K; ++k) {
#pragma unroll
			for (uint32_t q = 0; q < 8; ++q) if (open[k]) cur[q] = v[k][q];
			float w[3];
#pragma unroll
			for (int d = 0; d < 3; ++d) w[d] = p[k][d] - floorf(p[k][d]);
			float2 acc = make_float2(0.f, 0.f);
#pragma unroll
			for (uint32_t j = 0; j < 4; ++j) {                                          // k_hash_fwd's arithmetic: the reference's x, y, z multiplication order, terms 2 j and 2 j + 1 in turn
				const float wy = (j & 1u) ? w[1] : 1 - w[1], wz = (j >> 1) ? w[2] : 1 - w[2];
				const float w0 = ((1 - w[0]) * wy) * wz, w1 = (w[0] * wy) * wz;
				acc.x += w0 * cur[2 * j].x; acc.y += w0 * cur[2 * j].y;
				acc.x += w1 * cur[2 * j + 1].x; acc.y += w1 * cur[2 * j + 1].y;
			}
			r[k] = acc;
		}
		if (LAYOUT == NGP_LAYOUT_SOA) {
			float2 *dst = o + (size_t)level * n + first;
			if (whole && (wide & 2u)) {
				float4 *d4 = reinterpret_cast<float4 *>(dst);
#pragma unroll
				for (uint32_t h = 0; h < RUN_K / 2; ++h) d4[h] = make_float4(r[2 * h].x, r[2 * h].y, r[2 * h + 1].x, r[2 * h + 1].y);
			} else {
#pragma unroll
				for (uint32_t k = 0; k < RUN_K; ++k) if (k < live) dst[k] = r[k];
			}
		} else {
#pragma unroll
			for (uint32_t k = 0; k < RUN_K; ++k) if (k < live) o[(size_t)(first + k) * 16 + level] = r[k];
		}
	}
}
