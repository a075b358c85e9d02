// Shared by the three designs of the table-gradient scatter (hash_encode.hip: the atomics kernel and the launch code; hash_bwd_percorner.h: per-corner record lists,
// fp16 dL/dy; hash_bwd_regions.h: record regions, fp32 dL/dy): the bins' constants and plan structs, the small loads every kernel of the stage repeats, the abs-max pass,
// cell_entries, the fixed-point helpers, the riding Adam update and the RUN-COMBINING CORE of the two coarse-level record kernels.
#pragma once
#include "hash_common.h"
#include "mlp_tail.h"

#define BIN_BITS 13u
#define BIN_ENTRIES (1u << BIN_BITS)
#define BINS_PER_LEVEL 64u
#define BIN_LEVEL_MAX (BIN_ENTRIES * BINS_PER_LEVEL)                  // 2^19 entries: the largest level the bins cover
#define RUN_RES_MAX 300u                                              // levels up to this resolution go through the run-combining kernels (k_bin_records_runs / k_bin_runs2)
static_assert(RUN_RES_MAX == NGP_DP_COARSE_RES_MAX, "the data-parallel bucket boundary (ngp_dp_plan) is the boundary between the run-combined and the fine levels");
// One cursor per bin.  (r4 tried eight sub-lists with a cursor each, on the theory that same-address atomics queue behind each other: no change for the record kernels,
// +5 us for the accumulate's eight-way gather - the cost of these reservations is their NUMBER, see the edge records in hash_bwd_regions.h.  CUR_SUBS is kept as the switch.)
#define CUR_SUBS 1u
#define N_CURSORS (16u * BINS_PER_LEVEL * CUR_SUBS)                       // u32 cursors of a workspace: [16][64][CUR_SUBS]
#define N_ZEROED (N_CURSORS + 16u)                                        // (+ spare words) zeroed together with the cursors every step
struct BinPlan { uint32_t level[16]; uint32_t n_levels; uint32_t cap; uint32_t spill_cap; };   // binned levels, records per bin, entries of the spill list
struct LevelSel { uint32_t hl[16]; };                                  // the binned-level ordinals one launch works on (blockIdx.y, or blockIdx.x / 64)
struct SpillEntry { uint32_t key /* binned-level ordinal << 19 | entry */; float x, y; };       // value in record units (fp16 records: scaled)

// samples a kernel works on: all n, or the device-side count when the caller passes one
__device__ __forceinline__ uint32_t valid_count(uint32_t n, const uint32_t *n_valid) { uint32_t lim = n; if (n_valid) { uint32_t nv = *n_valid; lim = nv < n ? nv : n; } return lim; }
// dL/dy pair of (sample i + k, level): level-major [16][n] or the [n,32] rows
template <int LAYOUT, typename P>
__device__ __forceinline__ P load_dy(const P *dy, uint32_t n, uint32_t level, uint32_t i, uint32_t k = 0u) { return LAYOUT == NGP_LAYOUT_SOA ? dy[(size_t)level * n + i + k] : dy[(size_t)(i + k) * 16 + level]; }

__device__ __forceinline__ float bin_scale(uint32_t absmax_bits) {     // power of two s with 2^13 <= max*s < 2^14 (0 if the level has no gradient)
	const float m = __uint_as_float(absmax_bits);
	if (!(m > 0.f) || !(m < 3.0e38f)) return 0.f;
	int ex; frexpf(m, &ex);                                           // m = f * 2^ex, f in [0.5, 1)
	return ldexpf(1.0f, 14 - ex);
}

// Largest |dL/dy| of every level (the scale of the fixed-point accumulation).  Every workgroup writes the maximum of its share of the samples to ABSMAX_PARTS
// partial slots per level - no atomics (same-address global atomics retire one at a time at the L2: 8192 of them on 16 addresses took ~90 us), nothing to zero
// beforehand; the consumers take the maximum of a level's partials with scalar loads (level_absmax).  The pass also zeroes the record cursors and the spill
// count for the kernels behind it in the stream (that was a separate 5 us memset launch).
#define ABSMAX_PARTS NGP_ABSMAX_PARTS
#define ABSMAX_OWN_PARTS 64u                                                    // partials the scatter's own pass writes (its grid); the remaining slots are zeroed by it
__device__ __forceinline__ uint32_t level_absmax(const uint32_t *__restrict__ parts, uint32_t level) {      // positive floats order like their bit patterns
	const uint4 q = reinterpret_cast<const uint4 *>(parts + level * ABSMAX_PARTS)[threadIdx.x & 63u];         // four partials per lane + a wavefront reduction (called by full wavefronts, at kernel entry)
	uint32_t m = max(max(q.x, q.y), max(q.z, q.w));
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o));
	return m;
}
template <typename T, int LAYOUT>
__global__ __launch_bounds__(256) void k_level_absmax(uint32_t n, const T *__restrict__ dLdy, uint32_t *__restrict__ parts, const uint32_t *__restrict__ n_valid,
                                                      uint32_t *__restrict__ cursors, uint32_t *__restrict__ spill_count) {
	using P = typename Pair<T>::type;
	const uint32_t level = blockIdx.y;
	if (blockIdx.x == 0) {                                               // this level's sixteenth of the cursors, spill count
		for (uint32_t j = threadIdx.x; j < N_CURSORS / 16u; j += 256u) cursors[level * (N_CURSORS / 16u) + j] = 0u;
		if (level == 0 && threadIdx.x < N_ZEROED - N_CURSORS) cursors[N_CURSORS + threadIdx.x] = 0u;
		if (level == 0 && threadIdx.x == BINS_PER_LEVEL) *spill_count = 0u;
	}
	const uint32_t lim = valid_count(n, n_valid);
	const P *dy = reinterpret_cast<const P *>(dLdy);
	float m = 0.f;
	const uint32_t step = gridDim.x * 256u;
	uint32_t i = blockIdx.x * 256u + threadIdx.x;
	for (; i + 3 * step < lim; i += 4 * step) {                        // four independent loads in flight
		float2 g[4];
#pragma unroll
		for (int u = 0; u < 4; ++u) g[u] = to_f2(load_dy<LAYOUT>(dy, n, level, i, u * step));
#pragma unroll
		for (int u = 0; u < 4; ++u) m = fmaxf(m, fmaxf(fabsf(g[u].x), fabsf(g[u].y)));
	}
	for (; i < lim; i += step) {
		const float2 g = to_f2(load_dy<LAYOUT>(dy, n, level, i));
		m = fmaxf(m, fmaxf(fabsf(g.x), fabsf(g.y)));
	}
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
	__shared__ float wave_max[4];
	if ((threadIdx.x & 63u) == 0) wave_max[threadIdx.x >> 6] = m;
	__syncthreads();
	if (threadIdx.x == 0) {
		m = fmaxf(fmaxf(wave_max[0], wave_max[1]), fmaxf(wave_max[2], wave_max[3]));
		parts[level * ABSMAX_PARTS + blockIdx.x] = (m > 0.f) ? __float_as_uint(m) : 0u;     // (NaN -> 0: a level without a usable gradient is skipped, as before)
	}
	if (threadIdx.x >= 1 && threadIdx.x < ABSMAX_PARTS / ABSMAX_OWN_PARTS) parts[level * ABSMAX_PARTS + blockIdx.x + threadIdx.x * ABSMAX_OWN_PARTS] = 0u;   // the slots of the (larger) fused producer's grid
}

// the eight entries of the cell whose lowest corner is (gx, gy, gz): level-wide indices (HashEncode.h:68-94)
__device__ __forceinline__ void cell_entries(uint32_t size, uint32_t res, bool dense, uint32_t gx, uint32_t gy, uint32_t gz, uint32_t idx[8]) {
	if (dense) {
		const uint32_t y0 = gy * res, z0 = gz * res * res;
#pragma unroll
		for (uint32_t q = 0; q < 8; ++q) {
			uint32_t e = (gx + (q & 1u)) + (y0 + ((q & 2u) ? res : 0u)) + (z0 + ((q & 4u) ? res * res : 0u));
			if (e >= size) { e -= size; if (e >= size) e %= size; }              // wraps only at the +1 boundary corner
			idx[q] = e;
		}
	} else {
		const uint32_t ty0 = gy * 19349663u, tz0 = gz * 83492791u;
#pragma unroll
		for (uint32_t q = 0; q < 8; ++q) idx[q] = ((gx + (q & 1u)) ^ (ty0 + ((q & 2u) ? 19349663u : 0u)) ^ (tz0 + ((q & 4u) ? 83492791u : 0u))) & (size - 1u);
	}
}

// ---------------------------------------------------------------------------------------------------------------- the run-combining core (coarse levels, both workspace paths)
// One thread per RUN_K consecutive samples: the samples of a ray are consecutive in the batch and a cell of a level with res <= 300 is 3-40 marching steps long, so the
// thread sums the runs that share a cell in registers and emits one set of eight fp32 contributions per run.  The number of records a workgroup produces is data dependent
// (2048 samples: 2048 on the coarsest levels, 16384 for scattered positions), so a kernel runs the sweep twice over the registers: COUNT (LDS histogram of the bins) - a
// prefix or reservation - PLACE.  What a kernel does with the emitted contributions (its bins, its LDS layout, where its records go) is the kernel's own:
// k_bin_records_runs (hash_bwd_percorner.h) and both forms of k_bin_runs2 (hash_bwd_regions.h).
#define RUN_K 8u
#define RUN_WG 256u
// The thread's eight samples.  KEEP_P = false: cell and fraction per sample (48 registers).  KEEP_P = true: p = pos * scale + 0.5 (24 registers); every sweep takes cell
// and fraction from it again (k_bin_runs2's V2 form: nothing spills at five waves per SIMD).  Same values either way.
template <bool KEEP_P> struct RunSamples {
	float2 gk[RUN_K];
	uint32_t cell[KEEP_P ? 1 : RUN_K][3]; float frac[KEEP_P ? 1 : RUN_K][3]; float pp[KEEP_P ? RUN_K : 1][3];
};
// samples first .. first + RUN_K - 1 of `level` (first % RUN_K == 0); samples from lim on are zero rows
template <typename T, int LAYOUT, bool KEEP_P>
__device__ __forceinline__ void run_load(RunSamples<KEEP_P> &rs, uint32_t n, const float *pos, uint32_t stride, const T *dLdy, uint32_t level, float scale, uint32_t first, uint32_t lim) {
	using P = typename Pair<T>::type;
	const P *dy = reinterpret_cast<const P *>(dLdy);
	float px[RUN_K][3];
	if (first + RUN_K <= lim && stride == 3) {
		const float4 *p4 = reinterpret_cast<const float4 *>(pos + (size_t)first * 3);   // 24 floats, 16-byte aligned (first % 8 == 0)
		float4 v[6];
#pragma unroll
		for (int r = 0; r < 6; ++r) v[r] = p4[r];
		const float *f = reinterpret_cast<const float *>(v);
#pragma unroll
		for (uint32_t k = 0; k < RUN_K; ++k) { px[k][0] = f[3 * k]; px[k][1] = f[3 * k + 1]; px[k][2] = f[3 * k + 2]; }
		if (LAYOUT == NGP_LAYOUT_SOA && sizeof(P) == 8 && (n & 1u) == 0u) {       // (r6) level-major fp32 gradients: the thread's eight pairs are 64 contiguous, 16-byte aligned bytes - four loads instead of eight
			const float4 *g4 = reinterpret_cast<const float4 *>(dy + (size_t)level * n + first);
			float4 u[4];
#pragma unroll
			for (int r = 0; r < 4; ++r) u[r] = g4[r];
#pragma unroll
			for (int r = 0; r < 4; ++r) { rs.gk[2 * r] = make_float2(u[r].x, u[r].y); rs.gk[2 * r + 1] = make_float2(u[r].z, u[r].w); }
		} else {
#pragma unroll
			for (uint32_t k = 0; k < RUN_K; ++k) rs.gk[k] = to_f2(load_dy<LAYOUT>(dy, n, level, first, k));
		}
	} else {
#pragma unroll
		for (uint32_t k = 0; k < RUN_K; ++k) {
			const uint32_t i = first + k;
			if (i < lim) {
				px[k][0] = pos[(size_t)i * stride]; px[k][1] = pos[(size_t)i * stride + 1]; px[k][2] = pos[(size_t)i * stride + 2];
				rs.gk[k] = to_f2(load_dy<LAYOUT>(dy, n, level, i));
			} else { px[k][0] = px[k][1] = px[k][2] = 0.f; rs.gk[k] = make_float2(0.f, 0.f); }
		}
	}
#pragma unroll
	for (uint32_t k = 0; k < RUN_K; ++k)
#pragma unroll
		for (int d = 0; d < 3; ++d) {                                                  // pos_fract, HashEncode.h:106-115
			const float p = px[k][d] * scale + 0.5f;
			if constexpr (KEEP_P) rs.pp[k][d] = p; else { const float fl = floorf(p); rs.cell[k][d] = (uint32_t)(int)fl; rs.frac[k][d] = p - fl; }
		}
}
// one sweep over the thread's samples; emit(entry, x, y) is called for the eight corners of every finished run
template <bool KEEP_P, typename F>
__device__ __forceinline__ void run_sweep(const RunSamples<KEEP_P> &rs, uint32_t size, uint32_t res, bool dense, F emit) {
	bool open = false;
	uint32_t key[3] = {0u, 0u, 0u};
	float ax[8], ay[8];
	auto flush = [&]() {
		uint32_t idx[8];
		cell_entries(size, res, dense, key[0], key[1], key[2], idx);
#pragma unroll
		for (uint32_t q = 0; q < 8; ++q) emit(idx[q], ax[q], ay[q]);
	};
#pragma unroll
	for (uint32_t k = 0; k < RUN_K; ++k) {
		if (rs.gk[k].x == 0.f && rs.gk[k].y == 0.f) continue;        // zero rows (padding) add exact zeros in the reference: skipped, they do not end a run either
		uint32_t ck[3]; float fk[3];
#pragma unroll
		for (int d = 0; d < 3; ++d) {
			if constexpr (KEEP_P) { const float fl = floorf(rs.pp[k][d]); ck[d] = (uint32_t)(int)fl; fk[d] = rs.pp[k][d] - fl; }
			else { ck[d] = rs.cell[k][d]; fk[d] = rs.frac[k][d]; }
		}
		if (open && !(ck[0] == key[0] && ck[1] == key[1] && ck[2] == key[2])) { flush(); open = false; }
		if (!open) {
			open = true; key[0] = ck[0]; key[1] = ck[1]; key[2] = ck[2];
#pragma unroll
			for (uint32_t q = 0; q < 8; ++q) { ax[q] = 0.f; ay[q] = 0.f; }
		}
		const float x1 = fk[0], x0 = 1 - x1, y1 = fk[1], y0 = 1 - y1, z1 = fk[2], z0 = 1 - z1;
#pragma unroll
		for (uint32_t q = 0; q < 8; ++q) {
			const float w = ((q & 1u) ? x1 : x0) * ((q & 2u) ? y1 : y0) * ((q & 4u) ? z1 : z0);                 // the reference's x, y, z multiplication order
			ax[q] += rs.gk[k].x * w; ay[q] += rs.gk[k].y * w;
		}
	}
	if (open) flush();
}

// ---------------------------------------------------------------------------------------------------------------- fixed point (the accumulate kernels)
// value of one record in the accumulator's integer unit.  fp16 records: multiples of 2^-24 (exact).  fp32 records: fixed point at `s32` = 2^38 / (binade of the level's largest |dL/dy|): a contribution of that size keeps all 24 bits of its
// fp32 significand, one 2^-16 of it still keeps 8, and a 64-bit sum of 2^21 run records of <= 8 samples cannot overflow.
__device__ __forceinline__ void rec_to_fixed(__half2 v, float, long long &ix, long long &iy) {
	const float2 f = __half22float2(v);
	ix = (long long)(f.x * 16777216.0f); iy = (long long)(f.y * 16777216.0f);
}
__device__ __forceinline__ void rec_to_fixed(float2 v, float s32, long long &ix, long long &iy) { ix = __float2ll_rn(v.x * s32); iy = __float2ll_rn(v.y * s32); }
// c * s (s a power of two) rounded to the nearest integer (ties to even), as a 64-bit integer: __float2ll_rn without the generic expansion.  t = c * s is exact, rint(t) is
// an integer-valued float with <= 24 significant bits, so its split into hi * 2^32 + lo is exact too.  |t| < 2^62 by construction of the scale.
__host__ __device__ __forceinline__ long long fixed_rn(float c, float s) {
	const float r = rintf(c * s), m = fabsf(r);
	const float hi = floorf(m * 2.3283064365386963e-10f);               // floor(|r| / 2^32)
	const float lo = fmaf(hi, -4294967296.0f, m);                        // |r| - hi * 2^32, in [0, 2^32): exact (a multiple of ulp(|r|) below 2^32)
	const long long v = (long long)(((unsigned long long)(uint32_t)hi << 32) | (unsigned long long)(uint32_t)lo);
	return r < 0.f ? -v : v;
}

// (r6) ADAM: the table's Adam + EMA sweep rides in the accumulate kernels of both workspace paths (see k_bin_accumulate2, hash_bwd_regions.h): the entries a thread would
// store the gradient of get optim.hip's update instead - fp32 master, both moments and, when the table has one, the fp16 shadow the gathers read.
__device__ __forceinline__ void adam_ride_update(float &p, float &m, float &v, float g, const AdamRide &ar) {
	float e = p;
	if (ar.ema) adam_ema_update<true>(p, m, v, e, g, ar.c); else adam_ema_update<false>(p, m, v, e, g, ar.c);
}
