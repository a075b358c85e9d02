// Multiresolution hash-grid encode, forward + backward, for gfx950.
//
// What it computes: position_encoders/hash_encoder/op_header/HashEncode.h:117-203 (kernel_grid) and :299-396
// (kernel_grid_backward) of the reference, with the level table (offset/size/resolution/scale) precomputed on the host.
//
// MI355X design (not the reference's launch shape):
//  * one thread = one (sample, level); a workgroup works on ONE level so its gathers stay inside that level's slice of the
//    table (<= 2 MiB fp16 / 4 MiB fp32) ...
//  * ... and the blockIdx -> (level, chunk) map is XCD-aware: the dispatcher places block b on XCD b%8 and each XCD has a
//    private 4 MiB L2, so XCD x is handed level 15-x for ALL sample chunks first and level x afterwards.  A level's table
//    slice is then fetched from HBM/Infinity-Cache once per XCD and served out of that XCD's L2 for the rest of the pass
//    instead of being bounced between eight L2s.  This mapping affects speed only, never results.  (r10) k_hash_fwd_x2, the fp32 forward, pairs the XCDs instead - XCD x and
//    7 - x share four levels - because "15-x, then x" left seven XCDs waiting for XCD 0 (hash_fwd_runs.h: block_to_level_chunk_paired).
//  * no extract_position / transpose kernels: positions are read strided from the caller's buffer and features are written
//    either as the [n,32] rows HashEncoder returns or as a level-major [16][n] stream of pairs that the fused MLP consumes with
//    fully coalesced 256-B wave accesses (no 4-byte-per-64-byte-line partial writes from sixteen different XCDs).
//  * backward (this file: the atomics kernel, workspace layout, routing, the launch code of the three schemes; the record and accumulate kernels live in headers by
//    path - hash_bwd_common.h, hash_bwd_percorner.h, hash_bwd_regions.h - and this file stays the one translation unit): chosen by what the caller hands over
//    (hash_bwd_impl).  With a workspace (the training path): a binned scatter without any float atomic - every
//    contribution computed once, written as a record for the bin its entry lives in, summed per bin in 64-bit integer LDS accumulators, coarse levels with per-thread run
//    combining; bit-reproducible.  fp32 dL/dy (ngp_base.py), round 4: record REGIONS - no global atomic of any kind, one 16-byte record per cell edge on the fine levels, one
//    accumulate kernel for all levels (k_bin_runs2 / k_bin_pairs / k_bin_accumulate2).  fp16 dL/dy (ngp_fox.py): round 2/3's per-corner record lists with cursor
//    reservations (k_bin_records_runs / k_bin_records / k_bin_accumulate).  Without a workspace, with NGP_HASH_BWD_ATOMICS=1, or for a table the bins cannot take (a level
//    beyond 2^19 entries, a hashed table that is not a power of two): the reference's scheme, one global float atomic per corner (k_hash_bwd) - the ONE fallback since the
//    owner-computes scan of rounds 1-2 was deleted in round 5.  (r6) On the single-GPU training path the accumulate kernels of both workspace designs also apply the
//    table's Adam + EMA sweep in place of the gradient store (AdamRide: k_bin_accumulate2<float, true>, k_bin_accumulate<float, RV, true>).
#include "ngp_common.h"
#include <stdlib.h>
#include <string.h>
#include <mutex>
#pragma clang fp contract(off)

#include "hash_bwd_common.h"
#include "hash_bwd_percorner.h"
#include "hash_bwd_regions.h"
#include "hash_fwd_runs.h"

template <typename T, int LAYOUT>
__device__ __forceinline__ void hash_fwd_body(uint32_t n, const float *__restrict__ pos, uint32_t stride, const T *__restrict__ table, const LevelTable &lt,
                                              T *__restrict__ out, uint32_t nblk, const uint32_t *__restrict__ n_valid, uint32_t level, uint32_t chunk, float *__restrict__ dy_dx = nullptr);
// forward with d(encoding)/d(position) - the dy_dx branch of the reference's kernel_grid (HashEncode.h:205-251): same gathers, three more outputs per (sample, level)
template <typename T, int LAYOUT>
__global__ __launch_bounds__(256) void k_hash_fwd_dydx(uint32_t n, const float *__restrict__ pos, uint32_t stride, const T *__restrict__ table, LevelTable lt,
                                                       T *__restrict__ out, uint32_t nblk, const uint32_t *__restrict__ n_valid, float *__restrict__ dy_dx) {
	uint32_t level, chunk; block_to_level_chunk(nblk, level, chunk);
	hash_fwd_body<T, LAYOUT>(n, pos, stride, table, lt, out, nblk, n_valid, level, chunk, dy_dx);
}
template <typename T, int LAYOUT>
__global__ __launch_bounds__(256) void k_hash_fwd(uint32_t n, const float *__restrict__ pos, uint32_t stride, const T *__restrict__ table, LevelTable lt,
                                                  T *__restrict__ out, uint32_t nblk, const uint32_t *__restrict__ n_valid) {
	uint32_t level, chunk; block_to_level_chunk(nblk, level, chunk);
	hash_fwd_body<T, LAYOUT>(n, pos, stride, table, lt, out, nblk, n_valid, level, chunk);
}
template <typename T, int LAYOUT>
__device__ __forceinline__ void hash_fwd_body(uint32_t n, const float *__restrict__ pos, uint32_t stride, const T *__restrict__ table, const LevelTable &lt,
                                              T *__restrict__ out, uint32_t nblk, const uint32_t *__restrict__ n_valid, uint32_t level, uint32_t chunk, float *__restrict__ dy_dx) {
	using P = typename Pair<T>::type;
	uint32_t lim = n; if (n_valid) { uint32_t nv = *n_valid; lim = nv < n ? nv : n; }
	const uint32_t off = lt.v[4 * level], size = lt.v[4 * level + 1], res = lt.v[4 * level + 2];
	const float scale = __uint_as_float(lt.v[4 * level + 3]);
	const bool dense = level_is_dense(size, res);
	const P *tab = reinterpret_cast<const P *>(table) + off;
	// nblk is capped by the host: a block takes chunks chunk, chunk + nblk, ... of its level (one trip for a training batch; the fixed-capacity inference buffers
	// - 4 M rows of which a device-side count says how many are valid - used to launch 260 k blocks of which 87 % found nothing to do)
	for (uint32_t i = chunk * 256u + threadIdx.x; i < lim; i += nblk * 256u) {
	const Corner c = locate(pos, stride, i, scale);
	P v[8]; float w[8];
	// The two x-neighbours of a cell edge are adjacent in memory on dense levels (index x + ...; not across the wrap) and on hashed levels when x is even
	// ((x+1) ^ h == (x ^ h) ^ 1 then).  fp16 table: they are fetched with ONE 8-byte load then - 6 requests per (sample, level) on average instead of 8; the second single load
	// is issued only by the other lanes.  fp32 table (r5): NOT - rounds 1-4 used 16-byte loads there and measured them against nothing; an A/B in one call
	// (profiles/r05e_wide_loads_ab.txt) has the plain eight 8-byte loads FASTER (k_hash_fwd 101 -> 86 us per iteration incl. the refresh share, +2.4 % it/s: the three-way
	// branch serialises a wavefront's loads), and the 16-byte gathers were the one thing that made this kernel return wrong values for a quarter wavefront while ANOTHER PROCESS
	// trained with this package on the same GPU (profiles/r05d_shared_gpu.txt, DESIGN.md 6: 506 of 2909 launches with them, 0 of 3369 without; alone, or with two streams in one
	// process, never).  -DNGP_PROBE_WIDE_LOADS_F32 rebuilds the old kernel for that diagnosis (tools/probe_shared_gpu.sh).
	struct alignas(sizeof(P)) PP { P a, b; };
#ifdef NGP_PROBE_WIDE_LOADS_F32
	constexpr bool WIDE = true;
#else
	constexpr bool WIDE = sizeof(P) == 4;
#endif
	const bool pow2 = (size & (size - 1)) == 0;
#pragma unroll
	for (uint32_t j = 0; j < 4; ++j) {        // j = (y corner, z corner); all gathers are issued before the first use
		const uint32_t gy = c.g[1] + (j & 1u), gz = c.g[2] + (j >> 1);
		const float wy = (j & 1u) ? c.w[1] : 1 - c.w[1], wz = (j >> 1) ? c.w[2] : 1 - c.w[2];
		w[2 * j] = ((1 - c.w[0]) * wy) * wz; w[2 * j + 1] = (c.w[0] * wy) * wz;          // the reference's x, y, z multiplication order
		const uint32_t i0 = grid_index(size, res, dense, c.g[0], gy, gz), i1 = grid_index(size, res, dense, c.g[0] + 1, gy, gz);
		const bool adjacent_up = WIDE && i1 == i0 + 1u && (dense || pow2), adjacent_dn = WIDE && i0 == i1 + 1u && !dense && pow2;     // (x^h)^1 is either one above or one below
		if (adjacent_up) { const PP t = *reinterpret_cast<const PP *>(tab + i0); v[2 * j] = t.a; v[2 * j + 1] = t.b; }
		else if (adjacent_dn) { const PP t = *reinterpret_cast<const PP *>(tab + i1); v[2 * j] = t.b; v[2 * j + 1] = t.a; }
		else { v[2 * j] = tab[i0]; v[2 * j + 1] = tab[i1]; }
	}
	float2 acc = make_float2(0.f, 0.f);
#pragma unroll
	for (uint32_t k = 0; k < 8; ++k) { float2 f = to_f2(v[k]); acc.x += w[k] * f.x; acc.y += w[k] * f.y; }
	P r; from_f2(r, acc);
	P *o = reinterpret_cast<P *>(out);
	if (LAYOUT == NGP_LAYOUT_SOA) o[(size_t)level * n + i] = r;
	else o[(size_t)i * 16 + level] = r;
	if (dy_dx) {
		// HashEncode.h:205-251: per derivative dimension the four (left, right) pairs along it, weight = scale * w(first other dim) * w(second other dim) in that order,
		// summed in the reference's idx order (bit 0 = first other dim).  v[k]: corner k = x + 2 y + 4 z, already in registers - no extra gathers.
		float2 f[8];
#pragma unroll
		for (uint32_t k = 0; k < 8; ++k) f[k] = to_f2(v[k]);
#pragma unroll
		for (uint32_t gd = 0; gd < 3; ++gd) {
			const uint32_t d0 = gd == 0 ? 1u : 0u, d1 = gd == 2 ? 1u : 2u;           // the two non-derivative dimensions, ascending
			float2 a = make_float2(0.f, 0.f);
#pragma unroll
			for (uint32_t idx = 0; idx < 4; ++idx) {
				const uint32_t b0 = idx & 1u, b1 = idx >> 1;
				float weight = scale;
				weight *= b0 ? c.w[d0] : 1 - c.w[d0];
				weight *= b1 ? c.w[d1] : 1 - c.w[d1];
				const uint32_t left = (b0 << d0) | (b1 << d1), right = left | (1u << gd);
				a.x += weight * (f[right].x - f[left].x) * 1.0f;
				a.y += weight * (f[right].y - f[left].y) * 1.0f;
			}
			*reinterpret_cast<float2 *>(dy_dx + (size_t)i * 96 + gd * 32 + 2 * level) = a;
		}
	}
	}
}

// (r6) fp32 table, two LANES per (sample, level): lane pair (2p, 2p + 1) = the cell's x = g and x = g + 1 faces, four 8-byte gathers each.  The forward gather is bound by
// the number of distinct cache lines a wavefront's load instruction names (~one line per clock through the CU's texture path: 33.5 M lines of a 2^18-sample batch = 54 us of
// the kernel's 65), and the two x-neighbours of a cell edge are adjacent 8-byte entries - always on a dense level, and on a hashed one whenever x is even
// ((x + 1) ^ h == (x ^ h) ^ 1) - i.e. ONE line.  One lane loading both (the 16-byte pair loads of rounds 1-4) needed a three-way branch that serialised the loads; two
// adjacent lanes loading one each in the SAME instruction are merged by the address coalescer with no branch at all: 6 lines per (sample, hashed level) on average instead
// of 8.  Bit-exact: the lanes swap halves (lane 2p ends up with every corner's first component, lane 2p + 1 with the second) and each sums its component's eight terms in the
// reference's order, k = x + 2 y + 4 z.
// (r10) MAP, the workgroup's (level, chunk): X2_MAP_LEVELS = block_to_level_chunk (XCD x: level 15 - x, then level x; rounds 6-9), X2_MAP_PAIRED = block_to_level_chunk_paired
// (two XCDs share four levels), X2_MAP_SEL = the levels of `sel` alone, dealt out by sel_block - the levels k_hash_fwd_runs does not take (both hash_fwd_runs.h).  `sel` is
// read by X2_MAP_SEL only.  Speed only: every (sample, level) is computed by one lane pair, the same way, under every map.
enum { X2_MAP_LEVELS = 0, X2_MAP_PAIRED = 1, X2_MAP_SEL = 2 };
// (r11) The KIND of a level - how a lattice point becomes a table entry - is the same for every sample of a workgroup, so it is decided once, outside the sample loop, and
// each kind has its own loop body: X2_DENSE = x + y res + z res^2 with grid_index's wrap of the +1 boundary corner (for a dense level whose size is a power of two the wrap
// is grid_index's mask: both are index % size), X2_HASH_POW2 = the XOR hash masked (every hashed level GridEncode builds: 2^19 entries), X2_GENERAL = grid_index as it is
// (a hashed level of any other size).  Same entries in every case; the additions below are grid_index's multiplications taken apart, in arithmetic modulo 2^32.
enum { X2_DENSE = 0, X2_HASH_POW2 = 1, X2_GENERAL = 2 };
#define X2_SIZE_MAX32 (1u << 28)      // the specialised bodies address an entry by a 32-bit byte offset (8 bytes per fp32 entry); a larger level is X2_GENERAL's
#ifndef NGP_HASH_FWD_DEPTH
#define NGP_HASH_FWD_DEPTH 2          // samples whose loads are in flight together per lane pair (measured 1 | 2 | 4: profiles/r11_hash_fwd_trips.md)
#endif
// the four entries of one x face of the cell: j = (y corner, z corner)
template <int KIND>
__device__ __forceinline__ void x2_face_entries(uint32_t size, uint32_t res, bool dense, uint32_t gx, uint32_t gy, uint32_t gz, uint32_t (&e)[4]) {
	if constexpr (KIND == X2_DENSE) {
		const uint32_t rr = res * res, b = gx + gy * res + gz * rr;
#pragma unroll
		for (uint32_t j = 0; j < 4; ++j) e[j] = b + ((j & 1u) ? res : 0u) + ((j >> 1) ? rr : 0u);
		// grid_index's wrap: taken by the +1 boundary corner only, the division never for in-range positions - one test for the four entries, the wrap itself per entry as there
		if (max(max(e[0], e[1]), max(e[2], e[3])) >= size) {
#pragma unroll
			for (uint32_t j = 0; j < 4; ++j) if (e[j] >= size) { e[j] -= size; if (e[j] >= size) e[j] %= size; }
		}
	} else if constexpr (KIND == X2_HASH_POW2) {
		const uint32_t hy = gy * 19349663u, hz = gz * 83492791u, mask = size - 1u;
#pragma unroll
		for (uint32_t j = 0; j < 4; ++j) e[j] = (gx ^ (hy + ((j & 1u) ? 19349663u : 0u)) ^ (hz + ((j >> 1) ? 83492791u : 0u))) & mask;
	} else {
#pragma unroll
		for (uint32_t j = 0; j < 4; ++j) e[j] = grid_index(size, res, dense, gx, gy + (j & 1u), gz + (j >> 1));
	}
}
// One trip of a lane pair: samples i, i + step, ... (NS of them, all below the count).  All NS samples' position loads are issued together, then all 4 NS gathers, then the
// arithmetic - one memory round trip for the positions and one for the table per trip instead of per sample.
template <typename T, int LAYOUT, int KIND, int NS>
__device__ __forceinline__ void x2_trip(uint32_t n, const float *__restrict__ pos, uint32_t stride, const typename Pair<T>::type *__restrict__ tab, uint32_t size, uint32_t res,
                                        bool dense, float scale, T *__restrict__ out, uint32_t level, uint32_t xc, uint32_t i, uint32_t step) {
	using P = typename Pair<T>::type;
	Corner c[NS];
#pragma unroll
	for (int s = 0; s < NS; ++s) c[s] = locate(pos, stride, i + (uint32_t)s * step, scale);
	P v[NS][4];
#pragma unroll
	for (int s = 0; s < NS; ++s) {
		uint32_t e[4];
		x2_face_entries<KIND>(size, res, dense, c[s].g[0] + xc, c[s].g[1], c[s].g[2], e);
#pragma unroll
		for (uint32_t j = 0; j < 4; ++j) {                                                 // every gather of the trip is issued before the first use
			if constexpr (KIND == X2_GENERAL) v[s][j] = tab[e[j]];
			else v[s][j] = *reinterpret_cast<const P *>(reinterpret_cast<const char *>(tab) + e[j] * (uint32_t)sizeof(P));   // a 32-bit byte offset (size <= X2_SIZE_MAX32): no 64-bit address arithmetic per gather
		}
	}
#pragma unroll
	for (int s = 0; s < NS; ++s) {
		float acc = 0.f;
#pragma unroll
		for (uint32_t j = 0; j < 4; ++j) {
			const float wy = (j & 1u) ? c[s].w[1] : 1 - c[s].w[1], wz = (j >> 1) ? c[s].w[2] : 1 - c[s].w[2];
			const float w0 = ((1 - c[s].w[0]) * wy) * wz, w1 = (c[s].w[0] * wy) * wz;    // the reference's x, y, z multiplication order
			const float2 f = to_f2(v[s][j]);
			const float own = xc ? f.y : f.x, give = xc ? f.x : f.y;
			// the partner's value of MY component: quad_perm [1, 0, 3, 2] on the vector pipe (rounds 6-10: __shfl_xor, a bpermute through the LDS pipe and its address register)
			const float got = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(give), 0xB1, 0xf, 0xf, true));
			acc += w0 * (xc ? got : own);                                                // corner k = 2 j     (x = g)
			acc += w1 * (xc ? own : got);                                                // corner k = 2 j + 1 (x = g + 1)
		}
		const uint32_t is = i + (uint32_t)s * step;
		const size_t o = (LAYOUT == NGP_LAYOUT_SOA ? (size_t)level * n + is : (size_t)is * 16 + level) * 2u + xc;
		if (sizeof(T) == 4) reinterpret_cast<float *>(out)[o] = acc;
		else reinterpret_cast<__half *>(out)[o] = __float2half_rn(acc);
	}
}
// The sample loop of one level kind: the lane pair takes samples first, first + step, ... below lim, NGP_HASH_FWD_DEPTH per trip while that many are left and one per trip
// after that.  Both lanes of a pair hold the same sample numbers, so they take the same trips of the same depth and the swap in x2_trip always has its partner - also in
// the wavefront that straddles lim, where the pairs disagree.  `left` counts down instead of the sample number counting up: no sum here can pass 2^32.
template <typename T, int LAYOUT, int KIND>
__device__ __forceinline__ void x2_samples(uint32_t n, uint32_t lim, const float *__restrict__ pos, uint32_t stride, const typename Pair<T>::type *__restrict__ tab, uint32_t size,
                                           uint32_t res, bool dense, float scale, T *__restrict__ out, uint32_t level, uint32_t first, uint32_t step) {
	constexpr uint32_t NS = NGP_HASH_FWD_DEPTH;
	const uint32_t xc = threadIdx.x & 1u;
	if (first >= lim) return;
	uint32_t i = first, left = lim - first;                                           // samples i, i + step, ... exist while k step < left
	if constexpr (NS > 1) {
		while (left > (NS - 1u) * step) {
			x2_trip<T, LAYOUT, KIND, (int)NS>(n, pos, stride, tab, size, res, dense, scale, out, level, xc, i, step);
			if (left <= NS * step) return;
			i += NS * step; left -= NS * step;
		}
	}
	for (;;) {
		x2_trip<T, LAYOUT, KIND, 1>(n, pos, stride, tab, size, res, dense, scale, out, level, xc, i, step);
		if (left <= step) return;
		i += step; left -= step;
	}
}
template <typename T, int LAYOUT, int MAP = X2_MAP_LEVELS>
__global__ __launch_bounds__(256) void k_hash_fwd_x2(uint32_t n, const float *__restrict__ pos, uint32_t stride, const T *__restrict__ table, LevelTable lt,
                                                     T *__restrict__ out, uint32_t nblk, const uint32_t *__restrict__ n_valid, FwdSel sel) {
	using P = typename Pair<T>::type;
	uint32_t level, chunk;
	if constexpr (MAP == X2_MAP_SEL) { if (!sel_block(sel, nblk, level, chunk)) return; }
	else if constexpr (MAP == X2_MAP_PAIRED) { if (!block_to_level_chunk_paired(nblk, level, chunk)) return; }
	else block_to_level_chunk(nblk, level, chunk);
	uint32_t lim = n; if (n_valid) { uint32_t nv = *n_valid; lim = nv < n ? nv : n; }
	const uint32_t off = lt.v[4 * level], size = lt.v[4 * level + 1], res = lt.v[4 * level + 2];
	const float scale = __uint_as_float(lt.v[4 * level + 3]);
	const bool dense = level_is_dense(size, res);
	const P *tab = reinterpret_cast<const P *>(table) + off;
	const uint32_t first = chunk * 128u + (threadIdx.x >> 1), step = nblk * 128u;   // (nblk <= 2^16: the host)
	const bool small = size <= X2_SIZE_MAX32;
	if (small && dense) x2_samples<T, LAYOUT, X2_DENSE>(n, lim, pos, stride, tab, size, res, true, scale, out, level, first, step);
	else if (small && (size & (size - 1u)) == 0u) x2_samples<T, LAYOUT, X2_HASH_POW2>(n, lim, pos, stride, tab, size, res, false, scale, out, level, first, step);
	else x2_samples<T, LAYOUT, X2_GENERAL>(n, lim, pos, stride, tab, size, res, dense, scale, out, level, first, step);
}

template <typename T, typename G, int LAYOUT>
__global__ __launch_bounds__(256) void k_hash_bwd(uint32_t n, const float *__restrict__ pos, uint32_t stride, const T *__restrict__ dLdy, LevelTable lt,
                                                  G *__restrict__ grad, uint32_t nblk, const uint32_t *__restrict__ n_valid) {
	using P = typename Pair<T>::type;
	uint32_t level, chunk; block_to_level_chunk(nblk, level, chunk);
	const uint32_t i = chunk * 256u + threadIdx.x;
	const uint32_t lim = valid_count(n, n_valid);
	if (i >= lim) return;
	const uint32_t off = lt.v[4 * level], size = lt.v[4 * level + 1], res = lt.v[4 * level + 2];
	const float scale = __uint_as_float(lt.v[4 * level + 3]);
	const bool dense = level_is_dense(size, res);
	const P *dy = reinterpret_cast<const P *>(dLdy);
	const float2 g2 = to_f2(load_dy<LAYOUT>(dy, n, level, i));
	if (g2.x == 0.f && g2.y == 0.f) return;   // zero-padded rows add exact zeros in the reference; skipping them is value-identical
	const Corner c = locate(pos, stride, i, scale);
	G *gl = grad + (size_t)off * 2;
#pragma unroll
	for (uint32_t k = 0; k < 8; ++k) {
		float weight = 1; uint32_t g[3];
#pragma unroll
		for (int d = 0; d < 3; ++d) {
			if ((k & (1u << d)) == 0) { weight *= 1 - c.w[d]; g[d] = c.g[d]; }
			else { weight *= c.w[d]; g[d] = c.g[d] + 1; }
		}
		const uint32_t idx = grid_index(size, res, dense, g[0], g[1], g[2]);
		atomic_add_pair(gl + (size_t)idx * 2, make_float2(g2.x * weight, g2.y * weight));
	}
}

static bool level_run(const LevelTable &lt, int l);
// (r11) Chunks of 128 samples in flight per level for k_hash_fwd_x2 (a workgroup takes chunks chunk, chunk + nblk, ... of its level).  Fewer chunks = longer workgroups: the
// level row, the kind and the count are paid once for more samples and a trip holds NGP_HASH_FWD_DEPTH samples' loads - but a launch that no longer fills the machine
// several times over ends on its slowest workgroups.  Paired map: by launch size, from the sweep in profiles/r11_hash_fwd_trips.md; the other maps keep rounds 6-10's.
// A/B and test hook NGP_HASH_FWD_CHUNKS (read per call): forces the number for every map.
#define X2_CHUNKS_MAX 65536u          // step = 128 nblk stays below 2^23 (x2_samples multiplies it by the depth)
#define X2_CHUNKS_SMALL_N (1u << 19)  // launches up to this many samples (the 2^18-sample training batch: alone on the GPU 42.4 us at 512 chunks, 42.8 at 1024, 46.8 at 2048 = one trip
                                      // each; in the step, beside the side stream, 2334 / 2337 it/s at 512, 2345 / 2349 at 1024, 2315 / 2327 at 2048) ...
#ifndef X2_CHUNKS_SMALL
#define X2_CHUNKS_SMALL 1024u         // ... keep this many chunks in flight,
#endif
#define X2_CHUNKS_LARGE 4096u         // larger ones (the 2^20-point refresh query, the 4 M-row inference buffers: 235 us at 4096 chunks, 242 at 1024, 254 at 512) this many
static uint32_t x2_chunks(uint32_t n, bool paired) {
	const uint32_t all = div_up(n, 128);
	const char *e = getenv("NGP_HASH_FWD_CHUNKS");
	const long forced = e ? atol(e) : 0;
	if (forced > 0) return min((uint32_t)min(forced, (long)X2_CHUNKS_MAX), all);
	if (!paired) return min(all, 4096u);
	return min(all, n <= X2_CHUNKS_SMALL_N ? X2_CHUNKS_SMALL : X2_CHUNKS_LARGE);
}
NGP_API int ngp_hash_encode_fwd(void *stream, uint32_t n, const float *pos, uint32_t pos_stride, const void *table, const uint32_t *level_table_host,
                                void *out, int dtype, int out_layout, const uint32_t *n_valid) {
	NGP_REQUIRE(n == 0 || (pos && table && level_table_host && out), NGP_E_ARG, "ngp_hash_encode_fwd: null pointer");
	NGP_REQUIRE(dtype == NGP_F32 || dtype == NGP_F16, NGP_E_DTYPE, "ngp_hash_encode_fwd: bad dtype %d", dtype);
	if (n == 0) return 0;
	NGP_REQUIRE(pos_stride >= 3, NGP_E_ARG, "ngp_hash_encode_fwd: pos stride %u < 3", pos_stride);
	const dim3 block(256);
	const LevelTable lt = load_table(level_table_host);
	hipStream_t s = (hipStream_t)stream;
	// A/B hook NGP_HASH_FWD_X2: bit 0 = two lanes per (sample, level) for the fp32 table (default on), bit 1 = for the fp16 table (default off: its 8-byte pair loads stay)
	static const int x2 = [] { const char *e = getenv("NGP_HASH_FWD_X2"); return e ? atoi(e) : 1; }();
	// A/B hook NGP_HASH_FWD_MAP (r10): 1 (default) = fp32 table, k_hash_fwd_x2's workgroups by block_to_level_chunk_paired (two XCDs share four levels: the training launch
	// 60.6 -> 50.6 us alone on the GPU); 0 = by block_to_level_chunk, the launch of rounds 6-9
	const char *map_env = getenv("NGP_HASH_FWD_MAP");                      // (r11: read per call, like NGP_HASH_FWD_RUNS below - tests/test_hash_fwd_trips.py runs both maps in one process)
	const int paired = map_env ? atoi(map_env) : 1;
	// A/B hook NGP_HASH_FWD_RUNS (r10): 1 = fp32 table, the run levels (level_run: the levels the backward run-combines) through k_hash_fwd_runs and the others through
	// k_hash_fwd_x2 - two launches, every XCD an equal share of each; 0 (default: the run kernel lost its A/B, 75 against 61 us, hash_fwd_runs.h) = one k_hash_fwd_x2 launch
	// (read per call, like NGP_HASH_BWD_RUNS: tests/test_hash_fwd_runs.py runs both routings in one process)
	const char *runs_env = getenv("NGP_HASH_FWD_RUNS");
	const int runs = runs_env ? atoi(runs_env) : 0;
	const FwdSel no_sel{};
	if (dtype == NGP_F32 && (x2 & 1) && runs) {
		FwdSel sel_run{}, sel_fine{};
		for (int l = 0; l < 16; ++l) { FwdSel &t = level_run(lt, l) ? sel_run : sel_fine; t.level[t.m++] = (uint32_t)l; }
		if (sel_run.m) {
			if (sel_fine.m) {
				const uint32_t nblk2 = x2_chunks(n, false);
#define GO2S(L) NGP_LAUNCH((k_hash_fwd_x2<float, L, X2_MAP_SEL>), dim3(8 * div_up(sel_fine.m * nblk2, 8)), block, 0, s, n, pos, pos_stride, (const float *)table, lt, (float *)out, nblk2, n_valid, sel_fine)
				if (out_layout == NGP_LAYOUT_SOA) GO2S(NGP_LAYOUT_SOA); else GO2S(NGP_LAYOUT_AOS);
#undef GO2S
			}
			const uint32_t nblkr = min(div_up(n, FWD_RUN_SPAN), 2048u);
			// 16-byte accesses only where they are aligned: positions as 96-byte blocks (stride 3), a window's SOA feature pairs as 64 (level * n + first even)
			const uint32_t wide = ((pos_stride == 3 && ((uintptr_t)pos & 15u) == 0) ? 1u : 0u) | ((out_layout == NGP_LAYOUT_SOA && (n & 1u) == 0 && ((uintptr_t)out & 15u) == 0) ? 2u : 0u);
#define GOR(L) NGP_LAUNCH((k_hash_fwd_runs<float, L>), dim3(8 * div_up(sel_run.m * nblkr, 8)), dim3(FWD_RUN_WG), 0, s, n, pos, pos_stride, (const float *)table, lt, (float *)out, nblkr, n_valid, sel_run, wide)
			if (out_layout == NGP_LAYOUT_SOA) GOR(NGP_LAYOUT_SOA); else GOR(NGP_LAYOUT_AOS);
#undef GOR
			NGP_LAUNCH_CHECK("ngp_hash_encode_fwd");
			return 0;
		}
	}
	if (dtype == NGP_F32 && (x2 & 1) && paired) {                                     // two lanes per (sample, level), the XCDs in pairs
		const uint32_t nblk2 = x2_chunks(n, true);
#define GO2P(L) NGP_LAUNCH((k_hash_fwd_x2<float, L, X2_MAP_PAIRED>), dim3(32 * div_up(nblk2, 2)), block, 0, s, n, pos, pos_stride, (const float *)table, lt, (float *)out, nblk2, n_valid, no_sel)
		if (out_layout == NGP_LAYOUT_SOA) GO2P(NGP_LAYOUT_SOA); else GO2P(NGP_LAYOUT_AOS);
#undef GO2P
		NGP_LAUNCH_CHECK("ngp_hash_encode_fwd");
		return 0;
	}
	if ((dtype == NGP_F32 && (x2 & 1)) || (dtype == NGP_F16 && (x2 & 2))) {            // two lanes per (sample, level): 128 samples per workgroup
		const uint32_t nblk2 = x2_chunks(n, false);
#define GO2(T, L) NGP_LAUNCH((k_hash_fwd_x2<T, L>), dim3(16 * nblk2), block, 0, s, n, pos, pos_stride, (const T *)table, lt, (T *)out, nblk2, n_valid, no_sel)
		if (dtype == NGP_F32) { if (out_layout == NGP_LAYOUT_SOA) GO2(float, NGP_LAYOUT_SOA); else GO2(float, NGP_LAYOUT_AOS); }
		else { if (out_layout == NGP_LAYOUT_SOA) GO2(__half, NGP_LAYOUT_SOA); else GO2(__half, NGP_LAYOUT_AOS); }
#undef GO2
		NGP_LAUNCH_CHECK("ngp_hash_encode_fwd");
		return 0;
	}
	const uint32_t nblk = min(div_up(n, 256), 2048u);         // chunks per level in flight (k_hash_fwd strides over the rest)
	const dim3 grid(16 * nblk);
#define GO(T, L) NGP_LAUNCH((k_hash_fwd<T, L>), grid, block, 0, s, n, pos, pos_stride, (const T *)table, lt, (T *)out, nblk, n_valid)
	if (dtype == NGP_F32) { if (out_layout == NGP_LAYOUT_SOA) GO(float, NGP_LAYOUT_SOA); else GO(float, NGP_LAYOUT_AOS); }
	else { if (out_layout == NGP_LAYOUT_SOA) GO(__half, NGP_LAYOUT_SOA); else GO(__half, NGP_LAYOUT_AOS); }
#undef GO
	NGP_LAUNCH_CHECK("ngp_hash_encode_fwd");
	return 0;
}

NGP_API int ngp_hash_encode_fwd_dydx(void *stream, uint32_t n, const float *pos, uint32_t pos_stride, const void *table, const uint32_t *level_table_host,
                                     void *out, int dtype, int out_layout, const uint32_t *n_valid, float *dy_dx) {
	NGP_REQUIRE(n == 0 || (pos && table && level_table_host && out && dy_dx), NGP_E_ARG, "ngp_hash_encode_fwd_dydx: null pointer");
	NGP_REQUIRE(dtype == NGP_F32 || dtype == NGP_F16, NGP_E_DTYPE, "ngp_hash_encode_fwd_dydx: bad dtype %d", dtype);
	NGP_REQUIRE(((uintptr_t)dy_dx & 7) == 0, NGP_E_ALIGN, "ngp_hash_encode_fwd_dydx: dy_dx must be 8-byte aligned");
	if (n == 0) return 0;
	NGP_REQUIRE(pos_stride >= 3, NGP_E_ARG, "ngp_hash_encode_fwd_dydx: pos stride %u < 3", pos_stride);
	const uint32_t nblk = min(div_up(n, 256), 2048u);
	const dim3 grid(16 * nblk), block(256);
	const LevelTable lt = load_table(level_table_host);
	hipStream_t s = (hipStream_t)stream;
#define GO(T, L) NGP_LAUNCH((k_hash_fwd_dydx<T, L>), grid, block, 0, s, n, pos, pos_stride, (const T *)table, lt, (T *)out, nblk, n_valid, dy_dx)
	if (dtype == NGP_F32) { if (out_layout == NGP_LAYOUT_SOA) GO(float, NGP_LAYOUT_SOA); else GO(float, NGP_LAYOUT_AOS); }
	else { if (out_layout == NGP_LAYOUT_SOA) GO(__half, NGP_LAYOUT_SOA); else GO(__half, NGP_LAYOUT_AOS); }
#undef GO
	NGP_LAUNCH_CHECK("ngp_hash_encode_fwd_dydx");
	return 0;
}
// method: 0 = by what the caller hands over (a workspace: the binned scatter; none: global atomics), 1 = one global atomic per corner whatever is handed over
// (the reference's scheme; NGP_HASH_BWD_ATOMICS=1)
static int hash_bwd_method() {
	static int m = -1;
	if (m < 0) { const char *e = getenv("NGP_HASH_BWD_ATOMICS"); m = (e && e[0] == '1') ? 1 : 0; }
	return m;
}

// test hook (tests/test_host_cpu.py): entry of a level with `size` entries -> (bin, slot inside the bin, entry rebuilt from them, slots the bin's accumulate workgroup owns) as the region
// kernels and k_bin_accumulate2 compute them
NGP_API void ngp_x_bin2_map(uint32_t size, uint32_t e, uint32_t *out4_host) {
	const bool il = size < BIN_LEVEL_MAX;
	const uint32_t bin = bin2_of(e, il), local = local2_of(e, il), groups_all = (size + 7u) >> 3;
	out4_host[0] = bin; out4_host[1] = local; out4_host[2] = entry2_of(bin, local, il);
	out4_host[3] = il ? (groups_all > bin ? ((groups_all - bin + PAIR_BINS - 1u) / PAIR_BINS) << 3 : 0u) : PAIR_BIN_ENTRIES;
}
// test hook (tests/test_host_cpu.py): the same function on the host, against round-half-even of the exact product
NGP_API long long ngp_x_fixed_rn(float c, float s) { return fixed_rn(c, s); }

// the accumulate with the table's sweep riding, under its own name for NGP_LAUNCH's brackets (bench.py tells the two apart; rocprof shows the template arguments)
static constexpr auto k_bin_accumulate2_adam = k_bin_accumulate2<float, true>;
static constexpr auto k_bin_accumulate_adam_f32rec = k_bin_accumulate<float, float2, true>, k_bin_accumulate_adam_f16rec = k_bin_accumulate<float, __half2, true>;

// Which levels can take the binned path: up to 2^19 entries, and indexed the way the record kernels index (dense, or the XOR hash masked by a power of two).
// (aabb_scale 23.4 has a DENSE level with res 80 = 512000 entries - round 1 binned it with the XOR hash by looking at the size alone.)
static bool level_dense_host(uint32_t size, uint32_t res) { uint32_t stride = 1; for (int d = 0; d < 3; ++d) if (stride <= size) stride *= res; return !(size < stride); }
static bool level_binned(const LevelTable &lt, int l) {
	const uint32_t size = lt.v[4 * l + 1], res = lt.v[4 * l + 2];
	return size <= BIN_LEVEL_MAX && (level_dense_host(size, res) || (size & (size - 1)) == 0);
}
// capacity of one record list of the per-corner path: 4x the expected n*8/64 records per bin; % 8: 16-byte aligned streams
static uint32_t bin_capacity(uint32_t n) { uint32_t c = ((n / 2) / CUR_SUBS + 7u) & ~7u; const uint32_t lo = 4096u / CUR_SUBS; return c < lo ? lo : c; }
// the levels whose cell edges never leave a 4096-entry bin (k_bin_pairs): full 2^19-entry hashed tables (beyond res 2048: as eight single records per sample)
static bool level_pair_capable(const LevelTable &lt, int l) {
	const uint32_t size = lt.v[4 * l + 1], res = lt.v[4 * l + 2];
	return size == BIN_LEVEL_MAX && !level_dense_host(size, res);
}
static bool level_run(const LevelTable &lt, int l) { return lt.v[4 * l + 2] <= RUN_RES_MAX; }
// How a call with a workspace is routed - decided by the level table and the dtypes alone, so that the workspace can be SIZED for the path that will run (r5; rounds 2-4
// reserved the sum of both designs, ~2.3 GB at 2^18 samples):
//   HB_REGIONS    fp32 dL/dy -> fp32 gradient, every level a run level or edge-capable (every table GridEncode builds): record regions, no global atomic (r4)
//   HB_PERCORNER  everything else the bins can take (fp16 dL/dy - ngp_fox.py): per-corner record lists with cursor reservations (r2 / r3)
//   HB_ATOMICS    no workspace, a level beyond 2^19 entries, a hashed table that is not a power of two, NGP_HASH_BWD_ATOMICS=1: the reference's scheme, one global float
//                 atomic per corner (HashEncode.h:299-396) - correct, ~25x slower (7.8 ms per 2^18-sample batch), the ONE fallback of this stage
enum HashBwdPath { HB_ATOMICS = 0, HB_PERCORNER = 1, HB_REGIONS = 2 };
static HashBwdPath hash_bwd_path(const LevelTable &lt, int dtype, int grad_dtype, const void *grad) {
	if (hash_bwd_method() == 1) return HB_ATOMICS;
	bool regions = dtype == NGP_F32 && grad_dtype == NGP_F32 && ((uintptr_t)grad & 15u) == 0;
	for (int l = 0; l < 16; ++l) {
		if (!level_binned(lt, l)) return HB_ATOMICS;
		if (!level_run(lt, l) && !level_pair_capable(lt, l)) regions = false;
	}
	return regions ? HB_REGIONS : HB_PERCORNER;
}
// test hook (tests/test_host_cpu.py): the routing decision for a 16-byte aligned gradient buffer - 0 = global float atomics, 1 = per-corner lists, 2 = record regions
NGP_API int ngp_x_hash_bwd_path(const uint32_t *level_table_host, int dtype, int grad_dtype) {
	static float aligned_dummy[4] __attribute__((aligned(16)));
	return (int)hash_bwd_path(load_table(level_table_host), dtype, grad_dtype, aligned_dummy);
}
// workspace = cursors u32[N_ZEROED] | abs-max partials u32[16 * NGP_ABSMAX_PARTS], spill count | { per-corner: record values | record indices | spill list }
//                                                                                                 { regions: spill list | edge records | their bin offsets | run records | offsets }
struct WsLayout { uint64_t cursors, absmax, rec_val, rec_idx, spill, pair_rec, pair_off, run_rec, run_off, total; uint32_t cap, spill_cap, n_binned, n_pair, n_run, pair_s; };
static WsLayout ws_layout(const LevelTable &lt, uint32_t n, HashBwdPath path) {
	WsLayout w; memset(&w, 0, sizeof(w));
	bool any_split = false;                                              // an edge level beyond res 2048: 512-sample record workgroups (eight single records per sample)
	for (int l = 0; l < 16; ++l) {
		if (!level_binned(lt, l)) continue;
		++w.n_binned;
		if (level_run(lt, l)) ++w.n_run;
		else if (level_pair_capable(lt, l)) { ++w.n_pair; any_split |= lt.v[4 * l + 2] > PAIR_RES_MAX; }
	}
	w.pair_s = any_split ? 512u : 1024u;
	w.cap = bin_capacity(n);
	w.cursors = 0;
	w.absmax = w.cursors + N_ZEROED * 4u;
	const uint64_t body = w.absmax + 16u * ABSMAX_PARTS * 4u + 256;
	if (path == HB_REGIONS) {
		// spill list of the edge kernel: edges of positions OUTSIDE the unit cube (x + 1 can carry into the bin bits) - none in a marched batch; sized for the worst case,
		// every edge of every sample on every edge level (2 entries each), because a dropped entry would be a silently wrong gradient
		w.spill_cap = (uint32_t)(((uint64_t)w.n_pair * 8u * n < (1ull << 27)) ? (uint64_t)w.n_pair * 8u * n : (1ull << 27));
		w.spill = body;
		w.pair_rec = (w.spill + (uint64_t)w.spill_cap * sizeof(SpillEntry) + 255) & ~(uint64_t)255;
		const uint64_t regions_pair = div_up(n, w.pair_s);                  // one region per record workgroup
		w.pair_off = (w.pair_rec + (uint64_t)w.n_pair * regions_pair * pair_region_records() * sizeof(PairRec) + 255) & ~(uint64_t)255;
		w.run_rec = w.pair_off + (((uint64_t)w.n_pair * regions_pair * PAIR_OFFS * sizeof(uint16_t) + 255) & ~(uint64_t)255);
		const uint64_t regions_run = div_up(n, RUN_WG * RUN_K);             // a region per 2048-sample workgroup, worst case eight records per sample (scattered positions)
		w.run_off = (w.run_rec + (uint64_t)w.n_run * regions_run * run2_region_records() * sizeof(RunRec) + 255) & ~(uint64_t)255;
		w.total = w.run_off + (((uint64_t)w.n_run * regions_run * RUN2_OFFS * sizeof(uint16_t) + 255) & ~(uint64_t)255);
	} else if (path == HB_PERCORNER) {
		const uint32_t per = (1u << 25) / (w.n_binned ? w.n_binned : 1u);
		w.spill_cap = w.n_binned * 8u * (n < per ? n : per);              // worst case: every record of every binned level overflows (12 B each)
		w.rec_val = body;
		w.rec_idx = w.rec_val + (uint64_t)w.n_binned * BINS_PER_LEVEL * CUR_SUBS * w.cap * sizeof(float2);       // every level owns 64 * cap * 8 bytes (rec_val_at)
		w.spill = (w.rec_idx + (uint64_t)w.n_binned * BINS_PER_LEVEL * CUR_SUBS * w.cap * sizeof(uint16_t) + 255) & ~(uint64_t)255;
		w.total = (w.spill + (uint64_t)w.spill_cap * sizeof(SpillEntry) + 255) & ~(uint64_t)255;
	} else w.total = 0;
	return w;
}
// bytes ngp_hash_encode_bwd_ws needs for n samples: for the path the given dtypes take (ngp_base.py / fp32: ~0.6 GB at 2^18 samples, ngp_fox.py / fp16: ~1.7 GB) ...
NGP_API uint64_t ngp_hash_bwd_workspace_bytes_for(const uint32_t *level_table_host, uint32_t n, int dtype, int grad_dtype) {
	const LevelTable lt = load_table(level_table_host);
	static float aligned_dummy[4] __attribute__((aligned(16)));
	return ws_layout(lt, n, hash_bwd_path(lt, dtype, grad_dtype, aligned_dummy)).total;
}
// ... and for a caller that does not say: enough for either
NGP_API uint64_t ngp_hash_bwd_workspace_bytes(const uint32_t *level_table_host, uint32_t n) {
	const uint64_t a = ngp_hash_bwd_workspace_bytes_for(level_table_host, n, NGP_F32, NGP_F32), b = ngp_hash_bwd_workspace_bytes_for(level_table_host, n, NGP_F16, NGP_F32);
	return a > b ? a : b;
}

// ---------------------------------------------------------------------------------------------------------------- the three launch schemes
// One call of hash_bwd_impl past validation and routing: its arguments (see there), the level plan, the carved workspace, and what the launch functions report back.
struct HashBwdCall {
	hipStream_t s; uint32_t n; const float *pos; uint32_t pos_stride; const void *dLdy; LevelTable lt; void *grad; int ow; const uint32_t *n_valid;
	hipEvent_t after_coarse; bool absmax_done; const TailJobs *tail;
	const AdamRide *ride;                                                // the table's sweep when it rides in the accumulate launches; null: they store the gradient
	BinPlan bp; LevelSel sel_fine, sel_runs, sel_all, sel_pair;          // sel_all: every level with per-corner records (runs + fine); sel_pair: the edge-record levels
	uint32_t n_fine, n_runs, n_all, n_pair;
	WsLayout wl; char *ws; uint32_t *cursors, *absmax, *spill_count; SpillEntry *spill;
	bool tail_taken, coarse_marked;                                      // out: the tail jobs rode; after_coarse was recorded between two accumulate launches
};
static const AdamRide no_ride{nullptr, nullptr, nullptr, nullptr, AdamConsts{}, 0};
// dynamic-LDS limit of a kernel: every scheme lists its kernels in front of its launch function, hash_bwd_set_lds raises the limits once per device
struct LdsLimit { const void *kernel; uint32_t bytes; };

// ---- HB_ATOMICS: the reference's scheme, one global float atomic per corner (no dynamic LDS)
template <typename T, typename G, int LAYOUT>
static void launch_atomics(HashBwdCall &c) {
	const uint32_t nblk = div_up(c.n, 256);
	NGP_LAUNCH((k_hash_bwd<T, G, LAYOUT>), dim3(16 * nblk), dim3(256), 0, c.s, c.n, c.pos, c.pos_stride, (const T *)c.dLdy, c.lt, (G *)c.grad, nblk, c.n_valid);
}

// the abs-max pass in front of both workspace schemes; also zeroes the cursors and the spill count
template <typename T, int LAYOUT>
static void launch_absmax(const HashBwdCall &c) {
	if (!c.absmax_done) NGP_LAUNCH((k_level_absmax<T, LAYOUT>), dim3(ABSMAX_OWN_PARTS, 16), dim3(256), 0, c.s, c.n, (const T *)c.dLdy, c.absmax, c.n_valid, c.cursors, c.spill_count);
}

// ---- HB_REGIONS (hash_bwd_regions.h): fp32 -> fp32, run records + edge records in regions, no global atomics, ONE accumulate kernel - two launches of it when the
// data-parallel exchange wants the coarse levels first
static const LdsLimit lds_regions[] = {
	{(const void *)k_bin_runs2<float, NGP_LAYOUT_SOA, 5>, run2_stage_bytes(RUN2_STAGE)}, {(const void *)k_bin_runs2<float, NGP_LAYOUT_AOS, 5>, run2_stage_bytes(RUN2_STAGE)},
	{(const void *)k_bin_runs2<float, NGP_LAYOUT_SOA, 5, true>, run2_stage_bytes(RUN2_STAGE)}, {(const void *)k_bin_runs2<float, NGP_LAYOUT_AOS, 5, true>, run2_stage_bytes(RUN2_STAGE)},
	{(const void *)k_bin_pairs<float, NGP_LAYOUT_SOA, 512u>, pair_stage_bytes()}, {(const void *)k_bin_pairs<float, NGP_LAYOUT_AOS, 512u>, pair_stage_bytes()},
	{(const void *)k_bin_pairs<float, NGP_LAYOUT_SOA, 1024u>, pair_stage_bytes()}, {(const void *)k_bin_pairs<float, NGP_LAYOUT_AOS, 1024u>, pair_stage_bytes()},
	{(const void *)k_bin_accumulate2<float, false>, PAIR_BIN_ENTRIES * 16u + ACC2_LDS_EXTRA}, {(const void *)k_bin_accumulate2<float, true>, PAIR_BIN_ENTRIES * 16u + ACC2_LDS_EXTRA},
};
template <int LAYOUT>
static void launch_regions(HashBwdCall &c) {
	const uint32_t n = c.n, pair_s = c.wl.pair_s;
	const float *dLdy = (const float *)c.dLdy;
	PairRec *pair_rec = (PairRec *)(c.ws + c.wl.pair_rec); uint16_t *pair_off = (uint16_t *)(c.ws + c.wl.pair_off);
	RunRec *run_rec = (RunRec *)(c.ws + c.wl.run_rec); uint16_t *run_off = (uint16_t *)(c.ws + c.wl.run_off);
	// (r6) the MLP tail rides along when both record kernels run: every workgroup of k_bin_runs2 reduces its share of the slabs and sweeps those parameters, every workgroup
	// of k_bin_pairs - the next launch in the stream, so it reads the swept pack - gathers its share of the fragment buffer (mlp_tail.h)
	TailJobs tj_run = no_tail_jobs(), tj_pair = no_tail_jobs();
	const TailJobs *tail = c.tail;
	if (tail && tail->do_reduce && tail->do_sweep && tail->pack_table && c.n_runs && c.n_pair && n > 0 && (uint64_t)tail->n_slabs * tail->width < (1ull << 32)) {   // (the rider indexes the slabs with 32 bits)
		tj_run = *tail; tj_pair = *tail; tj_pair.do_reduce = 0;
		c.tail_taken = true;
	}
	// A/B hook NGP_HASH_BWD_RUNS: 1 (default) = k_bin_runs2's V2 form (r7: half the workgroups carry their tail unit last, nothing spills), 0 = round 4-6's; same records, same brackets
	const char *runs_env = getenv("NGP_HASH_BWD_RUNS");                   // (read per call: tests/test_hash_bwd_stage.py compares the two forms in one process)
	const int runs_v2 = runs_env ? atoi(runs_env) : 1;
#define RUNS2(V2) NGP_LAUNCH((k_bin_runs2<float, LAYOUT, 5, V2>), dim3(div_up(n, RUN_WG * RUN_K), c.n_runs), dim3(RUN_WG), run2_stage_bytes(RUN2_STAGE), c.s, n, c.pos, c.pos_stride, dLdy, c.lt, c.bp, c.sel_runs, (const uint32_t *)c.absmax, run_rec, run_off, c.n_valid, RUN2_STAGE, tj_run)
// (k_bin_pairs depends on the abs-max pass like k_bin_runs2 does, not on k_bin_runs2: both are plain in-order launches - the any-order launch of round 4 lost its A/B and raced with the abs-max pass when there was no run level)
#define PAIRS(S) NGP_LAUNCH((k_bin_pairs<float, LAYOUT, S>), dim3(div_up(n, S), c.n_pair), dim3(S), pair_stage_bytes(), c.s, n, c.pos, c.pos_stride, dLdy, c.lt, c.bp, c.sel_pair, (const uint32_t *)c.absmax, pair_rec, pair_off, c.spill_count, c.spill, c.n_valid, tj_pair)
	launch_absmax<float, LAYOUT>(c);
	if (c.n_runs) { if (runs_v2) RUNS2(true); else RUNS2(false); }
	if (c.n_pair) { if (pair_s == 512u) PAIRS(512u); else PAIRS(1024u); }
#undef PAIRS
#undef RUNS2
	// (r6) the timing probes of tools/probe_scatter.py - parts of a kernel skipped, results WRONG - are compile-time builds now (-DNGP_PROBE_SCATTER: no record stores;
	// -DNGP_PROBE_ACC=1|2: accumulate's records loaded but not processed | not loaded), no longer environment variables a user could set on the product binary
#ifndef NGP_PROBE_ACC
#define NGP_PROBE_ACC 0u
#endif
#define ACCUMULATE2(K, DST, OW, RIDE) NGP_LAUNCH(K, dim3(n_units), dim3(ACC2_WG), PAIR_BIN_ENTRIES * 16u + ACC2_LDS_EXTRA, c.s, c.lt, c.bp, c.sel_pair, c.sel_runs, ap, (const uint32_t *)c.absmax, (const PairRec *)pair_rec, \
	(const uint16_t *)pair_off, (const RunRec *)run_rec, (const uint16_t *)run_off, (const uint32_t *)c.spill_count, (const SpillEntry *)c.spill, DST, OW, RIDE)
	auto accumulate = [&](bool runs, bool pairs) {
		Acc2Plan ap;
		ap.n_pair = pairs ? c.n_pair : 0u; ap.n_run = runs ? c.n_runs : 0u;
		ap.pair_regions = div_up(n, pair_s); ap.pair_region_records = pair_region_records();
		ap.run_regions = div_up(n, RUN_WG * RUN_K); ap.run_region_records = run2_region_records();
		ap.probe = NGP_PROBE_ACC;
		const uint32_t n_units = (ap.n_pair + ap.n_run) * PAIR_BINS;
		if (!n_units) return;
		if (c.ride) ACCUMULATE2(k_bin_accumulate2_adam, (float *)nullptr, 1, *c.ride);
		else ACCUMULATE2((k_bin_accumulate2<float, false>), (float *)c.grad, c.ow, no_ride);
	};
#undef ACCUMULATE2
	if (c.after_coarse && c.n_runs && c.n_pair) { accumulate(true, false); (void)hipEventRecord(c.after_coarse, c.s); c.coarse_marked = true; accumulate(false, true); }
	else accumulate(true, true);
}

// ---- HB_PERCORNER (hash_bwd_percorner.h): per-corner record lists (fp16 dL/dy) - 6-byte fp16 records for the fine levels, fp32 run records for the coarse ones
#define RECORD_KERNELS(T) {(const void *)k_bin_records_runs<T, NGP_LAYOUT_SOA, 4>, run_stage_bytes(RUN_STAGE)}, {(const void *)k_bin_records_runs<T, NGP_LAYOUT_AOS, 4>, run_stage_bytes(RUN_STAGE)}, \
	{(const void *)k_bin_records<T, NGP_LAYOUT_SOA>, bin_stage_bytes<T>()}, {(const void *)k_bin_records<T, NGP_LAYOUT_AOS>, bin_stage_bytes<T>()}
static const LdsLimit lds_percorner[] = {
	RECORD_KERNELS(float), RECORD_KERNELS(__half),
	{(const void *)k_bin_accumulate<float, float2, false>, BIN_ENTRIES * 16}, {(const void *)k_bin_accumulate<float, __half2, false>, BIN_ENTRIES * 16},
	{(const void *)k_bin_accumulate<__half, float2, false>, BIN_ENTRIES * 16}, {(const void *)k_bin_accumulate<__half, __half2, false>, BIN_ENTRIES * 16},
	{(const void *)k_bin_accumulate<float, float2, true>, BIN_ENTRIES * 16}, {(const void *)k_bin_accumulate<float, __half2, true>, BIN_ENTRIES * 16},
};
#undef RECORD_KERNELS
template <typename T, typename G, int LAYOUT>
static void launch_percorner(HashBwdCall &c) {
	using RV = typename RecVal<T>::type;                                 // records of the fine levels; run records are float2 whatever T
	const uint32_t n = c.n;
	void *rec_val = (void *)(c.ws + c.wl.rec_val); uint16_t *rec_idx = (uint16_t *)(c.ws + c.wl.rec_idx);
	// (r6) fp16 configuration: the slab reduction that also sweeps the two MLP packs (k_reduce_slabs_sweep's job) rides as row 0 of the run-record launch
	TailJobs tj_pc = no_tail_jobs();
	const TailJobs *tail = c.tail;
	if (tail && tail->do_reduce && tail->do_sweep16 && !tail->do_sweep && c.n_runs && n > 0 && (uint64_t)tail->n_slabs * tail->width < (1ull << 32)) { tj_pc = *tail; c.tail_taken = true; }
	launch_absmax<T, LAYOUT>(c);
	if (c.n_runs) NGP_LAUNCH((k_bin_records_runs<T, LAYOUT, 4>), dim3(div_up(n, RUN_WG * RUN_K), c.n_runs), dim3(RUN_WG), run_stage_bytes(RUN_STAGE), c.s, n, c.pos, c.pos_stride, (const T *)c.dLdy, c.lt, c.bp, c.sel_runs, (const uint32_t *)c.absmax, c.cursors, rec_val, rec_idx, c.spill_count, c.spill, c.n_valid, RUN_STAGE, tj_pc);
	if (c.n_fine) NGP_LAUNCH((k_bin_records<T, LAYOUT>), dim3(div_up(n, BIN_WG), c.n_fine), dim3(BIN_WG), bin_stage_bytes<T>(), c.s, n, c.pos, c.pos_stride, (const T *)c.dLdy, c.lt, c.bp, c.sel_fine, (const uint32_t *)c.absmax, c.cursors, rec_val, rec_idx, c.spill_count, c.spill, c.n_valid);
	// one accumulate launch: kernel K over the N_LEVELS levels of SEL (none: no launch), into DST or - RIDE - with the table's update in place of the gradient store
#define ACCUMULATE(K, SEL, N_LEVELS, DST, OW, RIDE) do { if (N_LEVELS) NGP_LAUNCH(K, dim3((N_LEVELS) * BINS_PER_LEVEL), dim3(1024), BIN_ENTRIES * 16, c.s, c.lt, c.bp, SEL, (const uint32_t *)c.absmax, (const uint32_t *)c.cursors, \
	rec_val, rec_idx, (const uint32_t *)c.spill_count, (const SpillEntry *)c.spill, DST, OW, RIDE); } while (0)
	if (c.ride) {                                                        // (r6) the table's sweep rides (fp32 gradient only): same launches, the update in place of the gradient store
		if (sizeof(RV) == 8) ACCUMULATE(k_bin_accumulate_adam_f32rec, c.sel_all, c.n_all, (float *)nullptr, 1, *c.ride);
		else {
			ACCUMULATE(k_bin_accumulate_adam_f32rec, c.sel_runs, c.n_runs, (float *)nullptr, 1, *c.ride);
			ACCUMULATE(k_bin_accumulate_adam_f16rec, c.sel_fine, c.n_fine, (float *)nullptr, 1, *c.ride);
		}
	} else if (sizeof(RV) == 8 && !(c.after_coarse && c.n_runs && c.n_fine)) {   // fp32 records, one type: one accumulate launch over all their levels
		ACCUMULATE((k_bin_accumulate<G, float2, false>), c.sel_all, c.n_all, (G *)c.grad, c.ow, no_ride);
	} else {
		ACCUMULATE((k_bin_accumulate<G, float2, false>), c.sel_runs, c.n_runs, (G *)c.grad, c.ow, no_ride);
		if (c.n_runs && c.after_coarse && c.n_fine) { (void)hipEventRecord(c.after_coarse, c.s); c.coarse_marked = true; }
		ACCUMULATE((k_bin_accumulate<G, RV, false>), c.sel_fine, c.n_fine, (G *)c.grad, c.ow, no_ride);
	}
#undef ACCUMULATE
}

template <size_t N> static int set_lds_limits(const LdsLimit (&list)[N]) {
	for (const LdsLimit &l : list) {
		hipError_t e = hipFuncSetAttribute(l.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.bytes);
		if (e != hipSuccess) { ngp_set_error("ngp_hash_encode_bwd: hipFuncSetAttribute: %s", hipGetErrorString(e)); return (int)e; }
	}
	return 0;
}
// the dynamic-LDS limits of the scatter kernels, raised once per DEVICE and only marked done when every call succeeded
static int hash_bwd_set_lds() {
	static std::mutex mu;
	static bool done[64] = {false};
	int dev = 0;
	if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
	std::lock_guard<std::mutex> lk(mu);
	if (done[dev]) return 0;
	int rc = set_lds_limits(lds_percorner);
	if (!rc) rc = set_lds_limits(lds_regions);
	if (!rc) done[dev] = true;
	return rc;
}

// the dtype x layout switch of a scheme whose launch function is a template on <T = dL/dy, G = gradient, LAYOUT>
#define BY_DTYPE_AND_LAYOUT(F, c) do { \
	if (dtype == NGP_F32) { if (in_layout == NGP_LAYOUT_SOA) F<float, float, NGP_LAYOUT_SOA>(c); else F<float, float, NGP_LAYOUT_AOS>(c); } \
	else if (grad_dtype == NGP_F32) { if (in_layout == NGP_LAYOUT_SOA) F<__half, float, NGP_LAYOUT_SOA>(c); else F<__half, float, NGP_LAYOUT_AOS>(c); } \
	else { if (in_layout == NGP_LAYOUT_SOA) F<__half, __half, NGP_LAYOUT_SOA>(c); else F<__half, __half, NGP_LAYOUT_AOS>(c); } } while (0)

// validation and routing; the launches are the scheme's launch function
static int hash_bwd_impl(void *stream, uint32_t n, const float *pos, uint32_t pos_stride, const void *dLdy, const uint32_t *level_table_host,
                         void *grad, uint64_t n_params, int dtype, int grad_dtype, int in_layout, int zero_first, const uint32_t *n_valid, void *workspace, uint64_t workspace_bytes,
                         hipEvent_t after_coarse = nullptr /* data parallel, overlapped exchange: recorded behind the accumulate launch of the run-combined (coarse) levels, which then is a launch of its own */,
                         bool absmax_done = false /* the abs-max partials, zeroed cursors and spill count are already in the workspace (written by the field backward kernel, ngp_hash_bwd_absmax_slots) */,
                         const TailJobs *tail = nullptr /* (r6) jobs that may ride in the record launches (mlp_tail.h) */, int *tail_taken = nullptr /* set to 1 when they did */,
                         const AdamRide *adam = nullptr /* (r6) the table's Adam + EMA sweep, applied by the accumulate kernel INSTEAD of storing the gradient */, int *adam_taken = nullptr /* set to 1 when it was */) {
	if (tail_taken) *tail_taken = 0; if (adam_taken) *adam_taken = 0;
	NGP_REQUIRE(grad && level_table_host && (n == 0 || (pos && dLdy)), NGP_E_ARG, "ngp_hash_encode_bwd: null pointer");
	NGP_REQUIRE(dtype == NGP_F32 || dtype == NGP_F16, NGP_E_DTYPE, "ngp_hash_encode_bwd: bad dtype %d", dtype);
	NGP_REQUIRE(grad_dtype == NGP_F32 || (grad_dtype == NGP_F16 && dtype == NGP_F16), NGP_E_DTYPE, "ngp_hash_encode_bwd: bad grad dtype %d for dtype %d", grad_dtype, dtype);
	HashBwdCall c;
	c.s = (hipStream_t)stream; c.n = n; c.pos = pos; c.pos_stride = pos_stride; c.dLdy = dLdy; c.lt = load_table(level_table_host); c.grad = grad;
	c.ow = zero_first ? 1 : 0; c.n_valid = n_valid; c.after_coarse = after_coarse; c.absmax_done = absmax_done;
	c.tail = tail; c.tail_taken = false; c.coarse_marked = false;
	const LevelTable &lt = c.lt; hipStream_t s = c.s;
	const size_t gsz = grad_dtype == NGP_F16 ? 2 : 4;
	const HashBwdPath path = workspace ? hash_bwd_path(lt, dtype, grad_dtype, grad) : HB_ATOMICS;
	const WsLayout &wl = c.wl = ws_layout(lt, n, path);
	// (r6) the routing looks at the gradient pointer's alignment, the sizing function cannot: an fp32 call with an unaligned gradient used to land on the per-corner path,
	// which needs three times the bytes ngp_hash_bwd_workspace_bytes_for returned - and the capacity error below then named the wrong size.  The workspace path takes aligned
	// gradients only (every buffer torch or hipMalloc hands out is; a view into a flat parameter buffer at an odd offset is the caller's to avoid).
	NGP_REQUIRE(!workspace || ((uintptr_t)grad & 15u) == 0, NGP_E_ALIGN, "ngp_hash_encode_bwd: with a workspace the gradient buffer must be 16-byte aligned");
	// (r6) the spill lists are sized for the worst case up to a cap; beyond it entries would be DROPPED - a silently wrong gradient.  Refuse such a batch up front.
	if (path == HB_REGIONS) NGP_REQUIRE((uint64_t)wl.n_pair * 8u * n <= (1ull << 27), NGP_E_CAPACITY, "ngp_hash_encode_bwd: %u samples exceed the workspace path's spill capacity (%llu per call for this level table): split the batch", n, (unsigned long long)((1ull << 27) / (8u * (wl.n_pair ? wl.n_pair : 1u))));
	if (path == HB_PERCORNER) NGP_REQUIRE(n <= (1u << 25) / (wl.n_binned ? wl.n_binned : 1u), NGP_E_CAPACITY, "ngp_hash_encode_bwd: %u samples exceed the workspace path's spill capacity (%u per call for this level table): split the batch", n, (1u << 25) / (wl.n_binned ? wl.n_binned : 1u));
	// (r5) a workspace that is too small for the path its dtypes take is an ERROR - rounds 2-4 dropped silently to a slower path
	NGP_REQUIRE(path == HB_ATOMICS || workspace_bytes >= wl.total, NGP_E_CAPACITY, "ngp_hash_encode_bwd: workspace of %llu bytes, ngp_hash_bwd_workspace_bytes_for(n = %u) = %llu",
	            (unsigned long long)workspace_bytes, n, (unsigned long long)wl.total);
	if (path == HB_ATOMICS) {
		if (zero_first) {
			hipError_t e = hipMemsetAsync(grad, 0, n_params * gsz, s);
			if (e != hipSuccess) { ngp_set_error("ngp_hash_encode_bwd memset: %s", hipGetErrorString(e)); return (int)e; }
		}
		if (n == 0) { if (after_coarse) (void)hipEventRecord(after_coarse, s); return 0; }
		BY_DTYPE_AND_LAYOUT(launch_atomics, c);
		NGP_LAUNCH_CHECK("ngp_hash_encode_bwd");
		if (after_coarse) (void)hipEventRecord(after_coarse, s);
		return 0;
	}
	int rc = hash_bwd_set_lds(); if (rc) return rc;
	// ---- the binned scatter: every level through records - run levels (res <= 300) with run combining, the others as edge records (regions) or per-corner records
	const bool regions = path == HB_REGIONS;
	c.bp.n_levels = 0; c.bp.cap = wl.cap; c.bp.spill_cap = wl.spill_cap;
	c.n_fine = c.n_runs = c.n_pair = c.n_all = 0;
	for (int l = 0; l < 16; ++l) {                                       // (coarsest level first measured 1 % faster than finest first on both samplings)
		const uint32_t hl = c.bp.n_levels++;
		c.bp.level[hl] = (uint32_t)l;
		if (level_run(lt, l)) { c.sel_runs.hl[c.n_runs++] = hl; if (!regions) c.sel_all.hl[c.n_all++] = hl; }
		else if (regions) c.sel_pair.hl[c.n_pair++] = hl;
		else { c.sel_fine.hl[c.n_fine++] = hl; c.sel_all.hl[c.n_all++] = hl; }
	}
	c.ws = (char *)workspace; c.cursors = (uint32_t *)(c.ws + wl.cursors); c.spill = (SpillEntry *)(c.ws + wl.spill);
	c.absmax = (uint32_t *)(c.ws + wl.absmax); c.spill_count = c.absmax + 16u * ABSMAX_PARTS;
	// (r6) the table's sweep rides in the accumulate launches when together they OVERWRITE the whole table: every level is a unit level on the workspace paths, so that is
	// "the levels tile [0, n_params) without gaps" (every table GridEncode builds), an fp32 gradient (the sweep's input) and no data-parallel exchange between the two
	// (after_coarse); anything else leaves the sweep to the caller.  The fp32 region kernel has no shadow to write.
	bool ride = adam && adam->p && adam->m && adam->v && c.ow && !after_coarse && grad_dtype == NGP_F32 && (((uintptr_t)adam->p | (uintptr_t)adam->m | (uintptr_t)adam->v) & 15u) == 0 &&
	            (((uintptr_t)adam->p_half) & 7u) == 0 && !(regions && adam->p_half);
	if (ride) {
		uint64_t covered = 0;
		for (int l = 0; l < 16; ++l) { if ((uint64_t)lt.v[4 * l] * 2u != covered || (lt.v[4 * l] & 1u)) ride = false; covered += (uint64_t)lt.v[4 * l + 1] * 2u; }
		if (covered != n_params) ride = false;
	}
	c.ride = ride ? adam : nullptr;
	if (!regions) BY_DTYPE_AND_LAYOUT(launch_percorner, c);
	else if (in_layout == NGP_LAYOUT_SOA) launch_regions<NGP_LAYOUT_SOA>(c);
	else launch_regions<NGP_LAYOUT_AOS>(c);
	if (c.tail_taken && tail_taken) *tail_taken = 1;
	if (ride && adam_taken) *adam_taken = 1;
	NGP_LAUNCH_CHECK("ngp_hash_encode_bwd");
	if (after_coarse && !c.coarse_marked) (void)hipEventRecord(after_coarse, s);      // no separate coarse launch on this path: the marker follows the whole scatter
	return 0;
}
#undef BY_DTYPE_AND_LAYOUT

// the workspace path with the data-parallel marker and the fused abs-max (csrc/train_step.hip); not part of the public ABI
int ngp_hash_encode_bwd_ws_marked(void *stream, uint32_t n, const float *pos, uint32_t pos_stride, const void *dLdy, const uint32_t *level_table_host, void *grad, uint64_t n_params, int dtype,
                                  int grad_dtype, int in_layout, int zero_first, const uint32_t *n_valid, void *workspace, uint64_t workspace_bytes, hipEvent_t after_coarse, int absmax_done,
                                  const TailJobs *tail, int *tail_taken, const AdamRide *adam, int *adam_taken) {
	return hash_bwd_impl(stream, n, pos, pos_stride, dLdy, level_table_host, grad, n_params, dtype, grad_dtype, in_layout, zero_first, n_valid, workspace, workspace_bytes, after_coarse, absmax_done != 0,
	                     tail, tail_taken, adam, adam_taken);
}
// mirrors the routing of hash_bwd_impl: the slots are handed out only when that call will read them (grad: the gradient buffer the call will be given)
AbsmaxOut ngp_hash_bwd_absmax_slots(const uint32_t *level_table_host, uint32_t n, int dtype, int grad_dtype, void *workspace, uint64_t workspace_bytes, const void *grad) {
	AbsmaxOut am{nullptr, nullptr, 0u, nullptr};
	if (!workspace || !level_table_host || n == 0 || getenv("NGP_NO_FUSED_ABSMAX")) return am;
	const LevelTable lt = load_table(level_table_host);
	const HashBwdPath path = hash_bwd_path(lt, dtype, grad_dtype, grad);
	if (path == HB_ATOMICS) return am;
	const WsLayout wl = ws_layout(lt, n, path);
	if (workspace_bytes < wl.total) return am;                                                   // (the scatter call will report it)
	char *ws = (char *)workspace;
	am.parts = (uint32_t *)(ws + wl.absmax); am.cursors = (uint32_t *)(ws + wl.cursors); am.n_cursors = N_ZEROED; am.spill_count = am.parts + 16u * ABSMAX_PARTS;
	return am;
}

NGP_API int ngp_hash_encode_bwd(void *stream, uint32_t n, const float *pos, uint32_t pos_stride, const void *dLdy, const uint32_t *level_table_host,
                                void *grad, uint64_t n_params, int dtype, int grad_dtype, int in_layout, int zero_first, const uint32_t *n_valid) {
	return hash_bwd_impl(stream, n, pos, pos_stride, dLdy, level_table_host, grad, n_params, dtype, grad_dtype, in_layout, zero_first, n_valid, nullptr, 0);
}
NGP_API int ngp_hash_encode_bwd_ws(void *stream, uint32_t n, const float *pos, uint32_t pos_stride, const void *dLdy, const uint32_t *level_table_host,
                                   void *grad, uint64_t n_params, int dtype, int grad_dtype, int in_layout, int zero_first, const uint32_t *n_valid,
                                   void *workspace, uint64_t workspace_bytes) {
	return hash_bwd_impl(stream, n, pos, pos_stride, dLdy, level_table_host, grad, n_params, dtype, grad_dtype, in_layout, zero_first, n_valid, workspace, workspace_bytes);
}
