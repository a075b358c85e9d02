// Iso-surface extraction on the device: marching tetrahedra on a float32 lattice u[X][Y][Z] (z fastest, flat id (x*Y + y)*Z + z), with the decomposition and the
// conventions of jnerf_amd/utils/isosurface.py::marching_tetrahedra, which is the oracle (tests/test_iso_gpu.py):
//   - a point is ABOVE iff u > threshold; cube corner c has bit 0 = +x, bit 1 = +y, bit 2 = +z; six tetrahedra [0, 7, R[i], R[(i+1)%6]], R = 1 3 2 6 4 5;
//   - every edge of that decomposition runs from a point `lo` to lo + d, d one of seven offsets (dx,dy,dz) != 0 in {0,1}^3; edge TYPE = 4 dx + 2 dy + dz - 1, which
//     ascends with the flat id of lo + d.  Point lo OWNS its seven edges; its 7-bit mask marks the owned edges whose ends lie in the lattice on different sides;
//   - one vertex per marked edge, ordered by (lo, type) = ascending (lo, hi) flat ids - numpy.unique's order of the host's keys: index = base[lo] + popcount(mask[lo] & below type);
//   - triangles cube-major (flat id of corner 0), then tetrahedron, then the host's order inside one; normals point from above to below.
// Three steps, every output slot from a scan (deterministic order, no atomics, no waiting between workgroups):
//   ngp_iso_count: k_iso_classify (masks, per-cube triangle counts, per-tile totals) -> k_iso_scan_tiles (ONE workgroup: exclusive 64-bit tile bases, the two totals)
//   ngp_iso_emit:  k_iso_emit_vertices (per-point vertex base, positions) -> k_iso_emit_triangles.
// The eight corner reads of a cube go through L1 / L2 (no LDS halo tile): z-neighbours share the wavefront's cache lines, y / x-neighbours are re-read by the workgroups
// one row / one plane on, which L2 serves.
#include "ngp_common.h"

#define ISO_TILE 1024u          // lattice points per tile = per workgroup
#define ISO_BLOCK 256u
#define ISO_MAX_POINTS 2147483647ull

struct IsoShape { uint32_t X, Y, Z, n; };
// workspace: mask u8[np] | tcnt u8[np] | vbase u32[np] | tile totals u32[2][nt] | tile bases u64[2][nt]      (np = n rounded up to whole tiles)
struct IsoWs { uint64_t mask, tcnt, vbase, tot, base, bytes; uint32_t tiles; };

static IsoWs iso_layout(uint64_t n) {
	IsoWs w;
	w.tiles = (uint32_t)((n + ISO_TILE - 1) / ISO_TILE);
	const uint64_t np = (uint64_t)w.tiles * ISO_TILE;
	w.mask = 0; w.tcnt = np; w.vbase = 2 * np; w.tot = w.vbase + 4 * np;
	w.base = (w.tot + 8ull * w.tiles + 15) & ~15ull;
	w.bytes = w.base + 16ull * w.tiles;
	return w;
}

__device__ __forceinline__ uint32_t iso_edge_type(uint32_t cdiff) { return (((cdiff & 1u) << 2) | (cdiff & 2u) | ((cdiff >> 2) & 1u)) - 1u; }   // corner bits (x = bit 0) -> 4 dx + 2 dy + dz - 1
__device__ __forceinline__ uint32_t iso_tet_corners(int k) {           // nibbles: local corners 0..3 of tetrahedron k
	const uint32_t ring = 0x546231u;                                   // R = 1 3 2 6 4 5
	return 0x70u | (((ring >> (4 * k)) & 15u) << 8) | (((ring >> (4 * ((k + 1) % 6))) & 15u) << 12);
}

// exclusive scan over the workgroup (<= 1024 threads); sh: [17]
__device__ __forceinline__ uint32_t iso_block_scan(uint32_t v, uint32_t *sh, uint32_t &total) {
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
	uint32_t x = v;
#pragma unroll
	for (int off = 1; off < 64; off <<= 1) { const uint32_t y = __shfl_up(x, off); if (lane >= (uint32_t)off) x += y; }
	if (lane == 63) sh[wave] = x;
	__syncthreads();
	if (threadIdx.x == 0) { uint32_t acc = 0; for (uint32_t w = 0; w < n_waves; ++w) { const uint32_t t = sh[w]; sh[w] = acc; acc += t; } sh[16] = acc; }
	__syncthreads();
	const uint32_t res = sh[wave] + x - v;
	total = sh[16];
	__syncthreads();
	return res;
}

__global__ __launch_bounds__(ISO_BLOCK) void k_iso_classify(IsoShape s, double threshold, const float *__restrict__ u, uint8_t *__restrict__ mask, uint8_t *__restrict__ tcnt,
                                                            uint32_t *__restrict__ tot_v, uint32_t *__restrict__ tot_t) {
	__shared__ uint32_t sh[2][ISO_BLOCK / 64];
	const uint32_t YZ = s.Y * s.Z;
	uint32_t nv = 0, nt = 0;
#pragma unroll
	for (uint32_t r = 0; r < ISO_TILE / ISO_BLOCK; ++r) {
		const uint32_t id = blockIdx.x * ISO_TILE + r * ISO_BLOCK + threadIdx.x;          // consecutive lanes, consecutive z
		if (id >= s.n) break;                                                              // only in the last tile, from some wavefront on: whole wavefronts leave except one
		const uint32_t x = id / YZ, rem = id - x * YZ, y = rem / s.Z, z = rem - y * s.Z;
		const bool ix = x + 1 < s.X, iy = y + 1 < s.Y, iz = z + 1 < s.Z;
		const float u0 = u[id];
		uint32_t ab = (double)u0 > threshold ? 1u : 0u;
#pragma unroll
		for (uint32_t c = 1; c < 8; ++c) {
			const bool in = ((c & 1u) ? ix : true) && ((c & 2u) ? iy : true) && ((c & 4u) ? iz : true);
			const float v = in ? u[id + (c & 1u) * YZ + ((c >> 1) & 1u) * s.Z + (c >> 2)] : u0;      // a corner outside the lattice: no edge, no sign change
			ab |= ((double)v > threshold ? 1u : 0u) << c;
		}
		const uint32_t diff = (ab ^ (0u - (ab & 1u))) & 0xfeu;                                // corners on the other side than corner 0
		uint32_t m = 0, t = 0;
		if (__ballot(diff != 0u) != 0ull) {                                                   // most wavefronts see one side only
#pragma unroll
			for (uint32_t c = 1; c < 8; ++c) m |= ((diff >> c) & 1u) << iso_edge_type(c);
			if (diff != 0u && ix && iy && iz) {
#pragma unroll
				for (int k = 0; k < 6; ++k) {
					const uint32_t tc = iso_tet_corners(k);
					const uint32_t n_above = (ab & 1u) + ((ab >> 7) & 1u) + ((ab >> ((tc >> 8) & 15u)) & 1u) + ((ab >> (tc >> 12)) & 1u);
					t += n_above == 2u ? 2u : (n_above == 1u || n_above == 3u) ? 1u : 0u;
				}
			}
		}
		mask[id] = (uint8_t)m; tcnt[id] = (uint8_t)t;
		nv += __popc(m); nt += t;
	}
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) { nv += __shfl_xor(nv, off); nt += __shfl_xor(nt, off); }
	if ((threadIdx.x & 63u) == 0) { sh[0][threadIdx.x >> 6] = nv; sh[1][threadIdx.x >> 6] = nt; }
	__syncthreads();
	if (threadIdx.x == 0) {
		uint32_t a = 0, b = 0;
		for (uint32_t w = 0; w < ISO_BLOCK / 64; ++w) { a += sh[0][w]; b += sh[1][w]; }
		tot_v[blockIdx.x] = a; tot_t[blockIdx.x] = b;
	}
}

// one workgroup walks the tile totals 1024 at a time with a 64-bit carry
__global__ __launch_bounds__(1024) void k_iso_scan_tiles(uint32_t tiles, const uint32_t *__restrict__ tot_v, const uint32_t *__restrict__ tot_t, uint64_t *__restrict__ base_v,
                                                         uint64_t *__restrict__ base_t, uint64_t *__restrict__ counts) {
	__shared__ uint32_t sh[17];
	uint64_t cv = 0, ct = 0;
	for (uint32_t first = 0; first < tiles; first += 1024u) {
		const uint32_t i = first + threadIdx.x;
		const uint32_t a = i < tiles ? tot_v[i] : 0u, b = i < tiles ? tot_t[i] : 0u;          // <= 7 * 1024 and 12 * 1024 each: 1024 of them fit 32 bits
		uint32_t ta, tb;
		const uint32_t ea = iso_block_scan(a, sh, ta), eb = iso_block_scan(b, sh, tb);
		if (i < tiles) { base_v[i] = cv + ea; base_t[i] = ct + eb; }
		cv += ta; ct += tb;
	}
	if (threadIdx.x == 0) { counts[0] = cv; counts[1] = ct; }
}

// thread t of tile b owns the four points b * 1024 + 4 t .. + 3
__global__ __launch_bounds__(ISO_BLOCK) void k_iso_emit_vertices(IsoShape s, double threshold, const float *__restrict__ u, const uint8_t *__restrict__ mask, const uint64_t *__restrict__ base_v,
                                                                 uint32_t *__restrict__ vbase, uint64_t n_vertices, double *__restrict__ vertices) {
	__shared__ uint32_t sh[17];
	const uint32_t id0 = blockIdx.x * ISO_TILE + threadIdx.x * 4u;
	uint32_t m4 = id0 < s.n ? *(const uint32_t *)(mask + id0) : 0u;                           // the arrays are padded to whole tiles; bytes past n were never written
	if (id0 + 4u > s.n && id0 < s.n) m4 &= 0xffffffffu >> (8u * (id0 + 4u - s.n));
	m4 &= 0x7f7f7f7fu;
	uint32_t total;
	const uint64_t first = base_v[blockIdx.x] + iso_block_scan(__popc(m4), sh, total);
	if (id0 >= s.n) return;
	uint64_t b = first;
	uint32_t out[4];
#pragma unroll
	for (uint32_t k = 0; k < 4; ++k) { out[k] = (uint32_t)b; b += __popc((m4 >> (8u * k)) & 0xffu); }
	*(uint4 *)(vbase + id0) = make_uint4(out[0], out[1], out[2], out[3]);
	if (m4 == 0u) return;
	const uint32_t YZ = s.Y * s.Z;
	b = first;
	for (uint32_t k = 0; k < 4; ++k) {
		uint32_t m = (m4 >> (8u * k)) & 0xffu;
		if (m == 0u) continue;
		const uint32_t id = id0 + k;
		const uint32_t x = id / YZ, rem = id - x * YZ, y = rem / s.Z, z = rem - y * s.Z;
		const double ulo = (double)u[id];
		while (m) {
			const uint32_t ty = __ffs(m) - 1u, d = ty + 1u;                                   // d = 4 dx + 2 dy + dz
			m &= m - 1u;
			const uint32_t dx = d >> 2, dy = (d >> 1) & 1u, dz = d & 1u;
			const double uhi = (double)u[id + dx * YZ + dy * s.Z + dz];                       // in the lattice: the classify pass marks no edge that leaves it
			const double t = (threshold - ulo) / (uhi - ulo);
			if (b < n_vertices) {
				double *o = vertices + 3ull * b;
				o[0] = (double)x + t * (double)dx; o[1] = (double)y + t * (double)dy; o[2] = (double)z + t * (double)dz;
			}
			++b;
		}
	}
}

struct IsoLookup {
	const uint8_t *mask; const uint32_t *vbase; uint32_t id, YZ, Z;
	// vertex on the edge between cube corners ca and cb
	__device__ __forceinline__ int32_t operator()(uint32_t ca, uint32_t cb) const {
		const uint32_t lo = min(ca, cb), ty = iso_edge_type(ca ^ cb);
		const uint32_t p = id + (lo & 1u) * YZ + ((lo >> 1) & 1u) * Z + (lo >> 2);
		return (int32_t)(vbase[p] + __popc((uint32_t)mask[p] & ((1u << ty) - 1u)));
	}
};

__global__ __launch_bounds__(ISO_BLOCK) void k_iso_emit_triangles(IsoShape s, double threshold, const float *__restrict__ u, const uint8_t *__restrict__ mask, const uint8_t *__restrict__ tcnt,
                                                                  const uint32_t *__restrict__ vbase, const uint64_t *__restrict__ base_t, uint64_t n_triangles, int32_t *__restrict__ triangles) {
	__shared__ uint32_t sh[17];
	const uint32_t id0 = blockIdx.x * ISO_TILE + threadIdx.x * 4u;
	uint32_t c4 = id0 < s.n ? *(const uint32_t *)(tcnt + id0) : 0u;
	if (id0 + 4u > s.n && id0 < s.n) c4 &= 0xffffffffu >> (8u * (id0 + 4u - s.n));
	c4 &= 0x0f0f0f0fu;
	const uint32_t mine = (c4 & 0xffu) + ((c4 >> 8) & 0xffu) + ((c4 >> 16) & 0xffu) + (c4 >> 24);
	uint32_t total;
	uint64_t b = base_t[blockIdx.x] + iso_block_scan(mine, sh, total);
	if (c4 == 0u) return;
	const uint32_t YZ = s.Y * s.Z;
	for (uint32_t k = 0; k < 4; ++k) {
		if (((c4 >> (8u * k)) & 0xffu) == 0u) continue;
		const uint32_t id = id0 + k;                                                          // a cube with triangles has all eight corners in the lattice
		uint32_t ab = 0;
#pragma unroll
		for (uint32_t c = 0; c < 8; ++c) ab |= ((double)u[id + (c & 1u) * YZ + ((c >> 1) & 1u) * s.Z + (c >> 2)] > threshold ? 1u : 0u) << c;
		const IsoLookup vert{mask, vbase, id, YZ, s.Z};
#pragma unroll
		for (int tet = 0; tet < 6; ++tet) {
			const uint32_t tc = iso_tet_corners(tet);
			uint32_t in = 0;
#pragma unroll
			for (uint32_t j = 0; j < 4; ++j) in |= ((ab >> ((tc >> (4u * j)) & 15u)) & 1u) << j;
			const uint32_t n_above = __popc(in);
			if (n_above == 0u || n_above == 4u) continue;
			const bool flip0 = (0x4d24u >> in) & 1u, flip1 = (0x0420u >> in) & 1u;          // where the host's geometric test reverses the triangle (all six tetrahedra have one handedness)
			int32_t v0, v1, v2, w1 = 0, w2 = 0;
			if (n_above == 2u) {                                                              // a, b above and c, d below in local order: (ac, ad, bd) and (ac, bd, bc)
				const uint32_t out = ~in & 15u;
				const uint32_t ca = (tc >> (4u * (__ffs(in) - 1u))) & 15u, cb = (tc >> (4u * (31u - __clz(in)))) & 15u;
				const uint32_t cc = (tc >> (4u * (__ffs(out) - 1u))) & 15u, cd = (tc >> (4u * (31u - __clz(out)))) & 15u;
				v0 = vert(ca, cc); v1 = vert(ca, cd); v2 = vert(cb, cd); w1 = v2; w2 = vert(cb, cc);
			} else {                                                                          // one corner alone on its side, the others in local order
				const uint32_t lone = __ffs(n_above == 1u ? in : (~in & 15u)) - 1u;
				const uint32_t ca = (tc >> (4u * lone)) & 15u;
				const uint32_t o0 = lone == 0u ? 1u : 0u, o1 = lone <= 1u ? 2u : 1u, o2 = lone == 3u ? 2u : 3u;
				v0 = vert(ca, (tc >> (4u * o0)) & 15u); v1 = vert(ca, (tc >> (4u * o1)) & 15u); v2 = vert(ca, (tc >> (4u * o2)) & 15u);
			}
			if (b < n_triangles) {
				int32_t *o = triangles + 3ull * b;
				o[0] = flip0 ? v2 : v0; o[1] = v1; o[2] = flip0 ? v0 : v2;
			}
			++b;
			if (n_above == 2u) {
				if (b < n_triangles) {
					int32_t *o = triangles + 3ull * b;
					o[0] = flip1 ? w2 : v0; o[1] = w1; o[2] = flip1 ? v0 : w2;
				}
				++b;
			}
		}
	}
}

static int iso_check_shape(const char *who, uint32_t X, uint32_t Y, uint32_t Z, size_t workspace_bytes, IsoShape *s, IsoWs *w) {
	NGP_REQUIRE(X >= 2 && Y >= 2 && Z >= 2, NGP_E_ARG, "%s: every lattice dimension must be at least 2 (got %u x %u x %u)", who, X, Y, Z);
	const uint64_t n = (uint64_t)X * Y * Z;
	NGP_REQUIRE((uint64_t)X * Y <= ISO_MAX_POINTS && n <= ISO_MAX_POINTS, NGP_E_CAPACITY, "%s: %u x %u x %u lattice points exceed 2^31 - 1", who, X, Y, Z);
	*s = IsoShape{X, Y, Z, (uint32_t)n};
	*w = iso_layout(n);
	NGP_REQUIRE(workspace_bytes >= w->bytes, NGP_E_CAPACITY, "%s: workspace of %zu bytes, ngp_iso_workspace_bytes asks for %llu", who, workspace_bytes, (unsigned long long)w->bytes);
	return 0;
}

NGP_API size_t ngp_iso_workspace_bytes(uint32_t X, uint32_t Y, uint32_t Z) {
	if (X < 2 || Y < 2 || Z < 2) return 0;
	const uint64_t n = (uint64_t)X * Y * Z;
	if ((uint64_t)X * Y > ISO_MAX_POINTS || n > ISO_MAX_POINTS) return 0;
	return (size_t)iso_layout(n).bytes;
}

NGP_API int ngp_iso_count(void *stream, const float *u, uint32_t X, uint32_t Y, uint32_t Z, double threshold, void *workspace, size_t workspace_bytes, uint64_t *counts) {
	NGP_REQUIRE(u && workspace && counts, NGP_E_ARG, "ngp_iso_count: null pointer");
	NGP_REQUIRE(((uintptr_t)workspace & 15u) == 0 && ((uintptr_t)counts & 7u) == 0, NGP_E_ALIGN, "ngp_iso_count: workspace must be 16-byte aligned, counts 8-byte aligned");
	IsoShape s; IsoWs w;
	if (int rc = iso_check_shape("ngp_iso_count", X, Y, Z, workspace_bytes, &s, &w)) return rc;
	hipStream_t st = (hipStream_t)stream;
	uint8_t *ws = (uint8_t *)workspace;
	uint32_t *tot = (uint32_t *)(ws + w.tot);
	uint64_t *base = (uint64_t *)(ws + w.base);
	NGP_LAUNCH(k_iso_classify, dim3(w.tiles), dim3(ISO_BLOCK), 0, st, s, threshold, u, ws + w.mask, ws + w.tcnt, tot, tot + w.tiles);
	NGP_LAUNCH(k_iso_scan_tiles, dim3(1), dim3(1024), 0, st, w.tiles, (const uint32_t *)tot, (const uint32_t *)(tot + w.tiles), base, base + w.tiles, counts);
	NGP_LAUNCH_CHECK("ngp_iso_count");
	return 0;
}

NGP_API int ngp_iso_emit(void *stream, const float *u, uint32_t X, uint32_t Y, uint32_t Z, double threshold, const void *workspace, size_t workspace_bytes, uint64_t n_vertices,
                         uint64_t n_triangles, double *vertices, int32_t *triangles) {
	NGP_REQUIRE(u && workspace, NGP_E_ARG, "ngp_iso_emit: null pointer");
	NGP_REQUIRE((vertices || n_vertices == 0) && (triangles || n_triangles == 0), NGP_E_ARG, "ngp_iso_emit: null output for %llu vertices, %llu triangles", (unsigned long long)n_vertices,
	            (unsigned long long)n_triangles);
	NGP_REQUIRE(((uintptr_t)workspace & 15u) == 0 && ((uintptr_t)vertices & 7u) == 0 && ((uintptr_t)triangles & 3u) == 0, NGP_E_ALIGN, "ngp_iso_emit: workspace must be 16-byte aligned, outputs naturally aligned");
	IsoShape s; IsoWs w;
	if (int rc = iso_check_shape("ngp_iso_emit", X, Y, Z, workspace_bytes, &s, &w)) return rc;
	NGP_REQUIRE(n_vertices <= ISO_MAX_POINTS && n_triangles <= ISO_MAX_POINTS, NGP_E_CAPACITY, "ngp_iso_emit: %llu vertices / %llu triangles exceed 2^31 - 1 (int32 indices)",
	            (unsigned long long)n_vertices, (unsigned long long)n_triangles);
	if (n_vertices == 0 && n_triangles == 0) return 0;
	hipStream_t st = (hipStream_t)stream;
	// the emit kernels only read the workspace's masks, counts and tile bases; the per-point vertex bases are the one part they fill in
	uint8_t *ws = (uint8_t *)const_cast<void *>(workspace);
	const uint64_t *base = (const uint64_t *)(ws + w.base);
	NGP_LAUNCH(k_iso_emit_vertices, dim3(w.tiles), dim3(ISO_BLOCK), 0, st, s, threshold, u, (const uint8_t *)(ws + w.mask), base, (uint32_t *)(ws + w.vbase), n_vertices, vertices);
	if (n_triangles)
		NGP_LAUNCH(k_iso_emit_triangles, dim3(w.tiles), dim3(ISO_BLOCK), 0, st, s, threshold, u, (const uint8_t *)(ws + w.mask), (const uint8_t *)(ws + w.tcnt),
		           (const uint32_t *)(ws + w.vbase), base + w.tiles, n_triangles, triangles);
	NGP_LAUNCH_CHECK("ngp_iso_emit");
	return 0;
}
