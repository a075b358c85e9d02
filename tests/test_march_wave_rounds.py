"""The wave-per-ray count pass (csrc/sampler.hip, k_march_wave) round by round: small hand-built inputs that reach the paths a round can take - a skip that is still
running when a round ends (and one that passes a whole round), NERF_STEPS reached inside a round, binade crossings of the constant-step chain on and off a window's
edges, the verify-and-fallback of the parallel walk, rays that end before their first round.  Every case marches the same rays with the cooperative and with the serial
count pass and compares both, bit for bit, with the CPU port (oracle.march_rays + oracle.compact_coords).  At most 257 rays, one 128^3 bitfield per cascade.

The last test needs no GPU: it reads the compiler's assembly of both instantiations of the kernel."""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from oracle import oracle as O
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
G = 128
NC = 256                                    # candidates per round of k_march_wave<4, .>
NERF_STEPS = 1024
MIN_STEP = F(1.73205080757) / F(1024)       # min_cone_stepsize()


@pytest.fixture(scope="module")
def H():
    import hip_impl
    return hip_impl


# ---------------------------------------------------------------------------------------------------------------- inputs
_cache = {}


def _shared(key, make):
    """inputs and references are computed once per module and never written to afterwards"""
    if key not in _cache:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = v
    return _cache[key]


def _box_bits(cascades, lo, hi):
    """occupancy: at every cascade, the cells that meet the world-space box [lo, hi]"""
    bits = np.zeros(cascades * G ** 3 // 8, np.uint8)
    for c in range(cascades):
        r = []
        for k in range(3):
            a = int(np.floor(((lo[k] - 0.5) / 2.0 ** c + 0.5) * G)), int(np.floor(((hi[k] - 0.5) / 2.0 ** c + 0.5) * G))
            r.append(np.arange(max(a[0], 0), min(a[1], G - 1) + 1))
        X, Y, Z = np.meshgrid(*r, indexing="ij")
        cell = synth.morton3D(X.ravel(), Y.ravel(), Z.ravel()) + np.uint32(c * G ** 3)
        np.bitwise_or.at(bits, cell // 8, (np.uint8(1) << (cell % 8).astype(np.uint8)))
    return bits


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def _random_rays(n, aabb, seed):
    """origins inside and around the box, aimed at points inside it"""
    rng = np.random.default_rng(seed)
    lo, hi = aabb
    o = rng.uniform(lo - 0.6 * (hi - lo), hi + 0.6 * (hi - lo), (n, 3)).astype(np.float32)
    o[: n // 3] = rng.uniform(lo, hi, (n // 3, 3)).astype(np.float32)
    return o, _unit(rng.uniform(lo, hi, (n, 3)) - o)


# ---------------------------------------------------------------------------------------------------------------- the check every case makes
def _check(H, o, d, bits, aabb, const_dt, cascades=5, cone_angle=1.0 / 256, near=0.2, cap=None):
    """cooperative == serial == CPU port, bit for bit: numsteps, numsteps_compacted, the counters and every written row of coords.  -> the port's (numsteps, coords)"""
    from jnerf_amd import _lib
    o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
    n = o.shape[0]
    max_samples = n * NERF_STEPS
    co, no, cnto, _ = O.march_rays(o, d, bits, aabb, O.PCG32(1337), max_samples, cone_angle, near, const_dt, cascades)
    M = int(cnto[1])
    cap = M + 5 if cap is None else cap
    cc, nc, ccnt = O.compact_coords(co[:M], no, cap)
    k = min(M, cap)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    res = {}
    try:
        for name, mode in (("coop", 2), ("serial", 1)):
            lib.ngp_x_march_count_mode(mode)
            # (copies: the shared inputs are read-only, and a tensor made from a read-only array warns)
            res[name] = H.march_rays_compacted(o.copy(), d.copy(), np.array(bits), aabb, O.PCG32(1337), max_samples, cap, cone_angle, near, const_dt, cascades)
    finally:
        lib.ngp_x_march_count_mode(0)
    for name in ("coop", "serial"):
        c, ns, nsc, cnt = res[name]
        assert np.array_equal(ns, no), name
        assert np.array_equal(nsc, nc), name
        assert cnt[1] == cnto[1] and cnt[2] == ccnt[0] and cnt[3] == k, (name, cnt, cnto, ccnt, k)
        assert np.array_equal(c[:k].view(np.uint32), cc[:k].view(np.uint32)), name
    assert all(np.array_equal(a, b) for a, b in zip(res["coop"][1:], res["serial"][1:]))
    return no, co


# ---------------------------------------------------------------------------------------------------------------- a scalar fp32 port of one ray's traversal
def _calc_dt(t, cone_angle, const_dt, cascades):
    if const_dt:
        return F(MIN_STEP * F(0.5))
    hi = F(MIN_STEP * F(1 << (cascades - 1)) * F(NERF_STEPS) / F(G))
    v = F(t * F(cone_angle))
    return MIN_STEP if v < MIN_STEP else (hi if hi < v else v)


def _t_sequence(startt, count, cone_angle, const_dt, cascades):
    """the ray's fixed sequence t_0 = start, t_{k+1} = fl(t_k + calc_dt(t_k)): real fp32 adds, the thing the kernel's closed-form chain must reproduce"""
    t, out = F(startt), []
    for _ in range(count):
        out.append(t)
        t = F(t + _calc_dt(t, cone_angle, const_dt, cascades))
    return np.asarray(out, np.float32)


def _trace(o, d, startt, bits, aabb, cone_angle, const_dt, cascades):
    """ray_sampler.h:52-69 for one ray, as indices into its fixed sequence -> (emitted [(candidate, pos)], skips [(from candidate, landing candidate)])"""
    a0, a1 = F(aabb[0]), F(aabb[1])
    o, d = [F(x) for x in o], [F(x) for x in d]
    with np.errstate(divide="ignore"):
        idir = [F(1.0) / x for x in d]
    emitted, skips = [], []
    t, k = F(startt), 0
    while True:
        pos = [F(o[a] + F(t * d[a])) for a in range(3)]
        if not all(a0 <= p <= a1 for p in pos) or len(emitted) >= NERF_STEPS:
            break
        dt = _calc_dt(t, cone_angle, const_dt, cascades)
        mip = min(cascades - 1, max(0, int(np.frexp(max(abs(F(p - F(0.5))) for p in pos))[1]) + 1))
        dt2 = F(dt * F(2 * G))
        if not dt2 < F(1.0):
            mip = min(cascades - 1, max(int(np.frexp(dt2)[1]), mip))
        sc = F(2.0 ** -mip)
        c = [min(max(int(F(F(F(F(p - F(0.5)) * sc) + F(0.5)) * F(G))), 0), G - 1) for p in pos]
        idx = int(synth.morton3D(np.uint32(c[0]), np.uint32(c[1]), np.uint32(c[2])))
        if (int(bits[idx // 8 + (G ** 3 * mip) // 8]) >> (idx % 8)) & 1:
            emitted.append((k, pos))
            t = F(t + dt); k += 1
            continue
        res = F(G >> mip)
        with np.errstate(invalid="ignore"):
            t3 = []
            for a in range(3):
                q = F(res * pos[a])
                t3.append(F(F(np.floor(F(F(q + F(0.5)) + F(F(0.5) * np.copysign(F(1.0), d[a])))) - q) * idir[a]))
            tt = np.fmin(np.fmin(t3[0], t3[1]), t3[2])
            target = F(t + np.fmax(F(tt / res), F(0.0)))
        k0 = k
        while True:
            t = F(t + _calc_dt(t, cone_angle, const_dt, cascades)); k += 1
            if not t < target:
                break
        skips.append((k0, k))
    return emitted, skips


def _start_of_ray0_inside(near, cone_angle, const_dt, cascades):
    """ray 0 starts inside the box: the box entry lies behind it, so the march starts at near + calc_dt(near) * (the ray's first random number)"""
    u = F(O.PCG32(1337).next_float())
    return F(F(near) + F(_calc_dt(F(near), cone_angle, const_dt, cascades) * u))


# ---------------------------------------------------------------------------------------------------------------- GPU cases
@pytest.mark.gpu
def test_skip_across_round_boundaries(H):
    """Cone stepping through five cascades.  Ray 0 creeps along x (a short direction vector: a cascade-4 cell is hundreds of steps long) through empty space towards an
    occupied box, so single skips are still running when their round ends (`pend`), and at least one passes a whole round (`s == NC`)."""
    aabb, cascades, cone, near = (-7.5, 8.5), 5, 1.0 / 256, 0.2
    bits = _shared("skip_bits", lambda: _box_bits(cascades, (-3.0, -1.0, -1.0), (-1.5, 2.0, 2.0)))
    o, d = _random_rays(64, aabb, seed=7)
    o[0], d[0] = (-6.03, 0.37, 0.61), (0.05, 0.0004, -0.0003)
    o[1], d[1] = (-6.03, 0.37, 0.61), (0.02, 0.0004, -0.0003)
    no, co = _check(H, o, d, bits, aabb, False, cascades, cone, near)
    # the port's trace of ray 0, held against the oracle, shows the paths
    em, skips = _trace(o[0], d[0], _start_of_ray0_inside(near, cone, False, cascades), bits, aabb, cone, False, cascades)
    assert len(em) == no[0, 0] > 0 and no[0, 1] == 0
    want = np.asarray([[F(F(p - F(aabb[0])) / F(F(aabb[1]) - F(aabb[0]))) for p in pos] for _, pos in em], np.float32)
    assert np.array_equal(want, co[:len(em), :3])
    assert max(b - a for a, b in skips) > NC, "no skip of more than one round's candidates"
    assert any(b // NC >= a // NC + 2 for a, b in skips), "no skip passes a whole round"
    assert any(b // NC == a // NC + 1 for a, b in skips), "no skip ends in the round after the one it starts in"
    assert em[0][0] >= max(b for a, b in skips if b // NC >= a // NC + 2), "nothing is emitted behind the long skip"


@pytest.mark.gpu
@pytest.mark.parametrize("const_dt,aabb,cone", [(True, (-0.5, 1.5), 1.0 / 256), (False, (-1.5, 2.5), 1.0 / 1024)])
@pytest.mark.parametrize("grid", ["full", "full_with_gap"])
def test_nerf_steps_reached_in_a_round(H, grid, const_dt, aabb, cone):
    """Every cell occupied, a box two (constant step) or four (cone stepping, a narrow cone) times the unit cube: a diagonal ray has 2000 - 4000 candidates and stops at
    1024 samples.  With every candidate emitting, the limit falls on a round's end; an empty slab (full_with_gap) moves it inside a round for the rays that cross the
    slab before their 1024th sample, ray 0 among them."""
    cascades = 5

    def make():
        b = np.full(cascades * G ** 3 // 8, 0xFF, np.uint8)
        if grid == "full_with_gap":
            gap = _box_bits(cascades, (0.40, -1.5, -1.5), (0.47, 2.5, 2.5))
            gap[2 * G ** 3 // 8:] = 0                                      # (in cascades 0 and 1: what candidates near the centre select)
            b &= ~gap
        return b
    bits = _shared(("steps_bits", grid), make)
    o, d = _random_rays(48, aabb, seed=11)
    o[0], d[0] = (0.2, 0.21, 0.19), _unit((1.0, 1.01, 0.99))               # along the diagonal from inside: reaches the slab after 90 - 180 candidates
    o[1], d[1] = (aabb[0] - 0.3, aabb[0] - 0.3, aabb[0] - 0.3), _unit((1.0, 1.01, 0.99))      # the diagonal, corner to corner
    no, _ = _check(H, o, d, bits, aabb, const_dt, cascades, cone, cap=48 * NERF_STEPS)
    assert no[0, 0] == NERF_STEPS and no[1, 0] == NERF_STEPS and (no[:, 0] == NERF_STEPS).sum() >= 8
    if grid == "full_with_gap":
        em, skips = _trace(o[0], d[0], _start_of_ray0_inside(0.2, cone, const_dt, cascades), bits, aabb, cone, const_dt, cascades)
        assert len(em) == NERF_STEPS and skips and (em[-1][0] + 1) % NC != 0, "the limit falls on a round's end"


@pytest.mark.gpu
def test_binade_crossings_on_and_off_window_edges(H):
    """Constant step: the chain writes (a0 + i q) U inside a binade and takes real fp32 adds around a crossing.  Rays along x enter the unit box at a t chosen so that
    the sequence first reaches 0.5, 1.0 or 2.0 at a given candidate: a window's first (64, 128) and last (63, 127) candidate, a round's (255, 256), and inside a window."""
    aabb, cascades = (0.0, 1.0), 5
    bits = _shared("shell_bits", synth.shell_bitfield)
    dt = _calc_dt(F(0), 0.0, True, cascades)
    plan = [(B, m) for B in (0.5, 1.0, 2.0) for m in (20, 63, 64, 127, 128, 255, 256, 300)]
    o = np.zeros((len(plan), 3), np.float32); d = np.zeros((len(plan), 3), np.float32)
    starts = []
    for i, (B, m) in enumerate(plan):
        rng = O.PCG32(1337); rng.advance(i * 8)
        u = F(rng.next_float())
        T0 = F(B + (0.5 - m - float(u)) * float(dt))                        # the box entry: candidate m is the first at or above B, by half a step
        o[i] = (-float(T0), 0.41 + 0.004 * i, 0.47 + 0.002 * i)
        d[i] = (1.0, 2e-3 if i % 3 else 0.0, -1e-3 if i % 2 else 0.0)        # (some with zero components: infinite idir)
        tmin = F(F(F(0.0) - o[i, 0]) / d[i, 0])                               # BoundingBox::ray_intersect along x; the y and z slabs are entered long before
        starts.append(F(tmin + F(dt * u)))
        assert T0 > 0.2
    seen = set()
    for (B, m), s in zip(plan, starts):
        seq = _t_sequence(s, m + 2, 0.0, True, cascades)
        first = int(np.argmax(seq >= F(B)))
        assert first == m and seq[m - 1] < F(B), (B, m, first)
        seen.add(first % 64)
    assert {0, 63, 20, 44} <= seen
    no, _ = _check(H, o, d, bits, aabb, True, cascades)
    assert (no[:, 0] > 0).sum() >= len(plan) // 2


@pytest.mark.gpu
@pytest.mark.parametrize("const_dt,aabb", [(True, (0.0, 1.0)), (False, (-1.5, 2.5))])
def test_walk_falls_back_on_a_random_grid(H, const_dt, aabb):
    """Half the cells occupied, each on its own: skips of every length, two candidates of one empty cell landing differently (the parallel walk's check fails and
    lane 0 walks the links)."""
    bits = _shared("random_bits", lambda: np.packbits(np.random.default_rng(41).random(5 * G ** 3) < 0.5, bitorder="little"))
    o, d = _random_rays(64, aabb, seed=5)
    no, _ = _check(H, o, d, bits, aabb, const_dt)
    assert (no[:, 0] > 100).sum() >= 16


@pytest.mark.gpu
@pytest.mark.parametrize("const_dt,aabb", [(True, (0.0, 1.0)), (False, (-1.5, 2.5))])
@pytest.mark.parametrize("n_rays", [1, 63, 257])
def test_degenerate_rays_and_ragged_counts(H, n_rays, const_dt, aabb):
    """rays that miss the box, start inside it, run along an axis (zero direction components: infinite idir), point away from it; 1, 63 and 257 rays"""
    bits = _shared("shell_bits", synth.shell_bitfield)
    o, d = _shared(("degenerate_rays", aabb), lambda: _random_rays(257, aabb, seed=3))
    o, d = o.copy(), d.copy()
    lo, hi = aabb
    mid = 0.5 * (lo + hi)
    o[0], d[0] = (mid + 0.02, mid - 0.03, mid + 0.01), _unit((0.3, -0.5, 0.8))            # starts inside the box
    o[1], d[1] = (lo - 1.0, hi + 2.0, mid), (1.0, 0.0, 0.0)                                # misses the box, axis-parallel
    o[2], d[2] = (lo - 1.0, mid + 0.01, mid - 0.02), (1.0, 0.0, 0.0)                       # through the centre along x
    o[3], d[3] = (mid + 0.013, hi + 0.7, mid), (0.0, -1.0, 0.0)                            # along -y
    o[4], d[4] = (mid, mid + 0.03, lo - 0.5), (0.0, 0.0, 1.0)                              # along z
    o[5], d[5] = (lo - 1.0, mid, mid), _unit((-1.0, 0.1, 0.2))                             # points away: the box lies behind the ray
    o[6], d[6] = (lo - 0.5, mid + 0.21, mid), _unit((1.0, 0.0, 0.35))                      # one zero component
    o[7], d[7] = (hi + 3.0, hi + 3.0, hi + 3.0), _unit((1.0, 1.0, 1.0))                    # misses, diagonal
    if n_rays == 1:
        o, d = o[2:3], d[2:3]
    no, _ = _check(H, o[:n_rays], d[:n_rays], bits, aabb, const_dt)
    if n_rays > 8:
        assert no[0, 0] > 0 and no[2, 0] > 0 and no[1, 0] == 0 and no[5, 0] == 0 and no[7, 0] == 0
    else:
        assert no[0, 0] > 0


# ---------------------------------------------------------------------------------------------------------------- the compiler's assembly (no GPU)
def test_round_has_one_memory_round_trip_and_no_lds_cross_lane_moves():
    """Device-only compile of csrc/sampler.hip with build.sh's flags.  Both instantiations of k_march_wave<4, .>: no scratch; no ds_bpermute_b32 at all (there were 29: 24 in
    wave_incl_max, four __shfl_up(incl, 1), one __shfl of tgt[w]; the scan and the shift are DPP operands of v_max_u32 / v_mov_b32 now, the last a v_readlane_b32 - none
    remains); and the round's occupancy bytes - the kernel's last four byte loads, behind the one of the coarse map before the round loop - are issued with no
    `s_waitcnt vmcnt(0)` between the first and the last of them."""
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not installed")
    with tempfile.NamedTemporaryFile(suffix=".s") as f:
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics", "-fvisibility=hidden",
                            "-S", "--cuda-device-only", os.path.join(ROOT, "jnerf_amd", "csrc", "sampler.hip"), "-o", f.name, "-Rpass-analysis=kernel-resource-usage"],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        asm = open(f.name).read().split("\n")
    scratch, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (?:\S+ )?\s*(Function Name|ScratchSize \[bytes/lane\]): (\S+)", line)
        if m and m.group(1) == "Function Name":
            cur = m.group(2)
        elif m and cur is not None:
            scratch[cur] = int(m.group(2))
    for inst in ("k_march_waveILj4ELb1E", "k_march_waveILj4ELb0E"):
        name = [k for k in scratch if inst in k]
        assert len(name) == 1 and scratch[name[0]] == 0, (inst, scratch)
        start = next(i for i, l in enumerate(asm) if l.startswith("_Z") and inst in l and ":" in l)
        end = next(i for i in range(start, len(asm)) if asm[i].startswith(".Lfunc_end"))
        ins = [l.strip() for l in asm[start:end]]
        ins = [l for l in ins if l and not l.startswith((".", ";")) and not l.endswith(":")]
        assert sum(l.startswith("ds_bpermute_b32") for l in ins) == 0, inst
        loads = [i for i, l in enumerate(ins) if l.startswith("global_load_ubyte")]
        assert len(loads) >= 5, (inst, len(loads))
        first, last = loads[-4], loads[-1]
        between = ins[first:last + 1]
        assert not any(l.startswith("s_waitcnt") and "vmcnt(0)" in l for l in between), (inst, [l for l in between if l.startswith("s_waitcnt")])
        assert any(l.startswith("s_waitcnt") and "vmcnt" in l for l in ins[last:last + 400]), inst      # (the bytes are waited for behind the last load, not never)
