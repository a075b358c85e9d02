"""(r11) k_hash_fwd_x2 (csrc/hash_encode.hip), the fp32 hash forward: the level kind - dense, hashed with a power-of-two size, the general fallback - is chosen once per
workgroup and each kind has its own loop body; a trip of the sample loop holds two samples' loads (i and i + 128 * chunks) with single-sample trips for what is left; the
number of 128-sample chunks in flight depends on the launch size and NGP_HASH_FWD_CHUNKS forces it.

GPU part: fp32 output against the CPU oracle O.hash_encode_fwd, bit for bit (same table entries, same weights, the eight terms in the reference's order: no tolerance).
  sizes      n in {1, 127, 128, 129, 1000, 8209}; 8209 = 65 chunks with a ragged last one
  chunks     NGP_HASH_FWD_CHUNKS in {unset, 1, 3, 17, 64}: at n = 8209 loops of 65, 22, 4 and 2 trips - odd trip counts, and last trips in which only the first sample of
             the pair exists - each under NGP_HASH_FWD_MAP = 1 (the XCDs in pairs) and 0 (rounds 6-9's map); both hooks are read per call
  arguments  n_valid absent, 0, 1 and n - 5 (rows from the count on keep the sentinel the output was filled with); position row stride 3 and 7; AOS and SOA output
  tables     aabb_scale 1 and 4 (tests/golden_cases.py, tests/reference_configs.py: the tables of ngp_base.py and ngp_fox.py) hold dense levels and 2^19-entry hashed ones
             and NO hashed level whose size is not a power of two, so the fallback body is reached only through a synthetic level table: aabb_scale 1's resolutions with
             its hashed levels cut to 500 008, 300 000, ... entries (sizes GridEncode never builds; the oracle indexes any size).  A level beyond 2^28 entries, the
             fallback's other customer, would need a 2 GiB table and is not run.
  positions  uniform random; ray-coherent (consecutive steps along camera rays of tests/synth.py: equal addresses within a wavefront); a set pinned to 0.0, 1.0, the cell
             boundaries and the last cell of every dense level (and a few points beyond the box, where grid_index divides) - the oracle's index arithmetic, restated
             here, must take the `index >= size` wrap of the +1 corner on that set: a condition of the test
CPU part: k_hash_fwd_x2<float, SOA | AOS, paired map> uses no scratch and no LDS and runs at no fewer waves per SIMD than before this round (8, at 34 VGPRs then)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_MAX = 8209
SIZES = [1, 127, 128, 129, 1000, N_MAX]
CHUNKS = [None, 1, 3, 17, 64]
MAPS = [1, 0]
SENTINEL = 0xDEADBEEF
WAVES_PER_SIMD_BEFORE = 8                  # k_hash_fwd_x2<float, *, paired> at the parent of this round: 34 VGPRs, 0 B scratch, no LDS


def test_hash_fwd_x2_resources():
    """device-only compile through tools/kernel_resources.py: the paired-map instantiations of both layouts"""
    import shutil
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not installed")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), os.path.join(ROOT, "jnerf_amd", "csrc", "hash_encode.hip"), "k_hash_fwd_x2<float"],
                         capture_output=True, text=True, timeout=600).stdout
    print(out)
    rows = [l.split() for l in out.splitlines() if l.startswith("void k_hash_fwd_x2<float,") and l.split(">")[0].endswith(", 1")]      # MAP = X2_MAP_PAIRED
    assert len(rows) == 2, out
    for r in rows:                                      # columns: ... VGPR AGPR SGPR occ scratch LDS
        assert r[-2] == "0" and r[-1] == "0", r
        assert int(r[-3]) >= WAVES_PER_SIMD_BEFORE, r


# ---------------------------------------------------------------------------------------------------------------- level tables and position sets (CPU)
def _kinds(table):
    """per level: 'dense' | 'hash_pow2' | 'general', as the kernel (and HashEncode.h:82-91) decides it"""
    out = []
    for off, size, res, _ in table.tolist():
        stride = 1
        for _d in range(3):
            if stride <= size:
                stride *= res
        dense = not (size < stride)
        out.append("dense" if dense else "hash_pow2" if size & (size - 1) == 0 else "general")
    return out


def _synthetic_table():
    """aabb_scale 1's resolutions and scales; its hashed levels get sizes that are not powers of two (multiples of 8, like every size GridEncode builds)"""
    from oracle import oracle as O
    table = O.level_table(1)[0].copy()
    odd = [500008, 300000, 524280, 262152, 100000, 48]
    off, k = 0, 0
    for l, kind in enumerate(_kinds(table)):
        if kind != "dense":
            table[l, 1] = odd[k % len(odd)]; k += 1
        table[l, 0] = off
        off += int(table[l, 1])
    return table, off * 2


def _scale(table, l):
    return float(table[l, 3:4].view(np.float32)[0])


def _uniform():
    import synth
    return synth.uniform_positions(N_MAX, seed=21)


def _rays():
    """64 consecutive steps of sqrt(3) / 1024 along camera rays aimed at the box, clamped to it: runs of samples in one cell on the coarse levels"""
    import synth
    xf, focal, meta = synth.camera_ring(6, W=64, H=48, seed=5)
    _, o, d, _ = synth.rays_from_cameras(xf, focal, meta, 64, 48, (N_MAX + 63) // 64, seed=6)
    t = (np.float32(0.85) + np.arange(64, dtype=np.float32) * np.float32(np.sqrt(3.0) / 1024))[None, :, None]
    return np.clip(o[:, None, :] + d[:, None, :] * t, 0, 1).astype(np.float32).reshape(-1, 3)[:N_MAX].copy()


def _pinned(table):
    """0.0, 1.0, lattice planes of every dense level (with their float neighbours) and its last cell, a few points beyond the box; repeated up to N_MAX rows"""
    pts = [[0, 0, 0], [1, 1, 1], [1, 0, 0.5], [0, 1, 1], [1, 1, 0], [0.5, 1, 0.5], [1, 0.25, 1], [0, 0, 1], [1.5, 0.5, 0.5], [2.2, 2.2, 2.2], [1.03, 1.0, 0.99]]
    for l, kind in enumerate(_kinds(table)):
        if kind != "dense":
            continue
        scale, res = _scale(table, l), int(table[l, 2])
        for g in (1, res // 2, res - 2, res - 1):
            b = np.float32((g - 0.5) / scale)                                          # p = b * scale + 0.5 lands on (or one ulp beside) the lattice plane g
            for v in (np.nextafter(b, np.float32(0)), b, np.nextafter(b, np.float32(2))):
                if 0 <= v <= 1:
                    pts += [[v, v, v], [v, 0.5, 0.25], [0.75, v, 1.0], [1.0, 1.0, v]]
        last = np.float32(1.0 - 0.25 / scale)                                          # inside the last cell
        pts += [[last, last, last], [last, 1.0, 1.0], [1.0, last, 0.5]]
    x = np.array(pts, np.float32)
    return np.resize(x, (N_MAX, 3)).copy()


def _dense_wraps(table, x):
    """the oracle's index arithmetic (oracle/ngp_oracle.c grid_index) on the dense levels: how many corners have index >= size before the modulo"""
    count = 0
    for l, kind in enumerate(_kinds(table)):
        if kind != "dense":
            continue
        size, res, scale = int(table[l, 1]), int(table[l, 2]), np.float32(_scale(table, l))
        g = np.floor(x * scale + np.float32(0.5)).astype(np.int64)
        for k in range(8):
            c = g + np.array([k & 1, (k >> 1) & 1, k >> 2])
            index = (c[:, 0] + c[:, 1] * res + c[:, 2] * res * res) & 0xFFFFFFFF
            count += int((index >= size).sum())
    return count


class _Case:
    """one level table with its fp32 grid on the device and, per position set, the oracle's output - computed once, read-only"""
    def __init__(self, name):
        import torch
        from oracle import oracle as O
        import synth
        self.O, self.name = O, name
        if name == "synthetic":
            self.table, self.n_params = _synthetic_table()
        else:
            self.table, _, self.n_params = O.level_table(int(name))
        self.kinds = _kinds(self.table)
        self.grid = synth.table(self.n_params, np.float32, amp=2.0)
        self.grid_t = torch.from_numpy(self.grid).cuda()
        self.sets = {}

    def positions(self, which):
        """-> (x [N_MAX, 3], oracle rows [N_MAX, 32], x on the device with row stride 3, with row stride 7)"""
        if which not in self.sets:
            import torch
            x = {"uniform": _uniform, "rays": _rays, "pinned": lambda: _pinned(self.table)}[which]()
            ref = self.O.hash_encode_fwd(x, self.grid, self.table)
            ref.setflags(write=False)
            x3 = torch.from_numpy(x).cuda()
            buf = torch.full((N_MAX, 7), float("nan"), device="cuda")
            buf[:, 2:5] = x3
            self.sets[which] = (x, ref, x3, buf[:, 2:5])
        return self.sets[which]

    def run(self, x_t, layout, n_valid=None, out=None):
        """-> [n, 32] float32 rows whatever the layout"""
        from jnerf_amd import ops
        y = ops.hash_encode_fwd(x_t, self.grid_t, self.table, out=out, layout=layout, n_valid=n_valid).detach().cpu().numpy()
        return y if layout == ops.LAYOUT_AOS else np.ascontiguousarray(y.transpose(1, 0, 2)).reshape(-1, 32)


_CASES = {}
TABLES = ["1", "4", "synthetic"]


@pytest.fixture(params=TABLES)
def case(request, monkeypatch):
    monkeypatch.setenv("NGP_HASH_FWD_RUNS", "0")        # one k_hash_fwd_x2 launch over all sixteen levels
    monkeypatch.setenv("NGP_HASH_FWD_X2", "1")
    if request.param not in _CASES:
        _CASES[request.param] = _Case(request.param)
    return _CASES[request.param]


def _set_hooks(monkeypatch, chunks, paired):
    if chunks is None:
        monkeypatch.delenv("NGP_HASH_FWD_CHUNKS", raising=False)
    else:
        monkeypatch.setenv("NGP_HASH_FWD_CHUNKS", str(chunks))
    monkeypatch.setenv("NGP_HASH_FWD_MAP", str(paired))


def _table(name):
    from oracle import oracle as O
    return _synthetic_table()[0] if name == "synthetic" else O.level_table(int(name))[0]


def test_every_level_kind_is_covered():
    """(CPU) the three tables together hold every kind the kernel distinguishes; the reference's own tables hold dense and 2^19-entry hashed levels only"""
    real = [k for s in ("1", "4") for k in _kinds(_table(s))]
    assert "dense" in real and "hash_pow2" in real and "general" not in real
    for s in ("1", "4"):
        t = _table(s)
        assert all(int(t[l, 1]) == 1 << 19 for l, k in enumerate(_kinds(t)) if k == "hash_pow2")
    syn = _kinds(_table("synthetic"))
    assert "general" in syn and "dense" in syn and "hash_pow2" not in syn


@pytest.mark.parametrize("name", TABLES)
def test_pinned_set_takes_the_dense_wrap(name):
    """(CPU) a condition of test_sizes_chunks_maps[pinned]: the oracle wraps at least one +1 corner of a dense level on the pinned set, also among its positions inside the
    box (1.0 on level 0: 16 + 16 * 16 + 16 * 256 >= 4096)"""
    table = _table(name)
    x = _pinned(table)
    assert "dense" in _kinds(table)
    assert _dense_wraps(table, x) > 0
    inside = x[(x <= 1).all(axis=1) & (x >= 0).all(axis=1)]
    assert _dense_wraps(table, inside) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["uniform", "rays", "pinned"])
def test_sizes_chunks_maps(case, which, monkeypatch):
    """every size x chunks in flight x map x layout, bit for bit"""
    from jnerf_amd import ops
    x, ref, x3, _ = case.positions(which)
    for paired in MAPS:
        for chunks in CHUNKS:
            _set_hooks(monkeypatch, chunks, paired)
            for n in SIZES:
                for layout in (ops.LAYOUT_SOA, ops.LAYOUT_AOS):
                    out = case.run(x3[:n], layout)
                    bad = np.flatnonzero((out.view(np.uint32) != ref[:n].view(np.uint32)).any(axis=1))
                    assert bad.size == 0, f"table {case.name} {which} map {paired} chunks {chunks} n {n} layout {layout}: {bad.size} rows differ, first {bad[:5]}"


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["uniform", "pinned"])
def test_count_stride_layout(case, which, monkeypatch):
    """n_valid absent, 0, 1, n - 5 x row stride 3, 7 x layout x chunks unset, 3, 17 (one-, many- and few-trip loops) x map: rows below the count equal the oracle's, rows
    from the count on keep the sentinel"""
    import torch
    from jnerf_amd import ops
    x, ref, x3, x7 = case.positions(which)
    ref_u = ref.view(np.uint32)
    for paired in MAPS:
        for chunks in (None, 3, 17):
            _set_hooks(monkeypatch, chunks, paired)
            for n in (1000, N_MAX):
                for nv in (None, 0, 1, n - 5):
                    cnt = None if nv is None else torch.tensor([nv], dtype=torch.int32, device="cuda")
                    lim = n if nv is None else nv
                    for x_t in (x3[:n], x7[:n]):
                        for layout in (ops.LAYOUT_SOA, ops.LAYOUT_AOS):
                            shape = (n, 32) if layout == ops.LAYOUT_AOS else (16, n, 2)
                            out = torch.from_numpy(np.full(shape, SENTINEL, np.uint32).view(np.float32)).cuda()
                            got = case.run(x_t, layout, n_valid=cnt, out=out).view(np.uint32)
                            what = (case.name, which, paired, chunks, n, nv, x_t.stride(0), layout)
                            assert np.array_equal(got[:lim], ref_u[:lim]), what
                            assert (got[lim:] == SENTINEL).all(), what
