"""(r10) The two routings of the fp32 hash forward (ngp_hash_encode_fwd, csrc/hash_encode.hip).  Default: one k_hash_fwd_x2 launch whose workgroups are dealt to the XCDs in
pairs (block_to_level_chunk_paired, csrc/hash_fwd_runs.h).  NGP_HASH_FWD_RUNS=1: k_hash_fwd_runs (csrc/hash_fwd_runs.h) takes the levels with res <= 300 - one thread per
eight consecutive samples, a cell's eight corners gathered once per run of samples that share it - and k_hash_fwd_x2 the others.  Every GPU case runs under both.

GPU part: fp32 output against the CPU oracle O.hash_encode_fwd, bit for bit (same table entries, same weights, the eight terms in the reference's order: no tolerance), both
output layouts, level tables of aabb_scale 1, 4 and 64 (10, 8 and 5 run levels; dense and hashed ones among them), on the smallest inputs that reach every path of the
kernel: sizes ragged against the 8-sample window and the 512-sample workgroup, a device-side count below n, hand-built run shapes, lattice and box edges, strided and
unaligned positions (the per-sample loads), two calls on one input.
CPU part: the kernel uses no scratch (device-only compile through tools/kernel_resources.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = [1, 4, 64]
SENTINEL = 0xDEADBEEF


def test_hash_fwd_runs_kernel_uses_no_scratch():
    """k_hash_fwd_runs<float, AOS | SOA>: ScratchSize == 0 (its 64 gathered pairs, 24 position words and 16 results are meant to live in registers: ~210-250 VGPRs)."""
    import shutil
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not installed")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), os.path.join(ROOT, "jnerf_amd", "csrc", "hash_encode.hip"), "k_hash_fwd_runs"],
                         capture_output=True, text=True, timeout=600).stdout
    rows = [l.split() for l in out.splitlines() if "k_hash_fwd_runs<float" in l]
    print(out)
    assert len(rows) == 2, out
    for r in rows:
        assert r[-2] == "0", r          # columns: ... occ scratch LDS


# ---------------------------------------------------------------------------------------------------------------- GPU: bit for bit against the oracle
def _rays(n, seed=11):
    """the generator of tools/microbench_hash.py: rays of 64 consecutive steps of 1/1024 from origins in [0.25, 0.75]^3, clamped to the unit cube - runs of 1-40 samples per
    cell on the run levels"""
    rng = np.random.default_rng(seed)
    n_rays = (n + 63) // 64
    o = (rng.random((n_rays, 1, 3), dtype=np.float32) * np.float32(0.5) + np.float32(0.25))
    d = rng.normal(size=(n_rays, 1, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    t = (np.arange(64, dtype=np.float32) * np.float32(1.0 / 1024))[None, :, None]
    return np.clip(o + d * t, 0, 1).astype(np.float32).reshape(-1, 3)[:n].copy()


class _Case:
    """one level table with its fp32 grid on the device; the oracle's output of the shared 8209-sample ray batch is computed once"""
    def __init__(self, aabb_scale):
        import torch
        from oracle import oracle as O
        import synth
        self.O = O
        self.table, _, self.n_params = O.level_table(aabb_scale)
        self.grid = synth.table(self.n_params, np.float32, amp=2.0)
        self.grid_t = torch.from_numpy(self.grid).cuda()
        self.x = _rays(8209)
        self.ref = O.hash_encode_fwd(self.x, self.grid, self.table)
        self.ref.setflags(write=False)

    def oracle(self, x):
        return self.O.hash_encode_fwd(np.ascontiguousarray(x, np.float32), self.grid, self.table)

    def run(self, x_t, layout, n_valid=None, out=None):
        """-> [n, 32] float32 rows whatever the layout"""
        from jnerf_amd import ops
        y = ops.hash_encode_fwd(x_t, self.grid_t, self.table, out=out, layout=layout, n_valid=n_valid)
        y = y.detach().cpu().numpy()
        return y if layout == ops.LAYOUT_AOS else np.ascontiguousarray(y.transpose(1, 0, 2)).reshape(-1, 32)

    def check(self, x, ref=None, what=""):
        import torch
        from jnerf_amd import ops
        ref = self.oracle(x) if ref is None else ref
        x_t = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
        for layout in (ops.LAYOUT_AOS, ops.LAYOUT_SOA):
            out = self.run(x_t, layout)
            bad = np.flatnonzero((out.view(np.uint32) != ref.view(np.uint32)).any(axis=1))
            assert bad.size == 0, f"{what} layout {layout}: {bad.size} of {len(x)} rows differ, first {bad[:5]}"


_CASES = {}


@pytest.fixture(params=SCALES)
def case(request, routing):
    if request.param not in _CASES:                     # one oracle run per level table for the whole module, whatever the routing
        _CASES[request.param] = _Case(request.param)
    return _CASES[request.param]


@pytest.fixture(params=["x2_paired", "runs"])
def routing(request, monkeypatch):
    """both routings of the fp32 forward, in one process: the default (one k_hash_fwd_x2 launch, two XCDs sharing four levels: every (level, chunk) must still have exactly
    one workgroup, also where the chunk count is odd) and NGP_HASH_FWD_RUNS=1 (k_hash_fwd_runs on the run levels, k_hash_fwd_x2 on the others; read per call)"""
    monkeypatch.setenv("NGP_HASH_FWD_RUNS", "1" if request.param == "runs" else "0")
    return request.param


@pytest.mark.gpu
def test_run_levels_present(case):
    """the tables under test have run levels (res <= 300) and other levels, dense and hashed run levels among them at aabb_scale 1 and 4"""
    res = case.table[:, 2]
    assert 0 < int((res <= 300).sum()) < 16


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 7, 8, 9, 2047, 2048, 2049, 8209])
def test_ragged_sizes(case, n):
    case.check(case.x[:n], case.ref[:n], f"n={n}")


@pytest.mark.gpu
@pytest.mark.parametrize("nv", [0, 5, 1003])
def test_device_side_count_below_n(case, nv):
    """rows at or beyond min(n, *n_valid) keep the sentinel the output was filled with, bit for bit"""
    import torch
    from jnerf_amd import ops
    n = 2048                                             # even: the SOA layout stores whole windows as 64-byte blocks
    x_t = torch.from_numpy(case.x[:n]).cuda()
    cnt = torch.tensor([nv], dtype=torch.int32, device="cuda")
    for layout in (ops.LAYOUT_AOS, ops.LAYOUT_SOA):
        shape = (n, 32) if layout == ops.LAYOUT_AOS else (16, n, 2)
        out = torch.from_numpy(np.full(shape, SENTINEL, np.uint32).view(np.float32)).cuda()
        got = case.run(x_t, layout, n_valid=cnt, out=out).view(np.uint32)
        assert np.array_equal(got[:nv], case.ref[:nv].view(np.uint32)), (layout, nv)
        assert (got[nv:] == SENTINEL).all(), (layout, nv, int((got[nv:] != SENTINEL).sum()))


@pytest.mark.gpu
def test_run_shapes(case):
    import synth
    one = np.repeat(np.array([[0.37, 0.61, 0.23]], np.float32), 4099, axis=0)         # one run across windows and workgroups
    case.check(one, what="one position")
    case.check(synth.uniform_positions(2051, seed=7), what="every sample its own cell")
    ab = np.empty((2051, 3), np.float32)
    ab[0::2] = [0.30, 0.40, 0.50]; ab[1::2] = [0.80, 0.15, 0.65]                      # cells alternating A, B, A, B: every sample opens a run
    case.check(ab, what="alternating cells")
    # (runs of 1-40 samples along straight rays: the shared batch of test_ragged_sizes)


@pytest.mark.gpu
def test_lattice_and_box_edges(case):
    """0, 1, exact cell boundaries of several levels (and their float neighbours), and the +1 corner at 1.0 - the dense levels' wrap in grid_index"""
    pts = [[0, 0, 0], [1, 1, 1], [1, 0, 0.5], [0, 1, 1], [1, 1, 0], [0.5, 1, 0.5], [0.5, 0.5, 0.5], [1, 0.25, 1]]
    for l in (0, 1, 4, 7, 9, 12, 15):
        scale = float(case.table[l, 3:4].view(np.float32)[0])
        res = int(case.table[l, 2])
        for g in (1, 2, res // 2, res - 2, res - 1):
            b = np.float32((g - 0.5) / scale)                                          # p = b * scale + 0.5 lands on (or one ulp beside) the lattice plane g
            for v in (np.nextafter(b, np.float32(0)), b, np.nextafter(b, np.float32(1))):
                if 0 <= v <= 1:
                    pts += [[v, v, v], [v, 0.5, 0.25], [0.75, v, 1.0], [1.0, 0.1, v]]
    x = np.array(pts, np.float32)
    x = np.concatenate([x, np.repeat(x, 3, axis=0)])                                    # each alone, then as runs of three
    case.check(x, what="edges")


@pytest.mark.gpu
def test_position_layouts(case):
    """row stride 4 and 7, and a base pointer that is 4-byte but not 16-byte aligned: the per-sample loads give the bits of the 16-byte ones"""
    import torch
    from jnerf_amd import ops
    n = 2049
    x, ref = case.x[:n], case.ref[:n]
    views = []
    for stride, first in ((4, 0), (7, 2)):
        buf = torch.full((n, stride), float("nan"), device="cuda")
        buf[:, first:first + 3] = torch.from_numpy(x).cuda()
        views.append((f"stride {stride}", buf[:, first:first + 3]))
    flat = torch.full((3 * n + 1,), float("nan"), device="cuda")
    flat[1:] = torch.from_numpy(x).cuda().reshape(-1)
    v = flat[1:].view(n, 3)
    assert v.data_ptr() % 16 == 4
    views.append(("unaligned base", v))
    for what, x_t in views:
        for layout in (ops.LAYOUT_AOS, ops.LAYOUT_SOA):
            assert np.array_equal(case.run(x_t, layout).view(np.uint32), ref.view(np.uint32)), (what, layout)


@pytest.mark.gpu
def test_two_calls_give_equal_bits(case):
    import torch
    from jnerf_amd import ops
    x_t = torch.from_numpy(case.x).cuda()
    for layout in (ops.LAYOUT_AOS, ops.LAYOUT_SOA):
        a, b = case.run(x_t, layout), case.run(x_t, layout)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), layout
