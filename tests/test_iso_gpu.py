"""csrc/iso_surface.hip (ngp_iso_count / ngp_iso_emit) against its oracle, the host function jnerf_amd/utils/isosurface.py::marching_tetrahedra on the same float32 array:
same vertices in the same order (to 1e-9 lattice units: the device interpolates every edge from its lower end, the host from whichever end it met first - a few float64
roundings at magnitude <= 128, < 1e-13), the same set of index triples, the same orientation of every triangle that has an area; then the opt-in wiring of the NeuS and
NGP mesh paths.  Every call into the library goes through ops.check (a non-zero return code raises)."""
import functools
import os
import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu]

ATOL = 1e-9
AREA = 1e-9           # |cross| below which a host triangle counts as degenerate (an edge collapsed by a value exactly on the threshold)


def _four_spheres(n):
    """-(signed distance) to the union of the four spheres of dataset.synthetic_field on the lattice linspace(0, 1, n)^3: > 0 inside"""
    ax = np.linspace(0.0, 1.0, n)
    p = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3) - 0.5
    centres = np.array([[0.0, 0.0, 0.0], [0.18, 0.1, -0.05], [-0.15, 0.12, 0.1], [0.02, -0.2, 0.12]])
    radii = np.array([0.16, 0.09, 0.08, 0.07])
    return (-np.min(np.linalg.norm(p[:, None, :] - centres[None], axis=-1) - radii[None], axis=-1)).reshape(n, n, n).astype(np.float32)


def _sinusoids(shape):
    x, y, z = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij")
    return (np.sin(0.07 * x + 0.3) + np.sin(0.05 * y + 1.1) + np.sin(0.09 * z + 2.0) + 0.1).astype(np.float32)


def _integers():
    return np.random.default_rng(7).integers(0, 3, (12, 12, 12)).astype(np.int32)


# name -> (lattice, threshold); the kernels' tile is 1024 lattice points (csrc/iso_surface.hip: ISO_TILE)
CASES = {
    "random_2x2x2": lambda: (np.random.default_rng(1).uniform(-1, 1, (2, 2, 2)).astype(np.float32), 0.0),
    "random_3x2x5": lambda: (np.random.default_rng(2).uniform(-1, 1, (3, 2, 5)).astype(np.float32), 0.25),
    "random_9x7x5": lambda: (np.random.default_rng(3).uniform(-1, 1, (9, 7, 5)).astype(np.float32), 0.0),
    "random_17x16x33": lambda: (np.random.default_rng(4).uniform(-1, 1, (17, 16, 33)).astype(np.float32), 0.25),
    "occupancy": lambda: (_integers(), 0.5),
    "occupancy_on_threshold": lambda: (_integers(), 1.0),
    "halves_on_threshold": lambda: ((np.random.default_rng(8).integers(-2, 3, (10, 9, 8)) * 0.5).astype(np.float32), 0.0),
    "smooth_540_tiles": lambda: (_sinusoids((96, 80, 72)), 0.0),
    # 1105 tiles: the one workgroup that scans the tile totals takes 1024 per round, so this is the smallest kind of shape on which it carries a sum into a second round
    "smooth_1105_tiles": lambda: (_sinusoids((112, 100, 101)), 0.0),
    "four_spheres_33": lambda: (_four_spheres(33), 0.0),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(lattice, threshold, host vertices, host triangles), computed once and shared read-only"""
    from jnerf_amd.utils.isosurface import marching_tetrahedra
    u, thr = CASES[name]()
    hv, ht = marching_tetrahedra(u, thr)
    for a in (u, hv, ht):
        a.setflags(write=False)
    return u, thr, hv, ht


def _device(u, thr):
    from jnerf_amd.utils.isosurface import marching_tetrahedra_device
    v, t = marching_tetrahedra_device(torch.tensor(u, device="cuda"), thr)
    assert v.is_cuda and t.is_cuda and v.dtype == torch.float64 and t.dtype == torch.int32 and v.shape[1:] == (3,) and t.shape[1:] == (3,)
    return v.cpu().numpy(), t.cpu().numpy().astype(np.int64)


def _canonical(t):
    """every triple rotated so that its smallest index leads (orientation kept), rows sorted by (unordered triple, rotation)"""
    t = np.asarray(t, dtype=np.int64)
    k = np.argmin(t, 1)
    rot = np.stack([np.take_along_axis(t, ((k + j) % 3)[:, None], 1)[:, 0] for j in range(3)], 1)
    unordered = np.sort(t, 1)
    order = np.lexsort((rot[:, 2], rot[:, 1], unordered[:, 2], unordered[:, 1], unordered[:, 0]))
    return unordered[order], rot[order], order


def _assert_same_surface(name, min_with_area=None):
    """min_with_area None: every triangle must have the host's orientation; else at least that share of the host's triangles has an area, and those must"""
    u, thr, hv, ht = _case(name)
    dv, dt = _device(u, thr)
    print(f"{name}: host {len(hv)} vertices / {len(ht)} triangles, device {len(dv)} / {len(dt)}")
    assert len(dv) == len(hv)
    print(f"  largest vertex difference {np.abs(dv - hv).max() if len(hv) else 0.0:.3e}")
    np.testing.assert_allclose(dv, hv, rtol=0, atol=ATOL)
    assert len(dt) == len(ht)
    hs, hr, ho = _canonical(ht)
    ds, dr, _ = _canonical(dt)
    assert (hs == ds).all(), "the multisets of unordered index triples differ"
    tri = hv[np.asarray(ht)[ho]]
    has_area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1) >= AREA
    same = (hr == dr).all(1)
    print(f"  triangles with an area: {has_area.mean():.3f}; orientation equal on {same.mean():.3f} of all, differing on {int((~same & has_area).sum())} with an area")
    if min_with_area is None:
        assert same.all()
    else:
        assert has_area.mean() >= min_with_area
        assert same[has_area].all()
    return dv, dt


@pytest.mark.parametrize("name", ["random_2x2x2", "random_3x2x5", "random_9x7x5", "random_17x16x33"])
def test_random_lattices(name):
    """every cube is mixed: all 16 cases of a tetrahedron occur in bulk; none of the host's triangles is degenerate"""
    _assert_same_surface(name)


def test_integer_occupancy():
    """the NGP path's lattice: int32 values in {0, 1, 2}, threshold 0.5"""
    _assert_same_surface("occupancy")


@pytest.mark.parametrize("name", ["occupancy_on_threshold", "halves_on_threshold"])
def test_values_exactly_on_the_threshold(name):
    """a value equal to the threshold is below and collapses its edges onto the lattice point: 25 - 32 % of the host's triangles have no area here (the host alone keeps
    68 % / 75 %) and their orientation is not defined; all the others must agree"""
    _assert_same_surface(name, min_with_area=0.6)


@pytest.mark.parametrize("name", ["smooth_540_tiles", "smooth_1105_tiles"])
def test_more_than_one_tile_in_every_pass(name):
    _assert_same_surface(name)


def test_closed_surface():
    u, thr, hv, ht = _case("four_spheres_33")
    dv, dt = _device(u, thr)
    assert len(dt) > 100
    nv = len(dv)
    directed = np.concatenate([dt[:, [0, 1]], dt[:, [1, 2]], dt[:, [2, 0]]])
    key = directed[:, 0] * nv + directed[:, 1]
    uniq, cnt = np.unique(key, return_counts=True)
    assert (cnt == 1).all(), "a directed edge occurs twice"
    assert np.array_equal(uniq, np.unique(directed[:, 1] * nv + directed[:, 0])), "a directed edge without its reverse"

    def volume(v, t):
        a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
        return float((a * np.cross(b, c)).sum() / 6.0)

    vol_d, vol_h = volume(dv, dt), volume(hv, np.asarray(ht))
    print(f"signed volume: device {vol_d!r}, host {vol_h!r} (lattice units^3)")
    assert vol_d > 0
    assert abs(vol_d - vol_h) <= 1e-9 * abs(vol_h)


def test_two_calls_give_identical_bytes():
    from jnerf_amd import ops
    u_np, thr, hv, ht = _case("smooth_540_tiles")
    u = torch.tensor(u_np, device="cuda")
    results = []
    for poison in (0xFF, 0x5A):
        ws = torch.full((ops.iso_workspace_bytes(u.shape),), poison, dtype=torch.uint8, device="cuda")
        nv, nt = ops.iso_count(u, thr, ws).tolist()
        assert (nv, nt) == (len(hv), len(ht))
        v = torch.full((nv * 24,), poison, dtype=torch.uint8, device="cuda").view(torch.float64).view(nv, 3)
        t = torch.full((nt * 12,), poison, dtype=torch.uint8, device="cuda").view(torch.int32).view(nt, 3)
        ops.iso_emit(u, thr, ws, nv, nt, vertices=v, triangles=t)
        results.append((v.cpu().numpy().tobytes(), t.cpu().numpy().tobytes()))
    assert results[0][0] == results[1][0] and results[0][1] == results[1][1]


def test_no_surface():
    from jnerf_amd.utils.isosurface import marching_tetrahedra_device
    v, t = marching_tetrahedra_device(torch.ones((5, 5, 5), device="cuda"), 0.0)
    assert v.shape == (0, 3) and v.dtype == torch.float64 and t.shape == (0, 3) and t.dtype == torch.int32
    v, t = marching_tetrahedra_device(torch.ones((5, 1, 5), device="cuda"), 2.0)
    assert v.shape == (0, 3) and v.dtype == torch.float64 and t.shape == (0, 3) and t.dtype == torch.int32


def test_neus_extract_geometry_on_the_device():
    from jnerf_amd.neus_renderer import extract_geometry
    bound_min = torch.tensor([-1.0, -1.0, -1.0], device="cuda")
    bound_max = torch.tensor([1.0, 1.0, 1.0], device="cuda")
    sphere = lambda pts: 0.6 - torch.linalg.norm(pts - torch.tensor([0.05, -0.02, 0.03], device=pts.device), dim=-1)
    hv, ht = extract_geometry(bound_min, bound_max, 48, 0.0, sphere)
    dv, dt = extract_geometry(bound_min, bound_max, 48, 0.0, sphere, device=True)
    assert len(ht) > 1000 and dv.shape == hv.shape and dt.shape == ht.shape
    print(f"NeuS wiring: {len(hv)} vertices, {len(ht)} triangles, largest vertex difference {np.abs(dv - hv).max():.3e}")
    np.testing.assert_allclose(dv, hv, rtol=0, atol=1e-6)
    assert (_canonical(ht)[0] == _canonical(dt)[0]).all()


def test_ngp_extract_mesh_on_the_device(tmp_path):
    from jnerf_amd.presets import ngp_cfg
    from jnerf_amd.runner import Runner
    from jnerf_amd.mesh import extract_mesh
    from jnerf_amd.utils.isosurface import read_ply
    torch.manual_seed(0)
    ngp_cfg(n_images=8, W=96, H=96, target_batch_size=1 << 16, n_rays_per_batch=1024, fp16=False, aabb_scale=1, const_dt=True, log_dir=str(tmp_path))
    r = Runner()
    for i in range(400):
        r.train_step(i)
    r.drain()
    out = {}
    for iso in ("device", "host"):
        os.makedirs(tmp_path / iso)
        out[iso] = extract_mesh(r, resolution=64, save_dir=str(tmp_path / iso), log=lambda *a: None, iso=iso)
    (dv, dt, _), (hv, ht, _) = out["device"], out["host"]
    print(f"NGP wiring: host {len(hv)} vertices / {len(ht)} triangles, device {len(dv)} / {len(dt)}")
    assert len(ht) > 100 and dv.shape == hv.shape and dt.shape == ht.shape
    np.testing.assert_allclose(dv, hv, rtol=0, atol=2e-7)
    assert (_canonical(ht)[1] == _canonical(dt)[1]).all()
    for iso in ("device", "host"):
        cv, ct, cc = read_ply(os.path.join(tmp_path, iso, "mesh-color.ply"))
        assert len(cv) == len(hv) and len(ct) == len(ht) and cc is not None and cc.shape == (len(hv), 3)
