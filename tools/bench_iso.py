#!/usr/bin/env python
"""Iso-surface extraction, host path against device path, on the four-sphere signed field (negated, threshold 0) at 256^3 and 512^3:
    python tools/bench_iso.py [--sizes 256,512] [--device-reps 20] [--host-reps 3] [--out FILE]
prints ONE JSON line (and appends it to --out):
  host:    device -> host copy of the float32 lattice + utils/isosurface.py::marching_tetrahedra, host clock;
  device:  ngp_iso_count + read-back of the two counts + ngp_iso_emit + copy of vertices and triangles to the host, host clock around a final synchronise;
  kernels: per-kernel HIP-event times (ngp_prof_enable), taken in repetitions of their own (the event brackets are not inside the end-to-end figures);
  classify pass: achieved bytes/s over its algorithmic bytes - 4 B read per lattice point, 2 B written (edge mask, triangle count), 8 B per tile of 1024.
Every figure is the median over the repetitions after a warm-up, with the smallest and the largest beside it.  There is no CPU fall-back: without a GPU this fails."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_BYTES_PER_S = 8.0e12          # MI355X HBM3E, spec
KERNELS = ["k_iso_classify", "k_iso_scan_tiles", "k_iso_emit_vertices", "k_iso_emit_triangles"]


def four_spheres(n, device):
    """-(signed distance) to the union of the four spheres of dataset.synthetic_field on linspace(0, 1, n)^3 (tests/test_zz_mesh_gpu.py::_distance_to_scene without the abs)"""
    import torch
    ax = torch.linspace(0.0, 1.0, n, device=device, dtype=torch.float64) - 0.5
    centres = [[0.0, 0.0, 0.0], [0.18, 0.1, -0.05], [-0.15, 0.12, 0.1], [0.02, -0.2, 0.12]]
    radii = [0.16, 0.09, 0.08, 0.07]
    x, y, z = ax[:, None, None], ax[None, :, None], ax[None, None, :]
    sdf = None
    for (cx, cy, cz), r in zip(centres, radii):
        d = torch.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) - r
        sdf = d if sdf is None else torch.minimum(sdf, d)
    return (-sdf).to(torch.float32).contiguous()


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "reps": len(ms)}


def bench_size(n, device_reps, host_reps):
    import torch
    from jnerf_amd import ops
    from jnerf_amd.utils.isosurface import marching_tetrahedra, marching_tetrahedra_device
    u = four_spheres(n, "cuda")
    torch.cuda.synchronize()

    def device_path():
        v, t = marching_tetrahedra_device(u, 0.0)
        return v.cpu().numpy(), t.cpu().numpy()               # .cpu() synchronises

    def host_path():
        return marching_tetrahedra(u.cpu().numpy(), 0.0)

    for _ in range(3):                                         # warm-up: code objects, the cached workspace, the pinned staging of the copies
        dv, dt = device_path()
    device_ms = []
    for _ in range(device_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        device_path()
        device_ms.append((time.perf_counter() - t0) * 1e3)
    hv, ht = host_path()                                       # warm-up
    host_ms = []
    for _ in range(host_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_path()
        host_ms.append((time.perf_counter() - t0) * 1e3)
    if (len(hv), len(ht)) != (len(dv), len(dt)):
        raise RuntimeError(f"{n}^3: host {len(hv)} vertices / {len(ht)} triangles, device {len(dv)} / {len(dt)}")

    ops.prof_enable(KERNELS)                                   # per-kernel event brackets, in repetitions of their own
    ops.prof_read()
    for _ in range(device_reps):
        device_path()
    per_kernel = {k: stats(v) for k, v in ops.prof_read().items()}
    ops.prof_enable("")
    points = n ** 3
    classify_bytes = 4 * points + 2 * points + 8 * ((points + 1023) // 1024)
    rate = classify_bytes / (per_kernel["k_iso_classify"]["median_ms"] * 1e-3)
    return {"lattice": [n, n, n], "vertices": len(dv), "triangles": len(dt), "host_vertices": len(hv), "host_triangles": len(ht),
            "host": stats(host_ms), "device": stats(device_ms), "host_over_device": round(statistics.median(host_ms) / statistics.median(device_ms), 2),
            "kernels": per_kernel, "kernel_sum_median_ms": round(sum(k["median_ms"] for k in per_kernel.values()), 4),
            "classify": {"algorithmic_bytes": classify_bytes, "achieved_GBps": round(rate / 1e9, 1), "share_of_hbm_peak": round(rate / HBM_PEAK_BYTES_PER_S, 3)}}


def main():
    parser = argparse.ArgumentParser(description="host against device iso-surface extraction (libngp_hip, MI355X)")
    parser.add_argument("--sizes", default="256,512")
    parser.add_argument("--device-reps", type=int, default=20)
    parser.add_argument("--host-reps", type=int, default=3)
    parser.add_argument("--out", default="")
    args = parser.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_iso.py needs a GPU: there is nothing to measure without one")
    result = {"bench": "iso_surface", "field": "four spheres, -sdf, threshold 0", "corner_reads": "L1/L2 (no LDS halo tile)", "device": torch.cuda.get_device_name(0),
              "sizes": [bench_size(int(s), args.device_reps, args.host_reps) for s in args.sizes.split(",")]}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
