"""Where the hash forward's time goes, level by level (GPU; no bench run needed).  Times ngp_hash_encode_fwd (fp32 table, SOA output - the training call) on
  * the positions of a real training batch: the bench workload's runner after a burn-in, runner.sampler._pos_train up to its device-side count;
  * one occupancy refresh's Morton-ordered sample set (the two grid_generate_samples calls of DensityGridSampler.update_density_grid_nerf past step 256),
once with the real level table and once per level with a table whose sixteen rows are all THAT level's row: the launch then does sixteen levels' worth of that level's
work on all eight XCDs, and a sixteenth of its time is the level's cost at full machine width (every XCD holds the same table slice, so the L2 side is if anything
kinder than in the real launch, where an XCD serves two levels).
The routing is the library's: NGP_HASH_FWD_RUNS=1 sends the run levels (res <= 300) to k_hash_fwd_runs, NGP_HASH_FWD_MAP=0 | 1 picks k_hash_fwd_x2's level-to-XCD map
(the per-level rows mean what they say under NGP_HASH_FWD_MAP=0 and under NGP_HASH_FWD_RUNS=1: sixteen copies of a level keep every XCD equally busy there).
usage: python tools/probe_hash_fwd_levels.py [--positions FILE.npz] [--burn-in 320] [--reps 30]     (FILE: written if missing, read if present - the same batch for both modes)"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jnerf_amd import ops


def capture(burn_in):
    """-> (training-batch positions [n,3], refresh positions [m,3], level table) of the bench workload (lego configuration: fp32 table, aabb_scale 1, scene bricks)"""
    from jnerf_amd.presets import ngp_cfg
    from jnerf_amd.runner import Runner
    torch.manual_seed(1234)
    ngp_cfg(scene="bricks", fp16=False, aabb_scale=1, const_dt=True, n_images=100, W=800, H=800, device="cuda:0", rank=0, world_size=1, target_batch_size=1 << 18, n_rays_per_batch=4096)
    runner = Runner()
    with runner.training_stream():
        for step in range(burn_in):
            runner.train_step(step)
        torch.cuda.synchronize()
        s = runner.sampler
        n = int(s._counters[3].item())
        train = s._pos_train[:n].clone()
        # one refresh's sample set, as update_density_grid_nerf generates it past step 256 (on a copy of the generator state: the runner is not used again)
        G3, nc = s.NERF_GRIDSIZE ** 3, s.max_cascade + 1
        n_u = n_n = G3 * nc // 4
        pos = torch.empty((n_u + n_n, 3), dtype=torch.float32, device="cuda")
        idx = torch.empty(n_u + n_n, dtype=torch.int32, device="cuda")
        rng = s.rng_state.copy()
        mo = s.cfg.grid_samples_morton_order is not False
        ops.grid_generate_samples(n_u, rng, s.density_grid_ema_step, s.aabb_range, s.density_grid, nc, -0.01, pos=pos[:n_u], idx=idx[:n_u], morton_order=mo)
        ops.grid_generate_samples(n_n, rng, s.density_grid_ema_step, s.aabb_range, s.density_grid, nc, s.NERF_MIN_OPTICAL_THICKNESS, pos=pos[n_u:], idx=idx[n_u:], morton_order=mo)
        torch.cuda.synchronize()
        table = np.array(runner.model.pos_encoder.level_table, np.uint32).reshape(16, 4)
    runner.finish()
    return train.cpu().numpy(), pos.cpu().numpy(), table


def time_us(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[0], ts[len(ts) // 2]


def runs_per_window(x, scale):
    """average number of cell runs per 8-sample window of a level (what k_hash_fwd_runs gathers), and per 8 samples without the window boundaries"""
    c = np.floor(x * np.float32(scale) + np.float32(0.5)).astype(np.int64)
    change = np.ones(len(c), bool)
    change[1:] = (c[1:] != c[:-1]).any(axis=1)
    free = change.sum() * 8.0 / len(c)
    change[::8] = True
    return change.sum() * 8.0 / len(c), free


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", default="")
    ap.add_argument("--burn-in", type=int, default=320)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--no-levels", action="store_true", help="the real table only")
    args = ap.parse_args()
    if args.positions and os.path.isfile(args.positions):
        z = np.load(args.positions)
        train, refresh, table = z["train"], z["refresh"], z["table"]
    else:
        train, refresh, table = capture(args.burn_in)
        if args.positions:
            np.savez(args.positions, train=train, refresh=refresh, table=table)
    n_params = int(table[:, 1].sum()) * 2
    grid = (torch.rand(n_params, device="cuda") - 0.5) * 2e-4
    print(f"# NGP_HASH_FWD_RUNS={os.environ.get('NGP_HASH_FWD_RUNS', '(default)')} NGP_HASH_FWD_MAP={os.environ.get('NGP_HASH_FWD_MAP', '(default)')}; run levels (res <= 300): {int((table[:, 2] <= 300).sum())} of 16")
    for name, x in (("training batch", train), ("refresh set", refresh)):
        x_t = torch.from_numpy(x).cuda()
        n = x_t.shape[0]
        out = torch.empty((16, n, 2), device="cuda")
        lo, med = time_us(lambda: ops.hash_encode_fwd(x_t, grid, table, out=out, layout=ops.LAYOUT_SOA), args.reps)
        print(f"\n## {name}: {n} positions; the real table, one call: min {lo:.1f} us, median {med:.1f} us")
        if args.no_levels:
            continue
        print("| level | res | entries | kind | us per level (min) | (median) | runs per 8-sample window | without window cuts |")
        print("|---|---|---|---|---|---|---|---|")
        tot = {"run": 0.0, "other": 0.0}
        for l in range(16):
            t1 = np.tile(table[l], (16, 1))
            lo, med = time_us(lambda: ops.hash_encode_fwd(x_t, grid, t1, out=out, layout=ops.LAYOUT_SOA), args.reps)
            kind = "run" if table[l, 2] <= 300 else "other"
            tot[kind] += lo / 16
            rw, rf = runs_per_window(x, table[l, 3:4].view(np.float32)[0]) if kind == "run" else (float("nan"), float("nan"))
            print(f"| {l} | {table[l, 2]} | {table[l, 1]} | {kind} | {lo / 16:.2f} | {med / 16:.2f} | {rw:.2f} | {rf:.2f} |")
        s = tot["run"] + tot["other"]
        print(f"sum of the per-level minima: {s:.1f} us; run levels {tot['run']:.1f} us = {tot['run'] / max(s, 1e-9):.0%}, other levels {tot['other']:.1f} us")


if __name__ == "__main__":
    main()
