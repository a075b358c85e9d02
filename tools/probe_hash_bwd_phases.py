"""Where a workgroup of k_bin_runs2 and of k_bin_accumulate2 spends its life inside the fp32 training step (profiles/r07_hash_bwd_stage.md).

Needs the timing build of the library:   EXTRA=-DNGP_PROBE_CLOCK bash jnerf_amd/csrc/build.sh
(thread 0 of every workgroup stamps the 100 MHz wall clock at its phase boundaries; results are unchanged, the stamps cost a few stores).  Trains the bench
workload (bench.py's lego configuration and scene) for `steps` iterations and reads the stamps of the LAST step.
usage: python tools/probe_hash_bwd_phases.py [steps]      (NGP_HASH_BWD_RUNS=0 selects the previous form of k_bin_runs2)"""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jnerf_amd import _lib
from jnerf_amd.presets import ngp_cfg
from jnerf_amd.runner import Runner

RUNS_PHASES = ["tail rider at the head (V2: even workgroups only)", "loads + cells", "count sweep", "prefix", "emit sweep", "staged write-out"]
ACC_PHASES = ["tables + zeroing", "record gather", "barrier wait of thread 0", "sweep / store"]


def table(name, st, phases):
    """st: [workgroups, slots] stamps in 10 ns ticks, 0 = not stamped"""
    n_slots = len(phases) + 1
    live = st[(st[:, :n_slots] != 0).all(axis=1)][:, :n_slots].astype(np.int64)
    if not len(live):
        print(name, ": no workgroup stamped every phase"); return
    t0 = live[:, 0].min()
    d = np.diff(live, axis=1) * 0.01                              # us
    print(f"{name}: {len(live)} workgroups, first start -> last end {(live[:, -1].max() - t0) * 0.01:.1f} us, a workgroup's life median {np.median((live[:, -1] - live[:, 0]) * 0.01):.1f} us "
          f"(p10 {np.percentile((live[:, -1] - live[:, 0]) * 0.01, 10):.1f}, p90 {np.percentile((live[:, -1] - live[:, 0]) * 0.01, 90):.1f}); starts spread over {(live[:, 0].max() - t0) * 0.01:.1f} us")
    print(f"| phase | median us | p10 | p90 | share of the median life |")
    print("|---|---|---|---|---|")
    life = np.median((live[:, -1] - live[:, 0]) * 0.01)
    for i, p in enumerate(phases):
        print(f"| {p} | {np.median(d[:, i]):.2f} | {np.percentile(d[:, i], 10):.2f} | {np.percentile(d[:, i], 90):.2f} | {np.median(d[:, i]) / max(life, 1e-9):.0%} |")


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 320
    lib = _lib.lib()
    if not hasattr(lib, "ngp_x_probe_clock"):
        sys.exit("this library is not the -DNGP_PROBE_CLOCK build")
    lib.ngp_x_probe_clock.restype, lib.ngp_x_probe_clock.argtypes = C.c_int, [C.c_void_p, C.c_int]
    torch.manual_seed(1234)
    ngp_cfg(scene="bricks", fp16=False, aabb_scale=1, const_dt=True, n_images=100, W=800, H=800, device="cuda:0", target_batch_size=1 << 18, n_rays_per_batch=4096)
    r = Runner()
    with r.training_stream():
        for i in range(steps):
            r.train_step(i)
        r.drain()
    torch.cuda.synchronize()
    out = np.zeros((2, 4096, 8), np.uint64)
    rc = lib.ngp_x_probe_clock(out.ctypes.data_as(C.c_void_p), 0)
    assert rc == 0, rc
    print("form:", "previous" if os.environ.get("NGP_HASH_BWD_RUNS") == "0" else "V2", "| steps", steps)
    table("k_bin_runs2", out[0], RUNS_PHASES)
    last = out[0][out[0][:, 7] != 0].astype(np.int64)
    if len(last):
        print(f"k_bin_runs2: {len(last)} workgroups carried their tail unit at the end: median {np.median((last[:, 7] - last[:, 6]) * 0.01):.2f} us; "
              f"the launch, first start -> last stamp {(max(last[:, 7].max(), out[0][:, 6].max()) - out[0][:, 0][out[0][:, 0] != 0].min()) * 0.01:.1f} us")
    acc = out[1]
    table("k_bin_accumulate2 (all units)", acc, ACC_PHASES)
    if "PROBE_DUMP" in os.environ:
        np.save(os.environ["PROBE_DUMP"], out)


if __name__ == "__main__":
    main()
