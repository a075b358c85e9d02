"""Sweep of k_hash_fwd_x2's chunks in flight (NGP_HASH_FWD_CHUNKS, read by the library per call) on the captured position sets of tools/probe_hash_fwd_levels.py: the
training batch, the refresh set, and the refresh set as the first rows of a 4 M-row buffer with a device-side count (the shape of the inference buffers).  One process, one
library; min / median of --reps launches per value, us.
usage: python tools/probe_hash_fwd_chunks.py --positions FILE.npz [--chunks 256,512,1024,2048,4096] [--reps 50]      (FILE: written by probe_hash_fwd_levels.py --positions)"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jnerf_amd import ops
from probe_hash_fwd_levels import time_us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", required=True)
    ap.add_argument("--chunks", default="256,512,1024,2048,4096")
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    z = np.load(args.positions)
    train, refresh, table = z["train"], z["refresh"], z["table"]
    grid = (torch.rand(int(table[:, 1].sum()) * 2, device="cuda") - 0.5) * 2e-4
    big = torch.zeros((1 << 22, 3), device="cuda")
    big[:refresh.shape[0]] = torch.from_numpy(refresh).cuda()
    count = torch.tensor([refresh.shape[0]], dtype=torch.int32, device="cuda")
    sets = [("training batch", torch.from_numpy(train).cuda(), None), ("refresh set", torch.from_numpy(refresh).cuda(), None), ("4 M rows, count = refresh set", big, count)]
    outs = [torch.empty((16, x.shape[0], 2), device="cuda") for _, x, _ in sets]
    print(f"# NGP_HASH_FWD_MAP={os.environ.get('NGP_HASH_FWD_MAP', '(default)')}; min / median of {args.reps}, us")
    print("| chunks in flight | " + " | ".join(f"{name} ({x.shape[0]})" for name, x, _ in sets) + " |")
    print("|---|" + "---|" * len(sets))
    for c in ["(default)"] + args.chunks.split(","):
        if c == "(default)":
            os.environ.pop("NGP_HASH_FWD_CHUNKS", None)
        else:
            os.environ["NGP_HASH_FWD_CHUNKS"] = c
        cells = []
        for (name, x, nv), out in zip(sets, outs):
            lo, med = time_us(lambda: ops.hash_encode_fwd(x, grid, table, out=out, layout=ops.LAYOUT_SOA, n_valid=nv), args.reps)
            cells.append(f"{lo:.1f} / {med:.1f}")
        print(f"| {c} | " + " | ".join(cells) + " |", flush=True)


if __name__ == "__main__":
    main()
