"""Hashes of the field kernels' outputs (fp16 and split-fp32; forward, density, backward; both layouts) and of the hash backward's table gradient (both workspace
paths) on fixed inputs - run once per library file by tools/ab_prebuilt.sh to show whether a new build returns the same BITS as an earlier commit's
(profiles/r06s_lib_bits.txt, profiles/r08_hash_bwd_refactor.md)."""
import hashlib, os, sys
import numpy as np, torch
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
from jnerf_amd import ops
import synth
from test_hash_bwd_stage import _ray_batch

h = lambda t: hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()[:16]
for n in (8192 + 17, 1 << 18):
    rng = np.random.default_rng(10)
    feat = rng.normal(size=(n, 32)) * 0.5
    d = synth.unit_dirs01(n, seed=11)
    wd, wc = synth.mlp_weights(12)
    dout = np.random.default_rng(20).normal(size=(n, 4)) * 1e-2
    T = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a.astype(dt))).cuda()
    for name, fwd, den, bwd, dt in (("fp16", ops.field_fwd, ops.density_fwd, ops.field_bwd, np.float16), ("fp32", ops.field32_fwd, ops.density32_fwd, ops.field32_bwd, np.float32)):
        for layout in (ops.LAYOUT_AOS, ops.LAYOUT_SOA):
            f = feat if layout == ops.LAYOUT_AOS else feat.reshape(n, 16, 2).transpose(1, 0, 2)
            out = fwd(T(f, dt), T(d, np.float32), T(wd, dt), T(wc, dt), layout=layout)
            dn = den(T(f, dt), T(wd, dt), n, layout=layout)
            dfeat, slabs = bwd(T(f, dt), T(d, np.float32), T(wd, dt), T(wc, dt), T(dout, dt), layout=layout)
            torch.cuda.synchronize()
            print("bits", n, name, layout, h(out), h(dn), h(dfeat), h(slabs), "%.6e" % float(slabs.double().abs().sum()), flush=True)

# hash backward with a workspace, ray-coherent positions: fp32 dL/dy (record regions, aabb_scale 1) in both layouts, overwriting and accumulating into a non-zero gradient;
# fp16 dL/dy (per-corner lists, aabb_scale 4) into an fp32 and an fp16 gradient
for n in (4099, 1 << 18):
    g = np.random.default_rng(7).standard_normal((n, 32)) * 1e-3
    for name, dt, gdts, aabb in (("fp32", torch.float32, (torch.float32,), 1), ("fp16", torch.float16, (torch.float32, torch.float16), 4)):
        table, _, n_params = ops.level_table(aabb)
        pos = torch.from_numpy(_ray_batch(n, seed=11 + aabb)).cuda()
        seed = torch.from_numpy(np.random.default_rng(3).standard_normal(n_params) * 1e-4).cuda()
        for gdt in gdts:
            ws = torch.empty(ops.hash_bwd_workspace_bytes(table, n, dt, gdt), dtype=torch.uint8, device="cuda")
            for layout in (ops.LAYOUT_AOS, ops.LAYOUT_SOA):
                dl = torch.from_numpy(g).cuda().to(dt)
                dl = dl.contiguous() if layout == ops.LAYOUT_AOS else dl.view(n, 16, 2).permute(1, 0, 2).contiguous()
                over = ops.hash_encode_bwd(pos, dl, table, n_params, grad=torch.full((n_params,), float("nan"), dtype=gdt, device="cuda"), layout=layout, zero_first=True, workspace=ws)
                acc = ops.hash_encode_bwd(pos, dl, table, n_params, grad=seed.to(gdt), layout=layout, zero_first=False, workspace=ws)
                torch.cuda.synchronize()
                print("bits hash_bwd", n, name, str(gdt).split(".")[1], layout, h(over), h(acc), "%.6e" % float(over.double().abs().sum()), flush=True)
