"""(r7) The hash-backward stage: k_bin_runs2 (run records) + k_bin_pairs + k_bin_accumulate2 of the fp32 step (csrc/hash_bwd_regions.h), k_bin_records_runs + k_bin_records +
k_bin_accumulate of the fp16 step (csrc/hash_bwd_percorner.h); both run-record kernels are built on the run-combining core of csrc/hash_bwd_common.h, and
csrc/hash_encode.hip is the translation unit that includes the three.

CPU part: none of the stage's kernels that the fp32 or the fp16 step launches may spill or use AGPRs (device-only compile, as tests/test_abi.py's field-kernel guard).
GPU part: the run-record kernel the step launches (its V2 form) against the form it replaced (NGP_HASH_BWD_RUNS=0), byte for byte - the accumulation is exact integer
arithmetic over records whose values are the same fp32 sums, so there is no tolerance."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hash_bwd_stage_kernels_do_not_spill():
    """k_bin_runs2 (the form the step launches: last template argument true), k_bin_pairs<float, ...> and k_bin_accumulate2<float, true | false>: ScratchSize == 0 and
    AGPRs == 0, both layouts.  The earlier form of k_bin_runs2 that NGP_HASH_BWD_RUNS=0 still selects for A/B runs (last argument false, 48-52 B of scratch per
    lane) is not launched by the step and is not held to this.  The fp16 step's kernels, which share the run-combining core, are held to the same:
    k_bin_records_runs<*, *, 4> (four instantiations), k_bin_records<*, *> (four) and k_bin_accumulate<*, *, *> (six)."""
    import shutil
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not installed")
    path = os.path.join(ROOT, "jnerf_amd", "csrc", "hash_encode.hip")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics", "-fvisibility=hidden",
           "--cuda-device-only", "-c", path, "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"]
    err = subprocess.run(cmd, capture_output=True, text=True, timeout=600).stderr
    rows, cur = [], None
    for line in err.splitlines():
        m = re.search(r"remark: (?:\S+ )?\s*(Function Name|AGPRs|ScratchSize \[bytes/lane\]): (\S+)", line)
        if m and m.group(1) == "Function Name":
            cur = {"name": m.group(2)}; rows.append(cur)
        elif m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    runs = [r for r in rows if re.match(r"_Z11k_bin_runs2IfLi[01]ELi\d+ELb1EE", r["name"])]
    pairs = [r for r in rows if r["name"].startswith("_Z11k_bin_pairsIf")]
    acc = [r for r in rows if r["name"].startswith("_Z17k_bin_accumulate2IfLb")]
    assert len(runs) == 2 and len(pairs) == 4 and len(acc) == 2, [r["name"] for r in rows]
    rec_runs = [r for r in rows if re.match(r"_Z18k_bin_records_runsI\w+Li[01]ELi4EE", r["name"])]
    rec = [r for r in rows if r["name"].startswith("_Z13k_bin_recordsI")]
    acc1 = [r for r in rows if r["name"].startswith("_Z16k_bin_accumulateI")]
    assert len(rec_runs) == 4 and len(rec) == 4 and len(acc1) == 6, [r["name"] for r in rows]
    for r in runs + pairs + acc + rec_runs + rec + acc1:
        print(r)
        assert r["ScratchSize [bytes/lane]"] == 0, r
        assert r["AGPRs"] == 0, r


# ---------------------------------------------------------------------------------------------------------------- GPU: V2 form == previous form, bit for bit
def _ray_batch(n, seed):
    """ray-coherent positions in the unit cube: rays through the cube, consecutive samples a constant step apart (what the marcher hands the backward)"""
    rng = np.random.default_rng(seed)
    per = 256
    n_rays = (n + per - 1) // per
    o = rng.uniform(0.05, 0.95, (n_rays, 3)).astype(np.float32)
    d = rng.normal(size=(n_rays, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    t = (np.arange(per, dtype=np.float32) * np.float32(np.sqrt(3.0) / 1024.0))[None, :, None]
    x = (o[:, None, :] + d[:, None, :] * t).reshape(-1, 3)[:n]
    return np.ascontiguousarray(np.clip(x, 0.0, 1.0).astype(np.float32))


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def _both_forms(monkeypatch, fn):
    import torch
    out = {}
    for form in ("0", "1"):
        monkeypatch.setenv("NGP_HASH_BWD_RUNS", form)
        out[form] = fn()
        torch.cuda.synchronize()
    monkeypatch.delenv("NGP_HASH_BWD_RUNS", raising=False)
    return out["0"], out["1"]


CASES = [
    # name, n, n_valid, pos stride, zero rows, layout
    ("full_2e18", 1 << 18, None, 3, False, "soa"),
    ("ragged", 4099, None, 3, False, "soa"),
    ("n_valid", 6000, 4321, 3, False, "soa"),
    ("stride4", 5003, None, 4, False, "soa"),
    ("zero_rows", 4100, None, 3, True, "soa"),
    ("aos", 4099, None, 3, True, "aos"),
    ("aos_n_valid_stride4", 3001, 2222, 4, True, "aos"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("aabb_scale", [1, 4])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_run_records_v2_form_equals_previous_form_bitwise(case, aabb_scale, monkeypatch):
    """k_bin_accumulate2<float, false> behind both forms of k_bin_runs2: the gradient overwritten and accumulated into a non-zero buffer."""
    import torch
    from jnerf_amd import ops
    name, n, n_valid, stride, zero_rows, layout = case
    table, _, n_params = ops.level_table(aabb_scale)
    x = _ray_batch(n, seed=11 + aabb_scale)
    rng = np.random.default_rng(7)
    g = (rng.standard_normal((n, 32)) * 1e-3).astype(np.float32)
    if zero_rows:
        g[rng.random(n) < 0.3] = 0.0                                   # interleaved padding rows: skipped, they do not end a run
        g[64:96] = 0.0                                                 # whole groups of eight without a gradient
    pos = torch.zeros((n, stride), dtype=torch.float32, device="cuda")
    pos[:, :3] = torch.from_numpy(x).cuda()
    pos = pos[:, :3]
    gt = torch.from_numpy(g).cuda()
    dl = gt.contiguous() if layout == "aos" else gt.view(n, 16, 2).permute(1, 0, 2).contiguous()
    lay = ops.LAYOUT_AOS if layout == "aos" else ops.LAYOUT_SOA
    nv = None if n_valid is None else torch.tensor([n_valid], dtype=torch.int32, device="cuda")
    ws = torch.empty(ops.hash_bwd_workspace_bytes(table, n, torch.float32), dtype=torch.uint8, device="cuda")
    seed_grad = torch.from_numpy((np.random.default_rng(3).standard_normal(n_params) * 1e-4).astype(np.float32)).cuda()

    def run():
        over = torch.full((n_params,), float("nan"), dtype=torch.float32, device="cuda")
        ops.hash_encode_bwd(pos, dl, table, n_params, grad=over, layout=lay, zero_first=True, workspace=ws, n_valid=nv)
        acc = seed_grad.clone()
        ops.hash_encode_bwd(pos, dl, table, n_params, grad=acc, layout=lay, zero_first=False, workspace=ws, n_valid=nv)
        return over, acc

    (o0, a0), (o1, a1) = _both_forms(monkeypatch, run)
    assert float(o0.abs().max()) > 0 and not bool(torch.isnan(o0).any())
    assert torch.equal(_bits(o0), _bits(o1)), f"{name}: overwritten gradient differs in {int((_bits(o0) != _bits(o1)).sum())} words"
    assert torch.equal(_bits(a0), _bits(a1)), f"{name}: accumulated gradient differs in {int((_bits(a0) != _bits(a1)).sum())} words"


@pytest.mark.gpu
@pytest.mark.parametrize("aabb_scale", [1, 4])
def test_riding_sweep_behind_both_run_record_forms_bitwise(aabb_scale, monkeypatch):
    """The native fp32 step (k_bin_accumulate2<float, true>: the table's Adam + EMA sweep rides, the MLP tail rides in k_bin_runs2's workgroups): 16 iterations from the
    same seed leave the same bits in every parameter and both Adam moments behind either form."""
    import torch
    from jnerf_amd.presets import ngp_cfg
    from jnerf_amd.runner import Runner

    def run():
        torch.manual_seed(0)
        ngp_cfg(n_images=8, W=96, H=96, target_batch_size=1 << 16, n_rays_per_batch=1024, fp16=False, aabb_scale=aabb_scale, const_dt=True, pipeline_sampling=False)
        r = Runner()
        for i in range(16):
            loss = r.train_step(i)
        r.drain()
        assert r._fast and r._fast.native
        adam = r.optimizer._nested_optimizer
        state = [p.detach().clone() for p in r.model.parameters()] + [t.detach().clone() for t in adam.param_groups[0]["m"]] + [t.detach().clone() for t in adam.param_groups[0]["values"]]
        return state, loss.detach().clone()

    (s0, l0), (s1, l1) = _both_forms(monkeypatch, run)
    assert torch.equal(_bits(l0), _bits(l1))
    assert any(float(t.abs().max()) > 0 for t in s0)
    for a, b in zip(s0, s1):
        assert torch.equal(_bits(a.float()) if a.dtype != torch.float32 else _bits(a), _bits(b.float()) if b.dtype != torch.float32 else _bits(b))
