"""Static instruction counts of a kernel split by PHASE, from the compiler's assembly with line tables (no GPU).  A phase starts at a source line of the kernel that holds the
comment `// ---- <name>`; what stands before the first marker is `setup`.  Every instruction is booked on the phase of the last line of the KERNEL'S OWN body that the line
table named before it: code inlined from helpers (calc_dt, wave_incl_max, ...) carries the helper's line and so goes to the phase that called it, as far as the scheduler kept
the phases apart - it moves a few instructions across a marker, so read the split to within a dozen instructions.  The counts behind DESIGN.md section 4a's table.

usage: python tools/isa_phase_count.py jnerf_amd/csrc/sampler.hip k_march_waveILj4ELb1E [extra hipcc flags ...]      (second argument: substring of the mangled name)"""
import collections
import re
import subprocess
import sys
import tempfile

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics", "-fvisibility=hidden", "-S", "--cuda-device-only", "-gline-tables-only"]
KINDS = (("vector", lambda k: k.startswith("v_")), ("scalar", lambda k: k.startswith("s_")), ("LDS", lambda k: k.startswith("ds_")),
         ("global", lambda k: k.startswith(("global_", "buffer_", "scratch_", "flat_"))))


def main():
    src, pat = sys.argv[1], sys.argv[2]
    with tempfile.NamedTemporaryFile(suffix=".s") as f:
        r = subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, *sys.argv[3:], src, "-o", f.name], capture_output=True, text=True)
        asm = open(f.name).read().split("\n")
    if len(asm) < 10:
        sys.exit(r.stderr[-2000:])
    start = next(i for i, l in enumerate(asm) if l.startswith("_Z") and pat in l and ":" in l)
    end = next(i for i in range(start, len(asm)) if asm[i].startswith(".Lfunc_end"))
    source = open(src).read().split("\n")
    # the kernel's own lines: from its `__global__` line (the .loc of the function's entry, or the nearest one above it) to the closing brace in column 0
    fileno, entry = next((m.group(1), int(m.group(2))) for l in asm[start:end] for m in [re.match(r"\s+\.loc\s+(\d+)\s+(\d+)", l)] if m)
    first = max(i for i in range(entry) if "__global__" in source[i]) + 1
    last = next(i for i in range(first, len(source)) if source[i].startswith("}")) + 1
    marks = [(i + 1, m.group(1)) for i in range(first - 1, last) for m in [re.search(r"// ---- (\w+)", source[i])] if m]
    phase_of = lambda line: ([n for ln, n in marks if ln <= line] or ["setup"])[-1]
    cnt = collections.defaultdict(collections.Counter)
    cur = "setup"
    for l in asm[start:end]:
        m = re.match(r"\s+\.loc\s+(\d+)\s+(\d+)", l)
        if m:
            if m.group(1) == fileno and first <= int(m.group(2)) <= last:
                cur = phase_of(int(m.group(2)))
            continue
        t = l.split()
        if t and not t[0].startswith((".", ";")) and not t[0].endswith(":"):
            cnt[cur][t[0]] += 1
    print(asm[start].split(":")[0], f"(source lines {first}..{last})")
    order = ["setup"] + [n for _, n in marks]
    print(f"{'phase':10s}" + "".join(f"{k:>9s}" for k, _ in KINDS))
    for ph in order + ["total"]:
        c = cnt[ph] if ph != "total" else sum((cnt[p] for p in order), collections.Counter())
        print(f"{ph:10s}" + "".join(f"{sum(v for k, v in c.items() if pred(k)):9d}" for _, pred in KINDS))


if __name__ == "__main__":
    main()
