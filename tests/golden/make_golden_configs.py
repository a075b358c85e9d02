"""Mints tests/golden/reference_configs_v1.json: every configuration file of the reference that this repository restates, loaded UNCHANGED through
jnerf_amd.utils.config.Config (the reference's loader, restated) and dumped - settings only, keys and values.  Needs the reference checkout:
    python tests/golden/make_golden_configs.py <reference checkout>
Checking against the fixture (tests/test_host_cpu.py, tests/test_neus_cpu.py) does not."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from jnerf_amd.utils.config import Config  # noqa: E402
from tests import reference_configs as RC  # noqa: E402

if __name__ == "__main__":
    ref = sys.argv[1]
    out = {rel: RC.encode(Config(os.path.join(ref, "projects", rel)).dump()) for rel in RC.FILES}
    with open(RC.FIXTURE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    for rel in RC.FILES:
        assert RC.reference_dump(rel) == Config(os.path.join(ref, "projects", rel)).dump(), rel
    print("wrote", RC.FIXTURE)
