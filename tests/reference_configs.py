"""The reference's configuration files as its loader resolves them, recorded in tests/golden/reference_configs_v1.json (tests/golden/make_golden_configs.py): what the
config tests compare this repository's projects/*/configs against, without the reference checkout.  JSON has no tuples; they are stored as {"__tuple__": [...]}, so a
loaded recording compares equal to a live Config(...).dump() exactly where the values AND their container types agree."""
import json
import os

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_configs_v1.json")
FILES = ("ngp/configs/ngp_base.py", "ngp/configs/ngp_fox.py", "ngp/configs/ngp_comp.py", "nerf/configs/nerf_base.py", "neus/configs/neus_womask.py", "neus/configs/neus_wmask.py")


def encode(x):
    if isinstance(x, dict):
        return {str(k): encode(v) for k, v in x.items()}
    if isinstance(x, tuple):
        return {"__tuple__": [encode(v) for v in x]}
    if isinstance(x, list):
        return [encode(v) for v in x]
    assert x is None or isinstance(x, (bool, int, float, str)), type(x)
    return x


def decode(x):
    if isinstance(x, dict):
        if set(x) == {"__tuple__"}:
            return tuple(decode(v) for v in x["__tuple__"])
        return {k: decode(v) for k, v in x.items()}
    if isinstance(x, list):
        return [decode(v) for v in x]
    return x


def reference_dump(rel):
    """Config(<reference>/projects/<rel>).dump() as recorded"""
    with open(FIXTURE) as f:
        return decode(json.load(f)[rel])
