"""tests/golden/resnet_plan_launches.json: the launch sequences, backward-stage tags and gradient layouts of DeepLabV3-CA,
FCN and FCN-SE that tests/test_resnet_plans_host.py compares against, recorded with that test's own mock. Run it only
when a launch sequence is meant to change, and review the diff of the fixture.

    python tools/gen_golden_resnet_plans.py
"""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import test_resnet_plans_host as t            # noqa: E402

if __name__ == "__main__":
    out = {}
    for name in t.NETS:
        out[name] = {}
        for dtype in t.DTYPES:
            with pytest.MonkeyPatch.context() as mp:
                r = out[name][dtype] = t.record(mp, name, dtype)
            print(name, dtype, len(r["forward"]), len(r["backward"]), r["on_bucket"], r["stage_ends"])
    with open(t.GOLDEN, "w") as f:
        json.dump(out, f, indent=0, separators=(",", ":"))
        f.write("\n")
