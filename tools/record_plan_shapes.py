#!/usr/bin/env python3
"""Re-record tests/golden/plan_shapes.json (tests/test_plan_check.py test_plan_shapes_match_the_recorded_ones) from the
library in the tree: CPU only, planning-only engines.  Review the diff before committing it -- a moved budget or chunk
count moves speed.
usage: tools/record_plan_shapes.py [output.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest  # noqa: E402
import test_plan_check as tp  # noqa: E402

pkg = conftest.load_package()
import importlib  # noqa: E402
synth = importlib.import_module("iqtree_amd.synth")
records = {}
for env in tp.ENVS:
    for k in [k for k in os.environ if k.startswith("IQHIP_") and k != "IQHIP_LIB_DIR"]:
        del os.environ[k]
    os.environ.update(env)
    for cus in (256, 64):
        for shape in tp.SHAPES:
            records[tp.plan_shape_key(shape, env, cus)] = tp.plan_shapes(pkg, synth, shape, cus)
out = sys.argv[1] if len(sys.argv) > 1 else tp.GOLDEN_PLAN_SHAPES
with open(out, "w") as f:
    f.write('{"slots": %s,\n "records": {\n' % json.dumps(list(pkg.PLAN_SHAPE_SLOTS)))
    f.write(",\n".join('  %s: %s' % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in sorted(records.items())))
    f.write("\n }}\n")
print("wrote %s: %d keys" % (out, len(records)))
