#!/usr/bin/env python3
"""Records the null-group draws of the library that is built in the tree: a SHA-256 per case of tests/test_hip_null_draws.py.
Needs the GPU.  Run it on the commit whose draws are to be kept -- never to make a failing comparison pass.

    python tests/golden/make_golden_null_draws.py "<which build>"      # rewrites tests/golden/null_draws.json
"""
import json
import sys
from pathlib import Path

if len(sys.argv) != 2:
    sys.exit(__doc__)
ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from epilogos_amd import engine  # noqa: E402
from tests import test_hip_null_draws as t  # noqa: E402

engine.require_gpu()
doc = {"header": "SHA-256 of the outputs of epg_null_hist_from_binhist_parts (hist: null groups A, B) and epg_pair_count_null_parts "
                 "(fused: real groups A, B, state counts, null groups A, B), parts in order; cases and inputs: "
                 "tests/test_hip_null_draws.py.  Produced by: " + sys.argv[1],
       "digests": t.compute_digests(engine)}
t.FIXTURE.write_text(json.dumps(doc, indent=1) + "\n")
print("wrote", t.FIXTURE, len(doc["digests"]), "cases")
