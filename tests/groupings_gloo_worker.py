"""Worker for tests/test_groupings_host.py::test_two_ranks_keep_what_they_parsed (launched by torch.distributed.run, or plainly
for one rank): driver.run_groupings over the stand-in backend, one line of JSON per grouping in a file per rank next to the output directory."""
import json
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch.distributed as dist

from epilogos_amd import driver, helpers
from tests.groupings_backend import GroupingsBackend

ind, out, S = Path(sys.argv[1]), Path(sys.argv[2]), int(sys.argv[3])
specs = sys.argv[4:]
world = int(os.environ.get("WORLD_SIZE", "1"))
if world > 1:
    dist.init_process_group(backend="gloo")
plans = []
plan = driver._plan
driver._plan = lambda *a, **k: plans.append(plan(*a, **k)) or plans[-1]
groupings = [("g%d" % k, helpers.parseColumns(s)) for k, s in enumerate(specs)]
for name, _q, results, info in driver.run_groupings(sorted(ind.glob("*")), groupings, S, 1, out, "t", backend=GroupingsBackend(), keep_temps=False):
    helpers.flushCacheWrites()                                   # (--cache-dir: the side-cars of the first pass exist from here on)
    if world > 1:
        dist.barrier()
    rank = int(os.environ.get("RANK", "0"))
    with open(out.parent / ("info_%d_rank%d.jsonl" % (world, rank)), "a") as fh:      # (a file per rank: two ranks' stdout lines can mix)
        fh.write(json.dumps({"rank": rank, "name": name, "plans": len(plans), "layout": plans[0][0], "results": results is not None,
                             **info}) + "\n")
if world > 1:
    dist.destroy_process_group()
