"""`similaritySearch_run -b --gpus N` on the GPU: every output file of a build split over 2 and 3 STEP 2 processes is
byte-identical to the one-process build, and matches tests/golden/simsearch.npz as test_hip_simsearch.py checks it; also with
fewer regions than processes and on the chr1 example.  EPILOGOS_DIST_BACKEND=gloo lets the processes share one GPU; at most 3
of them hold it at once (the parent stays GPU-free)."""
import gzip
import os
import signal
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import simsearch_ref as ref

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
GOLD = np.load(ROOT / "tests" / "golden" / "simsearch.npz")
OUTPUTS = ["reduced_genome.npy", "simsearch.bed.gz", "simsearch.bed.gz.tbi", "simsearch_cube.npz", "simsearch_indices.npy"]


def _build(scores, out, gpus, extra=(), timeout=600):
    env = dict(os.environ, EPILOGOS_DIST_BACKEND="gloo")
    cmd = [sys.executable, "-m", "epilogos_amd.similaritySearch_run", "-b", "-s", str(scores), "-o", str(out),
           "--gpus", str(gpus)] + list(extra)
    # a session of its own: when the time limit ends the build, its STEP 2 children go with it
    p = subprocess.Popen(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         start_new_session=True)
    try:
        _out, err = p.communicate(timeout=timeout)
    finally:
        if p.poll() is None:
            os.killpg(p.pid, signal.SIGKILL)
            p.wait()
    assert p.returncode == 0, err[-3000:]
    assert sorted(p.name for p in out.iterdir()) == OUTPUTS
    return {f: (out / f).read_bytes() for f in OUTPUTS}


@pytest.mark.parametrize("case", ["s200", "s20"])
def test_split_builds_equal_the_one_gpu_build_and_the_golden(tmp_path, case):
    sp = tmp_path / "scores.txt"
    sp.write_bytes(GOLD[case + "_scores_txt"].tobytes())
    w = ["-w", str(int(GOLD[case + "_windowBP"])), "-j", "3"]
    one = _build(sp, tmp_path / "g1", 1, w)
    for n in (2, 3):
        got = _build(sp, tmp_path / ("g%d" % n), n, w)
        assert [f for f in OUTPUTS if got[f] != one[f]] == [], n
    assert gzip.decompress(one["simsearch.bed.gz"]) == GOLD[case + "_bed_text"].tobytes()
    got = np.load(tmp_path / "g3" / "simsearch_indices.npy")
    want = GOLD[case + "_indices"]
    keep = np.setdiff1d(np.arange(len(want)), GOLD[case + "_skip"])
    assert got.dtype == np.int32 and np.array_equal(got[keep], want[keep])


def test_fewer_regions_than_processes(tmp_path):
    lines = GOLD["s200_scores_txt"].tobytes().splitlines(keepends=True)
    sp = tmp_path / "short.txt"
    sp.write_bytes(b"".join(lines[:400]))                 # 400 bins: one region of interest
    one = _build(sp, tmp_path / "g1", 1)
    assert len(np.load(tmp_path / "g1" / "simsearch_indices.npy")) == 1
    assert _build(sp, tmp_path / "g3", 3) == one


def test_chr1_two_processes_equal_one(tmp_path):
    sp = ref.chr1_scores_file(tmp_path / "scores_chr1.txt.gz")
    one = _build(sp, tmp_path / "g1", 1, timeout=1200)
    two = _build(sp, tmp_path / "g2", 2, timeout=1200)
    assert [f for f in OUTPUTS if two[f] != one[f]] == []
    got = np.load(tmp_path / "g2" / "simsearch_indices.npy")[GOLD["chr1_rows"]]
    keep = np.setdiff1d(np.arange(len(got)), GOLD["chr1_skip"])
    assert np.array_equal(got[keep], GOLD["chr1_indices"][keep])
