#!/usr/bin/env python3
"""tests/golden/statebyline.npz: the reference's ten bundled ChromHMM state-by-line files of chr1 (data/ChromHMM), cut to their two
header lines plus bins 50 001 .. 52 048 (the slice of real_slice.npz), and the `matrix_chr1.txt` the reference's own
bin/preprocess_data_ChromHMM.sh makes of the cut files.  Data only: the script is run where it lies, nothing of it is stored.

Stored: names (the ten file names, metadata order), text_<k> (the bytes of cut file k, not compressed), metadata and chromsizes
(the bytes of the two files the script was given), matrix (the bytes of matrix_chr1.txt).

Runs only in the build container, where the reference is mounted (make_golden.py)."""
import gzip
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
from make_golden import HERE, REF  # noqa: E402

LO, HI = 50000, 52048


def main():
    work = Path(tempfile.mkdtemp(prefix="epg_golden_sbl_"))
    data = work / "calls"
    data.mkdir()
    src = sorted(Path(REF, "data", "ChromHMM").glob("*chr1_statebyline.txt.gz"))
    assert len(src) == 10, src
    names, texts = [], []
    for f in src:
        lines = gzip.open(f, "rb").read().split(b"\n")
        cut = b"\n".join(lines[:2] + lines[2 + LO:2 + HI]) + b"\n"
        with gzip.open(data / f.name, "wb") as out:
            out.write(cut)
        names.append(f.name)
        texts.append(cut)
    metadata = "biosample\tnote\n" + "".join("%s\tx\n" % n.split("_")[0] for n in names)
    (work / "metadata.txt").write_text(metadata)
    (work / "chr1.genome").write_text("chr1\t249250621\n")
    subprocess.run(["bash", REF + "/bin/preprocess_data_ChromHMM.sh", str(data), str(work / "metadata.txt"), str(work / "chr1.genome")],
                   cwd=work, check=True, stdout=subprocess.DEVNULL)
    matrix = (work / "matrix_chr1.txt").read_bytes()
    assert matrix.count(b"\n") == HI - LO
    arrays = {"names": np.array(names), "metadata": np.frombuffer(metadata.encode(), dtype=np.uint8),
              "chromsizes": np.frombuffer(b"chr1\t249250621\n", dtype=np.uint8), "matrix": np.frombuffer(matrix, dtype=np.uint8)}
    for k, t in enumerate(texts):
        arrays["text_%d" % k] = np.frombuffer(t, dtype=np.uint8)
    np.savez_compressed(HERE / "statebyline.npz", **arrays)
    print("statebyline.npz: %d bytes" % (HERE / "statebyline.npz").stat().st_size)


if __name__ == "__main__":
    main()
