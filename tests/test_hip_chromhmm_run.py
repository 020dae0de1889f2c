"""GPU: `epilogos --chromhmm DIR` against the two commands it joins -- `epilogos-prep DIR META SIZES -o M/`, then `epilogos -i M/`
with the same remaining options -- on small inputs whose shapes are about order, pitch and edges: the output directories hold the
same file names and the same bytes.  Everything runs in this process (the command lines through click's runner), so that the
whole module takes seconds; the inputs come from the generators of the prep kernels' tests."""
import io
import re
from pathlib import Path

import numpy as np
import pytest

from epilogos_amd import driver, preprocess, stateByLine as sbl
from tests.test_groupings_host import same_tree
from tests.test_hip_segments import make_lines, random_runs
from tests.test_hip_statebyline import make_text

pytestmark = pytest.mark.gpu

S = 18
CHROMS = [("chr10", 1), ("chr2", 513), ("chr1", 3001)]           # in the order of the chromsizes file; chrM, which no file holds, between them
SIZES = ["chr10", "chr2", "chrM", "chr1"]
RUN_ORDER = ["chr1", "chr2", "chr10"]
WIDTH = 100                                                      # of the segment files


def _states_file(path, n):
    path.write_text("zero_index\tone_index\tshort_name\n" + "".join("%d\t%d\tstate%d\n" % (i, i + 1, i + 1) for i in range(n)))
    return path


def _invoke(args):
    from click.testing import CliRunner
    from epilogos_amd import run
    try:
        return CliRunner().invoke(run.main, [str(a) for a in args])
    finally:
        driver.abort_early_readers()
        try:
            driver.finish_writes()
        except Exception:
            pass


def _ok(args):
    res = _invoke(args)
    assert res.exit_code == 0 and res.exception is None and "ERROR" not in res.output, res.output + repr(res.exception)
    return res.output


def _prep(src, meta, sizes, dest, **kw):
    out = io.StringIO()
    preprocess.run(src, meta, sizes, dest, out=out, **kw)
    return out.getvalue()


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The inputs, and the first of the two commands on each of them (module-wide: the matrices of the two-command route)."""
    base = tmp_path_factory.mktemp("chromhmm")
    rng = np.random.default_rng(1812)
    calls = base / "calls"
    calls.mkdir()
    for c, R in CHROMS:
        for k in range(17):
            v = rng.integers(1, S + 1, size=R)
            if c == "chr2" and k == 2:
                v[7] = S                                         # (whatever the draw: the model's last state is in the data)
            text = make_text(v, head=b"B%03d\t%s\nMaxStateE\n" % (k, c.encode()), final_newline=k % 2 == 0)
            if c == "chr2" and k == 3:
                text = text.replace(b"\n", b"\r\n")              # outside the strict grammar: the host fallback
            (calls / ("B%03d_18_%s_statebyline.txt" % (k, c))).write_bytes(text)
    for n in (5, 17):                                            # (B999: a biosample without files has no column)
        (base / ("meta%d.txt" % n)).write_text("id\n" + "".join("B%03d\n" % k for k in range(n // 2)) + "B999\n"
                                               + "".join("B%03d\n" % k for k in range(n // 2, n)))
    (base / "sizes.txt").write_text("".join("%s\t%d\n" % (c, dict(CHROMS).get(c, 83) * 200) for c in SIZES))

    segs = base / "segments"
    segs.mkdir()
    for k in range(5):
        per = [(c, *random_runs(rng, R, top=S)) for c, R in CHROMS[::-1]]
        labels = ("%d", "E%d", "Quies%.0s", "%d_TssFlnk") if k == 1 else ("%d", "E%d", "U%d", "%d_TssFlnk")
        lines = make_lines([("chrUn", [2, 1], [1, 2])] + per, W=WIDTH, labels=labels)
        (segs / ("B%03d_18_segments.bed" % k)).write_bytes(b"".join(b"\t".join(l) + b"\n" for l in lines))
    (base / "sizes_seg.txt").write_text("".join("%s\t%d\n" % (c, dict(CHROMS).get(c, 83) * WIDTH) for c in SIZES))
    (base / "names.tsv").write_text("one_index\tshort_name\n%d\tQuies\n" % S)

    small = base / "calls15"                                     # for the 15-state model: chr2 alone holds a state above 15
    small.mkdir()
    for c, R in (("chr2", 40), ("chr1", 33)):
        for k in range(5):
            v = rng.integers(1, 16, size=R)
            if c == "chr2" and k == 4:
                v[11] = S
            (small / ("B%03d_18_%s_statebyline.txt" % (k, c))).write_bytes(make_text(v, head=b"B%03d\t%s\nMaxStateE\n" % (k, c.encode())))

    progress = {}
    progress[17] = _prep(calls, base / "meta17.txt", base / "sizes.txt", base / "m17")
    progress[5] = _prep(calls, base / "meta5.txt", base / "sizes.txt", base / "m5")
    progress["seg"] = _prep(segs, base / "meta5.txt", base / "sizes_seg.txt", base / "mseg", segments=True, width=WIDTH,
                            state_names=base / "names.tsv")
    progress[15] = _prep(small, base / "meta5.txt", base / "sizes.txt", base / "m15")
    assert sorted(p.name for p in (base / "m17").iterdir()) == sorted("matrix_%s.epgm" % c for c in RUN_ORDER)
    h = sbl.read_epgm_header(base / "m17" / "matrix_chr2.epgm")
    assert (h["R"], h["N"], h["hi"]) == (513, 17, S) and sbl.read_epgm_header(base / "mseg" / "matrix_chr1.epgm")["width"] == WIDTH
    return {"base": base, "progress": progress, "j18": _states_file(base / "states18.tsv", 18), "j15": _states_file(base / "states15.tsv", 15),
            "src": {17: ["--chromhmm", calls, "--metadata", base / "meta17.txt", "--chromsizes", base / "sizes.txt"],
                    5: ["--chromhmm", calls, "--metadata", base / "meta5.txt", "--chromsizes", base / "sizes.txt"],
                    "seg": ["--chromhmm", segs, "--metadata", base / "meta5.txt", "--chromsizes", base / "sizes_seg.txt", "--segments",
                            "--bin-width", WIDTH, "--state-names", base / "names.tsv"],
                    15: ["--chromhmm", small, "--metadata", base / "meta5.txt", "--chromsizes", base / "sizes.txt"]},
            "m": {17: base / "m17", 5: base / "m5", "seg": base / "mseg", 15: base / "m15"}}


def _both(world, which, args, tmp_path):
    """The one command and the second of the two commands with the same options -> (output dir of the one, of the two, the one's output)."""
    args = list(args) + ["-j", world["j18"], "-f", "t", "-w", "5"]
    said = _ok(world["src"][which] + args + ["-o", tmp_path / "one"])
    _ok(["-i", world["m"][which]] + args + ["-o", tmp_path / "two"])
    return tmp_path / "one", tmp_path / "two", said


@pytest.mark.parametrize("which,args,a_file", [
    (17, ["-s", "1"], "scores_t_matrix_chr10.txt.gz"), (5, ["-s", "1"], "regionsOfInterest_t.txt"),
    (17, ["-s", "2"], "scores_t_matrix_chr2.txt.gz"), (17, ["-s", "3"], "scores_t_matrix_chr1.txt.gz"),
    (17, ["-s", "1", "--columns", "2-4,17,9"], "scores_t_matrix_chr1.txt.gz"),
    (5, ["-s", "1", "--columns", "5,1"], "scores_t_matrix_chr1.txt.gz"),
    ("seg", ["-s", "1"], "scores_t_matrix_chr10.txt.gz"),
])
def test_single_mode_writes_the_bytes_of_the_two_commands(world, tmp_path, which, args, a_file):
    one, two, said = _both(world, which, args, tmp_path)
    assert a_file in same_tree(one, two)
    # the progress lines of epilogos-prep first (a file read on the host is warned about in their midst, as there), then the run's own
    assert said.count("on the host") == 1                        # (the \r\n calls; the segment file whose labels are names)
    lines = re.sub(r"epilogos_amd: [^\n]*\n", "", said)
    assert lines.startswith(world["progress"][which]) and "State Model" in lines[len(world["progress"][which]):]
    assert "Processing chrM: 0 files found. Skipping.\n" in world["progress"][which]


@pytest.mark.parametrize("args", [
    ["-n", "--null-seed", "7", "-t", "1"],
    ["-n", "--null-seed", "7", "--null-draws", "3"],
    ["--null-seed", "7", "-s", "2", "-g", "4", "-q", "3"],
])
def test_paired_columns_follow_the_run_order_of_the_matrix_files(world, tmp_path, args):
    """The null shuffle is keyed by the file's ordinal: handed over in the order of the chromsizes file (chr10, chr2, chr1) these
    bytes differ.  (-n with one trial and the default -z: the fit is over all null distances, no sub-sample is drawn at random.)"""
    one, two, _said = _both(world, 17, ["-m", "paired", "--columns-a", "1-8", "--columns-b", "17,9-16"] + args, tmp_path)
    names = same_tree(one, two)
    assert "pairwiseMetrics_t.txt.gz" in names and "pairwiseDelta_t_matrix_chr10.txt.gz" in names


def _spy_on_groupings(monkeypatch):
    """-> [(info, bytes torch has allocated on the device)] of every grouping a run goes through, filled as it runs."""
    import torch
    seen = []
    real = driver.run_groupings

    def spy(*a, **k):
        runs = real(*a, **k)
        try:
            for item in runs:
                torch.cuda.synchronize()
                seen.append((item[3], torch.cuda.memory_allocated()))
                yield item
        finally:
            runs.close()
    monkeypatch.setattr(driver, "run_groupings", spy)
    return seen


@pytest.mark.parametrize("paired", [False, True])
def test_groupings_run_from_the_one_residency(world, tmp_path, monkeypatch, paired):
    g = tmp_path / "g.tsv"
    if paired:
        g.write_text("halves\t1-8\t9-17\nsmall\t3\t5,17\n")
        args, which, names = ["-m", "paired", "-n", "--null-seed", "7", "-t", "1", "--groupings", g], 17, ["halves", "small"]
    else:
        g.write_text("all\t1-5\none\t4\nmixed\t5,1-2\n")
        args, which, names = ["--groupings", g], 5, ["all", "one", "mixed"]
    monkeypatch.delenv("EPILOGOS_RESIDENT_BYTES", raising=False)
    seen = _spy_on_groupings(monkeypatch)
    said = _ok(world["src"][which] + args + ["-j", world["j18"], "-f", "t", "-w", "5", "-o", tmp_path / "one"])
    mine, seen[:] = list(seen), []
    _ok(["-i", world["m"][which]] + args + ["-j", world["j18"], "-f", "t", "-w", "5", "-o", tmp_path / "two"])
    assert sorted(p.name for p in (tmp_path / "one").iterdir()) == sorted(names)
    for name in names:
        same_tree(tmp_path / "one" / name, tmp_path / "two" / name)
    assert len(mine) == len(names) == len(seen)
    assert all(info["uploads"] == 0 and info["parsed_files"] == 0 and info["kept_files"] == 3 for info, _b in mine)
    assert (seen[0][0]["uploads"], seen[0][0]["parsed_files"]) == (3, 3)       # (the other route read and uploaded them)
    assert mine[-1][1] <= mine[0][1]                             # nothing is built again, nothing piles up between the groupings
    assert said.index("Processing chr10") < said.index("Grouping 1 of %d" % len(names))


def test_keep_matrices_writes_the_files_of_the_first_command(world, tmp_path):
    args = ["-s", "1", "-j", world["j18"], "-f", "t", "-w", "5"]
    _ok(world["src"][17] + args + ["-o", tmp_path / "kept", "--keep-matrices", tmp_path / "k" / "matrices"])
    _ok(world["src"][17] + args + ["-o", tmp_path / "plain"])
    same_tree(tmp_path / "k" / "matrices", world["m"][17])
    assert "scores_t_matrix_chr2.txt.gz" in same_tree(tmp_path / "kept", tmp_path / "plain")


def _files_under(d):
    return [p for p in Path(d).rglob("*") if p.is_file()] if Path(d).exists() else []


@pytest.mark.parametrize("check", [False, True])
def test_a_model_smaller_than_the_data_ends_as_on_the_two_command_route(world, tmp_path, check):
    """An 18-state call under a 15-state -j.  Whatever the route over the matrix files does with it -- their headers say 1..18, and the
    readers refuse that before a census is taken -- the one command does, naming the matrix by the path it would have had."""
    args = ["-j", world["j15"], "-f", "t"] + (["--check-states"] if check else [])
    two = _invoke(["-i", world["m"][15]] + args + ["-o", tmp_path / "two"])
    one = _invoke(world["src"][15] + args + ["-o", tmp_path / "one"])
    kept = _invoke(world["src"][15] + args + ["-o", tmp_path / "kept", "--keep-matrices", tmp_path / "k"])
    assert two.exit_code == one.exit_code == kept.exit_code == 1
    assert type(one.exception) is type(two.exception) is type(kept.exception)
    tail = str(two.exception)
    assert str(world["m"][15] / "matrix_chr2.epgm") in tail and "18" in tail and "15-state" in tail
    assert str(one.exception) == tail.replace(str(world["m"][15]) + "/", "")
    assert str(kept.exception) == tail.replace(str(world["m"][15]), str(tmp_path / "k"))
    for d in ("one", "two", "kept"):
        assert not _files_under(tmp_path / d)
    same_tree(tmp_path / "k", world["m"][15])                    # written as built, before the refusal


def test_check_states_censuses_a_resident_matrix_where_it_is(world, tmp_path, capsys):
    """driver.run_groupings over matrices handed in on the device: a byte that is no state is found by the census of the first
    grouping, named by the matrix's virtual path, before anything is written."""
    import torch
    rng = np.random.default_rng(5)
    files, resident = [Path("kept/matrix_chr1.epgm"), Path("kept/matrix_chr2.epgm")], {}
    for f, R in zip(files, (70, 33)):
        x = np.full((R, 16), -1, dtype=np.int8)
        x[:, :5] = rng.integers(0, S, size=(R, 5))
        resident[f] = (torch.from_numpy(x).cuda(), 5, sbl.synth_locations(f.stem[len("matrix_"):], 0, R))
    resident[files[1]][0][20, 3] = 77
    resident[files[1]][0][30, 0] = 99
    cols = np.arange(3)
    clean = {f: resident[f] for f in files[:1]}
    (name, q, results, info), = driver.run_groupings(files[:1], [("g", cols)], S, 1, tmp_path / "clean", "t", keep_temps=False,
                                                     checkStates=True, resident=clean)
    assert info["uploads"] == 0 and list(results) == ["matrix_chr1"]
    capsys.readouterr()
    with pytest.raises(driver.StateCheckFailed):
        list(driver.run_groupings(files, [("g", cols), ("h", cols)], S, 1, tmp_path / "bad", "t", keep_temps=False, checkStates=True,
                                  resident=resident))
    assert capsys.readouterr().out.strip() == driver.state_check_message("kept/matrix_chr2.epgm", 20, 4, 77, S)
    assert not _files_under(tmp_path / "bad")


def test_matrices_that_do_not_fit_next_to_a_session_stop_the_run(world, tmp_path, monkeypatch):
    """Only the reported number is changed: the device is asked nothing it could not give."""
    monkeypatch.setattr(driver, "_device_free", lambda X: 1 << 20)
    res = _invoke(world["src"][17] + ["-j", world["j18"], "-f", "t", "-o", tmp_path / "o"])
    nbytes = sum(R * 32 for _c, R in CHROMS)
    assert res.exit_code == 1
    last = res.output.strip().splitlines()[-1]
    assert last.startswith("ERROR: [--chromhmm] the matrices do not fit on the device")
    assert "%d bytes" % nbytes in last and "%d bytes free" % (2 * nbytes + (2 << 30)) in last and "%d bytes are free" % (1 << 20) in last
    assert "epilogos-prep" in last and "epilogos -i" in last
    assert "State Model" not in res.output and not _files_under(tmp_path / "o")
