"""GPU: the backend sessions fed with COLUMN GROUPS of one resident matrix give, bit for bit, what they give when fed with
matrices cut to those columns beforehand: exp_freq, the float32 scores of every part, and in paired mode the deltas, the null
distances (so the null groups agree draw by draw), the quiescence masks and STEP 4's reductions.

Parts of 64, 301 and 1 rows (two super-tiles and a tail, ten, a single row), 40 biosamples; the 18-state model takes the grouped
count pass (epg_bin_hist_groups), the 40-state model and S3 the device gather (engine.select_columns)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from epilogos_amd import backend, engine
from epilogos_amd.driver import shuffle_key

pytestmark = pytest.mark.gpu

ROWS, N = (64, 301, 1), 40
COLS = np.array([0, 1, 2, 5, 6, 7, 8, 11, 16, 17, 18, 19, 23, 30, 31, 38, 39])       # a scattered group, both ends of the row
COLS_A, COLS_B = np.arange(0, 17), np.arange(19, 40)                                  # biosamples 1-17 and 20-40


@pytest.fixture(scope="module")
def be():
    return backend.HipBackend()


def parts_of(S):
    rng = np.random.default_rng(S)
    # skewed like real data: most cells in the last state (the quiescent one); a fifth of the rows is quiescent in every column
    # of the paired groups and NOT in the two biosamples (18, 19) that belong to neither
    xs = [np.where(rng.random((r, N)) < 0.6, S - 1, rng.integers(0, S, size=(r, N))).astype(np.int8) for r in ROWS]
    for x in xs:
        quiet = rng.random(x.shape[0]) < 0.2
        x[quiet] = S - 1
        x[quiet, 17:19] = 0
    return xs


def run_single(be, S, sal, xs, columns):
    sess = be.open_single(S, sal)
    if columns is None:
        pids = [sess.add_device(engine.states_to_device(x), x.shape[1]) for x in xs]
        width = xs[0].shape[1]
    else:
        pids = [sess.add_device(engine.states_to_device(x), x.shape[1], columns=columns) for x in xs]
        width = len(columns)
    total = sum(x.shape[0] for x in xs)
    sess.launch(total, width, pids)
    q = sess.finish(total, width)
    return q, [sess.scores(pid) for pid in pids]


@pytest.mark.parametrize("S", (18, 40))
@pytest.mark.parametrize("sal", (1, 2, 3))
def test_single_session_columns(be, S, sal):
    xs = parts_of(S)
    q_cut, sc_cut = run_single(be, S, sal, [np.ascontiguousarray(x[:, COLS]) for x in xs], None)
    q_col, sc_col = run_single(be, S, sal, xs, COLS)
    assert q_col.shape == q_cut.shape and np.array_equal(q_col.view(np.uint32), q_cut.view(np.uint32))
    for a, b in zip(sc_col, sc_cut):
        assert a.shape == b.shape and a.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def run_paired(be, S, sal, groupSize, xs, cut):
    sess = be.open_paired(S, sal, S - 1, groupSize, 1234)
    pids = []
    for fi, x in enumerate(xs):
        if cut:
            pids.append(sess.add_staged(engine.states_to_device(x[:, COLS_A]), len(COLS_A), engine.states_to_device(x[:, COLS_B]),
                                        len(COLS_B), shuffle_key(fi, 0)))
        else:
            pids.append(sess.add_columns(engine.states_to_device(x), N, COLS_A, COLS_B, shuffle_key(fi, 0)))
    total, width = sum(x.shape[0] for x in xs), len(COLS_A) + len(COLS_B)
    sess.launch(total, width, pids)
    q = sess.finish(total, width)
    return q, [sess.results(pid) for pid in pids]


@pytest.mark.parametrize("S", (18, 40))
@pytest.mark.parametrize("groupSize", (-1, 10))
@pytest.mark.parametrize("sal", (1, 2))
def test_paired_session_columns(be, S, sal, groupSize):
    xs = parts_of(S)
    q_cut, res_cut = run_paired(be, S, sal, groupSize, xs, True)
    q_col, res_col = run_paired(be, S, sal, groupSize, xs, False)
    assert np.array_equal(q_col.view(np.uint32), q_cut.view(np.uint32))
    for a, b in zip(res_col, res_cut):
        assert sorted(a) == sorted(b)
        for key in a:
            assert a[key].shape == b[key].shape and a[key].dtype == b[key].dtype, key
            assert np.array_equal(a[key].view(np.uint8), b[key].view(np.uint8)), key
    assert any(r["quies"].any() for r in res_col) and any(r["null"].any() for r in res_col)


def test_columns_none_is_todays_path(be, monkeypatch):
    """Without columns the sessions never reach the grouped count pass or the gather."""
    def refuse(*a, **k):
        raise AssertionError("columns=None must take the existing path")
    monkeypatch.setattr(engine, "bin_hist_groups", refuse)
    monkeypatch.setattr(engine, "select_columns", refuse)
    xs = parts_of(18)
    run_single(be, 18, 1, xs, None)
    run_paired(be, 18, 1, -1, xs, True)
