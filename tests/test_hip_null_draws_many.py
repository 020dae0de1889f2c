"""GPU: K null draws per bin (include/epilogos_nulldraws.h, --null-draws K).

(a) epg_null_dist_draws_parts against K x (epg_null_hist_from_binhist_parts, epg_pair_scores_s1_parts): the same float32
    bits, for every sampler, a model of 15 / 18 / 25 states, a last tile that is not full, an empty part, rows of one state and
    rows with columns that hold no state, with and without a quiescence mask; the shapes it refuses.
(b) epg_null_exceed against np.sort + np.searchsorted on |x|.
(c) the paired session with draws=5 against the statistic computed in numpy from five one-draw sessions; the same in three
    chunks; draws=1 against a session opened without the argument; paired S2 through the loop over the seeds.
(d) the command line: the p-value column, pairwiseDelta_* unchanged, two runs alike."""
import gzip

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from epilogos_amd.helpers import null_draw_seeds
from tests.test_hip_null_draws import KEYS, _hist, _states

pytestmark = pytest.mark.gpu
ROWS = (130, 0, 71)
SEEDS = null_draw_seeds(77, 3)


@pytest.fixture(scope="module")
def eng():
    from epilogos_amd import engine
    engine.require_gpu()
    return engine


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _dev_hist(x, S):
    return torch.from_numpy(np.ascontiguousarray(_hist(x, S)).view(np.int16)).cuda()


def _tables(S, widths, seed):
    """{width: device float32 [width + 1, S]} from the reference's own table expression."""
    from epilogos_amd.scores import s1ScoreTable
    q = np.random.default_rng(seed).random(S).astype(np.float32) + 0.05
    q /= q.sum()
    return {w: torch.from_numpy(s1ScoreTable(q, w)[1]).cuda() for w in set(widths)}


def _two_calls(eng, HAs, HBs, S, NA, NB, ga, gb, T, seed, keys):
    """The null distances of every part by the two existing calls."""
    OAs, OBs = eng.null_hist_from_binhist_parts(HAs, HBs, NA + NB, S, ga, gb, int(seed), keys)
    outs = eng.pair_scores_s1_parts(list(zip(HAs, HBs, OAs, OBs)), S, NA, NB, ga, gb, T[NA], T[NB], T[ga], T[gb])
    return [o["null"] for o in outs]


# ------------------------------------------------------------------------------------------------ (a) the draws kernel
DRAW_CASES = [(17, 16, 18, None), (379, 342, 15, None), (379, 342, 18, None), (379, 342, 25, None), (400, 500, 18, None), (379, 342, 18, 100)]


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("NA,NB,S,g", DRAW_CASES)
def test_draws_equal_the_two_calls(eng, NA, NB, S, g, masked):
    rng = np.random.default_rng([NA, NB, S, g or 0])
    ga, gb = (NA, NB) if g is None else (g, g)
    T = _tables(S, (NA, NB, ga, gb), S)
    xs = [(_states(rng, r, NA, S), _states(rng, r, NB, S)) for r in ROWS]
    HAs, HBs = [_dev_hist(a, S) for a, _b in xs], [_dev_hist(b, S) for _a, b in xs]
    masks = [torch.from_numpy((rng.random(r) < 0.3).astype(np.uint8)).cuda() for r in ROWS] if masked else None
    got = eng.null_dist_draws_parts(HAs, HBs, KEYS, S, NA, NB, ga, gb, T[ga], T[gb], SEEDS, masks=masks)
    assert [tuple(o.shape) for o in got] == [(3, r) for r in ROWS]
    for k, seed in enumerate(SEEDS):
        want = _two_calls(eng, HAs, HBs, S, NA, NB, ga, gb, T, seed, KEYS)
        for p, r in enumerate(ROWS):
            g_, w_ = _bits(got[p][k]), _bits(want[p])
            if masked:
                m = masks[p].cpu().numpy().astype(bool)
                assert np.isnan(got[p][k].cpu().numpy()[m]).all()
                g_, w_ = g_[~m], w_[~m]
            assert np.array_equal(g_, w_), (k, p)
    if not masked and (NA, NB, S, g) == (379, 342, 18, None):
        assert len({_bits(got[0][k]).tobytes() for k in range(3)}) == 3       # three seeds, three nulls
        eng._abi.call("epg_test_force", 0, 1)                                   # the column-by-column sampler: the same draws
        try:
            seq = eng.null_dist_draws_parts(HAs, HBs, KEYS, S, NA, NB, ga, gb, T[ga], T[gb], SEEDS)
        finally:
            eng._abi.call("epg_test_force", 0, 0)
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(seq, got))


def test_draws_of_many_seeds_and_parts(eng):
    """More seeds and more parts than one launch carries in its argument (32 each)."""
    NA, NB, S, rows = 17, 16, 18, (9,) * 40
    rng = np.random.default_rng(8)
    T = _tables(S, (NA, NB), 2)
    xs = [(_states(rng, r, NA, S), _states(rng, r, NB, S)) for r in rows]
    HAs, HBs = [_dev_hist(a, S) for a, _b in xs], [_dev_hist(b, S) for _a, b in xs]
    keys = [1000 * i for i in range(len(rows))]
    seeds = null_draw_seeds(3, 35)
    got = eng.null_dist_draws_parts(HAs, HBs, keys, S, NA, NB, NA, NB, T[NA], T[NB], seeds)
    for k in (0, 31, 32, 34):
        want = _two_calls(eng, HAs, HBs, S, NA, NB, NA, NB, T, seeds[k], keys)
        assert all(np.array_equal(_bits(got[p][k]), _bits(want[p])) for p in range(len(rows))), k


@pytest.mark.parametrize("NA,NB,S", [(379, 342, 40), (3000, 3001, 18)])
def test_draws_refuse_other_shapes_and_touch_nothing(eng, NA, NB, S):
    rng = np.random.default_rng(1)
    HA, HB = _dev_hist(_states(rng, 70, NA, S), S), _dev_hist(_states(rng, 70, NB, S), S)
    Ta, Tb = (torch.zeros((n + 1, S), dtype=torch.float32, device="cuda") for n in (NA, NB))
    out = torch.full((3, 70), 7.0, dtype=torch.float32, device="cuda")
    with pytest.raises(eng._abi.EpilogosHipError) as e:
        eng.null_dist_draws_parts([HA], [HB], [0], S, NA, NB, NA, NB, Ta, Tb, SEEDS, outs=[out])
    assert e.value.code == -2
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------------------------------------ (b) the exceedance counts
from tests.null_sampler_ref import exceed_inputs as _exceed_inputs, exceed_np as _exceed_np   # noqa: E402  (shared with test_hip_persistent_loops.py)


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("n", [1, 1000, 70001])
def test_exceed_equals_numpy(eng, n, seed):
    x, d = _exceed_inputs(seed, n)
    d = np.where(np.isnan(d), np.float32(0.5), d)                               # (a tie with a left-out entry: any real value)
    want = _exceed_np(x, d)
    exceed = torch.zeros(len(d), dtype=torch.int64, device="cuda")
    eng.null_exceed(torch.from_numpy(x).cuda(), torch.from_numpy(d).cuda(), exceed)
    assert np.array_equal(exceed.cpu().numpy(), want)
    assert (want[115:120] == 0).all() and want[100] == int((~np.isnan(x)).sum())
    # a second chunk accumulates
    x2, _ = _exceed_inputs(seed + 10, 777)
    eng.null_exceed(torch.from_numpy(x2).cuda(), torch.from_numpy(d).cuda(), exceed)
    assert np.array_equal(exceed.cpu().numpy(), want + _exceed_np(x2, d))


def test_exceed_workspace_too_small(eng):
    x = torch.zeros(1000, dtype=torch.float32, device="cuda")
    d = torch.zeros(5, dtype=torch.float32, device="cuda")
    e = torch.zeros(5, dtype=torch.int64, device="cuda")
    with pytest.raises(eng._abi.EpilogosHipError) as err:
        eng.null_exceed(x, d, e, ws=torch.empty(4096, dtype=torch.uint8, device="cuda"))
    assert err.value.code == -4 and int(e.sum()) == 0


# ------------------------------------------------------------------------------------------------ (c) the session
S_, NA_, NB_, R_ = 18, 20, 24, 300
SEED = 4242


def _session_inputs():
    rng = np.random.default_rng(99)
    parts = []
    for _ in range(2):
        a, b = _states(rng, R_, NA_, S_), _states(rng, R_, NB_, S_)
        quiet = rng.random(R_) < 0.25
        a[quiet], b[quiet] = S_ - 1, S_ - 1
        a[a < 0], b[b < 0] = 0, 0                                               # (a session checks that every byte is a state)
        parts.append((a, b))
    return parts


def _run_session(eng, sal, seed, **kw):
    from epilogos_amd import backend
    from epilogos_amd.driver import shuffle_key
    be = backend.HipBackend()
    sess = be.open_paired(S_, sal, S_ - 1, -1, int(seed), **kw)
    pids = [sess.add_staged(eng.states_to_device(a), NA_, eng.states_to_device(b), NB_, shuffle_key(fi, 0))
            for fi, (a, b) in enumerate(_session_inputs())]
    return sess, pids


def _finish_session(sess, pids):
    sess.launch(2 * R_, NA_ + NB_, pids)
    sess.finish(2 * R_, NA_ + NB_)
    return [sess.results(pid) for pid in pids]


_reference = {}


def _statistic(eng, sal):
    """(exceed per part, M) in numpy from five sessions of one draw each, seeded with null_draw_seeds(SEED, 5)."""
    if sal not in _reference:
        runs = [_finish_session(*_run_session(eng, sal, s)) for s in null_draw_seeds(SEED, 5)]
        quies = [r["quies"] for r in runs[0]]
        assert all(q.any() and not q.all() for q in quies)
        pool = np.sort(np.abs(np.concatenate([r["null"][~q] for run in runs for r, q in zip(run, quies)])))
        if sal == 1:                                                            # quiescent bins: exactly 0 in every draw
            assert all((r["null"][q] == 0).all() for run in runs for r, q in zip(run, quies))
        exceed = [(len(pool) - np.searchsorted(pool, np.abs(r["rdist"]), side="left")).astype(np.int64) for r in runs[0]]
        _reference[sal] = (exceed, len(pool), runs[0])
    return _reference[sal]


@pytest.mark.parametrize("chunks", [1, 3])
def test_session_exceed_equals_numpy(eng, chunks):
    want, M, first = _statistic(eng, 1)
    sess, pids = _run_session(eng, 1, SEED, draws=5)
    if chunks == 3:                                                             # two draws per chunk: 2 + 2 + 1
        Rtot = 2 * R_
        sess.null_chunk_bytes = 4 * 2 * Rtot + eng.null_exceed_ws_bytes(2 * Rtot)
        assert sess.null_chunk_bytes < 4 * 3 * Rtot + eng.null_exceed_ws_bytes(3 * Rtot)
    got = _finish_session(sess, pids)
    assert sess.null_fused is True and sess.null_chunks == chunks
    assert sess.null_pool == M == 5 * sum(int((~r["quies"]).sum()) for r in first)
    for g, w, f in zip(got, want, first):
        assert g["exceed"].dtype == np.int64 and np.array_equal(g["exceed"], w)
        for key in ("delta", "null", "quies", "rdist", "mdiff"):                # draw 0 is the run's own null: nothing else moves
            assert np.array_equal(g[key], f[key]), key


def test_session_one_draw_is_todays_session(eng):
    _want, _M, first = _statistic(eng, 1)
    got = _finish_session(*_run_session(eng, 1, SEED, draws=1))
    for g, f in zip(got, first):
        assert sorted(g) == sorted(f) == ["delta", "mdiff", "null", "quies", "rdist"]
        for key in g:
            assert g[key].dtype == f[key].dtype and g[key].tobytes() == f[key].tobytes(), key


def test_session_s2_takes_the_loop(eng):
    want, M, _first = _statistic(eng, 2)
    sess, pids = _run_session(eng, 2, SEED, draws=5)
    got = _finish_session(sess, pids)
    assert sess.null_fused is False and sess.null_pool == M
    for g, w in zip(got, want):
        assert np.array_equal(g["exceed"], w)


# ------------------------------------------------------------------------------------------------ (d) the command line
@pytest.fixture(scope="module")
def cli_inputs(tmp_path_factory):
    from tests.test_host_logic import write_tsv
    base = tmp_path_factory.mktemp("nulldraws")
    rng = np.random.default_rng(21)
    xs = []
    for d in ("A", "B"):
        (base / d).mkdir()
    for k, r in enumerate((64, 301, 1)):
        a, b = _states(rng, r, NA_, S_), _states(rng, r, NB_, S_)
        quiet = rng.random(r) < 0.2
        a[quiet], b[quiet] = S_ - 1, S_ - 1
        a[a < 0], b[b < 0] = 0, 0                                               # (the text format has no "no state")
        xs.append((a, b))
        for d, x in (("A", a), ("B", b)):
            write_tsv(base / d / ("matrix_chr%d.txt.gz" % (k + 1)), x, chrom="chr%d" % (k + 1))
    meta = base / "metadata.tsv"
    meta.write_text("zero_index\tone_index\tshort_name\n" + "".join("%d\t%d\tstate%d\n" % (i, i + 1, i + 1) for i in range(S_)))
    return base, meta, xs


def test_command_line(eng, tmp_path, cli_inputs):
    from epilogos_amd import backend
    from epilogos_amd.driver import shuffle_key
    from tests.test_hip_groups_pipeline import run_cli
    base, meta, xs = cli_inputs
    common = ["-m", "paired", "-a", str(base / "A"), "-b", str(base / "B"), "-j", str(meta), "-n", "-t", "3", "--null-seed", "5"]
    one = run_cli(common + ["--null-draws", "4"], tmp_path / "one")
    two = run_cli(common + ["--null-draws", "4"], tmp_path / "two")
    plain = run_cli(common, tmp_path / "plain")
    names = sorted(p.name for p in one.iterdir())
    assert names == sorted(p.name for p in two.iterdir()) == sorted(p.name for p in plain.iterdir())
    assert not [n for n in names if n.startswith("temp_")]
    for n in names:
        opener = gzip.open if n.endswith(".gz") else open
        with opener(one / n, "rb") as f1, opener(two / n, "rb") as f2, opener(plain / n, "rb") as f0:
            b1, b0 = f1.read(), f0.read()
            assert b1 == f2.read(), n                                           # reproducible under --null-seed
            if n.startswith("pairwiseDelta_"):
                assert b1 == b0, n                                              # draw 0 is the plain run's null
    # the host formula on the run's own distances and four explicit draws
    runs = []
    for s in null_draw_seeds(5, 4):
        sess = backend.HipBackend().open_paired(S_, 1, S_ - 1, -1, int(s))
        pids = [sess.add_staged(eng.states_to_device(a), NA_, eng.states_to_device(b), NB_, shuffle_key(fi, 0)) for fi, (a, b) in enumerate(xs)]
        total = sum(a.shape[0] for a, _b in xs)
        sess.launch(total, NA_ + NB_, pids)
        sess.finish(total, NA_ + NB_)
        runs.append([sess.results(pid) for pid in pids])
    quies = [r["quies"] for r in runs[0]]
    pool = np.sort(np.abs(np.concatenate([r["null"][~q] for run in runs for r, q in zip(run, quies)])))
    d = np.concatenate([r["rdist"] for r in runs[0]])
    p = (1.0 + (len(pool) - np.searchsorted(pool, np.abs(d), side="left"))) / (1.0 + len(pool))
    with gzip.open(one / "pairwiseMetrics_t.txt.gz", "rt") as fh:
        rows = [l.split("\t") for l in fh.read().splitlines()]
    assert len(rows) == len(d) == 366
    assert [r[4] for r in rows] == ["%.5f" % abs(float(x)) for x in d]
    assert [r[6] for r in rows] == ["%.5e" % x for x in p]
