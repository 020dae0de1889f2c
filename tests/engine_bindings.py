"""The table tests/test_engine_bindings_host.py and tests/test_hip_engine_bindings.py share: for every engine wrapper that reaches the
library, a factory of the smallest valid call -- R = 8 bins, N = 5 columns, S = 3 states, K = 2 draws, two parts (8 and 3 rows), one
BGZF member, G = 16 rows and W = 4 for similarity search.  epg_pair_count_null_parts serves 15-, 18- and 25-state models only: its
row has S = 15, the smallest it accepts.  A factory builds everything on the device it is given ("cpu" for the host test) with
torch and numpy alone; the workspaces are sized by the engine's own size queries, so build the cases before patching _abi.call."""
import zlib

import numpy as np
import torch

R, N, S, K, G, W = 8, 5, 3, 2, 16, 4
ROWS = (R, 3)


class Case:
    """kwargs: the call.  pitched: arguments the kernel takes with a row pitch.  sizes: arguments whose own shape IS the call's
    size (one element fewer is a smaller valid call, nothing to refuse).  scratch: capacity buffers, whose size travels to the
    library next to them (too small is the library's EPG_ERR_WORKSPACE / its flags: tests/test_hip_abi_calls.py).  check(out, kwargs)
    -> bool: the result against a one-line oracle."""

    def __init__(self, kwargs, pitched=(), sizes=(), scratch=(), check=None):
        self.kwargs, self.pitched, self.sizes, self.scratch, self.check = kwargs, set(pitched), set(sizes), set(scratch), check


def states(dev, rows=R, n=N, s=S, seed=0):
    from epilogos_amd import engine
    x = np.full((rows, engine.padded_width(n)), -1, dtype=np.int8)
    x[:, :n] = np.random.default_rng(seed).integers(0, s, size=(rows, n))
    return torch.from_numpy(x).to(dev)


def hist(X, n=N, s=S):
    return torch.nn.functional.one_hot(X[:, :n].long(), s).sum(1).to(torch.int16)


def _z(dev, shape, dtype):
    return torch.zeros(shape, dtype=dtype, device=dev)


def _ws(dev, nbytes):
    return torch.empty(int(nbytes), dtype=torch.uint8, device=dev)


def _q(dev, n=S):
    return torch.full((n,), 1.0 / n, dtype=torch.float32, device=dev)


def _table(dev, width):
    """kl(c / width, 1 / S), c = 0 .. width: the S1 table of a uniform background."""
    p = np.arange(width + 1, dtype=np.float64)[:, None] / width * np.ones(S)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(p > 0, p * np.log2(p * S), 0.0)
    return torch.from_numpy(t.astype(np.float32)).to(dev)


def _hists(dev, s=S):
    XA, XB = [states(dev, r, seed=1 + r, s=s) for r in ROWS], [states(dev, r, seed=9 + r, s=s) for r in ROWS]
    return [hist(x, s=s) for x in XA], [hist(x, s=s) for x in XB]


def _outs(dev, rows=R):
    return dict(out32=_z(dev, (rows, S), torch.float32), out64=_z(dev, (rows, S), torch.float64))


def _tables(dev):
    return dict(TA=_table(dev, N), TB=_table(dev, N), TnA=_table(dev, N), TnB=_table(dev, N))


def _grid(dev, rows=G):
    return torch.from_numpy(np.random.default_rng(5).integers(0, 10, size=(rows, S)).astype(np.int32)).to(dev)


def _text(dev, data):
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev)


def _engine():
    from epilogos_amd import engine
    return engine


def bin_hist(dev):
    return Case(dict(X=states(dev), N=N, S=S, counts=_z(dev, S, torch.int64), H=_z(dev, (R, S), torch.int16)), pitched={"X"},
                check=lambda out, kw: torch.equal(out[0], hist(kw["X"])) and out[1].tolist() == hist(kw["X"]).long().sum(0).tolist())


def bin_hist_s2(dev):
    return Case(dict(X=states(dev), N=N, S=S, counts2=_z(dev, S * S, torch.int64), H=_z(dev, (R, S), torch.int16), counts=_z(dev, S, torch.int64)),
                pitched={"X"}, check=lambda out, kw: torch.equal(out[0], hist(kw["X"])))


def bin_hist_parts(dev):
    return Case(dict(Xs=[states(dev, r, seed=r) for r in ROWS], Ns=[N, N], S=S, counts=_z(dev, S, torch.int64),
                     Hs=[_z(dev, (r, S), torch.int16) for r in ROWS]), pitched={"Xs"},
                check=lambda out, kw: all(torch.equal(h, hist(x)) for h, x in zip(out[0], kw["Xs"])))


def bin_hist_groups(dev):
    return Case(dict(X=states(dev), N=N, S=S, groups=[np.array([0, 1]), np.array([2, 3, 4])], counts=_z(dev, 2 * S, torch.int64)), pitched={"X"},
                check=lambda out, kw: torch.equal(out[0][0] + out[0][1], hist(kw["X"])))


def state_census(dev):
    return Case(dict(X=states(dev), N=N, S=S, census=_z(dev, (N, S), torch.int64), other=_z(dev, N, torch.int64),
                     first_bad=torch.full((1,), _engine().FIRST_BAD_NONE, dtype=torch.int64, device=dev)), pitched={"X"},
                check=lambda out, kw: out[0].sum(0).tolist() == hist(kw["X"]).long().sum(0).tolist())


def concordance(dev):
    return Case(dict(X=states(dev), N=N, S=S, agree=_z(dev, (N, N), torch.int64), both=_z(dev, (N, N), torch.int64),
                     ws=_ws(dev, _engine().concordance_ws_bytes(R, N, S))), pitched={"X"}, scratch={"ws"},
                check=lambda out, kw: out[0].diagonal().tolist() == [R] * N)


def _sample(dev, M=64):
    return torch.from_numpy(np.random.default_rng(2).normal(size=M).astype(np.float32)).to(dev)


def gennorm_fit(dev):
    idx = torch.from_numpy(np.random.default_rng(3).integers(0, 64, size=(2, 32)).astype(np.int32)).to(dev)
    return Case(dict(x=_sample(dev), idx=idx, ws=_ws(dev, _engine().gennorm_ws_bytes(64, 2, 32))), sizes={"x", "idx"}, scratch={"ws"})


def gennorm_nnlf(dev):
    params = torch.tensor([[1.5, 0.0, 1.0], [2.0, 0.1, 0.9]], dtype=torch.float64, device=dev)
    return Case(dict(x=_sample(dev), params=params, ws=_ws(dev, _engine().gennorm_ws_bytes(64, 2, 0))), sizes={"x"}, scratch={"ws"})


def gennorm_pvals(dev):
    return Case(dict(x=_sample(dev), params=torch.tensor([2.0, 0.0, 1.0], dtype=torch.float64, device=dev)), sizes={"x"})


def bh_adjust(dev):
    p = torch.from_numpy(np.random.default_rng(4).uniform(size=64)).to(dev)
    return Case(dict(p=p, ws=_ws(dev, _engine().bh_ws_bytes(64))), sizes={"p"}, scratch={"ws"})


def format_scores(dev):
    eng = _engine()
    row = b"chr1\t100\t300"
    return Case(dict(scores=torch.arange(R * S, dtype=torch.float32, device=dev).view(R, S) / 8, loc=_text(dev, row * R),
                     loc_off=torch.arange(R + 1, dtype=torch.int64, device=dev) * len(row),
                     text=_ws(dev, eng._scratch_bytes("epgw_text_bytes_max", R, S, len(row) * R)), ws=_ws(dev, eng._scratch_bytes("epgw_format_ws_bytes", R))),
                pitched={"scores"}, sizes={"scores"}, scratch={"loc", "text", "ws"},
                check=lambda out, kw: int(out[2][0]) == 0 and bytes(out[0][:int(out[1][R])].tolist()).count(b"\n") == R)


def bgzf_compress(dev):
    import gzip
    eng = _engine()
    data = b"abc\n" * R
    return Case(dict(text=_text(dev, data), n=len(data), row_off=torch.arange(R + 1, dtype=torch.int64, device=dev) * 4,
                     out=_ws(dev, eng._scratch_bytes("epgw_bgzf_bytes_max", len(data), 1)), ws=_ws(dev, eng._scratch_bytes("epgw_bgzf_ws_bytes", len(data)))),
                sizes={"row_off"}, scratch={"out", "ws"}, check=lambda out, kw: gzip.decompress(bytes(out[0][:int(out[1][0])].tolist())) == data)


def format_metrics(dev):
    eng = _engine()
    chrom, chrom_off, chrom_bytes, _m = eng._name_table(["chr1", "chr2"], dev)
    names, names_off, names_bytes, _m = eng._name_table(["s%d" % k for k in range(S)], dev)
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
    limit = eng._abi.header_constant_of(eng._abi.METRICS["metrics_text"], "EPGM_NAME_MAX")
    return Case(dict(chrom=chrom, chrom_off=chrom_off, chrom_bytes=chrom_bytes, chrom_idx=_z(dev, R, torch.int32), start=i64(range(0, 200 * R, 200)),
                     end=i64(range(200, 200 * R + 200, 200)), names=names, names_off=names_off, names_bytes=names_bytes,
                     maxdiff=torch.ones(R, dtype=torch.int32, device=dev), dist=torch.linspace(-1, 1, R, dtype=torch.float32, device=dev),
                     pvals=torch.linspace(0.1, 0.9, R, dtype=torch.float64, device=dev), mh=torch.linspace(0.2, 1.0, R, dtype=torch.float64, device=dev),
                     text=_ws(dev, eng._scratch_bytes("epgm_text_bytes_max", R, limit, limit, 1)), ws=_ws(dev, eng._scratch_bytes("epgm_format_ws_bytes", R))),
                sizes={"dist", "chrom_off", "names_off"}, scratch={"chrom", "names", "text", "ws"},
                check=lambda out, kw: int(out[2][0]) == 0 and bytes(out[0][:int(out[1][R])].tolist()).count(b"\n") == R)


def _bgzf_member(data):
    """One BGZF member holding `data` and its bgzfIndex.members row: payload offset, payload bytes, text offset, ISIZE, CRC-32."""
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = c.compress(data) + c.flush()
    size = 18 + len(raw) + 8
    head = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, (size - 1) & 255, (size - 1) >> 8])
    crc = zlib.crc32(data)
    return head + raw + crc.to_bytes(4, "little") + len(data).to_bytes(4, "little"), [18, len(raw), 0, len(data), crc]


def bgzf_inflate(dev):
    data = b"chr1\t0\t200\t0.5\n" * R
    member, row = _bgzf_member(data)
    return Case(dict(comp=_text(dev, member), table=torch.tensor([row], dtype=torch.int64, device=dev), out=_ws(dev, len(data)),
                     status=_z(dev, 1, torch.int32), flags=_z(dev, 1, torch.int32)), scratch={"comp", "out"},
                check=lambda out, kw: int(out[2][0]) == 0 and bytes(out[0].tolist()) == data)


def newline_index(dev):
    return Case(dict(text=_text(dev, b"0123456\n" * 8), seg_bytes=16, n=64), check=lambda out, kw: out[0].tolist() == [2] * 4)


def null_hist_from_binhist_parts(dev):
    HAs, HBs = _hists(dev)
    return Case(dict(HAs=HAs, HBs=HBs, n_cols=2 * N, S=S, ga=N, gb=N, seed=7, row0s=[0, R]),
                check=lambda out, kw: all(torch.equal(a + b, x + y) for a, b, x, y in zip(out[0], out[1], kw["HAs"], kw["HBs"])))


def null_dist_draws_parts(dev):
    HAs, HBs = _hists(dev)
    return Case(dict(HAs=HAs, HBs=HBs, row0s=[0, R], S=S, NA=N, NB=N, ga=N, gb=N, TnA=_table(dev, N), TnB=_table(dev, N), seeds=[1, 2],
                     masks=[_z(dev, r, torch.uint8) for r in ROWS], outs=[_z(dev, (K, r), torch.float32) for r in ROWS]))


def null_exceed(dev):
    return Case(dict(null=torch.linspace(-1, 1, K * R, dtype=torch.float32, device=dev), d=torch.linspace(0, 1, R, dtype=torch.float32, device=dev),
                     exceed=_z(dev, R, torch.int64), ws=_ws(dev, _engine().null_exceed_ws_bytes(K * R))), sizes={"null", "d"}, scratch={"ws"},
                check=lambda out, kw: int(out[0]) == K * R)


def pair_count_null_parts(dev):
    return Case(dict(XAs=[states(dev, r, seed=1 + r, s=15) for r in ROWS], XBs=[states(dev, r, seed=9 + r, s=15) for r in ROWS], NA=N, NB=N, S=15,
                     seed=7, row0s=[0, R], counts=_z(dev, 15, torch.int64)), pitched={"XAs", "XBs"},
                check=lambda out, kw: all(torch.equal(h, hist(x, s=15)) for h, x in zip(out[0] + out[1], kw["XAs"] + kw["XBs"])))


def hist_s2_from_binhist(dev):
    return Case(dict(H=hist(states(dev)), S=S, counts=_z(dev, S * S, torch.int64)), check=lambda out, kw: int(out.sum()) == R * N * (N - 1))


def hist_s2_from_binhist_pair(dev):
    return Case(dict(HA=hist(states(dev, seed=1)), HB=hist(states(dev, seed=2)), S=S, counts=_z(dev, S * S, torch.int64)),
                check=lambda out, kw: int(out.sum()) == R * 2 * N * (2 * N - 1))


def hist_s3(dev):
    return Case(dict(X=states(dev), N=N, S=S, counts=_z(dev, N * N * S * S, torch.int32), ws=_ws(dev, _engine().hist_s3_ws_bytes(R, N, S))),
                pitched={"X"}, scratch={"ws"}, check=lambda out, kw: int(out.sum()) == R * N * (N - 1))


def normalise(dev):
    return Case(dict(counts=torch.tensor([1, 2, 5], dtype=torch.int64, device=dev), q=_z(dev, S, torch.float32), ws=_ws(dev, 256)),
                sizes={"counts"}, scratch={"ws"}, check=lambda out, kw: out.tolist() == [0.125, 0.25, 0.625])


def score_s1(dev):
    return Case(dict(X=states(dev), N=N, S=S, q=_q(dev), ws=_ws(dev, _engine()._scratch_bytes("epg_ws_bytes", 1, R, N, S)), **_outs(dev)), pitched={"X"},
                scratch={"ws"})


def score_s1_from_binhist(dev):
    return Case(dict(H=hist(states(dev)), N=N, S=S, q=_q(dev), ws=_ws(dev, _engine()._scratch_bytes("epg_ws_bytes", 1, 0, N, S)), **_outs(dev)),
                scratch={"ws"})


def score_s1_from_binhist_table(dev):
    H = hist(states(dev))
    return Case(dict(H=H, N=N, S=S, T64=_table(dev, N).double(), T32=_table(dev, N), **_outs(dev)),
                check=lambda out, kw: torch.equal(out[0], kw["T32"][kw["H"].long(), torch.arange(S, device=kw["H"].device)]))


def combine_score_s1(dev):
    return Case(dict(counts=torch.tensor([1, 2, 5], dtype=torch.int64, device=dev), H=hist(states(dev)), N=N, S=S, q=_z(dev, S, torch.float32),
                     ws=_ws(dev, _engine()._scratch_bytes("epg_ws_bytes", 1, 0, N, S)), **_outs(dev)), scratch={"ws"},
                check=lambda out, kw: out[0].tolist() == [0.125, 0.25, 0.625])


def s1_tables(dev):
    return Case(dict(counts=torch.tensor([1, 2, 5], dtype=torch.int64, device=dev), N=N, S=S, q=_z(dev, S, torch.float32),
                     ws=_ws(dev, _engine()._scratch_bytes("epg_ws_bytes", 1, 0, N, S))), scratch={"ws"},
                check=lambda out, kw: out[0].tolist() == [0.125, 0.25, 0.625] and out[2].numel() == (N + 1) * S)


def score_s2(dev):
    return Case(dict(X=states(dev), N=N, S=S, q=_q(dev, S * S)), pitched={"X"})


def score_s2_from_binhist(dev):
    return Case(dict(H=hist(states(dev)), N=N, S=S, q=_q(dev, S * S), ws=_ws(dev, _engine()._scratch_bytes("epg_ws_bytes", 2, 0, N, S)), **_outs(dev)),
                scratch={"ws"})


def score_s3(dev):
    return Case(dict(X=states(dev), N=N, S=S, q=_q(dev, N * N * S * S), ws=_ws(dev, _engine()._scratch_bytes("epg_ws_bytes", 3, R, N, S))), pitched={"X"},
                scratch={"ws"})


def pair_scores_s1_from_binhist(dev):
    HA, HB = hist(states(dev, seed=1)), hist(states(dev, seed=2))
    return Case(dict(HA=HA, HB=HB, HnA=HB.clone(), HnB=HA.clone(), S=S, NA=N, NB=N, ga=N, gb=N, **_tables(dev)),
                check=lambda out, kw: torch.equal(out[0], kw["TA"][kw["HA"].long(), torch.arange(S, device=out[0].device)]
                                                  - kw["TB"][kw["HB"].long(), torch.arange(S, device=out[0].device)]))


def pair_scores_s1_parts(dev):
    HAs, HBs = _hists(dev)
    return Case(dict(parts=[(a, b, b.clone(), a.clone()) for a, b in zip(HAs, HBs)], S=S, NA=N, NB=N, ga=N, gb=N, qstate=0, **_tables(dev)),
                check=lambda out, kw: [tuple(o["delta"].shape) for o in out] == [(r, S) for r in ROWS])


def pair_finish(dev):
    a = torch.arange(R * S, dtype=torch.float32, device=dev).view(R, S)
    return Case(dict(a=a, b=a.flip(0).contiguous()), sizes={"a"}, check=lambda out, kw: torch.equal(out[0], kw["a"] - kw["b"]))


def pair_metrics(dev):
    return Case(dict(delta=torch.arange(R * S, dtype=torch.float32, device=dev).view(R, S) / 4), sizes={"delta"},
                check=lambda out, kw: out[1].tolist() == [S] * R)


def quiescent(dev):
    XA, XB = states(dev, seed=1), states(dev, seed=2)
    XA[0, :N], XB[0, :N] = 0, 0
    return Case(dict(XA=XA, NA=N, XB=XB, NB=N, qstate=0), pitched={"XA", "XB"}, check=lambda out, kw: int(out[0]) == 1)


def null_hist(dev):
    return Case(dict(XA=states(dev, seed=1), NA=N, XB=states(dev, seed=2), NB=N, S=S, ga=N, gb=N, seed=7), pitched={"XA", "XB"},
                check=lambda out, kw: torch.equal(out[0] + out[1], hist(kw["XA"]) + hist(kw["XB"])))


def quiescent_from_binhist(dev):
    XA, XB = states(dev, seed=1), states(dev, seed=2)
    XA[0, :N], XB[0, :N] = 0, 0
    return Case(dict(HA=hist(XA), NA=N, HB=hist(XB), NB=N, S=S, qstate=0), check=lambda out, kw: out.tolist() == [1] + [0] * (R - 1))


def null_hist_from_binhist(dev):
    return Case(dict(HA=hist(states(dev, seed=1)), HB=hist(states(dev, seed=2)), n_cols=2 * N, S=S, ga=N, gb=N, seed=7),
                check=lambda out, kw: torch.equal(out[0] + out[1], kw["HA"] + kw["HB"]))


def simsearch(dev):
    g = _grid(dev)
    return Case(dict(g=g, W=W, q=torch.stack([g[0:W], g[8:8 + W]]).contiguous(), self_start=torch.tensor([0, 8], dtype=torch.int32, device=dev), n=3,
                     key_bound=W * S * 81, ws=_ws(dev, _engine().simsearch_ws_bytes(G, S, W, 2)), want_dist=True), sizes={"g", "self_start"},
                scratch={"ws"}, check=lambda out, kw: int(out[2][0, 0]) == 0 and int(out[2][1, 8]) == 0)


def simsearch_reduce(dev):
    return Case(dict(x=_grid(dev), blockSize=2), sizes={"x"}, check=lambda out, kw: tuple(out.shape) == (G // 2, S))


def simsearch_slices(dev):
    return Case(dict(x=_grid(dev), first=np.array([0, 4], dtype=np.int64), nblk=2, blockSize=2), sizes={"x"},
                check=lambda out, kw: tuple(out.shape) == (2, 2, S))


def simsearch_rowscore(dev):
    return Case(dict(x=_grid(dev)), sizes={"x"}, check=lambda out, kw: torch.allclose(out, kw["x"].double().sum(1) / 1e5, rtol=1e-12, atol=0))


def _keys(dev):
    return torch.from_numpy(np.random.default_rng(6).permutation(G).astype(np.float64)).to(dev)


def simsearch_rolling_max(dev):
    return Case(dict(v=_keys(dev), W=W), sizes={"v"}, check=lambda out, kw: float(out[W // 2]) == float(kw["v"][:W].max()))


def simsearch_rank(dev):
    k = _keys(dev)
    return Case(dict(rmax=k, rmean=k.clone(), score=k.clone()), sizes={"rmax"}, check=lambda out, kw: out.long().tolist() == (G - 1 - kw["rmax"]).long().tolist())


def simsearch_pick(dev):
    return Case(dict(rank=torch.arange(G, dtype=torch.int32, device=dev), W=W, maxRegions=G // W), sizes={"rank"},
                check=lambda out, kw: out[0][:int(out[1][0])].tolist() == [0, 4, 8, 12])


def scores_parse(dev):
    eng = _engine()
    data = b"".join(b"chr1\t%d\t%d\t0.5\t1.0\t-0.25\n" % (200 * r, 200 * r + 200) for r in range(R))
    return Case(dict(text=_text(dev, data), nbytes=len(data), F=S + 3, rows=R, row0=0, x=_z(dev, (R, S), torch.int32), start=_z(dev, R, torch.int64),
                     end=_z(dev, R, torch.int64), chrom_at=_z(dev, R, torch.int32), ws=_ws(dev, eng.scores_ws_bytes(len(data))),
                     status=torch.tensor([2 ** 63 - 1, 0], dtype=torch.int64, device=dev)), scratch={"ws"},
                check=lambda out, kw: kw["x"].tolist() == [[50000, 100000, -25000]] * R and kw["status"].tolist() == [2 ** 63 - 1, R])


TABLE = {f.__name__: f for f in (
    bin_hist, bin_hist_s2, bin_hist_parts, bin_hist_groups, state_census, concordance, gennorm_fit, gennorm_nnlf, gennorm_pvals, bh_adjust,
    format_scores, bgzf_compress, format_metrics, bgzf_inflate, newline_index, null_hist_from_binhist_parts, null_dist_draws_parts, null_exceed,
    pair_count_null_parts, hist_s2_from_binhist, hist_s2_from_binhist_pair, hist_s3, normalise, score_s1, score_s1_from_binhist,
    score_s1_from_binhist_table, combine_score_s1, s1_tables, score_s2, score_s2_from_binhist, score_s3, pair_scores_s1_from_binhist,
    pair_scores_s1_parts, pair_finish, pair_metrics, quiescent, null_hist, quiescent_from_binhist, null_hist_from_binhist, simsearch,
    simsearch_reduce, simsearch_slices, simsearch_rowscore, simsearch_rolling_max, simsearch_rank, simsearch_pick, scores_parse)}

# engine functions that hold an _abi.call and are no wrapper of a kernel entry point: the size query every wrapper's scratch goes through
NOT_WRAPPERS = {"_scratch_bytes"}
