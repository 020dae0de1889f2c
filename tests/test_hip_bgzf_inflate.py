"""GPU: the device BGZF reader (csrc/epg_bgzf_inflate.h).  The judge is never the code under test: every member's text is held against
zlib's, the newline index against numpy.  The streams are those of tests/bgzf_streams.py, which tests/test_inflate_host.py runs through
the host program (the same phases, under the sanitizers, verdicts held against zlib) before anything here runs them on the device.
The arena and stream cases follow tests/test_hip_textout.py: exact-size buffers between guards, dirty outputs, side stream, capture and
two replays.  A workgroup serves exactly one member, so there is no second member of a workgroup to pin."""
import gzip
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from epilogos_amd import _io, bgzfIndex
from tests import bgzf_streams as bs
from tests.test_hip_abi_contract import I32, I64, U8, Spec, run_case
from tests.test_hip_abi_streams import stream_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from epilogos_amd import engine
    engine.require_gpu()
    return engine


@pytest.fixture(scope="module")
def abi():
    from epilogos_amd import _abi, engine
    engine.require_gpu()
    return _abi


@pytest.fixture(scope="module")
def text():
    return bs.score_text(600)[:65280]


@pytest.fixture(scope="module")
def good(text):
    return bs.good_members(text)


@pytest.fixture(scope="module")
def bad(text):
    return bs.bad_members(text)


def layout(members, order=None, gap=3):
    """(comp bytes, table int64 [M, 5], total text bytes): the payloads back to back with `gap` bytes between them, the texts in the
    order of `members`, the table's rows in `order`."""
    comp, rows, at = bytearray(b"\xEE" * gap), [], 0
    for m in members:
        rows.append((len(comp), len(m.payload), at, m.isize, m.crc))
        comp += m.payload + b"\xEE" * gap
        at += m.isize
    table = np.asarray(rows, dtype=I64).reshape(-1, 5)
    return bytes(comp), table if order is None else table[order], at


def inflate(eng, members, order=None):
    comp, table, total = layout(members, order)
    out = torch.full((total + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    o, status, flags = eng.bgzf_inflate(torch.from_numpy(np.frombuffer(comp, dtype=U8).copy()).cuda(), torch.from_numpy(table).cuda(), out=out[:total])
    torch.cuda.synchronize()
    assert bool((out[total:] == 0xAB).all())
    return o.cpu().numpy().tobytes(), status.cpu().numpy(), int(flags[0])


def test_every_kind_of_stream(eng, good):
    for name, (m, want) in good.items():
        assert zlib.decompressobj(-15).decompress(m.payload) == want
        got, status, flags = inflate(eng, [m])
        assert list(status) == [0] and flags == 0 and got == want, name


def test_three_hundred_mixed_members_in_shuffled_order(eng, good):
    rng = np.random.default_rng(11)
    names = [n for n in good if good[n][0].isize <= 4000 or n in ("level 6", "stored", "65536 equal bytes", "fibonacci")]
    small = {n: good[n] for n in names}
    for k in range(24):                                                        # short members of every length around the 16-byte chunks
        t = bs.score_text(3, seed=100 + k)[:17 * k + 1]
        small["short %d" % k] = (bs.deflate(t, [1, 6, 9][k % 3], [zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED][k % 2]), t)
    pick = [list(small)[i] for i in rng.integers(0, len(small), 300)]
    members = [small[n][0] for n in pick]
    want = b"".join(small[n][1] for n in pick)
    order = rng.permutation(len(members))
    got, status, flags = inflate(eng, members, order)
    assert flags == 0 and not status.any() and got == want


def test_the_projects_own_files(eng, tmp_path, monkeypatch):
    """The host writer's BGZF (its own DEFLATE, and zlib level 6), the device writer's stream, simsearch.bed.gz's compressor."""
    from epilogos_amd import similaritySearch_write as ssw
    from tests.test_hip_textout import locations
    R = 3000
    x = np.random.default_rng(3).normal(0, 0.3, size=(R, 18)).astype(np.float32)
    loc = locations(R, "chr1")
    blobs = {}
    monkeypatch.setenv("EPILOGOS_BGZF", "1")
    _io.write_scores(tmp_path / "own.txt.gz", loc, x)
    blobs["host writer"] = (tmp_path / "own.txt.gz").read_bytes()
    monkeypatch.setenv("EPILOGOS_GZIP_LEVEL", "6")
    _io.write_scores(tmp_path / "six.txt.gz", loc, x)
    blobs["host writer, level 6"] = (tmp_path / "six.txt.gz").read_bytes()
    want = gzip.decompress(blobs["host writer"])
    got = eng.scores_text_bgzf(loc, torch.from_numpy(x).cuda(), eof=True)
    blobs["device writer"] = got[0][:got[1]].cpu().numpy().tobytes()
    blobs["simsearch"] = ssw.bgzf_compress(want)[0]
    for name, blob in blobs.items():
        assert gzip.decompress(blob) == want, name
        table, total = bgzfIndex.members(blob)
        assert total == len(want) and len(table) == -(-len(want) // 65280) + 1
        o, status, flags = eng.bgzf_inflate(torch.from_numpy(np.frombuffer(blob, dtype=U8).copy()).cuda(), torch.from_numpy(table).cuda())
        torch.cuda.synchronize()
        assert int(flags[0]) == 0 and not bool(status.any()) and o[:total].cpu().numpy().tobytes() == want, name
    eng.release_text_buffers()


def s_inflate(abi, members, texts, reasons, order):
    """The call in the guarded arena: comp, table and out exactly sized and off their alignment; a member that is given up leaves
    zeros, its neighbours their text."""
    comp, table, total = layout(members, order)
    M = len(members)
    sp = Spec(18)
    sp.inp("comp", np.frombuffer(comp, dtype=U8), mis=3)
    sp.inp("table", table, mis=8)
    sp.out("out", U8, total, mis=5)
    sp.out("status", I32, M, mis=4)
    sp.out("flags", I32, 1, mis=4)
    sp.call = lambda abi, P, st: abi.call("epgz_bgzf_inflate", P["comp"], len(comp), P["table"], M, P["out"], total, P["status"], P["flags"], st)
    want = b"".join(t if r == 0 else b"\0" * m.isize for m, t, r in zip(members, texts, reasons))

    def verify(o):
        assert list(o["status"]) == [reasons[k] for k in order], (list(o["status"]), [reasons[k] for k in order])
        assert list(o["flags"]) == [sum(1 for r in reasons if r)]
        assert o["out"].tobytes() == want
    sp.verify = verify
    return sp


def test_inflate_contract_and_streams(abi, good):
    names = ["level 6", "single distance code", "stored", "one byte", "end-of-file block", "Z_FIXED", "full flush", "no distance code"]
    members, texts = [good[n][0] for n in names], [good[n][1] for n in names]
    order = np.random.default_rng(5).permutation(len(names))
    run_case(s_inflate(abi, members, texts, [0] * len(names), order), abi)
    stream_case(s_inflate(abi, members, texts, [0] * len(names), order), abi)


def test_every_corruption_among_good_members(abi, good, bad):
    """One call: every bad member between good ones, rows shuffled.  The bad one's status is its reason, its bytes are zeros, the
    neighbours are intact, flags[0] counts them, and no byte outside the named ranges changes (the arena)."""
    fill = ["one byte", "literals only", "single distance code", "level 1"]
    members, texts, reasons = [], [], []
    for k, (name, (m, why)) in enumerate(bad.items()):
        g = good[fill[k % len(fill)]]
        members += [g[0], m]
        texts += [g[1], None]
        reasons += [0, why]
    members.append(good["level 9"][0])
    texts.append(good["level 9"][1])
    reasons.append(0)
    order = np.random.default_rng(6).permutation(len(members))
    run_case(s_inflate(abi, members, texts, reasons, order), abi)


def test_rows_the_kernel_refuses(eng, good):
    m, want = good["level 1"]
    comp, table, total = layout([m, m, m, m, m, m])
    table[1, 0] = len(comp) - 5                                                # the payload reaches beyond comp
    table[2, 2] = total - 10                                                   # the text reaches beyond out
    table[3, 3] = 65537
    table[4, 1] = -1
    table[5, 4] = 1 << 32
    out = torch.full((total + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    _o, status, flags = eng.bgzf_inflate(torch.from_numpy(np.frombuffer(comp, dtype=U8).copy()).cuda(), torch.from_numpy(table).cuda(), out=out[:total])
    torch.cuda.synchronize()
    assert list(status.cpu().numpy()) == [0, 1, 1, 1, 1, 1] and int(flags[0]) == 5
    got = out.cpu().numpy()
    assert got[:len(want)].tobytes() == want and bool((got[len(want):] == 0xAB).all())
    empty = eng.bgzf_inflate(torch.zeros(0, dtype=torch.uint8, device="cuda"), torch.zeros((0, 5), dtype=torch.int64, device="cuda"))
    torch.cuda.synchronize()
    assert int(empty[2][0]) == 0 and empty[1].numel() == 0                     # M = 0 is a valid call


# ---- the newline index -------------------------------------------------------------------------------------------------------------
def index_ref(a, seg):
    nseg = -(-len(a) // seg)
    count, last = np.zeros(nseg, dtype=I64), np.full(nseg, -1, dtype=I64)
    for s in range(nseg):
        nl = np.flatnonzero(a[s * seg:(s + 1) * seg] == 10)
        count[s] = len(nl)
        if len(nl):
            last[s] = s * seg + nl[-1]
    return count, last


def newline_cases():
    rng = np.random.default_rng(8)
    cases = {"n = 0": (np.zeros(0, dtype=U8), 64), "n = 1, a newline": (np.array([10], dtype=U8), 16), "n = 1, no newline": (np.array([7], dtype=U8), 16)}
    a = rng.integers(32, 127, 1000).astype(U8)                                 # no newline at all, then one per place that matters
    cases["a segment without a newline"] = (a.copy(), 64)
    b = a.copy()
    b[[63, 64, 127, 200, 999]] = 10                                            # the last byte of a segment and the first of the next
    cases["newlines at the borders, n no multiple"] = (b, 64)
    t = np.frombuffer(bs.score_text(900, seed=9), dtype=U8)
    cases["score text, 4096"] = (t, 4096)
    cases["score text, 16"] = (t[:5001], 16)
    cases["only newlines"] = (np.full(3 * 1024 + 5, 10, dtype=U8), 1024)
    return cases


@pytest.mark.parametrize("name", list(newline_cases()))
def test_newline_index(eng, name):
    a, seg = newline_cases()[name]
    text = torch.from_numpy(a.copy()).cuda() if len(a) else torch.zeros(0, dtype=torch.uint8, device="cuda")
    count, last = eng.newline_index(text, seg)
    torch.cuda.synchronize()
    want = index_ref(a, seg)
    assert np.array_equal(count.cpu().numpy(), want[0]) and np.array_equal(last.cpu().numpy(), want[1])


def s_newline(abi, a, seg):
    nseg = -(-len(a) // seg)
    sp = Spec(18)
    sp.inp("text", a, align=16)                                               # exactly n bytes: the last chunk's 16-byte load would reach the guard
    sp.out("count", I64, nseg, mis=8)
    sp.out("last", I64, nseg, mis=8)
    sp.call = lambda abi, P, st: abi.call("epgz_newline_index", P["text"], len(a), seg, P["count"], P["last"], st)
    want = index_ref(a, seg)

    def verify(o):
        assert np.array_equal(o["count"], want[0]) and np.array_equal(o["last"], want[1])
    sp.verify = verify
    return sp


def test_newline_index_contract_and_streams(abi):
    a, seg = newline_cases()["score text, 4096"]
    a = a[:len(a) - len(a) % 16 + 7]
    run_case(s_newline(abi, a, seg), abi)
    stream_case(s_newline(abi, a, seg), abi)
