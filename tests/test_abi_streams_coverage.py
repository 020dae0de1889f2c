"""No GPU: every prototype of the headers under include/ whose last parameter is `void* stream` has a case in
tests/test_hip_abi_streams.py that goes through the stream capture, or an entry in its EXEMPT with a reason that the function's own
header comment backs (it says that the call synchronises).  A new entry point that takes a stream fails here, before it reaches
a GPU; so does a case for a name no header declares."""
import re
import shutil
from pathlib import Path

import pytest

pytest.importorskip("torch")

INCLUDE = Path(__file__).resolve().parents[1] / "include"
STREAM_LAST = re.compile(r"void\s*\*\s*stream$")


def stream_prototypes(include=INCLUDE):
    """name -> the comment in front of the prototype, for every prototype of every header whose last parameter is the stream."""
    out = {}
    for path in sorted(Path(include).glob("*.h")):
        text = path.read_text()
        comments = [(m.start(), m.end()) for m in re.finditer(r"/\*.*?\*/", text, flags=re.S)]
        code = list(text)
        for a, b in comments:                                                  # blank the comments, keep every offset
            code[a:b] = " " * (b - a)
        code = "".join(code)
        for m in re.finditer(r"\b(epgt?_[a-z0-9_]+)\s*\(([^;()]*)\)\s*;", code):
            params = [p.strip() for p in " ".join(m.group(2).split()).split(",")]
            if not STREAM_LAST.search(params[-1]):
                continue
            before = [(a, b) for a, b in comments if b <= m.start() and ";" not in code[b:m.start()] and "#" not in code[b:m.start()]]
            assert m.group(1) not in out, "%s is declared twice" % m.group(1)
            out[m.group(1)] = text[before[-1][0]:before[-1][1]] if before else ""
    return out


def coverage_gaps(include=INCLUDE):
    """-> the list of what is wrong, empty when every stream-taking prototype is covered."""
    from tests.test_hip_abi_streams import CASES, EXEMPT, OTHERS, captured_entry_points
    protos, covered, gaps = stream_prototypes(include), captured_entry_points(), []
    with_case = {c.values[0] for c in list(CASES) + list(OTHERS)}
    for name in sorted(protos):
        if name in EXEMPT:
            if not EXEMPT[name].strip():
                gaps.append("%s is exempt without a reason" % name)
            if "synchronis" not in protos[name]:
                gaps.append("%s is exempt, but its header comment does not say that it synchronises" % name)
            if name not in with_case:
                gaps.append("%s is exempt from the capture and has no case for the side stream either" % name)
        elif name not in covered:
            gaps.append("%s takes a stream and has neither a capture case nor an exemption" % name)
    for name in sorted((covered | set(EXEMPT)) - set(protos)):
        gaps.append("%s has a case or an exemption, but no header declares it with a stream" % name)
    return gaps


def test_the_headers_are_parsed():
    protos = stream_prototypes()
    assert len(protos) >= 44 and len(list(INCLUDE.glob("*.h"))) >= 10          # 30 of epilogos_amd.h, 14 of the eight newer headers
    assert {"epg_bin_hist", "epg_simsearch_slices", "epgt_scores_parse", "epg_seg_expand", "epg_concordance"} <= set(protos)
    assert not {"epg_ws_bytes", "epg_test_force", "epg_sbl_constant"} & set(protos)                 # no stream: nothing to enqueue
    assert "Launches and synchronisations" in protos["epg_simsearch_pick"] and "EPG_ERR_WORKSPACE" in protos["epg_concordance"]


def test_every_prototype_that_takes_a_stream_has_a_capture_case_or_a_documented_exemption():
    assert coverage_gaps() == []


@pytest.fixture
def scratch(tmp_path):
    shutil.copytree(INCLUDE, tmp_path / "include")
    return tmp_path / "include"


def _append(header, prototype):
    text = header.read_text()
    at = text.rindex("#ifdef __cplusplus")
    header.write_text(text[:at] + prototype + "\n\n" + text[at:])


@pytest.mark.parametrize("header", ["epilogos_amd.h", "epilogos_census.h", "epilogos_segments.h"])
def test_a_new_prototype_without_a_case_is_reported(scratch, header):
    _append(scratch / header, "/* A new entry point. */\nint epg_brand_new(const int8_t* X, int64_t R,\n                  void* stream);")
    assert coverage_gaps(scratch) == ["epg_brand_new takes a stream and has neither a capture case nor an exemption"]


def test_an_exemption_needs_the_headers_word_and_a_case_needs_a_header(scratch, monkeypatch):
    from tests import test_hip_abi_streams as ts
    monkeypatch.setitem(ts.EXEMPT, "epg_simsearch_rank", "it is slow")          # the header documents no synchronisation of it
    assert coverage_gaps() == ["epg_simsearch_rank is exempt, but its header comment does not say that it synchronises"]
    monkeypatch.setattr(ts, "OTHERS", [c for c in ts.OTHERS if c.values[0] != "epg_simsearch_pick"])
    assert coverage_gaps()[0] == "epg_simsearch_pick is exempt from the capture and has no case for the side stream either"
    monkeypatch.undo()
    monkeypatch.setitem(ts.EXEMPT, "epg_gone", "synchronises")
    assert coverage_gaps() == ["epg_gone has a case or an exemption, but no header declares it with a stream"]
    monkeypatch.delitem(ts.EXEMPT, "epg_gone")
    text = (scratch / "epilogos_statebyline.h").read_text()                     # a case whose prototype has left the header
    (scratch / "epilogos_statebyline.h").write_text(re.sub(r"int epg_sbl_transpose\([^;]*;", "", text))
    assert coverage_gaps(scratch) == ["epg_sbl_transpose has a case or an exemption, but no header declares it with a stream"]
