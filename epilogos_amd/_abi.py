"""ctypes binding of the public headers under include/ (build.PUBLIC_HEADERS): one table of prototypes per header, all in the
registry HEADERS.  No fallbacks: a missing library or symbol raises."""
import ctypes as C
import re
from collections import namedtuple
from pathlib import Path

from . import build as _build

EPG_OK = 0
ERR_NAMES = {-1: "EPG_ERR_INVALID_ARG", -2: "EPG_ERR_UNSUPPORTED", -3: "EPG_ERR_HIP", -4: "EPG_ERR_WORKSPACE"}


class EpilogosHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s (%d): %s" % (ERR_NAMES.get(code, "EPG_ERR"), code, msg))
        self.code = code


_p = C.c_void_p
_i64 = C.c_int64
_i32 = C.c_int32
_u64 = C.c_uint64

# header -> {name: (restype, argtypes)}, keyed like build.PUBLIC_HEADERS; every table must list every prototype of its header and no
# name twice (tests/test_abi_symbols.py checks both, for every header)
_TABLES = {
    "core": {
        "epg_version": (C.c_int, []),
        "epg_last_error": (C.c_char_p, []),
        "epg_device_cus": (C.c_int, []),
        "epg_bin_hist": (C.c_int, [_p, _i64, _i32, _i64, _i32, _p, _p, _p]),
        "epg_bin_hist_s2": (C.c_int, [_p, _i64, _i32, _i64, _i32, _p, _p, _p, _p]),
        "epg_bin_hist_parts": (C.c_int, [_i32, _p, _p, _p, _p, _i32, _p, _p, _p]),
        "epg_hist_s1": (C.c_int, [_p, _i64, _i32, _i64, _i32, _p, _p]),
        "epg_hist_s2": (C.c_int, [_p, _i64, _i32, _i64, _i32, _p, _p, _i64, _p]),
        "epg_hist_s2_from_binhist": (C.c_int, [_p, _i64, _i32, _p, _p]),
        "epg_hist_s2_from_binhist_pair": (C.c_int, [_p, _p, _i64, _i32, _p, _p]),
        "epg_combine_score_s1": (C.c_int, [_p, _i32, _p, _i64, _i32, _i32, _p, _p, _p, _p, _i64, _p]),
        "epg_hist_s3": (C.c_int, [_p, _i64, _i32, _i64, _i32, _p, _p, _i64, _p]),
        "epg_normalise_i64": (C.c_int, [_p, _i64, _p, _p, _i64, _p]),
        "epg_normalise_i32": (C.c_int, [_p, _i64, _p, _p, _i64, _p]),
        "epg_ws_bytes": (_i64, [_i32, _i64, _i32, _i32]),
        "epg_score_s1": (C.c_int, [_p, _i64, _i32, _i64, _i32, _p, _p, _p, _p, _i64, _p]),
        "epg_score_s1_from_binhist": (C.c_int, [_p, _i64, _i32, _i32, _p, _p, _p, _p, _i64, _p]),
        "epg_score_s1_from_binhist_table": (C.c_int, [_p, _i64, _i32, _i32, _p, _p, _p, _p, _p]),
        "epg_pair_scores_s1_from_binhist": (C.c_int, [_p, _p, _p, _p, _i64, _i32, _i32, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
        "epg_pair_scores_s1_parts": (C.c_int, [_i32, _p, _p, _p, _p, _p, _i32, _i32, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i32, _p]),
        "epg_score_s2": (C.c_int, [_p, _i64, _i32, _i64, _i32, _i64, _p, _p, _p, _p, _i64, _p]),
        "epg_score_s2_from_binhist": (C.c_int, [_p, _i64, _i32, _i32, _i64, _p, _p, _p, _p, _i64, _p]),
        "epg_score_s3": (C.c_int, [_p, _i64, _i32, _i64, _i32, _p, _p, _p, _p, _i64, _p]),
        "epg_pair_finish": (C.c_int, [_p, _p, _i64, _i32, _p, _p, _p]),
        "epg_pair_metrics": (C.c_int, [_p, _i64, _i32, _i32, _p, _p, _p]),
        "epg_quiescent": (C.c_int, [_p, _i32, _i64, _p, _i32, _i64, _i64, _i32, _p, _p]),
        "epg_null_hist": (C.c_int, [_p, _i32, _i64, _p, _i32, _i64, _i64, _i32, _i32, _i32, _u64, _i64, _p, _p, _p]),
        "epg_quiescent_from_binhist": (C.c_int, [_p, _p, _i64, _i32, _i32, _i32, _i32, _p, _p]),
        "epg_null_hist_from_binhist": (C.c_int, [_p, _p, _i64, _i32, _i32, _i32, _i32, _u64, _i64, _p, _p, _p]),
        "epg_null_hist_from_binhist_parts": (C.c_int, [_i32, _p, _p, _p, _i32, _i32, _i32, _i32, _u64, _p, _p, _p, _p]),
        "epg_pair_count_null_parts": (C.c_int, [_i32, _p, _p, _p, _i32, _i32, _p, _p, _i32, _p, _p, _p, _u64, _p, _p, _p, _p]),
        "epg_simsearch_ws_bytes": (_i64, [_i64, _i32, _i32, _i32]),
        "epg_simsearch": (C.c_int, [_p, _i64, _i32, _i32, _p, _i32, _p, _i32, _u64, _p, _i64, _p, _p, _p, _p]),
        "epg_simsearch_reduce": (C.c_int, [_p, _i64, _i32, _i32, _p, _p, _p]),
        "epg_simsearch_slices": (C.c_int, [_p, _i64, _i32, _i32, _i32, _p, _i32, _p, _p]),
        "epg_test_force": (C.c_int, [_i32, _i32]),
    },
    "scores_text": {                                      # the GPU scores-text parser
        "epgt_scores_ws_bytes": (_i64, [_i64]),
        "epgt_scores_parse": (C.c_int, [_p, _i64, _i32, _i64, _i64, _p, _p, _p, _p, _p, _i64, _p, _p]),
    },
    "groups": {                                           # the column-group count pass
        "epg_bin_hist_groups": (C.c_int, [_p, _i64, _i32, _i64, _i32, _i32, _p, _p, _p, _p]),
    },
    "nulldraws": {                                        # the K-draw null of paired mode
        "epg_null_dist_draws_parts": (C.c_int, [_i32, _p, _p, _p, _p, _p, _i32, _i32, _i32, _i32, _i32, _p, _p, _p, _i32, _p, _p]),
        "epg_null_exceed_ws_bytes": (_i64, [_i64]),
        "epg_null_exceed": (C.c_int, [_p, _i64, _p, _i64, _p, _p, _i64, _p]),
    },
    "statebyline": {                                      # the reader of ChromHMM state-by-line calls
        "epg_sbl_ws_bytes": (_i64, [_i64]),
        "epg_sbl_constant": (_i32, [_i32]),
        "epg_sbl_parse": (C.c_int, [_p, _i64, _p, _i64, _p, _p, _i64, _p]),
        "epg_sbl_transpose": (C.c_int, [_p, _i32, _i64, _i64, _p, _i64, _i64, _p]),
    },
    "segments": {                                         # the reader of ChromHMM segment files
        "epg_seg_ws_bytes": (_i64, [_i64, _i32]),
        "epg_seg_constant": (_i32, [_i32]),
        "epg_seg_parse": (C.c_int, [_p, _i64, _p, _i32, _i32, _p, _p, _i64, _p, _p, _p, _i64, _p]),
        "epg_seg_expand": (C.c_int, [_p, _p, _p, _i32, _p, _i64, _p]),
    },
    "simsearch_pick": {                                   # the device STEP 1 of simsearch -b
        "epg_simsearch_rowscore": (C.c_int, [_p, _i64, _i32, _p, _p]),
        "epg_simsearch_rolling_max": (C.c_int, [_p, _i64, _i32, _p, _p]),
        "epg_simsearch_rank_ws_bytes": (_i64, [_i64]),
        "epg_simsearch_rank": (C.c_int, [_p, _p, _p, _i64, _p, _p, _i64, _p]),
        "epg_simsearch_pick_ws_bytes": (_i64, [_i64, _i32]),
        "epg_simsearch_pick": (C.c_int, [_p, _i64, _i32, _i64, _p, _p, _p, _p, _i64, _p]),
    },
    "census": {                                           # the per-biosample state census
        "epg_state_census": (C.c_int, [_p, _i64, _i32, _i64, _i32, _p, _p, _p, _p]),
    },
    "concordance": {                                      # the pairwise state agreement of biosample columns
        "epg_concordance_ws_bytes": (_i64, [_i64, _i32, _i32]),
        "epg_concordance": (C.c_int, [_p, _i64, _i32, _i64, _i32, _p, _p, _p, _i64, _p]),
    },
    "gennorm": {                                          # the device fit of the paired null distribution
        "epgf_gennorm_ws_bytes": (_i64, [_i64, _i32, _i64]),
        "epgf_gennorm_fit": (C.c_int, [_p, _i64, _p, _i32, _i64, _p, _p, _p, _p, _i64, _p]),
        "epgf_gennorm_nnlf": (C.c_int, [_p, _i64, _p, _i32, _p, _p, _i64, _p]),
    },
}

Header = namedtuple("Header", "path prototypes")
assert list(_TABLES) == list(_build.PUBLIC_HEADERS)
HEADERS = {which: Header(_build.ROOT / "include" / name, _TABLES[which]) for which, name in _build.PUBLIC_HEADERS.items()}
HEADER, PROTOTYPES = HEADERS["core"]

# package-internal entry points (build.INTERNAL_HEADERS): exported by the same library and bound by load() like the public ones, but
# declared under csrc/ and outside the registry above, whose ten headers and their names the binding tests pin.  csrc/epg_pvals.h
# says what promotes a header from here to HEADERS.  The device text writer's table ("textout", csrc/epg_textout.h, prefix epgw_) is
# package-internal in the same way and bound through WRITER (build.WRITER_HEADERS): INTERNAL stays the p-value stage's alone, as
# tests/test_pvals_host.py pins it.  The device BGZF reader's table ("bgzf_inflate", csrc/epg_bgzf_inflate.h, prefix epgz_) is bound
# through READER (build.READER_HEADERS) for the same reason: tests/test_writer_host.py pins WRITER to the text writer alone.
_INTERNAL_TABLES = {
    "pvals": {                                            # p-values and Benjamini-Hochberg of paired mode with -n
        "epgf_gennorm_pvals": (C.c_int, [_p, _i64, _p, _p, _p, _p]),
        "epgf_bh_ws_bytes": (_i64, [_i64]),
        "epgf_bh_adjust": (C.c_int, [_p, _i64, _p, _p, _p, _i64, _p]),
    },
    "textout": {                                          # the device text writer: score text and its BGZF compression
        "epgw_text_bytes_max": (_i64, [_i64, _i32, _i64]),
        "epgw_format_ws_bytes": (_i64, [_i64]),
        "epgw_format_scores": (C.c_int, [_p, _i64, _i32, _i64, _p, _p, _p, _i64, _p, _p, _p, _i64, _p]),
        "epgw_bgzf_bytes_max": (_i64, [_i64, _i32]),
        "epgw_bgzf_ws_bytes": (_i64, [_i64]),
        "epgw_bgzf_compress": (C.c_int, [_p, _i64, _p, _i64, _i32, _p, _i64, _p, _p, _p, _i64, _p]),
    },
    "bgzf_inflate": {                                     # the device BGZF reader: members inflated, the text's newline index
        "epgz_inflate_lds_bytes": (_i64, []),
        "epgz_bgzf_inflate": (C.c_int, [_p, _i64, _p, _i64, _p, _i64, _p, _p, _p]),
        "epgz_newline_segments": (_i64, [_i64, _i64]),
        "epgz_newline_index": (C.c_int, [_p, _i64, _i64, _p, _p, _p]),
    },
}
assert list(_INTERNAL_TABLES) == [*_build.INTERNAL_HEADERS, *_build.WRITER_HEADERS, *_build.READER_HEADERS]
INTERNAL = {which: Header(_build.CSRC / name, _INTERNAL_TABLES[which]) for which, name in _build.INTERNAL_HEADERS.items()}
WRITER = {which: Header(_build.CSRC / name, _INTERNAL_TABLES[which]) for which, name in _build.WRITER_HEADERS.items()}
READER = {which: Header(_build.CSRC / name, _INTERNAL_TABLES[which]) for which, name in _build.READER_HEADERS.items()}

# the device metrics writer's table ("metrics_text", csrc/epg_metrics_text.h, prefix epgm_), bound through METRICS
# (build.METRICS_HEADERS).  A table dictionary of its own: tests/test_inflate_host.py pins the keys of _INTERNAL_TABLES to the three
# registries above
_METRICS_TABLES = {
    "metrics_text": {                                     # pairwiseMetrics rows formatted on the device
        "epgm_text_bytes_max": (_i64, [_i64, _i64, _i64, _i32]),
        "epgm_format_ws_bytes": (_i64, [_i64]),
        "epgm_format_metrics": (C.c_int, [_p, _p, _i32, _i64, _p, _p, _p, _p, _p, _i32, _i64, _p, _p, _p, _p, _i64, _p, _i64, _p, _p, _p, _i64, _p]),
    },
}
assert list(_METRICS_TABLES) == list(_build.METRICS_HEADERS)
METRICS = {which: Header(_build.CSRC / name, _METRICS_TABLES[which]) for which, name in _build.METRICS_HEADERS.items()}

_lib = None


def header_symbols(which="core"):
    """Function names declared in the header `which` of HEADERS (epg_, epgt_ and epgf_ are the prefixes in use)."""
    txt = re.sub(r"/\*.*?\*/", "", HEADERS[which].path.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(epg[tf]?_[a-z0-9_]+)\s*\(", txt)))


def header_constant_of(header, name):
    """The value of `#define name <integer>` of a Header of any registry."""
    m = re.search(r"^#define\s+%s\s+(\d+)" % re.escape(name), header.path.read_text(), flags=re.M)
    if m is None:
        raise RuntimeError("%s not found in %s" % (name, header.path))
    return int(m.group(1))


def header_constant(which, name):
    """The value of `#define name <integer>` of the header `which` of HEADERS."""
    return header_constant_of(HEADERS[which], name)


def pick_header_constant(name):
    """header_constant("simsearch_pick", name).  Test modules of earlier commits read their tile size through this name at import;
    run against this package, as the project's checks do, they have to keep collecting."""
    return header_constant("simsearch_pick", name)


def lib_path():
    """The in-tree library; EPILOGOS_HIP_LIB=<path> loads another build of it (A/B measurements of kernel variants)."""
    import os
    p = os.environ.get("EPILOGOS_HIP_LIB")
    return Path(p) if p else _build.LIB_PATH


ABI_VERSION = header_constant("core", "EPG_ABI_VERSION")      # one source: the header the library is built from


def load():
    """Load libepilogos_hip.so (must have been built: __graft_entry__.build() or python -m epilogos_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own libamdhip64; it must be the HIP runtime of this process BEFORE our library resolves
    # its NEEDED libamdhip64.so.7, otherwise two runtimes coexist and our launches see no device.
    import torch  # noqa: F401
    path = lib_path()
    if not path.exists():
        raise EpilogosHipError(-3, "%s is missing: build it with `python -m epilogos_amd.build` "
                                   "(there is no CPU fallback)" % path)
    lib = C.CDLL(str(path))
    for header in [*HEADERS.values(), *INTERNAL.values(), *WRITER.values(), *READER.values(), *METRICS.values()]:
        for name, (res, args) in header.prototypes.items():
            fn = getattr(lib, name)  # AttributeError if the symbol is missing: fail loudly
            fn.restype = res
            fn.argtypes = args
    if lib.epg_version() != ABI_VERSION:                    # (EPG_ABI_VERSION of include/epilogos_amd.h the library was built from)
        raise EpilogosHipError(-3, "%s has ABI version %d, this package speaks %d: rebuild it with `python -m epilogos_amd.build`"
                               % (path, lib.epg_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(rc):
    if rc < 0:
        raise EpilogosHipError(rc, load().epg_last_error().decode(errors="replace"))
    return rc


def call(name, *args):
    return check(getattr(load(), name)(*args))
