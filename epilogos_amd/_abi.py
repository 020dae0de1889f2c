"""ctypes binding of include/epilogos_amd.h, include/epilogos_scores_text.h, include/epilogos_groups.h,
include/epilogos_nulldraws.h, include/epilogos_statebyline.h, include/epilogos_segments.h, include/epilogos_simsearch_pick.h,
include/epilogos_census.h, include/epilogos_concordance.h and include/epilogos_gennorm.h.  No fallbacks: a missing library or symbol raises."""
import ctypes as C
import re
from pathlib import Path

from . import build as _build

EPG_OK = 0
ERR_NAMES = {-1: "EPG_ERR_INVALID_ARG", -2: "EPG_ERR_UNSUPPORTED", -3: "EPG_ERR_HIP", -4: "EPG_ERR_WORKSPACE"}

HEADER = Path(__file__).resolve().parents[1] / "include" / "epilogos_amd.h"


class EpilogosHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s (%d): %s" % (ERR_NAMES.get(code, "EPG_ERR"), code, msg))
        self.code = code


_p = C.c_void_p
_i64 = C.c_int64
_i32 = C.c_int32
_u64 = C.c_uint64

# name -> (restype, argtypes); must list every prototype of the header (tests/test_abi_symbols.py checks it)
PROTOTYPES = {
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
}

# the same for include/epilogos_scores_text.h, the GPU scores-text parser (tests/test_scores_text_host.py checks it)
TEXT_HEADER = HEADER.with_name("epilogos_scores_text.h")
TEXT_PROTOTYPES = {
    "epgt_scores_ws_bytes": (_i64, [_i64]),
    "epgt_scores_parse": (C.c_int, [_p, _i64, _i32, _i64, _i64, _p, _p, _p, _p, _p, _i64, _p, _p]),
}

# and for include/epilogos_groups.h, the column-group count pass (tests/test_groups_host.py checks it)
GROUP_HEADER = HEADER.with_name("epilogos_groups.h")
GROUP_PROTOTYPES = {
    "epg_bin_hist_groups": (C.c_int, [_p, _i64, _i32, _i64, _i32, _i32, _p, _p, _p, _p]),
}

# and for include/epilogos_nulldraws.h, the K-draw null of paired mode (tests/test_null_draws_host.py checks it)
NULLDRAWS_HEADER = HEADER.with_name("epilogos_nulldraws.h")
NULLDRAWS_PROTOTYPES = {
    "epg_null_dist_draws_parts": (C.c_int, [_i32, _p, _p, _p, _p, _p, _i32, _i32, _i32, _i32, _i32, _p, _p, _p, _i32, _p, _p]),
    "epg_null_exceed_ws_bytes": (_i64, [_i64]),
    "epg_null_exceed": (C.c_int, [_p, _i64, _p, _i64, _p, _p, _i64, _p]),
}

# and for include/epilogos_statebyline.h, the reader of ChromHMM state-by-line calls (tests/test_statebyline_host.py checks it)
SBL_HEADER = HEADER.with_name("epilogos_statebyline.h")
SBL_PROTOTYPES = {
    "epg_sbl_ws_bytes": (_i64, [_i64]),
    "epg_sbl_constant": (_i32, [_i32]),
    "epg_sbl_parse": (C.c_int, [_p, _i64, _p, _i64, _p, _p, _i64, _p]),
    "epg_sbl_transpose": (C.c_int, [_p, _i32, _i64, _i64, _p, _i64, _i64, _p]),
}

# and for include/epilogos_segments.h, the reader of ChromHMM segment files (tests/test_segments_host.py checks it)
SEG_HEADER = HEADER.with_name("epilogos_segments.h")
SEG_PROTOTYPES = {
    "epg_seg_ws_bytes": (_i64, [_i64, _i32]),
    "epg_seg_constant": (_i32, [_i32]),
    "epg_seg_parse": (C.c_int, [_p, _i64, _p, _i32, _i32, _p, _p, _i64, _p, _p, _p, _i64, _p]),
    "epg_seg_expand": (C.c_int, [_p, _p, _p, _i32, _p, _i64, _p]),
}

# and for include/epilogos_simsearch_pick.h, the device STEP 1 of simsearch -b (tests/test_simsearch_pick_host.py checks it)
PICK_HEADER = HEADER.with_name("epilogos_simsearch_pick.h")
PICK_PROTOTYPES = {
    "epg_simsearch_rowscore": (C.c_int, [_p, _i64, _i32, _p, _p]),
    "epg_simsearch_rolling_max": (C.c_int, [_p, _i64, _i32, _p, _p]),
    "epg_simsearch_rank_ws_bytes": (_i64, [_i64]),
    "epg_simsearch_rank": (C.c_int, [_p, _p, _p, _i64, _p, _p, _i64, _p]),
    "epg_simsearch_pick_ws_bytes": (_i64, [_i64, _i32]),
    "epg_simsearch_pick": (C.c_int, [_p, _i64, _i32, _i64, _p, _p, _p, _p, _i64, _p]),
}

# and for include/epilogos_census.h, the per-biosample state census (tests/test_census_host.py checks it)
CENSUS_HEADER = HEADER.with_name("epilogos_census.h")
CENSUS_PROTOTYPES = {
    "epg_state_census": (C.c_int, [_p, _i64, _i32, _i64, _i32, _p, _p, _p, _p]),
}

# and for include/epilogos_concordance.h, the pairwise state agreement of biosample columns (tests/test_concordance_host.py checks it)
CONCORDANCE_HEADER = HEADER.with_name("epilogos_concordance.h")
CONCORDANCE_PROTOTYPES = {
    "epg_concordance_ws_bytes": (_i64, [_i64, _i32, _i32]),
    "epg_concordance": (C.c_int, [_p, _i64, _i32, _i64, _i32, _p, _p, _p, _i64, _p]),
}

# and for include/epilogos_gennorm.h, the device fit of the paired null distribution (tests/test_gennorm_host.py checks it)
GENNORM_HEADER = HEADER.with_name("epilogos_gennorm.h")
GENNORM_PROTOTYPES = {
    "epgf_gennorm_ws_bytes": (_i64, [_i64, _i32, _i64]),
    "epgf_gennorm_fit": (C.c_int, [_p, _i64, _p, _i32, _i64, _p, _p, _p, _p, _i64, _p]),
    "epgf_gennorm_nnlf": (C.c_int, [_p, _i64, _p, _i32, _p, _p, _i64, _p]),
}

_lib = None


def gennorm_header_symbols():
    """Function names declared in include/epilogos_gennorm.h."""
    txt = re.sub(r"/\*.*?\*/", "", GENNORM_HEADER.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(epgf_[a-z0-9_]+)\s*\(", txt)))


def concordance_header_symbols():
    """Function names declared in include/epilogos_concordance.h."""
    txt = re.sub(r"/\*.*?\*/", "", CONCORDANCE_HEADER.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(epg_[a-z0-9_]+)\s*\(", txt)))


def census_header_symbols():
    """Function names declared in include/epilogos_census.h."""
    txt = re.sub(r"/\*.*?\*/", "", CENSUS_HEADER.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(epg_[a-z0-9_]+)\s*\(", txt)))


def pick_header_symbols():
    """Function names declared in include/epilogos_simsearch_pick.h."""
    txt = re.sub(r"/\*.*?\*/", "", PICK_HEADER.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(epg_[a-z0-9_]+)\s*\(", txt)))


def pick_header_constant(name):
    """The value of `#define name <integer>` of include/epilogos_simsearch_pick.h (EPG_PICK_TILE, EPG_PICK_MAX_W)."""
    m = re.search(r"^#define\s+%s\s+(\d+)" % re.escape(name), PICK_HEADER.read_text(), flags=re.M)
    if m is None:
        raise RuntimeError("%s not found in %s" % (name, PICK_HEADER))
    return int(m.group(1))


def seg_header_symbols():
    """Function names declared in include/epilogos_segments.h."""
    txt = re.sub(r"/\*.*?\*/", "", SEG_HEADER.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(epg_[a-z0-9_]+)\s*\(", txt)))


def sbl_header_symbols():
    """Function names declared in include/epilogos_statebyline.h."""
    txt = re.sub(r"/\*.*?\*/", "", SBL_HEADER.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(epg_[a-z0-9_]+)\s*\(", txt)))


def text_header_symbols():
    """Function names declared in include/epilogos_scores_text.h."""
    txt = re.sub(r"/\*.*?\*/", "", TEXT_HEADER.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(epgt_[a-z0-9_]+)\s*\(", txt)))


def group_header_symbols():
    """Function names declared in include/epilogos_groups.h."""
    txt = re.sub(r"/\*.*?\*/", "", GROUP_HEADER.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(epg_[a-z0-9_]+)\s*\(", txt)))


def nulldraws_header_symbols():
    """Function names declared in include/epilogos_nulldraws.h."""
    txt = re.sub(r"/\*.*?\*/", "", NULLDRAWS_HEADER.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(epg_[a-z0-9_]+)\s*\(", txt)))


def header_symbols():
    """Function names declared in include/epilogos_amd.h."""
    txt = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(epg_[a-z0-9_]+)\s*\(", txt)))


def lib_path():
    """The in-tree library; EPILOGOS_HIP_LIB=<path> loads another build of it (A/B measurements of kernel variants)."""
    import os
    p = os.environ.get("EPILOGOS_HIP_LIB")
    return Path(p) if p else _build.LIB_PATH


def _header_abi_version():
    m = re.search(r"^#define\s+EPG_ABI_VERSION\s+(\d+)", HEADER.read_text(), flags=re.M)
    if m is None:
        raise RuntimeError("EPG_ABI_VERSION not found in %s" % HEADER)
    return int(m.group(1))


ABI_VERSION = _header_abi_version()                         # one source: the header the library is built from


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
    for name, (res, args) in list(PROTOTYPES.items()) + list(TEXT_PROTOTYPES.items()) + list(GROUP_PROTOTYPES.items()) + \
            list(NULLDRAWS_PROTOTYPES.items()) + list(SBL_PROTOTYPES.items()) + list(SEG_PROTOTYPES.items()) + list(PICK_PROTOTYPES.items()) + \
            list(CENSUS_PROTOTYPES.items()) + list(CONCORDANCE_PROTOTYPES.items()) + list(GENNORM_PROTOTYPES.items()):
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
