"""epg_test_force as a context manager, and the one-CU grid of tests/test_hip_persistent_loops.py.

Switch 5 (FORCE_CUS, csrc/epg_common.h) makes the library size every persistent grid as if the device had `value` compute units:
with 1 a wave walks many tiles of a small matrix, and the state it carries from tile to tile runs at test sizes.  A plain
module, not a conftest: the tests that want it import it."""
import contextlib

import numpy as np

FORCE_CUS = 5


@contextlib.contextmanager
def forced(abi, which, value, cus=None):
    """epg_test_force(which, value) for the block, reset to 0 whatever happens in it; cus: what epg_device_cus() must report
    while the switch is set."""
    abi.call("epg_test_force", which, value)
    try:
        if cus is not None:
            assert abi.call("epg_device_cus") == cus, "switch %d is not live" % which
        yield
    finally:
        abi.call("epg_test_force", which, 0)


@contextlib.contextmanager
def one_cu(abi):
    """Every grid of the block's calls is sized for ONE compute unit; the device's own count is back afterwards."""
    real = abi.call("epg_device_cus")
    assert real > 1, "the device reports %d compute unit(s): is the switch still set?" % real
    with forced(abi, FORCE_CUS, 1, cus=1):
        yield
    assert abi.call("epg_device_cus") == real


def capped_and_not(abi, fn):
    """fn() -> {name: host array}, once on the one-CU grid and once on the device's: the two runs must agree byte for byte.
    -> the capped run's outputs."""
    with one_cu(abi):
        capped = fn()
    free = fn()
    assert sorted(capped) == sorted(free)
    for name in capped:
        a, b = np.ascontiguousarray(capped[name]), np.ascontiguousarray(free[name])
        assert a.shape == b.shape and a.dtype == b.dtype, name
        diff = a.view(np.uint8) != b.view(np.uint8)
        assert not diff.any(), "%r: the one-CU grid and the device's grid differ in %d of %d bytes" % (name, int(diff.sum()), a.nbytes)
    return capped


# ----------------------------------------------------------------------------------------------------------------------------
# the dispatch code's grid arithmetic, restated (csrc/*.hip; `cus` = what num_cus() answers): what the cases of
# tests/test_hip_persistent_loops.py and the capped cases of tests/test_hip_abi_contract.py derive their tiles per wave from
# ----------------------------------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def count_grid(R, cus, per_cu=2):
    """grid_for_tiles (epg_s1.hip): workgroups of the count kernels; a workgroup is 4 waves, a wave's tile 32 rows."""
    nsuper = cdiv(R, 32)
    blocks = cdiv(nsuper, 4)
    cap = cus * per_cu
    if blocks > cap:
        iters = cdiv(nsuper, cap * 4)
        blocks = cdiv(nsuper, iters * 4)
    return max(blocks, 1)


def tiles_of_waves(ntiles, waves):
    """(fewest, most) tiles a wave of `waves` gets of ntiles tiles walked with a stride of `waves`."""
    return ntiles // waves, cdiv(ntiles, waves)


def tile_rows(row_bytes):
    """tile_rows (epg_common.h)"""
    tr = 64
    while tr > 8 and 4 * tr * row_bytes > 65536:
        tr >>= 1
    return tr


def flush_every(nmax):
    """bin_hist_body / k_pair_count_null: epilogues between two flushes of the packed 16-bit running counts."""
    return max(65535 // nmax - 1, 1)


def part_tiles(rows, tile):
    return sum(cdiv(r, tile) for r in rows)


def s1_from_hist_stride(total, nent, itemsize, cus):
    """launch_score_s1_from_hist_t (epg_s1.hip): threads of the grid = quads (four counts) per sweep."""
    tbytes = nent * itemsize
    if tbytes <= 150 * 1024:                                              # the table in LDS
        nb, threads = min(cdiv(total // 4, 4096), cus * (2 if tbytes <= 75 * 1024 else 1)), 1024
    else:
        nb, threads = min(cdiv(total // 4, 1024), cus * 8), 256
    return max(nb, 1) * threads


def pair_fused_waves(S, NA, NB, ga, gb):
    """epg_pair_scores_s1_parts: waves of the ONE workgroup per CU (a null table that is the real group's is not copied twice)."""
    ent = lambda n: (n + 1) * S
    tab = (ent(NA) + ent(NB) + (0 if ga == NA else ent(ga)) + (0 if gb == NB else ent(gb))) * 4
    tab = (tab + 15) & ~15
    per_wave = 64 * (4 * 2 * S + (0 if S in (15, 18, 25) else 4 * S))
    assert tab + 4 * per_wave <= 160 * 1024
    return min((160 * 1024 - tab) // per_wave, 12)


def nh_strings(n_cols, ga, gb):
    strings = 1 if ga + gb == n_cols else 2
    assert strings * cdiv(n_cols, 32) * 256 <= 24 * 1024
    return strings


def null_draws_waves(S, n_cols, ga, gb):
    """nd_waves (epg_null.hip)"""
    tab = ((ga + 1 + gb + 1) * S * 4 + 15) & ~15
    per_wave = 3 * 64 * 2 * S + nh_strings(n_cols, ga, gb) * cdiv(n_cols, 32) * 256
    return min((160 * 1024 - tab) // per_wave, 16)


def pair_count_null_waves(S, n_cols, cus):
    """launch_pair_count_null (epg_null.hip): workgroups per CU by their LDS, four waves each"""
    shmem = 4 * (2 * 64 * 2 * S + cdiv(n_cols, 32) * 256)
    return cus * max((160 * 1024 - 1024) // shmem, 1) * 4
