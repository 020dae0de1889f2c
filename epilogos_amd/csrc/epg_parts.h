// Several parts (the chromosome files of a genome, both groups of a paired run) in ONE kernel launch.  A parts struct travels in
// the kernel argument: per-part arrays of MAXP slots (pointers, shapes, shuffle keys: whatever the kernel needs), `long rows[MAXP]`,
// `long t0[MAXP + 1]` and `int n`.  Tiles of tile_rows rows are numbered through the n parts in order and never straddle two parts:
// t0[k] is the first tile of part k, t0[n] the number of tiles, a part's last tile may be partial.  The host fills the struct with
// pack_parts, a wave finds the part of its tile with a PartCursor.  Plain integer code, nothing from HIP: tests/test_parts_host.py
// walks packed tables on the host with the code that the kernels run.
#pragma once
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define EPG_HOST_DEVICE __host__ __device__ __forceinline__
#else
#define EPG_HOST_DEVICE
#endif

namespace epg {

// Where a wave is among the parts.  A wave's tile index only ascends, so its part only moves forward.
struct PartCursor {
    int part = 0;
    // `tile` (at or after the last one asked for) -> its first row in its part, `part`; t0 = first tile of every part, and the total
    EPG_HOST_DEVICE long advance(const long* t0, long tile, int tile_rows) {
        while (tile >= t0[part + 1]) ++part;
        return (tile - t0[part]) * tile_rows;
    }
};

// Host side: fills `pt` with the parts p0, p0 + 1 ... for which rows(p) is not 0 (0 leaves a part out of this launch), as many as
// it holds; fill(k, p) copies part p's pointers and shapes into slot k.  -> the first part not taken; pt.n == 0: nothing is left.
template <typename Parts, typename Rows, typename Fill>
static int pack_parts(Parts& pt, int p0, int nparts, int tile_rows, Rows&& rows, Fill&& fill) {
    constexpr int MAXP = (int)(sizeof(pt.rows) / sizeof(pt.rows[0]));
    memset(&pt, 0, sizeof(pt));
    long tiles = 0;
    int p = p0;
    for (; p < nparts && pt.n < MAXP; ++p) {
        const long r = rows(p);
        if (r == 0) continue;
        const int k = pt.n++;
        fill(k, p);
        pt.rows[k] = r;
        pt.t0[k] = tiles;
        tiles += (r + tile_rows - 1) / tile_rows;
    }
    pt.t0[pt.n] = tiles;
    return p;
}

// any of these pointers is not 16-byte aligned
template <typename... P>
static bool misaligned16(const P*... p) { return ((reinterpret_cast<uintptr_t>(p) | ...) & 15) != 0; }

}  // namespace epg
