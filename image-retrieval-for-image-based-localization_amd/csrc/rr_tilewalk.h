// librr.so — which tiles a block of a persistent kernel owns.  Blocks are dealt round-robin over
// the 8 XCDs (block b runs on XCD b & 7), and both walks keep the tiles in flight on one XCD
// neighbours, so the rows they share are hits in that XCD's L2.  Plain C++17, no HIP types: host
// programs include it (the markers below are empty outside hipcc).
// The expressions are the kernels' own, term for term, and the block comes first among the
// parameters: operand order follows from both, and with them the kernels compile to the
// instructions they had when each wrote its walk out (tools/isa_diff.py).
#pragma once

#if defined(__HIPCC__)
#define RR_HD __host__ __device__ __forceinline__
#else
#define RR_HD inline
#endif

namespace rr {

// Range walk: XCD x owns the contiguous tiles [s_x, s_x + n_x) and its nb_x blocks stride through
// them; block bx takes tiles s_x + li + m * nb_x for every m with li + m * nb_x < n_x.
struct XcdTiles {
    int s_x, n_x;
};
struct TileRange {
    int s_x, n_x, nb_x, li;
};
// the tiles of block bx's XCD
RR_HD XcdTiles xcd_tiles(int bx, int ntiles) {
    const int xcd = bx & 7;
    const int nt8 = ntiles >> 3, rt8 = ntiles & 7;
    XcdTiles r;
    r.s_x = xcd < rt8 ? xcd * (nt8 + 1) : rt8 * (nt8 + 1) + (xcd - rt8) * nt8;
    r.n_x = nt8 + (xcd < rt8 ? 1 : 0);
    return r;
}
// ... and block bx's stride through them in a grid of nwg blocks.  Needs nwg >= 8, or one block
// per tile (nwg == ntiles: a plain bijective remap): with fewer blocks some XCD's tiles have no block.
RR_HD TileRange xcd_tile_range(int bx, int ntiles, int nwg) {
    const XcdTiles x = xcd_tiles(bx, ntiles);
    TileRange r;
    r.s_x = x.s_x;
    r.n_x = x.n_x;
    r.nb_x = (nwg >> 3) + ((bx & 7) < (nwg & 7) ? 1 : 0);
    r.li = bx >> 3;
    return r;
}

// Round walk: in round i the G blocks take tiles [i G, (i + 1) G), XCD x the G / 8 consecutive ones
// from i G + x G / 8; block b takes xcd_round_tile(b, G, i).  Needs G % 8 == 0: otherwise not a bijection.
RR_HD int xcd_round_tile(int b, int G, int i) { return i * G + (b & 7) * (G >> 3) + (b >> 3); }
// the rounds in which block b's tile exists (is below ntiles).  Needs G % 8 == 0.
RR_HD int xcd_round_count(int b, int ntiles, int G) {
    return (ntiles - 1 - (b >> 3) - (b & 7) * (G >> 3)) >= 0 ? (ntiles - 1 - (b & 7) * (G >> 3) - (b >> 3)) / G + 1 : 0;
}

// Host: the grid of a persistent launch on cus CUs, a multiple of 8 that is at least 8 -- what both
// walks need.  (Blocks beyond the tiles find their range or rounds empty and leave.)
inline int persistent_grid8(long long ntiles, int cus) {
    const int grid = (int)(ntiles < cus ? ntiles : cus) & ~7;
    return grid < 8 ? 8 : grid;
}
// Host: the grid of a range-walk launch that keeps one block per CU.  A grid below 8 blocks would
// leave some XCD's tile range without a block (xcd_tile_range needs nwg >= 8), so with fewer than
// 8 CUs -- or fewer tiles than CUs -- it falls back to one block per tile, the plain bijective remap.
inline long long range_walk_grid(long long ntiles, long long cus) { return cus < 8 || ntiles < cus ? ntiles : cus; }

}  // namespace rr
