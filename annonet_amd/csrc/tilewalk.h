// tilewalk.h — the tile list of the conv and filter-gradient kernels, stated once: a layer's tiles are numbered row-major over
// (image, tile row, tile column); a kernel decodes a tile number with tile_pos, a persistent workgroup visits the numbers
// tile_walk gives it, and the hosts size the list with the tiles_* functions.  Plain C++ (no HIP needed):
// tests/cpp/tilewalk_check.cpp compiles this header alone and pins the walk (tests/test_tilewalk_host.py).
#pragma once

#ifdef __HIPCC__
#define ANH_TILE_FN __host__ __device__ __forceinline__
#else
#define ANH_TILE_FN inline
#endif

namespace anh {

// where tile number `tile` lies: column, row, image
struct TilePos { int tx, ty, n; };
ANH_TILE_FN TilePos tile_pos(int tile, int tiles_x, int tiles_y) {
    return TilePos{tile % tiles_x, (tile / tiles_x) % tiles_y, tile / (tiles_x * tiles_y)};
}

// Which tiles workgroup `wg` of `n_wgs` walks: first, first + step, ... below end.  Plain: tile wg, then every n_wgs-th.
// XCD bands (`bands`; n_wgs a multiple of 8, tile_bands_ok): the hardware deals workgroups round-robin over the 8 XCDs (observed,
// MI355X_MICROARCH.md: blocks b and b + 8 share one — used for speed only, any placement gives the same result), so the workgroups
// with equal wg & 7 take ONE contiguous eighth of the row-major tile list and step through it together, n_wgs / 8 consecutive tiles
// at a time: the halo rows and columns a patch shares with its neighbours are then re-read from that XCD's own L2 instead of once
// per XCD from the memory side.  (The spelling below is the one profiles/tile_walk_kernel_code.txt measured: the same values written
// as selects of precomputed band figures cost two conv3x3_ws forms 36 bytes of scratch.)
struct TileWalk { int first, step, end; };
ANH_TILE_FN TileWalk tile_walk(unsigned wg, unsigned n_wgs, int n_tiles, int bands) {
    const int band_len = (n_tiles + 7) >> 3;
    const int first = bands ? (int)(wg & 7) * band_len + (int)(wg >> 3) : (int)wg;
    const int step = bands ? (int)(n_wgs >> 3) : (int)n_wgs;
    const int band_end = ((int)(wg & 7) + 1) * band_len;
    return TileWalk{first, step, bands ? (n_tiles < band_end ? n_tiles : band_end) : n_tiles};
}
ANH_TILE_FN bool tile_bands_ok(int n_wgs) { return n_wgs % 8 == 0 && n_wgs >= 8; }

// A position that runs through a walk without a division per tile: pos == tile_pos(tile) after every advance().
struct TileCursor {
    int step, tiles_x, tiles_y;
    TilePos step_pos;   // the step as (columns, rows, images)
    int tile;
    TilePos pos;
    ANH_TILE_FN TileCursor(int first, int step_, int tiles_x_, int tiles_y_)
        : step(step_), tiles_x(tiles_x_), tiles_y(tiles_y_), step_pos(tile_pos(step_, tiles_x_, tiles_y_)), tile(first), pos(tile_pos(first, tiles_x_, tiles_y_)) {}
    ANH_TILE_FN void advance() {
        tile += step;
        pos.tx += step_pos.tx; if (pos.tx >= tiles_x) { pos.tx -= tiles_x; ++pos.ty; }
        pos.ty += step_pos.ty; if (pos.ty >= tiles_y) { pos.ty -= tiles_y; ++pos.n; }
        pos.n += step_pos.n;
    }
};

// Host side: how many tiles a layer has.  Every geometry's tile is 32 columns wide.
struct TileCounts { int tiles_x, tiles_y, total; };
ANH_TILE_FN TileCounts tile_counts(int h, int w, int tile_h, int n) {
    const int tiles_x = (w + 31) / 32, tiles_y = (h + tile_h - 1) / tile_h;
    return TileCounts{tiles_x, tiles_y, tiles_x * tiles_y * n};
}
ANH_TILE_FN TileCounts tiles_s1(int h_out, int w_out, int n) { return tile_counts(h_out, w_out, 8, n); }      // stride 1: 8 x 32 output tiles
ANH_TILE_FN TileCounts tiles_down(int h_out, int w_out, int n) { return tile_counts(h_out, w_out, 4, n); }    // stride-2 gather 0: 4 x 32 output tiles
ANH_TILE_FN TileCounts tiles_up(int h_in, int w_in, int n) { return tile_counts(h_in + 1, w_in + 1, 4, n); }  // stride-2 gather 1: 4 x 32 low-res positions, one past the input
ANH_TILE_FN TileCounts tiles_stem(int h_out, int w_out, int n) { return tile_counts(h_out, w_out, 8, n); }    // 5x5 stem, forward and filter gradient: 8 x 32
// filter gradient of the 3x3 layers: tile_h x 32 tiles of the low-resolution tensor (tile_h = 4 or 8: wgrad_plan_mfma)
ANH_TILE_FN TileCounts tiles_wgrad(int lr_h, int lr_w, int tile_h, int n) { return tile_counts(lr_h, lr_w, tile_h, n); }

}  // namespace anh
