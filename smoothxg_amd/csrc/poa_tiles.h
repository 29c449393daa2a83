// poa_tiles.h -- the column tiles of the 32-bit sweep (poa_dp.hip.h): which columns a tile owns, which lane of which tile a
// column belongs to, how wide the padded matrix is, and where a row's boundary record lies.
//
// Plain C++17, constexpr, no HIP: included by the sweep and its kernels (poa_dp.hip.h, poa_kernels.hip.h), by the host
// (sxg_poa.hip: the tile count of a block, the slot layout) and by the host-only check tests/csrc/tile_check.cpp.
//
// A workgroup of T lanes with W columns per lane sweeps tile_cols = T * W columns at once.  A sequence of L letters has the
// L + 1 columns 0 .. L; longer than one tile, the same workgroup sweeps the matrix tile after tile, left to right, every tile
// over all rows.  Tile k owns the columns [k * tile_cols, (k + 1) * tile_cols); lane t of tile k is the "virtual lane"
// k * T + t and owns the W columns from (k * T + t) * W on -- exactly the columns lane k * T + t of a workgroup of
// n_tiles * T lanes would own, so everything indexed per lane (row 0, the fold-step masks, the traceback bytes) is laid out
// as for that wider workgroup.  One tile describes today's sweep: Lpad_total = T * W, virtual lane = lane.
//
// What crosses a tile's right edge goes through one record per row (TileBoundary) in one of two buffers: tile k writes
// buffer k & 1 and reads buffer (k - 1) & 1, the one tile k - 1 wrote.
#pragma once

namespace sxg {

constexpr int tile_cols(int T, int W) { return T * W; }
// tiles of a sequence of L letters (columns 0 .. L), at least one
constexpr int n_tiles(int L, int T, int W) { return L < 0 ? 1 : (L + 1 + tile_cols(T, W) - 1) / tile_cols(T, W); }
// padded width of the matrix: row stride of the traceback plane and of row 0
constexpr long tiles_lpad_total(int tiles, int T, int W) { return (long)tiles * tile_cols(T, W); }
// first column of tile k, and of lane t inside it
constexpr int tile_col0(int k, int T, int W) { return k * tile_cols(T, W); }
constexpr int tile_lane_col0(int k, int t, int T, int W) { return tile_col0(k, T, W) + t * W; }
// virtual lane <-> (tile, lane)
constexpr int virtual_lane(int k, int t, int T) { return k * T + t; }
constexpr int vlane_tile(int v, int T) { return v / T; }
constexpr int vlane_lane(int v, int T) { return v % T; }
// the virtual lane that owns column j, and the column's index inside the lane's strip
constexpr int col_vlane(int j, int W) { return j / W; }
constexpr int col_in_strip(int j, int W) { return j % W; }
// lanes of the fold-step mask words and of row 0: one per virtual lane
constexpr int tiles_vlanes(int tiles, int T) { return tiles * T; }

// boundary buffers: the one tile k writes, the one it reads (k >= 1), records per buffer and the record of row i (0 = the
// virtual source row, 1 .. N = the graph rows)
constexpr int tile_wr_buf(int k) { return k & 1; }
constexpr int tile_rd_buf(int k) { return (k - 1) & 1; }
constexpr long tile_bnd_records(int rows_cap) { return (long)rows_cap + 1; }
constexpr long tile_bnd_index(int buf, int row, int rows_cap) { return (long)buf * tile_bnd_records(rows_cap) + row; }
constexpr int TILE_BND_BYTES = 16;   // sizeof(TileBoundary)

// longest sequence the tiled sweep takes: four tiles of the widest 32-bit geometry (1024 lanes x 12 columns)
constexpr int TILED_MAX_TILES = 4;
constexpr int TILED_MAX_SEQ_LEN = TILED_MAX_TILES * 12288 - 1;

}  // namespace sxg
