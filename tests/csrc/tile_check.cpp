// TEST HARNESS: the column tiles of the 32-bit sweep (smoothxg_amd/csrc/poa_tiles.h) on the host, plain C++.  Never shipped.
//
// For every 32-bit geometry the host can choose (variant_for_len over every length it covers, row modes 0 and 1 -- which
// includes the widest one, 16 waves of 12 columns, and the ones SXG_POA_TILE_COLS = 512 and 6144 stand for) and every sequence
// length L = 0 .. SXG_POA_MAX_SEQ_LEN_TILED:
//   * the tiles partition the columns 0 .. L: tile 0 starts at column 0, a tile starts where the one before it ends, the last
//     one holds column L, and none is empty;
//   * virtual lane <-> (tile, lane) is a bijection onto [0, n_tiles * T), a virtual lane's first column is W times its number,
//     and every column of a lane's strip maps back to that lane and to its index inside the strip;
//   * a sequence the geometry covers has one tile, whose padded width is the geometry's Lpad and whose virtual lanes are the lanes;
//   * the boundary buffers alternate: a tile reads what the tile before it wrote, never the buffer it writes, and the records of
//     the two buffers do not overlap;
//   * a tiled launch is priced rows x Lpad_total (poa_cost.h), a launch of one tile as before.
// Prints one line per geometry: T W tile_cols tiles(49151) Lpad_total(49151); exit status 1 with the first failures on stderr.
#include <cstdint>
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

#include "../../include/sxg_poa.h"
#include "../../smoothxg_amd/csrc/poa_classes.h"
#include "../../smoothxg_amd/csrc/poa_cost.h"
#include "../../smoothxg_amd/csrc/poa_tiles.h"

using namespace sxg;

static int bad = 0;
#define CHECK(cond, ...)                                                          \
    do {                                                                          \
        if (!(cond)) {                                                            \
            if (++bad <= 20) { fprintf(stderr, "%s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } \
        }                                                                         \
    } while (0)

static_assert(TILED_MAX_SEQ_LEN == SXG_POA_MAX_SEQ_LEN_TILED, "the header's limit");
static_assert(n_tiles(SXG_POA_MAX_SEQ_LEN_WIDE, 1024, 12) == 1 && n_tiles(SXG_POA_MAX_SEQ_LEN_WIDE + 1, 1024, 12) == 2, "today's limit is one tile");
static_assert(n_tiles(SXG_POA_MAX_SEQ_LEN_TILED, 1024, 12) == TILED_MAX_TILES, "the tiled limit fills the last tile");

int main() {
    std::set<std::pair<int, int>> geos;   // (T, W)
    for (int rm = 0; rm <= 1; ++rm)
        for (int len = 0; len <= SXG_POA_MAX_SEQ_LEN_WIDE; ++len) {
            Variant v{0, 0, 0, 0};
            if (!variant_for_len(len, rm, &v)) { CHECK(false, "no geometry for %d letters", len); continue; }
            geos.insert({v.T(), v.W});
            // a sequence its geometry covers: one tile, today's padded width
            CHECK(n_tiles(len, v.T(), v.W) == 1, "len %d T %d W %d", len, v.T(), v.W);
            CHECK(tiles_lpad_total(1, v.T(), v.W) == v.Lpad(), "T %d W %d", v.T(), v.W);
        }
    {
        Variant v{0, 0, 0, 0};
        CHECK(!variant_for_len(SXG_POA_MAX_SEQ_LEN_WIDE + 1, 0, &v) && !variant_for_len(SXG_POA_MAX_SEQ_LEN_WIDE + 1, 1, &v), "a geometry beyond the widest");
        CHECK(geos.count({1024, 12}) == 1 && geos.count({64, 8}) == 1 && geos.count({512, 12}) == 1, "the geometries the tests force");
    }
    for (const auto& g : geos) {
        const int T = g.first, W = g.second, tc = tile_cols(T, W);
        CHECK(tc == T * W, "T %d W %d", T, W);
        for (int L = 0; L <= SXG_POA_MAX_SEQ_LEN_TILED; ++L) {
            const int nt = n_tiles(L, T, W);
            CHECK(nt >= 1 && tile_col0(0, T, W) == 0, "L %d", L);
            CHECK(tile_col0(nt - 1, T, W) <= L && L < tile_col0(nt, T, W), "column L = %d outside the last of %d tiles of %d", L, nt, tc);
            CHECK(tiles_lpad_total(nt, T, W) == (long)nt * tc && tiles_lpad_total(nt, T, W) >= L + 1, "L %d", L);
            if (L < tc) CHECK(nt == 1, "L %d T %d W %d", L, T, W);
            // priced rows x Lpad_total; one tile: T * W whatever the length
            CHECK(cost_cols(0, T, W, 0, L, 2) == (uint64_t)tiles_lpad_total(nt, T, W), "cost L %d", L);
            CHECK(cost_cols(1, T, W, 0, L) == (uint64_t)tc && cost_cols(1, T, W, 0, L, 1) == (uint64_t)tc, "cost of one tile L %d", L);
        }
        // tiles follow each other without a gap; lanes of a tile likewise; the mappings invert each other
        const int nt = n_tiles(SXG_POA_MAX_SEQ_LEN_TILED, T, W);
        std::vector<char> seen((size_t)tiles_vlanes(nt, T), 0);
        for (int k = 0; k < nt; ++k) {
            CHECK(tile_col0(k + 1, T, W) - tile_col0(k, T, W) == tc, "tile %d", k);
            for (int t = 0; t < T; ++t) {
                const int v = virtual_lane(k, t, T);
                CHECK(v >= 0 && v < tiles_vlanes(nt, T) && !seen[(size_t)v], "virtual lane %d of (%d, %d)", v, k, t);
                if (v >= 0 && v < tiles_vlanes(nt, T)) seen[(size_t)v] = 1;
                CHECK(vlane_tile(v, T) == k && vlane_lane(v, T) == t, "(%d, %d) -> %d -> (%d, %d)", k, t, v, vlane_tile(v, T), vlane_lane(v, T));
                CHECK(tile_lane_col0(k, t, T, W) == v * W, "first column of (%d, %d)", k, t);
                if (k == 0) CHECK(v == t, "one tile: virtual lane %d of lane %d", v, t);
                for (int c = 0; c < W; ++c) {
                    const int j = tile_lane_col0(k, t, T, W) + c;
                    CHECK(col_vlane(j, W) == v && col_in_strip(j, W) == c, "column %d", j);
                    CHECK(j >= tile_col0(k, T, W) && j < tile_col0(k + 1, T, W), "column %d outside tile %d", j, k);
                }
            }
        }
        for (char s : seen) CHECK(s, "a virtual lane nobody owns (T %d W %d)", T, W);
        printf("%d %d %d %d %ld\n", T, W, tc, nt, tiles_lpad_total(nt, T, W));
    }
    // boundary buffers
    for (int k = 0; k < 200; ++k) {
        CHECK(tile_wr_buf(k) == 0 || tile_wr_buf(k) == 1, "tile %d", k);
        CHECK(tile_wr_buf(k) != tile_wr_buf(k + 1), "tile %d writes the buffer of tile %d", k + 1, k);
        CHECK(tile_rd_buf(k + 1) == tile_wr_buf(k), "tile %d does not read what tile %d wrote", k + 1, k);
        CHECK(tile_rd_buf(k + 1) != tile_wr_buf(k + 1), "tile %d reads the buffer it writes", k + 1);
    }
    for (int rows_cap : {0, 1, 7, 1000, (1 << 20) - 1}) {
        CHECK(tile_bnd_records(rows_cap) == (long)rows_cap + 1, "rows_cap %d", rows_cap);
        CHECK(tile_bnd_index(0, 0, rows_cap) == 0 && tile_bnd_index(0, rows_cap, rows_cap) + 1 == tile_bnd_index(1, 0, rows_cap), "rows_cap %d", rows_cap);
        CHECK(tile_bnd_index(1, rows_cap, rows_cap) + 1 == 2 * tile_bnd_records(rows_cap), "rows_cap %d", rows_cap);
        for (int row = 0; row + 1 <= rows_cap && row < 5; ++row)
            CHECK(tile_bnd_index(0, row + 1, rows_cap) == tile_bnd_index(0, row, rows_cap) + 1, "rows_cap %d row %d", rows_cap, row);
    }
    static_assert(TILE_BND_BYTES == 16, "one 16-byte record");
    if (bad) fprintf(stderr, "%d checks failed\n", bad);
    return bad ? 1 : 0;
}
