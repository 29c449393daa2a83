// poa_slot_prof.h -- the header of a slot arena and the profile the block kernel keeps in it: host + device, constants only.
//
// Every slot arena starts with SLOT_HDR_BYTES (SlotLayout::hdr): the graph's two counters (n_nodes, n_edges: slot_views), then, from
// byte SLOT_PROF_OFF, SLOT_PROF_WORDS 64-bit words that thread 0 of the slot's workgroup accumulates over the blocks the slot runs.
// A launch starts them at zero (launch_plan) and the host reads them back afterwards (fetch_slot_prof in sxg_poa.hip).
// The profile fills the header to its last byte, and the next byte is the first graph array (SlotLayout::code): one more word
// needs a larger header.
#pragma once

namespace sxg {

constexpr int SLOT_HDR_BYTES = 512;
constexpr int SLOT_PROF_OFF = 64;     // bytes from the start of the header
constexpr int SLOT_PROF_WORDS = 56;
constexpr int SLOT_PROF_BYTES = 8 * SLOT_PROF_WORDS;
static_assert(SLOT_PROF_OFF + SLOT_PROF_BYTES <= SLOT_HDR_BYTES, "the slot profile ends inside the slot header");

// words of the profile (unsigned long long each)
enum : int {
    // core-clock cycles of the slot's phases, in the order of the debug output's "slot time:" line
    SP_OTHER = 0, SP_PREP_ROWS = 1, SP_DP_FILL = 2, SP_TRACEBACK = 3, SP_ADD_ALIGNMENT = 4, SP_OUTPUT = 5,
    SP_PHASES = 6,             // (their count)
    SP_CLOCK0 = 6, SP_CLOCK1 = 7,   // core clock at the slot's start and end (s_memtime)
    SP_WALL0 = 8, SP_WALL1 = 9,     // constant 100 MHz clock at the slot's start and end (s_memrealtime)
    SP_WAVE = 10,              // SP_WAVES words: placement of every wave, smid << 32 | raw HW_ID
    SP_WAVES = 16,
    SP_TILES = 26,             // 32-bit sweep in column tiles: sweeps | tiles they swept << 32, of the launches laid out for more than one tile
    SP_HINT_REPEATS = 27,      // packed sweep: sweeps repeated after a hint shift
    SP_ROW = 28,               // ROWP_WORDS words: DpBuffers::row_prof (SXG_ROW_PROF builds)
    SP_RESORT = 41,            // RSP_WORDS words: spoa_resort's rprof (SXG_RESORT_PROF builds)
    SP_BAND_STRIPS = 47,       // packed sweep: strips per plane row, summed over the sweeps ...
    SP_BAND_SWEEPS = 48,       // ... and their count
    SP_SWEEPS = 49,            // [2] by width (0: the geometry's W, 1: the class's second width): packed sweeps,
    SP_SWEPT_COLS = 51,        // [2] the columns they swept (T * 2 * Wk each)
    SP_SWEPT_CELLS = 53,       // [2] and rows x those columns
    SP_TWIN = 55,              // twin steps | join rows << 32 of the rows the slot prepared
    SP_WORDS_USED = 56,
};

// the row profile, relative to SP_ROW
enum : int {
    ROWP_SEGS = 8,             // words 0 .. 7: cycles per segment of a row (RP_MARK / BP_MARK number them)
    ROWP_TB_STEPS = 8, ROWP_TB_LOADS = 9, ROWP_TB_CYCLES = 10, ROWP_TB_FILL_CYCLES = 11, ROWP_TB_HITS = 12,   // traceback_p16
    ROWP_WORDS = 13,
};

// the re-sort profile, relative to SP_RESORT
enum : int {
    RSP_PHASES = 5,            // words 0 .. 4: cycles per phase of spoa_resort_par (SXG_RSP numbers them)
    RSP_ROUNDS = 5,
    RSP_WORDS = 6,
};

static_assert(SP_WAVE + SP_WAVES == SP_TILES && SP_TILES + 1 == SP_HINT_REPEATS, "placement words, then the tile counters");
static_assert(SP_ROW + ROWP_WORDS <= SP_RESORT, "the row profile ends in front of the re-sort profile");
static_assert(SP_RESORT + RSP_WORDS <= SP_BAND_STRIPS, "the re-sort profile ends in front of the band counters");
static_assert(SP_SWEEPS + 2 == SP_SWEPT_COLS && SP_SWEPT_COLS + 2 == SP_SWEPT_CELLS && SP_SWEPT_CELLS + 2 == SP_TWIN, "one word per width");
static_assert(SP_TWIN < SP_WORDS_USED && SP_WORDS_USED <= SLOT_PROF_WORDS, "every word lies inside the profile");

}  // namespace sxg
