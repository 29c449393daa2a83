// TEST HARNESS: the packed sweep's pass 2 without the in-strip state of the long gap piece, and with the local clamp carried in
// E (smoothxg_amd/csrc/poa_fields.h: p16_strip_q_dominated; smoothxg_amd/csrc/poa_dp16_row.inc.h).  One row, restated on the
// host with plain integers in three forms, from the same H-before-the-in-row-gaps (pass 1's Hc):
//   PLAIN   the recurrence itself, column by column over the whole row: h = max(Hc, E, Q, clamp), E = max(h + g, E + e),
//           Q = max(h + q, Q + c);
//   KEPT    the sweep as it was: strips of W columns, the carries into a strip scanned from pass 1's a and b, Q updated per column;
//   SHORT   the sweep as it is: the same carries, h = max(Hc, E, Qin - k |c|), no Q update, and for local rows E floored at the
//           bias (entering a strip and in its update) instead of the clamp of h.
// A "wave" is a few strips: at its right edge E and the word of the long piece go to the next wave as the kernel's mailbox
// does -- E out of pass 2, the long piece as Q out of pass 2 (KEPT) or as max(Qin - W |c|, b) (SHORT).
// Checks: the three rows of H are equal; the mailbox words agree (local: exactly, E up to the floor at the bias; global: up to
// the floor P16_NWFLOOR + q, below which no word decides a cell); the fields of SHORT stay inside the range poa_fields.h
// argues for; the dominance condition holds at every strip width a default-score class is built for.
// Prints "<checks> <failures>".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../smoothxg_amd/csrc/poa_classes.h"
#include "../../smoothxg_amd/csrc/poa_fields.h"

using namespace sxg;

static long n_checks = 0, n_bad = 0;
#define CHECK(cond) do { ++n_checks; if (!(cond) && ++n_bad <= 5) fprintf(stderr, "line %d: %s\n", __LINE__, #cond); } while (0)

constexpr int G = P16_DEF_G, E_ = P16_DEF_E, Q_ = P16_DEF_Q, C = P16_DEF_C;
constexpr int NWFLOOR = -16000, NEGP = -16384;   // the global rows' clamp and "minus infinity" (poa_dp16.hip.h)
constexpr int FAR = -(1 << 28);                  // a scan that has seen nothing yet

struct Mode { bool sw; int bias, floorv, clamp; };
static Mode mode_of(bool sw) { return sw ? Mode{true, P16_BIAS, P16_FLOOR, P16_BIAS} : Mode{false, 0, NEGP, NWFLOOR}; }

static void row_plain(const Mode& m, const std::vector<int>& hc, std::vector<int>& h) {
    int E = m.floorv, Q = m.floorv;
    h.resize(hc.size());
    for (size_t j = 0; j < hc.size(); ++j) {
        const int v = std::max(std::max(hc[j], E), std::max(Q, m.clamp));
        h[j] = v;
        E = std::max(v + G, E + E_);
        Q = std::max(v + Q_, Q + C);
    }
}

struct Words { std::vector<int> e, q; };   // what crosses each wave's right edge

// the strip forms: W columns per strip, SPW strips per wave; short_form = false: KEPT, true: SHORT.  lo / hi: the least and the
// greatest field any register of pass 2 held
static void row_strips(const Mode& m, const std::vector<int>& hc, int W, int SPW, bool short_form, std::vector<int>& h, Words& mb, int* lo, int* hi, bool drop_b = false) {
    const int S = (int)hc.size() / W;
    const bool floorE = short_form && m.sw;
    h.assign(hc.size(), 0);
    mb.e.clear(); mb.q.clear();
    int ce = FAR, cq = FAR;   // the scans: max over the strips to the left of what they leave, run up to this strip
    for (int u = 0; u < S; ++u) {
        const int* x = &hc[(size_t)u * W];
        // pass 1's carries: an opening inside the strip, as it stands behind the strip's last column
        int a = FAR, b = FAR;
        for (int k = 0; k < W; ++k) { a = std::max(a, x[k] + (W - 1 - k) * E_); b = std::max(b, x[k] + (W - 1 - k) * C); }
        if (m.sw) { a = std::max(a, m.bias); b = std::max(b, m.bias); }
        a += G; b += Q_;
        if (drop_b) b = FAR;   // (the control: a strip that hands on no opening of its own)
        const int Ein = std::max(ce, floorE ? m.bias : m.floorv), Qin = std::max(cq, m.floorv);
        int E = Ein, Q = Qin;
        for (int k = 0; k < W; ++k) {
            int v;
            if (short_form) {
                const int Qr = Qin + k * C;
                *lo = std::min(*lo, std::min(Qr, E));
                v = std::max(std::max(x[k], E), Qr);
                if (!m.sw) v = std::max(v, m.clamp);
                E = std::max(v + G, E + E_);
                if (floorE) E = std::max(E, m.bias);
            } else {
                v = std::max(std::max(x[k], E), std::max(Q, m.clamp));
                E = std::max(v + G, E + E_);
                Q = std::max(v + Q_, Q + C);
            }
            *hi = std::max(*hi, std::max(v, E));
            h[(size_t)u * W + k] = v;
        }
        ce = std::max(ce + W * E_, a);
        cq = std::max(cq + W * C, b);
        if ((u + 1) % SPW == 0) {   // a wave's right edge: the mailbox replaces the scans
            const int qw = short_form ? std::max(Qin + W * C, b) : Q;
            mb.e.push_back(E); mb.q.push_back(qw);
            ce = E; cq = qw;
        }
    }
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (unsigned)(rng_state >> 32); }
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (unsigned)(hi - lo + 1)); }

// H before the in-row gaps, as scores: kind 0 random walk, 1 steps, 2 spikes over a flat run at 0, 3 flat at 0, 4 one cliff
static void make_row(bool sw, int kind, int n, std::vector<int>& hc) {
    hc.resize((size_t)n);
    const int low = sw ? -26 : -400;   // a local cell before the gaps: at least an opening below 0
    int v = sw ? rnd_in(0, 60) : rnd_in(-200, 200);
    const int step_every = rnd_in(3, 40), spike_every = rnd_in(2, 30);
    for (int j = 0; j < n; ++j) {
        switch (kind) {
        case 0: v += rnd_in(-6, 5); break;
        case 1: if (j % step_every == 0) v += rnd_in(-120, 120); break;
        case 2: v = (j % spike_every == 0) ? rnd_in(20, 400) : (sw ? rnd_in(-4, 0) : rnd_in(-300, -250)); break;
        case 3: v = sw ? 0 : -200; break;
        default: v = j < n / 2 ? 500 - (j & 1) : (sw ? -4 : -420); break;
        }
        v = std::max(v, low);
        hc[(size_t)j] = v;
    }
}

static void run_case(bool sw, int W, int kind, bool near_floor) {
    const Mode m = mode_of(sw);
    const int SPW = rnd_in(1, 4), S = SPW * rnd_in(2, 5);
    std::vector<int> hc, hp, hk, hs;
    make_row(sw, kind, S * W, hc);
    for (int& v : hc) v += m.bias;
    // global rows near the clamp: what the clamp hides may differ between the forms' mailbox words, never a cell
    if (near_floor) for (int& v : hc) v = std::max(NWFLOOR - 40, NWFLOOR + (v % 97) - 48);
    Words wk, ws;
    int lo = 1 << 30, hi = -(1 << 30), lo_k = 1 << 30, hi_k = -(1 << 30);
    row_plain(m, hc, hp);
    row_strips(m, hc, W, SPW, false, hk, wk, &lo_k, &hi_k);
    row_strips(m, hc, W, SPW, true, hs, ws, &lo, &hi);
    CHECK(hk == hp);
    CHECK(hs == hp);
    CHECK(ws.q.size() == wk.q.size());
    for (size_t x = 0; x < ws.q.size() && x < wk.q.size(); ++x) {
        if (sw) {
            CHECK(ws.q[x] == wk.q[x]);
            CHECK(ws.e[x] == std::max(wk.e[x], m.bias));
        } else {
            CHECK(std::max(ws.q[x], NWFLOOR + Q_) == wk.q[x]);
            CHECK(ws.e[x] == wk.e[x]);
        }
    }
    if (sw) {
        CHECK(lo >= P16_FLOOR - (W - 1) * p16_abs(C));
        CHECK(lo >= p16_bottom_field(P16_DEF_N, G, Q_, C, W) && hi <= p16_top_field(E_, C, W));
    }
}

int main() {
    // the condition, at every strip width a class compiled for the default scores has (the second width W - 1 included)
    int widths = 0;
    for (const ClassRow& c : kClasses) {
        if (!(c.rms & RM2) || !(c.modes & CLS_DS)) continue;
        for (int w = CLASS_W_MIN; w <= CLASS_W_MAX; ++w) {
            if (!(c.widths & cw(w))) continue;
            ++widths;
            CHECK(w <= P16_W_MAX && p16_strip_q_dominated(G, E_, Q_, C, w));
            if (c.widths2 & cw(w)) CHECK(p16_strip_q_dominated(G, E_, Q_, C, w - 1));
        }
    }
    CHECK(widths > 0);
    // ... and where it ends: g - q = 20 columns between the opening and the cell, a strip of 22
    CHECK(p16_strip_q_dominated(G, E_, Q_, C, 22) && !p16_strip_q_dominated(G, E_, Q_, C, 23));
    CHECK(!p16_strip_q_dominated(-6, -2, -6, -1, CLASS_W_MIN));   // g = q: a score set the generic classes admit
    CHECK(p16_bottom_field(P16_DEF_N, G, Q_, C, P16_W_MAX) == P16_FLOOR - 26);
    // the rows
    for (int W = CLASS_W_MIN; W <= P16_W_MAX; ++W)
        for (int sw = 0; sw < 2; ++sw) {
            for (int kind = 0; kind < 5; ++kind)
                for (int r = 0; r < (kind == 0 ? 1500 : 250); ++r) run_case(sw != 0, W, kind, false);
            if (!sw) for (int r = 0; r < 200; ++r) run_case(false, W, r % 5, true);
        }
    // a control: the carries must matter -- the SHORT form without b in the scan differs from the recurrence on such rows
    {
        const Mode m = mode_of(true);
        std::vector<int> hc(40, m.bias), hp;
        hc[3] = m.bias + 400;   // a spike: 30 columns on, only the long piece still carries it
        std::vector<int> hs, hb;
        Words w;
        int lo = 0, hi = 0;
        row_plain(m, hc, hp);
        CHECK(hp[35] == m.bias + 400 + Q_ + 31 * C && hp[35] > m.bias + 400 + G + 31 * E_);
        row_strips(m, hc, 10, 2, true, hs, w, &lo, &hi);
        row_strips(m, hc, 10, 2, true, hb, w, &lo, &hi, true);
        CHECK(hs == hp && hb != hp);
    }
    printf("%ld %ld\n", n_checks, n_bad);
    return n_bad ? 1 : 0;
}
