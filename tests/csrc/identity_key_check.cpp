// TEST HARNESS: the integer arithmetic of decree Q (smoothxg_amd/csrc/poa_identity_key.h, the header the kernels include) on the
// host.  Q2: the key orders (inter, uni) pairs exactly as cross-multiplication orders inter / uni, equal keys mean equal
// fractions, the word (key above uni) gives the counts back; Q3: the rank of the percentile.  Prints "<checks> <failures>".
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../smoothxg_amd/csrc/poa_identity_key.h"

struct pair_t { uint32_t inter, uni; };

// -1 / 0 / +1: a's Jaccard index against b's, a pair without a union counting as 0 / 1
static int cross_cmp(const pair_t a, const pair_t b) {
    const uint64_t an = a.uni ? a.inter : 0, ad = a.uni ? a.uni : 1, bn = b.uni ? b.inter : 0, bd = b.uni ? b.uni : 1;
    const uint64_t l = an * bd, r = bn * ad;
    return l < r ? -1 : l > r ? 1 : 0;
}

int main() {
    long checks = 0, bad = 0;
    std::vector<pair_t> ps;
    const uint32_t unis[] = {0, 1, 2, 3, 129, 255, 256, 257, 32767, 32768, 53246, 65534, 65535};
    for (uint32_t u : unis) {
        const uint32_t inters[] = {0, 1, 2, u / 3, u / 2, u ? u - 1 : 0, u};
        for (uint32_t i : inters)
            if (i <= u) ps.push_back(pair_t{i, u});
    }
    uint64_t x = 0x9E3779B97F4A7C15ull;   // seeded: splitmix64
    auto next = [&]() { x += 0x9E3779B97F4A7C15ull; uint64_t z = x; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); };
    for (int q = 0; q < 1500; ++q) {
        const uint32_t u = (uint32_t)(next() % 65536), i = (uint32_t)(next() % ((uint64_t)u + 1));
        ps.push_back(pair_t{i, u});
        if (u > 1) ps.push_back(pair_t{i ? i - 1 : 1, u - 1});   // neighbours: fractions that differ by about 1 / uni^2
    }
    for (int q = 0; q < 300; ++q) {                               // the closest two fractions can be: a / b and c / d with |ad - bc| = 1
        const uint32_t b = 65535 - (uint32_t)(next() % 200), a = (uint32_t)(next() % b);
        ps.push_back(pair_t{a, b});
        ps.push_back(pair_t{a, b - 1});
    }
    for (const pair_t p : ps) {
        ++checks;
        uint32_t i = ~0u, u = ~0u;
        const uint64_t w = sxg_identity_word(p.inter, p.uni);
        sxg_identity_counts(w, &i, &u);
        if (i != p.inter || u != p.uni || (w >> SXG_IDENT_WORD_BITS) != 0 || (w >> SXG_IDENT_UNI_BITS) != sxg_identity_key(p.inter, p.uni)) {
            ++bad;
            fprintf(stderr, "word of (%u, %u) gives (%u, %u)\n", p.inter, p.uni, i, u);
        }
    }
    for (const pair_t a : ps)
        for (const pair_t b : ps) {
            ++checks;
            const uint64_t ka = sxg_identity_key(a.inter, a.uni), kb = sxg_identity_key(b.inter, b.uni);
            const int kc = ka < kb ? -1 : ka > kb ? 1 : 0;
            if (kc != cross_cmp(a, b)) {
                ++bad;
                if (bad < 20) fprintf(stderr, "(%u, %u) against (%u, %u): keys say %d, fractions %d\n", a.inter, a.uni, b.inter, b.uni, kc, cross_cmp(a, b));
            }
            // the words order by key first: they never contradict the fractions
            const uint64_t wa = sxg_identity_word(a.inter, a.uni), wb = sxg_identity_word(b.inter, b.uni);
            if ((wa < wb && cross_cmp(a, b) > 0) || (wa > wb && cross_cmp(a, b) < 0)) ++bad;
        }
    const uint64_t P[] = {1, 2, 3, 4, 66, 499500}, want[] = {0, 0, 0, 0, 19, 149849};   // (size_t)((double)(P - 1) * 0.30)
    for (int q = 0; q < 6; ++q) {
        ++checks;
        if (sxg_identity_idx(P[q], 0.30) != want[q] || sxg_identity_idx(P[q], 0.0) != 0 || sxg_identity_idx(P[q], 1.0) != P[q] - 1) {
            ++bad;
            fprintf(stderr, "idx(%llu) = %llu\n", (unsigned long long)P[q], (unsigned long long)sxg_identity_idx(P[q], 0.30));
        }
    }
    for (int64_t n = 2; n < 70; ++n) {      // the row starts enumerate the pairs i < j in row-major order
        int64_t q = 0;
        for (int64_t i = 0; i + 1 < n; ++i) {
            ++checks;
            if (sxg_identity_row_start(i, n) != q) ++bad;
            q += n - 1 - i;
        }
        if (q != n * (n - 1) / 2) ++bad;
    }
    printf("%ld %ld\n", checks, bad);
    return bad ? 1 : 0;
}
