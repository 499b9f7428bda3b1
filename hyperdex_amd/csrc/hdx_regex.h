// hdx_regex.h — regex_match of common/regex_match.cc as a set-of-positions
// simulation: one parse of the pattern into a program (host), one step per
// text byte (host and device: hdx_cpu.cpp and hdx_check_eval.h run this very
// code, so the CPU form and the kernels cannot drift apart).  No HIP header:
// hdx_cpu.cpp includes it.
//
// The reference recurses and backtracks (anchored() / starred()); the language
// it accepts is regular.  After an optional leading '^' the pattern is read
// left to right into items:
//   \c                LIT(c)          a trailing lone \   DEAD: matches nothing
//   x*                STAR(x), x any byte but \ ('.': STAR(any); '^', '$', '*' are bytes here)
//   $ as the last byte  END: true iff the text is used up
//   .                 ANY             anything else       LIT
// When the items run out the match succeeds whatever text remains; without '^'
// every start position up to and including the text's end is tried.
//
// State: bit j = "items 0..j-1 matched at some tried start"; bit n (n = the
// items before END) = accepted.  Per byte b with class mask T[b] (the items b
// satisfies): LIT/ANY items move their bit up by one, STAR items keep theirs,
// bit 0 comes back when unanchored, and a STAR's bit also stands for the item
// behind it (the star matched nothing more): closed over a run of stars by one
// addition, the carry running up the run.
#pragma once

#include <stdint.h>

#include "../../include/hdxhash.h"

#ifdef __HIPCC__
#define HDX_RX_HD __host__ __device__
#else
#define HDX_RX_HD
#endif

namespace hdx {

struct RegexProg {
    uint64_t any;    // bit j: item j takes every byte (ANY, STAR(any))
    uint64_t star;   // bit j: item j is a STAR
    uint64_t dead;   // bit j: item j is DEAD
    uint8_t lit[HDX_REGEX_ITEMS_MAX];  // item j's byte where it is neither any nor dead
    uint8_t n;         // items before END: bit n accepts
    uint8_t anchored;  // a leading ^
    uint8_t end;       // END behind the items
    uint8_t pad_[5];
};
static_assert(sizeof(RegexProg) == 96, "the programs travel in the kernel arguments");

// The pattern's program; false where it has more than HDX_REGEX_ITEMS_MAX items (END counts).
inline bool regex_parse(const uint8_t* re, uint64_t len, RegexProg* g) {
    *g = RegexProg{};
    uint64_t i = 0;
    if (len && re[0] == '^') {
        g->anchored = 1;
        i = 1;
    }
    uint32_t n = 0;
    while (i < len) {
        if (n == HDX_REGEX_ITEMS_MAX) return false;
        const uint8_t ch = re[i];
        const uint64_t bit = 1ull << n;
        if (ch == '\\') {
            if (i + 1 < len)
                g->lit[n] = re[i + 1];
            else
                g->dead |= bit;
            i += 2;
        } else if (i + 1 < len && re[i + 1] == '*') {
            g->star |= bit;
            if (ch == '.')
                g->any |= bit;
            else
                g->lit[n] = ch;
            i += 2;
        } else if (ch == '$' && i + 1 == len) {
            g->end = 1;  // not among the n items: it takes no byte
            break;
        } else {
            if (ch == '.')
                g->any |= bit;
            else
                g->lit[n] = ch;
            i += 1;
        }
        ++n;
    }
    g->n = (uint8_t)n;
    return true;
}

// The items byte b satisfies.
HDX_RX_HD inline uint64_t regex_class(const RegexProg& g, uint32_t b) {
    uint64_t m = g.any;
    for (uint32_t j = 0; j < g.n; ++j)
        if (g.lit[j] == b) m |= 1ull << j;
    return m & ~g.dead;  // a DEAD item's lit is 0: byte 0 does not satisfy it either
}

// s and, for every STAR whose bit is set, the bits up to the first item behind its run of stars.
HDX_RX_HD inline uint64_t regex_close(const RegexProg& g, uint64_t s) { return s | (((s & g.star) + g.star) ^ g.star); }

HDX_RX_HD inline uint64_t regex_start(const RegexProg& g) { return regex_close(g, 1); }

// The state behind a byte of class mask t.
HDX_RX_HD inline uint64_t regex_step(const RegexProg& g, uint64_t s, uint64_t t) {
    const uint64_t adv = s & t;
    return regex_close(g, ((adv & ~g.star) << 1) | (adv & g.star) | (g.anchored ? 0 : 1));
}

// The items have run out: true whatever text remains (never with END, which needs the text's end).
HDX_RX_HD inline bool regex_accepted(const RegexProg& g, uint64_t s) { return !g.end && ((s >> g.n) & 1); }

// At the text's end.
HDX_RX_HD inline bool regex_at_end(const RegexProg& g, uint64_t s) { return (s >> g.n) & 1; }

}  // namespace hdx
