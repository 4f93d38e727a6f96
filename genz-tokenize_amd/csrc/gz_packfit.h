// gz_packfit.h -- the sequential part of best-fit packing, as plain host C++ (no HIP, no context: tests/test_packfit_plan.py compiles
// this file alone).  The kernels are in gz_packfit.inc, the calls in gz_rows_api.inc.
//
// The rule (include/genz_tokenize.h, "best-fit packing"): documents in the order (len descending, index ascending); a document of
// length l goes into the open row with the smallest (free, stamp) among those with free >= l, or opens the next row.
//
// Documents of one length are interchangeable apart from their index, so the decisions collapse onto the length histogram h[0 .. L]:
//   * a row of free space s that takes a document of length l has s - l left, less than any other candidate: it takes
//     k = s / l of them before the next row is touched;
//   * rows that reached the same free space wait in a FIFO queue of SEGMENTS [a, b): contiguous row numbers whose rows were filled
//     alike, one after the other, and hold the same number of documents.
// Per length l from L down to 2, the non-empty free-space classes s = l, l + 1, .. are walked in ascending order (a bitmap finds the
// next one), each queue from its front; what the classes do not take opens new rows with k = L / l.  Every step emits an EVENT: ranks
// [start, start + n_rows * k) of length l go k a row into rows [row, row + n_rows), from column col0 on, behind the `before`
// documents a row already holds.  Every event places a document, so there are at most N of them; in practice a few hundred to a
// few thousand whatever N is.  The segments left in the queues at the end partition [0, R).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

struct GzFitEvent {                     // (32 bytes: the place pass loads an event as two 16-byte words)
    int32_t start;                      // first rank (among the documents of this length, by index) the event places
    int32_t row;                        // first row
    int32_t k;                          // documents of this length a row takes
    int32_t col0;                       // column of the first of them
    int32_t before;                     // documents the row held already
    int32_t n_rows;
    int32_t pad[2];
};
struct GzFitSeg {                       // rows [row, next segment's row) hold `docs` documents each
    int32_t row, docs;
    int64_t base;                       // row_docs index of the first document of row `row`
};
struct GzFitPlan {
    std::vector<GzFitEvent> ev;         // grouped by length, longest first
    std::vector<int32_t> ev_off;        // [L + 2]: the events of length l are ev[ev_off[l + 1] .. ev_off[l])
    std::vector<GzFitSeg> seg;          // sorted by row, then one closing entry {R, 0, N}
    int64_t R = 0;
};

// h[l] = documents of length l (h[0] and h[1] are not read: no document is that short), 3 <= L.  Throws std::bad_alloc.
inline void gz_packfit_plan(const int32_t* h, int32_t L, GzFitPlan& P)
{
    struct Node { int32_t a, b, docs, next; };
    std::vector<Node> nodes;
    std::vector<int32_t> head((size_t)L + 1, -1), tail((size_t)L + 1, -1);
    std::vector<uint64_t> bits((size_t)L / 64 + 1, 0);
    P.ev.clear(); P.seg.clear(); P.ev_off.assign((size_t)L + 2, 0); P.R = 0;
    int64_t R = 0;

    const auto push = [&](int32_t s, int64_t a, int64_t b, int64_t docs) {
        if (tail[s] >= 0 && nodes[tail[s]].b == a && nodes[tail[s]].docs == docs) { nodes[tail[s]].b = (int32_t)b; return; }
        nodes.push_back(Node{(int32_t)a, (int32_t)b, (int32_t)docs, -1});
        const int32_t at = (int32_t)nodes.size() - 1;
        if (tail[s] >= 0) nodes[tail[s]].next = at; else { head[s] = at; bits[s >> 6] |= 1ull << (s & 63); }
        tail[s] = at;
    };
    const auto next_class = [&](int32_t s) -> int32_t {                   // the first non-empty class at or above s, or -1
        for (size_t w = (size_t)s >> 6; w < bits.size(); ++w) {
            const uint64_t m = w == ((size_t)s >> 6) ? bits[w] & (~0ull << (s & 63)) : bits[w];
            if (m) return (int32_t)(w * 64 + (size_t)__builtin_ctzll(m));
        }
        return -1;
    };
    const auto emit = [&](int64_t start, int64_t n_rows, int64_t k, int64_t row, int64_t col0, int64_t before) {
        P.ev.push_back(GzFitEvent{(int32_t)start, (int32_t)row, (int32_t)k, (int32_t)col0, (int32_t)before, (int32_t)n_rows, {0, 0}});
    };

    for (int32_t l = L; l >= 2; --l) {
        P.ev_off[(size_t)l + 1] = (int32_t)P.ev.size();
        int64_t c = h[l], j = 0;
        int32_t s = l;
        while (c > 0 && (s = next_class(s)) >= 0) {
            const int64_t k = s / l;
            const int32_t f = head[s];
            const int64_t a = nodes[f].a, docs = nodes[f].docs;
            const int64_t n_full = std::min<int64_t>(nodes[f].b - a, c / k);
            int64_t used = n_full;
            if (n_full) {
                emit(j, n_full, k, a, L - s, docs);
                push(s - (int32_t)(k * l), a, a + n_full, docs + k);
                j += n_full * k; c -= n_full * k;
            }
            if (c > 0 && c < k && a + n_full < nodes[f].b) {               // fewer than a row takes: one more row takes them all
                emit(j, 1, c, a + n_full, L - s, docs);
                push(s - (int32_t)(c * l), a + n_full, a + n_full + 1, docs + c);
                j += c; c = 0; used += 1;
            }
            nodes[f].a = (int32_t)(a + used);
            if (nodes[f].a == nodes[f].b) {                                 // the front segment is used up
                head[s] = nodes[f].next;
                if (head[s] < 0) { tail[s] = -1; bits[s >> 6] &= ~(1ull << (s & 63)); }
            }
        }
        if (c > 0) {                                                        // new rows
            const int64_t k = L / l, n_full = c / k, rest = c % k;
            if (n_full) {
                emit(j, n_full, k, R, 0, 0);
                push(L - (int32_t)(k * l), R, R + n_full, k);
                j += n_full * k; R += n_full;
            }
            if (rest) {
                emit(j, 1, rest, R, 0, 0);
                push(L - (int32_t)(rest * l), R, R + 1, rest);
                R += 1;
            }
        }
    }
    P.ev_off[1] = P.ev_off[0] = P.ev_off[2] = (int32_t)P.ev.size();
    for (int32_t s = 0; s <= L; ++s)
        for (int32_t f = head[s]; f >= 0; f = nodes[f].next) P.seg.push_back(GzFitSeg{nodes[f].a, nodes[f].docs, nodes[f].b});   // (base: b for now)
    std::sort(P.seg.begin(), P.seg.end(), [](const GzFitSeg& x, const GzFitSeg& y) { return x.row < y.row; });
    int64_t base = 0;
    for (GzFitSeg& g : P.seg) {
        const int64_t rows = g.base - g.row;
        g.base = base;
        base += rows * g.docs;
    }
    P.seg.push_back(GzFitSeg{(int32_t)R, 0, base});
    P.R = R;
}
