// The host rules of the BPE learner (gz_bpe_learn): the refusals, the initial symbols of a word set, the interning of merged
// symbols and the vocabulary's pieces.  No HIP and nothing of the library in this file: tests/test_learn_surface.py builds it into
// a stand-alone program under the sanitizers.  DESIGN.md section 8 states the rule these functions implement.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

constexpr int64_t GZ_LEARN_MERGES_MAX = (int64_t)1 << 20;       // == GZ_BPE_MERGES_MAX of the public header
constexpr int64_t GZ_LEARN_COUNT_LIMIT = (int64_t)1 << 62;      // total counts, and counts x symbols, stay below

// nullptr, or the sentence of the first rule the arguments break
inline const char* learn_args_fault(int64_t n_merges, int64_t min_frequency)
{
    if (n_merges < 0) return "BPE learner needs n_merges >= 0";
    if (n_merges > GZ_LEARN_MERGES_MAX) return "BPE learner takes at most 2^20 merges";
    if (min_frequency < 1) return "BPE learner needs min_frequency >= 1";
    return nullptr;
}

// bytes of the code point that starts at p (n > 0 bytes left): by the lead byte when the continuation bytes are there, else 1 -- a
// byte that starts no well-formed sequence is a symbol of its own
inline int learn_cp_len(const uint8_t* p, int64_t n)
{
    const uint8_t b = p[0];
    const int want = b < 0x80 ? 1 : b >= 0xC2 && b <= 0xDF ? 2 : b >= 0xE0 && b <= 0xEF ? 3 : b >= 0xF0 && b <= 0xF4 ? 4 : 1;
    if (want > n) return 1;
    for (int i = 1; i < want; ++i)
        if ((p[i] & 0xC0) != 0x80) return 1;
    return want;
}

struct LearnHost {
    std::vector<std::string> sym;                               // id -> bytes
    std::unordered_map<std::string, int32_t> ids;               // bytes -> id: a merged symbol whose string exists reuses its id
    std::vector<int32_t> flat;                                  // the words' initial symbols, word d = flat[woff[d] .. woff[d + 1])
    std::vector<uint32_t> woff;
    std::vector<uint32_t> longw;                                // words of more than lane_max symbols
    std::vector<std::pair<int32_t, int32_t>> merges;
    int64_t adjacent = 0;                                       // adjacent positions of the initial state

    // word d = bytes[off[d] .. off[d + 1]) with count cnt[d] >= 1.  The last code point of a word carries "</w>"; ids are the
    // distinct initial strings in ascending byte order.  nullptr, or the refusal.
    const char* init(const uint8_t* bytes, const int64_t* off, const int64_t* cnt, int64_t n, uint32_t lane_max)
    {
        sym.clear(); ids.clear(); flat.clear(); woff.assign(1, 0u); longw.clear(); merges.clear(); adjacent = 0;
        int64_t total = 0, weighted = 0;
        std::string s;
        for (int64_t d = 0; d < n; ++d) {
            const uint8_t* p = bytes + off[d];
            const int64_t len = off[d + 1] - off[d];
            if (len <= 0) return "BPE learner: an empty word";
            if (cnt[d] < 1) return "BPE learner: a word count below 1";
            int64_t k = 0;
            for (int64_t i = 0; i < len;) {
                const int m = learn_cp_len(p + i, len - i);
                s.assign((const char*)p + i, (size_t)m);
                i += m;
                if (i == len) s += "</w>";
                const auto it = ids.emplace(s, (int32_t)sym.size());
                if (it.second) sym.push_back(s);
                if (flat.size() >= (size_t)INT32_MAX) return "BPE learner: more than 2^31 - 1 symbol positions";
                flat.push_back(it.first->second);
                ++k;
            }
            if (cnt[d] >= GZ_LEARN_COUNT_LIMIT - total) return "BPE learner: the counts sum to 2^62 or more";
            total += cnt[d];
            if (cnt[d] > (GZ_LEARN_COUNT_LIMIT - 1 - weighted) / k) return "BPE learner: counts times symbols sum to 2^62 or more";
            weighted += cnt[d] * k;
            adjacent += k - 1;
            if (k > (int64_t)lane_max) longw.push_back((uint32_t)d);
            woff.push_back((uint32_t)flat.size());
        }
        // first-occurrence ids -> ids in byte order (std::string compares as unsigned bytes)
        std::vector<int32_t> order(sym.size()), newid(sym.size());
        for (size_t i = 0; i < order.size(); ++i) order[i] = (int32_t)i;
        std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return sym[(size_t)a] < sym[(size_t)b]; });
        std::vector<std::string> sorted(sym.size());
        for (size_t i = 0; i < order.size(); ++i) {
            newid[(size_t)order[i]] = (int32_t)i;
            sorted[i].swap(sym[(size_t)order[i]]);
        }
        sym.swap(sorted);
        for (size_t i = 0; i < sym.size(); ++i) ids[sym[i]] = (int32_t)i;
        for (int32_t& v : flat) v = newid[(size_t)v];
        return nullptr;
    }

    // the step's merged symbol: left + right, an existing id when that string is a symbol already
    int32_t merge(int32_t l, int32_t r)
    {
        std::string s = sym[(size_t)l] + sym[(size_t)r];
        const auto it = ids.emplace(s, (int32_t)sym.size());
        if (it.second) sym.push_back(std::move(s));
        merges.emplace_back(l, r);
        return it.first->second;
    }

    // hist[2 * id + last]: the count of symbol id at a word's last position (last = 1) or before it (0) in the final segmentation.
    // A piece that is not its word's last is written string + "@@", the last one without its final four bytes; equal strings add
    // up; the five default special strings are left out; largest count first, then ascending bytes.
    void pieces(const int64_t* hist, std::vector<std::pair<std::string, int64_t>>& out) const
    {
        std::unordered_map<std::string, int64_t> sum;
        for (size_t i = 0; i < sym.size(); ++i)
            for (int last = 0; last < 2; ++last) {
                const int64_t c = hist[2 * i + (size_t)last];
                if (c <= 0) continue;
                if (last && sym[i].size() <= 4) continue;
                sum[last ? sym[i].substr(0, sym[i].size() - 4) : sym[i] + "@@"] += c;
            }
        for (const char* sp : {"<pad>", "<s>", "</s>", "<mask>", "<unk>"}) sum.erase(sp);
        out.assign(sum.begin(), sum.end());
        std::sort(out.begin(), out.end(), [](const std::pair<std::string, int64_t>& a, const std::pair<std::string, int64_t>& b) {
            return a.second != b.second ? a.second > b.second : a.first < b.first;
        });
    }
};
