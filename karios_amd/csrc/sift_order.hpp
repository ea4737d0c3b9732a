// The final order of SIFT's key points on the host (removeDuplicatedSorted: sf::key_less, then a key point that equals its
// predecessor in x, y, size and angle is dropped).  Host only; compiled by hipcc into api_sift.hip and by g++ for the CPU suite.
//
// One std::sort on sf::key_less over 3 M records costs 0.5 s on one core (profiles/sift_probe.json before this file), most of it
// cache misses of the comparator.  x and y of a key point are positive finite floats - it lies inside the border - and the bit
// patterns of such floats order as their values do.  So a stable radix sort on the 64-bit word (x bits, y bits) puts the records in
// (x, y) order in a few linear passes, and only the runs that share one point (the orientations of one candidate: a few records)
// go through sf::key_less.  The result is the order of the single sort with the record's index as the last word; key points equal
// in all six fields are one record, their mutual order cannot show.  A record whose x or y is not positive and finite sends the
// whole list through the single sort.
#pragma once
#include "sift_math.hpp"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace sf {

struct order_item {
    uint64_t word;     // x bits << 32 | y bits
    int index;
};

inline bool index_less(const Key *keys, int a, int b)
{
    if (key_less(keys[a], keys[b])) return true;
    if (key_less(keys[b], keys[a])) return false;
    return a < b;
}

// perm: the indices of the records that stay, in the final order
inline void final_order(const Key *keys, size_t n, std::vector<int> &perm)
{
    const int DIGIT = 11, N_DIGITS = 6, BUCKETS = 1 << DIGIT;        // 6 x 11 bits cover the 64
    std::vector<int> order(n);
    std::vector<order_item> a(n), b;
    bool plain = true;
    for (size_t i = 0; i < n; i++) {
        uint32_t xb, yb;
        memcpy(&xb, &keys[i].x, 4);
        memcpy(&yb, &keys[i].y, 4);
        plain = plain && xb - 1u < 0x7f7fffffu && yb - 1u < 0x7f7fffffu;      // 0 < value < infinity, not NaN
        a[i].word = (uint64_t)xb << 32 | yb;
        a[i].index = (int)i;
    }
    if (!plain) {
        for (size_t i = 0; i < n; i++) order[i] = (int)i;
        std::sort(order.begin(), order.end(), [&](int p, int q) { return index_less(keys, p, q); });
    } else {
        std::vector<size_t> hist((size_t)N_DIGITS * BUCKETS, 0);
        for (size_t i = 0; i < n; i++)
            for (int d = 0; d < N_DIGITS; d++) hist[(size_t)d * BUCKETS + ((a[i].word >> (DIGIT * d)) & (BUCKETS - 1))]++;
        b.resize(n);
        for (int d = 0; d < N_DIGITS; d++) {
            size_t *h = &hist[(size_t)d * BUCKETS];
            if (n && h[(a[0].word >> (DIGIT * d)) & (BUCKETS - 1)] == n) continue;     // one value of this digit: nothing moves
            size_t at = 0;
            for (int k = 0; k < BUCKETS; k++) { const size_t c = h[k]; h[k] = at; at += c; }
            for (size_t i = 0; i < n; i++) b[h[(a[i].word >> (DIGIT * d)) & (BUCKETS - 1)]++] = a[i];
            a.swap(b);
        }
        for (size_t i = 0; i < n; i++) order[i] = a[i].index;
        for (size_t i = 0; i < n;) {                                                       // the runs of one point
            size_t j = i + 1;
            while (j < n && a[j].word == a[i].word) j++;
            if (j - i > 1) std::sort(order.begin() + (ptrdiff_t)i, order.begin() + (ptrdiff_t)j, [&](int p, int q) { return index_less(keys, p, q); });
            i = j;
        }
    }
    perm.clear();
    perm.reserve(n);
    for (size_t i = 0; i < n; i++)
        if (i == 0 || !key_duplicate(keys[order[i]], keys[order[i - 1]])) perm.push_back(order[i]);
}

}  // namespace sf
