// edit_shared.h -- device helpers of the Levenshtein search that edit.hip (tables of any size) and
// small_edit_search.hip (small tables, one workgroup per hash bin) both use: reading a record at any base offset,
// the hash a probe item meets index items under, the item payload, the configuration test of the
// first-matching-configuration rule and the bounded Levenshtein predicate on bit planes. edit.hip's header comment
// explains the scheme.
#pragma once
#include "fqd_internal.h"

namespace {

// 32 bits (or fewer at the key's end) of plane k starting at base `start`.
__device__ __forceinline__ uint32_t plane_bits(const uint32_t *rec, uint32_t K, uint32_t W, uint32_t k,
                                               uint32_t start)
{
    const uint32_t w = start >> 5, sft = start & 31u;
    const uint32_t lo = w < W ? rec[w * K + k] : 0u;
    const uint32_t hi = (w + 1 < W) ? rec[(w + 1) * K + k] : 0u;
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> sft);
}

// The hash fqd_segment_hash gives segment seg of a key of cls_len bases whose segment holds the nb bases that THIS
// record has from base `start` on: the record is read through a window shifted by delta = start - lo, word by word
// in the indexed key's coordinates. With it a probe item meets the index items the Hamming passes have hashed
// already (segment_hashes_kernel), and the edit search need not hash the index side again.
__device__ __forceinline__ uint32_t shifted_segment_hash(const uint32_t *rec, uint32_t K, uint32_t W, uint32_t cls_len,
                                                         uint32_t seg, uint32_t nseg, int delta)
{
    uint32_t lo, hi;
    fqd_segment(cls_len, seg, nseg, lo, hi);
    uint32_t part = 0;
    for (uint32_t w = lo >> 5; w * 32u < hi; w++) {
        const uint32_t m = fqd_range_mask(w, lo, hi);
        if (!m)
            continue;
        const int at = (int)(w * 32u) + delta;                // the record's base under bit 0 of word w
        for (uint32_t k = 0; k < K; k++) {
            const uint32_t bits = at >= 0 ? plane_bits(rec, K, W, k, (uint32_t)at)
                                          : plane_bits(rec, K, W, k, 0u) << (uint32_t)(-at);
            part += fqd_mix32((bits & m) + (w * K + k + 1u) * 0x9E3779B1u);
        }
    }
    return fqd_mix32(part + fqd_mix32(cls_len * 0x9E3779B1u + seg * 0x85EBCA77u + 0x165667B1u));
}

constexpr uint32_t ROLE_PROBE = 0x80000000u;

// item payload = uid (26 bits) | segment (2) | shift + 3 (3) | probe role (1), so d <= 3 and fewer than 2^26 keys
constexpr uint32_t EG_UID_BITS = 26, EG_UID_MASK = (1u << EG_UID_BITS) - 1u;

__device__ __forceinline__ uint32_t eg_payload(uint32_t uid, uint32_t seg, int delta, bool probe)
{
    return uid | (seg << EG_UID_BITS) | ((uint32_t)(delta + 3) << (EG_UID_BITS + 2)) | (probe ? ROLE_PROBE : 0u);
}

// bases [sa, sa + nb) of a  ==  bases [sb, sb + nb) of b ?
__device__ __forceinline__ bool eg_same_substring(const uint32_t *__restrict__ a, uint32_t sa,
                                                  const uint32_t *__restrict__ b, uint32_t sb, uint32_t nb, uint32_t K,
                                                  uint32_t W)
{
    for (uint32_t off = 0; off < nb; off += 32) {
        const uint32_t rem = nb - off;
        const uint32_t mask = rem >= 32 ? 0xFFFFFFFFu : ((1u << rem) - 1u);
        for (uint32_t k = 0; k < K; k++)
            if ((plane_bits(a, K, W, k, sa + off) ^ plane_bits(b, K, W, k, sb + off)) & mask)
                return false;
    }
    return true;
}

// Does configuration (prober a -> indexed b, segment s of b's class, shift delta) match?
__device__ __forceinline__ bool eg_config_matches(const uint32_t *__restrict__ ra, uint32_t la,
                                                  const uint32_t *__restrict__ rb, uint32_t lb, uint32_t s, int delta,
                                                  uint32_t d, uint32_t K, uint32_t W)
{
    uint32_t lo, hi;
    fqd_segment(lb, s, d + 1, lo, hi);
    const int start = (int)lo + delta;
    if (start < 0 || (uint32_t)start + (hi - lo) > la)
        return false;
    return eg_same_substring(ra, (uint32_t)start, rb, lo, hi - lo, K, W);
}

// bases a[i...] and b[j...] agree for how many positions? (bit planes: XOR, OR over the planes, count zeros)
__device__ __forceinline__ uint32_t eg_lcp(const uint32_t *__restrict__ a, uint32_t i, uint32_t la,
                                           const uint32_t *__restrict__ b, uint32_t j, uint32_t lb, uint32_t K, uint32_t W)
{
    const uint32_t n = (la - i) < (lb - j) ? la - i : lb - j;
    for (uint32_t off = 0; off < n; off += 32) {
        uint32_t x = 0;
        for (uint32_t k = 0; k < K; k++)
            x |= plane_bits(a, K, W, k, i + off) ^ plane_bits(b, K, W, k, j + off);
        if (x) {
            const uint32_t t = off + (uint32_t)__ffs((int)x) - 1u;
            return t < n ? t : n;
        }
    }
    return n;
}

// Levenshtein(a, b) <= d for d <= 3 by diagonals (Landau-Vishkin): with e edits, how far down
// diagonal k = j - i does a match run? Every extension is an eg_lcp over whole words -- a few dozen
// word operations per pair where the banded table of within_edit touches every base three times
// through a scratch array (272 ms instead of ~2 for the 11 M candidates of config 5's variant).
// The same predicate as distances.h:33-88.
__device__ bool eg_within_edit(const uint32_t *__restrict__ a, uint32_t la, const uint32_t *__restrict__ b, uint32_t lb,
                               int d, uint32_t K, uint32_t W)
{
    const int goal = (int)lb - (int)la;                  // the diagonal both keys end on
    if (goal > d || -goal > d)
        return false;
    constexpr int NONE = -1000000;
    int prev[7], cur[7];                                 // diagonals -3 .. 3 at index k + 3
#pragma unroll
    for (int t = 0; t < 7; t++)
        prev[t] = NONE;
    prev[3] = (int)eg_lcp(a, 0, la, b, 0, lb, K, W);
    if (goal == 0 && prev[3] >= (int)la)
        return true;
    for (int e = 1; e <= d; e++) {
#pragma unroll
        for (int t = 0; t < 7; t++) {
            const int k = t - 3;
            cur[t] = NONE;
            if (k < -e || k > e)
                continue;
            int row = NONE;
            if (prev[t] != NONE)
                row = prev[t] + 1;                                   // substitution
            if (t + 1 < 7 && prev[t + 1] != NONE && prev[t + 1] + 1 > row)
                row = prev[t + 1] + 1;                               // a base of a skipped
            if (t > 0 && prev[t - 1] != NONE && prev[t - 1] > row)
                row = prev[t - 1];                                   // a base of b skipped
            if (row == NONE)
                continue;
            if (row > (int)la)
                row = (int)la;
            if (row + k > (int)lb)
                row = (int)lb - k;
            if (row < 0 || row + k < 0)
                continue;
            row += (int)eg_lcp(a, (uint32_t)row, la, b, (uint32_t)(row + k), lb, K, W);
            cur[t] = row;
            if (k == goal && row >= (int)la)
                return true;
        }
#pragma unroll
        for (int t = 0; t < 7; t++)
            prev[t] = cur[t];
    }
    return false;
}

}  // namespace
