// group_inplace.hip -- the partitioned Hamming search (group.hip) for records of ONE uint4, without candidate lists:
// the wave that sub-sorts a bucket's (segment hash, position) items in LDS also stages the bucket's 16-byte records
// there and verifies every pair of equal hashes where it finds it -- distance, first-agreeing-segment rule, edge out.
// A record is as small as the two list entries that would name a pair, so the list, its budget and the second search
// that follows an outgrown budget (the sort path: d + 1 device-wide sorts) have no reason to exist for these keys.
// Same contract as grouped_candidates_kernel + verify_candidates_kernel: every pair within d is reported once, in the
// pass of the FIRST segment it agrees on (reference _triemodule.c:807-895).
//
// Work split: persistent grid, one wave per bucket, four waves per workgroup, waves share nothing but the segment
// masks (written once before the only workgroup barrier, at the start). bucket_start / bucket_end (slab mode) /
// skip[] (crowded buckets: theirs are the refinement's or the tiles') mean what they mean to the candidates kernel.
//
// LDS per wave, slice of 512 items:        hashes 2048 + uid|segment 2048 + records 8192 + sub-bin starts 264
//                                          + edge buffer 80 x 8 = 640 + control 8            = 13 200 B
//   ragged tables add the lengths, one byte each (a one-uint4 key is at most 128 nt):  + 512  = 13 712 B
// per workgroup (4 waves + 128 B of masks): 52 928 B -> 3 workgroups = 12 waves per CU of 160 KB; ragged: 54 976 B -> 2.
// 512 items: a bucket of the fused passes averages ~430 and is marked crowded from 512-1024 on, so nearly every
// bucket that reaches this kernel is staged whole; 1024 would leave one workgroup per CU. The item's segment rides in
// the top 3 bits of its uid word (tables of 2^29 keys and more keep the list path), so "same segment" costs no array.
#include "fqd_internal.h"

namespace {

constexpr uint32_t GI_THREADS = 256;
constexpr uint32_t GI_SLICE = 512;      // items of one bucket staged per wave
constexpr uint32_t GI_PER = GI_SLICE / 64;
constexpr uint32_t GI_WCAP = 80;        // edges buffered per wave (>= 64: every lane may note one at once)
constexpr uint32_t GI_UID_BITS = 29, GI_UID_MASK = (1u << GI_UID_BITS) - 1u;

template <int K>
struct GiXor {
    static constexpr uint32_t WMAX = 4 / K;     // 32-base words a one-uint4 record of K planes can hold
    uint32_t dw[WMAX];
    // OR over the planes of a ^ b, per 32-base word; returns the mismatches of the first W words
    __device__ __forceinline__ uint32_t set(const uint4 &a, const uint4 &b, uint32_t W)
    {
        const uint32_t x[4] = {a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w};
        uint32_t dist = 0;
#pragma unroll
        for (uint32_t w = 0; w < WMAX; w++) {
            uint32_t v = 0;
#pragma unroll
            for (int k = 0; k < K; k++)
                v |= x[w * K + k];
            dw[w] = w < W ? v : 0u;
            dist += __popc(dw[w]);
        }
        return dist;
    }
};

template <int K, bool RAGGED>
__global__ __launch_bounds__(GI_THREADS) void grouped_inplace_kernel(
    const uint2 *__restrict__ items, const uint32_t *__restrict__ bucket_start,
    const uint32_t *__restrict__ bucket_end /* NULL, or slab mode: where each bucket's cursor stopped */,
    uint32_t n_buckets, uint32_t sub_shift, const uint8_t *__restrict__ skip /* NULL, or skip[b] != 0: a crowded bucket */,
    uint32_t give_up_over, unsigned long long *__restrict__ cand_need /* give_up_over != 0: a bucket of more items is not
                          * walked but reported as a need beyond every budget, as by the candidates kernel */,
    const uint4 *__restrict__ recs4, const uint32_t *__restrict__ ulens, KeyShape sh, uint32_t d, uint32_t seg0,
    uint32_t nseg, uint32_t *__restrict__ edges, unsigned long long *__restrict__ edge_count, uint64_t edge_cap,
    fqd::PairStats *__restrict__ stats,
    uint32_t fused_U /* != 0: ALL passes in one -- an item's value is segment * fused_U + uid, its pass seg0 + segment */)
{
    constexpr uint32_t WAVES = GI_THREADS / 64, WMAX = GiXor<K>::WMAX;
    __shared__ __attribute__((aligned(16))) uint32_t s_hash[WAVES][GI_SLICE];
    __shared__ __attribute__((aligned(16))) uint4 s_rec[WAVES][GI_SLICE];
    __shared__ uint32_t s_uid[WAVES][GI_SLICE];          // uid | segment << 29
    __shared__ uint8_t s_len[WAVES][RAGGED ? GI_SLICE : 1];
    __shared__ uint32_t s_off[WAVES][66];                // sub-bin counts, then sub-bin starts (64 + end)
    __shared__ uint2 s_wbuf[WAVES][GI_WCAP];
    __shared__ uint32_t s_wcnt[WAVES];
    __shared__ uint32_t s_mask[8][4];                    // keys of max_len: the bits of word w inside segment s2
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t *hashes = s_hash[wave], *uids = s_uid[wave], *off = s_off[wave];
    uint4 *recs = s_rec[wave];
    uint8_t *lens = s_len[wave];
    uint2 *wbuf = s_wbuf[wave];
    const uint32_t W = sh.words;
    // (written by the leader lane, read by all: relaxed workgroup-scope atomics, as in grouped_candidates_kernel)
    auto ld_shared = [](uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
    auto st_shared = [](uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };

    if (tid < 32) {
        uint32_t slo = 0, shi = 0;
        const uint32_t s2 = tid >> 2, w = tid & 3u;
        if (s2 < nseg)
            fqd_segment(sh.max_len, s2, nseg, slo, shi);
        s_mask[s2][w] = s2 < nseg ? fqd_range_mask(w, slo, shi) : 0u;
    }
    if (lane == 0)
        st_shared(&s_wcnt[wave], 0u);
    __syncthreads();
    const bool fast_masks = nseg <= 8;
    unsigned long long n_pairs = 0, n_hits = 0, n_recs = 0;

    // the wave's buffer -> the edge list, ONE addition to the counter (which keeps counting past edge_cap)
    auto flush = [&](uint32_t have, uint32_t n, uint32_t rank, int leader) {
        unsigned long long g = 0;
        if ((int)lane == leader)
            g = atomicAdd(edge_count, (unsigned long long)have);
        g = __shfl(g, leader);
        for (uint32_t e = rank; e < have; e += n)
            if (g + e < edge_cap)
                reinterpret_cast<uint2 *>(edges)[g + e] = wbuf[e];
    };
    // called by whatever lanes are active at the call site (converged there): they take consecutive slots
    auto note = [&](uint32_t a, uint32_t b) {
        const unsigned long long act = __ballot(1);
        const uint32_t n = (uint32_t)__popcll(act), rank = (uint32_t)__popcll(act & fqd_lanemask_lt());
        const int leader = __ffsll((long long)act) - 1;
        uint32_t have = ld_shared(&s_wcnt[wave]);
        if (have + n > GI_WCAP) {
            flush(have, n, rank, leader);
            have = 0;
        }
        wbuf[have + rank] = make_uint2(a < b ? a : b, a < b ? b : a);
        if ((int)lane == leader)
            st_shared(&s_wcnt[wave], have + n);
    };
    // position in the [n_pass][fused_U] hash array -> uid | segment << 29 (n_pass <= 8: at most 7 steps, once per item)
    auto split = [&](uint32_t pos) {
        uint32_t sg = 0;
        if (fused_U)
            while (pos >= fused_U) {
                pos -= fused_U;
                sg++;
            }
        return pos | (sg << GI_UID_BITS);
    };
    // a pair of equal hashes, equal segments and equal lengths whose XOR words are in x: within d, and agreeing on no
    // segment before its own (an empty segment agrees trivially, as in gp_verify)
    auto first_agreeing = [&](const GiXor<K> &x, uint32_t len, uint32_t cseg) {
        if (fast_masks && len == sh.max_len) {
            bool ok = true;
#pragma unroll
            for (uint32_t s2 = 0; s2 < 8; s2++) {
                uint32_t mis = 0;
#pragma unroll
                for (uint32_t w = 0; w < WMAX; w++)
                    mis |= x.dw[w] & s_mask[s2][w];
                ok = ok && (s2 >= cseg || mis != 0);
            }
            return ok;
        }
        for (uint32_t s2 = 0; s2 < cseg; s2++) {       // (another length, or more than 8 segments: its own masks)
            uint32_t slo, shi, mis = 0;
            fqd_segment(len, s2, nseg, slo, shi);
#pragma unroll
            for (uint32_t w = 0; w < WMAX; w++)
                mis |= x.dw[w] & fqd_range_mask(w, slo, shi);
            if (!mis)
                return false;
        }
        return true;
    };
    auto verify = [&](const uint4 &a, const uint4 &b, uint32_t ua, uint32_t ub, uint32_t len_a, uint32_t len_b) {
        n_pairs++;
        if (((ua ^ ub) >> GI_UID_BITS) || len_a != len_b)      // (hashes of different segments meet only by collision)
            return;
        GiXor<K> x;
        if (x.set(a, b, W) > d || !first_agreeing(x, len_a, seg0 + (ua >> GI_UID_BITS)))
            return;
        n_hits++;
        note(ua & GI_UID_MASK, ub & GI_UID_MASK);
    };

    for (uint32_t b = blockIdx.x * WAVES + wave; b < n_buckets; b += gridDim.x * WAVES) {
        uint32_t two = 0;
        if (lane < 2)
            two = bucket_start[b + lane];
        const uint32_t lo = __shfl(two, 0);
        uint32_t hi = __shfl(two, 1);
        if (bucket_end)
            hi = min(hi, bucket_end[b]);
        const uint32_t m = hi - lo;
        if (m < 2 || (skip && skip[b]))
            continue;
        if (give_up_over && m > give_up_over) {
            if (lane == 0)
                atomicMax(cand_need, 1ull << 62);
            continue;
        }
        const uint2 *bucket = items + lo;
        const uint32_t m_lds = m < GI_SLICE ? m : GI_SLICE;
        // ---- load (all of the lane's items in flight before anything else), rank, scan, place
        uint2 v[GI_PER];
        uint32_t rank[GI_PER], at[GI_PER];
#pragma unroll
        for (uint32_t k = 0; k < GI_PER; k++) {
            v[k] = make_uint2(0, 0);
            if (lane + 64 * k < m_lds)
                v[k] = bucket[lane + 64 * k];
        }
        off[lane] = 0;
#pragma unroll
        for (uint32_t k = 0; k < GI_PER; k++) {
            v[k].y = split(v[k].y);
            if (lane + 64 * k < m_lds)
                rank[k] = atomicAdd(&off[(v[k].x >> sub_shift) & 63u], 1u);
        }
        const uint32_t my_count = off[lane];
        {
            uint32_t incl = my_count;
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t up = __shfl_up(incl, o);
                if ((int)lane >= o)
                    incl += up;
            }
            off[lane] = incl - my_count;      // start of sub-bin `lane`
            if (lane == 63)
                off[64] = incl;               // = m_lds
        }
        // ---- the records of the lane's items, all requested before any is used. An item alone in its sub-bin has no
        // partner and fetches nothing -- unless the bucket has a tail, whose items are compared against every staged one.
        uint4 r[GI_PER];
        uint32_t ln[GI_PER];
#pragma unroll
        for (uint32_t k = 0; k < GI_PER; k++) {
            const uint32_t sb = (v[k].x >> sub_shift) & 63u;
            at[k] = GI_SLICE;                 // (no item)
            r[k] = make_uint4(0, 0, 0, 0);
            ln[k] = 0;
            if (lane + 64 * k < m_lds) {
                const uint32_t first = off[sb];
                at[k] = first + rank[k];
                if (m > GI_SLICE || off[sb + 1] - first > 1) {
                    r[k] = recs4[v[k].y & GI_UID_MASK];
                    if (RAGGED)
                        ln[k] = ulens[v[k].y & GI_UID_MASK];
                    n_recs++;
                }
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < GI_PER; k++)
            if (at[k] < GI_SLICE) {
                hashes[at[k]] = v[k].x;
                uids[at[k]] = v[k].y;
                recs[at[k]] = r[k];
                if (RAGGED)
                    lens[at[k]] = (uint8_t)ln[k];
            }
        // (same wave wrote what it now reads: the LDS keeps a wave's accesses in order)
        // ---- every item against the items after it in its sub-bin: hashes first, records on a match
        for (uint32_t i = lane; i < m_lds; i += 64) {
            const uint32_t h = hashes[i];
            const uint32_t end = off[((h >> sub_shift) & 63u) + 1];
            if (i + 1 >= end)
                continue;
            const uint32_t ui = uids[i];
            const uint4 mine = recs[i];
            const uint32_t my_len = RAGGED ? lens[i] : sh.max_len;
            // windows of 8 hashes, 16-byte aligned, no branch per read
            for (uint32_t jbase = (i + 1) & ~3u; jbase < end; jbase += 8) {
                const uint32_t j1 = jbase + 4 < GI_SLICE ? jbase + 4 : GI_SLICE - 4;   // stay inside the slice
                const uint4 a = *reinterpret_cast<const uint4 *>(hashes + jbase);
                const uint4 c4 = *reinterpret_cast<const uint4 *>(hashes + j1);
                uint32_t match = (a.x == h ? 1u : 0u) | (a.y == h ? 2u : 0u) | (a.z == h ? 4u : 0u) |
                                 (a.w == h ? 8u : 0u) | (c4.x == h ? 16u : 0u) | (c4.y == h ? 32u : 0u) |
                                 (c4.z == h ? 64u : 0u) | (c4.w == h ? 128u : 0u);
                const uint32_t first = i + 1 > jbase ? i + 1 - jbase : 0u;      // < 4
                const uint32_t stop = end - jbase;                              // >= 1
                match &= 0xFFu << first;
                if (stop < 8)
                    match &= (1u << stop) - 1u;
                while (match) {
                    const uint32_t j = jbase + (uint32_t)__ffs((int)match) - 1u;
                    match &= match - 1;
                    verify(mine, recs[j], ui, uids[j], my_len, RAGGED ? lens[j] : my_len);
                }
            }
        }
        // ---- a bucket larger than the slice (no marking, or exact sizes under the crowded limit): its tail against the
        // staged part and against itself, items and records from global memory -- correct, not fast
        for (uint32_t t = GI_SLICE + lane; t < m; t += 64) {
            const uint2 me = bucket[t];
            const uint32_t um = split(me.y);
            const uint4 mine = recs4[um & GI_UID_MASK];
            const uint32_t my_len = RAGGED ? ulens[um & GI_UID_MASK] : sh.max_len;
            n_recs++;
            const uint32_t sb = (me.x >> sub_shift) & 63u;
            for (uint32_t j = off[sb]; j < off[sb + 1]; j++)
                if (hashes[j] == me.x)
                    verify(recs[j], mine, uids[j], um, RAGGED ? lens[j] : my_len, my_len);
            for (uint32_t t2 = t + 1; t2 < m; t2++) {
                const uint2 it = bucket[t2];
                if (it.x != me.x)
                    continue;
                const uint32_t uo = split(it.y);
                n_recs++;
                verify(mine, recs4[uo & GI_UID_MASK], um, uo, my_len, RAGGED ? ulens[uo & GI_UID_MASK] : my_len);
            }
        }
    }
    // what is left in the wave's buffer (all lanes are back together here)
    {
        const uint32_t have = ld_shared(&s_wcnt[wave]);
        if (have)
            flush(have, 64, lane, 0);
    }
    if (stats) {
        for (int o = 32; o; o >>= 1) {
            n_pairs += __shfl_xor(n_pairs, o);
            n_hits += __shfl_xor(n_hits, o);
            n_recs += __shfl_xor(n_recs, o);
        }
        if (lane == 0 && (n_pairs | n_recs)) {
            fqd::PairStats *slot = stats + ((blockIdx.x * WAVES + wave) % FQD_STAT_SLOTS);
            atomicAdd(&slot->pairs_compared, n_pairs);
            atomicAdd(&slot->keys_gathered, n_recs);
            if (n_hits)
                atomicAdd(&slot->edges, n_hits);
        }
    }
}

}  // namespace

namespace fqd {

// records of one uint4 whose K planes x W words fit it, uids that leave the top 3 bits to the item's segment
bool group_inplace_possible(KeyShape sh, uint64_t U, uint32_t n_pass_fused)
{
    return sh.stride == 4 && sh.planes >= 1 && sh.planes <= 4 && sh.planes * sh.words <= 4 && sh.max_len <= 128 &&
           U <= GI_UID_MASK && n_pass_fused <= 8;
}

hipError_t launch_grouped_inplace(const uint32_t *items, const uint32_t *bucket_start, const uint32_t *bucket_end,
                                  uint32_t n_buckets, uint32_t bucket_bits, const uint8_t *skip, uint32_t give_up_over,
                                  unsigned long long *cand_need, const uint32_t *urecs, const uint32_t *ulens, KeyShape sh,
                                  uint32_t d, uint32_t seg, uint32_t nseg, uint32_t *edges,
                                  unsigned long long *edge_count, uint64_t edge_cap, PairStats *stats, hipStream_t st,
                                  uint32_t fused_U)
{
    if (!n_buckets)
        return hipSuccess;
    if (sh.stride != 4 || sh.planes * sh.words > 4 || sh.max_len > 128 || bucket_bits > 26)
        return hipErrorInvalidValue;
    const uint32_t sub_shift = 32u - bucket_bits - 6u;      // the 6 hash bits below the bucket bits pick the sub-bin
    const uint32_t blocks = (n_buckets + 3) / 4;
    const unsigned grid = blocks < 8192 ? blocks : 8192;
#define FQD_GI_CASE(KK)                                                                                              \
    case KK:                                                                                                         \
        if (sh.ragged)                                                                                               \
            grouped_inplace_kernel<KK, true><<<grid, GI_THREADS, 0, st>>>(                                           \
                reinterpret_cast<const uint2 *>(items), bucket_start, bucket_end, n_buckets, sub_shift, skip,        \
                cand_need ? give_up_over : 0u, cand_need, reinterpret_cast<const uint4 *>(urecs), ulens, sh, d, seg, \
                nseg, edges, edge_count, edge_cap, stats, fused_U);                                                  \
        else                                                                                                         \
            grouped_inplace_kernel<KK, false><<<grid, GI_THREADS, 0, st>>>(                                          \
                reinterpret_cast<const uint2 *>(items), bucket_start, bucket_end, n_buckets, sub_shift, skip,        \
                cand_need ? give_up_over : 0u, cand_need, reinterpret_cast<const uint4 *>(urecs), ulens, sh, d, seg, \
                nseg, edges, edge_count, edge_cap, stats, fused_U);                                                  \
        break;
    switch (sh.planes) {
        FQD_GI_CASE(1)
        FQD_GI_CASE(2)
        FQD_GI_CASE(3)
        FQD_GI_CASE(4)
    default:
        return hipErrorInvalidValue;
    }
#undef FQD_GI_CASE
    return hipGetLastError();
}

}  // namespace fqd
