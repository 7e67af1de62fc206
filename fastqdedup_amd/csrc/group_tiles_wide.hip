// group_tiles_wide.hip -- the partitioned Hamming search's last resort (group.hip: ALL PAIRS of a crowded bucket in
// 128 x 128 tiles over the whole GPU) for the record shapes gp_crowded_tiles_kernel<K, Q4> does not take: any number of
// uint4 per record up to 16 (256 bytes: 200-, 250-, 500- and 600-nt keys over "ACGNT" are 6, 6, 12 and 15), and
// alphabets of 1 to 4 bit planes. Same inputs and work list (gp_tile_prefix_kernel, list / counts, the upper triangle
// of tile pairs per bucket, persistent grid), same pair rule -- equal item hash and pass, not the same key, k > tid on
// the diagonal tile, 0 < dist <= d, equal lengths when ragged, reported only in the pass of the FIRST main segment the
// pair agrees on (reference _triemodule.c:807-895) -- and the same edge path (per-wave LDS buffer, one atomic per flush,
// counting past edge_cap, PairStats).
//
// Work split: a workgroup of 128 lanes per pair of tiles. A lane keeps ITS row of tile i in registers, uint4 mine[QMAX];
// tile j's rows are staged in LDS at a stride of q4 + 1 uint4 and read by broadcast ds_read_b128. q4 = stride / 4 is a
// RUN-TIME value <= QMAX: QMAX comes from five classes (4, 6, 8, 12, 16), so the unit holds 4 planes x 5 classes = 20
// kernels and not one per (K, q4). Register slots from q4 on are zero on both sides, never loaded and never read from
// LDS (wave-uniform branches on q4); the distance is taken over the K * W key words alone, so padding words -- zero, or
// a ragged key's length -- are never compared.
//
// Long rows (classes of 8 uint4 and more) are read and compared in two halves: random members of a crowded bucket share
// one segment and differ everywhere else, so most pairs are beyond d after the first half, and when that holds for every
// lane of the wave (a ballot) the second half is not read at all.
//
// LDS per workgroup (static): rows 128 x (QMAX + 1) x 16 + items 3 x 512 + edge buffers 2 x 192 x 8 + 8:
// 14 856 B at QMAX = 4, 39 432 B at QMAX = 16 -- under 48 KB for every class, three workgroups share a CU's 160 KB.
#include "fqd_internal.h"

#ifndef FQD_WIDE_TILES_HALVES
#define FQD_WIDE_TILES_HALVES 1      // 0: a whole row at once in every class (the A/B of BASELINE.md section 9)
#endif

namespace {

constexpr uint32_t WT_TS = 128, WT_WCAP = 192;

template <uint32_t K, uint32_t QMAX>
__global__ __launch_bounds__(WT_TS) void gp_wide_tiles_kernel(
    const uint2 *__restrict__ items, const uint32_t *__restrict__ bucket_start, const uint32_t *__restrict__ bucket_end,
    const uint32_t *__restrict__ list, const unsigned long long *__restrict__ counts,
    const unsigned long long *__restrict__ tile_prefix, uint32_t fused_U, uint32_t seg0,
    const uint32_t *__restrict__ urecs, const uint32_t *__restrict__ ulens, KeyShape sh, uint32_t d, uint32_t nseg,
    uint32_t *__restrict__ edges, unsigned long long *__restrict__ edge_count, uint64_t edge_cap,
    fqd::PairStats *__restrict__ stats /* NULL, or stats[slot].edges += pairs reported */)
{
    constexpr uint32_t WMAX = QMAX * 4 / K;               // (words of 32 bases a record of QMAX uint4 can hold)
    constexpr bool HALVES = QMAX >= 8 && FQD_WIDE_TILES_HALVES;
    constexpr uint32_t H = HALVES ? QMAX / 2 : QMAX;      // uint4 of a row read first ...
    constexpr uint32_t WH = H * 4 / K;                    // ... and the 32-base words that lie wholly inside them
    __shared__ uint4 rec_j[WT_TS * (QMAX + 1)];
    __shared__ uint32_t h_j[WT_TS], uid_j[WT_TS], seg_j[WT_TS];
    __shared__ uint2 wbuf[WT_TS / 64][WT_WCAP];
    __shared__ uint32_t s_wn[WT_TS / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    // The unrolled loops below branch on q4 and W, slot by slot and chunk by chunk. Left to itself the compiler works
    // every one of those wave-uniform tests out once, ahead of all loops, and keeps the results as 64-bit lane masks: more
    // than a hundred scalar registers, spilled into vector lanes. The values are therefore made opaque where they are used
    // (an empty asm), so that each test is a scalar compare and a branch at its place.
    uint32_t W = sh.words, q4 = sh.stride / 4;
    const uint32_t row4 = q4 + 1;
    uint32_t my_hits = 0;
    if (lane == 0)
        s_wn[wave] = 0;
    // The starts of main segments 1 .. nseg of a key of len bases, 16 bits each (a row holds at most 2048 bases), in two
    // registers a hit indexes by shifting: one length for all, or each lane's own row's (ragged; worked out per tile).
    auto seg_bounds = [&](uint32_t len) {
        unsigned long long bnd[2] = {0ull, 0ull};
        for (uint32_t s2 = 1; s2 <= nseg; s2++)
            bnd[(s2 - 1) >> 2] |= (unsigned long long)(len * s2 / nseg) << (16u * ((s2 - 1) & 3u));
        return make_ulonglong2(bnd[0], bnd[1]);
    };
    auto seg_start = [](const ulonglong2 &bnd, uint32_t s2) {        // s2 in 0 .. nseg
        return s2 == 0 ? 0u : (uint32_t)((s2 <= 4 ? bnd.x : bnd.y) >> (16u * ((s2 - 1) & 3u))) & 0xFFFFu;
    };
    ulonglong2 bnd = seg_bounds(sh.max_len);
    uint32_t KW = K * W;
    const uint32_t n_list = (uint32_t)counts[0];
    const unsigned long long total = tile_prefix[n_list];
    auto flush = [&](uint32_t have) {
        unsigned long long g = 0;
        if (lane == 0)
            g = atomicAdd(edge_count, (unsigned long long)have);
        g = __shfl(g, 0);
        for (uint32_t e = lane; e < have; e += 64)
            if (g + e < edge_cap)
                reinterpret_cast<uint2 *>(edges)[g + e] = wbuf[wave][e];
    };
    const uint4 *recs4 = reinterpret_cast<const uint4 *>(urecs);
    const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
    // padding words (zero, or a ragged key's length) are cleared on their way into registers and LDS: the compare loops
    // below then run over whole chunks of a row without a test per word
    auto key_words = [&](uint4 v, uint32_t q) {
        v.x = q * 4u + 0u < KW ? v.x : 0u;
        v.y = q * 4u + 1u < KW ? v.y : 0u;
        v.z = q * 4u + 2u < KW ? v.z : 0u;
        v.w = q * 4u + 3u < KW ? v.w : 0u;
        return v;
    };
    for (unsigned long long g = blockIdx.x; g < total; g += gridDim.x) {
        // which bucket, which pair of tiles
        uint32_t a = 0, z = n_list;
        while (z - a > 1) {
            const uint32_t mid = (a + z) >> 1;
            if (tile_prefix[mid] <= g)
                a = mid;
            else
                z = mid;
        }
        const uint32_t b = list[a], lo = bucket_start[b];
        uint32_t hi = bucket_start[b + 1];
        if (bucket_end)
            hi = min(hi, bucket_end[b]);
        const uint32_t m = hi - lo, T = (m + WT_TS - 1) / WT_TS;
        const unsigned long long idx = g - tile_prefix[a];
        // row-major over the upper triangle: row ti holds T - ti pairs (ti, ti .. T - 1)
        uint32_t ti = (uint32_t)(((2.0 * T + 1.0) - sqrt((2.0 * T + 1.0) * (2.0 * T + 1.0) - 8.0 * (double)idx)) * 0.5);
        auto row_start = [&](uint32_t r) { return (unsigned long long)r * T - (unsigned long long)r * (r - 1) / 2; };
        ti = min(ti, T - 1);
        while (ti > 0 && row_start(ti) > idx)
            ti--;
        while (ti + 1 < T && row_start(ti + 1) <= idx)
            ti++;
        const uint32_t tj = ti + (uint32_t)(idx - row_start(ti));
        const uint32_t ni = min(WT_TS, m - ti * WT_TS), nj = min(WT_TS, m - tj * WT_TS);
        __syncthreads();                                  // (the tile of the pair before is done with)
        // my row of tile i: item and record (registers); row tid of tile j: item (LDS)
        const uint2 it_i = items[lo + ti * WT_TS + min(tid, ni - 1)];
        const uint32_t my_h = it_i.x, my_uid = fused_U ? it_i.y % fused_U : it_i.y;
        const uint32_t my_seg = seg0 + (fused_U ? it_i.y / fused_U : 0u);
        asm volatile("" : "+s"(q4), "+s"(KW));
        uint4 mine[QMAX];
#pragma unroll
        for (uint32_t q = 0; q < QMAX; q++) {
            mine[q] = zero4;
            if (q < q4) {
                mine[q] = recs4[(size_t)my_uid * q4 + q];
                if (q + 1 == q4)                           // (padding words sit in a row's last uint4 only)
                    mine[q] = key_words(mine[q], q);
            }
        }
        if (tid < nj) {
            const uint2 it = items[lo + tj * WT_TS + tid];
            h_j[tid] = it.x;
            uid_j[tid] = fused_U ? it.y % fused_U : it.y;
            seg_j[tid] = seg0 + (fused_U ? it.y / fused_U : 0u);
        }
        __syncthreads();
        // tile j's records as one coalesced stream of 128 * q4 uint4, four loads in flight per lane
        const uint32_t n4 = WT_TS * q4;
        for (uint32_t x0 = tid; x0 < n4; x0 += 4 * WT_TS) {
            uint4 vj[4];
#pragma unroll
            for (uint32_t t = 0; t < 4; t++) {             // (clamped, unconditional: in flight together)
                const uint32_t x = x0 + t * WT_TS, r = x / q4, q = x - r * q4;
                vj[t] = recs4[(size_t)uid_j[min(r, nj - 1)] * q4 + q];
            }
#pragma unroll
            for (uint32_t t = 0; t < 4; t++) {
                const uint32_t x = x0 + t * WT_TS, r = x / q4, q = x - r * q4;
                if (x < n4 && r < nj)
                    rec_j[r * row4 + q] = key_words(vj[t], q);
            }
        }
        __syncthreads();
        const uint32_t my_len = sh.ragged ? fqd_key_len(sh, ulens, my_uid) : sh.max_len;
        if (sh.ragged)
            bnd = seg_bounds(my_len);
        const uint32_t *mw = reinterpret_cast<const uint32_t *>(mine);
        for (uint32_t k = 0; k < nj; k++) {
            const uint32_t uk = uid_j[k];
            const bool cand = tid < ni && h_j[k] == my_h && seg_j[k] == my_seg && (ti != tj || k > tid) && uk != my_uid;
            if (!__ballot(cand))
                continue;                                  // (nobody in the wave: the row is not even read)
            asm volatile("" : "+s"(q4), "+s"(W));
            const uint4 *row = rec_j + k * row4;
            uint4 other[QMAX];
            const uint32_t *ow = reinterpret_cast<const uint32_t *>(other);
            auto diff = [&](uint32_t w) {                  // mismatching bases of 32-base word w
                uint32_t dw = 0;
#pragma unroll
                for (uint32_t kk = 0; kk < K; kk++)
                    dw |= mw[w * K + kk] ^ ow[w * K + kk];
                return dw;
            };
#pragma unroll
            for (uint32_t q = 0; q < QMAX; q++)
                other[q] = zero4;
#pragma unroll
            for (uint32_t q = 0; q < H; q++)
                if (q < q4)
                    other[q] = row[q];
            // (chunks of four words = K uint4: past the key both rows hold zeros, so a chunk is all or nothing)
            uint32_t dist = 0;
#pragma unroll
            for (uint32_t w0 = 0; w0 < WH; w0 += 4)
                if (w0 < W) {
#pragma unroll
                    for (uint32_t w = w0; w < w0 + 4 && w < WH; w++)
                        dist += __popc(diff(w));
                }
            if constexpr (HALVES) {
                if (!__ballot(cand && dist <= d))
                    continue;                              // (every lane's pair is beyond d already)
#pragma unroll
                for (uint32_t q = H; q < QMAX; q++)
                    if (q < q4)
                        other[q] = row[q];
#pragma unroll
                for (uint32_t w0 = WH; w0 < WMAX; w0 += 4)
                    if (w0 < W) {
#pragma unroll
                        for (uint32_t w = w0; w < w0 + 4 && w < WMAX; w++)
                            dist += __popc(diff(w));
                    }
            }
            bool hit = cand && dist && dist <= d && (!sh.ragged || fqd_key_len(sh, ulens, uk) == my_len);
            if (hit) {                                      // (rare: which main segments hold the differences)
                uint32_t seg_mis = 0;
#pragma unroll
                for (uint32_t w = 0; w < WMAX; w++) {
                    const uint32_t dw = diff(w);
                    if (dw)
#pragma unroll 1
                        for (uint32_t s2 = 0; s2 < nseg; s2++)
                            seg_mis |= (dw & fqd_range_mask(w, seg_start(bnd, s2), seg_start(bnd, s2 + 1))) ? 1u << s2 : 0u;
                }
                uint32_t first = 0;
                while (first < nseg && (seg_mis >> first & 1u))
                    first++;
                hit = first == my_seg;                   // reported in the pass of the FIRST segment the pair agrees on
            }
            const unsigned long long hm = __ballot(hit);
            if (hm) {
                const uint32_t n = (uint32_t)__popcll(hm);
                uint32_t have = s_wn[wave];
                if (have + n > WT_WCAP) {
                    flush(have);
                    have = 0;
                }
                if (hit)
                    wbuf[wave][have + (uint32_t)__popcll(hm & fqd_lanemask_lt())] = make_uint2(min(my_uid, uk), max(my_uid, uk));
                if (lane == 0)
                    s_wn[wave] = have + n;
                my_hits += hit ? 1u : 0u;
            }
        }
    }
    __syncthreads();
    const uint32_t left = s_wn[wave];
    if (left)
        flush(left);
    if (stats) {
        for (int o = 32; o; o >>= 1)
            my_hits += __shfl_xor(my_hits, o);
        if (lane == 0 && my_hits)
            atomicAdd(&stats[(blockIdx.x * (WT_TS / 64) + wave) % FQD_STAT_SLOTS].edges, (unsigned long long)my_hits);
    }
}

}  // namespace

namespace fqd {

// (what launch_group_wide_tiles takes; launch_group_crowded_tiles sends it the shapes its own kernel refuses)
bool group_wide_tiles_possible(KeyShape sh, uint32_t nseg)
{
    // (padding confined to a row's last uint4: what set_geometry lays out)
    return sh.stride >= 4 && sh.stride <= 64 && !(sh.stride & 3u) && sh.planes >= 1 && sh.planes <= 4 &&
           sh.planes * sh.words <= sh.stride && sh.planes * sh.words + 4 >= sh.stride && nseg >= 1 && nseg <= 8;
}

// tile_prefix is filled already (gp_tile_prefix_kernel, queued by launch_group_crowded_tiles on the same stream)
hipError_t launch_group_wide_tiles(const uint32_t *items, const uint32_t *bucket_start, const uint32_t *bucket_end,
                                   const uint32_t *list, const unsigned long long *counts,
                                   const unsigned long long *tile_prefix, uint32_t fused_U, uint32_t seg0,
                                   const uint32_t *urecs, const uint32_t *ulens, KeyShape sh, uint32_t d, uint32_t nseg,
                                   uint32_t *edges, unsigned long long *edge_count, uint64_t edge_cap, hipStream_t st,
                                   PairStats *stats)
{
    if (!group_wide_tiles_possible(sh, nseg))
        return hipErrorInvalidValue;
    const uint32_t q4 = sh.stride / 4;
#define FQD_WIDE(KK, QQ)                                                                                                \
    gp_wide_tiles_kernel<KK, QQ><<<8192, WT_TS, 0, st>>>(reinterpret_cast<const uint2 *>(items), bucket_start,         \
                                                         bucket_end, list, counts, tile_prefix, fused_U, seg0, urecs,  \
                                                         ulens, sh, d, nseg, edges, edge_count, edge_cap, stats)
#define FQD_WIDE_K(KK)                                                                                                  \
    case KK:                                                                                                            \
        if (q4 <= 4) FQD_WIDE(KK, 4); else if (q4 <= 6) FQD_WIDE(KK, 6); else if (q4 <= 8) FQD_WIDE(KK, 8);             \
        else if (q4 <= 12) FQD_WIDE(KK, 12); else FQD_WIDE(KK, 16);                                                     \
        break;
    switch (sh.planes) {
        FQD_WIDE_K(1)
        FQD_WIDE_K(2)
        FQD_WIDE_K(3)
        FQD_WIDE_K(4)
    }
#undef FQD_WIDE_K
#undef FQD_WIDE
    return hipGetLastError();
}

}  // namespace fqd
