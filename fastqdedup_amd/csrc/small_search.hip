// small_search.hip -- stage 3 for small unique tables: all d+1 pigeonhole passes of the Hamming
// neighbour search in ONE launch, without a sort, an iota or a library call (edges.hip explains the
// passes; this is the same search for tables of which a pass fits a few workgroups' LDS).
//
// Grid = n_pass x NB workgroups, NB a power of two. Workgroup (p, b) owns the keys whose hash of
// segment seg_lo + p has b in its top log2(NB) bits:
//   gather   it streams row p of the segment hashes (16-byte loads; NB x U x 4 bytes per pass, out of
//            L2) and ballot-compacts its (hash, uid) items into LDS. More than `cap` items: it raises
//            *need and leaves -- the host runs the search again on the sort path.
//   group    an open-addressed LDS table (>= 2 slots per item, linear probing, the slot claimed by a
//            CAS on the 32-bit hash) holds one chain head and one counter per hash value; item i
//            links itself with next[i] = atomicExch(&head[slot], i).
//   stage    items in a chain of >= 2 fetch their record once into a word-major LDS tile (word j of
//            item t at tile[j * cap + t]: neighbouring lanes, neighbouring banks) -- or, when the
//            records are too long for that, are compared from global memory (USE_LDS).
//   walk     item i walks next[i], next[next[i]], ...: every unordered pair of a chain is met once,
//            by its later-linked item. XOR/OR/popcount per 32-base word with early exit above d; a
//            pair is an edge of THIS pass only if this pass's segment is the first on which the two
//            keys truly agree, so every edge appears once over all passes.
//   crowded  chains of more than `chain_limit` items are not walked by one lane each (a lane on a
//            chain of thousands holds up its workgroup): their members are listed, every wave takes
//            one member and its 64 lanes stride over the members listed before it.
//   emit     (min uid, max uid) through an LDS buffer: wave ballot + popcount of the lanes below, one
//            LDS atomic per wave, one global atomic on the edge counter per flush. Writes are
//            bounded by edge_cap while the counter keeps counting (the host grows the buffer and
//            runs the search again).
#include "fqd_internal.h"

#include <algorithm>
#include <cstdlib>

namespace {

constexpr uint32_t SM_ECAP = 1024;            // edges buffered per workgroup
constexpr uint32_t SM_NONE = 0xFFFFFFFFu;     // free table slot / end of a chain
constexpr uint32_t SM_MAX_THREADS = 512;
constexpr uint32_t SM_DEFAULT_CAP = 1024;     // items per workgroup: 61 472 B of LDS at K = 3 / 32 nt, two workgroups per CU
constexpr uint32_t SM_LDS_BUDGET = 80 * 1024; // half a CU's LDS

struct SmallSearch {
    const uint32_t *seg_hashes;               // [n_pass][U], row p = segment seg_lo + p
    const uint32_t *urecs, *ulens;
    uint32_t U, d, seg_lo, nseg;
    uint32_t nb_bits;                         // NB = 1 << nb_bits bins per pass
    uint32_t cap;                             // items a workgroup holds (a multiple of 4)
    uint32_t slots;                           // table slots allocated: a power of two >= 2 * cap
    uint32_t chain_limit;
    uint32_t *edges;
    unsigned long long *edge_count;
    uint64_t edge_cap;
    unsigned long long *need;                 // raised to the item count of a workgroup that met more than cap
    fqd::PairStats *stats;
};

// the workgroup's LDS, in words
struct SmallLds {
    uint32_t *hs;        // [cap] an item's hash, later its table slot
    uint32_t *uid;       // [cap]
    uint32_t *next;      // [cap] the item linked before it in its chain (SM_NONE: none)
    uint32_t *len;       // [cap] key lengths of the items in chains of >= 2
    uint32_t *key;       // [slots] claimed hash values; once the chains stand: the list of crowded items
    uint32_t *head;      // [slots]
    uint32_t *cnt;       // [slots] items in the slot's chain
    uint32_t *ebuf;      // [2 * SM_ECAP]
    uint32_t *ctl;       // [0] buffered edges, [1..2] flush base, [3] items, [4] crowded items
    uint32_t *tile;      // [KW * cap] when USE_LDS
};

template <int K, bool USE_LDS>
__device__ __forceinline__ uint32_t sm_diff(const uint32_t *tile, uint32_t cap, uint32_t ia, uint32_t ib,
                                            const uint32_t *ra, const uint32_t *rb, uint32_t w)
{
    uint32_t dw = 0;
#pragma unroll
    for (int k = 0; k < K; k++) {
        const uint32_t j = w * K + k;
        const uint32_t a = USE_LDS ? tile[j * cap + ia] : ra[j];
        const uint32_t b = USE_LDS ? tile[j * cap + ib] : rb[j];
        dw |= a ^ b;
    }
    return dw;
}

// Are items ia and ib (keys of one length) within distance d, and is `seg` the first segment of the
// nseg-way split on which they truly agree? (bucket_pairs_kernel's rule; the agreement on `seg` itself
// is checked too, so two hash values sharing a chain cost compares and never an edge.)
template <int K, bool USE_LDS>
__device__ __forceinline__ bool sm_pair_hit(const uint32_t *tile, uint32_t cap, uint32_t ia, uint32_t ib,
                                            const uint32_t *ra, const uint32_t *rb, uint32_t len, uint32_t W,
                                            uint32_t d, uint32_t seg, uint32_t nseg)
{
    uint32_t dist = 0;
    for (uint32_t w = 0; w < W && dist <= d; w++)
        dist += __popc(sm_diff<K, USE_LDS>(tile, cap, ia, ib, ra, rb, w));
    if (dist > d)
        return false;
    for (uint32_t s2 = 0; s2 <= seg; s2++) {
        uint32_t lo, hi;
        fqd_segment(len, s2, nseg, lo, hi);
        bool agree = true;
        if (hi > lo)
            for (uint32_t w = lo >> 5; w <= ((hi - 1) >> 5) && agree; w++)
                if (sm_diff<K, USE_LDS>(tile, cap, ia, ib, ra, rb, w) & fqd_range_mask(w, lo, hi))
                    agree = false;
        if (agree)
            return s2 == seg;
    }
    return false;
}

// every lane of the wave calls this; the lanes with `hit` file (u, v)
__device__ __forceinline__ void sm_emit(bool hit, uint32_t u, uint32_t v, const SmallLds &L, const SmallSearch &A)
{
    const unsigned long long m = __ballot(hit);
    if (!m)
        return;
    const int leader = __ffsll((long long)m) - 1;
    uint32_t at = 0;
    if ((int)fqd_lane() == leader)
        at = atomicAdd(&L.ctl[0], (uint32_t)__popcll(m));
    at = __shfl(at, leader);
    if (hit) {
        at += __popcll(m & fqd_lanemask_lt());
        const uint32_t eu = u < v ? u : v, ev = u < v ? v : u;
        if (at < SM_ECAP) {
            L.ebuf[2 * at] = eu;
            L.ebuf[2 * at + 1] = ev;
        } else {
            // the buffer filled up between two flushes (a large chain of near keys): straight to global memory
            const unsigned long long g = atomicAdd(A.edge_count, 1ull);
            if (g < A.edge_cap) {
                A.edges[2 * g] = eu;
                A.edges[2 * g + 1] = ev;
            }
        }
    }
}

// the whole workgroup calls this: the buffered edges go out when the buffer is half full (or `force`)
__device__ __forceinline__ void sm_flush(bool force, const SmallLds &L, const SmallSearch &A)
{
    __syncthreads();
    const uint32_t buffered = L.ctl[0];
    __syncthreads();      // (every thread has read the count before a wave that goes on can file another edge: one decision per workgroup)
    if (buffered >= SM_ECAP / 2 || (force && buffered)) {
        const uint32_t n = buffered < SM_ECAP ? buffered : SM_ECAP;
        if (threadIdx.x == 0) {
            const unsigned long long g = atomicAdd(A.edge_count, (unsigned long long)n);
            L.ctl[1] = (uint32_t)g;
            L.ctl[2] = (uint32_t)(g >> 32);
        }
        __syncthreads();
        const unsigned long long g = ((unsigned long long)L.ctl[2] << 32) | L.ctl[1];
        for (uint32_t e = threadIdx.x; e < n; e += blockDim.x)
            if (g + e < A.edge_cap) {
                A.edges[2 * (g + e)] = L.ebuf[2 * e];
                A.edges[2 * (g + e) + 1] = L.ebuf[2 * e + 1];
            }
        __syncthreads();
        if (threadIdx.x == 0)
            L.ctl[0] = 0;
        __syncthreads();
    }
}

template <int K, bool USE_LDS>
__global__ __launch_bounds__(SM_MAX_THREADS) void small_search_kernel(SmallSearch A, KeyShape sh)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const uint32_t cap = A.cap;
    SmallLds L;
    L.hs = smem;
    L.uid = L.hs + cap;
    L.next = L.uid + cap;
    L.len = L.next + cap;
    L.key = L.len + cap;
    L.head = L.key + A.slots;
    L.cnt = L.head + A.slots;
    L.ebuf = L.cnt + A.slots;
    L.ctl = L.ebuf + 2 * SM_ECAP;
    L.tile = L.ctl + 8;

    const uint32_t T = blockDim.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, n_waves = T >> 6;
    const uint32_t p = blockIdx.x >> A.nb_bits, bin = blockIdx.x & ((1u << A.nb_bits) - 1u);
    const uint32_t seg = A.seg_lo + p;
    const uint32_t W = sh.words, KW = W * K, stride = sh.stride;
    unsigned long long n_pairs = 0, n_hits = 0, n_gathered = 0;

    if (tid < 8)
        L.ctl[tid] = 0;
    __syncthreads();

    // ---- gather: this pass's hashes, four per lane and step; those of this bin go to LDS
    {
        const uint64_t g0 = (uint64_t)p * A.U, g1 = g0 + A.U;
        // (the rows start anywhere: whole uint4 around them -- up to 12 bytes behind the last row are read and
        // dropped, see launch_small_search in fqd_internal.h)
        const uint64_t v0 = g0 >> 2, v1 = (g1 + 3) >> 2;
        const uint4 *src = reinterpret_cast<const uint4 *>(A.seg_hashes);
        for (uint64_t vb = v0; vb < v1; vb += T) {
            const uint64_t v = vb + tid;
            uint4 q = make_uint4(0, 0, 0, 0);
            if (v < v1)
                q = src[v];
            const uint32_t h[4] = {q.x, q.y, q.z, q.w};
            bool keep[4];
            unsigned long long m[4];
            uint32_t total = 0;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const uint64_t g = v * 4 + e;
                keep[e] = v < v1 && g >= g0 && g < g1 && (A.nb_bits == 0 || (h[e] >> (32u - A.nb_bits)) == bin);
                m[e] = __ballot(keep[e]);
                total += (uint32_t)__popcll(m[e]);
            }
            if (total) {
                uint32_t at = 0;
                if (lane == 0)
                    at = atomicAdd(&L.ctl[3], total);
                at = __shfl(at, 0);
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const uint32_t mine = at + (uint32_t)__popcll(m[e] & fqd_lanemask_lt());
                    if (keep[e] && mine < cap) {
                        L.hs[mine] = h[e];
                        L.uid[mine] = (uint32_t)(v * 4 + e - g0);
                    }
                    at += (uint32_t)__popcll(m[e]);
                }
            }
        }
    }
    __syncthreads();
    const uint32_t count = L.ctl[3];
    if (count > cap) {
        if (tid == 0)
            atomicMax(A.need, (unsigned long long)count);
        return;
    }
    if (count < 2)
        return;

    // ---- group: one chain per hash value
    const uint32_t n_slots = count <= 32 ? 64u : 1u << (32 - __clz((int)(2 * count - 1)));     // <= A.slots
    const uint32_t mask = n_slots - 1u;
    for (uint32_t s = tid; s < n_slots; s += T) {
        L.key[s] = SM_NONE;
        L.head[s] = SM_NONE;
        L.cnt[s] = 0;
    }
    __syncthreads();
    for (uint32_t i = tid; i < count; i += T) {
        uint32_t h = L.hs[i];
        if (h == SM_NONE)
            h = SM_NONE - 1u;              // (the free mark is no hash value; sharing a chain costs compares only)
        uint32_t slot = h & mask;
        for (;;) {
            const uint32_t was = atomicCAS(&L.key[slot], SM_NONE, h);
            if (was == SM_NONE || was == h)
                break;
            slot = (slot + 1u) & mask;
        }
        L.next[i] = atomicExch(&L.head[slot], i);
        atomicAdd(&L.cnt[slot], 1u);
        L.hs[i] = slot;
    }
    __syncthreads();

    // ---- stage: lengths and records of the items in chains of >= 2; the crowded chains' items are listed
    uint32_t *crowded = L.key;            // (the claimed hash values have done their work)
    for (uint32_t base = 0; base < count; base += T) {
        const uint32_t i = base + tid;
        const bool valid = i < count;
        const uint32_t in_chain = valid ? L.cnt[L.hs[i]] : 0u;
        if (in_chain >= 2) {
            n_gathered++;
            const uint32_t uid = L.uid[i];
            L.len[i] = fqd_key_len(sh, A.ulens, uid);
            if (USE_LDS) {
                const uint4 *src = reinterpret_cast<const uint4 *>(A.urecs + (uint64_t)uid * stride);
                for (uint32_t q = 0; q < stride / 4; q++) {
                    const uint4 v = src[q];
                    const uint32_t j = q * 4;
                    if (j + 0 < KW) L.tile[(j + 0) * cap + i] = v.x;
                    if (j + 1 < KW) L.tile[(j + 1) * cap + i] = v.y;
                    if (j + 2 < KW) L.tile[(j + 2) * cap + i] = v.z;
                    if (j + 3 < KW) L.tile[(j + 3) * cap + i] = v.w;
                }
            }
        }
        const bool is_crowded = in_chain > A.chain_limit;
        const unsigned long long m = __ballot(is_crowded);
        if (m) {
            uint32_t at = 0;
            if (lane == 0)
                at = atomicAdd(&L.ctl[4], (uint32_t)__popcll(m));
            at = __shfl(at, 0);
            if (is_crowded)
                crowded[at + (uint32_t)__popcll(m & fqd_lanemask_lt())] = i;
        }
    }
    __syncthreads();

    // ---- walk: item i against the items linked before it
    for (uint32_t base = 0; base < count; base += T) {
        const uint32_t i = base + tid;
        uint32_t j = SM_NONE, uid = 0, len = 0;
        const uint32_t *my_rec = A.urecs;
        if (i < count) {
            const uint32_t in_chain = L.cnt[L.hs[i]];
            if (in_chain >= 2 && in_chain <= A.chain_limit) {
                j = L.next[i];
                uid = L.uid[i];
                len = L.len[i];
                my_rec = A.urecs + (uint64_t)uid * stride;
            }
        }
        while (__any(j != SM_NONE)) {
            bool hit = false;
            uint32_t uj = 0;
            if (j != SM_NONE) {
                uj = L.uid[j];
                n_pairs++;
                if (L.len[j] == len)
                    hit = sm_pair_hit<K, USE_LDS>(L.tile, cap, i, j, my_rec, A.urecs + (uint64_t)uj * stride, len, W,
                                                  A.d, seg, A.nseg);
                n_hits += hit ? 1 : 0;
                j = L.next[j];
            }
            sm_emit(hit, uid, uj, L, A);
        }
        sm_flush(false, L, A);
    }

    // ---- crowded chains: a wave per listed item, its lanes over the items listed before it
    const uint32_t n_crowded = L.ctl[4];
    for (uint32_t a0 = 0; a0 < n_crowded; a0 += n_waves) {
        const uint32_t a = a0 + wave;
        if (a < n_crowded) {
            const uint32_t i = crowded[a], slot = L.hs[i], uid = L.uid[i], len = L.len[i];
            const uint32_t *my_rec = A.urecs + (uint64_t)uid * stride;
            for (uint32_t b0 = 0; b0 < a; b0 += 64) {
                const uint32_t b = b0 + lane;
                bool hit = false;
                uint32_t uj = 0;
                if (b < a) {
                    const uint32_t j = crowded[b];
                    if (L.hs[j] == slot) {
                        uj = L.uid[j];
                        n_pairs++;
                        if (L.len[j] == len)
                            hit = sm_pair_hit<K, USE_LDS>(L.tile, cap, i, j, my_rec, A.urecs + (uint64_t)uj * stride,
                                                          len, W, A.d, seg, A.nseg);
                        n_hits += hit ? 1 : 0;
                    }
                }
                sm_emit(hit, uid, uj, L, A);
            }
        }
        sm_flush(false, L, A);
    }
    sm_flush(true, L, A);

    if (A.stats) {
        // workgroup totals land in one of FQD_STAT_SLOTS slots: no hot counter
        for (int o = 32; o; o >>= 1) {
            n_gathered += __shfl_xor(n_gathered, o);
            n_pairs += __shfl_xor(n_pairs, o);
            n_hits += __shfl_xor(n_hits, o);
        }
        unsigned long long *red = reinterpret_cast<unsigned long long *>(L.ebuf);
        if (lane == 0) {
            red[wave * 3 + 0] = n_gathered;
            red[wave * 3 + 1] = n_pairs;
            red[wave * 3 + 2] = n_hits;
        }
        __syncthreads();
        if (tid < 3) {
            unsigned long long tot = 0;
            for (uint32_t wv = 0; wv < n_waves; wv++)
                tot += red[wv * 3 + tid];
            fqd::PairStats *slot = A.stats + (blockIdx.x % FQD_STAT_SLOTS);
            unsigned long long *dst = tid == 0 ? &slot->keys_gathered : (tid == 1 ? &slot->pairs_compared : &slot->edges);
            if (tot)
                atomicAdd(dst, tot);
        }
    }
}

template <int K, bool USE_LDS>
hipError_t small_search_go(const SmallSearch &A, KeyShape sh, unsigned grid, unsigned threads, size_t lds, hipStream_t st)
{
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&small_search_kernel<K, USE_LDS>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess)
            return e;
    }
    small_search_kernel<K, USE_LDS><<<grid, threads, lds, st>>>(A, sh);
    return hipGetLastError();
}

}  // namespace

namespace fqd {

uint32_t small_search_cap()
{
    uint32_t cap = SM_DEFAULT_CAP;
    if (const char *e = getenv("FQD_SMALL_CAP"))          // tests: several bins, overflow on small tables
        cap = (uint32_t)strtoul(e, nullptr, 10);
    cap = cap < 8 ? 8 : (cap > 2048 ? 2048 : cap);
    return cap & ~3u;
}

hipError_t launch_small_search(const uint32_t *seg_hashes, uint32_t n_pass, uint64_t U, const uint32_t *urecs,
                               const uint32_t *ulens, KeyShape sh, uint32_t d, uint32_t seg_lo, uint32_t nseg,
                               uint32_t *edges, unsigned long long *edge_count, uint64_t edge_cap,
                               unsigned long long *need, PairStats *stats, hipStream_t st)
{
    if (U < 2 || !n_pass)
        return hipSuccess;
    if (U >= 0xFFFFFF00ull || sh.planes < 1 || sh.planes > 7)
        return hipErrorInvalidValue;
    SmallSearch A;
    A.seg_hashes = seg_hashes;
    A.urecs = urecs;
    A.ulens = ulens;
    A.U = (uint32_t)U;
    A.d = d;
    A.seg_lo = seg_lo;
    A.nseg = nseg;
    A.cap = small_search_cap();
    // the expected items of a workgroup are at most cap / 2 (a table of millions, pinned here: the bins overflow and the
    // caller's sort path takes over)
    A.nb_bits = 0;
    while (A.nb_bits < 16 && (U >> A.nb_bits) > A.cap / 2)
        A.nb_bits++;
    A.slots = 64;
    while (A.slots < 2 * A.cap)
        A.slots <<= 1;
    A.chain_limit = 64;
    if (const char *e = getenv("FQD_SMALL_CHAIN_LIMIT"))
        A.chain_limit = (uint32_t)std::max(2, atoi(e));
    A.edges = edges;
    A.edge_count = edge_count;
    A.edge_cap = edge_cap;
    A.need = need;
    A.stats = stats;
    const uint32_t KW = sh.planes * sh.words;
    const size_t base_words = (size_t)4 * A.cap + (size_t)3 * A.slots + 2 * SM_ECAP + 8;
    const bool use_lds = (base_words + (size_t)KW * A.cap) * 4 <= SM_LDS_BUDGET;
    const size_t lds = (base_words + (use_lds ? (size_t)KW * A.cap : 0)) * 4;
    const uint64_t expected = U >> A.nb_bits;
    unsigned threads = 64;
    while (threads < SM_MAX_THREADS && threads < expected)
        threads <<= 1;
    const unsigned grid = n_pass << A.nb_bits;
#define FQD_SMALL_CASE(KK)                                                                     \
    case KK:                                                                                   \
        return use_lds ? small_search_go<KK, true>(A, sh, grid, threads, lds, st)              \
                       : small_search_go<KK, false>(A, sh, grid, threads, lds, st);
    switch (sh.planes) {
        FQD_SMALL_CASE(1)
        FQD_SMALL_CASE(2)
        FQD_SMALL_CASE(3)
        FQD_SMALL_CASE(4)
        FQD_SMALL_CASE(5)
        FQD_SMALL_CASE(6)
        FQD_SMALL_CASE(7)
    }
#undef FQD_SMALL_CASE
    return hipErrorInvalidValue;
}

}  // namespace fqd
