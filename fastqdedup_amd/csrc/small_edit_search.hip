// small_edit_search.hip -- the Levenshtein neighbour search (d = 1..3) of small unique tables in two launches, without
// a sort, a scan, a length histogram or a host round trip between them (edit.hip explains the pigeonhole scheme and
// the first-matching-configuration rule; small_search.hip is the Hamming search of the same tables).
//
// items    one lane per key. The key files an INDEX item per own segment (fqd_segment_hash: the hash the rest of
//          stage 3 uses) and PROBE items (shifted_segment_hash: the value an index item has whose segment holds these
//          bases) for every PRESENT length class in (len, len + d], and -- d >= 2 -- for its own class at shifts != 0.
//          "The shorter key probes": if lev(a, b) <= d, some segment of b occurs in a within d positions, whichever
//          of the two is called b -- so it is enough that the shorter key of a pair probes, and which classes are
//          present each workgroup finds out itself (an LDS bitmap of the table's lengths; a fixed-length table has
//          one class and skips that). An item goes straight to the slab of its hash bin (top nb_bits of the hash), its
//          place taken with an atomic on the bin's fill counter; an item beyond the slab raises *need.
// search   one workgroup per bin. The slab comes in with 8-byte loads; an open-addressed LDS table chains the items
//          of one hash value (small_search.hip's scheme); items in chains of >= 2 fetch their key's length and row
//          (row per item at an odd word stride: Landau-Vishkin reads a row at any word offset, and lanes on
//          different rows hit different banks; rows too long for the LDS budget are read from global memory). Item i
//          walks the items linked before it: a pair of items is dropped when both probe, both belong to one key, two
//          index items differ in length, the index item is of another segment number or the lengths are more than d
//          apart; otherwise the configurations FILED for the two keys are tried in the fixed order (direction in uid
//          order, segment, shift) and the pair of items that IS the first matching one runs eg_within_edit: every
//          edge comes out once. Chains above chain_limit go a wave per member; edges leave through an LDS buffer.
#include "fqd_internal.h"
#include "edit_shared.h"

#include <algorithm>
#include <cstdlib>

namespace {

using fqd::SmallEdit;

constexpr uint32_t SE_ECAP = 1024;            // edges buffered per workgroup
constexpr uint32_t SE_NONE = 0xFFFFFFFFu;     // free table slot / end of a chain
constexpr uint32_t SE_ITEM_THREADS = 256;
constexpr uint32_t SE_MAX_THREADS = 256;      // (the pair test holds two rows' windows and seven diagonals: 256 registers a lane)
constexpr uint32_t SE_LDS_BUDGET = 80 * 1024; // half a CU's LDS
constexpr uint32_t SE_MAX_BIN_BITS = 15;

// every lane of the wave calls this; the lanes with `valid` file (h, payload) in the slab of h's bin
__device__ __forceinline__ void se_file(bool valid, uint32_t h, uint32_t payload, const SmallEdit &A)
{
    const uint32_t bin = A.nb_bits ? h >> (32u - A.nb_bits) : 0u;
    uint32_t pos = 0;
    if (A.nb_bits <= 3) {
        // few bins, many lanes per bin: one atomic per bin and wave
        unsigned long long todo = __ballot(valid);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const uint32_t its = __shfl(bin, leader);
            const bool with = valid && bin == its;
            const unsigned long long same = __ballot(with);
            uint32_t base = 0;
            if ((int)fqd_lane() == leader)
                base = atomicAdd(&A.fill[its], (uint32_t)__popcll(same));
            base = __shfl(base, leader);
            if (with)
                pos = base + (uint32_t)__popcll(same & fqd_lanemask_lt());
            todo &= ~same;
        }
    } else if (valid) {
        pos = atomicAdd(&A.fill[bin], 1u);
    }
    if (valid) {
        if (pos < A.cap)
            A.slabs[(uint64_t)bin * A.cap + pos] = make_uint2(h, payload);
        else if (pos == A.cap)                                // (one lane per overfull bin says so)
            atomicMax(A.need, (unsigned long long)pos + 1ull);
    }
}

__global__ __launch_bounds__(SE_ITEM_THREADS) void small_edit_items_kernel(SmallEdit A, KeyShape sh)
{
    extern __shared__ uint32_t s_present[];       // ragged: bit l = some key is l bases long
    const uint32_t tid = threadIdx.x, T = blockDim.x;
    const uint32_t d = A.d, nseg = d + 1, K = sh.planes, W = sh.words, KW = K * W;
    if (sh.ragged) {
        for (uint32_t w = tid; w <= (sh.max_len >> 5); w += T)
            s_present[w] = 0;
        __syncthreads();
        // four loads in flight per lane; a bit that stands is not set again (almost all keys share a few lengths)
        for (uint32_t u0 = tid; u0 < A.U; u0 += 4 * T) {
            uint32_t l[4];
#pragma unroll
            for (uint32_t t = 0; t < 4; t++)
                l[t] = u0 + t * T < A.U ? A.ulens[u0 + t * T] : 0xFFFFFFFFu;
#pragma unroll
            for (uint32_t t = 0; t < 4; t++)
                if (l[t] <= sh.max_len && !((s_present[l[t] >> 5] >> (l[t] & 31u)) & 1u))
                    atomicOr(&s_present[l[t] >> 5], 1u << (l[t] & 31u));
        }
        __syncthreads();
    }
    const uint32_t u = blockIdx.x * T + tid;
    const bool live = u < A.U;
    const uint32_t la = live ? fqd_key_len(sh, A.ulens, u) : 0u;
    const uint32_t *rec = A.urecs + (uint64_t)(live ? u : 0u) * sh.stride;
    for (uint32_t s = 0; s < nseg; s++) {
        const uint32_t h = live ? fqd_segment_hash(rec, K, KW, la, s, nseg) : 0u;
        se_file(live, h, eg_payload(u, s, 0, false), A);
    }
    // class la + j: j = 0 is the own class (shifts != 0, which d = 1 never needs), j >= 1 the longer classes
    for (uint32_t j = d >= 2 ? 0u : 1u; j <= d; j++) {
        const uint32_t lb = la + j;
        bool probes = live;
        if (j)
            probes = live && sh.ragged && lb <= sh.max_len && ((s_present[lb >> 5] >> (lb & 31u)) & 1u);
        if (!__any(probes))
            continue;
        for (uint32_t s = 0; s < nseg; s++) {
            uint32_t lo, hi;
            fqd_segment(lb, s, nseg, lo, hi);
            for (int delta = -(int)d; delta <= (int)d; delta++) {
                if (j == 0 && delta == 0)
                    continue;                      // that is the index item
                const int start = (int)lo + delta;
                const bool valid = probes && start >= 0 && (uint32_t)start + (hi - lo) <= la;
                const uint32_t h = valid ? shifted_segment_hash(rec, K, W, lb, s, nseg, delta) : 0u;
                se_file(valid, h, eg_payload(u, s, delta, true), A);
            }
        }
    }
}

// the search workgroup's LDS, in words
struct SeLds {
    uint32_t *hs;        // [cap] an item's hash, later its table slot
    uint32_t *pl;        // [cap] its payload
    uint32_t *next;      // [cap] the item linked before it in its chain (SE_NONE: none)
    uint32_t *len;       // [cap] key lengths of the items in chains of >= 2
    uint32_t *key;       // [slots] claimed hash values; once the chains stand: the list of crowded items
    uint32_t *head;      // [slots]
    uint32_t *cnt;       // [slots] items in the slot's chain
    uint32_t *ebuf;      // [2 * SE_ECAP]
    uint32_t *ctl;       // [0] buffered edges, [1..2] flush base, [4] crowded items
    uint32_t *tile;      // [cap * row] when USE_LDS: item t's record at tile + t * row
};

// Items i and j share a hash value. Is their pair of keys an edge, and is THIS pair of items the one that reports it?
template <int K, bool USE_LDS>
__device__ __forceinline__ bool se_pair_hit(const SeLds &L, const SmallEdit &A, const KeyShape &sh, uint32_t row,
                                            uint32_t i, uint32_t j, uint32_t &eu, uint32_t &ev,
                                            unsigned long long &n_pairs)
{
    uint32_t pa = L.pl[i], pb = L.pl[j], ia = i, ib = j;
    uint32_t ua = pa & EG_UID_MASK, ub = pb & EG_UID_MASK;
    if (ua == ub || (pa & pb & ROLE_PROBE))
        return false;
    // (prober, indexed): the probe item's owner probes; two index items: the smaller uid "probes"
    if ((pb & ROLE_PROBE) || (!(pa & ROLE_PROBE) && ub < ua)) {
        const uint32_t tp = pa, tu = ua;
        pa = pb, pb = tp;
        ua = ub, ub = tu;
        ia = j, ib = i;
    }
    const uint32_t d = A.d, W = sh.words;
    const uint32_t la = L.len[ia], lb = L.len[ib];
    const uint32_t gap = la > lb ? la - lb : lb - la;
    const uint32_t seg = (pa >> EG_UID_BITS) & 3u;
    const int delta = (int)((pa >> (EG_UID_BITS + 2)) & 7u) - 3;
    const bool both_index = !((pa | pb) & ROLE_PROBE);
    // an index item of the other segment number cannot be this item's partner (two hash values that collide)
    if (gap > d || ((pb >> EG_UID_BITS) & 3u) != seg || (both_index && la != lb))
        return false;
    n_pairs++;
    const uint32_t *ra = USE_LDS ? L.tile + ia * row : A.urecs + (uint64_t)ua * sh.stride;
    const uint32_t *rb = USE_LDS ? L.tile + ib * row : A.urecs + (uint64_t)ub * sh.stride;
    // the first configuration under which the two keys match, among those the items kernel files: directions with the
    // smaller uid probing first (keys of different lengths: the shorter one probes, one direction), then segments,
    // then shifts (one class: shift 0 is the index-index match, counted once; the others exist from d = 2 on)
    const bool a_is_smaller = ua < ub;
    bool mine_is_first = false, found = false;
    for (int dir = 0; dir < 2 && !found; dir++) {
        const bool a_probes = (dir == 0) == a_is_smaller;
        const uint32_t *rp = a_probes ? ra : rb, *ri = a_probes ? rb : ra;
        const uint32_t lp = a_probes ? la : lb, li = a_probes ? lb : la;
        if (lp > li)
            continue;
        for (uint32_t s = 0; s <= d && !found; s++)
            for (int dl = -(int)d; dl <= (int)d && !found; dl++) {
                if (lp == li && (dl == 0 ? dir == 1 : d < 2))
                    continue;
                if (eg_config_matches(rp, lp, ri, li, s, dl, d, K, W)) {
                    found = true;
                    mine_is_first = a_probes && s == seg && dl == delta;
                }
            }
    }
    if (!mine_is_first)
        return false;
    eu = a_is_smaller ? ua : ub;
    ev = a_is_smaller ? ub : ua;
    // (inlined at both call sites: as a call it keeps a frame in scratch memory)
    [[clang::always_inline]] return eg_within_edit(ra, la, rb, lb, (int)d, K, W);
}

// every lane of the wave calls this; the lanes with `hit` file (eu, ev)
__device__ __forceinline__ void se_emit(bool hit, uint32_t eu, uint32_t ev, const SeLds &L, const SmallEdit &A)
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
        if (at < SE_ECAP) {
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
__device__ __forceinline__ void se_flush(bool force, const SeLds &L, const SmallEdit &A)
{
    __syncthreads();
    const uint32_t buffered = L.ctl[0];
    __syncthreads();      // (every thread has read the count before a wave that goes on can file another edge)
    if (buffered >= SE_ECAP / 2 || (force && buffered)) {
        const uint32_t n = buffered < SE_ECAP ? buffered : SE_ECAP;
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
__global__ __launch_bounds__(SE_MAX_THREADS) void small_edit_search_kernel(SmallEdit A, KeyShape sh)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const uint32_t cap = A.cap;
    SeLds L;
    L.hs = smem;
    L.pl = L.hs + cap;
    L.next = L.pl + cap;
    L.len = L.next + cap;
    L.key = L.len + cap;
    L.head = L.key + A.slots;
    L.cnt = L.head + A.slots;
    L.ebuf = L.cnt + A.slots;
    L.ctl = L.ebuf + 2 * SE_ECAP;
    L.tile = L.ctl + 8;

    const uint32_t T = blockDim.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, n_waves = T >> 6;
    const uint32_t KW = sh.words * K, stride = sh.stride, row = KW | 1u;
    const uint32_t count = A.fill[blockIdx.x];
    // (more than cap: the items kernel has raised *need and dropped the rest -- the host searches again another way)
    if (count < 2 || count > cap)
        return;
    unsigned long long n_pairs = 0, n_hits = 0, n_gathered = 0;

    // ---- load: this bin's slab
    const uint2 *slab = A.slabs + (uint64_t)blockIdx.x * cap;
    for (uint32_t i = tid; i < count; i += T) {
        const uint2 it = slab[i];
        L.hs[i] = it.x;
        L.pl[i] = it.y;
    }
    if (tid < 8)
        L.ctl[tid] = 0;

    // ---- group: one chain per hash value
    const uint32_t n_slots = count <= 32 ? 64u : 1u << (32 - __clz((int)(2 * count - 1)));     // <= A.slots
    const uint32_t mask = n_slots - 1u;
    for (uint32_t s = tid; s < n_slots; s += T) {
        L.key[s] = SE_NONE;
        L.head[s] = SE_NONE;
        L.cnt[s] = 0;
    }
    __syncthreads();
    for (uint32_t i = tid; i < count; i += T) {
        uint32_t h = L.hs[i];
        if (h == SE_NONE)
            h = SE_NONE - 1u;              // (the free mark is no hash value; sharing a chain costs compares only)
        uint32_t slot = h & mask;
        for (;;) {
            const uint32_t was = atomicCAS(&L.key[slot], SE_NONE, h);
            if (was == SE_NONE || was == h)
                break;
            slot = (slot + 1u) & mask;
        }
        L.next[i] = atomicExch(&L.head[slot], i);
        atomicAdd(&L.cnt[slot], 1u);
        L.hs[i] = slot;
    }
    __syncthreads();

    // ---- stage: lengths and rows of the items in chains of >= 2; the crowded chains' items are listed
    uint32_t *crowded = L.key;            // (the claimed hash values have done their work)
    for (uint32_t base = 0; base < count; base += T) {
        const uint32_t i = base + tid;
        const uint32_t in_chain = i < count ? L.cnt[L.hs[i]] : 0u;
        if (in_chain >= 2) {
            n_gathered++;
            const uint32_t uid = L.pl[i] & EG_UID_MASK;
            L.len[i] = fqd_key_len(sh, A.ulens, uid);
            if (USE_LDS) {
                const uint4 *src = reinterpret_cast<const uint4 *>(A.urecs + (uint64_t)uid * stride);
                uint32_t *dst = L.tile + i * row;
                for (uint32_t q = 0; q < stride / 4; q++) {
                    const uint4 v = src[q];
                    const uint32_t w = q * 4;
                    if (w + 0 < KW) dst[w + 0] = v.x;
                    if (w + 1 < KW) dst[w + 1] = v.y;
                    if (w + 2 < KW) dst[w + 2] = v.z;
                    if (w + 3 < KW) dst[w + 3] = v.w;
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
        uint32_t j = SE_NONE;
        if (i < count) {
            const uint32_t in_chain = L.cnt[L.hs[i]];
            if (in_chain >= 2 && in_chain <= A.chain_limit)
                j = L.next[i];
        }
        while (__any(j != SE_NONE)) {
            bool hit = false;
            uint32_t eu = 0, ev = 0;
            if (j != SE_NONE) {
                hit = se_pair_hit<K, USE_LDS>(L, A, sh, row, i, j, eu, ev, n_pairs);
                n_hits += hit ? 1 : 0;
                j = L.next[j];
            }
            se_emit(hit, eu, ev, L, A);
        }
        se_flush(false, L, A);
    }

    // ---- crowded chains: a wave per listed item, its lanes over the items listed before it
    const uint32_t n_crowded = L.ctl[4];
    for (uint32_t a0 = 0; a0 < n_crowded; a0 += n_waves) {
        const uint32_t a = a0 + wave;
        if (a < n_crowded) {
            const uint32_t i = crowded[a], slot = L.hs[i];
            for (uint32_t b0 = 0; b0 < a; b0 += 64) {
                const uint32_t b = b0 + lane;
                bool hit = false;
                uint32_t eu = 0, ev = 0;
                if (b < a) {
                    const uint32_t j = crowded[b];
                    if (L.hs[j] == slot) {
                        hit = se_pair_hit<K, USE_LDS>(L, A, sh, row, i, j, eu, ev, n_pairs);
                        n_hits += hit ? 1 : 0;
                    }
                }
                se_emit(hit, eu, ev, L, A);
            }
        }
        se_flush(false, L, A);
    }
    se_flush(true, L, A);

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
hipError_t small_edit_go(const SmallEdit &A, KeyShape sh, unsigned threads, size_t lds, hipStream_t st)
{
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&small_edit_search_kernel<K, USE_LDS>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess)
            return e;
    }
    small_edit_search_kernel<K, USE_LDS><<<1u << A.nb_bits, threads, lds, st>>>(A, sh);
    return hipGetLastError();
}

}  // namespace

namespace fqd {

SmallEdit small_edit_plan(uint64_t U, KeyShape sh, uint32_t d)
{
    SmallEdit A = {};
    A.U = (uint32_t)U;
    A.d = d;
    A.cap = small_search_cap();
    A.slots = 64;
    while (A.slots < 2 * A.cap)
        A.slots <<= 1;
    A.chain_limit = 64;
    if (const char *e = getenv("FQD_SMALL_CHAIN_LIMIT"))
        A.chain_limit = (uint32_t)std::max(2, atoi(e));
    // what a key files at most, known without a look at the table: d + 1 index items; probe items for up to d longer
    // classes (ragged tables) and the own class (d >= 2), d + 1 segments at 2d + 1 (2d) shifts each. The expected items
    // of a workgroup are at most cap / 2; a bin this bound provides for in vain is a workgroup that reads one counter.
    const uint32_t nseg = d + 1;
    A.items_per_key = nseg + (sh.ragged ? d * nseg * (2 * d + 1) : 0u) + (d >= 2 ? nseg * 2 * d : 0u);
    const uint64_t R = U * A.items_per_key;
    while (A.nb_bits < SE_MAX_BIN_BITS && (R >> A.nb_bits) > A.cap / 2)
        A.nb_bits++;
    return A;
}

hipError_t launch_small_edit_items(const SmallEdit &A, KeyShape sh, hipStream_t st)
{
    if (A.U < 2 || A.d < 1 || A.d > 3 || A.U >= (1u << EG_UID_BITS) || sh.max_len > SMALL_EDIT_MAX_LEN)
        return hipErrorInvalidValue;
    const size_t lds = sh.ragged ? ((size_t)(sh.max_len >> 5) + 1) * 4 : 0;
    small_edit_items_kernel<<<(A.U + SE_ITEM_THREADS - 1) / SE_ITEM_THREADS, SE_ITEM_THREADS, lds, st>>>(A, sh);
    return hipGetLastError();
}

hipError_t launch_small_edit_search(const SmallEdit &A, KeyShape sh, hipStream_t st)
{
    if (sh.planes < 1 || sh.planes > 7)
        return hipErrorInvalidValue;
    const uint32_t row = (sh.planes * sh.words) | 1u;
    const size_t base_words = (size_t)4 * A.cap + (size_t)3 * A.slots + 2 * SE_ECAP + 8;
    const bool use_lds = (base_words + (size_t)row * A.cap) * 4 <= SE_LDS_BUDGET;
    const size_t lds = (base_words + (use_lds ? (size_t)row * A.cap : 0)) * 4;
    const uint64_t expected = ((uint64_t)A.U * A.items_per_key) >> A.nb_bits;
    unsigned threads = 64;
    while (threads < SE_MAX_THREADS && threads < expected)
        threads <<= 1;
#define FQD_SMALL_EDIT_CASE(KK)                                                           \
    case KK:                                                                              \
        return use_lds ? small_edit_go<KK, true>(A, sh, threads, lds, st)                 \
                       : small_edit_go<KK, false>(A, sh, threads, lds, st);
    switch (sh.planes) {
        FQD_SMALL_EDIT_CASE(1)
        FQD_SMALL_EDIT_CASE(2)
        FQD_SMALL_EDIT_CASE(3)
        FQD_SMALL_EDIT_CASE(4)
        FQD_SMALL_EDIT_CASE(5)
        FQD_SMALL_EDIT_CASE(6)
        FQD_SMALL_EDIT_CASE(7)
    }
#undef FQD_SMALL_EDIT_CASE
    return hipErrorInvalidValue;
}

}  // namespace fqd
