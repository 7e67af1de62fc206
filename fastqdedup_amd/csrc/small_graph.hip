// small_graph.hip -- stages 4 and 5 of a SMALL unique table (up to 8 192 keys) in ONE launch of ONE workgroup.
//
// graph.hip runs a table of a few thousand keys as if it had 14 M: a dozen launches of a handful of workgroups each,
// device-wide atomics, and -- for the adjacency and the relaxation routes -- the host in the convergence loop. Here
// the whole stage lives in one workgroup's LDS:
//   R1  4 U bytes   the parents of the union-find; then the keys' counts (staged from ucounts[]) for the dissection;
//                   then the bit map of the id window (<= 2^18 ids = 32 KB) for the ascending kept-id list
//   R2  4 U bytes   best[] (highest_count, directional); the round stamps of the adjacency rounds
//   R3  U bytes     the state bytes (directional closed form: 2 dropped, 4 on a root: component tainted; adjacency:
//                   0 undecided, 1 kept, 2 dropped)
// 72 KB at U = 8 192, plus the control words. Edges are streamed from global memory as uint2, four loads in flight per
// lane, and again per sweep (they stay in L2); records are read from global memory only where two counts tie.
// One workgroup never waits for another: the unions are lock-free (every failed compare-and-swap is somebody else's
// successful hook, and there are at most U - 1 of those), sweeps run at most U + 2 times.
// LDS23 = false (FQD_GRAPH=small, 8 192 < U <= 16 384): R2 and R3 have no room and live in global memory.
// The restatement of the three dissections in graph.hip's header comment holds here word for word.
#include <algorithm>

#include "../../include/fqdedup_hip.h"
#include "fqd_internal.h"

namespace {

constexpr uint32_t SG_THREADS = 1024, SG_WAVES = SG_THREADS / 64, SG_EPT = 4;
constexpr uint32_t SG_CTRL_WORDS = 64;        // changed flag, wave totals, results
constexpr uint32_t SG_ST_DROP = 2u, SG_ST_TAINT = 4u;

__device__ __forceinline__ uint32_t sg_load(const uint32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void sg_store(uint32_t *p, uint32_t v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint32_t sg_state(const uint8_t *state, uint32_t v)
{
    return (sg_load(reinterpret_cast<const uint32_t *>(state) + (v >> 2)) >> (8u * (v & 3u))) & 0xFFu;
}

// bits into state[v], whatever the other bytes of its word are doing
__device__ __forceinline__ void sg_state_or(uint8_t *state, uint32_t v, uint32_t bits)
{
    atomicOr(reinterpret_cast<uint32_t *>(state) + (v >> 2), bits << (8u * (v & 3u)));
}

// adjacency: state[v] = s where it is still 0 (bytes of one word change side by side)
__device__ __forceinline__ void sg_state_set(uint8_t *state, uint32_t v, uint32_t s)
{
    uint32_t *w = reinterpret_cast<uint32_t *>(state) + (v >> 2);
    const uint32_t sh = 8u * (v & 3u);
    uint32_t old = sg_load(w);
    while (((old >> sh) & 0xFFu) == 0u) {
        const uint32_t seen = atomicCAS(w, old, old | (s << sh));
        if (seen == old)
            break;
        old = seen;
    }
}

__device__ __forceinline__ uint32_t sg_find(uint32_t *parent, uint32_t x)
{
    uint32_t p = sg_load(&parent[x]);
    while (p != x) {
        const uint32_t g = sg_load(&parent[p]);
        if (g != p)
            sg_store(&parent[x], g);      // path halving: g is an ancestor of x whatever others have written (graph.hip uf_find)
        x = p;
        p = g;
    }
    return x;
}

// (count, key) rank: a above b. Repeated keys of an uncollapsed table compare as neither greater.
__device__ __forceinline__ bool sg_rank_greater(uint32_t a, uint32_t b, const uint32_t *cnt, const fqd::SmallGraph &A,
                                                const KeyShape &sh)
{
    const uint32_t ca = cnt[a], cb = cnt[b];
    if (ca != cb)
        return ca > cb;
    return fqd_key_cmp(A.urecs + (uint64_t)a * sh.stride, fqd_key_len(sh, A.ulens, a), A.urecs + (uint64_t)b * sh.stride,
                       fqd_key_len(sh, A.ulens, b), sh.planes, sh.words) > 0;
}

// best[dst] = max_rank(best[dst], cand)
__device__ __forceinline__ bool sg_raise_best(uint32_t *best, uint32_t dst, uint32_t cand, const uint32_t *cnt,
                                              const fqd::SmallGraph &A, const KeyShape &sh)
{
    for (;;) {
        const uint32_t old = sg_load(&best[dst]);
        if (old == cand || !sg_rank_greater(cand, old, cnt, A, sh))
            return false;
        if (atomicCAS(&best[dst], old, cand) == old)
            return true;
    }
}

// the workgroup's sum of one value per lane (every lane gets it); slots: SG_WAVES words of LDS
__device__ __forceinline__ uint32_t sg_block_sum(uint32_t x, uint32_t *slots)
{
    for (int o = 32; o; o >>= 1)
        x += __shfl_xor(x, o);
    __syncthreads();
    if (fqd_lane() == 0)
        slots[threadIdx.x >> 6] = x;
    __syncthreads();
    uint32_t sum = 0;
    for (uint32_t w = 0; w < SG_WAVES; w++)
        sum += slots[w];
    return sum;
}

// Edge e of the list, ends checked against the table; a self-loop (what graph.hip's mask_dead_edges leaves, and what
// every consumer skips) or an end outside the table: not live.
struct SgEdges {
    uint2 uv[SG_EPT];
    bool live[SG_EPT];
};

__device__ __forceinline__ void sg_load_edges(const uint32_t *edges, uint32_t E, uint32_t U, uint32_t e0, SgEdges &x)
{
#pragma unroll
    for (uint32_t t = 0; t < SG_EPT; t++) {       // (clamped, unconditional: in flight together)
        const uint32_t e = e0 + t * SG_THREADS;
        x.uv[t] = reinterpret_cast<const uint2 *>(edges)[min(e, E - 1u)];
        x.live[t] = e < E;
    }
#pragma unroll
    for (uint32_t t = 0; t < SG_EPT; t++)
        x.live[t] = x.live[t] && x.uv[t].x != x.uv[t].y && x.uv[t].x < U && x.uv[t].y < U;
}

template <bool LDS23>
__global__ __launch_bounds__(SG_THREADS) void small_graph_kernel(fqd::SmallGraph A, KeyShape sh)
{
    extern __shared__ uint32_t sg_lds[];
    const uint32_t U = A.U, E = A.E, tid = threadIdx.x, lane = fqd_lane();
    uint32_t *ctrl = sg_lds;                       // [0]: changed, [8 .. 8 + SG_WAVES): sums, [32 ..): scan of the waves
    uint32_t *r1 = sg_lds + SG_CTRL_WORDS;
    uint32_t *best = LDS23 ? r1 + A.r1_words : A.g_best;
    uint8_t *state = LDS23 ? reinterpret_cast<uint8_t *>(r1 + A.r1_words + U) : A.g_state;
    uint32_t *edges = A.edges;

    // ---- phases 1 and 2: union, flatten -------------------------------------------------------------------------
    if (A.phases & 1u) {
        uint32_t *parent = r1;
        for (uint32_t v = tid; v < U; v += SG_THREADS)
            parent[v] = v;
        __syncthreads();
        for (uint32_t e0 = tid; e0 < E; e0 += SG_THREADS * SG_EPT) {
            SgEdges x;
            sg_load_edges(edges, E, U, e0, x);
#pragma unroll
            for (uint32_t t = 0; t < SG_EPT; t++) {
                uint32_t a = x.uv[t].x, b = x.uv[t].y;
                bool active = x.live[t];
                while (active) {
                    a = sg_find(parent, a);
                    b = sg_find(parent, b);
                    if (a == b)
                        break;
                    if (a > b) {
                        const uint32_t s = a;
                        a = b;
                        b = s;
                    }
                    active = atomicCAS(&parent[b], b, a) != b;      // hook the larger root under the smaller one
                }
            }
        }
        __syncthreads();
        uint32_t roots = 0;
        for (uint32_t v = tid; v < U; v += SG_THREADS) {
            uint32_t x = v, p = sg_load(&parent[x]);
            while (p != x) {
                x = p;
                p = sg_load(&parent[x]);
            }
            A.labels[v] = x;                       // the smallest uid of v's component
            roots += x == v ? 1u : 0u;
        }
        roots = sg_block_sum(roots, ctrl + 8);
        if (tid == 0)
            A.ctr64[0] = roots;                    // C64_ROOTS
        __syncthreads();                           // (labels[] are read below; R1 changes hands)
    }
    if (!(A.phases & 2u))
        return;

    // ---- phase 3: dissect -------------------------------------------------------------------------------------------
    uint32_t *cnt = r1;
    const uint32_t *labels = A.labels;
    for (uint32_t v = tid; v < U; v += SG_THREADS) {
        cnt[v] = A.ucounts[v];
        best[v] = v;
    }
    for (uint32_t q = tid; q < (U + 3u) / 4u; q += SG_THREADS)
        reinterpret_cast<uint32_t *>(state)[q] = 0u;
    __syncthreads();
    if (A.method == FQD_METHOD_HIGHEST_COUNT) {
        for (uint32_t v = tid; v < U; v += SG_THREADS) {
            const uint32_t r = labels[v];
            if (r != v)
                sg_raise_best(best, r, v, cnt, A, sh);
        }
    } else if (A.method == FQD_METHOD_DIRECTIONAL && A.closed_form) {
        // one sweep: in-arcs of keys with count >= 2, and the components where a count-1 key meets a bigger key
        for (uint32_t e0 = tid; e0 < E; e0 += SG_THREADS * SG_EPT) {
            SgEdges x;
            sg_load_edges(edges, E, U, e0, x);
#pragma unroll
            for (uint32_t t = 0; t < SG_EPT; t++) {
                if (!x.live[t])
                    continue;
                const uint32_t u = x.uv[t].x, v = x.uv[t].y;
                const long long cu = cnt[u], cv = cnt[v];
                if (cu == 1 && cv == 1)
                    continue;
                if (cv >= 2 && 2 * cv - 1 <= cu)
                    sg_state_or(state, v, SG_ST_DROP);          // arc u -> v from a key of larger count
                if (cu >= 2 && 2 * cu - 1 <= cv)
                    sg_state_or(state, u, SG_ST_DROP);
                if (cu == 1)
                    sg_state_or(state, labels[u], SG_ST_TAINT);  // here cv >= 2: v reaches u and outranks all of u's count-1 set
                if (cv == 1)
                    sg_state_or(state, labels[v], SG_ST_TAINT);
            }
        }
        __syncthreads();
        // the largest key of every untainted component of count-1 keys
        for (uint32_t v = tid; v < U; v += SG_THREADS) {
            if (cnt[v] != 1u)
                continue;
            const uint32_t r = labels[v];
            if (r != v && !(sg_state(state, r) & SG_ST_TAINT))
                sg_raise_best(best, r, v, cnt, A, sh);
        }
    } else if (A.method == FQD_METHOD_DIRECTIONAL) {
        // relaxation sweeps of best[] to a fixed point
        for (uint32_t round = 0; E && round < U + 2u; round++) {
            if (tid == 0)
                ctrl[0] = 0u;
            __syncthreads();
            bool moved = false;
            for (uint32_t e0 = tid; e0 < E; e0 += SG_THREADS * SG_EPT) {
                SgEdges x;
                sg_load_edges(edges, E, U, e0, x);
#pragma unroll
                for (uint32_t t = 0; t < SG_EPT; t++) {
                    if (!x.live[t])
                        continue;
                    const uint32_t u = x.uv[t].x, v = x.uv[t].y;
                    const long long cu = cnt[u], cv = cnt[v];
                    if (2 * cv - 1 <= cu && sg_raise_best(best, v, sg_load(&best[u]), cnt, A, sh))      // arc u -> v
                        moved = true;
                    if (2 * cu - 1 <= cv && sg_raise_best(best, u, sg_load(&best[v]), cnt, A, sh))      // arc v -> u
                        moved = true;
                }
            }
            if (__ballot(moved) && lane == 0)
                ctrl[0] = 1u;
            __syncthreads();
            const uint32_t changed = ctrl[0];
            __syncthreads();
            if (!changed)
                break;
        }
    } else {
        // adjacency: the end of higher rank first, once, in place (graph.hip orient_edges_kernel) ...
        for (uint32_t e0 = tid; e0 < E; e0 += SG_THREADS * SG_EPT) {
            SgEdges x;
            sg_load_edges(edges, E, U, e0, x);
#pragma unroll
            for (uint32_t t = 0; t < SG_EPT; t++)
                if (x.live[t] && !sg_rank_greater(x.uv[t].x, x.uv[t].y, cnt, A, sh))
                    reinterpret_cast<uint2 *>(edges)[e0 + t * SG_THREADS] = make_uint2(x.uv[t].y, x.uv[t].x);
        }
        // ... then rounds over state and stamps until a round changes nothing. stamp[v] == round: v still has an
        // undecided neighbour of higher rank (best[v] = v < U never equals a stamp U + round)
        uint32_t *stamp = best;
        for (uint32_t round = 1; round <= U + 2u; round++) {
            if (tid == 0)
                ctrl[0] = 0u;
            __syncthreads();                       // (and the oriented edges are in place)
            bool moved = false;                    // a key dropped or kept in this round
            for (uint32_t e0 = tid; e0 < E; e0 += SG_THREADS * SG_EPT) {
                SgEdges x;
                sg_load_edges(edges, E, U, e0, x);
#pragma unroll
                for (uint32_t t = 0; t < SG_EPT; t++) {
                    if (!x.live[t])
                        continue;
                    const uint32_t hi = x.uv[t].x, lo = x.uv[t].y;
                    if (sg_state(state, lo) != 0u)
                        continue;
                    const uint32_t s_hi = sg_state(state, hi);
                    if (s_hi == 1u) {
                        sg_state_set(state, lo, 2u);
                        moved = true;
                    } else if (s_hi == 0u) {
                        sg_store(&stamp[lo], U + round);
                    }
                }
            }
            __syncthreads();
            for (uint32_t v = tid; v < U; v += SG_THREADS)
                if (sg_state(state, v) == 0u && sg_load(&stamp[v]) != U + round) {
                    sg_state_set(state, v, 1u);
                    moved = true;
                }
            if (__ballot(moved) && lane == 0)
                ctrl[0] = 1u;
            __syncthreads();
            const uint32_t changed = ctrl[0];
            __syncthreads();
            if (!changed)
                break;
        }
    }
    __syncthreads();

    // ---- phase 4: kept flags, counters, the ascending list of kept first-holder ids ---------------------------------
    // verdicts first (they read the counts in R1), one bit per key of this lane; then R1 becomes the window's bit map
    uint32_t mine = 0, n_kept = 0;
    for (uint32_t v = tid, i = 0; v < U; v += SG_THREADS, i++) {
        bool k;
        if (A.method == FQD_METHOD_HIGHEST_COUNT) {
            k = sg_load(&best[labels[v]]) == v;
        } else if (A.method == FQD_METHOD_DIRECTIONAL && A.closed_form) {
            if (cnt[v] == 1u) {
                const uint32_t r = labels[v];
                k = !(sg_state(state, r) & SG_ST_TAINT) && sg_load(&best[r]) == v;
            } else {
                k = !(sg_state(state, v) & SG_ST_DROP);
            }
        } else if (A.method == FQD_METHOD_DIRECTIONAL) {
            k = sg_load(&best[v]) == v;
        } else {
            k = sg_state(state, v) == 1u;
        }
        A.kept[v] = k ? 1 : 0;
        mine |= (k ? 1u : 0u) << i;
        n_kept += k ? 1u : 0u;
    }
    n_kept = sg_block_sum(n_kept, ctrl + 8);       // (its barriers: every verdict is out before R1 is cleared)
    const uint32_t n_words = (uint32_t)((A.window + 31u) >> 5);
    uint32_t *map = r1;
    for (uint32_t w = tid; w < n_words; w += SG_THREADS)
        map[w] = 0u;
    __syncthreads();
    for (uint32_t v = tid, i = 0; v < U; v += SG_THREADS, i++) {
        if (!((mine >> i) & 1u))
            continue;
        const uint64_t id = A.ufirst[v];
        if (id >= A.base && id - A.base < A.window) {
            const uint32_t at = (uint32_t)(id - A.base);
            atomicOr(&map[at >> 5], 1u << (at & 31u));
        }
    }
    __syncthreads();
    // lane t owns words [t * wpl, (t + 1) * wpl): consecutive ids, so the lanes' runs are ascending as they stand
    const uint32_t wpl = (n_words + SG_THREADS - 1u) / SG_THREADS;
    const uint32_t w0 = min(tid * wpl, n_words), w1 = min(w0 + wpl, n_words);
    uint32_t own = 0;
    for (uint32_t w = w0; w < w1; w++)
        own += (uint32_t)__popc(map[w]);
    uint32_t incl = own;                           // prefix sum over the wave, then over the waves' totals
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o);
        if (lane >= o)
            incl += up;
    }
    if (lane == 63)
        ctrl[32 + (tid >> 6)] = incl;
    __syncthreads();
    uint32_t at = incl - own, listed = 0;
    for (uint32_t w = 0; w < SG_WAVES; w++) {
        const uint32_t c = ctrl[32 + w];
        at += w < (tid >> 6) ? c : 0u;
        listed += c;
    }
    for (uint32_t w = w0; w < w1; w++) {
        uint32_t bits = map[w];
        while (bits) {
            const uint32_t b = (uint32_t)__ffs((int)bits) - 1u;
            bits &= bits - 1u;
            A.list_out[at++] = A.base + ((uint64_t)w << 5) + b;
        }
    }
    if (tid == 0) {
        A.ctr64[1] = n_kept;                       // C64_SUM
        A.ctr64[2] = listed;                       // (the slot behind it: ids listed)
    }
}

}  // namespace

namespace fqd {

size_t small_graph_lds_bytes(const SmallGraph &A, bool lds23)
{
    size_t words = SG_CTRL_WORDS + A.r1_words;
    if (lds23)
        words += A.U + (A.U + 3u) / 4u;
    return words * 4;
}

hipError_t launch_small_graph(SmallGraph A, KeyShape sh, hipStream_t st)
{
    if (!A.U || A.U > SMALL_GRAPH_MAX_U_GLOBAL || A.E > SMALL_GRAPH_MAX_E || A.window > SMALL_GRAPH_MAX_WINDOW)
        return hipErrorInvalidValue;
    const bool lds23 = A.U <= SMALL_GRAPH_LDS_U;
    if (!lds23 && (!A.g_best || !A.g_state))
        return hipErrorInvalidValue;
    A.r1_words = std::max<uint32_t>(A.U, (uint32_t)((A.window + 31u) >> 5));
    const size_t lds = small_graph_lds_bytes(A, lds23);
    if (lds > 80 * 1024)
        return hipErrorInvalidValue;
    const void *fn = lds23 ? reinterpret_cast<const void *>(&small_graph_kernel<true>)
                           : reinterpret_cast<const void *>(&small_graph_kernel<false>);
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess)
            return e;
    }
    if (lds23)
        small_graph_kernel<true><<<1, SG_THREADS, lds, st>>>(A, sh);
    else
        small_graph_kernel<false><<<1, SG_THREADS, lds, st>>>(A, sh);
    return hipGetLastError();
}

}  // namespace fqd
