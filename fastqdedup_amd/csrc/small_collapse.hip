// small_collapse.hip -- stage 2 for small inputs: the whole exact-duplicate collapse (collapse.hip explains
// what it computes) in one launch that does the work and a small one behind it that writes the table, without a
// sort, a scan or a library call, and with one read-back behind both.
// For inputs of which a hash bin's DISTINCT keys fit a workgroup's LDS; the reads of a bin are never held
// anywhere, so one key with tens of thousands of copies costs atomics and nothing else.
//
// Grid = NB workgroups, NB the power of two with n / NB <= CAP / 2. Workgroup b owns the reads whose 32-bit key
// hash has b in its top log2(NB) bits; it streams the hash array twice (16-byte loads, 4 n bytes, out of L2):
//   claim    an open-addressed LDS table of >= 2 CAP slots, linear probing, a slot claimed by a CAS on the (masked)
//            hash value; atomicMin(rep[slot], position) leaves the EARLIEST read of the hash value as the slot's
//            representative. Lanes of a wave that hold the same hash value send one CAS and one min between them
//            (the lowest lane holds the smallest position). More than CAP claims: the overflow word is raised.
//   number   the claimed slots get dense numbers 0 .. claims - 1 (ballot + one LDS atomic per wave); with USE_LDS
//            the representatives' key words -- the first ceil(K W / 4) uint4 of their rows -- are staged in LDS.
//   count    second pass over the hashes: a read finds its slot and compares its row with the representative's
//            (uint4 by uint4, early exit; the lengths too when the keys are ragged: positions past a key's end
//            hold code 0). Equal: its weight is added to the slot's count, one LDS atomic per wave and slot where
//            lanes agree. Different (the 32-bit hashes collided): the position goes to a list of 256 entries; a
//            full list raises the overflow word.
//   collide  one wave, all pairs inside the list: an entry's leader is the entry of smallest position with an
//            equal row; leaders become rows of their own, their counts kept beside the list.
//   park     slots and leaders with a count != 0 are the bin's rows (a key whose weights sum to 0 is left out, as
//            run_weights_kernel does): numbered by ballot, added to the global row counter and the counted weight
//            with one atomic each, then RANKED by position in LDS (a row's rank is the number of rows with a
//            smaller position) and parked as (position, count) in global memory in that order. A bin's rows are
//            reads of that bin, so its entries start where its reads would: at the number of reads in the bins
//            below it, which the workgroup counted during the claim pass. No workgroup waits for another.
// The last workgroup to finish (a ticket counter) moves rows, counted weight and the overflow word to the words
// the host reads back and clears the running counters for the next job: no memset in front of the launch.
// small_collapse_emit_kernel, the second launch (a workgroup per bin again): adds up the row counts of the bins below
// its own and writes its rows behind them with stride / 4 lanes per row, padding words as zero. The first holder is
// the representative: the smallest position among ALL reads of the key, weight 0 included. So the table is ordered
// by (bin, first position) and two jobs over one input number their keys alike; the atomics above, whose order
// differs from run to run, decide nothing that is seen outside.
//
// LDS at CAP = 1024: 27 712 B of tables (key + rep per slot, rep + count per dense number, the collision list)
// plus CAP x ceil(K W / 4) x 16 B of staged rows while the total stays within 80 KB:
//   one uint4 of key words (32 nt over "ACGNT")     44 096 B   3 workgroups per CU
//   three (65-128 nt over "ACGNT")                  76 864 B   2 workgroups per CU
//   more (300 nt: eight)                            27 712 B   5 workgroups per CU, rows compared from global memory
#include "fqd_internal.h"

#include <cstdlib>

namespace {

constexpr uint32_t SC_EMPTY = 0xFFFFFFFFu;     // free table slot
constexpr uint32_t SC_COLL = 256;              // entries of the collision list
constexpr uint32_t SC_MAX_THREADS = 512;
constexpr uint32_t SC_DEFAULT_CAP = 1024;      // distinct keys per bin
constexpr uint32_t SC_LDS_BUDGET = 80 * 1024;  // half a CU's LDS
// ctl words of the workgroup
enum { SC_CLAIMS = 0, SC_OVER = 1, SC_NCOLL = 2, SC_ROWS = 3, SC_SUM = 4 /* and 5 */, SC_BELOW = 6, SC_DENSE = 7 };

struct SmallCollapse {
    const uint32_t *hashes, *recs, *lens /* NULL: fixed length */, *weights /* NULL: 1 */;
    const uint64_t *read_ids;                  // NULL: a read's id is its position
    uint32_t n, nb_bits, cap, slots, hash_mask;
    uint32_t Q, Qc, KW;                        // uint4 per row; uint4 that hold key words; key words
    uint32_t *urecs, *ulens, *ucounts;
    uint64_t *ufirst;
    uint32_t *ctr;                             // fqd::SMALL_COLLAPSE_CTR_WORDS words, see fqd_internal.h
    uint32_t *bin_rows, *bin_start;            // [NB] rows of a bin; reads in the bins below it
    uint2 *park;                               // [n] (position, count) of a bin's rows, from bin_start[bin] on
};

struct CollapseLds {
    uint4 *tile;         // [cap * Qc] when USE_LDS
    uint32_t *key;       // [slots] claimed hash values; at emit: the rows' positions
    uint32_t *rep;       // [slots] smallest position, then the slot's dense number; at emit: the rows' counts
    uint32_t *drep;      // [cap] representative of dense number d
    uint32_t *dcnt;      // [cap]
    uint32_t *cpos;      // [SC_COLL] positions whose row differs from their slot's representative
    uint32_t *ccnt;      // [SC_COLL] summed weight of the entries led by this one
    uint32_t *clead;     // [SC_COLL]
    uint32_t *ctl;       // [16]
};

__device__ __forceinline__ bool sc_ne(const uint4 &x, const uint4 &y)
{
    return ((x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w)) != 0u;
}

// n uint4 of two rows, four at a time: the loads of a step are in flight together (a row of 300 nt is eight of them,
// and a lane that waited for each in turn held up its wave), the exit is after every step
__device__ __forceinline__ bool sc_same_quads(const uint4 *pa, const uint4 *pb, uint32_t n)
{
    for (uint32_t q = 0; q < n; q += 4) {
        uint4 x[4], y[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t at = q + k < n ? q + k : q;      // (a step's spare loads repeat its first)
            x[k] = pa[at];
            y[k] = pb[at];
        }
        if (sc_ne(x[0], y[0]) || sc_ne(x[1], y[1]) || sc_ne(x[2], y[2]) || sc_ne(x[3], y[3]))
            return false;
    }
    return true;
}

// rows of positions a and b in global memory (the uint4 behind the key words hold zeros, or the length that is
// compared anyway)
__device__ __forceinline__ bool sc_same_global(const SmallCollapse &A, uint32_t a, uint32_t b)
{
    const uint4 *pa = reinterpret_cast<const uint4 *>(A.recs) + (uint64_t)a * A.Q;
    const uint4 *pb = reinterpret_cast<const uint4 *>(A.recs) + (uint64_t)b * A.Q;
    if (!sc_same_quads(pa, pb, A.Qc))
        return false;
    return !A.lens || A.lens[a] == A.lens[b];
}

template <bool USE_LDS>
__device__ __forceinline__ bool sc_same_rep(const SmallCollapse &A, const CollapseLds &L, uint32_t pos, uint32_t d,
                                            uint32_t rep)
{
    if (!USE_LDS)
        return sc_same_global(A, pos, rep);
    const uint4 *pa = reinterpret_cast<const uint4 *>(A.recs) + (uint64_t)pos * A.Q;
    const uint4 *pb = L.tile + d * A.Qc;
    if (!sc_same_quads(pa, pb, A.Qc))
        return false;
    return !A.lens || A.lens[pos] == A.lens[rep];
}

// the hash value a read is filed under, and whether this bin owns it
__device__ __forceinline__ bool sc_mine(const SmallCollapse &A, uint32_t bin, bool in_range, uint32_t pos, uint32_t raw,
                                        uint32_t &h)
{
    h = raw & A.hash_mask;
    if (h == SC_EMPTY)
        h = SC_EMPTY - 1u;         // (the free mark is no hash value; sharing a slot costs a compare and a list entry)
    return in_range && pos < A.n && (A.nb_bits == 0 || (raw >> (32u - A.nb_bits)) == bin);
}

template <bool USE_LDS>
__device__ __forceinline__ void sc_bin(const SmallCollapse &A, const CollapseLds &L, uint32_t bin)
{
    const uint32_t T = blockDim.x, tid = threadIdx.x, lane = tid & 63u;
    const uint32_t smask = A.slots - 1u;
    const uint32_t nv = (A.n + 3u) >> 2;       // (the hash array is readable up to the end of its last uint4)
    const uint4 *src = reinterpret_cast<const uint4 *>(A.hashes);
    uint4 ahead;

    for (uint32_t s = tid; s < A.slots; s += T) {
        L.key[s] = SC_EMPTY;
        L.rep[s] = 0xFFFFFFFFu;
    }
    for (uint32_t i = tid; i < SC_COLL; i += T)
        L.ccnt[i] = 0;
    if (tid < 16)
        L.ctl[tid] = 0;
    __syncthreads();

    // ---- claim: one slot per hash value, its representative the earliest read; on the way the reads of the bins
    // below this one are counted: that many entries of park[] lie in front of this bin's
    uint32_t below = 0;
    ahead = tid < nv ? src[tid] : make_uint4(0, 0, 0, 0);
    for (uint32_t vb = 0; vb < nv; vb += T) {
        const uint32_t v = vb + tid;
        const uint4 q4 = ahead;                 // (the next step's hashes are on their way while this step's are filed)
        ahead = v + T < nv ? src[v + T] : make_uint4(0, 0, 0, 0);
        const uint32_t raw[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const uint32_t pos = v * 4u + e;
            uint32_t h;
            bool active = sc_mine(A, bin, v < nv, pos, raw[e], h);
            below += v < nv && pos < A.n && A.nb_bits != 0 && (raw[e] >> (32u - A.nb_bits)) < bin;
            // lanes with one hash value: the lowest of them (the smallest position) claims for all; two rounds take
            // the heavy keys, whoever is left goes alone
            bool leads = false;
            for (int round = 0; round < 2; round++) {
                const unsigned long long m = __ballot(active && !leads);
                if (!m)
                    break;
                const int leader = __ffsll((long long)m) - 1;
                const uint32_t hl = __shfl(h, leader);
                if (active && !leads && h == hl) {
                    if ((int)lane == leader)
                        leads = true;
                    else
                        active = false;
                }
            }
            if (active) {
                uint32_t slot = h & smask;
                bool found = false;
                for (uint32_t probe = 0; probe < A.slots; probe++) {
                    const uint32_t was = atomicCAS(&L.key[slot], SC_EMPTY, h);
                    if (was == SC_EMPTY && atomicAdd(&L.ctl[SC_CLAIMS], 1u) >= A.cap)
                        L.ctl[SC_OVER] = 1u;
                    if (was == SC_EMPTY || was == h) {
                        found = true;
                        break;
                    }
                    slot = (slot + 1u) & smask;
                }
                if (found)
                    atomicMin(&L.rep[slot], pos);
                else
                    L.ctl[SC_OVER] = 1u;       // (the table is full: more than 2 CAP hash values)
            }
        }
    }
    for (int o = 32; o; o >>= 1)
        below += __shfl_xor(below, o);
    if (lane == 0 && below)
        atomicAdd(&L.ctl[SC_BELOW], below);
    __syncthreads();
    if (L.ctl[SC_OVER])
        return;

    // ---- number: dense numbers for the claimed slots
    for (uint32_t sb = 0; sb < A.slots; sb += T) {
        const uint32_t s = sb + tid;
        const bool claimed = s < A.slots && L.key[s] != SC_EMPTY;
        const unsigned long long m = __ballot(claimed);
        if (m) {
            uint32_t at = 0;
            if (lane == 0)
                at = atomicAdd(&L.ctl[SC_DENSE], (uint32_t)__popcll(m));
            at = __shfl(at, 0);
            if (claimed) {
                const uint32_t d = at + (uint32_t)__popcll(m & fqd_lanemask_lt());
                L.drep[d] = L.rep[s];
                L.dcnt[d] = 0;
                L.rep[s] = d;
            }
        }
    }
    __syncthreads();
    const uint32_t n_dense = L.ctl[SC_DENSE];          // <= cap
    if (USE_LDS) {
        for (uint32_t i = tid; i < n_dense * A.Qc; i += T) {
            const uint32_t d = i / A.Qc, q = i - d * A.Qc;
            L.tile[i] = (reinterpret_cast<const uint4 *>(A.recs) + (uint64_t)L.drep[d] * A.Q)[q];
        }
        __syncthreads();
    }

    // ---- count: every read against its slot's representative
    ahead = tid < nv ? src[tid] : make_uint4(0, 0, 0, 0);
    for (uint32_t vb = 0; vb < nv; vb += T) {
        const uint32_t v = vb + tid;
        const uint4 q4 = ahead;                 // (the next step's hashes are on their way while this step's are filed)
        ahead = v + T < nv ? src[v + T] : make_uint4(0, 0, 0, 0);
        const uint32_t raw[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const uint32_t pos = v * 4u + e;
            uint32_t h, d = 0, w = 0;
            const bool active = sc_mine(A, bin, v < nv, pos, raw[e], h);
            bool add = false;
            uint32_t slot = h & smask;
            if (active)     // (claimed in the first pass: it is there)
                for (uint32_t probe = 0; L.key[slot] != h && probe < A.slots; probe++)
                    slot = (slot + 1u) & smask;
            if (active && L.key[slot] == h) {
                d = L.rep[slot];
                const uint32_t rep = L.drep[d];
                w = A.weights ? A.weights[pos] : 1u;
                if (pos == rep || sc_same_rep<USE_LDS>(A, L, pos, d, rep)) {
                    add = w != 0u;
                } else {
                    const uint32_t at = atomicAdd(&L.ctl[SC_NCOLL], 1u);
                    if (at < SC_COLL)
                        L.cpos[at] = pos;
                    else
                        L.ctl[SC_OVER] = 1u;
                }
            } else if (active) {
                L.ctl[SC_OVER] = 1u;
            }
            for (int round = 0; round < 2; round++) {
                const unsigned long long m = __ballot(add);
                if (!m)
                    break;
                const int leader = __ffsll((long long)m) - 1;
                const uint32_t dl = __shfl(d, leader);
                const bool same = add && d == dl;
                uint32_t sum = same ? w : 0u;
                for (int o = 32; o; o >>= 1)
                    sum += __shfl_xor(sum, o);
                if ((int)lane == leader)
                    atomicAdd(&L.dcnt[dl], sum);
                if (same)
                    add = false;
            }
            if (add)
                atomicAdd(&L.dcnt[d], w);
        }
    }
    __syncthreads();
    if (L.ctl[SC_OVER])
        return;

    // ---- collide: all pairs inside the list, one wave
    const uint32_t n_coll = L.ctl[SC_NCOLL];           // <= SC_COLL
    if (tid < 64)
        for (uint32_t i = lane; i < n_coll; i += 64) {
            const uint32_t pi = L.cpos[i];
            uint32_t best = i, best_pos = pi;
            for (uint32_t j = 0; j < n_coll; j++) {
                const uint32_t pj = L.cpos[j];
                if (pj < best_pos && sc_same_global(A, pi, pj)) {
                    best = j;
                    best_pos = pj;
                }
            }
            L.clead[i] = best;
            const uint32_t w = A.weights ? A.weights[pi] : 1u;
            if (w)
                atomicAdd(&L.ccnt[best], w);
        }
    __syncthreads();

    // ---- park: the rows with a count, numbered, then ranked by position
    uint32_t *orep = L.key, *ocnt = L.rep;             // (slots >= cap + SC_COLL; neither table is read any more)
    unsigned long long wsum = 0;
    for (uint32_t base = 0; base < n_dense + n_coll; base += T) {
        const uint32_t x = base + tid;
        uint32_t cnt = 0, p = 0;
        if (x < n_dense) {
            cnt = L.dcnt[x];
            p = L.drep[x];
        } else if (x < n_dense + n_coll && L.clead[x - n_dense] == x - n_dense) {
            cnt = L.ccnt[x - n_dense];
            p = L.cpos[x - n_dense];
        }
        wsum += cnt;
        const unsigned long long m = __ballot(cnt != 0u);
        if (m) {
            uint32_t at = 0;
            if (lane == 0)
                at = atomicAdd(&L.ctl[SC_ROWS], (uint32_t)__popcll(m));
            at = __shfl(at, 0);
            if (cnt) {
                const uint32_t r = at + (uint32_t)__popcll(m & fqd_lanemask_lt());
                orep[r] = p;
                ocnt[r] = cnt;
            }
        }
    }
    for (int o = 32; o; o >>= 1)
        wsum += __shfl_xor(wsum, o);
    if (lane == 0 && wsum)
        atomicAdd(reinterpret_cast<unsigned long long *>(&L.ctl[SC_SUM]), wsum);
    __syncthreads();
    const uint32_t n_rows = L.ctl[SC_ROWS];
    const uint32_t start = L.ctl[SC_BELOW];
    if (tid == 0) {
        A.bin_start[bin] = start;
        if (n_rows) {
            atomicAdd(&A.ctr[0], n_rows);
            atomicAdd(reinterpret_cast<unsigned long long *>(A.ctr + 4),
                      *reinterpret_cast<unsigned long long *>(&L.ctl[SC_SUM]));
        }
    }
    // The numbers above follow the order in which waves and slots met, which differs from run to run. A row's place
    // among the bin's rows is the number of rows with a smaller position (the positions are distinct reads of this bin;
    // all lanes read one LDS word at a time: a broadcast), so the table comes out ordered by (bin, first position)
    // whatever happened on the way. The rows of a bin are reads of that bin: start + rank < n.
    for (uint32_t r = tid; r < n_rows; r += T) {
        const uint32_t p = orep[r];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < n_rows; j++)
            rank += orep[j] < p;
        A.park[start + rank] = make_uint2(p, ocnt[r]);
    }
}

// The table: workgroup b adds up the rows of the bins below b and writes its own behind them, stride / 4 lanes per row
// (a row's stores are one run), padding words as zero. Nothing is written after an overflow.
__global__ __launch_bounds__(256) void small_collapse_emit_kernel(SmallCollapse A)
{
    __shared__ uint32_t s_row0;
    const uint32_t T = blockDim.x, tid = threadIdx.x, bin = blockIdx.x;
    if (A.ctr[9])
        return;
    if (tid == 0)
        s_row0 = 0;
    __syncthreads();
    uint32_t part = 0;
    for (uint32_t j = tid; j < bin; j += T)
        part += A.bin_rows[j];
    for (int o = 32; o; o >>= 1)
        part += __shfl_xor(part, o);
    if ((tid & 63u) == 0 && part)
        atomicAdd(&s_row0, part);
    __syncthreads();
    const uint32_t row0 = s_row0, n_rows = A.bin_rows[bin], start = A.bin_start[bin];
    if ((uint64_t)row0 + n_rows > A.n || (uint64_t)start + n_rows > A.n)       // (the rows are distinct reads: it holds)
        return;
    const uint2 *park = A.park + start;
    for (uint32_t i = tid; i < n_rows * A.Q; i += T) {
        const uint32_t r = i / A.Q, q = i - r * A.Q;
        const uint2 pc = park[r];
        const uint32_t p = pc.x;
        uint4 val = (reinterpret_cast<const uint4 *>(A.recs) + (uint64_t)p * A.Q)[q];
        const uint32_t j = q * 4u;
        val.x = j + 0u < A.KW ? val.x : 0u;
        val.y = j + 1u < A.KW ? val.y : 0u;
        val.z = j + 2u < A.KW ? val.z : 0u;
        val.w = j + 3u < A.KW ? val.w : 0u;
        (reinterpret_cast<uint4 *>(A.urecs) + (uint64_t)(row0 + r) * A.Q)[q] = val;
        if (q == 0) {
            if (A.lens)
                A.ulens[row0 + r] = A.lens[p];
            A.ucounts[row0 + r] = pc.y;
            A.ufirst[row0 + r] = A.read_ids ? A.read_ids[p] : (uint64_t)p;
        }
    }
}

template <bool USE_LDS>
__global__ __launch_bounds__(SC_MAX_THREADS) void small_collapse_kernel(SmallCollapse A)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    CollapseLds L;
    L.tile = reinterpret_cast<uint4 *>(smem);
    L.key = smem + (USE_LDS ? A.cap * A.Qc * 4u : 0u);
    L.rep = L.key + A.slots;
    L.drep = L.rep + A.slots;
    L.dcnt = L.drep + A.cap;
    L.cpos = L.dcnt + A.cap;
    L.ccnt = L.cpos + SC_COLL;
    L.clead = L.ccnt + SC_COLL;
    L.ctl = L.clead + SC_COLL;

    sc_bin<USE_LDS>(A, L, blockIdx.x);     // (leaves early, as one, when the bin overflowed)

    __syncthreads();
    if (threadIdx.x == 0) {
        A.bin_rows[blockIdx.x] = L.ctl[SC_OVER] ? 0u : L.ctl[SC_ROWS];
        if (L.ctl[SC_OVER])
            atomicOr(&A.ctr[1], 1u);
        __threadfence();
        if (atomicAdd(&A.ctr[2], 1u) == gridDim.x - 1u) {
            // the last workgroup: results to the words the host reads, the running counters back to zero
            __threadfence();
            unsigned long long *sum = reinterpret_cast<unsigned long long *>(A.ctr + 4);
            A.ctr[8] = atomicExch(&A.ctr[0], 0u);
            A.ctr[9] = atomicExch(&A.ctr[1], 0u);
            *reinterpret_cast<unsigned long long *>(A.ctr + 10) = atomicExch(sum, 0ull);
            atomicExch(&A.ctr[2], 0u);
        }
    }
}

template <bool USE_LDS>
hipError_t small_collapse_go(const SmallCollapse &A, unsigned grid, unsigned threads, size_t lds, hipStream_t st)
{
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&small_collapse_kernel<USE_LDS>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess)
            return e;
    }
    small_collapse_kernel<USE_LDS><<<grid, threads, lds, st>>>(A);
    small_collapse_emit_kernel<<<grid, 256, 0, st>>>(A);
    return hipGetLastError();
}

}  // namespace

namespace fqd {

hipError_t launch_small_collapse(const uint32_t *hashes, const uint32_t *recs, const uint32_t *lens, uint64_t n,
                                 KeyShape sh, const uint32_t *weights, const uint64_t *read_ids, uint32_t *urecs,
                                 uint32_t *ulens, uint32_t *ucounts, uint64_t *ufirst, uint32_t *ctr, uint32_t *park,
                                 hipStream_t st)
{
    if (n < 1 || n >= SMALL_COLLAPSE_MAX_N || (sh.stride & 3u) || sh.stride > 256 || sh.planes * sh.words > sh.stride)
        return hipErrorInvalidValue;
    SmallCollapse A;
    A.hashes = hashes;
    A.recs = recs;
    A.lens = sh.ragged ? lens : nullptr;
    A.weights = weights;
    A.read_ids = read_ids;
    A.n = (uint32_t)n;
    A.cap = SC_DEFAULT_CAP;
    if (const char *e = getenv("FQD_SMALL_COLLAPSE_CAP"))     // tests: many bins, overflow on small inputs
        A.cap = (uint32_t)strtoul(e, nullptr, 10);
    A.cap = (A.cap < 8 ? 8 : (A.cap > SC_DEFAULT_CAP ? SC_DEFAULT_CAP : A.cap)) & ~3u;
    A.hash_mask = 0xFFFFFFFFu;
    if (const char *e = getenv("FQD_SMALL_HASH_MASK"))        // tests: distinct keys on one slot
        A.hash_mask = (uint32_t)strtoul(e, nullptr, 0);
    // (the bins follow the default CAP: a smaller one leaves them as they are and makes them overflow)
    A.nb_bits = 0;
    while ((n >> A.nb_bits) > SC_DEFAULT_CAP / 2)
        A.nb_bits++;
    A.slots = 512;                                            // a power of two >= 2 cap and >= cap + SC_COLL
    while (A.slots < 2 * A.cap)
        A.slots <<= 1;
    A.Q = sh.stride / 4;
    A.KW = sh.planes * sh.words;
    A.Qc = (A.KW + 3) / 4;
    A.urecs = urecs;
    A.ulens = ulens;
    A.ucounts = ucounts;
    A.ufirst = ufirst;
    A.ctr = ctr;
    A.bin_rows = park;
    A.bin_start = park + SMALL_COLLAPSE_MAX_BINS;
    A.park = reinterpret_cast<uint2 *>(park + 2 * SMALL_COLLAPSE_MAX_BINS);
    const size_t base_words = (size_t)2 * A.slots + 2 * A.cap + 3 * SC_COLL + 16;
    const size_t tile_words = (size_t)A.cap * A.Qc * 4;
    const bool use_lds = (base_words + tile_words) * 4 <= SC_LDS_BUDGET;
    const size_t lds = (base_words + (use_lds ? tile_words : 0)) * 4;
    const unsigned threads = n >= 8192 ? SC_MAX_THREADS : 256;
    const unsigned grid = 1u << A.nb_bits;
    if (grid > SMALL_COLLAPSE_MAX_BINS)
        return hipErrorInvalidValue;
    return use_lds ? small_collapse_go<true>(A, grid, threads, lds, st) : small_collapse_go<false>(A, grid, threads, lds, st);
}

}  // namespace fqd
