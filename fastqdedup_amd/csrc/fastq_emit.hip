// fastq_emit.hip -- pass 2 of the command line on the device: the kept records of one chunk, compacted into the
// exact output bytes of every file. Replaces the host's write loop over the records that
// filter_fastq_files_on_set selects (reference __init__.py:189-206): for every kept record, in order,
//     '@' name '\n' sequence '\n' '+' '\n' quality '\n'
// (dnaio's fastq_bytes: no '\r', a bare '+' line, a final newline also where the input has none).
//
// Two kernels per file, neither of which waits on another workgroup:
//   1. sizes   one lane per candidate j < min(n, kept ids left): kept[kept_from + j] is taken when it lies below
//              base + n (the ids are ascending, distinct and >= base: no search); its output size is
//              name_len + 2 * seq_len + 6. The sizes are scanned (prims.hip) between the two kernels.
//   2. copy    the work is split by OUTPUT bytes, not by records (the kept share is anything between a few per cent
//              and all of them): workgroup t owns bytes [t * T, (t + 1) * T) of the file's output. It finds the
//              records that overlap its tile by binary search in the inclusive scan, assembles the tile in LDS --
//              one wave per record, a lane per aligned 4-byte word of the tile, the source read in place from the
//              block (only kept records are touched: nothing is staged) -- and stores it with 16-byte stores.
//              A record longer than T simply overlaps several tiles. The grid comes from a bound the host knows
//              (a normalised record is never longer than its raw form but for one supplied newline); workgroups
//              behind the scanned total leave at once, so no read-back lies between the two kernels.
#include "fqd_internal.h"

namespace {

using fqd::FQ_EMIT_TILE;

constexpr uint32_t FE_THREADS = 256;
constexpr uint32_t FE_WAVES = FE_THREADS / 64;
static_assert(FQ_EMIT_TILE % (FE_THREADS * 16) == 0, "the store loop takes whole rounds of 16-byte units");

__global__ void fastq_emit_init_kernel(uint32_t *__restrict__ ctr)
{
    if (threadIdx.x < fqd::FQE_WORDS)
        ctr[threadIdx.x] = 0u;
}

// ---- 1. sizes ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FE_THREADS) void fastq_emit_sizes_kernel(const uint32_t *__restrict__ spans, uint32_t rec_cap,
                                                                      uint32_t file, uint32_t n, uint64_t base,
                                                                      const unsigned long long *__restrict__ kept,
                                                                      uint32_t m, uint32_t *__restrict__ sizes,
                                                                      uint32_t *__restrict__ ctr)
{
    const uint32_t j = blockIdx.x * FE_THREADS + threadIdx.x;
    if (j == 0)
        ctr[fqd::FQE_CONSUMED + file] = spans[fqd::FQS_REC_END * rec_cap + n - 1];
    if (j >= m)
        return;
    const unsigned long long id = kept[j];
    uint32_t size = 0;
    if (id < base) {
        atomicOr(&ctr[fqd::FQE_FAULT], 1u);
    } else if (id - base < n) {
        const uint32_t r = (uint32_t)(id - base);
        size = spans[fqd::FQS_NAME_LEN * rec_cap + r] + 2u * spans[fqd::FQS_SEQ_LEN * rec_cap + r] + 6u;
        // the last taken candidate says how many there are (ascending ids: the taken ones come first)
        if (file == 0 && (j + 1 == m || kept[j + 1] - base >= n))
            ctr[fqd::FQE_TAKEN] = j + 1;
    }
    sizes[j] = size;
}

// ---- 2. copy -------------------------------------------------------------------------------------------
// first j in [0, m) with incl[j] > v (upper = true) or incl[j] >= v (upper = false); m when there is none
__device__ __forceinline__ uint32_t scan_bound(const uint32_t *__restrict__ incl, uint32_t m, uint32_t v, bool upper)
{
    uint32_t a = 0, b = m;
    while (a < b) {
        const uint32_t mid = a + ((b - a) >> 1);
        const uint32_t x = incl[mid];
        if (upper ? x > v : x >= v)
            b = mid;
        else
            a = mid + 1;
    }
    return a;
}

// one kept record as the copy kernel sees it: where its pieces start in the output record and in the block
struct EmitRecord {
    uint32_t name_at, seq_at, qual_at;     // block positions of the three strings
    uint32_t seq_q, plus_q, qual_q, end_q; // output positions of the newline before the sequence, of "\n+\n", of the
                                           // quality string and of the last newline
    // byte q of '@' name '\n' sequence "\n+\n" quality '\n'
    __device__ __forceinline__ uint32_t byte_at(const uint8_t *__restrict__ src, uint32_t q) const
    {
        if (q >= qual_q)
            return q == end_q ? (uint32_t)'\n' : src[qual_at + (q - qual_q)];
        if (q >= plus_q)
            return q == plus_q + 1u ? (uint32_t)'+' : (uint32_t)'\n';
        if (q > seq_q)
            return src[seq_at + (q - seq_q - 1u)];
        if (q == seq_q)
            return (uint32_t)'\n';
        return q ? src[name_at + (q - 1u)] : (uint32_t)'@';
    }
};

__global__ __launch_bounds__(FE_THREADS) void fastq_emit_copy_kernel(const uint8_t *__restrict__ src,
                                                                     const uint32_t *__restrict__ spans, uint32_t rec_cap,
                                                                     uint32_t file, uint32_t n, uint64_t base,
                                                                     const unsigned long long *__restrict__ kept,
                                                                     uint32_t m, const uint32_t *__restrict__ incl,
                                                                     uint8_t *__restrict__ out, uint64_t out_capacity,
                                                                     uint32_t *__restrict__ ctr)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_tile[FQ_EMIT_TILE];
    __shared__ uint32_t s_first, s_last;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t total = incl[m - 1];
    if (blockIdx.x == 0 && tid == 0) {
        ctr[fqd::FQE_BYTES + file] = total;
        if (total > out_capacity)
            atomicOr(&ctr[fqd::FQE_OVERFLOW], 1u);
    }
    const uint64_t lo64 = (uint64_t)blockIdx.x * FQ_EMIT_TILE;
    // (the whole workgroup leaves; nothing is written on overflow, nor after a fault the sizes kernel of any file so far found)
    if (lo64 >= total || total > out_capacity || ctr[fqd::FQE_FAULT])
        return;
    const uint32_t lo = (uint32_t)lo64;
    const uint32_t hi = (uint32_t)min((uint64_t)total, lo64 + FQ_EMIT_TILE);
    // the records that overlap [lo, hi): the first whose end lies behind lo, the last whose end reaches hi
    if (tid == 0)
        s_first = scan_bound(incl, m, lo, true);
    if (tid == 64)
        s_last = scan_bound(incl, m, hi, false);
    __syncthreads();
    const uint32_t k0 = s_first, k1 = min(s_last, m - 1);
    for (uint32_t k = k0 + wave; k <= k1; k += FE_WAVES) {
        const uint32_t end = incl[k], start = k ? incl[k - 1] : 0u;
        if (end == start)                                // (a candidate of a later chunk)
            continue;
        const unsigned long long id = kept[k];
        if (id < base || id - base >= n)                 // (cannot be, its size would be 0: the reads below stay in the table)
            continue;
        const uint32_t r = (uint32_t)(id - base);
        const uint32_t name_len = spans[fqd::FQS_NAME_LEN * rec_cap + r], seq_len = spans[fqd::FQS_SEQ_LEN * rec_cap + r];
        EmitRecord R;
        R.name_at = spans[fqd::FQS_ID_START * rec_cap + r];
        R.seq_at = spans[fqd::FQS_SEQ_START * rec_cap + r];
        R.qual_at = spans[fqd::FQS_QUAL_START * rec_cap + r];
        R.seq_q = 1u + name_len;
        R.plus_q = R.seq_q + 1u + seq_len;
        R.qual_q = R.plus_q + 3u;
        R.end_q = R.qual_q + seq_len;
        // the record's part of the tile, in tile positions; a lane per aligned word of it
        const uint32_t a = max(start, lo) - lo, b = min(end, hi) - lo;
        for (uint32_t w = (a & ~3u) + lane * 4u; w < b; w += 64u * 4u) {
            const uint32_t q = lo + w - start;           // output position of the word's byte 0 in the record (wraps below a)
            if (w >= a && w + 4u <= b) {
                const uint32_t v = R.byte_at(src, q) | (R.byte_at(src, q + 1u) << 8) | (R.byte_at(src, q + 2u) << 16) |
                                   (R.byte_at(src, q + 3u) << 24);
                *reinterpret_cast<uint32_t *>(s_tile + w) = v;
            } else {                                     // the word is shared with a neighbour record or cut by the tile
                for (uint32_t i = 0; i < 4u; i++)
                    if (w + i >= a && w + i < b)
                        s_tile[w + i] = (uint8_t)R.byte_at(src, q + i);
            }
        }
    }
    __syncthreads();
    // the tile goes out in 16-byte units; bytes only in the last, partial unit of the file's output
    const uint32_t span = hi - lo;
    for (uint32_t o = tid * 16u; o < span; o += FE_THREADS * 16u) {
        if (o + 16u <= span) {
            *reinterpret_cast<uint4 *>(out + lo64 + o) = *reinterpret_cast<const uint4 *>(s_tile + o);
        } else {
            for (uint32_t i = o; i < span; i++)
                out[lo64 + i] = s_tile[i];
        }
    }
}

}  // namespace

namespace fqd {

hipError_t launch_fastq_emit_init(uint32_t *ctr, hipStream_t st)
{
    fastq_emit_init_kernel<<<1, 64, 0, st>>>(ctr);
    return hipGetLastError();
}

hipError_t launch_fastq_emit_sizes(const uint32_t *spans, uint32_t rec_cap, uint32_t file, uint32_t n, uint64_t base,
                                   const uint64_t *kept, uint32_t m, uint32_t *sizes, uint32_t *ctr, hipStream_t st)
{
    fastq_emit_sizes_kernel<<<(m + FE_THREADS - 1) / FE_THREADS, FE_THREADS, 0, st>>>(
        spans, rec_cap, file, n, base, reinterpret_cast<const unsigned long long *>(kept), m, sizes, ctr);
    return hipGetLastError();
}

hipError_t launch_fastq_emit_copy(const uint8_t *bytes, const uint32_t *spans, uint32_t rec_cap, uint32_t file, uint32_t n,
                                  uint64_t base, const uint64_t *kept, uint32_t m, const uint32_t *incl, uint64_t bound,
                                  uint8_t *out, uint64_t out_capacity, uint32_t *ctr, hipStream_t st)
{
    const uint64_t tiles = (bound + FQ_EMIT_TILE - 1) / FQ_EMIT_TILE;
    fastq_emit_copy_kernel<<<(unsigned)tiles, FE_THREADS, 0, st>>>(bytes, spans, rec_cap, file, n, base,
                                                                   reinterpret_cast<const unsigned long long *>(kept), m,
                                                                   incl, out, out_capacity, ctr);
    return hipGetLastError();
}

}  // namespace fqd
