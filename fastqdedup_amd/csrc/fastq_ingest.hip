// fastq_ingest.hip -- raw (decompressed) FASTQ bytes to key bytes, key offsets and pass weights, all on
// the device. Replaces the host passes in front of the hot path: the reference's record loop
// (__init__.py:54-57), its mate check (:180-185), the --check-lengths slicing of sequence and quality
// (:160-167) and the quality gate as deduplicate_cluster uses it (:243-251).
//
// Five kernels, none of which waits on another workgroup:
//   1. line index    a count launch and a scatter launch over tiles of FQ_LINE_TILE bytes, the tile counts
//                    scanned in between (prims.hip): nl[] = byte position of every newline
//   2. records       one lane per record: the four lines' spans, format checks, id span, record end
//   3. mates         one lane per record: id of file 0 against the id of every other file
//   4. key lengths   one lane per record: sum over the files of len(range(*slice.indices(seq_len)))
//   5. gather        a workgroup per R records: each file's byte span staged in LDS, one wave per record
//                    copies the sliced sequence into an LDS output tile, one lane per record sums the
//                    sliced quality string's error rates; the tile goes out with 16-byte stores
//
// Bit-exactness of the mean: as quality.hip -- table values added one by one in string order into a
// double (here carried in a register across the files), one division, no FMA, no tree.
#include <algorithm>

#include "fqd_internal.h"

namespace {

using fqd::FastqFiles;
using fqd::FastqSlice;
using fqd::FQ_LINE_TILE;
using fqd::FQ_SPAN_FIELDS;

constexpr uint32_t FQ_THREADS = 256;
constexpr uint32_t FQ_IN_TILE = 32 * 1024;    // LDS input tile of the gather kernel: one file's bytes of R records
constexpr uint32_t FQ_OUT_TILE = 32 * 1024;   // ... and its output tile: the key bytes of those records
static_assert(FQ_LINE_TILE == FQ_THREADS * 16, "one 16-byte load per lane and tile");

// 16 bytes at offset o (a multiple of 16) of a buffer of n_bytes; bytes behind the end read as 0
__device__ __forceinline__ uint4 load16_tail(const uint8_t *__restrict__ bytes, uint64_t n_bytes, uint64_t o)
{
    if (o + 16 <= n_bytes)
        return *reinterpret_cast<const uint4 *>(bytes + o);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t j = 0; j < 16; j++)
        if (o + j < n_bytes)
            w[j >> 2] |= (uint32_t)bytes[o + j] << (8 * (j & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// bit k set <=> byte k of the word is '\n': exact zero-byte test on w ^ 0x0A0A0A0A, the four 0x80 marks
// gathered into a nibble by one multiply (the partial products land on distinct bits, so nothing carries)
__device__ __forceinline__ uint32_t newline_nibble(uint32_t w)
{
    const uint32_t x = w ^ 0x0A0A0A0Au;
    const uint32_t t = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
    return (((t >> 7) * 0x01020408u) >> 24) & 0xFu;
}

__device__ __forceinline__ uint32_t newline_mask16(const uint8_t *__restrict__ bytes, uint64_t n_bytes, uint64_t o)
{
    if (o >= n_bytes)
        return 0u;
    const uint4 v = load16_tail(bytes, n_bytes, o);
    return newline_nibble(v.x) | (newline_nibble(v.y) << 4) | (newline_nibble(v.z) << 8) | (newline_nibble(v.w) << 12);
}

// ---- 1. line index ---------------------------------------------------------------------------------
__global__ __launch_bounds__(FQ_THREADS) void fastq_line_count_kernel(const uint8_t *__restrict__ bytes, uint64_t n_bytes,
                                                                      uint32_t *__restrict__ tile_count,
                                                                      unsigned long long *__restrict__ info)
{
    __shared__ uint32_t s_wave[FQ_THREADS / 64];
    const uint32_t tid = threadIdx.x;
    if (blockIdx.x == 0 && tid == 0) {        // the words the record kernel reduces into
        info[fqd::FQI_ERROR] = ~0ull;
        info[fqd::FQI_MAX_RECORD] = 0ull;
    }
    uint32_t c = __popc(newline_mask16(bytes, n_bytes, (uint64_t)blockIdx.x * FQ_LINE_TILE + tid * 16u));
    for (int o = 32; o; o >>= 1)
        c += __shfl_xor(c, o);
    if ((tid & 63u) == 0)
        s_wave[tid >> 6] = c;
    __syncthreads();
    if (tid == 0)
        tile_count[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

__global__ __launch_bounds__(FQ_THREADS) void fastq_line_scatter_kernel(const uint8_t *__restrict__ bytes, uint64_t n_bytes,
                                                                        const uint32_t *__restrict__ tile_incl,
                                                                        uint32_t *__restrict__ nl, uint32_t nl_cap)
{
    __shared__ uint32_t s_wave[FQ_THREADS / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t o = (uint64_t)blockIdx.x * FQ_LINE_TILE + tid * 16u;
    uint32_t mask = newline_mask16(bytes, n_bytes, o);
    const uint32_t mine = __popc(mask);
    uint32_t incl = mine;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d);
        if ((int)lane >= d)
            incl += up;
    }
    if (lane == 63)
        s_wave[wave] = incl;
    __syncthreads();
    uint32_t at = (blockIdx.x ? tile_incl[blockIdx.x - 1] : 0u) + incl - mine;
    for (uint32_t w = 0; w < wave; w++)
        at += s_wave[w];
    while (mask) {
        const uint32_t b = __ffs(mask) - 1;
        if (at < nl_cap)
            nl[at] = (uint32_t)o + b;
        at++;
        mask &= mask - 1;
    }
}

// ---- 2. records --------------------------------------------------------------------------------------
__global__ __launch_bounds__(FQ_THREADS) void fastq_records_kernel(const uint8_t *__restrict__ bytes, uint64_t n_bytes,
                                                                   const uint32_t *__restrict__ nl,
                                                                   const uint32_t *__restrict__ tile_incl, uint32_t n_tiles,
                                                                   uint32_t nl_cap, int final, uint32_t *__restrict__ spans,
                                                                   uint32_t rec_cap, unsigned long long *__restrict__ info)
{
    __shared__ uint32_t s_max;
    const uint32_t tid = threadIdx.x;
    const uint64_t gid = (uint64_t)blockIdx.x * FQ_THREADS + tid;
    const uint32_t n_nl = tile_incl[n_tiles - 1];
    if (gid == 0)
        info[fqd::FQI_NEWLINES] = n_nl;
    if (n_nl > nl_cap)          // nl[] is cut short: the host makes room and launches the scatter and this kernel again
        return;
    auto line_start = [&](uint32_t i) -> uint32_t { return i ? nl[i - 1] + 1u : 0u; };
    auto line_end = [&](uint32_t i) -> uint32_t { return i < n_nl ? nl[i] : (uint32_t)n_bytes; };
    // lines of this block: with `final` a last line without a newline counts, trailing blank lines do not
    uint32_t n_lines = n_nl;
    if (final) {
        if (n_bytes && (n_nl == 0 || nl[n_nl - 1] != (uint32_t)(n_bytes - 1)))
            n_lines++;
        while (n_lines && (n_lines & 3u) && line_start(n_lines - 1) >= line_end(n_lines - 1))
            n_lines--;
    }
    const uint32_t n_rec = min(n_lines >> 2, rec_cap);
    if (gid == 0) {
        info[fqd::FQI_RECORDS] = n_rec;
        if (final && (n_lines & 3u))
            atomicMin(&info[fqd::FQI_ERROR], ((unsigned long long)n_lines << 2) | fqd::FQ_ERR_PREMATURE);
    }
    if (tid == 0)
        s_max = 0;
    __syncthreads();
    for (uint64_t r64 = gid; r64 < n_rec; r64 += (uint64_t)gridDim.x * FQ_THREADS) {
        const uint32_t r = (uint32_t)r64;
        uint32_t s[4], e[4], ce[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            s[k] = line_start(4 * r + k);
            e[k] = line_end(4 * r + k);
            ce[k] = (e[k] > s[k] && bytes[e[k] - 1] == '\r') ? e[k] - 1 : e[k];
        }
        const unsigned long long line0 = 4ull * r;
        if (ce[0] == s[0] || bytes[s[0]] != '@')
            atomicMin(&info[fqd::FQI_ERROR], (line0 << 2) | fqd::FQ_ERR_AT);
        else if (!(ce[2] > s[2] && bytes[s[2]] == '+'))
            atomicMin(&info[fqd::FQI_ERROR], ((line0 + 2) << 2) | fqd::FQ_ERR_PLUS);
        else if (ce[1] - s[1] != ce[3] - s[3])
            atomicMin(&info[fqd::FQI_ERROR], ((line0 + 3) << 2) | fqd::FQ_ERR_LENGTHS);
        // the id: the name up to its first blank or tab; bit 0 of the id word: it ends in 1, 2 or 3
        const uint32_t name_start = min(s[0] + 1u, ce[0]);
        uint32_t id_end = name_start;
        while (id_end < ce[0] && bytes[id_end] != ' ' && bytes[id_end] != '\t')
            id_end++;
        const uint32_t id_len = id_end - name_start;
        const uint8_t last = id_len ? bytes[id_end - 1] : 0;
        const uint32_t rec_end = (uint32_t)min((uint64_t)e[3] + 1u, n_bytes);
        spans[fqd::FQS_SEQ_START * rec_cap + r] = s[1];
        spans[fqd::FQS_SEQ_LEN * rec_cap + r] = ce[1] - s[1];
        spans[fqd::FQS_QUAL_START * rec_cap + r] = s[3];
        spans[fqd::FQS_ID_START * rec_cap + r] = name_start;
        spans[fqd::FQS_ID_WORD * rec_cap + r] = (id_len << 1) | ((last >= '1' && last <= '3') ? 1u : 0u);
        spans[fqd::FQS_NAME_LEN * rec_cap + r] = ce[0] - name_start;
        spans[fqd::FQS_REC_END * rec_cap + r] = rec_end;
        atomicMax(&s_max, rec_end - s[0]);
    }
    __syncthreads();
    if (tid == 0 && s_max)
        atomicMax(&info[fqd::FQI_MAX_RECORD], (unsigned long long)s_max);
}

// ---- 3. mates ------------------------------------------------------------------------------------------
// dnaio's records_are_mates as fastq.check_mates states it: equal id lengths; when both ids end in 1/2/3 that
// last character is not compared.
__global__ __launch_bounds__(FQ_THREADS) void fastq_mates_kernel(FastqFiles F, uint32_t n, uint32_t *__restrict__ ctr)
{
    const uint64_t r = (uint64_t)blockIdx.x * FQ_THREADS + threadIdx.x;
    if (r >= n)
        return;
    const uint32_t s0 = F.spans[0][fqd::FQS_ID_START * F.rec_cap[0] + r];
    const uint32_t w0 = F.spans[0][fqd::FQS_ID_WORD * F.rec_cap[0] + r];
    bool ok = true;
    for (uint32_t f = 1; f < F.n_files && ok; f++) {
        const uint32_t s = F.spans[f][fqd::FQS_ID_START * F.rec_cap[f] + r];
        const uint32_t w = F.spans[f][fqd::FQS_ID_WORD * F.rec_cap[f] + r];
        ok = (w >> 1) == (w0 >> 1);
        const uint32_t cmp = (w0 >> 1) - ((w0 & w & 1u) ? 1u : 0u);
        for (uint32_t i = 0; ok && i < cmp; i++)
            ok = F.bytes[0][s0 + i] == F.bytes[f][s + i];
    }
    if (!ok)
        atomicMin(&ctr[fqd::FQC_MATE], (uint32_t)r);
}

// ---- 4. key lengths --------------------------------------------------------------------------------------
// slice.indices(len) for any start/stop/step (CPython's PySlice_AdjustIndices; None arrives as the extreme
// values it uses): the first index taken, and how many
__device__ __forceinline__ uint32_t slice_adjust(uint32_t len, const FastqSlice &sl, long long *first)
{
    const long long L = len, step = sl.step;
    long long a = sl.start, b = sl.stop;
    if (a < 0) {
        a += L;
        if (a < 0)
            a = step < 0 ? -1 : 0;
    } else if (a >= L) {
        a = step < 0 ? L - 1 : L;
    }
    if (b < 0) {
        b += L;
        if (b < 0)
            b = step < 0 ? -1 : 0;
    } else if (b >= L) {
        b = step < 0 ? L - 1 : L;
    }
    *first = a;
    if (step < 0)
        return b < a ? (uint32_t)((a - b - 1) / (-step) + 1) : 0u;
    return a < b ? (uint32_t)((b - a - 1) / step + 1) : 0u;
}

__global__ __launch_bounds__(FQ_THREADS) void fastq_key_lens_kernel(FastqFiles F, uint32_t n, uint32_t *__restrict__ lens,
                                                                    uint32_t *__restrict__ ctr)
{
    __shared__ uint32_t s_min, s_max;
    const uint64_t r = (uint64_t)blockIdx.x * FQ_THREADS + threadIdx.x;
    if (threadIdx.x == 0) {
        s_min = 0xFFFFFFFFu;
        s_max = 0u;
    }
    __syncthreads();
    if (r < n) {
        uint32_t total = 0;
        for (uint32_t f = 0; f < F.n_files; f++) {
            long long first;
            total += slice_adjust(F.spans[f][fqd::FQS_SEQ_LEN * F.rec_cap[f] + r], F.slice[f], &first);
        }
        lens[r] = total;
        atomicMin(&s_min, total);
        atomicMax(&s_max, total);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMin(&ctr[fqd::FQC_MIN_LEN], s_min);
        atomicMax(&ctr[fqd::FQC_MAX_LEN], s_max);
    }
}

__global__ void fastq_counters_init_kernel(uint32_t *__restrict__ ctr)
{
    if (threadIdx.x < fqd::FQC_WORDS)
        ctr[threadIdx.x] = (threadIdx.x == fqd::FQC_MIN_LEN || threadIdx.x == fqd::FQC_MATE) ? 0xFFFFFFFFu : 0u;
}

// ---- 5. gather and quality gate --------------------------------------------------------------------------
__global__ __launch_bounds__(FQ_THREADS) void fastq_gather_kernel(FastqFiles F, uint32_t n, uint32_t R,
                                                                  const uint32_t *__restrict__ incl,
                                                                  const double *__restrict__ table, uint32_t phred_offset,
                                                                  uint32_t max_score, double threshold, int do_quality,
                                                                  uint8_t *__restrict__ keys_out, uint64_t keys_capacity,
                                                                  uint64_t key_base, unsigned long long *__restrict__ offsets_out,
                                                                  uint32_t *__restrict__ weights_out,
                                                                  double *__restrict__ means_out, uint32_t *__restrict__ ctr)
{
    __shared__ double s_table[128];
    __shared__ __attribute__((aligned(16))) uint8_t s_in[FQ_IN_TILE];
    __shared__ __attribute__((aligned(16))) uint8_t s_out[FQ_OUT_TILE];
    __shared__ uint32_t s_pos[FQ_THREADS];     // where record k's next key byte goes, relative to a_out
    __shared__ uint32_t s_discarded;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t r0 = blockIdx.x * R;
    const uint32_t nr = min(R, n - r0);
    const uint32_t kb0 = r0 ? incl[r0 - 1] : 0u, kb1 = incl[r0 + nr - 1];
    const uint64_t g0 = key_base + kb0, g1 = key_base + kb1;       // this workgroup's bytes of the key buffer
    if (r0 + nr == n && tid == 0) {
        ctr[fqd::FQC_KEY_BYTES] = kb1;
        for (uint32_t f = 0; f < F.n_files; f++)
            ctr[fqd::FQC_CONSUMED + f] = F.spans[f][fqd::FQS_REC_END * F.rec_cap[f] + n - 1];
    }
    if (g1 > keys_capacity) {                                       // (the whole workgroup leaves)
        if (tid == 0)
            atomicOr(&ctr[fqd::FQC_OVERFLOW], 1u);
        return;
    }
    const uint64_t a_out = g0 & ~15ull;
    const uint32_t out_span = (uint32_t)(g1 - a_out);
    const bool staged_out = out_span <= FQ_OUT_TILE;
    uint8_t *const out_base = staged_out ? s_out : keys_out + a_out;
    if (tid < 128)
        s_table[tid] = table[tid];
    if (tid == 0)
        s_discarded = 0;
    if (tid < nr) {
        const uint32_t before = (r0 + tid) ? incl[r0 + tid - 1] : 0u;
        s_pos[tid] = (before - kb0) + (uint32_t)(g0 - a_out);
        offsets_out[r0 + tid + 1] = key_base + incl[r0 + tid];
        if (r0 + tid == 0)
            offsets_out[0] = key_base;
    }
    double total = 0.0;           // the record's error-rate sum, carried across the files
    uint32_t total_len = 0;
    bool bad = false;
    for (uint32_t f = 0; f < F.n_files; f++) {
        const uint32_t *__restrict__ sp = F.spans[f];
        const uint32_t cap = F.rec_cap[f];
        const uint8_t *__restrict__ fbytes = F.bytes[f];
        const uint32_t b0 = r0 ? sp[fqd::FQS_REC_END * cap + r0 - 1] : 0u;
        const uint32_t b1 = sp[fqd::FQS_REC_END * cap + r0 + nr - 1];
        const uint32_t a0 = b0 & ~15u;
        const uint32_t span = b1 - a0;
        const bool staged = span <= FQ_IN_TILE;       // else: a record larger than the tile, read from global memory
        __syncthreads();                              // the tile of the file before is done with; s_pos is up to date
        if (staged)
            for (uint32_t o = tid * 16; o < span; o += FQ_THREADS * 16)
                *reinterpret_cast<uint4 *>(s_in + o) = load16_tail(fbytes, F.n_bytes[f], (uint64_t)a0 + o);
        __syncthreads();
        const uint8_t *const src = staged ? s_in : fbytes + a0;      // src[p - a0] = byte p of the file's block
        for (uint32_t k = wave; k < nr; k += FQ_THREADS / 64) {      // one wave per record: the sliced sequence
            long long first;
            const uint32_t count = slice_adjust(sp[fqd::FQS_SEQ_LEN * cap + r0 + k], F.slice[f], &first);
            if (!count)
                continue;
            const uint8_t *const s = src + (sp[fqd::FQS_SEQ_START * cap + r0 + k] - a0) + first;
            uint8_t *const d = out_base + s_pos[k];
            for (uint32_t i = lane; i < count; i += 64)
                d[i] = s[(long long)i * F.slice[f].step];
        }
        uint32_t mine = 0;
        if (tid < nr) {                                               // one lane per record: the sliced quality string
            long long first;
            mine = slice_adjust(sp[fqd::FQS_SEQ_LEN * cap + r0 + tid], F.slice[f], &first);
            if (do_quality && mine && !bad) {
                const uint8_t *const q = src + (sp[fqd::FQS_QUAL_START * cap + r0 + tid] - a0) + first;
                for (uint32_t i = 0; i < mine; i++) {
                    const uint8_t ch = q[(long long)i * F.slice[f].step];
                    const uint32_t score = (uint32_t)ch - phred_offset;   // wraps below the offset
                    if (score > max_score || ch > 127) {
                        bad = true;
                        break;
                    }
                    total = __dadd_rn(total, s_table[score]);
                }
            }
            total_len += mine;
        }
        __syncthreads();
        if (tid < nr)
            s_pos[tid] += mine;
    }
    if (tid < nr && do_quality) {
        const double mean = __ddiv_rn(total, (double)total_len);      // 0/0 = NaN for an empty string: kept
        if (means_out)
            means_out[r0 + tid] = mean;
        if (weights_out) {
            const uint32_t pass = (mean > threshold) ? 0u : 1u;
            weights_out[r0 + tid] = pass;
            if (!pass)
                atomicAdd(&s_discarded, 1u);
        }
        if (bad)
            atomicOr(&ctr[fqd::FQC_BAD], 1u);
    }
    // the output tile: 16-byte stores where the whole unit is this workgroup's, byte stores at the two ends
    if (staged_out) {
        for (uint32_t o = tid * 16; o < out_span; o += FQ_THREADS * 16) {
            const uint64_t p = a_out + o;
            if (p >= g0 && p + 16 <= g1) {
                *reinterpret_cast<uint4 *>(keys_out + p) = *reinterpret_cast<const uint4 *>(s_out + o);
            } else {
                for (uint32_t j = 0; j < 16; j++)
                    if (p + j >= g0 && p + j < g1)
                        keys_out[p + j] = s_out[o + j];
            }
        }
    }
    __syncthreads();
    if (tid == 0 && s_discarded)
        atomicAdd(&ctr[fqd::FQC_DISCARDED], s_discarded);
}

}  // namespace

namespace fqd {

uint32_t fastq_line_tiles(uint64_t n_bytes) { return (uint32_t)((n_bytes + FQ_LINE_TILE - 1) / FQ_LINE_TILE); }

hipError_t launch_fastq_line_count(const uint8_t *bytes, uint64_t n_bytes, uint32_t *tile_count, unsigned long long *info,
                                   hipStream_t st)
{
    fastq_line_count_kernel<<<fastq_line_tiles(n_bytes), FQ_THREADS, 0, st>>>(bytes, n_bytes, tile_count, info);
    return hipGetLastError();
}

hipError_t launch_fastq_line_scatter(const uint8_t *bytes, uint64_t n_bytes, const uint32_t *tile_incl, uint32_t *nl,
                                     uint32_t nl_cap, hipStream_t st)
{
    fastq_line_scatter_kernel<<<fastq_line_tiles(n_bytes), FQ_THREADS, 0, st>>>(bytes, n_bytes, tile_incl, nl, nl_cap);
    return hipGetLastError();
}

hipError_t launch_fastq_records(const uint8_t *bytes, uint64_t n_bytes, const uint32_t *nl, const uint32_t *tile_incl,
                                uint32_t nl_cap, int final, uint32_t *spans, uint32_t rec_cap, unsigned long long *info,
                                hipStream_t st)
{
    // a record with no fault before it has 6 bytes or more; the lanes stride over whatever the block holds
    const uint64_t blocks = std::min<uint64_t>((n_bytes / 6 + FQ_THREADS) / FQ_THREADS, 4096);
    fastq_records_kernel<<<(unsigned)blocks, FQ_THREADS, 0, st>>>(bytes, n_bytes, nl, tile_incl, fastq_line_tiles(n_bytes),
                                                                   nl_cap, final, spans, rec_cap, info);
    return hipGetLastError();
}

hipError_t launch_fastq_counters_init(uint32_t *ctr, hipStream_t st)
{
    fastq_counters_init_kernel<<<1, 64, 0, st>>>(ctr);
    return hipGetLastError();
}

hipError_t launch_fastq_mates(const FastqFiles &files, uint32_t n, uint32_t *ctr, hipStream_t st)
{
    fastq_mates_kernel<<<(n + FQ_THREADS - 1) / FQ_THREADS, FQ_THREADS, 0, st>>>(files, n, ctr);
    return hipGetLastError();
}

hipError_t launch_fastq_key_lens(const FastqFiles &files, uint32_t n, uint32_t *lens, uint32_t *ctr, hipStream_t st)
{
    fastq_key_lens_kernel<<<(n + FQ_THREADS - 1) / FQ_THREADS, FQ_THREADS, 0, st>>>(files, n, lens, ctr);
    return hipGetLastError();
}

uint32_t fastq_gather_records(const uint32_t *max_record, uint32_t n_files)
{
    uint64_t largest = 0, key_bytes = 0;      // (a record's key bytes are at most half of it: sequence and quality are equally long)
    for (uint32_t f = 0; f < n_files; f++) {
        largest = std::max<uint64_t>(largest, max_record[f]);
        key_bytes += max_record[f] / 2;
    }
    uint32_t R = FQ_THREADS;
    while (R > 1 && ((uint64_t)R * largest + 16 > FQ_IN_TILE || (uint64_t)R * key_bytes + 16 > FQ_OUT_TILE))
        R >>= 1;
    return R;
}

hipError_t launch_fastq_gather(const FastqFiles &files, uint32_t n, uint32_t R, const uint32_t *incl, const double *table,
                               uint32_t phred_offset, uint32_t max_score, double threshold, int do_quality,
                               uint8_t *keys_out, uint64_t keys_capacity, uint64_t key_base, uint64_t *offsets_out,
                               uint32_t *weights_out, double *means_out, uint32_t *ctr, hipStream_t st)
{
    fastq_gather_kernel<<<(n + R - 1) / R, FQ_THREADS, 0, st>>>(files, n, R, incl, table, phred_offset, max_score, threshold,
                                                                do_quality, keys_out, keys_capacity, key_base,
                                                                reinterpret_cast<unsigned long long *>(offsets_out),
                                                                weights_out, means_out, ctr);
    return hipGetLastError();
}

}  // namespace fqd
