// api_fastq.hip -- the FASTQ ingest behind the C ABI (include/fqdedup_hip.h, fqd_fastq_*): one block of raw
// bytes per input file is indexed on the device (fastq_ingest.hip kernels 1-2), then the first n records of
// every block are turned into key bytes, offsets and weights in the caller's device buffers (kernels 3-5).
// One read-back per index call and one per append. Pass 2 (fqd_fastq_emit*) indexes the blocks the same way and turns
// the kept records among the first n into every file's output bytes (fastq_emit.hip): one read-back per emit.
#include "api_ctx.h"

namespace {

// a few words from the device in one copy, through the pinned buffer when they fit
int read_words(fqd_ctx *c, void *dst, const void *dev, size_t bytes)
{
    void *via = (c->h_pin && bytes <= 192) ? c->h_pin : dst;
    HIP_TRY(c, hipMemcpyAsync(via, dev, bytes, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(c, stream_wait(c->st));
    if (via != dst)
        memcpy(dst, via, bytes);
    return FQD_OK;
}

}  // namespace

void fqd_api_fastq_release(fqd_ctx *c)
{
    for (FastqSlot &s : c->fq)
        for (DevBuf *b : {&s.bytes, &s.nl, &s.tiles, &s.spans, &s.info})
            b->release();
    for (DevBuf *b : {&c->fq_lens, &c->fq_incl, &c->fq_ctr, &c->fq_table})
        b->release();
}

extern "C" {

int fqd_fastq_begin(fqd_ctx *c, uint32_t n_files)
{
    FQD_TRY(bind(c));
    if (!n_files || n_files > FQD_FASTQ_MAX_FILES)
        return fail(c, FQD_E_VALUE, "fqd_fastq_begin: between 1 and FQD_FASTQ_MAX_FILES files");
    c->fq_files = n_files;
    for (FastqSlot &s : c->fq) {
        s.indexed = s.faulty = false;
        s.n_rec = s.n_bytes = 0;
        s.d = nullptr;
    }
    c->fq_records = c->fq_key_bytes = c->fq_discarded = c->fq_chunks = 0;
    return FQD_OK;
}

int fqd_fastq_index(fqd_ctx *c, uint32_t file, const uint8_t *bytes, uint64_t n_bytes, int mem, int final,
                    uint64_t first_line, fqd_fastq_index_info *info)
{
    FQD_TRY(bind(c));
    if (file >= c->fq_files)
        return fail(c, FQD_E_VALUE, "fqd_fastq_index: no such file (fqd_fastq_begin sets their number)");
    if (!info || (n_bytes && !bytes))
        return fail(c, FQD_E_VALUE, "fqd_fastq_index: null argument");
    if (n_bytes >= 0xFFFFFFF0ull)
        return fail(c, FQD_E_VALUE, "fqd_fastq_index: a block must be shorter than 4 GiB");
    if (mem == FQD_DEVICE && ((uintptr_t)bytes & 15u))
        return fail(c, FQD_E_VALUE, "device buffer must be 16-byte aligned");
    FastqSlot &s = c->fq[file];
    s.indexed = s.faulty = false;
    s.n_bytes = n_bytes;
    s.n_rec = 0;
    s.max_rec = 0;
    *info = fqd_fastq_index_info{0, 0, 0, FQD_FASTQ_OK};
    if (!n_bytes) {
        s.d = nullptr;
        s.indexed = true;
        return FQD_OK;
    }
    FQD_TRY(to_device(c, bytes, (size_t)n_bytes, mem, s.bytes, &s.d));
    const uint32_t n_tiles = fqd::fastq_line_tiles(n_bytes);
    const size_t tile_words = ((size_t)n_tiles + 3) & ~(size_t)3;       // (both halves 16-byte aligned for the scan)
    HIP_TRY(c, s.tiles.reserve(2 * tile_words * 4));
    HIP_TRY(c, s.info.reserve(fqd::FQI_WORDS * 8));
    uint32_t *tile_count = s.tiles.as<uint32_t>(), *tile_incl = tile_count + tile_words;
    unsigned long long *d_info = s.info.as<unsigned long long>();
    KTIME(c, FQD_K_FASTQ_LINE_COUNT, fqd::launch_fastq_line_count(s.d, n_bytes, tile_count, d_info, c->st));
    FQD_TRY(scan_u32(c, tile_count, tile_incl, n_tiles));
    // room for the newline positions: a line of 8 bytes on average, or what the last block of this file needed; a
    // block with more lines says so in its read-back and gets its scatter and record launches once more
    uint64_t want_nl = std::max<uint64_t>(n_bytes / 8 + 1024, s.nl_cap);
    unsigned long long words[fqd::FQI_WORDS];
    for (int attempt = 0;; attempt++) {
        want_nl = std::min<uint64_t>(want_nl, n_bytes);
        HIP_TRY(c, s.nl.reserve((size_t)want_nl * 4 + 16));
        s.nl_cap = (uint32_t)want_nl;
        s.rec_cap = s.nl_cap / 4 + 1;
        HIP_TRY(c, s.spans.reserve((size_t)s.rec_cap * fqd::FQ_SPAN_FIELDS * 4 + 16));
        KTIME(c, FQD_K_FASTQ_LINE_SCATTER,
              fqd::launch_fastq_line_scatter(s.d, n_bytes, tile_incl, s.nl.as<uint32_t>(), s.nl_cap, c->st));
        KTIME(c, FQD_K_FASTQ_RECORDS,
              fqd::launch_fastq_records(s.d, n_bytes, s.nl.as<uint32_t>(), tile_incl, s.nl_cap, final,
                                        s.spans.as<uint32_t>(), s.rec_cap, d_info, c->st));
        FQD_TRY(read_words(c, words, d_info, sizeof words));
        if (words[fqd::FQI_NEWLINES] <= s.nl_cap)
            break;
        if (attempt)
            return fail(c, FQD_E_RUNTIME, "fqd_fastq_index: the line index did not fit twice");
        want_nl = words[fqd::FQI_NEWLINES];
    }
    if (c->kused > fqd_ctx::KPOOL - 40)
        ktime_collect(c);
    s.n_rec = words[fqd::FQI_RECORDS];
    s.max_rec = (uint32_t)words[fqd::FQI_MAX_RECORD];
    s.indexed = true;
    info->n_records = s.n_rec;
    info->max_record_bytes = s.max_rec;
    if (words[fqd::FQI_ERROR] != ~0ull) {
        static const int kinds[4] = {FQD_FASTQ_NO_AT, FQD_FASTQ_NO_PLUS, FQD_FASTQ_LENGTHS, FQD_FASTQ_PREMATURE};
        info->error_kind = kinds[words[fqd::FQI_ERROR] & 3u];
        info->error_line = first_line + (words[fqd::FQI_ERROR] >> 2);
        s.faulty = true;
    }
    return FQD_OK;
}

int fqd_fastq_append(fqd_ctx *c, uint64_t n, const fqd_fastq_slice *slices, double threshold, const double *table128,
                     uint32_t phred_offset, uint8_t *keys_out, uint64_t keys_capacity, uint64_t key_base,
                     uint64_t *offsets_out, uint32_t *weights_out, double *means_out, fqd_fastq_append_info *info)
{
    FQD_TRY(bind(c));
    if (!info || !offsets_out || (!keys_out && keys_capacity))
        return fail(c, FQD_E_VALUE, "fqd_fastq_append: null argument");
    if ((uintptr_t)keys_out & 15u)
        return fail(c, FQD_E_VALUE, "device buffer must be 16-byte aligned");
    if (phred_offset > 126)
        return fail(c, FQD_E_VALUE, "phred_offset out of range");
    if (!c->fq_files)
        return fail(c, FQD_E_STATE, "fqd_fastq_append before fqd_fastq_begin");
    memset(info, 0, sizeof *info);
    info->first_non_mate = ~0ull;
    fqd::FastqFiles F{};
    F.n_files = c->fq_files;
    uint32_t max_rec[FQD_FASTQ_MAX_FILES];
    uint64_t block_bytes = 0;
    for (uint32_t f = 0; f < c->fq_files; f++) {
        const FastqSlot &s = c->fq[f];
        if (!s.indexed || s.faulty)
            return fail(c, FQD_E_STATE, "fqd_fastq_append: every file needs a block indexed without a format error");
        if (n > s.n_rec)
            return fail(c, FQD_E_VALUE, "fqd_fastq_append: more records than a block holds");
        F.bytes[f] = s.d;
        F.spans[f] = s.spans.as<uint32_t>();
        F.n_bytes[f] = s.n_bytes;
        F.rec_cap[f] = s.rec_cap;
        F.slice[f] = slices ? fqd::FastqSlice{slices[f].start, slices[f].stop, slices[f].step}
                            : fqd::FastqSlice{0, INT64_MAX, 1};
        if (!F.slice[f].step)
            return fail(c, FQD_E_VALUE, "slice step cannot be zero");
        // (a step beyond any sequence length takes the same elements as 2^32, and its negation cannot overflow)
        F.slice[f].step = std::max<long long>(-(1ll << 32), std::min<long long>(1ll << 32, F.slice[f].step));
        max_rec[f] = s.max_rec;
        block_bytes += s.n_bytes;
    }
    if (block_bytes >= 0xFFFFFFF0ull)
        return fail(c, FQD_E_VALUE, "fqd_fastq_append: the blocks of all files together must be shorter than 4 GiB");
    if (!n) {
        HIP_TRY(c, hipMemcpyAsync(offsets_out, &key_base, 8, hipMemcpyHostToDevice, c->st));
        HIP_TRY(c, stream_wait(c->st));
        return FQD_OK;
    }
    const bool gate = threshold < 1.0;
    const int do_quality = (gate && weights_out) || means_out;
    if (gate && !weights_out)
        return fail(c, FQD_E_VALUE, "fqd_fastq_append: a threshold below 1.0 needs weights_out");
    if (do_quality) {
        double table[128];
        for (int i = 0; i < 128; i++)
            table[i] = table128 ? table128[i] : std::pow(10.0, -((double)i / 10.0));   // score_to_error_rate.py
        if (!c->fq_table_valid || memcmp(table, c->fq_table_host, sizeof table)) {
            HIP_TRY(c, c->fq_table.reserve(sizeof table));
            HIP_TRY(c, hipMemcpyAsync(c->fq_table.p, table, sizeof table, hipMemcpyHostToDevice, c->st));
            HIP_TRY(c, stream_wait(c->st));      // (the source is on this stack)
            memcpy(c->fq_table_host, table, sizeof table);
            c->fq_table_valid = true;
        }
    } else {
        HIP_TRY(c, c->fq_table.reserve(sizeof(double) * 128));
    }
    HIP_TRY(c, c->fq_ctr.reserve(fqd::FQC_WORDS * 4));
    HIP_TRY(c, c->fq_lens.reserve((size_t)n * 4 + 16));
    HIP_TRY(c, c->fq_incl.reserve((size_t)n * 4 + 16));
    uint32_t *ctr = c->fq_ctr.as<uint32_t>();
    HIP_TRY(c, fqd::launch_fastq_counters_init(ctr, c->st));
    uint32_t words[fqd::FQC_WORDS];
    if (c->fq_files > 1)
        KTIME(c, FQD_K_FASTQ_MATES, fqd::launch_fastq_mates(F, (uint32_t)n, ctr, c->st));
    KTIME(c, FQD_K_FASTQ_KEY_LENS, fqd::launch_fastq_key_lens(F, (uint32_t)n, c->fq_lens.as<uint32_t>(), ctr, c->st));
    FQD_TRY(scan_u32(c, c->fq_lens.as<uint32_t>(), c->fq_incl.as<uint32_t>(), n));
    const uint32_t R = fqd::fastq_gather_records(max_rec, c->fq_files);
    KTIME(c, FQD_K_FASTQ_GATHER,
          fqd::launch_fastq_gather(F, (uint32_t)n, R, c->fq_incl.as<uint32_t>(), c->fq_table.as<double>(), phred_offset,
                                   126u - phred_offset, threshold, do_quality, keys_out, keys_capacity, key_base,
                                   offsets_out, gate ? weights_out : nullptr, means_out, ctr, c->st));
    FQD_TRY(read_words(c, words, ctr, sizeof words));
    if (c->kused > fqd_ctx::KPOOL - 40)
        ktime_collect(c);
    if (words[fqd::FQC_MATE] != 0xFFFFFFFFu) {
        // files out of step (checked first, as the reference does): the names of the record for the message
        const uint32_t r = words[fqd::FQC_MATE];
        info->first_non_mate = r;
        for (uint32_t f = 0; f < c->fq_files; f++) {
            uint32_t v[2];
            HIP_TRY(c, hipMemcpyAsync(&v[0], F.spans[f] + (size_t)fqd::FQS_ID_START * F.rec_cap[f] + r, 4,
                                      hipMemcpyDeviceToHost, c->st));
            HIP_TRY(c, hipMemcpyAsync(&v[1], F.spans[f] + (size_t)fqd::FQS_NAME_LEN * F.rec_cap[f] + r, 4,
                                      hipMemcpyDeviceToHost, c->st));
            HIP_TRY(c, stream_wait(c->st));
            info->name_start[f] = v[0];
            info->name_len[f] = v[1];
        }
        return FQD_OK;
    }
    if (words[fqd::FQC_OVERFLOW])
        return fail(c, FQD_E_VALUE, "fqd_fastq_append: keys_capacity is too small for the keys of these records");
    if (words[fqd::FQC_BAD])
        return fail(c, FQD_E_VALUE, "a phred string holds a character outside the valid phred range");
    info->key_bytes = words[fqd::FQC_KEY_BYTES];
    info->n_discarded = words[fqd::FQC_DISCARDED];
    info->fixed_len = words[fqd::FQC_MIN_LEN] == words[fqd::FQC_MAX_LEN] ? words[fqd::FQC_MIN_LEN] : 0u;
    for (uint32_t f = 0; f < c->fq_files; f++)
        info->consumed[f] = words[fqd::FQC_CONSUMED + f];
    c->fq_chunks++;
    c->fq_records += n;
    c->fq_key_bytes += info->key_bytes;
    c->fq_discarded += info->n_discarded;
    return FQD_OK;
}

int fqd_fastq_emit_begin(fqd_ctx *c, uint32_t n_files)
{
    FQD_TRY(bind(c));
    if (!n_files || n_files > FQD_FASTQ_MAX_FILES)
        return fail(c, FQD_E_VALUE, "fqd_fastq_emit_begin: between 1 and FQD_FASTQ_MAX_FILES files");
    c->fq_files = n_files;
    for (FastqSlot &s : c->fq) {
        s.indexed = s.faulty = false;
        s.n_rec = s.n_bytes = 0;
        s.d = nullptr;
    }
    return FQD_OK;          // (the counters of fqd_fastq_stats belong to pass 1)
}

int fqd_fastq_emit(fqd_ctx *c, uint64_t n, uint64_t base_id, const uint64_t *kept_ids, uint64_t n_kept, uint64_t kept_from,
                   uint8_t *const *out, const uint64_t *out_capacity, fqd_fastq_emit_info *info)
{
    FQD_TRY(bind(c));
    if (!info || !out || !out_capacity || (n_kept && !kept_ids))
        return fail(c, FQD_E_VALUE, "fqd_fastq_emit: null argument");
    if (kept_from > n_kept)
        return fail(c, FQD_E_VALUE, "fqd_fastq_emit: kept_from lies behind the kept ids");
    if (!c->fq_files)
        return fail(c, FQD_E_STATE, "fqd_fastq_emit before fqd_fastq_emit_begin");
    memset(info, 0, sizeof *info);
    uint64_t block_bytes = 0;
    for (uint32_t f = 0; f < c->fq_files; f++) {
        const FastqSlot &s = c->fq[f];
        if (!s.indexed || s.faulty)
            return fail(c, FQD_E_STATE, "fqd_fastq_emit: every file needs a block indexed without a format error");
        if (n > s.n_rec)
            return fail(c, FQD_E_VALUE, "fqd_fastq_emit: more records than a block holds");
        if (((uintptr_t)out[f] & 15u) || (!out[f] && out_capacity[f]))
            return fail(c, FQD_E_VALUE, "device buffer must be 16-byte aligned");
        block_bytes += s.n_bytes;
    }
    if (block_bytes >= 0xFFFFFFF0ull)
        return fail(c, FQD_E_VALUE, "fqd_fastq_emit: the blocks of all files together must be shorter than 4 GiB");
    if (!n)
        return FQD_OK;
    const uint32_t m = (uint32_t)std::min<uint64_t>(n, n_kept - kept_from);
    if (!m) {
        // nothing left to write: only where the chunk ends in every block
        for (uint32_t f = 0; f < c->fq_files; f++) {
            const FastqSlot &s = c->fq[f];
            uint32_t end = 0;
            FQD_TRY(read_words(c, &end, s.spans.as<uint32_t>() + (size_t)fqd::FQS_REC_END * s.rec_cap + (n - 1), 4));
            info->consumed[f] = end;
        }
        return FQD_OK;
    }
    const uint64_t *kept = kept_ids + kept_from;
    HIP_TRY(c, c->fq_ctr.reserve(std::max<size_t>(fqd::FQC_WORDS, fqd::FQE_WORDS) * 4));
    HIP_TRY(c, c->fq_lens.reserve((size_t)m * 4 + 16));
    HIP_TRY(c, c->fq_incl.reserve((size_t)m * 4 + 16));
    uint32_t *ctr = c->fq_ctr.as<uint32_t>(), *sizes = c->fq_lens.as<uint32_t>(), *incl = c->fq_incl.as<uint32_t>();
    HIP_TRY(c, fqd::launch_fastq_emit_init(ctr, c->st));
    for (uint32_t f = 0; f < c->fq_files; f++) {
        const FastqSlot &s = c->fq[f];
        const uint32_t *spans = s.spans.as<uint32_t>();
        KTIME(c, FQD_K_FASTQ_EMIT_SIZES,
              fqd::launch_fastq_emit_sizes(spans, s.rec_cap, f, (uint32_t)n, base_id, kept, m, sizes, ctr, c->st));
        FQD_TRY(scan_u32(c, sizes, incl, m));
        // the grid: a record's output is its raw bytes or less, but for one newline the last record may lack
        KTIME(c, FQD_K_FASTQ_EMIT_COPY,
              fqd::launch_fastq_emit_copy(s.d, spans, s.rec_cap, f, (uint32_t)n, base_id, kept, m, incl, s.n_bytes + 1,
                                          out[f], out_capacity[f], ctr, c->st));
    }
    uint32_t words[fqd::FQE_WORDS];
    FQD_TRY(read_words(c, words, ctr, sizeof words));
    if (c->kused > fqd_ctx::KPOOL - 40)
        ktime_collect(c);
    if (words[fqd::FQE_FAULT])
        return fail(c, FQD_E_VALUE, "fqd_fastq_emit: a kept id at kept_from lies below base_id (ids ascending, cursor past "
                                    "the earlier chunks?)");
    if (words[fqd::FQE_OVERFLOW])
        return fail(c, FQD_E_VALUE, "fqd_fastq_emit: out_capacity is too small for the kept records of this chunk");
    info->n_emitted = words[fqd::FQE_TAKEN];
    for (uint32_t f = 0; f < c->fq_files; f++) {
        info->out_bytes[f] = words[fqd::FQE_BYTES + f];
        info->consumed[f] = words[fqd::FQE_CONSUMED + f];
    }
    return FQD_OK;
}

int fqd_fastq_stats(fqd_ctx *c, uint64_t *out4)
{
    if (!c || !out4)
        return FQD_E_VALUE;
    out4[0] = c->fq_records;
    out4[1] = c->fq_key_bytes;
    out4[2] = c->fq_discarded;
    out4[3] = c->fq_chunks;
    return FQD_OK;
}

}  // extern "C"
