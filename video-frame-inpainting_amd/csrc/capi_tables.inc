// Passes over a table of tensors (included by sepconv_capi.hip).

namespace {

// The host copy of a table of tensors, `stride` words a row, checked before anything is launched.  elements(row, next) is the
// family's rule for one row: the number of elements it adds to the run of `seg`-element segments, or -1 when the row is not
// what `row_format` says (its first segment must be `next`, the segments of the rows before it).
template <typename RowRule>
int check_table(const char* who, const char* row_format, const long long* table_host, int n_entries, int stride, long long seg,
                long long n_segments, RowRule elements) {
    long long next = 0;
    for (int t = 0; t < n_entries; ++t) {
        const long long n = elements(table_host + (long long)stride * t, next);
        if (n < 0) {
            std::snprintf(g_err, sizeof(g_err), "%s: row %d is not {%s, first segment %lld}", who, t, row_format, next);
            return TAI_SEPCONV_EINVAL;
        }
        next += (n + seg - 1) / seg;
    }
    if (next != n_segments) {
        std::snprintf(g_err, sizeof(g_err), "%s: the table has %lld segments, not %lld", who, next, n_segments);
        return TAI_SEPCONV_EINVAL;
    }
    return TAI_SEPCONV_OK;
}

bool count_ok(long long n) { return n >= 0 && n < (1LL << 40); }

// workgroups over the segments unless the caller names a count: a multiple of the 256 CUs, eight workgroups of four waves each at
// the most; fewer when there is less to do
int table_blocks(long long n_segments, int blocks = 0) {
    if (blocks > 0) return blocks;
    const long long want = (n_segments + 255) / 256 * 256;
    return (int)(want < 2048 ? want : 2048);
}

// the table of fp32 tensors of tai_grad_stats and tai_grad_scale: rows of {address, elements, unused, first segment}
int grad_table_ok(const char* who, const long long* table_host, int n_entries, long long n_segments) {
    return check_table(who, "4-byte aligned address (0 exactly when empty), 0 <= elements < 2^40, unused", table_host, n_entries, 4, gstat::SEG, n_segments,
                       [](const long long* row, long long next) {
                           const long long addr = row[0], n = row[1];
                           return count_ok(n) && (addr & 3) == 0 && (addr == 0) == (n == 0) && row[3] == next ? n : -1;
                       });
}

// the table of tai_fused_step and tai_fused_step_decay: rows of {p, g, m, v, step tensor, e, elements, first segment}
int step_table_ok(const char* who, const long long* table_host, int n_entries, long long n_segments) {
    return check_table(who, "p, g, m, v (4-byte aligned, 0 exactly when empty), step, e, 0 <= elements < 2^40", table_host, n_entries,
                       fstep::ROW, fstep::SEG, n_segments, [](const long long* row, long long next) {
                           const long long n = row[6];
                           bool ok = count_ok(n) && row[7] == next && (row[4] & 3) == 0;
                           for (int a = 0; a < 4 && ok; ++a) ok = (row[a] & 3) == 0 && (row[a] == 0) == (n == 0);
                           return ok && (row[5] & 3) == 0 && (n != 0 || row[5] == 0) ? n : -1;
                       });
}

}  // namespace

extern "C" {

long long tai_state_digest_workspace_bytes(int n_entries, long long n_segments) {
    if (n_entries <= 0 || n_segments < 0) return TAI_SEPCONV_EINVAL;
    return 8LL * (n_segments + n_entries + 1);
}

int tai_state_digest(const long long* table, const long long* table_host, int n_entries, long long n_segments, long long seg_words,
                     void* workspace, unsigned long long* result, void* hip_stream) {
    g_err[0] = 0;
    if (!table || !table_host || !workspace || !result) return fail(TAI_SEPCONV_EINVAL, "%s", "state_digest: null pointer");
    if (n_entries <= 0 || seg_words <= 0 || seg_words % 4 != 0 || seg_words > (1LL << 30))
        return fail(TAI_SEPCONV_EINVAL, "%s", "state_digest: needs n_entries > 0 and 0 < seg_words <= 2^30, a multiple of 4");
    // rows of {address, words, sum, first segment}; a row without an address takes no segment
    const int ok = check_table("state_digest", "4-byte aligned address, 0 <= words < 2^40, sum", table_host, n_entries, 4, seg_words, n_segments,
                               [](const long long* row, long long next) {
                                   return count_ok(row[1]) && (row[0] & 3) == 0 && row[3] == next ? (row[0] != 0 ? row[1] : 0) : -1;
                               });
    if (ok != TAI_SEPCONV_OK) return ok;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    unsigned long long* slot = static_cast<unsigned long long*>(workspace);
    if (n_segments > 0) {
        hipLaunchKernelGGL(sdig::segment_sums, dim3(table_blocks(n_segments)), dim3(sdig::THREADS), 0, s, table, n_entries, n_segments, seg_words, slot);
        const int rc = check_launch("state_digest segment_sums");
        if (rc != 0) return rc;
    }
    hipLaunchKernelGGL(sdig::finish, dim3(1), dim3(sdig::THREADS), 0, s, table, n_entries, n_segments, slot, slot + n_segments, result);
    return check_launch("state_digest finish");
}

long long tai_grad_stats_workspace_bytes(int n_entries, long long n_segments) {
    if (n_entries <= 0 || n_segments < 0) return TAI_SEPCONV_EINVAL;
    return (long long)sizeof(gstat::SegOut) * (n_segments + 1);
}

int tai_grad_stats(const long long* table, const long long* table_host, int n_entries, long long n_segments, int blocks, void* workspace,
                   double* sumsq, float* maxabs, long long* nonfinite, void* hip_stream) {
    g_err[0] = 0;
    if (!table || !table_host || !workspace || !sumsq || !maxabs || !nonfinite) return fail(TAI_SEPCONV_EINVAL, "%s", "grad_stats: null pointer");
    if (n_entries <= 0 || blocks < 0 || blocks > 65536) return fail(TAI_SEPCONV_EINVAL, "%s", "grad_stats: needs n_entries > 0 and 0 <= blocks <= 65536");
    if (!aligned(workspace, 16) || !aligned(sumsq, 8) || !aligned(maxabs, 4) || !aligned(nonfinite, 8))
        return fail(TAI_SEPCONV_EINVAL, "%s", "grad_stats: workspace must be 16-byte aligned, the result arrays aligned to their elements");
    const int ok = grad_table_ok("grad_stats", table_host, n_entries, n_segments);
    if (ok != TAI_SEPCONV_OK) return ok;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    gstat::SegOut* slot = static_cast<gstat::SegOut*>(workspace);
    if (n_segments > 0) {
        hipLaunchKernelGGL(gstat::segment_stats, dim3(table_blocks(n_segments, blocks)), dim3(gstat::THREADS), 0, s, table, n_entries, n_segments, slot);
        const int rc = check_launch("grad_stats segment_stats");
        if (rc != 0) return rc;
    }
    hipLaunchKernelGGL(gstat::finish, dim3(1), dim3(gstat::THREADS), 0, s, table, n_entries, n_segments, slot, sumsq, maxabs, nonfinite);
    return check_launch("grad_stats finish");
}

long long tai_grad_scale_workspace_bytes(int n_entries, long long n_segments) {
    if (n_entries <= 0 || n_segments < 0) return TAI_SEPCONV_EINVAL;
    return 0;
}

int tai_grad_scale(const long long* table, const long long* table_host, int n_entries, long long n_segments, float c, int blocks,
                   void* workspace, void* hip_stream) {
    g_err[0] = 0;
    (void)workspace;
    if (!table || !table_host) return fail(TAI_SEPCONV_EINVAL, "%s", "grad_scale: null pointer");
    if (n_entries <= 0 || blocks < 0 || blocks > 65536) return fail(TAI_SEPCONV_EINVAL, "%s", "grad_scale: needs n_entries > 0 and 0 <= blocks <= 65536");
    if (!(c == c) || c - c != 0.0f) return fail(TAI_SEPCONV_EINVAL, "%s", "grad_scale: the factor must be finite");
    const int ok = grad_table_ok("grad_scale", table_host, n_entries, n_segments);
    if (ok != TAI_SEPCONV_OK) return ok;
    if (n_segments == 0) return TAI_SEPCONV_OK;
    hipLaunchKernelGGL(gstat::scale_segments, dim3(table_blocks(n_segments, blocks)), dim3(gstat::THREADS), 0, static_cast<hipStream_t>(hip_stream),
                       table, n_entries, n_segments, c);
    return check_launch("grad_scale");
}

long long tai_step_verdict_workspace_bytes(void) {
    return 8LL * fstep::REC_WORDS;
}

int tai_step_verdict(const double* sumsq, const long long* nonfinite, int n_entries, double max_norm, int which, int close_update,
                     long long patience, long long table_len, long long* record, void* hip_stream) {
    g_err[0] = 0;
    if (!record || !aligned(record, 8)) return fail(TAI_SEPCONV_EINVAL, "%s", "step_verdict: the record must be an 8-byte aligned device pointer");
    if ((sumsq == nullptr) != (nonfinite == nullptr)) return fail(TAI_SEPCONV_EINVAL, "%s", "step_verdict: sumsq and nonfinite come together or not at all");
    if (!aligned(sumsq, 8) || !aligned(nonfinite, 8)) return fail(TAI_SEPCONV_EINVAL, "%s", "step_verdict: sumsq and nonfinite must be 8-byte aligned");
    if ((sumsq && n_entries <= 0) || n_entries < 0 || (which != 0 && which != 1) || patience < 1 || table_len < 1 || !(max_norm >= 0.0) || max_norm - max_norm != 0.0)
        return fail(TAI_SEPCONV_EINVAL, "%s", "step_verdict: needs n_entries > 0 with statistics, which in {0, 1}, patience >= 1, table_len >= 1 and a finite max_norm >= 0 (0 = no clipping)");
    hipLaunchKernelGGL(fstep::step_verdict, dim3(1), dim3(fstep::THREADS), 0, static_cast<hipStream_t>(hip_stream), sumsq, nonfinite, n_entries,
                       max_norm, which, close_update != 0, patience, table_len, record);
    return check_launch("step_verdict");
}

long long tai_fused_step_workspace_bytes(int n_entries, long long n_segments) {
    if (n_entries <= 0 || n_segments < 0) return TAI_SEPCONV_EINVAL;
    return 0;
}

int tai_fused_step(const long long* table, const long long* table_host, int n_entries, long long n_segments, const float* scalars,
                   long long table_len, float w1, float b2, float w2, float eps, float wE, const long long* record, int which, int nt,
                   int blocks, void* workspace, void* hip_stream) {
    g_err[0] = 0;
    (void)workspace;
    if (!table || !table_host || !scalars || !record) return fail(TAI_SEPCONV_EINVAL, "%s", "fused_step: null pointer");
    if (n_entries <= 0 || blocks < 0 || blocks > 65536 || (which != 0 && which != 1) || table_len < 1 || !aligned(record, 8) || !aligned(scalars, 4))
        return fail(TAI_SEPCONV_EINVAL, "%s", "fused_step: needs n_entries > 0, 0 <= blocks <= 65536, which in {0, 1}, table_len >= 1, aligned record and scalars");
    const int ok = step_table_ok("fused_step", table_host, n_entries, n_segments);
    if (ok != TAI_SEPCONV_OK) return ok;
    const fstep::Scalars k = {w1, b2, w2, eps, wE};
    const dim3 grid(table_blocks(n_segments > 0 ? n_segments : 1, blocks)), block(fstep::THREADS);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    hipLaunchKernelGGL(nt ? fstep::step_segments<true> : fstep::step_segments<false>, grid, block, 0, s, table, n_entries, n_segments, scalars, table_len,
                       k, record, which);
    return check_launch("fused_step");
}

long long tai_fused_step_decay_workspace_bytes(int n_entries, long long n_segments) {
    if (n_entries <= 0 || n_segments < 0) return TAI_SEPCONV_EINVAL;
    return 0;
}

int tai_fused_step_decay(const long long* table, const long long* table_host, const long long* flags, const long long* flags_host,
                         int n_entries, long long n_segments, const float* scalars, long long table_len, float w1, float b2, float w2,
                         float eps, float wE, const long long* record, int which, int blocks, void* workspace, void* stream) {
    g_err[0] = 0;
    (void)workspace;
    if (const char* why = fstep::refusal(table, table_host, flags, flags_host, n_entries, scalars, table_len, record, which, blocks))
        return fail(TAI_SEPCONV_EINVAL, "%s", why);
    const int ok = step_table_ok("fused_step_decay", table_host, n_entries, n_segments);
    if (ok != TAI_SEPCONV_OK) return ok;
    const fstep::Scalars k = {w1, b2, w2, eps, wE};
    const dim3 grid(table_blocks(n_segments > 0 ? n_segments : 1, blocks)), block(fstep::THREADS);
    hipLaunchKernelGGL(fstep::step_segments_decay, grid, block, 0, static_cast<hipStream_t>(stream), table, flags, n_entries, n_segments, scalars,
                       table_len, k, record, which);
    return check_launch("fused_step_decay");
}

}  // extern "C"
