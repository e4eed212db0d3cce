// C-ABI layer of the UMC drivers' device stages: asr_resize_pages_dev (page scans of any resolution -> pages of the
// networks' width), asr_unroll_systems_dev (page scans -> unrolled strips), asr_resample_batch_dev (recordings at any
// rate -> recordings at the front-end's rate), asr_spectrogram_batch_dev (recordings -> spectrograms) and
// asr_audio_stream_push_dev / asr_audio_stream_push_fft_dev (blocks of streamed samples at any rate -> the spectrogram
// frames they complete, by the direct DFT / by the FFT; audio_stream_fft_kernels.hip);
// include/asr_hip.h for the contract.  Kernels: page_resize_kernels.hip, umc_kernels.hip, resample_kernels.hip,
// piece_vote_kernels.hip (spectrogram_batch_kernel), audio_stream_kernels.hip.  Every call checks every offset against the buffer sizes the
// caller states before anything is launched, and returns after the work is done.
// asr_spectrogram_fft_batch_dev (asr_spectrogram_batch_dev's spectrograms with the magnitudes from a real-input FFT):
// spectrogram_fft_kernels.hip.
// asr_skew_estimate_dev / asr_deskew_pages_dev (the slope of a scan's staves and its correction, before the resize):
// page_deskew_kernels.hip.
// asr_flatten_pages_dev (a scan divided by the grey closing of its paper, before the deskew): page_flatten_kernels.hip.
// asr_crop_estimate_dev / asr_crop_pages_dev (the paper's rectangle inside a scanner's black border and its copy, before
// the flatten): page_crop_kernels.hip.
// asr_score_map_dev (the bar network's maps and the unroll table -> the measures of every piece in strip coordinates):
// score_map_kernels.hip.
#include "asr_ctx.h"

int asr_unroll_systems_dev(asr_ctx *ctx, const void *pages_dev, int64_t pages_bytes, const int64_t *page_offsets,
                           const int32_t *heights, const int32_t *widths, int n_pages, const int32_t *systems,
                           int n_systems, int system_height, const int64_t *strip_offsets, const int32_t *strip_widths,
                           int n_pieces, float *strips_dev, int64_t strips_floats) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n_pages < 0 || n_systems < 0 || n_pieces < 0 || system_height < 1 || pages_bytes < 0 || strips_floats < 0)
        return fail(ctx, ASR_ERR_INVALID, "unroll_systems: bad sizes");
    if (n_systems == 0) return ASR_OK;
    if (!pages_dev || !page_offsets || !heights || !widths || !systems || !strip_offsets || !strip_widths || !strips_dev)
        return fail(ctx, ASR_ERR_INVALID, "unroll_systems: NULL argument");
    for (int p = 0; p < n_pages; ++p)
        if (heights[p] < 0 || widths[p] < 0 || page_offsets[p] < 0 ||
            page_offsets[p] + (int64_t)heights[p] * widths[p] > pages_bytes)
            return fail(ctx, ASR_ERR_INVALID, "unroll_systems: page %d (%d x %d at %lld) outside the %lld-byte buffer", p,
                        heights[p], widths[p], (long long)page_offsets[p], (long long)pages_bytes);
    for (int q = 0; q < n_pieces; ++q)
        if (strip_widths[q] < 0 || strip_offsets[q] < 0 ||
            strip_offsets[q] + (int64_t)system_height * strip_widths[q] > strips_floats)
            return fail(ctx, ASR_ERR_INVALID, "unroll_systems: strip %d (%d x %d at %lld) outside the %lld-float buffer", q,
                        system_height, strip_widths[q], (long long)strip_offsets[q], (long long)strips_floats);
    std::vector<asr::UnrollSystem> table(n_systems);
    double pixels = 0.0;
    for (int i = 0; i < n_systems; ++i) {
        const int32_t *t = systems + (size_t)i * 8;
        const int32_t page = t[0], r0 = t[1], r1 = t[2], c0 = t[3], c1 = t[4], pad = t[5], piece = t[6], col = t[7];
        if (page < 0 || page >= n_pages || piece < 0 || piece >= n_pieces)
            return fail(ctx, ASR_ERR_INVALID, "unroll_systems: system %d names page %d / piece %d", i, page, piece);
        if (r0 < 0 || r1 <= r0 || r1 > heights[page] || c0 < 0 || c1 <= c0 || c1 > widths[page] || pad < 0 ||
            (int64_t)r1 - r0 + pad != system_height)
            return fail(ctx, ASR_ERR_INVALID, "unroll_systems: system %d rows [%d, %d) + %d, columns [%d, %d) do not fit "
                        "page %d (%d x %d) / height %d", i, r0, r1, pad, c0, c1, page, heights[page], widths[page],
                        system_height);
        if (col < 0 || (int64_t)col + (c1 - c0) > strip_widths[piece])
            return fail(ctx, ASR_ERR_INVALID, "unroll_systems: system %d columns [%d, %d) outside strip %d of width %d", i,
                        col, col + (c1 - c0), piece, strip_widths[piece]);
        asr::UnrollSystem &u = table[i];
        u.src = page_offsets[page] + (int64_t)r0 * widths[page] + c0;
        u.dst = strip_offsets[piece] + col;
        u.src_stride = widths[page];
        u.dst_stride = strip_widths[piece];
        u.rows = r1 - r0;
        u.width = c1 - c0;
        pixels += (double)system_height * (c1 - c0);
    }
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    int rc = join_views(ctx);
    if (rc != ASR_OK) return rc;
    asr::UnrollSystem *d_table = nullptr;
    const size_t bytes = table.size() * sizeof(asr::UnrollSystem);
    ASR_HIP(ctx, hipMalloc((void **)&d_table, bytes));
    hipError_t e = hipMemcpyAsync(d_table, table.data(), bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        ProfScope ps(ctx, "unroll_systems", 0, 0.0, 5.0 * pixels);
        e = asr::launch_unroll_systems(ctx->stream, (const uint8_t *)pages_dev, d_table, n_systems, system_height, strips_dev);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    (void)hipFree(d_table);
    if (e != hipSuccess) return fail(ctx, ASR_ERR_HIP, "unroll_systems: %s", hipGetErrorString(e));
    return mark_main(ctx);
}

int asr_spectrogram_batch_dev(asr_ctx *ctx, const float *samples_dev, int64_t samples_floats,
                              const int64_t *sample_offsets, const int64_t *sample_counts, const int64_t *n_frames,
                              const int64_t *out_offsets, int n_recordings, int frame_size, double hop,
                              const float *window, const int32_t *fb_start, const int32_t *fb_len,
                              const float *fb_weights, int n_filters, float mul, float add, int transposed,
                              float *out_dev, int64_t out_floats) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n_recordings < 0 || samples_floats < 0 || out_floats < 0 || frame_size < 64 || frame_size > 8192 ||
        (frame_size & (frame_size - 1)) || !(hop > 0.0) || n_filters < 1 || n_filters > 4096)
        return fail(ctx, ASR_ERR_INVALID, "spectrogram_batch: bad sizes (frame_size must be a power of two in [64, 8192])");
    if (n_recordings == 0) return ASR_OK;
    if (!sample_offsets || !sample_counts || !n_frames || !out_offsets)
        return fail(ctx, ASR_ERR_INVALID, "spectrogram_batch: NULL argument");
    std::vector<int64_t> tab((size_t)4 * n_recordings + 1);      // frame_first (n + 1) | sample_off | sample_cnt | out_off
    int64_t *first = tab.data(), *s_off = first + n_recordings + 1, *s_cnt = s_off + n_recordings,
            *o_off = s_cnt + n_recordings;
    int64_t total = 0;
    for (int i = 0; i < n_recordings; ++i) {
        if (sample_counts[i] < 0 || n_frames[i] < 0 || sample_offsets[i] < 0 || out_offsets[i] < 0 ||
            sample_offsets[i] + sample_counts[i] > samples_floats ||
            out_offsets[i] + n_frames[i] * (int64_t)n_filters > out_floats)
            return fail(ctx, ASR_ERR_INVALID, "spectrogram_batch: recording %d (%lld samples at %lld, %lld frames at %lld) "
                        "outside its buffers (%lld / %lld floats)", i, (long long)sample_counts[i],
                        (long long)sample_offsets[i], (long long)n_frames[i], (long long)out_offsets[i],
                        (long long)samples_floats, (long long)out_floats);
        first[i] = total;
        s_off[i] = sample_offsets[i];
        s_cnt[i] = sample_counts[i];
        o_off[i] = out_offsets[i];
        total += n_frames[i];
    }
    first[n_recordings] = total;
    if (total == 0) return ASR_OK;
    if (!samples_dev || !window || !fb_start || !fb_len || !fb_weights || !out_dev)
        return fail(ctx, ASR_ERR_INVALID, "spectrogram_batch: NULL argument");
    std::vector<int32_t> off(n_filters);
    int64_t total_w = 0;
    int max_bin = 0;
    for (int f = 0; f < n_filters; ++f) {
        if (fb_start[f] < 0 || fb_len[f] < 0 || fb_start[f] + fb_len[f] > frame_size / 2)
            return fail(ctx, ASR_ERR_INVALID, "spectrogram_batch: filter %d covers bins [%d, %d) outside [0, %d)", f,
                        fb_start[f], fb_start[f] + fb_len[f], frame_size / 2);
        off[f] = (int32_t)total_w;
        total_w += fb_len[f];
        max_bin = std::max(max_bin, fb_start[f] + fb_len[f]);
    }
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    int rc = join_views(ctx);
    if (rc != ASR_OK) return rc;
    char *buf = nullptr;
    const size_t b_tab = tab.size() * 8, b_win = (size_t)frame_size * 4, b_i = (size_t)n_filters * 4,
                 b_w = (size_t)std::max<int64_t>(total_w, 1) * 4;
    ASR_HIP(ctx, hipMalloc((void **)&buf, b_tab + b_win + 3 * b_i + b_w));
    int64_t *d_tab = (int64_t *)buf;
    float *d_win = (float *)(buf + b_tab);
    int32_t *d_start = (int32_t *)(buf + b_tab + b_win), *d_len = d_start + n_filters, *d_off = d_len + n_filters;
    float *d_w = (float *)(buf + b_tab + b_win + 3 * b_i);
    hipError_t e = hipMemcpyAsync(d_tab, tab.data(), b_tab, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_win, window, b_win, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_start, fb_start, b_i, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_len, fb_len, b_i, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_off, off.data(), b_i, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && total_w) e = hipMemcpyAsync(d_w, fb_weights, (size_t)total_w * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        ProfScope ps(ctx, "spectrogram_batch", 0, 4.0 * frame_size * (double)max_bin * (double)total,
                     4.0 * hop * (double)total);
        e = asr::launch_spectrogram_batch(ctx->stream, samples_dev, d_tab, d_tab + n_recordings + 1,
                                          d_tab + 2 * n_recordings + 1, d_tab + 3 * n_recordings + 1, n_recordings, total,
                                          d_win, frame_size, hop, max_bin, d_start, d_len, d_off, d_w, n_filters, mul, add,
                                          out_dev, transposed);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    (void)hipFree(buf);
    if (e != hipSuccess) return fail(ctx, ASR_ERR_HIP, "spectrogram_batch: %s", hipGetErrorString(e));
    return mark_main(ctx);
}

// the twiddle table of spectrogram_fft_kernels.hip: exp(-2 pi i t / 2048) as (cos, -sin), t = 0 .. 2047, float32 rounded
// from float64 - the one place it is computed.  The quadrant is taken out first so that the multiples of pi / 2 are exact.
static const std::vector<float> &specfft_twiddles() {
    static const std::vector<float> table = [] {
        std::vector<float> tw(2 * 2048);
        const double kPi = 3.14159265358979323846;
        for (int t = 0; t < 2048; ++t) {
            const int quad = t >> 9, r = t & 511;
            const double c = cos(2.0 * kPi * r / 2048.0), s = sin(2.0 * kPi * r / 2048.0);
            const double cs[4][2] = {{c, s}, {-s, c}, {-c, -s}, {s, -c}};    // cos, sin of the angle + quad * pi / 2
            tw[2 * t] = (float)cs[quad][0];
            tw[2 * t + 1] = (float)-cs[quad][1];
        }
        return tw;
    }();
    return table;
}

// the FFT routes' workspace (asr_spectrogram_fft_batch_dev, asr_audio_stream_push_fft_dev): the twiddle table in front,
// then the per-call tables of the batched call; a (re)allocation uploads the table again, so whichever call comes first
// in a context finds it on the device
static int specfft_workspace(asr_ctx *ctx, size_t need) {
    if (need <= ctx->specfft_ws_bytes) return ASR_OK;
    const std::vector<float> &tw = specfft_twiddles();
    ASR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->specfft_ws) ASR_HIP(ctx, hipFree(ctx->specfft_ws));
    ctx->specfft_ws = nullptr; ctx->specfft_ws_bytes = 0;
    const size_t bytes = need + need / 2;                           // growing recording tables do not reallocate each time
    ASR_HIP(ctx, hipMalloc(&ctx->specfft_ws, bytes));
    ctx->specfft_ws_bytes = bytes;
    ASR_HIP(ctx, hipMemcpy(ctx->specfft_ws, tw.data(), tw.size() * 4, hipMemcpyHostToDevice));
    return ASR_OK;
}

int asr_spectrogram_fft_batch_dev(asr_ctx *ctx, const float *samples_dev, int64_t samples_floats,
                                  const int64_t *sample_offsets, const int64_t *sample_counts, const int64_t *n_frames,
                                  const int64_t *out_offsets, int n_recordings, int frame_size, double hop,
                                  const float *window, const int32_t *fb_start, const int32_t *fb_len,
                                  const float *fb_weights, int n_filters, float mul, float add, int transposed,
                                  float *out_dev, int64_t out_floats) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n_recordings < 0 || samples_floats < 0 || out_floats < 0 || !(hop > 0.0) || n_filters < 1 || n_filters > 4096)
        return fail(ctx, ASR_ERR_INVALID, "spectrogram_fft_batch: bad sizes");
    if (frame_size != 2048)
        return fail(ctx, ASR_ERR_INVALID, "spectrogram_fft_batch: frame_size %d (the FFT route has frames of 2048 samples; "
                    "asr_spectrogram_batch_dev takes the others)", frame_size);
    if (n_recordings == 0) return ASR_OK;
    if (!sample_offsets || !sample_counts || !n_frames || !out_offsets)
        return fail(ctx, ASR_ERR_INVALID, "spectrogram_fft_batch: NULL argument");
    // one host image of everything the launch reads besides the samples:
    // frame_first (n + 1) | sample_off | sample_cnt | out_off | window | fb_start | fb_len | fb_off | weights
    const size_t n_tab = (size_t)4 * n_recordings + 1;
    std::vector<int64_t> tab(n_tab);
    int64_t *first = tab.data(), *s_off = first + n_recordings + 1, *s_cnt = s_off + n_recordings,
            *o_off = s_cnt + n_recordings;
    int64_t total = 0;
    for (int i = 0; i < n_recordings; ++i) {
        if (sample_counts[i] < 0 || n_frames[i] < 0 || sample_offsets[i] < 0 || out_offsets[i] < 0 ||
            sample_counts[i] > samples_floats || sample_offsets[i] > samples_floats - sample_counts[i] ||
            n_frames[i] > out_floats / n_filters || out_offsets[i] > out_floats - n_frames[i] * (int64_t)n_filters)
            return fail(ctx, ASR_ERR_INVALID, "spectrogram_fft_batch: recording %d (%lld samples at %lld, %lld frames at "
                        "%lld) outside its buffers (%lld / %lld floats)", i, (long long)sample_counts[i],
                        (long long)sample_offsets[i], (long long)n_frames[i], (long long)out_offsets[i],
                        (long long)samples_floats, (long long)out_floats);
        first[i] = total;
        s_off[i] = sample_offsets[i];
        s_cnt[i] = sample_counts[i];
        o_off[i] = out_offsets[i];
        total += n_frames[i];
    }
    first[n_recordings] = total;
    if (total == 0) return ASR_OK;
    if (!samples_dev || !window || !fb_start || !fb_len || !fb_weights || !out_dev)
        return fail(ctx, ASR_ERR_INVALID, "spectrogram_fft_batch: NULL argument");
    std::vector<int32_t> off(n_filters);
    int64_t total_w = 0;
    for (int f = 0; f < n_filters; ++f) {
        if (fb_start[f] < 0 || fb_len[f] < 0 || fb_start[f] > 1024 || fb_len[f] > 1024 - fb_start[f])
            return fail(ctx, ASR_ERR_INVALID, "spectrogram_fft_batch: filter %d covers bins [%d, %d) outside [0, 1024)", f,
                        fb_start[f], fb_start[f] + fb_len[f]);
        off[f] = (int32_t)total_w;
        total_w += fb_len[f];
    }
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    int rc = join_views(ctx);
    if (rc != ASR_OK) return rc;
    const std::vector<float> &tw = specfft_twiddles();
    const size_t b_tw = tw.size() * 4, b_tab = n_tab * 8, b_win = (size_t)2048 * 4, b_i = (size_t)n_filters * 4,
                 b_w = (size_t)total_w * 4, b_call = b_tab + b_win + 3 * b_i + b_w, need = b_tw + b_call;
    rc = specfft_workspace(ctx, need);
    if (rc != ASR_OK) return rc;
    std::vector<char> image(b_call);
    memcpy(image.data(), tab.data(), b_tab);
    memcpy(image.data() + b_tab, window, b_win);
    memcpy(image.data() + b_tab + b_win, fb_start, b_i);
    memcpy(image.data() + b_tab + b_win + b_i, fb_len, b_i);
    memcpy(image.data() + b_tab + b_win + 2 * b_i, off.data(), b_i);
    if (b_w) memcpy(image.data() + b_tab + b_win + 3 * b_i, fb_weights, b_w);
    char *d_call = (char *)ctx->specfft_ws + b_tw;                  // 8-byte aligned: b_tw, b_tab and b_win are multiples of 8
    const int64_t *d_tab = (const int64_t *)d_call;
    const float *d_win = (const float *)(d_call + b_tab);
    const int32_t *d_start = (const int32_t *)(d_call + b_tab + b_win), *d_len = d_start + n_filters,
                  *d_off = d_len + n_filters;
    const float *d_w = (const float *)(d_call + b_tab + b_win + 3 * b_i);
    hipError_t e = hipMemcpyAsync(d_call, image.data(), b_call, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        // 5 passes of 1024 complex values at about 8.5 FLOP per value, the post-pass, the filterbank
        ProfScope ps(ctx, "spectrogram_fft_batch", 0, (5.0 * 1024 * 8.5 + 1024 * 16.0 + 2.0 * total_w) * (double)total,
                     4.0 * hop * (double)total);
        e = asr::launch_spectrogram_fft_batch(ctx->stream, samples_dev, d_tab, d_tab + n_recordings + 1,
                                              d_tab + 2 * n_recordings + 1, d_tab + 3 * n_recordings + 1, n_recordings,
                                              total, (const float *)ctx->specfft_ws, d_win, hop, d_start, d_len, d_off,
                                              d_w, n_filters, mul, add, out_dev, transposed);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, ASR_ERR_HIP, "spectrogram_fft_batch: %s", hipGetErrorString(e));
    return mark_main(ctx);
}

int asr_resample_batch_dev(asr_ctx *ctx, const float *in_dev, int64_t in_floats, const int64_t *in_offsets,
                           const int64_t *in_counts, const int64_t *out_offsets, const int64_t *out_counts,
                           int n_recordings, int up, int down, const double *taps_phase_major, int taps_per_phase,
                           int half, int round_int16, float *out_dev, int64_t out_floats) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n_recordings < 0 || in_floats < 0 || out_floats < 0)
        return fail(ctx, ASR_ERR_INVALID, "resample_batch: bad sizes");
    if (up < 1 || down < 1)
        return fail(ctx, ASR_ERR_INVALID, "resample_batch: ratio %d / %d (up and down must be at least 1)", up, down);
    if (half < 0 || taps_per_phase < 1 || (int64_t)taps_per_phase * up < 2 * (int64_t)half + 1)
        return fail(ctx, ASR_ERR_INVALID, "resample_batch: %d taps per phase x %d phases do not hold the %lld taps of "
                    "half = %d", taps_per_phase, up, 2 * (long long)half + 1, half);
    if (((int64_t)asr::RESAMPLE_TILE * down + up - 1) / up + taps_per_phase + 1 > (int64_t)(asr::RESAMPLE_MAX_LDS / 4))
        return fail(ctx, ASR_ERR_INVALID, "resample_batch: ratio %d / %d with %d taps per phase: the input span of a tile "
                    "does not fit %zu bytes of LDS", up, down, taps_per_phase, asr::RESAMPLE_MAX_LDS);
    if (n_recordings == 0) return ASR_OK;
    if (!in_offsets || !in_counts || !out_offsets || !out_counts)
        return fail(ctx, ASR_ERR_INVALID, "resample_batch: NULL argument");
    std::vector<int64_t> tab((size_t)5 * n_recordings + 1);      // tile_first (n + 1) | in_off | in_cnt | out_off | out_cnt
    int64_t *first = tab.data(), *i_off = first + n_recordings + 1, *i_cnt = i_off + n_recordings,
            *o_off = i_cnt + n_recordings, *o_cnt = o_off + n_recordings;
    // every index the kernel forms stays below in_counts * up + half + down: keep that inside int64
    const int64_t max_count = (INT64_MAX - half - down) / up - 1;
    int64_t tiles = 0, total_out = 0;
    for (int i = 0; i < n_recordings; ++i) {
        if (in_counts[i] < 0 || out_counts[i] < 0 || in_offsets[i] < 0 || out_offsets[i] < 0 ||
            in_counts[i] > in_floats || in_offsets[i] > in_floats - in_counts[i] ||
            out_counts[i] > out_floats || out_offsets[i] > out_floats - out_counts[i])
            return fail(ctx, ASR_ERR_INVALID, "resample_batch: recording %d (%lld samples at %lld, %lld outputs at %lld) "
                        "outside its buffers (%lld / %lld floats)", i, (long long)in_counts[i], (long long)in_offsets[i],
                        (long long)out_counts[i], (long long)out_offsets[i], (long long)in_floats, (long long)out_floats);
        if (in_counts[i] > max_count)
            return fail(ctx, ASR_ERR_INVALID, "resample_batch: recording %d: %lld samples x %d overflow", i,
                        (long long)in_counts[i], up);
        const int64_t want = (in_counts[i] * up + down - 1) / down;
        if (out_counts[i] != want)
            return fail(ctx, ASR_ERR_INVALID, "resample_batch: recording %d: %lld outputs stated, %lld samples x %d / %d "
                        "give %lld", i, (long long)out_counts[i], (long long)in_counts[i], up, down, (long long)want);
        first[i] = tiles;
        i_off[i] = in_offsets[i];
        i_cnt[i] = in_counts[i];
        o_off[i] = out_offsets[i];
        o_cnt[i] = out_counts[i];
        tiles += (out_counts[i] + asr::RESAMPLE_TILE - 1) / asr::RESAMPLE_TILE;
        total_out += out_counts[i];
    }
    first[n_recordings] = tiles;
    if (tiles == 0) return ASR_OK;
    if (tiles > 0x7fffffffLL)
        return fail(ctx, ASR_ERR_INVALID, "resample_batch: %lld tiles in one call", (long long)tiles);
    if (!in_dev || !out_dev || !taps_phase_major) return fail(ctx, ASR_ERR_INVALID, "resample_batch: NULL argument");
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    int rc = join_views(ctx);
    if (rc != ASR_OK) return rc;
    const size_t b_tab = tab.size() * 8, b_taps = (size_t)up * taps_per_phase * 8, need = b_tab + b_taps;
    if (need > ctx->resample_ws_bytes) {
        ASR_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->resample_ws) ASR_HIP(ctx, hipFree(ctx->resample_ws));
        ctx->resample_ws = nullptr; ctx->resample_ws_bytes = 0;
        ASR_HIP(ctx, hipMalloc(&ctx->resample_ws, need));
        ctx->resample_ws_bytes = need;
    }
    int64_t *d_tab = (int64_t *)ctx->resample_ws;
    double *d_taps = (double *)((char *)ctx->resample_ws + b_tab);
    hipError_t e = hipMemcpyAsync(d_tab, tab.data(), b_tab, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_taps, taps_phase_major, b_taps, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        const double n_in_total = (double)total_out * down / up;
        ProfScope ps(ctx, "resample_batch", 0, 2.0 * taps_per_phase * (double)total_out,
                     4.0 * (n_in_total + (double)total_out));
        const int n = n_recordings;
        e = asr::launch_resample_batch(ctx->stream, in_dev, out_dev, d_tab, d_tab + n + 1, d_tab + 2 * n + 1,
                                       d_tab + 3 * n + 1, d_tab + 4 * n + 1, n, tiles, up, down, half, taps_per_phase,
                                       d_taps, round_int16 ? 1 : 0);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, ASR_ERR_HIP, "resample_batch: %s", hipGetErrorString(e));
    return mark_main(ctx);
}

// ---- asr_audio_stream_push_dev: the host half of the stream's integer plan (audio_frontend.audio_stream_plan restates it)
namespace {

struct StreamPlan {
    int up, down, half, T, F; double hop; bool native;
    int64_t start(int64_t i) const { return (int64_t)((double)i * hop); }
    // M(n): outputs of the resampler that n input samples make final, j0(m) = (m * down + half) / up < n
    int64_t final_outputs(int64_t n) const {
        if (native) return n;
        const int64_t num = n * up - half;
        return num <= 0 ? 0 : std::min((num + down - 1) / down, (n * up + down - 1) / down);
    }
    int64_t length(int64_t n) const { return native ? n : (n * up + down - 1) / down; }   // of the whole recording
    // frames i with start(i) + F <= m: an estimate, then the definition
    int64_t complete_frames(int64_t m) const {
        if (m < F) return 0;
        int64_t k = (int64_t)((double)(m - F) / hop);
        while (start(k) + F <= m) ++k;
        while (k > 0 && start(k - 1) + F > m) --k;
        return k;
    }
    int64_t keep_from(int64_t next_frame, int64_t n) const {
        const int64_t s = start(next_frame);
        const int64_t j = native ? s : (s * down + half) / up - (T - 1);
        return std::max<int64_t>(0, std::min(j, n));
    }
    // n - keep_from never exceeds this (the proof is with audio_frontend.audio_stream_state_len)
    int64_t state_len() const { return native ? F - 1 : ((int64_t)(F - 1) * down + up - 1) / up + T - 1; }
};

}  // namespace

// asr_audio_stream_push_dev (fft == false, who = "audio_stream_push") and asr_audio_stream_push_fft_dev (fft == true,
// "audio_stream_push_fft"): the checks, the plan, the rows, the overlap test and the taps cache are one; the two differ in
// the frame sizes and filters they take, in the LDS a frame needs and in the kernel that computes the frames
#define STREAM_FAIL(code, fmt, ...) fail(ctx, code, "%s: " fmt, who, ##__VA_ARGS__)
static int audio_stream_push(asr_ctx *ctx, bool fft, const char *who, const float *blocks_dev, int64_t blocks_floats,
                             const int64_t *block_offsets, const int64_t *block_counts, const int64_t *samples_before,
                             const int32_t *final_flags, const int64_t *first_frames, const int64_t *n_new_frames,
                             const int64_t *out_offsets, int n_streams, int up, int down, const double *taps_phase_major,
                             int taps_per_phase, int half, int round_int16, float *state_dev, int64_t state_floats,
                             const int64_t *state_offsets, int64_t state_cap, int frame_size, double hop,
                             const float *window, const int32_t *fb_start, const int32_t *fb_len,
                             const float *fb_weights, int n_filters, float mul, float add, int transposed,
                             float *out_dev, int64_t out_floats) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n_streams < 0 || blocks_floats < 0 || state_floats < 0 || state_cap < 0 || out_floats < 0 || frame_size < 64 ||
        frame_size > 8192 || (frame_size & (frame_size - 1)) || !(hop > 0.0) || n_filters < 1 || n_filters > 4096)
        return STREAM_FAIL(ASR_ERR_INVALID, "bad sizes (frame_size must be a power of two in [64, 8192])");
    if (fft && frame_size != 2048)
        return STREAM_FAIL(ASR_ERR_INVALID, "frame_size %d (the FFT route has frames of 2048 samples; "
                           "asr_audio_stream_push_dev takes the others)", frame_size);
    if (up < 1 || down < 1)
        return STREAM_FAIL(ASR_ERR_INVALID, "ratio %d / %d (up and down must be at least 1)", up, down);
    const bool native = !taps_phase_major;
    if (native && (up != 1 || down != 1))
        return STREAM_FAIL(ASR_ERR_INVALID, "ratio %d / %d without taps (only 1 / 1 is the front-end's "
                    "own rate)", up, down);
    if (!native && (half < 0 || taps_per_phase < 1 || (int64_t)taps_per_phase * up < 2 * (int64_t)half + 1))
        return STREAM_FAIL(ASR_ERR_INVALID, "%d taps per phase x %d phases do not hold the %lld taps of "
                    "half = %d", taps_per_phase, up, 2 * (long long)half + 1, half);
    if (!window || !fb_start || !fb_len || !fb_weights)
        return STREAM_FAIL(ASR_ERR_INVALID, "NULL argument");
    std::vector<int32_t> off(n_filters);
    int64_t total_w = 0;
    int max_bin = 0;
    for (int f = 0; f < n_filters; ++f) {
        if (fb_start[f] < 0 || fb_len[f] < 0 || fb_start[f] + fb_len[f] > frame_size / 2)
            return STREAM_FAIL(ASR_ERR_INVALID, "filter %d covers bins [%d, %d) outside [0, %d)", f,
                        fb_start[f], fb_start[f] + fb_len[f], frame_size / 2);
        off[f] = (int32_t)total_w;
        total_w += fb_len[f];
        max_bin = std::max(max_bin, fb_start[f] + fb_len[f]);
    }
    const StreamPlan plan{up, down, native ? 0 : half, native ? 1 : taps_per_phase, frame_size, hop, native};
    const int64_t span64 = native ? 0 : ((int64_t)(frame_size - 1) * down + up - 1) / up + taps_per_phase;
    // the FFT kernel never needs more than the direct one at the same span: it takes every ratio that one takes
    if (span64 > (int64_t)(asr::AUDIO_STREAM_MAX_LDS / 4) ||
        (fft ? asr::audio_stream_fft_lds((int)span64) : asr::audio_stream_lds(frame_size, max_bin, (int)span64)) >
            asr::AUDIO_STREAM_MAX_LDS)
        return STREAM_FAIL(ASR_ERR_INVALID, "ratio %d / %d with %d taps per phase and frames of %d: the "
                    "input span of a frame (%lld samples) does not fit %zu bytes of LDS", up, down, taps_per_phase,
                    frame_size, (long long)span64, asr::AUDIO_STREAM_MAX_LDS);
    if (state_cap < plan.state_len())
        return STREAM_FAIL(ASR_ERR_INVALID, "a state of %lld floats per stream, %lld are needed",
                    (long long)state_cap, (long long)plan.state_len());
    if (n_streams == 0) return ASR_OK;
    if (!block_offsets || !block_counts || !samples_before || !final_flags || !first_frames || !n_new_frames ||
        !out_offsets || !state_offsets)
        return STREAM_FAIL(ASR_ERR_INVALID, "NULL argument");
    const int n = n_streams;
    const size_t b_first = ((size_t)n + 1) * 8, b_rows = (size_t)n * sizeof(asr::StreamRow), b_win = (size_t)frame_size * 4,
                 b_i = (size_t)n_filters * 4, b_w = (size_t)std::max<int64_t>(total_w, 1) * 4;
    std::vector<char> tab(b_first + b_rows + b_win + 3 * b_i + b_w);  // frame_first | rows | window | start, len, off | w
    int64_t *first = (int64_t *)tab.data();
    asr::StreamRow *rows = (asr::StreamRow *)(tab.data() + b_first);
    // every index the kernels form stays below n1 * up + (frame_size + 2) * down + half: keep that inside int64
    const int64_t max_count = (INT64_MAX - half - (int64_t)(frame_size + 2) * down) / up - 1;
    int64_t total = 0;
    bool moves = false;
    std::vector<std::pair<int64_t, int>> ranges(n);
    for (int i = 0; i < n; ++i) {
        const int64_t n0 = samples_before[i], cnt = block_counts[i];
        if (n0 < 0 || cnt < 0 || block_offsets[i] < 0 || cnt > blocks_floats || block_offsets[i] > blocks_floats - cnt)
            return STREAM_FAIL(ASR_ERR_INVALID, "stream %d: block of %lld samples at %lld (after %lld) "
                        "outside the %lld-float buffer", i, (long long)cnt, (long long)block_offsets[i], (long long)n0,
                        (long long)blocks_floats);
        if (n0 > max_count || cnt > max_count - n0)
            return STREAM_FAIL(ASR_ERR_INVALID, "stream %d: %lld + %lld samples x %d overflow", i,
                        (long long)n0, (long long)cnt, up);
        if (state_offsets[i] < 0 || state_cap > state_floats || state_offsets[i] > state_floats - state_cap)
            return STREAM_FAIL(ASR_ERR_INVALID, "stream %d: state of %lld floats at %lld outside the "
                        "%lld-float buffer", i, (long long)state_cap, (long long)state_offsets[i], (long long)state_floats);
        ranges[i] = {state_offsets[i], i};
        const int64_t n1 = n0 + cnt;
        const int64_t f0 = plan.complete_frames(plan.final_outputs(n0));
        const int64_t f1 = final_flags[i] ? std::max(f0, (int64_t)std::ceil((double)plan.length(n1) / hop))
                                          : plan.complete_frames(plan.final_outputs(n1));
        if (first_frames[i] != f0 || n_new_frames[i] != f1 - f0)
            return STREAM_FAIL(ASR_ERR_INVALID, "stream %d: %lld new frames from frame %lld stated, %lld "
                        "+ %lld samples%s give %lld from %lld", i, (long long)n_new_frames[i], (long long)first_frames[i],
                        (long long)n0, (long long)cnt, final_flags[i] ? " (flushed)" : "", (long long)(f1 - f0),
                        (long long)f0);
        if (out_offsets[i] < 0 || (f1 - f0) > out_floats / n_filters ||
            out_offsets[i] > out_floats - (f1 - f0) * (int64_t)n_filters)
            return STREAM_FAIL(ASR_ERR_INVALID, "stream %d: %lld frames at %lld outside the %lld-float "
                        "output", i, (long long)(f1 - f0), (long long)out_offsets[i], (long long)out_floats);
        asr::StreamRow &r = rows[i];
        r.n0 = n0; r.n1 = n1;
        r.keep0 = n0 > 0 ? plan.keep_from(f0, n0) : 0;
        r.keep1 = plan.keep_from(f1, n1);
        r.first_frame = f0; r.n_new = f1 - f0;
        r.y_len = plan.length(n1);
        r.block_off = block_offsets[i]; r.state_off = state_offsets[i]; r.out_off = out_offsets[i];
        if (r.keep1 < r.keep0 || r.n1 - r.keep1 > state_cap || r.n0 - r.keep0 > state_cap)
            return STREAM_FAIL(ASR_ERR_INVALID, "stream %d: the state would hold samples %lld .. %lld "
                        "(before: from %lld) in %lld floats", i, (long long)r.keep1, (long long)r.n1, (long long)r.keep0,
                        (long long)state_cap);
        moves = moves || cnt > 0 || r.keep1 != r.keep0;
        first[i] = total;
        total += f1 - f0;
    }
    first[n] = total;
    std::sort(ranges.begin(), ranges.end());
    for (int i = 1; i < n; ++i)
        if (ranges[i].first < ranges[i - 1].first + state_cap)
            return STREAM_FAIL(ASR_ERR_INVALID, "the states of streams %d and %d overlap (%lld floats at "
                        "%lld and at %lld)", ranges[i - 1].second, ranges[i].second, (long long)state_cap,
                        (long long)ranges[i - 1].first, (long long)ranges[i].first);
    if (total > 0x7fffffffLL)
        return STREAM_FAIL(ASR_ERR_INVALID, "%lld frames in one call", (long long)total);
    if (total == 0 && !moves) return ASR_OK;
    if (!blocks_dev || !state_dev || (total && !out_dev))
        return STREAM_FAIL(ASR_ERR_INVALID, "NULL argument");
    char *t = tab.data() + b_first + b_rows;
    memcpy(t, window, b_win);
    memcpy(t + b_win, fb_start, b_i);
    memcpy(t + b_win + b_i, fb_len, b_i);
    memcpy(t + b_win + 2 * b_i, off.data(), b_i);
    if (total_w) memcpy(t + b_win + 3 * b_i, fb_weights, (size_t)total_w * 4);
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    int rc = join_views(ctx);
    if (rc != ASR_OK) return rc;
    if (tab.size() > ctx->stream_ws_bytes) {
        ASR_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->stream_ws) ASR_HIP(ctx, hipFree(ctx->stream_ws));
        ctx->stream_ws = nullptr; ctx->stream_ws_bytes = 0;
        ASR_HIP(ctx, hipMalloc(&ctx->stream_ws, tab.size()));
        ctx->stream_ws_bytes = tab.size();
    }
    // the taps stay on the device from call to call: a stream pushes the same table every time (82 KB at 48 kHz)
    const size_t n_taps = native ? 0 : (size_t)up * taps_per_phase;
    if (n_taps && (ctx->stream_taps_host.size() != n_taps ||
                   memcmp(ctx->stream_taps_host.data(), taps_phase_major, n_taps * 8) != 0)) {
        ASR_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->stream_taps) ASR_HIP(ctx, hipFree(ctx->stream_taps));
        ctx->stream_taps = nullptr; ctx->stream_taps_host.clear();
        ASR_HIP(ctx, hipMalloc((void **)&ctx->stream_taps, n_taps * 8));
        ASR_HIP(ctx, hipMemcpy(ctx->stream_taps, taps_phase_major, n_taps * 8, hipMemcpyHostToDevice));
        ctx->stream_taps_host.assign(taps_phase_major, taps_phase_major + n_taps);
    }
    if (fft) {                                                      // the twiddle table, whichever FFT call came first
        rc = specfft_workspace(ctx, specfft_twiddles().size() * 4);
        if (rc != ASR_OK) return rc;
    }
    char *d = (char *)ctx->stream_ws;
    const int64_t *d_first = (const int64_t *)d;
    const asr::StreamRow *d_rows = (const asr::StreamRow *)(d + b_first);
    const float *d_win = (const float *)(d + b_first + b_rows);
    const int32_t *d_start = (const int32_t *)(d + b_first + b_rows + b_win), *d_len = d_start + n_filters,
                  *d_off = d_len + n_filters;
    const float *d_w = (const float *)(d + b_first + b_rows + b_win + 3 * b_i);
    hipError_t e = hipMemcpyAsync(d, tab.data(), tab.size(), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && total) {
        const asr::StreamResample r{up, down, plan.half, plan.T, (int)span64, round_int16 ? 1 : 0,
                                    native ? nullptr : ctx->stream_taps};
        if (fft) {
            // 5 passes of 1024 complex values at about 8.5 FLOP per value, the post-pass, the filterbank, the resampler
            ProfScope ps(ctx, "audio_stream_fft_frames", 0,
                         (5.0 * 1024 * 8.5 + 1024 * 16.0 + 2.0 * total_w + (native ? 0.0 : 2.0 * taps_per_phase * frame_size)) *
                             (double)total,
                         4.0 * (double)(native ? frame_size : span64) * (double)total);
            e = asr::launch_audio_stream_fft_frames(ctx->stream, blocks_dev, state_dev, d_first, d_rows, n, total, r,
                                                    (const float *)ctx->specfft_ws, d_win, hop, d_start, d_len, d_off, d_w,
                                                    n_filters, mul, add, out_dev, transposed);
        } else {
            ProfScope ps(ctx, "audio_stream_frames", 0,
                         (4.0 * frame_size * (double)max_bin + (native ? 0.0 : 2.0 * taps_per_phase * frame_size)) * (double)total,
                         4.0 * (double)(native ? frame_size : span64) * (double)total);
            // fewer frames than CUs: split a frame's filters over workgroups of about 192 DFT bins each (a lane then sums one
            // bin, not three), balanced by the filters' bin counts, as long as every part of every frame still finds a CU
            asr::StreamParts parts{};
            const int64_t want = std::min<int64_t>({(int64_t)asr::STREAM_MAX_PARTS, (int64_t)(max_bin + 191) / 192,
                                                    (int64_t)ctx->num_cus / total, (int64_t)n_filters});
            const char *env = getenv("ASR_STREAM_PARTS");                   // debug: force the number of parts (1 .. 8)
            const int n_parts = (int)std::max<int64_t>(1, env ? std::min<int64_t>({(int64_t)atoi(env), (int64_t)asr::STREAM_MAX_PARTS,
                                                                                   (int64_t)n_filters}) : want);
            parts.n = n_parts;
            int f = 0;
            for (int p = 0; p < n_parts; ++p) {
                parts.f[p] = f;
                const int64_t upto = total_w * (p + 1) / n_parts;           // weights (= bins read) up to the end of part p
                while (f < n_filters && (p == n_parts - 1 || off[f] + fb_len[f] <= upto || f == parts.f[p])) ++f;
                parts.k0[p] = parts.k1[p] = 0;
                for (int q = parts.f[p]; q < f; ++q) {
                    if (q == parts.f[p] || fb_start[q] < parts.k0[p]) parts.k0[p] = fb_start[q];
                    parts.k1[p] = std::max(parts.k1[p], fb_start[q] + fb_len[q]);
                }
            }
            parts.f[n_parts] = n_filters;
            e = asr::launch_audio_stream_frames(ctx->stream, blocks_dev, state_dev, d_first, d_rows, n, total, r, parts, d_win,
                                                frame_size, hop, max_bin, d_start, d_len, d_off, d_w, n_filters, mul, add,
                                                out_dev, transposed);
        }
    }
    if (e == hipSuccess && moves) {
        ProfScope ps(ctx, "audio_stream_carry", 0, 0.0, 8.0 * (double)plan.state_len() * n);
        e = asr::launch_audio_stream_carry(ctx->stream, blocks_dev, state_dev, d_rows, n);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return STREAM_FAIL(ASR_ERR_HIP, "%s", hipGetErrorString(e));
    return mark_main(ctx);
}
#undef STREAM_FAIL

int asr_audio_stream_push_dev(asr_ctx *ctx, const float *blocks_dev, int64_t blocks_floats, const int64_t *block_offsets,
                              const int64_t *block_counts, const int64_t *samples_before, const int32_t *final_flags,
                              const int64_t *first_frames, const int64_t *n_new_frames, const int64_t *out_offsets,
                              int n_streams, int up, int down, const double *taps_phase_major, int taps_per_phase,
                              int half, int round_int16, float *state_dev, int64_t state_floats,
                              const int64_t *state_offsets, int64_t state_cap, int frame_size, double hop,
                              const float *window, const int32_t *fb_start, const int32_t *fb_len,
                              const float *fb_weights, int n_filters, float mul, float add, int transposed,
                              float *out_dev, int64_t out_floats) {
    return audio_stream_push(ctx, false, "audio_stream_push", blocks_dev, blocks_floats, block_offsets, block_counts,
                             samples_before, final_flags, first_frames, n_new_frames, out_offsets, n_streams, up, down,
                             taps_phase_major, taps_per_phase, half, round_int16, state_dev, state_floats, state_offsets,
                             state_cap, frame_size, hop, window, fb_start, fb_len, fb_weights, n_filters, mul, add,
                             transposed, out_dev, out_floats);
}

int asr_audio_stream_push_fft_dev(asr_ctx *ctx, const float *blocks_dev, int64_t blocks_floats,
                                  const int64_t *block_offsets, const int64_t *block_counts,
                                  const int64_t *samples_before, const int32_t *final_flags, const int64_t *first_frames,
                                  const int64_t *n_new_frames, const int64_t *out_offsets, int n_streams, int up, int down,
                                  const double *taps_phase_major, int taps_per_phase, int half, int round_int16,
                                  float *state_dev, int64_t state_floats, const int64_t *state_offsets, int64_t state_cap,
                                  int frame_size, double hop, const float *window, const int32_t *fb_start,
                                  const int32_t *fb_len, const float *fb_weights, int n_filters, float mul, float add,
                                  int transposed, float *out_dev, int64_t out_floats) {
    return audio_stream_push(ctx, true, "audio_stream_push_fft", blocks_dev, blocks_floats, block_offsets, block_counts,
                             samples_before, final_flags, first_frames, n_new_frames, out_offsets, n_streams, up, down,
                             taps_phase_major, taps_per_phase, half, round_int16, state_dev, state_floats, state_offsets,
                             state_cap, frame_size, hop, window, fb_start, fb_len, fb_weights, n_filters, mul, add,
                             transposed, out_dev, out_floats);
}

int asr_resize_pages_dev(asr_ctx *ctx, const void *pages_dev, int64_t pages_bytes, const int64_t *page_offsets,
                         const int32_t *heights, const int32_t *widths, int n_pages, const int64_t *out_offsets,
                         const int32_t *out_heights, const int32_t *out_widths, void *out_dev, int64_t out_bytes) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n_pages < 0 || pages_bytes < 0 || out_bytes < 0) return fail(ctx, ASR_ERR_INVALID, "resize_pages: bad sizes");
    if (n_pages == 0) return ASR_OK;
    if (!page_offsets || !heights || !widths || !out_offsets || !out_heights || !out_widths)
        return fail(ctx, ASR_ERR_INVALID, "resize_pages: NULL argument");
    const size_t b_first = ((size_t)n_pages + 1) * sizeof(int64_t);
    std::vector<char> tab(b_first + (size_t)n_pages * sizeof(asr::ResizePage));   // tile_first (n + 1) | page table
    int64_t *first = (int64_t *)tab.data();
    asr::ResizePage *table = (asr::ResizePage *)(tab.data() + b_first);
    int64_t tiles = 0;
    double bytes = 0.0;
    for (int p = 0; p < n_pages; ++p) {
        const int64_t h = heights[p], w = widths[p], ho = out_heights[p], wo = out_widths[p];
        if (h < 1 || w < 1 || ho < 1 || wo < 1)
            return fail(ctx, ASR_ERR_INVALID, "resize_pages: page %d: %lld x %lld -> %lld x %lld (every dimension must be at "
                        "least 1)", p, (long long)h, (long long)w, (long long)ho, (long long)wo);
        if (h > asr::RESIZE_MAX_DIM || w > asr::RESIZE_MAX_DIM || ho > asr::RESIZE_MAX_DIM || wo > asr::RESIZE_MAX_DIM ||
            h * w > 0x7fffffffLL)
            return fail(ctx, ASR_ERR_INVALID, "resize_pages: page %d: %lld x %lld -> %lld x %lld (a dimension above %d, or "
                        "2^31 source pixels and more)", p, (long long)h, (long long)w, (long long)ho, (long long)wo,
                        asr::RESIZE_MAX_DIM);
        if (h > asr::RESIZE_MAX_DOWN * ho || w > asr::RESIZE_MAX_DOWN * wo || ho > asr::RESIZE_MAX_UP * h ||
            wo > asr::RESIZE_MAX_UP * w)
            return fail(ctx, ASR_ERR_INVALID, "resize_pages: page %d: %lld x %lld -> %lld x %lld: the ratio in / out per axis "
                        "must lie in [1/%d, %d]", p, (long long)h, (long long)w, (long long)ho, (long long)wo,
                        asr::RESIZE_MAX_UP, asr::RESIZE_MAX_DOWN);
        if (page_offsets[p] < 0 || h * w > pages_bytes || page_offsets[p] > pages_bytes - h * w)
            return fail(ctx, ASR_ERR_INVALID, "resize_pages: page %d (%lld x %lld at %lld) outside the %lld-byte buffer", p,
                        (long long)h, (long long)w, (long long)page_offsets[p], (long long)pages_bytes);
        if (out_offsets[p] < 0 || ho * wo > out_bytes || out_offsets[p] > out_bytes - ho * wo)
            return fail(ctx, ASR_ERR_INVALID, "resize_pages: output %d (%lld x %lld at %lld) outside the %lld-byte buffer", p,
                        (long long)ho, (long long)wo, (long long)out_offsets[p], (long long)out_bytes);
        asr::ResizePage &r = table[p];
        r.src = page_offsets[p];
        r.dst = out_offsets[p];
        r.h_in = (int32_t)h; r.w_in = (int32_t)w; r.h_out = (int32_t)ho; r.w_out = (int32_t)wo;
        r.tiles_x = (int32_t)((wo + asr::RESIZE_TILE_W - 1) / asr::RESIZE_TILE_W);
        r.pad = 0;
        first[p] = tiles;
        tiles += (int64_t)r.tiles_x * ((ho + asr::RESIZE_TILE_H - 1) / asr::RESIZE_TILE_H);
        bytes += (double)(h * w + ho * wo);
    }
    first[n_pages] = tiles;
    if (tiles > 0x7fffffffLL) return fail(ctx, ASR_ERR_INVALID, "resize_pages: %lld tiles in one call", (long long)tiles);
    if (!pages_dev || !out_dev) return fail(ctx, ASR_ERR_INVALID, "resize_pages: NULL argument");
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    int rc = join_views(ctx);
    if (rc != ASR_OK) return rc;
    if (tab.size() > ctx->resize_ws_bytes) {
        ASR_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->resize_ws) ASR_HIP(ctx, hipFree(ctx->resize_ws));
        ctx->resize_ws = nullptr; ctx->resize_ws_bytes = 0;
        ASR_HIP(ctx, hipMalloc(&ctx->resize_ws, tab.size()));
        ctx->resize_ws_bytes = tab.size();
    }
    hipError_t e = hipMemcpyAsync(ctx->resize_ws, tab.data(), tab.size(), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        ProfScope ps(ctx, "resize_pages", 0, 0.0, bytes);
        e = asr::launch_resize_pages(ctx->stream, (const uint8_t *)pages_dev, (uint8_t *)out_dev,
                                     (const int64_t *)ctx->resize_ws,
                                     (const asr::ResizePage *)((const char *)ctx->resize_ws + b_first), n_pages, tiles);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, ASR_ERR_HIP, "resize_pages: %s", hipGetErrorString(e));
    return mark_main(ctx);
}

namespace {

// the shared checks of the two skew calls; on failure the message is set and the code returned
int skew_check_pages(asr_ctx *ctx, const char *who, int64_t pages_bytes, const int64_t *page_offsets, const int32_t *heights,
                     const int32_t *widths, int n_pages) {
    for (int p = 0; p < n_pages; ++p) {
        const int64_t h = heights[p], w = widths[p];
        if (h < 1 || w < 1 || h > asr::SKEW_MAX_DIM || w > asr::SKEW_MAX_DIM)
            return fail(ctx, ASR_ERR_INVALID, "%s: page %d: %lld x %lld (every dimension must lie in [1, %d])", who, p,
                        (long long)h, (long long)w, asr::SKEW_MAX_DIM);
        if (page_offsets[p] < 0 || h * w > pages_bytes || page_offsets[p] > pages_bytes - h * w)
            return fail(ctx, ASR_ERR_INVALID, "%s: page %d (%lld x %lld at %lld) outside the %lld-byte buffer", who, p,
                        (long long)h, (long long)w, (long long)page_offsets[p], (long long)pages_bytes);
    }
    return ASR_OK;
}

int skew_ws_reserve(asr_ctx *ctx, size_t bytes) {
    if (bytes <= ctx->skew_ws_bytes) return ASR_OK;
    ASR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->skew_ws) ASR_HIP(ctx, hipFree(ctx->skew_ws));
    ctx->skew_ws = nullptr; ctx->skew_ws_bytes = 0;
    ASR_HIP(ctx, hipMalloc(&ctx->skew_ws, bytes));
    ctx->skew_ws_bytes = bytes;
    return ASR_OK;
}

size_t skew_align(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

int asr_skew_estimate_dev(asr_ctx *ctx, const void *pages_dev, int64_t pages_bytes, const int64_t *page_offsets,
                          const int32_t *heights, const int32_t *widths, int n_pages, int max_slope, int32_t *slopes,
                          int64_t *scores) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n_pages < 0 || pages_bytes < 0) return fail(ctx, ASR_ERR_INVALID, "skew_estimate: bad sizes");
    if (max_slope < 0 || max_slope > asr::SKEW_MAX_SLOPE)
        return fail(ctx, ASR_ERR_INVALID, "skew_estimate: max_slope %d outside [0, %d]", max_slope, asr::SKEW_MAX_SLOPE);
    if (n_pages == 0) return ASR_OK;
    if (!page_offsets || !heights || !widths || !slopes || !pages_dev)
        return fail(ctx, ASR_ERR_INVALID, "skew_estimate: NULL argument");
    int rc = skew_check_pages(ctx, "skew_estimate", pages_bytes, page_offsets, heights, widths, n_pages);
    if (rc != ASR_OK) return rc;
    const int K = max_slope, n_slopes = 2 * K + 1;
    // chunks of whole pages whose profiles fit ASR_OMR_BUDGET_MB (at least one page each)
    const char *env = getenv("ASR_OMR_BUDGET_MB");
    const size_t budget = (size_t)std::max<int64_t>(env && *env ? atoll(env) : 4096, 1) << 20;
    struct Chunk { int first, n; size_t prof_bytes; int64_t tiles; size_t first_at; };
    std::vector<Chunk> chunks;
    std::vector<asr::SkewPage> table(n_pages);
    std::vector<int64_t> first;                                    // per chunk: n + 1 running tile counts
    double bytes = 0.0;
    for (int p = 0; p < n_pages; ++p) {
        const int h = heights[p], w = widths[p];
        asr::SkewPage &r = table[p];
        r.src = page_offsets[p];
        r.h = h; r.w = w;
        r.tiles_x = (w + asr::SKEW_TILE_W - 1) / asr::SKEW_TILE_W;
        r.dm = (K * (w - 1) + 1024) >> 11;
        r.len = h + 2 * r.dm;
        const size_t prof_bytes = (size_t)n_slopes * r.len * sizeof(uint32_t);
        if (chunks.empty() || chunks.back().prof_bytes + prof_bytes > budget) {
            if (!chunks.empty()) first.push_back(chunks.back().tiles);
            chunks.push_back({p, 0, 0, 0, first.size()});
        }
        Chunk &c = chunks.back();
        r.prof = (int64_t)(c.prof_bytes / sizeof(uint32_t));
        first.push_back(c.tiles);
        c.n += 1;
        c.prof_bytes += prof_bytes;
        c.tiles += (int64_t)r.tiles_x * ((h + asr::SKEW_TILE_H - 1) / asr::SKEW_TILE_H);
        r.pad = 0;
        bytes += (double)h * w;
    }
    first.push_back(chunks.back().tiles);
    size_t max_prof = 0;
    for (const Chunk &c : chunks) {
        if (c.tiles > 0x7fffffffLL) return fail(ctx, ASR_ERR_INVALID, "skew_estimate: %lld tiles in one chunk", (long long)c.tiles);
        max_prof = std::max(max_prof, c.prof_bytes);
    }
    // workspace: running tile counts | page table (one upload) | scores | slopes | profiles of one chunk
    const size_t b_first = first.size() * sizeof(int64_t), b_table = table.size() * sizeof(asr::SkewPage);
    const size_t o_table = b_first, o_scores = skew_align(o_table + b_table),
                 o_slopes = o_scores + (size_t)n_pages * n_slopes * sizeof(int64_t),
                 o_prof = skew_align(o_slopes + (size_t)n_pages * sizeof(int32_t)), total = o_prof + max_prof;
    std::vector<char> blob(o_table + b_table);
    memcpy(blob.data(), first.data(), b_first);
    memcpy(blob.data() + o_table, table.data(), b_table);
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    rc = join_views(ctx);
    if (rc != ASR_OK) return rc;
    rc = skew_ws_reserve(ctx, total);
    if (rc != ASR_OK) return rc;
    char *ws = (char *)ctx->skew_ws;
    int64_t *d_scores = (int64_t *)(ws + o_scores);
    int32_t *d_slopes = (int32_t *)(ws + o_slopes);
    uint32_t *d_prof = (uint32_t *)(ws + o_prof);
    hipError_t e = hipMemcpyAsync(ws, blob.data(), blob.size(), hipMemcpyHostToDevice, ctx->stream);
    for (size_t i = 0; i < chunks.size() && e == hipSuccess; ++i) {
        const Chunk &c = chunks[i];
        const asr::SkewPage *d_table = (const asr::SkewPage *)(ws + o_table) + c.first;
        e = hipMemsetAsync(d_prof, 0, c.prof_bytes, ctx->stream);
        if (e == hipSuccess) {
            ProfScope ps(ctx, "skew_profiles", 0, 0.0, bytes / chunks.size());
            e = asr::launch_skew_profiles(ctx->stream, (const uint8_t *)pages_dev, (const int64_t *)ws + c.first_at, d_table,
                                          c.n, c.tiles, K, d_prof);
        }
        if (e == hipSuccess) {
            ProfScope ps(ctx, "skew_scores", 0, 0.0, (double)c.prof_bytes);
            e = asr::launch_skew_scores(ctx->stream, d_table, c.n, K, d_prof, d_scores + (size_t)c.first * n_slopes,
                                        d_slopes + c.first);
        }
    }
    if (e == hipSuccess) e = hipMemcpyAsync(slopes, d_slopes, (size_t)n_pages * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && scores)
        e = hipMemcpyAsync(scores, d_scores, (size_t)n_pages * n_slopes * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, ASR_ERR_HIP, "skew_estimate: %s", hipGetErrorString(e));
    return mark_main(ctx);
}

int asr_deskew_pages_dev(asr_ctx *ctx, const void *pages_dev, int64_t pages_bytes, const int64_t *page_offsets,
                         const int32_t *heights, const int32_t *widths, int n_pages, const int32_t *slopes, int fill,
                         void *out_dev, int64_t out_bytes) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n_pages < 0 || pages_bytes < 0 || out_bytes < 0) return fail(ctx, ASR_ERR_INVALID, "deskew_pages: bad sizes");
    if (fill < 0 || fill > 255) return fail(ctx, ASR_ERR_INVALID, "deskew_pages: fill %d outside [0, 255]", fill);
    if (n_pages == 0) return ASR_OK;
    if (!page_offsets || !heights || !widths || !slopes || !pages_dev || !out_dev)
        return fail(ctx, ASR_ERR_INVALID, "deskew_pages: NULL argument");
    int rc = skew_check_pages(ctx, "deskew_pages", pages_bytes, page_offsets, heights, widths, n_pages);
    if (rc != ASR_OK) return rc;
    const char *in0 = (const char *)pages_dev, *out0 = (const char *)out_dev;
    if (in0 < out0 + out_bytes && out0 < in0 + pages_bytes)
        return fail(ctx, ASR_ERR_INVALID, "deskew_pages: the output buffer overlaps the pages");
    const size_t b_first = ((size_t)n_pages + 1) * sizeof(int64_t);
    std::vector<char> tab(b_first + (size_t)n_pages * sizeof(asr::DeskewPage));   // tile_first (n + 1) | page table
    int64_t *first = (int64_t *)tab.data();
    asr::DeskewPage *table = (asr::DeskewPage *)(tab.data() + b_first);
    int64_t tiles = 0;
    double bytes = 0.0;
    for (int p = 0; p < n_pages; ++p) {
        const int64_t h = heights[p], w = widths[p];
        if (slopes[p] < -asr::SKEW_MAX_SLOPE || slopes[p] > asr::SKEW_MAX_SLOPE)
            return fail(ctx, ASR_ERR_INVALID, "deskew_pages: page %d: slope %d outside [-%d, %d]", p, slopes[p],
                        asr::SKEW_MAX_SLOPE, asr::SKEW_MAX_SLOPE);
        if (h * w > out_bytes || page_offsets[p] > out_bytes - h * w)
            return fail(ctx, ASR_ERR_INVALID, "deskew_pages: output %d (%lld x %lld at %lld) outside the %lld-byte buffer", p,
                        (long long)h, (long long)w, (long long)page_offsets[p], (long long)out_bytes);
        asr::DeskewPage &r = table[p];
        r.off = page_offsets[p];
        r.h = (int32_t)h; r.w = (int32_t)w; r.k = slopes[p];
        r.tiles_x = (int32_t)((w + asr::DESKEW_TILE_W - 1) / asr::DESKEW_TILE_W);
        first[p] = tiles;
        tiles += (int64_t)r.tiles_x * ((h + asr::DESKEW_TILE_H - 1) / asr::DESKEW_TILE_H);
        bytes += 2.0 * (double)(h * w);
    }
    first[n_pages] = tiles;
    if (tiles > 0x7fffffffLL) return fail(ctx, ASR_ERR_INVALID, "deskew_pages: %lld tiles in one call", (long long)tiles);
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    rc = join_views(ctx);
    if (rc != ASR_OK) return rc;
    rc = skew_ws_reserve(ctx, tab.size());
    if (rc != ASR_OK) return rc;
    hipError_t e = hipMemcpyAsync(ctx->skew_ws, tab.data(), tab.size(), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        ProfScope ps(ctx, "deskew_pages", 0, 0.0, bytes);
        e = asr::launch_deskew_pages(ctx->stream, (const uint8_t *)pages_dev, (uint8_t *)out_dev,
                                     (const int64_t *)ctx->skew_ws,
                                     (const asr::DeskewPage *)((const char *)ctx->skew_ws + b_first), n_pages, tiles, fill);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, ASR_ERR_HIP, "deskew_pages: %s", hipGetErrorString(e));
    return mark_main(ctx);
}

int asr_flatten_pages_dev(asr_ctx *ctx, const void *pages_dev, int64_t pages_bytes, const int64_t *page_offsets,
                          const int32_t *heights, const int32_t *widths, int n_pages, const int32_t *radii, int floor,
                          void *out_dev, int64_t out_bytes, void *background_dev) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n_pages < 0 || pages_bytes < 0 || out_bytes < 0) return fail(ctx, ASR_ERR_INVALID, "flatten_pages: bad sizes");
    if (floor < 0 || floor > 255) return fail(ctx, ASR_ERR_INVALID, "flatten_pages: floor %d outside [0, 255]", floor);
    if (n_pages == 0) return ASR_OK;
    if (!page_offsets || !heights || !widths || !radii || !pages_dev || !out_dev)
        return fail(ctx, ASR_ERR_INVALID, "flatten_pages: NULL argument");
    static_assert(asr::FLATTEN_MAX_DIM == asr::SKEW_MAX_DIM, "skew_check_pages checks the dimensions of both stages");
    int rc = skew_check_pages(ctx, "flatten_pages", pages_bytes, page_offsets, heights, widths, n_pages);
    if (rc != ASR_OK) return rc;
    const char *in0 = (const char *)pages_dev, *out0 = (const char *)out_dev, *bg0 = (const char *)background_dev;
    if (in0 < out0 + out_bytes && out0 < in0 + pages_bytes)
        return fail(ctx, ASR_ERR_INVALID, "flatten_pages: the output buffer overlaps the pages");
    if (bg0 && bg0 < in0 + pages_bytes && in0 < bg0 + out_bytes)
        return fail(ctx, ASR_ERR_INVALID, "flatten_pages: the background buffer overlaps the pages");
    if (bg0 && bg0 < out0 + out_bytes && out0 < bg0 + out_bytes)
        return fail(ctx, ASR_ERR_INVALID, "flatten_pages: the background buffer overlaps the output");
    // chunks of whole pages whose D fit ASR_OMR_BUDGET_MB (at least one page each)
    const char *env = getenv("ASR_OMR_BUDGET_MB");
    const size_t budget = (size_t)std::max<int64_t>(env && *env ? atoll(env) : 4096, 1) << 20;
    struct Chunk { int first, n, max_r; size_t d_bytes; int64_t tiles_d, tiles_p; size_t first_at; };
    std::vector<Chunk> chunks;
    std::vector<asr::FlattenPage> table(n_pages);
    std::vector<int64_t> first_d, first_p;                         // per chunk: n + 1 running tile counts, of D and of the page
    double bytes_d = 0.0, bytes_p = 0.0;
    constexpr int T = asr::FLATTEN_TILE;
    for (int p = 0; p < n_pages; ++p) {
        const int64_t h = heights[p], w = widths[p], r = radii[p];
        if (r < 1 || r > asr::FLATTEN_MAX_RADIUS)
            return fail(ctx, ASR_ERR_INVALID, "flatten_pages: page %d: radius %d outside [1, %d]", p, radii[p],
                        asr::FLATTEN_MAX_RADIUS);
        if (h * w > out_bytes || page_offsets[p] > out_bytes - h * w)
            return fail(ctx, ASR_ERR_INVALID, "flatten_pages: output %d (%lld x %lld at %lld) outside the %lld-byte buffer", p,
                        (long long)h, (long long)w, (long long)page_offsets[p], (long long)out_bytes);
        const int64_t dh = h + 2 * r, dw = w + 2 * r;
        const size_t d_bytes = (size_t)(dh * dw);
        if (chunks.empty() || chunks.back().d_bytes + d_bytes > budget) {
            if (!chunks.empty()) {
                first_d.push_back(chunks.back().tiles_d);
                first_p.push_back(chunks.back().tiles_p);
            }
            chunks.push_back({p, 0, 0, 0, 0, 0, first_d.size()});
        }
        Chunk &c = chunks.back();
        asr::FlattenPage &e = table[p];
        e.off = page_offsets[p];
        e.d = (int64_t)c.d_bytes;
        e.h = (int32_t)h; e.w = (int32_t)w; e.r = (int32_t)r;
        e.tiles_x_d = (int32_t)((dw + T - 1) / T);
        e.tiles_x_p = (int32_t)((w + T - 1) / T);
        e.pad = 0;
        first_d.push_back(c.tiles_d);
        first_p.push_back(c.tiles_p);
        c.n += 1;
        c.max_r = std::max(c.max_r, (int)r);
        c.d_bytes += d_bytes;
        c.tiles_d += (int64_t)e.tiles_x_d * ((dh + T - 1) / T);
        c.tiles_p += (int64_t)e.tiles_x_p * ((h + T - 1) / T);
        bytes_d += (double)(h * w) + (double)d_bytes;
        bytes_p += (double)d_bytes + (double)(h * w) * (background_dev ? 3.0 : 2.0);
    }
    first_d.push_back(chunks.back().tiles_d);
    first_p.push_back(chunks.back().tiles_p);
    size_t max_d = 0;
    for (const Chunk &c : chunks) {
        if (c.tiles_d > 0x7fffffffLL)
            return fail(ctx, ASR_ERR_INVALID, "flatten_pages: %lld tiles in one chunk", (long long)c.tiles_d);
        max_d = std::max(max_d, c.d_bytes);
    }
    // workspace: running tile counts of D | of the pages | page table (one upload) | D of one chunk
    const size_t b_first = first_d.size() * sizeof(int64_t), b_table = table.size() * sizeof(asr::FlattenPage);
    const size_t o_table = 2 * b_first, o_d = skew_align(o_table + b_table), total = o_d + max_d;
    std::vector<char> blob(o_table + b_table);
    memcpy(blob.data(), first_d.data(), b_first);
    memcpy(blob.data() + b_first, first_p.data(), b_first);
    memcpy(blob.data() + o_table, table.data(), b_table);
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    rc = join_views(ctx);
    if (rc != ASR_OK) return rc;
    rc = skew_ws_reserve(ctx, total);
    if (rc != ASR_OK) return rc;
    char *ws = (char *)ctx->skew_ws;
    uint8_t *d_ws = (uint8_t *)(ws + o_d);
    hipError_t e = hipMemcpyAsync(ws, blob.data(), blob.size(), hipMemcpyHostToDevice, ctx->stream);
    for (size_t i = 0; i < chunks.size() && e == hipSuccess; ++i) {
        const Chunk &c = chunks[i];
        const asr::FlattenPage *d_table = (const asr::FlattenPage *)(ws + o_table) + c.first;
        {
            ProfScope ps(ctx, "flatten_dilate", 0, 0.0, bytes_d / chunks.size());
            e = asr::launch_flatten_dilate(ctx->stream, (const uint8_t *)pages_dev, (const int64_t *)ws + c.first_at, d_table,
                                           c.n, c.tiles_d, c.max_r, d_ws);
        }
        if (e == hipSuccess) {
            ProfScope ps(ctx, "flatten_erode", 0, 0.0, bytes_p / chunks.size());
            e = asr::launch_flatten_erode(ctx->stream, (const uint8_t *)pages_dev, d_ws,
                                          (const int64_t *)(ws + b_first) + c.first_at, d_table, c.n, c.tiles_p, c.max_r,
                                          floor, (uint8_t *)out_dev, (uint8_t *)background_dev);
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, ASR_ERR_HIP, "flatten_pages: %s", hipGetErrorString(e));
    return mark_main(ctx);
}

int asr_crop_estimate_dev(asr_ctx *ctx, const void *pages_dev, int64_t pages_bytes, const int64_t *page_offsets,
                          const int32_t *heights, const int32_t *widths, int n_pages, int floor, int share,
                          const int32_t *margins, int32_t *rects, int32_t *status, int32_t *row_counts,
                          int32_t *col_counts) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n_pages < 0 || pages_bytes < 0) return fail(ctx, ASR_ERR_INVALID, "crop_pages: bad sizes");
    if (floor < 0 || floor > 255) return fail(ctx, ASR_ERR_INVALID, "crop_pages: floor %d outside [0, 255]", floor);
    if (share < 1 || share > 1024) return fail(ctx, ASR_ERR_INVALID, "crop_pages: share %d outside [1, 1024]", share);
    if (n_pages == 0) return ASR_OK;
    if (!page_offsets || !heights || !widths || !margins || !rects || !status || !pages_dev)
        return fail(ctx, ASR_ERR_INVALID, "crop_pages: NULL argument");
    static_assert(asr::CROP_MAX_DIM == asr::SKEW_MAX_DIM, "skew_check_pages checks the dimensions of this stage too");
    int rc = skew_check_pages(ctx, "crop_pages", pages_bytes, page_offsets, heights, widths, n_pages);
    if (rc != ASR_OK) return rc;
    const size_t b_first = ((size_t)n_pages + 1) * sizeof(int64_t);
    std::vector<char> tab(b_first + (size_t)n_pages * sizeof(asr::CropPage));     // tile_first (n + 1) | page table
    int64_t *first = (int64_t *)tab.data();
    asr::CropPage *table = (asr::CropPage *)(tab.data() + b_first);
    int64_t tiles = 0, sum_h = 0, sum_w = 0;
    double bytes = 0.0;
    for (int p = 0; p < n_pages; ++p) {
        const int64_t h = heights[p], w = widths[p];
        if (margins[p] < 0) return fail(ctx, ASR_ERR_INVALID, "crop_pages: page %d: margin %d is negative", p, margins[p]);
        asr::CropPage &r = table[p];
        r.off = page_offsets[p];
        r.row_at = sum_h; r.col_at = sum_w;
        r.h = (int32_t)h; r.w = (int32_t)w;
        r.tiles_x = (int32_t)((w + asr::CROP_TILE_W - 1) / asr::CROP_TILE_W);
        r.margin = margins[p];
        first[p] = tiles;
        tiles += (int64_t)r.tiles_x * ((h + asr::CROP_TILE_H - 1) / asr::CROP_TILE_H);
        sum_h += h; sum_w += w;
        bytes += 0.75 * (double)(h * w);
    }
    first[n_pages] = tiles;
    if (tiles > 0x7fffffffLL) return fail(ctx, ASR_ERR_INVALID, "crop_pages: %lld tiles in one call", (long long)tiles);
    // workspace: running tile counts | page table (one upload) | rects | status | row counts | column counts
    const size_t o_rects = skew_align(tab.size()), o_status = o_rects + (size_t)n_pages * 4 * sizeof(int32_t),
                 o_rows = skew_align(o_status + (size_t)n_pages * sizeof(int32_t)),
                 o_cols = o_rows + (size_t)sum_h * sizeof(int32_t), total = o_cols + (size_t)sum_w * sizeof(int32_t);
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    rc = join_views(ctx);
    if (rc != ASR_OK) return rc;
    rc = skew_ws_reserve(ctx, total);
    if (rc != ASR_OK) return rc;
    char *ws = (char *)ctx->skew_ws;
    const asr::CropPage *d_table = (const asr::CropPage *)(ws + b_first);
    int32_t *d_rects = (int32_t *)(ws + o_rects), *d_status = (int32_t *)(ws + o_status);
    int32_t *d_rows = (int32_t *)(ws + o_rows), *d_cols = (int32_t *)(ws + o_cols);
    hipError_t e = hipMemcpyAsync(ws, tab.data(), tab.size(), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_rows, 0, total - o_rows, ctx->stream);
    if (e == hipSuccess) {
        ProfScope ps(ctx, "crop_counts", 0, 0.0, bytes);
        e = asr::launch_crop_counts(ctx->stream, (const uint8_t *)pages_dev, (const int64_t *)ws, d_table, n_pages, tiles,
                                    floor, d_rows, d_cols);
    }
    if (e == hipSuccess) {
        ProfScope ps(ctx, "crop_rects", 0, 0.0, (double)(total - o_rows));
        e = asr::launch_crop_rects(ctx->stream, d_table, n_pages, share, d_rows, d_cols, d_rects, d_status);
    }
    if (e == hipSuccess)
        e = hipMemcpyAsync(rects, d_rects, (size_t)n_pages * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(status, d_status, (size_t)n_pages * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && row_counts)
        e = hipMemcpyAsync(row_counts, d_rows, (size_t)sum_h * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && col_counts)
        e = hipMemcpyAsync(col_counts, d_cols, (size_t)sum_w * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, ASR_ERR_HIP, "crop_pages: %s", hipGetErrorString(e));
    return mark_main(ctx);
}

int asr_crop_pages_dev(asr_ctx *ctx, const void *pages_dev, int64_t pages_bytes, const int64_t *page_offsets,
                       const int32_t *heights, const int32_t *widths, int n_pages, const int32_t *rects,
                       const int64_t *out_offsets, void *out_dev, int64_t out_bytes) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n_pages < 0 || pages_bytes < 0 || out_bytes < 0) return fail(ctx, ASR_ERR_INVALID, "crop_pages: bad sizes");
    if (n_pages == 0) return ASR_OK;
    if (!page_offsets || !heights || !widths || !rects || !out_offsets || !pages_dev || !out_dev)
        return fail(ctx, ASR_ERR_INVALID, "crop_pages: NULL argument");
    int rc = skew_check_pages(ctx, "crop_pages", pages_bytes, page_offsets, heights, widths, n_pages);
    if (rc != ASR_OK) return rc;
    const char *in0 = (const char *)pages_dev, *out0 = (const char *)out_dev;
    if (in0 < out0 + out_bytes && out0 < in0 + pages_bytes)
        return fail(ctx, ASR_ERR_INVALID, "crop_pages: the output buffer overlaps the pages");
    const size_t b_first = ((size_t)n_pages + 1) * sizeof(int64_t);
    std::vector<char> tab(b_first + (size_t)n_pages * sizeof(asr::CropCopy));     // tile_first (n + 1) | rect table
    int64_t *first = (int64_t *)tab.data();
    asr::CropCopy *table = (asr::CropCopy *)(tab.data() + b_first);
    int64_t tiles = 0;
    double bytes = 0.0;
    for (int p = 0; p < n_pages; ++p) {
        const int64_t h = heights[p], w = widths[p];
        const int64_t r0 = rects[4 * p], r1 = rects[4 * p + 1], c0 = rects[4 * p + 2], c1 = rects[4 * p + 3];
        if (r0 < 0 || r0 >= r1 || r1 > h || c0 < 0 || c0 >= c1 || c1 > w)
            return fail(ctx, ASR_ERR_INVALID, "crop_pages: page %d: rect rows [%lld, %lld) columns [%lld, %lld) of a "
                        "%lld x %lld page (0 <= r0 < r1 <= H, 0 <= c0 < c1 <= W)", p, (long long)r0, (long long)r1,
                        (long long)c0, (long long)c1, (long long)h, (long long)w);
        const int64_t ch = r1 - r0, cw = c1 - c0;
        if (out_offsets[p] < 0 || ch * cw > out_bytes || out_offsets[p] > out_bytes - ch * cw)
            return fail(ctx, ASR_ERR_INVALID, "crop_pages: output %d (%lld x %lld at %lld) outside the %lld-byte buffer", p,
                        (long long)ch, (long long)cw, (long long)out_offsets[p], (long long)out_bytes);
        asr::CropCopy &r = table[p];
        r.src = page_offsets[p] + r0 * w + c0;
        r.dst = out_offsets[p];
        r.stride = (int32_t)w;
        r.h = (int32_t)ch; r.w = (int32_t)cw;
        r.pad = 0;
        first[p] = tiles;
        tiles += (ch + asr::CROP_COPY_ROWS - 1) / asr::CROP_COPY_ROWS;
        bytes += 2.0 * (double)(ch * cw);
    }
    first[n_pages] = tiles;
    if (tiles > 0x7fffffffLL) return fail(ctx, ASR_ERR_INVALID, "crop_pages: %lld tiles in one call", (long long)tiles);
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    rc = join_views(ctx);
    if (rc != ASR_OK) return rc;
    rc = skew_ws_reserve(ctx, tab.size());
    if (rc != ASR_OK) return rc;
    hipError_t e = hipMemcpyAsync(ctx->skew_ws, tab.data(), tab.size(), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        ProfScope ps(ctx, "crop_copy", 0, 0.0, bytes);
        e = asr::launch_crop_copy(ctx->stream, (const uint8_t *)pages_dev, (uint8_t *)out_dev, (const int64_t *)ctx->skew_ws,
                                  (const asr::CropCopy *)((const char *)ctx->skew_ws + b_first), n_pages, tiles);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, ASR_ERR_HIP, "crop_pages: %s", hipGetErrorString(e));
    return mark_main(ctx);
}

int asr_score_map_dev(asr_ctx *ctx, const double *maps_dev, int64_t maps_doubles, const int32_t *heights,
                      const int32_t *widths, int n_pages, const int32_t *page_in_piece, const int32_t *systems,
                      const int32_t *system_index, int n_systems, int n_pieces, double threshold, int min_rows, int tol,
                      int max_lines, int32_t *measures, int32_t *piece_first, int32_t *n_measures,
                      int32_t *overflow_system) {
    if (!ctx) return ASR_ERR_INVALID;
    if (n_pages < 0 || n_systems < 0 || n_pieces < 0 || maps_doubles < 0)
        return fail(ctx, ASR_ERR_INVALID, "score_map: bad sizes");
    if (min_rows < 1 || tol < 0 || max_lines < 0 || threshold != threshold)
        return fail(ctx, ASR_ERR_INVALID, "score_map: min_rows %d (>= 1) / tol %d (>= 0) / max_lines %d (>= 0) / threshold %g",
                    min_rows, tol, max_lines, threshold);
    if (!piece_first || !n_measures || !overflow_system) return fail(ctx, ASR_ERR_INVALID, "score_map: NULL argument");
    if (n_systems == 0) {
        for (int q = 0; q <= n_pieces; ++q) piece_first[q] = 0;
        *n_measures = 0;
        *overflow_system = -1;
        return ASR_OK;
    }
    if (!maps_dev || !heights || !widths || !page_in_piece || !systems || !system_index || !measures)
        return fail(ctx, ASR_ERR_INVALID, "score_map: NULL argument");
    std::vector<int64_t> map_off((size_t)n_pages + 1, 0);
    for (int p = 0; p < n_pages; ++p) {
        if (heights[p] < 0 || widths[p] < 0)
            return fail(ctx, ASR_ERR_INVALID, "score_map: page %d is %d x %d", p, heights[p], widths[p]);
        map_off[p + 1] = map_off[p] + (int64_t)heights[p] * widths[p];
        if (map_off[p + 1] > maps_doubles)
            return fail(ctx, ASR_ERR_INVALID, "score_map: map %d (%d x %d at %lld) outside the %lld-double buffer", p,
                        heights[p], widths[p], (long long)map_off[p], (long long)maps_doubles);
    }
    // workspace: system table (one upload) | flags | n_lines | lines | piece_count | sys_first | piece_first | header | rows
    std::vector<asr::ScoreSystem> table(n_systems);
    int64_t chunks = 0;
    double elements = 0.0;
    for (int i = 0; i < n_systems; ++i) {
        const int32_t *t = systems + (size_t)i * 8;
        const int32_t page = t[0], r0 = t[1], r1 = t[2], c0 = t[3], c1 = t[4], piece = t[6], x0 = t[7];
        if (page < 0 || page >= n_pages || piece < 0 || piece >= n_pieces)
            return fail(ctx, ASR_ERR_INVALID, "score_map: system %d names page %d / piece %d", i, page, piece);
        if (i > 0 && piece < systems[(size_t)(i - 1) * 8 + 6])
            return fail(ctx, ASR_ERR_INVALID, "score_map: system %d of piece %d follows one of piece %d", i, piece,
                        systems[(size_t)(i - 1) * 8 + 6]);
        if (r0 < 0 || r1 <= r0 || r1 > heights[page] || c0 < 0 || c1 <= c0 || c1 > widths[page])
            return fail(ctx, ASR_ERR_INVALID, "score_map: system %d rows [%d, %d), columns [%d, %d) do not fit page %d "
                        "(%d x %d)", i, r0, r1, c0, c1, page, heights[page], widths[page]);
        if (x0 < 0 || (int64_t)x0 + (c1 - c0) > 0x7fffffffLL)
            return fail(ctx, ASR_ERR_INVALID, "score_map: system %d at strip column %d", i, x0);
        asr::ScoreSystem &s = table[i];
        s.map = map_off[page] + (int64_t)r0 * widths[page] + c0;
        s.chunk_first = chunks;
        s.stride = widths[page];
        s.rows = r1 - r0; s.width = c1 - c0;
        s.r0 = r0; s.r1 = r1; s.c0 = c0;
        s.page = page_in_piece[page]; s.system = system_index[i];
        s.piece = piece; s.x0 = x0;
        chunks += (s.width + asr::SCORE_MAP_CHUNK - 1) / asr::SCORE_MAP_CHUNK;
        elements += (double)s.rows * s.width;
    }
    const int64_t cap_rows = (int64_t)n_systems * ((int64_t)max_lines + 1);
    if (chunks > 0x7fffffffLL || cap_rows * 8 > 0x7fffffffLL)
        return fail(ctx, ASR_ERR_INVALID, "score_map: %lld column chunks / %lld rows in one call", (long long)chunks,
                    (long long)cap_rows);
    const size_t b_table = table.size() * sizeof(asr::ScoreSystem);
    const size_t o_flags = skew_align(b_table), o_nlines = skew_align(o_flags + (size_t)chunks * 8),
                 o_lines = skew_align(o_nlines + (size_t)n_systems * 4),
                 o_pcount = skew_align(o_lines + (size_t)n_systems * (size_t)std::max(max_lines, 1) * 4),
                 o_sfirst = skew_align(o_pcount + (size_t)std::max(n_pieces, 1) * 4),
                 o_pfirst = skew_align(o_sfirst + (size_t)n_systems * 4),
                 o_header = o_pfirst + ((size_t)n_pieces + 1) * 4, o_rows = skew_align(o_header + 8),
                 total = o_rows + (size_t)cap_rows * 32;
    ASR_HIP(ctx, hipSetDevice(ctx->cfg.device));
    int rc = join_views(ctx);
    if (rc != ASR_OK) return rc;
    rc = skew_ws_reserve(ctx, total);
    if (rc != ASR_OK) return rc;
    char *ws = (char *)ctx->skew_ws;
    const asr::ScoreSystem *d_table = (const asr::ScoreSystem *)ws;
    unsigned long long *d_flags = (unsigned long long *)(ws + o_flags);
    int32_t *d_nlines = (int32_t *)(ws + o_nlines), *d_lines = (int32_t *)(ws + o_lines);
    int32_t *d_pfirst = (int32_t *)(ws + o_pfirst), *d_header = (int32_t *)(ws + o_header);
    hipError_t e = hipMemcpyAsync(ws, table.data(), b_table, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        ProfScope ps(ctx, "score_map_counts", 0, 0.0, 8.0 * elements);
        e = asr::launch_score_map_counts(ctx->stream, maps_dev, d_table, n_systems, chunks, threshold, min_rows, d_flags);
    }
    if (e == hipSuccess) {
        ProfScope ps(ctx, "score_map_lines", 0, 0.0, 8.0 * (double)chunks);
        e = asr::launch_score_map_lines(ctx->stream, d_table, n_systems, d_flags, tol, max_lines, d_nlines, d_lines);
    }
    if (e == hipSuccess) {
        ProfScope ps(ctx, "score_map_table", 0, 0.0, 32.0 * (double)n_systems);
        e = asr::launch_score_map_table(ctx->stream, d_table, n_systems, n_pieces, max_lines, d_nlines, d_lines,
                                        (int32_t *)(ws + o_pcount), d_pfirst, d_header, (int32_t *)(ws + o_sfirst),
                                        (int32_t *)(ws + o_rows));
    }
    std::vector<int32_t> head((size_t)n_pieces + 3);                       // piece_first (n + 1) | header (2): adjacent
    if (e == hipSuccess)
        e = hipMemcpyAsync(head.data(), d_pfirst, head.size() * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess && head[(size_t)n_pieces + 2] < 0 && head[(size_t)n_pieces + 1] > 0) {
        e = hipMemcpyAsync(measures, ws + o_rows, (size_t)head[(size_t)n_pieces + 1] * 32, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
    if (e != hipSuccess) return fail(ctx, ASR_ERR_HIP, "score_map: %s", hipGetErrorString(e));
    memcpy(piece_first, head.data(), ((size_t)n_pieces + 1) * 4);
    *n_measures = head[(size_t)n_pieces + 1];
    *overflow_system = head[(size_t)n_pieces + 2];
    return mark_main(ctx);
}
