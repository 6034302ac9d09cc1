// Part of libfxcorr's single translation unit: included by fxcorr.hip (not a stand-alone header).
// The rows tools' drivers -- delays, fringe fit, gain solve, detector, averager, beamformer, spectral kurtosis, dedispersion, boxcar search -- and
// the host helpers they share.
// The entry points that check a call's arguments and hand it to a driver are in fxcorr.hip.
#pragma once

namespace {

// The blocks of a call's workspace, listed once in their order: take() gives the offset of the next block and moves on by
// exactly `bytes` (a caller that wants a block on a 256-byte boundary rounds with up256 itself), total() is what ensure_ws
// is asked for, ws_at() the block's address once the workspace stands.
struct WsCarver {
    int64_t off = 0;
    int64_t take(int64_t bytes) { return (off += bytes) - bytes; }
    int64_t total() const { return off; }
};
template <typename T>
T* ws_at(const fxc_plan* p, int64_t off) { return reinterpret_cast<T*>(static_cast<char*>(p->d_ws.get()) + off); }

// Forward (sign -1, kernel exp(-2 pi i ...) like cp.fft.fft) or inverse (+1, un-normalised) transform of n_lines adjacent lines
// of len = 2^lg points in buf[0], ping-pong with buf[1]: radix-16 passes, then one radix-8 / 4 / 2 pass for the remaining bits
// of lg; at most kGridMax lines (gridDim.y) a launch.  -> the index of the buffer that holds the result
int stockham_lines(fxc_plan* p, cf* const buf[2], int64_t n_lines, int64_t len, int lg, double sign) {
    int cur = 0;
    int64_t pp = 1;
    for (int bits = lg; bits > 0;) {
        const int r = bits >= 4 ? 4 : bits;
        for (int64_t l0 = 0; l0 < n_lines; l0 += kGridMax) {
            const dim3 grid(grid_for(len >> r, 256, p->cu_count), (unsigned)std::min<int64_t>(kGridMax, n_lines - l0));
            const cf* in = buf[cur] + l0 * len;
            cf* out = buf[cur ^ 1] + l0 * len;
            if (r == 4) hipLaunchKernelGGL(stockham_stage_kernel<16>, grid, dim3(256), 0, p->stream, in, out, len, pp, sign);
            else if (r == 3) hipLaunchKernelGGL(stockham_stage_kernel<8>, grid, dim3(256), 0, p->stream, in, out, len, pp, sign);
            else if (r == 2) hipLaunchKernelGGL(stockham_stage_kernel<4>, grid, dim3(256), 0, p->stream, in, out, len, pp, sign);
            else hipLaunchKernelGGL(stockham_stage_kernel<2>, grid, dim3(256), 0, p->stream, in, out, len, pp, sign);
        }
        pp <<= r;
        bits -= r;
        cur ^= 1;
    }
    return cur;
}

// n rows of `width` elements, dst_stride / src_stride elements from one row to the next, between host and device: a slab of
// some whole baselines of some chunks of rows, weights or prior
template <typename T>
hipError_t copy_rows(fxc_plan* p, T* dst, int64_t dst_stride, const T* src, int64_t src_stride, int64_t width, int64_t n, hipMemcpyKind kind) {
    return hipMemcpy2DAsync(dst, (size_t)dst_stride * sizeof(T), src, (size_t)src_stride * sizeof(T), (size_t)width * sizeof(T), (size_t)n,
                            kind, p->stream);
}

// a call's result words to the host: the one copy and the one synchronisation that end it
int read_back(fxc_plan* p, const void* dev, int64_t bytes, std::vector<char>& host) {
    host.resize((size_t)bytes);
    FXC_HIP(p, hipMemcpyAsync(host.data(), dev, (size_t)bytes, hipMemcpyDeviceToHost, p->stream));
    FXC_HIP(p, hipStreamSynchronize(p->stream));
    return FXC_OK;
}

// the peak's offset from the middle of three magnitudes, in cells: a parabola through their logarithms (effex.py:619-625)
double peak_offset(double a, double b, double c) {
    const double la = std::log(a), lb = std::log(b), lc = std::log(c);
    return 0.5 * (la - lc) / (la - 2.0 * lb + lc);
}

// 0 .. n - 1 without ref: the order of the results of a call that measures against antenna (stream) ref
std::vector<int> all_but(int ref, int n) {
    std::vector<int> v;
    for (int i = 0; i < n; ++i) if (i != ref) v.push_back(i);
    return v;
}

// Delays of n_streams equal-length streams against streams[ref] (effex.py:583-627 for each pair (ref, s)): delays_s[s] is
// (n - (imax + delta)) / rate of the correlation f_ref * conj(f_s), delays_s[ref] = 0.  The reference's spectrum is formed once;
// the other streams go through in batches (k_delay.h) of as many as fit the workspace target (FXC_WS_MB), every batch's
// arg-max words into one result block: one copy to the host and one synchronisation for the whole call.
int estimate_delays_batch(fxc_plan* p, const cf* const* streams, int n_streams, int ref, int64_t n, int mem_kind, double rate,
                          double* delays_s) {
    if (n < 2 || n > (1ll << 28)) return fail(p, FXC_ERR_ARG, "n=%lld out of range", (long long)n);
    if (!(rate > 0.0)) return fail(p, FXC_ERR_ARG, "rate must be > 0");
    if (const int rc = bad_mem_kind(p, mem_kind)) return rc;
    if (n_streams < 2 || ref < 0 || ref >= n_streams) return fail(p, FXC_ERR_ARG, "ref=%d outside [0, %d)", ref, n_streams);
    FXC_DEVICE(p, p->device);
    int lg = 1;
    while ((1ll << lg) < 2 * n) ++lg;
    const int64_t len = 1ll << lg;
    // workspace: the reference's two transform buffers, two per stream of a batch, staging for host inputs (the reference
    // and a batch), the result words of every stream (best[n_streams], then out3[n_streams][3])
    const int64_t buf_bytes = len * (int64_t)sizeof(cf);
    const int64_t stage_one = mem_kind == FXC_MEM_HOST ? up256(n * (int64_t)sizeof(cf)) : 0;
    const int64_t res_bytes = up256((int64_t)n_streams * (8 + 3 * (int64_t)sizeof(cf)));
    const int64_t fixed = 2 * buf_bytes + stage_one + res_bytes, per_stream = 2 * buf_bytes + stage_one;
    const int n_other = n_streams - 1;
    const int64_t fit = (ws_target() - fixed) / per_stream;
    const int batch = (int)std::max<int64_t>(1, std::min<int64_t>(fit, std::min(n_other, kDelayBatch)));
    WsCarver ws;
    const int64_t o_rbuf[2] = {ws.take(buf_bytes), ws.take(buf_bytes)};
    const int64_t o_sbuf[2] = {ws.take(batch * buf_bytes), ws.take(batch * buf_bytes)};
    const int64_t o_stage = ws.take((1 + batch) * stage_one), o_res = ws.take(res_bytes);      // stage: [1 + batch][stage_one]
    if (const int rc = ensure_ws(p, ws.total())) return rc;
    cf* rbuf[2] = {ws_at<cf>(p, o_rbuf[0]), ws_at<cf>(p, o_rbuf[1])};
    cf* sbuf[2] = {ws_at<cf>(p, o_sbuf[0]), ws_at<cf>(p, o_sbuf[1])};
    cf* stage = ws_at<cf>(p, o_stage);
    unsigned long long* best = ws_at<unsigned long long>(p, o_res);
    cf* out3 = ws_at<cf>(p, o_res + 8 * (int64_t)n_streams);
    const int64_t stage_elems = stage_one / (int64_t)sizeof(cf);
    // stream s as the device sees it: staged into row `row` of the staging block when it is host memory
    auto device_stream = [&](int s, int row) -> const cf* {
        if (mem_kind == FXC_MEM_DEVICE) return streams[s];
        cf* st = stage + row * stage_elems;
        const hipError_t e = hipMemcpyAsync(st, streams[s], (size_t)n * sizeof(cf), hipMemcpyHostToDevice, p->stream);
        return e == hipSuccess ? st : nullptr;
    };
    const int g_len = grid_for(len, 256, p->cu_count);
    FXC_HIP(p, hipMemsetAsync(best, 0, 8 * (size_t)n_streams, p->stream));
    DelayStreams xs{};
    xs.x[0] = device_stream(ref, 0);
    if (!xs.x[0]) return fail(p, FXC_ERR_HIP, "host staging copy failed");
    hipLaunchKernelGGL(delay_pad_kernel, dim3(g_len, 1), dim3(256), 0, p->stream, xs, rbuf[0], n, len);
    const cf* f_ref = rbuf[stockham_lines(p, rbuf, 1, len, lg, -1.0)];
    const std::vector<int> others = all_but(ref, n_streams);
    for (int b0 = 0; b0 < n_other; b0 += batch) {
        const int nb = std::min(batch, n_other - b0);
        for (int q = 0; q < nb; ++q) {
            xs.x[q] = device_stream(others[b0 + q], 1 + q);
            if (!xs.x[q]) return fail(p, FXC_ERR_HIP, "host staging copy failed");
        }
        hipLaunchKernelGGL(delay_pad_kernel, dim3(g_len, nb), dim3(256), 0, p->stream, xs, sbuf[0], n, len);
        const int cur = stockham_lines(p, sbuf, nb, len, lg, -1.0);
        hipLaunchKernelGGL(mul_conj_kernel, dim3(g_len, nb), dim3(256), 0, p->stream, f_ref, sbuf[cur], len);   // f_ref * conj(f_s)
        cf* inv[2] = {sbuf[cur], sbuf[cur ^ 1]};      // back to lags, un-normalised: the peak fit is scale free
        cf* const r = inv[stockham_lines(p, inv, nb, len, lg, 1.0)];
        // the batch's streams are consecutive in `others`, so their result words are too
        hipLaunchKernelGGL(delay_argmax_kernel, dim3(grid_for(2 * n, 256, p->cu_count), nb), dim3(256), 0, p->stream, r, best + b0, n,
                           len);
        hipLaunchKernelGGL(delay_fetch_kernel, dim3(nb), dim3(64), 0, p->stream, r, best + b0, out3 + 3 * (int64_t)b0, n, len);
        FXC_HIP(p, hipGetLastError());
    }
    std::vector<char> h_res;
    if (const int rc = read_back(p, best, res_bytes, h_res)) return rc;
    const unsigned long long* h_best = reinterpret_cast<const unsigned long long*>(h_res.data());
    const cf* h3_all = reinterpret_cast<const cf*>(h_res.data() + 8 * (int64_t)n_streams);
    for (int q = 0; q < n_other; ++q) {
        const cf* h3 = h3_all + 3 * q;
        const int64_t imax = (int64_t)(0xFFFFFFFFull - (h_best[q] & 0xFFFFFFFFull));
        if (imax + 1 >= 2 * n)
            return fail(p, FXC_ERR_STATE, "correlation peak at the last lag (the reference raises IndexError here)");
        const double xprev = std::hypot((double)h3[0].x, (double)h3[0].y);
        const double xbest = std::hypot((double)h3[1].x, (double)h3[1].y);
        const double xnext = std::hypot((double)h3[2].x, (double)h3[2].y);
        delays_s[others[q]] = ((double)n - ((double)imax + peak_offset(xprev, xbest, xnext))) / rate;
    }
    delays_s[ref] = 0.0;
    return FXC_OK;
}

// The argument checks of both fringe fits, in the order that gives each call its code and message; the plain call has neither a
// baselines mode nor a threshold (FXC_FRINGE_REF, 0).  Sets the logarithms of the padded grid.
int check_fringe_fit(fxc_plan* p, const void* rows, int64_t n_chunks, int mem_kind, double bandwidth, double frequency, int ref, int pad,
                     int baselines, double min_snr, const double* delay_s, const double* rate_s_per_chunk, int* lk_log, int* lt_log) {
    if (!p || !rows || !delay_s || !rate_s_per_chunk) return fail(p, FXC_ERR_ARG, "NULL argument");
    if (p->n_ant < 2) return fail(p, FXC_ERR_ARG, "a fringe fit needs 2 or more antennas, the plan has %d", p->n_ant);
    if (ref < 0 || ref >= p->n_ant) return fail(p, FXC_ERR_ARG, "ref=%d outside [0, %d)", ref, p->n_ant);
    if (n_chunks < 2) return fail(p, FXC_ERR_ARG, "n_chunks=%lld: a fringe fit needs 2 or more chunks", (long long)n_chunks);
    if (pad != 1 && pad != 2 && pad != 4 && pad != 8) return fail(p, FXC_ERR_ARG, "pad=%d is not 1, 2, 4 or 8", pad);
    if (!std::isfinite(bandwidth) || !(bandwidth > 0.0)) return fail(p, FXC_ERR_ARG, "bandwidth must be finite and > 0");
    if (!std::isfinite(frequency) || !(frequency > 0.0)) return fail(p, FXC_ERR_ARG, "frequency must be finite and > 0");
    if (const int rc = bad_mem_kind(p, mem_kind)) return rc;
    if (baselines != FXC_FRINGE_REF && baselines != FXC_FRINGE_ALL)
        return fail(p, FXC_ERR_ARG, "baselines=%d is neither FXC_FRINGE_REF nor FXC_FRINGE_ALL", baselines);
    if (!std::isfinite(min_snr) || min_snr < 0.0) return fail(p, FXC_ERR_ARG, "min_snr must be finite and >= 0");
    if (baselines == FXC_FRINGE_REF && min_snr != 0.0)
        return fail(p, FXC_ERR_ARG, "min_snr=%g: the baselines to ref are not selected, min_snr must be 0 with FXC_FRINGE_REF", min_snr);
    if (p->nchan == 1) return fail(p, FXC_ERR_UNSUPPORTED, "a fringe fit needs a frequency axis: nchan is 1");
    *lk_log = *lt_log = 0;
    while ((1ll << *lk_log) < (int64_t)pad * p->nchan) ++*lk_log;
    while (*lt_log < 13 && (1ll << *lt_log) < (int64_t)pad * n_chunks) ++*lt_log;
    if (*lt_log > 12)
        return fail(p, FXC_ERR_UNSUPPORTED, "Lt = pad * n_chunks rounded up to a power of two exceeds 4096 (pad %d, %lld chunks)", pad,
                    (long long)n_chunks);
    if (*lk_log > 16)
        return fail(p, FXC_ERR_UNSUPPORTED, "Lk = pad * nchan rounded up to a power of two exceeds 65536 (pad %d, %d channels)", pad,
                    p->nchan);
    return FXC_OK;
}

// one fit of a fringe_fit_batch call: cross row `row` of the rows, conjugated first where `conj`
struct FringeItem {
    int64_t row;
    int conj;
};
// its result: delay in seconds, rate in seconds per chunk, peak over root power, and the power sum |R|^2 itself
struct FringeFit {
    double delay, rate, snr, power;
};

// row (a, b), a < b, in the baseline order of the results
int64_t cross_row(int a, int b, int n_ant) { return (int64_t)a * (2 * n_ant - a - 1) / 2 + (b - a - 1); }

// The fringe fits of a list of (row, conj) pairs (fxcorr.h fxc_fringe_fit: the baselines to ref; fxc_fringe_fit_weighted: those, or
// every cross row; kernels in k_fringe.h).  The fits go through in batches of as many as fit the workspace target (FXC_WS_MB), the
// staging of host rows and host weights counted: gather (the weighted one where there are weights), frequency transform, time
// transform + peak, stencil; every batch's result words go into one block sized by the list: one copy to the host and one
// synchronisation for the whole call.  fits[i] belongs to items[i]; with zero_guard a fit without power is all 0 (the plain call
// divides by it, as it always has).
int fringe_fit_batch(fxc_plan* p, const cf* rows, const float* weights, int64_t n_chunks, int mem_kind, double bandwidth, double frequency,
                     int lk_log, int lt_log, bool zero_guard, const std::vector<FringeItem>& items, std::vector<FringeFit>& fits) {
    FXC_DEVICE(p, p->device);
    const int nchan = p->nchan, n_items = (int)items.size();
    const int64_t lk = 1ll << lk_log, lt = 1ll << lt_log;
    const int64_t n_rows = p->n_prod;
    const bool host = mem_kind == FXC_MEM_HOST;
    // the time-axis tile: as many adjacent columns (a power of two, 64 at most) as fit the LDS budget beside the twiddles
    int tm_log = 0, pad = 1;
    for (int cand = 6; cand >= 0; --cand) {
        const int64_t tm = 1ll << cand, pd = tm < 32 ? tm : 0;
        if (tm <= lk && (lt * tm + (lt >> 4) * pd + lt) * (int64_t)sizeof(cf) <= kFringeLdsBytes) {
            tm_log = cand;
            pad = (int)pd;
            break;
        }
    }
    const int64_t lds = (lt * (1ll << tm_log) + (lt >> 4) * pad + lt) * (int64_t)sizeof(cf);
    const int first_log = lt_log % 4 ? lt_log % 4 : 4;
    // workspace: two transform buffers [n_chunks][Lk] per fit of a batch, its rows -- and its weights, as many elements -- staged
    // when they are host memory, and the result words of every fit (best[n], stencil[n][5] complex128, part[n][kFringeParts]; with weights wmax[n])
    const int64_t buf_one = n_chunks * lk * (int64_t)sizeof(cf);
    const int64_t stage_one = host ? up256(n_chunks * nchan * (int64_t)sizeof(cf)) : 0;
    const int64_t stage_elems = stage_one / (int64_t)sizeof(cf);
    const int64_t stage_w_one = host && weights ? stage_elems * (int64_t)sizeof(float) : 0;
    const int64_t res_bytes = up256((int64_t)n_items * (8 + 80 + 8 * kFringeParts + (weights ? 4 : 0)));
    const int64_t per_fit = 2 * buf_one + stage_one + stage_w_one;
    const int64_t fit = (ws_target() - res_bytes) / per_fit;
    const int batch = (int)std::max<int64_t>(1, std::min<int64_t>(fit, std::min(n_items, kFringeBatch)));
    WsCarver ws;
    const int64_t o_gbuf[2] = {ws.take(batch * buf_one), ws.take(batch * buf_one)};
    const int64_t o_stage = ws.take(batch * stage_one), o_res = ws.take(res_bytes), o_stage_w = ws.take(batch * stage_w_one);
    if (const int rc = ensure_ws(p, ws.total())) return rc;
    FXC_HIP(p, hipFuncSetAttribute(reinterpret_cast<const void*>(&fringe_time_peak_kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, kFringeLdsBytes));
    cf* gbuf[2] = {ws_at<cf>(p, o_gbuf[0]), ws_at<cf>(p, o_gbuf[1])};
    cf* stage = ws_at<cf>(p, o_stage);
    float* stage_w = ws_at<float>(p, o_stage_w);
    unsigned long long* best = ws_at<unsigned long long>(p, o_res);
    double* stencil = ws_at<double>(p, o_res + 8 * (int64_t)n_items);
    double* part = stencil + 10 * (int64_t)n_items;
    unsigned* wmax = reinterpret_cast<unsigned*>(part + (int64_t)kFringeParts * n_items);      // the largest counted weight, float bits
    FXC_HIP(p, hipMemsetAsync(best, 0, 8 * (size_t)n_items, p->stream));
    if (weights) FXC_HIP(p, hipMemsetAsync(wmax, 0, 4 * (size_t)n_items, p->stream));
    for (int b0 = 0; b0 < n_items; b0 += batch) {
        const int nb = std::min(batch, n_items - b0);
        FringeRows br{};
        for (int q = 0; q < nb; ++q) {
            const int64_t row = items[(size_t)(b0 + q)].row;
            br.conj[q] = items[(size_t)(b0 + q)].conj;
            if (host) {
                // a baseline's staged weights lie like its staged rows: one offset serves both
                br.off[q] = q * stage_elems;
                FXC_HIP(p, copy_rows(p, stage + br.off[q], nchan, rows + row * nchan, n_rows * nchan, nchan, n_chunks, hipMemcpyHostToDevice));
                if (weights)
                    FXC_HIP(p, copy_rows(p, stage_w + br.off[q], nchan, weights + row * nchan, (int64_t)p->n_base * nchan, nchan, n_chunks,
                                         hipMemcpyHostToDevice));
            } else {
                br.off[q] = row * nchan;
            }
        }
        const cf* src = host ? stage : rows;
        const int64_t t_stride = host ? nchan : n_rows * nchan;
        if (weights)
            hipLaunchKernelGGL(fringe_gather_weighted_kernel, dim3(kFringeParts, nb), dim3(kFringeThreads), 0, p->stream, src,
                               host ? stage_w : weights, br, t_stride, host ? (int64_t)nchan : (int64_t)p->n_base * nchan, gbuf[0],
                               part + (int64_t)b0 * kFringeParts, wmax + b0, (int)n_chunks, nchan, lk_log);
        else
            hipLaunchKernelGGL(fringe_gather_kernel, dim3(kFringeParts, nb), dim3(kFringeThreads), 0, p->stream, src, br, t_stride, gbuf[0],
                               part + (int64_t)b0 * kFringeParts, (int)n_chunks, nchan, lk_log);
        // frequency axis: forward Stockham stages over the nb n_chunks rows
        const cf* g = gbuf[stockham_lines(p, gbuf, (int64_t)nb * n_chunks, lk, lk_log, -1.0)];
        hipLaunchKernelGGL(fringe_time_peak_kernel, dim3((unsigned)(lk >> tm_log), nb), dim3(kFringeThreads), (size_t)lds, p->stream, g,
                           best + b0, (int)n_chunks, lk_log, lt_log, tm_log, pad, first_log);
        hipLaunchKernelGGL(fringe_stencil_kernel, dim3(nb), dim3(kFringeThreads), 0, p->stream, g, best + b0,
                           stencil + 10 * (int64_t)b0, (int)n_chunks, lk_log, lt_log);
        FXC_HIP(p, hipGetLastError());
    }
    std::vector<char> h_res;
    if (const int rc = read_back(p, best, res_bytes, h_res)) return rc;
    const unsigned long long* h_best = reinterpret_cast<const unsigned long long*>(h_res.data());
    const double* h_st = reinterpret_cast<const double*>(h_res.data() + 8 * (int64_t)n_items);
    const double* h_part = h_st + 10 * (int64_t)n_items;
    const float* h_wmax = reinterpret_cast<const float*>(h_part + (int64_t)kFringeParts * n_items);
    fits.assign((size_t)n_items, FringeFit{0.0, 0.0, 0.0, 0.0});
    for (int i = 0; i < n_items; ++i) {
        double power = 0.0;
        for (int k = 0; k < kFringeParts; ++k) power += h_part[(int64_t)i * kFringeParts + k];
        FringeFit& f = fits[(size_t)i];
        f.power = power;
        if (zero_guard && power == 0.0) continue;      // nothing counted: delay, rate and snr 0, the peak words are not used
        const unsigned lin = (unsigned)(0xFFFFFFFFull - (h_best[i] & 0xFFFFFFFFull));
        int64_t q = (int64_t)(lin >> lk_log) & (lt - 1), m = (int64_t)lin & (lk - 1);
        double a[5];
        for (int k = 0; k < 5; ++k) a[k] = std::hypot(h_st[(i * 5 + k) * 2], h_st[(i * 5 + k) * 2 + 1]);
        const double peak = a[0];
        if (weights) {
            // the magnitudes as of weights / 2^e, e = floor(log2 of the largest counted weight): exact, and it makes the logarithms
            // -- every bit -- independent of a common power-of-two factor of the weights; e = 0 for weights of 1
            int e;
            std::frexp((double)h_wmax[i], &e);
            for (int k = 0; k < 5; ++k) a[k] = std::ldexp(a[k], 1 - e);
        }
        const double dm = peak_offset(a[1], a[0], a[2]), dq = peak_offset(a[3], a[0], a[4]);
        if (m >= lk / 2) m -= lk;
        if (q >= lt / 2) q -= lt;
        f.delay = ((double)m + dm) * (double)nchan / ((double)lk * bandwidth);
        f.rate = ((double)q + dq) / ((double)lt * frequency);
        f.snr = peak / std::sqrt(power);
    }
    return FXC_OK;
}

// The antennas' delays from the baselines' (fxcorr.h fxc_fringe_fit_weighted, FXC_FRINGE_ALL; float64, on the host).  x[i] = the
// estimate of X_b - X_a of cross row i = (a, b), s[i] its snr, period the range x is known modulo; `used` and the tree's start
// values x0 (reached[a]: antenna a hangs on ref through used baselines) come from fringe_tree.  Unwraps every used baseline between
// reached antennas onto the tree, solves min sum s^2 (X_b - X_a - x)^2 with X_ref = 0 (normal equations in ascending row order,
// Cholesky) and wraps the solution into the principal range; antennas not reached get 0.
void fringe_solve_axis(int n_ant, int ref, const std::vector<double>& x, const std::vector<double>& s, const std::vector<char>& used,
                       const std::vector<char>& reached, const std::vector<double>& x0, double period, double* out) {
    std::vector<int> slot((size_t)n_ant, -1);
    int n = 0;
    for (int a = 0; a < n_ant; ++a) {
        out[a] = 0.0;
        if (reached[(size_t)a] && a != ref) slot[(size_t)a] = n++;
    }
    if (n == 0) return;
    std::vector<double> nm((size_t)n * n, 0.0), y((size_t)n, 0.0);
    int64_t i = 0;
    for (int a = 0; a < n_ant; ++a) {
        for (int b = a + 1; b < n_ant; ++b, ++i) {
            if (!used[(size_t)i] || !reached[(size_t)a] || !reached[(size_t)b]) continue;
            const double d = x[(size_t)i] + period * std::nearbyint((x0[(size_t)b] - x0[(size_t)a] - x[(size_t)i]) / period);
            const double w = s[(size_t)i] * s[(size_t)i];
            const int ia = slot[(size_t)a], ib = slot[(size_t)b];
            if (ia >= 0) {
                nm[(size_t)ia * n + ia] += w;
                y[(size_t)ia] -= w * d;
            }
            if (ib >= 0) {
                nm[(size_t)ib * n + ib] += w;
                y[(size_t)ib] += w * d;
            }
            if (ia >= 0 && ib >= 0) {
                nm[(size_t)ia * n + ib] -= w;
                nm[(size_t)ib * n + ia] -= w;
            }
        }
    }
    // Cholesky nm = L L^T in the lower triangle (the grounded Laplacian of a connected graph is positive definite), then the two
    // triangular solves in place
    for (int j = 0; j < n; ++j) {
        double d = nm[(size_t)j * n + j];
        for (int k = 0; k < j; ++k) d -= nm[(size_t)j * n + k] * nm[(size_t)j * n + k];
        d = std::sqrt(d);
        nm[(size_t)j * n + j] = d;
        for (int r = j + 1; r < n; ++r) {
            double v = nm[(size_t)r * n + j];
            for (int k = 0; k < j; ++k) v -= nm[(size_t)r * n + k] * nm[(size_t)j * n + k];
            nm[(size_t)r * n + j] = v / d;
        }
    }
    for (int r = 0; r < n; ++r) {
        double v = y[(size_t)r];
        for (int k = 0; k < r; ++k) v -= nm[(size_t)r * n + k] * y[(size_t)k];
        y[(size_t)r] = v / nm[(size_t)r * n + r];
    }
    for (int r = n - 1; r >= 0; --r) {
        double v = y[(size_t)r];
        for (int k = r + 1; k < n; ++k) v -= nm[(size_t)k * n + r] * y[(size_t)k];
        y[(size_t)r] = v / nm[(size_t)r * n + r];
    }
    for (int a = 0; a < n_ant; ++a)
        if (slot[(size_t)a] >= 0) {
            const double v = y[(size_t)slot[(size_t)a]];
            out[a] = v - period * std::nearbyint(v / period);
        }
}

// The antenna solution of FXC_FRINGE_ALL from base[n_base][3] = (delay, rate, snr) of every cross row: the baselines of snr >=
// threshold are used; a tree grows from ref by the used baseline of largest snr (ties: the lowest row) that joins a reached antenna
// to one not yet reached, and gives the start values; fringe_solve_axis does the rest for the delays (period pd) and the rates
// (pr).  snr[a] = the root of the sum of snr^2 over the used baselines between reached antennas that touch a; snr[ref] = 0.
void fringe_solve_antennas(int n_ant, int ref, const double* base, double threshold, double pd, double pr, double* delay_s,
                           double* rate_s_per_chunk, double* snr) {
    const int64_t n_base = (int64_t)n_ant * (n_ant - 1) / 2;
    std::vector<double> d((size_t)n_base), r((size_t)n_base), s((size_t)n_base);
    std::vector<char> used((size_t)n_base), reached((size_t)n_ant, 0);
    for (int64_t i = 0; i < n_base; ++i) {
        d[(size_t)i] = base[3 * i];
        r[(size_t)i] = base[3 * i + 1];
        s[(size_t)i] = base[3 * i + 2];
        used[(size_t)i] = s[(size_t)i] >= threshold;
    }
    std::vector<double> d0((size_t)n_ant, 0.0), r0((size_t)n_ant, 0.0);
    reached[(size_t)ref] = 1;
    for (;;) {
        int64_t pick = -1, i = 0;
        int pa = 0, pb = 0;
        for (int a = 0; a < n_ant; ++a)
            for (int b = a + 1; b < n_ant; ++b, ++i)
                if (used[(size_t)i] && reached[(size_t)a] != reached[(size_t)b] && (pick < 0 || s[(size_t)i] > s[(size_t)pick])) {
                    pick = i;
                    pa = a;
                    pb = b;
                }
        if (pick < 0) break;
        if (reached[(size_t)pa]) {
            d0[(size_t)pb] = d0[(size_t)pa] + d[(size_t)pick];
            r0[(size_t)pb] = r0[(size_t)pa] + r[(size_t)pick];
            reached[(size_t)pb] = 1;
        } else {
            d0[(size_t)pa] = d0[(size_t)pb] - d[(size_t)pick];
            r0[(size_t)pa] = r0[(size_t)pb] - r[(size_t)pick];
            reached[(size_t)pa] = 1;
        }
    }
    fringe_solve_axis(n_ant, ref, d, s, used, reached, d0, pd, delay_s);
    fringe_solve_axis(n_ant, ref, r, s, used, reached, r0, pr, rate_s_per_chunk);
    if (snr) {
        std::vector<double> sum((size_t)n_ant, 0.0);
        int64_t i = 0;
        for (int a = 0; a < n_ant; ++a)
            for (int b = a + 1; b < n_ant; ++b, ++i)
                if (used[(size_t)i] && reached[(size_t)a] && reached[(size_t)b]) {
                    sum[(size_t)a] += s[(size_t)i] * s[(size_t)i];
                    sum[(size_t)b] += s[(size_t)i] * s[(size_t)i];
                }
        for (int a = 0; a < n_ant; ++a) snr[a] = a == ref ? 0.0 : std::sqrt(sum[(size_t)a]);
    }
}

// fxc_fringe_fit (not `weighted`: no weights, FXC_FRINGE_REF, no base_out) and fxc_fringe_fit_weighted after their checks: the list of fits, the
// batches, and the outputs from the fits
int fringe_fit_run(fxc_plan* p, const cf* rows, const float* weights, int64_t n_chunks, int mem_kind, double bandwidth, double frequency,
                   int ref, int lk_log, int lt_log, bool weighted, int baselines, double min_snr, double* delay_s, double* rate_s_per_chunk, double* snr,
                   double* base_out) {
    const int n_ant = p->n_ant;
    const int64_t n_base = p->n_base;
    std::vector<FringeItem> items;
    if (baselines == FXC_FRINGE_ALL) {
        for (int64_t i = 0; i < n_base; ++i) items.push_back(FringeItem{i, 0});
    } else {
        for (int b : all_but(ref, n_ant)) items.push_back(FringeItem{cross_row(std::min(ref, b), std::max(ref, b), n_ant), b < ref});
    }
    std::vector<FringeFit> fits;
    if (const int rc = fringe_fit_batch(p, rows, weights, n_chunks, mem_kind, bandwidth, frequency, lk_log, lt_log, weighted, items, fits))
        return rc;
    if (baselines == FXC_FRINGE_ALL) {
        std::vector<double> base((size_t)n_base * 3);
        for (int64_t i = 0; i < n_base; ++i) {
            base[(size_t)(3 * i)] = fits[(size_t)i].delay;
            base[(size_t)(3 * i + 1)] = fits[(size_t)i].rate;
            base[(size_t)(3 * i + 2)] = fits[(size_t)i].snr;
        }
        const double threshold = min_snr > 0.0 ? min_snr : std::sqrt(std::log((double)(1ll << lk_log) * (double)(1ll << lt_log)) + std::log(1000.0));
        fringe_solve_antennas(n_ant, ref, base.data(), threshold, (double)p->nchan / bandwidth, 1.0 / frequency, delay_s, rate_s_per_chunk,
                              snr);
        if (base_out) std::memcpy(base_out, base.data(), base.size() * sizeof(double));
        return FXC_OK;
    }
    if (base_out) std::memset(base_out, 0, (size_t)n_base * 3 * sizeof(double));
    const std::vector<int> others = all_but(ref, n_ant);
    for (size_t i = 0; i < others.size(); ++i) {
        const int b = others[i];
        delay_s[b] = fits[i].delay;
        rate_s_per_chunk[b] = fits[i].rate;
        if (snr) snr[b] = fits[i].snr;
        if (base_out) {
            // as the row (lo, hi) reads: the conjugate's delay and rate are the negatives
            double* o = base_out + 3 * items[i].row;
            o[0] = items[i].conj ? -fits[i].delay : fits[i].delay;
            o[1] = items[i].conj ? -fits[i].rate : fits[i].rate;
            o[2] = fits[i].snr;
        }
    }
    delay_s[ref] = 0.0;
    rate_s_per_chunk[ref] = 0.0;
    if (snr) snr[ref] = 0.0;
    return FXC_OK;
}

// The argument checks of both gain solves, in the order that gives each call its code and message; the plain call has no model.
// Sets an interval of 0 or beyond the chunks to all of them.
int check_solve_gains(fxc_plan* p, const void* rows, int64_t n_chunks, int mem_kind, const void* model, int64_t n_model,
                      int64_t* interval, int ref, int iters, const double* gains_re_im) {
    if (!p || !rows || !gains_re_im) return fail(p, FXC_ERR_ARG, "NULL argument");
    if (n_chunks < 1) return fail(p, FXC_ERR_ARG, "n_chunks=%lld: a gain solve needs 1 or more chunks", (long long)n_chunks);
    if (*interval < 0) return fail(p, FXC_ERR_ARG, "interval=%lld is negative", (long long)*interval);
    if (ref < 0 || ref >= p->n_ant) return fail(p, FXC_ERR_ARG, "ref=%d outside [0, %d)", ref, p->n_ant);
    if (iters < 1 || iters > 1000) return fail(p, FXC_ERR_ARG, "iters=%d outside 1 .. 1000", iters);
    if (const int rc = bad_mem_kind(p, mem_kind)) return rc;
    if (*interval == 0 || *interval > n_chunks) *interval = n_chunks;
    const int64_t n_int = (n_chunks + *interval - 1) / *interval;
    if ((model == nullptr) != (n_model == 0)) return fail(p, FXC_ERR_ARG, "model and n_model=%lld disagree", (long long)n_model);
    if (model && n_model != 1 && n_model != n_int)
        return fail(p, FXC_ERR_ARG, "n_model=%lld is neither 1 nor the number of intervals %lld", (long long)n_model, (long long)n_int);
    if (p->n_ant < 3)
        return fail(p, FXC_ERR_UNSUPPORTED, "a gain solve needs 3 or more antennas, the plan has %d: one baseline closes nothing", p->n_ant);
    if (model) {
        const float* m = static_cast<const float*>(model);
        const int64_t n = 2 * n_model * (int64_t)p->n_base * p->nchan;
        for (int64_t i = 0; i < n; ++i)
            if (!std::isfinite(m[i])) return fail(p, FXC_ERR_ARG, "model value %lld is not finite", (long long)(i / 2));
    }
    return FXC_OK;
}

// The gain solve (fxcorr.h fxc_solve_gains and, `weighted`, fxc_solve_gains_weighted; kernels in k_gains.h).  The workspace holds
// the results of every interval (gains, step), the averaged matrices of a group of intervals (V; weighted: U and D, 24 bytes per
// baseline and bin) and, for host rows, a staging block of cross rows (weighted: with a weight block beside it where there are
// weights); the model of a group of intervals is uploaded once per group (of all intervals once when there is one model).  The
// intervals go through in groups and a group's host chunks in batches, both sized by the workspace target (FXC_WS_MB).  A batch
// continues the sums of the batch before it in V (U, D), so no bit depends on the sizes.  One copy to the host and one
// synchronisation.
int solve_gains_batch(fxc_plan* p, bool weighted, const cf* rows, const float* weights, int64_t n_chunks, int mem_kind, const cf* model,
                      int64_t n_model, int64_t interval, int ref, int iters, double* gains_re_im, double* step) {
    FXC_DEVICE(p, p->device);
    const int n_ant = p->n_ant, nchan = p->nchan, n_base = p->n_base;
    const int64_t n_rows = p->n_prod;
    const int64_t n_int = (n_chunks + interval - 1) / interval;
    // the solve's tile: as many adjacent bins (a power of two) as give every (antenna, bin) a thread and fit the LDS budget
    const int tile_bytes = weighted ? kGainsWeightedTileBytes : kGainsTileBytes;
    const int64_t lds_bin = (int64_t)n_base * tile_bytes + (int64_t)n_ant * kGainsImageBytes;
    int tm_log = 0;
    for (int cand = 6; cand >= 0; --cand) {
        const int64_t tm = 1ll << cand;
        if (tm <= kGainsMaxTile && n_ant * tm <= kGainsThreads && lds_bin * tm <= kGainsLdsBytes) {
            tm_log = cand;
            break;
        }
    }
    const int64_t lds = lds_bin << tm_log;
    const int64_t elems = (int64_t)n_base * nchan;
    const int64_t gains_bytes = n_int * n_ant * nchan * (int64_t)sizeof(cd);
    const int64_t res_bytes = up256(gains_bytes + n_int * nchan * (int64_t)sizeof(double));
    const int64_t model_one = elems * (int64_t)sizeof(cf);
    // per interval: V (U + D), and the interval's own model where there is one per interval; a single model is a fixed part
    const int64_t v_one = elems * tile_bytes + (n_model > 1 ? model_one : 0);
    const int64_t fixed = n_model == 1 ? model_one : 0;
    const int64_t stage_one = elems * (int64_t)(sizeof(cf) + (weights ? sizeof(float) : 0));
    const bool host = mem_kind == FXC_MEM_HOST;
    const int64_t avail = std::max<int64_t>(0, ws_target() - res_bytes - fixed);
    const int64_t group = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(n_int, kGridMax), (host ? avail / 2 : avail) / v_one));
    const int64_t group_chunks = std::min(n_chunks, group * interval);
    const int64_t batch = host ? std::max<int64_t>(1, std::min(group_chunks, (avail - group * v_one) / stage_one)) : 0;
    const int64_t model_slots = n_model > 1 ? group : n_model;
    WsCarver ws;
    const int64_t o_res = ws.take(res_bytes), o_v = ws.take(group * elems * tile_bytes);      // gains, then step; V (U, then D)
    const int64_t o_model = ws.take(model_slots * model_one), o_stage = ws.take(batch * stage_one);      // stage: rows, then weights
    if (const int rc = ensure_ws(p, ws.total())) return rc;
    FXC_HIP(p, hipFuncSetAttribute(weighted ? reinterpret_cast<const void*>(&gains_weighted_solve_kernel)
                                            : reinterpret_cast<const void*>(&gains_solve_kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, kGainsLdsBytes));
    cd* d_gains = ws_at<cd>(p, o_res);
    double* d_step = ws_at<double>(p, o_res + gains_bytes);
    cd* d_v = ws_at<cd>(p, o_v);
    double* d_d = ws_at<double>(p, o_v + group * elems * (int64_t)sizeof(cd));      // weighted only
    cf* d_model = ws_at<cf>(p, o_model);
    cf* stage = ws_at<cf>(p, o_stage);
    float* stage_w = reinterpret_cast<float*>(stage + batch * elems);
    const dim3 block(kGainsThreads);
    const dim3 solve_grid((unsigned)((nchan + (1 << tm_log) - 1) >> tm_log));
    const dim3 solve_block((unsigned)(((n_ant << tm_log) + 63) / 64 * 64));      // weighted
    const unsigned gx = (unsigned)(((nchan + 1) / 2 + kGainsThreads - 1) / kGainsThreads);
    const int64_t model_stride = n_model > 1 ? elems : 0;
    // rows [c_lo, c_hi) at src, c_stride elements a chunk (weights: elems a chunk), into the intervals sa .. sa + n_s - 1
    auto average = [&](const cf* src, int64_t c_stride, const float* w, int64_t c_lo, int64_t c_hi, int64_t sa, int64_t n_s, int64_t s0,
                       const cf* d_m, int vec) {
        const dim3 grid(gx, n_base, (unsigned)n_s);
        if (weighted)
            hipLaunchKernelGGL(gains_weighted_average_kernel, grid, block, 0, p->stream, src, c_stride, w, elems, d_m, model_stride, c_lo, c_hi,
                               interval, n_chunks, sa, s0, d_v, d_d, n_base, nchan, vec);
        else
            hipLaunchKernelGGL(gains_average_kernel, grid, block, 0, p->stream, src, c_stride, c_lo, c_hi, interval, n_chunks, sa, s0, d_v,
                               n_base, nchan, vec);
    };
    if (n_model == 1) FXC_HIP(p, hipMemcpyAsync(d_model, model, (size_t)model_one, hipMemcpyHostToDevice, p->stream));
    for (int64_t s0 = 0; s0 < n_int; s0 += group) {
        const int64_t s1 = std::min(n_int, s0 + group), c0 = s0 * interval, c1 = std::min(n_chunks, s1 * interval);
        if (n_model > 1)
            FXC_HIP(p, hipMemcpyAsync(d_model, model + s0 * elems, (size_t)((s1 - s0) * model_one), hipMemcpyHostToDevice, p->stream));
        const cf* d_m = n_model ? d_model : nullptr;
        if (host) {
            for (int64_t b0 = c0; b0 < c1; b0 += batch) {
                const int64_t b1 = std::min(c1, b0 + batch), sa = b0 / interval, sb = (b1 - 1) / interval;
                FXC_HIP(p, copy_rows(p, stage, elems, rows + b0 * n_rows * nchan, n_rows * nchan, elems, b1 - b0, hipMemcpyHostToDevice));
                if (weights)
                    FXC_HIP(p, hipMemcpyAsync(stage_w, weights + b0 * elems, (size_t)((b1 - b0) * elems) * sizeof(float),
                                              hipMemcpyHostToDevice, p->stream));
                average(stage, elems, weights ? stage_w : nullptr, b0, b1, sa, sb - sa + 1, s0, d_m, (int)(nchan % 2 == 0));
            }
        } else {
            const int vec = nchan % 2 == 0 && reinterpret_cast<uintptr_t>(rows) % 16 == 0 && reinterpret_cast<uintptr_t>(weights) % 8 == 0;
            average(rows + c0 * n_rows * nchan, n_rows * nchan, weights ? weights + c0 * elems : nullptr, c0, c1, s0, s1 - s0, s0, d_m, vec);
        }
        const dim3 grid(solve_grid.x, (unsigned)(s1 - s0));
        if (weighted)
            hipLaunchKernelGGL(gains_weighted_solve_kernel, grid, solve_block, (size_t)lds, p->stream, d_v, d_d, d_gains + s0 * n_ant * nchan,
                               d_step + s0 * nchan, n_ant, nchan, tm_log, ref, iters);
        else
            hipLaunchKernelGGL(gains_solve_kernel, grid, block, (size_t)lds, p->stream, d_v, d_gains + s0 * n_ant * nchan, d_step + s0 * nchan,
                               n_ant, nchan, tm_log, ref, iters);
        FXC_HIP(p, hipGetLastError());
    }
    std::vector<char> h_res;
    if (const int rc = read_back(p, d_gains, res_bytes, h_res)) return rc;
    std::memcpy(gains_re_im, h_res.data(), (size_t)gains_bytes);
    if (step) std::memcpy(step, h_res.data() + gains_bytes, (size_t)(n_int * nchan) * sizeof(double));
    return FXC_OK;
}

// The detector (fxcorr.h fxc_flag_rows; kernels in k_flag.h).  The workspace holds the counts of every window, the level and
// scatter planes of the windows and baselines of one launch and, for host rows, a slab: the rows, the prior and the weights of
// some whole baselines of one window (one strided copy each way).  Slabs and window groups are sized by the workspace target
// (FXC_WS_MB); a column belongs to one launch and a baseline's bins to one slab, so no bit depends on the sizes.
int flag_rows_batch(fxc_plan* p, const cf* rows, const float* prior, int64_t n_chunks, int mem_kind, int64_t window, float time_threshold,
                    float freq_threshold, int half_width, int iters, float* weights, int64_t* counts) {
    FXC_DEVICE(p, p->device);
    const int nchan = p->nchan, n_base = p->n_base;
    const int64_t n_rows = p->n_prod;
    const int64_t n_win = (n_chunks + window - 1) / window;
    // a wave's columns: as many (a power of two, 16 at most) as leave a lane 8 samples of the longest window -- short loops and
    // little LDS a wave, so that many waves share a CU --, 2 where the window is longer than that allows (32 samples at 1024 chunks)
    int q_log = 1;
    for (int cand = kFlagMaxQLog; cand >= 1; --cand) {
        if (((window << cand) + 63) / 64 <= kFlagTargetLaneSamples) {
            q_log = cand;
            break;
        }
    }
    const int plane_stride = (int)(((window << q_log) + 63) / 64 * 64);
    const size_t lds = (size_t)(kFlagThreads / 64) * 3 * plane_stride * sizeof(uint32_t);
    const bool host = mem_kind == FXC_MEM_HOST;
    const int64_t counts_bytes = up256(n_win * n_base * 3 * (int64_t)sizeof(unsigned long long));
    const int64_t stats_base = (int64_t)nchan * 2 * (int64_t)sizeof(uint32_t);      // per window and baseline
    const int64_t slab_base = host ? window * nchan * (int64_t)(sizeof(cf) + sizeof(float) + (prior ? sizeof(float) : 0)) : 0;
    const int64_t avail = std::max<int64_t>(0, ws_target() - counts_bytes);
    const int64_t nb_slab = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(n_base, kGridMax), avail / (stats_base + slab_base)));
    const int64_t group = host || nb_slab < n_base ? 1
                                                   : std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(n_win, kGridMax),
                                                                                            avail / (stats_base * n_base)));
    const int64_t slab_elems = nb_slab * window * nchan;      // samples of a host slab
    WsCarver ws;
    const int64_t o_counts = ws.take(counts_bytes), o_stats = ws.take(group * nb_slab * stats_base);
    const int64_t o_stage = ws.take(nb_slab * slab_base);      // host rows: the slab's rows, weights and prior
    if (const int rc = ensure_ws(p, ws.total())) return rc;
    FXC_HIP(p, hipFuncSetAttribute(reinterpret_cast<const void*>(&flag_time_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds));
    unsigned long long* d_counts = ws_at<unsigned long long>(p, o_counts);
    uint32_t* d_stats = ws_at<uint32_t>(p, o_stats);
    cf* stage = ws_at<cf>(p, o_stage);
    float* stage_w = reinterpret_cast<float*>(stage + (host ? slab_elems : 0));
    float* stage_p = stage_w + (host ? slab_elems : 0);
    FXC_HIP(p, hipMemsetAsync(d_counts, 0, (size_t)counts_bytes, p->stream));
    const dim3 block(kFlagThreads);
    const unsigned gx_time = (unsigned)((nchan + (4 << q_log) - 1) / (4 << q_log)), gx_freq = (unsigned)((nchan + kFlagThreads - 1) / kFlagThreads);
    for (int64_t s0 = 0; s0 < n_win; s0 += group) {
        const int64_t s1 = std::min(n_win, s0 + group), c0 = s0 * window;
        for (int64_t b0 = 0; b0 < n_base; b0 += nb_slab) {
            const int64_t nb = std::min<int64_t>(nb_slab, n_base - b0);
            unsigned long long* d_c = d_counts + (s0 * n_base + b0) * 3;
            const dim3 grid_time(gx_time, (unsigned)nb, (unsigned)(s1 - s0)), grid_freq(gx_freq, (unsigned)nb, (unsigned)(s1 - s0));
            const int64_t w_stride = (int64_t)n_base * nchan, at = (c0 * n_base + b0) * nchan;
            if (host) {
                const int64_t n = std::min(window, n_chunks - c0), width = nb * nchan;
                FXC_HIP(p, copy_rows(p, stage, width, rows + (c0 * n_rows + b0) * nchan, n_rows * nchan, width, n, hipMemcpyHostToDevice));
                if (prior) FXC_HIP(p, copy_rows(p, stage_p, width, prior + at, w_stride, width, n, hipMemcpyHostToDevice));
                hipLaunchKernelGGL(flag_time_kernel, grid_time, block, lds, p->stream, stage, width, prior ? stage_p : nullptr, stage_w, width,
                                   window, n, time_threshold, iters, d_stats, d_c, n_base, nchan, q_log, plane_stride);
                hipLaunchKernelGGL(flag_freq_kernel, grid_freq, block, 0, p->stream, d_stats, stage_w, width, window, n, freq_threshold,
                                   half_width, d_c, n_base, nchan);
                FXC_HIP(p, copy_rows(p, weights + at, w_stride, stage_w, width, width, n, hipMemcpyDeviceToHost));
            } else {
                hipLaunchKernelGGL(flag_time_kernel, grid_time, block, lds, p->stream, rows + (c0 * n_rows + b0) * nchan, n_rows * nchan,
                                   prior ? prior + at : nullptr, weights + at, w_stride, window, n_chunks - c0, time_threshold, iters, d_stats,
                                   d_c, n_base, nchan, q_log, plane_stride);
                hipLaunchKernelGGL(flag_freq_kernel, grid_freq, block, 0, p->stream, d_stats, weights + at, w_stride, window, n_chunks - c0,
                                   freq_threshold, half_width, d_c, n_base, nchan);
            }
            FXC_HIP(p, hipGetLastError());
        }
    }
    std::vector<char> h_counts;
    if (const int rc = read_back(p, d_counts, n_win * n_base * 3 * (int64_t)sizeof(int64_t), h_counts)) return rc;
    if (counts) std::memcpy(counts, h_counts.data(), h_counts.size());
    return FXC_OK;
}

// The averager (fxcorr.h fxc_average_rows; kernel in k_average.h).  Device rows need no workspace: the launches are bounded by the
// grid limits alone.  Host rows go through the workspace in slabs: the rows, the weights and the outputs of some whole baselines
// of one interval (one strided copy in, the slab's outputs copied back), sized by the workspace target (FXC_WS_MB), one baseline
// at least.  An output cell belongs to one launch, so no bit depends on the sizes.  One synchronisation ends the call.
int average_rows_batch(fxc_plan* p, const cf* rows, const float* weights, int64_t n_chunks, int mem_kind, int64_t interval, int freq_bin,
                       cf* out_rows, float* out_weights) {
    FXC_DEVICE(p, p->device);
    const int nchan = p->nchan, n_base = p->n_base;
    const int64_t n_rows = p->n_prod;
    const int64_t n_int = (n_chunks + interval - 1) / interval;
    const int n_out = (nchan + freq_bin - 1) / freq_bin;
    const int tile = kAverageTile / freq_bin * freq_bin;      // the largest multiple of freq_bin within two bins a thread
    const int64_t out_elems = (int64_t)n_base * n_out;        // per interval
    const dim3 block(kAverageThreads);
    const unsigned gx = (unsigned)((nchan + tile - 1) / tile);
    if (mem_kind == FXC_MEM_DEVICE) {
        const int64_t c_stride = n_rows * nchan, w_stride = (int64_t)n_base * nchan;
        const int vec = nchan % 2 == 0 && tile % 2 == 0 && reinterpret_cast<uintptr_t>(rows) % 16 == 0 &&
                        reinterpret_cast<uintptr_t>(weights) % 8 == 0;
        for (int64_t s0 = 0; s0 < n_int; s0 += kGridMax) {
            const int64_t n_s = std::min(kGridMax, n_int - s0), c0 = s0 * interval;
            for (int64_t b0 = 0; b0 < n_base; b0 += kGridMax) {
                const int64_t nb = std::min<int64_t>(kGridMax, n_base - b0), at = s0 * out_elems + b0 * n_out;
                hipLaunchKernelGGL(rows_average_kernel, dim3(gx, (unsigned)nb, (unsigned)n_s), block, 0, p->stream,
                                   rows + (c0 * n_rows + b0) * nchan, c_stride, weights ? weights + (c0 * n_base + b0) * nchan : nullptr,
                                   w_stride, interval, n_chunks - c0, out_rows + at, out_weights ? out_weights + at : nullptr, out_elems,
                                   nchan, freq_bin, tile, n_out, vec);
                FXC_HIP(p, hipGetLastError());
            }
        }
        FXC_HIP(p, hipStreamSynchronize(p->stream));
        return FXC_OK;
    }
    // per baseline of a slab: the interval's rows (and weights) and the outputs; the four blocks start on 256-byte boundaries
    const int64_t in_one = interval * nchan * (int64_t)(sizeof(cf) + (weights ? sizeof(float) : 0));
    const int64_t out_one = n_out * (int64_t)(sizeof(cf) + sizeof(float));
    const int64_t nb_slab = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(n_base, kGridMax), (ws_target() - 4 * 256) / (in_one + out_one)));
    WsCarver ws;
    const int64_t o_stage = ws.take(up256(nb_slab * interval * nchan * (int64_t)sizeof(cf)));
    const int64_t o_stage_w = ws.take(weights ? up256(nb_slab * interval * nchan * (int64_t)sizeof(float)) : 0);
    const int64_t o_vis = ws.take(up256(nb_slab * n_out * (int64_t)sizeof(cf))), o_sum = ws.take(up256(nb_slab * n_out * (int64_t)sizeof(float)));
    if (const int rc = ensure_ws(p, ws.total())) return rc;
    cf* stage = ws_at<cf>(p, o_stage);
    float* stage_w = ws_at<float>(p, o_stage_w);
    cf* stage_vis = ws_at<cf>(p, o_vis);
    float* stage_sum = ws_at<float>(p, o_sum);
    for (int64_t s = 0; s < n_int; ++s) {
        const int64_t c0 = s * interval, n = std::min(interval, n_chunks - c0);
        for (int64_t b0 = 0; b0 < n_base; b0 += nb_slab) {
            const int64_t nb = std::min<int64_t>(nb_slab, n_base - b0), at = s * out_elems + b0 * n_out, width = nb * nchan;
            FXC_HIP(p, copy_rows(p, stage, width, rows + (c0 * n_rows + b0) * nchan, n_rows * nchan, width, n, hipMemcpyHostToDevice));
            if (weights)
                FXC_HIP(p, copy_rows(p, stage_w, width, weights + (c0 * n_base + b0) * nchan, (int64_t)n_base * nchan, width, n,
                                     hipMemcpyHostToDevice));
            // the staging blocks are 256-byte aligned: an even width keeps every chunk of the slab 16-byte aligned
            const int vec = nchan % 2 == 0 && tile % 2 == 0;
            hipLaunchKernelGGL(rows_average_kernel, dim3(gx, (unsigned)nb, 1), block, 0, p->stream, stage, width,
                               weights ? stage_w : nullptr, width, interval, n, stage_vis, stage_sum, (int64_t)0, nchan, freq_bin,
                               tile, n_out, vec);
            FXC_HIP(p, hipGetLastError());
            FXC_HIP(p, hipMemcpyAsync(out_rows + at, stage_vis, (size_t)(nb * n_out) * sizeof(cf), hipMemcpyDeviceToHost, p->stream));
            if (out_weights)
                FXC_HIP(p, hipMemcpyAsync(out_weights + at, stage_sum, (size_t)(nb * n_out) * sizeof(float), hipMemcpyDeviceToHost, p->stream));
        }
    }
    FXC_HIP(p, hipStreamSynchronize(p->stream));
    return FXC_OK;
}

// The time bins of a chunk's n_pts frames (beamformer, masks, kurtosis), the rule in one place: `tint` frames a bin, 0 given = the
// whole chunk; n_bin = ceil(n_pts / tint), the last bin may be partial; n_full = the bins of tint frames: a partial last bin that is
// not the chunk's only bin is not full (it has thresholds of its own count, or is not counted).  For 0 <= tint <= n_pts, n_pts > 0.
struct TimeBins {
    int64_t tint, n_bin, n_full;
};
TimeBins time_bins(const fxc_plan* p, int64_t tint) {
    if (tint == 0) tint = p->n_pts;
    const int64_t n_bin = (p->n_pts + tint - 1) / tint;
    return {tint, n_bin, p->n_pts % tint != 0 && n_bin > 1 ? n_bin - 1 : n_bin};
}

// The beamformer (fxcorr.h fxc_beamform; kernels in k_beam.h), everything on the device.  The workspace holds, each from a
// 256-byte boundary: the device copy of host weights, a pass's spectra [chunk][antenna][frame][nchan] and -- plans with a track --
// the pass's effective weights [chunk][beam][antenna][nchan].  A pass takes as many chunks as the workspace target (FXC_WS_MB)
// allows, one at least; an output element belongs to one thread of one launch and no sum crosses a chunk, so no bit depends on
// the passes.  Under a track the pass's chunks take the plan's counter onwards; the caller puts it back when the call fails.
//
// fxc_beamform_ex adds: a mask [chunk][antenna][n_mbin][nchan] -- a host mask is staged pass by pass into a
// workspace block of its own --, the incoherent mode, and `align`: on a plan with whole-sample delays every pass goes through
// align_pass (h_ingest.h) into the plan's d_align first, exactly as a pass of fx_call_dev does, and the F stage reads from there;
// under an aligned track align_pass writes the pass's shifts, which track_tables reads for the same chunks right behind it.  The
// alignment buffer counts against the workspace target like the blocks of the workspace itself.
//
// A launch of the beam kernels (k_beam.h) over the spectra of a pass: what the call site means; the tile of beams, the kernel and
// the geometry are decided in launch_beam alone.
struct BeamLaunch {
    const cf* spec;                  // [chunk][antenna][frame][nchan], natural bin order
    const cf* weff;                  // [n_beam][antenna][nchan], w_chunk elements between chunks (0: one set for every chunk)
    int64_t w_chunk;
    const float* mask;               // the pass's [chunk][antenna][n_mbin][nchan], or nullptr: every antenna counts
    int64_t mask_tint, n_mbin;
    void* out;                       // the pass's first output element
    int64_t n_chunks;                // of the pass, at most kGridMax
    int n_beam, mode;
    int64_t tint, n_tbin;            // frames a time bin (1 .. n_pts) and bins a chunk
};

int launch_beam(fxc_plan* p, const BeamLaunch& k) {
    const int nchan = p->nchan, n_ant = p->n_ant;
    // frames per range (grid.y): whole time bins, 32 frames or more where a bin is shorter; a function of (n_pts, tint) alone
    const int64_t unit = k.mode == FXC_BEAM_VOLTAGE ? kBeamFrames : k.tint;
    int64_t fpr = unit * std::max<int64_t>(1, 32 / unit);
    fpr = std::max(fpr, ((p->n_pts + kGridMax - 1) / kGridMax + unit - 1) / unit * unit);
    const dim3 grid((unsigned)((nchan + kBeamThreads - 1) / kBeamThreads), (unsigned)((p->n_pts + fpr - 1) / fpr), (unsigned)k.n_chunks);
    // the kernel of a tile of BT beams: the three share one argument list (k_beam.h)
    const auto kernel = [&](auto bt) {
        constexpr int BT = decltype(bt)::value;
        if (k.mode == FXC_BEAM_INCOHERENT) return k.mask ? beam_inc_kernel<BT, true> : beam_inc_kernel<BT, false>;
        if (k.mask) return k.mode == FXC_BEAM_POWER ? beam_mask_kernel<BT, true> : beam_mask_kernel<BT, false>;
        return k.mode == FXC_BEAM_POWER ? beam_kernel<BT, true> : beam_kernel<BT, false>;
    };
    for (int b0 = 0; b0 < k.n_beam; b0 += kBeamTile) {      // the tile of a call's beams is a function of n_beam alone
        const int left = k.n_beam - b0;
        const auto fn = left > 4   ? kernel(std::integral_constant<int, 8>{})
                        : left > 2 ? kernel(std::integral_constant<int, 4>{})
                        : left > 1 ? kernel(std::integral_constant<int, 2>{})
                                   : kernel(std::integral_constant<int, 1>{});
        hipLaunchKernelGGL(fn, grid, dim3(kBeamThreads), 0, p->stream, k.spec, k.weff, k.w_chunk, k.mask, k.mask_tint, k.n_mbin, k.out, n_ant,
                           p->n_pts, nchan, k.n_beam, b0, k.tint, fpr, k.n_tbin);
    }
    FXC_HIP(p, hipGetLastError());
    return FXC_OK;
}

int beamform_dev(fxc_plan* p, const cf* x, const cf* weights, bool weights_on_host, int n_beam, const float* mask, int64_t mask_tint,
                 void* out, int64_t n_chunks, int mode, int64_t tint, bool align) {
    const int nchan = p->nchan, n_ant = p->n_ant;
    const bool voltage = mode == FXC_BEAM_VOLTAGE;
    const bool al = align && aligning(p);
    const TimeBins tb = time_bins(p, tint), mb = time_bins(p, mask_tint);
    const int64_t w_elems = (int64_t)n_beam * n_ant * nchan;
    const int64_t m_elems = (int64_t)n_ant * mb.n_bin * nchan;      // of a chunk's mask
    const int64_t wcopy_bytes = weights_on_host ? up256(w_elems * (int64_t)sizeof(cf)) : 0;
    const int64_t spec_per_chunk = (int64_t)n_ant * p->n_pts * nchan * (int64_t)sizeof(cf);
    const int64_t weff_per_chunk = p->track ? w_elems * (int64_t)sizeof(cf) : 0;
    const int64_t mask_per_chunk = mask && weights_on_host ? m_elems * (int64_t)sizeof(float) : 0;      // a host mask is staged
    const int64_t align_per_chunk = al ? (int64_t)n_ant * p->num_samp * (int64_t)sizeof(cf) : 0;
    int64_t cb = std::min<int64_t>(std::min(n_chunks, kGridMax),
                                   (ws_target() - wcopy_bytes) / (spec_per_chunk + weff_per_chunk + mask_per_chunk + align_per_chunk));
    if (al) cb = std::min<int64_t>(cb, kGridMax / n_ant);      // (the stream index rides in a grid dimension of the alignment kernel)
    cb = std::max<int64_t>(1, cb);
    WsCarver ws;
    const int64_t o_wcopy = ws.take(wcopy_bytes), o_spec = ws.take(up256(cb * spec_per_chunk)), o_weff = ws.take(up256(cb * weff_per_chunk));
    const int64_t o_mask = ws.take(up256(cb * mask_per_chunk));
    int rc = ensure_ws(p, ws.total());      // (flushes a pending fold: it lives in the workspace)
    if (rc) return rc;
    cf* spec = ws_at<cf>(p, o_spec);
    cf* weff = ws_at<cf>(p, o_weff);
    if (weights_on_host) {
        FXC_HIP(p, hipMemcpyAsync(ws_at<cf>(p, o_wcopy), weights, (size_t)w_elems * sizeof(cf), hipMemcpyHostToDevice, p->stream));
        weights = ws_at<cf>(p, o_wcopy);
    }
    const int64_t out_per_chunk = voltage ? (int64_t)n_beam * p->n_pts * nchan * (int64_t)sizeof(cf)
                                          : (int64_t)n_beam * tb.n_bin * nchan * (int64_t)sizeof(float);
    for (int64_t c0 = 0; c0 < n_chunks; c0 += cb) {
        const int64_t nc = std::min(cb, n_chunks - c0);
        PassInput in{chunk_at(p, x, c0)};
        if (al) {      // (under an aligned track: the shifts of the chunks p->track_t onwards, the chunks of the tables below)
            rc = align_pass(p, nc, &in);
            if (rc) return rc;
        }
        rc = run_channelize(p, in.x, spec, nc * n_ant);
        if (rc) return rc;
        const float* mk = mask ? mask + c0 * m_elems : nullptr;
        if (mask_per_chunk) {
            FXC_HIP(p, hipMemcpyAsync(ws_at<float>(p, o_mask), mk, (size_t)(nc * m_elems) * sizeof(float), hipMemcpyHostToDevice, p->stream));
            mk = ws_at<float>(p, o_mask);
        }
        const cf* wk = weights;
        if (p->track) {
            const int rg = grow(p, p->d_track, (size_t)(nc * n_ant * nchan) * sizeof(cd));
            if (rg) return rg;
            rc = track_tables(p, p->track_t, nc, static_cast<cd*>(p->d_track.get()), false);
            if (rc) return rc;
            p->track_t += nc;
            hipLaunchKernelGGL(beam_weights_kernel, dim3(grid_for(nc * w_elems, 256, p->cu_count)), dim3(256), 0, p->stream, weights,
                               static_cast<const cd*>(p->d_track.get()), weff, n_beam, n_ant, nchan, nc);
            FXC_HIP(p, hipGetLastError());
            wk = weff;
        }
        KernelTimer kt(p);
        rc = launch_beam(p, {spec, wk, p->track ? w_elems : 0, mk, mb.tint, mb.n_bin, static_cast<char*>(out) + c0 * out_per_chunk, nc, n_beam,
                             mode, tb.tint, tb.n_bin});
        kt.stop();
        if (rc) return rc;
    }
    return FXC_OK;
}

// The antenna mask from sk (fxc_kurtosis_antenna_mask), both on the device
int kurtosis_mask_dev(fxc_plan* p, const float* sk, float* mask, int64_t n_chunks, int64_t tint, double lo, double hi, double lo_last,
                      double hi_last) {
    const TimeBins tb = time_bins(p, tint);      // a bin that is not full has the thresholds of its own count
    const int64_t total = n_chunks * p->n_ant * tb.n_bin * p->nchan;
    if (total == 0) return FXC_OK;
    hipLaunchKernelGGL(kurtosis_mask_kernel, dim3(grid_for(total, 256, p->cu_count)), dim3(256), 0, p->stream, sk, mask, p->nchan, tb.n_bin,
                       tb.n_full, total, lo, hi, lo_last, hi_last);
    FXC_HIP(p, hipGetLastError());
    return FXC_OK;
}

// the arguments fxc_kurtosis and fxc_kurtosis_weights share; *done: the call has nothing to do
int check_kurtosis(fxc_plan* p, int64_t n_chunks, int mem_kind, int64_t tint, bool* done) {
    *done = false;
    if (!p) return fail(p, FXC_ERR_ARG, "NULL plan");
    if (n_chunks < 0) return fail(p, FXC_ERR_ARG, "n_chunks < 0");
    if (const int rc = bad_mem_kind(p, mem_kind)) return rc;
    if (tint < 0 || tint == 1 || tint > p->n_pts)
        return fail(p, FXC_ERR_ARG, "tint=%lld is not 0 or within 2 .. %lld frames", (long long)tint, (long long)p->n_pts);
    if (p->n_pts < 2) return fail(p, FXC_ERR_UNSUPPORTED, "n_pts=%lld: the estimator needs 2 or more frames a chunk", (long long)p->n_pts);
    *done = n_chunks == 0;
    return FXC_OK;
}

// A launch of kurtosis_kernel (k_kurtosis.h) over the spectra of n_streams consecutive (chunk, antenna) streams: what the call
// site means; the geometry is decided here alone
struct KurtosisLaunch {
    const cf* spec;                  // [stream][frame][nchan], natural bin order
    float* sk;                       // [stream][n_tbin][nchan]
    float* power;                    // the same shape, or nullptr
    int64_t n_streams;               // at most kGridMax
    int64_t tint, n_tbin;            // frames a time bin (1 .. n_pts) and bins a chunk
};

int launch_kurtosis(fxc_plan* p, const KurtosisLaunch& k) {
    // bins of one segment: a wave takes as many bins as make a segment's worth of frames, a workgroup no more waves than there are
    // bins for; longer bins: a workgroup a bin.  More bins than grid.y holds: the kernel walks on.  No bit depends on any of it.
    if ((int64_t)kKurtSegment * p->nchan >= (1ll << 31))      // (kurt_segment's 32-bit row offsets)
        return fail(p, FXC_ERR_UNSUPPORTED, "nchan=%d: a segment of %d spectra is addressed in 32 bits", p->nchan, kKurtSegment);
    int64_t bpw = 0, waves = kKurtWaves, groups = k.n_tbin;
    if (k.tint <= kKurtSegment) {
        bpw = std::max<int64_t>(1, kKurtSegment / k.tint);
        waves = std::min<int64_t>(kKurtWaves, (k.n_tbin + bpw - 1) / bpw);
        groups = (k.n_tbin + bpw * waves - 1) / (bpw * waves);
    }
    const dim3 grid((unsigned)((p->nchan + kKurtLanes - 1) / kKurtLanes), (unsigned)std::min(groups, kGridMax), (unsigned)k.n_streams);
    hipLaunchKernelGGL(kurtosis_kernel, grid, dim3((unsigned)(kKurtLanes * waves)), 0, p->stream, k.spec, k.sk, k.power, p->n_pts, p->nchan,
                       k.tint, k.n_tbin, bpw);
    FXC_HIP(p, hipGetLastError());
    return FXC_OK;
}

// Spectral kurtosis (fxcorr.h fxc_kurtosis; kernels in k_kurtosis.h), everything on the device, the route of beamform_dev: the
// workspace holds a pass's spectra [chunk][antenna][frame][nchan]; a pass takes as many chunks as the workspace target (FXC_WS_MB)
// allows, one at least.  An output element belongs to one workgroup of one launch and no sum crosses a chunk, so no bit depends on
// the passes.  The samples are taken as delivered: no shifts, no tables, and the track's counter stays.
int kurtosis_dev(fxc_plan* p, const cf* x, float* sk, float* power, int64_t n_chunks, int64_t tint) {
    const int nchan = p->nchan, n_ant = p->n_ant;
    const TimeBins tb = time_bins(p, tint);
    const int64_t spec_per_chunk = (int64_t)n_ant * p->n_pts * nchan * (int64_t)sizeof(cf);
    const int64_t cb = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(n_chunks, kGridMax / n_ant), ws_target() / spec_per_chunk));
    WsCarver ws;
    const int64_t o_spec = ws.take(up256(cb * spec_per_chunk));
    int rc = ensure_ws(p, ws.total());      // (flushes a pending fold: it lives in the workspace)
    if (rc) return rc;
    cf* spec = ws_at<cf>(p, o_spec);
    const int64_t out_per_chunk = (int64_t)n_ant * tb.n_bin * nchan;
    for (int64_t c0 = 0; c0 < n_chunks; c0 += cb) {
        const int64_t nc = std::min(cb, n_chunks - c0);
        rc = run_channelize(p, chunk_at(p, x, c0), spec, nc * n_ant);
        if (rc) return rc;
        KernelTimer kt(p);
        rc = launch_kurtosis(p, {spec, sk + c0 * out_per_chunk, power ? power + c0 * out_per_chunk : nullptr, nc * n_ant, tb.tint, tb.n_bin});
        kt.stop();
        if (rc) return rc;
    }
    return FXC_OK;
}

// The row weights from sk (fxc_kurtosis_weights), both on the device
int kurtosis_weights_dev(fxc_plan* p, const float* sk, float* weights, int64_t n_chunks, int64_t tint, double lo, double hi) {
    const TimeBins tb = time_bins(p, tint);      // a bin that is not full has another count than the thresholds were made for: not counted
    const int64_t total = n_chunks * p->n_base * p->nchan;
    if (total == 0) return FXC_OK;
    hipLaunchKernelGGL(kurtosis_weights_kernel, dim3(grid_for(total, 256, p->cu_count)), dim3(256), 0, p->stream, sk, weights, p->n_ant,
                       p->n_base, p->nchan, tb.n_bin, tb.n_full, n_chunks, lo, hi);
    FXC_HIP(p, hipGetLastError());
    return FXC_OK;
}

// A call's trial table as the dedispersion kernels (k_dedisperse.h) read it, made on the host from the caller's shifts and channel
// weights: the groups of kDedD consecutive trials, which of them the tiled kernel serves, and the geometry that follows.  The
// decision tiled against direct and the LDS a launch needs are made here alone.
struct DedTable {
    int n_dm = 0, n_groups = 0, n_step = 0;
    int64_t s_max = 0;
    // shifts [n_groups][n_step 32][kDedD], chan [n_step 32], cnt [n_step], bs [n_groups][n_step][2], the tiled groups, the direct groups
    std::vector<int> words;
    int64_t o_chan = 0, o_cnt = 0, o_bs = 0, o_tiled = 0, o_direct = 0;      // offsets into words
    int n_tiled = 0, n_direct = 0;          // groups
    int64_t trials_tiled = 0, trials_direct = 0;
    int wp = 0;                             // words of a channel's LDS line in the tiled launches: odd
    DedTab on_device(const int* d_words) const {
        return DedTab{d_words, d_words + o_chan, d_words + o_cnt, d_words + o_bs, n_step, n_dm};
    }
};

// -> FXC_ERR_ARG for a negative shift (the only check of the table's values; the caller compares s_max with n_t)
int build_ded_table(fxc_plan* p, const int32_t* shifts, int n_dm, const float* chan_weights, DedTable* t) {
    const int nchan = p->nchan;
    t->n_dm = n_dm;
    t->n_groups = (n_dm + kDedD - 1) / kDedD;
    t->n_step = (nchan + kDedStep - 1) / kDedStep;
    for (int64_t i = 0; i < (int64_t)n_dm * nchan; ++i) {
        if (shifts[i] < 0)
            return fail(p, FXC_ERR_ARG, "shifts[%lld][%lld]=%d is negative", (long long)(i / nchan), (long long)(i % nchan), (int)shifts[i]);
        t->s_max = std::max<int64_t>(t->s_max, shifts[i]);
    }
    const int64_t n_slots = (int64_t)t->n_step * kDedStep;
    t->o_chan = (int64_t)t->n_groups * n_slots * kDedD;
    t->o_cnt = t->o_chan + n_slots;
    t->o_bs = t->o_cnt + t->n_step;
    t->o_tiled = t->o_bs + (int64_t)t->n_groups * t->n_step * 2;
    t->o_direct = t->o_tiled + t->n_groups;
    t->words.assign((size_t)(t->o_direct + t->n_groups), 0);
    int* const w = t->words.data();
    // the counted channels of every step, in ascending order (a NaN weight does not count)
    for (int q = 0; q < t->n_step; ++q)
        for (int k = q * kDedStep; k < std::min(nchan, (q + 1) * kDedStep); ++k)
            if (!chan_weights || chan_weights[k] > 0.f) w[t->o_chan + q * kDedStep + w[t->o_cnt + q]++] = k;
    int span_max = 0;
    for (int g = 0; g < t->n_groups; ++g) {
        const int d0 = g * kDedD, nd = std::min(kDedD, n_dm - d0);
        bool fits = true;
        int span_g = 0;
        for (int q = 0; q < t->n_step; ++q) {
            int lo = INT32_MAX, hi = 0;
            for (int i = 0; i < w[t->o_cnt + q]; ++i) {
                const int64_t slot = (int64_t)q * kDedStep + i;
                const int k = w[t->o_chan + slot];
                for (int d = 0; d < kDedD; ++d) {
                    const int sh = shifts[(int64_t)(d0 + (d < nd ? d : 0)) * nchan + k];
                    w[((int64_t)g * n_slots + slot) * kDedD + d] = sh;
                    lo = std::min(lo, sh);
                    hi = std::max(hi, sh);
                }
            }
            if (lo > hi) lo = hi = 0;      // no channel of the step counts: the step is skipped
            w[t->o_bs + 2 * ((int64_t)g * t->n_step + q)] = lo;
            w[t->o_bs + 2 * ((int64_t)g * t->n_step + q) + 1] = hi - lo;
            if (hi - lo > kDedMaxSpan) fits = false;
            span_g = std::max(span_g, hi - lo);
        }
        if (fits) {
            w[t->o_tiled + t->n_tiled++] = g;
            t->trials_tiled += nd;
            span_max = std::max(span_max, span_g);
        } else {
            w[t->o_direct + t->n_direct++] = g;
            t->trials_direct += nd;
        }
    }
    t->wp = (kDedT + span_max) | 1;
    return FXC_OK;
}

// A launch of the dedispersion kernels over n_o output times of n_series series that lie s_in (outputs: s_out) elements apart: what
// the call site means; the grids are decided here alone, each dimension bounded by the grid limits
struct DedLaunch {
    DedIn in;
    int64_t s_in;
    int64_t n_series;
    unsigned t_lo, n_o;              // the first output time, in the time axis of `in`, and the outputs
    float* out;                      // output (series 0, trial 0, time t_lo)
    int64_t s_out, o_stride;         // elements between series and between trials
};

int launch_dedisperse(fxc_plan* p, const DedTable& t, const int* d_words, const DedLaunch& k) {
    const unsigned n_tiles = (k.n_o + kDedT - 1) / kDedT;
    const size_t lds = (size_t)kDedStep * t.wp * sizeof(float);
    const DedTab tb = t.on_device(d_words);
    // the tiled kernel's x: the tiles rounded up to eight, times the groups of the launch -- as many as keep it within 31 bits
    const int64_t tiles8 = ((int64_t)n_tiles + 7) / 8 * 8;
    const int64_t ng_max = std::max<int64_t>(1, std::min<int64_t>(kGridMax, ((1ll << 31) - 1) / tiles8));
    for (int64_t s0 = 0; s0 < k.n_series; s0 += kGridMax) {
        const unsigned ns = (unsigned)std::min(kGridMax, k.n_series - s0);
        DedIn in = k.in;
        in.p += s0 * k.s_in;
        float* out = k.out + s0 * k.s_out;
        for (int64_t g0 = 0; g0 < t.n_tiled; g0 += ng_max) {
            const int64_t ng = std::min<int64_t>(ng_max, t.n_tiled - g0);
            hipLaunchKernelGGL(dedisperse_tiled_kernel, dim3((unsigned)(tiles8 * ng), 1, ns), dim3(kDedThreads), lds, p->stream, in, k.s_in, tb,
                               d_words + t.o_tiled + g0, (unsigned)ng, n_tiles, k.t_lo, k.n_o, out, k.s_out, k.o_stride, t.wp);
        }
        constexpr int64_t per = kGridMax / kDedD;      // groups of a direct launch
        for (int64_t g0 = 0; g0 < t.n_direct; g0 += per)
            hipLaunchKernelGGL(dedisperse_direct_kernel, dim3(n_tiles, (unsigned)(std::min<int64_t>(per, t.n_direct - g0) * kDedD), ns),
                               dim3(kDedThreads), 0, p->stream, in, k.s_in, tb, d_words + t.o_direct + g0, k.t_lo, k.n_o, out, k.s_out,
                               k.o_stride);
    }
    FXC_HIP(p, hipGetLastError());
    return FXC_OK;
}

// Dedispersion (fxcorr.h fxc_dedisperse; kernels in k_dedisperse.h) after the argument checks; the table is valid and s_max < n_t.
// The workspace holds the table and, for host power, a slab: some whole chunks of one series (one strided copy in) and the
// outputs of every trial over the slab's times (one strided copy back).  A slab's outputs are the times whose samples, s_max
// further on included, lie inside it; the next slab starts with the chunk of the next output, so consecutive slabs overlap by the
// halo.  Slabs are sized by the workspace target (FXC_WS_MB) and hold at least the chunks one output needs wherever it lies in its
// chunk.  Device power needs no staging.  An output cell belongs to one thread of one launch, and no sum depends on the tile, so
// no bit depends on the sizes.  One synchronisation ends the call.
int dedisperse_batch(fxc_plan* p, const float* power, int64_t n_chunks, int64_t n_series, int64_t n_tbin, int mem_kind, const DedTable& t,
                     float* out, int64_t* info_out) {
    FXC_DEVICE(p, p->device);
    const int nchan = p->nchan, n_dm = t.n_dm;
    const int64_t n_t = n_chunks * n_tbin, n_out = n_t - t.s_max;
    const int64_t chunk_elems = n_tbin * nchan;
    const bool host = mem_kind == FXC_MEM_HOST;
    const int64_t tab_bytes = up256((int64_t)t.words.size() * (int64_t)sizeof(int));
    const int64_t need = std::min(n_chunks, 1 + (t.s_max + n_tbin - 1) / n_tbin);
    const int64_t per_chunk = (chunk_elems + (int64_t)n_dm * n_tbin) * (int64_t)sizeof(float);
    const int64_t cs = host ? std::min(n_chunks, std::max(need, (ws_target() - tab_bytes - 2 * 256) / per_chunk)) : 0;
    WsCarver ws;
    const int64_t o_tab = ws.take(tab_bytes), o_stage = ws.take(up256(cs * chunk_elems * (int64_t)sizeof(float)));
    const int64_t o_res = ws.take(up256(cs * n_tbin * n_dm * (int64_t)sizeof(float)));
    if (const int rc = ensure_ws(p, ws.total())) return rc;
    FXC_HIP(p, hipFuncSetAttribute(reinterpret_cast<const void*>(&dedisperse_tiled_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   kDedLdsBytes));
    int* d_words = ws_at<int>(p, o_tab);
    FXC_HIP(p, hipMemcpyAsync(d_words, t.words.data(), t.words.size() * sizeof(int), hipMemcpyHostToDevice, p->stream));
    if (!host) {
        // one chunk, or one series: the time axis is contiguous
        const bool flat = n_chunks == 1 || n_series == 1;
        const DedIn in{power, flat ? 0 : (n_series - 1) * chunk_elems, (unsigned)(flat ? n_t : n_tbin), (unsigned)n_t, nchan};
        if (const int rc = launch_dedisperse(p, t, d_words, {in, chunk_elems, n_series, 0u, (unsigned)n_out, out, (int64_t)n_dm * n_out, n_out}))
            return rc;
    } else {
        float* stage = ws_at<float>(p, o_stage);
        float* res = ws_at<float>(p, o_res);
        const int64_t cap = cs * n_tbin;
        for (int64_t s = 0; s < n_series; ++s) {
            for (int64_t o0 = 0; o0 < n_out;) {
                const int64_t c0 = o0 / n_tbin, c1 = std::min(n_chunks, c0 + cs), o1 = std::min(n_out, c1 * n_tbin - t.s_max);
                const int64_t n_loc = (c1 - c0) * n_tbin;
                FXC_HIP(p, copy_rows(p, stage, chunk_elems, power + (c0 * n_series + s) * chunk_elems, n_series * chunk_elems, chunk_elems,
                                     c1 - c0, hipMemcpyHostToDevice));
                const DedIn in{stage, 0, (unsigned)n_loc, (unsigned)n_loc, nchan};
                if (const int rc = launch_dedisperse(p, t, d_words, {in, 0, 1, (unsigned)(o0 - c0 * n_tbin), (unsigned)(o1 - o0), res, 0, cap}))
                    return rc;
                FXC_HIP(p, copy_rows(p, out + s * n_dm * n_out + o0, n_out, res, cap, o1 - o0, (int64_t)n_dm, hipMemcpyDeviceToHost));
                o0 = o1;
            }
        }
    }
    FXC_HIP(p, hipStreamSynchronize(p->stream));
    if (info_out) {
        info_out[0] = t.trials_tiled;
        info_out[1] = t.trials_direct;
    }
    return FXC_OK;
}

// How a boxcar search cuts a row of n_t samples into cells (the output's blocks) and filter tiles (k_boxcar.h BoxGeom), and what
// a launch of the filter needs: decided here alone.  A block that reaches past the starts is the one cell it leaves.
struct BoxPlan {
    BoxGeom g;
    int64_t n_tiles;          // filter workgroups a row
    int64_t n_seg;            // segments of 256 samples a row
    size_t lds;               // bytes of the filter's two level buffers, or of the bests that take their place
    bool partial() const { return g.tiles != 0; }
};

BoxPlan box_geometry(int64_t n_t, int j_lo, int j_hi, int64_t block) {
    BoxPlan b{};
    b.g.n_t = n_t;
    b.g.j_lo = j_lo;
    b.g.j_hi = j_hi;
    while ((1ll << b.g.j_hi) > n_t) --b.g.j_hi;      // a width that does not fit has no start; 2^j_lo <= n_t
    b.g.n_starts = n_t - (1ll << j_lo) + 1;
    b.g.block = std::min(block, b.g.n_starts);
    b.g.n_blk = (b.g.n_starts + b.g.block - 1) / b.g.block;
    if (b.g.block <= kBoxT) {
        b.g.cells = (unsigned)(kBoxT / b.g.block);
        b.g.tiles = 0;
        b.n_tiles = (b.g.n_blk + b.g.cells - 1) / b.g.cells;
    } else {
        b.g.cells = 0;
        b.g.tiles = (unsigned)((b.g.block + kBoxT - 1) / kBoxT);
        b.n_tiles = b.g.n_blk * b.g.tiles;
    }
    b.n_seg = (n_t + kBoxSeg - 1) / kBoxSeg;
    b.lds = sizeof(float) * (size_t)std::max<int64_t>(2 * (kBoxT + (1ll << b.g.j_hi) - 1), 2 * kBoxBestWords);
    return b;
}

// The kernels of a boxcar search over n rows that lie n_t samples apart on the device: the statistics' rounds, the filter and,
// where a block is larger than a tile, the fold of the partial bests.  Each grid dimension is bounded here: rows go through in
// launches of kGridMax at most.
struct BoxLaunch {
    const float* x;
    int64_t n;
    BoxRow* rows;
    double* seg_sum;
    int* seg_cnt;
    const double* root;
    float* p_snr;      // the partial bests (block > tile) ..
    int *p_w, *p_t;
    float* snr;        // .. and the outputs, [n][n_blk]
    int *width, *time;
};

int launch_boxcar(fxc_plan* p, const BoxPlan& b, const BoxLaunch& k, double c2, int rounds) {
    const BoxGeom& g = b.g;
    hipLaunchKernelGGL(boxcar_rows_init_kernel, dim3((unsigned)((k.n + 255) / 256)), dim3(256), 0, p->stream, k.rows, k.n);
    const unsigned sweep_x = (unsigned)((b.n_seg + kBoxSegs - 1) / kBoxSegs);
    for (int round = 0; round <= rounds; ++round)
        for (int second = 0; second < 2; ++second)
            for (int64_t r0 = 0; r0 < k.n; r0 += kGridMax) {
                const unsigned nr = (unsigned)std::min(kGridMax, k.n - r0);
                hipLaunchKernelGGL(boxcar_sweep_kernel, dim3(sweep_x, nr), dim3(kBoxThreads), 0, p->stream, k.x + r0 * g.n_t, g.n_t,
                                   k.rows + r0, k.seg_sum + r0 * b.n_seg, k.seg_cnt + r0 * b.n_seg, b.n_seg, second);
                hipLaunchKernelGGL(boxcar_round_kernel, dim3(nr), dim3(kBoxThreads), 0, p->stream, k.rows + r0, k.seg_sum + r0 * b.n_seg,
                                   k.seg_cnt + r0 * b.n_seg, b.n_seg, second, (int)(round == rounds), c2, k.root);
            }
    const int64_t stride = b.partial() ? b.n_tiles : g.n_blk;
    for (int64_t r0 = 0; r0 < k.n; r0 += kGridMax) {
        const unsigned nr = (unsigned)std::min(kGridMax, k.n - r0);
        hipLaunchKernelGGL(boxcar_filter_kernel, dim3((unsigned)b.n_tiles, nr), dim3(kBoxThreads), b.lds, p->stream, k.x + r0 * g.n_t,
                           k.rows + r0, g, (b.partial() ? k.p_snr : k.snr) + r0 * stride, (b.partial() ? k.p_w : k.width) + r0 * stride,
                           (b.partial() ? k.p_t : k.time) + r0 * stride, stride);
    }
    if (b.partial()) {
        constexpr int64_t per = (1ll << 31) - kBoxThreads;      // cells of a fold launch
        for (int64_t r0 = 0; r0 < k.n;) {
            const int64_t nr = std::max<int64_t>(1, std::min(k.n - r0, per / g.n_blk));
            hipLaunchKernelGGL(boxcar_fold_kernel, dim3((unsigned)((nr * g.n_blk + kBoxThreads - 1) / kBoxThreads)), dim3(kBoxThreads), 0,
                               p->stream, k.p_snr + r0 * stride, k.p_w + r0 * stride, k.p_t + r0 * stride, g, nr, k.snr + r0 * g.n_blk,
                               k.width + r0 * g.n_blk, k.time + r0 * g.n_blk);
            r0 += nr;
        }
    }
    FXC_HIP(p, hipGetLastError());
    return FXC_OK;
}

// The boxcar search (fxcorr.h fxc_boxcar_search; kernels in k_boxcar.h) after the argument checks.  The workspace holds the table of
// sqrt(2^j), and per row of a slab its state, the tree's segment sums and counts, the partial bests where a block is larger than a
// tile and, for host input, the row itself and its three outputs: a slab is some whole rows (one copy in, three copies back), sized
// by the workspace target (FXC_WS_MB) and one row at least, whatever the row's size.  Device input needs no staging and its outputs
// are written in place; it goes through in the same slabs, which bound the scratch.  No number depends on the slab: a row's
// statistics and cells belong to its own workgroups.  One synchronisation ends the call.
int boxcar_batch(fxc_plan* p, const float* x, int64_t n_rows, int64_t n_t, int mem_kind, int j_lo, int j_hi, int64_t block, double clip,
                 int clip_iters, float* snr_out, int* width_out, int* time_out, double* stats_out) {
    FXC_DEVICE(p, p->device);
    const BoxPlan b = box_geometry(n_t, j_lo, j_hi, block);
    const bool host = mem_kind == FXC_MEM_HOST;
    const int64_t n_blk = b.g.n_blk, n_part = b.partial() ? b.n_tiles : 0;
    const int rounds = clip == 0.0 ? 0 : clip_iters;
    const double c2 = clip * clip;
    double root[kBoxMaxJ + 1];
    for (int j = 0; j <= kBoxMaxJ; ++j) root[j] = std::sqrt((double)(1ll << j));
    const int64_t per_row = (int64_t)sizeof(BoxRow) + b.n_seg * 12 + n_part * 12 + (host ? (n_t + 3 * n_blk) * 4 : 0);
    const int64_t fixed = 256 + 9 * 256;      // the table, and the rounding of the blocks
    const int64_t slab = std::max<int64_t>(1, std::min(n_rows, (ws_target() - fixed) / per_row));
    WsCarver ws;
    const int64_t o_root = ws.take(256), o_rows = ws.take(up256(slab * (int64_t)sizeof(BoxRow)));
    const int64_t o_sum = ws.take(up256(slab * b.n_seg * 8)), o_cnt = ws.take(up256(slab * b.n_seg * 4));
    const int64_t o_ps = ws.take(up256(slab * n_part * 4)), o_pw = ws.take(up256(slab * n_part * 4)), o_pt = ws.take(up256(slab * n_part * 4));
    const int64_t o_x = ws.take(host ? up256(slab * n_t * 4) : 0);
    const int64_t o_s = ws.take(host ? up256(slab * n_blk * 4) : 0), o_w = ws.take(host ? up256(slab * n_blk * 4) : 0);
    const int64_t o_t = ws.take(host ? up256(slab * n_blk * 4) : 0);
    if (const int rc = ensure_ws(p, ws.total())) return rc;
    FXC_HIP(p, hipMemcpyAsync(ws_at<double>(p, o_root), root, sizeof root, hipMemcpyHostToDevice, p->stream));
    std::vector<BoxRow> states(stats_out ? (size_t)n_rows : 0);
    for (int64_t r0 = 0; r0 < n_rows; r0 += slab) {
        const int64_t n = std::min(slab, n_rows - r0);
        BoxLaunch k{};
        k.n = n;
        k.rows = ws_at<BoxRow>(p, o_rows);
        k.seg_sum = ws_at<double>(p, o_sum);
        k.seg_cnt = ws_at<int>(p, o_cnt);
        k.root = ws_at<double>(p, o_root);
        k.p_snr = ws_at<float>(p, o_ps);
        k.p_w = ws_at<int>(p, o_pw);
        k.p_t = ws_at<int>(p, o_pt);
        if (host) {
            float* stage = ws_at<float>(p, o_x);
            FXC_HIP(p, hipMemcpyAsync(stage, x + r0 * n_t, (size_t)(n * n_t) * sizeof(float), hipMemcpyHostToDevice, p->stream));
            k.x = stage;
            k.snr = ws_at<float>(p, o_s);
            k.width = ws_at<int>(p, o_w);
            k.time = ws_at<int>(p, o_t);
        } else {
            k.x = x + r0 * n_t;
            k.snr = snr_out + r0 * n_blk;
            k.width = width_out + r0 * n_blk;
            k.time = time_out + r0 * n_blk;
        }
        if (const int rc = launch_boxcar(p, b, k, c2, rounds)) return rc;
        if (host) {
            const size_t bytes = (size_t)(n * n_blk) * 4;
            FXC_HIP(p, hipMemcpyAsync(snr_out + r0 * n_blk, k.snr, bytes, hipMemcpyDeviceToHost, p->stream));
            FXC_HIP(p, hipMemcpyAsync(width_out + r0 * n_blk, k.width, bytes, hipMemcpyDeviceToHost, p->stream));
            FXC_HIP(p, hipMemcpyAsync(time_out + r0 * n_blk, k.time, bytes, hipMemcpyDeviceToHost, p->stream));
        }
        if (stats_out)
            FXC_HIP(p, hipMemcpyAsync(states.data() + r0, k.rows, (size_t)n * sizeof(BoxRow), hipMemcpyDeviceToHost, p->stream));
    }
    FXC_HIP(p, hipStreamSynchronize(p->stream));
    for (size_t i = 0; i < states.size(); ++i) {
        stats_out[3 * i] = states[i].m;
        stats_out[3 * i + 1] = states[i].stdv;
        stats_out[3 * i + 2] = (double)states[i].n;
    }
    return FXC_OK;
}

}  // namespace
