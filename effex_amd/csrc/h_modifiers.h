// Part of libfxcorr's single translation unit: included by fxcorr.hip (not a stand-alone header).
#pragma once

// what changes the rows a plan makes -- rot tables, the delay track, its gains, whole-sample shifts: the drivers behind the ABI's
// setters (fxcorr.hip keeps their argument checks)

namespace {

bool acc_empty(const fxc_plan* p) { return !(p->spectra_count > 0.0) && !p->pend.valid; }

// fxc_set_rot / fxc_set_rot_ant end a delay track -- unless the accumulator holds tracked chunks: their sums are rotated already,
// a static table at finalize would rotate them again
int end_track(fxc_plan* p) {
    if (p->track && p->acc_track && !acc_empty(p))
        return fail(p, FXC_ERR_STATE, "the accumulator holds chunks accumulated under the delay track: finalize or reset it first");
    p->track = false;
    p->track_align = false;      // (the per-chunk shifts of an aligned track end with it; static shifts are not the track's)
    p->gain_n = 0;      // the gains were solved under this track: they end with it (release_gain_q frees them once the stream is idle)
    return FXC_OK;
}

// the static whole-sample shifts, or none of them (shifts == nullptr); the caller has synchronised the plan's stream
int store_sample_shifts(fxc_plan* p, const int64_t* shifts) {
    bool any = false;
    for (int a = 0; shifts && a < p->n_ant; ++a) any = any || shifts[a] != 0;
    if (!any) {
        p->shifted = false;
        p->sample_shift.clear();
        return FXC_OK;
    }
    std::vector<int> s32((size_t)p->n_ant);
    for (int a = 0; a < p->n_ant; ++a) s32[(size_t)a] = (int)shifts[a];      // (|s| < num_samp <= 2^27: checked by the caller)
    if (!p->d_shift) FXC_HIP(p, p->d_shift.alloc((size_t)p->n_ant));
    FXC_HIP(p, hipMemcpy(p->d_shift, s32.data(), (size_t)p->n_ant * sizeof(int), hipMemcpyHostToDevice));
    p->sample_shift.assign(shifts, shifts + p->n_ant);
    p->shifted = true;
    return FXC_OK;
}

// s_a(t) of an aligned track as track_shift (k_align.h) forms it on the device: the same individually rounded operations
int64_t track_shift_host(const fxc_plan* p, int a, int64_t t) {
#pragma clang fp contract(off)
    const double tau = p->track_par_h[(size_t)a] + (double)t * p->track_par_h[(size_t)(p->n_ant + a)];
    double v = tau * p->track_bw;
    v = v > 2147483647.0 ? 2147483647.0 : (v < -2147483647.0 ? -2147483647.0 : v);
    return (int64_t)std::llrint(v);
}

constexpr int64_t kAlignMaxSamp = 1ll << 27;      // a stream within one buffer descriptor (align_c64_kernel)

// frees the table of a gain track that has ended; the caller has synchronised the plan's stream
void release_gain_q(fxc_plan* p) {
    if (p->gain_n == 0) p->d_gain_q.reset();
}

// fxc_set_delay_track and, `aligned`, fxc_set_delay_track_aligned: the same track, with the whole samples of every chunk's delays
// taken out of the tables and applied to the samples
int set_delay_track(fxc_plan* p, const double* tau0_s, const double* rate_s_per_chunk, double bandwidth, double frequency,
                    int64_t first_chunk, bool aligned) {
    if (!p || !tau0_s || !rate_s_per_chunk) return fail(p, FXC_ERR_ARG, "NULL argument");
    if (p->n_ant < 2) return fail(p, FXC_ERR_ARG, "a delay track needs 2 or more antennas, the plan has %d", p->n_ant);
    if (!(bandwidth > 0.0) || !std::isfinite(bandwidth) || !std::isfinite(frequency))
        return fail(p, FXC_ERR_ARG, "bandwidth must be > 0 and finite, frequency finite");
    if (first_chunk < 0) return fail(p, FXC_ERR_ARG, "first_chunk < 0");
    for (int a = 0; a < p->n_ant; ++a)
        if (!std::isfinite(tau0_s[a]) || !std::isfinite(rate_s_per_chunk[a]))
            return fail(p, FXC_ERR_ARG, "delay or rate of antenna %d is not finite", a);
    if (aligned && p->num_samp > kAlignMaxSamp)
        return fail(p, FXC_ERR_UNSUPPORTED, "whole-sample delays take chunks of up to 2^27 samples, the plan's have %lld", (long long)p->num_samp);
    if (p->live_pipes) return fail(p, FXC_ERR_STATE, "an fxc_pipe uses the plan");
    if (!acc_empty(p) && !p->acc_track)
        return fail(p, FXC_ERR_STATE, "the accumulator holds chunks accumulated without a delay track: finalize or reset it first");
    FXC_DEVICE(p, p->device);
    // ordered after any queued kernel that still reads the old parameters
    FXC_HIP(p, hipStreamSynchronize(p->stream));
    const size_t A = (size_t)p->n_ant, N = (size_t)p->nchan;
    if (!p->d_track_par) FXC_HIP(p, p->d_track_par.alloc(2 * A));
    if (!p->d_one) {      // (filled before the plan has it: a table that is there is a table of ones)
        DevBuf<cd> d_one;
        FXC_HIP(p, d_one.alloc(N));
        cd one;
        one.x = 1.0;
        one.y = 0.0;
        const std::vector<cd> ones(N, one);
        FXC_HIP(p, hipMemcpy(d_one, ones.data(), N * sizeof(cd), hipMemcpyHostToDevice));
        p->d_one = std::move(d_one);
    }
    FXC_HIP(p, hipMemcpy(p->d_track_par, tau0_s, A * sizeof(double), hipMemcpyHostToDevice));
    FXC_HIP(p, hipMemcpy(p->d_track_par + A, rate_s_per_chunk, A * sizeof(double), hipMemcpyHostToDevice));
    p->track_df = 1.0 / ((double)p->nchan * (1.0 / bandwidth));      // np.fft.fftfreq(nchan, d = 1 / bandwidth), step by step
    p->track_freq = frequency;
    p->track_t = first_chunk;
    p->track = true;
    p->rot_ant = false;
    p->gain_n = 0;      // gains were solved on rows made under one particular track: a new track drops them
    release_gain_q(p);
    p->track_align = aligned;
    if (aligned) {
        p->track_bw = bandwidth;
        p->track_par_h.assign(tau0_s, tau0_s + A);
        p->track_par_h.insert(p->track_par_h.end(), rate_s_per_chunk, rate_s_per_chunk + A);
        return store_sample_shifts(p, nullptr);      // the track's own shifts take the place of static ones
    }
    return FXC_OK;
}

// fxc_set_sample_delays below its checks
int set_sample_delays(fxc_plan* p, const int64_t* shift_samples) {
    FXC_DEVICE(p, p->device);
    // ordered after any queued alignment that still reads the old shifts
    FXC_HIP(p, hipStreamSynchronize(p->stream));
    return store_sample_shifts(p, shift_samples);
}

// fxc_set_track_gains below its checks: `count` gains in all
int set_track_gains(fxc_plan* p, const double* gains_re_im, int64_t n_solutions, int64_t interval, int64_t first_chunk, size_t count) {
    FXC_DEVICE(p, p->device);
    if (n_solutions == 0) {
        FXC_HIP(p, hipStreamSynchronize(p->stream));
        p->gain_n = p->gain_interval = p->gain_first = 0;
        release_gain_q(p);
        return FXC_OK;
    }
    // the new table is complete before the plan changes: a call that fails leaves an earlier gain track in force
    const size_t bytes = count * sizeof(cd);
    DevBuf<cd> g, q;
    if (q.alloc(count) != hipSuccess || g.alloc(count) != hipSuccess) {
        (void)hipGetLastError();
        return fail(p, FXC_ERR_NOMEM, "allocation of 2 x %zu bytes for the gain track failed", bytes);
    }
    hipError_t e = hipMemcpy(g, gains_re_im, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(track_gain_inverse_kernel, dim3(grid_for((int64_t)count, 256, p->cu_count)), dim3(256), 0, p->stream, g.get(),
                           q.get(), p->nchan, (int64_t)count);
        e = hipGetLastError();
    }
    // also ordered after any queued kernel that still reads the old table
    if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
    g.reset();
    if (e != hipSuccess) return fail(p, FXC_ERR_HIP, "forming the gain track's table failed: %s", hipGetErrorString(e));
    p->d_gain_q = std::move(q);
    p->gain_n = n_solutions;
    p->gain_interval = interval;
    p->gain_first = first_chunk;
    return FXC_OK;
}

// fxc_delay_track_tables below its checks
int delay_track_tables(fxc_plan* p, int64_t chunk, double* out_re_im) {
    FXC_DEVICE(p, p->device);
    const size_t bytes = (size_t)p->n_ant * p->nchan * sizeof(cd);
    const int rg = grow(p, p->d_stage[1], bytes);
    if (rg) return rg;
    if (p->track_align)      // the chunk's whole-sample shifts, where the aligned table kernels read them
        if (const int rs = track_shifts_pass(p, chunk, 1)) return rs;
    const int rc = track_tables(p, chunk, 1, static_cast<cd*>(p->d_stage[1].get()), false);
    if (rc) return rc;
    FXC_HIP(p, hipMemcpyAsync(out_re_im, p->d_stage[1], bytes, hipMemcpyDeviceToHost, p->stream));
    FXC_HIP(p, hipStreamSynchronize(p->stream));
    return FXC_OK;
}

// fxc_set_rot below its checks
int set_rot(fxc_plan* p, const double* rot_re_im) {
    if (const int rs = end_track(p)) return rs;
    FXC_DEVICE(p, p->device);
    // ordered after any queued finish kernel that still reads the old table
    FXC_HIP(p, hipStreamSynchronize(p->stream));
    release_gain_q(p);
    FXC_HIP(p, hipMemcpy(p->d_rot, rot_re_im, (size_t)p->nchan * sizeof(cd), hipMemcpyHostToDevice));
    p->rot_ant = false;
    return FXC_OK;
}

// fxc_set_rot_ant below its checks
int set_rot_ant(fxc_plan* p, const double* rot_ant_re_im) {
    if (const int rs = end_track(p)) return rs;
    FXC_DEVICE(p, p->device);
    FXC_HIP(p, hipStreamSynchronize(p->stream));
    release_gain_q(p);
    const size_t N = (size_t)p->nchan;
    const cd* r = reinterpret_cast<const cd*>(rot_ant_re_im);
    if (p->n_ant == 2) {
        // the one baseline's w = r_1 conj(r_0), in float64, into the shared table: every 2-antenna route runs as it is
        std::vector<cd> w(N);
        for (size_t k = 0; k < N; ++k) {
            const cd ra = r[k], rb = r[N + k];
            w[k].x = rb.x * ra.x + rb.y * ra.y;
            w[k].y = rb.y * ra.x - rb.x * ra.y;
        }
        FXC_HIP(p, hipMemcpy(p->d_rot, w.data(), N * sizeof(cd), hipMemcpyHostToDevice));
        p->rot_ant = false;
        return FXC_OK;
    }
    if (!p->d_rot_ant) FXC_HIP(p, p->d_rot_ant.alloc((size_t)p->n_ant * N));
    FXC_HIP(p, hipMemcpy(p->d_rot_ant, r, (size_t)p->n_ant * N * sizeof(cd), hipMemcpyHostToDevice));
    p->rot_ant = true;
    return FXC_OK;
}

}  // namespace
