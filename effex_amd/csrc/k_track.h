// Part of libfxcorr's single translation unit: included by fxcorr.hip (not a stand-alone header).
#pragma once

namespace {

// ------------------------------------------------------------------------------------------
// delay track (fxc_set_delay_track): the rot of antenna a at chunk t is
//     r_a[k](t) = exp(+2 pi i f_k tau_a(t)),  tau_a(t) = tau0[a] + t rate[a],  f_k = fftfreq(nchan, 1 / bandwidth)[k] + frequency
// The phase is 9e3 rad and more (1.42 GHz x 1 us), so f_k tau is formed in turns in float64, rounded once, reduced by rint
// (exact) and handed to sincospi.  Every step is an individually rounded float64 operation in the order numpy takes them for
// np.fft.fftfreq(..) + frequency and tau0 + t * rate (no contraction to fused multiply-adds), so a table depends on (a, k, t)
// alone: not on where a pass or a call started.
// ------------------------------------------------------------------------------------------
struct TrackPar {
    const double* tau0;      // [n_ant]
    const double* rate;      // [n_ant] seconds per chunk
    double df;               // 1 / (nchan * (1 / bandwidth)): numpy's bin spacing
    double frequency;
};

__device__ __forceinline__ cd track_phasor(const TrackPar& tp, int a, int k, int nchan, int64_t t) {
#pragma clang fp contract(off)      // every product and sum below is rounded on its own, as numpy rounds them
    const int kk = k < (nchan + 1) / 2 ? k : k - nchan;
    const double f = (double)kk * tp.df + tp.frequency;
    const double tau = tp.tau0[a] + (double)t * tp.rate[a];
    const double turns = f * tau;
    cd r;
    sincospi(2.0 * (turns - rint(turns)), &r.y, &r.x);
    return r;
}

// PAIR = false: out[t - t0][a][k] = r_a[k](t), the tables of 3 and more antennas (and of fxc_delay_track_tables)
// PAIR = true:  out[t - t0][k] = r_1 conj(r_0), the one baseline of two antennas (what fxc_set_rot_ant folds on the host)
template <bool PAIR>
__global__ void track_tables_kernel(TrackPar tp, cd* __restrict__ out, int n_ant, int nchan, int64_t t0, int64_t n_t) {
    const int rows = PAIR ? 1 : n_ant;
    const int64_t total = n_t * rows * nchan;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        const int k = (int)(idx % nchan);
        const int64_t ta = idx / nchan;
        const int64_t t = t0 + ta / rows;
        if constexpr (PAIR) {
            const cd ra = track_phasor(tp, 0, k, nchan, t), rb = track_phasor(tp, 1, k, nchan, t);
            cd w;
            w.x = rb.x * ra.x + rb.y * ra.y;
            w.y = rb.y * ra.x - rb.x * ra.y;
            out[idx] = w;
        } else {
            out[idx] = track_phasor(tp, (int)(ta % rows), k, nchan, t);
        }
    }
}

// ------------------------------------------------------------------------------------------
// gain track (fxc_set_track_gains): chunk t takes solution s(t) = clamp(floor((t - first_chunk) / interval), 0, n_solutions - 1)
// and the table of antenna a becomes r_a[k](t) = phasor_a[k](t) * q[s(t)][a][k], q = 1 / g in natural bin order.  Both steps
// are individually rounded float64 operations (no contraction), so a table still depends on (a, k, t) and the gain track alone,
// and with every gain 1 it is the plain track's table.
// ------------------------------------------------------------------------------------------
struct GainTrack {
    const cd* q;             // [n_solutions][n_ant][nchan], natural bin order
    int64_t n_solutions;
    int64_t interval;        // >= 1 (one solution for every chunk: n_solutions == 1)
    int64_t first_chunk;
};

__device__ __forceinline__ int64_t gain_solution(const GainTrack& gt, int64_t t) {
    const int64_t d = t - gt.first_chunk;
    if (d <= 0 || gt.n_solutions == 1) return 0;
    const int64_t s = d / gt.interval;
    return s < gt.n_solutions ? s : gt.n_solutions - 1;
}

__device__ __forceinline__ cd gain_apply(cd r, cd q) {
#pragma clang fp contract(off)
    cd o;
    o.x = r.x * q.x - r.y * q.y;
    o.y = r.x * q.y + r.y * q.x;
    return o;
}

// q[s][a][k] = 1 / g[s][a][(k + nchan / 2) % nchan]: the rows' fftshifted order back to natural order (numpy's ifftshift, odd
// channel counts included) and the inverse (x / d, -y / d), d = x x + y y, 0 where g is 0 so that a dead channel stays zero.
// Once per fxc_set_track_gains; total = n_solutions n_ant nchan.
__global__ __launch_bounds__(256) void track_gain_inverse_kernel(const cd* __restrict__ g, cd* __restrict__ q, int nchan, int64_t total) {
#pragma clang fp contract(off)
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int half = nchan / 2;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        const int k = (int)(idx % nchan);
        int j = k + half;
        if (j >= nchan) j -= nchan;
        const cd v = g[idx - k + j];
        const double d = v.x * v.x + v.y * v.y;
        cd o;
        o.x = 0.0;
        o.y = 0.0;
        if (d != 0.0) {
            o.x = v.x / d;
            o.y = -v.y / d;
        }
        q[idx] = o;
    }
}

// track_tables_kernel with the multiply by q[s(t)][a][k]: one coalesced 16-byte load per table element beside the store
// PAIR = true: r_0, r_1 with their gains, then w = r_1 conj(r_0) as track_tables_kernel<true> forms it
template <bool PAIR>
__global__ void track_gain_tables_kernel(TrackPar tp, GainTrack gt, cd* __restrict__ out, int n_ant, int nchan, int64_t t0, int64_t n_t) {
    const int rows = PAIR ? 1 : n_ant;
    const int64_t total = n_t * rows * nchan;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        const int k = (int)(idx % nchan);
        const int64_t ta = idx / nchan;
        const int64_t t = t0 + ta / rows;
        const cd* q = gt.q + gain_solution(gt, t) * n_ant * nchan + k;
        if constexpr (PAIR) {
            const cd ra = gain_apply(track_phasor(tp, 0, k, nchan, t), q[0]);
            const cd rb = gain_apply(track_phasor(tp, 1, k, nchan, t), q[nchan]);
            cd w;
            w.x = rb.x * ra.x + rb.y * ra.y;
            w.y = rb.y * ra.x - rb.x * ra.y;
            out[idx] = w;
        } else {
            const int a = (int)(ta % rows);
            out[idx] = gain_apply(track_phasor(tp, a, k, nchan, t), q[(int64_t)a * nchan]);
        }
    }
}

// ------------------------------------------------------------------------------------------
// aligned track (fxc_set_delay_track_aligned): chunk t's samples of antenna a are read s = s_a(t) whole samples later
// (k_align.h), which has already undone the baseband slope kk s / nchan turns of the table; the table keeps the rest:
//     u = f_k tau - rint(f_k tau),  m = (kk s) mod nchan (integers, non-negative),  v = u - m / nchan,
//     r_a[k](t) = exp(2 pi i (v - rint(v)))
// every operation rounded on its own, as in track_phasor.  s comes from the array track_shifts_kernel wrote for the pass,
// shifts[(t - t0) n_ant + a]: the same integer the alignment of chunk t used.  Sibling kernels: the plain track's
// instantiations above are untouched.  GAIN: times q[s(t)][a][k], as track_gain_tables_kernel.
// ------------------------------------------------------------------------------------------
struct TrackAlign {
    const int* shifts;       // [n_t][n_ant]
    int64_t t0;              // the chunk of shifts[0]
};

__device__ __forceinline__ cd track_phasor_aligned(const TrackPar& tp, const TrackAlign& al, int n_ant, int a, int k, int nchan, int64_t t) {
#pragma clang fp contract(off)
    const int kk = k < (nchan + 1) / 2 ? k : k - nchan;
    const double f = (double)kk * tp.df + tp.frequency;
    const double tau = tp.tau0[a] + (double)t * tp.rate[a];
    const double turns = f * tau;
    const double u = turns - rint(turns);
    int64_t m = ((int64_t)kk * (int64_t)al.shifts[(t - al.t0) * n_ant + a]) % nchan;
    if (m < 0) m += nchan;
    const double v = u - (double)m / (double)nchan;
    cd r;
    sincospi(2.0 * (v - rint(v)), &r.y, &r.x);
    return r;
}

template <bool PAIR, bool GAIN>
__global__ void track_tables_aligned_kernel(TrackPar tp, TrackAlign al, GainTrack gt, cd* __restrict__ out, int n_ant, int nchan, int64_t t0,
                                            int64_t n_t) {
#pragma clang fp contract(off)
    const int rows = PAIR ? 1 : n_ant;
    const int64_t total = n_t * rows * nchan;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        const int k = (int)(idx % nchan);
        const int64_t ta = idx / nchan;
        const int64_t t = t0 + ta / rows;
        const cd* q = nullptr;
        if constexpr (GAIN) q = gt.q + gain_solution(gt, t) * n_ant * nchan + k;
        if constexpr (PAIR) {
            cd ra = track_phasor_aligned(tp, al, n_ant, 0, k, nchan, t), rb = track_phasor_aligned(tp, al, n_ant, 1, k, nchan, t);
            if constexpr (GAIN) {
                ra = gain_apply(ra, q[0]);
                rb = gain_apply(rb, q[nchan]);
            }
            cd w;
            w.x = rb.x * ra.x + rb.y * ra.y;
            w.y = rb.y * ra.x - rb.x * ra.y;
            out[idx] = w;
        } else {
            const int a = (int)(ta % rows);
            cd r = track_phasor_aligned(tp, al, n_ant, a, k, nchan, t);
            if constexpr (GAIN) r = gain_apply(r, q[(int64_t)a * nchan]);
            out[idx] = r;
        }
    }
}

// Tracked integration: acc[p][k] +=(sum over the splits and leading parts of chunk c's raw row p) * conj(w_c[k]), chunk after
// chunk in the order of the stream, in float64 with explicit fused multiply-adds -- so the accumulator after chunks t0 .. t1 is
// the same bits whatever calls and passes brought them.  The accumulator is in natural bin order and holds rotated sums
// (auto rows: the plain sum of the real parts); the raw rows are the ones the rows kernels read (one row set per chunk).
// Thread = accumulator element: every raw element is read once.  Two antennas have only nchan elements, so the chunks whose
// rows are complete (one split, before the leading parts' tail) go eight at a time with their loads in flight together.
constexpr int kTrackFoldU = 8;

template <bool ANT>
__device__ __forceinline__ void track_fold_add(cd& a, double xr, double xi, const RotArg<ANT>& rot, int prow, int k, int nchan) {
    cd w;
    if constexpr (ANT)
        w = ant_rot(rot, prow, k, nchan);
    else
        w = rot[k];
    a.x = fma(xi, w.y, fma(xr, w.x, a.x));
    a.y = fma(-xr, w.y, fma(xi, w.x, a.y));
}

template <bool ANT>
__global__ __launch_bounds__(256) void track_fold_kernel(const cf* __restrict__ raw, cd* __restrict__ acc, TrackRot<ANT> rot,
                                                         int nchan, int64_t n_chunks, int n_splits, int64_t split_stride,
                                                         int slots, LeadRows lead, int n_prod, int n_cross) {
    const int64_t n = (int64_t)n_prod * nchan;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    // chunks before this one have one complete row each
    int64_t plain = 0;
    if (n_splits == 1) plain = lead.n_frames == 0 ? n_chunks : (slots == 3 ? lead.first_chunk / 2 : lead.first_chunk);
    if (plain > n_chunks) plain = n_chunks;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += stride) {
        const int k = (int)(idx % nchan);
        const int prow = (int)(idx / nchan);
        const bool au = prow >= n_cross;
        const cf* src = raw + (int64_t)prow * nchan + raw_index(k, slots);
        cd a = acc[idx];
        int64_t c = 0;
        for (; c + kTrackFoldU <= plain; c += kTrackFoldU) {
            cf r[kTrackFoldU];
#pragma unroll
            for (int u = 0; u < kTrackFoldU; ++u) r[u] = src[(c + u) * n];
#pragma unroll
            for (int u = 0; u < kTrackFoldU; ++u) {
                if (au)
                    a.x += (double)r[u].x;
                else
                    track_fold_add<ANT>(a, (double)r[u].x, (double)r[u].y, chunk_rot<ANT>(rot, c + u, 1), prow, k, nchan);
            }
        }
        for (; c < n_chunks; ++c) {
            const int64_t row = c * n_prod + prow;
            double xr = 0.0, xi = 0.0;
            sum_splits(src + c * n, n_splits, split_stride, xr, xi);
            float lr_re = 0.f, lr_im = 0.f;
            add_lead_rows(raw, lead, row, nchan, k, slots, lr_re, lr_im);
            xr += lr_re;
            xi += lr_im;
            if (au)
                a.x += xr;
            else
                track_fold_add<ANT>(a, xr, xi, chunk_rot<ANT>(rot, c, 1), prow, k, nchan);
        }
        acc[idx] = a;
    }
}

}  // namespace
