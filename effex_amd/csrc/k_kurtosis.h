// Part of libfxcorr's single translation unit: included by fxcorr.hip (not a stand-alone header).
#pragma once

namespace {

// ------------------------------------------------------------------------------------------
// spectral kurtosis per antenna (fxcorr.h fxc_kurtosis): over the M frames of a time bin, p_i = |f_a[c,i,k]|^2,
// S1 = sum p_i, S2 = sum p_i^2, sk = (M + 1) / (M - 1) (M S2 / S1^2 - 1), power = S1 / M, from the spectra the plan's F stage wrote
// to the workspace as [chunk][antenna][frame][nchan], natural bin order.  The shape of beam_kernel (k_beam.h): a 64-lane wave
// owns a column of 64 channels, 8-byte loads coalesced across channels, every spectrum read once with the nontemporal hint,
// kKurtLoads of them in flight before the first is used.
//
// The order of the additions is a function of (n_pts, tint) alone.  A bin is cut into segments of kKurtSegment frames from its
// first frame (the last may be partial).  A segment's S1 and S2 are float32 sums from 0 in frame order, by one thread.  The
// bin's sums are the segments' sums added in float64, from 0, in segment order.  Bins of one segment (tint <= kKurtSegment):
// every wave of a workgroup takes kurt bins of its own, and the float64 "sum" is the conversion.  Longer bins: the waves of the
// workgroup take the segments of a round of kKurtWaves, hand their float32 sums over through LDS (two buffers: one barrier a
// round), and every wave adds the round's sums to its own float64 totals in segment order; wave 0 stores.  Which wave summed a
// segment, and how many bins ride in a workgroup, changes no bit.  Every register array is indexed by unrolled loops only.
// ------------------------------------------------------------------------------------------
constexpr int kKurtLanes = 64;
constexpr int kKurtWaves = 4;         // waves of a workgroup
constexpr int kKurtLoads = 8;         // frames a trip: loads in flight per thread
constexpr int kKurtSegment = 64;      // frames of a segment: a float32 sum is never longer

// float32 S1, S2 of the n <= kKurtSegment frames from i0 of the column at s, in frame order from 0; the frames past the end of a
// last, partial trip are read as the segment's last frame and dropped
__device__ __forceinline__ void kurt_segment(const cf* __restrict__ s, int nchan, int64_t i0, int n, float& s1, float& s2) {
#pragma clang fp contract(off)
    s1 = 0.f;
    s2 = 0.f;
    const cf* __restrict__ q = s + i0 * nchan;      // (a segment's rows are within 2^31 elements of its first)
    for (int t = 0; t < n; t += kKurtLoads) {
        cf z[kKurtLoads];
#pragma unroll
        for (int f = 0; f < kKurtLoads; ++f) z[f] = FXC_X_LOAD(q + (t + f < n ? t + f : n - 1) * nchan);
        __builtin_amdgcn_sched_barrier(0);      // every load of the trip is issued before the first is waited for
#pragma unroll
        for (int f = 0; f < kKurtLoads; ++f) {
            if (t + f < n) {
                const float pw = __builtin_fmaf(z[f].y, z[f].y, z[f].x * z[f].x);
                s1 += pw;
                s2 = __builtin_fmaf(pw, pw, s2);
            }
        }
    }
}

// the bin's two outputs from its float64 sums over m frames.  m < 2: sk = 1 exactly (one frame is no evidence); a sum that is not
// finite (a non-finite sample, or |f|^4 beyond float32): NaN; S1 == 0 (a dead stream): 0
__device__ __forceinline__ void kurt_store(double S1, double S2, int64_t m, float* __restrict__ sk, float* __restrict__ power, int64_t at) {
    const double dm = (double)m;
    float v;
    if (m < 2) v = 1.f;
    else if (!(__builtin_isfinite(S1) && __builtin_isfinite(S2))) v = __builtin_nanf("");
    else if (S1 == 0.0) v = 0.f;
    else v = (float)((dm + 1.0) / (dm - 1.0) * (dm * S2 / (S1 * S1) - 1.0));
    sk[at] = v;
    if (power) power[at] = (float)(S1 / dm);
}

// Workgroup (x = column of 64 channels, y = time bin or group of bins, z = chunk * n_ant + antenna of the pass), blockDim.x / 64
// waves.  bpw > 0 (tint <= kKurtSegment): wave w of group g takes the bins (g waves + w) bpw .. + bpw - 1.  bpw == 0: a workgroup
// of kKurtWaves waves takes bin y.  Both walk on by gridDim.y where the bins outnumber the grid.  The lanes past nchan of a last,
// partial column read the last channel and store nothing.  Out: sk, power (may be nullptr) [z][n_tbin][nchan] float32, bin k at
// (k + nchan / 2) % nchan -- numpy's fftshift, odd counts included.
__global__ __launch_bounds__(kKurtLanes * kKurtWaves) void kurtosis_kernel(const cf* __restrict__ spec, float* __restrict__ sk,
                                                                           float* __restrict__ power, int64_t n_pts, int nchan,
                                                                           int64_t tint, int64_t n_tbin, int64_t bpw) {
    __shared__ float part[2][kKurtWaves][2][kKurtLanes];
    const int lane = threadIdx.x % kKurtLanes;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kKurtLanes);
    const int waves = blockDim.x / kKurtLanes;
    const int col = blockIdx.x * kKurtLanes + lane;
    const bool live = col < nchan;      // part of a wave
    const int pos = live ? col : nchan - 1;
    int kout = pos + nchan / 2;
    if (kout >= nchan) kout -= nchan;
    const int64_t ca = blockIdx.z;
    const cf* __restrict__ s = spec + ca * n_pts * nchan + pos;
    const int64_t o = ca * n_tbin * nchan + kout;
    if (bpw > 0) {
        const int64_t per_wg = bpw * waves;
        for (int64_t g = blockIdx.y; g * per_wg < n_tbin; g += gridDim.y) {
            const int64_t j0 = g * per_wg + wave * bpw;
            const int64_t j1 = j0 + bpw < n_tbin ? j0 + bpw : n_tbin;
            for (int64_t j = j0; j < j1; ++j) {
                const int64_t i0 = j * tint;
                const int64_t m = tint < n_pts - i0 ? tint : n_pts - i0;
                float a, b;
                kurt_segment(s, nchan, i0, (int)m, a, b);
                if (live) kurt_store((double)a, (double)b, m, sk, power, o + j * nchan);
            }
        }
        return;
    }
    int buf = 0;
    for (int64_t j = blockIdx.y; j < n_tbin; j += gridDim.y) {
        const int64_t i0 = j * tint;
        const int64_t m = tint < n_pts - i0 ? tint : n_pts - i0;
        const int64_t n_seg = (m + kKurtSegment - 1) / kKurtSegment;
        double S1 = 0.0, S2 = 0.0;
        for (int64_t r0 = 0; r0 < n_seg; r0 += kKurtWaves) {
            const int64_t sg = r0 + wave;
            float a = 0.f, b = 0.f;
            if (sg < n_seg) {
                const int64_t left = m - sg * kKurtSegment;
                kurt_segment(s, nchan, i0 + sg * kKurtSegment, (int)(left < kKurtSegment ? left : kKurtSegment), a, b);
            }
            part[buf][wave][0][lane] = a;
            part[buf][wave][1][lane] = b;
            __syncthreads();
            const int64_t in_round = n_seg - r0;
#pragma unroll
            for (int w = 0; w < kKurtWaves; ++w) {
                if (w < in_round) {
                    S1 += (double)part[buf][w][0][lane];
                    S2 += (double)part[buf][w][1][lane];
                }
            }
            buf ^= 1;      // the next round writes the other buffer: this one is read until every wave has passed the next barrier
        }
        if (wave == 0 && live) kurt_store(S1, S2, m, sk, power, o + j * nchan);
    }
}

// The row weights of fxc_kurtosis_weights: w[c][(a,b)][k'] = 1 iff lo <= sk <= hi for every counted bin of antenna a and of
// antenna b, else 0 -- a conjunction of comparisons in float64, so a NaN gives 0.  sk = [n_chunks][n_ant][n_tbin][nchan]; the bins
// 0 .. n_count - 1 are counted.  One thread per element, the baselines (a, b), a < b, a-major.
__global__ __launch_bounds__(256) void kurtosis_weights_kernel(const float* __restrict__ sk, float* __restrict__ w, int n_ant, int n_base,
                                                               int nchan, int64_t n_tbin, int64_t n_count, int64_t n_chunks, double lo,
                                                               double hi) {
    const int64_t total = n_chunks * n_base * nchan;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        const int k = (int)(idx % nchan);
        const int64_t cb = idx / nchan;
        const int base = (int)(cb % n_base);
        const int64_t c = cb / n_base;
        int a = 0, left = base;      // row `base` of the a-major list
        while (left >= n_ant - 1 - a) {
            left -= n_ant - 1 - a;
            ++a;
        }
        const int b = a + 1 + left;
        const float* __restrict__ sa = sk + ((c * n_ant + a) * n_tbin) * nchan + k;
        const float* __restrict__ sb = sk + ((c * n_ant + b) * n_tbin) * nchan + k;
        bool ok = true;
        for (int64_t j = 0; j < n_count; ++j) {
            const double va = (double)sa[j * nchan], vb = (double)sb[j * nchan];
            ok = ok && lo <= va && va <= hi && lo <= vb && vb <= hi;
        }
        w[idx] = ok ? 1.f : 0.f;
    }
}

// The antenna mask of fxc_kurtosis_antenna_mask: mask[c][a][j][k'] = 1 iff lo_j <= sk <= hi_j, else 0 -- comparisons in float64 on
// the float32 values, so a NaN gives 0.  sk and mask = [n_chunks][n_ant][n_tbin][nchan]; (lo_j, hi_j) = (lo_last, hi_last) for bin
// j >= n_full (a partial last bin that is not the chunk's only bin), (lo, hi) otherwise.  One thread per element.
__global__ __launch_bounds__(256) void kurtosis_mask_kernel(const float* __restrict__ sk, float* __restrict__ mask, int nchan, int64_t n_tbin,
                                                            int64_t n_full, int64_t total, double lo, double hi, double lo_last,
                                                            double hi_last) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        const int64_t j = idx / nchan % n_tbin;
        const bool last = j >= n_full;
        const double v = (double)sk[idx], l = last ? lo_last : lo, h = last ? hi_last : hi;
        mask[idx] = l <= v && v <= h ? 1.f : 0.f;
    }
}

}  // namespace
