// Part of libfxcorr's single translation unit: included by fxcorr.hip (not a stand-alone header).
#pragma once

namespace {

// ------------------------------------------------------------------------------------------
// incoherent dedispersion (fxcorr.h fxc_dedisperse): out[s][d][t] = the sum over the counted channels k of
// P[t + shifts[d][k]][s][k].  The order of the additions is the definition's and the same in both kernels: float32 sums over
// segments of 64 channels from +0 in ascending k, the segments' sums added in float64 in segment order, one rounding to float32.
// The channels are walked in steps of 32, half a segment.  Both kernels read one table (DedTab) in which the channels that do not
// count do not appear: a step's counted channels are listed in ascending order, so a channel is selected away by never being
// visited and its samples are never added.
// ------------------------------------------------------------------------------------------
constexpr int kDedThreads = 256;
constexpr int kDedT = kDedThreads;      // output times of a tile: one a thread
constexpr int kDedD = 8;                // trials of a tile: the accumulators a thread keeps in registers
constexpr int kDedSeg = 64;             // channels of a float32 segment sum (the definition's)
constexpr int kDedStep = 32;            // channels of one LDS pass: half a segment, the float32 sum runs on over the two halves
constexpr int kDedLdsBytes = 160 * 1024;
// the spread of a tile's shifts inside a step at most: T + span samples of a channel, rounded up to an odd count, fit the LDS
constexpr int kDedMaxSpan = kDedLdsBytes / (kDedStep * (int)sizeof(float)) - 1 - kDedT;

// The power of one series as a time series: sample tt lies at p[(tt / n_tbin) c_stride + (tt % n_tbin) nchan + k].  gap =
// c_stride - n_tbin nchan; where it is 0 the driver passes n_tbin = n_t.  Samples from n_t on do not exist.
struct DedIn {
    const float* p;
    int64_t gap;
    unsigned n_tbin, n_t;
    int nchan;
};

// The trial table on the device.  Slot step 32 + i, i < cnt[step], is the i-th counted channel of the step: chan[slot] its index
// and shifts[group][slot][0 .. kDedD) the shifts of the group's trials (the trials past the last repeat the group's first one:
// read, never stored).  bs[group][step] = (base, span): the smallest shift of the group's trials over the step's counted channels
// and the spread above it, (0, 0) where the step has none.
struct DedTab {
    const int* shifts;
    const int* chan;
    const int* cnt;
    const int* bs;
    int n_step, n_dm;
};

// Workgroup x of series z owns the outputs [t_lo + tile T, .. + T) of the kDedD trials of group g = groups[j % ng], with j = x / 8
// and tile = (j / ng) 8 + x % 8; thread i the time t_lo + tile T + i.  (Workgroups x and x + 8 share an L2, so the groups of a tile
// -- which read the same samples -- run next to each other behind one; nothing but speed depends on it.)  Per step of 32 channels:
// the wave's two half-waves load a row each -- 32 channels of one sample, 128 contiguous bytes -- of the window [tile T + base,
// .. + T + span), kDedLoads rows in flight a lane, and store them transposed into LDS, word kl wp + r for channel kl and row r; wp
// is odd, so the 32 lanes of a half-wave, wp words apart, fall on 32 different banks.  Rows from n_t on are stored as zeros; only
// threads without an output read them.  After the barrier thread i reads word kl wp + i + (shift - base) for every counted channel:
// the lanes of a wave read consecutive words, and channel and shift are scalars -- the table is read with scalar loads, a channel's
// kDedD shifts at a time.  The accumulators are indexed by unrolled loops only.
constexpr int kDedLoads = 12;
__global__ void __launch_bounds__(kDedThreads)
dedisperse_tiled_kernel(DedIn in, int64_t s_in, DedTab tb, const int* __restrict__ groups, unsigned ng, unsigned n_tiles, unsigned t_lo,
                        unsigned n_o, float* __restrict__ out, int64_t s_out, int64_t o_stride, int wp) {
    extern __shared__ float ded_lds[];
    const unsigned j = blockIdx.x >> 3;
    const unsigned tile = (j / ng) * 8u + (blockIdx.x & 7u);
    if (tile >= n_tiles) return;
    const int g = groups[j % ng];
    const int nchan = in.nchan, n_step = tb.n_step;
    const float* __restrict__ p = in.p + (int64_t)blockIdx.z * s_in;
    const unsigned x0 = tile * (unsigned)kDedT;
    const int kl = (int)(threadIdx.x & (kDedStep - 1));      // the channel of the step this lane loads
    const unsigned row0 = threadIdx.x / kDedStep;            // its first row; the workgroup loads kRows rows at a time
    constexpr unsigned kRows = kDedThreads / kDedStep;
    const int* __restrict__ shifts_g = static_cast<const int*>(__builtin_assume_aligned(tb.shifts, 32)) + (int64_t)g * n_step * kDedStep * kDedD;
    const int* __restrict__ bs_g = tb.bs + 2 * (int64_t)g * n_step;
    float acc[kDedD];
    double tot[kDedD];
#pragma unroll
    for (int d = 0; d < kDedD; ++d) {
        acc[d] = 0.f;
        tot[d] = 0.0;
    }
    for (int step = 0; step < n_step; ++step) {
        const int k0 = step * kDedStep;
        const int n_c = tb.cnt[step];
        const int base = bs_g[2 * step], span = bs_g[2 * step + 1];
        if (n_c > 0) {      // the same for the whole workgroup
            const unsigned rows = (unsigned)(kDedT + span);
            if (k0 + kl < nchan) {
                unsigned tt = t_lo + x0 + (unsigned)base + row0;
                const unsigned c = tt / in.n_tbin;
                unsigned jj = tt - c * in.n_tbin;
                int64_t off = (int64_t)c * ((int64_t)in.n_tbin * nchan + in.gap) + (int64_t)jj * nchan + (k0 + kl);
                float* __restrict__ col = ded_lds + kl * wp;
                for (unsigned r = row0; r < rows; r += kRows * kDedLoads) {
                    float v[kDedLoads];
#pragma unroll
                    for (int u = 0; u < kDedLoads; ++u) {
                        v[u] = 0.f;
                        if (r + kRows * u < rows && tt < in.n_t) v[u] = p[off];
                        tt += kRows;
                        jj += kRows;
                        off += (int64_t)kRows * nchan;
                        while (jj >= in.n_tbin) {
                            jj -= in.n_tbin;
                            off += in.gap;
                        }
                    }
#pragma unroll
                    for (int u = 0; u < kDedLoads; ++u)
                        if (r + kRows * u < rows) col[r + kRows * u] = v[u];
                }
            }
            __syncthreads();
            const int* __restrict__ ch = tb.chan + k0;
            const int* __restrict__ e = shifts_g + (int64_t)k0 * kDedD;
#pragma unroll 2
            for (int i = 0; i < n_c; ++i) {
                const int rel = (ch[i] - k0) * wp - base;
                int sh[kDedD];
#pragma unroll
                for (int d = 0; d < kDedD; ++d) sh[d] = e[i * kDedD + d];
#pragma unroll
                for (int d = 0; d < kDedD; ++d) acc[d] += ded_lds[(int)threadIdx.x + (rel + sh[d])];      // 0 .. span past the thread
            }
            __syncthreads();
        }
        if ((step & 1) || step == n_step - 1) {      // the segment of 64 channels is complete
#pragma unroll
            for (int d = 0; d < kDedD; ++d) {
                tot[d] += (double)acc[d];
                acc[d] = 0.f;
            }
        }
    }
    const unsigned t = x0 + threadIdx.x;
    if (t >= n_o) return;
    float* __restrict__ o = out + (int64_t)blockIdx.z * s_out + ((int64_t)g * kDedD) * o_stride + t;
#pragma unroll
    for (int d = 0; d < kDedD; ++d)
        if (g * kDedD + d < tb.n_dm) o[d * o_stride] = (float)tot[d];
}

// The trials whose spread does not fit the tile: one thread per (trial, time) reads its samples from memory -- a channel's lanes
// are nchan floats apart -- and adds them in the order of the tiled kernel.  blockIdx.y = entry of `groups` times kDedD + the
// trial within the group.  Any table with 0 <= shift < n_t is served.
__global__ void __launch_bounds__(kDedThreads)
dedisperse_direct_kernel(DedIn in, int64_t s_in, DedTab tb, const int* __restrict__ groups, unsigned t_lo, unsigned n_o,
                         float* __restrict__ out, int64_t s_out, int64_t o_stride) {
    const int g = groups[blockIdx.y / kDedD], i_d = (int)(blockIdx.y % kDedD);
    if (g * kDedD + i_d >= tb.n_dm) return;
    const unsigned t = blockIdx.x * (unsigned)kDedThreads + threadIdx.x;
    if (t >= n_o) return;
    const int nchan = in.nchan, n_step = tb.n_step;
    const float* __restrict__ p = in.p + (int64_t)blockIdx.z * s_in;
    const int* __restrict__ e = tb.shifts + (int64_t)g * n_step * kDedStep * kDedD + i_d;
    const int64_t c_stride = (int64_t)in.n_tbin * nchan + in.gap;
    double tot = 0.0;
    float acc = 0.f;
    for (int step = 0; step < n_step; ++step) {
        const int n_c = tb.cnt[step];
        for (int i = 0; i < n_c; ++i) {
            const int slot = step * kDedStep + i;
            const int k = tb.chan[slot];
            const unsigned tt = t_lo + t + (unsigned)e[(int64_t)slot * kDedD];
            if (in.gap == 0) {
                acc += p[(int64_t)tt * nchan + k];
            } else {
                const unsigned c = tt / in.n_tbin;
                acc += p[(int64_t)c * c_stride + (int64_t)(tt - c * in.n_tbin) * nchan + k];
            }
        }
        if ((step & 1) || step == n_step - 1) {
            tot += (double)acc;
            acc = 0.f;
        }
    }
    out[(int64_t)blockIdx.z * s_out + ((int64_t)g * kDedD + i_d) * o_stride + t] = (float)tot;
}

}  // namespace
