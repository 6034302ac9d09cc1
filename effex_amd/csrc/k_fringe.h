// Part of libfxcorr's single translation unit: included by fxcorr.hip (not a stand-alone header).
#pragma once

namespace {

// ------------------------------------------------------------------------------------------
// fringe fit (fxcorr.h fxc_fringe_fit): the zero-padded 2-D DFT of the SPECTRUM rows of one baseline over
// frequency (delay, index m < Lk) and over the chunks (fringe rate, index q < Lt), and the arg-max of its magnitude.
//   gather   rows of the baselines (ref, b) -> G0[b][t][Lk], conjugated where b < ref, zero-padded; sum |R|^2 in fixed order
//            (fxc_fringe_fit_weighted with weights: fringe_gather_weighted_kernel, the rows times their weights, any list of rows)
//   frequency axis: the batched Stockham stages of k_delay.h over the n_chunks rows of every baseline -> G[b][t][m]
//   time axis + peak (fringe_time_peak_kernel): a tile of adjacent delay columns in LDS, Lt-point transforms in place,
//            |F|^2 and one packed arg-max word per baseline; the 2-D spectrum never reaches HBM
//   stencil  the peak and its four neighbours again, in float64, from G
// Every value depends on its baseline's rows alone, never on how the baselines are batched.
// ------------------------------------------------------------------------------------------
constexpr int kFringeBatch = 64;        // baselines per batch at most (a plan has up to 64 antennas)
constexpr int kFringeParts = 128;       // partial sums of |R|^2 per baseline: the grid of the gather, fixed for a fixed order
constexpr int kFringeThreads = 256;
constexpr int kFringeLdsBytes = 80 * 1024;   // two workgroups a CU
struct FringeRows {
    int64_t off[kFringeBatch];          // element offset of chunk 0 of the baseline's row
    int conj[kFringeBatch];             // 1: the row is (b, ref), R is its conjugate
};

// g0[q][t][j] = R_q[t][j] for j < nchan, 0 up to lk; part[q][blockIdx.x] = this workgroup's share of sum |R|^2 (float64)
__global__ void __launch_bounds__(kFringeThreads)
fringe_gather_kernel(const cf* __restrict__ rows, FringeRows br, int64_t t_stride, cf* __restrict__ g0, double* __restrict__ part,
                     int n_chunks, int nchan, int lk_log) {
    __shared__ double red[kFringeThreads / 64];
    const int q = blockIdx.y;
    const cf* __restrict__ src = rows + br.off[q];
    const float sgn = br.conj[q] ? -1.f : 1.f;
    cf* __restrict__ dst = g0 + (((int64_t)q * n_chunks) << lk_log);
    const int64_t total = (int64_t)n_chunks << lk_log;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    double acc = 0.0;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        const int64_t t = idx >> lk_log;
        const int j = (int)(idx & ((1ll << lk_log) - 1));
        cf v = fxc::mk(0.f, 0.f);
        if (j < nchan) {
            v = src[t * t_stride + j];
            v.y *= sgn;
            acc += (double)v.x * (double)v.x + (double)v.y * (double)v.y;
        }
        dst[idx] = v;
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = red[0];
        for (int w = 1; w < kFringeThreads / 64; ++w) s += red[w];
        part[(int64_t)q * kFringeParts + blockIdx.x] = s;
    }
}

// The gather of fxc_fringe_fit_weighted: g0[q][t][j] = Rw_q[t][j] = w > 0 ? (w x, w y) : (+0, +0) with (x, y) = R_q[t][j] and
// w = weights at the same place (off[q] + t w_stride + j: a baseline's weights lie like its rows); part as above, of |Rw|^2.
// Rows (8 bytes a lane) and weights (4 bytes a lane) are read once each; the sample and its weight are selected first and
// multiplied after, so what a sample that does not count holds (NaN, Inf, 1e30) never meets an operation.  The loop, the
// lanes and the order of the sums are the plain gather's: weights of 1.0f give its g0 and its partial sums bit for bit.
// wmax[q] (zeroed by the caller) = the largest counted weight of the baseline as float bits: positive floats order like their
// bits, and a maximum does not depend on the order it is taken in.
__global__ void __launch_bounds__(kFringeThreads)
fringe_gather_weighted_kernel(const cf* __restrict__ rows, const float* __restrict__ weights, FringeRows br, int64_t t_stride,
                              int64_t w_stride, cf* __restrict__ g0, double* __restrict__ part, unsigned* __restrict__ wmax,
                              int n_chunks, int nchan, int lk_log) {
    __shared__ double red[kFringeThreads / 64];
    const int q = blockIdx.y;
    const cf* __restrict__ src = rows + br.off[q];
    const float* __restrict__ wsrc = weights + br.off[q];
    const float sgn = br.conj[q] ? -1.f : 1.f;
    cf* __restrict__ dst = g0 + (((int64_t)q * n_chunks) << lk_log);
    const int64_t total = (int64_t)n_chunks << lk_log;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    double acc = 0.0;
    float wm = 0.f;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        const int64_t t = idx >> lk_log;
        const int j = (int)(idx & ((1ll << lk_log) - 1));
        cf v = fxc::mk(0.f, 0.f);
        if (j < nchan) {
            const cf r = src[t * t_stride + j];
            const float w = wsrc[t * w_stride + j];
            const bool live = w > 0.f;                  // false for 0, negative and NaN weights
            const float wl = live ? w : 0.f;
            wm = wl > wm ? wl : wm;
            v.x = wl * (live ? r.x : 0.f);
            v.y = wl * (live ? r.y * sgn : 0.f);
            acc += (double)v.x * (double)v.x + (double)v.y * (double)v.y;
        }
        dst[idx] = v;
    }
    for (int off = 32; off > 0; off >>= 1) {
        acc += __shfl_down(acc, off);
        const float o = __shfl_down(wm, off);
        wm = o > wm ? o : wm;
    }
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6] = acc;
        atomicMax(wmax + q, __float_as_uint(wm));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = red[0];
        for (int w = 1; w < kFringeThreads / 64; ++w) s += red[w];
        part[(int64_t)q * kFringeParts + blockIdx.x] = s;
    }
}

// LDS image of a tile: element (pos, c), c < 2^tm_log the column, one cf of skew `pad` per 16 positions so that the
// butterflies of the last stage (16 consecutive positions each) of one 32-lane group fall on different banks
__device__ __forceinline__ int fringe_idx(int pos, int c, int tm_log, int pad) { return (pos << tm_log) + c + (pos >> 4) * pad; }

// one in-place decimation-in-frequency stage of radix R over every column of the tile: the sub-transforms have length
// n = R s; butterfly (block, j < s) takes positions block n + j + a s, a < R, and leaves output r, times w_n^(j r), at
// position block n + j + r s.  Kernel exp(+2 pi i ..) on conjugated data, as in k_delay.h.  A thread reads and writes the
// same R places and no other thread touches them: no barrier inside a stage.
template <int R>
__device__ __forceinline__ void fringe_stage(cf* __restrict__ tile, const cf* __restrict__ tw, int lt_log, int s_log, int tm_log,
                                             int pad) {
    constexpr int r_log = R == 16 ? 4 : (R == 8 ? 3 : (R == 4 ? 2 : 1));
    const int s = 1 << s_log;
    const int n_mask = (R << s_log) - 1;
    const int tw_shift = lt_log - s_log - r_log;          // w_n^x = tw[x Lt / n]
    const int total = 1 << (lt_log - r_log + tm_log);     // butterflies x columns
    for (int id = threadIdx.x; id < total; id += kFringeThreads) {
        const int c = id & ((1 << tm_log) - 1);
        const int bidx = id >> tm_log;
        const int j = bidx & (s - 1);
        const int base = ((bidx - j) << r_log) + j;
        cf v[16];
#pragma unroll
        for (int a = 0; a < R; ++a) v[a] = tile[fringe_idx(base + (a << s_log), c, tm_log, pad)];
        if (R == 16) {
            fxc::dft16(v);
        } else if (R == 8) {
            fxc::tiled::dft8(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
        } else if (R == 4) {
            fxc::dft4(v[0], v[1], v[2], v[3]);
        } else {
            fxc::tiled::dft2(v[0], v[1]);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            cf y = v[r];
            if (r > 0 && s > 1) y = fxc::cmul(y, tw[((j * r) & n_mask) << tw_shift]);
            tile[fringe_idx(base + (r << s_log), c, tm_log, pad)] = y;
        }
    }
}

// Time axis and peak.  Workgroup (x, y) takes the 2^tm_log delay columns m0 = x 2^tm_log .. of baseline y: its reads of
// g[y][t][m0 ..] run along m.  The columns go into LDS conjugated and zero-padded to Lt, are transformed in place -- one
// stage of radix 2^first_log (the bits of log2 Lt that radix 16 leaves over; 16 itself when there are none), then radix-16
// stages -- and position pos = r_1 Lt/R_1 + r_2 Lt/(R_1 16) + .. then holds conj F[q][m], q = r_1 + R_1 (r_2 + 16 (r_3 + ..)).
// best[y] = max over (q, m) of (|F|^2 as ordered bits << 32 | ~(q Lk + m)): the first maximum in row-major order wins.
__global__ void __launch_bounds__(kFringeThreads)
fringe_time_peak_kernel(const cf* __restrict__ g, unsigned long long* __restrict__ best, int n_chunks, int lk_log, int lt_log,
                        int tm_log, int pad, int first_log) {
    extern __shared__ __align__(16) unsigned char fringe_lds[];
    const int lt = 1 << lt_log;
    cf* tw = reinterpret_cast<cf*>(fringe_lds);          // [Lt] exp(+2 pi i x / Lt)
    cf* tile = tw + lt;
    const int tm = 1 << tm_log;
    const int m0 = blockIdx.x << tm_log;
    g += (((int64_t)blockIdx.y * n_chunks) << lk_log) + m0;
    for (int x = threadIdx.x; x < lt; x += kFringeThreads) {
        double sn, cs;
        sincospi(2.0 * (double)x / (double)lt, &sn, &cs);
        tw[x] = fxc::mk((float)cs, (float)sn);
    }
    for (int id = threadIdx.x; id < (lt << tm_log); id += kFringeThreads) {
        const int c = id & (tm - 1);
        const int t = id >> tm_log;
        cf v = fxc::mk(0.f, 0.f);
        if (t < n_chunks) {
            v = g[((int64_t)t << lk_log) + c];
            v.y = -v.y;
        }
        tile[fringe_idx(t, c, tm_log, pad)] = v;
    }
    __syncthreads();
    int s_log = lt_log - first_log;
    if (first_log == 4) fringe_stage<16>(tile, tw, lt_log, s_log, tm_log, pad);
    else if (first_log == 3) fringe_stage<8>(tile, tw, lt_log, s_log, tm_log, pad);
    else if (first_log == 2) fringe_stage<4>(tile, tw, lt_log, s_log, tm_log, pad);
    else fringe_stage<2>(tile, tw, lt_log, s_log, tm_log, pad);
    while (s_log > 0) {
        __syncthreads();
        s_log -= 4;
        fringe_stage<16>(tile, tw, lt_log, s_log, tm_log, pad);
    }
    __syncthreads();
    unsigned long long loc = 0;
    for (int id = threadIdx.x; id < (lt << tm_log); id += kFringeThreads) {
        const int c = id & (tm - 1);
        const int pos = id >> tm_log;
        // digits of pos, most significant first, are the digits of q, least significant first
        int sub_log = lt_log - first_log;
        int q = pos >> sub_log;
        int rem = pos & ((1 << sub_log) - 1);
        int mul_log = first_log;
        while (sub_log > 0) {
            sub_log -= 4;
            q += (rem >> sub_log) << mul_log;
            rem &= (1 << sub_log) - 1;
            mul_log += 4;
        }
        const cf v = tile[fringe_idx(pos, c, tm_log, pad)];
        const float mag = v.x * v.x + v.y * v.y;
        const unsigned lin = ((unsigned)q << lk_log) + (unsigned)(m0 + c);
        const unsigned long long key = ((unsigned long long)__float_as_uint(mag) << 32) | (0xFFFFFFFFull - lin);
        loc = key > loc ? key : loc;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(loc, off);
        loc = o > loc ? o : loc;
    }
    if ((threadIdx.x & 63) == 0) atomicMax(best + blockIdx.y, loc);
}

// out[y][5] (re, im as float64) = F at the peak (q0, m0) of baseline y, at (q0, m0 -+ 1) and at (q0 -+ 1, m0), indices
// wrapping: F[q][m] = sum_t g[t][m] exp(-2 pi i t q / Lt), n_chunks terms in float64, summed in a fixed order
__global__ void __launch_bounds__(kFringeThreads)
fringe_stencil_kernel(const cf* __restrict__ g, const unsigned long long* __restrict__ best, double* __restrict__ out,
                      int n_chunks, int lk_log, int lt_log) {
    __shared__ double red[kFringeThreads][2];
    g += ((int64_t)blockIdx.x * n_chunks) << lk_log;
    const unsigned lin = (unsigned)(0xFFFFFFFFull - (best[blockIdx.x] & 0xFFFFFFFFull));
    const int lk_mask = (1 << lk_log) - 1, lt_mask = (1 << lt_log) - 1;
    const int q0 = (int)(lin >> lk_log) & lt_mask, m0 = (int)lin & lk_mask;
    for (int k = 0; k < 5; ++k) {
        const int m = (m0 + (k == 1 ? -1 : (k == 2 ? 1 : 0))) & lk_mask;
        const int q = (q0 + (k == 3 ? -1 : (k == 4 ? 1 : 0))) & lt_mask;
        double re = 0.0, im = 0.0;
        for (int t = threadIdx.x; t < n_chunks; t += kFringeThreads) {
            const cf v = g[((int64_t)t << lk_log) + m];
            const int x = (int)(((int64_t)t * q) & lt_mask);
            double sn, cs;
            sincospi(2.0 * (double)x / (double)(lt_mask + 1), &sn, &cs);
            re += (double)v.x * cs + (double)v.y * sn;
            im += (double)v.y * cs - (double)v.x * sn;
        }
        red[threadIdx.x][0] = re;
        red[threadIdx.x][1] = im;
        __syncthreads();
        for (int h = kFringeThreads / 2; h > 0; h >>= 1) {
            if ((int)threadIdx.x < h) {
                red[threadIdx.x][0] += red[threadIdx.x + h][0];
                red[threadIdx.x][1] += red[threadIdx.x + h][1];
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            out[((int64_t)blockIdx.x * 5 + k) * 2] = red[0][0];
            out[((int64_t)blockIdx.x * 5 + k) * 2 + 1] = red[0][1];
        }
        __syncthreads();
    }
}

}  // namespace
