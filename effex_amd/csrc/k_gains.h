// Part of libfxcorr's single translation unit: included by fxcorr.hip (not a stand-alone header).
#pragma once

namespace {

// ------------------------------------------------------------------------------------------
// gain solve (fxcorr.h fxc_solve_gains and fxc_solve_gains_weighted): per solution interval and per bin,
// the complex gains g_a whose products g_a conj(g_b) fit the averaged cross rows in the least-squares sense.  One average body
// and one solve body, each compiled twice: plain, and WEIGHTED with a weight per sample and a model visibility per baseline and
// bin.
//   average  plain: rows [chunk][row][bin] complex64 -> V [interval][baseline][bin] complex128: the interval's chunks added in
//            float64 in ascending chunk order, then divided by their number.  A launch may hold only part of an interval's
//            chunks (host rows come in batches): it then continues the sum that the launch before left in V, so the adds
//            and their order -- and with them every bit -- are those of one pass over all chunks.
//            WEIGHTED: rows and weights [chunk][baseline][bin] -> U [interval][baseline][bin] complex128 and D [..] float64:
//            S = sum of w v and Sw = sum of w over the samples with w > 0, in the same order and continued from launch to launch
//            like V; the launch with the interval's last chunk divides by the number of chunks and applies the model:
//            U = (S / n) conj(M), D = (Sw / n) |M|^2.
//   solve    a tile of adjacent bins of one interval in LDS, a thread per (antenna, bin), the iteration in float64.  WEIGHTED:
//            U for V and the denominator sum over D_ab |g_b|^2; D is an LDS plane of its own.
// ------------------------------------------------------------------------------------------
constexpr int kGainsThreads = 256;
constexpr int kGainsUnroll = 16;             // loads of 16 bytes a thread keeps in flight
constexpr int kGainsLdsBytes = 144 * 1024;   // the solve's tile: 64 antennas x 4 bins are 134 KiB
constexpr int kGainsMaxTile = 64;            // bins of a tile at most
constexpr int kGainsTileBytes = 16;          // LDS per baseline and bin: V complex128
constexpr int kGainsWeightedTileBytes = 24;  // the same, WEIGHTED: U complex128 + D float64
constexpr int kGainsImageBytes = 32;         // LDS per antenna and bin: two complex128 gain images

// (wq, x, y) = w > 0 ? (w, re, im) : (0, 0, 0): a flagged sample (weight zero, negative or NaN) becomes weight 0 and value 0
// before any arithmetic sees it.  One compare and three conditional moves, written out so that they stay moves: left to the
// compiler the shared condition becomes a divergent branch around every sample's adds.
__device__ __forceinline__ void gains_flag(float w, float re, float im, float& wq, float& x, float& y) {
    asm("v_cmp_lt_f32_e32 vcc, 0, %3\n\tv_cndmask_b32_e32 %0, 0, %3, vcc\n\tv_cndmask_b32_e32 %1, 0, %4, vcc\n\t"
        "v_cndmask_b32_e32 %2, 0, %5, vcc"
        : "=&v"(wq), "=&v"(x), "=&v"(y)
        : "v"(w), "v"(re), "v"(im)
        : "vcc");
}

// adds the bins (k0, k0 + 1) of N consecutive chunks to the sums of bin k0, then of bin k0 + 1, in chunk order; the loads of
// all N are issued before the first add.  Plain: acc = (re, im) per bin.  WEIGHTED: acc = (S re, S im, Sw) per bin; a sample
// whose weight is not > 0 adds zeros, whatever its value holds; wsrc NULL (the same for every thread of the launch): no weight
// is read, every weight is 1.  VEC: one 16-byte row load (and one 8-byte weight load) per chunk, else 8-byte (and 4-byte) loads
// per bin.  The addresses are a base that is the same for the whole workgroup plus the thread's 32-bit k0.
template <bool WEIGHTED, int N, bool VEC>
__device__ __forceinline__ void gains_add_chunks(const cf* __restrict__ src, int64_t c_stride, const float* __restrict__ wsrc,
                                                 int64_t w_stride, unsigned k0, bool two, double (&acc)[WEIGHTED ? 6 : 4]) {
    typedef float v4f __attribute__((ext_vector_type(4)));
    typedef float v2f __attribute__((ext_vector_type(2)));
    if (VEC) two = true;      // an even channel count: every thread has both bins
    v4f v[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const cf* q = src + i * c_stride + k0;
        if (VEC) {
            v[i] = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(q));
        } else {
            const cf u0 = fxc::nt_load(q);
            v[i] = v4f{u0.x, u0.y, 0.f, 0.f};
            if (two) {
                const cf u1 = fxc::nt_load(q + 1);
                v[i][2] = u1.x;
                v[i][3] = u1.y;
            }
        }
    }
    if constexpr (WEIGHTED) {
        v2f w[N];
        if (wsrc) {
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const float* qw = wsrc + i * w_stride + k0;
                if (VEC) {
                    w[i] = __builtin_nontemporal_load(reinterpret_cast<const v2f*>(qw));
                } else {
                    w[i] = v2f{__builtin_nontemporal_load(qw), 0.f};
                    if (two) w[i][1] = __builtin_nontemporal_load(qw + 1);
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < N; ++i) w[i] = v2f{1.f, two ? 1.f : 0.f};
        }
#pragma unroll
        for (int i = 0; i < N; ++i) {
            float wq, x, y;
            gains_flag(w[i][0], v[i][0], v[i][1], wq, x, y);
            const double w0 = (double)wq;
            acc[0] += w0 * (double)x;              // float32 x float32 is exact in float64
            acc[1] += w0 * (double)y;
            acc[2] += w0;
            __builtin_amdgcn_sched_barrier(0);     // bin after bin, chunk after chunk: few converted values at a time
            gains_flag(w[i][1], v[i][2], v[i][3], wq, x, y);
            const double w1 = (double)wq;
            acc[3] += w1 * (double)x;
            acc[4] += w1 * (double)y;
            acc[5] += w1;
            __builtin_amdgcn_sched_barrier(0);
        }
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            acc[0] += (double)v[i][0];
            acc[1] += (double)v[i][1];
            acc[2] += (double)v[i][2];
            acc[3] += (double)v[i][3];
        }
    }
}

// the chunks [lo, hi) of one thread in ascending order: blocks of kGainsUnroll (of half as many on the narrow-load path, whose
// chunk takes twice the loads: the same number in flight), then halving blocks down to 1 for the rest
template <bool WEIGHTED, int N, bool VEC>
__device__ __forceinline__ void gains_rest(const cf* __restrict__& src, int64_t c_stride, const float* __restrict__& wsrc, int64_t w_stride,
                                           unsigned k0, int left, bool two, double (&acc)[WEIGHTED ? 6 : 4]) {
    if (left & N) {
        gains_add_chunks<WEIGHTED, N, VEC>(src, c_stride, wsrc, w_stride, k0, two, acc);
        src += N * c_stride;
        if (WEIGHTED && wsrc) wsrc += N * w_stride;
    }
    if constexpr (N > 1) gains_rest<WEIGHTED, N / 2, VEC>(src, c_stride, wsrc, w_stride, k0, left, two, acc);
}

template <bool WEIGHTED, bool VEC>
__device__ __forceinline__ void gains_walk(const cf* __restrict__ src, int64_t c_stride, const float* __restrict__ wsrc, int64_t w_stride,
                                           unsigned k0, int64_t lo, int64_t hi, bool two, double (&acc)[WEIGHTED ? 6 : 4]) {
    constexpr int kBlock = VEC ? kGainsUnroll : kGainsUnroll / 2;
    int64_t c = lo;
    for (; c + kBlock <= hi; c += kBlock, src += kBlock * c_stride) {
        gains_add_chunks<WEIGHTED, kBlock, VEC>(src, c_stride, wsrc, w_stride, k0, two, acc);
        if (WEIGHTED && wsrc) wsrc += kBlock * w_stride;
    }
    gains_rest<WEIGHTED, kBlock / 2, VEC>(src, c_stride, wsrc, w_stride, k0, (int)(hi - c), two, acc);
}

// Thread (x, y = baseline, z = interval - s_first) owns bins 2 x and 2 x + 1.  `rows` is the row set of chunk c_lo, chunk c
// of [c_lo, c_hi) lies c_stride elements further per chunk; interval s = s_first + z covers chunks [s L, min((s + 1) L,
// n_chunks)) and goes to u_out[s - s_v0].  vec: both bins in one 16-byte load (nchan and c_stride even, rows 16-byte aligned).
// WEIGHTED: `weights` (NULL: all 1, nothing read) is the [n_base][nchan] float32 block of chunk c_lo, w_stride elements further
// per chunk.  `model` (NULL: visibility 1) is the [n_base][nchan] complex64 block of interval s_v0, model_stride (0: one model
// for all) elements further per interval.  S goes through u_out and Sw through d_out between launches; vec also asks for 8-byte
// aligned weights.  Plain: weights, model and d_out are not looked at.
template <bool WEIGHTED>
__device__ __forceinline__ void gains_average_body(const cf* __restrict__ rows, int64_t c_stride, const float* __restrict__ weights,
                                                   int64_t w_stride, const cf* __restrict__ model, int64_t model_stride, int64_t c_lo,
                                                   int64_t c_hi, int64_t interval, int64_t n_chunks, int64_t s_first, int64_t s_v0,
                                                   cd* __restrict__ u_out, double* __restrict__ d_out, int n_base, int nchan, int vec) {
    constexpr int kSums = WEIGHTED ? 3 : 2;      // per bin
    unsigned k0 = 2u * (blockIdx.x * kGainsThreads + threadIdx.x);
    if (k0 >= (unsigned)nchan) return;
    const bool two = k0 + 1 < (unsigned)nchan;
    const int64_t s = s_first + blockIdx.z;
    const int64_t b = s * interval, e = b + interval < n_chunks ? b + interval : n_chunks;
    const int64_t lo = b > c_lo ? b : c_lo, hi = e < c_hi ? e : c_hi;
    if (lo >= hi) return;
    const int p = blockIdx.y;
    const int64_t row = (int64_t)p * nchan;      // the same for the whole workgroup
    const int64_t out_row = (s - s_v0) * n_base * (int64_t)nchan + row;
    double acc[2 * kSums] = {};
    if (lo > b) {      // the launch before left the sums of chunks [b, lo) here
        const cd* __restrict__ in = u_out + out_row + k0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (j == 1 && !two) break;
            acc[kSums * j] = in[j].x;
            acc[kSums * j + 1] = in[j].y;
            if constexpr (WEIGHTED) acc[kSums * j + 2] = d_out[out_row + k0 + j];
        }
    }
    // every address from here on is formed from this k0: none of the ones above stays in registers through the walk
    asm volatile("" : "+v"(k0));
    const cf* __restrict__ src = rows + (lo - c_lo) * c_stride + row;
    const float* __restrict__ wsrc = WEIGHTED && weights ? weights + (lo - c_lo) * w_stride + row : nullptr;
    if (vec)      // the same for every thread of the launch
        gains_walk<WEIGHTED, true>(src, c_stride, wsrc, w_stride, k0, lo, hi, two, acc);
    else
        gains_walk<WEIGHTED, false>(src, c_stride, wsrc, w_stride, k0, lo, hi, two, acc);
    if (hi == e) {
        const double n = (double)(e - b);
#pragma unroll
        for (int i = 0; i < 2 * kSums; ++i) acc[i] /= n;
        if constexpr (WEIGHTED) {
            if (model) {      // U = A conj(M), D = Wbar |M|^2
                const cf* __restrict__ mq = model + (s - s_v0) * model_stride + row + k0;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if (j == 1 && !two) break;
                    const cf mv = mq[j];
                    const double mx = (double)mv.x, my = (double)mv.y;
                    const double ax = acc[3 * j], ay = acc[3 * j + 1];
                    acc[3 * j] = ax * mx + ay * my;
                    acc[3 * j + 1] = ay * mx - ax * my;
                    acc[3 * j + 2] *= mx * mx + my * my;
                }
            }
        }
    }
    cd* __restrict__ out = u_out + out_row + k0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (j == 1 && !two) break;
        cd w;
        w.x = acc[kSums * j];
        w.y = acc[kSums * j + 1];
        out[j] = w;
        if constexpr (WEIGHTED) d_out[out_row + k0 + j] = acc[kSums * j + 2];
    }
}

__global__ void __launch_bounds__(kGainsThreads)
gains_average_kernel(const cf* __restrict__ rows, int64_t c_stride, int64_t c_lo, int64_t c_hi, int64_t interval, int64_t n_chunks,
                     int64_t s_first, int64_t s_v0, cd* __restrict__ v_out, int n_base, int nchan, int vec) {
    gains_average_body<false>(rows, c_stride, nullptr, 0, nullptr, 0, c_lo, c_hi, interval, n_chunks, s_first, s_v0, v_out, nullptr, n_base,
                              nchan, vec);
}

__global__ void __launch_bounds__(kGainsThreads) __attribute__((amdgpu_waves_per_eu(4)))      // 4 waves a SIMD: 128 VGPRs at most
gains_weighted_average_kernel(const cf* __restrict__ rows, int64_t c_stride, const float* __restrict__ weights, int64_t w_stride,
                              const cf* __restrict__ model, int64_t model_stride, int64_t c_lo, int64_t c_hi, int64_t interval,
                              int64_t n_chunks, int64_t s_first, int64_t s_v0, cd* __restrict__ u_out, double* __restrict__ d_out,
                              int n_base, int nchan, int vec) {
    gains_average_body<true>(rows, c_stride, weights, w_stride, model, model_stride, c_lo, c_hi, interval, n_chunks, s_first, s_v0, u_out,
                             d_out, n_base, nchan, vec);
}

// Workgroup (x, y) solves the 2^tm_log bins k0 = x 2^tm_log .. of interval y of v.  LDS: vt[baseline][m] complex128, the upper
// triangle of the bins' Hermitian matrices, bin fastest -- the lanes of a wave are (a, m) with m fastest, so for one b they
// read whole 16-byte slots that are adjacent in m and, where b < a, adjacent in a as well (row (b, a + 1) follows row (b, a)) --
// then two images g[2][antenna][m] of the gains: an iteration reads one and writes the other, one barrier per iteration.
// WEIGHTED: v is U, and after the images comes dt[baseline][m] float64 from dpl: the same index as vt, 8 bytes a lane, so the 32
// lanes of a ds_read_b64 group read 256 contiguous bytes wherever vt's 16 lanes read 256.
// Thread (a, m) = threadIdx.x >> tm_log, & (2^tm_log - 1); threads beyond n_ant 2^tm_log only help with the loads.
template <bool WEIGHTED>
__device__ __forceinline__ void gains_solve_body(const cd* __restrict__ v, const double* __restrict__ dpl, cd* __restrict__ gains,
                                                 double* __restrict__ step, int n_ant, int nchan, int tm_log, int ref, int iters) {
    extern __shared__ __align__(16) unsigned char gains_lds[];
    const int tm = 1 << tm_log;
    const int n_base = n_ant * (n_ant - 1) / 2;
    cd* vt = reinterpret_cast<cd*>(gains_lds);
    cd* img = vt + ((int64_t)n_base << tm_log);
    [[maybe_unused]] double* dt = reinterpret_cast<double*>(img + ((int64_t)(2 * n_ant) << tm_log));
    const int k0 = blockIdx.x << tm_log;
    v += (int64_t)blockIdx.y * n_base * nchan;
    if constexpr (WEIGHTED) dpl += (int64_t)blockIdx.y * n_base * nchan;
    for (int id = threadIdx.x; id < (n_base << tm_log); id += blockDim.x) {
        const int p = id >> tm_log, k = k0 + (id & (tm - 1));
        cd w;
        w.x = 0.0;
        w.y = 0.0;
        [[maybe_unused]] double dd = 0.0;
        if (k < nchan) {
            w = v[(int64_t)p * nchan + k];
            if constexpr (WEIGHTED) dd = dpl[(int64_t)p * nchan + k];
        }
        vt[id] = w;
        if constexpr (WEIGHTED) dt[id] = dd;
    }
    __syncthreads();
    const int a = threadIdx.x >> tm_log, m = threadIdx.x & (tm - 1);
    const bool active = a < n_ant;
    const int tri_a = a * (2 * n_ant - a - 1) / 2 - a - 1;      // row (a, b) = tri_a + b for a < b
    // LDS index of element (a, b) of the matrix, a != b: the stored row (a, b), or row (b, a)
    auto index = [&](int b) {
        const int tri_b = b * (2 * n_ant - b - 1) / 2 - b - 1;
        return ((b < a ? tri_b + a : tri_a + b) << tm_log) + m;
    };
    // element (a, b) from its index: the stored row, or the conjugate of the transposed one
    auto element = [&](int id, int b) {
        cd w = vt[id];
        if (b < a) w.y = -w.y;
        return w;
    };
    int cur = 0;
    cd g;
    g.x = 0.0;
    g.y = 0.0;
    if (active) {
        // start: s = mean_b |V_b,ref|, g_ref = sqrt(s), g_a = V_a,ref / sqrt(s); WEIGHTED: with Vhat_b = U_b,ref / D_b,ref for
        // V, over the b where D != 0
        const int tri_r = ref * (2 * n_ant - ref - 1) / 2 - ref - 1;
        double s = 0.0;
        [[maybe_unused]] int count = 0;
        for (int b = 0; b < n_ant; ++b) {
            if (b == ref) continue;
            const int id = ((b < ref ? b * (2 * n_ant - b - 1) / 2 - b - 1 + ref : tri_r + b) << tm_log) + m;
            if constexpr (WEIGHTED) {
                const double dd = dt[id];
                if (dd != 0.0) {
                    const cd w = vt[id];
                    s += hypot(w.x / dd, w.y / dd);
                    ++count;
                }
            } else {
                const cd w = vt[id];
                s += hypot(w.x, w.y);
            }
        }
        if constexpr (WEIGHTED) {
            if (count > 0) s /= (double)count;
        } else {
            s /= (double)(n_ant - 1);
        }
        if (s != 0.0) {
            const double r = sqrt(s);
            if (a == ref) {
                g.x = r;
            } else if constexpr (WEIGHTED) {
                const int id = index(ref);
                const double dd = dt[id];
                if (dd != 0.0) {
                    const cd w = element(id, ref);
                    g.x = w.x / dd / r;
                    g.y = w.y / dd / r;
                }
            } else {
                const cd w = element(index(ref), ref);
                g.x = w.x / r;
                g.y = w.y / r;
            }
        }
        img[(a << tm_log) + m] = g;
    }
    __syncthreads();
    for (int it = 1; it <= iters; ++it) {
        if (active) {
            const cd* __restrict__ gc = img + ((cur * n_ant) << tm_log) + m;
            double nx = 0.0, ny = 0.0, d = 0.0;
            for (int b = 0; b < n_ant; ++b) {
                if (b == a) continue;
                const int id = index(b);
                const cd w = element(id, b);
                [[maybe_unused]] double dd;
                if constexpr (WEIGHTED) dd = dt[id];
                const cd gb = gc[b << tm_log];
                nx += w.x * gb.x - w.y * gb.y;
                ny += w.x * gb.y + w.y * gb.x;
                if constexpr (WEIGHTED)
                    d += dd * (gb.x * gb.x + gb.y * gb.y);
                else
                    d += gb.x * gb.x + gb.y * gb.y;
            }
            cd nw;
            nw.x = d != 0.0 ? nx / d : 0.0;
            nw.y = d != 0.0 ? ny / d : 0.0;
            if ((it & 1) == 0) {
                nw.x = (nw.x + g.x) / 2.0;
                nw.y = (nw.y + g.y) / 2.0;
            }
            g = nw;
            img[(((cur ^ 1) * n_ant + a) << tm_log) + m] = nw;
        }
        cur ^= 1;
        __syncthreads();
    }
    if (!active || k0 + m >= nchan) return;
    // img[cur] holds the last iteration's values, img[cur ^ 1] the ones before it
    const cd* __restrict__ gn = img + ((cur * n_ant) << tm_log) + m;
    const cd* __restrict__ go = img + (((cur ^ 1) * n_ant) << tm_log) + m;
    const int64_t sol = blockIdx.y;
    if (a == 0 && step) {
        double num = 0.0, den = 0.0;
        for (int b = 0; b < n_ant; ++b) {
            const cd x = gn[b << tm_log], y = go[b << tm_log];
            const double dx = x.x - y.x, dy = x.y - y.y;
            num += dx * dx + dy * dy;
            den += x.x * x.x + x.y * x.y;
        }
        step[sol * nchan + k0 + m] = den != 0.0 ? sqrt(num / den) : 0.0;
    }
    // the reference antenna's gain becomes real and non-negative
    const cd gr = gn[ref << tm_log];
    const double mag = hypot(gr.x, gr.y);
    cd o = g;
    if (mag != 0.0) {
        const double cx = gr.x / mag, cy = -gr.y / mag;
        o.x = g.x * cx - g.y * cy;
        o.y = g.x * cy + g.y * cx;
        if (a == ref) {
            o.x = mag;
            o.y = 0.0;
        }
    }
    gains[(sol * n_ant + a) * (int64_t)nchan + k0 + m] = o;
}

// a workgroup of kGainsThreads threads
__global__ void __launch_bounds__(kGainsThreads)
gains_solve_kernel(const cd* __restrict__ v, cd* __restrict__ gains, double* __restrict__ step, int n_ant, int nchan, int tm_log,
                   int ref, int iters) {
    gains_solve_body<false>(v, nullptr, gains, step, n_ant, nchan, tm_log, ref, iters);
}

// a workgroup of n_ant 2^tm_log threads rounded up to whole waves
__global__ void __launch_bounds__(kGainsThreads)
gains_weighted_solve_kernel(const cd* __restrict__ u, const double* __restrict__ dpl, cd* __restrict__ gains, double* __restrict__ step,
                            int n_ant, int nchan, int tm_log, int ref, int iters) {
    gains_solve_body<true>(u, dpl, gains, step, n_ant, nchan, tm_log, ref, iters);
}

}  // namespace
