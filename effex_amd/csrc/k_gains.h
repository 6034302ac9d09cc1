// Part of libfxcorr's single translation unit: included by fxcorr.hip (not a stand-alone header).
#pragma once

namespace {

// ------------------------------------------------------------------------------------------
// gain solve (fxcorr.h fxc_solve_gains): per solution interval and per bin, the complex gains g_a whose
// products g_a conj(g_b) fit the averaged cross rows V_ab in the least-squares sense.
//   average  rows [chunk][row][bin] complex64 -> V [interval][baseline][bin] complex128: the interval's chunks added in
//            float64 in ascending chunk order, then divided by their number.  A launch may hold only part of an interval's
//            chunks (host rows come in batches): it then continues the sum that the launch before left in V, so the adds
//            and their order -- and with them every bit -- are those of one pass over all chunks.
//   solve    a tile of adjacent bins of one interval in LDS, a thread per (antenna, bin), the iteration in float64.
// ------------------------------------------------------------------------------------------
constexpr int kGainsThreads = 256;
constexpr int kGainsUnroll = 16;             // loads of 16 bytes a thread keeps in flight
constexpr int kGainsLdsBytes = 144 * 1024;   // the solve's tile: 64 antennas x 4 bins are 134 KiB
constexpr int kGainsMaxTile = 64;            // bins of a tile at most

// adds the bins (k0, k0 + 1) of `left` consecutive chunks (FULL: of kGainsUnroll) to the sums, in chunk order; the loads of all
// of them are issued before the first add
template <bool FULL>
__device__ __forceinline__ void gains_add_chunks(const cf* __restrict__ src, int64_t c_stride, int left, int vec, bool two, double& a0,
                                                 double& a1, double& a2, double& a3) {
    typedef float v4f __attribute__((ext_vector_type(4)));
    v4f v[kGainsUnroll];
#pragma unroll
    for (int i = 0; i < kGainsUnroll; ++i) {
        v[i] = v4f{0.f, 0.f, 0.f, 0.f};
        if (FULL || i < left) {
            const cf* q = src + i * c_stride;
            if (vec) {
                v[i] = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(q));
            } else {
                const cf u0 = fxc::nt_load(q);
                v[i][0] = u0.x;
                v[i][1] = u0.y;
                if (two) {
                    const cf u1 = fxc::nt_load(q + 1);
                    v[i][2] = u1.x;
                    v[i][3] = u1.y;
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < kGainsUnroll; ++i) {
        if (FULL || i < left) {
            a0 += (double)v[i][0];
            a1 += (double)v[i][1];
            a2 += (double)v[i][2];
            a3 += (double)v[i][3];
        }
    }
}

// Thread (x, y = baseline, z = interval - s_first) owns bins 2 x and 2 x + 1.  `rows` is the row set of chunk c_lo, chunk c
// of [c_lo, c_hi) lies c_stride elements further per chunk; interval s = s_first + z covers chunks [s L, min((s + 1) L,
// n_chunks)) and goes to V[s - s_v0].  vec: both bins in one 16-byte load (nchan and c_stride even, rows 16-byte aligned).
__global__ void __launch_bounds__(kGainsThreads)
gains_average_kernel(const cf* __restrict__ rows, int64_t c_stride, int64_t c_lo, int64_t c_hi, int64_t interval, int64_t n_chunks,
                     int64_t s_first, int64_t s_v0, cd* __restrict__ v_out, int n_base, int nchan, int vec) {
    const int k0 = 2 * (int)(blockIdx.x * kGainsThreads + threadIdx.x);
    if (k0 >= nchan) return;
    const bool two = k0 + 1 < nchan;
    const int64_t s = s_first + blockIdx.z;
    const int64_t b = s * interval, e = b + interval < n_chunks ? b + interval : n_chunks;
    const int64_t lo = b > c_lo ? b : c_lo, hi = e < c_hi ? e : c_hi;
    if (lo >= hi) return;
    const int p = blockIdx.y;
    cd* __restrict__ out = v_out + ((s - s_v0) * n_base + p) * (int64_t)nchan + k0;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if (lo > b) {      // the launch before left the sum of chunks [b, lo) here
        a0 = out[0].x;
        a1 = out[0].y;
        if (two) {
            a2 = out[1].x;
            a3 = out[1].y;
        }
    }
    const cf* __restrict__ src = rows + (lo - c_lo) * c_stride + (int64_t)p * nchan + k0;
    int64_t c = lo;
    for (; c + kGainsUnroll <= hi; c += kGainsUnroll, src += kGainsUnroll * c_stride)
        gains_add_chunks<true>(src, c_stride, kGainsUnroll, vec, two, a0, a1, a2, a3);
    if (c < hi) gains_add_chunks<false>(src, c_stride, (int)(hi - c), vec, two, a0, a1, a2, a3);
    if (hi == e) {
        const double n = (double)(e - b);
        a0 /= n;
        a1 /= n;
        a2 /= n;
        a3 /= n;
    }
    cd w;
    w.x = a0;
    w.y = a1;
    out[0] = w;
    if (two) {
        w.x = a2;
        w.y = a3;
        out[1] = w;
    }
}

// Workgroup (x, y) solves the 2^tm_log bins k0 = x 2^tm_log .. of interval y of v.  LDS: vt[baseline][m] complex128, the upper
// triangle of the bins' Hermitian matrices, bin fastest -- the lanes of a wave are (a, m) with m fastest, so for one b they
// read whole 16-byte slots that are adjacent in m and, where b < a, adjacent in a as well (row (b, a + 1) follows row (b, a)) --
// then two images g[2][antenna][m] of the gains: an iteration reads one and writes the other, one barrier per iteration.
// Thread (a, m) = threadIdx.x >> tm_log, & (2^tm_log - 1); threads beyond n_ant 2^tm_log only help with the loads.
__global__ void __launch_bounds__(kGainsThreads)
gains_solve_kernel(const cd* __restrict__ v, cd* __restrict__ gains, double* __restrict__ step, int n_ant, int nchan, int tm_log,
                   int ref, int iters) {
    extern __shared__ __align__(16) unsigned char gains_lds[];
    const int tm = 1 << tm_log;
    const int n_base = n_ant * (n_ant - 1) / 2;
    cd* vt = reinterpret_cast<cd*>(gains_lds);
    cd* img = vt + ((int64_t)n_base << tm_log);
    const int k0 = blockIdx.x << tm_log;
    v += (int64_t)blockIdx.y * n_base * nchan;
    for (int id = threadIdx.x; id < (n_base << tm_log); id += kGainsThreads) {
        const int p = id >> tm_log, k = k0 + (id & (tm - 1));
        cd w;
        w.x = 0.0;
        w.y = 0.0;
        if (k < nchan) w = v[(int64_t)p * nchan + k];
        vt[id] = w;
    }
    __syncthreads();
    const int a = threadIdx.x >> tm_log, m = threadIdx.x & (tm - 1);
    const bool active = a < n_ant;
    const int tri_a = a * (2 * n_ant - a - 1) / 2 - a - 1;      // row (a, b) = tri_a + b for a < b
    // element (a, b) of the matrix, a != b: the stored row, or the conjugate of the transposed one
    auto element = [&](int b) {
        const int tri_b = b * (2 * n_ant - b - 1) / 2 - b - 1;
        cd w = vt[((b < a ? tri_b + a : tri_a + b) << tm_log) + m];
        if (b < a) w.y = -w.y;
        return w;
    };
    int cur = 0;
    cd g;
    g.x = 0.0;
    g.y = 0.0;
    if (active) {
        // start: s = mean_b |V_b,ref|, g_ref = sqrt(s), g_a = V_a,ref / sqrt(s)
        const int tri_r = ref * (2 * n_ant - ref - 1) / 2 - ref - 1;
        double s = 0.0;
        for (int b = 0; b < n_ant; ++b) {
            if (b == ref) continue;
            const cd w = vt[((b < ref ? b * (2 * n_ant - b - 1) / 2 - b - 1 + ref : tri_r + b) << tm_log) + m];
            s += hypot(w.x, w.y);
        }
        s /= (double)(n_ant - 1);
        if (s != 0.0) {
            const double r = sqrt(s);
            if (a == ref) {
                g.x = r;
            } else {
                const cd w = element(ref);
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
                const cd w = element(b);
                const cd gb = gc[b << tm_log];
                nx += w.x * gb.x - w.y * gb.y;
                ny += w.x * gb.y + w.y * gb.x;
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

// ------------------------------------------------------------------------------------------
// weighted gain solve (fxcorr.h fxc_solve_gains_weighted): the same two steps with a weight per sample and a model
// visibility per baseline and bin.
//   average  rows and weights [chunk][baseline][bin] -> U [interval][baseline][bin] complex128 and D [..] float64: S = sum of
//            w v and Sw = sum of w over the samples with w > 0, in float64 in ascending chunk order, continued from launch to
//            launch like V above; the launch with the interval's last chunk divides by the number of chunks and applies the model:
//            U = (S / n) conj(M), D = (Sw / n) |M|^2.
//   solve    as above with U for V and the denominator sum over D_ab |g_b|^2; D is an LDS plane of its own.
// ------------------------------------------------------------------------------------------
constexpr int kGainsWeightedTileBytes = 24;      // LDS per baseline and bin: U complex128 + D float64
constexpr int kGainsImageBytes = 32;             // LDS per antenna and bin: two complex128 gain images

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

// gains_add_chunks with a weight per value: adds the bins (k0, k0 + 1) of N consecutive chunks to acc = (S re, S im, Sw) of bin
// k0, then of bin k0 + 1, in chunk order; the loads of all N are issued before the first add.  A sample whose weight is not > 0
// adds zeros, whatever its value holds.  wsrc NULL (the same for every thread of the launch): no weight is read, every weight is
// 1.  VEC: one 16-byte row load and one 8-byte weight load per chunk, else 8-byte and 4-byte loads per bin.  The addresses are a
// base that is the same for the whole workgroup plus the thread's 32-bit k0.
template <int N, bool VEC>
__device__ __forceinline__ void gains_weighted_add_chunks(const cf* __restrict__ src, int64_t c_stride, const float* __restrict__ wsrc,
                                                          int64_t w_stride, unsigned k0, bool two, double (&acc)[6]) {
    typedef float v4f __attribute__((ext_vector_type(4)));
    typedef float v2f __attribute__((ext_vector_type(2)));
    if (VEC) two = true;      // an even channel count: every thread has both bins
    v4f v[N];
    v2f w[N];
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
}

// the chunks [lo, hi) of one thread in ascending order: blocks of kGainsUnroll (of half as many on the narrow-load path, whose
// chunk takes four loads: the same 32 loads in flight), then halving blocks down to 1 for the rest
template <int N, bool VEC>
__device__ __forceinline__ void gains_weighted_rest(const cf* __restrict__& src, int64_t c_stride, const float* __restrict__& wsrc,
                                                    int64_t w_stride, unsigned k0, int left, bool two, double (&acc)[6]) {
    if (left & N) {
        gains_weighted_add_chunks<N, VEC>(src, c_stride, wsrc, w_stride, k0, two, acc);
        src += N * c_stride;
        if (wsrc) wsrc += N * w_stride;
    }
    if constexpr (N > 1) gains_weighted_rest<N / 2, VEC>(src, c_stride, wsrc, w_stride, k0, left, two, acc);
}

template <bool VEC>
__device__ __forceinline__ void gains_weighted_walk(const cf* __restrict__ src, int64_t c_stride, const float* __restrict__ wsrc,
                                                    int64_t w_stride, unsigned k0, int64_t lo, int64_t hi, bool two, double (&acc)[6]) {
    constexpr int kBlock = VEC ? kGainsUnroll : kGainsUnroll / 2;
    int64_t c = lo;
    for (; c + kBlock <= hi; c += kBlock, src += kBlock * c_stride) {
        gains_weighted_add_chunks<kBlock, VEC>(src, c_stride, wsrc, w_stride, k0, two, acc);
        if (wsrc) wsrc += kBlock * w_stride;
    }
    gains_weighted_rest<kBlock / 2, VEC>(src, c_stride, wsrc, w_stride, k0, (int)(hi - c), two, acc);
}

// gains_average_kernel's thread layout, chunk ranges and continuation rule.  `weights` (NULL: all 1, nothing read) is the
// [n_base][nchan] float32 block of chunk c_lo, w_stride elements further per chunk.  `model` (NULL: visibility 1) is the
// [n_base][nchan] complex64 block of interval s_v0, model_stride (0: one model for all) elements further per interval.  S goes
// through u_out and Sw through d_out between launches; vec also asks for 8-byte aligned weights.
__global__ void __launch_bounds__(kGainsThreads) __attribute__((amdgpu_waves_per_eu(4)))      // 4 waves a SIMD: 128 VGPRs at most
gains_weighted_average_kernel(const cf* __restrict__ rows, int64_t c_stride, const float* __restrict__ weights, int64_t w_stride,
                              const cf* __restrict__ model, int64_t model_stride, int64_t c_lo, int64_t c_hi, int64_t interval,
                              int64_t n_chunks, int64_t s_first, int64_t s_v0, cd* __restrict__ u_out, double* __restrict__ d_out,
                              int n_base, int nchan, int vec) {
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
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (lo > b) {      // the launch before left the sums of chunks [b, lo) here
        const cd* __restrict__ in = u_out + out_row + k0;
        const double* __restrict__ in_d = d_out + out_row + k0;
        acc[0] = in[0].x;
        acc[1] = in[0].y;
        acc[2] = in_d[0];
        if (two) {
            acc[3] = in[1].x;
            acc[4] = in[1].y;
            acc[5] = in_d[1];
        }
    }
    // every address from here on is formed from this k0: none of the ones above stays in registers through the walk
    asm volatile("" : "+v"(k0));
    const cf* __restrict__ src = rows + (lo - c_lo) * c_stride + row;
    const float* __restrict__ wsrc = weights ? weights + (lo - c_lo) * w_stride + row : nullptr;
    if (vec)      // the same for every thread of the launch
        gains_weighted_walk<true>(src, c_stride, wsrc, w_stride, k0, lo, hi, two, acc);
    else
        gains_weighted_walk<false>(src, c_stride, wsrc, w_stride, k0, lo, hi, two, acc);
    if (hi == e) {
        const double n = (double)(e - b);
#pragma unroll
        for (int i = 0; i < 6; ++i) acc[i] /= n;
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
    cd* __restrict__ out = u_out + out_row + k0;
    double* __restrict__ out_d = d_out + out_row + k0;
    cd w;
    w.x = acc[0];
    w.y = acc[1];
    out[0] = w;
    out_d[0] = acc[2];
    if (two) {
        w.x = acc[3];
        w.y = acc[4];
        out[1] = w;
        out_d[1] = acc[5];
    }
}

// gains_solve_kernel with U for V and a denominator plane.  LDS: ut[baseline][m] complex128 (the layout and bank reasoning of vt
// above), the two gain images, then dt[baseline][m] float64: the same index as ut, 8 bytes a lane, so the 32 lanes of a
// ds_read_b64 group read 256 contiguous bytes wherever ut's 16 lanes read 256.  The workgroup has n_ant 2^tm_log
// threads rounded up to whole waves.
__global__ void __launch_bounds__(kGainsThreads)
gains_weighted_solve_kernel(const cd* __restrict__ u, const double* __restrict__ dpl, cd* __restrict__ gains, double* __restrict__ step,
                            int n_ant, int nchan, int tm_log, int ref, int iters) {
    extern __shared__ __align__(16) unsigned char gains_lds[];
    const int tm = 1 << tm_log;
    const int n_base = n_ant * (n_ant - 1) / 2;
    cd* ut = reinterpret_cast<cd*>(gains_lds);
    cd* img = ut + ((int64_t)n_base << tm_log);
    double* dt = reinterpret_cast<double*>(img + ((int64_t)(2 * n_ant) << tm_log));
    const int k0 = blockIdx.x << tm_log;
    u += (int64_t)blockIdx.y * n_base * nchan;
    dpl += (int64_t)blockIdx.y * n_base * nchan;
    for (int id = threadIdx.x; id < (n_base << tm_log); id += blockDim.x) {
        const int p = id >> tm_log, k = k0 + (id & (tm - 1));
        cd w;
        w.x = 0.0;
        w.y = 0.0;
        double dd = 0.0;
        if (k < nchan) {
            w = u[(int64_t)p * nchan + k];
            dd = dpl[(int64_t)p * nchan + k];
        }
        ut[id] = w;
        dt[id] = dd;
    }
    __syncthreads();
    const int a = threadIdx.x >> tm_log, m = threadIdx.x & (tm - 1);
    const bool active = a < n_ant;
    const int tri_a = a * (2 * n_ant - a - 1) / 2 - a - 1;      // row (a, b) = tri_a + b for a < b
    // LDS index of element (a, b), a != b: the stored row (a, b), or row (b, a), whose U is the conjugate
    auto index = [&](int b) {
        const int tri_b = b * (2 * n_ant - b - 1) / 2 - b - 1;
        return ((b < a ? tri_b + a : tri_a + b) << tm_log) + m;
    };
    int cur = 0;
    cd g;
    g.x = 0.0;
    g.y = 0.0;
    if (active) {
        // start: Vhat_b = U_b,ref / D_b,ref where D != 0; s = their mean modulus, g_ref = sqrt(s), g_a = Vhat_a / sqrt(s)
        const int tri_r = ref * (2 * n_ant - ref - 1) / 2 - ref - 1;
        double s = 0.0;
        int count = 0;
        for (int b = 0; b < n_ant; ++b) {
            if (b == ref) continue;
            const int id = ((b < ref ? b * (2 * n_ant - b - 1) / 2 - b - 1 + ref : tri_r + b) << tm_log) + m;
            const double dd = dt[id];
            if (dd != 0.0) {
                const cd w = ut[id];
                s += hypot(w.x / dd, w.y / dd);
                ++count;
            }
        }
        if (count > 0) s /= (double)count;
        if (s != 0.0) {
            const double r = sqrt(s);
            if (a == ref) {
                g.x = r;
            } else {
                const int id = index(ref);
                const double dd = dt[id];
                if (dd != 0.0) {
                    const cd w = ut[id];
                    g.x = w.x / dd / r;
                    g.y = (ref < a ? -w.y : w.y) / dd / r;
                }
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
                cd w = ut[id];
                if (b < a) w.y = -w.y;
                const double dd = dt[id];
                const cd gb = gc[b << tm_log];
                nx += w.x * gb.x - w.y * gb.y;
                ny += w.x * gb.y + w.y * gb.x;
                d += dd * (gb.x * gb.x + gb.y * gb.y);
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

}  // namespace
