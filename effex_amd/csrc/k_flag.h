// Part of libfxcorr's single translation unit: included by fxcorr.hip (not a stand-alone header).
#pragma once

namespace {

// ------------------------------------------------------------------------------------------
// detector (fxcorr.h fxc_flag_rows): a weight per (chunk, baseline, bin) from the rows alone.
//   time   per window and (baseline, bin) column: lower medians of x, y and of the squared distance e from them over the column's
//          live samples, `iters` times, flagging e > threshold x median; then the column's level and scatter.
//   freq   per baseline: sliding lower medians of level and scatter over the bins around each bin; an outlier bin loses its column.
// Every median is an element of its set, found by bisection on the values' bit patterns: nothing is rounded, so the method cannot
// change a bit.
// ------------------------------------------------------------------------------------------
constexpr int kFlagThreads = 256;           // four waves, each with columns of its own: no barrier anywhere
constexpr int kFlagMaxChunks = 1024;        // chunks of a window at most
constexpr int kFlagMaxQLog = 4;             // columns of a wave at most: 16 (128 contiguous bytes of a row)
constexpr int kFlagTargetLaneSamples = 8;   // samples of a lane the host aims for when it picks a wave's columns
// (a lane then holds 32 samples at most -- 2 columns of 1024 chunks --, its liveness mask is one 64-bit register, and a workgroup's
// LDS is 4 waves x 3 planes x 2048 words = 96 KiB at most)
constexpr uint32_t kFlagUndefined = 0xffffffffu;      // level / scatter of a column without a live sample: no float >= 0 has these bits

// float32 <-> a key that orders as the values do (-0 below +0: the two give the same e and the same level)
__device__ __forceinline__ uint32_t flag_key(float v) {
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float flag_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// the sum of v over the lanes of this lane's column (the lanes with the same lane mod 2^q_log), in every one of them
__device__ __forceinline__ int flag_column_sum(int v, int q_log) {
    for (int off = 32; off >> q_log; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// The keys of rank `rank` (0-based, ascending) among the column's live values of NP planes at once: 32 steps from the top bit
// down, each counting the live keys below the candidate (the count of plane j in bits 16 j .. 16 j + 15: a column holds 1024).
// Lane `lane` holds the elements i 64 + lane, i < m, bit i of `live` says which count.  Every lane of a column gets the result.
template <int NP>
__device__ __forceinline__ void flag_select(const uint32_t* __restrict__ plane, int plane_stride, int lane, int m, uint64_t live, int rank,
                                            int q_log, uint32_t (&res)[NP]) {
#pragma unroll
    for (int j = 0; j < NP; ++j) res[j] = 0;
    for (int bit = 31; bit >= 0; --bit) {
        uint32_t cand[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) cand[j] = res[j] | (1u << bit);
        int cnt = 0;
        uint64_t bits = live;
        const uint32_t* __restrict__ q = plane + lane;
#pragma unroll 4
        for (int i = 0; i < m; ++i, q += 64, bits >>= 1) {      // four steps' reads in flight
            const int on = (int)(bits & 1);
#pragma unroll
            for (int j = 0; j < NP; ++j) cnt += (on & (int)(q[j * plane_stride] < cand[j])) << (16 * j);
        }
        cnt = flag_column_sum(cnt, q_log);
#pragma unroll
        for (int j = 0; j < NP; ++j)
            if (((cnt >> (16 * j)) & 0xffff) <= rank) res[j] = cand[j];
    }
}

// e of the lane's live samples about (mx, my) into the third plane: ONE float32 subtraction each, exact products in float64,
// one rounding
__device__ __forceinline__ void flag_deviations(uint32_t* __restrict__ plane, int plane_stride, int lane, int m, uint64_t live, float mx,
                                                float my) {
    uint32_t* __restrict__ q = plane + lane;
    uint64_t bits = live;
    for (int i = 0; i < m; ++i, q += 64, bits >>= 1) {
        if (bits & 1) {
            const float dx = flag_unkey(q[0]) - mx, dy = flag_unkey(q[plane_stride]) - my;
            q[2 * plane_stride] = __float_as_uint((float)((double)dx * (double)dx + (double)dy * (double)dy));
        }
    }
}

// Workgroup (x, y = baseline, z = window) owns the 4 Q bins from x 4 Q of its (window, baseline), Q = 2^q_log; wave w the Q bins
// from (4 x + w) Q, all chunks: n Q samples, sample f = chunk Q + column in lane f mod 64 (64 is a multiple of Q, so a lane
// stays in one column).  LDS: per wave three planes (the keys of x and y, the bits of e) of plane_stride words, word f of a plane
// is sample f: lane l reads and writes words i 64 + l only, 64 consecutive words an instruction -- conflict-free -- and no lane
// reads what another wrote, so there is no barrier; what lanes share goes through flag_column_sum.  Liveness is a bit per
// sample in the lane's registers.  `rows` is the row set of the launch's first chunk, chunk c lies c_stride elements further
// and baseline y y nchan; `prior` (NULL: none) and `weights` lie w_stride per chunk.  Window z covers the chunks [z window,
// min((z + 1) window, n_chunks)).  stats: level then scatter, [gridDim.z][gridDim.y][nchan] each; counts[(z count_nb + y) 3].
__global__ void __launch_bounds__(kFlagThreads)
flag_time_kernel(const cf* __restrict__ rows, int64_t c_stride, const float* __restrict__ prior, float* __restrict__ weights,
                 int64_t w_stride, int64_t window, int64_t n_chunks, float threshold, int iters, uint32_t* __restrict__ stats,
                 unsigned long long* __restrict__ counts, int count_nb, int nchan, int q_log, int plane_stride) {
    extern __shared__ __align__(16) unsigned char flag_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = ((((int)blockIdx.x << 2) + wave) << q_log) + (lane & ((1 << q_log) - 1));
    const bool in_band = k < nchan;
    const int64_t c0 = blockIdx.z * window;
    const int n = (int)(c0 + window < n_chunks ? window : n_chunks - c0);
    const int total = n << q_log, m = (total + 63) >> 6;
    uint32_t* __restrict__ plane = reinterpret_cast<uint32_t*>(flag_lds) + wave * 3 * plane_stride;
    const int64_t col = (int64_t)blockIdx.y * nchan + k;
    const cf* __restrict__ src = rows + c0 * c_stride + col;
    const float* __restrict__ pri = prior ? prior + c0 * w_stride + col : nullptr;
    float* __restrict__ dst = weights + c0 * w_stride + col;
    const int c_lane = lane >> q_log, c_step = 64 >> q_log;      // the lane's chunks: c_lane + i c_step

    // rows, read once
    uint64_t live = 0;
    int n_dead = 0;
#pragma unroll 4
    for (int i = 0; i < m; ++i) {
        const int c = c_lane + i * c_step;
        if (in_band && c < n) {
            const cf v = fxc::nt_load(src + c * c_stride);
            const uint32_t bx = __float_as_uint(v.x), by = __float_as_uint(v.y);
            bool ok = (bx & 0x7f800000u) != 0x7f800000u && (by & 0x7f800000u) != 0x7f800000u && !(v.x == 0.f && v.y == 0.f);
            if (pri) ok = ok && pri[c * w_stride] > 0.f;
            plane[i * 64 + lane] = flag_key(v.x);
            plane[plane_stride + i * 64 + lane] = flag_key(v.y);
            live |= (uint64_t)ok << i;
            n_dead += !ok;
        }
    }

    int n_time = 0;
    for (int it = 0; it <= iters; ++it) {      // the last round is the column's statistics
        const int n_live = flag_column_sum(__popcll(live), q_log);
        const int rank = n_live > 0 ? (n_live - 1) >> 1 : 0;
        uint32_t mk[2], dk[1];
        flag_select<2>(plane, plane_stride, lane, m, live, rank, q_log, mk);
        const float mx = flag_unkey(mk[0]), my = flag_unkey(mk[1]);
        flag_deviations(plane, plane_stride, lane, m, live, mx, my);
        flag_select<1>(plane + 2 * plane_stride, plane_stride, lane, m, live, rank, q_log, dk);
        const float d = __uint_as_float(dk[0]);
        if (it == iters) {
            if (in_band && c_lane == 0) {
                const int64_t at = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * nchan + k;
                const int64_t plane_elems = (int64_t)gridDim.z * gridDim.y * nchan;
                const float level = (float)((double)mx * (double)mx + (double)my * (double)my);
                stats[at] = n_live > 0 ? __float_as_uint(level) : kFlagUndefined;
                stats[plane_elems + at] = n_live > 0 ? dk[0] : kFlagUndefined;
            }
            break;
        }
        if (n_live > 0 && d > 0.f) {
            const float limit = threshold * d;
            const uint32_t* __restrict__ q = plane + 2 * plane_stride + lane;
            uint64_t keep = live;
            for (int i = 0; i < m; ++i, q += 64)
                if (((live >> i) & 1) && __uint_as_float(q[0]) > limit) keep &= ~((uint64_t)1 << i);
            n_time += __popcll(live ^ keep);
            live = keep;
        }
    }

    // weights, written once
    for (int i = 0; i < m; ++i) {
        const int c = c_lane + i * c_step;
        if (in_band && c < n) {
            float w = 0.f;
            if ((live >> i) & 1) w = pri ? pri[c * w_stride] : 1.f;
            dst[c * w_stride] = w;
        }
    }
    // counts: a wave's sums, one atomic each
    int lo = n_dead, hi = n_time;
    for (int off = 32; off; off >>= 1) {
        lo += __shfl_xor(lo, off);
        hi += __shfl_xor(hi, off);
    }
    if (lane == 0) {
        unsigned long long* __restrict__ out = counts + ((int64_t)blockIdx.z * count_nb + blockIdx.y) * 3;
        if (lo) atomicAdd(out, (unsigned long long)lo);
        if (hi) atomicAdd(out + 1, (unsigned long long)hi);
    }
}

// the bits of rank `rank` among S[lo .. hi] (DEV: among |S[j] - centre|, a float32 subtraction) over the defined bins
template <bool DEV>
__device__ __forceinline__ uint32_t flag_freq_select(const uint32_t* __restrict__ s, int lo, int hi, int rank, float centre) {
    uint32_t res = 0;
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t cand = res | (1u << bit);
        int cnt = 0;
        for (int j = lo; j <= hi; ++j) {
            const uint32_t v = s[j];
            const uint32_t key = DEV ? __float_as_uint(fabsf(__uint_as_float(v) - centre)) : v;
            cnt += (int)(v != kFlagUndefined && key < cand);
        }
        if (cnt <= rank) res = cand;
    }
    return res;
}

// Thread (x, y = baseline, z = window) owns bin k: the window's lower medians of level and scatter around k, the two tests, and
// an outlier's column of weights cleared -- adjacent outliers write adjacent words.  Reads the planes only, writes the weights
// only: every decision is taken from what the time stage left.
__global__ void __launch_bounds__(kFlagThreads)
flag_freq_kernel(const uint32_t* __restrict__ stats, float* __restrict__ weights, int64_t w_stride, int64_t window, int64_t n_chunks,
                 float threshold, int half_width, unsigned long long* __restrict__ counts, int count_nb, int nchan) {
    const int k = (int)(blockIdx.x * kFlagThreads + threadIdx.x);
    if (k >= nchan) return;
    const int64_t row = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * nchan;
    const int64_t plane_elems = (int64_t)gridDim.z * gridDim.y * nchan;
    if (stats[row + k] == kFlagUndefined) return;
    const int lo = k - half_width > 0 ? k - half_width : 0, hi = k + half_width < nchan - 1 ? k + half_width : nchan - 1;
    const uint32_t* __restrict__ level = stats + row;
    int m = 0;
    for (int j = lo; j <= hi; ++j) m += (int)(level[j] != kFlagUndefined);
    const int rank = (m - 1) >> 1;
    bool outlier = false;
#pragma unroll
    for (int which = 0; which < 2; ++which) {
        const uint32_t* __restrict__ s = level + which * plane_elems;
        const float r = __uint_as_float(flag_freq_select<false>(s, lo, hi, rank, 0.f));
        const float sd = __uint_as_float(flag_freq_select<true>(s, lo, hi, rank, r));
        float diff = __uint_as_float(s[k]) - r;
        if (which == 0) diff = fabsf(diff);      // the level test is two-sided
        outlier = outlier || (sd > 0.f && diff > threshold * sd);
    }
    if (!outlier) return;
    const int64_t c0 = blockIdx.z * window;
    const int n = (int)(c0 + window < n_chunks ? window : n_chunks - c0);
    float* __restrict__ dst = weights + c0 * w_stride + (int64_t)blockIdx.y * nchan + k;
    int cleared = 0;
    for (int c = 0; c < n; ++c) {
        cleared += (int)(dst[c * w_stride] > 0.f);
        dst[c * w_stride] = 0.f;
    }
    if (cleared) atomicAdd(counts + ((int64_t)blockIdx.z * count_nb + blockIdx.y) * 3 + 2, (unsigned long long)cleared);
}

}  // namespace
