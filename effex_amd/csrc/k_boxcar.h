// Part of libfxcorr's single translation unit: included by fxcorr.hip (not a stand-alone header).
#pragma once

namespace {

// ------------------------------------------------------------------------------------------
// single-pulse search on dedispersed series (fxcorr.h fxc_boxcar_search): per row a clipped mean and standard
// deviation in float64 with a fixed order of additions, the boxcars of widths 2^j as a tree of float32 adds, and the best S/N of
// every block of starts with its width and time.  The statistics take two sweeps a round -- the mean, then the squares about it --
// each followed by a small step that adds the tree's upper levels; the host is not needed between them.
// ------------------------------------------------------------------------------------------
constexpr int kBoxThreads = 256;
constexpr int kBoxT = 4096;                       // starts of a filter tile
constexpr int kBoxPer = kBoxT / kBoxThreads;      // starts a thread tracks in registers
constexpr int kBoxMaxJ = 12;                      // widths 2^0 .. 2^12
constexpr int kBoxSeg = 256;                      // samples of a segment sum, segment sums of a group sum (the definition's)
constexpr int kBoxSegs = 64;                      // segments of a sweep workgroup: one a lane of its first wave
constexpr int kBoxHalf = 128;                     // samples of a segment that lie in LDS at a time
constexpr int kBoxPad = kBoxHalf + 1;             // words of a segment's LDS line: odd, the lanes of the summing wave hit 64 banks

// A row's state on the device.  (m_cnt, limit, has_limit) say which samples count in the current round: all of them, or those with
// (x - m_cnt)^2 <= limit; m and n are the round's mean and count, v its variance.  den[j] = std sqrt(2^j) once the rounds are over.
struct BoxRow {
    double m_cnt, limit, m, v, stdv;
    double den[kBoxMaxJ + 1];
    long long n;
    int has_limit, degenerate;
};

// One sweep over the rows: workgroup x of row y owns the segments [64 x, 64 x + 64).  Half a segment at a time, 64 x 128 samples
// are loaded coalesced -- lanes on consecutive samples -- into LDS lines of 129 words, and lane s of the first wave adds line s in
// ascending t from +0: what the definition asks of a segment.  second = 0: the sum of the counted samples and their count;
// second = 1: the sum of the squares of (x - m) over the counted samples.  A sample that does not count is never added.
__global__ void __launch_bounds__(kBoxThreads)
boxcar_sweep_kernel(const float* __restrict__ x, int64_t n_t, BoxRow* __restrict__ rows, double* __restrict__ seg_sum,
                    int* __restrict__ seg_cnt, int64_t n_seg, int second) {
#pragma clang fp contract(off)
    __shared__ float line[kBoxSegs * kBoxPad];
    const BoxRow* __restrict__ r = rows + blockIdx.y;
    if (r->degenerate) return;
    const float* __restrict__ p = x + (int64_t)blockIdx.y * n_t;
    const int64_t seg0 = (int64_t)blockIdx.x * kBoxSegs;
    const double m_cnt = r->m_cnt, limit = r->limit, m = r->m;
    const bool all = !r->has_limit;
    double acc = 0.0;
    int cnt = 0;
    for (int half = 0; half < kBoxSeg / kBoxHalf; ++half) {
        constexpr int kLoads = 8;
        for (int q0 = (int)threadIdx.x; q0 < kBoxSegs * kBoxHalf; q0 += kBoxThreads * kLoads) {
            float v[kLoads];
#pragma unroll
            for (int u = 0; u < kLoads; ++u) {
                const int q = q0 + kBoxThreads * u;
                const int64_t t = (seg0 + (q / kBoxHalf)) * kBoxSeg + half * kBoxHalf + (q % kBoxHalf);
                v[u] = t < n_t ? p[t] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < kLoads; ++u) {
                const int q = q0 + kBoxThreads * u;
                line[(q / kBoxHalf) * kBoxPad + (q % kBoxHalf)] = v[u];
            }
        }
        __syncthreads();
        if (threadIdx.x < kBoxSegs) {
            const int64_t t0 = (seg0 + threadIdx.x) * kBoxSeg + half * kBoxHalf;
            const int n_here = (int)std::min<int64_t>(kBoxHalf, std::max<int64_t>(0, n_t - t0));
            const float* __restrict__ l = line + threadIdx.x * kBoxPad;
            for (int i = 0; i < n_here; ++i) {
                const double xv = (double)l[i];
                const double e = xv - m_cnt;
                const bool counted = all || e * e <= limit;
                if (second) {
                    const double d = xv - m;
                    const double term = d * d;
                    if (counted) acc = acc + term;
                } else if (counted) {
                    acc = acc + xv;
                    ++cnt;
                }
            }
        }
        __syncthreads();
    }
    if (threadIdx.x < kBoxSegs && seg0 + threadIdx.x < n_seg) {
        seg_sum[(int64_t)blockIdx.y * n_seg + seg0 + threadIdx.x] = acc;
        if (!second) seg_cnt[(int64_t)blockIdx.y * n_seg + seg0 + threadIdx.x] = cnt;
    }
}

// The tree's upper levels and the round's numbers, one workgroup a row: thread g adds the 256 segment sums of group g in
// ascending order, thread 0 the group sums in ascending order.  second = 0 (after the first sweep): m = sum / n, and a round that
// counts fewer than 2 samples ends the row as degenerate.  second = 1: v = sum / (n - 1); with last = 0 the next round's limit
// c2 v against this round's m; with last = 1 std = sqrt(v) and den[j] = std root[j], and v == 0 makes the row degenerate.
__global__ void __launch_bounds__(kBoxThreads)
boxcar_round_kernel(BoxRow* __restrict__ rows, const double* __restrict__ seg_sum, const int* __restrict__ seg_cnt, int64_t n_seg,
                    int second, int last, double c2, const double* __restrict__ root) {
#pragma clang fp contract(off)
    __shared__ double grp[kBoxThreads];
    __shared__ long long grp_n[kBoxThreads];
    BoxRow* __restrict__ r = rows + blockIdx.x;
    const bool dead = r->degenerate != 0;      // the same for the whole workgroup
    if (!dead) {
        const double* __restrict__ s = seg_sum + (int64_t)blockIdx.x * n_seg;
        const int* __restrict__ c = seg_cnt + (int64_t)blockIdx.x * n_seg;
        const int64_t n_grp = (n_seg + kBoxSeg - 1) / kBoxSeg;
        double total = 0.0;
        long long n = 0;
        for (int64_t g0 = 0; g0 < n_grp; g0 += kBoxThreads) {
            const int64_t g = g0 + threadIdx.x;
            double a = 0.0;
            long long k = 0;
            if (g < n_grp) {
                const int64_t i1 = std::min<int64_t>(n_seg, (g + 1) * kBoxSeg);
                for (int64_t i = g * kBoxSeg; i < i1; ++i) {
                    a = a + s[i];
                    if (!second) k += c[i];
                }
            }
            grp[threadIdx.x] = a;
            grp_n[threadIdx.x] = k;
            __syncthreads();
            if (threadIdx.x == 0) {
                const int here = (int)std::min<int64_t>(kBoxThreads, n_grp - g0);
                for (int i = 0; i < here; ++i) {
                    total = total + grp[i];
                    n += grp_n[i];
                }
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            if (!second) {
                r->n = n;
                r->m = total / (double)n;
                if (n < 2) r->degenerate = 1;
            } else {
                const double v = total / (double)(r->n - 1);
                r->v = v;
                if (!last) {
                    r->limit = c2 * v;
                    r->m_cnt = r->m;
                    r->has_limit = 1;
                } else if (v == 0.0) {
                    r->degenerate = 1;
                } else {
                    r->stdv = __dsqrt_rn(v);
                }
            }
        }
    }
    if (last && second && threadIdx.x == 0) {
        if (r->degenerate) r->stdv = 0.0;
        for (int j = 0; j <= kBoxMaxJ; ++j) r->den[j] = r->stdv * root[j];
    }
}

__global__ void boxcar_rows_init_kernel(BoxRow* __restrict__ rows, int64_t n_rows) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    BoxRow r;
    r.m_cnt = r.limit = r.m = r.v = r.stdv = 0.0;
    for (int j = 0; j <= kBoxMaxJ; ++j) r.den[j] = 0.0;
    r.n = 0;
    r.has_limit = r.degenerate = 0;
    rows[i] = r;
}

// How a row's starts are cut into tiles and cells (the blocks of the output): decided by the driver (box_geometry), read here.
// block <= kBoxT: a tile owns cells whole cells, tile i the starts from i cells block and the cells from i cells; it writes the
// outputs.  block > kBoxT: a cell is cut into tiles tiles of kBoxT starts, tile i = cell tiles + k begins at cell block + k kBoxT;
// it writes one partial best, and boxcar_fold_kernel takes a cell's partials in tile order.
struct BoxGeom {
    int64_t n_t, n_starts, n_blk, block;
    int j_lo, j_hi;
    unsigned cells, tiles;      // cells a tile (block <= kBoxT) / tiles a cell (block > kBoxT, else 0)
};

// the k-th start of a tile lies at word k + k / 32 of the arrays the cells are read from: a thread per cell walks its block's
// starts, and the pad spreads lanes that are `block` words apart over the banks
__device__ __forceinline__ int box_slot(int k) { return k + (k >> 5); }
constexpr int kBoxBestWords = kBoxT + kBoxT / 32;

// Workgroup x of row y owns one tile of at most kBoxT starts from x0.  It loads the tile's samples and the halo of 2^j_hi - 1 behind
// them once, lanes on consecutive samples (4-byte loads: a row may sit anywhere), subtracts the row's mean and rounds to float32
// into LDS; samples from n_t on are stored as zeros and only enter sums that are no candidates.  Level j is made from level j - 1
// between two buffers: L_j[e] = L_{j-1}[e] + L_{j-1}[e + 2^(j-1)], thread i on the words i, i + 256, ..: consecutive lanes read and
// write consecutive words at every level, and one barrier a level separates the readers of a buffer from its next writers.
// Thread i keeps the best of the starts i + 256 u, u < 16, in registers indexed by unrolled loops only: widths come in ascending
// order and only a strictly greater S/N replaces, so ties stay with the narrowest width.  The bests then go to LDS, and a thread per
// cell walks its block's starts in ascending order: greater S/N, or equal S/N and narrower width, replaces -- the candidate order's
// first of the largest.
__global__ void __launch_bounds__(kBoxThreads)
boxcar_filter_kernel(const float* __restrict__ x, const BoxRow* __restrict__ rows, BoxGeom g, float* __restrict__ snr_out,
                     int* __restrict__ width_out, int* __restrict__ time_out, int64_t out_stride) {
    extern __shared__ float box_lds[];
    const BoxRow* __restrict__ r = rows + blockIdx.y;
    const int64_t tile = blockIdx.x;
    int64_t x0, cell0, n_here64;
    if (g.tiles == 0) {
        x0 = tile * (int64_t)g.cells * g.block;
        cell0 = tile * (int64_t)g.cells;
        n_here64 = std::min<int64_t>((int64_t)g.cells * g.block, g.n_starts - x0);
    } else {
        const int64_t cell = tile / g.tiles, k = tile % g.tiles;
        x0 = cell * g.block + k * kBoxT;
        cell0 = tile;      // the partial's slot
        n_here64 = std::min<int64_t>(kBoxT, std::min<int64_t>((cell + 1) * g.block, g.n_starts) - x0);
    }
    if (n_here64 <= 0) return;      // the tail of the last cell's tiles: the fold does not read it
    const int n_here = (int)n_here64;
    const int64_t block_here = g.tiles == 0 ? g.block : (int64_t)kBoxT;
    const int n_cells = (int)((n_here + block_here - 1) / block_here);
    float* __restrict__ o_s = snr_out + (int64_t)blockIdx.y * out_stride + cell0;
    int* __restrict__ o_w = width_out + (int64_t)blockIdx.y * out_stride + cell0;
    int* __restrict__ o_t = time_out + (int64_t)blockIdx.y * out_stride + cell0;
    if (r->degenerate) {
        for (int c = (int)threadIdx.x; c < n_cells; c += kBoxThreads) {
            o_s[c] = 0.f;
            o_w[c] = g.j_lo;
            o_t[c] = (int)(x0 + c * block_here);
        }
        return;
    }
    const int tid = (int)threadIdx.x;
    const int w = kBoxT + (1 << g.j_hi) - 1;      // words of a level buffer
    float* __restrict__ buf0 = box_lds;
    float* __restrict__ buf1 = box_lds + w;
    const double m = r->m;
    const float* __restrict__ p = x + (int64_t)blockIdx.y * g.n_t + x0;
    const int64_t left = g.n_t - x0;              // samples of the row from x0 on
    {
        constexpr int kLoads = 8;
        for (int e0 = tid; e0 < w; e0 += kBoxThreads * kLoads) {
            float v[kLoads];
#pragma unroll
            for (int u = 0; u < kLoads; ++u) {
                const int e = e0 + kBoxThreads * u;
                v[u] = e < w && e < left ? p[e] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < kLoads; ++u) {
                const int e = e0 + kBoxThreads * u;
                if (e < w) buf0[e] = e < left ? (float)((double)v[u] - m) : 0.f;
            }
        }
    }
    __syncthreads();
    float best[kBoxPer];
    int best_j[kBoxPer];
#pragma unroll
    for (int u = 0; u < kBoxPer; ++u) {
        best[u] = 0.f;
        best_j[u] = g.j_lo;
    }
    if (g.j_lo == 0) {
        const double den = r->den[0];
#pragma unroll
        for (int u = 0; u < kBoxPer; ++u) best[u] = (float)((double)buf0[tid + kBoxThreads * u] / den);
    }
    for (int j = 1; j <= g.j_hi; ++j) {
        const float* __restrict__ src = (j & 1) ? buf0 : buf1;
        float* __restrict__ dst = (j & 1) ? buf1 : buf0;
        const int h = 1 << (j - 1);
        const int cnt = w - (1 << j) + 1;         // words of level j: kBoxT or more
        const double den = r->den[j];
        const int64_t fits = left - (1 << j);     // start e is a candidate of width j iff e <= fits (and e < n_here)
#pragma unroll
        for (int u = 0; u < kBoxPer; ++u) {
            const int e = tid + kBoxThreads * u;
            const float val = src[e] + src[e + h];
            dst[e] = val;
            if (j >= g.j_lo && e <= fits) {
                const float s = (float)((double)val / den);
                if (j == g.j_lo || s > best[u]) {
                    best[u] = s;
                    best_j[u] = j;
                }
            }
        }
        for (int e = kBoxT + tid; e < cnt; e += kBoxThreads) dst[e] = src[e] + src[e + h];
        __syncthreads();
    }
    // the levels are done with both buffers (the last barrier; with j_hi = 0 the one below): the bests take their place
    if (g.j_hi == 0) __syncthreads();
    float* sb = box_lds;
    int* jb = reinterpret_cast<int*>(box_lds) + kBoxBestWords;
#pragma unroll
    for (int u = 0; u < kBoxPer; ++u) {
        const int e = tid + kBoxThreads * u;
        sb[box_slot(e)] = best[u];
        jb[box_slot(e)] = best_j[u];
    }
    __syncthreads();
    for (int c = tid; c < n_cells; c += kBoxThreads) {
        const int k0 = (int)(c * block_here), k1 = (int)std::min<int64_t>(n_here, k0 + block_here);
        float bs = sb[box_slot(k0)];
        int bj = jb[box_slot(k0)], bk = k0;
        for (int k = k0 + 1; k < k1; ++k) {
            const float s = sb[box_slot(k)];
            const int jj = jb[box_slot(k)];
            if (s > bs || (s == bs && jj < bj)) {
                bs = s;
                bj = jj;
                bk = k;
            }
        }
        o_s[c] = bs;
        o_w[c] = bj;
        o_t[c] = (int)(x0 + bk);
    }
}

// block > kBoxT: thread per (row, cell) takes the cell's partial bests in tile order; greater S/N, or equal S/N and narrower
// width, replaces -- among equals of one width the earlier tile holds the earlier start
__global__ void __launch_bounds__(kBoxThreads)
boxcar_fold_kernel(const float* __restrict__ p_snr, const int* __restrict__ p_w, const int* __restrict__ p_t, BoxGeom g, int64_t n_rows,
                   float* __restrict__ snr_out, int* __restrict__ width_out, int* __restrict__ time_out) {
    const int64_t i = (int64_t)blockIdx.x * kBoxThreads + threadIdx.x;
    if (i >= n_rows * g.n_blk) return;
    const int64_t row = i / g.n_blk, cell = i % g.n_blk;
    const int64_t size = std::min<int64_t>(g.block, g.n_starts - cell * g.block);
    const int64_t n = (size + kBoxT - 1) / kBoxT;
    const int64_t at = (row * g.n_blk + cell) * (int64_t)g.tiles;
    float bs = p_snr[at];
    int bj = p_w[at], bt = p_t[at];
    for (int64_t k = 1; k < n; ++k) {
        const float s = p_snr[at + k];
        const int jj = p_w[at + k];
        if (s > bs || (s == bs && jj < bj)) {
            bs = s;
            bj = jj;
            bt = p_t[at + k];
        }
    }
    snr_out[i] = bs;
    width_out[i] = bj;
    time_out[i] = bt;
}

}  // namespace
