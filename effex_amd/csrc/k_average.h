// Part of libfxcorr's single translation unit: included by fxcorr.hip (not a stand-alone header).
#pragma once

namespace {

// ------------------------------------------------------------------------------------------
// averager (fxcorr.h fxc_average_rows): the weighted mean of the cross rows over intervals of chunks and bins of
// channels, and the summed weights.  One kernel: the rows and weights are read once, with the walk of the weighted gain average
// (k_gains.h gains_walk: sixteen 16-byte loads in flight, flagged samples turned into zeros before any arithmetic), and only the
// reduced output is written -- there is no float64 plane in global memory between the sum over chunks and the sum over bins.
// ------------------------------------------------------------------------------------------
constexpr int kAverageThreads = kGainsThreads;
constexpr int kAverageTile = 2 * kAverageThreads;      // input bins of a workgroup at most: two a thread
constexpr int kAverageMaxBin = kAverageThreads;        // freq_bin at most: a tile holds a whole output bin and a thread sums it
// one LDS plane: the tile's bins plus, where freq_bin is even, a word of padding per output bin (at most tile / 2 of them)
constexpr int kAveragePlane = kAverageTile + kAverageTile / 2;

// Workgroup (x, y = baseline, z = interval) owns the `tile` input bins from x tile of its (interval, baseline); thread t the bins
// k0 = x tile + 2 t and k0 + 1 where they lie inside the tile and the band.  `rows` is the row set of the launch's first chunk
// and first baseline, chunk c lies c_stride elements further and baseline y y nchan; `weights` (NULL: every weight 1, nothing
// read) likewise with w_stride.  Interval z covers the chunks [z interval, min((z + 1) interval, n_chunks)) of the launch and goes
// to out_rows / out_w (NULL: not wanted) + z out_stride + y n_out.  vec: both bins in one 16-byte load and one 8-byte weight load
// (nchan, the tile and c_stride even, rows 16-byte and weights 8-byte aligned); the same for every thread of the launch.
// freq_bin == 1: the thread divides and stores its own two bins.  freq_bin > 1: tile is a multiple of freq_bin, so an output bin
// lies in one tile; (Sx, Sy, W) go into three LDS planes of doubles, word p(j) = j + (freq_bin even ? j / freq_bin : 0) of a plane
// is the tile's bin j: a thread's two bins are adjacent words (an even freq_bin never parts them), the writes of a wave 128
// consecutive words but for the padding, and thread m, which adds the freq_bin words of output bin m in ascending order, is an
// odd number of 8-byte words from thread m + 1 -- freq_bin or freq_bin + 1 --, so the lanes that share an LDS cycle (32 of a
// ds_read_b64, 16 of a ds_read2_b64) fall on different bank pairs.  One barrier.  A partial last bin adds the bins inside the
// band only; nothing reads a word that was not written.
__global__ void __launch_bounds__(kAverageThreads) __attribute__((amdgpu_waves_per_eu(4)))      // 4 waves a SIMD: 128 VGPRs at most
rows_average_kernel(const cf* __restrict__ rows, int64_t c_stride, const float* __restrict__ weights, int64_t w_stride, int64_t interval,
                    int64_t n_chunks, cf* __restrict__ out_rows, float* __restrict__ out_w, int64_t out_stride, int nchan, int freq_bin,
                    int tile, int n_out, int vec) {
    __shared__ double plane[3][kAveragePlane];
    const unsigned j0 = 2u * threadIdx.x;                     // the thread's first bin within the tile
    unsigned k0 = blockIdx.x * (unsigned)tile + j0;
    const bool one = j0 < (unsigned)tile && k0 < (unsigned)nchan;
    const bool two = j0 + 1 < (unsigned)tile && k0 + 1 < (unsigned)nchan;
    const int64_t lo = blockIdx.z * interval, hi = lo + interval < n_chunks ? lo + interval : n_chunks;
    const int64_t row = (int64_t)blockIdx.y * nchan;          // the same for the whole workgroup
    const int64_t out_at = blockIdx.z * out_stride + (int64_t)blockIdx.y * n_out;
    double acc[6] = {};
    if (one) {
        asm volatile("" : "+v"(k0));      // every address of the walk is a workgroup's base plus this k0
        const cf* __restrict__ src = rows + lo * c_stride + row;
        const float* __restrict__ wsrc = weights ? weights + lo * w_stride + row : nullptr;
        if (vec)
            gains_walk<true, true>(src, c_stride, wsrc, w_stride, k0, lo, hi, two, acc);
        else
            gains_walk<true, false>(src, c_stride, wsrc, w_stride, k0, lo, hi, two, acc);
    }
    if (freq_bin == 1) {      // the same for the whole launch
        if (!one) return;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (j == 1 && !two) break;
            const double w = acc[3 * j + 2];
            cf v;
            v.x = w > 0.0 ? (float)(acc[3 * j] / w) : 0.f;
            v.y = w > 0.0 ? (float)(acc[3 * j + 1] / w) : 0.f;
            out_rows[out_at + k0 + j] = v;
            if (out_w) out_w[out_at + k0 + j] = (float)w;
        }
        return;
    }
    const bool padded = (freq_bin & 1) == 0;
    if (one) {
        const unsigned at = j0 + (padded ? j0 / (unsigned)freq_bin : 0u);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (j == 1 && !two) break;
#pragma unroll
            for (int q = 0; q < 3; ++q) plane[q][at + j] = acc[3 * j + q];
        }
    }
    __syncthreads();
    const int per_tile = tile / freq_bin;
    const int m = blockIdx.x * per_tile + (int)threadIdx.x;
    if ((int)threadIdx.x >= per_tile || m >= n_out) return;
    const int left = nchan - m * freq_bin;                    // the last bin may be partial
    const int count = left < freq_bin ? left : freq_bin;
    const int at = (int)threadIdx.x * (freq_bin + (padded ? 1 : 0));
    double tx = 0.0, ty = 0.0, wm = 0.0;
    for (int i = 0; i < count; ++i) {
        tx += plane[0][at + i];
        ty += plane[1][at + i];
        wm += plane[2][at + i];
    }
    cf v;
    v.x = wm > 0.0 ? (float)(tx / wm) : 0.f;
    v.y = wm > 0.0 ? (float)(ty / wm) : 0.f;
    out_rows[out_at + m] = v;
    if (out_w) out_w[out_at + m] = (float)wm;
}

}  // namespace
