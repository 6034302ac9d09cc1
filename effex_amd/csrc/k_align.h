// Part of libfxcorr's single translation unit: included by fxcorr.hip (not a stand-alone header).
#pragma once

namespace {

// ------------------------------------------------------------------------------------------
// whole-sample delays (fxc_set_sample_delays, fxc_set_delay_track_aligned): the plan's kernels read, for chunk c, antenna a,
// sample n, the delivered sample x[c][a][n + s] when 0 <= n + s < num_samp and exactly 0 otherwise.  Chunks stay independent:
// nothing comes from a neighbouring chunk or stream ("samples that do not exist are read as zeros").
//     out[c][a][n] = x[c][a][n + s_a],   s = shifts[c * shift_stride + a]   (shift_stride 0: static shifts, n_ant: a track's)
// A copy of bits (unsigned words: NaN payloads travel unchanged), every byte touched once, so both sides carry the
// nontemporal hint of the other single-touch passes (k_prepass.h).
// Workgroup (slice, stream).  A lane owns pairs of samples that are 16-byte aligned in the DESTINATION -- a stream of an odd
// num_samp starts on an odd 8-byte boundary, its first "pair" is then the one sample before the first 16-byte boundary -- and stores 16
// bytes; only a pair that hangs over either end of the stream is stored sample by sample.  The source pair is read by one
// 16-byte buffer load too: it is 16-byte aligned only when shift, stream start and the caller's pointer agree and 8-byte
// aligned otherwise (an odd shift), which a buffer load takes (dword alignment is all it asks; the cost of the straddle is
// what tools/bench_align.py reports for odd shifts).
// A workgroup walks its slice in steps of kAlignUnroll x 256 pairs.  A step that lies whole inside the destination stream and
// whose source lies whole inside the source stream (workgroup-uniform) issues its loads back to back and tests nothing per lane.
// Every other step -- the ends of a stream, the zero fill -- goes sample by sample: the offset of a sample outside
// [0, num_samp) is replaced by kAlignOob, past any descriptor (num_samp <= 2^27, a stream is at most 2^30 bytes), which the
// buffer load answers with zeros without touching memory.  Both descriptors span exactly one stream, so no address outside
// [stream, stream + num_samp) is ever formed into a load or a store: the neighbouring stream is never read.
// The offsets ride in the VGPR (tests/test_isa_hazards.py: no wide buffer store with a scalar offset).
// ------------------------------------------------------------------------------------------
constexpr unsigned kAlignOob = 0xC0000000u;
constexpr int kAlignAux = 2;           // nontemporal, loads and stores
constexpr int kAlignUnroll = 4;        // pairs in flight per lane in a whole step

// the pair of source samples m0, m0 + 1, zeros where there are none
__device__ __forceinline__ v4u32 align_load_edge(__amdgpu_buffer_rsrc_t rx, int64_t m0, int64_t num_samp) {
    const bool ok0 = m0 >= 0 && m0 < num_samp, ok1 = m0 + 1 >= 0 && m0 + 1 < num_samp;
    const unsigned off = (unsigned)(m0 * 8);      // (used only where the sample exists: < 2^30)
    const v2u32 lo = __builtin_amdgcn_raw_buffer_load_b64(rx, ok0 ? off : kAlignOob, 0, kAlignAux);
    const v2u32 hi = __builtin_amdgcn_raw_buffer_load_b64(rx, ok1 ? off + 8u : kAlignOob, 0, kAlignAux);
    return v4u32{ok0 ? lo[0] : 0u, ok0 ? lo[1] : 0u, ok1 ? hi[0] : 0u, ok1 ? hi[1] : 0u};
}

// the pair of destination samples n0, n0 + 1, those that exist
__device__ __forceinline__ void align_store_edge(__amdgpu_buffer_rsrc_t ro, v4u32 d, int64_t n0, int64_t num_samp) {
    const unsigned off = (unsigned)(n0 * 8);
    if (n0 >= 0 && n0 + 1 < num_samp) {
        __builtin_amdgcn_raw_buffer_store_b128(d, ro, off, 0, kAlignAux);
    } else {
        if (n0 >= 0 && n0 < num_samp) __builtin_amdgcn_raw_buffer_store_b64(v2u32{d[0], d[1]}, ro, off, 0, kAlignAux);
        if (n0 + 1 >= 0 && n0 + 1 < num_samp) __builtin_amdgcn_raw_buffer_store_b64(v2u32{d[2], d[3]}, ro, off + 8u, 0, kAlignAux);
    }
}

// grid (n_slices, streams <= 65535)
__global__ __launch_bounds__(256) void align_c64_kernel(const cf* __restrict__ x, cf* __restrict__ out, const int* __restrict__ shifts,
                                                       int shift_stride, int n_ant, int64_t num_samp, int n_slices) {
    const unsigned st = blockIdx.y, chunk = st / (unsigned)n_ant;
    const int64_t s = shifts[(int64_t)chunk * shift_stride + (st - chunk * (unsigned)n_ant)];
    const cf* xs = x + st * num_samp;
    cf* os = out + st * num_samp;
    const int bytes = (int)(num_samp * (int64_t)sizeof(cf));
    __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<cf*>(xs), 0, bytes, 0x00020000);
    __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(os, 0, bytes, 0x00020000);
    // pair j holds the samples 2 j - par and 2 j - par + 1: 16-byte aligned in the destination
    const int64_t par = (int64_t)((reinterpret_cast<uintptr_t>(os) >> 3) & 1);
    const int64_t n_pairs = (num_samp + par + 1) / 2;
    const int64_t per = (n_pairs + n_slices - 1) / n_slices;
    const int64_t lo = (int64_t)blockIdx.x * per, hi = (lo + per < n_pairs) ? lo + per : n_pairs;
    constexpr int kStep = kAlignUnroll * 256;
    for (int64_t jb = lo; jb < hi; jb += kStep) {      // (uniform: the workgroup's next kStep pairs)
        const int64_t n_lo = 2 * jb - par, n_hi = 2 * (jb + kStep) - par;
        if (jb + kStep <= hi && n_lo >= 0 && n_hi <= num_samp && n_lo + s >= 0 && n_hi + s <= num_samp) {
            const unsigned off = (unsigned)((n_lo + 2 * (int64_t)threadIdx.x) * 8), soff = (unsigned)((n_lo + s + 2 * (int64_t)threadIdx.x) * 8);
            v4u32 d[kAlignUnroll];
#pragma unroll
            for (int q = 0; q < kAlignUnroll; ++q) d[q] = __builtin_amdgcn_raw_buffer_load_b128(rx, soff + (unsigned)q * 4096u, 0, kAlignAux);
#pragma unroll
            for (int q = 0; q < kAlignUnroll; ++q) __builtin_amdgcn_raw_buffer_store_b128(d[q], ro, off + (unsigned)q * 4096u, 0, kAlignAux);
        } else {
            for (int64_t j = jb + threadIdx.x; j < hi && j < jb + kStep; j += 256)
                align_store_edge(ro, align_load_edge(rx, 2 * j - par + s, num_samp), 2 * j - par, num_samp);
        }
    }
}

// the shifts of a pass's chunks under an aligned track: s_a(t) = llrint(tau_a(t) bandwidth), tau_a(t) rounded as in track_phasor
// (k_track.h); ties to even, as np.rint.  Written once per pass, read by align_c64_kernel and by the aligned table kernels: the
// table of chunk t and the alignment of chunk t use the same integer.  Clamped to the int32 range (such a stream is all zeros
// whatever the number).
__device__ __forceinline__ int track_shift(const TrackPar& tp, double bandwidth, int a, int64_t t) {
#pragma clang fp contract(off)
    const double tau = tp.tau0[a] + (double)t * tp.rate[a];
    double v = tau * bandwidth;
    v = v > 2147483647.0 ? 2147483647.0 : (v < -2147483647.0 ? -2147483647.0 : v);
    return (int)llrint(v);
}

__global__ void track_shifts_kernel(TrackPar tp, double bandwidth, int* __restrict__ out, int n_ant, int64_t t0, int64_t n_t) {
    const int64_t total = n_t * n_ant;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride)
        out[idx] = track_shift(tp, bandwidth, (int)(idx % n_ant), t0 + idx / n_ant);
}

}  // namespace
