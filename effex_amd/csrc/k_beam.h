// Part of libfxcorr's single translation unit: included by fxcorr.hip (not a stand-alone header).
#pragma once

namespace {

// ------------------------------------------------------------------------------------------
// tied-array beamformer (fxcorr.h fxc_beamform): y_b[c,i,k] = sum_a weff[c,b,a,k] f_a[c,i,k] over the spectra the
// plan's F stage wrote to the workspace as [chunk][antenna][frame][nchan], natural bin order.  The shape of xengine_kernel
// (k_finish.h): one 64-lane wave per column of 64 channels, 8-byte loads coalesced across channels, every spectrum read once
// with the nontemporal hint.  A thread keeps BT beams x kBeamFrames frames of complex sums in registers and walks the antennas
// in index order, two a trip: 2 x 8 samples from HBM and 2 x BT effective weights from L2 in flight, then 2 x BT x 8 complex
// multiply-adds (four fused multiply-adds each).  BT <= kBeamFrames, so a trip never loads more weights than samples; BT = 8
// reads the spectra once for up to 8 beams (128 accumulator registers), BT = 4 / 2 / 1 spend no arithmetic on beams that are not
// there.  More than 8 beams: one launch per tile of 8 (the spectra are read once per tile).  Every register array is indexed
// by unrolled loops only.
//
// One body (beam_body) serves the three kernels: beam_kernel, beam_mask_kernel and beam_inc_kernel are its entry points, each
// with the launch bounds its registers were decided under, and share one argument list.
// ------------------------------------------------------------------------------------------
constexpr int kBeamThreads = 64;
constexpr int kBeamFrames = 8;      // F_T
constexpr int kBeamTile = 8;        // the largest B_T
constexpr int kBeamMax = 16;        // beams of one call (fxc_beamform)

// weff[c][b][a][k] = w[b][a][k] * (complex64) rho[c][a][k]: the chunk's track table rounded once to float32, then a float32
// complex product with every operation rounded on its own.  Plans without a track skip this: weff = w, the same for every chunk.
__global__ __launch_bounds__(256) void beam_weights_kernel(const cf* __restrict__ w, const cd* __restrict__ rho, cf* __restrict__ weff,
                                                           int n_beam, int n_ant, int nchan, int64_t n_chunks) {
#pragma clang fp contract(off)
    const int64_t per_beam = (int64_t)n_ant * nchan;
    const int64_t total = n_chunks * n_beam * per_beam;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        const int64_t ak = idx % per_beam;
        const int64_t cb = idx / per_beam;
        const int64_t b = cb % n_beam, c = cb / n_beam;
        const cd r = rho[c * per_beam + ak];
        const float rx = (float)r.x, ry = (float)r.y;
        const cf v = w[b * per_beam + ak];
        weff[idx] = fxc::mk(v.x * rx - v.y * ry, v.x * ry + v.y * rx);
    }
}

// what a thread sums and stores: the beams' voltages y, the mean of |y|^2 over a time bin, or the incoherent sums
enum BeamKind { kBeamVoltage, kBeamPower, kBeamInc };

// The antenna mask (fxcorr.h fxc_beamform_ex) = [chunk][antenna][n_mbin][nchan] float32 in the rows' fftshifted
// channel order -- the layout of fxc_kurtosis's sk --, frame i under mask bin i / mtint; antenna a counts in a cell iff its value
// is > 0.  A sample that does not count is selected away on the loaded value, ahead of the multiply-adds: a NaN in it reaches no
// sum, and with every value > 0 the sums are the unmasked ones, bit for bit.  The mask is read at kout, contiguous across the wave
// but for the one wrap of the fftshift, through L2 (no nontemporal hint: a value serves up to mtint frames).
//
// The mask bins of a thread's frames: frame i is in bin j with r frames of the bin behind it.  tile() gives the row offsets of the
// 8 frames from the current one and moves on by 8; the frames past `end` repeat the last one's bin, as their samples do.
struct MaskWalk {
    int64_t j, r, mtint;
    __device__ __forceinline__ MaskWalk(int64_t i, int64_t mtint_) : j(i / mtint_), r(i % mtint_), mtint(mtint_) {}
    // -> true when the tile lies inside one mask bin (off[0] serves every frame)
    __device__ __forceinline__ bool tile(int64_t i, int64_t end, int nchan, int64_t (&off)[kBeamFrames]) {
        const int64_t j0 = j;
#pragma unroll
        for (int f = 0; f < kBeamFrames; ++f) {
            off[f] = j * nchan;
            if (i + f + 1 < end && ++r == mtint) {
                r = 0;
                ++j;
            }
        }
        return off[kBeamFrames - 1] == j0 * nchan;
    }
};

// A trip's loads: NA antennas from `s` (antenna stride s_ant) into z and their BT weights from `w` (antenna stride nchan, beam b
// at wb[b]) into g, in the order each kernel's registers and times were settled with.  The unmasked coherent
// trip: an antenna's 8 samples, then its weights, then the next antenna.  Otherwise every antenna's samples -- MASKED: and its
// mask values from `mk` (antenna stride m_ant), one an antenna (ONE: the tile lies in one mask bin) or one a frame, then
// z = m > 0 ? z : 0 -- and the weights last.  The coherent masked 8-beam tile (227 / 201 registers, two waves a SIMD) issues every
// sample and mask load before the first select: without the barrier the scheduler puts the first antenna's selects, and a wait,
// ahead of the trip's last three sample loads, and the tile runs 5 % longer.
template <int BT, int NA, bool MASKED, bool ONE, bool COHERENT>
__device__ __forceinline__ void beam_load(cf (&z)[NA][kBeamFrames], cf (&g)[NA][BT], const cf* __restrict__ s, int64_t s_ant,
                                          const int64_t (&off)[kBeamFrames], const cf* __restrict__ w, int nchan, const int64_t (&wb)[BT],
                                          const float* __restrict__ mk, int64_t m_ant, const int64_t (&moff)[kBeamFrames]) {
    constexpr bool W_EACH = COHERENT && !MASKED;
    constexpr int NM = ONE ? 1 : kBeamFrames;
    [[maybe_unused]] float m[NA][NM];
#pragma unroll
    for (int u = 0; u < NA; ++u) {
#pragma unroll
        for (int f = 0; f < kBeamFrames; ++f) z[u][f] = FXC_X_LOAD(s + u * s_ant + off[f]);
        if constexpr (MASKED) {
#pragma unroll
            for (int f = 0; f < NM; ++f) m[u][f] = mk[u * m_ant + moff[f]];
        }
        if constexpr (W_EACH) {
#pragma unroll
            for (int b = 0; b < BT; ++b) g[u][b] = w[wb[b] + (int64_t)u * nchan];
        }
    }
    if constexpr (MASKED) {
        if constexpr (COHERENT && BT == kBeamTile) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < NA; ++u)
#pragma unroll
            for (int f = 0; f < kBeamFrames; ++f) {
                const bool in = m[u][ONE ? 0 : f] > 0.f;
                z[u][f].x = in ? z[u][f].x : 0.f;
                z[u][f].y = in ? z[u][f].y : 0.f;
            }
    }
    if constexpr (!W_EACH) {
#pragma unroll
        for (int u = 0; u < NA; ++u)
#pragma unroll
            for (int b = 0; b < BT; ++b) g[u][b] = w[wb[b] + (int64_t)u * nchan];
    }
}

// NA antennas into the sums y, the antennas in index order.  ACC = cf: y += g z, four fused multiply-adds.  ACC = float, the
// incoherent sums: p = |z|^2 once per antenna and frame, g2 = |weff|^2 once per antenna and beam, then y = fma(g2, p, y) (p = 0
// where the antenna does not count).
template <int BT, int NA, bool MASKED, bool ONE, typename ACC>
__device__ __forceinline__ void beam_trip(ACC (&y)[BT][kBeamFrames], const cf* __restrict__ s, int64_t s_ant,
                                          const int64_t (&off)[kBeamFrames], const cf* __restrict__ w, int nchan, const int64_t (&wb)[BT],
                                          const float* __restrict__ mk, int64_t m_ant, const int64_t (&moff)[kBeamFrames]) {
    constexpr bool coherent = std::is_same_v<ACC, cf>;
    cf z[NA][kBeamFrames], g[NA][BT];
    beam_load<BT, NA, MASKED, ONE, coherent>(z, g, s, s_ant, off, w, nchan, wb, mk, m_ant, moff);
#pragma unroll
    for (int u = 0; u < NA; ++u) {
        if constexpr (coherent) {
#pragma unroll
            for (int b = 0; b < BT; ++b)
#pragma unroll
                for (int f = 0; f < kBeamFrames; ++f) {
                    y[b][f].x = __builtin_fmaf(-g[u][b].y, z[u][f].y, __builtin_fmaf(g[u][b].x, z[u][f].x, y[b][f].x));
                    y[b][f].y = __builtin_fmaf(g[u][b].y, z[u][f].x, __builtin_fmaf(g[u][b].x, z[u][f].y, y[b][f].y));
                }
        } else {
            float pw[kBeamFrames];
#pragma unroll
            for (int f = 0; f < kBeamFrames; ++f) pw[f] = __builtin_fmaf(z[u][f].y, z[u][f].y, z[u][f].x * z[u][f].x);
#pragma unroll
            for (int b = 0; b < BT; ++b) {
                const float g2 = __builtin_fmaf(g[u][b].y, g[u][b].y, g[u][b].x * g[u][b].x);
#pragma unroll
                for (int f = 0; f < kBeamFrames; ++f) y[b][f] = __builtin_fmaf(g2, pw[f], y[b][f]);
            }
        }
    }
}

// Workgroup (x = column of 64 channels, y = frame range, z = chunk of the pass) forms the beams b0 .. b0 + BT - 1 (those below
// n_beam are stored; a partial tile reads the last beam's weights again) over the frames [y fpr, min((y + 1) fpr, n_pts)) in
// tiles of kBeamFrames; the frames past the range's end of a last, partial tile are read as the range's last frame and dropped.
// weff = [chunk][n_beam][n_ant][nchan] with w_chunk elements between chunks (0: one set for every chunk); MASKED: mask = the
// pass's [chunk][n_ant][n_mbin][nchan], else the three mask arguments are not used.
// kBeamVoltage: out[c][b][i][k] = y, complex64, natural order.
// kBeamPower, kBeamInc: fpr is a multiple of tint, so a range holds whole time bins: the thread adds a frame's p -- |y|^2, or the
// incoherent sum_{a counted} |weff[c,b,a,k]|^2 |f_a[c,i,k]|^2 -- in frame order from 0 and stores sum / count at the bin's last
// frame (count = tint, less in a partial last bin of the chunk), to bin (k + nchan / 2) % nchan -- numpy's fftshift, odd counts
// included: out[c][b][j][k'] float32.  What a bin's sum is made of does not depend on fpr, the pass or the launch.
// A tile that straddles mask bins takes a mask value a frame: the coherent sums then go one antenna a trip, so that the 8-beam
// tile stays within 256 registers; the incoherent ones stay at two.
template <int BT, BeamKind KIND, bool MASKED>
__device__ __forceinline__ void beam_body(const cf* __restrict__ spec, const cf* __restrict__ weff, int64_t w_chunk,
                                          const float* __restrict__ mask, int64_t mtint, int64_t n_mbin, void* __restrict__ out, int n_ant,
                                          int64_t n_pts, int nchan, int n_beam, int b0, int64_t tint, int64_t fpr, int64_t n_tbin) {
    using acc_t = std::conditional_t<KIND == kBeamInc, float, cf>;
    const int pos = blockIdx.x * kBeamThreads + threadIdx.x;
    if (pos >= nchan) return;      // part of a wave
    const int64_t c = blockIdx.z;
    const int64_t i0 = (int64_t)blockIdx.y * fpr;
    const int64_t i1 = i0 + fpr < n_pts ? i0 + fpr : n_pts;
    const int64_t s_ant = n_pts * nchan;
    const int64_t m_ant = n_mbin * nchan;
    const cf* __restrict__ s = spec + c * n_ant * s_ant + pos;
    const cf* __restrict__ w = weff + c * w_chunk + pos;
    int64_t wb[BT];
#pragma unroll
    for (int b = 0; b < BT; ++b) wb[b] = (int64_t)(b0 + b < n_beam ? b0 + b : n_beam - 1) * n_ant * nchan;
    float pacc[BT];
#pragma unroll
    for (int b = 0; b < BT; ++b) pacc[b] = 0.f;
    int64_t cnt = 0;
    int kout = pos + nchan / 2;
    if (kout >= nchan) kout -= nchan;
    const float* __restrict__ mk = MASKED ? mask + c * n_ant * m_ant + kout : nullptr;      // (not MASKED: never read)
    [[maybe_unused]] MaskWalk walk(i0, MASKED ? mtint : 1);
    for (int64_t i = i0; i < i1; i += kBeamFrames) {
        int64_t off[kBeamFrames], moff[kBeamFrames];
#pragma unroll
        for (int f = 0; f < kBeamFrames; ++f) off[f] = (i + f < i1 ? i + f : i1 - 1) * nchan;
        bool one = true;
        if constexpr (MASKED) one = walk.tile(i, i1, nchan, moff);
        acc_t y[BT][kBeamFrames];
#pragma unroll
        for (int b = 0; b < BT; ++b)
#pragma unroll
            for (int f = 0; f < kBeamFrames; ++f) y[b][f] = acc_t{};
        const auto trip = [&](auto na, auto one_bin, int a) {
            beam_trip<BT, decltype(na)::value, MASKED, decltype(one_bin)::value>(y, s + a * s_ant, s_ant, off, w + (int64_t)a * nchan, nchan, wb,
                                                                                 mk + a * m_ant, m_ant, moff);
        };
        constexpr std::integral_constant<int, 1> k1{};
        constexpr std::integral_constant<int, 2> k2{};
        int a = 0;
        if (one) {
            for (; a + 2 <= n_ant; a += 2) trip(k2, std::true_type{}, a);
            if (a < n_ant) trip(k1, std::true_type{}, a);
        } else if constexpr (KIND == kBeamInc) {
            for (; a + 2 <= n_ant; a += 2) trip(k2, std::false_type{}, a);
            if (a < n_ant) trip(k1, std::false_type{}, a);
        } else {
            for (; a < n_ant; ++a) trip(k1, std::false_type{}, a);
        }
#pragma unroll
        for (int f = 0; f < kBeamFrames; ++f) {
            const int64_t frame = i + f;
            if (frame >= i1) break;
            if constexpr (KIND == kBeamVoltage) {
#pragma unroll
                for (int b = 0; b < BT; ++b)
                    if (b0 + b < n_beam) static_cast<cf*>(out)[((c * n_beam + b0 + b) * n_pts + frame) * nchan + pos] = y[b][f];
            } else {
#pragma unroll
                for (int b = 0; b < BT; ++b) {
                    if constexpr (KIND == kBeamInc) pacc[b] += y[b][f];
                    else pacc[b] += __builtin_fmaf(y[b][f].y, y[b][f].y, y[b][f].x * y[b][f].x);
                }
                ++cnt;
                if (cnt == tint || frame == n_pts - 1) {
                    const int64_t j = frame / tint;
                    const float n = (float)cnt;
#pragma unroll
                    for (int b = 0; b < BT; ++b) {
                        if (b0 + b < n_beam)
                            static_cast<float*>(out)[((c * n_beam + b0 + b) * n_tbin + j) * nchan + kout] = pacc[b] / n;
                        pacc[b] = 0.f;
                    }
                    cnt = 0;
                }
            }
        }
    }
}

// The entry points' one argument list (launch_beam picks among them by pointer); beam_kernel ignores mask, mtint and n_mbin
#define FXC_BEAM_PARAMS                                                                                                                  \
    const cf *__restrict__ spec, const cf *__restrict__ weff, int64_t w_chunk, const float *__restrict__ mask, int64_t mtint, int64_t n_mbin, \
        void *__restrict__ out, int n_ant, int64_t n_pts, int nchan, int n_beam, int b0, int64_t tint, int64_t fpr, int64_t n_tbin
#define FXC_BEAM_ARGS spec, weff, w_chunk, mask, mtint, n_mbin, out, n_ant, n_pts, nchan, n_beam, b0, tint, fpr, n_tbin

template <int BT, bool POWER>
__global__ __launch_bounds__(kBeamThreads) void beam_kernel(FXC_BEAM_PARAMS) {
    beam_body<BT, POWER ? kBeamPower : kBeamVoltage, false>(FXC_BEAM_ARGS);
}

template <int BT, bool POWER>
__global__ __launch_bounds__(kBeamThreads, 2) void beam_mask_kernel(FXC_BEAM_PARAMS) {
    beam_body<BT, POWER ? kBeamPower : kBeamVoltage, true>(FXC_BEAM_ARGS);
}

// (the pragma is kept from the kernel's own text and is inert here: it is lexical and the entry point holds no arithmetic.  What
// fixes the incoherent sums' roundings is that every multiply-add of beam_trip and beam_body is an explicit __builtin_fmaf and
// every other operation a lone multiply, add or divide: there is nothing to contract)
template <int BT, bool MASKED>
__global__ __launch_bounds__(kBeamThreads) void beam_inc_kernel(FXC_BEAM_PARAMS) {
#pragma clang fp contract(off)
    beam_body<BT, kBeamInc, MASKED>(FXC_BEAM_ARGS);
}

#undef FXC_BEAM_PARAMS
#undef FXC_BEAM_ARGS

}  // namespace
