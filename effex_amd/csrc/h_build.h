// Part of libfxcorr's single translation unit: included by fxcorr.hip (not a stand-alone header).
#pragma once

// plan construction, in three steps: the route (plan_route: every route flag, from the shape and the developer knobs, no device
// call), the kernels built for the channel count that the route takes from the start (plan_spec), and the device tables and kernel
// attributes of that route (plan_build), each table built once by one of the builders below

namespace {

// the tiled design's workgroup kernels (512 .. 8192 channels) serve this plan: its path, or fxc_channelize (tiled_f)
bool tiled_kernels(const fxc_plan* p) { return !small_nchan(p->nchan) && (p->path == FXC_PATH_TILED || p->tiled_f); }

// the chirp-z convolution length for n channels: any 7-smooth number from 2 n - 1 up to the next power of two -- the one whose
// stages cost least (points x a weight per stage from the measured stage times), not the power of two itself (2049 channels:
// 4116 = 4 3 7 7 7 points instead of 8192).  FXC_BLU_SMOOTH=0: the power of two (developer knob)
int blu_length(int n) {
    int m_pow2 = 1;
    while (m_pow2 < 2 * n - 1) m_pow2 <<= 1;
    int m = m_pow2;
    if (FXC_DEV_ENV_INT("FXC_BLU_SMOOTH", 1)) {
        double best = 1e300;
        for (int cand = 2 * n - 1; cand <= std::min(m_pow2, kBluMaxNfft); ++cand) {
            int rest = cand;
            double w = 0.0;
            for (int q : {4, 2, 3, 5, 7}) {
                const double wq = q == 4 ? 1.0 : q == 2 ? 0.8 : q == 3 ? 1.0 : q == 5 ? 1.5 : 2.0;
                while (rest % q == 0) {
                    rest /= q;
                    w += wq;
                }
            }
            if (rest == 1 && w * cand < best) {
                best = w * cand;
                m = cand;
            }
        }
    }
    return m;
}

// Every route field of the plan, in dependency order, each set once.  Reads the developer knobs (once each) and makes no HIP or hiprtc
// call: the kernels built for the channel count are plan_spec's, the tables plan_build's.
int plan_route(fxc_plan* p, int force_path) {
    const int N = p->nchan, T = p->ntaps;
    // the fused kernel channelises pairs of antenna streams: 2 antennas (X fused in) or 4 / 6 / 8 (F-only +
    // xengine_kernel); num_samp is bounded by the 32-bit buffer-descriptor range of one stream pair
    const bool fused_shape = ((p->n_ant == 2 || p->n_ant == 4 || p->n_ant == 6 || p->n_ant == 8) && N == fxc::fused::kN &&
                              T == fxc::fused::kT && p->num_samp <= (1ll << 27));
    if (force_path == FXC_PATH_FUSED && !fused_shape)
        return fail(p, FXC_ERR_UNSUPPORTED, "no fused kernel for n_ant=%d nchan=%d ntaps=%d", p->n_ant, N, T);
    const bool stream_shape = (p->n_ant == 2 && N == 1);
    if (force_path == FXC_PATH_STREAM && !stream_shape)
        return fail(p, FXC_ERR_UNSUPPORTED, "the streaming kernel needs n_ant=2, nchan=1");
    // 2 antennas: X fused into the tiled kernel; 3 .. 8: F-only tiled kernel (an odd stream count leaves the last pair
    // half empty) + X-engine
    // 16 .. 256 channels, up to four taps: the wave-local variant of the tiled design (k_small.h) -- 2 antennas in one
    // F+X kernel, 3 .. 64 through its F-only variant + X-engine
    // (32-bit frame counters in the kernel; more than four taps: behind the pre-filter pass, whose buffer descriptors bound the stream)
    const bool small_n = small_nchan(N) && p->num_samp / N < (1ll << 31) && (T <= 4 || p->num_samp <= (1ll << 27));
    const bool small_shape = small_n && p->n_ant >= 2 && p->n_ant <= kMaxXAnt;
    const bool tiled_shape = small_shape || (p->n_ant >= 2 && p->n_ant <= kMaxXAnt && tiled_nchan(N) && p->num_samp <= (1ll << 27));
    if (force_path == FXC_PATH_TILED && !tiled_shape)
        return fail(p, FXC_ERR_UNSUPPORTED, "no tiled kernel for n_ant=%d nchan=%d", p->n_ant, N);
    p->path = FXC_PATH_GENERIC;
    if (tiled_shape && (force_path == -1 || force_path == FXC_PATH_TILED)) p->path = FXC_PATH_TILED;
    if (fused_shape && (force_path == -1 || force_path == FXC_PATH_FUSED)) p->path = FXC_PATH_FUSED;
    if (stream_shape && (force_path == -1 || force_path == FXC_PATH_STREAM)) p->path = FXC_PATH_STREAM;
    if (p->path == FXC_PATH_FUSED) {
        if (const char* e = FXC_DEV_ENV("FXC_FUSED_SEG")) p->fused_seg = std::max<int64_t>(1, std::atoll(e));   // developer knob
    }

    // generic F stage: every channel count that is not a power of two (and fits two LDS rows) takes the mixed-radix kernel;
    // FXC_GENERIC_FFT=mixed|radix2 moves the powers of two onto it / everything off it (developer knob)
    const char* gf = FXC_DEV_ENV("FXC_GENERIC_FFT");
    const bool force_mixed = gf && !std::strcmp(gf, "mixed");
    // (off the powers of two "radix2" means the direct DFT, a kernel only the developer build has)
    const bool force_old = gf && !std::strcmp(gf, "radix2") && (p->pow2 || FXC_DEV_KERNELS);
    // powers of two on the automatic path that no tuned kernel takes -- 4, 8 and 16384 channels -- ride along; a forced
    // generic path keeps the radix-2 kernels (the tests' independent reference)
    const bool auto_pow2 = force_path == -1 && (N == 4 || N == 8 || N == 16384);
    const fxc::MixedPlan direct = fxc::mixed_factor(N);
    p->mixed = N > 1 && N <= kMaxLdsFftN && !force_old && (!p->pow2 || force_mixed || auto_pow2) && direct.n_stages >= 0;
    p->rtc = env_int("FXC_RTC", 1) != 0;
    if (p->mixed) {
        // a large prime factor costs more as an O(N p) stage than the whole transform as a chirp-z convolution.  Measured
        // (profiles/r04/experiments.md §7): the stage costs ~p, the chirp-z rows ~nfft / N; they cross near p = 45 nfft / N
        int pmax = 1;
        for (int st = 0; st < direct.n_stages; ++st) pmax = std::max(pmax, direct.radix[st]);
        const int m = blu_length(N);
        const int p_min = FXC_DEV_ENV_INT("FXC_BLU_MIN_PRIME", (int)((int64_t)kBluPrimePerRatio * m / N));
        p->mixed_blu = pmax > p_min && m <= kBluMaxNfft;
        p->blu_nfft = p->mixed_blu ? m : 0;
        p->mixed_plan = p->mixed_blu ? fxc::mixed_factor(m) : direct;
        // (512 threads per row beyond 1320 channels, where three 256-thread workgroups stop fitting a CU's LDS: two antennas
        // 1350 ... 2000 channels 18 - 20 % faster, F only with two frames per slot 10 - 25 %; 1120 ... 1300 slower)
        const int tpr_cap = FXC_DEV_ENV_INT("FXC_MIXED_TPR", 1024), wide_from = FXC_DEV_ENV_INT("FXC_MIXED_WIDE_FROM", 1320);
        p->mixed_tpr = p->mixed_blu ? fxc::mixed_threads_per_row(m, 1024) : fxc::mixed_threads_per_row(N, tpr_cap, p->n_ant == 2, wide_from);
        p->mixed_xeng = p->n_ant >= 3 && FXC_DEV_ENV_INT("FXC_MIXED_XENGINE", 1);
    }
    if (p->mixed && !p->mixed_blu && p->n_ant == 2 && FXC_DEV_ENV_INT("FXC_MIXED_XF", 1)) {
        const size_t rpw = (size_t)(std::max(256, p->mixed_tpr) / p->mixed_tpr);
        // four rows (two antennas x ping-pong) must fit the LDS, with the twiddle table beside them (up to 4096 channels) or
        // without (up to 5120)
        p->mixed_xf_twl = (rpw * 4 + 1) * (size_t)N * sizeof(cf) <= (size_t)(160 * 1024) && FXC_DEV_ENV_INT("FXC_MIXED_TWLDS", 1);
        // (without the table in LDS that kernel has no register butterflies for 11 / 13: such channel counts go through the
        // F-only kernel, which has, and xmul_kernel)
        p->mixed_xf = rpw * 4 * (size_t)N * sizeof(cf) <= (size_t)(160 * 1024) && N <= kMixedXPoints * p->mixed_tpr &&
                      (p->mixed_xf_twl || fxc::mixed_rows_per_slot_cap(p->mixed_plan) != 1);
    }

    // the tiled design: 16 .. 256 channels inside one wave (small, small_f), 512 .. 8192 on workgroups (tiled_kernels)
    p->small = small_shape && p->n_ant == 2 && p->path == FXC_PATH_TILED;
    p->small_f = small_n && force_path != FXC_PATH_GENERIC;
    p->tiled_f = p->small_f || (tiled_nchan(N) && p->num_samp <= (1ll << 27) && force_path != FXC_PATH_GENERIC);
    const bool tiled = p->small || p->small_f || tiled_kernels(p);
    // nchan 8192, two antennas, up to four taps: two passes (f8192_ring_kernel and its XM form, h_launch.h::tiled_raw_sums;
    // FXC_X8192=0: off) -- or else, up to 16 taps, the split into two 4096-channel problems (FXC_SPLIT8192=0: off)
    const bool pair8192 = N == 8192 && p->n_ant == 2 && p->path == FXC_PATH_TILED;
    const bool f8192_knob = N == 8192 && T <= 4 && tiled && FXC_DEV_ENV_INT("FXC_F8192", 1);
    const bool want_x8192 = pair8192 && T <= 4 && p->num_samp < (1ll << 28) && f8192_knob && FXC_DEV_ENV_INT("FXC_X8192", 1);
    p->split8192 = pair8192 && T <= 16 && p->num_samp <= (1ll << 27) && !want_x8192 && FXC_DEV_ENV_INT("FXC_SPLIT8192", 1) != 0;
    // more than four taps (FXC_PREFILTER=1: developer knob, the same at <= 4): pfb_prefilter_kernel applies the FIR first
    // (k_prepass.h), the tiled kernels then run with one unit tap; the split route filters inside its own pass
    p->prefilter = tiled && !p->split8192 && (T > 4 || FXC_DEV_ENV_INT("FXC_PREFILTER", 0) == 1);
    p->pre_tp = p->split8192 ? (T <= 4 ? 4 : (T <= 8 ? 8 : 16)) : p->prefilter ? (T <= 8 ? 8 : (T <= 16 ? 16 : 32)) : 0;
    p->tiled_ring = tiled_kernels(p) && (T <= 4 || p->prefilter) && N <= 4096;
    // 8192 channels, up to four taps: the F stage alone has a ring kernel of its own (k_tiled.h::f8192_ring_kernel), fed with the
    // same window quads from L2.  FXC_F8192=0: the pair kernel (developer knob)
    p->f8192 = f8192_knob && tiled_kernels(p) && !p->prefilter;
    p->x8192 = want_x8192 && p->f8192;

    // more than 8 antennas: the matrix-core X-engine (k_xmfma.h) unless FXC_XENGINE=block (developer knob: the vector
    // kernel over blocks of 8 antennas it replaced)
    if (p->n_ant > kXB) {
        const char* xe = FXC_DEV_ENV("FXC_XENGINE");
        p->x_mfma = !(FXC_DEV_KERNELS && xe && std::string(xe) == "block");
    }
    return FXC_OK;
}

// The kernels built for the channel count (fx_spec.h through hiprtc, h_rtc.h) that two-antenna mixed-radix plans take from the
// start: the F+X one -- every sample fetched once, strides and trip counts compile-time constants -- or, above 4096 channels where
// there is none (sixteen points of two antennas: 256 registers of ring), the F stage alone, which then takes complex64 input with
// xmul_kernel (h_launch.h::mixed_one_pass).  Sets spec, spec_f and xf_bytes_only only.  FXC_RTC=0 keeps the any-shape kernel
// (developer knob, and what a box without hiprtc runs)
void plan_spec(fxc_plan* p) {
    const int N = p->nchan, T = p->ntaps;
    if (!p->mixed_xf || !spec_eligible(p)) return;
    if (!spec_first_radices(N, T).empty()) spec_once(p, &p->spec, &p->spec_tried, kSpecC64);
    if (!p->spec && N > 4096 && FXC_DEV_ENV_INT("FXC_MIXED_XF_BYTES_ONLY", 1) && !spec_first_radices(N, T, spec_rows(N, kSpecFOnly)).empty())
        p->xf_bytes_only = spec_once(p, &p->spec_f, &p->spec_f_tried, kSpecFOnly) != nullptr;
}

// ---- tables ------------------------------------------------------------------------------------------
template <class V>
int upload(fxc_plan* p, DevBuf<V>& dst, const std::vector<V>& host) {
    FXC_HIP(p, dst.alloc(host.size()));
    FXC_HIP(p, hipMemcpy(dst, host.data(), host.size() * sizeof(V), hipMemcpyHostToDevice));
    return FXC_OK;
}

cf expi(double ph) { return fxc::mk((float)std::cos(ph), (float)std::sin(ph)); }

// window quads [N]: quad[m] = (h[m], h[N + m], h[2N + m], h[3N + m]), zeros beyond the taps -- or one unit tap (behind the pre-filter)
std::vector<f4> window_quads(const std::vector<float>& wf, int N, int T, bool unit_tap) {
    std::vector<f4> w4((size_t)N);
    for (int m = 0; m < N; ++m) {
        w4[m].x = unit_tap ? 1.f : wf[m];
        w4[m].y = (T > 1 && !unit_tap) ? wf[(size_t)1 * N + m] : 0.f;
        w4[m].z = (T > 2 && !unit_tap) ? wf[(size_t)2 * N + m] : 0.f;
        w4[m].w = (T > 3 && !unit_tap) ? wf[(size_t)3 * N + m] : 0.f;
    }
    return w4;
}

// [tp][N] reversed polyphase coefficients of the pre-filter and split passes, zeros beyond the taps
std::vector<float> reversed_taps(const std::vector<float>& wf, int N, int T, int tp) {
    std::vector<float> hp((size_t)tp * N, 0.f);
    for (int t = 0; t < T; ++t)
        for (int n = 0; n < N; ++n) hp[(size_t)t * N + n] = wf[(size_t)t * N + (N - 1 - n)];
    return hp;
}

// generic FFT twiddles exp(+2 pi i j / n): cnt of them
std::vector<cf> fft_twiddles(int cnt, int n) {
    std::vector<cf> tw((size_t)cnt);
    for (int j = 0; j < cnt; ++j) tw[j] = expi(kTwoPi * (double)j / (double)n);
    return tw;
}

// the stages of the 4096-point transform (fused and tiled kernels): tw1 [16][256] w4096^(j k1), tw2 [16][16] w256^(j0 q1)
std::vector<cf> stage_tw1() {
    std::vector<cf> tw((size_t)16 * 256);
    for (int k1 = 0; k1 < 16; ++k1)
        for (int jx = 0; jx < 256; ++jx) tw[k1 * 256 + jx] = expi(kTwoPi * (double)((jx * k1) % 4096) / 4096.0);
    return tw;
}
std::vector<cf> stage_tw2() {
    std::vector<cf> tw((size_t)256);
    for (int q1 = 0; q1 < 16; ++q1)
        for (int j0 = 0; j0 < 16; ++j0) tw[q1 * 16 + j0] = expi(kTwoPi * (double)(j0 * q1) / 256.0);
    return tw;
}

// tiled pre-stage twiddles wN^((u + P g) k) at [g + G k][u]
std::vector<cf> tiled_tw0(int N) {
    const int P = N / 16, R0 = N >= 4096 ? N / 4096 : N / 256, G = 16 / R0;
    std::vector<cf> tw((size_t)16 * P);
    for (int r = 0; r < 16; ++r)
        for (int u = 0; u < P; ++u) {
            const int g = r % G, k = r / G;
            tw[(size_t)r * P + u] = expi(kTwoPi * (double)(((int64_t)(u + P * g) * k) % N) / (double)N);
        }
    return tw;
}

// the wave-local kernels' twiddles [N/16][16] wN^(u k1)
std::vector<cf> small_twiddles(int N) {
    std::vector<cf> tw((size_t)N);
    for (int u = 0; u < N / 16; ++u)
        for (int k1 = 0; k1 < 16; ++k1) tw[(size_t)u * 16 + k1] = expi(kTwoPi * (double)((u * k1) % N) / (double)N);
    return tw;
}

// the split route's twiddles [4096] w8192^(4095 - n)
std::vector<cf> split_twiddles() {
    std::vector<cf> tw((size_t)4096);
    for (int n = 0; n < 4096; ++n) tw[n] = expi(kTwoPi * (double)(4095 - n) / 8192.0);
    return tw;
}

// float64 transform of any length on the host, kernel exp(+2 pi i j k / n): decimation in time over the smallest prime factor,
// a direct sum for a prime length (the chirp-z table: 7-smooth lengths up to 8192, built once per plan)
std::vector<cd> host_dft(const std::vector<cd>& x) {
    const int n = (int)x.size();
    if (n == 1) return x;
    int p1 = n;
    for (int q = 2; q * q <= n; ++q)
        if (n % q == 0) {
            p1 = q;
            break;
        }
    std::vector<cd> out((size_t)n);
    if (p1 == n) {
        for (int k = 0; k < n; ++k) {
            double ar = 0.0, ai = 0.0;
            for (int j = 0; j < n; ++j) {
                const double ph = kTwoPi * (double)(((int64_t)j * k) % n) / (double)n;
                const double wr = std::cos(ph), wi = std::sin(ph);
                ar += x[j].x * wr - x[j].y * wi;
                ai += x[j].x * wi + x[j].y * wr;
            }
            out[k].x = ar;
            out[k].y = ai;
        }
        return out;
    }
    const int m = n / p1;                                   // x[p1 j + r] -> p1 transforms of m points
    std::vector<std::vector<cd>> sub((size_t)p1);
    for (int r = 0; r < p1; ++r) {
        std::vector<cd> part((size_t)m);
        for (int j = 0; j < m; ++j) part[j] = x[(size_t)p1 * j + r];
        sub[r] = host_dft(part);
    }
    for (int k = 0; k < n; ++k) {
        double ar = 0.0, ai = 0.0;
        for (int r = 0; r < p1; ++r) {
            const double ph = kTwoPi * (double)(((int64_t)r * k) % n) / (double)n;
            const double wr = std::cos(ph), wi = std::sin(ph);
            const cd v = sub[r][k % m];
            ar += v.x * wr - v.y * wi;
            ai += v.x * wi + v.y * wr;
        }
        out[k].x = ar;
        out[k].y = ai;
    }
    return out;
}

// the chirp-z tables: c[n] = exp(+i pi n^2 / N) with n^2 reduced mod 2N (exact), and D = FFT_M(d) / M for d[m] = d[M - m] = conj(c[m]),
// m < N, zero elsewhere; kernel exp(+2 pi i j k / M), float64 on the host
void chirp_tables(int N, int M, std::vector<cf>* chirp, std::vector<cf>* blud) {
    std::vector<cd> c((size_t)N);
    for (int n = 0; n < N; ++n) {
        const double ph = kTwoPi / 2.0 * (double)(((int64_t)n * n) % (2 * (int64_t)N)) / (double)N;
        c[n].x = std::cos(ph);
        c[n].y = std::sin(ph);
    }
    std::vector<cd> d((size_t)M);
    for (auto& v : d) v.x = v.y = 0.0;
    for (int m = 0; m < N; ++m) {
        d[m].x = c[m].x;
        d[m].y = -c[m].y;
        if (m) d[M - m] = d[m];
    }
    d = host_dft(d);
    chirp->resize((size_t)N);
    blud->resize((size_t)M);
    for (int n = 0; n < N; ++n) (*chirp)[n] = fxc::mk((float)c[n].x, (float)c[n].y);
    for (int k = 0; k < M; ++k) (*blud)[k] = fxc::mk((float)(d[k].x / M), (float)(d[k].y / M));
}

// xengine_kernel for n_ant antennas: 3 .. 8 (cross only; more: xengine_block_kernel), 2 .. 8 with the autos
template <bool AUTOS>
const void* xengine_fn(int n_ant) {
    switch (n_ant) {
        case 3: return reinterpret_cast<const void*>(&xengine_kernel<3, AUTOS>);
        case 4: return reinterpret_cast<const void*>(&xengine_kernel<4, AUTOS>);
        case 5: return reinterpret_cast<const void*>(&xengine_kernel<5, AUTOS>);
        case 6: return reinterpret_cast<const void*>(&xengine_kernel<6, AUTOS>);
        case 7: return reinterpret_cast<const void*>(&xengine_kernel<7, AUTOS>);
        case 8: return reinterpret_cast<const void*>(&xengine_kernel<8, AUTOS>);
        default:
            if constexpr (AUTOS) return reinterpret_cast<const void*>(&xengine_kernel<2, true>);
            else return reinterpret_cast<const void*>(&xengine_block_kernel);
    }
}

// One-wave X-engine workgroups resident on the device: the occupancy API, bounded by the register file (512 VGPRs per SIMD lane in
// granules of 8, at most 8 waves per SIMD) -- the API has been seen one block per CU high (MI355X_MICROARCH.md), and a launch
// sized one wave per CU too large would run a second round for that sliver
int xengine_resident(fxc_plan* p, const void* fn, int64_t* out) {
    int per_cu = 0;
    FXC_HIP(p, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, kXThreads, 0));
    hipFuncAttributes fa;
    FXC_HIP(p, hipFuncGetAttributes(&fa, fn));
    const int regs = std::max(8, (fa.numRegs + 7) / 8 * 8);
    per_cu = std::min(per_cu, 4 * std::min(8, 512 / regs));
    *out = (int64_t)std::max(per_cu, 1) * p->cu_count;
    return FXC_OK;
}

// the device side of the routed plan: stream and events, the tables of its kernels (each allocated once), the result slots, and the
// kernels' LDS attributes and resident workgroups
int plan_build(fxc_plan* p, const double* window) {
    hipDeviceProp_t prop;
    FXC_HIP(p, hipGetDeviceProperties(&prop, p->device));
    p->cu_count = prop.multiProcessorCount;
    if (p->own_stream) FXC_HIP(p, p->stream.create(hipStreamNonBlocking));
    FXC_HIP(p, p->ev_t0.create(hipEventDefault));
    FXC_HIP(p, p->ev_t1.create(hipEventDefault));
    FXC_HIP(p, p->ev_order.create(hipEventDisableTiming));

    const int N = p->nchan, T = p->ntaps;
    for (int t = 0; t < kMaxTaps; ++t) p->taps.h[t] = t < T ? (float)window[t] : 0.f;
    // window: float32 copy of the float64 design [ntaps][nchan]
    std::vector<float> wf((size_t)T * N);
    for (size_t n = 0; n < wf.size(); ++n) wf[n] = (float)window[n];
    if (int rc = upload(p, p->d_win, wf)) return rc;
    // window quads: the fused kernel, the tiled ring kernels, f8192_ring_kernel and the wave-local kernels (one unit tap behind the
    // pre-filter), and the lean builds of fx_spec.h (above 2048 channels, or with a prime factor of 17 ... 23), which read a point's
    // taps as one quad from L2
    const bool tiled_quads = p->small || p->small_f || (tiled_kernels(p) && (p->tiled_ring || p->f8192));
    const bool spec_quads = p->mixed && p->rtc && N <= 8192 && T <= 4;
    if (tiled_quads || spec_quads || p->path == FXC_PATH_FUSED)
        if (int rc = upload(p, p->d_win4, window_quads(wf, N, T, p->prefilter && tiled_quads))) return rc;
    if (p->prefilter || p->split8192)
        if (int rc = upload(p, p->d_hpre, reversed_taps(wf, N, T, p->pre_tp))) return rc;
    if (p->prefilter && tiled_kernels(p))      // (the plain tiled kernel behind the pre-filter)
        if (int rc = upload(p, p->d_ones, std::vector<float>((size_t)N, 1.f))) return rc;
    // generic FFT twiddles: [N/2] for the radix-2 kernel, [N] for the mixed-radix kernel and the direct DFT, [blu_nfft] for the chirp-z rows
    if (N > 1) {
        const int tn = p->mixed_blu ? p->blu_nfft : N;
        if (int rc = upload(p, p->d_tw, fft_twiddles((p->pow2 && !p->mixed) ? N / 2 : tn, tn))) return rc;
    }
    if (p->mixed_blu) {
        std::vector<cf> chirp, blud;
        chirp_tables(N, p->blu_nfft, &chirp, &blud);
        if (int rc = upload(p, p->d_chirp, chirp)) return rc;
        if (int rc = upload(p, p->d_blud, blud)) return rc;
    }
    if (p->path == FXC_PATH_FUSED || tiled_kernels(p)) {
        if (int rc = upload(p, p->d_tw1, stage_tw1())) return rc;
        if (int rc = upload(p, p->d_tw2, stage_tw2())) return rc;
    }
    if (tiled_kernels(p))
        if (int rc = upload(p, p->d_tw0, tiled_tw0(N))) return rc;
    if (p->small || p->small_f)
        if (int rc = upload(p, p->d_tw_small, small_twiddles(N))) return rc;
    if (p->split8192) {
        if (int rc = upload(p, p->d_tw8192, split_twiddles())) return rc;
        if (int rc = upload(p, p->d_unit4, window_quads(wf, fxc::fused::kN, T, true))) return rc;
    }
    cd one;
    one.x = 1.0;
    one.y = 0.0;
    if (int rc = upload(p, p->d_rot, std::vector<cd>((size_t)N, one))) return rc;
    // baseline -> (a, b) for per-antenna rot (fxc_set_rot_ant), in the order of the X-engines: (0,1),(0,2)..(A-2,A-1)
    if (p->n_ant >= 3) {
        std::vector<int2> pair;
        for (int a = 0; a < p->n_ant; ++a)
            for (int b = a + 1; b < p->n_ant; ++b) pair.push_back(make_int2(a, b));
        if (int rc = upload(p, p->d_pair, pair)) return rc;
    }

    const size_t acc_n = (size_t)acc_capacity(p);
    FXC_HIP(p, p->d_acc.alloc(acc_n));
    FXC_HIP(p, hipMemset(p->d_acc, 0, acc_n * sizeof(cd)));
    FXC_HIP(p, p->d_sums.alloc(acc_n + 1));
    FXC_HIP(p, hipMemset(p->d_sums, 0, (acc_n + 1) * sizeof(cd)));
    // finalize results: pinned host memory the finishing kernels write through the device's mapping of it (coherent,
    // so the host sees the bytes once the slot's event has completed)
    for (int k = 0; k < fxc_plan::kResSlots; ++k) {
        FXC_HIP(p, p->h_res[k].alloc(std::max<size_t>(acc_n, 16) * sizeof(cd), hipHostMallocMapped | hipHostMallocCoherent));
        FXC_HIP(p, hipHostGetDevicePointer(reinterpret_cast<void**>(&p->d_res[k]), p->h_res[k], 0));
        FXC_HIP(p, p->ev_res[k].create(hipEventReleaseToSystem));
    }

    // the fused kernel (also behind the 8192-channel split): one 512-thread workgroup (136 KiB LDS) per CU
    if (p->path == FXC_PATH_FUSED || p->split8192) {
        using namespace fxc::fused;
        const std::pair<const void*, int> fused_lds[] = {
            {reinterpret_cast<const void*>(&fx_fused4096_kernel<false, false>), kLdsBytes},
            {reinterpret_cast<const void*>(&fx_fused4096_kernel<true, false>), kLdsBytes},
            {reinterpret_cast<const void*>(&fx_fused4096_kernel<false, true>), kLdsBytes},
            {reinterpret_cast<const void*>(&fx_fused4096_kernel<false, true, true>), kLdsBytes + kDckLdsBytes},
            {reinterpret_cast<const void*>(&fx_fused4096_kernel<false, false, false, true>), kLdsBytes + kAutoLdsBytes},
        };
        for (const auto& f : fused_lds) FXC_HIP(p, hipFuncSetAttribute(f.first, hipFuncAttributeMaxDynamicSharedMemorySize, f.second));
        p->fused_grid_max = p->cu_count;
    }
    if (p->small || p->small_f)
        if (int rc = small_setup(p)) return rc;
    if (tiled_kernels(p)) {
        int rc = FXC_OK;
        FXC_TILED_DISPATCH(p, rc = tiled_setup<G>(p));
        if (rc) return rc;
    }
    if (p->n_ant >= 3 && p->n_ant <= kMaxXAnt) {
        const void* xfn = xengine_fn<false>(p->n_ant);
        if (p->x_mfma) {
            int per_cu = 0, threads = 0, lds = 0;
            FXC_XMFMA_DISPATCH(p, {
                xfn = reinterpret_cast<const void*>(&xengine_mfma_kernel<XT>);
                threads = XMfmaGeo<XT>::kThreads;
                lds = XMfmaGeo<XT>::kLdsBytes;
            });
            FXC_HIP(p, hipFuncSetAttribute(xfn, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
            FXC_HIP(p, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, xfn, threads, lds));
            p->x_resident = (int64_t)std::max(per_cu, 1) * p->cu_count;
        } else if (int rc = xengine_resident(p, xfn, &p->x_resident)) {
            return rc;
        }
    }
    if (p->mixed) {
        const void* const mixed_fns[] = {
            reinterpret_cast<const void*>(&pfb_fft_mixed_kernel<true, 1, false>),
            reinterpret_cast<const void*>(&pfb_fft_mixed_kernel<true, 2, false>),
            reinterpret_cast<const void*>(&pfb_fft_mixed_kernel<false, 1, false>),
            reinterpret_cast<const void*>(&pfb_fft_mixed_kernel<true, 2, true>),
            reinterpret_cast<const void*>(&pfb_fft_mixed_kernel<true, 2, true, false, false, true>),
            reinterpret_cast<const void*>(&pfb_fft_mixed_kernel<false, 2, true>),
            reinterpret_cast<const void*>(&pfb_fft_mixed_kernel<false, 2, true, false, false, true>),
            reinterpret_cast<const void*>(&pfb_fft_mixed_kernel<false, 1, false, false, true>),
            reinterpret_cast<const void*>(&pfb_fft_mixed_kernel<true, 1, false, true>),
            reinterpret_cast<const void*>(&pfb_fft_mixed_kernel<false, 1, false, true>),
        };
        for (const void* fn : mixed_fns) FXC_HIP(p, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    } else if (N > 1) {
        const int lds = N * (int)sizeof(cf);
        if (p->pow2)
            FXC_HIP(p, hipFuncSetAttribute(reinterpret_cast<const void*>(&fft_pow2_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, lds));
#if FXC_DEV_KERNELS
        else
            FXC_HIP(p, hipFuncSetAttribute(reinterpret_cast<const void*>(&dft_any_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, lds));
#endif
    }
    return FXC_OK;
}

}  // namespace
