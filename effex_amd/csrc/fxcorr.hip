// fxcorr.hip — MI355X (gfx950) F/X hot path: the C ABI of include/fxcorr.h over the kernels.
//
// One translation unit.  This file holds the ABI entry points -- argument checks, then a driver of the h_*.h files; it includes
//   fx_math.h, fx_fused4096.h, fx_tiled.h, fx_small.h, fx_mixed.h   index maps, butterflies and kernel phases (also compiled by
//                                           g++ for the host emulation under tests/emul)
//   k_generic.h k_finish.h k_xmfma.h k_fused4096.h k_tiled.h k_small.h k_prepass.h k_stream.h k_conditioning.h k_track.h k_align.h k_synth.h
//   k_delay.h k_fringe.h k_gains.h k_flag.h k_average.h k_beam.h k_kurtosis.h k_dedisperse.h k_boxcar.h
//                                           the __global__ kernels, one file per path / step and per rows tool (delays, fringe fit,
//                                           gain solve, detector, averager, beamformer, spectral kurtosis)
//   h_own.h h_plan.h h_rtc.h h_launch.h h_build.h h_run.h h_modifiers.h h_ingest.h h_pipe.h h_tools.h h_rccl.h
//                                           the owners of device memory, events and streams, fxc_plan, the kernels compiled per
//                                           channel count, the per-path launchers and workspace passes, plan construction (route,
//                                           tables), the device-resident fx_accumulate / fx_rows and the finalize queue, the row
//                                           modifiers (rot tables, delay track, gain track, sample shifts), the ingest front end of
//                                           every entry point that takes samples (formats, DC removal, host / device dispatch), the
//                                           host-fed pipe, the rows tools' drivers and the helpers they share, the run-time binding
//                                           of librccl
//
// Replaces, for effex's hot path:
//   cusignal.filtering.channelize_poly FIR half   effex/effex.py:553   -> pfb_fir_kernel / pfb_fft_mixed_kernel / fused phase 1
//   cusignal channelize_poly FFT half + conj      effex/effex.py:553   -> pfb_fft_mixed_kernel (any channel count: mixed radix,
//                                                                          chirp-z) / fft_pow2_kernel / dft_any_kernel / fused phases 1-3
//   f0 * conj(f1 * rot), mean(axis=0), fftshift   effex/effex.py:516-521 -> xmul_kernel / fused X + finish kernels
//   continuum tail mean_k / bandwidth             effex/effex.py:523-524 -> continuum kernels
// and the steps either side of the path:
//   per-chunk DC removal, uint8 -> complex        effex/effex.py:394-395, :652 -> dc_* / convert_u8 kernels
//   delay calibration                             effex/effex.py:583-627 -> delay_* / stockham_stage kernels
//   per-chunk blocking copies                     effex/effex.py:391-392, 508-509, 693 -> fxc_pipe_* (host side)
// Paths: fused (nchan 4096, ntaps 4; 2 antennas in one kernel, 4/6/8 via F-only + X-engine), tiled (2 antennas,
// nchan 512..8192, any ntaps: the fused design generalised, fx_tiled.h; nchan 16..256, ntaps <= 4: the same inside one
// wave, k_small.h), stream (nchan 1), generic (everything else: channel counts that are not a power of two on the mixed-radix
// kernel of k_generic.h / fx_mixed.h -- with two antennas F and X in one pass --, the rest on plain FIR / FFT / X kernels).  Written for gfx950 only: wave64, 160 KiB LDS, v_permlane32_swap, buffer loads.
// No CPU fallback.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <dlfcn.h>
#include <sys/stat.h>
#include <unistd.h>
// RCCL: types and prototypes only -- the library itself is bound at run time (rccl_api), so a ROCm install without the
// rccl headers still builds libfxcorr (single-GPU users need no RCCL at all)
#if __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>
#else
extern "C" {
typedef struct ncclComm* ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclFloat64 = 8 } ncclDataType_t;
typedef enum { ncclSum = 0 } ncclRedOp_t;
ncclResult_t ncclGetUniqueId(ncclUniqueId* uniqueId);
ncclResult_t ncclCommInitRank(ncclComm_t* comm, int nranks, ncclUniqueId commId, int rank);
ncclResult_t ncclCommDestroy(ncclComm_t comm);
const char* ncclGetErrorString(ncclResult_t result);
ncclResult_t ncclReduce(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype, ncclRedOp_t op, int root,
                        ncclComm_t comm, hipStream_t stream);
ncclResult_t ncclAllReduce(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype, ncclRedOp_t op,
                           ncclComm_t comm, hipStream_t stream);
ncclResult_t ncclCommCount(const ncclComm_t comm, int* count);
ncclResult_t ncclCommUserRank(const ncclComm_t comm, int* rank);
ncclResult_t ncclCommCuDevice(const ncclComm_t comm, int* device);
ncclResult_t ncclGetVersion(int* version);
ncclResult_t ncclCommGetAsyncError(ncclComm_t comm, ncclResult_t* asyncError);
}
#endif

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/fxcorr.h"

// FXC_DEV_KERNELS=1 (libfxcorr_dev.so, built by effex_amd/build.py for the tests and tools only): also the kernels and knobs
// that exist to check or time the shipped ones against -- the direct O(N^2) DFT for channel counts that are not a power of two
// (FXC_GENERIC_FFT=radix2) and the vector X-engine where the matrix-core one serves (FXC_XENGINE=block)
#ifndef FXC_DEV_KERNELS
#define FXC_DEV_KERNELS 0
#endif
namespace {
// an integer from the environment.  The shipped library reads FOUR variables, all documented in include/fxcorr.h: FXC_RTC, FXC_RTC_CACHE,
// FXC_RTC_VERBOSE, FXC_WS_MB.  Every other route / tuning knob exists in the developer library only (libfxcorr_dev.so, -DFXC_DEV_KERNELS=1:
// tests, tools/): FXC_DEV_ENV* below fold to their defaults in the shipped build, strings and all.
int env_int(const char* name, int dflt) {
    const char* e = std::getenv(name);
    return e ? std::atoi(e) : dflt;
}
#define FXC_DEV_ENV(name) (FXC_DEV_KERNELS ? std::getenv(name) : static_cast<const char*>(nullptr))
#define FXC_DEV_ENV_INT(name, dflt) (FXC_DEV_KERNELS ? env_int(name, dflt) : (dflt))
}  // namespace
#include "fx_fused4096.h"
#include "fx_tiled.h"
#include "fx_small.h"
#include "fx_mixed.h"
#include "fx_math.h"

using fxc::cd;
using fxc::cf;
using fxc::f4;

namespace {

constexpr double kTwoPi = 6.283185307179586476925286766559;
constexpr int kMaxTaps = 32;         // cusignal ships 8x8 / 16x16 / 32x32 channeliser kernels only
constexpr int kMaxXAnt = 64;         // antennas the F-only + X-engine route takes (fxc_plan_create's own limit)
constexpr int kMaxAutoAnt = 8;       // antennas fxc_set_products gives autos to (xengine_kernel<A, true>)
constexpr int kMaxLdsFftN = 16384;   // 128 KiB of complex64 in LDS
constexpr int kBluPrimePerRatio = 45;  // prime factors beyond 45 nfft / N: the chirp-z form (see pfb_fft_mixed_kernel, BLU)
constexpr int kBluMaxNfft = 10240;    // two chirp-z rows in the 160 KiB of LDS: up to 5120 channels
constexpr int kMixedMaxN = 10240;    // two rows of complex64 in the 160 KiB of LDS (pfb_fft_mixed_kernel)
size_t res_direct_bytes() {      // finalize results up to this size are written to host memory by the kernel (FXC_RES_DIRECT: developer knob, bytes)
    static const size_t v = [] { const char* e = FXC_DEV_ENV("FXC_RES_DIRECT"); return e ? (size_t)std::atoll(e) : (size_t)(256 << 10); }();
    return v;
}
// upper bound of the lazily grown workspace (288 GB of HBM per GPU): a call over more chunks than fit runs in passes.
// FXC_WS_MB: developer / test knob, the bound in MiB (tests/test_gpu_finish.py forces many passes with it)
int64_t ws_target() {
    static const int64_t v = [] {
        const char* e = std::getenv("FXC_WS_MB");
        const long long mb = e ? std::atoll(e) : 0;
        return mb > 0 ? (int64_t)mb << 20 : (int64_t)12 << 30;
    }();
    return v;
}

}  // namespace

#include "k_generic.h"
#include "k_finish.h"
#include "k_xmfma.h"
#include "k_fused4096.h"
#include "k_tiled.h"
#include "k_small.h"
#include "k_prepass.h"
#include "k_stream.h"
#include "k_conditioning.h"
#include "k_track.h"
#include "k_align.h"
#include "k_delay.h"
#include "k_fringe.h"
#include "k_gains.h"
#include "k_flag.h"
#include "k_average.h"
#include "k_beam.h"
#include "k_kurtosis.h"
#include "k_dedisperse.h"
#include "k_boxcar.h"
#include "k_synth.h"
#include "h_own.h"
#include "h_plan.h"
#include "h_rtc.h"
#include "h_launch.h"
#include "h_build.h"
#include "h_run.h"
#include "h_modifiers.h"
#include "h_ingest.h"
#include "h_pipe.h"
#include "h_tools.h"
#include "h_rccl.h"


// ------------------------------------------------------------------------------------------
// C ABI (include/fxcorr.h)
// ------------------------------------------------------------------------------------------
extern "C" {

int fxc_version(void) { return FXC_VERSION; }
int fxc_dev_kernels(void) { return FXC_DEV_KERNELS; }

const char* fxc_status_string(int status) {
    switch (status) {
        case FXC_OK: return "ok";
        case FXC_ERR_ARG: return "invalid argument";
        case FXC_ERR_UNSUPPORTED: return "unsupported configuration";
        case FXC_ERR_HIP: return "HIP runtime error";
        case FXC_ERR_NOMEM: return "out of device memory";
        case FXC_ERR_NODEVICE: return "no HIP device";
        case FXC_ERR_STATE: return "invalid call sequence";
        case FXC_ERR_COMM: return "RCCL unavailable or a collective failed";
        default: return "unknown status";
    }
}

int fxc_device_count(int* count) {
    if (!count) return fail(nullptr, FXC_ERR_ARG, "count is NULL");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
    return FXC_OK;
}

const char* fxc_last_error(const fxc_plan* plan) { return plan ? plan->error.c_str() : g_lib_error.c_str(); }

int fxc_plan_destroy(fxc_plan* p) {
    if (!p) return FXC_OK;
    if (p->live_pipes > 0)
        return fail(p, FXC_ERR_STATE, "%d pipe(s) still use this plan: destroy them first", p->live_pipes);
    DeviceGuard device_guard__(p->device);
    (void)hipStreamSynchronize(p->stream);
    if (p->big_res) (void)hipStreamSynchronize(p->big_res.s_copy);   // an uncollected large result may still be on its way to h_res[]
    delete p;      // memory, then events, then streams: the order of fxc_plan's members (h_plan.h)
    return FXC_OK;
}

int fxc_plan_create(fxc_plan** out, int device, int n_ant, int nchan, int ntaps, int64_t num_samp,
                    const double* window, void* stream, int force_path) {
    if (!out) return fail(nullptr, FXC_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!window) return fail(nullptr, FXC_ERR_ARG, "window is NULL");
    if (n_ant < 1 || n_ant > 64) return fail(nullptr, FXC_ERR_ARG, "n_ant=%d out of range [1,64]", n_ant);
    if (nchan < 1) return fail(nullptr, FXC_ERR_ARG, "nchan=%d must be >= 1", nchan);
    if (ntaps < 1) return fail(nullptr, FXC_ERR_ARG, "ntaps=%d must be >= 1", ntaps);
    if (ntaps > kMaxTaps)
        return fail(nullptr, FXC_ERR_UNSUPPORTED, "Number of taps (%d) must be less than (32).", ntaps);
    if (nchan > kMaxLdsFftN)
        return fail(nullptr, FXC_ERR_UNSUPPORTED, "nchan=%d exceeds the in-LDS FFT limit %d", nchan, kMaxLdsFftN);
    if (num_samp < nchan)
        return fail(nullptr, FXC_ERR_ARG, "num_samp=%lld shorter than one frame of nchan=%d", (long long)num_samp,
                    nchan);
    if (force_path < -1 || force_path > FXC_PATH_TILED) return fail(nullptr, FXC_ERR_ARG, "bad force_path");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(nullptr, FXC_ERR_NODEVICE, "no HIP device available (this library has no CPU backend)");
    if (device < 0 || device >= ndev) return fail(nullptr, FXC_ERR_ARG, "device %d out of range [0,%d)", device, ndev);
    FXC_DEVICE(nullptr, device);

    fxc_plan* p = new (std::nothrow) fxc_plan();
    if (!p) return fail(nullptr, FXC_ERR_NOMEM, "host allocation failed");
    p->device = device;
    p->n_ant = n_ant;
    p->n_base = n_ant * (n_ant - 1) / 2;
    p->n_prod = p->n_base;
    p->nchan = nchan;
    p->ntaps = ntaps;
    p->num_samp = num_samp;
    p->n_pts = num_samp / nchan;
    p->pow2 = (nchan & (nchan - 1)) == 0;
    p->lg2n = 0;
    while ((1 << p->lg2n) < nchan) ++p->lg2n;
    p->own_stream = (stream == FXC_STREAM_OWNED);
    if (!p->own_stream) p->stream.borrow(static_cast<hipStream_t>(stream));
    int rc = plan_route(p, force_path);
    if (rc == FXC_OK) {
        plan_spec(p);
        rc = plan_build(p, window);
    }
    if (rc != FXC_OK) {
        g_lib_error = p->error;
        fxc_plan_destroy(p);
        return rc;
    }
    *out = p;
    return FXC_OK;
}

int fxc_plan_get_info(const fxc_plan* p, fxc_info* info) {
    if (!p || !info) return fail(p, FXC_ERR_ARG, "NULL argument");
    std::memset(info, 0, sizeof *info);
    info->n_ant = p->n_ant;
    info->n_baselines = p->n_base;
    info->nchan = p->nchan;
    info->ntaps = p->ntaps;
    info->num_samp = p->num_samp;
    info->n_pts = p->n_pts;
    info->path = p->path;
    if (p->path == FXC_PATH_FUSED) {
        info->grid = p->fused_grid_max;
        info->block = fxc::fused::kThreads;
        info->lds_bytes = fxc::fused::kLdsBytes;
    } else if (p->path == FXC_PATH_TILED && small_nchan(p->nchan)) {
        info->grid = p->small_wgs;
        info->block = 256;
        info->lds_bytes = p->nchan * (int)sizeof(f4) + 4 * 1088 * (int)sizeof(cf);
    } else if (p->path == FXC_PATH_TILED) {
        info->grid = p->tiled_grid_max;
        info->block = p->nchan / 8;
        info->lds_bytes = 2 * (p->nchan + p->nchan / 16) * (int)sizeof(cf) + 256 * (int)sizeof(cf) +
                          (p->tiled_ring ? p->nchan * (int)sizeof(f4) : 0);
    } else if (p->path == FXC_PATH_STREAM) {
        info->grid = (int)stream_blocks(p);
        info->block = 256;
        info->lds_bytes = 2 * (kStreamBlock + p->ntaps - 1) * (int)sizeof(cf);
    } else {
        info->grid = p->cu_count * 4;
        info->block = 256;
        info->lds_bytes = p->nchan > 1 ? p->nchan * (int)sizeof(cf) : 0;
    }
    if (p->x8192) {       // 8192 channels, two antennas, two passes: f8192_ring_kernel and its XM form
        info->grid = p->cu_count * 8;
        info->block = kF8192Threads;
        info->lds_bytes = kF8192LdsCf * (int)sizeof(cf);
    }
    if (p->spec_f) info->specialised |= 2;
    if (p->spec_xm) info->specialised |= 4;
    if (p->spec) {
        info->specialised |= 1;
        info->spec_vgprs = p->spec->vgprs;
        info->spec_source = p->spec->source;
        info->spec_seconds = (float)p->spec->seconds;
        info->grid = p->cu_count * p->spec->wgs_per_cu;
        info->block = p->spec->shape.threads();
        info->lds_bytes = (int)p->spec->shape.lds_bytes();
    } else if (p->spec_f) {      // (no one-pass build: where the F-only build -- and the second pass behind it -- came from, what both took)
        info->spec_vgprs = p->spec_f->vgprs;
        info->spec_source = p->spec_f->source;
        info->spec_seconds = (float)(p->spec_f->seconds + (p->spec_xm ? p->spec_xm->seconds : 0.0));
    }
    info->device = p->device;
    info->cu_count = p->cu_count;
    info->workspace_bytes = (int64_t)p->d_ws.bytes();
    return FXC_OK;
}

int fxc_spec_probe(int nchan, int ntaps, int variant, const char* arch, char* report, int report_bytes) {
    if (variant < 0 || variant > 3) return fail(nullptr, FXC_ERR_ARG, "variant %d: 0 complex64 F+X, 1 bytes F+X, 2 F only, 3 second pass (F x another stream's spectra)", variant);
    if (report && report_bytes > 0) report[0] = 0;
    if (spec_first_radices(nchan, ntaps, spec_rows(nchan, variant)).empty())
        return fail(nullptr, FXC_ERR_UNSUPPORTED, "no specialised kernel for %d channels, %d taps", nchan, ntaps);
    std::string target = arch ? arch : "";
    if (target.empty()) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess)
            return fail(nullptr, FXC_ERR_NODEVICE, "no HIP device to take the architecture from");
        target = spec_arch(prop.gcnArchName);
    }
    const SpecBuild b = spec_search(nchan, ntaps, variant, target.c_str());
    if (b.image.empty()) return fail(nullptr, b.scratch ? FXC_ERR_UNSUPPORTED : FXC_ERR_HIP, "%s", b.error.c_str());
    if (report && report_bytes > 0) {
        const SpecShape& sh = b.shape;
        std::snprintf(report, (size_t)report_bytes,
                      "nchan=%d ntaps=%d tpr=%d slots=%d frames_per_step=%d stages=%s lds_bytes=%zu code_bytes=%zu vgprs=%lld scratch=%lld resident=%d lean=%d rows=%d "
                      "groups=%s pads=%s plane0=%d twfull=%d waves=%d source=%s",
                      sh.n, sh.taps, sh.tpr, sh.slots, sh.u, sh.list(sh.radix).c_str(), sh.lds_bytes(), b.image.size(), b.vgprs, b.scratch, b.resident,
                      (int)sh.lean, sh.rows, sh.list(sh.grp).c_str(), sh.list(sh.pad).c_str(), sh.plane0, sh.twfull, sh.waves,
                      b.source == kSpecPrebuilt ? "prebuilt" : b.source == kSpecCached ? "cache" : "built");
    }
    return FXC_OK;
}

int fxc_set_delay_track(fxc_plan* p, const double* tau0_s, const double* rate_s_per_chunk, double bandwidth, double frequency,
                        int64_t first_chunk) {
    return set_delay_track(p, tau0_s, rate_s_per_chunk, bandwidth, frequency, first_chunk, false);
}

int fxc_set_delay_track_aligned(fxc_plan* p, const double* tau0_s, const double* rate_s_per_chunk, double bandwidth, double frequency,
                                int64_t first_chunk) {
    return set_delay_track(p, tau0_s, rate_s_per_chunk, bandwidth, frequency, first_chunk, true);
}

int fxc_set_sample_delays(fxc_plan* p, const int64_t* shift_samples) {
    if (!p) return fail(p, FXC_ERR_ARG, "NULL plan");
    bool any = false;
    for (int a = 0; shift_samples && a < p->n_ant; ++a) {
        const int64_t s = shift_samples[a];
        if (s >= p->num_samp || s <= -p->num_samp)
            return fail(p, FXC_ERR_ARG, "shift %lld of antenna %d leaves none of the chunk's %lld samples", (long long)s, a, (long long)p->num_samp);
        any = any || s != 0;
    }
    if (any && p->track && p->track_align)
        return fail(p, FXC_ERR_STATE, "the aligned delay track sets the shifts of every chunk: end it first");
    if (any && p->num_samp > kAlignMaxSamp)
        return fail(p, FXC_ERR_UNSUPPORTED, "whole-sample delays take chunks of up to 2^27 samples, the plan's have %lld", (long long)p->num_samp);
    return set_sample_delays(p, shift_samples);
}

int fxc_sample_delays(const fxc_plan* p, int64_t chunk, int64_t* shift_samples_out) {
    if (!p || !shift_samples_out) return fail(p, FXC_ERR_ARG, "NULL argument");
    if (chunk < 0) return fail(p, FXC_ERR_ARG, "chunk < 0");
    for (int a = 0; a < p->n_ant; ++a)
        shift_samples_out[a] = p->track && p->track_align ? track_shift_host(p, a, chunk) : (p->shifted ? p->sample_shift[(size_t)a] : 0);
    return FXC_OK;
}

int fxc_set_track_gains(fxc_plan* p, const double* gains_re_im, int64_t n_solutions, int64_t interval, int64_t first_chunk) {
    if (!p) return fail(p, FXC_ERR_ARG, "NULL plan");
    if (n_solutions < 0) return fail(p, FXC_ERR_ARG, "n_solutions < 0");
    if (n_solutions > 0 && !gains_re_im) return fail(p, FXC_ERR_ARG, "gains_re_im is NULL");
    if (interval < 0 || (interval < 1 && n_solutions > 1))
        return fail(p, FXC_ERR_ARG, "interval=%lld: %lld solutions need an interval of 1 chunk or more", (long long)interval, (long long)n_solutions);
    if (first_chunk < 0) return fail(p, FXC_ERR_ARG, "first_chunk < 0");
    const size_t per = (size_t)p->n_ant * (size_t)p->nchan;
    if ((uint64_t)n_solutions > ((uint64_t)1 << 46) / (per * sizeof(cd)))
        return fail(p, FXC_ERR_NOMEM, "%lld solutions of %zu gains do not fit the device", (long long)n_solutions, per);
    const size_t count = (size_t)n_solutions * per;
    for (size_t i = 0; i < count; ++i) {
        const double x = gains_re_im[2 * i], y = gains_re_im[2 * i + 1];
        if (!std::isfinite(x) || !std::isfinite(y)) return fail(p, FXC_ERR_ARG, "gain %zu is not finite", i);
        const double m = std::hypot(x, y);
        // d = x x + y y of the inverse must neither overflow nor underflow
        if (m != 0.0 && (m < 1e-150 || m > 1e150)) return fail(p, FXC_ERR_ARG, "|gain %zu| = %g outside [1e-150, 1e150]", i, m);
    }
    if (!p->track) return fail(p, FXC_ERR_STATE, "the plan has no delay track");
    if (!acc_empty(p)) return fail(p, FXC_ERR_STATE, "the accumulator holds chunks: finalize or reset it first");
    if (p->live_pipes) return fail(p, FXC_ERR_STATE, "an fxc_pipe uses the plan");
    return set_track_gains(p, gains_re_im, n_solutions, interval, first_chunk, count);
}

int fxc_track_gains_info(const fxc_plan* p, int64_t* n_solutions, int64_t* interval, int64_t* first_chunk) {
    if (!p || !n_solutions || !interval || !first_chunk) return fail(p, FXC_ERR_ARG, "NULL argument");
    if (!p->track) return fail(p, FXC_ERR_STATE, "the plan has no delay track");
    *n_solutions = p->gain_n;
    *interval = p->gain_n ? p->gain_interval : 0;
    *first_chunk = p->gain_n ? p->gain_first : 0;
    return FXC_OK;
}

int fxc_delay_track_chunk(const fxc_plan* p, int64_t* next_chunk) {
    if (!p || !next_chunk) return fail(p, FXC_ERR_ARG, "NULL argument");
    if (!p->track) return fail(p, FXC_ERR_STATE, "the plan has no delay track");
    *next_chunk = p->track_t;
    return FXC_OK;
}

int fxc_delay_track_seek(fxc_plan* p, int64_t chunk) {
    if (!p) return fail(p, FXC_ERR_ARG, "NULL plan");
    if (chunk < 0) return fail(p, FXC_ERR_ARG, "chunk < 0");
    if (!p->track) return fail(p, FXC_ERR_STATE, "the plan has no delay track");
    p->track_t = chunk;
    return FXC_OK;
}

int fxc_delay_track_tables(fxc_plan* p, int64_t chunk, double* out_re_im) {
    if (!p || !out_re_im) return fail(p, FXC_ERR_ARG, "NULL argument");
    if (chunk < 0) return fail(p, FXC_ERR_ARG, "chunk < 0");
    if (!p->track) return fail(p, FXC_ERR_STATE, "the plan has no delay track");
    return delay_track_tables(p, chunk, out_re_im);
}

int fxc_set_rot(fxc_plan* p, const double* rot_re_im) {
    if (!p || !rot_re_im) return fail(p, FXC_ERR_ARG, "NULL argument");
    return set_rot(p, rot_re_im);
}

int fxc_set_rot_ant(fxc_plan* p, const double* rot_ant_re_im) {
    if (!p || !rot_ant_re_im) return fail(p, FXC_ERR_ARG, "NULL argument");
    if (p->n_ant < 2) return fail(p, FXC_ERR_ARG, "per-antenna rot needs 2 or more antennas, the plan has %d", p->n_ant);
    return set_rot_ant(p, rot_ant_re_im);
}

int fxc_set_products(fxc_plan* p, int products) {
    if (!p) return fail(p, FXC_ERR_ARG, "NULL plan");
    if (products != FXC_PRODUCTS_CROSS && products != FXC_PRODUCTS_CROSS_AUTO) return fail(p, FXC_ERR_ARG, "bad products %d", products);
    const bool autos = products == FXC_PRODUCTS_CROSS_AUTO;
    if (autos && (p->n_ant < 2 || p->n_ant > kMaxAutoAnt))
        return fail(p, FXC_ERR_UNSUPPORTED, "autos are produced for 2 .. %d antennas, not %d", kMaxAutoAnt, p->n_ant);
    // the accumulator, a queued result and a pipe's slots are all laid out in rows of the current products
    if (p->live_pipes) return fail(p, FXC_ERR_STATE, "an fxc_pipe uses the plan");
    if (p->res_head != p->res_tail) return fail(p, FXC_ERR_STATE, "finalize results outstanding");
    if (p->spectra_count > 0.0 || p->pend.valid) return fail(p, FXC_ERR_STATE, "the accumulator is not empty");
    if (autos == p->autos) return FXC_OK;
    FXC_DEVICE(p, p->device);
    if (autos && !p->x_resident_auto) {
        const int rc = xengine_resident(p, xengine_fn<true>(p->n_ant), &p->x_resident_auto);
        if (rc) return rc;
    }
    // the rows past the cross rows start from zero (they were never written, or an earlier autos plan cleared them)
    FXC_HIP(p, hipMemsetAsync(p->d_acc, 0, (size_t)acc_capacity(p) * sizeof(cd), p->stream));
    p->autos = autos;
    p->n_prod = p->n_base + (autos ? p->n_ant : 0);
    p->sums_valid = false;          // reduced sums of the other layout
    return FXC_OK;
}

int fxc_plan_products(const fxc_plan* p, int* products, int* n_rows) {
    if (!p) return fail(p, FXC_ERR_ARG, "NULL plan");
    if (products) *products = p->autos ? FXC_PRODUCTS_CROSS_AUTO : FXC_PRODUCTS_CROSS;
    if (n_rows) *n_rows = p->n_prod;
    return FXC_OK;
}

int fxc_set_stream(fxc_plan* p, void* stream) {
    if (!p) return fail(p, FXC_ERR_ARG, "NULL plan");
    if (p->own_stream) return fail(p, FXC_ERR_STATE, "the plan owns its stream (FXC_STREAM_OWNED)");
    hipStream_t next = static_cast<hipStream_t>(stream);
    if (next == p->stream) return FXC_OK;
    FXC_DEVICE(p, p->device);
    // the plan's workspace, accumulator and tables are shared by everything it launches: what is queued on the old
    // stream completes before anything on the new one starts (device-side dependency, no host wait)
    FXC_HIP(p, hipEventRecord(p->ev_order, p->stream));
    FXC_HIP(p, hipStreamWaitEvent(next, p->ev_order, 0));
    p->stream.borrow(next);
    return FXC_OK;
}


int fxc_comm_unique_id(void* id_out) {
    if (!id_out) return fail(nullptr, FXC_ERR_ARG, "id_out is NULL");
    static_assert(sizeof(ncclUniqueId) == FXC_COMM_ID_BYTES, "FXC_COMM_ID_BYTES must match ncclUniqueId");
    RcclApi* api = rccl_api();
    if (!api->handle) return fail(nullptr, FXC_ERR_COMM, "%s", api->error.c_str());
    ncclUniqueId id;
    const ncclResult_t r = api->get_unique_id(&id);
    if (r != ncclSuccess) return rccl_fail(nullptr, api, "ncclGetUniqueId", r);
    std::memcpy(id_out, &id, sizeof id);
    return FXC_OK;
}

int fxc_comm_create(void** rccl_comm_out, int device, int rank, int world_size, const void* id) {
    if (!rccl_comm_out || !id) return fail(nullptr, FXC_ERR_ARG, "NULL argument");
    *rccl_comm_out = nullptr;
    if (world_size < 1 || rank < 0 || rank >= world_size) return fail(nullptr, FXC_ERR_ARG, "rank %d outside world of %d", rank, world_size);
    RcclApi* api = rccl_api();
    if (!api->handle) return fail(nullptr, FXC_ERR_COMM, "%s", api->error.c_str());
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(nullptr, FXC_ERR_NODEVICE, "no HIP device available");
    if (device < 0 || device >= ndev) return fail(nullptr, FXC_ERR_ARG, "device %d out of range [0,%d)", device, ndev);
    FXC_DEVICE(nullptr, device);
    ncclUniqueId uid;
    std::memcpy(&uid, id, sizeof uid);
    ncclComm_t comm = nullptr;
    const ncclResult_t r = api->comm_init_rank(&comm, world_size, uid, rank);
    if (r != ncclSuccess) return rccl_fail(nullptr, api, "ncclCommInitRank", r);
    fxc_comm* c = new (std::nothrow) fxc_comm();
    if (!c) {
        (void)api->comm_destroy(comm);
        return fail(nullptr, FXC_ERR_NOMEM, "host allocation failed");
    }
    c->comm = comm;
    c->device = device;
    c->rank = rank;
    c->world_size = world_size;
    *rccl_comm_out = c;
    return FXC_OK;
}

int fxc_comm_destroy(void* rccl_comm) {
    if (!rccl_comm) return FXC_OK;
    fxc_comm* c = static_cast<fxc_comm*>(rccl_comm);
    if (c->magic != fxc_comm::kMagic) return fail(nullptr, FXC_ERR_ARG, "not a communicator made by fxc_comm_create");
    RcclApi* api = rccl_api();
    if (!api->handle) return fail(nullptr, FXC_ERR_COMM, "%s", api->error.c_str());
    DeviceGuard device_guard__(c->device);
    const ncclResult_t r = api->comm_destroy(c->comm);
    c->magic = 0;
    delete c;
    if (r != ncclSuccess) return rccl_fail(nullptr, api, "ncclCommDestroy", r);
    return FXC_OK;
}

int fxc_rccl_version(int* version, char* path_out, int path_bytes) {
    if (!version) return fail(nullptr, FXC_ERR_ARG, "version is NULL");
    *version = 0;
    if (path_out && path_bytes > 0) path_out[0] = 0;
    RcclApi* api = rccl_api();
    if (!api->handle) return fail(nullptr, FXC_ERR_COMM, "%s", api->error.c_str());
    if (api->get_version) {
        const ncclResult_t r = api->get_version(version);
        if (r != ncclSuccess) return rccl_fail(nullptr, api, "ncclGetVersion", r);
    }
    if (path_out && path_bytes > 0) std::snprintf(path_out, (size_t)path_bytes, "%s", api->path.c_str());
    return FXC_OK;
}

int fxc_comm_info(void* rccl_comm, fxc_comm_desc* info) {
    if (!rccl_comm || !info) return fail(nullptr, FXC_ERR_ARG, "NULL argument");
    fxc_comm* c = static_cast<fxc_comm*>(rccl_comm);
    if (c->magic != fxc_comm::kMagic) return fail(nullptr, FXC_ERR_ARG, "not a communicator made by fxc_comm_create");
    RcclApi* api = rccl_api();
    if (!api->handle) return fail(nullptr, FXC_ERR_COMM, "%s", api->error.c_str());
    std::memset(info, 0, sizeof *info);
    info->ranks_seen = info->rank_seen = info->device_seen = info->async_error = -1;   // -1: this RCCL has no such query
    info->world_given = c->world_size;
    info->rank_given = c->rank;
    info->device_given = c->device;
    info->reduces = c->reduces;
    // asked of the live ncclComm_t, not echoed from the arguments of fxc_comm_create
    ncclResult_t r = ncclSuccess;
    int v = 0;
    if (api->comm_count) {
        if ((r = api->comm_count(c->comm, &v)) != ncclSuccess) return rccl_fail(nullptr, api, "ncclCommCount", r);
        info->ranks_seen = v;
    }
    if (api->comm_user_rank) {
        if ((r = api->comm_user_rank(c->comm, &v)) != ncclSuccess) return rccl_fail(nullptr, api, "ncclCommUserRank", r);
        info->rank_seen = v;
    }
    if (api->comm_cu_device) {
        if ((r = api->comm_cu_device(c->comm, &v)) != ncclSuccess) return rccl_fail(nullptr, api, "ncclCommCuDevice", r);
        info->device_seen = v;
    }
    if (api->get_version && api->get_version(&v) == ncclSuccess) info->rccl_version = v;
    if (api->comm_async_error) {
        ncclResult_t async = ncclSuccess;
        if (api->comm_async_error(c->comm, &async) == ncclSuccess) info->async_error = (int)async;
    }
    return FXC_OK;
}

int fxc_comm_probe(void* rccl_comm, int64_t* ranks_summed) {
    if (!rccl_comm || !ranks_summed) return fail(nullptr, FXC_ERR_ARG, "NULL argument");
    *ranks_summed = 0;
    fxc_comm* c = static_cast<fxc_comm*>(rccl_comm);
    if (c->magic != fxc_comm::kMagic) return fail(nullptr, FXC_ERR_ARG, "not a communicator made by fxc_comm_create");
    RcclApi* api = rccl_api();
    if (!api->handle) return fail(nullptr, FXC_ERR_COMM, "%s", api->error.c_str());
    FXC_DEVICE(nullptr, c->device);
    // every rank puts in 1.0 (and its rank + 1 in a second slot): what comes back was added up by RCCL itself
    DevBuf<double> d;
    Stream s;
    FXC_HIP(nullptr, d.alloc(2));
    int rc = FXC_OK;
    double h[2] = {1.0, (double)(c->rank + 1)};
    hipError_t e = s.create(hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMemcpyAsync(d, h, sizeof h, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        const ncclResult_t r = api->all_reduce(d, d, 2, ncclFloat64, ncclSum, c->comm, s);
        if (r != ncclSuccess) rc = rccl_fail(nullptr, api, "ncclAllReduce", r);
    }
    if (e == hipSuccess && rc == FXC_OK) e = hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && rc == FXC_OK) e = hipStreamSynchronize(s);
    if (rc) return rc;
    if (e != hipSuccess) return fail(nullptr, FXC_ERR_HIP, "fxc_comm_probe: %s", hipGetErrorString(e));
    const double n = h[0];
    if (h[1] != n * (n + 1) / 2) return fail(nullptr, FXC_ERR_COMM, "fxc_comm_probe: %g ranks answered but their ranks sum to %g", n, h[1]);
    *ranks_summed = (int64_t)n;
    return FXC_OK;
}

int fxc_reduce(fxc_plan* p, void* rccl_comm, int root) {
    if (!p) return fail(p, FXC_ERR_ARG, "NULL plan");
    fxc_comm* c = static_cast<fxc_comm*>(rccl_comm);
    if (c) {
        // checked before anything is queued: a collective on the wrong device or with a root no rank has would leave
        // the other ranks waiting in theirs
        if (c->magic != fxc_comm::kMagic) return fail(p, FXC_ERR_ARG, "not a communicator made by fxc_comm_create");
        if (c->device != p->device)
            return fail(p, FXC_ERR_ARG, "the communicator was made on device %d, the plan is on device %d", c->device, p->device);
        if (root >= c->world_size) return fail(p, FXC_ERR_ARG, "root %d outside the communicator's world of %d", root, c->world_size);
    }
    FXC_DEVICE(p, p->device);
    int rc = fxc_acc_export(p, p->d_sums);
    if (rc) return rc;
    p->sums_valid = true;
    if (!c) return FXC_OK;                  // single rank: the exported sums are the reduced sums
    RcclApi* api = rccl_api();
    if (!api->handle) return fail(p, FXC_ERR_COMM, "%s", api->error.c_str());
    // raw float64 sums + the spectra count, in place, ordered on the plan's stream behind the export
    const size_t count = 2 * ((size_t)p->n_prod * p->nchan + 1);
    const ncclResult_t r = root < 0 ? api->all_reduce(p->d_sums, p->d_sums, count, ncclFloat64, ncclSum, c->comm, p->stream)
                                    : api->reduce(p->d_sums, p->d_sums, count, ncclFloat64, ncclSum, root, c->comm, p->stream);
    if (r != ncclSuccess) return rccl_fail(p, api, root < 0 ? "ncclAllReduce" : "ncclReduce", r);
    ++c->reduces;
    return FXC_OK;
}

int fxc_sync(fxc_plan* p) {
    if (!p) return fail(p, FXC_ERR_ARG, "NULL plan");
    FXC_DEVICE(p, p->device);
    const int rf = flush_pending(p);        // the fold of the last fx_accumulate pass belongs to "everything queued"
    if (rf) return rf;
    FXC_HIP(p, hipStreamSynchronize(p->stream));
    return FXC_OK;
}

int fxc_channelize(fxc_plan* p, const void* x, void* out, int64_t n_streams, int mem_kind) {
    if (!p) return fail(p, FXC_ERR_ARG, "NULL plan");
    if (n_streams < 0) return fail(p, FXC_ERR_ARG, "n_streams < 0");
    if (n_streams == 0) return FXC_OK;
    if (!x || !out) return fail(p, FXC_ERR_ARG, "NULL buffer");
    FXC_DEVICE(p, p->device);
    if (mem_kind == FXC_MEM_DEVICE)
        return run_channelize(p, static_cast<const cf*>(x), static_cast<cf*>(out), n_streams);
    if (const int rc = bad_mem_kind(p, mem_kind)) return rc;
    const size_t xb = (size_t)n_streams * p->num_samp * sizeof(cf);
    const size_t ob = (size_t)n_streams * p->n_pts * p->nchan * sizeof(cf);
    return with_host_staging(p, x, xb, out, ob, [&](const cf* dx, void* dout) {
        return run_channelize(p, dx, static_cast<cf*>(dout), n_streams);
    });
}

int fxc_fx_accumulate(fxc_plan* p, const void* x, int64_t n_chunks, int mem_kind) {
    return fx_call(p, {FXC_IQ_C64, false, false, FXC_MODE_SPECTRUM, 1.0}, x, nullptr, n_chunks, mem_kind);
}

int fxc_fx_rows(fxc_plan* p, const void* x, void* out, int64_t n_chunks, int mem_kind, int mode, double bandwidth) {
    return fx_call(p, {FXC_IQ_C64, false, true, mode, bandwidth}, x, out, n_chunks, mem_kind);
}

int fxc_acc_reset(fxc_plan* p) {
    if (!p) return fail(p, FXC_ERR_ARG, "NULL plan");
    FXC_DEVICE(p, p->device);
    p->pend.valid = false;                  // rows not folded yet are simply dropped
    FXC_HIP(p, hipMemsetAsync(p->d_acc, 0, (size_t)p->n_prod * p->nchan * sizeof(cd), p->stream));
    p->spectra_count = 0.0;
    return FXC_OK;
}

int fxc_acc_export(fxc_plan* p, void* sums_dev) {
    if (!p || !sums_dev) return fail(p, FXC_ERR_ARG, "NULL argument");
    FXC_DEVICE(p, p->device);
    const FoldFinish fin = {static_cast<cd*>(sums_dev), nullptr, nullptr, p->spectra_count, 0};
    return flush_pending(p, &fin);
}

int fxc_finalize_async(fxc_plan* p, int mode, double bandwidth, int reset) {
    if (!p) return fail(p, FXC_ERR_ARG, "NULL plan");
    FXC_DEVICE(p, p->device);
    return finalize_enqueue(p, nullptr, mode, bandwidth, reset);
}

int fxc_finalize_async_to(fxc_plan* p, void* out_host, int mode, double bandwidth, int reset) {
    if (!p || !out_host) return fail(p, FXC_ERR_ARG, "NULL argument");
    FXC_DEVICE(p, p->device);
    return finalize_enqueue(p, nullptr, mode, bandwidth, reset, out_host);
}

int fxc_finalize_sums_async(fxc_plan* p, const void* sums_dev, int mode, double bandwidth) {
    if (!p) return fail(p, FXC_ERR_ARG, "NULL plan");
    if (!sums_dev) {                         // what fxc_reduce left in the plan
        if (!p->sums_valid) return fail(p, FXC_ERR_STATE, "no reduced sums in the plan: call fxc_reduce first");
        sums_dev = p->d_sums;
    }
    FXC_DEVICE(p, p->device);
    return finalize_enqueue(p, static_cast<const cd*>(sums_dev), mode, bandwidth, 0);
}

int fxc_finalize_wait(fxc_plan* p, void* out_host) {
    if (!p) return fail(p, FXC_ERR_ARG, "NULL plan");
    if (p->res_head == p->res_tail) return fail(p, FXC_ERR_STATE, "no finalize result outstanding");
    const int slot = (int)(p->res_tail % fxc_plan::kResSlots);
    void* const dst = p->res_dst[slot];       // fxc_finalize_async_to: the buffer named when the result was queued
    if (dst ? (out_host && out_host != dst) : !out_host)
        return fail(p, FXC_ERR_ARG, dst ? "this result was queued with fxc_finalize_async_to: pass that buffer or NULL" : "out_host is NULL");
    FXC_DEVICE(p, p->device);
    FXC_HIP(p, hipEventSynchronize(p->ev_res[slot]));
    if (!p->res_user[slot]) std::memcpy(dst ? dst : out_host, p->h_res[slot], p->res_bytes[slot]);
    p->res_tail += 1;
    return FXC_OK;
}

int fxc_finalize_pending(const fxc_plan* p) { return p ? (int)(p->res_head - p->res_tail) : 0; }

int fxc_finalize_sums(fxc_plan* p, const void* sums_dev, void* out_host, int mode, double bandwidth) {
    if (!p || !out_host) return fail(p, FXC_ERR_ARG, "NULL argument");
    if (p->res_head != p->res_tail) return fail(p, FXC_ERR_STATE, "asynchronous finalize results outstanding");
    const int rc = fxc_finalize_sums_async(p, sums_dev, mode, bandwidth);
    if (rc) return rc;
    return fxc_finalize_wait(p, out_host);
}

int fxc_finalize(fxc_plan* p, void* out_host, int mode, double bandwidth, int reset) {
    if (!p || !out_host) return fail(p, FXC_ERR_ARG, "NULL argument");
    if (p->res_head != p->res_tail) return fail(p, FXC_ERR_STATE, "asynchronous finalize results outstanding");
    const int rc = fxc_finalize_async(p, mode, bandwidth, reset);
    if (rc) return rc;
    return fxc_finalize_wait(p, out_host);
}

static int conditioning_common(fxc_plan* p, int64_t n_streams, const void* x, void* out) {
    if (!p) return fail(p, FXC_ERR_ARG, "NULL plan");
    if (n_streams < 0) return fail(p, FXC_ERR_ARG, "n_streams < 0");
    if (n_streams > 65535) return fail(p, FXC_ERR_ARG, "at most 65535 streams per call");
    if (n_streams > 0 && (!x || !out)) return fail(p, FXC_ERR_ARG, "NULL buffer");
    return FXC_OK;
}

int fxc_remove_dc(fxc_plan* p, const void* x_dev, void* out_dev, int64_t n_streams) {
    int rc = conditioning_common(p, n_streams, x_dev, out_dev);
    if (rc || n_streams == 0) return rc;
    FXC_DEVICE(p, p->device);
    const int n_slices = 32;
    rc = ensure_ws(p, n_streams * n_slices * 2 * (int64_t)sizeof(double));
    if (rc) return rc;
    launch_remove_dc_c64(p, static_cast<const cf*>(x_dev), static_cast<cf*>(out_dev), static_cast<double*>(p->d_ws.get()), n_streams, n_slices);
    FXC_HIP(p, hipGetLastError());
    return FXC_OK;
}

int fxc_convert_u8(fxc_plan* p, const void* iq_u8_dev, void* out_dev, int64_t n_streams, int remove_dc) {
    int rc = conditioning_common(p, n_streams, iq_u8_dev, out_dev);
    if (rc || n_streams == 0) return rc;
    FXC_DEVICE(p, p->device);
    const int n_slices = 32;
    rc = ensure_ws(p, n_streams * n_slices * 2 * (int64_t)sizeof(double));
    if (rc) return rc;
    double* part = static_cast<double*>(p->d_ws.get());
    if (remove_dc) launch_dc_sum_u8(p, static_cast<const unsigned char*>(iq_u8_dev), part, n_streams, n_slices);
    launch_convert_u8(p, static_cast<const unsigned char*>(iq_u8_dev), static_cast<cf*>(out_dev), part, n_slices, n_streams, remove_dc != 0);
    FXC_HIP(p, hipGetLastError());
    return FXC_OK;
}

int fxc_fx_rows_iq(fxc_plan* p, const void* x, void* out, int64_t n_chunks, int mem_kind, int mode, double bandwidth,
                   int iq_format, int remove_dc) {
    return fx_call(p, {iq_format, remove_dc != 0, true, mode, bandwidth}, x, out, n_chunks, mem_kind);
}

int fxc_fx_accumulate_iq(fxc_plan* p, const void* x, int64_t n_chunks, int mem_kind, int iq_format, int remove_dc) {
    return fx_call(p, {iq_format, remove_dc != 0, false, FXC_MODE_SPECTRUM, 1.0}, x, nullptr, n_chunks, mem_kind);
}

int fxc_host_alloc(void** out, int64_t bytes) {
    if (!out) return fail(nullptr, FXC_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (bytes <= 0) return fail(nullptr, FXC_ERR_ARG, "bytes must be > 0");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(nullptr, FXC_ERR_NODEVICE, "no HIP device available (pinned memory needs the HIP runtime)");
    void* h = nullptr;
    const hipError_t e = hipHostMalloc(&h, (size_t)bytes, hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent);
    if (e != hipSuccess) return fail(nullptr, FXC_ERR_NOMEM, "hipHostMalloc of %lld bytes failed: %s", (long long)bytes, hipGetErrorString(e));
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess || !d) {
        (void)hipHostFree(h);
        return fail(nullptr, FXC_ERR_HIP, "hipHostGetDevicePointer failed for a fresh pinned block");
    }
    {
        std::lock_guard<std::mutex> lock(g_pinned_mutex);
        g_pinned.push_back({static_cast<char*>(h), static_cast<char*>(d), (size_t)bytes});
    }
    *out = h;
    return FXC_OK;
}

int fxc_host_free(void* ptr) {
    if (!ptr) return FXC_OK;
    {
        std::lock_guard<std::mutex> lock(g_pinned_mutex);
        size_t k = 0;
        while (k < g_pinned.size() && g_pinned[k].host != ptr) ++k;
        if (k == g_pinned.size()) return fail(nullptr, FXC_ERR_ARG, "not a pointer fxc_host_alloc returned");
        g_pinned.erase(g_pinned.begin() + (long)k);
    }
    // hipHostFree waits for the device: nothing queued can still touch the block when it goes
    const hipError_t e = hipHostFree(ptr);
    if (e != hipSuccess) return fail(nullptr, FXC_ERR_HIP, "hipHostFree failed: %s", hipGetErrorString(e));
    return FXC_OK;
}

int fxc_fx_rows_u8(fxc_plan* p, const void* iq_u8, void* out, int64_t n_chunks, int mem_kind, int mode, double bandwidth,
                   int remove_dc) {
    return fx_call(p, {FXC_IQ_U8, remove_dc != 0, true, mode, bandwidth}, iq_u8, out, n_chunks, mem_kind);
}

int fxc_fx_accumulate_u8(fxc_plan* p, const void* iq_u8, int64_t n_chunks, int mem_kind, int remove_dc) {
    return fx_call(p, {FXC_IQ_U8, remove_dc != 0, false, FXC_MODE_SPECTRUM, 1.0}, iq_u8, nullptr, n_chunks, mem_kind);
}

int fxc_estimate_delay(fxc_plan* p, const void* iq0, const void* iq1, int64_t n, int mem_kind, double rate,
                       double* delay_s) {
    if (!p || !iq0 || !iq1 || !delay_s) return fail(p, FXC_ERR_ARG, "NULL argument");
    const cf* streams[2] = {static_cast<const cf*>(iq0), static_cast<const cf*>(iq1)};
    double d[2];
    const int rc = estimate_delays_batch(p, streams, 2, 0, n, mem_kind, rate, d);
    if (rc == FXC_OK) *delay_s = d[1];
    return rc;
}

int fxc_estimate_delays(fxc_plan* p, const void* x, int64_t n, int mem_kind, double rate, int ref, double* delays_s) {
    if (!p || !x || !delays_s) return fail(p, FXC_ERR_ARG, "NULL argument");
    if (p->n_ant < 2) return fail(p, FXC_ERR_ARG, "delays need 2 or more antennas, the plan has %d", p->n_ant);
    if (ref < 0 || ref >= p->n_ant) return fail(p, FXC_ERR_ARG, "ref=%d outside [0, %d)", ref, p->n_ant);
    if (n < 2 || n > (1ll << 28)) return fail(p, FXC_ERR_ARG, "n=%lld out of range", (long long)n);
    std::vector<const cf*> streams((size_t)p->n_ant);
    for (int a = 0; a < p->n_ant; ++a) streams[(size_t)a] = static_cast<const cf*>(x) + (int64_t)a * n;
    return estimate_delays_batch(p, streams.data(), p->n_ant, ref, n, mem_kind, rate, delays_s);
}

int fxc_fringe_fit(fxc_plan* p, const void* rows, int64_t n_chunks, int mem_kind, double bandwidth, double frequency, int ref,
                   int pad, double* delay_s, double* rate_s_per_chunk, double* snr) {
    int lk_log, lt_log;
    if (const int rc = check_fringe_fit(p, rows, n_chunks, mem_kind, bandwidth, frequency, ref, pad, FXC_FRINGE_REF, 0.0, delay_s,
                                        rate_s_per_chunk, &lk_log, &lt_log))
        return rc;
    return fringe_fit_run(p, static_cast<const cf*>(rows), nullptr, n_chunks, mem_kind, bandwidth, frequency, ref, lk_log, lt_log, false,
                          FXC_FRINGE_REF, 0.0, delay_s, rate_s_per_chunk, snr, nullptr);
}

int fxc_fringe_fit_weighted(fxc_plan* p, const void* rows, const void* weights, int64_t n_chunks, int mem_kind, double bandwidth,
                            double frequency, int ref, int pad, int baselines, double min_snr, double* delay_s, double* rate_s_per_chunk,
                            double* snr, double* base_out) {
    int lk_log, lt_log;
    if (const int rc = check_fringe_fit(p, rows, n_chunks, mem_kind, bandwidth, frequency, ref, pad, baselines, min_snr, delay_s,
                                        rate_s_per_chunk, &lk_log, &lt_log))
        return rc;
    return fringe_fit_run(p, static_cast<const cf*>(rows), static_cast<const float*>(weights), n_chunks, mem_kind, bandwidth, frequency, ref,
                          lk_log, lt_log, true, baselines, min_snr, delay_s, rate_s_per_chunk, snr, base_out);
}

int fxc_flag_rows(fxc_plan* p, const void* rows, const void* prior, int64_t n_chunks, int mem_kind, int64_t window, float time_threshold,
                  float freq_threshold, int half_width, int iters, void* weights, int64_t* counts) {
    if (!p || !rows || !weights) return fail(p, FXC_ERR_ARG, "NULL argument");
    if (n_chunks < 1) return fail(p, FXC_ERR_ARG, "n_chunks=%lld: the detector needs 1 or more chunks", (long long)n_chunks);
    if (window < 0) return fail(p, FXC_ERR_ARG, "window=%lld is negative", (long long)window);
    if (!std::isfinite(time_threshold) || !(time_threshold > 0.f)) return fail(p, FXC_ERR_ARG, "time_threshold must be finite and > 0");
    if (!std::isfinite(freq_threshold) || !(freq_threshold > 0.f)) return fail(p, FXC_ERR_ARG, "freq_threshold must be finite and > 0");
    if (half_width < 0) return fail(p, FXC_ERR_ARG, "half_width=%d is negative", half_width);
    if (iters < 1 || iters > 8) return fail(p, FXC_ERR_ARG, "iters=%d outside 1 .. 8", iters);
    if (const int rc = bad_mem_kind(p, mem_kind)) return rc;
    if (p->n_base < 1) return fail(p, FXC_ERR_ARG, "the detector needs 2 or more antennas, the plan has %d", p->n_ant);
    if (window == 0 || window > n_chunks) window = n_chunks;
    if (window > kFlagMaxChunks)
        return fail(p, FXC_ERR_UNSUPPORTED, "%lld chunks in a window: a column lives in LDS, 1024 chunks at most", (long long)window);
    return flag_rows_batch(p, static_cast<const cf*>(rows), static_cast<const float*>(prior), n_chunks, mem_kind, window, time_threshold,
                           freq_threshold, std::min(half_width, p->nchan), iters, static_cast<float*>(weights), counts);
}

int fxc_average_rows(fxc_plan* p, const void* rows, const void* weights, int64_t n_chunks, int mem_kind, int64_t time_bin, int freq_bin,
                     void* out_rows, void* out_weights) {
    if (!p || !rows || !out_rows) return fail(p, FXC_ERR_ARG, "NULL argument");
    if (n_chunks < 1) return fail(p, FXC_ERR_ARG, "n_chunks=%lld: the averager needs 1 or more chunks", (long long)n_chunks);
    if (time_bin < 0) return fail(p, FXC_ERR_ARG, "time_bin=%lld is negative", (long long)time_bin);
    if (freq_bin < 1) return fail(p, FXC_ERR_ARG, "freq_bin=%d is not 1 or more", freq_bin);
    if (const int rc = bad_mem_kind(p, mem_kind)) return rc;
    if (p->n_base < 1) return fail(p, FXC_ERR_ARG, "the averager needs 2 or more antennas, the plan has %d", p->n_ant);
    if (freq_bin > kAverageMaxBin)
        return fail(p, FXC_ERR_UNSUPPORTED, "freq_bin=%d: a workgroup's tile holds a whole output bin, 256 input bins at most", freq_bin);
    if (time_bin == 0 || time_bin > n_chunks) time_bin = n_chunks;
    return average_rows_batch(p, static_cast<const cf*>(rows), static_cast<const float*>(weights), n_chunks, mem_kind, time_bin, freq_bin,
                              static_cast<cf*>(out_rows), static_cast<float*>(out_weights));
}

int fxc_dedisperse(fxc_plan* p, const void* power, int64_t n_chunks, int64_t n_series, int64_t n_tbin, int mem_kind, const int32_t* shifts,
                   int n_dm, const float* chan_weights, void* out, int64_t* info_out) {
    if (!p || !power || !shifts || !out) return fail(p, FXC_ERR_ARG, "NULL argument");
    if (n_chunks < 1 || n_series < 1 || n_tbin < 1)
        return fail(p, FXC_ERR_ARG, "n_chunks=%lld, n_series=%lld, n_tbin=%lld: each must be 1 or more", (long long)n_chunks, (long long)n_series,
                    (long long)n_tbin);
    if (n_dm < 1) return fail(p, FXC_ERR_ARG, "n_dm=%d is not 1 or more", n_dm);
    if (const int rc = bad_mem_kind(p, mem_kind)) return rc;
    DedTable table;
    if (const int rc = build_ded_table(p, shifts, n_dm, chan_weights, &table)) return rc;
    if (n_chunks >= (1ll << 31) || n_tbin >= (1ll << 31) || n_chunks * n_tbin >= (1ll << 31))
        return fail(p, FXC_ERR_UNSUPPORTED, "n_t = %lld chunks of %lld bins: the time axis is addressed in 31 bits", (long long)n_chunks,
                    (long long)n_tbin);
    if (table.s_max >= n_chunks * n_tbin)
        return fail(p, FXC_ERR_ARG, "the largest shift %lld leaves no output: n_t is %lld", (long long)table.s_max, (long long)(n_chunks * n_tbin));
    return dedisperse_batch(p, static_cast<const float*>(power), n_chunks, n_series, n_tbin, mem_kind, table, static_cast<float*>(out), info_out);
}

int fxc_boxcar_search(fxc_plan* p, const void* series, int64_t n_rows, int64_t n_t, int mem_kind, int j_lo, int j_hi, int64_t block,
                      double clip, int clip_iters, void* snr_out, void* width_out, void* time_out, double* stats_out) {
    if (!p || !series || !snr_out || !width_out || !time_out) return fail(p, FXC_ERR_ARG, "NULL argument");
    if (n_rows < 1 || n_t < 1 || block < 1)
        return fail(p, FXC_ERR_ARG, "n_rows=%lld, n_t=%lld, block=%lld: each must be 1 or more", (long long)n_rows, (long long)n_t,
                    (long long)block);
    if (j_lo < 0 || j_hi > kBoxMaxJ || j_lo > j_hi) return fail(p, FXC_ERR_ARG, "widths 2^%d .. 2^%d are not within 2^0 .. 2^%d", j_lo, j_hi, kBoxMaxJ);
    if ((1ll << j_lo) > n_t) return fail(p, FXC_ERR_ARG, "the narrowest width 2^%d leaves no start: n_t is %lld", j_lo, (long long)n_t);
    if (!(clip >= 0.0)) return fail(p, FXC_ERR_ARG, "clip must be 0 or more");
    if (clip_iters < 0 || clip_iters > 4) return fail(p, FXC_ERR_ARG, "clip_iters=%d outside 0 .. 4", clip_iters);
    if (const int rc = bad_mem_kind(p, mem_kind)) return rc;
    if (n_t >= (1ll << 31)) return fail(p, FXC_ERR_UNSUPPORTED, "n_t = %lld: the time axis is addressed in 31 bits", (long long)n_t);
    return boxcar_batch(p, static_cast<const float*>(series), n_rows, n_t, mem_kind, j_lo, j_hi, block, clip, clip_iters,
                        static_cast<float*>(snr_out), static_cast<int*>(width_out), static_cast<int*>(time_out), stats_out);
}

namespace {

// fxc_beamform (no mask, modes POWER and VOLTAGE, align 0) and fxc_beamform_ex: the argument checks in the order that gives each
// call its code and message, then the driver on the device or through the host staging; a failed call puts the track's counter back
int beamform_call(fxc_plan* p, const void* x, const void* weights, int n_beam, const void* mask, int64_t mask_tint, void* out,
                  int64_t n_chunks, int mem_kind, int mode, int n_modes, int64_t tint, int align) {
    if (!p) return fail(p, FXC_ERR_ARG, "NULL plan");
    if (n_chunks < 0) return fail(p, FXC_ERR_ARG, "n_chunks < 0");
    if (n_beam < 1) return fail(p, FXC_ERR_ARG, "n_beam=%d is not 1 or more", n_beam);
    if (mode < 0 || mode >= n_modes) return fail(p, FXC_ERR_ARG, "bad beam mode %d", mode);
    if (const int rc = bad_mem_kind(p, mem_kind)) return rc;
    if (tint < 0 || tint > p->n_pts) return fail(p, FXC_ERR_ARG, "tint=%lld is not within 0 .. %lld frames", (long long)tint, (long long)p->n_pts);
    if (mask_tint < 0 || mask_tint > p->n_pts)
        return fail(p, FXC_ERR_ARG, "mask_tint=%lld is not within 0 .. %lld frames", (long long)mask_tint, (long long)p->n_pts);
    if (align != 0 && align != 1) return fail(p, FXC_ERR_ARG, "align=%d is neither 0 nor 1", align);
    if (n_beam > kBeamMax) return fail(p, FXC_ERR_UNSUPPORTED, "n_beam=%d: a call forms %d beams at most", n_beam, kBeamMax);
    if (n_chunks == 0 || p->n_pts == 0) return FXC_OK;
    if (!x || !weights || !out) return fail(p, FXC_ERR_ARG, "NULL buffer");
    if (p->track && p->live_pipes) return fail(p, FXC_ERR_STATE, "an fxc_pipe uses the plan");
    if (aligning(p)) {
        if (!align)
            return fail(p, FXC_ERR_UNSUPPORTED, "the plan applies whole-sample delays (%s) and the beamformer's passes are not aligned: beams of "
                        "unaligned samples would lose amplitude silently.  Clear the shifts or use a plain delay track",
                        p->shifted ? "fxc_set_sample_delays" : "fxc_set_delay_track_aligned");
        if (p->live_pipes) return fail(p, FXC_ERR_STATE, "an fxc_pipe uses the plan");      // (its passes are aligned into the same buffer)
    }
    FXC_DEVICE(p, p->device);
    const int64_t t0 = p->track_t;
    int rc;
    if (mem_kind == FXC_MEM_DEVICE) {
        rc = beamform_dev(p, static_cast<const cf*>(x), static_cast<const cf*>(weights), false, n_beam, static_cast<const float*>(mask),
                          mask_tint, out, n_chunks, mode, tint, align != 0);
    } else {
        const int64_t n_tbin = time_bins(p, tint).n_bin;
        const size_t ob = mode == FXC_BEAM_VOLTAGE ? (size_t)n_chunks * n_beam * p->n_pts * p->nchan * sizeof(cf)
                                                   : (size_t)n_chunks * n_beam * n_tbin * p->nchan * sizeof(float);
        rc = with_host_staging(p, x, (size_t)n_chunks * p->n_ant * p->num_samp * sizeof(cf), out, ob, [&](const cf* dx, void* dout) {
            return beamform_dev(p, dx, static_cast<const cf*>(weights), true, n_beam, static_cast<const float*>(mask), mask_tint, dout,
                                n_chunks, mode, tint, align != 0);
        });
    }
    if (rc) p->track_t = t0;
    return rc;
}

}  // namespace

int fxc_beamform(fxc_plan* p, const void* x, const void* weights, int n_beam, void* out, int64_t n_chunks, int mem_kind, int mode,
                 int64_t tint) {
    return beamform_call(p, x, weights, n_beam, nullptr, 0, out, n_chunks, mem_kind, mode, 2, tint, 0);
}

int fxc_beamform_ex(fxc_plan* p, const void* x, const void* weights, int n_beam, const void* mask, int64_t mask_tint, void* out,
                    int64_t n_chunks, int mem_kind, int mode, int64_t tint, int align) {
    return beamform_call(p, x, weights, n_beam, mask, mask_tint, out, n_chunks, mem_kind, mode, 3, tint, align);
}

int fxc_kurtosis_antenna_mask(fxc_plan* p, const void* sk, int64_t n_chunks, int64_t tint, double lo, double hi, double lo_last,
                              double hi_last, void* mask_out, int mem_kind) {
    bool done;
    if (const int rc = check_kurtosis(p, n_chunks, mem_kind, tint, &done)) return rc;
    if (std::isnan(lo) || std::isnan(hi) || lo > hi || std::isnan(lo_last) || std::isnan(hi_last) || lo_last > hi_last)
        return fail(p, FXC_ERR_ARG, "the thresholds must be numbers with lo <= hi and lo_last <= hi_last");
    if (done) return FXC_OK;
    if (!sk || !mask_out) return fail(p, FXC_ERR_ARG, "NULL buffer");
    FXC_DEVICE(p, p->device);
    if (mem_kind == FXC_MEM_DEVICE)
        return kurtosis_mask_dev(p, static_cast<const float*>(sk), static_cast<float*>(mask_out), n_chunks, tint, lo, hi, lo_last, hi_last);
    const int64_t n_tbin = time_bins(p, tint).n_bin;
    const size_t bytes = (size_t)n_chunks * p->n_ant * n_tbin * p->nchan * sizeof(float);
    return with_host_staging(p, sk, bytes, mask_out, bytes, [&](const cf* dsk, void* dout) {
        return kurtosis_mask_dev(p, reinterpret_cast<const float*>(dsk), static_cast<float*>(dout), n_chunks, tint, lo, hi, lo_last, hi_last);
    });
}

int fxc_kurtosis(fxc_plan* p, const void* x, void* sk_out, void* power_out, int64_t n_chunks, int mem_kind, int64_t tint) {
    bool done;
    if (const int rc = check_kurtosis(p, n_chunks, mem_kind, tint, &done)) return rc;
    if (done) return FXC_OK;
    if (!x || !sk_out) return fail(p, FXC_ERR_ARG, "NULL buffer");
    FXC_DEVICE(p, p->device);
    if (mem_kind == FXC_MEM_DEVICE)
        return kurtosis_dev(p, static_cast<const cf*>(x), static_cast<float*>(sk_out), static_cast<float*>(power_out), n_chunks, tint);
    // host memory: sk and power leave through one staging block, sk first
    const int64_t n_tbin = time_bins(p, tint).n_bin;
    const size_t elems = (size_t)n_chunks * p->n_ant * n_tbin * p->nchan;
    std::vector<float> both;
    void* out = sk_out;
    if (power_out) {
        both.resize(2 * elems);
        out = both.data();
    }
    const int rc = with_host_staging(p, x, (size_t)n_chunks * p->n_ant * p->num_samp * sizeof(cf), out, (power_out ? 2 : 1) * elems * sizeof(float),
                                     [&](const cf* dx, void* dout) {
                                         float* d = static_cast<float*>(dout);
                                         return kurtosis_dev(p, dx, d, power_out ? d + elems : nullptr, n_chunks, tint);
                                     });
    if (rc) return rc;
    if (power_out) {
        std::memcpy(sk_out, both.data(), elems * sizeof(float));
        std::memcpy(power_out, both.data() + elems, elems * sizeof(float));
    }
    return FXC_OK;
}

int fxc_kurtosis_weights(fxc_plan* p, const void* sk, int64_t n_chunks, int64_t tint, double lo, double hi, void* weights_out, int mem_kind) {
    bool done;
    if (const int rc = check_kurtosis(p, n_chunks, mem_kind, tint, &done)) return rc;
    if (!std::isfinite(lo) || !std::isfinite(hi) || lo > hi) return fail(p, FXC_ERR_ARG, "the thresholds must be finite with lo <= hi");
    if (done) return FXC_OK;
    if (!sk || !weights_out) return fail(p, FXC_ERR_ARG, "NULL buffer");
    FXC_DEVICE(p, p->device);
    if (mem_kind == FXC_MEM_DEVICE)
        return kurtosis_weights_dev(p, static_cast<const float*>(sk), static_cast<float*>(weights_out), n_chunks, tint, lo, hi);
    const int64_t n_tbin = time_bins(p, tint).n_bin;
    return with_host_staging(p, sk, (size_t)n_chunks * p->n_ant * n_tbin * p->nchan * sizeof(float), weights_out,
                             (size_t)n_chunks * p->n_base * p->nchan * sizeof(float), [&](const cf* dsk, void* dout) {
                                 return kurtosis_weights_dev(p, reinterpret_cast<const float*>(dsk), static_cast<float*>(dout), n_chunks, tint, lo, hi);
                             });
}

int fxc_solve_gains_weighted(fxc_plan* p, const void* rows, const void* weights, int64_t n_chunks, int mem_kind, const void* model,
                             int64_t n_model, int64_t interval, int ref, int iters, double* gains_re_im, double* step) {
    if (int rc = check_solve_gains(p, rows, n_chunks, mem_kind, model, n_model, &interval, ref, iters, gains_re_im)) return rc;
    return solve_gains_batch(p, true, static_cast<const cf*>(rows), static_cast<const float*>(weights), n_chunks, mem_kind,
                             static_cast<const cf*>(model), n_model, interval, ref, iters, gains_re_im, step);
}

int fxc_solve_gains(fxc_plan* p, const void* rows, int64_t n_chunks, int mem_kind, int64_t interval, int ref, int iters,
                    double* gains_re_im, double* step) {
    if (int rc = check_solve_gains(p, rows, n_chunks, mem_kind, nullptr, 0, &interval, ref, iters, gains_re_im)) return rc;
    return solve_gains_batch(p, false, static_cast<const cf*>(rows), nullptr, n_chunks, mem_kind, nullptr, 0, interval, ref, iters,
                             gains_re_im, step);
}

int fxc_pipe_destroy(fxc_pipe* q) {
    if (!q) return FXC_OK;
    return pipe_destroy(q);
}

int fxc_pipe_create(fxc_pipe** out, fxc_plan* p, int64_t chunks_per_batch, int depth, int mode, double bandwidth) {
    return fxc_pipe_create_iq(out, p, chunks_per_batch, depth, mode, bandwidth, FXC_IQ_C64, 0);
}

int fxc_pipe_create_u8(fxc_pipe** out, fxc_plan* p, int64_t chunks_per_batch, int depth, int mode, double bandwidth,
                       int remove_dc) {
    return fxc_pipe_create_iq(out, p, chunks_per_batch, depth, mode, bandwidth, FXC_IQ_U8, remove_dc);
}

int fxc_pipe_create_iq(fxc_pipe** out, fxc_plan* p, int64_t chunks_per_batch, int depth, int mode, double bandwidth, int fmt,
                       int remove_dc) {
    if (!out || !p) return fail(p, FXC_ERR_ARG, "NULL argument");
    *out = nullptr;
    if (chunks_per_batch < 1 || depth < 1 || depth > 16) return fail(p, FXC_ERR_ARG, "bad batch size or depth");
    if (const int rc = check_call(p, {fmt, remove_dc != 0, true, mode, bandwidth})) return rc;
    return pipe_create(out, p, chunks_per_batch, depth, mode, bandwidth, fmt, remove_dc);
}

int fxc_pipe_in_flight(const fxc_pipe* q) { return q ? (int)(q->pushed - q->popped) : 0; }

int fxc_pipe_acquire(fxc_pipe* q, void** in_host) {
    if (!q || !in_host) return fail(q ? q->plan : nullptr, FXC_ERR_ARG, "NULL argument");
    return pipe_acquire(q, in_host);
}

int fxc_pipe_submit(fxc_pipe* q) {
    if (!q) return fail(nullptr, FXC_ERR_ARG, "NULL pipe");
    return pipe_submit(q);
}

int fxc_pipe_push(fxc_pipe* q, const void* x_host) {
    if (!q || !x_host) return fail(q ? q->plan : nullptr, FXC_ERR_ARG, "NULL argument");
    return pipe_push(q, x_host);
}

int fxc_pipe_pop(fxc_pipe* q, void* out_host) {
    if (!q || !out_host) return fail(q ? q->plan : nullptr, FXC_ERR_ARG, "NULL argument");
    return pipe_pop(q, out_host);
}

int fxc_timer_start(fxc_plan* p) {
    if (!p) return fail(p, FXC_ERR_ARG, "NULL plan");
    FXC_DEVICE(p, p->device);
    FXC_HIP(p, hipEventRecord(p->ev_t0, p->stream));
    return FXC_OK;
}

int fxc_timer_stop(fxc_plan* p, double* elapsed_ms) {
    if (!p || !elapsed_ms) return fail(p, FXC_ERR_ARG, "NULL argument");
    FXC_DEVICE(p, p->device);
    FXC_HIP(p, hipEventRecord(p->ev_t1, p->stream));
    FXC_HIP(p, hipEventSynchronize(p->ev_t1));
    float ms = 0.f;
    FXC_HIP(p, hipEventElapsedTime(&ms, p->ev_t0, p->ev_t1));
    *elapsed_ms = ms;
    return FXC_OK;
}

int fxc_kernel_profiling(fxc_plan* p, int enable) {
    if (!p) return fail(p, FXC_ERR_ARG, "NULL plan");
    p->profiling = enable != 0;
    return FXC_OK;
}

int fxc_kernel_time(fxc_plan* p, double* total_ms, int64_t* launches, int reset) {
    if (!p || !total_ms || !launches) return fail(p, FXC_ERR_ARG, "NULL argument");
    FXC_DEVICE(p, p->device);
    int rc = drain_kernel_events(p);
    if (rc) return rc;
#if FXC_STAMPS
    if (p->stamp_grid > 0 && p->d_stamps) {
        const int nw = p->stamp_grid * 8;
        std::vector<unsigned long long> h((size_t)nw * kStampSegs);
        FXC_HIP(p, hipStreamSynchronize(p->stream));
        FXC_HIP(p, hipMemcpy(h.data(), p->d_stamps, h.size() * 8, hipMemcpyDeviceToHost));
        double sum[kStampSegs] = {0};
        double steps = 0;
        for (int w = 0; w < nw; ++w) {
            for (int k = 0; k < kStampSegs - 1; ++k) sum[k] += (double)h[(size_t)w * kStampSegs + k];
            steps += (double)h[(size_t)w * kStampSegs + kStampSegs - 1];
        }
        double tot = 0;
        for (int k = 0; k < kStampSegs - 1; ++k) tot += sum[k];
        fprintf(stderr, "[fxc stamps] cycles per step per wave (s_memtime ticks), total %.0f:", tot / steps);
        for (int k = 0; k < kStampSegs - 1; ++k) fprintf(stderr, " s%d=%.0f", k, sum[k] / steps);
        fprintf(stderr, "\n");
    }
#endif
    *total_ms = p->kernel_ms;
    *launches = p->kernel_launches;
    if (reset) {
        p->kernel_ms = 0.0;
        p->kernel_launches = 0;
    }
    return FXC_OK;
}

int fxc_synth_fill(int device, void* stream, void* x_dev, uint64_t seed, int64_t first_chunk, int64_t n_chunks,
                   int n_ant, int64_t num_samp, const int32_t* delays, const float* tone_re_im, int tone_period) {
    if (!x_dev || !delays || !tone_re_im) return fail(nullptr, FXC_ERR_ARG, "NULL argument");
    if (n_chunks < 0 || n_ant < 1 || num_samp < 1 || tone_period < 1) return fail(nullptr, FXC_ERR_ARG, "bad size");
    if (n_chunks == 0) return FXC_OK;
    const fxc_plan* p = nullptr;
    FXC_DEVICE(p, device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    float lut[256];
    for (int b = 0; b < 256; ++b) lut[b] = ((float)b - 127.5f) / 127.5f;
    DevBuf<int> d_delays;
    DevBuf<cf> d_tone;
    DevBuf<float> d_lut;
    FXC_HIP(p, d_delays.alloc((size_t)n_ant));
    FXC_HIP(p, d_tone.alloc((size_t)tone_period));
    FXC_HIP(p, d_lut.alloc(256));
    FXC_HIP(p, hipMemcpy(d_delays, delays, (size_t)n_ant * sizeof(int), hipMemcpyHostToDevice));
    FXC_HIP(p, hipMemcpy(d_tone, tone_re_im, (size_t)tone_period * sizeof(cf), hipMemcpyHostToDevice));
    FXC_HIP(p, hipMemcpy(d_lut, lut, sizeof lut, hipMemcpyHostToDevice));
    const int64_t total = n_chunks * n_ant * num_samp;
    int64_t grid = (total + 255) / 256;
    if (grid > 256 * 16) grid = 256 * 16;
    hipLaunchKernelGGL(synth_kernel, dim3((int)grid), dim3(256), 0, st, static_cast<cf*>(x_dev), seed, first_chunk,
                       n_chunks, n_ant, num_samp, d_delays.get(), d_tone.get(), tone_period, d_lut.get());
    hipError_t e = hipGetLastError();
    hipError_t e2 = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(nullptr, FXC_ERR_HIP, "synth launch failed: %s", hipGetErrorString(e));
    if (e2 != hipSuccess) return fail(nullptr, FXC_ERR_HIP, "synth sync failed: %s", hipGetErrorString(e2));
    return FXC_OK;
}

}  // extern "C"
