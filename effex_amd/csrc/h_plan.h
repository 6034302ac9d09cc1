// Part of libfxcorr's single translation unit: included by fxcorr.hip (not a stand-alone header).
#pragma once

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
namespace {

thread_local std::string g_lib_error;


// Pinned host allocations handed out by fxc_host_alloc (process-wide).  with_host_staging looks a caller's pointer up
// here: an output buffer inside one of them is written by the finishing kernel through `dev` (no copy back).
struct PinnedBlock {
    char* host;
    char* dev;       // the same memory as the devices see it
    size_t bytes;
};
std::mutex g_pinned_mutex;
std::vector<PinnedBlock> g_pinned;

// device address of [ptr, ptr + bytes) if it lies inside one fxc_host_alloc block, else nullptr
void* pinned_device_ptr(const void* ptr, size_t bytes) {
    const char* q = static_cast<const char*>(ptr);
    std::lock_guard<std::mutex> lock(g_pinned_mutex);
    for (const PinnedBlock& b : g_pinned)
        if (q >= b.host && q + bytes <= b.host + b.bytes) return b.dev + (q - b.host);
    return nullptr;
}

}  // namespace


// ------------------------------------------------------------------------------------------
// host-fed front end: double-buffered pinned staging, H2D / compute / D2H on three
// streams chained by events, so batch k+1 crosses PCIe while batch k is on the CUs.  Replaces the
// reference's per-chunk blocking copies (effex/effex.py:391-392, 508-509, 693).
// ------------------------------------------------------------------------------------------
struct fxc_pipe_slot {      // (h_own.h owners: a slot frees itself, memory first)
    Event ev_in, ev_compute, ev_out;
    PinnedBuf h_in, h_out;
    DevBuf<void> d_in, d_out;
    bool busy = false;
};

namespace {
struct SpecKernel;      // h_rtc.h
}

struct fxc_plan {
    // What the plan holds on the device is held by the owners of h_own.h: fxc_plan_destroy waits for the streams and deletes the
    // plan, nothing more.  Members die in the reverse of their order here, and the order that matters is: memory is freed, then
    // events are destroyed, then streams.  So the streams and the events stand here, ahead of every buffer (and the large-result
    // group keeps the same order inside itself); a new handle goes here, a new buffer anywhere below.
    Stream stream;                   // the caller's unless own_stream
    bool own_stream = false;
    static constexpr int kResSlots = 2;
    // results too large to be worth a kernel's time on PCIe (28 baselines: 1.8 MB, 35 us inside the finishing kernel):
    // the kernel writes device memory and a copy on a side stream carries it to the slot while the next F+X runs (made by the
    // first such finalize)
    BigResults<cd, kResSlots> big_res;
    Event ev_order;                  // orders the old stream's work before the new one's (fxc_set_stream)
    Event ev_res[kResSlots];         // marks result slot k complete
    Event ev_t0, ev_t1;              // fxc_timer_start / _stop
    std::vector<std::pair<Event, Event>> kev;      // kernel profiling: start and stop of every timed launch not yet read
    int device = 0, cu_count = 0;
    int n_ant = 0, n_base = 0, nchan = 0, ntaps = 0;
    // products (fxc_set_products): the n_base cross rows of a result, then with autos one row per antenna -- n_prod rows
    bool autos = false;
    int n_prod = 0;
    int64_t x_resident_auto = 0;   // workgroups of xengine_kernel<n_ant, true> the device holds at once (set with the autos)
    int64_t num_samp = 0, n_pts = 0;
    int path = FXC_PATH_GENERIC;
    bool pow2 = false;
    int lg2n = 0;
    bool mixed = false;            // generic F stage = pfb_fft_mixed_kernel (FIR + mixed-radix FFT in one pass)
    fxc::MixedPlan mixed_plan{};
    int mixed_tpr = 256;           // threads per row
    bool mixed_blu = false;        // a large prime factor (plan_route): chirp-z rows of blu_nfft points (F only)
    int blu_nfft = 0;
    DevBuf<cf> d_chirp;         // [nchan] exp(+i pi n^2 / nchan)
    DevBuf<cf> d_blud;          // [blu_nfft] FFT of the wrapped conjugate chirp / blu_nfft
    bool mixed_xeng = false;       // 3 .. 64 antennas: F-only mixed kernel (antenna-interleaved spectra) + the X-engines
    bool mixed_xf_twl = true;      // ... with the twiddle table in LDS (up to 4096 channels; from L2 up to 5120)
    bool mixed_xf = false;         // two antennas: the same kernel multiplies and integrates too (no spectra in HBM)
    bool xf_bytes_only = false;    // ... for the receivers' bytes only: complex64 input takes the F stage built for the channel count + xmul_kernel
    // ... and, where the shape allows, in the build of fx_spec.h made for exactly this channel count (h_rtc.h); spec_u8: its
    // byte-ingest twin, compiled when bytes first arrive
    const SpecKernel* spec = nullptr;
    bool spec_tried = false;
    const SpecKernel* spec_u8 = nullptr;
    bool spec_u8_tried = false;
    const SpecKernel* spec_f = nullptr;      // the F stage alone (fxc_channelize, 3 + antennas), built on first use
    bool spec_f_tried = false;
    const SpecKernel* spec_xm = nullptr;     // two antennas above 4096 channels: antenna 1's F stage multiplied into sums with antenna 0's spectra (built on first use)
    bool spec_xm_tried = false;
    bool rtc = true;                         // FXC_RTC as it stood when the plan was made (developer knob: 0 keeps the any-shape kernels)
    int live_pipes = 0;              // fxc_pipe objects that hold a pointer to this plan
    // device tables
    DevBuf<float> d_win;        // [ntaps*nchan] float (generic)
    DevBuf<cf> d_tw;            // generic FFT twiddles
    DevBuf<cd> d_rot;           // [nchan]
    // per-antenna rot (fxc_set_rot_ant, 3 and more antennas; 2 antennas fold theirs into d_rot): the finish kernels' ANT
    // instantiations read r_a[k] from d_rot_ant[n_ant][nchan] (allocated by the first call) and baseline p's (a, b) from d_pair
    bool rot_ant = false;
    DevBuf<cd> d_rot_ant;
    DevBuf<int2> d_pair;        // [n_base] (plan_build)
    // delay track (fxc_set_delay_track): chunk t of every rows / accumulate call takes the rot of tau0 + t rate, written by
    // track_tables_kernel (k_track.h) for the chunks of a pass into d_track; track_t is the next chunk's index
    bool track = false;
    int64_t track_t = 0;
    double track_df = 0.0, track_freq = 0.0;     // bin spacing as numpy forms it, centre frequency
    DevBuf<double> d_track_par;   // [2][n_ant] tau0, rate
    DevBuf<void> d_track;         // the tables of one pass
    DevBuf<cd> d_one;             // [nchan] of 1: a tracked integration's accumulator holds rotated sums, the finalize kernels' rot
    bool acc_track = false;          // the chunks in the accumulator (spectra_count > 0) were folded under a track
    // gain track (fxc_set_track_gains) under the delay track: d_gain_q = 1 / g of every solution, [gain_n][n_ant][nchan] in
    // natural bin order, written once by track_gain_inverse_kernel; gain_n == 0: none, track_tables_kernel runs as before
    DevBuf<cd> d_gain_q;
    int64_t gain_n = 0, gain_interval = 0, gain_first = 0;
    // whole-sample delays: antenna a's samples are read s_a later, zeros where there are none (align_c64_kernel, k_align.h),
    // pass by pass in fx_call_dev into d_align.  shifted: the static shifts of fxc_set_sample_delays, sample_shift on the host
    // and d_shift [n_ant] on the device.  track_align: the per-chunk shifts of fxc_set_delay_track_aligned,
    // s_a(t) = llrint(tau_a(t) track_bw), written for every pass into d_tshift [chunks][n_ant] (tshift_t0: the chunk of its
    // first row) and read by the alignment and by the aligned table kernels alike; track_par_h: tau0, rate on the host
    bool shifted = false;
    std::vector<int64_t> sample_shift;
    DevBuf<int> d_shift;
    bool track_align = false;
    double track_bw = 0.0;
    std::vector<double> track_par_h;
    DevBuf<void> d_tshift;
    int64_t tshift_t0 = 0;
    DevBuf<void> d_align;         // the aligned samples of one pass
    DevBuf<f4> d_win4;          // [nchan] window quads (one unit tap behind the pre-filter): fused, tiled ring, wave-local, lean fx_spec.h
    DevBuf<cf> d_tw1;
    DevBuf<cf> d_tw2;
    DevBuf<cf> d_tw0;           // tiled: pre-stage twiddles [16][nchan/16]
    int tiled_grid_max = 0, tiled_grid_max_f = 0;   // resident workgroups of the F+X / F-only tiled kernels
    bool tiled_f = false;          // the F-only tiled kernel serves fxc_channelize
    bool small = false;            // tiled path, 2 antennas, nchan 16 .. 256: fx_small_ring_kernel (k_small.h);
                                   // tiled_grid_max counts the work items resident at once, small_wgs the workgroups
    bool small_f = false;          // its F-only variant serves fxc_channelize and the 3 .. 8 antenna route (with tiled_f)
    int small_wgs = 0;
    DevBuf<cf> d_tw_small;      // [nchan/16][16] wN^(u k1)
    bool tiled_ring = false;       // ntaps <= 4 and nchan <= 4096: VGPR frame ring + window in LDS
    bool prefilter = false;        // ntaps > 4: pfb_prefilter_kernel first, then the tiled kernels with one unit tap
    int pre_tp = 0;                // its register block: 8, 16 or 32 frames
    DevBuf<float> d_hpre;       // [pre_tp][nchan] reversed polyphase coefficients
    DevBuf<float> d_ones;       // [nchan] unit window of the plain tiled kernel behind the pre-filter
    DevBuf<void> d_pre;         // pre-filtered streams of one pass
    bool f8192 = false;            // nchan 8192, ntaps <= 4: fxc_channelize on f8192_ring_kernel (one stream per workgroup, VGPR ring)
    bool x8192 = false;            // nchan 8192, 2 antennas, ntaps <= 4: two passes (f8192_ring_kernel, then its XM form); FXC_X8192=0: off
    bool split8192 = false;        // nchan 8192, 2 antennas: pfb_split8192_kernel + the 4096-channel fused kernel
    DevBuf<cf> d_tw8192;        // [4096] w8192^(4095 - n')
    DevBuf<f4> d_unit4;         // [4096] unit-tap window quads of the fused kernel behind pfb_split8192_kernel
    DevBuf<unsigned long long> d_stamps;   // diagnostic builds only
    int fused_grid_max = 0;
    int64_t x_resident = 0;        // workgroups of the X-engine kernel the device holds at once
    bool x_mfma = false;           // more than 8 antennas: xengine_mfma_kernel (k_xmfma.h)
    int64_t fused_seg = 1;         // chunks per round-robin segment of the fused kernel (fx_fused4096.h::RangeWalk)
    DevBuf<cd> d_acc;           // [n_prod*nchan] (allocated for the autos too: acc_capacity)
    DevBuf<cd> d_sums;          // [n_prod*nchan + 1]
    DevBuf<cd> d_cont;          // [n_prod*nchan + 1] the export a CONTINUUM finalize of the accumulator reduces (lazy)
    bool sums_valid = false;       // d_sums holds exported sums (fxc_reduce): fxc_finalize_sums(plan, NULL, ...) may read it
    // raw rows of the last fx_accumulate pass whose fold into the accumulator is still to be launched: it is launched
    // by whatever needs the accumulator or the workspace next (flush_pending) -- by a finalize together with the
    // export / finalize / reset of every element, in the same kernel
    struct Pending {
        bool valid = false;
        const cf* raw = nullptr;
        cd* part = nullptr;
        int64_t n_rows = 0;
        int layout = 0;
    } pend;
    // finalize results: kResSlots pinned host buffers mapped into the device (the finishing kernel writes the
    // visibilities straight into them: no staging copy), each with the event that marks it complete
    PinnedBuf h_res[kResSlots];
    cd* d_res[kResSlots] = {nullptr, nullptr};     // the same memory as the device sees it (not owned: h_res[] is)
    size_t res_bytes[kResSlots] = {0, 0};
    void* res_dst[kResSlots] = {nullptr, nullptr};    // fxc_finalize_async_to: the caller's buffer for this result
    void* res_user[kResSlots] = {nullptr, nullptr};   // ... and whether the device delivers into it (else via the slot + a copy)
    int64_t res_head = 0, res_tail = 0;            // results queued / collected
    double spectra_count = 0.0;
    // workspace (grown on demand)
    DevBuf<void> d_ws;
    DevBuf<void> d_stage[3];       // host-buffer calls: device copies of x and out; uint8 calls on plans without the fused
                                   // ingest: the converted samples
    DevBuf<void> d_rowpart;        // continuum rows of a few-row call: float64 partial sums per bin slice
    DevBuf<void> d_dc;             // uint8 ingest: byte sums + conversion offsets per stream
    // timing
    bool profiling = false;
    double kernel_ms = 0.0;
    int64_t kernel_launches = 0;
    int stamp_grid = 0;
    StreamTaps taps;               // nchan == 1: the FIR taps by value
    mutable std::string error;
};

struct fxc_pipe {
    fxc_plan* plan = nullptr;
    int64_t chunks = 0;
    int depth = 0, mode = FXC_MODE_SPECTRUM;
    double bandwidth = 1.0;
    size_t in_bytes = 0, out_bytes = 0;
    bool counted = false;      // registered in plan->live_pipes
    int fmt = FXC_IQ_C64;      // sample format of the batches (fxc_iq_format)
    int remove_dc = 0;
    Stream s_in, s_out;        // (ahead of the slots: destroyed after them)
    std::vector<fxc_pipe_slot> slots;
    int64_t pushed = 0, popped = 0;
};

namespace {

// elements of the accumulator (and of every buffer sized like it): room for the autos rows of plans that may have them, so that
// fxc_set_products allocates nothing
int64_t acc_capacity(const fxc_plan* p) {
    return (int64_t)(p->n_base + (p->n_ant >= 2 && p->n_ant <= 8 ? p->n_ant : 0)) * p->nchan;
}

int fail(const fxc_plan* p, int status, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (p)
        p->error = buf;
    else
        g_lib_error = buf;
    return status;
}

// Every ABI entry runs on the plan's device and leaves the caller's current device as it found it (a process
// that drives several GPUs, or torch's own notion of the current device, must not see it change).
struct DeviceGuard {
    int prev = -1;
    bool changed = false, ok = true;
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) {
            ok = hipSetDevice(device) == hipSuccess;
            changed = ok && prev >= 0;
        }
    }
    ~DeviceGuard() {
        if (changed) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define FXC_DEVICE(p, device)                                                                  \
    DeviceGuard device_guard__(device);                                                        \
    if (!device_guard__.ok) return fail(p, FXC_ERR_HIP, "hipSetDevice(%d) failed", (int)(device))

#define FXC_HIP(p, call)                                                                                       \
    do {                                                                                                       \
        hipError_t e__ = (call);                                                                               \
        if (e__ != hipSuccess)                                                                                 \
            return fail(p, e__ == hipErrorOutOfMemory ? FXC_ERR_NOMEM : FXC_ERR_HIP, "%s failed: %s", #call,   \
                        hipGetErrorString(e__));                                                               \
    } while (0)

int bad_mem_kind(const fxc_plan* p, int mem_kind) {      // FXC_OK for host and for device memory
    return mem_kind == FXC_MEM_HOST || mem_kind == FXC_MEM_DEVICE ? FXC_OK : fail(p, FXC_ERR_ARG, "bad mem_kind %d", mem_kind);
}

constexpr int64_t kGridMax = 65535;      // gridDim.y, gridDim.z
int64_t up256(int64_t bytes) { return (bytes + 255) / 256 * 256; }      // up to the 256-byte boundary a workspace block starts on

int grid_for(int64_t work_items, int block, int cu_count) {
    int64_t g = (work_items + block - 1) / block;
    const int64_t cap = (int64_t)cu_count * 8;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

// launches the fold of the pending raw rows (h_launch.h); every user of the workspace or the accumulator calls it first
int flush_pending(fxc_plan* p, const FoldFinish* fin = nullptr, hipEvent_t done = nullptr);

int ensure_ws(fxc_plan* p, int64_t bytes) {
    const int rf = flush_pending(p);        // the pending rows (and their partials) live in the workspace
    if (rf) return rf;
    if ((size_t)bytes <= p->d_ws.bytes()) return FXC_OK;
    if (p->d_ws) {
        FXC_HIP(p, hipStreamSynchronize(p->stream));
        p->d_ws.reset();
    }
    FXC_HIP(p, p->d_ws.alloc((size_t)bytes));
    return FXC_OK;
}

// grow-only device buffer owned by the plan (staging, conversion offsets), `want` bytes
int grow(fxc_plan* p, DevBuf<void>& buf, size_t want) {
    bool sync_failed = false;
    const hipError_t e = buf.grow(p->stream, want, &sync_failed);
    if (sync_failed)
        return fail(p, e == hipErrorOutOfMemory ? FXC_ERR_NOMEM : FXC_ERR_HIP, "hipStreamSynchronize(p->stream) failed: %s", hipGetErrorString(e));
    if (e != hipSuccess) return fail(p, FXC_ERR_NOMEM, "allocation of %zu bytes failed: %s", want, hipGetErrorString(e));
    return FXC_OK;
}

struct KernelTimer {
    fxc_plan* p;
    Event a, b;
    explicit KernelTimer(fxc_plan* plan) : p(plan) {
        if (p->profiling && a.create(hipEventDefault) == hipSuccess && b.create(hipEventDefault) == hipSuccess)
            (void)hipEventRecord(a, p->stream);
        else
            a.reset();
    }
    void stop() {
        if (a) {
            (void)hipEventRecord(b, p->stream);
            p->kev.emplace_back(std::move(a), std::move(b));
        }
    }
};

int drain_kernel_events(fxc_plan* p) {
    for (auto& e : p->kev) {
        FXC_HIP(p, hipEventSynchronize(e.second));
        float ms = 0.f;
        FXC_HIP(p, hipEventElapsedTime(&ms, e.first, e.second));
        p->kernel_ms += ms;
        p->kernel_launches += 1;
    }
    p->kev.clear();
    return FXC_OK;
}
}  // namespace
