// Part of libfxcorr's single translation unit: included by fxcorr.hip (not a stand-alone header).
#pragma once

namespace {

// ---- the ingest front end --------------------------------------------------------------------------------------------------
// Every entry point that takes samples (fxc_fx_rows / fxc_fx_accumulate and their _u8 and _iq spellings) and the pipe describe
// their call as an FxCall and come through here: one set of sizes, one argument check, one host / device dispatch (fx_call) and
// one device-side driver (fx_call_dev) that conditions the samples pass by pass and hands each pass to the plan's kernels,
// fx_rows_dev / fx_accumulate_dev of h_run.h.
struct FxCall {
    int fmt;             // fxc_iq_format of the samples
    bool remove_dc;      // subtract every stream's mean first
    bool rows;           // fxc_fx_rows semantics, else accumulate: mode and bandwidth are then never read
    int mode;
    double bandwidth;
};

size_t sample_bytes(int fmt) { return fmt == FXC_IQ_U8 ? 2 : (fmt == FXC_IQ_C128 ? sizeof(cd) : sizeof(cf)); }
size_t input_bytes(const fxc_plan* p, int fmt, int64_t n_chunks) { return (size_t)n_chunks * p->n_ant * p->num_samp * sample_bytes(fmt); }
// rows of one chunk
size_t row_bytes(const fxc_plan* p, int mode) {
    return mode == FXC_MODE_SPECTRUM ? (size_t)p->n_prod * p->nchan * sizeof(cf) : (size_t)p->n_prod * sizeof(cd);
}

// what a plan and a call description must agree on (the pipe checks this much when it is created)
int check_call(const fxc_plan* p, const FxCall& c) {
    if (p->n_ant < 2) return fail(p, FXC_ERR_ARG, "cross-correlation needs n_ant >= 2");
    if (c.rows && c.mode != FXC_MODE_SPECTRUM && c.mode != FXC_MODE_CONTINUUM) return fail(p, FXC_ERR_ARG, "bad mode %d", c.mode);
    if (c.rows && c.mode == FXC_MODE_CONTINUUM && !(c.bandwidth > 0.0)) return fail(p, FXC_ERR_ARG, "bandwidth must be > 0");
    if (c.fmt != FXC_IQ_C64 && c.fmt != FXC_IQ_U8 && c.fmt != FXC_IQ_C128) return fail(p, FXC_ERR_ARG, "bad iq_format %d", c.fmt);
    return FXC_OK;
}

// the argument check of every entry point; *done: the call is valid and has nothing to do
int check_entry(const fxc_plan* p, const FxCall& c, const void* x, const void* out, int64_t n_chunks, bool* done) {
    *done = false;
    if (!p) return fail(p, FXC_ERR_ARG, "NULL plan");
    if (n_chunks < 0) return fail(p, FXC_ERR_ARG, "n_chunks < 0");
    if (const int rc = check_call(p, c)) return rc;
    *done = n_chunks == 0;
    if (!*done && (!x || (c.rows && !out))) return fail(p, FXC_ERR_ARG, "NULL buffer");
    return FXC_OK;
}

// FXC_MEM_DEVICE_TO_PINNED: the rows of device-resident samples go straight into fxc_host_alloc memory -- the finishing
// kernel writes them across PCIe through the device's mapping of the block, nothing is copied and nothing waits
int pinned_rows_out(fxc_plan* p, void** out, int* mem_kind, int64_t n_chunks, int mode) {
    if (*mem_kind != FXC_MEM_DEVICE_TO_PINNED) return FXC_OK;
    if (!p || !*out || n_chunks <= 0) {
        *mem_kind = FXC_MEM_DEVICE;         // (the entry's own argument checks answer)
        return FXC_OK;
    }
    const size_t ob = (size_t)n_chunks * row_bytes(p, mode);
    void* d = pinned_device_ptr(*out, ob);
    if (!d) return fail(p, FXC_ERR_ARG, "`out` of FXC_MEM_DEVICE_TO_PINNED (%zu bytes) is not inside memory from fxc_host_alloc", ob);
    *out = d;
    *mem_kind = FXC_MEM_DEVICE;
    return FXC_OK;
}

// whole-sample delays in force (fxc_set_sample_delays, fxc_set_delay_track_aligned): every pass is aligned before the plan's kernels
bool aligning(const fxc_plan* p) { return p->shifted || (p->track && p->track_align); }

// ---- conditioning launches (also what the stand-alone fxc_remove_dc / fxc_convert_u8 run) -------------------------------------
// workgroups per stream of the subtract / narrow pass: enough to fill the chip when a call has few streams (one chunk
// pair: the reference's own call), a handful when it has thousands
int cond_slices(const fxc_plan* p, int64_t n_streams) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(256, ((int64_t)p->cu_count * 8 + n_streams - 1) / n_streams));
}
// slice sums per stream (each a workgroup): 32 for batches, up to 256 when a call has a handful of streams (one chunk pair:
// 64 workgroups of 32 sequential loads each took 7 us for 4 MiB)
int sum_slices(const fxc_plan* p, int64_t n_streams) {
    return (int)std::max<int64_t>(32, std::min<int64_t>(256, (int64_t)p->cu_count * 4 / n_streams));
}

// complex64 streams minus their means: n_slices slice sums per stream into part, then the subtraction
void launch_remove_dc_c64(fxc_plan* p, const cf* x, cf* out, double* part, int64_t n_streams, int n_slices) {
    const int app = cond_slices(p, n_streams);
    hipLaunchKernelGGL(dc_sum_c64_kernel, dim3(n_slices, (unsigned)n_streams), dim3(256), 0, p->stream, x, part, p->num_samp, n_slices);
    hipLaunchKernelGGL(dc_apply_c64_kernel, dim3(app, (unsigned)n_streams), dim3(256), 0, p->stream, x, out, part, p->num_samp, app,
                       n_slices, 1);
}

// byte sums of n_streams streams, n_slices per stream
void launch_dc_sum_u8(fxc_plan* p, const unsigned char* x8, double* part, int64_t n_streams, int n_slices) {
    hipLaunchKernelGGL(dc_sum_u8_stream_kernel, dim3((unsigned)std::min<int64_t>(n_streams * n_slices, (int64_t)p->cu_count * 16)),
                       dim3(256), 0, p->stream, x8, part, p->num_samp, n_streams, n_slices);
}

// bytes -> complex64 of n_streams streams: a few thousand workgroups, each on one slice of a stream at a time
void launch_convert_u8(fxc_plan* p, const unsigned char* x8, cf* out, const double* part, int n_slices, int64_t n_streams, bool remove_dc) {
    const unsigned gy = (unsigned)std::min<int64_t>(n_streams, 65535);
    const int64_t per_stream = std::max<int64_t>(1, ((int64_t)p->cu_count * 16 + gy - 1) / gy);
    const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(per_stream, (p->num_samp + 1023) / 1024));
    hipLaunchKernelGGL(convert_u8_kernel, dim3(gx, gy), dim3(256), 0, p->stream, x8, out, part, p->num_samp, n_slices, n_streams,
                       remove_dc ? 1 : 0);
}

// ---- the per-format "condition this pass" steps ----------------------------------------------------------------------------
// What a step hands back: the samples the plan's kernels read and, where they read the receivers' bytes themselves, the
// per-stream conversion offsets and whether the kernel sums its later chunks' bytes itself (k_fused4096.h, DCK).
struct PassInput {
    const cf* x = nullptr;
    const cf* dc_u8 = nullptr;
    bool dck = false;
};

// uint8 I,Q in: fused plans (2 antennas: nchan 4096 / ntaps 4, the tiled ring and wave-local kernels, the mixed-radix F + X
// kernel) read the bytes in the F+X kernel itself; every other plan converts a pass into a complex64 staging buffer first
// (never with whole-sample delays in force: the bytes are converted, then aligned)
bool u8_fused_in(const fxc_plan* p) {
    return p->n_ant == 2 && !p->autos && !p->prefilter && !aligning(p) && (p->path == FXC_PATH_FUSED || (p->path == FXC_PATH_TILED && (p->tiled_ring || p->small || p->x8192)) ||
                                                           (p->path == FXC_PATH_GENERIC && p->mixed_xf && FXC_DEV_ENV_INT("FXC_MIXED_U8", 1)));
}

int condition_u8(fxc_plan* p, const unsigned char* xb, int64_t nc, bool remove_dc, bool fused_in, PassInput* in) {
    constexpr int kSlices = 32;
    const int64_t n_streams = nc * p->n_ant;
    // d_dc: the slice sums, then the conversion offsets
    const size_t part_bytes = (size_t)n_streams * kSlices * 2 * sizeof(double);
    int rc = grow(p, p->d_dc, part_bytes + (size_t)n_streams * sizeof(cf));
    if (rc) return rc;
    double* part = static_cast<double*>(p->d_dc.get());
    cf* dc = reinterpret_cast<cf*>(static_cast<char*>(p->d_dc.get()) + part_bytes);
    if (!fused_in) {
        if (remove_dc) launch_dc_sum_u8(p, xb, part, n_streams, kSlices);
        rc = grow(p, p->d_stage[2], (size_t)n_streams * p->num_samp * sizeof(cf));
        if (rc) return rc;
        cf* xc = static_cast<cf*>(p->d_stage[2].get());
        launch_convert_u8(p, xb, xc, part, kSlices, n_streams, remove_dc);
        FXC_HIP(p, hipGetLastError());
        in->x = xc;
        return FXC_OK;
    }
    // The fused 4096-channel kernel can sum the bytes of a workgroup's next chunk while it channelises the current one
    // (k_fused4096.h, DCK): the pre-pass then only covers the first chunk of every workgroup's round-robin share and
    // the tail chunks -- 272 of 10 000 chunk pairs.  Needs whole frames (num_samp % 4096 == 0), 16-byte aligned
    // streams, the default work split (so no delay track), one launch for the pass and at least two rounds of chunks.
    int64_t spec_b, raw_b;
    const int64_t g = p->fused_grid_max;
    // (num_samp <= 2^26: a wave's byte sums are reduced in 32 bits, 16384 frames x 4080 x 64 lanes < 2^32)
    const bool dck = remove_dc && fused_in && !p->track && p->path == FXC_PATH_FUSED && p->fused_seg == 1 &&
                     (p->num_samp % fxc::fused::kN) == 0 && p->num_samp <= (1ll << 26) &&
                     (reinterpret_cast<uintptr_t>(xb) % 16) == 0 &&
                     fused_chunks_per_pass(p, nc, &spec_b, &raw_b) >= nc && nc >= 2 * g;
    if (remove_dc) {
        const int64_t n_full = dck ? nc / g * g : nc;
        // chunk ranges the pre-pass sums: everything, or [0, g) and [n_full, nc)
        const int64_t lo[2] = {0, n_full}, hi[2] = {dck ? g : nc, dck ? nc : n_full};
        // a call of a few streams (one chunk pair: the reference's own call) is cut into slices to fill the chip
        const int sl = dck ? 1 : (int)std::max<int64_t>(1, std::min<int64_t>(kSlices, (int64_t)p->cu_count * 2 / n_streams));
        for (int r = 0; r < 2; ++r) {
            const int64_t ns = (hi[r] - lo[r]) * p->n_ant;
            if (ns <= 0) continue;
            launch_dc_sum_u8(p, xb + lo[r] * p->n_ant * p->num_samp * 2, part + lo[r] * p->n_ant * 2 * sl, ns, sl);
            hipLaunchKernelGGL(dc_offsets_u8_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, p->stream,
                               part + lo[r] * p->n_ant * 2 * sl, dc + lo[r] * p->n_ant, ns, sl, p->num_samp, 1);
        }
    } else {
        hipLaunchKernelGGL(dc_offsets_u8_kernel, dim3((unsigned)((n_streams + 255) / 256)), dim3(256), 0, p->stream, part, dc,
                           n_streams, 1, p->num_samp, 0);
    }
    FXC_HIP(p, hipGetLastError());
    *in = {reinterpret_cast<const cf*>(xb), dc, dck};
    return FXC_OK;
}

// complex64 with DC removal, or complex128 (narrowed on the device, after the DC removal when asked for): sums, then
// subtract / narrow into a complex64 staging buffer -- or in place when the pass is the library's own complex64 copy of a
// host buffer or a pipe slot.  The caller's device buffers are never written.
int condition_iq(fxc_plan* p, const void* xb, int64_t nc, int fmt, bool remove_dc, bool in_place, PassInput* in) {
    const int64_t n_streams = nc * p->n_ant;
    const int n_slices = sum_slices(p, n_streams);
    int rc = grow(p, p->d_dc, (size_t)n_streams * n_slices * 2 * sizeof(double));
    if (rc) return rc;
    double* part = static_cast<double*>(p->d_dc.get());
    cf* xc = in_place ? static_cast<cf*>(const_cast<void*>(xb)) : nullptr;
    if (!in_place) {
        rc = grow(p, p->d_stage[2], (size_t)n_streams * p->num_samp * sizeof(cf));
        if (rc) return rc;
        xc = static_cast<cf*>(p->d_stage[2].get());
    }
    if (fmt == FXC_IQ_C128) {
        const int app = cond_slices(p, n_streams);
        if (remove_dc)
            hipLaunchKernelGGL(dc_sum_c128_kernel, dim3(n_slices, (unsigned)n_streams), dim3(256), 0, p->stream, static_cast<const cd*>(xb),
                               part, p->num_samp, n_slices);
        hipLaunchKernelGGL(narrow_c128_kernel, dim3(app, (unsigned)n_streams), dim3(256), 0, p->stream, static_cast<const cd*>(xb), xc, part,
                           p->num_samp, app, n_slices, remove_dc ? 1 : 0);
    } else {
        launch_remove_dc_c64(p, static_cast<const cf*>(xb), xc, part, n_streams, n_slices);
    }
    FXC_HIP(p, hipGetLastError());
    in->x = xc;
    return FXC_OK;
}

// ---- whole-sample delays: the pass's complex64 samples, conditioned or the caller's own, into the plan's d_align, never in place ----
// Static shifts come from d_shift; under an aligned track the shifts of the pass's chunks -- p->track_t onwards at this moment --
// are written first, for the alignment here and for the tables of the same chunks behind it (track_shifts_pass, h_run.h).
void launch_align_c64(fxc_plan* p, const cf* x, cf* out, const int* shifts, int shift_stride, int64_t n_streams) {
    const int slices = cond_slices(p, n_streams);
    KernelTimer kt(p);
    hipLaunchKernelGGL(align_c64_kernel, dim3(slices, (unsigned)n_streams), dim3(256), 0, p->stream, x, out, shifts, shift_stride, p->n_ant,
                       p->num_samp, slices);
    kt.stop();
}

int align_pass(fxc_plan* p, int64_t nc, PassInput* in) {
    const int64_t n_streams = nc * p->n_ant;
    int rc = grow(p, p->d_align, (size_t)n_streams * p->num_samp * sizeof(cf));
    if (rc) return rc;
    const bool tracked = p->track && p->track_align;
    if (tracked) {
        rc = track_shifts_pass(p, p->track_t, nc);
        if (rc) return rc;
    }
    cf* xa = static_cast<cf*>(p->d_align.get());
    launch_align_c64(p, in->x, xa, tracked ? static_cast<const int*>(p->d_tshift.get()) : p->d_shift, tracked ? p->n_ant : 0, n_streams);
    FXC_HIP(p, hipGetLastError());
    *in = {xa};
    return FXC_OK;
}

// ---- the device-side driver ------------------------------------------------------------------------------------------------
// x on the device in call.fmt.  x_is_scratch: x is the library's own copy (the staging copy of a host buffer, a pipe slot), so
// complex64 samples are de-meaned in place.  Plain complex64 goes to the plan's kernels whole; every other format in passes --
// and so does plain complex64 with whole-sample delays in force: each pass is conditioned as its format asks, then aligned.
int fx_call_dev(fxc_plan* p, const FxCall& c, const void* x, void* out, int64_t n_chunks, bool x_is_scratch) {
    const auto run = [&](const PassInput& in, void* o, int64_t nc) {
        return c.rows ? fx_rows_dev(p, in.x, o, nc, c.mode, c.bandwidth, in.dc_u8, in.dck) : fx_accumulate_dev(p, in.x, nc, in.dc_u8, in.dck);
    };
    const bool al = aligning(p);
    const bool plain = c.fmt == FXC_IQ_C64 && !c.remove_dc;
    if (plain && !al) return run({static_cast<const cf*>(x)}, out, n_chunks);
    const bool u8 = c.fmt == FXC_IQ_U8;
    const bool fused_in = u8 && u8_fused_in(p);
    const bool in_place = x_is_scratch && c.fmt == FXC_IQ_C64;
    // chunks per pass: at most 65535 streams (the stream index rides in a grid dimension of the conditioning kernels), and a
    // pass that is conditioned into the complex64 staging buffer stays within the workspace target -- together with the
    // alignment's staging buffer where whole-sample delays are in force
    int64_t per_pass = 65535 / p->n_ant;
    if (u8) per_pass = std::min<int64_t>(16384, per_pass);
    const int stagings = (!plain && !fused_in && !in_place ? 1 : 0) + (al ? 1 : 0);
    if (stagings) per_pass = std::min<int64_t>(per_pass, ws_target() / (stagings * (int64_t)p->n_ant * p->num_samp * (int64_t)sizeof(cf)));
    if (!u8) per_pass = std::min<int64_t>(per_pass, n_chunks);
    per_pass = std::max<int64_t>(1, per_pass);
    for (int64_t c0 = 0; c0 < n_chunks; c0 += per_pass) {
        const int64_t nc = std::min<int64_t>(per_pass, n_chunks - c0);
        const char* xb = static_cast<const char*>(x) + input_bytes(p, c.fmt, c0);
        void* ob = c.rows ? static_cast<char*>(out) + (size_t)c0 * row_bytes(p, c.mode) : nullptr;
        PassInput in;
        int rc = FXC_OK;
        if (plain)
            in.x = reinterpret_cast<const cf*>(xb);
        else
            rc = u8 ? condition_u8(p, reinterpret_cast<const unsigned char*>(xb), nc, c.remove_dc, fused_in, &in)
                    : condition_iq(p, xb, nc, c.fmt, c.remove_dc, in_place, &in);
        if (rc) return rc;
        if (al) {
            rc = align_pass(p, nc, &in);
            if (rc) return rc;
        }
        rc = run(in, ob, nc);
        if (rc) return rc;
    }
    return FXC_OK;
}

// ---- the entry points' host / device dispatch ------------------------------------------------------------------------------
int fx_call(fxc_plan* p, const FxCall& c, const void* x, void* out, int64_t n_chunks, int mem_kind) {
    if (c.rows)
        if (const int rp = pinned_rows_out(p, &out, &mem_kind, n_chunks, c.mode)) return rp;
    bool done;
    if (const int rc = check_entry(p, c, x, out, n_chunks, &done)) return rc;
    if (done) return FXC_OK;
    FXC_DEVICE(p, p->device);
    if (mem_kind == FXC_MEM_DEVICE) return fx_call_dev(p, c, x, out, n_chunks, false);
    if (const int rc = bad_mem_kind(p, mem_kind)) return rc;
    return with_host_staging(p, x, input_bytes(p, c.fmt, n_chunks), out, c.rows ? (size_t)n_chunks * row_bytes(p, c.mode) : 0,
                             [&](const cf* dx, void* dout) { return fx_call_dev(p, c, dx, dout, n_chunks, true); });
}

}  // namespace
