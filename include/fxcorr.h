/*
 * fxcorr.h — C ABI of the MI355X-native F/X hot path (libfxcorr.so).
 *
 * The reference (evanmayer/effex) is pure Python and has no FFI of its own; its seam is the
 * method surface of `Correlator` (effex/effex.py).  This ABI sits *underneath* that surface and
 * replaces the third-party GPU calls the reference makes on its hot path.  Each entry point
 * names the reference lines it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - every function returns FXC_OK (0) or a negative fxc_status; no exception crosses the ABI;
 *     fxc_last_error(plan) returns a NUL-terminated message owned by the plan (or by the library
 *     for plan == NULL), valid until the next failing call on that plan.
 *   - "complex64" = interleaved float re,im (8 B); "complex128" = interleaved double (16 B).
 *   - all device work is issued asynchronously on the plan's HIP stream; the caller owns every
 *     x/out buffer and keeps it alive until fxc_sync() / a finalize call returns.
 *   - a plan is thread-compatible, not thread-safe (one caller thread per plan — the reference
 *     drives the path from one thread, effex/effex.py:326-417).
 *   - there is NO CPU backend: without a HIP device fxc_plan_create fails with FXC_ERR_NODEVICE.
 *
 * Environment.  The library reads FOUR variables and no others (`strings libfxcorr.so | grep '^FXC_'` lists exactly these):
 *   FXC_RTC          0: plans keep the any-shape kernels for channel counts that are not a power of two instead of building the kernel
 *                    for the channel count (fxc_info.specialised); read when a plan is made.  Default 1.
 *   FXC_RTC_CACHE    directory of the code objects built at run time (default $XDG_CACHE_HOME/fxcorr, else ~/.cache/fxcorr; "0" or
 *                    empty: no files).  The pre-built code objects that ship beside the library are looked up first.
 *   FXC_RTC_VERBOSE  1: one line on stderr per kernel built or loaded for a channel count (stage list, registers, where it came from).
 *   FXC_WS_MB        upper bound of the lazily grown device workspace in MiB (default 12288); calls over more chunks run in passes.
 * Results do not depend on any of them beyond rounding (FXC_RTC chooses between two kernels of the same arithmetic family).  Route and
 * tuning knobs for A/B measurements exist only in the developer build (libfxcorr_dev.so, fxc_dev_kernels() == 1), which tests and
 * tools load explicitly.
 */
#ifndef FXCORR_H
#define FXCORR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FXC_VERSION 106 /* 0.1.1: fxc_info.spec_source, spec_seconds */

typedef struct fxc_plan fxc_plan; /* opaque; one per (device, configuration) */
typedef struct fxc_pipe fxc_pipe; /* opaque; host-fed double-buffered front end on a plan */

#define FXC_STREAM_OWNED ((void*)(intptr_t)-1)

enum fxc_status {
    FXC_OK = 0,
    FXC_ERR_ARG = -1,         /* bad argument (NULL, non-positive size, ...)                     */
    FXC_ERR_UNSUPPORTED = -2, /* ntaps > 32 (cusignal raises NotImplementedError), nchan too big */
    FXC_ERR_HIP = -3,         /* a HIP runtime call failed; message has hipGetErrorString        */
    FXC_ERR_NOMEM = -4,
    FXC_ERR_NODEVICE = -5,
    FXC_ERR_STATE = -6,       /* call sequence error (e.g. finalize with nothing accumulated)    */
    FXC_ERR_COMM = -7         /* librccl could not be bound, or an RCCL call failed              */
};

/* FXC_MEM_DEVICE_TO_PINNED (fxc_fx_rows, _u8, _iq only): x is device memory, `out` lies in memory from fxc_host_alloc -- the
 * finishing kernel writes the rows there across PCIe (no copy, no wait: the call is asynchronous on the plan's stream like any
 * device call; the rows are complete when the stream reaches that point, fxc_sync or an event of the caller's).  For the
 * time-series product of device-resident samples (one row per chunk pair, effex.py:402-410, 687-696). */
enum fxc_mem_kind { FXC_MEM_HOST = 0, FXC_MEM_DEVICE = 1, FXC_MEM_DEVICE_TO_PINNED = 2 };
enum fxc_mode { FXC_MODE_SPECTRUM = 0, FXC_MODE_CONTINUUM = 1 }; /* TEST == CONTINUUM arithmetic */
/* sample formats of the fxc_*_iq entry points: complex64 (what the path computes in), the receivers' interleaved
 * unsigned 8-bit I,Q (pyrtlsdr's packed bytes, effex.py:652), and complex128 (the reference's own sample type,
 * effex.py:109-110: narrowed to complex64 on the device, after the DC removal when that is asked for) */
enum fxc_iq_format { FXC_IQ_C64 = 0, FXC_IQ_U8 = 1, FXC_IQ_C128 = 2 };
enum fxc_path {
    FXC_PATH_GENERIC = 0, /* any shape (nchan <= 16384, ntaps <= 32, 2..64 antennas).  Channel counts that are not a
                             power of two (effex.py:733-739: --resolution is a free integer) and nchan 4 / 8 / 16384 when the
                             path is chosen automatically: FIR + mixed-radix Stockham FFT (chirp-z for large prime factors)
                             in one kernel, which with 2 antennas also multiplies and integrates; otherwise FIR / radix-2
                             FFT / X kernels through a workspace (the tests' independent reference when forced)      */
    FXC_PATH_FUSED = 1,   /* nchan 4096, ntaps 4, 2 antennas (one kernel) or 4/6/8 (F-only kernel + X-engine) */
    FXC_PATH_STREAM = 2,  /* nchan 1, 2 antennas: the continuum streaming limit                             */
    FXC_PATH_TILED = 3    /* nchan 512/1024/2048/4096/8192, any ntaps: 2 antennas in one fused F+X kernel, 3..64
                             via its F-only variant + X-engine; nchan 16/32/64/128/256, ntaps <= 4: the same
                             design inside one wave (2 antennas, or 3..64 via its F-only variant)           */
};

typedef struct fxc_info {
    int32_t n_ant, n_baselines, nchan, ntaps;
    int64_t num_samp, n_pts;   /* n_pts = num_samp / nchan spectra per chunk (effex.py:553)     */
    int32_t path;              /* fxc_path actually used by fxc_fx_* for this configuration      */
    int32_t grid, block;       /* launch geometry of the dominant kernel                         */
    int32_t lds_bytes;         /* dynamic LDS of the dominant kernel                             */
    int32_t device, cu_count;
    int64_t workspace_bytes;
    int32_t specialised;       /* bit 0: the F+X kernel was compiled for exactly this channel count when the plan was made
                                  (two antennas, a channel count that is not a power of two, up to four taps); bit 1: so was
                                  the F stage alone (built at the first fxc_channelize / multi-antenna call); bit 2: and the second
                                  pass of two antennas above 4096 channels (antenna 1's F stage multiplied with antenna 0's spectra) */
    int32_t spec_vgprs;        /* its vector registers per lane                                                          */
    int32_t spec_source;       /* where its code object came from: 0 none, 1 built by hiprtc when the plan was made, 2 the cache of
                                  earlier builds (FXC_RTC_CACHE), 3 pre-built beside the library (rtc_prebuilt/, made at build time
                                  for a stated list of channel counts: effex_amd/build.py::PREBUILT)                     */
    float   spec_seconds;      /* what getting it took when the plan was made (hiprtc: seconds; a file: milliseconds)      */
} fxc_info;

int         fxc_version(void);
int         fxc_dev_kernels(void); /* 0: the shipped library; 1: the developer build with the reference / A-B kernels as well */
int         fxc_device_count(int* count);
const char* fxc_status_string(int status);

/* Plan = the configuration Correlator.__init__ fixes once (effex.py:109-127): antenna count,
 * nbins, ntaps, num_samp and the PFB window (float64 design, used as float32 on the device).
 * `window` is host memory, [ntaps*nchan] doubles, copied.  `stream` is the hipStream_t to issue
 * work on: the caller's stream (e.g. torch.cuda.current_stream().cuda_stream, so the plan's kernels
 * are ordered with the caller's own work on that stream), NULL for HIP's default (null) stream, or
 * FXC_STREAM_OWNED for a private non-blocking stream the caller then orders against with fxc_sync().
 * force_path: -1 = choose automatically, else an fxc_path (FUSED fails if the shape has none). */
int fxc_plan_create(fxc_plan** out, int device, int n_ant, int nchan, int ntaps, int64_t num_samp,
                    const double* window, void* stream, int force_path);
int fxc_plan_destroy(fxc_plan* plan); /* FXC_ERR_STATE while an fxc_pipe still uses the plan */
/* Move the plan to another hipStream_t (e.g. when the caller's current stream changes, `with torch.cuda.stream(s)`):
 * everything already queued on the old stream is ordered before what follows on the new one by an event, no host
 * wait.  Not for plans that own their stream. */
int fxc_set_stream(fxc_plan* plan, void* stream);
int fxc_plan_get_info(const fxc_plan* plan, fxc_info* info);
/* Diagnostic: build the specialised kernel (fxc_info.specialised) for `nchan` channels and `ntaps` taps -- variant 0: F+X from
 * complex64 samples, 1: F+X from the receivers' bytes, 2: the F stage alone (fxc_channelize; the F pass of 3 and more
 * antennas), 3: the second pass of two antennas above 4096 channels -- for the device architecture `arch` ("gfx950"; NULL: the current
 * device's), without a device and without a plan: the library's embedded kernel source through hiprtc.  FXC_OK and a one-line
 * description in `report` (may be NULL: "nchan= ntaps= tpr= slots= frames_per_step= stages= lds_bytes= code_bytes= vgprs= scratch=
 * resident= lean= rows= groups= pads= plane0= twfull= waves=" -- threads per frame, frames side by side in a workgroup, frames per step,
 * the stage radices in order, whether taps and twiddles come from tables (above 2048 channels), streams per workgroup, rows per work
 * item of each stage, the LDS layout of the stage buffers, the largest radix whose twiddles all stay in registers, waves per SIMD the
 * registers were held to); FXC_ERR_UNSUPPORTED when the shape has no such kernel (plans of that shape run the
 * any-shape kernel); FXC_ERR_HIP with the compiler's log in fxc_last_error(NULL) when the build fails.
 * (The reference takes any integer --resolution, effex.py:733-739; this is where the build meets that freedom.) */
int fxc_spec_probe(int nchan, int ntaps, int variant, const char* arch, char* report, int report_bytes);
const char* fxc_last_error(const fxc_plan* plan);

/* Products.  A plan makes cross products only (FXC_PRODUCTS_CROSS, the default) or cross products and the autocorrelation of
 * every antenna (FXC_PRODUCTS_CROSS_AUTO).  With autos a result has n_rows = n_baselines + n_ant rows: the cross rows first, in
 * the order and with the meaning they have without autos, then one row per antenna a = 0 .. n_ant-1:
 *   SPECTRUM : fftshift(mean_i |f_a[i,k]|^2) over the same spectra the cross rows average;
 *   CONTINUUM: the mean over the bins of that, divided by `bandwidth` (the cross formula, effex.py:523-524);
 *   rot (fxc_set_rot) is not applied to them (it is a per-baseline phase) and their imaginary part is an exact 0.
 * The autos are those of the samples the cross rows see: after the byte conversion and the DC removal of the *_u8 / *_iq calls.
 * Everything sized by n_baselines without autos is sized by n_rows with them: the rows of fxc_fx_rows (_u8, _iq) and of the
 * pipes, the results of every finalize call, the accumulator and its export (n_rows*nchan + 1 complex128).  Two antennas at
 * nchan 4096 / ntaps 4 (FXC_PATH_FUSED) sum the autos inside the fused F+X kernel, one pass over the samples; other plans with autos
 * take the plan's F stage alone (what fxc_channelize runs) into the workspace and then the X-engine that also sums |f_a|^2 --
 * streaming plans (nchan 1) pay about 30 x their cross-only time for that and should not ask for autos yet.  Plans without autos
 * run exactly the kernels they run without this call.
 * fxc_set_products: FXC_OK, FXC_ERR_ARG (NULL plan, unknown value), FXC_ERR_UNSUPPORTED (autos for more than 8 antennas),
 * FXC_ERR_STATE unless the accumulator is empty (nothing accumulated since the last reset or resetting finalize), no finalize
 * result is outstanding and no fxc_pipe uses the plan.  fxc_plan_products: the current products and rows per result (either
 * pointer may be NULL). */
enum fxc_products { FXC_PRODUCTS_CROSS = 0, FXC_PRODUCTS_CROSS_AUTO = 1 };
int fxc_set_products(fxc_plan* plan, int products);
int fxc_plan_products(const fxc_plan* plan, int* products, int* n_rows);

/* rot[k] = exp(+2*pi*i*f_k*tau), natural bin order — effex.py:516,519.  Formed by the caller in
 * float64 (phase ~ 9e3 rad), complex128[nchan] host memory, copied.  Default: all ones. */
int fxc_set_rot(fxc_plan* plan, const double* rot_re_im);

/* Per-antenna rot: rot_ant = [n_ant][nchan] complex128 host memory, copied; row a is antenna a's table
 * r_a[k] = exp(+2*pi*i*f_k*tau_a), natural bin order.  Cross row (a,b), a < b, in the baseline order of the results is then
 *   fftshift( raw_ab[k] * r_a[k] * conj(r_b[k]) / count )
 * (with r_0 = 1 and r_1 = rot: exactly fxc_set_rot(rot), effex.py:516-521).  The kernels form w[k] = r_b[k] * conj(r_a[k]) in
 * float64 and multiply by conj(w) as they do by conj(rot).  Auto rows (FXC_PRODUCTS_CROSS_AUTO) take no rot.  Two antennas: the
 * one w is formed here and becomes the shared table.  Like fxc_set_rot it synchronises the plan's stream first and applies to
 * every finishing kernel queued afterwards (rows, every finalize form, fxc_finalize_sums, pipes); of the two calls the last one
 * wins.  The tables need not have unit modulus: they are copied as they are, and r_a = 1 / g_a with the gains of
 * fxc_solve_gains corrects the rows' amplitudes and phases.  FXC_ERR_ARG: a NULL argument, n_ant < 2. */
int fxc_set_rot_ant(fxc_plan* plan, const double* rot_ant_re_im);

/* Delay track: delays that move with the chunk index (fringe stopping; the reference's TEST sweep, effex.py:403-404).  The plan
 * keeps a chunk counter t, set to first_chunk here.  Chunk t is phased with the per-antenna tables of
 *   tau_a(t) = tau0_s[a] + t * rate_s_per_chunk[a],   r_a[k](t) = exp(+2*pi*i*f_k*tau_a(t)),
 *   f_k = fftfreq(nchan, 1/bandwidth)[k] + frequency
 * exactly as fxc_set_rot_ant would phase it with the tables of that chunk (two antennas with tau0 = (0, tau) and rate 0:
 * fxc_set_rot of rot(tau)); auto rows take no rot.  The tables are formed on the device, in float64 (f_k*tau in turns, rounded
 * once, reduced, sincospi), from (a, k, t) alone: the rows of a chunk do not depend on how calls and passes batch the chunks.
 * Every call that consumes chunks takes t, t+1, ... for them and advances the counter by their number: fxc_fx_rows (_u8, _iq),
 * fxc_fx_accumulate (_u8, _iq), and the batches of a pipe in submit order.  A tracked fxc_fx_accumulate applies rot chunk by
 * chunk before it sums: it runs the raw rows of fxc_fx_rows (one row set per chunk) and folds raw * conj(w_t) into the float64
 * accumulator in chunk order, so the accumulator (and fxc_acc_export, fxc_reduce) holds rotated sums and every finalize form
 * multiplies by 1 instead of conj(rot) while the track is set; count, fftshift and continuum scaling are unchanged.  Chunks
 * accumulated with and without a track do not mix in one integration: fxc_set_delay_track answers FXC_ERR_STATE while the
 * accumulator holds chunks accumulated without one, fxc_set_rot / fxc_set_rot_ant while it holds tracked ones (fxc_acc_reset or
 * a finalize with reset empties it).  fxc_set_rot and fxc_set_rot_ant end the track; the last of the three calls wins.  Plans
 * without a track run exactly the kernels they run without these calls.
 * fxc_set_delay_track synchronises the plan's stream.  FXC_ERR_ARG: a NULL argument, n_ant < 2, a non-finite value,
 * bandwidth <= 0, first_chunk < 0.  FXC_ERR_STATE: as above, or an fxc_pipe uses the plan (create the pipe after the track).
 * fxc_delay_track_chunk: the counter (the index the next chunk takes); fxc_delay_track_seek moves it (a sharded run starts each
 * rank at the first chunk of its range); both FXC_ERR_STATE without a track, seek FXC_ERR_ARG for chunk < 0.
 * fxc_delay_track_tables: the tables r_a[k](chunk) as the device forms them, out_re_im = [n_ant][nchan] complex128 host memory,
 * computed by the same device code and copied out; synchronises. */
int fxc_set_delay_track(fxc_plan* plan, const double* tau0_s, const double* rate_s_per_chunk, double bandwidth, double frequency,
                        int64_t first_chunk);
int fxc_delay_track_chunk(const fxc_plan* plan, int64_t* next_chunk);
int fxc_delay_track_seek(fxc_plan* plan, int64_t chunk);
int fxc_delay_track_tables(fxc_plan* plan, int64_t chunk, double* out_re_im);

/* Gain track: per-interval gain corrections applied under a delay track.  A plan with a delay track may also carry a gain track:
 *   - n_solutions sets of gains g[s][a][j], gains_re_im = [n_solutions][n_ant][nchan] complex128 host memory with the bins in the
 *     rows' fftshifted order: exactly what fxc_solve_gains writes;
 *   - interval >= 1 chunks per solution, and a first_chunk.
 * Chunk t takes solution
 *   s(t) = clamp(floor((t - first_chunk) / interval), 0, n_solutions - 1):
 * chunks before the first interval use the first solution, chunks after the last interval the last one.  The solutions are
 * piecewise constant; interpolation between solutions is out of scope.
 * The correction of antenna a is
 *   q[s][a][k] = 1 / g[s][a][(k + nchan/2) % nchan]
 * (nchan/2 is integer division: numpy's ifftshift, odd channel counts included).  The inverse is (x/d, -y/d) with d = x*x + y*y,
 * every operation rounded on its own, and 0 where g == 0, so a dead channel stays zero.
 * The table of chunk t is
 *   r_a[k](t) = phasor_a[k](t) * q[s(t)][a][k],
 * phasor being the delay track's exp(+2*pi*i*f_k*tau_a(t)) above; the product is (c*qx - s*qy, c*qy + s*qx), without contraction
 * to fused multiply-adds, as the phasor itself.  A table therefore depends on (a, k, t) and the gain track alone, and with every
 * gain equal to 1 the tables are the plain track's tables, element for element.
 * Everything downstream of the tables is unchanged (rows, tracked fxc_fx_accumulate and every finalize form, pipes, sharded runs
 * with fxc_delay_track_seek): cross row (a,b) of chunk t is raw_ab * r_a * conj(r_b) / count, two antennas take w = r_1 conj(r_0),
 * and auto rows take no rot and no gain, as under fxc_set_rot_ant.
 * fxc_set_track_gains copies the gains to the device and forms q there, once (q stays resident in the plan and is freed with
 * it); it synchronises the plan's stream, as fxc_set_delay_track does.  n_solutions == 0 (gains_re_im may be NULL) removes the
 * gain track and keeps the delay track.  interval may be 0 only when n_solutions == 1: the one solution applies to every chunk.
 * FXC_ERR_ARG: a NULL plan, NULL gains with n_solutions > 0, n_solutions < 0, interval < 1 with more than one solution (or
 * < 0), first_chunk < 0, a non-finite gain, a non-zero gain with |g| outside [1e-150, 1e150] (d would overflow or underflow).
 * FXC_ERR_STATE: the plan has no delay track, the accumulator holds chunks (finalize or reset first), an fxc_pipe uses the plan.
 * FXC_ERR_NOMEM: the n_solutions * n_ant * nchan * 16 bytes of device memory (and as much again while the call runs) cannot be
 * allocated.  A call that fails changes nothing: an earlier gain track stays in force.
 * fxc_set_delay_track removes the gain track (gains were solved on rows made under one particular track: send them again after
 * a new track); fxc_set_rot and fxc_set_rot_ant end both, under the accumulator rule they already have.  The last call wins.
 * fxc_track_gains_info reports (n_solutions, interval, first_chunk), zeros when the plan has a delay track and no gain track;
 * FXC_ERR_STATE when it has no delay track, FXC_ERR_ARG for a NULL argument.  fxc_delay_track_tables returns the tables as
 * applied, gains included; fxc_delay_track_chunk and fxc_delay_track_seek are untouched.  Plans without a gain track launch
 * exactly the kernels they launch without these calls. */
int fxc_set_track_gains(fxc_plan* plan, const double* gains_re_im, int64_t n_solutions, int64_t interval, int64_t first_chunk);
int fxc_track_gains_info(const fxc_plan* plan, int64_t* n_solutions, int64_t* interval, int64_t* first_chunk);

/* Whole-sample delays: every delay above is a phase slope applied after the FFT -- the fractional-sample half of a correlator's
 * delay correction.  A slope cannot put back samples that sit in different frames: for a delay of d samples two antennas' frames
 * overlap only partly and the correlated amplitude falls roughly as 1 - d/nchan whatever the tables hold (half the signal at 64
 * channels and d = 42).  These calls are the whole-sample half: they move the sample stream.
 * A shift s_a (either sign) means that the plan's kernels read, for chunk c, antenna a and sample n, the delivered sample
 *   x[c][a][n + s_a]   when 0 <= n + s_a < num_samp,   and exactly 0 otherwise.
 * Chunks stay independent: nothing is fetched from a neighbouring chunk, so rows keep not depending on how calls batch the
 * chunks.  The sign is that of the delays above: a stream that is late by d samples (fxc_estimate_delays(..) * rate == +d) takes
 * s = +d, so s_a = rint(tau_a * bandwidth).  DC removal subtracts the mean of the chunk's num_samp delivered samples, as without
 * shifts, before the shift; the fill is exact zeros.  The zero fill costs baseline (a,b) the amplitude factor of about
 *   1 - |s_a - s_b| / num_samp.
 * With the whole samples applied to the stream the tables must keep only the rest.  Natural bin order, float64, kk the integer
 * bin index of fftfreq, f_k = kk*df + frequency:
 *   u = f_k*tau - rint(f_k*tau),   m = (kk*s) mod nchan (non-negative, exact in integers),   v = u - m/nchan,
 *   r[k] = exp(2*pi*i*(v - rint(v))):
 * the full table of tau without the baseband slope kk*s/nchan turns the shift has undone; the carrier term frequency*tau stays.
 * fxc_set_sample_delays: static shifts, shift_samples = [n_ant]; NULL or all zeros removes them, and the plan then launches
 * exactly the kernels it launches without this call.  The tables stay the caller's (fxc_set_rot / fxc_set_rot_ant with the
 * table above); the shifts are independent of those calls, survive them and survive a plain fxc_set_delay_track.  It synchronises
 * the plan's stream and, like fxc_set_rot_ant, may be called while a pipe uses the plan (it applies to the batches submitted
 * afterwards).  FXC_ERR_ARG: NULL plan, |s| >= num_samp.  FXC_ERR_STATE: a non-zero shift while an aligned track is in force.
 * FXC_ERR_UNSUPPORTED: num_samp > 2^27.
 * fxc_set_delay_track_aligned: fxc_set_delay_track plus, for every chunk t, the shifts
 *   s_a(t) = llrint(tau_a(t) * bandwidth)   (tau_a(t) rounded as in the tables; ties to even, as numpy's rint)
 * and the tables above with s = s_a(t), every operation rounded on its own, ending in sincospi.  The alignment of chunk t and the
 * table of chunk t read the same integer from one device array, written once per pass.  |s_a(t)| >= num_samp is no error: that
 * stream is all zeros.  It clears static shifts; arguments, errors, gain tracks (fxc_set_track_gains), fxc_delay_track_seek, the
 * chunk counter and fxc_delay_track_tables (which returns the aligned tables) behave as under a plain track, and whatever ends a
 * track ends it; a plain fxc_set_delay_track ends the aligned behaviour and keeps a track.
 * fxc_sample_delays: the shifts chunk `chunk` gets, shift_samples_out = [n_ant]: the static shifts whatever the chunk, the
 * track's under an aligned track, all zeros when none are set.  FXC_ERR_ARG: a NULL argument, chunk < 0.
 * How it runs, and what it costs: every call that takes antennas' samples (fxc_fx_rows*, fxc_fx_accumulate*, pipes) goes in
 * passes; a pass is conditioned as its format asks (bytes converted, complex128 narrowed, DC removed: the kernels of plans
 * without shifts, unchanged) and then copied once, shifted, into a buffer of the plan (never in place; the fused byte ingest is
 * off for such plans).  A complex64 sample that was read once (8 bytes) is additionally read and written once: about 3 x the
 * sample traffic at the headline shape (derived, not measured).  Reading at an offset inside the F kernels is the follow-up that
 * removes that cost.  fxc_beamform on a plan with shifts or an aligned track returns FXC_ERR_UNSUPPORTED (its passes are not
 * aligned; it forms no unaligned beams silently); fxc_beamform_ex with align = 1 aligns them.  fxc_channelize, fxc_estimate_delay(s), fxc_remove_dc and fxc_convert_u8 take
 * streams, not antennas, and are untouched. */
int fxc_set_sample_delays(fxc_plan* plan, const int64_t* shift_samples);
int fxc_set_delay_track_aligned(fxc_plan* plan, const double* tau0_s, const double* rate_s_per_chunk, double bandwidth,
                                double frequency, int64_t first_chunk);
int fxc_sample_delays(const fxc_plan* plan, int64_t chunk, int64_t* shift_samples_out);

/* F-stage only — replaces cusignal.filtering.channelize_poly + .T at effex.py:553 (and the
 * complex128 copy at :551).  x = [n_streams][num_samp] complex64, out = [n_streams][n_pts][nchan]
 * complex64, natural (un-shifted) bin order; trailing num_samp mod nchan samples ignored; zero
 * PFB history at the start of every stream. */
int fxc_channelize(fxc_plan* plan, const void* x, void* out, int64_t n_streams, int mem_kind);

/* F+X, integrate — replaces effex.py:508-521 for a batch of chunks: x = [n_chunks][n_ant][num_samp]
 * complex64.  Adds sum_chunks sum_i spec_a[i,k]*conj(spec_b[i,k]) (natural bin order, no rot, no
 * scale) into the plan's float64 accumulator [n_baselines][nchan], baselines ordered
 * (0,1),(0,2)..(A-2,A-1), and n_chunks*n_pts into its spectra counter. */
int fxc_fx_accumulate(fxc_plan* plan, const void* x, int64_t n_chunks, int mem_kind);

/* F+X, one visibility row per chunk — the reference's literal _run_task() output (effex.py:490-527):
 *   SPECTRUM : out = [n_chunks][n_baselines][nchan] complex64 = fftshift(mean_i(f_a*conj(f_b*rot)))
 *   CONTINUUM: out = [n_chunks][n_baselines] complex128      = mean_k(that) / bandwidth  (:523-524)
 * `out` has the same mem_kind as `x` (or is pinned host memory: FXC_MEM_DEVICE_TO_PINNED). */
int fxc_fx_rows(fxc_plan* plan, const void* x, void* out, int64_t n_chunks, int mem_kind, int mode,
                double bandwidth);

/* Accumulator access for the multi-GPU reduce.  fxc_acc_export writes
 * [n_baselines*nchan] complex128 raw sums followed by one complex128 whose real part is the
 * spectra count into device memory `sums_dev` (n_baselines*nchan + 1 complex128); the host sums
 * those buffers across ranks (torch.distributed / RCCL all-reduce) and hands the result to
 * fxc_finalize_sums on the root. */
int fxc_acc_reset(fxc_plan* plan);
int fxc_acc_export(fxc_plan* plan, void* sums_dev);
/* sums_dev == NULL: the plan's own copy, as fxc_reduce leaves it (FXC_ERR_STATE if fxc_reduce has not run) */
int fxc_finalize_sums(fxc_plan* plan, const void* sums_dev, void* out_host, int mode, double bandwidth);

/* The reduce itself: export the plan's accumulator and sum it over the ranks of `rccl_comm`
 * (made by fxc_comm_create; NULL = single rank) with one ncclReduce to `root` (root < 0: ncclAllReduce), float64, in place, on
 * the plan's stream -- no host synchronisation between the F+X kernels, the collective and fxc_finalize_sums(plan,
 * NULL, ...) on the root.  64 KiB for two antennas; latency-bound over xGMI.
 * fxc_comm_*: the communicator for it.  Rank 0 calls fxc_comm_unique_id and hands the FXC_COMM_ID_BYTES bytes to
 * every rank by any channel (bench.py: torch.distributed broadcast); every rank then calls fxc_comm_create (blocking,
 * collective: ncclCommInitRank on `device`).  librccl is bound at run time; FXC_ERR_COMM if it cannot be.
 * fxc_reduce refuses (FXC_ERR_ARG, nothing queued) a communicator made on another device than the plan's, and a root
 * outside its world: a collective entered on the wrong device leaves the other ranks waiting in theirs. */
#define FXC_COMM_ID_BYTES 128
int fxc_comm_unique_id(void* id_out);
int fxc_comm_create(void** rccl_comm_out, int device, int rank, int world_size, const void* id);
int fxc_comm_destroy(void* rccl_comm);
int fxc_reduce(fxc_plan* plan, void* rccl_comm, int root);

/* What a communicator says about itself, so that a multi-GPU result can carry the proof of the ranks RCCL saw (the
 * reference has no counterpart: its chunks are merely independent, effex.py:391-410).  *_seen are asked of the live
 * ncclComm_t (ncclCommCount / ncclCommUserRank / ncclCommCuDevice; -1 where the bound RCCL lacks the query), *_given are
 * the arguments fxc_comm_create was called with; rccl_version = ncclGetVersion (e.g. 22105); async_error =
 * ncclCommGetAsyncError (0 = ncclSuccess); reduces = collectives fxc_reduce has queued on this communicator.
 * fxc_comm_probe (collective, blocking): one ncclAllReduce in which every rank contributes 1.0 -- *ranks_summed is the
 * number of ranks RCCL itself added up; FXC_ERR_COMM if their rank numbers do not add up to 1 + ... + n.
 * fxc_rccl_version: the version and (path_out, may be NULL) the file name of the librccl that was bound at run time. */
typedef struct fxc_comm_desc {
    int32_t ranks_seen, rank_seen, device_seen;
    int32_t world_given, rank_given, device_given;
    int32_t rccl_version, async_error;
    int64_t reduces;
} fxc_comm_desc;
int fxc_comm_info(void* rccl_comm, fxc_comm_desc* info);
int fxc_comm_probe(void* rccl_comm, int64_t* ranks_summed);
int fxc_rccl_version(int* version, char* path_out, int path_bytes);

/* Single-GPU finalize: mean over everything accumulated, times conj(rot), fftshift; D2H.
 *   SPECTRUM : out_host = [n_baselines][nchan] complex128;  CONTINUUM: [n_baselines] complex128.
 * Waits for the result.  reset != 0 clears the accumulator afterwards.  = fxc_finalize_async + fxc_finalize_wait. */
int fxc_finalize(fxc_plan* plan, void* out_host, int mode, double bandwidth, int reset);

/* The same without the wait: the finalize is queued on the plan's stream -- on the 2-antenna fast paths as part of
 * the kernel that folds the last fx_accumulate call's partial sums into the accumulator: fold, mean, conj(rot),
 * fftshift, reset and the write into pinned host memory are one launch -- and the call returns.  The caller may queue
 * the next integration (fxc_fx_accumulate ...) before it collects the result with fxc_finalize_wait, which blocks on
 * that result's event only.  Up to two results may be outstanding (FXC_ERR_STATE beyond that, and from the blocking
 * finalize calls while any is); they are collected in the order they were queued.
 * fxc_finalize_sums_async: the multi-GPU form (sums as for fxc_finalize_sums; the accumulator is not touched). */
int fxc_finalize_async(fxc_plan* plan, int mode, double bandwidth, int reset);
/* fxc_finalize_async with the destination named up front: the result is delivered into out_host (same layout as
 * fxc_finalize) by the device -- written by the finishing kernel itself when it is small and out_host lies in
 * fxc_host_alloc memory, by the side-stream copy when it is large (28 baselines and more: a direct DMA into pinned memory) --
 * so that fxc_finalize_wait(plan, out_host or NULL) only waits: with 496 baselines of 4 096 bins the copy out of the plan's
 * slot is 32 MB of host memcpy per integration, more than the integration's kernels take.  The buffer must stay valid until
 * the wait returns. */
int fxc_finalize_async_to(fxc_plan* plan, void* out_host, int mode, double bandwidth, int reset);
int fxc_finalize_sums_async(fxc_plan* plan, const void* sums_dev, int mode, double bandwidth);
int fxc_finalize_wait(fxc_plan* plan, void* out_host);
int fxc_finalize_pending(const fxc_plan* plan); /* results queued and not yet collected */

int fxc_sync(fxc_plan* plan);

/* Input conditioning, device resident (both are steps the reference runs on the host
 * just before the path).  Streams are [n_streams][num_samp] with the plan's num_samp; n_streams <= 65535.
 *   fxc_remove_dc : out = x - mean(x) per stream, real and imaginary parts separately — effex.py:394-395
 *                   (complex64 in, complex64 out; out may alias x; means formed in float64).
 *   fxc_convert_u8: RTL-SDR interleaved unsigned 8-bit I,Q -> complex64 (byte - 127.5) / 127.5, what
 *                   pyrtlsdr does for sdr.stream(format='samples') (effex.py:652); with remove_dc != 0 the
 *                   per-stream mean is removed in the same pass from exact integer byte sums. */
int fxc_remove_dc(fxc_plan* plan, const void* x_dev, void* out_dev, int64_t n_streams);
int fxc_convert_u8(fxc_plan* plan, const void* iq_u8_dev, void* out_dev, int64_t n_streams, int remove_dc);

/* F+X straight from the RTL-SDR byte stream: iq_u8 = [n_chunks][n_ant][num_samp] interleaved unsigned 8-bit I,Q
 * (2 bytes per sample), converted as fxc_convert_u8 does (remove_dc != 0: per-stream mean removed, effex.py:394-395)
 * and then processed exactly like fxc_fx_rows / fxc_fx_accumulate.  On fused plans (2 antennas, nchan 4096, ntaps 4)
 * the F+X kernel loads the bytes itself -- a quarter of the complex64 stream's HBM traffic, no intermediate copy;
 * other plans convert into a staging buffer first.  Replaces, for byte sources, the chain pyrtlsdr conversion
 * (effex.py:652) -> host DC removal (effex.py:394-395) -> cp.array copies (effex.py:508-509) -> _pfb_xcorr. */
int fxc_fx_rows_u8(fxc_plan* plan, const void* iq_u8, void* out, int64_t n_chunks, int mem_kind, int mode,
                   double bandwidth, int remove_dc);
int fxc_fx_accumulate_u8(fxc_plan* plan, const void* iq_u8, int64_t n_chunks, int mem_kind, int remove_dc);

/* The same two calls for any sample format, with the per-chunk DC removal of effex.py:394-395 on the device:
 * x = [n_chunks][n_ant][num_samp] samples of `iq_format` (fxc_iq_format); remove_dc != 0 subtracts, per chunk and antenna,
 * the mean of the real and of the imaginary parts (float64 sums) before the path.  FXC_IQ_U8 = fxc_fx_rows_u8;
 * FXC_IQ_C64 with remove_dc == 0 = fxc_fx_rows.  complex64 / complex128 with DC removal run the sums and the subtraction
 * (complex128: subtraction in float64, then one rounding to complex64) as a pre-pass -- in place on the library's own
 * staging copy for host buffers, into a staging buffer for device buffers (the caller's samples are never written).
 * Replaces the host lines effex.py:394-395 (+ the narrowing copy of a complex128 source) in front of _pfb_xcorr. */
int fxc_fx_rows_iq(fxc_plan* plan, const void* x, void* out, int64_t n_chunks, int mem_kind, int mode, double bandwidth,
                   int iq_format, int remove_dc);
int fxc_fx_accumulate_iq(fxc_plan* plan, const void* x, int64_t n_chunks, int mem_kind, int iq_format, int remove_dc);

/* Pinned host memory for FXC_MEM_HOST buffers -- the counterpart of the reference's mapped pinned staging buffers
 * (cusignal.get_shared_mem, effex.py:109-110).  Buffers from fxc_host_alloc cross PCIe by direct DMA (pageable memory goes
 * through the runtime's bounce buffers at about half the rate), and an `out` buffer inside such an allocation is written by
 * the finishing kernel itself through the device's mapping of it: no copy back.  Any host pointer is still accepted
 * everywhere; these only make it fast.  fxc_host_free(NULL) is a no-op; FXC_ERR_ARG for a pointer fxc_host_alloc did not
 * return.  Process-wide, thread-safe; the memory is usable with every device. */
int fxc_host_alloc(void** out, int64_t bytes);
int fxc_host_free(void* ptr);

/* Delay calibration — replaces Correlator._estimate_delay_gaussian, effex.py:583-627:
 * zero-pad both streams, FFT, f0*conj(f1), inverse FFT, arg-max of |xcorr|, 3-point log-Gaussian peak;
 * *delay_s = (n - (imax + delta)) / rate.  iq0, iq1: n complex64 samples each (host or device), any n.
 * Uses the plan's device, stream and workspace; synchronises. */
int fxc_estimate_delay(fxc_plan* plan, const void* iq0, const void* iq1, int64_t n, int mem_kind, double rate,
                       double* delay_s);

/* Delay calibration of the whole array in one call: x = [n_ant][n] complex64 (host or device, mem_kind as above), delays_s[n_ant]
 * out.  delays_s[a] is bit for bit fxc_estimate_delay(plan, x[ref], x[a], n, mem_kind, rate) and delays_s[ref] = 0.0, so
 * per-antenna tables of these delays (fxc_set_rot_ant) remove the delay slope of every baseline.  The reference stream is
 * transformed once and the others in batches as large as the workspace target allows; one copy to the host, one
 * synchronisation.  FXC_ERR_ARG: a NULL argument, n_ant < 2, ref outside [0, n_ant), n or rate outside the ranges of
 * fxc_estimate_delay. */
int fxc_estimate_delays(fxc_plan* plan, const void* x, int64_t n, int mem_kind, double rate, int ref, double* delays_s);

/* Fringe fit: the residual delay and delay rate of every antenna against antenna `ref`, from the SPECTRUM rows of n_chunks
 * consecutive chunks -- the measurement that fxc_set_delay_track's rate_s_per_chunk needs.
 * rows = [n_chunks][n_rows][nchan] complex64, host or device (mem_kind), exactly what fxc_fx_rows(.., FXC_MODE_SPECTRUM) writes:
 * fftshifted bins, n_rows as fxc_plan_products reports; auto rows are ignored.  For every antenna b != ref:
 *   R[t][j]  = row (ref, b) of chunk t if ref < b, else the complex conjugate of row (b, ref); bin j has the frequency
 *              frequency + fftshift(fftfreq(nchan, 1/bandwidth))[j]: monotonic, spacing bandwidth / nchan;
 *   Lk, Lt   = the smallest powers of two >= pad * nchan, >= pad * n_chunks;
 *   F[q][m]  = sum_t sum_j R[t][j] exp(-2*pi*i*(j*m/Lk + t*q/Lt)), the zero-padded forward 2-D DFT;
 *   (q0, m0) = arg-max of |F|, the first maximum in row-major (q, m) order (numpy.argmax);
 *   dm, dq   = 0.5 (ln a - ln c) / (ln a - 2 ln b + ln c), a, b, c = |F| at index -1, 0, +1 along m and along q, indices
 *              wrapping (the three-point log-parabola of fxc_estimate_delay, effex.py:619-625);
 *   with m, q = m0, q0 as signed indices (m0 - Lk for m0 >= Lk/2, likewise q0):
 *   delay_s[b]          = (m + dm) * nchan / (Lk * bandwidth)
 *   rate_s_per_chunk[b] = (q + dq) / (Lt * frequency)
 *   snr[b]              = |F[q0][m0]| / sqrt(sum_t sum_j |R[t][j]|^2): the peak over the root-mean-square of |F| on the whole
 *                         padded grid (Parseval); pure noise gives about sqrt(ln(n_chunks * nchan)).
 * delay_s[ref] = rate_s_per_chunk[ref] = snr[ref] = 0.  The three outputs are host double[n_ant]; snr may be NULL.
 * Sign: rows made with the delays tau_used of a signal whose true delays are tau_true have R_ab[t][k] proportional to
 * exp(+2*pi*i*f_k*(D_b(t) - D_a(t))), D = tau_true - tau_used (row (a,b) is raw_ab r_a conj(r_b)).  The fit returns D_b - D_ref:
 * fxc_set_delay_track(tau0 + delay_s, rate + rate_s_per_chunk, ..) stops the fringes.
 * Limits: |delay| < nchan / (2 bandwidth) and |rate| < 1 / (2 frequency) per chunk are the unambiguous ranges.  The search takes
 * the fringe rate to be the same in every bin (f_k ~ frequency in the time term), which neglects the delay drift over the scan,
 * |rate| * n_chunks * bandwidth samples: n_chunks * bandwidth / (2 frequency) at the rate limit, 0.2 sample for 256 chunks at
 * 2.4 MHz / 1.4204 GHz.  Only the n_ant - 1 baselines to `ref` are used, and every sample as it stands; weights, and the
 * least-squares solution over all baselines: fxc_fringe_fit_weighted below.
 * The |F|^2 of the search is formed in float32 and never written out; the five values of the two parabolas are summed again in
 * float64.  The baselines go through in batches as large as the workspace target allows, and no value depends on the batching.
 * Uses the plan's device, stream and workspace; synchronises like fxc_estimate_delays; neither reads nor changes the rot tables,
 * the track or its counter.
 * FXC_ERR_ARG, before any device work: a NULL plan / rows / delay_s / rate_s_per_chunk, n_ant < 2, ref outside [0, n_ant),
 * n_chunks < 2, pad not 1, 2, 4 or 8, bandwidth or frequency <= 0 or not finite, an unknown mem_kind.
 * FXC_ERR_UNSUPPORTED: Lt > 4096, Lk > 65536, nchan == 1.  The outputs are written on FXC_OK only. */
int fxc_fringe_fit(fxc_plan* plan, const void* rows, int64_t n_chunks, int mem_kind, double bandwidth, double frequency,
                   int ref, int pad, double* delay_s, double* rate_s_per_chunk, double* snr);

/* Fringe fit with weights, over the baselines to `ref` or by least squares over all baselines: fxc_fringe_fit for
 * rows that the detector (fxc_flag_rows) has been over, and for arrays whose baseline to `ref` may be missing.
 * rows is as for fxc_fringe_fit.  weights = [n_chunks][n_baselines][nchan] float32 in the memory kind of rows, the layout of
 * fxc_solve_gains_weighted and fxc_flag_rows; NULL: no buffer is read and every weight is 1.
 * A sample counts iff its weight w > 0: a zero, negative or NaN weight leaves it out.  With (x, y) the sample,
 *   Rw[t][j] = (w x, w y) if w > 0, else (+0, +0): float32 products, one rounding each, so that w = 1.0f gives R exactly.
 * What a sample that does not count holds is never used: NaN, Inf or 1e30 there changes no output bit.  A counted value that is
 * not finite propagates.
 * The fit of one baseline is fxc_fringe_fit's, term for term, with Rw for R: Lk, Lt, the padded 2-D DFT F, the first arg-max
 * (q0, m0), the two log-parabolas dm and dq, delay = (m + dm) nchan / (Lk bandwidth), rate = (q + dq) / (Lt frequency) and
 * snr = |F[q0][m0]| / sqrt(sum_t sum_j |Rw[t][j]|^2).  The power sum is float64 in the order of fxc_fringe_fit: 128 fixed
 * partial sums per baseline, added on the host in order.  A baseline whose power sum is 0 -- nothing counted -- gets delay 0,
 * rate 0 and snr 0; its peak is not used (fxc_fringe_fit itself divides by the sum).  One term is added: with weights given,
 * the magnitudes a, b, c of the two log-parabolas are divided by 2^e, e = floor(log2(the largest counted weight of the baseline)),
 * before the logarithms -- exact, and e = 0 for weights of 1.  With it, multiplying every weight by the same power of two changes
 * no output bit, barring overflow and underflow (ln(4 a) and ln(a) round differently; snr is a ratio and needs no such term).
 * baselines = FXC_FRINGE_REF: the baselines to `ref` are fitted, conjugated where b < ref, and delay_s, rate_s_per_chunk and snr
 *   are as fxc_fringe_fit defines them; min_snr must be 0.  With NULL weights, or with every weight 1.0f, the three outputs are
 *   fxc_fringe_fit's bit for bit.  base_out (when given) holds (delay, rate, snr) of every fitted baseline at its row index, as
 *   row (lo, hi) reads -- not conjugated: the estimate of D_hi - D_lo --, and 0 in every other row.
 * baselines = FXC_FRINGE_ALL: every cross row i = (a, b), a < b, is fitted as it stands: base[i] = (d_i, r_i, s_i), the
 *   estimates of D_b - D_a, which base_out receives.  Then on the host, in float64:
 *   used     baseline i is used iff s_i >= T; T = min_snr if min_snr > 0, else T = sqrt(ln(Lk Lt) + ln(1000)): |F|^2 / sum |Rw|^2
 *            is exponential with mean 1 in each of the Lk Lt cells of noise alone (padding makes the count of independent cells
 *            an over-estimate), so a baseline of noise is used with a probability of 1e-3 at most.  T = 3.99 at Lk 128, Lt 64.
 *   tree     from {ref}: again and again the used baseline of largest s that joins a reached antenna to one not reached (ties:
 *            the lowest row index) is added, and the new antenna's D0, R0 are the reached end's plus or minus (d_i, r_i).
 *            Antennas never reached get delay, rate and snr 0.
 *   unwrap   with the periods Pd = nchan / bandwidth and Pr = 1 / frequency (a baseline measures a difference modulo the period),
 *            every used baseline between reached antennas takes d_i += Pd nearbyint((D0_b - D0_a - d_i) / Pd), r_i likewise with Pr.
 *   solve    minimise sum_i s_i^2 (D_b - D_a - d_i)^2 over the reached antennas, D_ref = 0, and the same for the rates: the
 *            normal equations are formed in ascending row order and solved by Cholesky.
 *            snr[a] = sqrt(sum of s_i^2 over the used baselines between reached antennas that touch a); snr[ref] = 0.
 *            Each result is wrapped into the principal range, x - P nearbyint(x / P).
 *   For baselines of equal sensitivity the solution has sqrt(2 / n_ant) of the error of the baselines to `ref`, and an antenna
 *   whose baseline to `ref` is flagged is still measured through the others.
 * delay_s, rate_s_per_chunk and snr are host double[n_ant] (snr may be NULL); base_out is host double[n_baselines][3] and may
 * be NULL.  Limits: those of fxc_fringe_fit per baseline; n_ant <= 64 (2016 baselines); fringes too weak for any single baseline
 * are not found (no coherent search across baselines); the auto rows are not used.
 * The baselines go through in batches as large as the workspace target allows, host rows and host weights staged baseline by
 * baseline; no bit of base_out or of the three outputs depends on the batches, the workspace target, or host against device
 * input.  Uses the plan's device, stream and workspace; one copy to the host and one synchronisation end the call; neither reads
 * nor changes the rot tables, the tracks or their counters.
 * FXC_ERR_ARG, before any device work: every case of fxc_fringe_fit; baselines neither FXC_FRINGE_REF nor FXC_FRINGE_ALL; min_snr
 * negative or not finite, or not 0 with FXC_FRINGE_REF.  FXC_ERR_UNSUPPORTED: the cases of fxc_fringe_fit.  The outputs are
 * written on FXC_OK only. */
#define FXC_FRINGE_REF 0
#define FXC_FRINGE_ALL 1
int fxc_fringe_fit_weighted(fxc_plan* plan, const void* rows, const void* weights, int64_t n_chunks, int mem_kind,
                            double bandwidth, double frequency, int ref, int pad, int baselines, double min_snr,
                            double* delay_s, double* rate_s_per_chunk, double* snr, double* base_out);

/* Gain solve: every antenna's complex gain per bin from the SPECTRUM rows of n_chunks consecutive chunks of a point source at
 * the phase centre (a calibrator; model visibility 1), by least squares over ALL baselines -- what is left
 * after fxc_estimate_delays / fxc_fringe_fit: the bandpass amplitudes and the residual phases.
 * rows = [n_chunks][n_rows][nchan] complex64, host or device (mem_kind), exactly what fxc_fx_rows(.., FXC_MODE_SPECTRUM) writes:
 * fftshifted bins, n_rows as fxc_plan_products reports.  Only the first n_baselines rows of a chunk are read: auto rows are
 * skipped.  Row (a,b), a < b, in the baseline order of the results, is modelled as g_a conj(g_b).
 * Solution intervals: with L = interval (0: L = n_chunks), interval s covers the chunks [s L, min((s + 1) L, n_chunks)) and
 * n_int = ceil(n_chunks / L).  Per interval and per bin k:
 *   V_ab     = the sum of the interval's rows (a,b), added in float64 one chunk after the other in ascending chunk order (plain
 *              adds from 0, real and imaginary parts apart), then each part divided by the number of chunks; V_ba = conj(V_ab);
 *              the diagonal is not used;
 *   start      s = mean over b != ref (b ascending) of |V_b,ref|; g_ref = sqrt(s), g_a = V_a,ref / sqrt(s); all 0 where s == 0;
 *   for it = 1 .. iters (Salvini & Wijnholds' StefCal with model visibility 1; every a from the g of the iteration before):
 *              n_a = sum over b != a of V_ab g_b and d_a = sum over b != a of |g_b|^2, b ascending;
 *              new_a = n_a / d_a, 0 where d_a == 0; on even it new = (new + g) / 2;
 *              step = sqrt(sum_a |new_a - g_a|^2 / sum_a |new_a|^2), a ascending, 0 for a zero denominator; g = new;
 *   end        with u = conj(g_ref) / |g_ref|: g_a = g_a u for a != ref and g_ref = |g_ref|, real and non-negative (nothing
 *              changes where g_ref == 0).
 * gains_re_im = [n_int][n_ant][nchan] complex128 and step = [n_int][nchan] float64 (the last iteration's value; may be NULL),
 * host memory, bins in the rows' order.  iters is a count, not a convergence test: the map from rows to gains is fixed, and
 * step says how far the iteration got (it converges fast from 8 antennas on, slowly at 3 .. 5).  Everything after the sum is
 * float64.  fxc_set_rot_ant with r_a = ifftshift(1 / g_a) then makes the rows of the same signal 1.
 * Host rows are staged through the workspace in batches and the intervals solved in groups, both sized by the workspace
 * target; a batch continues the sums of the one before it, so no bit of the outputs depends on the sizes, and host and device
 * rows give the same bits.  Uses the plan's device, stream and workspace; synchronises like fxc_fringe_fit (one copy to the
 * host and one synchronisation end the call); neither reads nor changes the rot tables, the track or its counter.
 * Under a delay track fxc_set_track_gains applies every solution, interval by interval.
 * A sky model other than a point source at the phase centre, weights and flags: fxc_solve_gains_weighted below.  Not covered:
 * two antennas.
 * FXC_ERR_ARG, before any device work: a NULL plan / rows / gains_re_im, n_chunks < 1, interval < 0, ref outside [0, n_ant),
 * iters outside 1 .. 1000, an unknown mem_kind.  FXC_ERR_UNSUPPORTED: fewer than 3 antennas (one baseline closes nothing).
 * The outputs are written on FXC_OK only. */
int fxc_solve_gains(fxc_plan* plan, const void* rows, int64_t n_chunks, int mem_kind, int64_t interval, int ref, int iters,
                    double* gains_re_im /* [n_int][n_ant][nchan] complex128, bins in the rows' order */,
                    double* step        /* [n_int][nchan], may be NULL */);

/* Weighted gain solve: fxc_solve_gains with a weight per sample (a weight that is not > 0 flags the sample) and a model
 * visibility per baseline and bin -- for data with dropped chunks, narrow-band interference or a dead antenna,
 * and for a calibrator that is resolved or away from the phase centre.
 * rows = [n_chunks][n_rows][nchan] complex64 as for fxc_solve_gains; only the first n_baselines rows of a chunk are read.
 * weights = [n_chunks][n_baselines][nchan] float32 in the memory kind of rows: cross rows only, with no room for auto rows also
 * on a plan with autos, bins in the rows' fftshifted order; NULL: every weight is 1 (no buffer is read).  A sample counts iff
 * w > 0: a zero, negative or NaN weight flags it.  Positive weights must be finite (stated, not checked).
 * model = [n_model][n_baselines][nchan] complex64 HOST memory in the rows' order; n_model is 1 (one model for every interval) or
 * n_int; NULL with n_model 0: model visibility 1.  Model values must be finite (checked on the host); a zero is allowed and takes
 * that baseline out of that bin.
 * Per interval (as in fxc_solve_gains; n chunks in the interval) and per bin:
 *   S_ab     = sum over the chunks c of [w_c > 0 ? (double)w_c (double)v_c : 0] and Sw_ab = sum of [w_c > 0 ? (double)w_c : 0]:
 *              real and imaginary parts apart, plain adds from 0 in ascending chunk order.  The product of two float32 values is
 *              exact in float64, so the sums have one value whether or not the compiler contracts.  The VALUE of a flagged
 *              sample is never used: NaN, Inf or 1e30 there changes no output bit;
 *   A_ab     = S_ab / n and Wbar_ab = Sw_ab / n, each part divided;
 *   U, D       without a model U_ab = A_ab and D_ab = Wbar_ab exactly; with a model M converted to float64
 *              U_ab = A_ab conj(M_ab) and D_ab = Wbar_ab (Mx^2 + My^2); U_ba = conj(U_ab), D_ba = D_ab; the diagonal is not used;
 *   start      Vhat_b = U_b,ref / D_b,ref where D_b,ref != 0; s = the mean of |Vhat_b| over those b != ref, b ascending;
 *              g_ref = sqrt(s), g_a = Vhat_a / sqrt(s) where D_a,ref != 0, else 0; all 0 where s == 0 or no such b exists: a
 *              bin whose reference antenna carries no weight is not solved;
 *   for it = 1 .. iters (every a from the g of the iteration before, b != a ascending):
 *              n_a = sum of U_ab g_b and d_a = sum of D_ab |g_b|^2; new_a = n_a / d_a, 0 where d_a == 0; on even it
 *              new = (new + g) / 2; step, g = new and the final rotation to a real non-negative g_ref exactly as in
 *              fxc_solve_gains.
 * With unit weights and no model this is fxc_solve_gains' definition term for term.  An antenna whose baselines all carry
 * zero weight gets g = 0 and takes no part in the other antennas' sums (fxc_set_track_gains then zeroes its rows).  Multiplying
 * all weights by a power of two changes no output bit.
 * Host rows and weights are staged through the workspace in batches, the intervals solved in groups and the model uploaded once
 * per group, all sized by the workspace target; no output bit depends on the sizes, and host and device input give the same
 * bits.  Uses the plan's device, stream and workspace; synchronises like fxc_solve_gains; neither reads nor changes the rot
 * tables, the tracks or their counters.
 * FXC_ERR_ARG, before any device work: every case of fxc_solve_gains; model and n_model disagree (one NULL / 0 without the
 * other); n_model neither 1 nor n_int; a model value that is not finite.  FXC_ERR_UNSUPPORTED: fewer than 3 antennas.
 * The outputs are written on FXC_OK only. */
int fxc_solve_gains_weighted(fxc_plan* plan, const void* rows, const void* weights, int64_t n_chunks, int mem_kind,
                             const void* model, int64_t n_model, int64_t interval, int ref, int iters,
                             double* gains_re_im /* [n_int][n_ant][nchan] complex128, bins in the rows' order */,
                             double* step        /* [n_int][nchan], may be NULL */);

/* Detector: the weights fxc_solve_gains_weighted takes, from the rows alone -- samples that stand out of their
 * (baseline, bin) column in time, and bins that stand out of their neighbours in frequency, get weight 0.
 * rows = [n_chunks][n_rows][nchan] complex64 as for fxc_solve_gains, exactly what fxc_fx_rows(.., FXC_MODE_SPECTRUM) writes, with
 * the fringes stopped (a complex median means nothing on a rotating phasor); only the first n_baselines rows of a chunk are
 * read: auto rows are skipped.  prior = [n_chunks][n_baselines][nchan] float32 in the memory kind of rows, or NULL.  weights has
 * fxc_solve_gains_weighted's layout: cross rows only, no room for auto rows.
 * Windows: with L = window (0: L = n_chunks), window s covers the chunks [s L, min((s + 1) L, n_chunks)) and n_win =
 * ceil(n_chunks / L).  Everything below is per window, per baseline b and, where it says so, per bin k.
 * Lower median of m values: the element at index (m - 1) / 2 (rounded down) of their ascending order -- an element of the set,
 * no arithmetic.
 * Live at the start: a sample (x, y) is live iff x and y are finite, not both zero (an exactly zero row is a dropped chunk), and
 * prior is NULL or its value is > 0.  The VALUE of a sample that is not live is never used.
 * Time stage, per column (b, k), `iters` times over the column's live samples (nothing happens once none is live):
 *   mx, my   = the lower medians of x and of y;
 *   dx, dy   = x - mx and y - my, each ONE float32 subtraction;
 *   e        = (float)((double)dx (double)dx + (double)dy (double)dy): the products are exact in float64, so the sum has one value
 *              whether or not the compiler contracts; then one rounding to float32;
 *   d        = the lower median of e; where d > 0 a live sample is flagged iff e > time_threshold d (one float32 multiply and a
 *              comparison; an infinite e compares like any value); where d == 0 nothing is flagged.
 * Column statistics: after the iterations a column with a live sample is "defined" and gets, over its survivors, mx, my and e
 * as above, level[k] = (float)((double)mx mx + (double)my my) and scatter[k] = the lower median of e.
 * Frequency stage, per baseline, every decision from the level, scatter and defined-ness the time stage left, before any bin is
 * cleared.  For a defined bin k take the defined bins j with |j - k| <= half_width, 0 <= j < nchan (k among them); for S in
 * {level, scatter}: r = the lower median of S[j] and s = the lower median of |S[j] - r| (a float32 subtraction, then the absolute
 * value).  Level test: k is an outlier iff s > 0 and |level[k] - r| > freq_threshold s (two-sided: a dead bin as well as a
 * tone).  Scatter test: iff s > 0 and scatter[k] - r > freq_threshold s (the high side only).  An outlier bin has all its samples
 * of the window flagged.  One pass: the neighbours' medians are not recomputed without the outliers.
 * Output: a sample that is live at the end gets the prior's value where a prior was given, else 1.0f; every other sample
 * +0.0f.  counts[s][b] = {not live at the start, flagged by the time stage, still live when the frequency stage flagged them}.
 * The thresholds are multiples of the median deviation, not sigmas: for complex Gaussian scatter the median of e is ln 2 sigma^2,
 * so time_threshold 20 is e > 13.9 sigma^2.
 * No output depends on what a non-live sample holds; permuting the chunks of a window permutes the weights and changes nothing
 * else; multiplying all rows by a power of two changes no output (barring overflow and underflow; float32 denormals are kept);
 * no output depends on batching, the workspace size or host against device input.  Host rows and the prior are staged through
 * the workspace in slabs of whole baselines of one window and a slab's weights copied back.  Uses the plan's device, stream and
 * workspace; synchronises like fxc_solve_gains; neither reads nor changes the rot tables, the tracks or their counters.  Works
 * from one baseline (2 antennas) up and at nchan 1 (where the frequency stage never fires: s is 0).
 * FXC_ERR_ARG, before any device work: a NULL plan / rows / weights, n_chunks < 1, window < 0, a threshold that is not finite or
 * not > 0, half_width < 0, iters outside 1 .. 8, an unknown mem_kind, a plan with fewer than 2 antennas.
 * FXC_ERR_UNSUPPORTED: more than 1024 chunks in a window (a column lives in LDS; larger windows are out of scope).
 * The outputs are written on FXC_OK only. */
int fxc_flag_rows(fxc_plan* plan, const void* rows, const void* prior, int64_t n_chunks, int mem_kind, int64_t window,
                  float time_threshold, float freq_threshold, int half_width, int iters,
                  void* weights   /* [n_chunks][n_baselines][nchan] float32, in the memory kind of rows */,
                  int64_t* counts /* [n_win][n_baselines][3], host, may be NULL */);

/* Averager: the weighted mean of the SPECTRUM rows over intervals of chunks and bins of channels, and the summed weights
 *  -- the integrated visibility spectrum with the flagged samples left out, the product fxc_flag_rows was added
 * for and the data-reduction step between flagging and whatever comes next.
 * rows = [n_chunks][n_rows][nchan] complex64 as for fxc_solve_gains, exactly what fxc_fx_rows(.., FXC_MODE_SPECTRUM) writes; only
 * the first n_baselines rows of a chunk are read: auto rows are skipped.  weights = [n_chunks][n_baselines][nchan] float32 in the
 * memory kind of rows (fxc_solve_gains_weighted's and fxc_flag_rows' layout), or NULL: no weight buffer is read and every weight
 * is 1.  A sample counts iff w > 0: a zero, negative or NaN weight leaves it out.  The VALUE of a sample that does not count is
 * never used: NaN, Inf or 1e30 there changes no output bit.  A counted sample's value is used as it is: a non-finite value with
 * a positive weight, or with NULL weights, propagates (stated, not checked).
 * Intervals: with L = time_bin (0: L = n_chunks), interval s covers the chunks [s L, min((s + 1) L, n_chunks)) and n_int =
 * ceil(n_chunks / L).  Output bins: with F = freq_bin, output bin m covers the input bins [m F, min((m + 1) F, nchan)) of the
 * rows' fftshifted order, which is monotonic in frequency; n_out = ceil(nchan / F), the last bin may be partial.
 * Per (interval, baseline, input bin j):
 *   Sx, Sy, W  start at 0; for the interval's chunks c ascending, if w_c > 0: Sx += (double)w_c (double)x_c, Sy likewise with y_c,
 *              W += (double)w_c.  The product of two float32 values is exact in float64, so the sums have one value whether or
 *              not the compiler contracts (the argument of fxc_solve_gains_weighted).
 * Per output bin m:
 *   Tx, Ty, Wm start at 0 and add the Sx, Sy, W of its input bins with plain float64 adds, j ascending;
 *   out_rows[s][b][m]    = Wm > 0 ? ((float)(Tx / Wm), (float)(Ty / Wm)) : (+0, +0): an IEEE float64 division, one rounding to
 *                          float32;
 *   out_weights[s][b][m] = (float)Wm.
 * out_rows = [n_int][n_baselines][n_out] complex64 and out_weights = [n_int][n_baselines][n_out] float32, both in the memory
 * kind of rows; out_weights may be NULL.  At freq_bin 1 the two have exactly the layout fxc_solve_gains_weighted, fxc_flag_rows
 * (prior) and fxc_fringe_fit take on a plan without autos.
 * Multiplying all weights by a power of two changes no bit of out_rows and scales out_weights by that power (barring overflow
 * and underflow).  No output depends on batching, the workspace target or host against device input.  At freq_bin 1 with NULL
 * weights out_rows is the complex64 rounding of the V that fxc_solve_gains averages.
 * Device rows go through in launches bounded by the grid limits; host rows and weights are staged through the workspace in
 * slabs of whole baselines of one interval and a slab's outputs copied back, so every output cell belongs to one launch.  Uses
 * the plan's device, stream and workspace; synchronises like fxc_flag_rows (one synchronisation ends the call); neither reads
 * nor changes the rot tables, the tracks or their counters.  Works from one baseline (2 antennas) up and at nchan 1.
 * FXC_ERR_ARG, before any device work: a NULL plan / rows / out_rows, n_chunks < 1, time_bin < 0, freq_bin < 1, an unknown
 * mem_kind, a plan with fewer than 2 antennas.
 * FXC_ERR_UNSUPPORTED: freq_bin > 256 (one workgroup's tile holds a whole output bin; wider bins are out of scope).
 * The outputs are written on FXC_OK only. */
int fxc_average_rows(fxc_plan* plan, const void* rows, const void* weights, int64_t n_chunks, int mem_kind, int64_t time_bin,
                     int freq_bin,
                     void* out_rows    /* [n_int][n_baselines][n_out] complex64, in the memory kind of rows */,
                     void* out_weights /* [n_int][n_baselines][n_out] float32, in the memory kind of rows, may be NULL */);

/* Tied-array beamformer: phased sums of the antennas' spectra -- the other product an array with calibrated
 * per-antenna delays and gains delivers beside visibilities: the sensitivity of the whole array at full time resolution.
 * With f_a[c,i,k] antenna a's spectrum of frame i of chunk c exactly as fxc_channelize writes it (natural bin order, n_pts =
 * num_samp / nchan frames a chunk) and weights = w[b][a][k], complex64 [n_beam][n_ant][nchan] in NATURAL bin order like every
 * rot table, the beam voltage is
 *     y_b[c,i,k] = sum_{a = 0 .. n_ant-1}  w[b,a,k] * rho_a[k](t_c) * f_a[c,i,k]
 * rho comes from the plan's state.  A delay track (fxc_set_delay_track, with or without fxc_set_track_gains): rho_a[k](t) is the
 * chunk's per-antenna table exactly as fxc_delay_track_tables returns it, rounded once to complex64; the call's chunks take
 * t = the plan's counter, counter + 1, ..; the counter advances by n_chunks as in fxc_fx_rows, and a call that fails puts it
 * back.  No track: rho = 1.  The tables of fxc_set_rot and fxc_set_rot_ant are NOT applied: they are host tables, and the caller
 * folds them into w (Python: beam_weights).  The effective weight w * rho is a float32 complex product; the antennas are added
 * in index order from 0, four fused multiply-adds each.
 * mode = FXC_BEAM_POWER:   out[c][b][j][k'] float32 [n_chunks][n_beam][n_tbin][nchan] = fftshift_k(mean_{i in bin j} |y_b[c,i,k]|^2):
 *   the bins in the rows' order (k' = (k + nchan / 2) % nchan, odd counts included).  tint = frames per time bin, 0 = the whole
 *   chunk; n_tbin = ceil(n_pts / tint); the last bin may be partial and is divided by its own count.  One thread adds a bin's
 *   |y|^2 in frame order in float32 and divides once: bins of many thousands of frames carry that sum's rounding.
 * mode = FXC_BEAM_VOLTAGE: out[c][b][i][k] = y_b, complex64 [n_chunks][n_beam][n_pts][nchan], natural bin order, the layout of
 *   fxc_channelize; tint is ignored (but checked).
 * x = [n_chunks][n_ant][num_samp] complex64.  x, weights and out are all host memory (FXC_MEM_HOST: staged like the other calls,
 * synchronous) or all device memory (FXC_MEM_DEVICE: queued on the plan's stream).  The F stage of the plan runs a pass of
 * chunks into the workspace and one kernel reads every spectrum once (9 .. 16 beams: twice); the passes are sized by the
 * workspace target (FXC_WS_MB), and no output bit depends on the batch size, the workspace target or host against device
 * input.  The call does not touch the accumulator (a pending fold is launched first).
 * FXC_OK: n_chunks == 0 (nothing is read).  FXC_ERR_ARG: a NULL argument, n_beam < 1, n_chunks < 0, an unknown mode or mem_kind
 * (FXC_MEM_DEVICE_TO_PINNED included), tint < 0 or tint > n_pts.  FXC_ERR_UNSUPPORTED: n_beam > 16.  FXC_ERR_STATE: the plan has
 * a track and an fxc_pipe uses the plan.  A plan with whole-sample delays: FXC_ERR_UNSUPPORTED (fxc_beamform_ex aligns its passes).
 * Out of scope: uint8 and complex128 input, pipes, more than 16 beams, Correlator integration, bench.py. */
enum fxc_beam_mode { FXC_BEAM_POWER = 0, FXC_BEAM_VOLTAGE = 1 };
enum fxc_beam_mode_ex { FXC_BEAM_INCOHERENT = 2 };      /* the third mode, of fxc_beamform_ex alone: fxc_beamform's modes stay two */
int fxc_beamform(fxc_plan* plan, const void* x, const void* weights, int n_beam, void* out, int64_t n_chunks, int mem_kind, int mode,
                 int64_t tint);

/* fxc_beamform with an antenna mask, incoherent beams and aligned passes.  With mask == NULL, mode POWER or
 * VOLTAGE and align == 0 it is fxc_beamform: the same kernels, the same bits.  Everything fxc_beamform's contract says holds
 * here; what follows is what is added.
 * mask (may be NULL: every antenna counts) = float32 [n_chunks][n_ant][n_mbin][nchan] in the memory of x (mem_kind), channels in
 * the rows' fftshifted order k' = (k + nchan / 2) % nchan: exactly the layout fxc_kurtosis(.., tint = mask_tint) writes sk in and
 * fxc_kurtosis_antenna_mask writes the mask in.  mask_tint = frames per mask bin, 0 = n_pts, 1 .. n_pts allowed; n_mbin =
 * ceil(n_pts / mask_tint); frame i is under mask bin i / mask_tint; mask_tint and tint are independent.  Antenna a counts in a
 * cell iff its mask value is > 0 (a NaN does not count): the convention of every `weights` argument.  A sample that does not count
 * is selected away, not multiplied: a NaN, an Inf or a tone in it changes no bit of the output.
 * POWER, VOLTAGE:  y_b[c,i,k] = sum_{a counted} weff[c,b,a,k] f_a[c,i,k], weff = w * rho as in fxc_beamform; the select is made on
 *   the loaded sample, ahead of the same fused multiply-adds in the same antenna and frame order, so a mask that is > 0 everywhere
 *   gives fxc_beamform's output bit for bit.  No normalisation is written: the sum of (mask > 0) over the antennas is the count of
 *   antennas in a cell, and the caller rescales by (n_ant / count)^2 for a point source (tint == mask_tint keeps one count a bin).
 * FXC_BEAM_INCOHERENT:  out[c][b][j][k'] = mean_{i in bin j} sum_{a counted} |weff[c,b,a,k]|^2 |f_a[c,i,k]|^2, float32 with POWER's
 *   shape, bins and partial-last-bin rule.  A gain track therefore scales the antennas and a plain delay track changes nothing.
 *   The arithmetic, float32: p = fma(im, im, re re) of the sample, g2 = fma(gy, gy, gx gx) of weff; per frame q = fma(g2, p, q) over
 *   the antennas in index order from q = 0; the bin adds the frames' q in frame order from 0 and divides by its own count.  The
 *   coherent power minus this is the cross-only power 2 Re sum_{a<b} weff_a conj(weff_b) f_a conj(f_b).
 * align = 0: a plan with whole-sample delays (fxc_set_sample_delays, fxc_set_delay_track_aligned) is refused exactly as fxc_beamform
 *   refuses it.  align = 1: every pass is first copied, shifted, into the plan's alignment buffer exactly as a pass of fxc_fx_rows
 *   is, and the F stage reads from there; under an aligned track the pass's chunks take the shifts and the aligned tables of the
 *   plan's counter onwards.  The pass costs what it costs fxc_fx_rows (fxc_set_sample_delays above).  On a plan without
 *   whole-sample delays align has no effect and no alignment kernel is launched.
 * The passes keep the spectra, the effective weights, the staging of a host mask and the alignment buffer within the workspace
 * target; no output bit depends on the pass, the workspace target, the batch or host against device input.
 * FXC_ERR_ARG: as fxc_beamform, and a mode outside the three, mask_tint < 0 or > n_pts, align not 0 or 1 (INCOHERENT has no
 * voltage form: its output is always power).  FXC_ERR_UNSUPPORTED: n_beam > 16; whole-sample delays with align == 0.
 * FXC_ERR_STATE: a pipe on a plan with a track, or on a plan with whole-sample delays and align == 1.  A failed call puts the
 * track's counter back.
 * Out of scope: uint8 and complex128 input, pipes, Correlator integration, a normalised output, more than 16 beams, per-beam masks. */
int fxc_beamform_ex(fxc_plan* plan, const void* x, const void* weights, int n_beam, const void* mask, int64_t mask_tint, void* out,
                    int64_t n_chunks, int mem_kind, int mode, int64_t tint, int align);

/* Spectral kurtosis per antenna, from the spectra (Nita & Gary 2010): the interference detector that runs before
 * any correlation -- on unstopped fringes, on one receiver's own interference, and inside a chunk, where fxc_flag_rows sees
 * nothing.  f_a[c,i,k] = antenna a's spectrum of frame i of chunk c as fxc_channelize writes it.  Time bins hold `tint` frames
 * (0: the chunk); the last bin of a chunk may be partial and uses its own count M_j.  Over the M_j frames of bin j, with
 * p_i = |f_a[c,i,k]|^2, S1 = sum p_i, S2 = sum p_i^2:
 *     power[c][a][j][k'] = S1 / M_j
 *     sk[c][a][j][k']    = (M_j + 1) / (M_j - 1) * (M_j S2 / S1^2 - 1)
 * both float32 [n_chunks][n_ant][n_tbin][nchan], n_tbin = ceil(n_pts / tint), k' = (k + nchan / 2) % nchan: the rows' fftshifted
 * order, odd channel counts included.  sk is 1 for Gaussian noise whatever its power, 0 for a carrier of constant amplitude,
 * about 1 / d - 1 for a signal of duty cycle d (so blind near d = 1 / 2), and does not change when the bin is scaled: it needs no
 * bandpass, gains or delays.  Special cases, in this order: M_j < 2 gives sk = 1 exactly (one frame is no evidence; the power is
 * still written); a non-finite sample -- or sums beyond float32 -- gives NaN; S1 == 0 (a dead stream) gives sk = 0.
 * The statistic is taken on each antenna's stream as delivered: sample shifts (fxc_set_sample_delays, an aligned track), the
 * tables of fxc_set_rot / fxc_set_rot_ant, the delay track and its gains are NOT applied -- sk is invariant to all of them but the
 * zero fill of a shift -- and the track's counter does not move.  The accumulator is untouched (a pending fold is launched first).
 * x = [n_chunks][n_ant][num_samp] complex64; x, sk_out and power_out (may be NULL) all host memory (FXC_MEM_HOST: staged,
 * synchronous) or all device memory (FXC_MEM_DEVICE: queued on the plan's stream).  The plan's F stage runs a pass of chunks into
 * the workspace and one kernel reads every spectrum once; the passes are sized by the workspace target (FXC_WS_MB).  A bin's
 * frames are added in an order that depends on (n_pts, tint) alone -- float32 sums over segments of 64 frames from the bin's
 * first frame, the segments' sums added in float64 in segment order -- so no output bit depends on the batch size, the workspace
 * target or host against device input.
 * FXC_OK: n_chunks == 0 (nothing is read).  FXC_ERR_ARG: a NULL plan, x or sk_out, n_chunks < 0, tint < 0, tint == 1,
 * tint > n_pts, an unknown mem_kind (FXC_MEM_DEVICE_TO_PINNED included).  FXC_ERR_UNSUPPORTED: n_pts < 2.
 * Out of scope: uint8 and complex128 input, pipes, Correlator integration. */
int fxc_kurtosis(fxc_plan* plan, const void* x, void* sk_out, void* power_out, int64_t n_chunks, int mem_kind, int64_t tint);

/* The row weights from fxc_kurtosis's sk: the array every `weights` and `prior` argument takes (fxc_flag_rows,
 * fxc_solve_gains_weighted, fxc_fringe_fit_weighted, fxc_average_rows).  sk = [n_chunks][n_ant][n_tbin][nchan] float32 as
 * fxc_kurtosis(.., tint) wrote it, weights_out = [n_chunks][n_baselines][nchan] float32 in the memory of sk (mem_kind), baselines
 * (a, b), a < b, a-major.  A bin is counted unless it is a partial last bin and not the only bin of its chunk (its count is not
 * the one the thresholds were made for).  Element (c, (a,b), k') is 1.0 iff lo <= sk <= hi holds for every counted bin of antenna
 * a and of antenna b, else 0.0: a conjunction of comparisons in float64, so a NaN gives 0.  One threshold pair serves all bins.
 * FXC_OK: n_chunks == 0.  FXC_ERR_ARG: a NULL plan, sk or weights_out, n_chunks < 0, tint < 0, tint == 1, tint > n_pts, an unknown
 * mem_kind, lo or hi not finite, lo > hi.  FXC_ERR_UNSUPPORTED: n_pts < 2. */
int fxc_kurtosis_weights(fxc_plan* plan, const void* sk, int64_t n_chunks, int64_t tint, double lo, double hi, void* weights_out,
                         int mem_kind);

/* The antenna mask from fxc_kurtosis's sk: the `mask` of fxc_beamform_ex (mask_tint = tint), which sums antennas, not baselines.
 * sk and mask_out = [n_chunks][n_ant][n_tbin][nchan] float32 in the memory of sk (mem_kind), sk as fxc_kurtosis(.., tint) wrote it.
 * mask[c][a][j][k'] = 1.0 iff lo_j <= sk <= hi_j, else 0.0: comparisons in float64 on the float32 values, so a NaN gives 0.
 * (lo_j, hi_j) = (lo_last, hi_last) for a partial last bin that is not the chunk's only bin -- its count is not the one (lo, hi)
 * were made for --, and (lo, hi) otherwise.  Infinite thresholds are allowed (a last bin of one frame has sk = 1 exactly and no
 * evidence: Python gives it (-inf, inf)).
 * FXC_OK: n_chunks == 0.  FXC_ERR_ARG: a NULL plan, sk or mask_out, n_chunks < 0, tint < 0, tint == 1, tint > n_pts, an unknown
 * mem_kind, a threshold that is NaN, lo > hi, lo_last > hi_last.  FXC_ERR_UNSUPPORTED: n_pts < 2. */
int fxc_kurtosis_antenna_mask(fxc_plan* plan, const void* sk, int64_t n_chunks, int64_t tint, double lo, double hi, double lo_last,
                              double hi_last, void* mask_out, int mem_kind);

/* Incoherent dedispersion of power at full time resolution over trial dispersion measures: the step between a
 * beam and a detection of a pulsar or a fast transient -- the channels added along the dispersion sweep, for many trials.
 * power = float32 [n_chunks][n_series][n_tbin][nchan], nchan the plan's, channels in the rows' fftshifted order: exactly what
 * fxc_beamform(.., FXC_BEAM_POWER), FXC_BEAM_INCOHERENT and the power_out of fxc_kurtosis write; n_series stands for beams or
 * antennas.  mem_kind = FXC_MEM_HOST or FXC_MEM_DEVICE.  Time sample t = c n_tbin + j of chunk c, bin j; n_t = n_chunks n_tbin.
 * Every bin must hold the same number of frames -- tint must divide n_pts --: the caller's business, stated, not checked.
 * shifts = int32 [n_dm][nchan], HOST memory always: shifts[d][k] >= 0 is the number of time samples by which channel k lags at
 * trial d.  chan_weights = float32 [nchan], HOST memory always, or NULL: channel k counts iff chan_weights == NULL or
 * chan_weights[k] > 0 -- a NaN weight does not count, the convention of every `weights` argument here.  A channel that does not
 * count is selected away, not multiplied: NaN, Inf or 1e30 in it changes no output bit.  A counted non-finite value propagates
 * (stated, not checked).  Both are small, and the driver reads them before any device work.
 * With S_max the largest entry of the whole table, counted channel or not, and n_out = n_t - S_max:
 *   out[s][d][t] = sum over the counted k of P[t + shifts[d][k]][s][k],   t in [0, n_out)
 * float32 [n_series][n_dm][n_out] in the memory kind of power.  Nothing is normalised: (chan_weights > 0).sum() is the count.
 * The order of the additions: the channels are cut into segments of 64 from channel 0 of the rows' order, the last may be
 * partial; a segment's sum is a float32 sum from +0 over its counted channels in ascending k -- plain adds, there is no product,
 * so contraction cannot change it --; the output is the segments' sums added in float64 from 0 in segment order and rounded once
 * to float32.  With no counted channel the output is +0.  No bit depends on which kernel served a trial, on how trials, times or
 * series were tiled, on the workspace target, on host against device input or on the alignment of a device tensor.
 * info_out (HOST, may be NULL): [0] the trials the tiled kernel served, [1] the trials the direct kernel served.  Trials go
 * through in groups of 8 consecutive ones; a group takes the tiled kernel -- the samples of 32 channels transposed through LDS and
 * read once for the whole group -- where, in every 32 channels, the spread of the group's shifts over the counted channels is at
 * most 1023 samples, and the direct kernel, which keeps the contract total for any table with 0 <= shift < n_t, otherwise.
 * Device power needs no staging; host power goes through the workspace per series in slabs of whole chunks with a halo of S_max
 * samples, sized by the workspace target (FXC_WS_MB), a slab's outputs copied back; every output cell belongs to one launch.
 * Uses the plan's device, stream and workspace; synchronises like fxc_average_rows (one synchronisation ends the call); neither
 * reads nor changes the rot tables, the tracks, their counters or the accumulator (a pending fold is launched first).
 * FXC_ERR_ARG, before any device work: a NULL plan / power / shifts / out, n_chunks, n_series, n_tbin or n_dm below 1, an unknown
 * mem_kind (FXC_MEM_DEVICE_TO_PINNED included), a negative shift, S_max >= n_t.  FXC_ERR_UNSUPPORTED: n_t >= 2^31.
 * out and info_out are written on FXC_OK only.
 * Out of scope: coherent dedispersion of VOLTAGE beams, sub-band or tree algorithms, folding, a per-time mask,
 * frequency-averaged input, pipes, Correlator integration.  (The detection on these series is fxc_boxcar_search.) */
int fxc_dedisperse(fxc_plan* plan, const void* power, int64_t n_chunks, int64_t n_series, int64_t n_tbin, int mem_kind,
                   const int32_t* shifts /* HOST, [n_dm][nchan] */, int n_dm,
                   const float* chan_weights /* HOST, [nchan], may be NULL */,
                   void* out /* [n_series][n_dm][n_out] float32, in the memory kind of power */,
                   int64_t* info_out /* may be NULL: [0] trials on the tiled kernel, [1] trials on the direct kernel */);

/* Single-pulse search on dedispersed series: every row is normalised by a clipped mean and standard deviation,
 * matched-filtered with boxcars of the widths 2^j, j_lo <= j <= j_hi, and reduced to the best S/N of every block of `block`
 * starts with its width and its time -- a small map, the only thing that has to leave the device.
 * series = float32 [n_rows][n_t], mem_kind = FXC_MEM_HOST or FXC_MEM_DEVICE: a row is one (series, trial) of fxc_dedisperse's
 * output, the leading axes flattened.  0 <= j_lo <= j_hi <= 12, block >= 1, clip >= 0, 0 <= clip_iters <= 4.
 * Row statistics, every step one IEEE float64 operation, nothing contracted.  The tree sum of per-sample terms: the samples are
 * cut into segments of 256 from t = 0; a segment's sum runs from +0 over its counted samples in ascending t; 256 consecutive
 * segment sums are added in ascending order to a group sum; the group sums are added in ascending order.  A sample that does not
 * count is selected away, never multiplied.  Round 0 counts every sample.  In a round with n counted samples
 *   m = treesum(double(x)) / double(n),   e = double(x) - m,   v = treesum(e e) / double(n - 1)
 * and the next round counts sample t iff e e <= c2 v, e against this round's m, c2 = clip clip formed once on the host and c2 v
 * once per row: a sample dropped earlier may come back.  R = clip_iters rounds follow round 0, none if clip == 0; the last
 * round's (m, v, n) are the row's statistics and std the correctly rounded float64 square root of v.  A round that counts fewer
 * than 2 samples ends the rounds: the row is degenerate, as is one whose final v == 0.
 * Filter: y[t] = float32(double(x[t]) - m); L_0 = y; L_j[t] = L_{j-1}[t] + L_{j-1}[t + 2^(j-1)], one float32 add, for t in
 * [0, n_t - 2^j]; snr_j[t] = float32(double(L_j[t]) / den_j), den_j = std r_j formed once per row and width, r_j the float64
 * sqrt(2^j) from a table of 13 entries made on the host.  A width with 2^j > n_t has no start and does not compete.
 * Reduction: n_blk = ceil((n_t - 2^j_lo + 1) / block); block b owns the starts [b block, (b + 1) block); its candidates are
 * ordered by ascending j, then ascending t; the best is the first candidate, replaced only by a candidate whose snr is strictly
 * greater -- ties go to the narrowest width, then the earliest start.
 * snr_out float32, width_out int32 (the index j, not the width), time_out int32 (the absolute start t): [n_rows][n_blk] each, in
 * the memory kind of series.  A degenerate row gives snr +0, width j_lo and the block's first start in every cell.
 * stats_out (HOST memory always, may be NULL): double [n_rows][3] = (m, std, n) of the last round made; std = 0 for a degenerate
 * row.  With block = 1 and j_lo == j_hi the output is the whole matched-filtered series of that width.  A counted non-finite
 * sample propagates (stated, not checked).  No output bit depends on the tiles, on host against device input, on the alignment of
 * a device tensor or on the workspace target.
 * On the device: two sweeps over the input per round (the mean, then the squares about it), each followed by a small step that
 * adds the tree's upper levels and forms the round's numbers -- the host is not needed between rounds --; then a filter kernel
 * whose workgroup loads a tile of 4096 starts and its halo of 2^j_hi - 1 samples once and forms the levels in LDS.  Where block is
 * at most 4096 tiles begin on block boundaries and a cell belongs to one workgroup; a larger block is cut into tiles whose
 * partial bests a fold step takes in tile order.  Device input needs no staging; host input goes through the workspace in slabs of
 * whole rows sized by the workspace target (FXC_WS_MB), one row at least whatever its size, the three outputs of a slab copied back.
 * Uses the plan's device, stream and workspace; one synchronisation ends the call; neither reads nor changes the rot tables, the
 * tracks, their counters or the accumulator (a pending fold is launched first).
 * FXC_ERR_ARG, before any device work: a NULL plan / series / snr_out / width_out / time_out, n_rows, n_t or block below 1, j_lo < 0,
 * j_hi > 12, j_lo > j_hi, 2^j_lo > n_t, clip negative or NaN, clip_iters outside 0 .. 4, an unknown mem_kind
 * (FXC_MEM_DEVICE_TO_PINNED included).  FXC_ERR_UNSUPPORTED: n_t >= 2^31.  The outputs are written on FXC_OK only.
 * Out of scope: fusing the filter into the dedispersion kernel so that the series is never written, a running (windowed)
 * baseline, widths that are not powers of two, a per-time mask, candidate grouping across beams, folding, pipes, Correlator
 * integration. */
int fxc_boxcar_search(fxc_plan* plan, const void* series, int64_t n_rows, int64_t n_t, int mem_kind, int j_lo, int j_hi, int64_t block,
                      double clip, int clip_iters, void* snr_out /* float32 [n_rows][n_blk], in the memory kind of series */,
                      void* width_out /* int32, likewise */, void* time_out /* int32, likewise */,
                      double* stats_out /* HOST, [n_rows][3], may be NULL */);

/* Host-fed front end: replaces the reference's blocking per-chunk copies
 * (effex.py:391-392, 508-509, 693).  A pipe owns `depth` slots of pinned host staging + device buffers.
 * fxc_pipe_acquire hands the producer the pinned input buffer of the next free slot
 * ([chunks_per_batch][n_ant][num_samp] complex64) to fill in place; fxc_pipe_submit queues
 * H2D -> fxc_fx_rows -> D2H on three streams chained by events and returns; fxc_pipe_push = acquire + memcpy
 * from any host memory + submit; fxc_pipe_pop waits for the oldest batch and copies its rows out (layout as
 * fxc_fx_rows).  With depth >= 2 batch k+1 crosses PCIe while batch k computes.  acquire/submit/push fail with
 * FXC_ERR_STATE when `depth` batches are in flight, pop when none is.
 * The pipe uses the plan's stream and workspace: do not interleave other fxc_fx_* calls on the plan. */
int fxc_pipe_create(fxc_pipe** out, fxc_plan* plan, int64_t chunks_per_batch, int depth, int mode, double bandwidth);
/* the same pipe fed with RTL-SDR bytes: batches are [chunks_per_batch][n_ant][num_samp] interleaved uint8 I,Q and go
 * through fxc_fx_rows_u8 (a quarter of the PCIe traffic of complex64 samples) */
int fxc_pipe_create_u8(fxc_pipe** out, fxc_plan* plan, int64_t chunks_per_batch, int depth, int mode, double bandwidth,
                       int remove_dc);
/* any sample format (fxc_iq_format), batches through fxc_fx_rows_iq: complex64 / complex128 recordings with the DC
 * removal of effex.py:394-395 on the device instead of a host pass per chunk */
int fxc_pipe_create_iq(fxc_pipe** out, fxc_plan* plan, int64_t chunks_per_batch, int depth, int mode, double bandwidth,
                       int iq_format, int remove_dc);
int fxc_pipe_acquire(fxc_pipe* pipe, void** in_host);
int fxc_pipe_submit(fxc_pipe* pipe);
int fxc_pipe_push(fxc_pipe* pipe, const void* x_host);
int fxc_pipe_pop(fxc_pipe* pipe, void* out_host);
int fxc_pipe_in_flight(const fxc_pipe* pipe);
int fxc_pipe_destroy(fxc_pipe* pipe);

/* Measurement hooks (bench.py): HIP events on the plan's stream.  fxc_timer_* bracket a region;
 * with kernel profiling on, every launch of the dominant kernel is bracketed by its own event
 * pair and fxc_kernel_time returns the summed duration and launch count since the last reset. */
int fxc_timer_start(fxc_plan* plan);
int fxc_timer_stop(fxc_plan* plan, double* elapsed_ms);
int fxc_kernel_profiling(fxc_plan* plan, int enable);
int fxc_kernel_time(fxc_plan* plan, double* total_ms, int64_t* launches, int reset);

/* Deterministic synthetic IQ straight into HBM (same arithmetic as effex_amd/synth.py, bit for
 * bit): x_dev = [n_chunks][n_ant][num_samp] complex64.  delays = n_ant ints (host), tone =
 * complex64[tone_period] (host). */
int fxc_synth_fill(int device, void* stream, void* x_dev, uint64_t seed, int64_t first_chunk,
                   int64_t n_chunks, int n_ant, int64_t num_samp, const int32_t* delays,
                   const float* tone_re_im, int tone_period);

#ifdef __cplusplus
}
#endif
#endif /* FXCORR_H */
