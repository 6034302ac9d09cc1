// Part of libfxcorr's single translation unit: included by fxcorr.hip (not a stand-alone header).
#pragma once

// what a call runs: fx_rows_dev and fx_accumulate_dev go through one route ladder (fx_routes), which hands every pass's raw rows
// to the call's consumer -- the rows kernels (launch_rows) or the fold into the accumulator (h_launch.h)

namespace {

// ---- plans with autos (fxcorr.h, FXC_PRODUCTS_CROSS_AUTO): the first route of fx_routes -----------------------------------
// Every shape but the fused kernel's own (fused_autos) takes it: the plan's F stage alone -- run_channelize, what fxc_channelize runs (the tiled, wave-local,
// per-channel-count, mixed-radix or generic F kernel of the shape) -- writes a pass of chunks' spectra to the workspace as
// [chunk][antenna][frame][nchan] in natural bin order, then xengine_kernel<A, true> reads every spectrum once and writes raw rows
// [n_prod][nchan]: the n_base cross rows, then the A auto rows.  A raw row is a float32 sum of at most kRowSpectra spectra: up
// to `unit` chunks (integrations), or one of `xr` frame ranges of a chunk (k_finish.h::x_range) -- the multi-antenna fused route's
// rows.  Byte input reaches it through the conversion pass (condition_u8, h_ingest.h).
struct AutoPass {
    int64_t cb;          // chunks per pass
    int64_t unit;        // chunks per raw row at most
    int xr;              // frame ranges per chunk
    int64_t spec_bytes, raw_bytes;
};

AutoPass autos_pass(const fxc_plan* p, int64_t n_chunks, bool rows) {
    AutoPass a;
    a.unit = rows ? 1 : fused_unit(p);
    a.xr = a.unit > 1 ? 1 : frame_ranges(p);
    const int64_t spec_per_chunk = (int64_t)p->n_ant * p->n_pts * p->nchan * (int64_t)sizeof(cf);
    const int64_t raw_per_chunk = (int64_t)p->n_prod * p->nchan * (int64_t)sizeof(cf) * a.xr;
    int64_t cb = ws_target() / (spec_per_chunk + raw_per_chunk);
    cb = std::max<int64_t>(1, std::min<int64_t>(cb, n_chunks));
    cb = std::min<int64_t>(cb, std::max<int64_t>(1, 65535 / a.xr));     // groups x ranges ride in grid.y
    a.cb = cb;
    a.spec_bytes = up256(cb * spec_per_chunk);
    a.raw_bytes = up256(cb * raw_per_chunk);
    return a;
}

// chunks per raw row of an integration pass over nc chunks: as many X-engine workgroups as the device holds at once, within `unit`
int64_t autos_group(const fxc_plan* p, int64_t nc, int64_t unit) {
    const int64_t cols = std::max<int64_t>(1, (p->nchan + kXThreads - 1) / kXThreads);
    const int64_t groups = std::max<int64_t>(1, p->x_resident_auto / cols);
    return std::max<int64_t>(1, std::min<int64_t>(unit, (nc + groups - 1) / groups));
}

// 2 antennas at 4096 channels / 4 taps (complex64; byte input is converted first): the fused kernel's AUTOS variant, one pass
// (k_fused4096.h) -- the route of the cross-only plan, whole chunks and frame ranges alike, with raw rows of [3][kN]
bool fused_autos(const fxc_plan* p) { return p->autos && p->path == FXC_PATH_FUSED && p->n_ant == 2; }

// Rows of a plan with per-antenna tables (fxc_set_rot_ant: 3 and more antennas) go to the rows kernels' ANT instantiations.
// Every route of those plans lays its rows out as [chunk][n_prod] with the n_base cross rows first, so the kernels take
// n_prod and n_cross from the plan then (launch_rows below, where every route's rows end).
//
// Plans with a delay track (fxc_set_delay_track) go to the tracked instantiations: the pass's rows are [chunk][p->n_prod] on
// every route (two antennas: 1 row, or cross + 2 autos), its chunks take the plan's counter onwards, and track_pass writes
// their tables first.  The counter advances here, pass by pass; fx_rows_dev puts it back when a call fails half way.
//
// An aligned track (fxc_set_delay_track_aligned) first writes the whole-sample shifts of a run of chunks to d_tshift
// (track_shifts_pass: fx_call_dev for every pass, fxc_delay_track_tables for its chunk); the alignment of the pass and the
// aligned table kernels read them from there, so track_tables is only asked for chunks of the run written last.
int track_shifts_pass(fxc_plan* p, int64_t t0, int64_t n_t) {
    const int rg = grow(p, p->d_tshift, (size_t)(n_t * p->n_ant) * sizeof(int));
    if (rg) return rg;
    const TrackPar tp = {p->d_track_par, p->d_track_par + p->n_ant, p->track_df, p->track_freq};
    hipLaunchKernelGGL(track_shifts_kernel, dim3(grid_for(n_t * p->n_ant, 256, p->cu_count)), dim3(256), 0, p->stream, tp, p->track_bw,
                       static_cast<int*>(p->d_tshift.get()), p->n_ant, t0, n_t);
    FXC_HIP(p, hipGetLastError());
    p->tshift_t0 = t0;
    return FXC_OK;
}

int track_tables(fxc_plan* p, int64_t t0, int64_t n_t, cd* out, bool pair) {
    const TrackPar tp = {p->d_track_par, p->d_track_par + p->n_ant, p->track_df, p->track_freq};
    const dim3 grid(grid_for(n_t * (pair ? 1 : p->n_ant) * p->nchan, 256, p->cu_count));
    if (p->track_align) {
        const TrackAlign al = {static_cast<const int*>(p->d_tshift.get()), p->tshift_t0};
        const bool gain = p->gain_n > 0;
        const GainTrack gt = {p->d_gain_q, p->gain_n, p->gain_interval > 0 ? p->gain_interval : 1, p->gain_first};
        const auto launch = [&](auto pr, auto gn) {
            hipLaunchKernelGGL((track_tables_aligned_kernel<decltype(pr)::value, decltype(gn)::value>), grid, dim3(256), 0, p->stream, tp, al,
                               gt, out, p->n_ant, p->nchan, t0, n_t);
        };
        if (pair && gain) launch(std::true_type{}, std::true_type{});
        else if (pair) launch(std::true_type{}, std::false_type{});
        else if (gain) launch(std::false_type{}, std::true_type{});
        else launch(std::false_type{}, std::false_type{});
    } else if (p->gain_n > 0) {      // a gain track (fxc_set_track_gains): the same tables times 1 / g of the chunk's solution
        const GainTrack gt = {p->d_gain_q, p->gain_n, p->gain_interval > 0 ? p->gain_interval : 1, p->gain_first};
        if (pair)
            hipLaunchKernelGGL(track_gain_tables_kernel<true>, grid, dim3(256), 0, p->stream, tp, gt, out, p->n_ant, p->nchan, t0, n_t);
        else
            hipLaunchKernelGGL(track_gain_tables_kernel<false>, grid, dim3(256), 0, p->stream, tp, gt, out, p->n_ant, p->nchan, t0, n_t);
    } else if (pair)
        hipLaunchKernelGGL(track_tables_kernel<true>, grid, dim3(256), 0, p->stream, tp, out, p->n_ant, p->nchan, t0, n_t);
    else
        hipLaunchKernelGGL(track_tables_kernel<false>, grid, dim3(256), 0, p->stream, tp, out, p->n_ant, p->nchan, t0, n_t);
    FXC_HIP(p, hipGetLastError());
    return FXC_OK;
}

int track_pass(fxc_plan* p, int64_t n_chunks) {
    const int rg = grow(p, p->d_track, (size_t)(n_chunks * track_stride(p)) * sizeof(cd));
    if (rg) return rg;
    const int rc = track_tables(p, p->track_t, n_chunks, static_cast<cd*>(p->d_track.get()), p->n_ant == 2);
    if (rc) return rc;
    p->track_t += n_chunks;
    return FXC_OK;
}

// SPECTRUM rows
void launch_rows_spectrum(fxc_plan* p, const cf* raw, cf* out, int nchan, int64_t rows, int n_splits, int64_t split_stride,
                          float inv_pts, int slots, LeadRows lead, int n_prod, int n_cross) {
    const dim3 grid(grid_for(rows * nchan, 256, p->cu_count));
    with_rows_rot(p, [&](auto ant, auto trk, auto rot) {
        hipLaunchKernelGGL((rows_spectrum_kernel<decltype(ant)::value, decltype(trk)::value>), grid, dim3(256), 0, p->stream, raw, out, rot,
                           nchan, rows, n_splits, split_stride, inv_pts, slots, lead, n_prod, n_cross);
    });
}

// CONTINUUM rows: one workgroup per row when there are rows enough to fill the chip, else bin slices + a second small kernel
int launch_rows_continuum(fxc_plan* p, const cf* raw, cd* out, int nchan, int64_t rows, int n_splits, int64_t split_stride,
                          double scale, int slots, LeadRows lead, int n_prod, int n_cross) {
    const int slices = (int)std::min<int64_t>(32, nchan / 128);
    if (slices >= 2 && rows * 2 <= p->cu_count && rows <= 65535) {
        const int rg = grow(p, p->d_rowpart, (size_t)rows * slices * sizeof(cd));
        if (rg) return rg;
        cd* part = static_cast<cd*>(p->d_rowpart.get());
        with_rows_rot(p, [&](auto ant, auto trk, auto rot) {
            hipLaunchKernelGGL((rows_continuum_part_kernel<decltype(ant)::value, decltype(trk)::value>), dim3(slices, (unsigned)rows),
                               dim3(256), 0, p->stream, raw, part, rot, nchan, rows, n_splits, split_stride, slots, lead, slices, n_prod,
                               n_cross);
        });
        hipLaunchKernelGGL(rows_continuum_fin_kernel, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, p->stream, part, out, rows, slices,
                           scale);
    } else {
        const dim3 grid((int)std::min<int64_t>(rows, (int64_t)p->cu_count * 8));
        with_rows_rot(p, [&](auto ant, auto trk, auto rot) {
            hipLaunchKernelGGL((rows_continuum_kernel<decltype(ant)::value, decltype(trk)::value>), grid, dim3(continuum_threads(nchan)), 0,
                               p->stream, raw, out, rot, nchan, rows, n_splits, split_stride, scale, slots, lead, n_prod, n_cross);
        });
    }
    return FXC_OK;
}

// What a pass does with its raw rows when they are one set per chunk: SPECTRUM or CONTINUUM rows into `out` from row `row0` on, or
// -- kModeTrackFold, a tracked fx_accumulate -- the fold of the pass's chunks into the accumulator (track_fold_kernel)
constexpr int kModeTrackFold = -1;
struct RowsOut {
    int mode;
    void* out;
    float inv_pts;
    double cscale;
};

int launch_rows(fxc_plan* p, const RowsOut& o, int64_t row0, const cf* raw, int nchan, int64_t rows, int n_splits,
                int64_t split_stride, int slots, LeadRows lead, int n_prod = 1, int n_cross = 1) {
    if (p->rot_ant || p->track) {      // rows of [chunk][n_prod] on every route then: the plan's own counts
        n_prod = p->n_prod;
        n_cross = p->n_base;
    }
    if (p->track) {
        const int rc = track_pass(p, rows / p->n_prod);
        if (rc) return rc;
    }
    if (o.mode == FXC_MODE_SPECTRUM) {
        launch_rows_spectrum(p, raw, static_cast<cf*>(o.out) + row0 * nchan, nchan, rows, n_splits, split_stride, o.inv_pts, slots, lead,
                             n_prod, n_cross);
    } else if (o.mode == FXC_MODE_CONTINUUM) {
        const int rc = launch_rows_continuum(p, raw, static_cast<cd*>(o.out) + row0, nchan, rows, n_splits, split_stride, o.cscale, slots,
                                             lead, n_prod, n_cross);
        if (rc) return rc;
    } else {
        const dim3 grid(grid_for((int64_t)p->n_prod * nchan, 256, p->cu_count));
        with_rows_rot(p, [&](auto ant, auto trk, auto rot) {
            if constexpr (decltype(trk)::value)      // (kModeTrackFold: plans with a track only)
                hipLaunchKernelGGL(track_fold_kernel<decltype(ant)::value>, grid, dim3(256), 0, p->stream, raw, p->d_acc, rot, nchan,
                                   rows / p->n_prod, n_splits, split_stride, slots, lead, p->n_prod, p->n_base);
        });
    }
    FXC_HIP(p, hipGetLastError());
    return FXC_OK;
}

// The workspace of a call: a pass's spectra, its raw rows and -- `fold`, the plain fold -- the fold's partial sums, each from a
// 256-byte boundary.  Once per call, before anything writes the workspace: ensure_ws flushes a pending fold that lives there.
struct Workspace {
    cf *spec, *raw;
    cd* part;
};

int carve_ws(fxc_plan* p, bool fold, int64_t spec_bytes, int64_t raw_bytes, Workspace* w) {
    spec_bytes = up256(spec_bytes);
    raw_bytes = up256(raw_bytes);
    const int rc = ensure_ws(p, spec_bytes + raw_bytes + (fold ? fold_part_bytes(p) : 0));
    if (rc) return rc;
    char* base = static_cast<char*>(p->d_ws.get());
    w->spec = reinterpret_cast<cf*>(base);
    w->raw = reinterpret_cast<cf*>(base + spec_bytes);
    w->part = fold ? reinterpret_cast<cd*>(base + spec_bytes + raw_bytes) : nullptr;
    return FXC_OK;
}

// chunk c0 of a call's samples: complex64, or -- bytes (2 antennas) -- the receivers' uint8 I,Q, two bytes per sample
const cf* chunk_at(const fxc_plan* p, const cf* x, int64_t c0, bool bytes = false) {
    return reinterpret_cast<const cf*>(reinterpret_cast<const char*>(x) + c0 * p->n_ant * p->num_samp * (bytes ? 2 : (int64_t)sizeof(cf)));
}

// The one route ladder: which kernels a call runs, for fx_rows and fx_accumulate alike.  A route sizes its passes, carves the
// workspace, and pass by pass writes raw rows (float32 sums) and hands them on.  The consumer shows in two places of a route only:
//   o != nullptr  rows (fx_rows, and kModeTrackFold): one chunk per raw row, each pass finished by launch_rows;
//   o == nullptr  the plain fold of an untracked fx_accumulate: as many chunks per raw row as a float32 sum and the device's
//                 width allow, each pass folded into the accumulator (the call's last one left pending: fold_or_defer).
// dc_u8 != nullptr (2-antenna plans only): x is the uint8 I,Q stream [n_chunks][2][num_samp][2] and dc_u8 its per-stream
// conversion offsets; dck: the fused kernel sums its later chunks' bytes itself (never under a delay track)
int fx_routes(fxc_plan* p, const cf* x, const RowsOut* o, int64_t n_chunks, const cf* dc_u8, bool dck) {
    const bool bytes = dc_u8 != nullptr;
    Workspace w;
    if (p->autos && !fused_autos(p)) {
        // rows: one raw row per chunk and frame range, the ranges as the rows kernels' splits
        const AutoPass a = autos_pass(p, n_chunks, o != nullptr);
        int rc = carve_ws(p, !o, a.spec_bytes, a.raw_bytes, &w);
        if (rc) return rc;
        for (int64_t c0 = 0; c0 < n_chunks; c0 += a.cb) {
            const int64_t nc = std::min(a.cb, n_chunks - c0);
            const int64_t cg = autos_group(p, nc, a.unit);      // (rows: unit = 1, so one chunk)
            const int xr = cg > 1 ? 1 : a.xr;
            // raw[range][group][n_prod][nchan]
            rc = run_channelize(p, chunk_at(p, x, c0), w.spec, nc * p->n_ant);
            if (rc) return rc;
            rc = launch_xengine<true>(p, w.spec, w.raw, nc, (int)cg, xr);
            if (rc) return rc;
            const int64_t rows = nc * p->n_prod;
            rc = o ? launch_rows(p, *o, c0 * p->n_prod, w.raw, p->nchan, rows, xr, rows * p->nchan, 0, kNoLead, p->n_prod, p->n_base)
                   : fold_or_defer(p, w.raw, w.part, (nc + cg - 1) / cg * xr, 0, c0 + nc >= n_chunks);
            if (rc) return rc;
        }
    } else if (p->path == FXC_PATH_STREAM) {
        const int nb = (int)stream_blocks(p);
        const int64_t cb = std::min<int64_t>(n_chunks, 65535);
        const bool fold_parts = false;      // (stream1_acc_kernel needs none)
        int rc = carve_ws(p, fold_parts, 0, cb * nb * (int64_t)sizeof(cf), &w);
        if (rc) return rc;
        for (int64_t c0 = 0; c0 < n_chunks; c0 += cb) {
            const int64_t nc = std::min(cb, n_chunks - c0);
            rc = stream_raw_sums(p, chunk_at(p, x, c0), nc, w.raw);
            if (rc) return rc;
            // raw[block][chunk]: the blocks play the role of the generic path's splits (nchan = n_base = 1)
            if (o) {
                rc = launch_rows(p, *o, c0, w.raw, 1, nc, nb, nc, 0, kNoLead);
                if (rc) return rc;
            } else {
                hipLaunchKernelGGL(stream1_acc_kernel, dim3(1), dim3(256), 0, p->stream, w.raw, p->d_acc, nc * nb);
                FXC_HIP(p, hipGetLastError());
            }
        }
    } else if (p->path == FXC_PATH_FUSED || (p->path == FXC_PATH_TILED && p->n_ant > 2)) {
        int64_t spec_bytes, raw_bytes;
        const int64_t cb = fused_chunks_per_pass(p, n_chunks, &spec_bytes, &raw_bytes);
        int rc = carve_ws(p, !o, spec_bytes, raw_bytes, &w);
        if (rc) return rc;
        for (int64_t c0 = 0; c0 < n_chunks; c0 += cb) {
            const int64_t nc = std::min(cb, n_chunks - c0);
            // chunks per raw row.  Rows: one.  The plain fold: 2 antennas, rows of up to kRowSpectra spectra; more, the X-engine's
            // chunk groups
            const int64_t unit = o ? 1 : p->n_ant == 2 ? fused_unit(p) : xengine_group(p, nc, fused_unit(p));
            rc = fused_raw_sums(p, chunk_at(p, x, c0, bytes), nc, w.spec, w.raw, bytes ? dc_u8 + c0 * 2 : nullptr, unit, o != nullptr,
                                bytes && dck);
            if (rc) return rc;
            if (o) {
                // 3 and more antennas: the frame ranges of a chunk are the rows kernels' splits (range-major raw rows)
                const int64_t rows = nc * p->n_prod;
                rc = launch_rows(p, *o, c0 * p->n_prod, w.raw, p->nchan, rows, x_ranges(p, 1), rows * p->nchan, fused_layout(p),
                                 p->n_ant == 2 ? fused_lead(p, nc) : kNoLead, p->n_prod, p->n_base);
            } else {
                // 2 antennas: all the raw rows, leading parts included; more: one row [n_base][nchan] per chunk group and range
                const int64_t n_rows = p->n_ant == 2 ? fused_rows(p, nc, unit, false) : (nc + unit - 1) / unit * x_ranges(p, unit);
                rc = fold_or_defer(p, w.raw, w.part, n_rows, fused_layout(p), c0 + nc >= n_chunks);
            }
            if (rc) return rc;
        }
    } else if (p->split8192 && !dc_u8) {
        const int N = p->nchan;
        const int64_t cb = split_chunks_per_pass(p, n_chunks);
        int rc = carve_ws(p, !o, 0, (2 * cb + p->fused_grid_max) * (int64_t)fxc::fused::kN * (int64_t)sizeof(cf), &w);
        if (rc) return rc;
        for (int64_t c0 = 0; c0 < n_chunks; c0 += cb) {
            const int64_t nc = std::min(cb, n_chunks - c0);
            rc = split_raw_sums(p, chunk_at(p, x, c0), nc, w.raw);
            if (rc) return rc;
            // the nc pairs of 4096-rows are nc rows of 8192 in layout 3; the leading-part rows are added by parity
            const LeadRows lead = fused_lead(p, 2 * nc);
            if (o) {
                rc = launch_rows(p, *o, c0, w.raw, N, nc, 1, 0, 3, lead);
                if (rc) return rc;
            } else {      // (folded at once, never left pending: the leading parts follow it into the accumulator)
                rc = fold_rows(p, w.raw, w.part, nc, 3, kNoFinish);
                if (rc) return rc;
                hipLaunchKernelGGL(split_lead_acc_kernel, dim3(N / 256), dim3(256), 0, p->stream, w.raw, p->d_acc, lead);
                FXC_HIP(p, hipGetLastError());
            }
        }
    } else if (p->path == FXC_PATH_TILED) {
        const int N = p->nchan;
        const int n_splits = tiled_splits(p, split_basis(p, n_chunks));
        const int64_t row_bytes = (int64_t)N * (int64_t)sizeof(cf);
        const int64_t cb = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(n_chunks, tiled_streams_per_pass(p) / 2),
                                                                  ws_target() / (row_bytes * n_splits)));
        int rc = carve_ws(p, !o, 0, cb * n_splits * row_bytes, &w);
        if (rc) return rc;
        for (int64_t c0 = 0; c0 < n_chunks; c0 += cb) {
            const int64_t nc = std::min(cb, n_chunks - c0);
            rc = tiled_raw_sums(p, chunk_at(p, x, c0, bytes), nc, n_splits, w.raw, bytes ? dc_u8 + c0 * 2 : nullptr);
            if (rc) return rc;
            rc = o ? launch_rows(p, *o, c0, w.raw, N, nc, n_splits, nc * N, 0, kNoLead)
                   : fold_or_defer(p, w.raw, w.part, nc * n_splits, 0, c0 + nc >= n_chunks);
            if (rc) return rc;
        }
    } else {
        const bool xf = mixed_one_pass(p, bytes);
        const bool xm = !xf && two_pass_xm(p, bytes);
        const XGeom g = x_geometry(p, split_basis(p, n_chunks), xf, xm);
        int64_t spec_bytes, raw_bytes;
        const int64_t cb = generic_chunks_per_pass(p, n_chunks, g, &spec_bytes, &raw_bytes, xf, xm);
        int rc = carve_ws(p, !o, spec_bytes, raw_bytes, &w);
        if (rc) return rc;
        for (int64_t c0 = 0; c0 < n_chunks; c0 += cb) {
            const int64_t nc = std::min(cb, n_chunks - c0);
            const cf* xc = chunk_at(p, x, c0, bytes);
            KernelTimer kt(p);
            if (xf) {
                // (bytes in: the offsets of this pass's streams)
                rc = mixed_fx_raw_sums(p, xc, nc, g.n_splits, w.raw, bytes ? dc_u8 + c0 * 2 : nullptr);
                if (rc) return rc;
            } else if (xm) {
                rc = two_pass_raw_sums(p, xc, nc, g.n_splits, w.spec, w.raw);
                if (rc) return rc;
            } else if (p->mixed_xeng) {
                // 3 .. 64 antennas off the powers of two: spectra antenna-interleaved, then the X-engines of the tiled paths
                rc = run_channelize(p, xc, w.spec, nc * p->n_ant, p->n_ant);
                if (rc) return rc;
                rc = launch_xengine(p, w.spec, w.raw, nc, 1, g.n_splits);
                if (rc) return rc;
            } else {
                rc = run_channelize(p, xc, w.spec, nc * p->n_ant);
                if (rc) return rc;
                const int kblocks = (p->nchan + g.kx - 1) / g.kx;
                const int64_t wgs = nc * p->n_base * kblocks * g.n_splits;
                hipLaunchKernelGGL(xmul_kernel, dim3((int)std::min<int64_t>(wgs, (int64_t)p->cu_count * 8)), dim3(256), 0,
                                   p->stream, w.spec, w.raw, p->n_ant, p->n_base, p->nchan, p->n_pts, g.kx, g.n_splits, nc);
            }
            kt.stop();
            FXC_HIP(p, hipGetLastError());
            // raw[split][chunk] = nc * n_splits rows of [n_base][nchan], natural bin order
            const int64_t rows = nc * p->n_base;
            rc = o ? launch_rows(p, *o, c0 * p->n_base, w.raw, p->nchan, rows, g.n_splits, rows * p->nchan, 0, kNoLead)
                   : fold_or_defer(p, w.raw, w.part, nc * g.n_splits, 0, c0 + nc >= n_chunks);
            if (rc) return rc;
        }
    }
    return FXC_OK;
}

// device-resident implementation of fx_rows; out = cf[n_chunks][n_prod][nchan] or cd[n_chunks][n_prod].  Under a delay track
// the call's chunks are the plan's chunks track_t .. track_t + n_chunks - 1 (launch_rows counts them pass by pass).
int fx_rows_dev(fxc_plan* p, const cf* x, void* out, int64_t n_chunks, int mode, double bandwidth, const cf* dc_u8, bool dck) {
    if (n_chunks == 0) return FXC_OK;
    const RowsOut o = {mode, out, (float)(1.0 / (double)p->n_pts), 1.0 / ((double)p->n_pts * (double)p->nchan * bandwidth)};
    const int64_t t0 = p->track_t;
    const int rc = fx_routes(p, x, &o, n_chunks, dc_u8, dck);
    if (rc) p->track_t = t0;
    return rc;
}

// device-resident implementation of fx_accumulate.  Under a delay track rot changes from chunk to chunk, so it is applied before
// the sum over chunks: the call runs the ladder as rows (one raw row set per chunk), folded by track_fold_kernel
int fx_accumulate_dev(fxc_plan* p, const cf* x, int64_t n_chunks, const cf* dc_u8, bool dck) {
    if (n_chunks == 0) return FXC_OK;
    p->acc_track = p->track;
    const int rc = p->track ? fx_rows_dev(p, x, nullptr, n_chunks, kModeTrackFold, 1.0, dc_u8, dck)
                            : fx_routes(p, x, nullptr, n_chunks, dc_u8, dck);
    if (rc) return rc;
    p->spectra_count += (double)n_chunks * (double)p->n_pts;
    return FXC_OK;
}

// host-buffer helper: stage in, run, stage out (synchronous)
// Pageable buffers go through the runtime's bounce buffers inside hipMemcpyAsync; buffers from fxc_host_alloc are pinned, so
// the same call is one DMA -- and an `out` inside such a block is handed to fn as the device's mapping of it: the finishing
// kernel writes the rows over PCIe itself (32 KiB per chunk pair) and no copy back is queued.
template <class Fn>
int with_host_staging(fxc_plan* p, const void* x, size_t x_bytes, void* out, size_t out_bytes, Fn fn) {
    // staging buffers live in the plan and only grow: the reference calls once per chunk pair (effex.py:490-494),
    // and a hipMalloc / hipFree pair per call costs more than the copy of one chunk
    void* out_mapped = out_bytes ? pinned_device_ptr(out, out_bytes) : nullptr;
    const size_t want[2] = {x_bytes ? x_bytes : 1, out_mapped ? 0 : out_bytes};
    for (int k = 0; k < 2; ++k) {
        const int rg = grow(p, p->d_stage[k], want[k]);
        if (rg) return rg;
    }
    void* dx = p->d_stage[0];
    void* dout = out_bytes ? (out_mapped ? out_mapped : p->d_stage[1]) : nullptr;
    int rc = FXC_OK;
    // (a kernel fetching the pinned block over PCIe itself instead of the copy engine was measured: 0.149 against 0.133 ms per
    // reference-sized call, profiles/r04/experiments.md)
    hipError_t e = hipMemcpyAsync(dx, x, x_bytes, hipMemcpyHostToDevice, p->stream);
    if (e == hipSuccess) rc = fn(static_cast<const cf*>(dx), dout);
    if (e == hipSuccess && rc == FXC_OK && out_bytes && !out_mapped)
        e = hipMemcpyAsync(out, dout, out_bytes, hipMemcpyDeviceToHost, p->stream);
    hipError_t e2 = hipStreamSynchronize(p->stream);
    if (rc != FXC_OK) return rc;
    if (e != hipSuccess) return fail(p, FXC_ERR_HIP, "host staging copy failed: %s", hipGetErrorString(e));
    if (e2 != hipSuccess) return fail(p, FXC_ERR_HIP, "stream sync failed: %s", hipGetErrorString(e2));
    return FXC_OK;
}

// Queue the finalize of `sums_src` (exported, possibly cross-rank reduced sums) or, sums_src == nullptr, of the plan's
// accumulator -- then together with the fold of the rows still pending and with the reset, in one kernel -- into the
// next result slot; the slot's event marks the host copy complete.
// user_out != nullptr (fxc_finalize_async_to): the result goes to that host buffer instead of the plan's pinned slot -- by
// the finishing kernel itself when it is small and lies in fxc_host_alloc memory, by the side-stream copy when it is large
// (a direct DMA for pinned memory) -- and fxc_finalize_wait copies nothing.
int finalize_enqueue(fxc_plan* p, const cd* sums_src, int mode, double bandwidth, int reset, void* user_out = nullptr) {
    if (mode != FXC_MODE_SPECTRUM && mode != FXC_MODE_CONTINUUM) return fail(p, FXC_ERR_ARG, "bad mode %d", mode);
    if (mode == FXC_MODE_CONTINUUM && !(bandwidth > 0.0)) return fail(p, FXC_ERR_ARG, "bandwidth must be > 0");
    if (p->res_head - p->res_tail >= fxc_plan::kResSlots)
        return fail(p, FXC_ERR_STATE, "%d finalize results outstanding: collect one with fxc_finalize_wait first",
                    fxc_plan::kResSlots);
    if (!sums_src && !(p->spectra_count > 0.0)) return fail(p, FXC_ERR_STATE, "nothing accumulated");
    const int slot = (int)(p->res_head % fxc_plan::kResSlots);
    const int64_t n = (int64_t)p->n_prod * p->nchan;
    const size_t bytes = mode == FXC_MODE_SPECTRUM ? (size_t)n * sizeof(cd) : (size_t)p->n_prod * sizeof(cd);
    // small results are written into the pinned slot by the finishing kernel itself; large ones go through device
    // memory and a copy on a side stream, off the F+X stream's critical path
    const bool big = bytes > res_direct_bytes();
    if (big && !p->big_res) FXC_HIP(p, p->big_res.create(hipStreamNonBlocking, hipEventDisableTiming, (size_t)acc_capacity(p)));
    cd* out = big ? p->big_res.d_res_big[slot] : p->d_res[slot];
    cd* const user_mapped = (user_out && !big) ? static_cast<cd*>(pinned_device_ptr(user_out, bytes)) : nullptr;
    if (user_mapped) out = user_mapped;
    // where fxc_finalize_wait finds the bytes: the caller's buffer (nothing to copy) or the plan's slot
    p->res_user[slot] = (user_out && (big || user_mapped)) ? user_out : nullptr;
    p->res_dst[slot] = user_out;
    if (!sums_src) {
        // SPECTRUM: one kernel.  CONTINUUM needs the mean over the bins of the finished accumulator: export, then reduce
        FoldFinish fin = {nullptr, out, nullptr, p->spectra_count, reset ? 1 : 0};
        if (mode == FXC_MODE_CONTINUUM) {
            // into a buffer of its own: d_sums may hold reduced sums (fxc_reduce) that fxc_finalize_sums(plan, NULL) has yet
            // to read, and only fxc_reduce makes that copy valid
            if (!p->d_cont) FXC_HIP(p, p->d_cont.alloc((size_t)acc_capacity(p) + 1));
            fin.sums = p->d_cont;
            fin.out = nullptr;
            sums_src = p->d_cont;
        }
        // the slot's event rides on the last kernel's own completion (hipExtLaunchKernelGGL): an event recorded behind it is
        // a packet of its own in the stream, and the next F+X kernel starts 11 us later for it
        const int rc = flush_pending(p, &fin, (mode == FXC_MODE_SPECTRUM && !big) ? p->ev_res[slot] : nullptr);
        if (rc) return rc;
        if (reset) p->spectra_count = 0.0;
    } else if (mode == FXC_MODE_SPECTRUM) {
        const int rc = flush_pending(p);
        if (rc) return rc;
        with_finish_rot(p, true, [&](auto ant, auto rot) {
            hipExtLaunchKernelGGL(finalize_spectrum_kernel<decltype(ant)::value>, dim3(grid_for(n, 256, p->cu_count)), dim3(256), 0, p->stream,
                                  nullptr, big ? nullptr : p->ev_res[slot], 0, sums_src, out, rot, p->nchan, p->n_prod, p->n_base);
        });
    }
    if (mode == FXC_MODE_CONTINUUM) {
        with_finish_rot(p, true, [&](auto ant, auto rot) {
            hipExtLaunchKernelGGL(finalize_continuum_kernel<decltype(ant)::value>, dim3(p->n_prod), dim3(256), 0, p->stream, nullptr,
                                  big ? nullptr : p->ev_res[slot], 0, sums_src, out, rot, p->nchan, p->n_prod, 1.0 / bandwidth, p->n_base);
        });
    }
    FXC_HIP(p, hipGetLastError());
    if (big) {
        FXC_HIP(p, hipEventRecord(p->big_res.ev_fin, p->stream));
        FXC_HIP(p, hipStreamWaitEvent(p->big_res.s_copy, p->big_res.ev_fin, 0));
        FXC_HIP(p, hipMemcpyAsync(user_out ? user_out : static_cast<void*>(p->h_res[slot]), out, bytes, hipMemcpyDeviceToHost, p->big_res.s_copy));
        FXC_HIP(p, hipEventRecord(p->ev_res[slot], p->big_res.s_copy));
    }
    p->res_bytes[slot] = bytes;
    p->res_head += 1;
    return FXC_OK;
}

}  // namespace
