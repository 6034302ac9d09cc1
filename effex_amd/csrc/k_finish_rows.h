// Part of libfxcorr's single translation unit: the rows kernels, included TWICE by k_finish.h -- once as the kernels of the plans
// without a delay track (rows_spectrum_kernel ...: rot operand `RotArg<ANT> rot`) and once as their tracked forms
// (rows_spectrum_track_kernel ...: operand `TrackRot<ANT> rot_arg`, and FXC_ROWS_CHUNK_ROT(row) declares `rot`, the operand of the
// row's chunk).  The same text twice rather than one template over both: the untracked kernels keep their names and compile to
// the code they had before there was a track.  FXC_ROWS_NAME(stem) names a kernel, FXC_ROWS_ROT declares its rot operand.

// SPECTRUM rows: out[c][p][(k + N/2) % N] = (sum_split raw) * conj(rot[k]) / n_pts   (effex.py:520-521)
// ANT: the rows are [chunk][n_prod] (baseline p = row % n_prod)
template <bool ANT = false>
__global__ void FXC_ROWS_NAME(rows_spectrum)(const cf* __restrict__ raw, cf* __restrict__ out, FXC_ROWS_ROT,
                                     int nchan, int64_t rows, int n_splits, int64_t split_stride, float inv_pts,
                                     int slots, LeadRows lead, int n_prod, int n_cross) {
    const int64_t total = rows * nchan;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        const int k = (int)(idx % nchan);
        const int64_t row = idx / nchan;
        float ar = 0.f, ai = 0.f;
        // sixteen loads in flight, added in the order of the splits (one at a time a bin of a single chunk with 256 rows -- few
        // channels, many slots -- waited out 256 trips to L2: 0.1 ms)
        const cf* src = raw + row * nchan + raw_index(k, slots);
        int s = 0;
        for (; s + 16 <= n_splits; s += 16) {
            cf r[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) r[q] = src[(s + q) * split_stride];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                ar += r[q].x;
                ai += r[q].y;
            }
        }
        for (; s < n_splits; ++s) {
            const cf r = src[s * split_stride];
            ar += r.x;
            ai += r.y;
        }
        add_lead_rows(raw, lead, row, nchan, k, slots, ar, ai);
        int ks = k + nchan / 2;
        if (ks >= nchan) ks -= nchan;
        if (auto_row(row, n_prod, n_cross)) {
            out[row * nchan + ks] = fxc::mk(ar * inv_pts, 0.f);
            continue;
        }
        float cr, ci;
        FXC_ROWS_CHUNK_ROT(row)
        if constexpr (ANT) {
            const cd w = ant_rot(rot, row % n_prod, k, nchan);
            cr = (float)w.x;
            ci = (float)w.y;
        } else {
            cr = (float)rot[k].x;
            ci = (float)rot[k].y;
        }
        // (ar + i ai) * (cr - i ci)
        const float orr = (ar * cr + ai * ci) * inv_pts;
        const float oi = (ai * cr - ar * ci) * inv_pts;
        out[row * nchan + ks] = fxc::mk(orr, oi);
    }
}

// CONTINUUM rows: out[row] = mean_k( raw * conj(rot) / n_pts ) / bandwidth   (effex.py:523-524); one WG per row, of
// kContinuumThreads threads: a reference-sized call is a single row whose frames the F+X kernel spread over the whole grid,
// so each bin gathers up to grid - 1 leading-part rows -- 72 us with 256 threads, the largest item of that call
template <bool ANT = false>
__global__ __launch_bounds__(kContinuumThreads) void FXC_ROWS_NAME(rows_continuum)(const cf* __restrict__ raw, cd* __restrict__ out,
                                                            FXC_ROWS_ROT, int nchan, int64_t rows,
                                                            int n_splits, int64_t split_stride, double scale,
                                                            int slots, LeadRows lead, int n_prod, int n_cross) {
    __shared__ double red[kContinuumThreads];
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const bool au = auto_row(row, n_prod, n_cross);
        FXC_ROWS_CHUNK_ROT(row)
        double ar = 0.0, ai = 0.0;
        for (int k = threadIdx.x; k < nchan; k += blockDim.x) {
            double xr = 0.0, xi = 0.0;
            sum_splits(raw + row * nchan + raw_index(k, slots), n_splits, split_stride, xr, xi);
            float lr_re = 0.f, lr_im = 0.f;
            add_lead_rows(raw, lead, row, nchan, k, slots, lr_re, lr_im);
            xr += lr_re;
            xi += lr_im;
            if (au) {
                ar += xr;
                continue;
            }
            cd w;
            if constexpr (ANT)
                w = ant_rot(rot, row % n_prod, k, nchan);
            else
                w = rot[k];
            ar += xr * w.x + xi * w.y;
            ai += xi * w.x - xr * w.y;
        }
        ar = block_sum(ar, red);
        ai = block_sum(ai, red);
        if (threadIdx.x == 0) {
            cd o;
            o.x = ar * scale;
            o.y = ai * scale;          // (auto rows: ai stayed an exact 0)
            out[row] = o;
        }
    }
}

// The same for a call of few rows (the reference's own call is ONE: effex.py:490-494): a row's bins are cut into `slices`
// workgroups (grid = slices x rows) that leave float64 partial sums, and rows_continuum_fin_kernel adds them in slice
// order -- one workgroup per row gathered a chunk pair's up to 255 leading-part rows for all 4096 bins in 33 us, the largest
// item of that call.
template <bool ANT = false>
__global__ __launch_bounds__(256) void FXC_ROWS_NAME(rows_continuum_part)(const cf* __restrict__ raw, cd* __restrict__ part,
                                                                 FXC_ROWS_ROT, int nchan, int64_t rows, int n_splits,
                                                                 int64_t split_stride, int slots, LeadRows lead, int slices,
                                                                 int n_prod, int n_cross) {
    __shared__ double red[256];
    const int64_t row = blockIdx.y;
    FXC_ROWS_CHUNK_ROT(row)
    const bool au = auto_row(row, n_prod, n_cross);
    const int per = (nchan + slices - 1) / slices;
    const int k_lo = blockIdx.x * per, k_hi = k_lo + per < nchan ? k_lo + per : nchan;
    double ar = 0.0, ai = 0.0;
    for (int k = k_lo + threadIdx.x; k < k_hi; k += blockDim.x) {
        double xr = 0.0, xi = 0.0;
        sum_splits(raw + row * nchan + raw_index(k, slots), n_splits, split_stride, xr, xi);
        float lr_re = 0.f, lr_im = 0.f;
        add_lead_rows(raw, lead, row, nchan, k, slots, lr_re, lr_im);
        xr += lr_re;
        xi += lr_im;
        if (au) {
            ar += xr;
            continue;
        }
        cd w;
        if constexpr (ANT)
            w = ant_rot(rot, row % n_prod, k, nchan);
        else
            w = rot[k];
        ar += xr * w.x + xi * w.y;
        ai += xi * w.x - xr * w.y;
    }
    ar = block_sum(ar, red);
    ai = block_sum(ai, red);
    if (threadIdx.x == 0) {
        cd o;
        o.x = ar;
        o.y = ai;
        part[row * slices + blockIdx.x] = o;
    }
}

