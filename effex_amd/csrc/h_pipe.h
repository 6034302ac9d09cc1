// Part of libfxcorr's single translation unit: included by fxcorr.hip (not a stand-alone header).
#pragma once

// the host-fed pipe (fxc_pipe, h_plan.h): the drivers behind fxc_pipe_* (fxcorr.hip keeps their argument checks)

namespace {

int pipe_destroy(fxc_pipe* q) {
    DeviceGuard device_guard__(q->plan->device);
    if (q->counted) q->plan->live_pipes -= 1;
    (void)hipStreamSynchronize(q->plan->stream);
    if (q->s_in) (void)hipStreamSynchronize(q->s_in);
    if (q->s_out) (void)hipStreamSynchronize(q->s_out);
    delete q;      // the slots (memory, then events), then the two streams: the order of fxc_pipe's members
    return FXC_OK;
}

// fxc_pipe_create_iq below its checks
int pipe_create(fxc_pipe** out, fxc_plan* p, int64_t chunks_per_batch, int depth, int mode, double bandwidth, int fmt, int remove_dc) {
    FXC_DEVICE(p, p->device);
    fxc_pipe* q = new (std::nothrow) fxc_pipe();
    if (!q) return fail(p, FXC_ERR_NOMEM, "host allocation failed");
    q->plan = p;
    q->chunks = chunks_per_batch;
    q->depth = depth;
    q->mode = mode;
    q->bandwidth = bandwidth;
    q->fmt = fmt;
    q->remove_dc = remove_dc;
    q->in_bytes = input_bytes(p, fmt, chunks_per_batch);
    q->out_bytes = (size_t)chunks_per_batch * row_bytes(p, mode);
    q->slots.resize((size_t)depth);
    hipError_t e = q->s_in.create(hipStreamNonBlocking);
    if (e == hipSuccess) e = q->s_out.create(hipStreamNonBlocking);
    for (auto& sl : q->slots) {
        if (e == hipSuccess) e = sl.h_in.alloc(q->in_bytes, hipHostMallocDefault);
        if (e == hipSuccess) e = sl.h_out.alloc(q->out_bytes, hipHostMallocDefault);
        if (e == hipSuccess) e = sl.d_in.alloc(q->in_bytes);
        if (e == hipSuccess) e = sl.d_out.alloc(q->out_bytes);
        if (e == hipSuccess) e = sl.ev_in.create(hipEventDisableTiming);
        if (e == hipSuccess) e = sl.ev_compute.create(hipEventDisableTiming);
        if (e == hipSuccess) e = sl.ev_out.create(hipEventDisableTiming);
    }
    if (e != hipSuccess) {
        delete q;
        return fail(p, e == hipErrorOutOfMemory ? FXC_ERR_NOMEM : FXC_ERR_HIP, "pipeline setup failed: %s",
                    hipGetErrorString(e));
    }
    p->live_pipes += 1;
    q->counted = true;
    *out = q;
    return FXC_OK;
}

int pipe_acquire(fxc_pipe* q, void** in_host) {
    if (q->pushed - q->popped >= q->depth)
        return fail(q->plan, FXC_ERR_STATE, "all %d slots in flight: pop first", q->depth);
    *in_host = q->slots[(size_t)(q->pushed % q->depth)].h_in;      // popped, hence idle
    return FXC_OK;
}

int pipe_submit(fxc_pipe* q) {
    fxc_plan* p = q->plan;
    if (q->pushed - q->popped >= q->depth) return fail(p, FXC_ERR_STATE, "all %d slots in flight: pop first", q->depth);
    FXC_DEVICE(p, p->device);
    fxc_pipe_slot& sl = q->slots[(size_t)(q->pushed % q->depth)];
    FXC_HIP(p, hipMemcpyAsync(sl.d_in, sl.h_in, q->in_bytes, hipMemcpyHostToDevice, q->s_in));
    FXC_HIP(p, hipEventRecord(sl.ev_in, q->s_in));
    FXC_HIP(p, hipStreamWaitEvent(p->stream, sl.ev_in, 0));
    // the slot's device copy is the pipe's own (x_is_scratch): complex64 batches are de-meaned in place
    int rc = fx_call_dev(p, {q->fmt, q->remove_dc != 0, true, q->mode, q->bandwidth}, sl.d_in, sl.d_out, q->chunks, true);
    if (rc) return rc;
    FXC_HIP(p, hipEventRecord(sl.ev_compute, p->stream));
    FXC_HIP(p, hipStreamWaitEvent(q->s_out, sl.ev_compute, 0));
    FXC_HIP(p, hipMemcpyAsync(sl.h_out, sl.d_out, q->out_bytes, hipMemcpyDeviceToHost, q->s_out));
    FXC_HIP(p, hipEventRecord(sl.ev_out, q->s_out));
    sl.busy = true;
    q->pushed += 1;
    return FXC_OK;
}

int pipe_push(fxc_pipe* q, const void* x_host) {
    void* dst = nullptr;
    int rc = pipe_acquire(q, &dst);
    if (rc) return rc;
    std::memcpy(dst, x_host, q->in_bytes);
    return pipe_submit(q);
}

int pipe_pop(fxc_pipe* q, void* out_host) {
    fxc_plan* p = q->plan;
    if (q->pushed == q->popped) return fail(p, FXC_ERR_STATE, "nothing in flight");
    FXC_DEVICE(p, p->device);
    fxc_pipe_slot& sl = q->slots[(size_t)(q->popped % q->depth)];
    FXC_HIP(p, hipEventSynchronize(sl.ev_out));
    std::memcpy(out_host, sl.h_out, q->out_bytes);
    sl.busy = false;
    q->popped += 1;
    return FXC_OK;
}

}  // namespace
