// Part of libfxcorr's single translation unit: included by fxcorr.hip ahead of h_plan.h (not a stand-alone header).
// The owners of what a plan, a pipe and a call hold on the device: each releases what it holds in its destructor, so a struct of
// them needs no list of things to free and an early return leaks nothing.  All are move-only and convert to the raw handle, so
// kernels and HIP calls take them as they took the raw pointers.  Of HIP they use hipMalloc / hipFree, hipHostMalloc / hipHostFree,
// hipEventCreateWithFlags / hipEventDestroy, hipStreamCreateWithFlags / hipStreamDestroy / hipStreamSynchronize and nothing else
// (flags come from the caller): tests/emul/emul_own.cpp compiles this file with g++ against counting stand-ins for those.
#pragma once
#include <cstddef>
#include <type_traits>
#include <utility>

namespace {

// one hipMalloc block of T (DevBuf<void>: of bytes)
template <class T>
class DevBuf {
    T* ptr_ = nullptr;
    size_t bytes_ = 0;
    static constexpr size_t kElem = sizeof(std::conditional_t<std::is_void<T>::value, char, T>);

  public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : ptr_(std::exchange(o.ptr_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) adopt(std::exchange(o.ptr_, nullptr), std::exchange(o.bytes_, 0));
        return *this;
    }
    ~DevBuf() { reset(); }
    operator T*() const { return ptr_; }
    T* get() const { return ptr_; }
    size_t bytes() const { return bytes_; }
    void reset() { adopt(nullptr, 0); }
    void adopt(T* ptr, size_t bytes) {      // takes over a hipMalloc block made elsewhere; frees what was held
        if (ptr_) (void)hipFree(ptr_);
        ptr_ = ptr;
        bytes_ = bytes;
    }
    hipError_t alloc(size_t count) {      // a fresh block of `count` elements; a failure leaves the buffer empty
        reset();
        void* v = nullptr;
        const hipError_t e = hipMalloc(&v, count * kElem);
        if (e == hipSuccess) adopt(static_cast<T*>(v), count * kElem);
        return e;
    }
    // grow-only: room for `count` elements, contents not kept.  Growing waits for `stream` (queued work may still use the old block),
    // frees, then allocates.  A failed wait changes nothing and sets *sync_failed; a failed allocation leaves the buffer empty
    hipError_t grow(hipStream_t stream, size_t count, bool* sync_failed = nullptr) {
        if (count * kElem <= bytes_) return hipSuccess;
        const hipError_t e = hipStreamSynchronize(stream);
        if (sync_failed) *sync_failed = e != hipSuccess;
        return e == hipSuccess ? alloc(count) : e;
    }
};

// one hipHostMalloc block
class PinnedBuf {
    void* ptr_ = nullptr;

  public:
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf&& o) noexcept : ptr_(std::exchange(o.ptr_, nullptr)) {}
    ~PinnedBuf() { reset(); }
    operator void*() const { return ptr_; }
    void reset() {
        if (ptr_) (void)hipHostFree(std::exchange(ptr_, nullptr));
    }
    hipError_t alloc(size_t bytes, unsigned flags) {
        reset();
        const hipError_t e = hipHostMalloc(&ptr_, bytes, flags);
        if (e != hipSuccess) ptr_ = nullptr;
        return e;
    }
};

class Event {
    hipEvent_t ev_ = nullptr;

  public:
    Event() = default;
    Event(Event&& o) noexcept : ev_(std::exchange(o.ev_, nullptr)) {}
    ~Event() { reset(); }
    operator hipEvent_t() const { return ev_; }
    void reset() {
        if (ev_) (void)hipEventDestroy(std::exchange(ev_, nullptr));
    }
    hipError_t create(unsigned flags) {
        reset();
        const hipError_t e = hipEventCreateWithFlags(&ev_, flags);
        if (e != hipSuccess) ev_ = nullptr;
        return e;
    }
};

// a stream of its own (create) or the caller's (borrow), which it only names
class Stream {
    hipStream_t s_ = nullptr;
    bool owned_ = false;

  public:
    Stream() = default;
    Stream(Stream&& o) noexcept : s_(std::exchange(o.s_, nullptr)), owned_(std::exchange(o.owned_, false)) {}
    ~Stream() { reset(); }
    operator hipStream_t() const { return s_; }
    void reset() { borrow(nullptr); }
    void borrow(hipStream_t s) {
        if (owned_ && s_) (void)hipStreamDestroy(s_);
        s_ = s;
        owned_ = false;
    }
    hipError_t create(unsigned flags) {
        reset();
        const hipError_t e = hipStreamCreateWithFlags(&s_, flags);
        owned_ = e == hipSuccess;
        if (!owned_) s_ = nullptr;
        return e;
    }
};

// What a finalize result too large for the finishing kernel to write over PCIe goes through: the side stream that copies it out,
// the event that orders that stream behind the kernel, a device buffer per result slot (in the order that frees memory first and
// destroys the stream last).  create() makes all of it or none
template <class T, int kSlots>
struct BigResults {
    Stream s_copy;
    Event ev_fin;
    DevBuf<T> d_res_big[kSlots];
    explicit operator bool() const { return s_copy != nullptr; }
    hipError_t create(unsigned stream_flags, unsigned event_flags, size_t count) {
        hipError_t e = s_copy.create(stream_flags);
        if (e == hipSuccess) e = ev_fin.create(event_flags);
        for (int k = 0; k < kSlots && e == hipSuccess; ++k) e = d_res_big[k].alloc(count);
        for (int k = 0; k < kSlots && e != hipSuccess; ++k) d_res_big[k].reset();
        if (e != hipSuccess) ev_fin.reset(), s_copy.reset();
        return e;
    }
};

}  // namespace
