// Host test of effex_amd/csrc/h_own.h: the owners against counting stand-ins for the HIP calls they make.  A program of its
// own (tests/test_own_host.py builds it with the address and undefined-behaviour sanitizers and runs it): exit status 0 when
// every check holds.  Memory comes from malloc, so a double free or a leak is the sanitizer's to report as well.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

// ---- stand-ins ---------------------------------------------------------------------------------------------------------
typedef int hipError_t;
constexpr hipError_t hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorUnknown = 999;
typedef struct StandInEvent* hipEvent_t;
typedef struct StandInStream* hipStream_t;
struct StandInEvent { unsigned flags; };
struct StandInStream { unsigned flags; };

static std::set<void*> g_live;              // every handle and block handed out and not yet released
static std::vector<std::string> g_log;      // the calls, in order
static int g_malloc_calls = 0, g_fail_malloc_at = 0;      // hipMalloc fails on its g_fail_malloc_at-th call (0: never)
static int g_fail_sync = 0, g_fail_stream = 0, g_fail_event = 0;
static int g_failures = 0;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++g_failures;                                                        \
        }                                                                        \
    } while (0)

static void hand_out(void* p, const char* what) {
    CHECK(g_live.insert(p).second);
    g_log.push_back(what);
}
static hipError_t release(void* p, const char* what) {
    g_log.push_back(what);
    CHECK(g_live.erase(p) == 1);      // released exactly once, and only what was handed out
    return hipSuccess;
}

hipError_t hipMalloc(void** p, size_t bytes) {
    if (++g_malloc_calls == g_fail_malloc_at) {
        g_log.push_back("malloc-failed");
        return hipErrorOutOfMemory;
    }
    *p = std::malloc(bytes ? bytes : 1);
    hand_out(*p, "malloc");
    return hipSuccess;
}
hipError_t hipFree(void* p) {
    const hipError_t e = release(p, "free");
    std::free(p);
    return e;
}
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) {
    *p = std::malloc(bytes ? bytes : 1);
    hand_out(*p, "host-malloc");
    return hipSuccess;
}
hipError_t hipHostFree(void* p) {
    const hipError_t e = release(p, "host-free");
    std::free(p);
    return e;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* ev, unsigned flags) {
    if (g_fail_event) return hipErrorUnknown;
    *ev = new StandInEvent{flags};
    hand_out(*ev, "event");
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t ev) {
    const hipError_t e = release(ev, "event-destroy");
    delete ev;
    return e;
}
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned flags) {
    if (g_fail_stream) return hipErrorUnknown;
    *s = new StandInStream{flags};
    hand_out(*s, "stream");
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) {
    const hipError_t e = release(s, "stream-destroy");
    delete s;
    return e;
}
hipError_t hipStreamSynchronize(hipStream_t) {
    g_log.push_back("sync");
    return g_fail_sync ? hipErrorUnknown : hipSuccess;
}

#include "../../effex_amd/csrc/h_own.h"

static void fresh() {
    CHECK(g_live.empty());
    g_log.clear();
    g_malloc_calls = g_fail_malloc_at = g_fail_sync = g_fail_stream = g_fail_event = 0;
}
static bool log_is(std::vector<std::string> want) { return g_log == want; }

struct Pair { double x, y; };

int main() {
    // ---- DevBuf: allocate, release once, moves ---------------------------------------------------------------------------
    fresh();
    {
        DevBuf<Pair> a;
        CHECK(!a && a.bytes() == 0);
        CHECK(a.alloc(10) == hipSuccess && a && a.bytes() == 10 * sizeof(Pair));
        Pair* raw = a;
        raw[9].x = 1.0;      // (the block is as large as it says)
        DevBuf<Pair> b(std::move(a));
        CHECK(!a && a.bytes() == 0 && b.get() == raw && b.bytes() == 10 * sizeof(Pair));      // a move leaves the source empty
        DevBuf<Pair> c;
        CHECK(c.alloc(3) == hipSuccess);
        c = std::move(b);      // frees what c held, takes b's
        CHECK(!b && b.bytes() == 0 && c.get() == raw && g_live.size() == 1);
        c = std::move(c);      // (self-assignment keeps the block)
        CHECK(c.get() == raw);
        c.reset();
        CHECK(!c && c.bytes() == 0 && g_live.empty());
        c.reset();      // (an empty buffer frees nothing)
    }
    CHECK(log_is({"malloc", "malloc", "free", "free"}));

    // ---- DevBuf<void>: counts are bytes; grow ----------------------------------------------------------------------------------
    fresh();
    {
        StandInStream st{0};
        DevBuf<void> v;
        CHECK(v.grow(&st, 100) == hipSuccess && v.bytes() == 100);
        CHECK(log_is({"sync", "malloc"}));      // (as grow() of the plan always did: the wait comes first, held or not)
        void* raw = v;
        CHECK(v.grow(&st, 100) == hipSuccess && v.grow(&st, 7) == hipSuccess && v.grow(&st, 0) == hipSuccess);
        CHECK(v.get() == raw && v.bytes() == 100 && g_log.size() == 2);      // smaller or equal: nothing is called, the pointer stays
        g_log.clear();
        CHECK(v.grow(&st, 101) == hipSuccess && v.bytes() == 101);
        CHECK(log_is({"sync", "free", "malloc"}));      // larger: wait, free, allocate -- in that order
        // a failed allocation leaves the buffer empty
        g_log.clear();
        g_fail_malloc_at = g_malloc_calls + 1;
        bool sync_failed = true;
        CHECK(v.grow(&st, 500, &sync_failed) == hipErrorOutOfMemory && !sync_failed);
        CHECK(!v && v.bytes() == 0 && g_live.empty());
        CHECK(log_is({"sync", "free", "malloc-failed"}));
        // a failed wait changes nothing
        CHECK(v.grow(&st, 64) == hipSuccess);
        raw = v;
        g_fail_sync = 1;
        CHECK(v.grow(&st, 65, &sync_failed) == hipErrorUnknown && sync_failed && v.get() == raw && v.bytes() == 64);
        g_fail_sync = 0;
    }
    CHECK(g_live.empty());

    // ---- adopt frees what was held -------------------------------------------------------------------------------------------
    fresh();
    {
        DevBuf<int> t;
        CHECK(t.alloc(4) == hipSuccess);
        int* held = t;
        void* made = nullptr;
        CHECK(hipMalloc(&made, 8 * sizeof(int)) == hipSuccess);
        t.adopt(static_cast<int*>(made), 8 * sizeof(int));
        CHECK(t.get() == made && t.bytes() == 8 * sizeof(int) && g_live.count(held) == 0 && g_live.size() == 1);
    }
    CHECK(log_is({"malloc", "malloc", "free", "free"}));

    // ---- PinnedBuf, Event, Stream --------------------------------------------------------------------------------------------
    fresh();
    {
        PinnedBuf h;
        CHECK(!h && h.alloc(256, 3) == hipSuccess && h);
        PinnedBuf h2(std::move(h));
        CHECK(!h && h2);
        CHECK(h2.alloc(16, 3) == hipSuccess && g_live.size() == 1);      // (a second alloc frees the first)
        Event e;
        CHECK(!e && e.create(2) == hipSuccess && e);
        CHECK(static_cast<hipEvent_t>(e)->flags == 2);
        Event e2(std::move(e));
        CHECK(!e && e2);
        CHECK(e2.create(1) == hipSuccess && g_live.size() == 2);      // (a second create destroys the first)
        g_fail_event = 1;
        CHECK(e2.create(0) == hipErrorUnknown && !e2 && g_live.size() == 1);
        g_fail_event = 0;
        Stream s;
        CHECK(!s && s.create(1) == hipSuccess && s);
        Stream s2(std::move(s));
        CHECK(!s && s2);
    }
    CHECK(g_live.empty());
    // a borrowed stream is the caller's: named, never destroyed
    fresh();
    {
        StandInStream callers{0};
        Stream s;
        s.borrow(&callers);
        CHECK(static_cast<hipStream_t>(s) == &callers);
        Stream moved(std::move(s));
        CHECK(!s && static_cast<hipStream_t>(moved) == &callers);
        Stream own;
        CHECK(own.create(1) == hipSuccess);
        own.borrow(&callers);      // the stream it owned goes, the caller's takes its place
        CHECK(g_live.empty() && static_cast<hipStream_t>(own) == &callers);
    }
    CHECK(log_is({"stream", "stream-destroy"}));

    // ---- the large-result group: all of it or none, whichever step fails --------------------------------------------------------
    for (int n = 0; n <= 3; ++n) {      // n: the allocation that fails (0: none; 3: past the last, none either)
        fresh();
        {
            BigResults<Pair, 2> big;
            g_fail_malloc_at = n;
            const hipError_t e = big.create(1, 2, 1000);
            const bool ok = n == 0 || n == 3;
            CHECK((e == hipSuccess) == ok && static_cast<bool>(big) == ok);
            if (ok) {
                CHECK(g_live.size() == 4 && big.d_res_big[0].bytes() == 1000 * sizeof(Pair) && big.d_res_big[1] && big.ev_fin);
            } else {
                CHECK(e == hipErrorOutOfMemory && g_live.empty());
                CHECK(!big.s_copy && !big.ev_fin && !big.d_res_big[0] && !big.d_res_big[1] && big.d_res_big[0].bytes() == 0);
                g_fail_malloc_at = 0;
                CHECK(big.create(1, 2, 1000) == hipSuccess && big && g_live.size() == 4);      // the next large finalize starts over
            }
        }
        CHECK(g_live.empty());
        // destruction: memory first, the stream last
        CHECK(g_log.size() >= 4 && g_log[g_log.size() - 1] == "stream-destroy" && g_log[g_log.size() - 2] == "event-destroy" &&
              g_log[g_log.size() - 3] == "free" && g_log[g_log.size() - 4] == "free");
    }
    for (int* knob : {&g_fail_stream, &g_fail_event}) {
        fresh();
        BigResults<Pair, 2> big;
        *knob = 1;
        CHECK(big.create(1, 2, 1000) == hipErrorUnknown && !big && g_live.empty() && g_malloc_calls == 0);
        *knob = 0;
    }

    // ---- a struct of owners needs no list: members go in the reverse of their order ---------------------------------------------
    fresh();
    {
        struct Holder {
            Stream s;
            Event ev;
            PinnedBuf h;
            DevBuf<float> d;
        } holder;
        CHECK(holder.s.create(0) == hipSuccess && holder.ev.create(0) == hipSuccess && holder.h.alloc(8, 0) == hipSuccess && holder.d.alloc(2) == hipSuccess);
        std::vector<Holder> grown(1);
        grown.push_back(std::move(holder));
        grown.resize(5);      // (what std::vector<fxc_pipe_slot>::resize needs: the elements move, nothing is released)
        CHECK(!holder.s && !holder.ev && !holder.h && !holder.d && g_live.size() == 4 && grown[1].d.bytes() == 2 * sizeof(float));
    }
    CHECK(log_is({"stream", "event", "host-malloc", "malloc", "free", "host-free", "event-destroy", "stream-destroy"}));
    CHECK(g_live.empty());

    if (g_failures) {
        std::fprintf(stderr, "emul_own: %d check(s) failed\n", g_failures);
        return 1;
    }
    std::puts("emul_own: ok");
    return 0;
}
