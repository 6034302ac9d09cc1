// Host traces of the fused 4096-channel kernel's exchanges -- TEST INFRASTRUCTURE ONLY (tests/test_exchange_planes.py).
// Compiles effex_amd/csrc/fx_fused4096.h with g++ and runs its own store and load functions over the 512 threads of a
// workgroup, the position of a hardware lane being wave * 64 + lane.  Nothing here is linked into libfxcorr.so.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../effex_amd/csrc/fx_fused4096.h"

using namespace fxc;
using namespace fxc::fused;

extern "C" int planes_region_dwords(void) { return kRegionBytes / 4; }
extern "C" int planes_lds_offset(int what) { return what == 0 ? kLdsRegion : (what == 1 ? kLdsWin : (what == 2 ? kLdsTw2 : kLdsBytes)); }
extern "C" int planes_branch_of_thread(int t) { return branch_of_thread(t); }
extern "C" int planes_thread_of_branch(int j) { return thread_of_branch(j); }
extern "C" int planes_sample_offset(int j, int r) { return sample_offset(j, r); }

// Exchange 1.  in[hw][16]: what hardware thread hw (= antenna * 256 + t) holds after dft16_a.  The thread runs
// phase1_finish_store under its logical id with unit twiddles; want[hw][16] = the same outputs from dft16_b (natural order);
// got[hw][16] = what phase2_load hands hardware thread hw.  owner[dword] = hardware thread that wrote it (-1: nobody,
// -2: written twice).
extern "C" void planes_exchange1(const float* in, float* want, float* got, int* owner) {
    const int ndw = kRegionBytes / 4;
    std::vector<float> region(ndw), before(ndw);
    std::vector<cf> v(kThreads * 16);
    std::memcpy(v.data(), in, sizeof(cf) * v.size());
    for (int d = 0; d < ndw; ++d) owner[d] = -1;
    for (int d = 0; d < ndw; ++d) region[d] = -1.0f - (float)d;      // (sentinels: a store shows as a changed dword)
    State st;
    state_reset_all(st);
    for (int k = 0; k < 16; ++k) st.tw1[k] = mk(1.f, 0.f);
    for (int hw = 0; hw < kThreads; ++hw) {
        cf a[16], b[16];
        for (int k = 0; k < 16; ++k) a[k] = b[k] = v[hw * 16 + k];
        dft16_b(a);
        std::memcpy(want + hw * 32, a, sizeof(a));
        before = region;
        phase1_finish_store(st, b, reinterpret_cast<cf*>(region.data()), (hw & ~255) | branch_of_thread(hw & 255));
        for (int d = 0; d < ndw; ++d)
            if (std::memcmp(&before[d], &region[d], 4) != 0) owner[d] = owner[d] == -1 ? hw : -2;
    }
    for (int hw = 0; hw < kThreads; ++hw) {
        cf o[16];
        phase2_load(reinterpret_cast<cf*>(region.data()), hw, o);
        std::memcpy(got + hw * 32, o, sizeof(o));
    }
}

// Exchange 2.  in[hw][16]: register q1 of hardware thread hw; got[hw][16]: what phase3_load hands it; owner as above.
extern "C" void planes_exchange2(const float* in, float* got, int* owner) {
    const int ndw = kRegionBytes / 4;
    std::vector<float> region(ndw), before(ndw);
    for (int d = 0; d < ndw; ++d) owner[d] = -1;
    for (int d = 0; d < ndw; ++d) region[d] = -1.0f - (float)d;
    for (int hw = 0; hw < kThreads; ++hw) {
        cf a[16];
        std::memcpy(a, in + hw * 32, sizeof(a));
        before = region;
        phase2_store(a, reinterpret_cast<cf*>(region.data()), hw);
        for (int d = 0; d < ndw; ++d)
            if (std::memcmp(&before[d], &region[d], 4) != 0) owner[d] = owner[d] == -1 ? hw : -2;
    }
    for (int hw = 0; hw < kThreads; ++hw) {
        cf o[16];
        phase3_load(reinterpret_cast<cf*>(region.data()), hw, o);
        std::memcpy(got + hw * 32, o, sizeof(o));
    }
}

// Read addresses: the region holds its own dword indices, so what a load returns is where it read.  which = 2: phase2_load,
// 3: phase3_load.  addr[hw][16][2] = dword index inside the region of the (re, im) parts of value n of hardware thread hw.
extern "C" void planes_read_addresses(int which, int* addr) {
    const int ndw = kRegionBytes / 4;
    std::vector<float> region(ndw);
    for (int d = 0; d < ndw; ++d) region[d] = (float)d;      // exact: ndw < 2^24
    for (int hw = 0; hw < kThreads; ++hw) {
        cf o[16];
        if (which == 2) phase2_load(reinterpret_cast<cf*>(region.data()), hw, o);
        else phase3_load(reinterpret_cast<cf*>(region.data()), hw, o);
        for (int n = 0; n < 16; ++n) {
            addr[(hw * 16 + n) * 2] = (int)o[n].x;
            addr[(hw * 16 + n) * 2 + 1] = (int)o[n].y;
        }
    }
}

// Window reads of the FIR with the column the kernel passes (the hardware thread): the table holds its own quad indices in
// the first tap and the frame is all ones, so v[r] = the quad read for branch r.  quad[hw][16].
extern "C" void planes_window_reads(int* quad) {
    std::vector<f4> win(kN);
    for (int q = 0; q < kN; ++q) {
        win[q].x = (float)q;
        win[q].y = win[q].z = win[q].w = 0.f;
    }
    State st;
    state_reset_all(st);
    for (int r = 0; r < 16; ++r) st.h[0][r] = mk(1.f, 0.f);
    for (int hw = 0; hw < kThreads; ++hw) {
        cf v[16];
        phase1_fir_col<0>(st, win.data(), hw & 255, v);
        for (int r = 0; r < 16; ++r) quad[hw * 16 + r] = (int)v[r].x;
    }
}
