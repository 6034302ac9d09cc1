// Developer micro-benchmark: the two LDS exchanges of the fused 4096-channel kernel, as they are and with
// lane-addressed stores (ds_write_addtid_b32: address = M0 + immediate + 4 * lane, no address register) into component
// planes.  One 512-thread workgroup per CU (140 KiB of dynamic LDS pins it: two waves per SIMD, the kernel's occupancy),
// sixteen complex values per thread and round; what a round reads is what the next round stores.
//   exchange_forms [rounds] [repeats]
// arms, each timed as ns per round per CU:
//   a  exchange 1 today:   16 ds_write_b64 at row pitch 272, barrier, 16 ds_read_b64, barrier
//   b  exchange 1 planes:  32 ds_write_addtid_b32, barrier, 16 ds_read_b64 from the planes, barrier
//   c  exchange 2 today:   8 ds_write2_b64, wave-local, 16 ds_read_b64
//   d  exchange 2 planes:  32 ds_write_addtid_b32, wave-local, 16 ds_read_b64
// Before the timing every arm runs one round on tagged values and each lane checks that it read the values of the
// lanes it should (a mismatch is an error: exit status 1).
// hipcc --offload-arch=gfx950 -O3 -o exchange_forms exchange_forms.hip
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef float2 cf;
constexpr int kThreads = 512;
constexpr int kPin = 140 * 1024;          // dynamic LDS: one workgroup per CU
constexpr int kRowPitch = 272;            // today's region, in cf
constexpr int kRegion = 16 * kRowPitch;
constexpr int kPlaneRow = 288;            // planes, in dwords: [antenna][re, im][k1 row]
constexpr int kPlane = 16 * kPlaneRow;    // 4 608
constexpr int kAntPlanes = 2 * kPlane;    // 9 216

__device__ __forceinline__ cf lds_load(const cf* p) {
    typedef const volatile __attribute__((address_space(3))) unsigned long long* lds_u64_ptr;
    const unsigned long long u = *(lds_u64_ptr)(p);
    return cf{__uint_as_float((unsigned)(u & 0xffffffffull)), __uint_as_float((unsigned)(u >> 32))};
}

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// one dword per lane to LDS byte address m0 + OFF + 4 * lane
template <int OFF>
__device__ __forceinline__ void store_addtid(float v, unsigned m0) {
    static_assert(OFF >= 0 && OFF < 65536, "16-bit immediate");
    asm volatile("ds_write_addtid_b32 %0 offset:%1" : : "v"(v), "n"(OFF), "{m0}"(m0) : "memory");
}
// an SALU write of M0 needs one wait state before a lane-addressed store reads it; the compiler does not look inside the
// stores' asm, so this goes between its write of M0 and the first of them
__device__ __forceinline__ void m0_settle(unsigned m0) { asm volatile("s_nop 0" : : "{m0}"(m0)); }
__device__ __forceinline__ void lds_drain() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

template <int K>
struct Unroll {
    template <typename F>
    __device__ __forceinline__ static void run(F&& f) {
        Unroll<K - 1>::run(f);
        f(std::integral_constant<int, K - 1>{});
    }
};
template <>
struct Unroll<0> {
    template <typename F>
    __device__ __forceinline__ static void run(F&&) {}
};

// phase-1 thread -> branch map that goes with the planes: lane bit 0 carries bit 4 of j
__device__ __forceinline__ int branch_of(int t) {
    const int l = t & 63, wv = t >> 6;
    return ((l >> 1) & 15) + 16 * ((l & 1) | ((l >> 5) << 1) | (wv << 2));
}

// value tag: (source thread, register); exact in float32
__device__ __forceinline__ cf tag(int tid, int k) { return cf{(float)(tid * 16 + k), -(float)(tid * 16 + k) - 0.5f}; }

template <int ARM>
__global__ __launch_bounds__(kThreads) void exchange_k(float* out, int rounds, int* bad) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    typedef __attribute__((address_space(3))) unsigned char* lptr_t;
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(lptr_t)smem);
    cf* region = reinterpret_cast<cf*>(smem);
    float* planes = reinterpret_cast<float*>(smem);
    const int tid = threadIdx.x, l = tid & 63, wave = tid >> 6, ant = tid >> 8, wv = wave & 3;
    const int ant2 = l >> 5, k1r = 2 * wave + ((l >> 4) & 1), lo = l & 15;       // this lane's antenna, row and j0 / q1 in phases 2, 3
    const bool verify = bad != nullptr;
    cf v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = tag(tid, k);

    for (int it = 0; it < rounds; ++it) {
        if (ARM == 0) {
            cf* mine = region + ant * kRegion + (tid & 255);
#pragma unroll
            for (int k1 = 0; k1 < 16; ++k1) mine[k1 * kRowPitch] = v[k1];
            __syncthreads();
            const cf* row = region + ant2 * kRegion + k1r * kRowPitch;
#pragma unroll
            for (int j1 = 0; j1 < 16; ++j1) v[j1] = lds_load(row + lo + 16 * j1);
            __syncthreads();
        } else if (ARM == 1) {
            const unsigned m0 = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)(ant * kAntPlanes * 4 + wv * 256));
            m0_settle(m0);
            Unroll<16>::run([&](auto k1) {
                store_addtid<k1() * kPlaneRow * 4>(v[k1()].x, m0);
                store_addtid<(kPlane + k1() * kPlaneRow) * 4>(v[k1()].y, m0);
            });
            lds_drain();
            __syncthreads();
            const float* row = planes + ant2 * kAntPlanes + k1r * kPlaneRow + 2 * lo;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const cf re = lds_load(reinterpret_cast<const cf*>(row + 32 * u));
                const cf im = lds_load(reinterpret_cast<const cf*>(row + kPlane + 32 * u));
                v[2 * u] = cf{re.x, im.x};
                v[2 * u + 1] = cf{re.y, im.y};
            }
            __syncthreads();
        } else if (ARM == 2) {
            cf* row = region + ant2 * kRegion + k1r * kRowPitch;
            wave_sync();
#pragma unroll
            for (int q1 = 0; q1 < 16; ++q1) row[q1 * 17 + lo] = v[q1];
            wave_sync();
#pragma unroll
            for (int j0 = 0; j0 < 16; ++j0) v[j0] = lds_load(row + lo * 17 + j0);
        } else {
            const unsigned m0 = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)(wave * 2 * kPlaneRow * 4));
            wave_sync();
            m0_settle(m0);
            Unroll<16>::run([&](auto q1) {
                constexpr int off = ((q1() >> 3) * (kPlane + 32) + (q1() & 7) * 66) * 4;
                store_addtid<off>(v[q1()].x, m0);
                store_addtid<off + kAntPlanes * 4>(v[q1()].y, m0);
            });
            lds_drain();
            wave_sync();
            const float* row = planes + wave * 2 * kPlaneRow + (lo >> 3) * (kPlane + 32) + (lo & 7) * 66 + (l >> 4) * 16;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const cf re = lds_load(reinterpret_cast<const cf*>(row + 2 * u));
                const cf im = lds_load(reinterpret_cast<const cf*>(row + kAntPlanes + 2 * u));
                v[2 * u] = cf{re.x, im.x};
                v[2 * u + 1] = cf{re.y, im.y};
            }
        }
        if (verify) {      // one round: value n of this lane came from ...
            int wrong = 0;
#pragma unroll
            for (int n = 0; n < 16; ++n) {
                cf want;
                if (ARM == 0) want = tag(ant2 * 256 + lo + 16 * n, k1r);                  // branch j0 + 16 j1, linear map
                else if (ARM == 1) {                                                      // the thread whose branch is j0 + 16 j1
                    const int t = 32 * (n >> 1) + 2 * lo + (n & 1);
                    if (branch_of(t) != lo + 16 * n) ++wrong;
                    want = tag(ant2 * 256 + t, k1r);
                } else want = tag((tid & ~15) + n, lo);                                   // lane j0 of the 16-lane group, register q1
                if (v[n].x != want.x || v[n].y != want.y) ++wrong;
            }
            if (wrong) atomicAdd(bad, wrong);
        }
    }
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += v[k].x + v[k].y;
    out[(blockIdx.x & 255) * kThreads + tid] = s;
}

typedef void (*kern_t)(float*, int, int*);

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 200000;
    const int repeats = argc > 2 ? atoi(argv[2]) : 7;
    const kern_t kerns[4] = {exchange_k<0>, exchange_k<1>, exchange_k<2>, exchange_k<3>};
    const char* names[4] = {"a exchange 1 today  (16 ds_write_b64, barriers)",
                            "b exchange 1 planes (32 ds_write_addtid_b32, barriers)",
                            "c exchange 2 today  (8 ds_write2_b64, wave-local)",
                            "d exchange 2 planes (32 ds_write_addtid_b32, wave-local)"};
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) != hipSuccess) { printf("no device\n"); return 2; }
    const int cus = prop.multiProcessorCount;
    float* out;
    int* bad;
    if (hipMalloc(&out, 256 * kThreads * 4) != hipSuccess || hipMalloc(&bad, 4) != hipSuccess) return 2;
    for (int a = 0; a < 4; ++a)
        if (hipFuncSetAttribute((const void*)kerns[a], hipFuncAttributeMaxDynamicSharedMemorySize, kPin) != hipSuccess) return 2;

    for (int a = 0; a < 4; ++a) {
        hipMemset(bad, 0, 4);
        hipLaunchKernelGGL(kerns[a], dim3(cus), dim3(kThreads), kPin, 0, out, 1, bad);
        int h = -1;
        if (hipMemcpy(&h, bad, 4, hipMemcpyDeviceToHost) != hipSuccess) { printf("arm %c: launch failed\n", 'a' + a); return 2; }
        printf("verify %c: %d wrong values\n", 'a' + a, h);
        if (h != 0) return 1;
    }

    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    std::vector<double> ns[4];
    for (int a = 0; a < 4; ++a) hipLaunchKernelGGL(kerns[a], dim3(cus), dim3(kThreads), kPin, 0, out, rounds, (int*)nullptr);   // warm-up
    for (int r = 0; r < repeats; ++r)
        for (int a = 0; a < 4; ++a) {     // arms alternate inside a repeat: drift hits all of them alike
            hipEventRecord(e0, 0);
            hipLaunchKernelGGL(kerns[a], dim3(cus), dim3(kThreads), kPin, 0, out, rounds, (int*)nullptr);
            hipEventRecord(e1, 0);
            if (hipEventSynchronize(e1) != hipSuccess) { printf("arm %c failed\n", 'a' + a); return 2; }
            float ms;
            hipEventElapsedTime(&ms, e0, e1);
            ns[a].push_back(ms * 1e6 / rounds);
        }
    printf("%d CUs, %d rounds per launch, %d launches per arm; ns per round per CU: min median max\n", cus, rounds, repeats);
    for (int a = 0; a < 4; ++a) {
        std::sort(ns[a].begin(), ns[a].end());
        printf("%-58s %8.2f %8.2f %8.2f\n", names[a], ns[a].front(), ns[a][ns[a].size() / 2], ns[a].back());
    }
    return 0;
}
