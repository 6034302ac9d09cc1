// fx_fused4096.h — per-thread phases of the fused 2-antenna F+X kernel for nchan = 4096, ntaps = 4.
//
// One 512-thread workgroup (8 waves, one per CU) walks whole chunks; per spectrum i it
//   phase 1  (thread = antenna h, branch set {j + 256 r}):  4-tap PFB FIR over a ring of four frames
//            held in VGPRs (every IQ sample is fetched from HBM exactly once; the frame loop is
//            unrolled by four so the ring rotates by renaming, not by moves),
//            radix-16 over r, twiddle w4096^(j*k1), exchange 1 through LDS        [s_barrier]
//            (hardware thread t of an antenna owns branch set j = branch_of_thread(t), not t: see "exchanges" below)
//   phase 2  (lane = antenna, k1, j0):  radix-16 over j1, twiddle w256^(j0*q1), exchange 2 —
//            a 16x16 transpose that stays inside one wave (no s_barrier)
//   phase 3  (lane = antenna, k1, q1):  radix-16 over j0 -> bins k = k1 + 16 q1 + 256 q2;
//            v_permlane32_swap pairs antenna 0 (lanes 0-31) with antenna 1 (lanes 32-63) so every
//            lane multiplies-and-accumulates 8 bins of  spec0 * conj(spec1).
// FFT decomposition (kernel exp(+2 pi i m k / 4096)):
//   m = j + 256 r,  j = j0 + 16 j1,  k = k1 + 16 q1 + 256 q2
//   w^(mk) = w16^(r k1) * w4096^(j k1) * w16^(j1 q1) * w256^(j0 q1) * w16^(j0 q2)
//
// Exchanges: both go through component planes of the region -- dwords [antenna][re, im][k1 row of kPlaneRow] -- and are
// stored with ds_write_addtid_b32 (LDS address = M0 + immediate + 4 * lane: no address register, 2 cycles of the
// register-to-LDS path per 4 bytes where ds_write_b64 takes 6 per 8 and ds_write2_b64 13 per 16).  A lane-addressed store
// puts a wave's 64 values side by side, so the map of phase 1 is chosen such that side by side is where phase 2 wants them:
// lane bit 0 carries bit 4 of j, and the two points j1 = 2u, 2u + 1 of a phase-2 lane are one ds_read_b64 of a plane.
// Exchange 2 (a 16x16 transpose inside every 16-lane group) needs no such map: its two points j0 = 2u, 2u + 1 are
// neighbouring lanes already.  The functions below keep taking the *logical* thread id (antenna << 8) | j for phase 1
// and the hardware thread id for phases 2 and 3; under g++ a store writes the dword the hardware lane would.
//
// The same source is compiled by g++ in tests/emul (host emulation of the index logic; test
// infrastructure only — the shipped library contains only the device build).
#pragma once
#include "fx_math.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define FXC_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define FXC_SCHED_FENCE() ((void)0)
#endif

namespace fxc {
namespace fused {

// One 8-byte LDS read that the compiler will not pair into ds_read2_b64 (half the LDS rate of
// ds_read_b64 on gfx950, MI355X_MICROARCH.md §LDS).
FX_HD cf lds_load(const cf* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const volatile __attribute__((address_space(3))) unsigned long long* lds_u64_ptr;
    const unsigned long long u = *(lds_u64_ptr)(p);
    cf r;
    r.x = __uint_as_float((unsigned)(u & 0xffffffffull));
    r.y = __uint_as_float((unsigned)(u >> 32));
    return r;
#else
    return *p;
#endif
}

// One 16-byte LDS read that stays where the source puts it: the compiler moves plain reads of the window table up past
// FXC_SCHED_FENCE() (all sixteen quads of a step in flight, 64 VGPRs); a volatile read keeps its place among the fences.
FX_HD f4 lds_load4(const f4* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef float lds_v4f __attribute__((ext_vector_type(4)));
    typedef const volatile __attribute__((address_space(3))) lds_v4f* lds_v4f_ptr;
    const lds_v4f u = *(lds_v4f_ptr)(p);
    f4 r;
    r.x = u[0]; r.y = u[1]; r.z = u[2]; r.w = u[3];
    return r;
#else
    return *p;
#endif
}

constexpr int kN = 4096;
constexpr int kT = 4;
constexpr int kThreads = 512;
constexpr int kPlaneRow = 288;              // dwords per k1 row of a plane: 256 columns + 32; == 32 (mod 64) keeps ds_read_b64 conflict-free
constexpr int kPlane = 16 * kPlaneRow;      // dwords per component plane
constexpr int kAntPlanes = 2 * kPlane;      // dwords per antenna: re plane, im plane
constexpr int kRegionBytes = 2 * kAntPlanes * 4;
constexpr int kAccPerThread = 8;
#ifndef FXC_FIR_GROUP
#define FXC_FIR_GROUP 4
#endif
constexpr int kFirGroup = FXC_FIR_GROUP;    // branches per software-pipeline group of the FIR's window reads

// LDS carve (bytes); every offset is a multiple of 16
// (the region comes first: the base of a lane-addressed store is the 16-bit M0 offset, so it has to lie below 64 KiB --
// also behind the 20 KiB of static LDS of the DCK variant)
constexpr int kLdsRegion = 0;                                // float[2][2][kPlane]
constexpr int kLdsWin = kLdsRegion + kRegionBytes;           // f4[4096]   window, [r*256 + col] = h[t*N + j + 256 r], t = x,y,z,w;
                                                             //            col = j for the header's own callers, the hardware thread in the kernel
constexpr int kLdsTw2 = kLdsWin + kN * 16;                   // cf[256]    w256^(j0*q1) at [q1*16 + j0]
constexpr int kLdsBytes = kLdsTw2 + 256 * 8;

// phase 1: hardware thread t (0..255 within its antenna; lane l = t & 63, wave wv = t >> 6) <-> branch set j
FX_HD int branch_of_thread(int t) {
    const int l = t & 63, wv = (t >> 6) & 3;
    return ((l >> 1) & 15) + 16 * ((l & 1) | ((l >> 5) << 1) | (wv << 2));
}
FX_HD int thread_of_branch(int j) { return ((j >> 4) & 1) | ((j & 15) << 1) | (j & 0xE0); }

// Lane-addressed stores of one wave: dword `base_dw + DW + lane` of the region.  Device: base in M0 (written once; an SALU
// write of M0 needs a wait state before such a store reads it, and the compiler does not look inside the asm), one
// ds_write_addtid_b32 per call.  The compiler does not count these stores: lane_store_end() waits for them (uncounted LDS
// operations in the queue only make the compiler's own lgkmcnt waits stricter: LDS operations return in order).
struct LaneStore {
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned m0;
#else
    float* at;
#endif
};

FX_HD LaneStore lane_store_begin(cf* region, int base_dw, int lane) {
    LaneStore ls;
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(3))) cf* lptr_t;
    (void)lane;
    ls.m0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(lptr_t)region + 4u * (unsigned)base_dw);
    asm volatile("s_nop 0" : : "{m0}"(ls.m0));
#else
    ls.at = reinterpret_cast<float*>(region) + base_dw + lane;
#endif
    return ls;
}

template <int DW>
FX_HD void lane_store(const LaneStore& ls, float val) {
    static_assert(DW >= 0 && 4 * DW < 65536, "16-bit immediate");
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("ds_write_addtid_b32 %0 offset:%1" : : "v"(val), "n"(4 * DW), "{m0}"(ls.m0));
#else
    ls.at[DW] = val;
#endif
}

FX_HD void lane_store_end() {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_waitcnt lgkmcnt(0)" : : : "memory");
#endif
}

// dft16_b_stream (fx_math.h) with the output index as a type, for the stores' immediates
template <int K>
struct KConst { static constexpr int value = K; };
template <class Sink>
FX_HD void dft16_b_stream_ct(cf (&v)[16], Sink&& sink) {
    dft4(v[0], v[1], v[2], v[3]);
    sink(KConst<0>{}, v[0]); sink(KConst<4>{}, v[1]); sink(KConst<8>{}, v[2]); sink(KConst<12>{}, v[3]);
    dft4_scaled_c_bd(v[4], v[5], v[6], v[7]);
    sink(KConst<1>{}, v[4]); sink(KConst<5>{}, v[5]); sink(KConst<9>{}, v[6]); sink(KConst<13>{}, v[7]);
    dft4_bd_scaled(v[8], v[9], v[10], v[11]);
    sink(KConst<2>{}, v[8]); sink(KConst<6>{}, v[9]); sink(KConst<10>{}, v[10]); sink(KConst<14>{}, v[11]);
    dft4_scaled_c_bd(v[12], v[13], v[14], v[15]);
    sink(KConst<3>{}, v[12]); sink(KConst<7>{}, v[13]); sink(KConst<11>{}, v[14]); sink(KConst<15>{}, v[15]);
}

struct State {
    // ring of four frames of this thread's 16 branch samples: slot PH holds the frame being
    // channelised, the other three the PFB history (and, once dead, the prefetch of the next frame)
    cf h[4][16];
    cf tw1[16];                  // w4096^(j*k1), k1 = 1..15 ([0] unused): 15 twiddles in 30 VGPRs beat 6 stored
                                 // powers + 9 extra complex multiplies (the kernel is limited by energy per spectrum)
    cf acc[kAccPerThread];       // sum_i spec0*conj(spec1) for this lane's 8 bins
    cf tw2[16];                  // w256^(j0*q1) of this lane's j0, q1 = 1..kTw2Resident (the rest unused): only the kernel's default
                                 // instantiation loads them (state_load_twiddles2) -- every other user reads the LDS table each step
};

// zero PFB history at the start of every chunk; the chunk's frame 0 sits in slot PH
template <int PH>
FX_HD void state_reset_history(State& s) {
#pragma unroll
    for (int d = 1; d < 4; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) s.h[(PH + d) & 3][r] = mk(0.f, 0.f);
}

FX_HD void state_reset_all(State& s) {
    state_reset_history<0>(s);
#pragma unroll
    for (int q = 0; q < kAccPerThread; ++q) s.acc[q] = mk(0.f, 0.f);
}

// Work split of one launch (fxcorr.hip::fx_fused4096_kernel) over g workgroups, in two parts:
//   rounds  the first n_full = rounds * g * seg chunks go out whole, in segments of `seg` consecutive chunks dealt
//           round-robin (workgroup b: segments b, b + g, b + 2g, ...): at any moment the g workgroups stream from one
//           compact window of g * seg chunks and start their chunks together (measured on 10 000 chunk pairs:
//           seg = 1 8.82 ms, seg = 39 8.94 ms, everything as frame ranges 8.92 ms);
//   tail    the remaining n_chunks - n_full chunks form one sequence of frames and workgroup b takes the contiguous
//           range [range_begin(b), range_begin(b + 1)) of it, chunk boundaries or not, so that every workgroup gets
//           the same number of frames (+-1) whatever n_chunks % g is.  A range that starts inside a chunk reloads the
//           (up to) three frames of PFB history before it.
// Raw rows (float32 sums of spectrum products): a row collects `unit` chunks finished in a row by one workgroup.
//   rows_are_chunks (unit = 1): row c = chunk c.  A tail chunk shared by several workgroups: the one that owns its
//   first frame writes row c, every other one its share into its leading-part row n_chunks + b (zeros if none).
//   otherwise (integration only): rounds part row b + g * j for workgroup b's j-th row, then one row per tail chunk
//   and the g leading-part rows; the sum of all range_rows() rows is the integration.
struct RangeWalk {
    int c, i;            // chunk and frame of the spectrum being computed
    int left;            // frames of this part still to do, this one included
    int row;             // raw row the sums in progress go to
    int n_pts;
    int seg, seg_left;   // chunks per segment; chunks of the current segment still to finish, this one included
    int seg_jump;        // chunks skipped at a segment end: (g - 1) * seg
    int unit, in_row;    // whole chunks per row; chunks finished in the row in progress
    int row_step;        // rows that are not chunks: next row = row + row_step
    int row_off;         // rows that are chunks: row = c + row_off
    bool rows_are_chunks;
    bool lead;                 // tail: the range starts inside a chunk
};

struct RangeSplit {
    int rounds, n_full, n_tail, rows_rounds, n_rows;   // n_rows: rows in all, leading-part rows included
};

FX_HD RangeSplit range_split(int g, int n_chunks, int seg, int unit, bool rows_are_chunks) {
    RangeSplit r;
    r.rounds = n_chunks / (g * seg);
    r.n_full = r.rounds * g * seg;
    r.n_tail = n_chunks - r.n_full;
    r.rows_rounds = rows_are_chunks ? r.n_full : g * ((r.rounds * seg + unit - 1) / unit);
    r.n_rows = r.rows_rounds + r.n_tail + g;
    return r;
}

FX_HD RangeWalk range_walk_rounds(int b, int g, int n_chunks, int n_pts, int seg,
                                   int unit, bool rows_are_chunks) {
    const RangeSplit sp = range_split(g, n_chunks, seg, unit, rows_are_chunks);
    RangeWalk w;
    w.c = b * seg;
    w.i = 0;
    w.left = sp.rounds * seg * n_pts;
    w.n_pts = n_pts;
    w.seg = w.seg_left = seg;
    w.seg_jump = (g - 1) * seg;
    w.unit = rows_are_chunks ? 1 : unit;
    w.in_row = 0;
    w.rows_are_chunks = rows_are_chunks;
    w.row_off = 0;
    w.row_step = g;
    w.row = rows_are_chunks ? w.c : b;
    w.lead = false;
    return w;
}

FX_HD RangeWalk range_walk_tail(int b, int g, int n_chunks, int n_pts, int seg,
                                 int unit, bool rows_are_chunks) {
    const RangeSplit sp = range_split(g, n_chunks, seg, unit, rows_are_chunks);
    RangeWalk w;
    const int n_frames = sp.n_tail * n_pts;
    const int f0 = range_begin(b, n_frames, g);
    w.left = range_begin(b + 1, n_frames, g) - f0;
    w.c = sp.n_full + f0 / n_pts;
    w.i = f0 % n_pts;
    w.n_pts = n_pts;
    w.seg = 1;
    w.seg_left = 1;
    w.seg_jump = 0;
    w.unit = 1;
    w.in_row = 0;
    w.rows_are_chunks = true;
    w.row_off = sp.rows_rounds - sp.n_full;
    w.row_step = 0;
    w.lead = w.i != 0;
    w.row = w.lead ? sp.rows_rounds + sp.n_tail + b : w.c + w.row_off;
    return w;
}

// the spectrum of (c, i) is the last one of the row in progress: last frame of the part, or of the row's last chunk
FX_HD bool range_walk_row_ends(const RangeWalk& w) {
    return w.left == 1 || (w.i + 1 == w.n_pts && w.in_row + 1 == w.unit);
}

// the frame to fetch while (c, i) is computed: the next one of the part (next frame of the chunk or frame 0 of the
// next chunk); at the very end of the part the current frame again (never used)
FX_HD void range_walk_prefetch(const RangeWalk& w, int& pc, int& pi) {
    pc = w.c;
    pi = w.i;
    if (w.left > 1 && ++pi == w.n_pts) {
        pi = 0;
        pc += 1 + (w.seg_left == 1 ? w.seg_jump : 0);
    }
}

// move on to the next frame of the part; call after the row store when range_walk_row_ends()
FX_HD void range_walk_advance(RangeWalk& w, bool row_ended) {
    if (++w.i == w.n_pts) {
        w.i = 0;
        w.c += 1;
        if (--w.seg_left == 0) {
            w.c += w.seg_jump;
            w.seg_left = w.seg;
        }
        w.in_row += 1;
    }
    w.left -= 1;
    if (row_ended) {
        w.in_row = 0;
        w.row = w.rows_are_chunks ? w.c + w.row_off : w.row + w.row_step;
    }
}

// element offset (in cf) inside one frame of the sample this thread feeds to branch j + 256 r
FX_HD int sample_offset(int j, int r) { return (kN - 1) - j - 256 * r; }

// phase 1a for a frame in ring slot PH: 4-tap FIR (taps t = 0..3 on frames i, i-1, i-2, i-3, summed
// in that order); result left in v[r]
// G: branches per group (the kernel's AUTOS variant takes 2: 16 VGPRs fewer quads in flight, for its power sums)
// col: this thread's column of the window table (see kLdsWin)
// PIN: the window reads keep their place between the fences (lds_load4): two groups of quads in flight, no more -- the kernel's
// default instantiation, whose resident w256 twiddles take registers the other quads would
template <int PH, int G = kFirGroup, bool PIN = false>
FX_HD void phase1_fir_col(const State& s, const f4* win, int col, cf (&v)[16]) {
    const int j = col;
    const cf (&x0)[16] = s.h[PH];
    const cf (&x1)[16] = s.h[(PH + 3) & 3];
    const cf (&x2)[16] = s.h[(PH + 2) & 3];
    const cf (&x3)[16] = s.h[(PH + 1) & 3];
    // software-pipelined in groups of kFirGroup branches: the window quads of group g + 1 are requested from LDS
    // before group g is computed, so only the first ds_read latency is exposed (2 * kFirGroup * 4 VGPRs of quads in
    // flight at the kernel's point of highest register pressure)
    constexpr int NG = 16 / G;
    f4 w[2][G];
#pragma unroll
    for (int q = 0; q < G; ++q) w[0][q] = PIN ? lds_load4(win + q * 256 + j) : win[q * 256 + j];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        if (g < NG - 1) {
#pragma unroll
            for (int q = 0; q < G; ++q) {
                const f4* at = win + (G * (g + 1) + q) * 256 + j;
                w[(g + 1) & 1][q] = PIN ? lds_load4(at) : *at;
            }
        }
        FXC_SCHED_FENCE();
#pragma unroll
        for (int q = 0; q < G; ++q) {
            const int r = G * g + q;
            const f4 t = w[g & 1][q];
            cf a = cscale(x0[r], t.x);
            a = cfma(t.y, x1[r], a);
            a = cfma(t.z, x2[r], a);
            v[r] = cfma(t.w, x3[r], a);
        }
#if defined(__HIP_DEVICE_COMPILE__)
        if (PIN) {      // the group's results exist before the next reads go out: an empty statement the reads cannot pass
#pragma unroll
            for (int q = 0; q < G; ++q) asm volatile("" : "+v"(v[G * g + q].x), "+v"(v[G * g + q].y));
        }
#endif
        FXC_SCHED_FENCE();
    }
}

template <int PH, int G = kFirGroup>
FX_HD void phase1_fir(const State& s, const f4* win, int tid, cf (&v)[16]) {
    phase1_fir_col<PH, G>(s, win, tid & 255, v);
}

// phase 1b: the second half of the radix-16 over r (dft16_b) with each output twiddled by w4096^(j*k1) and stored to
// exchange 1 as soon as it exists -- the stores are bound by the register-to-LDS path (64 KiB at ~128 B/clk per CU), and the
// 72 + 60 vector instructions of the butterflies and twiddles run in its shadow instead of in front of barrier B0.
// Call after dft16_a(v).
// LEAN_TW (the kernel's AUTOS variant): of the fifteen twiddles only w4096^(j k1) for k1 = 1, 2, 4, 8 live in registers across
// frames -- the others are their products, formed here per frame (11 complex multiplies, shared subexpressions; the powers pass
// through an empty asm so that the products cannot be hoisted out of the frame loop, where they would take the registers back)
// -- and the 22 VGPRs so freed hold the variant's power sums.
FX_HD cf tw1_of(const cf (&pw2)[4], int k1) {
    cf w = mk(1.f, 0.f);
    bool have = false;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        if (k1 & (1 << b)) {
            w = have ? cmul(w, pw2[b]) : pw2[b];
            have = true;
        }
    }
    return w;
}

// tid: the logical id (antenna << 8) | j.  Wave wv of antenna h stores at columns 64 wv .. 64 wv + 63 of every row of h's planes
template <bool LEAN_TW = false>
FX_HD void phase1_finish_store(const State& s, cf (&v)[16], cf* region, int tid) {
    const int t = thread_of_branch(tid & 255);
    const LaneStore ls = lane_store_begin(region, (tid >> 8) * kAntPlanes + (t & 0xC0), t & 63);
    cf pw2[4] = {s.tw1[1], s.tw1[2], s.tw1[4], s.tw1[8]};
#if defined(__HIP_DEVICE_COMPILE__)
    if (LEAN_TW) {
#pragma unroll
        for (int b = 0; b < 4; ++b) asm volatile("" : "+v"(pw2[b].x), "+v"(pw2[b].y));
    }
#endif
    dft16_b_stream_ct(v, [&](auto k, cf val) {
        constexpr int k1 = decltype(k)::value;
        if (k1 > 0) val = cmul(val, LEAN_TW ? tw1_of(pw2, k1) : s.tw1[k1]);
        lane_store<k1 * kPlaneRow>(ls, val.x);
        lane_store<kPlane + k1 * kPlaneRow>(ls, val.y);
    });
    lane_store_end();
}

// load this thread's twiddles from the [16][256] table w4096^(j*k1)
FX_HD void state_load_twiddles(State& s, const cf* tw1_table, int tid) {
    const int j = tid & 255;
#pragma unroll
    for (int k1 = 0; k1 < 16; ++k1) s.tw1[k1] = tw1_table[k1 * 256 + j];
}

// phase 2, lane = (antenna, k1, j0): the points j1 = 2u, 2u + 1 sit side by side in row k1 of the antenna's planes
// (columns 32 u + 2 j0 + {0, 1}: the hardware threads whose branch sets are j0 + 16 j1)
FX_HD void phase2_load(cf* region, int tid, cf (&v)[16]) {
    const int l = tid & 63, wave = tid >> 6;
    const int ant = l >> 5, k1 = 2 * wave + ((l >> 4) & 1), j0 = l & 15;
    const float* row = reinterpret_cast<const float*>(region) + ant * kAntPlanes + k1 * kPlaneRow + 2 * j0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const cf re = lds_load(reinterpret_cast<const cf*>(row + 32 * u));
        const cf im = lds_load(reinterpret_cast<const cf*>(row + kPlane + 32 * u));
        v[2 * u] = mk(re.x, im.x);
        v[2 * u + 1] = mk(re.y, im.y);
    }
}

FX_HD void phase2_twiddle(cf (&v)[16], const cf* tw2, int tid) {
    const int j0 = tid & 15;
    // same pipelining for the w256^(j0*q1) table: group g + 1 is in flight while group g multiplies
    cf t[2][4];
#pragma unroll
    for (int q = 1; q < 4; ++q) t[0][q] = lds_load(tw2 + q * 16 + j0);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        if (g < 3) {
#pragma unroll
            for (int q = 0; q < 4; ++q) t[(g + 1) & 1][q] = lds_load(tw2 + (4 * (g + 1) + q) * 16 + j0);
        }
        FXC_SCHED_FENCE();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int q1 = 4 * g + q;
            if (q1 > 0) v[q1] = cmul(v[q1], t[g & 1][q]);
        }
        FXC_SCHED_FENCE();
    }
}

// The same twiddles held in registers across frames (State::tw2): loaded once per launch, the same cmul with the same operands
// in the same order as phase2_twiddle -- bit-identical, without their ds_read_b64 every step
// How many of them: q1 = 1 .. kTw2Resident come from State::tw2, the others from the LDS table as before.  Ten is what the kernel's
// budget of 248 VGPRs (tests/test_autos_host.py) holds without scratch: every further twiddle is two registers more, all fifteen 256
#ifndef FXC_TW2_RESIDENT
#define FXC_TW2_RESIDENT 10
#endif
constexpr int kTw2Resident = FXC_TW2_RESIDENT;
static_assert(kTw2Resident >= 0 && kTw2Resident <= 15, "q1 = 1 .. 15");
FX_HD void state_load_twiddles2(State& s, const cf* tw2_table, int tid) {
    const int j0 = tid & 15;
#pragma unroll
    for (int q1 = 1; q1 <= kTw2Resident; ++q1) s.tw2[q1] = tw2_table[q1 * 16 + j0];
}

// fetch: the twiddles that are not resident, requested from the LDS table ahead of the radix-16 they follow, so that the reads'
// latency passes behind its butterflies (read right before their use, as phase2_twiddle does, the wave waits for them)
FX_HD void phase2_twiddle_fetch(cf (&t)[16], const cf* tw2, int tid) {
    const int j0 = tid & 15;
#pragma unroll
    for (int q1 = kTw2Resident + 1; q1 < 16; ++q1) t[q1] = lds_load(tw2 + q1 * 16 + j0);
}

// cmul with its two fused multiply-adds spelled out, as the compiler contracts phase2_twiddle's cmul: left to itself it picks the
// other product of the imaginary part for some of the fetched twiddles, and the last bit of 3 in 16 bins changes
FX_HD cf cmul_tw(cf a, cf b) {
    return mk(__builtin_fmaf(a.x, b.x, -(a.y * b.y)), __builtin_fmaf(a.y, b.x, a.x * b.y));
}

FX_HD void phase2_twiddle_reg(cf (&v)[16], const State& s, const cf (&t)[16]) {
#pragma unroll
    for (int q1 = 1; q1 <= kTw2Resident; ++q1) v[q1] = cmul_tw(v[q1], s.tw2[q1]);
#pragma unroll
    for (int q1 = kTw2Resident + 1; q1 < 16; ++q1) v[q1] = cmul_tw(v[q1], t[q1]);
}

// Exchange 2, wave-local: wave w reuses rows 2 w, 2 w + 1 of the four planes -- the rows its own phase 2 read, nobody
// else's.  Component c of register q1 goes to stripe stripe_of(q1) + c * kAntPlanes of the wave's area, a stripe being the
// wave's 64 lanes side by side: the real parts of q1 = 0..7 lie 66 dwords apart in what was antenna 0's re plane, those of
// q1 = 8..15 in its im plane, 32 dwords further on (so that the 32 lanes of a half-wave read 64 distinct banks), the
// imaginary parts the same in antenna 1's planes
constexpr int kStripeHi = kPlane + 32;
constexpr int stripe_of(int q1) { return (q1 >> 3) * kStripeHi + (q1 & 7) * 66; }

template <int Q1>
FX_HD void phase2_store_from(const LaneStore& ls, const cf (&v)[16]) {
    lane_store<stripe_of(Q1)>(ls, v[Q1].x);
    lane_store<stripe_of(Q1) + kAntPlanes>(ls, v[Q1].y);
    if constexpr (Q1 < 15) phase2_store_from<Q1 + 1>(ls, v);
}

FX_HD void phase2_store(const cf (&v)[16], cf* region, int tid) {
    const LaneStore ls = lane_store_begin(region, (tid >> 6) * 2 * kPlaneRow, tid & 63);
    phase2_store_from<0>(ls, v);
    lane_store_end();
}

// phase 3, lane = (antenna, k1, q1): the points j0 = 2u, 2u + 1 of its 16-lane group, side by side in stripe q1
FX_HD void phase3_load(cf* region, int tid, cf (&v)[16]) {
    const int l = tid & 63, wave = tid >> 6, q1 = l & 15;
    const float* row = reinterpret_cast<const float*>(region) + wave * 2 * kPlaneRow + stripe_of(q1) + (l >> 4) * 16;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const cf re = lds_load(reinterpret_cast<const cf*>(row + 2 * u));
        const cf im = lds_load(reinterpret_cast<const cf*>(row + kAntPlanes + 2 * u));
        v[2 * u] = mk(re.x, im.x);
        v[2 * u + 1] = mk(re.y, im.y);
    }
}

// X-stage on paired data: a = antenna 0, b = antenna 1 for this lane's bin q (lanes 0-31) or
// q + 8 (lanes 32-63) — effex/effex.py:520 without rot (applied once at finalize)
FX_HD void xacc(State& s, int q, cf a, cf b) { s.acc[q] = cmulc_acc(s.acc[q], a, b); }

// natural bin index of accumulator q of thread tid
FX_HD int bin_of(int tid, int q) {
    const int l = tid & 63, wave = tid >> 6;
    const int k1 = 2 * wave + ((l >> 4) & 1), q1 = l & 15, q2 = q + 8 * (l >> 5);
    return k1 + 16 * q1 + 256 * q2;
}

// inverse: where bin k lives in the [q*512 + tid] slot order the kernel stores partial sums in
FX_HD int slot_of_bin(int k) {
    const int k1 = k & 15, q1 = (k >> 4) & 15, q2 = k >> 8;
    const int l = (q2 >> 3) * 32 + (k1 & 1) * 16 + q1;
    const int tid = (k1 >> 1) * 64 + l;
    return (q2 & 7) * kThreads + tid;
}

// this lane's index L among the 256 (k1, q1) combinations of phase 3
FX_HD int lane_specpos(int tid) {
    const int l = tid & 63, wave = tid >> 6;
    return (2 * wave + ((l >> 4) & 1)) * 16 + (l & 15);
}

// position inside a spectrum row written by the F-only variant of the kernel (multi-antenna path) of the lane's bin
// q2: the lane's bins 2m and 2m + 1 sit side by side, so one 16-byte store takes both and the 32 lanes of a half-wave
// fill 512 consecutive bytes
FX_HD int specpos(int lane_l, int q2) { return (q2 >> 1) * 512 + 2 * lane_l + (q2 & 1); }
FX_HD int specpos_of_bin(int k) { return specpos((k & 15) * 16 + ((k >> 4) & 15), k >> 8); }

}  // namespace fused
}  // namespace fxc
