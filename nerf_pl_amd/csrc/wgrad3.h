// Weight gradient (wgrad.hip): the register-staged split-operand kernel.
// ---------------------------------------------------------------------------
// bf16x6 variant: the same task list and slabs on v_mfma_f32_32x32x16_bf16.
// A stage is 16 samples (half a block): each thread loads the float4s of two
// adjacent samples of one 4-column chunk, splits them exactly into three bf16
// pieces (x3.h) and writes them as [piece][column][16 samples] images
// (column stride 48 B: conflict-free ds_read_b128 fragments), double
// buffered; the bias sums come from the fp32 values during staging.
// ---------------------------------------------------------------------------
#pragma once
#include "wgrad_common.h"
#include "wgrad_b1.h"

namespace {

namespace w3 {
// Cache policy of the saved-segment reads (each byte is read once): plain
// loads.  Non-temporal register loads in the f16x3 / bf16x6 staging measured
// slower, 3.02 -> 3.13 ms (profiles/r02/nt_ab.txt).
template <class T>
__device__ __forceinline__ T ld_seg(const T* p) {
    return *p;
}
constexpr int kColB = 48;                        // bytes per column (16 pieces + pad)
constexpr int kPlane = 256 * kColB;              // one piece of one operand
constexpr int kOpnd = x3::kNP * kPlane;          // one operand (all pieces)
constexpr int kXPlane = 64 * kColB;              // one piece of a fused task's extra operand
constexpr int kXOpnd = kFuse ? x3::kNP * kXPlane : 0;
constexpr int kBufB = 2 * kOpnd + kXOpnd;        // one stage buffer (A + B [+ X])
constexpr int kLds = 2 * kBufB;                  // double buffered: 147,456 B (bf16x6), 110,592 B (f16x3)

// The bf16x6 pipeline saves every segment in x3.h's N16 layout: float4 (F,
// S, lane 16g + j) = columns 16F + 4g .. +3 of sample 16S + j (PE segments:
// columns = PE slots, packing.PE16_MAP / DIR16_MAP).  A staging chunk k is
// columns 8k .. 8k+7; half h of it is float4 group g = 2(k & 1) + h of tile
// F = k >> 1.
template <int KIND, int W>
struct Geo3 {
    static constexpr int CHUNKS = KIND == SEG_ACC ? W / 8 : (KIND == SEG_PE ? 8 : (KIND == SEG_DPE ? 4 : 0));
    __device__ static __forceinline__ int col(int k, int h) { return 8 * k + 4 * h; }
    // float4 index inside a block of sample j of half-block hb
    __device__ static __forceinline__ int f4(int k, int h, int hb, int j) {
        return ((k >> 1) * 2 + hb) * 64 + 16 * (2 * (k & 1) + h) + j;
    }
};

// one operand's half-block: loads (2 float4 per thread) and the split/store.
// ROWS: an input segment saved sample-major (x3.h store_row: row width
// RW = the segment's columns); else N16 slots (gradient segments)
template <int KIND, int W, bool ROWS = false>
struct Stager {
    static constexpr int RW = Geo3<KIND, W>::CHUNKS * 8;
    bool act;      // this thread owns a pair (loads run for every thread, clamped)
    int k, h, jp;  // chunk, lane half, sample pair
    f32x4 v0, v1;
    static constexpr bool ALL = KIND != SEG_HEAD && Geo3<KIND, W>::CHUNKS * 16 >= kThreads;
    __device__ __forceinline__ void init(int tid) {
        if constexpr (KIND == SEG_HEAD) {
            act = tid < 8; k = 0; h = 0; jp = tid & 7;
        } else {
            k = tid >> 4; h = (tid >> 3) & 1; jp = tid & 7;
            act = ALL || k < Geo3<KIND, W>::CHUNKS;
            k = act ? k : 0;
        }
    }
    // samples 16 hb + 2 jp and +1 of block blk (unconditional: keeps the
    // compiler's vmcnt bookkeeping exact across the prefetch)
    __device__ __forceinline__ void load(const float* base, int blk, int hb) {
        if constexpr (KIND == SEG_HEAD) {
            const f32x4* p = reinterpret_cast<const f32x4*>(base) + (size_t)blk * 32 + 16 * hb + 2 * jp;
            v0 = ld_seg(p); v1 = ld_seg(p + 1);
        } else {
            constexpr int F4 = Geo3<KIND, W>::CHUNKS * 64;
#if NR_BF1      // bf16 segments (x3.h store_slot): 8-B slots, sample-major chunks, NR_SEGF block stride
            const x3::u32x2* p = reinterpret_cast<const x3::u32x2*>(base) + (size_t)blk * F4 +
                                 x3::bf16_slot(Geo3<KIND, W>::f4(k, h, hb, 2 * jp));
            v0 = x3::unpack_bf16x4(p[0]); v1 = x3::unpack_bf16x4(p[4]);
#else
            if constexpr (ROWS) {
                const float* r = base + ((size_t)blk * 32 + 16 * hb + 2 * jp) * RW + Geo3<KIND, W>::col(k, h);
                v0 = ld_seg(reinterpret_cast<const f32x4*>(r));
                v1 = ld_seg(reinterpret_cast<const f32x4*>(r + RW));
            } else {
                const f32x4* p = reinterpret_cast<const f32x4*>(base) + (size_t)blk * F4 +
                                 Geo3<KIND, W>::f4(k, h, hb, 2 * jp);
                v0 = ld_seg(p); v1 = ld_seg(p + 1);
            }
#endif
        }
    }
    // the same two samples gathered: sample s of the list (s0, s1) sits at
    // block s / 32, half-block (s / 16) & 1, lane column s & 15
    __device__ __forceinline__ void load_g(const float* base, int s0, int s1) {
        static_assert(KIND != SEG_HEAD, "head segments are gradients (packed by position)");
#if NR_BF1
        (void)base; (void)s0; (void)s1;
#else
        if constexpr (ROWS) {
            v0 = ld_seg(reinterpret_cast<const f32x4*>(base + (size_t)s0 * RW + Geo3<KIND, W>::col(k, h)));
            v1 = ld_seg(reinterpret_cast<const f32x4*>(base + (size_t)s1 * RW + Geo3<KIND, W>::col(k, h)));
        } else {    // N16: block s / 32, half-block (s / 16) & 1, lane column s & 15
            constexpr int F4 = Geo3<KIND, W>::CHUNKS * 64;
            const f32x4* b = reinterpret_cast<const f32x4*>(base);
            v0 = ld_seg(b + (size_t)(s0 >> 5) * F4 + Geo3<KIND, W>::f4(k, h, (s0 >> 4) & 1, s0 & 15));
            v1 = ld_seg(b + (size_t)(s1 >> 5) * F4 + Geo3<KIND, W>::f4(k, h, (s1 >> 4) & 1, s1 & 15));
        }
#endif
    }
    // split + store column e of this thread's chunk into an operand image
    // (values times sc, a power of two); samples >= nval become 0; adds the two
    // samples' unscaled sum (bias) to s
    __device__ __forceinline__ void store_e(char* img, int nval, int e, float& s, float sc,
                                            int plane = kPlane) {
        if (!ALL && !act) return;
        const int j = 2 * jp;
        const float x0 = j < nval ? v0[e] : 0.f, x1 = j + 1 < nval ? v1[e] : 0.f;
        const int c0 = KIND == SEG_HEAD ? 0 : Geo3<KIND, W>::col(k, h);
        s += x0 + x1;
        x3::p2 pc[x3::kNP];
        x3::split_p2(x0 * sc, x1 * sc, pc);
        char* q = img + (c0 + e) * kColB + 4 * jp;
#pragma unroll
        for (int i = 0; i < x3::kNP; ++i) *reinterpret_cast<x3::p2*>(q + i * plane) = pc[i];
    }
};

// A fused task's extra operand, staged thin: thread q < W * 8 loads one float2
// (columns 2cp, 2cp + 1 of sample j of the half-block, q = 16 cp + j) -- 2
// registers per set instead of Stager's 8 -- and writes single pieces.
// ROWS: an input segment (sample-major rows of W), else the head gradient.
template <int KIND, int W, bool ROWS = false>
struct ThinStager {
    static constexpr int Q = W * 8;            // float2 per half-block
    bool act;
    int j, c;                                  // sample, first column
    x3::f32x2 v;
    __device__ __forceinline__ void init(int tid) {
        act = tid < Q;
        const int q = act ? tid : 0;
        j = q & 15; c = 2 * (q >> 4);
    }
    __device__ __forceinline__ void load(const float* base, int blk, int hb) {
        size_t f;   // float offset of the pair
        if constexpr (KIND == SEG_HEAD) f = 4 * ((size_t)blk * 32 + 16 * hb + j) + c;
        else if constexpr (ROWS) f = ((size_t)blk * 32 + 16 * hb + j) * W + c;
        else f = 4 * ((size_t)blk * (W / 8) * 64 + ((c >> 4) * 2 + hb) * 64 + 16 * ((c & 15) >> 2) + j) + (c & 3);
#if NR_BF1
        static_assert(KIND == SEG_HEAD, "bf16 runs no fused task pairs (kFuse)");
#endif
        v = ld_seg(reinterpret_cast<const x3::f32x2*>(base + f));
    }
    // the same pair of sample s (gathered, see Stager::load_g)
    __device__ __forceinline__ void load_g(const float* base, int s) {
        static_assert(KIND != SEG_HEAD, "head segments are gradients (packed by position)");
        const size_t f = ROWS ? (size_t)s * W + c
                              : 4 * ((size_t)(s >> 5) * (W / 8) * 64 + ((c >> 4) * 2 + ((s >> 4) & 1)) * 64 +
                                     16 * ((c & 15) >> 2) + (s & 15)) + (c & 3);
        v = ld_seg(reinterpret_cast<const x3::f32x2*>(base + f));
    }
    // split + store this thread's pair (times sc); s0/s1 += the unscaled values
    __device__ __forceinline__ void store(char* img, int nval, float& s0, float& s1, float sc) {
        if (!act) return;
        const float x0 = j < nval ? v[0] : 0.f, x1 = j < nval ? v[1] : 0.f;
        s0 += x0; s1 += x1;
        x3::p2 pc[x3::kNP];
        x3::split_p2(x0 * sc, x1 * sc, pc);
        char* q = img + c * kColB + 2 * j;
#pragma unroll
        for (int i = 0; i < x3::kNP; ++i) {
            *reinterpret_cast<x3::p1*>(q + i * kXPlane) = pc[i][0];
            *reinterpret_cast<x3::p1*>(q + kColB + i * kXPlane) = pc[i][1];
        }
    }
};

// the pieces of one 32-column fragment at q (plane stride `plane`)
__device__ __forceinline__ x3::Pieces frag(const char* q, int plane) {
    x3::Pieces f;
    f.hi = *reinterpret_cast<const x3::p8*>(q);
#if NR_F16
    f.lo = *reinterpret_cast<const x3::p8*>(q + plane);
#elif NR_BF1
    (void)plane;
#else
    f.mid = *reinterpret_cast<const x3::p8*>(q + plane);
    f.lo = *reinterpret_cast<const x3::p8*>(q + 2 * plane);
#endif
    return f;
}
}  // namespace w3

// One task's workgroup.  Optional fused extra operand X (kFuse, f16x3): XS = 0
// X is a second input segment sharing the gradient operand A (extra output
// M x XW), XS = 1 a second gradient segment sharing the input operand B (the
// 4-row head: extra output XW x N); its XWM x XWN wave grid covers the extra
// output (grids smaller than 8 waves are computed twice, written once) and the
// result goes to the partner task's slab `xslab`.
template <bool GA, bool ROWS, int KA, int WA, int KB, int WB, int WM, int WN, int XK = -1,
          int XW = 0, int XS = 0, int XWM = 1, int XWN = 1>
__device__ __forceinline__ void wgrad3_body(const WgArgs& a, const WgTask& T, int b0, int b1,
                                            char* lds, float* __restrict__ slab,
                                            float* __restrict__ xslab = nullptr) {
    using namespace w3;
    constexpr int MT = (WA / WM + 31) / 32, NT = (WB / WN + 31) / 32;
    constexpr int M = WA, N = WB;
    constexpr bool HX = XK >= 0;
    constexpr int XKK = HX ? XK : SEG_HEAD, XWW = HX ? XW : 4;
    constexpr int XM = XS ? XW : M, XN = XS ? N : XW;              // extra output
    constexpr int XMT = XS ? 1 : (M / XWM + 31) / 32;
    constexpr int XNT = XS ? (N / XWN + 31) / 32 : (XWW / XWN + 31) / 32;
    static_assert(!HX || (kFuse && XWM * XWN <= 8 && 8 % (XWM * XWN) == 0), "extra operand grid");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool active = wave < WM * WN;
    const int mi = wave / WN, ni = wave % WN;
    const int m0 = 32 * MT * mi, n0 = 32 * NT * ni;
    const int xw = wave % (XWM * XWN);
    const int xm0 = 32 * XMT * (xw / XWN), xn0 = 32 * XNT * (xw % XWN);
    const int h = lane >> 5, col = lane & 31;

    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = f32x16{};
    f32x16 xacc[HX ? XMT : 1][HX ? XNT : 1];
    if constexpr (HX) {
#pragma unroll
        for (int i = 0; i < XMT; ++i)
#pragma unroll
            for (int j = 0; j < XNT; ++j) xacc[i][j] = f32x16{};
    }
    float bacc[4] = {0.f, 0.f, 0.f, 0.f};
    float xbacc[2] = {0.f, 0.f};

    // two register sets per operand: the loads run two stages ahead
    Stager<KA, WA> sa[2];          // gradient operand (N16 slots, by position)
    Stager<KB, WB, ROWS> sb[2];    // input operand (sample-major rows, or N16)
    ThinStager<XKK, XWW, ROWS && HX && XS == 0> sx[2];
    sa[0].init(tid); sa[1].init(tid);
    sb[0].init(tid); sb[1].init(tid);
    if constexpr (HX) { sx[0].init(tid); sx[1].init(tid); }
    if constexpr (KA == SEG_HEAD) {     // rows 4..31 of the 4-row gradient image stay 0
        for (int i = tid; i < 2 * x3::kNP * 32 * kColB / 4; i += kThreads) {
            const int b = i / (x3::kNP * 32 * kColB / 4), r = i % (x3::kNP * 32 * kColB / 4);
            const int p = r / (32 * kColB / 4), o = r % (32 * kColB / 4);
            reinterpret_cast<uint32_t*>(lds + b * kBufB + p * kPlane)[o] = 0u;
        }
    }
    if constexpr (HX && XS == 1) {      // same for a head extra operand (whole X image)
        for (int i = tid; i < 2 * kXOpnd / 4; i += kThreads) {
            constexpr int kW = kXOpnd > 0 ? kXOpnd / 4 : 1;
            const int b = i / kW, o = i % kW;
            reinterpret_cast<uint32_t*>(lds + b * kBufB + 2 * kOpnd)[o] = 0u;
        }
    }
    if constexpr (KA == SEG_HEAD || (HX && XS == 1)) __syncthreads();
    const int nst = 2 * (b1 - b0);      // half-block stages
    // stages past the end load a valid block and store zeros into a buffer
    // nobody reads again
    const int blast = b1 > b0 ? b1 - 1 : b0;
    const float* xbase = HX ? (XS ? a.task[T.fuse].a.base : a.task[T.fuse].b.base) : nullptr;
    // [b0, b1) are blocks of positions.  With a sample list (a.slist) the
    // gradient operands are packed by position and the input operands are
    // gathered: position q holds sample slist[q] (positions past m load
    // sample 0 and stage zeros).  Each register set holds the list entries of
    // the stage it loads next, fetched when its previous stage was loaded
    const int m = wg_m(a);
    constexpr bool gat = GA;
    auto sample_at = [&](int st, int j) {   // positions past m: sample 0 (staged as zeros)
        const int q = min(b0 + (st >> 1), blast) * 32 + 16 * (st & 1) + j;
        return q < m ? a.slist[q] : 0;
    };
    constexpr bool XIN = HX && XS == 0;    // the extra operand is an input segment
    int ns[2][2] = {{0, 0}, {0, 0}}, nx[2] = {0, 0};
    // B operand (input segment): this thread's samples 2 jp, 2 jp + 1; the
    // extra input operand: sample j of its ThinStager
    auto fetch = [&](int set, int st) {
        if constexpr (!gat) return;
        ns[set][0] = sample_at(st, 2 * sb[set].jp);
        ns[set][1] = sample_at(st, 2 * sb[set].jp + 1);
        if constexpr (XIN) nx[set] = sample_at(st, sx[set].j);
    };
    fetch(0, 0);
    fetch(1, 1);
    auto load = [&](int set, int st) {
        const int blk = min(b0 + (st >> 1), blast), hb = st & 1;
        sa[set].load(T.a.base, blk, hb);
        if constexpr (gat) {
            sb[set].load_g(T.b.base, ns[set][0], ns[set][1]);
            if constexpr (XIN) sx[set].load_g(xbase, nx[set]);
            else if constexpr (HX) sx[set].load(xbase, blk, hb);
            fetch(set, st + 2);
        } else {
            sb[set].load(T.b.base, blk, hb);
            if constexpr (HX) sx[set].load(xbase, blk, hb);
        }
    };
    const float sca = task_scale(a, T);
    const float scx = HX && XS ? task_scale(a, a.task[T.fuse]) : 1.f;
    auto store = [&](int set, int buf, int st) {
        const int nval = st < nst ? m - (b0 + (st >> 1)) * 32 - 16 * (st & 1) : 0;
        float sdummy = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            sa[set].store_e(lds + buf * kBufB, nval, e, bacc[e], sca);
            sb[set].store_e(lds + buf * kBufB + kOpnd, nval, e, sdummy, 1.f);
        }
        if constexpr (HX) sx[set].store(lds + buf * kBufB + 2 * kOpnd, nval, xbacc[0], xbacc[1], scx);
    };
    // LDS-only barrier: keeps the prefetched global loads in flight
    auto barrier = [] {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };
    // compute stage (buffer buf) from LDS while staging the next stage from
    // register set `set` into buffer buf ^ 1: the 8 store units (2 operands x
    // 4 columns) are spread between the row tiles' MFMAs so their VALU and
    // LDS-store work overlaps the MFMAs in flight instead of idling both waves
    // of a SIMD at the same time; the extra operand's 4 units follow its MFMAs;
    // after(), the reload of the freed register set, comes last
    auto compute_store = [&](int buf, int set, int st_next, auto after) {
        const int nval = st_next < nst ? m - (b0 + (st_next >> 1)) * 32 - 16 * (st_next & 1) : 0;
        char* ia = lds + (buf ^ 1) * kBufB;
        char* ib = ia + kOpnd;
        char* ix = ia + 2 * kOpnd;
        float sdummy = 0.f;
        auto unit = [&](int u) {
            if (u < 4) sa[set].store_e(ia, nval, u, bacc[u], sca);
            else sb[set].store_e(ib, nval, u - 4, sdummy, 1.f);
        };
        const char* cur = lds + buf * kBufB;
        const char* la = cur + (m0 + col) * kColB + 16 * h;
        const char* lb = cur + kOpnd + (n0 + col) * kColB + 16 * h;
        const bool go = WM * WN == 8 || active;
        x3::Pieces bp[NT];
        if (go) {
#pragma unroll
            for (int j = 0; j < NT; ++j) bp[j] = frag(lb + 32 * j * kColB, kPlane);
        }
        constexpr int UPT = (8 + MT - 1) / MT;   // store units per row tile
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            if (go) {
                x3::p8 ap[x3::kNP];
#pragma unroll
                for (int k = 0; k < x3::kNP; ++k)
                    ap[k] = *reinterpret_cast<const x3::p8*>(la + 32 * i * kColB + k * kPlane);
                x3::mfma_xp_multi<NT>(ap, bp, acc[i]);
            }
#pragma unroll
            for (int v = 0; v < UPT; ++v)
                if (i * UPT + v < 8) unit(i * UPT + v);
        }
        if constexpr (HX) {
            // extra output: A rows from the A image (XS = 0) or the X image,
            // B columns from the X image (XS = 0) or the B image
            const char* xa = (XS ? cur + 2 * kOpnd : cur) + (xm0 + col) * kColB + 16 * h;
            const char* xb = (XS ? cur + kOpnd : cur + 2 * kOpnd) + (xn0 + col) * kColB + 16 * h;
            constexpr int PA = XS ? kXPlane : kPlane, PB = XS ? kPlane : kXPlane;
            x3::Pieces xp[XNT];
#pragma unroll
            for (int j = 0; j < XNT; ++j) xp[j] = frag(xb + 32 * j * kColB, PB);
#pragma unroll
            for (int i = 0; i < XMT; ++i) {
                x3::p8 ap[x3::kNP];
#pragma unroll
                for (int k = 0; k < x3::kNP; ++k)
                    ap[k] = *reinterpret_cast<const x3::p8*>(xa + 32 * i * kColB + k * PA);
                x3::mfma_xp_multi<XNT>(ap, xp, xacc[i]);
            }
            sx[set].store(ix, nval, xbacc[0], xbacc[1], scx);
        }
        // interleave: per row tile, its fragment reads, then each MFMA followed
        // by one VALU op of the store units, then the units' LDS stores
        if constexpr (WM * WN == 8) {
            __builtin_amdgcn_sched_group_barrier(0x100, x3::kNP * NT, 0);
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x100, x3::kNP, 0);
#pragma unroll
                for (int r = 0; r < x3::kNProd * NT; ++r) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002, 1, 0);
                }
                __builtin_amdgcn_sched_group_barrier(0x200, x3::kNP * UPT, 0);
            }
            if constexpr (HX) {
                __builtin_amdgcn_sched_group_barrier(0x100, x3::kNP * (XNT + XMT), 0);
#pragma unroll
                for (int r = 0; r < x3::kNProd * XNT * XMT; ++r) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002, 1, 0);
                }
                __builtin_amdgcn_sched_group_barrier(0x200, x3::kNP * 2, 0);
            }
        }
        after();
    };
    // stage st lives in LDS buffer st & 1 and register set st & 1; a set is
    // reloaded (two stages ahead) as soon as its stage has been stored
    load(0, 0);
    load(1, 1);
    store(0, 0, 0);
    load(0, 2);
    barrier();
#pragma unroll 1
    for (int st = 0; st < nst; st += 2) {
        // stage st from buffer 0; set 1 (stage st+1) -> buffer 1, then set 1 reloaded
        compute_store(0, 1, st + 1, [&] { load(1, st + 3); });
        barrier();
        // stage st+1 from buffer 1; set 0 (stage st+2) -> buffer 0, then set 0 reloaded
        compute_store(1, 0, st + 2, [&] { load(0, st + 4); });
        barrier();
    }
    // bias sums: reduce the 8 sample pairs of each (chunk, half) group of the
    // gradient operand; lane jp == 0 writes
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        bacc[e] += __shfl_xor(bacc[e], 1);
        bacc[e] += __shfl_xor(bacc[e], 2);
        bacc[e] += __shfl_xor(bacc[e], 4);
    }
    if constexpr (HX && XS == 1) {      // over the 16 samples of each column pair
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int d = 1; d < 16; d <<= 1) xbacc[e] += __shfl_xor(xbacc[e], d);
    }
    if (sa[0].act && sa[0].jp == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int o = KA == SEG_HEAD ? e : Geo3<KA, WA>::col(sa[0].k, sa[0].h) + e;
            if (o < M) {
                slab[M * N + o] = bacc[e];
                if constexpr (HX && XS == 0) xslab[XM * XN + o] = bacc[e];   // shared gradient operand
            }
        }
    }
    if constexpr (HX && XS == 1) {      // the head extra operand is a gradient: its bias sums
        if (sx[0].act && sx[0].j == 0) {
#pragma unroll
            for (int e = 0; e < 2; ++e)
                if (sx[0].c + e < XM) xslab[XM * XN + sx[0].c + e] = xbacc[e];
        }
    }
    if constexpr (HX) {
        if (wave < XWM * XWN) {
#pragma unroll
            for (int i = 0; i < XMT; ++i)
#pragma unroll
                for (int j = 0; j < XNT; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int o = xm0 + 32 * i + nr_acc_row(r, h);
                        const int c = xn0 + 32 * j + col;
                        if (o < XM && c < XN) xslab[o * XN + c] = xacc[i][j][r];
                    }
        }
    }
    if (!active) return;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = m0 + 32 * i + nr_acc_row(r, h);
                const int c = n0 + 32 * j + col;
                if (o < M && c < N) slab[o * N + c] = acc[i][j][r];
            }
}

// GA: the packed sample list a.slist (the *_active entry points); ROWS: the
// input segments are sample-major rows (the full graph's forward), else N16
// (the sigma-only training forward, mlp_fwd3.hip kRows)
template <bool GA, bool ROWS>
__global__ void __launch_bounds__(kThreads, 1) wgrad3_kernel(WgArgs a) {
#if NR_BF1
    __shared__ __attribute__((aligned(16))) char lds[b1::kLds > w3::kLds ? b1::kLds : w3::kLds];
#else
    __shared__ __attribute__((aligned(16))) char lds[w3::kLds];
#endif
    const auto [c, T, b0, b1, slab] = WgWork(a);
    const int fu = __builtin_amdgcn_readfirstlane(T.fuse);
    if constexpr (kFuse) if (fu >= 0) {
        // the partner's slab (wg_slab spelt out: called here, the compiler computes
        // it ahead of the task switch and this kernel's schedule moves)
        const WgTask& P = a.task[fu];
        float* xslab = a.slab + P.slab + (int64_t)c * (P.a.width * P.b.width + P.a.width);
#if NR_BF1
        switch (__builtin_amdgcn_readfirstlane(T.id)) {
            case 5:    // DZ(4) x [H(3) | PE]: xyz_encoding_5 (skip layer)
                if constexpr (kFuseMask & 1)
                    wgrad_b1_body<256, 256, 2, 4, false, 1, 64>(a, T, b0, b1, lds, slab, xslab);
                break;
            case 10:  // [dz_dir | head] x H(7): dir_encoding's feat columns (as G) and sigma
                wgrad_b1_body<128, 256, 2, 4, false, 2, 4>(a, T, b0, b1, lds, slab, xslab); break;
        }
#else
        switch (__builtin_amdgcn_readfirstlane(T.id)) {
            case 5:    // DZ(4) x [H(3) | PE]: xyz_encoding_5 (skip layer); the fused
                       // PE output (256 x 64) on a 4 x 2 wave grid
                if constexpr ((kFuseMask & 1) && (!GA || (kFuseMaskGather & 1)))
                    wgrad3_body<GA, ROWS, SEG_ACC, 256, SEG_ACC, 256, 2, 4, SEG_PE, 64, 0, 4, 2>(
                        a, T, b0, b1, lds, slab, xslab);
                break;
            case 10:   // [dz_dir | head] x H(7): dir_encoding's feat columns (as G) and sigma
                if constexpr (kFuseMask & 2)
                    wgrad3_body<GA, ROWS, SEG_ACC, 128, SEG_ACC, 256, 2, 4, SEG_HEAD, 4, 1, 1, 8>(
                        a, T, b0, b1, lds, slab, xslab);
                break;
        }
#endif
        return;
    }
#if NR_BF1
    switch (__builtin_amdgcn_readfirstlane(T.id)) {
        case 0: case 4:
            wgrad_b1_body<256, 64, 8, 1>(a, T, b0, b1, lds, slab); return;
        case 10:
            wgrad_b1_body<128, 256, 2, 4>(a, T, b0, b1, lds, slab); return;
        case 11:
            wgrad_b1_body<128, 32, 4, 1>(a, T, b0, b1, lds, slab); return;
        case 12:
            wgrad_b1_body<4, 256, 1, 8, true>(a, T, b0, b1, lds, slab); return;
        case 13:
            wgrad_b1_body<4, 128, 1, 4, true>(a, T, b0, b1, lds, slab); return;
        default:
            wgrad_b1_body<256, 256, 2, 4>(a, T, b0, b1, lds, slab); return;
    }
#endif
    switch (__builtin_amdgcn_readfirstlane(T.id)) {
        case 0: case 4:
            wgrad3_body<GA, ROWS, SEG_ACC, 256, SEG_PE, 64, 8, 1>(a, T, b0, b1, lds, slab); break;
        case 10:
            wgrad3_body<GA, ROWS, SEG_ACC, 128, SEG_ACC, 256, 2, 4>(a, T, b0, b1, lds, slab); break;
        case 11:
            wgrad3_body<GA, ROWS, SEG_ACC, 128, SEG_DPE, 32, 4, 1>(a, T, b0, b1, lds, slab); break;
        case 12:
            wgrad3_body<GA, ROWS, SEG_HEAD, 4, SEG_ACC, 256, 1, 8>(a, T, b0, b1, lds, slab); break;
        case 13:
            wgrad3_body<GA, ROWS, SEG_HEAD, 4, SEG_ACC, 128, 1, 4>(a, T, b0, b1, lds, slab); break;
        default:
            wgrad3_body<GA, ROWS, SEG_ACC, 256, SEG_ACC, 256, 2, 4>(a, T, b0, b1, lds, slab); break;
    }
}

}  // namespace
