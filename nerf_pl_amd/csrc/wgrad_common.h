// Weight gradient (wgrad.hip): what its kernels share -- the task and launch
// structs, the workgroup prologue, the flat parameter offsets.  The task table
// and the split-K and fusion constants: wgrad_plan.h.
#pragma once
#include "wgrad_plan.h"
#include "x3.h"

namespace x3 {

// ---- 32x32x16 helpers of the split-operand kernels ---------------------------
__device__ __forceinline__ f32x16 mfma32(const p8& a, const p8& b, f32x16 c) {
#if NR_F16
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
#else
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
#endif
}

// acc += A * B, small products first; a = the A pieces (hi[, mid], lo)
__device__ __forceinline__ f32x16 mfma_xp(const p8 (&a)[kNP], const Pieces& b, f32x16 acc) {
#if NR_F16
    acc = mfma32(a[1], b.hi, acc);
    acc = mfma32(a[0], b.lo, acc);
    acc = mfma32(a[0], b.hi, acc);
#elif NR_BF1
    acc = mfma32(a[0], b.hi, acc);
#else
    acc = mfma32(a[2], b.hi, acc);
    acc = mfma32(a[0], b.lo, acc);
    acc = mfma32(a[1], b.mid, acc);
    acc = mfma32(a[1], b.hi, acc);
    acc = mfma32(a[0], b.mid, acc);
    acc = mfma32(a[0], b.hi, acc);
#endif
    return acc;
}

// acc[j] += A * B[j] for NJ accumulators sharing the A pieces, product-major
template <int NJ>
__device__ __forceinline__ void mfma_xp_multi(const p8 (&a)[kNP], const Pieces (&b)[NJ], f32x16* acc) {
#if NR_F16
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = mfma32(a[1], b[j].hi, acc[j]);
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = mfma32(a[0], b[j].lo, acc[j]);
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = mfma32(a[0], b[j].hi, acc[j]);
#elif NR_BF1
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = mfma32(a[0], b[j].hi, acc[j]);
#else
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = mfma32(a[2], b[j].hi, acc[j]);
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = mfma32(a[0], b[j].lo, acc[j]);
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = mfma32(a[1], b[j].mid, acc[j]);
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = mfma32(a[1], b[j].hi, acc[j]);
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = mfma32(a[0], b[j].mid, acc[j]);
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = mfma32(a[0], b[j].hi, acc[j]);
#endif
}

}  // namespace x3

namespace {

constexpr int kThreads = 512;    // 8 waves: two per SIMD, so one wave's staging and
                                 // barrier time overlaps its partner's MFMAs

// f16x3: the task pairs that read the same saved segment (wgrad_plan.h
// kFused: DZ(4), H(7), dz_dir) run fused -- one workgroup stages the shared
// segment once and computes both outputs.  Compile time: it sizes the kernels' LDS.
constexpr bool kFuse = NR_F16 || NR_BF1;

// flat parameter offsets, NeRF.named_parameters() order (packing.py param_offsets)
struct POff {
    int w[12], b[12], fan[12];
};
constexpr POff make_poff() {
    POff p{};
    const int rows[12] = {256, 256, 256, 256, 256, 256, 256, 256, 256, 128, 1, 3};
    const int fans[12] = {63, 256, 256, 256, 319, 256, 256, 256, 256, 283, 256, 128};
    int o = 0;
    for (int i = 0; i < 12; ++i) {
        p.w[i] = o;
        p.fan[i] = fans[i];
        o += rows[i] * fans[i];
        p.b[i] = o;
        o += rows[i];
    }
    return p;
}
constexpr POff kP = make_poff();
static_assert(kP.b[11] + 3 == 595844, "parameter count");
// layer ids: 0..7 = xyz_encoding_1..8, 8 = final, 9 = dir, 10 = sigma, 11 = rgb

__device__ __forceinline__ int pe_feature(int g, int h, int np) {
    if (g == 0) return h;
    if (g == 1) return h == 0 ? 2 : -1;
    if (g < 2 + np) { const int m = g - 2 + np * h; return 3 + 6 * (m / 3) + m % 3; }
    if (g < 2 + 2 * np) { const int m = g - 2 - np + np * h; return 6 + 6 * (m / 3) + m % 3; }
    return -1;
}

struct WgSeg {
    const float* base;   // segment start (block-native)
    int kind, width;     // SegKind, columns
};

struct WgTask {
    WgSeg a, b;          // a = gradient (M = a.width), b = input (N = b.width)
    int wm, wn;          // wave grid (wm * wn == 4)
    int G;               // workgroups
    int64_t slab;        // slab offset (floats) of workgroup 0
    int id;              // task id: selects the gradient destination and the kernel shape
    int stat;            // f16x3: stats slot of the gradient operand (layout.h NR_STATS)
    int fuse;            // f16x3: index (in WgArgs::task) of the task whose output this task's
                         // workgroups also compute (same block ranges, its own slab), or -1
    int pa, pb;          // slab row / column order (wgrad4_kernel): 1 natural; V: each
                         // 32V-wide chunk holds its V interleaved MFMA tiles one after
                         // another (w4_unperm)
};

struct WgArgs {
    WgTask task[kTasks];
    int wg_start[kTasks + 1];
    int nb, n;
    float* slab;
    bool x3;             // segments in the bf16x6 pipeline's N16 layout (x3.h)
    const float* stats;  // f16x3: max |gradient| per segment (mlp_bwd3.hip), else null
    // optional (active.hip, split arithmetics' wgrad3_body only): the ascending
    // list of the samples with a nonzero output gradient and its length m on
    // the device.  The gradient segments (mlp_bwd3.hip *_active) then hold
    // position q's rows at q; the split-K ranges cover the ceil(m / 32) blocks
    // of positions, and the input operands are gathered from sample slist[q]
    const int32_t* slist; const int32_t* scount;
};

// samples (positions) a launch works on
__device__ __forceinline__ int wg_m(const WgArgs& a) {
    return a.slist ? __builtin_amdgcn_readfirstlane(*a.scount) : a.n;
}
// blocks of positions a launch's split-K ranges cover
__device__ __forceinline__ int wg_nact(const WgArgs& a) {
    return a.slist ? (wg_m(a) + 31) / 32 : a.nb;
}

// workgroup c's slab of task T
__device__ __forceinline__ float* wg_slab(const WgArgs& a, const WgTask& T, int c) {
    return a.slab + T.slab + (int64_t)c * (T.a.width * T.b.width + T.a.width);
}
// the dispatch position whose workgroups include this one
__device__ __forceinline__ int wg_task(const WgArgs& a) {
    int t = 0;
#pragma unroll 1
    while (t + 1 < kTasks && (int)blockIdx.x >= a.wg_start[t + 1]) ++t;
    return t;
}
// What every kernel's workgroup starts from: its index c among its task's G
// workgroups, the task, its blocks [b0, b1) of the split-K partition, and its
// slab (a fused partner's: wg_slab of a.task[T.fuse] at the same c)
struct WgWork {
    int c;
    const WgTask& T;
    int b0, b1;
    float* slab;
    __device__ __forceinline__ explicit WgWork(const WgArgs& a) : WgWork(a, wg_task(a)) {}
    __device__ __forceinline__ WgWork(const WgArgs& a, int t)
        : c(blockIdx.x - a.wg_start[t]), T(a.task[t]) {
        const int nact = wg_nact(a);
        b0 = (int)((int64_t)c * nact / T.G);
        b1 = (int)((int64_t)(c + 1) * nact / T.G);
        slab = wg_slab(a, T, c);
    }
};

// f16x3: the gradient operand of a task is scaled by 2^(kWT - e(max |dz|)) so
// its largest element sits in [2^kWT, 2^(kWT+1)) < 65504; the input operand
// (activations, |x| < 65504) is split unscaled.  The reduction divides the
// weight part of the slab sums by the same power of two (bias sums come from
// the unscaled values).
__device__ __forceinline__ float task_scale(const WgArgs& a, const WgTask& T) {
#if NR_F16
    constexpr int kWT = 14;
    return x3::pow2_norm(a.stats[T.stat], kWT, 126);
#else
    (void)a; (void)T;
    return 1.f;
#endif
}

}  // namespace
