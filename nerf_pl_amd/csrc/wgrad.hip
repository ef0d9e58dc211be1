// MLP backward, weight gradients: dW = sum_s dz[s]^T x[s] and db = sum_s dz[s]
// for every layer of NeRF (autograd of the nn.Linear layers, nerf.py:60-81).
//
// Grouped split-K GEMM on v_mfma_f32_32x32x2_f32.  Each of the 14 tasks
// (a gradient segment dz x an input segment x, both in the block-native layout
// of layout.h) is a <=256x256 output reduced over all samples.  Every task's
// sample blocks are split over G_t workgroups (G_t proportional to its cost,
// ~2 resident rounds in total).  A workgroup streams its blocks one 32-sample
// block per stage into LDS, transposing the block-native chunks to
// [sample][column] with ds_write_b128 (row stride 260: conflict-free), double
// buffered; its 4 waves split the task's output with a per-task wave grid so
// every SIMD holds MFMA work; k-step kk of a stage pairs samples 2kk and 2kk+1.
// Each workgroup writes one partial slab; a second kernel sums a task's slabs
// in a fixed order (bitwise reproducible) and scatters the result into the flat
// gradient buffer in NeRF.named_parameters() order.
//
// This file is the one translation unit (built three times: bf16x6 + exact
// fp32, f16x3, bf16); the kernels live in headers, one per kernel.  Here: the
// destination maps, the reductions, the launch plan and the entry points.
#include <stdlib.h>

#include <type_traits>

#include "wgrad_common.h"   // task / launch structs, the workgroup prologue; wgrad_plan.h: the launch plan
#include "wgrad_f32.h"      // wgrad_kernel: exact fp32 (base object only)
#include "wgrad3.h"         // wgrad3_kernel: register-staged split operands; bf16: wgrad_b1.h
#include "wgrad4.h"         // wgrad4_kernel: f16x3 LDS-DMA (f16x3 object only)

namespace {

// slab index p (row or column) of a WgTask::pa / pb order -> the natural index
__device__ __forceinline__ int w4_unperm(int p, int v) {
    if (v <= 1) return p;
    const int w = 32 * v, r = p % w;
    return p - r + v * (r & 31) + (r >> 5);
}

// Embedding channel of bf16x6 PE slot q (packing._pe16_channel / _dir16_channel)
__device__ __forceinline__ int pe16_channel(int q) {
    if (q == 58 || q == 59) return q - 58;
    if (q == 62) return 2;
    const int c = q >> 3, j = q & 7, m = 4 * c + (j & 3);
    if (m >= 30) return -1;
    return (j < 4 ? 3 : 6) + 6 * (m / 3) + m % 3;
}
__device__ __forceinline__ int dir16_channel(int q) {
    const int g = q >> 3, j = q & 7;
    if (j == 3) return g < 3 ? g : -1;
    if (j == 7) return -1;
    return (j < 4 ? 3 : 6) + 6 * g + (j & 3);
}

// destination of output element (o, c) of task t in the flat gradient (-1 = none)
__device__ int wgrad_dest(int t, int o, int c, bool x3) {
    switch (t) {
        case 0: { const int f = x3 ? pe16_channel(c) : pe_feature(c & 31, c >> 5, 15);
                  return f < 0 ? -1 : kP.w[0] + o * kP.fan[0] + f; }
        case 1: case 2: case 3: return kP.w[t] + o * kP.fan[t] + c;
        case 4: { const int f = x3 ? pe16_channel(c) : pe_feature(c & 31, c >> 5, 15);
                  return f < 0 ? -1 : kP.w[4] + o * kP.fan[4] + f; }
        case 5: return kP.w[4] + o * kP.fan[4] + NR_XYZ_CH + c;
        case 6: case 7: case 8: case 9: return kP.w[t - 1] + o * kP.fan[t - 1] + c;
        case 10: return kP.w[9] + o * kP.fan[9] + c;
        case 11: { const int f = x3 ? dir16_channel(c) : pe_feature(c & 15, c >> 4, 6);
                   return f < 0 ? -1 : kP.w[9] + o * kP.fan[9] + 256 + f; }
        case 12: return o == 3 ? kP.w[10] + c : -1;
        case 13: return o < 3 ? kP.w[11] + o * kP.fan[11] + c : -1;
    }
    return -1;
}

__device__ int wgrad_bias_dest(int t, int o) {
    switch (t) {
        case 0: return kP.b[0] + o;
        case 1: case 2: case 3: return kP.b[t] + o;
        case 4: return kP.b[4] + o;
        case 6: case 7: case 8: case 9: return kP.b[t - 1] + o;
        case 10: return kP.b[9] + o;
        case 12: return o == 3 ? kP.b[10] : kP.b[11] + o;
    }
    return -1;
}

#if NR_F16
// stats[l] = max over the per-wave maxima [l][nb] written by mlp_bwd3.hip;
// 1024 threads per segment, four independent loads in flight per thread (the
// max is order-independent: the result does not depend on the schedule)
constexpr int kStatT = 1024;
__global__ void __launch_bounds__(kStatT) stats_reduce_kernel(float* __restrict__ stats, int nb) {
    const int l = blockIdx.x;
    const float* w = stats + NR_STATS + (int64_t)l * nb;
    float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f;
    int i = threadIdx.x;
    for (; i + 3 * kStatT < nb; i += 4 * kStatT) {
        m0 = fmaxf(m0, w[i]);
        m1 = fmaxf(m1, w[i + kStatT]);
        m2 = fmaxf(m2, w[i + 2 * kStatT]);
        m3 = fmaxf(m3, w[i + 3 * kStatT]);
    }
    for (; i < nb; i += kStatT) m0 = fmaxf(m0, w[i]);
    float m = fmaxf(fmaxf(m0, m1), fmaxf(m2, m3));
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
    __shared__ float red[kStatT / 64];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kStatT / 64; ++k) m = fmaxf(m, red[k]);
        stats[l] = m;
    }
}
#endif

__global__ void wgrad_reduce_kernel(WgArgs a, float* __restrict__ grad) {
    const int t = blockIdx.y;
    const WgTask& T = a.task[t];
    const int M = T.a.width, N = T.b.width;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int nw = M * N, sz = nw + M;
    if (e >= sz) return;
    const int dst = e < nw ? wgrad_dest(T.id, w4_unperm(e / N, T.pa), w4_unperm(e % N, T.pb), a.x3)
                           : wgrad_bias_dest(T.id, e - nw);
    if (dst < 0) return;
    // 8 independent partial sums (fixed order: bitwise reproducible) keep 8
    // slab loads in flight per thread instead of one dependent chain
    const float* p = a.slab + T.slab + e;
    float q[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int w = 0;
    for (; w + 8 <= T.G; w += 8, p += 8 * (int64_t)sz)
#pragma unroll
        for (int i = 0; i < 8; ++i) q[i] += p[(int64_t)i * sz];
    for (int i = 0; w < T.G; ++w, ++i, p += sz) q[i] += *p;
    float s = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
    if (e < nw) s /= task_scale(a, T);    // exact: a power of two
    grad[dst] = s;
}

// the slab workspace every launch gets: the largest plan of any arithmetic and path
constexpr int64_t kWorkspaceFloats = wgrad_plan_max_floats();

}  // namespace

#if NR_X3_BASE_OBJECT
// dir_encoding.0.weight's first 256 columns (the xyz_encoding_final input,
// nerf.py:118): the weight-gradient launch leaves G = sum_s dz_dir h8^T there
// (task 10); the gradient of the reference's dW = sum_s dz_dir feat^T with
// feat = W_final h8 + b_final is G W_final^T + db_dir b_final^T.  One
// workgroup per output row (in place: a row reads only itself), fp32 fma
// chains over k in order.
__global__ void __launch_bounds__(256) dir_feat_kernel(const float* __restrict__ params,
                                                       float* __restrict__ grad) {
    __shared__ float g[256];
    const int o = blockIdx.x, c = threadIdx.x;
    constexpr int kFan = 283;                       // dir_encoding.0 fan-in
    float* row = grad + kP.w[9] + o * kFan;
    g[c] = row[c];
    __syncthreads();
    const float* w = params + kP.w[8] + c * 256;    // xyz_encoding_final.weight row c
    float acc = 0.f;
#pragma unroll 8
    for (int k = 0; k < 256; ++k) acc = fmaf(g[k], w[k], acc);
    row[c] = fmaf(grad[kP.b[9] + o], params[kP.b[8] + c], acc);
}

// xyz_encoding_final (nerf.py:116): dW = W_dir[:, :256]^T G, db = W_dir[:, :256]^T db_dir
// (dfeat = W_dir[:, :256]^T dz_dir is not stored).  Runs before dir_feat_kernel
// rewrites G.  Workgroup c = output row, thread k = column; fp32 fma chains over
// the 128 dir outputs in order.
__global__ void __launch_bounds__(256) final_from_g_kernel(const float* __restrict__ params,
                                                          float* __restrict__ grad) {
    const int c = blockIdx.x, k = threadIdx.x;
    constexpr int kFan = 283;
    const float* G = grad + kP.w[9];                 // G[o][k] at o * 283 + k
    const float* W = params + kP.w[9];               // W_dir[o][c] at o * 283 + c
    float acc = 0.f, b = 0.f;
#pragma unroll 8
    for (int o = 0; o < 128; ++o) {
        const float w = W[o * kFan + c];
        acc = fmaf(w, G[o * kFan + k], acc);
        if (k == 0) b = fmaf(w, grad[kP.b[9] + o], b);
    }
    grad[kP.w[8] + c * 256 + k] = acc;
    if (k == 0) grad[kP.b[8] + c] = b;
}

NR_API int nr_wgrad_dir_feat(const float* params, float* grad_flat, void* stream) {
    NR_REQUIRE(params && grad_flat, "nr_wgrad_dir_feat: null pointer");
    final_from_g_kernel<<<256, 256, 0, (hipStream_t)stream>>>(params, grad_flat);
    NR_LAUNCH_CHECK("nr_wgrad_dir_feat");
    dir_feat_kernel<<<128, 256, 0, (hipStream_t)stream>>>(params, grad_flat);
    NR_LAUNCH_CHECK("nr_wgrad_dir_feat");
    return 0;
}

NR_API int64_t nr_wgrad_workspace_bytes(int64_t n) {
    (void)n;
    return kWorkspaceFloats * (int64_t)sizeof(float);
}
#endif

namespace {
// this object's split arithmetic
constexpr WgArith kArith = NR_F16 ? kArithF16x3 : NR_BF1 ? kArithBf16 : kArithBf16x6;
static_assert(kArith.split && kArith.nprod == x3::kNProd && kArith.fuse == kFuse &&
              kArith.w4 == (NR_F16 == 1) && kArith.lists == !NR_BF1, "wgrad_plan.h: this object's row");

// (ga, rows) -> the kernels' template arguments, in the order that keeps the
// kernels' places in the code object.  bf16 has one kernel: no sample lists,
// and its segments are bf16 chunks in either graph
template <class F>
void with_ga_rows(bool ga, bool rows, F f) {
    using Y = std::true_type;
    using N = std::false_type;
    if constexpr (!NR_BF1) {
        if (ga && rows) return f(Y{}, Y{});
        if (ga) return f(Y{}, N{});
        if (rows) return f(N{}, Y{});
    }
    f(N{}, N{});
}

// slist / scount: the launch covers positions 0 .. *scount of the buffers; with
// gather the input operands are gathered from sample slist[q] (the *_active
// entry points), else they were saved by position (the *_listed ones)
int wgrad_launch(bool x3, bool sigma_only, const float* save, const float* grad_ws, int64_t n,
                 float* workspace, float* grad_flat, void* stream,
                 const int32_t* slist = nullptr, const int32_t* scount = nullptr,
                 bool gather = true) {
    const char* name = sigma_only ? "nr_wgrad_sigma" : "nr_wgrad";
    NR_REQUIRE(n >= 0 && n < (int64_t)1 << 31, "%s: n out of range", name);
    NR_REQUIRE(save && grad_ws && workspace && grad_flat, "%s: null pointer", name);
    NR_REQUIRE((((uintptr_t)save | (uintptr_t)grad_ws) & 15) == 0,
               "nr_wgrad: save/grad_ws must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        hipError_t e = hipMemsetAsync(grad_flat, 0, 595844 * sizeof(float), st);
        if (e != hipSuccess) { nr_set_error("nr_wgrad: memset failed"); return (int)e; }
        return 0;
    }
    const int64_t nb = (n + 31) / 32;          // blocks holding samples (the work)
    const int64_t nbp = nr_blocks_pad(n);      // segment stride of the buffers
    const WgArith& A = x3 ? kArith : kArithF32;
    // f16x3, full graph: the LDS-DMA weight gradient (wgrad4_kernel).  32-bit
    // buffer offsets: every segment it reads stays under 2 GiB below 2M samples.
    // NR_WGRAD_W4=0 in the environment: the register-staged wgrad3_kernel, for
    // A/B runs and the cross-check test (read per launch)
    const char* w4_env = getenv("NR_WGRAD_W4");
    const bool use_w4 = A.w4 && !sigma_only && n < ((int64_t)1 << 21) &&
                        !(w4_env && atoi(w4_env) == 0);
    const WgPlan plan = wgrad_plan(A, sigma_only, slist != nullptr, use_w4, nb);
    NR_REQUIRE(plan.slab_floats <= kWorkspaceFloats,
               "%s: the launch plan's slabs exceed nr_wgrad_workspace_bytes", name);
    // the tasks' segments (gradient, input), by task id (wgrad_plan.h kWgShape).
    // Task 10 (dir_encoding's feat columns) reads h8, not xyz_encoding_final's
    // output: dW = sum dz_dir feat^T = G W_final^T + db_dir b_final^T with
    // G = sum dz_dir h8^T (nerf.py:116, feat = W_final h8 + b_final), so the
    // forward saves no feat.  And task 9 (xyz_encoding_final) launches nothing:
    // its dW = sum dfeat h8^T with dfeat = W_dir[:, :256]^T dz_dir is
    // W_dir[:, :256]^T G (db = W_dir[:, :256]^T db_dir), so the data gradient
    // stores no dfeat either.  nr_wgrad_dir_feat forms both from G
    // (DESIGN.md 13); task 9's entry keeps the id order (its slot: a dummy)
    const float* SV = save;
    const float* GD = grad_ws;
    auto H = [&](int l) { return SV + nr_sv_h(l, nbp); };
    auto DZ = [&](int l) { return GD + nr_gd_dz(l, nbp); };
    const float* pe = SV;
    const float* dpe = SV + nr_sv_dirpe(nbp);
    const float* hdir = SV + nr_sv_hdir(nbp);
    const float* dzdir = GD + nr_gd_dzdir(nbp);
    const float* head = GD + nr_gd_dhead(nbp);
    const float* const seg[kTasks][2] = {
        {DZ(0), pe}, {DZ(1), H(0)}, {DZ(2), H(1)}, {DZ(3), H(2)},
        {DZ(4), pe}, {DZ(4), H(3)}, {DZ(5), H(4)}, {DZ(6), H(5)},
        {DZ(7), H(6)}, {DZ(0), H(7)} /* 9: dummy, no workgroups */,
        {dzdir, H(7)}, {dzdir, dpe}, {head, H(7)}, {head, hdir},
    };
    WgArgs a{};
    for (int k = 0; k < kTasks; ++k) {
        const WgPlanTask& p = plan.task[k];
        const WgShape& s = kWgShape[p.id];
        a.task[k] = WgTask{{seg[p.id][0], s.ka, s.M}, {seg[p.id][1], s.kb, s.N}, s.wm, s.wn,
                           p.G, p.slab, p.id, s.stat, p.fuse, p.pa, p.pb};
    }
    for (int k = 0; k <= kTasks; ++k) a.wg_start[k] = plan.wg_start[k];
    a.nb = (int)nb;
    a.n = (int)n;
    a.slab = workspace;
    a.x3 = x3;
    a.stats = NR_F16 ? SV + nr_sv_stats(nbp) : nullptr;
    a.slist = slist;
    a.scount = scount;
    const int wgs = a.wg_start[kTasks];
    // GA: gathered inputs; ROWS: the full graph's inputs are sample-major rows
    // (mlp_fwd.hip ROWS), the sigma-only graph's block-native
    const bool ga = slist && gather, rows = !sigma_only;
#if NR_F16
    stats_reduce_kernel<<<NR_STAT_SEGS, kStatT, 0, st>>>(const_cast<float*>(SV) + nr_sv_stats(nbp), (int)nbp);
    NR_LAUNCH_CHECK("nr_wgrad_stats");
    if (use_w4 && ga) wgrad4_kernel<true><<<wgs, w4::kT, 0, st>>>(a);
    else if (use_w4) wgrad4_kernel<false><<<wgs, w4::kT, 0, st>>>(a);
    else
#endif
    if (x3) with_ga_rows(ga, rows, [&](auto GA, auto ROWS) {
        wgrad3_kernel<GA(), ROWS()><<<wgs, kThreads, 0, st>>>(a);
    });
#if NR_X3_BASE_OBJECT
    else with_ga_rows(ga, rows, [&](auto GA, auto ROWS) {
        wgrad_kernel<GA(), ROWS()><<<wgs, kThreads, 0, st>>>(a);
    });
#endif
    NR_LAUNCH_CHECK("nr_wgrad");
    dim3 rg((256 * 256 + 256 + 255) / 256, kTasks);
    wgrad_reduce_kernel<<<rg, 256, 0, st>>>(a, grad_flat);
    NR_LAUNCH_CHECK("nr_wgrad_reduce");
    return 0;
}
}  // namespace

// The entry points: NAME(BASE) is the exported symbol (NR_PLAIN: the exact-fp32
// arithmetic, base object only; NR_X3_NAME: this object's split arithmetic),
// BASE alone names the call in its error message.
//   nr_wgrad         every sample of the full graph
//   nr_wgrad_sigma   the sigma-only graph's weight gradients (after
//                    nr_mlp_bwd_sigma*): every layer up to xyz_encoding_8 and
//                    the sigma head; the other parameters get 0
//   *_active         over the samples nr_active_samples listed (after
//                    nr_mlp_bwd*_active with the same list); the other samples'
//                    output gradients are exactly zero, so the sums are those of
//                    nr_wgrad* up to the order of the split-K partial sums
//   *_listed         over the first *count positions of buffers written by
//                    position (nr_mlp_fwd_listed* + nr_mlp_bwd*_listed, the
//                    deferred save)
#define NR_PLAIN(base) base
#define NR_WGRAD_ENTRY(NAME, BASE, X3, SIGMA)                                                  \
    NR_API int NAME(BASE)(const float* save, const float* grad_ws, int64_t n, float* workspace, \
                          float* grad_flat, void* stream) {                                    \
        return wgrad_launch(X3, SIGMA, save, grad_ws, n, workspace, grad_flat, stream);        \
    }
#define NR_WGRAD_LIST_ENTRY(NAME, BASE, X3, SIGMA, GATHER)                                      \
    NR_API int NAME(BASE)(const float* save, const float* grad_ws, int64_t n, float* workspace, \
                          float* grad_flat, const int32_t* samples, const int32_t* count,      \
                          void* stream) {                                                      \
        NR_REQUIRE(samples && count, #BASE ": null sample list");                              \
        return wgrad_launch(X3, SIGMA, save, grad_ws, n, workspace, grad_flat, stream, samples, \
                            count, GATHER);                                                    \
    }

#if NR_X3_BASE_OBJECT
NR_WGRAD_ENTRY(NR_PLAIN, nr_wgrad, false, false)
NR_WGRAD_ENTRY(NR_PLAIN, nr_wgrad_sigma, false, true)
NR_WGRAD_LIST_ENTRY(NR_PLAIN, nr_wgrad_active, false, false, true)
NR_WGRAD_LIST_ENTRY(NR_PLAIN, nr_wgrad_sigma_active, false, true, true)
NR_WGRAD_LIST_ENTRY(NR_PLAIN, nr_wgrad_listed, false, false, false)
NR_WGRAD_LIST_ENTRY(NR_PLAIN, nr_wgrad_sigma_listed, false, true, false)
#endif

NR_WGRAD_ENTRY(NR_X3_NAME, nr_wgrad, true, false)
NR_WGRAD_ENTRY(NR_X3_NAME, nr_wgrad_sigma, true, true)
#if !NR_BF1
NR_WGRAD_LIST_ENTRY(NR_X3_NAME, nr_wgrad_active, true, false, true)
NR_WGRAD_LIST_ENTRY(NR_X3_NAME, nr_wgrad_sigma_active, true, true, true)
NR_WGRAD_LIST_ENTRY(NR_X3_NAME, nr_wgrad_listed, true, false, false)
NR_WGRAD_LIST_ENTRY(NR_X3_NAME, nr_wgrad_sigma_listed, true, true, false)
#endif

