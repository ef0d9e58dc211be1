// Weight gradient (wgrad.hip): the split-K launch plan as plain C++ -- the task
// table, the four arithmetics, and one pure function from (arithmetic, graph,
// path, nb) to the dispatch order, the workgroup counts G_t, the fused pairs,
// the slab offsets and wg_start.  No HIP: tests/wgrad_plan_check.cpp compiles
// this header with a host compiler alone.
#pragma once
#include <stdint.h>

namespace {

constexpr int kTasks = 14;
constexpr int kTargetWG = 760;   // ~3 rounds of one workgroup per CU (short tail)
// the gathering kernels (a sample list, gathered inputs): 1024 measured 1.5%
// faster than 760 at cfg2's fine pass (three alternating rounds, profiles/r04/abalt_tw)
constexpr int kTargetWGGather = 1024;
// the LDS-DMA kernel (wgrad4_kernel, one workgroup per CU) over a sample list:
// 1536 measured 3% faster than 1024 (768: +0.5%, 2048: -1.5%) at cfg2's fine
// pass (two alternating rounds, profiles/r05/ab/u_*)
constexpr int kTargetWGW4 = 1536;

enum SegKind { SEG_ACC = 0, SEG_PE = 1, SEG_DPE = 2, SEG_HEAD = 3 };

// One task: dW = sum_s a[s]^T b[s], a = a gradient segment (M columns), b = an
// input segment (N columns); the id (the row's index) fixes wgrad_dest /
// wgrad_bias_dest.  DZ(l) = layer l's dz, H(l) = its output, in wgrad_launch's
// names.
struct WgShape {
    int M, N;        // gradient width, input width
    int ka, kb;      // their SegKind
    int wm, wn;      // wave grid (wm * wn <= 8)
    int stat;        // gradient operand's stats slot (layout.h NR_STATS)
    // wgrad4_kernel's slab orders: gradient rows 4-interleaved (not the head's),
    // input columns VB-interleaved (its dispatch in wgrad4.h)
    int pa, pb;
    constexpr bool head() const { return ka == SEG_HEAD; }   // the 4-row head gradient
};
constexpr WgShape kWgShape[kTasks] = {
    {256, 64, SEG_ACC, SEG_PE, 8, 1, 0, 4, 1},      //  0: DZ(0) x PE
    {256, 256, SEG_ACC, SEG_ACC, 2, 4, 1, 4, 4},    //  1: DZ(1) x H(0)
    {256, 256, SEG_ACC, SEG_ACC, 2, 4, 2, 4, 4},    //  2: DZ(2) x H(1)
    {256, 256, SEG_ACC, SEG_ACC, 2, 4, 3, 4, 4},    //  3: DZ(3) x H(2)
    {256, 64, SEG_ACC, SEG_PE, 8, 1, 4, 4, 1},      //  4: DZ(4) x PE (skip layer)
    {256, 256, SEG_ACC, SEG_ACC, 2, 4, 4, 4, 4},    //  5: DZ(4) x H(3)
    {256, 256, SEG_ACC, SEG_ACC, 2, 4, 5, 4, 4},    //  6: DZ(5) x H(4)
    {256, 256, SEG_ACC, SEG_ACC, 2, 4, 6, 4, 4},    //  7: DZ(6) x H(5)
    {256, 256, SEG_ACC, SEG_ACC, 2, 4, 7, 4, 4},    //  8: DZ(7) x H(6)
    {256, 256, SEG_ACC, SEG_ACC, 2, 4, 8, 4, 4},    //  9: xyz_encoding_final: no workgroups
    {128, 256, SEG_ACC, SEG_ACC, 2, 4, 9, 4, 2},    // 10: dz_dir x H(7)
    {128, 32, SEG_ACC, SEG_DPE, 4, 1, 9, 4, 1},     // 11: dz_dir x dir PE
    {4, 256, SEG_HEAD, SEG_ACC, 1, 8, 10, 1, 2},    // 12: head x H(7)
    {4, 128, SEG_HEAD, SEG_ACC, 1, 4, 10, 1, 1},    // 13: head x h_dir
};
// floats of one workgroup's slab: the M x N partial sums and the M bias sums
constexpr int64_t wg_slab_floats(int t) {
    return (int64_t)kWgShape[t].M * kWgShape[t].N + kWgShape[t].M;
}

// Task 9 (xyz_encoding_final) launches nothing: nr_wgrad_dir_feat forms its
// gradient from task 10's.  The sigma-only graph (rendering_shadows.py:167)
// has no xyz_encoding_final (task 9), dir_encoding (10, 11) or rgb head (13)
// either: their gradients are not computed (written as 0; the autograd leaves
// them None)
constexpr int kNoLaunch = 1 << 9;
constexpr int kNoLaunchSigma = kNoLaunch | (1 << 10) | (1 << 11) | (1 << 13);

// f16x3: the tasks that read the same saved segment run fused (wgrad3_body's
// extra operand): the primary's workgroups also compute the partner's output
// over the same block ranges into the partner's slabs, so DZ(4), H(7) and
// dz_dir (2.5 KB/sample) are read once.  The partner keeps its slabs and its
// reduction but launches no workgroups of its own.  (Task 9,
// xyz_encoding_final = DZ(8) x H(7), launches nothing, so the sigma head
// pairs with task 10, which reads H(7) too.)
constexpr int kFused[2][2] = {{5, 4}, {10, 12}};   // {primary, partner}
// bit i: pair i of kFused (f16x3 6: no spills, measured slower)
constexpr int kFuseMask = 7;
// the same for the gathering kernels (the *_active entry points): the fused
// PE pair (bit 0) leaves wgrad3_kernel<true, ROWS> 33 spilled VGPRs (8
// without it), and unfused its fine-pass launch runs 1.97 -> 1.83 ms
// (three alternating same-box rounds, profiles/r04/abalt_fuse6)
constexpr int kFuseMaskGather = 6;
// wgrad4_kernel fuses the sigma head into task 10 only
constexpr int kFuseMaskW4 = 2;

// What the plan (and the launch) needs to know of an arithmetic.  Each object
// of wgrad.hip asserts that its build configuration equals its row.
struct WgArith {
    bool split;      // operands split into pieces (x3.h), else exact fp32 MFMAs
    int nprod;       // piece products per fp32 product (x3::kNProd)
    bool fuse;       // runs the kFused pairs fused (wgrad_common.h kFuse)
    bool w4;         // has the LDS-DMA kernel (wgrad4_kernel)
    bool lists;      // has the *_active / *_listed entry points
};
constexpr WgArith kArithF32{false, 1, false, false, true};
constexpr WgArith kArithBf16x6{true, 6, false, false, true};
constexpr WgArith kArithF16x3{true, 3, true, true, true};
constexpr WgArith kArithBf16{true, 1, true, false, false};
constexpr WgArith kAriths[4] = {kArithF32, kArithBf16x6, kArithF16x3, kArithBf16};

// per-block cost of a task's workgroup, in cycles: the MFMA time of its
// busiest SIMD (fp32: 16 k-steps x 64 cycles per tile; bf16x6: 2 x 6 x 32),
// or the staging of (M + N) x 32 floats at ~8 B/cycle per CU, plus a fixed
// barrier/LDS-store overhead
constexpr int64_t wgrad_task_cost(const WgArith& A, int t) {
    const WgShape& S = kWgShape[t];
    const int mt = (S.M / S.wm + 31) / 32;
    const int nt = (S.N / S.wn + 31) / 32;
    const int64_t per_tile = A.split ? 64 * A.nprod : 1024;
    const int64_t mfma = per_tile * mt * nt * (S.wm * S.wn > 4 ? 2 : 1);
    const int64_t bytes = (int64_t)(S.M + S.N) * 32 * 4;
    return (mfma > bytes / 8 ? mfma : bytes / 8) + 512;
}
// tasks at least this costly are "heavy" (dispatched first, see wgrad_plan)
constexpr int64_t wgrad_heavy_cost(const WgArith& A) { return A.split ? 1024 * A.nprod : 16384; }

struct WgPlanTask {
    int id;          // task id (row of kWgShape)
    int G;           // workgroups splitting its sample blocks; 0: not computed
    int64_t slab;    // slab offset (floats) of workgroup 0
    int fuse;        // dispatch position of the partner whose output this task's
                     // workgroups also compute, or -1
    int pa, pb;      // slab row / column order (1 natural; WgShape::pa / pb under wgrad4)
};
struct WgPlan {
    WgPlanTask task[kTasks];     // in dispatch order
    int wg_start[kTasks + 1];    // first workgroup of every position; [kTasks] = the grid
    int64_t slab_floats;         // the launch's whole slab extent
};

// The plan of one launch over nb 32-sample blocks.  over_list: a launch over a
// sample list -- gathering (*_active) or over buffers saved by position
// (*_listed, the deferred save): both use the same split-K partition, so the
// two give bit-identical sums.  use_w4: wgrad4_kernel runs it (the caller
// decides; f16x3's full graph only).
constexpr WgPlan wgrad_plan(const WgArith& A, bool sigma_only, bool over_list, bool use_w4,
                            int64_t nb) {
    int64_t cost[kTasks] = {}, tot = 0;
    for (int t = 0; t < kTasks; ++t) tot += cost[t] = wgrad_task_cost(A, t);
    // dispatch order: the heavy tasks first; the small ones last and split ~3x
    // finer, so their short workgroups fill the tail of the final round
    const int64_t heavy = wgrad_heavy_cost(A);
    int order[kTasks] = {}, no = 0;
    for (int pass = 0; pass < 2; ++pass)
        for (int t = 0; t < kTasks; ++t)
            if ((cost[t] >= heavy) == (pass == 0)) order[no++] = t;
    const int none = sigma_only ? kNoLaunchSigma : kNoLaunch;
    const int64_t target_wg = !over_list ? kTargetWG : (use_w4 ? kTargetWGW4 : kTargetWGGather);
    auto clip = [nb](int64_t g) { return g < 1 ? 1 : (g < nb ? g : nb); };
    int64_t gt[kTasks] = {};
    int pos[kTasks] = {};
    for (int k = 0; k < kTasks; ++k) {
        const int t = order[k];
        // the 4-row head tasks' per-block time is mostly fixed cost, not
        // bytes: always split finer, so they fill the tail of the last round
        const int split = cost[t] >= heavy && !kWgShape[t].head() ? 1 : 3;
        gt[t] = (none >> t) & 1 ? 0 : clip(split * ((target_wg * cost[t] + tot - 1) / tot));
        pos[t] = k;
    }
    int partner[kTasks] = {};
    bool absorbed[kTasks] = {};
    for (int t = 0; t < kTasks; ++t) partner[t] = -1;
    if (A.fuse) {
        const int fmask = use_w4 ? kFuseMaskW4
                        : over_list ? (kFuseMask & kFuseMaskGather)
                                    : kFuseMask;
        for (int i = 0; i < 2; ++i) {
            const int p = kFused[i][0], q = kFused[i][1];
            if (!((fmask >> i) & 1) || ((none >> p) & 1) || ((none >> q) & 1)) continue;   // both must run
            gt[q] = gt[p] = clip((target_wg * (cost[p] + cost[q]) + tot - 1) / tot);
            partner[p] = q;
            absorbed[q] = true;
        }
    }
    WgPlan P{};
    for (int k = 0; k < kTasks; ++k) {
        const int t = order[k];
        P.task[k] = {t, (int)gt[t], P.slab_floats, partner[t] >= 0 ? pos[partner[t]] : -1,
                     use_w4 ? kWgShape[t].pa : 1, use_w4 ? kWgShape[t].pb : 1};
        P.slab_floats += gt[t] * wg_slab_floats(t);
        P.wg_start[k + 1] = P.wg_start[k] + (absorbed[t] ? 0 : (int)gt[t]);
    }
    return P;
}

// Slab floats of the largest plan any launch can ask for: the maximum over the
// four arithmetics and every path each one has.  G_t = min(g_t, nb) is
// non-decreasing in nb and every g_t < 3 * (kTargetWGW4 + 1) < 65,536 = the
// blocks of wgrad_launch's largest wgrad4 launch (n = 2^21 - 1), so that nb
// attains the maximum of every path.
constexpr int64_t wgrad_plan_max_floats() {
    constexpr int64_t nb = 65536;
    int64_t m = 0;
    for (const WgArith& A : kAriths)
        for (int sigma = 0; sigma < 2; ++sigma)
            for (int list = 0; list <= (A.lists ? 1 : 0); ++list)
                for (int w4 = 0; w4 <= (A.w4 && !sigma ? 1 : 0); ++w4) {
                    const int64_t f = wgrad_plan(A, sigma, list, w4, nb).slab_floats;
                    m = f > m ? f : m;
                }
    return m;
}

}  // namespace
