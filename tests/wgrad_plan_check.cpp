// CPU check of the weight gradient's launch plan (nerf_pl_amd/csrc/wgrad_plan.h):
// every arithmetic, graph, path and use_w4 value an object really has, over
// block counts below, between and above the tasks' G.  Built and run by
// tests/test_wgrad_plan.py under the address and undefined-behaviour
// sanitizers.  A violated property is printed and ends the run with status 1;
// the recorded totals are compared after the properties, every row that differs
// is printed, and any of them makes the status 2.
#include <stdio.h>
#include <stdlib.h>

#include "../nerf_pl_amd/csrc/wgrad_plan.h"

#define CHECK(cond, ...)                                                       \
    do {                                                                       \
        if (!(cond)) {                                                         \
            fprintf(stderr, "%s:%d: %s failed: ", __FILE__, __LINE__, #cond);  \
            fprintf(stderr, __VA_ARGS__);                                      \
            fprintf(stderr, "\n");                                             \
            exit(1);                                                           \
        }                                                                      \
    } while (0)

static const char* const kNames[4] = {"fp32", "bf16x6", "f16x3", "bf16"};
static const int64_t kNb[] = {1, 2, 7, 31, 130, 971, 65536, 3125000};

static int wgs(const WgPlan& P) { return P.wg_start[kTasks]; }

static int position(const WgPlan& P, int id) {
    for (int k = 0; k < kTasks; ++k)
        if (P.task[k].id == id) return k;
    return -1;
}

static bool fused(const WgPlan& P, int primary, int partner) {
    const int k = position(P, primary);
    return P.task[k].fuse >= 0 && P.task[P.task[k].fuse].id == partner;
}

static void check_plan(int ai, bool sigma, bool list, bool w4, int64_t nb, int64_t max_floats) {
    const WgArith& A = kAriths[ai];
    const WgPlan P = wgrad_plan(A, sigma, list, w4, nb);
    char tag[96];
    snprintf(tag, sizeof tag, "%s sigma=%d list=%d w4=%d nb=%lld", kNames[ai], sigma, list, w4,
             (long long)nb);
    bool seen[kTasks] = {}, absorbed[kTasks] = {};
    for (int k = 0; k < kTasks; ++k) {
        const WgPlanTask& T = P.task[k];
        CHECK(T.id >= 0 && T.id < kTasks && !seen[T.id], "%s: position %d", tag, k);
        seen[T.id] = true;
        CHECK(T.fuse >= -1 && T.fuse < kTasks && T.fuse != k, "%s: task %d fuse %d", tag, T.id, T.fuse);
        if (T.fuse >= 0) {
            CHECK(!absorbed[T.fuse], "%s: position %d absorbed twice", tag, T.fuse);
            absorbed[T.fuse] = true;
        }
    }
    int64_t slab = 0;
    int sum_g = 0;
    CHECK(P.wg_start[0] == 0, "%s", tag);
    for (int k = 0; k < kTasks; ++k) {
        const WgPlanTask& T = P.task[k];
        const bool none = T.id == 9 || (sigma && (T.id == 10 || T.id == 11 || T.id == 13));
        if (none) CHECK(T.G == 0 && T.fuse < 0 && !absorbed[k], "%s: task %d must not run", tag, T.id);
        else CHECK(T.G >= 1 && T.G <= nb, "%s: task %d G %d", tag, T.id, T.G);
        // slabs: disjoint and contiguous in dispatch order, G * (M N + M) floats each
        CHECK(T.slab == slab, "%s: task %d slab %lld, expected %lld", tag, T.id, (long long)T.slab,
              (long long)slab);
        slab += (int64_t)T.G * ((int64_t)kWgShape[T.id].M * kWgShape[T.id].N + kWgShape[T.id].M);
        CHECK(P.wg_start[k + 1] >= P.wg_start[k], "%s: wg_start decreases at %d", tag, k);
        // an absorbed partner adds no workgroups; every other task adds its G
        CHECK(P.wg_start[k + 1] - P.wg_start[k] == (absorbed[k] ? 0 : T.G), "%s: task %d", tag, T.id);
        if (!absorbed[k]) sum_g += T.G;
        if (T.fuse >= 0)
            CHECK(P.task[T.fuse].G == T.G, "%s: pair %d/%d G %d != %d", tag, T.id, P.task[T.fuse].id,
                  T.G, P.task[T.fuse].G);
        CHECK(T.pa == (w4 ? kWgShape[T.id].pa : 1) && T.pb == (w4 ? kWgShape[T.id].pb : 1),
              "%s: task %d pa %d pb %d", tag, T.id, T.pa, T.pb);
        if (k > 0)   // heavy tasks precede light ones
            CHECK(wgrad_task_cost(A, P.task[k - 1].id) >= wgrad_heavy_cost(A) ||
                      wgrad_task_cost(A, T.id) < wgrad_heavy_cost(A),
                  "%s: heavy task %d after light task %d", tag, T.id, P.task[k - 1].id);
    }
    CHECK(wgs(P) == sum_g, "%s: %d workgroups, sum of G %d", tag, wgs(P), sum_g);
    CHECK(P.slab_floats == slab, "%s: total %lld, slabs end at %lld", tag,
          (long long)P.slab_floats, (long long)slab);
    CHECK(P.slab_floats <= max_floats, "%s: %lld floats exceed the workspace's %lld", tag,
          (long long)P.slab_floats, (long long)max_floats);
    // the fused pairs: only f16x3 / bf16 fuse.  {5, 4}: the register-staged
    // kernels without a sample list; {10, 12}: every path of the full graph
    // (the sigma-only graph has no task 10)
    CHECK(fused(P, 5, 4) == (A.fuse && !list && !w4), "%s: pair {5, 4}", tag);
    CHECK(fused(P, 10, 12) == (A.fuse && !sigma), "%s: pair {10, 12}", tag);
    for (int k = 0; k < kTasks; ++k)
        if (P.task[k].fuse >= 0)
            CHECK(P.task[k].id == 5 || P.task[k].id == 10, "%s: task %d fuses", tag, P.task[k].id);
}

// (total slab floats, workgroups) of the parent's wgrad_launch, transcribed
struct Expect {
    int arith;
    bool sigma, list, w4;   // w4: NR_WGRAD_W4 in the environment
    int64_t big_floats;     // nb >= 65536 (the wgrad4 row, list && w4: nb == 65536)
    int big_wgs;
    int64_t floats7;      // nb == 7
    int wgs7;
};
static const Expect kExpect[] = {
    {0, false, false, false, 42743844, 972, 3727416, 91},
    {0, false, true, false, 57549864, 1305, 3727416, 91},
    {0, true, false, false, 38586120, 768, 3463964, 70},
    {0, true, true, false, 51940956, 1032, 3463964, 70},
    {1, false, false, false, 37871288, 1038, 3727416, 91},
    {1, false, true, false, 51175964, 1398, 3727416, 91},
    {1, true, false, false, 35824060, 851, 3463964, 70},
    {1, true, true, false, 48411724, 1145, 3463964, 70},
    {2, false, false, false, 39926876, 739, 3727416, 77},
    {2, false, false, true, 39926876, 739, 3727416, 84},
    {2, false, true, false, 48553260, 998, 3727416, 84},
    {2, false, true, true, 72366912, 1490, 3727416, 84},
    {2, true, false, false, 36921788, 675, 3463964, 63},
    {2, true, true, false, 44484684, 909, 3463964, 70},
    {3, false, false, false, 39926876, 739, 3727416, 77},
    {3, true, false, false, 36921788, 675, 3463964, 63},
};

int main() {
    const int64_t max_floats = wgrad_plan_max_floats();
    CHECK(max_floats * 4 == 289467648, "workspace %lld bytes", (long long)(max_floats * 4));
    // the four arithmetics as their objects are built (x3.h)
    CHECK(!kArithF32.split && !kArithF32.fuse && !kArithF32.w4 && kArithF32.lists, "fp32");
    CHECK(kArithBf16x6.split && kArithBf16x6.nprod == 6 && !kArithBf16x6.fuse && !kArithBf16x6.w4 &&
              kArithBf16x6.lists, "bf16x6");
    CHECK(kArithF16x3.split && kArithF16x3.nprod == 3 && kArithF16x3.fuse && kArithF16x3.w4 &&
              kArithF16x3.lists, "f16x3");
    CHECK(kArithBf16.split && kArithBf16.nprod == 1 && kArithBf16.fuse && !kArithBf16.w4 &&
              !kArithBf16.lists, "bf16");
    int plans = 0, rows = 0, wrong = 0;
    bool attained = false;
    for (int ai = 0; ai < 4; ++ai)
        for (int sigma = 0; sigma < 2; ++sigma)
            for (int list = 0; list <= (kAriths[ai].lists ? 1 : 0); ++list)
                for (int w4 = 0; w4 <= (kAriths[ai].w4 && !sigma ? 1 : 0); ++w4)
                    for (int64_t nb : kNb) {
                        check_plan(ai, sigma, list, w4, nb, max_floats);
                        ++plans;
                        if (wgrad_plan(kAriths[ai], sigma, list, w4, nb).slab_floats == max_floats) {
                            // the f16x3 full graph over a sample list with the LDS-DMA kernel
                            CHECK(ai == 2 && !sigma && list && w4, "maximum attained by %s", kNames[ai]);
                            attained = true;
                        }
                    }
    CHECK(attained, "no plan reaches the workspace size");
    printf("properties: %d plans hold; workspace %lld bytes\n", plans, (long long)(max_floats * 4));
    // the totals: every path has a row, every row a path; each mismatch is listed
    // A row's w4 is NR_WGRAD_W4 in the environment; the launch's use_w4 follows
    // wgrad_launch's rule, n < 2^21 (tests/test_wgrad_plan.py asserts that the
    // rule sits there).  The big column is a launch of nb full blocks, n = 32 nb
    // >= 2^21, where the f16x3 full graph falls back to the W4=0 plan -- but
    // for the wgrad4 row (over a list), whose nb = 65536 is n = 2^21 - 1, the
    // largest launch wgrad4_kernel takes; past it that row falls back as well.
    for (const Expect& E : kExpect) {
        const WgArith& A = kAriths[E.arith];
        CHECK((!E.list || A.lists) && (!E.w4 || (A.w4 && !E.sigma)), "row %d: no such path", rows);
        ++rows;
        const Expect* fallback = &E;   // the same path with NR_WGRAD_W4=0
        for (const Expect& F : kExpect)
            if (F.arith == E.arith && F.sigma == E.sigma && F.list == E.list && !F.w4) fallback = &F;
        for (int64_t nb : kNb) {
            if (nb != 7 && nb < 65536) continue;
            const int64_t n = E.w4 && E.list && nb == 65536 ? ((int64_t)1 << 21) - 1 : 32 * nb;
            const bool use_w4 = E.w4 && n < (int64_t)1 << 21;
            const Expect& X = E.w4 && !use_w4 && E.list ? *fallback : E;
            const WgPlan P = wgrad_plan(A, E.sigma, E.list, use_w4, nb);
            const int64_t floats = nb == 7 ? X.floats7 : X.big_floats;
            const int n_wg = nb == 7 ? X.wgs7 : X.big_wgs;
            if (P.slab_floats == floats && wgs(P) == n_wg) continue;
            ++wrong;
            printf("totals: %s sigma=%d list=%d w4=%d nb=%lld: %lld floats / %d workgroups, expected "
                   "%lld / %d\n", kNames[E.arith], E.sigma, E.list, E.w4, (long long)nb,
                   (long long)P.slab_floats, wgs(P), (long long)floats, n_wg);
        }
    }
    CHECK(rows * (int)(sizeof kNb / sizeof kNb[0]) == plans, "%d rows for %d plans", rows, plans);
    printf("totals: %d of %d rows differ\n", wrong, rows);
    return wrong ? 2 : 0;
}
