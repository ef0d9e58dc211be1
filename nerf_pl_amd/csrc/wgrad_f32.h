// Weight gradient (wgrad.hip): the exact-fp32 kernel on v_mfma_f32_32x32x2_f32,
// described at the top of wgrad.hip.
#pragma once
#include <type_traits>

#include "wgrad_common.h"

#if NR_X3_BASE_OBJECT   // the fp32-MFMA kernel lives in the bf16x6 object only
namespace {

constexpr int kCol = 36;         // LDS column stride (floats): [column][32 samples + 4 pad]
constexpr int kBufA = 256 * kCol;  // one operand region
constexpr int kBuf = 2 * kBufA;    // one buffer = A + B regions

// Staging geometry of one 32-sample block of a segment, all compile time:
// float4 e = tid + 512*i lands at LDS [sample j][column c].  In the
// block-native order float4 e is (t = e>>8, q = (e>>6)&3, lane = e&63).
template <int KIND, int W>
struct SegGeo {
    static constexpr int F4 = KIND == SEG_HEAD ? 32 : W * 8;     // float4 per block
    static constexpr int ITERS = (F4 + kThreads - 1) / kThreads;
    __device__ static __forceinline__ int j(int tid) { return KIND == SEG_HEAD ? tid : (tid & 31); }
    // column of float4 #i of thread tid
    __device__ static __forceinline__ int c(int tid, int i) {
        const int h = (tid >> 5) & 1, w = (tid >> 6) & 3, hi = tid >> 8;
        if constexpr (KIND == SEG_ACC) return 32 * (2 * i + hi) + 8 * w + 4 * h;   // t = 2i+hi, q = w
        else if constexpr (KIND == SEG_PE) return 32 * h + 4 * (8 * i + 4 * hi + w);  // gq = 8i+4hi+w
        else if constexpr (KIND == SEG_DPE) return 16 * h + 4 * w;               // gq = w (hi = 0)
        else return 0;
    }
};

// ROWS staging geometry of an input segment (sample-major rows of W): float4
// e = tid + 512 i is chunk (e & 3) + 4 (e >> 7) of sample (e >> 2) & 31, so a
// wave instruction reads 16 rows x 64 contiguous bytes (not 32 rows x 32 B)
// while the [column][sample] image writes stay at most 2-way bank conflicted
// (free for ds_write_b32); a thread's sample is the same in every iteration
template <int KIND, int W>
struct RowGeo {
    static constexpr int F4 = W * 8;
    static constexpr int ITERS = (F4 + kThreads - 1) / kThreads;
    __device__ static __forceinline__ int j(int tid) { return (tid >> 2) & 31; }
    __device__ static __forceinline__ int c(int tid, int i) {
        return 4 * ((tid & 3) + 4 * ((tid + kThreads * i) >> 7));
    }
};

// GAT: over the packed sample list (the fp32 *_active entry points): the
// gradient operand is read by position, the input operand gathered, each
// thread resolving one sample per stage; positions past m stage zeros.
// ROWS: the input operand saved as sample-major rows (mlp_fwd.hip, the full
// graph): the float4 of column c of sample s is row s at c -- a gathered
// sample's 128-B lines are read whole, and the same thread -> (sample,
// column) mapping keeps the LDS image writes conflict-free.  Else
// block-native: the float4 sits at (s >> 5) * F4 + (e & ~31) + (s & 31).
template <int KA, int WA, int KB, int WB, int WM, int WN, bool GAT = false, bool ROWS = false>
__device__ __forceinline__ void wgrad_body(const WgArgs& a, const WgTask& T, int b0, int b1,
                                           float* lds, float* __restrict__ slab) {
    using GA = SegGeo<KA, WA>;
    using GB = std::conditional_t<ROWS && KB != SEG_HEAD, RowGeo<KB, WB>, SegGeo<KB, WB>>;
    constexpr int MT = (WA / WM + 31) / 32, NT = (WB / WN + 31) / 32;
    constexpr int M = WA, N = WB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool active = wave < WM * WN;          // waves beyond the grid only stage
    const int mi = wave / WN, ni = wave % WN;
    const int m0 = 32 * MT * mi, n0 = 32 * NT * ni;
    const bool do_bias = active && ni == 0;

    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = f32x16{};
    float bsum[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) bsum[i] = 0.f;

    // per-thread staging addresses: global float4 index tid + 256 i, LDS [j][c]
    const bool ta = tid < GA::F4, tb = tid < GB::F4;
    const int ja = GA::j(tid), jb = GB::j(tid);
    f32x4 ra[GA::ITERS], rb[GB::ITERS];
    const int m = wg_m(a);
    auto load = [&](int blk) {
        const f32x4* pa = reinterpret_cast<const f32x4*>(T.a.base) + (size_t)blk * GA::F4 + tid;
        const f32x4* pb;
        if constexpr (ROWS) {
            const int sj = GAT ? a.slist[min(blk * 32 + jb, m - 1)] : blk * 32 + jb;
            const float* row = T.b.base + (size_t)sj * WB;
#pragma unroll
            for (int i = 0; i < GA::ITERS; ++i) if (ta) ra[i] = pa[kThreads * i];
#pragma unroll
            for (int i = 0; i < GB::ITERS; ++i)
                if (tb) rb[i] = *reinterpret_cast<const f32x4*>(row + GB::c(tid, i));
            return;
        } else if constexpr (GAT) {
            const int sj = a.slist[min(blk * 32 + jb, m - 1)];
            pb = reinterpret_cast<const f32x4*>(T.b.base) + (size_t)(sj >> 5) * GB::F4 +
                 (tid - jb) + (sj & 31);
        } else {
            pb = reinterpret_cast<const f32x4*>(T.b.base) + (size_t)blk * GB::F4 + tid;
        }
#pragma unroll
        for (int i = 0; i < GA::ITERS; ++i) if (ta) ra[i] = pa[kThreads * i];
#pragma unroll
        for (int i = 0; i < GB::ITERS; ++i) if (tb) rb[i] = pb[kThreads * i];
    };
    // write the staged block to LDS as [column][sample] (4 ds_write_b32 per
    // float4; lanes are consecutive samples -> conflict-free); samples >= n of
    // the tail block become 0
    auto store = [&](int buf, int blk) {
        const int nval = m - blk * 32;
        const bool ka = ja < nval, kb = jb < nval;
        float* la = lds + buf * kBuf + ja;
        float* lb = lds + buf * kBuf + kBufA + jb;
        if (ta)
#pragma unroll
            for (int i = 0; i < GA::ITERS; ++i) {
                const f32x4 v = ka ? ra[i] : f32x4{};
                const int c = GA::c(tid, i);
#pragma unroll
                for (int e = 0; e < 4; ++e) la[(c + e) * kCol] = v[e];
            }
        if (tb)
#pragma unroll
            for (int i = 0; i < GB::ITERS; ++i) {
                const f32x4 v = kb ? rb[i] : f32x4{};
                const int c = GB::c(tid, i);
#pragma unroll
                for (int e = 0; e < 4; ++e) lb[(c + e) * kCol] = v[e];
            }
    };

    const int nst = b1 - b0;
    if (nst > 0) {
        load(b0);
        store(0, b0);
    }
    __syncthreads();
    const int h = lane >> 5, col = lane & 31;
#pragma unroll 1
    for (int st = 0; st < nst; ++st) {
        const int buf = st & 1;
        if (st + 1 < nst) load(b0 + st + 1);
        // k-step kk pairs samples kk (lane half 0) and 16 + kk (half 1): a lane's
        // 16 samples of one column are contiguous -> 4 ds_read_b128 per column
        const float* la = lds + buf * kBuf + (m0 + col) * kCol + 16 * h;
        const float* lb = lds + buf * kBuf + kBufA + (n0 + col) * kCol + 16 * h;
        if (active) {
            f32x4 av[2][MT], bv[2][NT];
            auto rd = [&](int q, int p) {   // samples 4q..4q+3 of this lane half
#pragma unroll
                for (int i = 0; i < MT; ++i) av[p][i] = *reinterpret_cast<const f32x4*>(la + 32 * i * kCol + 4 * q);
#pragma unroll
                for (int j = 0; j < NT; ++j) bv[p][j] = *reinterpret_cast<const f32x4*>(lb + 32 * j * kCol + 4 * q);
            };
            auto mm = [&](int p) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
#pragma unroll
                    for (int i = 0; i < MT; ++i)
#pragma unroll
                        for (int j = 0; j < NT; ++j)
                            acc[i][j] = nr_mfma32(av[p][i][e], bv[p][j][e], acc[i][j]);
#pragma unroll
                    for (int i = 0; i < MT; ++i) bsum[i] += av[p][i][e];
                }
            };
            rd(0, 0);
            rd(1, 1);
            __builtin_amdgcn_sched_barrier(0);
            mm(0);
            rd(2, 0);
            __builtin_amdgcn_sched_barrier(0);
            mm(1);
            rd(3, 1);
            __builtin_amdgcn_sched_barrier(0);
            mm(0);
            __builtin_amdgcn_sched_barrier(0);
            mm(1);
        }
        if (st + 1 < nst) store(buf ^ 1, b0 + st + 1);
        __syncthreads();
    }
    if (!active) return;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = m0 + 32 * i + nr_acc_row(r, h);
                const int c = n0 + 32 * j + col;
                if (o < M && c < N) slab[o * N + c] = acc[i][j][r];
            }
        if (do_bias) {
            const float b = bsum[i] + __shfl_xor(bsum[i], 32);
            const int o = m0 + 32 * i + col;
            if (h == 0 && o < M) slab[M * N + o] = b;
        }
    }
}

template <bool GA, bool ROWS>
__global__ void __launch_bounds__(kThreads, 2) wgrad_kernel(WgArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[2 * kBuf];   // 144 KiB
    const auto [c, T, b0, b1, slab] = WgWork(a);
    // task shapes (see nr_wgrad's task list); wave-uniform
    // (WM, WN) = wave grid over the task's output (<= 8 waves; 128 accumulators max)
    switch (__builtin_amdgcn_readfirstlane(T.id)) {
        case 0: case 4:
            wgrad_body<SEG_ACC, 256, SEG_PE, 64, 8, 1, GA, ROWS>(a, T, b0, b1, lds, slab); break;
        case 10:
            wgrad_body<SEG_ACC, 128, SEG_ACC, 256, 2, 4, GA, ROWS>(a, T, b0, b1, lds, slab); break;
        case 11:
            wgrad_body<SEG_ACC, 128, SEG_DPE, 32, 4, 1, GA, ROWS>(a, T, b0, b1, lds, slab); break;
        case 12:
            wgrad_body<SEG_HEAD, 4, SEG_ACC, 256, 1, 8, GA, ROWS>(a, T, b0, b1, lds, slab); break;
        case 13:
            wgrad_body<SEG_HEAD, 4, SEG_ACC, 128, 1, 4, GA, ROWS>(a, T, b0, b1, lds, slab); break;
        default:
            wgrad_body<SEG_ACC, 256, SEG_ACC, 256, 2, 4, GA, ROWS>(a, T, b0, b1, lds, slab); break;
    }
}

}  // namespace
#endif  // NR_X3_BASE_OBJECT
