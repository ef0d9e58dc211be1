// Fused SGD, RAdam and Ranger steps over every parameter tensor of the NeRF
// pair (include/nerf_pl_amd_optim.h): the rest of the reference's optimizer
// choice (opt.py --optimizer sgd|adam|radam|ranger, utils/__init__.py:10-30;
// RAdam and Ranger are utils/optimizers.py:6-95 and :266-405, loops of about
// ten elementwise torch ops per tensor).  adam.hip is the fourth.
//
// As in adam.hip the tensor table travels in the kernel arguments and one
// launch updates all tensors, each element read once and written once.  These
// kernels move 16 bytes per access: the work unit is a chunk of 4 consecutive
// elements of ONE tensor (a tensor of n elements has ceil(n / 4) chunks, the
// last one short), each thread finds its chunk's tensor by a binary search
// over the table's chunk offsets, and takes the chunk as one f32x4 per array
// when it is whole and every pointer of the tensor is 16-byte aligned -- else
// element by element, so any length and any 4-byte aligned start is right.
// Arithmetic is the optimizer's, op for op, in unfused fp32:
//   SGD    torch/optim/sgd.py (_single_tensor_sgd, dampening 0, no nesterov)
//   RAdam  exp_avg_sq.mul_(b2).addcmul_(1 - b2, g, g); exp_avg.mul_(b1).add_(1 - b1, g)
//          p.add_(-wd * lr, p); p.addcdiv_(-step_size * lr, exp_avg, sqrt(v) + eps)
//          (addcdiv is self + value * t1 / t2, addcmul self + value * t1 * t2,
//          evaluated left to right as torch's CPU kernels do)
//   Ranger the same, then slow.add_(alpha, p - slow); p.copy_(slow) every k-th step
#include "common.h"

namespace {

constexpr int kOptMax = 48;

enum { kRectified = 0, kSgdLike = 1, kSkip = 2 };

// where a chunk lives: tensor k, first element i, n (1..4) elements, and
// whether it may move as one f32x4
struct Chunk { int k; int64_t i; int n; bool vec; };

template <typename Args>
__device__ __forceinline__ Chunk locate(const Args& a, int64_t c) {
    int lo = 0, hi = a.count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.start[mid] <= c) lo = mid; else hi = mid - 1;
    }
    const int64_t j = c - a.start[lo];
    const bool last = j + 1 == a.start[lo + 1] - a.start[lo];
    Chunk ch;
    ch.k = lo;
    ch.i = j * 4;
    ch.n = last ? (int)a.tail[lo] : 4;
    ch.vec = ch.n == 4 && ((a.aligned >> lo) & 1);
    return ch;
}

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// ---------------------------------------------------------------------------
// SGD
// ---------------------------------------------------------------------------
struct SgdArgs {
    float* p[kOptMax];
    const float* g[kOptMax];
    float* buf[kOptMax];
    int64_t start[kOptMax + 1];    // in chunks
    uint64_t aligned;              // bit k: every pointer of tensor k is 16-byte aligned
    uint8_t tail[kOptMax];         // elements of tensor k's last chunk
    int count;
    int has_momentum, first;
    float wd, momentum, neg_lr;
};

__device__ __forceinline__ void sgd_elem(const SgdArgs& a, float& p, float g, float& buf) {
    if (a.wd != 0.f) g = nr_add(g, nr_mul(a.wd, p));
    if (a.has_momentum) {
        buf = a.first ? g : nr_add(nr_mul(buf, a.momentum), g);
        g = buf;
    }
    p = nr_add(p, nr_mul(a.neg_lr, g));
}

__global__ void __launch_bounds__(256) sgd_kernel(const SgdArgs a) {
    const int64_t total = a.start[a.count];
    const bool rd_buf = a.has_momentum && !a.first;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < total;
         c += (int64_t)gridDim.x * blockDim.x) {
        const Chunk ch = locate(a, c);
        float* pp = a.p[ch.k] + ch.i;
        const float* gp = a.g[ch.k] + ch.i;
        float* bp = a.has_momentum ? a.buf[ch.k] + ch.i : nullptr;
        if (ch.vec) {
            f32x4 p = ld4(pp), g = ld4(gp), b = {0.f, 0.f, 0.f, 0.f};
            if (rd_buf) b = ld4(bp);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                float pt = p[t], bt = b[t];
                sgd_elem(a, pt, g[t], bt);
                p[t] = pt; b[t] = bt;
            }
            if (a.has_momentum) st4(bp, b);
            st4(pp, p);
        } else {
            for (int t = 0; t < ch.n; ++t) {
                float p = pp[t], b = rd_buf ? bp[t] : 0.f;
                sgd_elem(a, p, gp[t], b);
                if (a.has_momentum) bp[t] = b;
                pp[t] = p;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// RAdam / Ranger
// ---------------------------------------------------------------------------
struct RAdamArgs {
    float* p[kOptMax];
    const float* g[kOptMax];
    float* m[kOptMax];
    float* v[kOptMax];
    float* slow[kOptMax];
    int64_t start[kOptMax + 1];    // in chunks
    uint64_t aligned;
    uint8_t tail[kOptMax];
    int count;
    int mode, has_decay, sync;
    float beta1, w1, beta2, w2, eps, decay, neg_step, alpha;
};

// p and slow are meaningful (and written back by the caller) only where the
// caller's own flags say so: p unless skipped without a sync, slow on a sync
__device__ __forceinline__ void radam_elem(const RAdamArgs& a, float& p, float g, float& m,
                                           float& v, float& slow) {
    v = nr_add(nr_mul(v, a.beta2), nr_mul(nr_mul(a.w2, g), g));
    m = nr_add(nr_mul(m, a.beta1), nr_mul(a.w1, g));
    if (a.mode != kSkip) {
        if (a.has_decay) p = nr_add(p, nr_mul(a.decay, p));
        if (a.mode == kRectified) {
            const float denom = nr_add(sqrtf(v), a.eps);
            p = nr_add(p, nr_mul(a.neg_step, m) / denom);
        } else {
            p = nr_add(p, nr_mul(a.neg_step, m));
        }
    }
    if (a.sync) {
        slow = nr_add(slow, nr_mul(a.alpha, nr_sub(p, slow)));
        p = slow;
    }
}

__global__ void __launch_bounds__(256) radam_kernel(const RAdamArgs a) {
    const int64_t total = a.start[a.count];
    const bool use_p = a.mode != kSkip || a.sync;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < total;
         c += (int64_t)gridDim.x * blockDim.x) {
        const Chunk ch = locate(a, c);
        float* pp = a.p[ch.k] + ch.i;
        const float* gp = a.g[ch.k] + ch.i;
        float* mp = a.m[ch.k] + ch.i;
        float* vp = a.v[ch.k] + ch.i;
        float* sp = a.sync ? a.slow[ch.k] + ch.i : nullptr;
        if (ch.vec) {
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            f32x4 g = ld4(gp), m = ld4(mp), v = ld4(vp);
            f32x4 p = use_p ? ld4(pp) : z;
            f32x4 s = a.sync ? ld4(sp) : z;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                float pt = p[t], mt = m[t], vt = v[t], st = s[t];
                radam_elem(a, pt, g[t], mt, vt, st);
                p[t] = pt; m[t] = mt; v[t] = vt; s[t] = st;
            }
            st4(vp, v);
            st4(mp, m);
            if (use_p) st4(pp, p);
            if (a.sync) st4(sp, s);
        } else {
            for (int t = 0; t < ch.n; ++t) {
                float p = use_p ? pp[t] : 0.f, m = mp[t], v = vp[t], s = a.sync ? sp[t] : 0.f;
                radam_elem(a, p, gp[t], m, v, s);
                vp[t] = v;
                mp[t] = m;
                if (use_p) pp[t] = p;
                if (a.sync) sp[t] = s;
            }
        }
    }
}

constexpr int64_t kMaxNumel = (int64_t)1 << 48;     // 48 tensors of it stay below 2^63

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

inline unsigned grid_of(int64_t chunks) {
    // memory-bound: at most 8 workgroups of 256 on each of the 256 CUs, the
    // rest by the grid stride
    int64_t blocks = (chunks + 255) / 256;
    return (unsigned)(blocks > 2048 ? 2048 : blocks);
}

}  // namespace

NR_API int nr_optim_max_tensors(void) { return kOptMax; }

NR_API int nr_sgd_step(float* const* params, const float* const* grads,
                       float* const* momentum_buf, const int64_t* numel, int count, double lr,
                       double momentum, double weight_decay, int first, void* stream) {
    NR_REQUIRE(count >= 0 && count <= kOptMax, "nr_sgd_step: count %d outside [0, %d]", count,
               kOptMax);
    NR_REQUIRE(first == 0 || first == 1, "nr_sgd_step: first is 0 or 1, not %d", first);
    if (count == 0) return 0;
    NR_REQUIRE(params && grads && numel, "nr_sgd_step: null table");
    NR_REQUIRE(momentum == 0.0 || momentum_buf,
               "nr_sgd_step: null momentum_buf table with momentum %g", momentum);
    SgdArgs a{};
    a.start[0] = 0;
    for (int k = 0; k < count; ++k) {
        NR_REQUIRE(numel[k] >= 0 && numel[k] < kMaxNumel, "nr_sgd_step: bad numel[%d]", k);
        if (numel[k] > 0)
            NR_REQUIRE(params[k] && grads[k] && (momentum == 0.0 || momentum_buf[k]),
                       "nr_sgd_step: null pointer in the table (tensor %d)", k);
        a.p[k] = params[k]; a.g[k] = grads[k];
        a.buf[k] = momentum != 0.0 ? momentum_buf[k] : nullptr;
        a.start[k + 1] = a.start[k] + (numel[k] + 3) / 4;
        a.tail[k] = (uint8_t)(numel[k] == 0 ? 0 : numel[k] - ((numel[k] + 3) / 4 - 1) * 4);
        if (aligned16(a.p[k]) && aligned16(a.g[k]) && aligned16(a.buf[k]))
            a.aligned |= (uint64_t)1 << k;
    }
    a.count = count;
    a.has_momentum = momentum != 0.0;
    a.first = first;
    // scalars as torch forms them: python doubles, rounded to fp32 when applied
    a.wd = (float)weight_decay; a.momentum = (float)momentum; a.neg_lr = (float)(-lr);
    const int64_t total = a.start[count];
    if (total == 0) return 0;
    sgd_kernel<<<grid_of(total), 256, 0, (hipStream_t)stream>>>(a);
    NR_LAUNCH_CHECK("nr_sgd_step");
    return 0;
}

NR_API int nr_radam_step(float* const* params, const float* const* grads, float* const* exp_avg,
                         float* const* exp_avg_sq, float* const* slow, const int64_t* numel,
                         int count, double lr, double beta1, double beta2, double eps,
                         double weight_decay, int64_t step, int mode, double lookahead_alpha,
                         int lookahead_sync, void* stream) {
    NR_REQUIRE(count >= 0 && count <= kOptMax, "nr_radam_step: count %d outside [0, %d]", count,
               kOptMax);
    NR_REQUIRE(step >= 1, "nr_radam_step: step counts from 1");
    NR_REQUIRE(mode == kRectified || mode == kSgdLike || mode == kSkip,
               "nr_radam_step: unknown mode %d", mode);
    NR_REQUIRE(lookahead_alpha >= 0.0 && lookahead_alpha <= 1.0,
               "nr_radam_step: lookahead_alpha %g outside [0, 1]", lookahead_alpha);
    NR_REQUIRE(lookahead_sync == 0 || lookahead_sync == 1,
               "nr_radam_step: lookahead_sync is 0 or 1, not %d", lookahead_sync);
    NR_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0,
               "nr_radam_step: betas (%g, %g) outside [0, 1)", beta1, beta2);
    // step_size as utils/optimizers.py:68-80 forms it, in double, left to right
    const double st = (double)step;
    const double beta2_t = __builtin_pow(beta2, st);
    const double n_max = 2.0 / (1.0 - beta2) - 1.0;
    const double n_sma = n_max - 2.0 * st * beta2_t / (1.0 - beta2_t);
    const double bc1 = 1.0 - __builtin_pow(beta1, st);
    double step_size = 0.0;
    if (mode == kRectified) {
        const double r = (1.0 - beta2_t) * (n_sma - 4.0) / (n_max - 4.0) * (n_sma - 2.0) / n_sma
                         * n_max / (n_max - 2.0);
        NR_REQUIRE(r > 0.0, "nr_radam_step: rectified mode at step %lld where N_sma = %g <= 4",
                   (long long)step, n_sma);
        step_size = __builtin_sqrt(r) / bc1;
    } else if (mode == kSgdLike) {
        step_size = 1.0 / bc1;
    }
    if (count == 0) return 0;
    NR_REQUIRE(params && grads && exp_avg && exp_avg_sq && numel, "nr_radam_step: null table");
    NR_REQUIRE(!lookahead_sync || slow, "nr_radam_step: lookahead_sync with a null slow table");
    RAdamArgs a{};
    a.start[0] = 0;
    for (int k = 0; k < count; ++k) {
        NR_REQUIRE(numel[k] >= 0 && numel[k] < kMaxNumel, "nr_radam_step: bad numel[%d]", k);
        if (numel[k] > 0)
            NR_REQUIRE(params[k] && grads[k] && exp_avg[k] && exp_avg_sq[k]
                           && (!lookahead_sync || slow[k]),
                       "nr_radam_step: null pointer in the table (tensor %d)", k);
        a.p[k] = params[k]; a.g[k] = grads[k]; a.m[k] = exp_avg[k]; a.v[k] = exp_avg_sq[k];
        a.slow[k] = lookahead_sync ? slow[k] : nullptr;
        a.start[k + 1] = a.start[k] + (numel[k] + 3) / 4;
        a.tail[k] = (uint8_t)(numel[k] == 0 ? 0 : numel[k] - ((numel[k] + 3) / 4 - 1) * 4);
        if (aligned16(a.p[k]) && aligned16(a.g[k]) && aligned16(a.m[k]) && aligned16(a.v[k])
            && aligned16(a.slow[k]))
            a.aligned |= (uint64_t)1 << k;
    }
    a.count = count;
    a.mode = mode;
    a.has_decay = weight_decay != 0.0;
    a.sync = lookahead_sync;
    // scalars as torch forms them: python doubles, rounded to fp32 when applied
    a.beta1 = (float)beta1; a.w1 = (float)(1.0 - beta1);
    a.beta2 = (float)beta2; a.w2 = (float)(1.0 - beta2);
    a.eps = (float)eps;
    a.decay = (float)(-weight_decay * lr);
    a.neg_step = (float)(-step_size * lr);
    a.alpha = (float)lookahead_alpha;
    const int64_t total = a.start[count];
    if (total == 0) return 0;
    radam_kernel<<<grid_of(total), 256, 0, (hipStream_t)stream>>>(a);
    NR_LAUNCH_CHECK("nr_radam_step");
    return 0;
}
