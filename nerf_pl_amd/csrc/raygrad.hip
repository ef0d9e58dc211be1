// Gradients with respect to the rays (include/nerf_pl_amd_raygrad.h, DESIGN.md
// 18): the reference's render_rays is plain PyTorch and differentiates in its
// (N, 8) ray tensor; these kernels carry that gradient through the four stages
// of the fused path -- MLP input, compositing, merge, stratified depths.  None
// of the tuned kernels changes: everything here runs only when the rays
// require grad.
#include "layout.h"

namespace {

template <typename T>
__device__ __forceinline__ T rg_wave_sum(T v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__device__ __forceinline__ double rg_wave_incl_prod(double v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_up(v, d);
        if (lane >= d) v *= o;
    }
    return v;
}

// suffix scan of affine maps R -> a R + b (render.hip wave_suffix_affine)
__device__ __forceinline__ void rg_suffix_affine(double& a, double& b, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double na = __shfl_down(a, d);
        const double nb = __shfl_down(b, d);
        if (lane + d < 64) {
            b = fma(a, nb, b);
            a = a * na;
        }
    }
}

// ---------------------------------------------------------------------------
// flat fp32 parameters (NeRF.named_parameters order, models/nerf.py:41-81)
// ---------------------------------------------------------------------------
constexpr int kLayer(int fan) { return 256 * fan + 256; }
constexpr int kW1 = 0;                                       // xyz_encoding_1.0.weight (256, 63)
constexpr int kW5 = kLayer(63) + 3 * kLayer(256);            // xyz_encoding_5.0.weight (256, 319)
constexpr int kWFinal = kW5 + kLayer(319) + 3 * kLayer(256); // xyz_encoding_final.weight
constexpr int kWDir = kWFinal + kLayer(256);                 // dir_encoding.0.weight (128, 283)

// ---------------------------------------------------------------------------
// Stage 1: the MLP's input gradient.
//   g_e  = W1^T dz1 + W5[:, 0:63]^T dz5        (63 embedded position channels)
//   g_de = W_dir[:, 256:283]^T dz_dir          (27 embedded direction channels)
// One wave per kNB = 2 blocks of 32 positions (a weight fragment is loaded once
// for both: 1.76 -> 1.09 ms per fine launch), on the fp32 MFMA
// (32 channels x 32 samples per tile, k-steps of 2): the B operand of lane
// (h, j) is feature 8c + 4h + e of position j, which every gradient layout
// holds as one float4 per lane and chunk c of 8 features:
//   layout 0  block-native (layout.h):  [c][lane][4]
//   layout 1  N16 (x3.h):               [F = c/2][S = j/16][16 (2 (c&1) + h) + j%16][4]
//   layout 2  N16 in bf16 (x3.h NR_BF1): the same float4 as four bf16 at slot
//             bf16_slot, blocks at half the fp32 stride
// The A operand is the weight column read from the flat fp32 parameters.
// The accumulators pass through LDS ([channel][sample]) so that every lane
// then walks the encoding chain of its own sample:
//   g_x[a] = g_e[a] + sum_k 2^k (cos(2^k x_a) g_e[3+6k+a] - sin(2^k x_a) g_e[6+6k+a])
// (lane half h takes frequencies 5h .. 5h+4; the halves are added once), with
// x = o + d z formed in fp32, multiply then add, as the forward forms it.
// Per sample it leaves [g_x (3), g_z = d . g_x, g_dd (3), 0]: g_dd is the
// same chain through the direction embedding at d (nerf.py:33-38 is linear
// in the channel gradients, so summing per sample and per ray commute).
// ---------------------------------------------------------------------------
struct MlpArgs {
    const float* params; const float* grad; const float* rays; const float* z;
    int n, spr, n_rays, layout, sigma_only;
    const int32_t* slist; const int32_t* scount;
    float* out;      // (n, 8)
};

__device__ __forceinline__ int64_t rg_bf16_slot(int64_t idx) {
    return (idx & ~(int64_t)63) | (4 * (idx & 15) + ((idx >> 4) & 3));
}

// the lane's four values of chunk c of a width-W segment's block
template <int W>
__device__ __forceinline__ f32x4 rg_chunk(const float* __restrict__ seg, int layout, int blk,
                                          int c, int lane) {
    if (layout == 0)
        return *reinterpret_cast<const f32x4*>(seg + (size_t)blk * NR_NATIVE(W) + (c * 64 + lane) * 4);
    const int h = lane >> 5, j = lane & 31;
    const int idx = ((c >> 1) * 2 + (j >> 4)) * 64 + 16 * (2 * (c & 1) + h) + (j & 15);
    if (layout == 1)
        return *reinterpret_cast<const f32x4*>(seg + (size_t)blk * NR_NATIVE(W) + idx * 4);
    const uint2 u = *(reinterpret_cast<const uint2*>(seg + (size_t)blk * (NR_NATIVE(W) / 2)) +
                      rg_bf16_slot(idx));
    return f32x4{__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u),
                 __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u)};
}

// acc[b][t] += W[:, col0 + 32t + i]^T dz over a width-W segment (fan: W's row
// length) for the wave's kNB blocks blk0 .. blk0 + kNB - 1: every weight
// fragment is loaded once and used by each block
constexpr int kNB = 2;
template <int W, int NT>
__device__ __forceinline__ void rg_gemm(const float* __restrict__ w, int fan, int col0, int ncol,
                                        const float* __restrict__ seg, int layout, int blk0,
                                        int lane, const bool (&valid)[kNB],
                                        f32x16 (&acc)[kNB][NT]) {
    const int h = lane >> 5, i = lane & 31;
#pragma unroll 2
    for (int c = 0; c < W / 8; ++c) {
        f32x4 v[kNB];
#pragma unroll
        for (int b = 0; b < kNB; ++b) {
            v[b] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (valid[b]) v[b] = rg_chunk<W>(seg, layout, blk0 + b, c, lane);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float* row = w + (size_t)(8 * c + 4 * h + e) * fan + col0;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float a = 32 * t + i < ncol ? row[32 * t + i] : 0.f;
#pragma unroll
                for (int b = 0; b < kNB; ++b) acc[b][t] = nr_mfma32(a, v[b][e], acc[b][t]);
            }
        }
    }
}

// one axis of the encoding chain over frequencies k0 .. k0 + nk - 1: g[] are
// the channel gradients of one sample at LDS stride 32 (channel c at g[32 c])
__device__ __forceinline__ float rg_chain(const float* g, float x, int a, int k0, int nk) {
    float s = 0.f;
    for (int k = k0; k < k0 + nk; ++k) {
        const float f = (float)(1 << k);
        float sn, cs;
        sincosf(f * x, &sn, &cs);
        const float t = cs * g[32 * (3 + 6 * k + a)] - sn * g[32 * (6 + 6 * k + a)];
        s += f * t;
    }
    return s;
}

constexpr int kRgRows = 96;      // 64 position channels (63 + pad), 32 direction channels (27 + pad)

// the chain of the lane's own sample q (position) from the block's channel
// gradients in LDS; both lane halves of a sample take the same branches
__device__ __forceinline__ void rg_sample(const MlpArgs& a, const float* ge, int64_t q, int h) {
    const int s = a.slist ? a.slist[q] : (int)q;
    if (s < 0 || s >= a.n) return;
    const int ray = s / a.spr;
    if (ray >= a.n_rays) return;
    const float* r = a.rays + (size_t)ray * 8;
    const float zs = a.z[s];
    float gx[3], gd[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const float x = nr_add(r[ax], nr_mul(r[3 + ax], zs));
        float px = rg_chain(ge, x, ax, 5 * h, 5);
        if (h == 0) px += ge[32 * ax];
        gx[ax] = px + __shfl_xor(px, 32);
        float pd = 0.f;
        if (!a.sigma_only) {
            pd = rg_chain(ge + 64 * 32, r[3 + ax], ax, 2 * h, 2);
            if (h == 0) pd += ge[32 * (64 + ax)];
        }
        gd[ax] = pd + __shfl_xor(pd, 32);
    }
    f32x4 o;
    if (h == 0) {
        const float gz = fmaf(r[5], gx[2], fmaf(r[4], gx[1], r[3] * gx[0]));
        o = f32x4{gx[0], gx[1], gx[2], gz};
    } else {
        o = f32x4{gd[0], gd[1], gd[2], 0.f};
    }
    *reinterpret_cast<f32x4*>(a.out + (size_t)s * 8 + 4 * h) = o;
}

__global__ void __launch_bounds__(256) raygrad_mlp_kernel(MlpArgs a) {
    __shared__ float lds[4][kRgRows * 32];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int h = lane >> 5, j = lane & 31;
    const int blk0 = (blockIdx.x * 4 + wave) * kNB;
    const int nb = (int)nr_blocks_pad(a.n);
    const int m = a.scount ? min(max(__builtin_amdgcn_readfirstlane(*a.scount), 0), a.n) : a.n;
    bool valid[kNB];
#pragma unroll
    for (int b = 0; b < kNB; ++b) valid[b] = (int64_t)(blk0 + b) * 32 + j < m;    // position < count
    float* g = lds[wave];
    f32x16 acc[kNB][2] = {};
    f32x16 accd[kNB][1] = {};
    if ((int64_t)blk0 * 32 < m) {
        rg_gemm<256, 2>(a.params + kW1, 63, 0, 63, a.grad + nr_gd_dz(0, nb), a.layout, blk0, lane,
                        valid, acc);
        rg_gemm<256, 2>(a.params + kW5, 319, 0, 63, a.grad + nr_gd_dz(4, nb), a.layout, blk0, lane,
                        valid, acc);
        if (!a.sigma_only)
            rg_gemm<128, 1>(a.params + kWDir, 283, 256, 27, a.grad + nr_gd_dzdir(nb), a.layout,
                            blk0, lane, valid, accd);
    }
    // one block at a time through the wave's LDS tile ([channel][sample]); every
    // wave of the workgroup takes every barrier
#pragma unroll
    for (int b = 0; b < kNB; ++b) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) g[(32 * t + nr_acc_row(r, h)) * 32 + j] = acc[b][t][r];
#pragma unroll
        for (int r = 0; r < 16; ++r) g[(64 + nr_acc_row(r, h)) * 32 + j] = accd[b][0][r];
        __syncthreads();
        if (valid[b]) rg_sample(a, g + j, (int64_t)(blk0 + b) * 32 + j, h);
        __syncthreads();
    }
}

// Per ray, over its samples in index order (lane l takes samples l, l + 64,
// ...; the 64 partial sums meet in a fixed butterfly), in double:
//   g_o = sum g_x,  g_d = sum z g_x + sum g_dd;  columns 6, 7 are zero
__global__ void raygrad_reduce_kernel(const float* __restrict__ gs, const float* __restrict__ z,
                                      int n_rays, int S, float* __restrict__ g_rays) {
    const int lane = threadIdx.x & 63;
    const int ray = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (ray >= n_rays) return;
    const int64_t base = (int64_t)ray * S;
    double so[3] = {0.0, 0.0, 0.0}, sd[3] = {0.0, 0.0, 0.0};
    for (int i = lane; i < S; i += 64) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(gs + (base + i) * 8);
        const f32x4 d = *reinterpret_cast<const f32x4*>(gs + (base + i) * 8 + 4);
        const double zi = z[base + i];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            so[ax] += (double)x[ax];
            sd[ax] += zi * (double)x[ax] + (double)d[ax];
        }
    }
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        so[ax] = rg_wave_sum(so[ax]);
        sd[ax] = rg_wave_sum(sd[ax]);
    }
    if (lane == 0) {
        float* o = g_rays + (size_t)ray * 8;
        *reinterpret_cast<f32x4*>(o) = f32x4{(float)so[0], (float)so[1], (float)so[2], (float)sd[0]};
        *reinterpret_cast<f32x4*>(o + 4) = f32x4{(float)sd[1], (float)sd[2], 0.f, 0.f};
    }
}

// ---------------------------------------------------------------------------
// Stage 2: compositing (rendering.py:169-198) in the depths and |d|.
// composite_bwd_kernel's recurrences (render.hip), in double from the same
// fp32 inputs: da_i = T_i (dw_i - R_i); alpha_i = 1 - exp(-delta_i r_i), so
//   g_delta_i = da_i r_i exp(-delta_i r_i),        r_i = relu(sigma_i + noise_i)
// delta_i = (z_{i+1} - z_i) |d|, delta_last = 1e10 |d|:
//   g_z[i] = w_i (g_depth - gq O) + |d| (g_delta_{i-1} - [i < S-1] g_delta_i)
//   g_|d|  = sum_{i<S-1} g_delta_i (z_{i+1} - z_i) + 1e10 g_delta_{S-1}
//   g_d    = g_|d| d / |d|
// (gq, O: the disparity's terms, as in composite_bwd_kernel).
// ---------------------------------------------------------------------------
struct CompRayArgs {
    const float* raw; int raw_stride; int sig_col; const float* z; const float* rays; const float* noise;
    float noise_std; uint64_t seed; uint32_t stream;
    int n_rays, S, white_back;
    const float* g_rgb; const float* g_depth; const float* g_opacity;
    const float* g_disp; const float* depth; const float* opacity;
    float* g_z;      // (n_rays, S)
    float* g_rays;   // (n_rays, 8): columns 3..5, zeros elsewhere
};

__device__ __forceinline__ float rg_noise(const float* noise, float noise_std, uint64_t seed,
                                          uint32_t stream, int64_t idx) {
    if (noise) return nr_mul(noise[idx], noise_std);
    if (noise_std == 0.f) return 0.f;
    return nr_mul(nr_rand_normal(seed, stream, (uint64_t)idx), noise_std);
}

__device__ __forceinline__ double rg_delta(const float* z, int64_t base, int i, int S, double dn) {
    if (i + 1 < S) return ((double)z[base + i + 1] - (double)z[base + i]) * dn;
    return S > 1 ? 1e10 * dn : 0.0;
}

__global__ void composite_raygrad_kernel(CompRayArgs a) {
    const int lane = threadIdx.x & 63;
    const int ray = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (ray >= a.n_rays) return;
    const float* r = a.rays + (size_t)ray * 8;
    const double dn = sqrt((double)r[3] * r[3] + (double)r[4] * r[4] + (double)r[5] * r[5]);
    const int S = a.S;
    const int64_t base = (int64_t)ray * S;
    const float gr = a.g_rgb ? a.g_rgb[(size_t)ray * 3 + 0] : 0.f;
    const float gg = a.g_rgb ? a.g_rgb[(size_t)ray * 3 + 1] : 0.f;
    const float gb = a.g_rgb ? a.g_rgb[(size_t)ray * 3 + 2] : 0.f;
    const float gd = a.g_depth ? a.g_depth[ray] : 0.f;
    double go = a.g_opacity ? a.g_opacity[ray] : 0.f;
    bool has_q = false;
    double gq = 0.0, Dq = 0.0, Oq = 0.0;
    if (a.g_disp) {
        const float D = a.depth[ray], O = a.opacity[ray];
        if (D / O > 1e-10f) {
            has_q = true;
            Dq = D; Oq = O;
            gq = (double)a.g_disp[ray] / (Dq * Dq);
        }
    }
    if (a.white_back) go -= (double)gr + (double)gg + (double)gb;
    const double gdz = (double)gd - (has_q ? gq * Oq : 0.0);      // d loss / d depth, direct
    const int nchunks = (S + 63) >> 6;
    auto rel = [&](int i) {
        return nr_add(a.raw[(base + i) * a.raw_stride + a.sig_col],
                      rg_noise(a.noise, a.noise_std, a.seed, a.stream, base + i));
    };
    double Rcarry = 0.0;
    double g_dn = 0.0;
    double pend = 0.0;       // lane 0: its sample's g_z but for g_delta of the sample before it
    for (int ci = nchunks - 1; ci >= 0; --ci) {
        const int c0 = ci * 64;
        double carry = 1.0;
        for (int cj = 0; cj < ci; ++cj) {
            const int jj = cj * 64 + lane;
            double fac = 1.0;
            if (jj < S) {
                const float s = rel(jj);
                fac = exp(-rg_delta(a.z, base, jj, S, dn) * (s > 0.f ? (double)s : 0.0)) + 1e-10;
            }
            carry *= __shfl(rg_wave_incl_prod(fac, lane), 63);
        }
        const int i = c0 + lane;
        const bool v = i < S;
        double alpha = 0.0, e = 1.0, delta = 0.0;
        float srel = 0.f, cr = 0.f, cg = 0.f, cb = 0.f, zi = 0.f;
        if (v) {
            zi = a.z[base + i];
            delta = rg_delta(a.z, base, i, S, dn);
            const float* rr = a.raw + (base + i) * a.raw_stride;
            if (a.raw_stride == 4) { cr = rr[0]; cg = rr[1]; cb = rr[2]; }
            srel = rel(i);
            e = exp(-delta * (srel > 0.f ? (double)srel : 0.0));
            alpha = 1.0 - e;
        }
        const double fac = v ? e + 1e-10 : 1.0;
        const double incl = rg_wave_incl_prod(fac, lane);
        double excl = __shfl_up(incl, 1);
        if (lane == 0) excl = 1.0;
        const double T = carry * excl;
        double dw = 0.0;
        if (v) {
            dw = (double)gr * cr + (double)gg * cg + (double)gb * cb + (double)gd * zi + go;
            if (has_q) dw += gq * (Dq - Oq * (double)zi);
        }
        double A = fac, Bv = v ? dw * alpha : 0.0;
        rg_suffix_affine(A, Bv, lane);
        double An = __shfl_down(A, 1), Bn = __shfl_down(Bv, 1);
        if (lane == 63) { An = 1.0; Bn = 0.0; }
        const double Ri = fma(An, Rcarry, Bn);
        const double Rnext = fma(__shfl(A, 0), Rcarry, __shfl(Bv, 0));
        // g_delta_i, and its two uses
        const double gdel = (v && srel > 0.f) ? T * (dw - Ri) * (double)srel * e : 0.0;
        if (v) g_dn += gdel * (i + 1 < S ? (double)a.z[base + i + 1] - (double)zi
                                         : (S > 1 ? 1e10 : 0.0));
        double prev = __shfl_up(gdel, 1);
        if (lane == 0) prev = 0.0;
        const double own = v ? alpha * T * gdz - (i + 1 < S ? dn * gdel : 0.0) : 0.0;
        if (v && (lane > 0 || ci == 0)) a.g_z[base + i] = (float)(own + dn * prev);
        // the first sample of the chunk after this one waited for this chunk's last g_delta
        const double lastg = __shfl(gdel, 63);
        if (lane == 0 && ci + 1 < nchunks) a.g_z[base + c0 + 64] = (float)(pend + dn * lastg);
        pend = own;
        Rcarry = Rnext;
    }
    g_dn = rg_wave_sum(g_dn);
    if (lane == 0) {
        float* o = a.g_rays + (size_t)ray * 8;
        const double k = dn > 0.0 ? g_dn / dn : 0.0;
        *reinterpret_cast<f32x4*>(o) = f32x4{0.f, 0.f, 0.f, (float)(k * r[3])};
        *reinterpret_cast<f32x4*>(o + 4) = f32x4{(float)(k * r[4]), (float)(k * r[5]), 0.f, 0.f};
    }
}

// ---------------------------------------------------------------------------
// Stage 3: z_fine = sort(cat[z_coarse, z_pdf.detach()]) (rendering.py:257):
// g_zcoarse[i] = g_zfine[pos(i)].  nr_sample_pdf places coarse depth i before
// every importance depth that is not smaller, and equal coarse depths in
// index order, so pos(i) = #{z_fine < c_i} + #{k < i: c_k == c_i} -- the
// position a walk along the two sorted rows that matches equal bit patterns
// in order finds.  (Where a coarse and an importance depth tie, the forward
// is the same either way and the reference's unstable sort attributes the
// gradient arbitrarily; this rule is the coarse-first one.)
// ---------------------------------------------------------------------------
__global__ void merge_raygrad_kernel(const float* __restrict__ zc, const float* __restrict__ zf,
                                     const float* __restrict__ g_zf, int64_t n_rays, int S, int SF,
                                     float* __restrict__ g_zc) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_rays * S) return;
    const int64_t ray = t / S;
    const int i = (int)(t % S);
    const float* c = zc + ray * S;
    const float* f = zf + ray * SF;
    const float v = c[i];
    int lo = 0, hi = SF;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (f[mid] < v) lo = mid + 1; else hi = mid;
    }
    for (int k = 0; k < i; ++k) lo += c[k] == v;
    // a row that is not the merge of this coarse row (or holds a NaN) matches nothing
    g_zc[t] = (lo < SF && f[lo] == v) ? g_zf[ray * SF + lo] : 0.f;
}

// ---------------------------------------------------------------------------
// Stage 4: stratified depths (rendering.py:216-232) in near and far.
//   zb_k = near (1 - t_k) + far t_k,  or 1 / ((1 - t_k) / near + t_k / far)
//   z_k  = lower_k + (upper_k - lower_k) p u_k   (perturb p > 0), mids of zb
// linear in zb: g_zb gathers from z_{k-1}, z_k, z_{k+1}; then per ray, in
// double, g_near = sum g_zb dzb/dnear, g_far = sum g_zb dzb/dfar.
// ---------------------------------------------------------------------------
__global__ void coarse_z_raygrad_kernel(const float* __restrict__ rays, const float* __restrict__ tlin,
                                        int n_rays, int S, int use_disp, float perturb,
                                        const float* __restrict__ u, uint64_t seed,
                                        const float* __restrict__ g_z, float* __restrict__ g_rays) {
    const int lane = threadIdx.x & 63;
    const int ray = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (ray >= n_rays) return;
    const int64_t base = (int64_t)ray * S;
    const double near = rays[(size_t)ray * 8 + 6], far = rays[(size_t)ray * 8 + 7];
    // (g_lower, g_upper) of sample k
    auto lu = [&](int k, double& gl, double& gu) {
        const double g = g_z[base + k];
        if (!(perturb > 0.f)) { gl = g; gu = 0.0; return; }
        const float r = u ? u[base + k] : nr_rand_uniform(seed, 0, (uint64_t)(base + k));
        const double pu = (double)nr_mul(perturb, r);
        gl = g * (1.0 - pu);
        gu = g * pu;
    };
    double gn = 0.0, gf = 0.0;
    for (int k = lane; k < S; k += 64) {
        double gl, gu, gzb;
        lu(k, gl, gu);
        if (!(perturb > 0.f)) {
            gzb = gl;
        } else {
            gzb = (k > 0 ? 0.5 * gl : gl) + (k < S - 1 ? 0.5 * gu : gu);
            if (k < S - 1) { double l1, u1; lu(k + 1, l1, u1); gzb += 0.5 * l1; }
            if (k > 0) { double l0, u0; lu(k - 1, l0, u0); gzb += 0.5 * u0; }
        }
        const double t = tlin[k];
        if (!use_disp) {
            gn += gzb * (1.0 - t);
            gf += gzb * t;
        } else {
            const double zb = 1.0 / ((1.0 - t) / near + t / far);
            gn += gzb * zb * zb * (1.0 - t) / (near * near);
            gf += gzb * zb * zb * t / (far * far);
        }
    }
    gn = rg_wave_sum(gn);
    gf = rg_wave_sum(gf);
    if (lane == 0) {
        float* o = g_rays + (size_t)ray * 8;
        *reinterpret_cast<f32x4*>(o) = f32x4{0.f, 0.f, 0.f, 0.f};
        *reinterpret_cast<f32x4*>(o + 4) = f32x4{0.f, 0.f, (float)gn, (float)gf};
    }
}

constexpr int64_t kMaxN = (int64_t)1 << 31;
inline bool rg_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

NR_API int nr_raygrad_mlp(const float* params, const float* grad_ws, const float* rays,
                          const float* z, int64_t n, int samples_per_ray, int64_t n_rays,
                          int layout, int sigma_only, const int32_t* samples,
                          const int32_t* count, float* g_samples, void* stream) {
    NR_REQUIRE(n >= 0 && n < kMaxN && n_rays >= 0 && n_rays < kMaxN, "nr_raygrad_mlp: size out of range");
    NR_REQUIRE(samples_per_ray > 0 && n_rays * (int64_t)samples_per_ray == n,
               "nr_raygrad_mlp: n must be n_rays * samples_per_ray");
    NR_REQUIRE(layout >= 0 && layout <= 2, "nr_raygrad_mlp: layout must be 0 (native), 1 (N16) or 2 (N16 bf16)");
    NR_REQUIRE((samples == nullptr) == (count == nullptr),
               "nr_raygrad_mlp: samples and count go together");
    if (n == 0) return 0;
    NR_REQUIRE(params && grad_ws && rays && z && g_samples, "nr_raygrad_mlp: null pointer");
    NR_REQUIRE(rg_aligned16(grad_ws) && rg_aligned16(g_samples) && ((uintptr_t)params & 3) == 0,
               "nr_raygrad_mlp: grad_ws and g_samples must be 16-byte aligned");
    MlpArgs a{params, grad_ws, rays, z, (int)n, samples_per_ray, (int)n_rays, layout, sigma_only,
              samples, count, g_samples};
    const int64_t blocks = (n + 128 * kNB - 1) / (128 * kNB);
    raygrad_mlp_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(a);
    NR_LAUNCH_CHECK("nr_raygrad_mlp");
    return 0;
}

NR_API int nr_raygrad_reduce(const float* g_samples, const float* z, int64_t n_rays,
                             int samples_per_ray, float* g_rays, void* stream) {
    NR_REQUIRE(n_rays >= 0 && n_rays < kMaxN && samples_per_ray > 0 && n_rays * (int64_t)samples_per_ray < kMaxN,
               "nr_raygrad_reduce: bad sizes");
    if (n_rays == 0) return 0;
    NR_REQUIRE(g_samples && z && g_rays, "nr_raygrad_reduce: null pointer");
    NR_REQUIRE(rg_aligned16(g_samples) && rg_aligned16(g_rays),
               "nr_raygrad_reduce: g_samples and g_rays must be 16-byte aligned");
    raygrad_reduce_kernel<<<(unsigned)((n_rays + 3) / 4), 256, 0, (hipStream_t)stream>>>(
        g_samples, z, (int)n_rays, samples_per_ray, g_rays);
    NR_LAUNCH_CHECK("nr_raygrad_reduce");
    return 0;
}

NR_API int nr_composite_raygrad(const float* raw, int raw_stride, int sig_col, const float* z,
                                const float* rays, const float* noise, float noise_std,
                                uint64_t seed, int rng_stream, int64_t n_rays, int n_samples,
                                int white_back, const float* g_rgb, const float* g_depth,
                                const float* g_opacity, const float* g_disp, const float* depth,
                                const float* opacity, float* g_z, float* g_rays, void* stream) {
    NR_REQUIRE(n_rays >= 0 && n_rays < kMaxN && n_samples > 0 && n_rays * (int64_t)n_samples < kMaxN,
               "nr_composite_raygrad: bad sizes");
    if (n_rays == 0) return 0;
    NR_REQUIRE(raw && z && rays && g_z && g_rays, "nr_composite_raygrad: null pointer");
    NR_REQUIRE(!g_disp || (depth && opacity),
               "nr_composite_raygrad: g_disp needs the forward's depth and opacity");
    NR_REQUIRE(raw_stride == 4 ? sig_col == 3 : (raw_stride == 1 && sig_col == 0),
               "nr_composite_raygrad: raw rows must be [rgb, sigma] or [sigma]");
    NR_REQUIRE(rg_aligned16(g_rays), "nr_composite_raygrad: g_rays must be 16-byte aligned");
    CompRayArgs a{raw, raw_stride, sig_col, z, rays, noise, noise_std, seed, (uint32_t)rng_stream,
                  (int)n_rays, n_samples, white_back, g_rgb, g_depth, g_opacity, g_disp, depth,
                  opacity, g_z, g_rays};
    composite_raygrad_kernel<<<(unsigned)((n_rays + 3) / 4), 256, 0, (hipStream_t)stream>>>(a);
    NR_LAUNCH_CHECK("nr_composite_raygrad");
    return 0;
}

NR_API int nr_merge_raygrad(const float* z_coarse, const float* z_fine, const float* g_zfine,
                            int64_t n_rays, int n_samples, int n_importance, float* g_zcoarse,
                            void* stream) {
    NR_REQUIRE(n_rays >= 0 && n_rays < kMaxN && n_samples > 0 && n_importance >= 0 &&
                   n_rays * ((int64_t)n_samples + n_importance) < kMaxN,
               "nr_merge_raygrad: bad sizes");
    if (n_rays == 0) return 0;
    NR_REQUIRE(z_coarse && z_fine && g_zfine && g_zcoarse, "nr_merge_raygrad: null pointer");
    const int64_t n = n_rays * n_samples;
    merge_raygrad_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(
        z_coarse, z_fine, g_zfine, n_rays, n_samples, n_samples + n_importance, g_zcoarse);
    NR_LAUNCH_CHECK("nr_merge_raygrad");
    return 0;
}

NR_API int nr_coarse_z_raygrad(const float* rays, const float* tlin, int64_t n_rays, int n_samples,
                               int use_disp, float perturb, const float* u, uint64_t seed,
                               const float* g_z, float* g_rays, void* stream) {
    NR_REQUIRE(n_rays >= 0 && n_rays < kMaxN && n_samples > 0 && n_rays * (int64_t)n_samples < kMaxN,
               "nr_coarse_z_raygrad: bad sizes");
    if (n_rays == 0) return 0;
    NR_REQUIRE(rays && tlin && g_z && g_rays, "nr_coarse_z_raygrad: null pointer");
    NR_REQUIRE(rg_aligned16(g_rays), "nr_coarse_z_raygrad: g_rays must be 16-byte aligned");
    coarse_z_raygrad_kernel<<<(unsigned)((n_rays + 3) / 4), 256, 0, (hipStream_t)stream>>>(
        rays, tlin, (int)n_rays, n_samples, use_disp, perturb, u, seed, g_z, g_rays);
    NR_LAUNCH_CHECK("nr_coarse_z_raygrad");
    return 0;
}
