// Self-checks exported through the C ABI: layout constants (callable without a
// GPU), an MFMA lane-map probe (tests/test_gpu_kernels.py) and a probe of the
// in-kernel Philox draws (tests/test_gpu_philox.py).
#include "layout.h"

NR_API int64_t nr_layout_query(int what) {
    switch (what) {
        case 0: return NR_F_TOTAL;
        case 1: return NR_F_HEAD;
        case 2: return NR_B_TOTAL;
        case 3: return NR_SAVE_PER_BLOCK;
        case 4: return NR_GRAD_PER_BLOCK;
        case 5: return NR_H_SIZE;
        case 6: return NR_F_L5;
        case 7: return NR_F_DIR;
        case 8: return NR_B_L5T;
        // ABI revision: 2 = a full-graph nr_wgrad* launch leaves G = sum dz_dir h8^T
        // in dir_encoding.0.weight[:, :256] and zeros in xyz_encoding_final, and
        // nr_wgrad_dir_feat must follow it (round 5; 1 = every gradient final)
        case 9: return 2;
        default: return -1;
    }
}

namespace {
// D = A(32x2) * B(2x32) with A[i][k] = a_in[i*2+k], B[k][j] = b_in[k*32+j];
// writes D[row][col] = d_out[row*32+col] using the documented C/D lane map.
__global__ void probe_mfma_kernel(const float* a_in, const float* b_in, float* d_out) {
    const int l = threadIdx.x;
    const float a = a_in[(l & 31) * 2 + (l >> 5)];
    const float b = b_in[(l >> 5) * 32 + (l & 31)];
    f32x16 c = {};
    c = nr_mfma32(a, b, c);
    for (int r = 0; r < 16; ++r) d_out[nr_acc_row(r, l >> 5) * 32 + (l & 31)] = c[r];
}

// The in-kernel draws themselves (common.h), element i at counter idx0 + i:
// what coarse_z / composite / sample_pdf draw when their replay pointers are
// null (tests/test_gpu_philox.py)
__global__ void probe_rand_kernel(uint64_t seed, uint32_t stream, uint64_t idx0, int64_t n,
                                  float* __restrict__ uniform_out,
                                  float* __restrict__ normal_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (uniform_out) uniform_out[i] = nr_rand_uniform(seed, stream, idx0 + (uint64_t)i);
    if (normal_out) normal_out[i] = nr_rand_normal(seed, stream, idx0 + (uint64_t)i);
}
}  // namespace

NR_API int nr_probe_rand(uint64_t seed, int stream, uint64_t idx0, int64_t n, float* uniform_out,
                         float* normal_out, void* stream_) {
    NR_REQUIRE(n >= 0 && n <= ((int64_t)1 << 31), "nr_probe_rand: bad size");
    if (n == 0 || (!uniform_out && !normal_out)) return 0;
    probe_rand_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream_>>>(
        seed, (uint32_t)stream, idx0, n, uniform_out, normal_out);
    NR_LAUNCH_CHECK("nr_probe_rand");
    return 0;
}

NR_API int nr_probe_mfma32(const float* a, const float* b, float* d, void* stream) {
    probe_mfma_kernel<<<1, 64, 0, (hipStream_t)stream>>>(a, b, d);
    NR_LAUNCH_CHECK("nr_probe_mfma32");
    return 0;
}
