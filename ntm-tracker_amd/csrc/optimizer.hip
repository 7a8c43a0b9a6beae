// The optimiser of the training step:
//   * clip_by_global_norm + TF RMSProp                    (direct_offset_output.py:620-626)
// The global norm is a two-kernel sum of squares in a fixed order; the update is HBM-bound elementwise work.
#include "common.h"

namespace {

// sum of squares: one workgroup of SUMSQ_BLOCK threads per SUMSQ_PER_BLOCK elements, then one workgroup over the partial sums
constexpr int SUMSQ_BLOCK = 256;
constexpr int SUMSQ_PER_BLOCK = 4096;

__global__ void sumsq_partial_kernel(const float* __restrict__ g, float* __restrict__ partial, size_t n) {
    __shared__ float red[SUMSQ_BLOCK / 64];
    const size_t base = (size_t)blockIdx.x * SUMSQ_PER_BLOCK;
    float acc = 0.f;
    for (int i = threadIdx.x; i < SUMSQ_PER_BLOCK; i += SUMSQ_BLOCK) {
        const size_t idx = base + i;
        if (idx < n) { const float v = g[idx]; acc += v * v; }
    }
    const float s = block_sum<SUMSQ_BLOCK / 64>(wave_sum(acc), red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ void sumsq_final_kernel(const float* __restrict__ partial, int nblocks, float* __restrict__ gnorm) {
    __shared__ float red[16];
    float acc = 0.f;
    for (int i = threadIdx.x; i < nblocks; i += blockDim.x) acc += partial[i];
    const float s = block_sum(wave_sum(acc), red);
    if (threadIdx.x == 0) *gnorm = sqrtf(s);
}

// tf.train.RMSPropOptimizer on element i, its gradient times scale (ms slot starts at ONE, eps inside the sqrt)
__device__ __forceinline__ void rmsprop_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ ms,
                                               float* __restrict__ mom, size_t i, float scale, float lr, float decay,
                                               float momentum, float eps) {
    const float gi = g[i] * scale;
    const float m2 = decay * ms[i] + (1.0f - decay) * gi * gi;
    const float mo = momentum * mom[i] + lr * gi / sqrtf(m2 + eps);
    ms[i] = m2;
    mom[i] = mo;
    p[i] -= mo;
}

// tf.clip_by_global_norm then the update
__global__ void rmsprop_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ ms,
                               float* __restrict__ mom, size_t n, float lr, float decay, float momentum,
                               float eps, float clip, const float* __restrict__ gnorm) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float scale = 1.0f;
    if (clip > 0.f) scale = clip / fmaxf(*gnorm, clip);
    rmsprop_update(p, g, ms, mom, i, scale, lr, decay, momentum, eps);
}

// The same update behind a finiteness check of the global norm (every thread reads the same word, so the whole grid takes
// the same branch): a NaN / Inf norm -- an aborted cluster launch poisons the gradient, csrc/dnc_cluster_fwd.hip, or a
// genuine overflow -- leaves parameters and slots untouched, turns *loss into NaN and counts the skipped step.
__global__ void rmsprop_checked_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ ms,
                                       float* __restrict__ mom, size_t n, float lr, float decay, float momentum,
                                       float eps, float clip, const float* __restrict__ gnorm, float* __restrict__ loss,
                                       unsigned* __restrict__ skipped) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const float gn = *gnorm;
    if (!(fabsf(gn) <= 3.402823466e38f)) {                    // NaN or Inf
        if (i == 0) {
            if (loss) loss[0] = __int_as_float(0x7fc00000);
            if (skipped) *skipped += 1u;
        }
        return;
    }
    if (i >= n) return;
    float scale = 1.0f;
    if (clip > 0.f) scale = clip / fmaxf(gn, clip);
    rmsprop_update(p, g, ms, mom, i, scale, lr, decay, momentum, eps);
}

}  // namespace

extern "C" size_t ntk_global_norm_workspace_bytes(size_t n) {
    return ((n + SUMSQ_PER_BLOCK - 1) / SUMSQ_PER_BLOCK) * sizeof(float);
}

extern "C" int ntk_global_norm(const float* grads, size_t n, float* workspace, float* gnorm, void* stream) {
    NTK_REQUIRE(grads && workspace && gnorm, NTK_ERR_BAD_PTR, "ntk_global_norm: null pointer");
    NTK_REQUIRE(n > 0, NTK_ERR_BAD_SHAPE, "ntk_global_norm: n=0");
    const int nb = (int)((n + SUMSQ_PER_BLOCK - 1) / SUMSQ_PER_BLOCK);
    sumsq_partial_kernel<<<nb, SUMSQ_BLOCK, 0, (hipStream_t)stream>>>(grads, workspace, n);
    NTK_CHECK_LAUNCH("ntk_global_norm(partial)");
    sumsq_final_kernel<<<1, 1024, 0, (hipStream_t)stream>>>(workspace, nb, gnorm);
    NTK_CHECK_LAUNCH("ntk_global_norm(final)");
    return NTK_OK;
}

extern "C" int ntk_rmsprop_clip_step(float* params, const float* grads, float* ms, float* mom, size_t n,
                                     float lr, float decay, float momentum, float eps, float clip_norm,
                                     const float* gnorm, void* stream) {
    NTK_REQUIRE(params && grads && ms && mom, NTK_ERR_BAD_PTR, "ntk_rmsprop_clip_step: null pointer");
    NTK_REQUIRE(n > 0, NTK_ERR_BAD_SHAPE, "ntk_rmsprop_clip_step: n=0");
    NTK_REQUIRE(clip_norm <= 0.f || gnorm, NTK_ERR_BAD_PTR, "ntk_rmsprop_clip_step: clip_norm > 0 needs gnorm");
    const unsigned nb = (unsigned)((n + 255) / 256);
    rmsprop_kernel<<<nb, 256, 0, (hipStream_t)stream>>>(params, grads, ms, mom, n, lr, decay, momentum, eps, clip_norm, gnorm);
    NTK_CHECK_LAUNCH("ntk_rmsprop_clip_step");
    return NTK_OK;
}

extern "C" int ntk_rmsprop_clip_step_checked(float* params, const float* grads, float* ms, float* mom, size_t n,
                                             float lr, float decay, float momentum, float eps, float clip_norm,
                                             const float* gnorm, float* loss, unsigned* skipped, void* stream) {
    NTK_REQUIRE(params && grads && ms && mom && gnorm, NTK_ERR_BAD_PTR, "ntk_rmsprop_clip_step_checked: null pointer");
    NTK_REQUIRE(n > 0, NTK_ERR_BAD_SHAPE, "ntk_rmsprop_clip_step_checked: n=0");
    const unsigned nb = (unsigned)((n + 255) / 256);
    rmsprop_checked_kernel<<<nb, 256, 0, (hipStream_t)stream>>>(params, grads, ms, mom, n, lr, decay, momentum, eps, clip_norm,
                                                                gnorm, loss, skipped);
    NTK_CHECK_LAUNCH("ntk_rmsprop_clip_step_checked");
    return NTK_OK;
}
