// Repeat-copy task of the vendored DNC (dnc/repeat_copy.py): the batch layout and the masked sigmoid cross entropy
//   * one-launch batch packer: observations in the sequence kernels' input layout, targets, mask   (repeat_copy.py:252-377)
//   * masked_sigmoid_cross_entropy with its gradient and the copy score in one pass                 (:29-66, train.py:104-105)
// Small memory-bound kernels: plain C++, wave64 reductions of fixed order, no floating-point atomics -- every result is the same
// bits from run to run.
#include <float.h>
#include "common.h"

namespace {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One thread per element of X [B, S, ldx]; the thread of column c also writes target column c (c <= num_bits) and, at c == 0, the
// mask of its row (ldx >= num_bits + 2, so a row's threads cover both).  A sequence of pattern length L and r repeats:
//   step 0            start flag (channel num_bits)
//   steps 1 .. L      the pattern
//   step L + 1        r / norm_max (channel num_bits + 1)
//   rows L + 2 .. L + 1 + L r   target = the pattern tiled r times;  row L + 2 + L r: end marker (target channel num_bits)
//   mask 1 on rows L + 2 .. L + 2 + L r;  everything else, and everything from L (r + 1) + 3 to S, zero.
// L and r are clamped to their ranges, so a bad table cannot index past bits [B, max_length, num_bits]; every store is to a row
// s < S of sequence b < B, whatever the table holds.
__global__ __launch_bounds__(256) void repeat_copy_pack_kernel(const float* __restrict__ bits, const int* __restrict__ lengths,
                                                               const int* __restrict__ repeats, float* __restrict__ X,
                                                               float* __restrict__ target, float* __restrict__ mask, int B, int S,
                                                               int nb, int ldx, int min_len, int max_len, int min_rep, int max_rep,
                                                               float norm_max) {
    const size_t total = (size_t)B * S * ldx;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(idx % ldx);
        const size_t row = idx / ldx;
        const int s = (int)(row % S), b = (int)(row / S);
        const int L = clampi(lengths[b], min_len, max_len), r = clampi(repeats[b], min_rep, max_rep);
        const int t0 = L + 2, tend = L + 2 + L * r;           // first target row, end-marker row (the launcher bounds L (r + 1) + 3)
        const float* pat = bits + (size_t)b * max_len * nb;
        float x = 0.f;
        if (c < nb) x = (s >= 1 && s <= L) ? pat[(size_t)(s - 1) * nb + c] : 0.f;
        else if (c == nb) x = s == 0 ? 1.f : 0.f;
        else if (c == nb + 1) x = s == L + 1 ? (float)r / norm_max : 0.f;
        X[idx] = x;
        if (c <= nb) {
            float t = 0.f;
            if (c < nb) t = (s >= t0 && s < tend) ? pat[(size_t)((s - t0) % L) * nb + c] : 0.f;
            else t = s == tend ? 1.f : 0.f;
            target[row * (size_t)(nb + 1) + c] = t;
        }
        if (c == 0) mask[row] = (s >= t0 && s <= tend) ? 1.f : 0.f;
    }
}

constexpr int XT = 256;      // threads of a sequence's workgroup

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// One workgroup per sequence b over its rows of logits / target [S, O] and mask [S]:
//   xent = max(x, 0) - x z + log1p(exp(-|x|))   (TensorFlow's stable form), summed over channels, then over the steps with their mask
//   loss_batch[b] = that sum (/ (sum of the mask + FLT_EPSILON) with time_average)
//   dlogits = (sigmoid(x) - z) mask scale, scale = the factors between loss_batch[b] and the loss (1 / B, 1 / ln 2), and 1 / (count + eps)
//   score[b] = (scored bits, bits where (x > 0) != (z > 0.5))
// A step whose mask is 0 is SELECTED out: it adds exactly 0 and its dlogits are +0.0, whatever its logits hold (NaN included).
__global__ __launch_bounds__(XT) void masked_sigmoid_xent_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                                 const float* __restrict__ mask, float* __restrict__ loss_batch,
                                                                 float* __restrict__ dlogits, int* __restrict__ score, int S, int O,
                                                                 float batch_scale, int time_average) {
    __shared__ float red[XT / 64];
    __shared__ int redi[2][XT / 64];
    __shared__ float count_s;
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* mk = mask + (size_t)b * S;
    float inv_count = 1.f;
    if (time_average) {
        float cnt = 0.f;
        for (int s = tid; s < S; s += XT) cnt += mk[s];
        cnt = block_sum<XT / 64>(wave_sum(cnt), red);
        if (tid == 0) count_s = cnt;
        __syncthreads();                                       // also: red is free again
        inv_count = 1.f / (count_s + FLT_EPSILON);
    }
    const float scale = batch_scale * inv_count;
    const size_t base = (size_t)b * S * O;
    const int n = S * O;
    float acc = 0.f;
    int scored = 0, wrong = 0;
    for (int i = tid; i < n; i += XT) {
        const float m = mk[i / O];
        float d = 0.f;
        if (m != 0.f) {
            const float x = logits[base + i], z = target[base + i];
            const float e = expf(-fabsf(x));
            acc += m * (fmaxf(x, 0.f) - x * z + log1pf(e));
            const float sg = x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
            d = (sg - z) * m * scale;
            scored += 1;
            wrong += ((x > 0.f) != (z > 0.5f)) ? 1 : 0;
        }
        if (dlogits) dlogits[base + i] = d;
    }
    scored = wave_sum_int(scored);
    wrong = wave_sum_int(wrong);
    if ((tid & 63) == 0) { redi[0][tid >> 6] = scored; redi[1][tid >> 6] = wrong; }
    const float tot = block_sum<XT / 64>(wave_sum(acc), red);       // its barrier also publishes redi
    if (tid == 0) {
        loss_batch[b] = tot * inv_count;
        if (score) {
            int a0 = 0, a1 = 0;
            for (int w = 0; w < XT / 64; ++w) { a0 += redi[0][w]; a1 += redi[1][w]; }
            score[2 * b] = a0;
            score[2 * b + 1] = a1;
        }
    }
}

// loss = (sum_b loss_batch[b]) * batch_scale: one wave, lane l adds b = l, l + 64, ... in ascending order, then the wave's fixed tree
__global__ __launch_bounds__(64) void xent_batch_sum_kernel(const float* __restrict__ loss_batch, float* __restrict__ loss, int B,
                                                            float batch_scale) {
    float acc = 0.f;
    for (int b = threadIdx.x; b < B; b += 64) acc += loss_batch[b];
    acc = wave_sum(acc);
    if (threadIdx.x == 0) *loss = acc * batch_scale;
}

}  // namespace

extern "C" int ntk_repeat_copy_pack(const float* bits, const int* lengths, const int* repeats, float* X, float* target, float* mask,
                                    int B, int S, int num_bits, int ldx, int min_length, int max_length, int min_repeats,
                                    int max_repeats, float norm_max, void* stream) {
    NTK_REQUIRE(bits && lengths && repeats && X && target && mask, NTK_ERR_BAD_PTR, "ntk_repeat_copy_pack: null pointer");
    NTK_REQUIRE(B > 0 && num_bits >= 1 && ldx >= num_bits + 2 && (ldx % 4) == 0, NTK_ERR_BAD_SHAPE,
                "ntk_repeat_copy_pack: B=%d num_bits=%d ldx=%d (>= num_bits + 2, multiple of 4)", B, num_bits, ldx);
    NTK_REQUIRE(min_length >= 1 && max_length >= min_length && min_repeats >= 0 && max_repeats >= min_repeats && norm_max > 0.f,
                NTK_ERR_BAD_SHAPE, "ntk_repeat_copy_pack: length range [%d, %d] (min >= 1), repeats range [%d, %d] (min >= 0), norm_max=%g",
                min_length, max_length, min_repeats, max_repeats, (double)norm_max);
    NTK_REQUIRE((long)max_length * ((long)max_repeats + 1) + 3 < 2147483647L, NTK_ERR_BAD_SHAPE,
                "ntk_repeat_copy_pack: max_length=%d max_repeats=%d: the longest sequence does not fit an int", max_length, max_repeats);
    // the lengths are on the device: what can be refused here is a step count below the SHORTEST sequence the ranges allow
    NTK_REQUIRE(S >= min_length * (min_repeats + 1) + 3, NTK_ERR_BAD_SHAPE,
                "ntk_repeat_copy_pack: S=%d is below the shortest sequence, min_length (min_repeats + 1) + 3 = %d", S,
                min_length * (min_repeats + 1) + 3);
    NTK_REQUIRE(ntk_aligned16(X), NTK_ERR_BAD_PTR, "ntk_repeat_copy_pack: X must be 16-byte aligned");
    const size_t total = (size_t)B * S * ldx;
    const unsigned nb = (unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    repeat_copy_pack_kernel<<<nb, 256, 0, (hipStream_t)stream>>>(bits, lengths, repeats, X, target, mask, B, S, num_bits, ldx,
                                                                 min_length, max_length, min_repeats, max_repeats, norm_max);
    NTK_CHECK_LAUNCH("ntk_repeat_copy_pack");
    return NTK_OK;
}

extern "C" int ntk_masked_sigmoid_xent(const float* logits, const float* target, const float* mask, float* loss, float* loss_batch,
                                       float* dlogits, int* score, int B, int S, int O, int time_average, int log_prob_in_bits,
                                       void* stream) {
    NTK_REQUIRE(logits && target && mask && loss && loss_batch, NTK_ERR_BAD_PTR, "ntk_masked_sigmoid_xent: null pointer");
    NTK_REQUIRE(B > 0 && S > 0 && O > 0 && (long)S * O < 2147483647L, NTK_ERR_BAD_SHAPE, "ntk_masked_sigmoid_xent: B=%d S=%d O=%d", B, S, O);
    float batch_scale = 1.0f / (float)B;
    if (log_prob_in_bits) batch_scale /= 0.69314718055994530942f;
    masked_sigmoid_xent_kernel<<<(unsigned)B, XT, 0, (hipStream_t)stream>>>(logits, target, mask, loss_batch, dlogits, score, S, O,
                                                                            batch_scale, time_average ? 1 : 0);
    NTK_CHECK_LAUNCH("ntk_masked_sigmoid_xent");
    xent_batch_sum_kernel<<<1, 64, 0, (hipStream_t)stream>>>(loss_batch, loss, B, batch_scale);
    NTK_CHECK_LAUNCH("ntk_masked_sigmoid_xent");
    return NTK_OK;
}
