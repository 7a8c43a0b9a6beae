// Tracking head around the NTM cell, initial state, and the optimiser:
//   * 64-point gather from conv4_3 + input serialiser   (direct_offset_output.py:392-399, :439-500)
//   * output gather + tanh + l2 loss, and its gradient   (:581-606)
//   * trainable initial state tanh/sigmoid + its gradient (ntm_cell.py:284-315)
//   * clip_by_global_norm + TF RMSProp                    (direct_offset_output.py:620-626)
// All HBM-bound elementwise / gather work: coalesced 16-byte accesses, no LDS.
#include "common.h"

namespace {

// one 128-thread workgroup per serialised row (b, t, i), i in [0, NF]; row i == NF is the delimiter
__global__ void gather_serialize_kernel(const float* __restrict__ fmap, const float* __restrict__ gts0,
                                        float* __restrict__ X, int T, int Hf, int Wf, int C, int ldx,
                                        int g0, int gstep, int gn, int delim_first) {
    const int NF = gn * gn;
    const int row = blockIdx.x;               // (b*T + t)*(NF+1) + position
    const int pos = row % (NF + 1);
    // training order: 64 feature rows then the delimiter (direct_offset_output.py:480-481);
    // inference order (quirk Q8): the delimiter row FIRST (test_tracker.py:400-404)
    const int i = delim_first ? (pos == 0 ? NF : pos - 1) : pos;
    const int ft = row / (NF + 1);            // b*T + t
    const int t = ft % T, b = ft / T;
    float* xr = X + (size_t)row * ldx;
    const int C4 = C >> 2;
    if (i < NF) {
        const int y = g0 + (i / gn) * gstep, x = g0 + (i % gn) * gstep;
        const f32x4* src = reinterpret_cast<const f32x4*>(fmap + (((size_t)ft * Hf + y) * Wf + x) * C);
        f32x4* dst = reinterpret_cast<f32x4*>(xr);
        for (int c = threadIdx.x; c < C4; c += blockDim.x) dst[c] = src[c];
    } else {
        f32x4 z = {0.f, 0.f, 0.f, 0.f};
        f32x4* dst = reinterpret_cast<f32x4*>(xr);
        for (int c = threadIdx.x; c < C4; c += blockDim.x) dst[c] = z;
    }
    for (int c = C + threadIdx.x; c < ldx; c += blockDim.x) {
        float v = 0.f;
        if (c == C) v = (i == NF) ? 1.f : 0.f;                                    // frame delimiter bit
        else if (c == C + 1) v = (t == 0 && i < NF && gts0) ? gts0[(size_t)b * NF + i] : 0.f;  // target, frame 0 only
        xr[c] = v;
    }
}

// single workgroup: pred = tanh(logit at the delimiter step of frames 1..T-1), loss = 0.5*sum (pred-off)^2,
// dlogits = (pred-off)*(1-pred^2) at those steps and 0 elsewhere
__global__ __launch_bounds__(1024) void offset_loss_kernel(const float* __restrict__ logits,
                                                            const float* __restrict__ offsets,
                                                            float* __restrict__ pred, float* __restrict__ loss,
                                                            float* __restrict__ dlogits, int B, int T, int NF, int O) {
    __shared__ float red[16];
    const int S = T * (NF + 1);
    const int tid = threadIdx.x;
    if (dlogits) {
        const size_t tot = (size_t)B * S * O;
        for (size_t i = tid; i < tot; i += blockDim.x) dlogits[i] = 0.f;
    }
    __syncthreads();
    float acc = 0.f;
    const int cnt = B * (T - 1) * O;
    for (int i = tid; i < cnt; i += blockDim.x) {
        const int o = i % O;
        const int bt = i / O;
        const int t = bt % (T - 1) + 1, b = bt / (T - 1);
        const size_t li = ((size_t)b * S + (size_t)t * (NF + 1) + NF) * O + o;
        const float p = tanhf(logits[li]);
        const float dlt = p - offsets[((size_t)b * T + t) * O + o];
        acc += dlt * dlt;
        if (pred) pred[i] = p;
        if (dlogits) dlogits[li] = dlt * (1.0f - p * p);
    }
    acc = wave_sum(acc);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        float s = 0.f;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += red[w];
        if (loss) *loss = 0.5f * s;
    }
}

// Sequential presentation of main.py's heat-map trackers (ntm_sevenbyseven, main.py:1701-1775; the same layout in
// :979-1291): every position of the feature map is a feature (F = Hf * Wf), rows are [feat(C), feature delimiter,
// frame delimiter, target]:
//   frame 0      : F rows [feat_i, 0, 0, gt0_i]
//   frame t >= 1 : one frame-delimiter row [0.., 0, 1, 0], then per feature [feat_i, 0, 0, 0] and [0.., 1, 0, 0]
// -> S = F + (T - 1) (2 F + 1) rows.  One 128-thread workgroup per row.
__global__ void serialize_sequential_kernel(const float* __restrict__ fmap, const float* __restrict__ gts0,
                                            float* __restrict__ X, int T, int F, int C, int ldx) {
    const int S = F + (T - 1) * (2 * F + 1);
    const int row = blockIdx.x, b = row / S, s = row - b * S;
    int t = 0, i = s, kind = 0;                 // kind 0: feature row, 1: feature delimiter, 2: frame delimiter
    if (s >= F) {
        const int r = s - F;
        t = 1 + r / (2 * F + 1);
        const int p = r % (2 * F + 1);
        if (p == 0) { kind = 2; i = 0; }
        else { i = (p - 1) >> 1; kind = ((p - 1) & 1) ? 1 : 0; }
    }
    float* xr = X + (size_t)row * ldx;
    const int C4 = C >> 2;
    f32x4* dst = reinterpret_cast<f32x4*>(xr);
    if (kind == 0) {
        const f32x4* src = reinterpret_cast<const f32x4*>(fmap + (((size_t)b * T + t) * F + i) * C);
        for (int c = threadIdx.x; c < C4; c += blockDim.x) dst[c] = src[c];
    } else {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        for (int c = threadIdx.x; c < C4; c += blockDim.x) dst[c] = z;
    }
    for (int c = C + threadIdx.x; c < ldx; c += blockDim.x) {
        float v = 0.f;
        if (c == C) v = kind == 1 ? 1.f : 0.f;
        else if (c == C + 1) v = kind == 2 ? 1.f : 0.f;
        else if (c == C + 2) v = (t == 0 && gts0) ? gts0[(size_t)b * F + i] : 0.f;
        xr[c] = v;
    }
}

// Heat-map head of the sequential trackers (main.py:1880-1922): the logit (output_dim 1) at each FEATURE-DELIMITER step of
// frames 1..T-1 is one entry of that frame's F-way score vector; loss = sum_{b,t} softmax_cross_entropy(scores, gt[b,t]) /
// (T - 1).  One wave per (b, t >= 1): softmax over F, cross entropy against the (soft) labels, and the gradient
// (softmax * sum(labels) - labels) / (T - 1) scattered to the gathered steps (zero elsewhere; dlogits zeroed first).
__global__ __launch_bounds__(1024) void heatmap_ce_loss_kernel(const float* __restrict__ logits, const float* __restrict__ gt,
                                                                float* __restrict__ probs, float* __restrict__ loss,
                                                                float* __restrict__ dlogits, int B, int T, int F) {
    __shared__ float red[16];
    const int S = F + (T - 1) * (2 * F + 1);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    if (dlogits) {
        for (size_t i = tid; i < (size_t)B * S; i += blockDim.x) dlogits[i] = 0.f;
    }
    __syncthreads();
    float acc = 0.f;
    const float inv = 1.0f / (float)(T - 1);
    for (int bt = wave; bt < B * (T - 1); bt += nw) {
        const int b = bt / (T - 1), t = bt % (T - 1) + 1;
        const size_t base = (size_t)b * S + F + (size_t)(t - 1) * (2 * F + 1) + 1;      // first feature row of frame t
        const float* lab = gt + ((size_t)b * (T - 1) + (t - 1)) * F;
        float mx = -INFINITY;
        for (int i = lane; i < F; i += 64) mx = fmaxf(mx, logits[base + 2 * i + 1]);
        mx = wave_max(mx);
        float se = 0.f, sl = 0.f, dotl = 0.f;
        for (int i = lane; i < F; i += 64) {
            const float z = logits[base + 2 * i + 1] - mx, y = lab[i];
            se += expf(z); sl += y; dotl += y * z;
        }
        se = wave_sum(se); sl = wave_sum(sl); dotl = wave_sum(dotl);
        const float lse = logf(se);
        if (lane == 0) acc += sl * lse - dotl;                   // -sum y (z - lse)
        for (int i = lane; i < F; i += 64) {
            const float p = expf(logits[base + 2 * i + 1] - mx - lse);
            if (probs) probs[((size_t)b * (T - 1) + (t - 1)) * F + i] = p;
            if (dlogits) dlogits[base + 2 * i + 1] = (p * sl - lab[i]) * inv;
        }
    }
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        float s = 0.f;
        for (int w = 0; w < nw; ++w) s += red[w];
        if (loss) *loss = s * inv;
    }
}

// Two-step presentation of main.py's ntm_two_step (:862-977) / ntm_tracker_new.NTMTracker(two_step=True) (:112-195): a whole
// frame is ONE step.  Rows [switch, feat(D), target(F)]: step 0 = [0, feat_0, target]; frame t >= 1 = [0, feat_t, 0] then the
// query step [1, 0, 0]  ->  S = 2 T - 1 steps.  feat [B, T, D] (D a multiple of 4 is NOT required), target [B, F].
__global__ void serialize_two_step_kernel(const float* __restrict__ feat, const float* __restrict__ target, float* __restrict__ X,
                                          int B, int T, int D, int F, int ldx) {
    const int S = 2 * T - 1;
    const size_t total = (size_t)B * S * ldx;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(idx % ldx);
        const size_t r = idx / ldx;
        const int s = (int)(r % S), b = (int)(r / S);
        const bool query = s > 0 && (s & 1) == 0;               // steps 2, 4, ...: "ask for output"
        const int t = (s + 1) >> 1;                              // frame shown at steps 0, 1, 3, 5, ...
        float v = 0.f;
        if (c == 0) v = query ? 1.f : 0.f;
        else if (c <= D) v = query ? 0.f : feat[((size_t)b * T + t) * D + (c - 1)];
        else if (c <= D + F) v = (s == 0 && target) ? target[(size_t)b * F + (c - 1 - D)] : 0.f;
        X[idx] = v;
    }
}

// Loss of ntm_two_step (main.py:903-951): labels [B, 2T-1, F+1] = background row [0..0,1] at step 0 and at every
// presentation step, [gt_t, 0] at the query step of frame t >= 1; the labels pass through tf.nn.softmax before the cross
// entropy (as coded); loss = sum_rows CE(logits_row, softmax(label_row)) / ((2T-1) B).  One wave per row.
__global__ __launch_bounds__(1024) void two_step_ce_loss_kernel(const float* __restrict__ logits, const float* __restrict__ gt,
                                                                 float* __restrict__ probs, float* __restrict__ loss,
                                                                 float* __restrict__ dlogits, int B, int T, int F) {
    __shared__ float red[16];
    const int S = 2 * T - 1, K = F + 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const float inv = 1.0f / ((float)S * (float)B);
    float acc = 0.f;
    for (int r = wave; r < B * S; r += nw) {
        const int b = r / S, s = r - b * S;
        const bool query = s > 0 && (s & 1) == 0;
        const float* g = query ? gt + ((size_t)b * T + (s >> 1)) * F : nullptr;
        const float* z = logits + (size_t)r * K;
        // softmax of the label row (values 0/1, so no max subtraction is needed; done anyway for arbitrary heat-maps)
        float lmx = query ? 0.f : 1.f;
        if (query) { for (int i = lane; i < F; i += 64) lmx = fmaxf(lmx, g[i]); lmx = wave_max(lmx); }
        float lse_l = 0.f, mx = -INFINITY;
        for (int i = lane; i < K; i += 64) {
            const float y = (i < F) ? (query ? g[i] : 0.f) : (query ? 0.f : 1.f);
            lse_l += expf(y - lmx);
            mx = fmaxf(mx, z[i]);
        }
        lse_l = wave_sum(lse_l); mx = wave_max(mx);
        float se = 0.f;
        for (int i = lane; i < K; i += 64) se += expf(z[i] - mx);
        se = wave_sum(se);
        const float lse = logf(se);
        float ce = 0.f;
        for (int i = lane; i < K; i += 64) {
            const float y = (i < F) ? (query ? g[i] : 0.f) : (query ? 0.f : 1.f);
            const float q = expf(y - lmx) / lse_l;               // softmax(labels)
            const float lp = z[i] - mx - lse;
            ce -= q * lp;
            const float p = expf(lp);
            if (probs) probs[(size_t)r * K + i] = p;
            if (dlogits) dlogits[(size_t)r * K + i] = (p - q) * inv;
        }
        ce = wave_sum(ce);
        if (lane == 0) acc += ce;
    }
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        float sacc = 0.f;
        for (int w = 0; w < nw; ++w) sacc += red[w];
        if (loss) *loss = sacc * inv;
    }
}

// copy task head (main.py:1603-1610): p = sigmoid(logit); loss = mean(-(y log(p+eps) + (1-y) log(1-p+eps))), eps = 1e-7
// (tf.losses.log_loss defaults); dlogits = d loss / d logit.  Single workgroup, fixed-order reduction.
__global__ __launch_bounds__(1024) void log_loss_kernel(const float* __restrict__ logits, const float* __restrict__ labels,
                                                         float* __restrict__ loss, float* __restrict__ dlogits, int n) {
    __shared__ float red[16];
    const float eps = 1e-7f, inv = 1.0f / (float)n;
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const float p = 1.0f / (1.0f + expf(-logits[i]));
        const float y = labels[i];
        acc += -(y * logf(p + eps) + (1.0f - y) * logf(1.0f - p + eps));
        if (dlogits) dlogits[i] = inv * (-(y / (p + eps)) + (1.0f - y) / (1.0f - p + eps)) * p * (1.0f - p);
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += red[w];
        *loss = s * inv;
    }
}

// act: 0 = tanh, 1 = sigmoid.  out[b][i] = act(v[i])
__global__ void init_state_kernel(const float* __restrict__ v, float* __restrict__ out, int n, int B, int act) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = v[i];
    const float y = act ? 1.0f / (1.0f + expf(-x)) : tanhf(x);
    for (int b = 0; b < B; ++b) out[(size_t)b * n + i] = y;
}

// dv[i] (+)= act'(v[i]) * sum_b dout[b][i]
__global__ void init_state_bwd_kernel(const float* __restrict__ v, const float* __restrict__ dout,
                                      float* __restrict__ dv, int n, int B, int act, int accumulate) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += dout[(size_t)b * n + i];
    const float x = v[i];
    float dy;
    if (act) { const float y = 1.0f / (1.0f + expf(-x)); dy = y * (1.0f - y); }
    else { const float y = tanhf(x); dy = 1.0f - y * y; }
    const float g = s * dy;
    dv[i] = accumulate ? dv[i] + g : g;
}

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
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int w = 0; w < SUMSQ_BLOCK / 64; ++w) s += red[w];
        partial[blockIdx.x] = s;
    }
}

__global__ void sumsq_final_kernel(const float* __restrict__ partial, int nblocks, float* __restrict__ gnorm) {
    __shared__ float red[16];
    float acc = 0.f;
    for (int i = threadIdx.x; i < nblocks; i += blockDim.x) acc += partial[i];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += red[w];
        *gnorm = sqrtf(s);
    }
}

// tf.clip_by_global_norm then tf.train.RMSPropOptimizer (ms slot starts at ONE, eps inside the sqrt)
__global__ void rmsprop_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ ms,
                               float* __restrict__ mom, size_t n, float lr, float decay, float momentum,
                               float eps, float clip, const float* __restrict__ gnorm) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float scale = 1.0f;
    if (clip > 0.f) scale = clip / fmaxf(*gnorm, clip);
    const float gi = g[i] * scale;
    const float m2 = decay * ms[i] + (1.0f - decay) * gi * gi;
    const float mo = momentum * mom[i] + lr * gi / sqrtf(m2 + eps);
    ms[i] = m2;
    mom[i] = mo;
    p[i] -= mo;
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
    const float gi = g[i] * scale;
    const float m2 = decay * ms[i] + (1.0f - decay) * gi * gi;
    const float mo = momentum * mom[i] + lr * gi / sqrtf(m2 + eps);
    ms[i] = m2;
    mom[i] = mo;
    p[i] -= mo;
}

}  // namespace

static int gather_serialize_impl(const float* fmap, const float* gts0, float* X, int B, int T,
                                 int Hf, int Wf, int C, int ldx, int grid_start, int grid_step,
                                 int grid_n, int delim_first, void* stream) {
    NTK_REQUIRE(fmap && X, NTK_ERR_BAD_PTR, "ntk_gather_serialize: null pointer");
    NTK_REQUIRE(ntk_aligned16(fmap) && ntk_aligned16(X), NTK_ERR_BAD_PTR, "ntk_gather_serialize: 16-byte alignment");
    NTK_REQUIRE(B > 0 && T > 0 && C > 0 && (C % 4) == 0 && ldx >= C + 2 && (ldx % 4) == 0 && grid_n > 0 &&
                    grid_start >= 0 && grid_step > 0 && grid_start + (grid_n - 1) * grid_step < Hf &&
                    grid_start + (grid_n - 1) * grid_step < Wf,
                NTK_ERR_BAD_SHAPE, "ntk_gather_serialize: B=%d T=%d C=%d ldx=%d grid=(%d,%d,%d) map=%dx%d", B, T, C,
                ldx, grid_start, grid_step, grid_n, Hf, Wf);
    const long rows = (long)B * T * (grid_n * grid_n + 1);
    NTK_REQUIRE(rows < 2147483647L, NTK_ERR_BAD_SHAPE, "ntk_gather_serialize: too many rows");
    gather_serialize_kernel<<<(unsigned)rows, 128, 0, (hipStream_t)stream>>>(fmap, gts0, X, T, Hf, Wf, C, ldx,
                                                                            grid_start, grid_step, grid_n, delim_first);
    NTK_CHECK_LAUNCH("ntk_gather_serialize");
    return NTK_OK;
}

extern "C" int ntk_gather_serialize(const float* fmap, const float* gts0, float* X, int B, int T,
                                    int Hf, int Wf, int C, int ldx, int grid_start, int grid_step,
                                    int grid_n, void* stream) {
    return gather_serialize_impl(fmap, gts0, X, B, T, Hf, Wf, C, ldx, grid_start, grid_step, grid_n, 0, stream);
}

extern "C" int ntk_gather_serialize_online(const float* fmap, const float* gts0, float* X, int B, int T,
                                           int Hf, int Wf, int C, int ldx, int grid_start, int grid_step,
                                           int grid_n, void* stream) {
    return gather_serialize_impl(fmap, gts0, X, B, T, Hf, Wf, C, ldx, grid_start, grid_step, grid_n, 1, stream);
}

// Rounding of the image stages.  The two per-pixel functions below say which operations round: the sample positions and the
// fractions are separate multiplications, additions and subtractions, each rounded (contraction is off inside the functions), and
// each of the three interpolations a + (b - a) * t is ONE fused multiply-add, written as fmaf.  Left to the compiler, the choice
// depends on the code around the inlined function -- it fused `sy - floor(sy)` with the product behind sy in one kernel and not in
// another -- and the same stage would give different bits from different kernels.
//
// Sources of the image kernels.  A stage reads its input through an accessor, at(y, x, c) -> the fp32 value of one pixel, so that
// a stage is written ONCE and runs the same expressions whether its input lies in memory or is computed on the fly.
// DenseImage: a whole row-major image [H,W,C] in memory; PixelT float, or unsigned char (converted to fp32 exactly).
template <typename PixelT>
struct DenseImage {
    const PixelT* __restrict__ img;
    int W, C;
    __device__ __forceinline__ float at(int y, int x, int c) const { return (float)img[((size_t)y * W + x) * C + c]; }
};

// PackedRect: the sub-rectangle (y0, x0, h, w) of a uint8 image, stored row-major on its own at an arbitrary byte address (byte
// loads only: no alignment is assumed).  Indices are those of the FULL image; each is clamped into the rectangle before the load,
// so no index can leave the h * w * C bytes (a rectangle that covers every tap is read exactly as the full image would be).
struct PackedRect {
    const unsigned char* __restrict__ pix;
    int y0, x0, h, w, C;
    __device__ __forceinline__ float at(int y, int x, int c) const {
        const int yy = min(max(y - y0, 0), h - 1), xx = min(max(x - x0, 0), w - 1);
        return (float)pix[((size_t)yy * w + xx) * C + c];
    }
};

// One output element of tf.image.resize_images(..., BILINEAR) with TF-1 defaults (align_corners=False, no half-pixel centres):
// src = dst * (in / out); neighbours floor(src) and min(floor(src)+1, in-1).  The ONE copy of the per-pixel arithmetic, shared
// by resize_bilinear_kernel and (through ResizedView) by the fused frames kernel.
template <typename Src>
__device__ __forceinline__ float resize_bilinear_pixel(const Src& src, int H, int W, int OH, int OW, int y, int x, int c) {
#pragma clang fp contract(off)      // see "Rounding of the image stages" above: the fused multiply-adds are the three written out
    const float sy = (float)y * ((float)H / (float)OH), sx = (float)x * ((float)W / (float)OW);
    const int y0 = (int)floorf(sy), x0 = (int)floorf(sx);
    const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
    const float fy = sy - (float)y0, fx = sx - (float)x0;
    const float tl = src.at(y0, x0, c), tr = src.at(y0, x1, c);
    const float bl = src.at(y1, x0, c), br = src.at(y1, x1, c);
    const float top = fmaf(fx, tr - tl, tl), bot = fmaf(fx, br - bl, bl);
    return fmaf(fy, bot - top, top);
}

// ResizedView: the [OH,OW,C] bilinear resize of a source [H,W,C] that is never stored: every pixel is computed when it is read.
template <typename Src>
struct ResizedView {
    Src src;
    int H, W, OH, OW;
    __device__ __forceinline__ float at(int y, int x, int c) const { return resize_bilinear_pixel(src, H, W, OH, OW, y, x, c); }
};

// One output element of tf.image.crop_and_resize (bilinear, normalised box y1,x1,y2,x2) of (image - mean): the ONE copy of the
// per-pixel arithmetic, shared by the one-box kernel, the batched kernel and the fused frames kernel, so that the same box on
// the same image gives the same bits from every entry.  src: an accessor (above) of an image [H,W,C].
template <typename Src>
__device__ __forceinline__ float crop_resize_pixel(const Src& src, int H, int W, const float* __restrict__ mean,
                                                   float y1, float x1, float y2, float x2, int ch, int cw, float extrapolation,
                                                   int y, int x, int c) {
#pragma clang fp contract(off)      // see "Rounding of the image stages" above
    const float hs = (ch > 1) ? (y2 - y1) * (float)(H - 1) / (float)(ch - 1) : 0.f;
    const float wsc = (cw > 1) ? (x2 - x1) * (float)(W - 1) / (float)(cw - 1) : 0.f;
    const float in_y = (ch > 1) ? y1 * (float)(H - 1) + (float)y * hs : 0.5f * (y1 + y2) * (float)(H - 1);
    const float in_x = (cw > 1) ? x1 * (float)(W - 1) + (float)x * wsc : 0.5f * (x1 + x2) * (float)(W - 1);
    float v = extrapolation;
    if (in_y >= 0.f && in_y <= (float)(H - 1) && in_x >= 0.f && in_x <= (float)(W - 1)) {
        const int ty = (int)floorf(in_y), by = (int)ceilf(in_y);
        const int lx = (int)floorf(in_x), rx = (int)ceilf(in_x);
        const float yl = in_y - (float)ty, xl = in_x - (float)lx;
        const float m = mean ? mean[c] : 0.f;
        const float tl = src.at(ty, lx, c) - m, tr = src.at(ty, rx, c) - m;
        const float bl = src.at(by, lx, c) - m, br = src.at(by, rx, c) - m;
        const float top = fmaf(xl, tr - tl, tl), bot = fmaf(xl, br - bl, bl);
        v = fmaf(yl, bot - top, top);
    }
    return v;
}

// tf.image.crop_and_resize (bilinear, one box) of (image - mean): out[y][x][c], extrapolation outside the image
__global__ void crop_resize_kernel(const float* __restrict__ img, int H, int W, int C, const float* __restrict__ mean,
                                   float y1, float x1, float y2, float x2, float* __restrict__ out, int ch, int cw,
                                   float extrapolation) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= ch * cw * C) return;
    const int c = idx % C, x = (idx / C) % cw, y = idx / (C * cw);
    out[idx] = crop_resize_pixel(DenseImage<float>{img, W, C}, H, W, mean, y1, x1, y2, x2, ch, cw, extrapolation, y, x, c);
}

// The same for B boxes in one launch (blockIdx.y = tracker b): tracker b crops frame frame_of[b] of images [F,H,W,C] to boxes[b]
// (both read from device memory).  A frame index outside [0, F) is never dereferenced: that tracker's crop is the extrapolation value.
template <typename PixelT>
__global__ void crop_resize_batch_kernel(const PixelT* __restrict__ images, int F, int H, int W, int C,
                                         const int* __restrict__ frame_of, const float* __restrict__ boxes,
                                         const float* __restrict__ mean, float* __restrict__ out, int ch, int cw,
                                         float extrapolation) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int total = ch * cw * C;
    if (idx >= total) return;
    const int b = blockIdx.y;
    const int f = frame_of[b];
    float v = extrapolation;
    if (f >= 0 && f < F) {
        const int c = idx % C, x = (idx / C) % cw, y = idx / (C * cw);
        const float* box = boxes + 4 * (size_t)b;
        v = crop_resize_pixel(DenseImage<PixelT>{images + (size_t)f * H * W * C, W, C}, H, W, mean, box[0], box[1], box[2], box[3],
                              ch, cw, extrapolation, y, x, c);
    }
    out[(size_t)b * total + idx] = v;
}

// The training input of n frames in one launch (blockIdx.y = frame, one thread per output pixel, all C channels): the crop of
// (resize(frame) - mean), the resized image [RH,RW,C] never stored -- each of the crop stage's four taps is a pixel of
// ResizedView, computed from four source bytes.  table int64 [n,7]: byte_offset, H, W, y0, x0, h, w (include/ntmtrack.h).  A row
// whose rectangle is empty, leaves its image or leaves [0, pixels_bytes) is never dereferenced: its crop is the extrapolation
// value everywhere (so is one of a frame above 2^30 rows or columns: the stages' int indices stay far from overflow).  flip_x: output
// column x holds crop column cw-1-x.
__global__ void frames_crop_batch_kernel(const unsigned char* __restrict__ pixels, long long pixels_bytes,
                                         const long long* __restrict__ table, const float* __restrict__ boxes,
                                         const float* __restrict__ mean, float* __restrict__ out, int C, int RH, int RW, int ch, int cw,
                                         int flip_x, float extrapolation) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= ch * cw) return;
    const int f = blockIdx.y;
    const long long* row = table + 7 * (size_t)f;
    const long long off = row[0], H = row[1], W = row[2], y0 = row[3], x0 = row[4], h = row[5], w = row[6];
    const bool ok = H >= 1 && W >= 1 && H <= (1LL << 30) && W <= (1LL << 30) && h >= 1 && w >= 1 && y0 >= 0 && x0 >= 0 &&
                    y0 <= H - h && x0 <= W - w && off >= 0 && off < pixels_bytes && h <= (pixels_bytes - off) / (w * C);
    const int x = p % cw, y = p / cw;
    float* o = out + ((size_t)f * ch * cw + p) * C;
    if (!ok) {
        for (int c = 0; c < C; ++c) o[c] = extrapolation;
        return;
    }
    const ResizedView<PackedRect> view{PackedRect{pixels + off, (int)y0, (int)x0, (int)h, (int)w, C}, (int)H, (int)W, RH, RW};
    const float* box = boxes + 4 * (size_t)f;
    const float by1 = box[0], bx1 = box[1], by2 = box[2], bx2 = box[3];
    const int sx = flip_x ? cw - 1 - x : x;
    for (int c = 0; c < C; ++c)
        o[c] = crop_resize_pixel(view, RH, RW, mean, by1, bx1, by2, bx2, ch, cw, extrapolation, y, sx, c);
}

// Per-frame box bookkeeping of the online tracker for B trackers, one thread each, the geometry in double precision throughout
// (state layout: include/ntmtrack.h, NTK_TRACK_STATE_*).  offsets = fp32 tanh(logits[b, S-1, :]) ordered (dy, dx); the centred box
// 0.5 -+ bbox_grid / (2 cropbox_grid) shifted by them; back through the inverse of the crop transformation (the crop box was mapped
// onto the unit square, so the inverse is X * (x2 - x1) + x1); scaled by (w, h) -- NOT (w - 1, h - 1): the decode and
// normalize_bbox are asymmetric in the reference and here; the region (x, y, width, height); then the next frame's box state:
// a region whose four numbers are all < 1 is taken as already normalised (test_tracker.py:306-309), else divided by
// (h - 1, w - 1); the crop box is that box scaled about its centre by cropbox_grid / bbox_grid.
__global__ void track_boxes_update_kernel(const float* __restrict__ logits, int B, int S, double cropbox_grid, double bbox_grid,
                                          const unsigned char* __restrict__ active, double* __restrict__ state,
                                          float* __restrict__ cropbox32, double* __restrict__ regions, float* __restrict__ offsets,
                                          int* __restrict__ frame) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    if (active && !active[b]) return;
    double* st = state + (size_t)b * NTK_TRACK_STATE_DOUBLES;
    const float* lg = logits + ((size_t)b * S + (S - 1)) * 2;
    const float fy = tanhf(lg[0]), fx = tanhf(lg[1]);       // fp32 tanh, as the single tracker takes it (torch.tanh of fp32 logits)
    const double w = st[NTK_TRACK_STATE_W], h = st[NTK_TRACK_STATE_H];
    const double* cb = st + NTK_TRACK_STATE_CROPBOX;
    const double width = bbox_grid / cropbox_grid;
    const double lo = .5 - width / 2, hi = .5 + width / 2;
    const double sy = cb[2] - cb[0], sx = cb[3] - cb[1];
    // the shifted box is an fp32 sum, as in the single tracker: there a Python float plus an fp32 offset is an fp32 number
    const double oy1 = (float)lo + fy, ox1 = (float)lo + fx, oy2 = (float)hi + fy, ox2 = (float)hi + fx;
    const double y1 = (oy1 * sy + cb[0]) * h, x1 = (ox1 * sx + cb[1]) * w;
    const double y2 = (oy2 * sy + cb[0]) * h, x2 = (ox2 * sx + cb[1]) * w;
    const double rw = x2 - x1, rh = y2 - y1;
    const bool normalized = x1 < 1 && y1 < 1 && rw < 1 && rh < 1;
    const double by = normalized ? 1.0 : h - 1, bx = normalized ? 1.0 : w - 1;
    const double n0 = y1 / by, n1 = x1 / bx, n2 = (y1 + rh) / by, n3 = (x1 + rw) / bx;
    const double scale = cropbox_grid / bbox_grid;
    const double cy = (n0 + n2) / 2, cx = (n1 + n3) / 2, hy = (n2 - n0) * scale / 2, hx = (n3 - n1) * scale / 2;
    const double c0 = cy - hy, c1 = cx - hx, c2 = cy + hy, c3 = cx + hx;
    double* nb = st + NTK_TRACK_STATE_BBOX;
    double* ncb = st + NTK_TRACK_STATE_CROPBOX;
    nb[0] = n0; nb[1] = n1; nb[2] = n2; nb[3] = n3;
    ncb[0] = c0; ncb[1] = c1; ncb[2] = c2; ncb[3] = c3;
    float* c32 = cropbox32 + 4 * (size_t)b;
    c32[0] = (float)c0; c32[1] = (float)c1; c32[2] = (float)c2; c32[3] = (float)c3;
    double* rg = regions + 4 * (size_t)b;
    rg[0] = x1; rg[1] = y1; rg[2] = rw; rg[3] = rh;
    offsets[2 * (size_t)b] = fy;
    offsets[2 * (size_t)b + 1] = fx;
    if (frame) frame[b] += 1;
}

// Overlap of two rectangles (x, y, w, h) with w, h >= 0, in float64 on real-valued coordinates (the VOT / OTB overlap).  Both are
// taken to corners first and every width is a difference of corners, so the intersection of a box with itself has the box's own
// sides bit for bit: its IoU is a / (a + a - a) = 1.0 exactly, and boxes that only touch meet in a side of exactly 0.
// Contraction is off in these functions (the header's __dmul_rn is a plain product the compiler may still fuse): a product is
// rounded before it is added, so integer-valued boxes give the bits of any IEEE float64 evaluation of the same expression.
__device__ __forceinline__ double rect_iou(double px, double py, double pw, double ph, double gx, double gy, double gw, double gh) {
#pragma clang fp contract(off)
    const double px2 = px + pw, py2 = py + ph, gx2 = gx + gw, gy2 = gy + gh;
    const double ix = fmin(px2, gx2) - fmax(px, gx), iy = fmin(py2, gy2) - fmax(py, gy);
    if (!(ix > 0 && iy > 0)) return 0.0;
    const double inter = ix * iy;
    const double area_p = (px2 - px) * (py2 - py), area_g = (gx2 - gx) * (gy2 - gy);
    const double uni = (area_p + area_g) - inter;
    const double iou = inter / uni;
    if (!(iou > 0)) return 0.0;                 // an intersection that underflowed, or inf / inf of huge boxes
    return iou > 1.0 ? 1.0 : iou;
}

__device__ __forceinline__ bool finite4(const double* r) { return isfinite(r[0]) && isfinite(r[1]) && isfinite(r[2]) && isfinite(r[3]); }

// ---- polygon ground truth (contract: include/ntmtrack.h, NTK_POLY_*) ----------------------------------------------------------
// A region is double[NTK_POLY_DOUBLES]: the leading pairs whose two numbers are both finite are its vertices, the rest is padding.
__device__ __forceinline__ int poly_vertices(const double* g) {
    int n = 0;
    while (n < NTK_POLY_MAX_POINTS && isfinite(g[2 * n]) && isfinite(g[2 * n + 1])) ++n;
    return n;
}

// Shoelace area of n points (x0, y0, x1, y1, ...) about the first one, either orientation.  Integer coordinates give it exactly.
__device__ __forceinline__ double shoelace_area(const double* pts, int n) {
#pragma clang fp contract(off)
    if (n < 3) return 0.0;
    const double ox = pts[0], oy = pts[1];
    double s = 0.0;
    for (int i = 0; i < n; ++i) {
        const int j = i + 1 < n ? i + 1 : 0;
        s += (pts[2 * i] - ox) * (pts[2 * j + 1] - oy) - (pts[2 * j] - ox) * (pts[2 * i + 1] - oy);
    }
    return fabs(s) / 2;
}

// The ground truth of one frame as both kernels see it: the rectangle (the region itself, or the polygon's bounding rectangle:
// the true minimum and maximum over its vertices), and for a polygon its vertex count and area.
struct Truth {
    double x, y, w, h, area;
    int n;
};

// -> present.  POLY: at least 3 vertices, a bounding rectangle with w > 0 and h > 0, a shoelace area > 0.
template <bool POLY>
__device__ __forceinline__ bool read_truth(const double* g, Truth& tr) {
#pragma clang fp contract(off)
    if constexpr (!POLY) {
        tr.x = g[0]; tr.y = g[1]; tr.w = g[2]; tr.h = g[3];
        tr.area = 0.0; tr.n = 0;
        return finite4(g) && g[2] > 0 && g[3] > 0;
    } else {
        const int n = poly_vertices(g);
        tr.n = n;
        if (n < 3) return false;
        double x0 = g[0], x1 = g[0], y0 = g[1], y1 = g[1];
        for (int i = 1; i < n; ++i) {
            x0 = fmin(x0, g[2 * i]); x1 = fmax(x1, g[2 * i]);
            y0 = fmin(y0, g[2 * i + 1]); y1 = fmax(y1, g[2 * i + 1]);
        }
        tr.x = x0; tr.y = y0; tr.w = x1 - x0; tr.h = y1 - y0;
        if (!(tr.w > 0 && tr.h > 0)) return false;
        tr.area = shoelace_area(g, n);
        return tr.area > 0;
    }
}

// One half-plane of Sutherland-Hodgman: keeps the part of the n-gon ``in`` whose coordinate ``axis`` (0 = x, 1 = y) is strictly
// above (or strictly below) c.  A crossing point gets c itself on that axis, so the next test on it is exact.  -> points written
// to ``out``, never more than POLY_CLIP_MAX (a half-plane turns n points into at most 3n/2: 8 -> 12 -> 18 -> 27 -> 40).
constexpr int POLY_CLIP_MAX = 40;
__device__ __forceinline__ int clip_half_plane(const double* in, int n, double* out, int axis, double c, bool above) {
#pragma clang fp contract(off)
    const int o = 1 - axis;
    int m = 0;
    for (int i = 0; i < n; ++i) {
        const double* a = in + 2 * i;
        const double* b = in + 2 * (i + 1 < n ? i + 1 : 0);
        const bool ia = above ? a[axis] > c : a[axis] < c, ib = above ? b[axis] > c : b[axis] < c;
        if (ia != ib && m < POLY_CLIP_MAX) {
            out[2 * m + axis] = c;
            out[2 * m + o] = a[o] + (b[o] - a[o]) * ((c - a[axis]) / (b[axis] - a[axis]));
            ++m;
        }
        if (ib && m < POLY_CLIP_MAX) {
            out[2 * m] = b[0];
            out[2 * m + 1] = b[1];
            ++m;
        }
    }
    return m;
}

// Overlap of the rectangle (x, y, w, h), w, h >= 0, with a simple polygon of tr.n vertices at g: the polygon is clipped against
// the rectangle's four sides in turn and the shoelace area of what is left is |P n R|.  The inside tests are strict, so a polygon
// that only touches the rectangle, or lies beside it, leaves an empty list and scores exactly 0.0; an axis-aligned integer 4-gon
// goes through exact arithmetic only and gives rect_iou's bits.  No contraction, clamped to [0, 1].
__device__ __forceinline__ double poly_iou(double px, double py, double pw, double ph, const double* g, const Truth& tr) {
#pragma clang fp contract(off)
    const double px2 = px + pw, py2 = py + ph;
    double a[2 * POLY_CLIP_MAX], b[2 * POLY_CLIP_MAX];
    int m = clip_half_plane(g, tr.n, a, 0, px, true);
    if (m) m = clip_half_plane(a, m, b, 0, px2, false);
    if (m) m = clip_half_plane(b, m, a, 1, py, true);
    if (m) m = clip_half_plane(a, m, b, 1, py2, false);
    if (m < 3) return 0.0;
    const double inter = shoelace_area(b, m);
    const double area_p = (px2 - px) * (py2 - py);
    const double uni = (area_p + tr.area) - inter;
    const double iou = inter / uni;
    if (!(iou > 0)) return 0.0;
    return iou > 1.0 ? 1.0 : iou;
}

template <bool POLY>
__device__ __forceinline__ double truth_iou(double px, double py, double pw, double ph, const double* g, const Truth& tr) {
    if constexpr (POLY) return poly_iou(px, py, pw, ph, g, tr);
    else return rect_iou(px, py, pw, ph, tr.x, tr.y, tr.w, tr.h);
}

// (min x, min y, max x - min x, max y - min y) over each region's vertices, four NaNs for an absent one: one thread per region.
__global__ void track_poly_bounds_kernel(const double* __restrict__ poly, int n, double* __restrict__ rects) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Truth tr;
    const bool present = read_truth<true>(poly + (size_t)NTK_POLY_DOUBLES * i, tr);
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double* r = rects + 4 * (size_t)i;
    r[0] = present ? tr.x : nan; r[1] = present ? tr.y : nan; r[2] = present ? tr.w : nan; r[3] = present ? tr.h : nan;
}

// Per-clip tracking scores kept on the device (row layout: include/ntmtrack.h, NTK_SCORE_*).  One thread per slot walks its T
// frames in order and adds to the row clip_of[b] of the table: the head of the row is carried in registers and written back at the
// end, the threshold counts are incremented in place.  The row belongs to this thread alone (two slots never share a row: the
// caller's contract), so a clip's sums are formed in frame order and no atomics are needed.  A slot whose row is outside
// [0, n_clips) reads nothing but clip_of[b].  POLY: the ground truth is a polygon of NTK_POLY_DOUBLES doubles per frame; the
// overlap is poly_iou and the centre distance is taken to the centre of its bounding rectangle.
template <bool POLY>
__global__ void track_overlap_scores_kernel(const double* __restrict__ regions, const double* __restrict__ gt,
                                            const unsigned char* __restrict__ active, const int* __restrict__ clip_of, int T, int B,
                                            int n_clips, const double* __restrict__ iou_thr, int n_iou,
                                            const double* __restrict__ dist_thr, int n_dist, double* __restrict__ table,
                                            double* __restrict__ frame_iou) {
#pragma clang fp contract(off)
    constexpr int GT = POLY ? NTK_POLY_DOUBLES : 4;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const int clip = clip_of[b];
    if (clip < 0 || clip >= n_clips) {
        if (frame_iou)
            for (int t = 0; t < T; ++t) frame_iou[(size_t)t * B + b] = nan;
        return;
    }
    double* row = table + (size_t)clip * (NTK_SCORE_HEAD + n_iou + n_dist);
    double frames = row[NTK_SCORE_FRAMES], sum_iou = row[NTK_SCORE_SUM_IOU], sum_dist = row[NTK_SCORE_SUM_DIST];
    double lost = row[NTK_SCORE_LOST], first_lost = row[NTK_SCORE_FIRST_LOST];
    for (int t = 0; t < T; ++t) {
        const size_t at = (size_t)t * B + b;
        const double* g = gt + GT * at;
        Truth tr;
        const bool scored = (!active || active[at]) && read_truth<POLY>(g, tr);
        if (!scored) {
            if (frame_iou) frame_iou[at] = nan;
            continue;
        }
        const double* p = regions + 4 * at;
        double iou = 0.0;
        if (finite4(p)) {
            const double pw = fmax(p[2], 0.0), ph = fmax(p[3], 0.0);
            iou = truth_iou<POLY>(p[0], p[1], pw, ph, g, tr);
            const double dx = (p[0] + pw / 2) - (tr.x + tr.w / 2), dy = (p[1] + ph / 2) - (tr.y + tr.h / 2);
            const double dist = sqrt(dx * dx + dy * dy);
            sum_dist += dist;
            for (int k = 0; k < n_dist; ++k)
                if (dist <= dist_thr[k]) row[NTK_SCORE_HEAD + n_iou + k] += 1.0;
        }
        if (iou == 0.0) {
            if (first_lost < 0) first_lost = frames;
            lost += 1.0;
        }
        for (int k = 0; k < n_iou; ++k)
            if (iou > iou_thr[k]) row[NTK_SCORE_HEAD + k] += 1.0;
        sum_iou += iou;
        frames += 1.0;
        if (frame_iou) frame_iou[at] = iou;
    }
    row[NTK_SCORE_FRAMES] = frames;
    row[NTK_SCORE_SUM_IOU] = sum_iou;
    row[NTK_SCORE_SUM_DIST] = sum_dist;
    row[NTK_SCORE_LOST] = lost;
    row[NTK_SCORE_FIRST_LOST] = first_lost;
}

// First-frame geometry of the online tracker for the slots that restart on this frame (BatchNTMTracker._first_frame_inputs on the
// device, masked): one thread per slot, float64 in the operation order of ntmtrack/geometry.py, no contraction, so the state
// row, the crop box and the region have the bits of the NumPy path.  The heat-map row is discrete_gauss on the g x g grid about
// the centre of the object box taken through the crop transformation; the exponentials are evaluated three times (maximum, sum,
// values) rather than kept in g * g registers.  A slot that does not restart has its gts0 row zeroed and nothing else written.
__global__ void track_restart_boxes_kernel(const double* __restrict__ regions_in, const unsigned char* __restrict__ restart,
                                           const unsigned char* __restrict__ active, int B, double cropbox_grid, double bbox_grid,
                                           double sigma, int g, double* __restrict__ state, float* __restrict__ cropbox32,
                                           double* __restrict__ regions, float* __restrict__ offsets, int* __restrict__ frame,
                                           float* __restrict__ gts0, unsigned char* __restrict__ run_mask,
                                           unsigned char* __restrict__ move_mask) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const bool rs = restart[b] != 0, act = !active || active[b];
    if (run_mask) run_mask[b] = (rs || act) ? 1 : 0;
    if (move_mask) move_mask[b] = (act && !rs) ? 1 : 0;
    float* hm = gts0 + (size_t)b * g * g;
    if (!rs) {
        for (int i = 0; i < g * g; ++i) hm[i] = 0.f;
        return;
    }
    double* st = state + (size_t)b * NTK_TRACK_STATE_DOUBLES;
    const double* rin = regions_in + 4 * (size_t)b;
    const double x1 = rin[0], y1 = rin[1], rw = rin[2], rh = rin[3];
    const double w = st[NTK_TRACK_STATE_W], h = st[NTK_TRACK_STATE_H];
    const bool normalized = x1 < 1 && y1 < 1 && rw < 1 && rh < 1;
    double n0 = y1, n1 = x1, n2 = y1 + rh, n3 = x1 + rw;
    if (!normalized) {
        const double by = h - 1, bx = w - 1;
        n0 = n0 / by; n1 = n1 / bx; n2 = n2 / by; n3 = n3 / bx;
    }
    const double scale = cropbox_grid / bbox_grid;
    const double cy = (n0 + n2) / 2, cx = (n1 + n3) / 2, hy = (n2 - n0) * scale / 2, hx = (n3 - n1) * scale / 2;
    const double c0 = cy - hy, c1 = cx - hx, c2 = cy + hy, c3 = cx + hx;
    double* nb = st + NTK_TRACK_STATE_BBOX;
    double* ncb = st + NTK_TRACK_STATE_CROPBOX;
    nb[0] = n0; nb[1] = n1; nb[2] = n2; nb[3] = n3;
    ncb[0] = c0; ncb[1] = c1; ncb[2] = c2; ncb[3] = c3;
    float* c32 = cropbox32 + 4 * (size_t)b;
    c32[0] = (float)c0; c32[1] = (float)c1; c32[2] = (float)c2; c32[3] = (float)c3;
    double* rg = regions + 4 * (size_t)b;
    rg[0] = x1; rg[1] = y1; rg[2] = rw; rg[3] = rh;
    offsets[2 * (size_t)b] = 0.f;
    offsets[2 * (size_t)b + 1] = 0.f;
    frame[b] = 0;
    // the object box through the map that sends the crop box to the unit square (rows (sx, 0, -x1 sx) and (0, sy, -y1 sy))
    const double sx = 1.0 / (c3 - c1), sy = 1.0 / (c2 - c0);
    const double tx = -c1 * sx, ty = -c0 * sy;
    const double ux1 = sx * n1 + tx, ux2 = sx * n3 + tx, uy1 = sy * n0 + ty, uy2 = sy * n2 + ty;
    const double mx = (ux1 + ux2) / 2., my = (uy1 + uy2) / 2.;
    const double x0 = 0.5 - mx * g, y0 = 0.5 - my * g, den = 2.0 * sigma * sigma;
    double top = 0.0;
    for (int iy = 0; iy < g; ++iy)
        for (int ix = 0; ix < g; ++ix) {
            const double ys = y0 + iy, xs = x0 + ix;
            top = fmax(top, exp(-(ys * ys + xs * xs) / den));
        }
    const double cut = 2.220446049250313e-16 * top;             // np.finfo(float64).eps * max
    double total = 0.0;
    for (int iy = 0; iy < g; ++iy)
        for (int ix = 0; ix < g; ++ix) {
            const double ys = y0 + iy, xs = x0 + ix;
            const double v = exp(-(ys * ys + xs * xs) / den);
            total += v < cut ? 0.0 : v;
        }
    for (int iy = 0; iy < g; ++iy)
        for (int ix = 0; ix < g; ++ix) {
            const double ys = y0 + iy, xs = x0 + ix;
            double v = exp(-(ys * ys + xs * xs) / den);
            v = v < cut ? 0.0 : v;
            hm[iy * g + ix] = (float)(total != 0 ? v / total : v);
        }
}

// The supervised protocol's state machine (contract: include/ntmtrack.h, NTK_SUP_*), one thread per slot, one frame per call.
// plan decides before the frame's pass what every slot does on it; judge scores the tracked slots after the pass with the one
// overlap of the overlap table and moves a failed slot to WAIT.  The table row belongs to the slot's thread alone.  POLY: the ground
// truth is a polygon, as in track_overlap_scores_kernel.
template <bool POLY>
__global__ void track_supervise_plan_kernel(const double* __restrict__ gt, const unsigned char* __restrict__ active,
                                            const int* __restrict__ clip_of, int B, int n_clips, int* __restrict__ state,
                                            double* __restrict__ table, unsigned char* __restrict__ track,
                                            unsigned char* __restrict__ restart, signed char* __restrict__ codes,
                                            double* __restrict__ frame_iou) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    if (frame_iou) frame_iou[b] = __longlong_as_double(0x7ff8000000000000LL);
    const int clip = clip_of[b];
    unsigned char tr = 0, rs = 0;
    signed char code = NTK_SUP_CODE_INACTIVE;
    if (clip >= 0 && clip < n_clips && (!active || active[b])) {
        int* st = state + (size_t)b * NTK_SUP_STATE_INTS;
        double* row = table + (size_t)clip * NTK_SUP_HEAD;
        if (st[NTK_SUP_STATE_MODE] == NTK_SUP_MODE_TRACK) {
            tr = 1;
            code = NTK_SUP_CODE_TRACKED;
        } else {
            const int left = st[NTK_SUP_STATE_COUNTDOWN] > 1 ? st[NTK_SUP_STATE_COUNTDOWN] - 1 : 0;
            st[NTK_SUP_STATE_COUNTDOWN] = left;
            Truth tr;
            if (left == 0 && read_truth<POLY>(gt + (POLY ? NTK_POLY_DOUBLES : 4) * (size_t)b, tr)) {
                rs = 1;
                code = NTK_SUP_CODE_RESTART;
                row[NTK_SUP_RESTARTS] += 1.0;
                st[NTK_SUP_STATE_MODE] = NTK_SUP_MODE_TRACK;
                st[NTK_SUP_STATE_SINCE] = 0;
            } else {
                code = NTK_SUP_CODE_SKIPPED;
                row[NTK_SUP_SKIPPED] += 1.0;
            }
        }
    }
    track[b] = tr;
    restart[b] = rs;
    if (codes) codes[b] = code;
}

template <bool POLY>
__global__ void track_supervise_judge_kernel(const double* __restrict__ regions, const double* __restrict__ gt,
                                             const unsigned char* __restrict__ track, const int* __restrict__ clip_of, int B,
                                             int n_clips, int skip, int burn_in, double failure_overlap, int* __restrict__ state,
                                             double* __restrict__ table, signed char* __restrict__ codes,
                                             double* __restrict__ frame_iou) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int clip = clip_of[b];
    if (clip < 0 || clip >= n_clips || !track[b]) return;
    int* st = state + (size_t)b * NTK_SUP_STATE_INTS;
    const double* g = gt + (POLY ? NTK_POLY_DOUBLES : 4) * (size_t)b;
    Truth tr;
    if (!read_truth<POLY>(g, tr)) {                          // tracked, the object absent: the frame is counted nowhere
        st[NTK_SUP_STATE_SINCE] += 1;
        if (codes) codes[b] = NTK_SUP_CODE_TRACKED;
        return;
    }
    const double* p = regions + 4 * (size_t)b;
    double iou = 0.0;
    if (finite4(p)) iou = truth_iou<POLY>(p[0], p[1], fmax(p[2], 0.0), fmax(p[3], 0.0), g, tr);
    double* row = table + (size_t)clip * NTK_SUP_HEAD;
    const double tracked = row[NTK_SUP_TRACKED];
    row[NTK_SUP_TRACKED] = tracked + 1.0;
    if (frame_iou) frame_iou[b] = iou;
    if (iou <= failure_overlap) {
        row[NTK_SUP_FAILURES] += 1.0;
        if (row[NTK_SUP_FIRST_FAILURE] < 0) row[NTK_SUP_FIRST_FAILURE] = tracked;
        st[NTK_SUP_STATE_MODE] = NTK_SUP_MODE_WAIT;
        st[NTK_SUP_STATE_COUNTDOWN] = skip;
        if (codes) codes[b] = NTK_SUP_CODE_FAILURE;
        return;
    }
    const int since = st[NTK_SUP_STATE_SINCE] + 1;
    st[NTK_SUP_STATE_SINCE] = since;
    if (since > burn_in) {
        row[NTK_SUP_VALID] += 1.0;
        row[NTK_SUP_SUM_IOU] += iou;
    }
    if (codes) codes[b] = NTK_SUP_CODE_TRACKED;
}

// out[b, :] = mask[b] ? a[b, :] : b_[b, :]   (out may be a or b_: every element is read and written by the same thread)
__global__ void select_rows_kernel(const unsigned char* __restrict__ mask, const float* a, const float* b_, float* out,
                                   size_t total, int n) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    out[idx] = mask[idx / (size_t)n] ? a[idx] : b_[idx];
}

// Masked row copy of several tensors in one launch: for every b with (mask[b] != 0) == keep_where, row b of src[i] is copied to
// row b of dst[i], i < ntensors (rows of rows.n[i] floats).  Grid (chunks, B): workgroup x copies chunk x of the list of all
// tensors' chunks of KEEP_CHUNK floats (rows.first[i] = index of tensor i's first chunk).  A workgroup whose row is not selected
// exits before it reads a table or touches a row.  16-byte loads and stores where the row size and both bases allow, else
// one float per lane.
constexpr int KEEP_CHUNK = 1024;             // floats per workgroup: one 16-byte access per lane; a 512 x 512 link row is 256 workgroups
struct KeepRows {
    long long n[NTK_STATE_KEEP_MAX_TENSORS];
    int first[NTK_STATE_KEEP_MAX_TENSORS + 1];
};

__global__ __launch_bounds__(256) void dnc_state_keep_kernel(const unsigned char* __restrict__ mask, int keep_where, int ntensors,
                                                            const float* const* __restrict__ src, float* const* __restrict__ dst,
                                                            KeepRows rows) {
    const int b = blockIdx.y;
    if ((mask[b] != 0) != (keep_where != 0)) return;
    int i = 0;
    while (i + 1 < ntensors && (int)blockIdx.x >= rows.first[i + 1]) ++i;
    const long long n = rows.n[i];
    const long long off = (long long)((int)blockIdx.x - rows.first[i]) * KEEP_CHUNK;
    const int len = (int)(n - off < KEEP_CHUNK ? n - off : KEEP_CHUNK);
    const float* s = src[i] + (size_t)b * (size_t)n + (size_t)off;
    float* d = dst[i] + (size_t)b * (size_t)n + (size_t)off;
    if ((n & 3) == 0 && ((((uintptr_t)s) | ((uintptr_t)d)) & 15u) == 0) {
        for (int j = 4 * (int)threadIdx.x; j < len; j += 4 * 256)
            *reinterpret_cast<float4*>(d + j) = *reinterpret_cast<const float4*>(s + j);
    } else {
        for (int j = (int)threadIdx.x; j < len; j += 256) d[j] = s[j];
    }
}

// tf.image.resize_images(..., BILINEAR) with TF-1 defaults: one thread per output element (resize_bilinear_pixel)
__global__ void resize_bilinear_kernel(const float* __restrict__ img, int H, int W, int C, float* __restrict__ out,
                                       int OH, int OW) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)OH * OW * C) return;
    const int c = (int)(idx % C), x = (int)((idx / C) % OW), y = (int)(idx / ((size_t)C * OW));
    out[idx] = resize_bilinear_pixel(DenseImage<float>{img, W, C}, H, W, OH, OW, y, x, c);
}

extern "C" int ntk_resize_bilinear(const float* image, int H, int W, int C, float* out, int out_h, int out_w, void* stream) {
    NTK_REQUIRE(image && out, NTK_ERR_BAD_PTR, "ntk_resize_bilinear: null pointer");
    NTK_REQUIRE(H > 0 && W > 0 && C > 0 && out_h > 0 && out_w > 0, NTK_ERR_BAD_SHAPE, "ntk_resize_bilinear: %dx%dx%d -> %dx%d", H, W, C, out_h, out_w);
    const size_t total = (size_t)out_h * out_w * C;
    resize_bilinear_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(image, H, W, C, out, out_h, out_w);
    NTK_CHECK_LAUNCH("ntk_resize_bilinear");
    return NTK_OK;
}

extern "C" int ntk_crop_and_resize(const float* image, int H, int W, int C, const float* mean, float y1, float x1,
                                   float y2, float x2, float* out, int crop_h, int crop_w, float extrapolation,
                                   void* stream) {
    NTK_REQUIRE(image && out, NTK_ERR_BAD_PTR, "ntk_crop_and_resize: null pointer");
    NTK_REQUIRE(H > 0 && W > 0 && C > 0 && crop_h > 0 && crop_w > 0, NTK_ERR_BAD_SHAPE,
                "ntk_crop_and_resize: H=%d W=%d C=%d crop=%dx%d", H, W, C, crop_h, crop_w);
    const long total = (long)crop_h * crop_w * C;
    NTK_REQUIRE(total < 2147483647L - 256, NTK_ERR_BAD_SHAPE, "ntk_crop_and_resize: crop=%dx%d C=%d: too many elements", crop_h, crop_w, C);
    crop_resize_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(image, H, W, C, mean, y1, x1, y2, x2, out,
                                                                             crop_h, crop_w, extrapolation);
    NTK_CHECK_LAUNCH("ntk_crop_and_resize");
    return NTK_OK;
}

extern "C" int ntk_crop_and_resize_batch(const void* images, int dtype, int F, int H, int W, int C, const int* frame_of,
                                         const float* boxes, const float* mean, float* out, int B, int crop_h, int crop_w,
                                         float extrapolation, void* stream) {
    NTK_REQUIRE(images && frame_of && boxes && out, NTK_ERR_BAD_PTR, "ntk_crop_and_resize_batch: null pointer");
    NTK_REQUIRE(dtype == NTK_IMAGE_F32 || dtype == NTK_IMAGE_U8, NTK_ERR_BAD_SHAPE,
                "ntk_crop_and_resize_batch: dtype=%d (NTK_IMAGE_F32 or NTK_IMAGE_U8)", dtype);
    NTK_REQUIRE(B > 0 && B <= 65535 && F > 0 && H > 0 && W > 0 && C > 0 && crop_h > 0 && crop_w > 0, NTK_ERR_BAD_SHAPE,
                "ntk_crop_and_resize_batch: B=%d (1..65535) F=%d H=%d W=%d C=%d crop=%dx%d", B, F, H, W, C, crop_h, crop_w);
    const long total = (long)crop_h * crop_w * C;
    NTK_REQUIRE(total < 2147483647L - 256, NTK_ERR_BAD_SHAPE, "ntk_crop_and_resize_batch: crop=%dx%d C=%d: too many elements per box",
                crop_h, crop_w, C);
    const dim3 grid((unsigned)((total + 255) / 256), (unsigned)B);
    if (dtype == NTK_IMAGE_U8)
        crop_resize_batch_kernel<unsigned char><<<grid, 256, 0, (hipStream_t)stream>>>(
            (const unsigned char*)images, F, H, W, C, frame_of, boxes, mean, out, crop_h, crop_w, extrapolation);
    else
        crop_resize_batch_kernel<float><<<grid, 256, 0, (hipStream_t)stream>>>((const float*)images, F, H, W, C, frame_of, boxes, mean,
                                                                               out, crop_h, crop_w, extrapolation);
    NTK_CHECK_LAUNCH("ntk_crop_and_resize_batch");
    return NTK_OK;
}

extern "C" int ntk_frames_crop_batch(const unsigned char* pixels, long long pixels_bytes, const long long* frame_table,
                                     const float* boxes, const float* mean, float* out, int n, int C, int resize_h, int resize_w,
                                     int crop_h, int crop_w, int flip_x, float extrapolation, void* stream) {
    NTK_REQUIRE(pixels && frame_table && boxes && out, NTK_ERR_BAD_PTR, "ntk_frames_crop_batch: null pointer");
    NTK_REQUIRE(n > 0 && n <= 65535 && C > 0 && C <= 4 && resize_h > 0 && resize_w > 0 && crop_h > 0 && crop_w > 0 && pixels_bytes > 0,
                NTK_ERR_BAD_SHAPE, "ntk_frames_crop_batch: n=%d (1..65535) C=%d (1..4) resize=%dx%d crop=%dx%d pixels_bytes=%lld", n, C,
                resize_h, resize_w, crop_h, crop_w, pixels_bytes);
    const long total = (long)crop_h * crop_w * C;
    NTK_REQUIRE(total < 2147483648L - 256, NTK_ERR_BAD_SHAPE, "ntk_frames_crop_batch: crop=%dx%d C=%d: too many elements per frame",
                crop_h, crop_w, C);
    const dim3 grid((unsigned)(((long)crop_h * crop_w + 255) / 256), (unsigned)n);
    frames_crop_batch_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(pixels, pixels_bytes, frame_table, boxes, mean, out, C, resize_h,
                                                                    resize_w, crop_h, crop_w, flip_x ? 1 : 0, extrapolation);
    NTK_CHECK_LAUNCH("ntk_frames_crop_batch");
    return NTK_OK;
}

extern "C" int ntk_track_boxes_update(const float* logits, int B, int S, double cropbox_grid, double bbox_grid,
                                      const unsigned char* active, double* state, float* cropbox32, double* regions,
                                      float* offsets, int* frame, void* stream) {
    NTK_REQUIRE(logits && state && cropbox32 && regions && offsets, NTK_ERR_BAD_PTR, "ntk_track_boxes_update: null pointer");
    NTK_REQUIRE(B > 0 && S > 0 && cropbox_grid > 0 && bbox_grid > 0, NTK_ERR_BAD_SHAPE,
                "ntk_track_boxes_update: B=%d S=%d cropbox_grid=%g bbox_grid=%g", B, S, cropbox_grid, bbox_grid);
    track_boxes_update_kernel<<<(B + 63) / 64, 64, 0, (hipStream_t)stream>>>(logits, B, S, cropbox_grid, bbox_grid, active, state,
                                                                            cropbox32, regions, offsets, frame);
    NTK_CHECK_LAUNCH("ntk_track_boxes_update");
    return NTK_OK;
}

template <bool POLY>
static int track_overlap_scores(const char* name, const double* regions, const double* gt, const unsigned char* active,
                                const int* clip_of, int T, int B, int n_clips, const double* iou_thr, int n_iou,
                                const double* dist_thr, int n_dist, double* table, double* frame_iou, void* stream) {
    NTK_REQUIRE(regions && gt && clip_of && table, NTK_ERR_BAD_PTR, "%s: null pointer", name);
    NTK_REQUIRE(T > 0 && B > 0 && B <= 65535 && n_clips > 0, NTK_ERR_BAD_SHAPE, "%s: T=%d B=%d (1..65535) n_clips=%d", name, T, B, n_clips);
    NTK_REQUIRE(n_iou >= 0 && n_iou <= NTK_SCORE_MAX_THRESHOLDS && n_dist >= 0 && n_dist <= NTK_SCORE_MAX_THRESHOLDS, NTK_ERR_BAD_SHAPE,
                "%s: n_iou=%d n_dist=%d (0..%d each)", name, n_iou, n_dist, NTK_SCORE_MAX_THRESHOLDS);
    NTK_REQUIRE((n_iou == 0 || iou_thr) && (n_dist == 0 || dist_thr), NTK_ERR_BAD_SHAPE, "%s: n_iou=%d n_dist=%d but %s is null", name,
                n_iou, n_dist, (n_iou > 0 && !iou_thr) ? "iou_thr" : "dist_thr");
    track_overlap_scores_kernel<POLY><<<(B + 63) / 64, 64, 0, (hipStream_t)stream>>>(regions, gt, active, clip_of, T, B, n_clips, iou_thr,
                                                                                    n_iou, dist_thr, n_dist, table, frame_iou);
    NTK_CHECK_LAUNCH(name);
    return NTK_OK;
}

extern "C" int ntk_track_overlap_scores(const double* regions, const double* gt, const unsigned char* active, const int* clip_of,
                                        int T, int B, int n_clips, const double* iou_thr, int n_iou, const double* dist_thr,
                                        int n_dist, double* table, double* frame_iou, void* stream) {
    return track_overlap_scores<false>("ntk_track_overlap_scores", regions, gt, active, clip_of, T, B, n_clips, iou_thr, n_iou, dist_thr,
                                       n_dist, table, frame_iou, stream);
}

extern "C" int ntk_track_overlap_scores_poly(const double* regions, const double* gt, const unsigned char* active, const int* clip_of,
                                             int T, int B, int n_clips, const double* iou_thr, int n_iou, const double* dist_thr,
                                             int n_dist, double* table, double* frame_iou, void* stream) {
    return track_overlap_scores<true>("ntk_track_overlap_scores_poly", regions, gt, active, clip_of, T, B, n_clips, iou_thr, n_iou,
                                      dist_thr, n_dist, table, frame_iou, stream);
}

extern "C" int ntk_track_poly_bounds(const double* poly, int n, double* rects, void* stream) {
    NTK_REQUIRE(poly && rects, NTK_ERR_BAD_PTR, "ntk_track_poly_bounds: null pointer");
    NTK_REQUIRE(n > 0, NTK_ERR_BAD_SHAPE, "ntk_track_poly_bounds: n=%d", n);
    track_poly_bounds_kernel<<<(n + 63) / 64, 64, 0, (hipStream_t)stream>>>(poly, n, rects);
    NTK_CHECK_LAUNCH("ntk_track_poly_bounds");
    return NTK_OK;
}

extern "C" int ntk_track_restart_boxes(const double* regions_in, const unsigned char* restart, const unsigned char* active, int B,
                                       double cropbox_grid, double bbox_grid, double sigma, int gts_width, double* state,
                                       float* cropbox32, double* regions, float* offsets, int* frame, float* gts0,
                                       unsigned char* run_mask, unsigned char* move_mask, void* stream) {
    NTK_REQUIRE(regions_in && restart && state && cropbox32 && regions && offsets && frame && gts0, NTK_ERR_BAD_PTR,
                "ntk_track_restart_boxes: null pointer");
    NTK_REQUIRE(B > 0 && B <= 65535, NTK_ERR_BAD_SHAPE, "ntk_track_restart_boxes: B=%d (1..65535)", B);
    NTK_REQUIRE(cropbox_grid > 0 && bbox_grid > 0 && sigma > 0, NTK_ERR_BAD_SHAPE,
                "ntk_track_restart_boxes: cropbox_grid=%g bbox_grid=%g sigma=%g", cropbox_grid, bbox_grid, sigma);
    const int g = cropbox_grid <= 1024 ? (int)cropbox_grid : 0;
    NTK_REQUIRE(g >= 1 && (double)g == cropbox_grid && g * g == gts_width, NTK_ERR_BAD_SHAPE,
                "ntk_track_restart_boxes: gts_width=%d for cropbox_grid=%g (a whole number up to 1024, gts_width its square)",
                gts_width, cropbox_grid);
    track_restart_boxes_kernel<<<(B + 63) / 64, 64, 0, (hipStream_t)stream>>>(regions_in, restart, active, B, cropbox_grid, bbox_grid,
                                                                             sigma, g, state, cropbox32, regions, offsets, frame,
                                                                             gts0, run_mask, move_mask);
    NTK_CHECK_LAUNCH("ntk_track_restart_boxes");
    return NTK_OK;
}

template <bool POLY>
static int track_supervise(const char* name, int phase, const double* regions, const double* gt, const unsigned char* active,
                           const int* clip_of, int B, int n_clips, int skip, int burn_in, double failure_overlap, int* state,
                           double* table, unsigned char* track, unsigned char* restart, signed char* codes, double* frame_iou,
                           void* stream) {
    NTK_REQUIRE(phase == NTK_SUP_PLAN || phase == NTK_SUP_JUDGE, NTK_ERR_BAD_SHAPE, "%s: phase=%d (NTK_SUP_PLAN or NTK_SUP_JUDGE)", name,
                phase);
    NTK_REQUIRE(gt && clip_of && state && table && track && (phase == NTK_SUP_PLAN ? restart != nullptr : regions != nullptr),
                NTK_ERR_BAD_PTR, "%s: null pointer", name);
    NTK_REQUIRE(B > 0 && B <= 65535 && n_clips > 0, NTK_ERR_BAD_SHAPE, "%s: B=%d (1..65535) n_clips=%d", name, B, n_clips);
    NTK_REQUIRE(skip >= 1 && burn_in >= 0 && failure_overlap >= 0 && failure_overlap < 1, NTK_ERR_BAD_SHAPE,
                "%s: skip=%d (>= 1) burn_in=%d (>= 0) failure_overlap=%g (in [0,1))", name, skip, burn_in, failure_overlap);
    if (phase == NTK_SUP_PLAN)
        track_supervise_plan_kernel<POLY><<<(B + 63) / 64, 64, 0, (hipStream_t)stream>>>(gt, active, clip_of, B, n_clips, state, table,
                                                                                        track, restart, codes, frame_iou);
    else
        track_supervise_judge_kernel<POLY><<<(B + 63) / 64, 64, 0, (hipStream_t)stream>>>(regions, gt, track, clip_of, B, n_clips, skip,
                                                                                         burn_in, failure_overlap, state, table, codes,
                                                                                         frame_iou);
    NTK_CHECK_LAUNCH(name);
    return NTK_OK;
}

extern "C" int ntk_track_supervise(int phase, const double* regions, const double* gt, const unsigned char* active,
                                   const int* clip_of, int B, int n_clips, int skip, int burn_in, double failure_overlap,
                                   int* state, double* table, unsigned char* track, unsigned char* restart, signed char* codes,
                                   double* frame_iou, void* stream) {
    return track_supervise<false>("ntk_track_supervise", phase, regions, gt, active, clip_of, B, n_clips, skip, burn_in, failure_overlap,
                                  state, table, track, restart, codes, frame_iou, stream);
}

extern "C" int ntk_track_supervise_poly(int phase, const double* regions, const double* gt, const unsigned char* active,
                                        const int* clip_of, int B, int n_clips, int skip, int burn_in, double failure_overlap,
                                        int* state, double* table, unsigned char* track, unsigned char* restart, signed char* codes,
                                        double* frame_iou, void* stream) {
    return track_supervise<true>("ntk_track_supervise_poly", phase, regions, gt, active, clip_of, B, n_clips, skip, burn_in,
                                 failure_overlap, state, table, track, restart, codes, frame_iou, stream);
}

extern "C" int ntk_select_rows(const unsigned char* mask, const float* a, const float* b, float* out, int B, int n, void* stream) {
    NTK_REQUIRE(mask && a && b && out, NTK_ERR_BAD_PTR, "ntk_select_rows: null pointer");
    NTK_REQUIRE(B > 0 && n > 0, NTK_ERR_BAD_SHAPE, "ntk_select_rows: B=%d n=%d", B, n);
    const size_t total = (size_t)B * n;
    NTK_REQUIRE((total + 255) / 256 < 2147483647UL, NTK_ERR_BAD_SHAPE, "ntk_select_rows: B=%d n=%d: too many elements", B, n);
    select_rows_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(mask, a, b, out, total, n);
    NTK_CHECK_LAUNCH("ntk_select_rows");
    return NTK_OK;
}

extern "C" int ntk_dnc_state_keep(const unsigned char* mask, int keep_where, int B, int ntensors, const float* const* src,
                                  float* const* dst, const long long* row_floats, void* stream) {
    NTK_REQUIRE(mask && src && dst && row_floats, NTK_ERR_BAD_PTR, "ntk_dnc_state_keep: null pointer");
    NTK_REQUIRE(B >= 1 && B <= 65535, NTK_ERR_BAD_SHAPE, "ntk_dnc_state_keep: B=%d (1..65535)", B);
    NTK_REQUIRE(ntensors >= 1 && ntensors <= NTK_STATE_KEEP_MAX_TENSORS, NTK_ERR_BAD_SHAPE, "ntk_dnc_state_keep: ntensors=%d (1..%d)",
                ntensors, NTK_STATE_KEEP_MAX_TENSORS);
    KeepRows rows = {};
    long long chunks = 0;
    for (int i = 0; i < ntensors; ++i) {
        NTK_REQUIRE(row_floats[i] >= 0, NTK_ERR_BAD_SHAPE, "ntk_dnc_state_keep: row_floats[%d]=%lld", i, row_floats[i]);
        rows.n[i] = row_floats[i];
        rows.first[i] = (int)chunks;
        chunks += (row_floats[i] + KEEP_CHUNK - 1) / KEEP_CHUNK;
        NTK_REQUIRE(chunks < 2147483647LL, NTK_ERR_BAD_SHAPE, "ntk_dnc_state_keep: row_floats[%d]=%lld: too many elements per row", i,
                    row_floats[i]);
    }
    rows.first[ntensors] = (int)chunks;
    if (chunks == 0) return NTK_OK;
    dnc_state_keep_kernel<<<dim3((unsigned)chunks, (unsigned)B), 256, 0, (hipStream_t)stream>>>(mask, keep_where, ntensors, src, dst, rows);
    NTK_CHECK_LAUNCH("ntk_dnc_state_keep");
    return NTK_OK;
}

extern "C" int ntk_offset_loss(const float* logits, const float* offsets, float* pred, float* loss,
                               float* dlogits, int B, int T, int NF, int O, void* stream) {
    NTK_REQUIRE(logits && offsets && (loss || dlogits), NTK_ERR_BAD_PTR, "ntk_offset_loss: null pointer");
    NTK_REQUIRE(B > 0 && T >= 2 && NF > 0 && O > 0, NTK_ERR_BAD_SHAPE, "ntk_offset_loss: B=%d T=%d NF=%d O=%d (T >= 2)", B, T, NF, O);
    offset_loss_kernel<<<1, 1024, 0, (hipStream_t)stream>>>(logits, offsets, pred, loss, dlogits, B, T, NF, O);
    NTK_CHECK_LAUNCH("ntk_offset_loss");
    return NTK_OK;
}

extern "C" int ntk_log_loss(const float* logits, const float* labels, float* loss, float* dlogits, int n, void* stream) {
    NTK_REQUIRE(logits && labels && loss, NTK_ERR_BAD_PTR, "ntk_log_loss: null pointer");
    NTK_REQUIRE(n > 0, NTK_ERR_BAD_SHAPE, "ntk_log_loss: n=%d", n);
    log_loss_kernel<<<1, 1024, 0, (hipStream_t)stream>>>(logits, labels, loss, dlogits, n);
    NTK_CHECK_LAUNCH("ntk_log_loss");
    return NTK_OK;
}

extern "C" int ntk_serialize_sequential(const float* fmap, const float* gts0, float* X, int B, int T, int F, int C, int ldx,
                                        void* stream) {
    NTK_REQUIRE(fmap && X, NTK_ERR_BAD_PTR, "ntk_serialize_sequential: null pointer");
    NTK_REQUIRE(B > 0 && T > 0 && F > 0 && C > 0 && (C % 4) == 0 && ldx >= C + 3 && (ldx % 4) == 0, NTK_ERR_BAD_SHAPE,
                "ntk_serialize_sequential: B=%d T=%d F=%d C=%d (multiple of 4) ldx=%d (>= C + 3, multiple of 4)", B, T, F, C, ldx);
    NTK_REQUIRE(ntk_aligned16(fmap) && ntk_aligned16(X), NTK_ERR_BAD_PTR, "ntk_serialize_sequential: 16-byte alignment");
    const long rows = (long)B * (F + (long)(T - 1) * (2 * F + 1));
    NTK_REQUIRE(rows < 2147483647L, NTK_ERR_BAD_SHAPE, "ntk_serialize_sequential: too many rows");
    serialize_sequential_kernel<<<(unsigned)rows, 128, 0, (hipStream_t)stream>>>(fmap, gts0, X, T, F, C, ldx);
    NTK_CHECK_LAUNCH("ntk_serialize_sequential");
    return NTK_OK;
}

extern "C" int ntk_heatmap_ce_loss(const float* logits, const float* gt, float* probs, float* loss, float* dlogits,
                                   int B, int T, int F, void* stream) {
    NTK_REQUIRE(logits && gt && (loss || dlogits || probs), NTK_ERR_BAD_PTR, "ntk_heatmap_ce_loss: null pointer");
    NTK_REQUIRE(B > 0 && T >= 2 && F > 0, NTK_ERR_BAD_SHAPE, "ntk_heatmap_ce_loss: B=%d T=%d (>= 2) F=%d", B, T, F);
    heatmap_ce_loss_kernel<<<1, 1024, 0, (hipStream_t)stream>>>(logits, gt, probs, loss, dlogits, B, T, F);
    NTK_CHECK_LAUNCH("ntk_heatmap_ce_loss");
    return NTK_OK;
}

extern "C" int ntk_serialize_two_step(const float* feat, const float* target, float* X, int B, int T, int D, int F, int ldx,
                                      void* stream) {
    NTK_REQUIRE(feat && X, NTK_ERR_BAD_PTR, "ntk_serialize_two_step: null pointer");
    NTK_REQUIRE(B > 0 && T >= 1 && D > 0 && F > 0 && ldx >= 1 + D + F, NTK_ERR_BAD_SHAPE,
                "ntk_serialize_two_step: B=%d T=%d D=%d F=%d ldx=%d (>= 1 + D + F)", B, T, D, F, ldx);
    const size_t total = (size_t)B * (2 * T - 1) * ldx;
    const unsigned nb = (unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    serialize_two_step_kernel<<<nb, 256, 0, (hipStream_t)stream>>>(feat, target, X, B, T, D, F, ldx);
    NTK_CHECK_LAUNCH("ntk_serialize_two_step");
    return NTK_OK;
}

extern "C" int ntk_two_step_ce_loss(const float* logits, const float* gt, float* probs, float* loss, float* dlogits,
                                    int B, int T, int F, void* stream) {
    NTK_REQUIRE(logits && gt && (loss || dlogits || probs), NTK_ERR_BAD_PTR, "ntk_two_step_ce_loss: null pointer");
    NTK_REQUIRE(B > 0 && T >= 1 && F > 0, NTK_ERR_BAD_SHAPE, "ntk_two_step_ce_loss: B=%d T=%d F=%d", B, T, F);
    two_step_ce_loss_kernel<<<1, 1024, 0, (hipStream_t)stream>>>(logits, gt, probs, loss, dlogits, B, T, F);
    NTK_CHECK_LAUNCH("ntk_two_step_ce_loss");
    return NTK_OK;
}

extern "C" int ntk_ntm_init_state(const float* v, float* out, int n, int B, int act, void* stream) {
    NTK_REQUIRE(v && out, NTK_ERR_BAD_PTR, "ntk_ntm_init_state: null pointer");
    NTK_REQUIRE(n > 0 && B > 0 && (act == 0 || act == 1), NTK_ERR_BAD_SHAPE, "ntk_ntm_init_state: n=%d B=%d act=%d", n, B, act);
    init_state_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(v, out, n, B, act);
    NTK_CHECK_LAUNCH("ntk_ntm_init_state");
    return NTK_OK;
}

extern "C" int ntk_ntm_init_state_bwd(const float* v, const float* dout, float* dv, int n, int B, int act,
                                      int accumulate, void* stream) {
    NTK_REQUIRE(v && dout && dv, NTK_ERR_BAD_PTR, "ntk_ntm_init_state_bwd: null pointer");
    NTK_REQUIRE(n > 0 && B > 0 && (act == 0 || act == 1), NTK_ERR_BAD_SHAPE, "ntk_ntm_init_state_bwd: n=%d B=%d act=%d", n, B, act);
    init_state_bwd_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(v, dout, dv, n, B, act, accumulate);
    NTK_CHECK_LAUNCH("ntk_ntm_init_state_bwd");
    return NTK_OK;
}

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
