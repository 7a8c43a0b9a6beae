/*
 * ntmtrack.h -- C ABI of libntmtrack_hip.so (MI355X / gfx950 only).
 *
 * Drop-in boundary for the per-frame tracking hot path of
 * JeffOwOSun/ntm-tracker.  The reference is pure Python/TensorFlow-1 and has
 * no FFI of its own; each entry point below names the reference op group
 * (file:line in the reference tree) it replaces, and INTEGRATION.md shows the
 * ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is caller-owned DEVICE memory (fp32 unless noted);
 *     nothing is allocated, freed or retained by the library;
 *   - `stream` is a hipStream_t passed as void*; all work is asynchronous and
 *     ordered on that stream; no host synchronisation happens inside;
 *   - return value: NTK_OK (0) or a negative NTK_ERR_* code;
 *     ntk_last_error() returns a thread-local description of the last failure;
 *   - shapes are validated on the host before any launch: a bad shape is
 *     refused (NTK_ERR_BAD_SHAPE / NTK_ERR_UNSUPPORTED), never launched;
 *   - stateless and re-entrant: no mutable process-global switches; the only
 *     global state is a per-device cache of one-time kernel attributes.
 */
#ifndef NTMTRACK_H_
#define NTMTRACK_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NTK_OK               0
#define NTK_ERR_BAD_SHAPE   -1
#define NTK_ERR_BAD_PTR     -2
#define NTK_ERR_UNSUPPORTED -3
#define NTK_ERR_HIP         -4

/* library version (major*10000 + minor*100 + patch) and last error text */
int ntk_version(void);
const char* ntk_last_error(void);

/* ------------------------------------------------------------------------
 * VGG-16 feature extractor, conv1_1 .. conv4_3
 * replaces: frozen GraphDef import, direct_offset_output.py:417-422
 *           (layer spec vgg.py:155-161, arg scope vgg.py:49-63)
 * --------------------------------------------------------------------- */

/* Repack TF HWIO weights [3,3,Cin,Cout] into the kernel's [Cout][Kp] layout,
 * Kp = ntk_vgg_packed_k(Cin) (zero padded); for Cin % 32 == 0 the K order is
 * 32-channel chunk outer / tap inner: k = (c/32)*288 + (ky*3+kx)*32 + c%32;
 * for Cin = 3: k = (ky*3+kx)*Cin + c. */
int ntk_vgg_packed_k(int cin);
int ntk_vgg_pack_weights(const float* w_hwio, float* w_packed, int cin, int cout, void* stream);

/* out = relu(conv3x3_same(in, w) + bias), NHWC fp32; optional fused 2x2/2
 * max-pool (vgg.py:156,158,160).  in [frames,H,W,Cin]; out [frames,H,W,Cout]
 * or [frames,H/2,W/2,Cout] when fuse_pool.  H, W multiples of 4; Cin == 3 or
 * a multiple of 32; Cout a multiple of 64.  MFMA v_mfma_f32_32x32x2_f32. */
int ntk_vgg_conv3x3_relu_f32(const float* in, const float* w_packed, const float* bias,
                             float* out, int frames, int H, int W, int cin, int cout,
                             int fuse_pool, void* stream);

/* bf16 trunk (BASELINE config 5: "bf16 MFMA conv + fp32 memory"): bf16 NHWC activations and weights, fp32
 * accumulation (v_mfma_f32_32x32x16_bf16), output rounded once to bf16 (or kept fp32 when out_f32, for the
 * last layer feeding the memory cell).  Cin a multiple of 64.  Packed weights: bf16 [Cout][9*Cin],
 * k = (c/64)*576 + (ky*3+kx)*64 + c%64.  conv1_1 (Cin = 3) runs the fp32 kernel on the fp32 frames and
 * stores bf16 (ntk_vgg_conv3x3_relu_f32_to_bf16, fp32 packed weights from ntk_vgg_pack_weights). */
int ntk_vgg_pack_weights_bf16(const float* w_hwio, void* w_packed_bf16, int cin, int cout, void* stream);
int ntk_vgg_conv3x3_relu_bf16(const void* in_bf16, const void* w_packed_bf16, const float* bias, void* out,
                              int frames, int H, int W, int cin, int cout, int fuse_pool, int out_f32,
                              void* stream);
/* The same operator in PATCH form (csrc/conv_bf16p.hip, round 4): the input of a block of 512 output pixels is staged once per
 * channel chunk as a patch with its halo and serves all nine taps; weights go through LDS once per workgroup; everything moves by
 * LDS-DMA.  Takes frames whose sides are multiples of 4 (of 8 with the fused pool), cin a multiple of 32, cout of 64
 * (ntk_vgg_bf16p_supported says so for a shape; ntk_vgg_conv3x3_relu_bf16 runs the others).  The weights are packed per layer
 * AND frame shape (ntk_vgg_pack_weights_bf16p: the chunk size depends on H, W): 9 * cin * cout bf16 elements.  Same operand
 * rounding, accumulation type and output rounding as ntk_vgg_conv3x3_relu_bf16; the summation order differs. */
size_t ntk_vgg_bf16p_packed_elems(int cin, int cout);
int ntk_vgg_bf16p_supported(int H, int W, int cin, int cout, int fuse_pool);
int ntk_vgg_pack_weights_bf16p(const float* w_hwio, void* w_packed_bf16, int cin, int cout, int H, int W, void* stream);
int ntk_vgg_conv3x3_relu_bf16p(const void* in_bf16, const void* w_packed_bf16p, const float* bias, void* out,
                               int frames, int H, int W, int cin, int cout, int fuse_pool, int out_f32, void* stream);
int ntk_vgg_conv3x3_relu_f32_to_bf16(const float* in, const float* w_packed, const float* bias, void* out_bf16,
                                     int frames, int H, int W, int cin, int cout, void* stream);

/* The SPLIT form of the fp32 trunk (csrc/conv_bf16p.hip, template flag X3; round 4): the same fp32 operator (vgg.py:155-161) on the
 * fp16 matrix pipe.  Every fp32 value v travels as two fp16 numbers, hi = fp16(v) rounded toward zero and lo = fp16(v - hi) rounded to
 * nearest; a product x w is accumulated in fp32 as xh wh + xh wl + xl wh (per layer 0.7e-6 .. 1.7e-6 of the activation scale).
 * PRECISION of the parts: an activation v = hi + lo to 2^-22 |v| for 2^-3 <= |v| <= 65504; below 2^-3 lo is an fp16 subnormal and the
 * error is an ABSOLUTE 2^-25 (a map, or a channel, whose values are all small keeps fewer bits: at 2^-16 of unit scale, 2^-9 relative --
 * activations have no scale of their own); from 65504 to 131008 hi is 65504 and lo carries the rest at fp16's spacing there (up to 16).
 * A weight is exact to 2^-22 |w| down to 2^-17 of the layer's largest (one power-of-two scale per layer), to 2^-38 of the largest
 * below.  The matrix pipe keeps fp16 subnormal operands (measured, profiles/conv_values.txt).  The weights are scaled by a power of
 * two when packed (exact; the epilogue multiplies the sums by the inverse).
 * A split map is [frames][H][W][C / 16][2][16] fp16 (hi x16 | lo x16 per group of 16 channels: the bytes of the fp32 map).  Larger
 * activations saturate at 131008 instead of overflowing: on the way in (a split map holds no more; the staging of an fp32 map
 * clamps) and in the epilogue that writes a split map.  An fp32 OUTPUT (out_f32 = 1) is not clamped: sums beyond 131008 are written
 * as they are.
 * Shapes (ntk_vgg_split3_supported): H, W multiples of 8, or W = 28 with H >= 20 and no pool (runs of rows); cin a multiple of 16, cout
 * of 64.  Packed weights: ntk_vgg_split3_packed_elems(cin, cout) = 18 * cin * cout + 8 fp16 elements, packed per layer and frame shape:
 * the hi / lo parts, then a 16-byte tail the packing writes its scales into -- size the buffer with ntk_vgg_split3_packed_elems
 * (18 * cin * cout elements are 16 bytes short).  out_f32 = 1 writes fp32 NHWC (where the trunk leaves the split form); in_f32 = 1 reads
 * an fp32 NHWC map and splits it while staging (where the trunk enters it: cin <= 64, cout = 64, H and W multiples of 8 only). */
size_t ntk_vgg_split3_packed_elems(int cin, int cout);
int ntk_vgg_split3_supported(int H, int W, int cin, int cout, int fuse_pool);
int ntk_vgg_pack_weights_split3(const float* w_hwio, void* w_packed, int cin, int cout, int H, int W, void* stream);
int ntk_vgg_conv3x3_relu_split3(const void* in_split, const void* w_packed, const float* bias, void* out,
                                int frames, int H, int W, int cin, int cout, int fuse_pool, int in_f32, int out_f32, void* stream);

/* The fused stem: conv1_1 (3 -> 64) computed inside the staging of conv1_2 (64 -> 64, split form), so that conv1_1's
 * [frames][H][W][64] fp32 map is neither written nor read.  frames_f32: [frames][H][W][3] fp32; w1_packed / bias1: conv1_1's weights as
 * ntk_vgg_pack_weights(cin 3, cout 64) packs them ([64][32], k = tap * 3 + c) and its 64 biases; w2_packed / bias2: conv1_2's weights
 * from ntk_vgg_pack_weights_split3(cin 64, cout 64, H, W) and its biases; out as ntk_vgg_conv3x3_relu_split3 (a split map, or fp32 NHWC
 * with out_f32 = 1; H/2 x W/2 with fuse_pool).  conv1_1 is evaluated in fp32 (fp32 MFMAs over k in order, + bias, ReLU) on every pixel
 * of a sub-block and its one-pixel halo, clamped and split exactly as an fp32 input map is (in_f32 = 1 above); halo pixels outside the
 * frame are zero (conv1_2's padding).  Results: bit for bit those of ntk_vgg_conv3x3_relu_f32 + ntk_vgg_conv3x3_relu_split3(in_f32 = 1)
 * where W is a multiple of 32 (conv1_1's row kernel sums in the same order); equal to fp32 rounding of conv1_1 elsewhere.  Shapes
 * (ntk_vgg_split3_stem_supported): H, W multiples of 8; sub-blocks of 32x8 and 16x16 run two workgroups per CU, 8x8 (H or W not a
 * multiple of 16) one.  w2_packed, bias2 and out 16-byte aligned. */
int ntk_vgg_split3_stem_supported(int H, int W, int fuse_pool);
int ntk_vgg_conv3x3_relu_split3_stem(const float* frames_f32, const float* w1_packed, const float* bias1, const void* w2_packed,
                                     const float* bias2, void* out, int frames, int H, int W, int fuse_pool, int out_f32, void* stream);

/* The same operator by fused Winograd F(2x2,3x3) on the fp32 MFMA pipe (2.25x fewer multiplies; results equal to
 * ntk_vgg_conv3x3_relu_f32 up to rounding, ~1e-6 relative per layer).  Weights: U = G g G^T for the 16 transform
 * planes, packed lane-major for the MFMA B operand (ntk_vgg_wino_packed_floats(cin, cout) = 16*cin*cout floats).
 * cin a multiple of 16 and at most 1024, cout a multiple of 64 (64, 128, 256 or a multiple of 512); H and W multiples
 * of 4.  ntk_vgg_wino_supported: 1 for a layer shape the entry takes (the entry's own decision, from shapes alone). */
size_t ntk_vgg_wino_packed_floats(int cin, int cout);
int ntk_vgg_wino_supported(int frames, int H, int W, int cin, int cout);
int ntk_vgg_pack_weights_wino(const float* w_hwio, float* u_packed, int cin, int cout, void* stream);
int ntk_vgg_conv3x3_relu_wino_f32(const float* in, const float* u_packed, const float* bias, float* out,
                                  int frames, int H, int W, int cin, int cout, int fuse_pool, void* stream);

/* The same operator by fused Winograd F(4x4,3x3) (csrc/conv_wino43.hip): 36 transform planes, 4x fewer multiplies
 * than the direct form; fp32 rounding error ~16x that of F(2x2,3x3) (4e-6 .. 9e-6 of the activation scale per layer),
 * inside the 1e-4 bound of the path.  cin multiple of 16, cout multiple of 64 (cout/64 dividing or a multiple of 8),
 * H and W multiples of 4.  ntk_vgg_wino43_packed_floats(cin, cout) = 36*cin*cout floats.
 * ntk_vgg_wino43_supported: 1 for a whole-frame layer shape the entries below take (on four or eight waves);
 * ntk_vgg_wino43_blocked_supported: 1 where the eight-wave kernel takes it, which is what the channel-blocked entry
 * ntk_vgg_conv3x3_relu_wino43_layout_f32 needs (a layer cut into single tiles only while a block of 32 tiles spans less than
 * 16 MB of input).  Both are the launcher's own decision, from shapes alone. */
size_t ntk_vgg_wino43_packed_floats(int cin, int cout);
int ntk_vgg_wino43_supported(int frames, int H, int W, int cin, int cout);
int ntk_vgg_wino43_blocked_supported(int frames, int H, int W, int cin, int cout);
int ntk_vgg_pack_weights_wino43(const float* w_hwio, float* u_packed, int cin, int cout, void* stream);
int ntk_vgg_conv3x3_relu_wino43_f32(const float* in, const float* u_packed, const float* bias, float* out,
                                    int frames, int H, int W, int cin, int cout, int fuse_pool, void* stream);
/* The same layer computed only inside the window [y0, y1) x [x0, x1) of its un-pooled output (multiples of 4 inside the
 * frame): the tiles of the window are written exactly as the whole-frame call writes them, nothing else is touched.  For
 * the last layer of a trunk whose consumer reads fixed positions only (direct_offset_output.py:392-399 gathers 64 points
 * of conv4_3, receptive_field_sizes.py:135-143: rows / columns 6, 8, ..., 20 of 28). */
int ntk_vgg_conv3x3_relu_wino43_window_f32(const float* in, const float* u_packed, const float* bias, float* out,
                                           int frames, int H, int W, int cin, int cout, int fuse_pool,
                                           int y0, int x0, int y1, int x1, void* stream);
/* The general form: window + kernel form.  waves = 8 (what the two entries above launch): eight waves per workgroup, two per
 * SIMD -- one runs the patch staging and the input transform beside a third of the MFMAs, the other two thirds of the MFMAs and
 * nothing else; waves = 4: round 2's one-wave-per-SIMD kernel.  Same bits either way (tests/test_vgg_gpu.py). */
int ntk_vgg_conv3x3_relu_wino43_form_f32(const float* in, const float* u_packed, const float* bias, float* out,
                                         int frames, int H, int W, int cin, int cout, int fuse_pool,
                                         int y0, int x0, int y1, int x1, int waves, void* stream);
/* The eight-wave kernel with CHANNEL-BLOCKED activation maps on either side, [frames][H][C / 8][W][8] (channel blocks of 8
 * interleaved per image row) -- the layout the layers of a trunk hand to each other: the eight channels of a K step are one
 * contiguous 32-byte piece per pixel and a patch row is one contiguous run, so the patch staging reads whole cache lines (NHWC:
 * 32-byte pieces 4 * cin bytes apart).  in_blocked / out_blocked: which side is blocked (0 = NHWC).  Whole frames, any shape the
 * eight-wave kernel takes.  Same arithmetic and bits as ntk_vgg_conv3x3_relu_wino43_f32.
 * (vgg.py:155-161: the layers themselves; the layout between them is this library's own business.) */
int ntk_vgg_conv3x3_relu_wino43_layout_f32(const float* in, const float* u_packed, const float* bias, float* out,
                                           int frames, int H, int W, int cin, int cout, int fuse_pool,
                                           int in_blocked, int out_blocked, void* stream);

/* slim.max_pool2d [2,2] stride 2 on NHWC fp32 (vgg.py:155-161) as its own launch (ntk_maxpool2x2).
 * The trunk fuses the pool into the epilogue of conv1_2 / conv2_2 / conv3_3 (fuse_pool); this entry point is the
 * un-fused form with identical results.  H, W even; C a multiple of 4. */
int ntk_maxpool2x2(const float* in, float* out, int frames, int H, int W, int C, void* stream);

/* ------------------------------------------------------------------------
 * plain fp32 GEMMs used around the NTM recurrence (hoisted LSTM input
 * projection and the BPTT weight-gradient contractions)
 * replaces: tf.matmul inside BasicLSTMCell / _linear, ntm_cell.py:103-105,
 *           :124-126, :220 (and their tf.gradients)
 * --------------------------------------------------------------------- */

/* C[M,N] = A[M,K] * B[N,K]^T (+ bias[N]);  lda, ldb, K multiples of 4. */
int ntk_gemm_nt_f32(const float* A, int lda, const float* B, int ldb, const float* bias,
                    float* C, int ldc, int M, int N, int K, void* stream);

/* C[M,N] (+)= sum_k A[k,M] * B[k,N]  (both operands k-major), split over
 * `splits` K-ranges through `workspace` (splits*M*N floats) and reduced in a
 * fixed order (bitwise reproducible).  lda, ldb, M, N multiples of 4.
 * accumulate != 0 adds into C. */
size_t ntk_gemm_tn_workspace_bytes(int M, int N, int splits);
int ntk_gemm_tn_f32(const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                    int M, int N, int K, int splits, int accumulate, float* workspace,
                    void* stream);

/* out[cols][ldo] = in[rows][ldi]^T, zero padded to ldo (>= rows) */
int ntk_transpose_pad(const float* in, int ldi, float* out, int ldo, int rows, int cols, void* stream);

/* ------------------------------------------------------------------------
 * NTM cell sequence kernels
 * replaces: NTMCell.__call__ (ntm_cell.py:53-253) unrolled by LoopNTMTracker's
 *           tf.while_loop (ntm_tracker_new.py:13-64), ops.py:135-158 (cosine
 *           similarity, quirk Q1) and ops.py:180-242 (circular shift, quirk Q2)
 *
 * Packed parameter layouts (see ntm-tracker_amd/csrc/ntm_common.h):
 *   WxT [4*hid][ldx]  Wr [ldz][4*hid] (row K = LSTM bias)  Wa [ldh][PP] (row hid = biases)
 * with gate columns interleaved per unit (n' = unit*4 + gate, gate order i,j,f,o).
 * --------------------------------------------------------------------- */

/* control width P, padded widths and leading dimensions for a configuration */
int ntk_ntm_padded_dims(int N, int Md, int R, int Wh, int hid, int shift_range, int O,
                        int* P, int* PP, int* K, int* ldz, int* ldh);

/* Limits of the single-layer sequence kernels.  Every entry below checks them on the host before any launch; a shape outside
 * them is refused with NTK_ERR_BAD_SHAPE / NTK_ERR_UNSUPPORTED and the reason in ntk_last_error(), never computed wrongly.
 * H = R + Wh heads, SS = 2*shift_range + 1, P / PP / K from ntk_ntm_padded_dims, T = threads of the workgroup.
 *
 * Forward (ntk_ntm_seq_fwd, ntk_ntm_step_fwd):
 *   B >= 1, S >= 1, O >= 1, R >= 1, Wh >= 1                        (else NTK_ERR_BAD_SHAPE)
 *   mem_size N a multiple of 64 in [64, 1024];  mem_dim Md in [1, 256]
 *   H <= 15 (one wave per head);  hid in [1, 960];  shift_range <= 4 and SS < N (SS >= N: NTK_ERR_BAD_SHAPE)
 *   hid + Md <= 1024,  PP + Md <= 1024,  H*Md + H + 1 <= 1024,  R*Md <= 1024
 *   the state within 160 KiB of LDS: roughly 4 * (N*(Md|1) + 3*H*N + max(nsl*4*hid, nslB*PP, nslR*R*Md) + K + hid + PP + H*Md + Md)
 *   bytes, where the three slice counts are T/hid, min(T/(PP/4), hid) and min(T/(R*Md), N).
 *   T = min(1024, the largest of H*N, 3*hid, PP + Md, H*Md + H + 1, (ceil(hid/64) + 1)*64, (H + 1)*64, rounded up to whole
 *   waves): H*N may exceed T (every mem_size above 512 does).
 *
 * BPTT (ntk_ntm_seq_bwd, ntk_ntm_step_bwd) -- narrower: a shape may run forward and still be refused here, so a training caller
 * asks ntk_ntm_seq_plan BEFORE the forward pass:
 *   every forward limit, and
 *   hid a multiple of 4;  ldkT >= K, ldhT >= hid, both multiples of 4 (else NTK_ERR_BAD_SHAPE)
 *   T = the largest of H*N, 3*hid, PP, K, H*Md + Md + 2*Wh*Md, N*Md/8 (a thread prefetches at most 8 memory elements), rounded
 *   up to whole waves, must be <= 1024: so H*N <= 1024 (mem_size above 512 never trains), 3*hid <= 1024 (hid <= 340),
 *   PP <= 1024, K <= 1024, N*Md <= 8192
 *   the BPTT state within 160 KiB of LDS: roughly 4 * (4*N*(Md|1) + 8*H*N + 9*hid + ...) bytes, one more N*(Md|1) with write_first.
 *
 * Kernel ids ntk_ntm_seq_plan reports (0 = refused): */
#define NTK_NTM_FWD_WS           1   /* wave-specialised forward, tracker shape without write_first (768 threads) */
#define NTK_NTM_FWD_FIX512       2   /* fixed-dims forward with resident gate rows, tracker shape otherwise (512 threads) */
#define NTK_NTM_FWD_GENERIC768   3   /* generic forward, T <= 768 */
#define NTK_NTM_FWD_GENERIC1024  4   /* generic forward, 768 < T <= 1024 */
#define NTK_NTM_FWD_FIX640_DEV   5   /* development builds only (-DNTK_NTM_FWD_STREAM_ONLY) */
#define NTK_NTM_BWD_WS           1   /* wave-specialised BPTT: tracker shape, not write_first, ldkT 280, ldhT 200 (768 threads) */
#define NTK_NTM_BWD_FIX          2   /* fixed-dims BPTT: the same shapes under NTK_NTM_BWD_FORM=res (640 threads) */
#define NTK_NTM_BWD_GENERIC768   3   /* generic BPTT, T <= 768 */
#define NTK_NTM_BWD_GENERIC1024  4   /* generic BPTT, 768 < T <= 1024 */
/* bits of the value ntk_ntm_seq_plan / ntk_ntm_seq_deep_plan return */
#define NTK_NTM_PLAN_FWD 1
#define NTK_NTM_PLAN_BWD 2

/* What ntk_ntm_seq_fwd / ntk_ntm_seq_bwd would do with a shape, host arithmetic only (no device call): returns a mask of
 * NTK_NTM_PLAN_FWD (the forward runs) and NTK_NTM_PLAN_BWD (the BPTT runs) and, through the nullable out pointers, the kernel
 * id and the workgroup size of each direction (0 where refused).  The reason for a refusal is in ntk_last_error() (the
 * forward's where both refuse).  ldkT / ldhT: the leading dimensions the caller will hand ntk_ntm_seq_bwd; <= 0 stands for the
 * smallest valid ones, align4(K) and align4(hid).  The two entries decide through the same function, so the answer cannot
 * drift from the launch; it honours the development switches NTK_NTM_FWD_FORM / NTK_NTM_BWD_FORM as they are when it is called. */
int ntk_ntm_seq_plan(int B, int N, int Md, int R, int Wh, int hid, int shift_range, int O, int write_first,
                     int ldkT, int ldhT, int* fwd_kernel, int* fwd_threads, int* bwd_kernel, int* bwd_threads);

/* S steps of the cell for B sequences, one persistent workgroup per sequence.
 * xproj [B,S,4*hid] = X * WxT^T (no bias).  State in: M0 [B,N,Md], w0 [B,H,N],
 * read0 [B,R,Md], cs0 [B,2*hid] (c then h).  Out: logits [B,S,O], outputs
 * (softmax, nullable), final state.  st_* (all nullable): per-step records
 * = what LoopNTMTracker writes to its TensorArrays plus the BPTT stash. */
int ntk_ntm_seq_fwd(int B, int S, int N, int Md, int R, int Wh, int hid, int shift_range, int O,
                    int write_first,
                    const float* xproj, const float* Wr, const float* Wa,
                    const float* M0, const float* w0, const float* read0, const float* cs0,
                    float* logits, float* outputs,
                    float* M_out, float* w_out, float* read_out, float* cs_out,
                    float* st_z, float* st_gates, float* st_c, float* st_h, float* st_u,
                    float* st_wc, float* st_wv, float* st_w, float* st_M, float* st_read,
                    void* stream);

/* Full BPTT through a recorded sequence (tf.gradients through the while_loop,
 * direct_offset_output.py:611-621).  In: transposed weights WrT [4*hid][ldkT],
 * WaT [PP][ldhT], the records, dlogits [B,S,O], optional gradient of the final
 * state.  Out: raw gate gradients dgates [B,S,4*hid], raw control/logit
 * gradients du [B,S,PP], gradient of the initial state. */
int ntk_ntm_seq_bwd(int B, int S, int N, int Md, int R, int Wh, int hid, int shift_range, int O,
                    int write_first,
                    const float* WrT, int ldkT, const float* WaT, int ldhT,
                    const float* M0, const float* w0, const float* cs0,
                    const float* st_gates, const float* st_c, const float* st_u,
                    const float* st_wc, const float* st_wv, const float* st_w, const float* st_M,
                    const float* dlogits,
                    const float* dM_fin, const float* dw_fin, const float* dread_fin, const float* dcs_fin,
                    float* dgates, float* du, float* dM0, float* dw0, float* dread0, float* dcs0,
                    void* stream);

/* ------------------------------------------------------------------------
 * NTM cell with a deep controller: a MultiRNNCell of L >= 2 BasicLSTMCell
 * layers (ntm_cell.py:45-50, :101-105) inside the persistent sequence kernels.
 * Layer 0 reads [x_t ; read_{t-1}] and h_0(t-1), layer k >= 1 reads h_{k-1}(t)
 * and h_k(t-1), h_{L-1}(t) drives the unpack / output linear; addressing and
 * memory as ntk_ntm_seq_fwd.  Controller state [B][2*hid*L] = c_0, h_0, c_1,
 * h_1, ... (MultiRNNCell concatenation).
 *
 * Sizes (align4(n) = n rounded up to a multiple of 4; RM = R*Md; hid % 4 == 0):
 *   ldx = align4(D)              ldxt = align4(hid)       ldz, ldh, PP: ntk_ntm_padded_dims
 *   ld0 = align4(D + RM + hid + 1)                        ld1 = align4(2*hid + 1)
 *   rf0 = align4(RM + hid + 1)   rf1 = align4(2*hid + 1)  cb0 = align4(RM + hid)   cb1 = 2*hid
 * Gate columns n' = unit*4 + gate (gate order i,j,f,o) unless noted.
 *
 * Every entry validates on the host before any launch: NTK_ERR_BAD_SHAPE
 * (L < 2, non-positive sizes), NTK_ERR_UNSUPPORTED (a shape outside
 * ntk_ntm_seq_deep_supported), NTK_ERR_BAD_PTR (null or misaligned pointer);
 * the reason is in ntk_last_error().
 * --------------------------------------------------------------------- */

/* 1 if the deep kernels run this configuration (forward AND BPTT), else 0 with
 * the reason in ntk_last_error().  Host arithmetic only: the same limits as
 * ntk_ntm_seq_fwd, hid % 4 == 0, and every layer's state within the LDS.
 * Answers for write_first = 0; a write_first cell keeps one more copy of the memory (N*(Md|1) floats) in the BPTT's LDS, so
 * close to the 160 KiB bound ask ntk_ntm_seq_deep_plan, which takes the flag. */
int ntk_ntm_seq_deep_supported(int B, int N, int Md, int R, int Wh, int hid, int shift_range, int O, int L);

/* The deep form's ntk_ntm_seq_plan: the mask is NTK_NTM_PLAN_FWD | NTK_NTM_PLAN_BWD or 0 (the deep kernels take a shape in both
 * directions or not at all: every BPTT limit of the single-layer form applies to the deep forward too, and Tb also covers
 * 2*hid, so 3*hid <= 1024).  Kernel ids: the instantiation by workgroup size, for the forward (Tf) and the BPTT (Tb). */
#define NTK_NTM_DEEP_768   1   /* T <= 768 */
#define NTK_NTM_DEEP_1024  2   /* 768 < T <= 1024 */
int ntk_ntm_seq_deep_plan(int B, int N, int Md, int R, int Wh, int hid, int shift_range, int O, int L, int write_first,
                          int* fwd_kernel, int* fwd_threads, int* bwd_kernel, int* bwd_threads);

/* Float counts of the three packed weight buffers:
 *   n_wx0 = 4*hid*ldx   n_wf = 4*hid*(rf0 + (L-1)*rf1)   n_wb = 4*hid*(cb0 + (L-1)*cb1) */
int ntk_ntm_seq_deep_packed_floats(int D, int R, int Md, int hid, int L, size_t* n_wx0, size_t* n_wf, size_t* n_wb);

/* Pack the controller weights into the kernels' layouts (one launch; run it
 * whenever the weights change -- nothing is cached).  In:
 *   lowerT   the L-1 lower layers back to back, TF gate-major rows (g*hid + unit):
 *            layer 0 [4*hid][ld0]  columns x (D) | read (RM) | h_0 (hid) | bias | 0..
 *            layer k [4*hid][ld1]  columns h_{k-1} (hid) | h_k (hid) | bias | 0..   (k = 1 .. L-2)
 *   top_WxT  [4*hid][ldxt]          top layer, input h_{L-2} (the single-layer WxT layout)
 *   top_Wr   [align4(RM+hid+1)][4*hid]  top layer: rows 0..RM-1 unused, rows RM..RM+hid-1
 *            multiply h_{L-1}, row RM+hid = bias (the single-layer Wr layout)
 * Out (16-byte aligned):
 *   Wx0 [4*hid][ldx]     layer 0's x part, zero columns from D on; xproj = X * Wx0^T
 *   Wf  forward blocks [4*hid] wide: layer 0 [rf0] rows read | h_0 | bias | 0..,
 *       then layers 1..L-1 [rf1] rows each h_{k-1} | h_k | bias | 0..
 *   Wb  the blocks transposed, no bias: layer 0 [4*hid][cb0] columns read | h_0 | 0..,
 *       then layers 1..L-1 [4*hid][cb1] columns h_{k-1} | h_k */
int ntk_ntm_seq_deep_pack(int D, int R, int Md, int hid, int L, const float* lowerT, const float* top_WxT,
                          const float* top_Wr, float* Wx0, float* Wf, float* Wb, void* stream);

/* S steps for B sequences, one persistent workgroup per sequence.  In:
 * X [B,S,ldx] (read only for st_buf0), xproj [B,S,4*hid] = X * Wx0^T (no bias),
 * Wf, Wa [ldh][PP], M0 [B,N,Md], w0 [B,H,N], read0 [B,R,Md], cs0 [B,2*hid*L].
 * Out: logits [B,S,O], outputs (softmax, nullable), final state (cs_out [B,2*hid*L]).
 * Records (each nullable; st_gates with st_c): the top layer's as ntk_ntm_seq_fwd
 *   st_z [B,S,ldz] = [read_{t-1} | h_{L-1}(t-1) | 1 | 0..], st_gates [B,S,hid,4],
 *   st_c [B,S,hid], st_h [B,S,ldh] = [h_{L-1}(t) | 1 | 0..], st_u [B,S,PP],
 *   st_wc / st_wv / st_w [B,S,H,N], st_M [B,S,N,Md], st_read [B,S,R,Md];
 * and the lower layers'
 *   st_xtop   [B,S,ldxt]       h_{L-2}(t) | 0..  (the top layer's input)
 *   st_buf0   [B,S,ld0]        x_t (D) | read_{t-1} | h_0(t-1) | 1 | 0..
 *   st_bufk   [L-2][B,S,ld1]   layer k = 1..L-2: h_{k-1}(t) | h_k(t-1) | 1 | 0..  (unused at L = 2)
 *   st_lgates [L-1][B,S,hid,4] activated gates of layers 0..L-2 (16-byte aligned)
 *   st_lc     [L-1][B,S,hid]   c_k(t) of layers 0..L-2 */
int ntk_ntm_seq_fwd_deep(int B, int S, int N, int Md, int R, int Wh, int hid, int shift_range, int O, int L,
                         int write_first, int D,
                         const float* X, const float* xproj, const float* Wf, const float* Wa,
                         const float* M0, const float* w0, const float* read0, const float* cs0,
                         float* logits, float* outputs,
                         float* M_out, float* w_out, float* read_out, float* cs_out,
                         float* st_z, float* st_gates, float* st_c, float* st_h, float* st_u,
                         float* st_wc, float* st_wv, float* st_w, float* st_M, float* st_read,
                         float* st_xtop, float* st_buf0, float* st_bufk, float* st_lgates, float* st_lc,
                         void* stream);

/* Full BPTT through a recorded deep sequence.  In: Wb, WaT [PP][ldhT] (Wa
 * transposed, ldhT >= hid, multiple of 4), M0, w0, cs0 [B,2*hid*L], the forward's
 * records st_gates .. st_M (top layer and heads) and st_lgates, st_lc (lower
 * layers), dlogits [B,S,O], optional gradient of the final state (dcs_fin
 * [B,2*hid*L]).  Out: dgates [B,S,4*hid] (top layer, raw, n' = unit*4 + gate),
 * dpre [L-1][B,S,4*hid] (layers 0..L-2, raw, TF gate-major g*hid + unit),
 * du [B,S,PP], gradient of the initial state (dcs0 [B,2*hid*L]).  Weight
 * gradients are k-major GEMMs of these with the records (dgates with st_xtop and
 * st_z, du with st_h, dpre with st_buf0 / st_bufk).  Fixed summation order, no
 * atomics: bitwise reproducible. */
int ntk_ntm_seq_bwd_deep(int B, int S, int N, int Md, int R, int Wh, int hid, int shift_range, int O, int L,
                         int write_first,
                         const float* Wb, const float* WaT, int ldhT,
                         const float* M0, const float* w0, const float* cs0,
                         const float* st_gates, const float* st_c, const float* st_u,
                         const float* st_wc, const float* st_wv, const float* st_w, const float* st_M,
                         const float* st_lgates, const float* st_lc,
                         const float* dlogits,
                         const float* dM_fin, const float* dw_fin, const float* dread_fin, const float* dcs_fin,
                         float* dgates, float* dpre, float* du, float* dM0, float* dw0, float* dread0, float* dcs0,
                         void* stream);

/* Stand-alone addressing ops (ops.py, called by ops_test.py): batched_smooth_cosine_similarity (:135-158) --
 * mode 0 = as coded (quirk Q1: feature columns normalised over the slot axis; what NTMCell computes),
 * mode 1 = true smooth cosine dot/(|m||k| + 1e-3) (what ops_test.py:20-34 pins); memory [B,N,Md], keys [B,H,Md],
 * out [B,H,N].  batched_circular_convolution (:180-214) with the Python-2 taps (quirk Q2): w [B,H,N],
 * kernel [B,H,shift_space]. */
int ntk_ntm_cosine_similarity(const float* memory, const float* keys, float* out, int B, int N, int Md, int H,
                              int mode, void* stream);
int ntk_ntm_circular_convolution(const float* w, const float* kernel, float* out, int B, int H, int N, int shift_space,
                                 void* stream);
/* The intermediate tensors of ONE cell step that NTMCell.__call__ returns in `debug` (ntm_cell.py:230-250) and the fused
 * step keeps in registers: sw (:161, softmax of the raw shift block at oS), w_gated (:153-156), powed_w_conv (:173), M_write /
 * M_erase (:197-203), from what the step records
 * (u [B,ldu] = the activated control vector with g at oG, gamma at oY, erase at oE, add at oA; wc, wv, w, w_prev [B,H,N]). */
int ntk_ntm_step_debug(const float* u, int ldu, int oG, int oS, int shift_space, int oY, int oE, int oA, const float* wc, const float* wv,
                       const float* w, const float* w_prev, float* sw, float* w_gated, float* w_conv_powed, float* M_write,
                       float* M_erase, int B, int N, int Md, int R, int Wh, void* stream);

/* One step of the cell (ntk_ntm_step_fwd/bwd) = the sequence kernels with S = 1; argument meaning as
 * ntk_ntm_seq_fwd / ntk_ntm_seq_bwd (the state AFTER the step takes the place of the final state). */
int ntk_ntm_step_fwd(int B, int N, int Md, int R, int Wh, int hid, int shift_range, int O, int write_first,
                     const float* xproj, const float* Wr, const float* Wa,
                     const float* M_prev, const float* w_prev, const float* read_prev, const float* cs_prev,
                     float* logits, float* outputs, float* M, float* w, float* read, float* cs,
                     float* st_z, float* st_gates, float* st_c, float* st_h, float* st_u,
                     float* st_wc, float* st_wv, float* st_w, float* st_M, float* st_read, void* stream);
int ntk_ntm_step_bwd(int B, int N, int Md, int R, int Wh, int hid, int shift_range, int O, int write_first,
                     const float* WrT, int ldkT, const float* WaT, int ldhT,
                     const float* M_prev, const float* w_prev, const float* cs_prev,
                     const float* st_gates, const float* st_c, const float* st_u,
                     const float* st_wc, const float* st_wv, const float* st_w, const float* st_M,
                     const float* dlogits,
                     const float* dM, const float* dw, const float* dread, const float* dcs,
                     float* dgates, float* du, float* dM_prev, float* dw_prev, float* dread_prev, float* dcs_prev,
                     void* stream);

/* ------------------------------------------------------------------------
 * Similarity mode of the content addressing.  The entries above compute the reference's as-coded similarity (quirk Q1: every
 * feature column of the memory l2-normalised over the slots).  Their *_sim siblings take one more argument, `similarity`,
 * right after write_first, and are otherwise the same call:
 *   NTK_NTM_SIM_AS_CODED       what the entry without the suffix computes (which forwards here with this value)
 *   NTK_NTM_SIM_SMOOTH_COSINE  row-wise sim[h][n] = k_h . M[n] / (|k_h| |M[n]| + 1e-3) on the memory BEFORE this step's write
 *                              (with and without write_first), no clamp on either norm -- the content addressing of the NTM
 *                              paper and of the reference's ops_test.py, ntk_ntm_cosine_similarity's mode 1.
 * Any other value is refused with NTK_ERR_UNSUPPORTED before anything else is looked at (no pointer is read, nothing is
 * launched).  The mode is an argument of every call: the library keeps no mode state and reads no environment switch for it.
 * Forward and BPTT of one sequence must be given the same mode (the BPTT recomputes sim from the records u and M_prev; there
 * are no additional records).  In the BPTT the gradient through a norm that is exactly zero (an all-zero memory row, an
 * all-zero key) is defined as 0, where automatic differentiation yields NaN; sim itself is 0 there.
 * Shape limits are those of the as-coded entries, except that the normaliser takes N floats of LDS where it took Md
 * (forward: once; BPTT: twice), which the plans account for.  Smooth cosine has no wave-specialised form: the plans report
 * NTK_NTM_FWD_FIX512 / NTK_NTM_BWD_FIX for the tracker shape and never NTK_NTM_FWD_WS / NTK_NTM_BWD_WS.
 * --------------------------------------------------------------------- */
#define NTK_NTM_SIM_AS_CODED       0
#define NTK_NTM_SIM_SMOOTH_COSINE  1

/* ntk_ntm_seq_plan for a similarity mode; NTK_ERR_UNSUPPORTED (negative, not a mask) for an unknown mode */
int ntk_ntm_seq_plan_sim(int B, int N, int Md, int R, int Wh, int hid, int shift_range, int O, int write_first, int similarity,
                         int ldkT, int ldhT, int* fwd_kernel, int* fwd_threads, int* bwd_kernel, int* bwd_threads);
/* ntk_ntm_seq_fwd / ntk_ntm_seq_bwd in a similarity mode */
int ntk_ntm_seq_fwd_sim(int B, int S, int N, int Md, int R, int Wh, int hid, int shift_range, int O,
                        int write_first, int similarity,
                        const float* xproj, const float* Wr, const float* Wa,
                        const float* M0, const float* w0, const float* read0, const float* cs0,
                        float* logits, float* outputs,
                        float* M_out, float* w_out, float* read_out, float* cs_out,
                        float* st_z, float* st_gates, float* st_c, float* st_h, float* st_u,
                        float* st_wc, float* st_wv, float* st_w, float* st_M, float* st_read,
                        void* stream);
int ntk_ntm_seq_bwd_sim(int B, int S, int N, int Md, int R, int Wh, int hid, int shift_range, int O,
                        int write_first, int similarity,
                        const float* WrT, int ldkT, const float* WaT, int ldhT,
                        const float* M0, const float* w0, const float* cs0,
                        const float* st_gates, const float* st_c, const float* st_u,
                        const float* st_wc, const float* st_wv, const float* st_w, const float* st_M,
                        const float* dlogits,
                        const float* dM_fin, const float* dw_fin, const float* dread_fin, const float* dcs_fin,
                        float* dgates, float* du, float* dM0, float* dw0, float* dread0, float* dcs0,
                        void* stream);
/* ntk_ntm_step_fwd / ntk_ntm_step_bwd in a similarity mode (the *_sim sequence entries with S = 1) */
int ntk_ntm_step_fwd_sim(int B, int N, int Md, int R, int Wh, int hid, int shift_range, int O, int write_first, int similarity,
                         const float* xproj, const float* Wr, const float* Wa,
                         const float* M_prev, const float* w_prev, const float* read_prev, const float* cs_prev,
                         float* logits, float* outputs, float* M, float* w, float* read, float* cs,
                         float* st_z, float* st_gates, float* st_c, float* st_h, float* st_u,
                         float* st_wc, float* st_wv, float* st_w, float* st_M, float* st_read, void* stream);
int ntk_ntm_step_bwd_sim(int B, int N, int Md, int R, int Wh, int hid, int shift_range, int O, int write_first, int similarity,
                         const float* WrT, int ldkT, const float* WaT, int ldhT,
                         const float* M_prev, const float* w_prev, const float* cs_prev,
                         const float* st_gates, const float* st_c, const float* st_u,
                         const float* st_wc, const float* st_wv, const float* st_w, const float* st_M,
                         const float* dlogits,
                         const float* dM, const float* dw, const float* dread, const float* dcs,
                         float* dgates, float* du, float* dM_prev, float* dw_prev, float* dread_prev, float* dcs_prev,
                         void* stream);
/* ntk_ntm_seq_deep_plan / ntk_ntm_seq_fwd_deep / ntk_ntm_seq_bwd_deep in a similarity mode */
int ntk_ntm_seq_deep_plan_sim(int B, int N, int Md, int R, int Wh, int hid, int shift_range, int O, int L, int write_first,
                              int similarity, int* fwd_kernel, int* fwd_threads, int* bwd_kernel, int* bwd_threads);
int ntk_ntm_seq_fwd_deep_sim(int B, int S, int N, int Md, int R, int Wh, int hid, int shift_range, int O, int L,
                             int write_first, int similarity, int D,
                             const float* X, const float* xproj, const float* Wf, const float* Wa,
                             const float* M0, const float* w0, const float* read0, const float* cs0,
                             float* logits, float* outputs,
                             float* M_out, float* w_out, float* read_out, float* cs_out,
                             float* st_z, float* st_gates, float* st_c, float* st_h, float* st_u,
                             float* st_wc, float* st_wv, float* st_w, float* st_M, float* st_read,
                             float* st_xtop, float* st_buf0, float* st_bufk, float* st_lgates, float* st_lc,
                             void* stream);
int ntk_ntm_seq_bwd_deep_sim(int B, int S, int N, int Md, int R, int Wh, int hid, int shift_range, int O, int L,
                             int write_first, int similarity,
                             const float* Wb, const float* WaT, int ldhT,
                             const float* M0, const float* w0, const float* cs0,
                             const float* st_gates, const float* st_c, const float* st_u,
                             const float* st_wc, const float* st_wv, const float* st_w, const float* st_M,
                             const float* st_lgates, const float* st_lc,
                             const float* dlogits,
                             const float* dM_fin, const float* dw_fin, const float* dread_fin, const float* dcs_fin,
                             float* dgates, float* dpre, float* du, float* dM0, float* dw0, float* dread0, float* dcs0,
                             void* stream);

/* tf.contrib.rnn.BasicLSTMCell pointwise step (ntm_cell.py:45-50; gate pre-activations pre [B,4*hid] = [x,h] W + b from
 * ntk_gemm_nt_f32, TF block order i | j | f | o): c = c_prev*sigmoid(f + forget_bias) + sigmoid(i)*tanh(j),
 * h = tanh(c)*sigmoid(o); act [B,4*hid] (nullable) keeps the activated gates for the backward, which returns the
 * gradient of the pre-activations and of c_prev (dh or dc may be null = zero). */
int ntk_lstm_step_fwd(const float* pre, const float* c_prev, float forget_bias, float* c, float* h, float* act,
                      int B, int hid, void* stream);
int ntk_lstm_step_bwd(const float* act, const float* c_prev, const float* c, const float* dh, const float* dc,
                      float* dpre, float* dc_prev, int B, int hid, void* stream);

/* trainable initial state (ntm_cell.py:284-315): out[b][i] = act(v[i]),
 * act 0 = tanh, 1 = sigmoid; and its gradient summed over the batch */
int ntk_ntm_init_state(const float* v, float* out, int n, int B, int act, void* stream);
int ntk_ntm_init_state_bwd(const float* v, const float* dout, float* dv, int n, int B, int act,
                           int accumulate, void* stream);

/* ------------------------------------------------------------------------
 * DNC core sequence kernel (forward)
 * replaces: dnc.DNC._build (dnc/dnc.py:84-127) unrolled by tf.nn.dynamic_rnn
 *           (direct_offset_output_with_dnc.py:66-88): snt.LSTM controller,
 *           MemoryAccess (dnc/access.py:113-303), CosineWeights / TemporalLinkage /
 *           Freeness (dnc/addressing.py), output linear, clip_value.
 * Packed parameters: Wr [ldz][4*hid] (rows [reads ; h], row K = b_gates, columns
 * unit*4+gate), Wi [ldh][IP] = the ten interface linears side by side in the order
 * write_vectors, erase_vectors, free_gate, allocation_gate, write_gate, read_mode,
 * write_keys, write_strengths, read_keys, read_strengths (row hid = biases),
 * Wy [ldy][OP] (rows [h ; reads], row Ky = bias).  State tensors are updated IN PLACE.
 * Range (else NTK_ERR_UNSUPPORTED): N a multiple of 4 up to 1024, W a multiple of 4 up to 256,
 * R 1..4, Wn 1..8, R*W <= 1024, hid 1..1024, O 1..16, and a per-shape LDS layout of at most 160 KiB.
 * --------------------------------------------------------------------- */
int ntk_dnc_padded_dims(int N, int W, int R, int Wn, int hid, int O,
                        int* I, int* IP, int* K, int* ldz, int* ldh, int* Ky, int* ldy, int* OP);
int ntk_dnc_seq_fwd(int B, int S, int N, int W, int R, int Wn, int hid, int O, float clip_value,
                    const float* xproj, const float* Wr, const float* Wi, const float* Wy,
                    float* mem, float* link, float* usage, float* rw, float* ww, float* prec,
                    float* reads, float* hc, float* out,
                    /* per-step records for BPTT, all-or-none (null = inference): */
                    float* rec_z, float* rec_gates, float* rec_c, float* rec_hc, float* rec_yin,
                    float* rec_ifc, float* rec_u, float* rec_ww, float* rec_rw, float* rec_cw,
                    float* rec_cr, float* rec_al, float* rec_p, float* rec_fwd, float* rec_bwd,
                    float* rec_M, float* rec_L, float* rec_ypre, void* stream);

/* The same sequence kernel in CLUSTER form: k workgroups (one per CU) cooperate on each sequence -- the link rows and
 * the controller's hidden units are split k ways, the per-slot state and the N x W memory are replicated in LDS, and
 * two small exchanges per step go through a mailbox in `workspace` (csrc/dnc_cluster.h).  Same arguments, same state
 * in-place semantics and same records as ntk_dnc_seq_fwd; results differ from it by summation order only.
 * ntk_dnc_cluster_plan: the cluster size for a shape (k_request 0 = the largest that fits: B * k <= 256 CUs, link
 * rows + memory LDS resident; NTK_ERR_UNSUPPORTED and *k = 0 when the shape is outside the cluster kernels' range:
 * num_writes != 1, memory_size not a multiple of 64, ...) and the workspace size in bytes.  The workspace is
 * caller-owned device memory, 16-byte aligned, ZEROED ONCE by its owner, private to one launch at a time; its control
 * words are re-zeroed by every launch, its sticky error word (csrc/dnc_cluster.h) by ntk_dnc_cluster_status only.  ntk_dnc_cluster_status synchronises `stream` and reports whether a hand-off of the last launch on
 * that workspace timed out (every in-kernel spin is bounded; a launch that could not make progress aborts itself).
 * ntk_dnc_cluster_placement synchronises `stream` and reports how many of the B clusters of the last launch on that
 * workspace found all their k workgroups on one XCD and therefore ran the same-XCD form of the hand-offs (plain stores
 * kept in that XCD's L2; the others ran the write-through form: a speed difference only, csrc/dnc_cluster.h). */
int ntk_dnc_cluster_plan(int B, int N, int W, int R, int Wn, int hid, int O, int k_request, int* k, size_t* workspace_bytes);
int ntk_dnc_cluster_status(const void* workspace, int B, int k, void* stream);
int ntk_dnc_cluster_placement(const void* workspace, int B, int k, int* same_xcd_clusters, void* stream);
/* Device-side propagation of an aborted cluster launch, without a host synchronisation: when the sticky error word of
 * `workspace` (either form: mp_form 0 = ntk_dnc_cluster_*, 1 = ntk_dnc_mp_*, with its workspace_bytes) is set, loss[0]
 * and grad[0..n) become NaN: the NaN survives the data-parallel SUM all-reduce, so EVERY rank sees a NaN global norm and
 * ntk_rmsprop_clip_step_checked skips the update everywhere (zeros would have let the other ranks step on a partial
 * gradient).  loss / grad may be null.  ntk_dnc_cluster_inject_abort sets that sticky word the way a timed-out hand-off
 * does (fault injection for tests). */
int ntk_dnc_cluster_guard(const void* workspace, size_t workspace_bytes, int mp_form, int B, int k, float* loss, float* grad,
                          size_t n, void* stream);
int ntk_dnc_cluster_inject_abort(void* workspace, size_t workspace_bytes, int mp_form, int B, int k, void* stream);
int ntk_dnc_cluster_fwd(int B, int S, int N, int W, int R, int Wn, int hid, int O, float clip_value, int k,
                        const float* xproj, const float* Wr, const float* Wi, const float* Wy,
                        float* mem, float* link, float* usage, float* rw, float* ww, float* prec,
                        float* reads, float* hc, float* out,
                        float* rec_z, float* rec_gates, float* rec_c, float* rec_hc, float* rec_yin,
                        float* rec_ifc, float* rec_u, float* rec_ww, float* rec_rw, float* rec_cw,
                        float* rec_cr, float* rec_al, float* rec_p, float* rec_fwd, float* rec_bwd,
                        float* rec_M, float* rec_L, float* rec_ypre, void* workspace, void* stream);

/* Full BPTT in cluster form (arguments as ntk_dnc_seq_bwd; Wi is used un-transposed, WrT [4*hid][ldkT] as there):
 * d(link) rows LDS resident and split k ways, d(memory) register resident, two exchanges per step; bitwise
 * reproducible gradients (no float atomics).  Range: num_writes 1, memory_size a multiple of 64 up to 256,
 * word_size <= 64, hidden a multiple of 4 (ntk_dnc_cluster_bwd_plan says so for a shape; its own workspace). */
int ntk_dnc_cluster_bwd_plan(int B, int N, int W, int R, int Wn, int hid, int O, int k_request, int* k, size_t* workspace_bytes);
int ntk_dnc_cluster_bwd(int B, int S, int N, int W, int R, int Wn, int hid, int O, float clip_value, int k,
                        const float* WrT, int ldkT, const float* Wi, const float* Wy,
                        const float* mem0, const float* link0, const float* usage0, const float* rw0,
                        const float* ww0, const float* prec0, const float* hc0,
                        const float* rec_gates, const float* rec_c, const float* rec_ifc, const float* rec_u,
                        const float* rec_ww, const float* rec_rw, const float* rec_cw, const float* rec_cr,
                        const float* rec_al, const float* rec_p, const float* rec_fwd, const float* rec_bwd,
                        const float* rec_M, const float* rec_L, const float* rec_ypre,
                        const float* dout, float* gM, float* gL, float* dgates, float* dxi, float* dypre,
                        float* gcarry, int carry_in, void* workspace, void* stream);

/* The sequence kernels in MEMORY-PARTITIONED cluster form (csrc/dnc_mp.h): k workgroups per sequence, the N x N link
 * streamed through HBM once per step (N/k rows per workgroup; the BPTT record of step t-1 is the state step t reads),
 * the N x W memory partitioned by rows (LDS resident forward, register resident in BPTT), per-slot state replicated, four
 * hand-offs per step.  Nothing of size N x N or N x W is replicated, so this is the form for BASELINE configs[4]'s
 * core (memory 512 x 128: dnc/addressing.py:183-240 on 1 MiB of link per sequence-step), which the LDS-resident form
 * above cannot hold.  Same arguments, in-place state semantics and records as ntk_dnc_seq_fwd / ntk_dnc_seq_bwd; results
 * differ by summation order only and are bitwise reproducible run to run.
 * ntk_dnc_mp_plan / ntk_dnc_mp_bwd_plan: cluster size (k_request 0 = the smallest that fits; B * k <= the device's compute
 * units, queried per device) and the workspace size.  The workspace is caller-owned, 16-byte aligned, ZEROED ONCE by its
 * owner: besides the per-launch control words (re-zeroed by every launch) its last 256-byte line holds a STICKY error
 * word that a timed-out hand-off sets and no launch clears.  ntk_dnc_mp_status synchronises `stream` and fails when the
 * last launch or (sticky word) any launch since the word was last cleared aborted; clear_sticky != 0 clears it. */
/* Compute units the cooperative kernels may count on for the current device: hipDeviceAttributeMultiprocessorCount (assumes
 * the process has the device to itself -- a CU mask or another process's kernels are invisible to it), capped by the
 * environment variable NTK_DNC_CU_BUDGET when set; 0 when the device cannot be queried (the cluster forms are then refused
 * by every planner and the one-workgroup-per-sequence kernels run). */
int ntk_cu_count(void);
int ntk_dnc_mp_plan(int B, int N, int W, int R, int Wn, int hid, int O, int k_request, int* k, size_t* workspace_bytes);
/* > 0 when (shape, k) has a compile-time instantiation of the mp kernels (the generic one is functional but several times slower) */
int ntk_dnc_mp_compiled_shape(int N, int W, int R, int Wn, int hid, int O, int k);
int ntk_dnc_mp_status(const void* workspace, size_t workspace_bytes, int B, int k, int clear_sticky, void* stream);
int ntk_dnc_mp_placement(const void* workspace, int B, int k, int* same_xcd_clusters, void* stream);
int ntk_dnc_mp_fwd(int B, int S, int N, int W, int R, int Wn, int hid, int O, float clip_value, int k,
                   const float* xproj, const float* Wr, const float* Wi, const float* Wy,
                   float* mem, float* link, float* usage, float* rw, float* ww, float* prec,
                   float* reads, float* hc, float* out,
                   float* rec_z, float* rec_gates, float* rec_c, float* rec_hc, float* rec_yin,
                   float* rec_ifc, float* rec_u, float* rec_ww, float* rec_rw, float* rec_cw,
                   float* rec_cr, float* rec_al, float* rec_p, float* rec_fwd, float* rec_bwd,
                   float* rec_M, float* rec_L, float* rec_ypre, void* workspace, void* stream);

int ntk_dnc_mp_bwd_plan(int B, int N, int W, int R, int Wn, int hid, int O, int k_request, int* k, size_t* workspace_bytes);
int ntk_dnc_mp_bwd(int B, int S, int N, int W, int R, int Wn, int hid, int O, float clip_value, int k,
                   const float* WrT, int ldkT, const float* Wi, const float* Wy,
                   const float* mem0, const float* link0, const float* usage0, const float* rw0,
                   const float* ww0, const float* prec0, const float* hc0,
                   const float* rec_gates, const float* rec_c, const float* rec_ifc, const float* rec_u,
                   const float* rec_ww, const float* rec_rw, const float* rec_cw, const float* rec_cr,
                   const float* rec_al, const float* rec_p, const float* rec_fwd, const float* rec_bwd,
                   const float* rec_M, const float* rec_L, const float* rec_ypre,
                   const float* dout, float* gM, float* gL, float* dgates, float* dxi, float* dypre,
                   float* gcarry, int carry_in, void* workspace, void* stream);

/* Stand-alone DNC addressing modules (dnc/addressing.py), the module-level API the reference's own tests call:
 * CosineWeights._build (:83-105), TemporalLinkage._build (:133-153) and directional_read_weights (:155-181),
 * Freeness._build (:279-305) and write_allocation_weights (:307-340; one head: _allocation :376-405). */
int ntk_dnc_cosine_weights(const float* memory, const float* keys, const float* strengths, float* out,
                           int B, int N, int W, int H, void* stream);
int ntk_dnc_linkage(const float* prev_link, const float* prev_prec, const float* write_weights, float* link,
                    float* prec, int B, int N, int Wn, void* stream);
int ntk_dnc_directional_read_weights(const float* link, const float* prev_read_weights, float* out, int B, int N,
                                     int Wn, int R, int forward, void* stream);
int ntk_dnc_freeness(const float* write_weights, const float* free_gate, const float* read_weights,
                     const float* prev_usage, float* usage, int B, int N, int Wn, int R, void* stream);
int ntk_dnc_write_allocation_weights(const float* usage, const float* write_gates, float* out, int B, int N, int Wn,
                                     void* stream);

/* MemoryAccess pieces (dnc/access.py): the activations of _read_inputs (:160-218) on the RAW outputs of the ten
 * interface linears in the packed order [write_vectors | erase_vectors | free_gate | allocation_gate | write_gate |
 * read_mode | write_keys | write_strengths | read_keys | read_strengths] (row stride ldr); `act` receives each field
 * as a contiguous [B,width] array at act + B*offset(field).  _write_weights (:220-257), _erase_and_write (:32-63),
 * _read_weights (:259-303), read words (:151), and the whole step MemoryAccess._build (:113-158) = SURVEY's
 * ntk_dnc_access_step_fwd (its backward: ntk_dnc_access_step_bwd, below).
 * Workspaces (floats): write_weights 2*B*Wn*N + B*Wn; read_weights B*R*N*(1+2*Wn).
 * ntk_dnc_interface_activations: B, N, W, R, Wn >= 1 and ldr >= the interface width (else NTK_ERR_BAD_SHAPE). */
int ntk_dnc_interface_activations(const float* raw, int ldr, float* act, int B, int N, int W, int R, int Wn, void* stream);
int ntk_dnc_write_weights(const float* memory, const float* usage, const float* write_keys, const float* write_strengths,
                          const float* allocation_gate, const float* write_gate, float* write_weights, float* workspace,
                          int B, int N, int W, int Wn, void* stream);
int ntk_dnc_erase_and_write(const float* memory, const float* address, const float* reset_weights, const float* values,
                            float* out, int B, int N, int W, int Wn, void* stream);
int ntk_dnc_read_weights(const float* memory, const float* prev_read_weights, const float* link, const float* read_keys,
                         const float* read_strengths, const float* read_mode, float* read_weights, float* workspace,
                         int B, int N, int W, int R, int Wn, void* stream);
int ntk_dnc_read_words(const float* read_weights, const float* memory, float* out, int B, int N, int W, int R, void* stream);
size_t ntk_dnc_access_step_workspace_bytes(int B, int N, int W, int R, int Wn);
int ntk_dnc_access_step_fwd(const float* iface_raw, int ldr, const float* memory, const float* read_weights,
                            const float* write_weights, const float* link, const float* precedence, const float* usage,
                            float* memory_out, float* read_weights_out, float* write_weights_out, float* link_out,
                            float* precedence_out, float* usage_out, float* read_words, float* workspace,
                            int B, int N, int W, int R, int Wn, void* stream);

/* Backward of one MemoryAccess step at module granularity (what tf.gradients gives dnc/access_test.py:145-159).  The step
 * is recomputed from the PREVIOUS state and the raw interface; d_read_words [B,R,W] is the gradient w.r.t. the step's read
 * words; g_memory [B,N,W], g_read_weights [B,R,N], g_link [B,Wn,N,N], g_precedence [B,Wn,N], g_usage [B,N] are IN/OUT: in =
 * gradient w.r.t. the NEW state's field (zeros when the loss does not see it), out = gradient w.r.t. the previous state's
 * (write weights get none: they reach the next usage under stop_gradient only, addressing.py:302).  d_iface_raw [B,IP]
 * (IP from ntk_dnc_padded_dims): gradient w.r.t. the raw interface; the ten linears' gradients are GEMMs over it.
 * N and W multiples of 4, R <= 4, Wn <= 4, R*W <= 1020 (the step runs through ntk_dnc_seq_bwd with a controller of 4 units:
 * its K = R*W + 4 <= 1024).  Workspace: ntk_dnc_access_step_bwd_workspace_bytes. */
size_t ntk_dnc_access_step_bwd_workspace_bytes(int B, int N, int W, int R, int Wn);
int ntk_dnc_access_step_bwd(const float* iface_raw, int ldr, const float* memory, const float* read_weights,
                            const float* write_weights, const float* link, const float* precedence, const float* usage,
                            const float* d_read_words, float* g_memory, float* g_read_weights, float* g_link,
                            float* g_precedence, float* g_usage, float* d_iface_raw, float* workspace,
                            int B, int N, int W, int R, int Wn, void* stream);

/* Full BPTT through a recorded DNC sequence (num_writes 1..4: one write head runs the tuned kernel, 2..4 the
 * general one).  WrT [4*hid][ldkT], WiT [IP][ldhT]
 * are transposed copies of Wr / Wi; *0 pointers are the state BEFORE step 0; gM [B,N,W] and
 * gL [B,Wn,N,N] are zero-initialised scratch.  Out: raw gate gradients dgates [B,S,4*hid], raw
 * interface gradients dxi [B,S,IP], gradient of the pre-clip output dypre [B,S,OP]; weight
 * gradients follow as ntk_gemm_tn_f32 over the recorded rows.
 * Segmented BPTT (long sequences, config 5): run the segments last to first, re-recording each from its
 * checkpointed state; gM / gL are NOT re-zeroed between segments and gcarry [B, (Wn+1)*N + R*N + ldkT + hid]
 * (optional, may be null) carries the remaining state gradients: read when carry_in != 0, always written.
 * Range (else NTK_ERR_UNSUPPORTED): the forward's with Wn 1..4, hid a multiple of 4, K = R*W + hid <= 1024 (one
 * thread per element of d[reads_prev ; h_prev]) and its own LDS layout of at most 160 KiB. */
int ntk_dnc_seq_bwd(int B, int S, int N, int W, int R, int Wn, int hid, int O, float clip_value,
                    const float* WrT, int ldkT, const float* WiT, int ldhT, const float* Wy,
                    const float* mem0, const float* link0, const float* usage0, const float* rw0,
                    const float* ww0, const float* prec0, const float* hc0,
                    const float* rec_gates, const float* rec_c, const float* rec_ifc, const float* rec_u,
                    const float* rec_ww, const float* rec_rw, const float* rec_cw, const float* rec_cr,
                    const float* rec_al, const float* rec_p, const float* rec_fwd, const float* rec_bwd,
                    const float* rec_M, const float* rec_L, const float* rec_ypre,
                    const float* dout, float* gM, float* gL, float* dgates, float* dxi, float* dypre,
                    float* gcarry, int carry_in, void* stream);

/* ------------------------------------------------------------------------
 * tracking head (direct_offset_output.py)
 * --------------------------------------------------------------------- */

/* 64-point gather from conv4_3 (:392-399, receptive_field_sizes.py:135-143)
 * + input serialiser (:439-500): fmap [B*T,Hf,Wf,C] -> X [B, T*(n*n+1), ldx]
 * rows [feat(C), delimiter, target, 0 pad]; gts0 [B, n*n] = frame-0 heat-map
 * (nullable -> zeros). */
int ntk_gather_serialize(const float* fmap, const float* gts0, float* X, int B, int T,
                         int Hf, int Wf, int C, int ldx, int grid_start, int grid_step,
                         int grid_n, void* stream);

/* inference serialisation (quirk Q8, test_tracker.py:400-404): the delimiter row comes FIRST */
int ntk_gather_serialize_online(const float* fmap, const float* gts0, float* X, int B, int T,
                                int Hf, int Wf, int C, int ldx, int grid_start, int grid_step,
                                int grid_n, void* stream);

/* tf.image.crop_and_resize (bilinear, one normalised box y1,x1,y2,x2, extrapolation value) of (image - mean):
 * image [H,W,C] fp32, mean [C] (nullable) -> out [crop_h,crop_w,C]; crop_h * crop_w * C must stay below 2^31 - 256
 * (else NTK_ERR_BAD_SHAPE, as in the batched entry)
 * replaces: test_tracker.py:344-352 (online) / direct_offset_output.py:207-211 (training input pipeline) */
int ntk_crop_and_resize(const float* image, int H, int W, int C, const float* mean, float y1, float x1,
                        float y2, float x2, float* out, int crop_h, int crop_w, float extrapolation,
                        void* stream);

/* The same crop for B boxes in one launch, with boxes and frame indices read from DEVICE memory (the batched online tracker:
 * nothing comes back to the host between frames).  images [F,H,W,C], fp32 (dtype NTK_IMAGE_F32) or uint8 (NTK_IMAGE_U8, every
 * pixel converted to fp32 exactly); frame_of int32 [B]: tracker b reads frame frame_of[b] (several objects in one video share
 * an image, F = 1; separate clips of equal size have F = B) -- an index outside [0, F) is never dereferenced, that tracker's
 * crop is the extrapolation value everywhere; boxes fp32 [B,4] (y1,x1,y2,x2, normalised); mean [C] (nullable);
 * out [B,crop_h,crop_w,C].  Same box and same image give the same bits as ntk_crop_and_resize (one shared device function).
 * B <= 65535. */
#define NTK_IMAGE_F32 0
#define NTK_IMAGE_U8  1
int ntk_crop_and_resize_batch(const void* images, int dtype, int F, int H, int W, int C, const int* frame_of,
                              const float* boxes, const float* mean, float* out, int B, int crop_h, int crop_w,
                              float extrapolation, void* stream);

/* The training input of n frames in ONE launch: out[i] = crop_and_resize(resize_images(frame i, [resize_h, resize_w]) - mean,
 * boxes[i]) -> out fp32 [n,crop_h,crop_w,C], the composition direct_offset_output.py:193-211 performs per frame
 * (ntk_resize_bilinear, then ntk_crop_and_resize).  The resized image is never stored: each of the crop stage's four taps is
 * a pixel of the resized image computed from four source bytes (16 byte loads per output element), by the same two device
 * functions the single-stage kernels run.  flip_x != 0: output column x holds crop column crop_w-1-x (reverse_image, :203-204).
 * pixels: uint8, pixels_bytes long, the frames packed one after another, each of its own size; every pixel converted to fp32
 * exactly.  frame_table int64 [n,7], DEVICE memory, row i = byte_offset, H, W, y0, x0, h, w:
 *   H x W is the frame's FULL size -- all arithmetic uses it; (y0, x0, h, w) is the sub-rectangle of the frame that is present in
 *   `pixels`, row-major h*w*C bytes from byte_offset (any byte address: loads are single bytes, no alignment is assumed).
 *   Packing only the rectangle the crop can touch (data.crop_source_rect) gives the bits of packing the full frame.
 * No tap can fault: every source index is clamped into the row's rectangle before the load, and a row with h < 1 or w < 1, a
 * rectangle outside H x W, H or W outside 1..2^30, or bytes outside [0, pixels_bytes) is never dereferenced -- its crop is
 * `extrapolation` everywhere (the rule of ntk_crop_and_resize_batch for a frame index outside [0, F)).
 * boxes fp32 [n,4] (y1,x1,y2,x2 normalised, DEVICE memory); mean [C] (nullable).  Plain vector stores only.
 * Errors, before any launch: NTK_ERR_BAD_PTR for a null pixels / frame_table / boxes / out; NTK_ERR_BAD_SHAPE for n outside
 * 1..65535, C outside 1..4, resize_h / resize_w / crop_h / crop_w < 1, pixels_bytes < 1, or crop_h * crop_w * C >= 2^31 - 256. */
#define NTK_FRAME_TABLE_COLS 7
int ntk_frames_crop_batch(const unsigned char* pixels, long long pixels_bytes, const long long* frame_table, const float* boxes,
                          const float* mean, float* out, int n, int C, int resize_h, int resize_w, int crop_h, int crop_w,
                          int flip_x, float extrapolation, void* stream);

/* Baseline JPEG on the device (csrc/jpeg_parse.h, csrc/jpeg_entropy.h, csrc/jpeg_decode.hip): the host walks a file's markers and
 * removes the byte stuffing, the device decodes the Huffman stream, runs the inverse DCT, upsamples the chroma and converts the
 * colour with libjpeg's default integer pipeline -- the bits of Pillow's decode -- straight into the `pixels` buffer
 * ntk_frames_crop_batch reads.
 *
 * The domain of "the bits of Pillow's decode": streams whose dequantised coefficients are what a forward DCT of 8-bit samples
 * gives -- about +-1024 per coefficient, which every file from a real encoder keeps.  Outside it the two differ: Pillow's
 * libjpeg-turbo runs a SIMD inverse DCT that saturates 16-bit intermediates, the device keeps int32 throughout (libjpeg's C
 * code).  Measured (scripts/jpeg_domain_boundary.py): a quality-100 noise file with every quantisation value overwritten by q
 * decodes alike up to q = 12 (largest dequantised coefficient 2100) and differs from q = 13 on (2275).  Any table index 0..3,
 * Huffman code lengths up to 16, DC differences up to category 11, restart intervals, fill bytes and repeated DRI / DHT / DQT
 * segments (the last definition counts) are inside the domain.  One difference in what is accepted: a file whose scan is not
 * followed by EOI is an error to Pillow (decode="host" raises), while ntk_jpeg_parse accepts it and the device decodes what the
 * scan holds -- the whole image when only the marker is missing, NTK_JPEG_STATUS_TRUNCATED when the scan ends early.
 *
 * ntk_jpeg_parse (pure host code, thread-safe, no device-runtime call): file[file_bytes] -> one descriptor of NTK_JPEG_DESC_BYTES
 * bytes (nullable) and, when stream_dst is given, the scan's entropy-coded bytes with the stuffing removed (FF 00 -> FF), split at
 * the RSTn markers: segments[k] is the byte offset of segment k in stream_dst and segments[*n_segments] the end, so segment_cap
 * must be at least *n_segments + 1 and stream_cap at least *stream_bytes (both are reported with stream_dst = NULL, which writes
 * nothing but the descriptor; file_bytes always suffices for stream_cap).  The descriptor starts with NTK_JPEG_DESC_HDR_WORDS
 * int32 words (indices below; STREAM_OFF and WS_OFF are int64 at even words), then 4 dequantisation tables uint16 [64] in natural
 * order, then 4 DC + 4 AC Huffman tables (8-bit lookahead, maxcode / value offset per length, the values).  The caller sets
 * STREAM_OFF (byte offset of this frame's stream in the batch's stream buffer) and SEG_FIRST (index of its first segment entry).
 * Returns NTK_OK, NTK_JPEG_HOST_PATH (positive, not an error: the file is not for the device -- not a JPEG, not SOF0, not 8 bit,
 * 16-bit quantisation tables, several scans or a scan without all components, DNL, 4 components, sampling other than 1x1 / 2x1 /
 * 2x2 luma over 1x1 chroma, a colour space libjpeg would not read as YCbCr or gray, a side below NTK_JPEG_MIN_SIDE, restart
 * markers out of sequence or more of them than the MCU grid takes; the descriptor's NCOMP is then 0 and the device skips the
 * frame) or NTK_ERR_BAD_DATA for a malformed file (reason in ntk_last_error); no byte outside file[0, file_bytes) is read. */
#define NTK_ERR_BAD_DATA    -5
#define NTK_JPEG_HOST_PATH   1
#define NTK_JPEG_MIN_SIDE   16
#define NTK_JPEG_DESC_BYTES      7936
#define NTK_JPEG_DESC_HDR_WORDS  32
#define NTK_JPEG_DESC_H            0
#define NTK_JPEG_DESC_W            1
#define NTK_JPEG_DESC_NCOMP        2   /* 1 or 3; 0: not for the device */
#define NTK_JPEG_DESC_HS           3   /* luma sampling, horizontal (1 or 2) */
#define NTK_JPEG_DESC_VS           4   /* luma sampling, vertical (1 or 2) */
#define NTK_JPEG_DESC_RESTART      5   /* restart interval in MCUs, 0 = none */
#define NTK_JPEG_DESC_MCUS_X       6
#define NTK_JPEG_DESC_MCUS_Y       7
#define NTK_JPEG_DESC_NSEG         8
#define NTK_JPEG_DESC_SEG_FIRST    9
#define NTK_JPEG_DESC_STREAM_OFF  10   /* int64 */
#define NTK_JPEG_DESC_WS_OFF      12   /* int64, set by ntk_jpeg_decode_workspace_bytes */
#define NTK_JPEG_DESC_STREAM_BYTES 14
#define NTK_JPEG_DESC_TQ          16   /* [3] dequantisation table of each component */
#define NTK_JPEG_DESC_TD          19   /* [3] DC table */
#define NTK_JPEG_DESC_TA          22   /* [3] AC table */
int ntk_jpeg_parse(const unsigned char* file, long long file_bytes, void* desc, unsigned char* stream_dst, long long stream_cap,
                   int* segments, int segment_cap, long long* stream_bytes, int* n_segments);

/* Workspace of a batch, computed on the HOST from host copies of the descriptors [n] and the frame table [n,7]: per device frame
 * the int16 coefficients and the uint8 planes of the MCU window its rectangle needs (the rectangle widened by the one chroma
 * sample per side the triangle upsampling reads, rounded out to MCUs: NTK_JPEG_WS_BYTES_PER_BLOCK per 8x8 block).  Writes each
 * frame's offset into its descriptor (WS_OFF) -- upload the descriptors after this call -- and returns the total in *bytes.
 * NTK_ERR_BAD_SHAPE for n outside 1..65535 or a rectangle outside its frame, NTK_ERR_BAD_PTR for a null pointer. */
#define NTK_JPEG_WS_BYTES_PER_BLOCK 192
int ntk_jpeg_decode_workspace_bytes(void* descs_host, const long long* frame_table_host, int n, long long* bytes);

/* Decode n frames on `stream`: row i's rectangle (frame_table as in ntk_frames_crop_batch, C = 3) is written as h*w*3 RGB bytes
 * at byte_offset of `pixels`; a gray file gives Y in all three channels.  All pointers are DEVICE memory: streams (the unstuffed
 * scans), descs [n] (NTK_JPEG_DESC_BYTES each), segments int32 [n_segments], frame_table int64 [n,7], workspace, status int32 [n].
 * Three launches: one wave per frame decodes the Huffman stream (lane l takes restart segments l, l+64, ...; only the window's
 * blocks are stored, and decoding stops after the window's last MCU row), then dequantisation + inverse DCT into planes, then
 * upsampling + colour into the rectangle.  Plain vector stores only.  The entry allocates nothing: it clears workspace_bytes of
 * `workspace` and `status` on the stream and launches.  status[i]: NTK_JPEG_STATUS_*; a frame with a non-zero status has
 * unspecified bytes in its own rectangle and nothing else is touched.  No access rests on trust in the file's bytes:
 * every stream read is clamped to its segment, every coefficient index is checked, MCU counts come from the descriptor, and a
 * frame whose descriptor, segment entries, rectangle, pixel bytes or workspace range leave the sizes given here is skipped with
 * NTK_JPEG_STATUS_BAD_DESC / _WORKSPACE.  A descriptor with NCOMP = 0 is skipped with status 0 (a frame the host decoded).
 * Errors, before any launch: NTK_ERR_BAD_PTR for a null pointer; NTK_ERR_BAD_SHAPE, the value named in ntk_last_error, for n
 * outside 1..65535, streams_bytes / n_segments / pixels_bytes < 1, or workspace_bytes < n * NTK_JPEG_WS_BYTES_PER_BLOCK (no frame
 * needs less than one block). */
#define NTK_JPEG_STATUS_OK         0
#define NTK_JPEG_STATUS_BAD_CODE   1   /* a bit pattern no Huffman code matches, or a coefficient index past 63 */
#define NTK_JPEG_STATUS_TRUNCATED  2   /* a segment ended before its MCUs were decoded */
#define NTK_JPEG_STATUS_WORKSPACE  3
#define NTK_JPEG_STATUS_BAD_DESC   4
#define NTK_JPEG_STATUS_SEGMENTS   5   /* fewer restart segments than the window's MCUs need */
int ntk_jpeg_decode_batch(const unsigned char* streams, long long streams_bytes, const void* descs, const int* segments,
                          long long n_segments, const long long* frame_table, unsigned char* pixels, long long pixels_bytes,
                          void* workspace, long long workspace_bytes, int* status, int n, void* stream);

/* Per-frame box bookkeeping of the online tracker (test_tracker.py:274-329) for B trackers on the device, one thread per
 * tracker; the offsets are the fp32 tanh the single tracker takes and the shifted box is the fp32 sum it forms, everything after that is double precision.  Box state: double [B, NTK_TRACK_STATE_DOUBLES], per tracker
 *   [0] image width w   [1] image height h   [2..5] normalised object box (y1,x1,y2,x2)   [6..9] crop box (y1,x1,y2,x2)
 * logits fp32 [B,S,2]: the step read is the LAST one (quirk Q8).  Per active tracker: offsets (dy,dx) = tanh(logits[b,S-1,:]);
 * the centred box 0.5 -+ bbox_grid / (2 cropbox_grid) shifted by them; decoded through the inverse of the crop transformation
 * of the crop box in the state; scaled by (w, h) (not (w-1, h-1): the reference's asymmetry is kept); the region
 * (x, y, width, height) -> regions double [B,4]; then the state for the next frame: a region whose four numbers are all < 1 is
 * taken as already normalised (test_tracker.py:306-309), else divided by (h-1, w-1); crop box = that box scaled about its
 * centre by cropbox_grid / bbox_grid.  Writes regions, offsets fp32 [B,2], state[2..9], the crop box a second time as
 * cropbox32 fp32 [B,4] (what ntk_crop_and_resize_batch reads) and frame[b] += 1 (int32 [B], nullable).
 * active uint8 [B] (nullable = all active): NOTHING of an inactive tracker is written. */
#define NTK_TRACK_STATE_DOUBLES 10
#define NTK_TRACK_STATE_W        0
#define NTK_TRACK_STATE_H        1
#define NTK_TRACK_STATE_BBOX     2
#define NTK_TRACK_STATE_CROPBOX  6
int ntk_track_boxes_update(const float* logits, int B, int S, double cropbox_grid, double bbox_grid,
                           const unsigned char* active, double* state, float* cropbox32, double* regions,
                           float* offsets, int* frame, void* stream);

/* Per-clip tracking scores accumulated on the device, so that a validation run reads one table back at its end instead of the
 * regions after every round.  A small bookkeeping kernel, not a compute hot path: one thread per slot b walks its T frames in
 * order and adds to row clip_of[b] of the table; a clip's sums are therefore added in frame order and are reproducible bit
 * for bit, and T one-frame calls leave the same bits as one T-frame call.
 *   regions, gt  double [T,B,4] (x, y, w, h) in pixels: what BatchNTMTracker.track_clip returns, and the ground truth
 *   active       uint8 [T,B], nullable = every frame active
 *   clip_of      int32 [B]: the table row of slot b.  A row outside [0, n_clips) skips the slot: nothing of it is read or
 *                written but clip_of[b] (and its frame_iou entries, NaN).  NO TWO SLOTS MAY NAME THE SAME ROW IN ONE CALL: each
 *                thread owns its row without atomics, and two slots on one row would lose counts.  (ntmtrack.evaluate.ClipSchedule
 *                never gives two slots one clip.)
 *   iou_thr [n_iou], dist_thr [n_dist]: double thresholds in device memory; a count may be 0, then its array may be null
 *   table        double [n_clips, NTK_SCORE_HEAD + n_iou + n_dist], accumulated IN PLACE; row layout, every field a double and
 *                every count an exact integer:
 *     [NTK_SCORE_FRAMES]      frames scored
 *     [NTK_SCORE_SUM_IOU]     sum of their IoUs
 *     [NTK_SCORE_SUM_DIST]    sum of the distances between the centres, pixels
 *     [NTK_SCORE_LOST]        frames with IoU == 0
 *     [NTK_SCORE_FIRST_LOST]  the value of FRAMES when the first lost frame arrived (= the number of frames scored before
 *                             it), -1 while the clip has none: THE OWNER INITIALISES THIS FIELD TO -1, every other field to 0
 *     [NTK_SCORE_HEAD + k]          k < n_iou:  frames with IoU > iou_thr[k]  (strictly, as OTB counts success)
 *     [NTK_SCORE_HEAD + n_iou + k]  k < n_dist: frames with centre distance <= dist_thr[k]  (precision)
 *   frame_iou    double [T,B], nullable: the frame's IoU, NaN where the frame was not scored
 * A frame is scored when it is active and its ground truth is finite with w > 0 and h > 0 (an absent object is written with a
 * non-finite or empty box); any other frame changes nothing.  A predicted region that is not finite scores IoU 0 and counts as
 * lost; it adds nothing to SUM_DIST and to no precision count (its distance is taken as infinite).  Negative predicted sizes are
 * clamped to 0.
 * Arithmetic: float64 on real-valued rectangles, the VOT / OTB overlap |A n B| / |A u B| without a +1 pixel convention.  Boxes
 * are taken to corners (x, x + w) and every side is a difference of corners, products are not contracted into FMAs and the
 * result is clamped to [0, 1]: a box against itself gives exactly 1.0, boxes that only touch exactly 0.0, and integer-valued
 * boxes the bits of any IEEE evaluation of (ix iy) / ((ap + ag) - ix iy).
 * Errors, before any launch: NTK_ERR_BAD_PTR for a null regions / gt / clip_of / table; NTK_ERR_BAD_SHAPE, the value named in
 * ntk_last_error, for T, B or n_clips <= 0, B > 65535, a count < 0 or > NTK_SCORE_MAX_THRESHOLDS, or a count > 0 with a null
 * threshold array. */
#define NTK_SCORE_FRAMES      0
#define NTK_SCORE_SUM_IOU     1
#define NTK_SCORE_SUM_DIST    2
#define NTK_SCORE_LOST        3
#define NTK_SCORE_FIRST_LOST  4
#define NTK_SCORE_HEAD        5
#define NTK_SCORE_MAX_THRESHOLDS 256
int ntk_track_overlap_scores(const double* regions, const double* gt, const unsigned char* active, const int* clip_of,
                             int T, int B, int n_clips, const double* iou_thr, int n_iou, const double* dist_thr, int n_dist,
                             double* table, double* frame_iou, void* stream);

/* First-frame geometry of the online tracker on the device, for the slots that are (re)started on this frame: what
 * BatchNTMTracker computes on the host when a tracker is made or reset (test_tracker.py:300-329 and :370-405), masked per slot,
 * so that a restart costs no second pass and no host arithmetic.  A small bookkeeping kernel: one thread per slot, plain vector
 * stores, float64 without FMA contraction in the operation order of ntmtrack/geometry.py.
 *   regions_in  double [B,4] (x, y, w, h) in pixels; a region whose four numbers are all < 1 is taken as already normalised
 *               (test_tracker.py:306-309), any other is divided by (H-1, W-1) (normalize_bbox)
 *   restart     uint8 [B]
 *   active      uint8 [B], nullable = all active: read only to form the two masks below
 *   state       double [B, NTK_TRACK_STATE_DOUBLES]: W and H are read
 *   cropbox_grid, bbox_grid, sigma: sigma as generate_gt computes it (integer division of bbox_grid by the focus included);
 *               cropbox_grid must be a whole number g, the heat-map grid is g x g and gts_width must be g * g
 * A slot with restart[b] != 0: the crop box is the object box scaled about its centre by cropbox_grid / bbox_grid
 * (calculate_cropbox); state[2..9], cropbox32 fp32 [B,4], regions double [B,4] (= the region given), offsets fp32 [B,2] = 0 and
 * frame int32 [B] = 0 are written; gts0 fp32 [B, g*g] gets the heat-map row: the object box through the transformation that maps
 * the crop box to the unit square (apply_transformation), exp(-r^2 / 2 sigma^2) at the cell centres of the grid about the box
 * centre, values below eps * max dropped, normalised to sum 1 (discrete_gauss), cast to fp32.
 * A slot with restart[b] == 0: its gts0 row is written as zeros (what ntk_gather_serialize_online takes a null gts0 for: the row
 * serialises to the same bits) and NOTHING else of it is written.
 * run_mask, move_mask uint8 [B], both nullable, written for every slot: run_mask = active | restart (the slots whose recurrent
 * state the frame's sequence advances), move_mask = active & ~restart (the slots whose output moves their box: the output of a
 * first-frame pass is discarded).
 * Errors, before any launch: NTK_ERR_BAD_PTR for any other null pointer; NTK_ERR_BAD_SHAPE, the value named in ntk_last_error,
 * for B outside 1..65535, a grid or sigma <= 0, a cropbox_grid that is not whole or above 1024, gts_width != g * g. */
int ntk_track_restart_boxes(const double* regions_in, const unsigned char* restart, const unsigned char* active, int B,
                            double cropbox_grid, double bbox_grid, double sigma, int gts_width, double* state, float* cropbox32,
                            double* regions, float* offsets, int* frame, float* gts0, unsigned char* run_mask,
                            unsigned char* move_mask, void* stream);

/* The supervised protocol on the device: a tracker that has lost its object is started again from the ground truth a few frames
 * later, accuracy is the mean overlap outside a burn-in after every start, robustness the number of failures.  The model is the
 * behaviour of the VOT toolkit's supervised experiment.  Nothing in the reference pins these rules (its vot.py only hands regions
 * to the toolkit, which does the restarts itself): THE RULES BELOW ARE THE CONTRACT.
 * One call is one phase of ONE frame for B slots, one thread per slot; a frame is plan, the tracker's pass, judge.
 *   state    int32 [B, NTK_SUP_STATE_INTS]: [NTK_SUP_STATE_MODE] NTK_SUP_MODE_TRACK / NTK_SUP_MODE_WAIT, [NTK_SUP_STATE_COUNTDOWN]
 *            frames until the restart, [NTK_SUP_STATE_SINCE] frames tracked since the last start.  A clip's frame 0 starts the
 *            slot and counts as a start: THE OWNER SETS THE ROW TO (TRACK, 0, 0) when a slot takes a new clip.
 *   table    double [n_clips, NTK_SUP_HEAD], row clip_of[b], accumulated in place; every field a double, every count exact:
 *     [NTK_SUP_VALID]          frames that count towards accuracy
 *     [NTK_SUP_SUM_IOU]        sum of their overlaps, added in frame order
 *     [NTK_SUP_FAILURES]       [NTK_SUP_RESTARTS]
 *     [NTK_SUP_TRACKED]        frames judged
 *     [NTK_SUP_SKIPPED]        frames a slot sat out while it waited
 *     [NTK_SUP_FIRST_FAILURE]  the value of TRACKED when the first failure arrived; THE OWNER INITIALISES IT TO -1, the rest to 0
 *   clip_of  int32 [B]: as for ntk_track_overlap_scores -- a row outside [0, n_clips) skips the slot (code -1 in plan, nothing
 *            in judge), and NO TWO SLOTS MAY NAME ONE ROW
 *   gt       double [B,4] (x, y, w, h): this frame's ground truth; valid = finite with w > 0 and h > 0
 * phase NTK_SUP_PLAN, before the pass (active uint8 [B], nullable = all active; writes track and restart uint8 [B], every entry):
 *   an inactive slot: code -1, track = restart = 0, nothing else.
 *   mode TRACK: track[b] = 1 (code 0 until judge has seen the frame).
 *   mode WAIT: countdown = max(countdown - 1, 0); then, if countdown == 0 and the ground truth is valid: restart[b] = 1,
 *     RESTARTS += 1, mode TRACK, since = 0, code 1 -- the caller hands restart and this gt to ntk_track_restart_boxes;
 *     otherwise the slot sits the frame out: SKIPPED += 1, code 3 (a slot whose object is absent on its restart frame waits for
 *     the first frame that has one).
 * phase NTK_SUP_JUDGE, after the pass (regions double [B,4]: the tracked regions; track as plan wrote it), slots with track != 0:
 *   ground truth not valid: since += 1, code 0, counted nowhere.
 *   otherwise o = the overlap of ntk_track_overlap_scores (the same device function: corners first, no FMA contraction, clamped
 *     to [0,1], touching boxes exactly 0; a prediction that is not finite scores 0, negative sizes are clamped to 0);
 *     TRACKED += 1; if o <= failure_overlap: FAILURES += 1, FIRST_FAILURE set if it was < 0, code 2, mode WAIT, countdown = skip;
 *     else since += 1 and, when since > burn_in, VALID += 1 and SUM_IOU += o; code 0.
 * So a slot that fails on frame f is restarted on frame f + skip (or the first later frame with an object) and is judged again
 * from the frame after that.  codes int8 [B] and frame_iou double [B] are nullable: plan writes every code and fills frame_iou
 * with NaN, judge overwrites both for the slots it judged.  Frames are separate calls, so any split of a clip into calls leaves
 * the same bits.
 * Errors, before any launch: NTK_ERR_BAD_SHAPE, the value named in ntk_last_error, for a phase other than the two, B outside
 * 1..65535, n_clips <= 0, skip < 1, burn_in < 0, failure_overlap outside [0,1); NTK_ERR_BAD_PTR for a null gt / clip_of / state /
 * table / track, a null restart in plan, a null regions in judge. */
#define NTK_SUP_PLAN   0
#define NTK_SUP_JUDGE  1
#define NTK_SUP_STATE_INTS       3
#define NTK_SUP_STATE_MODE       0
#define NTK_SUP_STATE_COUNTDOWN  1
#define NTK_SUP_STATE_SINCE      2
#define NTK_SUP_MODE_TRACK  0
#define NTK_SUP_MODE_WAIT   1
#define NTK_SUP_VALID          0
#define NTK_SUP_SUM_IOU        1
#define NTK_SUP_FAILURES       2
#define NTK_SUP_RESTARTS       3
#define NTK_SUP_TRACKED        4
#define NTK_SUP_SKIPPED        5
#define NTK_SUP_FIRST_FAILURE  6
#define NTK_SUP_HEAD           7
#define NTK_SUP_CODE_INACTIVE (-1)
#define NTK_SUP_CODE_TRACKED   0
#define NTK_SUP_CODE_RESTART   1
#define NTK_SUP_CODE_FAILURE   2
#define NTK_SUP_CODE_SKIPPED   3
int ntk_track_supervise(int phase, const double* regions, const double* gt, const unsigned char* active, const int* clip_of, int B,
                        int n_clips, int skip, int burn_in, double failure_overlap, int* state, double* table,
                        unsigned char* track, unsigned char* restart, signed char* codes, double* frame_iou, void* stream);

/* Polygon ground truth (VOT regions: vot.py:27-33 reads a region line as a rectangle or as a polygon; the VOT sets from 2015 on
 * annotate every frame with a rotated rectangle of four points).  One layout everywhere: a region is double[NTK_POLY_DOUBLES], the
 * vertices (x0, y0, x1, y1, ...) in pixels.  The vertices used are the LEADING pairs whose two numbers are both finite, at most
 * NTK_POLY_MAX_POINTS; the rest is NaN padding.  Either orientation is accepted.  THE POLYGON MUST BE SIMPLE (no
 * self-intersection): the area of a self-intersecting one is not what the shoelace sum gives, and its overlap is not defined here.
 * A region is PRESENT when it has at least 3 vertices, its bounding rectangle has w > 0 and h > 0 and its shoelace area is > 0;
 * anything else is an absent object, exactly as a non-finite or empty box is for the rectangle entries.
 *
 * ntk_track_poly_bounds: poly double [n,NTK_POLY_DOUBLES] -> rects double [n,4] = (min x, min y, max x - min x, max y - min y)
 * over the used vertices: the rectangle vot.py:49-61 (convert_region) hands a tracker that asked for rectangles, and so what a
 * tracker is (re)started with.  ONE DIFFERENCE: the reference seeds its maxima with sys.float_info.min, the smallest POSITIVE
 * double, and is therefore wrong for a polygon whose coordinates are all <= 0; here the true maximum is taken.  An absent region
 * gives four NaNs.  One thread per region, plain vector stores.  Errors: NTK_ERR_BAD_PTR for a null pointer, NTK_ERR_BAD_SHAPE
 * (n named) for n <= 0.
 *
 * ntk_track_overlap_scores_poly: ntk_track_overlap_scores with gt double [T,B,NTK_POLY_DOUBLES].  Table layout, skip rules ("ground
 * truth finite with w > 0 and h > 0" reads "present"), thresholds, frame_iou, row ownership, frame-order accumulation and the
 * error checks are those of ntk_track_overlap_scores.  The overlap is |P n R| / (|P| + |R| - |P n R|), R the predicted rectangle
 * (negative sizes clamped to 0), P the polygon, in float64 without FMA contraction, clamped to [0,1]: P is clipped against the four
 * sides of R in turn (Sutherland-Hodgman, strict inside tests, a crossing point given the side's own coordinate exactly) and the
 * shoelace area of the rest is |P n R|.  So a convex polygon whose interior does not reach R's interior -- touching included --
 * scores exactly 0.0, and an integer-valued axis-aligned 4-gon against an integer rectangle gives the bits of
 * ntk_track_overlap_scores on the two boxes (1.0 against itself).  The centre distance is taken to the centre of the polygon's
 * bounding rectangle (that of ntk_track_poly_bounds).
 *
 * ntk_track_supervise_poly: ntk_track_supervise with gt double [B,NTK_POLY_DOUBLES]; "valid ground truth" reads "present", the
 * judge's overlap is the device function of ntk_track_overlap_scores_poly, every other rule and every error check is unchanged.
 * The caller hands the restarted slots' ntk_track_poly_bounds rectangles to ntk_track_restart_boxes. */
#define NTK_POLY_MAX_POINTS 8
#define NTK_POLY_DOUBLES    16
int ntk_track_poly_bounds(const double* poly, int n, double* rects, void* stream);
int ntk_track_overlap_scores_poly(const double* regions, const double* gt, const unsigned char* active, const int* clip_of,
                                  int T, int B, int n_clips, const double* iou_thr, int n_iou, const double* dist_thr, int n_dist,
                                  double* table, double* frame_iou, void* stream);
int ntk_track_supervise_poly(int phase, const double* regions, const double* gt, const unsigned char* active, const int* clip_of,
                             int B, int n_clips, int skip, int burn_in, double failure_overlap, int* state, double* table,
                             unsigned char* track, unsigned char* restart, signed char* codes, double* frame_iou, void* stream);

/* Segmentation-mask ground truth (the VOT short-term sets from 2020 on annotate every frame with a run-length coded mask, the
 * line "m x0,y0,w,h,c0,c1,..." of groundtruth.txt).  The tracker still emits rectangles: a mask is scored against the tracker's
 * rectangle, the way the VOT toolkit scores a rectangle tracker on a mask set.  Nothing in the reference reads masks (its vot.py
 * predates them) and the toolkit is not part of this project: THE RULES BELOW ARE THE CONTRACT.  They are modelled on the
 * toolkit's behaviour; THE RULE THAT RASTERISES A FRACTIONAL RECTANGLE IS THE PROJECT'S OWN.
 *
 * A set of n masks on the device:
 *   cells  int32 [n, NTK_MASK_CELL_INTS]: one mask is (x0, y0, w, h, first, count): (x0, y0, w, h) its box in frame pixels,
 *          first and count name its counts rle[first, first + count)
 *   rle    int32 [n_rle]: the toolkit's counts as they are.  Even-indexed counts (the first is index 0) are runs of zeros,
 *          odd-indexed counts runs of ones, in row-major order over the w x h box.  Pixels the counts do not reach are zero;
 *          pixels the counts run past w h are dropped (as NumPy's slice assignment drops them).
 * A mask is PRESENT when w > 0, h > 0 and w h <= NTK_MASK_MAX_PIXELS; first >= 0, count >= 0 and first + count <= n_rle; every
 * count is >= 0; and at least one pixel inside the box is set.  Anything else is an absent object, exactly as a non-finite or
 * empty box is for the rectangle entries.  The kernels stay inside rle[0, n_rle) for ANY contents of cells.
 * One 64-lane workgroup handles one mask and the counts are never rasterised: the workgroup walks the counts 64 at a time, a
 * wave inclusive scan plus a carry gives every run its start s, and a run of ones [s, s + len), clipped to w h, is handled in
 * closed form, in integer arithmetic: |M| gains len; the run bounds rows s / w .. (s + len - 1) / w, and columns s % w ..
 * (s + len - 1) % w when it lies in one row, 0 .. w - 1 when it crosses a row end; |M n R| gains the first partial row, the last
 * partial row and (middle rows inside R's rows) x (R's columns inside the box).  The sums are reduced across the wave; plain
 * vector stores, no atomics.
 *
 * THE PIXEL SET OF A PREDICTED RECTANGLE (x, y, w, h): negative sizes are clamped to 0 and the rectangle is taken to corners
 * first (x2 = x + w), like every other overlap here.  Pixel (c, r) belongs to it when its centre (c + 0.5, r + 0.5) lies in
 * [x, x2) x [y, y2): the columns ceil(x - 0.5) .. ceil(x2 - 0.5) - 1, the rows by the same rule, so an integer rectangle covers
 * exactly its w h pixels.  |R| is the product of the two counts as doubles (no FMA contraction).  The rectangle is NOT clipped to
 * the frame, as for rectangles and polygons.  A rectangle that is not finite has |R| = |M n R| = 0.
 *
 * ntk_track_mask_bounds: rects double [n,4] = (min col, min row, max col + 1 - min col, max row + 1 - min row) over the set
 * pixels, in frame pixels, and area double [n] = |M|; an absent mask gives four NaNs and a NaN area.  This rectangle starts and
 * restarts a tracker, and the centre distance is taken to its centre.
 * ntk_track_mask_overlaps: regions double [n,4] -> overlap double [n, NTK_MASK_OVERLAP_DOUBLES] = (|M n R|, |R|, |M|) per mask,
 * every value an exact integer held in a double; an absent mask gives NaNs.
 * Errors of both, before any launch: NTK_ERR_BAD_PTR for a null pointer; NTK_ERR_BAD_SHAPE, the values named in ntk_last_error,
 * for n <= 0 or n_rle < 0.
 *
 * ntk_track_overlap_scores_mask: ntk_track_overlap_scores with gt replaced by rects double [T,B,4] (ntk_track_mask_bounds) and
 * overlap double [T,B,NTK_MASK_OVERLAP_DOUBLES] (ntk_track_mask_overlaps of the regions).  "Ground truth finite with w > 0 and
 * h > 0" is read on rects; the overlap is I / ((R + M) - I), one float64 division, and 0.0 when I == 0 (a prediction that is not
 * finite scores 0 as everywhere); the centre distance goes to the centre of rects.  Table layout, skip rules, thresholds,
 * frame_iou, row ownership, frame-order accumulation and the error checks (a null overlap included) are those of
 * ntk_track_overlap_scores.  A filled integer rectangle as a mask, against an integer prediction, leaves the bits of
 * ntk_track_overlap_scores on the two boxes.
 * ntk_track_supervise_mask: ntk_track_supervise with gt replaced by rects double [B,4] and overlap double
 * [B,NTK_MASK_OVERLAP_DOUBLES]; overlap is read by judge only and may be null in plan.  Every other rule and every error check
 * is unchanged.  The caller hands the restarted slots' rects to ntk_track_restart_boxes. */
#define NTK_MASK_CELL_INTS        6
#define NTK_MASK_OVERLAP_DOUBLES  3
#define NTK_MASK_MAX_PIXELS       (1 << 30)
int ntk_track_mask_bounds(const int* cells, const int* rle, int n_rle, int n, double* rects, double* area, void* stream);
int ntk_track_mask_overlaps(const double* regions, const int* cells, const int* rle, int n_rle, int n, double* overlap,
                            void* stream);
int ntk_track_overlap_scores_mask(const double* regions, const double* rects, const double* overlap, const unsigned char* active,
                                  const int* clip_of, int T, int B, int n_clips, const double* iou_thr, int n_iou,
                                  const double* dist_thr, int n_dist, double* table, double* frame_iou, void* stream);
int ntk_track_supervise_mask(int phase, const double* regions, const double* rects, const double* overlap,
                             const unsigned char* active, const int* clip_of, int B, int n_clips, int skip, int burn_in,
                             double failure_overlap, int* state, double* table, unsigned char* track, unsigned char* restart,
                             signed char* codes, double* frame_iou, void* stream);

/* The multi-start (anchor-based) protocol of the VOT sets from 2020 on: a tracker is started at an anchor frame and run ONCE to an
 * end of its sequence, a run ends when the overlap stays low, and the figures are accuracy, robustness and the expected average
 * overlap (EAO).  A RUN is a clip to the validator (its frames in run order, built on the host); these entries score the rounds of
 * the runs and reduce the result.  The rules are this project's statement of the protocol after the wording of the VOT2020
 * report; where the report is silent the choice is marked (own rule).  No bit parity with the toolkit is claimed.
 *
 * ntk_track_multistart: one launch per round, one thread per slot, which walks its T frames in order.  ALL protocol state lives
 * in the run's table row, which belongs to the slot that holds the run (NO TWO SLOTS MAY NAME ONE ROW): no per-slot state, no
 * atomics, plain vector loads and stores; a slot that takes another run in a later round names another row.
 *   regions, gt, active, clip_of, T, B, frame_iou: as for ntk_track_overlap_scores; clip_of[b] is the RUN of slot b, a row
 *     outside [0, n_runs) skips the slot (only clip_of[b] is read; its frame_iou is NaN)
 *   table        double [n_runs, NTK_MS_HEAD], THE OWNER INITIALISES IT TO 0; every field a double, every count exact:
 *     [NTK_MS_FRAMES]   N: the scored frames of the run so far, those after a failure included
 *     [NTK_MS_TRACKED]  scored frames committed: the ordinal at which the open streak began, or FRAMES when none is open.  Of a
 *                       failed run it is the failure's ordinal f = N_F
 *     [NTK_MS_SUM_IOU]  sum of the committed frames' overlaps, added in frame order
 *     [NTK_MS_FAILED]   0 / 1
 *     [NTK_MS_LOW]      length of the open streak of low frames (0 <= LOW <= patience; 0 once the run has failed)
 *     [NTK_MS_PENDING]  what SUM_IOU becomes if the open streak is forgiven: SUM_IOU and then the streak's overlaps, added in
 *                       frame order.  Equal to SUM_IOU when no streak is open.
 *   trace_first  int64 [n_runs + 1], ascending: the run's overlaps are trace[trace_first[r] : trace_first[r + 1]]
 *   trace        double [trace_first[n_runs]]: the overlap of the run's scored frame of ordinal i goes to trace[trace_first[r]
 *                + i]; an ordinal that would reach trace_first[r + 1] is counted and NOT stored (a run of L frames needs L - 1)
 * A SCORED frame is active, has ground truth present (the rule of ntk_track_overlap_scores for the kind of ground truth) and gets
 * the overlap o of ntk_track_overlap_scores: the same device function, the same bits.  An inactive frame, or one whose ground
 * truth is absent, does not exist for the protocol (own rule): it gets no ordinal and neither extends nor breaks a streak.  With
 * i = FRAMES the ordinal of a scored frame, in order:
 *   trace[...] = o, frame_iou = o, FRAMES += 1; a run that has FAILED takes nothing more;
 *   o <= failure_overlap (LOW frame, the supervised protocol's <=): LOW += 1, PENDING += o; when LOW == patience + 1 the run has
 *     FAILED at ordinal f = TRACKED: frames f ... f + patience are all low.  FAILED = 1, LOW = 0, PENDING = SUM_IOU;
 *   otherwise the streak, if any, is forgiven and its frames count normally: PENDING += o, SUM_IOU = PENDING, TRACKED += LOW + 1,
 *     LOW = 0.
 * A streak still open when the run ends is not a failure (own rule), so of a finished run
 *   N = FRAMES, N_F = FAILED ? TRACKED : FRAMES, sum = FAILED ? SUM_IOU : PENDING = the sum of o_i over i < N_F in frame order,
 *   accuracy = sum / N_F (NaN for N_F = 0), robustness = N_F / N; a run with N = 0 takes part in nothing.
 * Rounds are separate calls and the row carries everything, so any split of a run's frames into calls leaves the same bits.
 * ntk_track_multistart_poly: gt double [T,B,NTK_POLY_DOUBLES]; ntk_track_multistart_mask: rects and overlap as for
 * ntk_track_overlap_scores_mask.  Everything else is unchanged.
 * Errors, before any launch: NTK_ERR_BAD_PTR for a null regions, gt / rects, overlap (mask), clip_of, table, trace_first or trace
 * (active and frame_iou are nullable); NTK_ERR_BAD_SHAPE, the value named in ntk_last_error, for T, B or n_runs <= 0, B > 65535,
 * patience < 0 or failure_overlap outside [0,1).
 *
 * ntk_track_eao_curve: the EAO curve of the finished runs, on the device (a long-term-sized set holds 1e8 trace entries: neither
 * the trace nor the reduction goes to the host).  With o^_s(i) = o_i for i < N_F and 0 afterwards -- of a failed run without end,
 * the report's "padded with zeros" -- and S_n = the failed runs and the unfailed runs with N >= n (runs with N = 0 never):
 *   curve[n - 1] = Phi(n) = (1 / |S_n|) sum over s in S_n of (1 / n) sum over i < n of o^_s(i), n = 1 ... n_max; NaN for an empty S_n.
 * Two kernels: (a) one 64-lane wavefront per run turns its o_i, i < min(N_F, n_max), into inclusive prefix sums in prefix (the
 * layout of trace, caller-provided, nothing stored beyond): chunks of 64 frames, a wave scan and a carried total; (b) one thread
 * per n adds P_s(min(n, N_F)) / n over the runs of S_n in run order.  Fixed orders and no atomics: the same input gives the same
 * bits.  N_F is cut to the run's trace length.  prefix double [trace_first[n_runs]], curve double [n_max].
 * Errors: NTK_ERR_BAD_PTR for any null pointer; NTK_ERR_BAD_SHAPE, the value named, for n_runs <= 0 or n_max <= 0. */
#define NTK_MS_FRAMES   0
#define NTK_MS_TRACKED  1
#define NTK_MS_SUM_IOU  2
#define NTK_MS_FAILED   3
#define NTK_MS_LOW      4
#define NTK_MS_PENDING  5
#define NTK_MS_HEAD     6
int ntk_track_multistart(const double* regions, const double* gt, const unsigned char* active, const int* clip_of, int T, int B,
                         int n_runs, double failure_overlap, int patience, double* table, const long long* trace_first,
                         double* trace, double* frame_iou, void* stream);
int ntk_track_multistart_poly(const double* regions, const double* gt, const unsigned char* active, const int* clip_of, int T,
                              int B, int n_runs, double failure_overlap, int patience, double* table,
                              const long long* trace_first, double* trace, double* frame_iou, void* stream);
int ntk_track_multistart_mask(const double* regions, const double* rects, const double* overlap, const unsigned char* active,
                              const int* clip_of, int T, int B, int n_runs, double failure_overlap, int patience, double* table,
                              const long long* trace_first, double* trace, double* frame_iou, void* stream);
int ntk_track_eao_curve(const double* table, const long long* trace_first, const double* trace, int n_runs, int n_max,
                        double* prefix, double* curve, void* stream);

/* Validation from image files decoded on the device (ntk_jpeg_decode_batch): which frames of a round may be tracked and scored.
 * A file can turn out undecodable only on the device; this entry turns such a frame off in the round's mask before the tracker
 * and the scoring launch read it, so that nothing is read back per round.  One launch per round, one thread per slot, which
 * walks its T frames in order; a table row belongs to its slot's thread alone (NO TWO SLOTS MAY NAME ONE ROW), so there are no
 * atomics: plain vector loads and stores.
 *   status       int32 [n_status]: the decoder's NTK_JPEG_STATUS_* per file of the round
 *   cell_index   int32 [T,B]: the file of cell (t, b) as an index into status; -1 = the cell has no device-decoded file, its
 *                status is 0.  An index >= n_status counts as NTK_JPEG_STATUS_BAD_DESC: nothing outside status is read.
 *   start_index  int32 [B]: the index of the slot's starting frame if the slot was reset this round, else -1
 *   clip_of      int32 [B]: the table row of slot b; a row outside [0, n_clips) leaves everything of the slot as it is
 *   dead         uint8 [B], in/out: the slot's clip started from an undecodable frame.  Written when start_index[b] >= 0
 *                (dead = the starting frame's status != 0, which also goes to START_STATUS), carried over rounds otherwise.
 *   active       uint8 [T,B], in/out.  For each t in order with active[t,b] != 0: a dead slot -> active = 0, MASKED += 1;
 *                else a status != 0 -> active = 0, FAILED += 1 and, while FIRST_FAILED < 0, FIRST_FAILED = DECODED + FAILED +
 *                MASKED as they stood before this frame and FIRST_STATUS = the status; else DECODED += 1.
 *   table        int64 [n_clips, NTK_CLIPDEC_HEAD], accumulated in place: THE OWNER INITIALISES FIRST_FAILED TO -1, the rest to 0.
 * Rounds are separate calls and the row carries the counts, so any split of a clip's frames into calls leaves the same bits.
 * Errors, before any launch: NTK_ERR_BAD_PTR for any null pointer; NTK_ERR_BAD_SHAPE, the value named in ntk_last_error, for T,
 * B, n_clips or n_status <= 0 or B > 65535. */
#define NTK_CLIPDEC_DECODED       0  /* active frames of the clip whose pixels are good (status 0, or no device file) */
#define NTK_CLIPDEC_FAILED        1  /* active frames whose decode status was not 0: made inactive */
#define NTK_CLIPDEC_MASKED        2  /* active frames made inactive because the clip's STARTING frame failed */
#define NTK_CLIPDEC_FIRST_FAILED  3  /* index among the clip's active frames (0 = first tracked frame) of the first failure; -1 = none */
#define NTK_CLIPDEC_FIRST_STATUS  4  /* that frame's NTK_JPEG_STATUS_*; 0 = none */
#define NTK_CLIPDEC_START_STATUS  5  /* status of the clip's starting frame */
#define NTK_CLIPDEC_HEAD          6
int ntk_track_decode_mask(const int* status, int n_status, const int* cell_index, const int* start_index, const int* clip_of,
                          int T, int B, int n_clips, unsigned char* dead, unsigned char* active, long long* table, void* stream);

/* out[b,:] = mask[b] ? a[b,:] : b[b,:] for fp32 [B,n] rows, mask uint8 [B] on the device (out may alias a or b): keeps the
 * recurrent state of a tracker that sat a frame out. */
int ntk_select_rows(const unsigned char* mask, const float* a, const float* b, float* out, int B, int n, void* stream);

/* Masked row copy of up to NTK_STATE_KEEP_MAX_TENSORS fp32 tensors in ONE launch: for every b < B with (mask[b] != 0) ==
 * (keep_where != 0) and every i < ntensors, row b of src[i] (row_floats[i] floats at src[i] + b * row_floats[i]) is copied to row
 * b of dst[i]; no other row is read or written (a workgroup of an unselected row exits on the mask alone).  The online DNC
 * tracker keeps the recurrent state of a tracker that sits a frame out with it: rows with mask 0 are saved before the in-place
 * forward pass and put back after it, and an active tracker's state is never copied.
 * mask uint8 [B] and the pointer tables src / dst [ntensors] lie in DEVICE memory (upload the tables once); row_floats
 * [ntensors] is a HOST array, read before the launch and passed to the kernel by value.  src[i] and dst[i] must not overlap.
 * Rows whose size is a multiple of 4 floats on 16-byte aligned bases move in 16-byte accesses, any other row one float at a
 * time; a row size of 0 is allowed (nothing moves).  Plain vector stores only.
 * Errors, before any launch: NTK_ERR_BAD_PTR for a null mask / table / row_floats; NTK_ERR_BAD_SHAPE for B < 1 or > 65535,
 * ntensors < 1 or > NTK_STATE_KEEP_MAX_TENSORS, a negative row size, or 2^31 chunks of 1024 floats per row set. */
#define NTK_STATE_KEEP_MAX_TENSORS 16
int ntk_dnc_state_keep(const unsigned char* mask, int keep_where, int B, int ntensors, const float* const* src, float* const* dst,
                       const long long* row_floats, void* stream);

/* tf.image.resize_images(img, [out_h, out_w]) (bilinear, TF-1 defaults) -- direct_offset_output.py:193 */
int ntk_resize_bilinear(const float* image, int H, int W, int C, float* out, int out_h, int out_w, void* stream);

/* output gather + tanh + l2 loss (:581-606) and its gradient:
 * pred [B,T-1,O] (nullable), loss [1], dlogits [B,S,O] (nullable). */
int ntk_offset_loss(const float* logits, const float* offsets, float* pred, float* loss,
                    float* dlogits, int B, int T, int NF, int O, void* stream);

/* the same in two calls (ntk_offset_loss_fwd/bwd) */
int ntk_offset_loss_fwd(const float* logits, const float* offsets, float* pred, float* loss, int B, int T, int NF, int O,
                        void* stream);
int ntk_offset_loss_bwd(const float* logits, const float* offsets, float* dlogits, int B, int T, int NF, int O, void* stream);

/* Sequential presentation + heat-map head of main.py's earlier trackers (ntm_sevenbyseven,
 * main.py:1646-1969; the same serialisation in :979-1291).  Every position of the feature map is a feature
 * (F = Hf * Wf), rows are [feat(C), feature delimiter, frame delimiter, target, 0 pad]:
 *   frame 0: F rows [feat_i, 0, 0, gt0_i];  frame t >= 1: one frame-delimiter row, then per feature the rows
 *   [feat_i, 0, 0, 0] and [0.., 1, 0, 0]  ->  S = F + (T - 1)(2 F + 1) steps (main.py:1701-1775).
 * fmap [B*T, F, C] (C a multiple of 4), gts0 [B, F] (nullable), X [B, S, ldx] (ldx >= C + 3, multiple of 4).
 * Loss (main.py:1880-1922): the cell has output_dim 1; the logits at the FEATURE-DELIMITER steps of frames 1..T-1 form
 * an F-way score vector per frame; loss = sum softmax_cross_entropy_with_logits(scores, gt[b, t]) / (T - 1).
 * logits [B, S] (= [B,S,1]), gt [B, T-1, F] soft labels; probs [B, T-1, F] (nullable), loss [1], dlogits [B, S] (nullable). */
int ntk_serialize_sequential(const float* fmap, const float* gts0, float* X, int B, int T, int F, int C, int ldx, void* stream);
int ntk_heatmap_ce_loss(const float* logits, const float* gt, float* probs, float* loss, float* dlogits,
                        int B, int T, int F, void* stream);

/* Two-step presentation + (F+1)-way head of main.py's ntm_two_step (:862-977; ntm_tracker_new.py:112-195 with
 * two_step=True): a whole frame is ONE step, rows [switch, feat(D), target(F)]: step 0 = [0, feat_0, target], frame
 * t >= 1 = the presentation step [0, feat_t, 0] then the query step [1, 0, 0]  ->  S = 2T - 1 steps.
 * feat [B, T, D] (the flattened, optionally compressed feature map), target [B, F] (nullable), X [B, S, ldx], ldx >= 1 + D + F.
 * Loss (:903-951): labels are the background row [0..0, 1] at step 0 and at every presentation step and [gt_t, 0] at the
 * query step of frame t; they pass through a softmax before the cross entropy (as coded);
 * loss = sum_rows CE(logits_row, softmax(label_row)) / ((2T - 1) B).  logits [B, S, F+1], gt [B, T, F] (row 0 unused),
 * probs [B, S, F+1] (nullable), loss [1], dlogits [B, S, F+1] (nullable). */
int ntk_serialize_two_step(const float* feat, const float* target, float* X, int B, int T, int D, int F, int ldx, void* stream);
int ntk_two_step_ce_loss(const float* logits, const float* gt, float* probs, float* loss, float* dlogits,
                         int B, int T, int F, void* stream);

/* copy-task head (main.py:1603-1610, BASELINE configs[0]): loss = tf.losses.log_loss(labels,
 * sigmoid(logits)) (mean over all n elements, epsilon 1e-7) and d loss / d logits (nullable). */
int ntk_log_loss(const float* logits, const float* labels, float* loss, float* dlogits, int n, void* stream);

/* Repeat-copy task of the vendored DNC (dnc/repeat_copy.py, dnc/train.py).
 *
 * ntk_repeat_copy_pack lays out one batch in ONE launch (repeat_copy.py:252-377).  bits [B, max_length, num_bits] fp32 in
 * {0, 1}; lengths [B], repeats [B] int32 ON THE DEVICE; S the padded step count.  Outputs, every element written:
 *   X [B, S, ldx]               observations, batch-major, in the sequence kernels' input layout (ldx >= num_bits + 2, a multiple
 *                               of 4; the padding columns num_bits + 2 .. ldx - 1 are written as zero)
 *   target [B, S, num_bits + 1] and mask [B, S].
 * A sequence of pattern length L and r repeats: step 0 carries the start flag (channel num_bits), steps 1..L the pattern, step
 * L + 1 carries r / norm_max (channel num_bits + 1); target rows L + 2 .. L + 1 + L r hold the pattern tiled r times, row
 * L + 2 + L r the end marker (channel num_bits); the mask is 1 on rows L + 2 .. L + 2 + L r; all else is zero, and so is
 * everything from the sequence's own length L (r + 1) + 3 to S.
 * Range contract: lengths lie in [min_length, max_length] and repeats in [min_repeats, max_repeats] (min_length >= 1,
 * min_repeats >= 0); the kernel CLAMPS values outside, it does not trust them, so a bad table cannot index past bits.
 * The launcher cannot see the device tables: it refuses S < min_length (min_repeats + 1) + 3; rows at or past S are never
 * written (a sequence longer than S is cut). */
int ntk_repeat_copy_pack(const float* bits, const int* lengths, const int* repeats, float* X, float* target, float* mask,
                         int B, int S, int num_bits, int ldx, int min_length, int max_length, int min_repeats, int max_repeats,
                         float norm_max, void* stream);

/* masked_sigmoid_cross_entropy (repeat_copy.py:29-66) with its gradient and the copy score, in one pass.  logits, target
 * [B, S, O] batch-major (what the sequence kernels write), mask [B, S].  xent = max(x, 0) - x z + log1p(exp(-|x|)), summed
 * over channels, then over steps times their mask; with time_average divided by (sum of the mask + FLT_EPSILON); that is
 * loss_batch [B]; loss [1] = sum(loss_batch) / B, divided by ln 2 with log_prob_in_bits.  dlogits [B, S, O] (nullable:
 * loss only) = (sigmoid(x) - z) times the same factors.  score [B, 2] int32 (nullable): the scored bits of the sequence and
 * those where (logit > 0) != (target > 0.5), i.e. where train.py:104-105's rounded output differs from the target.
 * Departure from the reference: a step whose mask is 0 is SELECTED out, not multiplied out -- it adds exactly 0 and its
 * dlogits are +0.0 whatever its logits hold, NaN included.  One workgroup per sequence, then a fixed-order batch sum:
 * the same bits from run to run. */
int ntk_masked_sigmoid_xent(const float* logits, const float* target, const float* mask, float* loss, float* loss_batch,
                            float* dlogits, int* score, int B, int S, int O, int time_average, int log_prob_in_bits,
                            void* stream);

/* ------------------------------------------------------------------------
 * optimiser (direct_offset_output.py:620-626): tf.clip_by_global_norm +
 * tf.train.RMSPropOptimizer on one flat buffer
 * --------------------------------------------------------------------- */
size_t ntk_global_norm_workspace_bytes(size_t n);
int ntk_global_norm(const float* grads, size_t n, float* workspace, float* gnorm, void* stream);
int ntk_rmsprop_clip_step(float* params, const float* grads, float* ms, float* mom, size_t n,
                          float lr, float decay, float momentum, float eps, float clip_norm,
                          const float* gnorm, void* stream);
/* The same update behind a finiteness check of *gnorm (required): when the global norm is NaN or Inf -- a poisoned
 * gradient (ntk_dnc_cluster_guard), on ANY data-parallel rank once the SUM all-reduce has run -- parameters and slots
 * stay untouched, loss[0] (nullable) becomes NaN and *skipped (nullable, device counter) is incremented; otherwise it is
 * ntk_rmsprop_clip_step bit for bit.  What the trackers' training steps run (the reference has no failure path here:
 * tf.clip_by_global_norm would write NaN into every variable). */
int ntk_rmsprop_clip_step_checked(float* params, const float* grads, float* ms, float* mom, size_t n,
                                  float lr, float decay, float momentum, float eps, float clip_norm,
                                  const float* gnorm, float* loss, unsigned* skipped, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NTMTRACK_H_ */
