// A6-A8, A10: the per-token decoder path.  With one new token per stream every projection is a
// skinny GEMM  y[B<=16, N] = f(x[B, K]) . W[N, K]^T  whose cost is streaming W once from HBM
// (1.6 GB per step for large-v3 in bf16), so these kernels are HBM-bound by construction:
//
//  * skinny_mfma_kernel (launch_gemv): the <=16 activation rows are exactly one MFMA operand tile, so one 16-row weight
//    tile per workgroup is streamed ONCE (fragment-major layout prepared at load time: every wavefront request is 1 KiB
//    contiguous) and contracted by v_mfma_f32_16x16x32_bf16 (f32 mode: 16x16x4_f32) for all streams at once; K is split
//    over the wavefronts and summed in a fixed order through LDS (deterministic, no atomics).  Fused: folded
//    pre-LayerNorm, bias, GELU, residual, KV-cache scatter, fp32 logits.
//  * dec_self_attn / dec_cross_attn: single-query attention over the KV cache, one wavefront per
//    (stream, head) [x4 for the 500..1500-key cross attention], lanes = 4 key groups x 16 dim
//    quads, online softmax in registers, 16-lane shuffle dot products.  Cross attention also emits
//    the softmax rows of the alignment heads for the DTW (A11).
//  * sampler: Whisper's logits processors + first-index argmax on the fp32 logits, one workgroup
//    per stream (HF:generation/logits_process.py:1816-2047, HF:generation/utils.py:2925).
#include "tw_common.h"

namespace {

// Row stride (floats) of the projection kernel's partial tiles in LDS.  A partial tile is written [weight row][stream] by the MFMA
// lanes and read [stream][weight row] by the epilogue threads (16 consecutive rows of one stream per 16 threads, for the stores):
// with 16 floats per row a 32-lane group of a ds_read_b32 hit 4 banks, 8 addresses each (8-way conflict on every read of the
// reduction); 17 spreads it over all 32 banks, the writers stay at <= 2 addresses per bank (free for stores).
constexpr int kRedStride = 17;
constexpr int kRedTile = 16 * kRedStride;   // floats per partial tile in LDS

__device__ __forceinline__ float wave_sum(float v) { return tw_wave_sum(v); }
// erf-GELU (activation_function = "gelu").  Strict-f32 contexts use the library erff; bf16 contexts, whose outputs are
// rounded to 8 mantissa bits anyway, use the Abramowitz-Stegun 7.1.26 rational form (|error| < 2e-7 on erf + one fast
// exp: ~12 instead of ~45 VALU instructions per element, which is a third of the fc1 GEMM's epilogue-bound run time).
template <typename T>
__device__ __forceinline__ float gelu_exact(float x) {
  const float z = x * 0.70710678118654752440f;
  if (sizeof(T) == 4) return 0.5f * x * (1.0f + erff(z));
  const float az = fabsf(z);
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, az, 1.0f));
  float p = fmaf(t, 1.061405429f, -1.453152027f);
  p = fmaf(t, p, 1.421413741f);
  p = fmaf(t, p, -0.284496736f);
  p = fmaf(t, p, 0.254829592f);
  const float e = fmaf(-(p * t), __expf(-az * az), 1.0f);   // (spelled out: one rounding sequence in every instantiation)
  return 0.5f * x * (1.0f + copysignf(e, z));
}

// NB for every helper below that takes bf16 pairs out of a 16-byte vector: hipcc (ROCm 7.2) folds `bit_cast<bf16x2>(v[i])`
// inside an unrolled loop to element 0 for every i (seen in the ISA: identical instructions), so pairs are always taken
// with named __builtin_shufflevector selections of the whole bf16x8 vector.

template <typename T> __device__ __forceinline__ u32x4_t pack16(const float* in);
template <> __device__ __forceinline__ u32x4_t pack16<float>(const float* in) {
  return __builtin_bit_cast(u32x4_t, f32x4_t{in[0], in[1], in[2], in[3]});
}
template <> __device__ __forceinline__ u32x4_t pack16<bf16_t>(const float* in) {
  bf16x8_t f;
#pragma unroll
  for (int i = 0; i < 8; ++i) f[i] = (bf16_t)in[i];
  return __builtin_bit_cast(u32x4_t, f);
}
template <> __device__ __forceinline__ u32x4_t pack16<f16_t>(const float* in) {   // probabilities: in range, no saturation needed
  f16x8_t f;
#pragma unroll
  for (int i = 0; i < 8; ++i) f[i] = (f16_t)in[i];
  return __builtin_bit_cast(u32x4_t, f);
}

// Folded pre-LayerNorm.  For y = LN(x) . W^T + bias with LN(x) = (x - mean) * rstd * g + beta:
//     y[n] = rstd * ( x . W'[n]  -  mean * gW[n] )  +  cb[n],
//     W'[n,k] = g[k] W[n,k],   gW[n] = sum_k g[k] W[n,k],   cb[n] = sum_k beta[k] W[n,k] + bias[n]
// W', gW and cb are prepared once at weight-finalisation time (fold_ln_kernel below), so the projection streams W'
// against the RAW residual stream exactly like a projection without LayerNorm, and only the two per-stream scalars
// (mean, rstd) have to be known when the epilogue runs - they are computed off the critical path while the weight
// loads are in flight.  No normalised copy of x is ever materialised.


// ---------------------------------------------------------------------------------------------
// Skinny MFMA GEMM for 1..16 concurrent streams:  y[b, n0..n0+15] for one 16-row weight tile per
// workgroup, K split over the NW wavefronts.  With 16 streams the activation block is exactly one
// MFMA tile (v_mfma_f32_16x16x32_bf16: A = 16 weight rows x 32 k, B = 16 streams x 32 k), so each
// 1-KiB weight fragment costs ONE matrix instruction and ONE 16-B activation fragment instead of
// 16 LDS reads + 64 dot2 + a wave reduction per stream in the VALU formulation; the contraction
// over k happens inside the MFMA and only NW partial 16x16 tiles are summed through LDS.
// All weight and activation fragments of a wavefront are requested up front (activations straight
// from L2 - the residual stream is 40 KB); with the folded LayerNorm (above) the per-stream
// (mean, rstd) are reduced by the wavefronts while those loads are in flight and meet the
// accumulators at the one barrier the partial-tile reduction needs anyway.
// Deterministic: fixed summation order, no atomics.
// ---------------------------------------------------------------------------------------------

template <typename T>
__device__ __forceinline__ f32x4_t sk_mfma(const u32x4_t& w, const u32x4_t& x, f32x4_t acc);
template <>
__device__ __forceinline__ f32x4_t sk_mfma<bf16_t>(const u32x4_t& w, const u32x4_t& x, f32x4_t acc) {
  return tw_mfma32<bf16_t>(w, x, acc);
}
template <>
__device__ __forceinline__ f32x4_t sk_mfma<f16_t>(const u32x4_t& w, const u32x4_t& x, f32x4_t acc) {
  return tw_mfma32<f16_t>(w, x, acc);
}
template <>
__device__ __forceinline__ f32x4_t sk_mfma<float>(const u32x4_t& w, const u32x4_t& x, f32x4_t acc) {
  const f32x4_t a = __builtin_bit_cast(f32x4_t, w), b = __builtin_bit_cast(f32x4_t, x);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], b[1], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], b[2], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], b[3], acc, 0, 0, 0);
  return acc;
}

// Epilogue flavours (compile-time: a runtime-uniform branch around a load makes hipcc wait for EVERY outstanding load at
// the join, which serialises the whole prologue - see the ordering note below).
enum : int { SK_STORE = 0, SK_RES = 1, SK_GELU = 2, SK_KV = 3, SK_F32 = 4,
             SK_KV_RAG = 5 };   // SK_KV of a ragged step (tw_common.h: tw_row_pos): the K / V^T scatter goes to the stream's ROW position

template <typename T>
__device__ __forceinline__ u32x4_t sk_load_w(const T* p) {  // weights are read exactly once per step: non-temporal
  return __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(p));
}

typedef int v8i_t __attribute__((ext_vector_type(8)));
typedef unsigned short u16x2_t __attribute__((ext_vector_type(2)));
typedef short s16x2_t __attribute__((ext_vector_type(2)));

// value of lane ^ 16 / lane ^ 32 (bit pattern; after the swap {a, b} = {own, partner} whichever half the lane is in)
__device__ __forceinline__ unsigned sk_from_xor16(unsigned v) {
  float a = __builtin_bit_cast(float, v), b = a;
  tw_swap16(a, b);
  return __builtin_bit_cast(unsigned, a) ^ __builtin_bit_cast(unsigned, b) ^ v;
}
__device__ __forceinline__ unsigned sk_from_xor32(unsigned v) {
  float a = __builtin_bit_cast(float, v), b = a;
  tw_swap32(a, b);
  return __builtin_bit_cast(unsigned, a) ^ __builtin_bit_cast(unsigned, b) ^ v;
}

// MXFP8 quantisation of one 128-k operand step held by a wavefront: lane (kq = lane>>4, idx = lane&15) holds 32 bf16
// values, 4 fragments of 8; byte 8m + e of its 32-B operand <- fragment m, element e.
// Block structure = what v_mfma_scale_f32_16x16x128_f8f6f4 scales together (measured with tools/dbg/mx_probe2.hip: the
// instruction's true k of operand byte q in lane group kq is (q/16)*64 + kq*16 + q%16, and the scale of the 32-k block t
// is byte 0 of the scale register in lane t*16 + idx): block (u, h) = 16-byte half h of the two lane groups kq = 2u, 2u+1,
// its scale lives in lane group h*2 + u.  Hence: per-half maxima, one exchange with lane^16, convert, and one exchange
// with lane^32 to put each scale byte where the hardware reads it.
// Scale byte sb = max(E - 7, 1), E = biased exponent of the block's largest magnitude; elements = RNE_e4m3(v / 2^(sb-127))
// (|.| < 256, never overflows).  One exponent more conservative than the OCP MX convention (E - 8 with saturation)
// because the gfx950 converts return NaN instead of saturating above 464.  Must be called by all 64 lanes.
__device__ __forceinline__ v8i_t sk_quant_mx8(const u32x4_t (&xv)[4], int& scale_operand) {
  u16x2_t mx[2] = {{0, 0}, {0, 0}};
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int q = 0; q < 4; ++q) mx[m >> 1] = __builtin_elementwise_max(mx[m >> 1], __builtin_bit_cast(u16x2_t, xv[m][q] & 0x7fff7fffu));
  const unsigned own = max((unsigned)mx[0][0], (unsigned)mx[0][1]) | (max((unsigned)mx[1][0], (unsigned)mx[1][1]) << 16);
  const unsigned oth = sk_from_xor16(own);
  const int sb0 = max((int)(max(own & 0xffffu, oth & 0xffffu) >> 7) - 7, 1);
  const int sb1 = max((int)(max(own >> 16, oth >> 16) >> 7) - 7, 1);
  const float X0 = __builtin_bit_cast(float, (unsigned)sb0 << 23), X1 = __builtin_bit_cast(float, (unsigned)sb1 << 23);  // 2^(sb-127)
  v8i_t out;
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    // named pairs of the whole vector, not bit_cast<bf16x2>(xv[m][q]): hipcc (ROCm 7.2) folds the latter to element 0 (NB at the top)
    const bf16x8_t a = __builtin_bit_cast(bf16x8_t, xv[m]);
    const float X = m < 2 ? X0 : X1;
    s16x2_t lo = {0, 0}, hi = {0, 0};
    lo = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(lo, __builtin_shufflevector(a, a, 0, 1), X, false);
    lo = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(lo, __builtin_shufflevector(a, a, 2, 3), X, true);
    hi = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(hi, __builtin_shufflevector(a, a, 4, 5), X, false);
    hi = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(hi, __builtin_shufflevector(a, a, 6, 7), X, true);
    out[2 * m] = __builtin_bit_cast(int, lo);
    out[2 * m + 1] = __builtin_bit_cast(int, hi);
  }
  // scale of block t belongs in lane group t: t = 0 <- (u 0, h 0), 1 <- (u 1, h 0), 2 <- (u 0, h 1), 3 <- (u 1, h 1); this
  // lane knows (u = kq/2, h = 0 and 1), the lane group kq^2 knows the other u
  const unsigned mine = (unsigned)sb0 | ((unsigned)sb1 << 8);
  const unsigned far = sk_from_xor32(mine);
  const int kq = (threadIdx.x >> 4) & 3;
  const unsigned pick = (kq == 0) ? (mine & 0xffu) : (kq == 3) ? (mine >> 8) : (kq == 1) ? (far & 0xffu) : (far >> 8);
  scale_operand = (int)(pick & 0xffu);
  return out;
}

// 16 e4m3 bytes -> two bf16 MFMA operands (bytes 0..7, 8..15), each value multiplied by X = 2^(scale byte - 127): exact in bf16
// (3 mantissa bits times a power of two).  v_cvt_scalef32_pk_bf16_fp8 converts one byte pair per instruction.
__device__ __forceinline__ void sk_widen8(const u32x4_t& raw, float X, u32x4_t& lo, u32x4_t& hi) {
  lo[0] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)raw[0], X, false));
  lo[1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)raw[0], X, true));
  lo[2] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)raw[1], X, false));
  lo[3] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)raw[1], X, true));
  hi[0] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)raw[2], X, false));
  hi[1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)raw[2], X, true));
  hi[2] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)raw[3], X, false));
  hi[3] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)raw[3], X, true));
}

// (sum, sum of squares) of the 16 bytes of one activation fragment, accumulated per lane
template <typename T> __device__ __forceinline__ void sk_stats(const u32x4_t& v, float& s, float& ss);
template <> __device__ __forceinline__ void sk_stats<bf16_t>(const u32x4_t& v, float& s, float& ss) {
  const bf16x8_t a = __builtin_bit_cast(bf16x8_t, v);
  const bf16x2_t one = {(bf16_t)1.0f, (bf16_t)1.0f};
  // named pairs, not a loop over v[i]: see the NB at the top of this file
  const bf16x2_t p0 = __builtin_shufflevector(a, a, 0, 1), p1 = __builtin_shufflevector(a, a, 2, 3);
  const bf16x2_t p2 = __builtin_shufflevector(a, a, 4, 5), p3 = __builtin_shufflevector(a, a, 6, 7);
  s = __builtin_amdgcn_fdot2_f32_bf16(p0, one, s, false);
  ss = __builtin_amdgcn_fdot2_f32_bf16(p0, p0, ss, false);
  s = __builtin_amdgcn_fdot2_f32_bf16(p1, one, s, false);
  ss = __builtin_amdgcn_fdot2_f32_bf16(p1, p1, ss, false);
  s = __builtin_amdgcn_fdot2_f32_bf16(p2, one, s, false);
  ss = __builtin_amdgcn_fdot2_f32_bf16(p2, p2, ss, false);
  s = __builtin_amdgcn_fdot2_f32_bf16(p3, one, s, false);
  ss = __builtin_amdgcn_fdot2_f32_bf16(p3, p3, ss, false);
}
template <> __device__ __forceinline__ void sk_stats<f16_t>(const u32x4_t& v, float& s, float& ss) {
  const f16x8_t a = __builtin_bit_cast(f16x8_t, v);
  const f16x2_t one = {(f16_t)1.0f, (f16_t)1.0f};
  const f16x2_t p0 = __builtin_shufflevector(a, a, 0, 1), p1 = __builtin_shufflevector(a, a, 2, 3);
  const f16x2_t p2 = __builtin_shufflevector(a, a, 4, 5), p3 = __builtin_shufflevector(a, a, 6, 7);
  s = tw_dot2<f16_t>(p0, one, s);
  ss = tw_dot2<f16_t>(p0, p0, ss);
  s = tw_dot2<f16_t>(p1, one, s);
  ss = tw_dot2<f16_t>(p1, p1, ss);
  s = tw_dot2<f16_t>(p2, one, s);
  ss = tw_dot2<f16_t>(p2, p2, ss);
  s = tw_dot2<f16_t>(p3, one, s);
  ss = tw_dot2<f16_t>(p3, p3, ss);
}
template <> __device__ __forceinline__ void sk_stats<float>(const u32x4_t& v, float& s, float& ss) {
  const f32x4_t a = __builtin_bit_cast(f32x4_t, v);
#pragma unroll
  for (int i = 0; i < 4; ++i) { s += a[i]; ss = fmaf(a[i], a[i], ss); }
}

// SK_MAXS = weight/activation fragments a wavefront keeps in flight (5 covers K = 1280 in bf16 with 8 wavefronts)
// LN      = folded pre-LayerNorm (ln_gw / ln_cb given), EPI = epilogue flavour, MULTI = several 16-row tiles per
//           workgroup (tall matrices: the tied logits projection), next tile prefetched behind the current reduction.
// Activations (x, the residual operand, and the outputs of SK_RES / SK_GELU) live in the fragment-major "xt" layout of
// tw_common.h (tw_xt_index): like the weights, every wavefront request is then 1 KiB contiguous.  The LayerNorm
// statistics come from the activation fragments the wavefront holds anyway (per-lane sum / sum of squares with
// v_dot2, folded over the 4 k-groups by two lane swaps, over the wavefronts in the epilogue through LDS): no extra
// loads and ~60 instead of ~500 VALU instructions on the critical path (at 4 cycles per wave64 VALU op that was 1 us).
// Ordering rules this kernel follows (measured with s_memrealtime stamps inside the kernel, profiles/r05_projection_probe.txt):
//  * all kernel arguments are pinned in SGPRs by one asm statement: one batch of scalar loads, one wait;
//  * vmcnt retires loads IN ORDER, so operands are requested in the order they are consumed: the (L2-resident)
//    activation fragments, then the HBM weight fragments; sched_barriers keep hipcc from reordering the groups or
//    hoisting arithmetic between them;
//  * no load sits inside a conditional block (clamped addresses, zero-selected operands instead): at the join of a
//    runtime-uniform branch around a load hipcc waits for EVERY outstanding load.
//
// W8 = MXFP8 weights (TW_BF16_MXFP8 contexts): the weight operand is OCP e4m3 with one power-of-two scale per 32 values
// (quant_mx8_kernel below), the bf16 activation fragments are quantised the same way in registers (sk_quant_mx8: a scale
// block is the same 16-byte half of two neighbouring lane groups, so one lane exchange finds its maximum and a second one
// puts the scale byte where the instruction reads it), and the product runs on v_mfma_scale_f32_16x16x128_f8f6f4, which
// applies both block scales in hardware.  One step is then 128 k: 2 KiB of weights + 64 scale bytes per tile, half the
// bytes of the bf16 kernel.
// CG = groups of 16 streams (1, 2 or 4: up to 64 streams per launch).  Every weight fragment is used for all groups, so the
// weight stream - the dominant cost - is paid once per launch whatever the number of streams; activations, accumulators
// and the epilogue are per group (group g of a fragment-major activation buffer starts at element g*16*K).
// TR = weight rows per workgroup tile (16, or 8 / 4 for the narrow projections): with N = 1280 a 16-row tiling yields only 80
// workgroups on a 256-CU chip and every CU has to take in 41 KB (K = 1280) or 164 KB (K = 5120) at ~50 GB/s; TR = 8 (4)
// spreads the same bytes over 160 (320) CUs.  The MFMA still contracts a 16-row A operand whose rows >= TR are zero (lanes
// fr >= TR issue no request): matrix-core time is not what bounds these launches.  Weight layout for TR < 16:
// [tile][step][kq * TR + fr][E] (tile_weights_kernel), i.e. a wavefront request is TR * 64 contiguous bytes.
// A16 (with W8) = "W8A16": the MXFP8 weight fragments are widened to bf16 in registers (sk_widen8: value x block scale, exact)
// and contracted with the UNQUANTISED bf16 activations on v_mfma_f32_16x16x32_bf16 - the same bytes from HBM as W8, no
// activation quantisation (neither its error nor its ~0.3 us of lane exchanges on the critical path of a latency-bound launch).
// A weight lane needs the scales of ITS two 32-value blocks (16-byte half h of lane groups 2u, 2u+1, u = kq / 2); the scale array
// holds block t = 2h + u in lane group t (where the scaled MFMA reads it), so the lane fetches groups u and 2 + u: two byte loads
// per step instead of one, no exchange.  Several groups of 16 streams (CG > 1) are available in this mode only.
//
// ONE reduction order for every number of rows (round 6).  A stream's result must not depend on who else is in the launch - the
// serving hub mixes sessions freely, and the draft-and-verify prefill (api.hip: verify_core) is only exact if a position computed in a
// 64-row launch has the bits the one-row step would have produced.  Every kernel flavour contracts a given k step with the same
// instruction and walks a wavefront's K slice in ascending order, so results can only differ through HOW K IS SPLIT over wavefronts.
// All projections use 8 slices [w S / 8, (w + 1) S / 8) summed in ascending order - except the long-K residual projection (fc2,
// K >= 4096), which takes 16 wavefronts when the launch has one group of streams (half the steps per wavefront on the critical
// path) and 8 with several groups (registers).  Its canonical order is therefore defined over SIXTEEN slices v = 0..15,
// P_v = sum over steps [v S / 16, (v + 1) S / 16), result = sum_{w = 0..7} (P_2w + P_2w+1): the 16-wavefront kernel adds its LDS tiles
// in pairs, the 8-wavefront kernel (SPLIT2) keeps two accumulators per group - the two halves of its slice - and adds them in
// registers before the tile goes to LDS.  Bit-identical by construction; tests/test_gpu_parity.py::test_rows_of_a_launch_do_not_matter.
template <typename T, int NW, int SK_MAXS, bool LN, int EPI, bool MULTI, bool W8, int CG, int TR, bool A16 = false, int MODE = 0, bool SPLIT2 = false>
__global__ __launch_bounds__(NW * 64, (CG > 1 ? ((NW >= 16 || (!MULTI && !W8 && MODE == 2)) ? 4 : 2) : (NW >= 16 ? 4 : (W8 ? (SK_MAXS <= 2 ? 4 : 2) : (SK_MAXS <= 5 ? 4 : 2)))))
void skinny_mfma_kernel(const void* x_arg, const void* w_arg, int k_arg, int b_arg, int n_arg, int rg_arg,
                        const unsigned char* wscale_arg, const void* bias_arg, const void* res_arg, const float* gw_arg, GemvArgs a) {
  // The first arguments repeat what the request addresses are formed from (operands, K, B, N, tiles per workgroup): gfx950
  // delivers the leading kernel-argument dwords in SGPRs with the wave (kernarg preload, build.py: -amdgpu-kernarg-preload-count),
  // so the activation and weight requests leave without waiting for a scalar load; everything else (epilogue operands, outputs)
  // stays in the GemvArgs block behind them - a struct is never preloaded - and arrives while those requests are in flight.
  static_assert(!W8 || ElemTraits<T>::kCode == 1, "MXFP8 weights go with bf16 activations");
  static_assert(TR == 16 || (!MULTI && EPI != SK_KV && EPI != SK_KV_RAG && EPI != SK_F32), "narrow tiles: plain / residual / GELU projections only");
  static_assert(!W8 || TR == 16 || TR == 8, "MXFP8 weights: 16- or 8-row tiles");
  static_assert(!A16 || W8, "A16 is a flavour of the MXFP8-weight kernel");
  static_assert(!W8 || CG == 1 || A16, "several stream groups with MXFP8 weights: W8A16 only");
  static_assert(!SPLIT2 || (NW == 8 && !LN && !MULTI && CG > 1), "SPLIT2: the 8-wavefront flavour of the long-K residual projection");
  constexpr int E = ElemTraits<T>::kPer16B;
  constexpr int XPS = W8 ? 4 : 1;  // 32-wide activation fragments per MFMA step
  constexpr int WPS = W8 ? 2 : 1;  // 16-B weight requests per MFMA step
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ float pstat[NW][CG * 16][2];  // per wavefront and stream: (sum, sum of squares) over the wavefront's K slice
  const T* x = reinterpret_cast<const T*>(x_arg);
  const T* W = reinterpret_cast<const T*>(w_arg);
  const unsigned char* wscale = wscale_arg;
  const T* bias = reinterpret_cast<const T*>(bias_arg);
  const T* res = reinterpret_cast<const T*>(res_arg);
  const float* gw_p = gw_arg;
  const float* cb_p = a.ln_cb;
  const int K = k_arg, N = n_arg, B = b_arg, ldy = a.ldy, RG = rg_arg, d_model = a.d_model;
  const long long cache_bstride = a.cache_bstride, cache_hstride = a.cache_hstride;
  T* y = reinterpret_cast<T*>(a.y);
  float* y_f32 = a.y_f32;
  T* kcache = reinterpret_cast<T*>(a.kcache);
  T* vcache = reinterpret_cast<T*>(a.vcache);
  const DecState* stt = a.stt;
  float* u_p = a.u;              // "cross query ahead" (tw_common.h): float32 [B][d_model] pre-activation, null = off
  float* stats_p = a.stats;
  const int nsplit = a.nsplit;   // SK_RES: rows >= nsplit accumulate into u (the launcher sets N when there is no such half)
  const int rows_streams = a.rows_streams;   // SK_KV: rows mode of the cache scatter (tw_row_of)
  // (1) what the activation / weight requests need: delivered with the wave (leading arguments), nothing to wait for
  asm volatile("" ::"s"(x), "s"(W), "s"(K), "s"(N), "s"(B), "s"(RG), "s"(wscale));
  int cur_pos = 0;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, kq = lane >> 4;
  const int S = K / (4 * E * XPS);  // MFMA steps per row (32 k each; 128 k with MXFP8 weights)
  const int s_lo = (int)((long long)wave * S / NW), s_hi = (int)((long long)(wave + 1) * S / NW);
  float* red = reinterpret_cast<float*>(smem);  // [NW][CG][256]
  const int n_tiles = (N + TR - 1) / TR;
  const int tile0 = blockIdx.x * RG;
  const int ej = (tid >> 4) & 15, ei = tid & 15;  // epilogue role of threads 0..255: stream ej, tile row ei (rows >= TR idle)

  // MODE (several groups of streams only; picked by the launcher): 0 = rounds of SK_MAXS fragments, 2 = operand rings over the
  // wavefront's whole K slice (SK_MAXS = the slice's step count; 16-bit or f32 weights only).  (1 - rounds with the next round's weights
  // requested a round ahead - was measured in round 5 and dropped: fc2 at 64 streams 12.1 -> 12.6 us, profiles/r05_projection_probe.txt)
  // The rings: weights 5 steps deep, activations 3 steps x CG groups, refilled as soon as a step has been contracted - straight-line
  // code, the compiler's vmcnt counts are exact.  The point is registers: the one-round scheme holds CG x 5 activation fragments at
  // once (80 registers at 64 streams, 134-158 in total: ONE 512-thread workgroup per CU, so the 320-workgroup launches ran as two
  // rounds on the decode loop's 160 CUs); the rings need 48 and two workgroups fit.
  constexpr bool RING = CG > 1 && !W8 && MODE == 2;
  // RING with MULTI = DUAL (round 5's "two tiles per workgroup", back in round 6): the workgroup contracts TWO weight tiles (tile0,
  // tile0 + 1; the launcher sets RG = 2) against ONE sweep of the activation rings - half the activation (L2) traffic of two workgroups,
  // 160 instead of 320 workgroups for the 5120-row launches (QKV, fc1).  Round 5 removed it because stream 63 of 64 decoded other ids
  // than stream 0 on the same audio; the cause was not in this structure but in the LayerNorm variance, which hipcc fused differently
  // for the two stream groups an epilogue thread finishes (profiles/r06_mode3_root_cause.txt) - spelled out now (tw_ln_scalars).
  constexpr bool DUAL = RING && MULTI;
  constexpr int DW = RING ? (SK_MAXS < 5 ? SK_MAXS : 5) : 1;   // ring depths (steps)
  constexpr int DX = RING ? (SK_MAXS < 3 ? SK_MAXS : 3) : 1;
  u32x4_t rw[DW], rx[DX][CG];
  u32x4_t rw2[DUAL ? DW : 1];
  // several groups: the two 256-thread halves of the workgroup take alternate groups in the epilogue
  constexpr bool EALL = CG > 1 && NW >= 8;
  constexpr int GPT = EALL ? CG / 2 : CG;     // groups per epilogue thread
  u32x4_t wq[SK_MAXS * WPS], xq[CG][SK_MAXS * XPS];
  int wsc[SK_MAXS];  // MXFP8: scale byte of the weight block this lane feeds to the scaled MFMA (A16: of its own first block)
  int wsc2[A16 ? SK_MAXS : 1];  // A16: scale byte of its own second block
  const int eh = EALL ? ((tid >> 8) & 1) : 0;   // which half of the workgroup this epilogue thread belongs to
  float e_c = 0.f, e_gw = 0.f, e_res[GPT];
#pragma unroll
  for (int g = 0; g < GPT; ++g) e_res[g] = 0.f;
  // --- request helpers: all unconditional, addresses clamped into the matrix ---
  auto load_epi = [&](int tile, float& c, float& gwv, float (&r)[GPT]) {
    const int n = min(tile * TR + min(ei, TR - 1), N - 1);
    const bool second = EPI == SK_RES && n >= nsplit;   // row of the composed half: its "residual" is u, it has no bias
    if (LN) {
      gwv = gw_p[n];
      c = cb_p[n];
    } else {
      const float v = (float)(bias ? bias : W)[(bias && !second) ? n : 0];
      c = (bias && !second) ? v : 0.f;
    }
    if (EPI == SK_RES) {
      // both operands are requested unconditionally (clamped addresses) and selected afterwards: no load inside a branch
      const float* up = u_p ? u_p : reinterpret_cast<const float*>(W);
      const int usz = u_p ? N - nsplit : 0;
      const int nu = (u_p && second) ? n - nsplit : 0;
#pragma unroll
      for (int gi = 0; gi < GPT; ++gi) {
        const int g = EALL ? gi * 2 + eh : gi;
        const float rb = (float)res[(long long)g * 16 * nsplit + tw_xt_index<T>(ej, second ? 0 : n)];
        const float ru = up[(long long)min(g * 16 + ej, B - 1) * usz + nu];
        r[gi] = second ? ru : rb;
      }
    }
  };
  const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<T*>(W), 0, TR == 16 ? 0 : (int)((long long)n_tiles * S * 4 * TR * 16 * (W8 ? 2 : 1)), 0x00020000);
  const __amdgpu_buffer_rsrc_t wsr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned char*>(wscale), 0, (W8 && TR != 16) ? (int)((long long)n_tiles * S * 4 * TR) : 0, 0x00020000);
  auto load_w_into = [&](auto& wq, auto& wsc, auto& wsc2, int tile, int s0) {  // fragment-major weights: 1 KiB contiguous per wavefront request
    const int tl = min(tile, n_tiles - 1);
    if (W8 && TR == 16) {
      const unsigned char* wt = reinterpret_cast<const unsigned char*>(W) + ((long long)tl * S * 128 + lane) * 16;
      const unsigned char* ws = wscale + (long long)tl * S * 64 + lane;
#pragma unroll
      for (int i = 0; i < SK_MAXS; ++i) {
        const long long st = min(s0 + i, S - 1);
        wq[2 * i] = sk_load_w<unsigned char>(wt + st * 2048);
        wq[2 * i + 1] = sk_load_w<unsigned char>(wt + st * 2048 + 1024);
        if constexpr (A16) {
          wsc[i] = wscale[(long long)tl * S * 64 + st * 64 + (kq >> 1) * 16 + fr];
          wsc2[i] = wscale[(long long)tl * S * 64 + st * 64 + (2 + (kq >> 1)) * 16 + fr];
        } else {
          wsc[i] = ws[st * 64];
        }
      }
    } else if (W8) {
      // 8-row MXFP8 tiles (quant_mx8_kernel with tr = 8): per (tile, 128-k step) [half][kq*8 + row][16 B] + 32 scale bytes;
      // the lanes of rows >= 8 are out of range of the descriptors (no request, zero data, zero scale)
      const unsigned lane_off = (fr < TR) ? (unsigned)((kq * TR + fr) * 16) : 0x80000000u;
      const unsigned sc_off = (fr < TR) ? (unsigned)(kq * TR + fr) : 0x80000000u;
      const unsigned tile_off = (unsigned)tl * (unsigned)(S * 8 * TR * 16);   // S steps x 2 halves x 4*TR lanes x 16 B
#pragma unroll
      for (int i = 0; i < SK_MAXS; ++i) {
        const unsigned st = (unsigned)min(s0 + i, S - 1);
        const unsigned o = lane_off + tile_off + st * (unsigned)(8 * TR * 16);
        wq[2 * i] = __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(wr, o, 0, 2 /* nt */));
        wq[2 * i + 1] = __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(wr, o + (unsigned)(4 * TR * 16), 0, 2));
        if constexpr (A16) {
          const unsigned sc_a = (fr < TR) ? (unsigned)((kq >> 1) * TR + fr) : 0x80000000u;
          const unsigned sc_b = (fr < TR) ? (unsigned)((2 + (kq >> 1)) * TR + fr) : 0x80000000u;
          wsc[i] = (int)__builtin_amdgcn_raw_buffer_load_b8(wsr, sc_a + ((unsigned)tl * S + st) * (unsigned)(4 * TR), 0, 0);
          wsc2[i] = (int)__builtin_amdgcn_raw_buffer_load_b8(wsr, sc_b + ((unsigned)tl * S + st) * (unsigned)(4 * TR), 0, 0);
        } else {
          wsc[i] = (int)__builtin_amdgcn_raw_buffer_load_b8(wsr, sc_off + ((unsigned)tl * S + st) * (unsigned)(4 * TR), 0, 0);
        }
      }
    } else if (TR == 16) {
      const T* wt = W + ((long long)tl * S * 64 + lane) * E;
#pragma unroll
      for (int i = 0; i < SK_MAXS; ++i) wq[i] = sk_load_w<T>(wt + (long long)min(s0 + i, S - 1) * (64 * E));
    } else {
      // narrow tile: only the lanes of weight rows fr < TR request (through a buffer descriptor: the others are out of range
      // and return zeros without a memory transaction)
      const unsigned lane_off = (fr < TR) ? (unsigned)((kq * TR + fr) * 16) : 0x80000000u;
      const unsigned tile_off = (unsigned)tl * (unsigned)(S * 4 * TR * 16);
#pragma unroll
      for (int i = 0; i < SK_MAXS; ++i)
        wq[i] = __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(
            wr, lane_off + tile_off + (unsigned)(min(s0 + i, S - 1) * (4 * TR * 16)), 0, 2 /* nt */));
    }
  };
  auto load_w = [&](int tile, int s0) { load_w_into(wq, wsc, wsc2, tile, s0); };
  // fragment-major activations: lane (stream fr, k-group kq) of each 32-k step.  Requested through a buffer descriptor so
  // that the lanes of streams >= B are out of range: they return zeros WITHOUT a memory request, i.e. a launch for one
  // stream moves 1/16 of the activation bytes of a launch for 16 (the block is re-read by every workgroup: at B = 1 that
  // is the difference between 160 KB and 10 KB per workgroup for fc2).
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(x), 0, CG * 16 * K * (int)sizeof(T), 0x00020000);
  unsigned xoff[CG];
#pragma unroll
  for (int g = 0; g < CG; ++g)
    xoff[g] = (g * 16 + fr < B) ? (unsigned)((g * 16 * K + lane * E) * (int)sizeof(T)) : 0x80000000u;
  auto load_x = [&](int s0) {
    if constexpr (CG > 1) {   // several groups: step-major, the order mfma_round consumes them in
#pragma unroll
      for (int i = 0; i < SK_MAXS; ++i)
#pragma unroll
        for (int g = 0; g < CG; ++g)
#pragma unroll
          for (int m = 0; m < XPS; ++m) {
            const unsigned step_bytes = (unsigned)((min(s0 + i, S - 1) * XPS + m) * (64 * E) * (int)sizeof(T));
            xq[g][i * XPS + m] = __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(xr, xoff[g] + step_bytes, 0, 0));
          }
    } else {
#pragma unroll
      for (int g = 0; g < CG; ++g)
#pragma unroll
        for (int i = 0; i < SK_MAXS; ++i)
#pragma unroll
          for (int m = 0; m < XPS; ++m) {
            const unsigned step_bytes = (unsigned)((min(s0 + i, S - 1) * XPS + m) * (64 * E) * (int)sizeof(T));
            xq[g][i * XPS + m] = __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(xr, xoff[g] + step_bytes, 0, 0));
          }
    }
  };

  auto ring_w = [&](int step, int tile_ofs = 0) -> u32x4_t {   // one weight fragment of this workgroup's tile (RING: every step is inside the matrix)
    const int tl = min(tile0 + tile_ofs, n_tiles - 1);
    if constexpr (TR == 16) {
      return sk_load_w<T>(W + ((long long)tl * S * 64 + lane) * E + (long long)step * (64 * E));
    } else {
      const unsigned lane_off = (fr < TR) ? (unsigned)((kq * TR + fr) * 16) : 0x80000000u;
      return __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(
          wr, lane_off + (unsigned)tl * (unsigned)(S * 4 * TR * 16) + (unsigned)(step * (4 * TR * 16)), 0, 2 /* nt */));
    }
  };
  auto ring_x = [&](int g, int step) -> u32x4_t {
    return __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(xr, xoff[g] + (unsigned)(step * (64 * E) * (int)sizeof(T)), 0, 0));
  };
  if constexpr (RING) {
    // HBM first, then the first DX steps of activations in consumption order; everything else is requested as registers free up
#pragma unroll
    for (int i = 0; i < DW; ++i) {
      rw[i] = ring_w(s_lo + i);
      if constexpr (DUAL) rw2[i] = ring_w(s_lo + i, 1);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < DX; ++i)
#pragma unroll
      for (int g = 0; g < CG; ++g) rx[i][g] = ring_x(g, s_lo + i);
    __builtin_amdgcn_sched_barrier(0);
  } else if constexpr (CG > 1) {
    // several groups of streams: a wavefront asks for up to 20 KiB of activations per round.  The HBM requests go first (their
    // latency is the long one; vmcnt retires in order, so by the time an activation fragment has arrived its weights have too)
    load_w(tile0, s_lo);
    __builtin_amdgcn_sched_barrier(0);
    load_x(s_lo);
    __builtin_amdgcn_sched_barrier(0);
  } else {
    load_x(s_lo);
    __builtin_amdgcn_sched_barrier(0);  // request order = consumption order: hipcc must not reorder the groups
    load_w(tile0, s_lo);
    __builtin_amdgcn_sched_barrier(0);
  }
  // (2) everything else (epilogue operands, outputs, cache geometry): ONE batch of scalar loads from the argument block, waited for
  // here, behind the operand requests that are already on their way
  asm volatile("" ::"s"(bias), "s"(res), "s"(gw_p), "s"(cb_p), "s"(a.gelu), "s"(ldy), "s"(d_model), "s"(cache_bstride), "s"(cache_hstride), "s"(y),
               "s"(y_f32), "s"(kcache), "s"(vcache), "s"(stt), "s"(u_p), "s"(nsplit), "s"(stats_p), "s"(rows_streams));
  if (EPI == SK_KV || EPI == SK_KV_RAG) cur_pos = stt->pos;
  load_epi(tile0, e_c, e_gw, e_res);
  __builtin_amdgcn_sched_barrier(0);  // ... nor hoist arithmetic between the requests

  float mean[GPT], rstd[GPT];
#pragma unroll
  for (int g = 0; g < GPT; ++g) { mean[g] = 0.f; rstd[g] = 1.f; }
  const int n_grp = MULTI ? RG : 1;
  f32x4_t accd[DUAL ? CG : 1];   // DUAL: the second tile's accumulators, filled together with the first tile's
  for (int grp = 0; grp < n_grp; ++grp) {
    const int tile = tile0 + grp;
    f32x4_t acc[CG], acc2[SPLIT2 ? CG : 1];   // acc2: the second half of the wavefront's K slice (SPLIT2, see the kernel's header)
    float ps[CG], pss[CG];
#pragma unroll
    for (int g = 0; g < CG; ++g) { acc[g] = f32x4_t{0.f, 0.f, 0.f, 0.f}; ps[g] = 0.f; pss[g] = 0.f; }
#pragma unroll
    for (int g = 0; g < (SPLIT2 ? CG : 1); ++g) acc2[g] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const int s_mid = SPLIT2 ? (int)((long long)(2 * wave + 1) * S / (2 * NW)) : 0x7fffffff;   // first step of slice 2 wave + 1 of 16
    auto mfma_round = [&](int s0) {
#pragma unroll
      for (int i = 0; i < SK_MAXS; ++i) {
        const bool on = s0 + i < s_hi;  // wave-uniform: steps past this wavefront's K slice contribute zero
        const bool second = SPLIT2 && s0 + i >= s_mid;   // wave-uniform: which of the two accumulator sets this step belongs to
        const u32x4_t zero = u32x4_t{0u, 0u, 0u, 0u};
        if constexpr (A16) {
          // fragments m = 0, 1 live in the first 16 bytes (block h = 0), m = 2, 3 in the second (h = 1)
          u32x4_t wf[4];
          sk_widen8(on ? wq[2 * i] : zero, __builtin_bit_cast(float, (unsigned)(wsc[i] & 0xff) << 23), wf[0], wf[1]);
          sk_widen8(on ? wq[2 * i + 1] : zero, __builtin_bit_cast(float, (unsigned)(wsc2[i] & 0xff) << 23), wf[2], wf[3]);
          if (SPLIT2 && second) {   // (a branch around matrix instructions only: no load inside)
#pragma unroll
            for (int g = 0; g < (SPLIT2 ? CG : 1); ++g)
#pragma unroll
              for (int m = 0; m < 4; ++m) acc2[g] = sk_mfma<T>(wf[m], on ? xq[g][i * 4 + m] : zero, acc2[g]);
          } else {
#pragma unroll
          for (int g = 0; g < CG; ++g)
#pragma unroll
            for (int m = 0; m < 4; ++m) {
              const u32x4_t xv = on ? xq[g][i * 4 + m] : zero;
              if (LN && (!MULTI || grp == 0)) sk_stats<T>(xv, ps[g], pss[g]);
              acc[g] = sk_mfma<T>(wf[m], xv, acc[g]);
            }
          }
        } else if (W8) {
          const u32x4_t w0 = on ? wq[2 * i] : zero, w1 = on ? wq[2 * i + 1] : zero;
          const v8i_t wb = {(int)w0[0], (int)w0[1], (int)w0[2], (int)w0[3], (int)w1[0], (int)w1[1], (int)w1[2], (int)w1[3]};
#pragma unroll
          for (int g = 0; g < CG; ++g) {
            u32x4_t xv[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
              xv[m] = on ? xq[g][i * 4 + m] : zero;
              if (LN && (!MULTI || grp == 0)) sk_stats<T>(xv[m], ps[g], pss[g]);
            }
            int xs;
            const v8i_t xb = sk_quant_mx8(xv, xs);
            acc[g] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wb, xb, acc[g], 0, 0, 0, wsc[i], 0, xs);
          }
        } else {
          const u32x4_t wv = on ? wq[i] : zero;
          if (SPLIT2 && second) {
#pragma unroll
            for (int g = 0; g < (SPLIT2 ? CG : 1); ++g) acc2[g] = sk_mfma<T>(wv, on ? xq[g][i] : zero, acc2[g]);
          } else {
#pragma unroll
          for (int g = 0; g < CG; ++g) {
            const u32x4_t xv = on ? xq[g][i] : zero;
            if (LN && (!MULTI || grp == 0)) sk_stats<T>(xv, ps[g], pss[g]);
            acc[g] = sk_mfma<T>(wv, xv, acc[g]);
          }
          }
        }
      }
    };
    if constexpr (RING) {
      static_assert(!SPLIT2 || SK_MAXS % 2 == 0, "SPLIT2 rings: the slice's midpoint is a step boundary");
      static_assert(!(SPLIT2 && DUAL), "SPLIT2 is the long-K residual projection, DUAL the 5120-row launches");
      if (!DUAL || grp == 0) {
#pragma unroll
        for (int g = 0; g < (DUAL ? CG : 1); ++g) accd[g] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < SK_MAXS; ++i) {
#pragma unroll
          for (int g = 0; g < CG; ++g) {
            const u32x4_t xv = rx[i % DX][g];
            if (LN) sk_stats<T>(xv, ps[g], pss[g]);
            if constexpr (SPLIT2) {   // (compile-time: S = NW * SK_MAXS, so s_mid = s_lo + SK_MAXS / 2)
              if (i >= SK_MAXS / 2) acc2[g] = sk_mfma<T>(rw[i % DW], xv, acc2[g]);
              else acc[g] = sk_mfma<T>(rw[i % DW], xv, acc[g]);
            } else {
              acc[g] = sk_mfma<T>(rw[i % DW], xv, acc[g]);
              if constexpr (DUAL) accd[g] = sk_mfma<T>(rw2[i % DW], xv, accd[g]);
            }
          }
          if (i + DX < SK_MAXS) {
#pragma unroll
            for (int g = 0; g < CG; ++g) rx[i % DX][g] = ring_x(g, s_lo + i + DX);
          }
          if (i + DW < SK_MAXS) {
            rw[i % DW] = ring_w(s_lo + i + DW);
            if constexpr (DUAL) rw2[i % DW] = ring_w(s_lo + i + DW, 1);
          }
          __builtin_amdgcn_sched_barrier(0);   // keep the software pipeline in this order
        }
      } else {   // DUAL, second tile: contracted together with the first (same K slices, same order: bit-identical to a tile of its own)
#pragma unroll
        for (int g = 0; g < (DUAL ? CG : 1); ++g) acc[g] = accd[g];
      }
    } else {
    mfma_round(s_lo);  // operands already in flight
    for (int s0 = s_lo + SK_MAXS; s0 < s_hi; s0 += SK_MAXS) {  // K longer than one round of fragments
      if constexpr (CG > 1) {
        load_w(tile, s0);
        __builtin_amdgcn_sched_barrier(0);
        load_x(s0);
      } else {
        load_x(s0);
        load_w(tile, s0);
      }
      mfma_round(s0);
    }
    }
    // operands of the tile after this one are requested now, behind the reduction and the epilogue of the current one
    // (MULTI is only launched with a single round of fragments per tile, so the activation fragments stay in registers)
    float n_c = 0.f, n_gw = 0.f, n_res[GPT];
#pragma unroll
    for (int g = 0; g < GPT; ++g) n_res[g] = 0.f;
    if (MULTI) {
      const int nt = min(tile + 1, n_tiles - 1);
      if constexpr (!RING) load_w(nt, s_lo);
      load_epi(nt, n_c, n_gw, n_res);
    }
    // D[i = weight row (lane>>4)*4 + reg][j = stream lane&15]
    if (MULTI && grp > 0) __syncthreads();  // previous tile's readers are done with `red`
    if constexpr (SPLIT2) {   // P_2w + P_2w+1: the addition the 16-wavefront kernel performs on its LDS tiles
#pragma unroll
      for (int g = 0; g < (SPLIT2 ? CG : 1); ++g) acc[g] += acc2[g];
    }
#pragma unroll
    for (int g = 0; g < CG; ++g)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[(wave * CG + g) * kRedTile + (kq * 4 + r) * kRedStride + fr] = acc[g][r];
    if (LN && (!MULTI || grp == 0)) {
#pragma unroll
      for (int g = 0; g < CG; ++g) {
        const float s1 = tw_xor32_sum(tw_xor16_sum(ps[g])), s2 = tw_xor32_sum(tw_xor16_sum(pss[g]));
        if (lane < 16) { pstat[wave][g * 16 + fr][0] = s1; pstat[wave][g * 16 + fr][1] = s2; }
      }
    }
    __syncthreads();
    if (tid < (EALL ? 512 : 256)) {
      const int j = ej, i = ei;  // stream (within its group), row: 16 consecutive rows of one stream per 16 threads
      const int n = tile * TR + i;
#pragma unroll
      for (int gi = 0; gi < GPT; ++gi) {
        const int g = EALL ? gi * 2 + eh : gi;
        const int jg = g * 16 + j;  // stream
        float v = 0.f;
        if constexpr (NW >= 16) {   // sixteen slices added in pairs: the order the 8-wavefront SPLIT2 flavour reproduces (kernel header)
#pragma unroll
          for (int w = 0; w < NW; w += 2)
            v += red[(w * CG + g) * kRedTile + i * kRedStride + j] + red[((w + 1) * CG + g) * kRedTile + i * kRedStride + j];
        } else {
#pragma unroll
          for (int w = 0; w < NW; ++w) v += red[(w * CG + g) * kRedTile + i * kRedStride + j];
        }
        const float vraw = v;
        if (LN) {
          if (!MULTI || grp == 0) {
            float sx = 0.f, sxx = 0.f;
#pragma unroll
            for (int w = 0; w < NW; ++w) { sx += pstat[w][jg][0]; sxx += pstat[w][jg][1]; }
            const float inv_k = __builtin_amdgcn_rcpf((float)K);
            tw_ln_scalars(sx, sxx, inv_k, mean[gi], rstd[gi]);
          }
          v = tw_ln_apply(v, mean[gi], rstd[gi], e_gw, e_c);
        } else {
          v += e_c;
        }
        if (EPI == SK_GELU) v = gelu_exact<T>(v);
        if (EPI == SK_RES) v += e_res[gi];
        if (EPI == SK_RES && u_p) {   // (kernel-uniform) LayerNorm statistics of the residual rows of this tile, as stored
          const float xs = (tile < n_tiles && n < nsplit && jg < B && i < TR) ? (float)tw_cast<T>(v) : 0.f;
          const float s1 = tw_row16_sum(xs), s2 = tw_row16_sum(xs * xs);   // the 16 threads of one stream are one DPP row
          if (i == 0 && jg < B && tile < n_tiles && tile * TR < nsplit) {
            float* sp = stats_p + ((long long)jg * (nsplit / TR) + tile) * 2;
            sp[0] = s1;
            sp[1] = s2;
          }
        }
        if (tile < n_tiles && n < N && jg < B && i < TR) {
          if (EPI == SK_F32) {
            y_f32[(long long)jg * N + n] = v;
          } else if (EPI == SK_KV || EPI == SK_KV_RAG) {
            // 0: query -> y, 1: key -> K cache, 2: value -> V^T cache, 3: cross query ahead   (one predicated store; compares and a
            // host-side per-head stride instead of the 32- and 64-bit divisions by run-time values this epilogue used to carry: ~0.3 us)
            const int seg = (n >= d_model) + (n >= 2 * d_model) + (n >= 3 * d_model);
            const int nn = n - seg * d_model, hh = nn >> 6, cc = nn & 63;
            if (seg == 3) {   // cross query ahead: x . W'^T + c0 WITHOUT this LayerNorm (its own is applied by the consumer)
              u_p[(long long)jg * d_model + nn] = vraw + e_c;
            } else {
              int srow, prow;   // rows mode (prefill): row jg is stream jg % rs at position cur_pos + jg / rs
              tw_row_of(jg, rows_streams, cur_pos, srow, prow);
              if (EPI == SK_KV_RAG) { srow = jg; prow = tw_row_pos(cur_pos, a.n_pad[jg]); }   // ragged step: row = stream (jg < B <= 64)
              const long long hb = (long long)srow * cache_bstride + (long long)hh * cache_hstride;  // (stream, head)
              T* dst = seg == 0 ? y + (long long)jg * ldy + n
                                : (seg == 1 ? kcache + hb + tw_kf_index<T>(prow, cc) : vcache + hb + tw_vtf_index<T>(prow, cc));
              *dst = tw_cast<T>(v);
            }
          } else if (EPI == SK_STORE) {
            y[(long long)jg * ldy + n] = tw_cast<T>(v);  // row-major [B][ldy] (the attention kernels' query operand)
          } else if (EPI == SK_RES) {
            if (n >= nsplit) u_p[(long long)jg * (N - nsplit) + (n - nsplit)] = v;   // composed half: u += attn . Wc^T
            else y[(long long)g * 16 * nsplit + tw_xt_index<T>(j, n)] = tw_cast<T>(v);       // residual stream, fragment-major
          } else {
            y[(long long)g * 16 * N + tw_xt_index<T>(j, n)] = tw_cast<T>(v);    // feeds the next projection: fragment-major
          }
        }
      }
    }
    if (MULTI) {
      e_c = n_c; e_gw = n_gw;
#pragma unroll
      for (int g = 0; g < GPT; ++g) e_res[g] = n_res[g];
    }
  }
}

// Row-major W[N][K] -> fragment-major layout read by skinny_mfma_kernel: for tile t = n/16 and step s = k/(4E) one
// 1-KiB block holds the MFMA A operand exactly as the 64 lanes consume it, lane l = kq*16 + fr <- row t*16+fr,
// 16-B vector s*4+kq.  A wavefront's K slice is then ONE contiguous run (its requests are full cache lines in address
// order, like a plain streaming copy) instead of 16 row segments of 64 B per request.  Rows >= N are zero.
template <typename T>
__global__ __launch_bounds__(256) void tile_weights_kernel(const T* __restrict__ src, T* __restrict__ dst, int N, int K, int TR) {
  constexpr int E = ElemTraits<T>::kPer16B;
  const int S = K / E / 4;
  const int LT = 4 * TR;                                            // 16-B vectors per (tile, step): 64 for 16-row tiles
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;  // destination vector index
  const long long total = (long long)((N + TR - 1) / TR) * S * LT;
  if (v >= total) return;
  const int l = (int)(v % LT);
  const long long ts = v / LT;
  const int s = (int)(ts % S);
  const int t = (int)(ts / S);
  const int n = t * TR + (l % TR), kv = s * 4 + (l / TR);
  u32x4_t val = u32x4_t{0u, 0u, 0u, 0u};
  if (n < N) val = *reinterpret_cast<const u32x4_t*>(src + (long long)n * K + (long long)kv * E);
  *reinterpret_cast<u32x4_t*>(dst + v * E) = val;
}

// Row-major bf16 W[N][K] -> MXFP8 operand of skinny_mfma_kernel<.., W8 = true>: per 16-row tile and 128-k step, 2 KiB of
// e4m3 as [half][lane][16 B] (lane = kq*16 + row%16; its 32 bytes, fragment m / element e at byte 8m + e, are
// W[row][(4s + m)*32 + kq*8 + e]: the same k set the activation lane (stream, kq) holds) followed, in a separate array, by
// one scale byte per lane (already placed in the lane the MFMA reads it from).  Quantisation = sk_quant_mx8, i.e. identical
// to what the projection kernel does to the activations.
__global__ __launch_bounds__(256) void quant_mx8_kernel(const bf16_t* __restrict__ src, unsigned char* __restrict__ dst,
                                                        unsigned char* __restrict__ scales, int N, int K, int TR) {
  const int S = K / 128;
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;  // (16-row tile, step, lane): quantisation always works on
  const long long total = (long long)((N + 15) / 16) * S * 64;    // whole wavefronts = 16 rows x 4 k-groups
  if (v >= total) return;
  const int l = (int)(v & 63);
  const long long ts = v >> 6;
  const int s = (int)(ts % S);
  const long long t = ts / S;
  const int n = (int)t * 16 + (l & 15), kq = l >> 4;
  u32x4_t xv[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    xv[m] = u32x4_t{0u, 0u, 0u, 0u};
    if (n < N) xv[m] = *reinterpret_cast<const u32x4_t*>(src + (long long)n * K + (4 * s + m) * 32 + kq * 8);
  }
  int sb;  // (whole wavefronts reach this point: `total` is a multiple of 64)
  const v8i_t q = sk_quant_mx8(xv, sb);
  // storage: tiles of TR rows (16, or 8 for the narrow projections): [tile][step][half][kq * TR + row % TR][16 B]
  const int fr = l & 15;
  const long long tile = t * (16 / TR) + fr / TR;
  const int slot = kq * TR + fr % TR;
  unsigned char* blk = dst + (tile * S + s) * (long long)(8 * TR * 16);
  *reinterpret_cast<u32x4_t*>(blk + slot * 16) = u32x4_t{(unsigned)q[0], (unsigned)q[1], (unsigned)q[2], (unsigned)q[3]};
  *reinterpret_cast<u32x4_t*>(blk + 4 * TR * 16 + slot * 16) = u32x4_t{(unsigned)q[4], (unsigned)q[5], (unsigned)q[6], (unsigned)q[7]};
  scales[(tile * S + s) * (long long)(4 * TR) + slot] = (unsigned char)sb;
}

// W[n,:] *= g (in place, rounded to T); gw[n] = sum_k g[k] W[n,k]; cb[n] = sum_k beta[k] W[n,k] + bias[n]   (one wave per row)
template <typename T>
__global__ __launch_bounds__(256) void fold_ln_kernel(T* __restrict__ W, const T* __restrict__ Wsrc, const T* __restrict__ g,
                                                       const T* __restrict__ beta, const T* __restrict__ bias,
                                                       float* __restrict__ gw, float* __restrict__ cb, int N, int K) {
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (n >= N) return;
  float sg = 0.f, sb = 0.f;
  for (int k = lane; k < K; k += 64) {
    const float w = (float)Wsrc[(long long)n * K + k];
    const float gk = (float)g[k];
    const T wr = (T)(gk * w);
    sg += (float)wr;   // of the weights AS STORED: rstd (x W'^T - mean gw) is then exactly rstd (x - mean) W'^T
    sb += (float)beta[k] * w;
    W[(long long)n * K + k] = wr;
  }
  sg = wave_sum(sg);
  sb = wave_sum(sb);
  if (lane == 0) {
    gw[n] = sg;
    cb[n] = sb + (bias ? (float)bias[n] : 0.f);
  }
}

// Load-time composition for "cross query ahead": out = A . Bm (row-major [N][J] x [J][K], float32 accumulation, one rounding
// to T), c0 = A . bvec.  Runs once per decoder layer in tw_finalize_weights: plain 16x16 LDS tiles, nothing to tune.
template <typename T>
__global__ __launch_bounds__(256) void compose_kernel(const T* __restrict__ A, const T* __restrict__ Bm, const T* __restrict__ bvec,
                                                      T* __restrict__ out, float* __restrict__ c0, int N, int J, int K) {
  __shared__ float ta[16][17], tb[16][17];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int n = blockIdx.y * 16 + ty, k = blockIdx.x * 16 + tx;
  float acc = 0.f, accb = 0.f;
  for (int j0 = 0; j0 < J; j0 += 16) {
    ta[ty][tx] = (n < N && j0 + tx < J) ? (float)A[(long long)n * J + j0 + tx] : 0.f;
    tb[ty][tx] = (j0 + ty < J && k < K) ? (float)Bm[(long long)(j0 + ty) * K + k] : 0.f;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 16; ++j) acc = fmaf(ta[ty][j], tb[j][tx], acc);
    if (blockIdx.x == 0 && tx == 0 && bvec) {
      for (int j = 0; j < 16 && j0 + j < J; ++j) accb = fmaf(ta[ty][j], (float)bvec[j0 + j], accb);
    }
    __syncthreads();
  }
  if (n < N && k < K) out[(long long)n * K + k] = (T)acc;
  if (blockIdx.x == 0 && tx == 0 && n < N && c0) c0[n] = accb;
}

// ---------------------------------------------------------------------------------------------
// single-query attention (decoder self-attention over the growing cache, cross-attention over the
// cached encoder K/V).  One workgroup per (stream, head), NW wavefronts, each owning 64 consecutive
// keys per chunk of NW*64 keys.  Both products run on the matrix cores although there is only one
// query: K is the A operand (16 keys x 64 dims per tile) against the query broadcast over the 16 B
// columns, V^T is the A operand (16 dims x 4E keys) against the probabilities.  15/16 of the MFMA
// columns are redundant, which is free - the kernel moves 128 KiB per head (cross attention, 10 s)
// and is bound by how fast one CU can take that in, and the VALU formulation (a dot product, a
// 16-lane reduction and an exp per key and 8-byte loads) cost more issue time than the loads.
// K and V^T are stored fragment-major (tw_kf_index / tw_vtf_index in tw_common.h), written in that
// layout by the producers (cross-K/V GEMM epilogue, QKV projection epilogue): every request of a
// wavefront is 1 KiB contiguous and a wavefront's 64 keys are one 8-KiB run of each operand.
// Softmax in fp32 (scores -> LDS, block max, exp, sum); probabilities are rounded to the storage
// type for the P.V product as the reference does (HF casts attn_weights to the value dtype).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_max(float v) { return tw_wave_max(v); }

// Fused query operand (FusedQ, tw_common.h): the query of the cross attention is the LayerNorm'd projection of the residual
// stream, q = rstd (u - mean gw) + cb, with u = x . W'^T accumulated by the two projections that ran before (api.hip:
// decode_core).  Every wavefront folds the partial row statistics the residual launch left behind (one coalesced 8-byte
// request per lane and 64 partials; reading the fragment-major row itself costs 64 cache lines per request and made the
// launch 3 us slower) and lane l forms element l of the head's query; the MFMA operand order is then read back from a 64-element LDS
// row PRIVATE to the wavefront (LDS operations of one wavefront stay in order: no barrier).  All requests are issued before
// the K / V^T requests of the caller and consumed after them, i.e. this arithmetic runs while the K fragments are in flight.
template <typename T>
struct QRaw {
  static constexpr int MAXP = 3;   // partial statistics per lane: n_part <= 192 (d = 1280 in 8-row tiles: 160)
  float u, gw, cb;
  f32x2_t st[MAXP];
};
template <typename T>
__device__ __forceinline__ void fq_request(QRaw<T>& r, const FusedQ& fq, int b, int h, int lane) {
  r.u = fq.u[(long long)b * fq.d + h * 64 + lane];
  r.gw = fq.gw[h * 64 + lane];
  r.cb = fq.cb[h * 64 + lane];
  const f32x2_t* sp = reinterpret_cast<const f32x2_t*>(fq.stats) + (long long)b * fq.n_part;
#pragma unroll
  for (int m = 0; m < QRaw<T>::MAXP; ++m) r.st[m] = sp[min(lane + 64 * m, fq.n_part - 1)];
}
// qrow: this wavefront's 64-element LDS row.  Returns with the element `lane` of the query stored there (type T).
template <typename T>
__device__ __forceinline__ void fq_finish(const QRaw<T>& r, const FusedQ& fq, int lane, T* qrow) {
  float s = 0.f, ss = 0.f;
#pragma unroll
  for (int m = 0; m < QRaw<T>::MAXP; ++m) {
    const bool on = lane + 64 * m < fq.n_part;
    s += on ? r.st[m][0] : 0.f;
    ss += on ? r.st[m][1] : 0.f;
  }
  s = tw_wave_sum(s);
  ss = tw_wave_sum(ss);
  const float inv_k = __builtin_amdgcn_rcpf((float)fq.d);
  float mean, rstd;
  tw_ln_scalars(s, ss, inv_k, mean, rstd);
  qrow[lane] = tw_cast<T>(tw_ln_apply(r.u, mean, rstd, r.gw, r.cb));
}

// SINGLE: n_bound <= NW*64, so every K and V^T fragment of the head is requested before anything is waited for
// (one memory round trip per head); otherwise two passes over chunks of NW*64 keys.
// n_keys = valid keys (rest masked), n_bound = keys addressable (multiple of 64, <= rows allocated per head).
// sc: LDS float[n_bound] (unnormalised probabilities on return); red: LDS float[2*NW + NW*64].
// Returns 1/L in every thread; threads 0..63 write the context vector (fragment-major activation layout).
// FQ: the query comes as a FusedQ (stream fq_b, head fq_h; qst = LDS T[NW][64]) instead of through q
template <typename T, int NW, bool SINGLE, bool FQ = false>
__device__ __forceinline__ float attn_mfma_block(const T* __restrict__ q, const T* __restrict__ kf, const T* __restrict__ vtf,
                                                 int n_keys, int n_bound, float* sc, float* red, T* __restrict__ out_base,
                                                 int out_j, int out_k0, const FusedQ& fq = FusedQ{}, int fq_b = 0, int fq_h = 0,
                                                 T* qst = nullptr) {
  constexpr int E = ElemTraits<T>::kPer16B;
  constexpr int DS = 64 / (4 * E);  // dim steps per key tile (QK^T) = key steps per 64 keys (P.V)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, kq = lane >> 4;
  const int n_chunks = SINGLE ? 1 : (n_bound + NW * 64 - 1) / (NW * 64);
  const int last64 = n_bound / 64 - 1;  // last addressable 64-key group
  u32x4_t qf[DS], kfr[4 * DS], vfr[4 * DS];
  auto load_k = [&](int g64) {  // 64 keys = 4 tiles x DS steps = 4*DS KiB contiguous
    const T* p = kf + ((long long)min(g64, last64) * (4 * DS) * 64 + lane) * E;
#pragma unroll
    for (int i = 0; i < 4 * DS; ++i) kfr[i] = *reinterpret_cast<const u32x4_t*>(p + (long long)i * 64 * E);
  };
  auto load_v = [&](int g64) {  // 64 keys = DS key steps x 4 dim tiles
    const T* p = vtf + ((long long)min(g64, last64) * (4 * DS) * 64 + lane) * E;
#pragma unroll
    for (int i = 0; i < 4 * DS; ++i) vfr[i] = *reinterpret_cast<const u32x4_t*>(p + (long long)i * 64 * E);
  };
  // K first: its addresses are formed from the leading (preloaded) kernel arguments alone, so these requests leave at once;
  // the query side needs the rest of the argument block (one scalar batch, pinned here) and goes out behind them
  load_k(wave);
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("" ::"s"(q), "s"(fq.u), "s"(fq.stats), "s"(fq.n_part), "s"(fq.gw), "s"(fq.cb), "s"(fq.d));
  QRaw<T> qr;
  if constexpr (FQ) {
    fq_request<T>(qr, fq, fq_b, fq_h, lane);
  } else {
#pragma unroll
    for (int ds = 0; ds < DS; ++ds) qf[ds] = *reinterpret_cast<const u32x4_t*>(q + ds * 4 * E + kq * E);
  }
  if (SINGLE) load_v(wave);
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (FQ) {
    T* qrow = qst + wave * 64;
    fq_finish<T>(qr, fq, lane, qrow);
#pragma unroll
    for (int ds = 0; ds < DS; ++ds) qf[ds] = *reinterpret_cast<const u32x4_t*>(qrow + ds * 4 * E + kq * E);
  }

  // ---- scores: D[i = key (lane>>4)*4 + r][j] identical in every column j; column 0 lanes publish them ----
  float m = -1.0e30f;
  for (int c = 0; c < n_chunks; ++c) {
    const int g64 = c * NW + wave;
    if (c > 0) load_k(g64);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      f32x4_t acc = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ds = 0; ds < DS; ++ds) acc = sk_mfma<T>(kfr[a * DS + ds], qf[ds], acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int t = g64 * 64 + a * 16 + kq * 4 + r;
        const float sv = (t < n_keys) ? acc[r] : -1.0e30f;
        m = fmaxf(m, sv);
        if (fr == 0 && t < n_bound) sc[t] = sv;
      }
    }
  }
  m = tw_xor32_max(tw_xor16_max(m));
  if (lane == 0) red[wave] = m;
  __syncthreads();
  float M = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) M = fmaxf(M, red[w]);

  // ---- probabilities of this wavefront's own keys (written back to LDS for the B operand and the alignment rows) and P.V
  f32x4_t o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float ls = 0.f;
  for (int c = 0; c < n_chunks; ++c) {
    const int g64 = c * NW + wave;
    if (!SINGLE) load_v(g64);
    const int t0 = g64 * 64 + lane;  // one key per lane
    float pr = 0.f;
    if (t0 < n_bound) {
      pr = (t0 < n_keys) ? expf(sc[t0] - M) : 0.f;
      sc[t0] = pr;
    }
    ls += pr;
#pragma unroll
    for (int ks = 0; ks < DS; ++ks) {
      float pv[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int t = g64 * 64 + ks * 4 * E + kq * E + e;
        pv[e] = (t < n_bound) ? sc[t] : 0.f;  // same wavefront wrote these: LDS operations of a wavefront stay in order
      }
      const u32x4_t pf = pack16<T>(pv);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) o[dt] = sk_mfma<T>(vfr[ks * 4 + dt], pf, o[dt]);
    }
  }
  ls = tw_wave_sum(ls);
  float* wl = red + NW;       // [NW]
  float* wo = red + 2 * NW;   // [NW][64]
  if (lane == 0) wl[wave] = ls;
  if (fr == 0) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r) wo[wave * 64 + dt * 16 + kq * 4 + r] = o[dt][r];
  }
  __syncthreads();
  float L = 0.f;
#pragma unroll
  for (int w = 0; w < NW; ++w) L += wl[w];
  const float inv = 1.0f / L;
  if (tid < 64) {
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) v += wo[w * 64 + tid];
    out_base[tw_xt_index<T>(out_j, out_k0 + tid)] = (T)(v * inv);  // feeds o-proj: fragment-major (tw_common.h)
  }
  return inv;
}

// fp8 variant of attn_mfma_block for the cross attention of TW_BF16_MXFP8 contexts (bf16 activations): K and V^T are stored as
// e4m3 with one power-of-two scale byte per (key, head) (layouts: tw_kf8_index / tw_vtf8_index, written by gemm_epilogue_kv8),
// which halves the bytes the step has to stream - at 16 streams the cross-attention K/V are as many bytes as all weights.
// The products stay bf16 MFMAs: fragments are widened in registers (v_cvt_scalef32_pk_bf16_fp8; the K scale is applied by
// that instruction, lane = key; the V scale multiplies the probability of its key before the P.V operand is packed), so q and
// the probabilities are NOT quantised.  A 16-B fp8 vector holds 16 dims (K) / 16 keys (V^T), i.e. two bf16 MFMA operands:
// the contraction index of an MFMA is order-free, so the q / probability operands are simply gathered in the same order.
__device__ __forceinline__ void kv8_widen(const u32x4_t& raw, float X, u32x4_t& lo, u32x4_t& hi) {
  lo[0] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)raw[0], X, false));
  lo[1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)raw[0], X, true));
  lo[2] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)raw[1], X, false));
  lo[3] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)raw[1], X, true));
  hi[0] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)raw[2], X, false));
  hi[1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)raw[2], X, true));
  hi[2] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)raw[3], X, false));
  hi[3] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)raw[3], X, true));
}

// G = 64-key groups per wavefront (1, 2 or 3: up to 512 / 1024 / 1536 keys with 8 wavefronts, i.e. every chunk length up to
// 30 s).  At 32 registers per group and operand the whole head fits the register file, so - unlike the bf16 kernel, which
// falls back to two dependent passes above 512 keys - EVERY fragment of the head is requested before anything is waited for:
// one memory round trip per head whatever the chunk length.
template <int NW, int G, bool FQ = false>
__device__ __forceinline__ float attn_mfma_block_kv8(const bf16_t* __restrict__ q, const unsigned char* __restrict__ kf8,
                                                     const unsigned char* __restrict__ vtf8, const unsigned char* __restrict__ ksc,
                                                     const unsigned char* __restrict__ vsc, int n_keys, int n_bound, float* sc,
                                                     float* scv, float* red, bf16_t* __restrict__ out_base, int out_j, int out_k0,
                                                     const FusedQ& fq = FusedQ{}, int fq_b = 0, int fq_h = 0,
                                                     bf16_t* qst = nullptr) {
  typedef bf16_t T;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, kq = lane >> 4;
  const int last64 = n_bound / 64 - 1;
  u32x4_t qf[2], kraw[G][4], vraw[G][4];
  unsigned ks4[G], vsb[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {  // 64 keys = 4 tiles of 1 KiB + their 64 scale bytes ([group][key % 16][tile]: one 32-bit load)
    const int gi = min(g * NW + wave, last64);
    const unsigned char* p = kf8 + ((long long)gi * 4 * 64 + lane) * 16;
#pragma unroll
    for (int a = 0; a < 4; ++a) kraw[g][a] = *reinterpret_cast<const u32x4_t*>(p + a * 1024);
    ks4[g] = *reinterpret_cast<const unsigned*>(ksc + gi * 64 + fr * 4);
  }
  __builtin_amdgcn_sched_barrier(0);
  // the query side behind the K requests (see attn_mfma_block)
  asm volatile("" ::"s"(q), "s"(fq.u), "s"(fq.stats), "s"(fq.n_part), "s"(fq.gw), "s"(fq.cb), "s"(fq.d));
  QRaw<T> qr;
  if constexpr (FQ) {
    fq_request<T>(qr, fq, fq_b, fq_h, lane);
  } else {
    qf[0] = *reinterpret_cast<const u32x4_t*>(q + kq * 16);
    qf[1] = *reinterpret_cast<const u32x4_t*>(q + kq * 16 + 8);
  }
#pragma unroll
  for (int g = 0; g < G; ++g) {  // 64 keys x 64 dims = 4 dim tiles of 1 KiB; lane `lane` also fetches the scale of ITS key
    const int gi = min(g * NW + wave, last64);
    const unsigned char* p = vtf8 + ((long long)gi * 4 * 64 + lane) * 16;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) vraw[g][dt] = *reinterpret_cast<const u32x4_t*>(p + dt * 1024);
    vsb[g] = vsc[gi * 64 + lane];
  }
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (FQ) {
    T* qrow = qst + wave * 64;
    fq_finish<T>(qr, fq, lane, qrow);
    qf[0] = *reinterpret_cast<const u32x4_t*>(qrow + kq * 16);
    qf[1] = *reinterpret_cast<const u32x4_t*>(qrow + kq * 16 + 8);
  }

  float m = -1.0e30f;
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int g64 = g * NW + wave;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      u32x4_t k0, k1;
      kv8_widen(kraw[g][a], __builtin_bit_cast(float, ((ks4[g] >> (8 * a)) & 0xffu) << 23), k0, k1);
      f32x4_t acc = f32x4_t{0.f, 0.f, 0.f, 0.f};
      acc = sk_mfma<T>(k0, qf[0], acc);
      acc = sk_mfma<T>(k1, qf[1], acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int t = g64 * 64 + a * 16 + kq * 4 + r;
        const float sv = (t < n_keys) ? acc[r] : -1.0e30f;
        m = fmaxf(m, sv);
        if (fr == 0 && t < n_bound) sc[t] = sv;
      }
    }
  }
  m = tw_xor32_max(tw_xor16_max(m));
  if (lane == 0) red[wave] = m;
  __syncthreads();
  float M = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) M = fmaxf(M, red[w]);

  f32x4_t o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float ls = 0.f;
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int g64 = g * NW + wave;
    const int t0 = g64 * 64 + lane;  // one key per lane
    float pr = 0.f;
    if (t0 < n_bound) {
      pr = (t0 < n_keys) ? expf(sc[t0] - M) : 0.f;
      sc[t0] = pr;                                                  // plain probability: alignment rows, normaliser
      scv[t0] = pr * __builtin_bit_cast(float, vsb[g] << 23);       // probability x the key's V scale: the P.V operand
    }
    ls += pr;
    u32x4_t v0[4], v1[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) kv8_widen(vraw[g][dt], 1.0f, v0[dt], v1[dt]);
#pragma unroll
    for (int j = 0; j < 2; ++j) {   // operand j of lane (kq, .): keys kq*16 + j*8 .. +7 of this 64-key group
      float pv[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int t = g64 * 64 + kq * 16 + j * 8 + e;
        pv[e] = (t < n_bound) ? scv[t] : 0.f;   // same wavefront wrote these: LDS operations of a wavefront stay in order
      }
      const u32x4_t pf = pack16<T>(pv);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) o[dt] = sk_mfma<T>(j == 0 ? v0[dt] : v1[dt], pf, o[dt]);
    }
  }
  ls = tw_wave_sum(ls);
  float* wl = red + NW;
  float* wo = red + 2 * NW;
  if (lane == 0) wl[wave] = ls;
  if (fr == 0) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r) wo[wave * 64 + dt * 16 + kq * 4 + r] = o[dt][r];
  }
  __syncthreads();
  float L = 0.f;
#pragma unroll
  for (int w = 0; w < NW; ++w) L += wl[w];
  const float inv = 1.0f / L;
  if (tid < 64) {
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) v += wo[w * 64 + tid];
    out_base[tw_xt_index<T>(out_j, out_k0 + tid)] = (T)(v * inv);
  }
  return inv;
}

// q [B, H*64] row-major; kc / vc per (stream, head): `rows` (multiple of 64) keys of K fragment-major / V^T fragment-major
// NW wavefronts of 64 keys each: 1 / 2 wavefronts while the sequence is shorter than 64 / 128 positions (the host picks the
// 64-key bucket per step): no idle wavefronts to launch and to meet at the barriers of the cross-wavefront reductions
template <typename T, bool SINGLE, int NW>
__global__ __launch_bounds__(NW * 64) void dec_self_attn_kernel(const T* __restrict__ q, const T* __restrict__ kc,
                                                                 const T* __restrict__ vc, int rows, int H, int key_bound,
                                                                 T* __restrict__ out, const DecState* __restrict__ stt, int rows_streams) {
  // argument order: what the K / V^T / q request addresses need comes first (kernarg preload, see skinny_mfma_kernel)
  __shared__ float sc[512];
  __shared__ float red[2 * 4 + 4 * 64];
  asm volatile("" ::"s"(q), "s"(kc), "s"(vc), "s"(rows), "s"(H), "s"(key_bound));
  const int h = blockIdx.x, b = blockIdx.y;
  // rows mode (prefill): row b is a position of stream b % rs - its K / V^T live in that stream's cache (the addresses depend on
  // kernel arguments only, as before) and it sees the keys up to ITS position (causal inside the launch)
  const int srow = rows_streams > 0 ? b % rows_streams : b;
  const int n_keys = stt->pos + (rows_streams > 0 ? b / rows_streams : 0) + 1;
  const long long base = ((long long)srow * H + h) * rows * 64;
  // the host guarantees pos < key_bound (a multiple of 64, <= rows): the requests do not wait for `pos`
  attn_mfma_block<T, NW, SINGLE>(q + ((long long)b * H + h) * 64, kc + base, vc + base, n_keys, key_bound, sc, red,
                                out + (long long)(b >> 4) * 16 * H * 64, b & 15, h * 64);  // fragment-major, groups of 16 streams
}

// The same for a ragged step (tw_common.h: tw_row_pos): stream b sees the keys [0, q] of its ROW position q <= pos < key_bound, so the
// requests cover them; the keys between q and the bucket's end are masked like the ones behind pos in the kernel above, and the
// result does not depend on the bucket (attn_mfma_block: masked keys contribute exact zeros).  The table pointer stands behind the
// leading arguments, which are the plain kernel's.
template <typename T, bool SINGLE, int NW>
__global__ __launch_bounds__(NW * 64) void dec_self_attn_ragged_kernel(const T* __restrict__ q, const T* __restrict__ kc,
                                                                        const T* __restrict__ vc, int rows, int H, int key_bound,
                                                                        T* __restrict__ out, const DecState* __restrict__ stt,
                                                                        const int* __restrict__ n_pad) {
  __shared__ float sc[512];
  __shared__ float red[2 * 4 + 4 * 64];
  asm volatile("" ::"s"(q), "s"(kc), "s"(vc), "s"(rows), "s"(H), "s"(key_bound));
  const int h = blockIdx.x, b = blockIdx.y;
  const int n_keys = tw_row_pos(stt->pos, n_pad[b]) + 1;
  const long long base = ((long long)b * H + h) * rows * 64;
  attn_mfma_block<T, NW, SINGLE>(q + ((long long)b * H + h) * 64, kc + base, vc + base, n_keys, key_bound, sc, red,
                                out + (long long)(b >> 4) * 16 * H * 64, b & 15, h * 64);
}

template <typename T, bool SINGLE, bool FQ>
__global__ __launch_bounds__(512) void dec_cross_attn_kernel(const T* __restrict__ ck, const T* __restrict__ cv, int H, int Tp,
                                                              int Tlen, int rows_streams, const T* __restrict__ q, T* __restrict__ out,
                                                              const int* __restrict__ align_slot, float* __restrict__ align,
                                                              int Ha, int P, const DecState* __restrict__ stt, FusedQ fq) {
  // (rows_streams sits among the LEADING arguments since round 5: the K / V^T request addresses depend on it - which stream's arena -
  //  and an argument behind the FusedQ block is not delivered with the wave: the requests waited for a scalar load)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* sc = reinterpret_cast<float*>(smem);  // [Tp] scores -> unnormalised probabilities
  __shared__ float red[2 * 8 + 8 * 64];
  __shared__ __attribute__((aligned(16))) T qst[FQ ? 8 * 64 : 8];
  asm volatile("" ::"s"(ck), "s"(cv), "s"(H), "s"(Tp), "s"(Tlen), "s"(rows_streams));
  const int h = blockIdx.x, b = blockIdx.y;
  const int srow = rows_streams > 0 ? b % rows_streams : b;   // rows mode (prefill): the stream whose encoder K / V this row attends to
  const long long base = ((long long)srow * H + h) * Tp * 64;
  const float inv = attn_mfma_block<T, 8, SINGLE, FQ>(q + ((long long)b * H + h) * 64, ck + base, cv + base, Tlen, Tp, sc, red,
                                                      out + (long long)(b >> 4) * 16 * H * 64, b & 15, h * 64, fq, b, h, qst);
  const int slot = align_slot ? align_slot[h] : -1;
  if (slot >= 0) {  // A11 side output: softmax row of an alignment head
    __syncthreads();
    const int prow = stt->pos + (rows_streams > 0 ? b / rows_streams : 0);
    float* row = align + (((long long)srow * Ha + slot) * P + prow) * Tlen;
    for (int t = threadIdx.x; t < Tlen; t += 512) row[t] = sc[t] * inv;
  }
}

// Rows flavour of dec_cross_attn_kernel (rows mode with more than one position per stream: prefill_core, verify_round,
// tw_score_tokens).  One workgroup per (stream, head, group of up to 16 of the stream's positions): column j of the MFMA B operands
// is position g * 16 + j of the stream, i.e. row srow + (g * 16 + j) * rows_streams of the launch, so ONE pass over the head's K / V^T
// serves 16 queries with the matrix instructions the single-query kernel spends on one (there every column carries the same query).
// Every column is computed by that kernel's expression tree - a column of an MFMA depends on its own B column only; column max
// over the kq lane groups, then over the wavefronts in index order; expf(sc - M), one key per lane; tw_wave_sum, then the wavefronts
// in index order; probabilities rounded by pack16 before P.V; partial context vectors added over the wavefronts in index order,
// then x 1/L - so a row's bits are the one-position step's.  Columns behind the group's last position repeat that position and are
// not written.
// LDS (dynamic): scores float[16][Tp + 4] | partial context vectors float[8][16][68] | column max float[8][16] | normaliser
// float[8][16] | query rows T[16][64]: 71 KiB at Tp = 512 (two workgroups per CU), 135 KiB at Tp = 1536 (one).
template <typename T, bool SINGLE, bool FQ>
__global__ __launch_bounds__(512) void dec_cross_attn_rows_kernel(const T* __restrict__ ck, const T* __restrict__ cv, int H, int Tp,
                                                                   int Tlen, int rows_streams, int n_pos, const T* __restrict__ q,
                                                                   T* __restrict__ out, const int* __restrict__ align_slot,
                                                                   float* __restrict__ align, int Ha, int P,
                                                                   const DecState* __restrict__ stt, FusedQ fq) {
  constexpr int NW = 8, WS = 68;
  constexpr int E = ElemTraits<T>::kPer16B;
  constexpr int DS = 64 / (4 * E);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int S = Tp + 4;
  float* sc = reinterpret_cast<float*>(smem);   // [16][S] scores -> unnormalised probabilities
  float* wo = sc + 16 * S;                      // [NW][16][WS]
  float* redm = wo + NW * 16 * WS;              // [NW][16]
  float* wl = redm + NW * 16;                   // [NW][16]
  T* qst = reinterpret_cast<T*>(wl + NW * 16);  // [16][64]
  const int h = blockIdx.x, srow = blockIdx.y, p0 = blockIdx.z * 16;
  const int nc = min(16, n_pos - p0);           // columns in use
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, kq = lane >> 4;
  const long long base = ((long long)srow * H + h) * Tp * 64;
  const T* kf = ck + base;
  const T* vtf = cv + base;
  const int n_keys = Tlen, n_bound = Tp;
  const int n_chunks = SINGLE ? 1 : (n_bound + NW * 64 - 1) / (NW * 64);
  const int last64 = n_bound / 64 - 1;
  u32x4_t qf[DS], kfr[4 * DS], vfr[4 * DS];
  auto load_k = [&](int g64) {
    const T* p = kf + ((long long)min(g64, last64) * (4 * DS) * 64 + lane) * E;
#pragma unroll
    for (int i = 0; i < 4 * DS; ++i) kfr[i] = *reinterpret_cast<const u32x4_t*>(p + (long long)i * 64 * E);
  };
  auto load_v = [&](int g64) {
    const T* p = vtf + ((long long)min(g64, last64) * (4 * DS) * 64 + lane) * E;
#pragma unroll
    for (int i = 0; i < 4 * DS; ++i) vfr[i] = *reinterpret_cast<const u32x4_t*>(p + (long long)i * 64 * E);
  };
  auto row_of = [&](int j) { return srow + (p0 + min(j, nc - 1)) * rows_streams; };   // launch row of column j
  load_k(wave);
  if constexpr (FQ) {
    // the group's query rows, once per workgroup: wavefront w builds the rows of columns w and w + 8
    QRaw<T> qr[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) fq_request<T>(qr[i], fq, row_of(wave + 8 * i), h, lane);
    if (SINGLE) load_v(wave);
#pragma unroll
    for (int i = 0; i < 2; ++i) fq_finish<T>(qr[i], fq, lane, qst + (wave + 8 * i) * 64);
    __syncthreads();
#pragma unroll
    for (int ds = 0; ds < DS; ++ds) qf[ds] = *reinterpret_cast<const u32x4_t*>(qst + fr * 64 + ds * 4 * E + kq * E);
  } else {
    const T* qrow = q + ((long long)row_of(fr) * H + h) * 64;
#pragma unroll
    for (int ds = 0; ds < DS; ++ds) qf[ds] = *reinterpret_cast<const u32x4_t*>(qrow + ds * 4 * E + kq * E);
    if (SINGLE) load_v(wave);
  }

  // ---- scores: lane (fr, kq) holds keys kq * 4 + r of the tile for column fr ----
  float m = -1.0e30f;
  for (int c = 0; c < n_chunks; ++c) {
    const int g64 = c * NW + wave;
    if (c > 0) load_k(g64);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      f32x4_t acc = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ds = 0; ds < DS; ++ds) acc = sk_mfma<T>(kfr[a * DS + ds], qf[ds], acc);
      f32x4_t sv4;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int t = g64 * 64 + a * 16 + kq * 4 + r;
        const float sv = (t < n_keys) ? acc[r] : -1.0e30f;
        m = fmaxf(m, sv);
        sv4[r] = sv;
      }
      if (g64 * 64 < n_bound) *reinterpret_cast<f32x4_t*>(sc + fr * S + g64 * 64 + a * 16 + kq * 4) = sv4;
    }
  }
  m = tw_xor32_max(tw_xor16_max(m));
  if (kq == 0) redm[wave * 16 + fr] = m;
  __syncthreads();
  float Mc = redm[fr];   // lane's column
#pragma unroll
  for (int w = 1; w < NW; ++w) Mc = fmaxf(Mc, redm[w * 16 + fr]);

  // ---- probabilities of this wavefront's own keys, every column, and P.V ----
  f32x4_t o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float ls[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) ls[j] = 0.f;
  for (int c = 0; c < n_chunks; ++c) {
    const int g64 = c * NW + wave;
    if (!SINGLE) load_v(g64);
    const int t0 = g64 * 64 + lane;  // one key per lane
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float M = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, Mc), j));
      float pr = 0.f;
      if (t0 < n_bound) {
        pr = (t0 < n_keys) ? expf(sc[j * S + t0] - M) : 0.f;
        sc[j * S + t0] = pr;
      }
      ls[j] += pr;
    }
#pragma unroll
    for (int ks = 0; ks < DS; ++ks) {
      float pv[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int t = g64 * 64 + ks * 4 * E + kq * E + e;
        pv[e] = (t < n_bound) ? sc[fr * S + t] : 0.f;  // same wavefront wrote these: LDS operations of a wavefront stay in order
      }
      const u32x4_t pf = pack16<T>(pv);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) o[dt] = sk_mfma<T>(vfr[ks * 4 + dt], pf, o[dt]);
    }
  }
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    // lane 0's sum, as in the single-query kernel: tw_wave_sum adds the four quads of a row in another order in odd quads
    // than in even ones, so the lanes of a wavefront do not all hold the same bits
    const float l = tw_wave_sum(ls[j]);
    if (lane == 0) wl[wave * 16 + j] = l;
  }
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) *reinterpret_cast<f32x4_t*>(wo + (wave * 16 + fr) * WS + dt * 16 + kq * 4) = o[dt];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 2; ++i) {   // 16 columns x 64 dims over 512 threads
    const int j = (tid >> 6) + 8 * i, k = tid & 63;
    float L = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) L += wl[w * 16 + j];
    const float inv = 1.0f / L;
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) v += wo[(w * 16 + j) * WS + k];
    if (j < nc) {
      const int b = srow + (p0 + j) * rows_streams;
      out[(long long)(b >> 4) * 16 * H * 64 + tw_xt_index<T>(b & 15, h * 64 + k)] = (T)(v * inv);
    }
  }
  const int slot = align_slot ? align_slot[h] : -1;
  if (slot >= 0) {  // A11 side output: every column writes the softmax row of its own (stream, position)
    const int pos = stt->pos;
    for (int j = 0; j < nc; ++j) {
      float L = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) L += wl[w * 16 + j];
      const float inv = 1.0f / L;
      float* row = align + (((long long)srow * Ha + slot) * P + pos + p0 + j) * Tlen;
      for (int t = tid; t < Tlen; t += 512) row[t] = sc[j * S + t] * inv;
    }
  }
}

template <int G, bool FQ>
__global__ __launch_bounds__(512) void dec_cross_attn_kv8_kernel(const unsigned char* __restrict__ ck, const unsigned char* __restrict__ cv,
                                                                  const unsigned char* __restrict__ ksc,
                                                                  const unsigned char* __restrict__ vsc, int H, int Tp, int Tlen,
                                                                  int rows_streams, const bf16_t* __restrict__ q, bf16_t* __restrict__ out,
                                                                  const int* __restrict__ align_slot, float* __restrict__ align,
                                                                  int Ha, int P, const DecState* __restrict__ stt, FusedQ fq) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* sc = reinterpret_cast<float*>(smem);  // [Tp] scores -> unnormalised probabilities
  float* scv = sc + Tp;                        // [Tp] probabilities x V scale
  __shared__ float red[2 * 8 + 8 * 64];
  __shared__ __attribute__((aligned(16))) bf16_t qst[FQ ? 8 * 64 : 8];
  asm volatile("" ::"s"(ck), "s"(cv), "s"(ksc), "s"(vsc), "s"(H), "s"(Tp), "s"(Tlen), "s"(rows_streams));
  const int h = blockIdx.x, b = blockIdx.y;
  const int srow = rows_streams > 0 ? b % rows_streams : b;   // rows mode (prefill), as in dec_cross_attn_kernel
  const long long hb = ((long long)srow * H + h) * Tp;
  const float inv = attn_mfma_block_kv8<8, G, FQ>(q + ((long long)b * H + h) * 64, ck + hb * 64, cv + hb * 64, ksc + hb, vsc + hb,
                                                  Tlen, Tp, sc, scv, red, out + (long long)(b >> 4) * 16 * H * 64, b & 15, h * 64,
                                                  fq, b, h, qst);
  const int slot = align_slot ? align_slot[h] : -1;
  if (slot >= 0) {  // A11 side output: softmax row of an alignment head
    __syncthreads();
    const int prow = stt->pos + (rows_streams > 0 ? b / rows_streams : 0);
    float* row = align + (((long long)srow * Ha + slot) * P + prow) * Tlen;
    for (int t = threadIdx.x; t < Tlen; t += 512) row[t] = sc[t] * inv;
  }
}

// ---------------------------------------------------------------------------------------------
// sampler: logits processors + argmax
// ---------------------------------------------------------------------------------------------
struct MaxIdx { float v; int i; };
__device__ __forceinline__ MaxIdx better(MaxIdx a, MaxIdx b) {
  // larger value wins; on ties the lower index (torch.argmax returns the first maximal index)
  if (b.v > a.v || (b.v == a.v && b.i < a.i)) return b;
  return a;
}
__device__ __forceinline__ MaxIdx wave_best(MaxIdx x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    MaxIdx y;
    y.v = __shfl_xor(x.v, o, 64);
    y.i = __shfl_xor(x.i, o, 64);
    x = better(x, y);
  }
  return x;
}

// static part of the mask (SuppressTokensLogitsProcessor list, HF:generation/logits_process.py:1869-1906) as a bitmap
__global__ void suppress_bitmap_kernel(const int* __restrict__ list, int n, unsigned* __restrict__ bits, int V) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const int v = list[i];
    if (v >= 0 && v < V) atomicOr(&bits[v >> 5], 1u << (v & 31));
  }
}

// Sampling = Whisper's logits processors + first-index argmax (HF:generation/logits_process.py:1816-2047,
// HF:generation/utils.py:2925), in two launches:
//  * sampler_part_kernel: SAMPLER_NS workgroups per stream, each owning a slice of the vocabulary (one CU cannot evaluate
//    the mask and the comparisons for 51866 logits in less than ~20 us - the work is VALU-, not memory-bound).  The slice
//    is requested before anything else (addresses depend on kernel arguments only) and kept in registers for both
//    passes.  Output per slice: best text token, best timestamp token, sum of exp(x - slice max) over timestamp tokens.
//  * sampler_finish_kernel: ONE workgroup, wavefront b merges the slices of stream b (log-sum-exp merge), applies the
//    "timestamp mass beats every text token" rule, appends the token, and thread 0 advances the position afterwards.
// 32 slices of <= 4 x 512 logits per stream (one stream would otherwise put the whole vocabulary on 8 CUs: 10 us of a turbo step's
// 220; at 16 streams 512 short workgroups also beat 128 long ones, see launch_sampler)
// The temperature sampler, the filtered draw and the scoring pass (below) are other compositions of the same pieces, each stated once:
// the mask of one id (sampler_masked_at), the slicing and the slice's requests (vocab_slice, slice_load), the timestamp sum of a slice
// (slice_ts_sum, block4_sum), the merge of a row's slices with the mass decision (merge_slices) and the append of the step's tokens
// (finish_step).
constexpr int SAMPLER_NS_MAX = 32;

struct SamplerMask {  // dynamic part of the mask: uniform scalars derived from the decoding state
  int b_lo, b_hi, c_lo, c_hi, d_hi, e_lo, ts_begin;
  bool mask_eos, first, in_prompt, fin;
};

// b = row of the launch: a stream at the device position (ordinary step), or - rows mode, SamplerArgs::rows_streams > 0 - stream
// b % rs at the host-known position row_pos0 + b / rs, sampled with the state the loop would have had there (draft-and-verify)
__device__ __forceinline__ SamplerMask sampler_mask(const SamplerArgs& a, int b) {
  SamplerMask k;
  const int V = a.V;
  const bool rows = a.rows_streams > 0;
  const int stream = rows ? b % a.rows_streams : b;
  const int pos = rows ? a.row_pos0 + b / a.rows_streams : a.stt->pos;
  const int n_prompt = a.stt->n_prompt;
  const int cur_len = pos + 1;
  const int* seq = a.seq + (long long)stream * a.seq_ld;
  k.in_prompt = cur_len < n_prompt;     // still consuming the forced prompt
  k.fin = rows ? false : a.finished[b] != 0;           // HF: finished rows keep receiving pad_token_id
  k.first = (cur_len == n_prompt);
  const int n_new = cur_len - n_prompt;
  k.ts_begin = a.timestamps ? a.no_ts_id + 1 : V;
  bool last_ts = false, penult_ts = true;
  int lastts_tok = -1;
  if (a.timestamps && !k.in_prompt) {
    last_ts = (n_new >= 1) && (seq[cur_len - 1] >= k.ts_begin);
    penult_ts = (n_new < 2) || (seq[cur_len - 2] >= k.ts_begin);
    lastts_tok = rows ? a.row_lastts[b] : a.last_ts[b];
  }
  k.b_lo = 0; k.b_hi = 0;  // range masked by the pairing rule
  if (last_ts) {
    if (penult_ts) { k.b_lo = k.ts_begin; k.b_hi = V; } else { k.b_lo = 0; k.b_hi = a.eos; }
  }
  k.c_lo = 0; k.c_hi = 0;  // non-decreasing timestamps
  if (a.timestamps && lastts_tok >= 0) {
    k.c_lo = k.ts_begin;
    k.c_hi = (last_ts && !penult_ts) ? lastts_tok : lastts_tok + 1;
  }
  k.d_hi = 0; k.e_lo = V;  // first sampled token must be a timestamp <= max_initial
  if (a.timestamps && k.first) {
    k.d_hi = k.ts_begin;
    if (a.max_initial_ts >= 0) k.e_lo = k.ts_begin + a.max_initial_ts + 1;
  }
  k.mask_eos = n_new < a.min_new;
  return k;
}

// Whisper's logits processors for one id (HF:generation/logits_process.py:1816-2047): is v masked?  word = suppress_bits[v >> 5]
__device__ __forceinline__ bool sampler_masked_at(const SamplerArgs& a, const SamplerMask& k, int v, unsigned word) {
  bool masked = ((word >> (v & 31)) & 1u) != 0;
  if (k.mask_eos && v == a.eos) masked = true;
  if (a.timestamps && v == a.no_ts_id) masked = true;
  if (v >= k.b_lo && v < k.b_hi) masked = true;
  if (v >= k.c_lo && v < k.c_hi) masked = true;
  if (v < k.d_hi) masked = true;
  if (v >= k.e_lo) masked = true;
  if (k.first)
    for (int i = 0; i < a.n_begin_suppress; ++i) masked |= (v == a.begin_suppress[i]);
  return masked;
}

// The slice [v0, v1) of the vocabulary that workgroup `part` of NS owns: even length ceil(V / 2 NS) * 2.  vec_ok: thread t holds the
// pairs (v, v + 1), v = v0 + (it * 256 + t) * 2, it < IT, in registers (vector path); otherwise the slice is walked id by id (scalar path)
struct VocabSlice { int v0, v1; bool vec_ok; };
template <int NS, int IT>
__device__ __forceinline__ VocabSlice vocab_slice(int V, int part) {
  const int chunk = ((V + 2 * NS - 1) / (2 * NS)) * 2;
  const int v0 = part * chunk;
  return VocabSlice{v0, min(v0 + chunk, V), (chunk <= IT * 512) && ((V & 1) == 0) && V >= 2};
}
// the vector path's requests: clamped into the row, so they can be issued whatever vec_ok says; the pair (v, v + 1) shares one bitmap word
template <int IT>
__device__ __forceinline__ void slice_load(const SamplerArgs& a, const float* lg, const VocabSlice& sl, int tid, float (&s0)[IT],
                                           float (&s1)[IT], unsigned (&wb)[IT]) {
  const int v_last = max(a.V - 2, 0) & ~1;
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int v = min(sl.v0 + (it * 256 + tid) * 2, v_last);
    const float2 x2 = *reinterpret_cast<const float2*>(lg + v);
    s0[it] = x2.x;
    s1[it] = x2.y;
    wb[it] = a.suppress_bits[v >> 5];
  }
}

// the block's sum of one value per thread (256 threads): wavefront reduction, then the four wavefronts in index order through LDS
__device__ __forceinline__ float block4_sum(float x, float* red, int lane, int wave) {
  x = wave_sum(x);
  if (lane == 0) red[wave] = x;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// sum of exp(x - m) over the slice's unmasked timestamp ids, m = the slice's best timestamp logit; s0 / s1: the slice AFTER the mask
// (-inf: masked or outside).  A thread adds its registers in `it` order.
template <int IT>
__device__ __forceinline__ float slice_ts_sum(const SamplerArgs& a, const SamplerMask& k, const VocabSlice& sl, const float* lg, int tid,
                                              const float (&s0)[IT], const float (&s1)[IT], float m, float* red) {
  float sum = 0.f;
  if (a.timestamps && m > -INFINITY) {
    if (sl.vec_ok) {
#pragma unroll
      for (int it = 0; it < IT; ++it) {
        const int v = sl.v0 + (it * 256 + tid) * 2;
        if (v < sl.v1) {
          if (v >= k.ts_begin) sum += expf(s0[it] - m);
          if (v + 1 >= k.ts_begin) sum += expf(s1[it] - m);
        }
      }
    } else {
      for (int v = max(sl.v0, k.ts_begin) + tid; v < sl.v1; v += 256)
        sum += sampler_masked_at(a, k, v, a.suppress_bits[v >> 5]) ? 0.f : expf(lg[v] - m);
    }
  }
  return block4_sum(sum, red, tid & 63, tid >> 6);
}

template <int SAMPLER_NS, int SAMPLER_IT>
__global__ __launch_bounds__(256) void sampler_part_kernel(SamplerArgs a) {
  __shared__ MaxIdx red_text[4], red_ts[4];
  __shared__ float red_sum[4];
  const int part = blockIdx.x, b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* lg = a.logits + (long long)b * a.V;
  const VocabSlice sl = vocab_slice<SAMPLER_NS, SAMPLER_IT>(a.V, part);
  const int v0 = sl.v0, v1 = sl.v1;
  float s0[SAMPLER_IT], s1[SAMPLER_IT];
  unsigned wb[SAMPLER_IT];
  slice_load(a, lg, sl, tid, s0, s1, wb);   // in front of everything else: the addresses depend on kernel arguments only
  __builtin_amdgcn_sched_barrier(0);
  const SamplerMask k = sampler_mask(a, b);
  // ---- pass 1: best text token, best timestamp token of the slice ----
  MaxIdx bt{-INFINITY, 0x7fffffff}, bs{-INFINITY, 0x7fffffff};
  if (sl.vec_ok) {
#pragma unroll
    for (int it = 0; it < SAMPLER_IT; ++it) {
      const int v = v0 + (it * 256 + tid) * 2;
      const bool in = v < v1;
      const int vc = in ? v : 0;
      s0[it] = (in && !sampler_masked_at(a, k, vc, wb[it])) ? s0[it] : -INFINITY;
      s1[it] = (in && !sampler_masked_at(a, k, vc + 1, wb[it])) ? s1[it] : -INFINITY;
      if (in) {
        MaxIdx c0{s0[it], v}, c1{s1[it], v + 1};
        if (v < k.ts_begin) bt = better(bt, c0); else bs = better(bs, c0);
        if (v + 1 < k.ts_begin) bt = better(bt, c1); else bs = better(bs, c1);
      }
    }
  } else {
    for (int v = v0 + tid; v < v1; v += 256) {
      MaxIdx c{sampler_masked_at(a, k, v, a.suppress_bits[v >> 5]) ? -INFINITY : lg[v], v};
      if (v < k.ts_begin) bt = better(bt, c); else bs = better(bs, c);
    }
  }
  bt = wave_best(bt);
  bs = wave_best(bs);
  if (lane == 0) { red_text[wave] = bt; red_ts[wave] = bs; }
  __syncthreads();
  bt = red_text[0];
  bs = red_ts[0];
  for (int w = 1; w < 4; ++w) { bt = better(bt, red_text[w]); bs = better(bs, red_ts[w]); }
  // ---- pass 2: the slice's timestamp sum ----
  const float sum = slice_ts_sum(a, k, sl, lg, tid, s0, s1, bs.v, red_sum);
  if (tid == 0) {
    SamplerPartial o;
    o.bt_v = bt.v; o.bt_i = bt.i; o.bs_v = bs.v; o.bs_i = bs.i;
    o.sum = sum;
    a.partials[b * SAMPLER_NS_MAX + part] = o;
  }
}

// the next step's input row of stream b (A6: HF:models/whisper/modeling_whisper.py:733-771), by one wavefront: 16-byte vectors of the
// token row and the positional row, added in float32, rounded once, stored where tw_xt_index puts elements 8v .. 8v+7 (E per vector)
template <typename T>
__device__ __forceinline__ void embed_row(const SamplerArgs& a, int b, int id, int p, int lane) {
  constexpr int E = ElemTraits<T>::kPer16B;
  const T* tok = reinterpret_cast<const T*>(a.tok_emb) + (long long)id * a.d;
  const T* pos = reinterpret_cast<const T*>(a.pos_emb) + (long long)p * a.d;
  T* x = reinterpret_cast<T*>(a.x_next) + (long long)(b >> 4) * 16 * a.d;
  for (int v = lane; v * E < a.d; v += 64) {
    const u32x4_t tv = *reinterpret_cast<const u32x4_t*>(tok + v * E), pv = *reinterpret_cast<const u32x4_t*>(pos + v * E);
    T o[E];
    const T* tp = reinterpret_cast<const T*>(&tv);
    const T* pp = reinterpret_cast<const T*>(&pv);
#pragma unroll
    for (int e = 0; e < E; ++e) o[e] = (T)((float)tp[e] + (float)pp[e]);
    *reinterpret_cast<u32x4_t*>(x + tw_xt_index<T>(b & 15, v * E)) = *reinterpret_cast<const u32x4_t*>(o);
  }
}

// Merge of the vocabulary slices of row b by one wavefront, in every lane: the row's best text and timestamp token over the unmasked
// logits and the "timestamp mass beats every text token" decision (log-sum-exp merge of the slices' timestamp sums).  P: SamplerPartial,
// SamplePartial or BeamPartial, which begin with the same five fields (only those are read).
struct SliceMerge { MaxIdx bt, bs; bool force_ts; };
template <typename P>
__device__ __forceinline__ SliceMerge merge_slices(const SamplerArgs& a, const P* parts, int b, int lane) {
  const P p = parts[b * SAMPLER_NS_MAX + min(lane, a.n_slices - 1)];
  const bool on = lane < a.n_slices;
  SliceMerge m{{on ? p.bt_v : -INFINITY, on ? p.bt_i : 0x7fffffff}, {on ? p.bs_v : -INFINITY, on ? p.bs_i : 0x7fffffff}, false};
  const float my_m = m.bs.v;
  m.bt = wave_best(m.bt);
  m.bs = wave_best(m.bs);
  const float part_sum = (on && my_m > -INFINITY) ? p.sum * expf(my_m - m.bs.v) : 0.f;
  const float tot = wave_sum(part_sum);
  if (a.timestamps && m.bs.v > -INFINITY) m.force_ts = (m.bs.v + logf(tot)) > m.bt.v;
  return m;
}

// the token HF's processors + argmax pick for row b, in every lane
__device__ __forceinline__ int sampler_merge(const SamplerArgs& a, int b, int lane) {
  const SliceMerge m = merge_slices(a, a.partials, b, lane);
  int choice = (m.force_ts || m.bs.v > m.bt.v) ? m.bs.i : m.bt.i;
  if (choice == 0x7fffffff) choice = 0;  // everything masked: torch.argmax of all -inf is 0
  return choice;
}

// The last launch of a step, whichever sampler ran: ONE workgroup, wavefront w takes streams w, w + 16, ...; choice_of(b, lane) yields
// the stream's sampled token in every lane.  Lane 0 appends (a prompt token while the prompt lasts, pad_id once finished), the wavefront
// writes the next step's input row, and thread 0 advances the position once every wavefront has used it.
template <typename ChoiceOf>
__device__ __forceinline__ void finish_step(const SamplerArgs& a, ChoiceOf choice_of) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int pos_now = a.stt->pos;
  for (int b = tid >> 6; b < a.B; b += 16) {
    int next_id = 0;
    const SamplerMask k = sampler_mask(a, b);
    const int choice = choice_of(b, lane);
    if (lane == 0) {
      const int cur_len = a.stt->pos + 1;
      int* seq = a.seq + (long long)b * a.seq_ld;
      if (k.in_prompt) {
        next_id = seq[cur_len];
        a.cur_ids[b] = next_id;
      } else if (k.fin) {
        seq[cur_len] = a.pad;
        a.cur_ids[b] = a.pad;
        next_id = a.pad;
      } else {
        seq[cur_len] = choice;
        a.cur_ids[b] = choice;
        next_id = choice;
        if (a.timestamps && choice >= k.ts_begin) a.last_ts[b] = choice;
        if (choice == a.eos) a.finished[b] = 1;
      }
    }
    if (a.x_next) {   // (kernel-uniform) the token just appended is the next step's input at position pos + 1
      const int id = __builtin_amdgcn_readfirstlane(next_id);   // lane 0's
      if (a.dtype == 1) embed_row<bf16_t>(a, b, id, pos_now + 1, lane);
      else if (a.dtype == 2) embed_row<f16_t>(a, b, id, pos_now + 1, lane);
      else embed_row<float>(a, b, id, pos_now + 1, lane);
    }
  }
  __syncthreads();
  if (tid == 0) a.stt->pos += 1;
}

__global__ __launch_bounds__(1024) void sampler_finish_kernel(SamplerArgs a) {
  finish_step(a, [&](int b, int lane) { return sampler_merge(a, b, lane); });
}

// Rows mode (draft-and-verify; SamplerArgs): every row's token, the first position at which a stream's token differs from the token the
// NEXT row was given, and - once the round is decided (a mismatch, or the round's last launch) - the state the ordinary loop would have
// after producing the token at p_acc + 1 itself: that token appended to every stream's history (seq, cur_ids, last_ts, finished), the
// device position = p_acc + 1.  Everything at positions > p_acc + 1 (self-attention K / V rows, alignment rows, stale given tokens) is
// overwritten by the steps that follow before anything reads it.  One workgroup; rows = streams x positions <= 64.
__global__ __launch_bounds__(1024) void sampler_rows_finish_kernel(SamplerArgs a) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int rs = a.rows_streams;
  for (int r = tid >> 6; r < a.B; r += 16) {
    const int stream = r % rs, p = a.row_pos0 + r / rs;
    const SamplerMask k = sampler_mask(a, r);
    int choice = sampler_merge(a, r, lane);
    if (lane == 0) {
      const int* seq = a.seq + (long long)stream * a.seq_ld;
      if (k.in_prompt) choice = seq[p + 1];          // the prompt is not sampled
      a.row_choice[r] = choice;
      if (p < a.row_last_pos && choice != seq[p + 1]) atomicMin(&a.verify_state[0], p);
    }
  }
  __syncthreads();
  __shared__ int p_acc_s;
  if (tid == 0) {
    const int fm = a.verify_state[0];     // (this workgroup's own atomics, behind the barrier)
    int p_acc = -1;
    if (fm != 0x7fffffff) p_acc = fm;
    else if (a.row_is_last) p_acc = a.row_last_pos;
    p_acc_s = p_acc;
  }
  __syncthreads();
  const int p_acc = p_acc_s;
  if (p_acc < 0) {                        // undecided: the next launch of the round continues behind this launch's positions
    if (tid == 0) a.stt->pos += a.B / rs;
    return;
  }
  const int n_streams = rs;
  if (tid < n_streams) {
    const int b = tid;
    const int n_prompt = a.stt->n_prompt;
    const int ts_begin = a.timestamps ? a.no_ts_id + 1 : a.V;
    int* seq = a.seq + (long long)b * a.seq_ld;
    const int tok = a.row_choice[(p_acc - a.row_pos0) * rs + b];   // (a mismatch can only be found in THIS launch: earlier ones ended the round)
    int lt = -1;
    for (int i = n_prompt; i <= p_acc; ++i) if (a.timestamps && seq[i] >= ts_begin) lt = seq[i];
    if (p_acc + 1 >= n_prompt) {          // a sampled token (not a prompt token)
      if (a.timestamps && tok >= ts_begin) lt = tok;
      a.finished[b] = (tok == a.eos) ? 1 : 0;
    } else {
      a.finished[b] = 0;
    }
    seq[p_acc + 1] = tok;
    a.cur_ids[b] = tok;
    a.last_ts[b] = lt;
    a.verify_state[2 + b] = tok;
  }
  if (tid == 0) {
    a.verify_state[1] = p_acc + 1;
    a.stt->pos = p_acc + 1;
  }
}

// Temperature sampling (tw_generate_sample, api.hip; the draw is defined at SampleArgs, tw_common.h): the greedy sampler's two launches
// with Gumbel noise on the scaled logits.
//  * sample_part_kernel: the slicing, the register-resident slice and the vector / scalar paths of sampler_part_kernel.  Per slice: the
//    greedy partials of the UNSCALED logits (best text, best timestamp, sum exp(x - slice max) over timestamps: what the mass rule is
//    decided on) and the best perturbed text and timestamp (value, id).  One Philox4x32-10 block serves the ids 4j .. 4j + 3, so a
//    thread's pair (v, v + 1), v even, costs one block; the block and the two logf per logit are VALU work behind the logit requests.
//  * sample_finish_kernel: merge_slices on the unscaled partials (a mass decision equals the greedy one bit for bit on equal logits);
//    mass rule fired: the best perturbed timestamp, else the better of the two perturbed maxima (lower id on a tie); then finish_step.
struct Philox4 { unsigned w[4]; };
__device__ __forceinline__ Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}
__device__ __forceinline__ float gumbel_of(unsigned w) {
  const float u = (float)((w >> 9) * 2u + 1u) * 5.9604644775390625e-08f;   // 2^-24; the integer is odd and below 2^24: exact
  return -logf(-logf(u));
}

template <int SAMPLER_NS, int SAMPLER_IT>
__global__ __launch_bounds__(256) void sample_part_kernel(SampleArgs sa) {
  __shared__ MaxIdx red[4][4];
  __shared__ float red_sum[4];
  const SamplerArgs& a = sa.s;
  const int part = blockIdx.x, b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* lg = a.logits + (long long)b * a.V;
  const VocabSlice sl = vocab_slice<SAMPLER_NS, SAMPLER_IT>(a.V, part);
  const int v0 = sl.v0, v1 = sl.v1;
  float s0[SAMPLER_IT], s1[SAMPLER_IT];
  unsigned wb[SAMPLER_IT];
  slice_load(a, lg, sl, tid, s0, s1, wb);   // in front of everything else, as in sampler_part_kernel
  __builtin_amdgcn_sched_barrier(0);
  const SamplerMask k = sampler_mask(a, b);
  const unsigned p = (unsigned)a.stt->pos;
  const bool noisy = sa.noisy[b] != 0;
  const float inv_t = sa.inv_t[b];
  const unsigned k0 = sa.key[2 * b], k1 = sa.key[2 * b + 1], o0 = sa.off[2 * b], o1 = sa.off[2 * b + 1];
  // x: a logit after the mask (-inf: masked, stays -inf); w: its Philox word
  auto perturbed = [&](float x, unsigned w) -> float { return noisy ? __fadd_rn(__fmul_rn(x, inv_t), gumbel_of(w)) : x; };
  // ---- pass 1: best text / timestamp of the slice, unscaled and perturbed ----
  MaxIdx bt{-INFINITY, 0x7fffffff}, bs{-INFINITY, 0x7fffffff}, pt{-INFINITY, 0x7fffffff}, ps{-INFINITY, 0x7fffffff};
  if (sl.vec_ok) {
#pragma unroll
    for (int it = 0; it < SAMPLER_IT; ++it) {
      const int v = v0 + (it * 256 + tid) * 2;
      const bool in = v < v1;
      const int vc = in ? v : 0;
      s0[it] = (in && !sampler_masked_at(a, k, vc, wb[it])) ? s0[it] : -INFINITY;
      s1[it] = (in && !sampler_masked_at(a, k, vc + 1, wb[it])) ? s1[it] : -INFINITY;
      if (in) {
        MaxIdx c0{s0[it], v}, c1{s1[it], v + 1};
        MaxIdx q0 = c0, q1 = c1;
        if (noisy) {   // (uniform) v is even: v and v + 1 are words v & 3 and (v & 3) + 1 of one block
          const Philox4 r = philox4x32_10((unsigned)v >> 2, p, o0, o1, k0, k1);
          const bool up = (v & 2) != 0;
          q0.v = perturbed(c0.v, up ? r.w[2] : r.w[0]);
          q1.v = perturbed(c1.v, up ? r.w[3] : r.w[1]);
        }
        if (v < k.ts_begin) { bt = better(bt, c0); pt = better(pt, q0); } else { bs = better(bs, c0); ps = better(ps, q0); }
        if (v + 1 < k.ts_begin) { bt = better(bt, c1); pt = better(pt, q1); } else { bs = better(bs, c1); ps = better(ps, q1); }
      }
    }
  } else {
    for (int v = v0 + tid; v < v1; v += 256) {
      MaxIdx c{sampler_masked_at(a, k, v, a.suppress_bits[v >> 5]) ? -INFINITY : lg[v], v};
      MaxIdx q = c;
      if (noisy) {
        const Philox4 r = philox4x32_10((unsigned)v >> 2, p, o0, o1, k0, k1);
        const unsigned lo = (v & 1) ? r.w[1] : r.w[0], hi = (v & 1) ? r.w[3] : r.w[2];
        q.v = perturbed(c.v, (v & 2) ? hi : lo);
      }
      if (v < k.ts_begin) { bt = better(bt, c); pt = better(pt, q); } else { bs = better(bs, c); ps = better(ps, q); }
    }
  }
  bt = wave_best(bt);
  bs = wave_best(bs);
  pt = wave_best(pt);
  ps = wave_best(ps);
  if (lane == 0) { red[0][wave] = bt; red[1][wave] = bs; red[2][wave] = pt; red[3][wave] = ps; }
  __syncthreads();
  bt = red[0][0]; bs = red[1][0]; pt = red[2][0]; ps = red[3][0];
  for (int w = 1; w < 4; ++w) { bt = better(bt, red[0][w]); bs = better(bs, red[1][w]); pt = better(pt, red[2][w]); ps = better(ps, red[3][w]); }
  // ---- pass 2: the slice's timestamp sum, on the unscaled logits ----
  const float sum = slice_ts_sum(a, k, sl, lg, tid, s0, s1, bs.v, red_sum);
  if (tid == 0) {
    SamplePartial o;
    o.bt_v = bt.v; o.bt_i = bt.i; o.bs_v = bs.v; o.bs_i = bs.i;
    o.sum = sum;
    o.pt_v = pt.v; o.pt_i = pt.i; o.ps_v = ps.v; o.ps_i = ps.i;
    o.pad_[0] = o.pad_[1] = o.pad_[2] = 0;
    sa.parts[b * SAMPLER_NS_MAX + part] = o;
  }
}

// the token of row b, in every lane: the mass decision on the unscaled partials, the token from the perturbed ones
__device__ __forceinline__ int sample_merge(const SampleArgs& sa, int b, int lane) {
  const SamplerArgs& a = sa.s;
  const SamplePartial p = sa.parts[b * SAMPLER_NS_MAX + min(lane, a.n_slices - 1)];
  const bool on = lane < a.n_slices;
  MaxIdx pt{on ? p.pt_v : -INFINITY, on ? p.pt_i : 0x7fffffff}, ps{on ? p.ps_v : -INFINITY, on ? p.ps_i : 0x7fffffff};
  pt = wave_best(pt);
  ps = wave_best(ps);
  int choice = merge_slices(a, sa.parts, b, lane).force_ts ? ps.i : better(pt, ps).i;   // (text ids lie below timestamp ids: a tie goes to the text token)
  if (choice == 0x7fffffff) choice = 0;  // everything masked
  return choice;
}

__global__ __launch_bounds__(1024) void sample_finish_kernel(SampleArgs sa) {
  finish_step(sa.s, [&](int b, int lane) { return sample_merge(sa, b, lane); });
}

// Scoring (tw_score_tokens, api.hip): log-softmax of the GIVEN next token of every row of a rows-mode launch, twice - over the raw
// logits, and over the logits after Whisper's processors for that row's history (what HF's _retrieve_avg_logprobs takes its
// log_softmax of).  Shaped like the sampler for the sampler's reason (exp over 51866 logits is VALU work no single CU does in time):
//  * score_part_kernel: SCORE_NS workgroups per row, each holding its vocabulary slice in registers; ONE read of the slice yields the
//    slice maximum and sum exp(x - maximum) of three sets - every logit, the unmasked text tokens, the unmasked timestamp tokens.
//  * score_finish_kernel: one workgroup, wavefront r merges the 32 slices of row r in double precision by a fixed butterfly, applies the
//    "timestamp mass beats every text token" rule (text drops out of the masked normaliser), and lane 0 stores both numbers.
// The slicing and the merge order are compile-time constants: a row's numbers do not depend on the other rows of its launch.
constexpr int SCORE_NS = 32;

// the block's value of three per-thread values: wavefront reduction, then the four wavefronts in a fixed order through LDS
template <bool MAX>
__device__ __forceinline__ void score_block3(float (&v)[3], float (*red)[4], int lane, int wave) {
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float w = MAX ? wave_max(v[j]) : wave_sum(v[j]);
    if (lane == 0) red[j][wave] = w;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 3; ++j)
    v[j] = MAX ? fmaxf(fmaxf(red[j][0], red[j][1]), fmaxf(red[j][2], red[j][3])) : ((red[j][0] + red[j][1]) + red[j][2]) + red[j][3];
  __syncthreads();
}

template <int SCORE_IT>
__global__ __launch_bounds__(256) void score_part_kernel(ScoreArgs sa) {
  __shared__ float red[3][4];
  const SamplerArgs& a = sa.s;
  const int part = blockIdx.x, b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* lg = a.logits + (long long)b * a.V;
  const VocabSlice sl = vocab_slice<SCORE_NS, SCORE_IT>(a.V, part);
  const int v0 = sl.v0, v1 = sl.v1;
  const bool vec_ok = sl.vec_ok;
  float s0[SCORE_IT], s1[SCORE_IT];
  unsigned wb[SCORE_IT];
  // Only where the slice is read from registers, and not pinned in front of the mask's scalar loads by a sched_barrier as in the two
  // sampler kernels: this pass runs once per call, not once per step, and its scalar path reads every logit twice whatever is requested
  // here - the requests it would never use are spared instead.
  if (vec_ok) slice_load(a, lg, sl, tid, s0, s1, wb);
  const SamplerMask k = sampler_mask(a, b);
  // ---- pass 1: the three maxima (0 raw, 1 unmasked text, 2 unmasked timestamps); cls = the set an element's exp goes to (-1 none) ----
  float m[3] = {-INFINITY, -INFINITY, -INFINITY};
  int cls0[SCORE_IT], cls1[SCORE_IT];
  auto classify = [&](int v, unsigned word) -> int { return sampler_masked_at(a, k, v, word) ? -1 : (v < k.ts_begin ? 1 : 2); };
  if (vec_ok) {
#pragma unroll
    for (int it = 0; it < SCORE_IT; ++it) {
      const int v = v0 + (it * 256 + tid) * 2;
      const bool in = v < v1;      // (v1 - v0 is even: the pair is inside or outside together)
      cls0[it] = cls1[it] = -2;    // outside the slice
      if (in) {
        cls0[it] = classify(v, wb[it]);
        cls1[it] = classify(v + 1, wb[it]);
        m[0] = fmaxf(m[0], fmaxf(s0[it], s1[it]));
        if (cls0[it] == 1) m[1] = fmaxf(m[1], s0[it]); else if (cls0[it] == 2) m[2] = fmaxf(m[2], s0[it]);
        if (cls1[it] == 1) m[1] = fmaxf(m[1], s1[it]); else if (cls1[it] == 2) m[2] = fmaxf(m[2], s1[it]);
      }
    }
  } else {
    for (int v = v0 + tid; v < v1; v += 256) {
      const float x = lg[v];
      const int cl = classify(v, a.suppress_bits[v >> 5]);
      m[0] = fmaxf(m[0], x);
      if (cl == 1) m[1] = fmaxf(m[1], x); else if (cl == 2) m[2] = fmaxf(m[2], x);
    }
  }
  score_block3<true>(m, red, lane, wave);
  // ---- pass 2: sum exp(x - maximum) of each set (an element of a set is finite and <= the set's maximum: no exp of inf - inf) ----
  float s[3] = {0.f, 0.f, 0.f};
  if (vec_ok) {
#pragma unroll
    for (int it = 0; it < SCORE_IT; ++it) {
      if (cls0[it] != -2) {
        s[0] += expf(s0[it] - m[0]);
        s[0] += expf(s1[it] - m[0]);
        if (cls0[it] == 1) s[1] += expf(s0[it] - m[1]); else if (cls0[it] == 2) s[2] += expf(s0[it] - m[2]);
        if (cls1[it] == 1) s[1] += expf(s1[it] - m[1]); else if (cls1[it] == 2) s[2] += expf(s1[it] - m[2]);
      }
    }
  } else {
    for (int v = v0 + tid; v < v1; v += 256) {
      const float x = lg[v];
      const int cl = classify(v, a.suppress_bits[v >> 5]);
      s[0] += expf(x - m[0]);
      if (cl == 1) s[1] += expf(x - m[1]); else if (cl == 2) s[2] += expf(x - m[2]);
    }
  }
  score_block3<false>(s, red, lane, wave);
  if (tid == 0) {
    ScorePartial o;
    o.raw_m = m[0]; o.raw_s = s[0]; o.tx_m = m[1]; o.tx_s = s[1]; o.ts_m = m[2]; o.ts_s = s[2]; o.pad_[0] = o.pad_[1] = 0.f;
    sa.parts[b * SCORE_NS + part] = o;
  }
}

__device__ __forceinline__ double score_wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double score_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// (maximum, sum exp(x - maximum)) of a set over the whole vocabulary from its 32 slices, in every lane; an empty set: (-inf, 0)
__device__ __forceinline__ void score_merge(float pm, float ps, bool on, double& M, double& S) {
  const double mi = on ? (double)pm : -INFINITY;
  M = score_wave_max(mi);
  S = score_wave_sum(mi > -INFINITY ? (double)ps * exp(mi - M) : 0.0);
}

__global__ __launch_bounds__(1024) void score_finish_kernel(ScoreArgs sa) {
  const SamplerArgs& a = sa.s;
  const int tid = threadIdx.x, lane = tid & 63;
  const int rs = a.rows_streams;
  for (int r = tid >> 6; r < a.B; r += 16) {
    const int stream = r % rs, p = a.row_pos0 + r / rs;
    const SamplerMask k = sampler_mask(a, r);
    const ScorePartial q = sa.parts[r * SCORE_NS + min(lane, SCORE_NS - 1)];
    const bool on = lane < SCORE_NS;
    double rM, rS, xM, xS, tM, tS;
    score_merge(q.raw_m, q.raw_s, on, rM, rS);
    score_merge(q.tx_m, q.tx_s, on, xM, xS);
    score_merge(q.ts_m, q.ts_s, on, tM, tS);
    if (lane == 0) {
      const float* lg = a.logits + (long long)r * a.V;
      const int t = a.seq[(long long)stream * a.seq_ld + p + 1];   // the given next token (host-checked: inside the vocabulary)
      const double z = (double)lg[t];
      const double lse_raw = rM + log(rS);
      // "if the probability mass of the timestamps is above every text token, sample a timestamp": log_softmax subtracts the same
      // constant on both sides (HF:generation/logits_process.py:2040-2047)
      const bool force_ts = a.timestamps && tM > -INFINITY && (tM + log(tS)) > xM;
      double lse_m = -INFINITY;
      if (force_ts) {
        lse_m = tM + log(tS);
      } else {
        const double M = fmax(xM, tM);
        if (M > -INFINITY) lse_m = M + log((xM > -INFINITY ? xS * exp(xM - M) : 0.0) + (tM > -INFINITY ? tS * exp(tM - M) : 0.0));
      }
      const bool t_masked = sampler_masked_at(a, k, t, a.suppress_bits[t >> 5]) || (force_ts && t < k.ts_begin);
      const long long o = (long long)stream * sa.out_ld + p + 1;
      sa.out_raw[o] = (float)(z - lse_raw);
      sa.out_masked[o] = t_masked ? -INFINITY : (float)(z - lse_m);
      if (sa.ns_id >= 0 && p == sa.ns_pos) sa.out_ns[stream] = (float)exp((double)lg[sa.ns_id] - lse_raw);
    }
  }
}

// Top-k / top-p filtered draw (tw_generate_sample_filtered, api.hip; the rule is stated at FilterArgs, tw_common.h): three launches.
//  * sample_part_kernel, as it is: its unscaled partials carry the mass decision; its perturbed partials are not read.
//  * sample_filter_kernel: ONE workgroup of 1024 threads per row, the row in registers (kFilterPerThread values per thread, as keys: the
//    order-preserving integer image of the float, -0 folded onto +0).  Every wavefront takes the mass decision from the partials
//    (merge_slices); the mask is sampler_masked_at plus "text out" when the rule fired.  tau: the largest key t with count(key >= t) >= k, bit
//    by bit from the top (32 rounds, one block count each).  The keys of x then give way to the keys of y = x * inv_t of the ids kept so
//    far (0: dropped).  Top-p: the smallest key c with sum of exp(y - m) over {key > c} below top_p * Z, by the same search (32 rounds,
//    one block sum each); a thread's sum runs over its registers in float in a fixed order, the block's over the threads in double in a
//    fixed tree, so it is monotone in c and H(0) is Z itself, bit for bit.  Last the perturbed arg-max over the kept ids (one Philox
//    block per four consecutive ids, computed only where one of them is kept) and one choice[b] store.
//    The slice, the trees and the searches are compile-time shapes: a row's token depends on its logits, its state and its row of the
//    per-row arrays alone.  Rows still in the prompt, finished rows and rows that sit the call out leave at once.
//  * sample_choice_finish_kernel: finish_step on choice[b].
__device__ __forceinline__ unsigned filter_key(float x) {
  const unsigned u = __float_as_uint(x == 0.f ? 0.f : x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float filter_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
constexpr unsigned kFilterNegInfKey = 0x007fffffu;   // filter_key(-inf): masked, or outside the vocabulary
// x, as a value the compiler knows nothing about: what is derived from it is computed where it is used, not once at the top of the
// kernel and kept in registers (or scratch) beside the row all the way down
__device__ __forceinline__ int filter_opaque(int x) {
  asm volatile("" : "+v"(x));
  return x;
}

// the block's sum of one value per wavefront (already reduced over the wavefront), wavefronts in index order; `red` alternates between
// two buffers from call to call, so one barrier per call is enough
template <typename T>
__device__ __forceinline__ T filter_block_sum(T w, T* red, int lane, int wave) {
  if (lane == 0) red[wave] = w;
  __syncthreads();
  T s = red[0];
#pragma unroll
  for (int i = 1; i < 16; ++i) s += red[i];
  return s;
}

__global__ __launch_bounds__(1024) void sample_filter_kernel(FilterArgs fa) {
  constexpr int PER = kFilterPerThread;
  __shared__ int red_n[2][16];
  __shared__ double red_s[2][16];
  __shared__ unsigned red_m[16];
  __shared__ MaxIdx red_b[16];
  const SampleArgs& sa = fa.sm;
  const SamplerArgs& a = sa.s;
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int V = a.V;
  const SamplerMask k = sampler_mask(a, b);
  if (k.in_prompt || k.fin) return;   // (uniform over the workgroup) the finish kernel does not read choice[b] of such a row
  const float* lg = a.logits + (long long)b * V;
  const bool force_ts = merge_slices(a, sa.parts, b, lane).force_ts;
  const bool noisy = sa.noisy[b] != 0;
  const float inv_t = sa.inv_t[b];
  const int top_k = noisy ? fa.top_k[b] : 0;
  const float top_p = noisy ? fa.top_p[b] : 1.f;
  // thread t, register 4 q + j  <-  id (q * 1024 + t) * 4 + j: four consecutive ids share a Philox block and a bitmap word.  Sixteen
  // requests in flight at a time (all 64 at once would need their addresses beside the row: more registers than a thread has)
  unsigned key[PER];
#pragma unroll
  for (int g = 0; g < PER / 16; ++g) {
    const int tg = filter_opaque(tid);
#pragma unroll
    for (int q = 4 * g; q < 4 * g + 4; ++q) {
      const int v0 = (q * 1024 + tg) * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) key[4 * q + j] = __float_as_uint(lg[min(v0 + j, V - 1)]);
    }
#pragma unroll
    for (int q = 4 * g; q < 4 * g + 4; ++q) {
      const int v0 = (q * 1024 + tg) * 4;
      const unsigned word = a.suppress_bits[min(v0, V - 1) >> 5];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int v = v0 + j;
        const bool out = v >= V || sampler_masked_at(a, k, min(v, V - 1), word) || (force_ts && v < k.ts_begin);
        key[4 * q + j] = out ? kFilterNegInfKey : filter_key(__uint_as_float(key[4 * q + j]));
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  int round = 0;
  // ---- top-k: tau = the k-th largest key (masked ids count as -inf: with k or fewer ids unmasked tau ends at or below -inf) ----
  unsigned tau = 0;
  if (top_k > 0) {
#pragma unroll 1
    for (int bit = 31; bit >= 0; --bit) {
      const unsigned t = tau | (1u << bit);
      int n = 0;
#pragma unroll
      for (int i = 0; i < PER; ++i) {
        n += key[i] >= t ? 1 : 0;
        if ((i & 15) == 15) __builtin_amdgcn_sched_barrier(0);
      }
      n = filter_block_sum<int>((int)wave_sum((float)n), red_n[round & 1], lane, wave);   // (counts up to 65536: exact in float32)
      ++round;
      if (n >= top_k) tau = t;
    }
  }
  // ---- the keys of y = x * inv_t over K; 0: not in K ----
  unsigned kmax = 0;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const unsigned kx = key[i], ky = filter_key(__fmul_rn(filter_unkey(kx), inv_t));
    key[i] = (kx >= tau && kx > kFilterNegInfKey) ? ky : 0u;
    kmax = max(kmax, key[i]);
    if ((i & 7) == 7) __builtin_amdgcn_sched_barrier(0);   // (eight at a time: the row itself fills half the register file)
  }
  // ---- top-p: the smallest key c with H(c) = sum of e over {key > c} < top_p * Z ----
  unsigned cut = 1;   // kept: key >= cut
  if (top_p < 1.f) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, o, 64));
    if (lane == 0) red_m[wave] = kmax;
    __syncthreads();
    kmax = red_m[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) kmax = max(kmax, red_m[i]);
    if (kmax != 0) {   // (uniform) something is kept
      const float m = filter_unkey(kmax);
      // H(t - 1): a thread's registers in index order in float, the wavefront's butterfly and the block's chain in double
      // (y and e are computed again in every round: kept, either would take as many registers again as the row does, and the compiler,
      //  left to itself, hoists them out of the search and spills - the empty statement hides that a key is the same in every round)
      auto mass_from = [&](unsigned t) -> double {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
          asm volatile("" : "+v"(key[i]));
          s += key[i] >= t ? __expf(filter_unkey(key[i]) - m) : 0.f;
          if ((i & 7) == 7) __builtin_amdgcn_sched_barrier(0);
        }
        const double w = score_wave_sum((double)s);
        const double r = filter_block_sum<double>(w, red_s[round & 1], lane, wave);
        ++round;
        return r;
      };
      const double thr = (double)top_p * mass_from(1u);
      unsigned c = 0;
#pragma unroll 1
      for (int bit = 31; bit >= 0; --bit) {
        const unsigned t = c | (1u << bit);
        if (!(mass_from(t) < thr)) c = t;   // H(t - 1) >= top_p * Z: the answer lies at t or above
      }
      cut = max(c, 1u);
    }
  }
  // ---- the perturbed arg-max over the kept ids ----
  const unsigned p = (unsigned)a.stt->pos;
  const unsigned k0 = sa.key[2 * b], k1 = sa.key[2 * b + 1], o0 = sa.off[2 * b], o1 = sa.off[2 * b + 1];
  MaxIdx best{-INFINITY, 0x7fffffff};
#pragma unroll
  for (int q = 0; q < PER / 4; ++q) {
    const bool any = key[4 * q] >= cut || key[4 * q + 1] >= cut || key[4 * q + 2] >= cut || key[4 * q + 3] >= cut;
    if (any) {
      const int v0 = (q * 1024 + filter_opaque(tid)) * 4;
      Philox4 r{{0u, 0u, 0u, 0u}};
      if (noisy) r = philox4x32_10((unsigned)v0 >> 2, p, o0, o1, k0, k1);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (key[4 * q + j] >= cut) {
          const float y = filter_unkey(key[4 * q + j]);
          best = better(best, MaxIdx{noisy ? __fadd_rn(y, gumbel_of(r.w[j])) : y, v0 + j});
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  best = wave_best(best);
  if (lane == 0) red_b[wave] = best;
  __syncthreads();
  if (tid == 0) {
    best = red_b[0];
    for (int w = 1; w < 16; ++w) best = better(best, red_b[w]);
    fa.choice[b] = best.i == 0x7fffffff ? 0 : best.i;   // everything masked
  }
}

__global__ __launch_bounds__(1024) void sample_choice_finish_kernel(FilterArgs fa) {
  finish_step(fa.sm.s, [&](int b, int) { return fa.choice[b]; });   // (read, but not used, for a row the filter kernel left early)
}

// Per-stream sequence bias (tw_generate_greedy_biased; the rule is stated in include/thewhisper.h): one launch in front of the step's
// sampler that edits the float32 logits in place.  One workgroup per row of the launch (a stream at the device position, or - rows
// mode - stream r % rs at position row_pos0 + r / rs, as sampler_mask derives it).  The stream's sequences arrive grouped by last
// token (SeqBiasArgs: the packed table); a thread owns whole groups, walks a group's members in table order - the length-1 member,
// then the caller's order - and adds the active ones into ONE float32 register starting from 0.0f, then does one load, one add and one
// store of the logit.  No atomics and no cross-thread reduction: the order of the sum, hence its bits, is the table's.
__global__ __launch_bounds__(256) void seq_bias_kernel(SeqBiasArgs a) {
  const int r = blockIdx.x;
  int stream, p;
  tw_row_of(r, a.rows_streams, a.rows_streams > 0 ? a.row_pos0 : a.stt->pos, stream, p);
  const int* tab = a.tab;
  const int g0 = tab[kSeqBiasStreamOff + stream], g1 = tab[kSeqBiasStreamOff + stream + 1];
  if (g0 == g1) return;                                   // a row without sequences
  const int n = p + 1;                                    // ids of the history: positions 0 .. p
  if (n < a.stt->n_prompt) return;                        // still consuming its prompt: nothing is sampled
  if (a.rows_streams == 0 && a.finished[r] != 0) return;  // finished: the row receives pad_id whatever the logits say
  const int* grp_off = tab + tab[0];
  const int* grp_tok = tab + tab[1];
  const int* seq_off = tab + tab[2];
  const float* bias = reinterpret_cast<const float*>(tab + tab[3]);
  const int* tokens = tab + tab[4];
  const int* h = a.seq + (long long)stream * a.seq_ld;
  float* lg = a.logits + (long long)r * a.V;
  for (int g = g0 + (int)threadIdx.x; g < g1; g += 256) {
    float total = 0.0f;
    bool any = false;
    const int s1 = grp_off[g + 1];
    for (int s = grp_off[g]; s < s1; ++s) {
      const int t0 = seq_off[s], L = seq_off[s + 1] - t0;
      bool active = L == 1;
      if (!active && L <= n) {
        active = true;
        const int* tail = h + (n - (L - 1));
        for (int j = 0; j < L - 1; ++j)
          if (tail[j] != tokens[t0 + j]) { active = false; break; }
      }
      if (active) { total += bias[s]; any = true; }
    }
    if (any) {
      const int v = grp_tok[g];
      lg[v] = lg[v] + total;
    }
  }
}

// Repetition penalty and no-repeat n-grams on one row (tw_generate_greedy_repeat, tw_repeat_logits; the rule is stated in
// include/thewhisper.h), by one workgroup of kRepeatMaxHist threads: thread i owns history index i.  h: the row's n ids (n <=
// kRepeatMaxHist, every id in [0, V)), hi = h[i] loaded by the caller for every i below the row's allocated length - the address
// does not depend on n, so the load flies beside the loads n comes from; r: the penalty (1.0f = off); N: the n-gram size (0 = off);
// sh: kRepeatMaxHist words of LDS.
// Every argument but the thread index is uniform over the workgroup, so the barriers are reached by all of its threads.
//   penalty: every thread of [ignore, n) loads the ORIGINAL logit of its id; behind a barrier the FIRST occurrence of an id in
//            [ignore, n) - found by scanning the history in LDS, four ids per (broadcast) read - stores the penalised value: an id is
//            penalised once, from its original value, and has one writer.  `/` is IEEE division (the build passes no fast-math flag;
//            __fdiv_rn says so), not a multiply by a reciprocal.
//   n-gram:  behind a second barrier (a banned id may also be a penalised one: -inf has to be the later store) thread i compares the
//            window h[i .. i+N-2] with the suffix h[n-N+1 .. n-1] and stores -inf to h[i+N-1].  Several threads may ban one id: they
//            store the same bits.
// No atomics, and no store whose value depends on the order of the threads.
__device__ __forceinline__ void repeat_row(float* lg, int hi, int n, float r, int N, int ignore, int* sh) {
  const int i = threadIdx.x;
  const int id = i < n ? hi : -1;
  sh[i] = id;
  const bool pen = r != 1.0f && i >= ignore && i < n;
  float x = 0.f;
  if (pen) x = lg[id];
  __syncthreads();
  if (pen) {
    bool first = true;
    const int4* sh4 = reinterpret_cast<const int4*>(sh);
    for (int j = ignore & ~3; j < i; j += 4) {      // (ids in front of `ignore` and at or behind i do not count)
      const int4 q = sh4[j >> 2];
      first &= !((q.x == id && j >= ignore) || (q.y == id && j + 1 >= ignore && j + 1 < i) || (q.z == id && j + 2 >= ignore && j + 2 < i) ||
                 (q.w == id && j + 3 >= ignore && j + 3 < i));
    }
    if (first) lg[id] = x < 0.f ? x * r : __fdiv_rn(x, r);
  }
  if (N < 1 || n < N) return;
  __syncthreads();
  if (i <= n - N) {
    const int* suf = sh + (n - N + 1);
    bool same = true;
    for (int j = 0; j < N - 1; ++j) same &= sh[i + j] == suf[j];
    if (same) lg[sh[i + N - 1]] = -INFINITY;
  }
}

// tw_generate_greedy_repeat: one launch behind seq_bias_kernel (if the call has a bias) and in front of the step's sampler.  One
// workgroup per row of the launch, rows as seq_bias_kernel derives them; rows still consuming their prompt and finished rows are left
// alone, and so is a row whose table entry is off (penalty 1.0f, N 0): its logits keep their bits.
__global__ __launch_bounds__(kRepeatMaxHist) void repeat_kernel(RepeatArgs a) {
  __shared__ __attribute__((aligned(16))) int sh[kRepeatMaxHist];
  const int r = blockIdx.x;
  // (rows mode: r % rows_streams; the ordinary step: r - known before the position is)
  const int stream = a.rows_streams > 0 ? r % a.rows_streams : r;
  const int hi = (int)threadIdx.x < a.seq_ld ? a.seq[(long long)stream * a.seq_ld + threadIdx.x] : -1;
  int stream_, p;
  tw_row_of(r, a.rows_streams, a.rows_streams > 0 ? a.row_pos0 : a.stt->pos, stream_, p);
  const float pen = __int_as_float(a.tab[stream]);
  const int N = a.tab[64 + stream];
  if (pen == 1.0f && N == 0) return;                      // a row with both options off
  const int n = p + 1;                                    // ids of the history: positions 0 .. p
  if (n < a.stt->n_prompt || n > a.seq_ld) return;        // still consuming its prompt: nothing is sampled
  if (a.rows_streams == 0 && a.finished[r] != 0) return;  // finished: the row receives pad_id whatever the logits say
  repeat_row(a.logits + (long long)r * a.V, hi, n, pen, N, a.tab[128], sh);
}

// tw_repeat_logits: the same rule, state from arguments (row r: its own history and its own table entry)
__global__ __launch_bounds__(kRepeatMaxHist) void repeat_logits_kernel(float* logits, int V, const int* hist, int ld, const int* n_hist,
                                                                       const int* tab) {
  __shared__ __attribute__((aligned(16))) int sh[kRepeatMaxHist];
  const int r = blockIdx.x;
  const int hi = (int)threadIdx.x < ld ? hist[(long long)r * ld + threadIdx.x] : -1;
  repeat_row(logits + (long long)r * V, hi, n_hist[r], __int_as_float(tab[r]), tab[64 + r], tab[128], sh);
}

__global__ void advance_kernel(DecState* stt, int n) { stt->pos += n; }

// Language detection (tw_language_logits, tw_detect_language; THE RULE is in include/thewhisper.h): one wavefront per row, lane l holds
// the listed logits j = l and j = l + 64 (n_lang <= kLangMax = 128).  Only the listed logits are read.  The maximum, the lowest token id
// that attains it and the sum are butterflies over the 64 lanes - the operands and their order depend on n_lang alone, never on the
// number of rows or on the row's index - and every lane ends with the same m, id and s.  No LDS, no atomics.
__global__ __launch_bounds__(64) void lang_detect_kernel(const float* logits, int V, const int* ids, int n_lang, int* out_id, float* out_prob) {
  const int r = blockIdx.x, l = threadIdx.x;
  const float* row = logits + (long long)r * V;
  const float ninf = -__builtin_inff();
  const int j0 = l, j1 = l + 64;
  const bool on0 = j0 < n_lang, on1 = j1 < n_lang;
  const int t0 = on0 ? ids[j0] : 0x7fffffff, t1 = on1 ? ids[j1] : 0x7fffffff;
  float x0 = on0 ? row[t0] : ninf, x1 = on1 ? row[t1] : ninf;
  if (x0 != x0) x0 = ninf;   // a NaN counts as -inf
  if (x1 != x1) x1 = ninf;
  const float m = tw_wave_max(fmaxf(x0, x1));
  int best = min((on0 && x0 == m) ? t0 : 0x7fffffff, (on1 && x1 == m) ? t1 : 0x7fffffff);   // m == -inf: every listed id qualifies
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o, 64));
  const bool dead = m == ninf;   // nothing finite in the list: every probability is 0
  const float e0 = (on0 && !dead) ? expf(x0 - m) : 0.f, e1 = (on1 && !dead) ? expf(x1 - m) : 0.f;
  const float s = tw_wave_sum(e0 + e1);
  if (l == 0) out_id[r] = best;
  if (out_prob) {
    float* p = out_prob + (long long)r * n_lang;
    if (on0) p[j0] = dead ? 0.f : e0 / s;
    if (on1) p[j1] = dead ? 0.f : e1 / s;
  }
}

// Beam search (tw_generate_beam, api.hip; THE RULE is in include/thewhisper.h; the tables are BeamArgs', tw_common.h): a step is the
// ordinary decoder pass over n_clips x K rows, then
//  * beam_part_kernel: the slicing, the register-resident slice and the vector / scalar paths of sampler_part_kernel.  Per (row, slice):
//    (max, sum exp(x - max)) over ALL ids (the row's log-softmax is taken before any processor), the greedy partials of the masked
//    logits (what merge_slices decides the mass rule on), and the slice's 2K best unmasked text ids and 2K best unmasked timestamp ids
//    by 2K rounds of "the best one strictly behind the previous one" in the order (logit descending, id ascending).  Within a row the
//    accumulated score is a non-decreasing function of the logit, so the row's 2K best are among them; where the float32 rounding of
//    lp maps two different logits of a row onto one score, the larger logit comes first here (the rule says: the lower id).
//  * beam_finish_kernel: one workgroup per clip, wavefront k merges the slices of beam k (fixed butterfly order), turns the listed
//    logits into accumulated scores and extracts the row's 2K best by the same rounds; the K x 2K survivors are ranked by counting
//    (score descending, flat index k V + v ascending); one thread does steps 4-6, 8 and 9 of the rule; all threads then write the
//    gathered histories from the copies the workgroup took into LDS at its start.
//  * beam_reorder_kernel: the self-attention caches follow beam_idx, in place (see there).
// No atomics, no reduction whose order depends on the launch: a clip's result does not depend on its slot or its batch-mates.

// strictly behind `p` in the order (value descending, id ascending)
__device__ __forceinline__ bool beam_behind(float v, int i, MaxIdx p) { return v < p.v || (v == p.v && i > p.i); }

template <int BEAM_NS, int BEAM_IT>
__global__ __launch_bounds__(256) void beam_part_kernel(BeamArgs ba) {
  __shared__ MaxIdx red_text[2][4], red_ts[2][4];
  __shared__ float red_sum[4], red_raw[2][4];
  const SamplerArgs& a = ba.s;
  const int part = blockIdx.x, b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* lg = a.logits + (long long)b * a.V;
  const VocabSlice sl = vocab_slice<BEAM_NS, BEAM_IT>(a.V, part);
  const int v0 = sl.v0, v1 = sl.v1;
  float s0[BEAM_IT], s1[BEAM_IT];
  unsigned wb[BEAM_IT];
  slice_load(a, lg, sl, tid, s0, s1, wb);
  __builtin_amdgcn_sched_barrier(0);
  const SamplerMask k = sampler_mask(a, b);
  if (k.in_prompt || ba.done[b % ba.n_clips] != 0) return;   // (workgroup-uniform) nothing is selected for this row
  // ---- the slice's part of the row's log-softmax: over every id, before the mask ----
  float rm = -INFINITY;
  if (sl.vec_ok) {
#pragma unroll
    for (int it = 0; it < BEAM_IT; ++it)
      if (v0 + (it * 256 + tid) * 2 < v1) rm = fmaxf(rm, fmaxf(s0[it], s1[it]));
  } else {
    for (int v = v0 + tid; v < v1; v += 256) rm = fmaxf(rm, lg[v]);
  }
  rm = wave_max(rm);
  if (lane == 0) red_raw[0][wave] = rm;
  __syncthreads();
  rm = fmaxf(fmaxf(red_raw[0][0], red_raw[0][1]), fmaxf(red_raw[0][2], red_raw[0][3]));
  float rs = 0.f;
  if (sl.vec_ok) {
#pragma unroll
    for (int it = 0; it < BEAM_IT; ++it)
      if (v0 + (it * 256 + tid) * 2 < v1) { rs += expf(s0[it] - rm); rs += expf(s1[it] - rm); }
  } else {
    for (int v = v0 + tid; v < v1; v += 256) rs += expf(lg[v] - rm);
  }
  rs = wave_sum(rs);
  if (lane == 0) red_raw[1][wave] = rs;
  __syncthreads();
  rs = ((red_raw[1][0] + red_raw[1][1]) + red_raw[1][2]) + red_raw[1][3];
  // ---- the mask, as sampler_part_kernel applies it ----
  if (sl.vec_ok) {
#pragma unroll
    for (int it = 0; it < BEAM_IT; ++it) {
      const int v = v0 + (it * 256 + tid) * 2;
      const bool in = v < v1;
      const int vc = in ? v : 0;
      s0[it] = (in && !sampler_masked_at(a, k, vc, wb[it])) ? s0[it] : -INFINITY;
      s1[it] = (in && !sampler_masked_at(a, k, vc + 1, wb[it])) ? s1[it] : -INFINITY;
    }
  }
  // ---- 2K rounds: the best text and the best timestamp id strictly behind the previous round's ----
  BeamPartial* o = ba.parts + b * SAMPLER_NS_MAX + part;
  MaxIdx pt{INFINITY, -1}, ps{INFINITY, -1}, first_t{-INFINITY, 0x7fffffff}, first_s{-INFINITY, 0x7fffffff};
  const int n_round = 2 * ba.K;
  for (int r = 0; r < n_round; ++r) {
    MaxIdx bt{-INFINITY, 0x7fffffff}, bs{-INFINITY, 0x7fffffff};
    auto take = [&](float x, int v) {
      if (v < k.ts_begin) { if (beam_behind(x, v, pt)) bt = better(bt, MaxIdx{x, v}); }
      else { if (beam_behind(x, v, ps)) bs = better(bs, MaxIdx{x, v}); }
    };
    if (sl.vec_ok) {
#pragma unroll
      for (int it = 0; it < BEAM_IT; ++it) {
        const int v = v0 + (it * 256 + tid) * 2;
        if (v < v1) { take(s0[it], v); take(s1[it], v + 1); }
      }
    } else {
      for (int v = v0 + tid; v < v1; v += 256) take(sampler_masked_at(a, k, v, a.suppress_bits[v >> 5]) ? -INFINITY : lg[v], v);
    }
    bt = wave_best(bt);
    bs = wave_best(bs);
    if (lane == 0) { red_text[r & 1][wave] = bt; red_ts[r & 1][wave] = bs; }
    __syncthreads();
    bt = red_text[r & 1][0];
    bs = red_ts[r & 1][0];
    for (int w = 1; w < 4; ++w) { bt = better(bt, red_text[r & 1][w]); bs = better(bs, red_ts[r & 1][w]); }
    if (!(bt.v > -INFINITY)) bt.i = 0x7fffffff;   // the list is exhausted
    if (!(bs.v > -INFINITY)) bs.i = 0x7fffffff;
    if (tid == 0) { o->tx_v[r] = bt.v; o->tx_i[r] = bt.i; o->ts_v[r] = bs.v; o->ts_i[r] = bs.i; }
    if (r == 0) { first_t = bt; first_s = bs; }
    pt = bt;
    ps = bs;
  }
  const float sum = slice_ts_sum(a, k, sl, lg, tid, s0, s1, first_s.v, red_sum);
  if (tid == 0) {
    o->bt_v = first_t.v; o->bt_i = first_t.i; o->bs_v = first_s.v; o->bs_i = first_s.i;
    o->sum = sum; o->raw_m = rm; o->raw_s = rs; o->pad_ = 0;
  }
}

__global__ __launch_bounds__(512) void beam_finish_kernel(BeamArgs ba) {
  __shared__ int sh_run[kBeamMax][kBeamSeqMax], sh_fin[kBeamMax][kBeamSeqMax];   // the clip's histories as they were before this step
  __shared__ float top_a[kBeamMax][kBeamCand];
  __shared__ int top_t[kBeamMax][kBeamCand];
  __shared__ float cand_s[kBeamCand], cand_r[kBeamCand], cand_f[kBeamCand];
  __shared__ int cand_b[kBeamCand], cand_t[kBeamCand], cand_hit[kBeamCand];
  __shared__ float old_fs[kBeamMax], run_new_s[kBeamMax], fin_new_s[kBeamMax];
  __shared__ int old_flag[kBeamMax], old_len[kBeamMax], run_src[kBeamMax], run_tok[kBeamMax], fin_src[kBeamMax];
  const SamplerArgs& a = ba.s;
  const int c = blockIdx.x, n = ba.n_clips, K = ba.K, C2 = 2 * ba.K;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cur = a.stt->pos + 1, n0 = a.stt->n_prompt;   // cur: tokens every running hypothesis holds
  const long long ld = a.seq_ld;
  if (cur < n0) {   // the prompt lasts: its next token, for every beam
    if (tid < K) {
      const int r = tid * n + c;
      a.cur_ids[r] = a.seq[r * ld + cur];
      ba.beam_idx[r] = tid;
      if (ba.back) ba.back[(cur - 1) * 64 + r] = tid;
    }
    return;
  }
  if (ba.done[c] != 0) {   // frozen
    if (tid < K) {
      ba.beam_idx[tid * n + c] = tid;
      if (ba.back) ba.back[(cur - 1) * 64 + tid * n + c] = tid;
    }
    return;
  }
  for (int idx = tid; idx < K * (cur + 1); idx += 512) {
    const int kk = idx / (cur + 1), i = idx % (cur + 1);
    sh_run[kk][i] = a.seq[(kk * n + c) * ld + i];
    sh_fin[kk][i] = ba.fin_seq[(kk * n + c) * ld + i];
  }
  // ---- per beam: lp of the listed ids, accumulated scores, the row's 2K best ----
  if (wave < K) {
    const int r = wave * n + c;
    const SliceMerge m = merge_slices(a, ba.parts, r, lane);
    const BeamPartial* pp = ba.parts + r * SAMPLER_NS_MAX + (lane & 31);
    const bool on = lane < 32;
    const float pm = on ? pp->raw_m : -INFINITY;
    const float M = wave_max(pm);
    const float S = wave_sum(pm > -INFINITY ? pp->raw_s * expf(pm - M) : 0.f);
    const float logZ = logf(S);
    const float acc = ba.run_score[r];
    const bool is_ts = lane >= 32;
    const float* cvp = is_ts ? pp->ts_v : pp->tx_v;
    const int* cip = is_ts ? pp->ts_i : pp->tx_i;
    float ca[kBeamCand];
    int ci[kBeamCand];
#pragma unroll
    for (int j = 0; j < kBeamCand; ++j) {
      const float x = j < C2 ? cvp[j] : -INFINITY;
      const bool ok = x > -INFINITY && !(m.force_ts && !is_ts);
      ca[j] = ok ? __fadd_rn(__fsub_rn(__fsub_rn(x, M), logZ), acc) : -INFINITY;
      ci[j] = ok ? cip[j] : 0x7fffffff;
    }
    MaxIdx prev{INFINITY, -1};
    for (int rd = 0; rd < C2; ++rd) {
      MaxIdx best{-INFINITY, 0x7fffffff};
#pragma unroll
      for (int j = 0; j < kBeamCand; ++j)
        if (beam_behind(ca[j], ci[j], prev)) best = better(best, MaxIdx{ca[j], ci[j]});
      best = wave_best(best);
      if (lane == 0) { top_a[wave][rd] = best.v; top_t[wave][rd] = best.i; }
      prev = best;
    }
  }
  __syncthreads();
  // ---- the 2K candidates of the clip: rank by counting over the K x 2K survivors ----
  if (tid < K * C2) {
    const int kk = tid / C2, j = tid % C2;
    const float av = top_a[kk][j];
    const int tv = top_t[kk][j];
    int rank = 0;
    for (int e = 0; e < K * C2; ++e) {
      const int k2 = e / C2;
      const float a2 = top_a[k2][e % C2];
      const int t2 = top_t[k2][e % C2];
      const bool beats = a2 > av || (a2 == av && (k2 < kk || (k2 == kk && (t2 < tv || (t2 == tv && e < tid)))));
      rank += beats ? 1 : 0;
    }
    if (rank < C2) {
      cand_s[rank] = av;
      cand_b[rank] = kk;
      cand_t[rank] = tv == 0x7fffffff ? 0 : tv;   // fewer than 2K unmasked ids in the whole clip: score -inf
    }
  }
  __syncthreads();
  // ---- steps 4-6, 8, 9 ----
  if (tid == 0) {
    const float NEG = -1e9f;
    bool all_fin = true;
    for (int kk = 0; kk < K; ++kk) {
      old_fs[kk] = ba.fin_score[kk * n + c];
      old_flag[kk] = ba.fin_flag[kk * n + c];
      old_len[kk] = ba.fin_len[kk * n + c];
      all_fin = all_fin && old_flag[kk] != 0;
    }
    const bool open0 = ba.open[c] != 0;
    const float penv = ba.pen[cur + 1 - n0];
    bool all_hit = true;
    for (int j = 0; j < C2; ++j) {
      const bool hit = cand_t[j] == a.eos || cur + 1 >= ba.max_len;
      cand_hit[j] = hit ? 1 : 0;
      all_hit = all_hit && hit;
      cand_r[j] = hit ? __fadd_rn(cand_s[j], NEG) : cand_s[j];
      float f = __fdiv_rn(cand_s[j], penv);
      if (ba.early && all_fin) f = __fadd_rn(f, NEG);
      if (!open0) f = __fadd_rn(f, NEG);
      if (!(j < K && hit)) f = __fadd_rn(f, NEG);
      cand_f[j] = f;
    }
    unsigned used = 0;
    for (int i = 0; i < K; ++i) {   // step 5: the K best running candidates, lower j first on ties
      int best = -1;
      for (int j = 0; j < C2; ++j)
        if (!((used >> j) & 1u) && (best < 0 || cand_r[j] > cand_r[best])) best = j;
      used |= 1u << best;
      run_src[i] = cand_b[best];
      run_tok[i] = cand_t[best];
      run_new_s[i] = cand_r[best];
    }
    used = 0;
    bool all_new_fin = true;
    int new_flag[kBeamMax], new_len[kBeamMax];
    for (int i = 0; i < K; ++i) {   // step 6: the K best of [old finished, candidates], lower index first on ties
      int best = -1;
      float bv = 0.f;
      for (int p = 0; p < K + C2; ++p) {
        if ((used >> p) & 1u) continue;
        const float v = p < K ? old_fs[p] : cand_f[p - K];
        if (best < 0 || v > bv) { best = p; bv = v; }
      }
      used |= 1u << best;
      fin_src[i] = best;
      fin_new_s[i] = bv;
      new_flag[i] = best < K ? old_flag[best] : ((best - K < K && cand_hit[best - K]) ? 1 : 0);
      new_len[i] = best < K ? old_len[best] : cur + 1;
      all_new_fin = all_new_fin && new_flag[i] != 0;
    }
    const float lhs = __fdiv_rn(run_new_s[0], penv);   // step 8 (pen[cur' - n0] with cur' = cur + 1)
    bool any = false;
    for (int kk = 0; kk < K; ++kk) any = any || lhs > (new_flag[kk] ? fin_new_s[K - 1] : NEG);
    const bool open1 = open0 && any;
    for (int kk = 0; kk < K; ++kk) {
      ba.fin_score[kk * n + c] = fin_new_s[kk];
      ba.fin_flag[kk * n + c] = new_flag[kk];
      ba.fin_len[kk * n + c] = new_len[kk];
    }
    ba.open[c] = open1 ? 1 : 0;
    ba.done[c] = (!open1 || (ba.early && all_new_fin) || all_hit) ? 1 : 0;   // step 9
    if (ba.fin_last) {   // a finished entry keeps the beam that produced its last token as it moves through the set
      int old_last[kBeamMax];
      for (int kk = 0; kk < K; ++kk) old_last[kk] = ba.fin_last[kk * n + c];
      for (int kk = 0; kk < K; ++kk) ba.fin_last[kk * n + c] = fin_src[kk] < K ? old_last[fin_src[kk]] : cand_b[fin_src[kk] - K];
    }
  }
  __syncthreads();
  // ---- the new histories, gathered from the LDS copies ----
  for (int idx = tid; idx < K * (cur + 1); idx += 512) {
    const int kk = idx / (cur + 1), i = idx % (cur + 1);
    a.seq[(kk * n + c) * ld + i] = i < cur ? sh_run[run_src[kk]][i] : run_tok[kk];
    const int fs = fin_src[kk];
    ba.fin_seq[(kk * n + c) * ld + i] = fs < K ? sh_fin[fs][i] : (i < cur ? sh_run[cand_b[fs - K]][i] : cand_t[fs - K]);
  }
  if (tid < K) {
    const int r = tid * n + c, src = run_src[tid], tok = run_tok[tid];
    const int ts_begin = a.timestamps ? a.no_ts_id + 1 : a.V;
    int lt = -1;   // recomputed from the gathered history, as sampler_rows_finish_kernel does
    for (int i = n0; i < cur; ++i) if (sh_run[src][i] >= ts_begin) lt = sh_run[src][i];
    if (tok >= ts_begin) lt = tok;
    a.last_ts[r] = lt;
    a.cur_ids[r] = tok;
    ba.beam_idx[r] = src;
    ba.run_score[r] = run_new_s[tid];
    if (ba.back) ba.back[(cur - 1) * 64 + r] = src;
  }
}

// The alignment rows follow the finished hypotheses (tw_generate_beam_aligned), in place, one launch behind the loop.  The cross
// attention wrote row (slot, position) once, for the beam that sat in the slot when the position was consumed, and the loop never moved
// a row; BeamArgs::back holds who continued whom.  Hypothesis k of a clip, of `len` tokens: its row at position len - 2 is in the slot
// fin_last[k], and the row at position p - 1 in slot back[p - 1][slot of p].  Workgroup = (PCH positions, alignment head, clip): the
// clip's back-pointers from the chunk's first position on are staged in LDS as bytes (4 KiB for 512 positions), thread k walks
// hypothesis k down to the chunk and leaves the source slot of each of its positions (-1: nothing to copy - the row is in place, behind
// the hypothesis's end, or the entry is a placeholder).  Then, per position, a thread loads the elements it owns from ALL K sources
// before it stores any: two hypotheses may share a source and a destination may be another one's source (beam_reorder_kernel's
// pattern; no other thread touches those addresses).  VEC 4: 16-byte accesses, taken only when T % 4 == 0 (every row then starts on a
// 16-byte boundary); VEC 1 otherwise.  No atomics.
constexpr int kAlignGatherPos = 4;
template <int VEC>
__global__ __launch_bounds__(256) void beam_align_gather_kernel(float* align, int Ha, int P, int T, int n_pos, BeamArgs ba) {
  __shared__ unsigned char sh_back[kBeamSeqMax][kBeamMax];
  __shared__ int sh_src[kAlignGatherPos][kBeamMax];
  using vec_t = typename std::conditional<VEC == 4, u32x4_t, float>::type;
  const int p0 = blockIdx.x * kAlignGatherPos, h = blockIdx.y, c = blockIdx.z, n = ba.n_clips, K = ba.K;
  const int tid = threadIdx.x;
  const int n0 = ba.s.stt->n_prompt;
  const int hi = min(n_pos, kBeamSeqMax);   // positions [p0, hi) may be walked
  for (int idx = tid; idx < (hi - p0) * K; idx += 256) {
    const int s = p0 + idx / K, k = idx % K;
    const int b = ba.back[s * 64 + k * n + c];
    sh_back[s][k] = (unsigned char)((b >= 0 && b < K) ? b : k);
  }
  if (tid < kAlignGatherPos * kBeamMax) sh_src[tid / kBeamMax][tid % kBeamMax] = -1;
  __syncthreads();
  if (tid < K) {
    const int r = tid * n + c;
    const int len = min(max(ba.fin_len[r], n0), ba.max_len);
    const bool live = ba.fin_score[r] > -1e9f && len >= 2;
    int b = ba.fin_last[r];
    b = (b >= 0 && b < K) ? b : tid;
    if (live && len - 2 >= p0) {
      for (int p = min(len - 2, hi - 1); p >= p0; --p) {   // (len - 2 <= hi - 1 always: a finished entry ends inside the loop's positions)
        if (p < p0 + kAlignGatherPos && b != tid) sh_src[p - p0][tid] = b;
        if (p > p0) b = sh_back[p - 1][b];
      }
    }
  }
  __syncthreads();
  const int TV = T / VEC;
  for (int pl = 0; pl < kAlignGatherPos; ++pl) {
    const int p = p0 + pl;
    if (p >= hi) break;
    int src[kBeamMax];
    bool any = false;
#pragma unroll
    for (int k = 0; k < kBeamMax; ++k) {
      src[k] = sh_src[pl][k];
      any = any || src[k] >= 0;
    }
    if (!any) continue;   // (workgroup-uniform)
    vec_t* base = reinterpret_cast<vec_t*>(align + ((long long)h * P + p) * T);
    const long long slot_vec = (long long)Ha * P * T / VEC;
    for (int t = tid; t < TV; t += 256) {
      vec_t val[kBeamMax];
#pragma unroll
      for (int k = 0; k < kBeamMax; ++k)
        if (src[k] >= 0) val[k] = base[(long long)(src[k] * n + c) * slot_vec + t];
#pragma unroll
      for (int k = 0; k < kBeamMax; ++k)
        if (src[k] >= 0) base[(long long)(k * n + c) * slot_vec + t] = val[k];
    }
  }
}

// Self-attention caches follow the beams, in place, one launch: workgroup = (64-key chunk, head, (layer, K | V, clip)).  A thread owns
// VPT 16-byte vector offsets of the chunk and, for them, the vectors of ALL the clip's beams: it loads every vector it will
// overwrite's source first, then stores - no other thread touches those addresses, so there is no staging arena and nothing to order.
// Beams that continue themselves are not copied; a clip whose beam_idx is the identity, or which is done, returns at once.
template <int VPT>   // 4: float32, 2: 16-bit elements (64 keys x 64 dims = VPT x 256 vectors)
__global__ __launch_bounds__(256) void beam_reorder_kernel(u32x4_t* kc, u32x4_t* vc, long long layer_vec, long long b_vec, long long h_vec,
                                                           BeamArgs ba) {
  const int chunk = blockIdx.x, h = blockIdx.y, n = ba.n_clips, K = ba.K;
  const int clip = blockIdx.z % n, kv = (blockIdx.z / n) & 1, layer = blockIdx.z / (2 * n);
  if (chunk * 64 > ba.s.stt->pos || ba.done[clip] != 0) return;
  int src[kBeamMax];
  bool any = false;
#pragma unroll
  for (int k = 0; k < kBeamMax; ++k) {
    src[k] = k < K ? ba.beam_idx[k * n + clip] : k;
    any = any || src[k] != k;
  }
  if (!any) return;
  u32x4_t* base = (kv ? vc : kc) + layer * layer_vec + h * h_vec + (long long)chunk * (VPT * 256) + threadIdx.x;
  u32x4_t val[kBeamMax][VPT];
#pragma unroll
  for (int k = 0; k < kBeamMax; ++k)
    if (src[k] != k) {
#pragma unroll
      for (int j = 0; j < VPT; ++j) val[k][j] = base[(long long)(src[k] * n + clip) * b_vec + j * 256];
    }
#pragma unroll
  for (int k = 0; k < kBeamMax; ++k)
    if (src[k] != k) {
#pragma unroll
      for (int j = 0; j < VPT; ++j) base[(long long)(k * n + clip) * b_vec + j * 256] = val[k][j];
    }
}

// cross K / V of slot c -> slots k n + c, k >= 1: workgroup = (1024 vectors of a slot, destination slot - n, (layer, K | V))
__global__ __launch_bounds__(256) void beam_cross_copy_kernel(u32x4_t* ck, u32x4_t* cv, long long layer_vec, long long slot_vec, int n) {
  const int dst = n + blockIdx.y, clip = dst % n;
  u32x4_t* base = ((blockIdx.z & 1) ? cv : ck) + (long long)(blockIdx.z >> 1) * layer_vec;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long long i = ((long long)blockIdx.x * 4 + j) * 256 + threadIdx.x;
    if (i < slot_vec) base[dst * slot_vec + i] = base[clip * slot_vec + i];
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// Projection dispatch.  api.hip's decode_core issues seven projections per token (with the tile rows its retile picks): QKV
// (LN, K/V scatter, 16-row tiles), out-projection (residual; 16-row tiles when the fused form has more than 2048 rows), cross query
// (LN, 8-row), cross out-projection (residual, 8-row), fc1 (LN + GELU; 16-row above 2048 rows), fc2 (residual, 8-row) and the tied
// logits (LN, fp32 out, 16-row).  Only those flavours are built.

// one launch; the epilogue follows from the arguments
template <typename T, int NW, int SK_MAXS, bool MULTI, bool W8, int CG, int TR, bool A16 = false, int MODE = 0, bool SPLIT2 = false>
static hipError_t sk_go(const GemvArgs& a, dim3 grid, size_t lds1, hipStream_t st) {
  const bool ln = a.ln_gw != nullptr;
  const size_t lds = lds1 * CG;
#define SK_GO(LNV, EPIV) hipLaunchKernelGGL((skinny_mfma_kernel<T, NW, SK_MAXS, LNV, EPIV, MULTI, W8, CG, TR, A16, MODE, SPLIT2>), grid, dim3(NW * 64), lds, st, \
                                            a.x, a.W, a.K, a.B, a.N, a.rg, a.wscale, a.bias, a.res, a.ln_gw, a)
  if constexpr (NW >= 16 || SPLIT2) {  // the long-K residual projection (fc2)
    if (ln || a.y_f32 || a.kcache || a.gelu || !a.res) return hipErrorInvalidValue;
    SK_GO(false, SK_RES);
  } else if constexpr (TR != 16) {  // narrow tiles: residual, LN, LN + GELU projections
    if (a.y_f32 || a.kcache) return hipErrorInvalidValue;
    if (a.gelu) { if (!ln || a.res) return hipErrorInvalidValue; SK_GO(true, SK_GELU); }
    else if (a.res) { if (ln) return hipErrorInvalidValue; SK_GO(false, SK_RES); }
    else if (ln) SK_GO(true, SK_STORE);
    else return hipErrorInvalidValue;
  } else if (a.y_f32) {
    if (!ln || a.res || a.gelu || a.kcache) return hipErrorInvalidValue;
    SK_GO(true, SK_F32);
  } else if (a.kcache) {
    if (!ln || a.res || a.gelu) return hipErrorInvalidValue;
    if (a.n_pad) {   // ragged step: an instantiation of its own, the plain call's launch is untouched
      if (a.rows_streams != 0) return hipErrorInvalidValue;
      SK_GO(true, SK_KV_RAG);
    } else {
      SK_GO(true, SK_KV);
    }
  } else if (a.gelu) {
    if (!ln || a.res) return hipErrorInvalidValue;
    SK_GO(true, SK_GELU);
  } else if (a.res) {
    if (ln) return hipErrorInvalidValue;
    SK_GO(false, SK_RES);
  } else {
    return hipErrorInvalidValue;
  }
#undef SK_GO
  return hipGetLastError();
}

// 16-bit or f32 weights.  NW = 16 only for the long-K residual projection with one group of streams (`big` in skinny_launch);
// split2: its several-groups form on 8 wavefronts.
template <typename T, int NW, int TR>
static hipError_t skinny_launch_nw(const GemvArgs& a0, hipStream_t st, bool split2 = false) {
  constexpr int E = ElemTraits<T>::kPer16B;
  GemvArgs a = a0;
  if (a.K % (4 * E) != 0 || a.B > 64) return hipErrorInvalidValue;
  const size_t lds = (size_t)NW * kRedTile * 4;
  const int tiles = (a.N + TR - 1) / TR;
  const int steps = a.K / E / 4;
  const int steps_per_wave = (steps + NW - 1) / NW;
  const bool groups = a.B > 16;  // several groups of 16 streams: 5 fragments in flight, further rounds for longer K
  // at most 512 workgroups: tall matrices (the tied logits projection) walk several tiles per workgroup
  a.rg = (tiles + 511) / 512;
  if (a.rg < 1 || steps_per_wave > (groups ? 5 : 10)) a.rg = 1;  // several tiles per workgroup only with one round per tile
  if constexpr (TR != 16) { if (a.rg > 1) return hipErrorInvalidValue; }
  dim3 grid((tiles + a.rg - 1) / a.rg);
  if constexpr (NW == 16) {   // K >= 4096: at least 8 steps per wavefront, rounds of 10
    if (groups || a.rg != 1) return hipErrorInvalidValue;
    return sk_go<T, 16, 10, false, false, 1, TR>(a, grid, lds, st);
  } else {
    // more than 16 streams, K an exact multiple of the wavefronts' step: operand rings (skinny_mfma_kernel MODE 2), one tile per
    // workgroup - or, for the launches with more 16-row tiles than the decode loop has compute units (QKV, fc1: 320 on 160 CUs),
    // TWO tiles per workgroup contracted against one sweep of the activation rings (DUAL: half the activation traffic)
    if (groups && a.rg == 1 && steps % NW == 0 && !a.y_f32) {
      const int spw = steps / NW;
      constexpr int SPW = E == 8 ? 5 : 10;    // K = 1280
      bool dual = false;
      if constexpr (TR == 16) dual = !split2 && (a.kcache || a.gelu) && tiles > 160 && tiles <= 320 && tiles % 2 == 0 && spw == SPW;
      if (dual) { a.rg = 2; grid = dim3(tiles / 2); }
#define SK_RING(SPWV, SP2, MU) (a.B <= 32 ? sk_go<T, NW, SPWV, MU, false, 2, TR, false, 2, SP2>(a, grid, lds, st) \
                                          : sk_go<T, NW, SPWV, MU, false, 4, TR, false, 2, SP2>(a, grid, lds, st))
      if constexpr (TR == 16) { if (dual) return SK_RING(SPW, false, true); }
      if (spw == SPW && !split2) return SK_RING(SPW, false, false);
      if (spw == 4 * SPW && split2) return SK_RING(4 * SPW, true, false);   // K = 5120: fc2 of the large models
#undef SK_RING
    }
    if (split2) {   // other long K (e.g. ffn = 4096): rounds of 5 fragments, the slice's midpoint found per step
      if (!groups || a.rg != 1) return hipErrorInvalidValue;
      return a.B <= 32 ? sk_go<T, NW, 5, false, false, 2, TR, false, 0, true>(a, grid, lds, st)
                       : sk_go<T, NW, 5, false, false, 4, TR, false, 0, true>(a, grid, lds, st);
    }
    if (groups) {   // several groups of 16 streams: 8 wavefronts x 5 fragments in flight (more rounds for long K) keep the
                    // per-group activation fragments inside the register file
      if constexpr (TR == 16) {
        if (a.rg > 1) return a.B <= 32 ? sk_go<T, NW, 5, true, false, 2, TR>(a, grid, lds, st) : sk_go<T, NW, 5, true, false, 4, TR>(a, grid, lds, st);
      }
      return a.B <= 32 ? sk_go<T, NW, 5, false, false, 2, TR>(a, grid, lds, st) : sk_go<T, NW, 5, false, false, 4, TR>(a, grid, lds, st);
    }
    if constexpr (TR == 16) {
      if (a.rg > 1) return steps_per_wave <= 5 ? sk_go<T, NW, 5, true, false, 1, TR>(a, grid, lds, st) : sk_go<T, NW, 10, true, false, 1, TR>(a, grid, lds, st);
    }
    return steps_per_wave <= 5 ? sk_go<T, NW, 5, false, false, 1, TR>(a, grid, lds, st) : sk_go<T, NW, 10, false, false, 1, TR>(a, grid, lds, st);
  }
}

// MXFP8 weights: 128-k steps; 2 steps per wavefront cover K = 1280 with 8 wavefronts, 3 cover K = 5120 with 16.  a.a16: W8A16
// (weights widened in registers, bf16 activations) - the only flavour with several groups of 16 streams (2 steps = 8 activation
// fragments per group in flight, further rounds for longer K)
template <int NW, int TR>
static hipError_t skinny_launch_w8(const GemvArgs& a0, hipStream_t st, bool split2 = false) {
  GemvArgs a = a0;
  if (a.K % 128 != 0 || a.B > 64) return hipErrorInvalidValue;
  const size_t lds = (size_t)NW * kRedTile * 4;
  const int tiles = (a.N + TR - 1) / TR;
  const int steps_per_wave = (a.K / 128 + NW - 1) / NW;
  const bool groups = a.B > 16;
  if (groups && !a.a16) return hipErrorInvalidValue;
  // several groups of streams: every workgroup re-reads the whole activation block (164 KB per 64 streams at K = 1280, more bytes than
  // its weight tile), so the 320-tile launches walk TWO tiles per workgroup and keep the activation fragments in registers
  // (64 streams x 15 s: 3.50 -> 3.32 ms per step, profiles/r04_b64_15s_two_tiles_per_workgroup.txt; neutral for the bf16 kernels);
  // one group: at most 512 workgroups (the tied logits projection)
  const int max_blocks = groups ? 160 : 512;
  a.rg = (tiles + max_blocks - 1) / max_blocks;
  if (a.rg < 1 || steps_per_wave > (groups ? 2 : 3)) a.rg = 1;   // several tiles per workgroup only with one round per tile
  if (groups && !a.kcache && !a.gelu && !a.y_f32) a.rg = 1;      // ... and with several groups only for QKV, fc1 and the logits
  if constexpr (TR != 16) { if (a.rg > 1) return hipErrorInvalidValue; }
  dim3 grid((tiles + a.rg - 1) / a.rg);
  if (split2) {   // W8A16 above 16 rows, long K: rounds of 2 steps, two accumulator sets (skinny_mfma_kernel's header)
    if constexpr (NW != 8) {
      return hipErrorInvalidValue;
    } else {
      if (!groups || a.rg != 1) return hipErrorInvalidValue;
      return a.B <= 32 ? sk_go<bf16_t, NW, 2, false, true, 2, TR, true, 0, true>(a, grid, lds, st)
                       : sk_go<bf16_t, NW, 2, false, true, 4, TR, true, 0, true>(a, grid, lds, st);
    }
  }
  if (groups) {
    if constexpr (NW != 8) {
      return hipErrorInvalidValue;
    } else {
      if constexpr (TR == 16) {
        if (a.rg > 1) return a.B <= 32 ? sk_go<bf16_t, NW, 2, true, true, 2, TR, true>(a, grid, lds, st) : sk_go<bf16_t, NW, 2, true, true, 4, TR, true>(a, grid, lds, st);
      }
      return a.B <= 32 ? sk_go<bf16_t, NW, 2, false, true, 2, TR, true>(a, grid, lds, st) : sk_go<bf16_t, NW, 2, false, true, 4, TR, true>(a, grid, lds, st);
    }
  }
#define SK_W8(S, MU) (a.a16 ? sk_go<bf16_t, NW, S, MU, true, 1, TR, true>(a, grid, lds, st) : sk_go<bf16_t, NW, S, MU, true, 1, TR>(a, grid, lds, st))
  if constexpr (TR == 16) {
    if (a.rg > 1) return steps_per_wave <= 2 ? SK_W8(2, true) : SK_W8(3, true);
  }
  return steps_per_wave <= 2 ? SK_W8(2, false) : SK_W8(3, false);
#undef SK_W8
}

template <typename T>
static hipError_t skinny_launch(const GemvArgs& a, hipStream_t st) {
  // long-K residual projection (fc2, N = d_model: always 8-row tiles): 16 wavefronts per tile with one group of streams, 8 (two
  // accumulator sets: the same sixteen K slices, the same order of additions - skinny_mfma_kernel's header) with several
  const bool longk = a.K >= 4096 && !a.ln_gw && !a.y_f32 && !a.kcache && !a.gelu;
  const bool big = longk && a.B <= 16, split2 = longk && a.B > 16;
  if (a.tr != 0 && a.tr != 8 && a.tr != 16) return hipErrorInvalidValue;
  if (a.tr != 8 && longk) return hipErrorInvalidValue;
  if (a.wscale) {
    if (ElemTraits<T>::kCode != 1) return hipErrorInvalidValue;
    if (a.tr == 8) return big ? skinny_launch_w8<16, 8>(a, st) : skinny_launch_w8<8, 8>(a, st, split2);
    return skinny_launch_w8<8, 16>(a, st);
  }
  if (a.tr == 8) return big ? skinny_launch_nw<T, 16, 8>(a, st) : skinny_launch_nw<T, 8, 8>(a, st, split2);
  return skinny_launch_nw<T, 8, 16>(a, st);
}

template <typename T>
static hipError_t gemv_b(const GemvArgs& a0, hipStream_t st) {
  if (a0.B < 1 || a0.B > 64) return hipErrorInvalidValue;
  GemvArgs a = a0;
  if (a.kcache) {   // QKV launch: a fourth segment of d_model rows only together with its destination
    if ((a.N == 4 * a.d_model) != (a.u != nullptr)) return hipErrorInvalidValue;
    a.nsplit = a.N;
  } else if (a.u) {  // residual launch with a composed half
    if (!a.res || !a.stats || a.nsplit <= 0 || a.nsplit >= a.N || a.nsplit % 16 != 0) return hipErrorInvalidValue;
  } else {
    a.nsplit = a.N;
  }
  return skinny_launch<T>(a, st);
}

hipError_t launch_gemv(int dtype, const GemvArgs& a, hipStream_t st) {
  return dtype == 1 ? gemv_b<bf16_t>(a, st) : (dtype == 2 ? gemv_b<f16_t>(a, st) : gemv_b<float>(a, st));
}

hipError_t launch_dec_self_attn(int dtype, const void* q, const void* kc, const void* vc, int rows, void* out, int B, int H,
                                int key_bound, const DecState* stt, int rows_streams, hipStream_t st) {
  // key_bound: an upper bound of pos+1 for this call known on the host (prompt + max new tokens)
  int kb = (key_bound + 63) / 64 * 64;
  if (rows % 64 != 0 || rows > 512 || kb > rows) return hipErrorInvalidValue;
  const bool single = kb <= 256;
  const int nw = kb <= 64 ? 1 : (kb <= 128 ? 2 : 4);
#define SA_GO(TT, SV, NWV) hipLaunchKernelGGL((dec_self_attn_kernel<TT, SV, NWV>), dim3(H, B), dim3(NWV * 64), 0, st, (const TT*)q, \
                                              (const TT*)kc, (const TT*)vc, rows, H, kb, (TT*)out, stt, rows_streams)
#define SA_PICK(TT) do { if (nw == 1) SA_GO(TT, true, 1); else if (nw == 2) SA_GO(TT, true, 2); else if (single) SA_GO(TT, true, 4); \
                         else SA_GO(TT, false, 4); } while (0)
  if (dtype == 1) SA_PICK(bf16_t); else if (dtype == 2) SA_PICK(f16_t); else SA_PICK(float);
#undef SA_PICK
#undef SA_GO
  return hipGetLastError();
}

hipError_t launch_dec_self_attn_ragged(int dtype, const void* q, const void* kc, const void* vc, int rows, void* out, int B, int H,
                                       int key_bound, const DecState* stt, const int* n_pad, hipStream_t st) {
  // the bucket is the plain launch's, picked from the ABSOLUTE position: a row position is never behind it
  int kb = (key_bound + 63) / 64 * 64;
  if (rows % 64 != 0 || rows > 512 || kb > rows || !n_pad || B < 1 || B > 64) return hipErrorInvalidValue;
  const bool single = kb <= 256;
  const int nw = kb <= 64 ? 1 : (kb <= 128 ? 2 : 4);
#define SA_GO(TT, SV, NWV) hipLaunchKernelGGL((dec_self_attn_ragged_kernel<TT, SV, NWV>), dim3(H, B), dim3(NWV * 64), 0, st, (const TT*)q, \
                                              (const TT*)kc, (const TT*)vc, rows, H, kb, (TT*)out, stt, n_pad)
#define SA_PICK(TT) do { if (nw == 1) SA_GO(TT, true, 1); else if (nw == 2) SA_GO(TT, true, 2); else if (single) SA_GO(TT, true, 4); \
                         else SA_GO(TT, false, 4); } while (0)
  if (dtype == 1) SA_PICK(bf16_t); else if (dtype == 2) SA_PICK(f16_t); else SA_PICK(float);
#undef SA_PICK
#undef SA_GO
  return hipGetLastError();
}

hipError_t launch_dec_cross_attn(int dtype, const void* q, const FusedQ& fq, const void* ck, const void* cv, void* out, int B, int H,
                                 int T, int Tp, const int* align_slot_for_head, float* align, int Ha, int P,
                                 const DecState* stt, const unsigned char* ksc, const unsigned char* vsc, int rows_streams,
                                 hipStream_t st) {
  if (Tp % 64 != 0 || Tp < T) return hipErrorInvalidValue;
  const bool single = Tp <= 512;
  const bool f = fq.u != nullptr;
  if (f) {   // the partial statistics must fit the per-lane request budget of fq_request
    if (!fq.stats || !fq.gw || !fq.cb || fq.d != H * 64 || fq.n_part < 1 || fq.n_part > 192) return hipErrorInvalidValue;
  } else if (!q) {
    return hipErrorInvalidValue;
  }
  if (ksc || vsc) {  // fp8 K / V^T caches with per-key scales (TW_BF16_MXFP8 contexts)
    if (!ksc || !vsc || dtype != 1) return hipErrorInvalidValue;
    const size_t lds8 = (size_t)Tp * sizeof(float) * 2;
#define CA8_GO(GV, FV) hipLaunchKernelGGL((dec_cross_attn_kv8_kernel<GV, FV>), dim3(H, B), dim3(512), lds8, st,                        \
                                          (const unsigned char*)ck, (const unsigned char*)cv, ksc, vsc, H, Tp, T, rows_streams, (const bf16_t*)q,  \
                                          (bf16_t*)out, align_slot_for_head, align, Ha, P, stt, fq)
#define CA8_PICK(FV) do { if (Tp <= 512) CA8_GO(1, FV); else if (Tp <= 1024) CA8_GO(2, FV); else if (Tp <= 1536) CA8_GO(3, FV);      \
                          else return hipErrorInvalidValue; } while (0)
    if (f) CA8_PICK(true); else CA8_PICK(false);
#undef CA8_PICK
#undef CA8_GO
    return hipGetLastError();
  }
  if (rows_streams > 0 && B > rows_streams) {   // several positions per stream: one K / V^T pass per (stream, head, 16 positions)
    if (B % rows_streams != 0 || Tp > 1536) return hipErrorInvalidValue;
    const int n_pos = B / rows_streams;
    const dim3 grid(H, rows_streams, (n_pos + 15) / 16);
    const size_t esz = dtype == 0 ? 4 : 2;
    const size_t ldsr = ((size_t)16 * (Tp + 4) + 8 * 16 * 68 + 2 * 8 * 16) * sizeof(float) + 16 * 64 * esz;
    constexpr int lds_cap = 16 * (1536 + 4) * 4 + 8 * 16 * 68 * 4 + 2 * 8 * 16 * 4 + 16 * 64 * 4;
    static_assert(lds_cap <= 160 * 1024, "LDS of a compute unit");
#define CAR_GO(TT, SV, FV) do {                                                                                                        \
      static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&dec_cross_attn_rows_kernel<TT, SV, FV>),       \
                                                          hipFuncAttributeMaxDynamicSharedMemorySize, lds_cap);                        \
      if (attr != hipSuccess) return attr;                                                                                             \
      hipLaunchKernelGGL((dec_cross_attn_rows_kernel<TT, SV, FV>), grid, dim3(512), ldsr, st, (const TT*)ck, (const TT*)cv, H, Tp, T,  \
                         rows_streams, n_pos, (const TT*)q, (TT*)out, align_slot_for_head, align, Ha, P, stt, fq);                     \
    } while (0)
#define CAR_PICK(TT) do { if (single) { if (f) CAR_GO(TT, true, true); else CAR_GO(TT, true, false); }                               \
                          else { if (f) CAR_GO(TT, false, true); else CAR_GO(TT, false, false); } } while (0)
    if (dtype == 1) CAR_PICK(bf16_t); else if (dtype == 2) CAR_PICK(f16_t); else CAR_PICK(float);
#undef CAR_PICK
#undef CAR_GO
    return hipGetLastError();
  }
  const size_t lds = (size_t)Tp * sizeof(float);
#define CA_GO(TT, SV, FV) hipLaunchKernelGGL((dec_cross_attn_kernel<TT, SV, FV>), dim3(H, B), dim3(512), lds, st, (const TT*)ck,      \
                                             (const TT*)cv, H, Tp, T, rows_streams, (const TT*)q, (TT*)out, align_slot_for_head, align, Ha, P, stt, fq)
#define CA_PICK(TT) do { if (single) { if (f) CA_GO(TT, true, true); else CA_GO(TT, true, false); }                                  \
                         else { if (f) CA_GO(TT, false, true); else CA_GO(TT, false, false); } } while (0)
  if (dtype == 1) CA_PICK(bf16_t); else if (dtype == 2) CA_PICK(f16_t); else CA_PICK(float);
#undef CA_PICK
#undef CA_GO
  return hipGetLastError();
}

hipError_t launch_sampler(const SamplerArgs& a0, hipStream_t st) {
  if (a0.B < 1 || a0.B > 64 || !a0.partials || !a0.suppress_bits) return hipErrorInvalidValue;
  SamplerArgs a = a0;
  // 32 vocabulary slices per stream (<= 4 x 512 logits per workgroup).  Until round 3 launches for >= 8 streams used 8 slices of 13 x 512
  // ("8 x B workgroups cover the chip"); same-box A/B at 16 streams: 1.3824 -> 1.3759 ms per step with 32
  a.n_slices = 32;
  hipLaunchKernelGGL((sampler_part_kernel<32, 4>), dim3(32, a.B), dim3(256), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sampler_finish_kernel, dim3(1), dim3(1024), 0, st, a);  // also advances the position
  return hipGetLastError();
}

hipError_t launch_sampler_rows(const SamplerArgs& a0, hipStream_t st) {
  if (a0.B < 1 || a0.B > 64 || !a0.partials || !a0.suppress_bits || a0.rows_streams < 1 || a0.B % a0.rows_streams != 0 || !a0.row_lastts ||
      !a0.row_choice || !a0.verify_state)
    return hipErrorInvalidValue;
  SamplerArgs a = a0;
  a.n_slices = 32;    // the slicing of launch_sampler (the partial sums are merged in the same order: same bits)
  a.x_next = nullptr;
  hipLaunchKernelGGL((sampler_part_kernel<32, 4>), dim3(32, a.B), dim3(256), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sampler_rows_finish_kernel, dim3(1), dim3(1024), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_sample(const SampleArgs& a0, hipStream_t st) {
  const SamplerArgs& s = a0.s;
  if (s.B < 1 || s.B > 64 || s.rows_streams != 0 || !s.suppress_bits || !a0.inv_t || !a0.key || !a0.off || !a0.noisy || !a0.parts)
    return hipErrorInvalidValue;
  SampleArgs a = a0;
  a.s.n_slices = 32;   // the slicing of launch_sampler: the unscaled partials, and the order they are merged in, are the greedy call's
  hipLaunchKernelGGL((sample_part_kernel<32, 4>), dim3(32, s.B), dim3(256), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sample_finish_kernel, dim3(1), dim3(1024), 0, st, a);  // also advances the position
  return hipGetLastError();
}

hipError_t launch_sample_filtered(const FilterArgs& a0, hipStream_t st) {
  const SamplerArgs& s = a0.sm.s;
  if (s.B < 1 || s.B > 64 || s.V < 1 || s.V > kFilterMaxVocab || s.rows_streams != 0 || !s.suppress_bits || !a0.sm.inv_t || !a0.sm.key ||
      !a0.sm.off || !a0.sm.noisy || !a0.sm.parts || !a0.top_k || !a0.top_p || !a0.choice)
    return hipErrorInvalidValue;
  FilterArgs a = a0;
  a.sm.s.n_slices = 32;   // the slicing of launch_sampler, as launch_sample: the mass decision is the unfiltered call's
  hipLaunchKernelGGL((sample_part_kernel<32, 4>), dim3(32, s.B), dim3(256), 0, st, a.sm);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sample_filter_kernel, dim3(s.B), dim3(1024), 0, st, a);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sample_choice_finish_kernel, dim3(1), dim3(1024), 0, st, a);  // also advances the position
  return hipGetLastError();
}

hipError_t launch_score_rows(const ScoreArgs& a, hipStream_t st) {
  const SamplerArgs& s = a.s;
  if (s.B < 1 || s.B > 64 || s.rows_streams < 1 || s.B % s.rows_streams != 0 || !s.logits || !s.seq || !s.stt || !s.suppress_bits ||
      !s.row_lastts || !a.parts || !a.out_masked || !a.out_raw || (a.ns_id >= 0 && !a.out_ns) || a.ns_id >= s.V)
    return hipErrorInvalidValue;
  // 32 slices of <= 4 x 512 logits per row whatever the number of rows (the sampler's slicing): a row's partials, and the order they
  // are merged in, are the same in every launch
  hipLaunchKernelGGL((score_part_kernel<4>), dim3(SCORE_NS, s.B), dim3(256), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(score_finish_kernel, dim3(1), dim3(1024), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_suppress_bitmap(const int* list, int n, unsigned* bits, int V, hipStream_t st) {
  hipError_t e = hipMemsetAsync(bits, 0, (size_t)((V + 31) / 32) * 4, st);
  if (e != hipSuccess || n <= 0) return e;
  hipLaunchKernelGGL(suppress_bitmap_kernel, dim3((n + 255) / 256), dim3(256), 0, st, list, n, bits, V);
  return hipGetLastError();
}

hipError_t launch_seq_bias(const SeqBiasArgs& a, hipStream_t st) {
  if (a.rows < 1 || a.rows > 64 || !a.logits || !a.seq || !a.stt || !a.tab || a.rows_streams < 0 ||
      (a.rows_streams == 0 ? !a.finished : a.rows % a.rows_streams != 0))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(seq_bias_kernel, dim3(a.rows), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_repeat(const RepeatArgs& a, hipStream_t st) {
  if (a.rows < 1 || a.rows > 64 || !a.logits || !a.seq || !a.stt || !a.tab || a.rows_streams < 0 || a.seq_ld > kRepeatMaxHist ||
      (a.rows_streams == 0 ? !a.finished : a.rows % a.rows_streams != 0))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(repeat_kernel, dim3(a.rows), dim3(kRepeatMaxHist), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_repeat_logits(float* logits, int V, int rows, const int* hist, int ld, const int* n_hist, const int* tab, hipStream_t st) {
  if (rows < 1 || rows > 64 || V < 1 || ld < 0 || !logits || !hist || !n_hist || !tab) return hipErrorInvalidValue;
  hipLaunchKernelGGL(repeat_logits_kernel, dim3(rows), dim3(kRepeatMaxHist), 0, st, logits, V, hist, ld, n_hist, tab);
  return hipGetLastError();
}

hipError_t launch_lang_detect(const float* logits, int V, int rows, const int* ids, int n_lang, int* out_id, float* out_prob, hipStream_t st) {
  if (rows < 1 || V < 1 || n_lang < 1 || n_lang > kLangMax || !logits || !ids || !out_id) return hipErrorInvalidValue;
  hipLaunchKernelGGL(lang_detect_kernel, dim3(rows), dim3(64), 0, st, logits, V, ids, n_lang, out_id, out_prob);
  return hipGetLastError();
}

hipError_t launch_advance(DecState* stt, int n, hipStream_t st) {
  hipLaunchKernelGGL(advance_kernel, dim3(1), dim3(1), 0, st, stt, n);
  return hipGetLastError();
}

hipError_t launch_beam_step(const BeamArgs& a0, bool in_prompt, hipStream_t st) {
  const SamplerArgs& s = a0.s;
  if (a0.K < 2 || a0.K > kBeamMax || a0.n_clips < 1 || s.B != a0.n_clips * a0.K || s.B > 64 || s.seq_ld > kBeamSeqMax || s.rows_streams != 0 ||
      !s.logits || !s.seq || !s.cur_ids || !s.finished || !s.last_ts || !s.stt || !s.suppress_bits || !a0.parts || !a0.run_score ||
      !a0.fin_seq || !a0.fin_score || !a0.fin_flag || !a0.fin_len || !a0.open || !a0.done || !a0.beam_idx || !a0.pen)
    return hipErrorInvalidValue;
  BeamArgs a = a0;
  a.s.n_slices = 32;   // the slicing of launch_sampler whatever the number of rows: a row's partials, and the order they are merged in
  if (!in_prompt) {    // (host-known: while the prompt lasts nothing is selected)
    hipLaunchKernelGGL((beam_part_kernel<32, 4>), dim3(32, s.B), dim3(256), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(beam_finish_kernel, dim3(a.n_clips), dim3(512), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_beam_reorder(int dtype, void* kc, void* vc, long long layer_stride, long long bstride, long long hstride, int Ld, int H,
                               int key_bound, const BeamArgs& a, hipStream_t st) {
  const int E = dtype == 0 ? 4 : 8;   // elements per 16-byte vector
  const int kb = (key_bound + 63) / 64 * 64;
  if (a.K < 2 || a.K > kBeamMax || a.n_clips < 1 || a.n_clips * a.K > 64 || kb < 64 || hstride < (long long)kb * 64 || layer_stride % E != 0 ||
      bstride % E != 0 || hstride % E != 0 || !kc || !vc || !a.beam_idx || !a.done || !a.s.stt)
    return hipErrorInvalidValue;
  const dim3 grid(kb / 64, H, Ld * 2 * a.n_clips);
  if (dtype == 0) hipLaunchKernelGGL(beam_reorder_kernel<4>, grid, dim3(256), 0, st, (u32x4_t*)kc, (u32x4_t*)vc, layer_stride / E, bstride / E, hstride / E, a);
  else hipLaunchKernelGGL(beam_reorder_kernel<2>, grid, dim3(256), 0, st, (u32x4_t*)kc, (u32x4_t*)vc, layer_stride / E, bstride / E, hstride / E, a);
  return hipGetLastError();
}

hipError_t launch_beam_cross_copy(void* ck, void* cv, long long layer_bytes, long long slot_bytes, int Ld, int n_clips, int K, hipStream_t st) {
  if (!ck || !cv || layer_bytes % 16 != 0 || slot_bytes % 16 != 0 || slot_bytes < 16 || n_clips < 1 || K < 2 || (long long)n_clips * K * slot_bytes > layer_bytes)
    return hipErrorInvalidValue;
  const long long slot_vec = slot_bytes / 16;
  hipLaunchKernelGGL(beam_cross_copy_kernel, dim3((unsigned)((slot_vec + 1023) / 1024), (K - 1) * n_clips, Ld * 2), dim3(256), 0, st, (u32x4_t*)ck,
                     (u32x4_t*)cv, layer_bytes / 16, slot_vec, n_clips);
  return hipGetLastError();
}

hipError_t launch_beam_align_gather(float* align, int Ha, int P, int T, int n_pos, const BeamArgs& a, hipStream_t st) {
  if (!align || !a.back || !a.fin_last || !a.fin_len || !a.fin_score || !a.s.stt || Ha < 1 || T < 1 || a.K < 2 || a.K > kBeamMax ||
      a.n_clips < 1 || a.n_clips * a.K > 64 || n_pos < 1 || n_pos >= P || P > kBeamSeqMax || a.max_len != n_pos + 1)
    return hipErrorInvalidValue;
  const dim3 grid((n_pos + kAlignGatherPos - 1) / kAlignGatherPos, Ha, a.n_clips);
  if (T % 4 == 0 && (reinterpret_cast<uintptr_t>(align) & 15) == 0)
    hipLaunchKernelGGL(beam_align_gather_kernel<4>, grid, dim3(256), 0, st, align, Ha, P, T, n_pos, a);
  else
    hipLaunchKernelGGL(beam_align_gather_kernel<1>, grid, dim3(256), 0, st, align, Ha, P, T, n_pos, a);
  return hipGetLastError();
}

hipError_t launch_tile_weights(int dtype, const void* src, void* dst, int N, int K, int tr, hipStream_t st) {
  const int E = dtype == 0 ? 4 : 8;
  if (K % (4 * E) != 0 || (tr != 16 && tr != 8 && tr != 4) || N % tr != 0 && tr != 16) return hipErrorInvalidValue;
  const long long total = (long long)((N + tr - 1) / tr) * (K / E / 4) * 4 * tr;
  dim3 grid((unsigned)((total + 255) / 256));
  if (dtype != 0) hipLaunchKernelGGL(tile_weights_kernel<bf16_t>, grid, dim3(256), 0, st, (const bf16_t*)src, (bf16_t*)dst, N, K, tr);   // a pure copy: bf16 and f16 alike
  else hipLaunchKernelGGL(tile_weights_kernel<float>, grid, dim3(256), 0, st, (const float*)src, (float*)dst, N, K, tr);
  return hipGetLastError();
}

hipError_t launch_quant_mx8(const void* src_bf16, void* dst_fp8, void* dst_scales, int N, int K, int tr, hipStream_t st) {
  if (K % 128 != 0 || (tr != 16 && tr != 8) || (tr == 8 && N % 16 != 0)) return hipErrorInvalidValue;
  const long long total = (long long)((N + 15) / 16) * (K / 128) * 64;
  hipLaunchKernelGGL(quant_mx8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const bf16_t*)src_bf16,
                     (unsigned char*)dst_fp8, (unsigned char*)dst_scales, N, K, tr);
  return hipGetLastError();
}

hipError_t launch_compose(int dtype, const void* A, const void* Bm, const void* bvec, void* out, float* c0, int N, int J, int K,
                          hipStream_t st) {
  const dim3 grid((K + 15) / 16, (N + 15) / 16);
  TW_DISPATCH3(dtype, T, hipLaunchKernelGGL(compose_kernel<T>, grid, dim3(256), 0, st, (const T*)A, (const T*)Bm, (const T*)bvec, (T*)out, c0, N, J, K));
  return hipGetLastError();
}

hipError_t launch_fold_ln(int dtype, void* W, const void* Wsrc, const void* g, const void* beta, const void* bias, float* gw,
                          float* cb, int N, int K, hipStream_t st) {
  dim3 grid((N + 3) / 4);
  TW_DISPATCH3(dtype, T, hipLaunchKernelGGL(fold_ln_kernel<T>, grid, dim3(256), 0, st, (T*)W, (const T*)Wsrc, (const T*)g, (const T*)beta,
                                             (const T*)bias, gw, cb, N, K));
  return hipGetLastError();
}
