// Device helpers shared by the decode kernels of k_decode.hip and k_decode_kv8_rows.hip: operand packing, the MFMA wrapper, the e4m3
// widening and the fused cross-attention query.  Each translation unit gets its own copies (anonymous namespace, all forceinline).
#pragma once
#include "tw_common.h"

namespace {

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

// 16 e4m3 bytes -> two MFMA operands of T (bytes 0..7, 8..15), each value multiplied by X = 2^(scale byte - 127); one byte pair per
// v_cvt_scalef32_pk_bf16_fp8 / v_cvt_scalef32_pk_f16_fp8.  bf16: exact (3 mantissa bits times a power of two).
// float16 (TW_F16_W8A16): the convert returns RNE_f16(value x X) with gradual underflow and +-inf above the float16 range (all 256
// bytes x 254 scale bytes against the float32 widening followed by a float16 cast: profiles/r24_f16cvt_probe.txt, tools/dbg/
// f16cvt_probe.hip), so the weight a row sees is the pure function  w(byte, sb) = RNE_f16(e4m3(byte) x 2^(sb-127))  of the stored bytes.
// With sb = max(E - 7, 1) every element is a multiple of 2^(E-143): the product is EXACT for every block whose largest magnitude is
// >= 2^-8 (E >= 119) - up to the top of the range, because the packers clamp to 63488 (sk_quant_mx8) and 248 x 2^8 is the largest
// image.  In a block of smaller weights the elements below 2^-14 land on the float16 subnormal grid (|error| <= 2^-25) and those
// below 2^-25 vanish.  The float16 MFMA takes subnormal operands as they are (same probe: 2^-24 x 1024 = 2^-14).
template <typename T, bool HI> __device__ __forceinline__ unsigned sk_cvt8_pair(unsigned src, float X) {
  if constexpr (ElemTraits<T>::kCode == 2) return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)src, X, HI));
  else return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)src, X, HI));
}
template <typename T> __device__ __forceinline__ void sk_widen8(const u32x4_t& raw, float X, u32x4_t& lo, u32x4_t& hi) {
  lo[0] = sk_cvt8_pair<T, false>(raw[0], X);
  lo[1] = sk_cvt8_pair<T, true>(raw[0], X);
  lo[2] = sk_cvt8_pair<T, false>(raw[1], X);
  lo[3] = sk_cvt8_pair<T, true>(raw[1], X);
  hi[0] = sk_cvt8_pair<T, false>(raw[2], X);
  hi[1] = sk_cvt8_pair<T, true>(raw[2], X);
  hi[2] = sk_cvt8_pair<T, false>(raw[3], X);
  hi[3] = sk_cvt8_pair<T, true>(raw[3], X);
}

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

}  // namespace
