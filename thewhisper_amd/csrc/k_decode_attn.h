// Device helpers shared by the decode kernels of k_decode.hip, k_decode_kv8_rows.hip, k_decode_kv8_beams.hip and k_decode_beam_cross.hip: operand packing, the
// MFMA wrapper, the e4m3 widening, the fused cross-attention query, the shared pieces of the attention kernels (row map, LDS layout
// of the rows flavours) and the launchers' dispatch helpers.  Each translation unit gets its own
// copies (anonymous namespace, device code all forceinline).
#pragma once
#include <type_traits>
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

// ---- pieces shared by the attention kernels (dec_self_attn, dec_cross_attn and their kv8 / rows / beams flavours) ----

// attn_row_map: launch row b -> the stream whose cache it attends to and the number of keys it sees.  Two policies; the trailing
// kernel argument is the policy's Arg.
//  * AttnRowsMap (int rows_streams): 0 = plain, row b is stream b at stt->pos; > 0 = rows mode (prefill), row b is position
//    pos + b / rows_streams of stream b % rows_streams (causal inside the launch).  The addresses depend on kernel arguments only.
//  * AttnRaggedMap (const int* n_pad; tw_common.h: tw_row_pos): stream b sees the keys [0, q] of its ROW position q <= pos < key_bound;
//    the keys between q and the bucket's end are masked like the ones behind pos, and masked keys contribute exact zeros.
struct AttnRowsMap {
  using Arg = int;
  static __device__ __forceinline__ int stream(int b, int rs) { return rs > 0 ? b % rs : b; }
  static __device__ __forceinline__ int pos(int p, int b, int rs) { return p + (rs > 0 ? b / rs : 0); }
};
struct AttnRaggedMap {
  using Arg = const int* __restrict__;
  static __device__ __forceinline__ int stream(int b, const int*) { return b; }
  static __device__ __forceinline__ int pos(int p, int b, const int* n_pad) { return tw_row_pos(p, n_pad[b]); }
};

// Score rows (= columns that are computed to the end) of the beams mode below: a clip has at most kBeamMax = 8 beams
constexpr int kBeamCols = 8;

// LDS (dynamic) of the rows and beams flavours, 8 wavefronts, NC columns, query elements of ESZ bytes:
//   scores float[NC][Tp + 4] | partial context vectors float[8][NC][68] | column max float[8][16] | normaliser float[8][NC] |
//   query rows [NC][64] x ESZ.  Offsets in floats from the start: the launchers size the launch and the cap from it, the kernels carve
//   their pointers as one chain in this order.
template <int NC, int ESZ>
struct RowsLds {
  static constexpr int NW = 8, WS = 68;
  static constexpr __host__ __device__ int wo(int Tp) { return NC * (Tp + 4); }
  static constexpr __host__ __device__ int redm(int Tp) { return wo(Tp) + NW * NC * WS; }
  static constexpr __host__ __device__ int wl(int Tp) { return redm(Tp) + NW * 16; }
  static constexpr __host__ __device__ int qst(int Tp) { return wl(Tp) + NW * NC; }
  static constexpr __host__ __device__ size_t bytes(int Tp) { return (size_t)qst(Tp) * sizeof(float) + NC * 64 * ESZ; }
  static constexpr int cap = (int)bytes(1536);   // Tp <= 1536: launch_dec_cross_attn
  static_assert(cap <= 160 * 1024, "LDS of a compute unit");
};

// ---- launcher side ----
// a run-time bool / small int as a compile-time constant: f(std::bool_constant) / f(std::integral_constant), which returns hipError_t
template <typename F> hipError_t tw_with_bool(bool v, F&& f) { return v ? f(std::true_type{}) : f(std::false_type{}); }
template <int... Vs, typename F> hipError_t tw_with_int(int v, F&& f) {
  hipError_t e = hipErrorInvalidValue;   // v is none of Vs
  (void)((v == Vs && ((e = f(std::integral_constant<int, Vs>{})), true)) || ...);
  return e;
}
// launch a kernel whose dynamic LDS exceeds the 64-KiB default: the attribute is set once per instantiation
template <auto Kernel, int Cap, typename... A>
hipError_t tw_launch_big_lds(dim3 grid, dim3 block, size_t lds, hipStream_t st, A... args) {
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, Cap);
  if (attr != hipSuccess) return attr;
  hipLaunchKernelGGL(Kernel, grid, block, lds, st, args...);
  return hipGetLastError();
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
// LDS (dynamic): RowsLds<16, sizeof(T)> - 71 KiB at Tp = 512 (two workgroups per CU), 135 KiB at Tp = 1536 (one).
//
// BEAMS (a step of tw_generate_beam; grid (heads, n_clips, 1), rows_streams = n_clips, n_pos = K <= kBeamCols): the columns of a
// workgroup are not consecutive positions of a stream but the K beams of clip `srow` at the SAME position.  Beam j is launch row
// srow + j * n_clips - the row map above with p0 = 0 - and every one of them reads the K / V^T of slot srow, so a clip's cross K / V
// is streamed once per (layer, head, step) whatever K is, and the slots behind the clips are neither read nor written.  What differs:
//  * the alignment side output of column j is the softmax row of SLOT r_j = srow + j * n_clips at position stt->pos (the beam's row,
//    where tw_generate_beam_aligned's gather expects it), not (srow, pos + j);
//  * NC = kBeamCols columns instead of 16 are carried behind the score MFMAs: score rows, exponentials, normalisers, partial context
//    vectors and query rows exist for columns 0 .. 7 only, and the P.V operand of column fr >= 8 is column fr - 8's (an MFMA column
//    nobody reads).  LDS: 36.7 KiB at Tp = 512, 69 KiB at Tp = 1536 in float32, and half the expf of the 16-column layout.
// Columns K .. 7 repeat beam K - 1 and are not written.  Every column that is written runs the expression tree above, operation for
// operation, so a beam's context vector and alignment row keep the bits of the one-row kernel.
template <typename T, bool SINGLE, bool FQ, bool BEAMS = false>
__global__ __launch_bounds__(512) void dec_cross_attn_rows_kernel(const T* __restrict__ ck, const T* __restrict__ cv, int H, int Tp,
                                                                   int Tlen, int rows_streams, int n_pos, const T* __restrict__ q,
                                                                   T* __restrict__ out, const int* __restrict__ align_slot,
                                                                   float* __restrict__ align, int Ha, int P,
                                                                   const DecState* __restrict__ stt, FusedQ fq) {
  constexpr int NW = 8, WS = 68;
  constexpr int NC = BEAMS ? kBeamCols : 16;    // columns with score rows, normalisers and partial context vectors
  constexpr int E = ElemTraits<T>::kPer16B;
  constexpr int DS = 64 / (4 * E);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int S = Tp + 4;                         // carved in the order of RowsLds<NC, sizeof(T)>
  float* sc = reinterpret_cast<float*>(smem);   // [NC][S] scores -> unnormalised probabilities
  float* wo = sc + NC * S;                      // [NW][NC][WS]
  float* redm = wo + NW * NC * WS;              // [NW][16]
  float* wl = redm + NW * 16;                   // [NW][NC]
  T* qst = reinterpret_cast<T*>(wl + NW * NC);  // [NC][64]
  const int h = blockIdx.x, srow = blockIdx.y, p0 = BEAMS ? 0 : blockIdx.z * 16;
  const int nc = min(NC, n_pos - p0);           // columns in use
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, kq = lane >> 4;
  const int fc = fr & (NC - 1);                 // the column whose LDS rows lane (fr, .) reads: fr itself in the rows flavour
  const bool own = NC == 16 || fr < NC;         // lane's MFMA column is one of the NC
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
    // the group's query rows, once per workgroup: wavefront w builds the rows of columns w and (rows flavour) w + 8
    QRaw<T> qr[NC / 8];
#pragma unroll
    for (int i = 0; i < NC / 8; ++i) fq_request<T>(qr[i], fq, row_of(wave + 8 * i), h, lane);
    if (SINGLE) load_v(wave);
#pragma unroll
    for (int i = 0; i < NC / 8; ++i) fq_finish<T>(qr[i], fq, lane, qst + (wave + 8 * i) * 64);
    __syncthreads();
#pragma unroll
    for (int ds = 0; ds < DS; ++ds) qf[ds] = *reinterpret_cast<const u32x4_t*>(qst + fc * 64 + ds * 4 * E + kq * E);
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
      if (own && g64 * 64 < n_bound) *reinterpret_cast<f32x4_t*>(sc + fr * S + g64 * 64 + a * 16 + kq * 4) = sv4;
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
  float ls[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) ls[j] = 0.f;
  for (int c = 0; c < n_chunks; ++c) {
    const int g64 = c * NW + wave;
    if (!SINGLE) load_v(g64);
    const int t0 = g64 * 64 + lane;  // one key per lane
#pragma unroll
    for (int j = 0; j < NC; ++j) {
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
        pv[e] = (t < n_bound) ? sc[fc * S + t] : 0.f;  // same wavefront wrote these: LDS operations of a wavefront stay in order
      }
      const u32x4_t pf = pack16<T>(pv);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) o[dt] = sk_mfma<T>(vfr[ks * 4 + dt], pf, o[dt]);
    }
  }
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    // lane 0's sum, as in the single-query kernel: tw_wave_sum adds the four quads of a row in another order in odd quads
    // than in even ones, so the lanes of a wavefront do not all hold the same bits
    const float l = tw_wave_sum(ls[j]);
    if (lane == 0) wl[wave * NC + j] = l;
  }
  if (own) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) *reinterpret_cast<f32x4_t*>(wo + (wave * NC + fr) * WS + dt * 16 + kq * 4) = o[dt];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NC / 8; ++i) {   // NC columns x 64 dims over 512 threads
    const int j = (tid >> 6) + 8 * i, k = tid & 63;
    float L = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) L += wl[w * NC + j];
    const float inv = 1.0f / L;
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) v += wo[(w * NC + j) * WS + k];
    if (j < nc) {
      const int b = srow + (p0 + j) * rows_streams;
      out[(long long)(b >> 4) * 16 * H * 64 + tw_xt_index<T>(b & 15, h * 64 + k)] = (T)(v * inv);
    }
  }
  const int slot = align_slot ? align_slot[h] : -1;
  if (slot >= 0) {  // A11 side output: every column writes the softmax row of its own (stream, position) - BEAMS: (beam's row, pos)
    const int pos = stt->pos;
    for (int j = 0; j < nc; ++j) {
      float L = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) L += wl[w * NC + j];
      const float inv = 1.0f / L;
      float* row = BEAMS ? align + (((long long)(srow + j * rows_streams) * Ha + slot) * P + pos) * Tlen
                         : align + (((long long)srow * Ha + slot) * P + pos + p0 + j) * Tlen;
      for (int t = tid; t < Tlen; t += 512) row[t] = sc[j * S + t] * inv;
    }
  }
}

}  // namespace
