// Rows flavour of the fp8 contexts' decoder cross attention (launch_dec_cross_attn's fp8 branch, rows mode with several positions per
// stream).  A translation unit of its own: it is built without the packed float32 instructions (thewhisper_amd/build.py: FILE_FLAGS),
// the older sources keep the flags their code objects were measured with.  The device helpers are k_decode.hip's (k_decode_attn.h).
#include "tw_common.h"
#include "k_decode_attn.h"

namespace {

// Rows flavour of dec_cross_attn_kv8_kernel (fp8 contexts, rows mode with more than one position per stream), the split of
// dec_cross_attn_rows_kernel: one workgroup of 8 wavefronts per (stream, head, group of up to 16 of the stream's positions), column j
// of the MFMA B operands = launch row srow + (16 g + j) * rows_streams, so ONE pass over the head's e4m3 K / V^T and their scale
// bytes serves 16 queries with the sk_mfma instructions the single-query kernel spends on one.  As in attn_mfma_block_kv8 every raw
// fragment of the head (G x 4 K tiles, G x 4 V^T tiles, the scale bytes) is requested before anything is waited for, and widened in
// registers (sk_widen8<T>: the K scale goes into the convert, lane = key; V^T unscaled).
// A column runs the single-query kernel's expression tree - column max over the kq lane groups, then over the wavefronts in index
// order; expf(sc - M), one key per lane; lane 0's tw_wave_sum, then the wavefronts in index order; the P.V operand is probability x
// 2^(V scale) (float16: x 2^7 more, taken back in float32: kPvUp), rounded by pack16; partial context vectors added over the
// wavefronts in index order, then x 1/L - so a row's bits are the one-position step's.
// The scaled operand is NOT stored (the single-query kernel's second array, scv): it is the exact float32 product of the stored
// probability and a power of two, so it is formed where the operand is gathered - lane (fr, kq) holds the 16 V-scale bytes of the
// keys kq * 16 .. + 15 of each of its groups in registers (one 16-byte request per group, the same for the 16 columns).
// Columns behind the group's last position repeat that position's query, stop behind the scores (no exponentials, no normaliser:
// a column of an MFMA depends on its own B column only) and are not written.
// LDS (dynamic): RowsLds<16, 2> (k_decode_attn.h) - 69.3 KiB at Tp = 512 (two workgroups per CU), 133.3 KiB at Tp = 1536 (one).
template <typename T, int G, bool FQ>
__global__ __launch_bounds__(512) void dec_cross_attn_kv8_rows_kernel(const unsigned char* __restrict__ ck, const unsigned char* __restrict__ cv,
                                                                       const unsigned char* __restrict__ ksc,
                                                                       const unsigned char* __restrict__ vsc, int H, int Tp, int Tlen,
                                                                       int rows_streams, int n_pos, const T* __restrict__ q,
                                                                       T* __restrict__ out, const int* __restrict__ align_slot,
                                                                       float* __restrict__ align, int Ha, int P,
                                                                       const DecState* __restrict__ stt, FusedQ fq) {
  constexpr int NW = 8, WS = 68;
  constexpr bool kPvUp = ElemTraits<T>::kCode == 2;   // float16: the P.V operand is carried times 2^7 (attn_mfma_block_kv8)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  asm volatile("" ::"s"(ck), "s"(cv), "s"(ksc), "s"(vsc), "s"(H), "s"(Tp), "s"(Tlen), "s"(rows_streams), "s"(n_pos));
  const int S = Tp + 4;                         // carved in the order of RowsLds<16, 2>
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
  const long long hb = ((long long)srow * H + h) * Tp;
  const unsigned char* kf8 = ck + hb * 64;
  const unsigned char* vtf8 = cv + hb * 64;
  const int n_keys = Tlen, n_bound = Tp;
  const int last64 = n_bound / 64 - 1;
  auto row_of = [&](int j) { return srow + (p0 + min(j, nc - 1)) * rows_streams; };   // launch row of column j

  u32x4_t qf[2], kraw[G][4], vraw[G][4], vs16[G];
  unsigned ks4[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {  // 64 keys = 4 tiles of 1 KiB + their 64 scale bytes ([group][key % 16][tile]: one 32-bit load)
    const int gi = min(g * NW + wave, last64);
    const unsigned char* p = kf8 + ((long long)gi * 4 * 64 + lane) * 16;
#pragma unroll
    for (int a = 0; a < 4; ++a) kraw[g][a] = *reinterpret_cast<const u32x4_t*>(p + a * 1024);
    ks4[g] = *reinterpret_cast<const unsigned*>(ksc + hb + gi * 64 + fr * 4);
  }
  __builtin_amdgcn_sched_barrier(0);
  // the query side behind the K requests (see attn_mfma_block)
  asm volatile("" ::"s"(q), "s"(fq.u), "s"(fq.stats), "s"(fq.n_part), "s"(fq.gw), "s"(fq.cb), "s"(fq.d));
  QRaw<T> qr[2];
  if constexpr (FQ) {
    // the group's query rows, once per workgroup: wavefront w builds the rows of columns w and w + 8
#pragma unroll
    for (int i = 0; i < 2; ++i) fq_request<T>(qr[i], fq, row_of(wave + 8 * i), h, lane);
  } else {
    const T* qrow = q + ((long long)row_of(fr) * H + h) * 64;
    qf[0] = *reinterpret_cast<const u32x4_t*>(qrow + kq * 16);
    qf[1] = *reinterpret_cast<const u32x4_t*>(qrow + kq * 16 + 8);
  }
#pragma unroll
  for (int g = 0; g < G; ++g) {  // 64 keys x 64 dims = 4 dim tiles of 1 KiB; lane (., kq) also fetches the V scales of the keys it gathers
    const int gi = min(g * NW + wave, last64);
    const unsigned char* p = vtf8 + ((long long)gi * 4 * 64 + lane) * 16;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) vraw[g][dt] = *reinterpret_cast<const u32x4_t*>(p + dt * 1024);
    vs16[g] = *reinterpret_cast<const u32x4_t*>(vsc + hb + gi * 64 + kq * 16);
  }
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (FQ) {
#pragma unroll
    for (int i = 0; i < 2; ++i) fq_finish<T>(qr[i], fq, lane, qst + (wave + 8 * i) * 64);
    __syncthreads();
    qf[0] = *reinterpret_cast<const u32x4_t*>(qst + fr * 64 + kq * 16);
    qf[1] = *reinterpret_cast<const u32x4_t*>(qst + fr * 64 + kq * 16 + 8);
  }

  // ---- scores: lane (fr, kq) holds keys kq * 4 + r of the tile for column fr ----
  float m = -1.0e30f;
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int g64 = g * NW + wave;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      u32x4_t k0, k1;
      sk_widen8<T>(kraw[g][a], __builtin_bit_cast(float, ((ks4[g] >> (8 * a)) & 0xffu) << 23), k0, k1);
      f32x4_t acc = f32x4_t{0.f, 0.f, 0.f, 0.f};
      acc = sk_mfma<T>(k0, qf[0], acc);
      acc = sk_mfma<T>(k1, qf[1], acc);
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
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int g64 = g * NW + wave;
    const int t0 = g64 * 64 + lane;  // one key per lane
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float M = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, Mc), j));
      float pr = 0.f;
      if (j < nc && t0 < n_bound) {   // (a column behind the group's last position is never written: its exponentials are not taken)
        pr = (t0 < n_keys) ? expf(sc[j * S + t0] - M) : 0.f;
        sc[j * S + t0] = pr;   // plain probability: alignment rows, normaliser, and - times the key's V scale - the P.V operand
      }
      ls[j] += pr;
    }
    u32x4_t v0[4], v1[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) sk_widen8<T>(vraw[g][dt], 1.0f, v0[dt], v1[dt]);
#pragma unroll
    for (int j2 = 0; j2 < 2; ++j2) {   // operand j2 of lane (fr, kq): keys kq*16 + j2*8 .. +7 of this 64-key group, column fr
      const unsigned sb_lo = j2 == 0 ? vs16[g][0] : vs16[g][2];   // scale bytes of keys +0..3
      const unsigned sb_hi = j2 == 0 ? vs16[g][1] : vs16[g][3];   //                      +4..7
      float pv[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int t = g64 * 64 + kq * 16 + j2 * 8 + e;
        const unsigned sb = ((e < 4 ? sb_lo : sb_hi) >> (8 * (e & 3))) & 0xffu;
        // same wavefront wrote the probabilities: LDS operations of a wavefront stay in order
        pv[e] = (t < n_bound) ? sc[fr * S + t] * __builtin_bit_cast(float, (sb + (kPvUp ? 7u : 0u)) << 23) : 0.f;
      }
      const u32x4_t pf = pack16<T>(pv);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) o[dt] = sk_mfma<T>(j2 == 0 ? v0[dt] : v1[dt], pf, o[dt]);
    }
  }
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    // lane 0's sum, as in the single-query kernel (see dec_cross_attn_rows_kernel)
    if (j < nc) {
      const float l = tw_wave_sum(ls[j]);
      if (lane == 0) wl[wave * 16 + j] = l;
    }
  }
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) *reinterpret_cast<f32x4_t*>(wo + (wave * 16 + fr) * WS + dt * 16 + kq * 4) = o[dt];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 2; ++i) {   // 16 columns x 64 dims over 512 threads
    const int j = (tid >> 6) + 8 * i, k = tid & 63;   // (j is uniform in a wavefront)
    if (j < nc) {   // a column behind the last position has no normaliser
      float L = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) L += wl[w * 16 + j];
      const float inv = 1.0f / L;
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) v += wo[(w * 16 + j) * WS + k];
      const int b = srow + (p0 + j) * rows_streams;
      T* dst = out + (long long)(b >> 4) * 16 * H * 64 + tw_xt_index<T>(b & 15, h * 64 + k);
      if constexpr (kPvUp) *dst = tw_cast<T>(v * inv * 0.0078125f);
      else *dst = (T)(v * inv);
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

}  // namespace

// Reached through launch_dec_cross_attn only, which has made every check (dtype 1 or 2, B a multiple of rows_streams, Tp <= 1536)
// and reports the grid.
hipError_t launch_dec_cross_attn_kv8_rows(int dtype, const void* q, const FusedQ& fq, const void* ck, const void* cv, void* out, int B, int H,
                                          int T, int Tp, const int* align_slot_for_head, float* align, int Ha, int P, const DecState* stt,
                                          const unsigned char* ksc, const unsigned char* vsc, int rows_streams, hipStream_t st) {
  const int n_pos = B / rows_streams;
  const dim3 grid(H, rows_streams, (n_pos + 15) / 16);
  using Lds = RowsLds<16, 2>;
  return tw_with_bool(dtype == 1, [&](auto is_bf16) {   // fp8 caches: bf16 or float16 activations
    using TT = std::conditional_t<is_bf16(), bf16_t, f16_t>;
    return tw_with_int<1, 2, 3>(Tp <= 512 ? 1 : (Tp <= 1024 ? 2 : 3), [&](auto g) {
      return tw_with_bool(fq.u != nullptr, [&](auto f) {
        return tw_launch_big_lds<&dec_cross_attn_kv8_rows_kernel<TT, g(), f()>, Lds::cap>(
            grid, dim3(512), Lds::bytes(Tp), st, (const unsigned char*)ck, (const unsigned char*)cv, ksc, vsc, H, Tp, T, rows_streams, n_pos,
            (const TT*)q, (TT*)out, align_slot_for_head, align, Ha, P, stt, fq);
      });
    });
  });
}
