// Beams mode of the fp8 contexts' decoder cross attention (launch_dec_cross_attn's fp8 branch with beam_clips > 0: a step of
// tw_generate_beam in a TW_F16_W8A16 context).  A translation unit of its own: it is built without the packed float32 instructions
// (thewhisper_amd/build.py: FILE_FLAGS), the older sources keep the flags their code objects were measured with.  The device helpers
// are k_decode.hip's (k_decode_attn.h).
#include "tw_common.h"
#include "k_decode_attn.h"

static_assert(kBeamMax <= kBeamCols, "a clip's beams are the columns of one workgroup");

namespace {

// Beams flavour of dec_cross_attn_kv8_kernel: what the BEAMS mode of dec_cross_attn_rows_kernel is to dec_cross_attn_kernel, with the
// data movement of dec_cross_attn_kv8_rows_kernel.  Grid (heads, n_clips, 1), one workgroup of 8 wavefronts per (head h, clip c):
// column j < K of the MFMA B operands is launch row c + j * n_clips (beam j of the clip, the beam-major row map of tw_generate_beam) and
// EVERY column reads the e4m3 K, the e4m3 V^T and the two scale-byte arrays of slot c - one pass over a clip's K / V^T per (layer,
// head, step) serves all K beams, and no slot behind n_clips is read or written.
// Every raw fragment of the head (G x 4 K tiles and their scale words, G x 4 V^T tiles and the 16 V-scale bytes of the keys a lane
// gathers) is requested before anything is waited for, the query side stands behind the K requests (FQ: wavefront w forms the fused
// query row of column w in LDS, once per workgroup; !FQ: the rows are loaded), and the fragments are widened in registers
// (sk_widen8<T>: the K scale goes into the convert, lane = key; V^T unscaled).  The P.V operand is formed where it is gathered:
// probability x 2^(V scale), float16: x 2^7 more, taken back in float32 (kPvUp).
// Only kBeamCols = 8 columns are carried behind the score MFMAs: score rows, exponentials, normalisers, partial context vectors and
// query rows exist for columns 0 .. 7, and the P.V operand of column fr >= 8 is column fr - 8's (an MFMA column nobody reads).
// Columns K .. 7 repeat beam K - 1, stop behind the scores (no exponentials, no normaliser) and are not written.
// A written column runs the single-query kernel's expression tree, operation for operation - column max over the kq lane groups,
// then over the wavefronts in index order; expf(sc - M), one key per lane; lane 0's tw_wave_sum, then the wavefronts in index order;
// the operand rounded by pack16; partial context vectors added over the wavefronts in index order, then x 1/L (float16: x 2^-7) -
// so a beam's context vector and alignment row keep the bits dec_cross_attn_kv8_kernel gives that row alone.
// Alignment side output: column j writes the softmax row of SLOT c + j * n_clips at position stt->pos (the beam's own row, where
// beam_align_gather_kernel expects it).
// LDS (dynamic): RowsLds<kBeamCols, 2> (k_decode_attn.h) - 34.9 KiB at Tp = 512, 50.9 KiB at Tp = 1024, 66.9 KiB at Tp = 1536.
template <typename T, int G, bool FQ>
__global__ __launch_bounds__(512) void dec_cross_attn_kv8_beams_kernel(const unsigned char* __restrict__ ck, const unsigned char* __restrict__ cv,
                                                                        const unsigned char* __restrict__ ksc,
                                                                        const unsigned char* __restrict__ vsc, int H, int Tp, int Tlen,
                                                                        int n_clips, int K, const T* __restrict__ q, T* __restrict__ out,
                                                                        const int* __restrict__ align_slot, float* __restrict__ align,
                                                                        int Ha, int P, const DecState* __restrict__ stt, FusedQ fq) {
  constexpr int NW = 8, WS = 68, NC = kBeamCols;
  constexpr bool kPvUp = ElemTraits<T>::kCode == 2;   // float16: the P.V operand is carried times 2^7 (attn_mfma_block_kv8)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  asm volatile("" ::"s"(ck), "s"(cv), "s"(ksc), "s"(vsc), "s"(H), "s"(Tp), "s"(Tlen), "s"(n_clips), "s"(K));
  const int S = Tp + 4;                         // carved in the order of RowsLds<NC, 2>
  float* sc = reinterpret_cast<float*>(smem);   // [NC][S] scores -> unnormalised probabilities
  float* wo = sc + NC * S;                      // [NW][NC][WS]
  float* redm = wo + NW * NC * WS;              // [NW][16]
  float* wl = redm + NW * 16;                   // [NW][NC]
  T* qst = reinterpret_cast<T*>(wl + NW * NC);  // [NC][64]
  const int h = blockIdx.x, clip = blockIdx.y;
  const int nc = min(NC, K);                    // columns in use: the clip's beams
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, kq = lane >> 4;
  const int fc = fr & (NC - 1);                 // the column whose LDS rows lane (fr, .) reads
  const bool own = fr < NC;                     // lane's MFMA column is one of the NC
  const long long hb = ((long long)clip * H + h) * Tp;   // slot `clip`, whatever the column
  const unsigned char* kf8 = ck + hb * 64;
  const unsigned char* vtf8 = cv + hb * 64;
  const int n_keys = Tlen, n_bound = Tp;
  const int last64 = n_bound / 64 - 1;
  auto row_of = [&](int j) { return clip + min(j, nc - 1) * n_clips; };   // launch row of column j: beam j of the clip

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
  QRaw<T> qr;
  if constexpr (FQ) {
    fq_request<T>(qr, fq, row_of(wave), h, lane);   // the clip's query rows, once per workgroup: wavefront w builds the row of column w
  } else {
    const T* qrow = q + ((long long)row_of(fc) * H + h) * 64;
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
    fq_finish<T>(qr, fq, lane, qst + wave * 64);
    __syncthreads();
    qf[0] = *reinterpret_cast<const u32x4_t*>(qst + fc * 64 + kq * 16);
    qf[1] = *reinterpret_cast<const u32x4_t*>(qst + fc * 64 + kq * 16 + 8);
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
      if (own && g64 * 64 < n_bound) *reinterpret_cast<f32x4_t*>(sc + fr * S + g64 * 64 + a * 16 + kq * 4) = sv4;
    }
  }
  m = tw_xor32_max(tw_xor16_max(m));
  if (kq == 0) redm[wave * 16 + fr] = m;
  __syncthreads();
  float Mc = redm[fr];   // lane's column
#pragma unroll
  for (int w = 1; w < NW; ++w) Mc = fmaxf(Mc, redm[w * 16 + fr]);

  // ---- probabilities of this wavefront's own keys, every beam, and P.V ----
  f32x4_t o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float ls[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) ls[j] = 0.f;
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int g64 = g * NW + wave;
    const int t0 = g64 * 64 + lane;  // one key per lane
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const float M = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, Mc), j));
      float pr = 0.f;
      if (j < nc && t0 < n_bound) {   // (a column behind the last beam is never written: its exponentials are not taken)
        pr = (t0 < n_keys) ? expf(sc[j * S + t0] - M) : 0.f;
        sc[j * S + t0] = pr;   // plain probability: alignment rows, normaliser, and - times the key's V scale - the P.V operand
      }
      ls[j] += pr;
    }
    u32x4_t v0[4], v1[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) sk_widen8<T>(vraw[g][dt], 1.0f, v0[dt], v1[dt]);
#pragma unroll
    for (int j2 = 0; j2 < 2; ++j2) {   // operand j2 of lane (fr, kq): keys kq*16 + j2*8 .. +7 of this 64-key group, column fc
      const unsigned sb_lo = j2 == 0 ? vs16[g][0] : vs16[g][2];   // scale bytes of keys +0..3
      const unsigned sb_hi = j2 == 0 ? vs16[g][1] : vs16[g][3];   //                      +4..7
      float pv[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int t = g64 * 64 + kq * 16 + j2 * 8 + e;
        const unsigned sb = ((e < 4 ? sb_lo : sb_hi) >> (8 * (e & 3))) & 0xffu;
        // same wavefront wrote the probabilities: LDS operations of a wavefront stay in order
        pv[e] = (t < n_bound) ? sc[fc * S + t] * __builtin_bit_cast(float, (sb + (kPvUp ? 7u : 0u)) << 23) : 0.f;
      }
      const u32x4_t pf = pack16<T>(pv);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) o[dt] = sk_mfma<T>(j2 == 0 ? v0[dt] : v1[dt], pf, o[dt]);
    }
  }
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    // lane 0's sum, as in the single-query kernel (see dec_cross_attn_rows_kernel)
    if (j < nc) {
      const float l = tw_wave_sum(ls[j]);
      if (lane == 0) wl[wave * NC + j] = l;
    }
  }
  if (own) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) *reinterpret_cast<f32x4_t*>(wo + (wave * NC + fr) * WS + dt * 16 + kq * 4) = o[dt];
  }
  __syncthreads();
  {   // NC columns x 64 dims over 512 threads
    const int j = tid >> 6, k = tid & 63;   // (j is uniform in a wavefront)
    if (j < nc) {   // a column behind the last beam has no normaliser
      float L = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) L += wl[w * NC + j];
      const float inv = 1.0f / L;
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) v += wo[(w * NC + j) * WS + k];
      const int b = clip + j * n_clips;
      T* dst = out + (long long)(b >> 4) * 16 * H * 64 + tw_xt_index<T>(b & 15, h * 64 + k);
      if constexpr (kPvUp) *dst = tw_cast<T>(v * inv * 0.0078125f);
      else *dst = (T)(v * inv);
    }
  }
  const int slot = align_slot ? align_slot[h] : -1;
  if (slot >= 0) {  // A11 side output: every beam writes the softmax row of its own slot at this position
    const int pos = stt->pos;
    for (int j = 0; j < nc; ++j) {
      float L = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) L += wl[w * NC + j];
      const float inv = 1.0f / L;
      float* row = align + (((long long)(clip + j * n_clips) * Ha + slot) * P + pos) * Tlen;
      for (int t = tid; t < Tlen; t += 512) row[t] = sc[j * S + t] * inv;
    }
  }
}

}  // namespace

// Reached through launch_dec_cross_attn only, which has made every check (float16 activations, fp8 caches with both scale arrays,
// rows_streams == 0, B a multiple of n_clips, 2 <= B / n_clips <= kBeamMax, Tp <= 1536) and reports the grid.  B = n_clips * K rows,
// beam k of clip c = row k * n_clips + c.  Float16 only: tw_generate_beam refuses the bf16-based fp8 contexts.
hipError_t launch_dec_cross_attn_kv8_beams(const void* q, const FusedQ& fq, const void* ck, const void* cv, void* out, int B, int H, int T,
                                           int Tp, const int* align_slot_for_head, float* align, int Ha, int P, const DecState* stt,
                                           const unsigned char* ksc, const unsigned char* vsc, int n_clips, hipStream_t st) {
  using TT = f16_t;
  using Lds = RowsLds<kBeamCols, 2>;
  const int K = B / n_clips;
  const dim3 grid(H, n_clips, 1);
  return tw_with_int<1, 2, 3>(Tp <= 512 ? 1 : (Tp <= 1024 ? 2 : 3), [&](auto g) {
    return tw_with_bool(fq.u != nullptr, [&](auto f) {
      return tw_launch_big_lds<&dec_cross_attn_kv8_beams_kernel<TT, g(), f()>, Lds::cap>(
          grid, dim3(512), Lds::bytes(Tp), st, (const unsigned char*)ck, (const unsigned char*)cv, ksc, vsc, H, Tp, T, n_clips, K,
          (const TT*)q, (TT*)out, align_slot_for_head, align, Ha, P, stt, fq);
    });
  });
}
