// Large-M MFMA GEMM over MXFP8 weights (TW_F16_W8A16_FULL: the encoder's four linears per layer and the cross-K/V projection):
//   C[M,N] = epilogue(A[M,K] . w(W8, WS)[N,K]^T),   w = RNE_f16(e4m3 x 2^(sb-127))  (sk_widen8<f16_t>, k_decode_attn.h),
// float16 activations, NOT quantised ("W8A16").  gemm_w8reg_kernel is gemm_wreg_kernel (k_gemm.hip) with a new weight side: block
// geometry, activation ring (global->LDS DMA, 3 stages, source-side swizzle), tile order and every epilogue are that kernel's, through
// k_gemm.h.  A K tile of 64 is contracted with v_mfma_f32_16x16x32_f16 in ascending k into one accumulator per output tile, as in both
// kernels of k_gemm.hip: on equal weight VALUES the output bits are theirs, whatever M, the tile height or the batch.
//
// Weight side
//  * Storage (launch_quant_mx8 with 16-row tiles + launch_w8_scales, once at tw_finalize_weights): fragment of n-tile t = n / 16 and
//    K tile kt = k / 64 is 1 KiB at ((t * K/64 + kt) * 64 + lane) * 16, lane = kq*16 + n%16; its 16 bytes are the lane's 8 e4m3 of
//    k-step 0 (W[n][kt*64 + kq*8 .. +8]) and of k-step 1 (W[n][kt*64 + 32 + kq*8 .. +8]): ONE 16-byte request per lane, n-tile and K
//    tile brings the MFMA A operands of both 32-k steps - four requests per wavefront and K tile where gemm_wreg_kernel issues eight.
//  * Blocks are the decoder's (sk_quant_mx8): inside a K tile, the 2 x 16 values of the lane groups kq = 2u, 2u+1 share scale (kt, u),
//    so a lane widens its whole 16-byte fragment with ONE scale.  Scale bytes, per 64 rows (one wavefront's columns) and PAIR of K
//    tiles: [u][n%16][n-tile of the 64][kt & 1] - a lane fetches the 8 bytes of its 4 n-tiles x 2 K tiles with one 64-bit request (256
//    contiguous bytes per wavefront), every second K tile.
//  * Pipeline, per K tile kt: the widened fragments of tile kt sit in one of two alternating register sets (32 VGPRs each), the raw
//    bytes of tile kt+1 have landed (16 VGPRs).  Tile kt+1 is widened into the idle set - 32 converts per lane beside the 16 x MT
//    MFMAs of tile kt, which read the other set and so never wait on a convert of their own tile - and the raw registers are then
//    re-requested for tile kt+2, in front of the activation DMA of tile kt+2.  Requests are unconditional (past the end they re-fetch
//    the last tile), straight-line and in consumption order; one hand-placed s_waitcnt vmcnt(AV) per K tile covers A(kt) and raw(kt+1).
#include "k_decode_attn.h"   // sk_widen8
#include "k_gemm.h"

namespace {

__device__ __forceinline__ void tw_tie2(u32x2_t& x) { asm volatile("" : "+v"(x)); }
// 8-B global load invisible to hipcc's wait-count pass (tw_gload's note)
__device__ __forceinline__ void tw_gload2(u32x2_t& dst, const void* p) { asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(dst) : "v"(p)); }

template <typename T, int BM, int NW, int ST>
__global__ __launch_bounds__(NW * 64, 2) void gemm_w8reg_kernel(const T* __restrict__ A, RowMap amap, const unsigned char* __restrict__ W8,
                                                              const unsigned char* __restrict__ WS, int M, int N, int K, int Tm, int Tn,
                                                              int swz, GemmEpilogue ep) {
  constexpr int E = ElemTraits<T>::kPer16B;
  constexpr int BKE = 8 * E;
  constexpr int BN = NW * 64;
  constexpr int NTHR = NW * 64;
  constexpr int AV = (BM * 8 + NTHR - 1) / NTHR;   // DMA pieces per thread and stage (gemm_wreg_kernel: rows past the tile land where nobody reads)
  constexpr int MT = BM / 16, NT = 4;
  static_assert(sizeof(T) == 2 && BM % 16 == 0 && AV >= 1 && ST == 3, "tile layout");
  constexpr int STAGE = AV * NTHR;
  __shared__ u32x4_t lds[ST * STAGE];
  __shared__ f32x2_t ln_rows[BM];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  int tile_m, tile_n;
  if (!tw_tile_of_block(blockIdx.x, Tm, Tn, swz, tile_m, tile_n)) return;   // (whole workgroup: before any barrier)
  const int n0 = tile_n * BN + wave * 64;
  const int m0 = tile_m * BM;
  const int nk = K / BKE;          // even: K % 128 == 0
  const int fr = lane & 15, fq = lane >> 4;

  const T* asrc[AV];
#pragma unroll
  for (int i = 0; i < AV; ++i) {
    const int p = (i * NW + wave) * 64 + lane;
    const int row = p >> 3, slot = (p & 7) ^ ((row >> 1) & 7);
    int m = m0 + row;
    if (m >= M) m = M - 1;
    asrc[i] = A + rowmap(amap, m) + slot * E;
  }
  // this wavefront's 4 n-tiles, K tile 0 (a wavefront past N - launches with N % BN != 0 - reads the last tiles and stores nothing)
  const unsigned char* wsrc[NT];
#pragma unroll
  for (int a = 0; a < NT; ++a) wsrc[a] = W8 + ((long long)min(n0 / 16 + a, N / 16 - 1) * nk * 64 + lane) * 16;
  const unsigned char* ssrc = WS + ((long long)min(n0 / 64, N / 64 - 1) * (nk >> 1) * 32 + (fq >> 1) * 16 + fr) * 8;
  typedef __attribute__((address_space(1))) const void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;
  auto issue_a = [&](int kt, int b) {
    u32x4_t* sa = lds + b * STAGE;
#pragma unroll
    for (int i = 0; i < AV; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(asrc[i] + kt * BKE), (lptr_t)(sa + (i * NW + wave) * 64), 16, 0, 0);
  };
  u32x4_t raw[NT];              // e4m3 fragments of the tile that is widened next
  u32x2_t sc;                   // scale bytes of that tile's pair: byte 2a + (kt & 1)
  u32x4_t w0[NT][2], w1[NT][2]; // widened fragments [n-tile][k-step], used alternately (the K loop is unrolled by two)
  auto load_raw = [&](int kt) {
#pragma unroll
    for (int a = 0; a < NT; ++a) tw_gload<0>(raw[a], wsrc[a] + (long long)kt * 1024);
  };
  auto load_sc = [&](int pair) { tw_gload2(sc, ssrc + (long long)pair * 256); };
  auto widen = [&](u32x4_t (&w)[NT][2], int odd) {
#pragma unroll
    for (int a = 0; a < NT; ++a) {
      const unsigned sb = (sc[a >> 1] >> (16 * (a & 1) + 8 * odd)) & 0xffu;
      sk_widen8<T>(raw[a], __builtin_bit_cast(float, sb << 23), w[a][0], w[a][1]);
    }
  };

  f32x4_t acc[NT][MT];
  int buf = 0;
  unsigned a_addr[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) a_addr[kk] = tw_lds_addr(lds) + (unsigned)(fr * 8 + ((kk * 4 + fq) ^ ((fr >> 1) & 7))) * 16;
  // one K tile.  A(kt), raw(kt+1) and the scales of tile kt+1's pair have landed once vmcnt says that only the AV pieces of A(kt+1) may
  // be in flight (requests retire in order); `cur` = widened tile kt was finished in the previous step (the ties keep its converts
  // there).  Then: tile kt+1 -> `nxt`; raw(kt+2) [even kt: + the scales of pair (kt+2)/2], A(kt+2); tile kt is multiplied.
  auto step = [&](int kt, auto oddc, u32x4_t (&cur)[NT][2], u32x4_t (&nxt)[NT][2]) {
    constexpr int odd = decltype(oddc)::value;   // kt & 1
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(AV) : "memory");
#pragma unroll
    for (int a = 0; a < NT; ++a) { tw_tie(cur[a][0]); tw_tie(cur[a][1]); tw_tie(raw[a]); }
    tw_tie2(sc);
    tw_barrier_only();
    widen(nxt, 1 - odd);
    load_raw(min(kt + 2, nk - 1));
    if constexpr (odd == 0) load_sc(min((kt + 2) >> 1, (nk >> 1) - 1));
    {
      int nb = buf + ST - 1;
      if (nb >= ST) nb -= ST;
      issue_a(min(kt + ST - 1, nk - 1), nb);
    }
    const unsigned stage_off = (unsigned)buf * (STAGE * 16);
    tw_static_for<0, 2>([&](auto kkc) {
      constexpr int kk = decltype(kkc)::value;
      u32x4_t af[MT];
      tw_static_for<0, MT>([&](auto bc) { tw_lds_read<decltype(bc)::value * 2048>(af[decltype(bc)::value], a_addr[kk] + stage_off); });
      // fragments are consumed in arrival order: MFMAs on af[b] start while af[b+1..] are still on their way
      tw_static_for<0, MT>([&](auto bc) {
        constexpr int b = decltype(bc)::value;
        tw_lds_ready<MT - 1 - b>(af[b]);
#pragma unroll
        for (int a = 0; a < NT; ++a) acc[a][b] = mfma_step<T>(cur[a][kk], af[b], acc[a][b]);
      });
    });
    if (++buf == ST) buf = 0;
  };
  // request order: [row statistics of a folded LayerNorm,] raw(0), scales(0), A(0) | raw(1), A(1) | per tile: raw(kt+2) [, scales], A(kt+2)
  LnRaw ln_raw;
  if (ep.stats_in) gemm_ln_request<BM, NTHR>(ep, m0, M, tid, ln_raw);
  load_raw(0);
  load_sc(0);
  issue_a(0, 0);
  if (ep.stats_in) gemm_ln_publish<BM, NTHR>(ep, tid, ln_raw, ln_rows);
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(AV) : "memory");   // raw(0) and its scales
#pragma unroll
  for (int a = 0; a < NT; ++a) tw_tie(raw[a]);
  tw_tie2(sc);
  widen(w0, 0);
  load_raw(1);
  issue_a(1, 1);
#pragma unroll
  for (int a = 0; a < NT; ++a)   // (zeroed here, after the prologue's registers are free again)
#pragma unroll
    for (int b = 0; b < MT; ++b) acc[a][b] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  for (int kt = 0; kt < nk; kt += 2) {
    step(kt, std::integral_constant<int, 0>{}, w0, w1);
    step(kt + 1, std::integral_constant<int, 1>{}, w1, w0);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the redundant tail requests must not outlive the LDS allocation
  gemm_wreg_finish<T, NT, MT, ST * STAGE * 4 / NW>(acc, m0, n0, M, N, ep, fr, fq, lane, ln_rows, reinterpret_cast<float*>(lds), wave);
}

// scale bytes as launch_quant_mx8 (16-row tiles) leaves them - per (n-tile, 128-k step) 64 bytes, block (K-tile half h, lane-group pair u) of
// row r at (2h + u) * 16 + r - into the per-wavefront layout of the header comment; one thread per byte
__global__ __launch_bounds__(256) void w8_scales_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int N, int K) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)N * (K / 32)) return;
  const int j = (int)(i & 1), a = (int)(i >> 1) & 3, r = (int)(i >> 3) & 15, u = (int)(i >> 7) & 1;
  const long long bp = i >> 8;                    // (64-row block, pair of K tiles)
  const int pairs = K / 128;
  const long long blk = bp / pairs, p = bp - blk * pairs;
  dst[i] = src[((blk * 4 + a) * pairs + p) * 64 + (2 * j + u) * 16 + r];
}

template <int BM, int NW>
hipError_t gemm_w8_go(const void* A, RowMap amap, const void* W8, const void* WS, int M, int N, int K, const GemmEpilogue& ep, hipStream_t st) {
  const int Tn = (N + NW * 64 - 1) / (NW * 64), Tm = (M + BM - 1) / BM;
  int swz;
  dim3 grid(gemm_grid(Tm, Tn, true, &swz));
  hipLaunchKernelGGL((gemm_w8reg_kernel<f16_t, BM, NW, 3>), grid, dim3(NW * 64), 0, st, reinterpret_cast<const f16_t*>(A), amap,
                     reinterpret_cast<const unsigned char*>(W8), reinterpret_cast<const unsigned char*>(WS), M, N, K, Tm, Tn, swz, ep);
  return hipGetLastError();
}

}  // namespace

// Tile of a launch: where gemm_plan gives the 16-bit weights their BM x 256 tiles (from 256 tiles of 128 x 256 on), 80 x 256 over 4
// wavefronts - the one height of gemm_plan's four that this kernel holds in 256 registers: 16 raw + 2 scale registers beside the two
// widened sets make 96 rows spill 2 registers and 128 rows 99 (hipcc's resource remarks), and a spilled register of an in-flight
// request is read before its data has landed.  Below that - one stream, the micro models: this context has no 16-bit weights for the
// small-M kernel - 64 x 128 tiles over 2 wavefronts (one 10 s clip of large-v3: 80 to 320 workgroups where 128 x 256 tiles would be 20
// to 80).  kernel = 3 either way.
GemmPlan gemm_w8_plan(int M, int N) { return GemmPlan{3, gemm_plan(EPI_ROWMAJOR, M, N).kernel == 2 ? 80 : 64}; }

hipError_t launch_gemm_w8(const void* A, RowMap amap, const void* W8, const void* WS, int M, int N, int K, const GemmEpilogue& ep0,
                          hipStream_t st) {
  if (M <= 0) return hipSuccess;
  if (K % 128 != 0 || N % 128 != 0) return hipErrorInvalidValue;
  GemmEpilogue ep = ep0;
  ep.staged = 1;
  switch (gemm_w8_plan(M, N).bm) {
    case 64: return gemm_w8_go<64, 2>(A, amap, W8, WS, M, N, K, ep, st);
    default: return gemm_w8_go<80, 4>(A, amap, W8, WS, M, N, K, ep, st);
  }
}

hipError_t launch_w8_scales(const void* src, void* dst, int N, int K, hipStream_t st) {
  if (K % 128 != 0 || N % 64 != 0) return hipErrorInvalidValue;
  const long long total = (long long)N * (K / 32);
  hipLaunchKernelGGL(w8_scales_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const unsigned char*>(src),
                     reinterpret_cast<unsigned char*>(dst), N, K);
  return hipGetLastError();
}
