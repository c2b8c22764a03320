// MFMA GEMM for the MFMA-bound part of the hot path (A2 conv stem, A3 encoder projections/FFN,
// A5 cross-K/V projection):  C[M,N] = epilogue(A[M,K] . W[N,K]^T),  both operands K-contiguous
// (activations token-major, weights in the HF nn.Linear [out,in] layout).
//
// gfx950 design
//  * 256 threads = 4 waves in a 2x2 arrangement; block tile BM (activation rows) x BN (weight rows),
//    K tile = 8 x 16 B per row (64 bf16 / 32 f32).  128x128 for large M, 64x64 when the grid
//    would otherwise not cover the 256 CUs.
//  * LDS image: [row][k-slot ^ ((row>>1)&7)] of 16-B vectors, filled by direct global->LDS DMA
//    (global_load_lds_dwordx4, swizzle applied on the source side: 8 lanes still cover one 128-B
//    row segment); the MFMA fragment read (16 lanes = 16 consecutive rows of one k-slot,
//    ds_read_b128) touches every bank once.
//  * "swapped" MFMA: the weight tile is the A operand and the activation tile the B operand of
//    v_mfma_f32_16x16x32_bf16 (or 4 x v_mfma_f32_16x16x4_f32 in strict-f32 mode, using a
//    k-permutation so that the same 16-B fragment feeds both), so every lane ends up with 4
//    consecutive output columns of one row -> 8/16-B epilogue stores and vector bias loads.
//  * double-buffered LDS, one barrier per K tile: the DMA of tile k+1 is issued right after the
//    barrier that retires tile k and runs under the MFMAs of tile k (no staging registers, no
//    ds_write pass: 1.2-1.5x the register-staged version of this kernel).
//  * fused epilogues: bias, exact GELU, residual / positional add, and the head-split / transposed
//    layouts the attention kernels consume (no separate permute kernels).
#include "k_gemm.h"   // LDS / global request helpers, tw_tile_of_block, the folded-LayerNorm rows and every epilogue (shared with k_gemm_w8.hip)

namespace {

// The weight operand W[N,K] of every GEMM is stored FRAGMENT-MAJOR (launch_tile_weights with 16-row tiles, done once at
// tw_finalize_weights): for n-tile t = n/16 and k-step s = k/(4E) one contiguous 1-KiB block holds the MFMA A operand exactly
// as the 64 lanes consume it (lane = kq*16 + n%16 holds W[n][s*4E + kq*E .. +E]); element offset ((t*S + s)*64 + lane)*E with
// S = K/(4E).  Either kernel moves whole 1-KiB fragments: kernel 1 by DMA into LDS (fragment reads are then linear and
// conflict-free), kernel 2 straight into registers.

// Kernel 1.  BM x BN block tile, WM x WN wavefronts (each owns a (BM/WM) x (BN/WN) sub-tile), both operands through an
// ST-stage LDS ring filled by global->LDS DMA with prefetch distance ST-1.  One barrier per K tile: after it, tile kt is
// visible to every wavefront and buffer (kt-1) % ST - consumed in the previous iteration - is free for tile kt + ST - 1.
// Used for small M (single stream) where the grid needs small tiles.
template <typename T, int BM, int BN, int WM, int WN, int ST>
__global__ __launch_bounds__(WM * WN * 64) void gemm_kernel(const T* __restrict__ A, RowMap amap, const T* __restrict__ W,
                                                              int M, int N, int K, int Tm, int Tn, int swz, GemmEpilogue ep) {
  constexpr int E = ElemTraits<T>::kPer16B;  // elements per 16-B vector
  constexpr int BKE = 8 * E;                 // elements per K tile (two MFMA k-steps)
  constexpr int NWAVE = WM * WN;
  constexpr int NTHR = NWAVE * 64;
  constexpr int AV = BM * 8 / NTHR;          // 16-B vectors per thread per tile (activations)
  constexpr int WV = BN * 8 / NTHR;          // (weights): BN/8 fragments of 64 vectors per K tile
  constexpr int RM = BM / WM, RN = BN / WN;  // rows / columns of a wavefront's sub-tile
  constexpr int MT = RM / 16;                // 16-row MFMA tiles per wave along M
  constexpr int NT = RN / 16;                // along N
  static_assert(AV >= 1 && WV >= 1 && MT >= 1 && NT >= 1, "tile / wavefront layout");
  constexpr int STAGE = 8 * (BM + BN);       // 16-B vectors per ring stage
  constexpr int PER = AV + WV;               // DMA requests per thread and stage
  static_assert(ST >= 2 && (ST - 2) * PER <= 63, "ring depth against the 6-bit vmcnt");
  // the ring lives in dynamic LDS (any depth the 160 KB of a CU and the 6-bit vmcnt allow; deep rings were tried, see gemm_dispatch)
  extern __shared__ __attribute__((aligned(16))) unsigned char gemm_smem[];
  u32x4_t* lds = reinterpret_cast<u32x4_t*>(gemm_smem);
  f32x2_t* ln_rows = reinterpret_cast<f32x2_t*>(gemm_smem + (size_t)ST * STAGE * 16);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wn = wave % WN;  // wave position along N
  const int wm = wave / WN;  // along M
  int tile_m, tile_n;
  if (!tw_tile_of_block(blockIdx.x, Tm, Tn, swz, tile_m, tile_n)) return;   // (whole workgroup: before any barrier)
  const int n0 = tile_n * BN;
  const int m0 = tile_m * BM;
  const int S = K / (4 * E);

  // Activations: the DMA writes the 64 lanes of a wavefront to 64 consecutive 16-B LDS slots, so the swizzle is applied on
  // the SOURCE side: linear LDS position p (16-B units) of a tile holds row p>>3, k-slot (p&7) ^ ((row>>1)&7); 8 consecutive
  // lanes still cover one 128-B row segment of global memory (coalesced), and the fragment read - 16 lanes = 16 consecutive
  // rows of one k-slot, ds_read_b128 - touches every bank exactly once.
  const T* asrc[AV];
#pragma unroll
  for (int i = 0; i < AV; ++i) {
    const int p = (i * NWAVE + wave) * 64 + lane;
    const int row = p >> 3, slot = (p & 7) ^ ((row >> 1) & 7);
    int m = m0 + row;
    if (m >= M) m = M - 1;
    asrc[i] = A + rowmap(amap, m) + slot * E;
  }
  // Weights: DMA piece q = i*NWAVE + wave is fragment (n-tile q>>1, k-step q&1) of this K tile
  const T* wsrc[WV];
#pragma unroll
  for (int i = 0; i < WV; ++i) {
    const int q = i * NWAVE + wave;
    const int tile = min(n0 / 16 + (q >> 1), N / 16 - 1);
    wsrc[i] = W + (((long long)tile * S + (q & 1)) * 64 + lane) * E;
  }
  typedef __attribute__((address_space(1))) const void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;
  auto issue_tile = [&](int kt, int b) {
    u32x4_t* sa = lds + b * STAGE;
    u32x4_t* sw = sa + 8 * BM;
#pragma unroll
    for (int i = 0; i < AV; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(asrc[i] + kt * BKE), (lptr_t)(sa + (i * NWAVE + wave) * 64), 16, 0, 0);
#pragma unroll
    for (int i = 0; i < WV; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(wsrc[i] + (long long)kt * (2 * 64 * E)), (lptr_t)(sw + (i * NWAVE + wave) * 64), 16, 0, 0);
  };

  f32x4_t acc[NT][MT];
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int b = 0; b < MT; ++b) acc[a][b] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int nk = K / BKE;
  const int fr = lane & 15;  // fragment row within a 16-row tile
  const int fq = lane >> 4;  // k-slot quad
  unsigned a_addr[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    const int row = wm * RM + fr;
    a_addr[kk] = tw_lds_addr(lds) + (unsigned)(row * 8 + ((kk * 4 + fq) ^ ((row >> 1) & 7))) * 16;
  }
  const unsigned w_addr = tw_lds_addr(lds) + (unsigned)(8 * BM + ((wn * RN) / 16) * 2 * 64 + lane) * 16;
  LnRaw ln_raw;
  if (ep.stats_in) gemm_ln_request<BM, NTHR>(ep, m0, M, tid, ln_raw);
#pragma unroll
  for (int t = 0; t < ST - 1; ++t)
    if (t < nk) issue_tile(t, t);
  if (ep.stats_in) gemm_ln_publish<BM, NTHR>(ep, tid, ln_raw, ln_rows);
  int buf = 0;
  for (int kt = 0; kt < nk; ++kt) {
    // tile kt has landed: this wavefront's own DMA by vmcnt (requests retire in order; the ST-2 younger tiles may stay in
    // flight), the other wavefronts' by the barrier
    if (ST > 2 && kt + ST - 2 < nk) {
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"((ST - 2) * PER) : "memory");
    } else if (ST > 3) {
      // the last ST - 2 tiles: r = nk - 1 - kt younger tiles are in flight (r < ST - 2)
      const int r = nk - 1 - kt;
      tw_static_for<0, (ST > 3 ? ST - 2 : 1)>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        if (r == i) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(i * PER) : "memory");
      });
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    tw_barrier_only();
    if (kt + ST - 1 < nk) {
      int nb = buf + ST - 1;
      if (nb >= ST) nb -= ST;
      issue_tile(kt + ST - 1, nb);
    }
    const unsigned stage_off = (unsigned)buf * (STAGE * 16);
    tw_static_for<0, 2>([&](auto kkc) {
      constexpr int kk = decltype(kkc)::value;
      u32x4_t af[MT], wf[NT];
      // activation fragment b: row wm*RM + b*16 + fr (the swizzle term (row>>1)&7 does not depend on b), k-slot kk*4 + fq
      tw_static_for<0, MT>([&](auto bc) { tw_lds_read<decltype(bc)::value * 2048>(af[decltype(bc)::value], a_addr[kk] + stage_off); });
      // weight fragment a of this wavefront: linear, 1 KiB per (n-tile, k-step)
      tw_static_for<0, NT>([&](auto ac) { tw_lds_read<(decltype(ac)::value * 2 + kk) * 1024>(wf[decltype(ac)::value], w_addr + stage_off); });
      tw_lds_ready<0>(af[0]);
#pragma unroll
      for (int b = 1; b < MT; ++b) tw_tie(af[b]);
#pragma unroll
      for (int a = 0; a < NT; ++a) tw_tie(wf[a]);
#pragma unroll
      for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int b = 0; b < MT; ++b) acc[a][b] = mfma_step<T>(wf[a], af[b], acc[a][b]);
    });
    if (++buf == ST) buf = 0;
  }
  gemm_epilogue<T, NT, MT>(acc, m0 + wm * RM, n0 + wn * RN, M, N, ep, fr, fq, ep.stats_in ? ln_rows + wm * RM : nullptr);
}

// Kernel 2 (large M: the batched encoder, the cross-K/V projection).  The round-1 kernel staged both operands through LDS in
// 128 x 128 tiles and ran at 22 % of the matrix-core peak: per K tile the LDS pipe had to take 32 KB of DMA writes and serve
// 64 fragment reads for 128 MFMAs, about as many LDS cycles as MFMA cycles, and 32 KB per 2.1 MFLOP is also right at what a CU
// can pull from L2 (64 B/clk).  Here only the ACTIVATION tile goes through LDS; every wavefront owns a BM x 64 slab of the
// block tile (all NW wavefronts side by side along N, none stacked along M) and takes its weight fragments - which nobody
// else in the workgroup needs - straight from global memory into registers, 1 KiB contiguous per request, one K tile ahead.
// Per K tile and CU: 16 KB of DMA + 32 fragment reads per wavefront for 64 MFMAs each, and (16 + 32) KB for 4.2 MFLOP.
template <typename T, int BM, int NW, int ST>
__global__ __launch_bounds__(NW * 64, 2) void gemm_wreg_kernel(const T* __restrict__ A, RowMap amap, const T* __restrict__ W,
                                                             int M, int N, int K, int Tm, int Tn, int swz, GemmEpilogue ep) {
  constexpr int E = ElemTraits<T>::kPer16B;
  constexpr int BKE = 8 * E;
  constexpr int BN = NW * 64;
  constexpr int NTHR = NW * 64;
  // DMA pieces (64 x 16 B, one per wavefront request) per thread and stage.  BM need not be a multiple of NTHR / 8 rows (80, 96,
  // 112: tile heights that divide the grid better, see gemm_pick_bm): the last piece then also fetches rows past the tile
  // (clamped to the matrix; they land in LDS rows nobody reads)
  constexpr int AV = (BM * 8 + NTHR - 1) / NTHR;
  constexpr int MT = BM / 16, NT = 4;
  static_assert(BM % 16 == 0 && AV >= 1 && (ST == 2 || ST == 3), "tile layout");
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
  const int S = K / (4 * E);
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
  const T* wsrc[NT];   // this wavefront's 4 n-tiles, k-step 0
#pragma unroll
  for (int a = 0; a < NT; ++a) wsrc[a] = W + ((long long)min(n0 / 16 + a, N / 16 - 1) * S * 64 + lane) * E;
  typedef __attribute__((address_space(1))) const void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;
  auto issue_a = [&](int kt, int b) {
    u32x4_t* sa = lds + b * STAGE;
#pragma unroll
    for (int i = 0; i < AV; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(asrc[i] + kt * BKE), (lptr_t)(sa + (i * NW + wave) * 64), 16, 0, 0);
  };
  // two register sets for the weight fragments, used alternately (the K loop is unrolled by two): a copy "current <- next"
  // would let the compiler sink the copy - and with it the wait for the freshly issued loads - into the MFMA block
  u32x4_t w0[NT][2], w1[NT][2];
  auto load_w = [&](u32x4_t (&w)[NT][2], int kt) {
#pragma unroll
    for (int a = 0; a < NT; ++a) {
      const T* p = wsrc[a] + (long long)kt * (2 * 64 * E);
      tw_gload<0>(w[a][0], p);
      tw_gload<1024>(w[a][1], p);
    }
  };

  f32x4_t acc[NT][MT];
  const int nk = K / BKE;
  int buf = 0;
  unsigned a_addr[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) a_addr[kk] = tw_lds_addr(lds) + (unsigned)(fr * 8 + ((kk * 4 + fq) ^ ((fr >> 1) & 7))) * 16;
  // one K tile: A(kt) and `cur` = W(kt) have landed (vmcnt retires in order: with three stages the younger A(kt+1) may stay
  // in flight); then W(kt+1) -> `nxt` and A(kt+ST-1) are requested, in that order, and tile kt is multiplied
  auto step = [&](int kt, u32x4_t (&cur)[NT][2], u32x4_t (&nxt)[NT][2]) {
    // (requests are unconditional - past the last tile they re-fetch tile nk-1 into a free stage / the idle register set -
    // so that the loop body is straight-line code: with requests inside branches hipcc's wait-count bookkeeping gives up
    // at the join and drains everything, vmcnt(0), in front of the first MFMA)
    if (ST == 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(AV) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int a = 0; a < NT; ++a) { tw_tie(cur[a][0]); tw_tie(cur[a][1]); }
    tw_barrier_only();
    load_w(nxt, min(kt + 1, nk - 1));
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
  // request order: [row statistics of a folded LayerNorm,] A(0), W(0), A(1) | per tile: W(kt+1), A(kt+ST-1)
  LnRaw ln_raw;
  if (ep.stats_in) gemm_ln_request<BM, NTHR>(ep, m0, M, tid, ln_raw);
  issue_a(0, 0);
  load_w(w0, 0);
  if (ST == 3) issue_a(min(1, nk - 1), 1);
  if (ep.stats_in) gemm_ln_publish<BM, NTHR>(ep, tid, ln_raw, ln_rows);
#pragma unroll
  for (int a = 0; a < NT; ++a)   // (zeroed here, after the prologue's registers are free again)
#pragma unroll
    for (int b = 0; b < MT; ++b) acc[a][b] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  for (int kt = 0; kt < nk; kt += 2) {
    step(kt, w0, w1);
    if (kt + 1 < nk) step(kt + 1, w1, w0);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the redundant tail requests must not outlive the LDS allocation
  if constexpr (sizeof(T) == 2) {
    // rows contiguous over this wavefront's 64 columns: the epilogue staged through this wavefront's share of the ring
    constexpr int WAVE_FLOATS = ST * STAGE * 4 / NW;
    constexpr int RB = WAVE_FLOATS >= 2 * 16 * TW_STAGE_LD ? 2 : 1;
    static_assert(WAVE_FLOATS >= 16 * TW_STAGE_LD, "a 16-row chunk per wavefront");
    const bool rows64 = n0 + 64 <= N && (ep.mode == EPI_ROWMAJOR || (ep.mode == EPI_QKV_ENC && n0 < 2 * ep.H * 64));
    if (ep.staged && rows64) {   // (wavefront-uniform; the barrier below is reached by every wavefront: ep.staged is a launch constant)
      tw_barrier_only();         // every wavefront has read its last fragments and every DMA has landed: the ring is free
      gemm_epilogue_staged<T, NT, MT, RB>(acc, m0, n0, M, N, ep, fr, fq, lane, ep.stats_in ? ln_rows : nullptr,
                                          reinterpret_cast<float*>(lds) + wave * WAVE_FLOATS);
      return;
    }
    if (ep.staged) tw_barrier_only();   // (keep the barrier count equal across the workgroup)
    constexpr int RBT = WAVE_FLOATS >= 64 * (2 * 16 + 4) ? 2 : 1;
    static_assert(WAVE_FLOATS >= 64 * (16 + 4), "a transposed 16-token chunk per wavefront");
    if (ep.staged == 1 && ep.mode == EPI_QKV_ENC && n0 >= 2 * ep.H * 64 && n0 + 64 <= N && ep.T % 4 == 0 && M % 4 == 0) {   // the V segment
      gemm_epilogue_staged_vt<T, NT, MT, RBT>(acc, m0, n0, M, N, ep, fr, fq, lane, ep.stats_in ? ln_rows : nullptr,
                                              reinterpret_cast<float*>(lds) + wave * WAVE_FLOATS);
      return;
    }
  }
  if (ep.mode == EPI_KV_CROSS8) gemm_epilogue_kv8<T, NT, MT>(acc, m0, n0, M, N, ep, fr, fq);
  else gemm_epilogue<T, NT, MT>(acc, m0, n0, M, N, ep, fr, fq, ep.stats_in ? ln_rows : nullptr);
}

}  // namespace

template <typename T, int BM, int BN, int WM, int WN, int ST>
static hipError_t gemm_go(const void* A, RowMap amap, const void* W, int M, int N, int K, const GemmEpilogue& ep, hipStream_t st) {
  const int Tn = (N + BN - 1) / BN, Tm = (M + BM - 1) / BM;
  int swz;
  dim3 grid(gemm_grid(Tm, Tn, false, &swz));
  constexpr size_t lds_bytes = (size_t)ST * 8 * (BM + BN) * 16 + (size_t)BM * sizeof(f32x2_t);   // ring + folded-LayerNorm rows
  static_assert(lds_bytes <= 160 * 1024, "LDS of a compute unit");
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_kernel<T, BM, BN, WM, WN, ST>),
                                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  if (attr != hipSuccess) return attr;
  hipLaunchKernelGGL((gemm_kernel<T, BM, BN, WM, WN, ST>), grid, dim3(WM * WN * 64), lds_bytes, st, reinterpret_cast<const T*>(A), amap,
                     reinterpret_cast<const T*>(W), M, N, K, Tm, Tn, swz, ep);
  return hipGetLastError();
}

template <typename T, int BM, int NW, int ST>
static hipError_t gemm_wreg_go(const void* A, RowMap amap, const void* W, int M, int N, int K, const GemmEpilogue& ep, hipStream_t st) {
  const int Tn = (N + NW * 64 - 1) / (NW * 64), Tm = (M + BM - 1) / BM;
  int swz;
  dim3 grid(gemm_grid(Tm, Tn, true, &swz));
  hipLaunchKernelGGL((gemm_wreg_kernel<T, BM, NW, ST>), grid, dim3(NW * 64), 0, st, reinterpret_cast<const T*>(A), amap,
                     reinterpret_cast<const T*>(W), M, N, K, Tm, Tn, swz, ep);
  return hipGetLastError();
}

// Which kernel and tile height a launch gets: the ONE copy of the choice (gemm_dispatch calls it; tw_gemm_plan reports it, so that a
// test can prove which path a shape took).  kernel 2 = gemm_wreg_kernel with a bm x 256 tile, kernel 1 = gemm_kernel with bm x 64.
GemmPlan gemm_plan(int mode, int M, int N) {
  if (mode == EPI_KV_CROSS8) return GemmPlan{2, 128};   // fp8 cross-K/V epilogue: one head per wavefront, i.e. kernel 2 whatever the shape
  // kernel 2 from 512 128 x 128 tiles on: 128 x 256 tiles need >= 256 workgroups to cover the chip.  One 30 s chunk's fc1
  // (M = 1500, N = 5120: 480 tiles = 240 workgroups) is faster in 128 x 64 tiles (encoder 6.27 -> 6.00 ms, profiles/r03_gemm_tiles.txt)
  const long long b128 = (long long)((M + 127) / 128) * ((N + 127) / 128);
  if (N % 256 == 0 && b128 >= 512) {
    // Tile HEIGHT of kernel 2 by how the grid divides over the chip.  Two workgroups share a CU's matrix pipe, so a CU's time is
    // proportional to the rows of the tiles it gets, ceil(tiles / 256) x BM, and the kernel ends with the last CU.  The out-projection
    // and fc2 of 16 x 10 s (M = 8000, N = 1280) are 63 x 5 = 315 tiles of 128 rows: 59 CUs get two and everybody waits for them (the
    // launch runs at the pace of 512 tiles); 100 x 5 tiles of 80 rows put two on (almost) every CU: 160 instead of 256 rows per CU.
    // `ovh` rows stand for the per-tile prologue + epilogue (24 picked 96-row tiles for the QKV projection, 111 vs 106 us, and lost
    // 3 % at 16 x 30 s).
    constexpr int ovh = 48;
    int best = 128;
    long long best_cost = -1;
    for (int bm : {128, 112, 96, 80}) {
      const long long tiles = (long long)((M + bm - 1) / bm) * (N / 256);
      const long long cost = ((tiles + 255) / 256) * (bm + ovh);
      if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = bm; }
    }
    return GemmPlan{2, best};
  }
  return GemmPlan{1, M <= 1000 ? 64 : 128};   // (gemm_dispatch: why 64 x 64 up to 1000 rows)
}

template <typename T>
static hipError_t gemm_dispatch(const void* A, RowMap amap, const void* W, int M, int N, int K,
                                const GemmEpilogue& ep, hipStream_t st) {
  constexpr int E = ElemTraits<T>::kPer16B;
  if (M <= 0) return hipSuccess;
  if (K % (8 * E) != 0 || N % 64 != 0) return hipErrorInvalidValue;
  // Tile choice:
  //   kernel 2: BM x 256 (BM = 80 ... 128), 4 wavefronts side by side, weights straight to registers, 3-stage activation ring - large M
  //   kernel 1: 128 x 64 (3 stages) or 64 x 64 (4 stages), both operands through an LDS ring - small M (one to three streams)
  if (ep.mode == EPI_KV_CROSS8 && (ElemTraits<T>::kCode == 0 || N % 64 != 0)) return hipErrorInvalidValue;   // 16-bit contexts only
  const GemmPlan plan = gemm_plan(ep.mode, M, N);
  if (plan.kernel == 2) {
    switch (plan.bm) {
      case 80: return gemm_wreg_go<T, 80, 4, 3>(A, amap, W, M, N, K, ep, st);
      case 96: return gemm_wreg_go<T, 96, 4, 3>(A, amap, W, M, N, K, ep, st);
      case 112: return gemm_wreg_go<T, 112, 4, 3>(A, amap, W, M, N, K, ep, st);
      default: return gemm_wreg_go<T, 128, 4, 3>(A, amap, W, M, N, K, ep, st);
    }
  }
  // Below that: 128 x 64 tiles on a 3-stage ring, or - up to 1000 rows (one chunk of <= 20 s, two of 10 s) - 64 x 64 tiles on a
  // 4-stage ring (64 KB: two workgroups per CU): one 10 s chunk 3.51 -> 3.04 ms, 15 s 3.90 -> 3.55, 2 x 10 s 4.32 -> 4.24; 30 s and
  // 3 x 10 s lose with it (5.46 -> 5.71, 4.96 -> 5.22) and stay.  Same accumulation order as every other tile shape: results do not
  // change.  Round 4 also tried DEEP rings on the theory that a single stream's K tiles each wait ~2 us for operands nobody has
  // warmed in L2 (8 x 16 KB of a 64 x 64 tile, 6 x 24 KB of a 128 x 64 tile, one workgroup per CU): out-projection 15.5 -> 12.5 us and
  // fc2 39.5 -> 30, but fc1 18.4 -> 34 and QKV 15.3 -> 24.5 - with one workgroup per CU the wide projections run 2.5 rounds and the
  // launch is bound by the aggregate operand traffic of its small tiles (210 MB for fc1 at M = 500 = 6 TB/s), not by latency
  // (profiles/r04_gemm_deep_ring_ab.txt).
  if (plan.bm == 64) return gemm_go<T, 64, 64, 2, 2, 4>(A, amap, W, M, N, K, ep, st);   // 64 KB: two workgroups per CU
  return gemm_go<T, 128, 64, 2, 2, 3>(A, amap, W, M, N, K, ep, st);
}

hipError_t launch_gemm(int dtype, const void* A, RowMap amap, const void* W, int M, int N, int K,
                       const GemmEpilogue& ep0, hipStream_t st) {
  GemmEpilogue ep = ep0;
  ep.staged = 1;   // the LDS-staged epilogue (and its V^T form) everywhere
  if (dtype == 1) return gemm_dispatch<bf16_t>(A, amap, W, M, N, K, ep, st);
  if (dtype == 2) return gemm_dispatch<f16_t>(A, amap, W, M, N, K, ep, st);
  return gemm_dispatch<float>(A, amap, W, M, N, K, ep, st);
}
