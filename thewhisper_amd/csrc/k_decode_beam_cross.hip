// Beams mode of the decoder cross attention (launch_dec_cross_attn with beam_clips > 0: a step of tw_generate_beam).  The kernel is
// dec_cross_attn_rows_kernel<T, SINGLE, FQ, BEAMS = true> of k_decode_attn.h - one workgroup per (head, clip) reads the clip's K / V^T
// once for all of its beams.  A translation unit of its own: it is built without the packed float32 instructions (thewhisper_amd/
// build.py: FILE_FLAGS), the older sources keep the flags their code objects were measured with.
#include "tw_common.h"
#include "k_decode_attn.h"

static_assert(kBeamMax <= kBeamCols, "a clip's beams are the columns of one workgroup");

// The checks on Tp, the FusedQ block and q are launch_dec_cross_attn's, which is the only caller.  B = n_clips * K rows, beam k of
// clip c = row k * n_clips + c; fp8 caches have no beams mode (tw_generate_beam refuses fp8 contexts).
hipError_t launch_dec_cross_attn_beams(int dtype, const void* q, const FusedQ& fq, const void* ck, const void* cv, void* out, int B, int H,
                                       int T, int Tp, const int* align_slot_for_head, float* align, int Ha, int P, const DecState* stt,
                                       int n_clips, hipStream_t st, int* grid3) {
  if (n_clips < 1 || B % n_clips != 0 || B / n_clips > kBeamMax || B / n_clips < 2 || Tp > 1536 || dtype < 0 || dtype > 2)
    return hipErrorInvalidValue;
  const int K = B / n_clips;
  const dim3 grid(H, n_clips, 1);
  const bool single = Tp <= 512;
  const bool f = fq.u != nullptr;
  const size_t esz = dtype == 0 ? 4 : 2;
  const size_t ldsb = ((size_t)kBeamCols * (Tp + 4) + 8 * kBeamCols * 68 + 8 * 16 + 8 * kBeamCols) * sizeof(float) + kBeamCols * 64 * esz;
  constexpr int lds_cap = (kBeamCols * (1536 + 4) + 8 * kBeamCols * 68 + 8 * 16 + 8 * kBeamCols) * 4 + kBeamCols * 64 * 4;
  static_assert(lds_cap <= 160 * 1024, "LDS of a compute unit");
#define CAB_GO(TT, SV, FV) do {                                                                                                        \
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&dec_cross_attn_rows_kernel<TT, SV, FV, true>),   \
                                                        hipFuncAttributeMaxDynamicSharedMemorySize, lds_cap);                          \
    if (attr != hipSuccess) return attr;                                                                                               \
    hipLaunchKernelGGL((dec_cross_attn_rows_kernel<TT, SV, FV, true>), grid, dim3(512), ldsb, st, (const TT*)ck, (const TT*)cv, H, Tp, \
                       T, n_clips, K, (const TT*)q, (TT*)out, align_slot_for_head, align, Ha, P, stt, fq);                             \
  } while (0)
#define CAB_PICK(TT) do { if (single) { if (f) CAB_GO(TT, true, true); else CAB_GO(TT, true, false); }                               \
                          else { if (f) CAB_GO(TT, false, true); else CAB_GO(TT, false, false); } } while (0)
  if (dtype == 1) CAB_PICK(bf16_t); else if (dtype == 2) CAB_PICK(f16_t); else CAB_PICK(float);
#undef CAB_PICK
#undef CAB_GO
  if (grid3) { grid3[0] = H; grid3[1] = n_clips; grid3[2] = 1; }
  return hipGetLastError();
}
