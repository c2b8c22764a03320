// Beams mode of the decoder cross attention (launch_dec_cross_attn with beam_clips > 0: a step of tw_generate_beam).  The kernel is
// dec_cross_attn_rows_kernel<T, SINGLE, FQ, BEAMS = true> of k_decode_attn.h - one workgroup per (head, clip) reads the clip's K / V^T
// once for all of its beams.  A translation unit of its own: it is built without the packed float32 instructions (thewhisper_amd/
// build.py: FILE_FLAGS), the older sources keep the flags their code objects were measured with.
#include "tw_common.h"
#include "k_decode_attn.h"

static_assert(kBeamMax <= kBeamCols, "a clip's beams are the columns of one workgroup");

// Reached through launch_dec_cross_attn only, which has made every check (2 <= B / n_clips <= kBeamMax, Tp <= 1536) and reports the
// grid.  B = n_clips * K rows, beam k of clip c = row k * n_clips + c; the fp8 caches' beams kernel is k_decode_kv8_beams.hip's.
// One cap for the three element types.
hipError_t launch_dec_cross_attn_beams(int dtype, const void* q, const FusedQ& fq, const void* ck, const void* cv, void* out, int B, int H,
                                       int T, int Tp, const int* align_slot_for_head, float* align, int Ha, int P, const DecState* stt,
                                       int n_clips, hipStream_t st) {
  const int K = B / n_clips;
  const dim3 grid(H, n_clips, 1);
  TW_DISPATCH3(dtype, TT, return tw_with_bool(Tp <= 512, [&](auto single) {
    return tw_with_bool(fq.u != nullptr, [&](auto f) {
      return tw_launch_big_lds<&dec_cross_attn_rows_kernel<TT, single(), f(), true>, RowsLds<kBeamCols, 4>::cap>(
          grid, dim3(512), RowsLds<kBeamCols, (int)sizeof(TT)>::bytes(Tp), st, (const TT*)ck, (const TT*)cv, H, Tp, T, n_clips, K,
          (const TT*)q, (TT*)out, align_slot_for_head, align, Ha, P, stt, fq);
    });
  }));
}
