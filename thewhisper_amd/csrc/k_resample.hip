// Sample-rate / sample-format front end: whatever a client sends (8-96 kHz, float32 or int16, 1-8 interleaved channels)
// becomes the 16 kHz mono float32 that tw_logmel and tw_vad_energy expect.
//
// The reference resamples outside its hot path with librosa (R:thestage_speechkit/streaming/streams.py:103-105,
// R:examples/run_nvidia_asr.py:30).  This is NOT a port of librosa or soxr: it is this project's own rational polyphase
// windowed-sinc resampler, stated here, restated in float64 in tests/resample_ref.py and pinned there to
// scipy.signal.resample_poly with the same prototype:
//
//     g = gcd(sr_in, sr_out)   L = sr_out / g   M = sr_in / g   F = max(L, M)   half = 16 F   fc = 0.945 / F
//     h[j] = L fc sinc(fc j) I0(8.6 sqrt(1 - (j / half)^2)) / I0(8.6)          j = -half .. half   (float64, host: api.hip)
//     x[k] = mean over the channels of frame k, in float32, channels added in order; int16 samples are v / 32767 first
//     y[n] = sum_k x[k] h[n M - k L]                                             x[k] = 0 outside what the row holds
//
// sr_in == sr_out is the one-tap table {1}: y[n] = x[n] bit for bit.
//
// The kernel is a pure function of (input window, absolute indices).  Row b of a launch brings the absolute index of its
// first input frame, how many frames it holds and the absolute index of its first output; frames outside the window or left
// of absolute 0 read as zero, so a stream's state (a tail of input, two counters) lives in the caller.  One thread owns one
// output sample and runs ONE fmaf chain over ALL k of its support in ascending order, zeros included: the bits of y[n] then
// depend neither on the launch shape nor on how a stream was cut.
//
// A block of 256 threads makes 256 consecutive outputs of one row.  Their common input window is converted and down-mixed
// ONCE into LDS when it fits (every rate up to 13 x sr_out does); a thread reads its phase's taps with stride L from the
// table, which sits in LDS as well when L <= 2 (one phase or two: all threads walk the same few taps).
#include "tw_common.h"

namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ long long floor_div(long long a, long long b) {   // b > 0
  const long long q = a / b;
  return (a % b < 0) ? q - 1 : q;
}
__device__ __forceinline__ long long ceil_div(long long a, long long b) { return -floor_div(-a, b); }

// frame k (absolute) of a row as the filter sees it: converted, down-mixed, zero outside [max(0, first), first + count)
template <typename T>
__device__ __forceinline__ float load_frame(const T* __restrict__ row, long long k, long long first, int count, int channels) {
  const long long rel = k - first;
  if (k < 0 || rel < 0 || rel >= count) return 0.f;
  const T* p = row + rel * channels;
  float s;
  if constexpr (sizeof(T) == 2) {
    s = (float)p[0] / 32767.0f;
    for (int c = 1; c < channels; ++c) s += (float)p[c] / 32767.0f;
  } else {
    s = p[0];
    for (int c = 1; c < channels; ++c) s += p[c];
  }
  return channels > 1 ? s / (float)channels : s;
}

template <typename T, bool STAGE, bool TAPS_LDS>
__global__ __launch_bounds__(kBlock) void resample_kernel(const T* __restrict__ in, float* __restrict__ out,
                                                          const float* __restrict__ taps, long long in_stride_frames,
                                                          long long out_stride, int channels, int L, int M, int half, int n_out,
                                                          ResampleRows rows) {
  __shared__ float xs[STAGE ? kResampleWindow : 1];
  __shared__ float hs[TAPS_LDS ? kResampleTapsLds : 1];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int o0 = blockIdx.x * kBlock;
  const int n_blk = min(kBlock, n_out - o0);
  const long long first = rows.in_first[b];
  const int count = rows.in_count[b];
  const T* row = in + (long long)b * in_stride_frames * channels;
  const long long n0 = rows.out_first[b] + o0;
  const long long k_base = ceil_div(n0 * M - half, L);
  if constexpr (STAGE) {
    const int span = (int)(floor_div((n0 + n_blk - 1) * M + half, L) - k_base) + 1;   // <= kResampleWindow (checked by the launcher)
    for (int i = tid; i < span; i += kBlock) xs[i] = load_frame(row, k_base + i, first, count, channels);
  }
  if constexpr (TAPS_LDS) {
    for (int i = tid; i <= 2 * half; i += kBlock) hs[i] = taps[i];
  }
  if constexpr (STAGE || TAPS_LDS) __syncthreads();
  if (tid >= n_blk) return;
  const long long c = (n0 + tid) * M;
  const long long klo = ceil_div(c - half, L), khi = floor_div(c + half, L);
  int t = (int)(c - klo * L) + half;     // tap of the first frame, in [0, 2 half]; the next frame's is L lower
  const int nk = (int)(khi - klo) + 1;
  const int x0 = (int)(klo - k_base);
  float acc = 0.f;
  for (int j = 0; j < nk; ++j, t -= L) {
    float x, h;
    if constexpr (STAGE) x = xs[x0 + j]; else x = load_frame(row, klo + j, first, count, channels);
    if constexpr (TAPS_LDS) h = hs[t]; else h = taps[t];
    acc = fmaf(x, h, acc);
  }
  out[(long long)b * out_stride + o0 + tid] = acc;
}

template <typename T>
hipError_t launch_t(const ResampleArgs& a, hipStream_t st) {
  // the widest window a block can need: its 256 outputs' centres span 255 M / L frames, plus the filter's reach on both sides
  const long long span = (255LL * a.M + 2LL * a.half) / a.L + 2;
  const bool stage = span <= kResampleWindow;
  const bool taps_lds = stage && a.L <= 2 && 2 * a.half + 1 <= kResampleTapsLds;
  const dim3 grid((a.n_out + kBlock - 1) / kBlock, a.B), block(kBlock);
  const T* in = static_cast<const T*>(a.in);
#define TW_RESAMPLE_LAUNCH(S, H)                                                                                          \
  hipLaunchKernelGGL((resample_kernel<T, S, H>), grid, block, 0, st, in, a.out, a.taps, a.in_stride_frames, a.out_stride, \
                     a.channels, a.L, a.M, a.half, a.n_out, a.rows)
  if (taps_lds) TW_RESAMPLE_LAUNCH(true, true);
  else if (stage) TW_RESAMPLE_LAUNCH(true, false);
  else TW_RESAMPLE_LAUNCH(false, false);
#undef TW_RESAMPLE_LAUNCH
  return hipGetLastError();
}

}  // namespace

hipError_t launch_resample(const ResampleArgs& a, hipStream_t st) {
  if (a.B < 1 || a.B > 64 || a.n_out < 1 || a.L < 1 || a.M < 1 || a.half < 0 || a.channels < 1) return hipErrorInvalidValue;
  return a.s16 ? launch_t<short>(a, st) : launch_t<float>(a, st);
}
