// probe: v_cvt_scalef32_pk_f16_fp8 against f32 widen + RNE f16 cast for every byte x scale byte; f16 MFMA with subnormal operands
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cmath>
#include <vector>
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x2 __attribute__((ext_vector_type(2)));
__global__ void k(unsigned short* direct, float* wide) {
  const int byte = threadIdx.x, sb = blockIdx.x;   // 256 x 256
  const float X = __builtin_bit_cast(float, (unsigned)sb << 23);
  const int src = byte | (byte << 8) | (byte << 16) | (byte << 24);
  f16x2 h = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(src, X, true);
  f32x2 f = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(src, X, false);
  direct[sb * 256 + byte] = __builtin_bit_cast(unsigned short, (_Float16)h[1]);
  wide[sb * 256 + byte] = f[0];
}
// quantiser: cvt_scalef32_pk_fp8_f32 (value / scale, RNE e4m3)
__global__ void kq(const float* in, int n, float X, unsigned* out) {
  int i = threadIdx.x;
  if (i >= n) return;
  s16x2 old = {0, 0};
  s16x2 r = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(old, in[i], 0.f, X, false);
  out[i] = (unsigned)(unsigned short)r[0] & 0xff;
}
// D = A(16x32) . B(32x16): A[row 0][k 0] = a, B[k 0][col 0] = b, everything else zero
__global__ void km(unsigned short abits, float bval, float* out) {
  const int lane = threadIdx.x;
  f16x8 a = {0, 0, 0, 0, 0, 0, 0, 0}, b = {0, 0, 0, 0, 0, 0, 0, 0};
  if (lane == 0) { a[0] = __builtin_bit_cast(_Float16, abits); b[0] = (_Float16)bval; }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc, 0, 0, 0);
  if (lane == 0) out[0] = acc[0];
}
static unsigned short f16_rne(float v) { _Float16 h = (_Float16)v; unsigned short u; __builtin_memcpy(&u, &h, 2); return u; }
int main() {
  unsigned short* d; float* w; float* o;
  if (hipMalloc(&d, 65536 * 2) != hipSuccess || hipMalloc(&w, 65536 * 4) != hipSuccess || hipMalloc(&o, 16) != hipSuccess) return 2;
  hipLaunchKernelGGL(k, dim3(256), dim3(256), 0, 0, d, w);
  std::vector<unsigned short> hd(65536); std::vector<float> hw(65536);
  if (hipMemcpy(hd.data(), d, 65536 * 2, hipMemcpyDeviceToHost) != hipSuccess) return 3;
  if (hipMemcpy(hw.data(), w, 65536 * 4, hipMemcpyDeviceToHost) != hipSuccess) return 3;
  long bad = 0, sub = 0, subnz = 0, nan_skip = 0, ovf = 0; int shown = 0;
  for (int sb = 1; sb < 255; ++sb) for (int b = 0; b < 256; ++b) {
    if ((b & 0x7f) == 0x7f) { ++nan_skip; continue; }
    const float v = hw[sb * 256 + b];
    const float q = (((b >> 3) & 15) == 0 ? ldexpf((float)(b & 7), -9) : ldexpf(1.0f + (b & 7) / 8.0f, ((b >> 3) & 15) - 7)) * ((b & 0x80) ? -1.f : 1.f);
    const float expect = ldexpf(q, sb - 127);
    if (v != expect && shown < 10) { printf("f32 widen differs: sb=%d b=0x%02x got %g want %g\n", sb, b, v, expect); ++shown; }
    if (fabsf(expect) > 65504.f) { ++ovf; continue; }
    const unsigned short want = f16_rne(expect), got = hd[sb * 256 + b];
    const bool is_sub = fabsf(expect) < 6.103515625e-05f && expect != 0.f;
    if (is_sub) { ++sub; if (got & 0x7fff) ++subnz; }
    if (want != got) { ++bad; if (shown < 40) { printf("f16 direct differs: sb=%d b=0x%02x value %g: got 0x%04x want(RNE, gradual) 0x%04x\n", sb, b, expect, got, want); ++shown; } }
  }
  printf("cvt_scalef32_pk_f16_fp8: mismatches vs RNE-with-subnormals = %ld; results below 2^-14: %ld, of which non-zero from hardware: %ld; skipped nan %ld overflow %ld\n", bad, sub, subnz, nan_skip, ovf);
  // overflow behaviour samples
  for (int sb : {140, 143, 150}) printf("overflow sample sb=%d b=0x7e (448 * 2^%d): 0x%04x\n", sb, sb - 127, hd[sb * 256 + 0x7e]);
  // quantiser
  {
    std::vector<float> in = {0.f, 1.f, 1.0625f, 1.125f, 1.1875f, -3.3f, 17.f, 18.f, 19.f, 208.f, 216.f, 255.9f, 0.001f, 0.002f, 0.003f, 0.0009765625f, 1e-5f};
    int n = in.size(); float* di; unsigned* dq; hipMalloc(&di, n * 4); hipMalloc(&dq, n * 4);
    hipMemcpy(di, in.data(), n * 4, hipMemcpyHostToDevice);
    for (float X : {1.0f, 0.25f, 4.0f}) {
      hipLaunchKernelGGL(kq, dim3(1), dim3(64), 0, 0, di, n, X, dq);
      std::vector<unsigned> q(n); if (hipMemcpy(q.data(), dq, n * 4, hipMemcpyDeviceToHost) != hipSuccess) return 4;
      printf("quant scale=%g:", X);
      for (int i = 0; i < n; ++i) printf(" %g->0x%02x", in[i], q[i]);
      printf("\n");
    }
  }
  // MFMA with f16 subnormal A operand
  for (unsigned short ab : {(unsigned short)0x0001, (unsigned short)0x0200, (unsigned short)0x03ff, (unsigned short)0x0400}) {
    hipLaunchKernelGGL(km, dim3(1), dim3(64), 0, 0, ab, 1024.f, o);
    float r = 0; if (hipMemcpy(&r, o, 4, hipMemcpyDeviceToHost) != hipSuccess) return 5;
    _Float16 h; __builtin_memcpy(&h, &ab, 2);
    printf("mfma f16: a=0x%04x (%g) x 1024 -> %g (exact %g)\n", ab, (float)h, r, (float)h * 1024.f);
  }
  return 0;
}
