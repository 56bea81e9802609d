// probe of v_mfma_scale_f32_16x16x128_f8f6f4 with A = e4m3 (cbsz 0), B = e2m1 (blgp 4): k-slot correspondence and scale lanes
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ void probe(float* out, float* sc_b, float* sc_a, float* swapped) {
  const int lane = threadIdx.x, i = lane & 15, g = lane >> 4;
  for (int a = 0; a < 128; ++a) {
    i32x8 A = {0, 0, 0, 0, 0, 0, 0, 0};
    if (i == 0 && g == a / 32) A[(a % 32) / 4] = 0x38 << (8 * (a % 4));
    for (int b = 0; b < 128; ++b) {
      i32x8 B = {0, 0, 0, 0, 0, 0, 0, 0};
      if (i == 0 && g == b / 32) B[(b % 32) / 8] = 0x2 << (4 * (b % 8));
      f32x4 c = {0.f, 0.f, 0.f, 0.f};
      c = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(A, B, c, 0, 4, 0, 127, 0, 127);
      if (lane == 0) out[a * 128 + b] = c[0];
      // swapped roles: A = fp4 (cbsz 4), B = fp8 (blgp 0)
      f32x4 d = {0.f, 0.f, 0.f, 0.f};
      d = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(B, A, d, 4, 0, 0, 127, 0, 127);
      if (lane == 0) swapped[a * 128 + b] = d[0];
    }
  }
  // scales: B one-hot at slot s of column 0, A all ones in row 0; scale_b = 128 in ONE lane (16 gs + 0), or in lane 16 gs + 1 (variant 1)
  for (int s = 0; s < 128; ++s) {
    i32x8 A = {0, 0, 0, 0, 0, 0, 0, 0};
    if (i == 0) A = i32x8{0x38383838, 0x38383838, 0x38383838, 0x38383838, 0x38383838, 0x38383838, 0x38383838, 0x38383838};
    i32x8 B = {0, 0, 0, 0, 0, 0, 0, 0};
    if (i == 0 && g == s / 32) B[(s % 32) / 8] = 0x2 << (4 * (s % 8));
    for (int gs = 0; gs < 4; ++gs)
      for (int v = 0; v < 2; ++v) {
        const int sb = lane == 16 * gs + v ? 128 : 127;
        f32x4 c = {0.f, 0.f, 0.f, 0.f};
        c = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(A, B, c, 0, 4, 0, 127, 0, sb);
        if (lane == 0) sc_b[(s * 4 + gs) * 2 + v] = c[0];
      }
    // A one-hot at byte slot s of row 0, B all ones in column 0; scale_a = 128 in one lane
    i32x8 A1 = {0, 0, 0, 0, 0, 0, 0, 0};
    if (i == 0 && g == s / 32) A1[(s % 32) / 4] = 0x38 << (8 * (s % 4));
    i32x8 B1 = {0, 0, 0, 0, 0, 0, 0, 0};
    if (i == 0) B1 = i32x8{0x22222222, 0x22222222, 0x22222222, 0x22222222, 0, 0, 0, 0};
    for (int gs = 0; gs < 4; ++gs)
      for (int v = 0; v < 2; ++v) {
        const int sa = lane == 16 * gs + v ? 128 : 127;
        f32x4 c = {0.f, 0.f, 0.f, 0.f};
        c = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(A1, B1, c, 0, 4, 0, sa, 0, 127);
        if (lane == 0) sc_a[(s * 4 + gs) * 2 + v] = c[0];
      }
  }
}

int main(int argc, char** argv) {
  float *out, *scb, *sca, *sw;
  if (hipMalloc(&out, 128 * 128 * 4) != hipSuccess) return 2;
  hipMalloc(&sw, 128 * 128 * 4);
  hipMalloc(&scb, 128 * 8 * 4);
  hipMalloc(&sca, 128 * 8 * 4);
  hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, out, scb, sca, sw);
  if (hipDeviceSynchronize() != hipSuccess) { printf("sync failed\n"); return 3; }
  std::vector<float> h(128 * 128), hs(128 * 128), hb(1024), ha(1024);
  hipMemcpy(h.data(), out, h.size() * 4, hipMemcpyDeviceToHost);
  hipMemcpy(hs.data(), sw, hs.size() * 4, hipMemcpyDeviceToHost);
  hipMemcpy(hb.data(), scb, 4096, hipMemcpyDeviceToHost);
  hipMemcpy(ha.data(), sca, 4096, hipMemcpyDeviceToHost);
  FILE* f = argc > 1 ? fopen(argv[1], "w") : stdout;
  if (!f) f = stdout;
  for (int which = 0; which < 2; ++which) {
    const std::vector<float>& m = which ? hs : h;
    fprintf(f, which ? "swapped (A fp4, B fp8): for B-format fp4 slot b, the fp8 slot a\n" : "A fp8, B fp4: for fp4 slot b (g * 32 + nibble), the fp8 slot a (g * 32 + byte)\n");
    for (int b = 0; b < 128; ++b) {
      int cnt = 0, at = -1;
      float val = 0;
      for (int a = 0; a < 128; ++a)
        if (m[a * 128 + b] != 0.f) { ++cnt; at = a; val = m[a * 128 + b]; }
      fprintf(f, "%d%s%s ", at, cnt == 1 && val == 1.f ? "" : "!", (b % 32 == 31) ? "\n" : "");
    }
  }
  fprintf(f, "scale_b: per fp4 slot s, the (lane group, lane-in-group variant) whose scale register doubled the result\n");
  for (int s = 0; s < 128; ++s) {
    for (int j = 0; j < 8; ++j)
      if (hb[s * 8 + j] == 2.f) fprintf(f, "%d.%d", j / 2, j % 2);
      else if (hb[s * 8 + j] != 1.f) fprintf(f, "?%g", hb[s * 8 + j]);
    fprintf(f, s % 32 == 31 ? "\n" : " ");
  }
  fprintf(f, "scale_a: per fp8 slot s likewise\n");
  for (int s = 0; s < 128; ++s) {
    for (int j = 0; j < 8; ++j)
      if (ha[s * 8 + j] == 2.f) fprintf(f, "%d.%d", j / 2, j % 2);
      else if (ha[s * 8 + j] != 1.f) fprintf(f, "?%g", ha[s * 8 + j]);
    fprintf(f, s % 32 == 31 ? "\n" : " ");
  }
  if (f != stdout) fclose(f);
  printf("probe done\n");
  return 0;
}
