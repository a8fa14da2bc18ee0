// Measurement aid behind fbank.hip.h::fb_logf: the device library's logf and fb_logf on the float32 values of a file.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/probe/fbank_logf_probe.hip -o build/probe_bin/fbank_logf_probe
//   fbank_logf_probe IN.f32 OUT_logf.f32 OUT_fb_logf.f32      (compare both with numpy's float64 log of IN)
// On 2^20 values exp(uniform(-16, 27)): logf up to 2.31 ulp of its result = 35.3 float32 eps of its argument, fb_logf 8.33 eps.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
#include "../../wekws_amd/csrc/fbank.hip.h"
__global__ void k(const float* x, float* a, float* b, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { a[i] = logf(x[i]); b[i] = wekws::fb_logf(x[i]); }
}
int main(int argc, char** argv) {
  if (argc < 4) return 2;
  FILE* f = fopen(argv[1], "rb"); if (!f) return 3;
  fseek(f, 0, SEEK_END); long bytes = ftell(f); fseek(f, 0, SEEK_SET);
  int n = int(bytes / 4); std::vector<float> x(n), a(n), b(n);
  if (fread(x.data(), 4, n, f) != size_t(n)) return 4; fclose(f);
  float *dx, *da, *db;
  if (hipMalloc(&dx, bytes) != hipSuccess || hipMalloc(&da, bytes) != hipSuccess || hipMalloc(&db, bytes) != hipSuccess) return 5;
  hipMemcpy(dx, x.data(), bytes, hipMemcpyHostToDevice);
  hipLaunchKernelGGL(k, dim3((n + 255) / 256), dim3(256), 0, 0, dx, da, db, n);
  if (hipDeviceSynchronize() != hipSuccess) return 6;
  hipMemcpy(a.data(), da, bytes, hipMemcpyDeviceToHost); hipMemcpy(b.data(), db, bytes, hipMemcpyDeviceToHost);
  f = fopen(argv[2], "wb"); fwrite(a.data(), 4, n, f); fclose(f);
  f = fopen(argv[3], "wb"); fwrite(b.data(), 4, n, f); fclose(f);
  printf("logf probe: %d values\n", n);
  return 0;
}
