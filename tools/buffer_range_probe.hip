// What does a raw buffer load return when the SCALAR offset carries the address past num_records?  All reads stay inside one
// 4 KiB allocation: the descriptor covers its first 256 bytes only.
#include <hip/hip_runtime.h>
#include <cstdio>
__global__ void probe(const float* p, unsigned bytes, unsigned voff, unsigned soff, float* out) {
  __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0, (int)bytes, 0x00020000);
  out[threadIdx.x] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, voff, soff, 0));
}
int main() {
  float h[1024], *d, *o, r;
  for (int i = 0; i < 1024; ++i) h[i] = (float)(i + 1);
  if (hipMalloc(&d, sizeof h) != hipSuccess || hipMalloc(&o, 256) != hipSuccess) return 2;
  if (hipMemcpy(d, h, sizeof h, hipMemcpyHostToDevice) != hipSuccess) return 2;
  const unsigned cases[][2] = {{0, 0}, {252, 0}, {256, 0}, {0, 252}, {0, 256}, {128, 124}, {128, 128}, {4, 252}, {0, 1024}, {0x80000000u, 0}, {0x80000000u, 64}};
  for (auto& c : cases) {
    hipLaunchKernelGGL(probe, dim3(1), dim3(1), 0, 0, d, 256u, c[0], c[1], o);
    if (hipMemcpy(&r, o, 4, hipMemcpyDeviceToHost) != hipSuccess) return 3;
    printf("num_records 256  voffset %10u  soffset %5u  -> %g  (element at voffset+soffset holds %g)\n", c[0], c[1], r,
           (c[0] + c[1]) / 4 < 1024 ? h[(c[0] + c[1]) / 4] : -1.f);
  }
  return 0;
}
