// Microbenchmark: what does an exec-masked buffer_load_dwordx4 gather cost?  Diagnostic only
// (not shipped).  cost_x with several planes per thread reloads a (pixel, view)'s taps under a
// divergent branch, in the lanes whose tap floor moved; whether that saves time depends on
// whether the texture path's work follows the active lanes.
//
// The loads are cost_x's: a c8 feature image of 1600 x 1184 pixels (4 chunk images of 32-B
// pixels), two lanes per pixel (lane h takes 16-B half h), a wave = 32 pixels of one row, 4 x 32
// pixel tiles of 256 threads, and per "view" 16 independent loads per lane (4 bilinear taps x 4
// chunks) issued before the first is consumed.  Per view a lane is active or not:
//   run    the active pixels of a wave are one contiguous run (what a moving tap floor gives)
//   quads  the active pixels are single quads (2 pixels = 4 lanes) spread over the wave
// at 100 / 50 / 30 / 10 / 0 % of the lanes.  Reported: device time per wave-load, i.e. launch
// time x CUs / (waves x views x 16), and the time relative to the 100 % mask.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP %s @%d\n", hipGetErrorString(e), __LINE__); exit(1); } } while (0)

constexpr int H = 1184, W = 1600, kChunks = 4, kViews = 6;
constexpr int kRows = 4, kTileW = 32;

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t mix(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}

// npx: active pixels per wave (of 32) for `run`, active quads per wave (of 16) for `quads`
template <bool QUADS>
__global__ void __launch_bounds__(2 * kRows * kTileW) __attribute__((amdgpu_waves_per_eu(4)))
gather(const float* __restrict__ img, float* __restrict__ out, int n) {
  const int tid = threadIdx.x, h = tid & 1, q = tid >> 1;
  const int tiles_x = W / kTileW;
  const int gy = (blockIdx.x / tiles_x) * kRows + q / kTileW, gx = (blockIdx.x % tiles_x) * kTileW + q % kTileW;
  const int HW = H * W;
  const uint32_t bytes = (uint32_t)((size_t)kChunks * HW * 32);
  const __amdgpu_buffer_rsrc_t r =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(img), (short)0, (int)bytes, 0x00020000);
  const int wave = blockIdx.x * (2 * kRows * kTileW / 64) + (tid >> 6), px = q % kTileW;
  float acc = 0.f;
  for (int v = 0; v < kViews; ++v) {
    const uint32_t hsh = mix((uint32_t)wave * kViews + v);
    bool on;
    if (QUADS)
      on = ((5 * (px >> 1) + (int)(hsh & 15)) & 15) < n;     // 5 q mod 16: a spread-out set
    else
      on = (unsigned)(px - (int)(hsh % (uint32_t)(kTileW - n + 1))) < (unsigned)n;
    // a tap position inside the image for every pixel: a shift that grows with the view
    const int x0 = min(gx + 3 + 7 * v, W - 2), y0 = min(gy + 1 + v, H - 2);
    const uint32_t p00 = (uint32_t)(y0 * W + x0);
    if (on) {
      u32x4 t[16];
#pragma unroll
      for (int c = 0; c < kChunks; ++c)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t p = p00 + (uint32_t)(k & 1) + (uint32_t)(k >> 1) * W;
          t[4 * c + k] = __builtin_amdgcn_raw_buffer_load_b128(r, (uint32_t)c * HW * 32u + p * 32u + 16u * h, 0, 0);
        }
#pragma unroll
      for (int i = 0; i < 16; ++i) acc += __uint_as_float(t[i].x) + __uint_as_float(t[i].w);
    }
  }
  out[(size_t)(gy * W + gx) * 2 + h] = acc;
}

int main() {
  const size_t n = (size_t)kChunks * H * W * 8;
  std::vector<float> hs(n);
  uint32_t st = 1;
  for (auto& x : hs) { st = st * 1664525u + 1013904223u; x = ((st >> 8) & 0xFFFF) / 65536.0f - 0.5f; }
  float *img, *out;
  CK(hipMalloc(&img, n * 4)); CK(hipMemcpy(img, hs.data(), n * 4, hipMemcpyHostToDevice));
  CK(hipMalloc(&out, (size_t)H * W * 2 * 4));
  hipDeviceProp_t prop; CK(hipGetDeviceProperties(&prop, 0));
  const int cus = prop.multiProcessorCount;
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const int blocks = (W / kTileW) * (H / kRows), waves = blocks * (2 * kRows * kTileW / 64);
  const int R = 20;
  auto run = [&](bool quads, int cnt) {
    auto go = [&] {
      if (quads) hipLaunchKernelGGL(gather<true>, dim3(blocks), dim3(2 * kRows * kTileW), 0, 0, img, out, cnt);
      else hipLaunchKernelGGL(gather<false>, dim3(blocks), dim3(2 * kRows * kTileW), 0, 0, img, out, cnt);
    };
    for (int i = 0; i < 3; ++i) go();
    CK(hipDeviceSynchronize());
    CK(hipEventRecord(e0));
    for (int i = 0; i < R; ++i) go();
    CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
    float ms; CK(hipEventElapsedTime(&ms, e0, e1));
    return (double)ms / R;
  };
  printf("masked buffer_load_dwordx4 gather, %dx%d c8 image, %d views x 16 loads per lane, %d CUs\n", W, H, kViews, cus);
  printf("%-6s %8s %10s %14s %10s\n", "mask", "active", "ms/launch", "ns/wave-load", "vs 100%");
  const double full = run(false, 32), none = run(false, 0);
  for (int quads = 0; quads < 2; ++quads)
    for (int pct : {100, 50, 30, 10, 0}) {
      const int cnt = quads ? (pct * 16 + 50) / 100 : (pct * 32 + 50) / 100;
      const double ms = run(quads, cnt);
      printf("%-6s %7.1f%% %10.4f %14.3f %10.3f\n", quads ? "quads" : "run", 100.0 * cnt / (quads ? 16 : 32), ms,
             ms * 1e6 * cus / ((double)waves * kViews * 16), ms / full);
    }
  printf("floor (no lane active) %.4f ms; full - floor %.4f ms\n", none, full - none);
  return 0;
}
