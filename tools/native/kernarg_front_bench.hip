// kernarg_front_bench.hip — what the kernarg fetch at the head of a launch costs on MI355X (round 11: kernarg preloading).
// The kernel has k_classify's shape of front: 196 blocks x 512 threads, seven pointers and an int; it loads one word through
// each pointer, adds them and stores the sum through the last.  2 000 launches go back to back on one stream, each reading what the one before
// wrote (the output rotates through the seven buffers), timed with one event pair around the whole train.
// Built twice, the second time with the leading arguments delivered in SGPRs at wave launch:
//   hipcc -O3 --offload-arch=gfx950 tools/native/kernarg_front_bench.hip -o tools/native/kernarg_front_bench
//   hipcc -O3 --offload-arch=gfx950 -mllvm -amdgpu-kernarg-preload-count=16 tools/native/kernarg_front_bench.hip -o tools/native/kernarg_front_bench_preload
//   run them alternating; each prints one line per train: the per-launch time in us
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

constexpr int kBlocks = 196, kThreads = 512, kN = kBlocks * kThreads, kBufs = 7;

// n stands in front of the last pointer: six pointers and the int are what the user SGPRs left beside the kernarg pointer hold
// (14 dwords), so the six loads and the bounds check can go out while the seventh pointer is still being fetched
__global__ void __launch_bounds__(kThreads) k_front(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, const uint32_t* __restrict__ c,
                                                    const uint32_t* __restrict__ d, const uint32_t* __restrict__ e, const uint32_t* __restrict__ f,
                                                    int n, uint32_t* __restrict__ g) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n) g[i] = a[i] + b[i] + c[i] + d[i] + e[i] + f[i] + g[i];
}

int main(int argc, char** argv) {
  const int launches = argc > 1 ? atoi(argv[1]) : 2000;
  const int trains = argc > 2 ? atoi(argv[2]) : 5;
  uint32_t* buf[kBufs];
  for (int k = 0; k < kBufs; ++k) {
    CK(hipMalloc(&buf[k], kN * 4));
    CK(hipMemset(buf[k], k + 1, kN * 4));
  }
  hipStream_t s; CK(hipStreamCreate(&s));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  // launch l adds the other six buffers into buffer l % 7, the newest (launch l - 1's output) among them
  auto train = [&](int count) {
    for (int l = 0; l < count; ++l) {
      const int o = l % kBufs;
      hipLaunchKernelGGL(k_front, dim3(kBlocks), dim3(kThreads), 0, s, buf[(o + 6) % kBufs], buf[(o + 5) % kBufs], buf[(o + 4) % kBufs],
                         buf[(o + 3) % kBufs], buf[(o + 2) % kBufs], buf[(o + 1) % kBufs], kN, buf[o]);
    }
  };
  train(200);
  CK(hipStreamSynchronize(s));
  for (int t = 0; t < trains; ++t) {
    CK(hipEventRecord(e0, s));
    train(launches);
    CK(hipEventRecord(e1, s));
    CK(hipEventSynchronize(e1));
    CK(hipGetLastError());
    float ms; CK(hipEventElapsedTime(&ms, e0, e1));
    std::printf("train %d: %d launches, %.3f us per launch\n", t, launches, ms * 1e3f / launches);
  }
  return 0;
}
