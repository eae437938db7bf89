// What does an event between two dependent kernels of one stream cost?  Two 128-workgroup kernels of ~50 us each, 200 pairs:
//   0   nothing between them
//   a   hipEventRecord between them (a marker packet of its own; the next dispatch waits for it)
//   b   the first kernel launched with hipExtLaunchKernelGGL(..., stopEvent): the event is bound to the kernel's own completion
//   b2  as b, and a second stream waits for the event (hipStreamWaitEvent + a small kernel) - the use the env step would make
// Per variant: HIP-event time of the 200 pairs / 200, and the gap seen on the device (last workgroup of kernel 1 out ->
// first workgroup of kernel 2 in, wall_clock64 ticks of 10 ns), mean over the pairs.
// hipcc -O2 --offload-arch=gfx950 tools/micro/event_gap.hip -o tools/micro/bin/event_gap && tools/micro/bin/event_gap
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x)                                                                            \
  do {                                                                                   \
    hipError_t e_ = (x);                                                                 \
    if (e_ != hipSuccess) {                                                              \
      std::fprintf(stderr, "%s: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__);   \
      std::exit(1);                                                                      \
    }                                                                                    \
  } while (0)

constexpr int NWG = 128, PAIRS = 200, TICKS = 5000;   // 5000 ticks of the 100 MHz wall clock = 50 us

// stamps[2 * blockIdx.x] = first tick seen, [2 * blockIdx.x + 1] = last; the spin is bounded by an iteration count as well
__global__ void spin_kernel(long long* stamps, int ticks) {
  const long long t0 = wall_clock64();
  long long t = t0;
  for (int i = 0; i < (1 << 22) && t - t0 < ticks; ++i) t = wall_clock64();
  if (threadIdx.x == 0) {
    stamps[2 * blockIdx.x] = t0;
    stamps[2 * blockIdx.x + 1] = t;
  }
}
__global__ void tiny_kernel(int* p) {
  if (threadIdx.x == 0 && blockIdx.x == 0) p[0] += 1;
}

int main() {
  hipStream_t s1, s2;
  CK(hipStreamCreateWithFlags(&s1, hipStreamNonBlocking));
  CK(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
  long long* stamps;   // [PAIRS][2 kernels][NWG][2]
  int* cnt;
  const size_t per = 2 * NWG;
  CK(hipMalloc(&stamps, sizeof(long long) * PAIRS * 2 * per));
  CK(hipMalloc(&cnt, sizeof(int)));
  CK(hipMemset(cnt, 0, sizeof(int)));
  std::vector<long long> h(PAIRS * 2 * per);
  hipEvent_t t0, t1, mid;
  CK(hipEventCreate(&t0));
  CK(hipEventCreate(&t1));
  CK(hipEventCreateWithFlags(&mid, hipEventDisableTiming));
  const char* names[4] = {"0  (no event)", "a  (hipEventRecord)", "b  (event on the kernel)", "b2 (event on the kernel + waiting stream)"};
  for (int rep = 0; rep < 2; ++rep) {        // rep 0: warm-up of every variant
    for (int var = 0; var < 4; ++var) {
      CK(hipMemsetAsync(stamps, 0, sizeof(long long) * PAIRS * 2 * per, s1));
      CK(hipStreamSynchronize(s1));
      CK(hipEventRecord(t0, s1));
      for (int p = 0; p < PAIRS; ++p) {
        long long* a = stamps + (size_t)(2 * p) * per;
        long long* b = a + per;
        if (var <= 1) {
          hipLaunchKernelGGL(spin_kernel, dim3(NWG), dim3(64), 0, s1, a, TICKS);
          if (var == 1) CK(hipEventRecord(mid, s1));
        } else {
          hipExtLaunchKernelGGL(spin_kernel, dim3(NWG), dim3(64), 0, s1, nullptr, mid, 0, a, TICKS);
          if (var == 3) {
            CK(hipStreamWaitEvent(s2, mid, 0));
            hipLaunchKernelGGL(tiny_kernel, dim3(1), dim3(64), 0, s2, cnt);
          }
        }
        hipLaunchKernelGGL(spin_kernel, dim3(NWG), dim3(64), 0, s1, b, TICKS);
      }
      CK(hipEventRecord(t1, s1));
      CK(hipEventSynchronize(t1));
      CK(hipStreamSynchronize(s2));
      CK(hipGetLastError());
      float ms = 0.f;
      CK(hipEventElapsedTime(&ms, t0, t1));
      CK(hipMemcpy(h.data(), stamps, sizeof(long long) * h.size(), hipMemcpyDeviceToHost));
      double gap = 0.0, dur = 0.0, next = 0.0;
      for (int p = 0; p < PAIRS; ++p) {
        const long long* a = h.data() + (size_t)(2 * p) * per;
        const long long* b = a + per;
        long long a_in = a[0], a_out = a[1], b_in = b[0], b_out = b[1];
        for (int w = 1; w < NWG; ++w) {
          a_in = std::min(a_in, a[2 * w]);
          a_out = std::max(a_out, a[2 * w + 1]);
          b_in = std::min(b_in, b[2 * w]);
          b_out = std::max(b_out, b[2 * w + 1]);
        }
        gap += (b_in - a_out) * 0.01;
        dur += ((a_out - a_in) + (b_out - b_in)) * 0.005;
        if (p + 1 < PAIRS) {
          const long long* c = b + per;
          long long c_in = c[0];
          for (int w = 1; w < NWG; ++w) c_in = std::min(c_in, c[2 * w]);
          next += (c_in - b_out) * 0.01;
        }
      }
      if (rep)
        std::printf("%-44s %8.2f us per pair (HIP events) | on the device: kernel %6.2f us, gap inside the pair %6.2f us, "
                    "gap to the next pair %6.2f us\n", names[var], ms * 1e3 / PAIRS, dur / PAIRS, gap / PAIRS, next / (PAIRS - 1));
    }
  }
  return 0;
}
