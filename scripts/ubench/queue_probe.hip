// queue_probe.hip -- which HIP streams share a hardware queue, by creation order and priority.
//
// The library creates the streams of its cascades at start-up and lays them out on the assumption that the runtime deals
// streams onto its hardware queues (GPU_MAX_HW_QUEUES of them) round robin in the order they are created, and that streams
// on one queue run one after the other (p7x_device.hpp).  This probe measures that map.  It creates one stream per letter
// of a pattern -- g: greatest priority (the cascade sets, the ensemble tail stream), l: least priority (the envelope tail
// stream), d: default priority (hipStreamCreateWithFlags: the context's two streams, the long-target streams) -- and then
// launches a one-workgroup spin kernel (a fixed number of dependent multiply-adds, no memory traffic) on two streams at the
// same moment: the pair takes as long as one kernel when the streams sit on different queues and twice as long when they
// share one.  Every stream is compared with stream 0 and, for the full map, with one representative of every queue class
// found so far.
//
// output: one line per stream (creation index, priority, queue class, pair time against stream 0 over one kernel's time),
// then the classes by priority and whether the g streams follow class(i) == class(i mod Q).
//
// build: hipcc -O3 --offload-arch=gfx950 -o queue_probe queue_probe.hip
// run:   GPU_MAX_HW_QUEUES=4 ./queue_probe [pattern] [iterations]     (and with 8; the variable is read by the runtime)
#include <hip/hip_runtime.h>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define CHECK(call)                                                                                             \
  do { hipError_t e_ = (call); if (e_ != hipSuccess) {                                                          \
    std::fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_)); std::exit(1); } } while (0)

__global__ void spin_kernel(uint32_t iters, uint32_t seed, uint32_t *sink)
{
  uint32_t x = seed + threadIdx.x;
  for (uint32_t i = 0; i < iters; ++i) x = x * 1664525u + 1013904223u;        // dependent chain: nothing to overlap within the lane
  if (x == 0x9e3779b9u && seed == 0xffffffffu) sink[0] = x;                    // keeps the loop; never taken (seed is small)
}

static double pair_ms(hipStream_t a, hipStream_t b, uint32_t iters, uint32_t *sink)
{
  CHECK(hipDeviceSynchronize());
  const auto t0 = std::chrono::steady_clock::now();
  hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, a, iters, 1u, sink);
  if (b) hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, b, iters, 2u, sink);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// the smaller of two tries: a pair that overlapped once sits on two queues
static double pair_ms2(hipStream_t a, hipStream_t b, uint32_t iters, uint32_t *sink)
{
  const double x = pair_ms(a, b, iters, sink), y = pair_ms(a, b, iters, sink);
  return x < y ? x : y;
}

int main(int argc, char **argv)
{
  const std::string pattern = argc > 1 ? argv[1] : "gggggggggggggggglgdlgdlgdlgd";
  const uint32_t iters = argc > 2 ? (uint32_t) std::strtoul(argv[2], nullptr, 10) : (1u << 19);
  const int n = (int) pattern.size();
  if (n < 2 || n > 64 || pattern.find_first_not_of("gld") != std::string::npos) { std::fprintf(stderr, "pattern: 2..64 letters of g, l, d\n"); return 2; }
  const char *env = std::getenv("GPU_MAX_HW_QUEUES");
  CHECK(hipSetDevice(0));
  int least = 0, greatest = 0;
  CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
  std::printf("GPU_MAX_HW_QUEUES %s; stream priorities: least %d greatest %d; pattern %s; %u iterations\n", env ? env : "(unset)", least, greatest,
              pattern.c_str(), iters);
  uint32_t *sink = nullptr;
  CHECK(hipMalloc(&sink, 256));
  std::vector<hipStream_t> s((size_t) n);
  for (int i = 0; i < n; ++i) {
    if (pattern[(size_t) i] == 'd') CHECK(hipStreamCreateWithFlags(&s[(size_t) i], hipStreamNonBlocking));
    else CHECK(hipStreamCreateWithPriority(&s[(size_t) i], hipStreamNonBlocking, pattern[(size_t) i] == 'g' ? greatest : least));
  }
  for (int i = 0; i < n; ++i) (void) pair_ms(s[(size_t) i], nullptr, 1024, sink);        // first use of every stream, code object loaded
  double one = 1e30;
  for (int k = 0; k < 3; ++k) { const double t = pair_ms(s[0], nullptr, iters, sink); if (t < one) one = t; }
  std::printf("one kernel alone: %.3f ms\n", one);
  const double cut = 1.5 * one;
  std::vector<int> cls((size_t) n, -1), rep;
  std::vector<double> vs0((size_t) n, 0.0);
  for (int i = 0; i < n; ++i) {
    if (i > 0) vs0[(size_t) i] = pair_ms2(s[0], s[(size_t) i], iters, sink);
    for (size_t c = 0; c < rep.size() && cls[(size_t) i] < 0; ++c) {
      const double t = rep[c] == 0 && i > 0 ? vs0[(size_t) i] : pair_ms2(s[(size_t) rep[c]], s[(size_t) i], iters, sink);
      if (t > cut) cls[(size_t) i] = (int) c;
    }
    if (cls[(size_t) i] < 0) { cls[(size_t) i] = (int) rep.size(); rep.push_back(i); }
  }
  std::printf("index prio class  pair_with_0 / one\n");
  for (int i = 0; i < n; ++i)
    std::printf("%5d    %c  %4d  %s%.2f\n", i, pattern[(size_t) i], cls[(size_t) i], i == 0 ? "   -  " : (vs0[(size_t) i] > cut ? "same  " : "other "), i == 0 ? 1.0 : vs0[(size_t) i] / one);
  std::printf("queue classes: %zu\n", rep.size());
  for (const char p : std::string("gld")) {
    std::string line;
    std::vector<char> seen(rep.size(), 0);
    for (int i = 0; i < n; ++i) if (pattern[(size_t) i] == p) { seen[(size_t) cls[(size_t) i]] = 1; line += " " + std::to_string(cls[(size_t) i]); }
    int k = 0; for (const char x : seen) k += x;
    if (!line.empty()) std::printf("classes of the %c streams (in creation order):%s   -- %d different\n", p, line.c_str(), k);
  }
  // round robin among the g streams: with Q classes among them, the i-th g stream has the class of the (i mod Q)-th
  {
    std::vector<int> g;
    for (int i = 0; i < n; ++i) if (pattern[(size_t) i] == 'g') g.push_back(cls[(size_t) i]);
    std::vector<int> first;
    for (const int c : g) { bool have = false; for (const int f : first) have = have || f == c; if (!have) first.push_back(c); }
    const size_t Q = first.size();
    bool rr = true;
    for (size_t i = 0; i < g.size(); ++i) rr = rr && g[i] == g[i % Q];
    std::printf("g streams: %zu queue classes; class(i) == class(i mod %zu) for all of them: %s\n", Q, Q, rr ? "yes" : "NO");
  }
  for (auto q : s) CHECK(hipStreamDestroy(q));
  CHECK(hipFree(sink));
  return 0;
}
