// p7x_devmem.hip -- the two pools all device and pinned memory of the drivers comes from (p7x_devmem.hpp), and the test
// seam that reads their byte counts.
#include "p7x_device.hpp"
#include <map>

namespace p7x {

// Pinned host blocks are recycled through a process-wide pool and never handed back to the runtime: hipHostFree from a
// thread that is winding down (thread_local workspaces) while other threads drive the device is not something the
// runtime tolerates reliably, and the blocks are small.
struct PinnedPool { std::mutex mu; std::multimap<size_t, void *> free; size_t obtained_bytes = 0, free_bytes = 0; };
static PinnedPool &pinned_pool() { static PinnedPool *p = new PinnedPool(); return *p; }      // never destroyed
int pinned_acquire(size_t bytes, void **out, size_t *got)
{
  size_t want = 256;
  while (want < bytes) want *= 2;
  PinnedPool &pp = pinned_pool();
  {
    std::lock_guard<std::mutex> lk(pp.mu);
    auto it = pp.free.find(want);
    if (it != pp.free.end()) { *out = it->second; *got = want; pp.free.erase(it); pp.free_bytes -= want; return P7X_OK; }
  }
  P7X_HIP(hipHostMalloc(out, want, hipHostMallocDefault));
  *got = want;
  std::lock_guard<std::mutex> lk(pp.mu);
  pp.obtained_bytes += want;
  return P7X_OK;
}
void pinned_release(void *p, size_t bytes)
{
  if (!p) return;
  PinnedPool &pp = pinned_pool();
  std::lock_guard<std::mutex> lk(pp.mu);
  pp.free.emplace(bytes, p); pp.free_bytes += bytes;
}

int slab_acquire(DeviceCtx *ctx, size_t bytes, void **out, size_t *got)
{
  const size_t want = ((bytes + 65535) / 65536) * 65536;
  {
    std::lock_guard<std::mutex> lk(ctx->slab_mu);
    auto it = ctx->slab_free.lower_bound(want);
    if (it != ctx->slab_free.end() && it->first <= want * 2) {
      *out = it->second; *got = it->first; ctx->slab_free_bytes -= it->first; ctx->slab_free.erase(it);
      return P7X_OK;
    }
  }
  if (hipMalloc(out, want) != hipSuccess) {
    // the device is full while slabs sit parked: hand the parked ones back and try once more (a pool sized for
    // 288 GiB must not run a smaller device -- or one shared with other processes -- out of memory)
    (void) hipGetLastError();
    std::vector<void *> parked;
    {
      std::lock_guard<std::mutex> lk(ctx->slab_mu);
      for (auto &kv : ctx->slab_free) parked.push_back(kv.second);
      ctx->slab_obtained_bytes -= ctx->slab_free_bytes;
      ctx->slab_free.clear(); ctx->slab_free_bytes = 0;
    }
    for (void *q : parked) (void) hipFree(q);
    P7X_HIP(hipMalloc(out, want));
  }
  *got = want;
  std::lock_guard<std::mutex> lk(ctx->slab_mu);
  ctx->slab_obtained_bytes += want;
  return P7X_OK;
}

void slab_release(DeviceCtx *ctx, void *p, size_t bytes)
{
  if (!p) return;
  std::lock_guard<std::mutex> lk(ctx->slab_mu);
  // keep at most 32 GiB parked (of 288), and never more than an eighth of the device's memory
  size_t cap = (size_t) 32 << 30, free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && total_b / 8 < cap) cap = total_b / 8;
  if (ctx->slab_free_bytes + bytes > cap) { (void) hipFree(p); ctx->slab_obtained_bytes -= bytes; return; }
  ctx->slab_free.emplace(bytes, p); ctx->slab_free_bytes += bytes;
}

} // namespace p7x

using namespace p7x;

extern "C" int p7x_debug_memory_stats(int device, int64_t out[4])
{
  if (!out) { set_error("p7x_debug_memory_stats: bad arguments"); return P7X_EINVAL; }
  DeviceCtx *ctx = nullptr;
  const int st = get_ctx(device, &ctx);
  if (st != P7X_OK) return st;
  { std::lock_guard<std::mutex> lk(ctx->slab_mu); out[0] = (int64_t) ctx->slab_obtained_bytes; out[1] = (int64_t) ctx->slab_free_bytes; }
  PinnedPool &pp = pinned_pool();
  std::lock_guard<std::mutex> lk(pp.mu);
  out[2] = (int64_t) pp.obtained_bytes; out[3] = (int64_t) pp.free_bytes;
  return P7X_OK;
}
