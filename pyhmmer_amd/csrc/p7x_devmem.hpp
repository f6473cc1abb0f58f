// p7x_devmem.hpp -- who owns device and pinned memory: the two pools it comes from, one owning buffer type for each, and
// the pool that the drivers lease their buffer sets from.
//
// hipMalloc / hipFree / hipHostFree wait for every stream of the device, i.e. for the cascades of all the other searches
// in flight, so the drivers never call them: memory comes from two pools (p7x_devmem.hip) that park what is given back
// and hand it out again, and the objects that hold it are leased from process-wide pools that are never torn down (no
// device memory, stream or event is destroyed from a thread that is exiting, or at process exit).
#pragma once
#include "p7x_internal.hpp"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <mutex>
#include <vector>

namespace p7x {

struct DeviceCtx;
// device blocks of a context's slab pool (64 KiB granules; a parked block of up to twice the size is taken again)
int slab_acquire(DeviceCtx *ctx, size_t bytes, void **out, size_t *got);
void slab_release(DeviceCtx *ctx, void *p, size_t bytes);
// pinned host blocks of the process-wide pool (powers of two from 256 bytes; never handed back to the runtime)
int pinned_acquire(size_t bytes, void **out, size_t *got);
void pinned_release(void *p, size_t bytes);

// A block of one of the pools and the capacity the pool returned for it; the block goes back to its pool with the buffer.
// Move-only.  No object of these types may have static storage duration: the pools are leaked singletons so that nothing
// touches the runtime at process exit.
class PoolBuf {
public:
  PoolBuf() = default;
  PoolBuf(PoolBuf &&o) noexcept : ctx_(o.ctx_), p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  PoolBuf &operator=(PoolBuf &&o) noexcept
  {
    if (this != &o) { reset(); ctx_ = o.ctx_; p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
    return *this;
  }
  ~PoolBuf() { reset(); }
  void reset()
  {
    if (p_) { if (ctx_) slab_release(ctx_, p_, cap_); else pinned_release(p_, cap_); }
    p_ = nullptr; cap_ = 0;
  }
  template <class T> T *as() const { return static_cast<T *>(p_); }
  size_t capacity() const { return cap_; }

protected:
  // Room for <need> bytes: nothing when they fit, else the old block goes back and one of max(need, grow_to) bytes is
  // taken (the sites' growth policies are measured choices and stay with them).  On failure the buffer is empty.
  int grow(DeviceCtx *ctx, size_t need, size_t grow_to)
  {
    if (need <= cap_) return P7X_OK;
    reset();
    ctx_ = ctx;
    const size_t want = std::max(need, grow_to);
    const int st = ctx ? slab_acquire(ctx, want, &p_, &cap_) : pinned_acquire(want, &p_, &cap_);
    if (st != P7X_OK) { p_ = nullptr; cap_ = 0; }
    return st;
  }

private:
  DeviceCtx *ctx_ = nullptr;      // the context whose slab pool the block is from; nullptr: the pinned pool
  void *p_ = nullptr;
  size_t cap_ = 0;
};
struct DeviceBuf : PoolBuf {
  int reserve(DeviceCtx *ctx, size_t need_bytes, size_t grow_to_bytes = 0)
  {
    if (!ctx) { set_error("DeviceBuf::reserve: no device context"); return P7X_EINVAL; }
    return grow(ctx, need_bytes, grow_to_bytes);
  }
};
struct PinnedBuf : PoolBuf {
  int reserve(size_t need_bytes, size_t grow_to_bytes = 0) { return grow(nullptr, need_bytes, grow_to_bytes); }
};

namespace detail {      // T::on_return(), where a T has one: what a lease gives back besides the object (a stream set)
template <class T> auto returned(T &o, int) -> decltype(o.on_return(), void()) { o.on_return(); }
template <class T> void returned(T &, long) {}
}

// The objects of type T (a set of buffers with an <int device>, a stream, events) of the process, each with a busy mark:
// a driver leases one for its device, grows what is too small, and gives it back.  One pool per T, never destroyed.
template <class T> class LeasePool {
  struct Slot { T obj; bool busy = true; };

public:
  static LeasePool &instance() { static LeasePool *p = new LeasePool(); return *p; }

  // Move-only handle: the object goes back to the pool with it.
  class Lease {
  public:
    Lease() = default;
    Lease(Lease &&o) noexcept : s_(o.s_) { o.s_ = nullptr; }
    Lease &operator=(Lease &&o) noexcept { if (this != &o) { reset(); s_ = o.s_; o.s_ = nullptr; } return *this; }
    ~Lease() { reset(); }
    void reset() { if (s_) instance().give_back(s_); s_ = nullptr; }
    void discard() { if (s_) instance().drop(s_); s_ = nullptr; }     // an object that could not be completed: destroyed, not pooled
    T *get() const { return s_ ? &s_->obj : nullptr; }
    T *operator->() const { return &s_->obj; }
    T &operator*() const { return s_->obj; }
    explicit operator bool() const { return s_ != nullptr; }

  private:
    friend class LeasePool;
    explicit Lease(Slot *s) : s_(s) {}
    Slot *s_ = nullptr;
  };

  // The free object of <device> that <better> prefers: better(a, b) tells whether a is to be taken rather than b, the
  // best one so far (nullptr: none yet -- so it also says whether a will do at all).  A new, default-constructed one
  // when none is free.
  template <class Better> Lease lease(int device, Better better)
  {
    std::lock_guard<std::mutex> lk(mu_);
    Slot *best = nullptr;
    for (Slot *s : all_)
      if (!s->busy && s->obj.device == device && better(const_cast<const T &>(s->obj), best ? &best->obj : (const T *) nullptr)) best = s;
    if (!best) { best = new Slot(); best->obj.device = device; all_.push_back(best); }
    best->busy = true;
    return Lease(best);
  }
  // every object of <device>, leased or not
  template <class F> void for_each(int device, F f)
  {
    std::lock_guard<std::mutex> lk(mu_);
    for (Slot *s : all_) if (s->obj.device == device) f(const_cast<const T &>(s->obj));
  }

private:
  void give_back(Slot *s)
  {
    detail::returned(s->obj, 0);
    std::lock_guard<std::mutex> lk(mu_);
    s->busy = false;
  }
  void drop(Slot *s)
  {
    { std::lock_guard<std::mutex> lk(mu_); all_.erase(std::find(all_.begin(), all_.end(), s)); }
    detail::returned(s->obj, 0);
    delete s;
  }
  std::mutex mu_;
  std::vector<Slot *> all_;
};
template <class T> using Lease = typename LeasePool<T>::Lease;

// the end of a lease whose object carries a stream: whatever is queued on it finishes first
template <class L> void sync_and_return(L &l)
{
  if (!l) return;
  if (l->stream) (void) hipStreamSynchronize(l->stream);
  l.reset();
}

} // namespace p7x
