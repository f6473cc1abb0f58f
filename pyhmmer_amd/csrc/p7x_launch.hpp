// p7x_launch.hpp -- the dynamic-LDS opt-in and the occupancy of a kernel instantiation: the one place where both are asked of
// the runtime (p7x_device.hip).  More than 64 KiB of dynamic LDS must be granted per kernel and per device before a launch
// (and before the occupancy is asked); the grant of a kernel only grows, so an instantiation whose LDS size depends on the
// model (the alphabet's rows) is right whichever model comes first.
#pragma once
#include "p7x_device.hpp"

namespace p7x {

int kernel_grant_lds_fn(const void *kernel, size_t lds_bytes);
int kernel_blocks_per_cu_fn(const void *kernel, int threads, size_t lds_bytes, int *per_cu, size_t grant_bytes, const char *trace);

// The current device grants <kernel> at least <lds_bytes> of dynamic LDS: for the launches that size their grid otherwise.
template <class K> int kernel_grant_lds(K kernel, size_t lds_bytes) { return kernel_grant_lds_fn(reinterpret_cast<const void *>(kernel), lds_bytes); }

// Resident blocks per CU (at least 1) of <kernel> with <threads> per block and <lds_bytes> of dynamic LDS on the current
// device, looked up once per (device, kernel, threads, lds_bytes); the grant is max(lds_bytes, grant_bytes), for a kernel that
// takes its largest size in one step.  <trace>: with option "trace_envelope", the registers and LDS of a first lookup on stderr.
template <class K> int kernel_blocks_per_cu(K kernel, int threads, size_t lds_bytes, int *per_cu, size_t grant_bytes = 0, const char *trace = nullptr)
{ return kernel_blocks_per_cu_fn(reinterpret_cast<const void *>(kernel), threads, lds_bytes, per_cu, grant_bytes, trace); }

} // namespace p7x
