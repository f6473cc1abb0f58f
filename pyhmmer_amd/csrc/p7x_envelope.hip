// p7x_envelope.hip -- rescoring of one domain envelope on CDNA4: env_kernel (p7x_envkernel.hpp) in its two envelope
// modes, protein and long-target.  The host (p7x_domaindef.cpp) turns the trace into the alignment display and applies
// the null2 correction.
#include "p7x_envkernel.hpp"

namespace p7x {

int env_max_blocks(EnvMode mode, int C, int nrows, int num_cu, int *nblocks)
{
  if (mode == EnvMode::Align) return align_max_blocks(C, nrows, num_cu, nblocks);
  return env_max_blocks_of<EnvMode::Envelope>(C, nrows, num_cu, nblocks);      // (long-target: the same, as before)
}

int env_launch(EnvMode mode, const ArgRun<EnvArgs> &a, hipStream_t st)
{
  switch (mode) {
    case EnvMode::Align: return align_launch(a, st);
    case EnvMode::LongTarget: return env_launch_of<EnvMode::LongTarget>(a, st);
    default: return env_launch_of<EnvMode::Envelope>(a, st);
  }
}

} // namespace p7x

#ifdef P7X_ENV_PROFILE
extern "C" int p7x_debug_env_profile(unsigned long long *out8)
{
  unsigned long long zero[8] = { 0 };
  if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(p7x::g_env_prof), sizeof zero) != hipSuccess) return 1;
  return hipMemcpyToSymbol(HIP_SYMBOL(p7x::g_env_prof), zero, sizeof zero) != hipSuccess;
}
#endif
