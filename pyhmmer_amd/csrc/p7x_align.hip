// p7x_align.hip -- hmmalign on CDNA4 (upstream p7_tracealign_computeTraces, tracealign.c): env_kernel (p7x_envkernel.hpp)
// in alignment mode, one whole sequence per WAVEFRONT, the profile in unihit local mode with the sequence's own length
// model.
// The host (p7x_tracealign.cpp) repeats every sequence whose status word flags a near-tie on the trace, a posterior
// within the guard of a printed digit's boundary, or a traceback failure, with the host twin in upstream's order.
#include "p7x_envkernel.hpp"

namespace p7x {

int align_max_blocks(int C, int nrows, int num_cu, int *nblocks) { return env_max_blocks_of<EnvMode::Align>(C, nrows, num_cu, nblocks); }
int align_launch(const ArgRun<EnvArgs> &a, hipStream_t st) { return env_launch_of<EnvMode::Align>(a, st); }

} // namespace p7x
