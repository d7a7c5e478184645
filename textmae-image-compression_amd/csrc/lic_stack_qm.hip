// tmae_lic_stack's chain at a quantiser step per pixel of the latent grid: the QSTEP = 2
// instantiation of lic_stack_kernel in a translation unit of its own, so that the instantiations of lic_stack.hip and
// lic_stack_q.hip compile without it (lic_stack_kernel.h says why).  tmae_lic_stack validates the arguments and calls
// the launch below when cqm is set.
#undef LSTK_TRACE
#define LSTK_TRACE 0  // timeline builds trace the instantiations of lic_stack.hip, where the trace buffer lives
#include "lic_stack_kernel.h"

int lic_stack_launch_qm(const tmae_lic_stack_args& a, int nwg, hipStream_t stream) {
  hipLaunchKernelGGL((lic_stack_kernel<false, 2>), dim3(nwg), dim3(lstk::NW * 64), 0, stream, a);
  TMAE_LAUNCH_CHECK("tmae_lic_stack");
}
