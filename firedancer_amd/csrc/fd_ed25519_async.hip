/* firedancer_amd/csrc/fd_ed25519_async.hip
 *
 * k_ticket: the completion word of an asynchronous submission
 * (fd_ed25519_amd_submit_*, include/fd_ed25519_amd.h).  The last kernel on
 * the slot's stream stores the submission's ticket to the slot's word in
 * mapped coherent host memory, so that fd_ed25519_amd_async_poll's "not
 * finished yet" is one host load and no runtime call.  A source file of its
 * own: no other kernel's code depends on it (k_tile_persist's spills, the
 * build's guard).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fd_ed25519_kernels.h"

/* One wave, one lane.  Release at system scope: the stream has ordered the
   chunk's kernels before this one; the release makes this wave's view of
   their writes precede the word.  Delivery does not rest on that -- it waits
   for the slot's event -- the word only says when waiting is worth a call. */
__global__ void __launch_bounds__(64)
k_ticket( uint64_t * word, uint64_t ticket ) {
  if( threadIdx.x == 0u ) __hip_atomic_store( word, ticket, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM );
}

int
fd_amd_launch_ticket( void * d_word, uint64_t ticket, hipStream_t stream ) {
  hipLaunchKernelGGL( k_ticket, dim3(1), dim3(64), 0, stream, (uint64_t *)d_word, ticket );
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
