// swb_wide.hip -- the cover kernels of canvases wider than 320 px (20 words of 32 pixels per canvas row).
//
// A translation unit of its own because it is compiled with another instruction scheduler than swb.hip
// (-amdgpu-sched-strategy=iterative-ilp, see spriteworld_amd/build.py for the flags and the measurements).
#define SWB_WIDE_TU 1
#include "swb_kernels.hip.inc"
#include "swb_pow.hip.inc"

template __global__ void swb_cover_kernel<20, false>(const swb_params);
// ... and the build with live sprite overrides (swb_set_sprite_attr)
template __global__ void swb_cover_kernel<20, true>(const swb_params);

// The builds of handles with task sets (swb_set_task_sets), at EVERY width, and their two small kernels
// (swb_ms_state_sets_kernel, swb_env_task_sets_kernel: defined by swb_kernels.hip.inc in this unit).  They live here, behind
// the wide kernels, so that the code object of swb.hip -- every kernel a handle without task sets launches up to 320 px -- is
// byte for byte what it was before there were task sets: text, addresses, descriptors, metadata.
template __global__ void swb_cover_sets_kernel<2, false>(const swb_params);
template __global__ void swb_cover_sets_kernel<2, true>(const swb_params);
template __global__ void swb_cover_sets_kernel<4, false>(const swb_params);
template __global__ void swb_cover_sets_kernel<5, false>(const swb_params);
template __global__ void swb_cover_sets_kernel<10, false>(const swb_params);
template __global__ void swb_cover_sets_kernel<20, false>(const swb_params);
