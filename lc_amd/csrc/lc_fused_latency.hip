// The metric's launch: the pose-unit kernel for at most kLatencyGridMax poses + samples (B = 256: 256 two-wave solve workgroups and 128
// loss workgroups of two samples each, lc_fused_kernel.h; with -DLC_PNP_TEAM2=0, or beyond 1024 waves of that form, one-wave workgroups), in a
// translation unit of its own because it is compiled with the max-ILP machine scheduler (lc_amd/build.py: PER_FILE_FLAGS; measurements
// and why only here: lc_pnp_latency.hip).  The solve is the critical path of the launch; the loss half, 4 % slower under this
// scheduler when run alone, still finishes well inside it.
#ifndef LC_SINCOS_FALLBACK_CALL
#define LC_SINCOS_FALLBACK_CALL 1  // the never-taken full-range sincos() out of the LM loop's code (lc_common.h: sincos_small)
#endif
#include "lc_fused_kernel.h"

namespace lc {

int launch_pose_unit_latency(const LossParams& lp, const PnpParams& pp, hipStream_t stream) {
    const int samples = lp.B > 0 ? lp.B : 0, poses = pp.B > 0 ? pp.B : 0;
#if LC_PNP_TEAM2
    if (2 * poses + samples <= kLatencyGridMax) hipLaunchKernelGGL((lc_pose_unit_kernel<1, true>), dim3(poses + (samples + 1) / 2), dim3(128), 0, stream, lp, pp);
    else
#endif
    hipLaunchKernelGGL(lc_pose_unit_kernel<1>, dim3(poses + samples), dim3(64), 0, stream, lp, pp);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // namespace lc
