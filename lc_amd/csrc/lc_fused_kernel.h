// The pose-unit kernel (loss and solve workgroups in one grid), shared by lc_fused.hip (large grids) and lc_fused_latency.hip
// (small grids: the metric's launch, compiled with the max-ILP machine scheduler, see lc_pnp_latency.hip).
// The plain form runs one-wave workgroups: one pose or one sample each.  The TEAM form (latency build only, LC_PNP_TEAM2) runs 128-thread
// workgroups: a solve workgroup is ONE pose solved by its two wavefronts (lc_pnp_body.h: TeamWave), a loss workgroup is TWO samples, one per
// wavefront, each with its own LossSharedN<1> and no workgroup barrier.  At B = 256 that is 512 solve waves + 256 loss waves on the chip's
// 1024 SIMDs, where the one-wave form leaves half of them idle for the whole launch; it is launched while every wave still gets a SIMD of
// its own (two per pose + one per sample <= kLatencyGridMax: the kernel needs more than half a SIMD's registers).
// Code size: the TEAM kernel is two copies of the solve (one per parity) and the loss body, run side by side by the wavefronts of neighbouring
// compute units that share one 64 KB instruction cache.  The latency build calls the never-taken full-range sincos() instead of inlining it
// into every evaluation (lc_common.h: LC_SINCOS_FALLBACK_CALL): 42 KB against 51 KB.  Folding the three inlined evaluations of a solve copy
// into one loop body (35 KB) was measured 10-14 % SLOWER and is not done; counters, timings and both decisions: profiles/icache2/NOTES.md.
#pragma once
#include "lc_loss_body.h"
#include "lc_pnp_body.h"

namespace lc {
namespace {

union __attribute__((aligned(16))) FusedShared {
    loss::LossShared loss;
    double bc[pnp::kPnpLdsDoubles<1>];
};
union __attribute__((aligned(16))) FusedSharedTeam {
    loss::LossSharedN<1> loss[2];
    double bc[pnp::kPnpTeamLdsDoubles];
};

template <int WPS, bool TEAM = false>  // WPS, see lc_pnp.hip: 1 = latency build for small grids, 2 = occupancy build for large ones
__global__ __launch_bounds__(TEAM ? 128 : 64, WPS) void lc_pose_unit_kernel(const LossParams lp, const PnpParams pp) {
    static_assert(!TEAM || WPS == 1, "two wavefronts per pose where SIMDs idle");
    if constexpr (TEAM) {
        __shared__ FusedSharedTeam sh;
        const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        if ((int)blockIdx.x < pp.B) {
            __builtin_amdgcn_s_setprio(3);  // the solve is the critical path of the launch: its waves win the CU's shared issue/LDS arbitration (measured: scripts/ubench/pnp_ab.py)
            if (wave == 0) pnp::solve_pose<pnp::TeamWave<0>>(pp, blockIdx.x, lane, sh.bc, true);
            else pnp::solve_pose<pnp::TeamWave<1>>(pp, blockIdx.x, lane, sh.bc, false);
        } else {
            const int b = 2 * ((int)blockIdx.x - pp.B) + wave;
            if (b < lp.B) loss::sample<true, false, false, loss::LossSharedN<1>, true>(lp, b, sh.loss[wave]);
        }
    } else {
        __shared__ FusedShared sh;
        if ((int)blockIdx.x < pp.B) {
            __builtin_amdgcn_s_setprio(3);  // the solve is the critical path of the launch: its wave wins the CU's shared issue/LDS arbitration (measured: scripts/ubench/pnp_ab.py)
            pnp::solve_pose<pnp::OneWave<>>(pp, blockIdx.x, threadIdx.x, sh.bc);
        } else {
            loss::sample<true>(lp, (int)blockIdx.x - pp.B, sh.loss);
        }
    }
}

}  // namespace

int launch_pose_unit_latency(const LossParams& lp, const PnpParams& pp, hipStream_t stream);  // at most kLatencyGridMax poses + samples (lc_fused_latency.hip)

}  // namespace lc
