// The one-correspondence-per-lane kernel (N <= 64) of the weighted-PnP solve, shared by lc_pnp.hip (large grids) and lc_pnp_latency.hip (small grids).
#pragma once
#include "lc_pnp_body.h"

namespace lc {
namespace {

// WPS = waves per SIMD the register allocator must allow: 1 for small grids (latency: B <= ~1000 poses leave most SIMDs
// idle anyway, spilling would only lengthen the lone wave), 2 for large grids (+43 % throughput at B = 16384).
// OPTS: honours PnpParams::options / weight_mask (lc_pnp_lm2_f32); the plain instantiations are the ones the metric runs
// TEAM (latency build of the plain solve, LC_PNP_TEAM2): 128-thread workgroups, TWO wavefronts per pose, each with half of the products and of
// the block sum (lc_pnp_body.h: TeamWave); the same bits as the one-wave forms
// REG is always true (one wave has one correspondence per lane).  It stays in the parameter list because the list is part of the kernel's
// mangled name, which tests/launch_forms.py and scripts/kernel_resources.py match.
template <bool REG, int WPS, bool OPTS = false, bool TEAM = false>
__global__ __launch_bounds__(TEAM ? 128 : 64, WPS) void lc_pnp_lm_kernel(const PnpParams p) {
    static_assert(REG, "one wave: one correspondence per lane");
    if constexpr (TEAM) {
        static_assert(WPS == 1 && !OPTS, "two wavefronts per pose where SIMDs idle");
        __shared__ __attribute__((aligned(16))) double bc[pnp::kPnpTeamLdsDoubles];
        const int lane = threadIdx.x & 63;
        if (__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) == 0) pnp::solve_pose<pnp::TeamWave<0>>(p, blockIdx.x, lane, bc, true);
        else pnp::solve_pose<pnp::TeamWave<1>>(p, blockIdx.x, lane, bc, false);
    } else {
        __shared__ __attribute__((aligned(16))) double bc[pnp::kPnpLdsDoubles<1>];
        // WPS == 2 keeps the per-pivot test of the LDL^T (FormDefaults::PIVOTS_RUNNING): with the running form this kernel, and only this
        // one, spills (scripts/kernel_resources.py: scratch 20-28 B).  Once it has two register pairs to spare, pass `true` here and
        // remove the flag and the per-pivot arm of ldlt_solve6: no other kernel uses them.
        pnp::solve_pose<pnp::OneWave<OPTS, WPS == 1>>(p, blockIdx.x, threadIdx.x, bc);
    }
}

}  // namespace

int launch_pnp_lm_latency(const PnpParams& p, hipStream_t stream);  // N <= 64, B <= kLatencyGridMax (lc_pnp_latency.hip)
int launch_pnp_lm_chain_latency(const PnpParams& a, const PnpParams& b, int second_starts_from_first, hipStream_t stream);  // both jobs N <= 64, b.B <= kLatencyGridMax

}  // namespace lc
