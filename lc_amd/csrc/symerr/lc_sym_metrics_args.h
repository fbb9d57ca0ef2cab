// Argument rules and workspace size of the symmetry-aware pose errors (lc_sym_pose_errors_f32, lc_sym_pose_errors_workspace_bytes), each
// stated once.  Pure C++ (no HIP, no allocation, no pointer is dereferenced): lc_sym_metrics.hip calls them before a launch and
// takes its chunking from here, and tests/native/sym_metrics_args_sanitize.cpp runs them under AddressSanitizer + UBSan on the CPU.
// The table's own rules are sym_table_error of ../lc_sym_args.h.  Each rule function returns the message of the first rule that is broken, or null.
#pragma once
#include <cstddef>
#include <cstdint>

namespace lc {
namespace host {

constexpr int kSymErrChunk = 8;  // symmetries per workgroup: four wavefronts, two symmetries each

// workgroups per pose of a launch whose largest object has max_k transforms (max_k >= 1)
inline long long sym_errors_chunks(int max_k) { return ((long long)max_k + kSymErrChunk - 1) / kSymErrChunk; }

// per pose: (mssd, mspd) keys of every chunk, 8 bytes each, then the pose's proj as a double.  0 for an empty batch or a bad size.
inline size_t sym_errors_workspace_bytes(int B, int max_k) {
    if (B <= 0 || max_k <= 0) return 0;
    return (size_t)B * (2 * (size_t)sym_errors_chunks(max_k) + 1) * 8;
}

// the sizes (checked before B == 0 returns)
inline const char* sym_errors_size_error(int B, int P, int max_k) {
    if (B < 0 || P < 0 || max_k < 0) return "bad size";
    if ((long long)P >= (1ll << 31) / 3) return "pts of 2^31 elements or more";
    if (B > 0 && max_k > 0 && (long long)B * sym_errors_chunks(max_k) >= (1ll << 31)) return "B x chunks of max_k of 2^31 or more";
    return nullptr;
}

// everything but the table, for B >= 1
inline const char* sym_errors_args_error(const void* R_est, const void* t_est, const void* R_gt, const void* t_gt, const void* cam_K, const void* pts,
                                         const void* pts_off, const void* pts_cnt, int P, int max_k, int B, const void* err, const void* arg,
                                         const void* workspace, size_t workspace_bytes) {
    if (P <= 0) return "pts needs at least one vertex";
    if (max_k <= 0) return "max_k must be at least 1";
    if (!R_est || !t_est || !R_gt || !t_gt || !cam_K || !pts || !err || !arg) return "null pointer (pose, cam_K, pts, err or arg)";
    if ((pts_off == nullptr) != (pts_cnt == nullptr)) return "pts_off and pts_cnt go together";
    if ((reinterpret_cast<uintptr_t>(R_est) | reinterpret_cast<uintptr_t>(t_est) | reinterpret_cast<uintptr_t>(R_gt) | reinterpret_cast<uintptr_t>(t_gt) |
         reinterpret_cast<uintptr_t>(cam_K) | reinterpret_cast<uintptr_t>(pts) | reinterpret_cast<uintptr_t>(pts_off) | reinterpret_cast<uintptr_t>(pts_cnt) |
         reinterpret_cast<uintptr_t>(err) | reinterpret_cast<uintptr_t>(arg)) & 3)
        return "poses, cam_K, pts, pts_off, pts_cnt, err and arg must be 4-byte aligned";
    if (!workspace) return "null workspace (lc_sym_pose_errors_workspace_bytes)";
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return "workspace must be 8-byte aligned";
    if (workspace_bytes < sym_errors_workspace_bytes(B, max_k)) return "workspace smaller than lc_sym_pose_errors_workspace_bytes(B, max_k)";
    return nullptr;
}

}  // namespace host
}  // namespace lc
