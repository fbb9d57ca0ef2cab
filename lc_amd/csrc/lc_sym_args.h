// Argument rules of the symmetry entry points (lc_sym_select_f32, lc_sym_select_table_f32, lc_sym_candidates_f32), each stated once.
// Pure C++ (no HIP, no allocation, no pointer is dereferenced): lc_capi.hip calls them before a launch, and
// tests/native/sym_args_sanitize.cpp runs them under AddressSanitizer + UBSan on the CPU.  Each returns the message of the first rule
// that is broken, or null.
#pragma once
#include <cstddef>
#include <cstdint>

namespace lc {
namespace host {

constexpr int kSymArgMaxPoints = 1024;  // lc::kSymMaxPoints

// the sizes every selection shares
inline const char* sym_select_size_error(int mode, int B, int N, int H, int W) {
    if (B < 0 || N <= 0 || H < 0 || W < 0) return "bad size";
    if (N > kSymArgMaxPoints) return "more than 1024 check points per sample";
    if (mode != 0 && mode != 1) return "mode must be 0 (2D) or 1 (3D)";
    return nullptr;
}

// the point sources of a selection with at least one row
inline const char* sym_select_points_error(int mode, const void* cam_K, const void* pts_a, const void* pts_b, const void* xyz_map, int map_dtype,
                                           long long map_bstride, const void* noc_scale, const void* homo_z, const void* ck, int B, int H, int W,
                                           const void* Rt_best) {
    if (!cam_K || !Rt_best) return "null pointer";
    if (mode == 0) {
        if (!pts_a || !pts_b) return "2D mode needs pts3d and pts2d";
        return nullptr;
    }
    if (!pts_a && (!xyz_map || !noc_scale)) return "3D mode needs the predicted points or the xyz map with noc_scale";
    if (!pts_b && !homo_z) return "3D mode needs homo_z at the points or the homo_z map";
    if (!pts_a || !pts_b) {
        if (!ck) return "reading a map needs the check pixels";
        if (H <= 0 || W <= 0) return "bad map size";
        const long long hw3 = (long long)H * W >= (1ll << 31) / 3 ? (1ll << 31) : 3ll * H * W;  // (the plain product of four ints can leave 64 bits)
        if (hw3 * B >= (1ll << 31)) return "maps of 2^31 elements or more";
    }
    if (!pts_a) {
        if (map_dtype < 0 || map_dtype > 2) return "map_dtype must be LC_F32, LC_F16 or LC_BF16";
        if (map_bstride < 0 || (map_bstride && map_bstride < 3ll * H * W)) return "batch stride smaller than a sample";
    }
    return nullptr;
}

// the symmetry table and the batch's view of it (B >= 1)
inline const char* sym_table_error(const void* Rt_base, const void* obj_index, const void* sym_tab, const void* obj_off, const void* obj_k, int n_obj,
                                   int sym_rows) {
    if (n_obj <= 0 || sym_rows <= 0) return "the symmetry table needs at least one object and one transform";
    if ((long long)sym_rows >= (1ll << 31) / 12) return "symmetry table of 2^31 elements or more";
    if (!Rt_base || !obj_index || !sym_tab || !obj_off || !obj_k) return "null pointer (base pose, obj_index or symmetry table)";
    if (reinterpret_cast<uintptr_t>(sym_tab) & 7) return "sym_tab must be 8-byte aligned";
    if ((reinterpret_cast<uintptr_t>(Rt_base) | reinterpret_cast<uintptr_t>(obj_index) | reinterpret_cast<uintptr_t>(obj_off) |
         reinterpret_cast<uintptr_t>(obj_k)) & 3)
        return "Rt_base, obj_index, obj_off and obj_k must be 4-byte aligned";
    return nullptr;
}

// the output side of lc_sym_candidates_f32 (B >= 1)
inline const char* sym_candidates_out_error(const void* row_off, const void* out, int out_rows) {
    if (out_rows <= 0 || (long long)out_rows >= (1ll << 31) / 12) return "out_rows must lie in [1, 2^31 / 12)";
    if (!row_off || !out) return "null pointer (row_off or out)";
    if ((reinterpret_cast<uintptr_t>(row_off) | reinterpret_cast<uintptr_t>(out)) & 3) return "row_off and out must be 4-byte aligned";
    return nullptr;
}

}  // namespace host
}  // namespace lc
