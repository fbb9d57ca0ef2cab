/*
 * lc_amd models -- C ABI of the per-object model preparation (liblc_amd_models.so, built from lc_amd/csrc/models/).
 *
 * A library of its own, next to liblc_amd.so and its four siblings: the kernels of an offline tool (python -m lc_amd.prep_models); no
 * other ABI is changed by it.
 *
 * What models_info.json (extents, diameter) and the sparse heads' `fps` asset (dataset.py:232-236) hold, from the vertices of a mesh set.
 * verts (total,3); table (n_meshes,4) int32 rows (vert_off, n_vert, face_off, n_face) on the DEVICE and the same rows in HOST memory as
 * table_host: the argument rules are checked from the host copy, the kernels read the device copy; max_verts >= every n_vert,
 * 3 * max_verts < 2^31.  (The host copy is what lets fps_count <= V be refused before a launch: a table on the device alone could only be judged by
 * a kernel or after a wait.)
 * All arithmetic is IEEE fp32, every operation rounded on its own (no FMA), with
 *     d2(a, b) = ((ax-bx)*(ax-bx) + (ay-by)*(ay-by)) + (az-bz)*(az-bz).
 * Per mesh m with vertices v[0..V), V >= 1:
 *   lo, hi (n_meshes,3): component-wise min and max.
 *   diameter (n_meshes,), pair (n_meshes,2) int32: over all pairs i < j the largest d2(v[i], v[j]), ties to the smallest i, then the smallest j;
 *     diameter = sqrt(d2) correctly rounded, pair = (i, j) local to the mesh.  V == 1: diameter 0, pair (0, 0).
 *   fps (n_meshes,fps_count,3), fps_index (n_meshes,fps_count) int32: c = (lo + hi) * 0.5f, mind[v] = d2(v, c); fps_count times:
 *     k = argmax mind (ties: smallest index), record k and v[k], mind[v] = min(mind[v], d2(v, v[k])).  The first n rows of a result are the
 *     n-point result.  fps_count > V is refused.
 * The same inputs give the same bits on every call.  Any output may be NULL: the parts (lo, hi), (diameter, pair) and (fps, fps_index) with
 * both pointers NULL -- or fps_count == 0 -- are not computed.  workspace: lc_model_workspace_bytes(n_meshes, max_verts, fps_count) bytes,
 * 16-byte aligned, = 16 * n_meshes * T (T + 1) / 2 with T = ceil(max_verts / LC_MODEL_DIAM_TILE) for the diameter's tile partials, plus
 * 4 * n_meshes * (max_verts rounded up to 4) when fps_count > 0 and max_verts > LC_MODEL_FPS_RESIDENT (larger meshes keep their distances
 * there); it carries nothing from call to call.  Every rule is checked before anything is launched; up to four launches on `stream`
 * (a hipStream_t passed as void*, NULL = default stream), no wait, graph-capturable.
 * Return value: 0 on success, non-zero on error (lc_amd_models_last_error() gives the text).
 */
#ifndef LC_AMD_MODELS_H
#define LC_AMD_MODELS_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LC_AMD_MODELS_VERSION 1
#define LC_MODEL_DIAM_TILE 256
#define LC_MODEL_FPS_RESIDENT 8192

int lc_amd_models_version(void);
const char *lc_amd_models_last_error(void);
const char *lc_amd_models_source_hash(void);
size_t lc_model_workspace_bytes(int n_meshes, int max_verts, int fps_count);
int lc_model_prepare_f32(const float *verts, const int *table, const int *table_host, int n_meshes, int max_verts, int fps_count, float *lo,
                         float *hi, float *diameter, int *pair, float *fps, int *fps_index, void *workspace, size_t workspace_bytes,
                         void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LC_AMD_MODELS_H */
