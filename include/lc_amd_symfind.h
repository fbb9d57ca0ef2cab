/*
 * lc_amd symfind -- C ABI of the symmetry deviation of a model (liblc_amd_symfind.so, built from lc_amd/csrc/symfind/).
 *
 * A library of its own, next to liblc_amd.so and its siblings: the kernels of an offline tool (python -m lc_amd.prep_models
 * --check-symmetries / --symmetries); no other ABI is changed by it.
 *
 * BOP's rule for a symmetry (the BOP 2020 challenge paper, section 2.3): a rigid transform S is a potential symmetry of a model when the
 * deviation between its vertices and its transformed vertices stays below max(15 mm, 0.1 diameter).  This library computes the directed
 * deviation max_i min_j |S x_i - v_j| of many transforms of many meshes in one call; whoever wants the Hausdorff deviation passes S and its
 * inverse as two rows and takes the larger result.
 *
 * INPUTS.  verts (total_verts,3) fp32; mesh_table (n_meshes,4) int32 rows (vert_off, n_vert, face_off, n_face) on the DEVICE and the same rows
 * in HOST memory as mesh_table_host: the argument rules are checked from the host copy (vert_off >= 0, 0 <= n_vert <= max_verts,
 * vert_off + n_vert <= total_verts, 3 * max_verts < 2^31), the kernels read the device copy and check it again.  Faces are not read.
 * table (total_rows,12) fp64 on the DEVICE: a transform per row as a row-major 3 x 4 [R | t], the layout of lc_amd.symmetry.SymmetrySet.
 * Jobs, all int32 on the DEVICE, g in [0, n_jobs): mesh_index[g]; row_off[g], row_k[g]: the job's rows of `table`; and, unless query_idx is
 * NULL, query_off[g], query_n[g]: the job's entries of query_idx (total_queries,), each a vertex index local to the job's mesh.  With
 * query_idx NULL (query_off, query_n are then not read) the queries of a job are all vertices of its mesh, in order.  A query's POSITION
 * is its place in the job's list, its INDEX the vertex it names; without a list the two are equal.
 *
 * THE DEFINITION.  For job g, row k with entries R[3][3], t[3], and the query vertex (x, y, z), fp32 widened exactly to fp64:
 *     p[r] = fp32( ((R[r][0]*x + R[r][1]*y) + R[r][2]*z) + t[r] )          r = 0, 1, 2
 * every fp64 operation rounded on its own, nothing fused, ONE final rounding to fp32 -- an exact symmetry of a mesh on a lattice scores
 * exactly 0 even with 1e-16 of noise in R.  For target vertex v_j of the same mesh, in fp32, every operation rounded on its own (no FMA):
 *     dx = p.x - v_j.x (dy, dz alike),  d2(i, j) = (dx*dx + dy*dy) + dz*dz
 *     n_i   = min_j d2(i, j), its witness the lowest j that has it;
 *     score = max_i n_i over the queries, its witness the lowest query POSITION that has it.
 * NaN: a NaN d2 never wins a min -- n_i is the minimum of the d2 that are not NaN, +inf if there is none, and then (no d2 equals n_i) the
 * witness is target 0.  n_i is therefore never NaN, and the max meets no NaN.  (A d2 is a sum of squares: never -0, so non-negative
 * floats order as their bits.)  min and max are exact: the result does not depend on how vertices, queries, rows or jobs are split.
 *
 * OUTPUTS, each (n_jobs, max_k), entry g * max_k + k for row k < row_k[g] of job g: dev2 fp32 the score, arg_query int32 the INDEX of the
 * witness query, arg_target int32 the witness target of that query.  Every entry is first set to -1 (dev2 -1.0f), and stays so for
 * k >= row_k[g], for a job with no vertices or no queries (or whose queries were all skipped), and for a refused job.  info (n_jobs,)
 * int32: 0; -1 for a job refused on the device -- mesh_index outside [0, n_meshes), a mesh row that leaves verts or exceeds max_verts,
 * row_off < 0, row_k outside [0, max_k], row_off + row_k > total_rows, query_off < 0, query_n outside [0, max_queries],
 * query_off + query_n > total_queries -- of which nothing but its job entries and mesh row is read; 1 if a query index lies outside
 * [0, n_vert): that query is skipped, the others count.  A mesh without vertices comes first: its job's query list is not looked at and
 * info stays 0.  Nothing out of bounds is ever read.
 *
 * KERNELS.  Three launches on `stream` (a hipStream_t passed as void*, NULL = default stream): the clear (outputs, info, workspace), the
 * walk -- a workgroup per (job, row, tile of LC_SYMFIND_QUERIES queries): each lane transforms its queries once and keeps them in
 * registers, the mesh's vertices go through LDS in tiles of LC_SYMFIND_TILE and are read as broadcasts, a query's min is complete inside
 * the workgroup, and the workgroup's largest (n_i bits << 32 | ~position) joins the row's 64-bit slot by one vector atomic max -- and the
 * finish, a workgroup per (job, row): the slot's query once more against every vertex under the key (d2 bits << 32 | j), which gives the
 * witness target.  workspace: lc_symfind_workspace_bytes(n_jobs, max_k) = 8 * n_jobs * max_k rounded up to 16 bytes, 16-byte aligned; it
 * is cleared on the stream and carries nothing from call to call.  Every argument rule is checked before anything is launched; no
 * allocation, no wait, no read-back, graph-capturable.  max_queries is not read when query_idx is NULL (max_verts takes its place).
 * Return value: 0 on success, non-zero on error (lc_amd_symfind_last_error() gives the text).
 */
#ifndef LC_AMD_SYMFIND_H
#define LC_AMD_SYMFIND_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LC_AMD_SYMFIND_VERSION 1
#define LC_SYMFIND_TILE 256
#define LC_SYMFIND_QUERIES 256

int lc_amd_symfind_version(void);
const char *lc_amd_symfind_last_error(void);
const char *lc_amd_symfind_source_hash(void);
size_t lc_symfind_workspace_bytes(int n_jobs, int max_k);
int lc_symfind_deviation_f32(const float *verts, int total_verts, const int *mesh_table, const int *mesh_table_host, int n_meshes, int max_verts,
                             const double *table, int total_rows, const int *mesh_index, const int *row_off, const int *row_k, int n_jobs,
                             int max_k, const int *query_idx, const int *query_off, const int *query_n, int total_queries, int max_queries,
                             float *dev2, int *arg_query, int *arg_target, int *info, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LC_AMD_SYMFIND_H */
