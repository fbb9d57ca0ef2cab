// The fused Ranger step (include/lc_amd_optim.h): every parameter tensor of an optimizer in one launch.
//
// Per element, in the order of the reference's torch ops (lib/optim/ranger.py:145-196), one fp32 rounding per op; a multiply is fused
// into an add only where the reference writes `a + s*b` as ONE op (add_ with alpha, addcmul_, addcdiv_):
//   g  = g + (-mean(row))                      (written back to p.grad: the reference centres p.grad in place)
//   v  = v * b2;  v = v + ((1-b2) * g) * g     (mul_, addcmul_)
//   m  = m * b1;  m = m + (1-b1) * g           (mul_, add_)
//   p  = p + (-wd*lr) * p                      (only when weight_decay != 0)
//   p  = p + (-step_size*lr) * (m / (sqrt(v) + eps))    or    p = p + (-step_size*lr) * m
//   on the tensor's Lookahead step: s = s + alpha * (p - s);  p = s
// The row mean is a float64 sum in a fixed order (one wave per row, lane-strided, then a fixed butterfly): no atomics, the same bits on
// every run.  A workgroup owns whole rows of up to LC_RANGER_ONE_PASS_ROW elements and keeps their gradients in LDS between the mean and
// the update; longer rows get their means from a row-mean launch first.
#include <hip/hip_runtime.h>

#include <string>

#include "../../../include/lc_amd_optim.h"

#ifndef LC_AMD_OPTIM_SRC_HASH
#define LC_AMD_OPTIM_SRC_HASH "unrecorded"
#endif

namespace {

const char kSrcHash[] = "LC_AMD_OPTIM_SRC_HASH:" LC_AMD_OPTIM_SRC_HASH;
thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxElems = LC_RANGER_BLOCK_ELEMS;
constexpr int kMaxRows = LC_RANGER_BLOCK_ROWS;
static_assert(LC_RANGER_ONE_PASS_ROW <= kMaxElems, "a one-pass row must fit one workgroup");
static_assert(sizeof(lc_ranger_scalars) == 48 && sizeof(lc_ranger_tensor) == 56 && sizeof(lc_ranger_block) == 16, "table layout");

struct Table {
    const lc_ranger_scalars* sc;
    const lc_ranger_tensor* td;
    const lc_ranger_block* blocks;
};

__device__ inline Table table_of(const void* table, int ntensors) {
    const char* b = static_cast<const char*>(table);
    Table t;
    t.sc = reinterpret_cast<const lc_ranger_scalars*>(b);
    t.td = reinterpret_cast<const lc_ranger_tensor*>(b + sizeof(lc_ranger_scalars) * (size_t)ntensors);
    t.blocks = reinterpret_cast<const lc_ranger_block*>(b + (sizeof(lc_ranger_scalars) + sizeof(lc_ranger_tensor)) * (size_t)ntensors);
    return t;
}

__device__ inline void update(float& p, float& g, float& m, float& v, float& s, float neg_mean, bool centre, const lc_ranger_scalars& c) {
    if (centre) g = g + neg_mean;
    v = v * c.beta2;
    v = fmaf(c.one_minus_beta2 * g, g, v);
    m = m * c.beta1;
    m = fmaf(c.one_minus_beta1, g, m);
    if (c.flags & LC_RANGER_WEIGHT_DECAY) p = fmaf(c.neg_wd_lr, p, p);
    if (c.flags & LC_RANGER_ADAPTIVE) {
        const float denom = sqrtf(v) + c.eps;
        p = fmaf(c.neg_step_lr, m / denom, p);
    } else {
        p = fmaf(c.neg_step_lr, m, p);
    }
    if (c.flags & LC_RANGER_LOOKAHEAD) {
        s = fmaf(c.alpha, p - s, s);
        p = s;
    }
}

// Four consecutive floats: one 16-byte access for an array in phase with p (the address is then 16-byte aligned), else four 4-byte ones.
__device__ inline float4 load4(const float* x, bool in_phase) {
    if (in_phase) return *reinterpret_cast<const float4*>(x);
    return make_float4(x[0], x[1], x[2], x[3]);
}

__device__ inline void store4(float* x, float4 v, bool in_phase) {
    if (in_phase) {
        *reinterpret_cast<float4*>(x) = v;
    } else {
        x[0] = v.x;
        x[1] = v.y;
        x[2] = v.z;
        x[3] = v.w;
    }
}

// One float64 row sum: lane-strided over the row, then a fixed butterfly; every lane ends with the same value.
__device__ inline double wave_sum(double x) {
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

// The row-mean launch: one workgroup per row longer than LC_RANGER_ONE_PASS_ROW (thread-strided float64 sum, fixed tree over LDS).
__global__ __launch_bounds__(kThreads) void lc_ranger_row_mean_kernel(const void* table, int ntensors, float* __restrict__ row_means) {
    const Table t = table_of(table, ntensors);
    const lc_ranger_block b = t.blocks[blockIdx.x];
    const lc_ranger_tensor d = t.td[b.tensor];
    const long long L = d.row;
    const float* g = t.sc[b.tensor].grad + b.e0 * L;
    double acc = 0.0;
    for (long long i = threadIdx.x; i < L; i += kThreads) acc += (double)g[i];
    __shared__ double part[kThreads];
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int w = kThreads / 2; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) row_means[d.mean_off + b.e0] = (float)(part[0] / (double)L);
}

// The update launch.  Chunk j of a block covers the elements [4j - h, 4j - h + 4) of its range [e0, e0 + n), h chosen so that p's chunks
// start on 16-byte boundaries: a full chunk is one float4 per array in phase with p (load4 / store4), and the first and last chunks are
// read element by element.
// ALL: every array in phase with p (the common case: separate allocations), compiled without the 4-byte access paths.
template <bool ALL>
__device__ inline void update_block(const Table& t, const lc_ranger_block& b, const float* __restrict__ row_means, float4* sg4, float* smean) {
    const lc_ranger_tensor d = t.td[b.tensor];
    const lc_ranger_scalars c = t.sc[b.tensor];
    float* const grad = c.grad;
    const int n = b.n;
    const long long e0 = b.e0;
    const int h = (int)(((reinterpret_cast<unsigned long long>(d.p) >> 2) + (unsigned long long)e0) & 3);
    const int nchunks = (n + h + 3) >> 2;
    const long long base = e0 - h;  // element index of chunk 0's first element: d.p + base is 16-byte aligned
    const int L = d.row;
    const bool centre = L > 0;
    const bool local = centre && L <= LC_RANGER_ONE_PASS_ROW;  // whole rows in this workgroup: mean on chip
    const bool lookahead = (c.flags & LC_RANGER_LOOKAHEAD) != 0;
    const bool g4 = ALL || (c.flags & LC_RANGER_GRAD_IN_PHASE) != 0;
    const bool m4 = ALL || (d.phase & LC_RANGER_EXP_AVG_IN_PHASE) != 0;
    const bool v4 = ALL || (d.phase & LC_RANGER_EXP_AVG_SQ_IN_PHASE) != 0;
    const bool s4 = ALL || (d.phase & LC_RANGER_SLOW_IN_PHASE) != 0;
    float* sg = reinterpret_cast<float*>(sg4);

    if (local) {
        for (int j = threadIdx.x; j < nchunks; j += kThreads) {
            const int i0 = 4 * j - h;
            if (i0 >= 0 && i0 + 4 <= n) {
                sg4[j] = load4(grad + base + 4 * j, g4);
            } else {
                for (int q = 0; q < 4; ++q) {
                    const int i = i0 + q;
                    if (i >= 0 && i < n) sg[i + h] = grad[e0 + i];
                }
            }
        }
        __syncthreads();
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        const int nrows = n / L;
        for (int r = wave; r < nrows; r += kWaves) {
            double acc = 0.0;
            const float* row = sg + h + r * L;
            for (int i = lane; i < L; i += 64) acc += (double)row[i];
            acc = wave_sum(acc);
            if (lane == 0) smean[r] = -(float)(acc / (double)L);
        }
        __syncthreads();
    }

    for (int j = threadIdx.x; j < nchunks; j += kThreads) {
        const int i0 = 4 * j - h;
        float neg_mean[4] = {0.f, 0.f, 0.f, 0.f};
        if (local) {
            for (int q = 0; q < 4; ++q) {
                const int i = i0 + q;
                if (i >= 0 && i < n) neg_mean[q] = smean[i / L];
            }
        } else if (centre) {
            for (int q = 0; q < 4; ++q) {
                const int i = i0 + q;
                if (i >= 0 && i < n) neg_mean[q] = -row_means[d.mean_off + (e0 + i) / L];
            }
        }
        if (i0 >= 0 && i0 + 4 <= n) {
            const long long e = base + 4 * j;
            float4 g = local ? sg4[j] : load4(grad + e, g4);
            float4 p = *reinterpret_cast<const float4*>(d.p + e);
            float4 m = load4(d.exp_avg + e, m4);
            float4 v = load4(d.exp_avg_sq + e, v4);
            float4 s = lookahead ? load4(d.slow + e, s4) : make_float4(0.f, 0.f, 0.f, 0.f);
            update(p.x, g.x, m.x, v.x, s.x, neg_mean[0], centre, c);
            update(p.y, g.y, m.y, v.y, s.y, neg_mean[1], centre, c);
            update(p.z, g.z, m.z, v.z, s.z, neg_mean[2], centre, c);
            update(p.w, g.w, m.w, v.w, s.w, neg_mean[3], centre, c);
            if (centre) store4(grad + e, g, g4);
            *reinterpret_cast<float4*>(d.p + e) = p;
            store4(d.exp_avg + e, m, m4);
            store4(d.exp_avg_sq + e, v, v4);
            if (lookahead) store4(d.slow + e, s, s4);
        } else {
            for (int q = 0; q < 4; ++q) {
                const int i = i0 + q;
                if (i < 0 || i >= n) continue;
                const long long e = e0 + i;
                float g = local ? sg[i + h] : grad[e];
                float p = d.p[e], m = d.exp_avg[e], v = d.exp_avg_sq[e];
                float s = lookahead ? d.slow[e] : 0.f;
                update(p, g, m, v, s, neg_mean[q], centre, c);
                if (centre) grad[e] = g;
                d.p[e] = p;
                d.exp_avg[e] = m;
                d.exp_avg_sq[e] = v;
                if (lookahead) d.slow[e] = s;
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void lc_ranger_update_kernel(const void* table, int ntensors, int nrowsum, const float* __restrict__ row_means) {
    const Table t = table_of(table, ntensors);
    const lc_ranger_block b = t.blocks[nrowsum + blockIdx.x];
    __shared__ float4 sg4[kMaxElems / 4 + 1];  // this block's gradients, element i at float index i + h
    __shared__ float smean[kMaxRows];          // -mean of each local row
    const int all = LC_RANGER_EXP_AVG_IN_PHASE | LC_RANGER_EXP_AVG_SQ_IN_PHASE | LC_RANGER_SLOW_IN_PHASE;
    if ((t.td[b.tensor].phase & all) == all && (t.sc[b.tensor].flags & LC_RANGER_GRAD_IN_PHASE))
        update_block<true>(t, b, row_means, sg4, smean);
    else
        update_block<false>(t, b, row_means, sg4, smean);
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int lc_amd_optim_version(void) { return LC_AMD_OPTIM_VERSION; }
const char* lc_amd_optim_source_hash(void) { return kSrcHash + sizeof("LC_AMD_OPTIM_SRC_HASH:") - 1; }
const char* lc_amd_optim_last_error(void) { return g_err.c_str(); }

int lc_ranger_step_f32(const void* table, int ntensors, int nrowsum, int nupdate, float* row_means, void* stream) {
    if (ntensors < 0 || nrowsum < 0 || nupdate < 0) return fail(1, "lc_ranger_step_f32: negative count");
    if (nupdate == 0) return nrowsum == 0 ? 0 : fail(1, "lc_ranger_step_f32: row means without an update launch");
    if (!table || ntensors == 0) return fail(1, "lc_ranger_step_f32: null or empty tensor table");
    if (nrowsum > 0 && !row_means) return fail(1, "lc_ranger_step_f32: rows longer than LC_RANGER_ONE_PASS_ROW need the row_means workspace");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (nrowsum > 0) hipLaunchKernelGGL(lc_ranger_row_mean_kernel, dim3(nrowsum), dim3(kThreads), 0, s, table, ntensors, row_means);
    hipLaunchKernelGGL(lc_ranger_update_kernel, dim3(nupdate), dim3(kThreads), 0, s, table, ntensors, nrowsum, row_means);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(10, std::string("lc_ranger_step_f32: launch: ") + hipGetErrorString(e));
    return 0;
}

}  // extern "C"
#pragma GCC visibility pop
