// Device helpers shared by more than one library (gfx950 / CDNA4, wave64): included by lc_common.h (liblc_amd.so) and by
// posecov/lc_pose_cov.hip (liblc_amd_posecov.so).  A library that includes a header of this directory declares it in its Target
// (lc_amd/build.py: `shared`), so that its source hash covers it.
//
// The fp64 cross-lane layer: the order-defining reductions that "the same bits for every slicing" rests on, in ONE copy.  None of
// them touches LDS: the 32- and 16-lane exchanges use gfx950's v_permlane32_swap / v_permlane16_swap (a swap of register halves IS
// the reduce-scatter exchange, so no select is needed), the 8-, 4-, 2- and 1-lane exchanges use DPP row_mirror / row_half_mirror /
// quad_perm moves.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>

namespace lc {

constexpr int kWave = 64;

// DPP controls (cdna4 ISA 'DPP_CTRL')
constexpr int kDppQuadXor1 = 0xB1;      // quad_perm:[1,0,3,2]
constexpr int kDppQuadXor2 = 0x4E;      // quad_perm:[2,3,0,1]
constexpr int kDppIdentity = 0xE4;      // quad_perm:[0,1,2,3]
constexpr int kDppRowMirror = 0x140;    // lane i <-> 15-i inside each row of 16
constexpr int kDppHalfMirror = 0x141;   // lane i <-> 7-i inside each half row of 8

template <int CTRL, int BANK_MASK = 0xF>
__device__ __forceinline__ double dpp_mov_f64(double old, double src) {
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(src), CTRL, 0xF, BANK_MASK, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(src), CTRL, 0xF, BANK_MASK, false);
    return __hiloint2double(hi, lo);
}

// value of `v` in lane `src` (ds_bpermute: LDS crossbar, no LDS memory)
__device__ __forceinline__ double shfl_f64(double v, int src) {
    const int lo = __shfl(__double2loint(v), src, kWave), hi = __shfl(__double2hiint(v), src, kWave);
    return __hiloint2double(hi, lo);
}

// a' (returned in a) and b' after swapping a's upper 32 lanes with b's lower 32 lanes; a'+b' then holds, in the lower
// half-wave, the two-half sum of a and, in the upper half-wave, the two-half sum of b.
__device__ __forceinline__ double swap32_add(double a, double b) {
    const auto lo = __builtin_amdgcn_permlane32_swap(__double2loint(a), __double2loint(b), false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap(__double2hiint(a), __double2hiint(b), false, false);
    return __hiloint2double(hi[0], lo[0]) + __hiloint2double(hi[1], lo[1]);
}
// same for rows of 16: even rows end with the (row, row+1) sum of a, odd rows with that of b
__device__ __forceinline__ double swap16_add(double a, double b) {
    const auto lo = __builtin_amdgcn_permlane16_swap(__double2loint(a), __double2loint(b), false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap(__double2hiint(a), __double2hiint(b), false, false);
    return __hiloint2double(hi[0], lo[0]) + __hiloint2double(hi[1], lo[1]);
}

// lanes with bit 3 set ("up", banks 2-3 of each row) keep hi, the others keep lo; the partner (row mirror) supplies
// the same quantity.  BANK_UP = bank mask of the up lanes: 0xC for the 8-exchange, 0xA for the 4-exchange.
template <int CTRL, int BANK_UP>
__device__ __forceinline__ double dpp_exchange_add(double lo, double hi) {
    constexpr int BANK_DOWN = 0xF & ~BANK_UP;
    const double keep = dpp_mov_f64<kDppIdentity, BANK_UP>(lo, hi);              // up lanes <- hi
    double recv = dpp_mov_f64<CTRL, BANK_UP>(lo, hi);                            // up lanes <- partner's hi
    recv = dpp_mov_f64<CTRL, BANK_DOWN>(recv, lo);                               // down lanes <- partner's lo
    return keep + recv;
}

// All-reduce of K doubles across the 64 lanes of a wave (every lane gets the sum), LDS-free.
template <int K>
__device__ __forceinline__ void wave_allreduce(double (&v)[K]) {
#pragma unroll
    for (int i = 0; i < K; ++i) {
        double x = v[i];
        x += dpp_mov_f64<kDppQuadXor1>(x, x);
        x += dpp_mov_f64<kDppQuadXor2>(x, x);
        x += dpp_mov_f64<kDppHalfMirror>(x, x);
        x += dpp_mov_f64<kDppRowMirror>(x, x);
        x = swap16_add(x, x);
        x = swap32_add(x, x);
        v[i] = x;
    }
}

// Reduce-scatter of K = 16*R doubles across a wave: after the call lane l holds, in v[0..R-1], the full
// wave sums of entries base..base+R-1 with base = R*(8*b5 + 4*b4 + 2*b3 + b2) (b_i = bit i of l).
// K/2 + K/4 + K/8 + K/16 + 2R exchanges instead of 6K for a butterfly all-reduce, none of them through LDS.
template <int K>
__device__ __forceinline__ void wave_reduce_scatter16(double (&v)[K], int /*lane*/) {
    static_assert(K % 16 == 0, "K must be a multiple of 16");
    constexpr int R = K / 16;
#pragma unroll
    for (int i = 0; i < K / 2; ++i) v[i] = swap32_add(v[i], v[i + K / 2]);
#pragma unroll
    for (int i = 0; i < K / 4; ++i) v[i] = swap16_add(v[i], v[i + K / 4]);
#pragma unroll
    for (int i = 0; i < K / 8; ++i) v[i] = dpp_exchange_add<kDppRowMirror, 0xC>(v[i], v[i + K / 8]);
#pragma unroll
    for (int i = 0; i < K / 16; ++i) v[i] = dpp_exchange_add<kDppHalfMirror, 0xA>(v[i], v[i + K / 16]);
#pragma unroll
    for (int i = 0; i < R; ++i) {
        v[i] += dpp_mov_f64<kDppQuadXor2>(v[i], v[i]);
        v[i] += dpp_mov_f64<kDppQuadXor1>(v[i], v[i]);
    }
}

__device__ __forceinline__ int scatter16_base(int lane, int R) {
    return R * (((lane >> 5) & 1) * 8 + ((lane >> 4) & 1) * 4 + ((lane >> 3) & 1) * 2 + ((lane >> 2) & 1));
}

// Reduce-scatter of K <= 16 doubles across a wave that pairs the lanes as the LDS block sum pairs its slots (lc_common.h:
// block_sum_segment over lane t's slot t, then segment 0 + segment 1): lane xor 16, 8, 4, 2, 1, 32, in that order.  Every add is
// own + partner of the two partial sums the LDS tree adds at that level, and fp64 addition is commutative: the totals have that tree's bits
// (wave_reduce_scatter16 pairs 32, 16, mirror-15, mirror-7, 2, 1: other partial sums, other roundings).
// The values halve at every stage: the 16-lane exchange is v_permlane16_swap, the 8- and 4-lane exchanges are DPP row moves under bank
// masks (the lanes that keep the upper half are whole banks of 4), the 2-lane exchange needs a per-lane select; the last two stages move
// one value.  With K = 14 entry e travels in slot e + e / 7 of the 16, so that the two slots nobody owns are
// 7 and 15: partners at the first stage (no exchange at all), and the upper half of one pair at the second (a plain own + partner).
// Returns, in lane l, the total of the entry in slot (l >> 1) & 15 (reduce_scatter_lds_order_entry; -1: nobody's slot, any finite or
// non-finite value); lanes l, l ^ 1 and l ^ 32 hold the same total.
template <int K>
__device__ __forceinline__ constexpr int reduce_scatter_lds_order_entry(int slot) {
    static_assert(K == 14 || K == 16, "16 slots, or 14 with slots 7 and 15 empty");
    if (K == 16) return slot;
    return (slot & 7) == 7 ? -1 : slot - (slot >> 3);
}
constexpr int kDppRowRor8 = 0x128;  // row_ror:8: lane i <- lane i ^ 8 of its row of 16
constexpr int kDppRowShl4 = 0x104;  // row_shl:4: lane i <- lane i + 4 of its row
constexpr int kDppRowShr4 = 0x114;  // row_shr:4: lane i <- lane i - 4 of its row
template <int K>
__device__ __forceinline__ double wave_reduce_scatter_lds_order(const double (&v)[K], int lane) {
    constexpr auto entry = reduce_scatter_lds_order_entry<K>;
    static_assert((entry(7) < 0) == (entry(15) < 0), "an empty slot's partner is empty");
    double w[8];
    // xor 16: lanes with bit 4 clear go on with slots 0-7, the others with slots 8-15
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (entry(i) >= 0) w[i] = swap16_add(v[entry(i)], v[entry(i + 8)]);
    }
    // xor 8: bit 3 clear (banks 0-1 of the row) keeps lo, set (banks 2-3) keeps hi.  The kept half by a select, the received one by two
    // moves onto the same register (7 instructions an exchange; the select as a third masked move costs two copies more).  Written out
    // with constant indices: in a loop the compiler turns the select of w[i] and w[i + 4] into a load at a selected index -- scratch
    const bool up8 = (lane & 8) != 0, up4 = (lane & 4) != 0;
    auto exchange8 = [up8](double lo, double hi) {
        const double keep = up8 ? hi : lo;
        double recv = dpp_mov_f64<kDppRowRor8>(lo, lo);       // every lane <- partner's lo ...
        recv = dpp_mov_f64<kDppRowRor8, 0xC>(recv, hi);       // ... the upper lanes <- partner's hi instead
        return keep + recv;
    };
    w[0] = exchange8(w[0], w[4]);
    w[1] = exchange8(w[1], w[5]);
    w[2] = exchange8(w[2], w[6]);
    if constexpr (entry(7) >= 0) w[3] = exchange8(w[3], w[7]);
    else w[3] += dpp_mov_f64<kDppRowRor8>(w[3], w[3]);        // nobody's slot above: the lanes with bit 3 set end with a copy
    // xor 4: bit 2 clear (banks 0 and 2) keeps lo, set (banks 1 and 3) keeps hi; the partner is 4 lanes up / down
    auto exchange4 = [up4](double lo, double hi) {
        const double keep = up4 ? hi : lo;
        double recv = dpp_mov_f64<kDppRowShl4, 0x5>(lo, lo);  // the lower lanes <- lo of the lane 4 up ...
        recv = dpp_mov_f64<kDppRowShr4, 0xA>(recv, hi);       // ... the upper lanes <- hi of the lane 4 down
        return keep + recv;
    };
    w[0] = exchange4(w[0], w[2]);
    w[1] = exchange4(w[1], w[3]);
    // xor 2: bit 1 clear keeps w[0], set keeps w[1] (half a bank: a select per lane)
    const bool up = (lane & 2) != 0;
    const double keep = up ? w[1] : w[0], send = up ? w[0] : w[1];
    double s = keep + dpp_mov_f64<kDppQuadXor2>(send, send);
    s += dpp_mov_f64<kDppQuadXor1>(s, s);  // xor 1
    return swap32_add(s, s);               // xor 32
}

// index of (i,j), i<=j, in a packed upper-triangular 6x6 (21 entries, row-major)
__host__ __device__ constexpr int tri6(int i, int j) { return i * 6 - (i * (i - 1)) / 2 + (j - i); }

// torch.nan_to_num with its defaults: NaN -> 0, +-inf -> +-FLT_MAX (cer_solver.py:29-31 applies it to every input when asked to)
__device__ __forceinline__ float nan_to_num(float f) { return f != f ? 0.f : fminf(fmaxf(f, -FLT_MAX), FLT_MAX); }

// rotation matrix of the quaternion q = (r, i, j, k) scaled by two_s (2/|q|^2: the proper rotation; the reference uses 2/|q|, rotation_conversions.py:52)
__device__ __forceinline__ void quat_matrix(const double q[4], double two_s, double R[9]) {
    const double r = q[0], i = q[1], j = q[2], k = q[3];
    R[0] = 1 - two_s * (j * j + k * k); R[1] = two_s * (i * j - k * r); R[2] = two_s * (i * k + j * r);
    R[3] = two_s * (i * j + k * r); R[4] = 1 - two_s * (i * i + k * k); R[5] = two_s * (j * k - i * r);
    R[6] = two_s * (i * k - j * r); R[7] = two_s * (j * k + i * r); R[8] = 1 - two_s * (i * i + j * j);
}

}  // namespace lc
