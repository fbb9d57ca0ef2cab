// The finished output value of an image byte (the definition: include/lc_amd_crop.h) and the types it is stored as, in ONE copy for the
// zoom-in crops (crop/lc_crop.hip) and the colour augmentation (augment/lc_augment.hip).  The dtype codes are this header's own; each
// library asserts that its public LC_*_U8 .. LC_*_BF16 are the same numbers.
#pragma once
#include <hip/hip_runtime.h>

namespace lc {

constexpr int kByteU8 = 0, kByteF32 = 1, kByteF16 = 2, kByteBF16 = 3;

template <int DT> struct Store { using type = unsigned short; };
template <> struct Store<kByteU8> { using type = unsigned char; };
template <> struct Store<kByteF32> { using type = float; };

template <typename T> struct alignas(4 * sizeof(T)) Vec4 { T v[4]; };

// The finished output value of byte v in channel c under the launch's parameters p (normalize, mean[3], std[3]): v / 255, then
// (. - mean) / std, each an IEEE fp32 operation; a 16-bit type is rounded once (nearest even) from that fp32.
template <int DT, typename P>
__device__ inline typename Store<DT>::type finish(int v, int c, const P& p) {
    if constexpr (DT == kByteU8) {
        return (unsigned char)v;
    } else {
        float q = __fdiv_rn((float)v, 255.0f);
        if (p.normalize) {
            q = __fsub_rn(q, p.mean[c]);
            q = __fdiv_rn(q, p.std[c]);
        }
        if constexpr (DT == kByteF32) {
            return q;
        } else if constexpr (DT == kByteF16) {
            return __builtin_bit_cast(unsigned short, (_Float16)q);
        } else {
            const unsigned u = __float_as_uint(q);
            if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)0x7fc0;
            return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
        }
    }
}

}  // namespace lc
