// The keyed integer hash behind the device's random numbers (the definition: include/lc_amd_maskcrop.h), in ONE copy for the mask
// crops' check points (maskcrop/lc_maskcrop.hip), the colour augmentation (augment/lc_augment.hip) and the drawn crop geometry
// (geometry/lc_geometry.hip): key(seed, sample, op, i) = fmix32(fmix32(sample_state(seed_state(seed), sample) ^ op) ^ i).  Pieces, not
// a kernel: each library mixes its own op codes or round numbers into the state.  (lc_select_rows.h hashes with other constants: another
// hash.)
#pragma once
#include <hip/hip_runtime.h>

namespace lc {

// MurmurHash3's 32-bit finaliser
__device__ __forceinline__ unsigned fmix32(unsigned v) {
    v ^= v >> 16;
    v *= 0x85ebca6bu;
    v ^= v >> 13;
    v *= 0xc2b2ae35u;
    v ^= v >> 16;
    return v;
}

// The key state behind a seed, and behind (seed, sample id): every op code or round number is mixed into the latter.  Two functions, so
// that a caller's sample id (a load behind a NULL test) is formed after the seed's two steps: as one function of three arguments the
// mask crops' check-point kernel compiles to other code.
__device__ __forceinline__ unsigned seed_state(unsigned seed_lo, unsigned seed_hi) { return fmix32(fmix32(seed_lo) ^ seed_hi); }
__device__ __forceinline__ unsigned sample_state(unsigned seed_state, unsigned sample_id) { return fmix32(seed_state ^ sample_id); }

// A key's upper 24 bits as a number in [0, 1): exact
__device__ __forceinline__ double key_uniform(unsigned key) { return __dmul_rn((double)(key >> 8), 0x1p-24); }

}  // namespace lc
