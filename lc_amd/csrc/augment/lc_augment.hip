// Training-time background switch and colour augmentation of the network's crops, one launch (liblc_amd_augment.so; C ABI and the exact
// definition of every output in include/lc_amd_augment.h; tests/augment_oracle.py is its numpy restatement).  What the reference's
// loader does per instance on a host core (dataset.py:137-148,413-419, imgaug).
//
// One workgroup of four waves per (row, 32 x 32 tile).  The row's 64 parameter words go to LDS, thread 0 judges them (a refused row has
// every stage off and is written as its crop), and all threads fill a 768-entry table of the FINISHED output values of the row: the
// LUT of the point operations (or the identity) followed by v / 255 and the normalisation, so that the last stage is one look-up.
//
// lc_augment_drawn_u8 launches the same kernels with the row DRAWN instead of loaded: the first wavefront forms the 64 words and the
// three tables from (configuration, seed word on the device, sample id) -- `draw` of lc_amd/augment.py restated, below -- and leaves them
// in LDS where a loaded row would lie; judging, the finished table and the pixel work do not know the difference.
//
// A thread works on a quad: four consecutive x of one image row, the three channels as the bytes of three words.
//   head (point-wise): the blend with the background, salt and pepper, and for rows without filter A the dropout
//   filtered form: the head of the tile plus a 4-pixel halo (40 x 40 x 3 bytes) is staged in LDS; filter A is evaluated on the
//     36 x 36 region at in-image positions, the dropout applied, the result staged in a second buffer; filter B is evaluated on the
//     tile.  Both filters read LDS through indices reflected at the IMAGE border; a reflected position of an in-image pixel always
//     lies inside the staged region (h, w >= 8: one reflection), and every LDS index is clamped to the region besides.
//   point-wise form (the caller states that no row uses a filter): the head of the tile's quads goes straight to the output.
// Global loads and stores move four pixels (4 bytes of uint8, 16 of the mask and of an fp32 output) where w is a multiple of four and
// the pointers are aligned to it; element by element otherwise.
//
// The hash is maskcrop's (include/lc_amd_maskcrop.h): shared/lc_keyed_hash.h.
//
// Bounds: every quad is judged against the image before it is loaded or stored, the background index and the NULL inputs are judged
// before they are used, and a refused row reads its crop only.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../../include/lc_amd_augment.h"
#include "../shared/lc_byte_finish.h"
#include "../shared/lc_keyed_hash.h"

#ifndef LC_AMD_AUGMENT_SRC_HASH
#define LC_AMD_AUGMENT_SRC_HASH "unrecorded"
#endif

namespace lc {
namespace {

const char kSrcHash[] = "LC_AMD_AUGMENT_SRC_HASH:" LC_AMD_AUGMENT_SRC_HASH;
thread_local std::string g_err;

int fail(int code, std::string msg) {
    g_err = std::move(msg);
    return code;
}

constexpr int kThreads = 256;
constexpr int kTile = 32;
constexpr int kHalo = 4;
constexpr int kFrame = kTile + 2 * kHalo;     // 40: the staged region's side
constexpr int kFrameQuads = kFrame / 4;       // 10 quads per staged row
constexpr int kPlaneWords = kFrame * kFrameQuads;  // 400 words = 1600 bytes per channel
constexpr int kWords = LC_AUGMENT_WORDS;

constexpr int kBlend = 1, kSnp = 2, kFilterA = 4, kDrop = 8, kFilterB = 16, kLut = 32;

struct Params {
    const unsigned char* crops;  // (B,3,h,w)
    const unsigned char* bg;     // (G,3,h,w) or null
    const float* msk;            // (B,h,w) or null
    const int* params;           // (B,64)
    const unsigned char* lut;    // (B,3,256)
    const int* sample_id;        // (B) or null
    void* out;                   // (B,3,h,w)
    int* info;                   // (B) or null
    int B, G, h, w, tiles_x, tiles_y;
    int vec;                     // four-pixel loads and stores are possible
    int normalize;
    unsigned seed_lo, seed_hi;
    float mean[3], std[3];
    // lc_augment_drawn_u8: the rows are drawn by the kernel
    int drawn;
    lc_augment_draw_config cfg;
    const unsigned long long* seed;  // one word on the device, in the place of seed_lo / seed_hi
    int* params_out;                 // (B,64) or null
    unsigned char* lut_out;          // (B,3,256) or null
};

// the finished output value of a byte (lc_amd_crop.h): shared/lc_byte_finish.h, with the zoom-in crops
static_assert(LC_AUGMENT_U8 == kByteU8 && LC_AUGMENT_F32 == kByteF32 && LC_AUGMENT_F16 == kByteF16 && LC_AUGMENT_BF16 == kByteBF16, "the dtype codes of lc_byte_finish.h");

// What a workgroup knows of its row once it is judged
struct Row {
    int flags;                 // P[0], or 0 for a refused row
    int g, gh, gw;
    unsigned snp_th, drop_th;
    unsigned k_snp, k_snpv, k_drop;  // the key states behind the three op codes
};

__device__ inline bool weights_ok(const int* wq) {
    long long sum = 0;
    bool ok = true;
    for (int i = 0; i < 25; ++i) {
        ok = ok && wq[i] >= 0;
        sum += wq[i];
    }
    return ok && sum == 65536;
}

// four bytes at q as one word; pixels at x >= w read 0
__device__ __forceinline__ unsigned load4(const unsigned char* q, int x0, int w, int vec) {
    if (vec) return *reinterpret_cast<const unsigned*>(q);
    unsigned r = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (x0 + j < w) r |= (unsigned)q[j] << (8 * j);
    return r;
}

// coarse dropout of the quad (x0.., y)
__device__ __forceinline__ void drop_quad(const Params& p, const Row& r, int x0, int y, unsigned (&v)[3]) {
    const int cy = (int)((unsigned)(y * r.gh) / (unsigned)p.h) * r.gw;
    unsigned keep = 0xffffffffu;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int cell = cy + (int)((unsigned)((x0 + j) * r.gw) / (unsigned)p.w);
        if (fmix32(r.k_drop ^ (unsigned)cell) < r.drop_th) keep &= ~(0xffu << (8 * j));
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] &= keep;
}

// The point-wise head of the in-image quad (x0.., y) of row b, 0 <= y < h, 0 <= x0 < w: blend, salt and pepper, and with `drop` the dropout
__device__ __forceinline__ void head_quad(const Params& p, const Row& r, int b, int x0, int y, bool drop, unsigned (&v)[3]) {
    const size_t plane = (size_t)p.h * p.w;
    const size_t o = (size_t)y * p.w + x0;
    const unsigned char* src = p.crops + (size_t)b * 3 * plane + o;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = load4(src + c * plane, x0, p.w, p.vec);
    if (r.flags & kBlend) {
        float m[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        const float* mp = p.msk + (size_t)b * plane + o;
        if (p.vec) {
            const float4 t = *reinterpret_cast<const float4*>(mp);
            m[0] = t.x, m[1] = t.y, m[2] = t.z, m[3] = t.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + j < p.w) m[j] = mp[j];
        }
        unsigned k[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float t = __fmul_rn(m[j], 1024.0f);
            k[j] = t >= 1024.0f ? 1024u : t > 0.0f ? (unsigned)rintf(t) : 0u;  // NaN: 0
        }
        const unsigned char* bgp = p.bg + (size_t)r.g * 3 * plane + o;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned back = load4(bgp + c * plane, x0, p.w, p.vec);
            unsigned res = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned S = k[j] * ((v[c] >> (8 * j)) & 0xffu) + (1024u - k[j]) * ((back >> (8 * j)) & 0xffu);
                const unsigned q = S >> 10, rem = S & 1023u;
                res |= (q + ((rem > 512u || (rem == 512u && (q & 1u))) ? 1u : 0u)) << (8 * j);  // <= 255: S <= 1024 * 255
            }
            v[c] = res;
        }
    }
    if (r.flags & kSnp) {
        unsigned keep = 0xffffffffu, salt = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned q = (unsigned)(y * p.w + x0 + j);
            if (fmix32(r.k_snp ^ q) < r.snp_th) {
                keep &= ~(0xffu << (8 * j));
                if (fmix32(r.k_snpv ^ q) >> 31) salt |= 0xffu << (8 * j);
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (v[c] & keep) | salt;
    }
    if (drop) drop_quad(p, r, x0, y, v);
}

__device__ __forceinline__ int reflect101(int i, int n) { return i < 0 ? -i : i >= n ? 2 * n - 2 - i : i; }
__device__ __forceinline__ int in_frame(int i) { return min(max(i, 0), kFrame - 1); }

// The 5x5 filter of the quad (x0.., y) with the Q16 weights wq (LDS), read from the staged planes `src` whose corner is image pixel (fx0, fy0)
__device__ __forceinline__ void filter_quad(const unsigned char* src, const int* wq, int fx0, int fy0, int x0, int y, int h, int w, unsigned (&v)[3]) {
    int rr[5], cc[8];
#pragma unroll
    for (int d = 0; d < 5; ++d) rr[d] = in_frame(reflect101(y + d - 2, h) - fy0) * kFrame;
#pragma unroll
    for (int i = 0; i < 8; ++i) cc[i] = in_frame(reflect101(x0 + i - 2, w) - fx0);
    int wv[25];
#pragma unroll
    for (int i = 0; i < 25; ++i) wv[i] = wq[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        unsigned acc[4] = {32768u, 32768u, 32768u, 32768u};
#pragma unroll
        for (int d = 0; d < 5; ++d)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const unsigned t = src[c * (kPlaneWords * 4) + rr[d] + cc[i]];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (i - j >= 0 && i - j <= 4) acc[j] += (unsigned)wv[d * 5 + i - j] * t;
            }
        // non-negative weights that sum to 65536: at most 255 after the shift
        v[c] = (acc[0] >> 16) | ((acc[1] >> 16) << 8) | ((acc[2] >> 16) << 16) | ((acc[3] >> 16) << 24);
    }
}

// ---- the row drawn by the kernel (lc_augment_drawn_u8): `draw` of lc_amd/augment.py restated for one wavefront.  The gates and every
// number behind them are the same in all 64 lanes (they depend on the seed word and the row's sample id alone); the lanes share out the
// 64 parameter words, one each, and the 768 table entries, four per lane and channel.  Every fp64 product and sum that `draw` rounds on
// its own is written as __dmul_rn / __dadd_rn / __dsub_rn / __ddiv_rn here, so that nothing is fused under -ffp-contract=on.

// the key state behind (seed, sample id), which every op code is mixed into
__device__ __forceinline__ unsigned row_key(const Params& p, int b) {
    unsigned lo = p.seed_lo, hi = p.seed_hi;
    if (p.drawn) {
        const unsigned long long s = *p.seed;
        lo = (unsigned)s, hi = (unsigned)(s >> 32);
    }
    return sample_state(seed_state(lo, hi), (unsigned)(p.sample_id ? p.sample_id[b] : b));
}

// exp(x) for x <= 0: x = k ln 2 + r with |r| <= ln 2 / 2 and the rational form of fdlibm's e_exp.c on r (below one unit in the last
// place).  Below -700 the result is 0: a term under 1e-300 changes neither the sum of the five taps (which holds a 1) nor a Q16 weight.
__device__ inline double exp_neg(double x) {
    if (x < -700.0) return 0.0;
    const double k = rint(x * 1.44269504088896338700e+00);
    const double hi = fma(-k, 6.93147180369123816490e-01, x);  // exact: the high part of ln 2 ends in 32 zero bits, |k| < 2^11
    const double lo = k * 1.90821492927058770002e-10;
    const double r = hi - lo;
    const double z = r * r;
    const double c = r - z * fma(z, fma(z, fma(z, fma(z, 4.13813679705723846039e-08, -1.65339022054652515390e-06), 6.61375632143793436117e-05),
                                        -2.77777777770155933842e-03), 1.66666666666666019037e-01);
    const double y = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi);
    return ldexp(y, (int)k);
}

// sin and cos on |x| <= pi / 4 (and a few units in the last place beyond): the polynomials of fdlibm's k_sin.c and k_cos.c
__device__ inline double sin_reduced(double x) {
    const double z = x * x;
    const double r = fma(z, fma(z, fma(z, fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08), 2.75573137070700676789e-06),
                                -1.98412698298579493134e-04), 8.33333333332248946124e-03);
    return x + (z * x) * fma(z, r, -1.66666666666666324348e-01);
}

__device__ inline double cos_reduced(double x) {
    const double z = x * x;
    const double r = z * fma(z, fma(z, fma(z, fma(z, fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09), -2.75573143513906633035e-07),
                                           2.48015872894767294178e-05), -1.38888888888741095749e-03), 4.16666666666666019037e-02);
    const double ax = fabs(x);
    if (ax < 0.3) return 1.0 - (0.5 * z - z * r);
    // 1 - qx and z / 2 - qx are exact for a qx near x / 4 with a short mantissa: the leading 1 - z / 2 loses nothing
    const double qx = ax > 0.78125 ? 0.28125 : __longlong_as_double(__double_as_longlong(ax * 0.25) & (long long)0xffffffff00000000ull);
    return (1.0 - qx) - ((0.5 * z - qx) - z * r);
}

// The sum of the 25 values held by lanes base .. base + 24, in every lane, in the order numpy's pairwise sum takes for 25 elements:
// eight running sums over i mod 8, combined as a tree, then the last element.
__device__ __forceinline__ double sum25(double a, int base) {
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = __dadd_rn(__dadd_rn(__shfl(a, base + j), __shfl(a, base + 8 + j)), __shfl(a, base + 16 + j));
    const double res = __dadd_rn(__dadd_rn(__dadd_rn(r[0], r[1]), __dadd_rn(r[2], r[3])), __dadd_rn(__dadd_rn(r[4], r[5]), __dadd_rn(r[6], r[7])));
    return __dadd_rn(res, __shfl(a, base + 24));
}

// `_quantise`: floor(x 65536 + 1/2) in lanes base .. base + 24 (0 in every other lane), the remainder to 65536 added to the centre
__device__ __forceinline__ int quantise25(double x, int lane, int base) {
    int q = (lane >= base && lane < base + 25) ? (int)floor(__dadd_rn(__dmul_rn(x, 65536.0), 0.5)) : 0;
    int sum = q;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
    if (lane == base + 12) q += 65536 - sum;
    return q;
}

__device__ __forceinline__ double table_step(double x) { return fmin(fmax(rint(x), 0.0), 255.0); }

// Called by the first wavefront, all 64 lanes: lane l leaves word l of the row in s_P and its twelve table entries in s_lut, and with
// `store` (the row's first tile) writes them to params_out / lut_out as well.
template <bool FILTERED>
__device__ __forceinline__ void draw_row(const Params& p, int b, bool store, int lane, int* s_P, unsigned* s_lut) {
    const lc_augment_draw_config& cfg = p.cfg;
    const unsigned k = row_key(p, b);
    const auto key = [k](unsigned op, unsigned i) { return fmix32(fmix32(k ^ op) ^ i); };
    const auto u = [&key](unsigned op, unsigned i) { return key_uniform(key(op, i)); };
    // one value per channel where the op's own draw says so, else the first for all three
    const auto per_channel = [&u](unsigned op, double prob, int c) { return u(op, 1) < prob ? u(op, 2 + c) : u(op, 2); };

    const int nb = cfg.n_backgrounds;
    const bool sw = u(LC_AUGMENT_OP_SWITCH, 0) < cfg.switch_bg_prob && nb > 0;
    const int which = min((int)__dmul_rn(u(LC_AUGMENT_OP_SWITCH, 1), (double)nb), max(nb - 1, 0));
    const bool chain = u(LC_AUGMENT_OP_CHAIN, 0) < cfg.pixel_aug_prob;
    const bool salt = chain && cfg.use_peper_salt && u(LC_AUGMENT_OP_SALT, 0) < 0.3;
    const bool motion = chain && cfg.use_motion_blur && u(LC_AUGMENT_OP_MOTION, 0) < 0.2;
    const bool dropout = chain && u(LC_AUGMENT_OP_DROPOUT, 0) < 0.5;
    const double sigma = __dmul_rn(1.2, u(LC_AUGMENT_OP_GAUSS, 1));
    const bool gauss = chain && u(LC_AUGMENT_OP_GAUSS, 0) < 0.5 && sigma >= 1e-3;
    const bool add = chain && u(LC_AUGMENT_OP_ADD, 0) < 0.5;
    const bool invert = chain && cfg.use_invert && u(LC_AUGMENT_OP_INVERT, 0) < 0.4;
    const bool mul_pc = chain && u(LC_AUGMENT_OP_MUL_PC, 0) < 0.5;
    const bool mul = chain && u(LC_AUGMENT_OP_MUL, 0) < 0.5;
    const bool contrast = chain && u(LC_AUGMENT_OP_CONTRAST, 0) < 0.5;
    const bool table = add || invert || mul_pc || mul || contrast;

    int word = 0;
    if (lane == 0) word = (sw ? kBlend : 0) | (salt ? kSnp : 0) | (motion ? kFilterA : 0) | (dropout ? kDrop : 0) | (gauss ? kFilterB : 0) | (table ? kLut : 0);
    if (lane == 1 && sw) word = which;
    if (lane == 2 && salt) word = 214748364;    // floor(0.05 2^32)
    if (lane == 3 && dropout) word = 429496729;  // floor(0.1 2^32)
    if (lane == 4 && dropout) word = max(1, p.h * 5 / 100);
    if (lane == 5 && dropout) word = max(1, p.w * 5 / 100);

    if constexpr (FILTERED) {  // (the point-wise form refuses a row with a filter bit: its weights are never read)
        if (motion) {  // lanes 6 .. 30 hold the cell (yy, xx) of the 5x5 grid
            const unsigned m = key(LC_AUGMENT_OP_MOTION, 1) >> 8;  // the angle is 360 m / 2^24 degrees
            const double t = __dmul_rn(__dmul_rn(360.0, (double)m * 0x1p-24), 3.141592653589793 / 180.0);  // math.radians
            // t = q pi / 2 + x: the quadrant from m, exactly; pi / 2 in two parts, the first of 33 bits (q times it is exact, and so is the difference)
            const int q = (int)((m + (1u << 21)) >> 22);
            const double x = (t - (double)q * 1.57079632673412561417e+00) - (double)q * 6.07710050650619224932e-11;
            const double sx = sin_reduced(x), cx = cos_reduced(x);
            const double sn = (q & 1) ? ((q & 2) ? -cx : cx) : ((q & 2) ? -sx : sx);
            const double cs = (q & 1) ? ((q & 2) ? sx : -sx) : ((q & 2) ? -cx : cx);
            const double d = __dsub_rn(__dmul_rn(2.0, u(LC_AUGMENT_OP_MOTION, 2)), 1.0);
            const int c = min(max(lane - 6, 0), 24), yy = c / 5, xx = c - 5 * yy;
            double acc = 0.0;
#pragma unroll
            for (int s = -2; s <= 2; ++s) {
                const double wgt = __dadd_rn(__ddiv_rn(__dsub_rn(1.0, d), 2.0), __dmul_rn((double)(s + 2) / 4.0, d));
                const double px = __dadd_rn(2.0, __dmul_rn((double)s, sn)), py = __dsub_rn(2.0, __dmul_rn((double)s, cs));
                const int x0 = min(max((int)floor(px), 0), 4), y0 = min(max((int)floor(py), 0), 4);
                const double fx = __dsub_rn(px, (double)x0), fy = __dsub_rn(py, (double)y0);
                const double wy = yy == y0 ? __dsub_rn(1.0, fy) : fy, wx = xx == x0 ? __dsub_rn(1.0, fx) : fx;
                if ((yy == y0 || yy == y0 + 1) && (xx == x0 || xx == x0 + 1)) acc = __dadd_rn(acc, __dmul_rn(__dmul_rn(wgt, wy), wx));
            }
            const int wq = quantise25(__ddiv_rn(acc, sum25(acc, 6)), lane, 6);
            if (lane >= 6 && lane < 31) word = wq;
        }
        if (gauss) {  // lanes 31 .. 55
            const double den = __dmul_rn(2.0, __dmul_rn(sigma, sigma));
            const double e1 = exp_neg(__ddiv_rn(-1.0, den)), e2 = exp_neg(__ddiv_rn(-4.0, den));
            const double total = __dadd_rn(__dadd_rn(__dadd_rn(__dadd_rn(e2, e1), 1.0), e1), e2);
            const int c = min(max(lane - 31, 0), 24), yy = c / 5, xx = c - 5 * yy;
            const int ay = abs(yy - 2), ax = abs(xx - 2);
            const double gy = __ddiv_rn(ay == 0 ? 1.0 : ay == 1 ? e1 : e2, total), gx = __ddiv_rn(ax == 0 ? 1.0 : ax == 1 ? e1 : e2, total);
            const int wq = quantise25(__dmul_rn(gy, gx), lane, 31);
            if (lane >= 31 && lane < 56) word = wq;
        }
    }
    s_P[lane] = word;
    if (store && p.params_out) p.params_out[(size_t)b * kWords + lane] = word;

    double add_v[3], mul_pc_v[3], alpha[3];
    bool inv[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        add_v[c] = fmin(__dadd_rn(-25.0, floor(__dmul_rn(per_channel(LC_AUGMENT_OP_ADD, 0.3, c), 51.0))), 25.0);
        inv[c] = u(LC_AUGMENT_OP_INVERT, 1 + c) < 0.2;
        mul_pc_v[c] = __dadd_rn(0.6, __dmul_rn(0.8, per_channel(LC_AUGMENT_OP_MUL_PC, 0.5, c)));
        alpha[c] = __dadd_rn(0.5, __dmul_rn(1.7, per_channel(LC_AUGMENT_OP_CONTRAST, 0.3, c)));
    }
    const double mul_v = __dadd_rn(0.6, __dmul_rn(0.8, u(LC_AUGMENT_OP_MUL, 1)));
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        unsigned four = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double v = (double)(4 * lane + j);
            if (add) v = table_step(__dadd_rn(v, add_v[c]));
            if (invert && inv[c]) v = table_step(__dsub_rn(255.0, v));
            if (mul_pc) v = table_step(__dmul_rn(v, mul_pc_v[c]));
            if (mul) v = table_step(__dmul_rn(v, mul_v));
            if (contrast) v = table_step(__dadd_rn(128.0, __dmul_rn(alpha[c], __dsub_rn(v, 128.0))));
            four |= (unsigned)(int)v << (8 * j);
        }
        s_lut[c * 64 + lane] = four;
        if (store && p.lut_out) reinterpret_cast<unsigned*>(p.lut_out + (size_t)b * 768)[c * 64 + lane] = four;
    }
}

template <int DT, bool FILTERED>
__global__ __launch_bounds__(kThreads) void lc_augment_kernel(const Params p) {
    using T = typename Store<DT>::type;
    __shared__ int s_P[kWords];
    __shared__ Row s_row;
    __shared__ T s_table[768];
    __shared__ unsigned s_lut[192];  // the drawn row's tables
    __shared__ unsigned s_buf[FILTERED ? 2 * 3 * kPlaneWords : 1];

    const int tid = threadIdx.x;
    const int tiles = p.tiles_x * p.tiles_y;
    const int b = blockIdx.x / tiles, t = blockIdx.x - b * tiles;
    const int tyi = t / p.tiles_x, txi = t - tyi * p.tiles_x;
    const int ty0 = tyi * kTile, tx0 = txi * kTile;

    if (p.drawn) {  // uniform over the launch
        if (tid < 64) draw_row<FILTERED>(p, b, t == 0, tid, s_P, s_lut);
    } else if (tid < kWords) {
        s_P[tid] = p.params[(size_t)b * kWords + tid];
    }
    __syncthreads();
    if (tid == 0) {
        const int f = s_P[0];
        bool ok = (f & ~63) == 0;
        for (int j = 56; j < kWords; ++j) ok = ok && s_P[j] == 0;
        if (f & kFilterA) ok = ok && weights_ok(s_P + 6);
        if (f & kFilterB) ok = ok && weights_ok(s_P + 31);
        if (f & kDrop) ok = ok && s_P[4] >= 1 && s_P[4] <= p.h && s_P[5] >= 1 && s_P[5] <= p.w;
        if (f & kBlend) ok = ok && p.msk != nullptr && p.bg != nullptr && s_P[1] >= 0 && s_P[1] < p.G;
        if (!FILTERED && (f & (kFilterA | kFilterB))) ok = false;
        Row r;
        r.flags = ok ? f : 0;
        r.g = s_P[1], r.gh = s_P[4], r.gw = s_P[5];
        r.snp_th = (unsigned)s_P[2], r.drop_th = (unsigned)s_P[3];
        const unsigned k = row_key(p, b);
        r.k_snp = fmix32(k ^ (unsigned)LC_AUGMENT_OP_SNP);
        r.k_snpv = fmix32(k ^ (unsigned)LC_AUGMENT_OP_SNPV);
        r.k_drop = fmix32(k ^ (unsigned)LC_AUGMENT_OP_DROP);
        s_row = r;
        if (t == 0 && p.info) p.info[b] = ok ? 0 : -1;
    }
    __syncthreads();
    const Row r = s_row;

    if (tid < 192) {  // the row's LUT, four entries per lane, finished
        const unsigned word = !(r.flags & kLut) ? 0u : p.drawn ? s_lut[tid] : reinterpret_cast<const unsigned*>(p.lut + (size_t)b * 768)[tid];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = 4 * tid + j;
            const int v = (r.flags & kLut) ? (int)((word >> (8 * j)) & 0xffu) : (i & 255);
            s_table[i] = finish<DT>(v, i >> 8, p);
        }
    }

    unsigned v[3] = {0u, 0u, 0u};
    int x0, y;
    if constexpr (FILTERED) {
        const int fx0 = tx0 - kHalo, fy0 = ty0 - kHalo;
        const bool filter_a = (r.flags & kFilterA) != 0, filter_b = (r.flags & kFilterB) != 0, drop = (r.flags & kDrop) != 0;
        unsigned* head = s_buf;
        unsigned* mid = s_buf + 3 * kPlaneWords;
        for (int q = tid; q < kPlaneWords; q += kThreads) {
            const int ry = q / kFrameQuads, qx = q - ry * kFrameQuads;
            const int yy = fy0 + ry, xx = fx0 + 4 * qx;
            unsigned u[3] = {0u, 0u, 0u};
            if (yy >= 0 && yy < p.h && xx >= 0 && xx < p.w) head_quad(p, r, b, xx, yy, drop && !filter_a, u);
#pragma unroll
            for (int c = 0; c < 3; ++c) head[c * kPlaneWords + q] = u[c];
        }
        __syncthreads();
        if (filter_a) {  // uniform over the workgroup
            for (int q = tid; q < (kFrame - 4) * kFrameQuads; q += kThreads) {
                const int ry = 2 + q / kFrameQuads, qx = q % kFrameQuads;
                const int yy = fy0 + ry, xx = fx0 + 4 * qx;
                unsigned u[3] = {0u, 0u, 0u};
                if (yy >= 0 && yy < p.h && xx >= 0 && xx < p.w) {
                    // (the quad's columns 0, 1, 38, 39 of the region are formed from clamped taps and never read)
                    filter_quad(reinterpret_cast<const unsigned char*>(head), s_P + 6, fx0, fy0, xx, yy, p.h, p.w, u);
                    if (drop) drop_quad(p, r, xx, yy, u);
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) mid[c * kPlaneWords + ry * kFrameQuads + qx] = u[c];
            }
            __syncthreads();
        }
        const unsigned* src = filter_a ? mid : head;
        const int ry = kHalo + (tid >> 3), qx = 1 + (tid & 7);
        y = fy0 + ry, x0 = fx0 + 4 * qx;
        if (y >= p.h || x0 >= p.w) return;  // behind the last barrier
        if (filter_b) {
            filter_quad(reinterpret_cast<const unsigned char*>(src), s_P + 31, fx0, fy0, x0, y, p.h, p.w, v);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = src[c * kPlaneWords + ry * kFrameQuads + qx];
        }
    } else {
        __syncthreads();  // the table
        y = ty0 + (tid >> 3), x0 = tx0 + 4 * (tid & 7);
        if (y >= p.h || x0 >= p.w) return;
        head_quad(p, r, b, x0, y, (r.flags & kDrop) != 0, v);
    }

    const size_t plane = (size_t)p.h * p.w;
    T* out = static_cast<T*>(p.out) + (size_t)b * 3 * plane + (size_t)y * p.w + x0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        Vec4<T> res;
#pragma unroll
        for (int j = 0; j < 4; ++j) res.v[j] = s_table[c * 256 + ((v[c] >> (8 * j)) & 0xffu)];
        if (p.vec) {
            *reinterpret_cast<Vec4<T>*>(out + c * plane) = res;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + j < p.w) out[c * plane + j] = res.v[j];
        }
    }
}

template <int DT>
void launch(const Params& p, int form, unsigned blocks, hipStream_t s) {
    if (form == LC_AUGMENT_POINTWISE) hipLaunchKernelGGL((lc_augment_kernel<DT, false>), dim3(blocks), dim3(kThreads), 0, s, p);
    else hipLaunchKernelGGL((lc_augment_kernel<DT, true>), dim3(blocks), dim3(kThreads), 0, s, p);
}

bool misaligned(const void* q, size_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) != 0; }

// What the two entry points ask of a row's source: the arrays of lc_augment_u8, or the draw of lc_augment_drawn_u8
struct Rows {
    const int* params = nullptr;
    const unsigned char* lut = nullptr;
    uint64_t seed = 0;
    const lc_augment_draw_config* cfg = nullptr;  // the drawn call
    const uint64_t* seed_word = nullptr;
    int* params_out = nullptr;
    unsigned char* lut_out = nullptr;
};

// The rules both entry points share, in the order lc_augment_u8 has always checked them, and the launch
int run(const std::string& me, const unsigned char* crops, const unsigned char* backgrounds, int G, const float* msk_in, const Rows& rows, int B, int h, int w,
        const int* sample_id, int out_dtype, int form, const float* mean, const float* std, void* out, int* info, void* stream) {
    const bool drawn = rows.cfg != nullptr;
    if (B < 0) return fail(1, me + "B < 0");
    if (B == 0) return 0;
    if (G < 0) return fail(2, me + "G < 0");
    const int lo = LC_AUGMENT_MIN_SIZE, hi = LC_AUGMENT_MAX_SIZE;
    if (h < lo || w < lo || h > hi || w > hi)
        return fail(3, me + "crop sizes must be in [" + std::to_string(lo) + ", " + std::to_string(hi) + "], got " + std::to_string(h) + " x " + std::to_string(w));
    if (out_dtype < LC_AUGMENT_U8 || out_dtype > LC_AUGMENT_BF16) return fail(4, me + "unknown out_dtype " + std::to_string(out_dtype));
    if (form != LC_AUGMENT_FILTERED && form != LC_AUGMENT_POINTWISE) return fail(5, me + "form must be LC_AUGMENT_FILTERED or LC_AUGMENT_POINTWISE");
    if ((mean == nullptr) != (std == nullptr)) return fail(6, me + "mean and std come together");
    if (mean && out_dtype == LC_AUGMENT_U8) return fail(6, me + "mean and std need a float output");
    if (drawn) {
        if (!crops || !out) return fail(7, me + "crops and out must not be NULL");
        if (!rows.seed_word) return fail(12, me + "seed must not be NULL: it points to one uint64 on the device");
        if (!sample_id) return fail(13, me + "sample_id must not be NULL: a drawn row belongs to its sample");
    } else if (!crops || !rows.params || !rows.lut || !out) {
        return fail(7, me + "crops, params, lut and out must not be NULL");
    }
    if ((G > 0) != (backgrounds != nullptr)) return fail(8, me + "backgrounds is NULL exactly when G = 0");
    if (drawn) {
        const lc_augment_draw_config& c = *rows.cfg;
        if (!(c.pixel_aug_prob >= 0.0 && c.pixel_aug_prob <= 1.0)) return fail(14, me + "pixel_aug_prob must lie in [0, 1], got " + std::to_string(c.pixel_aug_prob));
        if (!(c.switch_bg_prob >= 0.0 && c.switch_bg_prob <= 1.0)) return fail(14, me + "switch_bg_prob must lie in [0, 1], got " + std::to_string(c.switch_bg_prob));
        if (c.n_backgrounds < 0 || c.n_backgrounds > G)
            return fail(15, me + "n_backgrounds = " + std::to_string(c.n_backgrounds) + " without as many backgrounds (G = " + std::to_string(G) + ")");
    }
    const size_t elem = out_dtype == LC_AUGMENT_U8 ? 1 : out_dtype == LC_AUGMENT_F32 ? 4 : 2;
    if (misaligned(rows.params, 4) || misaligned(rows.lut, 4) || misaligned(msk_in, 4) || misaligned(sample_id, 4) || misaligned(info, 4) || misaligned(out, elem))
        return fail(9, me + "params, lut, msk_in, sample_id, info and out must be aligned to their element (lut to 4 bytes)");
    if (misaligned(rows.seed_word, 8) || misaligned(rows.params_out, 4) || misaligned(rows.lut_out, 4))
        return fail(9, me + "seed must be aligned to 8 bytes, params_out and lut_out to 4");

    Params p{};
    p.crops = crops; p.bg = backgrounds; p.msk = msk_in; p.params = rows.params; p.lut = rows.lut; p.sample_id = sample_id;
    p.out = out; p.info = info;
    p.B = B; p.G = G; p.h = h; p.w = w;
    p.tiles_x = (w + kTile - 1) / kTile;
    p.tiles_y = (h + kTile - 1) / kTile;
    p.vec = (w % 4 == 0) && !misaligned(crops, 4) && !misaligned(backgrounds, 4) && !misaligned(msk_in, 16) && !misaligned(out, 4 * elem);
    p.normalize = mean != nullptr;
    for (int c = 0; c < 3 && mean; ++c) p.mean[c] = mean[c], p.std[c] = std[c];
    p.seed_lo = (unsigned)(rows.seed & 0xffffffffull); p.seed_hi = (unsigned)(rows.seed >> 32);
    if (drawn) {
        p.drawn = 1; p.cfg = *rows.cfg;
        p.seed = reinterpret_cast<const unsigned long long*>(rows.seed_word);
        p.params_out = rows.params_out; p.lut_out = rows.lut_out;
    }
    const long long blocks = (long long)B * p.tiles_x * p.tiles_y;
    if (blocks > 0x7fffffffLL) return fail(10, me + "too many rows and tiles for one launch");

    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (out_dtype) {
        case LC_AUGMENT_U8: launch<LC_AUGMENT_U8>(p, form, (unsigned)blocks, s); break;
        case LC_AUGMENT_F32: launch<LC_AUGMENT_F32>(p, form, (unsigned)blocks, s); break;
        case LC_AUGMENT_F16: launch<LC_AUGMENT_F16>(p, form, (unsigned)blocks, s); break;
        default: launch<LC_AUGMENT_BF16>(p, form, (unsigned)blocks, s); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(11, me + "launch: " + hipGetErrorString(e));
    return 0;
}

}  // namespace
}  // namespace lc

#pragma GCC visibility push(default)
extern "C" {

int lc_amd_augment_version(void) { return LC_AMD_AUGMENT_VERSION; }
const char* lc_amd_augment_source_hash(void) { return lc::kSrcHash + sizeof("LC_AMD_AUGMENT_SRC_HASH:") - 1; }
const char* lc_amd_augment_last_error(void) { return lc::g_err.c_str(); }

int lc_augment_u8(const unsigned char* crops, const unsigned char* backgrounds, int G, const float* msk_in, const int* params, const unsigned char* lut,
                  int B, int h, int w, uint64_t seed, const int* sample_id, int out_dtype, int form, const float* mean, const float* std, void* out,
                  int* info, void* stream) {
    lc::Rows rows;
    rows.params = params; rows.lut = lut; rows.seed = seed;
    return lc::run("lc_augment_u8: ", crops, backgrounds, G, msk_in, rows, B, h, w, sample_id, out_dtype, form, mean, std, out, info, stream);
}

int lc_augment_drawn_u8(const unsigned char* crops, const unsigned char* backgrounds, int G, const float* msk_in, lc_augment_draw_config cfg,
                        const uint64_t* seed, const int* sample_id, int B, int h, int w, int out_dtype, const float* mean, const float* std, void* out,
                        int* info, int* params_out, unsigned char* lut_out, void* stream) {
    lc::Rows rows;
    rows.cfg = &cfg; rows.seed_word = seed; rows.params_out = params_out; rows.lut_out = lut_out;
    // both filters stand behind the chain's gate: a chain that never opens rules them out, and the launch streams without a halo
    const int form = cfg.pixel_aug_prob == 0.0 ? LC_AUGMENT_POINTWISE : LC_AUGMENT_FILTERED;
    return lc::run("lc_augment_drawn_u8: ", crops, backgrounds, G, msk_in, rows, B, h, w, sample_id, out_dtype, form, mean, std, out, info, stream);
}

}  // extern "C"
#pragma GCC visibility pop
