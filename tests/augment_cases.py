"""The case list of the augmentation tests: the smallest shapes at which the launch of lc_augment.hip can go wrong, and seeded inputs.

Sizes: 8 is the lower limit and a single partial tile; 31 / 32 / 33 lie around the 32-pixel tile edge (33: a second tile of ONE pixel, whose
halo is all reflection); 40 is the staged region's side; 65 is three tiles with a one-pixel last one, so that a halo crosses a tile edge
and the image border at once.  Every value is taken by h and by w; 8, 32 and 40 are multiples of four (four-pixel loads and stores), the
others are not (element by element)."""
import numpy as np

SIZES = ((8, 8), (31, 40), (32, 32), (33, 65), (40, 31), (65, 33))
G = 2
SWITCH, SALT, FILTER_A, DROPOUT, FILTER_B, LUT = 1, 2, 4, 8, 16, 32
# each stage alone, every pair of neighbouring stages, A -> dropout -> B (the reflected-halo chain), everything, nothing
STAGE_SETS = (SWITCH, SALT, FILTER_A, DROPOUT, FILTER_B, LUT,
              SWITCH | SALT, SALT | FILTER_A, FILTER_A | DROPOUT, DROPOUT | FILTER_B, FILTER_B | LUT,
              FILTER_A | DROPOUT | FILTER_B, 63, 0, SALT | FILTER_B)
BATCHES = tuple(STAGE_SETS[i:i + 3] for i in range(0, len(STAGE_SETS), 3))  # B = 3, different stage sets per row
POINTWISE_BATCHES = ((SWITCH, SALT, DROPOUT), (LUT, SWITCH | SALT, 0), (SALT | DROPOUT, SWITCH | SALT | DROPOUT | LUT, DROPOUT | LUT))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SEED = 0x1234_5678_9ABC_DEF1  # both halves of the seed in use


def random_weights(rng):
    """25 non-negative Q16 weights without any symmetry that sum to 65536 (a transposed or mirrored kernel changes bytes)."""
    g = rng.random(25) ** 3
    q = np.floor(g / g.sum() * 65536.0).astype(np.int64)
    q[int(rng.integers(25))] += 65536 - int(q.sum())
    return q


def make_params(bits, rng, h, w):
    """One row with the stages `bits` on.  The dropout's threshold lies above 2^31 (a negative int32: the comparison is unsigned)."""
    P = np.zeros(64, dtype=np.int64)
    P[0] = bits
    P[1] = rng.integers(G)
    P[2] = int(0.3 * 2 ** 32)
    P[3] = int(0.6 * 2 ** 32)
    P[4], P[5] = rng.integers(1, min(h, 7) + 1), rng.integers(1, min(w, 7) + 1)
    P[6:31], P[31:56] = random_weights(rng), random_weights(rng)
    return (P & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def make_inputs(h, w, B, seed):
    """crops, backgrounds (G), msk_in with many 0, 1 and exact ties (k = 512 against odd and even sums), lut (B,3,256)."""
    rng = np.random.default_rng(seed)
    crops = rng.integers(0, 256, (B, 3, h, w), dtype=np.uint8)
    backgrounds = rng.integers(0, 256, (G, 3, h, w), dtype=np.uint8)
    k = rng.choice(np.array([0, 1024, 512, 1, 1023, 300, 777]), size=(B, h, w), p=[0.2, 0.2, 0.3, 0.05, 0.05, 0.1, 0.1])
    msk = (k / 1024.0).astype(np.float32)
    lut = rng.integers(0, 256, (B, 3, 256), dtype=np.uint8)
    return crops, backgrounds, msk, lut


def make_batch(stage_sets, h, w, seed):
    rng = np.random.default_rng(seed + 1000)
    crops, backgrounds, msk, lut = make_inputs(h, w, len(stage_sets), seed)
    params = np.stack([make_params(bits, rng, h, w) for bits in stage_sets])
    return crops, backgrounds, msk, params, lut
