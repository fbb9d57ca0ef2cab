"""The case list of the background-store tests: the smallest stores and crops at which lc_bgstore.hip can go wrong, and seeded inputs.

Stores: three images of 5 x 7 (smaller than every crop: the whole image is stretched), 48 x 64 (rows of 192 bytes) and 37 x 101 (rows of
303 bytes: no image row but the first starts on a multiple of four, and the image's length is odd, so the next start is rounded up);
and a store of one image.  Crops: (8, 8) is one quad row of two four-pixel groups, (31, 40) takes the four-pixel loads and stores,
(33, 65) goes element by element and ends a row in a group of one pixel (tests/augment_cases.SIZES).  Twelve rows, ids 0..11, at the
seed of the augmentation tests: with the default config rows 1, 2, 4, 5, 6, 7, 9 switch to images 1, 0, 0, 2, 1, 1, 2 of three and five
rows stay closed (tests/test_bgstore_host.py asserts it)."""
import functools

import numpy as np

from tests import augment_cases

SEED = augment_cases.SEED  # 0x1234_5678_9ABC_DEF1
IDS = np.arange(12, dtype=np.int32)
SWITCHED = {1: 1, 2: 0, 4: 0, 5: 2, 6: 1, 7: 1, 9: 2}  # row -> image, G = 3, default AugmentConfig
STORES = {"three": ((5, 7), (48, 64), (37, 101)), "one": ((37, 101),)}
SIZES = ((8, 8), (31, 40), (33, 65))
CASES = tuple((store, hw) for store in STORES for hw in SIZES)


def make_images(store):
    """The store's images: noise, so that a tap one pixel or one byte off changes the cut."""
    rng = np.random.default_rng(len(STORES[store]) + 40)
    return [rng.integers(0, 256, (hb, wb, 3), dtype=np.uint8) for hb, wb in STORES[store]]


def make_inputs(h, w, seed=11):
    """crops (B,3,h,w) uint8 noise (the sentinel: an untouched byte is recognised) and msk_in (B,h,w) float32: many 0, 1 and k = 512
    (S & 1023 == 512 wherever fg + bg is odd, towards an even and towards an odd neighbour), other k / 1024, and in every row's first
    two lines a group of four ones beside a mixed group, a NaN (k = 0) and 1.5 (k = 1024)."""
    rng = np.random.default_rng(seed + 131 * h + w)
    B = len(IDS)
    crops = rng.integers(0, 256, (B, 3, h, w), dtype=np.uint8)
    k = rng.choice(np.array([0, 1024, 512, 1, 1023, 300, 777]), size=(B, h, w), p=[0.2, 0.2, 0.3, 0.05, 0.05, 0.1, 0.1])
    msk = (k / 1024.0).astype(np.float32)
    msk[:, 0, 0:4] = 1.0
    msk[:, 0, 4:8] = np.array([1.0, 0.5, 0.0, 1.0], dtype=np.float32)
    msk[:, 1, 0], msk[:, 1, 1] = np.nan, 1.5
    msk[:, 1, 4:8] = 1.0
    return crops, msk


@functools.lru_cache(maxsize=None)
def reference(store, hw):
    """One case's inputs and the oracle's outputs, computed once and shared (nobody writes into them):
    dict(images, crops, msk, out, info, which, M) with the default AugmentConfig."""
    from lc_amd import augment
    from tests import bgstore_oracle

    images = make_images(store)
    crops, msk = make_inputs(*hw)
    out, info, which, M = bgstore_oracle.switch(crops, images, augment.AugmentConfig(), SEED, IDS, msk)
    return dict(images=images, crops=crops, msk=msk, out=out, info=info, which=which, M=M)
