"""Fixed points and batches of the crop-geometry tests (tests/test_geometry_host.py).

EDGE_DRAWS: (numerator k of u4 = k / 2^24, seed, sample_id) with `augment.u(seed, sample_id, OP_ZOOM, 4) == k / 2^24`, found once by a
search over sample ids on the CPU: u4 on each of the 16 octant edges j / 16 (the reduced argument is 0 there, or pi / 4 coming from
above), and on the largest draw (2^24 - 1) / 2^24.  u4 = 0 is the first entry."""
import numpy as np

EDGE_DRAWS = (
    (0 << 20, 7, -14679698), (1 << 20, 7, -12358399), (2 << 20, 7, -13965215), (3 << 20, 7, -5424212), (4 << 20, 7, -13561381),
    (5 << 20, 7, -5229743), (6 << 20, 7, -8585743), (7 << 20, 4294967301, -13209358), (8 << 20, 7, -11608645),
    (9 << 20, 9223372036854788153, -16310712), (10 << 20, 7, -15855061), (11 << 20, 4294967301, -9712841), (12 << 20, 7, -9406957),
    (13 << 20, 9223372036854788153, -8436640), (14 << 20, 9223372036854788153, -13905400), (15 << 20, 7, -14619390),
    ((1 << 24) - 1, 4294967301, -10786831),
)
EDGE_SEEDS = tuple(sorted({s for _, s, _ in EDGE_DRAWS}))


def edge_ids(seed):
    return np.array([i for _, s, i in EDGE_DRAWS if s == seed], dtype=np.int64)


def batch(B, seed=0, im_hw=(480, 640), cameras=("rot", "bop", "stress")):
    """B rows: sample ids that are negative, repeated and large; boxes inside the frame, some so large that the scale meets the
    max(im_h, im_w) clamp; the cameras named (lc_amd.synth.CAMERAS; tests/camera_cases.py names the skewed and stretched ones) cycled over the rows.  -> ids (B,) int64, box (B,4) f32, K (B,3,3) f32"""
    import torch

    from lc_amd import synth

    rng = np.random.default_rng(1000 + seed)
    ids = rng.integers(-2 ** 31, 2 ** 31, size=B, dtype=np.int64)
    ids[::7] = ids[0]
    if B > 2:
        ids[1], ids[2] = -1, 2 ** 31 - 1
    H, W = im_hw
    x1, y1 = rng.uniform(0, W * 0.6, B), rng.uniform(0, H * 0.6, B)
    w, h = rng.uniform(4, W * 0.4, B), rng.uniform(4, H * 0.4, B)
    big = np.arange(B) % 5 == 3
    w[big], h[big] = W * 0.9, H * 0.95  # 1.5 x the larger side exceeds max(H, W): clamped whatever the draw
    box = np.stack((x1, y1, x1 + w, y1 + h), axis=1).astype(np.float32)
    f, th = torch.from_numpy(rng.uniform(400, 1200, B)), torch.from_numpy(rng.uniform(-0.3, 0.3, B))
    cx, cy = torch.from_numpy(rng.uniform(0.4, 0.6, B) * W), torch.from_numpy(rng.uniform(0.4, 0.6, B) * H)
    K = np.stack([synth.crop_camera(f[i:i + 1], th[i:i + 1], cx[i:i + 1], cy[i:i + 1], cameras[i % len(cameras)])[0].numpy() for i in range(B)]).astype(np.float32)
    return ids, box, K
