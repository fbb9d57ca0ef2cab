"""Cases shared by tests/test_sampler_host.py and tests/test_gpu_sampler.py: hand-written selections with their expected results, the
patterns the device test scales to any number of rows, and a small annotation table."""
import numpy as np

TH = 100

# (name, valid_cnt, info, batch, expected take, expected shortfall) with valid_th = TH
SELECT_CASES = (
    ("all rows good", [100, 500, 101, 100, 300, 100], [0, 0, 0, 0, 0, 0], 3, [0, 1, 2], 0),
    ("no spare good", [100, 0, 99, 100, 99, 0, 50], [0, 0, 0, 0, 0, 0, 0], 4, [0, -1, -1, 3], 2),
    ("more bad primaries than good spares", [0, 0, 200, 0, 0, 300, 0, 400], [0, 0, 0, 0, 0, 0, 0, 0], 5, [5, 7, 2, -1, -1], 2),
    ("info = -1 on a primary and on a spare", [500, 500, 500, 500, 500, 500], [0, -1, 0, -1, 0, 0], 3, [0, 4, 2], 0),
    ("valid_cnt == valid_th is good, valid_th - 1 is bad", [TH, TH - 1, TH - 1, TH], [0, 0, 0, 0], 2, [0, 3], 0),
    ("one row", [5], [0], 1, [-1], 1),
)


def select_pattern(name, rows, batch, rng=None):
    """(valid_cnt, info) int32 of `rows` rows for the named pattern."""
    cnt, info = np.full(rows, TH, np.int32), np.zeros(rows, np.int32)
    if name == "all good":
        pass
    elif name == "no spare good":
        cnt[::2] = TH - 1
        cnt[batch:] = 0
    elif name == "more bad than spares":
        cnt[:batch] = 0
        cnt[batch:] = np.where(np.arange(rows - batch) % 3 == 0, TH, TH - 1)
    elif name == "info":
        info[1::3] = -1
    elif name == "threshold":
        cnt[:] = np.where(np.arange(rows) % 2 == 0, TH - 1, TH)
    elif name == "random":
        cnt[:] = rng.integers(TH - 2, TH + 2, rows)
        info[:] = -(rng.random(rows) < 0.2).astype(np.int32)
    else:
        raise KeyError(name)
    return cnt, info


PATTERNS = ("all good", "no spare good", "more bad than spares", "info", "threshold", "random")


def table_columns(n, seed=0, n_frames=3, n_masks=None, n_meshes=2):
    """Ten columns of n annotations with distinct, recognisable values."""
    rng = np.random.default_rng(seed)
    n_masks = n if n_masks is None else n_masks
    K = np.tile(np.array([[572.4, 0.0, 325.3], [0.0, 573.6, 242.0], [0.0, 0.0, 1.0]], np.float32), (n, 1, 1))
    K[:, 0, 2] += np.arange(n, dtype=np.float32)
    return dict(frame_index=(np.arange(n) % n_frames).astype(np.int32), mask_index=(np.arange(n) % n_masks).astype(np.int32),
                mesh_index=(np.arange(n) % n_meshes).astype(np.int32), obj_id=(np.arange(n) * 3 + 1).astype(np.int32), scene_id=(np.arange(n) // 4).astype(np.int32),
                im_id=(1000 - np.arange(n)).astype(np.int32), bbox_xyxy=rng.uniform(0, 60, (n, 4)).astype(np.float32), cam_K=K,
                R=rng.standard_normal((n, 3, 3)).astype(np.float32), t=rng.standard_normal((n, 3)).astype(np.float32))
