"""Frames, keypoint lists and sampling tables shared by tests/test_gpu_describe_dev.py and tests/test_describe_host.py: the CPU test shows on the
same inputs that describe()'s border drop really happens, which is the GPU cases' precondition."""
import numpy as np

SINGLE_SHAPES = ((120, 160), (93, 131))          # the second: odd H, so the pyramid's column pitch (96) differs from H
WINDOWS = (5, 9, 15)
SET_SHAPE, SET_S, SET_MAX_POINTS, SET_GRID, SET_CELL = (120, 160), 3, 150, (4, 5), 35
WIDE_SHAPE, WIDE_S, WIDE_MAX_POINTS, WIDE_GRID = (64, 80), 72, 60, (2, 3)

_CACHE = {}


def q8(img):
    return np.asfortranarray(np.round(np.asarray(img) * 255).astype(np.uint8))


def as_f64(u8):
    """Gray{Float64} of an 8-bit frame: raw / 255"""
    return np.asfortranarray(u8.astype(np.float64) / 255.0)


def frames(syn, H, W, seed, n=2, step=(1.3, -2.1)):
    """n consecutive left frames of a synthetic stream as (float64 image, u8 image) pairs"""
    key = (H, W, seed, n, step)
    if key not in _CACHE:
        L, _, flows = syn.stereo_stream((H, W), n, seed, step, 6.3)
        _CACHE[key] = ([(np.asfortranarray(im), q8(im)) for im in L], flows)
    return _CACHE[key]


def set_stream(syn, s):
    return frames(syn, *SET_SHAPE, seed=30 + s, step=(1.0 + 0.2 * s, -1.4))


def wide_frame(syn, s):
    """stream s of the 72-stream case: a window of one larger texture (one canvas for all streams keeps the case quick)"""
    key = ("wide",)
    if key not in _CACHE:
        H, W = WIDE_SHAPE
        _CACHE[key] = q8(syn.texture_canvas(4 * H, 18 * W + 8, seed=77, margin=0))
    H, W = WIDE_SHAPE
    r, c = divmod(s, 18)
    return np.asfortranarray(_CACHE[key][r * H:(r + 1) * H, c * W + (s % 7):c * W + (s % 7) + W])


def edge_pattern(n_bits, window, seed=7):
    """a sampling table whose offsets reach +-lim (lim = (window + 1) / 2, one past ImageFeatures' +-window / 2) in all four columns"""
    lim = (window + 1) // 2
    rng = np.random.default_rng(seed + window)
    p = rng.integers(-lim, lim + 1, (n_bits, 4)).astype(np.int32)
    p[:4] = [[lim, lim, -lim, -lim], [-lim, -lim, lim, lim], [lim, -lim, -lim, lim], [-lim, lim, lim, -lim]]
    return p


def hand_placed(H, W, window):
    """(kept, dropped): the four corners of the region describe() keeps; one-pixel outside neighbours of each and the image corners"""
    lim = (window + 1) // 2
    kept = np.array([[lim + 1, lim + 1], [H - lim, W - lim], [lim + 1, W - lim], [H - lim, lim + 1]], dtype=np.int64)
    dropped = np.array([[lim, lim + 1], [H - lim + 1, W - lim], [lim + 1, W - lim + 1], [H - lim, lim], [1, 1], [H, W]], dtype=np.int64)
    return kept, dropped
