"""The 8-bit conversion of the blit (rt_quantize_rgba8 / rt_present) restated in numpy, and the
floats both test files try it on (tests/test_present_cpu.py, tests/test_gpu_present.py).

The rule, per channel v of r, g, b in binary32 without contraction: NaN -> 0, v <= 0 -> 0,
v >= 1 -> 255, else (uint8)(v * 255.0f + 0.5f) truncated; alpha 255."""
import numpy as np

F32 = np.float32
ONE_BITS = 0x3F800000


def from_bits(bits) -> np.ndarray:
    return np.asarray(bits, np.uint32).view(np.float32)


def q_ref(v) -> np.ndarray:
    """The rule on a float32 array of channel values -> uint8, every step in float32."""
    v = np.asarray(v, np.float32)
    out = np.zeros(v.shape, np.uint8)
    with np.errstate(invalid="ignore"):
        mid = (v > F32(0.0)) & (v < F32(1.0))
        pre = v[mid] * F32(255.0) + F32(0.5)
        assert pre.dtype == np.float32
        out[mid] = pre.astype(np.int32).astype(np.uint8)  # 0 < pre < 256: the cast truncates
        out[v >= F32(1.0)] = 255
    return out


def quantize_ref(img, top_down: bool) -> np.ndarray:
    """q_ref on an [R][W][4] image: r, g, b converted, alpha 255, rows reversed when top_down."""
    img = np.asarray(img, np.float32)
    out = np.empty(img.shape, np.uint8)
    out[..., :3] = q_ref(img[..., :3])
    out[..., 3] = 255
    return out[::-1].copy() if top_down else out


def steps() -> np.ndarray:
    """Bit patterns of the smallest float with Q >= k, k = 1..255, by bisection on q_ref over the
    bit patterns 0 .. 0x3f800000 (Q is non-decreasing there)."""
    k = np.arange(1, 256)
    lo = np.zeros(255, np.int64)              # Q(lo) < k
    hi = np.full(255, ONE_BITS, np.int64)     # Q(hi) >= k
    while (hi - lo > 1).any():
        mid = (lo + hi) // 2
        ge = q_ref(from_bits(mid.astype(np.uint32))) >= k
        hi = np.where(ge, mid, hi)
        lo = np.where(ge, lo, mid)
    return hi.astype(np.uint32)


SPECIAL_BITS = np.array([
    0x00000000, 0x80000000,              # +-0
    0x00000001, 0x80000001,              # smallest subnormals
    0x007FFFFF, 0x807FFFFF,              # largest subnormals
    0x7F800000, 0xFF800000,              # +-inf
    0x7FC00000, 0xFFC00000,              # quiet NaNs
    0x7F800001, 0xFF800001,              # signalling NaNs
    0x3F7FFFFF, 0x3F800000, 0x3F800001,  # 1 - 1 ulp, 1, 1 + 1 ulp
], np.uint32)


def specials() -> np.ndarray:
    return np.concatenate([from_bits(SPECIAL_BITS), np.array([-1e-30, 1e30], np.float32)])


def value_set() -> np.ndarray:
    """Every float the CPU test converts: the 255 steps with two neighbours on each side,
    float32(k / 255), the specials and 1e5 seeded random floats in [-0.5, 1.5)."""
    s = steps().astype(np.int64)
    near = (s[:, None] + np.arange(-2, 3)[None, :]).reshape(-1).astype(np.uint32)
    exact = (np.arange(256) / 255.0).astype(np.float32)
    rnd = (np.random.default_rng(20261).random(100_000, np.float32) * F32(2.0) - F32(0.5)).astype(np.float32)
    return np.concatenate([from_bits(near), exact, specials(), rnd])


def as_image(vals, w=None) -> np.ndarray:
    """Channel values, three to a pixel (the tail repeats the head), as a [1][n][4] image; alpha = w
    or, when None, the pixel's red value."""
    vals = np.asarray(vals, np.float32)
    n = (vals.size + 2) // 3
    v = np.resize(vals, 3 * n).reshape(1, n, 3)
    img = np.empty((1, n, 4), np.float32)
    img[..., :3] = v
    img[..., 3] = v[..., 0] if w is None else w
    return img
