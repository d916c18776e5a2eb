"""rt_resample_rgba8 (rt_host.cpp): the blit at window size (src/main.cpp:783-797, the texture sampled
with GL_LINEAR and GL_CLAMP_TO_EDGE, 381-388) on the host, the specification the device kernel of
rt_present_scaled is compared with byte for byte (tests/test_gpu_present_scaled.py).  No GPU.

The rule (include/rt/abi.h), restated here op by op in float32 numpy.  For output column i of out_w
over W texels, in integers: n = (2i + 1) W - out_w, d = 2 out_w, x0 = floor(n / d), rem = n - x0 d,
a = float32(rem) / float32(d); taps clamp(x0) and clamp(x0 + 1).  Rows likewise (y0, y1, b).  Per
channel h = (a == 0) ? t0 : (1 - a) t0 + a t1 on both rows, v = (b == 0) ? h0 : (1 - b) h0 + b h1,
then the 8-bit conversion of tests/present_values.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from present_values import q_ref, specials, value_set
from real_time_ray_tracer_amd import _lib, quantize_rgba8, resample_rgba8
from test_present_cpu import SAN_FLAGS

F32 = np.float32
SOURCES = [(1, 1), (2, 3), (7, 5), (44, 33), (64, 48)]  # (W, R)


def outputs(W, R):
    return [(1, 1), (3, 2), (W, R), (2 * W, 2 * R), (2 * W + 1, 3 * R - 1), (max(1, W // 2), max(1, R // 3)),
            (192, 108)]


CASES = [(W, R, ow, oh) for W, R in SOURCES for ow, oh in outputs(W, R)]


def taps(n_out: int, n_src: int):
    """One axis of the rule: the two clamped taps and the float32 weight of the second."""
    i = np.arange(n_out, dtype=np.int64)
    n = (2 * i + 1) * n_src - n_out
    d = 2 * n_out
    x0 = n // d  # numpy's // floors, also for the negative n of the first samples
    rem = n - x0 * d
    assert ((rem >= 0) & (rem < d)).all()
    a = rem.astype(np.float32) / F32(d)
    assert a.dtype == np.float32
    return np.clip(x0, 0, n_src - 1), np.clip(x0 + 1, 0, n_src - 1), a


def mix(w, t0, t1):
    with np.errstate(invalid="ignore", over="ignore"):
        m = (F32(1.0) - w) * t0 + w * t1
    assert m.dtype == np.float32
    return np.where(w == F32(0.0), t0, m)


def resample_ref(img, ow: int, oh: int, top_down: bool) -> np.ndarray:
    img = np.asarray(img, np.float32)
    R, W = img.shape[:2]
    x0, x1, a = taps(ow, W)
    y0, y1, b = taps(oh, R)
    c = img[..., :3]
    a = a[None, :, None]
    h0 = mix(a, c[y0][:, x0], c[y0][:, x1])
    h1 = mix(a, c[y1][:, x0], c[y1][:, x1])
    v = mix(b[:, None, None], h0, h1)
    out = np.empty((oh, ow, 4), np.uint8)
    out[..., :3] = q_ref(v)
    out[..., 3] = 255
    return out[::-1].copy() if top_down else out


def bilinear_f64(img, ow: int, oh: int) -> np.ndarray:
    """Bottom-up bilinear sampling and the conversion in float64 (no NaN in img)."""
    c = np.asarray(img, np.float64)[..., :3]
    R, W = c.shape[:2]

    def axis(n_out, n_src):
        x = (np.arange(n_out) + 0.5) * n_src / n_out - 0.5
        f = np.floor(x)
        return (np.clip(f, 0, n_src - 1).astype(int), np.clip(f + 1, 0, n_src - 1).astype(int), x - f)

    x0, x1, a = axis(ow, W)
    y0, y1, b = axis(oh, R)
    a, b = a[None, :, None], b[:, None, None]
    h0 = (1 - a) * c[y0][:, x0] + a * c[y0][:, x1]
    h1 = (1 - a) * c[y1][:, x0] + a * c[y1][:, x1]
    v = (1 - b) * h0 + b * h1
    return np.where(v >= 1, 255, np.where(v > 0, np.floor(v * 255 + 0.5), 0)).astype(np.uint8)


def random_image(W, R, seed):
    return (np.random.default_rng(seed).random((R, W, 4), np.float32) * F32(1.2) - F32(0.1)).astype(np.float32)


def value_image(W, R, start=0):
    """[R][W][4] tiled from the 8-bit conversion's value set (NaN, infinities and negatives included)."""
    return np.resize(np.roll(VALUES, -start), R * W * 4).reshape(R, W, 4).astype(np.float32)


# the set shuffled, behind its specials (NaNs, infinities, subnormals), so that small images hold them too
VALUES = value_set()
VALUES = np.concatenate([specials(), VALUES[np.random.default_rng(12).permutation(VALUES.size)]])


@pytest.mark.parametrize("top_down", [False, True])
@pytest.mark.parametrize("W,R", [(1, 1), (5, 1), (1, 7), (67, 5), (257, 100)])
def test_identity_is_the_1_to_1_conversion(W, R, top_down):
    """Equal sizes: every weight is exactly 0, so the neighbour taps (NaN and infinities among them)
    never count and the bytes are quantize_rgba8's.  257 x 100 holds the whole value set."""
    assert 257 * 100 * 4 >= VALUES.size
    img = value_image(W, R)
    assert W * R < 5 or (np.isnan(img).any() and np.isinf(img).any() and (img < 0).any())
    got = resample_rgba8(img, W, R, top_down)
    assert got.shape == (R, W, 4) and got.dtype == np.uint8
    assert np.array_equal(got, quantize_rgba8(img, top_down))


@pytest.mark.parametrize("W,R,ow,oh", CASES)
def test_equals_the_restatement(W, R, ow, oh):
    for k, img in enumerate((random_image(W, R, 100 + W), value_image(W, R, start=W * 31 + ow))):
        for top_down in (False, True):
            got = resample_rgba8(img, ow, oh, top_down)
            want = resample_ref(img, ow, oh, top_down)
            bad = np.argwhere(got != want)
            assert bad.size == 0, (f"image {k} top_down {top_down}: {len(bad)} bytes differ; first at "
                                   f"{tuple(bad[0])}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}")


def ramp_row(n):
    """One row whose red channel is 16 k / 255: a blend with weight 1/4, 1/2 or 3/4 of neighbours lands
    on an integer / 255, so v * 255 + 0.5 sits mid-step and no rounding can move the byte."""
    img = np.zeros((1, n, 4), np.float32)
    img[0, :, 0] = (16 * np.arange(n) / 255.0).astype(np.float32)
    return img


def test_known_weights_4_to_8():
    x0, x1, a = taps(8, 4)
    assert a.tolist() == [0.75, 0.25] * 4
    assert list(zip(x0.tolist(), x1.tolist())) == [(0, 0), (0, 1), (0, 1), (1, 2), (1, 2), (2, 3), (2, 3), (3, 3)]
    got = resample_rgba8(ramp_row(4), 8, 1, False)
    assert got[0, :, 0].tolist() == [0, 4, 12, 20, 28, 36, 44, 48]  # (1 - a) * 16 k0 + a * 16 k1
    assert (got[0, :, 1:3] == 0).all() and (got[..., 3] == 255).all()


def test_known_weights_6_to_3():
    x0, x1, a = taps(3, 6)
    assert a.tolist() == [0.5] * 3 and list(zip(x0.tolist(), x1.tolist())) == [(0, 1), (2, 3), (4, 5)]
    got = resample_rgba8(ramp_row(6), 3, 1, False)
    assert got[0, :, 0].tolist() == [8, 40, 72]
    # the same ramp as a column
    col = np.ascontiguousarray(ramp_row(6).transpose(1, 0, 2))
    assert resample_rgba8(col, 1, 3, False)[:, 0, 0].tolist() == [8, 40, 72]
    assert resample_rgba8(col, 1, 3, True)[:, 0, 0].tolist() == [72, 40, 8]


@pytest.mark.parametrize("k", [0, 1, 127, 128, 254])
def test_constant_image_stays_constant(k):
    """(k + 0.25) / 255 sits mid-step: (1 - a) c + a c may be an ulp off c and still gives byte k."""
    img = np.full((5, 7, 4), F32((k + 0.25) / 255.0), np.float32)
    got = resample_rgba8(img, 19, 11, False)
    assert (got[..., :3] == k).all() and (got[..., 3] == 255).all()


@pytest.mark.parametrize("W,R,ow,oh", CASES)
def test_against_a_float64_bilinear(W, R, ow, oh):
    """The float32 rule against the same filter in float64: no byte off by more than one level, at
    most 0.1% of a case's bytes off at all (over all 35 cases the rule differs in a handful)."""
    img = random_image(W, R, 500 + W)
    got = resample_rgba8(img, ow, oh, False)[..., :3].astype(int)
    want = bilinear_f64(img, ow, oh).astype(int)
    diff = np.abs(got - want)
    print(f"\n{W}x{R} -> {ow}x{oh}: {int((diff > 0).sum())} of {diff.size} bytes differ, max {int(diff.max())}")
    assert diff.max() <= 1
    assert (diff > 0).sum() <= 0.001 * diff.size


@pytest.mark.parametrize("W,R,ow,oh", [(1, 1, 3, 2), (7, 5, 15, 14), (7, 5, 3, 1), (44, 33, 192, 108)])
def test_top_down_is_the_rows_reversed(W, R, ow, oh):
    img = value_image(W, R, start=5)
    up = resample_rgba8(img, ow, oh, top_down=False)
    down = resample_rgba8(img, ow, oh, top_down=True)
    assert up.shape == (oh, ow, 4)
    assert np.array_equal(down, up[::-1])
    assert np.array_equal(down, resample_rgba8(img, ow, oh))  # top_down is the default, as quantize_rgba8's


@pytest.mark.parametrize("special", [float("nan"), float("inf"), float("-inf")])
def test_zero_weight_taps_do_not_leak(special):
    """Weights are exactly 0 where (2i + 1) W - out_w is a multiple of 2 out_w: at W = 3 out_w output i
    is texel 3i + 1 alone, its second tap 3i + 2 has weight 0 and texel 3i is not read.  (At W =
    2 out_w every weight is 1/2, so a 2x axis has no zero-weight tap; it is the other axis below.)
    A finite checker on the texels with weight, the special value on every other texel."""
    m, r = 8, 6
    yy, xx = np.mgrid[0:r, 0:m]
    checker = np.where((xx + yy) % 2 == 0, F32(0.25), F32(0.75)).astype(np.float32)
    # 3x down in both axes: only texels (3j + 1, 3i + 1) count
    img = np.full((3 * r, 3 * m, 4), special, np.float32)
    img[1::3, 1::3, :3] = checker[..., None]
    a = taps(m, 3 * m)
    assert (a[2] == 0).all() and a[0].tolist() == list(range(1, 3 * m, 3)) and a[1].tolist() == list(range(2, 3 * m, 3))
    got = resample_rgba8(img, m, r, False)
    want = quantize_rgba8(np.ascontiguousarray(img[1::3, 1::3]), False)
    assert np.array_equal(got, want)
    assert set(np.unique(got[..., :3]).tolist()) == {64, 191}
    # 2x down along x (weights 1/2 on finite texels), 3x down along y with the special value on the
    # rows of weight 0 and on the rows that are not read
    img2 = np.full((3 * r, 2 * m, 4), special, np.float32)
    img2[1::3, :, :3] = np.repeat(checker, 2, axis=1)[..., None]
    got2 = resample_rgba8(img2, m, r, False)
    clean = img2.copy()
    clean[~np.isfinite(clean)] = 0.0
    assert np.array_equal(got2, resample_rgba8(clean, m, r, False))
    assert np.array_equal(got2, want)


def test_bad_arguments():
    lib = _lib.load()
    img = np.zeros((2, 2, 4), np.float32)
    out = np.zeros((4, 4, 4), np.uint8)
    o = out.ctypes.data_as(_lib.C.c_void_p)
    p = _lib.fptr(img)
    assert lib.rt_resample_rgba8(p, 2, 2, 4, 4, 0, o) == _lib.RT_OK
    assert lib.rt_resample_rgba8(None, 2, 2, 4, 4, 0, o) == _lib.RT_E_INVAL
    assert lib.rt_resample_rgba8(p, 2, 2, 4, 4, 0, None) == _lib.RT_E_INVAL
    for bad in (0, -1, 16385):
        assert lib.rt_resample_rgba8(p, bad, 2, 4, 4, 0, o) == _lib.RT_E_INVAL
        assert lib.rt_resample_rgba8(p, 2, bad, 4, 4, 0, o) == _lib.RT_E_INVAL
        assert lib.rt_resample_rgba8(p, 2, 2, bad, 4, 0, o) == _lib.RT_E_INVAL
        assert lib.rt_resample_rgba8(p, 2, 2, 4, bad, 0, o) == _lib.RT_E_INVAL
    with pytest.raises(ValueError):
        resample_rgba8(np.zeros((2, 2, 3), np.float32), 4, 4)
    with pytest.raises(_lib.RtError):
        resample_rgba8(img, 0, 4)
    with pytest.raises(_lib.RtError):
        resample_rgba8(img, 4, 16385)


def test_the_largest_sizes_are_accepted():
    """16384 on every axis is inside the rule's 32-bit arithmetic: one row each way."""
    wide = np.zeros((1, 16384, 4), np.float32)
    wide[0, :, 1] = np.linspace(0.0, 1.0, 16384, dtype=np.float32)
    assert np.array_equal(resample_rgba8(wide, 16384, 1, False), quantize_rgba8(wide, False))
    got = resample_rgba8(wide, 16383, 1, False)
    assert np.array_equal(got, resample_ref(wide, 16383, 1, False))
    tall = np.ascontiguousarray(wide.transpose(1, 0, 2))
    assert np.array_equal(resample_rgba8(tall, 1, 16383, False), resample_ref(tall, 1, 16383, False))
    one = np.full((1, 1, 4), F32(0.5), np.float32)
    assert (resample_rgba8(one, 16384, 1, False)[..., :3] == 128).all()


EDGE_CASES = [(1, 1, 5, 3), (7, 5, 1, 1), (3, 2, 16, 16), (5, 1, 1, 7)]  # W, R, out_w, out_h


def edge_image(W, R):
    """tests/native/present_scaled_edges.cpp's fill: float k of the image is ((37 k + 11) % 257 - 1) / 255
    in float32, +inf where k % 13 == 5, NaN where k % 17 == 3."""
    k = np.arange(R * W * 4)
    v = ((37 * k + 11) % 257 - 1).astype(np.float32) / F32(255.0)
    v[k % 13 == 5] = np.inf
    v[k % 17 == 3] = np.nan
    return v.reshape(R, W, 4)


def test_edges_under_the_host_sanitizers(tmp_path):
    """rt_host.cpp and a stand-alone program (tests/native/present_scaled_edges.cpp) built with ASan,
    UBSan and the float-cast-overflow check, run as a child process: exactly sized heap buffers at
    the sizes where the clamped taps touch the image's first and last texels.  Exit 0, nothing on
    stderr, and the bytes this build's library gives.  Host code on the CPU only."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no C++ compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    p = subprocess.run([cxx, *SAN_FLAGS, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if p.returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip(f"{cxx} cannot link a sanitizer runtime that starts here")
    exe = tmp_path / "present_scaled_edges"
    p = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", *SAN_FLAGS, f"-I{ROOT / 'include'}",
                        str(ROOT / "tests" / "native" / "present_scaled_edges.cpp"),
                        str(ROOT / "real_time_ray_tracer_amd" / "csrc" / "rt_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, f"exit {p.returncode}\n{p.stdout}\n{p.stderr}"
    assert p.stderr == ""
    lines = p.stdout.strip().split("\n")
    assert len(lines) == 2 * len(EDGE_CASES)
    n = 0
    for W, R, ow, oh in EDGE_CASES:
        img = edge_image(W, R)
        assert W * R < 5 or (np.isnan(img).any() and np.isinf(img).any())
        for top_down in (False, True):
            head, _, body = lines[n].partition(":")
            assert head.split() == [str(x) for x in (W, R, ow, oh, int(top_down))]
            got = np.array([int(x, 16) for x in body.split()], np.uint8).reshape(oh, ow, 4)
            assert np.array_equal(got, resample_rgba8(img, ow, oh, top_down)), lines[n]
            assert np.array_equal(got, resample_ref(img, ow, oh, top_down)), lines[n]
            n += 1
