"""rt_quantize_rgba8 (rt_host.cpp): the blit's 8-bit conversion (src/main.cpp:783-797,
resources/shader_fragment.glsl:9-19) on the host, the specification the device kernel of
rt_present is compared with byte for byte (tests/test_gpu_present.py).  No GPU.

Here it is compared with a numpy restatement of the rule (tests/present_values.py): NaN -> 0,
v <= 0 -> 0, v >= 1 -> 255, else float32 v * 255 + 0.5 truncated; alpha 255."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from present_values import (SPECIAL_BITS, as_image, from_bits, q_ref, quantize_ref, specials, steps,
                            value_set)
from real_time_ray_tracer_amd import _lib, quantize_rgba8


def channels(vals) -> np.ndarray:
    """quantize_rgba8 of the values (three to a pixel), one byte per value."""
    vals = np.asarray(vals, np.float32)
    return quantize_rgba8(as_image(vals), top_down=False)[0, :, :3].reshape(-1)[:vals.size]


def test_the_rule_has_255_steps_at_the_stated_floats():
    s = steps()
    assert len(np.unique(s)) == 255
    assert s[0] == 0x3B008080 and s[-1] == 0x3F7F7F7F
    # each is a step of the restatement: k at the float, k - 1 just below it
    assert np.array_equal(q_ref(from_bits(s)), np.arange(1, 256))
    assert np.array_equal(q_ref(from_bits(s - np.uint32(1))), np.arange(0, 255))


def test_steps_and_their_neighbours():
    s = steps().astype(np.int64)
    near = from_bits((s[:, None] + np.arange(-2, 3)[None, :]).reshape(-1).astype(np.uint32))
    got = channels(near)
    assert np.array_equal(got, q_ref(near))
    assert np.array_equal(got.reshape(255, 5)[:, 2], np.arange(1, 256))
    assert np.array_equal(got.reshape(255, 5)[:, 1], np.arange(0, 255))


def test_k_over_255_gives_k():
    exact = (np.arange(256) / 255.0).astype(np.float32)
    got = channels(exact)
    assert np.array_equal(got, np.arange(256))
    assert np.array_equal(got, q_ref(exact))


def test_specials():
    v = specials()
    assert v.size == SPECIAL_BITS.size + 2 and np.isnan(v).sum() == 4
    got = channels(v)
    assert np.array_equal(got, q_ref(v))
    want = [0, 0, 0, 0, 0, 0, 255, 0, 0, 0, 0, 0, 255, 255, 255, 0, 255]  # the rule, by hand
    assert got.tolist() == want


def test_random_floats():
    rnd = value_set()[-100_000:]
    assert rnd.min() >= -0.5 and rnd.max() < 1.5 and (rnd < 0).any() and (rnd > 1).any()
    assert np.array_equal(channels(rnd), q_ref(rnd))


@pytest.mark.parametrize("w", [0.0, float("nan"), 7.0])
def test_alpha_is_255_whatever_w_is(w):
    vals = value_set()[:3000]
    out = quantize_rgba8(as_image(vals, w=w), top_down=False)
    assert (out[..., 3] == 255).all()
    assert np.array_equal(out, quantize_ref(as_image(vals, w=w), False))


@pytest.mark.parametrize("R,W", [(1, 1), (1, 5), (3, 1), (7, 5)])
def test_top_down_is_the_rows_reversed(R, W):
    img = np.resize(value_set()[::97], R * W * 4).reshape(R, W, 4).astype(np.float32)
    up = quantize_rgba8(img, top_down=False)
    down = quantize_rgba8(img, top_down=True)
    assert up.shape == (R, W, 4) and up.dtype == np.uint8
    assert np.array_equal(down, up[::-1])
    assert np.array_equal(up, quantize_ref(img, False)) and np.array_equal(down, quantize_ref(img, True))


def test_equals_the_clip_formula_on_every_non_nan_input():
    """clip(v, 0, 1) * 255 + 0.5 floored, as tests/test_gpu_image.py states the PPM's bytes."""
    v = value_set()
    v = v[~np.isnan(v)]
    c = np.clip(v, np.float32(0.0), np.float32(1.0)).astype(np.float32)
    want = np.floor(c * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)
    assert np.array_equal(channels(v), want)


def test_bad_arguments():
    lib = _lib.load()
    img = np.zeros((2, 2, 4), np.float32)
    out = np.zeros((2, 2, 4), np.uint8)
    o = out.ctypes.data_as(_lib.C.c_void_p)
    assert lib.rt_quantize_rgba8(None, 2, 2, 0, o) == _lib.RT_E_INVAL
    assert lib.rt_quantize_rgba8(_lib.fptr(img), 2, 2, 0, None) == _lib.RT_E_INVAL
    assert lib.rt_quantize_rgba8(_lib.fptr(img), 0, 2, 0, o) == _lib.RT_E_INVAL
    assert lib.rt_quantize_rgba8(_lib.fptr(img), 2, -1, 0, o) == _lib.RT_E_INVAL
    with pytest.raises(ValueError):
        quantize_rgba8(np.zeros((2, 2, 3), np.float32))


SAN_FLAGS = ["-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def test_specials_under_the_host_sanitizers(tmp_path):
    """rt_host.cpp and a stand-alone program (tests/native/present_specials.cpp) built with ASan,
    UBSan and the float-cast-overflow check, run as a child process on the specials (the NaNs, the
    infinities and 1e30 are the floats whose cast to an integer type would be undefined): exit 0 and
    the restatement's bytes.  Host code on the CPU only."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no C++ compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    p = subprocess.run([cxx, *SAN_FLAGS, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if p.returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip(f"{cxx} cannot link a sanitizer runtime that starts here")
    exe = tmp_path / "present_specials"
    p = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", *SAN_FLAGS, f"-I{ROOT / 'include'}",
                        str(ROOT / "tests" / "native" / "present_specials.cpp"),
                        str(ROOT / "real_time_ray_tracer_amd" / "csrc" / "rt_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    v = np.concatenate([specials(), np.float32([0.5, 0.25, 0.999])])
    bits = [hex(int(b)) for b in v.view(np.uint32)]
    p = subprocess.run([str(exe), *bits], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, f"exit {p.returncode}\n{p.stdout}\n{p.stderr}"
    assert p.stderr == ""
    got = [int(x, 16) for x in p.stdout.split()]
    assert got == q_ref(v).tolist()
