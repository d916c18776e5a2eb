"""8-bit display output at window size on the GPU (rt_present_scaled, rt_download_rgba8_scaled,
rt_group_download_rgba8_scaled): the blit of src/main.cpp:783-797 into a framebuffer of any size, the
image sampled with GL_LINEAR and GL_CLAMP_TO_EDGE (381-388), as a gfx950 kernel.

Every case is bytes-exact against resample_rgba8 (rt_resample_rgba8, the host specification that
tests/test_present_scaled_cpu.py checks against numpy) of the float image the same context holds:
both sides start from the GPU's own floats, so no tolerance applies anywhere."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from present_values import specials, value_set
from real_time_ray_tracer_amd import (Header, Renderer, RtError, StripGroup, aspect_for, quantize_rgba8,
                                      resample_rgba8)
from test_gpu_present import FILL, PAD, advance, devices, image_tensor

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shuffled():
    """The 8-bit conversion's value set shuffled, behind its specials (NaN, infinities, subnormals),
    so that images of a few pixels hold them too."""
    v = value_set()
    return np.concatenate([specials(), v[np.random.default_rng(13).permutation(v.size)]])


def differing(got, want) -> str:
    bad = np.argwhere(got != want)
    if bad.size == 0:
        return ""
    return f"{len(bad)} bytes differ; first at {tuple(bad[0])}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"


def check_kernel_alone(vals, W, R, ow, oh, top_down, offset=0, start=0):
    """A value-set image bound as the context's image, the output bound into the middle of a larger
    tensor of 0xA5: every byte of the window right, every byte outside it unchanged."""
    import torch

    img = image_tensor(vals, R, W, start)
    n = oh * ow * 4
    big = torch.full((PAD + n + PAD,), FILL, dtype=torch.uint8, device="cuda")
    assert big.data_ptr() % 16 == 0
    torch.cuda.synchronize()  # the tensors are filled on torch's stream, the context has its own
    with Renderer(W, R, 1, 1) as r:  # no header is uploaded and nothing is rendered
        r.bind_image(img.data_ptr())
        r.bind_present_scaled(big.data_ptr() + PAD + offset)
        r.present_scaled(ow, oh, top_down)
        r.synchronize()
        assert r.present_scaled_device_ptr() == big.data_ptr() + PAD + offset
        assert r.present_scaled_size() == (ow, oh)
        assert r.present_device_ptr() == 0  # the 1:1 present's buffer is not touched
        held = r.image()
    host = big.cpu().numpy()
    lo, hi = PAD + offset, PAD + offset + n
    got, outside = host[lo:hi].reshape(oh, ow, 4), np.concatenate([host[:lo], host[hi:]])
    assert np.array_equal(held.view(np.uint32), img.cpu().numpy().view(np.uint32))
    want = resample_rgba8(held, ow, oh, top_down)
    assert (outside == FILL).all(), f"{int((outside != FILL).sum())} bytes outside the window changed"
    assert not differing(got, want), differing(got, want)
    assert (got[..., 3] == 255).all()


@pytest.mark.parametrize("top_down", [False, True])
@pytest.mark.parametrize("oh", [1, 2, 5])
@pytest.mark.parametrize("ow", [1, 3, 4, 5, 64, 67, 256, 260])
@pytest.mark.parametrize("W,R", [(1, 1), (3, 2), (67, 5), (64, 48)])
def test_kernel_alone(shuffled, W, R, ow, oh, top_down):
    """Both store paths (ow % 4 == 0: four pixels and one 16-byte store per lane; else one pixel per
    lane), the row tail, the last partial workgroup (ow = 260: 65 lanes of the second block's 256),
    scaling up and down along each axis, the equal-size axis (all weights 0) and the clamped edge
    taps; every byte inside the window written, none outside."""
    check_kernel_alone(shuffled, W, R, ow, oh, top_down, start=(W * 131 + ow * 17 + oh) % shuffled.size)


@pytest.mark.parametrize("top_down", [False, True])
def test_kernel_alone_misaligned_output(shuffled, top_down):
    """ow = 256 again with the output 4 bytes off a 16-byte boundary: the one-pixel path."""
    check_kernel_alone(shuffled, 67, 5, 256, 5, top_down, offset=4)


def test_lanes_walk_several_rows(shuffled):
    """More output rows than the launch has rows of workgroups (about 512 workgroups in all: 256
    rows of them at two blocks along x, 512 at one), so every lane's row loop runs more than once:
    the wide path, the one-pixel path, and a tall source scaled down."""
    check_kernel_alone(shuffled, 64, 48, 1028, 1100, True)
    check_kernel_alone(shuffled, 67, 5, 260, 1100, False)
    check_kernel_alone(shuffled, 8, 3000, 4, 1100, True)


@pytest.mark.parametrize("top_down", [False, True])
@pytest.mark.parametrize("W,R", [(256, 100), (257, 100)])
def test_identity_is_the_1_to_1_present(shuffled, W, R, top_down):
    """Equal sizes: the whole value set (NaN and infinite neighbours under zero weights) gives the 1:1
    present's bytes."""
    import torch

    assert R * W * 4 >= shuffled.size
    img = image_tensor(shuffled, R, W)
    torch.cuda.synchronize()
    with Renderer(W, R, 1, 1) as r:
        r.bind_image(img.data_ptr())
        got = r.image8_scaled(W, R, top_down)
        assert np.array_equal(got, r.image8(top_down))
        assert np.array_equal(got, quantize_rgba8(r.image(), top_down))


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_after_real_frames(mode):
    W, H, spp = 64, 48, 4
    h = Header.builtin(1, spp, aspect_for(W, H))
    with Renderer(W, H, h.S, h.AA) as r:
        assert r.present_scaled_device_ptr() == 0
        r.compute_frames(h, mode, 0, 3)
        for ow, oh in ((200, 150), (21, 16)):
            for top_down in (True, False):
                got = r.image8_scaled(ow, oh, top_down)
                want = resample_rgba8(r.image(), ow, oh, top_down)
                assert not differing(got, want), f"mode {mode} {ow}x{oh} top_down {top_down}: {differing(got, want)}"
            assert len(np.unique(got[..., :3])) > 8  # not a blank frame
        assert r.present_scaled_device_ptr() != 0 and r.present_scaled_size() == (21, 16)


@pytest.mark.parametrize("modes", [[1] * 10, [1, 3] * 5], ids=["mode1", "modes1and3"])
def test_ordering_under_pipelining(modes):
    """Ten pipelined frames, each followed by a scaled present into its own slot with nothing
    synchronising in between: it reads its frame's image after the pass that wrote it (the output
    stream for a pipelined mode-1 frame, the main stream for mode 3) and before the next frame
    overwrites it."""
    import torch

    W, H, spp, ow, oh = 640, 480, 4, 320, 200
    h0 = Header.synthetic(24, spp, 1234, aspect_for(W, H))
    want = []
    with Renderer(W, H, h0.S, h0.AA) as seq:
        h, f = h0.copy(), 0
        for k, mode in enumerate(modes):
            f = advance(seq, h, mode, f, k)
            want.append(resample_rgba8(seq.image(), ow, oh, True))
    assert any(not np.array_equal(want[k], want[k + 1]) for k in range(len(modes) - 1))
    slots = torch.zeros((len(modes), oh, ow, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with Renderer(W, H, h0.S, h0.AA) as r:
        r.enable_pipelining(True)
        h, f = h0.copy(), 0
        for k, mode in enumerate(modes):
            f = advance(r, h, mode, f, k)
            r.bind_present_scaled(slots[k].data_ptr())
            r.present_scaled(ow, oh, True)
        r.synchronize()
        got = slots.cpu().numpy()
    for k in range(len(modes)):
        assert np.array_equal(got[k], want[k]), f"slot {k} (mode {modes[k]}) is not frame {k}"


def test_resize_replaces_the_own_buffer():
    """A window that grows and shrinks again, on the context's own buffer; the 1:1 present is unaffected."""
    W, H, spp = 64, 48, 4
    h = Header.builtin(1, spp, aspect_for(W, H))
    with Renderer(W, H, h.S, h.AA) as r:
        r.compute_frames(h, 3, 0, 2)
        img = r.image()
        for ow, oh in ((100, 75), (300, 200), (100, 75)):
            got = r.image8_scaled(ow, oh)
            assert not differing(got, resample_rgba8(img, ow, oh)), f"{ow}x{oh}"
            assert r.present_scaled_device_ptr() != 0 and r.present_scaled_size() == (ow, oh)
        # enqueued presents into the buffer a larger one then replaces: nothing synchronises before it
        r.present_scaled(310, 200)
        r.present_scaled(400, 300)
        r.synchronize()
        assert r.present_scaled_size() == (400, 300)
        assert np.array_equal(r.image8(), quantize_rgba8(img))
        assert r.present_device_ptr() != 0 and r.present_device_ptr() != r.present_scaled_device_ptr()
        assert np.array_equal(r.image().view(np.uint32), img.view(np.uint32))


def test_strip_context_is_refused():
    """A strip does not hold the rows its edge output rows filter from: an error, not a wrong seam."""
    with Renderer(67, 40, 1, 1, rows=(11, 29)) as strip:
        with pytest.raises(RtError) as e:
            strip.present_scaled(67, 18)
        assert e.value.status == -5  # RT_E_STATE
        with pytest.raises(RtError):
            strip.image8_scaled(67, 18)
        with pytest.raises(RtError):
            strip.bind_present_scaled(None)
        with pytest.raises(RtError):
            strip.present_scaled_size()
        assert strip.present_scaled_device_ptr() == 0
        assert strip.image8().shape == (18, 67, 4)  # the 1:1 present of a strip works as before


def test_group_on_one_gpu():
    """Three strips with the copy path forced and the root in the middle: the assembled float frame
    through the scaled blit equals the whole-frame context's; refused while 8-bit strips are on."""
    W, H, spp = 200, 150, 4
    h0 = Header.synthetic(24, spp, 99, aspect_for(W, H))
    with Renderer(W, H, h0.S, h0.AA) as whole, StripGroup(W, H, h0.S, h0.AA, devices(3)) as g:
        g.enable_pipelining(True)
        g.force_copies(True)
        g.set_plan([0, 37, 101, 150], 1)
        hw, hg = h0.copy(), h0.copy()
        fw = fg = 0
        for mode, n in ((1, 4), (3, 3)):
            fw = whole.compute_frames(hw, mode, fw, n)
            fg = g.compute_frames(hg, mode, fg, n)
            assert fw == fg
            for top_down in (True, False):
                got = g.image8_scaled(320, 240, top_down)
                want = resample_rgba8(whole.image(), 320, 240, top_down)
                assert not differing(got, want), f"mode {mode} top_down {top_down}: {differing(got, want)}"
        assert len(np.unique(got[..., :3])) > 8
        assert not differing(g.image8_scaled(50, 30), resample_rgba8(whole.image(), 50, 30))  # scratch reused
        assert not differing(g.image8_scaled(640, 400), resample_rgba8(whole.image(), 640, 400))  # and regrown
        g.enable_rgba8(True)
        with pytest.raises(RtError) as e:
            g.image8_scaled(320, 240)
        assert e.value.status == -5  # RT_E_STATE: the float frame is not assembled
        g.enable_rgba8(False)
        fw = whole.compute_frames(hw, 1, fw, 1)
        fg = g.compute_frames(hg, 1, fg, 1)
        assert not differing(g.image8_scaled(320, 240), resample_rgba8(whole.image(), 320, 240))


@pytest.mark.parametrize("strips,mode", [(1, 1), (3, 3)])
def test_headless_ppm_size(tmp_path, strips, mode):
    """rt_headless --ppm-size 1920x1080 on its default 440x330 scene (the reference's own screenshot
    case): the PPM is the float image of the same frames through resample_rgba8, top row first; with
    --strips the group's on-demand call over the assembled float frame."""
    exe = ROOT / "build" / "rt_headless"
    if not exe.exists():
        subprocess.run(["make", "-C", str(ROOT), "headless"], check=True, capture_output=True)
    W, H, spp, frames, ow, oh = 440, 330, 4, 8, 1920, 1080
    out = tmp_path / "frame.ppm"
    p = subprocess.run([str(exe), "--mode", str(mode), "--strips", str(strips), "--ppm", str(out), "--ppm-size",
                        f"{ow}x{oh}"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    data = out.read_bytes()
    head = f"P6\n{ow} {oh}\n255\n".encode()
    assert data.startswith(head) and len(data) == len(head) + ow * oh * 3
    got = np.frombuffer(data[len(head):], np.uint8).reshape(oh, ow, 3)
    h = Header.builtin(1, spp, aspect_for(W, H))
    with Renderer(W, H, h.S, h.AA) as r:
        f = 0
        for k in range(frames):  # rt_headless's loop (src/main.cpp:553-578 per frame)
            if mode in (1, 2):
                h.fill_rand_buffer(7000 + k)
            else:
                h.moving_light(False)
            h.set_mode(f, h.num_objects)
            r.upload_header(h)
            f = r.dispatch(mode, f)
        want = resample_rgba8(r.image(), ow, oh, True)[..., :3]
    assert not differing(got, want), differing(got, want)
    assert len(np.unique(got)) > 8  # not a blank frame
    p = subprocess.run([str(exe), "--ppm", str(out), "--ppm-size", "1920"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "--ppm-size" in p.stderr


def test_errors():
    r = Renderer(16, 8, 1, 1)
    assert r.present_scaled_device_ptr() == 0
    with pytest.raises(RtError):
        r.present_scaled_size()  # nothing was presented
    for bad in (0, -1, 16385):
        with pytest.raises(RtError):
            r.present_scaled(bad, 8)
        with pytest.raises(RtError):
            r.present_scaled(16, bad)
        with pytest.raises(RtError):
            r.image8_scaled(bad, 8)
    with pytest.raises(RtError):
        r._c(r._lib.rt_download_rgba8_scaled(r.ctx, 16, 8, 1, None), "rt_download_rgba8_scaled(NULL)")
    with pytest.raises(RtError):
        r.bind_present_scaled(2)  # not a whole pixel's alignment
    assert r.present_scaled_device_ptr() == 0  # nothing was presented
    r.present_scaled(32, 4)
    assert r.present_scaled_device_ptr() != 0 and r.present_scaled_size() == (32, 4)
    assert r.image8_scaled(5, 3).shape == (3, 5, 4)
    r.close()
    with pytest.raises(RtError):
        r.present_scaled(16, 8)
    with pytest.raises(RtError):
        r.image8_scaled(16, 8)
    with pytest.raises(RtError):
        r.bind_present_scaled(None)
    with pytest.raises(RtError):
        r.present_scaled_size()
    out = np.zeros((8, 16, 4), np.uint8)
    assert r._lib.rt_present_scaled_device_ptr(None) is None
    assert r._lib.rt_group_download_rgba8_scaled(None, 16, 8, 1, out.ctypes.data_as(C.c_void_p)) < 0
    assert r._lib.rt_group_download_rgba8_scaled(None, 16, 8, 1, None) < 0


def test_group_errors():
    with StripGroup(16, 8, 1, 1, devices(2)) as g:
        out = np.zeros((8, 16, 4), np.uint8)
        o = out.ctypes.data_as(C.c_void_p)
        assert g._lib.rt_group_download_rgba8_scaled(g.g, 16, 8, 1, None) == -1
        for bad in (0, -1, 16385):
            assert g._lib.rt_group_download_rgba8_scaled(g.g, bad, 8, 1, o) == -1
            assert g._lib.rt_group_download_rgba8_scaled(g.g, 16, bad, 1, o) == -1
        assert g.image8_scaled(16, 8).shape == (8, 16, 4)
