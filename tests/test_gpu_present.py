"""8-bit display output on the GPU (rt_present and the rt_group_*rgba8 entry points): the blit of
src/main.cpp:783-797 (resources/shader_fragment.glsl:9-19: colour unchanged, alpha 1) as a
gfx950 kernel.

Every case is bytes-exact against quantize_rgba8 (rt_quantize_rgba8, the host specification that
tests/test_present_cpu.py checks against numpy) of the float image the same context holds: both
sides start from the GPU's own floats, so no tolerance applies anywhere."""
import numpy as np
import pytest

from present_values import value_set
from real_time_ray_tracer_amd import Header, Renderer, RtError, StripGroup, aspect_for, quantize_rgba8

pytestmark = pytest.mark.gpu

FILL = 0xA5
PAD = 256  # bytes of the output tensor on either side of the bound window (a multiple of 16)


def devices(g: int) -> list[int]:
    import torch

    n = max(1, torch.cuda.device_count())
    return [i % n for i in range(g)]


@pytest.fixture(scope="module")
def shuffled():
    """The CPU test's value set (steps and neighbours, k/255, specials, random floats), shuffled."""
    v = value_set()
    return v[np.random.default_rng(11).permutation(v.size)]


def image_tensor(vals, R, W, start=0):
    """[R][W][4] float32 on the device, the values tiled from `start` on (alpha included)."""
    import torch

    n = R * W * 4
    host = np.resize(np.roll(vals, -start), n).reshape(R, W, 4)
    return torch.from_numpy(host.copy()).cuda()


def present_into_window(r: Renderer, top_down: bool, offset: int = 0):
    """r.present() into the middle of a larger uint8 tensor filled with 0xA5 -> (window, outside)."""
    import torch

    n = r.R * r.W * 4
    big = torch.full((PAD + n + PAD,), FILL, dtype=torch.uint8, device="cuda")
    assert big.data_ptr() % 16 == 0
    torch.cuda.synchronize()  # the tensors are filled on torch's stream, the context has its own
    r.bind_present(big.data_ptr() + PAD + offset)
    r.present(top_down)
    r.synchronize()
    assert r.present_device_ptr() == big.data_ptr() + PAD + offset
    host = big.cpu().numpy()
    lo, hi = PAD + offset, PAD + offset + n
    return host[lo:hi].reshape(r.R, r.W, 4), np.concatenate([host[:lo], host[hi:]])


def check_kernel_alone(vals, W, R, top_down, offset=0, start=0):
    img = image_tensor(vals, R, W, start)
    with Renderer(W, R, 1, 1) as r:  # no header is uploaded and nothing is rendered
        r.bind_image(img.data_ptr())
        got, outside = present_into_window(r, top_down, offset)
        held = r.image()
    assert np.array_equal(held.view(np.uint32), img.cpu().numpy().view(np.uint32))
    want = quantize_rgba8(held, top_down)
    assert (outside == FILL).all(), f"{int((outside != FILL).sum())} bytes outside the window changed"
    bad = np.argwhere(got != want)
    assert bad.size == 0, (f"{len(bad)} bytes differ; first at {tuple(bad[0])}: got {got[tuple(bad[0])]}, "
                           f"want {want[tuple(bad[0])]}")
    assert (got[..., 3] == 255).all()


@pytest.mark.parametrize("top_down", [False, True])
@pytest.mark.parametrize("R", [1, 2, 5])
@pytest.mark.parametrize("W", [1, 3, 4, 5, 64, 67, 256, 260])
def test_kernel_alone(shuffled, W, R, top_down):
    """Both paths (W % 4 == 0: four pixels and one 16-byte store per lane; else one pixel per lane),
    the row tail, the last partial workgroup (W = 260: 65 lanes of the second block's 256; W = 67)
    and the flip; every byte inside the window written, none outside."""
    check_kernel_alone(shuffled, W, R, top_down, start=(W * 131 + R * 17) % shuffled.size)


@pytest.mark.parametrize("top_down", [False, True])
def test_kernel_alone_misaligned_output(shuffled, top_down):
    """W = 256 again with the output 4 bytes off a 16-byte boundary: the one-pixel path."""
    check_kernel_alone(shuffled, 256, 5, top_down, offset=4)


@pytest.mark.parametrize("W", [256, 257])
def test_kernel_converts_the_whole_value_set(shuffled, W):
    """Every float of the CPU test's set through each path (R * W * 4 >= the set's size)."""
    R = 100
    assert R * W * 4 >= shuffled.size
    check_kernel_alone(shuffled, W, R, True)


@pytest.mark.parametrize("top_down", [False, True])
def test_strip_context(shuffled, top_down):
    """A strip context converts its own rows and flips within the strip: rows [11, 29) of a 67x40
    frame equal the matching rows of the whole frame's conversion of the same image contents."""
    import torch

    W, H, r0, r1 = 67, 40, 11, 29
    img = image_tensor(shuffled, H, W)
    torch.cuda.synchronize()
    with Renderer(W, H, 1, 1) as whole, Renderer(W, H, 1, 1, rows=(r0, r1)) as strip:
        whole.bind_image(img.data_ptr())
        strip.bind_image(img.data_ptr() + r0 * W * 16)
        full = whole.image8(top_down)
        got = strip.image8(top_down)
        assert got.shape == (r1 - r0, W, 4)
        assert np.array_equal(got, quantize_rgba8(strip.image(), top_down))
    want = full[H - r1:H - r0] if top_down else full[r0:r1]
    assert np.array_equal(got, want)


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_after_real_frames(mode):
    W, H, spp = 64, 48, 4
    h = Header.builtin(1, spp, aspect_for(W, H))
    with Renderer(W, H, h.S, h.AA) as r:
        assert r.present_device_ptr() == 0
        r.compute_frames(h, mode, 0, 3)
        for top_down in (True, False):
            got = r.image8(top_down)
            assert np.array_equal(got, quantize_rgba8(r.image(), top_down)), f"mode {mode} top_down {top_down}"
        assert r.present_device_ptr() != 0
        assert len(np.unique(got[..., :3])) > 8  # not a blank frame


def advance(r: Renderer, h: Header, mode: int, frame: int, k: int) -> int:
    """One frame of the render loop (src/main.cpp:763-781, 553-578) in `mode`."""
    if mode in (1, 2):
        h.fill_rand_buffer(7000 + k)
    else:
        h.moving_light(True)
    h.set_mode(frame, h.num_objects)
    r.upload_header(h)
    return r.dispatch(mode, frame)


@pytest.mark.parametrize("modes", [[1] * 10, [1, 3] * 5], ids=["mode1", "modes1and3"])
def test_ordering_under_pipelining(modes):
    """Ten pipelined frames, each followed by a present into its own slot with nothing synchronising
    in between: a present reads its frame's image after the pass that wrote it (the output stream for
    a pipelined mode-1 frame, the main stream for mode 3) and before the next frame overwrites it."""
    import torch

    W, H, spp = 640, 480, 4
    h0 = Header.synthetic(24, spp, 1234, aspect_for(W, H))
    want = []
    with Renderer(W, H, h0.S, h0.AA) as seq:
        h, f = h0.copy(), 0
        for k, mode in enumerate(modes):
            f = advance(seq, h, mode, f, k)
            want.append(quantize_rgba8(seq.image(), True))
    assert any(not np.array_equal(want[k], want[k + 1]) for k in range(len(modes) - 1))
    slots = torch.zeros((len(modes), H, W, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with Renderer(W, H, h0.S, h0.AA) as r:
        r.enable_pipelining(True)
        h, f = h0.copy(), 0
        for k, mode in enumerate(modes):
            f = advance(r, h, mode, f, k)
            r.bind_present(slots[k].data_ptr())
            r.present(True)
        r.synchronize()
        got = slots.cpu().numpy()
    for k in range(len(modes)):
        assert np.array_equal(got[k], want[k]), f"slot {k} (mode {modes[k]}) is not frame {k}"


@pytest.mark.parametrize("enable_first", [False, True], ids=["plan-then-enable", "enable-then-plan"])
@pytest.mark.parametrize("top_down", [False, True])
def test_group_on_one_gpu(top_down, enable_first):
    """Three strips with the copy path forced and the root in the middle: strip 1 presents straight
    into its rows of the 8-bit frame, strips 0 and 2 copy their 8-bit strips; re-planning after
    enabling rebinds the rows."""
    W, H, spp = 200, 150, 4
    h0 = Header.synthetic(24, spp, 99, aspect_for(W, H))
    with Renderer(W, H, h0.S, h0.AA) as whole, StripGroup(W, H, h0.S, h0.AA, devices(3)) as g:
        g.enable_pipelining(True)
        if enable_first:
            g.enable_rgba8(True, top_down)
        g.force_copies(True)
        g.set_plan([0, 37, 101, 150], 1)
        if not enable_first:
            g.enable_rgba8(True, top_down)
        assert [g.strip_copies(i) for i in range(3)] == [True, False, True]
        assert g.rgba8_device_ptr() != 0
        hw, hg = h0.copy(), h0.copy()
        fw = fg = 0
        for mode, n in ((1, 10), (3, 3)):
            fw = whole.compute_frames(hw, mode, fw, n)
            fg = g.compute_frames(hg, mode, fg, n)
            assert fw == fg
            want = quantize_rgba8(whole.image(), top_down)
            got = g.image8()
            assert np.array_equal(got, want), f"mode {mode}: {int((got != want).sum())} bytes differ"
            with pytest.raises(RtError):
                g.image()
        assert len(np.unique(got[..., :3])) > 8
        g.enable_rgba8(False)
        assert g.rgba8_device_ptr() == 0
        with pytest.raises(RtError):
            g.image8()
        fw = whole.compute_frames(hw, 1, fw, 1)
        fg = g.compute_frames(hg, 1, fg, 1)
        assert np.array_equal(g.image().view(np.uint32), whole.image().view(np.uint32))


def test_errors():
    r = Renderer(16, 8, 1, 1)
    assert r.present_device_ptr() == 0
    with pytest.raises(RtError):
        r._c(r._lib.rt_download_rgba8(r.ctx, 1, None), "rt_download_rgba8(NULL)")
    with pytest.raises(RtError):
        r.bind_present(2)  # not a whole pixel's alignment
    assert r.present_device_ptr() == 0  # nothing was presented
    r.present()
    assert r.present_device_ptr() != 0
    assert r.image8().shape == (8, 16, 4)
    r.close()
    with pytest.raises(RtError):
        r.present()
    with pytest.raises(RtError):
        r.image8()
    with pytest.raises(RtError):
        r.bind_present(None)
    assert r._lib.rt_present_device_ptr(None) is None
    assert r._lib.rt_group_download_rgba8(None, None) < 0
    assert r._lib.rt_group_enable_rgba8(None, 1, 1) < 0
    assert r._lib.rt_group_rgba8_device_ptr(None) is None
