"""FreeU on the GPU (csrc/freeu.hip): the launch against diffusers' fourier_filter written with torch.fft in float64, its
exact cases, and a tiny fused W8A8 UNet with enable_freeu -- all-ones, a graph replay, new values under a captured graph."""
import pytest
import torch

from tests.test_freeu_host import reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SETTINGS = ((0.9, 1.5), (0.2, 1.6), (0.6, 1.1), (0.4, 1.2), (0.0, 1.4))   # (s, b): diffusers' published ones, and s = 0
cl = torch.channels_last


def _pair(shape, seed):
    """Random with a DC offset (mean about 0.7): the low frequencies are not noise."""
    B, C_s, C_h, H, W = shape
    g = torch.Generator().manual_seed(seed)
    skip = (torch.randn(B, C_s, H, W, generator=g) * 0.5 + 0.7).half()
    hidden = (torch.randn(B, C_h, H, W, generator=g) * 0.5 + 0.7).half()
    return hidden.to(DEV).contiguous(memory_format=cl), skip.to(DEV).contiguous(memory_format=cl)


def _ratio(got_h, got_s, hidden, skip, b, s):
    """Largest error / bound over the pair.  The bound, per element of the skip, with m = the plane's mean |x|, n = H W:

        2^-11 |y_ref|  +  2^-25  +  |s - 1| * m * 7 * (ceil(n / 256) + 32) * 2^-24

    the one rounding to FP16 (half an ulp, or half the subnormal step), and the FP32 error of the correction, from the
    kernel's summation order (include/mixdq_math.h): a sum S_t is a chain of ceil(n / 256) FMAs in a lane, 6 additions
    across the wave and 3 across the waves, over terms of total size <= n m -- (ceil(n / 256) + 9) u n m with u = 2^-24;
    a basis value is off by <= 3 u (table entries rounded once, the product frequency two products and an FMA), in the
    sums and again in the correction: 6 u; g = (s - 1) / n and g S_t round twice: 2 u; seven such terms, each |g S_t w_t|
    <= |s - 1| m, then seven FMAs on partial sums <= 7 |s - 1| m: 7 u each.  Together 7 (ceil(n / 256) + 24) u |s - 1| m;
    the 8 more stand for the FP32 addition x + correction in front of the rounding.  The hidden is the float64 product
    rounded to FP32, then to FP16: (2^-11 + 2^-24) |h b| + 2^-25."""
    ref_h, ref_s = reference(hidden.cpu(), skip.cpu(), b, s)
    n = skip.shape[2] * skip.shape[3]
    m = skip.cpu().double().abs().mean(dim=(2, 3), keepdim=True)
    bound_s = 2.0 ** -11 * ref_s.abs() + 2.0 ** -25 + abs(s - 1.0) * m * 7 * (-(-n // 256) + 32) * 2.0 ** -24
    bound_h = (2.0 ** -11 + 2.0 ** -24) * ref_h.abs() + 2.0 ** -25
    r_s = ((got_s.cpu().double() - ref_s).abs() / bound_s).max().item()
    r_h = ((got_h.cpu().double() - ref_h).abs() / bound_h).max().item()
    return r_s, r_h


def _check(C, shape, seed=0):
    hidden, skip = _pair(shape, seed)
    for s, b in SETTINGS:
        table = torch.tensor([[7.0, 7.0], [b, s]], device=DEV)                     # (stage 1 is read, not stage 0)
        got_h, got_s = C.freeu(hidden, skip, table, 1)
        assert got_s.is_contiguous(memory_format=cl) and got_h.is_contiguous(memory_format=cl)
        r_s, r_h = _ratio(got_h, got_s, hidden, skip, b, s)
        print(f"freeu {shape} s={s} b={b}: error / bound skip {r_s:.3f} hidden {r_h:.3f}")
        assert r_s <= 1.0 and r_h <= 1.0


@pytest.mark.parametrize("shape", ((1, 8, 16, 2, 2), (2, 16, 32, 5, 7), (1, 24, 16, 8, 8), (2, 520, 16, 4, 4)))
def test_launch_against_float64(C, shape):
    """y = s x at 2 x 2; odd, non-square, tail lanes; three octets; 130 workgroups: two whole XCD groups and a tail."""
    _check(C, shape)


@pytest.mark.parametrize("side", (0, 1))
@pytest.mark.parametrize("ppl", (1, 2, 4, 8, 16))
def test_launch_at_every_route_boundary(C, ppl, side):
    """The largest plane of every pixels-per-lane instantiation and the smallest of the next; behind the last one the
    route that reads the plane twice."""
    assert ppl in C.FREEU_PPL
    H, W = 16, C.FREEU_LANES * ppl // 16 + side
    assert (H * W > C.FREEU_RESIDENT_PIXELS) == (ppl == max(C.FREEU_PPL) and side == 1)
    _check(C, (1, 8, 16, H, W), seed=ppl)


def test_exact_cases(C):
    hidden, skip = _pair((2, 16, 32, 5, 7), 11)
    h0, s0 = hidden.clone(), skip.clone()
    table = torch.tensor([[1.0, 0.3], [1.7, 1.0]], device=DEV)
    got_h, got_s = C.freeu(hidden, skip, table, 0)                                  # b == 1
    assert torch.equal(got_h.view(torch.int16), h0.view(torch.int16)) and not torch.equal(got_s, s0)
    got_h, got_s = C.freeu(hidden, skip, table, 1)                                  # s == 1
    assert torch.equal(got_s.view(torch.int16), s0.view(torch.int16)) and not torch.equal(got_h, h0)
    assert torch.equal(got_h[:, 16:].view(torch.int16), h0[:, 16:].view(torch.int16))      # channels >= C_h / 2
    assert torch.equal(hidden, h0) and torch.equal(skip, s0)                       # neither input is modified
    assert got_h.data_ptr() != hidden.data_ptr() and got_s.data_ptr() != skip.data_ptr()
    with pytest.raises(RuntimeError, match="at least 2"):
        C.freeu(hidden[:, :, :1].contiguous(memory_format=cl), skip[:, :, :1].contiguous(memory_format=cl), table, 0)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        C.freeu(hidden, skip[:, :12].contiguous(memory_format=cl), table, 0)


# ---- a tiny fused W8A8 UNet (the ControlNet tests' recipe) -------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(C):
    import bench
    from mixdq_amd.quantize_sdxl import example_inputs
    from mixdq_amd.unet import build_unet
    from tests.test_control_gpu import _w8a8
    inputs = example_inputs(2, 32, DEV, seed=7)
    unet = _w8a8(build_unet(DEV, cfg=dict(bench.TINY_CFG, block_out_channels=(64, 128, 256), head_dim=64)), inputs)
    with torch.no_grad():
        plain = unet(**inputs)[0].clone()
    yield dict(unet=unet, inputs=inputs, plain=plain)
    unet.disable_freeu()
    del unet
    torch.cuda.empty_cache()


def test_all_ones_is_the_plain_forward(tiny):
    unet = tiny["unet"].enable_freeu(1, 1, 1, 1)
    with torch.no_grad():
        assert torch.equal(unet(**tiny["inputs"])[0], tiny["plain"])
    unet.disable_freeu()
    with torch.no_grad():
        assert torch.equal(unet(**tiny["inputs"])[0], tiny["plain"])


def test_graph_replay_follows_the_table(tiny):
    unet, inp = tiny["unet"].enable_freeu(0.9, 0.2, 1.5, 1.6), tiny["inputs"]
    with torch.no_grad():
        eager = unet(**inp)[0].clone()
        assert not torch.equal(eager, tiny["plain"])
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            unet(**inp)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = unet(**inp)[0]
        for _ in range(3):
            graph.replay()
            assert torch.equal(out, eager)
        unet.enable_freeu(0.6, 0.4, 1.1, 1.2)                                      # new values under the captured graph
        graph.replay()
        fresh = unet(**inp)[0]
        assert torch.equal(out, fresh) and not torch.equal(fresh, eager)
        # disable under the live graph: the table stays, the graph keeps running FreeU with the last values; eager is plain
        unet.disable_freeu()
        filler = [torch.full((2, 2), 9.0, device=DEV) for _ in range(64)]          # (would land in a freed table)
        assert torch.equal(unet(**inp)[0], tiny["plain"])
        graph.replay()
        assert torch.equal(out, fresh)
        unet.enable_freeu(0.9, 0.2, 1.5, 1.6)                                      # the same table again: the graph follows
        graph.replay()
        assert torch.equal(out, eager)
        del graph, filler


def test_up_block_hook_against_float64(tiny):
    unet = tiny["unet"].enable_freeu(0.9, 0.2, 1.5, 1.6)
    hidden, skip = _pair((2, 128, 256, 16, 16), 21)                                 # up-block 1's second pair
    got_h, got_s = unet.up_blocks[1]._freeu(hidden, skip)
    assert got_h.is_contiguous(memory_format=cl) and got_s.is_contiguous(memory_format=cl)
    r_s, r_h = _ratio(got_h, got_s, hidden, skip, 1.6, 0.2)
    print(f"up-block 1 hook: error / bound skip {r_s:.3f} hidden {r_h:.3f}")
    assert r_s <= 1.0 and r_h <= 1.0
    assert unet.up_blocks[2].freeu is None
