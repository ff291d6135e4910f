"""ControlNet support on the GPU.  The three launches of csrc/control.hip bit for bit against their numpy restatements
(tests/control_ref.py): mixdq_control_add_f16 over 16 segments that meet every first and last workgroup of a segment,
mixdq_silu_f16 over all 65 536 FP16 bit patterns, mixdq_hint_to_nhwc8_f16 over dtypes and strides; ControlNet.hint_term
against the same eight convs of stock torch; and a tiny W8A8 UNet + ControlNet: fused == de-fused bit for bit, a graph
replay == eager, the torch form of the adds == the launch, diffusers' keywords == control= with the table [[1.0]]."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import control_ref as R
from tests import inpaint_ref as I
from tests import multistep_ref as M
from tests import sampler_ref as S
from tests.test_control_host import segment_sizes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L_TINY = 32
SENTINEL = np.float16(-7.25)
GAP = 8                                   # sentinel halves behind every segment (keeps the next one 16-byte aligned)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    a = a.detach().cpu().contiguous().numpy() if torch.is_tensor(a) else np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _same(got, want, what):
    """Bit for bit; NaNs compare as NaNs."""
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if g.dtype == np.uint16:
        gn, wn = np.isnan(g.view(np.float16)), np.isnan(w.view(np.float16))
        assert np.array_equal(gn, wn), f"{what}: NaNs at different places"
        g, w = np.where(gn, 0, g), np.where(wn, 0, w)
    assert np.array_equal(g, w), f"{what}: {int((g != w).sum())} of {g.size} elements differ"


# ---- control_add -------------------------------------------------------------------------------------------------
def _coded(seg, n, k):
    """Index-coded FP16 values: a wrong segment, net or offset cannot cancel."""
    e = np.arange(n, dtype=np.int64)
    return (((e * 7 + seg * 131 + k * 977) % 2039 - 1019) / 64.0).astype(np.float16)


class Segments:
    """16 segments carved out of one buffer per operand, a gap of sentinel halves behind each."""

    def __init__(self, C, K, sizes=None):
        self.sizes = sizes if sizes is not None else segment_sizes(C.CONTROL_CHUNK)
        self.K = K
        self.off = np.concatenate([[0], np.cumsum([n + GAP for n in self.sizes])])
        total = int(self.off[-1])
        self.skip = np.full(total, SENTINEL, np.float16)
        self.res = [np.full(total, SENTINEL, np.float16) for _ in range(K)]
        for i, n in enumerate(self.sizes):
            self.skip[self.off[i]:self.off[i] + n] = _coded(i, n, 0)
            for k in range(K):
                self.res[k][self.off[i]:self.off[i] + n] = _coded(i, n, k + 1)

    def views(self, buf):
        return [buf[int(o):int(o) + n] for o, n in zip(self.off, self.sizes)]

    def run(self, C, table, step, in_place=False):
        skip_d, res_d = t(self.skip), [t(r) for r in self.res]
        dst_d = skip_d if in_place else torch.full_like(skip_d, float(SENTINEL))
        out = C.control_add(self.views(skip_d), [self.views(r) for r in res_d], t(np.asarray(table, np.float32)),
                            torch.tensor([step], dtype=torch.int32, device=DEV), out=self.views(dst_d))
        assert all(o.data_ptr() == v.data_ptr() for o, v in zip(out, self.views(dst_d)))
        torch.cuda.synchronize()
        return dst_d.cpu().numpy()

    def want(self, table, step):
        out = np.full_like(self.skip, SENTINEL)
        for i, n in enumerate(self.sizes):
            sl = slice(int(self.off[i]), int(self.off[i]) + n)
            out[sl] = R.control_add_at(self.skip[sl], [r[sl] for r in self.res], table, step)
        return out


TABLE4 = np.array([[1.0, 0.5, 0.25, 2.0, 0.75], [0.3, 1.5, 0.8, 0.1, 1.25], [2.5, 0.7, 1.0, 0.33, 0.9],
                   [0.05, 1.1, 3.0, 0.6, 1.7]], np.float32)


@pytest.mark.parametrize("K", (1, 2, 4))
@pytest.mark.parametrize("step", (0, 2, 4))
def test_control_add_is_the_restatement(C, K, step):
    chunk = C.CONTROL_CHUNK
    s = Segments(C, K)
    assert {8, chunk - 8, chunk, chunk + 8, 3 * chunk + 1000, 0} <= set(s.sizes) and len(s.sizes) == 16
    _same(s.run(C, TABLE4[:K], step), s.want(TABLE4[:K], step), f"K={K}, step {step}")       # (the gaps included)


def test_control_add_skips_a_net_whose_scale_is_zero(C):
    s = Segments(C, 3)
    table = np.array([[0.5, 0.5], [0.0, -0.0], [1.5, 1.5]], np.float32)
    s.res[1][:] = np.float16(np.nan)                                   # never loaded: the result does not see it
    for step in (0, 1):
        got = s.run(C, table, step)
        assert not np.isnan(got).any()
        _same(got, s.want(table, step), f"closed window, step {step}")
    two = Segments(C, 2)
    two.res[1] = s.res[2]
    _same(got, two.want(table[[0, 2]], 1), "K = 3 with a closed net is K = 2 without it")


def test_control_add_with_every_net_off_returns_the_skips_bits(C):
    s = Segments(C, 2)
    s.skip[0:8] = np.array([-0.0, 0.0, np.nan, np.inf, -np.inf, 6.1e-5, -5.96e-8, 65504.0], np.float16)
    s.skip[s.off[4]:s.off[4] + 16:2] = np.float16(-0.0)
    want = s.skip                                                       # (the gaps of both hold the sentinel)
    table = np.array([[0.0, 1.0, 1.0], [0.0, 1.0, 1.0]], np.float32)
    for what, step in (("all scales 0", 0), ("step -1", -1), ("step n_steps", 3), ("step far out", 1 << 30)):
        got = s.run(C, table, step)
        assert np.array_equal(_bits(got), _bits(want)), what              # bits: -0.0 stays -0.0, a NaN keeps its payload
    _same(s.run(C, table, 1), s.want(table, 1), "the same table, in its window")


def test_control_add_in_place(C):
    s = Segments(C, 2)
    _same(s.run(C, TABLE4[:2], 3, in_place=True), s.want(TABLE4[:2], 3), "dst is skip")


def test_control_add_infinities_and_overflow(C):
    s = Segments(C, 2, sizes=[16, C.CONTROL_CHUNK + 8])
    s.res[0][0:8] = np.array([60000, -60000, np.inf, -np.inf, 40000, 65504, 1, np.nan], np.float16)
    s.res[1][0:8] = np.array([1, 1, 1, np.inf, 40000, -65504, np.inf, 1], np.float16)
    s.skip[0:8] = np.array([1, 1, -np.inf, 1, 1, 1, -np.inf, 1], np.float16)
    table = np.array([[2.0], [1.0]], np.float32)                        # 60000 * 2 overflows FP16: inf
    got, want = s.run(C, table, 0), s.want(table, 0)
    assert np.isinf(want[0]) and np.isnan(want[2]) and np.isnan(want[3]) and np.isinf(want[4])
    _same(got, want, "non-finite values")


def test_control_add_refusals_leave_dst_untouched(C):
    lib, chunk = C._lib, C.CONTROL_CHUNK
    n = [chunk + 8, 64]
    skip = [torch.ones(v + 8, dtype=torch.float16, device=DEV) for v in n]
    res = [torch.ones(v + 8, dtype=torch.float16, device=DEV) for v in n]
    dst = [torch.full((v + 8,), float(SENTINEL), dtype=torch.float16, device=DEV) for v in n]
    scales = torch.ones((1, 2), dtype=torch.float32, device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)

    def call(S=2, K=1, n=n, skip_off=0, dst_off=0, res_off=0, n_steps=2, null=None):
        def arr(name, ts, off):
            return (ctypes.c_void_p * 2)(*[None if null == (name, i) else x.data_ptr() + off for i, x in enumerate(ts)])
        return lib.mixdq_control_add_f16(arr("skip", skip, skip_off), arr("dst", dst, dst_off), arr("res", res, res_off),
                                         (ctypes.c_int64 * 2)(*n), S, K, scales.data_ptr(), n_steps, step.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream)

    assert call(n=[chunk + 12, 64]) == 2 and call(n=[chunk + 8, 60]) == 2           # n % 8
    assert call(skip_off=2) == 2 and call(dst_off=8) == 2 and call(res_off=4) == 2    # 16-byte alignment
    assert call(S=0) == 1 and call(S=17) == 1 and call(K=0) == 1 and call(K=5) == 1 and call(n_steps=0) == 1
    assert call(null=("skip", 1)) == 1 and call(null=("dst", 0)) == 1 and call(null=("res", 1)) == 1
    assert call(n=[chunk + 8, -8]) == 1
    torch.cuda.synchronize()
    assert all(bool((d == float(SENTINEL)).all()) for d in dst)
    assert call() == 0                                                              # ... and the call they all vary works
    torch.cuda.synchronize()
    assert all(bool((d[:v] == 2).all()) and bool((d[v:] == float(SENTINEL)).all()) for d, v in zip(dst, n))
    with pytest.raises(RuntimeError, match="multiple of 8 elements"):
        C.control_add([skip[0][:12]], [[res[0][:12]]], scales, step)
    with pytest.raises(RuntimeError, match="should hold 1 tensors"):
        C.control_add([skip[0][:16]], [[res[0][:16], res[0][:16]]], scales, step)
    with pytest.raises(RuntimeError, match=r"scales should be a contiguous fp32 \[1, n_steps\]"):
        C.control_add([skip[0][:16]], [[res[0][:16]]], scales.half(), step)


# ---- silu_f16 ----------------------------------------------------------------------------------------------------
def test_silu_over_every_fp16_value(C, oracle):
    x = np.concatenate([np.arange(65536, dtype=np.uint32), np.arange(1000, dtype=np.uint32) * 61 % 65536]).astype(np.uint16)
    assert x.size % 2048 != 0 and x.size % 8 == 0                       # the last workgroup is partly filled
    x = x.view(np.float16)
    want = R.silu_f16(x, oracle)
    x_d = t(x)
    out = C.silu_f16(x_d)
    _same(out, want, "silu_f16, out of place")
    assert np.array_equal(_bits(x_d), _bits(x))
    buf = torch.full((x.size + 8,), float(SENTINEL), dtype=torch.float16, device=DEV)
    buf[:x.size] = x_d
    assert C.silu_f16(buf[:x.size], out=buf[:x.size]).data_ptr() == buf.data_ptr()
    _same(buf[:x.size], want, "silu_f16, in place")
    assert bool((buf[x.size:] == float(SENTINEL)).all())
    with pytest.raises(RuntimeError, match="multiple of 8 elements"):
        C.silu_f16(x_d[:12])
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        C.silu_f16(x_d[4:20])


# ---- hint_to_nhwc8_f16 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ("uint8", "float16", "float32"))
@pytest.mark.parametrize("layout", ("nchw", "channels_last", "slice"))
@pytest.mark.parametrize("shape", ((1, 3, 5, 7), (2, 1, 5, 7), (2, 3, 24, 40)))
def test_hint_ingest_is_the_restatement(C, dtype, layout, shape):
    rng = np.random.default_rng(sum(shape) + len(dtype) + len(layout))
    B, Cc, H, W = shape
    big = (B, Cc + 1, H + 3, 2 * W + 1)
    if dtype == "uint8":
        src = rng.integers(0, 256, big, dtype=np.uint8)
        src.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)           # every byte value occurs
    else:
        src = rng.uniform(-0.25, 1.25, big).astype(dtype)                # (no clamp: values outside [0, 1] pass through)
    if layout == "slice":
        img_d = t(src)[:, 1:, 2:2 + H, 1:1 + 2 * W:2]
        img = src[:, 1:, 2:2 + H, 1:1 + 2 * W:2]
    else:
        img = np.ascontiguousarray(src[:, :Cc, :H, :W])
        img_d = t(img)
        if layout == "channels_last":
            img_d = img_d.contiguous(memory_format=torch.channels_last)
    out = C.hint_to_nhwc8_f16(img_d)
    assert tuple(out.shape) == (B, 8, H, W) and out.is_contiguous(memory_format=torch.channels_last)
    got = out.permute(0, 2, 3, 1).contiguous().cpu().numpy()
    _same(got, R.hint_to_nhwc8(img), f"{dtype} {layout} {shape}")
    assert not _bits(got[..., Cc:]).any()                               # the padding channels are +0.0


def test_hint_ingest_of_uint8_is_float_div_255_half(C):
    u = torch.arange(256, dtype=torch.uint8, device=DEV).reshape(1, 1, 16, 16)
    got = C.hint_to_nhwc8_f16(u)[:, 0]
    assert torch.equal(got, u[:, 0].float().div(255).half())
    with pytest.raises(RuntimeError, match="1 to 8 channels"):
        C.hint_to_nhwc8_f16(torch.zeros((1, 9, 4, 4), dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="uint8, fp16 or fp32"):
        C.hint_to_nhwc8_f16(torch.zeros((1, 3, 4, 4), dtype=torch.int32, device=DEV))


# ---- hint_term -----------------------------------------------------------------------------------------------------
def test_hint_term_against_stock_convs(C):
    """err_ours <= max(1.5 * err_stock, one FP16 ulp at max |ref|) (the rule of tests/test_vae_enc_gpu.py): ref = the eight
    convs of stock torch in FP32 on the CPU, stock = the same in FP16 on this GPU."""
    import bench
    from mixdq_amd.controlnet import build_controlnet
    net = build_controlnet(DEV, cfg=dict(bench.TINY_CFG, conditioning_embedding_out_channels=(8, 16, 32, 64)))
    emb = net.controlnet_cond_embedding
    with torch.no_grad():                                               # (weights large enough that the output is not all rounding)
        g = torch.Generator(device="cpu").manual_seed(5)
        for m in [emb.conv_in, *emb.blocks, emb.conv_out]:
            fan = m.weight.shape[1] * 9
            m.weight.copy_((torch.randn(m.weight.shape, generator=g) * (2.0 / fan) ** 0.5).to(m.weight))
            m.bias.copy_((torch.randn(m.bias.shape, generator=g) * 0.1).to(m.bias))
    g = torch.Generator(device="cpu").manual_seed(6)
    image = torch.randint(0, 256, (2, 3, 128, 128), generator=g, dtype=torch.uint8).to(DEV)
    term = net.hint_term(image)
    assert tuple(term.shape) == (2, 32, 16, 16) and term.dtype == torch.float16
    assert term.is_contiguous(memory_format=torch.channels_last)
    x16 = image.float().div(255).half()                                 # what the ingest feeds the first conv

    def stock(x, dtype, dev):
        for i, m in enumerate([emb.conv_in, *emb.blocks, emb.conv_out]):
            x = F.conv2d(x, m.weight.to(dev, dtype), m.bias.to(dev, dtype), m.stride, m.padding)
            if i < 7:
                x = F.silu(x)
        return x

    with torch.no_grad():
        ref = stock(x16.float().cpu(), torch.float32, "cpu")
        stock16 = stock(x16, torch.float16, DEV).float().cpu()
    err_ours = (term.float().cpu() - ref).abs().max().item()
    err_stock = (stock16 - ref).abs().max().item()
    amax = ref.abs().max().item()
    ulp = 2.0 ** (torch.tensor(amax).log2().floor().item() - 10)
    print(f"hint_term tiny: max |ref| {amax:.4f}, max err ours {err_ours:.3e}, stock fp16 {err_stock:.3e}, ulp floor {ulp:.3e}")
    assert amax > 1e-2
    assert err_ours <= max(1.5 * err_stock, ulp)
    # an fp16 / fp32 image in [0, 1] of other strides: the same term as its uint8 origin where the values are the same
    assert torch.equal(net.hint_term(x16.contiguous(memory_format=torch.channels_last)), term)
    assert torch.equal(net.hint_term(x16.float()), term)


# ---- a tiny W8A8 UNet and ControlNet -----------------------------------------------------------------------------------
FP16_LAYERS = ("conv_in", "conv_out", "controlnet_cond_embedding", "controlnet_down_blocks", "controlnet_mid_block")


def _w8a8(net, batch):
    import bench
    from mixdq_amd.calib import calibrate, precompute_bos
    from mixdq_amd.quantize_sdxl import quantize_unet
    from mixdq_amd.unet import quantizable_layers
    ckpt = calibrate(net, [batch])
    bos_dict = precompute_bos(net, batch["encoder_hidden_states"])
    names = list(quantizable_layers(net))
    act = {n: 8 for n in names if n.split(".")[0] not in FP16_LAYERS}
    quantize_unet(net, bench.Cfg({n: 8 for n in names}, act), ckpt, bos=True, bos_dict=bos_dict)
    net.set_fused(True)
    return net


@pytest.fixture(scope="module")
def tiny(C):
    """tests/test_ip2p_gpu.py::tiny8's recipe: bench.TINY_CFG with block_out_channels (64, 128, 256), head_dim 64, latent
    32; conv_in and the ControlNet's FP16 layers stay out of the activation config."""
    import bench
    from mixdq_amd.controlnet import build_controlnet
    from mixdq_amd.quantize_sdxl import example_inputs
    from mixdq_amd.unet import build_unet
    cfg = dict(bench.TINY_CFG, block_out_channels=(64, 128, 256), head_dim=64)
    inputs = example_inputs(2, L_TINY, DEV, seed=7)
    g = torch.Generator(device="cpu").manual_seed(8)
    image = torch.randint(0, 256, (2, 3, 8 * L_TINY, 8 * L_TINY), generator=g, dtype=torch.uint8).to(DEV)
    unet = _w8a8(build_unet(DEV, cfg=cfg), inputs)
    nets = [_w8a8(build_controlnet(DEV, seed=4242 + 100 * i, cfg=dict(cfg, conditioning_embedding_out_channels=(8, 16, 32, 64))),
                  dict(inputs, controlnet_cond=image)) for i in range(2)]
    assert not unet.conv_in.valid_for_acceleration and not nets[0].controlnet_mid_block.valid_for_acceleration
    assert nets[0].down_blocks[1].resnets[0].conv1.valid_for_acceleration
    yield dict(unet=unet, nets=nets, inputs=inputs, image=image)
    del unet, nets
    torch.cuda.empty_cache()


def _rows(inputs, B):
    def cut(v):
        if torch.is_tensor(v):
            return v[:B] if v.dim() > 0 and v.shape[0] == 2 else v
        return {k: cut(x) for k, x in v.items()} if isinstance(v, dict) else v
    return {k: cut(v) for k, v in inputs.items()}


def _residuals(net, inp, image):
    term = net.hint_term(image)
    return net(inp["sample"], inp["timestep"], inp["encoder_hidden_states"], inp["added_cond_kwargs"], hint_term=term)


@pytest.mark.parametrize("B", (2, 1))
def test_fused_is_defused_for_both_networks(tiny, B):
    from mixdq_amd import unet as U
    from mixdq_amd.unet import ControlResiduals
    unet, net = tiny["unet"], tiny["nets"][0]
    inp, image = _rows(tiny["inputs"], B), tiny["image"][:B]
    with torch.no_grad():
        down, mid = _residuals(net, inp, image)
        with U.defused():
            down_d, mid_d = _residuals(net, inp, image)
        assert len(down) == unet.n_skips() == 9
        for i, (a, b) in enumerate(zip(down + [mid], down_d + [mid_d])):
            assert a.is_contiguous(memory_format=torch.channels_last) and float(a.abs().max()) > 0
            _same(a, b, f"ControlNet residual {i}, fused vs de-fused")
        table = torch.tensor([[0.5, 1.25, 2.0]], device=DEV)
        ctl = ControlResiduals([(down, mid)], table, torch.tensor([1], dtype=torch.int32, device=DEV))
        fused = unet(**inp, control=ctl)[0]
        with U.defused():
            defused = unet(**inp, control=ctl)[0]
        _same(fused, defused, "UNet with control=, fused vs de-fused")
        plain = unet(**inp)[0]
        assert not torch.equal(fused, plain)                            # the comparison is of something
        # diffusers' keywords with residuals r == control= with the table [[1.0]] on the same r
        one = ControlResiduals([(down, mid)], torch.ones((1, 1), device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV))
        kw = unet(**inp, down_block_additional_residuals=down, mid_block_additional_residual=mid)[0]
        _same(kw, unet(**inp, control=one)[0], "diffusers' keywords vs control=")
        assert not torch.equal(kw, fused) and not torch.equal(kw, plain)
        # the closed window is the plain forward
        off = ControlResiduals([(down, mid)], torch.zeros((1, 2), device=DEV), torch.ones(1, dtype=torch.int32, device=DEV))
        _same(unet(**inp, control=off)[0], plain, "scale 0")


def test_two_nets_and_a_graph_replay(tiny):
    from mixdq_amd.unet import ControlResiduals
    unet, nets = tiny["unet"], tiny["nets"]
    inp, image = tiny["inputs"], tiny["image"]
    table = torch.tensor([[0.5, 1.0, 0.0], [0.0, 0.75, 1.5]], device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    with torch.no_grad():
        terms = [n.hint_term(image) for n in nets]
        args = (inp["sample"], inp["timestep"], inp["encoder_hidden_states"], inp["added_cond_kwargs"])

        def forward():
            res = [n(*args, hint_term=h) for n, h in zip(nets, terms)]
            return unet(**inp, control=ControlResiduals(res, table, step))[0]

        eager = []
        for s in range(3):
            step.fill_(s)
            eager.append(forward().clone())
        assert not torch.equal(eager[0], eager[1]) and not torch.equal(eager[1], eager[2])
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            forward()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = forward()
        for s in range(3):                                              # ONE graph, every column of the table
            step.fill_(s)
            graph.replay()
            _same(out, eager[s], f"graph replay at step {s}")


def _skip_shapes(cfg, B, L):
    """The shapes of the skip tensors and of the mid-block output of a UNet of `cfg` at latent size L."""
    boc, n = cfg["block_out_channels"], cfg.get("layers_per_block", 2)
    shapes = [(B, boc[0], L, L)]
    for i, c in enumerate(boc):
        shapes += [(B, c, L, L)] * n
        if i < len(boc) - 1:
            L //= 2
            shapes.append((B, c, L, L))
    return shapes, (B, boc[-1], L, L)


def torch_form_child():
    """Runs in a process started with MIXDQ_CONTROL_ADD=0: the fused forward of the tiny W8A8 UNet with two nets' worth of
    random residuals, once as the knob asks (torch half operations) and once with the launch switched back on."""
    import bench
    from mixdq_amd import unet as U
    from mixdq_amd.quantize_sdxl import example_inputs
    from mixdq_amd.unet import ControlResiduals, build_unet
    assert U.CONTROL_ADD is False
    cfg = dict(bench.TINY_CFG, block_out_channels=(64, 128, 256), head_dim=64)
    inputs = example_inputs(2, L_TINY, DEV, seed=7)
    unet = _w8a8(build_unet(DEV, cfg=cfg), inputs)
    g = torch.Generator(device="cpu").manual_seed(21)
    down_shapes, mid_shape = _skip_shapes(unet.cfg, 2, L_TINY)
    rand = lambda sh: (torch.randn(sh, generator=g) * 0.5).half().to(DEV).contiguous(memory_format=torch.channels_last)  # noqa: E731
    res = [([rand(sh) for sh in down_shapes], rand(mid_shape)) for _ in range(2)]
    table = torch.tensor([[0.5, 1.0, 0.0], [0.0, 0.75, 1.5]], device=DEV)
    outs = {}
    with torch.no_grad():
        plain = unet(**inputs)[0]
        for flag in (False, True):
            U.CONTROL_ADD = flag
            outs[flag] = [unet(**inputs, control=ControlResiduals(res, table, torch.tensor([s], dtype=torch.int32,
                                                                                           device=DEV)))[0]
                          for s in range(4)]
    for s in range(4):
        assert torch.equal(outs[False][s], outs[True][s]), (s, int((outs[False][s] != outs[True][s]).sum()))
        assert torch.equal(outs[True][s], plain) == (s == 3)            # (step 3 is outside the table)
    print("SAME BITS")


def test_the_torch_form_of_the_adds_gives_the_same_bits():
    """MIXDQ_CONTROL_ADD=0 is read once per process: a child."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MIXDQ_CONTROL_ADD="0")
    r = subprocess.run([sys.executable, "-c", "from tests import test_control_gpu as T; T.torch_form_child()"], cwd=root,
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "SAME BITS" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- the Sampler ---------------------------------------------------------------------------------------------------
N_STEPS, GUIDANCE = 3, 7.5


def _sampler_inputs(B, seed, uses_noise):
    from mixdq_amd.quantize_sdxl import example_inputs
    inp = example_inputs(2 * B, L_TINY, DEV, seed=seed)
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    noise = torch.randn(B, 4, L_TINY, L_TINY, generator=g).to(DEV)
    z = (torch.randn(B, 4, L_TINY, L_TINY, generator=g) * 0.13025).to(DEV)
    mask = (torch.rand(B, L_TINY, L_TINY, generator=g) < 0.5).float().to(DEV)
    images = [torch.randint(0, 256, (B, 3, 8 * L_TINY, 8 * L_TINY), generator=g, dtype=torch.uint8).to(DEV)
              for _ in range(2)]
    step_noise = torch.randn(N_STEPS, B, 4, L_TINY, L_TINY, generator=g).to(DEV) if uses_noise else None
    return noise, inp["encoder_hidden_states"], inp["added_cond_kwargs"], z, mask, images, step_noise


def _eager_loop(unet, nets, sampler, noise, ehs, added, images, scales, starts, ends, step_noise=None, z=None, mask=None):
    """The loop a user would have to write: hint_term once per net, then per step every ControlNet, the scaled residuals
    summed with torch half operations (a net whose scale is 0 at that step left out), the UNet with diffusers' keywords,
    and the numpy restatement of the step (order 2: with the history carried along), the blend's where there is a mask."""
    s, g = sampler.schedule, sampler.guidance_scale
    B = noise.shape[0]
    table = R.scale_table(s.n_steps, 0, scales, starts, ends)
    cl = torch.channels_last
    with torch.no_grad():
        terms = [torch.cat([n.hint_term(im)] * 2, dim=0).contiguous(memory_format=cl) for n, im in zip(nets, images)]
    x, inp = S.init(noise.float().cpu().numpy(), s.init_scale, s.input_scale0)
    if mask is not None:
        z_np, n0 = z.float().cpu().numpy(), noise.float().cpu().numpy()
        m = np.broadcast_to(mask.cpu().numpy().reshape(B, 1, L_TINY, L_TINY), x.shape)
    hist = None
    for i in range(s.n_steps):
        sample = t(np.concatenate([inp] * 2, axis=0))
        ts = torch.tensor(float(s.timesteps[i]), device=DEV)
        with torch.no_grad():
            down = mid = None
            for k, net in enumerate(nets):
                d, md = net(sample, ts, ehs, added, hint_term=terms[k])      # (every net runs, as in the graph)
                c = float(table[k, i])
                if c == 0.0:
                    continue
                d, md = [r * c for r in d], md * c
                down, mid = (d, md) if down is None else ([a + b for a, b in zip(down, d)], mid + md)
            kw = {} if down is None else dict(down_block_additional_residuals=down, mid_block_additional_residual=mid)
            eps = unet(sample, ts, ehs, added, **kw)[0]
        eps = eps.float().cpu().numpy().astype(np.float16)
        if s.order == 2:
            y, hist = M.step(x, hist, eps[:B], eps[B:], s.coef[i], g, M.is_second(s.coef[i], i, 0))
            s_next = s.coef[i, 6]
        else:
            y, _ = S.step(x, eps[:B], eps[B:], s.coef[i], g, step_noise[i].float().cpu().numpy() if s.uses_noise else None)
            s_next = s.coef[i, 3]
        x = y if mask is None else I.blend(y, z_np, n0, m, s.blend[i, 0], s.blend[i, 1])
        inp = M.scaled_input(x, s_next)
    return x


SAMPLER_CALLS = {"euler": ("euler", None), "ancestral_seed": ("euler_ancestral", 11), "dpmpp_2m": ("dpmpp_2m", None)}
# two calls on one Sampler: other scales, other windows -- (0.0, 0.5) closes net 0 for the last two of three steps
CONTROL_ARGS = ((dict(control_scale=[0.8, 1.3], control_start=[0.0, 0.0], control_end=[0.5, 1.0])),
                (dict(control_scale=[1.5, 0.6], control_start=[0.3, 0.0], control_end=[1.0, 0.7])))


@pytest.mark.parametrize("K", (1, 2))
@pytest.mark.parametrize("call", list(SAMPLER_CALLS))
def test_sampler_with_controlnets_equals_the_eager_loop(C, tiny, call, K):
    from mixdq_amd import Sampler
    kind, seed = SAMPLER_CALLS[call]
    unet, nets = tiny["unet"], tiny["nets"][:K]
    sm = Sampler(unet, kind, N_STEPS, GUIDANCE, controlnet=nets if K > 1 else nets[0])
    assert sm.rows_per_image == 2
    graphs, results = None, []
    for j, args in enumerate(CONTROL_ARGS):
        noise, ehs, added, z, mask, images, sn = _sampler_inputs(2, 60 + j, sm.schedule.uses_noise and seed is None)
        kw = {k: v[:K] for k, v in args.items()}
        control = images[:K] if K > 1 else images[0]
        if seed is not None:
            shape = tuple(noise.shape)
            sd = torch.tensor([seed, seed + 1], dtype=torch.int64, device=DEV)
            got = sm.sample(shape, ehs, added, seed=seed, control=control, **kw)
            noise = C.randn(shape, sd)
            sn = torch.stack([C.randn(shape, sd, C.RNG_STREAM_STEP, i) for i in range(N_STEPS)])
        else:
            got = sm.sample(noise, ehs, added, sn, control=control, **kw)
        now = (sm._graph, sm._graph_masked, sm._graph_rng, sm._graph_masked_rng)
        assert sum(gr is not None for gr in now) == 1 and (graphs is None or now == graphs), "one graph, never re-captured"
        graphs = now
        table = R.scale_table(N_STEPS, 0, kw["control_scale"], kw["control_start"], kw["control_end"])
        assert np.array_equal(sm._ctl_scales.cpu().numpy(), table)          # the table of THIS call
        want = _eager_loop(unet, nets, sm, noise, ehs, added, images, kw["control_scale"], kw["control_start"],
                           kw["control_end"], sn)
        assert got.dtype == torch.float32 and bool(torch.isfinite(got).all())
        _same(got, want, f"{call}, K = {K}, call {j}")
        results.append(got)
    assert not torch.equal(results[0], results[1])
    if call == "euler":
        # a masked call on the same Sampler: a second graph, the first untouched; the hint as a ready term this time
        kw = {k: v[:K] for k, v in CONTROL_ARGS[0].items()}
        terms = [n.hint_term(im) for n, im in zip(nets, images)]
        got = sm.sample(noise, ehs, added, init_latents=z, mask=mask, control=terms if K > 1 else terms[0], **kw)
        assert sm._graph is graphs[0] and sm._graph_masked is not None
        want = _eager_loop(unet, nets, sm, noise, ehs, added, images, kw["control_scale"], kw["control_start"],
                           kw["control_end"], None, z, mask)
        _same(got, want, f"masked, K = {K}")


def test_sampler_without_controlnet_is_what_it_was(C, tiny):
    """No controlnet=: the binding and the graph count recorded before, the bits of the plain eager loop -- and a Sampler
    WITH a ControlNet whose scale is 0 returns those same bits (dst is the skip's own bits)."""
    from mixdq_amd import Sampler
    unet, nets = tiny["unet"], tiny["nets"]
    noise, ehs, added, z, mask, images, _ = _sampler_inputs(2, 70, False)
    plain = Sampler(unet, "euler", N_STEPS, GUIDANCE)
    got = plain.sample(noise, ehs, added)
    assert plain._step_binding == "sampler_step" and plain._hint_terms is None and plain._ctl_scales is None
    assert [g is not None for g in (plain._graph, plain._graph_masked, plain._graph_rng, plain._graph_masked_rng)] == [
        True, False, False, False]
    _same(got, _eager_loop(unet, [], plain, noise, ehs, added, [], [], [], []), "plain Sampler vs the plain eager loop")
    with pytest.raises(TypeError, match="built without controlnet="):
        plain.sample(noise, ehs, added, control=images[0])
    ctl = Sampler(unet, "euler", N_STEPS, GUIDANCE, controlnet=nets[0])
    assert ctl.sample(noise, ehs, added, control=images[0])._version >= 0 and ctl._step_binding == "sampler_step"
    on = ctl.sample(noise, ehs, added, control=images[0])
    off = ctl.sample(noise, ehs, added, control=images[0], control_scale=0.0)
    _same(off, got, "scale 0 vs no ControlNet")
    assert not torch.equal(on, got)
    with pytest.raises(TypeError, match="control= .* is required"):
        ctl.sample(noise, ehs, added)
