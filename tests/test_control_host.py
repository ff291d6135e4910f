"""ControlNet support, the parts that need no GPU: the scale table of a run against diffusers' controlnet_keep loop, the
ControlNet's parameter counts and names, the uint8 ingest rule, the UNet's residual entry on the CPU against a
hand-written forward, the refusals, the header -- and what the three entry points of csrc/control.hip LAUNCH, recorded
as tests/test_launch_trace_rescale_host.py records its unit: exact grids, refusals that launch nothing, and the objects
of mixdq_amd/_obj/ and _obj/ext/ registering what they registered before (the new unit's object lives in _obj/ext2/).

`python -m tests.test_control_host trace` is the child process that drives the trace library
(_obj/ext2/libmixdq_trace_control.so: the stand-in runtime linked against every object)."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import control_ref as R
from tests import launch_trace as lt

EXT = os.path.join(lt.OBJ, "ext")
EXT2 = os.path.join(lt.OBJ, "ext2")
TRACE_LIB = os.path.join(EXT2, "libmixdq_trace_control.so")
INVALID, ALIGNMENT = 1, 2
SILU_SPAN = 2048


# ---------------------------------------------------------------------------------------------- the scale table
def diffusers_keep(num_steps, starts, ends):
    """diffusers' pipeline loop, literally (StableDiffusionControlNetPipeline.__call__):
        keeps = [1.0 - float(i / len(timesteps) < s or (i + 1) / len(timesteps) > e) for s, e in zip(start, end)]"""
    controlnet_keep = []
    for i in range(num_steps):
        keeps = [1.0 - float(i / num_steps < s or (i + 1) / num_steps > e) for s, e in zip(starts, ends)]
        controlnet_keep.append(keeps)
    return controlnet_keep


WINDOWS = ((0.0, 1.0), (0.0, 0.5), (0.25, 0.75), (0.5, 0.5))


@pytest.mark.parametrize("n_steps", (1, 4, 20))
@pytest.mark.parametrize("window", WINDOWS)
def test_scale_table_is_diffusers_keep_rule(n_steps, window):
    from mixdq_amd.controlnet import control_scale_table
    for scale in (1.0, 0.35):
        got = control_scale_table(n_steps, 0, [scale], [window[0]], [window[1]])
        keep = diffusers_keep(n_steps, [window[0]], [window[1]])
        want = np.array([[np.float32(scale * keep[j][0]) for j in range(n_steps)]], np.float32)
        assert got.dtype == np.float32 and got.shape == (1, n_steps)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (n_steps, window, got, want)
        assert np.array_equal(got, R.scale_table(n_steps, 0, [scale], [window[0]], [window[1]]))
    if window == (0.0, 0.5) and n_steps == 20:
        assert got[0, :10].all() and not got[0, 10:].any()             # the last steps run with scale 0


def test_scale_table_of_an_img2img_start_and_of_two_nets():
    from mixdq_amd.controlnet import control_scale_table
    # a run of 20 scheduled steps that starts at step 8: diffusers' loop sees 12 timesteps
    got = control_scale_table(20, 8, [0.75, 1.5], [0.0, 0.25], [0.5, 0.75])
    keep = diffusers_keep(12, [0.0, 0.25], [0.5, 0.75])
    want = np.zeros((2, 20), np.float32)
    for j in range(12):
        for k, s in enumerate((0.75, 1.5)):
            want[k, 8 + j] = np.float32(s * keep[j][k])
    assert np.array_equal(got, want) and not got[:, :8].any()
    assert got[0].tolist() != got[1].tolist()
    assert np.array_equal(got, R.scale_table(20, 8, [0.75, 1.5], [0.0, 0.25], [0.5, 0.75]))
    with pytest.raises(ValueError, match="one scale, start and end per net"):
        control_scale_table(4, 0, [1.0, 1.0], [0.0], [1.0])
    with pytest.raises(ValueError, match="control_start <= control_end"):
        control_scale_table(4, 0, [1.0], [0.75], [0.5])
    with pytest.raises(ValueError, match="first step"):
        control_scale_table(4, 4, [1.0], [0.0], [1.0])


# ---------------------------------------------------------------------------------------------- the module
@pytest.mark.parametrize("which,count", (("SD15", 361_279_120), ("SDXL", 1_251_014_160), ("SD21", 364_228_240)))
def test_parameter_counts(which, count):
    from mixdq_amd import controlnet as CN
    with torch.device("meta"):
        net = CN.ControlNet(getattr(CN, f"CONTROLNET_{which}_CONFIG"))
    assert sum(p.numel() for p in net.parameters()) == count


def test_state_dict_names_are_diffusers():
    from mixdq_amd import controlnet as CN
    from mixdq_amd.unet import SD15_CONFIG, SDXLUNet
    with torch.device("meta"):
        net = CN.ControlNet(CN.CONTROLNET_SD15_CONFIG)
        unet = SDXLUNet(SD15_CONFIG)
    trunk = {k for k in unet.state_dict() if k.split(".")[0] in ("conv_in", "time_embedding", "down_blocks", "mid_block")}
    own = set()
    for name in (["controlnet_cond_embedding.conv_in", "controlnet_cond_embedding.conv_out", "controlnet_mid_block"]
                 + [f"controlnet_cond_embedding.blocks.{i}" for i in range(6)]
                 + [f"controlnet_down_blocks.{i}" for i in range(12)]):
        own |= {name + ".weight", name + ".bias"}
    assert set(net.state_dict()) == trunk | own
    sd = net.state_dict()
    assert tuple(sd["controlnet_cond_embedding.conv_in.weight"].shape) == (16, 3, 3, 3)
    assert tuple(sd["controlnet_cond_embedding.blocks.1.weight"].shape) == (32, 16, 3, 3)
    assert tuple(sd["controlnet_cond_embedding.conv_out.weight"].shape) == (320, 256, 3, 3)
    assert tuple(sd["controlnet_down_blocks.0.weight"].shape) == (320, 320, 1, 1)
    assert tuple(sd["controlnet_down_blocks.11.weight"].shape) == (1280, 1280, 1, 1)
    emb = net.controlnet_cond_embedding
    assert [b.stride[0] for b in emb.blocks] == [1, 2, 1, 2, 1, 2] and all(b.padding == (1, 1) for b in emb.blocks)
    assert net.n_skips() == unet.n_skips() == 12


def test_uint8_ingest_rule_is_float_div_255_half():
    u = np.arange(256, dtype=np.uint8)
    want = torch.tensor(u).float().div(255).half().numpy()
    assert np.array_equal(R.hint_unit_u8(u).view(np.uint16), want.view(np.uint16))
    img = np.arange(2 * 3 * 5 * 7, dtype=np.int64).reshape(2, 3, 5, 7).astype(np.uint8)
    out = R.hint_to_nhwc8(img)
    assert out.shape == (2, 5, 7, 8) and not out[..., 3:].view(np.uint16).any()
    assert np.array_equal(out[..., :3], np.transpose(want[img], (0, 2, 3, 1)))


# ---------------------------------------------------------------------------------------------- the UNet's entry
TINY = dict(block_out_channels=(32, 64, 128), transformer_layers_per_block=(0, 1, 2), mid_transformer_layers=1,
            head_dim=16, cross_attention_dim=64, time_embed_dim=128, addition_time_embed_dim=16,
            projection_class_embeddings_input_dim=32 + 96, norm_num_groups=8)


def _tiny_inputs(B=2, L=8, seed=3):
    g = torch.Generator().manual_seed(seed)
    return dict(sample=torch.randn(B, 4, L, L, generator=g), timestep=torch.tensor(500.0),
                encoder_hidden_states=torch.randn(B, 7, 64, generator=g),
                added_cond_kwargs=dict(time_ids=torch.tensor([[64., 64, 0, 0, 64, 64]]).repeat(B, 1),
                                       text_embeds=torch.randn(B, 32, generator=g)))


@pytest.fixture(scope="module")
def tiny():
    from mixdq_amd.controlnet import ControlNet
    from mixdq_amd.unet import SDXLUNet, init_synthetic_weights
    unet = init_synthetic_weights(SDXLUNet(TINY), std=0.05).eval()
    net = init_synthetic_weights(ControlNet(dict(TINY, conditioning_embedding_out_channels=(8, 16, 32, 64))), seed=77,
                                 std=0.05).eval()
    return unet, net


def _by_hand(unet, inp, down, mid):
    """SDXLUNet.forward written out, with the residuals added to the skips and to the mid-block output."""
    emb = unet._embed(inp["sample"], inp["timestep"], inp["added_cond_kwargs"])
    ehs = inp["encoder_hidden_states"]
    x = unet.conv_in(inp["sample"].contiguous(memory_format=torch.channels_last))
    skips = [x]
    for blk in unet.down_blocks:
        x, outs = blk(x, emb, ehs)
        skips += outs
    x = unet.mid_block(x, emb, ehs)
    skips = [s + r for s, r in zip(skips, down)]
    x = x + mid
    for blk in unet.up_blocks:
        x = blk(x, skips, emb, ehs)
    return unet.conv_out(unet.conv_act(unet.conv_norm_out(x)))


@torch.no_grad()
def test_cpu_forward_with_residuals_equals_a_hand_written_forward(tiny):
    from mixdq_amd.unet import ControlResiduals
    unet, net = tiny
    inp = _tiny_inputs()
    g = torch.Generator().manual_seed(11)
    image = torch.rand(2, 3, 64, 64, generator=g)
    down, mid = net(inp["sample"], inp["timestep"], inp["encoder_hidden_states"], inp["added_cond_kwargs"],
                    controlnet_cond=image)
    assert len(down) == unet.n_skips() == 9 and all(d.abs().max() > 0 for d in down) and mid.abs().max() > 0
    plain = unet(**inp)[0]
    got = unet(**inp, down_block_additional_residuals=down, mid_block_additional_residual=mid)[0]
    assert torch.equal(got, _by_hand(unet, inp, down, mid))
    assert not torch.equal(got, plain)
    # control= with the scale table [[1.0]] at step 0 is the same thing; scale 0 and a step outside the table: the plain forward
    one = ControlResiduals([(down, mid)], torch.ones(1, 1), torch.zeros(1, dtype=torch.int32))
    assert torch.equal(unet(**inp, control=one)[0], got)
    off = ControlResiduals([(down, mid)], torch.zeros(1, 1), torch.zeros(1, dtype=torch.int32))
    assert torch.equal(unet(**inp, control=off)[0], plain)
    out_of_table = ControlResiduals([(down, mid)], torch.ones(1, 3), torch.full((1,), 3, dtype=torch.int32))
    assert torch.equal(unet(**inp, control=out_of_table)[0], plain)
    # two nets, scales read at step 1 of a table whose rows differ: skip + (r0 * a + r1 * b), left to right
    table = torch.tensor([[9.0, 0.5, 9.0], [9.0, 2.0, 9.0]])
    two = ControlResiduals([(down, mid), ([d.flip(0) for d in down], mid.flip(0))], table,
                           torch.ones(1, dtype=torch.int32))
    want = _by_hand(unet, inp, [d * 0.5 + d.flip(0) * 2.0 for d in down], mid * 0.5 + mid.flip(0) * 2.0)
    assert torch.equal(unet(**inp, control=two)[0], want)
    # the ControlNet's two call shapes agree, and conditioning_scale multiplies
    term = net.hint_term(image)
    d2, m2 = net(inp["sample"], inp["timestep"], inp["encoder_hidden_states"], inp["added_cond_kwargs"], hint_term=term)
    assert all(torch.equal(a, b) for a, b in zip(down, d2)) and torch.equal(mid, m2)
    d3, m3 = net(inp["sample"], inp["timestep"], inp["encoder_hidden_states"], inp["added_cond_kwargs"],
                 controlnet_cond=(image * 255).round().to(torch.uint8), conditioning_scale=0.5)
    ref_term = net.controlnet_cond_embedding((image * 255).round().to(torch.uint8).float().div(255))
    d4, m4 = net(inp["sample"], inp["timestep"], inp["encoder_hidden_states"], inp["added_cond_kwargs"],
                 hint_term=ref_term.contiguous(memory_format=torch.channels_last))
    assert all(torch.equal(a, b * 0.5) for a, b in zip(d3, d4)) and torch.equal(m3, m4 * 0.5)


@torch.no_grad()
def test_unet_refusals(tiny):
    from mixdq_amd.unet import ControlResiduals
    unet, net = tiny
    inp = _tiny_inputs()
    image = torch.rand(2, 3, 64, 64)
    down, mid = net(inp["sample"], inp["timestep"], inp["encoder_hidden_states"], inp["added_cond_kwargs"],
                    controlnet_cond=image)
    step, one = torch.zeros(1, dtype=torch.int32), torch.ones(1, 1)
    with pytest.raises(RuntimeError, match="go together"):
        unet(**inp, down_block_additional_residuals=down)
    with pytest.raises(RuntimeError, match="exclude each other"):
        unet(**inp, mid_block_additional_residual=mid, control=ControlResiduals([(down, mid)], one, step))
    with pytest.raises(RuntimeError, match="should be a mixdq_amd.unet.ControlResiduals"):
        unet(**inp, control=(down, mid))
    with pytest.raises(RuntimeError, match="9 skip tensors: net 0 should bring 9 down residuals, got 8"):
        unet(**inp, down_block_additional_residuals=down[:-1], mid_block_additional_residual=mid)
    with pytest.raises(RuntimeError, match="1 to 4 ControlNets, got 5"):
        unet(**inp, control=ControlResiduals([(down, mid)] * 5, torch.ones(5, 1), step))
    with pytest.raises(RuntimeError, match=r"control.scales should be a contiguous fp32 \[1, n_steps\]"):
        unet(**inp, control=ControlResiduals([(down, mid)], torch.ones(2, 1), step))
    with pytest.raises(RuntimeError, match="control.step should be one int32"):
        unet(**inp, control=ControlResiduals([(down, mid)], one, torch.zeros(1)))
    bad = list(down)
    bad[2] = bad[2][:, :-1]
    with pytest.raises(RuntimeError, match="net 0, down residual 2 should be a channels-last torch.float32 tensor of shape"):
        unet(**inp, down_block_additional_residuals=bad, mid_block_additional_residual=mid)
    with pytest.raises(RuntimeError, match="the mid residual should be"):
        unet(**inp, down_block_additional_residuals=down, mid_block_additional_residual=mid.half())
    nchw = list(down)
    nchw[1] = nchw[1].contiguous()
    with pytest.raises(RuntimeError, match="down residual 1 should be a channels-last"):
        unet(**inp, down_block_additional_residuals=nchw, mid_block_additional_residual=mid)
    # the ControlNet's own
    args = (inp["sample"], inp["timestep"], inp["encoder_hidden_states"], inp["added_cond_kwargs"])
    with pytest.raises(RuntimeError, match="one of the two"):
        net(*args)
    with pytest.raises(RuntimeError, match="one of the two"):
        net(*args, hint_term=down[0], controlnet_cond=image)
    with pytest.raises(RuntimeError, match="8 times its height and width"):
        net(*args, controlnet_cond=image[:, :, :32])
    with pytest.raises(RuntimeError, match="hint image should be a uint8, fp16 or fp32"):
        net.hint_term(image[:, :2])
    with pytest.raises(RuntimeError, match="hint_term should be a channels-last"):
        net(*args, hint_term=down[0][:1])
    net.conv_in.valid_for_acceleration = True
    try:
        with pytest.raises(RuntimeError, match="leave 'conv_in' out of the activation bit-width config"):
            net(*args, controlnet_cond=image)
    finally:
        del net.conv_in.valid_for_acceleration


def test_sampler_refusals(tiny):
    """The calling convention of Sampler(controlnet=) / sample(control=): every refusal comes before any GPU work."""
    from mixdq_amd import Sampler
    unet, net = tiny
    with pytest.raises(TypeError, match="controlnet should be a mixdq_amd.controlnet.ControlNet or a list of them"):
        Sampler(unet, "euler", 4, 7.5, controlnet=unet)
    with pytest.raises(TypeError, match="controlnet should be"):
        Sampler(unet, "euler", 4, 7.5, controlnet=[])
    with pytest.raises(ValueError, match="at most 4 ControlNets, got 5"):
        Sampler(unet, "euler", 4, 7.5, controlnet=[net] * 5)
    with pytest.raises(ValueError, match="three guidance rows .* together with controlnet= are not supported yet"):
        Sampler(unet, "euler", 4, 7.5, image_guidance_scale=1.5, controlnet=net)
    inp = _tiny_inputs()
    noise, ehs, added = torch.randn(1, 4, 8, 8), inp["encoder_hidden_states"], inp["added_cond_kwargs"]
    with_net = Sampler(unet, "euler", 4, 7.5, controlnet=net)
    assert with_net.controlnets == [net] and with_net.rows_per_image == 2
    assert Sampler(unet, "euler", 4, 7.5, controlnet=[net, net]).controlnets == [net, net]
    with pytest.raises(TypeError, match="built with controlnet=: control= .* is required"):
        with_net.sample(noise, ehs, added)
    without = Sampler(unet, "euler", 4, 7.5)
    assert without.controlnets == []
    with pytest.raises(TypeError, match="control given, but this Sampler was built without controlnet="):
        without.sample(noise, ehs, added, control=torch.zeros(1, 3, 64, 64))
    with pytest.raises(TypeError, match="built without controlnet="):
        without.sample_image(None, noise, ehs, added, control=torch.zeros(1, 3, 64, 64))
    # what needs the shapes only: the counts per net and the forms of a hint
    dev = noise.device
    for kw, text in ((dict(control=[torch.zeros(1, 3, 64, 64)] * 2), r"one hint per ControlNet \(1\), got 2"),
                     (dict(control=torch.zeros(1, 3, 64, 64), control_scale=[1.0, 2.0]),
                      r"control_scale should be a number or one per ControlNet \(1\)"),
                     (dict(control=torch.zeros(1, 3, 64, 64), control_start=0.75, control_end=0.5),
                      "control_start <= control_end")):
        with pytest.raises(ValueError, match=text):
            with_net._set_control(kw["control"], kw.get("control_scale", 1.0), kw.get("control_start", 0.0),
                                  kw.get("control_end", 1.0), noise, 0)
    for bad in (torch.zeros(1, 3, 32, 64), torch.zeros(3, 3, 64, 64), torch.zeros(1, 32, 8, 8), "image"):
        with pytest.raises(RuntimeError, match=r"control\[0\] should be"):
            with_net._set_control(bad, 1.0, 0.0, 1.0, noise, 0)
    assert dev.type == "cpu"


def test_header_declares_the_entry_points():
    header = open(lt.HEADER).read()
    for name in ("mixdq_control_add_f16", "mixdq_silu_f16", "mixdq_hint_to_nhwc8_f16", "mixdq_control_chunk"):
        assert re.search(rf"^int {name}\(", header, re.M), name
    assert re.search(r"^#define MIXDQ_ABI_VERSION 3$", header, re.M)
    from mixdq_amd.build import build
    lib = ctypes.CDLL(build())
    assert lib.mixdq_abi_version() == 3
    chunk = lib.mixdq_control_chunk()
    assert chunk >= 2048 and chunk % 2048 == 0
    math_h = open(os.path.join(lt.ROOT, "include", "mixdq_math.h")).read()
    for name in ("mixdq_control_scaled", "mixdq_control_sum", "mixdq_hint_unit"):
        assert name in math_h


# ---------------------------------------------------------------------------------------------- the launch trace
def build_trace_lib():
    objs = sorted(os.path.join(d, f) for d in (lt.OBJ, EXT, EXT2) for f in os.listdir(d) if f.endswith(".o"))
    assert any(o.startswith(EXT2) for o in objs), f"no objects under {EXT2}: run mixdq_amd.build.build() first"
    deps = objs + [lt.RUNTIME_SRC]
    if not os.path.exists(TRACE_LIB) or any(os.path.getmtime(d) > os.path.getmtime(TRACE_LIB) for d in deps):
        tmp = TRACE_LIB + f".{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wl,-Bsymbolic", "-o", tmp,
                               lt.RUNTIME_SRC] + objs)
        os.replace(tmp, TRACE_LIB)
    return TRACE_LIB


class Tracer(lt.Tracer):
    def __init__(self):
        self.lib = ctypes.CDLL(build_trace_lib())
        self.lib.launch_trace_take.restype = ctypes.c_char_p
        self.lib.launch_trace_kernels.restype = ctypes.c_char_p
        self.sig = lt.signatures()
        self.kernels = sorted(set(self.lib.launch_trace_kernels().decode().split()))
        self.index = {k: i for i, k in enumerate(self.kernels)}
        self.out = {}
        self.keep = []


def segment_sizes(chunk):
    """16 segments: every first and last workgroup of a segment, and two empty ones."""
    return [8, chunk - 8, chunk, chunk + 8, 3 * chunk + 1000, 0, 2 * chunk, 16, chunk - 16, 0, 5 * chunk + 8, 8,
            chunk + 2048, 2 * chunk - 8, 4 * chunk, 24]


def record():
    t = Tracer()
    chunk = t.lib.mixdq_control_chunk()
    sizes = segment_sizes(chunk)

    def arrays(S, K, n=None, skip_at=None, dst_at=None, res_at=None):
        n = list(n if n is not None else sizes[:S])
        skip = [lt.ptr(100 + i) for i in range(S)]
        dst = [lt.ptr(120 + i) for i in range(S)]
        res = [lt.ptr(140 + k * 16 + i) for k in range(K) for i in range(S)]
        for at, arr in ((skip_at, skip), (dst_at, dst), (res_at, res)):
            if at is not None:
                arr[at[0]] = at[1]
        return dict(skip=t.host(ctypes.c_void_p, skip), dst=t.host(ctypes.c_void_p, dst),
                    residuals=t.host(ctypes.c_void_p, res), n=t.host(ctypes.c_int64, n), S=S, K=K)

    e = t.entry("mixdq_control_add_f16", n_steps=20, **arrays(16, 1))
    for K in (1, 2, 3, 4):
        e.case(f"s16_k{K}", **arrays(16, K))
        e.case(f"s1_k{K}", **arrays(1, K, n=[chunk + 8]))
    e.case("s13_sd15", **arrays(13, 2, n=[320 * 4096] * 3 + [320 * 1024] + [640 * 1024] * 2 + [640 * 256]
                                + [1280 * 256] * 2 + [1280 * 64] * 4))
    e.case("in_place", **dict(arrays(16, 2), dst=arrays(16, 2)["skip"]))
    e.case("all_empty", **arrays(3, 2, n=[0, 0, 0]))
    e.case("empty_with_null_pointers", **arrays(2, 1, n=[0, chunk], skip_at=(0, None), res_at=(0, None)))
    e.case("refuse_s0", **dict(arrays(1, 1), S=0))
    e.case("refuse_s17", **dict(arrays(16, 1), S=17))
    e.case("refuse_k0", **dict(arrays(2, 1), K=0))
    e.case("refuse_k5", **dict(arrays(2, 4), K=5))
    e.case("refuse_n_steps0", n_steps=0)
    e.case("refuse_null_skip_array", skip=None)
    e.case("refuse_null_dst_array", dst=None)
    e.case("refuse_null_residual_array", residuals=None)
    e.case("refuse_null_n", n=None)
    e.case("refuse_null_scales", scales=None)
    e.case("refuse_null_step", step=None)
    e.case("refuse_negative_n", **arrays(3, 1, n=[8, -8, 8]))
    e.case("refuse_null_skip", **arrays(3, 1, skip_at=(1, None)))
    e.case("refuse_null_dst", **arrays(3, 1, dst_at=(2, None)))
    e.case("refuse_null_residual", **arrays(3, 2, res_at=(4, None)))
    e.case("refuse_n_not_multiple_of_8", **arrays(3, 1, n=[8, 12, 8]))
    e.case("refuse_skip_misaligned", **arrays(3, 1, skip_at=(0, lt.ptr(100) + 8)))
    e.case("refuse_dst_misaligned", **arrays(3, 1, dst_at=(1, lt.ptr(121) + 2)))
    e.case("refuse_residual_misaligned", **arrays(3, 2, res_at=(5, lt.ptr(150) + 4)))
    e.case("refuse_scales_misaligned", scales=lt.ptr(7) + 2)
    e.case("refuse_step_misaligned", step=lt.ptr(9) + 1)
    s = t.entry("mixdq_silu_f16", n=4096)
    for n in (8, SILU_SPAN - 8, SILU_SPAN, SILU_SPAN + 8, 65536, 3 * SILU_SPAN + 1000):
        s.case(f"n{n}", n=n)
    s.case("in_place", out_f16=lt.ptr(1))
    s.case("n0", n=0, x_f16=None, out_f16=None)
    s.case("refuse_negative", n=-8)
    s.case("refuse_null_x", x_f16=None)
    s.case("refuse_null_out", out_f16=None)
    s.case("refuse_n_not_multiple_of_8", n=12)
    s.case("refuse_x_misaligned", x_f16=lt.ptr(1) + 8)
    s.case("refuse_out_misaligned", out_f16=lt.ptr(2) + 2)
    h = t.entry("mixdq_hint_to_nhwc8_f16", dtype=0, B=2, C=3, H=64, W=64, sb=3 * 64 * 64, sc=64 * 64, sh=64, sw=1)
    for d, dl in ((0, "u8"), (1, "f16"), (2, "f32")):
        h.case(dl, dtype=d)
        h.case(f"{dl}_5x7", dtype=d, B=1, H=5, W=7)
    h.case("large", B=8, H=1024, W=1024, sb=3 << 20, sc=1 << 20, sh=1024)
    h.case("empty", B=0, img=None, out_f16=None)
    h.case("refuse_dtype", dtype=3)
    h.case("refuse_c0", C=0)
    h.case("refuse_c9", C=9)
    h.case("refuse_negative", H=-1)
    h.case("refuse_null_img", img=None)
    h.case("refuse_null_out", out_f16=None)
    h.case("refuse_out_misaligned", out_f16=lt.ptr(7) + 8)
    h.case("refuse_img_misaligned", dtype=2, img=lt.ptr(1) + 2)
    return {"kernels": t.kernels, "cases": t.out, "chunk": chunk}


@pytest.fixture(scope="module")
def trace():
    build_trace_lib()
    env = {k: v for k, v in os.environ.items() if not k.startswith("MIXDQ_") or k == "MIXDQ_TRACE_OBJ"}
    r = subprocess.run([sys.executable, "-m", "tests.test_control_host", "trace"], cwd=lt.ROOT, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout)


def _demangled(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return r.stdout.split("\n")[:len(names)]


def _events(trace, case):
    status, events = trace["cases"][case].split("|", 1)
    names = _demangled(trace["kernels"])
    out = []
    for ev in filter(None, events.split(";")):
        assert ev.startswith("L"), (case, ev)              # nothing but launches: no copy, no synchronisation
        i, grid, block, lds = ev[1:].split(":")
        out.append((names[int(i)], grid, block, lds))
    return int(status), out


def test_control_add_grids_are_exact(trace):
    chunk = trace["chunk"]
    blocks = lambda n: sum((v + chunk - 1) // chunk for v in n)          # noqa: E731
    sizes = segment_sizes(chunk)
    for K in (1, 2, 3, 4):
        for case, n in ((f"s16_k{K}", sizes), (f"s1_k{K}", [chunk + 8])):
            status, ev = _events(trace, f"control_add_f16/{case}")
            assert status == 0 and len(ev) == 1, (case, ev)                 # ONE launch for all segments
            name, grid, block, lds = ev[0]
            assert f"control_add_kernel<{K}>" in name and grid == f"{blocks(n)},1,1" and block == "256" and lds == "0"
    status, ev = _events(trace, "control_add_f16/s13_sd15")
    n = [320 * 4096] * 3 + [320 * 1024] + [640 * 1024] * 2 + [640 * 256] + [1280 * 256] * 2 + [1280 * 64] * 4
    assert status == 0 and [e[1] for e in ev] == [f"{blocks(n)},1,1"]
    status, ev = _events(trace, "control_add_f16/in_place")
    assert status == 0 and len(ev) == 1
    assert _events(trace, "control_add_f16/all_empty") == (0, [])
    status, ev = _events(trace, "control_add_f16/empty_with_null_pointers")
    assert status == 0 and [e[1] for e in ev] == ["1,1,1"]


def test_silu_and_hint_grids_are_exact(trace):
    for n in (8, SILU_SPAN - 8, SILU_SPAN, SILU_SPAN + 8, 65536, 3 * SILU_SPAN + 1000):
        status, ev = _events(trace, f"silu_f16/n{n}")
        assert status == 0 and len(ev) == 1 and "silu_f16_kernel" in ev[0][0]
        assert ev[0][1:] == (f"{(n + SILU_SPAN - 1) // SILU_SPAN},1,1", "256", "0")
    assert _events(trace, "silu_f16/in_place")[1][0][1] == "2,1,1"
    assert _events(trace, "silu_f16/n0") == (0, [])
    for dl, T in (("u8", "unsigned char"), ("f16", "__half"), ("f32", "float")):
        for case, pixels in ((dl, 2 * 64 * 64), (f"{dl}_5x7", 35)):
            status, ev = _events(trace, f"hint_to_nhwc8_f16/{case}")
            assert status == 0 and len(ev) == 1 and f"hint_to_nhwc8_kernel<{T}>" in ev[0][0], ev
            assert ev[0][1:] == (f"{(pixels + 255) // 256},1,1", "256", "0")
    assert _events(trace, "hint_to_nhwc8_f16/large")[1][0][1] == f"{8 * 1024 * 1024 // 256},1,1"
    assert _events(trace, "hint_to_nhwc8_f16/empty") == (0, [])


def test_refusals_launch_nothing(trace):
    misaligned = ("n_not_multiple_of_8", "misaligned")
    refused = {c: v for c, v in trace["cases"].items() if "/refuse_" in c}
    assert len(refused) == 21 + 6 + 8
    for c, v in refused.items():
        want = ALIGNMENT if c.endswith(misaligned) else INVALID
        assert v == f"{want}|", (c, v)


def test_the_recorded_objects_register_what_they_registered(trace):
    """_obj/*.o: the kernels of tests/golden/launch_trace.json; _obj/ext/*.o: 35 more, the rescale unit's; everything
    beyond those comes from csrc/control.hip and is its eight kernels."""
    with open(lt.GOLDEN) as f:
        before = set(json.load(f)["kernels"])
    now = set(trace["kernels"])
    assert before <= now, sorted(before - now)[:4]
    new = _demangled(sorted(now - before))
    rescale = [k for k in new if "sampler_rescale_" in k or "sampler_step_rescaled_kernel<" in k]
    assert len(rescale) == 4 + 1 + 30
    ours = sorted(k for k in new if k not in rescale)
    assert len(ours) == 8, ours
    for want in [f"control_add_kernel<{K}>" for K in (1, 2, 3, 4)] + ["silu_f16_kernel"] + [
            f"hint_to_nhwc8_kernel<{T}>" for T in ("unsigned char", "__half", "float")]:
        assert sum(want in k for k in ours) == 1, (want, ours)
    # ... and the libraries of the two earlier object sets do not see the new unit at all
    for d in (lt.OBJ, EXT):
        assert not any(f.startswith("control") for f in os.listdir(d))


if __name__ == "__main__":
    assert sys.argv[1] == "trace"
    json.dump(record(), sys.stdout)
