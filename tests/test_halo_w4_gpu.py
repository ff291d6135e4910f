"""Packed-W4 3x3 / stride 1 / pad 1 convs on the LDS-halo kernel (csrc/iconv.hip, the W4 instantiations):
bit-exact against the oracle on the unpacked integers, against the implicit-GEMM W4 launch and against the W8
halo launch, on every tile; the upsample fold; the range; the module and the fused graph."""
import numpy as np
import pytest
import torch

from tests import detdata as dd
from tests.test_host import Args, TINY, prepared, tiny_inputs
from tests.cases import MODULE_CASES, module_ckpt, module_input

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(params=["A", "B"], ids=["fma", "mul_add"])
def epilogue_variant(request, monkeypatch):
    """Both roundings of the epilogue's multiply-add (tests/test_ops_gpu.py): the operator tests take this fixture."""
    import mixdq_amd._C as C_
    monkeypatch.setattr(C_, "FLAGS", 1 if request.param == "B" else 0)
    return request.param


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def scal(v):
    return torch.tensor(float(v), dtype=torch.float32, device=DEV)


# n, h, w, c, k, bias, residual ("", "full", "image"), forced tile (0 = automatic), weights ("rand", "min", "max")
W4_HALO_CASES = [
    # tests/test_ops_gpu.py HALO_CASES, one for one
    (2, 16, 16, 320, 320, True, "", 0, "rand"),          # C = 2.5 chunks of 128, automatic
    (1, 16, 32, 128, 80, True, "full", 90, "rand"),      # 8 x 16 patches, one whole chunk, conv2's residual
    (1, 16, 16, 64, 72, False, "", 91, "rand"),          # half a chunk, N tail (72 < 80), 8 x 8 patches
    (2, 8, 16, 192, 168, True, "image", 90, "rand"),     # 1.5 chunks, N tail in the third tile, temb add
    (1, 8, 8, 448, 84, True, "full", 91, "rand"),        # a single patch: every pixel a border class; N % 8 == 4
    (1, 24, 48, 256, 160, False, "full", 0, "rand"),     # several patches per row / column, two chunks
    (3, 32, 32, 640, 96, True, "image", 0, "rand"),      # batch 3, five chunks
    (1, 16, 32, 320, 168, True, "full", 92, "rand"),     # 16 x 16 patches, 64-channel chunks (5 of them), N tail
    (2, 32, 16, 64, 80, False, "image", 92, "rand"),     # one chunk
    (1, 16, 16, 192, 72, True, "", 92, "rand"),          # a single all-border patch; the stage's zero-page slots
    (1, 32, 16, 320, 320, True, "full", 93, "rand"),     # 16 x 16 x 160 on 4 x 2 waves, two channel tiles
    (2, 16, 32, 128, 168, True, "image", 93, "rand"),    # N tail in the second channel tile (8 of 160)
    (1, 16, 16, 64, 72, False, "", 93, "rand"),          # N tail inside the first wave group; all-border patch
    (8, 32, 32, 64, 160, True, "full", 0, "rand"),       # automatic, batch 8
    # the tiles the list above does not force on these edges
    (1, 16, 16, 64, 84, True, "full", 90, "rand"),       # C = 64 on a 128-channel chunk; N % 8 == 4
    (2, 16, 16, 320, 84, True, "image", 92, "rand"),     # N % 8 == 4 on the 64-channel-chunk tile, batch 2
    (1, 16, 16, 320, 164, False, "full", 93, "rand"),    # N % 8 == 4 in the second channel tile of 160
    (3, 16, 16, 128, 40, True, "", 92, "rand"),          # N tail inside the first three fragments; batch 3
    (1, 32, 32, 64, 240, True, "image", 91, "rand"),     # 16 patches of 8 x 8, three channel tiles
    (8, 16, 16, 128, 320, True, "image", 93, "rand"),    # batch 8, forced 160-channel tile
    (1, 16, 32, 1280, 80, True, "", 90, "rand"),         # ten chunks
    (1, 16, 16, 320, 4, True, "", 91, "rand"),           # conv_out's 4 channels: off the automatic rule, forced
    (2, 16, 16, 64, 16, False, "full", 92, "rand"),
    # weight extremes: every nibble -8 (0x88 bytes; 16 q = -128 in the MFMA) and every nibble 7
    (2, 16, 16, 320, 168, True, "full", 0, "min"),
    (1, 16, 16, 128, 80, True, "", 90, "min"),
    (1, 16, 16, 192, 160, True, "image", 93, "max"),
    (1, 16, 16, 64, 72, False, "full", 92, "max"),
]


def _w4_conv_inputs(n, h, w_, c, k, has_bias, wmode):
    from mixdq_amd.nn.utils import pack_w4
    x = dd.int8(1901, (n, h, w_, c))
    if wmode == "rand":
        q = dd.int8(1902, (k, 3, 3, c), -8, 8)           # the whole 4-bit range [-8, 7]
        assert q.min() == -8 and q.max() == 7
    else:
        q = np.full((k, 3, 3, c), -8 if wmode == "min" else 7, dtype=np.int8)
    packed = pack_w4(torch.from_numpy(q))                # [K, 3, 3, C / 2]
    scale = dd.f32(1903, (k,), 1e-4, 6e-4)
    bias = dd.f16(1904, (k,), -1, 1) if has_bias else None
    return x, q, packed, scale, bias


def _case_id(c):
    return f"n{c[0]}_{c[1]}x{c[2]}_c{c[3]}_k{c[4]}_{c[6] or 'plain'}_t{c[7]}_{c[8]}"


@pytest.mark.parametrize("case", W4_HALO_CASES, ids=[_case_id(c) for c in W4_HALO_CASES])
def test_w4_halo_kernel_bit_exact(C, oracle, epilogue_variant, case):
    """The W4 halo launch == (a) the oracle on oracle.unpack_w4(packed) in the library's epilogue variant, (b) the
    implicit-GEMM W4 launch of the same arguments, (c) the W8 halo launch on the unpacked int8 weights."""
    n, h, w_, c, k, has_bias, res_kind, tile, wmode = case
    x, q, packed, scale, bias = _w4_conv_inputs(n, h, w_, c, k, has_bias, wmode)
    in_zp = -11.0
    unpacked = oracle.unpack_w4(packed.numpy())
    assert np.array_equal(unpacked, q)
    wsum = unpacked.astype(np.float32).sum(axis=3, dtype=np.float32)
    assert C.conv_halo_select(n, h, w_, c, k, 3, 3, 1, 1, w4=True) in ((90, 91, 92, 93) if k > 16 else (0,))
    tail = (t(scale), scal(1.0), scal(in_zp), t(scale), t(wsum.reshape(k, 1, 3, 3)), None,
            None if bias is None else t(bias), 1, 1)
    xin = t(x).permute(0, 3, 1, 2)
    w4in = packed.to(DEV).permute(0, 3, 1, 2)            # [K, C / 2, 3, 3], channels-last in memory
    w8in = t(unpacked).permute(0, 3, 1, 2)
    kw, add = {}, None
    if res_kind == "full":
        r = t(dd.normal_f16(1905, (n, h, w_, k), 2.0)).permute(0, 3, 1, 2)
        kw, add = dict(_residual=r), r
    elif res_kind == "image":
        r = t(dd.normal_f16(1906, (n, k), 2.0))
        kw, add = dict(_residual=r, _residual_per_image=True), r[:, :, None, None]
    got = C.qconv2d_w8_a8_ohalf(xin, w4in, *tail, _cfg=tile, _w4=True, **kw)
    want = torch.from_numpy(oracle.qconv2d(x, unpacked, scale, wsum, in_zp, None, bias, 1, 1, C.FLAGS & 1)
                            ).to(DEV).permute(0, 3, 1, 2)
    if add is not None:
        want = want + add                     # the epilogue add == a following torch half add
    assert torch.equal(got, want), f"W4 halo kernel != oracle: {int((got != want).sum())} elements"
    assert torch.equal(got, C.qconv2d_w8_a8_ohalf(xin, w4in, *tail, _cfg=4, _w4=True, **kw)), \
        "W4 halo != W4 implicit GEMM"
    assert torch.equal(got, C.qconv2d_w8_a8_ohalf(xin, w8in, *tail, _cfg=tile, **kw)), "W4 halo != W8 halo"


@pytest.mark.parametrize("n,h,w_,c,k,tile", [(2, 8, 8, 192, 168, 0), (1, 16, 8, 64, 80, 92), (1, 8, 8, 128, 168, 93),
                                             (1, 4, 8, 320, 72, 91), (3, 8, 16, 128, 96, 90), (1, 8, 8, 64, 84, 90),
                                             (2, 8, 16, 320, 160, 92), (1, 16, 16, 640, 320, 93), (2, 4, 4, 128, 40, 91)])
def test_w4_upsample2x_reads_the_small_tensor(C, epilogue_variant, n, h, w_, c, k, tile):
    """MIXDQ_FLAG_UPSAMPLE2X | MIXDQ_FLAG_W4: conv(nearest-2x-upsample(x)) from the [n, h, w] tensor == the W4 conv
    on the materialised upsampling (halo and implicit GEMM), bit for bit, on every tile."""
    from mixdq_amd.nn.utils import pack_w4
    x = t(dd.int8(1921, (n, h, w_, c))).permute(0, 3, 1, 2)
    q = dd.int8(1922, (k, 3, 3, c), -8, 8)
    w4in = pack_w4(torch.from_numpy(q)).to(DEV).permute(0, 3, 1, 2)
    scale = t(dd.f32(1923, (k,), 1e-4, 6e-4))
    bias = t(dd.f16(1924, (k,), -1, 1))
    wsum = t(q.astype(np.float32).sum(axis=3, dtype=np.float32).reshape(k, 1, 3, 3))
    args = (w4in, scale, scal(1.0), scal(7.0), scale, wsum, None, bias, 1, 1)
    assert C.conv_upsample2x_supported(tuple(x.shape), (k, c, 3, 3), 1, 1, w4=True)
    big = torch.nn.functional.interpolate(x.float(), scale_factor=2.0, mode="nearest").to(torch.int8
                                          ).contiguous(memory_format=torch.channels_last)
    want = C.qconv2d_w8_a8_ohalf(big, *args, _cfg=4, _w4=True)
    got = C.qconv2d_w8_a8_ohalf(x, *args, _cfg=tile, _w4=True, _upsample2x=True)
    assert got.shape == want.shape and torch.equal(got, want)
    assert torch.equal(got, C.qconv2d_w8_a8_ohalf(big, *args, _cfg=tile, _w4=True))
    with pytest.raises(RuntimeError, match="shape outside"):
        C.qconv2d_w8_a8_ohalf(x, *args, _cfg=4, _w4=True, _upsample2x=True)      # implicit-GEMM tile forced


def test_w4_halo_kernel_range(C):
    """The flags query answers for W4 exactly where the rule says (the W8 rule, but K <= 16 without 16 x 16 patches
    stays on the implicit-GEMM family: measured); outside the range the automatic choice is the implicit-GEMM family
    and a forced halo id still fails."""
    assert C.conv_halo_select(1, 128, 128, 320, 4, 3, 3, 1, 1) == 91
    assert C.conv_halo_select(1, 128, 128, 320, 4, 3, 3, 1, 1, w4=True) == 0
    assert C.conv_halo_select(8, 128, 128, 320, 4, 3, 3, 1, 1, w4=True) == 92
    for shape in [(1, 128, 128, 320, 320), (1, 64, 64, 640, 640), (1, 32, 32, 1280, 1280), (8, 128, 128, 320, 320),
                  (2, 16, 16, 320, 320), (1, 8, 8, 64, 72), (1, 64, 64, 1920, 640), (8, 32, 32, 2560, 1280)]:
        t8 = C.conv_halo_select(*shape, 3, 3, 1, 1)
        assert t8 != 0 and C.conv_halo_select(*shape, 3, 3, 1, 1, w4=True) == t8
    for w4 in (False, True):
        assert C.conv_halo_select(1, 12, 12, 960, 640, 3, 3, 1, 1, w4=w4) == 0      # H % 8 != 0
        assert C.conv_halo_select(1, 16, 16, 320, 320, 3, 3, 2, 1, w4=w4) == 0      # stride 2
        assert C.conv_halo_select(1, 16, 16, 320, 320, 1, 1, 1, 0, w4=w4) == 0      # 1x1
        assert C.conv_halo_select(1, 16, 16, 48, 320, 3, 3, 1, 1, w4=w4) == 0       # C % 64 != 0
        assert C.conv_halo_select(1, 16, 16, 96, 320, 3, 3, 1, 1, w4=w4) == 0
    # the nine-argument query: unchanged answers
    assert C.conv_halo_select(1, 128, 128, 320, 320, 3, 3, 1, 1) == 92
    assert C.conv_halo_select(8, 128, 128, 320, 320, 3, 3, 1, 1) == 93
    assert C.conv_halo_select(1, 32, 32, 1280, 1280, 3, 3, 1, 1) == 91
    v = torch.ones(16, device=DEV)
    ws = torch.ones(16, 1, 3, 3, device=DEV)
    for hw, c in ((12, 64), (16, 96)):                   # H % 8 != 0; C % 64 != 0 (a legal packed conv: C % 32 == 0)
        x = t(dd.int8(1911, (1, hw, hw, c))).permute(0, 3, 1, 2)
        w = t(dd.int8(1912, (16, 3, 3, c // 2))).permute(0, 3, 1, 2)
        for cfg in (90, 91, 92, 93):
            with pytest.raises(RuntimeError, match="shape outside"):
                C.qconv2d_w8_a8_ohalf(x, w, v, scal(1), scal(0), v, ws, None, None, 1, 1, _cfg=cfg, _w4=True)
        out = C.qconv2d_w8_a8_ohalf(x, w, v, scal(1), scal(0), v, ws, None, None, 1, 1, _w4=True)   # implicit GEMM
        assert out.shape == (1, 16, hw, hw)
    x = t(dd.int8(1913, (1, 8, 16, 64))).permute(0, 3, 1, 2)        # in range, but no 16-row patch fits
    w = t(dd.int8(1914, (16, 3, 3, 32))).permute(0, 3, 1, 2)
    for cfg in (92, 93):
        with pytest.raises(RuntimeError, match="shape outside"):
            C.qconv2d_w8_a8_ohalf(x, w, v, scal(1), scal(0), v, ws, None, None, 1, 1, _cfg=cfg, _w4=True)


def test_w4_conv_module_runs_on_the_halo_kernel(C, oracle, modules_golden):
    """QuantizedConv2d.from_float(..., w4_kernel=True) on a 3x3 conv: forward == the oracle's INT chain (quantize,
    conv) on the unpacked Path A integers; the upsample fold is offered; the launch is recorded as conv_halo*."""
    from mixdq_amd.nn import QuantizedConv2d
    c = next(m for m in MODULE_CASES if m["key"] == "conv_p1")          # 64 -> 96, 3x3, pad 1, 8 x 8 pixels
    fm = prepared(c, modules_golden, w_bit=4)
    fm.w4_kernel = True
    qm = QuantizedConv2d.from_float(fm, ckpt=module_ckpt(c, modules_golden)).to(DEV)
    assert qm.valid_for_acceleration and qm.w_packed4
    n, cin, h, w_ = c["xshape"]
    assert qm.upsample2x_supported((n, cin, h, w_)) is True
    assert qm.upsample2x_supported((n, cin, h + 1, w_)) is False        # 2 * (h + 1) = 18: H % 8 != 0
    x = module_input(c)
    saved = C.RECORD
    C.RECORD = []
    try:
        with torch.no_grad():
            y = qm(x.to(DEV))
        kinds = [e[0] for e in C.RECORD]
    finally:
        C.RECORD = saved
    assert [k for k in kinds if k.startswith("conv")] == [f"conv_halo{C.conv_halo_select(n, h, w_, cin, 96, 3, 3, 1, 1, w4=True)}"]
    variant = C.FLAGS & 1
    zp = float(qm.act_zero_points)
    xq = oracle.quantize(x.permute(0, 2, 3, 1).contiguous().numpy(), float(qm.act_scales_inv), zp, variant)
    wt = qm._weight_values().permute(0, 2, 3, 1).contiguous().cpu().numpy()          # [K, 3, 3, C] in [-8, 7]
    assert wt.min() >= -8 and wt.max() <= 7
    wsum = qm.weight_sum_by_input_channels.cpu().numpy().reshape(96, 3, 3)
    want = oracle.qconv2d(xq, wt, qm.scale.cpu().numpy(), wsum, zp, None, qm.bias.cpu().numpy(), 1, 1, variant)
    got = y.permute(0, 2, 3, 1).contiguous().cpu().numpy()
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
    # the fold, through the module: conv(upsample(x)) from the small quantized tensor
    from mixdq_amd.nn.Conv2d import quant_op
    with torch.no_grad():
        xd = x.to(DEV).contiguous(memory_format=torch.channels_last)
        folded = qm.forward_quantized(quant_op(xd, qm.act_scales_inv, qm.act_zero_points), upsample2x=True)
        plain = qm(torch.nn.functional.interpolate(xd, scale_factor=2.0, mode="nearest"))
    assert torch.equal(folded, plain)


TINY64 = dict(TINY, block_out_channels=(64, 128, 256), head_dim=64)


def _tiny_w4_unet(B, L):
    """tests/test_unet_gpu.py _tiny_quantized_gpu's pattern: every layer at 4 bits, w4_kernel=True."""
    from mixdq_amd.calib import calibrate, precompute_bos
    from mixdq_amd.quantize_sdxl import quantize_unet
    from mixdq_amd.unet import build_unet, quantizable_layers
    host = tiny_inputs(B=B, L=L)
    unet_c = build_unet("cpu", dtype=torch.float32, cfg=TINY64)
    with torch.no_grad():
        ckpt = calibrate(unet_c, [host])
        bos = {k: v.half().to(DEV) for k, v in precompute_bos(unet_c, host["encoder_hidden_states"]).items()}
    del unet_c
    unet = build_unet(DEV, cfg=TINY64)
    inp = dict(sample=host["sample"].half().to(DEV), timestep=host["timestep"].to(DEV),
               encoder_hidden_states=host["encoder_hidden_states"].half().to(DEV),
               added_cond_kwargs={k: v.half().to(DEV) for k, v in host["added_cond_kwargs"].items()})
    names = list(quantizable_layers(unet))
    quantize_unet(unet, Args({"model." + n: 4 for n in names}, {"model." + n: 8 for n in names}), ckpt, bos=True,
                  bos_dict=bos, w4_kernel=True)
    return unet, inp


def _slice(inp, lo, hi):
    return dict(sample=inp["sample"][lo:hi].contiguous(), timestep=inp["timestep"],
                encoder_hidden_states=inp["encoder_hidden_states"][lo:hi].contiguous(),
                added_cond_kwargs={k: v[lo:hi].contiguous() for k, v in inp["added_cond_kwargs"].items()})


def test_w4_unet_graph_runs_its_convs_on_the_halo_kernel(C, monkeypatch):
    """A small SDXL-shaped UNet, every layer 4-bit on the packed kernels, latent 32 (levels 32, 16, 8: H, W % 8 == 0
    everywhere): fused == de-fused == hipGraph replay, batch rows == single runs; every packed 3x3 / stride-1 /
    pad-1 conv with C % 64 == 0 is recorded on the halo kernel -- but conv_out, whose 4 output channels the W4 rule
    keeps on the implicit-GEMM family at this size --, each packed Upsample2D conv with the fold."""
    import mixdq_amd.unet as U
    from mixdq_amd.nn import QuantizedConv2d
    from mixdq_amd.quantize_sdxl import hip_graph_opt
    unet, inp = _tiny_w4_unet(B=2, L=32)
    convs = [m for m in unet.modules() if isinstance(m, QuantizedConv2d) and m.valid_for_acceleration and m.w_packed4]
    ups = [m for m in unet.modules() if isinstance(m, U.Upsample2D)]
    assert len(ups) == 2 and all(u.conv in convs for u in ups)
    n33 = sum(m.kernel_size == (3, 3) and m.stride == (1, 1) and m.in_channels % 64 == 0 for m in convs)
    assert n33 >= 20
    unet.set_fused(True)
    calls = []
    real = C.qconv2d_w8_a8_ohalf

    def spy(x_int, w, *a, **kw):
        out = real(x_int, w, *a, **kw)
        stride, pad = a[7], a[8]
        up = bool(kw.get("_upsample2x"))
        calls.append(dict(kind=C.RECORD[-1][0], w4=bool(kw.get("_w4")), up=up, rs=tuple(w.shape[2:]), stride=stride, k=w.shape[0],
                          pad=pad, c=x_int.shape[1], hw=tuple(s * (2 if up else 1) for s in x_int.shape[2:])))
        return out

    def halo_convs(cs):
        return [c for c in cs if c["w4"] and c["rs"] == (3, 3) and c["stride"] == 1 and c["pad"] == 1
                and c["c"] % 64 == 0 and c["hw"][0] % 8 == 0 and c["hw"][1] % 8 == 0]

    monkeypatch.setattr(C, "qconv2d_w8_a8_ohalf", spy)
    monkeypatch.setattr(C, "RECORD", [])
    with torch.no_grad():
        fused2 = unet(**inp)[0].clone()
        fused_calls, calls = calls, []
        with U.defused():
            ref2 = unet(**inp)[0].clone()
        defused_calls, calls = calls, []
    monkeypatch.setattr(C, "RECORD", None)
    monkeypatch.setattr(C, "qconv2d_w8_a8_ohalf", real)
    for cs in (fused_calls, defused_calls):
        in_range = halo_convs(cs)
        assert len(in_range) == n33, (len(in_range), n33)
        assert [c["k"] for c in in_range if c["k"] <= 16] == [4]          # conv_out: routed to the implicit GEMM
        in_range = [c for c in in_range if c["k"] > 16]
        assert all(c["kind"].startswith("conv_halo") for c in in_range), [c for c in in_range if c["kind"] == "conv"]
        assert all(c["kind"] == "conv" for c in cs if c not in in_range)
    assert sum(c["up"] for c in fused_calls) == 2 and sum(c["up"] for c in defused_calls) == 0
    assert torch.isfinite(fused2).all()
    assert torch.equal(fused2, ref2), f"fused != de-fused: {int((fused2 != ref2).sum())} elements"
    with torch.no_grad():
        for i in (0, 1):
            assert torch.equal(unet(**_slice(inp, i, i + 1))[0], fused2[i:i + 1]), f"row {i} != its batch-1 run"
    eager = unet.forward
    hip_graph_opt(unet)
    try:
        with torch.no_grad():
            g1 = unet(**inp)[0].clone()
            g2 = unet(**inp)[0].clone()
    finally:
        unet.forward = eager
    assert torch.equal(g1, fused2) and torch.equal(g2, fused2)
