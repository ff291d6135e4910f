"""4-bit activation quantizers on the INT8 kernels (a4_kernel=True, MIXDQ_FLAG_A4_*) on the host: the C-ABI
flags, QuantizedLinear's acceptance rules, the layer counts of a mixed-precision configuration, the quantizer
grouping of the fused graph and an A4 module's forward over oracle-backed ops."""
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests.test_host import Args, tiny_inputs, tiny_unet


def test_a4_flag_constants_match_header():
    import mixdq_amd._C as C
    hdr = open(__import__("os").path.join(__import__("os").path.dirname(__file__), "..", "include",
                                          "mixdq_hip.h")).read()
    got = {m.group(1): eval(m.group(2)) for m in re.finditer(r"MIXDQ_FLAG_(A4_\d) = ([0-9 <]+),?\n", hdr)}
    assert got == {"A4_0": 1 << 16, "A4_1": 1 << 17, "A4_2": 1 << 18}
    assert (C.FLAG_A4_0, C.FLAG_A4_1, C.FLAG_A4_2) == (got["A4_0"], got["A4_1"], got["A4_2"])
    assert C.FLAG_A4 == (C.FLAG_A4_0, C.FLAG_A4_1, C.FLAG_A4_2)
    assert "#define MIXDQ_ABI_VERSION 3" in hdr and C.ABI_VERSION == 3
    # no overlap with the forced-configuration byte (bits 8..15) or the other flags
    others = C.FLAG_W4 | C.FLAG_W2 | C.FLAG_UPSAMPLE2X | C.FLAG_A_ROWMAP | 1 | (0xff << 8)
    assert not (others & (C.FLAG_A4_0 | C.FLAG_A4_1 | C.FLAG_A4_2))
    assert C._aflag(8) == 0 and C._aflag(4) == C.FLAG_A4_0 and C._aflag(4, 2) == C.FLAG_A4_2
    with pytest.raises(RuntimeError):
        C._aflag(2)


def test_f16in_never_takes_an_a4_layer():
    import mixdq_amd._C as C
    x = torch.zeros(4, 64, dtype=torch.float16)       # (CPU tensor: False either way; the A4 rule comes first)
    assert C.qlinear_f16in_supported(x, 64, 64, abits=4) is False
    assert C.qlinear_f16in_wanted(x, 64, 64, abits=4) is False


def _ckpt(N, name, a_bits, a_zp=7.0, a_delta=0.05):
    """Kernel-format checkpoint of one Linear: int8 weight deltas; the activation quantizer's delta / zero point at
    index log2(a_bits) - 1 of the [2, 4, 8] stacks (nn/utils.get_quant_para shifts the zero point by -128)."""
    wd = torch.full((3, N), 0.01)
    ad, az = torch.full((3,), 0.02), torch.full((3,), 131.0)
    idx = {2: 0, 4: 1, 8: 2}[a_bits]
    ad[idx], az[idx] = a_delta, a_zp
    return {f"{name}.weight_quantizer": {"delta_list": wd, "zero_point_list": torch.zeros(3, N)},
            f"{name}.act_quantizer": {"delta_list": ad, "zero_point_list": az}}


def a4_linear(w_bits=8, a_bits=4, a4_kernel=True, w4_kernel=True, w2_kernel=True, K=128, N=64, seed=0,
              name="blk.attn2.to_out.0", half=False, bias=True):
    """A QuantizedLinear converted from a float nn.Linear with `w_bits` weights and an `a_bits` activation quantizer."""
    from torch.ao.quantization import PlaceholderObserver, QConfig
    from mixdq_amd.nn import QuantizedLinear
    from mixdq_amd.quantize_sdxl import BW_TO_DTYPE
    g = torch.Generator().manual_seed(seed)
    fm = nn.Linear(K, N, bias=bias)
    with torch.no_grad():
        fm.weight.copy_(torch.randn(N, K, generator=g) * 0.05)
        if bias:
            fm.bias.copy_(torch.randn(N, generator=g) * 0.1)
    fm.qconfig = QConfig(weight=PlaceholderObserver.with_args(dtype=BW_TO_DTYPE[w_bits]),
                         activation=PlaceholderObserver.with_args(dtype=BW_TO_DTYPE[a_bits]))
    fm.module_name = name
    fm.w_bit, fm.a_bit = w_bits, a_bits
    fm.w4_kernel, fm.w2_kernel, fm.a4_kernel = w4_kernel, w2_kernel, a4_kernel
    ckpt = _ckpt(N, name, a_bits)
    wd = fm.weight.detach().abs().amax(dim=1) / (2 ** (w_bits - 1) - 1 if w_bits == 8 else 2 ** (w_bits - 1))
    ckpt[f"{name}.weight_quantizer"]["delta_list"][{2: 0, 4: 1, 8: 2}[w_bits]] = wd
    if half:
        fm.half()
    return fm, QuantizedLinear.from_float(fm, ckpt=ckpt)


@pytest.mark.parametrize("w_bits,name,store", [(8, "QuantizedLinearW8A4", "weight_int"),
                                               (4, "QuantizedLinearW4A4", "weight_int4"),
                                               (2, "QuantizedLinearW2A4", "weight_int2")])
def test_from_float_accepts_a4_layers_with_a4_kernel(w_bits, name, store):
    _, m = a4_linear(w_bits)
    assert m.valid_for_acceleration and m.act_bits == 4 and m._get_name() == name
    assert hasattr(m, store)
    # the 4-bit quantizer of the checkpoint (index 1 of the stacks), zero point shifted by -128
    assert torch.equal(m.act_scales, torch.tensor(0.05)) and torch.equal(m.act_zero_points, torch.tensor(7.0 - 128))
    assert torch.equal(m.bias0, m.weight_sum_by_input_channels * m.act_zero_points)


def test_without_a4_kernel_a4_layers_keep_the_fp16_fallback_and_todays_buffers():
    fm, m = a4_linear(8, a4_kernel=False)
    assert not m.valid_for_acceleration and m._get_name() == "QuantizedLinearFPFallback" and m.act_bits == 8
    assert sorted(n for n, _ in m.named_buffers()) == ["bias", "weight"]
    assert torch.equal(m.weight, fm.weight.detach())
    # the class default is off; a per-module attribute or quantize_unet turns it on
    from mixdq_amd.nn import QuantizedLinear
    assert QuantizedLinear.a4_kernel is False
    # an 8-bit activation layer is byte-for-byte the same with or without the flag
    _, m8a = a4_linear(8, a_bits=8, a4_kernel=True)
    _, m8b = a4_linear(8, a_bits=8, a4_kernel=False)
    assert m8a._get_name() == m8b._get_name() == "QuantizedLinearW8A8" and m8a.act_bits == 8
    sa, sb = m8a.state_dict(), m8b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)


def test_a4_weight_rules_follow_the_weight_flags():
    _, m = a4_linear(4, w4_kernel=False)                   # a 4-bit weight needs w4_kernel
    assert not m.valid_for_acceleration
    _, m = a4_linear(2, w4_kernel=False, w2_kernel=True)   # a 2-bit weight qualifies through w2_kernel alone
    assert m.valid_for_acceleration and m.w_packed2 and m.act_bits == 4
    _, m = a4_linear(2, w4_kernel=False, w2_kernel=False)
    assert not m.valid_for_acceleration
    _, m = a4_linear(8, a_bits=2)                          # other activation widths stay FP16
    assert not m.valid_for_acceleration


def test_a4_conv_stays_fp16():
    """QuantizedConv2d is out of scope: a conv with a 4-bit activation quantizer keeps the FP16 fallback."""
    from torch.ao.quantization import PlaceholderObserver, QConfig
    from mixdq_amd.nn import QuantizedConv2d
    fm = nn.Conv2d(32, 32, 3, 1, 1)
    fm.qconfig = QConfig(weight=PlaceholderObserver.with_args(dtype=torch.qint8),
                         activation=PlaceholderObserver.with_args(dtype=torch.quint4x2))
    fm.module_name, fm.w_bit, fm.a_bit, fm.a4_kernel = "conv", 8, 4, True
    ckpt = _ckpt(32, "conv", 4)
    m = QuantizedConv2d.from_float(fm, ckpt=ckpt)
    assert not m.valid_for_acceleration


def _inventory_counts(a4):
    from mixdq_amd import cfgs
    from mixdq_amd.nn import QuantizedConv2d, QuantizedLinear
    from mixdq_amd.nn.utils import QParam
    from mixdq_amd.quantize_sdxl import BW_TO_DTYPE
    from mixdq_amd.unet import SDXLUNet, quantizable_layers
    with torch.device("meta"):
        inv = quantizable_layers(SDXLUNet())
    w, a = cfgs.load("weight/weight_4.00"), cfgs.load("act/act_7.77")
    lin = conv = 0
    for name, m in inv.items():
        wb, ab = w[name], a.get(name)
        n_out = m.out_features if isinstance(m, nn.Linear) else m.out_channels
        wq = QParam(torch.per_channel_affine, BW_TO_DTYPE[wb], torch.ones(n_out), torch.zeros(n_out), 0)
        aq = None if ab is None else QParam(torch.per_tensor_affine, BW_TO_DTYPE[ab], torch.tensor(0.1),
                                            torch.tensor(-120.0), 0)
        if isinstance(m, nn.Linear):
            q = QuantizedLinear(m.in_features, m.out_features, device="cpu", w_qparams=wq, a_qparams=aq,
                                w4_kernel=wb in (2, 4), w2_kernel=wb == 2, w_bit=wb, a4_kernel=a4, a_bit=ab)
            lin += q.valid_for_acceleration
            assert not q.valid_for_acceleration or q.act_bits == (ab if a4 else 8)
        else:
            split = getattr(m, "split", 0)
            q = QuantizedConv2d(m.in_channels, m.out_channels, m.kernel_size, m.stride, m.padding, m.dilation,
                                device="cpu", w_qparams=wq, w_qparams_0=wq if split else None, a_qparams=aq,
                                a_qparams_0=aq if split else None, split=split, w4_kernel=wb in (2, 4))
            conv += q.valid_for_acceleration
    return lin, conv


def test_layer_counts_weight_4_act_7_77():
    """SDXL inventory, weight_4.00 + act_7.77 with w4_kernel + w2_kernel: 719 accelerated layers (672 Linears + 47
    convs) without a4_kernel, 785 -- every layer with an activation quantizer -- with it: the 66 Linears with a
    4-bit activation quantizer (attn2.to_q / to_v / to_out.0)."""
    assert _inventory_counts(False) == (672, 47)
    assert _inventory_counts(True) == (738, 47)


def test_quantizer_identity_includes_the_width():
    """_quantizer_groups / _same_qparams: equal tensors but different widths are different quantizers."""
    from mixdq_amd.unet import _quantizer_groups, _same_qparams

    class L:
        def __init__(self, bits):
            self.act_scales_inv, self.act_zero_points = torch.tensor(20.0), torch.tensor(-120.0)
            if bits != 8:
                self.act_bits = bits
    a8, b8, a4, b4 = L(8), L(8), L(4), L(4)
    assert _quantizer_groups({}, "k", [a8, b8, a4, b4]) == [0, 0, 1, 1]
    assert _same_qparams(a8, b8) and _same_qparams(a4, b4) and not _same_qparams(a8, a4)
    memo = {}
    assert _quantizer_groups(memo, "k", [a8, b8]) == [0, 0]
    b8.act_bits = 4                                          # a width change invalidates the memo
    assert _quantizer_groups(memo, "k", [a8, b8]) == [0, 1]


def test_tagged_operand_matches_the_width():
    """swap_glue: an operand attached for an 8-bit quantizer is never handed to a 4-bit layer with the same buffers."""
    from mixdq_amd.nn.glue import _attach, tagged_operand

    class L:
        valid_for_acceleration = True
        in_features = 8

        def __init__(self, s, z, bits=8):
            self.act_scales_inv, self.act_zero_points, self.act_bits = s, z, bits
    s, z = torch.tensor(20.0), torch.tensor(-120.0)
    l8, l4 = L(s, z), L(s, z, 4)
    y, q = torch.zeros(2, 8), torch.zeros(2, 8, dtype=torch.int8)
    _attach(y, [l8], [q])
    assert tagged_operand(y, l8) is q and tagged_operand(y, l4) is None
    y2 = torch.zeros(2, 8)
    _attach(y2, [l4], [q])
    assert tagged_operand(y2, l4) is q and tagged_operand(y2, l8) is None


def test_a4_forward_over_oracle_ops(monkeypatch):
    """The plain and BOS forwards of an A4 layer pass _abits=4 to every quantize they issue; with the oracle standing
    in for the kernels the result is the 4-bit INT chain."""
    import mixdq_amd.nn.Linear as L
    from oracle import oracle
    seen = []

    def quant(x, s_inv, zp, _abits=8):
        seen.append(_abits)
        q = oracle.quantize(x.contiguous().numpy(), float(s_inv), float(zp))
        if _abits == 4:
            q = np.minimum(q, -113).astype(np.int8)
        return torch.from_numpy(q)

    def qlin(x_int, w, wscale, ascale, azp, wsum, scale, bias0, bias=None, _out=None, _row_map=None,
             _residual=None, _w4=False, _w2=False):
        from mixdq_amd.nn.utils import unpack_w2
        if _w4:
            w = torch.from_numpy(oracle.unpack_w4(w.contiguous().numpy()))
        if _w2:
            w = unpack_w2(w)
        D = oracle.qlinear(x_int.reshape(-1, x_int.shape[-1]).contiguous().numpy(), w.numpy(), bias0.numpy(),
                           scale.numpy(), None if bias is None else bias.numpy())
        y = torch.from_numpy(D).reshape(*x_int.shape[:-1], -1)
        if _out is not None:
            _out[:, 1:, :] = y
            return _out
        return y
    monkeypatch.setattr(L, "quant_op", quant)
    monkeypatch.setattr(L, "qlinear", qlin)
    fm, m = a4_linear(2, K=128, N=64, half=True)
    x = (torch.randn(1, 6, 128, generator=torch.Generator().manual_seed(5)) * 1.5).half()
    y = m(x)
    assert seen == [4]
    q = quant(x, m.act_scales_inv, m.act_zero_points, _abits=4)
    assert int(q.max()) <= -113 and int(q.min()) >= -128
    D = oracle.qlinear(q.reshape(-1, 128).numpy(), m._weight_values().numpy(), m.bias0.numpy(), m.scale.numpy(),
                       m.bias.numpy())
    assert np.array_equal(y.reshape(-1, 64).numpy().view(np.uint16), D.view(np.uint16))
    # BOS path (attn2.to_v): tokens 1.. quantized with the 4-bit clamp
    seen.clear()
    m.bos = True
    m.register_buffer("bos_pre_computed", torch.zeros(1, 1, 64, dtype=torch.float16))
    yb = m(x)
    assert seen == [4] and torch.equal(yb[:, 0], torch.zeros(1, 64, dtype=torch.float16))
    assert np.array_equal(yb[:, 1:].reshape(-1, 64).numpy().view(np.uint16),
                          D.reshape(6, 64)[1:].view(np.uint16))


def test_quantize_unet_a4_kernel_flags_only_a4_linears(monkeypatch):
    """quantize_unet(..., a4_kernel=True) marks the float Linears whose activation quantizer is 4-bit."""
    import mixdq_amd.quantize_sdxl as Q
    unet = tiny_unet()
    lin = [m for m in unet.modules() if isinstance(m, nn.Linear)]
    conv = [m for m in unet.modules() if isinstance(m, nn.Conv2d)]
    marks = {}
    monkeypatch.setattr(Q, "convert_to_quantized", lambda u, ck: marks.update(
        {id(m): getattr(m, "a4_kernel", False) for m in u.modules()}))

    def reg(u, args, bos, bos_dict):
        for m in lin[:3] + conv[:1]:
            m.a_bit = 4
        for m in lin[3:5]:
            m.a_bit = 8
    monkeypatch.setattr(Q, "register_qconfig_from_input_files", reg)
    Q.quantize_unet(unet, Args(None, None), None, None, None, a4_kernel=True)
    assert [marks[id(m)] for m in lin[:5]] == [True, True, True, False, False]
    assert marks[id(conv[0])] is False
