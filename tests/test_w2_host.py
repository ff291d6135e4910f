"""Packed-W2 storage (MIXDQ_FLAG_W2) on the host: the pack layout, QuantizedLinear's W2 storage, the
group unification of set_fused, the C-ABI queries and a W2 module's forward over oracle-backed ops."""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_host import Args, tiny_inputs, tiny_unet


def _rand_w2(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2, 2, shape, generator=g, dtype=torch.int64).to(torch.int8)


def test_pack_w2_round_trip_covers_every_value():
    from mixdq_amd.nn.utils import pack_w2, unpack_w2
    for shape in [(1, 64), (3, 128), (5, 7, 192), (17, 640)]:
        q = _rand_w2(shape, seed=shape[-1])
        p = pack_w2(q)
        assert p.dtype == torch.int8 and p.shape == (*shape[:-1], shape[-1] // 4)
        assert torch.equal(unpack_w2(p), q)
    every = torch.tensor([-2, -1, 0, 1], dtype=torch.int8).repeat(16)[None]   # every value at every crumb
    assert torch.equal(unpack_w2(pack_w2(every)), every)
    assert torch.equal(unpack_w2(pack_w2(every.roll(1, -1))), every.roll(1, -1))


def test_pack_w2_byte_layout_is_crumb_planar_per_16():
    """Byte j of each 16-k group's dword: k[j] in bits 7:6, k[4+j] in 5:4, k[8+j] in 3:2, k[12+j] in 1:0."""
    from mixdq_amd.nn.utils import pack_w2
    q = torch.zeros(1, 64, dtype=torch.int8)
    q[0, 0], q[0, 4], q[0, 8], q[0, 12] = -2, 1, -1, 0       # byte 0 of group 0
    q[0, 3], q[0, 15] = 1, -1                                # byte 3 of group 0: bits 7:6 = 01, 1:0 = 11
    q[0, 16 + 1] = -1                                        # byte 1 of group 1: bits 7:6 = 11
    p = pack_w2(q).view(torch.uint8)[0].tolist()
    expect = [0] * 16
    expect[0] = (0b10 << 6) | (0b01 << 4) | (0b11 << 2) | 0b00
    expect[3] = (0b01 << 6) | 0b11
    expect[4 + 1] = 0b11 << 6
    assert p == expect
    # the kernel's unpack (csrc/igemm_kernel.h): r_i = (w << 2i) & 0xC0C0C0C0 = 64 * q in natural k order
    w = int.from_bytes(bytes(pack_w2(_rand_w2((1, 64), 3)).view(torch.uint8)[0, :4].tolist()), "little")
    vals = _rand_w2((1, 64), 3)[0, :16].tolist()
    got = []
    for i in range(4):
        r = ((w << (2 * i)) & 0xC0C0C0C0).to_bytes(8, "little")[:4]
        got += [int(np.int8(np.uint8(b))) // 64 for b in r]
    assert got == vals


def test_pack_w2_refuses_out_of_range_and_ragged_k():
    from mixdq_amd.nn.utils import pack_w2
    with pytest.raises(ValueError):
        pack_w2(torch.full((2, 64), 2, dtype=torch.int8))
    with pytest.raises(ValueError):
        pack_w2(torch.full((2, 64), -3, dtype=torch.int8))
    with pytest.raises(ValueError):
        pack_w2(torch.zeros(2, 96, dtype=torch.int8))
    with pytest.raises(ValueError):
        pack_w2(torch.zeros(2, 64, dtype=torch.int16))


def _ckpt(N, delta, bits, name="blk.ff.net.2"):
    """Kernel-format checkpoint of one Linear (nn/utils.get_quant_para): per-bit-width stacks [2, 4, 8],
    the layer's per-channel weight delta at `bits`, a per-tensor activation quantizer."""
    idx = {2: 0, 4: 1, 8: 2}[bits]
    wd = torch.ones(3, N)
    wd[idx] = delta
    return {f"{name}.weight_quantizer": {"delta_list": wd, "zero_point_list": torch.zeros(3, N)},
            f"{name}.act_quantizer": {"delta_list": torch.full((3,), 0.02),
                                      "zero_point_list": torch.full((3,), 131.0)}}


def _two_bit_linear(w2_kernel=True, w4_kernel=False, K=128, N=64, bias=True, seed=0, half=False):
    """A QuantizedLinear converted from a float nn.Linear with 2-bit quint4x2 weights (per-channel deltas)."""
    import torch.nn as nn
    from torch.ao.quantization import PlaceholderObserver, QConfig
    from mixdq_amd.nn import QuantizedLinear
    g = torch.Generator().manual_seed(seed)
    fm = nn.Linear(K, N, bias=bias)
    with torch.no_grad():
        fm.weight.copy_(torch.randn(N, K, generator=g) * 0.05)
        if bias:
            fm.bias.copy_(torch.randn(N, generator=g) * 0.1)
    fm.qconfig = QConfig(weight=PlaceholderObserver.with_args(dtype=torch.quint4x2),
                         activation=PlaceholderObserver.with_args(dtype=torch.qint8))
    fm.module_name = "blk.ff.net.2"
    fm.w_bit, fm.a_bit = 2, 8
    fm.w2_kernel, fm.w4_kernel = w2_kernel, w4_kernel
    delta = fm.weight.detach().abs().amax(dim=1) / 2
    ckpt = _ckpt(N, delta, bits=2)
    if half:
        fm.half()
    return fm, QuantizedLinear.from_float(fm, ckpt=ckpt), delta


def test_from_float_stores_two_bit_layers_packed_with_w2_kernel():
    fm, m, delta = _two_bit_linear()
    assert m.valid_for_acceleration and m.w_packed2 and not m.w_packed4
    assert m._get_name() == "QuantizedLinearW2A8"
    assert m.weight_int2.shape == (64, 128 // 4) and m.weight_int2.dtype == torch.int8
    assert not hasattr(m, "weight_int4") and not hasattr(m, "weight_int")
    expect = torch.clamp(torch.round(fm.weight.detach().float() / m.weight_scales[:, None]), -2, 1).to(torch.int8)
    assert torch.equal(m._weight_values(), expect)
    assert torch.allclose(m.weight_scales, delta)
    assert torch.equal(m.weight_sum_by_input_channels, expect.float().sum(1))


def test_without_w2_kernel_two_bit_layers_keep_todays_storage():
    _, m4, _ = _two_bit_linear(w2_kernel=False, w4_kernel=True)
    assert m4.w_packed4 and not m4.w_packed2 and m4._get_name() == "QuantizedLinearW4A8"
    _, m2, _ = _two_bit_linear(w2_kernel=True, w4_kernel=True)
    assert torch.equal(m2._weight_values(), m4._weight_values())
    assert torch.equal(m2.bias0, m4.bias0) and torch.equal(m2.scale, m4.scale)
    _, mf, _ = _two_bit_linear(w2_kernel=False, w4_kernel=False)
    assert not mf.valid_for_acceleration                    # the reference's FP16 fallback, as today
    # K % 64 != 0: W2 cannot take the layer; w4_kernel decides as before
    _, mk, _ = _two_bit_linear(w2_kernel=True, w4_kernel=True, K=96)
    assert mk.w_packed4 and not mk.w_packed2


def test_misaligned_two_bit_layer_is_an_fp_fallback_without_w2_storage():
    _, m, _ = _two_bit_linear(w2_kernel=True, N=62)            # out_features % 4 != 0
    assert not m.valid_for_acceleration and not m.w_packed2 and not hasattr(m, "weight_int2")
    assert m._get_name() == "QuantizedLinearFPFallback"


def test_w2_kernel_leaves_four_and_eight_bit_layers_alone():
    import torch.nn as nn
    from torch.ao.quantization import PlaceholderObserver, QConfig
    from mixdq_amd.nn import QuantizedLinear
    for bits, dt in ((4, torch.quint4x2), (8, torch.qint8)):
        fm = nn.Linear(128, 64)
        fm.qconfig = QConfig(weight=PlaceholderObserver.with_args(dtype=dt),
                             activation=PlaceholderObserver.with_args(dtype=torch.qint8))
        fm.module_name = "blk.ff.net.2"
        fm.w_bit, fm.a_bit, fm.w2_kernel, fm.w4_kernel = bits, 8, True, True
        delta = fm.weight.detach().abs().amax(dim=1) / (2 ** (bits - 1) - 1)
        ckpt = _ckpt(64, delta, bits=bits)
        m = QuantizedLinear.from_float(fm, ckpt=ckpt)
        assert not m.w_packed2 and m.w_packed4 == (bits == 4)


def test_w2_state_dict_round_trip():
    _, m, _ = _two_bit_linear(seed=5)
    sd = m.state_dict()
    assert "weight_int2" in sd and "weight_int4" not in sd
    _, m2, _ = _two_bit_linear(seed=6)
    m2.load_state_dict(sd)
    assert torch.equal(m2.weight_int2, m.weight_int2) and torch.equal(m2._weight_values(), m._weight_values())


def test_w2_forward_on_oracle_ops_equals_w4_storage(oracle_ops_w2):
    _, m2, _ = _two_bit_linear(w2_kernel=True, seed=2)
    _, m4, _ = _two_bit_linear(w2_kernel=False, w4_kernel=True, seed=2)
    x = (torch.randn(2, 5, 128, generator=torch.Generator().manual_seed(1)) * 0.5).half()
    y2, y4 = m2(x), m4(x)
    assert y2.dtype == torch.float16 and torch.equal(y2, y4)


@pytest.fixture
def oracle_ops_w2(monkeypatch, oracle):
    """Oracle stand-ins for quantize and the GEMM (test-only), which unpack either storage."""
    import mixdq_amd.nn.Linear as L
    from mixdq_amd.nn.utils import unpack_w2

    def quant(x, s_inv, zp):
        return torch.from_numpy(oracle.quantize(x.numpy(), float(s_inv), float(zp)))

    def qlin(x_int, w, ws, a_s, a_zp, wsum, scale, bias0, bias=None, _out=None, _row_map=None,
             _residual=None, _residual_div=1, _cfg=0, _w4=False, _w2=False):
        assert _out is None and _row_map is None and _residual is None
        if _w4:
            w = torch.from_numpy(oracle.unpack_w4(w.contiguous().numpy()))
        if _w2:
            w = unpack_w2(w)
        x2 = x_int.reshape(-1, x_int.shape[-1]).contiguous().numpy()
        D = oracle.qlinear(x2, w.numpy(), bias0.numpy(), scale.numpy(), None if bias is None else bias.numpy())
        return torch.from_numpy(D).reshape(*x_int.shape[:-1], -1)

    monkeypatch.setattr(L, "quant_op", quant)
    monkeypatch.setattr(L, "qlinear", qlin)


# ------------------------------------------------------------------ group unification (set_fused)
def _tiny_mixed(bits_of):
    from mixdq_amd.calib import calibrate, precompute_bos
    from mixdq_amd.quantize_sdxl import quantize_unet
    from mixdq_amd.unet import quantizable_layers
    unet = tiny_unet()
    inp = tiny_inputs()
    ckpt = calibrate(unet, [inp])
    bos = precompute_bos(unet.half(), inp["encoder_hidden_states"].half())
    names = list(quantizable_layers(unet))
    quantize_unet(unet, Args({"model." + n: bits_of(n) for n in names}, {"model." + n: 8 for n in names}),
                  ckpt, bos=True, bos_dict=bos, w4_kernel=True, w2_kernel=True)
    return unet


def test_group_unification_of_two_bit_members_happens_in_set_fused_only():
    import mixdq_amd.unet as U

    def bits(n):
        if n.endswith("attn1.to_q"):
            return 2                                    # {2, 4, 4} q|k|v -> W4
        if n.endswith("attn1.to_k") or n.endswith("attn1.to_v"):
            return 4
        if n.endswith("attn2.to_k"):
            return 2                                    # {2, 8} k|v -> int8
        if n.endswith("attn2.to_q") or n.endswith("attn2.to_out.0") or n.endswith("ff.net.2"):
            return 2                                    # single layers stay W2
        return 8
    unet = _tiny_mixed(bits)
    blk = next(m for m in unet.modules() if isinstance(m, U.BasicTransformerBlock))
    a1, a2 = blk.attn1, blk.attn2
    assert a1.to_q.w_packed2 and a1.to_k.w_packed4 and a2.to_k.w_packed2 and not a2.to_v.w_packed4
    assert a2.to_q.w_packed2 and blk.ff.net[2].w_packed2
    keys0 = sorted(unet.state_dict())
    assert blk._qkv_fused() is None and U.SDXLUNet._kv_pack(blk) is None      # pure queries
    assert sorted(unet.state_dict()) == keys0
    q_vals, k_vals = a1.to_q._weight_values().clone(), a2.to_k._weight_values().clone()
    unet.set_fused(True)
    keys1 = sorted(unet.state_dict())
    assert keys1 != keys0
    assert a1.to_q.w_packed4 and not a1.to_q.w_packed2 and torch.equal(a1.to_q._weight_values(), q_vals)
    assert not a2.to_k.w_packed2 and not a2.to_k.w_packed4 and torch.equal(a2.to_k.weight_int, k_vals)
    assert a2.to_q.w_packed2 and blk.ff.net[2].w_packed2                   # not in a group: unchanged
    assert blk._qkv_fused() is not None and U.SDXLUNet._kv_pack(blk) is not None
    unet.set_fused(True)
    assert sorted(unet.state_dict()) == keys1


def test_uniform_two_bit_group_stays_packed():
    import mixdq_amd.unet as U
    unet = _tiny_mixed(lambda n: 2 if ("attn1.to_" in n and not n.endswith("to_out.0")) else 8)
    blk = next(m for m in unet.modules() if isinstance(m, U.BasicTransformerBlock))
    keys0 = sorted(unet.state_dict())
    unet.set_fused(True)
    assert sorted(unet.state_dict()) == keys0
    assert all(m.w_packed2 for m in (blk.attn1.to_q, blk.attn1.to_k, blk.attn1.to_v))
    pack = blk._qkv_fused()
    assert pack is not None and pack["wbits"] == 2 and pack["w"].shape[1] == blk.attn1.to_q.in_features // 4


# ------------------------------------------------------------------ C-ABI
def _lib():
    from mixdq_amd import build
    lib = ctypes.CDLL(build.LIB)
    lib.mixdq_igemm_select_id_w2.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.mixdq_igemm_select_id_w2.restype = ctypes.c_int
    lib.mixdq_igemm_select_id_geglu_w2.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_int]
    lib.mixdq_igemm_select_id_geglu_w2.restype = ctypes.c_int
    lib.mixdq_status_string.argtypes = [ctypes.c_int]
    lib.mixdq_status_string.restype = ctypes.c_char_p
    lib.mixdq_abi_version.restype = ctypes.c_int
    return lib


# the UNet's 2-bit Linear families (N, K) at 1024 px: M = 77 context rows, 1024 / 4096 tokens, x batch
W2_SHAPES = [(640, 2048), (1280, 2048), (640, 640), (1280, 1280), (10240, 1280), (1280, 5120), (5120, 640),
             (640, 2560)]


def test_cabi_w2_queries():
    lib = _lib()
    assert lib.mixdq_abi_version() == 3
    bad = (27, 42, 43, 44, 45, 56)
    for N, K in W2_SHAPES:
        for M in (77, 154, 616, 1024, 4096, 8192, 32768):
            c = lib.mixdq_igemm_select_id_w2(M, N, K, K)
            assert c > 0 and c not in bad, (M, N, K, c)
            if N % 32 == 0:
                g = lib.mixdq_igemm_select_id_geglu_w2(M, N, K)
                assert g > 0 and g not in bad, (M, N, K, g)
    assert lib.mixdq_igemm_select_id_w2(1024, 640, 96, 96) == -1
    assert lib.mixdq_igemm_select_id_w2(1024, 640, 32, 32) == -1
    assert lib.mixdq_igemm_select_id_geglu_w2(1024, 640, 96) == -1
    assert b"K % 64" in lib.mixdq_status_string(10)


def test_python_select_and_f16in_report_w2():
    from mixdq_amd import _C
    assert _C.FLAG_W2 == 16 and _C.FLAG_W4 == 2
    for N, K in W2_SHAPES:
        c = _C.igemm_select_id(4096, N, K, K, w2=True)
        assert c > 0 and c not in _C.W2_INADMISSIBLE
    with pytest.raises(RuntimeError):
        _C.igemm_select_id(4096, 640, 640, w4=True, w2=True)
    x = torch.zeros(4, 640, dtype=torch.float16)
    assert _C.qlinear_f16in_supported(x, 640, 640, w2=True) is False
    assert _C.qlinear_f16in_wanted(x, 640, 640, w2=True) is False


def test_record_entries_keep_the_four_tuple_and_carry_wbits():
    from mixdq_amd import _C
    saved = _C.RECORD
    _C.RECORD = []
    try:
        _C._record("linear", 1, 64, 128, 128, False, lambda: None, (), {}, w2=True)
        _C._record("linear", 1, 64, 128, 128, True, lambda: None, (), {})
        (k0, dims0, w40, _), (k1, _, w41, _) = _C.RECORD
        assert dims0 == (1, 64, 128, 128) and w40 is False and w41 is True
        assert [e.wbits for e in _C.RECORD] == [2, 4]
    finally:
        _C.RECORD = saved
