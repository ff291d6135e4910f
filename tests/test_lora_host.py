"""Host side of the LoRA launch: table order and prefix, the conv factor permutation, every refusal (nothing is launched)."""
import ctypes

import numpy as np
import pytest
import torch

import mixdq_amd._C as C

OK, INVALID, SHAPE = 0, 1, 9


def test_table_longest_rows_first_and_prefix():
    layers = [C.LoraLayer(N=40, Kf=36), C.LoraLayer(N=17, Kf=96), C.LoraLayer(N=16, Kf=36), C.LoraLayer(N=1, Kf=640)]
    order, prefix, grid = C.lora_order(layers)
    assert order == [3, 1, 0, 2]                               # largest Kf first, ties in table order
    assert prefix == [0, 1, 3, 6, 7] and grid == 7             # ceil(N / 16) workgroups each
    assert ctypes.sizeof(C.LoraLayer) == 136                  # struct mixdq_lora_layer
    with pytest.raises(RuntimeError):
        C.lora_order([C.LoraLayer(N=0, Kf=36)])


def test_conv_factor_is_permuted_to_stored_order():
    from mixdq_amd.lora import conv_factor_stored
    g = torch.Generator().manual_seed(0)
    A, w = torch.randn(4, 6, 3, 3, generator=g), torch.randn(5, 6, 3, 3, generator=g)
    stored_w = w.permute(0, 2, 3, 1).reshape(5, -1)            # the layer's [N, R*S*C] memory
    want = torch.einsum("nk,rk->nr", stored_w, conv_factor_stored(A))
    assert torch.allclose(want, torch.einsum("ncij,rcij->nr", w, A), atol=1e-5)


def _valid(buf, **over):
    p = buf.ctypes.data
    d = dict(W=p, Bcat=p, Acat=p, svec=p, out=p, weight_scales=p, scale=p, act_scale=p, act_zero_point=p, ldw=64, w_col0=0,
             N=16, Kf=64, R=32, mode=C.LORA_INT8, rule=C.LORA_KEEP, bits=8, tap_len=64)
    d.update(over)
    return C.LoraLayer(**d)


@pytest.mark.parametrize("over,status", [
    ({}, OK), ({"R": 48}, SHAPE), ({"R": 288}, SHAPE), ({"R": 0}, SHAPE), ({"Kf": 38, "tap_len": 38}, SHAPE),
    ({"mode": C.LORA_W4, "bits": 4, "Kf": 48, "tap_len": 48}, SHAPE), ({"mode": C.LORA_W2, "bits": 2}, SHAPE),
    ({"ldw": 66}, SHAPE), ({"w_col0": 2}, SHAPE), ({"tap_len": 24}, SHAPE), ({"tap_len": 4, "Kf": 128}, SHAPE),
    ({"W": 4}, SHAPE), ({"out": 8}, SHAPE), ({"scale": 2}, SHAPE), ({"row_map": 2}, SHAPE),
    ({"W": None}, INVALID), ({"scale": None}, INVALID), ({"mode": 7}, INVALID), ({"bits": 3}, INVALID), ({"N": 0}, INVALID),
    ({"mode": C.LORA_F16, "scale": None, "weight_scales": None}, OK)])
def test_refusals(over, status):
    buf = np.zeros(64, np.float64)                             # 16-byte aligned host memory: only looked at
    base = buf.ctypes.data
    over = {k: (base + v if k in ("W", "out", "scale", "row_map") and v is not None else v) for k, v in over.items()}
    assert C.lora_status([_valid(buf, **over)]) == status
    assert C.lora_status([]) == INVALID


def _stub(**attrs):
    """A one-layer 'UNet' on the CPU: a W8A8 QuantizedLinear `blk.to_q` [16, 32] quantized from `w` as from_float does."""
    from mixdq_amd.nn import QuantizedLinear
    from mixdq_amd.nn.utils import QParam
    w = torch.randn(16, 32, generator=torch.Generator().manual_seed(1)).half()
    sc, z = w.float().abs().amax(1) / 127, torch.zeros(16)
    lin = QuantizedLinear(32, 16, bias=False, device="cpu", module_name="blk.to_q",
                          w_qparams=QParam(torch.per_channel_affine, torch.qint8, sc, z, 0),
                          a_qparams=QParam(torch.per_tensor_affine, torch.qint8, torch.tensor(0.1), torch.tensor(0.0)))
    q = torch.quantize_per_channel(w.float(), sc, z, 0, torch.qint8).int_repr()
    for n, v in (("weight_int", q), ("weight_sum_by_input_channels", q.float().sum(1)), ("bias0", z.clone()), ("scale", sc * 0.1)):
        lin.register_buffer(n, v)
    for k, v in attrs.items():
        setattr(lin, k, v)
    net = torch.nn.Module()
    net.blk = torch.nn.Module()
    net.blk.to_q = lin
    return net, {"blk.to_q.weight": w}


@pytest.mark.parametrize("attrs,name,r,n_out,error,match", [
    ({}, "blk.nowhere", 4, 16, KeyError, "blk.nowhere matches no"),
    ({}, "blk.to_q", 40, 16, ValueError, "blk.to_q: summed rank 40 exceeds max_rank 32"),
    ({}, "blk.to_q", 4, 12, ValueError, "blk.to_q: factors .* do not fit"),
    ({"w_packed2": True}, "blk.to_q", 4, 16, ValueError, "blk.to_q stores 2-bit weights"),
    ({"bos": True}, "blk.to_q", 4, 16, ValueError, "blk.to_q is a BOS layer")])
def test_bank_errors_name_the_layer(attrs, name, r, n_out, error, match):
    from mixdq_amd.lora import LoraBank
    net, state = _stub(**attrs)
    with pytest.raises(error, match=match):                   # (every one is raised before anything is launched)
        LoraBank(net, state, max_rank=32).apply([{name: (torch.zeros(r, 32), torch.zeros(n_out, r), 4.0)}], [1.0])


def test_bank_finds_the_quantizer_width_or_refuses():
    from mixdq_amd.lora import LoraBank
    net, state = _stub()
    bank = LoraBank(net, state, max_rank=32)
    bank._tables(["blk.to_q"])
    assert bank.targets["blk.to_q"][0].desc.bits == 8 and bank.targets["blk.to_q"][0].snapshot[-1] is None
    with pytest.raises(ValueError, match="blk.to_q: float_state does not reproduce"):
        LoraBank(net, {"blk.to_q.weight": state["blk.to_q.weight"] * 1.5}, max_rank=32)._tables(["blk.to_q"])
