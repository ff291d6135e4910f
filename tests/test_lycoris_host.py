"""Host side of the LoHa / DoRA launch: the descriptor, every refusal (nothing is launched), LoraBank's errors by layer
name, conv factor order, and that an apply() of tuples leaves the new tables alone."""
import ctypes

import numpy as np
import pytest
import torch

import mixdq_amd._C as C
from tests.test_lora_host import INVALID, OK, SHAPE, _stub, _valid


def test_descriptor_and_table():
    assert ctypes.sizeof(C.LycorisLayer) == 200 and C.LycorisLayer.B2cat.offset == ctypes.sizeof(C.LoraLayer) == 136
    tab = C.LycorisTable([C.LycorisLayer(N=40, Kf=36), C.LycorisLayer(N=17, Kf=96), C.LycorisLayer(N=1, Kf=640)], "cpu")
    assert tab.order == [2, 1, 0] and tab.prefix == [0, 1, 3, 6] and tab.grid == 6


@pytest.mark.parametrize("over,status", [
    ({}, OK), ({"R_lin": 0, "had_end": [32]}, OK), ({"R": 128, "R_lin": 32, "had_end": [64, 128]}, OK),
    ({"R_lin": 0}, OK),                                         # no rank at all: the row norm alone
    ({"R_lin": 16}, SHAPE), ({"R_lin": 64}, SHAPE), ({"R_lin": 0, "had_end": [16]}, SHAPE),
    ({"R": 64, "R_lin": 32, "had_end": [32]}, SHAPE),           # an empty range
    ({"R": 64, "R_lin": 32, "had_end": [96]}, SHAPE),           # beyond R
    ({"R_lin": 0, "had_end": [32], "B2cat": None}, INVALID), ({"R_lin": 0, "had_end": [32], "A2cat": None}, INVALID),
    ({"n_had": 9}, INVALID), ({"n_had": -1}, INVALID), ({"B2cat": 4}, SHAPE), ({"magnitude": 2}, SHAPE),
    ({"R": 48}, SHAPE), ({"mode": C.LORA_W2, "bits": 2}, SHAPE), ({"W": None}, INVALID)])
def test_refusals(over, status):
    buf = np.zeros(64, np.float64)
    base = buf.ctypes.data
    over = {k: (base + v if k in ("B2cat", "magnitude") and v is not None else v) for k, v in over.items()}
    d = C.LycorisLayer.from_lora(_valid(buf), **{"R_lin": 32, "B2cat": base, "A2cat": base, "magnitude": base, **over})
    assert C.lycoris_status([d]) == status
    assert C.lycoris_status([]) == INVALID


def _loha(r, n=16, k=32, **more):
    return dict(kind="loha", w1_a=torch.zeros(n, r), w1_b=torch.zeros(r, k), w2_a=torch.zeros(n, r), w2_b=torch.zeros(r, k),
                alpha=1.0, **more)


def _dora(r=4):
    return dict(kind="lora", A=torch.zeros(r, 32), B=torch.zeros(16, r), alpha=1.0, magnitude=torch.ones(16))


@pytest.mark.parametrize("attrs,adapters,match", [
    ({}, [{"blk.to_q": _dora()}, {"blk.to_q": _dora()}], "blk.to_q: more than one magnitude"),
    ({}, [{"blk.to_q": _loha(33)}, {"blk.to_q": (torch.zeros(4, 32), torch.zeros(16, 4), 1.0)}], "blk.to_q: summed rank 96 .* exceeds max_rank 64"),
    ({}, [{"blk.to_q": _loha(4, hada_t1=torch.zeros(4, 4, 3, 3))}], "blk.to_q: Tucker-form LoHa"),
    ({}, [{"blk.to_q": _loha(4, n=12)}], "blk.to_q: factors .* do not fit"),
    ({}, [{"blk.to_q": {"kind": "lokr"}}], "blk.to_q: adapter kind 'lokr'"),
    ({"w_packed2": True}, [{"blk.to_q": _loha(4)}], "blk.to_q stores 2-bit weights"),
    ({"split": 16, "in_channels": 32}, [{"blk.to_q": _dora()}], "blk.to_q: a magnitude on a split conv_shortcut")])
def test_bank_errors_name_the_layer(attrs, adapters, match):
    from mixdq_amd.lora import LoraBank
    net, state = _stub(**attrs)
    if "split" in attrs:                                      # the second half's buffers, as a split shortcut keeps them
        lin = net.blk.to_q
        for n in ("weight_int", "weight_scales", "weight_sum_by_input_channels", "bias0", "scale", "act_scales", "act_zero_points"):
            v = getattr(lin, n, None)
            if v is not None:
                setattr(lin, n + "_0", v[:, 16:].contiguous() if n == "weight_int" else v.clone())
        lin.weight_int = lin.weight_int[:, :16].contiguous()
    with pytest.raises(ValueError, match=match):              # (every one is raised before anything is launched)
        LoraBank(net, state, max_rank=64).apply(adapters, [1.0] * len(adapters))


def test_flat_conv_factor_is_reordered_and_tuples_leave_the_new_tables_alone():
    from mixdq_amd.lora import LoraBank, conv_factor_stored
    A = torch.randn(4, 6, 3, 3, generator=torch.Generator().manual_seed(0))
    bank = LoraBank(torch.nn.Module(), {"c.weight": torch.zeros(5, 6, 3, 3)})
    assert torch.equal(bank._stored_factor("c", A.reshape(4, -1), 4, True), conv_factor_stored(A))
    assert torch.equal(bank._stored_factor("c", A, 4, True), conv_factor_stored(A))
    net, state = _stub()
    bank = LoraBank(net, state, max_rank=32)
    with pytest.raises(RuntimeError, match="lora_requant: the table should be on the GPU"):      # the LoRA entry point
        bank.apply([{"blk.to_q": (torch.zeros(4, 32), torch.zeros(16, 4), 4.0)}], [1.0])
    tg = bank.targets["blk.to_q"][0]
    assert bank.lyco is None and tg.B2cat is None and tg.A2cat is None and tg.mag is None
    with pytest.raises(RuntimeError, match="lycoris_requant: the table should be on the GPU"):
        bank.apply([{"blk.to_q": _loha(4)}], [1.0])
    assert tg.B2cat is not None and bank.lyco["ranges"]["blk.to_q"] == (0, [32])
