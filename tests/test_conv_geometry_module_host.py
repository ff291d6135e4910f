"""QuantizedConv2d over the conv geometries of tests/conv_geometry.py, on the CPU (the HIP operators replaced by the
oracle-backed stand-ins of tests/test_host.py): a layer runs on the INT8 operators, or is an FP fallback from its
construction on -- forward() never meets a refusal of the library."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.ao.quantization import QConfig, PlaceholderObserver

from tests import conv_geometry as cg
from tests import detdata as dd
from tests.test_host import oracle_ops  # noqa: F401  (fixture)

CIN, COUT = 16, 12


def quantized_conv(kernel_size, stride, padding, cin=CIN, cout=COUT):
    """(QuantizedConv2d.from_float(nn.Conv2d(cin, cout, kernel_size, stride, padding)) at W8A8, an fp32 input
    [2, cin, 9, 7])."""
    from mixdq_amd.nn import QuantizedConv2d
    fm = nn.Conv2d(cin, cout, kernel_size, stride, padding)
    seed = 7000 + 97 * kernel_size[0] + 13 * kernel_size[1] + 5 * stride[0] + padding[0]
    fm.weight.data = torch.from_numpy(dd.normal_f16(seed, tuple(fm.weight.shape), 0.05).astype(np.float32))
    fm.bias.data = torch.from_numpy(dd.normal_f16(seed + 1, (cout,), 0.1).astype(np.float32))
    fm = fm.half()
    fm.module_name = "geom.conv"
    fm.qconfig = QConfig(activation=PlaceholderObserver.with_args(dtype=torch.qint8),
                         weight=PlaceholderObserver.with_args(dtype=torch.qint8))
    fm.w_bit = fm.a_bit = 8
    wmax = fm.weight.detach().float().abs().amax(dim=(1, 2, 3))
    ckpt = {"geom.conv.weight_quantizer": dict(delta_list=(wmax / 127)[None].repeat(3, 1).half(),
                                               zero_point_list=torch.zeros(3, cout).half()),
            "geom.conv.act_quantizer": dict(delta_list=torch.full((3,), 0.03).half(),
                                            zero_point_list=torch.full((3,), 121.0).half())}
    x = torch.from_numpy(dd.normal_f16(seed + 2, (2, cin, 9, 7), 1.2).astype(np.float32))
    return QuantizedConv2d.from_float(fm, ckpt=ckpt), x


@pytest.mark.parametrize("g", cg.GEOMETRIES + cg.REFUSED, ids=str)
def test_module_runs_on_the_int8_operators_or_falls_back_at_construction(oracle, oracle_ops, g):
    R, S, stride, pad = g
    qm, x = quantized_conv((R, S), (stride, stride), (pad, pad))
    assert qm.valid_for_acceleration == (pad < R and pad < S)
    if not qm.valid_for_acceleration:
        assert qm._get_name() == "QuantizedConv2dFPFallback" and qm.weight.shape == (COUT, CIN, R, S)
        with torch.no_grad():
            y = qm.float()(x)                                 # F.conv2d on the CPU
        assert torch.equal(y, F.conv2d(x, qm.weight, qm.bias, stride, pad))
        return
    with torch.no_grad():
        y = qm(x.half())
    zp = float(qm.act_zero_points)
    xq = oracle.quantize(x.half().permute(0, 2, 3, 1).contiguous().numpy(), float(qm.act_scales_inv), zp)
    wt = qm.weight_int.permute(0, 2, 3, 1).contiguous().numpy()
    assert wt.shape == (COUT, R, S, CIN)
    # the reference chain, through this file's own window-intersection reference
    acc = cg.ei.conv_accumulate(xq.transpose(0, 3, 1, 2), wt.transpose(0, 3, 1, 2), stride, pad, dtype=np.int64)
    b0 = cg.zero_point_term(cg.wsum_of(wt), zp, 9, 7, stride, pad)
    if pad == 0:
        assert np.array_equal(qm.bias0.numpy(), b0[0, 0])
    want = cg.epilogue(acc.transpose(0, 2, 3, 1), b0[None], qm.scale.numpy(), qm.bias.numpy(), 0)
    got = y.permute(0, 2, 3, 1).contiguous().numpy()
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))


def test_one_by_three_with_unit_padding_is_an_fp_fallback_not_a_forward_error():
    """nn.Conv2d(.., (1, 3), padding=(1, 1)) passes the symmetric-stride / -padding test, and the INT8 entry refuses
    pad >= R: before the constructor checked it, forward() raised MIXDQ_ERR_PADDING."""
    qm, _ = quantized_conv((1, 3), (1, 1), (1, 1))
    assert not qm.valid_for_acceleration and not hasattr(qm, "weight_int")
    qm, _ = quantized_conv((3, 1), (1, 1), (1, 1))
    assert not qm.valid_for_acceleration
    qm, _ = quantized_conv((3, 3), (1, 1), (2, 2))
    assert qm.valid_for_acceleration


@pytest.mark.parametrize("stride,padding", [((2, 1), (1, 1)), ((1, 1), (1, 0)), ((2, 1), (1, 0))])
def test_asymmetric_stride_or_padding_stays_on_the_fp_path(stride, padding):
    qm, x = quantized_conv((3, 3), stride, padding)
    assert not qm.valid_for_acceleration and qm._get_name() == "QuantizedConv2dFPFallback"
    with torch.no_grad():
        y = qm.float()(x)
    assert torch.equal(y, F.conv2d(x, qm.weight, qm.bias, stride, padding))
