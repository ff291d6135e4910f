"""A derived tensor under a captured graph: the zero-padded weight of an FP-fallback QuantizedConv2d (every quantized
UNet's conv_in: 4 input channels padded to 8) follows an in-place load_state_dict at its address, so a graph captured
before the load replays with the new weights.  (On the commit before mixdq_amd/derived.py the same sequence was run
once and failed as predicted: the padded copy was only re-allocated by the next eager forward, and the replay after the
load was bit-equal to the output of the OLD weights.)"""
import pytest
import torch

from tests import detdata as dd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _pad8(t):
    out = torch.zeros((t.shape[0], 8) + tuple(t.shape[2:]), dtype=t.dtype, device=t.device
                      ).contiguous(memory_format=torch.channels_last)
    out[:, :t.shape[1]] = t
    return out


def test_padded_fp_fallback_conv_follows_a_load_under_a_captured_graph(C):
    from mixdq_amd.derived import holder_of, stored
    from mixdq_amd.nn.Conv2d import QuantizedConv2d
    w1 = torch.from_numpy(dd.normal_f16(301, (8, 4, 3, 3), 0.2)).to(DEV)
    w2 = torch.from_numpy(dd.normal_f16(302, (8, 4, 3, 3), 0.2)).to(DEV)
    x = torch.from_numpy(dd.normal_f16(303, (1, 4, 8, 8), 1.0)).to(DEV).contiguous(memory_format=torch.channels_last)
    conv = QuantizedConv2d(4, 8, (3, 3), (1, 1), (1, 1), (1, 1), bias=False)      # no quantizers: the FP fallback
    assert not conv.valid_for_acceleration
    conv.register_buffer("weight", w1.clone())
    conv.bias = None
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        eager = conv(x).clone()
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(eager, C.conv2d_f16(_pad8(x), _pad8(w1), None, 1, 1))
    (padded,) = stored(holder_of(conv), "w_padded")
    ptr = padded.data_ptr()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g), torch.no_grad():
        y = conv(x)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, eager)

    missing, unexpected = conv.load_state_dict({"weight": w2})
    assert not missing and not unexpected and torch.equal(conv.weight, w2)
    g.replay()
    torch.cuda.synchronize()
    want = C.conv2d_f16(_pad8(x), _pad8(w2), None, 1, 1)
    assert not torch.equal(want, eager)
    assert torch.equal(y, want), "the replay still shows the weights from before the load"
    assert stored(holder_of(conv), "w_padded")[0].data_ptr() == ptr == padded.data_ptr()
    assert torch.equal(padded, _pad8(w2))
    with torch.no_grad():
        assert torch.equal(conv(x), want)
