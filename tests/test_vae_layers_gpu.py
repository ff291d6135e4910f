"""Every distinct conv launch of the FP16 VAE (mixdq_amd.vae, both halves) at VAE_SDXL_CONFIG's widths, on every tile of
C.F16_CONFIGS -- among them the two a full-size decode spends most of its time on (13: 256x128x64, 20: 256x256x128;
DESIGN.md section 3.23), which no small image takes by the automatic rule.

The launches are enumerated from the config the way the forward passes walk it (tests/vae_layers.py;
tests/test_vae_host.py checks the list on the CPU): the 3x3 convs of the ResNets with and without the residual fold, the
1x1 shortcuts, the folded upsamplers (`_upsample2x`), the pad-after stride-2 convs (`_pad_after`), the 8-channel conv_in,
the padded 4-channel conv_out, the encoder's 8-channel conv_out and quant_conv, and the decoder's two 4-channel convs
(the one-output-per-thread kernel, which has no tiles: every `_cfg` is the same launch).  Each runs at N = 2 with a 12 x 10 output: 240 output rows, so that on a 256-row tile the two images
share one tile, and on every tile the last one is ragged.

Required of each: every tile gives the same bits; the result is within tests/test_f16_gpu.py's bound, 2^-10 |ref| +
2^-10 rms(ref), of F.conv2d in float64 on the CPU (on the explicitly upsampled / padded tensor for the two flags); with
a residual the result is bit-equal to the launch without it plus the residual.
"""
import pytest
import torch
import torch.nn.functional as F

from tests.test_f16_gpu import close, rnd
from tests.vae_layers import LAUNCHES, launch_id

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P_OUT, Q_OUT, BATCH = 12, 10, 2


@pytest.mark.parametrize("geom", LAUNCHES, ids=[launch_id(g) for g in LAUNCHES])
def test_vae_conv_launch_on_every_tile(C, geom):
    cin, cout, k, stride, flag, residual = geom
    pad = k // 2
    up, after = flag == "upsample2x", flag == "pad_after"
    H, W = (P_OUT // 2, Q_OUT // 2) if up else (P_OUT * stride, Q_OUT * stride)
    seed = 100 + 7 * LAUNCHES.index(geom)
    x = rnd((BATCH, cin, H, W), seed).contiguous(memory_format=torch.channels_last)
    w, b = rnd((cout, cin, k, k), seed + 1, 0.05), rnd((cout,), seed + 2)
    kw = dict(_upsample2x=up, _pad_after=after)
    auto = C.conv2d_f16(x, w, b, stride, pad, **kw)
    assert tuple(auto.shape) == (BATCH, cout, P_OUT, Q_OUT) and auto.dtype == torch.float16
    # the definition in float64, on the tensor the flag stands for
    xr = x.cpu().double()
    if up:
        ref = F.conv2d(F.interpolate(xr, scale_factor=2, mode="nearest"), w.cpu().double(), b.cpu().double(), 1, 1)
    elif after:
        ref = F.conv2d(F.pad(xr, (0, pad, 0, pad)), w.cpu().double(), b.cpu().double(), stride, 0)
    else:
        ref = F.conv2d(xr, w.cpu().double(), b.cpu().double(), stride, pad)
    close(auto, ref)
    res = rnd((BATCH, cout, P_OUT, Q_OUT), seed + 3).contiguous(memory_format=torch.channels_last) if residual else None
    want = auto + res if residual else auto
    if residual:
        assert torch.equal(C.conv2d_f16(x, w, b, stride, pad, _residual=res, **kw), want)
    for cfg in (13, 20) + tuple(c for c in C.F16_CONFIGS if c not in (13, 20)):
        got = C.conv2d_f16(x, w, b, stride, pad, _residual=res, _cfg=cfg, **kw)
        assert torch.equal(got, want), f"tile {cfg}: {int((got != want).sum())} of {got.numel()} values differ"
    assert {13, 20} <= set(C.F16_CONFIGS)
