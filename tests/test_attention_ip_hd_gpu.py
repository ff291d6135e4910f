"""GPU tests of the decoupled cross-attention launch at SD 1.5's head widths (mixdq_attention_f16_ip_hd,
csrc/attention_ip_hd.hip): tests/test_attention_ip_gpu.py's three checks -- the float64 oracle at the attention tests'
tolerance per term plus the two added FP16 roundings, FP16 / INT8 / 4-bit outputs bit-equal to the chain of existing
launches, zero scales that read nothing -- at D = 40, 80 and 160, and the fused route of a W8A8 UNet with eight heads of
40 / 80 columns against the de-fused one and from a captured graph."""
import numpy as np
import pytest
import torch

from tests.test_attention_gpu import scal
from tests.test_attention_hd_gpu import ATOL, RTOL, WIDTHS
from tests.test_attention_ip_gpu import HEADS, S_INV, ZP, chain, make, same

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FOUR = (160, 77, (4, 4, 4, 4), (1.0, 0.6, -0.5, 0.6))     # two text stages + four blocks: past a CU's LDS at D = 160
CASES = [  # tq (33: a ragged last wave; 160: a second workgroup), tkv, image tokens per adapter, scales
    (33, 77, (4,), (0.6,)), (160, 1, (1,), (-0.5,)), (160, 128, (33,), (0.6,)), (33, 128, (64,), (1.0,)),
    (160, 77, (4, 16), (0.6, -0.5)), (33, 1, (4, 4, 4, 4), (0.6, 1.0, -0.5, 1.0)),
]
PARAMS = [(D, c) for D in WIDTHS for c in CASES + [FOUR] * (D != 160)]
REFUSED = {40: (129, (4,)), 80: (77, (33, 33, 4)), 160: FOUR[1:3]}


@pytest.mark.parametrize("D,case", PARAMS, ids=[f"d{D}_q{c[0]}_k{c[1]}_ip{'_'.join(map(str, c[2]))}" for D, c in PARAMS])
def test_one_launch_against_float64_the_chain_and_zero_scales(C, oracle, D, case):
    tq, tkv, tokens, scales = case
    ch = HEADS * D
    assert C.attention_ip_hd_supported(D, tkv, tokens) and not C.attention_ip_supported(D, tkv, tokens)
    (q, k, v, ip), (qd, kd, vd, ipd) = make(4100 + D + tq + tkv + sum(tokens), tq, tkv, tokens, ch)
    sd = torch.tensor(scales, dtype=torch.float32, device=qd.device)
    got = C.attention_ip(qd, kd, vd, ipd, sd, HEADS)
    assert got.shape == (2, tq, ch) and got.dtype == torch.float16
    # (a) float64
    s64 = [float(np.float32(s)) for s in scales]
    ref_t = oracle.attention_f16(q, k, v, HEADS)[1]
    ref_j = [oracle.attention_f16(q, kj, vj, HEADS)[1] for kj, vj in ip]
    ref = ref_t + sum(s * r for s, r in zip(s64, ref_j))
    tol = ((1 + sum(abs(s) for s in s64)) * ATOL + RTOL * (np.abs(ref_t) + sum(abs(s) * np.abs(r) for s, r in zip(s64, ref_j)))
           + 2.0 ** -11 * (sum(np.abs(s * r) for s, r in zip(s64, ref_j)) + np.abs(ref)))
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
    print(f"max err {err.max():.3e}, max err / tol {(err / tol).max():.3f}")
    assert (err <= tol).all()
    # (b) the chain of existing launches: FP16, INT8 and 4-bit
    want = chain(C, qd, kd, vd, ipd, scales)
    assert same(got, want)
    si, zp = scal(S_INV), scal(ZP)
    got8 = C.attention_ip(qd, kd, vd, ipd, sd, HEADS, si, zp)
    assert torch.equal(got8, C.quantize_per_tensor_to_int8(want, si, zp)) and (got8 != got8.flatten()[0]).any()
    assert torch.equal(C.attention_ip(qd, kd, vd, ipd, sd, HEADS, si, zp, _abits=4),
                       C.quantize_per_tensor_to_int8(want, si, zp, _abits=4))
    # (c) a zero scale of either sign: the adapter's NaN keys and values are not read
    nan = [(torch.full_like(kj, float("nan")), torch.full_like(vj, float("nan"))) for kj, vj in ipd]
    s0 = sd.clone()
    s0[0] = -0.0
    one_off = C.attention_ip(qd, kd, vd, nan[:1] + ipd[1:], s0, HEADS)
    rest = C.attention_ip(qd, kd, vd, ipd[1:], sd[1:].clone(), HEADS) if len(ipd) > 1 else C.attention_f16(qd, kd, vd, HEADS)
    assert torch.isfinite(one_off).all() and same(one_off, rest)
    assert same(C.attention_ip(qd, kd, vd, nan, torch.zeros_like(sd), HEADS), C.attention_f16(qd, kd, vd, HEADS))


@pytest.mark.parametrize("D", WIDTHS)
def test_refused_shapes_run_the_chain(C, D):
    tkv, tokens = REFUSED[D]
    assert not C.attention_ip_hd_supported(D, tkv, tokens)
    _, (qd, kd, vd, ipd) = make(4600 + D, 33, tkv, tokens, HEADS * D)
    scales = (0.6, -0.5, 1.0, 0.6)[:len(tokens)]
    sd = torch.tensor(scales, dtype=torch.float32, device=qd.device)
    want = chain(C, qd, kd, vd, ipd, scales)
    assert same(C.attention_ip(qd, kd, vd, ipd, sd, HEADS), want)
    si, zp = scal(S_INV), scal(ZP)
    assert torch.equal(C.attention_ip(qd, kd, vd, ipd, sd, HEADS, si, zp), C.quantize_per_tensor_to_int8(want, si, zp))


@pytest.fixture(scope="module")
def tiny15(C):
    """tests/test_ip_adapter_gpu.py's tiny W8A8 UNet with SD 1.5's heads: EIGHT per level, 40 columns at the 320-channel
    level (256 queries at latent 32), 80 at the 640-channel level and in the mid block (64 queries)."""
    import bench
    from mixdq_amd.quantize_sdxl import example_inputs
    from mixdq_amd.unet import build_unet
    from tests.test_control_gpu import L_TINY, _w8a8
    cfg = dict(bench.TINY_CFG, block_out_channels=(64, 320, 640), transformer_layers_per_block=(0, 1, 1), head_dim=None,
               num_attention_heads=8)
    inputs = example_inputs(2, L_TINY, DEV, seed=7)
    unet = _w8a8(build_unet(DEV, cfg=cfg), inputs)
    yield dict(cfg=cfg, unet=unet, inputs=inputs)
    del unet
    torch.cuda.empty_cache()


@pytest.mark.parametrize("num_tokens", [4, 16])
def test_fused_sd15_heads_equal_defused_and_a_graph_serves_every_scale(C, tiny15, num_tokens):
    from mixdq_amd import unet as U
    from mixdq_amd.ip_adapter import IPState, build_ip_adapter
    from tests.test_control_gpu import _same
    unet, inp = tiny15["unet"], tiny15["inputs"]
    assert all(C.attention_ip_hd_supported(D, 77, (num_tokens,)) for D in (40, 80))
    adapter = build_ip_adapter(tiny15["cfg"], 64, num_tokens=num_tokens, device=DEV)
    embeds = torch.randn(2, 64, generator=torch.Generator(device="cpu").manual_seed(9)).half().to(DEV)
    ip = IPState([adapter.kv(adapter.tokens(embeds))], torch.full((len(adapter.dims), 1), 0.6, dtype=torch.float32, device=DEV))
    with torch.no_grad():
        eager = {}
        for s in (0.6, -0.5):
            ip.scales.fill_(s)
            eager[s] = unet(**inp, ip=ip)[0].clone()
        with U.defused():
            _same(eager[-0.5], unet(**inp, ip=ip)[0], "UNet with ip=, fused vs de-fused")
        assert not torch.equal(eager[0.6], eager[-0.5]) and bool(torch.isfinite(eager[0.6]).all())
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            unet(**inp, ip=ip)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = unet(**inp, ip=ip)[0]
        for s in (0.6, -0.5, 0.6):                                      # ONE graph, two scale tables, several replays
            ip.scales.fill_(s)
            graph.replay()
            _same(out, eager[s], f"graph replay at scale {s}")
