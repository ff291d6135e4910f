"""IP-Adapter through the UNet and the Sampler on the GPU: the tiny W8A8 UNet of tests/test_control_gpu.py with one
4-token adapter.  Fused == de-fused bit for bit (the one mixdq_attention_f16_ip launch per cross-attention against the
chain of attention_f16 launches and torch operations), a graph replay == eager for every scale table, and a 3-step
guided Sampler run == the loop a user would write around unet(..., ip=), twice on one graph with different scales."""
import numpy as np
import pytest
import torch

from tests import sampler_ref as S
from tests.test_control_gpu import DEV, GUIDANCE, L_TINY, N_STEPS, _same, _sampler_inputs, _w8a8, t

pytestmark = pytest.mark.gpu
EMBED = 64


@pytest.fixture(scope="module")
def tiny_ip(C):
    import bench
    from mixdq_amd.ip_adapter import build_ip_adapter
    from mixdq_amd.quantize_sdxl import example_inputs
    from mixdq_amd.unet import build_unet
    cfg = dict(bench.TINY_CFG, block_out_channels=(64, 128, 256), head_dim=64)
    inputs = example_inputs(2, L_TINY, DEV, seed=7)
    unet = _w8a8(build_unet(DEV, cfg=cfg), inputs)
    adapter = build_ip_adapter(cfg, EMBED, num_tokens=4, device=DEV)
    g = torch.Generator(device="cpu").manual_seed(9)
    embeds = torch.randn(2, EMBED, generator=g).half().to(DEV)
    yield dict(unet=unet, adapter=adapter, inputs=inputs, embeds=embeds)
    del unet, adapter
    torch.cuda.empty_cache()


def _state(adapter, embeds, scale):
    from mixdq_amd.ip_adapter import IPState
    kv = adapter.kv(adapter.tokens(embeds))
    return IPState([kv], torch.full((len(adapter.dims), 1), scale, dtype=torch.float32, device=DEV))


def test_fused_is_defused_and_a_graph_serves_every_scale(tiny_ip):
    from mixdq_amd import unet as U
    unet, inp = tiny_ip["unet"], tiny_ip["inputs"]
    ip = _state(tiny_ip["adapter"], tiny_ip["embeds"], 0.6)
    with torch.no_grad():
        fused = unet(**inp, ip=ip)[0]
        with U.defused():
            defused = unet(**inp, ip=ip)[0]
        _same(fused, defused, "UNet with ip=, fused vs de-fused")
        plain = unet(**inp)[0]
        assert not torch.equal(fused, plain) and bool(torch.isfinite(fused).all())
        eager = {}
        for s in (0.6, -0.5, 0.0):
            ip.scales.fill_(s)
            eager[s] = unet(**inp, ip=ip)[0].clone()
        _same(eager[0.0], plain, "scale 0 is the plain forward")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            unet(**inp, ip=ip)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = unet(**inp, ip=ip)[0]
        for s in (0.6, -0.5, 0.0, 0.6):                                 # ONE graph, every scale, several replays
            ip.scales.fill_(s)
            graph.replay()
            _same(out, eager[s], f"graph replay at scale {s}")


def _eager_loop(unet, adapter, sampler, noise, ehs, added, embeds, scale):
    """The loop a user would write: tokens and keys | values once (zero embeddings for the unconditional rows), per
    step the UNet with ip= and the numpy restatement of the guided Euler step."""
    from mixdq_amd.ip_adapter import IPState
    s, B = sampler.schedule, noise.shape[0]
    kv = adapter.kv(adapter.tokens(torch.cat([torch.zeros_like(embeds), embeds])))
    ip = IPState([kv], torch.full((len(adapter.dims), 1), scale, dtype=torch.float32, device=DEV))
    x, inp = S.init(noise.float().cpu().numpy(), s.init_scale, s.input_scale0)
    for i in range(s.n_steps):
        sample = t(np.concatenate([inp] * 2, axis=0))
        with torch.no_grad():
            eps = unet(sample, torch.tensor(float(s.timesteps[i]), device=DEV), ehs, added, ip=ip)[0]
        eps = eps.float().cpu().numpy().astype(np.float16)
        x, inp = S.step(x, eps[:B], eps[B:], s.coef[i], sampler.guidance_scale, None)
    return x


def test_sampler_with_an_adapter_equals_the_eager_loop_and_reuses_its_graph(C, tiny_ip):
    from mixdq_amd import Sampler
    unet, adapter, embeds = tiny_ip["unet"], tiny_ip["adapter"], tiny_ip["embeds"]
    sm = Sampler(unet, "euler", N_STEPS, GUIDANCE, ip_adapter=adapter)
    noise, ehs, added, *_ = _sampler_inputs(2, 80, False)
    results, graph = [], None
    for scale in (0.6, 1.0):
        got = sm.sample(noise, ehs, added, ip_embeds=embeds, ip_scale=scale)
        assert graph is None or sm._graph is graph, "one graph, never re-captured"
        graph = sm._graph
        _same(got, _eager_loop(unet, adapter, sm, noise, ehs, added, embeds, scale), f"ip_scale {scale}")
        results.append(got)
    assert not torch.equal(results[0], results[1])
    with pytest.raises(TypeError):
        sm.sample(noise, ehs, added)                                    # built with ip_adapter=: the image is required
    with pytest.raises(TypeError):
        Sampler(unet, "euler", N_STEPS, GUIDANCE).sample(noise, ehs, added, ip_embeds=embeds)
    with pytest.raises(ValueError):
        Sampler(unet, "euler", N_STEPS, GUIDANCE, image_guidance_scale=1.5, ip_adapter=adapter)
