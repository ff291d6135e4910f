"""GPU tests of the FP16 VAE encoder (mixdq_amd.vae.VAEEncoder) and its two own kernels.

mixdq_image_to_nhwc8_f16 and mixdq_vae_latent_sample are compared BIT FOR BIT with their numpy float32 restatements
(tests/vae_enc_ref.py; the exponential from the oracle library).

The encoder runs on a small config that still reaches every kernel of the full one: the ingest, conv_in on the MFMA
tiles through the 8-channel form, 3x3 / 1x1 convs with the residual fold, the three pad-after downsampling convs,
GroupNorm (+SiLU), the fused q|k|v projection, attention at head width 512, the 8-channel conv_out / quant_conv and the
posterior sample.  Bound (that of tests/test_vae_gpu.py): the oracle is the same network built from stock torch modules
in FP32 on the CPU with the same weights upcast; required is max |moments - fp32| <= max(1.5 x max |stock fp16 on this
GPU - fp32|, one FP16 ulp at max |fp32|).
"""
import numpy as np
import pytest
import torch

from tests import vae_enc_ref as ER

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _same(got, want, what):
    g = got.detach().cpu().contiguous().numpy()
    g, w = g.view({2: np.uint16, 4: np.uint32}[g.dtype.itemsize]), want.view({2: np.uint16, 4: np.uint32}[want.dtype.itemsize])
    assert g.shape == w.shape and np.array_equal(g, w), f"{what}: {int((g != w).sum())} of {g.size} elements differ"


def _nhwc(t):
    """The storage of a channels-last [B, C, H, W] result as [B, H, W, C]."""
    assert t.is_contiguous(memory_format=torch.channels_last) or t.shape[1] == 1
    return t.permute(0, 2, 3, 1)


# ---- (b) the ingest ----------------------------------------------------------------------------------------------
def test_ingest_uint8_all_values_in_both_layouts(C):
    rng = np.random.default_rng(5)
    img = np.concatenate([np.arange(256, dtype=np.uint8), rng.integers(0, 256, 3 * 16 * 16 - 256, dtype=np.uint8)])
    img = rng.permutation(img).reshape(1, 3, 16, 16)
    assert len(np.unique(img)) == 256
    want = ER.ingest(img)
    nchw = torch.from_numpy(img).to(DEV)
    nhwc = nchw.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)                  # same values, NHWC strides
    assert nchw.stride() != nhwc.stride()
    for name, src in (("nchw", nchw), ("nhwc", nhwc)):
        out = C.image_to_nhwc8_f16(src)
        assert out.dtype == torch.float16 and tuple(out.shape) == (1, 8, 16, 16)
        assert out.is_contiguous(memory_format=torch.channels_last)
        _same(_nhwc(out), want, name)
        assert not bool(out[:, 3:].any())


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_ingest_float_sources_are_rounded_not_clamped(C, dtype):
    """A [1, 3, 3, 5] image (45 values, no multiple of anything): +-65520 is the FP32 halfway point between the largest
    finite FP16 and 2^16 and rounds to infinity; 65519.996 does not; values beyond [-1, 1] pass."""
    rng = np.random.default_rng(6)
    img = rng.uniform(-1, 1, (1, 3, 3, 5)).astype(np.float32)
    edge = np.array([65520.0, -65520.0, 65519.996, 3.5, -7.25, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2.0 ** -25, -0.0],
                    dtype=np.float32)
    if dtype == torch.float16:
        with np.errstate(over="ignore"):
            edge = edge.astype(np.float16).astype(np.float32)               # what an FP16 source can hold (+-inf too)
    img.reshape(-1)[:len(edge)] = edge
    src = torch.from_numpy(img).to(DEV).to(dtype)
    want = ER.ingest(src.cpu().numpy())
    if dtype == torch.float32:
        assert np.isinf(want[0, 0, 0, 0]) and np.isinf(want[0, 0, 1, 0]) and want[0, 0, 2, 0] == np.float16(65504)
    for name, s in (("nchw", src), ("nhwc", src.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)),
                    ("slice", torch.cat([src, src], 3)[:, :, :, 5:])):       # a view with a row stride of its own
        out = C.image_to_nhwc8_f16(s)
        assert tuple(out.shape) == (1, 8, 3, 5)
        _same(_nhwc(out), want, name)


def test_ingest_channel_counts_grid_stride_and_errors(C):
    rng = np.random.default_rng(7)
    for ch in (1, 4, 8):
        img = rng.integers(0, 256, (2, ch, 5, 7), dtype=np.uint8)
        _same(_nhwc(C.image_to_nhwc8_f16(torch.from_numpy(img).to(DEV))), ER.ingest(img), f"C = {ch}")
    # more pixels than the capped grid has lanes (2048 workgroups x 256): a second trip of the grid-stride loop
    img = rng.integers(0, 256, (1, 3, 8, 2048 * 32 + 24), dtype=np.uint8)
    _same(_nhwc(C.image_to_nhwc8_f16(torch.from_numpy(img).to(DEV))), ER.ingest(img), "grid stride")
    assert tuple(C.image_to_nhwc8_f16(torch.zeros(0, 3, 8, 8, dtype=torch.uint8, device=DEV)).shape) == (0, 8, 8, 8)
    with pytest.raises(RuntimeError, match="1 to 8 channels"):
        C.image_to_nhwc8_f16(torch.zeros(1, 9, 4, 4, dtype=torch.uint8, device=DEV))
    x = torch.zeros(1, 3, 4, 4, dtype=torch.uint8, device=DEV)
    sentinel = 0x5a5a
    out = torch.full((4 * 4 * 8 + 8,), sentinel, dtype=torch.int16, device=DEV)
    call = lambda ptr, c, dt=0, o=out.data_ptr(), b=1: C._lib.mixdq_image_to_nhwc8_f16(ptr, dt, 48, 16, 4, 1, o, b, c, 4, 4, None)
    assert call(x.data_ptr(), 0) == 1 and call(x.data_ptr(), 9) == 1 and call(None, 3) == 1      # INVALID_ARG
    assert call(x.data_ptr(), 3, dt=3) == 1 and call(x.data_ptr(), 3, b=-1) == 1
    assert call(x.data_ptr(), 3, o=None) == 1
    assert call(x.data_ptr(), 3, o=out.data_ptr() + 2) == 2                                         # ALIGNMENT
    assert call(x.data_ptr(), 3, b=0) == 0
    torch.cuda.synchronize()
    assert bool((out == sentinel).all())
    assert call(x.data_ptr(), 3) == 0
    torch.cuda.synchronize()
    assert bool((out[4 * 4 * 8:] == sentinel).all()) and not bool((out[:4 * 4 * 8] == sentinel).any())


# ---- (c) the posterior sample ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 3, 5, 4), (2, 8, 10, 4), (1, 3, 5, 8)], ids=lambda s: "x".join(map(str, s)))
def test_latent_sample_equals_the_restatement(C, oracle, shape):
    B, h, w, L = shape
    rng = np.random.default_rng(8 + h)
    m = np.empty((B, h, w, 2 * L), dtype=np.float16)
    m[..., :L] = rng.standard_normal((B, h, w, L)) * 3
    m[..., L:] = rng.uniform(-12, 6, (B, h, w, L))
    edge = np.array([-31, -30, 20, 21, -30.02, 19.98, 0, -0.0, -64, 40, 1e-3], dtype=np.float16)   # the clamp and around it
    m.reshape(-1, 2 * L)[:len(edge), L] = edge                     # (a view: m is contiguous)
    noise = rng.standard_normal((B, h, w, L)).astype(np.float32)
    md = torch.from_numpy(m).to(DEV).permute(0, 3, 1, 2)
    nd = torch.from_numpy(noise).to(DEV).permute(0, 3, 1, 2)
    for sf in (0.13025, 1.0):
        z = C.vae_latent_sample(md, nd, sf)
        assert z.dtype == torch.float32 and tuple(z.shape) == (B, L, h, w)
        assert z.is_contiguous(memory_format=torch.channels_last) or L == 1
        want = ER.latent_sample(oracle.lib(), m, noise, sf)
        assert np.isfinite(want).all()
        _same(_nhwc(z), want, f"sample, sf {sf}")
        _same(_nhwc(C.vae_latent_sample(md, None, sf)), ER.latent_sample(oracle.lib(), m, None, sf), f"mode, sf {sf}")
    # logvar -31 and -30 give the same std, 21 and 20 too
    one = np.zeros((1, 1, 4, 8), dtype=np.float16)
    one[0, 0, :, 4:] = np.array([-31, -30, 20, 21], dtype=np.float16)[:, None]
    z = C.vae_latent_sample(torch.from_numpy(one).to(DEV).permute(0, 3, 1, 2),
                            torch.ones(1, 4, 1, 4, device=DEV).contiguous(memory_format=torch.channels_last), 1.0)
    z = _nhwc(z).cpu().numpy()[0, 0]
    assert (z[0] == z[1]).all() and (z[2] == z[3]).all() and z[0, 0] > 0 and abs(z[2, 0] / np.exp(10.0) - 1) < 1e-6


def test_latent_sample_grid_stride_and_errors(C, oracle):
    rng = np.random.default_rng(9)
    n = 2048 * 256 + 77                                            # more pixels than the capped grid has lanes
    m = rng.uniform(-2, 2, (1, 1, n, 8)).astype(np.float16)
    noise = rng.standard_normal((1, 1, n, 4)).astype(np.float32)
    z = C.vae_latent_sample(torch.from_numpy(m).to(DEV).permute(0, 3, 1, 2),
                            torch.from_numpy(noise).to(DEV).permute(0, 3, 1, 2), 0.18215)
    half = np.float32(0.5) * m[..., 4:].astype(np.float32)
    vals, inv = np.unique(half, return_inverse=True)               # FP16 log-variances: few distinct values
    std = np.array([oracle.lib().mixdq_oracle_expf(float(v)) for v in vals], np.float32)[inv].reshape(half.shape)
    _same(_nhwc(z), (m[..., :4].astype(np.float32) + std * noise) * np.float32(0.18215), "grid stride")
    md = torch.zeros(1, 8, 2, 2, dtype=torch.float16, device=DEV).contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match="noise should be"):
        C.vae_latent_sample(md, torch.zeros(1, 4, 2, 2, device=DEV))                      # not channels-last
    with pytest.raises(RuntimeError, match="alignment"):
        C.vae_latent_sample(torch.zeros(1, 4, 2, 2, dtype=torch.float16, device=DEV).contiguous(
            memory_format=torch.channels_last))                                           # L = 2
    zbuf = torch.full((20,), -7.0, device=DEV)
    lib = C._lib.mixdq_vae_latent_sample
    assert lib(None, None, zbuf.data_ptr(), 4, 4, 1.0, None) == 1 and lib(md.data_ptr(), None, None, 4, 4, 1.0, None) == 1
    assert lib(md.data_ptr(), None, zbuf.data_ptr(), -1, 4, 1.0, None) == 1
    assert lib(md.data_ptr(), None, zbuf.data_ptr() + 4, 4, 4, 1.0, None) == 2
    assert lib(md.data_ptr() + 8, None, zbuf.data_ptr(), 3, 4, 1.0, None) == 2
    assert lib(md.data_ptr(), None, zbuf.data_ptr(), 0, 4, 1.0, None) == 0
    torch.cuda.synchronize()
    assert bool((zbuf == -7.0).all())


# ---- the encoder --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    from mixdq_amd import vae as V
    cfg = dict(V.VAE_SDXL_CONFIG, block_out_channels=(32, 64, 128, 512), layers_per_block=1, norm_num_groups=8)
    enc = V.build_vae_encoder(cfg, seed=11, device=DEV)
    g = torch.Generator(device="cpu").manual_seed(12)
    image = (torch.rand(2, 3, 64, 80, generator=g) * 2 - 1).to(DEV)                   # uniform in [-1, 1], FP32
    noise = torch.randn(2, 4, 8, 10, generator=g).to(DEV)
    moments = enc.moments(image)
    latents = enc.encode(image, noise)
    torch.cuda.synchronize()
    return dict(cfg=cfg, enc=enc, image=image, noise=noise, moments=moments, latents=latents)


def test_vae_moments_vs_the_stock_network(small):
    cfg, enc, image, moments = small["cfg"], small["enc"], small["image"], small["moments"]
    assert moments.dtype == torch.float16 and tuple(moments.shape) == (2, 8, 8, 10)
    assert moments.is_contiguous(memory_format=torch.channels_last) and bool(torch.isfinite(moments).all())
    sd = enc.state_dict()
    x16 = image.half()                                              # what the ingest feeds conv_in
    ref = ER.stock_encoder(cfg, sd, torch.float32, "cpu")(x16.float().cpu())
    stock16 = ER.stock_encoder(cfg, sd, torch.float16, DEV)(x16).float().cpu()
    err_ours = (moments.float().cpu() - ref).abs().max().item()
    err_stock = (stock16 - ref).abs().max().item()
    amax = ref.abs().max().item()
    ulp = 2.0 ** (torch.tensor(amax).log2().floor().item() - 10)          # one FP16 ulp at the top of the output range
    print(f"vae encoder small: max |ref| {amax:.4f}, max |logvar| {ref[:, 4:].abs().max().item():.4f}, "
          f"max err ours {err_ours:.3e}, stock fp16 {err_stock:.3e}, ulp floor {ulp:.3e}")
    assert amax > 1e-2                                                   # (the comparison is of something)
    assert err_ours <= max(1.5 * err_stock, ulp)


def test_vae_encode_is_the_restatement_on_its_own_moments(small, oracle):
    enc, moments, noise = small["enc"], small["moments"], small["noise"]
    z = small["latents"]
    assert z.dtype == torch.float32 and tuple(z.shape) == (2, 4, 8, 10) and z.is_contiguous(memory_format=torch.channels_last)
    m = _nhwc(moments).cpu().numpy()
    n = noise.permute(0, 2, 3, 1).cpu().numpy()
    _same(_nhwc(z), ER.latent_sample(oracle.lib(), m, n, enc.scaling_factor), "encode(image, noise)")
    _same(_nhwc(enc.encode(small["image"])), ER.latent_sample(oracle.lib(), m, None, enc.scaling_factor), "encode(image)")
    assert torch.equal(bits(enc(small["image"], noise)), bits(z))                       # forward is encode
    # channels-last noise is taken as it is
    assert torch.equal(bits(enc.encode(small["image"], noise.contiguous(memory_format=torch.channels_last))), bits(z))


def test_vae_image_dtypes_and_strides(small):
    from mixdq_amd import vae as V
    enc, image = small["enc"], small["image"]
    px = V.to_uint8(image)
    assert px.dtype == torch.uint8
    want = enc.moments(V.from_uint8(px))
    assert torch.equal(bits(enc.moments(px)), bits(want))
    nhwc = px.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)                   # as an image file is decoded
    assert torch.equal(bits(enc.moments(nhwc)), bits(want))
    assert torch.equal(bits(enc.moments(image.half())), bits(small["moments"]))         # FP32 and its FP16 rounding
    assert torch.equal(bits(enc.encode(px, small["noise"])), bits(enc.encode(V.from_uint8(px), small["noise"])))


def test_vae_batch_row_equals_the_image_alone(small):
    enc = small["enc"]
    for i in range(2):
        alone = enc.encode(small["image"][i:i + 1], small["noise"][i:i + 1])
        assert torch.equal(bits(alone), bits(small["latents"][i:i + 1])), i
        assert torch.equal(bits(enc.moments(small["image"][i:i + 1])), bits(small["moments"][i:i + 1])), i


def test_vae_graph_replay_equals_eager_bit_for_bit(small):
    from mixdq_amd import vae as V
    from mixdq_amd.quantize_sdxl import hip_graph_opt
    enc = V.build_vae_encoder(small["cfg"], seed=11, device=DEV)
    hip_graph_opt(enc)
    first = enc.encode(small["image"], small["noise"]).clone()
    assert torch.equal(bits(first), bits(small["latents"]))
    image2, noise2 = small["image"].flip(0).contiguous(), small["noise"].flip(0).contiguous()
    eager = small["enc"].encode(image2, noise2)
    assert torch.equal(bits(enc.encode(image2, noise2)), bits(eager))              # the same graph on a second input
    assert len(enc.forward._cached) == 1
    assert torch.equal(bits(enc.encode(small["image"], small["noise"])), bits(small["latents"]))


def test_vae_graph_replay_sees_a_later_load_state_dict(small):
    """A captured encode holds the addresses of the parameters AND of the tensors derived from them (q|k|v, the
    8-channel conv_in) and of the GroupNorm workspaces; load_state_dict rewrites the first two in place and keeps the
    third, so a replay computes with the new weights."""
    from mixdq_amd import vae as V
    from mixdq_amd.quantize_sdxl import hip_graph_opt
    image, noise = small["image"], small["noise"]
    enc = V.build_vae_encoder(small["cfg"], seed=11, device=DEV)
    donor = V.build_vae_encoder(small["cfg"], seed=12, device=DEV)
    want = donor.encode(image, noise)
    hip_graph_opt(enc)
    before = enc.encode(image, noise).clone()
    assert torch.equal(bits(before), bits(small["latents"]))
    held = {k: list(v) for k, v in enc._derived().items()}          # (kept alive: their addresses cannot be handed out again)
    ptrs = {k: [t.data_ptr() for t in v] for k, v in held.items()}
    assert set(ptrs) == {"qkv", "conv_in"}
    ws = {k: v.data_ptr() for k, v in enc._gn_ws.items()}
    assert ws
    enc.load_state_dict(donor.state_dict())
    assert {k: [t.data_ptr() for t in v] for k, v in enc._derived().items()} == ptrs
    assert {k: v.data_ptr() for k, v in enc._gn_ws.items()} == ws
    after = enc.encode(image, noise)
    assert len(enc.forward._cached) == 1                               # a replay, not a new capture
    assert torch.equal(bits(after), bits(want))
    assert not torch.equal(bits(after), bits(before))


def test_encode_refuses_what_it_cannot_run(small):
    enc, image, noise = small["enc"], small["image"], small["noise"]
    for bad in (image[:, :2], image[:, :, :60], image.double(), image[0]):
        with pytest.raises(RuntimeError, match="image should be"):
            enc.encode(bad)
    for bad in (noise[:, :, :7], noise.half(), noise.cpu(), noise[:1]):
        with pytest.raises(RuntimeError, match="noise should be"):
            enc.encode(image, bad)
    from mixdq_amd import vae as V
    with pytest.raises(RuntimeError, match="FP16"):
        V.build_vae_encoder(small["cfg"], device=DEV, dtype=torch.float32).encode(image)
