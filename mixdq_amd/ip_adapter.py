"""IP-Adapter: image-prompt conditioning through decoupled cross-attention.

An adapter brings, per cross-attention of the UNet, a bias-free `to_k_ip` / `to_v_ip` pair that projects a few image
tokens to extra keys and values; the cross-attention becomes

    out = attn(q, K_text, V_text) + s * attn(q, K_ip, V_ip)

(diffusers' IPAdapterAttnProcessor2_0), which `SDXLUNet.forward(ip=IPState(...))` runs as ONE mixdq_attention_f16_ip
launch per layer.  The image keys and values do not change during a run: `IPAdapter.tokens` and `IPAdapter.kv` compute
them once per run, outside a captured graph.

Parameter names are the published checkpoint's: `image_proj.proj`, `image_proj.norm`, `ip_adapter.<i>.to_k_ip` /
`to_v_ip` with i = 2 n + 1, n counting the UNet's transformer blocks (one cross-attention each) in registration order:
down, mid, up.  diffusers is not available where this was written: that index rule is NOT verified against its loader.
The image embeddings come from mixdq_amd.vision (`vision(image).image_embeds`) or from the caller.

The "plus" adapters (ip-adapter-plus_sd15, -plus-face_sd15, -plus_sdxl_vit-h) replace `image_proj` by a Resampler: a
perceiver in which `num_tokens` learned latent rows attend to the vision tower's `penultimate` hidden states and to
themselves (`build_ip_adapter(..., resampler=RESAMPLER_PLUS_SD15)`).  Its parameter names and
its forward are those of Tencent's `resampler.py` as remembered: neither that file nor diffusers is available where
this was written, so both are NOT verified against a published checkpoint.
Not here: ip_adapter_masks, FaceID's projection and LoRA, quantized to_k_ip / to_v_ip or Resampler layers, the
257-token "full-face" projections, real weights.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from mixdq_amd import derived


class IPState:
    """What SDXLUNet.forward(ip=...) reads: `kv` -- per adapter (1 to 4) the [R, T_j, sum_l 2 C_l] tensor IPAdapter.kv
    returned, layer l's k | v at columns IPAdapter.offsets[l] (one row per sample row) -- and `scales`, FP32
    [layers, n_ip] on the sample's device: cross-attention l reads row l (per-block scales work), in the kernel."""

    def __init__(self, kv, scales):
        self.kv = list(kv)
        self.scales = scales


def cross_attention_dims(unet_cfg):
    """(cross_attention_dim, [C_l of every cross-attention in registration order]) of the UNet this config builds."""
    from mixdq_amd.unet import SDXLUNet, cross_attentions
    with torch.device("meta"):
        unet = SDXLUNet(unet_cfg)
    attns = cross_attentions(unet)
    return attns[0].to_k.in_features, [a.to_k.out_features for a in attns]


class _ImageProj(nn.Module):
    def __init__(self, clip_embed_dim, cross_dim, num_tokens):
        super().__init__()
        self.proj = nn.Linear(clip_embed_dim, num_tokens * cross_dim)
        self.norm = nn.LayerNorm(cross_dim)


RESAMPLER_PLUS_SD15 = dict(dim=768, depth=4, dim_head=64, heads=12, embedding_dim=1280, ff_mult=4)
RESAMPLER_PLUS_SDXL = dict(dim=1280, depth=4, dim_head=64, heads=20, embedding_dim=1280, ff_mult=4)


class _PerceiverAttention(nn.Module):
    def __init__(self, dim, dim_head, heads):
        super().__init__()
        self.heads, self.dim_head = heads, dim_head
        self.norm1 = nn.LayerNorm(dim)                 # of the image tokens
        self.norm2 = nn.LayerNorm(dim)                 # of the latents
        self.to_q = nn.Linear(dim, dim_head * heads, bias=False)
        self.to_kv = nn.Linear(dim, 2 * dim_head * heads, bias=False)
        self.to_out = nn.Linear(dim_head * heads, dim, bias=False)

    def forward(self, x, lat):
        """Stock torch: softmax(q [k_x ; k_lat]^T / sqrt(d)) [v_x ; v_lat], the scale applied once to the product
        (upstream scales q and k by d ** -0.25 each), the softmax in FP32."""
        ln = self.norm2(lat)
        B, T, _ = lat.shape
        q = self.to_q(ln)
        k, v = self.to_kv(torch.cat([self.norm1(x), ln], dim=1)).chunk(2, dim=-1)
        q, k, v = (t.reshape(B, t.shape[1], self.heads, self.dim_head).transpose(1, 2) for t in (q, k, v))
        w = torch.softmax((q @ k.transpose(-1, -2)).float() * self.dim_head ** -0.5, dim=-1).to(v.dtype)
        return self.to_out((w @ v).transpose(1, 2).reshape(B, T, -1))


class Resampler(nn.Module):
    """`image_proj` of a "plus" adapter: hidden [B, n1, embedding_dim] -> [B, num_queries, output_dim].

        x = proj_in(hidden);  per layer: lat += to_out(attn(q = to_q(norm2(lat)), kv = to_kv([norm1(x) ; norm2(lat)])))
                                         lat += ff(lat)        (LayerNorm, Linear, GELU (erf), Linear; no biases)
        return norm_out(proj_out(lat))

    On the GPU in FP16 (dim_head 64, num_queries <= 16, B * num_queries <= 256 rows) this is 5 * depth + 5 launches
    (and the copy of the latents) up to 16 rows, a few more above (`_linear`), and no concatenation: proj_in, ONE unit
    LayerNorm of x (x does not change between layers, only norm1's affine does), ONE GEMM against every layer's to_kv with that affine folded in, then per layer
    mixdq_linear_f16_skinny (norm2 + [to_q ; to_kv]), mixdq_attention_f16_perceiver (image keys and latent keys in one
    softmax), and three more skinny launches (to_out + residual, LayerNorm + fc1 + GELU, fc2 + residual), then
    proj_out and norm_out.  Everything else runs `_forward_torch`, the stock network."""

    def __init__(self, dim, depth, dim_head, heads, num_queries, embedding_dim, output_dim, ff_mult=4):
        super().__init__()
        self.dim, self.depth, self.dim_head, self.heads = dim, depth, dim_head, heads
        self.num_queries, self.embedding_dim, self.output_dim = int(num_queries), embedding_dim, output_dim
        self.latents = nn.Parameter(torch.randn(1, self.num_queries, dim) / dim ** 0.5)
        self.proj_in = nn.Linear(embedding_dim, dim)
        self.proj_out = nn.Linear(dim, output_dim)
        self.norm_out = nn.LayerNorm(output_dim)
        self.layers = nn.ModuleList([
            nn.ModuleList([_PerceiverAttention(dim, dim_head, heads),
                           nn.Sequential(nn.LayerNorm(dim), nn.Linear(dim, dim * ff_mult, bias=False), nn.GELU(),
                                         nn.Linear(dim * ff_mult, dim, bias=False))])
            for _ in range(depth)])

    def _forward_torch(self, hidden):
        x = self.proj_in(hidden)
        lat = self.latents.expand(hidden.shape[0], -1, -1)
        for attn, ff in self.layers:
            lat = lat + attn(x, lat)
            lat = lat + ff(lat)
        return self.norm_out(self.proj_out(lat))

    def folded_kv(self):
        """(weight [depth * 2 * inner, dim], bias [depth * 2 * inner]): row block l is to_kv_l . diag(gamma1_l) with
        bias to_kv_l . beta1_l, so that one GEMM on the unit-normalised x gives every layer's to_kv(norm1(x)).  Folded
        in FP32, rounded once; a derived tensor (rebuilt in place when a source was written)."""
        src = [t for attn, _ in self.layers for t in (attn.to_kv.weight, attn.norm1.weight, attn.norm1.bias)]

        def build(old, *ts):
            ct = torch.promote_types(ts[0].dtype, torch.float32)             # FP32 for FP16 weights
            ws = [ts[i].to(ct) * ts[i + 1].to(ct)[None, :] for i in range(0, len(ts), 3)]
            bs = [ts[i].to(ct) @ ts[i + 2].to(ct) for i in range(0, len(ts), 3)]
            return torch.cat(ws, dim=0).to(ts[0].dtype), torch.cat(bs, dim=0).to(ts[0].dtype)
        return derived.derive(derived.holder_of(self), "kv_fold", src, build)

    def _stacked_qkv(self, i):
        attn = self.layers[i][0]
        return derived.derive(derived.holder_of(self), ("qkv", i), [attn.to_q.weight, attn.to_kv.weight],
                              lambda old, q, kv: (torch.cat([q, kv], dim=0),))[0]

    def _unit(self):
        w = self.proj_in.weight
        return derived.derive(derived.holder_of(self), "unit", [],
                              lambda old: (torch.ones(self.dim, dtype=w.dtype, device=w.device),
                                           torch.zeros(self.dim, dtype=w.dtype, device=w.device)))

    def _fast(self, hidden):
        from mixdq_amd import _C
        inner, rows = self.dim_head * self.heads, hidden.shape[0] * self.num_queries
        hid = self.layers[0][1][1].out_features if self.depth else self.dim
        return (hidden.is_cuda and hidden.dtype == torch.float16 and self.proj_in.weight.dtype == torch.float16
                and self.depth > 0 and self.dim_head == 64 and self.num_queries <= _C.PERCEIVER_MAX_Q
                and hidden.shape[1] + self.num_queries <= _C.PERCEIVER_MAX_KEYS
                and self.dim % 16 == 0 and self.dim <= 2048 and self.output_dim % 16 == 0 and self.output_dim <= 2048
                and _C.linear_f16_skinny_supported(rows, 3 * inner, self.dim, ln=True)
                and _C.linear_f16_skinny_supported(rows, self.dim, inner)
                and _C.linear_f16_skinny_supported(rows, hid, self.dim, ln=True)
                and _C.linear_f16_skinny_supported(rows, self.dim, hid)
                and _C.linear_f16_skinny_supported(rows, self.output_dim, self.dim))

    @torch.no_grad()
    def forward(self, hidden):
        if not self._fast(hidden):
            return self._forward_torch(hidden)
        from mixdq_amd import _C
        B, inner = hidden.shape[0], self.dim_head * self.heads
        x = _C.linear_f16(hidden, self.proj_in.weight, self.proj_in.bias)
        one, zero = self._unit()
        xh = _C.layernorm_quantize(x, one, zero, self.layers[0][0].norm1.eps, [], want_f16=True)[1]
        wf, bf = self.folded_kv()
        kv = _C.linear_f16(xh, wf, bf)                                       # [B, n1, depth * 2 * inner]
        lat = self.latents.repeat(B, 1, 1)               # a copy at every B: the layers write it in place
        for i, (attn, ff) in enumerate(self.layers):
            qkv = self._linear(lat, self._stacked_qkv(i), ln=attn.norm2)
            c0 = 2 * inner * i
            o = _C.attention_perceiver(qkv[..., :inner], kv[..., c0:c0 + inner], kv[..., c0 + inner:c0 + 2 * inner],
                                       qkv[..., inner:2 * inner], qkv[..., 2 * inner:], self.heads)
            lat = self._linear(o, attn.to_out.weight, residual=lat)
            h = self._linear(lat, ff[1].weight, ln=ff[0], act="gelu")
            lat = self._linear(h, ff[3].weight, residual=lat)
        y = self._linear(lat, self.proj_out.weight, self.proj_out.bias)
        n = self.norm_out
        return _C.layernorm_quantize(y, n.weight, n.bias, n.eps, [], want_f16=True)[1]

    # Above one 16-row tile every row tile of mixdq_linear_f16_skinny streams the weight again (and repeats the
    # LayerNorm prologue per column tile).  Measured at 64 rows (profiles/resampler_bench.txt): the LayerNorm forms lose
    # to the LayerNorm launch + mixdq_linear_f16 at three shapes of four, the plain forms win up to 768 x 3072 weights
    # and are level or behind above -- those calls take the existing launches.
    SKINNY_WEIGHT_ABOVE_ONE_TILE = 768 * 3072

    def _linear(self, x, w, bias=None, residual=None, ln=None, act=None):
        from mixdq_amd import _C
        rows = x.numel() // x.shape[-1]
        if rows <= 16 or (ln is None and w.numel() <= self.SKINNY_WEIGHT_ABOVE_ONE_TILE):
            return _C.linear_f16_skinny(x, w, bias, residual=residual, out=residual, act=act,
                                        ln=None if ln is None else (ln.weight, ln.bias, ln.eps))
        if ln is not None:
            x = _C.layernorm_quantize(x, ln.weight, ln.bias, ln.eps, [], want_f16=True)[1]
        return _C.linear_f16(x, w, bias, _residual=residual, _act=act)

    def _apply(self, fn, recurse=True):                # a move or a dtype change: the derived tensors go with it
        derived.drop(derived.holder_of(self))
        return super()._apply(fn, recurse)


class _IPLayer(nn.Module):
    def __init__(self, cross_dim, dim):
        super().__init__()
        self.to_k_ip = nn.Linear(cross_dim, dim, bias=False)
        self.to_v_ip = nn.Linear(cross_dim, dim, bias=False)


class IPAdapter(nn.Module):
    def __init__(self, unet_cfg, clip_embed_dim, num_tokens=4, resampler=None):
        super().__init__()
        self.cross_dim, self.dims = cross_attention_dims(unet_cfg)
        self.num_tokens = int(num_tokens)
        if resampler is None:
            self.image_proj = _ImageProj(clip_embed_dim, self.cross_dim, self.num_tokens)
        else:
            self.image_proj = Resampler(num_queries=self.num_tokens, output_dim=self.cross_dim, **resampler)
        self.ip_adapter = nn.ModuleDict({str(2 * n + 1): _IPLayer(self.cross_dim, c) for n, c in enumerate(self.dims)})
        self.offsets = [2 * sum(self.dims[:n]) for n in range(len(self.dims))]     # layer n: k at off, v at off + C_n

    def _fast(self, x):
        return x.is_cuda and x.dtype == torch.float16 and self.ip_adapter["1"].to_k_ip.weight.dtype == torch.float16

    @torch.no_grad()
    def tokens(self, image_embeds):
        """image_embeds [B, clip_embed_dim] -> [B, num_tokens, cross_dim]: the projection (mixdq_linear_f16) and the
        LayerNorm with FP16 output the text encoders use; stock torch on the CPU or for other dtypes.
        An adapter built with `resampler=` takes the vision tower's `penultimate` hidden states instead,
        [B, n1, embedding_dim], and returns the Resampler's [B, num_tokens, cross_dim]."""
        p = self.image_proj
        if isinstance(p, Resampler):
            if not (torch.is_tensor(image_embeds) and image_embeds.dim() == 3 and image_embeds.shape[2] == p.embedding_dim):
                raise RuntimeError(f"IPAdapter.tokens: this adapter has a Resampler: it reads hidden states "
                                   f"[B, n1, {p.embedding_dim}] (the vision tower's `penultimate`), not image_embeds")
            return p(image_embeds)
        if torch.is_tensor(image_embeds) and image_embeds.dim() == 3:
            raise RuntimeError(f"IPAdapter.tokens: this adapter has no Resampler: it reads image_embeds "
                               f"[B, {p.proj.in_features}], not hidden states (build it with resampler=...)")
        if not (torch.is_tensor(image_embeds) and image_embeds.dim() == 2
                and image_embeds.shape[1] == p.proj.in_features):
            raise RuntimeError(f"IPAdapter.tokens: image_embeds should be [B, {p.proj.in_features}]")
        if self._fast(image_embeds):
            from mixdq_amd import _C
            y = _C.linear_f16(image_embeds, p.proj.weight, p.proj.bias).reshape(-1, self.num_tokens, self.cross_dim)
            return _C.layernorm_quantize(y, p.norm.weight, p.norm.bias, p.norm.eps, [], want_f16=True)[1]
        return p.norm(p.proj(image_embeds).reshape(-1, self.num_tokens, self.cross_dim))

    def stacked_weight(self):
        """[sum_l 2 C_l, cross_dim]: every layer's to_k_ip then to_v_ip rows, through the version-keyed cache (rebuilt
        in place when a weight was written, so a captured reader keeps its address)."""
        ws = [w for n in range(len(self.dims)) for w in (self.ip_adapter[str(2 * n + 1)].to_k_ip.weight,
                                                         self.ip_adapter[str(2 * n + 1)].to_v_ip.weight)]
        return derived.derive(derived.holder_of(self), "ip_kv", ws, lambda old, *w: (torch.cat(w, dim=0),))[0]

    @torch.no_grad()
    def kv(self, tokens):
        """tokens [R, T, cross_dim] -> [R, T, sum_l 2 C_l]: ONE mixdq_linear_f16 launch against the row-stacked
        weight; layer l's keys are columns offsets[l] .. + C_l, its values the C_l columns behind them."""
        if not (torch.is_tensor(tokens) and tokens.dim() == 3 and tokens.shape[2] == self.cross_dim):
            raise RuntimeError(f"IPAdapter.kv: tokens should be [R, T, {self.cross_dim}]")
        w = self.stacked_weight()
        if self._fast(tokens):
            from mixdq_amd import _C
            return _C.linear_f16(tokens, w, None)
        return F.linear(tokens, w)

    def _apply(self, fn, recurse=True):                # a move or a dtype change: the stacked weight goes with it
        derived.drop(derived.holder_of(self))
        return super()._apply(fn, recurse)


def build_ip_adapter(unet_cfg, clip_embed_dim, num_tokens=4, resampler=None, device=None, dtype=torch.float16, seed=4343):
    """An IPAdapter for the UNet `unet_cfg` builds, with synthetic weights (deterministic in `seed`).  `resampler`:
    None (the linear image projection) or a Resampler config -- dim, depth, dim_head, heads, embedding_dim, ff_mult,
    e.g. RESAMPLER_PLUS_SD15 -- for a "plus" adapter (num_queries = num_tokens, output_dim = the UNet's cross dimension)."""
    if device is not None and torch.device(device).type == "meta":
        with torch.device("meta"):
            return IPAdapter(unet_cfg, clip_embed_dim, num_tokens, resampler)
    ad = IPAdapter(unet_cfg, clip_embed_dim, num_tokens, resampler)
    g = torch.Generator().manual_seed(seed)
    gains = {n + ".weight" for n, m in ad.named_modules() if isinstance(m, nn.LayerNorm)}
    with torch.no_grad():
        for name, p in ad.named_parameters():
            if p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=g) * (p.shape[1] ** -0.5))
            elif name in gains:
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    ad = ad.to(dtype=dtype)
    return (ad.to(device) if device is not None else ad).eval()
