"""LoRA adapters on a QUANTIZED UNet: W' = W + sum_j s_j (alpha_j / r_j) B_j A_j is formed once per adapter change,
quantized with each layer's own quantizer and written in place into the buffers the kernels already read -- one
`_C.lora_requant` launch over every targeted layer (csrc/lora.hip).  A step costs what it costs
without an adapter, and captured graphs read the new weights at the old addresses.

    bank = LoraBank(unet, float_state, bos_embedding=ehs[:1, 0])      # float_state: {"<module>.weight": tensor}
    bank.apply([{"down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_q": (A, B, alpha), ...}], [0.8])
    bank.set_scales([0.4]); bank.restore()

The activation quantizers stay as calibrated (the reference calibrates after fusing LoRA into the float weights; here
that is a limit).  LoHa terms and DoRA magnitudes come as dict values of apply() and go through `_C.lycoris_requant`
(csrc/lycoris.hip).  W2-stored layers, text encoders, LoKr, Tucker forms and key-format parsing
are not here."""
from __future__ import annotations

import torch

from mixdq_amd import _C
from mixdq_amd.nn import QuantizedConv2d, QuantizedLinear

_VECS = ("weight_scales", "weight_sum_by_input_channels", "bias0", "scale")


def conv_factor_stored(A: torch.Tensor) -> torch.Tensor:
    """A conv's down factor [r, C, R, S] in the layer's stored column order: [r, R * S * C] (channels-last)."""
    return A.permute(0, 2, 3, 1).reshape(A.shape[0], -1)


def _touch(t):
    """The launch wrote `t` behind torch's back: bump its version so that derived tensors see it (derived.py)."""
    if t is not None:
        torch.autograd.graph.increment_version(t)


class _Target:
    """One descriptor: a layer, or one half of a split conv_shortcut (its `_0` buffers over a column range)."""

    def __init__(self, name, mod, sfx, master, col0, kf, rank, rule, row_map, w_bit=None):
        dev = master.device
        self.name, self.mod, self.sfx, self.col0, self.kf = name, mod, sfx, col0, kf
        self.N = master.shape[0]
        self.Bcat = torch.zeros((self.N, rank), dtype=torch.float16, device=dev)
        self.Acat = torch.zeros((rank, kf), dtype=torch.float16, device=dev)
        self.svec = torch.zeros(rank, dtype=torch.float32, device=dev)
        self.B2cat = self.A2cat = self.mag = None              # LoHa's second factors, DoRA's magnitude: made when first needed
        conv = isinstance(mod, QuantizedConv2d)
        get = lambda n: getattr(mod, n + sfx, None)            # noqa: E731
        self.written = []
        part = master[:, col0:col0 + kf]
        if not mod.valid_for_acceleration:
            out, mode, bits, tap, vec = mod.weight, _C.LORA_F16, 8, kf, {}
            if out.dtype != torch.float16:
                raise ValueError(f"LoraBank: {name}: an FP-fallback layer needs an FP16 weight")
            if conv and not out.is_contiguous(memory_format=torch.channels_last):
                # KRSC in memory, as the FP16 conv kernel wants it, in the SAME storage: the buffer's address stays
                krsc = out.contiguous(memory_format=torch.channels_last)
                out.as_strided_(out.shape, krsc.stride()).copy_(krsc)
            exact = torch.equal(part, (out.permute(0, 2, 3, 1) if conv else out).reshape(self.N, -1))
        else:
            if getattr(mod, "w_packed2", False):
                raise ValueError(f"LoraBank: {name} stores 2-bit weights (weight_int2): not supported")
            out = get("weight_int4") if mod.w_packed4 else get("weight_int")
            mode = _C.LORA_W4 if mod.w_packed4 else _C.LORA_INT8
            vec = {n: get(n) for n in _VECS}
            tap = kf
            if conv and vec["weight_sum_by_input_channels"] is not None:      # a padded conv: per-tap sums
                tap = mod.in_channels
            self.written = [v for v in vec.values() if v is not None]
        dense = out.permute(0, 2, 3, 1) if out.dim() == 4 else out
        if not dense.is_contiguous():
            raise ValueError(f"LoraBank: {name}: the stored weight is not dense in [N, R*S*C] order")
        if mod.valid_for_acceleration:
            bits, exact = self._quantizer_bits(name, mod, part, dense.reshape(self.N, -1), vec["weight_scales"], row_map, w_bit)
        # what restore() copies back: the FP32 vectors always (KEEP reads the scales), the weight itself only where
        # re-quantizing the master does not give it back (an FP32 float_state)
        self.out, self.written = out, self.written + [out]
        self.snapshot = [t.clone() if t.dtype == torch.float32 or not exact else None for t in self.written]
        self.bos_snapshot = mod.bos_pre_computed.clone() if getattr(mod, "bos", False) else None
        self.keep, self.bos_base = (master, row_map), None
        p = lambda t: None if t is None else t.data_ptr()      # noqa: E731
        self.desc = _C.LoraLayer(
            W=master.data_ptr(), Bcat=self.Bcat.data_ptr(), Acat=self.Acat.data_ptr(), svec=self.svec.data_ptr(),
            row_map=p(row_map), out=out.data_ptr(), weight_scales=p(vec.get("weight_scales")),
            wsum=p(vec.get("weight_sum_by_input_channels")), bias0=p(vec.get("bias0")), scale=p(vec.get("scale")),
            act_scale=p(get("act_scales")), act_zero_point=p(get("act_zero_points")), ldw=master.stride(0), w_col0=col0,
            N=self.N, Kf=kf, R=rank, mode=mode, rule=rule, bits=bits, tap_len=tap)


    @staticmethod
    def _quantizer_bits(name, mod, part, stored, scales, row_map, w_bit):
        """(width of the layer's weight quantizer, whether re-quantizing the master gives the stored integers back).
        A module does not always record the width (QuantizedLinear keeps none; q|k|v groups are widened to one storage
        kind): with no `w_bit` given it is the NARROWEST one under which from_float's arithmetic on the master
        reproduces the stored integers -- a wider layer does not survive a narrower clamp, while a narrow layer also
        reproduces under a wider one (its delta keeps it inside its own range) and would then be clamped and rounded
        wrongly once an adapter is on it -- and a layer that reproduces under none is refused by name."""
        from mixdq_amd.nn.utils import unpack_w4
        if mod.w_packed4:
            stored = unpack_w4(stored)
        rm = slice(None) if row_map is None else row_map.long()
        stored, d, w = stored[rm], scales[rm], part.float()
        known = w_bit if w_bit is not None else getattr(mod, "w_bit", None)
        for bits in ((2, 4, 8) if not mod.w_packed4 else (2, 4)) if known is None else (int(known),):
            if bits == 8:
                q = torch.quantize_per_channel(w, d, torch.zeros_like(d), 0, torch.qint8).int_repr()
            else:
                q = torch.clamp(torch.round(w / d[:, None]), -2 ** (bits - 1), 2 ** (bits - 1) - 1).to(torch.int8)
            if torch.equal(q, stored):
                return bits, True
        if known is None:
            raise ValueError(f"LoraBank: {name}: float_state does not reproduce the stored integers under any weight "
                             "width; pass w_bits={name: bits} (and the weights the UNet was quantized from)")
        return int(known), False


class LoraBank:
    """Adapters on a quantized UNet (fused or not, module-swapped or this project's own graph).

    float_state:   {"<module name>.weight": tensor}, the FP16 / FP32 weights the UNet was quantized from; kept as FP16
                   masters on the device in stored order (a conv's [K, C, R, S] becomes [K, R*S*C]), per targeted layer.
    bos_embedding: the token-0 embedding [K]; needed once a BOS layer (attn2.to_k / to_v) is targeted.
    max_rank:      rows of the static factor buffers of every targeted layer: the summed rank of one apply() may not
                   exceed it (a multiple of 32, at most 256; ranks beyond the adapters' own are zero).
    scales:        'absmax' re-derives every row's weight scale from max |W'|; 'keep' leaves the calibrated ones.
    w_bits:        {module name: weight bit width} where the caller knows it (the config the UNet was quantized with);
                   otherwise a conv's recorded `w_bit`, otherwise found from the stored integers (_quantizer_bits).
    Factor buffers, svec, the descriptor table and a snapshot of every buffer the launch may overwrite are made the first
    time a layer is targeted; a later apply() on the same layers allocates nothing."""

    def __init__(self, unet, float_state, *, bos_embedding=None, max_rank=256, scales="absmax", w_bits=None):
        if scales not in ("absmax", "keep"):
            raise ValueError("scales: 'absmax' or 'keep'")
        if max_rank % 32 or not 32 <= max_rank <= 256:
            raise ValueError("max_rank: a multiple of 32, at most 256")
        self.unet, self.max_rank, self.bos_embedding = unet, max_rank, bos_embedding
        self.rule = _C.LORA_ABSMAX if scales == "absmax" else _C.LORA_KEEP
        self.modules = {n: m for n, m in unet.named_modules() if isinstance(m, (QuantizedLinear, QuantizedConv2d))}
        self.float_state, self.w_bits = float_state, dict(w_bits or {})
        self.targets, self.table, self.keep_table, self.adapters = {}, None, None, []
        self.lyco = None                                       # the LoHa / DoRA state of the last apply(), if it had any

    # ---- the static side: masters, factor buffers, descriptors -- built once per set of targeted layers
    def _row_map(self, name, mod):
        for owner in self.unet.modules():
            if owner.__dict__.get("_interleaved") and owner.net[0].proj is mod:
                perm = _C.geglu_row_order(mod.out_features // 2, mod.weight_scales.device)
                return torch.argsort(perm).to(torch.int32)     # logical row -> where it is stored
        return None

    def _make_targets(self, name):
        if name not in self.modules:
            raise KeyError(f"LoraBank: {name} matches no quantized Linear or Conv2d of the UNet")
        mod = self.modules[name]
        key = name + ".weight"
        if key not in self.float_state:
            raise KeyError(f"LoraBank: float_state has no {key}")
        if getattr(mod, "bos", False) and self.bos_embedding is None:
            raise ValueError(f"LoraBank: {name} is a BOS layer (its token-0 row is precomputed): pass bos_embedding=")
        dev = next(b.device for b in mod.buffers())
        w = self.float_state[key].detach().to(dev, torch.float16)
        if w.dim() == 4:
            w = w.permute(0, 2, 3, 1)
        master = w.reshape(w.shape[0], -1).contiguous()
        split = getattr(mod, "split", 0) if mod.valid_for_acceleration else 0
        if split and master.shape[1] != mod.in_channels:
            raise ValueError(f"LoraBank: {name}: a split layer must be 1x1")
        parts = [("", 0, master.shape[1])] if not split else [("", 0, split), ("_0", split, master.shape[1] - split)]
        rm = self._row_map(name, mod) if isinstance(mod, QuantizedLinear) and mod.valid_for_acceleration else None
        return [_Target(name, mod, sfx, master, c0, kf, self.max_rank, self.rule, rm, self.w_bits.get(name))
                for sfx, c0, kf in parts]

    def _tables(self, names):
        for n in names:
            if n not in self.targets:
                self.targets[n] = self._make_targets(n)
                self.table = None
        if self.table is None:
            flat = [t for ts in self.targets.values() for t in ts]
            dev = flat[0].Bcat.device

            def make(rule):
                descs = []
                for t in flat:
                    d = _C.LoraLayer.from_buffer_copy(t.desc)
                    d.rule = rule
                    descs.append(d)
                return _C.LoraTable(descs, dev, keep=flat)
            self.table, self.keep_table = make(self.rule), make(_C.LORA_KEEP)

    # ---- the dynamic side
    def apply(self, adapters, scales):
        """adapters: list of {module name: (A [r, ...], B [N, r], alpha)}; scales: one strength per adapter.

        A value may also be a dict (LyCORIS's hada_* tensors, PEFT's lora_magnitude_vector / kohya's dora_scale, brought
        by module name):
            {"kind": "lora", "A": [r, ...], "B": [N, r], "alpha": a, "magnitude": m [N]}           DoRA (magnitude optional)
            {"kind": "loha", "w1_a": [N, r], "w1_b": [r, ...], "w2_a": [N, r], "w2_b": [r, ...], "alpha": a}
        A dict's conv factor is [r, C, R, S] or flat [r, C*R*S] in (C, R, S) order.  W' = g (W + sum_j s_j dW_j) with
        g[n] = m[n] / ||row n||: the strength scales dW only, as PEFT does.  An adapter whose strength is exactly 0 is
        skipped TOGETHER WITH its magnitude: 0 means off, and all-zero strengths give what no adapter gives.  An apply()
        of tuples only launches what it always did (_C.lora_requant); any dict routes the launch to _C.lycoris_requant
        (csrc/lycoris.hip), where a Hadamard term takes its rank rounded up to 32 of max_rank."""
        if len(adapters) != len(scales):
            raise ValueError("one scale per adapter")
        if any(isinstance(v, dict) for ad in adapters for v in ad.values()):
            return self._apply_lycoris(adapters, scales)
        self.lyco = None
        names = sorted({n for ad in adapters for n in ad})
        self._tables(names)
        self.adapters = []
        for ts in self.targets.values():
            for t in ts:
                t.Bcat.zero_(), t.Acat.zero_(), t.svec.zero_()
        used = {}
        for j, ad in enumerate(adapters):
            spans = {}
            for name, (A, B, alpha) in ad.items():
                ts = self.targets[name]
                r = A.shape[0]
                A2 = conv_factor_stored(A) if A.dim() == 4 else A
                kf = sum(t.kf for t in ts)
                if B.shape != (ts[0].N, r) or A2.shape != (r, kf):
                    raise ValueError(f"LoraBank: {name}: factors {tuple(A.shape)}, {tuple(B.shape)} do not fit a "
                                     f"[{ts[0].N}, {kf}] layer")
                r0 = used.get(name, 0)
                if r0 + r > self.max_rank:
                    raise ValueError(f"LoraBank: {name}: summed rank {r0 + r} exceeds max_rank {self.max_rank}")
                used[name] = r0 + r
                for t in ts:
                    t.Bcat[:, r0:r0 + r] = B.to(t.Bcat)
                    t.Acat[r0:r0 + r] = A2[:, t.col0:t.col0 + t.kf].to(t.Acat)
                spans[name] = (r0, r, float(alpha) / r)
            self.adapters.append(spans)
        self.set_scales(scales)

    def set_scales(self, scales):
        """New strengths for the adapters of the last apply(): rewrites svec and relaunches; copies no factor."""
        if len(scales) != len(self.adapters):
            raise ValueError("one scale per adapter of the last apply()")
        for spans, s in zip(self.adapters, scales):
            for name, (r0, r, unit) in spans.items():
                for t in self.targets[name]:
                    t.svec[r0:r0 + r] = float(s) * unit
        if self.lyco is not None:                              # a magnitude is on exactly while its adapter's strength is not 0
            self.lyco["on"] = {n for n, (j, _) in self.lyco["magnitude"].items() if float(scales[j]) != 0.0}
        self._launch(self.table)

    def restore(self):
        """Every buffer bit-identical to before the first apply(): the snapshot's scales, no adapter."""
        if not self.targets:
            return
        for t in (t for ts in self.targets.values() for t in ts):
            t.svec.zero_()
            for dst, src in zip(t.written, t.snapshot):          # (the scales KEEP reads; the launch rewrites the rest)
                if src is not None and src.dtype == torch.float32:
                    dst.copy_(src)
        self.adapters, self.lyco = [], None
        self._launch(self.keep_table, restoring=True)

    # ---- LoHa / DoRA: the same buffers with rank ranges, second factors and a magnitude (csrc/lycoris.hip)
    @staticmethod
    def _term(name, v):
        """One adapter value -> ('lin' | 'had', factors, alpha, magnitude or None)."""
        if not isinstance(v, dict):
            A, B, alpha = v
            return "lin", (A, B), alpha, None
        if any(k in v for k in ("hada_t1", "hada_t2", "t1", "t2")):
            raise ValueError(f"LoraBank: {name}: Tucker-form LoHa (hada_t1 / hada_t2) is not supported")
        kind = v.get("kind")
        if kind == "lora":
            return "lin", (v["A"], v["B"]), v["alpha"], v.get("magnitude")
        if kind == "loha":
            if v.get("magnitude") is not None:
                raise ValueError(f"LoraBank: {name}: a magnitude goes with a 'lora' term")
            return "had", (v["w1_b"], v["w1_a"], v["w2_b"], v["w2_a"]), v["alpha"], None
        raise ValueError(f"LoraBank: {name}: adapter kind {kind!r} is not 'lora' or 'loha'")

    def _stored_factor(self, name, A, r, from_dict):
        """A down factor in the layer's stored column order [r, Kf]; a dict's flat conv factor is in (C, R, S) order."""
        shape = tuple(self.float_state[name + ".weight"].shape)
        if from_dict and A.dim() == 2 and len(shape) == 4 and A.shape[1] == shape[1] * shape[2] * shape[3]:
            A = A.reshape((r,) + shape[1:])
        return conv_factor_stored(A) if A.dim() == 4 else A

    def _apply_lycoris(self, adapters, scales):
        parsed = [{n: self._term(n, v) + (isinstance(v, dict),) for n, v in ad.items()} for ad in adapters]
        names = sorted({n for ad in adapters for n in ad})
        self._tables(names)
        flat = [t for ts in self.targets.values() for t in ts]
        for t in flat:
            t.Bcat.zero_(), t.Acat.zero_(), t.svec.zero_()
        lyco = dict(ranges={}, magnitude={}, on=set())
        self.adapters = [{} for _ in adapters]
        for name in names:
            ts = self.targets[name]
            N, kf = ts[0].N, sum(t.kf for t in ts)
            terms = [(j,) + ad[name] for j, ad in enumerate(parsed) if name in ad]
            lin = [x for x in terms if x[1] == "lin"]
            had = [x for x in terms if x[1] == "had"]
            r_lin = -(-sum(x[2][0].shape[0] for x in lin) // 32) * 32
            total = r_lin + sum(-(-x[2][0].shape[0] // 32) * 32 for x in had)
            if total > self.max_rank:
                raise ValueError(f"LoraBank: {name}: summed rank {total} (every Hadamard term and the linear terms "
                                 f"together each padded to 32) exceeds max_rank {self.max_rank}")
            if len(had) > _C.LYCORIS_MAX_HADAMARD:
                raise ValueError(f"LoraBank: {name}: more than {_C.LYCORIS_MAX_HADAMARD} Hadamard terms")
            mags = [(j, m) for j, _, _, _, m, _ in terms if m is not None]
            if len(mags) > 1:
                raise ValueError(f"LoraBank: {name}: more than one magnitude on a layer")
            if mags and len(ts) > 1:
                raise ValueError(f"LoraBank: {name}: a magnitude on a split conv_shortcut is not supported (the row norm "
                                 "spans both halves)")
            if mags and mags[0][1].numel() != N:
                raise ValueError(f"LoraBank: {name}: the magnitude has {mags[0][1].numel()} elements, the layer {N} rows")
            if had:
                for t in ts:
                    if t.B2cat is None:      # the second factor buffers: the first time they are needed
                        t.B2cat, t.A2cat = torch.zeros_like(t.Bcat), torch.zeros_like(t.Acat)
                    t.B2cat.zero_(), t.A2cat.zero_()
            r0, ends = 0, []
            for j, kind, fac, alpha, _, from_dict in lin + had:
                r = fac[0].shape[0]
                if kind == "had":
                    r0 = r_lin if not ends else ends[-1]
                    ends.append(r0 + -(-r // 32) * 32)
                downs = [self._stored_factor(name, A, r, from_dict) for A in fac[0::2]]
                for A2, B in zip(downs, fac[1::2]):
                    if B.shape != (N, r) or A2.shape != (r, kf):
                        raise ValueError(f"LoraBank: {name}: factors {tuple(A2.shape)}, {tuple(B.shape)} do not fit a "
                                         f"[{N}, {kf}] layer")
                for t in ts:
                    for A2, B, Bd, Ad in zip(downs, fac[1::2], (t.Bcat, t.B2cat), (t.Acat, t.A2cat)):
                        Bd[:, r0:r0 + r] = B.to(Bd)
                        Ad[r0:r0 + r] = A2[:, t.col0:t.col0 + t.kf].to(Ad)
                self.adapters[j][name] = (r0, r, float(alpha) / r)
                r0 += r
            lyco["ranges"][name] = (r_lin, ends)
            if mags:
                t = ts[0]
                if t.mag is None:
                    t.mag = torch.zeros(N, dtype=torch.float32, device=t.Bcat.device)
                t.mag.copy_(mags[0][1].reshape(N).to(t.mag))
                lyco["magnitude"][name] = (mags[0][0], t.mag)
        self.lyco = lyco
        self.set_scales(scales)

    def _lycoris_table(self):
        """The descriptors of this state: every target's LoRA descriptor with its rank ranges, second factors and -- while
        its adapter is on -- its magnitude.  A target the last apply() did not name has no ranges: it is re-quantized
        from its master."""
        flat = [t for ts in self.targets.values() for t in ts]
        descs = []
        for t in flat:
            r_lin, ends = self.lyco["ranges"].get(t.name, (0, []))
            on = t.name in self.lyco["on"]
            d = _C.LycorisLayer.from_lora(t.desc, R_lin=r_lin, had_end=ends,
                                          B2cat=t.B2cat.data_ptr() if ends else None, A2cat=t.A2cat.data_ptr() if ends else None,
                                          magnitude=t.mag.data_ptr() if on else None)
            d.rule = self.rule
            descs.append(d)
        return _C.LycorisTable(descs, flat[0].Bcat.device, keep=flat)

    def _merged_f32(self, t):
        """W' of a layer in FP32 torch, from the master and the factor buffers: what the BOS row of a layer with a
        Hadamard term or a magnitude is computed from (a layer-sized temporary)."""
        r_lin, ends = self.lyco["ranges"].get(t.name, (0, []))
        bs = (t.svec * t.Bcat.float()).half().float()
        w = t.keep[0].float() + bs[:, :r_lin] @ t.Acat[:r_lin].float()
        for a, b in zip([r_lin] + ends[:-1], ends):
            w = w + (bs[:, a:b] @ t.Acat[a:b].float()) * (t.B2cat[:, a:b].float() @ t.A2cat[a:b].float())
        if t.name in self.lyco["on"]:
            ss = (w * w).sum(dim=1)
            w = w * torch.where(ss > 0, t.mag / ss.sqrt(), torch.ones_like(ss))[:, None]
        return w

    @torch.no_grad()
    def _launch(self, table, restoring=False):
        if self.lyco is not None and not restoring:
            self.lyco["table"] = self._lycoris_table()
            _C.lycoris_requant(self.lyco["table"])
        else:
            _C.lora_requant(table)
        for ts in self.targets.values():
            for t in ts:
                if restoring and t.snapshot[-1] is not None:     # a weight the master does not reproduce: its copy
                    t.out.copy_(t.snapshot[-1])
                for w in t.written:
                    _touch(w)
            self._bos(ts[0], restoring)
        for m in {id(t[0].mod): t[0].mod for t in self.targets.values()}.values():
            if hasattr(m, "refresh_derived_"):
                m.refresh_derived_()
        if hasattr(self.unet, "refresh_derived_"):
            self.unet.refresh_derived_()

    def _bos(self, t, restoring):
        """bos_pre_computed of a BOS layer follows: f16(x W^T + ((x A^T) s) B^T) in FP32, from the master."""
        if not getattr(t.mod, "bos", False):
            return
        if restoring:
            t.mod.bos_pre_computed.copy_(t.bos_snapshot)
            return
        x = self.bos_embedding.reshape(1, -1).to(t.Acat.device, torch.float32)
        if self.lyco is not None and (self.lyco["ranges"].get(t.name, (0, []))[1] or t.name in self.lyco["on"]):
            y = x @ self._merged_f32(t).t()                     # a Hadamard term or a row norm: from the merged weight
            t.mod.bos_pre_computed.copy_(y.to(torch.float16).reshape(t.mod.bos_pre_computed.shape))
            return
        if t.bos_base is None:                                 # x W^T, once (the only layer-sized FP32 temporary)
            t.bos_base = x @ t.keep[0].float().t()
        y = t.bos_base + ((x @ t.Acat.float().t()) * t.svec) @ t.Bcat.float().t()
        t.mod.bos_pre_computed.copy_(y.to(torch.float16).reshape(t.mod.bos_pre_computed.shape))
