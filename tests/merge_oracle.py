"""Merge-then-quantize: the independent definition of what LoraBank (mixdq_amd/lora.py) must leave in a quantized UNet.
The adapters are merged into the FLOAT weights in the weights' own [K, C, R, S] layout (float64), and the normal
quantize_unet path runs on the result -- that path, not the bank, decides every stored layout.  Nothing here imports
mixdq_amd.lora or reads what the bank staged.  The planting helpers make inputs on which every product, sum, FP16 cast
and scale is exact, so that the bank's UNet and the freshly quantized merged UNet have the same state_dict() bit for bit."""
from collections import OrderedDict

import numpy as np
import torch

UNIT = 2.0 ** -10                                  # every planted weight is an integer (or a quarter) times UNIT
QMAX = {8: 127, 4: 7, 2: 1}
ROW_MAX = {8: 127, 4: 112, 2: 128}                 # qmax * 2^j in UNITs: the planted row maximum (times 1 or 2)
NORM_ROWS = {8: (127, 15, 5, 2, 1), 4: (112, 48, 32, 16, 16)}      # squares sum to 16384 = 4^7: the row norm is 128


def _f64(x):
    return x.detach().to("cpu", torch.float64)


def term(v, shape):
    """One adapter value -> (dW in float64 in the weight's `shape`, alpha / r, magnitude or None).  A down factor is
    [r, C, R, S] or flat [r, C * R * S] in (C, R, S) order: row-major over the weight's trailing dimensions."""
    rest = tuple(shape[1:])
    if isinstance(v, dict) and v.get("kind") == "loha":
        p = [_f64(v[a]) @ _f64(v[b]).reshape(v[b].shape[0], -1) for a, b in (("w1_a", "w1_b"), ("w2_a", "w2_b"))]
        return (p[0] * p[1]).reshape(shape), float(v["alpha"]) / v["w1_b"].shape[0], None
    if isinstance(v, dict):
        assert v.get("kind") == "lora", v.get("kind")
        A, B, alpha, m = v["A"], v["B"], v["alpha"], v.get("magnitude")
    else:
        (A, B, alpha), m = v, None
    dW = torch.einsum("nr,r...->n...", _f64(B), _f64(A).reshape((A.shape[0],) + rest))
    return dW, float(alpha) / A.shape[0], m


def merged_f64(w, name, adapters, scales):
    """g * (W + sum_j s_j (alpha_j / r_j) dW_j) of one weight in float64, in the weight's own shape.  An adapter whose
    strength is exactly 0 is skipped together with its magnitude."""
    acc, mag = _f64(w).clone(), None
    for ad, s in zip(adapters, scales):
        if name not in ad or float(s) == 0.0:
            continue
        dW, unit, m = term(ad[name], tuple(w.shape))
        acc += float(s) * unit * dW
        if m is not None:
            assert mag is None, f"{name}: more than one magnitude"
            mag = _f64(m).reshape(-1)
    if mag is not None:
        norm = (acc * acc).flatten(1).sum(dim=1).sqrt()
        g = torch.where(norm > 0, mag / torch.where(norm > 0, norm, torch.ones_like(norm)), torch.ones_like(norm))
        acc = acc * g.reshape((-1,) + (1,) * (acc.dim() - 1))
    return acc


def merged_state(state, adapters, scales, exact=False):
    """A new {"<module>.weight": tensor, ...}: `state` with every targeted weight replaced by its merged weight, cast
    to FP16.  `exact`: the caller planted the inputs -- the cast must then lose nothing."""
    assert len(adapters) == len(scales)
    out = dict(state)
    for name in sorted({n for ad in adapters for n in ad}):
        w = state[name + ".weight"]
        acc = merged_f64(w, name, adapters, scales)
        h = acc.to(torch.float16)
        if exact:
            assert torch.equal(h.to(torch.float64), acc), f"{name}: the merged weight is not an FP16 value"
        out[name + ".weight"] = h.to(w.device)
    return out


def split_of(mod, name):
    """Where a float conv_shortcut of an up block is split (mixdq_amd.calib.calibrate's rule); 0: not split."""
    return getattr(mod, "split", 0) if ("up_blocks" in name and "conv_shortcut" in name) else 0


def oracle_unet(cfg, merged, ckpt, rule, *, qcfg, targets, ehs, device, inp=None, **flags):
    """(a fresh UNet holding `merged`, quantized like the unit under test and fused; its FLOAT output for `inp` or None).
    `ckpt`: the ORIGINAL calibration -- the activation quantizers stay as calibrated; under 'absmax' the weight
    quantizers of `targets` alone are those of the merged weights.  bos_dict: from the merged float UNet."""
    from mixdq_amd import unet as U
    from mixdq_amd.calib import precompute_bos, weight_quantizer_entry
    from mixdq_amd.quantize_sdxl import quantize_unet
    unet = U.build_unet(device, cfg=cfg)
    unet.load_state_dict(merged)
    ck = OrderedDict(ckpt)
    if rule == "absmax":
        layers = U.quantizable_layers(unet)
        for name in targets:
            w, split = layers[name].weight, split_of(layers[name], name)
            if split:
                ck[name + ".weight_quantizer"] = weight_quantizer_entry(w[:, :split])
                ck[name + ".weight_quantizer_0"] = weight_quantizer_entry(w[:, split:])
            else:
                ck[name + ".weight_quantizer"] = weight_quantizer_entry(w)
    with torch.no_grad():
        y = unet(**inp)[0].clone() if inp is not None else None
        quantize_unet(unet, qcfg, ck, bos=True, bos_dict=precompute_bos(unet, ehs), **flags)
    unet.set_fused(True)
    return unet, y


def first_difference(got, want):
    """The first key (in `want`'s order) at which two state_dicts differ in keys, dtype, shape or raw bytes, with a
    short description; None: they are the same, bit for bit."""
    if list(got) != list(want):
        return f"keys differ: {sorted(set(got) ^ set(want))[:4]}"
    for k, w in want.items():
        g = got[k]
        if g.dtype != w.dtype or g.shape != w.shape:
            return f"{k}: {g.dtype} {tuple(g.shape)} against {w.dtype} {tuple(w.shape)}"
        a, b = (x.detach().cpu().contiguous().numpy().reshape(-1).view(np.uint8) for x in (g, w))
        if not np.array_equal(a, b):
            n = int((a.reshape(-1, g.element_size()) != b.reshape(-1, g.element_size())).any(axis=1).sum())
            return f"{k}: {n} of {g.numel()} elements differ"
    return None


# ---- planting: inputs on which the bank's arithmetic and merge-then-quantize are both exact --------------------------
def free_mask(g, shape, parts=((0, None),), count=3):
    """A boolean mask over the weight's trailing dimensions with `count` columns set in every range of `parts` (ranges of
    the flat (C, R, S) index: the halves of a split shortcut).  Every factor is zero there (`small_factor`), so no dW
    reaches those columns and a row maximum planted there stays the row maximum at any strengths."""
    kf = int(np.prod(shape[1:]))
    mask = np.zeros(kf, bool)
    for a, b in parts:
        b = kf if b is None else b
        mask[a + g.choice(b - a, count, replace=False)] = True
    return torch.from_numpy(mask.reshape(shape[1:]))


def small_factor(g, shape, lim=3, scale=1.0, free=None, nonzero=None):
    """FP16 integers in [-lim, lim] times `scale` (a power of two).  `free` (down factors): zero at those columns, for
    a 4-D [r, C, R, S] or a flat [r, C * R * S] factor alike.  `nonzero` (up factors): that many +-1 per row, the
    rest 0 -- what keeps a Hadamard term small."""
    if nonzero is not None:
        f = np.zeros(shape)
        for row in f:
            row[g.choice(shape[1], nonzero, replace=False)] = g.choice([-1.0, 1.0], nonzero)
    else:
        f = g.integers(-lim, lim + 1, shape).astype(np.float64)
    t = torch.from_numpy(f * scale)
    if free is not None:
        t.reshape(shape[0], -1)[:, free.reshape(-1)] = 0
    h = t.to(torch.float16)
    assert torch.equal(h.double(), t)
    return h


def planted_target(g, shape, bits, free, parts=((0, None),), norm=False, lim=40):
    """The merged weight T in UNITs, float64 in the weight's `shape`.  In every range of `parts` a row's largest
    magnitude is ROW_MAX[bits] * (1 or 2), at a `free` column, so 'absmax' gives delta = 2^j UNIT in FP32 and in the
    checkpoint's FP16 alike; no row is all zero.  Without `norm` the other elements are integers in [-lim, lim]; with
    it a row holds NORM_ROWS[bits] * (1 or 2) with random signs and zeros: its norm is 128 or 256 UNITs."""
    n, kf = shape[0], int(np.prod(shape[1:]))
    T, fm = np.zeros((n, kf)), free.reshape(-1).numpy()
    for a, b in parts:
        b = kf if b is None else b
        cols, fcols = np.arange(a, b), a + np.flatnonzero(fm[a:b])
        for row in range(n):
            big, c = ROW_MAX[bits] * g.choice([1, 2]), g.choice(fcols)
            if norm:
                vals = np.array(NORM_ROWS[bits]) * (big // ROW_MAX[bits])
                others = g.choice(cols[cols != c], len(vals) - 1, replace=False)
                T[row, others] = vals[1:] * g.choice([-1, 1], len(vals) - 1)
            else:
                T[row, a:b] = g.integers(-lim, lim + 1, b - a)
            T[row, c] = big * g.choice([-1, 1])
    assert not norm or len(parts) == 1
    return torch.from_numpy(T.reshape(shape))


def plant_base(T, name, adapters, scales):
    """W = T UNIT - sum_j s_j (alpha_j / r_j) dW_j as FP16 -- exactly, or the planting is refused."""
    w = T * UNIT
    for ad, s in zip(adapters, scales):
        if name in ad:
            dW, unit, _ = term(ad[name], tuple(T.shape))
            w = w - float(s) * unit * dW
    h = w.to(torch.float16)
    assert torch.equal(h.double(), w), f"{name}: the planted base weight is not an FP16 value"
    return h


def magnitude_for(g, T):
    """m = ||row of T UNIT|| * 2^j, j in {-1, 0, 1}, as FP32: g = m / ||row|| is that power of two."""
    norm = (T * T).flatten(1).sum(dim=1).sqrt() * UNIT
    m = norm * torch.from_numpy(2.0 ** g.integers(-1, 2, T.shape[0]))
    assert torch.equal(m.float().double(), m)
    return m.float()


def row_maxima_exact(w, bits, parts=((0, None),)):
    """Is every row maximum of `w` (any float dtype, the weight's own shape), in every range of `parts`, qmax * 2^j?
    Then max / qmax is a power of two: the kernel's FP32 delta and the checkpoint's FP16 delta are the same number."""
    flat = _f64(w).flatten(1).abs()
    for a, b in parts:
        mx = flat[:, a:b].max(dim=1)[0] / QMAX[bits]
        if not (bool((mx > 0).all()) and torch.equal(torch.exp2(torch.log2(mx).round()), mx)):
            return False
    return True


def row_norms_exact(w):
    """Is every row norm of `w` a power of two (its squares sum to a power of 4)?"""
    ss = (_f64(w) ** 2).flatten(1).sum(dim=1)
    e = torch.log2(ss).round()
    return bool((ss > 0).all()) and torch.equal(torch.exp2(e), ss) and bool((e % 2 == 0).all())


# ---- Gaussian inputs: how many integers may differ between the bank and merge-then-quantize --------------------------
def staged_layer(w, name, adapters, scales, cols=(0, None)):
    """The layer dict of tests/lycoris_ref.py for one weight (columns `cols` of its flat (C, R, S) order), laid out from
    the ADAPTERS: linear ranks first, every Hadamard term in a range of its own, each padded to 32.  Only the error
    bound reads this layout; the merged weight itself is cross-checked against merged_f64 by the caller."""
    n, kf = w.shape[0], int(np.prod(w.shape[1:]))
    a, b = cols[0], kf if cols[1] is None else cols[1]
    f16 = lambda x, *s: x.detach().cpu().to(torch.float16).reshape(*s).numpy()      # noqa: E731
    lin, had, m = [], [], None
    for ad, s in zip(adapters, scales):
        if name not in ad:
            continue
        v = ad[name]
        if isinstance(v, dict) and v.get("kind") == "loha":
            r = v["w1_b"].shape[0]
            had.append((r, float(s) * float(v["alpha"]) / r, [f16(v[k], n, r) for k in ("w1_a", "w2_a")],
                        [f16(v[k], r, kf)[:, a:b] for k in ("w1_b", "w2_b")]))
        else:
            A, B, alpha = (v["A"], v["B"], v["alpha"]) if isinstance(v, dict) else v
            lin.append((A.shape[0], float(s) * float(alpha) / A.shape[0], [f16(B, n, A.shape[0])], [f16(A, A.shape[0], kf)[:, a:b]]))
            if isinstance(v, dict) and v.get("magnitude") is not None and float(s) != 0.0:
                m = v["magnitude"].detach().cpu().float().reshape(n).numpy()
    up = lambda r: -(-r // 32) * 32                            # noqa: E731
    r_lin = up(sum(t[0] for t in lin))
    ends = [int(e) for e in r_lin + np.cumsum([up(t[0]) for t in had])]
    rank = max(32, ends[-1] if ends else r_lin)
    B, A, B2, A2 = (np.zeros(s, np.float16) for s in ((n, rank), (rank, b - a)) * 2)
    svec, r0 = np.zeros(rank, np.float32), 0
    for r, s, ups, downs in lin:
        B[:, r0:r0 + r], A[r0:r0 + r], svec[r0:r0 + r] = ups[0], downs[0], s
        r0 += r
    for (r, s, ups, downs), e in zip(had, ends):
        r0 = e - up(r)
        B[:, r0:r0 + r], A[r0:r0 + r], B2[:, r0:r0 + r], A2[r0:r0 + r], svec[r0:r0 + r] = ups[0], downs[0], ups[1], downs[1], s
    W = w.detach().cpu().to(torch.float16).reshape(n, kf)[:, a:b].numpy()
    return dict(W=W, B=B, A=A, B2=B2, A2=A2, svec=svec, r_lin=r_lin, ends=ends, m=m)


def accumulation_bound(w, name, adapters, scales, max_rank, cols=(0, None)):
    """(W' in float64 [N, Kf], the absolute error bound of the kernel's FP32 W') for one weight: (R + 2) 2^-24 (|W| +
    sum |Bs A|) of tests/lora_ref.py for linear terms alone (R = max_rank: the kernel sums every rank of its buffers),
    `tol` of tests/lycoris_ref.py with a Hadamard term or a magnitude."""
    from tests import lora_ref, lycoris_ref
    L = staged_layer(w, name, adapters, scales, cols)
    if not L["ends"] and L["m"] is None:
        wp, mag = lora_ref.merged(L["W"], L["B"], L["A"], L["svec"])
        return wp, (max_rank + 2) * 2.0 ** -24 * mag
    assert cols == (0, None), "a magnitude's row norm spans the whole row"
    r = lycoris_ref.requant(dict(L, mode="f16"), 1.0, 0.0)
    return r["ws"], r["tol"]


def band(w, name, adapters, scales, delta, bits, max_rank, cols=(0, None)):
    """(in_band [N, Kf] bool, W' in float64) for one weight and its logical-order `delta` [N]: the elements whose
    float64 quotient W' / delta lies within tau of a half-integer, where the bank (FP32 accumulators on the FP16 master)
    and merge-then-quantize (W' rounded to FP16) may round to different integers.
    tau = (accumulation_bound + 2^-11 |W'|) / delta."""
    wp, tol = accumulation_bound(w, name, adapters, scales, max_rank, cols)
    d64 = delta.astype(np.float64)[:, None]
    quot = wp * (np.float32(1) / delta).astype(np.float64)[:, None] if bits == 8 else wp / d64
    tau = (tol + 2.0 ** -11 * np.abs(wp)) / d64
    return np.abs(quot - np.floor(quot) - 0.5) <= tau, wp


# ---- the cases of tests/test_lora_oracle_gpu.py, made on the CPU so that the host tests can check their conditions ----
def _parts(split):
    return ((0, split), (split, None)) if split else ((0, None),)


def exact_case(form, shapes, bits, splits, stacked, seed=0):
    """Planted adapters for `shapes` ({module name: weight shape}; bits: the quantizers' widths, 16 for an FP16 layer;
    splits: {name: split}; `stacked`: the layer that also takes a second Hadamard term and a linear tuple under
    'loha').  Returns dict(adapters, scales, scales2, base={"<name>.weight": the planted FP16 base weight}, T).
    alpha / r: 2 / 4, 3 / 6 (linear), 2.5 / 5, 3 / 6 (Hadamard).  `scales2`: what set_scales() is given afterwards."""
    g = np.random.default_rng(seed)
    names = list(shapes)
    free = {n: free_mask(g, shapes[n], _parts(splits.get(n, 0))) for n in names}
    rest = {n: tuple(shapes[n][1:]) for n in names}

    def lin(n, r, alpha, as_dict):
        A = small_factor(g, (r,) + rest[n], scale=UNIT, free=free[n])
        B = small_factor(g, (shapes[n][0], r))
        return dict(kind="lora", A=A, B=B, alpha=alpha) if as_dict else (A, B, alpha)

    def had(n, r, alpha):
        flat = (r, int(np.prod(rest[n])))
        return dict(kind="loha", alpha=alpha, w1_a=small_factor(g, (shapes[n][0], r), nonzero=2),
                    w1_b=small_factor(g, flat, lim=2, scale=UNIT, free=free[n]),          # flat, (C, R, S) order
                    w2_a=small_factor(g, (shapes[n][0], r), nonzero=2),
                    w2_b=small_factor(g, (r,) + rest[n], lim=2, free=free[n]))            # 4-D
    if form == "lora":
        adapters = [{n: lin(n, 4, 2.0, False) for n in names}, {n: lin(n, 6, 3.0, False) for n in names}]
        scales, scales2 = [1.0, 0.5], [0.5, 2.0]
    elif form == "loha":
        adapters = [{n: had(n, 5, 2.5) for n in names}, {stacked: had(stacked, 6, 3.0)}, {stacked: lin(stacked, 4, 2.0, False)}]
        scales, scales2 = [1.0, 0.5, 1.0], [2.0, 1.0, 0.5]
    else:
        assert form == "dora", form
        adapters = [{n: lin(n, 6, 3.0, True) for n in names}, {n: lin(n, 4, 2.0, True) for n in names}]
        scales, scales2 = [1.0, 0.5], [0.0, 2.0]
    T = {n: planted_target(g, shapes[n], min(bits[n], 8), free[n], _parts(splits.get(n, 0)), norm=form == "dora")
         for n in names}
    if form == "dora":
        for n in names:
            adapters[0][n]["magnitude"] = magnitude_for(g, T[n])
    base = {n + ".weight": plant_base(T[n], n, adapters, scales) for n in names}
    return dict(adapters=adapters, scales=scales, scales2=scales2, base=base, T=T)


def random_case(form, shapes, state, seed=3):
    """Gaussian adapters, as the bank tests of tests/test_lora_gpu.py and tests/test_lycoris_gpu.py draw them.  Strengths and
    alpha / r are powers of two: the kernel's Bs = f16(s * alpha / r * B) is then B scaled, not rounded a second time --
    a rounding merge-then-quantize does not have and tau does not cover."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    rnd = lambda std, *s: (torch.randn(s, generator=g) * std).half()      # noqa: E731
    if form == "lora":
        return [{n: (rnd(0.05, 8, *s[1:]), rnd(0.05, s[0], 8), 16.0) for n, s in shapes.items()}], [1.0]
    loha, dora = {}, {}
    for n, s in shapes.items():
        kf = int(np.prod(s[1:]))
        loha[n] = dict(kind="loha", w1_a=rnd(0.2, s[0], 4), w1_b=rnd(0.2, 4, kf), w2_a=rnd(0.2, s[0], 4), w2_b=rnd(0.2, 4, *s[1:]),
                       alpha=4.0)
        dora[n] = dict(kind="lora", A=rnd(0.2, 8, *s[1:]), B=rnd(0.2, s[0], 8), alpha=8.0)
        if form == "dora":
            dora[n]["magnitude"] = state[n + ".weight"].detach().cpu().float().flatten(1).norm(dim=1) * 1.1
    return ([loha], [1.0]) if form == "loha" else ([dora, loha], [0.5, 1.0])


def to_device(adapters, dev):
    mv = lambda v: v.to(dev) if torch.is_tensor(v) else v      # noqa: E731
    return [{n: ({k: mv(x) for k, x in v.items()} if isinstance(v, dict) else tuple(mv(x) for x in v))
             for n, v in ad.items()} for ad in adapters]


def tiny_cfg():
    """The tiny UNet of the bank tests (tests/test_lora_gpu.py, tests/test_lycoris_gpu.py)."""
    import bench
    return dict(bench.TINY_CFG, block_out_channels=(64, 128, 256), head_dim=64)


def form_targets(form):
    from tests.test_lora_gpu import BLK, TARGETS
    from tests.test_lycoris_gpu import TARGETS as LYCO
    dora = (BLK + "attn1.to_q", BLK + "attn1.to_out.0", "down_blocks.0.resnets.0.conv1", BLK + "attn2.to_k", "conv_in")
    return {"lora": TARGETS, "loha": LYCO, "dora": dora}[form]      # dora: a Linear, packed W4, a conv, BOS, FP16


def target_info(unet, form):
    """(shapes, bits, splits) of the form's targets, from the FLOAT UNet and the config of the bank tests."""
    from mixdq_amd.unet import quantizable_layers
    from tests.test_control_gpu import FP16_LAYERS
    from tests.test_lora_gpu import NARROW
    layers = quantizable_layers(unet)
    names = form_targets(form)
    return ({n: tuple(layers[n].weight.shape) for n in names},
            {n: 16 if n.split(".")[0] in FP16_LAYERS else NARROW.get(n, 8) for n in names},
            {n: split_of(layers[n], n) for n in names})


def layer_parts(name, shape, split):
    """[(buffer suffix, columns of the flat (C, R, S) order)]: a split conv_shortcut has two quantizers."""
    return [("", (0, split)), ("_0", (split, None))] if split else [("", (0, None))]


def random_bands(form, state, info, deltas, max_rank, seed=3):
    """{(name, suffix): (in-band mask, W' float64, delta)} of random_case() for every quantized target; `deltas`:
    {checkpoint key: entry} -- the ORIGINAL checkpoint's weight quantizers (KEEP keeps them)."""
    from mixdq_amd.nn.utils import bit_index
    shapes, bits, splits = info
    adapters, scales = random_case(form, shapes, state, seed)
    out = {}
    for n in shapes:
        if bits[n] == 16:
            continue
        for sfx, cols in layer_parts(n, shapes[n], splits[n]):
            delta = deltas[n + ".weight_quantizer" + sfx]["delta_list"][bit_index(bits[n])].detach().cpu().float().numpy()
            out[n, sfx] = band(state[n + ".weight"], n, adapters, scales, delta, bits[n], max_rank, cols) + (delta,)
    return out
