"""GPU tests of the FP16 attention core on exact-result inputs (tests/exact_inputs.py): every form of every head
width -- attn_fwd_kernel (128- and 64-query workgroups), attn_short_kernel, attn_hd_kernel at 40 / 80 / 160 in both
forms, attn_hd_short_kernel -- on the separate and the fused q|k|v / k|v layouts, at key counts 1 .. 4097.

  a. selection      one-hot softmax: out[i] == v[j(i)] BIT FOR BIT, the INT8 / A4 outputs == quantize(v[j(i)]).  A
                    dropped or permuted key, a wrong ds_read_b64_tr_b16 slot, a stale ring stage give another row.
  b. counted once   q = 0, one probe key per channel: out == 2048 / tkv within one FP16 ulp (bit-exact where tkv is a
                    power of two): a dropped key gives 0, a key counted twice or an admitted masked copy of the last
                    key twice the value or 2048 / (tkv + 1).  Small-integer values at power-of-two key counts:
                    out == fp16(sum / tkv) bit for bit.
  c. rescale        score staircases of 4 and 40 log2 units per key tile (rising: alpha = 2^-4 / 2^-40 at every tile;
                    falling: P down to FP16 subnormals and zero), a dominant key in the last tile after a large
                    maximum in the first, equal scores of +-60, |v| up to 6e4.  Held to the float64 oracle at the
                    tolerance of tests/test_attention_gpu.py (imported, not restated) and to PyTorch's FP16 SDPA;
                    finite; every channel within [min_j v, max_j v] of its head up to one ulp; every form and layout
                    the same bits; a batch row equal to its single run.

Magnitudes of (c), as built (tests/exact_inputs.py rescale(); none had to be shrunk): |scaled score| up to ~170 log2
units (rise40 / fall40 at 640 keys: ~360), values N(0, 1.2^2), `huge_values` |v| in [3e4, 6e4] with one sign per
channel.  Measured on an MI355X, the largest figure of each kind over widths and key counts (each case prints its
own, `-s`), as error / (2e-3 + 4e-3 |ref|), this kernel | PyTorch's FP16 SDPA, and the largest absolute error:
    rise4 0.108 | 0.106 (5.6e-4 | 6.0e-4)      rise40 0.151 | 0.151 (6.7e-4 | 6.8e-4)
    fall4 0.086 | 0.086 (3.4e-4 | 3.4e-4)      fall40 0.085 | 0.083 (3.2e-4 | 3.2e-4)
    late_dominant 0.000 | 0.000 (1.9e-13: the FP16 output is the dominant key's value row)
    equal_large 0.039 | 0.039, equal_large_negative 0.040 | 0.040 (1.2e-4 | 1.2e-4)
    huge_values 0.117 | 0.125 (17.3 | 21.4 on results of 3e4 .. 6e4)
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import exact_inputs as ei
from tests.test_attention_gpu import ATOL, RTOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S_INV, ZP = float(np.float32(1) / np.float32(0.0173)), 7.0
LAYOUTS = ("separate", "fused")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def scal(v):
    return torch.tensor(float(v), dtype=torch.float32, device=DEV)


def forms(tkv):
    """Every form that accepts the shape: the library's choice, 64- and 128-query workgroups, the short-key kernel."""
    return (0, 2, 4, 1) if tkv <= 128 else (0, 2, 4)


def views(c, layout):
    """Device q / k / v: contiguous tensors, or column slices of one [B, T, 3C] q|k|v buffer (tq == tkv) / of a
    [B, Tkv, 2C] k|v buffer: row strides of 3C and 2C, as the UNet's fused projections leave them."""
    q, k, v = c["q"], c["k"], c["v"]
    Cc = q.shape[-1]
    if layout == "separate":
        return t(q), t(k), t(v)
    if q.shape[1] == k.shape[1]:
        d = t(np.concatenate([q, k, v], axis=-1))
        return d[..., :Cc], d[..., Cc:2 * Cc], d[..., 2 * Cc:]
    kv = t(np.concatenate([k, v], axis=-1))
    return t(q), kv[..., :Cc], kv[..., Cc:]


def bits(x):
    return x.cpu().numpy().view(np.uint16)


def assert_bits(got, want, what, c=None):
    g, w = bits(got), np.ascontiguousarray(want).view(np.uint16)
    if np.array_equal(g, w):
        return
    bad = np.argwhere(g != w)
    b, i, ch = (int(x) for x in bad[0])
    msg = f"{what}: {len(bad)} of {g.size} elements differ; first at batch {b} query {i} channel {ch}: " \
          f"got {got[b, i, ch].item()!r} want {np.asarray(want)[b, i, ch]!r}"
    if c is not None and "hot" in c:
        D = g.shape[-1] // c["heads"]
        msg += f" (hot key {int(c['hot'][b, ch // D, i])}; queries hit: {sorted(set(int(x) for x in bad[:, 1]))[:12]})"
    raise AssertionError(msg)


CASES = [(D, tkv) for D in ei.WIDTHS for tkv in ei.KEY_COUNTS]
IDS = [f"d{D}_k{tkv}" for D, tkv in CASES]


@pytest.mark.parametrize("D,tkv", CASES, ids=IDS)
def test_selection_returns_the_hot_value_row_bit_for_bit(C, oracle, D, tkv):
    c = ei.selection(D, tkv)
    heads, want = c["heads"], c["expected"]
    want8 = oracle.quantize(want, S_INV, ZP, C.FLAGS & 1)
    assert (want8 != want8.flat[0]).any()
    s, z = scal(S_INV), scal(ZP)
    for layout in LAYOUTS:
        qd, kd, vd = views(c, layout)
        for cfg in forms(tkv):
            what = f"selection d{D} k{tkv} q{want.shape[1]} {layout} form {cfg}"
            got = C.attention_f16(qd, kd, vd, heads, _cfg=cfg)
            assert got.shape == want.shape and got.dtype == torch.float16
            assert_bits(got, want, what, c)
            o8 = C.attention_f16(qd, kd, vd, heads, s, z, _cfg=cfg)
            assert np.array_equal(o8.cpu().numpy(), want8), what + " INT8"
            o4 = C.attention_f16(qd, kd, vd, heads, s, z, _cfg=cfg, _abits=4)
            assert np.array_equal(o4.cpu().numpy(), np.minimum(want8, -113)), what + " A4"


@pytest.mark.parametrize("D,tkv", CASES, ids=IDS)
def test_every_key_is_counted_exactly_once(C, D, tkv):
    c = ei.every_key_once(D, tkv)
    heads = c["heads"]
    for layout in LAYOUTS:
        qd, kd, vd = views(c, layout)
        for cfg in forms(tkv):
            what = f"probes d{D} k{tkv} {layout} form {cfg}"
            got = C.attention_f16(qd, kd, vd, heads, _cfg=cfg)
            g = got.cpu().numpy().astype(np.float64)
            err = np.abs(g - c["expected"])
            bad = np.argwhere(err > c["ulp"])
            if len(bad):
                b, i, ch = (int(x) for x in bad[0])
                keys = sorted({int(c["probes"][int(bb), int(cc)]) for bb, _, cc in bad})
                raise AssertionError(f"{what}: {len(bad)} outputs off; first batch {b} query {i} channel {ch}: got "
                                     f"{g[b, i, ch]!r} want {c['expected'][b, i, ch]!r}; probe keys involved {keys[:16]}")
            if c["exact"]:
                assert_bits(got, c["expected16"], what)
    if c["exact"]:
        s = ei.small_integers(D, tkv)
        for layout in LAYOUTS:
            qd, kd, vd = views(s, layout)
            for cfg in forms(tkv):
                assert_bits(C.attention_f16(qd, kd, vd, heads, _cfg=cfg), s["expected"],
                            f"integer mean d{D} k{tkv} {layout} form {cfg}")


def sdpa(q, k, v, heads):
    B, tq, Cc = q.shape
    D = Cc // heads
    return F.scaled_dot_product_attention(*(x.unflatten(-1, (heads, D)).transpose(1, 2) for x in (q, k, v))
                                          ).transpose(1, 2).reshape(B, tq, Cc)


RESCALE = [(kind, D, tkv) for kind in ei.RESCALE_KINDS for D in ei.WIDTHS for tkv in ei.RESCALE_KEY_COUNTS]


@pytest.mark.parametrize("kind,D,tkv", RESCALE, ids=[f"{k}_d{D}_k{n}" for k, D, n in RESCALE])
def test_rescale_path_and_extremes(C, oracle, kind, D, tkv):
    c = ei.rescale(kind, D, tkv)
    heads, (B, tq, Cc) = c["heads"], c["q"].shape
    _, ref64 = oracle.attention_f16(c["q"], c["k"], c["v"], heads)
    qd, kd, vd = views(c, "separate")
    got = C.attention_f16(qd, kd, vd, heads)
    g = got.cpu().numpy().astype(np.float64)
    err = np.abs(g - ref64)
    tol = ATOL + RTOL * np.abs(ref64)
    sd = sdpa(qd, kd, vd, heads).cpu().numpy().astype(np.float64)
    err_sd = np.abs(sd - ref64)
    rms, rms_sd = np.sqrt((err ** 2).mean()), np.sqrt((err_sd ** 2).mean())
    with np.errstate(invalid="ignore"):
        print(f"{kind} d{D} k{tkv}: max err {err.max():.3e} (worst err / tol {np.nanmax(err / tol):.3f}) rms {rms:.3e}; "
              f"SDPA max err {np.nanmax(err_sd):.3e} (worst err / tol {np.nanmax(err_sd / tol):.3f}) rms {rms_sd:.3e}; "
              f"max |ref| {np.abs(ref64).max():.4g}")
    assert np.isfinite(g).all()
    assert (err <= tol).all(), f"max err {err.max():.3e}, worst err / tol {(err / tol).max():.3f}"
    assert err.max() <= 1.5 * err_sd.max() + 1e-3
    assert rms <= 1.5 * rms_sd + 1e-5
    # a convex combination: every channel within the range of its head's values, up to one ulp of the bound
    v64 = c["v"].astype(np.float64)
    lo, hi = v64.min(axis=1, keepdims=True), v64.max(axis=1, keepdims=True)
    assert (g >= lo - ei.ulp16(lo)).all() and (g <= hi + ei.ulp16(hi)).all()
    # every form, both layouts: the same bits; a batch row: the bits of its single run
    for layout in LAYOUTS:
        ql, kl, vl = views(c, layout)
        for cfg in forms(tkv):
            assert torch.equal(C.attention_f16(ql, kl, vl, heads, _cfg=cfg).view(torch.int16), got.view(torch.int16)), \
                f"{layout} form {cfg}"
    for b in range(B):
        one = C.attention_f16(qd[b:b + 1], kd[b:b + 1], vd[b:b + 1], heads)
        assert torch.equal(one[0].view(torch.int16), got[b].view(torch.int16)), f"batch row {b}"
