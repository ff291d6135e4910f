"""GPU tests of the Resampler's two launches (csrc/resampler.hip) against float64 references, and of the whole Resampler
against the same network from stock torch functions (tests/resampler_ref.py)."""
import math

import numpy as np
import pytest
import torch

from mixdq_amd.ip_adapter import Resampler
from tests import resampler_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24                                # unit roundoff of FP32


def rnd(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).half()


def same(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


# ---------------------------------------------------------------------------------------------- attention_perceiver

def packed(qkv, img, tq, t2, C):
    """q, k2, v2: column slices of one [B, max(tq, t2), 3 C] buffer; k1, v1: slices of a [B, t1, 4 C] buffer at column 2 C."""
    k2, v2 = (qkv[:, :t2, C:2 * C], qkv[:, :t2, 2 * C:]) if t2 else (None, None)
    return qkv[:, :tq, :C], img[..., 2 * C:3 * C], img[..., 3 * C:], k2, v2


def attention64(q, k1, v1, k2, v2, heads):
    k, v = (torch.cat([a, b], dim=1) if b is not None else a for a, b in ((k1, k2), (v1, v2)))
    q, k, v = (t.double().cpu().reshape(t.shape[0], t.shape[1], heads, 64).transpose(1, 2) for t in (q, k, v))
    o = torch.softmax(q @ k.transpose(-1, -2) * 0.125, dim=-1) @ v
    return o.transpose(1, 2).reshape(q.shape[0], q.shape[2], heads * 64)


@pytest.mark.parametrize("B,H", [(1, 1), (2, 3)])
@pytest.mark.parametrize("tq", (1, 5, 16))
@pytest.mark.parametrize("t1,t2", [(1, 0), (3, 5), (31, 1), (33, 16), (64, 16), (257, 16)])
def test_perceiver_against_float64_over_the_concatenation(C, t1, t2, tq, B, H):
    """One to three empty waves, a block that straddles the seam, a ragged last block, partial query rows, strided
    operands.  Tolerance: tests/test_attention_gpu.py's."""
    Cw = H * 64
    qkv, img = rnd((B, max(tq, t2), 3 * Cw), 7 * t1 + tq).to(DEV), rnd((B, t1, 4 * Cw), 11 * t1 + t2).to(DEV)
    ops = packed(qkv, img, tq, t2, Cw)
    got = C.attention_perceiver(*ops, H).double().cpu()
    ref = attention64(*ops, H)
    err = (got - ref).abs()
    print(f"max |got - ref| = {err.max().item():.3e}")
    assert bool((err <= 2e-3 + 4e-3 * ref.abs()).all())


@pytest.mark.parametrize("t1,t2", [(48, 16), (64, 0), (7, 57)])
def test_perceiver_zero_keys_give_the_exact_mean(C, t1, t2):
    """64 zero keys: every P is 1, the sums of small integers are exact, and each column sum is a multiple of 64."""
    B, H, tq = 2, 2, 16
    g = torch.Generator().manual_seed(t1)
    v = torch.randint(-8, 9, (B, 64, H * 64), generator=g).double()
    v[:, 63] -= v.sum(dim=1) - 64 * torch.round(v[:, :63].sum(dim=1) / 64)
    q, zk = rnd((B, tq, H * 64), 5).to(DEV), torch.zeros((B, 64, H * 64), dtype=torch.float16, device=DEV)
    vh = v.half().to(DEV)
    got = C.attention_perceiver(q, zk[:, :t1], vh[:, :t1], zk[:, t1:] if t2 else None, vh[:, t1:] if t2 else None, H)
    want = (v.sum(dim=1, keepdim=True) / 64).expand(B, tq, H * 64).half()
    assert same(got.cpu(), want.contiguous())


@pytest.mark.parametrize("last_of", (1, 2))
def test_perceiver_one_dominating_key_gives_its_value_row(C, last_of):
    """q = 1, one key = 32 (score 256 after scaling; exp(-256) is 0 in FP32), the rest 0: the output is that V row."""
    B, H, tq, t1, t2 = 1, 2, 16, 33, 16
    q = torch.ones((B, tq, H * 64), dtype=torch.float16, device=DEV)
    k1, k2 = (torch.zeros((B, t, H * 64), dtype=torch.float16, device=DEV) for t in (t1, t2))
    v1, v2 = rnd((B, t1, H * 64), 1).to(DEV), rnd((B, t2, H * 64), 2).to(DEV)
    (k1 if last_of == 1 else k2)[:, -1] = 32.0
    got = C.attention_perceiver(q, k1, v1, k2, v2, H)
    assert same(got, (v1 if last_of == 1 else v2)[:, -1:].expand(B, tq, H * 64).contiguous())


@pytest.mark.parametrize("what", ("tq17", "head80", "t1_0", "stride"))
def test_perceiver_refusals_leave_out_untouched(C, what):
    H, hd = 2, 80 if what == "head80" else 64
    tq, t1, w = 17 if what == "tq17" else 8, 0 if what == "t1_0" else 8, H * hd + (4 if what == "stride" else 0)
    q, k1, v1 = (torch.zeros((1, t, w), dtype=torch.float16, device=DEV)[..., :H * hd] for t in (tq, t1, t1))
    out = torch.full((1, tq, H * hd), 3.0, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match="attention_perceiver"):
        C.attention_perceiver(q, k1, v1, None, None, H, out=out)
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())


# ------------------------------------------------------------------------------------------------ linear_f16_skinny

def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def f16(x):
    return x.half().double()


def midpoint_gap(x):
    """|x - the FP16 rounding boundary next to it| for a float64 tensor."""
    x = x.numpy()
    near = x.astype(np.float16)
    other = np.nextafter(near, np.where(x > near.astype(np.float64), np.float16(np.inf), np.float16(-np.inf)))
    return torch.from_numpy(np.abs(x - (near.astype(np.float64) + other.astype(np.float64)) / 2))


def skinny_case(C, M, N, K, opts, seed):
    """Runs the launch and checks it against float64 of the specified arithmetic.
    Band of the first rounding: wave w adds its K / 4 products in an order that is the hardware's inside an instruction,
    so at most K / 4 + 3 roundings lie on the path of any product (+ 1 for the bias): |s32 - s64| <= (K / 4 + 4) U mag,
    mag = sum |a w| + |bias|.  With the LayerNorm prologue an element of LN(A) whose float64 value lies within the FP32
    LayerNorm's error e_y of an FP16 boundary may round to the other neighbour, which moves s by |w| ulp(a):
    e_y = (K / 16 + 16) U (|gamma| rstd mean|x| + |y| + |beta|) (K / 16 + 4 additions per statistic, the rest for the
    divisions, the root and the affine).  An element farther than the band from its boundary is decided and must EQUAL
    float64's chain (with GELU: unless gelu64 lies within mixdq_geluf's 1e-7 |x| + 4 U |gelu| of a boundary); the others
    must lie within the band, carried through GELU's slope (<= 1.13), plus one ulp per rounding."""
    a = rnd((M, K), seed)
    w = rnd((N, K), seed + 1, K ** -0.5)
    bias = rnd((N,), seed + 2) if "bias" in opts else None
    res = rnd((M, N), seed + 3) if "res" in opts else None
    ln = None
    a64, extra = a.double(), torch.zeros((M, N), dtype=torch.float64)
    if "ln" in opts:
        a[0] += 1000.0                                           # a row with a large common offset ...
        a[M - 1] = 0.25                                          # ... and one without variance
        ln = (1 + 0.2 * rnd((K,), seed + 4), 0.2 * rnd((K,), seed + 5), 1e-5)
        x, gm, bt = a.double(), ln[0].double(), ln[1].double()
        rstd = 1.0 / torch.sqrt(x.var(dim=1, unbiased=False, keepdim=True) + 1e-5)
        y = (x - x.mean(dim=1, keepdim=True)) * rstd * gm + bt
        e_y = (K / 16 + 16) * U * (gm.abs() * rstd * x.abs().mean(dim=1, keepdim=True) + y.abs() + bt.abs())
        a64 = f16(y)
        ulp_a = torch.from_numpy(np.spacing(np.abs(a64.numpy()).astype(np.float16)).astype(np.float64))
        extra = ((midpoint_gap(y) <= e_y) * ulp_a) @ w.double().abs().T
    s = a64 @ w.double().T + (bias.double() if bias is not None else 0.0)
    mag = a64.abs() @ w.double().abs().T + (bias.double().abs() if bias is not None else 0.0)
    band = (K / 4 + 4) * U * mag + extra
    loose = midpoint_gap(s) <= band
    y0 = f16(s)
    tol = band + torch.from_numpy(np.spacing(np.abs(y0.numpy()).astype(np.float16)).astype(np.float64))
    ref = y0
    if "gelu" in opts:
        gl = gelu64(y0)
        loose |= midpoint_gap(gl) <= 1e-7 * y0.abs() + 4 * U * gl.abs()
        ref = f16(gl)
        tol = 1.13 * tol + torch.from_numpy(np.spacing(np.abs(ref.numpy()).astype(np.float16)).astype(np.float64))
    if res is not None:
        ref = f16(ref + res.double())
        tol = tol + torch.from_numpy(np.spacing(np.abs(ref.numpy()).astype(np.float16)).astype(np.float64))
    dev = [None if t is None else t.to(DEV) for t in (a, w, bias, res)]
    got = C.linear_f16_skinny(dev[0], dev[1], dev[2], residual=dev[3], ln=None if ln is None else tuple(
        t.to(DEV) if torch.is_tensor(t) else t for t in ln), act="gelu" if "gelu" in opts else None).double().cpu()
    print(f"M {M} N {N} K {K} {opts}: {loose.double().mean().item():.2%} inside the band, "
          f"{(got != ref).double().mean().item():.2%} differ from float64's chain")
    assert torch.equal(got[~loose], ref[~loose])
    assert bool(((got - ref).abs() <= tol)[loose].all())


OPTS = [(), ("bias",), ("bias", "res"), ("gelu",), ("ln",), ("ln", "gelu", "bias")]


@pytest.mark.parametrize("opts", OPTS, ids=lambda o: "+".join(o) or "none")
@pytest.mark.parametrize("K", (32, 160, 2048))
@pytest.mark.parametrize("N", (16, 80))
@pytest.mark.parametrize("M", (1, 16, 17, 48))
def test_skinny_against_float64(C, M, N, K, opts):
    skinny_case(C, M, N, K, opts, 1000 * M + 10 * N + K)


@pytest.mark.parametrize("opts", [o for o in OPTS if "ln" not in o], ids=lambda o: "+".join(o) or "none")
def test_skinny_against_float64_at_the_longest_row(C, opts):
    skinny_case(C, 16, 16, 8192, opts, 8192)


@pytest.mark.parametrize("M,N,K", [(1, 16, 32), (17, 80, 160), (48, 80, 2048), (16, 16, 8192)])
def test_skinny_exact_integers_match_linear_f16(C, M, N, K):
    """Inputs in {-2 .. 2} x {-1, 0, 1}: every partial sum is an integer below 2^24, so any order gives the same bits."""
    g = torch.Generator().manual_seed(K)
    a = torch.randint(-2, 3, (M, K), generator=g).half().to(DEV)
    w = torch.randint(-1, 2, (N, K), generator=g).half().to(DEV)
    bias = torch.randint(-4, 5, (N,), generator=g).half().to(DEV)
    res = torch.randint(-4, 5, (M, N), generator=g).half().to(DEV)
    assert same(C.linear_f16_skinny(a, w, bias, residual=res), C.linear_f16(a, w, bias, _residual=res))
    assert same(C.linear_f16_skinny(a, w, bias, act="gelu"), C.linear_f16(a, w, bias, _act="gelu"))
    wide = torch.zeros((M, K + 8), dtype=torch.float16, device=DEV)           # a column slice as A, D on the residual
    wide[:, 8:] = a
    out = res.clone()
    assert C.linear_f16_skinny(wide[:, 8:], w, residual=out, out=out) is out
    assert same(out, C.linear_f16(a, w, None, _residual=res))


@pytest.mark.parametrize("what", ("N24", "K48", "M257", "lnK4096", "one_ln_vector"))
def test_skinny_refusals(C, what):
    M, N, K = 257 if what == "M257" else 4, 24 if what == "N24" else 32, {"K48": 48, "lnK4096": 4096}.get(what, 64)
    a, w = (torch.zeros(s, dtype=torch.float16, device=DEV) for s in ((M, K), (N, K)))
    v = torch.ones(K, dtype=torch.float16, device=DEV)
    ln = (v, v, 1e-5) if what == "lnK4096" else (v, None, 1e-5) if what == "one_ln_vector" else None
    out = torch.full((M, N), 3.0, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match="linear_f16_skinny"):
        C.linear_f16_skinny(a, w, ln=ln, out=out)
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())


# ---------------------------------------------------------------------------------------------------- the Resampler

SMALL = dict(dim=128, depth=2, dim_head=64, heads=2, embedding_dim=96, ff_mult=2)


def small_resampler(T, seed=5):
    torch.manual_seed(seed)
    rs = Resampler(num_queries=T, output_dim=64, **SMALL)
    with torch.no_grad():
        for name, p in rs.named_parameters():                    # LayerNorms that do something
            if p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape))
    return rs.eval()


@pytest.mark.parametrize("B", (1, 2))
@pytest.mark.parametrize("n1", (10, 50))
@pytest.mark.parametrize("T", (5, 16))
def test_resampler_against_the_stock_network(T, n1, B):
    """tests/test_text_gpu.py's rule: max |ours - fp32| <= max(1.5 x max |stock FP16 on the GPU - fp32|, one FP16 ulp at
    the top of the output range); then a captured graph replayed three times equals the eager result bit for bit."""
    rs = small_resampler(T)
    hidden = torch.randn(B, n1, 96, generator=torch.Generator().manual_seed(n1))
    truth = resampler_ref.forward(rs.state_dict(), hidden, heads=2, depth=2)
    rs = rs.half().to(DEV)
    hd = hidden.half().to(DEV)
    stock = resampler_ref.forward(rs.state_dict(), hd, heads=2, depth=2)
    assert rs._fast(hd)
    ours = rs(hd)
    err_ours, err_stock = ((t.float().cpu() - truth).abs().max().item() for t in (ours, stock))
    ulp = 2.0 ** (math.floor(math.log2(truth.abs().max().item())) - 10)
    print(f"T {T} n1 {n1} B {B}: ours {err_ours:.3e}, stock fp16 {err_stock:.3e}, ulp floor {ulp:.3e}")
    assert err_ours <= max(1.5 * err_stock, ulp)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            captured = rs(hd)
    for _ in range(3):
        captured.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert same(captured, ours)


def test_resampler_follows_an_in_place_write_to_norm1():
    rs = small_resampler(16).half().to(DEV)
    hd = torch.randn(1, 10, 96, generator=torch.Generator().manual_seed(1)).half().to(DEV)
    before, (w_before, _) = rs(hd).clone(), rs.folded_kv()
    with torch.no_grad():
        rs.layers[1][0].norm1.weight.mul_(1.5)                   # in place: the version counter moves
    after = rs(hd)
    assert rs.folded_kv()[0] is w_before and not same(after, before)     # rebuilt in place, and read
    truth = resampler_ref.forward({k: v.float().cpu() for k, v in rs.state_dict().items()}, hd.float().cpu(), heads=2, depth=2)
    stock = resampler_ref.forward(rs.state_dict(), hd, heads=2, depth=2)
    err_ours, err_stock = ((t.float().cpu() - truth).abs().max().item() for t in (after, stock))
    ulp = 2.0 ** (math.floor(math.log2(truth.abs().max().item())) - 10)
    assert err_ours <= max(1.5 * err_stock, ulp)
