"""Every GEMM tile configuration at its tile-grid and pipeline edges (cases: tests/tile_edges.py, derived from
each configuration's own BM, BN, BK and STAGES): one and two K-tiles, STAGES - 1 .. STAGES + 1 of them, ragged
K; M and N one short of, at and one past a tile; packed W4 / W2 weights, the residual epilogue and the BOS row
map; convs whose K-tiles straddle filter taps; GEMM + GEGLU; the persistent 256x256 kernel; the quantizing
(f16in) family, the FP16 layers and the grouped launch.

Each INT8 result is checked two ways: bit for bit against the oracle (the contract), and against a plain
float64 evaluation that shares no code with it -- the accumulator an exact float64 product of the int8 values
(|acc| < 2^53), the epilogue (acc - bias0) * scale + bias in float64 -- within

    |out - ref| <= ulp16(ref) + 2^-22 * (|acc - bias0| * scale + |bias|)

i.e. one fp16 ulp of the reference (the output rounding) plus the FP32 roundings of the epilogue's subtraction
and multiply-add (2^-24 each, with margin), ulp16(x) = 2^(max(floor(log2 |x|), -14) - 10).  The FP16 layers
are held to test_f16_gpu.py's bound against float64 F.linear."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import detdata as dd
from tests import tile_edges as te

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def scal(v):
    return torch.tensor(float(v), dtype=torch.float32, device=DEV)


def seed_of(*vals):
    s = 17
    for v in vals:
        s = (s * 1000003 + int(v)) % (1 << 31)
    return s


def bits_equal(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    g = got.view(np.uint16) if got.dtype == np.float16 else got
    w = want.view(np.uint16) if want.dtype == np.float16 else want
    assert g.shape == w.shape, f"{what}: shape {g.shape} vs {w.shape}"
    bad = np.nonzero(g.reshape(-1) != w.reshape(-1))[0]
    assert bad.size == 0, (f"{what}: {bad.size}/{g.size} elements differ; first at flat index {bad[0]}: "
                           f"got {got.reshape(-1)[bad[0]]!r} want {want.reshape(-1)[bad[0]]!r}")


def ulp16(x):
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -24)))
    return 2.0 ** (np.maximum(e, -14) - 10)


def close_f64(got, acc, bias0, scale, bias, what):
    """The module docstring's bound: float64 epilogue on the exact accumulator."""
    got = (got.cpu().numpy() if isinstance(got, torch.Tensor) else got).astype(np.float64)
    d = acc - bias0.astype(np.float64)
    b = 0.0 if bias is None else bias.astype(np.float64)
    ref = d * scale.astype(np.float64) + b
    tol = ulp16(ref) + 2.0 ** -22 * (np.abs(d) * scale.astype(np.float64) + np.abs(b))
    err = np.abs(got - ref)
    bad = ~(err <= tol)
    assert not bad.any(), (f"{what}: {int(bad.sum())}/{bad.size} outside the float64 bound; worst err "
                           f"{err.max():.4g} (tol there {tol.reshape(-1)[err.argmax()]:.4g})")


def acc64(a, w):
    return a.reshape(-1, a.shape[-1]).astype(np.float64) @ w.astype(np.float64).T


def gemm(C, a, w, sc, b0, bias, **kw):
    return C.qlinear_w8_a8_ohalf(a, w, sc, scal(1), scal(0), b0, sc, b0, bias, **kw)


# ------------------------------------------------------------------------------ INT8 Linear, every id
LINEAR = te.all_linear()


@pytest.mark.parametrize("case", LINEAR, ids=[te.linear_id(c) for c in LINEAR])
def test_linear_tile_edges(C, oracle, case):
    from mixdq_amd.nn.utils import pack_w2, pack_w4, unpack_w2
    cfg, M, N, K = case["cfg"], case["M"], case["N"], case["K"]
    s = seed_of(cfg, M, N, K)
    variant = C.FLAGS & 1
    a = dd.int8(s, (M, K))
    b0, sc = dd.f32(s + 2, (N,), -500, 500), dd.f32(s + 3, (N,), 1e-4, 1e-3)
    bias = dd.f16(s + 4, (N,), -1, 1) if case["bias"] else None
    bd = None if bias is None else t(bias)
    ad, b0d, scd = t(a), t(b0), t(sc)

    w = dd.int8(s + 1, (N, K))
    out = gemm(C, ad, t(w), scd, b0d, bd, _cfg=cfg)
    bits_equal(out, oracle.qlinear(a, w, b0, sc, bias, variant), f"w8 cfg {cfg}")
    close_f64(out, acc64(a, w), b0, sc, bias, f"w8 cfg {cfg}")

    if case["residual"]:
        res = dd.normal_f16(s + 5, (M, N), 2.0)
        fused = gemm(C, ad, t(w), scd, b0d, bd, _cfg=cfg, _residual=t(res))
        assert torch.equal(fused, out + t(res)), f"residual cfg {cfg}"
        bits_equal(fused, oracle.add_f16(out.cpu().numpy(), res), f"residual cfg {cfg}")
    if case["rowmap"]:
        g = next(d for d in (7, 5, 3, 2, 1) if M % d == 0)        # g groups of M / g rows
        rows = M // g
        o = torch.full((g, rows + 1, N), 7.0, dtype=torch.float16, device=DEV)
        gemm(C, ad, t(w), scd, b0d, bd, _cfg=cfg, _out=o, _row_map=(rows, rows + 1, 1))
        assert torch.equal(o[:, 1:].reshape(M, N), out), f"row map cfg {cfg}"
        assert bool((o[:, 0] == 7.0).all()), f"row map cfg {cfg}: a row outside the map was written"

    if case["w4"]:
        q4 = dd.int8(s + 6, (N, K), -8, 8)
        p4 = pack_w4(torch.from_numpy(q4))
        assert np.array_equal(oracle.unpack_w4(p4.numpy()), q4)
        o4 = gemm(C, ad, p4.to(DEV), scd, b0d, bd, _cfg=cfg, _w4=True)
        bits_equal(o4, oracle.qlinear(a, oracle.unpack_w4(p4.numpy()), b0, sc, bias, variant), f"w4 cfg {cfg}")
        close_f64(o4, acc64(a, q4), b0, sc, bias, f"w4 cfg {cfg}")
    else:
        with pytest.raises(RuntimeError, match="K % 32"):
            gemm(C, ad, torch.zeros(N, K // 2, dtype=torch.int8, device=DEV), scd, b0d, bd, _cfg=cfg, _w4=True)

    if case["w2"] and te.w2_admissible(cfg):
        q2 = dd.int8(s + 7, (N, K), -2, 2)
        p2 = pack_w2(torch.from_numpy(q2))
        assert torch.equal(unpack_w2(p2), torch.from_numpy(q2))
        o2 = gemm(C, ad, p2.to(DEV), scd, b0d, bd, _cfg=cfg, _w2=True)
        bits_equal(o2, oracle.qlinear(a, unpack_w2(p2).numpy(), b0, sc, bias, variant), f"w2 cfg {cfg}")
        close_f64(o2, acc64(a, q2), b0, sc, bias, f"w2 cfg {cfg}")
    else:                       # K % 64 != 0, or a tile whose weight stage is not whole packed pieces
        with pytest.raises(RuntimeError, match="packed 2-bit weights"):
            gemm(C, ad, torch.zeros(N, K // 4, dtype=torch.int8, device=DEV), scd, b0d, bd, _cfg=cfg, _w2=True)


# ------------------------------------------------------------------------------- INT8 conv, every id
CONV = te.all_conv()


@pytest.mark.parametrize("case", CONV, ids=[te.conv_id(c) for c in CONV])
def test_conv_tile_edges(C, oracle, case):
    from mixdq_amd.nn.utils import pack_w4
    cfg, n, H, W, Cin, K, R = (case[k] for k in ("cfg", "n", "H", "W", "C", "K", "R"))
    stride, pad = case["stride"], case["pad"]
    s = seed_of(cfg, n, H, W, Cin, K, R, stride, pad)
    variant = C.FLAGS & 1
    zp = np.float32(-11.0)
    x = dd.int8(s, (n, H, W, Cin))
    sc = dd.f32(s + 2, (K,), 1e-4, 6e-4)
    bias = dd.f16(s + 3, (K,), -1, 1) if (cfg + R + pad) % 2 else None
    xd = t(x).permute(0, 3, 1, 2)
    forms = [("w8", dd.int8(s + 1, (K, R, R, Cin)))]
    if Cin % 32 == 0:
        forms.append(("w4", dd.int8(s + 4, (K, R, R, Cin), -8, 8)))
    else:
        win = torch.zeros(K, R, R, Cin // 2, dtype=torch.int8, device=DEV).permute(0, 3, 1, 2)
        ws = torch.ones(K, 1, R, R, device=DEV)
        with pytest.raises(RuntimeError, match="K % 32"):
            C.qconv2d_w8_a8_ohalf(xd, win, t(sc), scal(1), scal(zp), t(sc), ws, ws.reshape(K, -1)[:, 0].contiguous(),
                                  None, stride, pad, _w4=True, _cfg=cfg)
    for form, q in forms:
        wsum = q.astype(np.float32).sum(axis=3, dtype=np.float32)                     # [K, R, S]
        bias0 = (wsum.reshape(K, -1).sum(axis=1, dtype=np.float32) * zp).astype(np.float32)
        if form == "w4":
            packed = pack_w4(torch.from_numpy(q))
            assert np.array_equal(oracle.unpack_w4(packed.numpy()), q)
            win, wq = packed.to(DEV).permute(0, 3, 1, 2), oracle.unpack_w4(packed.numpy())
        else:
            win, wq = t(q).permute(0, 3, 1, 2), q
        out = C.qconv2d_w8_a8_ohalf(xd, win, t(sc), scal(1), scal(zp), t(sc),
                                    t(wsum.reshape(K, 1, R, R)) if pad else None, None if pad else t(bias0),
                                    None if bias is None else t(bias), stride, pad, _w4=form == "w4", _cfg=cfg)
        got = out.permute(0, 2, 3, 1).contiguous().cpu().numpy()
        want = oracle.qconv2d(x, wq, sc, wsum if pad else None, zp, None if pad else bias0, bias, stride, pad,
                              variant)
        bits_equal(got, want, f"{form} conv cfg {cfg}")
        # float64: the zero point's share is zp x the weight sums of the taps inside the image
        xf = torch.from_numpy(x).permute(0, 3, 1, 2).double()
        wf = torch.from_numpy(q).permute(0, 3, 1, 2).double()
        acc = F.conv2d(xf, wf, stride=stride, padding=pad)
        b0 = float(zp) * F.conv2d(torch.ones(n, 1, H, W, dtype=torch.float64),
                                  torch.from_numpy(wsum).double().reshape(K, 1, R, R), stride=stride, padding=pad)
        acc = acc.permute(0, 2, 3, 1).reshape(-1, K).numpy()
        b0 = b0.permute(0, 2, 3, 1).reshape(-1, K).numpy()
        close_f64(got.reshape(-1, K), acc, b0, sc, bias, f"{form} conv cfg {cfg}")


# --------------------------------------------------------------------------------- GEMM + GEGLU
GEGLU = te.all_geglu()


@pytest.mark.parametrize("case", GEGLU, ids=[te.geglu_id(c) for c in GEGLU])
def test_geglu_tile_edges(C, oracle, case):
    """The fused launch == the oracle's qlinear -> geglu_quantize chain == the HIP two-launch chain."""
    cfg, M, N, K = case["cfg"], case["M"], case["N"], case["K"]
    s = seed_of(cfg, M, N, K, 5)
    variant = C.FLAGS & 1
    D = N // 2
    a, w = dd.int8(s, (M, K)), dd.int8(s + 1, (N, K))
    scale, bias0 = dd.f32(s + 2, (N,), 2e-4, 9e-4), dd.f32(s + 3, (N,), -300, 300)
    bias = dd.normal_f16(s + 4, (N,), 0.5) if case["bias"] else None
    s_inv, zp = float(np.float32(1) / np.float32(0.02)), -60.0
    q_ref, _ = oracle.geglu_quantize(oracle.qlinear(a, w, bias0, scale, bias, variant), s_inv, zp, variant)
    perm = C.geglu_row_order(D, DEV)
    got = C.qlinear_geglu(t(a), t(w)[perm].contiguous(), t(scale)[perm].contiguous(), t(bias0)[perm].contiguous(),
                          None if bias is None else t(bias)[perm].contiguous(), scal(s_inv), scal(zp), _cfg=cfg)
    bits_equal(got, q_ref, f"geglu cfg {cfg}")
    h = gemm(C, t(a), t(w), t(scale), t(bias0), None if bias is None else t(bias))
    assert torch.equal(got, C.geglu_quantize(h, scal(s_inv), scal(zp))[0]), f"geglu cfg {cfg} vs two launches"


@pytest.mark.parametrize("cfg", [c for c in sorted(te.IGEMM) if not te.geglu_admissible(c)])
def test_geglu_refuses_tiles_without_whole_groups(C, cfg):
    bm, bn, bk, st = te.tile(cfg)
    a = torch.zeros(bm + 1, bk, dtype=torch.int8, device=DEV)
    w = torch.zeros(2 * bn, bk, dtype=torch.int8, device=DEV) if bn % 32 == 0 else \
        torch.zeros(320, bk, dtype=torch.int8, device=DEV)
    v = torch.ones(w.size(0), device=DEV)
    with pytest.raises(RuntimeError, match="N % 32"):
        C.qlinear_geglu(a, w, v, v, None, scal(1.0), scal(0.0), _cfg=cfg)


# ------------------------------------------------------------------- persistent 256x256 (configuration 71)
PP = te.pp_cases()


@pytest.mark.parametrize("case", PP, ids=[te.pp_id(c) for c in PP])
def test_persistent_kernel_grid_edges_equal_70_and_the_oracle(C, oracle, case):
    M, N, K, form = case["M"], case["N"], case["K"], case["form"]
    s = seed_of(M, N, K, 71)
    variant = C.FLAGS & 1
    a, w = dd.int8(s, (M, K)), dd.int8(s + 1, (N, K))
    scale, bias0 = dd.f32(s + 2, (N,), 2e-4, 9e-4), dd.f32(s + 3, (N,), -300, 300)
    bias = dd.normal_f16(s + 4, (N,), 0.5) if case["bias"] else None
    want = oracle.qlinear(a, w, bias0, scale, bias, variant)
    if form == "geglu":
        D = N // 2
        s_inv, zp = float(np.float32(1) / np.float32(0.02)), -60.0
        perm = C.geglu_row_order(D, DEV)
        args = (t(a), t(w)[perm].contiguous(), t(scale)[perm].contiguous(), t(bias0)[perm].contiguous(),
                None if bias is None else t(bias)[perm].contiguous(), scal(s_inv), scal(zp))
        got = C.qlinear_geglu(*args, _cfg=71)
        bits_equal(got, oracle.geglu_quantize(want, s_inv, zp, variant)[0], "geglu 71")
        assert torch.equal(got, C.qlinear_geglu(*args, _cfg=70)), "geglu 71 != 70"
        return
    kw = {}
    if form == "residual":
        r = dd.normal_f16(s + 5, (M, N), 1.5)
        kw = dict(_residual=t(r))
        want = oracle.add_f16(want, r)
    args = (t(a), t(w), t(scale), t(bias0), None if bias is None else t(bias))
    got = gemm(C, *args, _cfg=71, **kw)
    bits_equal(got, want, f"{form} 71")
    assert torch.equal(got.view(torch.int16), gemm(C, *args, _cfg=70, **kw).view(torch.int16)), f"{form} 71 != 70"
    if form == "f16":
        close_f64(got, acc64(a, w), bias0, scale, bias, "71")


# --------------------------------------------------------------------- quantize in the prologue (f16in)
F16IN = te.all_f16in()


@pytest.mark.parametrize("case", F16IN, ids=[te.f16in_id(c) for c in F16IN])
def test_f16in_tile_edges(C, oracle, case):
    """One launch == quantize -> GEMM on the same tile == the oracle; a K tail is refused (MIXDQ_ERR_SHAPE)."""
    cfg, M, N, K = case["cfg"], case["M"], case["N"], case["K"]
    s = seed_of(cfg, M, N, K, 16)
    variant = C.FLAGS & 1
    x = dd.f16(s, (M, K), -4, 4)
    w = dd.int8(s + 1, (N, K))
    sc, b0 = dd.f32(s + 2, (N,), 1e-4, 1e-3), dd.f32(s + 3, (N,), -500, 500)
    bias = dd.f16(s + 4, (N,), -1, 1) if case["bias"] else None
    s_inv, zp = 31.37, -9.0                      # |x| <= 4: both rails clamp
    args = (t(w), t(sc), t(b0), None if bias is None else t(bias))
    got = C.qlinear_f16in(t(x), scal(s_inv), scal(zp), *args, _cfg=cfg)
    want = oracle.qlinear(oracle.quantize(x, s_inv, zp, variant), w, b0, sc, bias, variant)
    bits_equal(got, want, f"f16in cfg {cfg}")
    q = C.quantize_per_tensor_to_int8(t(x), scal(s_inv), scal(zp))
    two = C.qlinear_w8_a8_ohalf(q, t(w), t(sc), scal(1), scal(0), t(b0), t(sc), t(b0), args[3], _cfg=cfg)
    assert torch.equal(got, two), f"f16in cfg {cfg} vs two launches"
    if K > 16:
        with pytest.raises(RuntimeError, match="shape outside"):
            C.qlinear_f16in(t(x[:, :K - 16]), scal(s_inv), scal(zp), t(w[:, :K - 16]), *args[1:], _cfg=cfg)


# ----------------------------------------------------------------------------------- FP16 layers
F16L = te.all_f16()


def close_f16(out, ref):
    ref = ref.to(out.device).float()
    tol = 2.0 ** -10 * ref.abs() + 2.0 ** -10 * ref.pow(2).mean().sqrt()
    err = (out.float() - ref).abs()
    bad = err > tol
    assert not bad.any(), f"{int(bad.sum())} of {bad.numel()} outside tolerance; max err {err.max().item():.3e}"


@pytest.mark.parametrize("case", F16L, ids=[te.f16_id(c) for c in F16L])
def test_f16_tile_edges_every_configuration_same_bits(C, case):
    M, N, K = case["M"], case["N"], case["K"]
    g = torch.Generator(device="cpu").manual_seed(seed_of(case["cfg"], M, N, K))
    x = torch.randn((M, K), generator=g).half()
    w = (torch.randn((N, K), generator=g) * 0.05).half()
    b = torch.randn((N,), generator=g).half() if case["bias"] else None
    ref = F.linear(x.double(), w.double(), None if b is None else b.double())
    xd, wd, bd = x.to(DEV), w.to(DEV), None if b is None else b.to(DEV)
    outs = {cfg: C.linear_f16(xd, wd, bd, _cfg=cfg) for cfg in sorted(te.F16)}
    first = outs[case["cfg"]]
    close_f16(first, ref)
    for cfg, o in outs.items():
        assert torch.equal(o, first), f"FP16 cfg {cfg} != cfg {case['cfg']}"


# ------------------------------------------------------------------------------------ grouped launch
GROUPED = te.all_grouped()


@pytest.mark.parametrize("case", GROUPED, ids=[te.grouped_id(c) for c in GROUPED])
def test_grouped_tile_edges_members_equal_their_own_launches(C, oracle, case):
    cfg, M, K = case["cfg"], case["M"], case["K"]
    s = seed_of(cfg, M, K, 9)
    a = dd.int8(s, (M, K))
    members, singles, wants, outs = [], [], [], []
    for i, N in enumerate(case["Ns"]):
        q = dd.int8(s + 10 + i, (N, K))
        b0, sc = dd.f32(s + 20 + i, (N,), -300, 300), dd.f32(s + 30 + i, (N,), 1e-4, 1e-3)
        bias = dd.f16(s + 40 + i, (N,), -1, 1) if i % 2 else None
        wants.append(oracle.qlinear(a, q, b0, sc, bias, C.FLAGS & 1))
        singles.append(gemm(C, t(a), t(q), t(sc), t(b0), None if bias is None else t(bias), _cfg=cfg))
        out = torch.full((M, N), 7.0, dtype=torch.float16, device=DEV)
        outs.append(out)
        members.append((t(q), t(b0), t(sc), None if bias is None else t(bias), out))
    table = C.GemmGroupTable(members)
    C.qlinear_grouped(t(a), table, _cfg=cfg)
    for i, (o, single, want) in enumerate(zip(outs, singles, wants)):
        assert torch.equal(o, single), f"member {i} (N = {case['Ns'][i]}) != its own launch, cfg {cfg}"
        bits_equal(o, want, f"member {i} cfg {cfg}")
