"""Every capped-grid launch of tests/grid_caps.py's new rows, run past its cap: more work items than kNumCU * per_cu *
256, so every lane takes its grid-stride loop a second time (and some lanes not: the last trip is partial).

Every comparison is equality of bits with a restatement that shares no code with the kernel: tests/inpaint_ref.py,
inpaint9_ref.py (its ingest is vae_enc_ref.py's), ip2p_ref.py, rng_ref.py, conv_geometry.py's tap-rectangle sums, the C
oracle's qlinear, qconv2d, zp_propagate and gemm_f16, and -- for the 34 M-element masks of mask_to_latent and for the
radius-40 growth -- stock torch on the device (F.max_pool2d of the binarisation).  No tolerances.

Inputs are index-coded (tests/grid_caps.py's generators: a misplaced element is a mismatch with certainty), masks are
planted with set and clear runs across the first item of the second trip, and the arithmetic kernels run a random input
as well.  Every output is written, through the C ABI, into a buffer pre-filled with a sentinel byte that the expected
result does not contain, with guard bytes on both sides that must stay untouched.  Each test asserts that its shape is
the table's: tests/test_grid_caps_host.py has traced that very call to a grid at the cap."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_geometry as cg
from tests import detdata as dd
from tests import grid_caps as gc
from tests import inpaint9_ref as I9
from tests import inpaint_ref as I
from tests import ip2p_ref as P
from tests import launch_trace as lt
from tests import rng_ref as G

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 256
SIGNATURES = lt.signatures()               # {entry point: [(argument name, ctype)]} of include/mixdq_hip.h
TORCH = {gc.U8: torch.uint8, gc.F16: torch.float16, gc.F32: torch.float32}
CAP8, CAP32 = gc.cap_items(8), gc.cap_items(32)


# ------------------------------------------------------------------------------------------------------ helpers
class Guarded:
    """Device memory for the expected result `want`, pre-filled with a sentinel byte and lying between two guard zones of
    the same byte.  The sentinel is one whose repetition is no element of `want` (an unwritten element cannot pass);
    byte results, where every value may occur, run under two sentinels instead."""

    def __init__(self, want, dtype, sentinel=None, dev=DEV):
        self.want = _bits(np.ascontiguousarray(want))
        size = self.want.itemsize
        if sentinel is None:
            present = set(np.unique(self.want).tolist())
            sentinel = next(b for b in (0xA5, 0x5A, 0xC3, 0x3C, 0x96, 0x69)
                            if int.from_bytes(bytes([b]) * size, "little") not in present)
        self.nbytes, self.sentinel = self.want.nbytes, sentinel
        self.buf = torch.full((GUARD + self.nbytes + GUARD,), sentinel, dtype=torch.uint8, device=dev)
        self.out = self.buf[GUARD:GUARD + self.nbytes].view(dtype)

    def check(self, what):
        """The guards are untouched and the output equals the expected result bit for bit."""
        assert bool((self.buf[:GUARD] == self.sentinel).all()), f"{what}: bytes before the output were written"
        assert bool((self.buf[GUARD + self.nbytes:] == self.sentinel).all()), f"{what}: bytes behind the output were written"
        g = _bits(self.out.cpu().numpy()).reshape(-1)
        assert g.size == self.want.size, (g.size, self.want.size)
        bad = np.flatnonzero(g != self.want.reshape(-1))
        assert bad.size == 0, f"{what}: {bad.size} of {g.size} elements differ, first at flat index {bad[0]}"


def _bits(a):
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.itemsize])


def call(C, c, flags=None, **tensors):
    """The case's entry point: the table's scalar arguments, NULL where the table says so, these tensors elsewhere.
    A pointer sits where the table's trace had it: `ptr_off` bytes past a 16-byte boundary."""
    a = dict(gc.entry_args(c))
    if flags is not None:
        a["flags"] = flags                  # (the epilogue variant of the process: the table traced flags = 0)
    for name in c["null"]:
        a[name] = None
    for name, t in tensors.items():
        assert t.data_ptr() % 16 == c["ptr_off"].get(name, 0), (name, t.data_ptr() % 16)
        a[name] = t.data_ptr()
    a["stream"] = torch.cuda.current_stream().cuda_stream
    names = [n for n, _ in SIGNATURES[c["entry"]]]
    assert sorted(a) == sorted(names), (sorted(set(a) ^ set(names)))
    code = getattr(C._lib, c["entry"])(*(a[n] for n in names))
    torch.cuda.synchronize()
    assert code == 0, (c["entry"], code)


def pixel_index(B, H, W, dev):
    i = torch.arange(B * H * W, device=dev).view(B, H, W)
    return i, (i // W) % H, i % W


def planted_mask(set_, i, dtype, layout, dev):
    """A [B, H, W] mask of element type `dtype` that binarises to `set_`: dense, or every second element of rows twice
    as long whose other elements hold the opposite decision."""
    v = gc.mask_values(set_, i, dtype, torch).to(TORCH[dtype])
    if layout == "dense":
        return v
    back = torch.empty(v.shape[:2] + (2 * v.shape[2],), dtype=TORCH[dtype], device=dev)
    back[..., ::2] = v
    back[..., 1::2] = gc.mask_values(~set_, i, dtype, torch).to(TORCH[dtype])
    return back[..., ::2]


def coded_image(i, C, dtype):
    """[B, C, H, W] of the byte code (7 i + c) % 251: bytes, or the same small integers centred on zero as floats."""
    code = torch.stack([gc.image_code(i, ch) for ch in range(C)], dim=1)
    return code.to(torch.uint8) if dtype == gc.U8 else (code - 125).to(TORCH[dtype])


def both(a, what):
    assert bool(a.any()) and not bool(a.all()), f"{what}: all set or all clear"


def mask_strides(m):
    return dict(zip(("mb", "mh", "mw"), m.stride()))


# ------------------------------------------------------------------------------------------------- csrc/vae.hip
def composite_case(c, dev):
    a = c["args"]
    assert a == gc.composite_args(a["mask_dtype"], c["layout"]) and gc.B_ * gc.H_ * gc.W_ == c["items"]
    B, H, W = a["B"], a["H"], a["W"]
    i, _, _ = pixel_index(B, H, W, dev)
    dec = ((torch.stack([gc.image_code(i, 5 + ch) for ch in range(3)], dim=1) - 125).float() / 104).half()   # [-1.2, 1.2]
    orig = coded_image(i, 3, gc.U8)
    set_ = gc.pattern(i, CAP8)
    mask = planted_mask(set_, i, a["mask_dtype"], c["layout"], dev)
    if c["layout"] == "strided":
        dec = dec.contiguous(memory_format=torch.channels_last)
        back = torch.full((B, 3, H, W + 3), 77, dtype=torch.uint8, device=dev)
        back[..., :W] = orig
        orig = back[..., :W]
    assert dict(zip(("db", "dc", "dh", "dw"), dec.stride()), **dict(zip(("ob", "oc", "oh", "ow"), orig.stride())),
                **mask_strides(mask)) == {k: a[k] for k in ("db", "dc", "dh", "dw", "ob", "oc", "oh", "ow", "mb", "mh", "mw")}
    s = I.mask_set(mask.cpu().numpy())
    both(s.reshape(-1)[CAP8:], "the mask within the second trip")
    painted = I.to_uint8(dec.cpu().numpy().transpose(0, 2, 3, 1))
    assert painted.min() == 0 and painted.max() == 255
    want = np.where(s[..., None], painted, orig.cpu().numpy().transpose(0, 2, 3, 1))
    return (dec, orig, mask), want


@pytest.mark.parametrize("c", **gc.by_test("test_composite"))
def test_composite(C, c):
    (dec, orig, mask), want = composite_case(c, DEV)
    for sentinel in (0xA5, 0x5A):           # bytes: an unwritten one differs from the expected under one of the two
        g = Guarded(want, torch.uint8, sentinel)
        call(C, c, decoded_f16=dec, original=orig, mask=mask, out=g.out)
        g.check(f"composite_u8 {c['name']}")


def ingest_masked_case(c, dev):
    a = c["args"]
    assert a == gc.ingest_masked_args(a["dtype"], a["mask_dtype"], a["C"], c["layout"]) and c["items"] == gc.PIXELS
    B, H, W = a["B"], a["H"], a["W"]
    i, _, _ = pixel_index(B, H, W, dev)
    img = coded_image(i, a["C"], a["dtype"])
    set_ = gc.pattern(i, CAP8)
    mask = planted_mask(set_, i, a["mask_dtype"], c["layout"], dev)
    if c["layout"] == "strided":
        img = img.contiguous(memory_format=torch.channels_last)
    assert dict(zip(("sb", "sc", "sh", "sw"), img.stride()), **mask_strides(mask)) == \
        {k: a[k] for k in ("sb", "sc", "sh", "sw", "mb", "mh", "mw")}
    both(I.mask_set(mask.cpu().numpy()).reshape(-1)[CAP8:], "the mask within the second trip")
    return (img, mask), I9.ingest_masked(img.cpu().numpy(), mask.cpu().numpy())


@pytest.mark.parametrize("c", **gc.by_test("test_ingest_masked"))
def test_ingest_masked(C, c):
    (img, mask), want = ingest_masked_case(c, DEV)
    g = Guarded(want, torch.float16)
    call(C, c, img=img, mask=mask, out_f16=g.out)
    g.check(f"image_to_nhwc8_f16_masked {c['name']}")


def mask_to_latent_case(c, dev):
    """The mask built on the device from its latent-resolution planting (tests/grid_caps.latent_planting): per 8x8 block
    pixel (0, 0) and one moving decoy pixel.  Expected: stock torch on the mask itself -- and that is what was planted."""
    a = c["args"]
    narrow = c["layout"] == "narrow"
    assert a == gc.mask_to_latent_args(a["dtype"], a["mode"], narrow) and c["items"] == gc.PIXELS
    B, H, W, dt = a["B"], a["H"], a["W"], TORCH[a["dtype"]]
    back = torch.zeros((B, H, a["sh"]), dtype=dt, device=dev)
    if narrow:                              # set elements on both sides of the view: a read beside it finds them
        back[..., 0] = 255 if a["dtype"] == gc.U8 else 1.0
        back[..., W + 1:] = 255 if a["dtype"] == gc.U8 else 1.0
    mask = back[..., 1:W + 1] if narrow else back
    assert tuple(mask.stride()) == (a["sb"], a["sh"], a["sw"]) and tuple(mask.shape) == (B, H, W)
    j, y, x = pixel_index(B, H // 8, W // 8, dev)
    p, q, r, cc = gc.latent_planting(j, CAP8)
    mask[:, ::8, ::8] = gc.mask_values(p, j, a["dtype"], torch).to(dt)
    mask[j // ((H // 8) * (W // 8)), 8 * y + r, 8 * x + cc] = gc.mask_values(q, j + 1, a["dtype"], torch).to(dt)
    binar = (mask >= 128) if a["dtype"] == gc.U8 else (mask.float() >= 0.5)
    if a["mode"] == 0:
        want, planted = binar[:, ::8, ::8].float(), p
    else:
        want, planted = F.max_pool2d(binar[:, None].float(), 8)[:, 0], p | q
    assert torch.equal(want, planted.float())
    both(want.reshape(-1)[CAP8:] == 1, "the latent mask within the second trip")
    return mask, want.cpu().numpy()


@pytest.mark.parametrize("c", **gc.by_test("test_mask_to_latent"))
def test_mask_to_latent(C, c):
    mask, want = mask_to_latent_case(c, DEV)
    g = Guarded(want, torch.float32)
    call(C, c, mask=mask, out=g.out)
    g.check(f"mask_to_latent {c['name']}")


def inpaint_cond_case(c, dev):
    a = c["args"]
    assert a["pixels"] == gc.PIXELS == c["items"]
    n, L = a["pixels"], a["L"]
    i = torch.arange(n, device=dev)
    mask_lat = gc.mask_values(gc.pattern(i, CAP8), i, gc.F32, torch).float()       # (a soft mask: the values pass through)
    zl = torch.stack([(gc.image_code(i, ch) - 125).float() * 0.3 for ch in range(L)], dim=1)
    off = c["ptr_off"].get("zl", 0) // 4
    store = torch.full((n * L + 4,), 9.0, device=dev)
    store[off:off + n * L] = zl.reshape(-1)
    zl = store[off:off + n * L].view(n, L)
    want = I9.inpaint_cond(mask_lat.cpu().numpy().reshape(gc.B_, gc.H_, gc.W_),
                           zl.cpu().numpy().reshape(gc.B_, gc.H_, gc.W_, L))
    return (mask_lat, zl), want


@pytest.mark.parametrize("c", **gc.by_test("test_inpaint_cond"))
def test_inpaint_cond(C, c):
    (mask_lat, zl), want = inpaint_cond_case(c, DEV)
    g = Guarded(want, torch.float16)
    call(C, c, mask_lat=mask_lat, zl=zl, out_f16=g.out)
    g.check(f"inpaint_cond_f16 {c['name']}")


def ip2p_cond_case(c, dev):
    a = c["args"]
    assert (a["B"], a["pixels_per_image"]) == (gc.B_, gc.H_ * gc.W_) and c["items"] == gc.PIXELS
    n, L = gc.PIXELS, a["L"]
    i = torch.arange(n, device=dev)
    mean = [(gc.image_code(i, ch) - 125).float() * 0.03 for ch in range(L)]
    logvar = [torch.full((n,), 7.0 + ch, device=dev) for ch in range(L)]            # never read
    moments = torch.stack(mean + logvar, dim=1).half()
    want = P.ip2p_cond(moments.cpu().numpy().reshape(gc.B_, gc.H_, gc.W_, 2 * L), a["rows"], a["scale"])
    return moments, want


@pytest.mark.parametrize("c", **gc.by_test("test_ip2p_cond"))
def test_ip2p_cond(C, c):
    """rows 3: all three row blocks -- the second trip writes at total + i and 2 * total + i as well."""
    moments, want = ip2p_cond_case(c, DEV)
    assert want.shape[0] == c["args"]["rows"] * gc.B_
    if c["args"]["rows"] == 3:
        assert want[:gc.B_].any() and np.array_equal(want[:gc.B_], want[gc.B_:2 * gc.B_]) and not want[2 * gc.B_:].any()
    g = Guarded(want, torch.float16)
    call(C, c, moments_f16=moments, out_f16=g.out)
    g.check(f"ip2p_cond_f16 {c['name']}")


# ----------------------------------------------------------------------------------------------- csrc/image.hip
def mask_dilate_case(c, dev):
    a = c["args"]
    assert a == gc.dilate_args(a["dtype"], a["radius"], c["layout"]) and c["items"] == 2 * gc.DIL_H * gc.DIL_W
    i, y, x = pixel_index(a["B"], a["H"], a["W"], dev)
    seed = gc.dilate_seed(i, y, x, CAP32)
    mask = planted_mask(seed, i, a["dtype"], c["layout"], dev)
    assert tuple(mask.stride()) == (a["sb"], a["sh"], a["sw"])
    binar = (mask >= 128) if a["dtype"] == gc.U8 else (mask.float() >= 0.5)
    assert torch.equal(binar, seed)
    r = a["radius"]
    rows = F.max_pool2d(binar[:, None].float(), (1, 2 * r + 1), stride=1, padding=(0, r))      # (a maximum is separable)
    grown = F.max_pool2d(rows, (2 * r + 1, 1), stride=1, padding=(r, 0))[:, 0] > 0
    both(grown.reshape(-1)[CAP32:], "the grown mask within the second trip")
    want = np.where(grown.cpu().numpy(), np.uint8(255), np.uint8(0))
    if r == 2 and c["layout"] == "dense":   # ... and the definition in numpy, where it is quick
        assert np.array_equal(want, I9.mask_dilate(mask.cpu().numpy(), r))
    return mask, want


@pytest.mark.parametrize("c", **gc.by_test("test_mask_dilate"))
def test_mask_dilate(C, c):
    mask, want = mask_dilate_case(c, DEV)
    scratch = torch.full((want.size,), 0x3C, dtype=torch.uint8, device=DEV)
    g = Guarded(want, torch.uint8)
    call(C, c, mask=mask, scratch=scratch, out=g.out)
    g.check(f"mask_dilate_u8 {c['name']}")


# ----------------------------------------------------------------------------------------------- csrc/igemm.hip
def coded_int8(shape, mult, mod):
    """int8 of the flat index: (mult * i) % mod - mod // 2 (mod <= 255, prime to mult)."""
    n = int(np.prod(shape))
    return ((np.arange(n, dtype=np.int64) * mult) % mod - mod // 2).astype(np.int8).reshape(shape)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("data", ["coded", "random"])
@pytest.mark.parametrize("c", **gc.by_test("test_igemm_generic_linear"))
def test_igemm_generic_linear(C, oracle, c, data):
    a = c["args"]
    M, N, K = a["M"], a["N"], a["K"]
    assert a == gc.LINEAR and M * N == c["items"]
    if data == "coded":
        A, W = coded_int8((M, K), 7, 251), coded_int8((N, K), 11, 241)
    else:
        A, W = dd.int8(901, (M, K)), dd.int8(902, (N, K))
    bias0, scale, bias = dd.f32(903, (N,), -300, 300), dd.f32(904, (N,), 1e-4, 6e-4), dd.f16(905, (N,), -1, 1)
    want = oracle.qlinear(A, W, bias0, scale, bias, C.FLAGS & 1)
    g = Guarded(want, torch.float16)
    call(C, c, flags=C.FLAGS, A=_dev(A), W=_dev(W), bias0=_dev(bias0), scale=_dev(scale), bias_f16_or_null=_dev(bias),
         D_f16=g.out)
    g.check(f"qlinear generic {data}")


def border_table_ref(wsum):
    """mixdq_conv_border_table of wsum [K, R, S] in numpy: row ((rlo R + rhi) S + slo) S + shi holds the tap-rectangle
    sums (tests/conv_geometry.rect_sum), zeros where the rectangle is empty."""
    K, R, S = wsum.shape
    table = np.zeros((R * R * S * S, K), np.float32)
    for rlo in range(R):
        for rhi in range(rlo, R):
            for slo in range(S):
                for shi in range(slo, S):
                    table[cg.class_index(R, S, rlo, rhi, slo, shi)] = cg.rect_sum(wsum, rlo, rhi, slo, shi)
    return table


@pytest.mark.parametrize("data", ["coded", "random"])
@pytest.mark.parametrize("c", **gc.by_test("test_igemm_generic_conv"))
def test_igemm_generic_conv(C, oracle, c, data):
    """pad 1: bias0 from the border table (made here in numpy); pad 0: the bias0 vector."""
    a = c["args"]
    assert a == gc.conv_args(a["pad"]) and c["items"] == 58 * 57 * 320
    n, H, W, Cin, K, pad = a["N"], a["H"], a["W"], a["C"], a["K"], a["pad"]
    if data == "coded":
        x, w = coded_int8((n, H, W, Cin), 7, 251), coded_int8((K, 3, 3, Cin), 11, 241)
    else:
        x, w = dd.int8(911, (n, H, W, Cin)), dd.int8(912, (K, 3, 3, Cin))
    scale, bias = dd.f32(913, (K,), 1e-4, 6e-4), dd.f16(914, (K,), -1, 1)
    wsum = cg.wsum_of(w)
    zp = np.array([cg.ZP], np.float32)
    bias0 = None if pad else dd.f32(915, (K,), -300, 300)
    want = oracle.qconv2d(x, w, scale, wsum if pad else None, cg.ZP, bias0, bias, 1, pad, C.FLAGS & 1)
    assert want.shape == (1, 58, 57, 320)
    g = Guarded(want, torch.float16)
    more = dict(table_or_null=_dev(border_table_ref(wsum))) if pad else dict(bias0_or_null=_dev(bias0))
    call(C, c, flags=C.FLAGS, X_nhwc=_dev(x), Wt_krsc=_dev(w), scale=_dev(scale), zero_point=_dev(zp),
         bias_f16_or_null=_dev(bias), D_nhwc_f16=g.out, **more)
    g.check(f"qconv2d generic pad {pad} {data}")


@pytest.mark.parametrize("data", ["coded", "random"])
@pytest.mark.parametrize("c", **gc.by_test("test_gemm_f16"))
def test_gemm_f16(C, oracle, c, data):
    a = c["args"]
    M, N, K = a["M"], a["N"], a["K"]
    assert (M, N, K) == (1031, 1020, 8) and M * N == c["items"]
    if data == "coded":                     # small integers: exact in any order, and no two neighbours alike
        A, Bm = coded_int8((M, K), 7, 251).astype(np.float16), coded_int8((K, N), 11, 241).astype(np.float16)
        A = A * np.float16(0.125)
    else:
        A, Bm = dd.normal_f16(921, (M, K), 1.0), dd.normal_f16(922, (K, N), 1.0)
    want = oracle.gemm_f16(A, Bm)
    g = Guarded(want, torch.float16)
    call(C, c, A_f16=_dev(A), B_f16_kn=_dev(Bm), D_f16=g.out)
    g.check(f"gemm_f16 {data}")


def coded_wsum(K, mult, mod):
    return ((np.arange(K * 9, dtype=np.int64) * mult) % mod - mod // 2).astype(np.float32).reshape(K, 3, 3)


@pytest.mark.parametrize("data", ["coded", "random"])
@pytest.mark.parametrize("c", **gc.by_test("test_zp_propagate"))
def test_zp_propagate(C, oracle, c, data):
    a = c["args"]
    assert c["items"] == a["N"] * 29 * 31 * a["K"] and (a["H"], a["W"], a["R"], a["S"], a["pad"]) == (29, 31, 3, 3, 1)
    K = a["K"]
    if data == "coded":
        wsum, zp = coded_wsum(K, 13, 2003), -11.0
    else:                                   # tap sums of random int8 weights over 320 channels: integers, as in a layer
        wsum, zp = dd.int8(931, (K, 3, 3, 320)).astype(np.float32).sum(axis=3, dtype=np.float32), 3.0
    want = oracle.zp_propagate(wsum, zp, a["N"], a["H"], a["W"], a["stride"], a["pad"])
    g = Guarded(want, torch.float32)
    call(C, c, wsum_krs=_dev(wsum), zero_point=_dev(np.array([zp], np.float32)), out_npqk=g.out)
    g.check(f"zp_propagate {data}")


@pytest.mark.parametrize("c", **gc.by_test("test_border_table"))
def test_border_table(C, c):
    a = c["args"]
    assert c["items"] == 81 * a["K"] and (a["R"], a["S"]) == (3, 3)
    wsum = coded_wsum(a["K"], 13, 2003)
    want = border_table_ref(wsum)
    g = Guarded(want, torch.float32)
    call(C, c, wsum_krs=_dev(wsum), table=g.out)
    g.check("conv_border_table")


# -------------------------------------------------------------------------------------------- csrc/quantize.hip
@pytest.mark.parametrize("data", ["coded", "random"])
@pytest.mark.parametrize("c", **gc.by_test("test_embed_tokens"))
def test_embed_tokens(C, c, data):
    a = c["args"]
    B, T, Cw, V = a["B"], a["T"], a["C"], a["V"]
    assert B * T * (Cw // 8) == c["items"]
    ids = gc.token_ids(np.arange(B * T), V).astype(np.int32).reshape(B, T)
    if data == "coded":                     # tok: integers (exact); pos: quarters -- the sum is rounded to FP16
        tok = ((np.arange(V * Cw) % 2039) - 1019).astype(np.float16).reshape(V, Cw)
        pos = (((np.arange(T * Cw) * 3) % 1021) * 0.25 - 100).astype(np.float16).reshape(T, Cw)
    else:
        tok, pos = dd.normal_f16(941, (V, Cw), 1.0), dd.normal_f16(942, (T, Cw), 0.5)
    want = (tok[ids].astype(np.float32) + pos[None].astype(np.float32)).astype(np.float16)
    g = Guarded(want, torch.float16)
    call(C, c, ids=_dev(ids), tok_f16=_dev(tok), pos_f16=_dev(pos), out_f16=g.out)
    g.check(f"embed_tokens_f16 {data}")


# --------------------------------------------------------------------------------------------- csrc/sampler.hip
@pytest.mark.parametrize("c", **gc.by_test("test_normals_from_bits"))
def test_normals_from_bits(C, c):
    n = c["args"]["n_quads"]
    assert n == c["items"] == CAP8 + 37
    k = np.arange(4 * n, dtype=np.uint64)
    words = ((k * np.uint64(2654435761) + (k >> np.uint64(3)) * np.uint64(40503)) & np.uint64(0xffffffff)).astype(np.uint32)
    words = words.reshape(n, 4)
    want = G.normals_from_bits(words)
    assert want.dtype == np.float32 and np.isfinite(want).all()
    g = Guarded(want, torch.float32)
    call(C, c, r=_dev(words.view(np.int32)), z=g.out)
    g.check("rng_normals_from_bits")
