"""GPU tests of the epilogue activation of mixdq_linear_f16 (MIXDQ_FLAG_ACT_GELU / MIXDQ_FLAG_ACT_QUICK_GELU).

Contract: with h = f16(acc + bias), the bits the unflagged launch stores, the flagged launch stores f16(act(f32(h))).
The activation is therefore a function of 16 bits, and the whole specification is two tables of 65 536 entries computed
on the host from include/mixdq_math.h through the oracle library: GELU from mixdq_oracle_geluf, quick-GELU restated
here in numpy float32 from mixdq_oracle_expf in the stated operation order.  Every comparison below is bit for bit
(NaN against NaN by NaN-ness).
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import detdata as dd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ACTS = ("gelu", "quick_gelu")
ERR_INVALID_ARG, ERR_UNSUPPORTED = 1, 3


@pytest.fixture(scope="module")
def spec(oracle):
    """act -> uint16[65536]: the bits of f16(act(f32(h))) for every FP16 bit pattern h."""
    L = oracle.lib()
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float32)
    with np.errstate(all="ignore"):
        gelu = np.array([L.mixdq_oracle_geluf(float(a)) for a in h], np.float32)
        t = np.float32(1.702) * h                                     # one rounded product,
        e = np.array([L.mixdq_oracle_expf(float(-a)) for a in t], np.float32)      # negated, one exp,
        quick = h / (np.float32(1.0) + e)                             # one rounded sum, a correctly rounded division
        assert quick.dtype == np.float32
        return dict(gelu=gelu.astype(np.float16).view(np.uint16), quick_gelu=quick.astype(np.float16).view(np.uint16))


def same_bits(got, want):
    got, want = np.asarray(got).view(np.uint16).ravel(), np.asarray(want).view(np.uint16).ravel()
    gn, wn = np.isnan(got.view(np.float16)), np.isnan(want.view(np.float16))
    return np.array_equal(gn, wn) and np.array_equal(got[~gn], want[~wn])


def mapped(table, h):
    return table[h.cpu().numpy().view(np.uint16).astype(np.int64)]


SHAPES = [(77, 512, 128), (77, 3072, 768), (154, 5120, 1280), (5, 12, 8)]       # M, N, K


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_fused_activation_is_the_activation_of_the_unfused_output(C, spec, act, M, N, K):
    x = torch.from_numpy(dd.normal_f16(1, (M, K), 1.0)).to(DEV)
    w = torch.from_numpy(dd.normal_f16(2, (N, K), 2.0 / np.sqrt(K))).to(DEV)       # h ~ N(0, 2): both GELU branches
    b = torch.from_numpy(dd.normal_f16(3, (N,), 0.5)).to(DEV)
    for cfg in (0,) + tuple(C.F16_CONFIGS):
        for bias in (b, None):
            h = C.linear_f16(x, w, bias, _cfg=cfg)
            got = C.linear_f16(x, w, bias, _cfg=cfg, _act=act)
            assert same_bits(got.cpu().numpy(), mapped(spec[act], h)), (cfg, bias is not None)


@pytest.mark.parametrize("act", ACTS)
def test_fused_activation_on_the_one_output_per_thread_kernel(C, spec, act):
    M, N, K = 37, 20, 12                                             # K % 8 != 0: no MFMA tile takes it
    x = torch.from_numpy(dd.normal_f16(4, (M, K), 1.0)).to(DEV)
    w = torch.from_numpy(dd.normal_f16(5, (N, K), 0.6)).to(DEV)
    b = torch.from_numpy(dd.normal_f16(6, (N,), 0.5)).to(DEV)
    h = C.linear_f16(x, w, b)
    assert same_bits(C.linear_f16(x, w, b, _act=act).cpu().numpy(), mapped(spec[act], h))


def test_gelu_epilogue_equals_the_device_gelu_table(C, spec):
    tab = C.gelu_table(DEV).cpu().numpy().view(np.uint16)             # [2, MAG]: sign, magnitude
    bits = np.arange(65536, dtype=np.uint32)
    near = (bits & 0x7fff) < C.GELU_TABLE_MAG
    assert np.array_equal(tab[bits[near] >> 15, bits[near] & 0x7fff], spec["gelu"][near])


@pytest.mark.parametrize("K", (8, 4))                                # the MFMA tiles; the one-output-per-thread kernel
@pytest.mark.parametrize("act", ACTS)
def test_every_fp16_input_of_the_activation(C, spec, act, K):
    """One launch per activation covers every value h can take: A[m] = (pattern m, 0, ...), W[n] = (1, 0, ...), no
    bias -- h[m, n] is pattern m exactly (0 * 0 products beside it; +-inf and NaN stay themselves).  The one exception
    is the pattern -0: an accumulator that starts at +0 and adds a -0 product holds +0, so h is +0 there -- as in any
    launch of this kernel family, which can never store a -0 that the activation would then see (a bias of -0 added to
    a +0 accumulator gives +0 as well).  The flagged launch is therefore compared with the specification AT THE BITS
    THE UNFLAGGED LAUNCH STORES, which is the contract, and those bits are required to be the 65 535 other patterns."""
    pat = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    a = np.zeros((65536, K), np.uint16)
    a[:, 0] = pat
    w = np.zeros((8, K), np.float16)
    w[:, 0] = 1.0
    A, W = torch.from_numpy(a.view(np.float16)).to(DEV), torch.from_numpy(w).to(DEV)
    h = C.linear_f16(A, W, None).cpu().numpy().view(np.uint16)
    finite = np.isfinite(pat.view(np.float16))
    expect_h = pat.copy()
    expect_h[0x8000] = 0                                             # -0 * 1 added to a +0 accumulator
    bad = np.nonzero(finite & (h != expect_h[:, None]).any(axis=1))[0]
    print(f"identity GEMM K={K}: {len(bad)} finite patterns not reproduced", [hex(int(b)) for b in bad[:8]])
    assert len(bad) == 0
    infs = np.isinf(pat.view(np.float16))
    assert np.array_equal(h[infs], np.repeat(pat[infs, None], 8, axis=1))
    assert np.isnan(h.view(np.float16)[~finite & ~infs]).all()
    got = C.linear_f16(A, W, None, _act=act).cpu().numpy().view(np.uint16)
    want = spec[act][h.astype(np.int64)]
    assert same_bits(got, want)                                      # finite bits, NaN -> NaN, +-inf as the specification
    assert np.isnan(got.view(np.float16)[~finite & ~infs]).all()


def test_activation_flag_refusals(C):
    x = torch.from_numpy(dd.normal_f16(7, (16, 64), 1.0)).to(DEV)
    w = torch.from_numpy(dd.normal_f16(8, (32, 64), 0.1)).to(DEV)
    res = torch.zeros(16, 32, dtype=torch.float16, device=DEV)
    out = torch.full((16, 32), -2.5, dtype=torch.float16, device=DEV)
    s = torch.cuda.current_stream().cuda_stream

    def raw(flags, residual=None):
        return C._lib.mixdq_linear_f16(x.data_ptr(), w.data_ptr(), None, out.data_ptr(), 16, 32, 64,
                                       None if residual is None else residual.data_ptr(), 1, flags, s)
    both = C.FLAG_ACT["gelu"] | C.FLAG_ACT["quick_gelu"]
    assert raw(both) == ERR_INVALID_ARG
    for act in ACTS:
        assert raw(C.FLAG_ACT[act], res) == ERR_INVALID_ARG
        with pytest.raises(RuntimeError):
            C.linear_f16(x, w, None, _residual=res, _act=act)
    with pytest.raises(RuntimeError):
        C.linear_f16(x, w, None, _act="silu")
    # any other entry point: unsupported
    q = torch.from_numpy(dd.normal_f16(9, (1, 16, 64), 1.0)).to(DEV)
    o3 = torch.full((1, 16, 64), -2.5, dtype=torch.float16, device=DEV)
    for act in ACTS:
        code = C._lib.mixdq_attention_f16(q.data_ptr(), q.data_ptr(), q.data_ptr(), o3.data_ptr(), 1, 1, 64, 16, 16,
                                          q.stride(0), q.stride(1), q.stride(0), q.stride(1), q.stride(0), q.stride(1),
                                          o3.stride(0), o3.stride(1), ctypes.c_float(0.125), None, None,
                                          C.FLAG_ACT[act], s)
        assert code == ERR_UNSUPPORTED
        xc = torch.zeros(1, 4, 4, 8, dtype=torch.float16, device=DEV)
        wc = torch.zeros(8, 1, 1, 8, dtype=torch.float16, device=DEV)
        oc = torch.full((1, 4, 4, 8), -2.5, dtype=torch.float16, device=DEV)
        code = C._lib.mixdq_conv2d_f16(xc.data_ptr(), wc.data_ptr(), None, oc.data_ptr(), 1, 4, 4, 8, 8, 1, 1, 1, 0,
                                       None, 1, C.FLAG_ACT[act], s)
        assert code == ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert bool((oc == -2.5).all()) and bool((o3 == -2.5).all())
    torch.cuda.synchronize()
    assert bool((out == -2.5).all())
