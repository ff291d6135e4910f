"""GPU tests of MIXDQ_FLAG_CAUSAL on mixdq_attention_f16 (the short-key kernel's causal instantiation: a text
encoder's self-attention, head width 64, tq == tkv <= 128).

Exact-result inputs pin WHICH keys a row admits (a tolerance cannot tell key i from key i + 1 of random data):
  diagonal selection  q rows (256, 0, ...), k[j] = (j, 0, ...), scale 0.125: score(i, j) = 32 j.  Causally the admitted
                      maximum is key i and every other admitted key lies >= 32 below it -- exp(-32) < 2^-46 rounds to
                      FP16 zero (smallest subnormal 2^-24) -- so P is one-hot, lsum == 1 and the output is v, bit for bit.
                      An admitted future key turns row i into a later row of v; a masked diagonal into v[i - 1] (NaN
                      at row 0).  Without the flag every row is v[T - 1]: the inputs discriminate.
  prefix mean         q = 0: every admitted key weighs exp2(0) = 1 (exactly 1 in FP16), v constant per column: the
                      output is (n c) / n over the n = i + 1 admitted keys -- c exactly (n c is exact in FP32 for an
                      FP16 c and n <= 128; the product with the rounded 1 / n is within half an FP16 ulp of c).
Random data is held to the bound of tests/test_attention_gpu.py, |err| <= 2e-3 + 4e-3 |ref|, against a float64
restatement with an explicit mask.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import detdata as dd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ATOL, RTOL = 2e-3, 4e-3
T_EDGES = (1, 2, 31, 32, 33, 63, 64, 65, 77, 127, 128)      # wave (32 rows), tile (64 keys) and ragged edges


def bits(x):
    return x.contiguous().view(torch.int16)


def diag_inputs(B, T, heads, fused_layout, seed=3):
    """q / k / v [B, T, 64 heads] of the diagonal-selection case, dense or as column slices of one [B, T, 3C]."""
    C = 64 * heads
    q = torch.zeros(B, T, C, dtype=torch.float16)
    k = torch.zeros(B, T, C, dtype=torch.float16)
    q[..., ::64] = 256.0
    k[..., ::64] = torch.arange(T, dtype=torch.float16).view(1, T, 1)
    v = torch.from_numpy(dd.normal_f16(seed, (B, T, C), 1.0))
    if fused_layout:
        buf = torch.cat([q, k, v], dim=-1).to(DEV)
        return buf[..., :C], buf[..., C:2 * C], buf[..., 2 * C:]
    return q.to(DEV), k.to(DEV), v.to(DEV)


@pytest.mark.parametrize("fused_layout", (False, True))
@pytest.mark.parametrize("heads", (1, 3))
def test_causal_diagonal_selection_exact(C, heads, fused_layout):
    for T in T_EDGES:
        q, k, v = diag_inputs(2, T, heads, fused_layout)
        out = C.attention_f16(q, k, v, heads, _causal=True)
        assert torch.equal(bits(out), bits(v)), (T, heads, fused_layout)
        assert torch.equal(bits(C.attention_f16(q, k, v, heads, _causal=True, _cfg=1)), bits(v)), T
        plain = C.attention_f16(q, k, v, heads)                     # no flag: every row selects the last key
        assert torch.equal(bits(plain), bits(v[:, T - 1:T].expand_as(v))), (T, "unmasked")


@pytest.mark.parametrize("heads", (1, 3))
def test_causal_prefix_mean_exact(C, heads):
    for T in T_EDGES:
        Cw = 64 * heads
        q = torch.zeros(2, T, Cw, dtype=torch.float16, device=DEV)
        k = torch.from_numpy(dd.normal_f16(5, (2, T, Cw), 1.0)).to(DEV)
        col = torch.from_numpy(dd.normal_f16(6, (2, 1, Cw), 1.5)).to(DEV)
        v = col.expand(2, T, Cw).contiguous()
        out = C.attention_f16(q, k, v, heads, _causal=True)
        assert torch.equal(bits(out), bits(v)), T


def causal_ref(q, k, v, heads):
    """float64, explicit mask: out[b, i] = softmax_{j <= i}(q_i . k_j / 8) v_j per head."""
    q, k, v = (np.asarray(a, np.float16).astype(np.float64) for a in (q, k, v))
    B, T, Cw = q.shape
    sp = lambda a: a.reshape(B, T, heads, 64).transpose(0, 2, 1, 3)
    s = np.einsum("bhqd,bhkd->bhqk", sp(q), sp(k)) * 0.125
    s = np.where(np.tril(np.ones((T, T), bool)), s, -np.inf)
    s -= s.max(axis=-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(axis=-1, keepdims=True)
    return np.einsum("bhqk,bhkd->bhqd", p, sp(v)).transpose(0, 2, 1, 3).reshape(B, T, Cw)


@pytest.mark.parametrize("heads", (12, 20))
@pytest.mark.parametrize("T", (77, 128, 20))
def test_causal_random_vs_float64(C, T, heads):
    Cw = 64 * heads
    qkv = dd.normal_f16(40 + T, (2, T, 3 * Cw), 1.0)
    d = torch.from_numpy(qkv).to(DEV)
    out = C.attention_f16(d[..., :Cw], d[..., Cw:2 * Cw], d[..., 2 * Cw:], heads, _causal=True)
    ref = causal_ref(qkv[..., :Cw], qkv[..., Cw:2 * Cw], qkv[..., 2 * Cw:], heads)
    err = np.abs(out.cpu().numpy().astype(np.float64) - ref)
    print(f"causal T={T} heads={heads}: max err {err.max():.3e}")
    assert (err <= ATOL + RTOL * np.abs(ref)).all(), err.max()
    # a batch row equals the sequence alone, bit for bit
    for b in range(2):
        alone = C.attention_f16(d[b:b + 1, :, :Cw], d[b:b + 1, :, Cw:2 * Cw], d[b:b + 1, :, 2 * Cw:], heads, _causal=True)
        assert torch.equal(bits(alone), bits(out[b:b + 1])), b


def _raw_launch(C, q, k, v, out, heads, D, flags, s_inv=None, zp=None):
    B, Tq, _ = q.shape
    return C._lib.mixdq_attention_f16(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, heads, D, Tq, k.shape[1],
        q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1), out.stride(0), out.stride(1),
        ctypes.c_float(D ** -0.5), None if s_inv is None else s_inv.data_ptr(), None if zp is None else zp.data_ptr(),
        flags, torch.cuda.current_stream().cuda_stream)


def test_causal_refusals_write_nothing(C):
    ERR_SHAPE = 9
    mk = lambda T, Cw: torch.from_numpy(dd.normal_f16(7, (1, T, Cw), 1.0)).to(DEV)
    one = lambda val: torch.tensor(val, dtype=torch.float32, device=DEV)
    cases = dict(tq_ne_tkv=(mk(64, 64), mk(77, 64), 1, 64, None),
                 t129=(mk(129, 64), mk(129, 64), 1, 64, None),
                 width40=(mk(77, 80), mk(77, 80), 2, 40, None),
                 quantizer=(mk(77, 64), mk(77, 64), 1, 64, (one(20.0), one(1.0))))
    for name, (q, kv, heads, D, qp) in cases.items():
        out = torch.full(q.shape, -2.5, dtype=torch.float16, device=DEV)
        want = out.clone()
        code = _raw_launch(C, q, kv, kv, out, heads, D, C.FLAG_CAUSAL, *(qp or ()))
        torch.cuda.synchronize()
        assert code == ERR_SHAPE, (name, code)
        assert torch.equal(bits(out), bits(want)), name
    q = mk(77, 64)                                                   # a forced tiled form with the flag
    out = torch.full(q.shape, -2.5, dtype=torch.float16, device=DEV)
    assert _raw_launch(C, q, q, q, out, 1, 64, C.FLAG_CAUSAL | (2 << 8)) == ERR_SHAPE
    torch.cuda.synchronize()
    assert bool((out == -2.5).all())
    with pytest.raises(RuntimeError):
        C.attention_f16(q, q, q, 1, one(20.0), one(1.0), _causal=True)
