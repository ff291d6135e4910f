"""GPU tests of the decoupled cross-attention launch (mixdq_attention_f16_ip, csrc/attention_ip.hip; IP-Adapter).

Every case is checked three ways: (a) the FP16 output against a float64 evaluation of
out = attn(q, K, V) + sum_j s_j attn(q, K_j, V_j) at the attention tests' ATOL / RTOL per term plus the two FP16 roundings
the specification adds (2^-11 relative each); (b) FP16 and INT8 outputs bit-equal to the chain the launch replaces --
`attention_f16` per key set, torch half operations, `quantize_per_tensor_to_int8`; (c) a zero scale skips its adapter
without reading it.  q, k | v and every adapter's k | v are column slices of packed tensors; batch 2, 2 heads.
"""
import numpy as np
import pytest
import torch

from tests import detdata as dd
from tests.test_attention_gpu import ATOL, RTOL, scal, t

pytestmark = pytest.mark.gpu
B, HEADS, CH = 2, 2, 128
S_INV, ZP = 23.0, 3.0

CASES = [  # tq (33: a ragged last wave; 160: a second workgroup), tkv, image tokens per adapter, scales
    (33, 77, (4,), (0.6,)), (160, 77, (16,), (1.0,)), (33, 1, (1,), (-0.5,)), (160, 128, (33,), (0.6,)),
    (33, 77, (64,), (1.0,)), (160, 77, (65,), (-0.5,)), (33, 128, (128,), (0.6,)), (160, 77, (4, 16), (0.6, -0.5)),
    (33, 1, (4, 4, 4, 4), (0.6, 1.0, -0.5, 1.0)), (160, 128, (4, 4, 4, 4), (1.0, 0.6, -0.5, 0.6)),
    (160, 1, (16,), (0.6,)), (33, 128, (4, 16), (1.0, 0.6)),
]


def make(seed, tq, tkv, tokens, ch=CH):
    """Host (q, k, v, [(k_j, v_j)]) and the same as device views of the packed tensors."""
    qp = dd.normal_f16(seed, (B, tq, 3 * ch), 1.2)
    sets = [dd.normal_f16(seed + 1 + i, (B, n, 2 * ch), 1.2) for i, n in enumerate((tkv,) + tuple(tokens))]
    cut = lambda kv: (kv[..., :ch], kv[..., ch:])
    host = (qp[..., ch:2 * ch],) + cut(sets[0]) + ([cut(s) for s in sets[1:]],)
    dev = (t(qp)[..., ch:2 * ch],) + cut(t(sets[0])) + ([cut(t(s)) for s in sets[1:]],)
    return host, dev


def chain(C, q, k, v, ip, scales, heads=HEADS):
    acc = C.attention_f16(q, k, v, heads)
    for (kj, vj), s in zip(ip, scales):
        acc = acc + float(np.float32(s)) * C.attention_f16(q, kj, vj, heads)
    return acc


def same(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("case", CASES, ids=[f"q{c[0]}_k{c[1]}_ip{'_'.join(map(str, c[2]))}" for c in CASES])
def test_one_launch_against_float64_the_chain_and_zero_scales(C, oracle, case):
    tq, tkv, tokens, scales = case
    assert C.attention_ip_supported(64, tkv, tokens)
    (q, k, v, ip), (qd, kd, vd, ipd) = make(4000 + tq + tkv + sum(tokens), tq, tkv, tokens)
    sd = torch.tensor(scales, dtype=torch.float32, device=qd.device)
    got = C.attention_ip(qd, kd, vd, ipd, sd, HEADS)
    assert got.shape == (B, tq, CH) and got.dtype == torch.float16
    # (a) float64
    s64 = [float(np.float32(s)) for s in scales]
    ref_t = oracle.attention_f16(q, k, v, HEADS)[1]
    ref_j = [oracle.attention_f16(q, kj, vj, HEADS)[1] for kj, vj in ip]
    ref = ref_t + sum(s * r for s, r in zip(s64, ref_j))
    tol = ((1 + sum(abs(s) for s in s64)) * ATOL + RTOL * (np.abs(ref_t) + sum(abs(s) * np.abs(r) for s, r in zip(s64, ref_j)))
           + 2.0 ** -11 * (sum(np.abs(s * r) for s, r in zip(s64, ref_j)) + np.abs(ref)))
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
    print(f"max err {err.max():.3e}, max err / tol {(err / tol).max():.3f}")
    assert (err <= tol).all()
    # (b) the chain of existing launches, FP16 and INT8
    want = chain(C, qd, kd, vd, ipd, scales)
    assert same(got, want)
    si, zp = scal(S_INV), scal(ZP)
    got8 = C.attention_ip(qd, kd, vd, ipd, sd, HEADS, si, zp)
    assert torch.equal(got8, C.quantize_per_tensor_to_int8(want, si, zp)) and (got8 != got8.flatten()[0]).any()
    assert torch.equal(C.attention_ip(qd, kd, vd, ipd, sd, HEADS, si, zp, _abits=4), got8.clamp(max=-113))
    # (c) a zero scale: the adapter's NaN keys and values are not read
    nan = [(torch.full_like(kj, float("nan")), torch.full_like(vj, float("nan"))) for kj, vj in ipd]
    s0 = sd.clone()
    s0[0] = -0.0
    one_off = C.attention_ip(qd, kd, vd, nan[:1] + ipd[1:], s0, HEADS)
    rest = C.attention_ip(qd, kd, vd, ipd[1:], sd[1:].clone(), HEADS) if len(ipd) > 1 else C.attention_f16(qd, kd, vd, HEADS)
    assert torch.isfinite(one_off).all() and same(one_off, rest)
    assert same(C.attention_ip(qd, kd, vd, nan, torch.zeros_like(sd), HEADS), C.attention_f16(qd, kd, vd, HEADS))


@pytest.mark.parametrize("ch,tkv,tokens", [(80, 77, (4,)), (128, 77, (33, 33, 4)), (128, 129, (4,))],
                         ids=["head_dim_40", "five_blocks", "tkv_129"])
def test_refused_shapes_run_the_chain(C, ch, tkv, tokens):
    assert not C.attention_ip_supported(ch // HEADS, tkv, tokens)
    _, (qd, kd, vd, ipd) = make(4500 + tkv, 33, tkv, tokens, ch)
    scales = (0.6, -0.5, 1.0)[:len(tokens)]
    sd = torch.tensor(scales, dtype=torch.float32, device=qd.device)
    want = chain(C, qd, kd, vd, ipd, scales)
    assert same(C.attention_ip(qd, kd, vd, ipd, sd, HEADS), want)
    si, zp = scal(S_INV), scal(ZP)
    assert torch.equal(C.attention_ip(qd, kd, vd, ipd, sd, HEADS, si, zp), C.quantize_per_tensor_to_int8(want, si, zp))
