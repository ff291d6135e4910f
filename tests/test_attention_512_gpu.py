"""GPU tests of mixdq_attention_f16 at head width 512 (csrc/attention.hip attn_512_kernel): the VAE decoder's single
mid-block head, q / k / v read as column slices of one [B, T, 1536] projection.

Tolerance: that of the other widths (tests/test_attention_gpu.py) against the float64 restatement
oracle.attention_f16, |got - ref| <= 2e-3 + 4e-3 * |ref|.  Exact-result inputs pin the column map (a slice of D per
wave) and the key-tile bookkeeping; a row of a batch must equal the image alone bit for bit.
"""
import numpy as np
import pytest
import torch

from tests import detdata as dd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ATOL, RTOL = 2e-3, 4e-3
D = 512


def bits(t):
    return t.contiguous().view(torch.int16)


def qkv_slices(qkv):
    return qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]


SHAPES = [(1, 100, 100), (2, 256, 256), (1, 32, 32), (1, 33, 33), (1, 96, 200)]   # B, tq, tkv


@pytest.mark.parametrize("B,tq,tkv", SHAPES, ids=[f"b{b}_q{q}_k{k}" for b, q, k in SHAPES])
def test_attention_512_vs_float64_oracle(C, oracle, B, tq, tkv):
    """Unit-normal q / k / v, the default scale 512 ** -0.5, one head; tq == tkv: the three are column slices of one
    [B, T, 1536] tensor (row stride 1536); the cross shape reads q from its own tensor and k | v from a [B, tkv, 1024]
    one."""
    if tq == tkv:
        host = dd.normal_f16(5120 + tq, (B, tq, 3 * D), 1.0)
        hq, hk, hv = qkv_slices(host)
        q, k, v = qkv_slices(torch.from_numpy(host).to(DEV))
    else:
        hq = dd.normal_f16(5121, (B, tq, D), 1.0)
        hkv = dd.normal_f16(5122, (B, tkv, 2 * D), 1.0)
        hk, hv = hkv[..., :D], hkv[..., D:]
        q, kv = torch.from_numpy(hq).to(DEV), torch.from_numpy(hkv).to(DEV)
        k, v = kv[..., :D], kv[..., D:]
    _, ref = oracle.attention_f16(hq, hk, hv, 1)
    out = C.attention_f16(q, k, v, 1)
    assert out.dtype == torch.float16 and tuple(out.shape) == (B, tq, D)
    got = out.cpu().numpy().astype(np.float64)
    err = np.abs(got - ref)
    print(f"attention 512 B{B} tq{tq} tkv{tkv}: max |err| {err.max():.3e}, max err / tol {(err / (ATOL + RTOL * np.abs(ref))).max():.3f}")
    assert np.isfinite(got).all()
    assert (err <= ATOL + RTOL * np.abs(ref)).all()
    assert torch.equal(bits(out), bits(C.attention_f16(q, k, v, 1)))          # deterministic


@pytest.mark.parametrize("tq", [40, 128])
def test_attention_512_uniform_probabilities_give_the_column_means_exactly(C, tq):
    """k = 0: every score is 0 and P is uniform over the 128 keys (four key tiles); with v[j, d] = j % 4 + d % 8 the
    output must EQUAL 1.5 + d % 8 in every one of the 512 columns -- a wave that read another wave's column slice, or a
    transposed read that permuted columns, shows."""
    tkv = 128
    g = torch.Generator(device="cpu").manual_seed(31)
    q = torch.randn(1, tq, D, generator=g).half().to(DEV)
    k = torch.zeros(1, tkv, D, dtype=torch.float16, device=DEV)
    j = torch.arange(tkv).view(tkv, 1)
    d = torch.arange(D).view(1, D)
    v = ((j % 4) + (d % 8)).to(torch.float16).view(1, tkv, D).to(DEV)
    out = C.attention_f16(q, k, v, 1)
    want = (1.5 + (d % 8).float()).half().expand(tq, D).to(DEV)
    assert torch.equal(out[0], want)


@pytest.mark.parametrize("T", [64, 77])
def test_attention_512_one_hot_scores_return_the_value_row_bit_for_bit(C, T):
    """q[i] and k[j] are 32 * unit vectors along column (7 i + 3) % 512 resp. (7 j + 3) % 512: score(i, i) = 1024 *
    512 ** -0.5 = 45.3, every other score 0 -- a gap above 30, so every other probability rounds to FP16 zero and
    out[i] is v[i], whatever tile key i sits in.  (v has no zeros: a zero would leave the sign of an underflowed
    remainder.)"""
    col = (7 * torch.arange(T) + 3) % D
    q = torch.zeros(1, T, D, dtype=torch.float16)
    q[0, torch.arange(T), col] = 32.0
    g = torch.Generator(device="cpu").manual_seed(32)
    mag = torch.randint(1, 33, (1, T, D), generator=g).float() / 8
    sign = torch.randint(0, 2, (1, T, D), generator=g).float() * 2 - 1
    v = (mag * sign).half()
    qd, vd = q.to(DEV), v.to(DEV)
    out = C.attention_f16(qd, qd.clone(), vd, 1)
    assert torch.equal(bits(out), bits(vd))


def test_attention_512_batch_row_equals_the_image_alone(C):
    """One launch geometry (32 query rows per workgroup), whatever the batch: row 1 of a batch of 2 has the bits the
    same image has alone."""
    host = dd.normal_f16(5130, (2, 100, 3 * D), 1.0)
    dev = torch.from_numpy(host).to(DEV)
    both = C.attention_f16(*qkv_slices(dev), 1)
    alone = C.attention_f16(*qkv_slices(dev[1:2].contiguous()), 1)
    assert torch.equal(bits(both[1:2]), bits(alone))


def test_attention_512_two_heads_read_their_own_columns(C, oracle):
    """`heads` may be any count: head h is the 512-column slice h * 512 .. of each row."""
    B, T = 1, 48
    hq = dd.normal_f16(5140, (B, T, 2 * D), 1.0)
    hkv = dd.normal_f16(5141, (B, T, 4 * D), 1.0)
    _, ref = oracle.attention_f16(hq, hkv[..., :2 * D], hkv[..., 2 * D:], 2)
    kv = torch.from_numpy(hkv).to(DEV)
    out = C.attention_f16(torch.from_numpy(hq).to(DEV), kv[..., :2 * D], kv[..., 2 * D:], 2)
    err = np.abs(out.cpu().numpy().astype(np.float64) - ref)
    assert (err <= ATOL + RTOL * np.abs(ref)).all()


def test_attention_512_refuses_the_int8_output_and_forced_forms(C):
    """FP16 output only at this width: with an output quantizer the library answers MIXDQ_ERR_SHAPE (9) and writes
    nothing; 512 is listed among the widths, 32 still is not."""
    assert 512 in C.ATTENTION_HEAD_DIMS and 32 not in C.ATTENTION_HEAD_DIMS
    x = torch.from_numpy(dd.normal_f16(5150, (1, 64, 3 * D), 1.0)).to(DEV)
    q, k, v = qkv_slices(x)
    s, z = torch.tensor(30.0, device=DEV), torch.tensor(2.0, device=DEV)
    with pytest.raises(RuntimeError, match="shape outside"):
        C.attention_f16(q, k, v, 1, s, z)
    out = torch.full((1, 64, D), 77, dtype=torch.int8, device=DEV)
    code = C._lib.mixdq_attention_f16(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), 1, 1, D, 64, 64,
                                      q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1),
                                      out.stride(0), out.stride(1), D ** -0.5, s.data_ptr(), z.data_ptr(), 0, None)
    torch.cuda.synchronize()
    assert code == 9 and bool((out == 77).all())
    for cfg in (1, 2, 4):                                  # one form at this width
        with pytest.raises(RuntimeError, match="shape outside"):
            C.attention_f16(q, k, v, 1, _cfg=cfg)
