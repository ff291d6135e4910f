"""GPU tests of mixdq_attention_f16 at head width 512 (csrc/attention.hip attn_512_kernel): the VAE decoder's single
mid-block head, q / k / v read as column slices of one [B, T, 1536] projection.

Tolerance: that of the other widths (tests/test_attention_gpu.py) against the float64 restatement
oracle.attention_f16, |got - ref| <= 2e-3 + 4e-3 * |ref|.  Exact-result inputs pin the column map (a slice of D per
wave) and the key-tile bookkeeping; a row of a batch must equal the image alone bit for bit.

The launch forms only a full-size decode takes (16,384 tokens: 512 key tiles, 512 workgroups an image) are reached by
small shapes further down: more workgroups than CUs in a count that is no multiple of 8 (tq = 8229 over 40 keys), 513
key tiles with a ragged last one (tkv = 16391 / 16388 under 40 queries), all by exact-result inputs -- at that length the
tolerance above cannot see a dropped tile (unit-normal data: an output over 16k keys is about 0.008) -- and one
unit-normal self-attention of 2080 tokens on a sample of rows.
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


def _no_zero_values(shape, seed):
    """FP16 values k / 8, k = 1..32, of either sign (a zero would leave the sign of an underflowed remainder)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    mag = torch.randint(1, 33, shape, generator=g).float() / 8
    sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    return (mag * sign).half()


SENTINEL = 0x7bcd          # the bits of FP16 63904: no output of these tests


def _launch_into_sentinel(C, q, k, v):
    """mixdq_attention_f16 (one head of 512) into an output pre-filled with SENTINEL, with a guard row behind it."""
    B, tq, tkv = q.shape[0], q.shape[1], k.shape[1]
    buf = torch.full((B * tq + 1, D), SENTINEL, dtype=torch.int16, device=DEV)
    out = buf[:B * tq].view(B, tq, D)
    code = C._lib.mixdq_attention_f16(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, 1, D, tq, tkv,
                                      q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1),
                                      out.stride(0), out.stride(1), D ** -0.5, None, None, C.FLAGS, C._stream())
    torch.cuda.synchronize()
    assert code == 0
    assert bool((buf[B * tq] == SENTINEL).all())                       # nothing written past the last row
    return out


@pytest.mark.parametrize("B", [1, 2])
def test_attention_512_more_workgroups_than_cus_return_their_value_rows(C, B):
    """tq = 8229 over 40 keys: 258 query blocks an image (516 at B = 2) -- more workgroups than the 256 CUs, a count
    that is no multiple of 8 (258 = 8 x 32 + 2, 516 = 8 x 64 + 4: attn_block_of's remainder branch), the last block
    with 5 of its 32 rows.  q[i] = 32 e_col(i % 40), k[j] = 32 e_col(j), col(j) = (7 j + 3) % 512: row i scores
    1024 x 512 ** -0.5 = 45.25 on key i % 40 and 0 elsewhere, so out[b, i] must EQUAL v[b, i % 40] bit for bit (the
    one-hot test's gap; v without zeros, other values per image).

    What it would catch.  A workgroup map that is not a bijection onto (batch, query block) leaves rows unwritten --
    they keep the sentinel the output is filled with -- e.g. the identity on a grid dealt in 8 runs without the
    remainder (bid -> (bid % 8) * (258 / 8) + bid / 8) computes blocks 32 and 64 twice and blocks 256, 257 never.  A map
    that sends a workgroup to the other image returns the other image's value rows.  The keys span two tiles (32 + 8):
    with ntiles lowered by one, keys 32..39 are never read and the rows with i % 40 >= 32 come out as the mean of
    v[0..31].  A ragged last block that wrote all of its 32 rows overwrites the next image (B = 2) or the guard row."""
    tq, tkv = 8229, 40
    assert (tq + 31) // 32 == 258 and (B * 258) % 8 != 0 and tq % 32 == 5
    col = (7 * torch.arange(tkv) + 3) % D
    assert len(set(col.tolist())) == tkv
    k = torch.zeros(B, tkv, D, dtype=torch.float16)
    k[:, torch.arange(tkv), col] = 32.0
    q = k[:, torch.arange(tq) % tkv].contiguous()
    v = _no_zero_values((B, tkv, D), 33)
    assert not torch.equal(v[0], v[-1]) or B == 1
    out = _launch_into_sentinel(C, q.to(DEV), k.to(DEV), v.to(DEV))
    want = bits(v[:, torch.arange(tq) % tkv])
    got = out.cpu()
    unwritten = (got == SENTINEL).all(dim=2)
    assert not bool(unwritten.any()), f"{int(unwritten.sum())} rows were never written, first {unwritten.nonzero()[0].tolist()}"
    wrong = (got != want).any(dim=2)
    assert not bool(wrong.any()), f"{int(wrong.sum())} rows differ, first {wrong.nonzero()[0].tolist()}"


def _late_targets(tkv):
    """Forty key positions: the first and last key of tiles 0, 1, 510, 511 and of the ragged tile 512, a middle tile,
    and seeded others."""
    fixed = [0, 31, 32, 63, 8192 + 5, 8192 + 31, 16320, 16351, 16352, 16383, 16384, tkv - 1]
    rng = np.random.default_rng(34)
    rest = [int(x) for x in rng.permutation(tkv) if int(x) not in fixed][:40 - len(fixed)]
    pos = fixed + rest
    assert len(pos) == 40 == len(set(pos)) and max(pos) == tkv - 1
    return torch.tensor(pos)


def test_attention_512_one_key_among_16391_returns_its_value_row(C, oracle):
    """tkv = 16391: 513 key tiles (the decoder's 512 at 1024 px, and a ragged one of 7 keys), 40 queries.  Query i and
    its target key are 32 e_c(i) (40 distinct columns); EVERY OTHER KEY IS ZERO: row i scores 45.25 on its target and 0
    on the 16390 others, whose probabilities e^-45.25 round to FP16 zero.  out[i] must EQUAL v[target_i] bit for bit
    (the float64 restatement, whose weight away from the target is below 16390 e^-45 = 4e-16, is asserted to round to
    exactly that: the expectation does not lean on the kernel).

    Until its target's tile a row's running maximum is 0 and its accumulators fill with the plain sum of every v seen
    (P = 1); the target then raises the maximum and `alpha = exp2(-45.25 log2 e)` must wipe them; after it hundreds of
    tiles contribute P = 0.  Targets sit on the first and last key of tiles 0, 1, 510, 511, in a middle tile and on the
    first and last key (16390) of the ragged tile.  What it would catch: with ntiles lowered by one the row whose target
    is key 16384 or 16390 never meets it and returns the mean of all v; a stage of the two-stage K | V pipeline that
    lagged or led by a tile pairs a target's score with another tile's V rows; a rescale skipped or applied to part of
    the accumulators leaves sums of hundreds of v rows in the result; a ragged-tile mask off by one drops key 16390 or
    admits a re-read copy of it (P = 1 twice: still v -- but the mask's other side is pinned by the uniform test)."""
    tq, tkv = 40, 16391
    assert (tkv + 31) // 32 == 513 and tkv % 32 == 7
    target = _late_targets(tkv)
    col = (7 * torch.arange(tq) + 3) % D
    q = torch.zeros(1, tq, D, dtype=torch.float16)
    q[0, torch.arange(tq), col] = 32.0
    kv = torch.zeros(1, tkv, 2 * D, dtype=torch.float16)                # k | v, as a fused projection leaves them
    kv[0, target, :D] = q[0]
    kv[0, :, D:] = _no_zero_values((tkv, D), 35)
    want = kv[:, target, D:]
    ref16, _ = oracle.attention_f16(q.numpy(), kv[..., :D].numpy(), kv[..., D:].numpy(), 1)
    assert np.array_equal(ref16.view(np.uint16), want.contiguous().numpy().view(np.uint16))
    kvd = kv.to(DEV)
    out = _launch_into_sentinel(C, q.to(DEV), kvd[..., :D], kvd[..., D:]).cpu()
    wrong = (out != bits(want)).any(dim=2)[0]
    assert not bool(wrong.any()), f"rows {wrong.nonzero().view(-1).tolist()} (targets {target[wrong].tolist()}) differ"


def test_attention_512_uniform_probabilities_over_16388_keys(C):
    """k = 0 over 16388 keys (513 tiles, 4 keys in the last): P is uniform, and with v[j, d] = j % 4 + d % 8 every
    column must EQUAL 1.5 + d % 8.  Exact: every P is FP16 1; the column sums are integers below 2^24 and the row sum
    is 16388, all exact in FP32; their product with the rounded 1 / 16388 lies within 2^-24 (relative) of 1.5 + d % 8,
    a multiple of 0.5 below 16, and rounds to it in FP16.  This pins the row sum and the accumulators over 513 tiles
    (a tile counted twice or dropped in `lsum` alone moves every column by 2e-3, two FP16 ulps at 1.5) and the ragged
    mask from the side the one-key test cannot see: the 28 absent keys of the last tile re-read key 16387 (j % 4 = 3),
    and one of them admitted shifts every mean upwards.  (It cannot see the LAST tile dropped whole: its four keys
    carry j % 4 = 0..3, the mean of the first 16384 is the same -- the one-key test's targets 16384 and 16390 do.)"""
    tq, tkv = 40, 16388
    assert tkv % 4 == 0 and tkv % 32 == 4 and (tkv + 31) // 32 == 513
    g = torch.Generator(device="cpu").manual_seed(36)
    q = torch.randn(1, tq, D, generator=g).half().to(DEV)
    k = torch.zeros(1, tkv, D, dtype=torch.float16, device=DEV)
    j = torch.arange(tkv).view(tkv, 1)
    d = torch.arange(D).view(1, D)
    v = ((j % 4) + (d % 8)).to(torch.float16).view(1, tkv, D).to(DEV)
    out = _launch_into_sentinel(C, q, k, v).view(torch.float16)
    want = (1.5 + (d % 8).float()).half().expand(tq, D).to(DEV)
    assert torch.equal(out[0], want), f"{int((out[0] != want).sum())} values differ, first {out[0][out[0] != want][:4].tolist()}"


def test_attention_512_self_attention_of_2080_tokens_on_a_sample_of_rows(C, oracle):
    """(B, T) = (2, 2080) in the fused [B, T, 1536] layout, unit-normal: 65 query blocks and 65 key tiles an image.  A
    seeded sample of 64 query rows per image, rows 0 and T - 1 among them, against the float64 restatement at this
    file's bound (the restatement gets those rows' q and the full k, v: an attention row depends on its own q row
    only); and the batch row must equal the image alone, bit for bit."""
    B, T = 2, 2080
    host = dd.normal_f16(5160, (B, T, 3 * D), 1.0)
    dev = torch.from_numpy(host).to(DEV)
    out = C.attention_f16(*qkv_slices(dev), 1)
    assert tuple(out.shape) == (B, T, D) and bool(torch.isfinite(out).all())
    got = out.cpu().numpy().astype(np.float64)
    hq, hk, hv = qkv_slices(host)
    worst = 0.0
    for b in range(B):
        rng = np.random.default_rng(5161 + b)
        rows = np.unique(np.concatenate([[0, T - 1], rng.choice(np.arange(1, T - 1), 62, replace=False)]))
        assert len(rows) == 64
        _, ref = oracle.attention_f16(hq[b:b + 1, rows], hk[b:b + 1], hv[b:b + 1], 1)
        err = np.abs(got[b, rows] - ref[0])
        ratio = (err / (ATOL + RTOL * np.abs(ref[0]))).max()
        worst = max(worst, ratio)
        print(f"attention 512 B{B} T{T} image {b}: max |ref| {np.abs(ref).max():.3e}, max |err| {err.max():.3e}, max err / tol {ratio:.3f}")
        assert (err <= ATOL + RTOL * np.abs(ref[0])).all(), (b, ratio)
    for b in range(B):
        alone = C.attention_f16(*qkv_slices(dev[b:b + 1].contiguous()), 1)
        assert torch.equal(bits(out[b:b + 1]), bits(alone)), b


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
