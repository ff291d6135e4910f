"""GPU tests of the short-key form of the FP16 attention core at SD 1.5's head widths (attn_hd_short_kernel: form 1,
tkv <= 128, every key and value of a head staged once).

It runs attn_hd_kernel's per-wave arithmetic in attn_hd_kernel's order, so `_cfg=1` must be accepted, equal `_cfg=2`
and `_cfg=4` bit for bit (FP16, A8 and A4 outputs), give a batch row the bits of its single run, and lie within the
float64 oracle's tolerance of tests/test_attention_hd_gpu.py (its ATOL / RTOL, imported, not restated).  More than 128
keys with a forced form 1 are refused, and the A/B switch MIXDQ_ATTN_HD_SHORT=0 changes no bit.
"""
import numpy as np
import pytest
import torch

from tests import detdata as dd
from tests.test_attention_hd_gpu import ATOL, RTOL, S_INV, WIDTHS, ZP, scal, t

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

TKV = (1, 64, 77, 128)
TQ = (100, 256, 1024)
HEADS = 3


def make(seed, B, tq, tkv, C, packed):
    """Host q / k / v and device views: contiguous tensors, or -- `packed` -- column slices of the projections'
    packed outputs (q out of a [B, Tq, 3C] q|k|v-shaped buffer, k | v out of one [B, Tkv, 2C] buffer)."""
    if packed:
        qb = dd.normal_f16(seed, (B, tq, 3 * C), 1.2)
        kv = dd.normal_f16(seed + 1, (B, tkv, 2 * C), 1.2)
        qd, kvd = t(qb), t(kv)
        return (qb[..., C:2 * C], kv[..., :C], kv[..., C:]), (qd[..., C:2 * C], kvd[..., :C], kvd[..., C:])
    q, k, v = (dd.normal_f16(seed + i, (B, n, C), 1.2) for i, n in enumerate((tq, tkv, tkv)))
    return (q, k, v), (t(q), t(k), t(v))


CASES = [(D, tkv, tq, B, packed) for D in WIDTHS for tkv in TKV for tq in TQ for B in (1, 3)
         for packed in (False, True)]


def _id(c):
    return f"d{c[0]}_k{c[1]}_q{c[2]}_b{c[3]}_{'packed' if c[4] else 'contig'}"


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_short_form_is_accepted_and_equals_every_other_form(C, oracle, case):
    D, tkv, tq, B, packed = case
    Cc = HEADS * D
    (q, k, v), (qd, kd, vd) = make(700 + D + tkv, B, tq, tkv, Cc, packed)
    s, z = scal(S_INV), scal(ZP)
    got = C.attention_f16(qd, kd, vd, HEADS, _cfg=1)              # (raises without the short-key form)
    assert got.shape == (B, tq, Cc) and got.dtype == torch.float16 and got.is_contiguous()
    # the float64 oracle, at the tolerance of tests/test_attention_hd_gpu.py
    _, ref64 = oracle.attention_f16(q, k, v, HEADS)
    g = got.cpu().numpy().astype(np.float64)
    assert np.isfinite(g).all()
    err = np.abs(g - ref64)
    print(f"{_id(case)}: max err {err.max():.3e}")
    assert (err <= ATOL + RTOL * np.abs(ref64)).all(), f"max err {err.max():.3e}"
    if tkv == 1:
        assert torch.equal(got, vd.expand(B, tq, Cc).contiguous())
    # every form and the automatic choice: the same bits, FP16 / A8 / A4 outputs
    o8 = C.attention_f16(qd, kd, vd, HEADS, s, z, _cfg=1)
    o4 = C.attention_f16(qd, kd, vd, HEADS, s, z, _cfg=1, _abits=4)
    assert torch.equal(o8, C.quantize_per_tensor_to_int8(got, s, z))
    assert torch.equal(o4, o8.clamp(max=-113)) and (o8 != o8.flatten()[0]).any()
    for cfg in (0, 2, 4):
        assert torch.equal(C.attention_f16(qd, kd, vd, HEADS, _cfg=cfg).view(torch.int16), got.view(torch.int16)), cfg
        assert torch.equal(C.attention_f16(qd, kd, vd, HEADS, s, z, _cfg=cfg), o8), cfg
        assert torch.equal(C.attention_f16(qd, kd, vd, HEADS, s, z, _cfg=cfg, _abits=4), o4), cfg
    # a batch row equals its single run
    if B > 1:
        for b in range(B):
            one = C.attention_f16(qd[b:b + 1], kd[b:b + 1], vd[b:b + 1], HEADS, _cfg=1)
            assert torch.equal(one[0].view(torch.int16), got[b].view(torch.int16)), b
            one8 = C.attention_f16(qd[b:b + 1], kd[b:b + 1], vd[b:b + 1], HEADS, s, z, _cfg=1)
            assert torch.equal(one8[0], o8[b]), b


@pytest.mark.parametrize("D", WIDTHS)
def test_short_form_refuses_more_than_128_keys(C, D):
    Cc = 2 * D
    _, (qd, kd, vd) = make(50, 1, 64, 129, Cc, False)
    with pytest.raises(RuntimeError):
        C.attention_f16(qd, kd, vd, 2, _cfg=1)
    ok = C.attention_f16(qd, kd, vd, 2)                            # the automatic choice: the tiled kernel
    assert torch.equal(ok, C.attention_f16(qd, kd, vd, 2, _cfg=2))
    assert torch.isfinite(C.attention_f16(qd, kd[:, :128], vd[:, :128], 2, _cfg=1)).all()


def test_short_form_switch_off_gives_the_same_bits(C):
    """MIXDQ_ATTN_HD_SHORT=0 (read once per process: child processes) routes the automatic choice to the tiled
    kernel; the bits are those of the default routing."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    shapes = [(D, B, tq, tkv) for D in WIDTHS for B, tq, tkv in ((2, 1024, 77), (1, 100, 128), (3, 256, 1))]
    code = r'''
import sys, hashlib, torch
sys.path.insert(0, %r)
import mixdq_amd._C as C
from tests import detdata as dd
out = []
for D, B, tq, tkv in %r:
    Cc = 8 * D
    q = torch.from_numpy(dd.normal_f16(911, (B, tq, Cc), 1.0)).cuda()
    kv = torch.from_numpy(dd.normal_f16(912, (B, tkv, 2 * Cc), 1.0)).cuda()
    s, z = torch.tensor(30.0, device="cuda"), torch.tensor(2.0, device="cuda")
    for quant in (False, True):
        o = C.attention_f16(q, kv[..., :Cc], kv[..., Cc:], 8, *((s, z) if quant else ()))
        out.append(hashlib.sha256(o.cpu().numpy().tobytes()).hexdigest())
print("HASHES " + " ".join(out))
''' % (root, shapes)
    got = {}
    for flag in ("1", "0"):
        r = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(os.environ, MIXDQ_ATTN_HD_SHORT=flag),
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:]
        got[flag] = [ln for ln in r.stdout.splitlines() if ln.startswith("HASHES ")][-1]
    assert got["1"] == got["0"] and len(got["1"].split()) == 1 + 2 * len(shapes)
