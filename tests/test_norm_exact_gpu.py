"""Exact-result inputs through the norm producers (tests/exact_inputs.py, norm section): GroupNorm on integer data
whose group sums are exact in any order, one heavy element moved through every edge of the launch geometry, against
the closed formula of the kernel's finalize tail -- a dropped, doubled or mis-grouped element changes an integer and
with it the bits; LayerNorm on zero-sum rows against its closed formula, the heavy element against the float64
reference; and the quantizers' ties and clamp ends through both producers."""
import numpy as np
import pytest
import torch

from tests import exact_inputs as ei
from tests import norm_edges as ne

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

GN_EXACT = [  # N, HW, C, G, silu, C1 (None: one source) -- one per geometry class of tests/norm_edges.py
    (2, 33, 64, 8, True, None), (1, 2080, 64, 8, False, None), (1, 16385, 64, 8, True, None),
    (1, 7, 320, 32, False, None), (2, 390, 320, 32, True, None), (1, 70, 32, 8, True, None),
    (1, 43, 96, 8, False, None), (1, 43, 96, 8, True, 8), (1, 43, 96, 8, False, 24), (1, 390, 320, 32, True, 168),
    (1, 3, 960, 32, True, None), (1, 130, 1920, 32, False, None), (1, 9, 1280, 32, True, None),
    (1, 1025, 1280, 32, False, None), (1, 65, 2560, 32, True, None), (1, 65, 8192, 32, False, None),
    (1, 5, 2048, 256, True, None),
]


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def scal(v):
    return torch.tensor(float(v), dtype=torch.float32, device=DEV)


def silu_spec(oracle, pre):
    """f16(silu(pre)) by the scalar specification (include/mixdq_math.h through the oracle library)."""
    L = oracle.lib()
    bits, inv = np.unique(pre.view(np.uint16), return_inverse=True)
    with np.errstate(all="ignore"):
        tab = np.array([L.mixdq_oracle_siluf(float(v)) for v in bits.view(np.float16).astype(np.float32)],
                       np.float32).astype(np.float16)
    return tab[inv].reshape(pre.shape)


def run_gn(C, x, gamma, beta, G, silu, C1, qp=None, raw_qp=None):
    xa = t(x if C1 is None else x[..., :C1])
    xb = None if C1 is None else t(x[..., C1:])
    kw = dict(x2=xb) if C1 is not None else {}
    if raw_qp is not None:
        kw["raw_qparams"] = [(scal(a), scal(b)) for a, b in raw_qp]
    args = (scal(qp[0]), scal(qp[1])) if qp else ()
    return C.groupnorm_silu_quantize(xa, G, t(gamma), t(beta), 1e-5, *args, silu=silu, want_f16=True, **kw)


@pytest.mark.parametrize("case", GN_EXACT, ids=[f"n{c[0]}_hw{c[1]}_c{c[2]}_g{c[3]}_{'silu' if c[4] else 'plain'}"
                                                 f"{'' if c[5] is None else '_split%d' % c[5]}" for c in GN_EXACT])
def test_groupnorm_exact_every_pixel_once_in_its_group(C, oracle, case):
    N, HW, Cc, G, silu, C1 = case
    geom = ne.gn_launch(N, HW, Cc, G, silu)
    base = ei.gn_base(N, HW, Cc, G)
    runs = [("base", base[0], None)]
    for name, (p, ch) in ei.gn_heavy_positions(geom, C1).items():
        x, _, _, info = ei.gn_heavy(N, HW, Cc, G, p, ch)
        runs.append((name, x, info))
    gamma, beta = base[1], base[2]
    s0, q0 = ei.gn_group_sums(base[0], G)
    for name, x, info in runs:
        want, st = ei.gn_expected(x, gamma, beta, G)
        if info is not None:                   # the heavy element moved exactly one group's integers
            ds, dq = st["s"] - s0, st["q"] - q0
            assert ds[info["image"], info["group"]] == info["ds"] and dq[info["image"], info["group"]] == info["dq"]
            assert np.count_nonzero(ds) <= 1 and np.count_nonzero(dq) == 1
        _, pre = run_gn(C, x, gamma, beta, G, False, C1)
        got = pre.cpu().numpy()
        bad = got.view(np.uint16) != want.view(np.uint16)
        assert not bad.any(), f"{name}: {bad.sum()} pre-activation values differ, first at {np.argwhere(bad)[0]}"
        if silu:
            _, h = run_gn(C, x, gamma, beta, G, True, C1)
            assert np.array_equal(h.cpu().numpy().view(np.uint16), silu_spec(oracle, want).view(np.uint16)), name
    # the constant group (variance exactly 0: rstd = 1 / sqrt(eps)) and the all-zero image are in the base tensor
    _, st = ei.gn_expected(base[0], gamma, beta, G)
    assert st["var"][N - 1, 1] == 0 and st["rstd"][N - 1, 1] == np.float32(1) / np.sqrt(np.float32(1e-5))
    if N > 1:
        want, _ = ei.gn_expected(base[0], gamma, beta, G)
        assert np.array_equal(want[0], np.broadcast_to(beta, want[0].shape))       # zero image: exactly beta


LN_EXACT = (16, 32, 48, 96, 160, 320, 512, 960, 1024, 1168, 1536, 1920, 2032, 2048)


@pytest.mark.parametrize("Cc", LN_EXACT)
def test_layernorm_exact_zero_sum_rows_and_a_moving_heavy_element(C, Cc):
    x, gamma, beta, cols = ei.ln_heavy(Cc)
    consts = (0, 3, 4, -7)
    xc = np.concatenate([x] + [np.full((1, Cc), c, np.float16) for c in consts] +
                        [ei.ln_zero_sum_rows(5, Cc, seed=1)], axis=0)
    _, h = C.layernorm_quantize(t(xc), t(gamma), t(beta), 1e-5, [], want_f16=True)
    got = h.cpu().numpy()
    n = 1 + len(cols)
    # zero-sum rows: the closed formula, bit for bit
    zs = np.r_[0, np.arange(n + len(consts), xc.shape[0])]
    want = ei.ln_expected_zero_mean(xc[zs], gamma, beta)
    assert np.array_equal(got[zs].view(np.uint16), want.view(np.uint16))
    for i, c in enumerate(consts):
        assert np.array_equal(got[n + i].view(np.uint16), ei.ln_expected_constant(c, Cc, gamma, beta).view(np.uint16)), c
    assert np.array_equal(got[n].view(np.uint16), beta.view(np.uint16))                     # the zero row: exactly beta
    # the heavy element: the float64 bound, and the change against the base row as the float64 reference has it
    ref = ne.layernorm64(xc[:n], gamma, beta, 1e-5)
    assert ne.within_norm_bound(got[:n], ref).all()
    d_got = got[1:n].astype(np.float64) - got[0].astype(np.float64)
    d_ref = ref[1:] - ref[0]
    am = np.abs(d_ref).argmax(axis=1)
    assert np.array_equal(am, np.asarray(cols)) and np.array_equal(np.abs(d_got).argmax(axis=1), am)
    r = np.arange(len(cols))
    assert np.array_equal(np.sign(d_got[r, am]), np.sign(d_ref[r, am]))


@pytest.mark.parametrize("M,Cc", [(5, 320), (8193, 16), (3, 2032)])
def test_layernorm_quantizer_edges(C, oracle, M, Cc):
    """gamma = 0 on the even columns: the output there IS beta, placed on the three quantizers' ties and clamp ends
    (asserted); the odd columns carry ordinary normalised values.  INT8 == oracle.quantize of the kernel's own FP16."""
    x, gamma, _ = ne.ln_inputs(M, Cc)
    gamma = gamma.copy()
    gamma[0::2] = 0
    beta = ei.qedge_values(Cc)
    for qp in ei.QEDGE_LN:
        f = ei.qedge_facts(beta[0::2], *qp)
        assert Cc < 512 or all(f.values()), (qp, f)
    outs, h = C.layernorm_quantize(t(x), t(gamma), t(beta), 1e-5, [(scal(a), scal(b)) for a, b in ei.QEDGE_LN],
                                   want_f16=True)
    hn = h.cpu().numpy()
    assert np.array_equal(hn[:, 0::2].view(np.uint16), np.broadcast_to(beta[0::2], (M, Cc // 2)).view(np.uint16))
    for o, (a, b) in zip(outs, ei.QEDGE_LN):
        assert np.array_equal(o.cpu().numpy(), oracle.quantize(hn, a, b, C.FLAGS & 1))


@pytest.mark.parametrize("N,HW,Cc,G,C1", [(1, 33, 64, 8, None), (2, 390, 320, 32, 168), (1, 2080, 64, 8, 32)])
def test_groupnorm_quantizer_edges(C, oracle, N, HW, Cc, G, C1):
    """The input itself lies on the raw quantizers' edges (values k / 8 in [-80, 80]); gamma = 0 on the even channels
    puts the norm's own output on the consumer quantizer's.  Every INT8 == oracle.quantize of the FP16 it is made of."""
    x = ei.qedge_values(N * HW * Cc, seed=3).reshape(N, HW, Cc)
    gamma, _ = ei._seeded_affine(5, Cc)
    gamma = gamma.copy()
    gamma[0::2] = 0
    beta = ei.qedge_values(Cc, seed=4)
    assert all(ei.qedge_facts(x, *qp)[k] for qp in ei.QEDGE_RAW for k in ("tie_even", "tie_odd", "below", "above"))
    raw_qp = list(ei.QEDGE_RAW[:1 if C1 is None else 2])
    q, h, raws = run_gn(C, x, gamma, beta, G, False, C1, qp=ei.QEDGE_GN, raw_qp=raw_qp)
    hn = h.cpu().numpy()
    assert np.array_equal(hn[..., 0::2].view(np.uint16), np.broadcast_to(beta[0::2], hn[..., 0::2].shape).view(np.uint16))
    assert np.array_equal(q.cpu().numpy(), oracle.quantize(hn, *ei.QEDGE_GN, C.FLAGS & 1))
    srcs = [x] if C1 is None else [x[..., :C1], x[..., C1:]]
    for r, src, qp in zip(raws, srcs, raw_qp):
        assert np.array_equal(r.cpu().numpy(), oracle.quantize(np.ascontiguousarray(src), *qp, C.FLAGS & 1))
