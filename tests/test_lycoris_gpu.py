"""mixdq_lycoris_requant (csrc/lycoris.hip) against its float64 restatement (tests/lycoris_ref.py): exact inputs bit for
bit, a linear-only table against lora_requant's bytes, random inputs within the derived band, LoraBank on a tiny UNet."""
import numpy as np
import pytest
import torch

from mixdq_amd.nn.utils import unpack_w4
from tests import lycoris_ref as R
from tests.lora_ref import stored
from tests.test_control_gpu import DEV, t
from tests.test_lora_gpu import ACT_SCALE, ACT_ZP, COL0, MODES, PAD, _check      # the strided master, the bitwise compare

pytestmark = pytest.mark.gpu
TERMS = {"had4": ((), (4,)), "lin8+had4+had40": ((8,), (4, 40))}      # (linear ranks, Hadamard ranks): 40 spans two pieces


def _launch(C, layers, lora=False):
    """One launch over `layers` (numpy, logical row order); per layer the device results as numpy, in STORED row order."""
    descs, keep = [], []
    for L in layers:
        n, kf = L["W"].shape
        master = np.full((n, kf + PAD), 7.0, np.float16)
        master[:, COL0:COL0 + kf] = L["W"]
        taps = kf // L["tap_len"]
        d = dict(W=t(master), Bcat=t(L["B"]), Acat=t(L["A"]), svec=t(L["svec"]), row_map=t(L["row_map"].astype(np.int32)),
                 out=torch.full((n, kf // 2 if L["mode"] == "w4" else kf), 5, device=DEV,
                                dtype=torch.float16 if L["mode"] == "f16" else torch.int8),
                 weight_scales=t(stored(L["old_scales"], L["row_map"])), wsum=torch.zeros((n, taps), device=DEV),
                 bias0=torch.zeros(n, device=DEV) if taps == 1 else None, scale=torch.zeros(n, device=DEV),
                 act_scale=t(np.float32([ACT_SCALE])), act_zero_point=t(np.float32([ACT_ZP])))
        base = C.LoraLayer(ldw=kf + PAD, w_col0=COL0, N=n, Kf=kf, R=L["B"].shape[1], mode=MODES[L["mode"]],
                           rule=int(L["rule"] == "absmax"), bits=L["bits"], tap_len=L["tap_len"],
                           **{k: (v.data_ptr() if v is not None else None) for k, v in d.items()})
        if not lora:
            d.update(B2cat=t(L["B2"]), A2cat=t(L["A2"]), magnitude=None if L["m"] is None else t(L["m"]))
            base = C.LycorisLayer.from_lora(base, R_lin=L["r_lin"], had_end=L["ends"], B2cat=d["B2cat"].data_ptr(),
                                            A2cat=d["A2cat"].data_ptr(),
                                            magnitude=None if L["m"] is None else d["magnitude"].data_ptr())
        keep.append(d)
        descs.append(base)
    C.lora_requant(C.LoraTable(descs, DEV, keep)) if lora else C.lycoris_requant(C.LycorisTable(descs, DEV, keep))
    torch.cuda.synchronize()
    return [{k: v.cpu().numpy() for k, v in d.items() if v is not None} for d in keep]


def _layer(seed, n, kf, terms, mode, rule, bits, tap_len, mag, exact=True):
    """Exact: small integers times powers of two, every product and partial sum exact in FP32 in any order; a Hadamard
    factor row has four non-zero ranks, so |dW| < 300.  With a magnitude the merged row is planted: W = T - dW with
    sum T^2 = 2 * 64 + 6 * 16 + 6 * 4 + 8 = 256 = 4^4 and m = 16 * 2^j, so g = 2^j; row 5 is all zero (g = 1, ABSMAX
    keeps its old scale).  Not exact: Gaussian factors."""
    g = np.random.default_rng(seed)
    lin, had = terms
    r_lin = -(-sum(lin) // 32) * 32
    ends = [int(e) for e in r_lin + np.cumsum([-(-r // 32) * 32 for r in had])]
    rank = max(32, ends[-1] if ends else r_lin)
    B, A, B2, A2 = (np.zeros(s, np.float16) for s in ((n, rank), (rank, kf)) * 2)
    svec, a = np.zeros(rank, np.float32), 0
    for r in lin:
        B[:, a:a + r], A[a:a + r] = (g.integers(-3, 4, s) if exact else g.standard_normal(s) * 0.1 for s in ((n, r), (r, kf)))
        svec[a:a + r], a = 0.5, a + r
    for r, e in zip(had, ends):
        a = e - -(-r // 32) * 32
        for Bx, Ax in ((B, A), (B2, A2)):
            if exact:
                Ax[a:a + r] = g.integers(-2, 3, (r, kf))
                for row in range(n):
                    Bx[row, a + g.choice(r, min(r, 4), replace=False)] = g.choice([-2, -1, 1, 2], min(r, 4))
            else:
                Bx[:, a:a + r], Ax[a:a + r] = g.standard_normal((n, r)) * 0.15, g.standard_normal((r, kf)) * 0.15
        svec[a:a + r] = 0.5
    B[5], B2[5] = 0, 0
    W = (g.integers(-100, 101, (n, kf)) * 0.25 if exact else g.standard_normal((n, kf)) * 0.05).astype(np.float16)
    W[5] = 0
    old = (2.0 ** g.integers(-2, 1, n) * (16 if mode == "w4" else 1)).astype(np.float32)
    if not exact:
        old = (np.abs(W).max(axis=1).astype(np.float32) * 1.3 + 0.01) / np.float32(2 ** (bits - 1) - 1)
    L = dict(W=W, B=B, A=A, B2=B2, A2=A2, svec=svec, r_lin=r_lin, ends=ends, m=None, row_map=g.permutation(n), mode=mode,
             rule=rule, bits=bits, old_scales=old, tap_len=tap_len)
    if mag and exact:
        T = np.zeros((n, kf))
        for row in range(n):
            T[row, g.permutation(kf)[:22]] = np.repeat([8, 4, 2, 1], [2, 6, 6, 8]) * g.choice([-1, 1], 22)
        T[5] = 0
        dW = R.merged(dict(L, W=np.zeros_like(W)))[0]
        L["W"] = (T - dW).astype(np.float16)
        assert np.array_equal(L["W"].astype(np.float64), T - dW), "the planted master is FP16"
        L["m"] = (16.0 * 2.0 ** g.integers(-2, 2, n)).astype(np.float32)
    elif mag:
        L["m"] = (np.abs(g.standard_normal(n)) + 0.5).astype(np.float32)
    return L


# per mode: (N, Kf, columns per tap sum) -- the row tail with 4-byte stores, a partial second trip, a padded conv's taps
SHAPES = {"int8": [(17, 36, 36), (16, 272, 272), (17, 72, 8)], "w4": [(17, 32, 32), (16, 288, 96)],
          "f16": [(17, 36, 36), (16, 272, 272)]}
CASES = [("int8", "keep"), ("int8", "absmax"), ("w4", "keep"), ("w4", "absmax"), ("f16", "keep")]


@pytest.mark.parametrize("mag", [False, True])
@pytest.mark.parametrize("terms", list(TERMS))
@pytest.mark.parametrize("mode,rule", CASES)
def test_exact_inputs_bit_for_bit(C, mode, rule, terms, mag):
    layers = [_layer(10 * i + mag, n, kf, TERMS[terms], mode, rule, 8 if mode != "w4" else (4, 2)[i], tap, mag)
              for i, (n, kf, tap) in enumerate(SHAPES[mode])]
    got = _launch(C, layers)                                   # layers of different Kf in one launch: the prefix search
    for g_, L in zip(got, layers):
        _check(g_, L, R.requant(L, ACT_SCALE, ACT_ZP))


@pytest.mark.parametrize("mode,rule", CASES)
def test_linear_terms_only_write_lora_requant_bytes(C, mode, rule):
    layers = [_layer(3 + i, n, kf, ((8, 24, 40), ()), mode, rule, 8 if mode != "w4" else 4, tap, False, exact=False)
              for i, (n, kf, tap) in enumerate(SHAPES[mode])]
    for a, b in zip(_launch(C, layers), _launch(C, layers, lora=True)):
        for k in b:
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


@pytest.mark.parametrize("mode,rule", [("int8", "keep"), ("int8", "absmax"), ("w4", "absmax"), ("f16", "keep")])
def test_random_inputs_within_the_accumulation_band(C, mode, rule):
    """Gaussian factors, a rank-16 pair, Hadamard ranks 24 and 40 and a magnitude.  An integer may differ by 1, and only
    where the restatement's quotient lies within tau of a half-integer (tau: tests/lycoris_ref.py, from the ranks, Kf and
    the magnitudes of the terms); such elements may be at most 1 % of a case.  Share inside the band, found on the CPU
    from the restatement alone for seed 11: int8 keep 0.37 %, int8 absmax 0.42 %, w4 absmax 0.02 %."""
    kf = 520 if mode != "w4" else 544
    L = _layer(11, 48, kf, ((16,), (24, 40)), mode, rule, 4 if mode == "w4" else 8, kf, True, exact=False)
    got = _launch(C, [L])[0]
    want = R.requant(L, ACT_SCALE, ACT_ZP)
    if mode == "f16":
        err = np.abs(got["out"][L["row_map"]].astype(np.float64) - want["ws"])
        assert (err <= 2.0 ** -11 * np.abs(want["ws"]) + 2.0 ** -25 + want["tol"]).all()
        return
    delta = got["weight_scales"][L["row_map"]]
    assert (np.abs(delta - want["weight_scales"]) <= (2.0 ** -20 + want["g_rel"]) * want["weight_scales"]).all(), "delta_n"
    want = R.requant(L, ACT_SCALE, ACT_ZP, delta=delta)
    q = got["out"][L["row_map"]]
    q = q if mode == "int8" else unpack_w4(torch.from_numpy(q)).numpy()
    band = np.abs(want["quot"] - np.floor(want["quot"]) - 0.5) <= want["tau"]
    print(f"{mode} {rule}: share inside the band {band.mean():.5%}, differing {int((q != want['q']).sum())}")
    assert band.mean() < 0.01
    assert np.array_equal(q[~band], want["q"][~band]), "outside the band the integers are equal"
    assert (np.abs(q.astype(int) - want["q"].astype(int)) <= 1).all()
    assert np.array_equal(got["wsum"][L["row_map"], 0], q.astype(np.int64).sum(axis=1).astype(np.float32)), "wsum of ITS q"


BLK = "down_blocks.1.attentions.0.transformer_blocks.0."
TARGETS = (BLK + "attn1.to_q", BLK + "attn1.to_out.0", BLK + "attn2.to_k", BLK + "ff.net.0.proj",
           "down_blocks.0.resnets.0.conv1", "conv_in")         # a q|k|v view, packed W4, BOS, a row map, a padded conv, FP16


@pytest.mark.parametrize("rule", ["keep", "absmax"])
def test_bank_loha_and_dora_on_a_unet(C, rule):
    import bench
    from mixdq_amd import unet as U
    from mixdq_amd.calib import calibrate, precompute_bos
    from mixdq_amd.lora import LoraBank
    from mixdq_amd.quantize_sdxl import example_inputs, quantize_unet
    from tests.test_control_gpu import FP16_LAYERS, L_TINY, _same
    inp = example_inputs(2, L_TINY, DEV, seed=7)
    unet = U.build_unet(DEV, cfg=dict(bench.TINY_CFG, block_out_channels=(64, 128, 256), head_dim=64))
    state = {k: v.detach().clone() for k, v in unet.state_dict().items()}
    names = list(U.quantizable_layers(unet))
    cfg = bench.Cfg({n: 4 if n == BLK + "attn1.to_out.0" else 8 for n in names},
                    {n: 8 for n in names if n.split(".")[0] not in FP16_LAYERS})
    quantize_unet(unet, cfg, calibrate(unet, [inp]), bos=True, bos_dict=precompute_bos(unet, inp["encoder_hidden_states"]),
                  w4_kernel=True)
    unet.set_fused(True)
    g = torch.Generator(device="cpu").manual_seed(3)
    rnd = lambda *s: (torch.randn(s, generator=g) * 0.2).half().to(DEV)      # noqa: E731
    loha, dora = {}, {}
    for name in TARGETS:
        w = state[name + ".weight"]
        n, rest = w.shape[0], tuple(w.shape[1:])
        loha[name] = dict(kind="loha", w1_a=rnd(n, 4), w1_b=rnd(4, w[0].numel()), w2_a=rnd(n, 4), w2_b=rnd(4, *rest), alpha=4.0)
        dora[name] = dict(kind="lora", A=rnd(8, *rest), B=rnd(n, 8), alpha=8.0,
                          magnitude=w.float().flatten(1).norm(dim=1) * 1.1)
    with torch.no_grad():
        before = unet(**inp)[0].clone()
        bank = LoraBank(unet, state, bos_embedding=inp["encoder_hidden_states"][0, 0], max_rank=64, scales=rule)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            unet(**inp)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                           # captured BEFORE apply
            out = unet(**inp)[0]
        snap = {k: v.clone() for k, v in unet.state_dict().items()}
        bank.apply([loha, dora], [1.0, 0.8])
        after = unet(**inp)[0].clone()
        assert not torch.equal(after, before) and bool(torch.isfinite(after).all())
        with U.defused():
            _same(after, unet(**inp)[0], "fused vs de-fused under LoHa + DoRA")
        for _ in range(3):
            graph.replay()
            _same(out, after, "a graph captured before apply, replayed after it")
        bank.set_scales([0.0, 0.0])
        zero = {k: v.clone() for k, v in unet.state_dict().items()}
        bank.restore()
        for k, v in unet.state_dict().items():
            assert torch.equal(v, snap[k]), f"restore(): {k}"
            if rule == "keep" and "bos_pre_computed" not in k:  # all zeros == restore under KEEP
                assert torch.equal(zero[k], snap[k]), f"set_scales(0): {k}"
        graph.replay()
        _same(out, before, "the graph after restore()")
