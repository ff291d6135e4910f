"""mixdq_lora_requant (csrc/lora.hip) against its float64 restatement (tests/lora_ref.py): exact inputs bit for bit,
random inputs within the derived FP32 accumulation band, and LoraBank end to end on a tiny UNet."""
import numpy as np
import pytest
import torch

from mixdq_amd.nn.utils import unpack_w4
from tests import lora_ref as R
from tests.test_control_gpu import DEV, t

pytestmark = pytest.mark.gpu
N = 40                                           # not a multiple of the 16-row block
MODES = {"int8": 0, "w4": 1, "f16": 2}
PAD, COL0, ACT_SCALE, ACT_ZP = 24, 8, 0.03125, -9.0   # master row stride Kf + 24, column offset 8; the activation quantizer


def _launch(C, layers):
    """One launch over `layers` (numpy, logical row order); per layer the device results as numpy, in STORED row order."""
    descs, keep = [], []
    for L in layers:
        n, kf = L["W"].shape
        ld = kf + PAD
        master = np.full((n, ld), 7.0, np.float16)
        master[:, COL0:COL0 + kf] = L["W"]
        out = torch.full((n, kf // 2 if L["mode"] == "w4" else kf), 5, device=DEV,
                         dtype=torch.float16 if L["mode"] == "f16" else torch.int8)
        taps = kf // L["tap_len"]
        d = dict(W=t(master), Bcat=t(L["B"]), Acat=t(L["A"]), svec=t(L["svec"]), row_map=t(L["row_map"].astype(np.int32)),
                 out=out, weight_scales=t(R.stored(L["old_scales"], L["row_map"])),
                 wsum=torch.zeros((n, taps), device=DEV), bias0=torch.zeros(n, device=DEV) if taps == 1 else None,
                 scale=torch.zeros(n, device=DEV), act_scale=t(np.float32([ACT_SCALE])), act_zero_point=t(np.float32([ACT_ZP])))
        keep.append(d)
        descs.append(C.LoraLayer(ldw=ld, w_col0=COL0, N=n, Kf=kf, R=L["B"].shape[1], mode=MODES[L["mode"]],
                                 rule=int(L["rule"] == "absmax"), bits=L["bits"], tap_len=L["tap_len"],
                                 **{k: (v.data_ptr() if v is not None else None) for k, v in d.items()}))
    C.lora_requant(C.LoraTable(descs, DEV, keep))
    torch.cuda.synchronize()
    return [{k: v.cpu().numpy() for k, v in d.items() if v is not None} for d in keep]


def _check(got, L, want):
    names = ("out",) if L["mode"] == "f16" else ("out", "weight_scales", "wsum", "scale") + (("bias0",) if "bias0" in got else ())
    for name in names:
        w = np.ascontiguousarray(R.stored(want[name], L["row_map"]))
        assert np.array_equal(got[name].view(np.uint8), w.view(np.uint8)), name


def _exact_layer(seed, kf, rank, mode, rule, bits, tap_len):
    """Small integers times powers of two: every product and partial sum is exact in FP32 in any order.  R = 32: one
    rank-4 adapter padded with zeros; R = 96: three rank-32 adapters, the middle one with svec == 0.  Row 5 is all zero
    (ABSMAX keeps its old scale); under ABSMAX every other row's maximum is planted so that delta_n is a power of two."""
    g = np.random.default_rng(seed)
    W = (g.integers(-100, 101, (N, kf)) * 0.25).astype(np.float16)
    B = g.integers(-3, 4, (N, rank)).astype(np.float16)
    A = g.integers(-3, 4, (rank, kf)).astype(np.float16)
    svec = np.zeros(rank, np.float32)
    if rank == 32:
        B[:, 4:], A[4:], svec[:4] = 0, 0, 0.5
    else:
        svec[:32], svec[64:] = 0.5, -0.25
    W[5], B[5] = 0, 0
    qmax = 2 ** (bits - 1) - 1
    target = {127: 127.0, 7: 112.0, 1: 128.0}[qmax]
    if rule == "absmax" and mode != "f16":
        wp, _ = R.merged(W, B, A, svec)
        col = g.integers(0, kf, N)
        rows = np.arange(N)
        W[rows, col] = (W[rows, col].astype(np.float64) + target - wp[rows, col]).astype(np.float16)
        W[5] = 0
        wp, _ = R.merged(W, B, A, svec)
        assert (np.abs(np.delete(wp, 5, 0)).max(axis=1) == target).all(), "the planted maximum is the row maximum"
    old = (2.0 ** g.integers(-2, 1, N) * (16 if mode == "w4" else 1)).astype(np.float32)
    return dict(W=W, B=B, A=A, svec=svec, row_map=g.permutation(N), mode=mode, rule=rule, bits=bits, old_scales=old,
                tap_len=tap_len)


# (Kf, columns per tap sum): the small end, one trip + tail, two trips + tail -- INT8 / FP16 and packed W4
KF = {"int8": [(36, 12), (264, 88), (520, 104)], "w4": [(96, 32), (288, 96), (544, 136)],
      "f16": [(36, 12), (264, 88), (520, 104)]}


@pytest.mark.parametrize("rank", [32, 96])
@pytest.mark.parametrize("pair", [(0, 1), (2, 0)])
@pytest.mark.parametrize("mode,rule", [("int8", "keep"), ("int8", "absmax"), ("w4", "keep"), ("w4", "absmax"), ("f16", "keep")])
def test_exact_inputs_bit_for_bit(C, mode, rule, pair, rank):
    layers = []
    for i, p in enumerate(pair):
        kf, tap = KF[mode][p]
        bits = 8 if mode != "w4" else (4, 2)[i]               # the second W4 layer: a 2-bit quantizer in 4-bit storage
        layers.append(_exact_layer(100 * rank + 10 * p + i, kf, rank, mode, rule, bits, tap if i == 0 else kf))
    got = _launch(C, layers)                                   # two layers of different Kf: the prefix search
    for g_, L in zip(got, layers):
        _check(g_, L, R.requant(L["W"], L["B"], L["A"], L["svec"], mode, rule, L["bits"], L["old_scales"], ACT_SCALE, ACT_ZP,
                                L["tap_len"]))


def _band_rule(q, want, delta, rank, what):
    tau = (rank + 2) * 2.0 ** -24 * want["mag"] / delta[:, None].astype(np.float64)
    band = np.abs(want["quot"] - np.floor(want["quot"]) - 0.5) <= tau
    print(f"{what}: share inside the band {band.mean():.5%}, differing {int((q != want['q']).sum())}")
    assert band.mean() < 0.005, what
    assert np.array_equal(q[~band], want["q"][~band]), f"{what}: outside the band the integers are equal"
    assert (np.abs(q.astype(int) - want["q"].astype(int)) <= 1).all(), what


@pytest.mark.parametrize("mode,rule", [("int8", "keep"), ("int8", "absmax"), ("w4", "absmax")])
def test_random_inputs_within_the_accumulation_band(C, mode, rule):
    """Gaussian masters and one rank-64 pair.  An integer may differ by 1, and only where the restatement's quotient lies
    within tau = (R + 2) 2^-24 (|W| + sum |Bs A|) / delta of a half-integer.  Share of elements inside the band, found
    on the CPU for seed 11: int8 0.088 % (keep) and 0.084 % (absmax), w4 0.011 % -- the condition is < 0.5 %."""
    g = np.random.default_rng(11)
    n, kf, rank = 48, 520 if mode == "int8" else 544, 64
    W = (g.standard_normal((n, kf)) * 0.05).astype(np.float16)
    B = (g.standard_normal((n, rank)) * 0.05).astype(np.float16)
    A = (g.standard_normal((rank, kf)) * 0.1).astype(np.float16)
    bits = 8 if mode == "int8" else 4
    old = (np.abs(W).max(axis=1).astype(np.float32) * 1.3 / (2 ** (bits - 1) - 1)).astype(np.float32)
    L = dict(W=W, B=B, A=A, svec=np.full(rank, 0.75, np.float32), row_map=g.permutation(n), mode=mode, rule=rule,
             bits=bits, old_scales=old, tap_len=kf)
    got = _launch(C, [L])[0]
    args = (W, B, A, L["svec"], mode, rule, bits, old, ACT_SCALE, ACT_ZP, kf)
    want = R.requant(*args)
    delta = got["weight_scales"][L["row_map"]]
    assert (np.abs(delta - want["weight_scales"]) <= 2.0 ** -20 * want["weight_scales"]).all(), "delta_n"
    want = R.requant(*args, delta=delta)
    q = got["out"][L["row_map"]]
    q = q if mode == "int8" else unpack_w4(torch.from_numpy(q)).numpy()
    _band_rule(q, want, delta, rank, f"{mode} {rule}")
    assert np.array_equal(got["wsum"][L["row_map"], 0], q.astype(np.int64).sum(axis=1).astype(np.float32)), "wsum of ITS q"


# ---- end to end: LoraBank on the tiny UNet of tests/test_control_gpu.py, W8A8 with narrow and FP-fallback layers in it ----
BLK = "down_blocks.1.attentions.0.transformer_blocks.0."
NARROW = {BLK + "attn1.to_k": 4,                 # a 4-bit quantizer widened to INT8 storage beside to_q / to_v
          BLK + "attn1.to_out.0": 4,             # a packed-W4 Linear
          BLK + "ff.net.2": 2,                   # a 2-bit quantizer in W4 storage
          "down_blocks.0.resnets.0.conv2": 4}    # a packed-W4 conv, per-tap sums
TARGETS = tuple(NARROW) + (BLK + "attn1.to_q",   # a view of the stacked q|k|v weights
                           BLK + "attn2.to_k",   # a BOS layer
                           BLK + "ff.net.0.proj",                        # value|gate interleaved rows
                           "down_blocks.0.resnets.0.conv1",              # a padded INT8 conv
                           "up_blocks.0.resnets.0.conv_shortcut",        # split: two descriptors over one master
                           "conv_in")                                    # an FP-fallback layer


def _check_target(tg, rule):
    """One descriptor's buffers after apply() against the restatement on its master and factors: the random-input rule
    for the integers (under the GPU's delta_n), the vectors exactly from ITS integers; FP16: half an FP16 ulp plus the
    accumulation bound."""
    # (reads the bank's OWN staging: it pins the launch; tests/test_lora_oracle_gpu.py pins the staging itself)
    d, rm = tg.desc, (np.arange(tg.N) if tg.keep[1] is None else tg.keep[1].cpu().numpy())
    mode = ("int8", "w4", "f16")[d.mode]
    args = [a.cpu().numpy() for a in (tg.keep[0][:, tg.col0:tg.col0 + tg.kf], tg.Bcat, tg.Acat, tg.svec)]
    dense = (tg.out.permute(0, 2, 3, 1) if tg.out.dim() == 4 else tg.out).reshape(tg.N, -1)
    if mode == "f16":
        wp, mag = R.merged(*args)
        err = np.abs(dense.cpu().numpy().astype(np.float64) - wp)
        assert (err <= 2.0 ** -11 * np.abs(wp) + 2.0 ** -25 + 34 * 2.0 ** -24 * mag).all(), tg.name
        return
    get = lambda n: getattr(tg.mod, n + tg.sfx)                # noqa: E731
    delta, asc, azp = get("weight_scales").cpu().numpy()[rm], float(get("act_scales")), float(get("act_zero_points"))
    args += [mode, rule, d.bits, tg.snapshot[0].cpu().numpy()[rm], asc, azp, d.tap_len]
    want = R.requant(*args)["weight_scales"]
    assert (np.abs(delta - want) <= 2.0 ** -20 * want).all(), f"{tg.name}: delta_n"
    q = (unpack_w4(dense) if mode == "w4" else dense).cpu().numpy()[rm]
    _band_rule(q, R.requant(*args, delta=delta), delta, 32, f"{tg.name}{tg.sfx} {mode} {d.bits} bits")
    taps = q.reshape(tg.N, -1, d.tap_len).astype(np.int64).sum(axis=2)
    if get("weight_sum_by_input_channels") is not None:
        assert np.array_equal(get("weight_sum_by_input_channels").reshape(tg.N, -1).cpu().numpy()[rm], taps.astype(np.float32))
    if get("bias0") is not None:
        assert np.array_equal(get("bias0").cpu().numpy()[rm], taps.sum(axis=1).astype(np.float32) * np.float32(azp))
    assert np.array_equal(get("scale").cpu().numpy()[rm], delta * np.float32(asc)), f"{tg.name}: scale"


@pytest.mark.parametrize("rule", ["keep", "absmax"])
def test_bank_on_a_unet_graph_replay_restore_and_zero_scales(C, rule):
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
    cfg = bench.Cfg({n: NARROW.get(n, 8) for n in names}, {n: 8 for n in names if n.split(".")[0] not in FP16_LAYERS})
    quantize_unet(unet, cfg, calibrate(unet, [inp]), bos=True, bos_dict=precompute_bos(unet, inp["encoder_hidden_states"]),
                  w4_kernel=True)
    unet.set_fused(True)
    g = torch.Generator(device="cpu").manual_seed(3)
    adapter = {}
    for name in TARGETS:
        w = state[name + ".weight"]
        adapter[name] = ((torch.randn((8,) + tuple(w.shape[1:]), generator=g) * 0.05).half().to(DEV),
                         (torch.randn((w.shape[0], 8), generator=g) * 0.05).half().to(DEV), 16.0)
    with torch.no_grad():
        before = unet(**inp)[0].clone()
        bank = LoraBank(unet, state, bos_embedding=inp["encoder_hidden_states"][0, 0], max_rank=32, scales=rule)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            unet(**inp)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                           # captured BEFORE apply
            out = unet(**inp)[0]
        snap = {k: v.clone() for k, v in unet.state_dict().items()}
        bank.apply([adapter], [1.0])
        assert [t.desc.bits for n in NARROW for t in bank.targets[n]] == list(NARROW.values()), "the quantizers' own widths"
        after = unet(**inp)[0].clone()
        assert not torch.equal(after, before) and bool(torch.isfinite(after).all())
        with U.defused():
            _same(after, unet(**inp)[0], "fused vs de-fused under an adapter")
        for _ in range(3):
            graph.replay()
            _same(out, after, "a graph captured before apply, replayed after it")
        for name in TARGETS:                                    # every targeted layer, every buffer
            for tg in bank.targets[name]:
                _check_target(tg, rule)
        tk, x = bank.targets[BLK + "attn2.to_k"][0], inp["encoder_hidden_states"][0, 0].float()
        bos = x @ tk.keep[0].float().t() + ((x @ tk.Acat.float().t()) * tk.svec) @ tk.Bcat.float().t()
        _same(tk.mod.bos_pre_computed.flatten(), bos.half(), "the BOS row follows")
        bank.set_scales([0.0])
        zero = {k: v.clone() for k, v in unet.state_dict().items()}
        bank.restore()
        for k, v in unet.state_dict().items():
            assert torch.equal(v, snap[k]), f"restore(): {k}"
            if rule == "keep" and "bos_pre_computed" not in k:  # all zeros == restore under KEEP
                assert torch.equal(zero[k], snap[k]), f"set_scales(0): {k}"
        _same(unet(**inp)[0], before, "the forward after restore()")
        graph.replay()
        _same(out, before, "the graph after restore()")
