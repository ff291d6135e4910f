"""LoraBank (mixdq_amd/lora.py) against merge-then-quantize (tests/merge_oracle.py): the adapters merged into the float
weights in their own [K, C, R, S] layout and the normal quantize_unet path run on the result.  Everything the bank does
between a user's adapter tensors and its launches -- factor order, alpha / r, column slices, rank offsets, strengths,
rank ranges, the magnitude's on / off rule, the BOS row -- is pinned here; the launches themselves are pinned by
tests/test_lora_gpu.py and tests/test_lycoris_gpu.py."""
import numpy as np
import pytest
import torch

from tests import merge_oracle as M
from tests.test_control_gpu import DEV, FP16_LAYERS, L_TINY
from tests.test_lora_gpu import NARROW

pytestmark = pytest.mark.gpu
MAX_RANK = {"lora": 32, "loha": 128, "dora": 64}               # loha: 32 linear ranks and three Hadamard ranges at most


def _unit(form, plant):
    """The unit under test: the tiny UNet of the bank tests, W8A8 with NARROW's layers, w4_kernel, bos, fused.
    `plant(info) -> {"<name>.weight": tensor}` replaces float weights BEFORE calibration."""
    import bench
    from mixdq_amd import unet as U
    from mixdq_amd.calib import calibrate, precompute_bos
    from mixdq_amd.quantize_sdxl import example_inputs, quantize_unet
    inp = example_inputs(2, L_TINY, DEV, seed=7)
    g = torch.Generator(device="cpu").manual_seed(5)               # token 0: small integers, so that the BOS row is exact
    inp["encoder_hidden_states"][:, 0] = torch.randint(-2, 3, (2048,), generator=g).half().to(DEV)
    unet = U.build_unet(DEV, cfg=M.tiny_cfg())
    info = M.target_info(unet, form)
    state = {k: v.detach().clone() for k, v in unet.state_dict().items()}
    state.update({k: v.to(DEV) for k, v in plant(info).items()})
    unet.load_state_dict(state)
    names = list(U.quantizable_layers(unet))
    qcfg = bench.Cfg({n: NARROW.get(n, 8) for n in names}, {n: 8 for n in names if n.split(".")[0] not in FP16_LAYERS})
    with torch.no_grad():
        ckpt = calibrate(unet, [inp])
        quantize_unet(unet, qcfg, ckpt, bos=True, bos_dict=precompute_bos(unet, inp["encoder_hidden_states"]), w4_kernel=True)
    unet.set_fused(True)
    return unet, state, ckpt, qcfg, inp, info


def _oracle(state, adapters, scales, ckpt, rule, qcfg, inp, info, exact, forward=False):
    return M.oracle_unet(M.tiny_cfg(), M.merged_state(state, adapters, scales, exact=exact), ckpt, rule, qcfg=qcfg,
                         targets=list(info[0]), ehs=inp["encoder_hidden_states"], device=DEV, inp=inp if forward else None,
                         w4_kernel=True)


@pytest.mark.parametrize("form", ["lora", "loha", "dora"])
@pytest.mark.parametrize("rule", ["keep", "absmax"])
def test_exact_adapters_equal_merge_then_quantize(C, rule, form):
    """Planted inputs (tests/merge_oracle.py exact_case; their conditions are checked on the CPU by
    tests/test_merge_oracle_host.py): every product, partial sum, FP16 cast and -- under 'absmax' -- every delta is
    exact, so after apply() and after set_scales() the bank's UNet and a freshly quantized merged UNet have the same
    state_dict(), key by key, bit for bit: integers, packed nibbles, scales, sums, the FP16 layer and the BOS rows
    (token 0 is small integers: x W'^T is exact in FP32 on both sides and rounded to FP16 once)."""
    from mixdq_amd.lora import LoraBank
    case = {}

    def plant(info):
        case.update(M.exact_case(form, *info, stacked=M.form_targets(form)[0]))
        return case["base"]
    unet, state, ckpt, qcfg, inp, info = _unit(form, plant)
    adapters = M.to_device(case["adapters"], DEV)
    with torch.no_grad():
        bank = LoraBank(unet, state, bos_embedding=inp["encoder_hidden_states"][0, 0], max_rank=MAX_RANK[form], scales=rule)
        snap = {k: v.clone() for k, v in unet.state_dict().items()}
        bank.apply(adapters, case["scales"])
        want, _ = _oracle(state, adapters, case["scales"], ckpt, rule, qcfg, inp, info, exact=True)
        diff = M.first_difference(unet.state_dict(), want.state_dict())
        assert diff is None, f"apply({case['scales']}): {diff}"
        assert M.first_difference(unet.state_dict(), snap) is not None, "the adapters changed something"
        del want
        bank.set_scales(case["scales2"])                       # copies no factor: svec and the magnitude's on / off rule
        want, _ = _oracle(state, adapters, case["scales2"], ckpt, rule, qcfg, inp, info, exact=True)
        diff = M.first_difference(unet.state_dict(), want.state_dict())
        assert diff is None, f"set_scales({case['scales2']}): {diff}"
        bank.restore()
        diff = M.first_difference(unet.state_dict(), snap)
        assert diff is None, f"restore(): {diff}"


def _ints(mod, sfx):
    from mixdq_amd.nn import QuantizedConv2d
    return (mod._weight_values(sfx) if isinstance(mod, QuantizedConv2d) else mod._weight_values()).cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("form", ["lora", "loha", "dora"])
def test_random_adapters_against_merge_then_quantize(C, form):
    """Gaussian factors under KEEP.  The oracle's merged weights are rounded to FP16, the kernel's FP32 accumulators are
    not, so an integer may differ by 1 -- per layer at no more elements than lie inside the band of
    tests/merge_oracle.py band() (a float64 count that does not depend on the stored order; below 5 % of a layer, a
    condition on the inputs that tests/test_merge_oracle_host.py checks on the CPU).  Scales are bit-equal, every sum
    moves by at most its row's differing integers, every other key is bit-equal, and the FP16 layer agrees within the
    two roundings plus the accumulation bound.  The forward outputs are printed for the record:
    max |bank - oracle| against max |oracle - float merged UNet| (the network's own quantization error, measured on the
    oracle); only that the first is not the larger one is asserted.  Measured on an MI355X: lora 6.1e-02 against
    3.0e-01, loha 8.3e-02 against 2.7e-01, dora 7.1e-02 against 3.0e-01; about a sixth of a layer's in-band integers differ."""
    from mixdq_amd.lora import LoraBank
    unet, state, ckpt, qcfg, inp, info = _unit(form, lambda info: {})
    shapes, bits, splits = info
    cpu_state = {k: v.cpu() for k, v in state.items()}
    adapters, scales = M.random_case(form, shapes, cpu_state)
    bands = M.random_bands(form, cpu_state, info, ckpt, MAX_RANK[form])
    with torch.no_grad():
        bank = LoraBank(unet, state, bos_embedding=inp["encoder_hidden_states"][0, 0], max_rank=MAX_RANK[form], scales="keep")
        bank.apply(M.to_device(adapters, DEV), scales)
        want, y_float = _oracle(state, adapters, scales, ckpt, "keep", qcfg, inp, info, exact=False, forward=True)
        y_bank, y_want = unet(**inp)[0].float(), want(**inp)[0].float()
    got_mods, want_mods = dict(unet.named_modules()), dict(want.named_modules())
    checked = set()
    for n in shapes:
        gm, wm = got_mods[n], want_mods[n]
        if bits[n] == 16:
            wp, tol = M.accumulation_bound(cpu_state[n + ".weight"], n, adapters, scales, MAX_RANK[form])
            err = np.abs(gm.weight.float().cpu().numpy().astype(np.float64) - wm.weight.float().cpu().numpy()).reshape(wp.shape)
            assert (err <= 2.0 ** -10 * np.abs(wp) + 2.0 ** -24 + tol).all(), n
            checked.add(n + ".weight")
            continue
        for sfx, _ in M.layer_parts(n, shapes[n], splits[n]):
            inb, _, delta = bands[n, sfx]
            q, qw = _ints(gm, sfx), _ints(wm, sfx)
            d = np.abs(q - qw)
            print(f"{form} {n}{sfx}: {int((d != 0).sum())} integers differ, {int(inb.sum())} of {inb.size} ({inb.mean():.3%}) in the band")
            assert inb.mean() < 0.05, (n, sfx)
            assert d.max() <= 1 and (d != 0).sum() <= inb.sum(), (n, sfx)
            for v in ("weight_scales", "scale"):
                assert torch.equal(getattr(gm, v + sfx), getattr(wm, v + sfx)), (n, v + sfx)
            ws, ww = (getattr(m, "weight_sum_by_input_channels" + sfx) for m in (gm, wm))
            if q.ndim == 4:
                taps, rows = q.sum(axis=1, keepdims=True), (d != 0).sum(axis=1, keepdims=True)
            else:
                taps, rows = q.sum(axis=1), (d != 0).sum(axis=1)
            if ws is not None:
                assert np.array_equal(ws.cpu().numpy(), taps.astype(np.float32)), f"{n}{sfx}: the sums of ITS integers"
                assert (np.abs(ws.cpu().numpy() - ww.cpu().numpy()) <= rows).all(), (n, sfx)
            b0 = getattr(gm, "bias0" + sfx)
            if b0 is not None:
                azp = np.float32(float(getattr(gm, "act_zero_points" + sfx)))
                assert np.array_equal(b0.cpu().numpy(), taps.reshape(len(q), -1).sum(axis=1).astype(np.float32) * azp), (n, sfx)
            for k in dict(gm.named_buffers(recurse=False)):
                if k.endswith(sfx) or sfx == "":
                    checked.add(f"{n}.{k}")
    sd, sw = unet.state_dict(), want.state_dict()
    assert list(sd) == list(sw)
    for k in sd:                                               # every key no adapter reaches: bit for bit
        if k not in checked and not k.endswith("bos_pre_computed"):
            assert torch.equal(sd[k], sw[k]), k
    a, b = float((y_bank - y_want).abs().max()), float((y_want - y_float.float()).abs().max())
    print(f"{form}: max |bank - oracle| {a:.3e}, max |oracle - float merged| {b:.3e}")
    assert np.isfinite(a) and np.isfinite(b) and a <= b
