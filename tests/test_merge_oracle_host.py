"""tests/merge_oracle.py on the CPU: its merge against a second, differently written formula, the documented rules of
LoraBank.apply() it restates, what the planting helpers promise, and the band condition of the Gaussian cases."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import merge_oracle as M

FORMS = ("lora", "loha", "dora")


def _composed(A, B, shape):
    """dW of a pair of factors as the COMPOSITION of the two layers applied to an identity basis, in float64."""
    if len(shape) == 4:
        kf = int(np.prod(shape[1:]))
        eye = torch.eye(kf, dtype=torch.float64).reshape((kf,) + tuple(shape[1:]))       # one basis image per column
        up = F.conv2d(F.conv2d(eye, A.double().reshape((-1,) + tuple(shape[1:]))), B.double()[:, :, None, None])
        return up.reshape(kf, shape[0]).t().reshape(shape)
    return F.linear(F.linear(torch.eye(shape[1], dtype=torch.float64), A.double()), B.double()).t()


@pytest.mark.parametrize("shape", [(5, 6, 3, 3), (7, 10)])
def test_merged_state_against_the_composed_layers(shape):
    g = torch.Generator().manual_seed(1)
    rnd = lambda *s: torch.randn(s, generator=g).half()        # noqa: E731
    rest, kf = tuple(shape[1:]), int(np.prod(shape[1:]))
    w = rnd(*shape)
    lo = [(rnd(4, *rest), rnd(shape[0], 4), 2.0), dict(kind="lora", A=rnd(6, kf), B=rnd(shape[0], 6), alpha=3.0)]
    ha = dict(kind="loha", w1_a=rnd(shape[0], 3), w1_b=rnd(3, kf), w2_a=rnd(shape[0], 3), w2_b=rnd(3, *rest), alpha=1.5)
    scales = [1.0, 0.5, 0.25]
    want = w.double() + 1.0 * (2.0 / 4) * _composed(lo[0][0], lo[0][1], shape) \
        + 0.5 * (3.0 / 6) * _composed(lo[1]["A"], lo[1]["B"], shape) \
        + 0.25 * (1.5 / 3) * _composed(ha["w1_b"], ha["w1_a"], shape) * _composed(ha["w2_b"], ha["w2_a"], shape)
    got = M.merged_f64(w, "l", [{"l": lo[0]}, {"l": lo[1]}, {"l": ha}], scales)
    assert got.shape == w.shape and torch.allclose(got, want, rtol=0, atol=1e-12)
    state = {"l.weight": w, "other.weight": rnd(3, 3)}
    out = M.merged_state(state, [{"l": lo[0]}, {"l": lo[1]}, {"l": ha}], scales)
    assert out["l.weight"].dtype == torch.float16 and torch.equal(out["l.weight"], want.half())
    assert out["other.weight"] is state["other.weight"] and state["l.weight"] is w, "a new dict; the input is left alone"
    with pytest.raises(AssertionError):
        M.merged_state(state, [{"l": lo[0]}], [1.0], exact=True)       # Gaussian inputs are not exact, and it says so


def test_flat_and_4d_factors_agree_and_flat_is_crs_order():
    g = torch.Generator().manual_seed(2)
    rnd = lambda *s: torch.randn(s, generator=g).half()        # noqa: E731
    shape = (5, 6, 3, 3)
    A, B = rnd(4, 6, 3, 3), rnd(5, 4)
    w = torch.zeros(shape, dtype=torch.float16)
    four = M.merged_f64(w, "c", [{"c": dict(kind="lora", A=A, B=B, alpha=4.0)}], [1.0])
    flat = M.merged_f64(w, "c", [{"c": dict(kind="lora", A=A.reshape(4, -1), B=B, alpha=4.0)}], [1.0])
    assert torch.equal(four, flat)
    assert torch.equal(four[:, 2, 1, 0], B.double() @ A.double()[:, 2, 1, 0])          # column (c, r, s) of A -> W[:, c, r, s]
    stored = A.permute(0, 2, 3, 1).reshape(4, -1)                                      # (R, S, C): NOT the contract
    assert not torch.equal(M.merged_f64(w, "c", [{"c": dict(kind="lora", A=stored, B=B, alpha=4.0)}], [1.0]), four)


def test_strength_zero_drops_the_adapter_with_its_magnitude():
    g = torch.Generator().manual_seed(3)
    rnd = lambda *s: torch.randn(s, generator=g).half()        # noqa: E731
    w = rnd(6, 8)
    dora = dict(kind="lora", A=rnd(2, 8), B=rnd(6, 2), alpha=2.0, magnitude=torch.full((6,), 3.0))
    plain = (rnd(2, 8), rnd(6, 2), 2.0)
    on = M.merged_f64(w, "l", [{"l": dora}, {"l": plain}], [0.5, 1.0])
    assert torch.allclose(on.norm(dim=1), torch.full((6,), 3.0, dtype=torch.float64), rtol=1e-12), "g = m / ||row||"
    off = M.merged_f64(w, "l", [{"l": dora}, {"l": plain}], [0.0, 1.0])
    assert torch.equal(off, M.merged_f64(w, "l", [{"l": plain}], [1.0])), "0 means off: no dW and no magnitude"
    assert torch.equal(M.merged_f64(w, "l", [{"l": dora}, {"l": plain}], [0.0, 0.0]), w.double())


@pytest.fixture(scope="module")
def tiny():
    from mixdq_amd import unet as U
    unet = U.build_unet(None, cfg=M.tiny_cfg())
    return unet, {k: v.detach().clone() for k, v in unet.state_dict().items()}


@pytest.mark.parametrize("form", FORMS)
def test_planted_cases_are_exact_at_both_sets_of_strengths(tiny, form):
    """What tests/test_lora_oracle_gpu.py relies on: the FP16 casts lose nothing (merged_state asserts it), every row
    maximum is qmax 2^j in every quantizer's columns at the strengths of apply() AND of set_scales(), no row is zero,
    and with a magnitude the row norms are powers of two."""
    unet, state = tiny
    shapes, bits, splits = info = M.target_info(unet, form)
    case = M.exact_case(form, *info, stacked=M.form_targets(form)[0])
    planted = dict(state, **case["base"])
    for scales in (case["scales"], case["scales2"]):
        merged = M.merged_state(planted, case["adapters"], scales, exact=True)
        for n in shapes:
            w = merged[n + ".weight"]
            assert w.dtype == torch.float16 and w.shape == shapes[n]
            parts = tuple(c for _, c in M.layer_parts(n, shapes[n], splits[n]))
            assert M.row_maxima_exact(w, min(bits[n], 8), parts), (n, scales)
    for n in shapes:
        T = case["T"][n] * M.UNIT
        got = M.merged_f64(planted[n + ".weight"], n, case["adapters"], case["scales"])
        if form != "dora":
            assert torch.equal(got, T), f"{n}: the merged weight is the planted target"
            continue
        assert M.row_norms_exact(T), n
        g = (got / T)[T != 0]
        assert torch.equal(torch.exp2(torch.log2(g).round()), g) and len(g.unique()) > 1, f"{n}: g is a power of two, not one"


def test_planting_refuses_what_is_not_exact():
    g = np.random.default_rng(0)
    free = M.free_mask(g, (8, 16))
    T = M.planted_target(g, (8, 16), 8, free)
    assert M.row_maxima_exact(T * M.UNIT, 8) and not M.row_maxima_exact(T * M.UNIT, 4)
    assert M.row_norms_exact(M.planted_target(g, (8, 16), 4, free, norm=True)) and not M.row_norms_exact(T)
    third = (torch.full((1, 16), 64 / 3).half(), torch.ones(8, 1).half(), 1.0)
    with pytest.raises(AssertionError):
        M.plant_base(T, "l", [{"l": third}], [1.0])


@pytest.mark.parametrize("form", FORMS)
def test_random_cases_meet_the_band_condition(tiny, form):
    """A condition on the INPUTS of test_random_adapters_against_merge_then_quantize: per quantized layer fewer than
    5 % of the elements may lie where the bank and merge-then-quantize can round to different integers."""
    from mixdq_amd.calib import weight_quantizer_entry
    unet, state = tiny
    shapes, bits, splits = info = M.target_info(unet, form)
    deltas = {}
    for n in shapes:
        for sfx, (a, b) in M.layer_parts(n, shapes[n], splits[n]):
            deltas[n + ".weight_quantizer" + sfx] = weight_quantizer_entry(state[n + ".weight"][:, a:b])
    adapters, scales = M.random_case(form, shapes, state)
    for (n, sfx), (inb, wp, _) in M.random_bands(form, state, info, deltas, max_rank=64).items():
        print(f"{form} {n}{sfx}: share inside the band {inb.mean():.4%}")
        assert inb.mean() < 0.05, (n, sfx)
        a, b = dict(M.layer_parts(n, shapes[n], splits[n]))[sfx]
        want = M.merged_f64(state[n + ".weight"], n, adapters, scales).flatten(1)[:, a:b].numpy()
        assert np.allclose(wp, want, rtol=1e-12, atol=1e-14), f"{n}: the staged layer is the merged weight"
