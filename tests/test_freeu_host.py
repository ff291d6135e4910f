"""FreeU without a GPU: the torch FP32 closed form against diffusers' fourier_filter written with torch.fft in float64, the
enable / disable state, the stage rule and the launch's refusals (host checks, nothing launched)."""
import pytest
import torch


def fourier_filter64(x, s):
    """diffusers' fourier_filter(x, threshold=1, scale=s), literally, in float64."""
    x = x.double()
    H, W = x.shape[-2:]
    f = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones_like(x)
    mask[..., H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1] = s
    return torch.fft.ifftn(torch.fft.ifftshift(f * mask, dim=(-2, -1)), dim=(-2, -1)).real


def reference(hidden, skip, b, s):
    """(hidden', skip') of diffusers' apply_freeu in float64."""
    h = hidden.double().clone()
    h[:, :h.shape[1] // 2] *= b
    return h, fourier_filter64(skip, s)


@pytest.mark.parametrize("shape", ((2, 3, 5, 7), (1, 2, 8, 6)))
def test_torch_form_is_the_fourier_filter(shape):
    from mixdq_amd.unet import _freeu_torch
    g = torch.Generator().manual_seed(3)
    skip = torch.randn(shape, generator=g) * 0.5 + 0.7
    hidden = torch.randn(shape[0], 4, *shape[2:], generator=g)
    for b, s in ((1.5, 0.9), (1.6, 0.2), (1.2, 0.0)):
        got_h, got_s = _freeu_torch(hidden, skip, torch.tensor(b), torch.tensor(s))
        ref_h, ref_s = reference(hidden, skip, b, s)
        # FP32 sums of H W <= 48 terms of size <= 4 and a 7-term correction: well inside 1e-5
        assert (got_s.double() - ref_s).abs().max() < 1e-5 and (got_h.double() - ref_h).abs().max() < 1e-6
    same_h, same_s = _freeu_torch(hidden, skip, torch.tensor(1.0), torch.tensor(1.0))
    assert torch.equal(same_h, hidden) and torch.equal(same_s, skip)
    with pytest.raises(RuntimeError, match="at least 2"):
        _freeu_torch(hidden[..., :1], skip[..., :1], torch.tensor(1.5), torch.tensor(0.9))


def test_enable_disable_and_the_stage_rule():
    import bench
    from mixdq_amd.unet import build_unet
    unet = build_unet("cpu", cfg=dict(bench.TINY_CFG, block_out_channels=(32, 32, 64), head_dim=32))
    assert not unet.freeu_enabled and all(blk.freeu is None for blk in unet.up_blocks)
    unet.enable_freeu(0.9, 0.2, 1.5, 1.6)                              # diffusers' order: s1, s2, b1, b2
    table = unet.up_blocks[0].freeu[0]
    assert table.tolist() == torch.tensor([[1.5, 0.9], [1.6, 0.2]]).tolist()
    assert [blk.freeu is not None for blk in unet.up_blocks] == [True, True, False]      # only up-blocks 0 and 1
    assert [blk.freeu[1] for blk in unet.up_blocks[:2]] == [0, 1]
    unet.enable_freeu(0.6, 0.4, 1.1, 1.2)                              # rewritten in place: the same tensor
    assert unet.up_blocks[1].freeu[0] is table and table[1].tolist() == torch.tensor([1.2, 0.4]).tolist()
    # the hook of up-block 1 is the float64 reference at (b2, s2)
    g = torch.Generator().manual_seed(5)
    x, skip = torch.randn(1, 8, 4, 6, generator=g), torch.randn(1, 6, 4, 6, generator=g) + 0.7
    got_h, got_s = unet.up_blocks[1]._freeu(x, skip)
    ref_h, ref_s = reference(x, skip, 1.2, 0.4)
    assert (got_h.double() - ref_h).abs().max() < 1e-6 and (got_s.double() - ref_s).abs().max() < 1e-5
    unet.disable_freeu()
    assert not unet.freeu_enabled
    # the table outlives a disable (a captured graph may still read it) and the next enable rewrites the same tensor
    assert unet.enable_freeu(0.9, 0.2, 1.5, 1.6).up_blocks[0].freeu[0] is table
    assert table.tolist() == torch.tensor([[1.5, 0.9], [1.6, 0.2]]).tolist()


@pytest.mark.parametrize("case, status", (("ok_shape_null", 1), ("H1", 9), ("W1", 9), ("C_s", 9), ("C_h", 9), ("in_place_skip", 1),
                                          ("in_place_hidden", 1), ("stage", 1), ("alignment", 2)))
def test_refusals_need_no_gpu(case, status):
    """mixdq_freeu_f16 answers on the host, before any launch: every call here is refused.  The addresses are made up and
    never dereferenced: each case differs from a valid call only in what the entry checks BEFORE it launches, and a case
    whose refusal were lost would fail here on its status (tests/test_cabi.py's validation test works the same way)."""
    from mixdq_amd import _C
    B, C_h, C_s, H, W = 1, 16, 8, 4, 4
    hid, skip, out_h, out_s, table, tw = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
    stage = 0
    if case == "ok_shape_null":
        hid = None
    elif case in ("H1", "W1"):
        H, W = (1, 4) if case == "H1" else (4, 1)
    elif case == "C_s":
        C_s = 12
    elif case == "C_h":
        C_h = 24                                                       # half of it is no multiple of 8
    elif case == "in_place_skip":
        out_s = skip
    elif case == "in_place_hidden":
        out_h = hid + 16                                               # overlapping, not equal
    elif case == "stage":
        stage = 2
    else:
        skip += 8
    assert _C._lib.mixdq_freeu_f16(hid, skip, out_h, out_s, table, stage, tw, B, C_h, C_s, H, W, None) == status


def test_exported_route_constants_agree():
    from mixdq_amd import _C
    assert _C.FREEU_RESIDENT_PIXELS == _C.FREEU_LANES * max(_C.FREEU_PPL)
