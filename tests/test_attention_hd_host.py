"""Host-side routing of SD 1.5's head widths (mixdq_amd/nn/glue.py): which attention modules the kernel takes."""
from mixdq_amd.nn.glue import attention_head_dim, kernel_takes_scale


def test_attention_head_dim():
    assert [attention_head_dim(8 * d, 8) for d in (40, 64, 80, 160)] == [40, 64, 80, 160]
    assert [attention_head_dim(2 * d, 2) for d in (16, 32, 48, 96, 128)] == [None] * 5
    assert attention_head_dim(330, 8) is None and attention_head_dim(320, 0) is None
    assert attention_head_dim(None, 8) is None


def test_kernel_takes_scale():
    assert kernel_takes_scale(64, 0.125) and kernel_takes_scale(None, 0.125)     # the rule of head width 64 stays
    assert not kernel_takes_scale(64, 0.1) and not kernel_takes_scale(None, 40 ** -0.5)
    for d in (40, 80, 160):                                                       # diffusers' default only
        assert kernel_takes_scale(d, d ** -0.5)
        assert not kernel_takes_scale(d, 0.125) and not kernel_takes_scale(d, 1.0)
    assert not kernel_takes_scale(32, 32 ** -0.5)
