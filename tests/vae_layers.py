"""The distinct conv launches of the FP16 VAE (mixdq_amd.vae, both halves), enumerated from a config the way the two
forward passes walk their blocks (tests/test_vae_layers_gpu.py runs them, tests/test_vae_host.py checks the list).
Plain Python; imports without a GPU."""
from mixdq_amd import vae as V


def vae_conv_launches(cfg):
    """The distinct (Cin, Cout, kernel, stride, flag, residual) of the mixdq_conv2d_f16 launches of VAEDecoder.forward
    and VAEEncoder._moments, in the order the two walk their blocks (padding is kernel // 2 throughout)."""
    ch, layers, lc = tuple(cfg["block_out_channels"]), cfg["layers_per_block"], cfg["latent_channels"]
    out = []

    def res(cin, cout):                       # VaeResnetBlock.run
        out.append((cin, cout, 3, 1, None, False))
        if cin != cout:
            out.append((cin, cout, 1, 1, None, False))
        out.append((cout, cout, 3, 1, None, True))

    def mid(c):                               # VaeMidBlock.run (the attention between them has no conv)
        res(c, c)
        res(c, c)

    # the decoder
    rev = ch[::-1]
    out.append((lc, lc, 1, 1, None, False))                              # post_quant_conv
    out.append((lc, rev[0], 3, 1, None, False))                          # conv_in
    mid(rev[0])
    for i in range(len(rev)):
        for j in range(layers + 1):
            res(rev[max(i - 1, 0)] if j == 0 else rev[i], rev[i])
        if i != len(rev) - 1:
            out.append((rev[i], rev[i], 3, 1, "upsample2x", False))
    out.append((ch[0], (cfg.get("out_channels", 3) + 3) // 4 * 4, 3, 1, None, False))   # conv_out, padded to four
    # the encoder
    out.append((8, ch[0], 3, 1, None, False))                            # conv_in on the 8-channel ingest
    for i in range(len(ch)):
        for j in range(layers):
            res(ch[max(i - 1, 0)] if j == 0 else ch[i], ch[i])
        if i != len(ch) - 1:
            out.append((ch[i], ch[i], 3, 2, "pad_after", False))
    mid(ch[-1])
    out.append((ch[-1], 2 * lc, 3, 1, None, False))                      # conv_out
    out.append((2 * lc, 2 * lc, 1, 1, None, False))                      # quant_conv
    return list(dict.fromkeys(out))


LAUNCHES = vae_conv_launches(V.VAE_SDXL_CONFIG)


def launch_id(g):
    cin, cout, k, stride, flag, residual = g
    return f"c{cin}_k{cout}_{k}x{k}_s{stride}" + (f"_{flag}" if flag else "") + ("_res" if residual else "")


