"""Edge-case generator of the producer launches of csrc/fused_norm.hip -- GroupNorm(+SiLU)+quantize,
LayerNorm+quantize, GEGLU+quantize -- and of LayerNorm inside the GEMM launch (tests/test_norm_edges_gpu.py runs the
cases, tests/test_norm_edges_host.py checks on the CPU that they reach every class they are there for and that this
restatement agrees with the library wherever the library answers without a GPU).

The launch code branches on quantities DERIVED from the shape, not on the shape: this module restates those
derivations in plain Python (make_gn_geom and mixdq_groupnorm_silu_quantize3; the LayerNorm kernel's (G, U, per,
chunks per lane, rows per wave); the GEGLU grids) and every case carries the derived quantities it is there for, so
that the coverage is an assertion over fields and not a reading of shapes.

Plain Python + numpy; imports without a GPU and without the built library.
"""
import numpy as np

from tests import detdata as dd

NUM_CU = 256                 # csrc/common.h kNumCU
TARGET_CHUNKS = 512          # make_gn_geom: blocks per image
SELF_FINALIZE_MAX = 64       # nchunk <= 64: the apply blocks finalize themselves
TAB_MIN = 2 << 20            # MIXDQ_GN_SILU_TAB_MIN / the GEGLU table threshold: elements
LN_MAX_CHUNKS = 4            # kLnMaxChunks
ELEMENT_CAP = 4 << 20        # "about 4 Mi elements" per tensor
VAE_EPS = (1e-6, 1e-5)       # mixdq_amd.vae.GN_EPS, and the UNet's


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ GroupNorm
def gn_geom(N, HW, C, G):
    """make_gn_geom: None where the library refuses the shape, else the statistics geometry."""
    if N <= 0 or HW <= 0 or C <= 0 or G <= 0 or C % G or C % 8:
        return None
    cg, OC = C // G, C // 8
    if OC > 1024:
        return None
    if any((8 * o + 7) // cg - (8 * o) // cg > 1 for o in range(OC)):     # an octet spans at most two groups
        return None
    PP = 1 if OC >= 256 else 256 // OC
    threads = OC * PP
    if G > threads:
        return None
    ppb = cdiv(cdiv(HW, TARGET_CHUNKS), PP) * PP
    nchunk = cdiv(HW, ppb)
    return dict(N=N, HW=HW, C=C, G=G, cg=cg, OC=OC, PP=PP, threads=threads, ppb=ppb, nchunk=nchunk,
                last_chunk_pixels=HW - (nchunk - 1) * ppb)


def gn_workspace_bytes(N, HW, C, G):
    g = gn_geom(N, HW, C, G)
    return 0 if g is None else (N * g["nchunk"] * G + N * G) * 8


def gn_launch(N, HW, C, G, silu, tab_mode=-1, stats_unroll=0):
    """mixdq_groupnorm_silu_quantize3 (unsliced: MIXDQ_GN_SLICED off): the statistics geometry plus
      unroll        pixels of a thread in flight in the statistics pass (2 where a thread has at most two, else 4)
      stats_iters   block iterations a statistics thread makes at most (ppb / PP); iterations past p_end are clamped
      finalize      "self" (apply blocks reduce the partials; nchunk <= 64) or "launch" (gn_finalize_kernel)
      nfull         complete waves of a block: only they reduce in the self-finalize
      self_branch   "pair" (GS <= 2 nfull: one pair of groups per wave) or "loop"; None with the finalize launch
      finalize_k    partials per lane the finalize launch really adds (ceil(nchunk / 64) of its 8 clamped loads)
      half_apply    the half-length apply pass (SiLU, N nchunk < 1024, ppb >= 2 PP)
      table         the SiLU-table apply pass; then PPa, gx (blocks per image) and chunks_per_block (max)."""
    g = gn_geom(N, HW, C, G)
    if g is None:
        return None
    g = dict(g, silu=bool(silu))
    g["stats_iters"] = g["ppb"] // g["PP"]
    g["unroll"] = stats_unroll if stats_unroll in (1, 2, 4) else (2 if g["stats_iters"] <= 2 else 4)
    g["finalize"] = "self" if g["nchunk"] <= SELF_FINALIZE_MAX else "launch"
    g["nfull"] = g["threads"] >> 6
    g["whole_waves"] = g["threads"] % 64 == 0
    g["self_branch"] = None if g["finalize"] == "launch" else ("pair" if G <= 2 * g["nfull"] else "loop")
    g["finalize_k"] = cdiv(g["nchunk"], 64)
    ppb_apply, nchunk_apply = g["ppb"], g["nchunk"]
    g["half_apply"] = bool(silu and N * g["nchunk"] < 1024 and g["ppb"] >= 2 * g["PP"])
    if g["half_apply"]:
        ppb_apply = (g["ppb"] // 2 // g["PP"]) * g["PP"]
        nchunk_apply = cdiv(HW, ppb_apply)
    g["table"] = bool(silu and g["finalize"] == "launch" and tab_mode != 0 and
                      (tab_mode == 1 or N * HW * C >= TAB_MIN))
    g["PPa"], g["gx"], g["chunks_per_block"] = g["PP"], nchunk_apply, 1
    if g["table"]:
        iters = ppb_apply // g["PP"]
        g["PPa"] = 1 if g["OC"] >= 512 else 512 // g["OC"]
        ppb_apply = iters * g["PPa"]
        nchunk_apply = cdiv(HW, ppb_apply)
        g["gx"] = max(1, min(cdiv(2 * NUM_CU, N), nchunk_apply))
        g["chunks_per_block"] = cdiv(nchunk_apply, g["gx"])
    g["ppb_apply"], g["nchunk_apply"] = ppb_apply, nchunk_apply
    return g


def _gn(name, N, HW, C, G, silu, C1=None, eps=1e-5):
    c = dict(name=name, N=N, HW=HW, C=C, G=G, silu=silu, C1=C if C1 is None else C1, eps=eps)
    c["geom"] = gn_launch(N, HW, C, G, silu)
    c["geom_tab"] = gn_launch(N, HW, C, G, silu, tab_mode=1)          # under MIXDQ_GN_SILU_TAB=1
    assert c["geom"] is not None, name
    assert N * HW * C <= ELEMENT_CAP, name
    if c["C1"] != C:
        c["split"] = "boundary" if c["C1"] % c["geom"]["cg"] == 0 else "inside"
    return c


def gn_cases():
    out = []
    for i, HW in enumerate((1, 31, 32, 33, 2048, 2080, 4128, 16384, 16385)):      # PP = 32
        out.append(_gn(f"c64_hw{HW}", 3 if HW in (33, 16384) else 1, HW, 64, 8, i % 2 == 0))
    for i, HW in enumerate((5, 6, 7, 384, 390)):                                  # cg = 10, 240 threads
        out.append(_gn(f"c320_hw{HW}", 3 if HW == 7 else 1, HW, 320, 32, i % 2 == 1))
    out.append(_gn("c320_hw4224_n3", 3, 4224, 320, 32, True))                     # table blocks walk two chunks
    out.append(_gn("c32_cg4", 1, 70, 32, 8, True))
    out.append(_gn("c96_cg12", 3, 43, 96, 8, False))
    for C in (960, 1920):
        for i, HW in enumerate((1, 3, 130)):
            out.append(_gn(f"c{C}_hw{HW}", 1, HW, C, 32, (i + C // 960) % 2 == 0))
    out.append(_gn("c1280_hw9", 1, 9, 1280, 32, True))                            # 160 threads, self-finalize loop
    out.append(_gn("c1280_hw1025", 1, 1025, 1280, 32, False))                     # three iterations: unroll 4, clamped
    for HW in (1, 64, 65):
        out.append(_gn(f"c2560_hw{HW}", 1, HW, 2560, 32, HW != 64))
    out.append(_gn("c2560_hw513_n3", 3, 513, 2560, 32, True))                     # half-length + table, 3 chunks a block
    for HW in (1, 65):
        out.append(_gn(f"c8192_hw{HW}", 1, HW, 8192, 32, HW == 65))
    out.append(_gn("c2048_g256", 1, 5, 2048, 256, True))                          # G == threads
    # two sources: C1 inside a group and on a group boundary
    out.append(_gn("c96_split8", 1, 43, 96, 8, True, C1=8))
    out.append(_gn("c96_split24", 3, 43, 96, 8, False, C1=24))
    out.append(_gn("c320_split168", 1, 390, 320, 32, True, C1=168))
    out.append(_gn("c320_split160", 1, 7, 320, 32, False, C1=160))
    # the VAE's widths (mixdq_amd.vae: 32 groups, eps 1e-6), SiLU and plain, at both eps.  C = 128: groups of 4 channels,
    # every octet straddles two, 32 reducing threads of 256; HW = 16384 is 2 Mi elements (the table pass by the size
    # rule) in 512 chunks.  C = 512 at HW = 8192 is the 4 Mi element cap, 512 chunks again.
    for eps in VAE_EPS:
        for silu in (True, False):
            out.append(_gn("vae_c128_hw70", 1, 70, 128, 32, silu, eps=eps))
            out.append(_gn("vae_c128_hw16384", 1, 16384, 128, 32, silu, eps=eps))
            out.append(_gn("vae_c256_hw1040", 2, 1040, 256, 32, silu, eps=eps))      # 130 chunks: the finalize launch
            out.append(_gn("vae_c512_hw8192", 1, 8192, 512, 32, silu, eps=eps))
    return out


GN_REFUSED = [(1, 16, 8200, 8), (1, 16, 2048, 512), (1, 16, 36, 6)]     # OC > 1024; G > threads; C % 8


def gn_id(c):
    return f"{c['name']}_n{c['N']}_{'silu' if c['silu'] else 'plain'}" + ("" if c["eps"] == 1e-5 else f"_eps{c['eps']:g}")


def gn_inputs(c, seed=0):
    """x [N, HW, C] FP16 (Gaussian, per-channel offsets), gamma, beta, and the quantizer (scale_inv, zero_point)."""
    N, HW, C = c["N"], c["HW"], c["C"]
    s = 1000 + seed + 7 * HW + C
    x = (dd.normal_f16(s, (N, HW, C), 1.5).astype(np.float32) +
         dd.normal_f16(s + 1, (1, 1, C), 0.7).astype(np.float32)).astype(np.float16)
    gamma = (dd.normal_f16(s + 2, (C,), 0.3).astype(np.float32) + 1).astype(np.float16)
    beta = dd.normal_f16(s + 3, (C,), 0.2)
    return x, gamma, beta, (float(np.float32(1) / np.float32(0.031)), -20.0)


# ------------------------------------------------------------------------------------------------ LayerNorm
def ln_geom(M, C):
    """ln_quant_kernel / mixdq_layernorm_quantize: None where refused."""
    if C <= 0 or C % 16 or C // 8 > 64 * LN_MAX_CHUNKS:
        return None
    G = C // 16
    U = 1
    while U < 16 and G % (2 * U) == 0:
        U *= 2
    nch = C // 8
    return dict(M=M, C=C, G=G, U=U, per=G // U, nch=nch, chunks_per_lane=cdiv(nch, 64),
                partial_last_chunk=nch % 64 != 0, rows_per_wave=2 if M >= 8192 else 1,
                odd_tail=M >= 8192 and M % 2 == 1)


LN_WIDTHS = (16, 32, 48, 96, 160, 320, 512, 960, 1024, 1168, 1536, 1920, 2032, 2048)   # (1168: three chunks, the last partial)
LN_REFUSED = (24, 2064)


def ln_cases():
    out = []
    for i, C in enumerate(LN_WIDTHS):
        for j, M in enumerate((1, 3, 4, 5)):
            out.append(dict(M=M, C=C, nq=(i + j) % 4, geom=ln_geom(M, C)))
    for C in (16, 320):
        for M in (8192, 8193):
            out.append(dict(M=M, C=C, nq=1 + (M + C // 16) % 3, geom=ln_geom(M, C)))
    assert all(c["geom"] is not None and c["M"] * c["C"] <= ELEMENT_CAP for c in out)
    return out


def ln_id(c):
    return f"m{c['M']}_c{c['C']}_q{c['nq']}"


def ln_inputs(M, C, seed=0):
    s = 2000 + seed + 3 * M + C
    x = (dd.normal_f16(s, (M, C), 1.2).astype(np.float32) + 0.4).astype(np.float16)
    gamma = (dd.normal_f16(s + 1, (C,), 0.3).astype(np.float32) + 1).astype(np.float16)
    beta = dd.normal_f16(s + 2, (C,), 0.2)
    return x, gamma, beta


def ln_qparams(nq):
    return [(float(np.float32(1) / np.float32(0.02 + 0.01 * i)), float(-7 + 11 * i)) for i in range(nq)]


# ------------------------------------------------------------------------------------------------ GEGLU
def geglu_geom(M, D, tab_mode=-1):
    """mixdq_geglu_quantize: the kernel, its grid and how many 8-element pieces a thread walks at most."""
    if D <= 0 or D % 8:
        return None
    total = M * (D // 8)
    table = tab_mode != 0 and (tab_mode == 1 or M * D >= TAB_MIN)
    block = 1024 if table else 256
    blocks = min(cdiv(total, block), 2 * NUM_CU if table else 8 * NUM_CU)
    stride = blocks * block
    return dict(M=M, D=D, total=total, table=table, block=block, blocks=blocks, stride=stride,
                pieces_per_thread=cdiv(total, stride), capped=cdiv(total, block) > blocks,
                odd_octets=(D // 8) % 2 == 1, stride_splits_rows=stride % (D // 8) != 0)


GEGLU_SHAPES = [(1, 8), (3, 24), (5, 8 * 127), (257, 40), (174771, 24)]


def geglu_cases():
    out = [dict(M=M, D=D, geom=geglu_geom(M, D), geom_tab=geglu_geom(M, D, 1)) for M, D in GEGLU_SHAPES]
    assert all(c["M"] * c["D"] <= ELEMENT_CAP + (1 << 16) for c in out)     # (the capped grid needs > 4 Mi outputs)
    return out


def geglu_id(c):
    return f"m{c['M']}_d{c['D']}"


def geglu_inputs(M, D, seed=0):
    return dd.normal_f16(3000 + seed + M + D, (M, 2 * D), 2.0)


# ------------------------------------------------------------------------------- LayerNorm in the GEMM launch
LN_GEMM_WIDTHS = (320, 160, 80)
LN_GEMM_ROW_TILE = {56: 64, 45: 64, 44: 128}       # csrc/igemm_ln.hip: BM of the tiles select_ln returns


def ln_gemm_cases(select_id):
    """For N in {320, 160, 80}: the smallest (K, M) the library's select rule (`select_id(M, N, K)`, asked -- not
    restated) returns a tile for, and one M that leaves a ragged last row tile; where it accepts nothing (K up to
    2048, M up to 256), one case with cfg = None: the GPU test asserts qlinear_ln_supported is false there."""
    out = []
    for N in LN_GEMM_WIDTHS:
        found = next(((M, K) for K in range(16, 2049, 16) for M in (1, 2, 4, 8, 16, 32, 64, 128, 256)
                      if select_id(M, N, K) > 0), None)
        if found is None:
            out.append(dict(M=64, N=N, K=128, cfg=None, ragged=False))
            continue
        M, K = found
        cfg = select_id(M, N, K)
        out.append(dict(M=M, N=N, K=K, cfg=cfg, ragged=M % LN_GEMM_ROW_TILE[cfg] != 0))
        Mr = LN_GEMM_ROW_TILE[cfg] + 13                      # two row tiles, the second with 13 rows
        if select_id(Mr, N, K) > 0:
            out.append(dict(M=Mr, N=N, K=K, cfg=select_id(Mr, N, K), ragged=True))
    return out


def ln_gemm_id(c):
    return f"m{c['M']}_n{c['N']}_k{c['K']}_cfg{c['cfg']}"


# ------------------------------------------------------------------------------------------------ references
def ulp16(x):
    """Spacing of the FP16 numbers at |x| (float64; 2^-24 below 2^-14)."""
    m, e = np.frexp(np.abs(np.asarray(x, np.float64)))
    return np.exp2(np.where(m == 0, -14, np.maximum(e - 1, -14)).astype(np.float64) - 10)


def groupnorm64(x, gamma, beta, eps, G):
    """The definition, float64, two passes (neither the oracle nor the kernel's order): x [N, HW, C]."""
    N, HW, C = x.shape
    v = x.astype(np.float64).reshape(N, HW, G, C // G)
    mean = v.mean(axis=(1, 3), keepdims=True)
    var = ((v - mean) ** 2).mean(axis=(1, 3), keepdims=True)
    y = ((v - mean) / np.sqrt(var + eps)).reshape(N, HW, C)
    return y * gamma.astype(np.float64) + beta.astype(np.float64)


def layernorm64(x, gamma, beta, eps):
    v = x.astype(np.float64)
    mean = v.mean(axis=-1, keepdims=True)
    var = ((v - mean) ** 2).mean(axis=-1, keepdims=True)
    return (v - mean) / np.sqrt(var + eps) * gamma.astype(np.float64) + beta.astype(np.float64)


def silu64(y):
    y = np.asarray(y, np.float64)
    return y / (1.0 + np.exp(-y))


def geglu64(h):
    """y = fp16(x * fp16(gelu(gate))) in float64 with the two FP16 roundings: [M, 2D] -> [M, D] float64 before the
    last rounding, and the FP16 GELU value."""
    from math import erf
    D = h.shape[-1] // 2
    x = h[..., :D].astype(np.float64)
    bits, inv = np.unique(np.ascontiguousarray(h[..., D:]).view(np.uint16), return_inverse=True)   # <= 65536 gates
    g = bits.view(np.float16).astype(np.float64)
    ge = (0.5 * g * (1.0 + np.array([erf(v / 2.0 ** 0.5) for v in g]))).astype(np.float16)
    return x * ge.astype(np.float64)[inv].reshape(x.shape)


def within_geglu_bound(got16, h):
    """|got - fp16(ref)| <= 2.001 ulp16 + 4e-7 |x| max(|gate|, 1): a 1-ulp difference of the FP16 GELU value, times x,
    rounded again; for gate << 0, 1 + erf cancels and any FP32 erf carries ~1e-7 |gate| of absolute error -- the
    bound of tests/test_fused_gpu.py."""
    D = h.shape[-1] // 2
    ref16 = geglu64(h).astype(np.float16).astype(np.float64)
    atol = 4e-7 * np.abs(h[..., :D].astype(np.float64)) * np.maximum(np.abs(h[..., D:].astype(np.float64)), 1.0)
    return np.abs(np.asarray(got16).astype(np.float64) - ref16) <= 2.001 * ulp16(ref16) + atol


def within_norm_bound(got16, ref64):
    """|got - fp16(ref)| <= 1.001 ulp16(fp16(ref)) + 2e-6 (one FP16 rounding point; + 2e-6: where a x + b cancels to
    ~0 the FP32 rounding of its O(1) terms exceeds an FP16 ulp) -- the bound of tests/test_fused_gpu.py."""
    ref16 = np.asarray(ref64).astype(np.float16).astype(np.float64)
    err = np.abs(np.asarray(got16).astype(np.float64) - ref16)
    return err <= 1.001 * ulp16(ref16) + 2e-6
