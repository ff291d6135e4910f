"""Edge-case generator of the INT8 / FP16 GEMM tile configurations (tests/test_tile_edges_gpu.py runs the
cases, tests/test_tile_edges_host.py checks on the CPU that they cover every configuration's edges).

Every case is derived from a configuration's own (BM, BN, BK, STAGES), read from the X-macro tables of
csrc/igemm.hip and csrc/igemm_aq.hip -- the tables the library is compiled from -- so that a configuration
added there is covered without a hand-written shape.  The edges of a tiled, software-pipelined kernel:

  K-tile count nk in {1, 2, STAGES - 1, STAGES, STAGES + 1} (fewer K-tiles than stages: the prologue stages
  tiles past the end of K), each as K = nk * BK and as a ragged K = nk * BK - 16;
  M in {1, BM - 1, BM, BM + 1, 2 * BM + 1};  N in {4, BN - 4, BN, BN + 4, 2 * BN + 4} (N % 8 == 4 included).

The values are covered, not multiplied: case i takes the i-th K and cycles M and N with co-prime steps.
Imports without a GPU and without the built library.
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mixdq_amd", "csrc")


def _xmacro(path, name):
    """{id: (params...)} of `#define name(X) X(id, ...) ...` in a source file."""
    text = open(path).read()
    m = re.search(r"#define\s+" + name + r"\(X\)(.*?)\n(?!\s*X\()", text + "\n", flags=re.S)
    assert m, f"{name} not found in {path}"
    rows = {}
    for args in re.findall(r"X\(([^)]*)\)", m.group(1)):
        vals = [v.strip() for v in args.split(",")]
        nums = tuple(int(v) for v in vals if re.fullmatch(r"-?\d+", v))
        rows[nums[0]] = nums[1:]
    return rows


def _tables():
    ig = _xmacro(os.path.join(CSRC, "igemm.hip"), "MIXDQ_IGEMM_CONFIGS")
    return dict(
        # id -> (BM, BN, BK, STAGES, WM, WN, KSPLIT, MT)
        igemm={i: v[:8] for i, v in ig.items()},
        f16=_xmacro(os.path.join(CSRC, "igemm.hip"), "MIXDQ_F16_CONFIGS"),
        grouped=_xmacro(os.path.join(CSRC, "igemm.hip"), "MIXDQ_GROUPED_CONFIGS"),
        aq=_xmacro(os.path.join(CSRC, "igemm_aq.hip"), "MIXDQ_AQ_CONFIGS"),
    )


TABLES = _tables()
IGEMM = TABLES["igemm"]                 # id -> (BM, BN, BK, STAGES, WM, WN, KSPLIT, MT)
F16 = TABLES["f16"]
GROUPED = TABLES["grouped"]
AQ = TABLES["aq"]


def tile(cfg, table=None):
    """(BM, BN, BK, STAGES) of a configuration."""
    return tuple((table or IGEMM)[cfg][:4])


def w2_admissible(cfg):
    """csrc/igemm.hip w2_tile_ok: the weight stage is whole 1-KiB pieces at a quarter of the bytes, not tile 27."""
    bm, bn, bk, st = tile(cfg)
    return (bn * bk // 4) % 1024 == 0 and cfg != 27


def geglu_admissible(cfg):
    """csrc/igemm_kernel.h launch_kernel: whole 32-column value|gate groups per tile and per wave."""
    bm, bn, bk, st, wm, wn, ks, mt = IGEMM[cfg]
    return bn % 32 == 0 and (bn // wn) % 32 == 0


def aq_depth(cfg):
    """AD of csrc/igemm_kernel.h: K-tiles of raw FP16 activations an AQ kernel keeps in flight."""
    return max(tile(cfg)[3] - 1, 2)


def nk_values(stages):
    return sorted({1, 2, max(stages - 1, 1), stages, stages + 1})


def m_edges(bm):
    return [1, bm - 1, bm, bm + 1, 2 * bm + 1]


def n_edges(bn, step=4):
    """N edges in units of `step` columns (4: the output quads; 32: whole GEGLU value|gate groups)."""
    return sorted({step, bn - step, bn, bn + step, 2 * bn + step} - {0})


def k_values(bk, nks, ragged=True):
    """[(nk, K)]: K = nk * BK, and the ragged K = nk * BK - 16 where that is >= 16."""
    out = []
    for nk in nks:
        out.append((nk, nk * bk))
        if ragged and nk * bk - 16 >= 16:
            out.append((nk, nk * bk - 16))
    return out


def _cover(ks, ms, ns):
    """Cases (M, N, nk, K) in which every K, M and N value occurs at least once."""
    n = max(len(ks), len(ms), len(ns))
    step = 2 if len(ns) % 2 else 1          # co-prime with len(ns): every N value is reached
    return [(ms[i % len(ms)], ns[(step * i + 1) % len(ns)], *ks[i % len(ks)]) for i in range(n)]


def linear_cases(cfg):
    """Linear problems of one INT8 configuration: dicts with M, N, K, nk, bias and the forms to also run
    (w4, w2 -- False where the configuration refuses them --, residual, rowmap)."""
    bm, bn, bk, st = tile(cfg)
    out = []
    for i, (M, N, nk, K) in enumerate(_cover(k_values(bk, nk_values(st)), m_edges(bm), n_edges(bn))):
        out.append(dict(cfg=cfg, M=M, N=N, K=K, nk=nk, bias=i % 2 == 0, w4=K % 32 == 0,
                        w2=K % 64 == 0, residual=i % 3 == 1, rowmap=i % 3 == 2))
    return out


def linear_id(c):
    return f"cfg{c['cfg']}_m{c['M']}_n{c['N']}_k{c['K']}_{'bias' if c['bias'] else 'nobias'}"


# conv: (batch, H, W, C, Kout, R, stride, pad) -- taps straddled by BK = 128 K-tiles (C = 320, 960), short K
# (C = 16 / 48: K = 144 / 48), pad 0 (the plain bias0 path) and 1 (the border table), 1x1, odd H and W; Kout
# puts an N tail into the second N tile.
def conv_cases(cfg):
    bm, bn, bk, st = tile(cfg)
    return [
        dict(cfg=cfg, n=2, H=7, W=9, C=16, K=bn + 4, R=3, stride=1, pad=1),
        dict(cfg=cfg, n=1, H=9, W=11, C=48, K=bn + 8, R=3, stride=2, pad=0),
        dict(cfg=cfg, n=1, H=5, W=7, C=48, K=2 * bn - 4, R=1, stride=1, pad=0),
        dict(cfg=cfg, n=2, H=5, W=7, C=320, K=bn + 4, R=3, stride=1, pad=1),
        dict(cfg=cfg, n=1, H=7, W=5, C=320, K=bn + 12, R=1, stride=2, pad=0),
        dict(cfg=cfg, n=1, H=5, W=5, C=960, K=bn + 4, R=3, stride=2, pad=1),
        dict(cfg=cfg, n=1, H=5, W=3, C=960, K=2 * bn - 4, R=3, stride=1, pad=0),
    ]


def conv_id(c):
    return (f"cfg{c['cfg']}_n{c['n']}_{c['H']}x{c['W']}_c{c['C']}_k{c['K']}_r{c['R']}"
            f"_s{c['stride']}_p{c['pad']}")


def geglu_cases(cfg):
    """GEMM + GEGLU (N = 2D in whole 32-column value|gate groups) at nk in {1, 2, STAGES}."""
    bm, bn, bk, st = tile(cfg)
    ks = [(nk, nk * bk) for nk in sorted({1, 2, st})]
    return [dict(cfg=cfg, M=M, N=N, K=K, nk=nk, bias=i % 2 == 0)
            for i, (M, N, nk, K) in enumerate(_cover(ks, m_edges(bm), n_edges(bn, 32)))]


def geglu_id(c):
    return f"cfg{c['cfg']}_m{c['M']}_n{c['N']}_k{c['K']}_{'bias' if c['bias'] else 'nobias'}"


def pp_cases():
    """Configuration 71 (persistent 256x256) at the 256 grid edges: (M, N, K, output form).  N % 8 == 4 and
    K < 256 are outside pp_ok: the launch runs 70's kernel there."""
    return [
        dict(M=255, N=248, K=256, form="f16", bias=True),
        dict(M=256, N=264, K=384, form="residual", bias=False),
        dict(M=257, N=504, K=256, form="f16", bias=False),
        dict(M=511, N=544, K=384, form="geglu", bias=True),     # (GEGLU: whole 32-column groups)
        dict(M=512, N=248, K=256, form="residual", bias=True),
        dict(M=513, N=264, K=640, form="f16", bias=True),
        dict(M=257, N=256, K=512, form="geglu", bias=False),
        dict(M=300, N=260, K=384, form="f16", bias=True),       # N % 8 == 4
        dict(M=513, N=516, K=256, form="residual", bias=False),  # N % 8 == 4
        dict(M=257, N=264, K=128, form="f16", bias=True),       # one K-tile
        dict(M=255, N=224, K=128, form="geglu", bias=True),
    ]


def pp_id(c):
    return f"m{c['M']}_n{c['N']}_k{c['K']}_{c['form']}_{'bias' if c['bias'] else 'nobias'}"


def f16in_cases(cfg):
    """Quantize-in-prologue (AQ) launches at nk in {1, 2, AD, AD + 1}; K = nk * BK only (the AQ family refuses
    K tails: MIXDQ_ERR_SHAPE)."""
    bm, bn, bk, st = tile(cfg, AQ)
    ad = aq_depth(cfg)
    ks = [(nk, nk * bk) for nk in sorted({1, 2, ad, ad + 1})]
    return [dict(cfg=cfg, M=M, N=N, K=K, nk=nk, bias=i % 2 == 0)
            for i, (M, N, nk, K) in enumerate(_cover(ks, m_edges(bm), n_edges(bn)))]


def f16in_id(c):
    return f"cfg{c['cfg']}_m{c['M']}_n{c['N']}_k{c['K']}_{'bias' if c['bias'] else 'nobias'}"


def f16_cases(cfg):
    """FP16 layer launches: K counts bytes in the tile table (2 per element), so nk K-tiles are nk * BK / 2
    elements; ragged K one 16-byte piece short."""
    bm, bn, bk, st = tile(cfg, F16)
    ks = [(nk, kb // 2) for nk, kb in k_values(bk, nk_values(st))]
    return [dict(cfg=cfg, M=M, N=N, K=K, nk=nk, bias=i % 2 == 0)
            for i, (M, N, nk, K) in enumerate(_cover(ks, m_edges(bm), n_edges(bn)))]


def f16_id(c):
    return f"cfg{c['cfg']}_m{c['M']}_n{c['N']}_k{c['K']}_{'bias' if c['bias'] else 'nobias'}"


def grouped_cases(cfg):
    """Grouped launches: members whose N hit BN - 4, BN and BN + 4, at nk = 1 and STAGES."""
    bm, bn, bk, st = tile(cfg, GROUPED)
    return [dict(cfg=cfg, M=M, K=nk * bk, nk=nk, Ns=[bn - 4, bn, bn + 4]) for M, nk in ((bm + 1, 1), (1, st))]


def grouped_id(c):
    return f"cfg{c['cfg']}_m{c['M']}_k{c['K']}_n{'-'.join(str(n) for n in c['Ns'])}"


def all_linear():
    return [c for cfg in sorted(IGEMM) for c in linear_cases(cfg)]


def all_conv():
    return [c for cfg in sorted(IGEMM) for c in conv_cases(cfg)]


def all_geglu():
    return [c for cfg in sorted(IGEMM) if geglu_admissible(cfg) for c in geglu_cases(cfg)]


def all_f16in():
    return [c for cfg in sorted(AQ) for c in f16in_cases(cfg)]


def all_f16():
    return [c for cfg in sorted(F16) for c in f16_cases(cfg)]


def all_grouped():
    return [c for cfg in sorted(GROUPED) for c in grouped_cases(cfg)]
