#!/usr/bin/env python3
"""Micro-benchmark of the INT8 GEMM / conv kernel configurations on the dominant SDXL shapes
(SURVEY.md Appendix A).  Runs on the GPU box:  python tools/bench_gemm.py [--conv] [--bs B]

For every shape x configuration: checks the result bit-for-bit against configuration 1 and
reports the mean kernel time over a hipGraph of back-to-back launches (HIP events).

--halo-w4: the packed-W4 3x3 / stride-1 convs of the SDXL UNet (every shape, 1024 px) on the implicit-GEMM
family's automatic W4 tile (what MIXDQ_HALO_W4=0 runs: the tool sets it, so `_cfg=0` is that launch) against
each LDS-halo tile (forced ids 90 .. 93, which the switch does not touch), with the W8 halo launch of the same
shape beside it (rule_tile: the W4 rule's choice, 0 = implicit GEMM; w8_tile: the int8 rule's); --repeats whole
tables, one JSON line per shape and repeat, then the run-to-run spread."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mixdq_amd._C as C  # noqa: E402

DEV = "cuda:0"
LINEAR = [  # (count per 1024px image, M per image, N, K)
    (372, 1024, 1280, 1280), (60, 1024, 10240, 1280), (60, 1024, 1280, 5120),
    (70, 4096, 640, 640), (10, 4096, 5120, 640), (10, 4096, 640, 2560),
    (120, 77, 1280, 2048), (20, 77, 640, 2048), (17, 1, 1280, 1280),
    (60, 1024, 3840, 1280), (10, 4096, 1920, 640), (60, 77, 2560, 2048),   # fused q|k|v, k|v
]
CONV = [  # (count, H=W, Cin, Cout, ksize, stride)
    (10, 32, 1280, 1280, 3, 1), (7, 128, 320, 320, 3, 1), (6, 64, 640, 640, 3, 1),
    (2, 32, 2560, 1280, 3, 1), (1, 64, 1280, 1280, 3, 1), (1, 128, 640, 640, 3, 1),
    (2, 128, 640, 320, 3, 1), (1, 64, 1920, 640, 3, 1), (1, 128, 960, 320, 3, 1),
    (3, 32, 1280, 1280, 1, 1),
]


# (count, H=W, Cin, Cout): every 3x3 / stride 1 / pad 1 conv of the SDXL UNet at 1024 px with C % 64 == 0 (37 of 38:
# conv_in has 4 input channels)
CONV3X3 = [(7, 128, 320, 320), (2, 128, 640, 320), (1, 128, 960, 320), (1, 128, 640, 640), (1, 128, 320, 4),
           (1, 64, 320, 640), (6, 64, 640, 640), (1, 64, 960, 640), (1, 64, 1280, 640), (1, 64, 1920, 640),
           (1, 64, 1280, 1280), (1, 32, 640, 1280), (10, 32, 1280, 1280), (1, 32, 1920, 1280), (2, 32, 2560, 1280)]


def timeit_median(fn, iters=20, reps=5):
    """us per launch: `iters` launches in one captured graph, median of `reps` replays."""
    import statistics
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / iters)
    return statistics.median(out)


def _w4_rule_tiles(shapes):
    """The shipped W4 rule for (bs, hw, cin, cout) shapes: asked in a child process without the A/B switches, since this
    process runs with MIXDQ_HALO_W4=0 and the library reads its switches once (host code only: the child opens no GPU)."""
    import subprocess
    code = ("import ctypes, json, sys; from mixdq_amd.build import build; lib = ctypes.CDLL(build()); "
            "f = lib.mixdq_conv_halo_select_flags; f.argtypes = [ctypes.c_int] * 10; "
            "print('TILES', json.dumps([f(b, hw, hw, ci, co, 3, 3, 1, 1, 2) for b, hw, ci, co in json.loads(sys.argv[1])]))")
    env = {k: v for k, v in os.environ.items() if k not in ("MIXDQ_HALO_W4", "MIXDQ_HALO_CONV")}
    r = subprocess.run([sys.executable, "-c", code, json.dumps(shapes)], env=env, capture_output=True, text=True,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), check=True)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("TILES ")][-1]
    return json.loads(line[6:])


def halo_w4(batches, repeats):
    from mixdq_amd.nn.utils import pack_w4
    rule = dict(zip([(bs, hw, cin, cout) for bs in batches for _, hw, cin, cout in CONV3X3],
                    _w4_rule_tiles([(bs, hw, cin, cout) for bs in batches for _, hw, cin, cout in CONV3X3])))
    g = torch.Generator(device="cpu").manual_seed(0)
    zero = torch.zeros((), device=DEV)
    cases = []
    for bs in batches:
        for cnt, hw, cin, cout in CONV3X3:
            x = torch.randint(-128, 128, (bs, cin, hw, hw), generator=g, dtype=torch.int8
                              ).to(DEV).contiguous(memory_format=torch.channels_last)
            q = torch.randint(-8, 8, (cout, 3, 3, cin), generator=g, dtype=torch.int8)
            w8 = q.to(DEV).permute(0, 3, 1, 2)                       # [K, C, 3, 3] channels-last
            w4 = pack_w4(q).to(DEV).permute(0, 3, 1, 2)
            wsum = w8.float().sum(dim=1, keepdim=True)
            table = C.conv_border_table(wsum)
            sc = torch.rand(cout, generator=g).to(DEV) * 1e-4
            bias = torch.rand(cout, generator=g).half().to(DEV)

            def run(cfg, packed, x=x, w8=w8, w4=w4, sc=sc, wsum=wsum, bias=bias, table=table):
                return C.qconv2d_w8_a8_ohalf(x, w4 if packed else w8, sc, zero, zero, sc, wsum, None, bias, 1, 1, 1,
                                             _table=table, _cfg=cfg, _w4=packed)
            ref = run(0, True)                                       # implicit GEMM (MIXDQ_HALO_W4=0)
            tiles = {}
            for tile in (90, 91, 92, 93):
                try:
                    tiles[tile] = bool(torch.equal(run(tile, True), ref))
                except RuntimeError:
                    pass
            assert all(tiles.values()), (hw, cin, cout, tiles)
            assert torch.equal(run(0, False), ref)
            M = bs * hw * hw
            cases.append(dict(shape=f"conv {hw}x{hw} {cin}->{cout} k3", bs=bs, count=cnt, run=run, tiles=sorted(tiles),
                              igemm_cfg=C.igemm_select_id(M, cout, cin, 9 * cin, w4=True),
                              rule_tile=rule[(bs, hw, cin, cout)],      # the W4 rule; 0 = implicit GEMM
                              w8_tile=C.conv_halo_select(bs, hw, hw, cin, cout, 3, 3, 1, 1)))
    for _ in range(2):                  # clocks and caches settled before the first figure (the first row of a cold
        for c in cases:                 # process read 15 % high in its first repeat): every launch that is timed
            for cfg, packed in [(0, True), (0, False)] + [(t, True) for t in c["tiles"]]:
                for _ in range(5):
                    c["run"](cfg, packed)
    torch.cuda.synchronize()
    rows = {}
    for rep in range(repeats):
        for i, c in enumerate(cases):
            run = c["run"]
            row = dict(repeat=rep, shape=c["shape"], bs=c["bs"], count=c["count"], igemm_cfg=c["igemm_cfg"],
                       rule_tile=c["rule_tile"], w8_tile=c["w8_tile"],
                       w4_igemm_us=round(timeit_median(lambda: run(0, True)), 2),
                       w4_halo_us={t: round(timeit_median(lambda: run(t, True)), 2) for t in c["tiles"]},
                       w8_halo_us=round(timeit_median(lambda: run(0, False)), 2))
            rows.setdefault(i, []).append(row)
            print(json.dumps(row), flush=True)
    spread = 0.0
    for i, rs in rows.items():
        series = [[r["w4_igemm_us"] for r in rs], [r["w8_halo_us"] for r in rs]]
        series += [[r["w4_halo_us"][t] for r in rs] for t in rs[0]["w4_halo_us"]]
        for s in series:
            spread = max(spread, (max(s) - min(s)) / min(s))
    print(json.dumps(dict(run_to_run_spread=round(spread, 4),
                          note="largest (max - min) / min of one figure over the repeats")), flush=True)
    for bs in batches:
        tot = dict(igemm=0.0, rule=0.0, best=0.0, w8=0.0)
        for i, rs in rows.items():
            if rs[0]["bs"] != bs:
                continue
            med = lambda xs: sorted(xs)[len(xs) // 2]
            tot["igemm"] += rs[0]["count"] * med([r["w4_igemm_us"] for r in rs])
            rt = rs[0]["rule_tile"]          # what the library runs: the rule's halo tile, or the implicit GEMM
            tot["rule"] += rs[0]["count"] * med([r["w4_halo_us"][rt] if rt else r["w4_igemm_us"] for r in rs])
            tot["best"] += rs[0]["count"] * min(med([r["w4_halo_us"][t] for r in rs]) for t in rs[0]["w4_halo_us"])
            tot["w8"] += rs[0]["count"] * med([r["w8_halo_us"] for r in rs])
        print(json.dumps(dict(bs=bs, all_convs_of_a_step_ms={k: round(v / 1e3, 3) for k, v in tot.items()})), flush=True)


def timeit(fn, iters=20):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e9
    for _ in range(3):
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / iters)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=1)
    ap.add_argument("--conv", action="store_true")
    ap.add_argument("--cfgs", default="")
    ap.add_argument("--w4", action="store_true", help="packed 4-bit weights (MIXDQ_FLAG_W4)")
    ap.add_argument("--halo-w4", action="store_true", help="W4 3x3 convs: implicit GEMM against every halo tile")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batches", default="1,8")
    args = ap.parse_args()
    if args.halo_w4:
        os.environ["MIXDQ_HALO_W4"] = "0"        # read by the library at its first conv launch: `_cfg=0` = implicit GEMM
        halo_w4([int(b) for b in args.batches.split(",")], args.repeats)
        return
    cfgs = [int(c) for c in args.cfgs.split(",")] if args.cfgs else sorted(C.IGEMM_CONFIGS)
    g = torch.Generator(device="cpu").manual_seed(0)
    zero = torch.zeros((), device=DEV)
    results = []
    shapes = CONV if args.conv else LINEAR
    for shp in shapes:
        if args.conv:
            cnt, hw, cin, cout, ks, stride = shp
            x = torch.randint(-128, 128, (args.bs, cin, hw, hw), generator=g, dtype=torch.int8
                              ).to(DEV).contiguous(memory_format=torch.channels_last)
            w = torch.randint(-128, 128, (cout, cin, ks, ks), generator=g, dtype=torch.int8
                              ).to(DEV).contiguous(memory_format=torch.channels_last)
            pad = ks // 2
            wsum = w.float().sum(dim=1, keepdim=True)
            if args.w4:
                from mixdq_amd.nn.utils import pack_w4
                w = pack_w4((w >> 4).permute(0, 2, 3, 1).contiguous()).permute(0, 3, 1, 2)
            table = C.conv_border_table(wsum) if pad else None
            b0 = None if pad else w.float().sum(dim=[1, 2, 3])
            sc = torch.rand(cout, generator=g).to(DEV) * 1e-4
            bias = torch.rand(cout, generator=g).half().to(DEV)
            ops = 2.0 * args.bs * (hw // stride) ** 2 * cout * cin * ks * ks

            def run(cfg):
                return C.qconv2d_w8_a8_ohalf(x, w, sc, zero, zero, sc, wsum if pad else None, b0,
                                             bias, stride, pad, 1, _table=table, _cfg=cfg,
                                             _w4=args.w4)
            label = f"conv {hw}x{hw} {cin}->{cout} k{ks}"
        else:
            cnt, M, N, K = shp
            M *= args.bs
            a = torch.randint(-128, 128, (M, K), generator=g, dtype=torch.int8).to(DEV)
            w = torch.randint(-128, 128, (N, K), generator=g, dtype=torch.int8).to(DEV)
            if args.w4:
                from mixdq_amd.nn.utils import pack_w4
                w = pack_w4(w >> 4)
            sc = torch.rand(N, generator=g).to(DEV) * 1e-4
            b0 = torch.rand(N, generator=g).to(DEV) * 100
            bias = torch.rand(N, generator=g).half().to(DEV)
            ops = 2.0 * M * N * K

            def run(cfg):
                return C.qlinear_w8_a8_ohalf(a, w, sc, zero, zero, b0, sc, b0, bias, _cfg=cfg,
                                             _w4=args.w4)
            label = f"lin M{M} N{N} K{K}"
        ref = run(1)
        row = dict(shape=label, count=cnt, gops=ops / 1e9, us={})
        for cfg in cfgs:
            try:
                out = run(cfg)
            except RuntimeError as e:           # a tile that does not take this problem (halo: 3x3 only)
                row["us"][cfg] = f"n/a ({str(e)[-40:]})"
                continue
            ok = torch.equal(out, ref)
            us = timeit(lambda: run(cfg))
            row["us"][cfg] = round(us, 2)
            if not ok:
                row["us"][cfg] = f"MISMATCH({us:.1f})"
        auto = timeit(lambda: run(0))
        row["auto_us"] = round(auto, 2)
        best = min((v, k) for k, v in row["us"].items() if not isinstance(v, str))
        row["best"] = f"cfg{best[1]} {best[0]}us {ops / best[0] / 1e6:.0f} TOPS"
        results.append(row)
        print(json.dumps(row), flush=True)
    tot_auto = sum(r["count"] * r["auto_us"] for r in results)
    tot_best = sum(r["count"] * min(v for v in r["us"].values() if not isinstance(v, str))
                   for r in results)
    print(f"weighted total per image: auto {tot_auto / 1e3:.2f} ms, best-per-shape {tot_best / 1e3:.2f} ms")


if __name__ == "__main__":
    main()
